"""What sample- / v-prediction and min-SNR weighting cost: configs[1] (256 x 256 x 4) at its own batch 16, in ONE process, after a
warm-up of every shape, alternating rounds of each pair; HIP events around a burst of launches, achieved bytes/s from the streams
each form has to move:
  (1) dsg_ddim_step_pt, v-prediction (x, v in; prev out = 3 streams) next to dsg_ddim_step (the same 3 streams);
  (2) dsg_add_noise_target (x0, z in; noisy, target out = 4 streams, one launch) next to dsg_add_noise followed by a separate
      velocity pass (dsg_add_noise_target with noisy = NULL): 3 + 3 streams, two launches;
  (3) dsg_mse_loss_weighted next to dsg_mse_loss (pred, target in; dpred out = 3 streams, + the finishing launch);
  (4) the configs[2] training step (batch 64 by default, device noise) on a v-prediction scheduler with snr_gamma=5 next to the
      same commit's epsilon step: host clock around steps that end in a synchronise.
Nothing here says anything about image quality: no trained weights exist for this network.

    python tools/predtype_probe.py [--rounds 5] [--train-batch 64] [--out profiles/predtype_probe.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import _lib, synth  # noqa: E402
from drivescenegen_amd.configs import CFG2, CFG3, synth_weights  # noqa: E402
from drivescenegen_amd.train_loop import DeviceNoise, train_step  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--launches", type=int, default=2000)
ap.add_argument("--train-batch", type=int, default=64)
ap.add_argument("--train-steps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
spread = lambda v: (max(v) - min(v)) / med(v) * 100  # noqa: E731
dev = torch.device("cuda", 0)
B = args.batch
def hw(cfg):
    ss = cfg["sample_size"]
    return (ss, ss) if isinstance(ss, int) else tuple(ss)


shape = (B, CFG2["in_channels"], *hw(CFG2))
lib, st = _lib.load(), _lib.stream_ptr(dev)
x, m, z = (torch.randn(shape, device=dev) for _ in range(3))
out_a, out_b = torch.empty_like(x), torch.empty_like(x)
numel, per = x.numel(), x.numel() // B
MB = numel * 4 / 2 ** 20

ddim = d.DDIMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")
ddim.set_timesteps(50)
ds = ddim.step_scalars(499)
step_args = (ds["sqrt_beta_prod_t"], ds["sqrt_alpha_prod_t"], 1.0, ds["sqrt_alpha_prev"], ds["dir_coef"], st)
t = torch.randint(0, 1000, (B,), device=dev)
sa_t, sb_t = ddim._sqrt_tables(dev)
sa, sb = sa_t[t].contiguous(), sb_t[t].contiguous()
w = ddim.snr_weights(5.0, dev)[t].contiguous()
loss = torch.empty(1, device=dev)
ws = torch.empty(2048, dtype=torch.float64, device=dev)


def ddim_eps():
    _lib.check(lib.dsg_ddim_step(x.data_ptr(), m.data_ptr(), out_a.data_ptr(), numel, *step_args))


def ddim_v():
    _lib.check(lib.dsg_ddim_step_pt(x.data_ptr(), m.data_ptr(), out_a.data_ptr(), numel, _lib.DSG_PRED_V, *step_args))


def target_fused():
    _lib.check(lib.dsg_add_noise_target(x.data_ptr(), z.data_ptr(), sa.data_ptr(), sb.data_ptr(), out_a.data_ptr(), out_b.data_ptr(),
                                        B, per, st))


def target_two_launches():
    _lib.check(lib.dsg_add_noise(x.data_ptr(), z.data_ptr(), sa.data_ptr(), sb.data_ptr(), out_a.data_ptr(), B, per, st))
    _lib.check(lib.dsg_add_noise_target(x.data_ptr(), z.data_ptr(), sa.data_ptr(), sb.data_ptr(), None, out_b.data_ptr(), B, per, st))


def loss_plain():
    _lib.check(lib.dsg_mse_loss(x.data_ptr(), m.data_ptr(), numel, 1.0, loss.data_ptr(), out_a.data_ptr(), ws.data_ptr(),
                                ws.numel() * 8, st))


def loss_weighted():
    _lib.check(lib.dsg_mse_loss_weighted(x.data_ptr(), m.data_ptr(), w.data_ptr(), B, per, 1.0, loss.data_ptr(), out_a.data_ptr(),
                                         ws.data_ptr(), ws.numel() * 8, st))


def burst_us(launch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.launches):
        launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / args.launches


def pair(title, old, old_streams, new, new_streams, expectation):
    name_old, f_old = old
    name_new, f_new = new
    for f in (f_old, f_new):
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    say(title)
    u_old, u_new = [], []
    for r in range(args.rounds):
        u_old.append(burst_us(f_old))
        u_new.append(burst_us(f_new))
        say(f"round {r}: {name_old} {u_old[-1]:.1f} us = {old_streams * numel * 4 / u_old[-1] * 1e-6:.3f} TB/s ({old_streams} streams) | "
            f"{name_new} {u_new[-1]:.1f} us = {new_streams * numel * 4 / u_new[-1] * 1e-6:.3f} TB/s ({new_streams} streams)")
    say(f"time, {name_new} / {name_old}: of medians {med(u_new) / med(u_old):.3f}, of minima {min(u_new) / min(u_old):.3f}; "
        f"repeat-to-repeat spread (max - min) / median: {name_old} {spread(u_old):.2f} %, {name_new} {spread(u_new):.2f} %  "
        f"(expectation: {expectation})")


say(f"batch {B} of configs[1]: {numel} floats ({MB:.1f} MiB per stream), {args.launches} launches per burst, {args.rounds} rounds")
pair("(1) DDIM step", ("dsg_ddim_step", ddim_eps), 3, ("dsg_ddim_step_pt v", ddim_v), 3,
     "the same three streams: no slower than the epsilon step's own spread")
pair("(2) x_t and the velocity target", ("dsg_add_noise + velocity pass", target_two_launches), 6,
     ("dsg_add_noise_target", target_fused), 4, "the fused pass moves 4 streams where two launches move 6: ratio < 1")
pair("(3) MSE loss and its gradient", ("dsg_mse_loss", loss_plain), 3, ("dsg_mse_loss_weighted", loss_weighted), 3,
     "the same three streams + one weight per sample")

# ---- (4) the training step ----------------------------------------------------------------------------------------------------
TB = args.train_batch


def trainer(sched):
    torch.manual_seed(7)
    acc = d.Accelerator(mixed_precision="no")
    net = synth_weights(d.UNet2DModel(**CFG3)).to(dev)
    opt = d.AdamW(net.parameters(), lr=1e-4)
    lrs = d.get_cosine_schedule_with_warmup(optimizer=opt, num_warmup_steps=2, num_training_steps=1000)
    net, opt, lrs = acc.prepare(net, opt, lrs)
    return dict(acc=acc, net=net, opt=opt, lrs=lrs, sch=sched, noise=DeviceNoise(seed=3))


def steps_ms(tr, gamma):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.train_steps):
        train_step(tr["acc"], tr["net"], tr["sch"], tr["opt"], tr["lrs"], batch, noise=tr["noise"], snr_gamma=gamma)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.train_steps * 1e3


batch = torch.from_numpy(synth.synth_scene_rasters(TB, CFG3["in_channels"], *hw(CFG3), 5)).to(dev)
eps_tr = trainer(d.DDPMScheduler())
v_tr = trainer(d.DDPMScheduler(prediction_type="v_prediction"))
for tr, gamma in ((eps_tr, None), (v_tr, 5.0)):
    for _ in range(3):
        steps_ms(tr, gamma)
say(f"(4) configs[2] training step, fp32-equivalent, batch {TB}, device noise, {args.train_steps} steps per window")
a, b = [], []
for r in range(args.rounds):
    a.append(steps_ms(eps_tr, None))
    b.append(steps_ms(v_tr, 5.0))
    say(f"round {r}: epsilon, unweighted {a[-1]:.2f} ms per step | v_prediction, snr_gamma=5 {b[-1]:.2f} ms per step")
say(f"ms per step, v + min-SNR / epsilon: of medians {med(b) / med(a):.4f}, of minima {min(b) / min(a):.4f}; spread (max - min) / "
    f"median: epsilon {spread(a):.2f} %, v {spread(b):.2f} %  (the target and the weights are two more streams of the batch "
    "beside a whole U-Net step)")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
