"""What the averaged weights cost per training step, in ONE process, after a warm-up, alternating rounds of each pair:
  (1) dsg_ema_step (param, shadow in; shadow out = 3 streams) next to dsg_adamw_step (param, grad, m, v in; param, m, v out = 7
      streams) on the default network's 56.6 M parameters, one job / one slab each: us per launch and achieved bytes/s, HIP
      events around a burst of launches, and the EMA launch as a fraction of the AdamW launch;
  (2) the configs[2] training step (default 4-channel network, fp32-equivalent tape, device noise) through `train_step` with
      and without `ema=`: ms per step, host clock around steps that end in a synchronise, and their ratio on this box.

    python tools/ema_probe.py [--rounds 3] [--batch 64] [--steps 5] [--out profiles/ema_probe.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import ops  # noqa: E402
from drivescenegen_amd.configs import CFG3, PARAM_COUNTS, synth_weights  # noqa: E402
from drivescenegen_amd.train_loop import DeviceNoise, train_step  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
dev = torch.device("cuda", 0)

# ---- (1) the two slab kernels -----------------------------------------------------------------------------------------------
numel = PARAM_COUNTS["CFG2"]
p, g, m, v, s = (torch.randn(numel, device=dev) * 0.02 for _ in range(5))
v.abs_()
table = ops.EmaTable([(p.data_ptr(), s.data_ptr(), numel, False)], dev)


def launch_ema():
    table.run(1e-4)


def launch_adamw():
    ops.adamw_step_(p, g, m, v, 10, 1e-4)


def burst_us(launch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.launches):
        launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / args.launches


for f in (launch_ema, launch_adamw):
    for _ in range(10):
        f()
torch.cuda.synchronize()
say(f"(1) slab kernels on {numel} floats ({numel * 4 / 2 ** 20:.1f} MiB per stream), {args.launches} launches per burst")
u_e, u_a = [], []
for r in range(args.rounds):
    u_a.append(burst_us(launch_adamw))
    u_e.append(burst_us(launch_ema))
    say(f"round {r}: dsg_adamw_step {u_a[-1]:.1f} us = {7 * numel * 4 / u_a[-1] * 1e-6:.3f} TB/s (7 streams) | dsg_ema_step "
        f"{u_e[-1]:.1f} us = {3 * numel * 4 / u_e[-1] * 1e-6:.3f} TB/s (3 streams)")
say(f"dsg_ema_step / dsg_adamw_step, time per launch: of medians {med(u_e) / med(u_a):.3f}, of minima {min(u_e) / min(u_a):.3f}  "
    f"(3 streams against 7: 0.429 at equal bytes/s)")
del p, g, m, v, s, table

# ---- (2) the training step ----------------------------------------------------------------------------------------------------
B = args.batch
acc = d.Accelerator(mixed_precision="no")
net = synth_weights(d.UNet2DModel(**CFG3)).to(dev)
opt = d.AdamW(net.parameters(), lr=1e-4)
lrs = d.get_cosine_schedule_with_warmup(optimizer=opt, num_warmup_steps=2, num_training_steps=10000)
net, opt, lrs = acc.prepare(net, opt, lrs)
sch = d.DDPMScheduler()
ema = d.EMAModel(net.parameters())
noise = DeviceNoise(seed=1)
ss = CFG3["sample_size"]
h, w = (ss, ss) if isinstance(ss, int) else ss
batch = torch.rand((B, CFG3["in_channels"], h, w), device=dev) * 2 - 1


def steps_ms(e):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        train_step(acc, net, sch, opt, lrs, batch, noise=noise, ema=e)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


for e in (None, ema, None, ema):   # warm-up: the tape, AdamW's slab, the EMA table before and after the parameters move
    train_step(acc, net, sch, opt, lrs, batch, noise=noise, ema=e)
torch.cuda.synchronize()
say(f"(2) configs[2] training step, fp32-equivalent tape, batch {B}, device noise, {args.steps} steps per round; the EMA table has "
    f"{ema._table.n} job(s)")
a, b = [], []
for r in range(args.rounds):
    a.append(steps_ms(None))
    b.append(steps_ms(ema))
    say(f"round {r}: without ema {a[-1]:.2f} ms per step | with ema {b[-1]:.2f} ms per step")
say(f"ms per step, with ema / without: of medians {med(b) / med(a):.4f}, of minima {min(b) / min(a):.4f}; spread without ema "
    f"(max - min) / median {(max(a) - min(a)) / med(a) * 100:.2f} %")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
