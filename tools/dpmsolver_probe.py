"""What the DPM-Solver++ step costs and what the shorter schedule buys: configs[1] (256 x 256 x 4) at its own batch 16, in ONE
process, after a warm-up of every shape, three alternating rounds of each pair:
  (1) the fused order-2 step kernel (dsg_dpmsolver_step: x, eps, m1 in; prev, m0 out = 5 streams) next to dsg_ddim_step
      (x, eps in; prev out = 3 streams) on the batch's 4.19 M floats: achieved bytes/s of each, HIP events around a burst of launches;
  (2) DDIMPipeline with DDIMScheduler, 50 steps, next to DDIMPipeline with DPMSolverMultistepScheduler (order 2, midpoint),
      20 steps: ms per U-Net entry (time / steps) and whole-call images/s, host clock around work that ends in a synchronise.
The images/s ratio is a statement about STEP COUNT, not about image quality: nobody has measured quality on trained weights here.

    python tools/dpmsolver_probe.py [--rounds 3] [--out profiles/dpmsolver_probe.txt] [--short]   (--short: 4 / 10 steps, for a kernel trace)
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import _lib  # noqa: E402
from drivescenegen_amd.configs import CFG2, synth_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--launches", type=int, default=2000)
ap.add_argument("--out", default=None)
ap.add_argument("--short", action="store_true")
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
dev = torch.device("cuda", 0)
B = args.batch
shape = (B, CFG2["in_channels"], CFG2["sample_size"], CFG2["sample_size"])
lib, st = _lib.load(), _lib.stream_ptr(dev)

# ---- (1) the step kernels ---------------------------------------------------------------------------------------------------
x, e, m1 = (torch.randn(shape, device=dev) for _ in range(3))
prev, m0 = torch.empty_like(x), torch.empty_like(x)
numel = x.numel()
sch = d.DPMSolverMultistepScheduler()
sch.set_timesteps(20)
ts = sch.timesteps.tolist()
s = sch.step_scalars(ts[10], ts[11], ts[9], None, 2)
dpm_args = _lib.DpmSolverStepArgs(sample=x.data_ptr(), eps=e.data_ptr(), m1=m1.data_ptr(), m2=None, noise=None,
                                  prev=prev.data_ptr(), m0_out=m0.data_ptr(), noise_out=None, numel=numel, order=2, add_noise=0,
                                  seed=0, offset=0, **s)
ddim = d.DDIMScheduler()
ddim.set_timesteps(50)
ds = ddim.step_scalars(500)


def launch_dpm():
    _lib.check(lib.dsg_dpmsolver_step(ctypes.byref(dpm_args), st))


def launch_ddim():
    _lib.check(lib.dsg_ddim_step(x.data_ptr(), e.data_ptr(), prev.data_ptr(), numel, ds["sqrt_beta_prod_t"],
                                 ds["sqrt_alpha_prod_t"], 1.0, ds["sqrt_alpha_prev"], ds["dir_coef"], st))


def burst_us(launch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.launches):
        launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / args.launches


for f in (launch_dpm, launch_ddim):
    for _ in range(20):
        f()
torch.cuda.synchronize()
say(f"(1) step kernels on {numel} floats ({numel * 4 / 2 ** 20:.1f} MiB per stream), {args.launches} launches per burst")
bw_dpm, bw_ddim = [], []
for r in range(args.rounds):
    u_ddim, u_dpm = burst_us(launch_ddim), burst_us(launch_dpm)
    bw_ddim.append(3 * numel * 4 / u_ddim * 1e-6)
    bw_dpm.append(5 * numel * 4 / u_dpm * 1e-6)
    say(f"round {r}: dsg_ddim_step {u_ddim:.1f} us = {bw_ddim[-1]:.3f} TB/s (3 streams) | dsg_dpmsolver_step order 2 "
        f"{u_dpm:.1f} us = {bw_dpm[-1]:.3f} TB/s (5 streams)")
say(f"achieved bytes/s, fused order-2 step / ddim step: of medians {med(bw_dpm) / med(bw_ddim):.3f}, of best "
    f"{max(bw_dpm) / max(bw_ddim):.3f}  (expectation: >= 0.85)")

# ---- (2) the pipelines --------------------------------------------------------------------------------------------------------
net = synth_weights(d.UNet2DModel(**CFG2)).to(dev).eval().requires_grad_(False)
p_ddim = d.DDIMPipeline(net, d.DDIMScheduler())
p_dpm = d.DDIMPipeline(net, d.DDIMScheduler())
p_dpm.scheduler = d.DPMSolverMultistepScheduler.from_config(p_dpm.scheduler.config)
n_ddim, n_dpm = (10, 4) if args.short else (50, 20)


def timed(pipe, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe(batch_size=B, num_inference_steps=steps, generator=torch.Generator().manual_seed(1), output_type="np.array")
    torch.cuda.synchronize()
    return time.perf_counter() - t0


timed(p_ddim, 4)
timed(p_dpm, 4)
say(f"(2) configs[1] batch {B}: DDIMPipeline + DDIMScheduler {n_ddim} steps | DDIMPipeline + DPMSolverMultistepScheduler "
    f"(order 2, midpoint, {p_dpm.scheduler.config.timestep_spacing}) {n_dpm} steps")
a, b, ia, ib = [], [], [], []
for r in range(args.rounds):
    ta, tb = timed(p_ddim, n_ddim), timed(p_dpm, n_dpm)
    a.append(ta / n_ddim * 1e3)
    b.append(tb / n_dpm * 1e3)
    ia.append(B / ta)
    ib.append(B / tb)
    say(f"round {r}: DDIM {a[-1]:.3f} ms per U-Net entry, {ia[-1]:.2f} images/s | DPM-Solver++ {b[-1]:.3f} ms per U-Net entry, "
        f"{ib[-1]:.2f} images/s")
say(f"ms per U-Net entry, DPM-Solver++ / DDIM: of medians {med(b) / med(a):.4f}, of minima {min(b) / min(a):.4f}  "
    f"(expectation: <= 1.02); DDIM spread (max - min) / median {(max(a) - min(a)) / med(a) * 100:.2f} %")
say(f"whole-call images/s: DDIM {n_ddim} steps {med(ia):.2f}, DPM-Solver++ {n_dpm} steps {med(ib):.2f}, ratio "
    f"{med(ib) / med(ia):.3f}  (step count, not image quality: quality on trained weights has not been measured)")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
