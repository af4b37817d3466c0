"""What dynamic thresholding costs per denoising step: configs[1] (256 x 256 x 4) at its own batch 16, in ONE process, after a
warm-up of every shape, alternating rounds:
  (a) dsg_dynthresh_scale + dsg_ddim_step_thr (1 zero-fill + 3 histogram + 3 scan launches, then the step) next to dsg_ddim_step
      on the batch's 4.19 M floats: us per step, HIP events around a burst;
  (b) the same thresholded step written in torch on the GPU (torch.quantile + clamp + divide + the DDIM expression): what a user
      would otherwise write, and the figure (a) is compared against;
  (c) (a) again on an all-equal tensor (every element in one bin in every pass: the worst case for the histogram atomics);
  (d) DDIMPipeline ms per step with and without thresholding, host clock around work that ends in a synchronise.
Nothing here is a gate.

    python tools/dynthresh_probe.py [--rounds 3] [--out profiles/dynthresh_probe.txt] [--short]   (--short: fewer launches / steps)
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
ap.add_argument("--launches", type=int, default=500)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default=None)
ap.add_argument("--short", action="store_true")
args = ap.parse_args()
if args.short:
    args.launches, args.steps = 50, 8

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
if not torch.cuda.is_available():
    raise SystemExit("dynthresh_probe: no GPU (a timing taken elsewhere says nothing)")
dev = torch.device("cuda", 0)
B = args.batch
shape = (B, CFG2["in_channels"], CFG2["sample_size"], CFG2["sample_size"])
lib, st = _lib.load(), _lib.stream_ptr(dev)

sch = d.DDIMScheduler(thresholding=True, sample_max_value=1.5)
sch.set_timesteps(50)
sc = sch.step_scalars(500)
Q, MX = sch.config.dynamic_thresholding_ratio, sch.config.sample_max_value
x, e = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
x_eq, e_eq = torch.full(shape, 0.5, device=dev), torch.full(shape, 0.25, device=dev)
prev = torch.empty_like(x)
numel, per = x.numel(), x.numel() // B
k_lo, k_hi, w = sch.threshold_ranks(per)
nbytes = ctypes.c_size_t()
_lib.check(lib.dsg_dynthresh_workspace_bytes(B, ctypes.byref(nbytes)))
ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
scale = torch.empty(B, dtype=torch.float32, device=dev)


def launch_thr(xs=x, es=e):
    _lib.check(lib.dsg_dynthresh_scale(xs.data_ptr(), es.data_ptr(), scale.data_ptr(), B, per, sc["sqrt_beta_prod_t"],
                                       sc["sqrt_alpha_prod_t"], k_lo, k_hi, w, MX, ws.data_ptr(), nbytes.value, st))
    _lib.check(lib.dsg_ddim_step_thr(xs.data_ptr(), es.data_ptr(), scale.data_ptr(), prev.data_ptr(), numel, per,
                                     sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], sc["sqrt_alpha_prev"], sc["dir_coef"], st))


def launch_thr_equal():
    launch_thr(x_eq, e_eq)


def launch_ddim():
    _lib.check(lib.dsg_ddim_step(x.data_ptr(), e.data_ptr(), prev.data_ptr(), numel, sc["sqrt_beta_prod_t"],
                                 sc["sqrt_alpha_prod_t"], 1.0, sc["sqrt_alpha_prev"], sc["dir_coef"], st))


def launch_torch():
    p0 = (x - sc["sqrt_beta_prod_t"] * e) / sc["sqrt_alpha_prod_t"]
    s = torch.quantile(p0.abs().reshape(B, -1), Q, dim=1).clamp(min=1, max=MX).view(B, 1, 1, 1)
    p0 = torch.clamp(p0, -s, s) / s
    return sc["sqrt_alpha_prev"] * p0 + sc["dir_coef"] * e


def burst_us(launch, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


for f in (launch_thr, launch_thr_equal, launch_ddim, launch_torch):
    for _ in range(5):
        f()
torch.cuda.synchronize()
# the two ways agree on the data they are timed on (torch's p0 is the same three fp32 operations)
launch_thr()
s_ours = scale.clone()
s_torch = torch.quantile(((x - sc["sqrt_beta_prod_t"] * e) / sc["sqrt_alpha_prod_t"]).abs().reshape(B, -1), Q, dim=1).clamp(min=1, max=MX)
say(f"scale of the timed batch: ours == torch.quantile's on {int((s_ours == s_torch).sum())} of {B} samples "
    f"(max |d| {float((s_ours - s_torch).abs().max()):.3e})")
say(f"(a)-(c) one DDIM step on {numel} floats ({numel * 4 / 2 ** 20:.1f} MiB per stream), batch {B}, q {Q}, max {MX}; "
    f"{args.launches} steps per burst ({max(10, args.launches // 10)} for torch)")
u = dict(ddim=[], thr=[], eq=[], torch=[])
for r in range(args.rounds):
    u["ddim"].append(burst_us(launch_ddim, args.launches))
    u["thr"].append(burst_us(launch_thr, args.launches))
    u["eq"].append(burst_us(launch_thr_equal, args.launches))
    u["torch"].append(burst_us(launch_torch, max(10, args.launches // 10)))
    say(f"round {r}: dsg_ddim_step {u['ddim'][-1]:.1f} us | (a) dsg_dynthresh_scale + dsg_ddim_step_thr {u['thr'][-1]:.1f} us | "
        f"(c) the same, all-equal tensor {u['eq'][-1]:.1f} us | (b) torch.quantile form {u['torch'][-1]:.1f} us")
say(f"medians: ddim {med(u['ddim']):.1f} us, thresholded {med(u['thr']):.1f} us (+{med(u['thr']) - med(u['ddim']):.1f} us per step), "
    f"all-equal {med(u['eq']):.1f} us, torch {med(u['torch']):.1f} us; torch / ours {med(u['torch']) / med(u['thr']):.1f}x")

# ---- (d) the pipeline ---------------------------------------------------------------------------------------------------------
net = synth_weights(d.UNet2DModel(**CFG2)).to(dev).eval().requires_grad_(False)
p_clip = d.DDIMPipeline(net, d.DDIMScheduler())
p_thr = d.DDIMPipeline(net, d.DDIMScheduler.from_config(p_clip.scheduler.config, thresholding=True, sample_max_value=1.5))


def timed(pipe, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe(batch_size=B, num_inference_steps=steps, generator=torch.Generator().manual_seed(1), output_type="np.array")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


timed(p_clip, 4)
timed(p_thr, 4)
say(f"(d) configs[1] batch {B}, DDIMPipeline, {args.steps} steps: ms per step (whole call / steps)")
a, b = [], []
for r in range(args.rounds):
    a.append(timed(p_clip, args.steps))
    b.append(timed(p_thr, args.steps))
    say(f"round {r}: clip_sample {a[-1]:.3f} ms | thresholding {b[-1]:.3f} ms")
say(f"ms per step, thresholding / clip_sample: of medians {med(b) / med(a):.4f}, of minima {min(b) / min(a):.4f}  "
    f"(expectation, not a gate: < 1.01); clip_sample spread (max - min) / median {(max(a) - min(a)) / med(a) * 100:.2f} %")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
