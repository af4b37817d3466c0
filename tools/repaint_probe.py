"""What scene completion costs per U-Net entry next to plain sampling: configs[1] (256 x 256 x 4) at its own batch 16, in ONE
process, after a warm-up of every shape, alternating
  (a) DDIMPipeline, 50 steps                                        -> ms per U-Net entry = time / 50
  (b) RePaintPipeline (50, 5, 3), noise="device"  (140 U-Net entries + 90 undo entries) -> time / 140, undo entries included
three rounds each, host clock around work that ends in a synchronise; then (c) RePaintPipeline with a seeded CPU generator
(a full-batch host draw per entry), recorded without a criterion.

    python tools/repaint_probe.py [--rounds 3] [--short]      (--short: a 10-step schedule, for a kernel trace)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import synth  # noqa: E402
from drivescenegen_amd.configs import CFG2, synth_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--short", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda", 0)
net = synth_weights(d.UNet2DModel(**CFG2)).to(dev).eval().requires_grad_(False)
ddim = d.DDIMPipeline(net, d.DDIMScheduler())
rp = d.RePaintPipeline(net, d.RePaintScheduler())
B = args.batch
orig = torch.from_numpy(synth.synth_scene_rasters(1, 4, 256, 256, 3))
mask = torch.zeros(1, 1, 256, 256)
mask[..., :128] = 1                                   # keep the left half of the tile, outpaint the right
steps, jl, jn = (10, 5, 2) if args.short else (50, 5, 3)
rp.scheduler.set_timesteps(steps, jl, jn)
ts = rp.scheduler.timesteps.tolist()
unet_entries = sum(1 for i, t in enumerate(ts) if i == 0 or t < ts[i - 1])
undo_entries = len(ts) - unet_entries


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_ddim():
    ddim(batch_size=B, num_inference_steps=steps, generator=torch.Generator().manual_seed(1), output_type="np.array")


def run_rp_device():
    rp(orig, mask, num_inference_steps=steps, jump_length=jl, jump_n_sample=jn, batch_size=B, noise="device", seed=1,
       output_type="np.array")


def run_rp_host():
    rp(orig, mask, num_inference_steps=steps, jump_length=jl, jump_n_sample=jn, batch_size=B,
       generator=torch.Generator().manual_seed(1), output_type="np.array")


# warm-up: every shape, every path (plans, workspaces, pinned buffers)
ddim(batch_size=B, num_inference_steps=4, output_type="np.array")
rp(orig, mask, num_inference_steps=6, jump_length=2, jump_n_sample=2, batch_size=B, noise="device", seed=0, output_type="np.array")
rp(orig, mask, num_inference_steps=6, jump_length=2, jump_n_sample=2, batch_size=B, generator=torch.Generator().manual_seed(0),
   output_type="np.array")
torch.cuda.synchronize()

print(f"configs[1] batch {B}, schedule ({steps}, {jl}, {jn}): {len(ts)} entries = {unet_entries} U-Net + {undo_entries} undo")
a, b = [], []
for r in range(args.rounds):
    a.append(timed(run_ddim) / steps * 1e3)
    b.append(timed(run_rp_device) / unet_entries * 1e3)
    print(f"round {r}: (a) DDIM {a[-1]:.3f} ms per U-Net entry | (b) RePaint, device noise {b[-1]:.3f} ms per U-Net entry")
c = timed(run_rp_host) / unet_entries * 1e3
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
spread = (max(a) - min(a)) / med(a)
print(f"(a) median {med(a):.3f} ms, spread (max - min) / median {spread * 100:.2f} %")
print(f"(b) median {med(b):.3f} ms; ratio (b) / (a) of medians {med(b) / med(a):.4f}; of minima {min(b) / min(a):.4f}")
print(f"(c) RePaint, seeded CPU generator (host draw of a full batch per entry): {c:.3f} ms per U-Net entry, {c / med(a):.3f} x (a)")
