"""What the skeleton stage costs, in ONE process, after a warm-up of every shape, alternating rounds.  Scene lane masks
(get_gray_image of the synthetic scenes) at [16, 256, 256] and [8, 512, 512]:
  (a) dsg_thin_lut_u8: us per launch (the whole batch), HIP events around a burst; the per-image iteration counts;
  (b) dsg_skel_nodes_u8 on the skeletons, the same way;
  (c) what a user does without them: copy the masks to the host and run the NumPy restatement (tests/skeleton_oracle.py: thinning +
      node detection, one image at a time), host clock from the copy's start.  The restatement is vectorised NumPy, far quicker
      than the reference's scikit-image + per-pixel Python loop would be expected to be -- it is the comparison point that is
      available here (scikit-image is not), and it is also checked: its skeletons and node lists equal the kernels';
  (d) the worst case for the barrier loop: one all-ones 512 x 512 image, 257 iterations.
One workgroup per image: a batch of 8 or 16 uses 8 or 16 of the chip's 256 CUs.  Nothing here is a gate.

    timeout -k 10 600 python tools/skeleton_probe.py [--rounds 3] [--launches 200] [--out profiles/skeleton_probe.txt] [--short]

Run it under a time limit, as above; the script starts no further process and stops at its first error.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from drivescenegen_amd import _lib, imageops, synth  # noqa: E402
from oracle.postproc_oracle import get_gray_mask  # noqa: E402
from tests import skeleton_oracle as so  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--out", default=None)
ap.add_argument("--short", action="store_true")
args = ap.parse_args()
if args.short:
    args.launches = 20

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
if not torch.cuda.is_available():
    raise SystemExit("skeleton_probe: no GPU (a timing taken elsewhere says nothing)")
dev = torch.device("cuda", 0)
lib, st = _lib.load(), _lib.stream_ptr(dev)
table = torch.from_numpy(imageops.zhang_suen_lut()).to(dev)


def scene_masks(n, h, w):
    r = synth.synth_scene_rasters(n, 3, h, w, 14555)
    imgs = ((r.transpose(0, 2, 3, 1) * 0.5 + 0.5) * 255).round().astype(np.uint8)
    return np.stack([get_gray_mask(i) for i in imgs])


def burst_us(launch, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


class Case:
    def __init__(self, masks_np):
        self.host = masks_np
        self.n, self.h, self.w = masks_np.shape
        self.mask = torch.from_numpy(masks_np).to(dev)
        self.skel = torch.empty_like(self.mask)
        self.iters = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.cap = imageops.DEFAULT_NODE_CAP
        self.coords = torch.full((self.n, self.cap, 2), -1, dtype=torch.int32, device=dev)
        self.counts = torch.empty(self.n, dtype=torch.int32, device=dev)

    def thin(self):
        _lib.check(lib.dsg_thin_lut_u8(self.mask.data_ptr(), self.n, self.h, self.w, table.data_ptr(), self.h + self.w,
                                       self.skel.data_ptr(), self.iters.data_ptr(), st))

    def nodes(self):
        _lib.check(lib.dsg_skel_nodes_u8(self.skel.data_ptr(), self.n, self.h, self.w, None, self.coords.data_ptr(), self.cap,
                                         self.counts.data_ptr(), st))

    def host_path(self):
        """Device-to-host copy of the masks, then the restatement image by image: (seconds, skeletons, node lists)."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = self.mask.cpu().numpy()
        skels, lists = [], []
        for x in m:
            s, _ = so.thin(x)
            skels.append(s)
            lists.append(so.nodes(s))
        return time.perf_counter() - t0, skels, lists


cases = {"[16, 256, 256] scene masks": Case(scene_masks(16, 256, 256)), "[8, 512, 512] scene masks": Case(scene_masks(8, 512, 512)),
         "[1, 512, 512] all ones": Case(np.full((1, 512, 512), 255, np.uint8))}
for c in cases.values():
    for _ in range(3):
        c.thin()
        c.nodes()
torch.cuda.synchronize()

for name, c in cases.items():
    worst = "all ones" in name
    launches = max(5, args.launches // 20) if worst else args.launches
    on = float((c.host != 0).mean()) * 100
    say(f"{name}: {on:.1f} % of the pixels on; iterations per image {c.iters.cpu().tolist()}; nodes per image {c.counts.cpu().tolist()}; "
        f"{launches} launches per burst")
    t_thin, t_nodes, t_host = [], [], []
    for r in range(args.rounds):
        t_thin.append(burst_us(c.thin, launches))
        t_nodes.append(burst_us(c.nodes, launches))
        line = f"  round {r}: dsg_thin_lut_u8 {t_thin[-1]:.1f} us | dsg_skel_nodes_u8 {t_nodes[-1]:.1f} us"
        if not worst:
            sec, skels, lists = c.host_path()
            t_host.append(sec * 1e6)
            line += f" | host: D2H copy + NumPy restatement {t_host[-1] / 1e3:.1f} ms"
            if r == 0:   # the comparison point computes the same thing
                g_skel, g_coords, g_counts = c.skel.cpu().numpy(), c.coords.cpu().numpy(), c.counts.cpu().numpy()
                same = all(np.array_equal(g_skel[i], skels[i]) and g_counts[i] == len(lists[i])
                           and np.array_equal(g_coords[i, :len(lists[i])], lists[i]) for i in range(c.n))
                line += f" (same skeletons and node lists: {same})"
        say(line)
    both = med(t_thin) + med(t_nodes)
    tail = (f"; host {med(t_host) / 1e3:.1f} ms = {med(t_host) / both:.0f}x the two launches" if t_host else "")
    say(f"  medians: thinning {med(t_thin):.1f} us ({med(t_thin) / c.n:.1f} us per image of the batch), nodes {med(t_nodes):.1f} us{tail}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
