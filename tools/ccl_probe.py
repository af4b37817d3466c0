"""What the connected-component stage costs, in ONE process, after a warm-up of every case, alternating rounds.
  (a) imageops.dense_skeleton_nodes_batch on the skeletons of scene lane masks (erode 2 x 2, label with 4 neighbours, statistics,
      centres: a zero fill and ten launches) and imageops.agent_blobs_batch on the scene images (mask, label with 8 neighbours,
      statistics, centres), at [16, 256, 256] and [8, 512, 512]: us per call of the WRAPPER (allocations and Python included),
      HIP events around a burst of calls;
  (b) the same two calls on worst cases for the labelling: one all-ones image (one component through every tile; the
      most LDS passes per tile) and one image of noise at density 0.59 (the percolation threshold of 4 neighbours: large ragged
      components, the longest union-find walks), [1, 512, 512], labelled through imageops.label_batch + component_stats_batch;
  (c) what a user does without them: copy the batch to the host and call scipy.ndimage, the library the reference itself calls
      (binary_erosion + label + center_of_mass; for the agents label + find_objects + the five sums), one image at a time,
      host clock from the copy's start.  Its results are compared with the GPU's once.
Medians of the rounds.  Nothing here is a gate.

    timeout -k 10 600 python tools/ccl_probe.py [--rounds 3] [--calls 100] [--out profiles/ccl_probe.txt] [--short]

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
from scipy import ndimage  # noqa: E402
from drivescenegen_amd import imageops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--out", default=None)
ap.add_argument("--short", action="store_true")
args = ap.parse_args()
if args.short:
    args.calls = 10

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
if not torch.cuda.is_available():
    raise SystemExit("ccl_probe: no GPU (a timing taken elsewhere says nothing)")
dev = torch.device("cuda", 0)
EIGHT = np.ones((3, 3), int)


def scene_images(n, h, w):
    r = synth.synth_scene_rasters(n, 3, h, w, 14555)
    return torch.from_numpy(((r.transpose(0, 2, 3, 1) * 0.5 + 0.5) * 255).round().astype(np.uint8)).to(dev)


def burst_us(call, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def host_dense(skel):
    """find_dense_skeleton_nodes per image, from the device tensor: (seconds, lists)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = []
    for s in skel.cpu().numpy():
        eroded = ndimage.binary_erosion(np.pad(s, 1), np.ones((2, 2)))[1:-1, 1:-1]
        lab, k = ndimage.label(eroded)
        out.append([(int(x), int(y)) for x, y in ndimage.center_of_mass(eroded, lab, [*range(1, k + 1)])])
    return time.perf_counter() - t0, out


def host_blobs(mask, structure=EIGHT):
    """label + bounding boxes + area and the five sums per image: (seconds, [(labels, k, areas)])."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = []
    for m in mask.cpu().numpy():
        lab, k = ndimage.label(m, structure)
        idx = np.arange(1, k + 1)
        ndimage.find_objects(lab)
        rr, cc = np.mgrid[0:m.shape[0], 0:m.shape[1]]
        area = ndimage.sum(np.ones_like(lab), lab, idx)
        for v in (rr, cc, rr * rr, cc * cc, rr * cc):
            ndimage.sum(v, lab, idx)
        out.append((lab, k, np.asarray(area).astype(np.int64)))
    return time.perf_counter() - t0, out


def same_dense(coords, counts, lists):
    coords, counts = coords.cpu().numpy(), counts.cpu().numpy()
    return all(counts[i] == len(want) and coords[i, :len(want)].tolist() == [list(p) for p in want] for i, want in enumerate(lists))


def same_blobs(labels, counts, stats, host):
    labels, counts, area = labels.cpu().numpy(), counts.cpu().numpy(), stats["area"].cpu().numpy()
    return all(counts[i] == k and np.array_equal(labels[i], lab) and np.array_equal(area[i, :min(k, area.shape[1])], a[:area.shape[1]])
               for i, (lab, k, a) in enumerate(host))


cases = []
for n, h, w in ((16, 256, 256), (8, 512, 512)):
    imgs = scene_images(n, h, w)
    skel = imageops.lane_skeleton_batch(imgs)[1]
    agent = imageops.agent_mask_batch(imgs)
    cases.append((f"[{n}, {h}, {w}] scene skeletons: dense_skeleton_nodes_batch", lambda skel=skel: imageops.dense_skeleton_nodes_batch(skel),
                  lambda skel=skel: host_dense(skel), same_dense, skel))
    cases.append((f"[{n}, {h}, {w}] scene images: agent_blobs_batch", lambda imgs=imgs: imageops.agent_blobs_batch(imgs),
                  lambda agent=agent: host_blobs(agent), lambda l, c, s, host: same_blobs(l, c, s, host), agent))
rng = np.random.default_rng(3)
worst = {"all ones": np.full((1, 512, 512), 255, np.uint8), "noise 0.59": ((rng.random((1, 512, 512)) < 0.59) * 255).astype(np.uint8)}
for name, a in worst.items():
    m = torch.from_numpy(a).to(dev)

    def gpu(m=m):
        labels, counts = imageops.label_batch(m, 1)
        return labels, counts, imageops.component_stats_batch(labels, counts, cap=65536)

    cases.append((f"[1, 512, 512] {name}: label_batch (4 neighbours) + component_stats_batch", gpu,
                  lambda m=m: host_blobs(m, None), lambda l, c, s, host: same_blobs(l, c, s, host), m))

for _, gpu, _, _, _ in cases:
    for _ in range(3):
        gpu()
torch.cuda.synchronize()

for name, gpu, host, same, data in cases:
    out = gpu()
    counts = out[1]
    say(f"{name}: {float((data != 0).float().mean()) * 100:.1f} % of the pixels on; components per image {counts.cpu().tolist()}; "
        f"{args.calls} calls per burst")
    t_gpu, t_host = [], []
    for r in range(args.rounds):
        t_gpu.append(burst_us(gpu, args.calls))
        sec, res = host()
        t_host.append(sec * 1e6)
        line = f"  round {r}: GPU {t_gpu[-1]:.1f} us per call | host: D2H copy + scipy.ndimage {t_host[-1] / 1e3:.2f} ms"
        if r == 0:
            line += f" (same result: {same(*out, res)})"
        say(line)
    say(f"  medians: GPU {med(t_gpu):.1f} us, host {med(t_host) / 1e3:.2f} ms = {med(t_host) / med(t_gpu):.1f}x")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
