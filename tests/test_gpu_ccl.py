"""Connected components on the GPU: ``dsg_ccl_u8``, ``dsg_cc_stats_i32``, ``dsg_cc_centers_i32``, ``dsg_merge_nodes_i32``
(csrc/ccl.hip) and their wrappers in drivescenegen_amd/imageops.py against tests/ccl_oracle.py, BITWISE -- labels, counts,
statistics, centres, merged lists and their order; nothing here has a tolerance.  (tests/test_ccl_cpu.py pins that oracle to
scipy.ndimage.)

The kernel tests go through the C ABI on buffers between sentinel margins (the ``Guarded`` idiom of
tests/test_gpu_skeleton.py).  The mask's margins are NON-ZERO bytes, so a read outside the image would show as a wrong label;
every input and every row an output list does not reach must come back untouched; the workspace sits between margins too.
Shapes at the tile borders are derived from the kernel's own tile (``imageops.ccl_tile_shape``)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drivescenegen_amd import _lib, imageops, synth  # noqa: E402
from oracle.postproc_oracle import get_gray_mask  # noqa: E402
from tests import ccl_oracle as co  # noqa: E402
from tests import skeleton_oracle as so  # noqa: E402

DEV = "cuda"
MARGIN = 4096            # bytes (uint8 buffers) / elements (int32 buffers)
SENT8, SENT32 = 0xA5, -777
SMALL = [(1, 1), (1, 40), (37, 1), (2, 2), (5, 31), (5, 32), (5, 33), (9, 64), (37, 53), (96, 70)]
MODES = [(1, 0), (1, 1), (2, 0), (2, 1)]      # (connectivity, erode2x2)


# ---- guarded buffers ----------------------------------------------------------------------------------------------------------
class Guarded:
    def __init__(self, shape, dtype, off=0, fill=None):
        self.sent = SENT8 if dtype == torch.uint8 else SENT32
        self.numel, self.off = int(np.prod(shape)), off
        self.whole = torch.full((self.numel + 2 * MARGIN + off,), self.sent, dtype=dtype, device=DEV)
        self.view = self.whole[MARGIN + off:MARGIN + off + self.numel].view(shape)
        if dtype == torch.uint8:
            assert self.view.data_ptr() % 16 == off % 16
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.array(fill)).to(DEV))      # (a copy: the shared cases are read-only arrays)

    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        """The interior as a NumPy array, after checking both margins."""
        w = self.whole.cpu().numpy()
        a, b = MARGIN + self.off, MARGIN + self.off + self.numel
        assert (w[:a] == w.dtype.type(self.sent)).all() and (w[b:] == w.dtype.type(self.sent)).all(), "a margin was written"
        return w[a:b].reshape(tuple(self.view.shape)).copy()


def workspace_bytes(n, h, w):
    need = ctypes.c_size_t()
    _lib.check(_lib.load().dsg_ccl_workspace_bytes(n, h, w, ctypes.byref(need)))
    return need.value


def ccl_abi(imgs, connectivity, erode, off=0, stream=None):
    """dsg_ccl_u8 on guarded buffers -> (labels, counts); margins, the workspace's margins and the input are checked."""
    n, h, w = imgs.shape
    need = workspace_bytes(n, h, w)
    src, ws = Guarded((n, h, w), torch.uint8, off, imgs), Guarded((need,), torch.uint8)
    lab, cnt = Guarded((n, h, w), torch.int32), Guarded((n,), torch.int32)
    st = _lib.stream_ptr(torch.device(DEV)) if stream is None else stream.cuda_stream
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    _lib.check(_lib.load().dsg_ccl_u8(src.ptr(), n, h, w, connectivity, erode, lab.ptr(), cnt.ptr(), ws.ptr(), need, st))
    torch.cuda.synchronize()
    assert np.array_equal(src.get(), imgs)
    ws.get()
    return lab.get(), cnt.get()


def stats_abi(labels, counts, cap):
    """dsg_cc_stats_i32 + dsg_cc_centers_i32 -> (records as int32 [n, cap, 16], centres [n, cap, 2]); SENT32 where nothing was written."""
    n, h, w = labels.shape
    lab, cnt = Guarded((n, h, w), torch.int32, 0, labels), Guarded((n,), torch.int32, 0, counts)
    rec, cen = Guarded((n, max(cap, 1), 16), torch.int32), Guarded((n, max(cap, 1), 2), torch.int32)
    assert rec.ptr() % 8 == 0
    lib, st = _lib.load(), _lib.stream_ptr(torch.device(DEV))
    _lib.check(lib.dsg_cc_stats_i32(lab.ptr(), n, h, w, cnt.ptr(), rec.ptr() if cap else None, cap, st))
    _lib.check(lib.dsg_cc_centers_i32(rec.ptr() if cap else None, cnt.ptr(), n, cap, cen.ptr() if cap else None, st))
    torch.cuda.synchronize()
    assert np.array_equal(lab.get(), labels) and np.array_equal(cnt.get(), counts)
    return rec.get()[:, :cap], cen.get()[:, :cap]


def merge_abi(nodes, counts, cap, dense, dense_counts, dense_cap, min_d2=25):
    """dsg_merge_nodes_i32 -> (nodes [n, cap, 2], out_counts).  `nodes` / `dense`: lists of [k, 2] arrays, cut to the caps; rows
    behind a list are SENT32."""
    n = len(nodes)
    a, d = Guarded((n, max(cap, 1), 2), torch.int32), Guarded((n, max(dense_cap, 1), 2), torch.int32)
    for i in range(n):
        a.view[i, :min(len(nodes[i]), cap)] = torch.from_numpy(np.asarray(nodes[i][:cap], np.int32).reshape(-1, 2)).to(DEV)
        d.view[i, :min(len(dense[i]), dense_cap)] = torch.from_numpy(np.asarray(dense[i][:dense_cap], np.int32).reshape(-1, 2)).to(DEV)
    ca, cd = Guarded((n,), torch.int32, 0, np.asarray(counts, np.int32)), Guarded((n,), torch.int32, 0, np.asarray(dense_counts, np.int32))
    out = Guarded((n,), torch.int32)
    dense_before = d.get()
    _lib.check(_lib.load().dsg_merge_nodes_i32(a.ptr() if cap else None, ca.ptr(), n, cap, d.ptr() if dense_cap else None, cd.ptr(),
                                              dense_cap, min_d2, out.ptr(), _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert np.array_equal(d.get(), dense_before) and np.array_equal(ca.get(), counts) and np.array_equal(cd.get(), dense_counts)
    return a.get()[:, :cap], out.get()


# ---- contents -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tile():
    return imageops.ccl_tile_shape()


def scene_images(n, h, w, seed=14555):
    r = synth.synth_scene_rasters(n, 3, h, w, seed)
    return ((r.transpose(0, 2, 3, 1) * 0.5 + 0.5) * 255).round().astype(np.uint8)


def noise(h, w, density, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    return ((rng.random((h, w)) < density) * rng.integers(1, 256, (h, w))).astype(np.uint8)   # any non-zero byte is "on"


def corners(h, w):
    a = np.zeros((h, w), np.uint8)
    a[0, 0] = a[0, -1] = a[-1, 0] = a[-1, -1] = 3
    return a


def checkerboard(h, w):
    return (np.indices((h, w)).sum(0) % 2 == 0).astype(np.uint8)


def bars_along(h, w):
    """One-pixel bars ALONG the tile borders: the last row / column of every tile and, a tile further, the first ones."""
    th, tw = tile()
    a = np.zeros((h, w), np.uint8)
    for k, y in enumerate(range(th, h + th, th)):
        a[min(h - 1, y - 1 if k % 2 == 0 else y - th)] = 1
    for k, x in enumerate(range(tw, w + tw, tw)):
        a[::2, min(w - 1, x - 1 if k % 2 == 0 else x - tw)] = 1
    return a


def bars_across(h, w):
    """Short one-pixel bars ACROSS every tile border, every third row / column, not touching each other."""
    th, tw = tile()
    a = np.zeros((h, w), np.uint8)
    for x in range(tw, w, tw):
        a[0::3, max(0, x - 2):x + 2] = 1
    for y in range(th, h, th):
        for x in range(tw // 2, w, 3):
            if x % tw >= 4 and x % tw < tw - 4:
                a[max(0, y - 2):y + 2, x] = 1
    return a


def staircase(h, w):
    """(i, i), (i, i + 1): one component with 4 neighbours; beside it a pure anti-diagonal: one component only with 8."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = xx - yy
    return (((d == 0) | (d == 1)) | (xx + yy == max(h, w) + 3)).astype(np.uint8)


def serpentine(h, w):
    """Full rows every second line, joined at alternating ends: ONE long path that crosses every tile border many times."""
    a = np.zeros((h, w), np.uint8)
    a[0::2] = 1
    for k, y in enumerate(range(1, h, 2)):
        a[y, w - 1 if k % 2 == 0 else 0] = 1
    return a


def spiral(h, w):
    a = np.zeros((h, w), np.uint8)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    a[0, :] = 1
    while True:                                  # right side down, bottom to the left, left side up, top to the right, two in
        if right - left < 2 or bottom - top < 2:
            break
        a[top:bottom + 1, right] = 1
        a[bottom, left:right + 1] = 1
        top += 2
        if bottom - top < 0:
            break
        a[top:bottom + 1, left] = 1
        right -= 2
        if right - left < 0:
            break
        a[top, left:right + 1] = 1
        bottom -= 2
        left += 2
    return a


def comb(h, w):
    """Arms in every second column that join only in the last row: many low roots, all merged late."""
    a = np.zeros((h, w), np.uint8)
    a[:, 0::2] = 1
    a[-1, :] = 1
    return a


def rings(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (np.maximum(np.abs(yy - h // 2), np.abs(xx - w // 2)) % 2 == 0).astype(np.uint8)


LONG_PATHS = [serpentine, spiral, comb, bars_along]
FIGURES = LONG_PATHS + [bars_across, staircase, rings, corners, checkerboard]


@functools.lru_cache(maxsize=None)
def images(h, w, full=True):
    """The pictures of one shape as one read-only batch."""
    imgs = [f(h, w) for f in (FIGURES if full else LONG_PATHS)]
    imgs += [noise(h, w, 0.59)]
    if full:
        imgs += [np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)]
        imgs += [noise(h, w, d) for d in (0.3, 0.5, 0.8)]
    if h >= 37 and w >= 53:
        imgs.extend(get_gray_mask(i) for i in scene_images(3 if full else 1, h, w))
    imgs = np.stack(imgs)
    imgs.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def expected(h, w, full, connectivity, erode):
    """(labels, counts) of images(h, w, full) from the oracle -- computed once and shared (never written to)."""
    out = [co.label(co.erode2x2(x) if erode else x, connectivity) for x in images(h, w, full)]
    labels, counts = np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)
    labels.setflags(write=False)
    counts.setflags(write=False)
    return labels, counts


def check_labels(h, w, full, connectivity, erode, off=0):
    want, want_k = expected(h, w, full, connectivity, erode)
    got, got_k = ccl_abi(images(h, w, full), connectivity, erode, off)
    assert np.array_equal(got_k, want_k), (h, w, connectivity, erode, got_k.tolist(), want_k.tolist())
    assert np.array_equal(got, want), (h, w, connectivity, erode, [int((g != x).sum()) for g, x in zip(got, want)])
    return want, want_k


# ---- labelling ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("h,w", SMALL)
def test_labels_small_shapes(h, w, off):
    for connectivity, erode in MODES:
        check_labels(h, w, True, connectivity, erode, off)


@pytest.mark.parametrize("which", ["one_tile", "one_over_in_rows", "one_over_in_columns", "three_by_three_ragged"])
def test_labels_at_the_tile_borders(which):
    th, tw = tile()
    h, w = {"one_tile": (th, tw), "one_over_in_rows": (th + 1, tw), "one_over_in_columns": (th, tw + 1),
            "three_by_three_ragged": (2 * th + 5, 2 * tw + 7)}[which]
    for connectivity, erode in MODES:
        _, k = check_labels(h, w, True, connectivity, erode)
    if which == "three_by_three_ragged":     # the checkerboard: the most components an image can have, and ONE with 8 neighbours
        i = [j for j, x in enumerate(images(h, w)) if np.array_equal(x, checkerboard(h, w))][0]
        assert expected(h, w, True, 1, 0)[1][i] == (h * w + 1) // 2 and expected(h, w, True, 2, 0)[1][i] == 1


@pytest.mark.parametrize("h,w,full", [(256, 256, True), (512, 512, False), (700, 900, False)])
def test_labels_baseline_sizes_and_one_beyond_the_skeleton_limit(h, w, full):
    """256 x 256 with every picture; 512 x 512 and 700 x 900 (no one-workgroup-per-image limit here) with the long-path figures,
    noise at the percolation density and a scene mask: the eroded image with 4 neighbours (the dense nodes' mode) and the
    plain one with 8 (the agents')."""
    for connectivity, erode in ((1, 1), (2, 0)):
        _, k = check_labels(h, w, full, connectivity, erode)
        assert k.max() > 100


def test_two_runs_give_the_same_bytes_and_a_side_stream_works():
    th, tw = tile()
    h, w = 3 * th + 1, 4 * tw - 3
    imgs = images(h, w)
    a, ka = ccl_abi(imgs, 2, 0)
    b, kb = ccl_abi(imgs, 2, 0)
    assert np.array_equal(a, b) and np.array_equal(ka, kb)
    c, kc = ccl_abi(imgs, 2, 0, stream=torch.cuda.Stream())
    assert np.array_equal(a, c) and np.array_equal(ka, kc)
    assert np.array_equal(a, expected(h, w, True, 2, 0)[0])


# ---- statistics, centres, merge -------------------------------------------------------------------------------------------------
def check_stats(labels, counts, cap):
    rec, cen = stats_abi(labels, counts, cap)
    for i in range(len(labels)):
        s = co.stats(labels[i], int(counts[i]))
        k = min(int(counts[i]), cap)
        assert np.array_equal(rec[i, :k], co.pack(s).view(np.int32).reshape(-1, 16)[:k]), (labels.shape, i, cap)
        assert np.array_equal(cen[i, :k], co.centers(s)[:k]), (labels.shape, i, cap)
        assert (rec[i, k:] == SENT32).all() and (cen[i, k:] == SENT32).all(), (labels.shape, i, cap)      # not written


@pytest.mark.parametrize("h,w", [(1, 1), (5, 33), (37, 53), (96, 70), (133, 211)])
def test_statistics_and_centres(h, w):
    for connectivity, erode in ((1, 1), (2, 0), (1, 0)):
        labels, counts = expected(h, w, True, connectivity, erode)
        check_stats(labels, counts, int(counts.max()) + 5)


def test_one_batch_of_three_different_images_and_caps_below_equal_and_above_the_count():
    h, w = 96, 70
    imgs = np.stack([noise(h, w, 0.3), np.zeros((h, w), np.uint8), rings(h, w)])
    got, counts = ccl_abi(imgs, 1, 0)
    want = [co.label(x, 1) for x in imgs]
    assert counts.tolist() == [k for _, k in want] and counts[1] == 0 and 1 < counts[2] < counts[0]
    assert np.array_equal(got, np.stack([x for x, _ in want])) and not got[1].any()
    for cap in (0, 1, int(counts[2]) - 1, int(counts[2]), int(counts[2]) + 1, int(counts[0]), int(counts[0]) + 7):
        check_stats(got, counts, cap)       # image 1: counts 0, nothing written, whatever the cap
    a, b = stats_abi(got, counts, 300), stats_abi(got, counts, 300)       # two runs: identical bytes
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_statistics_of_a_large_image_with_many_labels_per_workgroup():
    """256 x 256 checkerboard (32768 labels: every slot of a workgroup's table is fought over) and noise (large components
    that span many workgroups)."""
    imgs = np.stack([checkerboard(256, 256), noise(256, 256, 0.59), np.full((256, 256), 1, np.uint8)])
    out = [co.label(x, 1) for x in imgs]
    labels, counts = np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)
    check_stats(labels, counts, 40000)
    check_stats(labels, counts, 100)


def test_merge_nodes_against_the_oracle():
    rng = np.random.default_rng(5)
    dense = [co.dense_nodes(noise(96, 70, 0.59)), co.dense_nodes(noise(96, 70, 0.8)), np.zeros((0, 2), np.int32),
             np.array([[10, 14], [13, 14], [15, 11], [14, 12]], np.int32)]
    nodes = [rng.integers(0, 96, (40, 2)).astype(np.int32), np.zeros((0, 2), np.int32), rng.integers(0, 70, (9, 2)).astype(np.int32),
             np.array([[10, 10]], np.int32)]
    assert len(dense[0]) > 256 > len(dense[1]) > 3             # more than one round of the workgroup / less than one
    counts, dcounts = [len(x) for x in nodes], [len(x) for x in dense]
    want = [co.merge_nodes(a, d) for a, d in zip(nodes, dense)]
    assert want[3].tolist() == [[10, 10], [13, 14], [15, 11]]   # squared distances 20, 25, 26, 20 against < 25
    assert 40 < len(want[0]) < 40 + len(dense[0])
    for cap in (max(map(len, want)) + 3, len(want[0]), len(want[0]) - 1, 41, 40):
        got, out = merge_abi(nodes, counts, cap, dense, dcounts, max(dcounts))
        assert out.tolist() == [len(x) for x in want], cap         # the true count, whatever fits
        for i in range(4):
            k = min(len(want[i]), cap)
            assert np.array_equal(got[i, :k], want[i][:k]) and (got[i, k:] == SENT32).all(), (cap, i)
    # an original list that was cut (counts > cap): only the listed nodes are compared, nothing is appended
    got, out = merge_abi(nodes, counts, 10, dense, dcounts, max(dcounts))
    assert np.array_equal(got[0], nodes[0][:10]) and out[0] == 40 + len(co.merge_nodes(nodes[0][:10], dense[0])) - 10
    # a dense list that was cut, and other thresholds
    got, out = merge_abi(nodes, counts, 600, dense, dcounts, 5, min_d2=26)
    for i in range(4):
        w = co.merge_nodes(nodes[i], dense[i][:5], 26)
        assert out[i] == len(w) and np.array_equal(got[i, :len(w)], w) and (got[i, len(w):] == SENT32).all()
    assert got[3, :int(out[3])].tolist() == [[10, 10], [15, 11]]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    h, w = 40, 50
    need = workspace_bytes(1, h, w)
    src, ws = Guarded((1, h, w), torch.uint8, 0, np.ones((1, h, w), np.uint8)), Guarded((need,), torch.uint8)
    lab, cnt = Guarded((1, h, w), torch.int32), Guarded((1,), torch.int32)
    lib, st = _lib.load(), _lib.stream_ptr(torch.device(DEV))
    call = lambda **k: lib.dsg_ccl_u8(k.get("mask", src.ptr()), 1, k.get("h", h), k.get("w", w), k.get("conn", 1), k.get("erode", 0),  # noqa: E731
                                      k.get("labels", lab.ptr()), k.get("counts", cnt.ptr()), k.get("ws", ws.ptr()),
                                      k.get("bytes", need), st)
    assert call(conn=0) == -1 and b"connectivity" in lib.dsg_last_error()
    assert call(conn=3) == -1 and call(erode=2) == -1
    for name in ("mask", "labels", "counts", "ws"):
        assert call(**{name: None}) == -1 and b"NULL" in lib.dsg_last_error()
    assert call(h=32768, w=32769) == -1 and b"2^30" in lib.dsg_last_error()
    assert call(h=0) == -1 and call(w=-1) == -1
    assert call(bytes=need - 1) == -3 and b"needed" in lib.dsg_last_error()
    assert call(labels=src.ptr()) == -1 and b"overlaps" in lib.dsg_last_error()
    assert call(labels=src.ptr() + h * w - 4) == -1 and call(counts=src.ptr() + 8) == -1 and call(ws=src.ptr() - need + 1) == -1
    assert call(ws=lab.ptr() + 4) == -1 and call(counts=lab.ptr()) == -1 and call(ws=ws.ptr() + 1) == -1     # (the last: misaligned)
    size = ctypes.c_size_t()
    assert lib.dsg_ccl_workspace_bytes(1, 32768, 32769, ctypes.byref(size)) == -1 and lib.dsg_ccl_workspace_bytes(1, h, w, None) == -1
    rec = Guarded((1, 4, 16), torch.int32)
    assert lib.dsg_cc_stats_i32(None, 1, h, w, cnt.ptr(), rec.ptr(), 4, st) == -1
    assert lib.dsg_cc_stats_i32(lab.ptr(), 1, 40000, 2, cnt.ptr(), rec.ptr(), 4, st) == -1 and b"2^15" in lib.dsg_last_error()
    assert lib.dsg_cc_stats_i32(lab.ptr(), 1, h, w, cnt.ptr(), lab.ptr() + 64, 4, st) == -1
    assert lib.dsg_cc_centers_i32(rec.ptr(), None, 1, 4, lab.ptr(), st) == -1
    assert lib.dsg_merge_nodes_i32(lab.ptr(), cnt.ptr(), 1, 4, lab.ptr() + 4096, cnt.ptr(), 4, 25, cnt.ptr(), st) == -1
    assert lib.dsg_merge_nodes_i32(lab.ptr(), cnt.ptr(), 1, 4, lab.ptr() + 4096, cnt.ptr(), 4, -1, rec.ptr(), st) == -1
    torch.cuda.synchronize()
    for g, sent in ((lab, SENT32), (cnt, SENT32), (ws, SENT8), (rec, SENT32)):
        assert (g.get() == sent).all()                                                           # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert cnt.get().tolist() == [1] and (lab.get() == 1).all()
    with pytest.raises(_lib.DsgError, match="DSG_ERR_INVALID_ARG"):
        imageops.label_batch(src.view, connectivity=4)


# ---- wrappers -------------------------------------------------------------------------------------------------------------------
def test_wrappers_match_the_oracle():
    h, w = 96, 70
    imgs = images(h, w)
    x = torch.from_numpy(np.array(imgs)).to(DEV)
    for connectivity, erode in MODES:
        labels, counts = imageops.label_batch(x, connectivity, bool(erode))
        want, want_k = expected(h, w, True, connectivity, erode)
        assert labels.dtype == torch.int32 and counts.dtype == torch.int32
        assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_k)
    assert np.array_equal(x.cpu().numpy(), imgs)
    labels, counts = imageops.label_batch(x, 2)
    want, want_k = expected(h, w, True, 2, 0)
    st = imageops.component_stats_batch(labels, counts, cap=50)
    assert st["raw"].shape == (len(imgs), 50, 8) and st["area"].shape == (len(imgs), 50) and st["bbox"].shape == (len(imgs), 50, 4)
    assert st["sums"].shape == (len(imgs), 50, 5) and st["centers"].shape == (len(imgs), 50, 2)
    for i in range(len(imgs)):
        s, k = co.stats(want[i], int(want_k[i])), min(int(want_k[i]), 50)
        assert np.array_equal(st["area"][i].cpu().numpy(), np.pad(s["area"][:k], (0, 50 - k)))
        assert np.array_equal(st["bbox"][i, :k].cpu().numpy(), s["bbox"][:k]) and not st["raw"][i, k:].any()
        assert np.array_equal(st["sums"][i, :k].cpu().numpy(), s["sums"][:k])
        assert np.array_equal(st["centers"][i, :k].cpu().numpy(), co.centers(s)[:k]) and (st["centers"][i, k:] == -1).all()
    dense, dcounts = imageops.dense_skeleton_nodes_batch(x)
    assert dense.shape == (len(imgs), imageops.DEFAULT_NODE_CAP, 2)
    for i in range(len(imgs)):
        d = co.dense_nodes(imgs[i])
        assert dcounts[i].item() == len(d) and np.array_equal(dense[i, :len(d)].cpu().numpy(), d) and (dense[i, len(d):] == -1).all()
    few, nfew = imageops.dense_skeleton_nodes_batch(x, cap=2)
    assert few.shape == (len(imgs), 2, 2) and torch.equal(nfew, dcounts)


def test_lane_nodes_batch_end_to_end():
    """[4, 64, 64, 3] generated-style images against the chain get_gray_mask -> thin -> nodes -> oracle dense nodes -> oracle
    merge: the node list connect_graph holds after extract_network.py:242, in this engine's orientation."""
    images_u8 = scene_images(4, 64, 64, seed=77)
    x = torch.from_numpy(images_u8).to(DEV)
    mask, skel, coords, counts = imageops.lane_nodes_batch(x)
    base = imageops.lane_skeleton_batch(x)
    assert torch.equal(mask, base[0]) and torch.equal(skel, base[1])
    coords_h, counts_h = coords.cpu().numpy(), counts.cpu().numpy()
    for i, im in enumerate(images_u8):
        s, _ = so.thin(get_gray_mask(im))
        assert np.array_equal(skel[i].cpu().numpy(), s)
        want = co.merge_nodes(so.nodes(s), co.dense_nodes(s))
        assert counts_h[i] == len(want) >= len(so.nodes(s)) > 0
        assert np.array_equal(coords_h[i, :len(want)], want) and (coords_h[i, len(want):] == -1).all()
    # a thinned scene has few 2 x 2 blocks; the raw mask has many: the merge on it keeps and drops some
    dense, dcounts = imageops.dense_skeleton_nodes_batch(mask)
    merged, mcounts = imageops.merge_dense_nodes_batch(base[2], base[3], dense, dcounts, min_distance=3)
    kept = 0
    for i, im in enumerate(images_u8):
        m = get_gray_mask(im)
        nodes, d = so.nodes(so.thin(m)[0]), co.dense_nodes(m)
        want = co.merge_nodes(nodes, d, 9)
        kept += len(want) - len(nodes)
        assert mcounts[i].item() == len(want) and np.array_equal(merged[i, :len(want)].cpu().numpy(), want)
    assert kept > 0


def test_agent_blobs_batch_end_to_end():
    images_u8 = scene_images(4, 96, 128, seed=9)
    x = torch.from_numpy(images_u8).to(DEV)
    labels, counts, st = imageops.agent_blobs_batch(x, cap=64)
    mask = imageops.agent_mask_batch(x).cpu().numpy()
    assert mask.any()
    for i in range(len(images_u8)):
        want, k = co.label(mask[i], 2)
        s = co.stats(want, k)
        assert counts[i].item() == k and np.array_equal(labels[i].cpu().numpy(), want)
        kk = min(k, 64)
        assert np.array_equal(st["raw"][i, :kk].cpu().numpy(), co.pack(s)[:kk]) and not st["raw"][i, kk:].any()
        assert np.array_equal(st["centers"][i, :kk].cpu().numpy(), co.centers(s)[:kk])
    assert counts.sum().item() > 0


def test_the_chain_runs_under_graph_capture():
    """label_batch + component_stats_batch + dense_skeleton_nodes_batch + merge_dense_nodes_batch recorded into one graph after
    a warm-up call, replayed once and compared with the eager result: no allocation outside torch's, no readback, no
    synchronisation in any of them."""
    h, w = 96, 70
    x = torch.from_numpy(np.array(images(h, w))).to(DEV)
    nodes = torch.full((len(x), 600, 2), -1, dtype=torch.int32, device=DEV)      # one original node per image, at (0, 0)
    nodes[:, 0] = 0
    ncounts = torch.ones((len(x),), dtype=torch.int32, device=DEV)

    def chain():
        labels, counts = imageops.label_batch(x, 2)
        st = imageops.component_stats_batch(labels, counts, cap=128)
        dense, dcounts = imageops.dense_skeleton_nodes_batch(x, cap=512)
        merged, mcounts = imageops.merge_dense_nodes_batch(nodes, ncounts, dense, dcounts)
        return labels, counts, st["raw"], st["centers"], dense, dcounts, merged, mcounts

    eager = [t.clone() for t in chain()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        chain()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = chain()
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))
    assert eager[1].max().item() > 1 and eager[5].max().item() > 1 and eager[7].max().item() > 100
