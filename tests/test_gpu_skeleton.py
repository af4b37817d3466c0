"""The skeleton stage on the GPU: ``dsg_thin_lut_u8`` and ``dsg_skel_nodes_u8`` (csrc/skeleton.hip) and their wrappers in
drivescenegen_amd/imageops.py against tests/skeleton_oracle.py, BITWISE -- skeleton bytes, iteration counts, node classes,
coordinates, their order and their counts; nothing here has a tolerance.

The kernel tests go through the C ABI on buffers that sit between sentinel margins (>= 4 KiB each side; the ``_guarded``
idiom of tests/test_gpu_ema.py -- tests/redzone_child.py does not list these kernels and stays as it is).  The input's
margins are NON-ZERO bytes, so a neighbour read outside the image would also show as a wrong skeleton.  Every input must
come back unchanged.  ``off`` moves a buffer off its 16-byte alignment: the kernel then packs and unpacks one pixel per lane
instead of sixteen, also for widths that are multiples of 32."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drivescenegen_amd import _lib, imageops, synth  # noqa: E402
from oracle.postproc_oracle import get_gray_mask  # noqa: E402
from tests import skeleton_oracle as so  # noqa: E402

DEV = "cuda"
MARGIN = 4096            # bytes (uint8 buffers) / elements (int32 buffers)
SENT8, SENT32 = 0xA5, -777
SMALL = [(1, 1), (1, 40), (37, 1), (2, 2), (5, 31), (5, 32), (5, 33), (9, 64), (37, 53), (96, 70)]
BASELINE = [(256, 256), (512, 512)]
TABLE = so.zhang_suen_table()


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


def thin_abi(imgs, table=TABLE, max_iters=None, off=0, stream=None):
    """dsg_thin_lut_u8 on guarded buffers -> (skeleton, iterations); margins and the input are checked."""
    n, h, w = imgs.shape
    src, lut = Guarded((n, h, w), torch.uint8, off, imgs), Guarded((256,), torch.uint8, 0, table)
    dst, its = Guarded((n, h, w), torch.uint8, off), Guarded((n,), torch.int32)
    st = _lib.stream_ptr(torch.device(DEV)) if stream is None else stream.cuda_stream
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    _lib.check(_lib.load().dsg_thin_lut_u8(src.ptr(), n, h, w, lut.ptr(), h + w if max_iters is None else max_iters, dst.ptr(),
                                          its.ptr(), st))
    torch.cuda.synchronize()
    assert np.array_equal(src.get(), imgs) and np.array_equal(lut.get(), table)
    return dst.get(), its.get()


def nodes_abi(imgs, cap, with_class=True, off=0):
    """dsg_skel_nodes_u8 on guarded buffers -> (coords [n, cap, 2] with SENT32 where nothing was written, counts, class or None)."""
    n, h, w = imgs.shape
    src = Guarded((n, h, w), torch.uint8, off, imgs)
    cls = Guarded((n, h, w), torch.uint8, off) if with_class else None
    co, cn = Guarded((n, max(cap, 1), 2), torch.int32), Guarded((n,), torch.int32)
    _lib.check(_lib.load().dsg_skel_nodes_u8(src.ptr(), n, h, w, cls.ptr() if with_class else None, co.ptr() if cap else None,
                                            cap, cn.ptr(), _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert np.array_equal(src.get(), imgs)
    return co.get()[:, :cap], cn.get(), cls.get() if with_class else None


def check_nodes(imgs, cap, with_class=True, off=0):
    coords, counts, cls = nodes_abi(imgs, cap, with_class, off)
    for i, img in enumerate(imgs):
        want = so.nodes(img)
        assert counts[i] == len(want), (imgs.shape, i, counts[i], len(want))      # the true number, whatever cap is
        k = min(len(want), cap)
        assert np.array_equal(coords[i, :k], want[:k]), (imgs.shape, i, cap)
        assert (coords[i, k:] == SENT32).all(), (imgs.shape, i, cap)              # rows behind the list: untouched
        if with_class:
            assert np.array_equal(cls[i], so.node_class(img)), (imgs.shape, i)
    return counts


# ---- contents -----------------------------------------------------------------------------------------------------------------
def scene_images(n, h, w, seed=14555):
    r = synth.synth_scene_rasters(n, 3, h, w, seed)
    return ((r.transpose(0, 2, 3, 1) * 0.5 + 0.5) * 255).round().astype(np.uint8)


def scene_masks(n, h, w, seed=14555):
    return np.stack([get_gray_mask(i) for i in scene_images(n, h, w, seed)])


def noise(h, w, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    return ((rng.random((h, w)) < 0.35) * rng.integers(1, 256, (h, w))).astype(np.uint8)   # any non-zero byte is "on"


def bars(h, w):
    """Bars two and three pixels thick -- horizontal, vertical, both diagonals -- laid across the 32-pixel word boundaries."""
    a = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for k, t in enumerate((2, 3)):
        y0 = (3 + 9 * k) % max(h, 1)
        a[y0:y0 + t, max(0, w // 8):] = 255                       # horizontal, over every word boundary to the right edge
        for xb in range(32, w + 32, 32):                          # vertical, straddling (t = 2) or ending at / starting on a boundary
            x0 = xb - 1 - k
            a[h // 4:, max(0, x0):max(0, x0) + t] = 255
        d = xx - yy - (5 + 40 * k)
        a[(d >= 0) & (d < t)] = 255                               # diagonal, crossing boundaries one column per row
        e = xx + yy - (w - 1 + 7 * k)
        a[(e >= 0) & (e < t)] = 255
    return a


def borders(h, w):
    """A frame on all four borders, 3 x 3 blobs in all four corners, and a cross that runs from border to border."""
    a = np.zeros((h, w), np.uint8)
    a[0, :] = a[-1, :] = a[:, 0] = a[:, -1] = 1
    a[:3, :3] = a[:3, -3:] = a[-3:, :3] = a[-3:, -3:] = 1
    a[h // 2, :] = a[:, w // 2] = 1
    return a


def single(h, w):
    a = np.zeros((h, w), np.uint8)
    a[h // 2, w - 1] = 7
    return a


def _thinned(imgs):
    imgs = np.stack(imgs)
    thinned = [so.thin(x) for x in imgs]
    skel, its = np.stack([t[0] for t in thinned]), np.array([t[1] for t in thinned], np.int32)
    for a in (imgs, skel, its):
        a.setflags(write=False)
    return imgs, skel, its


@functools.lru_cache(maxsize=None)
def case(h, w):
    """(images [n, h, w], oracle skeletons, oracle iteration counts) -- computed once and shared (never written to)."""
    imgs = [noise(h, w), bars(h, w), borders(h, w)]
    if h * w > 512 * 512:
        return _thinned(imgs)
    imgs += [np.zeros((h, w), np.uint8), single(h, w)]
    if h * w <= 96 * 70:
        imgs.append(np.full((h, w), 255, np.uint8))
    if h >= 37 and w >= 53:
        imgs.extend(scene_masks(2, h, w))
    return _thinned(imgs)


# ---- thinning -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("h,w", SMALL)
def test_thinning_small_shapes(h, w, off):
    imgs, skel, its = case(h, w)
    got, got_its = thin_abi(imgs, off=off)
    assert np.array_equal(got_its, its), (got_its, its)
    assert np.array_equal(got, skel), [int((g != s).sum()) for g, s in zip(got, skel)]


@pytest.mark.parametrize("h,w", BASELINE)
def test_thinning_and_nodes_baseline_sizes(h, w):
    imgs, skel, its = case(h, w)
    got, got_its = thin_abi(imgs)
    assert np.array_equal(got_its, its), (got_its, its)
    assert np.array_equal(got, skel), [int((g != s).sum()) for g, s in zip(got, skel)]
    assert all(4 <= k <= 9 for k in its[-2:])                       # the two scene masks
    check_nodes(np.concatenate([skel[-2:], imgs[:1]]), cap=imageops.DEFAULT_NODE_CAP if h == 256 else 100)
    if h == 256:   # the noise image alone has more nodes per wave than the kernel keeps in LDS: its second walk, with room to spare
        assert check_nodes(imgs[:1], cap=12000, with_class=False)[0] > 4096


def test_thinning_more_than_eight_words_per_thread():
    """544 x 600: 10336 packed words, the kernel's instantiation for more than 8 words per thread (up to 4: everything up to
    256 x 512; up to 8: 512 x 512), near the LDS limit (57.9 of 64 KiB), a width that is no multiple of 32."""
    imgs, skel, its = case(544, 600)
    got, got_its = thin_abi(imgs[:3])
    assert np.array_equal(got_its, its[:3]), (got_its, its)
    assert np.array_equal(got, skel[:3]), [int((g != s).sum()) for g, s in zip(got, skel)]


def test_more_than_128_iterations_wrap_the_change_bytes():
    """A two-pixel staircase diagonal is eaten from both ends, two pixels per iteration: 272 x 272 takes 137 iterations,
    274 sub-iterations, so the kernel's one-byte "last change" stamps wrap (they count sub-iterations mod 256) while most of
    the image has been still for long; a skeleton that is already thin sits beside it and must stay as it is throughout.
    (The bars of the 512 x 512 and 544 x 600 cases run for 152 iterations and wrap as well.)"""
    h = w = 272
    yy, xx = np.mgrid[0:h, 0:w]
    e = xx + yy - (w - 1)
    thin_already = np.pad(case(96, 70)[1][-1], ((88, 88), (101, 101)))      # a scene's skeleton in the middle of the image
    imgs = np.stack([((e >= 0) & (e < 2)).astype(np.uint8), thin_already])
    want = [so.thin(x) for x in imgs]
    assert want[0][1] == 137 and want[0][0].sum() == 1 and want[1][1] == 1
    got, its = thin_abi(imgs)
    assert its.tolist() == [137, 1] and np.array_equal(got, np.stack([t[0] for t in want]))


def test_one_batch_with_very_different_iteration_counts():
    """All-zero, single-pixel, all-ones and scene images in ONE launch: 1, 1, 33 and a handful of iterations.  Each workgroup
    leaves its loop on its own count; a wrong exit or a barrier under divergent control shows here."""
    imgs = np.stack([np.zeros((64, 64), np.uint8), single(64, 64), np.full((64, 64), 255, np.uint8)] + list(scene_masks(3, 64, 64)))
    want = [so.thin(x) for x in imgs]
    got, its = thin_abi(imgs)
    assert its.tolist() == [t[1] for t in want] and its[:3].tolist() == [1, 1, 33] and all(4 <= k <= 9 for k in its[3:])
    assert np.array_equal(got, np.stack([t[0] for t in want]))
    assert got[2].sum() == 1 and np.array_equal(got[1], (imgs[1] != 0).astype(np.uint8))
    again, its2 = thin_abi(imgs)                                       # two runs: identical bytes
    assert np.array_equal(again, got) and np.array_equal(its2, its)
    side = torch.cuda.Stream()                                         # and on a stream that is not the default one
    third, its3 = thin_abi(imgs, stream=side)
    assert np.array_equal(third, got) and np.array_equal(its3, its)


@pytest.mark.parametrize("h,w", [(37, 53), (96, 70), (9, 64)])
def test_custom_table(h, w):
    """256 seeded random values in 0..3: the kernel is table-driven, not Zhang-Suen in disguise.  A table only deletes, so the
    loop ends within h * w iterations."""
    table = np.random.default_rng(42).integers(0, 4, 256).astype(np.uint8)
    imgs = np.stack([noise(h, w), noise(h, w, 1)])
    want = [so.thin(x, table) for x in imgs]
    got, its = thin_abi(imgs, table=table, max_iters=h * w + 1)
    assert its.tolist() == [t[1] for t in want] and np.array_equal(got, np.stack([t[0] for t in want]))
    assert not np.array_equal(got[0], so.thin(imgs[0])[0])


def test_iteration_bound():
    """max_iters = 3 on the all-ones 64 x 64 image (33 iterations to converge): the call returns, iters is -1 and the image is
    the oracle's after three iterations; beside it an image that does converge within three."""
    imgs = np.stack([np.full((64, 64), 255, np.uint8), single(64, 64)])
    cut, it = so.thin(imgs[0], max_iters=3)
    assert it == -1
    got, its = thin_abi(imgs, max_iters=3)
    assert its.tolist() == [-1, 1] and np.array_equal(got[0], cut) and got[0].sum() > 1
    got33, its33 = thin_abi(imgs, max_iters=33)                        # the idle iteration is the 33rd: converged
    assert its33.tolist() == [33, 1] and got33[0].sum() == 1
    x = torch.from_numpy(imgs).to(DEV)
    with pytest.raises(RuntimeError, match="not converged"):
        imageops.skeletonize_batch(x, max_iters=3, return_iters=True)
    assert np.array_equal(imageops.skeletonize_batch(x, max_iters=3).cpu().numpy()[0], cut)   # not asked for: not read back


def test_a_shape_beyond_the_lds_limit_is_refused_before_any_launch():
    h = w = 768
    src, lut = Guarded((1, h, w), torch.uint8, 0, np.ones((1, h, w), np.uint8)), Guarded((256,), torch.uint8, 0, TABLE)
    dst, its = Guarded((1, h, w), torch.uint8), Guarded((1,), torch.int32)
    lib = _lib.load()
    rc = lib.dsg_thin_lut_u8(src.ptr(), 1, h, w, lut.ptr(), 10, dst.ptr(), its.ptr(), _lib.stream_ptr(torch.device(DEV)))
    assert rc == -1 and b"does not fit" in lib.dsg_last_error()
    torch.cuda.synchronize()
    assert (dst.get() == SENT8).all() and (its.get() == SENT32).all()          # nothing ran
    with pytest.raises(_lib.DsgError, match="DSG_ERR_INVALID_ARG"):
        imageops.skeletonize_batch(src.view)
    assert lib.dsg_thin_lut_u8(src.ptr(), 1, 640, 640, lut.ptr(), 10, src.ptr(), its.ptr(), None) == -1     # skel aliases mask


# ---- nodes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("h,w", SMALL)
def test_nodes_small_shapes(h, w, off):
    """On the skeletons and on the raw images (input that is not a skeleton is legal), with room to spare: the rows behind
    the list stay untouched."""
    imgs, skel, _ = case(h, w)
    both = np.concatenate([skel, imgs])
    counts = check_nodes(both, cap=h * w + 5, off=off)
    if h * w > 1:
        assert counts.max() > 0 or max(h, w) <= 2


def test_nodes_cap_smaller_than_the_count_and_no_class_buffer():
    imgs, skel, _ = case(96, 70)
    both = np.concatenate([skel, imgs])
    full = check_nodes(both, cap=96 * 70, with_class=False)
    assert full.max() > 64
    for cap in (0, 1, 63, 64, 65):
        assert np.array_equal(check_nodes(both, cap=cap, with_class=(cap == 64)), full)
    a, b = nodes_abi(both, 200), nodes_abi(both, 200)                  # two runs: identical bytes
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- wrappers -----------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_what_they_cannot_run():
    cpu = torch.zeros((1, 8, 8), dtype=torch.uint8)
    for fn in (imageops.skeletonize_batch, imageops.skeleton_nodes_batch):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(cpu)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(cpu.to(DEV).float())
    x = cpu.to(DEV)
    for bad in (np.zeros(255, np.uint8), np.full(256, 4, np.uint8), np.zeros(256, np.float32)):
        with pytest.raises(ValueError, match="lut"):
            imageops.skeletonize_batch(x, lut=bad)


def test_wrappers_match_the_oracle_and_a_custom_table_reaches_the_kernel():
    imgs, skel, its = case(96, 70)
    x = torch.from_numpy(np.array(imgs)).to(DEV)
    got, got_its = imageops.skeletonize_batch(x, return_iters=True)
    assert got.dtype == torch.uint8 and got_its.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), skel) and np.array_equal(got_its.cpu().numpy(), its)
    assert np.array_equal(x.cpu().numpy(), imgs)
    table = np.random.default_rng(42).integers(0, 4, 256)
    custom = imageops.skeletonize_batch(x[:1], lut=table, max_iters=96 * 70 + 1)
    assert np.array_equal(custom.cpu().numpy()[0], so.thin(imgs[0], table.astype(np.uint8))[0])
    coords, counts, cls = imageops.skeleton_nodes_batch(got, return_class=True)
    assert coords.shape == (len(imgs), imageops.DEFAULT_NODE_CAP, 2) and coords.dtype == torch.int32 and counts.dtype == torch.int32
    coords, counts, cls = coords.cpu().numpy(), counts.cpu().numpy(), cls.cpu().numpy()
    for i, s in enumerate(skel):
        want = so.nodes(s)
        assert counts[i] == len(want) and np.array_equal(coords[i, :len(want)], want) and (coords[i, len(want):] == -1).all()
        assert np.array_equal(cls[i], so.node_class(s))
    few, n_few = imageops.skeleton_nodes_batch(got, cap=2)
    assert few.shape == (len(imgs), 2, 2) and np.array_equal(n_few.cpu().numpy(), counts)


def test_lane_skeleton_batch_end_to_end_and_under_graph_capture():
    """[4, 64, 64, 3] generated-style images -> mask, skeleton, nodes against the oracle chain get_gray_mask -> thin -> nodes.

    ``gray_mask_batch`` reads its histograms back to build the decision tables on the host, and a device-to-host copy cannot
    be recorded into a graph; so the captured part is ``skeletonize_batch`` + ``skeleton_nodes_batch`` on the mask -- a linear
    chain of a fill and two kernels -- replayed once and compared with the eager result."""
    images = scene_images(4, 64, 64, seed=77)
    x = torch.from_numpy(images).to(DEV)
    mask, skel, coords, counts = imageops.lane_skeleton_batch(x)
    torch.cuda.synchronize()
    want_mask = np.stack([get_gray_mask(i) for i in images])
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    coords_h, counts_h = coords.cpu().numpy(), counts.cpu().numpy()
    for i, m in enumerate(want_mask):
        s, _ = so.thin(m)
        want = so.nodes(s)
        assert np.array_equal(skel[i].cpu().numpy(), s)
        assert counts_h[i] == len(want) > 0 and np.array_equal(coords_h[i, :len(want)], want)
        assert (coords_h[i, len(want):] == -1).all()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        imageops.skeleton_nodes_batch(imageops.skeletonize_batch(mask))            # warm-up: the default table is uploaded here
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            g_skel = imageops.skeletonize_batch(mask)
            g_coords, g_counts = imageops.skeleton_nodes_batch(g_skel)
    torch.cuda.current_stream().wait_stream(side)
    g_skel.zero_()
    g_coords.zero_()
    g_counts.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_skel, skel) and torch.equal(g_coords, coords) and torch.equal(g_counts, counts)
