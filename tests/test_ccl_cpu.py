"""tests/ccl_oracle.py -- the NumPy restatement the GPU tests compare with, bit for bit -- against scipy.ndimage, the library the
reference itself calls for this step (extract_network.py:98-103: binary_erosion via skimage, label, center_of_mass), and
against figures whose answers are known.  No GPU."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import ccl_oracle as co

SMALL = [(1, 1), (1, 40), (37, 1), (2, 2), (5, 31), (5, 32), (5, 33), (9, 64), (37, 53), (96, 70)]
DENSITIES = [0.3, 0.5, 0.59, 0.8]
EIGHT = np.ones((3, 3), int)


def noise(h, w, density, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    return ((rng.random((h, w)) < density) * rng.integers(1, 256, (h, w))).astype(np.uint8)


def check_against_scipy(a):
    for connectivity, structure in ((1, None), (2, EIGHT)):
        want, k = ndimage.label(a, structure)
        got, got_k = co.label(a, connectivity)
        assert got_k == k and got.dtype == np.int32 and np.array_equal(got, want), (a.shape, connectivity)
        s = co.stats(got, k)
        idx = np.arange(1, k + 1)
        rr, cc = np.mgrid[0:a.shape[0], 0:a.shape[1]]
        assert np.array_equal(s["area"], ndimage.sum(np.ones_like(want), want, idx).astype(np.int64))
        for col, v in enumerate((rr, cc, rr * rr, cc * cc, rr * cc)):
            assert np.array_equal(s["sums"][:, col], np.asarray(ndimage.sum(v, want, idx)).astype(np.int64))
        boxes = [(sl[0].start, sl[1].start, sl[0].stop, sl[1].stop) for sl in ndimage.find_objects(want)]
        assert np.array_equal(s["bbox"], np.array(boxes, np.int32).reshape(k, 4))
        com = ndimage.center_of_mass(a != 0, want, [*range(1, k + 1)])
        assert np.array_equal(co.centers(s), np.array([(int(x), int(y)) for x, y in com], np.int32).reshape(k, 2))
        assert co.pack(s).shape == (k, 8)
    eroded = ndimage.binary_erosion(np.pad(a != 0, 1), np.ones((2, 2)))[1:-1, 1:-1]
    assert np.array_equal(co.erode2x2(a), eroded)
    # find_dense_skeleton_nodes, line by line
    lab, k = ndimage.label(eroded)
    com = ndimage.center_of_mass(eroded, lab, [*range(1, k + 1)])
    assert np.array_equal(co.dense_nodes(a), np.array([(int(x), int(y)) for x, y in com], np.int32).reshape(k, 2))


@pytest.mark.parametrize("h,w", SMALL)
def test_oracle_equals_scipy_on_noise(h, w):
    for density in DENSITIES:
        check_against_scipy(noise(h, w, density))


def test_named_figures():
    board = (np.indices((8, 8)).sum(0) % 2 == 0).astype(np.uint8)
    assert co.label(board, 1)[1] == 32 and co.label(board, 2)[1] == 1
    lab, k = co.label(board, 1)
    assert np.array_equal(lab[board != 0], np.arange(1, 33))          # numbered in row-major order of the first pixel
    ring = np.zeros((9, 11), np.uint8)
    ring[1:8, 1:10] = 1
    ring[2:7, 2:9] = 0
    assert co.label(ring, 1)[1] == 1 and co.label(ring, 2)[1] == 1
    s = co.stats(*co.label(ring, 1))
    assert s["area"].tolist() == [28] and s["bbox"].tolist() == [[1, 1, 8, 10]] and co.centers(s).tolist() == [[4, 5]]
    block = np.zeros((6, 7), np.uint8)
    block[2:4, 3:5] = 9
    assert np.argwhere(co.erode2x2(block)).tolist() == [[3, 4]]       # the corner with the larger indices
    assert co.dense_nodes(block).tolist() == [[3, 4]]
    edge = np.ones((3, 3), np.uint8)                                   # outside the image is off: row 0 and column 0 go
    assert np.array_equal(co.erode2x2(edge), np.array([[0, 0, 0], [0, 1, 1], [0, 1, 1]], bool))
    diag = np.eye(5, dtype=np.uint8)
    assert co.label(diag, 1)[1] == 5 and co.label(diag, 2)[1] == 1
    assert co.label(np.zeros((4, 4), np.uint8), 2)[1] == 0 and co.stats(np.zeros((4, 4), np.int32), 0)["area"].shape == (0,)
    for a in (board, ring, block, edge, diag):
        check_against_scipy(a)


@pytest.mark.parametrize("h,w", [(37, 53), (96, 70)])
def test_dense_nodes_of_the_transpose_are_the_same_set_with_coordinates_swapped(h, w):
    """The reference works on mask.T; the engine keeps the image's orientation.  Only the list order differs."""
    for density in (0.59, 0.8):
        a = noise(h, w, density)
        here, there = co.dense_nodes(a), co.dense_nodes(a.T)
        assert len(here) == len(there) > 1
        assert sorted(map(tuple, here.tolist())) == sorted((c, r) for r, c in there.tolist())


def test_add_dense_nodes_is_strict_and_compares_with_the_original_nodes_only():
    # distances sqrt(24), 5 and sqrt(26) from the one original node: kept from 5 on.  (24 is no sum of two squares, so that
    # point is off the lattice: 24 ** 0.5 squared is 24 to within an ulp, far from 25.)
    got = co.merge_nodes([(10.0, 10.0)], [(10.0, 10 + 24 ** 0.5), (13.0, 14.0), (10 + 26 ** 0.5, 10.0)], 25)
    assert got.tolist() == [[10.0, 10.0], [13.0, 14.0], [10 + 26 ** 0.5, 10.0]]
    # on the lattice: squared distances 20, 25, 26 against min_d2 = 25, and 25 against 24 and 26
    nodes = [(10, 10)]
    near, exact, beyond = (12, 14), (13, 14), (15, 11)
    got = co.merge_nodes(nodes, [near, exact, beyond], 25)
    assert got.dtype == np.int32 and got.tolist() == [[10, 10], [13, 14], [15, 11]]
    assert co.merge_nodes(nodes, [exact], 26).tolist() == [[10, 10]]
    assert co.merge_nodes(nodes, [exact], 24).tolist() == [[10, 10], [13, 14]]
    # two dense nodes next to each other, far from every original: both kept (kept nodes are not compared with)
    assert co.merge_nodes(nodes, [(40, 40), (40, 41)], 25).tolist() == [[10, 10], [40, 40], [40, 41]]
    # the reference's function, restated by hand on one more list, order kept
    ref = [*nodes, (3, 3), (30, 2)]
    dense = [(3, 4), (20, 20), (30, 7), (30, 6), (0, 0)]
    want = ref + [d for d in dense if all((d[0] - n[0]) ** 2 + (d[1] - n[1]) ** 2 >= 25 for n in ref)]
    assert co.merge_nodes(ref, dense).tolist() == [list(p) for p in want] and len(want) == 5
    assert co.merge_nodes([], dense).tolist() == [list(p) for p in dense] and co.merge_nodes(ref, []).shape == (3, 2)


def test_wrappers_refuse_cpu_tensors():
    from drivescenegen_amd import imageops
    m = torch.zeros((1, 8, 8), dtype=torch.uint8)
    lab, cnt = torch.zeros((1, 8, 8), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32)
    nodes = torch.zeros((1, 4, 2), dtype=torch.int32)
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    for fn, args in ((imageops.label_batch, (m,)), (imageops.component_stats_batch, (lab, cnt)),
                     (imageops.dense_skeleton_nodes_batch, (m,)), (imageops.merge_dense_nodes_batch, (nodes, cnt, nodes, cnt)),
                     (imageops.lane_nodes_batch, (img,)), (imageops.agent_blobs_batch, (img,))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*args)
