"""The skeleton stage without a GPU: tests/skeleton_oracle.py (the NumPy restatement the GPU tests compare against) held to
the known answers of the published definition (Zhang & Suen, CACM 27(3), 1984), and the one piece of product code that runs
on the host, ``imageops.zhang_suen_lut``.  Every comparison is exact."""
import numpy as np
import pytest
from scipy import ndimage

from drivescenegen_amd import synth
from oracle.postproc_oracle import get_gray_mask
from tests import skeleton_oracle as so

EIGHT = np.ones((3, 3), int)


def scene_masks(n, h, w, seed=14555):
    """The lane masks (0 / 255) of n synthetic scenes: rasters -> uint8 images as a pipeline returns them -> get_gray_image."""
    r = synth.synth_scene_rasters(n, 3, h, w, seed)
    imgs = ((r.transpose(0, 2, 3, 1) * 0.5 + 0.5) * 255).round().astype(np.uint8)
    return np.stack([get_gray_mask(i) for i in imgs])


@pytest.fixture(scope="module")
def scenes():
    """shape -> (masks, [(skeleton, iterations)]), thinned once for the module."""
    out = {}
    for n, h, w in ((3, 64, 64), (3, 96, 70), (2, 256, 256), (1, 512, 512)):
        m = scene_masks(n, h, w)
        out[(h, w)] = (m, [so.thin(x) for x in m])
    return out


def test_default_table_known_answers_and_product_table():
    t = so.zhang_suen_table()
    assert t.dtype == np.uint8 and t.shape == (256,)
    assert np.bincount(t, minlength=4).tolist() == [216, 6, 6, 28]
    assert t[:16].tolist() == [0, 0, 0, 3, 0, 0, 3, 3, 0, 0, 0, 0, 3, 0, 3, 3]
    from drivescenegen_amd import imageops
    p = imageops.zhang_suen_lut()
    assert p.dtype == np.uint8 and p.shape == (256,) and np.array_equal(p, t)


@pytest.mark.parametrize("side,iters", [(64, 33), (512, 257)])
def test_all_ones_square(side, iters):
    skel, it = so.thin(np.ones((side, side), np.uint8))
    assert it == iters and int(skel.sum()) == 1


def test_iteration_bound_and_idle_iteration():
    ones = np.ones((64, 64), np.uint8)
    full, _ = so.thin(ones)
    cut, it = so.thin(ones, max_iters=3)
    assert it == -1 and cut.sum() > full.sum() and np.all(cut >= full)
    assert so.thin(ones, max_iters=33)[1] == 33 and so.thin(ones, max_iters=32)[1] == -1   # the idle iteration counts
    assert so.thin(np.zeros((5, 7), np.uint8)) [1] == 1
    one = np.zeros((5, 7), np.uint8)
    one[2, 3] = 200                                         # non-zero = on; an isolated pixel has B = 0 and stays
    skel, it = so.thin(one)
    assert it == 1 and skel[2, 3] == 1 and skel.sum() == 1


def test_scene_masks_thin_in_few_iterations_to_a_subset_that_is_stable_and_transposes(scenes):
    for (h, w), (masks, thinned) in scenes.items():
        for m, (skel, it) in zip(masks, thinned):
            assert 4 <= it <= 9, (h, w, it)   # (a known answer for THESE scenes; others of the same generator take up to 38)
            assert set(np.unique(skel)) <= {0, 1} and skel.sum() > 0
            assert not np.any(skel.astype(bool) & ~(m != 0))                 # a subset of the mask
            again, it2 = so.thin(skel)
            assert it2 == 1 and np.array_equal(again, skel)                  # idempotent
            if h <= 256:
                t_skel, t_it = so.thin(np.ascontiguousarray(m.T))
                assert t_it == it and np.array_equal(t_skel.T, skel)         # the reference thins mask.T: no difference


def test_component_counts_are_kept(scenes):
    for shape in ((64, 64), (96, 70)):
        masks, thinned = scenes[shape]
        for m, (skel, _) in zip(masks, thinned):
            before, after = ndimage.label(m != 0, structure=EIGHT)[1], ndimage.label(skel, structure=EIGHT)[1]
            assert before == after and before >= 1, (shape, before, after)


def _nodes(img):
    return [tuple(int(v) for v in p) for p in so.nodes(img)]


def test_nodes_of_hand_checkable_figures():
    line = np.zeros((5, 9), np.uint8)
    line[2, 1:8] = 1
    assert _nodes(line) == [(2, 1), (2, 7)]
    assert _nodes(line.T) == [(1, 2), (7, 2)]

    # a "T": the bar's two ends, the stem's end and the junction (W, E and S on: three runs).  The bar pixels beside the
    # junction see the junction and the stem's first pixel as ONE run (E + SE), the stem's first pixel sees NW + N + NE as one
    t = np.zeros((7, 9), np.uint8)
    t[1, 1:8] = 1
    t[2:6, 4] = 1
    want_t = [(1, 1), (1, 4), (1, 7), (5, 4)]
    assert _nodes(t) == want_t
    cls = so.node_class(t)
    assert cls[1, 1] == 1 and cls[1, 7] == 1 and cls[5, 4] == 1 and cls[1, 4] == 3 and cls[1, 3] == 0 and cls[2, 4] == 0

    plus = np.zeros((7, 7), np.uint8)
    plus[3, 1:6] = 1
    plus[1:6, 3] = 1
    assert _nodes(plus) == [(1, 3), (3, 1), (3, 3), (3, 5), (5, 3)]
    assert so.node_class(plus)[3, 3] == 4

    dot = np.zeros((3, 3), np.uint8)
    dot[1, 1] = 1
    assert _nodes(dot) == [] and so.crossings(dot)[1, 1] == 0

    ring = np.zeros((6, 6), np.uint8)
    ring[1, 1:5] = ring[4, 1:5] = 1
    ring[1:5, 1] = ring[1:5, 4] = 1
    assert _nodes(ring) == [] and set(so.crossings(ring)[ring == 1]) == {2}

    # the border is off: a line along row 0 ending in the corner
    edge = np.zeros((3, 4), np.uint8)
    edge[0, :] = 1
    assert _nodes(edge) == [(0, 0), (0, 3)]
    assert so.nodes(np.zeros((4, 4), np.uint8)).shape == (0, 2) and so.nodes(edge).dtype == np.int32


def test_custom_table_and_values_outside_zero_one():
    rng = np.random.default_rng(5)
    img = ((rng.random((40, 37)) < 0.35) * rng.integers(1, 256, (40, 37))).astype(np.uint8)
    base, it = so.thin(img)
    assert np.array_equal(so.thin((img != 0).astype(np.uint8))[0], base)
    nothing = np.zeros(256, np.uint8)
    same, it0 = so.thin(img, nothing)
    assert it0 == 1 and np.array_equal(same, (img != 0).astype(np.uint8))
    table = rng.integers(0, 4, 256).astype(np.uint8)
    other, it1 = so.thin(img, table)
    assert it1 >= 1 and not np.any(other.astype(bool) & ~(img != 0)) and not np.array_equal(other, base)
