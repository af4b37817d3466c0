"""Edge shapes of the streaming kernels around the convolutions (csrc/groupnorm.hip, csrc/train_ops.hip, csrc/temb.hip) against
the fp64 restatements of tests/stream_oracle.py, through drivescenegen_amd.ops only.

The case tables below are module-level constants: tests/test_stream_oracle_cpu.py restates every kernel's branch selector as a
function of the shape and asserts that these tables reach every value of it.  A kernel that grows a branch must grow its table
(and the selector there).  Every tolerance is the existing one of the op (cited), derived in a comment, or measured against the
oracle with the measured value next to it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drivescenegen_amd import _lib, ops, synth  # noqa: E402
from tests import stream_oracle as so  # noqa: E402
from tests.common import max_abs, rel_l2  # noqa: E402

DEV = "cuda"
EPS = 1e-5
U24, U23, U22 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
MODES = ("bf16", "fp16")

# ---- case tables -------------------------------------------------------------------------------------------------------------
# GroupNorm forward, fp32 NCHW: (n, c0, c1, groups, h, w)
GN_FWD_CASES = [(3, 8, 0, 8, 3, 5),
                (1, 12, 20, 8, 7, 9),      # a group edge on the concat edge; groups wholly in source 1
                (2, 10, 6, 4, 4, 257),     # a straddling group; hw / 4 = 257
                (2, 32, 0, 1, 4, 4),
                (1, 8, 0, 2, 4, 513)]
GN_HARD_CASES = GN_FWD_CASES[:3]           # the same data shifted to group mean / std = 30 and 300
GN_HARD_RATIOS = (30.0, 300.0)
# one constant group (var = 0) per value of hw % 4: (n, c0, c1, groups, h, w)
GN_CONST_CASES = [(2, 8, 0, 2, 4, 4), (2, 8, 0, 2, 1, 5), (2, 8, 0, 2, 2, 3), (2, 8, 0, 2, 3, 5)]
# gn_scale_shift_from_parts: (c0, c1, groups, t0, t1), n = 2, 10 x 10 pixels
PARTS_N, PARTS_HW = 2, (10, 10)
PARTS_CASES = [(192, 0, 2, 1, 0),          # cpg 96 > 64: a lane owns two channels; run of 96 partials
               (12, 12, 4, 50, 3),         # runs of 300 (a second trip of the four-in-flight loop) and 18 partials; t0 != t1
               (8, 24, 4, 16, 20),         # groups wholly in one source; runs of 128 and 160
               (10, 6, 4, 7, 5)]           # a straddling group
PARTS_SLICED = (16, 0, 2, 256, 0, 16, 16)  # (c0, c1, groups, t0, t1, h, w): c * tiles = 4096 -> two slices of range_bound_kernel
# gn_channel_stats_blocked: ((n, c, h, w), splits)
STATS_BLK_CASES = [((2, 16, 9, 31), (1, 3, 9)), ((1, 8, 10, 103), (1, 2, 5))]
# GroupNorm backward, fp32: (n, c0, c1, groups, h, w) -> [(silu, fan-in form)]
FANIN = ("none", "add0", "add0+add0b", "add0+add1")
GNB_CASES = [(3, 8, 0, 8, 3, 5), (5, 10, 6, 4, 4, 257), (1, 8, 8, 2, 4, 513), (130, 8, 0, 2, 2, 2), (257, 8, 0, 2, 2, 2)]
GNB_VARIANTS = [[(True, "none"), (False, "add0+add0b"), (True, "add0")],
                [(True, "add0+add1"), (False, "none")],
                [(True, "add0+add0b"), (False, "add0+add1")],
                [(True, "add0"), (False, "none")],
                [(True, "none"), (False, "add0")]]
# GroupNorm backward, blocked 16-bit: (n, c0, c1, groups, h, w)
GNB_BLK_CASES = [(3, 8, 8, 2, 5, 7),
                 (1, 8, 8, 2, 10, 103),    # hw = 1030: the second x-block holds 6 pixels, loads clamped
                 (1, 8, 8, 2, 64, 64),     # splits = 2: the finalize pass adds the partials
                 (1, 8, 8, 2, 64, 128),    # splits = 4: sum_splits_kernel
                 (3, 16, 0, 4, 5, 7)]
GNB_BLK_VARIANTS = [(False, "none"), (True, "none"), (True, "add0"), (True, "add0+add0b"), (True, "add0+add1"), (False, "add0+add0b")]
# sums and linear layers
CSUM_CASES = [(3, 7, 9, 11), (2, 5, 4, 257), (1, 3, 1, 1)]
CSUM_BLK_CASES = [(2, 16, 5, 7), (2, 16, 32, 32), (2, 16, 10, 103), (2, 16, 13, 100)]   # hw = 35, 1024, 1030, 1300
ROWS_CASES = [(1, 300, 320), (8, 300, 320), (9, 300, 320)]                             # (n, c, stride)
LINEAR_BWD_CASES = [(1, 1, 1), (5, 31, 7), (9, 33, 100), (4, 64, 9)]                   # (n, in_f, out_f)
# (the issue's four cases all have out_f % 4 != 0; the fifth is the self-check's out_f % 4 == 0)
LINEAR_CASES = [(1, 1, 1), (8, 63, 3), (9, 65, 5), (17, 64, 6), (4, 32, 8)]            # (n, in_f, out_f)
TEMB_CASES = [(32, 100), (64, 256), (224, 512), (6, 300)]                              # (ch, dim)
TEMB_STEPS = ([0, 1, 499, 999], [37])
# elementwise, loss, optimiser
SILU_NUMELS = (1, 255, 257)
SILU_GRID = [0.0] + [s * v for v in (1e-8, 1.0, 10.0, 20.0, 50.0, 87.0, 88.8, 100.0, 1e4) for s in (1.0, -1.0)]
LOSS_CASES = [(1, 1), (1, 255), (5, 205), (3, 5000), (700, 11), (4, 3072), (4, 550000)]   # (n, per): numel 1, 255, 1025, 15000, ...
UNSCALE_NUMELS = (1, 1000, 5001)
ADAMW_NUMELS = (1, 257, 5001)
ADAMW_LRS = (1e-5, 1e-3)
ADAMW_WDS = (0.0, 1e-2)
FLAT_NUMELS = (1, 1023, 4097)
UPS_CASES = [(3, 1, 2), (2, 5, 6), (1, 3, 130)]     # (planes, h, w) of the small image
UPS_BLK_CASES = [(2, 3, 5), (2, 3, 6)]              # w = 5: sumpool2x2_blk_kernel, the odd-width fallback
ADD16_NUMELS = (8, 4104)


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _r(seed, shape, scale=1.0):
    return (synth.normal(seed, shape) * float(scale)).astype(np.float32)


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().float().numpy() if t.dtype in (torch.bfloat16, torch.float16) else t.detach().cpu().numpy()


def _check(got, want, tol_rel, tol_abs):
    """tests/test_gpu_ops.py's _check: rel-L2 and max-abs scaled by max(1, max|want|)"""
    got, want = torch.from_numpy(np.asarray(got)), torch.from_numpy(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all()
    assert rel_l2(got, want) <= tol_rel, rel_l2(got, want)
    assert max_abs(got, want) <= tol_abs * max(1.0, float(want.abs().max())), max_abs(got, want)


def _close(got, want, rel=2e-5, ab=2e-5):
    """tests/test_gpu_train_ops.py's _close (the same form, its defaults)"""
    _check(got, want, rel, ab)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gn_inputs(case, seed):
    """N(0, 1) * 1.3 + 0.7 * per-channel + 1.5, as test_gpu_gnb._case; gamma, beta"""
    n, c0, c1, groups, h, w = case
    c = c0 + c1
    x = _r(seed, (n, c, h, w), 1.3) + 0.7 * _r(seed + 1, (1, c, 1, 1)) + np.float32(1.5)
    return x.astype(np.float32), 1 + _r(seed + 4, (c,), 0.2), _r(seed + 5, (c,), 0.2)


def _srcs(x, c0):
    return np.ascontiguousarray(x[:, :c0]), (np.ascontiguousarray(x[:, c0:]) if x.shape[1] > c0 else None)


def _gn_bound(f, beta):
    """B = 2^-24 * (|x * sc| + |mean * sc| + |beta| + |y|) elementwise, from the oracle's fp64 tables"""
    sc, mean = f["scale"][..., None], f["mean"][..., None]
    return U24 * (np.abs(f["x"] * sc) + np.abs(mean * sc) + np.abs(so.f64(beta))[None, :, None] + np.abs(f["y"]))


def _gn_run(x, c0, gamma, beta, groups, silu):
    """(scale_shift, mean_rstd, y) of the fp32 kernels on [N, C, H, W] numpy data"""
    x0, x1 = _srcs(x, c0)
    ss = ops.gn_scale_shift(_dev(x0), _dev(gamma), _dev(beta), groups, EPS, src1=_dev(x1))
    ss_t, mr = ops.gn_scale_shift_train(_dev(x0), _dev(gamma), _dev(beta), groups, EPS, src1=_dev(x1))
    assert torch.equal(ss, ss_t)                    # one finalize kernel with and without the mean_rstd output
    y = ops.gn_apply(_dev(x), ss, silu)
    n, c = x.shape[:2]
    return _np(ss), _np(mr), _np(y).reshape(n, c, -1)


def _check_mean_rstd(mr, f):
    # (float) of an fp64 value: half an ulp = 2^-24 relative; the fp64 raw moments' cancellation at the ratios used here is
    # 1e-16 * (mean / std)^2 <= 1e-11 -- 2^-23 is the issue's bound
    assert (np.abs(mr[..., 0] - f["mean"]) <= U23 * np.abs(f["mean"])).all(), float(np.abs(mr[..., 0] - f["mean"]).max())
    assert (np.abs(mr[..., 1] - f["rstd"]) <= U23 * f["rstd"]).all(), float(np.abs(mr[..., 1] - f["rstd"]).max())


# ---- GroupNorm forward, fp32 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [False, True], ids=["affine", "silu"])
@pytest.mark.parametrize("case", GN_FWD_CASES, ids=lambda c: "n%d_c%d+%d_g%d_%dx%d" % c)
def test_groupnorm_forward_fp32(case, silu):
    x, gamma, beta = _gn_inputs(case, seed=100 + sum(case))
    x0, x1 = _srcs(x, case[1])
    f = so.gn_forward(x0, gamma, beta, case[3], src1=x1, silu_on=silu)
    ss, mr, y = _gn_run(x, case[1], gamma, beta, case[3], silu)
    _check_mean_rstd(mr, f)
    _check(y, f["y"], tol_rel=2e-6, tol_abs=5e-6)          # test_gpu_ops.test_groupnorm's tolerances


@pytest.mark.parametrize("case", GN_CONST_CASES, ids=lambda c: "hw%d" % (c[4] * c[5]))
def test_groupnorm_forward_constant_group(case):
    """var = 0 must not go negative: a constant group comes out as beta, finite (one case per value of hw % 4)"""
    n, c0, c1, groups, h, w = case
    x, gamma, beta = _gn_inputs(case, seed=150 + h * w)
    cpg = (c0 + c1) // groups
    x[:, :cpg] = np.float32(1.7)                            # group 0 of every image is constant
    f = so.gn_forward(x, gamma, beta, groups)
    ss, mr, y = _gn_run(x, c0, gamma, beta, groups, False)
    assert np.isfinite(ss).all() and np.isfinite(mr).all() and np.isfinite(y).all()
    bound = _gn_bound(f, beta)
    err = np.abs(y[:, :cpg] - so.f64(beta)[None, :cpg, None])
    assert (err <= 4 * bound[:, :cpg]).all(), float((err / bound[:, :cpg]).max())
    assert (np.abs(y - f["y"]) <= 4 * bound).all()


@pytest.mark.parametrize("ratio", GN_HARD_RATIOS)
@pytest.mark.parametrize("case", GN_HARD_CASES, ids=lambda c: "n%d_c%d+%d_g%d_%dx%d" % c)
def test_groupnorm_forward_hard_numerics(case, ratio):
    """Group mean / std of 30 and 300: |got - fp64| <= 4 * B elementwise, B = 2^-24 * (|x sc| + |mean sc| + |beta| + |y|).
    The 4: the largest count of half-ulp roundings on one term (rstd, sc, mean_f and their product); the fp32 emulation of the
    kernel's formula in test_stream_oracle_cpu.py stays below 1.3 * B, measured on the GPU: 0.84 * B at the worst."""
    n, c0, c1, groups, h, w = case
    x, gamma, beta = _gn_inputs(case, seed=100 + sum(case))
    f0 = so.gn_forward(x, gamma, beta, groups)
    std = 1.0 / f0["rstd"]                                 # (eps is 1e-5 beside a variance of 2)
    x = (x.astype(np.float64) + (ratio * std - f0["mean"])[:, :, None, None]).astype(np.float32)
    f = so.gn_forward(x, gamma, beta, groups)
    assert np.allclose(f["mean"] * f["rstd"], ratio, rtol=1e-3)
    ss, mr, y = _gn_run(x, c0, gamma, beta, groups, False)
    _check_mean_rstd(mr, f)
    worst = float((np.abs(y - f["y"]) / _gn_bound(f, beta)).max())
    print(f"gn hard numerics {case} ratio {ratio:g}: max |err| / B = {worst:.3f}")
    assert worst <= 4.0, worst


# ---- gn_scale_shift_from_parts(_train), the bound ------------------------------------------------------------------------------
def _float_of_bits(t):
    return t.cpu().view(torch.float32).numpy()


def _parts_tables(c0, c1, t0, t1, h, w, seed):
    x = _r(seed, (PARTS_N, c0 + c1, h, w), 1.3) + 0.7 * _r(seed + 1, (1, c0 + c1, 1, 1)) + np.float32(1.5)
    x0, x1 = _srcs(x.astype(np.float32), c0)
    return x0, x1, so.split_stats(x0, t0), (so.split_stats(x1, t1) if c1 else None)


def _check_parts(c0, c1, groups, t0, t1, h, w, seed):
    x0, x1, st0, st1 = _parts_tables(c0, c1, t0, t1, h, w, seed)
    c = c0 + c1
    gamma, beta = 1 + _r(seed + 4, (c,), 0.2), _r(seed + 5, (c,), 0.2)
    f = so.gn_from_parts(st0, gamma, beta, groups, h * w, stats1=st1)
    args = (_dev(st0), _dev(gamma), _dev(beta), groups, EPS, h * w)
    ss = ops.gn_scale_shift_from_parts(*args, stats1=_dev(st1))
    ss_t, mr = ops.gn_scale_shift_from_parts_train(*args, stats1=_dev(st1))
    ss_b, bound = ops.gn_scale_shift_from_parts_bound(*args, stats1=_dev(st1))
    assert torch.equal(ss, ss_t) and torch.equal(ss, ss_b)   # one kernel, three sets of outputs
    ss, mr = _np(ss), _np(mr)
    _check_mean_rstd(mr, f)
    # scale = fl(fl(rstd) * gamma): two half-ulp roundings, 2 * 2^-24 relative to first order -> 3 * 2^-24
    assert (np.abs(ss[..., 0] - f["scale"]) <= 3 * U24 * np.abs(f["scale"])).all()
    # shift = fl(beta - fl(mean_f * sc)): mean_f, sc (two), the product and the difference: <= 4 * 2^-24 * (|mean sc| + |beta|)
    lim = 4 * U24 * (np.abs(f["mean"] * f["scale"]) + np.abs(so.f64(beta))[None, :])
    assert (np.abs(ss[..., 1] - f["shift"]) <= lim).all(), float((np.abs(ss[..., 1] - f["shift"]) / lim).max())
    # the bound: >= max|x| of the tensors behind the tables, <= fl(sqrt(fl(largest per-tile sum of squares))) plus one ulp
    xmax = np.abs(x0).reshape(PARTS_N, -1).max(1)
    sq = st0[..., 1].reshape(PARTS_N, -1).max(1)
    if c1:
        xmax = np.maximum(xmax, np.abs(x1).reshape(PARTS_N, -1).max(1))
        sq = np.maximum(sq, st1[..., 1].reshape(PARTS_N, -1).max(1))
    top = np.nextafter(np.sqrt(sq.astype(np.float32)), np.float32(np.inf))
    rb = ops.range_bound_from_stats(_dev(st0))
    if c1:
        rb = ops.range_bound_from_stats(_dev(st1), bound=rb)
    for got in (_float_of_bits(bound), _float_of_bits(rb)):
        assert (got >= xmax).all() and (got <= top).all(), (got, xmax, top)


@pytest.mark.parametrize("case", PARTS_CASES, ids=lambda c: "c%d+%d_g%d_t%d_%d" % c)
def test_groupnorm_finalize_from_parts_and_bound(case):
    _check_parts(*case, *PARTS_HW, seed=200 + sum(case))


def test_groupnorm_bound_with_more_than_one_slice():
    """c * tiles = 4096: range_bound_kernel runs two slices per image; one pixel per tile, so the bound is max|x| to an ulp"""
    _check_parts(*PARTS_SLICED, seed=260)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", STATS_BLK_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_channel_stats_blocked(case, mode):
    (n, c, h, w), all_splits = case
    x = so.ROUND[mode](_r(300 + h, (n, c, h, w), 1.3) + np.float32(0.4))
    xb = _dev(so.to_blocked(x), TDT.get(mode))
    for splits in all_splits:
        st = ops.gn_channel_stats_blocked(xb, splits).cpu()
        assert st.shape == (n, c, splits, 2)
        runs = so.f64(x).reshape(n, c, splits, -1)            # a split is a run of hw / splits consecutive pixels
        ref = torch.from_numpy(np.stack([runs.sum(3), (runs ** 2).sum(3)], -1))
        assert torch.allclose(st, ref, rtol=1e-12, atol=1e-12), float((st - ref).abs().max())   # test_gpu_ops' blocked-stats bound


# ---- GroupNorm backward ----------------------------------------------------------------------------------------------------------
def _prefill(c):
    return (0.25 + 0.125 * (np.arange(c) % 5)).astype(np.float32)      # exact in every type: dgamma / dbeta must be added to


_gnb_cache = {}


def _gnb_case(case, mode="fp32"):
    """inputs (as stored in `mode`) and the fp64 closed-form gradients with and without SiLU: computed once per case, unchanged"""
    key = (case, mode)
    if key not in _gnb_cache:
        n, c0, c1, groups, h, w = case
        seed = 400 + sum(case)
        rnd = so.ROUND[mode]
        x, gamma, beta = _gn_inputs(case, seed)
        x = rnd(x)
        dy = rnd(_r(seed + 2, x.shape))
        adds = {k: rnd(_r(seed + 6 + i, (n, cc, h, w), 0.5)) for i, (k, cc) in enumerate((("add0", c0), ("add0b", c0), ("add1", c1))) if cc}
        x0, x1 = _srcs(x, c0)
        ref = {s: so.gn_backward(x0, dy, gamma, beta, groups, src1=x1, silu_on=s) for s in (False, True)}
        _gnb_cache[key] = (x0, x1, dy, gamma, beta, adds, ref)
    return _gnb_cache[key]


def _fanin(adds, form, c0, c1, shape_hw):
    """the addends of a fan-in form and their fp64 sum over cat(src0, src1)"""
    use = {"none": (), "add0": ("add0",), "add0+add0b": ("add0", "add0b"), "add0+add1": ("add0", "add1")}[form]
    if "add1" in use and not c1:
        use = ("add0",)
    n = next(iter(adds.values())).shape[0]
    tot = np.zeros((n, c0 + c1, shape_hw), dtype=np.float64)
    for k in use:
        a = so.f64(adds[k]).reshape(n, -1, shape_hw)
        if k == "add1":
            tot[:, c0:] += a
        else:
            tot[:, :c0] += a
    return {k: adds[k] for k in use}, tot


@pytest.mark.parametrize("idx", range(len(GNB_CASES)), ids=["n%d_c%d+%d_g%d_%dx%d" % c for c in GNB_CASES])
def test_groupnorm_backward_fp32(idx):
    case = GNB_CASES[idx]
    n, c0, c1, groups, h, w = case
    c, hw = c0 + c1, h * w
    x0, x1, dy, gamma, beta, adds, ref = _gnb_case(case)
    d0, d1, ddy, dgam = _dev(x0), _dev(x1), _dev(dy), _dev(gamma)
    dadds = {k: _dev(v) for k, v in adds.items()}
    ss, mr = ops.gn_scale_shift_train(d0, dgam, _dev(beta), groups, EPS, src1=d1)
    pg, pb = _prefill(c), _prefill(c)[::-1].copy()
    for silu, form in GNB_VARIANTS[idx]:
        use, tot = _fanin(adds, form, c0, c1, hw)
        dg, db = _dev(pg), _dev(pb)
        dx0, dx1 = ops.gn_bwd(d0, ddy, ss, mr, dgam, groups, silu, dg, db, src1=d1, **{k: dadds[k] for k in use})
        dx = np.concatenate([_np(t).reshape(n, -1, hw) for t in (dx0, dx1) if t is not None], 1)
        want_dx, want_dg, want_db = ref[silu]
        # tests/test_gpu_train_ops.test_groupnorm_backward's tolerances; dgamma / dbeta: what the call added to the prefill
        _close(dx, want_dx + tot, rel=2e-5, ab=2e-5)
        _close(so.f64(_np(dg)) - pg, want_dg, rel=2e-5, ab=1e-4)
        _close(so.f64(_np(db)) - pb, want_db, rel=2e-5, ab=1e-4)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", GNB_BLK_CASES, ids=lambda c: "n%d_c%d+%d_g%d_%dx%d" % c)
def test_groupnorm_backward_blocked(case, mode):
    n, c0, c1, groups, h, w = case
    c, hw = c0 + c1, h * w
    x0, x1, dy, gamma, beta, adds, ref = _gnb_case(case, mode)
    blk = lambda a: None if a is None else _dev(so.to_blocked(a), TDT[mode])
    d0, d1, ddy, dgam = _dev(x0), _dev(x1), _dev(dy), _dev(gamma)
    b0, b1, bdy = blk(x0), blk(x1), blk(dy)
    badds = {k: blk(v) for k, v in adds.items()}
    ss, mr = ops.gn_scale_shift_train(d0, dgam, _dev(beta), groups, EPS, src1=d1)
    ulp = 2.0 ** -8 if mode == "bf16" else 2.0 ** -11
    pg, pb = _prefill(c), _prefill(c)[::-1].copy()
    added = lambda t, pre: torch.from_numpy(so.f64(_np(t)) - pre)
    tape32 = {}
    for silu in (False, True):     # the fp32-tape kernel on the same stored operands (the fan-in does not enter dgamma / dbeta)
        dg32, db32 = _dev(pg), _dev(pb)
        ops.gn_bwd(d0, ddy, ss, mr, dgam, groups, silu, dg32, db32, src1=d1)
        tape32[silu] = (added(dg32, pg), added(db32, pb))
    for silu, form in GNB_BLK_VARIANTS:
        use, tot = _fanin(adds, form, c0, c1, hw)
        dg, db = _dev(pg), _dev(pb)
        g0, g1 = ops.gn_bwd_blocked(b0, bdy, ss, mr, dgam, groups, silu, dg, db, src1=b1, **{k: badds[k] for k in use})
        assert g0.dtype == TDT[mode]
        dx = np.concatenate([so.from_blocked(_np(t)).reshape(n, -1, hw) for t in (g0, g1) if t is not None], 1)
        want_dx, want_dg, want_db = ref[silu]
        want_dx = want_dx + tot
        # 1e-5 against the fp32 tape: test_streaming_backward_ops_blocked16; 5e-5 against fp64: test_gpu_gnb
        assert rel_l2(added(dg, pg), tape32[silu][0]) <= 1e-5 and rel_l2(added(db, pb), tape32[silu][1]) <= 1e-5
        assert rel_l2(added(dg, pg), torch.from_numpy(want_dg)) <= 5e-5 and rel_l2(added(db, pb), torch.from_numpy(want_db)) <= 5e-5
        # dx: one rounding of the 16-bit result (test_streaming_backward_ops_blocked16's rel-L2) ...
        assert np.isfinite(dx).all()
        assert rel_l2(torch.from_numpy(dx), torch.from_numpy(want_dx)) <= (4e-3 if mode == "bf16" else 6e-4)
        # ... and elementwise one ulp of the stored type plus the fp32 tape's absolute class (2e-5 * max|ref|, its `ab`)
        lim = ulp * np.abs(want_dx) + 2e-5 * np.abs(want_dx).max()
        assert (np.abs(dx - want_dx) <= lim).all(), float((np.abs(dx - want_dx) / lim).max())


def test_second_fan_in_term_needs_the_first():
    """add0b without add0 is an argument refusal (DsgError) on both tapes, before any launch"""
    case = GNB_BLK_CASES[0]
    n, c0, c1, groups, h, w = case
    c = c0 + c1
    x0, x1, dy, gamma, beta, adds, _ = _gnb_case(case, "bf16")
    ss, mr = ops.gn_scale_shift_train(_dev(x0), _dev(gamma), _dev(beta), groups, EPS, src1=_dev(x1))
    dg, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    with pytest.raises(_lib.DsgError):
        ops.gn_bwd(_dev(x0), _dev(dy), ss, mr, _dev(gamma), groups, True, dg, db, src1=_dev(x1), add0b=_dev(adds["add0b"]))
    blk = lambda a: _dev(so.to_blocked(a), torch.bfloat16)
    with pytest.raises(_lib.DsgError):
        ops.gn_bwd_blocked(blk(x0), blk(dy), ss, mr, _dev(gamma), groups, True, dg, db, src1=blk(x1), add0b=blk(adds["add0b"]))
    assert not dg.any() and not db.any()


# ---- sums and linear layers ----------------------------------------------------------------------------------------------------
def _check_channel_sums(xdev, x, n, c):
    """into columns [2, 2 + c) of a wider matrix whose other columns keep their sentinel.  8 * 2^-24 * sum|x| per channel: a
    thread's fp32 partial sums hold at most six terms (five roundings) before the fp64 tree, the result is rounded once (six)"""
    wide = torch.full((n, c + 5), 7.0, device=DEV)
    out = ops.channel_sums(xdev, out=wide[:, 2:2 + c])
    assert out.data_ptr() == wide[:, 2:2 + c].data_ptr()
    got = wide.cpu().numpy()
    assert (got[:, :2] == 7.0).all() and (got[:, 2 + c:] == 7.0).all()
    want, mag = so.channel_sums(x)
    assert (np.abs(got[:, 2:2 + c] - want) <= 8 * U24 * mag).all(), float((np.abs(got[:, 2:2 + c] - want) / (U24 * mag)).max())
    assert torch.equal(ops.channel_sums(xdev), wide[:, 2:2 + c])      # the plain call: the same sums, its own matrix


@pytest.mark.parametrize("shape", CSUM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_channel_sums_fp32(shape):
    x = _r(500 + shape[3], shape) + np.float32(0.3)
    _check_channel_sums(_dev(x), x, shape[0], shape[1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", CSUM_BLK_CASES, ids=lambda s: "hw%d" % (s[2] * s[3]))
def test_channel_sums_blocked(shape, mode):
    x = so.ROUND[mode](_r(520 + shape[3], shape) + np.float32(0.3))
    _check_channel_sums(_dev(so.to_blocked(x), TDT[mode]), x, shape[0], shape[1])


@pytest.mark.parametrize("case", ROWS_CASES, ids=lambda c: "n%d" % c[0])
def test_reduce_rows_add(case):
    n, c, stride = case
    src = _r(540 + n, (n, stride))
    dst0 = _r(541, (c,), 2.0)
    sdev, dst = _dev(src), _dev(dst0)
    ops.reduce_rows_add(sdev[:, :c], dst)
    s = so.f64(src)[:, :c].sum(0)
    # fp64 sum over the rows, rounded to fp32 (2^-24 |s|), added to dst in fp32 (2^-24 |dst + s|): <= 2^-23 * (|s| + |dst|)
    assert (np.abs(_np(dst) - (dst0 + s)) <= U23 * (np.abs(s) + np.abs(dst0))).all()


@pytest.mark.parametrize("case", LINEAR_BWD_CASES, ids=lambda c: "n%d_in%d_out%d" % c)
def test_linear_backward(case):
    n, in_f, out_f = case
    x, w = _r(560 + n, (n, in_f)), _r(561, (out_f, in_f), 0.2)
    dyw = _r(562, (n, out_f + 5))                                   # dy = columns [2, 2 + out_f): dy_stride > out_f
    dy = dyw[:, 2:2 + out_f]
    want_dx, want_dw, want_db = so.linear_bwd(x, w, dy)
    pw, pb = _r(563, (out_f, in_f), 0.5), _r(564, (out_f,), 0.5)
    xd, wd, dyd = _dev(x), _dev(w), _dev(dyw)[:, 2:2 + out_f]
    dw, db = _dev(pw), _dev(pb)
    dx = ops.linear_bwd(xd, wd, dyd, dw, db)
    # tests/test_gpu_train_ops.test_linear_silu_backward_and_sums' _close defaults; dw / db: what the call added
    _close(_np(dx), want_dx)
    _close(so.f64(_np(dw)) - pw, want_dw)
    _close(so.f64(_np(db)) - pb, want_db)
    # a call without one of the outputs writes the others only
    dw1, db1 = dw.clone(), db.clone()
    dx2 = ops.linear_bwd(xd, wd, dyd, None, db)
    assert torch.equal(dw, dw1) and torch.equal(dx2, dx)
    _close(so.f64(_np(db)) - pb, 2 * want_db)
    db2 = db.clone()
    ops.linear_bwd(xd, wd, dyd, dw, None)
    assert torch.equal(db, db2)
    _close(so.f64(_np(dw)) - pw, 2 * want_dw)
    dw2, dx1 = dw.clone(), dx.clone()
    assert ops.linear_bwd(xd, wd, dyd, None, db, need_dx=False) is None
    assert torch.equal(dw, dw2) and torch.equal(dx, dx1)
    _close(so.f64(_np(db)) - pb, 3 * want_db)


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "n%d_in%d_out%d" % c)
def test_linear_forward(case):
    n, in_f, out_f = case
    x, w, b = _r(580 + n, (n, in_f)), _r(581, (out_f, in_f), 1.0 / np.sqrt(in_f)), _r(582, (out_f,), 0.1)
    # tests/test_gpu_ops.test_time_embedding_and_proj's tolerances
    _check(_np(ops.linear(_dev(x), _dev(w), _dev(b))), so.linear(x, w, b), tol_rel=2e-6, tol_abs=5e-6)
    if in_f == 65:
        _check(_np(ops.linear(_dev(x), _dev(w))), so.linear(x, w), tol_rel=2e-6, tol_abs=5e-6)


@pytest.mark.parametrize("steps", TEMB_STEPS, ids=["batch4", "batch1"])
@pytest.mark.parametrize("case", TEMB_CASES, ids=lambda c: "ch%d_dim%d" % c)
def test_time_embedding(case, steps):
    ch, dim = case
    t = torch.tensor(steps, dtype=torch.long)
    w1, b1 = _r(600 + ch, (dim, ch), 1.0 / np.sqrt(ch)), _r(601, (dim,), 0.1)
    w2, b2 = _r(602, (dim, dim), 1.0 / np.sqrt(dim)), _r(603, (dim,), 0.1)
    freqs = ops.sinusoid_freqs(ch)
    want = so.time_embed(t.numpy(), freqs.numpy(), w1, b1, w2, b2)
    args = (t.to(DEV), _dev(w1), _dev(b1), _dev(w2), _dev(b2))
    act, emb, z1, z2 = ops.time_embed_train(*args, freqs.to(DEV))
    # cosf / sinf: <= 2 ulp (HIP's documented bound) of values <= 1 -> 2^-22 absolute, against fp64 of the same fp32 angle
    assert float(np.abs(_np(emb) - want["emb"]).max()) <= U22, float(np.abs(_np(emb) - want["emb"]).max())
    for got, key in ((z1, "z1"), (z2, "z2"), (act, "act")):
        _check(_np(got), want[key], tol_rel=2e-6, tol_abs=5e-6)    # test_time_embedding_and_proj's tolerances
    assert torch.equal(ops.time_embed(*args), act)                  # the plain call (its own freqs table): the same bits
    assert torch.equal(ops.time_embed(*args, freqs=freqs.to(DEV)), act)


# ---- elementwise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numel", SILU_NUMELS)
def test_silu_forward_backward_over_the_range(numel):
    z = np.resize(np.array(SILU_GRID, dtype=np.float32), numel)
    dy = _r(620 + numel, (numel,))
    y, dz = _np(ops.silu_fwd(_dev(z))), _np(ops.silu_bwd(_dev(z), _dev(dy)))
    assert np.isfinite(y).all() and np.isfinite(dz).all()
    _close(y, so.silu(z))                                            # test_gpu_train_ops' _close defaults
    _close(dz, so.f64(dy) * so.dsilu(z))
    # max|want| is 1e4 on this grid, so next to it every element on its own.  silu_f: expf and an IEEE division, a few ulp.
    # dsilu: the hardware exp2 of z * log2(e), whose rounding (2^-24 * 128 at |z| <= 88.8) is 5.3e-6 relative in the result, plus
    # the hardware reciprocal's ulp: 2e-5 leaves 3x.  1e-30: results below fp32's normal range may come out as 0.
    for got, want in ((y, so.silu(z)), (dz, so.f64(dy) * so.dsilu(z))):
        assert (np.abs(got - want) <= 2e-5 * np.abs(want) + 1e-30).all(), float(np.abs(got - want).max())


def _loss_inputs(n, per):
    pred, tgt = _r(640 + n, (n, per)), _r(641 + n, (n, per))
    wts = (0.25 + np.abs(_r(642 + n, (n,)))).astype(np.float32)
    if n > 1:
        wts[n // 2] = 0.0
    return pred, tgt, wts


@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: "n%d_per%d" % c)
def test_losses_and_norm(case):
    """1e-6 relative on the loss, _close(rel=1e-6, ab=1e-7) on the gradient: test_mse_norm_adamw_match_torch's values (fp64
    accumulation, one rounding of the result: 2^-24; the gradient is two or three fp32 roundings of an O(1 / numel) value)"""
    n, per = case
    pred, tgt, wts = _loss_inputs(n, per)
    pd, td = _dev(pred), _dev(tgt)
    gs = 128.0 if n == 3 else 1.0
    loss, grad = ops.mse_loss(pd, td, grad_scale=gs)
    want_l, want_g = so.mse(pred, tgt, gs)
    assert abs(float(loss.cpu()) - want_l) <= 1e-6 * want_l
    _close(_np(grad), want_g, rel=1e-6, ab=1e-7)
    lw, gw = ops.mse_loss_weighted(pd, td, _dev(wts), grad_scale=gs)
    want_lw, want_gw = so.mse_weighted(pred, tgt, wts, gs)
    assert abs(float(lw.cpu()) - want_lw) <= 1e-6 * want_lw
    _close(_np(gw), want_gw, rel=1e-6, ab=1e-7)
    # all-ones weights: mse_loss's bits
    l1, g1 = ops.mse_loss_weighted(pd, td, torch.ones(n, device=DEV), grad_scale=gs)
    assert torch.equal(l1, loss) and torch.equal(g1, grad)
    # without the gradient: the same loss
    l0, g0 = ops.mse_loss(pd, td, need_grad=False)
    assert g0 is None and abs(float(l0.cpu()) - want_l) <= 1e-6 * want_l
    l0w, g0w = ops.mse_loss_weighted(pd, td, _dev(wts), need_grad=False)
    assert g0w is None and torch.equal(l0w, lw)
    want_n = so.l2_norm(pred)
    assert abs(float(ops.l2_norm(pd).cpu()) - want_n) <= 1e-6 * want_n


@pytest.mark.parametrize("numel", UNSCALE_NUMELS)
def test_unscale_check(numel):
    """found_inf is torch's rule: an element non-finite BEFORE scaling; g comes back as g * inv bitwise"""
    base = _r(660 + numel, (numel,), 3.0)
    spots = sorted({0, numel - 1, min(63 + 64 * (numel // 128), numel - 1)})
    inv = 1.0 / 1024.0

    def run(g0, inv_scale, found0):
        g, found = _dev(g0), torch.full((1,), found0, dtype=torch.int32, device=DEV)
        assert ops.unscale_check_(g, inv_scale, found) is g
        want, want_found = so.unscale_check_f32(g0, inv_scale, found0)
        got = _np(g)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(_bits(got)[~np.isnan(want)], _bits(want)[~np.isnan(want)])
        assert int(found.cpu()) == want_found
        return want_found

    for bad in (np.inf, -np.inf, np.nan):
        for at in spots:
            g0 = base.copy()
            g0[at] = bad
            assert run(g0, inv, 0) == 1
    assert run(base, inv, 0) == 0
    assert run(base, inv, 1) == 1                    # a flag that is already up stays up
    big = base.copy()
    big[numel - 1] = np.float32(3e38)                # finite, and its product with 2 is not: torch does not flag that
    assert run(big, 2.0, 0) == 0


@pytest.mark.parametrize("numel", UNSCALE_NUMELS)
def test_clip_scale(numel):
    g0 = _r(680 + numel, (numel,), 3.0)
    g0[0] = np.float32(2.5)                          # (norm > 1 at numel 1 too)
    g = _dev(g0)
    norm = ops.l2_norm(g)
    nf = float(norm.cpu())
    assert ops.clip_scale_(g, norm, 2.0 * nf + 1.0) is g and np.array_equal(_bits(_np(g)), _bits(g0))   # below max_norm: untouched
    cf = so.clip_factor_f32(np.float32(nf), 1.0)
    assert cf < 1
    ops.clip_scale_(g, norm, 1.0)
    assert np.array_equal(_bits(_np(g)), _bits(g0 * cf))


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("wd", ADAMW_WDS)
@pytest.mark.parametrize("lr", ADAMW_LRS)
def test_adamw_three_steps(lr, wd, clip):
    """p, exp_avg and exp_avg_sq against torch.optim.AdamW on the CPU, each at test_mse_norm_adamw_match_torch's rel=1e-6, ab=1e-6"""
    for numel in ADAMW_NUMELS:
        p_ref = torch.nn.Parameter(torch.from_numpy(_r(700 + numel, (numel,))))
        opt = torch.optim.AdamW([p_ref], lr=lr, weight_decay=wd)
        p = p_ref.detach().clone().to(DEV)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for step in range(1, 4):
            g = torch.from_numpy(_r(710 + step, (numel,), 3.0))
            p_ref.grad = g.clone()
            if clip:
                torch.nn.utils.clip_grad_norm_([p_ref], 1.0)
            opt.step()
            gd = g.to(DEV)
            ops.adamw_step_(p, gd, m, v, step, lr=lr, weight_decay=wd, total_norm=ops.l2_norm(gd) if clip else None, max_norm=1.0)
            st = opt.state[p_ref]
            for got, want in ((p, p_ref.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                _close(_np(got), want.numpy(), rel=1e-6, ab=1e-6)


@pytest.mark.parametrize("numel", FLAT_NUMELS)
def test_add_and_scale_bitwise(numel):
    a, b = _r(720 + numel, (numel,)), _r(721 + numel, (numel,))
    assert np.array_equal(_bits(_np(ops.add(_dev(a), _dev(b)))), _bits(a + b))
    x = _dev(a)
    assert np.array_equal(_bits(_np(ops.scale(x, mult=0.3))), _bits(a * (np.float32(1.0) * np.float32(0.3))))
    alpha = np.float32(1.0 / 3.0)
    al = _dev(np.array([alpha], dtype=np.float32))
    want = a * (alpha * np.float32(0.75))
    assert np.array_equal(_bits(_np(ops.scale(x, al, mult=0.75))), _bits(want))
    assert np.array_equal(_bits(_np(x)), _bits(a))                  # (the source is read only)
    assert ops.scale(x, al, mult=0.75, out=x) is x and np.array_equal(_bits(_np(x)), _bits(want))   # in place


@pytest.mark.parametrize("case", UPS_CASES, ids=lambda c: "p%d_%dx%d" % c)
def test_upsample_and_sumpool_fp32(case):
    planes, h, w = case
    x = _r(740 + w, (1, planes, h, w))
    assert np.array_equal(_bits(_np(ops.upsample_nearest2x(_dev(x)))), _bits(so.upsample_nearest2x(x)))
    g, a = _r(741 + w, (1, planes, 2 * h, 2 * w)), _r(742 + w, (1, planes, h, w))
    # atol 2e-6: tests/test_gpu_train_ops.test_upsample_and_its_adjoint
    assert float(np.abs(_np(ops.sumpool2x2(_dev(g))) - so.sumpool2x2(g)).max()) <= 2e-6
    assert float(np.abs(_np(ops.sumpool2x2(_dev(g), add=_dev(a))) - so.sumpool2x2(g, a)).max()) <= 2e-6


def test_upsample_and_sumpool_fp32_refuse_an_odd_width():
    with pytest.raises(_lib.DsgError):
        ops.upsample_nearest2x(_dev(_r(760, (1, 2, 2, 3))))
    with pytest.raises(_lib.DsgError):
        ops.sumpool2x2(_dev(_r(761, (1, 2, 4, 6))))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", UPS_BLK_CASES, ids=lambda c: "p%d_%dx%d" % c)
def test_upsample_and_sumpool_blocked(case, mode):
    """bitwise: the copy, and fp32 (a + b) + (c + d), + add, rounded once to the stored type"""
    planes, h, w = case
    rnd, ax = so.ROUND[mode], (-3, -2)
    x = rnd(_r(780 + w, (1, planes, h, w, 8)))
    up = ops.upsample_nearest2x(_dev(x, TDT[mode]))
    assert up.dtype == TDT[mode] and np.array_equal(_bits(_np(up)), _bits(so.upsample_nearest2x(x, ax)))
    g, a = rnd(_r(781 + w, (1, planes, 2 * h, 2 * w, 8))), rnd(_r(782 + w, (1, planes, h, w, 8)))
    assert np.array_equal(_bits(_np(ops.sumpool2x2(_dev(g, TDT[mode])))), _bits(rnd(so.sumpool2x2_f32(g, axes=ax))))
    got = ops.sumpool2x2(_dev(g, TDT[mode]), add=_dev(a, TDT[mode]))
    assert np.array_equal(_bits(_np(got)), _bits(rnd(so.sumpool2x2_f32(g, a, axes=ax))))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("numel", ADD16_NUMELS)
def test_add_16bit_is_the_rounded_fp32_sum(numel, mode):
    rnd = so.ROUND[mode]
    a, b = rnd(_r(800 + numel, (numel,))), rnd(_r(801 + numel, (numel,)))
    got = ops.add(_dev(a, TDT[mode]), _dev(b, TDT[mode]))
    assert got.dtype == TDT[mode] and np.array_equal(_bits(_np(got)), _bits(rnd(a + b)))
