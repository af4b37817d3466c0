"""tests/stream_oracle.py against torch fp64, and the path-coverage self-check of tests/test_gpu_stream_edges.py's case tables:
every branch selector of the streaming kernels, restated here as a pure function of the shape, must take each of its values on
at least one case.  A kernel that grows a branch grows its selector here and its table there.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from drivescenegen_amd import synth
from tests import stream_oracle as so
from tests import test_gpu_stream_edges as T


def _r(seed, shape, scale=1.0):
    return (synth.normal(seed, shape) * float(scale)).astype(np.float32)


# ---- the oracle itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("case", [T.GNB_CASES[0], T.GNB_CASES[1], T.GNB_BLK_CASES[0]], ids=lambda c: "n%d_c%d+%d_g%d_%dx%d" % c)
def test_closed_form_groupnorm_equals_fp64_autograd(case, silu):
    n, c0, c1, groups, h, w = case
    x, gamma, beta = T._gn_inputs(case, seed=7)
    dy = _r(9, x.shape)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    g64, b64 = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    y = F.group_norm(x64, groups, g64, b64, so.EPS_GN)
    y = F.silu(y) if silu else y
    (y * torch.from_numpy(dy).double()).sum().backward()
    x0, x1 = T._srcs(x, c0)
    f = so.gn_forward(x0, gamma, beta, groups, src1=x1, silu_on=silu)
    dx, dg, db = so.gn_backward(x0, dy, gamma, beta, groups, src1=x1, silu_on=silu)
    for got, want in ((f["y"], y.detach()), (dx, x64.grad), (dg, g64.grad), (db, b64.grad)):
        want = want.numpy().reshape(got.shape)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the tables: scale / shift reproduce y, and the statistics route gives the same moments
    y_ss = f["x"] * f["scale"][..., None] + f["shift"][..., None]
    assert np.abs((so.silu(y_ss) if silu else y_ss) - f["y"]).max() <= 1e-12 * np.abs(f["y"]).max()
    st0, st1 = so.split_stats(x0, 3), (so.split_stats(x1, 2) if c1 else None)
    p = so.gn_from_parts(st0, gamma, beta, groups, h * w, stats1=st1)
    for k in ("mean", "rstd", "scale", "shift"):
        assert np.allclose(p[k], f[k], rtol=1e-11, atol=1e-11), k


def test_roundings_layout_and_small_ops_match_torch():
    x = _r(11, (3, 16, 5, 7), 3.0)
    x[0, 0, 0, :4] = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 65504.0, 1e-7]          # bf16 ties both ways, fp16's ends
    xt = torch.from_numpy(x)
    assert np.array_equal(so.round_bf16(x), xt.to(torch.bfloat16).float().numpy())
    assert np.array_equal(so.round_fp16(x), xt.to(torch.float16).float().numpy())
    xb = so.to_blocked(x)
    assert xb.shape == (3, 2, 5, 7, 8) and xb[1, 1, 2, 3, 5] == x[1, 13, 2, 3] and np.array_equal(so.from_blocked(xb), x)
    z = np.array(T.SILU_GRID)
    zt = torch.from_numpy(z).requires_grad_(True)
    F.silu(zt).sum().backward()
    assert np.allclose(so.silu(z), F.silu(zt).detach().numpy(), rtol=1e-13, atol=1e-300) and np.isfinite(so.dsilu(z)).all()
    assert np.allclose(so.dsilu(z), zt.grad.numpy(), rtol=1e-12, atol=1e-300)
    # nearest x2, its adjoint (<up(x), g> = <x, pool(g)>), the fp32 order, and both in the blocked layout
    s, g = _r(12, (2, 3, 4, 6)), _r(13, (2, 3, 8, 12))
    assert np.array_equal(so.upsample_nearest2x(s), F.interpolate(torch.from_numpy(s), scale_factor=2.0, mode="nearest").numpy())
    assert np.allclose((so.upsample_nearest2x(s).astype(np.float64) * g).sum(), (s * so.sumpool2x2(g)).sum(), rtol=1e-12)
    assert np.abs(so.sumpool2x2_f32(g, s) - so.sumpool2x2(g, s)).max() <= 1e-6
    sb, gb = _r(14, (1, 2, 3, 5, 8)), _r(15, (1, 2, 6, 10, 8))
    assert np.array_equal(so.from_blocked(so.upsample_nearest2x(sb, (-3, -2))), so.upsample_nearest2x(so.from_blocked(sb)))
    assert np.array_equal(so.from_blocked(so.sumpool2x2_f32(gb, sb, (-3, -2))), so.sumpool2x2_f32(so.from_blocked(gb), so.from_blocked(sb)))
    # linear layer and the losses against autograd
    xl, wl, bl, dyl = (torch.from_numpy(_r(20 + i, sh)).double() for i, sh in enumerate(((5, 7), (4, 7), (4,), (5, 4))))
    xl.requires_grad_(True), wl.requires_grad_(True), bl.requires_grad_(True)
    (F.linear(xl, wl, bl) * dyl).sum().backward()
    for got, want in zip(so.linear_bwd(xl.detach(), wl.detach(), dyl), (xl.grad, wl.grad, bl.grad)):
        assert np.allclose(got, want.numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(so.linear(xl.detach(), wl.detach(), bl.detach()), F.linear(xl, wl, bl).detach().numpy(), rtol=1e-13)
    pr, tg, wt = torch.from_numpy(_r(30, (4, 3, 5))).double().requires_grad_(True), torch.from_numpy(_r(31, (4, 3, 5))).double(), \
        torch.tensor([0.5, 0.0, 2.0, 1.0], dtype=torch.float64)
    (3.0 * (wt[:, None, None] * (pr - tg) ** 2).mean()).backward()
    loss, grad = so.mse_weighted(pr.detach(), tg, wt, 3.0)
    assert abs(loss - float((wt[:, None, None] * (pr.detach() - tg) ** 2).mean())) <= 1e-14 and np.allclose(grad, pr.grad.numpy(), rtol=1e-13)
    assert so.mse(pr.detach(), tg)[0] == so.mse_weighted(pr.detach(), tg, np.ones(4))[0]
    assert abs(so.l2_norm(x) - float(xt.double().norm())) <= 1e-12 * so.l2_norm(x)


@pytest.mark.parametrize("clip", [False, True])
def test_adamw_rule_equals_torch_optim_in_fp64(clip):
    p_ref = torch.nn.Parameter(torch.from_numpy(_r(40, (50,))).double())
    opt = torch.optim.AdamW([p_ref], lr=1e-3, weight_decay=1e-2)
    p, m, v = p_ref.detach().numpy().copy(), np.zeros(50), np.zeros(50)
    for step in range(1, 4):
        g = _r(41 + step, (50,), 3.0).astype(np.float64)
        p_ref.grad = torch.from_numpy(g.copy())
        tn = float(torch.nn.utils.clip_grad_norm_([p_ref], 1.0)) if clip else None
        opt.step()
        p, m, v = so.adamw_step(p, g, m, v, step, 1e-3, weight_decay=1e-2, total_norm=tn, max_norm=1.0)
        st = opt.state[p_ref]
        for got, want in ((p, p_ref.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert np.allclose(got, want.numpy(), rtol=1e-12, atol=1e-15)
    g32 = np.array([1.0, np.inf, 3e38], dtype=np.float32)
    assert so.unscale_check_f32(g32, 2.0)[1] == 1 and so.unscale_check_f32(g32[[0, 2]], 2.0)[1] == 0     # torch's rule: before scaling
    assert so.clip_factor_f32(np.float32(4.0), 1.0) == np.float32(1.0) / (np.float32(4.0) + np.float32(1e-6))


# ---- path coverage ---------------------------------------------------------------------------------------------------------
def _quads(hw):
    """hw % 4 == 0: the two-pairs-in-flight loop of gn_bwd_stats_kernel over hw / 4 float4s -- no trip / one trip, no tail for
    most threads / a trip and a tail (gn_channel_stats_kernel: one stride of its loop, or more)"""
    q = hw // 4
    return "<=256" if q <= 256 else ("257-512" if q <= 512 else ">512")


def _batch_class(n):
    """gn_bwd_finalize_kernel: cpb = 256 / n channels per block (tail threads dead unless n divides 256), cpb = 1 from 129,
    a thread strides over the images above 256"""
    return ">256" if n > 256 else ("129-255" if n > 128 else ("divides" if 256 % n == 0 else "does not divide"))


def _run_class(entries):
    """gn_finalize_parts_kernel: a group's run of partials in one source against the wave (64) and one four-in-flight trip (256)"""
    return "<64" if entries < 64 else ("64-256" if entries <= 256 else ">256")


def _runs(c0, c1, groups, t0, t1):
    """per group: (partials in source 0, partials in source 1)"""
    cpg = (c0 + c1) // groups
    return [((min(g * cpg + cpg, c0) - min(g * cpg, c0)) * t0, (max(g * cpg + cpg, c0) - max(g * cpg, c0)) * t1) for g in range(groups)]


def _apply_blk_class(hw):
    """gn_bwd_apply_blk_kernel: 1024 pixels per block, clamped loads in a ragged last block"""
    return "<1024" if hw < 1024 else ("multiple" if hw % 1024 == 0 else "ragged")


def _csum_blk_class(hw):
    """channel_sums_blk_kernel: (main-loop trips of thread 0, tail iterations of thread 0 capped at 2 -- parity a, then b)"""
    i = trips = 0
    while i + 768 < hw:
        i, trips = i + 1024, trips + 1
    return (min(trips, 1), min(len(range(i, hw, 256)), 2))


def _temb_class(dim):
    """time_embed_kernel's row loops: 256 rows per stride"""
    return "<256" if dim < 256 else ("one stride" if dim == 256 else ("strides" if dim % 256 == 0 else "ragged strides"))


def test_case_tables_reach_every_selector_value(lib_built):
    from drivescenegen_amd import _lib
    splits = _lib.load().dsg_gn_bwd_blocked_splits
    hw_of = lambda cases: [c[-2] * c[-1] for c in cases]
    parts = [c[:5] for c in T.PARTS_CASES + [T.PARTS_SLICED]]
    table = [
        # (selector, the values its kernel distinguishes, the values the tables reach)
        ("gn fwd: hw % 4 == 0", {True, False}, {hw % 4 == 0 for hw in hw_of(T.GN_FWD_CASES)}),
        ("gn fwd, constant group: hw % 4", {0, 1, 2, 3}, {hw % 4 for hw in hw_of(T.GN_CONST_CASES)}),
        ("gn fwd: hw / 4", {"<=256", "257-512", ">512"}, {_quads(hw) for hw in hw_of(T.GN_FWD_CASES) if hw % 4 == 0}),
        ("gn fwd: sources", {"one", "edge", "straddle"},
         {"one" if not c[2] else ("edge" if c[1] % ((c[1] + c[2]) // c[3]) == 0 else "straddle") for c in T.GN_FWD_CASES}),
        ("gn bwd: hw % 4 == 0", {True, False}, {hw % 4 == 0 for hw in hw_of(T.GNB_CASES)}),
        ("gn bwd: hw / 4", {"<=256", "257-512", ">512"}, {_quads(hw) for hw in hw_of(T.GNB_CASES) if hw % 4 == 0}),
        ("gn bwd: batch", {"divides", "does not divide", "129-255", ">256"}, {_batch_class(c[0]) for c in T.GNB_CASES}),
        ("gn bwd: fan-in with SiLU", set(T.FANIN), {f for v in T.GNB_VARIANTS for s, f in v if s}),
        ("gn bwd: SiLU off", {False}, {s for v in T.GNB_VARIANTS for s, f in v if not s}),
        ("gn bwd blocked: splits", {"1", "2", ">2"}, {str(s) if s <= 2 else ">2" for s in (splits(hw) for hw in hw_of(T.GNB_BLK_CASES))}),
        ("gn bwd blocked: hw against 1024", {"<1024", "multiple", "ragged"}, {_apply_blk_class(hw) for hw in hw_of(T.GNB_BLK_CASES)}),
        ("gn bwd blocked: batch", {"divides", "does not divide"}, {_batch_class(c[0]) for c in T.GNB_BLK_CASES}),
        ("gn bwd blocked: fan-in with SiLU", set(T.FANIN), {f for s, f in T.GNB_BLK_VARIANTS if s}),
        ("gn bwd blocked: SiLU", {True, False}, {s for s, f in T.GNB_BLK_VARIANTS}),
        ("finalize parts: cpg <= 64", {True, False}, {(c[0] + c[1]) // c[2] <= 64 for c in parts}),
        ("finalize parts: run length", {"<64", "64-256", ">256"}, {_run_class(r) for c in parts for rr in _runs(*c) for r in rr if r}),
        ("finalize parts: t0 != t1", {True}, {c[3] != c[4] for c in parts if c[1]}),
        ("finalize parts: a group's sources", {"0", "1", "both"},
         {"both" if a and b else ("0" if a else "1") for c in parts for a, b in _runs(*c)}),
        ("range bound: slices", {1, 2}, {min(32, max(1, c[0] * c[3] // 2048)) for c in parts}),
        ("channel sums: hw % 4 == 0", {True, False}, {hw % 4 == 0 for hw in hw_of(T.CSUM_CASES)}),
        ("channel sums blocked: main loop, tail", {(0, 1), (1, 0), (1, 1), (1, 2)}, {_csum_blk_class(hw) for hw in hw_of(T.CSUM_BLK_CASES)}),
        ("sumpool blocked: w even", {True, False}, {c[2] % 2 == 0 for c in T.UPS_BLK_CASES}),
        ("linear bwd: n % 4 == 0", {True, False}, {c[0] % 4 == 0 for c in T.LINEAR_BWD_CASES}),
        ("linear bwd: in_f % 32 == 0", {True, False}, {c[1] % 32 == 0 for c in T.LINEAR_BWD_CASES}),
        ("linear bwd: out_f against its 8 wave-halves", {"<8", ">=8"}, {"<8" if c[2] < 8 else ">=8" for c in T.LINEAR_BWD_CASES}),
        ("linear: n % 8 == 0", {True, False}, {c[0] % 8 == 0 for c in T.LINEAR_CASES}),
        ("linear: a second pass of 8 images", {True, False}, {c[0] > 8 for c in T.LINEAR_CASES}),
        ("linear: out_f % 4 == 0", {True, False}, {c[2] % 4 == 0 for c in T.LINEAR_CASES}),
        ("linear: in_f against the wave", {"<64", "64", ">64"}, {"<64" if c[1] < 64 else ("64" if c[1] == 64 else ">64") for c in T.LINEAR_CASES}),
        ("time embedding: dim", {"<256", "one stride", "strides", "ragged strides"}, {_temb_class(d) for _, d in T.TEMB_CASES}),
        ("reduce rows: n against its unroll of 8", {"<8", "8", ">8"}, {"<8" if c[0] < 8 else ("8" if c[0] == 8 else ">8") for c in T.ROWS_CASES}),
        ("loss: grid capped at 2048 blocks", {True, False}, {n * per > 2048 * 1024 for n, per in T.LOSS_CASES}),
        ("loss: stride a whole number of samples", {True, False},
         {(min(2048, -(-n * per // 1024)) * 256) % per == 0 for n, per in T.LOSS_CASES if n > 1}),
        ("loss: per above the grid stride", {True, False}, {per > min(2048, -(-n * per // 1024)) * 256 for n, per in T.LOSS_CASES}),
        ("flat kernels: more than one block", {True, False}, {k > 1024 for k in T.FLAT_NUMELS + T.UNSCALE_NUMELS + T.ADAMW_NUMELS}),
    ]
    missing = {name: sorted(map(str, want - got)) for name, want, got in table if want - got}
    assert not missing, missing
    # every backward case runs once with SiLU on (each is the only case of one selector value)
    assert all(any(s for s, _ in v) for v in T.GNB_VARIANTS) and len(T.GNB_VARIANTS) == len(T.GNB_CASES)
    # the shapes the tables promise in their comments
    assert [splits(hw) for hw in hw_of(T.GNB_BLK_CASES)] == [1, 1, 2, 4, 1]
    assert [sorted({r for rr in _runs(*c) for r in rr if r}) for c in T.PARTS_CASES] == [[96], [18, 300], [128, 160], [10, 14, 20, 28]]


# ---- the scale / shift rounding model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.35, 3.0, 30.0, 300.0, 3000.0])
def test_scale_shift_formula_in_fp32_stays_inside_twice_the_bound(ratio):
    """The kernels' formula emulated in fp32 -- sc = fl(rstd * gamma), sh = fl(beta - fl(mean_f * sc)), y = fl(x * sc + sh) --
    stays below 2 * B of the fp64 value, B = 2^-24 * (|x sc| + |mean sc| + |beta| + |y|), at every group mean / std ratio: the GPU
    test's 4 * B leaves the kernel the roundings of its own statistics.  Worst measured here: 1.27 * B, at ratio 3."""
    f32 = np.float32
    n, c, groups, hw = 2, 8, 2, 63
    x = (_r(50, (n, c, hw)) + f32(ratio)).astype(f32)
    gamma, beta = 1 + _r(51, (c,), 0.2), _r(52, (c,), 0.2)
    f = so.gn_forward(x[..., None], gamma, beta, groups)
    assert np.allclose(f["mean"] * f["rstd"], ratio, rtol=0.15, atol=0.1)     # (the sample moments of 252 values)
    rstd_f, mean_f = f["rstd"].astype(f32), f["mean"].astype(f32)
    sc = (rstd_f * gamma[None, :]).astype(f32)
    sh = (beta[None, :] - (mean_f * sc).astype(f32)).astype(f32)
    y = (x.astype(np.float64) * sc[..., None].astype(np.float64) + sh[..., None].astype(np.float64)).astype(f32)   # one rounding: an fma
    bound = T._gn_bound(f, beta)
    worst = float((np.abs(y - f["y"]) / bound).max())
    print(f"ratio {ratio:g}: max |err| / B = {worst:.3f}")
    assert worst <= 2.0, worst
