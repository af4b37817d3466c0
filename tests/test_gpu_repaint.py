"""RePaint on the GPU: ``dsg_repaint_step`` / ``dsg_repaint_undo`` against the NumPy fp32 restatement (tests/repaint_oracle.py)
value for value, the in-kernel Philox source against ``dsg_philox_normal``, ``RePaintPipeline`` against ``DDIMPipeline`` where
the two must coincide, the invariants of real runs, teacher-forced parity with a CPU run, and guard margins round every output.

Comparisons of kernel outputs use ``np.array_equal`` on the fp32 VALUES (not bit views: ``0*known + 1*unknown`` may turn -0
into +0); no tolerance.  SURVEY 8c's teacher-forced bound applies only where the U-Net is in the path."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import _lib, ops  # noqa: E402
from tests import repaint_oracle as ro  # noqa: E402
from tests.common import CFG1, CFG2, max_abs, rel_l2, synth_weights, trajectory_weights  # noqa: E402

DEV = "cuda"
SENTINEL = 123456.0
TABS = ro.tables()


def _guarded(numel, margin):
    """(whole buffer, interior view of `numel` floats) with `margin` floats of SENTINEL on each side (>= 4 KiB)."""
    assert margin * 4 >= 4096
    whole = torch.full((numel + 2 * margin,), SENTINEL, dtype=torch.float32, device=DEV)
    return whole, whole[margin:margin + numel]


def _margins_intact(whole, numel, margin):
    w = whole.cpu().numpy()
    return bool((w[:margin] == SENTINEL).all() and (w[margin + numel:] == SENTINEL).all())


def _inputs(shape, orig_n, mask_n, mask_c, mask_kind, seed):
    n, c, h, w = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    e = rng.standard_normal(shape).astype(np.float32)
    z = rng.standard_normal(shape).astype(np.float32)
    orig = rng.uniform(-1, 1, (orig_n, c, h, w)).astype(np.float32)
    if mask_kind == "binary":
        m = (rng.uniform(0, 1, (mask_n, mask_c, h, w)) < 0.5).astype(np.float32)
    elif mask_kind == "channel":            # keep whole planes, generate the others
        m = np.zeros((mask_n, mask_c, h, w), np.float32)
        m[:, ::2] = 1
    else:                                   # the kernel is a blend: any weight in [0, 1]
        m = rng.uniform(0, 1, (mask_n, mask_c, h, w)).astype(np.float32)
    return x, e, orig, m, z


def _call_step(x, e, orig, m, z, s, clip, add_std, margin, seed=0, offset=0, want_noise_out=False):
    """One dsg_repaint_step with `prev` (and `noise_out`) as interior views of sentinel-filled buffers.  z=None: Philox.
    Returns (prev ndarray, noise_out ndarray | None, margins intact)."""
    shape = x.shape
    numel = x.size
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in dict(x=x, e=e, orig=orig, m=m).items()}
    zt = torch.from_numpy(z).to(DEV) if z is not None else None
    pw, prev = _guarded(numel, margin)
    nw, nout = _guarded(numel, margin) if want_noise_out else (None, None)
    a = _lib.RepaintStepArgs(
        sample=t["x"].data_ptr(), eps=t["e"].data_ptr(), original=t["orig"].data_ptr(), mask=t["m"].data_ptr(),
        noise=zt.data_ptr() if zt is not None else None, prev=prev.data_ptr(),
        noise_out=nout.data_ptr() if nout is not None else None, n=shape[0], c=shape[1], h=shape[2], w=shape[3],
        original_n=orig.shape[0], mask_n=m.shape[0], mask_c=m.shape[1], add_std=int(add_std),
        sqrt_beta_prod_t=float(s["sb"]), sqrt_alpha_prod_t=float(s["sa"]), clip=float(clip), sqrt_alpha_prev=float(s["sap"]),
        dir_coef=float(s["dc"]), std=float(s["std"]), sqrt_beta_prev=float(s["sbp"]), seed=seed, offset=offset)
    _lib.check(_lib.load().dsg_repaint_step(ctypes.byref(a), _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    ok = _margins_intact(pw, numel, margin) and (nw is None or _margins_intact(nw, numel, margin))
    return prev.cpu().numpy().reshape(shape), (nout.cpu().numpy().reshape(shape) if nout is not None else None), ok


def _call_undo(x, z, ck, cz, margin, seed=0, offset=0):
    numel = x.size
    xt = torch.from_numpy(x).to(DEV)
    zt = torch.from_numpy(z).to(DEV) if z is not None else None
    ow, out = _guarded(numel, margin)
    _lib.check(_lib.load().dsg_repaint_undo(xt.data_ptr(), zt.data_ptr() if zt is not None else None, out.data_ptr(), numel,
                                           float(ck), float(cz), seed, offset, _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(x.shape), _margins_intact(ow, numel, margin)


# (t, eta) of an 8-step schedule: mid schedule, late, and the LAST step (prev_t < 0: sap = 1, sbp = 0, dc = 0)
SCALARS = {"t875": (875, 0.0), "t875_eta1": (875, 1.0), "t125_eta1": (125, 1.0), "t125_eta03": (125, 0.3), "t0_last": (0, 1.0)}
# numel multiple of 1024; 210 (not a multiple of 4); hw = 279 odd with numel % 4 == 0; 3600 (not a multiple of 256); 1 element
SHAPES = [(2, 4, 16, 16), (2, 3, 5, 7), (3, 4, 9, 31), (5, 3, 20, 12), (1, 1, 1, 1), (2, 3, 64, 64)]
# margin in floats: 1024 keeps the interior 16-byte aligned (dwordx4 path), 1027 does not (dword path)
MARGINS = (1024, 1027)


def _step_cases():
    cases = []
    for si, shape in enumerate(SHAPES):                         # every shape x every broadcast form of orig / mask
        n, c = shape[0], shape[1]
        for on in sorted({1, n}):
            for mn in sorted({1, n}):
                for mc in sorted({1, c}):
                    cases.append((shape, on, mn, mc, "binary", "t125_eta1", 1.0, True, MARGINS[(si + on + mn + mc) % 2]))
    for key in SCALARS:                                          # every scalar set x clip on / off x std term on / off
        for clip in (1.0, 0.0):
            for add_std in (False, True):
                for margin in MARGINS:
                    cases.append(((2, 4, 16, 16), 1, 2, 4, "binary", key, clip, add_std, margin))
                cases.append(((2, 3, 5, 7), 2, 1, 3, "soft", key, clip, add_std, 1024))
    for margin in MARGINS:                                       # a per-channel mask: keep planes 0 and 2, generate 1 and 3
        cases.append(((2, 4, 16, 16), 1, 1, 4, "channel", "t875", 1.0, False, margin))
        cases.append(((3, 4, 9, 31), 3, 1, 4, "channel", "t0_last", 1.0, True, margin))
    return cases


STEP_CASES = _step_cases()


def _run_step_case(i, case):
    shape, on, mn, mc, kind, key, clip, add_std, margin = case
    t, eta = SCALARS[key]
    s = ro.step_scalars(t, 8, eta, tabs=TABS)
    x, e, orig, m, z = _inputs(shape, on, mn, mc, kind, 100 + i)
    got, _, intact = _call_step(x, e, orig, m, z, s, clip, add_std, margin)
    return got, ro.step(x, e, orig, m, z, s, clip, add_std), intact, (x, e, orig, m, z, s)


def test_step_equals_the_numpy_restatement_every_element():
    """Check 1: supplied noise; clip on / off, std term on / off, last step, all broadcast forms, odd sizes, per-channel mask."""
    assert len(STEP_CASES) > 80
    clipped = 0
    for i, case in enumerate(STEP_CASES):
        got, want, _, (x, e, orig, m, z, s) = _run_step_case(i, case)
        assert np.isfinite(want).all()
        assert np.array_equal(got, want), (i, case, int((got != want).sum()), float(np.abs(got - want).max()))
        clipped += int(case[6] > 0)
    assert clipped
    # the last step returns the original exactly where the mask keeps (sap = 1, sbp = 0)
    case = ((3, 4, 9, 31), 3, 1, 4, "channel", "t0_last", 1.0, True, 1024)
    got, want, _, (x, e, orig, m, z, s) = _run_step_case(999, case)
    keep = np.broadcast_to(m, got.shape) == 1
    assert np.array_equal(got[keep], np.broadcast_to(orig, got.shape)[keep]) and keep.any() and not keep.all()


def test_step_and_undo_stay_inside_their_buffers():
    """Check 6: every output of check 1's cases (and noise_out, and undo's) is an interior view of a larger buffer whose
    margins (>= 4 KiB each side) hold a sentinel; the margins are unchanged afterwards."""
    for i, case in enumerate(STEP_CASES):
        assert _run_step_case(i, case)[2], (i, case)
    for i, shape in enumerate(SHAPES):
        for margin in MARGINS:
            x, e, orig, m, _ = _inputs(shape, 1, 1, 1, "binary", 7 + i)
            s = ro.step_scalars(125, 8, 1.0, tabs=TABS)
            got, nout, intact = _call_step(x, e, orig, m, None, s, 1.0, True, margin, seed=5, offset=i, want_noise_out=True)
            assert intact and np.isfinite(got).all() and np.isfinite(nout).all(), (shape, margin)
            for z in (_inputs(shape, 1, 1, 1, "binary", 70 + i)[4], None):
                assert _call_undo(x, z, 0.8, 0.6, margin, seed=5, offset=i)[1], (shape, margin)


def test_undo_equals_the_numpy_restatement_every_element():
    for i, shape in enumerate(SHAPES):
        for margin in MARGINS:
            x, _, _, _, z = _inputs(shape, 1, 1, 1, "binary", 40 + i)
            for ck, cz in ro.undo_scalars(375, 8, tabs=TABS)[:3] + [ro.undo_scalars_fused(375, 8, tabs=TABS), (1.0, 0.0)]:
                got, intact = _call_undo(x, z, ck, cz, margin)
                assert intact and np.array_equal(got, ro.undo(x, z, ck, cz)), (shape, margin, ck, cz)


@pytest.mark.parametrize("seed,offset", [(0, 0), (14555, 3), (2 ** 63 + 12345, (5 << 40) | 77)])
def test_philox_source_is_the_named_tensor(seed, offset):
    """Check 2: noise_out is bitwise dsg_philox_normal(numel, seed, offset); prev is value-equal to the supplied-noise call fed
    that tensor; another offset names another tensor.  Same for undo."""
    for i, shape in enumerate(SHAPES):
        for margin in MARGINS:
            numel = int(np.prod(shape))
            named = ops.philox_normal((numel,), seed, offset).cpu().numpy().reshape(shape)
            x, e, orig, m, _ = _inputs(shape, 1, shape[0], 1, "binary", 60 + i)
            s = ro.step_scalars(125, 8, 1.0, tabs=TABS)
            got, nout, intact = _call_step(x, e, orig, m, None, s, 1.0, True, margin, seed, offset, want_noise_out=True)
            assert intact and np.array_equal(nout.view(np.uint32), named.view(np.uint32)), (shape, margin)
            fed, _, _ = _call_step(x, e, orig, m, named, s, 1.0, True, margin)
            assert np.array_equal(got, fed) and np.array_equal(got, ro.step(x, e, orig, m, named, s, 1.0, True))
            other, nout2, _ = _call_step(x, e, orig, m, None, s, 1.0, True, margin, seed, offset + 1, want_noise_out=True)
            assert not np.array_equal(nout2, nout)
            assert numel < 64 or not np.array_equal(other, got)
            und, _ = _call_undo(x, None, 0.8, 0.6, margin, seed, offset)
            assert np.array_equal(und, ro.undo(x, named, 0.8, 0.6)), (shape, margin)


# ---- whole runs on the tiny network ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    return synth_weights(d.UNet2DModel(**CFG1)).to(DEV).eval().requires_grad_(False)


def _scene(n, c, hw, seed=5):
    from drivescenegen_amd import synth
    return torch.from_numpy(synth.synth_scene_rasters(n, c, hw, hw, seed))


def test_with_nothing_kept_the_run_is_ddim(tiny):
    """Check 3: mask == 0, eta == 0, jump_n_sample == 1: step by step and at the end, RePaint == DDIM (same network, seed and
    step count).  Only tested code is trusted here."""
    steps, batch = 12, 2
    shape = (batch, 3, 64, 64)
    orig, mask = _scene(1, 3, 64), torch.zeros(1, 1, 64, 64)
    ddim, rp = d.DDIMScheduler(), d.RePaintScheduler()
    ddim.set_timesteps(steps)
    rp.set_timesteps(steps, jump_length=5, jump_n_sample=1)
    assert torch.equal(ddim.timesteps, rp.timesteps)
    g = torch.Generator().manual_seed(7)
    xd = xr = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    od, md = orig.to(DEV), mask.to(DEV)
    for t in ddim.timesteps.tolist():
        xd = ddim.step(tiny(xd, t).sample, t, xd).prev_sample
        xr = rp.step(tiny(xr, t).sample, t, xr, od, md, generator=g).prev_sample
        assert np.array_equal(xd.cpu().numpy(), xr.cpu().numpy()), t
    a = d.DDIMPipeline(tiny, d.DDIMScheduler())(batch_size=batch, generator=torch.Generator().manual_seed(11),
                                                num_inference_steps=steps, output_type="np.array").images
    b = d.RePaintPipeline(tiny, d.RePaintScheduler())(orig, mask, num_inference_steps=steps, jump_length=5, jump_n_sample=1,
                                                      generator=torch.Generator().manual_seed(11), output_type="np.array",
                                                      batch_size=batch).images
    assert a.shape == b.shape == (batch, 64, 64, 3) and np.array_equal(a, b)


def _final_sample(pipe, *args, **kw):
    """The pipeline's final x (model domain, [N, C, H, W]) from its float output: images = x/2 + 0.5 clamped, NHWC."""
    return pipe(*args, output_type="np.array", **kw).images


def _expect_image(orig):
    """What _finish makes of the original (the kept region of a result must equal this, exactly)."""
    x = orig.numpy().astype(np.float32)
    return np.clip(x / np.float32(2.0) + np.float32(0.5), 0, 1).transpose(0, 2, 3, 1)


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_invariants_of_a_real_run(tiny, noise, eta):
    """Check 4 on (20, 5, 2): the kept region equals the original exactly (spatial and per-channel masks); everything kept ->
    the input comes back whatever the network says; batch_size=K on one image agrees on the kept region and differs off it;
    the same seed gives the same result twice, bitwise; device noise leaves the host generator untouched."""
    pipe = d.RePaintPipeline(tiny, d.RePaintScheduler())
    orig = _scene(1, 3, 64)
    want = _expect_image(orig)
    spatial = torch.zeros(1, 1, 64, 64)
    spatial[..., :, :32] = 1                                   # keep the left half, outpaint the right
    planes = torch.zeros(1, 3, 64, 64)
    planes[:, :2] = 1                                          # keep planes 0 and 1, re-draw plane 2
    K = 3

    def run(mask, seed):
        g = torch.Generator().manual_seed(seed)
        before = g.get_state()
        kw = dict(noise="device", seed=seed) if noise == "device" else {}
        out = _final_sample(pipe, orig, mask, num_inference_steps=20, jump_length=5, jump_n_sample=2, eta=eta, generator=g,
                            batch_size=K, **kw)
        if noise == "device":
            assert torch.equal(g.get_state(), before)
        else:
            assert not torch.equal(g.get_state(), before)
        return out

    for mask in (spatial, planes):
        out = run(mask, 21)
        assert out.shape == (K, 64, 64, 3) and np.isfinite(out).all()
        keep = np.broadcast_to(mask.numpy().transpose(0, 2, 3, 1) == 1, out.shape)
        assert np.array_equal(out[keep], np.broadcast_to(want, out.shape)[keep])
        free = ~keep
        for k in range(1, K):
            assert not np.array_equal(out[0][free[0]], out[k][free[k]])
        assert np.array_equal(out, run(mask, 21))               # same seed, same bits
        assert not np.array_equal(out, run(mask, 22))
    everything = _final_sample(pipe, orig, torch.ones(1, 1, 64, 64), num_inference_steps=20, jump_length=5, jump_n_sample=2,
                               eta=eta, generator=torch.Generator().manual_seed(1), batch_size=2,
                               **(dict(noise="device", seed=1) if noise == "device" else {}))
    assert np.array_equal(everything, np.broadcast_to(want, everything.shape))


def test_pil_and_bool_inputs_reach_the_kernels(tiny):
    from PIL import Image
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    mask = np.zeros((64, 64), bool)
    mask[:32] = True
    pipe = d.RePaintPipeline(tiny, d.RePaintScheduler())
    out = pipe(Image.fromarray(u8), Image.fromarray(mask.astype(np.uint8) * 255), num_inference_steps=6,
               jump_length=2, jump_n_sample=2, generator=torch.Generator().manual_seed(0))
    assert len(out.images) == 1 and out.images[0].mode == "RGB" and out.images[0].size == (64, 64)
    assert np.array_equal(np.array(out.images[0])[:32], u8[:32])          # uint8 -> [-1, 1] -> uint8 round trip of the kept half
    tup = pipe(u8, mask, num_inference_steps=6, jump_length=2, jump_n_sample=2, generator=torch.Generator().manual_seed(0),
               return_dict=False)
    assert np.array_equal(np.array(tup[0][0]), np.array(out.images[0]))


def test_teacher_forced_parity_with_a_cpu_run():
    """Check 5: the oracle U-Net (contractive synthetic weights) + tests/repaint_oracle.py run (8, 3, 2) with eta = 1 from a
    seeded CPU generator; at every entry the engine gets the oracle's input.  SURVEY 8c's teacher-forced bound on eps and on
    the step's output; undo entries value-equal.  The engine's scheduler draws from its own equally seeded generator: the bound
    can only hold if the order and shapes of its draws are the oracle's."""
    from oracle.unet_oracle import OracleUNet2DModel
    net = trajectory_weights(d.UNet2DModel(**CFG1), "tiny_c").to(DEV).eval().requires_grad_(False)
    ora = trajectory_weights(OracleUNet2DModel(**CFG1), "tiny_c").eval()
    shape = (2, 3, 64, 64)
    orig = _scene(1, 3, 64, seed=9)
    mask = torch.zeros(1, 3, 64, 64)
    mask[:, :, :, 20:] = 1
    mask[:, 2] = 0                                             # spatial on planes 0, 1; plane 2 generated everywhere

    def eps_fn(x, t):
        with torch.no_grad():
            return ora(torch.from_numpy(x), t).sample.numpy()

    final, rec = ro.run(eps_fn, orig.numpy(), mask.numpy(), shape, 8, 3, 2, 1.0, torch.Generator().manual_seed(14555))
    assert sum(r["kind"] == "undo" for r in rec) == 6 and len(rec) == 20

    def within(got, want, what):
        got, want = torch.from_numpy(got), torch.from_numpy(want)
        ma, rl = max_abs(got, want), rel_l2(got, want)
        print(f"{what}: max|d| {ma:.3e} (bound {2e-4 * max(1.0, float(want.abs().max())):.3e}), rel-L2 {rl:.3e}")
        assert ma <= 2e-4 * max(1.0, float(want.abs().max())) and rl <= 1e-4, (what, ma, rl)

    sch = d.RePaintScheduler()
    sch.set_timesteps(8, 3, 2)
    sch.eta = 1.0
    assert sch.timesteps.tolist() == [int(r["t"]) for r in rec]
    g = torch.Generator().manual_seed(14555)
    x_T = torch.randn(shape, generator=g)
    assert np.array_equal(x_T.numpy(), rec[0]["x_in"])
    od, md = orig.to(DEV), mask.to(DEV)
    for i, r in enumerate(rec):
        x_in = torch.from_numpy(r["x_in"]).to(DEV)
        if r["kind"] == "step":
            eps = net(x_in, r["t"]).sample
            within(eps.cpu().numpy(), r["eps"], f"entry {i} t={r['t']} eps")
            out = sch.step(eps, r["t"], x_in, od, md, generator=g).prev_sample
            within(out.cpu().numpy(), r["x_out"], f"entry {i} t={r['t']} step")
        else:
            out = sch.undo_step(x_in, r["t_from"], generator=g)
            assert np.array_equal(out.cpu().numpy(), r["x_out"]), (i, r["t_from"])
    keep = np.broadcast_to(mask.numpy() == 1, final.shape)
    assert np.array_equal(final[keep], np.broadcast_to(orig.numpy(), final.shape)[keep])


def test_full_size_call():
    """Check 7: configs[1]'s network (256 x 256 x 4) at batch 2, (20, 5, 2), half-image mask."""
    net = synth_weights(d.UNet2DModel(**CFG2)).to(DEV).eval().requires_grad_(False)
    pipe = d.RePaintPipeline(net, d.RePaintScheduler())
    orig = _scene(2, 4, 256, seed=3)
    mask = torch.zeros(1, 1, 256, 256)
    mask[..., :128, :] = 1
    out = pipe(orig, mask, num_inference_steps=20, jump_length=5, jump_n_sample=2, generator=torch.Generator().manual_seed(2),
               output_type="np.array").images
    assert out.shape == (2, 256, 256, 4) and np.isfinite(out).all()
    assert np.array_equal(out[:, :128], _expect_image(orig)[:, :128])
    assert not np.array_equal(out[0, 128:], out[1, 128:])
    pil = pipe(orig, mask, num_inference_steps=4, jump_length=2, jump_n_sample=1, noise="device", seed=4).images
    assert len(pil) == 2 and pil[0].mode == "RGBA" and pil[0].size == (256, 256)
    want = (_expect_image(orig) * 255).round().astype("uint8")
    assert np.array_equal(np.array(pil[1])[:128], want[1, :128])
