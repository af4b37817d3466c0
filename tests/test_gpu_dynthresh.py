"""Dynamic thresholding on the GPU: ``dsg_dynthresh_scale``, ``dsg_ddpm_step_thr`` and ``dsg_ddim_step_thr`` against the NumPy
fp32 restatement (tests/dynthresh_oracle.py) value for value, whole scheduler loops on a model with a known answer, and the
pipelines / ``fit`` with a thresholding scheduler.

Comparisons use ``np.array_equal`` on the fp32 VALUES; no tolerance.  Every output, ``s`` and the workspace are interior views
of sentinel-filled buffers (the ``_guarded`` idiom of tests/test_gpu_dpmsolver.py: margins of 1024 floats -- the interior
16-byte aligned, dwordx4 path -- and 1027 floats -- dword path); margins and inputs are checked intact."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import _lib  # noqa: E402
from tests import dpmsolver_oracle as do  # noqa: E402
from tests import dynthresh_oracle as dto  # noqa: E402
from tests.common import CFG1, synth_weights  # noqa: E402

DEV = "cuda"
F = np.float32
SENTINEL = 123456.0
MARGINS = (1024, 1027)
# per = 105: scalar tail, one block;  1116: odd hw, two blocks per row, three rows;  1024;  16384: many blocks per row
SHAPES = [(1, 3, 7, 5), (3, 4, 9, 31), (2, 4, 16, 16), (2, 4, 64, 64)]
RATIOS = (0.995, 0.5, 1.0)
MAX_VALUES = (1.0, 2.0)
ROW_SCALES = (0.1, 1.0, 10.0)
_DDPM, _DDIM = d.DDPMScheduler(), d.DDIMScheduler()
_DDIM.set_timesteps(50)            # (t = 500 and t = 20 are entries of the 50-step table)
STEP_TS = (500, 20)


def _guarded(numel, margin):
    assert margin * 4 >= 4096
    whole = torch.full((numel + 2 * margin,), SENTINEL, dtype=torch.float32, device=DEV)
    return whole, whole[margin:margin + numel]


def _margins_intact(whole, numel, margin):
    w = whole.cpu().numpy()
    return bool((w[:margin] == SENTINEL).all() and (w[margin + numel:] == SENTINEL).all())


def _ws_floats(n):
    b = ctypes.c_size_t()
    _lib.check(_lib.load().dsg_dynthresh_workspace_bytes(n, ctypes.byref(b)))
    assert b.value % 4 == 0
    return b.value // 4


def _upload(v, off):
    """`v` on the device, `off` floats past a 16-byte boundary."""
    return torch.zeros(v.size + 4, dtype=torch.float32, device=DEV)[off:off + v.size].view(v.shape).copy_(
        torch.from_numpy(np.ascontiguousarray(v)))


def _same(a, b):
    """value for value; NaN equals NaN (a row the contract makes NaN)"""
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


class _Run:
    """x, e (and z) on the device once; then the three entries, every output guarded.  With the misaligned margin the sample
    sits 3 floats off a 16-byte boundary too (a mix of aligned and misaligned inputs)."""

    def __init__(self, x, e, z, margin):
        self.host = dict(x=x, e=e, z=z)
        self.dev = {k: _upload(v, margin % 4 if k == "x" else 0) for k, v in self.host.items() if v is not None}
        self.n, self.numel, self.margin = x.shape[0], x.size, margin
        self.per = self.numel // self.n
        self.lib, self.st = _lib.load(), _lib.stream_ptr(torch.device(DEV))
        self.ok = True

    def scale(self, sb, sa, q, mx):
        k_lo, k_hi, w = dto.ranks(self.per, q)
        words = _ws_floats(self.n)
        sw, s = _guarded(self.n, self.margin)
        ww, ws = _guarded(words, self.margin)
        _lib.check(self.lib.dsg_dynthresh_scale(self.dev["x"].data_ptr(), self.dev["e"].data_ptr(), s.data_ptr(), self.n, self.per,
                                                float(sb), float(sa), k_lo, k_hi, float(w), float(mx), ws.data_ptr(), words * 4,
                                                self.st))
        torch.cuda.synchronize()
        self.ok = self.ok and _margins_intact(sw, self.n, self.margin) and _margins_intact(ww, words, self.margin)
        self.s = s
        return s.cpu().numpy()

    def _finish(self, pw, prev):
        torch.cuda.synchronize()
        self.ok = self.ok and _margins_intact(pw, self.numel, self.margin)
        return prev.cpu().numpy().reshape(self.host["x"].shape)

    def ddpm(self, sc, noise):
        pw, prev = _guarded(self.numel, self.margin)
        _lib.check(self.lib.dsg_ddpm_step_thr(self.dev["x"].data_ptr(), self.dev["e"].data_ptr(),
                                              self.dev["z"].data_ptr() if noise else None, self.s.data_ptr(), prev.data_ptr(),
                                              self.numel, self.per, sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], sc["coef_x0"],
                                              sc["coef_xt"], sc["sigma"], self.st))
        return self._finish(pw, prev)

    def ddim(self, sc):
        pw, prev = _guarded(self.numel, self.margin)
        _lib.check(self.lib.dsg_ddim_step_thr(self.dev["x"].data_ptr(), self.dev["e"].data_ptr(), self.s.data_ptr(), prev.data_ptr(),
                                              self.numel, self.per, sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"],
                                              sc["sqrt_alpha_prev"], sc["dir_coef"], self.st))
        return self._finish(pw, prev)

    def inputs_unchanged(self):
        return all(np.array_equal(self.dev[k].cpu().numpy(), self.host[k], equal_nan=True) for k in self.dev)


def _check_all(run, t, q, mx, what):
    """scale, DDPM step (device noise; none, as at t = 0), DDIM step against the restatement; two scale calls, same bits."""
    x, e, z = run.host["x"], run.host["e"], run.host["z"]
    pm, im = _DDPM.step_scalars(t), _DDIM.step_scalars(t)
    assert pm["sqrt_beta_prod_t"] == im["sqrt_beta_prod_t"] and pm["sqrt_alpha_prod_t"] == im["sqrt_alpha_prod_t"]
    want_noise, want_s = dto.ddpm_step(x, e, z, pm, q, mx)
    want_plain, _ = dto.ddpm_step(x, e, None, pm, q, mx)
    want_ddim, _ = dto.ddim_step(x, e, im, q, mx)
    s = run.scale(pm["sqrt_beta_prod_t"], pm["sqrt_alpha_prod_t"], q, mx)
    print(what, "s", s, "oracle", want_s)
    assert _same(s, want_s), (what, s, want_s)
    for name, got, want in (("ddpm+noise", run.ddpm(pm, True), want_noise), ("ddpm", run.ddpm(pm, False), want_plain),
                            ("ddim", run.ddim(im), want_ddim)):
        assert _same(got, want), (what, name, int((got != want).sum()))
    again = run.scale(pm["sqrt_beta_prod_t"], pm["sqrt_alpha_prod_t"], q, mx)
    assert np.array_equal(again.view(np.uint32), s.view(np.uint32)), what
    assert run.ok and run.inputs_unchanged(), what
    return want_s


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scale_and_steps_equal_the_numpy_restatement(shape):
    """Scalars of t = 500 and t = 20, three ratios, two maxima, rows scaled by 0.1 / 1 / 10, both margins."""
    seen = set()
    for ti, t in enumerate(STEP_TS):
        for si in range(len(ROW_SCALES)):
            rng = np.random.default_rng(1000 * ti + 10 * si + shape[-1])
            x, e, z = (rng.standard_normal(shape).astype(F) for _ in range(3))
            for r in range(shape[0]):          # row r of call si: every row sees every scale, every call mixes them
                x[r] *= F(ROW_SCALES[(si + r) % 3])
                e[r] *= F(ROW_SCALES[(si + r) % 3])
            for margin in MARGINS:
                run = _Run(x, e, z, margin)
                for q in RATIOS:
                    for mx in MAX_VALUES:
                        want_s = _check_all(run, t, q, mx, (shape, t, si, margin, q, mx))
                        assert np.isfinite(want_s).all()
                        if mx == 2.0:
                            seen |= {"lower" if v == 1.0 else "upper" if v == 2.0 else "inside" for v in want_s}
    # (a condition on the ORACLE's values: the grid reaches the lower clamp, the open interval and the upper clamp)
    assert seen == {"lower", "inside", "upper"}, seen


def _constructed(per):
    """name -> row of `per` values; p0 = x when sb = 0, sa = 1 and e = 0."""
    rng = np.random.default_rng(per)
    k_lo, k_hi, _ = dto.ranks(per, 0.9)
    assert k_hi == k_lo + 1
    two = np.full(per, 1.25, dtype=F)
    two[:k_lo + 1] = 1.0                              # rank k_lo is the last 1.0, rank k_hi the first 1.25
    rows = dict(equal=np.full(per, 1.37, dtype=F), two=rng.permutation(two), zero=np.zeros(per, dtype=F),
                negative=-np.abs(rng.standard_normal(per).astype(F)) * F(1.5) - F(0.01),
                denormal=(rng.integers(1, 2 ** 20, per).astype(np.uint32)).view(F) * rng.choice(np.array([-1, 1], dtype=F), per),
                normal=rng.standard_normal(per).astype(F) * F(1.2))
    assert (np.abs(rows["denormal"]) < np.finfo(F).tiny).all() and (rows["denormal"] != 0).all()
    nan = rows["normal"].copy()
    nan[per // 3] = np.nan
    rows["nan"] = nan
    return rows


@pytest.mark.parametrize("shape", [(3, 3, 7, 5), (3, 4, 9, 31)], ids=["per105", "per1116"])
def test_constructed_rows(shape):
    """All-equal, two-valued with the ranks on the jump, all-zero, negative-only, denormal rows; one NaN in row 1 of 3: that row
    is NaN, its neighbours equal the restatement, the calls return normally."""
    per = int(np.prod(shape[1:]))
    rows = _constructed(per)
    batches = [("equal", "two", "zero"), ("negative", "denormal", "normal"), ("normal", "nan", "negative")]
    z = np.random.default_rng(3).standard_normal(shape).astype(F)
    for names in batches:
        x = np.stack([rows[k] for k in names]).reshape(shape)
        for e in (np.zeros(shape, dtype=F), np.random.default_rng(4).standard_normal(shape).astype(F) * F(0.25)):
            if "denormal" in names and e.any():
                e = e.copy()
                e[names.index("denormal")] = 0                 # (keep the row's p0 denormal)
            for margin in MARGINS:
                run = _Run(x, e, z, margin)
                for q in (0.9, 1.0, 0.0):
                    for t in STEP_TS:
                        want_s = _check_all(run, t, q, 2.0, (names, margin, q, t))
                        assert np.isnan(want_s).tolist() == [k == "nan" for k in names]
                # p0 = x exactly: the scale of a constructed row is known without the oracle
                if not e.any():
                    s = run.scale(0.0, 1.0, 0.9, 2.0)
                    known = dict(equal=F(1.37), zero=F(1.0), denormal=F(1.0))
                    for r, k in enumerate(names):
                        if k in known:
                            assert s[r] == known[k], (k, s[r])
                        if k == "two":
                            assert 1.0 < s[r] < 1.25 and s[r] == dto.scale_of_abs(np.abs(x[r].reshape(1, -1)), 0.9, 2.0)[0]
                        if k == "nan":
                            assert np.isnan(s[r])
                    assert run.ok


# ---- scheduler level ----------------------------------------------------------------------------------------------------------
TABS = do.tables(F)


@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_a_ten_step_loop_equals_the_restatement(kind):
    """eps of the analytic model computed on the host in NumPy fp32 from the engine's own x; thresholding=True,
    sample_max_value=1.5.  Every step equals the restatement's step on the same chain (DDPM: the seeded CPU generator's draws)."""
    shape, steps, q, mx = (3, 4, 9, 31), 10, 0.995, 1.5
    cls = d.DDIMScheduler if kind == "ddim" else d.DDPMScheduler
    sch = cls(thresholding=True, sample_max_value=mx)
    ref = cls()                                   # (the host scalars: not what thresholding changes)
    sch.set_timesteps(steps)
    ref.set_timesteps(steps)
    x_np = np.random.default_rng(8).standard_normal(shape).astype(F) * F(1.5)
    x = torch.from_numpy(x_np).to(DEV)
    g, twin = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
    scales = []
    for i, t in enumerate(sch.timesteps.tolist()):
        eps = do.analytic_eps(x_np, t, TABS, F) * F(1.3)              # (pushed off the optimum: the quantile passes 1 on the way)
        if kind == "ddim":
            want, s = dto.ddim_step(x_np, eps, ref.step_scalars(t), q, mx)
            out = sch.step(torch.from_numpy(eps).to(DEV), t, x).prev_sample
        else:
            z = torch.randn(shape, generator=twin).numpy() if t > 0 else None
            want, s = dto.ddpm_step(x_np, eps, z, ref.step_scalars(t), q, mx)
            out = sch.step(torch.from_numpy(eps).to(DEV), t, x, generator=g).prev_sample
        got = out.cpu().numpy()
        scales.append(s)
        assert np.isfinite(want).all() and np.array_equal(got, want), (kind, i, t, s, int((got != want).sum()))
        x, x_np = out, got
    scales = np.stack(scales)
    print(kind, "oracle scales per step", scales.tolist())
    assert (scales > 1.0).any(), scales           # thresholding acted somewhere on the chain
    if kind == "ddpm":
        assert torch.equal(g.get_state(), twin.get_state())


@pytest.fixture(scope="module")
def tiny():
    return synth_weights(d.UNet2DModel(**CFG1)).to(DEV).eval().requires_grad_(False)


def _images(pipe_cls, net, steps, batch=2, seed=5, **sched):
    pipe = pipe_cls(net, pipe_cls._scheduler_cls())
    pipe.scheduler = type(pipe.scheduler).from_config(pipe.scheduler.config, **sched)
    return pipe(batch_size=batch, generator=torch.Generator().manual_seed(seed), num_inference_steps=steps,
                output_type="np.array").images


@pytest.mark.parametrize("pipe_cls", [d.DDIMPipeline, d.DDPMPipeline], ids=["ddim_pipeline", "ddpm_pipeline"])
def test_a_maximum_of_one_is_the_static_clip(tiny, pipe_cls):
    """sample_max_value = 1: s == 1 for every sample, x / 1 is exact, so the whole call is bit-identical to clip_sample=True."""
    thr = _images(pipe_cls, tiny, 8, thresholding=True, sample_max_value=1.0)
    clip = _images(pipe_cls, tiny, 8, thresholding=False, clip_sample=True)
    assert thr.shape == (2, 64, 64, 3) and np.array_equal(thr, clip)
    # thresholding wins over clip_sample, whatever the latter says
    assert np.array_equal(_images(pipe_cls, tiny, 8, thresholding=True, sample_max_value=1.0, clip_sample=False), clip)


def test_a_thresholded_pipeline_call(tiny):
    thr = _images(d.DDIMPipeline, tiny, 8, thresholding=True, sample_max_value=1.5)
    clip = _images(d.DDIMPipeline, tiny, 8)
    assert thr.shape == (2, 64, 64, 3) and np.isfinite(thr).all() and not np.array_equal(thr, clip)
    assert np.array_equal(thr, _images(d.DDIMPipeline, tiny, 8, thresholding=True, sample_max_value=1.5))      # same seed, same bits
    # rows are thresholded one by one: a shard's rows are the full call's
    pipe = d.DDIMPipeline(tiny, d.DDIMScheduler(thresholding=True, sample_max_value=1.5))
    part = pipe(batch_size=2, generator=torch.Generator().manual_seed(5), num_inference_steps=8, output_type="np.array",
                shard=(1, 2)).images
    assert np.array_equal(part, thr[1:2])


def test_fit_samples_with_a_thresholding_scheduler(tmp_path):
    """``fit(..., ema=)``: the epoch-end sampling call runs DDPMPipeline on the scheduler it was handed."""
    import os
    from PIL import Image
    from drivescenegen_amd import synth
    from drivescenegen_amd.dataset import Image_Dataset
    from drivescenegen_amd.train_loop import fit
    root = tmp_path / "pngs"
    root.mkdir()
    for k, r in enumerate(synth.synth_scene_rasters(4, 3, 64, 64, 3)):
        Image.fromarray(((r.transpose(1, 2, 0) * 0.5 + 0.5) * 255).round().astype(np.uint8)).save(root / f"{k}.png")
    out = tmp_path / "run"
    cfg = SimpleNamespace(dataset_name=str(root / "*"), patterns_size_height=64, patterns_size_width=64, mixed_precision="no",
                          gradient_accumulation_steps=1, output_dir=str(out), num_epochs=1, save_image_epochs=1,
                          save_model_epochs=1, eval_batch_size=2, seed=14555, learning_rate=1e-3)
    torch.manual_seed(3)
    net = synth_weights(d.UNet2DModel(**CFG1)).to(DEV)
    loader = torch.utils.data.DataLoader(Image_Dataset(cfg), batch_size=4, shuffle=True)
    opt = d.AdamW(net.parameters(), lr=cfg.learning_rate)
    lrs = d.get_cosine_schedule_with_warmup(optimizer=opt, num_warmup_steps=1, num_training_steps=2)
    sch = d.DDPMScheduler(thresholding=True, sample_max_value=1.5)
    assert fit(cfg, net, sch, opt, loader, lrs, sample_steps=4, ema=d.EMAModel(net.parameters())) == 1
    assert sorted(os.listdir(out / "samples")) == ["000.png"]
    saved = d.DDPMPipeline.from_pretrained(str(out))
    assert saved.scheduler.config.thresholding is True and saved.scheduler.config.sample_max_value == 1.5
