"""Dynamic thresholding without a GPU: tests/dynthresh_oracle.py against ``torch.quantile`` (diffusers 0.20.0's
``_threshold_sample``, restated here in torch) bit for bit, the schedulers' configuration handling, and the C entries' argument
checks (which run before any HIP call)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import drivescenegen_amd as d
from drivescenegen_amd import _lib
from tests import dynthresh_oracle as dto

F = np.float32
QS = (0.5, 0.9, 0.995, 0.999)
# per -> rows: 304 rows per ratio, 1216 in all
GRID = {35: 64, 105: 64, 1024: 64, 1116: 64, 4096: 32, 262144: 16}


def _torch_scale(abs_rows, q, max_value):
    """diffusers 0.20.0 ``_threshold_sample`` up to s: quantile over each sample's magnitudes, clamped into [1, max]."""
    s = torch.quantile(torch.from_numpy(abs_rows), q, dim=1)
    return torch.clamp(s, min=1, max=max_value).numpy()


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_oracle_scale_is_torch_quantile_bit_for_bit_on_random_rows():
    """1216 random rows (magnitudes of a normal draw scaled so that the quantile lands below 1, inside and above the maximum)."""
    rows = 0
    for pi, (per, n) in enumerate(GRID.items()):
        rng = np.random.default_rng(100 + pi)
        base = rng.standard_normal((n, per)).astype(F)
        base *= rng.choice(np.array([0.2, 0.6, 1.0, 4.0], dtype=F), size=(n, 1))
        a = np.abs(base)
        for q in QS:
            got, want = dto.scale_of_abs(a, q, 2.0), _torch_scale(a, q, 2.0)
            assert _same_bits(got, want), (per, q, int((got != want).sum()))
            # the UNCLAMPED quantile too (a maximum nothing reaches, no lower clamp to hide behind: values far below 1 scaled up)
            big = a * F(1000.0)
            assert _same_bits(dto.scale_of_abs(big, q, 3e38), _torch_scale(big, q, 3e38)), (per, q)
            rows += n
    assert rows == 1216


def test_oracle_scale_on_constructed_rows():
    per = 1000
    equal = np.full((1, per), 1.37, dtype=F)
    zero = np.zeros((1, per), dtype=F)
    k_lo, k_hi, w = dto.ranks(per, 0.9)
    assert (k_lo, k_hi) == (899, 900) and 0 < w < 1
    two = np.full((1, per), 1.25, dtype=F)
    two[0, :k_lo + 1] = 1.0                    # sorted: ranks 0..k_lo hold 1.0, k_hi.. hold 1.25 -- the ranks straddle the jump
    two = two[:, np.random.default_rng(0).permutation(per)]
    for q in (0.9, 1.0, 0.0, 0.5, 0.995):
        for rows in (equal, two, zero):
            for mx in (1.0, 2.0):
                assert _same_bits(dto.scale_of_abs(rows, q, mx), _torch_scale(rows, q, mx)), (q, mx)
    assert dto.scale_of_abs(zero, 0.995, 2.0)[0] == 1.0
    assert dto.scale_of_abs(equal, 0.995, 2.0)[0] == F(1.37)
    s = dto.scale_of_abs(two, 0.9, 2.0)[0]
    assert 1.0 < s < 1.25
    assert dto.scale_of_abs(two, 1.0, 2.0)[0] == 1.25 and dto.scale_of_abs(two, 0.0, 2.0)[0] == 1.0
    assert dto.ranks(per, 1.0) == (per - 1, per - 1, 0) and dto.ranks(per, 0.0) == (0, 0, 0)
    # a NaN makes the row's answer NaN, as torch's; the row beside it is untouched
    rows = np.abs(np.random.default_rng(1).standard_normal((3, 105)).astype(F)) * F(1.5)
    rows[1, 17] = np.nan
    got, want = dto.scale_of_abs(rows, 0.9, 2.0), _torch_scale(rows, 0.9, 2.0)
    assert np.isnan(got[1]) and np.isnan(want[1]) and _same_bits(got, want)


def test_oracle_fmaf_rounds_once():
    # a*b + c whose fp64 sum is exact: compare with the exact rational value rounded to fp32
    from fractions import Fraction
    rng = np.random.default_rng(5)
    for _ in range(2000):
        a, b, c = (F(v) for v in rng.standard_normal(3) * 10.0 ** rng.integers(-3, 4))
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        lo = F(float(exact))                          # candidate; correct unless the double rounding bit
        cands = [np.nextafter(lo, F(-np.inf)), lo, np.nextafter(lo, F(np.inf))]
        best = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))
        got = dto.fmaf(a, b, c)
        assert abs(Fraction(float(got)) - exact) == abs(Fraction(float(best)) - exact), (a, b, c)
    # the double-rounding case itself: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 sits half way between two fp32 values; the 2^-60 decides,
    # and a plain fp64 sum has dropped it before the rounding to fp32 (ties to even: down)
    a = F(1 + 2.0 ** -12)
    assert dto.fmaf(a, a, F(2.0 ** -60)) == F(1 + 2.0 ** -11 + 2.0 ** -23)
    assert dto.fmaf(a, a, F(-2.0 ** -60)) == F(1 + 2.0 ** -11)
    assert dto.fmaf(a, a, F(0)) == F(1 + 2.0 ** -11)


def test_the_schedulers_accept_thresholding(lib_built, tmp_path):
    ddpm = d.DDPMScheduler(thresholding=True, sample_max_value=2.0)
    ddim = d.DDIMScheduler(thresholding=True, sample_max_value=2.0)
    for s in (ddpm, ddim):
        assert s.config.thresholding is True and s.config.sample_max_value == 2.0 and s.config.dynamic_thresholding_ratio == 0.995
    for q in (0.0, 0.5, 1.0):
        assert d.DDIMScheduler(thresholding=True, dynamic_thresholding_ratio=q).config.dynamic_thresholding_ratio == q
    # the ratio and the maximum are plain config values when thresholding is off, too
    assert d.DDPMScheduler(dynamic_thresholding_ratio=0.9, sample_max_value=1.5).config.thresholding is False
    # the rank scalars are torch.quantile's, memoised
    s = d.DDIMScheduler(thresholding=True, dynamic_thresholding_ratio=0.9)
    assert s.threshold_ranks(1000) == (899, 900, float(F(0.9) * F(999) - F(899))) and s.threshold_ranks(1000) is s.threshold_ranks(1000)
    for per in (1, 35, 105, 1024, 262144):
        for q in (0.0, 0.5, 0.995, 1.0):
            k_lo, k_hi, w = d.DDPMScheduler(thresholding=True, dynamic_thresholding_ratio=q).threshold_ranks(per)
            o = dto.ranks(per, q)
            assert (k_lo, k_hi) == o[:2] and F(w) == o[2] and 0 <= k_lo <= k_hi < per and k_hi - k_lo <= 1
    # save / load / swap
    ddim = d.DDIMScheduler(thresholding=True, sample_max_value=1.5, dynamic_thresholding_ratio=0.99, clip_sample=False)
    ddim.save_pretrained(str(tmp_path / "a"))
    cfg = json.load(open(os.path.join(str(tmp_path / "a"), "scheduler_config.json")))
    assert cfg["thresholding"] is True and cfg["sample_max_value"] == 1.5 and cfg["dynamic_thresholding_ratio"] == 0.99
    assert d.DDIMScheduler.from_pretrained(str(tmp_path / "a")).config.to_dict() == ddim.config.to_dict()
    ddpm = d.DDPMScheduler(thresholding=True, sample_max_value=2.0, dynamic_thresholding_ratio=0.9)
    ddpm.save_pretrained(str(tmp_path / "b"))
    assert d.DDPMScheduler.from_pretrained(str(tmp_path / "b")).config.to_dict() == ddpm.config.to_dict()
    swapped = d.DDIMScheduler.from_config(ddpm.config)
    assert (swapped.config.thresholding, swapped.config.sample_max_value, swapped.config.dynamic_thresholding_ratio) == (True, 2.0, 0.9)
    plain = d.DDIMScheduler.from_config(d.DDPMScheduler().config, thresholding=True, sample_max_value=1.5)     # README's line
    assert plain.config.thresholding is True and plain.config.sample_max_value == 1.5
    back = d.DDPMScheduler.from_config(swapped.config)
    assert back.config.thresholding is True and back.config.sample_max_value == 2.0


@pytest.mark.parametrize("cls", [d.DDPMScheduler, d.DDIMScheduler], ids=["ddpm", "ddim"])
@pytest.mark.parametrize("kw", [dict(dynamic_thresholding_ratio=-0.1), dict(dynamic_thresholding_ratio=1.01),
                                dict(dynamic_thresholding_ratio=float("nan")), dict(sample_max_value=0.99),
                                dict(sample_max_value=0.0), dict(sample_max_value=float("nan")), dict(sample_max_value=float("inf")),
                                dict(thresholding=True, sample_max_value=0.5), dict(thresholding=True, dynamic_thresholding_ratio=2)])
def test_out_of_range_values_raise(lib_built, cls, kw):
    with pytest.raises(ValueError, match="dynamic_thresholding_ratio|sample_max_value"):
        cls(**kw)


def test_the_other_refusals_stand(lib_built):
    for kw in (dict(thresholding=True), dict(dynamic_thresholding_ratio=0.9), dict(sample_max_value=2.0)):
        with pytest.raises(TypeError, match="unexpected"):
            d.RePaintScheduler(**kw)
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            d.DPMSolverMultistepScheduler(**kw)
    thr = d.DDIMScheduler(thresholding=True, sample_max_value=2.0)
    with pytest.raises(NotImplementedError, match="thresholding"):
        d.DPMSolverMultistepScheduler.from_config(thr.config)
    # RePaint's config has no such key (diffusers): the swap drops it, and the class has no thresholded step
    rp = d.RePaintScheduler.from_config(thr.config)
    assert not hasattr(rp.config, "thresholding") and d.RePaintScheduler.step is not d.DDIMScheduler.step
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="use_clipped_model_output"):
        thr.step(x, 10, x, use_clipped_model_output=True)
    with pytest.raises(RuntimeError, match="HIP engine"):
        thr.step(x, 10, x)
    with pytest.raises(RuntimeError, match="HIP engine"):
        d.DDPMScheduler(thresholding=True).step(x, 10, x)
    for kw in (dict(prediction_type="v_prediction"), dict(beta_schedule="scaled_linear"), dict(timestep_spacing="trailing")):
        with pytest.raises(NotImplementedError):
            d.DDPMScheduler(thresholding=True, **kw)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def _ws_bytes(lib, n):
    b = ctypes.c_size_t()
    assert lib.dsg_dynthresh_workspace_bytes(n, ctypes.byref(b)) == 0
    return b.value


def test_abi_refuses_bad_arguments_before_any_hip_call(lib_built):
    """(addresses that are never dereferenced: every call below is refused before any HIP call)"""
    lib = _lib.load()
    for name in ("dsg_dynthresh_workspace_bytes", "dsg_dynthresh_scale", "dsg_ddpm_step_thr", "dsg_ddim_step_thr"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dsg_dynthresh_workspace_bytes(2, None) == -1 and b"NULL" in lib.dsg_last_error()
    b = ctypes.c_size_t()
    for n in (0, -1, 65536):
        assert lib.dsg_dynthresh_workspace_bytes(n, ctypes.byref(b)) == -1
    one, four = _ws_bytes(lib, 1), _ws_bytes(lib, 4)
    assert one > 0 and one % 4 == 0 and four == 4 * one

    n, per = 4, 1024
    X, E, S, W = 0x100000, 0x200000, 0x300000, 0x400000
    in_bytes = n * per * 4

    def scale(**kw):
        a = dict(sample=X, eps=E, s=S, n=n, per=per, sb=0.5, sa=0.5, k_lo=1017, k_hi=1018, w=0.25, mx=2.0, ws=W, wsb=four)
        a.update(kw)
        return lib.dsg_dynthresh_scale(a["sample"], a["eps"], a["s"], a["n"], a["per"], a["sb"], a["sa"], a["k_lo"], a["k_hi"],
                                       a["w"], a["mx"], a["ws"], a["wsb"], None)

    cases = [(dict(sample=None), b"NULL"), (dict(eps=None), b"NULL"), (dict(s=None), b"NULL"), (dict(ws=None), b"NULL"),
             (dict(n=0), b"n="), (dict(n=-2), b"n="), (dict(per=0), b"per_sample"), (dict(per=-8), b"per_sample"),
             (dict(per=2 ** 31), b"per_sample"),
             (dict(k_lo=-1, k_hi=0), b"rank"), (dict(k_lo=1023, k_hi=1024), b"rank"), (dict(k_lo=1024, k_hi=1024), b"rank"),
             (dict(k_lo=5, k_hi=7), b"rank"), (dict(k_lo=6, k_hi=5), b"rank"),
             (dict(w=-0.1), b"weight"), (dict(w=1.0), b"weight"), (dict(w=float("nan")), b"weight"),
             (dict(mx=0.5), b"sample_max_value"), (dict(mx=float("nan")), b"sample_max_value"),
             (dict(ws=W + 2), b"aligned"),
             (dict(s=X), b"overlap"), (dict(s=X + in_bytes - 4), b"overlap"), (dict(s=X - 12), b"overlap"), (dict(s=E + 64), b"overlap"),
             (dict(ws=X + 4), b"overlap"), (dict(ws=E - four + 4), b"overlap"), (dict(ws=E + in_bytes - 4), b"overlap"),
             (dict(ws=S), b"overlap"), (dict(ws=S - four + 4), b"overlap"), (dict(s=W + four - 4), b"overlap")]
    for kw, word in cases:
        assert scale(**kw) == -1, kw
        assert word in lib.dsg_last_error(), (kw, lib.dsg_last_error())
    assert scale(wsb=four - 4) == -3 and b"workspace" in lib.dsg_last_error()       # DSG_ERR_WORKSPACE_TOO_SMALL
    assert scale(wsb=0) == -3

    numel = n * per

    def ddpm(**kw):
        a = dict(sample=X, eps=E, noise=None, thr=S, prev=W, numel=numel, per=per)
        a.update(kw)
        return lib.dsg_ddpm_step_thr(a["sample"], a["eps"], a["noise"], a["thr"], a["prev"], a["numel"], a["per"], 0.5, 0.5, 0.1,
                                     0.9, 0.01, None)

    def ddim(**kw):
        a = dict(sample=X, eps=E, thr=S, prev=W, numel=numel, per=per)
        a.update(kw)
        return lib.dsg_ddim_step_thr(a["sample"], a["eps"], a["thr"], a["prev"], a["numel"], a["per"], 0.5, 0.5, 0.9, 0.1, None)

    for call in (ddpm, ddim):
        for kw, word in [(dict(sample=None), b"NULL"), (dict(eps=None), b"NULL"), (dict(thr=None), b"NULL"), (dict(prev=None), b"NULL"),
                         (dict(numel=0), b"positive"), (dict(numel=-4), b"positive"), (dict(per=0), b"per_sample"),
                         (dict(per=-1), b"per_sample"), (dict(per=1000), b"per_sample"), (dict(per=2 * numel), b"per_sample"),
                         (dict(prev=S), b"overlap"), (dict(prev=S + 12), b"overlap"), (dict(prev=S - numel * 4 + 4), b"overlap")]:
            assert call(**kw) == -1, (call.__name__, kw)
            assert word in lib.dsg_last_error(), (call.__name__, kw, lib.dsg_last_error())
