"""Prediction types, beta schedules, timestep spacings, zero terminal SNR and min-SNR weights without a GPU: the host tables
against tests/predtype_oracle.py bit for bit, the known-answer timestep tables, config round trips and swaps, every refusal that
stays, and the new C entries' argument checks (which run before any HIP call)."""
import ctypes
import json
import os

import pytest
import torch

import drivescenegen_amd as d
from drivescenegen_amd import _lib
from tests import predtype_oracle as po

SCHEDULES = ("linear", "scaled_linear", "squaredcos_cap_v2")


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("cls", [d.DDPMScheduler, d.DDIMScheduler], ids=["ddpm", "ddim"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_beta_tables_equal_the_restatement(lib_built, cls, schedule):
    s = cls(beta_schedule=schedule)
    want = po.betas(schedule)
    assert _bits(s.betas, want) and _bits(s.alphas_cumprod, po.alphas_cumprod(want))
    assert 0 < float(s.betas.min()) and float(s.betas.max()) <= float(torch.tensor(0.999, dtype=torch.float32))
    other = cls(beta_schedule=schedule, num_train_timesteps=250, beta_start=0.001, beta_end=0.05)
    assert _bits(other.betas, po.betas(schedule, 250, 0.001, 0.05))
    if schedule == "linear":
        assert _bits(s.betas, torch.linspace(0.0001, 0.02, 1000, dtype=torch.float32))
    else:
        assert not torch.equal(s.betas, cls().betas)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_zero_terminal_snr_table(lib_built, schedule):
    plain = d.DDIMScheduler(beta_schedule=schedule)
    zero = d.DDIMScheduler(beta_schedule=schedule, rescale_betas_zero_snr=True)
    assert _bits(zero.betas, po.rescale_zero_terminal_snr(po.betas(schedule)))
    assert _bits(zero.alphas_cumprod, po.alphas_cumprod(zero.betas))
    assert float(zero.alphas_cumprod[-1]) == 0.0 and float(plain.alphas_cumprod[-1]) > 0.0
    # the first entry is kept: exactly on the default table; on the other two the fp32 formula itself -- (a0 - aT) * (a0 / (a0 - aT)),
    # squared, then 1 - (1 - .) -- makes four roundings of a value just below 1, each at most 2^-24 relative
    first, kept = float(zero.alphas_cumprod[0]), float(plain.alphas_cumprod[0])
    assert first == kept if schedule == "linear" else abs(first - kept) <= 4 * 2.0 ** -24 * kept, (first, kept)
    assert bool((zero.alphas_cumprod[:-1] > 0).all())
    # DDPMScheduler has no such key (diffusers 0.20.0): unexpected as an argument, dropped by the swap
    with pytest.raises(TypeError, match="unexpected"):
        d.DDPMScheduler(rescale_betas_zero_snr=True)
    back = d.DDPMScheduler.from_config(zero.config)
    assert not hasattr(back.config, "rescale_betas_zero_snr") and _bits(back.betas, plain.betas)


KNOWN = [(50, "trailing", [999, 979, 959], [39, 19]), (50, "linspace", [999, 979, 958], [20, 0]),
         (7, "trailing", [999, 856, 713], [285, 142]), (750, "trailing", [999, 998, 996], [2, 0])]


@pytest.mark.parametrize("cls", [d.DDPMScheduler, d.DDIMScheduler], ids=["ddpm", "ddim"])
def test_timestep_known_answers(lib_built, cls):
    for steps, spacing, head, tail in KNOWN:
        s = cls(timestep_spacing=spacing)
        s.set_timesteps(steps)
        ts = s.timesteps.tolist()
        assert len(ts) == steps and ts[:3] == head and ts[-2:] == tail, (steps, spacing, ts[:3], ts[-2:])
        assert ts == po.timesteps(spacing, 1000, steps) and s.timesteps.dtype == torch.int64
        assert all(a > b for a, b in zip(ts, ts[1:])) and 0 <= ts[-1] and ts[0] <= 999
        # diffusers 0.20.0: the previous timestep is t - n_train // steps whatever the spacing (for 7 trailing steps 999 -> 857,
        # not the table's 856)
        for t in (ts[0], ts[len(ts) // 2], ts[-1]):
            assert s.previous_timestep(t) == t - 1000 // steps
    assert cls(timestep_spacing="trailing").previous_timestep(999) == 998       # (before set_timesteps: one training step)
    s = cls(timestep_spacing="trailing")
    s.set_timesteps(7)
    assert s.previous_timestep(999) == 857 and s.timesteps.tolist()[1] == 856
    # leading is what it was, steps_offset included; the offset belongs to leading alone
    lead = cls(steps_offset=1)
    lead.set_timesteps(50)
    assert lead.timesteps.tolist() == [20 * i + 1 for i in range(49, -1, -1)] == po.timesteps("leading", 1000, 50, 1)
    trail = cls(steps_offset=1, timestep_spacing="trailing")
    trail.set_timesteps(50)
    assert trail.timesteps.tolist() == po.timesteps("trailing", 1000, 50)
    cls().set_timesteps(750)
    with pytest.raises(ValueError, match="num_inference_steps"):
        cls(timestep_spacing="trailing").set_timesteps(1001)


NEW = dict(prediction_type="v_prediction", beta_schedule="squaredcos_cap_v2", timestep_spacing="trailing")


def test_config_round_trips_and_swaps(lib_built, tmp_path):
    ddim = d.DDIMScheduler(rescale_betas_zero_snr=True, clip_sample=False, **NEW)
    ddim.save_pretrained(str(tmp_path / "a"))
    cfg = json.load(open(os.path.join(str(tmp_path / "a"), "scheduler_config.json")))
    assert cfg["rescale_betas_zero_snr"] is True and all(cfg[k] == v for k, v in NEW.items())
    again = d.DDIMScheduler.from_pretrained(str(tmp_path / "a"))
    assert again.config.to_dict() == ddim.config.to_dict() and _bits(again.betas, ddim.betas)
    ddpm = d.DDPMScheduler(prediction_type="sample", beta_schedule="scaled_linear", timestep_spacing="linspace")
    ddpm.save_pretrained(str(tmp_path / "b"))
    assert d.DDPMScheduler.from_pretrained(str(tmp_path / "b")).config.to_dict() == ddpm.config.to_dict()
    # DDPM <-> DDIM keep the keys both have
    as_ddim = d.DDIMScheduler.from_config(ddpm.config)
    assert (as_ddim.config.prediction_type, as_ddim.config.beta_schedule, as_ddim.config.timestep_spacing) == (
        "sample", "scaled_linear", "linspace") and as_ddim.config.rescale_betas_zero_snr is False
    as_ddpm = d.DDPMScheduler.from_config(ddim.config)
    assert all(getattr(as_ddpm.config, k) == v for k, v in NEW.items()) and as_ddpm.config.clip_sample is False
    over = d.DDIMScheduler.from_config(d.DDPMScheduler().config, prediction_type="v_prediction", rescale_betas_zero_snr=True,
                                       timestep_spacing="trailing")
    assert over.config.prediction_type == "v_prediction" and float(over.alphas_cumprod[-1]) == 0.0
    # the defaults are what they were
    assert d.DDPMScheduler().config.to_dict() == dict(
        num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
        variance_type="fixed_small", clip_sample=True, prediction_type="epsilon", thresholding=False,
        dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0, timestep_spacing="leading", steps_offset=0)
    assert d.DDIMScheduler().config.rescale_betas_zero_snr is False and d.DDIMScheduler().config.prediction_type == "epsilon"
    # a pipeline folder carries the keys (model_index.json + scheduler/scheduler_config.json), no pipeline code involved
    from tests.common import CFG1
    d.DDIMPipeline(d.UNet2DModel(**CFG1), ddim).save_pretrained(str(tmp_path / "pipe"))
    loaded = json.load(open(os.path.join(str(tmp_path / "pipe"), "scheduler", "scheduler_config.json")))
    assert loaded["prediction_type"] == "v_prediction" and loaded["rescale_betas_zero_snr"] is True


def test_the_swap_into_the_other_samplers_is_as_before(lib_built):
    for key, value in NEW.items():
        src = d.DDIMScheduler(**{key: value})
        if key == "timestep_spacing":          # (a key DPM-Solver++ runs at all three values)
            assert d.DPMSolverMultistepScheduler.from_config(src.config).config.timestep_spacing == "trailing"
        else:
            with pytest.raises(NotImplementedError, match=key):
                d.DPMSolverMultistepScheduler.from_config(src.config)
        if key == "beta_schedule":
            with pytest.raises(NotImplementedError, match=key):
                d.RePaintScheduler.from_config(src.config)
        else:                                   # RePaint's config has no such key: dropped
            assert not hasattr(d.RePaintScheduler.from_config(src.config).config, key)
    zero = d.DDIMScheduler(rescale_betas_zero_snr=True)
    for cls in (d.DPMSolverMultistepScheduler, d.RePaintScheduler):
        other = cls.from_config(zero.config)
        assert not hasattr(other.config, "rescale_betas_zero_snr") and _bits(other.betas, d.DDPMScheduler().betas)


def test_the_refusals_that_stay(lib_built):
    for cls in (d.DDPMScheduler, d.DDIMScheduler):
        for kw in (dict(prediction_type="v_prediction"), dict(prediction_type="sample"), dict(beta_schedule="scaled_linear"),
                   dict(beta_schedule="squaredcos_cap_v2"), dict(timestep_spacing="trailing"), dict(timestep_spacing="linspace")):
            with pytest.raises(NotImplementedError, match=next(iter(kw))):
                cls(thresholding=True, **kw)
        with pytest.raises(NotImplementedError, match="trained_betas"):
            cls(trained_betas=[0.1, 0.2])
        with pytest.raises(NotImplementedError, match="beta_schedule"):
            cls(beta_schedule="sigmoid")
        with pytest.raises(NotImplementedError, match="timestep_spacing"):
            cls(timestep_spacing="karras")
        for bad in ("v", "eps", None, 2):
            with pytest.raises(ValueError, match="prediction_type"):
                cls(prediction_type=bad)
    with pytest.raises(NotImplementedError, match="rescale_betas_zero_snr"):
        d.DDIMScheduler(thresholding=True, rescale_betas_zero_snr=True)
    for vt in ("fixed_large", "learned", "learned_range"):
        with pytest.raises(NotImplementedError, match="variance_type"):
            d.DDPMScheduler(variance_type=vt)
    with pytest.raises(TypeError, match="unexpected"):
        d.DDIMScheduler(variance_type="fixed_small")
    for kw in (dict(prediction_type="v_prediction"), dict(prediction_type="sample"), dict(beta_schedule="scaled_linear"),
               dict(trained_betas=[0.1])):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            d.DPMSolverMultistepScheduler(**kw)
    with pytest.raises(TypeError, match="unexpected"):
        d.RePaintScheduler(prediction_type="v_prediction")
    for kw in (dict(beta_schedule="scaled_linear"), dict(trained_betas=[0.1])):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            d.RePaintScheduler(**kw)
    with pytest.raises(NotImplementedError, match="use_clipped_model_output"):
        d.DDIMScheduler(prediction_type="v_prediction").step(torch.zeros(1, 3, 8, 8), 10, torch.zeros(1, 3, 8, 8),
                                                            use_clipped_model_output=True)


def test_snr_weights(lib_built):
    for pred in ("epsilon", "sample", "v_prediction"):
        for cls, kw in ((d.DDPMScheduler, {}), (d.DDIMScheduler, dict(beta_schedule="squaredcos_cap_v2"))):
            s = cls(prediction_type=pred, **kw)
            w = s.snr_weights(5.0)
            assert _bits(w, po.snr_weights(s.alphas_cumprod, 5.0, pred)) and w.shape == (1000,)
            assert s.snr_weights(5.0) is w and s.snr_weights(5) is w            # cached
            assert bool(torch.isfinite(w).all()) and bool((w > 0).all())
            assert not torch.equal(s.snr_weights(1.0), w)
    # the shapes the paper describes: eps weights are 1 where snr <= gamma and fall where it is larger; v weights stay <= 1
    e = d.DDPMScheduler().snr_weights(5.0)
    assert float(e[-1]) == 1.0 and float(e[0]) < 1e-3 and bool((e <= 1.0).all())
    assert bool((d.DDPMScheduler(prediction_type="v_prediction").snr_weights(5.0) <= 1.0).all())
    assert float(d.DDPMScheduler(prediction_type="sample").snr_weights(5.0).max()) == 5.0
    # zero terminal SNR: v and sample have a weight at every timestep (0 at the last), epsilon has none
    for pred in ("sample", "v_prediction"):
        z = d.DDIMScheduler(rescale_betas_zero_snr=True, prediction_type=pred)
        w = z.snr_weights(5.0)
        assert _bits(w, po.snr_weights(z.alphas_cumprod, 5.0, pred)) and float(w[-1]) == 0.0 and bool(torch.isfinite(w).all())
    with pytest.raises(ValueError, match="zero-terminal-SNR"):
        d.DDIMScheduler(rescale_betas_zero_snr=True).snr_weights(5.0)
    for gamma in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            d.DDPMScheduler().snr_weights(gamma)
    # schedulers without the key weigh as epsilon predictors
    assert _bits(d.RePaintScheduler().snr_weights(5.0), e)


def test_abi_refuses_bad_arguments_before_any_hip_call(lib_built):
    """(addresses that are never dereferenced: every call below is refused before any HIP call)"""
    lib = _lib.load()
    for name in ("dsg_ddpm_step_pt", "dsg_ddim_step_pt", "dsg_add_noise_target", "dsg_add_noise_target_philox",
                 "dsg_mse_loss_weighted"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert (_lib.DSG_PRED_EPSILON, _lib.DSG_PRED_SAMPLE, _lib.DSG_PRED_V) == (0, 1, 2)
    assert _lib.PRED_CODES == dict(epsilon=0, sample=1, v_prediction=2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsg.h")).read()
    assert "DSG_PRED_EPSILON = 0, DSG_PRED_SAMPLE = 1, DSG_PRED_V = 2" in header
    X, M, Z, P, T = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    numel = 4096

    def ddpm(**kw):
        a = dict(sample=X, mo=M, noise=Z, prev=P, numel=numel, pred=2)
        a.update(kw)
        return lib.dsg_ddpm_step_pt(a["sample"], a["mo"], a["noise"], a["prev"], a["numel"], a["pred"], 0.5, 0.5, 1.0, 0.1, 0.9,
                                    0.01, None)

    def ddim(**kw):
        a = dict(sample=X, mo=M, prev=P, numel=numel, pred=2)
        a.update(kw)
        return lib.dsg_ddim_step_pt(a["sample"], a["mo"], a["prev"], a["numel"], a["pred"], 0.5, 0.5, 1.0, 0.9, 0.1, None)

    for call in (ddpm, ddim):
        for kw, word in [(dict(sample=None), b"NULL"), (dict(mo=None), b"NULL"), (dict(prev=None), b"NULL"),
                         (dict(numel=0), b"positive"), (dict(numel=-4), b"positive"), (dict(pred=3), b"pred_type"),
                         (dict(pred=-1), b"pred_type"), (dict(prev=X), b"overlap"), (dict(prev=M + numel * 4 - 4), b"overlap"),
                         (dict(prev=X - numel * 4 + 4), b"overlap")]:
            assert call(**kw) == -1, (call.__name__, kw)
            assert word in lib.dsg_last_error(), (call.__name__, kw, lib.dsg_last_error())
    assert ddpm(prev=Z + 8) == -1 and b"overlap" in lib.dsg_last_error()

    n, per = 4, 1024
    SA, SB = 0x600000, 0x700000
    nbytes = n * per * 4

    def target(**kw):
        a = dict(x0=X, noise=Z, sa=SA, sb=SB, noisy=P, target=T, n=n, per=per)
        a.update(kw)
        return lib.dsg_add_noise_target(a["x0"], a["noise"], a["sa"], a["sb"], a["noisy"], a["target"], a["n"], a["per"], None)

    def philox(**kw):
        a = dict(x0=X, sa=SA, sb=SB, noisy=P, target=T, n=n, per=per)
        a.update(kw)
        return lib.dsg_add_noise_target_philox(a["x0"], a["sa"], a["sb"], a["noisy"], a["target"], a["n"], a["per"], 1, 2, None)

    for call in (target, philox):
        for kw, word in [(dict(x0=None), b"NULL"), (dict(sa=None), b"NULL"), (dict(sb=None), b"NULL"),
                         (dict(noisy=None, target=None), b"both NULL"), (dict(n=0), b"bad dims"), (dict(n=-1), b"bad dims"),
                         (dict(per=0), b"bad dims"), (dict(per=-3), b"bad dims"), (dict(noisy=X), b"overlap"),
                         (dict(target=X + nbytes - 4), b"overlap"), (dict(target=SA), b"overlap"), (dict(noisy=SB - nbytes + 4), b"overlap"),
                         (dict(noisy=T), b"overlap"), (dict(noisy=T + nbytes - 4), b"overlap")]:
            assert call(**kw) == -1, (call.__name__, kw)
            assert word in lib.dsg_last_error(), (call.__name__, kw, lib.dsg_last_error())
    assert target(noise=None) == -1 and b"NULL" in lib.dsg_last_error()
    assert target(target=Z) == -1 and b"overlap" in lib.dsg_last_error()

    W, L, D, WS = 0x800000, 0x900000, 0xA00000, 0xB00000

    def wloss(**kw):
        a = dict(pred=X, target=M, w=W, n=n, per=per, loss=L, dpred=D, ws=WS, wsb=2048 * 8)
        a.update(kw)
        return lib.dsg_mse_loss_weighted(a["pred"], a["target"], a["w"], a["n"], a["per"], 1.0, a["loss"], a["dpred"], a["ws"],
                                         a["wsb"], None)

    for kw, word in [(dict(pred=None), b"NULL"), (dict(target=None), b"NULL"), (dict(w=None), b"NULL"), (dict(loss=None), b"NULL"),
                     (dict(ws=None), b"NULL"), (dict(n=0), b"bad dims"), (dict(per=0), b"bad dims"), (dict(per=-1), b"bad dims")]:
        assert wloss(**kw) == -1, kw
        assert word in lib.dsg_last_error(), (kw, lib.dsg_last_error())
    assert wloss(wsb=8) == -3 and b"workspace" in lib.dsg_last_error()          # DSG_ERR_WORKSPACE_TOO_SMALL
    assert wloss(wsb=0) == -3


def test_cpu_tensors_are_refused(lib_built):
    x, t = torch.zeros(2, 3, 8, 8), torch.tensor([1, 2])
    for cls in (d.DDPMScheduler, d.DDIMScheduler):
        for pred in ("sample", "v_prediction"):
            with pytest.raises(RuntimeError, match="HIP engine"):
                cls(prediction_type=pred).step(x, 10, x)
    s = d.DDPMScheduler(prediction_type="v_prediction")
    with pytest.raises(RuntimeError, match="HIP engine"):
        s.get_velocity(x, x, t)
    with pytest.raises(RuntimeError, match="HIP engine"):
        s.add_noise_velocity(x, x, t)
    with pytest.raises(RuntimeError, match="HIP engine"):
        s.add_noise_velocity_device(x, t, 1, 0)
    with pytest.raises(RuntimeError, match="HIP engine"):
        d.mse_loss(x, x, weights=torch.ones(2))
    assert d.DPMSolverMultistepScheduler.get_velocity is d.DDPMScheduler.get_velocity
    assert isinstance(ctypes.c_int32(_lib.PRED_CODES["v_prediction"]).value, int)
