"""DPM-Solver++ multistep -- everything that needs no GPU: the timestep tables against stated properties and a committed
fixture, the order bookkeeping, the host scalars against the NumPy restatement (tests/dpmsolver_oracle.py) bit for bit, order 1
against the oracle's DDIM step, the convergence orders on a model with a known answer, config I/O and its refusals, and the C
ABI's argument checks (made before any HIP call)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import drivescenegen_amd as d
from drivescenegen_amd import _lib
from tests import dpmsolver_oracle as do
from tests.common import CFG1

HERE = os.path.dirname(os.path.abspath(__file__))
SPACINGS = ("linspace", "leading", "trailing")
COUNTS = (1, 2, 14, 15, 20, 50, 750, 1000)
F = np.float32


# ---- timestep tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", SPACINGS)
def test_timestep_tables(lib_built, spacing):
    golden = json.load(open(os.path.join(HERE, "golden", "dpmsolver_timesteps.json")))
    s = d.DPMSolverMultistepScheduler(timestep_spacing=spacing)
    for n in COUNTS:
        s.set_timesteps(n)
        ts = s.timesteps.numpy()
        assert ts.dtype == np.int64 and 1 <= len(ts) <= n and s.num_inference_steps == len(ts), (spacing, n)
        assert (np.diff(ts) < 0).all() and ts.min() >= 0 and ts.max() <= 999, (spacing, n)
        assert np.array_equal(ts, do.timesteps(n, spacing)), (spacing, n)
        assert ts.tolist() == golden[f"{spacing}/{n}"], (spacing, n)
        assert s.lower_order_nums == 0
    if spacing == "leading":
        s.set_timesteps(20)
        assert s.timesteps.tolist() == list(range(940, 0, -47))
        o = d.DPMSolverMultistepScheduler(timestep_spacing="leading", steps_offset=1)
        o.set_timesteps(20)
        assert o.timesteps.tolist() == list(range(941, 1, -47))
    if spacing == "linspace":
        s.set_timesteps(10)
        assert s.timesteps.tolist() == [999, 899, 799, 699, 599, 500, 400, 300, 200, 100]
    if spacing == "trailing":
        s.set_timesteps(10)
        assert s.timesteps.tolist() == [999, 899, 799, 699, 599, 499, 399, 299, 199, 99]
    with pytest.raises(ValueError):
        s.set_timesteps(1001)
    with pytest.raises(ValueError):
        s.set_timesteps(0)


# ---- order bookkeeping ------------------------------------------------------------------------------------------------------
ORDER_GRID = [
    (3, 10, True, [1, 2, 3, 3, 3, 3, 3, 3, 2, 1]),
    (3, 20, True, [1, 2] + [3] * 18),
    (3, 10, False, [1, 2] + [3] * 8),
    (3, 14, True, [1, 2] + [3] * 10 + [2, 1]),
    (3, 15, True, [1, 2] + [3] * 13),
    (2, 10, True, [1] + [2] * 8 + [1]),
    (2, 10, False, [1] + [2] * 9),
    (2, 20, True, [1] + [2] * 19),
    (1, 10, True, [1] * 10),
    (3, 2, True, [1, 1]),
    (3, 3, True, [1, 2, 1]),
    (2, 1, True, [1]),
]


@pytest.mark.parametrize("solver_order,L,lof,want", ORDER_GRID)
def test_order_bookkeeping(lib_built, solver_order, L, lof, want):
    assert do.orders(solver_order, L, lof) == want
    s = d.DPMSolverMultistepScheduler(solver_order=solver_order, lower_order_final=lof)
    s.set_timesteps(L)
    assert len(s.timesteps) == L
    got = []
    for i in range(L):                      # the scheduler's own decision, advanced as step() advances it
        got.append(s._order_at(i))
        s.lower_order_nums = min(s.lower_order_nums + 1, solver_order)
    assert got == want
    s.set_timesteps(L)
    assert s.lower_order_nums == 0


# ---- host scalars ---------------------------------------------------------------------------------------------------------
KEYS = ("sigma_s", "alpha_s", "inv_r0", "inv_r1", "q", "p", "kx", "c0", "c1", "c2", "cn")


def test_tables_equal_the_restatement(lib_built):
    s = d.DPMSolverMultistepScheduler()
    tb = do.tables(F)
    assert np.array_equal(s.alphas_cumprod.numpy(), tb["acp"])
    assert np.array_equal(s.alpha_t.numpy(), tb["alpha"]) and np.array_equal(s.sigma_t.numpy(), tb["sigma"])
    assert np.array_equal(s.lambda_t.numpy(), tb["lam"]) and s.lambda_t.dtype == torch.float32
    assert (np.diff(tb["lam"]) < 0).all()       # the half log-SNR falls with t: every h of a run is positive


@pytest.mark.parametrize("algorithm", do.ALGORITHMS)
@pytest.mark.parametrize("solver_type", do.SOLVER_TYPES)
def test_host_scalars_equal_the_numpy_restatement(lib_built, algorithm, solver_type):
    """Every scalar the kernel is given, for every step of runs of 5, 10, 20 and 50 steps in each spacing, at every order the
    run uses there: the scheduler (torch 0-d fp32 arithmetic) against NumPy fp32, bit for bit."""
    tb = do.tables(F)
    max_order = 2 if algorithm == "sde-dpmsolver++" else 3
    checked = 0
    for spacing in SPACINGS:
        s = d.DPMSolverMultistepScheduler(solver_order=max_order, algorithm_type=algorithm, solver_type=solver_type,
                                          timestep_spacing=spacing)
        for n in (5, 10, 20, 50):
            s.set_timesteps(n)
            ts = s.timesteps.tolist()
            for i, s0 in enumerate(ts):
                t = ts[i + 1] if i + 1 < len(ts) else 0
                for order in range(1, min(max_order, i + 1) + 1):
                    s1 = ts[i - 1] if order >= 2 else None
                    s2 = ts[i - 2] if order >= 3 else None
                    got = s.step_scalars(s0, t, s1, s2, order)
                    want = do.step_scalars(s0, t, s1, s2, order, algorithm, solver_type, tb, F)
                    assert set(got) == set(KEYS) == set(want)
                    for k in KEYS:
                        assert np.isfinite(want[k]) and got[k] == float(want[k]), (spacing, n, s0, order, k, got[k], want[k])
                    checked += 1
    assert checked > 400


# ---- order 1 is DDIM --------------------------------------------------------------------------------------------------------
def test_first_order_is_ddim():
    """The oracle's order-1 step against oracle/scheduler_oracle.py's DDIM step (eta = 0, no clip) in float64, over 50 random
    (t, prev_t) pairs with prev_t >= 0: 1e-12 relative."""
    from oracle.scheduler_oracle import OracleDDIMScheduler
    tb = do.tables(np.float64)
    ddim = OracleDDIMScheduler(clip_sample=False)
    ddim.alphas_cumprod = torch.from_numpy(tb["acp"].copy())            # the same float64 table on both sides
    rng = np.random.default_rng(0)
    for _ in range(50):
        t = int(rng.integers(1, 1000))
        prev_t = int(rng.integers(0, t))
        x, e = rng.standard_normal((2, 3, 4, 5)), rng.standard_normal((2, 3, 4, 5))
        ddim._prev = lambda _t, p=prev_t: p
        want = ddim.step(torch.from_numpy(e), t, torch.from_numpy(x)).prev_sample.numpy()
        assert want.dtype == np.float64
        s = do.step_scalars(t, prev_t, order=1, tabs=tb, dtype=np.float64)
        got, _ = do.step(x, e, None, None, None, s, 1, dtype=np.float64)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (t, prev_t)


# ---- convergence ------------------------------------------------------------------------------------------------------------
def _end_error(n, solver_order, solver_type):
    tb = do.tables(np.float64)
    x_T = np.array([1.3, -0.7])
    got = do.run(lambda x, t: do.analytic_eps(x, t, tb, np.float64), x_T, n, solver_order=solver_order,
                 solver_type=solver_type, lower_order_final=True, spacing="linspace", dtype=np.float64)
    want = do.analytic_end(x_T, int(do.timesteps(n, "linspace")[0]), tb)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def test_convergence_orders_on_a_model_with_a_known_answer():
    """Data ~ N(0, 0.25): the optimal predictor and the exact ODE solution are closed forms.  Relative end error at 80, 160 and
    320 steps (linspace, lower_order_final, float64): order 1 halves per doubling, order 2 quarters, order 3 does better."""
    err = {(o, st): [_end_error(n, o, st) for n in (80, 160, 320)]
           for o, st in ((1, "midpoint"), (2, "midpoint"), (2, "heun"), (3, "midpoint"))}
    ratio = {k: (v[0] / v[1], v[1] / v[2]) for k, v in err.items()}
    for k in err:
        print(k, ["%.3e" % e for e in err[k]], "ratios %.2f %.2f" % ratio[k])
    assert all(1.8 <= r <= 2.2 for r in ratio[(1, "midpoint")])
    for st in do.SOLVER_TYPES:
        assert all(r >= 3.5 for r in ratio[(2, st)]), (st, ratio[(2, st)])
    assert ratio[(3, "midpoint")][1] >= 6
    for i in (1, 2):
        assert err[(3, "midpoint")][i] < min(err[(2, "midpoint")][i], err[(2, "heun")][i])


# ---- config ---------------------------------------------------------------------------------------------------------------
def test_config_round_trip(lib_built, tmp_path):
    s = d.DPMSolverMultistepScheduler(solver_order=3, solver_type="heun", timestep_spacing="trailing", beta_end=0.03,
                                      lower_order_final=False, steps_offset=2)
    assert s.order == 1 and s.config.algorithm_type == "dpmsolver++" and s.init_noise_sigma == 1.0
    s.save_pretrained(str(tmp_path))
    cfg = json.load(open(os.path.join(str(tmp_path), "scheduler_config.json")))
    assert cfg["_class_name"] == "DPMSolverMultistepScheduler" and cfg["solver_order"] == 3 and cfg["solver_type"] == "heun"
    assert cfg["lambda_min_clipped"] == -float("inf") and cfg["variance_type"] is None
    r = d.DPMSolverMultistepScheduler.from_pretrained(str(tmp_path))
    assert r.config.to_dict() == s.config.to_dict() and torch.equal(r.lambda_t, s.lambda_t)
    assert d.DPMSolverMultistepScheduler.from_config(s.config).config.to_dict() == s.config.to_dict()
    assert d.DPMSolverMultistepScheduler().config.to_dict() == dict(
        num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None, solver_order=2,
        prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
        algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, use_karras_sigmas=False,
        lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0)


def test_from_config_of_the_other_schedulers(lib_built):
    """The swap idiom: keys the class lacks (clip_sample, set_alpha_to_one, ...) are dropped, shared ones carried over."""
    a = d.DPMSolverMultistepScheduler.from_config(d.DDPMScheduler(beta_end=0.03).config)
    assert a.config.beta_end == 0.03 and a.config.timestep_spacing == "leading" and a.config.solver_order == 2
    assert not hasattr(a.config, "clip_sample") and a.config.variance_type == "fixed_small"
    b = d.DPMSolverMultistepScheduler.from_config(d.DDIMScheduler(steps_offset=1).config)
    assert b.config.steps_offset == 1 and b.config.variance_type is None and not hasattr(b.config, "set_alpha_to_one")
    a.set_timesteps(20)
    assert a.timesteps.tolist() == list(range(940, 0, -47))
    # and back: the pipelines' own classes take the solver's config
    assert d.DDIMScheduler.from_config(a.config).config.beta_end == 0.03
    # add_noise is inherited, so the class can stand in for DDPMScheduler in the training loop (GPU tensors only)
    assert d.DPMSolverMultistepScheduler.add_noise is d.DDPMScheduler.add_noise


@pytest.mark.parametrize("kw,word", [
    (dict(beta_schedule="scaled_linear"), "beta_schedule"), (dict(trained_betas=[0.1, 0.2]), "trained_betas"),
    (dict(solver_order=4), "solver_order"), (dict(solver_order=0), "solver_order"), (dict(solver_order=True), "solver_order"),
    (dict(prediction_type="v_prediction"), "prediction_type"), (dict(prediction_type="sample"), "prediction_type"),
    (dict(thresholding=True), "thresholding"), (dict(dynamic_thresholding_ratio=0.9), "dynamic_thresholding_ratio"),
    (dict(sample_max_value=2.0), "sample_max_value"), (dict(algorithm_type="dpmsolver"), "algorithm_type"),
    (dict(algorithm_type="sde-dpmsolver"), "algorithm_type"), (dict(algorithm_type="deis"), "algorithm_type"),
    (dict(solver_type="bh1"), "solver_type"), (dict(lower_order_final=1), "lower_order_final"),
    (dict(use_karras_sigmas=True), "use_karras_sigmas"), (dict(lambda_min_clipped=-5.1), "lambda_min_clipped"),
    (dict(variance_type="learned"), "variance_type"), (dict(variance_type="learned_range"), "variance_type"),
    (dict(timestep_spacing="karras"), "timestep_spacing"), (dict(steps_offset=0.5), "steps_offset"),
    (dict(algorithm_type="sde-dpmsolver++", solver_order=3), "solver_order=3"),
])
def test_unsupported_values_raise(lib_built, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        d.DPMSolverMultistepScheduler(**kw)


def test_other_refusals(lib_built):
    with pytest.raises(TypeError, match="unexpected"):
        d.DPMSolverMultistepScheduler(clip_sample=True)
    s = d.DPMSolverMultistepScheduler()
    x = torch.zeros(1, 3, 8, 8)
    s.set_timesteps(10)
    with pytest.raises(RuntimeError, match="HIP engine"):
        s.step(x, 999, x)
    with pytest.raises(RuntimeError, match="HIP engine"):
        s.add_noise(x, x, torch.tensor([1]))
    with pytest.raises(ValueError, match="seed"):
        s.use_device_noise(None)
    with pytest.raises(ValueError):
        d.DPMSolverMultistepScheduler(timestep_spacing="leading", steps_offset=100).set_timesteps(20)   # 940 + 100 > 999


def test_pipeline_folders_keep_the_scheduler(lib_built, tmp_path):
    """model_index.json names the solver: DDPMPipeline / DDIMPipeline read it back as it is, RePaintPipeline converts."""
    unet = d.UNet2DModel(**CFG1)
    sch = d.DPMSolverMultistepScheduler(solver_order=3, beta_end=0.03, timestep_spacing="trailing")
    for cls in (d.DDPMPipeline, d.DDIMPipeline):
        path = str(tmp_path / cls.__name__)
        cls(unet, sch).save_pretrained(path)
        index = json.load(open(os.path.join(path, "model_index.json")))
        assert index["scheduler"] == ["diffusers", "DPMSolverMultistepScheduler"] and index["_class_name"] == cls._class_name
        p = cls.from_pretrained(path)
        assert type(p.scheduler) is d.DPMSolverMultistepScheduler and p.scheduler.config.to_dict() == sch.config.to_dict()
        assert type(p) is cls
    q = d.RePaintPipeline.from_pretrained(str(tmp_path / "DDIMPipeline"))
    assert type(q.scheduler) is d.RePaintScheduler and q.scheduler.config.beta_end == 0.03
    # the pipelines' own folders load as before
    d.DDPMPipeline(unet, d.DDPMScheduler()).save_pretrained(str(tmp_path / "plain"))
    assert type(d.DDPMPipeline.from_pretrained(str(tmp_path / "plain")).scheduler) is d.DDPMScheduler
    assert type(d.DDIMPipeline.from_pretrained(str(tmp_path / "plain")).scheduler) is d.DDIMScheduler


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def _args(**kw):
    # (addresses that are never dereferenced: every call below is refused before any HIP call)
    base = dict(sample=0x10000, eps=0x20000, m1=0x30000, m2=0x40000, noise=None, prev=0x50000, m0_out=0x60000, noise_out=None,
                numel=64, order=3, add_noise=0, sigma_s=0.5, alpha_s=0.5, inv_r0=1.0, inv_r1=1.0, q=0.5, p=0.5, kx=0.9, c0=0.1,
                c1=0.05, c2=0.01, cn=0.0, seed=0, offset=0)
    base.update(kw)
    return _lib.DpmSolverStepArgs(**base)


def test_abi_refuses_bad_arguments_before_any_hip_call(lib_built):
    lib = _lib.load()
    assert lib.dsg_dpmsolver_step(None, None) == -1 and b"NULL" in lib.dsg_last_error()
    cases = [(dict(sample=None), b"NULL"), (dict(eps=None), b"NULL"), (dict(prev=None), b"NULL"), (dict(m0_out=None), b"NULL"),
             (dict(numel=0), b"positive"), (dict(numel=-4), b"positive"), (dict(order=0), b"order"), (dict(order=4), b"order"),
             (dict(order=2, m1=None), b"m1"), (dict(order=3, m1=None), b"m1"), (dict(order=3, m2=None), b"m2"),
             (dict(prev=0x10000), b"overlap"), (dict(prev=0x20000 + 252), b"overlap"), (dict(prev=0x20000 - 252), b"overlap"),
             (dict(m0_out=0x30000), b"overlap"), (dict(m0_out=0x40000 + 4), b"overlap"), (dict(m0_out=0x50000 + 128), b"overlap"),
             (dict(add_noise=1, noise=0x70000, prev=0x70000 + 16), b"overlap"),
             (dict(add_noise=1, noise_out=0x10000 + 64), b"overlap"), (dict(add_noise=1, noise_out=0x60000), b"overlap")]
    for kw, word in cases:
        a = _args(**kw)
        assert lib.dsg_dpmsolver_step(ctypes.byref(a), None) == -1, kw
        assert word in lib.dsg_last_error(), (kw, lib.dsg_last_error())
    assert ctypes.sizeof(_lib.DpmSolverStepArgs) == 144       # 8 pointers, int64, 2 int32, 11 floats (+4 pad), 2 uint64
