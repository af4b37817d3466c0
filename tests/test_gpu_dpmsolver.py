"""DPM-Solver++ on the GPU: ``dsg_dpmsolver_step`` against the NumPy fp32 restatement (tests/dpmsolver_oracle.py) value for
value, the in-kernel Philox source against ``dsg_philox_normal``, whole scheduler loops on a model with a known answer, the
two pipelines with the scheduler swapped in, teacher-forced parity with a CPU run, and guard margins round every output.

Comparisons of kernel outputs use ``np.array_equal`` on the fp32 VALUES; no tolerance.  SURVEY 8c's teacher-forced bound
applies only where the U-Net is in the path."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import _lib, ops  # noqa: E402
from tests import dpmsolver_oracle as do  # noqa: E402
from tests.common import CFG1, CFG2, max_abs, rel_l2, synth_weights, trajectory_weights  # noqa: E402

DEV = "cuda"
F = np.float32
SENTINEL = 123456.0
TABS = do.tables(F)
# margin in floats: 1024 keeps the interior 16-byte aligned (dwordx4 path), 1027 does not (dword path)
MARGINS = (1024, 1027)
# numel a multiple of 1024; hw = 279 odd with numel % 4 == 0 and more than one block; numel % 4 != 0 (a scalar tail)
SHAPES = [(2, 4, 16, 16), (3, 4, 9, 31), (1, 3, 7, 5)]
TS20 = [int(t) for t in do.timesteps(20, "linspace")]
# index into the 20-step table: an early step (the first with two history entries), a middle one, the LAST (t -> 0)
POSITIONS = {"early": 2, "middle": 10, "last": 19}
# (algorithm, order, solver type): every form the kernel's scalars take
FORMS = [("dpmsolver++", 1, "midpoint"), ("dpmsolver++", 2, "midpoint"), ("dpmsolver++", 2, "heun"), ("dpmsolver++", 3, "midpoint"),
         ("dpmsolver++", 3, "heun"), ("sde-dpmsolver++", 1, "midpoint"), ("sde-dpmsolver++", 2, "midpoint"),
         ("sde-dpmsolver++", 2, "heun")]


def _guarded(numel, margin):
    """(whole buffer, interior view of `numel` floats) with `margin` floats of SENTINEL on each side (>= 4 KiB)."""
    assert margin * 4 >= 4096
    whole = torch.full((numel + 2 * margin,), SENTINEL, dtype=torch.float32, device=DEV)
    return whole, whole[margin:margin + numel]


def _margins_intact(whole, numel, margin):
    w = whole.cpu().numpy()
    return bool((w[:margin] == SENTINEL).all() and (w[margin + numel:] == SENTINEL).all())


def _scalars(form, pos):
    algorithm, order, solver_type = form
    i = POSITIONS[pos]
    t = TS20[i + 1] if i + 1 < len(TS20) else 0
    return do.step_scalars(TS20[i], t, TS20[i - 1], TS20[i - 2], order, algorithm, solver_type, TABS, F)


def _inputs(shape, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(shape).astype(F) for _ in range(5))      # x, e, m1, m2, z


def _call(x, e, m1, m2, z, s, order, add_noise, margin, seed=0, offset=0, want_noise_out=False):
    """One dsg_dpmsolver_step with every output an interior view of a sentinel-filled buffer.  z=None with add_noise: Philox.
    Returns (prev, m0_out, noise_out | None, margins intact and inputs unchanged)."""
    shape, numel = x.shape, x.size
    host = dict(x=x, e=e, m1=m1 if order >= 2 else None, m2=m2 if order >= 3 else None, z=z if add_noise else None)
    # with the misaligned margin the sample and m1 sit 3 floats off a 16-byte boundary too (a mix of aligned and misaligned inputs)
    off = {k: (margin % 4 if k in ("x", "m1") else 0) for k in host}
    t = {k: torch.zeros(numel + 4, dtype=torch.float32, device=DEV)[off[k]:off[k] + numel].view(v.shape).copy_(
            torch.from_numpy(np.ascontiguousarray(v))) if v is not None else None for k, v in host.items()}
    p = {k: (v.data_ptr() if v is not None else None) for k, v in t.items()}
    pw, prev = _guarded(numel, margin)
    mw, m0o = _guarded(numel, margin)
    nw, nout = _guarded(numel, margin) if want_noise_out else (None, None)
    a = _lib.DpmSolverStepArgs(
        sample=p["x"], eps=p["e"], m1=p["m1"], m2=p["m2"], noise=p["z"], prev=prev.data_ptr(), m0_out=m0o.data_ptr(),
        noise_out=nout.data_ptr() if nout is not None else None, numel=numel, order=order, add_noise=int(add_noise),
        seed=seed, offset=offset, **{k: float(v) for k, v in s.items()})
    _lib.check(_lib.load().dsg_dpmsolver_step(ctypes.byref(a), _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    ok = _margins_intact(pw, numel, margin) and _margins_intact(mw, numel, margin)
    ok = ok and (nw is None or _margins_intact(nw, numel, margin))
    ok = ok and all(np.array_equal(t[k].cpu().numpy(), host[k]) for k in host if host[k] is not None)
    return (prev.cpu().numpy().reshape(shape), m0o.cpu().numpy().reshape(shape),
            nout.cpu().numpy().reshape(shape) if nout is not None else None, ok)


@pytest.mark.parametrize("shape", SHAPES)
def test_step_equals_the_numpy_restatement_every_element(shape):
    """Orders 1-3, both solver types, both algorithms, scalars of an early, a middle and the last step, the noise term on and
    off (whatever the algorithm: the kernel takes a flag and a coefficient), aligned and misaligned outputs: prev and m0_out
    equal the restatement on every element; margins intact; inputs unchanged."""
    n = 0
    for fi, form in enumerate(FORMS):
        order = form[1]
        for pi, pos in enumerate(POSITIONS):
            s = dict(_scalars(form, pos))
            assert all(np.isfinite(v) for v in s.values())
            for add_noise in (False, True):
                if add_noise and s["cn"] == 0:
                    s["cn"] = F(0.37)                               # (an ODE step's scalars with a noise term on top)
                for margin in MARGINS:
                    x, e, m1, m2, z = _inputs(shape, 1000 * fi + 10 * pi + n % 7)
                    prev, m0, _, ok = _call(x, e, m1, m2, z, s, order, add_noise, margin)
                    want_prev, want_m0 = do.step(x, e, m1, m2, z, s, order, add_noise, F)
                    what = (form, pos, add_noise, margin)
                    assert ok, what
                    assert np.isfinite(want_prev).all() and np.array_equal(m0, want_m0), what
                    assert np.array_equal(prev, want_prev), (what, int((prev != want_prev).sum()),
                                                             float(np.abs(prev - want_prev).max()))
                    n += 1
    assert n == len(FORMS) * 3 * 2 * 2
    # the terms are really there: leaving one out changes the answer
    s = _scalars(("dpmsolver++", 3, "midpoint"), "middle")
    x, e, m1, m2, z = _inputs(shape, 5)
    full = do.step(x, e, m1, m2, z, s, 3, False, F)[0]
    assert not np.array_equal(full, do.step(x, e, m1, m2, z, s, 2, False, F)[0])
    assert not np.array_equal(full, do.step(x, e, m1, m2, z, dict(s, cn=F(0.1)), 3, True, F)[0])


@pytest.mark.parametrize("seed,offset", [(0, 0), (14555, 3), (2 ** 63 + 12345, (5 << 40) | 77)])
def test_philox_source_is_the_named_tensor(seed, offset):
    """noise_out is bitwise dsg_philox_normal(numel, seed, offset); prev equals the supplied-noise call fed that tensor and
    the restatement; the next offset names another tensor and gives another prev."""
    form = ("sde-dpmsolver++", 2, "midpoint")
    s = _scalars(form, "middle")
    for i, shape in enumerate(SHAPES):
        for margin in MARGINS:
            numel = int(np.prod(shape))
            named = ops.philox_normal((numel,), seed, offset).cpu().numpy().reshape(shape)
            x, e, m1, m2, _ = _inputs(shape, 60 + i)
            got, m0, nout, ok = _call(x, e, m1, m2, None, s, 2, True, margin, seed, offset, want_noise_out=True)
            assert ok and np.array_equal(nout.view(np.uint32), named.view(np.uint32)), (shape, margin)
            fed, m0_fed, _, _ = _call(x, e, m1, m2, named, s, 2, True, margin)
            want, want_m0 = do.step(x, e, m1, m2, named, s, 2, True, F)
            assert np.array_equal(got, fed) and np.array_equal(got, want), (shape, margin)
            assert np.array_equal(m0, want_m0) and np.array_equal(m0_fed, want_m0)
            other, _, nout2, _ = _call(x, e, m1, m2, None, s, 2, True, margin, seed, offset + 1, want_noise_out=True)
            assert not np.array_equal(nout2, nout) and not np.array_equal(other, got)


# ---- whole scheduler loops on the model with a known answer ------------------------------------------------------------------
LOOPS = [(so, "dpmsolver++", st) for so in (1, 2, 3) for st in do.SOLVER_TYPES] + \
        [(so, "sde-dpmsolver++", st) for so in (1, 2) for st in do.SOLVER_TYPES]


@pytest.mark.parametrize("steps", [20, 10])
@pytest.mark.parametrize("solver_order,algorithm,solver_type", LOOPS)
def test_a_whole_scheduler_loop_equals_the_restatement(solver_order, algorithm, solver_type, steps):
    """eps of the analytic model computed on the host in NumPy fp32 from the engine's own x and uploaded each step; the SDE
    variant's noise handed in.  The end state (and every step on the way) equals the fp32 restatement running the same loop:
    the history ring, the order bookkeeping, lower_order_final (10 steps) and the last step (t -> 0)."""
    shape = (2, 3, 7, 5)
    rng = np.random.default_rng(steps + solver_order)
    x_T = rng.standard_normal(shape).astype(F)
    zs = [rng.standard_normal(shape).astype(F) for _ in range(steps)]
    rec = []
    want = do.run(lambda x, t: do.analytic_eps(x, t, TABS, F), x_T, steps, solver_order, algorithm, solver_type,
                  noise_fn=lambda i: zs[i], dtype=F, records=rec)
    assert [r["order"] for r in rec] == do.orders(solver_order, steps) and np.isfinite(want).all()
    sch = d.DPMSolverMultistepScheduler(solver_order=solver_order, algorithm_type=algorithm, solver_type=solver_type)
    sch.set_timesteps(steps)
    x = torch.from_numpy(x_T).to(DEV)
    for i, t in enumerate(sch.timesteps.tolist()):
        eps = do.analytic_eps(x.cpu().numpy(), t, TABS, F)
        z = torch.from_numpy(zs[i]).to(DEV) if sch.needs_step_noise else None
        x = sch.step(torch.from_numpy(eps).to(DEV), t, x, variance_noise=z).prev_sample
        assert np.array_equal(x.cpu().numpy(), rec[i]["x_out"]), (i, t, rec[i]["order"])
    assert np.array_equal(x.cpu().numpy(), want)


def test_device_noise_names_one_philox_tensor_per_step():
    """use_device_noise(seed, offset): step k's noise is dsg_philox_normal(seed, offset + k); nothing is drawn on the host."""
    shape, steps, seed = (2, 3, 7, 5), 6, 991
    x_T = np.random.default_rng(3).standard_normal(shape).astype(F)
    want = do.run(lambda x, t: do.analytic_eps(x, t, TABS, F), x_T, steps, 2, "sde-dpmsolver++", "midpoint",
                  noise_fn=lambda i: ops.philox_normal(shape, seed, 4 + i).cpu().numpy(), dtype=F)
    sch = d.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    sch.set_timesteps(steps)
    sch.use_device_noise(seed, offset=4)
    g = torch.Generator().manual_seed(0)
    before = g.get_state()
    x = torch.from_numpy(x_T).to(DEV)
    for t in sch.timesteps.tolist():
        x = sch.step(torch.from_numpy(do.analytic_eps(x.cpu().numpy(), t, TABS, F)).to(DEV), t, x, generator=g).prev_sample
    assert np.array_equal(x.cpu().numpy(), want) and sch.noise_offset == 4 + steps and torch.equal(g.get_state(), before)


# ---- the pipelines on the tiny network ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    return synth_weights(d.UNet2DModel(**CFG1)).to(DEV).eval().requires_grad_(False)


def _swapped(pipe_cls, net, **overrides):
    pipe = pipe_cls(net, pipe_cls._scheduler_cls())
    pipe.scheduler = d.DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, **overrides)     # the swap idiom
    return pipe


def _after_draws(seed, shape, count):
    g = torch.Generator().manual_seed(seed)
    for _ in range(count):
        torch.randn(shape, generator=g)
    return g.get_state()


@pytest.mark.parametrize("pipe_cls", [d.DDPMPipeline, d.DDIMPipeline], ids=["ddpm_pipeline", "ddim_pipeline"])
@pytest.mark.parametrize("algorithm", do.ALGORITHMS)
def test_pipelines_with_the_swapped_scheduler(tiny, tmp_path, pipe_cls, algorithm):
    """10 and 20 steps: the same seed gives the same bits, another seed other bits; the folder round trip gives the same image;
    the ODE run draws x_T and nothing else from the generator, the SDE run 1 + steps tensors."""
    batch, shape = 2, (2, 3, 64, 64)
    pipe = _swapped(pipe_cls, tiny, algorithm_type=algorithm)
    assert type(pipe.scheduler) is d.DPMSolverMultistepScheduler and pipe.scheduler.config.timestep_spacing == "leading"

    def run(p, seed, steps):
        g = torch.Generator().manual_seed(seed)
        out = p(batch_size=batch, generator=g, num_inference_steps=steps, output_type="np.array").images
        return out, g.get_state()

    for steps in (10, 20):
        out, state = run(pipe, 21, steps)
        assert out.shape == (batch, 64, 64, 3) and np.isfinite(out).all() and not np.array_equal(out[0], out[1])
        draws = 1 + (steps if algorithm == "sde-dpmsolver++" else 0)
        assert torch.equal(state, _after_draws(21, shape, draws)), (steps, draws)
        again, _ = run(pipe, 21, steps)
        assert np.array_equal(out, again)
        assert not np.array_equal(out, run(pipe, 22, steps)[0])
    pipe.save_pretrained(str(tmp_path / "p"))
    back = pipe_cls.from_pretrained(str(tmp_path / "p")).to(DEV)
    assert type(back.scheduler) is d.DPMSolverMultistepScheduler
    assert back.scheduler.config.to_dict() == pipe.scheduler.config.to_dict()
    back.unet.eval().requires_grad_(False)
    assert np.array_equal(run(back, 21, 20)[0], out)
    # the pipelines' own schedulers are served as before by the same objects
    own = pipe_cls(tiny, pipe_cls._scheduler_cls())
    a = own(batch_size=batch, generator=torch.Generator().manual_seed(21), num_inference_steps=10, output_type="np.array").images
    assert a.shape == out.shape and not np.array_equal(a, out)


def test_device_noise_and_sharding(tiny):
    """The SDE variant with the scheduler's device noise: the generator supplies x_T only; with shard= it is refused.  The ODE
    variant shards like DDIM: a shard's rows equal the full call's."""
    shape = (2, 3, 64, 64)
    for pipe_cls in (d.DDPMPipeline, d.DDIMPipeline):
        pipe = _swapped(pipe_cls, tiny, algorithm_type="sde-dpmsolver++")
        pipe.scheduler.use_device_noise(7)
        g = torch.Generator().manual_seed(4)
        a = pipe(batch_size=2, generator=g, num_inference_steps=10, output_type="np.array").images
        assert torch.equal(g.get_state(), _after_draws(4, shape, 1)) and np.isfinite(a).all()
        assert pipe.scheduler.noise_offset == 10
        with pytest.raises(NotImplementedError, match="shard"):
            pipe(batch_size=2, generator=g, num_inference_steps=10, output_type="np.array", shard=(0, 2))
        ode = _swapped(pipe_cls, tiny)
        full = ode(batch_size=2, generator=torch.Generator().manual_seed(4), num_inference_steps=10, output_type="np.array").images
        for rank in (0, 1):
            part = ode(batch_size=2, generator=torch.Generator().manual_seed(4), num_inference_steps=10, output_type="np.array",
                       shard=(rank, 2)).images
            assert part.shape == (1, 64, 64, 3) and np.array_equal(part, full[rank:rank + 1])    # batch rows are independent


def test_an_early_exit_leaves_the_generator_where_the_serial_loop_would(tiny):
    """DDPMPipeline + the SDE variant + a CPU generator: the noise comes through the pinned ring, drawn one step ahead by a
    worker.  A call that dies in step 4 has drawn x_T and four steps' noise, no more; the ODE variant x_T alone."""
    shape = (2, 3, 64, 64)
    for algorithm, draws in (("sde-dpmsolver++", 5), ("dpmsolver++", 1)):
        pipe = _swapped(d.DDPMPipeline, tiny, algorithm_type=algorithm)
        sch, calls = pipe.scheduler, {"n": 0}
        real_step = sch.step

        def failing_step(*a, **k):
            calls["n"] += 1
            if calls["n"] == 4:
                raise KeyError("step 4 failed")
            return real_step(*a, **k)
        sch.step = failing_step
        gen = torch.Generator().manual_seed(4242)
        with pytest.raises(KeyError):
            pipe(num_inference_steps=12, batch_size=2, generator=gen, output_type="np.array")
        sch.step = real_step
        assert torch.equal(gen.get_state(), _after_draws(4242, shape, draws)), algorithm
        # and the pipeline is usable afterwards (set_timesteps starts a fresh history)
        out = pipe(num_inference_steps=12, batch_size=2, generator=torch.Generator().manual_seed(1), output_type="np.array").images
        assert np.isfinite(out).all()


@pytest.mark.parametrize("algorithm", do.ALGORITHMS)
def test_teacher_forced_parity_with_a_cpu_run(algorithm):
    """The oracle U-Net (contractive synthetic weights) + tests/dpmsolver_oracle.py run 8 steps at order 2 from a seeded CPU
    generator; at every step the engine gets the oracle's input.  SURVEY 8c's teacher-forced bound on eps and on the step's
    output (the engine's history is its own: made from its own eps).  The SDE variant's scheduler draws from its own equally
    seeded generator: the bound can only hold if the order and shapes of its draws are the oracle's."""
    from oracle.unet_oracle import OracleUNet2DModel
    net = trajectory_weights(d.UNet2DModel(**CFG1), "tiny_c").to(DEV).eval().requires_grad_(False)
    ora = trajectory_weights(OracleUNet2DModel(**CFG1), "tiny_c").eval()
    shape, steps = (2, 3, 64, 64), 8

    def eps_fn(x, t):
        with torch.no_grad():
            return ora(torch.from_numpy(x), t).sample.numpy()

    g_o = torch.Generator().manual_seed(14555)
    x_T = torch.randn(shape, generator=g_o).numpy()
    rec = []
    do.run(eps_fn, x_T, steps, 2, algorithm, "midpoint", noise_fn=lambda i: torch.randn(shape, generator=g_o).numpy(),
           dtype=F, records=rec)
    assert [r["order"] for r in rec] == [1, 2, 2, 2, 2, 2, 2, 1]

    def within(got, want, what):
        got, want = torch.from_numpy(got), torch.from_numpy(want)
        ma, rl = max_abs(got, want), rel_l2(got, want)
        print(f"{what}: max|d| {ma:.3e} (bound {2e-4 * max(1.0, float(want.abs().max())):.3e}), rel-L2 {rl:.3e}")
        assert ma <= 2e-4 * max(1.0, float(want.abs().max())) and rl <= 1e-4, (what, ma, rl)

    sch = d.DPMSolverMultistepScheduler(algorithm_type=algorithm)
    sch.set_timesteps(steps)
    assert sch.timesteps.tolist() == [r["t"] for r in rec]
    g = torch.Generator().manual_seed(14555)
    assert np.array_equal(torch.randn(shape, generator=g).numpy(), x_T)
    for i, r in enumerate(rec):
        x_in = torch.from_numpy(r["x_in"]).to(DEV)
        eps = net(x_in, r["t"]).sample
        within(eps.cpu().numpy(), r["eps"], f"step {i} t={r['t']} eps")
        out = sch.step(eps, r["t"], x_in, generator=g).prev_sample
        within(out.cpu().numpy(), r["x_out"], f"step {i} t={r['t']} order {r['order']} step")
    assert torch.equal(g.get_state(), g_o.get_state())


def test_full_size_call():
    """configs[1]'s network (256 x 256 x 4) at batch 2, 3 steps, through both pipelines."""
    net = synth_weights(d.UNet2DModel(**CFG2)).to(DEV).eval().requires_grad_(False)
    for pipe_cls, algorithm in ((d.DDIMPipeline, "dpmsolver++"), (d.DDPMPipeline, "sde-dpmsolver++")):
        pipe = _swapped(pipe_cls, net, algorithm_type=algorithm)
        out = pipe(batch_size=2, generator=torch.Generator().manual_seed(2), num_inference_steps=3, output_type="np.array").images
        assert out.shape == (2, 256, 256, 4) and np.isfinite(out).all() and not np.array_equal(out[0], out[1])
    pil = pipe(batch_size=2, num_inference_steps=3).images
    assert len(pil) == 2 and pil[0].mode == "RGBA" and pil[0].size == (256, 256)
