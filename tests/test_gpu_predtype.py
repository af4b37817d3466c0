"""Sample- and v-prediction on the GPU: ``dsg_ddpm_step_pt`` / ``dsg_ddim_step_pt``, ``dsg_add_noise_target`` (+ Philox) and
``dsg_mse_loss_weighted`` against the torch-CPU fp32 restatement (tests/predtype_oracle.py) bit for bit, a closed-form check that
does not go through the restatement, scheduler loops, and the pipelines / ``train_step`` / ``fit`` on a v-prediction scheduler.

Comparisons are on the fp32 BITS unless a bound is stated.  Every output is an interior view of a poison-filled buffer; the
words around it and the inputs are checked intact.  Layouts: [3, 3, 5, 7] (per = 105: a tail, 4-element groups that straddle
samples), [2, 4, 16, 16] (whole aligned groups) and the latter one float past a 16-byte boundary (the dword path)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import _lib, ops  # noqa: E402
from tests import predtype_oracle as po  # noqa: E402
from tests.common import CFG1, synth_weights  # noqa: E402

DEV = "cuda"
POISON = 123456.0
MARGIN = 1024                       # floats; the interior starts `off` floats past a 16-byte boundary
LAYOUTS = [((3, 3, 5, 7), 0), ((2, 4, 16, 16), 0), ((2, 4, 16, 16), 1)]
LAYOUT_IDS = ["3x3x5x7", "2x4x16x16", "2x4x16x16_off1"]
PREDS = ("sample", "v_prediction")
CODE = _lib.PRED_CODES

ZERO = d.DDIMScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing")      # the host scalars: no prediction type in them
ZERO.set_timesteps(50)
_TS = ZERO.timesteps.tolist()
DDIM_TS = (_TS[0], _TS[25], _TS[-1])
assert DDIM_TS == (999, 499, 19) and float(ZERO.alphas_cumprod[999]) == 0.0
DDPM = d.DDPMScheduler()
DDPM.set_timesteps(50)
DDPM_TS = (500, 0)                  # (t = 0 has no noise term)


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _guarded(shape, off):
    numel = int(np.prod(shape))
    whole = torch.full((numel + 2 * MARGIN + 4,), POISON, dtype=torch.float32, device=DEV)
    return whole, whole[MARGIN + off:MARGIN + off + numel].view(shape)


def _intact(whole, view, off):
    w = whole.cpu()
    return bool((w[:MARGIN + off] == POISON).all() and (w[MARGIN + off + view.numel():] == POISON).all())


def _upload(v, off):
    buf = torch.zeros(v.numel() + 4, dtype=torch.float32, device=DEV)
    return buf[off:off + v.numel()].view(v.shape).copy_(v)


def _draws(shape, seed):
    """x0 uniform in [-1, 1] (a raster), model output and two noise tensors N(0, 1), on the CPU"""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(shape, generator=g) * 2 - 1
    return x0, torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(shape, generator=g)


class _Call:
    """The C entries on one layout: inputs uploaded once, every output guarded."""

    def __init__(self, shape, off, **host):
        self.shape, self.off, self.host = shape, off, host
        self.dev = {k: _upload(v, off) for k, v in host.items()}
        self.numel = int(np.prod(shape))
        self.lib, self.st = _lib.load(), _lib.stream_ptr(torch.device(DEV))
        self.ok = True

    def out(self, shape=None):
        return _guarded(shape or self.shape, self.off)

    def done(self, *pairs):
        torch.cuda.synchronize()
        for whole, view in pairs:
            self.ok = self.ok and _intact(whole, view, self.off)
        return [view.cpu() for _, view in pairs]

    def ddim(self, sc, code, clip, pt=True):
        pw, prev = self.out()
        a = (sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], clip, sc["sqrt_alpha_prev"], sc["dir_coef"], self.st)
        x, m = self.dev["x"].data_ptr(), self.dev["m"].data_ptr()
        if pt:
            _lib.check(self.lib.dsg_ddim_step_pt(x, m, prev.data_ptr(), self.numel, code, *a))
        else:
            _lib.check(self.lib.dsg_ddim_step(x, m, prev.data_ptr(), self.numel, *a))
        return self.done((pw, prev))[0]

    def ddpm(self, sc, code, clip, noise, pt=True):
        pw, prev = self.out()
        a = (sc["sqrt_beta_prod_t"], sc["sqrt_alpha_prod_t"], clip, sc["coef_x0"], sc["coef_xt"], sc["sigma"], self.st)
        x, m, z = self.dev["x"].data_ptr(), self.dev["m"].data_ptr(), self.dev["z"].data_ptr() if noise else None
        if pt:
            _lib.check(self.lib.dsg_ddpm_step_pt(x, m, z, prev.data_ptr(), self.numel, code, *a))
        else:
            _lib.check(self.lib.dsg_ddpm_step(x, m, z, prev.data_ptr(), self.numel, *a))
        return self.done((pw, prev))[0]

    def inputs_unchanged(self):
        return all(_bits_equal(self.dev[k].cpu(), self.host[k]) for k in self.dev)


# ---- the steps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_steps_equal_the_restatement(layout):
    """DDPM (with noise, and t = 0 without) and DDIM (the first, a middle and the last step of a 50-step trailing run on the
    zero-terminal-SNR table: abar = 0 at t = 999), sample and v, with and without the clip."""
    shape, off = layout
    x0, m, z, e = _draws(shape, 11 + off)
    x = x0 * 0.6 + e * 0.9                       # (values on both sides of the clip)
    run = _Call(shape, off, x=x, m=m, z=z)
    for pred in PREDS:
        for clip in (0.0, 1.0):
            for t in DDIM_TS:
                sc = ZERO.step_scalars(t)
                want = po.ddim_step(x, m, sc, pred, clip)
                got = run.ddim(sc, CODE[pred], clip)
                assert torch.isfinite(want).all() and _bits_equal(got, want), ("ddim", pred, clip, t, int((got != want).sum()))
            for t in DDPM_TS:
                sc = DDPM.step_scalars(t)
                want = po.ddpm_step(x, m, z if t > 0 else None, sc, pred, clip)
                got = run.ddpm(sc, CODE[pred], clip, noise=t > 0)
                assert torch.isfinite(want).all() and _bits_equal(got, want), ("ddpm", pred, clip, t, int((got != want).sum()))
    # the clip acted, and only on the data prediction
    sc = ZERO.step_scalars(499)
    assert not _bits_equal(po.ddim_step(x, m, sc, "v_prediction", 1.0), po.ddim_step(x, m, sc, "v_prediction", 0.0))
    assert run.ok and run.inputs_unchanged()


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_the_epsilon_form_of_the_new_entries_is_the_old_kernels(layout):
    shape, off = layout
    x0, m, z, e = _draws(shape, 21 + off)
    run = _Call(shape, off, x=x0 * 0.6 + e * 0.9, m=m, z=z)
    for clip in (0.0, 1.0):
        for t in DDIM_TS[1:] + (500, 0):         # (not t = 999 of the zero-SNR table: epsilon prediction is undefined at abar = 0)
            sc = ZERO.step_scalars(t)
            assert _bits_equal(run.ddim(sc, CODE["epsilon"], clip), run.ddim(sc, None, clip, pt=False)), ("ddim", clip, t)
        for t in DDPM_TS:
            sc = DDPM.step_scalars(t)
            assert _bits_equal(run.ddpm(sc, CODE["epsilon"], clip, t > 0), run.ddpm(sc, None, clip, t > 0, pt=False)), ("ddpm", clip, t)
    # and it is the restatement's epsilon form
    sc = ZERO.step_scalars(499)
    assert _bits_equal(run.ddim(sc, CODE["epsilon"], 1.0), po.ddim_step(run.host["x"], m, sc, "epsilon", 1.0))
    assert run.ok and run.inputs_unchanged()


# ---- x_t and the velocity target ------------------------------------------------------------------------------------------------
def _coefs(sch, t):
    sa, sb = po.sqrt_tables(sch.alphas_cumprod)
    return sa[t], sb[t]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_noisy_and_target_in_one_pass(layout):
    shape, off = layout
    n = shape[0]
    x0, _, z, _ = _draws(shape, 31 + off)
    t = torch.tensor([999, 499, 0][:n])
    sch = d.DDIMScheduler(rescale_betas_zero_snr=True, prediction_type="v_prediction")
    sa, sb = _coefs(sch, t)
    want_noisy, want_v = po.add_noise(x0, z, sa, sb), po.velocity(x0, z, sa, sb)
    run = _Call(shape, off, x0=x0, z=z)
    sa_d, sb_d = sa.to(DEV).contiguous(), sb.to(DEV).contiguous()
    per = run.numel // n

    def entry(noisy, target):
        (nw, nv), (tw, tv) = run.out(), run.out()
        _lib.check(run.lib.dsg_add_noise_target(run.dev["x0"].data_ptr(), run.dev["z"].data_ptr(), sa_d.data_ptr(), sb_d.data_ptr(),
                                                nv.data_ptr() if noisy else None, tv.data_ptr() if target else None, n, per, run.st))
        got_n, got_t = run.done((nw, nv), (tw, tv))
        return got_n, got_t

    got_n, got_t = entry(True, True)
    assert _bits_equal(got_n, want_noisy) and _bits_equal(got_t, want_v)
    only_t = entry(False, True)
    assert _bits_equal(only_t[1], want_v) and bool((only_t[0] == POISON).all())
    only_n = entry(True, False)
    assert _bits_equal(only_n[0], want_noisy) and bool((only_n[1] == POISON).all())
    # the scheduler's methods: add_noise's bits, get_velocity, both at once
    x0_d, z_d, t_d = x0.to(DEV), z.to(DEV), t.to(DEV)
    assert _bits_equal(sch.add_noise(x0_d, z_d, t_d).cpu(), want_noisy)
    assert _bits_equal(sch.get_velocity(x0_d, z_d, t_d).cpu(), want_v)
    both = sch.add_noise_velocity(x0_d, z_d, t_d)
    assert _bits_equal(both[0].cpu(), want_noisy) and _bits_equal(both[1].cpu(), want_v)
    # one timestep for the whole tensor (add_noise's other rule)
    one = torch.tensor([499])
    sa1, sb1 = _coefs(sch, one)
    assert _bits_equal(sch.get_velocity(x0_d, z_d, one).cpu(), po.velocity(x0[None], z[None], sa1, sb1)[0])
    with pytest.raises(ValueError, match="timesteps"):
        sch.get_velocity(x0_d, z_d, torch.tensor([1] * (n + 1)))
    # Philox: the noise of add_noise_device, made in the kernel
    seed, offset = 0x1234567890ABCDEF, 7
    ref_noisy, ref_noise = sch.add_noise_device(x0_d, t_d, seed, offset)
    (nw, nv), (tw, tv) = run.out(), run.out()
    _lib.check(run.lib.dsg_add_noise_target_philox(run.dev["x0"].data_ptr(), sa_d.data_ptr(), sb_d.data_ptr(), nv.data_ptr(),
                                                   tv.data_ptr(), n, per, seed, offset, run.st))
    got_n, got_t = run.done((nw, nv), (tw, tv))
    assert _bits_equal(got_n, ref_noisy.cpu()) and _bits_equal(got_t, sch.get_velocity(x0_d, ref_noise, t_d).cpu())
    assert _bits_equal(got_t, po.velocity(x0, ref_noise.cpu(), sa, sb))
    dev_n, dev_t = sch.add_noise_velocity_device(x0_d, t_d, seed, offset)
    assert _bits_equal(dev_n.cpu(), got_n) and _bits_equal(dev_t.cpu(), got_t)
    assert run.ok and run.inputs_unchanged()


# ---- the weighted loss ------------------------------------------------------------------------------------------------------------
# [5, 3, 9, 31]: five blocks whose stride (1280) is no multiple of per (837) -- the carried sample index wraps
@pytest.mark.parametrize("layout", LAYOUTS + [((5, 3, 9, 31), 0)], ids=LAYOUT_IDS + ["5x3x9x31"])
def test_weighted_loss(layout):
    shape, off = layout
    n = shape[0]
    _, pred, target, _ = _draws(shape, 41 + off)
    run = _Call(shape, off, pred=pred, target=target)
    ws = torch.empty(2048, dtype=torch.float64, device=DEV)

    def entry(w, need_grad=True):
        w_d = _upload(w, off)
        (lw, lv), (dw, dv) = run.out((1,)), run.out()
        _lib.check(run.lib.dsg_mse_loss_weighted(run.dev["pred"].data_ptr(), run.dev["target"].data_ptr(), w_d.data_ptr(), n,
                                                 run.numel // n, 1.0, lv.data_ptr(), dv.data_ptr() if need_grad else None,
                                                 ws.data_ptr(), ws.numel() * 8, run.st))
        loss, dpred = run.done((lw, lv), (dw, dv))
        assert _bits_equal(w_d.cpu(), w)
        return loss, dpred

    # all weights 1: dsg_mse_loss, bit for bit
    ref_loss, ref_dpred = ops.mse_loss(pred.to(DEV), target.to(DEV))
    loss, dpred = entry(torch.ones(n))
    assert _bits_equal(loss, ref_loss.cpu()) and _bits_equal(dpred, ref_dpred.cpu())
    # random positive weights
    w = torch.rand(n, generator=torch.Generator().manual_seed(5)) * 3 + 0.05
    loss, dpred = entry(w)
    want = po.weighted_mse_fp64(pred, target, w)
    print(shape, off, "weighted loss", float(loss), "fp64", want, "rel", abs(float(loss) - want) / want)
    assert _bits_equal(dpred, po.weighted_mse_grad(pred, target, w))
    assert abs(float(loss) - want) <= 1e-6 * want
    loss_only, untouched = entry(w, need_grad=False)
    assert _bits_equal(loss_only, loss) and bool((untouched == POISON).all())
    # a zero weight takes its sample out of the gradient exactly
    w0 = w.clone()
    w0[n // 2] = 0.0
    loss, dpred = entry(w0)
    assert bool((dpred[n // 2] == 0).all()) and _bits_equal(dpred, po.weighted_mse_grad(pred, target, w0))
    assert abs(float(loss) - po.weighted_mse_fp64(pred, target, w0)) <= 1e-6 * po.weighted_mse_fp64(pred, target, w0)
    # through autograd: the gradient arrives at pred
    p = pred.to(DEV).requires_grad_(True)
    out = d.mse_loss(p, target.to(DEV), weights=w.to(DEV))
    out.backward()
    assert _bits_equal(p.grad.cpu(), po.weighted_mse_grad(pred, target, w)) and abs(float(out.detach()) - want) <= 1e-6 * want
    assert run.ok and run.inputs_unchanged()


# ---- not through the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_snr", [False, True], ids=["linear", "zero_snr"])
def test_a_v_step_from_the_true_velocity_lands_on_the_closed_form(zero_snr):
    """x_t = add_noise(x0, z, t), v = get_velocity(x0, z, t): the data prediction is x0 and the noise prediction z, so one DDIM
    step without clipping is sqrt(abar_prev)*x0 + sqrt(1 - abar_prev)*z.  Bound 16 * 2^-24 * (|x0| + |z| + 1) per element: the
    restatement itself stays below 3.4 * 2^-24 * (...) on inputs drawn this way (x0 uniform in [-1, 1], z normal)."""
    sch = d.DDIMScheduler(prediction_type="v_prediction", clip_sample=False, rescale_betas_zero_snr=zero_snr,
                          timestep_spacing="trailing")
    sch.set_timesteps(50)
    shape = (3, 3, 5, 7)
    x0, _, z, _ = _draws(shape, 51)
    x0_d, z_d = x0.to(DEV), z.to(DEV)
    worst = 0.0
    for t in (999, 979, 500, 19, 0):
        tt = torch.tensor([t], device=DEV)
        x_t, v = sch.add_noise_velocity(x0_d, z_d, tt)
        prev = sch.step(v, t, x_t).prev_sample.cpu().double()
        sc = sch.step_scalars(t)
        want = sc["sqrt_alpha_prev"] * x0.double() + sc["dir_coef"] * z.double()
        ratio = float(((prev - want).abs() / (x0.double().abs() + z.double().abs() + 1)).max()) / 2.0 ** -24
        print("zero_snr", zero_snr, "t", t, "error / (2^-24 (|x0| + |z| + 1))", ratio)
        worst = max(worst, ratio)
    assert worst <= 16.0, worst


# ---- scheduler loops ------------------------------------------------------------------------------------------------------------
def _stand_in(x, t, pred):
    """a fixed elementwise 'network' (torch-CPU fp32): something of the size of the quantity `pred` names"""
    k = torch.tensor(0.5 + 0.4 * (t / 999.0), dtype=torch.float32)
    return torch.tanh(x) * k if pred == "sample" else torch.sin(x * 1.7) * k - x * 0.2


def test_a_ten_step_ddim_v_loop_equals_the_restatement():
    shape, steps = (3, 3, 5, 7), 10
    sch = d.DDIMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")
    sch.set_timesteps(steps)
    assert sch.timesteps.tolist()[0] == 999
    x_cpu = torch.randn(shape, generator=torch.Generator().manual_seed(8))
    x = x_cpu.to(DEV)
    for i, t in enumerate(sch.timesteps.tolist()):
        m = _stand_in(x_cpu, t, "v_prediction")
        want = po.ddim_step(x_cpu, m, sch.step_scalars(t), "v_prediction", 1.0)
        out = sch.step(m.to(DEV), t, x).prev_sample
        assert torch.isfinite(want).all() and _bits_equal(out.cpu(), want), (i, t, int((out.cpu() != want).sum()))
        x, x_cpu = out, out.cpu()


def test_a_ten_step_ddpm_sample_loop_equals_the_restatement():
    shape, steps = (3, 3, 5, 7), 10
    sch = d.DDPMScheduler(prediction_type="sample", timestep_spacing="trailing", beta_schedule="squaredcos_cap_v2")
    sch.set_timesteps(steps)
    g, twin = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
    x_cpu = torch.randn(shape, generator=torch.Generator().manual_seed(9))
    x = x_cpu.to(DEV)
    for i, t in enumerate(sch.timesteps.tolist()):
        m = _stand_in(x_cpu, t, "sample")
        z = torch.randn(shape, generator=twin) if t > 0 else None
        want = po.ddpm_step(x_cpu, m, z, sch.step_scalars(t), "sample", 1.0)
        out = sch.step(m.to(DEV), t, x, generator=g).prev_sample
        assert torch.isfinite(want).all() and _bits_equal(out.cpu(), want), (i, t, int((out.cpu() != want).sum()))
        x, x_cpu = out, out.cpu()
    assert torch.equal(g.get_state(), twin.get_state())


# ---- pipeline and training ------------------------------------------------------------------------------------------------------
def _v_scheduler(cls=d.DDIMScheduler, **kw):
    if cls is d.DDIMScheduler:
        kw.setdefault("rescale_betas_zero_snr", True)
    return cls(prediction_type="v_prediction", timestep_spacing="trailing", **kw)


def test_the_ddim_pipeline_runs_a_v_scheduler():
    net = synth_weights(d.UNet2DModel(**CFG1)).to(DEV).eval().requires_grad_(False)
    pipe = d.DDIMPipeline(net, _v_scheduler())
    images = pipe(batch_size=2, generator=torch.Generator().manual_seed(5), num_inference_steps=4, output_type="np.array").images
    assert images.shape == (2, 64, 64, 3) and np.isfinite(images).all()
    # the same call written out: unet + scheduler.step
    sch = _v_scheduler()
    sch.set_timesteps(4)
    assert sch.timesteps.tolist() == [999, 749, 499, 249]
    x = torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        for t in sch.timesteps.tolist():
            x = sch.step(net(x, torch.full((2,), t, device=DEV)).sample, t, x).prev_sample
    want = (x / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(images, want)
    # and it is not what an epsilon scheduler makes of the same network
    eps = d.DDIMPipeline(net, d.DDIMScheduler())(batch_size=2, generator=torch.Generator().manual_seed(5), num_inference_steps=4,
                                                 output_type="np.array").images
    assert not np.array_equal(images, eps)


def _trainer(seed=7):
    from oracle.unet_oracle import OracleUNet2DModel
    torch.manual_seed(seed)
    acc = d.Accelerator(mixed_precision="no")
    net = synth_weights(d.UNet2DModel(**CFG1)).to(DEV)
    opt = d.AdamW(net.parameters(), lr=1e-3)
    lrs = d.get_cosine_schedule_with_warmup(optimizer=opt, num_warmup_steps=1, num_training_steps=10)
    net, opt, lrs = acc.prepare(net, opt, lrs)
    return acc, net, opt, lrs, OracleUNet2DModel(**CFG1).train()


def _two_v_steps(device_noise):
    from drivescenegen_amd import synth
    from drivescenegen_amd.train_loop import DeviceNoise, train_step
    acc, net, opt, lrs, ora = _trainer()
    sch = _v_scheduler(d.DDPMScheduler)
    w_table = po.snr_weights(sch.alphas_cumprod, 5.0, "v_prediction")
    sa_t, sb_t = po.sqrt_tables(sch.alphas_cumprod)
    gen = DeviceNoise(seed=11) if device_noise else None
    before = [p.detach().clone() for p in net.parameters()]
    losses = []
    for k in range(2):
        x0 = torch.from_numpy(synth.synth_scene_rasters(2, 3, 64, 64, 100 + k))
        torch.manual_seed(50 + k)
        t = torch.randint(0, 1000, (2,), device=DEV).long()          # what train_step draws after the same seeding
        torch.manual_seed(50 + k)
        if device_noise:
            noise = sch.add_noise_device(x0.to(DEV), t, gen.seed, (gen.rank << 40) | gen.step)[1].cpu()
            arg = gen
        else:
            noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(60 + k))
            arg = noise.to(DEV)
        # the oracle's weighted v loss on the weights the step starts from
        with torch.no_grad():
            for (name, p), (oname, q) in zip(net.named_parameters(), ora.named_parameters()):
                assert name == oname
                q.copy_(p.detach().cpu())
        tc = t.cpu()
        with torch.no_grad():
            pred_o = ora(po.add_noise(x0, noise, sa_t[tc], sb_t[tc]), tc, return_dict=False)[0]
        want = po.weighted_mse_fp64(pred_o, po.velocity(x0, noise, sa_t[tc], sb_t[tc]), w_table[tc])
        loss = float(train_step(acc, net, sch, opt, lrs, x0.to(DEV), noise=arg, snr_gamma=5.0))
        print("device_noise", device_noise, "step", k, "loss", loss, "oracle", want, "rel", abs(loss - want) / want)
        assert abs(loss - want) <= 1e-5 * want, (k, loss, want)
        losses.append(loss)
    # every weight tensor moved (a bias that is exactly zero with an exactly zero gradient may stay)
    assert all(float((p.detach() - b).abs().max()) > 0 for p, b in zip(net.parameters(), before) if p.dim() >= 2)
    return losses, torch.cat([p.detach().flatten().cpu() for p in net.parameters()])


@pytest.mark.parametrize("device_noise", [False, True], ids=["host_noise", "device_noise"])
def test_train_step_on_a_v_scheduler_with_min_snr_weights(device_noise):
    first, again = _two_v_steps(device_noise), _two_v_steps(device_noise)
    assert first[0] == again[0] and _bits_equal(first[1], again[1])          # same seed, same bits


def test_the_default_train_step_is_the_reference_expression():
    """epsilon scheduler, snr_gamma=None: the loss bits of ``mse_loss(model(add_noise(x0, noise, t), t), noise)`` written out."""
    from drivescenegen_amd import synth
    from drivescenegen_amd.train_loop import train_step
    x0 = torch.from_numpy(synth.synth_scene_rasters(2, 3, 64, 64, 100)).to(DEV)
    noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(60)).to(DEV)
    sch = d.DDPMScheduler()
    acc, net, opt, lrs, _ = _trainer()
    torch.manual_seed(50)
    got = train_step(acc, net, sch, opt, lrs, x0, noise=noise)
    _, net2, _, _, _ = _trainer()
    torch.manual_seed(50)
    t = torch.randint(0, 1000, (2,), device=DEV).long()
    want = d.mse_loss(net2(sch.add_noise(x0, noise, t), t, return_dict=False)[0], noise)
    assert _bits_equal(got.reshape(1).cpu(), want.detach().reshape(1).cpu())
    # "sample": the clean batch is the target
    acc3, net3, opt3, lrs3, _ = _trainer()
    torch.manual_seed(50)
    got = train_step(acc3, net3, d.DDPMScheduler(prediction_type="sample"), opt3, lrs3, x0, noise=noise)
    _, net4, _, _, _ = _trainer()
    want = d.mse_loss(net4(sch.add_noise(x0, noise, t), t, return_dict=False)[0], x0)
    assert _bits_equal(got.reshape(1).cpu(), want.detach().reshape(1).cpu())


def test_fit_with_a_v_scheduler_saves_its_config(tmp_path):
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
    sch = _v_scheduler(d.DDPMScheduler, beta_schedule="squaredcos_cap_v2")
    seen = []
    assert fit(cfg, net, sch, opt, loader, lrs, sample_steps=4, snr_gamma=5.0, on_step=lambda e, r: seen.append(r["loss"])) == 1
    assert len(seen) == 1 and np.isfinite(seen[0]) and seen[0] > 0
    assert sorted(os.listdir(out / "samples")) == ["000.png"]
    saved = d.DDPMPipeline.from_pretrained(str(out))
    assert type(saved.scheduler) is d.DDPMScheduler and saved.scheduler.config.to_dict() == sch.config.to_dict()
    assert d.DDIMPipeline.from_pretrained(str(out)).scheduler.config.prediction_type == "v_prediction"
