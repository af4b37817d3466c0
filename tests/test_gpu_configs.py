"""Every BASELINE.json config at its own size (configs_untested): configs[2] -- a training step of the
256x256x4 default network against torch-CPU autograd of the oracle plus a batch-64 size-independent property --,
configs[3] -- the 6-level 512x512 attention network (SURVEY 8d reading, 66,294,660 parameters) --, configs[4] -- a bf16
training step of the 8-channel network plus its batch-128 property --, the reference's own training operating point
(fp16 AMP, batch 14, train.py:16,24) and its own sampling call (750-step seeded DDPM at batch 1,
training_pipeline.py:26-32) teacher-forced against the oracle.

The full-size oracle results these tests compare with are committed golden vectors (tests/golden/fullsize_golden.npz,
made by tests/golden/make_fullsize_golden.py from the same torch-CPU oracle; the CPU suite re-runs the oracle against
them): the GPU box's host cores are shared and a 56-66 M-parameter oracle pass costs them seconds to a minute each
(848 s of the driver's 1200 s).  The oracle still runs LIVE here where the input only exists at run time
(the teacher-forced checkpoints of the free-running 750-step trajectory)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import synth  # noqa: E402
from oracle.scheduler_oracle import OracleDDPMScheduler  # noqa: E402
from oracle.unet_oracle import OracleUNet2DModel  # noqa: E402
from tests.common import (CFG3, CFG4, CFG5, DEFAULT3, DEFAULT3_STEP_TS, PARAM_COUNTS, assert_matches_fullsize_golden,  # noqa: E402
                          compare_grads_with_golden, fullsize_case, fullsize_golden, fullsize_train_case, max_abs,
                          noisy_inputs, rel_l2, synth_weights)

DEV = "cuda"


def _train_inputs(cfg, b, seed=5):
    ss = cfg["sample_size"]
    h, w = (ss, ss) if isinstance(ss, int) else ss
    x0 = torch.from_numpy(synth.synth_scene_rasters(b, cfg["in_channels"], h, w, seed))
    noise = torch.from_numpy(synth.normal(seed + 1, tuple(x0.shape)))
    t = torch.from_numpy((synth.uniform01(seed + 2, b) * 1000).astype(np.int64))
    return x0, noise, t


def test_cfg3_training_step_256_vs_oracle_autograd():
    """configs[2] network (256x256x4, 56,575,748 parameters): loss and all 282 gradients of one DDPM training step at
    batch 2 against torch-CPU autograd of the fp32 oracle (stored: the loss, every gradient's L2 norm and <= 512 evenly
    spaced entries of each)."""
    cfg, x0, noise, t = fullsize_train_case("cfg3_train_b2")
    loss_o = float(fullsize_golden()["cfg3_train_b2/loss"][0])
    net = synth_weights(d.UNet2DModel(**cfg)).to(DEV).train()
    assert sum(p.numel() for p in net.parameters()) == PARAM_COUNTS["CFG2"] and len(list(net.parameters())) == 282
    noisy = d.DDPMScheduler().add_noise(x0.to(DEV), noise.to(DEV), t.to(DEV))   # (bit-exact vs the oracle's: test_gpu_ops)
    loss = d.mse_loss(net(noisy, t.to(DEV), return_dict=False)[0], noise.to(DEV))
    loss.backward()
    assert abs(float(loss.detach().cpu()) - loss_o) <= 2e-5 * loss_o
    err, norm_err, bad = compare_grads_with_golden(((n, p.grad) for n, p in net.named_parameters()), "cfg3_train_b2")
    assert err <= 1e-4, err
    assert norm_err <= 5e-4, norm_err
    assert not bad, bad[:8]


def test_cfg3_batch64_gradients_equal_those_of_the_repeated_pair():
    """configs[2] at its own batch (64 per GPU): a mean-reduced loss over 32 copies of a 2-sample batch has the
    gradients of the 2-sample batch -- a size-independent check of the full-size backward (split-K over 64 images,
    bucket / slab arithmetic), finite everywhere, within the memory of one MI355X."""
    x0, noise, t = _train_inputs(CFG3, 2, seed=9)
    sch = d.DDPMScheduler()
    net = synth_weights(d.UNet2DModel(**CFG3)).to(DEV).train()
    noisy = sch.add_noise(x0.to(DEV), noise.to(DEV), t.to(DEV))
    d.mse_loss(net(noisy, t.to(DEV), return_dict=False)[0], noise.to(DEV)).backward()
    small = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    for p in net.parameters():
        p.grad.zero_()
    torch.cuda.reset_peak_memory_stats()
    rep = lambda a: a.to(DEV).repeat(32, *([1] * (a.dim() - 1)))
    loss = d.mse_loss(net(rep(noisy), rep(t), return_dict=False)[0], rep(noise))
    loss.backward()
    assert torch.isfinite(loss.detach()).all()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    assert peak < 200, peak
    worst = 0.0
    for n, p in net.named_parameters():
        assert torch.isfinite(p.grad).all(), n
        if float(small[n].norm()) > 1e-7:
            worst = max(worst, rel_l2(p.grad.cpu(), small[n].cpu()))
    assert worst <= 5e-4, worst


def test_cfg4_six_level_512_forward_vs_oracle_and_row_independence():
    """configs[3]: 512x512x4, (64,64,128,128,256,512), attention at 32^2 and 16^2 (66,294,660 parameters): batch-1
    forward against the CPU oracle, and at the config's batch 8 every row equals its own batch-1 run bit for bit."""
    net = synth_weights(d.UNet2DModel(**CFG4)).to(DEV).eval().requires_grad_(False)
    assert sum(p.numel() for p in net.parameters()) == PARAM_COUNTS["CFG4"]
    from tests.common import same_kernels_at_any_batch
    x = noisy_inputs(CFG4, 8)
    t = torch.tensor([990, 700, 500, 300, 100, 50, 10, 0])
    with same_kernels_at_any_batch():   # (its 16^2 levels are small grids even at batch 8: K would be cut by batch size)
        got = net(x.to(DEV), t.to(DEV)).sample
    fast = net(x.to(DEV), t.to(DEV)).sample
    assert rel_l2(fast.cpu(), got.cpu()) <= 2e-6
    assert torch.isfinite(got).all()
    assert torch.equal(fullsize_case("cfg4_b8_row0_t990")[2], x[:1])
    assert_matches_fullsize_golden(got[:1], "cfg4_b8_row0_t990")   # (the oracle's stored output: every 2nd pixel + whole-map moments)
    for i in (3, 7):
        with same_kernels_at_any_batch():
            assert torch.equal(net(x[i:i + 1].to(DEV), t[i:i + 1].to(DEV)).sample, got[i:i + 1])
        assert rel_l2(net(x[i:i + 1].to(DEV), t[i:i + 1].to(DEV)).sample.cpu(), got[i:i + 1].cpu()) <= 2e-6


def test_cfg5_bf16_training_step_256_vs_oracle_autograd():
    """configs[4] network (256x256x8, 56,580,360 parameters), one mixed-bf16 training step at batch 2 against fp32
    autograd of the oracle (stored): loss within 1e-2, the gradient vector within 3e-2 (rel-L2 over the stored entries),
    every gradient tensor's norm within 6e-2."""
    cfg, x0, noise, t = fullsize_train_case("cfg5_train_b2")
    loss_o = float(fullsize_golden()["cfg5_train_b2/loss"][0])
    net = synth_weights(d.UNet2DModel(**cfg)).to(DEV).train().set_compute_dtype("bf16")
    noisy = d.DDPMScheduler().add_noise(x0.to(DEV), noise.to(DEV), t.to(DEV))
    loss = d.mse_loss(net(noisy, t.to(DEV), return_dict=False)[0], noise.to(DEV))
    loss.backward()
    assert abs(float(loss.detach().cpu()) - loss_o) <= 1e-2 * loss_o
    err, norm_err, _ = compare_grads_with_golden(((n, p.grad) for n, p in net.named_parameters()), "cfg5_train_b2")
    assert err <= 3e-2, err
    assert norm_err <= 6e-2, norm_err


def test_cfg5_bf16_batch128_rows_are_independent():
    """configs[4] at its own batch (128 per GPU, mixed bf16): three rows of the batch-128 forward equal their own batch-1
    runs bit for bit, everything is finite, and the call stays far inside one MI355X's memory."""
    net = synth_weights(d.UNet2DModel(**CFG5)).to(DEV).eval().requires_grad_(False).set_compute_dtype("bf16")
    x8 = noisy_inputs(CFG5, 8)
    x = x8.repeat(16, 1, 1, 1)
    x[5], x[77], x[127] = x8[1] * 0.5, -x8[2], x8[3].flip(-1)        # rows that are nobody's copy
    t = (torch.arange(128) * 7) % 1000
    torch.cuda.reset_peak_memory_stats()
    out = net(x.to(DEV), t.to(DEV)).sample
    assert out.shape == (128, 8, 256, 256) and torch.isfinite(out).all()
    assert torch.cuda.max_memory_allocated() / 2 ** 30 < 100
    for i in (5, 77, 127):
        assert torch.equal(net(x[i:i + 1].to(DEV), t[i:i + 1].to(DEV)).sample, out[i:i + 1]), i
    assert torch.equal(out[0], out[8]) is False and rel_l2(out[8].cpu(), out[0].cpu()) > 1e-3   # (different timesteps)


def test_cfg5_bf16_batch128_gradients_equal_those_of_the_repeated_pair():
    """configs[4] at its own batch (128 per GPU, mixed bf16), TRAINING: a mean-reduced loss over 64 copies of the stored
    2-sample batch has that batch's gradients -- the twin of the configs[2] test above for the 16-bit tape (weight gradients
    summed over 128 images, GroupNorm backward, the wide weight-gradient workgroups), finite everywhere and inside one
    MI355X's memory.  Tolerance: bf16 products, fp32 accumulation -- the order of a 128-image sum against a 2-image sum moves
    a gradient by a few 1e-3 relative; the 2-sample step itself is checked against the oracle's autograd in the test above."""
    cfg, x0, noise, t = fullsize_train_case("cfg5_train_b2")
    sch = d.DDPMScheduler()
    net = synth_weights(d.UNet2DModel(**cfg)).to(DEV).train().set_compute_dtype("bf16")
    noisy = sch.add_noise(x0.to(DEV), noise.to(DEV), t.to(DEV))
    loss2 = d.mse_loss(net(noisy, t.to(DEV), return_dict=False)[0], noise.to(DEV))
    loss2.backward()
    small = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    for p in net.parameters():
        p.grad.zero_()
    torch.cuda.reset_peak_memory_stats()
    rep = lambda a: a.to(DEV).repeat(64, *([1] * (a.dim() - 1)))
    loss = d.mse_loss(net(rep(noisy), rep(t), return_dict=False)[0], rep(noise))
    loss.backward()
    assert torch.isfinite(loss.detach()).all()
    assert abs(float(loss.detach()) - float(loss2.detach())) <= 2e-3 * float(loss2.detach())
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    assert peak < 100, peak
    # (round 6: at batch 128 the GroupNorm-backward statistics come out of the data-gradient convs' epilogues, at batch 2 -- small
    #  grids -- mostly from the statistics pass: two roundings of the same sums.  With the pass on both sides the two gradients were
    #  bit-identical; now they differ at the tape's own noise level, most on the tensors whose gradient is three orders of
    #  magnitude below the others -- the attention block's to_q / to_k at ~1e-5 against ~1e-2.  Both stay in the same distance
    #  from the oracle's autograd: 2.981e-3 / 2.983e-3 of the gradient vector.)
    worst, worst_small, num, den = 0.0, 0.0, 0.0, 0.0
    top = max(float(g.norm()) for g in small.values())
    for n, p in net.named_parameters():
        assert torch.isfinite(p.grad).all(), n
        if float(small[n].norm()) > 1e-3 * top:
            worst = max(worst, rel_l2(p.grad.cpu(), small[n].cpu()))
        elif float(small[n].norm()) > 1e-7:
            worst_small = max(worst_small, rel_l2(p.grad.cpu(), small[n].cpu()))
        num += float((p.grad - small[n]).double().pow(2).sum())
        den += float(small[n].double().pow(2).sum())
    assert (num / den) ** 0.5 <= 5e-3, (num / den) ** 0.5     # the whole gradient vector
    assert worst <= 2e-2, worst                               # every tensor on its own
    assert worst_small <= 6e-2, worst_small                   # ... the ones that are mostly rounding noise
    err, norm_err, _ = compare_grads_with_golden(((n, p.grad) for n, p in net.named_parameters()), "cfg5_train_b2")
    assert err <= 3e-2 and norm_err <= 6e-2, (err, norm_err)  # and the batch-128 gradients against the oracle's autograd directly


def _train_step_fp16(net, noisy, t, noise, scale=65536.0):
    """One fp16-AMP backward as accelerate drives it (training_pipeline.py:48-49,84-88): scaled loss, then unscale."""
    from drivescenegen_amd.training import GradScaler, _ScaleLoss
    sc = GradScaler(init_scale=scale)
    loss = d.mse_loss(net(noisy, t, return_dict=False)[0], noise)
    _ScaleLoss.apply(loss, sc.get_scale()).backward()
    params = list(net.parameters())
    sc.unscale_(params)
    assert not bool(sc._found.item())
    return float(loss.detach().cpu())


def test_reference_operating_point_fp16_amp_default_net():
    """The reference's own training configuration (train.py:16,24,39-57): the 3-channel default network under fp16 AMP with
    the GradScaler.  Batch 2: loss and gradients against fp32 autograd of the oracle (stored: default3_train_b2);
    batch 14 = the reference's: seven copies of the pair give the pair's gradients (mean-reduced loss), finite throughout."""
    cfg, x0, noise, t = fullsize_train_case("default3_train_b2")
    loss_o = float(fullsize_golden()["default3_train_b2/loss"][0])
    net = synth_weights(d.UNet2DModel(**cfg)).to(DEV).train().set_compute_dtype("fp16")
    noisy = d.DDPMScheduler().add_noise(x0.to(DEV), noise.to(DEV), t.to(DEV))
    loss = _train_step_fp16(net, noisy, t.to(DEV), noise.to(DEV))
    assert abs(loss - loss_o) <= 1e-2 * loss_o
    err, norm_err, _ = compare_grads_with_golden(((n, p.grad) for n, p in net.named_parameters()), "default3_train_b2")
    assert err <= 1e-2, err            # (fp16 carries 3 more mantissa bits than bf16: measured ~1e-3)
    assert norm_err <= 2e-2, norm_err
    small = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    for p in net.parameters():
        p.grad.zero_()
    rep = lambda a: a.repeat(7, *([1] * (a.dim() - 1)))
    _train_step_fp16(net, rep(noisy), rep(t.to(DEV)), rep(noise.to(DEV)))
    worst = 0.0
    for n, p in net.named_parameters():
        assert torch.isfinite(p.grad).all(), n
        if float(small[n].norm()) > 1e-7:
            worst = max(worst, rel_l2(p.grad.cpu(), small[n].cpu()))
    assert worst <= 5e-3, worst


def test_reference_evaluate_call_750_steps_teacher_forced():
    """training_pipeline.py:26-32: 750-step DDPM, batch 1, CPU generator seeded 14555, on the train.py:39-57 network.
    The engine free-runs the whole trajectory; at t = 749, 499, 249 and 0 its x_t is handed to the LIVE CPU oracle, whose
    eps and x_{t-1} for that step must agree (rel-L2 <= 1e-4): teacher-forced checkpoints on inputs that only exist at run
    time.  Every 50th timestep of the 749 ... 0 table is additionally checked on a synthetic x_t against the oracle's
    stored eps (16 cases, tests/golden).  The pipeline object, seeded the same way, reproduces the free-running result
    bit for bit."""
    net = synth_weights(d.UNet2DModel(**DEFAULT3)).to(DEV).eval().requires_grad_(False)
    ora = synth_weights(OracleUNet2DModel(**DEFAULT3)).eval()
    sch, osch = d.DDPMScheduler(), OracleDDPMScheduler()
    sch.set_timesteps(750)
    osch.set_timesteps(750)
    assert [int(v) for v in sch.timesteps[:3]] == [749, 748, 747] and int(sch.timesteps[-1]) == 0
    gen = torch.manual_seed(14555)
    x = torch.randn((1, 3, 256, 256), generator=gen).to(DEV)
    checked = 0
    for i, tt in enumerate(sch.timesteps):
        t = int(tt)
        eps = net(x, t).sample
        noise = torch.randn((1, 3, 256, 256), generator=gen) if t > 0 else None
        nxt = sch.step(eps, t, x, variance_noise=None if noise is None else noise.to(DEV)).prev_sample
        if i % 250 == 0 or t == 0:
            with torch.no_grad():
                oeps = ora(x.cpu(), t).sample
            onxt = osch.step(oeps, t, x.cpu(), noise=noise).prev_sample
            assert rel_l2(eps.cpu(), oeps) <= 1e-4, (t, rel_l2(eps.cpu(), oeps))
            assert rel_l2(nxt.cpu(), onxt) <= 1e-4, (t, rel_l2(nxt.cpu(), onxt))
            checked += 1
        x = nxt
    assert checked == 4 and torch.isfinite(x).all()
    for ts in DEFAULT3_STEP_TS:   # 749, 699, ..., 49, 0: the timestep embedding path at every stretch of the table
        _, _, xs, tt, _ = fullsize_case(f"default3_step_t{ts}")
        assert_matches_fullsize_golden(net(xs.to(DEV), tt).sample, f"default3_step_t{ts}")
    pipe = d.DDPMPipeline(unet=net, scheduler=d.DDPMScheduler())
    img = pipe(num_inference_steps=750, batch_size=1, generator=torch.manual_seed(14555), output_type="np.array",
               return_dict=False)[0]
    want = (x.cpu() / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy()
    assert img.shape == (1, 256, 256, 3) and np.array_equal(img, want)


def test_generation_batch5_forward_vs_live_oracle_and_selection_rules():
    """generation.py:14-20 samples at batch 5 on the train.py:39-57 network: at that batch the 32 x 32 level runs the
    three-slice split-K with 16-row tiles and the 64 x 64 level the 64-cout slices (the rows_rule switch, default on; ADVICE r05: no
    whole-net check existed at this batch).  One forward of 5 different x_t at 5 timesteps against the LIVE CPU oracle
    (rel-L2 <= 1e-4 per row), and rows_rule = 0 (the round-4 selection) gives the same eps BIT FOR BIT: at this batch
    the rule changes tile HEIGHT under the same three K slices, and tile geometry never changes a bit (per-pixel summation
    order and the 8 x 32 statistics tiles are geometry-independent by construction)."""
    from drivescenegen_amd import ops
    net = synth_weights(d.UNet2DModel(**DEFAULT3)).to(DEV).eval().requires_grad_(False)
    ora = synth_weights(OracleUNet2DModel(**DEFAULT3)).eval()
    x = noisy_inputs(DEFAULT3, 5)
    t = torch.tensor([749, 500, 250, 20, 0])
    got = {}
    for on in (1, 0):
        with ops.tuning(rows_rule=on):
            got[on] = net(x.to(DEV), t.to(DEV)).sample.cpu()
    with torch.no_grad():
        want = ora(x, t).sample
    for i in range(5):
        assert rel_l2(got[1][i], want[i]) <= 1e-4, (i, rel_l2(got[1][i], want[i]))
        assert rel_l2(got[0][i], want[i]) <= 1e-4, i
    assert torch.equal(got[0], got[1])
