"""EMAModel on the GPU: ``dsg_ema_step`` against torch on the CPU evaluating diffusers 0.20.0's literal expression in fp32,
BITWISE (three individually rounded fp32 operations: tolerance zero), with guard margins round every buffer; merged job
tables; the table rebuild after AdamW moves the parameters; eight training steps with the averaged weights tracked step by
step and the training itself untouched; the version bump of ``copy_to`` / ``restore``; the diffusers protocol; ``fit(ema=)``.

tests/redzone_child.py does not list this kernel (existing test files stay as they are): the kernel test here carries its
own >= 4 KiB sentinel margins, the ``_guarded`` idiom of tests/test_gpu_dpmsolver.py."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import drivescenegen_amd as d  # noqa: E402
from drivescenegen_amd import _lib, ops, synth  # noqa: E402
from drivescenegen_amd.train_loop import fit, train_step  # noqa: E402
from tests.common import CFG1, synth_weights  # noqa: E402

DEV = "cuda"
F = np.float32
SENTINEL = 123456.0
MARGIN = 1024                        # floats: 4 KiB; the interior starts 16-byte aligned
CHUNK = 4096                         # DSG_EMA_CHUNK (tests/test_ema_cpu.py holds the header and dsg_ema_job_chunks to it)
SIZES = [1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]
OMDS = [F(1.0), F(0.0), F(1 - 0.9999)]   # the first step (shadow becomes param), shadow unchanged, the steady state


def _guarded(numel, off):
    """(whole buffer, interior view of `numel` floats `off` floats past a 16-byte boundary), SENTINEL on each side (>= 4 KiB)."""
    whole = torch.full((numel + 2 * MARGIN + off,), SENTINEL, dtype=torch.float32, device=DEV)
    inner = whole[MARGIN + off:MARGIN + off + numel]
    assert inner.data_ptr() % 16 == 4 * off
    return whole, inner


def _margins_intact(whole, numel, off):
    w = whole.cpu().numpy()
    return bool((w[:MARGIN + off] == SENTINEL).all() and (w[MARGIN + off + numel:] == SENTINEL).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _oracle(s, p, omd, copy_only):
    """diffusers 0.20.0 EMAModel.step on one parameter, torch on the CPU, fp32."""
    s_param, param = torch.from_numpy(s.copy()), torch.from_numpy(p)
    one_minus_decay = float(F(omd))
    if copy_only:
        s_param.copy_(param)
    else:
        s_param.sub_(one_minus_decay * (s_param - param))
    return s_param.numpy()


def _values(n, seed):
    v = np.random.default_rng(seed).standard_normal(n).astype(F)
    v[::7] = 0.0
    v[3::11] = -0.0
    return v


@pytest.mark.parametrize("p_off,s_off", [(0, 0), (0, 3), (3, 0), (3, 3)])
def test_kernel_is_bitwise_the_cpu_expression_and_stays_inside_its_buffers(p_off, s_off):
    """Every size class in ONE launch (one job each: nothing is merged), param and shadow aligned / 3 floats off independently,
    the three one_minus_decay values, each job once as an averaging job and once as a copy_only one."""
    launches = 0
    for oi, omd in enumerate(OMDS):
        for flip in (0, 1):
            host, dev, jobs = [], [], []
            for i, n in enumerate(SIZES):
                p, s = _values(n, 100 * oi + 2 * i), _values(n, 100 * oi + 2 * i + 1)
                pw, pv = _guarded(n, p_off)
                sw, sv = _guarded(n, s_off)
                pv.copy_(torch.from_numpy(p))
                sv.copy_(torch.from_numpy(s))
                co = (i + flip) % 2 == 1
                host.append((p, s, co))
                dev.append((pw, pv, sw, sv))
                jobs.append((pv.data_ptr(), sv.data_ptr(), n, co))
            table = ops.EmaTable(jobs, DEV, merge=False)
            assert table.n == len(SIZES) and table.total == sum(-(-n // CHUNK) for n in SIZES)
            table.run(omd)
            torch.cuda.synchronize()
            launches += 1
            for n, (p, s, co), (pw, pv, sw, sv) in zip(SIZES, host, dev):
                what = (float(omd), n, co, p_off, s_off)
                got, want = sv.cpu().numpy(), _oracle(s, p, omd, co)
                assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))
                assert np.array_equal(_bits(pv.cpu().numpy()), _bits(p)), what          # the parameter is only read
                assert _margins_intact(pw, n, p_off) and _margins_intact(sw, n, s_off), what
                if co:
                    assert np.array_equal(_bits(got), _bits(p)), what
                elif omd == 0:
                    assert np.array_equal(_bits(got), _bits(s)), what
    assert launches == 6


def test_raw_abi_call_and_empty_table():
    """The C entry point with a hand-built table (the ABI, not the wrapper); njobs == 0 launches nothing."""
    lib = _lib.load()
    n = CHUNK + 5
    p, s = _values(n, 1), _values(n, 2)
    pw, pv = _guarded(n, 0)
    sw, sv = _guarded(n, 0)
    pv.copy_(torch.from_numpy(p))
    sv.copy_(torch.from_numpy(s))
    job = _lib.EmaJob(param=pv.data_ptr(), shadow=sv.data_ptr(), numel=n, copy_only=0)
    chunks = ctypes.c_int64()
    _lib.check(lib.dsg_ema_job_chunks(ctypes.byref(job), ctypes.byref(chunks)))
    assert chunks.value == 2
    jobs = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).to(DEV)
    first = torch.tensor([0, 2], dtype=torch.int64, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    _lib.check(lib.dsg_ema_step(None, None, 0, 0, 0.5, st))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(sv.cpu().numpy()), _bits(s))
    _lib.check(lib.dsg_ema_step(jobs.data_ptr(), first.data_ptr(), 1, 2, 0.25, st))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(sv.cpu().numpy()), _bits(_oracle(s, p, 0.25, False)))
    assert _margins_intact(pw, n, 0) and _margins_intact(sw, n, 0)


def test_merged_jobs_give_the_bits_of_one_job_per_slice():
    """Slices that are contiguous in both buffers merge into one job (mixed copy_only: one job per run); same bits as one
    job per slice, and as the CPU expression."""
    sizes = [5, 64, CHUNK + 3, 1, 2 * CHUNK + 8]
    total = sum(sizes)
    p, s = _values(total, 11), _values(total, 12)
    omd = F(1 - 0.9999)
    for copy_only, njobs in (([False] * 5, 1), ([False, False, True, True, False], 3)):
        out = {}
        for merge in (False, True):
            pw, pv = _guarded(total, 0)
            sw, sv = _guarded(total, 0)
            pv.copy_(torch.from_numpy(p))
            sv.copy_(torch.from_numpy(s))
            cuts = np.cumsum([0] + sizes)
            table = ops.ema_step_([pv[a:b] for a, b in zip(cuts, cuts[1:])], [sv[a:b] for a, b in zip(cuts, cuts[1:])], omd,
                                  copy_only=copy_only, merge=merge)
            torch.cuda.synchronize()
            assert table.n == (njobs if merge else len(sizes))
            assert _margins_intact(pw, total, 0) and _margins_intact(sw, total, 0)
            out[merge] = sv.cpu().numpy()
        want = np.concatenate([_oracle(s[a:b], p[a:b], omd, co) for a, b, co in zip(cuts, cuts[1:], copy_only)])
        assert np.array_equal(_bits(out[True]), _bits(out[False])) and np.array_equal(_bits(out[True]), _bits(want))


def _flat_cpu(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu()


def _recur(shadow_cpu, params_cpu, decay):
    """One diffusers step on the CPU over the concatenated parameters (every one requires_grad)."""
    shadow_cpu.sub_(float(F(1 - decay)) * (shadow_cpu - params_cpu))


def test_table_is_rebuilt_when_adamw_moves_the_parameters():
    """AdamW's first step moves every p.data into its slab: pointers cached before it are stale.  The step after it must
    average the MOVED parameters -- and they now sit at the shadow's own offsets, so the table is one job."""
    net = synth_weights(d.UNet2DModel(**CFG1)).to(DEV).train()
    params = list(net.parameters())
    ema = d.EMAModel(params, decay=0.75)
    want = _flat_cpu(params)
    ema.step(net.parameters())
    _recur(want, _flat_cpu(params), ema.get_decay(1))
    assert ema.cur_decay_value == 0.0 and torch.equal(_flat_cpu(ema.shadow_params), want)
    before = [p.data_ptr() for p in params]
    x = torch.from_numpy(synth.normal(3, (2, 3, 64, 64))).to(DEV)
    opt = d.AdamW(net.parameters(), lr=1e-2)
    d.mse_loss(net(x, torch.tensor([10, 700], device=DEV), return_dict=False)[0], torch.zeros_like(x)).backward()
    opt.step()
    assert all(p.data_ptr() != b for p, b in zip(params, before))
    moved = _flat_cpu(params)
    assert not torch.equal(moved, want)
    for k in (2, 3):
        ema.step(net.parameters())
        _recur(want, moved, ema.get_decay(k))
        assert ema.optimization_step == k and ema.cur_decay_value == ema.get_decay(k) > 0
        assert torch.equal(_flat_cpu(ema.shadow_params), want), k
    assert ema._table.n == 1
    assert torch.equal(_flat_cpu(params), moved)
    pad = ema._pad_index()
    assert pad.numel() and not bool(ema._flat.cpu()[pad].ne(0).any())    # the shadow buffer's padding is still zero


def _eight_steps(mode, with_ema):
    torch.manual_seed(7)
    acc = d.Accelerator(mixed_precision=mode)
    net = synth_weights(d.UNet2DModel(**CFG1)).to(DEV)
    opt = d.AdamW(net.parameters(), lr=1e-3)
    lrs = d.get_cosine_schedule_with_warmup(optimizer=opt, num_warmup_steps=2, num_training_steps=100)
    net, opt, lrs = acc.prepare(net, opt, lrs)
    sch = d.DDPMScheduler()
    data = [torch.from_numpy(synth.synth_scene_rasters(2, 3, 64, 64, 100 + i)).to(DEV) for i in range(3)]
    ema = d.EMAModel(net.parameters()) if with_ema else None
    want = _flat_cpu(net.parameters())
    losses = []
    for k in range(8):
        losses.append(train_step(acc, net, sch, opt, lrs, data[k % 3], ema=ema) if with_ema
                      else train_step(acc, net, sch, opt, lrs, data[k % 3]))
        if with_ema:
            _recur(want, _flat_cpu(net.parameters()), ema.get_decay(k + 1))
            assert ema.optimization_step == k + 1
            assert torch.equal(_flat_cpu(ema.shadow_params), want), (mode, k)
    if with_ema:
        assert not torch.equal(want, _flat_cpu(net.parameters()))     # an average, not a copy of the last step
    return [float(l) for l in losses]


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_eight_training_steps_track_the_cpu_recurrence_and_leave_training_alone(mode):
    with_ema = _eight_steps(mode, True)
    without = _eight_steps(mode, False)
    assert len(with_ema) == 8 and all(np.isfinite(with_ema)) and with_ema == without, (with_ema, without)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_copy_to_and_restore_reach_the_next_forward(dtype):
    """copy_to / restore write through raw pointers; the plan's weight copies are refreshed by the version counter."""
    net = synth_weights(d.UNet2DModel(**CFG1)).to(DEV).set_compute_dtype(dtype)
    other = synth_weights(d.UNet2DModel(**CFG1), seed=99).to(DEV)
    ema = d.EMAModel(other.parameters())
    x = torch.from_numpy(synth.normal(5, (2, 3, 64, 64))).to(DEV)
    t = torch.tensor([20, 800], device=DEV)
    with torch.no_grad():
        y0 = net(x, t).sample.clone()
        ema.store(net.parameters())
        ema.copy_to(net.parameters())
        y1 = net(x, t).sample.clone()
        fresh = d.UNet2DModel(**CFG1)
        fresh.load_state_dict({k: s.cpu() for k, s in zip(fresh.state_dict(), ema.shadow_params)})
        want = fresh.to(DEV).set_compute_dtype(dtype)(x, t).sample
        assert torch.equal(y1, want) and not torch.equal(y1, y0)
        ema.restore(net.parameters())
        assert torch.equal(net(x, t).sample, y0)
    assert ema.temp_stored_params is None


def test_protocol_state_dict_and_checkpoint_folder(tmp_path):
    net = synth_weights(d.UNet2DModel(**CFG1)).to(DEV)
    ema = d.EMAModel(net.parameters(), decay=0.95, min_decay=0.25, update_after_step=1, use_ema_warmup=True, inv_gamma=2.0,
                     power=0.75, model_cls=d.UNet2DModel, model_config=net.config)
    with pytest.raises(RuntimeError, match="store"):
        ema.restore(net.parameters())
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.5)
    for k in range(4):
        if k == 2:   # (the first two steps have decay 0: the shadows ARE the parameters; move them again so that the average is not)
            with torch.no_grad():
                for p in net.parameters():
                    p.mul_(1.25)
        ema.step(net.parameters())
    assert ema.optimization_step == 4 and ema.cur_decay_value == ema.get_decay(4)
    sd = ema.state_dict()
    assert sorted(sd) == sorted(["decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma",
                                 "power", "shadow_params"])
    scalars = {k: v for k, v in sd.items() if k != "shadow_params"}
    again = d.EMAModel(net.parameters())
    again.load_state_dict(sd)
    assert {k: v for k, v in again.state_dict().items() if k != "shadow_params"} == scalars
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(again.shadow_params, ema.shadow_params))
    for bad in (dict(decay=2.0), dict(min_decay=0), dict(optimization_step=1.5), dict(use_ema_warmup=1), dict(power="x"),
                dict(shadow_params=(1,)), dict(shadow_params=[1])):
        with pytest.raises(ValueError):
            d.EMAModel(net.parameters()).load_state_dict(bad)
    with pytest.raises(ValueError, match="model_cls"):
        d.EMAModel(net.parameters()).save_pretrained(str(tmp_path / "none"))
    ema.to(DEV)
    with pytest.raises(RuntimeError):
        ema.to(dtype=torch.float16)
    out = str(tmp_path / "unet_ema")
    ema.save_pretrained(out)
    back = d.EMAModel.from_pretrained(out, d.UNet2DModel)
    assert {k: v for k, v in back.state_dict().items() if k != "shadow_params"} == scalars
    assert all(torch.equal(a, b) for a, b in zip(back.shadow_params, ema.shadow_params))
    plain = d.UNet2DModel.from_pretrained(out)                   # the folder is also a plain model checkpoint
    assert all(torch.equal(p.detach(), s.cpu()) for p, s in zip(plain.parameters(), ema.shadow_params))
    assert not torch.equal(_flat_cpu(net.parameters()), _flat_cpu(ema.shadow_params))   # an average, not the live weights


def _png_folder(root, count, side=64):
    from PIL import Image
    root.mkdir()
    rasters = synth.synth_scene_rasters(count, 3, side, side, 3)
    for k, r in enumerate(rasters):
        Image.fromarray(((r.transpose(1, 2, 0) * 0.5 + 0.5) * 255).round().astype(np.uint8)).save(root / f"{k}.png")
    return str(root / "*")


def test_fit_samples_and_saves_the_averaged_weights_and_trains_on_the_raw_ones(tmp_path):
    from drivescenegen_amd.dataset import Image_Dataset
    pngs = _png_folder(tmp_path / "pngs", 6)
    live, ema = {}, None
    for with_ema in (False, True):
        out = tmp_path / f"run{int(with_ema)}"
        cfg = SimpleNamespace(dataset_name=pngs, patterns_size_height=64, patterns_size_width=64, mixed_precision="no",
                              gradient_accumulation_steps=1, output_dir=str(out), num_epochs=2, save_image_epochs=1,
                              save_model_epochs=5, eval_batch_size=1, seed=14555, learning_rate=1e-3)
        torch.manual_seed(3)
        net = synth_weights(d.UNet2DModel(**CFG1)).to(DEV)
        loader = torch.utils.data.DataLoader(Image_Dataset(cfg), batch_size=4, shuffle=True)
        opt = d.AdamW(net.parameters(), lr=cfg.learning_rate)
        lrs = d.get_cosine_schedule_with_warmup(optimizer=opt, num_warmup_steps=1, num_training_steps=4)
        ema = d.EMAModel(net.parameters()) if with_ema else None
        assert fit(cfg, net, d.DDPMScheduler(), opt, loader, lrs, sample_steps=4, ema=ema) == 4
        live[with_ema] = [p.detach().clone() for p in net.parameters()]
        assert os.path.exists(out / "unet_ema" / "config.json") == with_ema
        assert sorted(os.listdir(out / "samples")) == ["000.png", "001.png"]
    assert all(torch.equal(a, b) for a, b in zip(live[True], live[False]))           # training never saw the averaged weights
    assert ema.optimization_step == 4 and ema.model_cls is d.UNet2DModel and ema.temp_stored_params is None
    assert not all(torch.equal(a, s) for a, s in zip(live[True], ema.shadow_params))
    saved = d.UNet2DModel.from_pretrained(str(tmp_path / "run1"), subfolder="unet")
    assert all(torch.equal(p.detach(), s.cpu()) for p, s in zip(saved.parameters(), ema.shadow_params))
    back = d.EMAModel.from_pretrained(str(tmp_path / "run1" / "unet_ema"), d.UNet2DModel)
    assert back.optimization_step == 4 and back.decay == ema.decay
    assert all(torch.equal(a, b) for a, b in zip(back.shadow_params, ema.shadow_params))
