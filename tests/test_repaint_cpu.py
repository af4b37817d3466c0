"""RePaint (scene completion) -- everything that needs no GPU: the jump schedule against known answers, the host scalars
against the NumPy restatement (tests/repaint_oracle.py), config I/O, the C ABI's argument checks (made before any HIP call),
and the pipeline's input handling (refused before a kernel runs)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import drivescenegen_amd as d
from drivescenegen_amd import _lib
from tests import repaint_oracle as ro
from tests.common import CFG1


def _entries(ts):
    p = ro.plan(ts)
    return len(ts), sum(p), len(p) - sum(p)


@pytest.mark.parametrize("args,counts", [((250, 10, 10), (4570, 2410, 2160)), ((50, 5, 3), (230, 140, 90)),
                                         ((20, 10, 1), (20, 20, 0))])
def test_timestep_table_entry_counts(lib_built, args, counts):
    s = d.RePaintScheduler()
    s.set_timesteps(*args)
    ts = s.timesteps.numpy()
    assert ts.dtype == np.int64 and _entries(ts) == counts
    assert np.array_equal(ts, ro.timesteps(*args))
    if args == (250, 10, 10):
        assert list(ts[:3]) == [996, 992, 988] and list(ts[-3:]) == [8, 4, 0]
    if args == (20, 10, 1):
        ddim = d.DDIMScheduler()
        ddim.set_timesteps(20)
        assert torch.equal(s.timesteps, ddim.timesteps)


def test_timestep_tables_known_answers(lib_built):
    s = d.RePaintScheduler()
    s.set_timesteps(8, 3, 2)
    assert s.timesteps.tolist() == [875, 750, 625, 500, 375, 500, 625, 750, 625, 500, 375, 250, 125, 0, 125, 250, 375, 250,
                                    125, 0]
    s.set_timesteps(10, jump_length=2, jump_n_sample=2)
    assert s.timesteps.tolist() == [900, 800, 700, 600, 700, 800, 700, 600, 500, 400, 500, 600, 500, 400, 300, 200, 300, 400,
                                    300, 200, 100, 0, 100, 200, 100, 0]
    s.set_timesteps(5000)                       # min(num_train_timesteps, num_inference_steps)
    assert s.num_inference_steps == 1000 and int(s.timesteps[0]) == 999


def test_host_scalars_equal_the_numpy_restatement(lib_built):
    """Every fp32 scalar the kernels are given, for every entry of three schedules and eta 0 / 0.3 / 1: the scheduler (torch 0-d
    fp32 tensors, DDIMScheduler._step_scalars' order) against NumPy fp32, bit for bit."""
    s = d.RePaintScheduler()
    betas, acp = ro.tables()
    assert np.array_equal(s.betas.numpy(), betas) and np.array_equal(s.alphas_cumprod.numpy(), acp)
    assert float(s.final_alpha_cumprod) == 1.0
    for n, jl, jn in ((8, 3, 2), (50, 5, 3), (1000, 10, 1)):
        s.set_timesteps(n, jl, jn)
        for t in sorted(set(s.timesteps.tolist())):
            for eta in (0.0, 0.3, 1.0):
                got, want = s.step_scalars(t, eta), ro.step_scalars(t, n, eta, tabs=(betas, acp))
                for a, b in (("sqrt_beta_prod_t", "sb"), ("sqrt_alpha_prod_t", "sa"), ("sqrt_alpha_prev", "sap"),
                             ("dir_coef", "dc"), ("std", "std"), ("sqrt_beta_prev", "sbp")):
                    assert np.float32(got[a]) == want[b] and got[a] == float(want[b]), (n, t, eta, a, got[a], want[b])
            if n < 1000 or t % 100 == 0:
                passes, fused = s.undo_scalars(t) if t + 1000 // n <= 1000 else (None, None)
                if passes is not None:
                    assert passes == [(float(a), float(b)) for a, b in ro.undo_scalars(t, n, tabs=(betas, acp))]
                    assert fused == tuple(float(v) for v in ro.undo_scalars_fused(t, n, tabs=(betas, acp)))
    s.set_timesteps(8, 3, 2)
    last = s.step_scalars(0, 1.0)                 # prev_t < 0: the kept region comes out as the original, exactly
    assert last["sqrt_alpha_prev"] == 1.0 and last["sqrt_beta_prev"] == 0.0 and last["dir_coef"] == 0.0


def test_config_round_trip_and_refusals(lib_built, tmp_path):
    s = d.RePaintScheduler(eta=0.25, clip_sample=False, beta_end=0.03)
    assert s.config.num_train_timesteps == 1000 and s.config.beta_schedule == "linear" and s.eta == 0.25
    s.save_pretrained(str(tmp_path))
    cfg = json.load(open(os.path.join(str(tmp_path), "scheduler_config.json")))
    assert cfg["_class_name"] == "RePaintScheduler" and cfg["eta"] == 0.25 and cfg["clip_sample"] is False
    r = d.RePaintScheduler.from_pretrained(str(tmp_path))
    assert r.config.to_dict() == s.config.to_dict() and torch.equal(r.betas, s.betas)
    assert d.RePaintScheduler.from_config(s.config).config.to_dict() == s.config.to_dict()
    assert d.RePaintScheduler().config.to_dict() == dict(
        num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", eta=0.0, trained_betas=None,
        clip_sample=True)
    with pytest.raises(NotImplementedError, match="beta_schedule"):
        d.RePaintScheduler(beta_schedule="squaredcos_cap_v2")
    with pytest.raises(NotImplementedError, match="trained_betas"):
        d.RePaintScheduler(trained_betas=[0.1, 0.2])
    with pytest.raises(TypeError, match="unexpected"):
        d.RePaintScheduler(prediction_type="epsilon")
    with pytest.raises(ValueError):
        d.RePaintScheduler().set_timesteps(10, jump_length=0)


def test_cpu_tensors_are_refused(lib_built):
    s = d.RePaintScheduler()
    s.set_timesteps(8, 3, 2)
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="HIP engine"):
        s.step(x, 875, x, x, x)
    with pytest.raises(RuntimeError, match="HIP engine"):
        s.undo_step(x, 375)


def test_pipeline_adopts_a_ddpm_folder(lib_built, tmp_path):
    unet = d.UNet2DModel(**CFG1)
    d.DDPMPipeline(unet, d.DDPMScheduler(beta_end=0.03)).save_pretrained(str(tmp_path / "ddpm"))
    p = d.RePaintPipeline.from_pretrained(str(tmp_path / "ddpm"))
    assert isinstance(p.scheduler, d.RePaintScheduler) and p.scheduler.config.beta_end == 0.03
    assert p.scheduler.config.eta == 0.0 and p.unet.config.in_channels == 3
    p.save_pretrained(str(tmp_path / "rp"))
    index = json.load(open(str(tmp_path / "rp" / "model_index.json")))
    assert index["_class_name"] == "RePaintPipeline" and index["scheduler"] == ["diffusers", "RePaintScheduler"]
    q = d.RePaintPipeline.from_pretrained(str(tmp_path / "rp"))
    assert isinstance(q.scheduler, d.RePaintScheduler) and q.scheduler.config.beta_end == 0.03
    # the sibling pipelines read the folder back too (the base class's name table knows the new scheduler)
    assert isinstance(d.DDIMPipeline.from_pretrained(str(tmp_path / "rp")).scheduler, d.DDIMScheduler)


def _args(**kw):
    base = dict(sample=16, eps=16, original=16, mask=16, noise=None, prev=16, noise_out=None, n=2, c=3, h=4, w=4,
                original_n=1, mask_n=1, mask_c=1, add_std=0, sqrt_beta_prod_t=0.5, sqrt_alpha_prod_t=0.5, clip=1.0,
                sqrt_alpha_prev=0.5, dir_coef=0.5, std=0.0, sqrt_beta_prev=0.5, seed=0, offset=0)
    base.update(kw)
    return _lib.RepaintStepArgs(**base)


def test_abi_refuses_bad_arguments_before_any_hip_call(lib_built):
    lib = _lib.load()
    assert lib.dsg_repaint_step(None, None) == -1 and b"NULL" in lib.dsg_last_error()
    for kw, word in ((dict(sample=None), b"NULL"), (dict(mask=None), b"NULL"), (dict(prev=None), b"NULL"),
                     (dict(n=0), b"positive"), (dict(h=-1), b"positive"), (dict(original_n=3), b"original_n"),
                     (dict(mask_n=3), b"mask_n"), (dict(mask_c=2), b"mask_c"), (dict(mask_c=0), b"mask_c")):
        a = _args(**kw)
        assert lib.dsg_repaint_step(ctypes.byref(a), None) == -1, kw
        assert word in lib.dsg_last_error(), (kw, lib.dsg_last_error())
    assert lib.dsg_repaint_undo(None, None, 16, 4, 1.0, 0.0, 0, 0, None) == -1 and b"NULL" in lib.dsg_last_error()
    assert lib.dsg_repaint_undo(16, None, None, 4, 1.0, 0.0, 0, 0, None) == -1
    assert lib.dsg_repaint_undo(16, None, 16, 0, 1.0, 0.0, 0, 0, None) == -1 and b"positive" in lib.dsg_last_error()


def test_pipeline_refuses_wrong_inputs_before_any_kernel(lib_built):
    """Shape / channel mismatches and a mask of the wrong extent raise ValueError -- on a CPU-resident pipeline, i.e. before
    the device check and before anything could be launched."""
    from PIL import Image
    p = d.RePaintPipeline(d.UNet2DModel(**CFG1), d.RePaintScheduler())      # 3 x 64 x 64
    img, m = torch.zeros(1, 3, 64, 64), torch.ones(1, 1, 64, 64)
    bad = [(torch.zeros(1, 4, 64, 64), m), (torch.zeros(1, 3, 32, 64), m), (torch.zeros(3, 64), m),
           (np.zeros((1, 64, 64, 4), np.uint8), m), (Image.new("RGBA", (64, 64)), m), (Image.new("RGB", (32, 32)), m),
           (img, torch.ones(1, 1, 32, 64)), (img, torch.ones(1, 2, 64, 64)), (img, torch.ones(2, 1, 64, 64)),
           (torch.zeros(2, 3, 64, 64), torch.ones(3, 1, 64, 64)), (img, Image.new("L", (32, 32))),
           (img, np.ones((1, 1, 64, 64), np.int32))]
    for image, mask in bad:
        with pytest.raises(ValueError):
            p(image, mask, num_inference_steps=4)
    with pytest.raises(ValueError, match="batch_size"):
        p(torch.zeros(2, 3, 64, 64), m, batch_size=3)
    with pytest.raises(ValueError, match="seed"):
        p(img, m, noise="device")
    with pytest.raises(ValueError, match="noise"):
        p(img, m, noise="philox")
    with pytest.raises(TypeError):
        p(img, m, shard=(0, 2))                  # sample sharding is not part of this pipeline
    # well-formed inputs get as far as the device check
    for image, mask in ((img, m), (Image.new("RGB", (64, 64)), Image.new("L", (64, 64), 255)),
                        (np.zeros((64, 64, 3), np.uint8), np.ones((64, 64), bool)), (img, torch.ones(1, 3, 64, 64))):
        with pytest.raises(RuntimeError, match="HIP engine"):
            p(image, mask, num_inference_steps=4)


def test_input_mapping(lib_built):
    from drivescenegen_amd.pipelines import _as_binary_mask, _as_model_domain
    u8 = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4) * 10
    x = _as_model_domain(u8)
    assert x.shape == (1, 4, 2, 3) and x.dtype == torch.float32
    assert np.array_equal(x[0].numpy(), (u8.astype(np.float32) / np.float32(255) * np.float32(2) - np.float32(1)).transpose(2, 0, 1))
    f = torch.randn(2, 3, 4, 4)
    assert torch.equal(_as_model_domain(f), f) and _as_model_domain(f[0]).shape == (1, 3, 4, 4)
    m = _as_binary_mask(np.array([[0.0, 0.49, 0.5, 1.0]], np.float32))
    assert m.shape == (1, 1, 1, 4) and m.flatten().tolist() == [0.0, 0.0, 1.0, 1.0]
    assert _as_binary_mask(np.array([[0, 127, 128, 255]], np.uint8)).flatten().tolist() == [0.0, 0.0, 1.0, 1.0]
    assert _as_binary_mask(torch.tensor([[True, False]])).flatten().tolist() == [1.0, 0.0]


def test_oracle_loop_draw_order_and_invariants():
    """The restatement on its own: a network that returns zeros, (8,3,2): 14 step entries + 6 undo entries of 125 passes, so the
    generator is drawn from 1 + 14 + 6*125 times; the kept region of the result is the original exactly."""
    shape = (1, 2, 4, 4)
    orig = np.linspace(-1, 1, 32, dtype=np.float32).reshape(shape)
    mask = np.zeros(shape, np.float32)
    mask[:, :, :, :2] = 1
    g = torch.Generator().manual_seed(3)
    x, rec = ro.run(lambda x, t: np.zeros_like(x), orig, mask, shape, 8, 3, 2, 1.0, g)
    assert [r["kind"] for r in rec].count("step") == 14 and len(rec) == 20
    g2 = torch.Generator().manual_seed(3)
    for _ in range(1 + 14 + 6 * 125):
        torch.randn(shape, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())
    assert np.array_equal(x[mask == 1], orig[mask == 1]) and np.isfinite(x).all()
