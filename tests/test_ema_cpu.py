"""EMAModel's host side and the dsg_ema_* ABI, checked without a GPU: the decay schedule against a restatement of diffusers
0.20.0's expressions (exact, Python doubles), the chunk rule of include/dsg.h, argument validation before any HIP call, and
the loud refusal of CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bare_ema(**kw):
    """An EMAModel without a device buffer: get_decay reads the hyper-parameters only."""
    from drivescenegen_amd import EMAModel
    e = EMAModel.__new__(EMAModel)
    hp = dict(decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3)
    hp.update(kw)
    for k, v in hp.items():
        setattr(e, k, v)
    return e


def _decay_restated(t, decay, min_decay, update_after_step, use_ema_warmup, inv_gamma, power):
    step = t - update_after_step - 1
    if step <= 0:
        return 0.0
    value = 1 - (1 + step / inv_gamma) ** -power if use_ema_warmup else (1 + step) / (10 + step)
    return max(min(value, decay), min_decay)


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("after", [0, 5])
def test_get_decay_is_diffusers_schedule_exactly(lib_built, warmup, after):
    cases = [dict(), dict(decay=0.5), dict(min_decay=0.6), dict(decay=0.95, min_decay=0.2, inv_gamma=2.0, power=0.75)]
    clamped_hi = clamped_lo = free = 0
    for hp in cases:
        hp = dict(dict(decay=0.9999, min_decay=0.0, inv_gamma=1.0, power=2 / 3), **hp)
        e = _bare_ema(update_after_step=after, use_ema_warmup=warmup, **hp)
        for t in list(range(0, 51)) + [10 ** 6]:
            got = e.get_decay(t)
            want = _decay_restated(t, hp["decay"], hp["min_decay"], after, warmup, hp["inv_gamma"], hp["power"])
            assert isinstance(got, float) and got == want, (hp, t, got, want)
            if t <= after + 1:
                assert got == 0.0                   # (diffusers returns before the clamps: min_decay does not apply yet)
            else:
                clamped_hi += got == hp["decay"]
                clamped_lo += got == hp["min_decay"] and hp["min_decay"] > 0
                free += hp["min_decay"] < got < hp["decay"]
    assert clamped_hi and clamped_lo and free       # both clamps and the unclamped range were exercised
    assert _bare_ema().get_decay(10 ** 6) == 0.9999 and _bare_ema().get_decay(2) == 2 / 11


def test_chunk_rule_and_running_sum(lib_built):
    from drivescenegen_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "dsg.h")).read()
    chunk = int(re.search(r"#define\s+DSG_EMA_CHUNK\s+(\d+)", hdr).group(1))
    assert "chunks = ceil(numel / DSG_EMA_CHUNK)" in hdr
    assert chunk % 1024 == 0     # 256 lanes x 16 bytes: a chunk start keeps the job's 16-byte alignment
    assert ctypes.sizeof(_lib.EmaJob) == 32
    sizes = [1, 3, 4, 5, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 7, 56_600_000, 2 ** 33 + 1]
    first = [0]
    for n in sizes:
        job = _lib.EmaJob(param=4096, shadow=8192, numel=n, copy_only=0)
        out = ctypes.c_int64(-1)
        assert lib.dsg_ema_job_chunks(ctypes.byref(job), ctypes.byref(out)) == 0
        assert out.value == -(-n // chunk), (n, out.value)
        first.append(first[-1] + out.value)
    assert first[-1] == sum(-(-n // chunk) for n in sizes) and all(b > a for a, b in zip(first, first[1:]))
    # the Python wrapper builds the same table (host side only here: an empty table needs no device)
    from drivescenegen_amd import ops
    t = ops.EmaTable([], "cpu")
    assert t.n == 0 and t.total == 0
    t.run(0.5)                   # njobs == 0: nothing to launch
    for bad in (dict(numel=0), dict(numel=-4), dict(param=None), dict(shadow=None), dict(param=4098)):
        job = _lib.EmaJob(**dict(dict(param=4096, shadow=8192, numel=8, copy_only=0), **bad))
        assert lib.dsg_ema_job_chunks(ctypes.byref(job), ctypes.byref(out)) == -1, bad
    assert lib.dsg_ema_job_chunks(None, ctypes.byref(out)) == -1 and b"NULL" in lib.dsg_last_error()


def test_error_path_without_gpu(lib_built):
    """Argument validation happens before any HIP call, so it is checkable on a CPU-only host."""
    from drivescenegen_amd import _lib
    lib = _lib.load()
    assert lib.dsg_ema_step(None, None, 0, 0, 0.5, None) == 0            # njobs == 0 is OK and launches nothing
    rc = lib.dsg_ema_step(None, None, 1, 1, 0.5, None)
    assert rc == -1 and b"NULL" in lib.dsg_last_error()
    rc = lib.dsg_ema_step(4096, 8192, -1, 1, 0.5, None)
    assert rc == -1 and b"njobs" in lib.dsg_last_error()
    rc = lib.dsg_ema_step(4096, 8192, 2, 1, 0.5, None)                   # fewer chunks than jobs
    assert rc == -1 and b"total_chunks" in lib.dsg_last_error()
    for omd in (-0.1, 1.5, float("nan")):
        rc = lib.dsg_ema_step(4096, 8192, 1, 1, omd, None)
        assert rc == -1 and b"one_minus_decay" in lib.dsg_last_error(), omd


def test_cpu_parameters_other_dtypes_and_modules_are_refused_loudly(lib_built):
    import drivescenegen_amd as d
    from drivescenegen_amd import ops
    lin = torch.nn.Linear(4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.EMAModel(lin.parameters())
    with pytest.raises(TypeError, match="parameters"):
        d.EMAModel(lin)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ema_step_([torch.zeros(8)], [torch.zeros(8)], 0.5)
    with pytest.raises(RuntimeError, match="fp32"):
        d.EMAModel([torch.zeros(8, dtype=torch.float16)])
    for kw in ("max_value", "min_value", "device", "foreach"):
        with pytest.raises(TypeError):
            d.EMAModel(lin.parameters(), **{kw: 1})
    e = _bare_ema()
    e.temp_stored_params = None
    with pytest.raises(RuntimeError, match="store"):
        e.restore(lin.parameters())
