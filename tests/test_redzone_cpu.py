"""The red-zone allocator of tests/test_gpu_redzones.py without a GPU: it builds with hipcc, and its layout arithmetic
(rz_layout, the function every allocation goes through) is the one tests/redzone_alloc.cpp documents."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 1 << 20


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("hipcc"):
        pytest.fail("hipcc not on PATH (the library's own build needs it too)")
    so = str(tmp_path_factory.mktemp("rz") / "libredzone.so")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-O2", "-o", so,
                    os.path.join(ROOT, "tests", "redzone_alloc.cpp")], check=True, capture_output=True)
    lib = C.CDLL(so)
    lib.rz_layout.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.rz_layout.restype = None
    return lib


def _layout(lib, size, guard=0):
    out = (C.c_size_t * 5)()
    lib.rz_layout(size, guard, out)
    return dict(zip(("user", "slack", "tail", "tail_len", "total"), out))


@pytest.mark.parametrize("size", [1, 255, 256, 257, 2 ** 31 + 3])
def test_layout_matches_the_spec(shim, size):
    lay = _layout(shim, size)
    rounded = (size + 255) // 256 * 256
    assert lay["user"] == G and lay["user"] % 256 == 0          # head zone of G bytes; the user region is 256-byte aligned
    assert lay["slack"] == rounded - size and 0 <= lay["slack"] < 256
    assert lay["tail"] == lay["user"] + size                     # the checked tail starts at the user's last byte + 1 ...
    assert lay["tail_len"] == lay["slack"] + G                   # ... and covers the slack and a full G-byte zone
    assert lay["total"] == 2 * G + rounded == lay["tail"] + lay["tail_len"]


def test_layout_takes_another_guard(shim):
    lay = _layout(shim, 1000, guard=4096)
    assert (lay["user"], lay["slack"], lay["tail"], lay["tail_len"], lay["total"]) == (4096, 24, 5096, 4120, 9216)


def test_shim_exports_the_allocator_interface(shim):
    for name in ("rz_alloc", "rz_free", "rz_set_word", "rz_check_live", "rz_violations", "rz_serial", "rz_fill_zones"):
        assert hasattr(shim, name), name


def test_case_table_is_static_and_unique():
    from tests.redzone_child import CASE_IDS, SELFTESTS
    assert list(CASE_IDS[:2]) == list(SELFTESTS)
    assert len(CASE_IDS) == len(set(CASE_IDS)) and len(CASE_IDS) > 100
