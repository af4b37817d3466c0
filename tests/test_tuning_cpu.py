"""The kernel-selection switches are ONE table (csrc/tuning.h): the list in include/dsg.h, dsg_set_tuning / dsg_get_tuning /
dsg_tuning_key and the values each key accepts are held against each other here.  No GPU needed: the entry points are host code."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = range(64)
VALUES = (-1, 0, 1, 2, 3, 4, 5, 8, 16, 512, 1000)

# (key, value) pairs dsg_set_tuning accepted, for KEYS x VALUES, RECORDED from the library before the switches became a table
# (the if-chain in conv.hip, built and called under DSG_TESTING=1): the table must accept exactly these.
_ONOFF = (0, 1)
ACCEPTED = {1: (0, 4, 8), 2: _ONOFF, 3: (0, 2, 3, 4), 5: _ONOFF, 6: (4, 8), 7: _ONOFF, 8: _ONOFF, 10: _ONOFF, 11: _ONOFF,
            13: _ONOFF, 14: _ONOFF, 15: _ONOFF, 16: (0, 1, 2, 3, 4, 5, 8, 16, 512, 1000), 17: _ONOFF, 18: _ONOFF, 19: _ONOFF,
            20: _ONOFF, 21: _ONOFF, 22: _ONOFF, 23: _ONOFF, 25: _ONOFF, 26: _ONOFF, 27: (1, 2, 3, 4, 5, 8, 16, 512, 1000),
            29: _ONOFF, 30: _ONOFF, 31: _ONOFF, 32: _ONOFF, 34: _ONOFF, 36: _ONOFF, 37: (0, 1, 2, 3), 38: _ONOFF, 39: _ONOFF,
            40: _ONOFF, 41: _ONOFF}


def _documented():
    """{key: default} from the comment above dsg_set_tuning: a paragraph starts ' *  NN  ', its default is the first '[number' that
    is not an index (configs[3])."""
    txt = open(os.path.join(ROOT, "include", "dsg.h")).read()
    body = txt[txt.index("Kernel-selection switches for A/B measurements"):txt.index("int dsg_set_tuning(")]
    doc = {}
    for par in re.split(r"\n \*\s{1,3}(?=\d{1,2}  \S)", body)[1:]:
        key = int(par.split()[0])
        assert key not in doc, f"key {key} is listed twice"
        doc[key] = int(re.search(r"(?<!\w)\[(-?\d+)\b", par).group(1))
    assert list(doc) == sorted(doc), "the header lists the keys in order"
    return doc


def _field_names():
    src = open(os.path.join(ROOT, "drivescenegen_amd", "csrc", "tuning.h")).read()
    return {int(k): name for k, name in re.findall(r"^\s*X\((\d+), (\w+),", src, re.M)}


def _get(lib, key):
    v = C.c_int32(-12345)
    return v.value if lib.dsg_get_tuning(key, C.byref(v)) == 0 else None


def _fresh_process(lib_path, code, **env_extra):
    """Run `code` (which prints one JSON value) against the library in a process without DSG_TESTING / DSG_TUNING."""
    env = {k: v for k, v in os.environ.items() if k not in ("DSG_TESTING", "DSG_TUNING")}
    env.update(env_extra)
    pre = ("import ctypes as C, json, sys\nlib = C.CDLL(sys.argv[1])\nlib.dsg_last_error.restype = C.c_char_p\n"
           "def get(k):\n    v = C.c_int32(-12345)\n    return v.value if lib.dsg_get_tuning(k, C.byref(v)) == 0 else None\n")
    out = subprocess.run([sys.executable, "-c", pre + code, lib_path], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def test_header_lists_the_keys_and_defaults_the_library_has(lib_built):
    got = _fresh_process(lib_built, "print(json.dumps({k: get(k) for k in range(64) if get(k) is not None}))")
    have = {int(k): v for k, v in got.items()}
    doc = _documented()
    assert sorted(doc) == sorted(have), (sorted(set(doc) - set(have)), sorted(set(have) - set(doc)))
    assert doc == have, {k: (doc[k], have[k]) for k in doc if doc[k] != have[k]}
    assert sorted(have) == sorted(ACCEPTED)


def test_every_switch_round_trips_and_moves_the_epoch(lib_built):
    lib = C.CDLL(lib_built)
    assert os.environ.get("DSG_TESTING") == "1"
    names = _field_names()
    assert sorted(names) == sorted(ACCEPTED)
    for key in KEYS:
        before, e0 = _get(lib, key), lib.dsg_tuning_epoch()
        if key not in ACCEPTED:
            assert before is None and lib.dsg_set_tuning(key, 1) != 0 and lib.dsg_tuning_epoch() == e0, key
            continue
        assert lib.dsg_set_tuning(key, before) == 0, key
        assert _get(lib, key) == before and lib.dsg_tuning_epoch() > e0, key
        e1 = lib.dsg_tuning_epoch()
        refused = next(v for v in VALUES if v not in ACCEPTED[key])
        assert lib.dsg_set_tuning(key, refused) != 0 and lib.dsg_tuning_epoch() == e1 and _get(lib, key) == before, key
        k = C.c_int32(-1)
        assert lib.dsg_tuning_key(names[key].encode(), C.byref(k)) == 0 and k.value == key, names[key]
    k = C.c_int32(-1)
    assert lib.dsg_tuning_key(b"no_such_switch", C.byref(k)) != 0 and k.value == -1


def test_accepted_values_are_those_of_the_if_chain(lib_built):
    lib = C.CDLL(lib_built)
    saved = {k: _get(lib, k) for k in ACCEPTED}
    try:
        got = {(k, v) for k in KEYS for v in VALUES if lib.dsg_set_tuning(k, v) == 0}
    finally:
        for k, v in saved.items():
            assert lib.dsg_set_tuning(k, v) == 0
    want = {(k, v) for k, vs in ACCEPTED.items() for v in vs}
    assert got == want, (sorted(got - want), sorted(want - got))


def test_without_dsg_testing_set_is_refused_and_the_readers_answer(lib_built):
    code = ("k = C.c_int32(-1)\nrc_key = lib.dsg_tuning_key(b'splitk', C.byref(k))\nbefore = get(k.value)\n"
            "rc = lib.dsg_set_tuning(k.value, 0)\nmsg = lib.dsg_last_error().decode()\n"
            "print(json.dumps([rc_key, k.value, before, rc, msg, get(k.value), lib.dsg_tuning_epoch()]))")
    rc_key, key, before, rc, msg, after, epoch = _fresh_process(lib_built, code)
    assert rc_key == 0 and key == 19 and before == 1
    assert rc == -1 and "DSG_TESTING" in msg
    assert after == 1 and epoch == 0
