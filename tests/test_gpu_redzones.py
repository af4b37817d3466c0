"""Every kernel stays inside its buffers: the engine's kernels run with each tensor between poisoned, mapped red zones.

tests/redzone_alloc.cpp (host-only, built here with hipcc) is installed as torch's device allocator in ONE fresh child process,
tests/redzone_child.py, which runs the case table twice -- fill word 0xFFFFFFFF, then 0x5A5A5A5A -- and reports per case:
no red-zone byte changed, no input changed, every result bitwise the same in both passes, and the pass-B result against its
fp64 / oracle reference.  The first two cases plant an overrun of each kind and must see it reported.
If the child dies or times out, every case from the one that was running on fails with its exit status and stderr tail, and
nothing else is started on the GPU."""
import json
import os
import subprocess
import sys

import pytest

from tests.redzone_child import CASE_IDS, SELFTESTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 800


@pytest.fixture(scope="module")
def redzone_report(tmp_path_factory, lib_built):
    work = tmp_path_factory.mktemp("redzones")
    so = str(work / "libredzone.so")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-O2", "-o", so,
                    os.path.join(ROOT, "tests", "redzone_alloc.cpp")], check=True, capture_output=True)
    report = str(work / "report.jsonl")
    status, stderr = None, ""
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "redzone_child.py"), so, report], cwd=ROOT,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        status, stderr = p.returncode, p.stderr + p.stdout[-4000:]
    except subprocess.TimeoutExpired as e:
        status, stderr = f"timed out after {CHILD_TIMEOUT_S} s", ((e.stderr or b"").decode(errors="replace") if isinstance(e.stderr, bytes)
                                                                   else (e.stderr or ""))
    rows = []
    if os.path.exists(report):
        with open(report) as f:
            for ln in f:
                try:
                    rows.append(json.loads(ln))
                except ValueError:
                    pass   # (a line cut by the child's death)
    return {"status": status, "stderr": stderr[-3000:], "rows": rows}


def _fmt(row):
    keep = {k: row.get(k) for k in ("item", "problems", "violations", "ab_diffs") if row.get(k)}
    return json.dumps(keep, indent=1)[:6000]


@pytest.mark.parametrize("case", CASE_IDS)
def test_kernels_stay_inside_their_buffers(redzone_report, case):
    rows = redzone_report["rows"]
    mine = [r for r in rows if r.get("case") == case]
    started = {r["item"] if "item" in r else case for r in mine if r.get("event") == "started"}
    done = [r for r in mine if r.get("event") == "done"]
    finished = any(r.get("event") == "finished" for r in rows)
    if not finished:
        last = [r for r in rows if r.get("event") == "started"]
        running = last[-1].get("item", last[-1].get("case")) if last else None
        ended = {r.get("item", r.get("case")) for r in rows if r.get("event") == "done"}
        if not mine or started - ended:
            pytest.fail(f"red-zone child ended ({redzone_report['status']}) while running {running}; "
                        f"stderr tail:\n{redzone_report['stderr']}")
    assert done, f"no result row for {case} (child status {redzone_report['status']})"
    bad = [r for r in done if not r.get("ok")]
    assert not bad, "\n".join(_fmt(r) for r in bad[:4])
    if case in SELFTESTS:
        assert len(done) == 1 and not done[0].get("problems")
