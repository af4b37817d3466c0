"""Red-zone runner: every kernel of the engine with its buffers between poisoned, mapped red zones.

    python tests/redzone_child.py LIBREDZONE_SO REPORT_JSONL

A fresh process (tests/test_gpu_redzones.py starts it once).  Before the first CUDA allocation it routes torch's device
allocator through tests/redzone_alloc.cpp, so every tensor the tests, the wrappers, the tape and the whole-network plan's
workspace allocate is its own hipMalloc between two 1 MiB zones, and starts filled with the current fill word.
Every case runs twice, with the word 0xFFFFFFFF (NaN / -1) and then 0x5A5A5A5A (finite in fp32, bf16, fp16):
  (a) after synchronize + gc, no zone of a live or freed allocation differs from the word it was filled with;
  (b) no input of a wrapper call (drivescenegen_amd.ops / imageops / rasterization) changed, except its result arguments;
  (c) every result is bitwise the same in both passes (the engine has no float atomics and a fixed split-K order, so a
      difference means a result depends on memory no kernel wrote);
  (d) in pass B the result matches the fp64 / oracle reference: the op-level cases are the existing GPU tests (their
      own references and tolerances), run under this process's pytest with a recorder around the wrappers.
One JSON line per case and pass-pair, flushed: `started` before the first launch, then `done`.  Never retries.
"""
import ast
import ctypes as C
import gc
import hashlib
import json
import os
import random
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = (0xFFFFFFFF, 0x5A5A5A5A)

SELFTESTS = ("selftest::write_past_output", "selftest::read_past_inputs")

# the op-level GPU test modules run under the recorder: file -> test functions left out (and why)
STEP = "a whole training step: the train_step:: cases run those geometries without the per-call recorder"
SUITE = {
    "test_gpu_ops.py": {"test_errors_are_reported_not_fatal": "provokes argument errors on purpose; no kernel result"},
    "test_gpu_train_ops.py": {},
    "test_gpu_gnb.py": {"test_training_step_gradients_with_and_without_the_epilogue_statistics": STEP,
                        "test_query_and_dispatch_agree_over_a_shape_sweep": "dispatch queries; the launches are the other gnb cases'"},
    "test_gpu_ups_dgrad.py": {},
    "test_gpu_fused_shortcut.py": {},
    "test_gpu_operand.py": {},
    "test_gpu_mixed.py": {},
    "test_gpu_mixed_train.py": {"test_upsampler_data_gradient_routes_agree": STEP, "test_training_step_mixed_vs_fp32_oracle": STEP,
                                "test_fp16_grad_scaler_skips_a_non_finite_step_and_recovers": STEP,
                                "test_bf16_accelerator_needs_no_scaler_and_accumulates": STEP,
                                "test_folded_upsampler_weight_gradient_in_a_whole_step": STEP,
                                "test_fp32_tape_keeps_precision_when_dy_is_tiny": STEP},
    "test_gpu_rows_f.py": {"test_f3_training_resume": STEP},
    "test_gpu_rows_f4.py": {},
    "test_gpu_philox.py": {"test_train_steps_with_device_noise_is_reproducible_and_rank_disjoint": STEP},
    "test_gpu_pack_batch.py": {"test_training_with_batched_refresh_is_bitwise_the_one_by_one_run": STEP},
    "test_gpu_conv_in.py": {},
    "test_gpu_conv_out.py": {},
    "test_gpu_range_guard.py": {},
    "test_gpu_stream_edges.py": {},
    "test_gpu_train_step.py": {},   # (its two steps are checked against the fp64 oracle: check (d) of a whole step)
}

# whole-network forwards: (config, batch, compute dtype, DSG_UNET_BATCH_INVARIANT)
NET_CFGS = ("CFG1", "CFG2", "CFG4_SMALL", "CFG4", "CFG5", "DEFAULT3")
UNET_FWD = tuple((c, b, dt, False) for c in NET_CFGS for b in (1, 2, 5) for dt in ("fp32", "bf16")) + \
    tuple((c, 2, dt, True) for c in NET_CFGS for dt in ("fp32", "bf16"))
# training steps (forward, backward, clip, AdamW): (config, batch, tape dtype); the last two are the drivers' operating points
TRAIN = (("CFG1", 2, "fp32"), ("CFG4_SMALL", 2, "fp32"), ("CFG3", 2, "fp32"),
         ("CFG1", 2, "bf16"), ("CFG4_SMALL", 2, "bf16"), ("CFG3", 2, "bf16"), ("CFG5", 2, "bf16"),
         ("DEFAULT3", 2, "fp16"), ("CFG5", 128, "bf16"), ("CFG3", 64, "fp32"))
# the wrapper arguments a call may write (everything else is an input and must come back bitwise unchanged)
RESULT_ARGS = {"out", "dw", "dst", "stats_buf", "dgamma", "dbeta", "dy_sums", "bias_grad", "db", "found_inf", "g", "param",
               "exp_avg", "exp_avg_sq"}


def _suite_funcs(fname):
    """the file's GPU test functions (module-wide `pytestmark = pytest.mark.gpu`, or their own mark) minus the left-out ones"""
    tree = ast.parse(open(os.path.join(ROOT, "tests", fname)).read())
    all_gpu = any(isinstance(n, ast.Assign) and any(getattr(t, "id", "") == "pytestmark" for t in n.targets)
                  and "mark.gpu" in ast.unparse(n.value) for n in tree.body)
    return [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")
            and n.name not in SUITE[fname] and (all_gpu or any("mark.gpu" in ast.unparse(dec) for dec in n.decorator_list))]


def _stem(fname):
    return fname[len("test_gpu_"):-3]


def unet_id(c, b, dt, bi):
    return f"unet_fwd::{c.lower()}_b{b}_{dt}" + ("_batch_invariant" if bi else "")


def train_id(c, b, dt):
    return f"train::{c.lower()}_b{b}_{dt}"


CASE_IDS = list(SELFTESTS) + [f"{_stem(f)}::{fn}" for f in SUITE for fn in _suite_funcs(f)] + \
    [unet_id(*k) for k in UNET_FWD] + [train_id(*k) for k in TRAIN]


# ---------------------------------------------------------------------------------------------------------------------
class Runner:
    def __init__(self, so, report):
        import torch
        self.torch = torch
        alloc = torch.cuda.memory.CUDAPluggableAllocator(so, "rz_alloc", "rz_free")
        torch.cuda.memory.change_current_allocator(alloc)
        self.rz = C.CDLL(so)
        self.rz.rz_set_word.argtypes = [C.c_uint32]
        self.rz.rz_violations.argtypes = [C.c_char_p, C.c_int64]
        self.rz.rz_violations.restype = C.c_int64
        self.rz.rz_violation_count.restype = C.c_int64
        self.rz.rz_serial_of.argtypes = [C.c_void_p]
        self.rz.rz_serial_of.restype = C.c_uint64
        self.rz.rz_fill_zones.argtypes = [C.c_void_p, C.c_uint32]
        self.out = open(report, "a")
        self.rec = None       # the wrapper recorder of the running pass (suite cases)
        self.depth = 0

    def emit(self, **row):
        self.out.write(json.dumps(row) + "\n")
        self.out.flush()

    def violations(self, since):
        n = self.rz.rz_violations(None, 0)
        buf = C.create_string_buffer(int(n))
        self.rz.rz_violations(buf, n)
        return json.loads(buf.value.decode())[since:]

    def settle(self):
        torch = self.torch
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.synchronize()
        self.rz.rz_check_live()
        err = self.rz.rz_last_error()
        return err

    # -- bytes and comparisons --------------------------------------------------------------------------------------
    def raw(self, t):
        return t.detach().cpu().contiguous().reshape(-1).view(self.torch.uint8).clone()

    @staticmethod
    def digest(b):
        return hashlib.blake2b(b.numpy().tobytes(), digest_size=16).hexdigest()

    def ab_diff(self, a, b):
        """(differing bytes, of which never written in either pass: 0xFF in pass A and 0x5A in pass B)"""
        torch = self.torch
        if a.numel() != b.numel():
            return max(a.numel(), b.numel()), 0
        ne = a != b
        n = int(ne.sum())
        if not n:
            return 0, 0
        unw = int((ne & (a == 0xFF) & (b == 0x5A)).sum())
        first = int(torch.nonzero(ne)[0])
        return n, unw, first

    # -- one case, two passes ---------------------------------------------------------------------------------------
    def two_passes(self, fn):
        """fn() -> dict name -> tensor of results.  Returns (per-pass results, per-pass violations, per-pass errors)."""
        torch = self.torch
        res, viol, errs = [], [], []
        for word in WORDS:
            self.rz.rz_set_word(word)
            v0 = self.rz.rz_violation_count()
            random.seed(0)
            torch.manual_seed(0)
            err, got = None, {}
            try:
                got = {k: self.raw(v) for k, v in (fn(word) or {}).items()}
            except Exception as e:   # noqa: BLE001 -- recorded, the run goes on
                err = f"{type(e).__name__}: {e}"[:1500] + "\n" + traceback.format_exc()[-1500:]
            herr = self.settle()
            if herr:
                err = (err or "") + f" [allocator met HIP error {herr}]"
            res.append(got)
            viol.append(self.violations(v0))
            errs.append(err)
        return res, viol, errs

    def compare(self, res):
        diffs = []
        for k in res[0]:
            if k not in res[1]:
                continue
            d = self.ab_diff(res[0][k], res[1][k])
            if d[0]:
                diffs.append({"result": k, "bytes_differ": d[0], "never_written": d[1], "first_byte": d[2] if len(d) > 2 else None,
                              "bytes": int(res[0][k].numel())})
        return diffs

    # -- self-test: the harness must report planted faults ----------------------------------------------------------
    def selftest(self, which):
        torch = self.torch
        from drivescenegen_amd import _lib
        lib = _lib.load()
        n = 1 << 18   # floats: 1 MiB, a multiple of 64 -> no tail slack
        serial = {}   # fill word -> serial of the output allocation

        def run(word):
            if which == "write":
                a = torch.ones(n + 4, device="cuda")
                b = torch.ones(n + 4, device="cuda")
                out = torch.empty(n, device="cuda")
                serial[word] = self.rz.rz_serial_of(out.data_ptr())
                # numel n + 4 into an n-float output: the last 16 bytes land at offset 0 of its tail zone
                _lib.check(lib.dsg_add(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n + 4, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(_lib.stream_ptr())))
                torch.cuda.synchronize()
                return {"out": out}
            a = torch.ones(n, device="cuda")
            b = torch.ones(n, device="cuda")
            out = torch.empty(n + 4, device="cuda")
            # numel n + 4 over n-float inputs: 16 bytes of each input's tail zone are read
            _lib.check(lib.dsg_add(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n + 4, C.c_void_p(out.data_ptr()),
                                   C.c_void_p(_lib.stream_ptr())))
            torch.cuda.synchronize()
            return {"out": out}

        res, viol, errs = self.two_passes(run)
        diffs = self.compare(res)
        problems = [f"pass {p}: {e}" for p, e in zip("AB", errs) if e]
        if which == "write":
            for p, word, v in zip("AB", WORDS, viol):
                want = [x for x in v if x["serial"] == serial.get(word) and x["side"] == "tail" and x["offset"] == 0 and x["nbad"] <= 16]
                if len(v) != 1 or len(want) != 1:
                    problems.append(f"pass {p}: expected exactly one tail violation at offset 0 of the output's zone, got {v}")
        else:
            if any(viol):
                problems.append(f"expected no zone violation, got {viol}")
            if res[0] and res[1]:
                a = res[0]["out"].view(torch.int32)
                b = res[1]["out"].view(torch.int32)
                idx = torch.nonzero(a != b).flatten().tolist()
                if idx != [n, n + 1, n + 2, n + 3]:
                    problems.append(f"expected a pass A/B difference in exactly the last 4 values ({n}..{n + 3}), got {idx[:16]}")
        return {"ok": not problems, "problems": problems, "violations": viol, "ab_diffs": diffs}

    # -- whole-network forward / training step -----------------------------------------------------------------------
    def unet_forward(self, cfg_name, batch, dtype, bi):
        torch = self.torch
        import drivescenegen_amd as d
        from drivescenegen_amd import configs
        cfg = getattr(configs, cfg_name)
        x0 = configs.noisy_inputs(cfg, batch)
        ts = [980, 500, 20, 3, 750][:batch]
        keep = {}

        def run(word):
            net = configs.synth_weights(d.UNet2DModel(**cfg)).to("cuda").eval().requires_grad_(False).set_compute_dtype(dtype)
            net.batch_invariant = bi
            x = x0.to("cuda")
            t = torch.tensor(ts, device="cuda")
            before = (self.raw(x), self.raw(t))
            y = net(x, t).sample
            torch.cuda.synchronize()
            if not (torch.equal(before[0], self.raw(x)) and torch.equal(before[1], self.raw(t))):
                keep.setdefault("inputs_changed", []).append(hex(word))
            keep["y"] = y.detach().cpu()
            return {"sample": y}

        res, viol, errs = self.two_passes(run)
        problems = [f"pass {p}: {e}" for p, e in zip("AB", errs) if e]
        if "inputs_changed" in keep:
            problems.append(f"the forward changed its inputs (passes {keep['inputs_changed']})")
        if not problems and "y" in keep:
            y = keep["y"]
            if not torch.isfinite(y).all():
                problems.append("non-finite output")
            elif cfg_name in ("CFG1", "CFG4_SMALL"):   # the oracle at the small configs, with the tolerances of
                from oracle.unet_oracle import OracleUNet2DModel   # tests/test_gpu_unet.py (fp32) / test_gpu_mixed.py (16-bit)
                from tests.common import rel_l2
                from tests.test_gpu_unet import _assert_close
                ora = configs.synth_weights(OracleUNet2DModel(**cfg)).eval()
                with torch.no_grad():
                    want = ora(x0, torch.tensor(ts)).sample
                try:
                    if dtype == "fp32":
                        _assert_close(y, want)
                    else:
                        assert rel_l2(y, want) <= 2e-2, rel_l2(y, want)
                except AssertionError as e:
                    problems.append(f"pass B against the oracle: {e}")
        return self.verdict(res, viol, problems)

    def train_step(self, cfg_name, batch, dtype):
        torch = self.torch
        import drivescenegen_amd as d
        from drivescenegen_amd import configs, synth
        cfg = getattr(configs, cfg_name)
        ss = cfg["sample_size"]
        h, w = (ss, ss) if isinstance(ss, int) else ss
        c = cfg["in_channels"]
        x0c = torch.from_numpy(synth.synth_scene_rasters(batch, c, h, w, 1))
        noisec = torch.from_numpy(synth.normal(2, (batch, c, h, w)))
        tc = torch.tensor([3, 250, 600, 999] * ((batch + 3) // 4))[:batch]
        finite = {}

        def run(word):
            net = configs.synth_weights(d.UNet2DModel(**cfg)).to("cuda").train().set_compute_dtype(dtype)
            opt = d.AdamW(net.parameters(), lr=1e-4)
            sch = d.DDPMScheduler()
            x0, noise, t = x0c.to("cuda"), noisec.to("cuda"), tc.to("cuda")
            loss = d.mse_loss(net(sch.add_noise(x0, noise, t), t, return_dict=False)[0], noise)
            loss.backward()
            out = {"loss": loss.detach().reshape(1)}
            grads = [p.grad.detach().reshape(-1) for p in net.parameters() if p.grad is not None]
            out["grads"] = torch.cat(grads)
            d.clip_grad_norm_(net.parameters(), 1.0)
            opt.step()
            out["params"] = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
            finite[hex(word)] = bool(torch.isfinite(out["loss"]).all()) and bool(torch.isfinite(out["grads"]).all())
            return out

        res, viol, errs = self.two_passes(run)
        problems = [f"pass {p}: {e}" for p, e in zip("AB", errs) if e]
        if not all(finite.values()) or len(finite) != 2:
            problems.append(f"loss / gradients not finite: {finite}")
        return self.verdict(res, viol, problems)

    def verdict(self, res, viol, problems, extra=None):
        diffs = self.compare(res)
        if any(viol):
            problems.append("zone violations")
        if diffs:
            problems.append("results differ between pass A and pass B")
        row = {"ok": not problems, "problems": problems, "violations": viol, "ab_diffs": diffs}
        row.update(extra or {})
        return row

    # -- the existing op-level tests under a wrapper recorder --------------------------------------------------------
    def install_recorder(self):
        import functools
        import inspect
        torch = self.torch
        from drivescenegen_amd import imageops, ops, rasterization
        runner = self

        def flat(name, v, acc):
            if isinstance(v, torch.Tensor):
                if v.is_cuda:
                    acc.append((name, v))
            elif isinstance(v, dict):
                for k, x in v.items():
                    flat(f"{name}.{k}", x, acc)
            elif isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    flat(f"{name}[{i}]", x, acc)
            return acc

        def wrap(mod, name, f):
            sig = inspect.signature(f)

            @functools.wraps(f)
            def rec(*a, **k):
                if runner.rec is None or runner.depth:
                    return f(*a, **k)
                try:
                    bound = sig.bind(*a, **k)
                except TypeError:
                    return f(*a, **k)
                args = []
                for pn, v in bound.arguments.items():
                    flat(pn, v, args)
                torch.cuda.synchronize()
                pre = [(n, runner.raw(t)) for n, t in args]
                runner.depth += 1
                try:
                    r = f(*a, **k)
                finally:
                    runner.depth -= 1
                torch.cuda.synchronize()
                rets = flat("return", r, [])
                ret_ptrs = {t.untyped_storage().data_ptr() for _, t in rets}
                post = [(n, runner.raw(t)) for n, t in args]
                changed = []
                for (n, b0), (_, b1), (_, t) in zip(pre, post, args):
                    if not torch.equal(b0, b1) and n.split(".")[0].split("[")[0] not in RESULT_ARGS \
                            and t.untyped_storage().data_ptr() not in ret_ptrs:
                        changed.append(n)
                runner.rec.append({"op": f"{mod.__name__.split('.')[-1]}.{name}",
                                   "in": runner.digest(torch.cat([b for _, b in pre])) if pre else "",
                                   "results": [(n, b) for n, b in post] + [(n, runner.raw(t)) for n, t in rets],
                                   "changed": changed})
                return r
            return rec

        # the pack-batch job table holds device pointers and its row offsets index them: its zones read as 0 (null, empty)
        # rather than as the poison word, so an over-read of it meets no wild address (check (c) cannot see such a read)
        init = ops.PackTable.__init__

        def table_init(tbl, jobs):
            init(tbl, jobs)
            torch.cuda.synchronize()
            for t in (tbl.jobs, tbl.first):
                if runner.rz.rz_fill_zones(t.data_ptr(), 0):
                    raise RuntimeError("rz_fill_zones refused the pack-batch table")
        ops.PackTable.__init__ = table_init

        for mod in (ops, imageops, rasterization):
            for name, f in list(vars(mod).items()):
                if inspect.isfunction(f) and f.__module__ == mod.__name__ and not name.startswith("_"):
                    setattr(mod, name, wrap(mod, name, f))

    def suite_item(self, item):
        import pytest
        torch = self.torch
        args = {a: item.funcargs[a] for a in item._fixtureinfo.argnames}
        recs, viol, errs, skipped = [], [], [], None
        for word in WORDS:
            self.rz.rz_set_word(word)
            v0 = self.rz.rz_violation_count()
            random.seed(0)
            torch.manual_seed(0)
            self.rec, err = [], None
            try:
                item.obj(**args)
            except pytest.skip.Exception as e:
                skipped = str(e)[:300]
            except BaseException as e:   # noqa: BLE001 -- recorded, the run goes on (KeyboardInterrupt aside)
                if isinstance(e, KeyboardInterrupt):
                    raise
                err = f"{type(e).__name__}: {str(e)[:1200]}\n" + traceback.format_exc()[-1500:]
            recs.append(self.rec)
            self.rec = None
            herr = self.settle()
            if herr:
                err = (err or "") + f" [allocator met HIP error {herr}]"
            viol.append(self.violations(v0))
            errs.append(err)
        problems = []
        if errs[1]:
            problems.append("pass B: " + errs[1])
        if errs[0] and not errs[1]:
            problems.append("pass A only (the result depends on the fill word): " + errs[0])
        if any(viol):
            problems.append("zone violations")
        changed = sorted({f"{r['op']}({n})" for rs in recs for r in rs for n in r["changed"]})
        if changed:
            problems.append(f"inputs written: {changed}")
        diffs = []
        if len(recs[0]) != len(recs[1]) and not any(errs):
            problems.append(f"the passes made different wrapper calls ({len(recs[0])} vs {len(recs[1])})")
        for i, (ra, rb) in enumerate(zip(recs[0], recs[1])):
            if ra["op"] != rb["op"] or ra["in"] != rb["in"]:
                break   # inputs already differ: the first differing result upstream names the cause
            for (n, a), (_, b) in zip(ra["results"], rb["results"]):
                d = self.ab_diff(a, b)
                if d[0]:
                    diffs.append({"call": i, "op": ra["op"], "result": n, "bytes_differ": d[0], "never_written": d[1],
                                  "first_byte": d[2] if len(d) > 2 else None, "bytes": int(a.numel())})
            if diffs:
                break
        if diffs:
            problems.append("results differ between pass A and pass B")
        return {"ok": not problems, "problems": problems, "violations": viol, "ab_diffs": diffs, "skipped": skipped,
                "calls": len(recs[1])}


class _Plugin:
    def __init__(self, runner):
        self.r = runner
        self.sel = {(f, fn) for f in SUITE for fn in _suite_funcs(f)}
        self.done = set()

    def _case(self, item):
        return f"{_stem(os.path.basename(str(item.fspath)))}::{item.originalname}"

    def pytest_collection_modifyitems(self, session, config, items):
        keep = [it for it in items if (os.path.basename(str(it.fspath)), it.originalname) in self.sel]
        drop = [it for it in items if it not in keep]
        if drop:
            config.hook.pytest_deselected(items=drop)
        items[:] = keep

    def pytest_runtest_setup(self, item):
        self.r.emit(case=self._case(item), item=item.nodeid, event="started", t=time.time())

    def pytest_pyfunc_call(self, pyfuncitem):
        t0 = time.time()
        row = self.r.suite_item(pyfuncitem)
        self.r.emit(case=self._case(pyfuncitem), item=pyfuncitem.nodeid, event="done", s=round(time.time() - t0, 2), **row)
        self.done.add(pyfuncitem.nodeid)
        return True

    def pytest_runtest_logreport(self, report):
        if report.when == "setup" and not report.passed and report.nodeid not in self.done:
            case = f"{_stem(os.path.basename(report.location[0]))}::{report.nodeid.split('::')[-1].split('[')[0]}"
            self.r.emit(case=case, item=report.nodeid, event="done", ok=bool(report.skipped), skipped=report.skipped or None,
                        problems=[] if report.skipped else ["fixture setup failed: " + str(report.longrepr)[-1500:]],
                        violations=[[], []], ab_diffs=[])


def main(so, report):
    t00 = time.time()
    os.environ.setdefault("DSG_TESTING", "1")
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    r = Runner(so, report)

    def case(cid, fn, *a):
        r.emit(case=cid, event="started", t=time.time())
        t0 = time.time()
        try:
            row = fn(*a)
        except Exception as e:   # noqa: BLE001
            row = {"ok": False, "problems": [f"{type(e).__name__}: {e}"[:1500] + traceback.format_exc()[-1500:]]}
        r.emit(case=cid, event="done", s=round(time.time() - t0, 2), **row)

    case(SELFTESTS[0], r.selftest, "write")
    case(SELFTESTS[1], r.selftest, "read")
    r.install_recorder()
    import pytest
    files = [os.path.join(ROOT, "tests", f) for f in SUITE]
    rc = pytest.main(files + ["-m", "gpu", "-q", "-p", "no:cacheprovider", "--rootdir", ROOT], plugins=[_Plugin(r)])
    r.emit(event="suite_exit", rc=int(rc))
    for k in UNET_FWD:
        case(unet_id(*k), r.unet_forward, *k)
    for k in TRAIN:
        case(train_id(*k), r.train_step, *k)
    r.emit(event="finished", s=round(time.time() - t00, 1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
