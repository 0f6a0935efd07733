"""The catalogue of tests/submit_edges.py on an MI355X: every schedule on a fresh HipEngine through the C ABI, twice.  Host submissions go
through faqcs_submit_async from faqcs_host_alloc memory -- arenas, offsets, terminal_n flags and results --, device submissions through
faqcs_submit_device from torch buffers; nothing waits but where the schedule says so.  Per-read results are compared with the oracle's
behind the faqcs_wait of their ticket, or behind the next call that waits for the compute stream; the whole counter block at every finish
and export; and at the end the tallies of faqcs_path_tallies_get() must be the ones submit_edges.trace() predicts from the schedule alone,
which is what says that the arm a schedule is about -- tail fold, aux fold, slot regrow, ring wait -- is the arm that ran.  Everything
is an integer and compared for equality.  tests/test_submit_edges_model.py ties the expectations and the trace down without a GPU.

FAQCS_TRIM_LDS=0 is read once per process: the schedules of that setting run in this module once more, in one child process."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import submit_edges as se
from faqcs_amd import _capi as capi

pytestmark = pytest.mark.gpu

SETTING = "single_pass" if os.environ.get("FAQCS_TRIM_LDS") == "0" else "lds"
ENGINE_ERRORS = []
PAIRS = [f for f in se.FAMILIES if se.schedules_of(f, SETTING)]


@pytest.fixture(scope="module")
def schedules():
    return se.all_schedules()


class Pinned:
    """faqcs_host_alloc memory bound as numpy arrays; free() hands every block back (call it with nothing in flight)"""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def array(self, src):
        src = np.ascontiguousarray(src)
        nbytes = max(src.nbytes, 16)
        p = self.lib.faqcs_host_alloc(nbytes)
        assert p, "faqcs_host_alloc(%d) failed" % nbytes
        self.ptrs.append(p)
        a = np.frombuffer((C.c_uint8 * nbytes).from_address(p), np.uint8)[:src.nbytes].view(src.dtype)
        a[...] = src.ravel()
        return p, a

    def free(self):
        for p in self.ptrs:
            self.lib.faqcs_host_free(p)
        self.ptrs = []


def first_difference(what, k, got, want, b):
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        a, z = int(b.offset[i]), int(b.offset[i + 1])
        raise AssertionError("%s: submission %d, read %d (the first of %d that differ): hip=%s oracle=%s seq=%r qual=%r" % (
            what, k, i, len(bad), got[i], want[i], b.seq[a:z].tobytes()[:80], b.qual[a:z].tobytes()[:80]))


def block_difference(what, at, got, want, s):
    bad = np.nonzero(got != want)[0]
    if len(bad):
        lay = capi.python_layout(s.R, len(s.opt().adapter) if s.opt().adapters_active() else 0)
        names = []
        for k in bad[:8]:
            name = [nm for nm, v in lay.items() if nm != "total" and v[0] <= k < v[0] + v[1]][0]
            names.append("%s[%d]: hip=%d oracle=%d" % (name, k - lay[name][0], got[k], want[k]))
        raise AssertionError("%s: operation %d: %d counters differ: %s" % (what, at, len(bad), "; ".join(names)))


def run_on(hip, s, e, T, what):
    import torch

    from faqcs_amd.engine import _check

    lib, ctx, dev = hip.lib, hip.ctx, torch.device("cuda:0")
    pinned, keep, subs, exported = Pinned(lib), [], [], None
    total = hip.n_counters
    env_before = os.environ.pop("FAQCS_TAIL_FOLD", None)

    def results_of(k):
        r = subs[k]
        if r["res"] is None:
            return None
        return r["res"].copy() if r["via"] == "host" else r["res"][:r["b"].n].cpu().numpy().view(np.uint16).view(capi.RESULT_DTYPE).ravel()

    def check_results(upto=None):
        for k, r in enumerate(subs):
            if not r["checked"] and r["res"] is not None and e["results"][k] is not None and (upto is None or k < upto):
                first_difference(what, k, results_of(k), e["results"][k], r["b"])
                r["checked"] = True

    try:
        # every buffer of the schedule before its first call: no allocation, upload or device-wide wait of the test's own falls between two submissions
        ready, inputs = [], {}
        for b in s.batches:
            if b.via == "host":
                if id(b) not in inputs:  # (a Batch object submitted several times is the same host memory each time, as a caller's unchanged buffer is)
                    seq, qual, off = b.host_arenas()
                    inputs[id(b)] = (pinned.array(seq), pinned.array(qual), pinned.array(off), pinned.array(b.terminal_n()) if b.tn else (None, None))
                ready.append(inputs[id(b)] + ((pinned.array(np.full(max(b.n, 1), 0xAB, np.uint64)) if b.results else (None, None)),))  # (0xABAB is never a result's flags)
            else:
                seq, qual, front = b.device_arenas()
                d_seq, d_qual = torch.from_numpy(seq).to(dev), torch.from_numpy(qual).to(dev)
                d_off = torch.from_numpy(b.offset.view(np.int32)).to(dev)
                res = torch.full((max(b.n, 1), 4), 0x2B2B, dtype=torch.int16, device=dev)
                assert d_seq.data_ptr() % 16 == 0 and d_qual.data_ptr() % 16 == 0 and b.n and b.longest
                ready.append((seq, qual, front, d_seq, d_qual, d_off, res))
        spare = torch.zeros(total, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for at, op in enumerate(s.ops):
            kind = op[0]
            if kind == "tail_fold":
                if op[1] is None:
                    os.environ.pop("FAQCS_TAIL_FOLD", None)
                else:
                    os.environ["FAQCS_TAIL_FOLD"] = op[1]
            elif kind == "submit":
                b, k = op[1], len(subs)
                keep.append(b.seg)
                if b.via == "host":
                    (ps, a_s), (pq, a_q), (po, a_o), (pt, a_t), (pr, a_r) = ready[k]
                    batch = capi.Batch(ps, pq, po, b.n, 1, b.seg.ctypes.data, 0, pt)
                    ticket = C.c_uint64(1 << 60)
                    _check(lib, lib.faqcs_submit_async(ctx, C.byref(batch), pr, C.byref(ticket)))
                    assert ticket.value == T.subs[k]["ticket"], "%s: submission %d got ticket %d" % (what, k, ticket.value)
                    subs.append(dict(b=b, via="host", res=None if a_r is None else a_r.view(capi.RESULT_DTYPE)[:b.n], checked=False, arrays=[a_s, a_q, a_o, a_t], ticket=ticket.value))
                else:
                    seq, qual, front, d_seq, d_qual, d_off, res = ready[k]
                    batch = capi.Batch(d_seq.data_ptr() + front, d_qual.data_ptr() + front, d_off.data_ptr(), b.n, 1, b.seg.ctypes.data, b.longest, None)
                    _check(lib, lib.faqcs_submit_device(ctx, C.byref(batch), res.data_ptr()))
                    subs.append(dict(b=b, via="device", res=res, checked=False, tensors=(d_seq, d_qual, d_off), host=(seq, qual)))
            elif kind == "wait":
                k = op[1]
                if k >= len(subs) or subs[k]["via"] != "host":
                    n_host = sum(1 for r in subs if r["via"] == "host")
                    assert lib.faqcs_wait(ctx, n_host + 5) == capi.E_INVAL and lib.faqcs_wait(ctx, n_host) == capi.E_INVAL, "%s: an unknown ticket was taken" % what
                else:
                    _check(lib, lib.faqcs_wait(ctx, subs[k]["ticket"]))
                    if subs[k]["res"] is not None:  # behind faqcs_wait alone: whatever was submitted later may still be in flight
                        first_difference(what, k, results_of(k), e["results"][k], subs[k]["b"])
                        subs[k]["checked"] = True
            elif kind == "hostile":
                a_s, a_q, a_o, a_t = subs[op[1]]["arrays"]
                a_s[...] = 0xFF
                a_q[...] = se.HOSTILE_Q
                a_o[...] = 0xFFFFFFF0
                if a_t is not None:
                    a_t[...] = 3
            elif kind == "sync":
                _check(lib, lib.faqcs_sync(ctx))
                check_results()
            elif kind == "finish":
                block = np.zeros(total, np.uint64)
                _check(lib, lib.faqcs_finish(ctx, block.ctypes.data, total))
                check_results()
                block_difference(what, at, block, e["blocks"][at], s)
            elif kind == "export":
                exported = spare
                _check(lib, lib.faqcs_counters_export(ctx, exported.data_ptr(), total))
                check_results()
                block_difference(what, at, exported.cpu().numpy().view(np.uint64), e["blocks"][at], s)
            elif kind == "import":
                _check(lib, lib.faqcs_counters_import(ctx, exported.data_ptr(), total))
                check_results()
            elif kind == "reset":
                _check(lib, lib.faqcs_reset_counters(ctx))
            elif kind == "set_quality":
                _check(lib, lib.faqcs_set_quality(ctx, op[1]))
            elif kind == "set_offset":
                _check(lib, lib.faqcs_set_input_quality_offset(ctx, op[1]))
                check_results()
            elif kind == "expect_error":
                rc = lib.faqcs_sync(ctx)
                j, code = e["error"]
                assert rc == op[1] == code, "%s: faqcs_sync returned %d, the oracle stops with %d" % (what, rc, code)
                check_results(upto=j)
                at_read = int(subs[j]["b"].kind.split()[-1])
                flags = int(results_of(j)[at_read]["flags"])
                assert flags & capi.F_ERR_QUALITY, "%s: read %d of submission %d has flags %#x" % (what, at_read, j, flags)
            else:
                raise AssertionError(kind)
        assert all(r["checked"] or r["res"] is None or e["results"][k] is None for k, r in enumerate(subs)), what
        for k, r in enumerate(subs):  # a device-resident batch is the caller's: the library wrote nothing into it
            if r["via"] == "device":
                assert (r["tensors"][0].cpu().numpy() == r["host"][0]).all() and (r["tensors"][1].cpu().numpy() == r["host"][1]).all(), "%s: submission %d: the library wrote into the batch" % (what, k)
        t = capi.PathTallies()
        assert lib.faqcs_path_tallies_get(ctx, C.byref(t)) == 0
        got = {n: int(getattr(t, n)) for n in se.TALLIES}
        assert got == T.tallies, "%s: the arms taken %s, trace() predicts %s" % (what, got, T.tallies)
        return got
    finally:
        lib.faqcs_sync(ctx)  # (nothing in flight when the pinned memory goes back; its verdict was taken above)
        pinned.free()
        os.environ.pop("FAQCS_TAIL_FOLD", None)
        if env_before is not None:
            os.environ["FAQCS_TAIL_FOLD"] = env_before


def run_schedule(s):
    from faqcs_amd.engine import FaqcsError, HipEngine

    e, T = s.expected(), se.trace(s)
    taken = None
    for turn in range(2):
        what = "%s (engine %d)" % (s.name, turn)
        hip = HipEngine(s.opt(), s.R, s.in_off, device=0)
        try:
            taken = run_on(hip, s, e, T, what)
        except FaqcsError as x:
            ENGINE_ERRORS.append("%s: %s" % (what, x))
            raise
        finally:
            hip.close()
    return taken


@pytest.mark.parametrize("family", PAIRS)
def test_catalogue(schedules, family):
    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    todo = se.schedules_of(family, SETTING, schedules)
    assert todo
    t0 = time.time()
    for s in todo:
        s.expected()
    t1 = time.time()
    arms = dict.fromkeys(se.TALLIES, 0)
    for s in todo:
        for k, v in run_schedule(s).items():
            arms[k] += v
    print("%s under %s: %d schedules, %d reads, oracle %.1f s, device %.1f s; arms taken: %s" % (
        family, SETTING, len(todo), sum(s.n_reads() for s in todo), t1 - t0, time.time() - t1, arms))


if SETTING == "lds":  # (not in the child process itself)
    def test_single_pass_setting_in_one_child_process(schedules):
        """FAQCS_TRIM_LDS=0 is read once per process: the schedules of that setting run in one fresh child, which starts no further process."""
        assert not ENGINE_ERRORS, "not run: an engine call failed before (%s)" % ENGINE_ERRORS[0]
        env = dict(os.environ, FAQCS_TRIM_LDS="0")
        env.pop("FAQCS_TAIL_FOLD", None)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-s", "-k", "test_catalogue"],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode(errors="replace")
        print(out[-1500:])
        n = len([f for f in se.FAMILIES if se.schedules_of(f, "single_pass", schedules)])
        assert n >= 1 and r.returncode == 0 and "%d passed" % n in out, out[-3000:]


def test_no_schedule_is_left_out(schedules):
    ran = {s.name for st in se.SETTINGS for f in se.FAMILIES for s in se.schedules_of(f, st, schedules)}
    assert ran == {s.name for s in schedules}
    assert set(PAIRS) == {s.family for s in schedules if s.setting == SETTING}
