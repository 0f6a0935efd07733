"""The catalogue of tests/trim_edges.py on an MI355X: every case through HipEngine and the C ABI, its submissions on one engine.  The per-read
results of every submission are held to the plain model of the catalogue first, then the whole counter block (tests/test_trim_edges_model.py
ties the model to the oracle without a GPU); an expected error must be the engine's error.  Every case is run twice, on fresh engines.  The
catalogue runs under three settings:
    lds          the default: trim_lds up to 304 bases, trim_filter_accumulate up to 1 024, trim_long past that
    long         FAQCS_TRIM_LONG=1 (read at every submission): every batch through trim_long
    single_pass  FAQCS_TRIM_LDS=0 (read once per process): trim_filter_accumulate instead of trim_lds -- this module once more, in one child
                 process, where the default setting is single_pass
One test per family and setting; the kernel faqcs_kernel_report() names is asserted after every submission.  A case that does not run under a
setting is excluded by name in the catalogue (trim_edges.cases_of), never skipped here.

faqcs_submit() copies a host batch into device buffers whose pads the library owns, so what lies around a host arena never reaches the kernels.
The cases that are about the bytes around the arenas and about the arenas' device address (TCase.shifts) are therefore submitted device-resident,
through faqcs_submit_device(): the arenas lie in a torch buffer at the named address mod 16, with 0xFF, N and qualities above 41 in the 64 bytes
and more either side of them, which is where the kernels' over-reads land."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import trim_edges as te
from faqcs_amd import _capi as capi
from faqcs_amd import driver

pytestmark = pytest.mark.gpu

DEFAULT = "single_pass" if os.environ.get("FAQCS_TRIM_LDS") == "0" else "lds"
ENGINE_ERRORS = []
PAIRS = [(f, s) for s in (DEFAULT, "long") for f in te.FAMILIES if te.cases_of(f, s)]


@pytest.fixture(scope="module")
def cases():
    return te.all_cases()


def expected_kernel(case, k, setting):
    """The kernel the k-th submission of a case must report under a setting, or None for a batch without a base"""
    longest = max([len(r[1]) for seg in case.subs[k] for r in seg] or [0])
    if longest == 0:
        return None
    if setting == "long" or longest > te.FAST_READ_LENGTH:
        return "trim_long"
    if setting == "single_pass" or longest > te.ROW_LAST[-1] or case.opt().replace_to_N_q:
        return "trim_filter_accumulate"
    return "trim_lds"


def counter_name(lay, k):
    name = [nm for nm, v in lay.items() if nm != "total" and v[0] <= k < v[0] + v[1]][0]
    return "%s[%d]" % (name, k - lay[name][0])


def submit_device_resident(hip, case, k):
    """Submission k of a case through faqcs_submit_device: the arenas lie in device memory of the test's own, at the address mod 16 the case names,
    and the bytes in front of them and behind them (te.device_buffers) are what the kernels' over-reads meet"""
    import torch

    from faqcs_amd.engine import _check

    dev = torch.device("cuda:0")
    sub = case.subs[k]
    seq, qual, front, offset, seg = te.device_buffers(sub, case.in_off, case.shifts[k], case.hostile)
    n = len(offset) - 1
    d_seq, d_qual = torch.from_numpy(seq).to(dev), torch.from_numpy(qual).to(dev)
    d_off = torch.from_numpy(offset.view(np.int32)).to(dev)
    res = torch.zeros((max(n, 1), 4), dtype=torch.int16, device=dev)
    assert d_seq.data_ptr() % 16 == 0 and d_qual.data_ptr() % 16 == 0 and front >= capi.ARENA_PAD_BEFORE and len(seq) - front - int(offset[-1]) >= capi.ARENA_PAD_AFTER
    torch.cuda.synchronize()
    longest = max([len(r[1]) for s in sub for r in s] or [0])
    b = capi.Batch(d_seq.data_ptr() + front, d_qual.data_ptr() + front, d_off.data_ptr(), n, len(seg) - 1, seg.ctypes.data, longest)
    _check(hip.lib, hip.lib.faqcs_submit_device(hip.ctx, C.byref(b), res.data_ptr()))
    _check(hip.lib, hip.lib.faqcs_sync(hip.ctx))
    assert (d_seq.cpu().numpy() == seq).all() and (d_qual.cpu().numpy() == qual).all(), "%s: submission %d: the library wrote into the batch" % (case.name, k)
    return res[:n].cpu().numpy().view(np.uint16).view(capi.RESULT_DTYPE).ravel()


def run_case(case, setting):
    from faqcs_amd.engine import HipEngine

    e = case.expected()
    for turn in range(2):
        hip = HipEngine(case.opt(), case.R, case.in_off, device=0)
        try:
            run_on(hip, case, setting, e, "%s under %s (engine %d)" % (case.name, setting, turn))
        finally:
            hip.close()


def run_on(hip, case, setting, e, what):
    from faqcs_amd.engine import FaqcsError

    lay = te.layout(case.R)
    error = 0
    try:
        for k, sub in enumerate(case.subs):
            got = submit_device_resident(hip, case, k) if case.shifts is not None else hip.process(*driver.pack_segments(sub))
            if case.error:
                continue
            want = e["results"][k]
            bad = np.nonzero(got != want)[0]
            if len(bad):
                reads = [r for seg in sub for r in seg]
                raise AssertionError("%s: submission %d, read %d (the first of %d that differ): hip=%s model=%s seq=%r qual=%r" % (
                    what, k, bad[0], len(bad), got[bad[0]], want[bad[0]], reads[bad[0]][1][:80], reads[bad[0]][2][:80]))
            kernel = expected_kernel(case, k, setting)
            if case.kernels and setting == "lds":
                assert kernel == case.kernels[k], "%s: the catalogue names %s for submission %d" % (what, case.kernels[k], k)
            if kernel:
                kt = capi.KernelTimes()
                assert hip.lib.faqcs_kernel_report(hip.ctx, C.byref(kt)) == 0
                assert (kt.trim_kernel or b"").decode() == kernel, "%s: submission %d ran %s, not %s" % (what, k, kt.trim_kernel, kernel)
        counters = hip.counters()
    except FaqcsError as x:
        error = x.code
        if not case.error:
            ENGINE_ERRORS.append("%s: %s" % (what, x))
            raise
    assert error == e["error"], "%s: error %d, the model's %d" % (what, error, e["error"])
    if not error:
        bad = np.nonzero(counters != e["counters"])[0]
        assert len(bad) == 0, "%s: %d counters differ: %s" % (what, len(bad), "; ".join(
            "%s: hip=%d model=%d" % (counter_name(lay, int(k)), counters[k], e["counters"][k]) for k in bad[:8]))


@pytest.mark.parametrize("family,setting", PAIRS, ids=["%s-%s" % (s, f) for f, s in PAIRS])
def test_catalogue(cases, family, setting, monkeypatch):
    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    if setting == "long":
        monkeypatch.setenv("FAQCS_TRIM_LONG", "1")
    else:
        monkeypatch.delenv("FAQCS_TRIM_LONG", raising=False)
    todo = te.cases_of(family, setting, cases)
    assert todo
    t0 = time.time()
    for case in todo:
        case.expected()
    t1 = time.time()
    for case in todo:
        run_case(case, setting)
    print("%s under %s: %d cases, %d reads, model %.1f s, device %.1f s" % (family, setting, len(todo), sum(c.n_reads() for c in todo), t1 - t0, time.time() - t1))


if DEFAULT == "lds":  # (not in the child process itself)
    def test_single_pass_setting_in_one_child_process():
        """FAQCS_TRIM_LDS=0 is read once per process: the catalogue's single_pass tests run in one fresh child, which starts no further process."""
        env = dict(os.environ, FAQCS_TRIM_LDS="0")
        env.pop("FAQCS_TRIM_LONG", None)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-s", "-k", "test_catalogue and single_pass"],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode(errors="replace")
        print(out[-1500:])
        n = len([f for f in te.FAMILIES if te.cases_of(f, "single_pass")])
        assert r.returncode == 0 and "%d passed" % n in out, out[-3000:]


def test_no_case_is_left_out(cases):
    ran = {(c.name, s) for s in te.SETTINGS for f in te.FAMILIES for c in te.cases_of(f, s, cases)}
    assert ran == {(c.name, s) for c in cases for s in te.SETTINGS if s not in c.exclude}
    assert {c.name for c in cases} == {name for name, _ in ran}
    assert {s for _, s in PAIRS} | {"single_pass"} >= set(te.SETTINGS) and {f for f, _ in PAIRS} == set(te.FAMILIES)
