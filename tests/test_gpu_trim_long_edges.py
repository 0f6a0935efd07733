"""The catalogue of tests/trim_long_edges.py on an MI355X: every case through HipEngine and the C ABI, its submissions on one engine, built for
the compute units of the device that runs it.  The per-read results of every submission are held to the plain model of tests/trim_edges.py
first, then the whole counter block (tests/test_trim_long_edges_model.py ties the model to the oracle without a GPU); the window family,
which has adapters, is held to OracleEngine; an expected error must be the engine's error.  Every case is run twice, on fresh engines.  One
test per family.  FAQCS_TRIM_LONG, which the library reads at every submission, is set for the cases that send short batches to trim_long
and removed for the others; faqcs_kernel_report() must name trim_long after every submission with a base that the catalogue sends there, and
the chunked kernel after the others.  A difference names the case, the submission, the read and the counter by its layout name.  After the
first engine error nothing more is started on the device."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import trim_edges as te
import trim_long_edges as tl
from faqcs_amd import _capi as capi
from faqcs_amd import driver

pytestmark = pytest.mark.gpu

ENGINE_ERRORS = []


@pytest.fixture(scope="module")
def n_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def counter_name(lay, k):
    name = [nm for nm, v in lay.items() if nm != "total" and v[0] <= k < v[0] + v[1]][0]
    return "%s[%d]" % (name, k - lay[name][0])


def submit_device_resident(hip, case, k):
    """Submission k through faqcs_submit_device with the max_read_len the case names (0: the library falls back to the context's capacity)"""
    import torch

    from faqcs_amd.engine import _check

    dev = torch.device("cuda:0")
    seq, qual, front, offset, seg = te.device_buffers(case.subs[k], case.in_off, 0, False)
    n = len(offset) - 1
    d_seq, d_qual = torch.from_numpy(seq).to(dev), torch.from_numpy(qual).to(dev)
    d_off = torch.from_numpy(offset.view(np.int32)).to(dev)
    res = torch.zeros((max(n, 1), 4), dtype=torch.int16, device=dev)
    assert d_seq.data_ptr() % 16 == 0 and d_qual.data_ptr() % 16 == 0 and front >= capi.ARENA_PAD_BEFORE and len(seq) - front - int(offset[-1]) >= capi.ARENA_PAD_AFTER
    torch.cuda.synchronize()
    b = capi.Batch(d_seq.data_ptr() + front, d_qual.data_ptr() + front, d_off.data_ptr(), n, len(seg) - 1, seg.ctypes.data, case.device_max_len)
    _check(hip.lib, hip.lib.faqcs_submit_device(hip.ctx, C.byref(b), res.data_ptr()))
    _check(hip.lib, hip.lib.faqcs_sync(hip.ctx))
    return res[:n].cpu().numpy().view(np.uint16).view(capi.RESULT_DTYPE).ravel()


def expected_kernel(case, k):
    longest = max([len(r[1]) for seg in case.subs[k] for r in seg] or [0])
    if longest == 0:
        return None
    if case.runs_trim_long(k):
        return "trim_long"
    return "trim_filter_accumulate" if longest > te.ROW_LAST[-1] or case.opt().replace_to_N_q or os.environ.get("FAQCS_TRIM_LDS") == "0" else "trim_lds"


def run_on(hip, case, e, what):
    from faqcs_amd.engine import FaqcsError

    lay = capi.python_layout(case.R, hip.holder.n_adapters)
    error = 0
    try:
        for k, sub in enumerate(case.subs):
            got = submit_device_resident(hip, case, k) if case.device_max_len is not None else hip.process(*driver.pack_segments(sub))
            if case.error:
                continue
            want = e["results"][k]
            bad = np.nonzero(got != want)[0]
            if len(bad):
                reads = [r for seg in sub for r in seg]
                raise AssertionError("%s: submission %d, read %d of %d bases (the first of %d that differ): hip=%s %s=%s seq=%r qual=%r" % (
                    what, k, bad[0], len(reads[bad[0]][1]), len(bad), got[bad[0]], tl.FAMILY_REFERENCE[case.family], want[bad[0]], reads[bad[0]][1][:80], reads[bad[0]][2][:80]))
            kernel = expected_kernel(case, k)
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
    assert error == e["error"], "%s: error %d, expected %d" % (what, error, e["error"])
    if not error:
        assert len(counters) == len(e["counters"]), what
        bad = np.nonzero(counters != e["counters"])[0]
        assert len(bad) == 0, "%s: %d counters differ: %s" % (what, len(bad), "; ".join(
            "%s: hip=%d %s=%d" % (counter_name(lay, int(k)), counters[k], tl.FAMILY_REFERENCE[case.family], e["counters"][k]) for k in bad[:8]))


@pytest.mark.parametrize("family", tl.FAMILIES)
def test_catalogue(family, n_cu, monkeypatch):
    from faqcs_amd.engine import HipEngine

    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    todo = tl.family_cases(family, n_cu)
    assert todo and any(c.runs_trim_long(k) for c in todo for k in range(len(c.subs)))
    t0 = time.time()
    for case in todo:
        case.expected()
    t1 = time.time()
    for case in todo:
        if case.force_long:
            monkeypatch.setenv("FAQCS_TRIM_LONG", "1")
        else:
            monkeypatch.delenv("FAQCS_TRIM_LONG", raising=False)
        for turn in range(2):
            hip = HipEngine(case.opt(), case.R, case.in_off, device=0)
            try:
                run_on(hip, case, case.expected(), "%s (engine %d, %d compute units)" % (case.name, turn, n_cu))
            finally:
                hip.close()
    print("%s: %d cases, %d reads, %s %.1f s, device %.1f s" % (family, len(todo), sum(c.n_reads() for c in todo), tl.FAMILY_REFERENCE[family], t1 - t0, time.time() - t1))


def test_no_case_is_left_out(n_cu):
    cases = tl.all_cases(n_cu)
    assert sorted(c.name for f in tl.FAMILIES for c in tl.family_cases(f, n_cu)) == sorted(c.name for c in cases) and len({c.name for c in cases}) == len(cases)
    assert {c.family for c in cases} == set(tl.FAMILIES)
