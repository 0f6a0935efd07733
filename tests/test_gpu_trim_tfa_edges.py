"""The catalogue of tests/trim_tfa_edges.py on an MI355X: every case through HipEngine and the C ABI, its submissions on one engine, built for
the compute units of the device that runs it.  The per-read results of every submission are held to the plain model first, then the whole
counter block, exactly (tests/test_trim_tfa_edges_model.py ties the model to the oracle without a GPU); the window family, which has
adapters, is held to OracleEngine.  Every case is run twice, on fresh engines.  After every submission with a base faqcs_kernel_report() must name the kernel the catalogue names and count ONE trim launch.  A
difference names the case, the submission, the read and the counter by its layout name.  Two settings:
    natural      no switch, in process: the cases whose every batch holds a read past 304 bases, and every --replace_to_N_q case
    single_pass  FAQCS_TRIM_LDS=0 (read once per process): the cases below 305 bases, which trim_lds would take -- this module once more, in
                 one child process, where the default setting is single_pass
One test per family and setting; the catalogue selects the cases of a setting (FCase.setting), nothing is skipped.  A submission of millions
of reads is a Tiled one: its arenas are unfolded by numpy, its expected results and counters by the repeats identity.  The cases about the
arenas' device address and the bytes around them go through faqcs_submit_device (TCase.shifts, te.device_buffers).  After the first engine
error nothing more is started on the device."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import trim_edges as te
import trim_tfa_edges as tf
from faqcs_amd import _capi as capi

pytestmark = pytest.mark.gpu

DEFAULT = "single_pass" if os.environ.get("FAQCS_TRIM_LDS") == "0" else "natural"
ENGINE_ERRORS = []
PAIRS = [(f, DEFAULT) for f in tf.FAMILIES if tf.cases_of(f, DEFAULT)]


@pytest.fixture(scope="module")
def n_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def counter_name(lay, k):
    name = [nm for nm, v in lay.items() if nm != "total" and v[0] <= k < v[0] + v[1]][0]
    return "%s[%d]" % (name, k - lay[name][0])


def submit_device_resident(hip, case, k):
    """Submission k through faqcs_submit_device: the arenas lie in device memory of the test's own, at the address mod 16 the case names, and the bytes in
    front of them and behind them (te.device_buffers) are what the kernel's over-reads meet"""
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
    b = capi.Batch(d_seq.data_ptr() + front, d_qual.data_ptr() + front, d_off.data_ptr(), n, len(seg) - 1, seg.ctypes.data, tf.sub_longest(sub))
    _check(hip.lib, hip.lib.faqcs_submit_device(hip.ctx, C.byref(b), res.data_ptr()))
    _check(hip.lib, hip.lib.faqcs_sync(hip.ctx))
    assert (d_seq.cpu().numpy() == seq).all() and (d_qual.cpu().numpy() == qual).all(), "%s: submission %d: the library wrote into the batch" % (case.name, k)
    return res[:n].cpu().numpy().view(np.uint16).view(capi.RESULT_DTYPE).ravel()


def describe_read(sub, k):
    """the k-th read of a submission (a Tiled one: by its place in the period or the remainder)"""
    if isinstance(sub, tf.Tiled):
        p, n = sub[0], len(sub[0]) * sub.repeats
        r = p[k % len(p)] if k < n else sub[1][k - n]
    else:
        r = [x for seg in sub for x in seg][k]
    return "%d bases seq=%r qual=%r" % (len(r[1]), r[1][:80], r[2][:80])


def run_on(hip, case, e, what):
    from faqcs_amd.engine import FaqcsError

    lay = capi.python_layout(case.R, hip.holder.n_adapters)
    try:
        for k, sub in enumerate(case.subs):
            got = submit_device_resident(hip, case, k) if case.shifts is not None else hip.process(*tf.arenas(sub))
            want = e["results"][k]
            assert len(got) == len(want) == tf.sub_n(sub), what
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, "%s: submission %d of %d reads, read %d (the first of %d that differ): hip=%s %s=%s: %s" % (
                what, k, len(got), bad[0], len(bad), got[bad[0]], tf.FAMILY_REFERENCE[case.family], want[bad[0]], describe_read(sub, int(bad[0])))
            kernel = case.kernel(k)
            if kernel:
                kt = capi.KernelTimes()
                assert hip.lib.faqcs_kernel_report(hip.ctx, C.byref(kt)) == 0
                assert (kt.trim_kernel or b"").decode() == kernel, "%s: submission %d ran %s, not %s" % (what, k, kt.trim_kernel, kernel)
                assert kt.n_launches == 1, "%s: submission %d took %d trim launches" % (what, k, kt.n_launches)
        counters = hip.counters()
    except FaqcsError as x:
        ENGINE_ERRORS.append("%s: %s" % (what, x))
        raise
    assert len(counters) == len(e["counters"]), what
    bad = np.nonzero(counters != e["counters"])[0]
    assert len(bad) == 0, "%s: %d counters differ: %s" % (what, len(bad), "; ".join(
        "%s: hip=%d %s=%d" % (counter_name(lay, int(k)), counters[k], tf.FAMILY_REFERENCE[case.family], e["counters"][k]) for k in bad[:8]))


@pytest.mark.parametrize("family,setting", PAIRS, ids=["%s-%s" % (s, f) for f, s in PAIRS])
def test_catalogue(family, setting, n_cu, monkeypatch):
    from faqcs_amd.engine import HipEngine

    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    monkeypatch.delenv("FAQCS_TRIM_LONG", raising=False)
    todo = tf.cases_of(family, setting, n_cu)
    assert todo
    t0 = time.time()
    for case in todo:
        assert case.expected()["error"] == 0
        if setting == "natural":   # (without a switch the plan must name this kernel by itself)
            assert all(case.plan(k, "natural")["kernel"] == case.kernel(k) for k in range(len(case.subs)) if case.kernel(k)), case.name
    t1 = time.time()
    for case in todo:
        for turn in range(2):
            hip = HipEngine(case.opt(), case.R, case.in_off, device=0)
            try:
                run_on(hip, case, case.expected(), "%s under %s (engine %d, %d compute units)" % (case.name, setting, turn, n_cu))
            finally:
                hip.close()
    print("%s under %s: %d cases, %d reads, %s %.1f s, device %.1f s" % (family, setting, len(todo), sum(c.n_reads() for c in todo), tf.FAMILY_REFERENCE[family], t1 - t0, time.time() - t1))


if DEFAULT == "natural":  # (not in the child process itself)
    def test_single_pass_setting_in_one_child_process():
        """FAQCS_TRIM_LDS=0 is read once per process: the catalogue's single_pass tests run in one fresh child, which starts no further process."""
        env = dict(os.environ, FAQCS_TRIM_LDS="0")
        env.pop("FAQCS_TRIM_LONG", None)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-s", "-k", "test_catalogue and single_pass"],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode(errors="replace")
        print(out[-2500:])
        n = len([f for f in tf.FAMILIES if tf.cases_of(f, "single_pass")])
        assert r.returncode == 0 and "%d passed" % n in out, out[-3000:]


def test_no_case_is_left_out(n_cu):
    cases = tf.all_cases(n_cu)
    ran = sorted(c.name for s in tf.SETTINGS for f in tf.FAMILIES for c in tf.cases_of(f, s, n_cu))
    assert ran == sorted(c.name for c in cases) and len({c.name for c in cases}) == len(cases)
    assert {c.family for c in cases} == set(tf.FAMILIES)
