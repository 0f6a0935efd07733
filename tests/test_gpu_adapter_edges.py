"""The catalogue of tests/adapter_edges.py on an MI355X: every case through HipEngine and the C ABI, its submissions on one engine.  After every
submission the whole records equal the OracleEngine's bit for bit, and the fields the catalogue's plain model predicts (adapter, FAQCS_F_ADAPTER,
FAQCS_F_VALID, start / len of a read that is not filtered) equal the model's; after the last one the whole counter block equals the oracle's and
adapter_stats the model's (tests/test_adapter_edges_model.py ties the model to the oracle without a GPU).  A case with a rejected byte expects
FAQCS_F_ERR_BASE on the reads that hold one, on no other, and FAQCS_E_BASE from faqcs_sync.  Every case is run twice, on fresh engines.  The
catalogue runs under three settings:
    default        the normal dispatch
    prefilter_off  FAQCS_DBG=8 (read by faqcs_create; set per test, before the engine is made): every target goes to the exact aligner and the pair
                   kernel is off -- the results must be those with the filters on, which is what makes the filters sound
    no_pair        FAQCS_ADAPTER_PAIR=0 (read once per process): adapter_overlap<., 256> for the cases that take the pair kernel by default -- this
                   module once more, in one child process
One test per family and setting.  A case that does not run under a setting is excluded by name in the catalogue (adapter_edges.cases_of), never
skipped here."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import adapter_edges as ae
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from test_adapter_edges_model import check_fields, compare_with_oracle

pytestmark = pytest.mark.gpu

CHILD = os.environ.get("FAQCS_ADAPTER_PAIR") == "0"
ENGINE_ERRORS = []
PAIRS = [(f, s) for s in (("no_pair",) if CHILD else ("default", "prefilter_off")) for f in ae.FAMILIES if ae.cases_of(f, s)]


@pytest.fixture(scope="module")
def cases():
    return ae.all_cases()


def oracle_of(case):
    """(results per submission, counters) of the OracleEngine, or (None, None) where it fails with the error the model expects; once per case"""
    if getattr(case, "_oracle", None) is None:
        case._oracle = compare_with_oracle(case, case.expected())
    return case._oracle


def run_case(case, setting):
    from faqcs_amd.engine import HipEngine

    for turn in range(2):
        hip = HipEngine(case.opt(), case.R, case.in_off, device=0)
        try:
            run_on(hip, case, "%s under %s (engine %d)" % (case.name, setting, turn))
        finally:
            hip.close()


def run_on(hip, case, what):
    from faqcs_amd.engine import FaqcsError

    e = case.expected()
    ora_results, ora_counters = oracle_of(case)
    try:
        for k in range(len(case.subs)):
            recs = case.records(k)
            if e["error"]:                                     # the submission fails: the records are read past the error
                seq, qual, offset, seg = driver.pack_segments(recs)
                got = np.zeros(len(offset) - 1, dtype=capi.RESULT_DTYPE)
                b = capi.Batch(seq.ctypes.data, qual.ctypes.data, offset.ctypes.data, len(got), len(seg) - 1, seg.ctypes.data, 0, None)
                rc = hip.lib.faqcs_submit(hip.ctx, C.byref(b), got.ctypes.data)
                assert rc == 0, "%s: faqcs_submit returned %d" % (what, rc)
                rc = hip.lib.faqcs_sync(hip.ctx)
                assert rc == e["error"], "%s: faqcs_sync returned %d, the model expects %d" % (what, rc, e["error"])
                want = e["results"][k]
                flagged, bad = np.nonzero(got["flags"] & ae.F_ERR_BASE)[0], np.nonzero(want["flags"] & ae.F_ERR_BASE)[0]
                assert list(flagged) == list(bad), "%s: FAQCS_F_ERR_BASE on the reads %s, the model expects it on %s" % (what, list(flagged), list(bad))
                ok = (want["flags"] & ae.F_ERR_BASE) == 0      # every other read's result stands
                check_fields(got[ok], want[ok], "%s: submission %d: the reads without a rejected byte: hip" % (what, k))
                return
            got = hip.process(*driver.pack_segments(recs))
            check_fields(got, e["results"][k], "%s: submission %d: hip" % (what, k))
            diff = np.nonzero(got != ora_results[k])[0]
            assert len(diff) == 0, "%s: submission %d, read %d (the first of %d that differ): hip=%s oracle=%s seq=%r" % (
                what, k, diff[0], len(diff), got[diff[0]], ora_results[k][diff[0]], [r for seg in case.subs[k] for r in seg][diff[0]][:100])
        counters = hip.counters()
    except FaqcsError as x:
        ENGINE_ERRORS.append("%s: %s" % (what, x))
        raise
    lay = capi.python_layout(case.R, len(case.lib))
    o, n = lay["adapter_stats"]
    assert (counters[o:o + n] == e["stats"]).all(), "%s: adapter_stats: hip %s, the model %s" % (what, counters[o:o + n], e["stats"])
    diff = np.nonzero(counters != ora_counters)[0]
    assert len(diff) == 0, "%s: %d counters differ from the oracle's, the first at %d: hip=%d oracle=%d" % (what, len(diff), diff[0] if len(diff) else -1,
                                                                                                   counters[diff[0]] if len(diff) else 0, ora_counters[diff[0]] if len(diff) else 0)


@pytest.mark.parametrize("family,setting", PAIRS, ids=["%s-%s" % (s, f) for f, s in PAIRS])
def test_catalogue(cases, family, setting, monkeypatch):
    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    if setting == "prefilter_off":
        monkeypatch.setenv("FAQCS_DBG", "8")
    else:
        monkeypatch.delenv("FAQCS_DBG", raising=False)
    todo = ae.cases_of(family, setting, cases)
    assert todo
    t0 = time.time()
    for case in todo:
        oracle_of(case)
    t1 = time.time()
    for case in todo:
        run_case(case, setting)
    print("%s under %s: %d cases, %d reads, model and oracle %.1f s, device %.1f s" % (family, setting, len(todo), sum(c.n_reads() for c in todo), t1 - t0, time.time() - t1))


if not CHILD:  # (not in the child process itself)
    def test_no_pair_setting_in_one_child_process():
        """FAQCS_ADAPTER_PAIR=0 is read once per process: the catalogue's no_pair tests run in one fresh child, which starts no further process."""
        env = dict(os.environ, FAQCS_ADAPTER_PAIR="0")
        env.pop("FAQCS_DBG", None)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-s", "-k", "test_catalogue and no_pair"],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode(errors="replace")
        print(out[-1500:])
        n = len([f for f in ae.FAMILIES if ae.cases_of(f, "no_pair")])
        assert n >= 5 and r.returncode == 0 and "%d passed" % n in out, out[-3000:]


def test_no_case_is_left_out(cases):
    ran = {(c.name, s) for s in ae.SETTINGS for f in ae.FAMILIES for c in ae.cases_of(f, s, cases)}
    assert ran == {(c.name, s) for c in cases for s in ae.SETTINGS if s not in c.exclude}
    assert {c.name for c in cases} == {name for name, _ in ran}
    assert {s for _, s in PAIRS} | ({"default", "prefilter_off"} if CHILD else {"no_pair"}) >= set(ae.SETTINGS)
    assert {f for f, s in PAIRS if s != "no_pair"} == (set() if CHILD else set(ae.FAMILIES))
    assert all(c.takes_pair() == ("no_pair" not in c.exclude) for c in cases)
