"""The catalogue of tests/adapter_edges.py without a GPU: its restated constants and its restated dispatch against their sources, its coverage
table (every edge claimed, every claim of a case true, every case in a family), its mutants (every wrong variant of the model changes what some
case expects), and its plain model against the oracle: pair by pair through faqcs_oracle_align and faqcs_oracle_find_mask_range, and on every
whole case through OracleEngine.process -- the predicted record fields, adapter_stats, and FAQCS_E_BASE where a read holds a rejected byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adapter_edges as ae
from faqcs_amd import _capi as capi
from faqcs_amd import driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return ae.all_cases()


def test_restated_constants_equal_the_sources():
    for name, (path, rx) in ae.CONSTANT_SOURCES.items():
        m = re.search(rx, open(os.path.join(ROOT, path)).read())
        assert m, "%s: %s no longer states it as %r" % (name, path, rx)
        assert getattr(ae, name) == int(m.group(1)), name
    assert (ae.F_VALID, ae.F_ADAPTER, ae.F_ERR_BASE, ae.E_BASE) == (capi.F_VALID, capi.F_ADAPTER, capi.F_ERR_BASE, capi.E_BASE)
    assert ae.RESULT_DTYPE == capi.RESULT_DTYPE
    kernel = open(os.path.join(ROOT, "faqcs_amd", "csrc", "faqcs_adapter_kernel.hip")).read()
    launcher = kernel[kernel.index("static hipError_t launch_adapter("):kernel.index("hipError_t faqcs_launch_adapter(")]
    at = 0
    for rx, want in ae.LAUNCHER_SOURCES:                       # the gates, in the launcher's order
        m = re.compile(rx).search(launcher, at)
        assert m, "launch_adapter no longer states %r" % rx
        assert tuple(int(g) for g in m.groups()) == want, rx
        at = m.end()
    assert ae.WIDTHS == (256, 320, 1024, 4096, 8192, 16384, 32768)
    # a library with a '-' in a target: no pair kernel, no prefilter, no bound pass (launches(gap=True) is launches under prefilter_off)
    assert "(dbg & 8u) == 0u && A.has_gap == 0u) {" in launcher and "const bool prefilter_on = uni((int)((dbg & 8u) == 0u && A.has_gap == 0u)) != 0;" in kernel
    assert re.search(r"const bool pruned = .* && A\.has_gap == 0u;", kernel)
    assert ae.launches([40, 30], 150, "default", gap=True) == ae.launches([40, 30], 150, "prefilter_off") == [("256", True, 0, 2)]
    assert re.search(r"constexpr int NB_LO = NBR == 4 \? 3 : \(NBR == 6 \? 4 : 5\)", kernel) and ae.NB_LO == {4: 3, 6: 4, 7: 5}
    assert re.search(r"if \(MAXLEN == 320\) stage1\(std::integral_constant<int, 7>\{\}\);\s+// .*\n\s+else if \(!has_long && qlen \+ short_tlen_max - 1 <= 256\) stage1\(std::integral_constant<int, 4>", kernel)
    # the group partition of faqcs_create
    capi_src = open(os.path.join(ROOT, "faqcs_amd", "csrc", "faqcs_capi.hip")).read()
    assert "if (p->n_adapters > FAQCS_ADAPTER_GROUP || c->adapter_longest > FAQCS_ADAPTER_SINGLE_LENGTH) {" in capi_src
    assert "while (j < p->n_adapters && g.n < FAQCS_ADAPTER_GROUP && 4u * (wstart[j + 1] - g.w0) <= FAQCS_ADAPTER_TPL_CAP) {" in capi_src


def test_variant_and_partition():
    v = ae.variant
    assert v(160, 32, 128, 4096, False) == ("pair", True) and v(161, 32, 128, 4096, False) == ("256", True)
    assert v(160, 33, 128, 100, False)[0] == v(160, 32, 129, 100, False)[0] == v(160, 32, 128, 100, False, pair_on=False)[0] == v(160, 32, 128, 100, False, prefilter_on=False)[0] == "256"
    assert v(160, 32, 128, 4097, False) == ("256", False) and v(160, 3, 40, 12, True) == ("grouped_256", True)
    for lo, w in zip((0, 257, 321, 1025, 4097, 8193, 16385), ae.WIDTHS):
        assert v(max(lo, 1), 3, 40, 12, False, pair_on=False)[0] == str(w) == v({256: 256, 320: 320, 1024: 1024, 4096: 4096, 8192: 8192, 16384: 16384, 32768: 32767}[w], 3, 40, 12, False)[0]
    assert ae.partition([30] * 64) is None and ae.partition([8192]) is None
    assert ae.partition([30] * 65) == [(0, 64, 30, 256), (64, 1, 30, 4)]
    assert ae.partition([8193]) == [(0, 1, 8193, 1028)] and ae.partition([32767, 40]) == [(0, 1, 32767, 4096), (1, 1, 40, 8)]
    assert ae.partition([8193, 8642, 8641, 32767, 40]) == [(0, 3, 8642, 3196), (3, 1, 32767, 4096), (4, 1, 40, 8)]
    assert 4 * 5 * ae.plane_words(7000) == 4380 > ae.TPL_CAP >= 4 * 5 * ae.plane_words(6500) == 4080


def test_every_edge_is_claimed_and_every_claim_holds(cases):
    assert len({c.name for c in cases}) == len(cases), "two cases share a name"
    table, lost, _ = ae.coverage(cases)
    assert not lost, "claims that do not hold: %s" % lost
    missing = sorted(e for e, v in table.items() if not v)
    assert not missing, "edges no case reaches: %s" % missing
    assert len(table) >= 140 and all(e in ae.EDGES for c in cases for e in c.claims)
    assert {c.family for c in cases} == set(ae.FAMILIES), "a family without a case"
    assert sum(c.n_reads() for c in cases) <= 2000, "a family has tens of reads, not thousands"
    for c in cases:                                            # the sizes the catalogue keeps to
        longest = sorted(len(r) for sub in c.subs for seg in sub for r in seg)
        assert all(n <= 321 for n in longest[:-1]) or c.name == "dispatch_by_the_longest_read_long" or c.family == "groups", c.name
        assert max(c.tlens) <= 129 or max(longest) <= 320, "%s: a long target meets reads of at most 320 bases" % c.name
        assert set(c.exclude) <= {"no_pair"} and (("no_pair" in c.exclude) != c.takes_pair()), c.name
        assert np.float32(c.opt().filterAdapterMismatchRate) == np.float32(float(c.args[c.args.index("--rate") + 1] if "--rate" in c.args else "0.2")), c.name


def test_the_float32_thresholds_the_catalogue_names():
    for n, (thr, exact) in ae.FLOAT_THR.items():
        assert ae.threshold("0.6", n) == thr and ae.threshold("0.6", n, "threshold_in_double") == exact, n
    assert ae.threshold("0.35", 180) == 116 and ae.threshold("0.35", 180, "threshold_in_double") == 117
    assert ae.threshold("0.2", 40) == 32 and ae.threshold("0.2", 20) == 16 and ae.threshold("0.2", 1) == 0


def test_every_mutant_is_told_apart(cases):
    """A kernel wrong in one of these ways would fail the catalogue: for every wrong variant of the model some case expects other records or counters."""
    small = [c for c in cases if c.family not in ("uncached", "groups", "dispatch")]    # (the mutants are told apart on the small families)
    for mutant in ae.MUTANTS:
        told = []
        for c in small:
            e, m = c.expected(), ae.run_model(c, mutant)
            if any((a != b).any() for a, b in zip(e["results"], m["results"])) or (e["stats"] != m["stats"]).any():
                told.append(c.name)
                break
        assert told, "no case tells the mutant %s from the model" % mutant


def _align_oracle(lib, q, t):
    score, a, b = C.c_int(0), C.c_int(-1), C.c_int(-1)
    qa, ta = np.frombuffer(q, np.uint8), np.frombuffer(t, np.uint8)
    have = lib.faqcs_oracle_align(qa.ctypes.data if len(qa) else None, len(qa), ta.ctypes.data, len(ta), C.byref(score), C.byref(a), C.byref(b))
    return have, score.value, a.value, b.value


def test_model_equals_oracle_pair_by_pair(cases):
    from oracle_engine import load_oracle

    lib = load_oracle()
    n = 0
    for c in cases:
        if c.family in ("uncached", "groups"):                 # (the long targets are held to the oracle on the whole cases, below)
            continue
        for i in c.expected()["info"]:
            if i.bad:
                continue
            for h in i.hits:
                have, score, a, b = _align_oracle(lib, i.seq, c.lib[h.t][1].encode())
                assert bool(have) == h.any, (c.name, i.index, h.t)
                if have and not h.stale:
                    assert (score, a, b) == (h.score, h.start, h.stop), "%s: read %d target %d: oracle %s model %s" % (c.name, i.index, h.t, (score, a, b), (h.score, h.start, h.stop))
                    n += 1
            if i.credit:
                mask = np.array(i.mask, np.uint8)
                st, ln = C.c_uint32(), C.c_uint32()
                lib.faqcs_oracle_find_mask_range(mask.ctypes.data, len(mask), C.byref(st), C.byref(ln))
                assert (st.value, ln.value) == (i.first, i.second), (c.name, i.index)
    assert n > 500
    rng = np.random.Generator(np.random.PCG64(7))
    for _ in range(300):                                        # find_mask_range alone, on masks of a few runs
        mask = np.repeat(rng.integers(0, 2, 12), rng.integers(1, 6, 12)).astype(np.uint8)
        st, ln = C.c_uint32(), C.c_uint32()
        lib.faqcs_oracle_find_mask_range(mask.ctypes.data, len(mask), C.byref(st), C.byref(ln))
        assert (st.value, ln.value) == ae.find_mask_range([bool(x) for x in mask])


def compare_with_oracle(case, e):
    """the whole case through the OracleEngine -> (results per submission, counters) or the error; the model's predicted fields and adapter_stats
    are held to them"""
    from oracle_engine import OracleEngine

    from faqcs_amd.engine import FaqcsError

    ora = OracleEngine(case.opt(), case.R, case.in_off)
    try:
        error, results = 0, []
        try:
            for k in range(len(case.subs)):
                results.append(ora.process(*driver.pack_segments(case.records(k))))
        except FaqcsError as x:
            error = x.code
        assert error == e["error"], "%s: the oracle's error %d, the model's %d" % (case.name, error, e["error"])
        if error:
            return None, None
        for k, (got, want) in enumerate(zip(results, e["results"])):
            check_fields(got, want, "%s: submission %d: oracle" % (case.name, k))
        lay = capi.python_layout(case.R, len(case.lib))
        o, n = lay["adapter_stats"]
        counters = ora.counters()
        assert (counters[o:o + n] == e["stats"]).all(), "%s: adapter_stats: oracle %s model %s" % (case.name, counters[o:o + n], e["stats"])
        return results, counters
    finally:
        ora.close()


def check_fields(got, want, what):
    """the fields the model predicts: adapter, FAQCS_F_ADAPTER, FAQCS_F_VALID, and start / len of a read that is not filtered"""
    mask = ae.F_ADAPTER | ae.F_VALID | ae.F_ERR_BASE
    bad = np.nonzero((got["adapter"] != want["adapter"]) | ((got["flags"] & mask) != (want["flags"] & mask)) |
                     (((want["flags"] & ae.F_VALID) != 0) & ((got["start"] != want["start"]) | (got["len"] != want["len"]))))[0]
    assert len(bad) == 0, "%s: read %d (the first of %d that differ): got %s, the model %s" % (what, bad[0], len(bad), got[bad[0]], want[bad[0]])


def test_model_equals_oracle_on_every_case(cases):
    for c in cases:
        compare_with_oracle(c, c.expected())
    assert sum(1 for c in cases if c.expected()["error"]) >= 2
