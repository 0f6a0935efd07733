"""The catalogue of tests/trim_edges.py without a GPU: its restated constants against their sources, its coverage table (every edge claimed,
every claim of a case true, every case in a family, the exclusions counted), and its plain model against the oracle on every case: the
per-read results of every submission and the whole counter block, bit for bit, and the expected errors."""
import os
import re

import numpy as np
import pytest

import trim_edges as te
from faqcs_amd import _capi as capi
from faqcs_amd import driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return te.all_cases()


def test_restated_constants_equal_the_sources():
    hdr = open(os.path.join(ROOT, "include", "faqcs_mi.h")).read()
    for name, rx in te.CONSTANT_SOURCES.items():
        m = re.search(rx, hdr)
        assert m, "%s: include/faqcs_mi.h no longer states it as %r" % (name, rx)
        assert getattr(te, name) == int(m.group(1)), name
    assert (te.PAD_BEFORE, te.PAD_AFTER) == (capi.ARENA_PAD_BEFORE, capi.ARENA_PAD_AFTER)
    assert [getattr(capi, n) for n in te.STAT] == list(range(len(te.STAT)))
    assert (te.F_VALID, te.F_QUAL_TRIMMED, te.F_POLY_N_SEEN, te.E_QUALITY) == (capi.F_VALID, capi.F_QUAL_TRIMMED, capi.F_POLY_N_SEEN, capi.E_QUALITY)
    filt = re.search(r"enum \{ (FAQCS_FILT_NONE = 0.*?) \};", hdr, re.S).group(1)
    assert [x.split("=")[0].strip() for x in filt.split(",")] == ["FAQCS_FILT_NONE", "FAQCS_FILT_LENGTH_PRE", "FAQCS_FILT_LENGTH_POST", "FAQCS_FILT_POLY_N", "FAQCS_FILT_AVG_Q",
                                                                  "FAQCS_FILT_LOW_COMPLEXITY"]
    assert te.RESULT_DTYPE == capi.RESULT_DTYPE and capi.F_FILTER_SHIFT == 1
    from faqcs_amd import options

    assert (te.MODE_HARD, te.MODE_BWA, te.MODE_BWA_PLUS) == (options.MODE_HARD, options.MODE_BWA, options.MODE_BWA_PLUS)
    for R in (256, 1024, 4096):
        assert te.layout(R) == capi.python_layout(R, 0)
    assert te.ROW_LAST == [52, 76, 104, 152, 252, 304] and te.ROW_FIRST == [1, 53, 77, 105, 153, 253] and te.TFA_FIRST == 305


def test_every_edge_is_claimed_and_every_claim_holds(cases):
    assert len({c.name for c in cases}) == len(cases), "two cases share a name"
    table, lost, _ = te.coverage(cases)
    assert not lost, "claims that do not hold: %s" % lost
    missing = sorted(e for e, v in table.items() if not v)
    assert not missing, "edges no case reaches: %s" % missing
    assert len(table) >= 100 and all(e in te.EDGES for c in cases for e in c.claims)
    assert {c.family for c in cases} == set(te.FAMILIES) and all(getattr(c, "family", None) in te.FAMILIES for c in cases), "a case is in no family"
    assert 100000 <= sum(c.n_reads() for c in cases) <= 200000


def test_exclusions_are_by_name_and_counted(cases):
    """No case is skipped on the device: a case that does not run under a setting says so, with its reason, and runs under another."""
    excluded = {s: sorted(c.name for c in cases if s in c.exclude) for s in te.SETTINGS}
    for c in cases:
        assert all(s in te.SETTINGS and reason for s, reason in c.exclude.items()), c.name
        assert len(c.exclude) < len(te.SETTINGS), "%s runs nowhere" % c.name
    by_family = lambda s: {f: sum(1 for c in cases if c.family == f and s in c.exclude) for f in te.FAMILIES}
    n = {f: sum(1 for c in cases if c.family == f) for f in te.FAMILIES}
    assert by_family("lds") == dict({f: 0 for f in te.FAMILIES}, long=n["long"]) == by_family("single_pass")
    assert by_family("long") == dict({f: 0 for f in te.FAMILIES}, composition=n["composition"], chunks=n["chunks"])
    assert len(excluded["long"]) == n["composition"] + n["chunks"]
    for f in te.FAMILIES:
        assert sorted(c.name for s in te.SETTINGS for c in te.cases_of(f, s, cases)) == sorted(c.name for c in cases if c.family == f for s in te.SETTINGS if s not in c.exclude)


def test_error_cases_expect_an_error_and_no_others(cases):
    for c in cases:
        assert (c.expected()["error"] == te.E_QUALITY) == c.error, c.name
    assert sum(c.error for c in cases) >= 7


def test_model_equals_oracle_on_every_case(cases):
    from oracle_engine import OracleEngine

    from faqcs_amd.engine import FaqcsError

    for c in cases:
        e = c.expected()
        ora = OracleEngine(c.opt(), c.R, c.in_off)
        lay = te.layout(c.R)
        got_error, results = 0, []
        try:
            for sub in c.subs:
                results.append(ora.process(*(te.hostile_arenas(sub, c.in_off) if c.hostile else driver.pack_segments(sub))))
        except FaqcsError as x:
            got_error = x.code
        assert got_error == e["error"], "%s: the oracle's error %d, the model's %d" % (c.name, got_error, e["error"])
        if not got_error:
            for k, (a, b) in enumerate(zip(results, e["results"])):
                bad = np.nonzero(a != b)[0]
                assert len(bad) == 0, "%s: submission %d read %d: oracle=%s model=%s" % (c.name, k, bad[0], a[bad[0]], b[bad[0]])
            c1, c2 = ora.counters(), e["counters"]
            bad = np.nonzero(c1 != c2)[0]
            if len(bad):
                k = int(bad[0])
                name = [nm for nm, v in lay.items() if nm != "total" and v[0] <= k < v[0] + v[1]][0]
                raise AssertionError("%s: %d counters differ, first %s[%d]: oracle=%d model=%d" % (c.name, len(bad), name, k - lay[name][0], c1[k], c2[k]))
        ora.close()


def test_float_searches_behind_the_catalogue():
    """The lengths the catalogue fixes are what the searches find: where the float32 threshold of --lc is not the exact one, the 70 composition
    pairs up to 304 bases, and an --avg_q value whose float32 rule is not the exact one."""
    for text, want in (("0.2", [15, 30, 60, 120, 240, 255, 480, 510, 960, 1020]), ("0.4", [15, 30, 60, 120, 240, 255, 480, 510, 960, 1020])):
        assert [n for n in range(1, 1025) if te.lc_thr(n, te.f32(float(text))) != te.lc_thr_exact(n, text)] == want
    diff = [n for n in range(1, 1025) if te.lc_thr(n, te.f32(0.75)) != te.lc_thr_exact(n, "0.75")]
    assert len(diff) == 27 and set(diff) >= {28, 56, 60, 112, 120, 224, 240, 252}
    low = te.comp_low_pairs(304)
    assert len(low) == 70 and {(75, 15), (75, 30), (150, 15), (150, 30)} <= set(low)
    for a, (kind, lengths) in te.AVGQ_DIFF.items():
        assert all(te.avg_pass_sum(n, float(te.f32(float(a))), 33) != te.avg_pass_sum_exact(n, a, kind) for n in lengths), a
    for a in ("25", "12.5"):
        assert all(te.avg_pass_sum(n, float(a), 33) == te.avg_pass_sum_exact(n, a, "typed") for n in range(1, 1025)), a
