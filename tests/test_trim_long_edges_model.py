"""The catalogue of tests/trim_long_edges.py without a GPU: its restated constants against their sources by regex, its coverage table (every
edge claimed, every claim of a case true, every case in a family), the exclusions by name and counted, the plain model against the oracle on
every case -- the per-read results of every submission and the whole counter block, bit for bit, and the expected errors; the oracle stands
alone for the window family --, the piecewise model against the plain one and each of its mutants against the case that tells it apart, and
the float search of the composition bins over every length a long read can have."""
import os
import re

import numpy as np
import pytest

import trim_edges as te
import trim_long_edges as tl
from faqcs_amd import _capi as capi
from faqcs_amd import driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return tl.all_cases()


def test_restated_constants_equal_the_sources():
    text = {}
    for name, (path, rx) in tl.CONSTANT_SOURCES.items():
        src = text.setdefault(path, open(os.path.join(ROOT, path)).read())
        m = re.search(rx, src)
        assert m, "%s: %s no longer states it as %r" % (name, path, rx)
        assert getattr(tl, name) == int(m.group(1)), name
    for what, (path, rx) in tl.STATEMENT_SOURCES.items():
        src = text.setdefault(path, open(os.path.join(ROOT, path)).read())
        assert re.search(rx, src), "%s: %s no longer says so (%r)" % (what, path, rx)
    assert tl.LA_BLOCKS_PER_CU == 1 and tl.ROUND == 4 * tl.PIECE and tl.LA_TILE == 8 * tl.PIECE
    assert tl.full_waves(256) == 8192 and tl.trim_long_grid(8193, 256) == 2048 and tl.trim_long_grid(5, 256) == 2 and tl.accumulate_grid(17, 256) == 2 and tl.accumulate_grid(10 ** 6, 256) == 256
    assert (tl.NQ, tl.NBASE, tl.E_QUALITY, tl.F_ADAPTER) == (capi.NQ, capi.NBASE, capi.E_QUALITY, capi.F_ADAPTER)
    from faqcs_amd import options

    built_in = [s for _, s in options.BUILTIN_ADAPTERS]
    assert tl.ADAPTER_3.decode() in built_in and tl.ADAPTER_5.decode() in built_in
    assert te.layout(tl.MAX_READ_LENGTH) == capi.python_layout(tl.MAX_READ_LENGTH, 0)


def test_every_edge_is_claimed_and_every_claim_holds(cases):
    assert len({c.name for c in cases}) == len(cases), "two cases share a name"
    table, lost, _ = tl.coverage(cases)
    assert not lost, "claims that do not hold: %s" % lost
    missing = sorted(e for e, v in table.items() if not v)
    assert not missing, "edges no case reaches: %s" % missing
    assert len(table) >= 150 and all(e in tl.EDGES for c in cases for e in c.claims)
    assert {c.family for c in cases} == set(tl.FAMILIES) and all(getattr(c, "family", None) in tl.FAMILIES for c in cases), "a case is in no family"
    assert all(c.claims for c in cases), "a case claims no edge"
    prefix = dict(walk="walk:", terminal_n="tn:", poly_n="pn:", fields="fd:", transitions="tr:", tiles="tl:", waves="wv:", window="wd:")
    for c in cases:
        assert all(e.startswith(prefix[c.family]) for e in c.claims), c.name


def test_sizes_stay_within_the_budget(cases):
    """below about 4 M bases and 30 000 reads per family; waves is the exception the batch sizes force: W - 1, W, W + 1, 2 W + 1 and 3 W + 1 are 8 W + 2 reads"""
    for f in tl.FAMILIES:
        cs = [c for c in cases if c.family == f]
        reads, bases = sum(c.n_reads() for c in cs), sum(len(r[1]) for c in cs for sub in c.subs for seg in sub for r in seg)
        assert bases <= 4000000, (f, bases)
        assert reads <= (8 * tl.full_waves(256) + 2 + 13 if f == "waves" else 30000), (f, reads)
    assert sum(1 for c in cases if c.R == tl.MAX_READ_LENGTH) <= 30


def test_exclusions_are_by_name_and_counted(cases):
    assert sorted(tl.EXCLUSIONS) == ["long_accumulate:flush_after_65535_increments", "poly_n:whole_N_piece_narrower_than_64", "walk:first_re-arm_after_step_0"]
    assert all(tl.EXCLUSIONS.values()) and not set(tl.EXCLUSIONS) & set(tl.EDGES)
    assert [f for f in tl.FAMILIES if tl.FAMILY_REFERENCE[f] == "oracle"] == ["window"]
    assert all(c.oracle == (c.family == "window") for c in cases)
    # the flush that stays untested: no batch comes near 65 535 reads per block and tile
    assert max(len([r for seg in sub for r in seg]) for c in cases for sub in c.subs) / tl.accumulate_grid(10 ** 9, 256) < 65535 - tl.LA_NW


def test_error_cases_expect_an_error_and_no_others(cases):
    for c in cases:
        assert (c.expected()["error"] == tl.E_QUALITY) == c.error, c.name
    assert sum(c.error for c in cases) == 1


@pytest.mark.parametrize("family", tl.FAMILIES)
def test_model_equals_oracle_on_every_case(family):
    """(for the window family the oracle is the reference itself: there the test holds the results to what the case says of them, through its edges)"""
    from oracle_engine import OracleEngine

    from faqcs_amd.engine import FaqcsError

    for c in tl.family_cases(family):
        e = c.expected()
        if c.oracle:
            assert e["error"] == 0 and all(pred(c.ctx()) for name, pred in tl.EDGES.items() if name in c.claims), c.name
            continue
        ora = OracleEngine(c.opt(), c.R, c.in_off)
        lay = te.layout(c.R)
        got_error, results = 0, []
        try:
            for sub in c.subs:
                results.append(ora.process(*driver.pack_segments(sub)))
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


@pytest.mark.parametrize("family", [f for f in tl.FAMILIES if tl.FAMILY_REFERENCE[f] == "model"])
def test_piecewise_model_equals_the_model(family):
    for c in tl.family_cases(family):
        d = tl.pieces_differ(c, tl.pieces(c))
        assert d is None, "%s: the piecewise model: %s" % (c.name, d)


def test_every_mutant_is_caught_by_its_case(cases):
    assert len(tl.MUTANTS) >= 10
    names = {c.name for c in cases}
    for m, (what, name) in tl.MUTANTS.items():
        assert name in names, m
        assert tl.caught(m) is not None, "the case %s does not tell the mutant %r (%s) from the model" % (name, m, what)
    for m, (what, family) in tl.EQUIVALENT_MUTANTS.items():      # (named among the exclusions: no input can tell them apart)
        for c in tl.family_cases(family):
            assert tl.pieces_differ(c, tl.pieces(c, m)) is None, (m, c.name)


def test_grids_follow_the_compute_units():
    """the batch-size edges hold on a card with another number of compute units: the builders and the predicates take it"""
    for n_cu in (8, 304):
        for family, names in (("tiles", ("tl_batch_sizes",)), ("waves", ("wv_W-1_equal_lengths", "wv_W+1_every_4_reads"))):
            cs = [c for c in tl.family_cases(family, n_cu) if c.name in names]
            assert len(cs) == len(names)
            table, lost, _ = tl.coverage(cs)
            assert not lost, (n_cu, lost)
            assert all(table[e] for c in cs for e in c.claims)
    assert [len(s[0]) for s in [c for c in tl.family_cases("tiles", 8) if c.name == "tl_batch_sizes"][0].subs] == [1, 15, 16, 17, 127, 128, 129, 257]


def test_composition_bins_need_no_bound_check():
    """composition_bins() writes bin trunc(norm * nG) + trunc(norm * nC) of the GC column without a bound check.  Over every length 1 025 .. 32 767 and
    every split of the read between the two, the float32 products never give more than 10 000 (the last bin)."""
    assert tl.comp_bin_search() == te.NCOMP_BIN - 1
    assert tl.comp_bin_search(1, tl.FAST_READ_LENGTH) == te.NCOMP_BIN - 1
