"""The catalogue of tests/trim_tfa_edges.py without a GPU: its restated constants against their sources by regex, the plans of the shapes family
against trim_plan() itself (tools/trim_plan_check.cpp) and every compiled variant reached, its coverage table (every edge claimed, every claim
of a case true, every case in a family), the exclusions by name and counted, the batch-size edges at 8 and 304 compute units, the plain model
against the oracle on every case -- the per-read results of every submission and the whole counter block, bit for bit; the oracle stands alone for the window family --, the repeats
identity that the Tiled submissions rest on, the lanewise model against the plain one and each of its mutants against the case that tells
it apart."""
import os
import re
import subprocess

import numpy as np
import pytest

import trim_dispatch_cases as td
import trim_edges as te
import trim_tfa_edges as tf
from faqcs_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return tf.all_cases()


def test_restated_constants_equal_the_sources():
    text = {}
    for name, (path, rx) in tf.CONSTANT_SOURCES.items():
        src = text.setdefault(path, open(os.path.join(ROOT, path)).read())
        m = re.search(rx, src)
        assert m, "%s: %s no longer states it as %r" % (name, path, rx)
        got, want = tuple(int(g) for g in m.groups()), getattr(tf, name)
        if isinstance(want, dict):      # REG_FLUSH_EVERY: LPR == 16 ? 3 : (LPR == 8 ? 7 : (LPR == 4 ? 15 : 1)), the last for 32 and 64 lanes
            want = (16, want[16], 8, want[8], 4, want[4], want[32])
        assert got == (want if isinstance(want, tuple) else (want,)), name
    for what, (path, rx) in tf.STATEMENT_SOURCES.items():
        src = text.setdefault(path, open(os.path.join(ROOT, path)).read())
        assert re.search(rx, src), "%s: %s no longer says so (%r)" % (what, path, rx)
    assert tf.REG_FLUSH_EVERY[64] == tf.REG_FLUSH_EVERY[32] == 1 and tf.COMP_FLUSH_EVERY == 15 and tf.COMP_ROUND == 4096
    assert tf.TFA_FLUSH_EVERY == {4: 255, 8: 127} and tf.HQ8_EVERY * 8 <= 255 < 4 * tf.HQ8_EVERY * 8
    assert [s[1] for s in tf.SHAPES] == [64, 76, 104, 128, 152, 160, 208, 256, 320, 512, 768, 1024] and [s[2] for s in tf.SHAPES] == [16, 19, 13, 16, 19, 20, 13, 16, 10, 16, 12, 16]
    # one iteration, from expected_plan: 131 072 reads up to 320 bases, 65 536 for 512 / 768, 131 072 for 1 024 on 256 compute units
    assert [tf.iteration(s, 256) for s in tf.SHAPES] == [131072] * 9 + [65536, 65536, 131072]
    # the 6-bit fields: 60 / 56 / 48 / 32 / 32 of 63 as the schedule stands, 64 with a spill one iteration late, 64 without the spill in front of read 32
    assert [tf.field_peak(l, 1 << 30, 1) for l in tf.LPR_CLASSES] == [60, 56, 48, 32, 32]
    assert all(tf.field_peak(l, 1 << 30, 1, late=1) > 63 for l in (4, 8, 16, 32)) and tf.field_peak(64, 65, 1, mid_chunk=False) > 63
    assert (tf.te.NQ, tf.te.NBASE) == (capi.NQ, capi.NBASE) and te.layout(1024) == capi.python_layout(1024, 0)
    from faqcs_amd import options

    assert tf.ADAPTER_3.decode() in [a for _, a in options.BUILTIN_ADAPTERS] and tf.F_ADAPTER == capi.F_ADAPTER
    assert tf.seam_ms(tf.SHAPES[8]) == [1, 16, 31] and tf.seam_ms(tf.SHAPES[11]) == [1, 16, 32, 48, 63] and tf.borders(tf.SHAPES[10]) == [12, 192, 384, 576, 756]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("trim_tfa_plan") / "trim_plan_check")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", path, os.path.join(ROOT, "tools", "trim_plan_check.cpp")], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return path


def test_shapes_family_plans_are_trim_plans(plan_exe):
    """kernel, C, LPR, NW, windowed, ext and grid of every submission of the shapes family, from trim_plan() itself, equal expected_plan; the four option sets
    reach every compiled (WINDOWED, GENERIC) variant of every shape, and at 512 / 768 / 1 024 bases the requests that have no variant run the superset"""
    import test_trim_plan as tp

    cs = tf.family_cases("shapes")
    rows = [(c, k, s) for c in cs for k in range(len(c.subs)) for s in tf.SETTINGS]
    got = tp.plans(plan_exe, [(td.option_fields(c.args), tf.sub_longest(c.subs[k]), tf.sub_n(c.subs[k]), c.n_cu, tf.switches(s)) for c, k, s in rows])
    reached = set()
    for (c, k, s), p in zip(rows, got):
        assert p == c.plan(k, s), (c.name, k, s)
        if s == "single_pass" or tf.sub_longest(c.subs[k]) > tf.LDS_LAST:
            assert p["kernel"] == c.kernel(k), (c.name, k, s)
        if p["kernel"] == "trim_filter_accumulate":
            sh = tf.shape_of(tf.sub_longest(c.subs[k]))
            assert (p["C"], p["LPR"], p["NW"]) == sh[2:5]
            reached.add((p["C"], p["LPR"], p["windowed"], p["ext"]))
    assert reached == tf.compiled_variants() and len(reached) == 9 * 4 + 2 + 1 + 1
    # the requests as the option sets make them, and what runs
    for w, runs in ((512, {(0, 0): (0, 0), (1, 0): (1, 1), (0, 1): (1, 1), (1, 1): (1, 1)}), (768, {k: (1, 1) for k in ((0, 0), (1, 0), (0, 1), (1, 1))}), (1024, {k: (1, 1) for k in ((0, 0), (1, 0), (0, 1), (1, 1))})):
        for nm, extra in tf.OPTION_SETS.items():
            o = td.option_fields(["--min_L", "10", "--lc", "0.85"] + extra)
            request = (int(bool(o["trim5"])), int(bool(o["avgq_on"])))
            p = [c for c in cs if c.name == "sh_%d_%s" % (w, nm)][0].plan(1, "single_pass")
            assert (p["windowed"], p["ext"]) == runs[request], (w, nm)


def test_every_edge_is_claimed_and_every_claim_holds(cases):
    assert len({c.name for c in cases}) == len(cases), "two cases share a name"
    table, lost, _ = tf.coverage(cases)
    assert not lost, "claims that do not hold: %s" % lost
    missing = sorted(e for e, v in table.items() if not v)
    assert not missing, "edges no case reaches: %s" % missing
    assert len(table) >= 70 and all(e in tf.EDGES for c in cases for e in c.claims)
    assert {c.family for c in cases} == set(tf.FAMILIES) and all(getattr(c, "family", None) in tf.FAMILIES for c in cases), "a case is in no family"
    assert all(c.claims for c in cases), "a case claims no edge"
    for c in cases:
        assert all(e.startswith(tf.PREFIX[c.family]) for e in c.claims), c.name
    # every shape has a context case narrower than it
    assert sorted(tf.shape_of(c.R)[1] for c in cases if "ln:context_narrower_than_the_shape" in c.claims) == [s[1] for s in tf.SHAPES]


def test_settings_select_the_cases_and_skip_none(cases):
    """natural: every batch has a read past 304 bases, or the case runs --replace_to_N_q; the rest runs under FAQCS_TRIM_LDS=0.  Counted, so that a case cannot
    move silently"""
    by = {s: [c for c in cases if c.setting() == s] for s in tf.SETTINGS}
    assert len(by["natural"]) + len(by["single_pass"]) == len(cases)
    for c in by["natural"]:
        assert c.opt().replace_to_N_q or all(tf.sub_longest(s) > tf.LDS_LAST for s in c.subs if tf.sub_longest(s)), c.name
        assert all(c.plan(k, "natural")["kernel"] == c.kernel(k) for k in range(len(c.subs)) if c.kernel(k)), c.name
    assert all(c.family in ("replace", "window") and c.setting() == "natural" for c in cases if c.opt().replace_to_N_q) and len([c for c in cases if c.family == "replace"]) == 5
    assert {f: len([c for c in by["natural"] if c.family == f]) for f in tf.FAMILIES} == dict(shapes=13, seams=0, lengths=4, ns=0, transitions=0, replace=5, sums=1, chunks=3, spills=2, window=2)
    assert len(cases) == 110


def test_sizes_stay_within_the_budget(cases):
    """what the model reads stays small (periods, not tiled batches); the device sees the iteration counts the issue names and no more"""
    for f in tf.FAMILIES:
        cs = [c for c in cases if c.family == f]
        assert sum(len(c.ctx().reads) for c in cs) <= 10000, f
        assert sum(c.n_reads() for c in cs) <= (23000000 if f == "spills" else 2200000 if f == "chunks" else 3000), f
    big = {c.name: c.n_reads() for c in cases if c.n_reads() > 1000000}
    assert sorted(big) == ["ch_sizes", "sp_comp_narrow_16_rounds", "sp_comp_narrow_rounds", "sp_comp_wide_16_rounds", "sp_comp_wide_rounds", "sp_lpr4", "sp_lpr8"]
    assert big["sp_lpr4"] == 16 * 131072 and big["sp_comp_narrow_16_rounds"] == 16 * 128 * 4096


def test_exclusions_are_by_name_and_counted(cases):
    assert sorted(tf.EXCLUSIONS) == ["flush_block:16-bit_flush_after_FLUSH_EVERY_iterations", "walk:final_pos_3_one_below_final_pos_5"]
    assert [f for f in tf.FAMILIES if tf.FAMILY_REFERENCE[f] == "oracle"] == ["window"] and all(c.oracle == (c.family == "window") for c in cases)
    assert all(tf.EXCLUSIONS.values()) and not set(tf.EXCLUSIONS) & set(tf.EDGES)
    # the flush that stays untested: no launch comes near FLUSH_EVERY iterations
    for c in cases:
        for k, sub in enumerate(c.subs):
            sh = tf.shape_of(tf.sub_longest(sub))
            if sh and tf.sub_longest(sub):
                assert tf.sub_n(sub) <= 64 * tf.iteration(sh, c.n_cu) < tf.TFA_FLUSH_EVERY[sh[4]] * tf.iteration(sh, c.n_cu), (c.name, k)
    # what the closed form cannot reach: the family that walks every placement has no such read
    sm = [c for c in cases if "sm:no_read_with_final_pos_3_one_below_final_pos_5" in c.claims]
    assert len(sm) == 1 and tf.EDGES["sm:no_read_with_final_pos_3_one_below_final_pos_5"](sm[0].ctx())
    assert list(tf.EDGES)[[e.startswith("sm:") for e in tf.EDGES].index(True)].startswith("sm:bwa_plus_3")


def test_grids_follow_the_compute_units():
    """the batch-size edges hold on a card with another number of compute units: the builders and the predicates take it"""
    for n_cu in (8, 304):
        for family, names in (("chunks", ("ch_sizes",)), ("spills", ("sp_lpr4", "sp_lpr8", "sp_lpr16", "sp_lpr32", "sp_comp_narrow_rounds", "sp_comp_wide_16_rounds"))):
            cs = [c for c in tf.family_cases(family, n_cu) if c.name in names]
            assert len(cs) == len(names)
            table, lost, _ = tf.coverage(cs)
            assert not lost, (n_cu, lost)
            assert all(table[e] for c in cs for e in c.claims)
    assert [tf.iteration(tf.shape_of(w), 8) for w in (64, 512, 1024)] == [4096, 2048, 4096]
    assert tf.batch_sizes(tf.shape_of(64), 8) == [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 4353]


def test_repeats_identity():
    """every counter is a sum over reads: the block of a Tiled submission is repeats x block(period) + block(remainder), and its results are the period's results
    tiled -- held here against the plain model on the unfolded batch, at a small size, for a period that trims, filters and edits"""
    per = te.ragged(23, 40, 3) + [te.rd(b"G" * 30, te.Qs([3] * 30)), te.rd(b"ANNA" + te.rb(20, 1))]
    rest = te.ragged(5, 64, 9)
    for args in (["--min_L", "10"], ["--min_L", "1", "--replace_to_N_q", "15", "--avg_q", "12"]):
        tiled = tf.FCase("identity", args, [tf.Tiled(per, 7, rest), [rest]], ())
        flat = tf.FCase("identity_flat", args, [[per * 7 + rest], [rest]], ())
        a, b = tiled.expected(), flat.expected()
        assert a["error"] == b["error"] == 0 and (a["counters"] == b["counters"]).all()
        assert all((x == y).all() for x, y in zip(a["results"], b["results"])) and tiled.n_reads() == flat.n_reads() == 7 * 25 + 10
        # and the arenas unfold to the same bytes
        from faqcs_amd import driver

        for u, v in zip(tf.arenas(tiled.subs[0]), driver.pack_segments(flat.subs[0])):
            assert (np.asarray(u) == np.asarray(v)).all()


@pytest.mark.parametrize("family", tf.FAMILIES)
def test_model_equals_oracle_on_every_case(family):
    """(a Tiled submission goes to the oracle as the model reads it: the period and the remainder once)"""
    from oracle_engine import OracleEngine

    from faqcs_amd import driver

    for c in tf.family_cases(family):
        if c.oracle:       # (the oracle is the reference itself: the test holds its results to what the case says of them, through its edges)
            assert c.expected()["error"] == 0 and c.claims and all(tf.EDGES[e](c.ctx()) for e in c.claims), c.name
            continue
        flat = tf.FCase(c.name, c.args, [[list(seg) for seg in sub] for sub in c.subs], (), R=c.R)
        e = flat.expected()
        assert e["error"] == 0, c.name
        ora = OracleEngine(c.opt(), c.R, c.in_off)
        lay = te.layout(c.R)
        results = [ora.process(*driver.pack_segments(sub)) for sub in flat.subs]
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


@pytest.mark.parametrize("family", tf.FAMILIES)
def test_lanewise_model_equals_the_model(family):
    """lanes(): the per-read results (with the N bin of the post-trim composition, where the edit shows) and column 0 of pre_qual"""
    for c in tf.family_cases(family):
        d = tf.lanes_differ(c, tf.lanes(c))
        assert d is None, "%s: the lanewise model: %s" % (c.name, d)


def test_every_mutant_is_caught_by_its_case(cases):
    assert len(tf.MUTANTS) >= 12
    names = {c.name for c in cases}
    for m, (what, name) in tf.MUTANTS.items():
        assert name in names, m
        assert tf.caught(m) is not None, "the case %s does not tell the mutant %r (%s) from the model" % (name, m, what)


def test_every_schedule_mutant_passes_its_field(cases):
    """the schedule as it stands keeps the largest value of a field within its width on the case that aims at it; one spill, flush or round later it does not"""
    assert sorted(tf.SCHEDULE_MUTANTS) == ["comp_flush_late_narrow", "comp_flush_late_wide", "hq8_every_64", "no_mid_chunk_spill", "spill_late_lpr16", "spill_late_lpr32",
                                           "spill_late_lpr4", "spill_late_lpr8"]
    for m, (what, name) in tf.SCHEDULE_MUTANTS.items():
        for n_cu in (8, 256, 304):
            ok, mutated, width = tf.schedule_peak(m, n_cu)
            assert ok <= width < mutated, (m, n_cu, ok, mutated, width)
    assert [tf.schedule_peak("spill_late_lpr%d" % l)[0] for l in (4, 8, 16, 32)] == [60, 56, 48, 32] and tf.schedule_peak("hq8_every_64")[0] == 128
    assert tf.schedule_peak("comp_flush_late_narrow")[:2] == (61440, 65536)


def test_equivalent_mutants_equal_the_model():
    """named with their reasons: no input can tell them apart, and none of the family's cases does"""
    assert sorted(tf.EQUIVALENT_MUTANTS) == ["e_left_out_of_the_5_test", "p_le_R", "stale_prefetch"]
    for m, (why, family) in tf.EQUIVALENT_MUTANTS.items():
        for c in tf.family_cases(family):
            assert tf.lanes_differ(c, tf.lanes(c, m)) is None, (m, c.name)
    # a lane with pmax <= 0 < pmax + E exists in the family that the first of them names: the test is decided by another lane of the same read
    c = tf.case_named("sm_bwa_plus_5")
    assert any(i.w and i.w["step5"] >= 0 and len(r[1]) > 2 * tf.shape_of(len(r[1]))[2] for r, i in c.ctx().rt)
