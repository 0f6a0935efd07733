"""The catalogue of tests/pair_edges.py without a GPU: its restated constants against the sources, its coverage table (every edge reached,
every claim of a case true), and every case through the host statements (faqcs_pair_host, faqcs_render_pair_host).  Cases of at most
5 000 pairs are held to the numpy models (driver.pair_model, driver.render_pair_model) and, where the route is the pair call's own, to the
existing single-batch statement on the joined batch (pair_cases.joined_files); the models are loops, so the big cases hold the host
statements to the catalogue's own vectorised expectations and to the model on their first and last 2 000 records."""
import os
import re

import numpy as np
import pytest

import pair_cases as pcs
import pair_edges as pg
import render_cases as rc
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_PAIRS = 5000
ENDS = 2000


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.fixture(scope="module")
def cases():
    return pg.all_cases()


def settings(case):
    """(options, input offset, parameters) of a case's engine arguments"""
    args = pg.ARG_SETS[case.args]
    opt = parse_args(["-1", "a", "-2", "b", "-d", "y"] + args)
    return opt, rc.in_offset(args), capi.ParamsHolder(opt, capi.MAX_READ_LENGTH, rc.in_offset(args))


def test_restated_constants_equal_the_sources():
    csrc = os.path.join(ROOT, "faqcs_amd", "csrc")
    assert set(pg.CONSTANT_SOURCES) == {"PAIR_TILE", "CAND_TILE", "SCAN_THREADS", "VOID_BLOCKS_PER_CU", "DEFAULT_CU"}
    for name, (fn, rx) in pg.CONSTANT_SOURCES.items():
        m = re.search(rx, open(os.path.join(csrc, fn)).read())
        assert m, "%s: %s no longer states it as %r" % (name, fn, rx)
        v = int(np.prod([int(g) for g in m.groups()]))
        assert getattr(pg, name) == v, "%s: the catalogue says %d, %s says %d" % (name, getattr(pg, name), fn, v)
    wave = int(re.search(r"#define\s+FAQCS_WAVE\s+(\d+)", open(os.path.join(csrc, "faqcs_dev.h")).read()).group(1))
    rpt = int(re.search(r"TILE_RPT = (\d+)", open(os.path.join(csrc, "faqcs_pack_common.h")).read()).group(1))
    assert (pg.WAVE, pg.PAIRS_PER_THREAD * 2, pg.CAND_TILE, pg.SCAN_THREADS, pg.VEC) == (wave, rpt, 2 * 512, 1024, 16)
    assert re.search(r"for \(uint32_t o = 0; o < len; o \+= %d\)" % pg.VEC, open(os.path.join(csrc, "faqcs_pair_kernel.hip")).read())
    assert (pg.F_VALID, pg.ROUTE_NOWHERE, pg.FILES) == (capi.F_VALID, capi.ROUTE_NOWHERE, pcs.FILES)
    assert (pg.QC1, pg.QC2, pg.UNPAIRED, pg.DISCARD) == (capi.FILE_QC1, capi.FILE_QC2, capi.FILE_UNPAIRED, capi.FILE_DISCARD)
    assert pg.ARG_SETS["default"] == [] and all(a in pg.ARG_SETS.values() for a in (["--replace_to_N_q", "15", "--out_ascii", "64"], ["--ascii", "64"]))


def test_every_edge_is_reached_and_every_claim_holds(cases):
    table, per_case = pg.coverage(cases)
    assert len(per_case) == len(cases), "two cases share a name"
    missing = sorted(k for k, v in table.items() if not v)
    assert not missing, "edges no case reaches: %s" % missing
    assert set(table) == pg.required() and len(table) >= 400
    for case in cases:
        lost = [e for e in case.claims if e not in per_case[case.name]]
        assert not lost, "%s claims %s and does not reach it" % (case.name, lost)
        assert all(e in table for e in case.claims), case.name
    # what the families promise of every case of theirs
    for case in cases:
        c = case.ctx()
        if case.family == "tiles" and case.m[0].total:
            assert (case.m[0].res["len"][:case.n] != case.m[1].res["len"][:case.n]).mean() > 0.8, case.name  # paired_base_length tells the mates apart
        if case.family == "ids" and not case.name.startswith(("one_byte_", "suffix_against_", "two_id_bytes_", "odd_byte_")):
            assert c.mismatch == 0, "%s: pair %d does not match" % (case.name, c.n_pairs)
        if case.family == "ids":
            assert case.m[0].def_pos[0] == 0 and int(case.m[0].def_pos[-1]) + int(case.m[0].def_len[-1]) == len(case.m[0].text)


def test_id_entries_one_by_one(cases):
    """Every defline of the id cases: the catalogue's vectorised id lengths and verdicts are driver.parse_id's, entry by entry."""
    n = 0
    for case in cases:
        if case.deflines is None:
            continue
        c = case.ctx()
        for i, (a, b) in enumerate(zip(*case.deflines)):
            ia, ib = driver.parse_id(a), driver.parse_id(b)
            assert (int(c.id_len[0][i]), int(c.id_len[1][i]), bool(c.same[i])) == (len(ia), len(ib), ia == ib), (case.name, i, a, b)
            n += 1
    assert n >= 1300
    P = driver.parse_id
    assert (P(b"ab//"), P(b"ab/:"), P(b"ab-1"), P(b"ab01"), P(b"a/1/2"), P(b"ab cd/1"), P(b"7"), P(b"/1"), P(b"a\xa0b c"), P(b"a\x00b/1")) == (
        b"ab//", b"ab/:", b"ab-1", b"ab01", b"a/1", b"ab", b"7", b"", b"a\xa0b", b"a\x00b")


def check_pair(lib, case, small):
    c = case.ctx()
    route, info = pcs.pair_host(lib, case, with_res=case.routed)
    assert info == c.info, case.name
    if case.routed:
        assert (route == c.pair_route).all(), case.name
    if small:
        m_route, m_info = driver.pair_model(*case.model_mates())
        assert m_info == info and (m_route is None or (m_route == route).all()), case.name
    if case.routed:  # check only: the same verdict, zero counters, no route
        for with_route in (True, False):
            r0, i0 = pcs.pair_host(lib, case, with_res=False, with_route=with_route)
            assert r0 is None and i0 == dict(c.info, paired_read_number=0, paired_base_length=0, n_one_valid=0, n_none_valid=0), case.name
    return route


def check_files(lib, case, small):
    c = case.ctx()
    opt, in_off, holder = settings(case)
    joined = pcs.joined_files(lib, holder, _Joinable(case), c.route) if small and case.route is None and case.n_pairs == case.n and case.m[0].n == case.m[1].n else None
    for f in case.files:
        fc = c.files[f]
        if case.overflow:
            for cap in ((fc.n_bytes - 1, 0) if fc.n_bytes else ()) if case.overflow is True else (case.capacity,):
                o = pcs.render_pair_host(lib, holder, case, f, c.route, case.n_pairs, capacity=cap)
                assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (fc.n_bytes, fc.n_reads, 1), (case.name, f, cap)
                rc.assert_untouched(o, fc.n_bytes, fc.n_reads, overflow=True)
            if case.overflow == "only":
                continue
        o = pcs.render_pair_host(lib, holder, case, f, c.route, case.n_pairs, capacity=fc.n_bytes if case.overflow else case.capacity)
        text, roff, ridx = pcs.rendering(o)
        assert (o["n_bytes"], o["n_reads"]) == (fc.n_bytes, fc.n_reads), (case.name, f)
        assert (roff == fc.offset).all() and (ridx == fc.rec_index).all(), (case.name, f)
        rc.assert_untouched(o, fc.n_bytes, fc.n_reads)
        if fc.n_reads == 0:
            assert o["rec_offset"][0] == 0
        if small:
            model = driver.render_pair_model(opt, in_off, f, *case.model_mates(), c.route, case.n_pairs)
            rc.assert_rendering(o, model, "%s file %d" % (case.name, f))
            if joined is not None:
                rc.assert_rendering(o, joined[f], "%s file %d against the joined batch" % (case.name, f))
        else:
            # the first ENDS records, and the records of the last pairs
            k = min(ENDS, fc.n_reads)
            if k:
                head = driver.render_pair_model(opt, in_off, f, *case.model_mates(), c.route, int(fc.rec_index[k - 1] >> 1) + 1)
                assert head[0][:int(fc.offset[k])].tobytes() == text[:int(fc.offset[k])].tobytes(), (case.name, f)
            lo = case.n_pairs - ENDS // 2
            tail = driver.render_pair_model(opt, in_off, f, *case.model_mates(lo=lo), c.route[lo:], case.n_pairs - lo)
            assert len(tail[0]) == 0 or tail[0].tobytes() == text[-len(tail[0]):].tobytes(), (case.name, f)


class _Joinable:
    """a case as pair_cases.joined_files reads it: r1 / r2 as (defline, bases, qualities) and m"""

    def __init__(self, case):
        self.n, self.m = case.n, case.m
        self.r1, self.r2 = ([(bytes(m.text[int(m.def_pos[i]):int(m.def_pos[i]) + int(m.def_len[i])]), bytes(m.seq[int(m.offset[i]):int(m.offset[i + 1])]),
                              bytes(m.qual[int(m.offset[i]):int(m.offset[i + 1])])) for i in range(case.n)] for m in case.m)


FAMILIES = ("ids", "tiles", "scan", "source", "gather")


@pytest.mark.parametrize("family", FAMILIES)
def test_host_statements_equal_the_models(lib, cases, family):
    """Every case of at most 5 000 pairs: route, info, text, rec_offset, rec_index and canaries of the host statements against the numpy
    models, the catalogue's expectations and (where results route the pairs) the single-batch statement on the joined batch."""
    n = 0
    for case in (c for c in cases if c.family == family):
        small = case.n <= MODEL_PAIRS
        if case.pair:
            check_pair(lib, case, small)
        if case.render:
            check_files(lib, case, small)
        n += 1
    assert n >= {"ids": 200, "tiles": 30, "scan": 15, "source": 15, "gather": 40}[family]


def test_shadow_mates_swapped_arenas_change_every_record(lib, cases):
    """What the catalogue claims of the mates that share offsets: rendered from the other mate's arrays, every record of every file differs."""
    case = [c for c in cases if c.name == "shadow_mates"][0]
    opt, in_off, holder = settings(case)
    a, b = case.model_mates()
    for f in case.files:
        x = driver.render_pair_model(opt, in_off, f, a, b, case.route, case.n_pairs)
        y = driver.render_pair_model(opt, in_off, f, dict(a, text=b["text"], seq=b["seq"], qual=b["qual"]), dict(b, text=a["text"], seq=a["seq"], qual=a["qual"]), case.route, case.n_pairs)
        assert (x[1] == y[1]).all() and len(x[2]) > 50
        for k in range(len(x[2])):
            assert x[0][x[1][k]:x[1][k + 1]].tobytes() != y[0][y[1][k]:y[1][k + 1]].tobytes(), (f, k)


@pytest.mark.parametrize("name", ("big_clean", "big_bad_at_3", "big_bad_beyond_round", "big_bad_last"))
def test_big_cases_host_statements_equal_the_expectations(lib, cases, name):
    """The cases beyond one round of the finishing block: the host statements against the catalogue's vectorised expectations -- verdict,
    n_pairs, route, counters; record count, rec_offset, rec_index -- and the bytes of the first and last 2 000 records against the model."""
    case = [c for c in cases if c.name == name][0]
    assert case.n == pg.big_size() > MODEL_PAIRS
    check_pair(lib, case, False)
    check_files(lib, case, False)
