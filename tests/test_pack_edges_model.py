"""The catalogue of tests/pack_edges.py without a GPU: its restated constants against the sources, its coverage table (every edge reached,
every claim of a case true, no case left out), and every case through the host statements (faqcs_parse_host, faqcs_render_host) against the
numpy models (driver.parse_model, driver.emit_model, driver.render_model).  The models take about a second on the million-record cases,
so they are the expected value everywhere: no case is compared with a host statement in place of its model."""
import os
import re
import types

import numpy as np
import pytest

import pack_edges as pe
import parse_cases as pc
import render_cases as rc
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_SETS = [[], ["--replace_to_N_q", "15", "--out_ascii", "64"]]  # the gathers' copy path and their EDIT path


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.fixture(scope="module")
def cases():
    return pe.all_cases()


def test_restated_constants_equal_the_sources():
    """Every structure constant of the catalogue is the product of the numbers its constexpr states (x FAQCS_WAVE where the source says so)."""
    csrc = os.path.join(ROOT, "faqcs_amd", "csrc")
    wave = int(re.search(r"#define\s+FAQCS_WAVE\s+(\d+)", open(os.path.join(csrc, "faqcs_dev.h")).read()).group(1))
    assert set(pe.CONSTANT_SOURCES) == {"PIECE", "WAVE_BYTES", "SPAN_BYTES", "TEXT_TILE", "REC_TILE", "TILE_ITEMS", "SCAN_THREADS", "GRID_BLOCKS_PER_CU", "DEFAULT_CU"}
    for name, (fn, rx) in pe.CONSTANT_SOURCES.items():
        m = re.search(rx, open(os.path.join(csrc, fn)).read())
        assert m, "%s: %s no longer states it as %r" % (name, fn, rx)
        v = int(np.prod([int(g) for g in m.groups()])) * (wave if name in pe.WAVE_CONSTANTS else 1)
        assert getattr(pe, name) == v, "%s: the catalogue says %d, %s says %d" % (name, getattr(pe, name), fn, v)
    # the gathers and the record kernels stride beyond the same number of blocks
    assert re.search(r"\(n_cu > 0 \? n_cu : %d\) \* %d" % (pe.DEFAULT_CU, pe.GRID_BLOCKS_PER_CU), open(os.path.join(csrc, "faqcs_pack_common.h")).read())
    assert pe.TAILS == pc.TAILS and pe.RESULT_DTYPE == capi.RESULT_DTYPE and pe.F_VALID == capi.F_VALID
    assert all(pe._TAIL_TEXT[t] == pc.make_text(np.random.default_rng(0), [], b"\n", t) for t in pe.TAILS)


def test_every_edge_is_reached_and_every_claim_holds(cases):
    """coverage() over EVERY case of the catalogue: each (entry point, edge) of the table has a case, each case reaches the edges it names."""
    table, per_case = pe.coverage(cases)
    assert len(per_case) == len(cases), "two cases share a name"
    missing = sorted(k for k, v in table.items() if not v)
    assert not missing, "edges no case reaches: %s" % missing
    assert set(table) == pe.required() and len(table) >= 300
    for case in cases:
        lost = [e for e in case.claims if e not in per_case[(case.kind, case.name)]]
        assert not lost, "%s %s claims %s and does not reach it" % (case.kind, case.name, lost)
        assert case.claims, "%s %s claims nothing" % (case.kind, case.name)


def test_parse_cases_host_statement_equals_the_model(lib, cases):
    """Every parse text, both values of `final`, with and without the defline arrays: faqcs_parse_host against driver.parse_model, and
    the catalogue's own reading of the rules (ParseCtx, what the predicates look at) against both."""
    n = 0
    for case in (c for c in cases if c.kind == "parse"):
        for final in (True, False):
            model = driver.parse_model(case.text, final)
            for with_def in (True, False):
                rc_, o = pc.parse_host(lib, case.text, final, with_def=with_def)
                assert rc_ == 0
                pc.assert_parse(o, case.text, final, round16=False, what="%s final=%d" % (case.name, final), model=model)
            c = pe.ParseCtx(case.text, final)
            assert c.n_reads == len(model[2]) - 1 and (c.offset == model[2]).all() and (len(c.bad) > 0) == (model[7] == capi.PARSE_E_LENGTH), case.name
            if final and not len(c.bad):
                assert model[7] == pc.TAIL_ERROR[c.tail()], case.name
            n += 1
    assert n >= 200


def test_chunked_parse_cases(lib, cases):
    parse = lambda piece, final: pc.parse_host(lib, piece, final)[1]
    chunked = [c for c in cases if c.kind == "parse" and c.cuts]
    assert len(chunked) == 2
    for case in chunked:
        rc_, whole = pc.parse_host(lib, case.text, True)
        assert pc.chunked(parse, case.text, case.cuts) == (pc.records_of(whole), whole["info"]["consumed"], whole["info"]["error"]), case.name


def defline_free(b):
    """The batch as faqcs_render_host takes it, every defline empty: a rendered record is then  \\n S \\n+\\n Q \\n."""
    return types.SimpleNamespace(n=b.n, text=np.zeros(1, np.uint8), seq=b.seq, qual=b.qual, offset=b.offset, res=b.res,
                                 def_pos=np.zeros(b.n, np.uint32), def_len=np.zeros(b.n, np.uint32))


@pytest.mark.parametrize("args", OPTION_SETS, ids=lambda a: " ".join(a) or "default")
def test_emit_cases_model_equals_the_host_statement(lib, cases, args):
    """Every emit batch: driver.emit_model against the library's host statement of the same edits and the same selection -- faqcs_render_host
    with empty deflines, whose records are the emitted windows between fixed bytes."""
    opt = parse_args(["-u", "x", "-d", "y"] + args)
    holder = capi.ParamsHolder(opt, capi.MAX_READ_LENGTH, 33)
    n = 0
    for b in (c for c in cases if c.kind == "emit"):
        es, eq, eoff, eidx = driver.emit_model(opt, 33, b.seq, b.qual, b.offset, b.res, b.keep)
        o = rc.render_host(lib, holder, defline_free(b), True, b.keep, None, capacity=2 * b.total + 5 * b.n)
        ne, nb = len(eidx), len(es)
        assert (o["n_reads"], o["n_bytes"], o["overflow"]) == (ne, 2 * nb + 5 * ne, 0), b.name
        assert (o["rec_index"][:ne] == eidx).all(), b.name
        text = o["text"][o["base"]:o["base"] + o["n_bytes"]]
        lens = np.diff(eoff.astype(np.int64))
        at = o["rec_offset"][:ne].astype(np.int64)
        assert (np.diff(o["rec_offset"][:ne + 1].astype(np.int64)) == 2 * lens + 5).all(), b.name
        flat = np.arange(nb, dtype=np.int64) - np.repeat(eoff[:-1].astype(np.int64), lens)
        assert (text[np.repeat(at + 1, lens) + flat] == es).all(), b.name
        assert (text[np.repeat(at + 4 + lens, lens) + flat] == eq).all(), b.name
        n += 1
    assert n >= 45


@pytest.mark.parametrize("args", OPTION_SETS, ids=lambda a: " ".join(a) or "default")
def test_render_cases_host_statement_equals_the_model(lib, cases, args):
    """Every render batch through render_cases.render_host against driver.render_model: the trimmed stream and the discard stream."""
    opt = parse_args(["-u", "x", "-d", "y"] + args)
    holder = capi.ParamsHolder(opt, capi.MAX_READ_LENGTH, 33)
    n = 0
    for b in (c for c in cases if c.kind == "render"):
        for with_res in (True, False):
            if not with_res and args:
                continue  # (the discard stream takes no options)
            o = rc.render_host(lib, holder, b, with_res, b.select, b.order, capacity=b.render_capacity)
            rc.assert_rendering(o, driver.render_model(opt, 33, b.text, b.def_pos, b.def_len, b.seq, b.qual, b.offset, b.res if with_res else None, b.select, b.order),
                                "%s results=%s" % (b.name, with_res))
        n += 1
    assert n >= 25
