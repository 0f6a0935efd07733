"""The catalogue of tests/pack_edges.py on an MI355X: every parse text through faqcs_parse_device against driver.parse_model, every emit
batch through faqcs_emit_device against driver.emit_model, every render batch through faqcs_render_device against the host statement --
byte for byte, canaries around every buffer, with the helpers of test_gpu_parse.py, test_gpu_emit.py and test_gpu_render.py.  One test per
edge family; tests/test_pack_edges_model.py holds the same cases against the models without a GPU and asserts the coverage table."""
import numpy as np
import pytest

import pack_edges as pe
import parse_cases as pc
import render_cases as rc
import test_gpu_emit as ge
import test_gpu_render as gr
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args
from test_gpu_parse import parse_device

pytestmark = pytest.mark.gpu

PADS = (10, 13)        # the padding around the text: '\n' alone, '\r' alone
SHIFTS = (0, 1, 15)    # the text's first byte relative to 16-byte alignment
EVERY_RUN = [(pad, shift, with_def) for pad in PADS for shift in SHIFTS for with_def in (True, False)]
EDIT = ["--replace_to_N_q", "15", "--out_ascii", "64"]


@pytest.fixture(scope="module")
def eng():
    from faqcs_amd.engine import HipEngine

    e = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def parse_texts(n_cu):
    """Every parse text, built once; the grid-stride texts are sized for the compute units of THIS device."""
    return {c.name: c for c in pe.parse_texts(n_cu)}


def run_parse(eng, case, finals=(True, False)):
    """Every text alike, whatever its size: per value of `final` one model, and against it both paddings at shifts 0, 1 and 15, with and
    without def_*.  (The model is what takes time on the texts of a megabyte and more, up to two seconds; their tests take one value of
    `final` per case of a parametrised test.)"""
    for final in finals:
        model = driver.parse_model(case.text, final)
        for pad, shift, with_def in EVERY_RUN:
            o = parse_device(eng, case.text, final, with_def=with_def, shift=shift, pad=pad)
            pc.assert_parse(o, case.text, final, round16=True, what="%s final=%d pad=%d shift=%d def=%d" % (case.name, final, pad, shift, with_def), model=model)


FINALS = pytest.mark.parametrize("final", (True, False), ids=("final", "open"))


def family(parse_texts, *prefixes):
    out = [c for n, c in parse_texts.items() if n.startswith(prefixes)]
    assert out
    return out


def test_parse_text_sizes_and_last_piece_tails(eng, parse_texts):
    cases = family(parse_texts, "size_")
    assert len(cases) == 28
    for case in cases:
        run_parse(eng, case)


def test_parse_tile_and_piece_edges(eng, parse_texts):
    for case in family(parse_texts, "nl_at_tile_edge", "crlf_across_", "line_over_three_tiles"):
        run_parse(eng, case)


def test_parse_saturated_tiles(eng, parse_texts):
    cases = family(parse_texts, "saturated_")
    assert len(cases) == 6
    for case in cases:
        run_parse(eng, case)


def test_parse_content_len(eng, parse_texts):
    for case in family(parse_texts, "cr_positions_", "cr_behind_line_end", "empty_lines_cr_behind", "cr_in_last_tile_only"):
        run_parse(eng, case)


def test_parse_first_bad_record(eng, parse_texts):
    cases = family(parse_texts, "bad_at_", "bad_last_tail_")
    assert len(cases) == 5 + len(pc.TAILS)
    for case in cases:
        run_parse(eng, case)
        assert driver.parse_model(case.text, True)[7] == capi.PARSE_E_LENGTH


@FINALS
@pytest.mark.parametrize("name", ("bad_beyond_scan_round", "bad_in_lower_scan_slot"))
def test_parse_bad_record_beyond_one_scan_round(eng, parse_texts, name, final):
    case = parse_texts[name]
    c = case.ctx(final)
    assert len(c.bad) == 2 and c.bad[1] >= pe.SCAN_THREADS * pe.REC_TILE
    run_parse(eng, case, (final,))


@FINALS
@pytest.mark.parametrize("name", ("grid_stride_bad", "grid_stride_clean"))
def test_parse_grid_stride(eng, parse_texts, n_cu, name, final):
    """More record tiles than parse_rec_totals / parse_rec_apply have blocks (8 per compute unit of THIS device): the first bad record in the
    second stride, and a clean text."""
    case = parse_texts[name]
    c = case.ctx(final)
    print("n_cu %d: %s holds %d records in %d record tiles, grid %d" % (n_cu, name, c.n_cand, -(-c.n_cand // pe.REC_TILE), n_cu * pe.GRID_BLOCKS_PER_CU))
    assert c.n_cand > n_cu * pe.GRID_BLOCKS_PER_CU * pe.REC_TILE
    assert len(c.bad) == (name == "grid_stride_bad")
    assert not len(c.bad) or c.n_reads // pe.REC_TILE >= n_cu * pe.GRID_BLOCKS_PER_CU
    run_parse(eng, case, (final,))


@FINALS
def test_parse_ragged_text_of_more_than_1024_tiles(eng, parse_texts, final):
    case = parse_texts["ragged_16MiB"]
    assert len(case.text) > pe.SCAN_THREADS * pe.TEXT_TILE
    run_parse(eng, case, (final,))


def test_parse_chunked_feed_at_tile_and_piece_edges(eng, parse_texts):
    for case in family(parse_texts, "chunked_"):
        seq, qual, offset, tn, dpos, dlen, consumed, error = driver.parse_model(case.text, True)
        want = [(int(dpos[k]), int(dlen[k]), bytes(seq[offset[k]:offset[k + 1]]), bytes(qual[offset[k]:offset[k + 1]]), int(tn[k])) for k in range(len(tn))]
        for pad, shift in ((10, 0), (13, 1), (10, 15)):
            parse = lambda piece, final: parse_device(eng, piece, final, shift=shift, pad=pad)
            assert pc.chunked(parse, case.text, case.cuts) == (want, consumed, error), case.name
        run_parse(eng, case)


def test_parse_gather_layouts(eng, parse_texts):
    cases = family(parse_texts, "layout_")
    assert len(cases) >= 35
    for case in cases:
        run_parse(eng, case)


# ---- emit -------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emit_engines():
    from faqcs_amd.engine import HipEngine

    out = []
    for args in ([], EDIT):
        opt = parse_args(["-u", "x", "-d", "y"] + args)
        out.append((opt, HipEngine(opt, capi.MAX_READ_LENGTH, 33, device=0)))
    yield out
    for _, e in out:
        e.close()


def run_emit(engines, b):
    """Default options (the copy path) and the EDIT path, terminal_n given and absent, with and without the index."""
    import torch

    db = ge.DeviceBatch(b.seq, b.qual, b.offset, b.seg)
    assert (db.h_tn == b.tn).all()
    db.res[:b.n] = torch.from_numpy(b.res.view(np.int16).reshape(-1, 4).copy()).to(db.dev)
    torch.cuda.synchronize()
    for opt, eng in engines:
        want = driver.emit_model(opt, 33, b.seq, b.qual, b.offset, b.res, b.keep)
        for tn, with_index in ((True, True), (False, False)):
            o = ge.emit(eng, db, capi.MAX_READ_LENGTH, keep=b.keep, tn=tn, with_index=with_index)
            ge.assert_emission(o, want, "%s replace_to_N_q=%d terminal_n=%s" % (b.name, opt.replace_to_N_q, tn))


@pytest.fixture(scope="module")
def emit_batches():
    return {b.name: b for b in pe.batch_cases("emit")}


def batches(table, *prefixes):
    out = [b for n, b in table.items() if n.startswith(prefixes)]
    assert out
    return out


def test_emit_gather_layouts(emit_engines, emit_batches):
    cases = batches(emit_batches, "layout_")
    assert len(cases) >= 35
    for b in cases:
        run_emit(emit_engines, b)


def test_emit_scan_tiles(emit_engines, emit_batches):
    cases = batches(emit_batches, "n_reads_", "tile_all_dropped", "last_of_tile_first_of_next", "tiles_alternate")
    assert len(cases) == 9
    for b in cases:
        run_emit(emit_engines, b)


def test_emit_scan_carries_into_a_second_round(emit_engines, emit_batches):
    b = emit_batches["scan_second_round"]
    assert b.n == pe.SCAN_THREADS * pe.TILE_ITEMS + 1500
    run_emit(emit_engines, b)


def test_emit_terminal_n_extents(emit_engines, emit_batches):
    run_emit(emit_engines, emit_batches["terminal_N"])


# ---- render -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def render_engines():
    out = []
    for args in ([], EDIT):
        opt, e = gr.engine(args)  # (no --ascii: render_cases.in_offset gives the engine Phred+33)
        out.append((opt, e, capi.ParamsHolder(opt, capi.MAX_READ_LENGTH, 33)))
    yield out
    for _, e, _ in out:
        e.close()


def run_render(engines, b):
    """The trimmed stream under default options and on the EDIT path, the discard stream; terminal_n given and absent."""
    dc = gr.DeviceCase(b)
    for i, (opt, eng, holder) in enumerate(engines):
        for with_res in ((True, False) if i == 0 else (True,)):
            want = gr.host_statement(eng.lib, holder, b, with_res, b.select, b.order, capacity=b.render_capacity)
            for tn, with_arrays in ((True, True), (False, False)):
                o = gr.render(eng, dc, with_res, b.select, b.order, tn=tn, with_offset=with_arrays, with_index=with_arrays, capacity=b.render_capacity)
                rc.assert_rendering(o, want, "%s replace_to_N_q=%d results=%s terminal_n=%s" % (b.name, opt.replace_to_N_q, with_res, tn))


@pytest.fixture(scope="module")
def render_batches():
    return {b.name: b for b in pe.batch_cases("render")}


def test_render_gather_layouts(render_engines, render_batches):
    cases = batches(render_batches, "layout_")
    assert len(cases) >= 20
    for b in cases:
        run_render(render_engines, b)


def test_render_scan_tiles(render_engines, render_batches):
    """The tile patterns over the reads as they lie, over the candidates of a permutation, and with holes in the order doing the dropping."""
    cases = batches(render_batches, "n_reads_", "tile_all_dropped", "last_of_tile_first_of_next", "tiles_alternate")
    assert len(cases) == 15 and sum(b.order is not None for b in cases) == 6
    for b in cases:
        run_render(render_engines, b)


@pytest.mark.parametrize("name", ("scan_second_round", "scan_second_round_permuted", "scan_second_round_holes"))
def test_render_scan_carries_into_a_second_round(render_engines, render_batches, name):
    b = render_batches[name]
    assert b.n == pe.SCAN_THREADS * pe.TILE_ITEMS + 1500 and (b.order is None) == (name == "scan_second_round")
    run_render(render_engines, b)


def test_render_terminal_n_extents(render_engines, render_batches):
    run_render(render_engines, render_batches["terminal_N"])


def test_no_case_is_left_out(parse_texts, emit_batches, render_batches):
    """Every case of the catalogue (pack_edges.all_cases() is the three fixtures' builders, one after the other) belongs to one of the families above."""
    parse_prefixes = ("size_", "nl_at_tile_edge", "crlf_across_", "line_over_three_tiles", "saturated_", "cr_positions_", "cr_behind_line_end", "empty_lines_cr_behind",
                      "cr_in_last_tile_only", "bad_at_", "bad_last_tail_", "bad_beyond_scan_round", "bad_in_lower_scan_slot", "grid_stride_", "ragged_16MiB", "chunked_", "layout_")
    batch_prefixes = ("layout_", "n_reads_", "tile_all_dropped", "last_of_tile_first_of_next", "tiles_alternate", "scan_second_round", "terminal_N")
    assert all(n.startswith(parse_prefixes) for n in parse_texts)
    assert all(n.startswith(batch_prefixes) for n in list(emit_batches) + list(render_batches))
