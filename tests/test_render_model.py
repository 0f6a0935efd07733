"""CPU-side checks of the device rendering (faqcs_render_device): the numpy model the GPU tests use as their expected value agrees with the
library's host statement of the rules (faqcs_render_host) and, record by record, with faqcs_apply_edits; both reproduce the REFERENCE's own
output files byte for byte (the md5s of the golden cases) from the oracle's per-read results; the entry points are there, declared as the
header says, and refuse a null context before they touch a device."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import render_cases as rc
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    return capi.load_library()


@pytest.mark.parametrize("args", rc.OPTION_SETS, ids=lambda a: " ".join(a) or "default")
def test_render_model_matches_render_host(lib, args):
    """300 random ragged reads, deflines of 0 .. 80 bytes, N runs at the ends, random windows (empty ones too), flags, select, order (a
    permutation, and one with entries that name no read), with results and without: model == host statement, sentinels untouched; and each
    record of the trimmed form is defline + what faqcs_apply_edits writes for that window."""
    rng = np.random.default_rng(11)
    opt = parse_args(["-u", "x", "-d", "y"] + args)
    in_off = rc.in_offset(args)
    h = capi.ParamsHolder(opt, 256, in_off)
    case = rc.Case(rng, rc.random_reads(rng, 300, in_off))
    lens = np.diff(case.offset.astype(np.int64))
    n_var = 0
    for with_res, sel, order in case.variants():
        want = case.model(opt, in_off, with_res, sel, order)
        wtext, woff, widx = want
        assert 20 < len(widx) <= case.n
        for with_offset, with_index in ((True, True), (False, False)):
            o = rc.render_host(lib, h, case, with_res, sel, order, with_offset=with_offset, with_index=with_index)
            rc.assert_rendering(o, want, "%s results=%s select=%s order=%s" % (args, with_res, sel is not None, order is not None))
        n_var += 1
        # the rules, spelled out once more without the model's helpers
        cand = range(case.n) if order is None else [int(x) for x in order if x < case.n]
        idx = [i for i in cand if (sel is None or sel[i]) and (not with_res or case.res["flags"][i] & 1)]
        assert widx.tolist() == idx
        for k, i in enumerate(idx):
            a = int(case.offset[i])
            d = case.text[case.def_pos[i]:case.def_pos[i] + case.def_len[i]].tobytes()
            if with_res:
                ln = int(case.res["len"][i])
                os_, oq = np.zeros(ln + 1, np.uint8), np.zeros(ln + 1, np.uint8)
                assert lib.faqcs_apply_edits(C.byref(h.p), case.seq[a:].ctypes.data, case.qual[a:].ctypes.data, int(lens[i]), case.res[i:].ctypes.data,
                                             os_.ctypes.data, oq.ctypes.data) == 0
                rec = d + b"\n" + os_[:ln].tobytes() + b"\n+\n" + oq[:ln].tobytes() + b"\n"
                assert len(rec) == len(d) + 2 * ln + 5
            else:
                rec = d + b"\n" + case.reads[i][1] + b"\n+\n" + case.reads[i][2] + b"\n"
            assert wtext[woff[k]:woff[k + 1]].tobytes() == rec, (args, with_res, k, i)
    assert n_var == 12


def test_render_host_overflow_and_empty(lib):
    """info is complete on overflow and nothing else is written; the exact capacity is enough; nothing rendered yields zeros."""
    rng = np.random.default_rng(12)
    opt = parse_args(["-u", "x", "-d", "y"])
    h = capi.ParamsHolder(opt, 256, 33)
    case = rc.Case(rng, rc.random_reads(rng, 200, 33))
    for with_res in (True, False):
        want = case.model(opt, 33, with_res, None, case.perm)
        nb, nr = len(want[0]), len(want[2])
        assert nb > 1000
        for cap in (nb - 1, 0):
            o = rc.render_host(lib, h, case, with_res, None, case.perm, capacity=cap)
            assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (nb, nr, 1)
            rc.assert_untouched(o, nb, nr, overflow=True)
        rc.assert_rendering(rc.render_host(lib, h, case, with_res, None, case.perm, capacity=nb), want)
        # nothing selected
        o = rc.render_host(lib, h, case, with_res, np.zeros(case.n, np.uint8), None)
        assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (0, 0, 0) and o["rec_offset"][0] == 0
        rc.assert_untouched(o, 0, 0)
    # no reads at all
    empty = rc.Case(rng, [])
    for with_res in (True, False):
        o = rc.render_host(lib, h, empty, with_res, None, None)
        assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (0, 0, 0) and o["rec_offset"][0] == 0
        rc.assert_untouched(o, 0, 0)
    # only 5-byte records: empty deflines, empty windows
    tiny = rc.Case(rng, [(b"", b"ACGT", b"IIII")] * 50, windows="empty")
    want = tiny.model(opt, 33, True, None, None)
    assert want[0].tobytes() == b"\n\n+\n\n" * 50
    rc.assert_rendering(rc.render_host(lib, h, tiny, True, None, None), want)


@pytest.mark.parametrize("name", rc.GOLDEN)
def test_render_reproduces_the_reference_files(lib, name, fixture_cache, tmp_path):
    """The files the REFERENCE wrote for the golden cases -- bytes, records, md5 as stored in tests/golden/cases -- from the fixture's FASTQ
    text (mate 1 then mate 2 in one text), the oracle's per-read results, the masks and the fixed interleave of INTEGRATION.md section 3.1:
    one faqcs_render_host call per file, and the model gives the same bytes."""
    from oracle_engine import OracleEngine

    case, opt, in_off, r1, r2 = rc.golden_inputs(name, fixture_cache, tmp_path)
    paired = r2 is not None
    m = len(r1)
    reads = r1 + (r2 or [])
    cs = rc.Case(np.random.default_rng(0), reads, windows=None)
    bufs = [r1, r2] if paired else [r1]
    seq, qual, offset, seg = driver.pack_segments(bufs)
    res = OracleEngine(opt, 1024, in_off).process(seq, qual, offset, seg)
    cs.res = res
    valid = (res["flags"] & capi.F_VALID) != 0
    v1, v2 = valid[:m], valid[m:] if paired else None
    inter = np.stack([np.arange(m), np.arange(m) + m], axis=1).ravel().astype(np.uint32) if paired else None
    h = capi.ParamsHolder(opt, 1024, in_off)
    plans = rc.file_plans(case, m, paired)
    if name == "adv_discard":
        assert len(plans) == 4
    for fn, (with_res, selfn, interleaved) in plans.items():
        sel = selfn(v1, v2, lambda a, b: np.concatenate([a, b]), np.zeros(m, bool)).astype(np.uint8) if selfn else None
        order = inter if interleaved else None
        o = rc.render_host(lib, h, cs, with_res, sel, order, with_index=False)
        meta = case["fastq"][fn]
        text = o["text"][o["base"]:o["base"] + o["n_bytes"]].tobytes()
        assert (o["n_reads"], o["n_bytes"], o["overflow"]) == (meta["records"], meta["bytes"], 0), fn
        assert hashlib.md5(text).hexdigest() == meta["md5"], fn
        want = cs.model(opt, in_off, with_res, sel, order)
        assert want[0].tobytes() == text, fn
    if name == "adv_discard":
        assert case["fastq"]["QC.discard.trimmed.fastq"]["records"] == 422 and case["fastq"]["QC.discard.trimmed.fastq"]["bytes"] == 98357
        assert case["fastq"]["QC.unpaired.trimmed.fastq"]["records"] == 372
    if name == "adv_unpaired_only":
        assert case["fastq"]["QC.discard.trimmed.fastq"]["records"] == 203


def test_render_entry_points_are_declared_and_check_their_arguments(lib):
    for s in ("faqcs_render_device", "faqcs_render_host", "faqcs_render_time_ms"):
        assert s in capi.declared_symbols() and hasattr(lib, s)
    assert C.sizeof(capi.RenderInfo) == 16
    assert C.sizeof(capi.RenderOut) == 40
    b = capi.Batch(None, None, None, 0, 0, None, 0, None)
    info = capi.RenderInfo()
    out = capi.RenderOut(None, 0, None, None, None)
    # a null context is refused at call time, before any device is touched (this machine may have none)
    assert lib.faqcs_render_device(None, C.byref(b), None, None, None, None, None, None, C.byref(out)) == capi.E_INVAL
    assert b"null ctx" in lib.faqcs_last_error()
    a, g = C.c_double(), C.c_double()
    assert lib.faqcs_render_time_ms(None, C.byref(a), C.byref(g)) == capi.E_INVAL
    # the host form: null batch / spans / out / text / info, a text that is not 16-byte aligned
    z = np.zeros(64, np.uint32)
    buf = np.zeros(256, np.uint8)
    t = buf.ctypes.data + (-buf.ctypes.data) % 16
    good = capi.RenderOut(t, 64, None, None, C.addressof(info))
    assert lib.faqcs_render_host(None, C.byref(b), None, None, z.ctypes.data, z.ctypes.data, None, None, C.byref(good)) == 0
    assert (info.n_bytes, info.n_reads, info.overflow) == (0, 0, 0)
    assert lib.faqcs_render_host(None, None, None, None, z.ctypes.data, z.ctypes.data, None, None, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_host(None, C.byref(b), None, None, None, z.ctypes.data, None, None, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_host(None, C.byref(b), None, None, z.ctypes.data, None, None, None, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_host(None, C.byref(b), None, None, z.ctypes.data, z.ctypes.data, None, None, None) == capi.E_INVAL
    for bad in (capi.RenderOut(None, 64, None, None, C.addressof(info)), capi.RenderOut(t, 64, None, None, None),
                capi.RenderOut(t + 4, 64, None, None, C.addressof(info))):
        assert lib.faqcs_render_host(None, C.byref(b), None, None, z.ctypes.data, z.ctypes.data, None, None, C.byref(bad)) == capi.E_INVAL
    one = capi.Batch(buf.ctypes.data, buf.ctypes.data, z.ctypes.data, 1, 1, None, 0, None)
    assert lib.faqcs_render_host(None, C.byref(one), None, None, z.ctypes.data, z.ctypes.data, None, None, C.byref(good)) == capi.E_INVAL  # reads, no text
