"""faqcs_render_device on an MI355X: the FASTQ text of the output files assembled on the device, against the library's host statement
(faqcs_render_host, which tests/test_render_model.py ties to the numpy model, to faqcs_apply_edits and to the reference's files) and, text to
text, against the md5s of the reference's own files (the golden cases)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import render_cases as rc
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args
from test_gpu_parity import SEED

pytestmark = pytest.mark.gpu

# bytes moved per byte moved by a copy of the text, 2x150 default: 1.17; the guard is twice that, rounded up
SPEED_K = 3.0


def engine(args, R=capi.MAX_READ_LENGTH):
    from faqcs_amd.engine import HipEngine

    opt = parse_args(["-u", "x", "-d", "y"] + args)
    return opt, HipEngine(opt, R, rc.in_offset(args), device=0)


class DeviceCase:
    """A render_cases.Case in device memory under the padding contracts (16 readable bytes in front of the text and the arenas, 64 behind);
    the padding of the text holds '\\n' and '\\r', that of the arenas 'N'."""

    def __init__(self, case):
        import torch

        self.case = case
        self.dev = dev = torch.device("cuda:0")

        def padded(a, n, fill):
            h = np.full(64 + n + 64, fill, np.uint8)
            h[64:64 + n] = a[:n]
            return torch.from_numpy(h).to(dev)

        def u32(a):
            return torch.from_numpy(np.concatenate([np.asarray(a, np.uint32), np.zeros(1, np.uint32)]).view(np.int32)).to(dev)

        self.text = padded(case.text, len(case.text), 10)
        self.text[1:64:2] = 13
        self.seq, self.qual = padded(case.seq, case.total, ord("N")), padded(case.qual, case.total, 33)
        self.off, self.def_pos, self.def_len = u32(case.offset)[:case.n + 1], u32(case.def_pos), u32(case.def_len)
        self.res = torch.from_numpy(np.concatenate([case.res, np.zeros(1, capi.RESULT_DTYPE)]).view(np.int16).reshape(-1, 4)).to(dev)
        self.tn = torch.from_numpy(np.concatenate([case.tn, np.zeros(1, np.uint8)])).to(dev)
        torch.cuda.synchronize()

    def batch(self, tn=True):
        return capi.Batch(self.seq.data_ptr() + 64, self.qual.data_ptr() + 64, self.off.data_ptr(), self.case.n, 0, None, 0,
                          self.tn.data_ptr() if tn and self.case.n else None)


def render(eng, dc, with_res, select, order, tn=True, with_offset=True, with_index=True, capacity=None):
    """One faqcs_render_device into sentinel-filled buffers; the WHOLE buffers come back as host arrays, in the form of render_cases.render_host."""
    import torch

    case, dev, n = dc.case, dc.dev, dc.case.n
    cap = (len(case.text) + 5 * n) if capacity is None else capacity
    text = torch.full((rc.FRONT + cap + capi.ARENA_PAD_AFTER,), rc.CANARY, dtype=torch.uint8, device=dev)
    can32 = -0x5A5A5A5B
    roff = torch.full((n + 2,), can32, dtype=torch.int32, device=dev)
    ridx = torch.full((n + 1,), can32, dtype=torch.int32, device=dev)
    info = torch.full((2,), -1, dtype=torch.int64, device=dev)
    d_sel = torch.from_numpy(np.concatenate([np.asarray(select, np.uint8), np.zeros(1, np.uint8)])).to(dev) if select is not None else None
    d_ord = torch.from_numpy(np.concatenate([np.asarray(order, np.uint32), np.zeros(1, np.uint32)]).view(np.int32)).to(dev) if order is not None else None
    torch.cuda.synchronize()
    assert (text.data_ptr() + rc.FRONT) % 16 == 0
    out = capi.RenderOut(text.data_ptr() + rc.FRONT, cap, roff.data_ptr() if with_offset else None, ridx.data_ptr() if with_index else None, info.data_ptr())
    eng.render_device(dc.batch(tn), dc.res.data_ptr() if with_res else None, dc.text.data_ptr() + 64, dc.def_pos.data_ptr(), dc.def_len.data_ptr(), out,
                      d_sel.data_ptr() if d_sel is not None else None, d_ord.data_ptr() if d_ord is not None else None)
    eng.sync()
    h = info.cpu().numpy().view(np.uint64)
    return {"text": text.cpu().numpy(), "base": rc.FRONT, "rec_offset": roff.cpu().numpy().view(np.uint32), "rec_index": ridx.cpu().numpy().view(np.uint32),
            "n_bytes": int(h[0]), "n_reads": int(h[1] & np.uint64(0xFFFFFFFF)), "overflow": int(h[1] >> np.uint64(32)),
            "with_offset": with_offset, "with_index": with_index, "exact": False}


def host_statement(lib, holder, case, with_res, select, order, capacity=None):
    o = rc.render_host(lib, holder, case, with_res, select, order, capacity=capacity)
    assert o["overflow"] == 0
    nb, nr = o["n_bytes"], o["n_reads"]
    return o["text"][o["base"]:o["base"] + nb].copy(), o["rec_offset"][:nr + 1].copy(), o["rec_index"][:nr].copy()


SHAPES = {"short": (3000, 0, 60, 80), "150": (3000, 100, 150, 40), "6000": (120, 0, 6000, 80), "32767": (12, 20000, capi.MAX_READ_LENGTH, 80)}


@pytest.mark.parametrize("args", rc.OPTION_SETS, ids=lambda a: " ".join(a) or "default")
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_equals_the_host_statement(args, shape):
    """The random families of the CPU test in shapes up to 32 767-base reads: every (results, select, order) combination, with and without
    terminal_n, rec_offset and rec_index."""
    n, lo, hi, max_def = SHAPES[shape]
    rng = np.random.Generator(np.random.PCG64([41, list(SHAPES).index(shape), rc.OPTION_SETS.index(args), SEED]))
    in_off = rc.in_offset(args)
    reads = rc.random_reads(rng, n, in_off, max_len=hi, max_def=max_def, min_len=lo)
    if shape == "32767":
        L = capi.MAX_READ_LENGTH
        reads += [(b"@all-N", b"N" * L, bytes([in_off + 20]) * L), (b"", b"ACGT" * 30, bytes([in_off + 37]) * 120),
                  (b"@longest", bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)]), bytes((rng.integers(0, 42, L) + in_off).astype(np.uint8)))]
    case = rc.Case(rng, reads)
    if shape == "32767":
        case.res["flags"] |= 1
        case.res["start"][-3:] = 0
        case.res["len"][-3:] = [capi.MAX_READ_LENGTH, 120, capi.MAX_READ_LENGTH]
    opt, eng = engine(args)
    holder = capi.ParamsHolder(opt, capi.MAX_READ_LENGTH, in_off)
    dc = DeviceCase(case)
    for v, (with_res, sel, order) in enumerate(case.variants()):
        want = host_statement(eng.lib, holder, case, with_res, sel, order)
        assert len(want[2]) >= 2
        for tn, with_offset, with_index in ((True, True, True), (False, False, False)) if v % 3 == 0 else (((v & 1) == 0, (v & 2) == 0, (v & 4) == 0),):
            o = render(eng, dc, with_res, sel, order, tn=tn, with_offset=with_offset, with_index=with_index)
            rc.assert_rendering(o, want, "%s %s results=%s select=%s order=%s terminal_n=%s" % (shape, args, with_res, sel is not None, order is not None, tn))
    eng.close()


def test_batches_of_only_5_byte_records():
    """Empty deflines and empty windows / empty reads: more than 200 records end in every KiB of the text, which takes the lane's own search."""
    rng = np.random.Generator(np.random.PCG64([43, SEED]))
    opt, eng = engine([])
    holder = capi.ParamsHolder(opt, 256, 33)
    trimmed = rc.Case(rng, [(b"", b"ACGTACGT", b"IIIIIIII")] * 9000, windows="empty")
    raw = rc.Case(rng, [(b"", b"", b"")] * 9000, windows="empty")
    for case, with_res in ((trimmed, True), (raw, False)):
        dc = DeviceCase(case)
        for sel, order in ((None, None), (case.select, case.holes)):
            want = host_statement(eng.lib, holder, case, with_res, sel, order)
            assert len(want[0]) == 5 * len(want[2]) > 5000 and want[0][:5].tobytes() == b"\n\n+\n\n"
            rc.assert_rendering(render(eng, dc, with_res, sel, order), want)
    # ... and mixed with ordinary records
    reads = rc.random_reads(rng, 4000, 33, max_len=150, max_def=30)
    for k in range(0, 4000, 3):
        reads[k] = (b"", b"", b"")
    case = rc.Case(rng, reads)
    dc = DeviceCase(case)
    for with_res in (True, False):
        rc.assert_rendering(render(eng, dc, with_res, None, case.perm), host_statement(eng.lib, holder, case, with_res, None, case.perm))
    eng.close()


def test_bounds_overflow_and_empty():
    """Sentinel-filled buffers much larger than the text: only the stated ranges change.  On overflow only info changes; the exact capacity is
    enough; nothing rendered and no reads at all yield zeros."""
    rng = np.random.Generator(np.random.PCG64([47, SEED]))
    opt, eng = engine(["--replace_to_N_q", "15"])
    holder = capi.ParamsHolder(opt, 256, 33)
    case = rc.Case(rng, rc.random_reads(rng, 3000, 33, max_len=150))
    dc = DeviceCase(case)
    for with_res in (True, False):
        want = host_statement(eng.lib, holder, case, with_res, case.select, case.perm)
        nb, nr = len(want[0]), len(want[2])
        rc.assert_rendering(render(eng, dc, with_res, case.select, case.perm, capacity=3 * len(case.text) + 12345), want)
        for cap in (nb - 1, 0):
            o = render(eng, dc, with_res, case.select, case.perm, capacity=cap)
            assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (nb, nr, 1)
            rc.assert_untouched(o, nb, nr, overflow=True)
        rc.assert_rendering(render(eng, dc, with_res, case.select, case.perm, capacity=nb), want)
        o = render(eng, dc, with_res, np.zeros(case.n, np.uint8), None)
        assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (0, 0, 0) and o["rec_offset"][0] == 0
        rc.assert_untouched(o, 0, 0)
    empty = DeviceCase(rc.Case(rng, []))
    for with_res in (True, False):
        o = render(eng, empty, with_res, None, None)
        assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (0, 0, 0) and o["rec_offset"][0] == 0
        rc.assert_untouched(o, 0, 0)
    # argument checks (nothing is enqueued)
    lib, b = eng.lib, dc.batch()
    t0 = dc.text.data_ptr() + 64
    assert t0 % 16 == 0
    good = capi.RenderOut(t0, 100, None, None, dc.off.data_ptr())
    args = (dc.res.data_ptr(), t0, dc.def_pos.data_ptr(), dc.def_len.data_ptr(), None, None)
    for bad in (capi.RenderOut(t0 + 4, 100, None, None, dc.off.data_ptr()), capi.RenderOut(None, 100, None, None, dc.off.data_ptr()),
                capi.RenderOut(t0, 100, None, None, None)):
        assert lib.faqcs_render_device(eng.ctx, C.byref(b), *args, C.byref(bad)) == capi.E_INVAL
    assert lib.faqcs_render_device(eng.ctx, C.byref(b), *args, None) == capi.E_INVAL
    assert lib.faqcs_render_device(eng.ctx, None, *args, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_device(eng.ctx, C.byref(b), args[0], None, *args[2:], C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_device(eng.ctx, C.byref(b), args[0], args[1], None, *args[3:], C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_device(eng.ctx, C.byref(b), args[0], args[1], args[2], None, None, None, C.byref(good)) == capi.E_INVAL
    eng.close()


@pytest.mark.parametrize("name", rc.GOLDEN)
def test_text_to_text_reproduces_the_reference_files(name, fixture_cache, tmp_path):
    """The fixture's FASTQ text (mate 1 then mate 2 in one device buffer) -> faqcs_parse_device -> faqcs_submit_device -> one
    faqcs_render_device per output file, masks and interleave made with torch on the device: the md5 of each rendered text equals the
    reference's file.  No record is joined on the host."""
    import torch

    from faqcs_amd.device import rendered_fastq
    from faqcs_amd.engine import HipEngine, _check
    from tools.parse_bench import parse_buffers, read_info

    case, opt, in_off, r1, r2 = rc.golden_inputs(name, fixture_cache, tmp_path)
    paired = r2 is not None
    m = len(r1)
    n = 2 * m if paired else m
    text = rc.fastq_text(r1 + (r2 or []))
    dev = torch.device("cuda:0")
    store = torch.full((64 + len(text) + 64,), 10, dtype=torch.uint8, device=dev)
    store[64:64 + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
    d_text = store[64:64 + len(text)]
    hip = HipEngine(opt, 1024, in_off, device=0)
    pout, t = parse_buffers(dev, len(text), n)
    torch.cuda.synchronize()
    hip.parse_device(d_text.data_ptr(), len(text), True, pout)
    hip.sync()
    pinfo = read_info(t["info"])
    assert (pinfo["n_reads"], pinfo["error"], pinfo["overflow"]) == (n, 0, 0)
    seg = np.array([0, m, n] if paired else [0, n], dtype=np.uint32)
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    b = capi.Batch(t["seq"].data_ptr() + 64, t["qual"].data_ptr() + 64, t["offset"].data_ptr(), n, len(seg) - 1, seg.ctypes.data, pinfo["max_read_len"],
                   t["terminal_n"].data_ptr())
    _check(hip.lib, hip.lib.faqcs_submit_device(hip.ctx, C.byref(b), res.data_ptr()))
    hip.sync()
    valid = (res[:, 2] & 1) != 0
    v1, v2 = valid[:m], valid[m:] if paired else None
    inter = torch.stack([torch.arange(m, device=dev), torch.arange(m, device=dev) + m], dim=1).reshape(-1).to(torch.int32) if paired else None
    nb = pinfo["n_bytes"]
    d_seq, d_qual = t["seq"][64:64 + nb], t["qual"][64:64 + nb]
    for fn, (with_res, selfn, interleaved) in rc.file_plans(case, m, paired).items():
        sel = selfn(v1, v2, lambda a, c: torch.cat([a, c]), torch.zeros_like(v1)) if selfn else None
        out, roff = rendered_fastq(hip, d_text, t["def_pos"][:n], t["def_len"][:n], d_seq, d_qual, t["offset"][:n + 1], results=res if with_res else None,
                                   select=sel, order=inter if interleaved else None, terminal_n=t["terminal_n"][:n])
        meta = case["fastq"][fn]
        data = out.cpu().numpy().tobytes()
        assert (int(roff.numel()) - 1, len(data)) == (meta["records"], meta["bytes"]), fn
        assert hashlib.md5(data).hexdigest() == meta["md5"], fn
    hip.close()


def _render_big(eng, dev, b, d_res, store, dpos, dlen, n, cap):
    import torch

    o_text = torch.empty(rc.FRONT + cap + 64, dtype=torch.uint8, device=dev)
    roff = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ridx = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    out = capi.RenderOut(o_text.data_ptr() + rc.FRONT, cap, roff.data_ptr(), ridx.data_ptr(), info.data_ptr())
    eng.render_device(b, d_res, store.data_ptr() + 64, dpos.data_ptr(), dlen.data_ptr(), out)
    eng.sync()
    h = info.cpu().numpy().view(np.uint64)
    return o_text, roff, ridx, (int(h[0]), int(h[1] & np.uint64(0xFFFFFFFF)), int(h[1] >> np.uint64(32)))


def test_text_past_2_31_and_just_below_2_32_bytes():
    """A device-built text of 13.4 M 321-byte records whose end lies just below 2^32.  Without results the rendering of every record in input
    order IS that text, byte for byte -- every 32-bit position up to 2^32 is exercised.  With the results of a submission (default options) the
    text passes 2^31: totals exact, and 10 000 sampled records -- the first and last thousands and those around 2^31 -- against the model."""
    import torch

    from faqcs_amd.engine import HipEngine, _check
    from tools.parse_bench import record_bytes, synth_text

    L, W = 150, 16
    R = record_bytes(L)
    n = ((1 << 32) - 1) // R
    dev = torch.device("cuda:0")
    opt = parse_args(["-u", "x", "-d", "y", "--ascii", "33"])
    eng = HipEngine(opt, 256, 33, device=0)
    store, n_text, s2, q2 = synth_text(eng.lib, dev, n, L)
    assert (1 << 32) - R <= n_text < (1 << 32)
    seq0, qual0 = s2.data_ptr(), q2.data_ptr()  # (views 64 bytes into tensors with 128 spare bytes behind)
    off = torch.from_numpy((np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32).view(np.int32)).to(dev)
    dpos = torch.from_numpy((np.arange(n, dtype=np.uint64) * R).astype(np.uint32).view(np.int32)).to(dev)
    dlen = torch.full((n,), W, dtype=torch.int32, device=dev)
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    seg = np.array([0, n], dtype=np.uint32)
    b = capi.Batch(seq0, qual0, off.data_ptr(), n, 1, seg.ctypes.data, L, None)
    # the original records
    o_text, roff, ridx, info = _render_big(eng, dev, b, None, store, dpos, dlen, n, n_text)
    assert info == (n_text, n, 0)
    assert torch.equal(o_text[rc.FRONT:rc.FRONT + n_text], store[64:64 + n_text])
    ro = roff.to(torch.int64) & 0xFFFFFFFF
    assert bool((ro == torch.arange(n + 1, device=dev, dtype=torch.int64) * R).all())
    assert bool((ridx.to(torch.int64) == torch.arange(n, device=dev)).all())
    del ro
    # one byte short: overflow, info complete
    o2 = _render_big(eng, dev, b, None, store, dpos, dlen, n, n_text - 1)
    assert o2[3] == (n_text, n, 1)
    del o2
    # the trimmed records
    _check(eng.lib, eng.lib.faqcs_submit_device(eng.ctx, C.byref(b), res.data_ptr()))
    eng.sync()
    o_text, roff, ridx, info = _render_big(eng, dev, b, res.data_ptr(), store, dpos, dlen, n, n_text)
    lens = res[:, 1].to(torch.int64) & 0xFFFF
    valid = (res[:, 2] & 1) != 0
    n_rec = int(valid.sum())
    n_bytes = int((2 * lens[valid] + W + 5).sum())
    assert info == (n_bytes, n_rec, 0)
    assert n_bytes > 1 << 31, "the premise of this test: the trimmed text passes 2^31 bytes (%d)" % n_bytes
    ro = roff[:n_rec + 1].to(torch.int64) & 0xFFFFFFFF
    assert int(ro[0]) == 0 and int(ro[n_rec]) == n_bytes and bool((ro[1:] > ro[:-1]).all())
    assert bool((ridx[:n_rec].to(torch.int64) == torch.nonzero(valid).ravel()).all())
    rng = np.random.Generator(np.random.PCG64([53, SEED]))
    mid = int(torch.searchsorted(ro, torch.tensor([1 << 31], device=dev))[0])
    ks = np.unique(np.concatenate([np.arange(1000), np.arange(n_rec - 1000, n_rec), np.arange(mid - 500, mid + 500), rng.integers(0, n_rec, 7000)]))
    kt = torch.from_numpy(ks).to(dev)
    it = ridx[:n_rec][kt].to(torch.int64)
    sub_text = store[64:64 + n_text].view(n, R)[it].cpu().numpy().ravel()
    pad = np.zeros(64, np.uint8)
    sub_s, sub_q = np.concatenate([s2[it].cpu().numpy().ravel(), pad]), np.concatenate([q2[it].cpu().numpy().ravel(), pad])
    sub_res = res[it].cpu().numpy().view(np.uint16).view(capi.RESULT_DTYPE).ravel()
    m = len(ks)
    wtext, woff, widx = driver.render_model(opt, 33, sub_text, np.arange(m, dtype=np.uint32) * R, np.full(m, W, np.uint32), sub_s, sub_q,
                                            (np.arange(m + 1, dtype=np.uint64) * L).astype(np.uint32), sub_res)
    assert len(widx) == m  # every sampled record is a rendered one
    a, e = ro[kt], ro[kt + 1]
    assert ((e - a).cpu().numpy() == np.diff(woff.astype(np.int64))).all()
    flat = torch.repeat_interleave(a - torch.from_numpy(woff[:-1].astype(np.int64)).to(dev), e - a) + torch.arange(len(wtext), device=dev)
    assert (o_text[rc.FRONT + flat].cpu().numpy() == wtext).all()
    eng.close()


def test_render_is_not_slower_than_its_traffic():
    """Speed guard: on 8 M device-built 2x150-shaped records, default options, the trimmed rendering (scan + gather, HIP events on the
    library's stream, median of 7 after a warm-up) takes at most SPEED_K x the runtime's device-to-device copy of the same number of bytes in
    the same run.  The yardstick is the copy.  SPEED_K = 2 x the design's traffic count, rounded up (750 bytes moved per
    rendered 321-byte record against 642 for its copy, 1.17); the factor 2 covers what parse_gather, of the same shape, ran above its
    count (1.4 x) and the shared machine.  Measured on the MI355X: 2.37 ms against 0.953 ms, 2.48 x."""
    import torch

    from faqcs_amd.engine import HipEngine, _check
    from tools.parse_bench import record_bytes, synth_text

    L, W, n = 150, 16, 8_000_000
    R = record_bytes(L)
    dev = torch.device("cuda:0")
    opt = parse_args(["-u", "x", "-d", "y", "--ascii", "33"])
    eng = HipEngine(opt, 256, 33, device=0)
    store, n_text, s2, q2 = synth_text(eng.lib, dev, n, L)
    off = torch.from_numpy((np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32).view(np.int32)).to(dev)
    dpos = torch.from_numpy((np.arange(n, dtype=np.uint64) * R).astype(np.uint32).view(np.int32)).to(dev)
    dlen = torch.full((n,), W, dtype=torch.int32, device=dev)
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    tn = torch.zeros(n, dtype=torch.uint8, device=dev)
    _check(eng.lib, eng.lib.faqcs_terminal_n_flags(0, s2.data_ptr(), off.data_ptr(), n, tn.data_ptr()))
    seg = np.array([0, n], dtype=np.uint32)
    b = capi.Batch(s2.data_ptr(), q2.data_ptr(), off.data_ptr(), n, 1, seg.ctypes.data, L, tn.data_ptr())
    _check(eng.lib, eng.lib.faqcs_submit_device(eng.ctx, C.byref(b), res.data_ptr()))
    eng.sync()
    o_text = torch.empty(rc.FRONT + n_text + 64, dtype=torch.uint8, device=dev)
    roff = torch.empty(n + 1, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    out = capi.RenderOut(o_text.data_ptr() + rc.FRONT, n_text, roff.data_ptr(), None, info.data_ptr())
    copy_dst = torch.empty(n_text, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    render_ms, copy_ms, n_bytes = [], [], 0
    for rep in range(8):  # the first round warms both up (and grows the scratch)
        eng.render_device(b, res.data_ptr(), store.data_ptr() + 64, dpos.data_ptr(), dlen.data_ptr(), out)
        eng.sync()
        render_ms.append(sum(eng.render_time_ms()))
        n_bytes = int(info.cpu().numpy()[0])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        copy_dst[:n_bytes].copy_(o_text[rc.FRONT:rc.FRONT + n_bytes])
        e1.record()
        torch.cuda.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    rm, cp = float(np.median(render_ms[1:])), float(np.median(copy_ms[1:]))
    print("faqcs_render_device %.3f ms, copy of the %d rendered bytes %.3f ms, ratio %.2f" % (rm, n_bytes, cp, rm / cp))
    assert n_bytes > n_text // 2
    assert rm <= SPEED_K * cp, "faqcs_render_device %.3f ms vs %.3f ms for the copy of the rendered bytes" % (rm, cp)
    eng.close()
