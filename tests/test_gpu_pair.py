"""The pair stage on an MI355X (faqcs_pair_device, faqcs_render_pair_device): against the library's host statements (faqcs_pair_host,
faqcs_render_pair_host, which tests/test_pair_model.py ties to the numpy models, to the existing rendering statement and to the reference's
files), text to text from TWO device texts against the md5s of the reference's own files -- whole and in chunks that hold different numbers
of records per mate --, the argument checks, and two speed guards against the runtime's device-to-device copy."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import pair_cases as pcs
import render_cases as rc
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args
from test_gpu_parity import SEED
from test_gpu_render import SPEED_K, DeviceCase

pytestmark = pytest.mark.gpu

# faqcs_pair_device against the copy of the two texts: twice the ratio of the traffic counts of DESIGN.md section 4.10 (0.5 - 0.55), rounded up
# to the next half
PAIR_SPEED_K = 1.5


def engine(args, R=1024):
    from faqcs_amd.engine import HipEngine

    opt = parse_args(["-1", "a", "-2", "b", "-d", "y"] + args)
    return opt, HipEngine(opt, R, rc.in_offset(args), device=0)


class DevicePair:
    """A pair_cases.PairCase in device memory: each mate a test_gpu_render.DeviceCase of its own (own text, spans, arenas, results)."""

    def __init__(self, pc):
        self.pc = pc
        self.d = [DeviceCase(c) for c in pc.m]
        self.dev = self.d[0].dev

    def mates(self, with_res=(True, True), tn=True):
        out = []
        for dc, wr in zip(self.d, with_res):
            b = dc.batch(tn)
            m = capi.Mate(C.pointer(b), dc.res.data_ptr() if wr else None, dc.text.data_ptr() + 64, dc.def_pos.data_ptr(), dc.def_len.data_ptr())
            m._batch = b
            out.append(m)
        return out


def pair_dev(eng, m1, m2, n, with_res=True, with_route=True):
    """One faqcs_pair_device with canaries around route -> (route or None, info dict, the raw bytes of route and info)"""
    import torch

    dev = torch.device("cuda:0")
    buf = torch.full((64 + n + 64,), rc.CANARY, dtype=torch.uint8, device=dev)
    info = torch.full((5,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    eng.pair_device(m1, m2, buf.data_ptr() + 64 if with_route else None, info.data_ptr())
    eng.sync()
    h, raw = buf.cpu().numpy(), info.cpu().numpy().tobytes()
    assert (h[:64] == rc.CANARY).all() and (h[64 + n:] == rc.CANARY).all(), "bytes around route[0 .. n) were written"
    if not with_res:
        assert (h == rc.CANARY).all(), "check only: route was written"
    return (h[64:64 + n].copy() if with_res else None), pcs.info_dict(capi.PairInfo.from_buffer_copy(raw)), h.tobytes() + raw


def render_pair_dev(eng, dp, m1, m2, file, route, n_pairs, with_offset=True, with_index=True, capacity=None):
    """One faqcs_render_pair_device into sentinel-filled buffers; the WHOLE buffers come back as host arrays, in the form of render_cases.render_host."""
    import torch

    dev, nc = dp.dev, 2 * n_pairs
    cap = (len(dp.pc.m[0].text) + len(dp.pc.m[1].text) + 5 * nc) if capacity is None else capacity
    text = torch.full((rc.FRONT + cap + capi.ARENA_PAD_AFTER,), rc.CANARY, dtype=torch.uint8, device=dev)
    can32 = -0x5A5A5A5B
    roff = torch.full((nc + 2,), can32, dtype=torch.int32, device=dev)
    ridx = torch.full((nc + 1,), can32, dtype=torch.int32, device=dev)
    info = torch.full((2,), -1, dtype=torch.int64, device=dev)
    d_route = torch.from_numpy(np.concatenate([np.asarray(route, np.uint8), np.zeros(1, np.uint8)])).to(dev)
    torch.cuda.synchronize()
    assert (text.data_ptr() + rc.FRONT) % 16 == 0
    out = capi.RenderOut(text.data_ptr() + rc.FRONT, cap, roff.data_ptr() if with_offset else None, ridx.data_ptr() if with_index else None, info.data_ptr())
    eng.render_pair_device(file, m1, m2, d_route.data_ptr() if n_pairs else None, n_pairs, out)
    eng.sync()
    h = info.cpu().numpy().view(np.uint64)
    return {"text": text.cpu().numpy(), "base": rc.FRONT, "rec_offset": roff.cpu().numpy().view(np.uint32), "rec_index": ridx.cpu().numpy().view(np.uint32),
            "n_bytes": int(h[0]), "n_reads": int(h[1] & np.uint64(0xFFFFFFFF)), "overflow": int(h[1] >> np.uint64(32)),
            "with_offset": with_offset, "with_index": with_index, "exact": False}


def check_pair_and_files(eng, holder, pc, what, files=pcs.FILES):
    """Device == host statement for the pair call and the four files, each run twice on the one context with identical bytes."""
    lib = eng.lib
    dp = DevicePair(pc)
    m1, m2 = dp.mates()
    want_route, want = pcs.pair_host(lib, pc)
    first = None
    for rep in range(2):
        route, info, raw = pair_dev(eng, m1, m2, pc.n)
        assert info == want, what
        assert (route == want_route).all(), what
        assert first is None or raw == first, "the second run's bytes differ"
        first = raw
    # check only, with and without a route pointer, and without terminal_n
    c1, c2 = dp.mates(with_res=(False, False), tn=False)
    _, want0 = pcs.pair_host(lib, pc, with_res=False)
    for with_route in (True, False):
        r0, i0, _ = pair_dev(eng, c1, c2, pc.n, with_res=False, with_route=with_route)
        assert r0 is None and i0 == want0, what
    n = pc.n
    for f in files:
        o = pcs.render_pair_host(lib, holder, pc, f, want_route, n)
        w = pcs.rendering(o)
        first = None
        for rep, (with_offset, with_index) in enumerate(((True, True), (True, True), (False, False))):
            a, b = (m1, m2) if rep < 2 else dp.mates(tn=False)
            o = render_pair_dev(eng, dp, a, b, f, want_route, n, with_offset=with_offset, with_index=with_index)
            rc.assert_rendering(o, w, "%s file %d" % (what, f))
            if rep < 2:
                raw = o["text"].tobytes() + o["rec_offset"].tobytes() + o["rec_index"].tobytes()
                assert first is None or raw == first, "the second run's bytes differ"
                first = raw
    return want_route, want


SIZES = [0, 1, 2, 511, 512, 513, 1025, 3000]


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_host_statements(n):
    """Random pairs with ids from the catalogue at sizes around the tiles (256 pairs of the check, 512 pairs = 1 024 candidates of the scan): no
    mismatch with unequal counts, a mismatch in the last tile, a mismatch in the first tile with another behind it.  Route, info and the four
    files with rec_offset and rec_index equal the host statements byte for byte; every call runs twice on one context with identical bytes."""
    args = rc.OPTION_SETS[SIZES.index(n) % len(rc.OPTION_SETS)]
    rng = np.random.Generator(np.random.PCG64([61, SIZES.index(n), SEED]))
    opt, eng = engine(args)
    in_off = rc.in_offset(args)
    holder = capi.ParamsHolder(opt, 1024, in_off)
    variants = [("none", n, n + 3, ())]
    if n >= 1:
        variants.append(("last_tile", n + 2, n, (n - 1,)))
    if n >= 513:
        variants.append(("first_tile", n, n, (7, n - 100)))
    for name, n1, n2, bad in variants:
        pc = pcs.PairCase(rng, n1, n2, bad=bad, in_off=in_off, max_len=150 if n < 1025 else 60)
        route, info = check_pair_and_files(eng, holder, pc, "%d %s" % (n, name))
        assert info["n_pairs"] == (min(bad) if bad else n) and info["mismatch"] == (1 if bad else 0)
    eng.close()


@pytest.mark.parametrize("r", [3, 1, 2, 0])
def test_every_pair_routes_to_one_file(r):
    """600 pairs whose every route is r: one file (two for r = 3) holds everything, the others are empty (zeros, rec_offset[0] = 0)."""
    rng = np.random.Generator(np.random.PCG64([62, r, SEED]))
    opt, eng = engine(["--replace_to_N_q", "15"])
    holder = capi.ParamsHolder(opt, 1024, 33)
    pc = pcs.PairCase(rng, 600, max_len=150)
    for s, c in enumerate(pc.m):
        c.res["flags"] = (c.res["flags"] & ~np.uint16(1)) | (r >> s & 1)
    route, info = check_pair_and_files(eng, holder, pc, "route %d" % r)
    assert (route == r).all()
    dp = DevicePair(pc)
    m1, m2 = dp.mates()
    for f in pcs.FILES:
        o = render_pair_dev(eng, dp, m1, m2, f, route, 600)
        full = {3: (capi.FILE_QC1, capi.FILE_QC2), 1: (capi.FILE_UNPAIRED, capi.FILE_DISCARD), 2: (capi.FILE_UNPAIRED, capi.FILE_DISCARD), 0: (capi.FILE_DISCARD,)}[r]
        assert o["n_reads"] == ((1200 if r == 0 else 600) if f in full else 0), (r, f)
        if f not in full:
            assert (o["n_bytes"], o["overflow"]) == (0, 0) and o["rec_offset"][0] == 0
            rc.assert_untouched(o, 0, 0)
    eng.close()


class _Spans:
    """A mate for the id check alone: the deflines back to back as the whole text (the first starts at text position 0, the last ends at the
    text's last byte); the padding around the text holds bytes that would change a verdict if they were interpreted."""

    def __init__(self, deflines):
        self.n = len(deflines)
        self.text = np.frombuffer(b"".join(deflines), np.uint8)
        lens = np.array([len(d) for d in deflines], np.int64)
        self.def_len = lens.astype(np.uint32)
        self.def_pos = (np.cumsum(lens) - lens).astype(np.uint32)
        self.res = None
        self.seq = self.qual = np.zeros(1, np.uint8)
        self.offset = np.zeros(self.n + 1, np.uint32)


HOSTILE_PAD = b"/1 a9.2x"


def spans_on_device(dev, m):
    """A mate of deflines alone (text, def_pos, def_len, n) for the id check: the text with 64 bytes of HOSTILE_PAD in front of it and behind
    it (the pattern begins anew right behind the text).  -> (capi.Mate, what has to stay alive)"""
    import torch

    h = np.resize(np.frombuffer(HOSTILE_PAD, np.uint8), 64 + len(m.text) + 64).copy()
    h[64 + len(m.text):64 + len(m.text) + 8] = np.frombuffer(HOSTILE_PAD, np.uint8)
    h[64:64 + len(m.text)] = m.text
    t = torch.from_numpy(h).to(dev)
    dpos = torch.from_numpy(np.concatenate([m.def_pos, np.zeros(1, np.uint32)]).view(np.int32)).to(dev)
    dlen = torch.from_numpy(np.concatenate([m.def_len, np.zeros(1, np.uint32)]).view(np.int32)).to(dev)
    bt = capi.Batch(None, None, None, m.n, 0, None, 0, None)
    return capi.Mate(C.pointer(bt), None, t.data_ptr() + 64, dpos.data_ptr(), dlen.data_ptr()), [t, dpos, dlen, bt]


def test_deflines_at_the_ends_of_the_text_and_of_every_length():
    """Check only, on texts that are nothing but deflines: position 0, the text's last byte, a 0-byte defline next to one of 300, and every
    catalogue entry both ways round; the bytes in front of the text and the 64 behind it ("/1 a9.2x" ...) would change verdicts if they were read as part of a defline."""
    import torch

    rng = np.random.Generator(np.random.PCG64([63, SEED]))
    opt, eng = engine([])
    dev = torch.device("cuda:0")
    good = pcs.matching() + [(b, a) for a, b in pcs.matching()]
    long300 = [p for p in good if len(p[0]) == 300][0]
    base = [long300, (b"", b""), long300[::-1], (b"/1", b"")] + good

    def run(pairs):
        a, b = _Spans([p[0] for p in pairs]), _Spans([p[1] for p in pairs])
        pc = type("P", (), {"m": [a, b], "n": len(pairs)})()
        _, want = pcs.pair_host(eng.lib, pc, with_res=False)
        keep, mates = [], []
        for m in (a, b):
            mate, alive = spans_on_device(dev, m)
            keep += alive
            mates.append(mate)
        _, got, _ = pair_dev(eng, mates[0], mates[1], len(pairs), with_res=False, with_route=False)
        assert got == want, pairs[want["n_pairs"]] if want["mismatch"] else None
        return got

    got = run(base)
    assert (got["n_pairs"], got["mismatch"]) == (len(base), 0)
    # every mismatching entry in turn, as the LAST defline of both texts (it ends at the text's last byte), both ways round
    for a, b, ia, ib in pcs.mismatching():
        for x, y, lx, ly in ((a, b, len(ia), len(ib)), (b, a, len(ib), len(ia))):
            k = int(rng.integers(0, 40))
            got = run(base[:k] + [(x, y)])
            assert (got["n_pairs"], got["mismatch"], got["id_len"]) == (k, 1, (lx, ly)), (x, y)
    eng.close()


def _device_text(dev, text):
    import torch

    store = torch.full((64 + len(text) + 64,), 10, dtype=torch.uint8, device=dev)
    store[64:64 + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
    return store


def _parse_and_submit(hip, dev, stores, pos, ends, final, total_reads):
    """Both mates: faqcs_parse_device of text[pos : end], then faqcs_submit_device of the first n = min(n1, n2) reads of each.
    -> (n, [DeviceMate], [parse info], [tensors])"""
    import torch

    from faqcs_amd.device import DeviceMate
    from faqcs_amd.engine import _check
    from tools.parse_bench import parse_buffers, read_info

    parsed = []
    for s in range(2):
        n_text = ends[s] - pos[s]
        pout, t = parse_buffers(dev, n_text, total_reads)
        torch.cuda.synchronize()
        hip.parse_device(stores[s].data_ptr() + 64 + pos[s], n_text, final[s], pout)
        hip.sync()
        info = read_info(t["info"])
        assert (info["error"], info["overflow"]) == (0, 0)
        parsed.append((t, info))
    n = min(p[1]["n_reads"] for p in parsed)
    mates = []
    for s, (t, info) in enumerate(parsed):
        res = torch.zeros((max(n, 1), 4), dtype=torch.int16, device=dev)
        seg = np.array([0, n], dtype=np.uint32)
        b = capi.Batch(t["seq"].data_ptr() + 64, t["qual"].data_ptr() + 64, t["offset"].data_ptr(), n, 1, seg.ctypes.data, info["max_read_len"], t["terminal_n"].data_ptr())
        if n:
            _check(hip.lib, hip.lib.faqcs_submit_device(hip.ctx, C.byref(b), res.data_ptr()))
            hip.sync()
        mates.append(DeviceMate(stores[s][64 + pos[s]:], t["def_pos"][:n], t["def_len"][:n], t["seq"][64:], t["qual"][64:], t["offset"][:n + 1],
                                results=res[:n], terminal_n=t["terminal_n"][:n]))
    return n, mates, [p[1] for p in parsed], [p[0] for p in parsed]


PAIRED_GOLDEN = [n for n in rc.GOLDEN if n != "adv_unpaired_only"]


@pytest.mark.parametrize("name", PAIRED_GOLDEN)
def test_text_to_text_from_two_texts(name, fixture_cache, tmp_path):
    """Each mate's FASTQ text in its own device buffer -> two faqcs_parse_device -> two faqcs_submit_device -> pair_route -> paired_files: the
    md5 of each of the four texts is the reference's file and both counters are what the host driver counts.  No record or mask is made on
    the host and the mates are never concatenated.  Then the same input in three chunks cut at different places per mate (final = 0; the chunks
    hold different numbers of records, the surplus is carried by def_pos[n]): the concatenated outputs have the same md5s."""
    import golden_util
    import torch
    from oracle_engine import OracleEngine

    from faqcs_amd.device import pair_route, paired_files
    from faqcs_amd.engine import HipEngine

    case, opt, in_off, r1, r2 = rc.golden_inputs(name, fixture_cache, tmp_path)
    m = len(r1)
    texts = [rc.fastq_text(r1), rc.fastq_text(r2)]
    dev = torch.device("cuda:0")
    stores = [_device_text(dev, t) for t in texts]
    assert golden_util.run_case(case, fixture_cache, tmp_path, lambda o, R, q: OracleEngine(o, R, q), max_read_length=golden_util.case_max_read_length(case)) == []
    want_prn, want_pbl = driver.run.last.paired_read_number, driver.run.last.paired_base_length

    def check(files, prn, pbl, what):
        for f in pcs.FILES:
            fn = capi.PAIR_FILES[f]
            if fn in case["fastq"]:
                meta = case["fastq"][fn]
                assert (files[f][1], len(files[f][0])) == (meta["records"], meta["bytes"]), (what, fn)
                assert hashlib.md5(files[f][0]).hexdigest() == meta["md5"], (what, fn)
        assert (prn, pbl) == (want_prn, want_pbl), what

    # whole files
    hip = HipEngine(opt, 1024, in_off, device=0)
    n, mates, infos, keep = _parse_and_submit(hip, dev, stores, [0, 0], [len(t) for t in texts], [True, True], m)
    assert n == m
    route, info = pair_route(hip, mates[0], mates[1])
    assert (info["n_pairs"], info["mismatch"]) == (m, 0)
    out = paired_files(hip, mates[0], mates[1], route, info["n_pairs"])
    check({f: (out[f][0].cpu().numpy().tobytes(), int(out[f][1].numel()) - 1) for f in pcs.FILES}, info["paired_read_number"], info["paired_base_length"], "whole")
    hip.close()
    # three chunks, cut inside records: mate 1's text at 40 % and 80 %, mate 2's at 55 % and 70 %
    hip = HipEngine(opt, 1024, in_off, device=0)
    cuts = [[len(texts[0]) * 2 // 5, len(texts[0]) * 4 // 5, len(texts[0])], [len(texts[1]) * 11 // 20, len(texts[1]) * 7 // 10, len(texts[1])]]
    pos, acc, prn, pbl, counts = [0, 0], {f: [b"", 0] for f in pcs.FILES}, 0, 0, []
    for chunk in range(3):
        last = chunk == 2
        ends = [c[chunk] for c in cuts]
        n, mates, infos, keep = _parse_and_submit(hip, dev, stores, pos, ends, [last, last], m)
        counts.append([i["n_reads"] for i in infos])
        route, info = pair_route(hip, mates[0], mates[1])
        assert (info["n_pairs"], info["mismatch"]) == (n, 0)
        out = paired_files(hip, mates[0], mates[1], route, n)
        for f in pcs.FILES:
            acc[f][0] += out[f][0].cpu().numpy().tobytes()
            acc[f][1] += int(out[f][1].numel()) - 1
        prn += info["paired_read_number"]
        pbl += info["paired_base_length"]
        for s in range(2):  # the mate with surplus records resumes at the defline of its record n
            t, i = keep[s], infos[s]
            pos[s] += (int(t["def_pos"][n]) & 0xFFFFFFFF) if n < i["n_reads"] else i["consumed"]
    assert pos == [len(t) for t in texts]
    assert len(counts) == 3 and counts[0][0] < counts[0][1] and counts[1][0] > counts[1][1] and counts[2][0] == counts[2][1], counts  # (the surplus changed sides)
    check({f: tuple(acc[f]) for f in pcs.FILES}, prn, pbl, "chunks")
    hip.close()


def test_mate_id_mismatch_on_the_device(fixture_cache):
    """The fixture of err_mate_id_mismatch from two device texts, checked before anything is submitted: the ids of the reference's message."""
    import golden_util
    import make_fixtures
    import torch

    from faqcs_amd.device import DeviceMate, pair_route
    from faqcs_amd.engine import HipEngine
    from tools.parse_bench import parse_buffers, read_info

    case = golden_util.load_case("err_mate_id_mismatch")
    paths = golden_util.fixture_paths(case["fixture"], fixture_cache)
    dev = torch.device("cuda:0")
    hip = HipEngine(parse_args(["-1", "a", "-2", "b", "-d", "y"]), 1024, 33, device=0)
    mates = []
    for p in paths:
        text = rc.fastq_text(make_fixtures.read_fastq(p))
        store = _device_text(dev, text)
        pout, t = parse_buffers(dev, len(text), text.count(b"\n") // 4)
        torch.cuda.synchronize()
        hip.parse_device(store.data_ptr() + 64, len(text), True, pout)
        hip.sync()
        n = read_info(t["info"])["n_reads"]
        mates.append(DeviceMate(store[64:], t["def_pos"][:n], t["def_len"][:n], t["seq"][64:], t["qual"][64:], t["offset"][:n + 1]))
    route, info = pair_route(hip, mates[0], mates[1])
    assert route is None and (info["mismatch"], info["n_pairs"]) == (1, 20)
    assert info["ids"] == (b"@R20", b"@OTHER20")
    assert "Read one id (%s)" % info["ids"][0].decode() in case["stderr"] and "read two id (%s)" % info["ids"][1].decode() in case["stderr"]
    hip.close()


def test_argument_errors_leave_the_context_usable():
    """Every FAQCS_E_INVAL of the two entry points is returned at call time (nothing is enqueued), and the context works afterwards."""
    rng = np.random.Generator(np.random.PCG64([64, SEED]))
    opt, eng = engine([])
    holder = capi.ParamsHolder(opt, 1024, 33)
    lib = eng.lib
    pc = pcs.PairCase(rng, 50, 60)
    dp = DevicePair(pc)
    a, b = dp.mates()
    route, info = dp.d[0].tn.data_ptr(), dp.d[0].off.data_ptr()  # (device memory; never written: every call below is refused)
    E = capi.E_INVAL
    P = lib.faqcs_pair_device
    assert P(eng.ctx, None, C.byref(b), route, info) == E and P(eng.ctx, C.byref(a), None, route, info) == E
    assert P(eng.ctx, C.byref(a), C.byref(b), route, None) == E
    assert P(eng.ctx, C.byref(a), C.byref(b), None, info) == E  # results without a route
    for wr in ((True, False), (False, True)):  # exactly one results
        x, y = dp.mates(with_res=wr)
        assert P(eng.ctx, C.byref(x), C.byref(y), route, info) == E
    for bad in (capi.Mate(None, a.results, a.text, a.def_pos, a.def_len), capi.Mate(a.batch, a.results, None, a.def_pos, a.def_len),
                capi.Mate(a.batch, a.results, a.text, None, a.def_len), capi.Mate(a.batch, a.results, a.text, a.def_pos, None)):
        assert P(eng.ctx, C.byref(bad), C.byref(b), route, info) == E and P(eng.ctx, C.byref(b), C.byref(bad), route, info) == E
    big = capi.Batch(None, None, None, 1 << 31, 0, None, 0, None)
    bigm = capi.Mate(C.pointer(big), a.results, a.text, a.def_pos, a.def_len)
    assert P(eng.ctx, C.byref(bigm), C.byref(bigm), route, info) == E
    R = lib.faqcs_render_pair_device
    t0 = dp.d[0].text.data_ptr() + 64
    assert t0 % 16 == 0
    good = capi.RenderOut(t0, 100, None, None, info)
    for f in (-1, 4):
        assert R(eng.ctx, f, C.byref(a), C.byref(b), route, 50, C.byref(good)) == E
    assert R(eng.ctx, 0, C.byref(a), C.byref(b), route, 51, C.byref(good)) == E  # more pairs than mate 1 has reads
    assert R(eng.ctx, 0, C.byref(b), C.byref(a), route, 51, C.byref(good)) == E
    assert R(eng.ctx, 0, C.byref(bigm), C.byref(bigm), route, 1 << 31, C.byref(good)) == E
    assert R(eng.ctx, 0, C.byref(a), C.byref(b), None, 50, C.byref(good)) == E
    assert R(eng.ctx, 0, None, C.byref(b), route, 50, C.byref(good)) == E and R(eng.ctx, 0, C.byref(a), None, route, 50, C.byref(good)) == E
    assert R(eng.ctx, 0, C.byref(a), C.byref(b), route, 50, None) == E
    x, y = dp.mates(with_res=(True, False))
    assert R(eng.ctx, capi.FILE_QC1, C.byref(x), C.byref(y), route, 50, C.byref(good)) == E  # a trimmed file without results
    for bad in (capi.RenderOut(t0 + 4, 100, None, None, info), capi.RenderOut(None, 100, None, None, info), capi.RenderOut(t0, 100, None, None, None)):
        assert R(eng.ctx, 0, C.byref(a), C.byref(b), route, 50, C.byref(bad)) == E
    for bad in (capi.Mate(a.batch, a.results, None, a.def_pos, a.def_len), capi.Mate(a.batch, a.results, a.text, None, a.def_len),
                capi.Mate(a.batch, a.results, a.text, a.def_pos, None)):
        assert R(eng.ctx, 0, C.byref(bad), C.byref(b), route, 50, C.byref(good)) == E
    nob = capi.Batch(None, None, None, 50, 0, None, 0, None)
    assert R(eng.ctx, 0, C.byref(capi.Mate(C.pointer(nob), a.results, a.text, a.def_pos, a.def_len)), C.byref(b), route, 50, C.byref(good)) == E
    # the context is as good as new
    check_pair_and_files(eng, holder, pc, "after the refusals")
    eng.close()


@pytest.fixture(scope="module")
def big_pairs():
    """4 M device-built 2x150-shaped pairs: two texts with 16-byte deflines (tools.parse_bench.synth_text, one seed per mate), their arenas
    as the batches, full-window results, terminal_n.  Shared by the two speed guards."""
    import torch

    from faqcs_amd.engine import HipEngine, _check
    from tools.parse_bench import record_bytes, synth_text

    L, W, n = 150, 16, 4_000_000
    R = record_bytes(L)
    dev = torch.device("cuda:0")
    opt = parse_args(["-1", "a", "-2", "b", "-d", "y", "--ascii", "33"])
    eng = HipEngine(opt, 256, 33, device=0)
    off = torch.from_numpy((np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32).view(np.int32)).to(dev)
    dpos = torch.from_numpy((np.arange(n, dtype=np.uint64) * R).astype(np.uint32).view(np.int32)).to(dev)
    dlen = torch.full((n,), W, dtype=torch.int32, device=dev)
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    res[:, 1] = L
    res[:, 2] = 1
    keep, mates, batches, stores = [off, dpos, dlen, res], [], [], []
    for s in range(2):
        store, n_text, s2, q2 = synth_text(eng.lib, dev, n, L, seed=20260101 + s)
        tn = torch.zeros(n, dtype=torch.uint8, device=dev)
        _check(eng.lib, eng.lib.faqcs_terminal_n_flags(0, s2.data_ptr(), off.data_ptr(), n, tn.data_ptr()))
        b = capi.Batch(s2.data_ptr(), q2.data_ptr(), off.data_ptr(), n, 0, None, L, tn.data_ptr())
        mates.append(capi.Mate(C.pointer(b), res.data_ptr(), store.data_ptr() + 64, dpos.data_ptr(), dlen.data_ptr()))
        keep += [store, s2, q2, tn]
        batches.append(b)
        stores.append(store)
    torch.cuda.synchronize()
    yield {"eng": eng, "dev": dev, "n": n, "n_text": n * R, "mates": mates, "batches": batches, "stores": stores, "res": res, "dpos": dpos, "dlen": dlen, "keep": keep}
    eng.close()


def test_render_pair_is_not_slower_than_its_traffic(big_pairs):
    """Speed guard, in the form of test_render_is_not_slower_than_its_traffic: faqcs_render_pair_device(UNPAIRED) of 4 M pairs whose route
    alternates 1, 2, 1, 2 ... -- 4 M records of 321 bytes, every other one from the other mate's text and arenas -- takes at most SPEED_K
    (3.0, tests/test_gpu_render.py) x the runtime's device-to-device copy of the rendered bytes, HIP events on the library's stream, median
    of 7 after a warm-up, the copy timed in the same run.  The traffic per rendered record is that of faqcs_render_device plus half a route
    byte.  A single-source faqcs_render_device of 4 M records of mate 1 is timed alongside; the ratio is printed and recorded in DESIGN.md
    section 4.10, not asserted.  Measured on the MI355X: 1.348 ms against 0.493 ms for the copy, 2.74 x; the single-source rendering 1.351 ms,
    pair / single 1.00."""
    import torch

    g = big_pairs
    eng, dev, n, n_text = g["eng"], g["dev"], g["n"], g["n_text"]
    route = ((torch.arange(n, device=dev) & 1) + 1).to(torch.uint8)
    o_text = torch.empty(rc.FRONT + n_text + 64, dtype=torch.uint8, device=dev)
    roff = torch.empty(2 * n + 1, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    out = capi.RenderOut(o_text.data_ptr() + rc.FRONT, n_text, roff.data_ptr(), None, info.data_ptr())
    copy_dst = torch.empty(n_text, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    pair_ms, single_ms, copy_ms, n_bytes = [], [], [], 0
    for rep in range(8):  # the first round warms everything up (and grows the scratch)
        eng.render_pair_device(capi.FILE_UNPAIRED, g["mates"][0], g["mates"][1], route.data_ptr(), n, out)
        eng.sync()
        pair_ms.append(sum(eng.render_pair_time_ms()))
        h = info.cpu().numpy()
        n_bytes = int(h[0])
        assert (int(h[1]) & 0xFFFFFFFF, int(h[1]) >> 32) == (n, 0)
        eng.render_device(g["batches"][0], g["res"].data_ptr(), g["stores"][0].data_ptr() + 64, g["dpos"].data_ptr(), g["dlen"].data_ptr(), out)
        eng.sync()
        single_ms.append(sum(eng.render_time_ms()))
        assert int(info.cpu().numpy()[0]) == n_bytes
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        copy_dst[:n_bytes].copy_(o_text[rc.FRONT:rc.FRONT + n_bytes])
        e1.record()
        torch.cuda.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    pm, sm, cp = float(np.median(pair_ms[1:])), float(np.median(single_ms[1:])), float(np.median(copy_ms[1:]))
    print("faqcs_render_pair_device(UNPAIRED) %.3f ms, faqcs_render_device of as many records %.3f ms (pair / single %.2f), copy of the %d rendered bytes %.3f ms, ratio %.2f"
          % (pm, sm, pm / sm, n_bytes, cp, pm / cp))
    assert n_bytes == n_text
    assert pm <= SPEED_K * cp, "faqcs_render_pair_device %.3f ms vs %.3f ms for the copy of the rendered bytes" % (pm, cp)


def test_pair_is_not_slower_than_its_traffic(big_pairs):
    """Speed guard: faqcs_pair_device (ids, route, counters; check + finish, HIP events on the library's stream, median of 7 after a warm-up) on
    the 4 M pairs takes at most PAIR_SPEED_K = 1.5 x the runtime's device-to-device copy of the two texts in the same run.  The traffic
    counts: the 128-byte requests that hold the two 16-byte deflines, each made twice (the scan for the ' ', the
    comparison), 32 bytes of spans and results and 1 byte of route per pair, against 4 x 321 bytes for the copy: 0.5 - 0.55; twice that,
    rounded up to the next half.  Measured on the MI355X: 0.422 ms against 1.004 ms for the copy of the two texts, 0.42 x."""
    import torch

    g = big_pairs
    eng, dev, n, n_text = g["eng"], g["dev"], g["n"], g["n_text"]
    route = torch.empty(n, dtype=torch.uint8, device=dev)
    info = torch.zeros(5, dtype=torch.int64, device=dev)
    dst = [torch.empty(n_text, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    pair_ms, copy_ms = [], []
    for rep in range(8):
        eng.pair_device(g["mates"][0], g["mates"][1], route.data_ptr(), info.data_ptr())
        eng.sync()
        pair_ms.append(sum(eng.pair_time_ms()))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(2):
            dst[s].copy_(g["stores"][s][64:64 + n_text])
        e1.record()
        torch.cuda.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    p = pcs.info_dict(capi.PairInfo.from_buffer_copy(info.cpu().numpy().tobytes()))
    assert p == dict(paired_read_number=2 * n, paired_base_length=300 * n, n_pairs=n, mismatch=0, id_len=(0, 0), n_one_valid=0, n_none_valid=0)
    assert bool((route == 3).all())
    pm, cp = float(np.median(pair_ms[1:])), float(np.median(copy_ms[1:]))
    print("faqcs_pair_device %.3f ms, copy of the two texts (%d bytes each) %.3f ms, ratio %.2f" % (pm, n_text, cp, pm / cp))
    assert pm <= PAIR_SPEED_K * cp, "faqcs_pair_device %.3f ms vs %.3f ms for the copy of the two texts" % (pm, cp)
