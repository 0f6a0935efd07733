"""faqcs_parse_device on an MI355X: FASTQ text in device memory to the packed batch, against the numpy model (driver.parse_model) and the
ORACLE -- never against the code under test -- on the texts of tests/parse_cases.py and on larger shapes, canaries around every buffer."""
import ctypes as C

import numpy as np
import pytest

import parse_cases as pc
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args
from test_gpu_parity import SEED, random_batch

pytestmark = pytest.mark.gpu

TEXT_FRONT = 64  # bytes in front of the text in its tensor (>= FAQCS_ARENA_PAD_BEFORE)


@pytest.fixture(scope="module")
def eng():
    from faqcs_amd.engine import HipEngine

    e = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    yield e
    e.close()


def device_text(text, shift=0, pad=None):
    """The text in device memory, hostile bytes ('\\n', '\\r') in the padding either side; `shift` moves it off 16-byte alignment.  pad: one
    byte value for the whole padding (10 or 13) in place of the two alternating."""
    import torch

    dev = torch.device("cuda:0")
    host = np.full(TEXT_FRONT + shift + len(text) + capi.ARENA_PAD_AFTER, 10 if pad is None else pad, np.uint8)
    if pad is None:
        host[1::2] = 13
    host[TEXT_FRONT + shift:TEXT_FRONT + shift + len(text)] = np.frombuffer(text, np.uint8)
    t = torch.from_numpy(host).to(dev)
    return t, t.data_ptr() + TEXT_FRONT + shift


def parse_device(eng, text, final, cap_bytes=None, cap_reads=None, with_def=True, shift=0, keep=False, pad=None):
    """One faqcs_parse_device into canary-filled device buffers; everything comes back as host arrays (the WHOLE buffers), in the form of
    parse_cases.parse_host."""
    import torch

    text = bytes(text)
    dev = torch.device("cuda:0")
    cap_bytes = len(text) // 2 + 8 if cap_bytes is None else cap_bytes
    cap_reads = len(text) // 4 + 8 if cap_reads is None else cap_reads
    t_text, d_text = device_text(text, shift, pad)
    seq = torch.full((pc.FRONT + cap_bytes + capi.ARENA_PAD_AFTER,), pc.CANARY, dtype=torch.uint8, device=dev)
    qual = torch.full_like(seq, pc.CANARY)
    can32 = -0x5A5A5A5B
    off = torch.full((cap_reads + 1,), can32, dtype=torch.int32, device=dev)
    tn = torch.full((cap_reads + 1,), pc.CANARY, dtype=torch.uint8, device=dev)
    dpos, dlen = torch.full((cap_reads + 1,), can32, dtype=torch.int32, device=dev), torch.full((cap_reads + 1,), can32, dtype=torch.int32, device=dev)
    info = torch.full((4,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert (seq.data_ptr() + pc.FRONT) % 16 == 0 and (qual.data_ptr() + pc.FRONT) % 16 == 0
    out = capi.ParseOut(seq.data_ptr() + pc.FRONT, qual.data_ptr() + pc.FRONT, cap_bytes, cap_reads, off.data_ptr(), tn.data_ptr(),
                        dpos.data_ptr() if with_def else None, dlen.data_ptr() if with_def else None, info.data_ptr())
    eng.parse_device(d_text, len(text), final, out)
    eng.sync()
    p = capi.ParseInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    o = {"seq": seq.cpu().numpy(), "qual": qual.cpu().numpy(), "offset": off.cpu().numpy().view(np.uint32), "terminal_n": tn.cpu().numpy(),
         "def_pos": dpos.cpu().numpy().view(np.uint32), "def_len": dlen.cpu().numpy().view(np.uint32), "with_def": with_def,
         "info": {f: int(getattr(p, f)) for f, _ in capi.ParseInfo._fields_}, "cap_bytes": cap_bytes, "cap_reads": cap_reads}
    if keep:
        o.update(d_seq=seq, d_qual=qual, d_off=off, d_tn=tn)
    return o


def test_small_texts_equal_the_model(eng):
    """The texts of the host test (every tail, '\\r' in every place, mismatches, reads of 0 .. 400 bases), both values of `final`, the text at
    every alignment, with and without the defline arrays."""
    rng = np.random.Generator(np.random.PCG64([61, SEED]))
    k = 0
    for name, text in pc.small_texts(rng, rounds=2):
        for final in (True, False):
            o = parse_device(eng, text, final, with_def=(k % 3 != 0), shift=k % 16)
            pc.assert_parse(o, text, final, round16=True, what="%s final=%d shift=%d" % (name, final, k % 16))
            k += 1
    assert k >= 150


def _shape_lens(rng, shape):
    if shape == "uniform150":
        return np.full(20000, 150)
    if shape == "ragged6000":
        return rng.integers(0, 6001, 700)
    if shape == "tiny":        # thousands of records of 0 .. 3 bases: hundreds of records per KiB of output
        return rng.integers(0, 4, 40000)
    lens = rng.integers(0, 200, 300)  # one base line of >= 300 000 bytes among short ones
    lens[137] = 300000 + int(rng.integers(0, 50000))
    return lens


@pytest.mark.parametrize("final", [True, False], ids=["final", "open"])
@pytest.mark.parametrize("cr", [False, True], ids=["lf", "cr"])
@pytest.mark.parametrize("shape", ["uniform150", "ragged6000", "tiny", "long_line"])
def test_shapes_equal_the_model(eng, shape, cr, final):
    rng = np.random.Generator(np.random.PCG64([67, len(shape), int(cr), int(final), SEED]))
    lens = _shape_lens(rng, shape)
    # with '\r': a '\r\n' file whose records also carry lone '\r's and junk (a cut in one line only would end the parse at that record)
    text = pc.make_text(rng, lens, b"\r\n" if cr else b"\n", "clean_open" if final else "no_quality", (), 0.0)
    if cr:
        head = pc.make_text(rng, rng.integers(0, 300, 200), b"\r\n", "clean", (), 0.0)
        quirky = b"".join(b"@q%d\rjunk\n" % i + b"ACGTN" * i + b"\rTTTT\r\n+\r+\n" + b"IIIII" * i + b"\r!!!!!!!\n" for i in range(60))
        text = head + quirky + text
    assert (b"\r" in text) == cr
    o = parse_device(eng, text, final, shift=5)
    n, nb = pc.assert_parse(o, text, final, round16=True, what=shape)
    assert n >= len(lens) and o["info"]["error"] == 0 and o["info"]["max_read_len"] >= int(lens.max())


def test_chunked_feed_equals_one_call(eng):
    rng = np.random.Generator(np.random.PCG64([71, SEED]))
    parse = lambda piece, final: parse_device(eng, piece, final)
    for rnd in range(8):
        eol = (b"\n", b"\r\n")[rnd % 2]
        n = int(rng.integers(500, 3000))
        text = pc.make_text(rng, rng.integers(0, 200, n), eol, pc.TAILS[rnd % len(pc.TAILS)], {n - 3} if rnd == 5 else (), 0.0)
        nls = np.nonzero(np.frombuffer(text, np.uint8) == 10)[0]
        cuts = set(rng.integers(0, len(text) + 1, 5).tolist())
        for i in rng.choice(nls, 2, replace=False).tolist():
            cuts.add(i + 1)
            if eol == b"\r\n":
                cuts.add(i)
        seq, qual, offset, tn, dpos, dlen, consumed, error = driver.parse_model(text, True)
        want = [(int(dpos[k]), int(dlen[k]), bytes(seq[offset[k]:offset[k + 1]]), bytes(qual[offset[k]:offset[k + 1]]), int(tn[k])) for k in range(len(tn))]
        assert pc.chunked(parse, text, sorted(cuts)) == (want, consumed, error), "round %d" % rnd


def test_overflow_writes_nothing_but_info(eng):
    """Two of the three causes can be reached: too few bytes, too few reads.  The third, n_bytes >= 2^32, cannot be produced by a text
    below 2^32 bytes (an arena takes less than half of its text) and is a guard only."""
    rng = np.random.Generator(np.random.PCG64([73, SEED]))
    text = pc.make_text(rng, rng.integers(1, 300, 3000), b"\n", "clean")
    want = driver.parse_model(text, True)
    n, nb = len(want[2]) - 1, len(want[0])
    for cb, cr in ((nb - 1, n), (nb, n - 1), (0, 0), (nb + 5000, 7), (16, n + 100)):
        o = parse_device(eng, text, True, cap_bytes=cb, cap_reads=cr)
        assert o["info"] == {"n_bytes": nb, "consumed": len(text), "n_reads": n, "max_read_len": int(np.diff(want[2].astype(np.int64)).max()), "overflow": 1, "error": 0}
        assert (o["seq"] == pc.CANARY).all() and (o["qual"] == pc.CANARY).all() and (o["offset"] == pc.CAN32).all() and (o["terminal_n"] == pc.CANARY).all()
        assert (o["def_pos"] == pc.CAN32).all() and (o["def_len"] == pc.CAN32).all()
    pc.assert_parse(parse_device(eng, text, True, cap_bytes=nb, cap_reads=n), text, True, round16=True)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_length_mismatch_delivers_what_lies_in_front(eng, where, eol):
    rng = np.random.Generator(np.random.PCG64([79, len(where), len(eol), SEED]))
    n = 5000
    bad = {"first": 0, "middle": 2777, "last": n - 1}[where]
    text = pc.make_text(rng, rng.integers(0, 300, n), eol, "clean", {bad, min(bad + 600, n - 1)})
    for final in (True, False):
        o = parse_device(eng, text, final)
        pc.assert_parse(o, text, final, round16=True)
        assert (o["info"]["error"], o["info"]["n_reads"]) == (capi.PARSE_E_LENGTH, bad)


@pytest.mark.parametrize("tail", pc.TAILS)
def test_tail_errors(eng, tail):
    rng = np.random.Generator(np.random.PCG64([83, pc.TAILS.index(tail), SEED]))
    text = pc.make_text(rng, rng.integers(0, 300, 1500), b"\n", tail)
    for final in (True, False):
        o = parse_device(eng, text, final)
        pc.assert_parse(o, text, final, round16=True)
        assert o["info"]["error"] == (pc.TAIL_ERROR[tail] if final else 0) and o["info"]["n_reads"] >= 1499


def test_argument_checks(eng):
    import torch

    dev = torch.device("cuda:0")
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    assert base % 16 == 0

    def out(**kw):
        f = dict(seq=base + 256, qual=base + 512, capacity_bytes=64, capacity_reads=4, offset=base + 1024, terminal_n=base + 1280,
                 def_pos=base + 1536, def_len=base + 1792, info=base + 2048)
        f.update(kw)
        return capi.ParseOut(**f)

    lib = eng.lib
    for bad in (out(seq=base + 260), out(qual=base + 520), out(def_pos=None), out(def_len=None), out(info=None), out(terminal_n=None), out(offset=None)):
        assert lib.faqcs_parse_device(eng.ctx, base + 3072, 100, 1, C.byref(bad)) == capi.E_INVAL
    assert lib.faqcs_parse_device(eng.ctx, base + 3072, 1 << 32, 1, C.byref(out())) == capi.E_INVAL
    assert lib.faqcs_parse_device(eng.ctx, None, 100, 1, C.byref(out())) == capi.E_INVAL
    assert lib.faqcs_parse_device(eng.ctx, base + 3072, 100, 1, None) == capi.E_INVAL
    eng.sync()
    assert int(buf.sum()) == 0


@pytest.mark.parametrize("args", [[], ["--adapter", "--polyA"], ["--replace_to_N_q", "15"]], ids=lambda a: " ".join(a) or "default")
def test_round_trip_parse_submit_emit(args):
    """The three-call device pipeline.  The parse output, with its terminal_n, goes straight into faqcs_submit_device: per-read results and the
    counter block equal the ORACLE's on the same reads; faqcs_emit_device on it equals driver.emit_model fed with the oracle's results."""
    import torch
    from oracle_engine import OracleEngine

    from faqcs_amd.engine import HipEngine, _check

    rng = np.random.Generator(np.random.PCG64([89, len(args), SEED]))
    n = 700 if "--adapter" in args else 3000
    reads = random_batch(rng, n, 150, "adv")
    text = b"".join(b"@r%d\n" % i + s + b"\n+\n" + q + b"\n" for i, (d, s, q) in enumerate(reads))
    opt = parse_args(["-u", "x", "-d", "y", "--ascii", "33"] + args)
    hip, ora = HipEngine(opt, 256, 33, device=0), OracleEngine(opt, 256, 33)
    o = parse_device(hip, text, True, keep=True)
    assert (o["info"]["n_reads"], o["info"]["error"], o["info"]["overflow"]) == (n, 0, 0)
    seq, qual, offset, seg = driver.pack_segments([reads[i:i + 517] for i in range(0, n, 517)])
    want = ora.process(seq, qual, offset, seg)
    dev = torch.device("cuda:0")
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    b = capi.Batch(o["d_seq"].data_ptr() + pc.FRONT, o["d_qual"].data_ptr() + pc.FRONT, o["d_off"].data_ptr(), n, len(seg) - 1, seg.ctypes.data,
                   o["info"]["max_read_len"], o["d_tn"].data_ptr())
    _check(hip.lib, hip.lib.faqcs_submit_device(hip.ctx, C.byref(b), res.data_ptr()))
    hip.sync()
    got = res.cpu().numpy().view(np.uint16).view(capi.RESULT_DTYPE).ravel()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "first differing read %d: hip=%s oracle=%s" % (bad[0], got[bad[0]], want[bad[0]])
    assert (hip.counters() == ora.counters()).all()
    es, eq, eoff, eidx = driver.emit_model(opt, 33, seq, qual, offset, want)
    cap = int(offset[-1])
    e_seq = torch.full((pc.FRONT + cap + capi.ARENA_PAD_AFTER,), pc.CANARY, dtype=torch.uint8, device=dev)
    e_qual = torch.full_like(e_seq, pc.CANARY)
    e_off, e_idx = torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    e_info = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    eout = capi.EmitOut(e_seq.data_ptr() + pc.FRONT, e_qual.data_ptr() + pc.FRONT, cap, e_off.data_ptr(), e_idx.data_ptr(), e_info.data_ptr())
    hip.emit_device(b, res.data_ptr(), eout)
    hip.sync()
    h = e_info.cpu().numpy().view(np.uint64)
    assert (int(h[0]), int(h[1] & np.uint64(0xFFFFFFFF)), int(h[1] >> np.uint64(32))) == (len(es), len(eidx), 0)
    assert (e_off.cpu().numpy().view(np.uint32)[:len(eidx) + 1] == eoff).all() and (e_idx.cpu().numpy().view(np.uint32)[:len(eidx)] == eidx).all()
    assert (e_seq.cpu().numpy()[pc.FRONT:pc.FRONT + len(es)] == es).all() and (e_qual.cpu().numpy()[pc.FRONT:pc.FRONT + len(eq)] == eq).all()
    hip.close()


def test_text_just_below_2_32_bytes(eng):
    """A device-built text of 321-byte records whose end lies just below 2^32: n_reads, n_bytes, consumed exact; the records at the start, either
    side of text position 2^31 and at the end against the model on those slices of the text."""
    import torch

    from tools.parse_bench import parse_buffers, read_info, record_bytes, synth_text

    L = 150
    R = record_bytes(L)
    n = ((1 << 32) - 1) // R
    dev = torch.device("cuda:0")
    store, n_text, s2, q2 = synth_text(eng.lib, dev, n, L)
    del s2, q2
    assert (1 << 32) - R <= n_text < (1 << 32)
    out, t = parse_buffers(dev, n * L, n)
    torch.cuda.synchronize()
    eng.parse_device(store.data_ptr() + 64, n_text, True, out)
    eng.sync()
    assert read_info(t["info"]) == {"n_bytes": n * L, "consumed": n_text, "n_reads": n, "max_read_len": L, "overflow": 0, "error": 0}
    mid = (1 << 31) // R
    for k0, k1 in ((0, 1000), (mid - 500, mid + 500), (n - 1000, n)):
        piece = store[64 + k0 * R:64 + k1 * R].cpu().numpy().tobytes()
        seq, qual, offset, tn, dpos, dlen, consumed, error = driver.parse_model(piece, True)
        m = k1 - k0
        assert (len(offset) - 1, consumed, error) == (m, m * R, 0)
        assert (t["seq"][64 + k0 * L:64 + k1 * L].cpu().numpy() == seq).all() and (t["qual"][64 + k0 * L:64 + k1 * L].cpu().numpy() == qual).all()
        assert (t["offset"][k0:k1 + 1].cpu().numpy().view(np.uint32).astype(np.int64) == offset.astype(np.int64) + k0 * L).all()
        assert (t["terminal_n"][k0:k1].cpu().numpy() == tn).all()
        assert (t["def_pos"][k0:k1].cpu().numpy().view(np.uint32).astype(np.int64) == dpos.astype(np.int64) + k0 * R).all()
        assert (t["def_len"][k0:k1].cpu().numpy().view(np.uint32) == dlen).all()
    # the offsets as a whole: record k starts at k x L
    off = t["offset"][:n + 1].to(torch.int64) & 0xFFFFFFFF
    assert bool((off == torch.arange(n + 1, device=dev, dtype=torch.int64) * L).all())


def test_parse_is_not_serialised(eng):
    """A condition, not a measurement: on a device-built text of about 1 GiB of 2x150-shaped records the median of 5 HIP-event timings of
    faqcs_parse_device stays below 6 x the median time of a torch device-to-device copy of the same text in the same process.  The yardstick
    is the copy; 6 is twice the median ratio tools/parse_bench.py measured on the MI355X (2.79, profiles/parse/parse_bench.json, DESIGN.md
    section 4.6), rounded up -- the factor 2 is for a shared machine."""
    import torch

    from tools.parse_bench import parse_buffers, read_info, record_bytes, synth_text

    L = 150
    R = record_bytes(L)
    n = (1 << 30) // R
    dev = torch.device("cuda:0")
    store, n_text, s2, q2 = synth_text(eng.lib, dev, n, L)
    del s2, q2
    out, t = parse_buffers(dev, n * L, n)
    dst = torch.empty(n_text, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    parse_ms, copy_ms = [], []
    for rep in range(6):  # the first round warms both up
        eng.parse_device(store.data_ptr() + 64, n_text, True, out)
        eng.sync()
        parse_ms.append(sum(eng.parse_time_ms()))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(store[64:64 + n_text])
        e1.record()
        torch.cuda.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    pm, cp = float(np.median(parse_ms[1:])), float(np.median(copy_ms[1:]))
    print("faqcs_parse_device %.3f ms, copy of the text %.3f ms, ratio %.2f" % (pm, cp, pm / cp))
    assert read_info(t["info"]) == {"n_bytes": n * L, "consumed": n_text, "n_reads": n, "max_read_len": L, "overflow": 0, "error": 0}
    assert pm <= 6.0 * cp, "faqcs_parse_device %.3f ms vs %.3f ms for the copy of the text" % (pm, cp)
