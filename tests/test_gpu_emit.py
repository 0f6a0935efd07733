"""faqcs_emit_device on an MI355X: the trimmed, edited reads packed on the device, against the numpy model (driver.emit_model) fed with the
ORACLE's per-read results -- never the HIP results, which are asserted equal to the oracle's besides -- and, for pair routing, against the
reference's own output files (the md5s of the golden cases)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args
from test_gpu_parity import OPTION_SETS, SEED, random_batch

pytestmark = pytest.mark.gpu

CANARY = 0xA5
FRONT = 64  # canary bytes in front of the output arenas (>= FAQCS_ARENA_PAD_BEFORE, keeps them 16-byte aligned)

# the option sets of the parity test that test_gpu_parity has too ...
_SHARED = [[], ["--replace_to_N_q", "15"], ["--replace_to_N_q", "30", "--lc", "0.4", "-n", "4"], ["--out_ascii", "64"], ["--qc_only"],
           ["--adapter", "--polyA"], ["--5end", "3", "--3end", "5"], ["-q", "0", "--min_L", "1"]]
assert all(s in OPTION_SETS for s in _SHARED)
# ... the Phred+64 input, and one set that keeps reads with long N runs at their ends
EMIT_SETS = _SHARED + [["--ascii", "64", "--out_ascii", "33"], ["-n", "7", "--min_L", "1"]]
SHAPES = [("adv", 150), ("ragged", 64), ("ragged", 250), ("adv", 1024), ("ragged", 6000)]

_A = b"ACGTTGCATCAGGATC" * 5  # 80 bases, no low-complexity filter
# empty; one base; all N; an N run at the start only; at the end only; at both ends with a low-quality G between (Phred+33)
HAND = [(b"@h0", b"", b""), (b"@h1", b"A", b"I"), (b"@h2", b"N" * 70, b"5" * 70), (b"@h3", b"N" + _A, b"I" * 81),
        (b"@h4", _A + b"NN", b"I" * 82), (b"@h5", b"N" + _A[:40] + b"G" + _A[40:] + b"N", b"I" * 41 + b"$" + b"I" * 41)]


def in_offset(args):
    return 64 if "--ascii" in args else 33


def rebase(reads, in_off):
    """Reads written in Phred+33 as the engine's input offset wants them."""
    if in_off == 33:
        return list(reads)
    up = bytes(min(255, c + in_off - 33) for c in range(256))
    return [(d, s, q.translate(up)) for d, s, q in reads]


class DeviceBatch:
    """A packed host batch copied to the GPU under the padding contract of faqcs_batch."""

    def __init__(self, seq, qual, offset, seg, with_tn=True):
        import torch

        self.dev = torch.device("cuda:0")
        self.n = len(offset) - 1
        self.total = int(offset[-1])
        self.h_seq, self.h_qual, self.h_offset, self.seg = seq, qual, np.ascontiguousarray(offset, dtype=np.uint32), np.ascontiguousarray(seg, dtype=np.uint32)
        self.seq = torch.zeros(64 + self.total + 64, dtype=torch.uint8, device=self.dev)
        self.qual = torch.zeros(64 + self.total + 64, dtype=torch.uint8, device=self.dev)
        if self.total:
            self.seq[64:64 + self.total] = torch.from_numpy(np.array(seq[:self.total])).to(self.dev)
            self.qual[64:64 + self.total] = torch.from_numpy(np.array(qual[:self.total])).to(self.dev)
        self.off = torch.from_numpy(self.h_offset.view(np.int32).copy()).to(self.dev)
        self.res = torch.zeros((max(self.n, 1), 4), dtype=torch.int16, device=self.dev)
        self.h_tn = driver.terminal_n_flags(seq, self.h_offset) if self.n else np.zeros(0, np.uint8)
        self.tn = torch.from_numpy(np.concatenate([self.h_tn, np.zeros(1, np.uint8)])).to(self.dev)
        torch.cuda.synchronize()

    def batch(self, max_len, tn=True):
        return capi.Batch(self.seq.data_ptr() + 64, self.qual.data_ptr() + 64, self.off.data_ptr(), self.n, len(self.seg) - 1,
                          self.seg.ctypes.data, max_len, self.tn.data_ptr() if tn and self.n else None)

    def submit(self, eng, max_len):
        from faqcs_amd.engine import _check

        b = self.batch(max_len)
        _check(eng.lib, eng.lib.faqcs_submit_device(eng.ctx, C.byref(b), self.res.data_ptr()))
        eng.sync()
        return self.res[:self.n].cpu().numpy().view(np.uint16).view(capi.RESULT_DTYPE).ravel()


def emit(eng, db, max_len, keep=None, tn=True, with_index=True, capacity=None):
    """One faqcs_emit_device into canary-filled buffers; everything comes back as host arrays (the WHOLE buffers)."""
    import torch

    cap = db.total if capacity is None else capacity
    o_seq = torch.full((FRONT + max(cap, 0) + capi.ARENA_PAD_AFTER,), CANARY, dtype=torch.uint8, device=db.dev)
    o_qual = torch.full_like(o_seq, CANARY)
    o_off = torch.full((db.n + 1,), -0x5A5A5A5B, dtype=torch.int32, device=db.dev)
    o_idx = torch.full((max(db.n, 1),), -0x5A5A5A5B, dtype=torch.int32, device=db.dev)
    info = torch.full((2,), -1, dtype=torch.int64, device=db.dev)
    d_keep = torch.from_numpy(np.concatenate([np.asarray(keep, np.uint8), np.zeros(1, np.uint8)])).to(db.dev) if keep is not None else None
    torch.cuda.synchronize()
    assert (o_seq.data_ptr() + FRONT) % 16 == 0 and (o_qual.data_ptr() + FRONT) % 16 == 0
    out = capi.EmitOut(o_seq.data_ptr() + FRONT, o_qual.data_ptr() + FRONT, max(cap, 0), o_off.data_ptr(), o_idx.data_ptr() if with_index else None, info.data_ptr())
    b = db.batch(max_len, tn)
    eng.emit_device(b, db.res.data_ptr(), out, d_keep.data_ptr() if d_keep is not None else None)
    eng.sync()
    h = info.cpu().numpy().view(np.uint64)
    return {"seq": o_seq.cpu().numpy(), "qual": o_qual.cpu().numpy(), "offset": o_off.cpu().numpy().view(np.uint32), "index": o_idx.cpu().numpy().view(np.uint32),
            "n_bytes": int(h[0]), "n_reads": int(h[1] & np.uint64(0xFFFFFFFF)), "overflow": int(h[1] >> np.uint64(32)), "cap": cap,
            "d_seq": o_seq, "d_qual": o_qual, "d_off": o_off, "with_index": with_index, "n": db.n}


CAN32 = np.uint32(0xA5A5A5A5)


def assert_untouched(o, nb, ne):
    """Canaries: everything outside [0, round_up(nb, 16)) of the arenas, offset[ne + 1 ..], index[ne ..]."""
    r16 = (nb + 15) // 16 * 16
    for name in ("seq", "qual"):
        assert (o[name][:FRONT] == CANARY).all(), name + ": bytes in front of the arena were written"
        assert (o[name][FRONT + r16:] == CANARY).all(), name + ": bytes behind the emission were written"
    assert (o["offset"][ne + 1:] == CAN32).all(), "offset[] behind the emitted reads was written"
    assert (o["index"][ne if o["with_index"] else 0:] == CAN32).all(), "index[] behind the emitted reads was written"


def assert_emission(o, want, what=""):
    es, eq, eoff, eidx = want
    nb, ne = len(es), len(eidx)
    assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (nb, ne, 0), what
    assert (o["offset"][:ne + 1] == eoff).all(), what
    if o["with_index"]:
        assert (o["index"][:ne] == eidx).all(), what
    for name, w in (("seq", es), ("qual", eq)):
        got = o[name][FRONT:FRONT + nb]
        bad = np.nonzero(got != w)[0]
        assert len(bad) == 0, "%s %s: first differing byte %d of %d (emitted read %d): got %r want %r" % (
            what, name, bad[0], nb, int(np.searchsorted(eoff, bad[0], side="right")) - 1, bytes(got[bad[0]:bad[0] + 8]), bytes(w[bad[0]:bad[0] + 8]))
    assert_untouched(o, nb, ne)


def engines(opt, R, in_off):
    from oracle_engine import OracleEngine

    from faqcs_amd.engine import HipEngine

    return HipEngine(opt, R, in_off, device=0), OracleEngine(opt, R, in_off)


def oracle_and_hip(opt, reads, R, in_off, seg_size):
    """Packs, runs both engines (device-resident submission on the HIP side), asserts their per-read results and counter blocks equal."""
    bufs = [reads[i:i + seg_size] for i in range(0, len(reads), seg_size)] or [[]]
    seq, qual, offset, seg = driver.pack_segments(bufs)
    hip, ora = engines(opt, R, in_off)
    want = ora.process(seq, qual, offset, seg)
    db = DeviceBatch(seq, qual, offset, seg)
    got = db.submit(hip, R)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "first differing read %d: hip=%s oracle=%s" % (bad[0], got[bad[0]], want[bad[0]])
    assert (hip.counters() == ora.counters()).all()
    return hip, db, want


def check_variants(opt, in_off, hip, db, want_res, R, rng, what):
    keep = (rng.random(db.n) < 0.6).astype(np.uint8)
    for kp, tn, with_index in ((None, True, True), (None, False, False), (keep, True, True), (keep, False, True)):
        want = driver.emit_model(opt, in_off, db.h_seq, db.h_qual, db.h_offset, want_res, kp)
        o = emit(hip, db, R, keep=kp, tn=tn, with_index=with_index)
        assert_emission(o, want, "%s keep=%s terminal_n=%s index=%s" % (what, kp is not None, tn, with_index))


@pytest.mark.parametrize("args", EMIT_SETS, ids=lambda a: " ".join(a) or "default")
@pytest.mark.parametrize("kind,maxlen", SHAPES)
def test_emission_matches_model_on_oracle_results(args, kind, maxlen):
    rng = np.random.Generator(np.random.PCG64([17, len(kind), maxlen, EMIT_SETS.index(args), SEED]))
    opt = parse_args(["-u", "x", "-d", "y"] + args)
    in_off = in_offset(args)
    n = {150: 3000, 64: 3000, 250: 3000, 1024: 500, 6000: 120}[maxlen]
    if "--adapter" in args:
        n = max(n // 4, 40)
    reads = rebase(random_batch(rng, n, maxlen, kind) + HAND, in_off)
    R = 256 if maxlen <= 250 else (1024 if maxlen <= 1024 else capi.MAX_READ_LENGTH)
    hip, db, res = oracle_and_hip(opt, reads, R, in_off, seg_size=517)
    # the edit paths are not passed vacuously: the oracle keeps reads whose first / last base is 'N'
    valid = (res["flags"] & capi.F_VALID) != 0
    assert int((valid & ((db.h_tn & 1) != 0)).sum()) >= 1 and int((valid & ((db.h_tn & 2) != 0)).sum()) >= 1
    check_variants(opt, in_off, hip, db, res, R, rng, "%s/%d %s" % (kind, maxlen, args))


@pytest.mark.parametrize("args", [[], ["--qc_only"], ["--mode", "BWA", "--min_L", "1", "--replace_to_N_q", "20"]], ids=["default", "qc_only", "bwa_replaceN"])
def test_emission_of_the_longest_reads(args):
    """The three reads of test_longest_read: 32 767 random bases, 32 767 x 'N' (emitted under --qc_only: the longest end scan there is), 120 bases."""
    L = capi.MAX_READ_LENGTH
    rng = np.random.Generator(np.random.PCG64([L, SEED]))
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)]
    q = rng.integers(5, 42, L) + 33
    q[L - 900:] = 35
    reads = [(b"@e", s.tobytes(), q.astype(np.uint8).tobytes()), (b"@e", b"N" * L, bytes([33 + 20] * L)), (b"@e", b"ACGT" * 30, bytes([70] * 120))]
    opt = parse_args(["-u", "x", "-d", "y"] + args)
    hip, db, res = oracle_and_hip(opt, reads, L, 33, seg_size=1)
    assert (res["flags"] & capi.F_VALID).sum() >= (3 if "--qc_only" in args else 2)
    check_variants(opt, 33, hip, db, res, L, rng, "longest %s" % args)


def _adv_case(args, n=3000, seed=3):
    rng = np.random.Generator(np.random.PCG64([23, seed, SEED]))
    opt = parse_args(["-u", "x", "-d", "y"] + args)
    reads = random_batch(rng, n, 150, "adv") + HAND
    hip, db, res = oracle_and_hip(opt, reads, 256, 33, seg_size=517)
    return opt, hip, db, res, rng


def test_nothing_else_is_written():
    """Canary-filled output buffers much larger than the emission: only [0, round_up(n_bytes, 16)), offset[0 .. n] and index[0 .. n) change."""
    opt, hip, db, res, rng = _adv_case(["--replace_to_N_q", "15"])
    keep = (rng.random(db.n) < 0.3).astype(np.uint8)
    want = driver.emit_model(opt, 33, db.h_seq, db.h_qual, db.h_offset, res, keep)
    assert 0 < len(want[0]) < db.total // 2
    o = emit(hip, db, 256, keep=keep, capacity=2 * db.total + 12345)
    assert_emission(o, want)


def test_overflow_writes_nothing():
    opt, hip, db, res, rng = _adv_case([])
    want = driver.emit_model(opt, 33, db.h_seq, db.h_qual, db.h_offset, res)
    nb, ne = len(want[0]), len(want[3])
    assert nb > 1000
    o = emit(hip, db, 256, capacity=nb - 1)
    assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (nb, ne, 1)
    for name in ("seq", "qual"):
        assert (o[name] == CANARY).all(), name + " was written in spite of the overflow"
    assert (o["offset"][1:] == CAN32).all() and o["offset"][0] in (0, CAN32)
    assert (o["index"] == CAN32).all()
    # ... and the exact capacity is enough
    assert_emission(emit(hip, db, 256, capacity=nb), want)


def test_empty_and_all_filtered_batches():
    opt = parse_args(["-u", "x", "-d", "y"])
    for reads in ([], [(b"@s", b"ACGT" * 3, b"I" * 12)] * 700):  # no reads at all; 700 reads shorter than --min_L
        hip, db, res = oracle_and_hip(opt, reads, 256, 33, seg_size=300)
        assert not (res["flags"] & capi.F_VALID).any()
        for tn in (True, False):
            o = emit(hip, db, 256, tn=tn)
            assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (0, 0, 0)
            assert o["offset"][0] == 0
            assert_untouched(o, 0, 0)
    # a batch with valid reads and a keep mask of zeros
    opt, hip, db, res, rng = _adv_case([], n=600)
    assert (res["flags"] & capi.F_VALID).sum() > 100
    o = emit(hip, db, 256, keep=np.zeros(db.n, np.uint8))
    assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (0, 0, 0) and o["offset"][0] == 0
    assert_untouched(o, 0, 0)


@pytest.mark.parametrize("name", ["adv_default", "adv_replaceN15", "adv_adapter_polyA", "adv_out64", "adv64_ascii64_out33"])
def test_pair_routing_reproduces_the_reference_files(name, fixture_cache, tmp_path):
    """The reference's three trimmed FASTQ files (FaQCs.cpp:296-361) from three emissions with torch-made keep masks: valid1 & valid2 for the
    two paired streams, valid1 ^ valid2 for the unpaired one, whose records are merged by pair index through `index`."""
    import torch

    import golden_util
    import make_fixtures

    from faqcs_amd.device import trimmed_reads
    from oracle_engine import OracleEngine

    from faqcs_amd.engine import HipEngine

    case = golden_util.load_case(name)
    p1, p2 = golden_util.fixture_paths(case["fixture"], fixture_cache)
    m = {"{1}": p1, "{2}": p2, "{U}": p1, "{D}": str(tmp_path)}
    opt = parse_args([m.get(a, a) for a in case["args"]])
    r1, r2 = make_fixtures.read_fastq(p1), make_fixtures.read_fastq(p2)
    assert len(r1) == len(r2) <= driver.BUFFER_SIZE  # one 32 768-record buffer per mate: two segments
    in_off = opt.input_quality_offset
    if in_off == driver.AUTO_DETECT_QUALITY_OFFSET:
        in_off = driver.auto_detect_quality_offset([r[2] for r in r1])
    seq, qual, offset, seg = driver.pack_segments([r1, r2])
    hip, ora = HipEngine(opt, 1024, in_off, device=0), OracleEngine(opt, 1024, in_off)
    db = DeviceBatch(seq, qual, offset, seg)
    got = db.submit(hip, 1024)
    assert (got == ora.process(seq, qual, offset, seg)).all()
    np_, deflines = len(r1), [r[0] for r in r1 + r2]
    valid = (db.res[:db.n, 2] & 1) != 0
    v1, v2 = valid[:np_], valid[np_:]
    zeros = torch.zeros_like(v1)
    masks = {"QC.1.trimmed.fastq": torch.cat([v1 & v2, zeros]), "QC.2.trimmed.fastq": torch.cat([zeros, v1 & v2]),
             "QC.unpaired.trimmed.fastq": torch.cat([v1 ^ v2, v1 ^ v2])}
    d_seq, d_qual = db.seq[64:64 + db.total], db.qual[64:64 + db.total]
    for fn, keep in masks.items():
        s, q, off, idx = trimmed_reads(hip, d_seq, d_qual, db.off, db.res, keep=keep, terminal_n=db.tn)
        s, q, off, idx = s.cpu().numpy().tobytes(), q.cpu().numpy().tobytes(), off.cpu().numpy().view(np.uint32), idx.cpu().numpy().view(np.uint32)
        order = np.argsort(idx % np_, kind="stable") if "unpaired" in fn else np.arange(len(idx))
        text = b"".join(deflines[idx[k]] + b"\n" + s[off[k]:off[k + 1]] + b"\n+\n" + q[off[k]:off[k + 1]] + b"\n" for k in order)
        meta = case["fastq"][fn]
        assert len(idx) == meta["records"] and len(text) == meta["bytes"], fn
        assert hashlib.md5(text).hexdigest() == meta["md5"], fn


def test_emitted_arenas_feed_a_second_submission():
    """(seq, qual, offset, n_reads) of an emission, 16 bytes left in front, is a valid faqcs_submit_device batch: a fresh engine's results
    and counter block on it equal the oracle's on the same bytes copied to the host."""
    from faqcs_amd.engine import _check

    opt, hip, db, res, rng = _adv_case(["--5end", "3", "--3end", "5"], seed=9)
    o = emit(hip, db, 256)
    nb, ne = o["n_bytes"], o["n_reads"]
    assert ne > 500 and o["overflow"] == 0
    opt2 = parse_args(["-u", "x", "-d", "y", "-q", "20", "--min_L", "30"])
    hip2, ora2 = engines(opt2, 256, 33)
    import torch

    res2 = torch.zeros((ne, 4), dtype=torch.int16, device=db.dev)
    seg = np.array([0, ne], dtype=np.uint32)
    b = capi.Batch(o["d_seq"].data_ptr() + FRONT, o["d_qual"].data_ptr() + FRONT, o["d_off"].data_ptr(), ne, 1, seg.ctypes.data, 256, None)
    _check(hip2.lib, hip2.lib.faqcs_submit_device(hip2.ctx, C.byref(b), res2.data_ptr()))
    hip2.sync()
    got = res2.cpu().numpy().view(np.uint16).view(capi.RESULT_DTYPE).ravel()
    pad = np.zeros(64, np.uint8)
    hs = np.concatenate([pad, o["seq"][FRONT:FRONT + nb], pad])[64:]
    hq = np.concatenate([pad, o["qual"][FRONT:FRONT + nb], pad])[64:]
    want = ora2.process(hs, hq, o["offset"][:ne + 1].copy(), seg)
    assert (got == want).all()
    assert (hip2.counters() == ora2.counters()).all()


def _synth_batch(lib, n, L):
    """n equal-length device-synthesised reads (faqcs_synth_fill) and their offsets; the arenas proper start 64 bytes in."""
    import torch

    from test_gpu_parity import _fill_arenas

    dev = torch.device("cuda:0")
    seq, qual = _fill_arenas(lib, dev, n * L, L)
    off_host = (np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32)
    off = torch.from_numpy(off_host.view(np.int32)).to(dev)
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    return dev, seq, qual, off, res


def test_emission_past_2_31_bytes():
    """17.5 M synthesised 150-base reads (the default options keep 88 % of their bytes): the emitted bytes pass 2^31, so every 32-bit offset
    computation is exercised with the top bit set."""
    import torch

    from faqcs_amd.engine import HipEngine, _check

    n, L = 17_500_000, 150
    opt = parse_args(["-u", "x", "-d", "y", "--ascii", "33"])
    eng = HipEngine(opt, 256, 33, device=0)
    dev, seq, qual, off, res = _synth_batch(eng.lib, n, L)
    seg = np.array([0, n], dtype=np.uint32)
    b = capi.Batch(seq.data_ptr() + 64, qual.data_ptr() + 64, off.data_ptr(), n, 1, seg.ctypes.data, L, None)
    _check(eng.lib, eng.lib.faqcs_submit_device(eng.ctx, C.byref(b), res.data_ptr()))
    eng.sync()
    cap = n * L
    o_seq = torch.empty(FRONT + cap + 64, dtype=torch.uint8, device=dev)
    o_qual = torch.empty_like(o_seq)
    o_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    o_idx = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    out = capi.EmitOut(o_seq.data_ptr() + FRONT, o_qual.data_ptr() + FRONT, cap, o_off.data_ptr(), o_idx.data_ptr(), info.data_ptr())
    eng.emit_device(b, res.data_ptr(), out)
    eng.sync()
    h = info.cpu().numpy().view(np.uint64)
    n_bytes, n_emit, overflow = int(h[0]), int(h[1] & np.uint64(0xFFFFFFFF)), int(h[1] >> np.uint64(32))
    lens = res[:, 1].to(torch.int64) & 0xFFFF
    valid = (res[:, 2] & 1) != 0
    assert overflow == 0 and n_emit == int(valid.sum()) and n_bytes == int(lens[valid].sum())
    assert n_bytes > 1 << 31, "the premise of this test: the emission passes 2^31 bytes (%d)" % n_bytes
    eo = o_off[:n_emit + 1].to(torch.int64) & 0xFFFFFFFF
    assert int(eo[0]) == 0 and int(eo[n_emit]) == n_bytes and bool((eo[1:] >= eo[:-1]).all())
    assert bool((o_idx[:n_emit].to(torch.int64) == torch.nonzero(valid).ravel()).all())
    # 10 000 emitted reads, the first and last thousands and the ones around 2^31 among them, against the model on their source reads
    rng = np.random.Generator(np.random.PCG64([31, SEED]))
    mid = int(torch.searchsorted(eo, torch.tensor([1 << 31], device=dev))[0])
    ks = np.unique(np.concatenate([np.arange(1000), np.arange(n_emit - 1000, n_emit), np.arange(mid - 500, mid + 500), rng.integers(0, n_emit, 7000)]))
    kt = torch.from_numpy(ks).to(dev)
    it = o_idx[:n_emit][kt].to(torch.int64)
    src_s = seq[64:64 + n * L].view(n, L)[it].cpu().numpy()
    src_q = qual[64:64 + n * L].view(n, L)[it].cpu().numpy()
    res_s = res[it].cpu().numpy().view(np.uint16).view(capi.RESULT_DTYPE).ravel()
    pad = np.zeros(64, np.uint8)
    es, eq, eoff, eidx = driver.emit_model(opt, 33, np.concatenate([src_s.ravel(), pad]), np.concatenate([src_q.ravel(), pad]),
                                           (np.arange(len(ks) + 1, dtype=np.uint64) * L).astype(np.uint32), res_s)
    assert len(eidx) == len(ks)  # every sampled read is an emitted one
    a, e = eo[kt], eo[kt + 1]
    assert ((e - a).cpu().numpy() == np.diff(eoff.astype(np.int64))).all()
    flat = torch.repeat_interleave(a - torch.from_numpy(eoff[:-1].astype(np.int64)).to(dev), e - a) + torch.arange(len(es), device=dev)
    assert (o_seq[FRONT + flat].cpu().numpy() == es).all()
    assert (o_qual[FRONT + flat].cpu().numpy() == eq).all()


def test_gather_is_not_serialised():
    """A condition, not a measurement: on 8 M synthesised 150-base reads, default options, the median of 5 HIP-event timings of
    faqcs_emit_device stays below 4 x the median time of a torch device-to-device copy of the two input arenas in the same process.  The
    yardstick is the copy; 4 x is loose on purpose and only catches an uncoalesced or per-read-serial gather."""
    import torch

    from faqcs_amd.engine import HipEngine, _check

    n, L = 8_000_000, 150
    opt = parse_args(["-u", "x", "-d", "y", "--ascii", "33"])
    eng = HipEngine(opt, 256, 33, device=0)
    dev, seq, qual, off, res = _synth_batch(eng.lib, n, L)
    seg = np.array([0, n], dtype=np.uint32)
    b = capi.Batch(seq.data_ptr() + 64, qual.data_ptr() + 64, off.data_ptr(), n, 1, seg.ctypes.data, L, None)
    _check(eng.lib, eng.lib.faqcs_submit_device(eng.ctx, C.byref(b), res.data_ptr()))
    eng.sync()
    cap = n * L
    o_seq = torch.empty(FRONT + cap + 64, dtype=torch.uint8, device=dev)
    o_qual = torch.empty_like(o_seq)
    o_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    o_idx = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    out = capi.EmitOut(o_seq.data_ptr() + FRONT, o_qual.data_ptr() + FRONT, cap, o_off.data_ptr(), o_idx.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    emit_ms, copy_ms = [], []
    for rep in range(6):  # the first round warms both up
        eng.emit_device(b, res.data_ptr(), out)
        eng.sync()
        emit_ms.append(sum(eng.emit_time_ms()))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o_seq[FRONT:FRONT + cap].copy_(seq[64:64 + cap])
        o_qual[FRONT:FRONT + cap].copy_(qual[64:64 + cap])
        e1.record()
        torch.cuda.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    em, cp = float(np.median(emit_ms[1:])), float(np.median(copy_ms[1:]))
    print("faqcs_emit_device %.3f ms, copy of both arenas %.3f ms, ratio %.2f" % (em, cp, em / cp))
    assert int(info.cpu().numpy()[0]) > cap // 2
    assert em < 4.0 * cp, "faqcs_emit_device %.3f ms vs %.3f ms for the copy of both arenas" % (em, cp)
