"""The decisions around trim() on an MI355X (faqcs_detect_device, faqcs_first_error_device, faqcs_set_input_quality_offset): the device
forms against the library's host statements (which tests/test_detect_model.py ties to the numpy models and to the existing helpers) on the
constructed catalogue of tests/detect_cases.py, with hostile bytes around every array and canaries around info; the argument checks; a
context whose offset is set after its creation against one created with it; and the paired chunk loop of INTEGRATION.md section 3.2 with
its detect, set and first-error steps on golden fixtures, from two device texts to the md5s of the reference's files."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import detect_cases as dc
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import AUTO_DETECT_QUALITY_OFFSET, DEFAULT_NEXTSEQ_QUALITY_SCORE, parse_args

pytestmark = pytest.mark.gpu

CANARY32 = -0x5A5A5A5B
PLACEHOLDER = 0  # the offset of a context that has not seen a quality byte yet


@pytest.fixture(scope="module")
def eng():
    from faqcs_amd.engine import HipEngine

    e = HipEngine(parse_args(["-1", "a", "-2", "b", "-d", "y"]), 1024, PLACEHOLDER, device=0)
    yield e
    e.close()


def _i32(dev, a, spare=1):
    import torch

    return torch.from_numpy(np.concatenate([np.asarray(a, np.uint32), np.zeros(spare, np.uint32)]).view(np.int32)).to(dev)


class DeviceDetect:
    """A detect_cases.DetectCase in device memory.  Arena position 0 lies `mis` bytes behind a multiple of 16; the bytes in front of the
    arena's padding and behind it are decisive too, and so are the 64 bytes around the text ("@NS@NS...")."""

    def __init__(self, dev, c, mis=0):
        import torch

        self.c = c
        buf = torch.full((16 + len(c.store) + 64,), dc.LO, dtype=torch.uint8, device=dev)
        k = (mis - buf.data_ptr() - dc.PAD_BEFORE) % 16
        buf[k:k + len(c.store)] = torch.from_numpy(c.store).to(dev)
        self.qual = buf.data_ptr() + k + dc.PAD_BEFORE
        assert self.qual % 16 == mis
        self.off = _i32(dev, c.offset)
        self.batch = capi.Batch(None, self.qual, self.off.data_ptr(), c.n, 0, None, 0, None)
        self.keep = [buf]
        self.text = self.def_pos = self.def_len = None
        if c.text is not None:
            h = np.resize(np.frombuffer(b"@NS", np.uint8), 64 + len(c.text) + 64).copy()
            h[64:64 + len(c.text)] = c.text
            t = torch.from_numpy(h).to(dev)
            dp, dl = _i32(dev, c.def_pos), _i32(dev, c.def_len)
            self.text, self.def_pos, self.def_len = t.data_ptr() + 64, dp.data_ptr(), dl.data_ptr()
            self.keep += [t, dp, dl]


def info_with_canaries(dev, words):
    import torch

    return torch.full((8 + words + 8,), CANARY32, dtype=torch.int32, device=dev)


def read_info(buf, words, struct):
    h = buf.cpu().numpy()
    assert (h[:8] == CANARY32).all() and (h[8 + words:] == CANARY32).all(), "bytes around info were written"
    return struct.from_buffer_copy(h[8:8 + words].tobytes())


def detect_dev(eng, d):
    import torch

    info = info_with_canaries(d.keep[0].device, 6)
    torch.cuda.synchronize()
    eng.detect_device(d.batch, d.c.first, d.c.count, info.data_ptr() + 32, d.text, d.def_pos, d.def_len)
    eng.sync()
    return dc.info_dict(read_info(info, 6, capi.DetectInfo))


def first_error_dev(eng, dev, c):
    """-> (n_good, flags); the results lie between two flagged results that belong to nobody (they have no padding: nothing outside [0, n) may be loaded, and what is outside would change the answer)"""
    import torch

    guard = np.zeros(4, capi.RESULT_DTYPE)
    guard["flags"] = capi.F_ERR_QUALITY | capi.F_ERR_BASE
    res = torch.from_numpy(np.concatenate([guard, c.res, guard]).view(np.int16).reshape(-1, 4)).to(dev)
    info = info_with_canaries(dev, 2)
    torch.cuda.synchronize()
    eng.first_error_device(res.data_ptr() + 32 if c.n else None, c.n, info.data_ptr() + 32)
    eng.sync()
    p = read_info(info, 2, capi.ErrorInfo)
    return int(p.n_good), int(p.flags)


def test_detect_device_equals_the_host_statement_on_every_case(eng):
    """Every case of the catalogue but the three large ones, with the arena 16-byte aligned and 5 bytes behind that: info equals
    faqcs_detect_host field for field, nothing around info is written, and the constructed expectation holds."""
    import torch

    dev = torch.device("cuda:0")
    first_raw = {}
    for mis in (0, 5):
        for c in dc.detect_cases():
            if c.big:
                continue
            got = detect_dev(eng, DeviceDetect(dev, c, mis))
            assert got == c.host(eng.lib), (c.name, mis)
            for k, v in c.expect.items():
                assert got[k] == v, (c.name, mis, k)
            assert first_raw.setdefault(c.name, got) == got


@pytest.mark.parametrize("name", ["big_last_tile", "big_tile0", "big_none"])
def test_detect_device_over_more_tiles_than_the_finishing_block_has_threads(eng, name):
    import torch

    c = [x for x in dc.detect_cases() if x.name == name][0]
    assert c.total > dc.FINISH_THREADS * dc.T
    got = detect_dev(eng, DeviceDetect(torch.device("cuda:0"), c))
    assert got == c.host(eng.lib)
    for k, v in c.expect.items():
        assert got[k] == v, k


def test_first_error_device_equals_the_host_statement_on_every_case(eng):
    import torch

    dev = torch.device("cuda:0")
    for c in dc.error_cases():
        if not c.big:
            assert first_error_dev(eng, dev, c) == c.host(eng.lib) == c.expect, c.name


@pytest.mark.parametrize("name", ["big_last_tile", "big_tile0", "big_none"])
def test_first_error_device_over_more_tiles_than_the_finishing_block_has_threads(eng, name):
    import torch

    c = [x for x in dc.error_cases() if x.name == name][0]
    assert c.n > dc.FINISH_THREADS * dc.T_RESULTS
    assert first_error_dev(eng, torch.device("cuda:0"), c) == c.host(eng.lib) == c.expect


def test_argument_errors_leave_the_context_usable(eng):
    """Every FAQCS_E_INVAL of the two device entry points is returned at call time (nothing is enqueued), and the context works afterwards."""
    import torch

    dev = torch.device("cuda:0")
    c = [x for x in dc.detect_cases() if x.name == "defline_@NS_first0_start"][0]
    d = DeviceDetect(dev, c)
    info = info_with_canaries(dev, 6)
    ip = info.data_ptr() + 32
    E, D, b = capi.E_INVAL, eng.lib.faqcs_detect_device, d.batch
    assert D(eng.ctx, None, 0, c.n, None, None, None, ip) == E and D(eng.ctx, C.byref(b), 0, c.n, None, None, None, None) == E
    assert D(eng.ctx, C.byref(b), 0, c.n + 1, None, None, None, ip) == E and D(eng.ctx, C.byref(b), c.n, 1, None, None, None, ip) == E
    assert D(eng.ctx, C.byref(b), 0xFFFFFFFF, 2, None, None, None, ip) == E
    for t, p, ln in ((d.text, None, None), (d.text, d.def_pos, None), (d.text, None, d.def_len), (None, d.def_pos, d.def_len), (None, None, d.def_len), (None, d.def_pos, None)):
        assert D(eng.ctx, C.byref(b), 0, c.n, t, p, ln, ip) == E
    for bad in (capi.Batch(None, None, d.off.data_ptr(), c.n, 0, None, 0, None), capi.Batch(None, d.qual, None, c.n, 0, None, 0, None)):
        assert D(eng.ctx, C.byref(bad), 0, c.n, None, None, None, ip) == E
    F = eng.lib.faqcs_first_error_device
    assert F(eng.ctx, None, 5, ip) == E and F(eng.ctx, d.off.data_ptr(), 1, None) == E
    eng.sync()
    assert (info.cpu().numpy() == CANARY32).all(), "a refused call wrote info"
    # count == 0 without arrays is fine, and the context is as good as new
    empty = capi.Batch(None, None, None, 7, 0, None, 0, None)
    eng.detect_device(empty, 7, 0, ip)
    eng.sync()
    assert dc.info_dict(read_info(info, 6, capi.DetectInfo)) == dict(quality_offset=0, read=7, pos=0, byte=0, next_seq=0, reserved=0)
    assert detect_dev(eng, d) == c.host(eng.lib)
    ec = dc.error_cases()[0]
    assert first_error_dev(eng, dev, ec) == ec.expect


@pytest.mark.parametrize("args", [[], ["--avg_q", "25"]], ids=["default", "avg_q25"])
def test_a_context_whose_offset_is_set_equals_one_created_with_it(args, fixture_cache):
    """The adv64 fixture (Phred+64) on a context created with 33 and set to 64: per-read results and the counter block equal those of a
    context created with 64 -- with --avg_q 25, the option the table derived from the offset serves, and with default options.  Set back to
    33, the same context gives on the adv fixture (Phred+33) what a context created with 33 gives."""
    import golden_util
    import make_fixtures

    from faqcs_amd.engine import HipEngine, _check

    opt = parse_args(["-1", "a", "-2", "b", "-d", "y"] + args)
    batches = {}
    for fx in ("adv64", "adv"):
        p1, p2 = golden_util.fixture_paths(fx, fixture_cache)
        batches[fx] = driver.pack_segments([make_fixtures.read_fastq(p1), make_fixtures.read_fastq(p2)])

    def run(e, fx):
        seq, qual, offset, seg = batches[fx]
        r = e.process(seq, qual, offset, seg, driver.terminal_n_flags(seq, offset))
        return r, e.counters()

    made64, made33, moved = HipEngine(opt, 1024, 64, device=0), HipEngine(opt, 1024, 33, device=0), HipEngine(opt, 1024, 33, device=0)
    moved.set_input_quality_offset(64)
    want_r, want_c = run(made64, "adv64")
    got_r, got_c = run(moved, "adv64")
    assert (got_r == want_r).all() and (got_c == want_c).all()
    assert int((want_r["flags"] & capi.F_VALID).sum()) > 0
    if args:  # the option bites: some reads fall to the average-quality filter
        assert int((((want_r["flags"] & capi.F_FILTER_MASK) >> capi.F_FILTER_SHIFT) == 4).sum()) > 0
    _check(moved.lib, moved.lib.faqcs_reset_counters(moved.ctx))
    moved.set_input_quality_offset(33)
    want_r, want_c = run(made33, "adv")
    got_r, got_c = run(moved, "adv")
    assert (got_r == want_r).all() and (got_c == want_c).all()
    for e in (made64, made33, moved):
        e.close()


# ---- the paired chunk loop of INTEGRATION.md section 3.2, with its detect / set / first-error steps ---------------------------------------

def _sync_rc(hip):
    return hip.lib.faqcs_sync(hip.ctx)


def _seam_run(case, fixture_cache, tmp_path):
    """One chunk per mate (the whole file) through: parse both mates, faqcs_detect_device on each, compare, set offset and quality, id
    check, submit, faqcs_first_error_device on each result array, pair, render the four files.  Only infos come back before the render.
    -> dict of what the reference's driver would have decided, and the rendered files."""
    import golden_util
    import make_fixtures
    import torch

    import render_cases as rc
    from faqcs_amd.device import DeviceMate, first_buffer_decisions
    from faqcs_amd.engine import HipEngine, _check
    from tools.parse_bench import parse_buffers
    from tools.parse_bench import read_info as parse_info

    p1, p2 = golden_util.fixture_paths(case["fixture"], fixture_cache)
    m = {"{1}": p1, "{2}": p2, "{D}": str(tmp_path)}
    opt = parse_args([m.get(a, a) for a in case["args"]])
    assert opt.input_quality_offset == AUTO_DETECT_QUALITY_OFFSET
    texts = [rc.fastq_text(make_fixtures.read_fastq(p)) for p in (p1, p2)]
    dev = torch.device("cuda:0")
    out = {"stderr": [], "quality": opt.quality}
    hip = HipEngine(opt, 1024, PLACEHOLDER, device=0)
    # 1. parse both mates
    stores, parsed = [], []
    for t in texts:
        store = torch.full((64 + len(t) + 64,), 10, dtype=torch.uint8, device=dev)
        store[64:64 + len(t)] = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).to(dev)
        pout, tens = parse_buffers(dev, len(t), t.count(b"\n") // 4)
        torch.cuda.synchronize()
        hip.parse_device(store.data_ptr() + 64, len(t), True, pout)
        stores.append(store)
        parsed.append(tens)
    hip.sync()
    pinfo = [parse_info(t["info"]) for t in parsed]
    assert all((i["error"], i["overflow"]) == (0, 0) for i in pinfo)
    n = min(i["n_reads"] for i in pinfo)
    seg = np.array(sorted(set(list(range(0, n, capi.SEGMENT_READS)) + [n])), dtype=np.uint32)
    batches = [capi.Batch(t["seq"].data_ptr() + 64, t["qual"].data_ptr() + 64, t["offset"].data_ptr(), n, len(seg) - 1, seg.ctypes.data, i["max_read_len"],
                          t["terminal_n"].data_ptr()) for t, i in zip(parsed, pinfo)]
    # 2. detect on each mate: the reference's buffer is the first 32 768 reads (first_buffer_decisions: faqcs_detect_device per mate, 2 x 24 bytes back)
    mates = [DeviceMate(stores[s][64:], parsed[s]["def_pos"][:n], parsed[s]["def_len"][:n], parsed[s]["seq"][64:], parsed[s]["qual"][64:], parsed[s]["offset"][:n + 1],
                        terminal_n=parsed[s]["terminal_n"][:n]) for s in range(2)]
    det = list(first_buffer_decisions(hip, mates[0], mates[1]))
    count = min(n, capi.SEGMENT_READS)
    out["detect"], out["detect_count"] = det, count
    # the same call through the C ABI as it stands, on a range given explicitly: the same bytes
    dinfo = torch.zeros(6, dtype=torch.int32, device=dev)
    hip.detect_device(batches[1], 0, count, dinfo.data_ptr(), stores[1].data_ptr() + 64, parsed[1]["def_pos"].data_ptr(), parsed[1]["def_len"].data_ptr())
    hip.sync()
    assert dc.info_dict(capi.DetectInfo.from_buffer_copy(dinfo.cpu().numpy().tobytes())) == det[1]
    # 3. compare the two verdicts; 4. set offset and quality
    if det[0]["quality_offset"] == 0 or det[1]["quality_offset"] == 0:
        raise driver.FatalError("trim.cpp:auto_detect_quality_offset: Unknown quality format!")
    if det[0]["quality_offset"] != det[1]["quality_offset"]:
        out["stderr"].append("Inconsistent quality offset detection between reads one and two")
        raise driver.FatalError("FaQCs.cpp:process_paired: I/O Error")
    hip.set_input_quality_offset(det[0]["quality_offset"])
    if det[0]["next_seq"] and out["quality"] < DEFAULT_NEXTSEQ_QUALITY_SCORE:
        out["stderr"].append("The input looks like NextSeq data and the quality level (-q) is adjusted to %d for trimming." % DEFAULT_NEXTSEQ_QUALITY_SCORE)
        out["quality"] = DEFAULT_NEXTSEQ_QUALITY_SCORE
        hip.set_quality(out["quality"])
    if n > capi.SEGMENT_READS and n % capi.SEGMENT_READS:  # the reference looks again at the last partial buffer (driver.py: Q16)
        last = n - n % capi.SEGMENT_READS
        out["detect_last"] = first_buffer_decisions(hip, mates[0], first=last, count=n - last)
        assert not (out["detect_last"]["next_seq"] and out["quality"] < DEFAULT_NEXTSEQ_QUALITY_SCORE), "the test's fixtures do not bump -q in the middle of a chunk"
    # 5. the id check, before trim()
    pair_info = torch.zeros(5, dtype=torch.int64, device=dev)
    hip.pair_device(mates[0].capi(), mates[1].capi(), None, pair_info.data_ptr())
    hip.sync()
    pr = capi.PairInfo.from_buffer_copy(pair_info.cpu().numpy().tobytes())
    assert (pr.mismatch, pr.n_pairs) == (0, n)
    # 6. submit, mate 1 first; 7. where trim() threw
    results = [torch.zeros((max(n, 1), 4), dtype=torch.int16, device=dev) for _ in range(2)]
    einfo = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    for s in range(2):
        _check(hip.lib, hip.lib.faqcs_submit_device(hip.ctx, C.byref(batches[s]), results[s].data_ptr()))
        hip.first_error_device(results[s].data_ptr(), n, einfo[s].data_ptr())
    out["sync_rc"] = _sync_rc(hip)  # (a submission with a bad read fails here, and says no more than that)
    err = [capi.ErrorInfo.from_buffer_copy(einfo[s].cpu().numpy().tobytes()) for s in range(2)]  # 2 x 8 bytes
    out["first_error"] = [(int(e.n_good), int(e.flags)) for e in err]
    # the reference stops before the buffer that holds the bad read: trim(buffer1), trim(buffer2) of buffer k come before anything of it is written
    n_good = min(e.n_good for e in err)
    n_write = n if n_good == n else n_good // capi.SEGMENT_READS * capi.SEGMENT_READS
    out["n_write"] = n_write
    # 8. pair; 9. render the files
    for s in range(2):
        mates[s].results = results[s][:n]
    route = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    cm = [mates[0].capi(), mates[1].capi()]
    hip.pair_device(cm[0], cm[1], route.data_ptr(), pair_info.data_ptr())
    cap = len(texts[0]) + len(texts[1]) + 10 * n
    files = {}
    for f in range(4):
        o_text = torch.empty(cap + 64 + 16, dtype=torch.uint8, device=dev)
        shift = (-o_text.data_ptr()) % 16
        rinfo = torch.zeros(2, dtype=torch.int64, device=dev)
        hip.render_pair_device(f, cm[0], cm[1], route.data_ptr(), n_write, capi.RenderOut(o_text.data_ptr() + shift, cap, None, None, rinfo.data_ptr()))
        files[f] = (o_text, shift, rinfo)
    assert _sync_rc(hip) == out["sync_rc"]
    out["files"] = {}
    for f, (o_text, shift, rinfo) in files.items():
        h = rinfo.cpu().numpy()
        assert int(h[1]) >> 32 == 0
        out["files"][capi.PAIR_FILES[f]] = (o_text[shift:shift + int(h[0])].cpu().numpy().tobytes(), int(h[1]) & 0xFFFFFFFF)
    hip.close()
    return out


def _check_files(case, out):
    for fn, meta in case["fastq"].items():
        text, records = out["files"][fn]
        assert (records, len(text)) == (meta["records"], meta["bytes"]), fn
        assert hashlib.md5(text).hexdigest() == meta["md5"], fn


GOLDEN_LOOP = ["adv64_autodetect", "nextseq_default", "nextseq_phix", "err_quality_above_41", "err_unknown_base_adapter", "advbig_default"]


@pytest.mark.parametrize("name", GOLDEN_LOOP)
def test_the_paired_loop_with_its_decisions_on_the_device(name, fixture_cache, tmp_path):
    """The golden fixtures through the paired loop of INTEGRATION.md section 3.2 on ONE context created with a placeholder offset: the
    verdicts, the bump and the bad read are what the reference's process shows (its stderr, its files), and the rendered files have the md5s of
    the golden case."""
    import golden_util

    case = golden_util.load_case(name)
    out = _seam_run(case, fixture_cache, tmp_path)
    d1, d2 = out["detect"]
    n_all = out["first_error"]
    if name == "adv64_autodetect":
        assert (d1["quality_offset"], d2["quality_offset"]) == (64, 64) and out["sync_rc"] == 0
    elif name.startswith("nextseq"):
        assert d1["next_seq"] == 1 and (d1["quality_offset"], d2["quality_offset"]) == (33, 33)
        assert out["quality"] == 20 and out["stderr"] == [case["stderr"][1]]
    elif name == "err_quality_above_41":
        assert n_all[0] == (57, capi.F_ERR_QUALITY) and n_all[1][1] == 0 and n_all[1][0] == 200
        assert out["sync_rc"] == capi.E_QUALITY and out["n_write"] == 0
    elif name == "err_unknown_base_adapter":
        assert n_all[1] == (91, capi.F_ERR_BASE) and n_all[0] == (200, 0)
        assert out["sync_rc"] == capi.E_BASE and out["n_write"] == 0
    elif name == "advbig_default":
        assert out["detect_count"] == capi.SEGMENT_READS and (d1["quality_offset"], d2["quality_offset"]) == (33, 33)
        assert d1["read"] < capi.SEGMENT_READS and d2["read"] < capi.SEGMENT_READS and out["detect_last"]["next_seq"] == 0
    if not name.startswith("nextseq"):
        assert out["stderr"] == [] and d1["next_seq"] == 0
    if not name.startswith("err"):
        assert out["sync_rc"] == 0 and all(f == 0 for _, f in n_all) and out["n_write"] == n_all[0][0]
    _check_files(case, out)
