"""faqcs_gunzip_stream_device on the MI355X: chunked feeds of gunzip_stream_cases.py against the host statement faqcs_gunzip_stream_host,
call by call -- the text byte for byte, info and the carried state field for field, the valid window byte for byte --, two files fed
alternately on one context, and the chain gunzip_stream -> parse with the tail carried in device memory against the parse of the whole text.  Every feed has
been through the host statement, and the same text through the sanitizers, in tests/test_gunzip_stream_model.py."""
import gzip
import os

import numpy as np
import pytest

import gunzip_cases as gc
import gunzip_stream_cases as gs
from faqcs_amd import _capi as capi
from faqcs_amd.options import parse_args

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example_1.fastq.gz")
MAX_CUTS = 16


@pytest.fixture(scope="module")
def eng():
    from faqcs_amd.engine import HipEngine

    e = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    yield e
    e.close()


def device_window(skew=0):
    """-> (tensor, address, read()): a window in device memory, `skew` bytes behind a 256-byte aligned address, filled as host_window()'s"""
    import torch

    t = torch.full((gs.WIN + 256,), 0xEE, dtype=torch.uint8, device="cuda:0")
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + skew, lambda: t[skew:skew + gs.WIN].cpu().numpy()


def device_call(eng, shift=1):
    """-> call(...) of gunzip_stream_cases.host_call over faqcs_gunzip_stream_device: canary-filled device buffers, the compressed bytes
    `shift` bytes behind a 256-byte aligned address"""
    import torch

    dev = torch.device("cuda:0")

    def call(chunk, final, st, window, piece, max_rounds, capacity):
        d_comp = torch.zeros(shift + len(chunk) + 1, dtype=torch.uint8, device=dev)
        if chunk:
            d_comp[shift:shift + len(chunk)] = torch.from_numpy(np.frombuffer(chunk, np.uint8).copy()).to(dev)
        text = torch.full((gc.FRONT + capacity + 64,), gc.CANARY, dtype=torch.uint8, device=dev)
        info = torch.full((5,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        assert (text.data_ptr() + gc.FRONT) % 16 == 0 and d_comp.data_ptr() % 256 == 0
        out = capi.GunzipOut(text.data_ptr() + gc.FRONT, capacity, info.data_ptr())
        eng.gunzip_stream_device(d_comp.data_ptr() + shift if chunk else None, len(chunk), final, st, out, piece, max_rounds)   # (the call blocks)
        p = capi.GunzipInfo.from_buffer_copy(info.cpu().numpy().tobytes())
        return 0, gc.info_dict(p), text.cpu().numpy()
    return call


def both(eng, comp, ends, piece, max_rounds, what, shift=1, skew=0):
    """one feed on the host and on the device -> the device's calls, equal to the host's call by call"""
    h = gs.feed(gs.host_call(eng.lib), comp, ends, piece, max_rounds)
    d = gs.feed(device_call(eng, shift), comp, ends, piece, max_rounds, window=device_window(skew))
    assert len(h) == len(d), what
    for k, (a, b) in enumerate(zip(h, d)):
        w = "%s, call %d" % (what, k)
        assert b.info == a.info, "%s: device %s host %s" % (w, b.info, a.info)
        assert b.state == a.state, "%s: device %s host %s" % (w, b.state, a.state)
        assert b.text == a.text, "%s: the text differs" % w
        assert b.window == a.window, "%s: the window differs" % w
    return d


@pytest.mark.parametrize("piece", gc.PIECES)
def test_the_feeds_equal_the_host_statement(eng, piece):
    """the targeted feeds at this piece size, at most MAX_CUTS cuts each, and every case of gunzip_cases.py in three chunks; at 1 024,
    where every feed runs, the table of edges is reached on the device too"""
    rng = np.random.Generator(np.random.PCG64([353, gc.SEED, piece]))
    seen = set()
    for k, f in enumerate(gs.feeds()):
        if piece not in f.pieces:
            continue
        ends = f.ends if len(f.ends) <= MAX_CUTS else f.ends[::len(f.ends) // MAX_CUTS + 1]
        what = "%s at %d" % (f.name, piece)
        calls = both(eng, f.comp, ends, piece, f.max_rounds, what, shift=k % 7, skew=k % 5)
        seen |= gs.check_calls(f.comp, calls, what, serial="E_SERIAL, continued" in f.edges) | f.edges
        gs.expect(f, calls, what)
        gs.check_stops(f, calls, what)
    for k, c in enumerate(gc.cases()):
        if piece not in c.pieces or c.code == gc.E_SERIAL or len(c.comp) < 3:
            continue
        ends = sorted(int(v) for v in rng.integers(1, len(c.comp), 2))
        both(eng, c.comp, ends, piece, c.max_rounds, "%s at %d in three chunks" % (c.name, piece), shift=k % 7)
    if piece == 1024:
        seen |= gs.overflow_continued(device_call(eng), device_window()) | gs.isize_modulo(device_call(eng), device_window())
        assert not gs.unreached(seen), "edges the device did not reach"


def test_every_alignment_of_the_compressed_bytes_and_the_window(eng):
    """d_comp at every residue mod 16 for a continued member, the window at the same residue: the window kernels' 16-byte groups start
    anywhere"""
    f = next(f for f in gs.feeds() if f.name == "a short window, then a full one shifted")
    for shift in range(16):
        calls = both(eng, f.comp, f.ends, 1024, f.max_rounds, "shift %d" % shift, shift=shift, skew=shift)
        gs.check_calls(f.comp, calls, "shift %d" % shift)


def test_two_streams_on_one_context(eng):
    """two files fed alternately: neither state disturbs the other"""
    from faqcs_amd.device import GunzipStream
    import torch

    t300, t200, _ = gc.texts()
    files = [gc.gz_member(t300, 1) + gc.gz_member(t200[:50000], 9), gc.gz_member(t200, 6)]
    streams = [GunzipStream(eng, piece_bytes=4096), GunzipStream(eng)]
    at, got, step = [0, 0], [b"", b""], [41000, 17000]
    end = [0, 0]
    while any(a < len(f) for a, f in zip(at, files)):
        for k in (0, 1):
            if at[k] >= len(files[k]):
                continue
            end[k] = min(len(files[k]), max(end[k], at[k]) + step[k])
            d = torch.from_numpy(np.frombuffer(files[k][at[k]:end[k]], np.uint8).copy()).to("cuda:0")
            text, info = streams[k].feed(d, end[k] == len(files[k]))
            got[k] += bytes(text.cpu().numpy())
            at[k] += info.consumed
            st = streams[k].state
            assert st.total_comp == at[k] and st.total_bytes == len(got[k])
    assert got[0] == t300 + t200[:50000] and got[1] == t200
    assert (streams[0].state.members, streams[1].state.members) == (2, 1) and all(s.state.phase == gs.BETWEEN for s in streams)


def test_overflow_writes_nothing_but_info(eng):
    assert gs.overflow_continued(device_call(eng, shift=3), device_window(5)) == {"overflow, continued"}


def test_gunzip_stream_feeds_the_parse(eng):
    """the golden gzip file in three chunks cut at arbitrary bytes: faqcs_gunzip_stream_device -> faqcs_parse_device with final = 0 and the
    unparsed tail carried in device memory in front of the next call's text; the reads equal the parse of the whole text in every array"""
    import torch

    from faqcs_amd.device import GunzipStream
    from tools.parse_bench import parse_buffers, read_info

    with open(GOLDEN, "rb") as f:
        golden = f.read()
    text = gzip.decompress(golden)
    dev = torch.device("cuda:0")
    n_reads = text.count(b"\n") // 4

    def parse(d_text, n, final):
        pout, t = parse_buffers(dev, max(n, 64), n_reads + 8)
        torch.cuda.synchronize()
        eng.parse_device(d_text.data_ptr(), n, final, pout)
        eng.sync()
        info = read_info(t["info"])
        assert info["error"] == 0 and info["overflow"] == 0
        nb, k = info["n_bytes"], info["n_reads"]
        off = t["offset"][:k + 1].cpu().numpy().astype(np.int64)
        return info, [t["seq"][64:64 + nb].cpu().numpy(), t["qual"][64:64 + nb].cpu().numpy(), np.diff(off), t["terminal_n"][:k].cpu().numpy(),
                      t["def_pos"][:k].cpu().numpy().astype(np.int64), t["def_len"][:k].cpu().numpy()]

    def padded(b):
        store = torch.full((64 + len(b) + 64,), 10, dtype=torch.uint8, device=dev)
        if b:
            store[64:64 + len(b)] = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dev)
        return store[64:64 + len(b)]

    want_info, want = parse(padded(text), len(text), True)
    assert want_info["n_reads"] == n_reads
    # the loop of INTEGRATION.md section 3.2: ONE text arena in device memory; the tail a parse leaves is copied, device to device, to where
    # its end is 16-byte aligned, the next call's text goes behind it (out->text = d_text + have), and the parse reads tail and text as one
    for comp, piece, ends in ((golden, 1024, (len(golden) // 3 + 1, 2 * len(golden) // 3 + 5)), (gzip.compress(text, 6), 0, (4097, len(golden) // 2))):
        d_comp = torch.from_numpy(np.frombuffer(comp, np.uint8).copy()).to(dev)
        arena = torch.full((64 + 16 + len(text) + 64 + capi.ARENA_PAD_AFTER,), 10, dtype=torch.uint8, device=dev)
        base = 64 + (-(arena.data_ptr() + 64)) % 16        # 16-byte aligned, 64 bytes and more in front
        window = torch.zeros(gs.WIN, dtype=torch.uint8, device=dev)
        st = gs.new_state(window.data_ptr())
        d_info = torch.zeros(5, dtype=torch.int64, device=dev)
        at, have, begin, done, parts = 0, 0, base, 0, []
        for end in list(ends) + [len(comp)]:
            final = end == len(comp)
            room = len(text) - done - have
            out = capi.GunzipOut(arena.data_ptr() + begin + have, room, d_info.data_ptr())
            assert (arena.data_ptr() + begin + have) % 16 == 0
            torch.cuda.synchronize()
            eng.gunzip_stream_device(d_comp.data_ptr() + at, end - at, final, st, out, piece, 0)
            gi = capi.GunzipInfo.from_buffer_copy(d_info.cpu().numpy().tobytes())
            assert (gi.error, gi.overflow) == (0, 0)
            at += gi.consumed
            n = have + gi.n_bytes
            pinfo, got = parse(arena[begin:begin + n], n, final)
            got[4] = got[4] + done   # def_pos: of the whole text
            parts.append(got)
            done += pinfo["consumed"]
            have = n - pinfo["consumed"]
            tail = arena[begin + pinfo["consumed"]:begin + n].clone()
            begin = base + (-have) % 16
            arena[begin:begin + have] = tail                 # the carried tail, device to device
        assert at == len(comp) and have == 0 and done == len(text) and st.members == 1 and st.total_bytes == len(text)
        for k in range(6):
            assert (np.concatenate([p[k] for p in parts]) == want[k]).all(), k
    # GunzipStream is the same call with the state and the window kept for the caller
    gzs = GunzipStream(eng)
    d_text, info = gzs.feed(torch.from_numpy(np.frombuffer(golden, np.uint8).copy()).to(dev), True)
    assert bytes(d_text.cpu().numpy()) == text and info.error == 0 and gzs.state.members == 1
    # a bad member is info.error, not an exception: what stands in front of it is still handed over
    bad = bytearray(golden)
    bad[-6] ^= 1
    gzs = GunzipStream(eng)
    d_text, info = gzs.feed(torch.from_numpy(np.frombuffer(bytes(bad), np.uint8).copy()).to(dev), True)
    assert (info.error, info.n_bytes, info.consumed, info.n_members) == (capi.INFLATE_E_CRC, 0, 0, 0) and int(d_text.numel()) == 0
    assert (gzs.state.total_comp, gzs.state.total_bytes, gzs.state.members) == (0, 0, 0)
