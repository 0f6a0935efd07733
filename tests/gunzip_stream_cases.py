"""Chunked feeds for the streamed gunzip (faqcs_gunzip_stream_host / faqcs_gunzip_stream_device, include/faqcs_mi.h): the files of
gunzip_cases.py and a few hand-written ones, cut at chosen bytes, a feeder that presents comp[at : end_k] call after call, and what every call
must leave behind.  EDGES is the coverage table: an edge is reached when the feeder sees it in the state a call returns, or when a feed is
built for it AND the calls stopped where the feed says (check_stops: consumed, bit and the carried bytes at the intended block boundary)
or its last call states the error it is built for (expect); a test fails when one is unreached.

The yardstick is zlib: zlib_model() of gunzip_cases.py and an incremental decompressobj for the text, zlib.crc32 and slicing for the carried
state.  It is never the code under test."""
import ctypes as C
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

import deflate_streams as ds
import gunzip_cases as gc
from faqcs_amd import _capi as capi

WIN = capi.GUNZIP_WINDOW
BETWEEN, STREAM, TRAILER = capi.GUNZIP_BETWEEN, capi.GUNZIP_STREAM, capi.GUNZIP_TRAILER
STATE_FIELDS = tuple(f for f, _ in capi.GunzipState._fields_ if f != "window")

EDGES = {
    "cut in the fixed header": "inside the 10 fixed header bytes", "cut in FEXTRA": "inside FEXTRA", "cut in FNAME": "inside FNAME",
    "cut at the first block": "the header is whole, no bit of the stream is there", "cut in mid-block": "bytes of a block that is not whole are left over",
    "stored block end": "a byte-aligned block end behind a stored block",
    **{"bit %d" % k: "a block end that leaves bit = %d" % k for k in range(1, 8)},
    **{"trailer byte %d" % k: "phase TRAILER with %d of the 8 trailer bytes resident" % k for k in range(8)},
    "cut between members": "exactly between two members", "cut in garbage": "inside trailing garbage",
    "empty member across a cut": "a member without text whose bytes come in two calls", "member over 3 calls": "a member over three or more calls",
    "header, no text": "a call that consumes a header and delivers no text", "no progress": "a call that consumes nothing and leaves the state as it is",
    "window below 32768": "a carried window shorter than 32 768 that the next call reads", "window of 32768": "a carried window of exactly 32 768",
    "window shifted twice": "two calls in a row that add fewer than 32 768 bytes to a full window",
    "distance 32768 to the window's first byte": "a match of distance 32 768 whose source is the carried window's first byte",
    "markers of markers across a call": "a marker copied by a match, copied on by a later piece, its source in the carried window",
    "source straddles the call": "dist < len, the source straddles the call boundary",
    "distance in front of the member, two calls on": "a distance in front of the member's first byte when that byte came two calls earlier: E_DATA",
    "wrong crc, two calls on": "a wrong CRC in a member opened two calls earlier", "wrong isize, two calls on": "a wrong ISIZE in a member opened two calls earlier",
    "truncated stream, continued": "final = 1 in the stream of a continued member", "truncated trailer, continued": "final = 1 in the trailer of a continued member",
    "damage, continued": "a damaged stream in a continued member", "E_SERIAL, continued": "max_rounds = 1 on a continued level-0 member",
    "overflow, continued": "overflow on a continued call: the state untouched, success on a shorter prefix",
    "member_bytes + 2^32": "member_bytes raised by 2^32 between two calls: ISIZE is modulo",
}

# one call of a feed: the chunk was comp[at : end]; info; the text it delivered; the state behind it {field: value}; the valid window
Call = namedtuple("Call", "at end final info text state window")
# name; the file; the chunk ends (the last call takes the rest with final = 1); piece sizes; max_rounds; edges it is built for; where it is
# built to stop: ((call index, {state field: value, or (lowest, highest)}), ..), what check_stops() asserts of the state behind that call
Feed = namedtuple("Feed", "name comp ends pieces max_rounds edges stops")


def new_state(window_address):
    st = capi.GunzipState()
    st.window = window_address
    return st


def state_dict(st):
    return {f: int(getattr(st, f)) for f in STATE_FIELDS}


def host_call(lib):
    """-> call(chunk, final, state, window array, piece_bytes, max_rounds, capacity) -> (rc, info dict, the WHOLE canary-filled text buffer)
    over faqcs_gunzip_stream_host"""
    def call(chunk, final, st, window, piece, max_rounds, capacity):
        cb = np.frombuffer(chunk, np.uint8).copy() if chunk else np.zeros(1, np.uint8)
        text = gc.ic.pc.aligned_bytes(gc.FRONT + capacity + 64)
        info = capi.GunzipInfo()
        C.memset(C.byref(info), 0xFF, C.sizeof(info))
        out = capi.GunzipOut(text.ctypes.data + gc.FRONT, capacity, C.addressof(info))
        rc = lib.faqcs_gunzip_stream_host(cb.ctypes.data if chunk else None, len(chunk), 1 if final else 0, piece, max_rounds, C.byref(st), C.byref(out))
        return rc, gc.info_dict(info), text
    return call


def host_window():
    """-> (array, address, read()): a window in host memory, filled with a pattern no text holds in a row"""
    w = np.full(WIN, 0xEE, np.uint8)
    return w, w.ctypes.data, lambda: w.copy()


def feed(call, comp, ends, piece, max_rounds, window=None, capacity=None, state=None):
    """Presents comp[at : end_k] for every chunk end, then the rest with final = 1; a call without progress is followed by the next, larger
    chunk.  Stops behind the first call that states an error.  -> [Call]; every call's buffer is checked for writes outside
    text[0 .. n_bytes)."""
    comp = bytes(comp)
    warr, waddr, wread = window or host_window()
    st = state or new_state(waddr)
    # (exactly zlib's text; where zlib refuses a member, room for what the walk counts of it before a pass finds the fault)
    cap = capacity if capacity is not None else model(comp).n_text + (400000 if model(comp).error else 0)
    at, calls = 0, []
    for end in [e for e in ends if e < len(comp)] + [len(comp)]:
        final = end == len(comp)
        rc, info, text = call(comp[at:end], final, st, warr, piece, max_rounds, cap)
        assert rc == 0, (rc, at, end)
        assert info["overflow"] == 0, info
        nb = info["n_bytes"]
        assert (text[:gc.FRONT] == gc.CANARY).all() and (text[gc.FRONT + cap:] == gc.CANARY).all(), "bytes outside the text buffer were written"
        sd = state_dict(st)
        calls.append(Call(at, end, final, info, bytes(text[gc.FRONT:gc.FRONT + nb]), sd, bytes(wread()[WIN - sd["window_bytes"]:])))
        at += info["consumed"]
        if info["error"]:
            break
    return calls


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
Model = namedtuple("Model", "texts error consumed partial n_text")


@functools.lru_cache(maxsize=None)
def model(comp):
    """zlib on the whole file: the members it takes whole, whether it stops with an error and where (zlib_model), and what it delivers of
    the member it refuses before it does (fed 64 bytes at a time)"""
    texts, error, consumed = gc.zlib_model(comp)
    partial = b""
    if error:
        d = zlib.decompressobj(31)
        try:
            for i in range(consumed, len(comp), 64):
                partial += d.decompress(comp[i:i + 64])
        except zlib.error:
            pass
    return Model(tuple(texts), error, consumed, partial, sum(len(t) for t in texts) + len(partial))


def check_calls(comp, calls, what, code=None, serial=False):
    """What every call must leave behind, against zlib: the text so far, state.crc, the valid window, the counters, consumed + carried adding
    up to the file; behind the last call the members, the error exactly when zlib has one (code: which), consumed as zlib's.
    serial: the feed ends with E_SERIAL, no property of the data.  -> the edges the calls were seen to reach"""
    comp = bytes(comp)
    md = model(comp)
    whole = b"".join(md.texts)
    seen, got, prev, run, shifts = set(), b"", dict.fromkeys(STATE_FIELDS, 0), 0, 0
    for k, c in enumerate(calls):
        w = "%s, call %d [%d : %d)" % (what, k, c.at, c.end)
        s, info = c.state, c.info
        got += c.text
        assert info["n_bytes"] == len(c.text) and s["total_bytes"] == len(got), w
        assert s["total_comp"] == c.at + info["consumed"] and c.at + info["consumed"] <= c.end, w
        assert s["members"] == prev["members"] + info["n_members"] and s["reserved"] == 0, w
        # the text so far: zlib's, as far as zlib delivers one (behind an error of zlib's, what it handed on before)
        ref = whole + md.partial
        assert got[:len(ref)] == ref[:len(got)], "%s: the text differs from zlib's" % w
        if not md.error:
            assert len(got) <= len(whole), w
        done = sum(len(t) for t in md.texts[:s["members"]]) if s["members"] <= len(md.texts) else None
        assert done is not None and done + s["member_bytes"] == len(got), "%s: %s" % (w, s)
        open_text = got[done:]
        assert s["crc"] == (zlib.crc32(open_text) & 0xFFFFFFFF if s["phase"] != BETWEEN else 0), "%s: crc %s" % (w, s)
        assert s["window_bytes"] == min(len(open_text), WIN) and c.window == open_text[len(open_text) - s["window_bytes"]:], "%s: window" % w
        assert s["phase"] in (BETWEEN, STREAM, TRAILER) and (s["bit"] == 0 or s["phase"] == STREAM) and s["bit"] < 8, w
        assert s["phase"] != BETWEEN or s["member_bytes"] == 0, w
        if info["error"]:
            assert k == len(calls) - 1, w
            continue
        left = c.end - (c.at + info["consumed"])
        n_in = c.end - c.at
        if not c.final:
            if info["consumed"] == 0 and info["n_bytes"] == 0:
                assert s == prev, "%s: no progress, and the state changed" % w
                if n_in:
                    seen.add("no progress")
            if s["phase"] == BETWEEN and 0 < left < 10 and comp[c.end - left] == 31:
                seen.add("cut in the fixed header")
            if s["phase"] == BETWEEN and left == 0 and s["members"] and comp[c.end:c.end + 2] == b"\x1f\x8b":
                seen.add("cut between members")
            if s["phase"] == STREAM:
                if s["member_bytes"] == 0 and left == 0 and s["bit"] == 0:
                    seen.add("cut at the first block")
                if info["n_bytes"] == 0 and info["consumed"] and prev["phase"] == BETWEEN:
                    seen.add("header, no text")
                if left > 1:
                    seen.add("cut in mid-block")
                if s["member_bytes"] and s["bit"]:
                    seen.add("bit %d" % s["bit"])
            if s["phase"] == TRAILER:
                assert left < 8, w
                seen.add("trailer byte %d" % left)
        # the carried window this call read
        if prev["phase"] == STREAM and info["n_bytes"]:
            seen.add("window of 32768" if prev["window_bytes"] == WIN else "window below 32768")
            shifts = shifts + 1 if prev["window_bytes"] == WIN and s["members"] == prev["members"] and s["member_bytes"] - prev["member_bytes"] < WIN else 0
            if shifts >= 2:
                seen.add("window shifted twice")
        # run: the calls so far that delivered text of the member that was open at entry, or opened first in this call
        run = (run if prev["phase"] == STREAM else 0) + (1 if info["n_bytes"] else 0)
        if run >= 3:
            seen.add("member over 3 calls")
        if s["members"] != prev["members"]:
            run = 1 if s["member_bytes"] else 0
        prev = s
    last = calls[-1]
    if serial:
        assert last.info["error"] == gc.E_SERIAL, what
        return seen
    assert last.final or last.info["error"], what
    assert bool(last.info["error"]) == md.error, "%s: error %d, zlib %s" % (what, last.info["error"], "refuses" if md.error else "accepts")
    if md.error:
        assert last.state["members"] == len(md.texts), what
        assert code is None or last.info["error"] == code, "%s: %s" % (what, last.info)
        assert last.state["total_comp"] >= md.consumed if last.state["phase"] != BETWEEN else last.state["total_comp"] == md.consumed, what
    else:
        assert got == whole and last.state["members"] == len(md.texts) and last.state["total_comp"] == md.consumed and last.state["phase"] == BETWEEN, what
    return seen


# ---- hand-written members ---------------------------------------------------------------------------------------------------------------
def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _member_of(s):
    return gc.gz_member(ds.expand(s.items), raw=s.getvalue())


def _boundary(s, k, head=10):
    """a chunk end that makes a call stop at block k's start of Stream s behind a header of `head` bytes: the byte of that bit is resident,
    the block is not"""
    return head + gc.block_starts(s)[0][k] // 8 + 1


def stored_blocks(member, head=10):
    """a member of stored blocks only (zlib level 0) -> [(file byte where the block's header stands, its LEN)]"""
    p, out = head, []
    while True:
        n = struct.unpack_from("<H", member, p + 1)[0]
        assert member[p] in (0, 1) and struct.unpack_from("<H", member, p + 3)[0] == n ^ 0xFFFF
        out.append((p, n))
        p += 5 + n
        if member[out[-1][0]] == 1:
            return out


@functools.lru_cache(maxsize=None)
def handmade():
    """{name: (member, the Stream)}"""
    rng = np.random.Generator(np.random.PCG64([331, gc.SEED]))
    out = {}
    s = ds.Stream()  # 60 small dynamic blocks, each with up to 7 matches of 13 bits behind its literals of 8: block ends at every bit of a byte
    for _ in range(60):
        s.dynamic(gc._lit(rng, int(rng.integers(20, 90))) + [(8, 1)] * int(rng.integers(0, 8)), ds.PLAIN_LIT, ds.PLAIN_DIST)
    s.fixed(gc._lit(rng, 10), final=True)
    assert {b % 8 for b in gc.block_starts(s)[0][1:]} == set(range(8))
    out["small blocks"] = s
    s = ds.Stream()  # gunzip_cases' marker stream with the call boundary where the piece boundary was
    s.stored(_bytes(rng, 33000))
    n_b = 2 + 50 + 10 + 20 + 4600
    s.dynamic([65, 66, (50, 5), (10, 32768), (20, 15)] + gc._lit(rng, 4600), ds.PLAIN_LIT, ds.PLAIN_DIST)
    s.dynamic([(30, n_b - 62)] + gc._lit(rng, 4600), ds.PLAIN_LIT, ds.PLAIN_DIST, final=True)
    out["markers"] = s
    s = ds.Stream()  # a window of exactly 32 768 and a first symbol that copies its first byte
    s.stored(_bytes(rng, WIN))
    s.dynamic([(10, WIN)] + gc._lit(rng, 300), ds.PLAIN_LIT, ds.PLAIN_DIST, final=True)
    out["first byte of the window"] = s
    s = ds.Stream()  # a short window, read at its first byte; then three calls that add little to a full one
    s.stored(_bytes(rng, 1000))
    s.dynamic([(20, 1000)] + gc._lit(rng, 200), ds.PLAIN_LIT, ds.PLAIN_DIST)
    s.stored(_bytes(rng, 40000))
    for _ in range(3):
        s.dynamic([(100, 30000)] + gc._lit(rng, 500), ds.PLAIN_LIT, ds.PLAIN_DIST)
    s.fixed([1, 2, 3], final=True)
    out["windows"] = s
    s = ds.Stream()  # one byte in front of the member, when that byte came two calls earlier
    s.stored(_bytes(rng, 500))
    s.dynamic(gc._lit(rng, 300), ds.PLAIN_LIT, ds.PLAIN_DIST)
    s.dynamic([(20, 801)] + gc._lit(rng, 50), ds.PLAIN_LIT, ds.PLAIN_DIST, final=True)
    out["in front of the member"] = s
    return out


@functools.lru_cache(maxsize=None)
def feeds():
    """the targeted feeds: every one is checked by check_calls() against zlib, and those with an expectation of their own by expect()"""
    rng = np.random.Generator(np.random.PCG64([337, gc.SEED]))
    t300, t200, t120 = gc.texts()
    hm = handmade()
    out = []

    def add(name, comp, ends, *edges, pieces=gc.PIECES, max_rounds=0, stops=()):
        for e in edges:
            assert e in EDGES, e
        out.append(Feed(name, bytes(comp), tuple(int(e) for e in ends), tuple(pieces), max_rounds, frozenset(edges), tuple(stops)))
        # an edge that check_calls() cannot see for itself is credited only to a feed that states where it stops, or what its last call says
        assert all(e in AUTO for e in edges) or stops or name in EXPECT, name

    five = t300[:30000]
    m6 = gc.gz_member(t120, 6)
    # headers
    fx = gc.gz_member(five, 6, fextra=b"QQ" + struct.pack("<H", 300) + bytes(300), fname=b"reads_of_a_lane.fastq")
    assert fx[3] == 4 | 8 and 12 <= 100 < 12 + 304 and fx[12 + 304 + 5:].index(0) > 3   # the cuts lie in FEXTRA's bytes and in FNAME's
    nothing = dict(phase=BETWEEN, total_comp=0, members=0, total_bytes=0)
    add("cut in FEXTRA", fx, [100], "cut in FEXTRA", stops=[(0, nothing)])
    add("cut in FNAME", fx, [12 + 304 + 5], "cut in FNAME", stops=[(0, nothing)])
    add("cut in the fixed header", m6 + fx, [len(m6) + 4], "cut in the fixed header")
    add("cut at the first block", m6, [10, 20000], "cut at the first block", "header, no text")
    add("a chunk too small, then larger ones", m6, [10, 12, 14, 40, 20000], "no progress", "cut in mid-block")
    # block ends
    s = hm["small blocks"]
    starts = gc.block_starts(s)[0]
    small = _member_of(s)
    for r in range(1, 8):
        k = next(k for k in range(1, len(starts)) if starts[k] % 8 == r)
        add("a block end at bit %d" % r, small, [_boundary(s, k)], "bit %d" % r, pieces=(1024,))
    add("every block of the small member", small, [_boundary(s, k) for k in range(1, len(starts))], "member over 3 calls", pieces=(1024, 0))
    m0 = gc.gz_member(t200, 0)
    sb = stored_blocks(m0)
    assert len(sb) >= 4
    at_block = [(k, dict(phase=STREAM, bit=0, total_comp=sb[k + 1][0], member_bytes=sum(n for _, n in sb[:k + 1]))) for k in range(len(sb) - 1)]
    add("level 0, a cut behind every stored block", m0, [p for p, _ in sb[1:]], "stored block end", "member over 3 calls", max_rounds=4000, stops=at_block)
    # trailers and members
    for j in range(8):
        add("trailer byte %d" % j, m6 + fx, [len(m6) - 8 + j], "trailer byte %d" % j, pieces=(1024,))
    add("cut between members", m6 + fx, [len(m6)], "cut between members")
    add("cut in garbage", fx + b"\0\0\0\0 the end", [len(fx) + 3], "cut in garbage", stops=[(0, dict(phase=BETWEEN, members=1, total_comp=len(fx) + 3))])
    add("cut in garbage that begins 1f", fx + b"\x1f\x00", [len(fx) + 1], "cut in garbage", stops=[(0, dict(phase=BETWEEN, members=1, total_comp=len(fx)))])
    e = gc.gz_member(b"", 6)
    for cut in (3, 10, 11, len(e) - 8, len(e) - 3):
        add("an empty member cut at %d" % cut, fx + e + fx, [len(fx) + cut], "empty member across a cut", pieces=(1024,),
            stops=[(0, dict(members=1, member_bytes=0, total_comp=(len(fx), len(fx) + cut))), (1, dict(members=3, phase=BETWEEN))])
    add("three chunks", gc.gz_member(t300, 1), [30000, 70000], "member over 3 calls")
    # the carried window
    s = hm["markers"]
    def at_start(s, k, n_bytes, call):
        """behind call `call` the stream stands at block k's first bit, n_bytes of text delivered: what follows reads the carried window"""
        b = gc.block_starts(s)[0][k]
        return (call, dict(phase=STREAM, total_comp=10 + b // 8, bit=b % 8, member_bytes=n_bytes, window_bytes=min(n_bytes, WIN)))

    # (B's first symbols: two literals, then 50 bytes from 5 back -- three of them in front of the call --, 10 from 32 768 back, 20 that copy those)
    add("markers across a call", _member_of(s), [_boundary(s, 1)], "markers of markers across a call", "source straddles the call", "window of 32768",
        stops=[at_start(s, 1, 33000, 0)])
    s = hm["first byte of the window"]
    add("distance 32768 to the window's first byte", _member_of(s), [_boundary(s, 1)], "distance 32768 to the window's first byte", "window of 32768",
        stops=[at_start(s, 1, WIN, 0)])   # (exactly WIN bytes are carried and the next symbol reaches WIN back: the window's first byte)
    s = hm["windows"]
    add("a short window, then a full one shifted", _member_of(s), [_boundary(s, k) for k in (1, 3, 4, 5)], "window below 32768", "window shifted twice", "member over 3 calls",
        stops=[at_start(s, 1, 1000, 0), at_start(s, 3, 41220, 1), at_start(s, 4, 41820, 2), at_start(s, 5, 42420, 3)])
    s = hm["in front of the member"]
    add("a distance in front of the member, two calls on", gc.gz_member(b"no text: the stream is refused", raw=s.getvalue()), [_boundary(s, 1), _boundary(s, 2)],
        "distance in front of the member, two calls on", stops=[at_start(s, 1, 500, 0), at_start(s, 2, 800, 1)])
    # errors in a member that began calls ago
    n6 = len(m6)
    add("wrong crc, two calls on", gc.gz_member(t120, 6, crc=zlib.crc32(t120) ^ 0x10), [n6 // 3, 2 * n6 // 3], "wrong crc, two calls on")
    add("wrong crc, the trailer alone in the last call", gc.gz_member(t120, 6, crc=7), [n6 // 3, n6 - 8], "wrong crc, two calls on", "trailer byte 0")
    add("wrong isize, two calls on", gc.gz_member(t120, 6, isize=len(t120) + 1), [n6 // 3, 2 * n6 // 3], "wrong isize, two calls on")
    add("a stream cut short, continued", m6[:-n6 // 4], [n6 // 3, n6 // 2], "truncated stream, continued")
    add("a trailer cut short, continued", m6[:-3], [n6 // 3, n6 - 20], "truncated trailer, continued")
    add("a trailer cut short, in phase TRAILER", m6[:-3], [n6 // 3, n6 - 6], "truncated trailer, continued", pieces=(1024,))
    dm = next(c for c in gc.cases() if c.name == "damaged in the middle")
    add("damage in a continued member", dm.comp, [dm.consumed + 2000, dm.consumed + 9000], "damage, continued")
    add("E_SERIAL, continued", m0, [sb[1][0]], "E_SERIAL, continued", "stored block end", pieces=(1024,), max_rounds=1, stops=at_block[:1])
    assert len({f.name for f in out}) == len(out)
    return tuple(out)


# what a targeted feed states beyond zlib's text: {name: (error code, consumed of the last call, whether it leaves the state as it was)}
EXPECT = {
    "a distance in front of the member, two calls on": (gc.E_DATA, 0, True),
    "wrong crc, two calls on": (gc.E_CRC, 0, True), "wrong crc, the trailer alone in the last call": (gc.E_CRC, 0, True),
    "wrong isize, two calls on": (gc.E_LENGTH, 0, True),
    "a stream cut short, continued": (gc.E_TRUNCATED, 0, True), "a trailer cut short, continued": (gc.E_TRUNCATED, 0, True),
    "a trailer cut short, in phase TRAILER": (gc.E_TRUNCATED, 0, True), "damage in a continued member": (None, 0, True),
    "E_SERIAL, continued": (gc.E_SERIAL, 0, True),
}


def expect(f, calls, what):
    """the error of a feed that is built for one: reported by the LAST of its calls, of the member that was open at entry -- consumed 0,
    nothing delivered, the state as the call in front left it"""
    if f.name not in EXPECT:
        return
    code, consumed, unchanged = EXPECT[f.name]
    last = calls[-1]
    assert len(calls) >= 2 and all(c.info["error"] == 0 for c in calls[:-1]), what
    assert last.info["error"] == code if code is not None else last.info["error"] in (gc.E_DATA, gc.E_LENGTH, gc.E_CRC, gc.E_TRUNCATED), "%s: %s" % (what, last.info)
    assert (last.info["consumed"], last.info["n_bytes"], last.info["n_members"]) == (consumed, 0, 0), "%s: %s" % (what, last.info)
    assert not unchanged or (last.state == calls[-2].state and last.window == calls[-2].window), what
    assert calls[-2].state["phase"] != BETWEEN, what
    if f.name == "a trailer cut short, in phase TRAILER" or f.name == "wrong crc, the trailer alone in the last call":
        assert calls[-2].state["phase"] == TRAILER, what


def check_stops(f, calls, what):
    """the states a feed is built to leave: the call stopped where the edge needs it -- at that block's first bit, with that much text
    carried -- so that what the feed is credited with is what the next call met"""
    for k, want in f.stops:
        assert k < len(calls), "%s: no call %d" % (what, k)
        for field, v in want.items():
            got = calls[k].state[field]
            assert (v[0] <= got <= v[1]) if isinstance(v, tuple) else got == v, "%s: behind call %d %s is %d, built for %s" % (what, k, field, got, v)


def run_feed(call, f, piece, window=None):
    """one targeted feed at one piece size -> the edges it reached: those it is built for, once every check holds, and those seen"""
    what = "%s at %d" % (f.name, piece)
    calls = feed(call, f.comp, f.ends, piece, f.max_rounds, window=window)
    seen = check_calls(f.comp, calls, what, serial="E_SERIAL, continued" in f.edges)
    expect(f, calls, what)
    check_stops(f, calls, what)
    auto = {e for e in f.edges if e in AUTO}
    assert auto <= seen, "%s: built for %s, the calls reached %s" % (what, sorted(auto), sorted(seen))
    return seen | f.edges, calls


# the edges check_calls() sees for itself; the others are a feed's by construction
AUTO = frozenset(["cut in the fixed header", "cut at the first block", "cut in mid-block", "cut between members", "member over 3 calls", "header, no text", "no progress",
                  "window below 32768", "window of 32768", "window shifted twice"] + ["bit %d" % k for k in range(1, 8)] + ["trailer byte %d" % k for k in range(8)])
# the edges that tests reach outside feeds(): they state so through reached()
BY_TEST = frozenset(["overflow, continued", "member_bytes + 2^32"])


def overflow_continued(call, window=None):
    """A level-0 member (stored blocks): the first block, then the rest into room for little more than one block -- overflow, info says
    what is needed, nothing else is written and the state stands; a prefix that holds one more block succeeds into the same room.
    -> its edge"""
    t = gc.texts()[1]
    comp = gc.gz_member(t, 0)
    warr, waddr, wread = window or host_window()
    st = new_state(waddr)
    (p0, n0), (p1, n1), (p2, _) = stored_blocks(comp)[:3]
    cap = max(n0, n1) + 1000
    assert n0 + n1 >= WIN and len(t) - n0 > cap
    rc, i1, tx = call(comp[:p1], False, st, warr, 1024, 4000, cap)
    assert rc == 0 and (i1["error"], i1["overflow"], i1["n_bytes"], i1["consumed"]) == (0, 0, n0, p1) and st.phase == STREAM, i1
    before, wbefore, at = state_dict(st), wread().tobytes(), i1["consumed"]
    rc, i2, tx = call(comp[at:], True, st, warr, 1024, 4000, cap)
    assert rc == 0 and (i2["overflow"], i2["error"], i2["n_bytes"], i2["n_members"], i2["consumed"]) == (1, 0, len(t) - n0, 1, len(comp) - at), i2
    assert (tx == gc.CANARY).all() and state_dict(st) == before and wread().tobytes() == wbefore, "overflow wrote more than info"
    rc, i3, tx = call(comp[at:p2 + 100], False, st, warr, 1024, 4000, cap)
    assert rc == 0 and (i3["overflow"], i3["error"], i3["n_bytes"], i3["consumed"]) == (0, 0, n1, p2 - p1), i3
    assert bytes(tx[gc.FRONT:gc.FRONT + n1]) == t[n0:n0 + n1] and (tx[gc.FRONT + n1:] == gc.CANARY).all()
    assert st.member_bytes == n0 + n1 and st.crc == zlib.crc32(t[:n0 + n1]) and wread().tobytes() == t[n0 + n1 - WIN:n0 + n1]
    return {"overflow, continued"}


def isize_modulo(call, window=None):
    """member_bytes raised by 2^32 between two calls, as if 4 GiB of text had gone by: ISIZE is the length modulo 2^32, the member passes.
    -> its edge"""
    t = gc.texts()[2]
    comp = gc.gz_member(t, 6)
    warr, waddr, wread = window or host_window()
    st = new_state(waddr)
    rc, i1, tx = call(comp[:len(comp) // 2], False, st, warr, 4096, 0, len(t))
    assert rc == 0 and i1["error"] == 0 and i1["n_bytes"] >= WIN and st.phase == STREAM, i1
    st.member_bytes += 1 << 32
    rc, i2, tx2 = call(comp[i1["consumed"]:], True, st, warr, 4096, 0, len(t))
    assert rc == 0 and (i2["error"], i2["n_members"], i2["n_bytes"]) == (0, 1, len(t) - i1["n_bytes"]), i2
    assert bytes(tx[gc.FRONT:gc.FRONT + i1["n_bytes"]]) + bytes(tx2[gc.FRONT:gc.FRONT + i2["n_bytes"]]) == t
    assert (st.members, st.member_bytes, st.phase, st.total_bytes) == (1, 0, BETWEEN, len(t))
    return {"member_bytes + 2^32"}


def unreached(seen):
    return sorted(set(EDGES) - set(seen))
