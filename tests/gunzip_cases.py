"""A constructed catalogue for the piece-wise gunzip (faqcs_gunzip_host / faqcs_gunzip_device, include/faqcs_mi.h): every case is a file of
gzip members, what zlib makes of it, and the edges of the scheme it reaches; EDGES is the coverage table, and a test fails when an edge is
unreached.  Streams come from Python's zlib (wbits 31 and raw) and from the bit writer of deflate_streams.py, whose Stream records where
every block starts: the edges that are about blocks and piece ranges are asserted from those positions where the case is built.

What a case must give is stated by zlib_model(): zlib.decompressobj(31) member by member, as gzread goes.  It is the yardstick, never the
code under test; a case's own expectation (texts, bad member, code, consumed) is checked against it in test_gunzip_model.py.

The scheme's shapes the sizes come from (csrc/faqcs_gunzip.h): the compressed bytes are cut every piece_bytes bytes (PIECES: 1 024, 4 096
and 0, the default of 65 536); a run stops at the first block end at or behind its range end, so a block of more than piece_bytes
compressed bytes is a piece of its own; a marker is resolved within 32 768 symbols of its piece's end, elsewhere when the text is made."""
import ctypes as C
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

import deflate_streams as ds
import inflate_cases as ic
from faqcs_amd import _capi as capi

SEED = ic.SEED
PIECES = (1024, 4096, 0)
FRONT, CANARY = ic.FRONT, ic.CANARY
E_HEADER, E_LENGTH, E_DATA, E_CRC, E_TRUNCATED, E_SERIAL = (capi.INFLATE_E_HEADER, capi.INFLATE_E_LENGTH, capi.INFLATE_E_DATA, capi.INFLATE_E_CRC,
                                                            capi.INFLATE_E_TRUNCATED, capi.INFLATE_E_SERIAL)

# name; the file; the texts of the members in front of the first bad one; index of the bad member (None: none) and its code (None: any
# error); consumed; the piece sizes to run at; max_rounds; the edges
Case = namedtuple("Case", "name comp texts bad code consumed pieces max_rounds edges")

EDGES = {
    "level 1": "zlib level 1", "level 6": "zlib level 6", "level 9": "zlib level 9",
    "level 0": "stored blocks only: no piece but the first finds a start", "Z_FIXED": "no dynamic block at all",
    "Z_HUFFMAN_ONLY": "no match", "Z_RLE": "matches of distance 1",
    "block spans 3 pieces": "a block over three or more piece ranges", "several blocks in a range": "a piece range that holds several blocks",
    "block ends on a range end": "a block that ends exactly on a range end", "shorter than a piece": "a stream shorter than one piece",
    "distance 32768 across an edge": "a match of distance exactly 32 768 whose source lies in front of the piece",
    "markers of markers": "a marker copied by a match, copied on by a later piece", "source straddles the start": "dist < len, the source straddles the piece start",
    "false start": "a stored block carries a byte-aligned dynamic-block stream where a piece range begins",
    "members": "two to five members, a boundary in the middle of a piece", "window at member 2": "a distance in front of member 2's first byte",
    "fname": "FNAME", "fcomment": "FCOMMENT", "fextra": "FEXTRA", "fhcrc": "FHCRC", "bgzip": "a bgzip file", "empty member": "a member without text",
    "trailing garbage": "bytes behind the last member that are not gzip", "wrong crc": "in a late member", "wrong isize": "in a late member",
    "truncated stream": "the last member's stream is cut", "truncated trailer": "the last member's trailer is cut",
    "damaged mid piece": "a stream damaged in the middle of a chain piece", "header refused": "CM != 8, a reserved FLG bit",
    "E_SERIAL": "max_rounds = 1 on streams no probe splits", "many rounds": "the same streams with a large max_rounds",
}


def gz_member(text, level=6, strategy="default", raw=None, fname=None, fcomment=None, fextra=None, fhcrc=False, crc=None, isize=None, flg_or=0, cm=8):
    """One gzip member of `text` (RFC 1952).  raw: the deflate stream to use; crc / isize: trailer values to use; flg_or: bits to set in FLG."""
    data = ic.deflate_raw(text, level, strategy) if raw is None else raw
    flg = (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0) | flg_or
    head = struct.pack("<BBBBIBB", 31, 139, cm, flg, 0x5F3759DF, 2, 3)
    if fextra is not None:
        head += struct.pack("<H", len(fextra)) + fextra
    for s in (fname, fcomment):
        if s is not None:
            head += s + b"\0"
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + data + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF if crc is None else crc, (len(text) if isize is None else isize) & 0xFFFFFFFF)


def zlib_model(comp):
    """-> (texts of the members zlib takes whole, whether it stops with an error, consumed when it does not)"""
    comp, p, texts = bytes(comp), 0, []
    while p < len(comp):
        if comp[p] != 31 or (p + 1 < len(comp) and comp[p + 1] != 139):
            return texts, False, len(comp)
        d = zlib.decompressobj(31)
        try:
            t = d.decompress(comp[p:]) + d.flush()
        except zlib.error:
            return texts, True, p
        if not d.eof:
            return texts, True, p
        texts.append(t)
        p = len(comp) - len(d.unused_data)
    return texts, False, p


def block_starts(s):
    """bit positions of a Stream's block headers, and where the stream ends"""
    return [a for k, a, _ in s.fields if k == "block_header"], s.w.bitpos


def _lit(rng, n):
    return [int(v) for v in rng.integers(33, 127, n)]


def _structure_stream(rng, head):
    """One block over 3+ ranges of 1 024, six blocks inside one range, a stored block that ends on a multiple of 4 096 file bytes, a dynamic
    block that starts there, a final fixed block.  head: bytes of the member header in front of the stream."""
    s = ds.Stream()
    s.dynamic(_lit(rng, 5000), ds.PLAIN_LIT, ds.PLAIN_DIST)
    for _ in range(6):
        s.dynamic(_lit(rng, 30) + [(20, 25)], ds.PLAIN_LIT, ds.PLAIN_DIST)
    data_at = head + (s.w.bitpos + 3 + 7) // 8 + 4
    s.stored(bytes(_lit(rng, (-data_at) % 4096 + 4096)))
    on_edge = s.w.bitpos
    s.dynamic(_lit(rng, 700) + [(258, 600)], ds.PLAIN_LIT, ds.PLAIN_DIST)
    s.fixed(_lit(rng, 40), final=True)
    starts, end = block_starts(s)
    a, b = head * 8 + starts[0], head * 8 + starts[1]
    assert b // 8192 - a // 8192 >= 3                                         # block 0 lies over three ranges and more
    ranges = [(head * 8 + x) // 8192 for x in starts[1:7]]
    assert max(ranges.count(r) for r in ranges) >= 3                          # three of the small blocks and more start in one range
    assert (head * 8 + on_edge) % (8 * 4096) == 0 and on_edge in starts       # the stored block ends, and a dynamic one starts, on a range end
    return s


def _marker_stream(rng):
    """A: 33 000 stored bytes.  B (a piece of its own at 1 024 and 4 096): two literals, a match of length 50 and distance 5 -- three source
    bytes in front of the piece --, a match of distance 32 768, a match that copies markers, 4 600 literals.  C: a match whose source is what
    B copied, 4 600 literals."""
    s = ds.Stream()
    s.stored(rng.integers(0, 256, 33000, dtype=np.uint8).tobytes())
    head_b = [65, 66, (50, 5), (10, 32768), (20, 15)]
    n_b = 2 + 50 + 10 + 20 + 4600
    s.dynamic(head_b + _lit(rng, 4600), ds.PLAIN_LIT, ds.PLAIN_DIST)
    s.dynamic([(30, n_b - 62)] + _lit(rng, 4600), ds.PLAIN_LIT, ds.PLAIN_DIST, final=True)
    starts, end = block_starts(s)
    assert starts[2] - starts[1] > 8 * 4096 and end - starts[2] > 8 * 4096   # B and C are longer than a range: each its own piece
    return s


def _false_start_stream(rng, head):
    """A (dynamic, over a range of 1 024), S (stored: filler over the next range start, then a whole two-block dynamic stream byte-aligned,
    filler; ends inside that range), B (dynamic, final)."""
    inner = ds.Stream()
    inner.dynamic(_lit(rng, 120), ds.PLAIN_LIT, ds.PLAIN_DIST)
    inner.dynamic(_lit(rng, 60), ds.PLAIN_LIT, ds.PLAIN_DIST, final=True)
    copy = inner.getvalue()
    s = ds.Stream()
    s.dynamic(_lit(rng, 1500), ds.PLAIN_LIT, ds.PLAIN_DIST)
    data_at = head + (s.w.bitpos + 3 + 7) // 8 + 4
    edge = (data_at // 1024 + 1) * 1024
    f1 = edge - data_at + 16
    payload = bytes(_lit(rng, f1)) + copy + bytes(_lit(rng, 40))
    assert data_at + len(payload) < edge + 1024 - 8
    s.stored(payload)
    s.dynamic(_lit(rng, 300), ds.PLAIN_LIT, ds.PLAIN_DIST, final=True)
    return s


def _damaged_mid(rng, text):
    """a level-6 stream of `text` with one bit changed in its middle third that zlib notices"""
    raw = bytearray(ic.deflate_raw(text, 6))
    while True:
        i, b = int(rng.integers(len(raw) // 3, 2 * len(raw) // 3)), int(rng.integers(0, 8))
        raw[i] ^= 1 << b
        try:
            d = zlib.decompressobj(-15)
            if d.decompress(bytes(raw)) + d.flush() != text or not d.eof or d.unused_data:
                return bytes(raw)
        except zlib.error:
            return bytes(raw)
        raw[i] ^= 1 << b


@functools.lru_cache(maxsize=None)
def texts():
    """the FASTQ-shaped texts the zlib-written streams hold: 300, 200 and 120 KiB, reads of 150, 100 and 250"""
    rng = np.random.Generator(np.random.PCG64([307, SEED]))
    return tuple(ic.fastq_text(rng, n << 10, L) for n, L in ((300, 150), (200, 100), (120, 250)))


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.Generator(np.random.PCG64([311, SEED]))
    t300, t200, t120 = texts()
    out = []

    def add(name, comp, tx, *edges, bad=None, code=0, consumed=None, pieces=PIECES, max_rounds=0):
        for e in edges:
            assert e in EDGES, e
        out.append(Case(name, bytes(comp), tuple(tx), bad, code, len(comp) if consumed is None else consumed, tuple(pieces), max_rounds, frozenset(edges)))

    for lv, t in ((1, t300), (6, t200), (9, t120)):
        add("level %d" % lv, gz_member(t, lv), [t], "level %d" % lv)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    add("zlib's own gzip wrapper", co.compress(t120) + co.flush(), [t120], "level 6")
    serial = {"level 0": gz_member(t200, 0), "Z_FIXED": gz_member(t120, 6, "fixed")}
    for edge, m in serial.items():
        add(edge + ", rounds as needed", m, [t200 if edge == "level 0" else t120], edge, "many rounds", max_rounds=4000)
        add(edge + ", max_rounds = 1", m, [], edge, "E_SERIAL", bad=0, code=E_SERIAL, consumed=0, pieces=(1024,), max_rounds=1)
    add("Z_HUFFMAN_ONLY", gz_member(t120, 6, "huffman"), [t120], "Z_HUFFMAN_ONLY", max_rounds=4000)
    add("Z_RLE", gz_member(t120, 6, "rle"), [t120], "Z_RLE", max_rounds=4000)
    s = _structure_stream(rng, 10)
    t = ds.expand(s.items)
    add("blocks against the ranges", gz_member(t, raw=s.getvalue()), [t], "block spans 3 pieces", "several blocks in a range", "block ends on a range end", max_rounds=64)
    small = t300[:300]
    m = gz_member(small, 6)
    assert len(m) < 1024
    add("shorter than one piece", m, [small], "shorter than a piece")
    s = _marker_stream(rng)
    t = ds.expand(s.items)
    add("markers", gz_member(t, raw=s.getvalue()), [t], "distance 32768 across an edge", "markers of markers", "source straddles the start")
    s = _false_start_stream(rng, 10)
    t = ds.expand(s.items)
    add("false start", gz_member(t, raw=s.getvalue()), [t], "false start")
    # members
    parts = [t120, t300[:150000], t200[:101000]]
    ms = [gz_member(p, lv) for p, lv in zip(parts, (6, 1, 9))]
    assert all(len(b"".join(ms[:k])) % 4096 not in (0, 4095) for k in (1, 2))
    add("three members", b"".join(ms), parts, "members")
    five = [t300[i * 30000:(i + 1) * 30000] for i in range(5)]
    add("five members", b"".join(gz_member(p, 6) for p in five), five, "members")
    bad2 = gz_member(b"aaa", raw=ic.fixed_block_first_symbol_is_a_match())
    add("member 2 starts with a match", ms[0] + bad2 + ms[1], parts[:1], "window at member 2", bad=1, code=E_DATA, consumed=len(ms[0]))
    deep = ds.Stream().stored(t200[:20000]).fixed([1, 2, (258, 20003), 3], final=True)
    bad2 = gz_member(t200[:20000] + bytes(261), raw=deep.getvalue())
    add("member 2 reaches one byte in front of itself", ms[0] + bad2, parts[:1], "window at member 2", bad=1, code=E_DATA, consumed=len(ms[0]))
    hs = [gz_member(five[0], 6, fname=b"reads.fastq"), gz_member(five[1], 6, fcomment=b"made by hand"), gz_member(five[2], 6, fextra=b"ZZ\x03\x00abc"),
          gz_member(five[3], 6, fhcrc=True), gz_member(five[4], 1, fname=b"a", fcomment=b"b", fextra=b"", fhcrc=True)]
    add("header fields", b"".join(hs), five, "fname", "fcomment", "fextra", "fhcrc", "members")
    add("a long FEXTRA and FNAME", gz_member(five[0], 6, fextra=b"QQ" + struct.pack("<H", 3000) + bytes(3000), fname=b"n" * 2000), five[:1], "fextra", "fname")
    chunks = [t200[i:i + 65280] for i in range(0, len(t200), 65280)]
    add("a bgzip file", b"".join(ic.member(c) for c in chunks) + ic.EOF_MEMBER, chunks + [b""], "bgzip", "members", "empty member", max_rounds=4)
    add("an empty member alone", gz_member(b"", 6), [b""], "empty member")
    add("an empty member between members", ms[2] + gz_member(b"", 9) + ms[0], [parts[2], b"", parts[0]], "empty member", "members")
    for junk in (b"\0", b"\0\0\0\0 the end", b"\x1f\x00", b"\n" * 40):
        add("trailing garbage %r" % junk[:4], ms[2] + junk, [parts[2]], "trailing garbage")
    add("nothing", b"", [], "trailing garbage")
    add("no gzip at all", b"@r1\nACGT\n+\nIIII\n", [], "trailing garbage")
    # damage in a late member
    good = ms[2] + ms[0]
    at3 = len(good)
    add("wrong crc in member 3", good + gz_member(five[0], 6, crc=zlib.crc32(five[0]) ^ 0x10), [parts[2], parts[0]], "wrong crc", bad=2, code=E_CRC, consumed=at3)
    add("wrong isize in member 3", good + gz_member(five[0], 6, isize=len(five[0]) + 1), [parts[2], parts[0]], "wrong isize", bad=2, code=E_LENGTH, consumed=at3)
    add("wrong crc and isize in member 3", good + gz_member(five[0], 6, crc=1, isize=7), [parts[2], parts[0]], "wrong isize", "wrong crc", bad=2, code=E_LENGTH, consumed=at3)
    third = gz_member(five[0], 6)
    for cut, edge in ((len(third) // 2, "truncated stream"), (9, "truncated stream"), (8, "truncated trailer"), (3, "truncated trailer"), (1, "truncated trailer")):
        add("member 3 cut %d bytes short" % cut, good + third[:-cut], [parts[2], parts[0]], edge, bad=2, code=E_TRUNCATED, consumed=at3)
    for keep in (1, 2, 3, 9, 11):
        add("member 3 is %d bytes of header" % keep, good + gz_member(five[0], 6, fname=b"x")[:keep], [parts[2], parts[0]], "truncated stream", bad=2, code=E_TRUNCATED, consumed=at3)
    add("damaged in the middle", ms[2] + gz_member(t200, raw=_damaged_mid(rng, t200)), [parts[2]], "damaged mid piece", bad=1, code=None, consumed=len(ms[2]))
    add("member 2 has CM 7", ms[2] + gz_member(five[0], 6, cm=7), [parts[2]], "header refused", bad=1, code=E_HEADER, consumed=len(ms[2]))
    add("member 2 has a reserved FLG bit", ms[2] + gz_member(five[0], 6, flg_or=0x40), [parts[2]], "header refused", bad=1, code=E_HEADER, consumed=len(ms[2]))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def coverage():
    """{edge: the cases that reach it}"""
    cov = {e: [] for e in EDGES}
    for c in cases():
        for e in c.edges:
            cov[e].append(c.name)
    return cov


def runs():
    """(case, piece_bytes) of the whole catalogue"""
    return [(c, p) for c in cases() for p in c.pieces]


def info_dict(info):
    return {f: int(getattr(info, f)) for f, _ in capi.GunzipInfo._fields_}


def gunzip_host(lib, comp, piece_bytes, max_rounds, capacity):
    """One faqcs_gunzip_host into canary-filled buffers -> (rc, info dict, the WHOLE text buffer: FRONT canaries, capacity bytes, 64 canaries)"""
    comp = bytes(comp)
    cb = np.frombuffer(comp, np.uint8).copy() if comp else np.zeros(1, np.uint8)
    text = ic.pc.aligned_bytes(FRONT + capacity + 64)
    info = capi.GunzipInfo()
    C.memset(C.byref(info), 0xFF, C.sizeof(info))
    out = capi.GunzipOut(text.ctypes.data + FRONT, capacity, C.addressof(info))
    rc = lib.faqcs_gunzip_host(cb.ctypes.data if comp else None, len(comp), piece_bytes, max_rounds, C.byref(out))
    return rc, info_dict(info), text


def assert_case(c, info, text, what):
    """info and text (the layout of gunzip_host) against the case: the text of the members in front of the bad one byte for byte, nothing in
    front of it, and -- for the host statement -- nothing behind it"""
    want = b"".join(c.texts)
    assert info["overflow"] == 0, what
    assert (info["n_bytes"], info["n_members"], info["consumed"]) == (len(want), len(c.texts), c.consumed), "%s: %s" % (what, info)
    if c.bad is None:
        assert info["error"] == 0, "%s: %s" % (what, info)
    else:
        assert info["n_members"] == c.bad and (info["error"] == c.code if c.code is not None else info["error"] in (E_DATA, E_LENGTH, E_CRC, E_TRUNCATED)), "%s: %s" % (what, info)
    got = bytes(text[FRONT:FRONT + len(want)])
    if got != want:
        i = next(k for k in range(len(want)) if got[k] != want[k])
        raise AssertionError("%s: first differing byte %d of %d: got %r want %r" % (what, i, len(want), got[i:i + 12], want[i:i + 12]))
    assert (text[:FRONT] == CANARY).all(), what + ": bytes in front of the text were written"
