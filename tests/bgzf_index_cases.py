"""A constructed catalogue for the BGZF index (faqcs_bgzf_index_host / faqcs_bgzf_index_device, include/faqcs_mi.h): every case is
(bytes, final, capacity_members) and names the edges it reaches; EDGES is the coverage table, and a test fails when an edge is unreached.

The index reads headers only: it follows BSIZE from byte 0 and never looks at a deflate stream, a CRC or ISIZE.  So the members here are a
header, a body of chosen bytes and a trailer -- built with struct, sized to the byte -- and only the chain into faqcs_inflate_device
(test_gpu_bgzf_index.py) uses members zlib would take (inflate_cases.member).

What a case must give is stated by walk(), a plain-Python restatement of the walk written from the text of include/faqcs_mi.h (and of
BgzfReader::member_size's rule for the BC subfield).  It is not the code under test: faqcs_bgzf_index_host has to agree with it
(test_bgzf_index_model.py) before the device is asked, and the device is compared with the host statement byte for byte.

The kernels' shapes the sizes come from (faqcs_bgzf_index_kernel.hip): a tile is TILE = 16 384 positions (256 threads x 4 vectors of 16
bytes), the block scan has a wave level (64 threads) and a block level, the one-block scan of the tile counts takes 1 024 tiles per turn,
and a round of pointer jumping doubles the ranks that are known.

IMPOSTORS are bytes inside a member that pass the header test -- ID, CM, FEXTRA, XLEN and a BC subfield with a size of 26 or more -- at a
position the chain from byte 0 never lands on.  A header's BC subfield holds SLEN = 02 00, so an impostor placed where FNAME or FCOMMENT
stands ends that string at its first zero byte for a gzip reader; the index does not parse either and sees the bytes as they are.
"An impostor at each of the last 18 bytes of a member" is built twice: with the data ending behind the member (the header test has
avail = 1 .. 18 there) and with a member behind it (the header's later bytes are then the next member's)."""
import ctypes as C
import functools
import struct
from collections import namedtuple

import numpy as np

from faqcs_amd import _capi as capi

TILE = 16384
SCAN_TILES = 1024           # tiles per turn of the one-block scan of the tile counts
MIN_MEMBER = 26
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CAN32 = 0xA5A5A5A5
# 28-byte members that fill SCAN_TILES tiles and one more: the tile scan takes a second turn (its second level), every tile's block scan has
# both of its levels (585 candidates in 256 threads), and ranks up to 2^19 make 20 rounds of pointer jumping say something
DENSE_MEMBERS = (SCAN_TILES + 1) * TILE // len(EOF_MEMBER) + 1

Case = namedtuple("Case", "name comp final capacity edges")

EDGES = {
    # the ends of the data
    "avail=1": "the walk stops with one byte left, 1f", "avail=2": "1f 8b and nothing more", "avail=3": "three bytes left",
    "avail=17": "a header short of its 18 bytes", "avail=12+xlen-1": "the extra field short of one byte", "avail=ms-1": "a member short of one byte",
    "partial,final=0": "an incomplete last member left to the caller", "partial,final=1": "an incomplete last member is E_TRUNCATED",
    "stop at n": "the data ends behind a member",
    # what can stand behind a well-formed chain
    "1f then not 8b": "ends the data", "not 1f": "ends the data", "cm!=8": "E_HEADER", "fextra unset": "E_HEADER", "no bc": "E_HEADER",
    "bc slen=3": "a BC subfield of another length is passed over", "bc overruns xlen": "a BC cut off by XLEN is not taken",
    "size below min": "a stated size of MIN_MEMBER - 1 is E_HEADER", "reserved flg bit": "indexed: not the index's business",
    "subfield skipped": "a subfield in front of BC",
    # impostors
    "impostor in stored": "in a stored block's payload", "impostor in fname": "where FNAME stands", "impostor in fcomment": "where FCOMMENT stands",
    "impostor in extra": "in an FEXTRA subfield in front of the real BC", "impostor merges": "its stated size lands on a true member boundary",
    "impostor mid-member": "its stated size lands inside a later member", "impostor beyond n": "its stated size lands behind the data",
    "impostor at last 18, data ends": "a header starts j = 1 .. 18 bytes in front of the data's end",
    "impostor at last 18, member follows": "a header starts j = 1 .. 18 bytes in front of a member's end",
    # density and size
    "dense chain": "%d members of 28 bytes" % DENSE_MEMBERS, "member of 65536": "BSIZE = 65 535, four tiles",
    "header at tile boundary": "a member starts at T - 18 .. T", "bc in next tile": "XLEN carries the BC subfield over a tile boundary",
    # placement and capacity
    "n_comp=0": "no bytes", "one member": "one member alone", "capacity=n-1": "overflow", "capacity=n": "fits", "capacity=n+1": "fits with room",
    "capacity=0": "overflow with members, fits without",
}
# edges walk() observes itself; the impostor edges are observed by impostors(); the rest are facts of the construction, asserted where built
WALK_EDGES = {"avail=1", "avail=2", "avail=3", "avail=17", "avail=12+xlen-1", "avail=ms-1", "partial,final=0", "partial,final=1", "stop at n",
              "1f then not 8b", "not 1f", "cm!=8", "fextra unset", "no bc", "bc slen=3", "bc overruns xlen", "size below min", "reserved flg bit",
              "subfield skipped"}
IMPOSTOR_EDGES = {"impostor merges", "impostor mid-member", "impostor beyond n"}


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def member_size(b, p, avail, seen):
    """BSIZE + 1 of the header at b[p:] with avail bytes, 0: not a BGZF member header."""
    if avail < 18 or b[p] != 0x1F or b[p + 1] != 0x8B or b[p + 2] != 8 or not b[p + 3] & 4:
        return 0
    xlen = b[p + 10] | b[p + 11] << 8
    if avail < 12 + xlen:
        return 0
    x = 0
    while x + 4 <= xlen:
        f = p + 12 + x
        slen = b[f + 2] | b[f + 3] << 8
        if b[f] == 0x42 and b[f + 1] == 0x43:
            if slen == 2 and x + 6 <= xlen:
                return (b[f + 4] | b[f + 5] << 8) + 1
            seen.add("bc slen=3" if slen == 3 else "bc overruns xlen" if slen == 2 else "bc slen other")
        else:
            seen.add("subfield skipped")
        x += 4 + slen
    return 0


def at(b, n, p, seen):
    """What the walk decides at position p: ("member", size), ("stop",), ("end",), ("header",) or ("partial",)."""
    avail = n - p
    if avail == 0:
        seen.add("stop at n")
        return ("stop",)
    if b[p] != 0x1F:
        seen.add("not 1f")
        return ("end",)
    if avail >= 2 and b[p + 1] != 0x8B:
        seen.add("1f then not 8b")
        return ("end",)
    if avail >= 4 and b[p + 2] != 8:
        seen.add("cm!=8")
        return ("header",)
    if avail >= 4 and not b[p + 3] & 4:
        seen.add("fextra unset")
        return ("header",)
    if avail >= 18 and avail >= 12 + (b[p + 10] | b[p + 11] << 8):
        ms = member_size(b, p, avail, seen)
        if ms == 0:
            seen.add("no bc")
            return ("header",)
        if ms < MIN_MEMBER:
            seen.add("size below min")
            return ("header",)
        if ms <= avail:
            if b[p + 3] & 0xE0:
                seen.add("reserved flg bit")
            return ("member", ms)
        if avail == ms - 1:
            seen.add("avail=ms-1")
    else:
        for a in (1, 2, 3, 17):
            if avail == a:
                seen.add("avail=%d" % a)
        if avail >= 18 and avail == 12 + (b[p + 10] | b[p + 11] << 8) - 1:
            seen.add("avail=12+xlen-1")
    return ("partial",)


def walk(comp, final, capacity):
    """-> (info dict, member_offset list or None on overflow, the WALK_EDGES seen)"""
    b, n, p, offs, seen = bytes(comp), len(comp), 0, [0], set()
    while True:
        d = at(b, n, p, seen)
        if d[0] != "member":
            break
        p += d[1]
        offs.append(p)
    error = 0
    if d[0] == "header":
        error = capi.INFLATE_E_HEADER
    elif d[0] == "partial":
        seen.add("partial,final=%d" % (1 if final else 0))
        error = capi.INFLATE_E_TRUNCATED if final else 0
    k = len(offs) - 1
    info = {"consumed": n if d[0] == "end" else p, "n_members": k, "overflow": 1 if k > capacity else 0, "error": error}
    return info, (None if info["overflow"] else offs), seen


def impostors(comp):
    """[(position, stated size)] of the positions off the chain whose bytes pass the header test with all of comp behind them, and the
    IMPOSTOR_EDGES they make."""
    b, n = bytes(comp), len(comp)
    chain, p = {0}, 0
    while True:
        d = at(b, n, p, set())
        if d[0] != "member":
            break
        p += d[1]
        chain.add(p)
    found, seen, q = [], set(), b.find(b"\x1f\x8b\x08")
    while q >= 0:
        ms = 0 if q in chain else member_size(b, q, n - q, set())
        if ms >= MIN_MEMBER:
            found.append((q, ms))
            seen.add("impostor beyond n" if q + ms > n else "impostor merges" if q + ms in chain else "impostor mid-member")
        q = b.find(b"\x1f\x8b\x08", q + 1)
    return found, seen


# ---- construction -------------------------------------------------------------------------------------------------------------------
def header(size, flg=4, extra_front=b"", bc=b"BC", slen=2, xlen=None, cm=8, id2=0x8B):
    """A member header that states `size` bytes: 12 bytes, the subfields in front, the BC subfield."""
    extra = extra_front + bc + struct.pack("<HH", slen, (size - 1) & 0xFFFF) + (b"\0" if slen == 3 else b"")
    return struct.pack("<BBBBIBBH", 31, id2, cm, flg, 0x01010101, 1, 255, len(extra) if xlen is None else xlen) + extra


def fake(size, fill=0x55, body=None, **kw):
    """A member of exactly `size` bytes for the index: header, body (given bytes first, `fill` behind them), an 8-byte trailer."""
    h = header(size, **kw)
    body = b"" if body is None else body
    room = size - len(h) - 8
    assert room >= len(body), "the member is too small for its body"
    return h + body + bytes([fill]) * (room - len(body)) + struct.pack("<II", 0x11223344, 0)


def stored_with(payload):
    """The body of a member whose deflate stream is one stored block of `payload`."""
    return struct.pack("<BHH", 1, len(payload), len(payload) ^ 0xFFFF) + payload


def subfield(si, data):
    return si + struct.pack("<H", len(data)) + data


def chain_of(sizes, **kw):
    return b"".join(fake(s, fill=0x40 + i % 32, **kw) for i, s in enumerate(sizes))


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, comp, final, capacity, *edges):
        for e in edges:
            assert e in EDGES, e
        out.append(Case(name, bytes(comp), int(final), int(capacity), frozenset(edges)))

    front = chain_of([40, 26, 300])  # a well-formed chain in front of what is tried
    # the ends of the data: every length 1 .. ms - 1 of a last member, final 0 and 1.  XLEN = 30: avail = 17, 12 + XLEN - 1 = 41, ms - 1 = 59
    last = fake(60, extra_front=subfield(b"ZZ", b"q" * 20))
    assert struct.unpack_from("<H", last, 10)[0] == 30
    named = {1: "avail=1", 2: "avail=2", 3: "avail=3", 17: "avail=17", 41: "avail=12+xlen-1", 59: "avail=ms-1"}
    for cut in range(1, len(last)):
        for final in (0, 1):
            add("last member cut to %d, final=%d" % (cut, final), front + last[:cut], final, 8, "partial,final=%d" % final,
                *([named[cut]] if cut in named else []), *(["subfield skipped"] if cut >= 42 else []))
    add("last member whole", front + last, 1, 8, "stop at n", "subfield skipped")
    # what can stand behind a well-formed chain
    behind = {
        "1f then not 8b": b"\x1f\x8c" + b"x" * 40, "not 1f": b"\x00" + b"x" * 40, "cm!=8": header(60, cm=7) + b"x" * 42,
        "fextra unset": header(60, flg=0) + b"x" * 42, "no bc": header(60, bc=b"XY") + b"x" * 42,
        "bc slen=3": header(60, slen=3) + b"x" * 41, "bc overruns xlen": header(60, xlen=5) + b"x" * 42,
        "size below min": header(MIN_MEMBER - 1) + b"x" * 42, "reserved flg bit": fake(60, flg=4 | 0x80),
    }
    for edge, tail in behind.items():
        for final in (0, 1):
            add("%s behind the chain, final=%d" % (edge, final), front + tail, final, 8, edge)
        add("%s at byte 0" % edge, tail, 1, 8, edge)
    add("1f alone in front of the end, then not 8b in two bytes", front + b"\x1f\x00", 1, 8, "1f then not 8b")
    add("a BC of SLEN 3 in front of the real BC", front + fake(80, extra_front=b"BC" + struct.pack("<H", 3) + b"abc") + front, 1, 16, "bc slen=3", "stop at n")
    add("a BC cut off by XLEN behind a subfield", front + header(60, extra_front=subfield(b"AB", b"12"), xlen=11) + b"x" * 40, 1, 8, "bc overruns xlen", "subfield skipped", "no bc")
    # impostors: a complete header with BC inside a member.  The chain is [front 366][host 4000][after 500][after 700] ...
    host_at, host = len(front), 4000
    tails = chain_of([500, 700, 90])
    boundary, middle = host + 500, host + 500 + 333  # relative to the host member's start: a true boundary, the middle of a member

    def hosted(place, q_body, target):
        """the host member with an impostor in `place` whose stated size carries it from its position to `target` (relative to the host's start)"""
        kw, lead = {}, b""
        if place == "impostor in extra":
            pre = subfield(b"YY", b"p" * q_body) if q_body else b""
            pos = 12 + len(pre) + 4                        # the impostor is the data of a subfield
            kw["extra_front"] = pre + subfield(b"ZZ", header(target - pos))
        elif place == "impostor in stored":
            pos = 18 + 5 + q_body
            lead = stored_with(b"s" * q_body + header(target - pos) + b"s" * 50)
        else:                                              # FNAME / FCOMMENT stand behind the extra field
            pos = 18 + q_body
            kw["flg"] = 4 | (8 if place == "impostor in fname" else 16)
            lead = b"n" * q_body + header(target - pos) + b"\0"
        m = fake(host, body=lead, **kw)
        assert m[pos:pos + 4] == b"\x1f\x8b\x08\x04"
        return m

    for place in ("impostor in stored", "impostor in fname", "impostor in fcomment", "impostor in extra"):
        for q_body in (0, 7):
            for edge, target in (("impostor merges", boundary), ("impostor mid-member", middle), ("impostor beyond n", 60000)):
                add("%s at +%d, %s" % (place, q_body, edge), front + hosted(place, q_body, target) + tails, 1, 16, place, edge, "stop at n")
    add("an impostor merges, and the data ends in a cut member", front + hosted("impostor in stored", 3, boundary) + tails[:-5], 0, 16, "impostor in stored", "impostor merges", "partial,final=0")
    add("a chain of impostors inside one member", front + fake(2000, body=stored_with(chain_of([100, 200, 300]) + b"z" * 9)) + tails, 1, 16, "impostor in stored", "impostor mid-member")
    # an impostor header that starts j bytes in front of the data's end, and in front of a member's end with a member behind it
    for j in range(1, 19):
        imp = header(64)[:j]
        m = fake(200)
        add("header pattern %d bytes in front of the data's end" % j, front + m[:200 - j] + imp, 1, 16, "impostor at last 18, data ends", "stop at n")
        add("header pattern %d bytes in front of a member's end" % j, front + m[:200 - j] + imp + tails, 1, 16, "impostor at last 18, member follows", "stop at n")
    # density and size
    add("dense chain", EOF_MEMBER * DENSE_MEMBERS, 1, DENSE_MEMBERS, "dense chain", "stop at n")
    add("dense chain cut in its last member, capacity short", EOF_MEMBER * 3000 + EOF_MEMBER[:27], 0, 2999, "dense chain", "capacity=n-1", "partial,final=0", "avail=ms-1")
    big = fake(65536, body=stored_with(b"B" * 65505))
    assert len(big) == 65536 and big[16:18] == b"\xff\xff"
    add("a member of exactly 65 536 bytes between small ones", front + big + tails, 1, 16, "member of 65536", "stop at n")
    add("members of 65 536 bytes and an impostor in the last", big + big + fake(65536, body=stored_with(header(65536) + b"B" * 65000)) + tails, 1, 16,
        "member of 65536", "impostor in stored", "impostor mid-member")
    for d in range(19):
        s = TILE - 18 + d
        add("a member starts at T - 18 + %d" % d, fake(s) + tails, 1, 16, "header at tile boundary", "stop at n")
        add("a member starts at 3 T - 18 + %d behind a dense run" % d, EOF_MEMBER * 1000 + fake(3 * TILE - 18 + d - 28000) + tails, 1, 1100, "header at tile boundary", "dense chain")
    add("XLEN carries BC into the next tile", fake(TILE - 20) + fake(9000, extra_front=subfield(b"ZZ", b"e" * 4000)) + tails, 1, 16, "bc in next tile", "subfield skipped", "stop at n")
    wide = fake(40000, extra_front=subfield(b"ZZ", b"e" * 33000))
    add("XLEN carries BC over two tile boundaries", fake(TILE - 20) + wide + tails, 1, 16, "bc in next tile", "subfield skipped", "stop at n")
    add("an extra field of two tiles, cut inside it", fake(TILE - 20) + wide[:30000], 0, 16, "partial,final=0")
    # placement and capacity
    add("no bytes", b"", 1, 4, "n_comp=0", "stop at n")
    add("no bytes, capacity 0", b"", 0, 0, "n_comp=0", "capacity=0", "stop at n")
    add("one member alone", EOF_MEMBER, 1, 1, "one member", "capacity=n", "stop at n")
    add("one member alone, 65 536 bytes", big, 1, 1, "one member", "member of 65536", "capacity=n")
    seven = chain_of([30, 26, 1000, 28, 64, 5000, 77])
    for edge, cap in (("capacity=n-1", 6), ("capacity=n", 7), ("capacity=n+1", 8), ("capacity=0", 0)):
        add("seven members, %s" % edge, seven, 1, cap, edge, "stop at n")
        add("seven members and an error behind them, %s" % edge, seven + header(60, bc=b"XY") + b"x" * 42, 1, cap, edge, "no bc")
    add("no member, capacity 0", b"not gzip", 1, 0, "capacity=0", "not 1f")
    return tuple(out)


def residue_case():
    """the case the GPU test places at every residue mod 16: members, impostors and a cut end over a tile boundary"""
    return chain_of([TILE - 100, 26]) + fake(3000, body=stored_with(header(2500) + b"s" * 40)) + EOF_MEMBER * 40 + header(60)[:13]


# ---- the host statement into canary-filled arrays -----------------------------------------------------------------------------------
def index_host(lib, comp, final, capacity):
    """faqcs_bgzf_index_host -> (rc, info dict, the WHOLE offset array: a canary, capacity + 1 entries, a canary)"""
    buf = np.frombuffer(bytes(comp), np.uint8).copy() if len(comp) else np.zeros(1, np.uint8)
    off = np.full(capacity + 3, CAN32, np.uint32)
    info = capi.BgzfIndexInfo()
    C.memset(C.byref(info), 0xFF, C.sizeof(info))
    rc = lib.faqcs_bgzf_index_host(buf.ctypes.data if len(comp) else None, len(comp), final, off.ctypes.data + 4, capacity, C.byref(info))
    return rc, {f: int(getattr(info, f)) for f, _ in capi.BgzfIndexInfo._fields_}, off


def expected_offsets(offs, capacity):
    """walk()'s offsets in the layout of index_host()"""
    off = np.full(capacity + 3, CAN32, np.uint32)
    if offs is not None:
        off[1:1 + len(offs)] = offs
    return off


# ---- the randomised round -----------------------------------------------------------------------------------------------------------
def random_input(rng):
    """A concatenation of catalogue members and impostor payloads, an end of some kind behind it: (bytes, final, capacity)."""
    parts = []
    for _ in range(int(rng.integers(0, 9))):
        r = int(rng.integers(0, 8))
        size = int(rng.integers(MIN_MEMBER, 400)) if r < 6 else int(rng.integers(400, 40000))
        if r == 0:
            parts.append(EOF_MEMBER * int(rng.integers(1, 30)))
        elif r == 1 and size >= 80:
            parts.append(fake(size, body=stored_with(header(int(rng.integers(MIN_MEMBER, 3000))) + b"i" * int(rng.integers(0, size - 79)))))
        elif r == 2:
            parts.append(fake(size + 40, extra_front=subfield(b"ZZ", header(int(rng.integers(MIN_MEMBER, 3000))))))
        elif r == 3:
            parts.append(fake(size + 60, flg=4 | 8 | 0x20, body=b"nm" + header(int(rng.integers(MIN_MEMBER, 65537))) + b"\0"))
        else:
            parts.append(fake(size, fill=int(rng.integers(0, 256))))
    comp = b"".join(parts)
    e = int(rng.integers(0, 8))
    if e == 0 and parts:
        comp = comp[:len(comp) - int(rng.integers(1, min(len(parts[-1]), 70)))]
    elif e == 1:
        comp += [b"\x1f", b"\x1f\x8b", b"\x1f\x8b\x08", b"\x1f\x8c", b"\x00\x1f\x8b", b"\x1f\x8b\x07\x04", b"\x1f\x8b\x08\x00"][int(rng.integers(0, 7))]
    elif e == 2:
        comp += [header(60, bc=b"XY"), header(25), header(60, slen=3), header(60, xlen=5), header(60)[:17], header(3000)][int(rng.integers(0, 6))] + b"t" * int(rng.integers(0, 30))
    n = walk(comp, 1, 1 << 30)[0]["n_members"]
    capacity = max(0, n + int(rng.integers(-1, 3))) if rng.random() < 0.3 else n + 4
    return comp, int(rng.integers(0, 2)), capacity
