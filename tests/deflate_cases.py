"""Texts and checks of the deflate tests (faqcs_deflate_device / faqcs_deflate_host): the member shapes of inflate_cases.py, an
Illumina-shaped text, texts built to reach one rule of the encoder each, and the format check of a compressed file.  The yardstick is always
Python's zlib and gzip, never the code under test."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np

import inflate_cases as ic
import parse_cases as pc
from faqcs_amd import _capi as capi

SEED = ic.SEED
CANARY, CAN32, FRONT = ic.CANARY, ic.CAN32, ic.FRONT
MAX_TEXT = 65280
HEADER = bytes.fromhex("1f8b08040000000000ff0600424302 00".replace(" ", ""))  # the 16 bytes in front of BSIZE
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 260, 4095, 4096, 4097, 65279, 65280, 65281, 200000)
MEMBER_BYTES = (1, 64, 259, 4096, 0)
MOST_MEMBERS = 70000


def illumina_text(n_bytes, L=150, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed)); out = []; tot = 0; x = 1000; tile = 1101
    qa = np.frombuffer(b"F:,#", np.uint8)
    while tot < n_bytes:
        x += int(rng.integers(1, 40)); y = int(rng.integers(1000, 37000))
        if x > 32000: x = 1000; tile += 1
        d = b"@A00789:123:HXYZ2DSXX:1:%d:%d:%d 1:N:0:ACGTACGT+TGCATGCA" % (tile, x, y)
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)]
        q = qa[np.minimum(rng.geometric(0.8, L) - 1, 3)].copy()
        k = int(rng.integers(0, 40))
        if k < 10: q[L - k * 3:] = ord("#")
        r = d + b"\n" + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n"; out.append(r); tot += len(r)
    return b"".join(out)[:n_bytes]


def grid_cases(shape):
    """(n_text, member_bytes, final) of the size grid for one shape; pairs of more than MOST_MEMBERS members are left out."""
    for n in SIZES:
        for mb in MEMBER_BYTES:
            if -(-n // (mb or MAX_TEXT)) > MOST_MEMBERS:
                continue
            for final in (0, 1):
                yield n, mb, final


def grid_text(shape, n):
    return ic.shape_text(np.random.Generator(np.random.PCG64([211, ic.SHAPES.index(shape), n, SEED])), shape, n)


def no_repeated_trigram(rng, n=4000, lo=0, hi=256):
    """n bytes of the values lo .. hi - 1 in which no three consecutive bytes occur twice (a byte that would repeat a trigram is drawn again)."""
    out, seen = bytearray(rng.integers(lo, hi, 2, dtype=np.uint8).tobytes()), set()
    while len(out) < n:
        b = int(rng.integers(lo, hi))
        t = (out[-2], out[-1], b)
        if t not in seen:
            seen.add(t)
            out.append(b)
    return bytes(out)


def single_distance(rng):
    """Matches at one distance only: 2 048 bytes without a repeated trigram, twice."""
    a = no_repeated_trigram(rng, 2048)
    return a + a


def far_repeat(rng, distances):
    """65 280 bytes of one filler byte but for 40 rare bytes in front of each copy and, D bytes behind them, the same 40 bytes -- one pair
    per D of `distances`, every pair with bytes of its own.  A copy starts where a 1 024-byte tile of the member starts, and between a
    source and its copy lies nothing but filler and the other pairs (a few hundred bytes): the encoder's table of latest positions still
    points at the source when the copy is looked up, so whether the match is taken is decided by its distance alone."""
    t = bytearray(b"z" * MAX_TEXT)
    for k, D in enumerate(distances):
        T = 1024 * (63 - 2 * k)
        src = rng.integers(130, 250, 40, dtype=np.uint8).tobytes()
        assert T - D >= 0 and T + 40 <= MAX_TEXT
        t[T - D:T - D + 40] = src
        t[T:T + 40] = src
    return bytes(t)


DISTANCE_OF_CODE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769) + tuple(
    b + 16 * (k + 1) for k, b in enumerate((1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)))  # (no two sources in one place)


def every_length_and_distance_code(rng):
    """Two members of 65 280 bytes.  The first holds, for every length L = 3 .. 258, a run of L + 1 equal bytes between runs of other bytes:
    a literal and a match of length L at distance 1.  The second is one filler byte but for eight rare bytes at each of 29 places and, a
    chosen distance D behind each place, the bytes the place holds (for D < 8: the period D continued): a match at D, one D per distance
    code; the filler's runs are distance code 0.  Copies start where a 1 024-byte tile of the member starts, so that their source lies in a
    tile in front of theirs whatever D is."""
    a = bytearray()
    for k, L in enumerate(range(3, 259)):
        a += bytes([1 + k % 250]) * (L + 1)
    a += b"z" * (MAX_TEXT - len(a))
    b = bytearray(b"z" * MAX_TEXT)
    for c in range(1, 30):
        D, T = DISTANCE_OF_CODE[c], 1024 * (33 + c)
        src = rng.integers(130, 250, 8, dtype=np.uint8).tobytes()
        m = min(D, 8)
        b[T - D:T - D + m] = src[:m]
        for i in range(8):
            b[T + i] = b[T + i - D]
    return bytes(a) + bytes(b)


def distance_code(d):
    x = d - 1
    if x < 4:
        return x
    e = x.bit_length() - 2
    return 2 * e + 2 + ((x >> e) & 1)


def edge_texts():
    """name -> text, one member each (but `every_code`, whose members are checked together)."""
    rng = np.random.Generator(np.random.PCG64([223, SEED]))
    return {
        "one_byte_65280": b"Q" * MAX_TEXT,
        "all_256_values": bytes(range(256)) * 3,
        "no_repeated_trigram": no_repeated_trigram(rng, 4000, 97, 121),  # (24 letters: the literals alone make a dynamic block pay)
        "single_distance": single_distance(rng),
        "far_only": far_repeat(rng, (32769, 32770, 33000, 36000, 40000)),
        "far_at_32768": far_repeat(rng, (32768, 32769, 32767)),
        "every_code": every_length_and_distance_code(rng),
        "random": rng.integers(0, 256, MAX_TEXT, dtype=np.uint8).tobytes(),
    }


def deflate_host(lib, text, member_bytes=0, final=1, capacity=None, with_offsets=True, shift=0):
    """One faqcs_deflate_host into canary-filled buffers -> (rc, dict of the WHOLE buffers and info).  shift: the text starts that many bytes
    into its buffer."""
    text = bytes(text)
    mb = member_bytes or MAX_TEXT
    n = -(-len(text) // mb) + (1 if final else 0)
    cap = len(text) + 31 * n + 8 if capacity is None else capacity
    tb = np.zeros(shift + len(text) + 1, np.uint8)
    tb[shift:shift + len(text)] = np.frombuffer(text, np.uint8)
    comp = pc.aligned_bytes(FRONT + cap + 64)
    moff = np.full(n + 2, CAN32, np.uint32)
    info = capi.DeflateInfo(0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5)
    out = capi.DeflateOut(comp.ctypes.data + FRONT, cap, moff.ctypes.data if with_offsets else None, C.addressof(info))
    rc = lib.faqcs_deflate_host(tb.ctypes.data + shift if len(text) else None, len(text), member_bytes, final, C.byref(out))
    return rc, {"comp": comp, "member_offset": moff, "with_offsets": with_offsets, "cap": cap,
                "info": {f: int(getattr(info, f)) for f, _ in capi.DeflateInfo._fields_}}


def raw_stream(m):
    return m[18:len(m) - 8]


def parse_tokens(stream):
    """(lengths, distances) of the matches of ONE raw deflate stream, by a small decoder of its own (dynamic and fixed blocks)."""
    pos = [0]

    def bits(n):
        v = 0
        for i in range(n):
            v |= ((stream[pos[0] >> 3] >> (pos[0] & 7)) & 1) << i
            pos[0] += 1
        return v

    def table(lens):
        code, out = 0, {}
        for L in range(1, 16):
            for s, l in enumerate(lens):
                if l == L:
                    out[(L, code)] = s
                    code += 1
            code <<= 1
        return out

    def sym(tab):
        c = 0
        for L in range(1, 16):
            c = c << 1 | bits(1)
            if (L, c) in tab:
                return tab[(L, c)]
        raise AssertionError("no code")

    lens_out, dists_out = [], []
    while True:
        last, typ = bits(1), bits(2)
        if typ == 0:
            pos[0] = (pos[0] + 7) & ~7
            n = bits(16); bits(16)
            pos[0] += 8 * n
        else:
            if typ == 1:
                lit, dist = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 32)
            else:
                nl, nd, nc = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(nc):
                    cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = bits(3)
                ct, ls = table(cl), []
                while len(ls) < nl + nd:
                    s = sym(ct)
                    if s < 16: ls.append(s)
                    elif s == 16: ls += [ls[-1]] * (3 + bits(2))
                    elif s == 17: ls += [0] * (3 + bits(3))
                    else: ls += [0] * (11 + bits(7))
                lit, dist = table(ls[:nl]), table(ls[nl:])
            while True:
                s = sym(lit)
                if s == 256:
                    break
                if s > 256:
                    c = s - 257
                    L = 3 + c if c < 8 else 258 if c == 28 else 3 + ((4 + (c & 3)) << ((c >> 2) - 1)) + bits((c >> 2) - 1)
                    d = sym(dist)
                    D = 1 + d if d < 4 else 1 + ((2 + (d & 1)) << ((d >> 1) - 1)) + bits((d >> 1) - 1)
                    lens_out.append(L); dists_out.append(D)
        if last:
            return lens_out, dists_out


def assert_deflate(lib, o, text, member_bytes, final, round16=False, what="", per_member=True):
    """One deflate (deflate_host's dict, or the device's in the same form) against the rules: every member's header, stream, trailer; the
    whole by gzip; the member index and the text by the library's own inflate side; info in every field; canaries."""
    mb = member_bytes or MAX_TEXT
    n_data = -(-len(text) // mb)
    n = n_data + (1 if final else 0)
    info = o["info"]
    assert info["overflow"] == 0 and info["n_members"] == n and info["reserved"] == 0, "%s: %s" % (what, info)
    nb = info["n_bytes"]
    comp = bytes(o["comp"][FRONT:FRONT + nb])
    assert (o["comp"][:FRONT] == CANARY).all(), what + ": bytes in front of comp were written"
    r = (nb + 15) // 16 * 16 if round16 else nb
    assert (o["comp"][FRONT + r:] == CANARY).all(), what + ": bytes behind comp were written"
    # the members by their BSIZE chain
    ends, p, stored = [0], 0, 0
    while p < nb:
        assert comp[p:p + 16] == HEADER, "%s: header of the member at %d" % (what, p)
        size = struct.unpack_from("<H", comp, p + 16)[0] + 1
        k = len(ends) - 1
        if k < n_data:
            piece = text[k * mb:(k + 1) * mb]
            assert size <= len(piece) + 31, what
            if per_member:
                d = zlib.decompressobj(-15)
                got = d.decompress(comp[p + 18:p + size - 8]) + d.flush()
                assert got == piece and d.eof and not d.unused_data, "%s: member %d" % (what, k)
                assert struct.unpack_from("<II", comp, p + size - 8) == (zlib.crc32(piece) & 0xFFFFFFFF, len(piece)), what
            stored += (comp[p + 18] & 7) == 1
        else:
            assert comp[p:p + size] == ic.EOF_MEMBER and final and k == n_data, what
        p += size
        ends.append(p)
    assert p == nb and len(ends) == n + 1, what
    assert info["n_stored"] == stored, "%s: %s" % (what, info)
    assert gzip.decompress(comp) == text if nb else text == b"", what
    if o["with_offsets"]:
        assert (o["member_offset"][:n + 1] == ends).all() and o["member_offset"][n + 1] == CAN32, what
    else:
        assert (o["member_offset"] == CAN32).all(), what
    # the library's own index and inflate
    off = np.full(n + 3, CAN32, np.uint32)
    ii = capi.BgzfIndexInfo()
    cb = np.frombuffer(comp, np.uint8) if comp else np.zeros(1, np.uint8)
    assert lib.faqcs_bgzf_index_host(cb.ctypes.data if comp else None, nb, 1, off.ctypes.data, n + 1, C.byref(ii)) == 0
    assert (ii.n_members, ii.error, ii.overflow, ii.consumed) == (n, 0, 0, nb) and (off[:n + 1] == ends).all(), what
    rc, h = ic.inflate_host(lib, comp, np.array(ends, np.uint32), capacity=len(text))
    assert rc == 0, what
    ic.assert_inflate(h, [text[k * mb:(k + 1) * mb] for k in range(n_data)] + ([b""] if final else []), what=what)
    return comp, ends


def assert_nothing_written(o):
    assert (o["comp"] == CANARY).all() and (o["member_offset"] == CAN32).all()
