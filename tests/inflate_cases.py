"""BGZF files built by hand for the inflate tests (faqcs_inflate_device / faqcs_inflate_host): header with the BC subfield, a raw deflate
stream from Python's zlib, CRC-32 and ISIZE.  No bgzip binary is needed, and the yardstick is always Python's zlib, never the code under
test."""
import ctypes as C
import struct
import zlib

import numpy as np

import parse_cases as pc
from faqcs_amd import _capi as capi

SEED = pc.SEED
CANARY, CAN32, FRONT = pc.CANARY, 0xA5A5A5A5, pc.FRONT
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")  # the 28-byte member bgzip ends a file with
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE, "filtered": zlib.Z_FILTERED}


def deflate_raw(text, level=6, strategy="default", mem_level=8, flush_at=()):
    """A raw deflate stream of `text`; flush_at: text positions behind which the stream is flushed with Z_FULL_FLUSH (an empty stored block,
    several blocks in the member)."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, STRATEGIES[strategy])
    out, a = [], 0
    for c in sorted(flush_at):
        out.append(co.compress(text[a:c]))
        out.append(co.flush(zlib.Z_FULL_FLUSH))
        a = c
    out.append(co.compress(text[a:]))
    out.append(co.flush())
    return b"".join(out)


def member(text, level=6, strategy="default", mem_level=8, flush_at=(), fname=None, extra_front=b"", fcomment=None, fhcrc=False, raw=None,
           crc=None, isize=None, with_bc=True):
    """One BGZF member of `text`.  raw: the deflate stream to use instead; crc / isize: trailer values to use instead; fname / fcomment /
    fhcrc: the optional gzip header parts; extra_front: subfields in front of BC; with_bc = False: the BC subfield carries another name."""
    data = deflate_raw(text, level, strategy, mem_level, flush_at) if raw is None else raw
    flg = 4 | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0)
    tail = b"" + (fname + b"\0" if fname is not None else b"") + (fcomment + b"\0" if fcomment is not None else b"")
    xlen = len(extra_front) + 6
    total = 12 + xlen + len(tail) + (2 if fhcrc else 0) + len(data) + 8
    assert total <= 65536, "the member does not fit BSIZE"
    extra = extra_front + (b"BC" if with_bc else b"XY") + struct.pack("<HH", 2, total - 1)
    head = struct.pack("<BBBBIBBH", 31, 139, 8, flg, 0, 0, 255, xlen) + extra + tail
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + data + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF if crc is None else crc, len(text) if isize is None else isize)


def first_block_type(m):
    """BTYPE of a member's first deflate block (0 stored, 1 fixed, 2 dynamic), parsed from its first header bits."""
    flg, xlen = m[3], struct.unpack_from("<H", m, 10)[0]
    q = 12 + xlen
    for bit in (8, 16):
        if flg & bit:
            q = m.index(b"\0", q) + 1
    if flg & 2:
        q += 2
    return (m[q] >> 1) & 3


def fastq_text(rng, n_bytes, read_len=150):
    """n_bytes of FASTQ-like text: records of parse_cases.make_text, the last one cut where the size says."""
    if n_bytes <= 0:
        return b""
    return pc.make_text(rng, np.full(n_bytes // (2 * read_len) + 1, read_len), p_empty_def=0.0)[:n_bytes]


def shape_text(rng, shape, n):
    """n bytes of one of the member shapes."""
    if shape == "fastq":
        return fastq_text(rng, n, int(rng.integers(20, 200)))
    if shape == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if shape == "repeat":       # distance-1 matches of 258
        return bytes([int(rng.integers(0, 256))]) * n
    if shape == "periodic":     # distance < length
        p = int(rng.integers(2, 12))
        unit = rng.integers(65, 91, p, dtype=np.uint8).tobytes()
        return (unit * (n // p + 1))[:n]
    raise ValueError(shape)


SHAPES = ("fastq", "random", "repeat", "periodic")
LEVELS = (0, 1, 6, 9)


def random_member(rng, max_text=65280):
    """(member bytes, text) of one member of a random shape, size, level, strategy and header variant that fits BSIZE."""
    shape = SHAPES[int(rng.integers(0, len(SHAPES)))]
    r = rng.random()
    n = int(rng.integers(0, 40)) if r < 0.15 else int(rng.integers(0, min(3000, max_text) + 1)) if r < 0.8 else int(rng.integers(min(3000, max_text), max_text + 1))
    level = LEVELS[int(rng.integers(0, 4))]
    strategy = list(STRATEGIES)[int(rng.integers(0, 5))] if rng.random() < 0.5 else "default"
    if shape == "random" or level == 0 or strategy in ("huffman", "fixed"):
        n = min(n, 48000)  # (incompressible or barely compressed: must still fit BSIZE; fixed codes of 9 bits: 48 000 x 9 / 8 = 54 000)
    text = shape_text(rng, shape, n)
    kw = {}
    v = int(rng.integers(0, 8))
    if v == 0:
        kw["fname"] = b"reads.fastq"
    elif v == 1:
        kw["extra_front"] = b"ZZ" + struct.pack("<H", 3) + b"abc"
    elif v == 2:
        kw["fcomment"], kw["fhcrc"] = b"made by hand", True
    if n > 4 and rng.random() < 0.25:
        kw["flush_at"] = sorted(set(rng.integers(0, n + 1, int(rng.integers(1, 4))).tolist()))
    return member(text, level, strategy, int(rng.integers(1, 10)), **kw), text


def edge_members(rng):
    """(member, text) of the sizes 0, 1, 65 280 and exactly 65 536 (the last compressible, so that the member fits BSIZE), the EOF member, one
    member per strategy, and one per level of every shape."""
    out = [(EOF_MEMBER, b""), (member(b"", 6), b""), (member(b"x", 6), b"x"), (member(b"x", 0), b"x")]
    t = shape_text(rng, "fastq", 65280)
    out.append((member(t, 6), t))
    t = shape_text(rng, "fastq", 65536)
    out.append((member(t, 1), t))
    t = shape_text(rng, "repeat", 65536)
    out.append((member(t, 9), t))
    t = shape_text(rng, "periodic", 65536)
    out.append((member(t, 6), t))
    for s in STRATEGIES:
        t = shape_text(rng, "fastq", 20000)
        out.append((member(t, 6, s), t))
    for shape in SHAPES:
        for lv in LEVELS:
            t = shape_text(rng, shape, 30000)
            out.append((member(t, lv), t))
    t = shape_text(rng, "fastq", 9000)
    out.append((member(t, 6, flush_at=(0, 3000, 3000, 9000)), t))
    out.append((member(t, 6, fname=b"a.fq", extra_front=b"AB" + struct.pack("<H", 0)), t))
    return out


def random_file(rng, n_members, max_text=65280):
    """([member bytes], [text]) of a file of n_members random members; now and then the EOF member in the middle."""
    ms, ts = [], []
    for _ in range(n_members):
        if rng.random() < 0.05:
            ms.append(EOF_MEMBER)
            ts.append(b"")
        else:
            m, t = random_member(rng, max_text)
            ms.append(m)
            ts.append(t)
    return ms, ts


def _fixed_code(sym):
    """(code, bits) of a literal/length symbol in the fixed Huffman code, MSB first."""
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + sym - 280, 8


def fixed_block_first_symbol_is_a_match():
    """A raw deflate stream: one final fixed-Huffman block whose first symbol is length 3, distance 1 -- a distance in front of the member --
    followed by the end-of-block code."""
    bits = [1, 1, 0]  # BFINAL = 1, BTYPE = 01 (LSB first)
    for sym in (257, None, 256):
        if sym is None:
            bits += [0, 0, 0, 0, 0]  # distance code 0 (5 bits, MSB first): distance 1
            continue
        code, n = _fixed_code(sym)
        bits += [(code >> (n - 1 - i)) & 1 for i in range(n)]
    bits += [0] * (-len(bits) % 8)
    return bytes(sum(b << i for i, b in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))


DAMAGE = ("crc", "isize_plus", "isize_minus", "isize_big", "no_bc", "btype3", "match_first", "bitflip")
DAMAGE_CODE = {"crc": capi.INFLATE_E_CRC, "isize_plus": capi.INFLATE_E_LENGTH, "isize_minus": capi.INFLATE_E_LENGTH, "isize_big": capi.INFLATE_E_LENGTH,
               "no_bc": capi.INFLATE_E_HEADER, "btype3": capi.INFLATE_E_DATA, "match_first": capi.INFLATE_E_DATA, "bitflip": None}  # None: some error, never OK


def damaged(rng, kind, text):
    """One member of `text` (FASTQ-like, a few thousand bytes) with exactly one thing wrong."""
    crc = zlib.crc32(text) & 0xFFFFFFFF
    if kind == "crc":
        return member(text, crc=crc ^ (1 << int(rng.integers(0, 32))))
    if kind == "isize_plus":
        return member(text, isize=len(text) + 1)
    if kind == "isize_minus":
        return member(text, isize=len(text) - 1)
    if kind == "isize_big":
        return member(text, isize=65537)
    if kind == "no_bc":
        return member(text, with_bc=False)
    if kind == "btype3":
        raw = bytearray(deflate_raw(text))
        raw[0] |= 6
        return member(text, raw=bytes(raw))
    if kind == "match_first":
        return member(b"aaa", raw=fixed_block_first_symbol_is_a_match())
    if kind == "bitflip":
        raw = bytearray(deflate_raw(text))
        while True:
            i, b = int(rng.integers(0, len(raw))), int(rng.integers(0, 8))
            raw[i] ^= 1 << b
            try:  # (a flip zlib does not notice and that leaves the text as it was -- unused header bits -- is no damage)
                d = zlib.decompressobj(-15)
                got = d.decompress(bytes(raw)) + d.flush()
                if got != text or not d.eof or d.unused_data:
                    break
            except zlib.error:
                break
            raw[i] ^= 1 << b
        return member(text, raw=bytes(raw))
    raise ValueError(kind)


def zlib_members(ms):
    """[text] of whole members by Python's zlib (raw inflate behind a header parsed here); raises on anything zlib refuses."""
    out = []
    for m in ms:
        flg, xlen = m[3], struct.unpack_from("<H", m, 10)[0]
        q = 12 + xlen
        for bit in (8, 16):
            if flg & bit:
                q = m.index(b"\0", q) + 1
        if flg & 2:
            q += 2
        d = zlib.decompressobj(-15)
        t = d.decompress(m[q:len(m) - 8]) + d.flush()
        assert d.eof and not d.unused_data
        assert struct.unpack_from("<II", m, len(m) - 8) == (zlib.crc32(t) & 0xFFFFFFFF, len(t))
        out.append(t)
    return out


def offsets_of(ms):
    return np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.uint32)


def inflate_host(lib, comp, moff, capacity=None, with_offsets=True):
    """One faqcs_inflate_host into canary-filled buffers -> (rc, dict of the WHOLE buffers and info)."""
    comp = bytes(comp)
    n = len(moff) - 1
    cap = 65536 * n + 8 if capacity is None else capacity
    cb = np.frombuffer(comp, dtype=np.uint8) if comp else np.zeros(1, np.uint8)
    moff = np.ascontiguousarray(moff, dtype=np.uint32)
    text = pc.aligned_bytes(FRONT + cap + 64)
    mto = np.full(n + 2, CAN32, np.uint32)
    info = capi.InflateInfo(0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5, -1, 0xA5A5A5A5)
    out = capi.InflateOut(text.ctypes.data + FRONT, cap, mto.ctypes.data if with_offsets else None, C.addressof(info))
    rc = lib.faqcs_inflate_host(cb.ctypes.data, len(comp), moff.ctypes.data, n, C.byref(out))
    return rc, {"text": text, "member_text_offset": mto, "with_offsets": with_offsets, "cap": cap,
                "info": {f: int(getattr(info, f)) for f, _ in capi.InflateInfo._fields_ if f != "reserved"}}


def assert_inflate(o, texts, bad=None, code=0, round16=False, what=""):
    """One inflate (inflate_host's dict, or the device's in the same form) against the members' texts by zlib.  bad: index of the member that
    is damaged (None: none), code: the error it must give (None: any but OK).  info field by field, the text in front of the bad member byte
    for byte, member_text_offset, canaries around every buffer."""
    good = texts if bad is None else texts[:bad]
    want_text = b"".join(good)
    info = o["info"]
    assert info["overflow"] == 0, what
    if bad is None:
        assert info == {"n_bytes": len(want_text), "n_members": len(texts), "overflow": 0, "error": 0}, "%s: %s" % (what, info)
    else:
        assert (info["n_bytes"], info["n_members"]) == (len(want_text), bad), "%s: %s" % (what, info)
        assert info["error"] == code if code is not None else info["error"] in range(1, 5), "%s: %s" % (what, info)
    got = bytes(o["text"][FRONT:FRONT + len(want_text)])
    if got != want_text:
        i = next(k for k in range(len(want_text)) if got[k] != want_text[k])
        raise AssertionError("%s: first differing byte %d of %d: got %r want %r" % (what, i, len(want_text), got[i:i + 12], want_text[i:i + 12]))
    if o["with_offsets"]:
        ends = np.concatenate([[0], np.cumsum([len(t) for t in good])])
        assert (o["member_text_offset"][:len(ends)] == ends).all(), what
        assert o["member_text_offset"][len(texts) + 1] == CAN32, what
    else:
        assert (o["member_text_offset"] == CAN32).all(), what
    assert (o["text"][:FRONT] == CANARY).all(), what + ": bytes in front of the text were written"
    if bad is None:
        r = (len(want_text) + 15) // 16 * 16 if round16 else len(want_text)
        assert (o["text"][FRONT + r:] == CANARY).all(), what + ": bytes behind the text were written"
    else:  # the device may have decoded members behind the bad one: nothing beyond the scanned total (at most every member's ISIZE)
        total = sum(len(t) for t in texts) + 65536
        lim = (total + 15) // 16 * 16 if round16 else len(want_text)
        assert (o["text"][FRONT + lim:] == CANARY).all(), what + ": bytes behind the text were written"


def assert_nothing_written(o):
    assert (o["text"] == CANARY).all() and (o["member_text_offset"] == CAN32).all()
