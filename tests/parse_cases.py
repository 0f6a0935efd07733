"""Shared by tests/test_parse_model.py (faqcs_parse_host, no GPU) and tests/test_gpu_parse.py (faqcs_parse_device): seeded FASTQ texts
that cover the parse rules of include/faqcs_mi.h, canary-filled output buffers, and the comparison of one parse with driver.parse_model."""
import ctypes as C
import os

import numpy as np

from faqcs_amd import _capi as capi
from faqcs_amd import driver

SEED = int(os.environ.get("FAQCS_TEST_SEED", "0"))  # re-seeds every random text, as in the other suites
CANARY = 0xA5
CAN32 = np.uint32(0xA5A5A5A5)
FRONT = 64  # canary bytes in front of the output arenas (keeps them 16-byte aligned)

TAILS = ("clean", "clean_open", "blank_line", "defline_only", "defline_open", "no_plus", "no_plus_open", "plus_open", "no_quality")
TAIL_ERROR = {"clean": capi.PARSE_OK, "clean_open": capi.PARSE_OK, "blank_line": capi.PARSE_E_SEQUENCE, "defline_only": capi.PARSE_E_SEQUENCE,
              "defline_open": capi.PARSE_E_SEQUENCE, "no_plus": capi.PARSE_E_PLUS, "no_plus_open": capi.PARSE_E_PLUS,
              "plus_open": capi.PARSE_E_PLUS_DELIM, "no_quality": capi.PARSE_E_QUALITY}

_BASES = np.frombuffer(b"ACGTN", np.uint8)


def _junk(rng, n):
    """Bytes that may stand between a '\\r' and the line's '\\n': anything but '\\n' ('\\r' included)."""
    return bytes(b for b in rng.integers(32, 127, n).tolist()) if rng.random() < 0.8 else b"\r" * n


def make_text(rng, lens, eol=b"\n", tail="clean", mismatch=(), p_quirk=0.0, p_empty_def=0.05, fixed_def=None):
    """One FASTQ text.  lens: base count per record; eol: b"\\n" or b"\\r\\n"; mismatch: record indices whose quality line is one byte off;
    p_quirk: per record, a lone '\\r' inside the base line, the quality line (either alone: a length mismatch unless both fall on the same
    position, which also happens) or the defline, and junk between a '\\r' and its '\\n'."""
    out = []
    n = len(lens)
    for k, L in enumerate(lens):
        L = int(L)
        if tail == "clean_open" and k == n - 1:
            L = max(L, 1)  # (an empty last quality line without '\n' is no line at all: that text ends behind its plus line)
        s = _BASES[rng.choice(5, L, p=[.24, .24, .24, .24, .04])].tobytes()
        q = (rng.integers(0, 42, L) + 33).astype(np.uint8).tobytes()
        d = fixed_def(k) if fixed_def else (b"" if rng.random() < p_empty_def else b"@r%d len=%d" % (k, L))
        p = b"+" if rng.random() < 0.8 else b"+" + d[1:]
        if k in mismatch:
            q = q + b"I" if (L == 0 or rng.random() < 0.5) else q[:-1]
        e = [eol, eol, eol, eol]
        if rng.random() < p_quirk:
            what = int(rng.integers(0, 6))
            at = int(rng.integers(0, L + 1))
            if what == 0:    # the same cut in both lines: a shorter, valid record
                s, q = s[:at] + b"\r" + s[at:], q[:at] + b"\r" + q[at:]
            elif what == 1:  # in the base line only
                s = s[:at] + b"\r" + s[at:]
            elif what == 2:  # in the quality line only
                q = q[:at] + b"\r" + q[at:]
            elif what == 3:  # in the defline
                c = int(rng.integers(0, len(d) + 1))
                d = d[:c] + b"\r" + d[c:]
            elif what == 4:  # junk between '\r' and '\n' of any of the four lines
                e[int(rng.integers(0, 4))] = b"\r" + _junk(rng, int(rng.integers(1, 40))) + b"\n"
            else:            # '\r' in the plus line
                p = p + b"\rxyz"
        out.append(d + e[0] + s + e[1] + p + e[2] + q + (b"" if (tail == "clean_open" and k == n - 1) else e[3]))
    out.append({"clean": b"", "clean_open": b"", "blank_line": eol, "defline_only": b"@tail" + eol, "defline_open": b"@tail", "no_plus": b"@tail" + eol + b"ACGT" + eol,
                "no_plus_open": b"@tail" + eol + b"ACGT", "plus_open": b"@tail" + eol + b"ACGT" + eol + b"+", "no_quality": b"@tail" + eol + b"ACGT" + eol + b"+" + eol}[tail])
    return b"".join(out)


def small_texts(rng, rounds=1):
    """(name, text) of texts of up to a few dozen records that cover, together: reads of 0 .. 400 bases, empty deflines, '\\r\\n' files, lone
    '\\r's, junk behind a '\\r', every tail shape, a length mismatch at the first, a middle and the last record."""
    yield "empty", b""
    yield "newline", b"\n"
    yield "cr", b"\r"
    yield "one_open", b"@a\nACGT\n+\nIIII"
    yield "one_cr_open", b"@a\r\nACGT\r\n+\r\nIIII\rjunk"
    yield "zero_bases", b"@a\n\n+\n\n" * 5
    for r in range(rounds):
        for eol in (b"\n", b"\r\n"):
            for tail in TAILS:
                for quirk in (0.0, 0.3):
                    n = int(rng.integers(0, 40))
                    lens = rng.integers(0, 401, n) if rng.random() < 0.7 else rng.integers(0, 4, n)
                    mm = ()
                    if n and rng.random() < 0.35:
                        mm = ({0}, {n // 2}, {n - 1}, {n // 2, n - 1})[int(rng.integers(0, 4))]
                    yield "r%d_%s_%s_q%d_n%d_mm%s" % (r, "crlf" if eol != b"\n" else "lf", tail, int(quirk * 10), n, sorted(mm)), make_text(rng, lens, eol, tail, mm, quirk)
    # the three mismatch positions, once each for certain
    for where, idx in (("first", 0), ("middle", 7), ("last", 14)):
        yield "mismatch_" + where, make_text(rng, rng.integers(0, 401, 15), b"\n", "clean", {idx})


def aligned_bytes(n, fill=CANARY):
    """uint8[n], 64-byte aligned."""
    raw = np.full(n + 64, fill, dtype=np.uint8)
    o = (-raw.ctypes.data) % 64
    return raw[o:o + n]


def parse_host(lib, text, final, cap_bytes=None, cap_reads=None, with_def=True):
    """One faqcs_parse_host into canary-filled buffers -> (rc, dict of the WHOLE buffers and info)."""
    text = bytes(text)
    cap_bytes = len(text) // 2 + 8 if cap_bytes is None else cap_bytes
    cap_reads = len(text) // 4 + 8 if cap_reads is None else cap_reads
    tb = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)
    seq = aligned_bytes(FRONT + cap_bytes + capi.ARENA_PAD_AFTER)
    qual = aligned_bytes(FRONT + cap_bytes + capi.ARENA_PAD_AFTER)
    off = np.full(cap_reads + 1, CAN32, np.uint32)
    tn = np.full(cap_reads + 1, CANARY, np.uint8)
    dpos = np.full(cap_reads + 1, CAN32, np.uint32)
    dlen = np.full(cap_reads + 1, CAN32, np.uint32)
    info = capi.ParseInfo(0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5, -1)
    out = capi.ParseOut(seq.ctypes.data + FRONT, qual.ctypes.data + FRONT, cap_bytes, cap_reads, off.ctypes.data, tn.ctypes.data,
                        dpos.ctypes.data if with_def else None, dlen.ctypes.data if with_def else None, C.addressof(info))
    rc = lib.faqcs_parse_host(tb.ctypes.data, len(text), 1 if final else 0, C.byref(out))
    return rc, {"seq": seq, "qual": qual, "offset": off, "terminal_n": tn, "def_pos": dpos, "def_len": dlen, "with_def": with_def,
                "info": {f: int(getattr(info, f)) for f, _ in capi.ParseInfo._fields_}, "cap_bytes": cap_bytes, "cap_reads": cap_reads}


def assert_untouched(o, nb, n, round16):
    """Canaries around every buffer: outside [0, nb) -- [0, nb rounded up to 16) for the device -- of the arenas, offset[n + 1 ..],
    terminal_n[n ..], def_*[n ..] (all of def_* when they were not given)."""
    r = (nb + 15) // 16 * 16 if round16 else nb
    for name in ("seq", "qual"):
        assert (o[name][:FRONT] == CANARY).all(), name + ": bytes in front of the arena were written"
        assert (o[name][FRONT + r:] == CANARY).all(), name + ": bytes behind the records were written"
    assert (o["offset"][n + 1:] == CAN32).all(), "offset[] behind the records was written"
    assert (o["terminal_n"][n:] == CANARY).all(), "terminal_n[] behind the records was written"
    for name in ("def_pos", "def_len"):
        assert (o[name][n if o["with_def"] else 0:] == CAN32).all(), name + "[] behind the records was written"


def assert_parse(o, text, final, round16, what="", model=None):
    """One parse (parse_host's dict, or the device's in the same form) against driver.parse_model, info field by field.  model: what
    driver.parse_model(text, final) returned, when the caller holds one text against several parses."""
    seq, qual, offset, tn, dpos, dlen, consumed, error = driver.parse_model(text, final) if model is None else model
    n, nb = len(offset) - 1, len(seq)
    lens = np.diff(offset.astype(np.int64))
    want = {"n_bytes": nb, "consumed": consumed, "n_reads": n, "max_read_len": int(lens.max()) if n else 0, "overflow": 0, "error": error}
    assert o["info"] == want, "%s: info %s, model %s" % (what, o["info"], want)
    assert (o["offset"][:n + 1] == offset).all(), what
    assert (o["terminal_n"][:n] == tn).all(), what
    if o["with_def"]:
        assert (o["def_pos"][:n] == dpos).all() and (o["def_len"][:n] == dlen).all(), what
    for name, w in (("seq", seq), ("qual", qual)):
        got = o[name][FRONT:FRONT + nb]
        bad = np.nonzero(got != w)[0]
        assert len(bad) == 0, "%s %s: first differing byte %d of %d (record %d): got %r want %r" % (
            what, name, bad[0], nb, int(np.searchsorted(offset, bad[0], side="right")) - 1, bytes(got[bad[0]:bad[0] + 8]), bytes(w[bad[0]:bad[0] + 8]))
    assert_untouched(o, nb, n, round16)
    return n, nb


def records_of(o):
    """[(defline position, defline length, bases, qualities, terminal_n)] of a parse's dict."""
    n = o["info"]["n_reads"]
    off = o["offset"]
    s, q = o["seq"][FRONT:], o["qual"][FRONT:]
    return [(int(o["def_pos"][k]), int(o["def_len"][k]), bytes(s[off[k]:off[k + 1]]), bytes(q[off[k]:off[k + 1]]), int(o["terminal_n"][k])) for k in range(n)]


def chunked(parse, text, cuts):
    """Feeds text[.. cuts[0]), then up to every further cut, with final = 0, each call starting where the last one's `consumed` ended, and the
    rest with final = 1.  parse(piece, final) -> dict.  -> (records with defline positions in `text`, consumed, error)"""
    start, recs = 0, []
    for c in list(cuts) + [None]:
        final = c is None
        end = len(text) if final else c
        if end < start:
            continue
        o = parse(text[start:end], final)
        assert o["info"]["overflow"] == 0
        recs += [(start + r[0],) + r[1:] for r in records_of(o)]
        start += o["info"]["consumed"]
        if o["info"]["error"]:
            return recs, start, o["info"]["error"]
    return recs, start, 0
