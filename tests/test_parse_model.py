"""The parse rules of include/faqcs_mi.h (faqcs_parse_device / faqcs_parse_host) without a GPU: the numpy model driver.parse_model against
the library's host statement faqcs_parse_host, both against the repository's older host parser (driver.FastqReader) and, where it is
built, against the real reference's messages."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parse_cases as pc
from faqcs_amd import _capi as capi
from faqcs_amd import driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF_BIN = os.path.join(ROOT, "oracle", "_ref", "FaQCs_ref")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def test_model_equals_host_statement(lib):
    """A few hundred seeded texts (parse_cases.small_texts: reads of 0 .. 400 bases, empty deflines, '\\r\\n' files, lone '\\r's in every
    line, junk behind a '\\r', all tail shapes, mismatches at the first / a middle / the last record), both values of `final`, with and
    without the defline arrays: every output array, info field by field, canaries around every buffer."""
    rng = np.random.Generator(np.random.PCG64([41, pc.SEED]))
    n_texts, seen_err, seen_cr = 0, set(), 0
    for name, text in pc.small_texts(rng, rounds=9):
        for final in (True, False):
            rc, o = pc.parse_host(lib, text, final, with_def=(n_texts % 3 != 0))
            assert rc == 0
            pc.assert_parse(o, text, final, round16=False, what="%s final=%d" % (name, final))
            seen_err.add(o["info"]["error"])
        seen_cr += b"\r" in text
        n_texts += 1
    assert n_texts >= 300 and seen_cr >= 100
    assert seen_err == set(range(6)), "every FAQCS_PARSE_* code has to come up: %s" % sorted(seen_err)


@pytest.mark.parametrize("tail", pc.TAILS)
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_tail_shapes(lib, tail, eol):
    """Every tail by name: the code the rules give it with final = 1, none with final = 0, and the records in front of it either way."""
    rng = np.random.Generator(np.random.PCG64([43, pc.TAILS.index(tail), len(eol), pc.SEED]))
    lens = rng.integers(0, 401, 9)
    text = pc.make_text(rng, lens, eol, tail)
    for final in (True, False):
        rc, o = pc.parse_host(lib, text, final)
        assert rc == 0
        pc.assert_parse(o, text, final, round16=False, what=tail)
        assert o["info"]["error"] == (pc.TAIL_ERROR[tail] if final else 0)
        assert o["info"]["n_reads"] == (9 if final or tail != "clean_open" else 8)
    for code in range(1, 6):
        assert lib.faqcs_parse_error_text(code).startswith(b"fastq.cpp:next_read: ")
    assert lib.faqcs_parse_error_text(0) == b"" and lib.faqcs_parse_error_text(6) is None and lib.faqcs_parse_error_text(-1) is None


def test_chunked_feed_equals_one_call(lib):
    """A text cut at arbitrary points -- inside a '\\r\\n' and right behind a '\\n' among them --, fed with final = 0 from where the last
    call's `consumed` ended, the rest with final = 1: the concatenation is the one-call parse."""
    rng = np.random.Generator(np.random.PCG64([47, pc.SEED]))
    parse = lambda piece, final: pc.parse_host(lib, piece, final)[1]
    for rnd in range(60):
        eol = (b"\n", b"\r\n")[rnd % 2]
        n = int(rng.integers(1, 60))
        mm = {int(rng.integers(0, n))} if rnd % 5 == 4 else ()
        text = pc.make_text(rng, rng.integers(0, 200, n), eol, pc.TAILS[rnd % len(pc.TAILS)], mm, 0.2 if rnd % 3 == 0 else 0.0)
        nls = [i for i in range(len(text)) if text[i:i + 1] == b"\n"]
        cuts = set(rng.integers(0, len(text) + 1, int(rng.integers(1, 12))).tolist())
        if nls:
            for i in rng.choice(nls, min(3, len(nls)), replace=False).tolist():
                cuts.add(i + 1)                # right behind a '\n'
                if eol == b"\r\n":
                    cuts.add(i)                # between the '\r' and the '\n'
        rc, whole = pc.parse_host(lib, text, True)
        assert rc == 0
        got = pc.chunked(parse, text, sorted(cuts))
        assert got == (pc.records_of(whole), whole["info"]["consumed"], whole["info"]["error"]), "round %d cuts %s" % (rnd, sorted(cuts))


def test_agrees_with_fastq_reader(lib, tmp_path):
    """Well-formed texts: the records equal what the driver's host parser (driver.FastqReader, fastq.cpp:8-125) returns for the same file."""
    rng = np.random.Generator(np.random.PCG64([53, pc.SEED]))
    for rnd, (eol, tail) in enumerate(((b"\n", "clean"), (b"\r\n", "clean"), (b"\n", "clean_open"), (b"\r\n", "clean_open"))):
        text = pc.make_text(rng, rng.integers(0, 401, 300), eol, tail, p_empty_def=0.0)
        p = tmp_path / ("t%d.fastq" % rnd)
        p.write_bytes(text)
        rd, want = driver.FastqReader(str(p), "x"), []
        while True:
            r = rd.next_read()
            if r is None:
                break
            want.append(r)
        rd.close()
        rc, o = pc.parse_host(lib, text, True)
        assert rc == 0 and o["info"]["error"] == 0
        got = [(text[a:a + l], s, q) for a, l, s, q, _ in pc.records_of(o)]
        assert got == want


_REF_CASES = {
    capi.PARSE_E_SEQUENCE: b"@tail\n",
    capi.PARSE_E_PLUS: b"@tail\nACGTACGTAC\n",
    capi.PARSE_E_PLUS_DELIM: b"@tail\nACGTACGTAC\n+",
    capi.PARSE_E_QUALITY: b"@tail\nACGTACGTAC\n+\n",
    capi.PARSE_E_LENGTH: b"@tail\nACGTACGTAC\n+\nIIIIIIIII\n",
}


@pytest.mark.parametrize("code", sorted(_REF_CASES))
def test_error_messages_are_the_references(lib, code, tmp_path):
    """The real reference on a small file per error code: exit code 1 and faqcs_parse_error_text(code) in its stderr, and the same code from
    the host statement.  One tail is left out: a last quality line without a newline, which this repository accepts by design
    (test_native_cli_mapped_path_equals_streaming_path) and next_read does not."""
    if not os.path.exists(_REF_BIN):
        pytest.skip("oracle/_ref/FaQCs_ref not built (needs the reference sources at build time: make -C oracle ref)")
    good = b"".join(b"@r%d\n" % i + b"ACGTTGCAAC" * 6 + b"\n+\n" + b"I" * 60 + b"\n" for i in range(5))
    text = good + _REF_CASES[code]
    rc, o = pc.parse_host(lib, text, True)
    assert rc == 0 and (o["info"]["error"], o["info"]["n_reads"]) == (code, 5)
    p = tmp_path / "in.fastq"
    p.write_bytes(text)
    r = subprocess.run([_REF_BIN, "-u", str(p), "-d", str(tmp_path / "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr.decode()[-400:])
    assert lib.faqcs_parse_error_text(code) in r.stderr, r.stderr.decode()[-400:]


def test_overflow_on_the_host(lib):
    """Too few bytes or too few reads: info states what is needed and nothing else is written; the exact sizes are enough."""
    rng = np.random.Generator(np.random.PCG64([59, pc.SEED]))
    text = pc.make_text(rng, rng.integers(1, 300, 50), b"\n", "clean")
    want = driver.parse_model(text, True)
    n, nb = len(want[2]) - 1, len(want[0])
    for cb, cr in ((nb - 1, n), (nb, n - 1)):
        rc, o = pc.parse_host(lib, text, True, cap_bytes=cb, cap_reads=cr)
        assert rc == 0
        assert o["info"] == {"n_bytes": nb, "consumed": len(text), "n_reads": n, "max_read_len": int(np.diff(want[2].astype(np.int64)).max()), "overflow": 1, "error": 0}
        assert (o["seq"] == pc.CANARY).all() and (o["qual"] == pc.CANARY).all() and (o["offset"] == pc.CAN32).all() and (o["terminal_n"] == pc.CANARY).all()
        assert (o["def_pos"] == pc.CAN32).all() and (o["def_len"] == pc.CAN32).all()
    rc, o = pc.parse_host(lib, text, True, cap_bytes=nb, cap_reads=n)
    assert rc == 0
    pc.assert_parse(o, text, True, round16=False)


def test_declarations_and_argument_checks(lib):
    names = {"faqcs_parse_device", "faqcs_parse_host", "faqcs_parse_time_ms", "faqcs_parse_error_text"}
    assert names <= set(capi.declared_symbols()) and names <= set(lib._faqcs_symbols)
    for nm in names:
        assert getattr(lib, nm) is not None
    assert C.sizeof(capi.ParseInfo) == 32
    text = np.frombuffer(b"@a\nAC\n+\nII\n", np.uint8)
    seq, qual = pc.aligned_bytes(256), pc.aligned_bytes(256)
    off, tn, dp, dl = np.zeros(8, np.uint32), np.zeros(8, np.uint8), np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    info = capi.ParseInfo()

    def out(**kw):
        f = dict(seq=seq.ctypes.data, qual=qual.ctypes.data, capacity_bytes=64, capacity_reads=4, offset=off.ctypes.data, terminal_n=tn.ctypes.data,
                 def_pos=dp.ctypes.data, def_len=dl.ctypes.data, info=C.addressof(info))
        f.update(kw)
        return capi.ParseOut(**f)

    good = out()
    # a null context is refused before any device is touched (this test runs without one)
    assert lib.faqcs_parse_device(None, text.ctypes.data, len(text), 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_parse_time_ms(None, None, None) == capi.E_INVAL
    assert lib.faqcs_parse_host(text.ctypes.data, len(text), 1, C.byref(good)) == 0 and info.n_reads == 1
    assert lib.faqcs_parse_host(text.ctypes.data, 1 << 32, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_parse_host(text.ctypes.data, len(text), 1, None) == capi.E_INVAL
    assert lib.faqcs_parse_host(None, len(text), 1, C.byref(good)) == capi.E_INVAL
    for bad in (out(seq=seq.ctypes.data + 4), out(qual=qual.ctypes.data + 8), out(def_pos=None), out(def_len=None), out(seq=None), out(qual=None),
                out(offset=None), out(terminal_n=None), out(info=None)):
        assert lib.faqcs_parse_host(text.ctypes.data, len(text), 1, C.byref(bad)) == capi.E_INVAL
        assert lib.faqcs_last_error()
    assert lib.faqcs_parse_host(text.ctypes.data, len(text), 1, C.byref(out(def_pos=None, def_len=None))) == 0
