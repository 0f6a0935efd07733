"""The gunzip rules of include/faqcs_mi.h (faqcs_gunzip_device / faqcs_gunzip_host) without a GPU: the library's host statement -- built
from the text the gfx950 kernels compile (csrc/faqcs_gunzip.h) -- against Python's zlib on the catalogue of gunzip_cases.py, the condition
under which the default max_rounds stands, and that text under AddressSanitizer and UBSan (tools/gunzip_host_fuzz.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gunzip_cases as gc
from faqcs_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def test_the_three_symbols_are_there(lib):
    for nm in ("faqcs_gunzip_device", "faqcs_gunzip_host", "faqcs_gunzip_time_ms"):
        assert hasattr(lib, nm), nm
        assert nm in capi.declared_symbols()
    assert C.sizeof(capi.GunzipInfo) == 40 and lib.faqcs_abi_version() == 2
    assert lib.faqcs_inflate_error_text(capi.INFLATE_E_SERIAL).startswith(b"gzip: ")


def test_every_edge_is_reached():
    cov = gc.coverage()
    assert not [e for e, names in cov.items() if not names], "edges without a case"
    assert all(set(c.pieces) <= set(gc.PIECES) for c in gc.cases())
    assert all(100 << 10 <= len(t) <= 400 << 10 for t in gc.texts())


def test_the_catalogue_is_what_zlib_says():
    """a case's own expectation against the yardstick: the members zlib takes whole, whether it stops with an error, consumed"""
    for c in gc.cases():
        if c.code == gc.E_SERIAL:
            assert gc.zlib_model(c.comp)[1] is False, c.name   # (no property of the data: zlib reads it)
            continue
        texts, error, consumed = gc.zlib_model(c.comp)
        assert tuple(texts) == c.texts and error == (c.bad is not None) and consumed == c.consumed, c.name


@pytest.mark.parametrize("piece", gc.PIECES)
def test_host_statement_on_the_catalogue(lib, piece):
    """text, consumed, the member index and the error class of every case; exactly text[0 .. n_bytes) is written"""
    seen = set()
    for c in gc.cases():
        if piece not in c.pieces:
            continue
        cap = sum(len(t) for t in c.texts) + (0 if c.bad is None else 400000)
        rc, info, text = gc.gunzip_host(lib, c.comp, piece, c.max_rounds, cap)
        assert rc == 0, c.name
        gc.assert_case(c, info, text, "%s at %d" % (c.name, piece))
        assert (text[gc.FRONT + info["n_bytes"]:] == gc.CANARY).all(), c.name + ": bytes behind the text were written"
        seen.add(info["error"])
        if "false start" in c.edges and piece == 1024:
            assert info["n_fixups"] >= 1, info
        if "level 0" in c.edges and c.bad is None and piece == 1024:
            assert info["n_rounds"] >= 3 and info["n_fixups"] == info["n_rounds"] - 1, info   # every block behind the first is a forced start
        if "shorter than a piece" in c.edges:
            assert (info["n_pieces"], info["n_rounds"], info["n_fixups"]) == (1, 1, 0), info
        if "bgzip" in c.edges:
            assert info["n_rounds"] >= info["n_members"] - 1, info
    if piece == 1024:
        assert seen == {0, gc.E_HEADER, gc.E_LENGTH, gc.E_DATA, gc.E_CRC, gc.E_TRUNCATED, gc.E_SERIAL}


def test_overflow_on_the_host(lib):
    """capacity one byte short: info states what is needed and nothing else is written; the exact size is enough"""
    c = next(c for c in gc.cases() if c.name == "three members")
    nb = sum(len(t) for t in c.texts)
    for piece in gc.PIECES:
        rc, info, text = gc.gunzip_host(lib, c.comp, piece, 0, nb - 1)
        assert rc == 0 and (info["overflow"], info["n_bytes"], info["n_members"], info["error"], info["consumed"]) == (1, nb, 3, 0, len(c.comp)), info
        assert (text == gc.CANARY).all()
        rc, info, text = gc.gunzip_host(lib, c.comp, piece, 0, nb)
        assert rc == 0
        gc.assert_case(c, info, text, "exact capacity")


def test_the_default_max_rounds_stands_on_zlib_streams(lib):
    """The cap condition: zlib-written streams of levels 1 .. 9 of the catalogue's texts, at every piece size, need no more rounds than the
    default allows -- no E_SERIAL -- and the figure DESIGN.md section 4.8 states is the largest seen here."""
    worst = 0
    for t in gc.texts():
        for level in range(1, 10):
            comp = gc.gz_member(t, level)
            for piece in gc.PIECES:
                rc, info, text = gc.gunzip_host(lib, comp, piece, 0, len(t))
                assert rc == 0 and info["error"] == 0 and info["n_bytes"] == len(t), (level, piece, info)
                assert bytes(text[gc.FRONT:gc.FRONT + len(t)]) == t
                assert info["n_rounds"] <= capi.GUNZIP_DEFAULT_ROUNDS, (level, piece, info)
                worst = max(worst, info["n_rounds"])
    print("largest n_rounds on zlib streams of levels 1 .. 9: %d (default max_rounds %d)" % (worst, capi.GUNZIP_DEFAULT_ROUNDS))
    assert worst <= 8, "DESIGN.md section 4.8 states at most 8 rounds here"


def test_argument_checks(lib):
    c = next(c for c in gc.cases() if c.name == "shorter than one piece")
    comp = np.frombuffer(c.comp, np.uint8).copy()
    text = gc.ic.pc.aligned_bytes(1024)
    info = capi.GunzipInfo()

    def out(**kw):
        f = dict(text=text.ctypes.data, capacity_bytes=512, info=C.addressof(info))
        f.update(kw)
        return capi.GunzipOut(**f)

    good = out()
    assert lib.faqcs_gunzip_device(None, comp.ctypes.data, len(comp), 0, 0, C.byref(good)) == capi.E_INVAL   # before any device is touched
    assert lib.faqcs_gunzip_time_ms(None, None, None, None) == capi.E_INVAL
    assert lib.faqcs_gunzip_host(comp.ctypes.data, len(comp), 0, 0, C.byref(good)) == 0 and (info.n_members, info.n_bytes, info.error) == (1, 300, 0)
    assert lib.faqcs_gunzip_host(comp.ctypes.data, len(comp), 1024, 0, C.byref(good)) == 0
    assert lib.faqcs_gunzip_host(comp.ctypes.data, len(comp), 1023, 0, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_gunzip_host(comp.ctypes.data, 1 << 32, 0, 0, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_gunzip_host(None, len(comp), 0, 0, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_gunzip_host(comp.ctypes.data, len(comp), 0, 0, None) == capi.E_INVAL
    for bad in (out(text=text.ctypes.data + 4), out(text=None), out(info=None)):
        assert lib.faqcs_gunzip_host(comp.ctypes.data, len(comp), 0, 0, C.byref(bad)) == capi.E_INVAL
        assert lib.faqcs_last_error()
    assert lib.faqcs_gunzip_host(None, 0, 0, 0, C.byref(good)) == 0
    assert (info.n_members, info.n_bytes, info.error, info.overflow, info.consumed, info.n_rounds) == (0, 0, 0, 0, 0, 0)
    from faqcs_amd.engine import gunzip_host
    t, d = gunzip_host(c.comp, lib=lib)
    assert t == c.texts[0] and d["error"] == 0 and d["n_pieces"] == 1


def test_the_shared_text_under_the_sanitizers(tmp_path):
    """tools/gunzip_host_fuzz.cpp: the walk and the passes as host C++ with AddressSanitizer and UBSan, buffers of exactly the stated sizes,
    generated and damaged files against zlib: equal texts, an error exactly where zlib has one, no access out of range."""
    exe = str(tmp_path / "gunzip_host_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "gunzip_host_fuzz.cpp"), "-lz"], capture_output=True, timeout=600)
    if r.returncode != 0 and b"asan" in r.stderr.lower():
        pytest.skip("no sanitizer runtime in this image")
    assert r.returncode == 0, r.stderr.decode()
    seed = os.environ.get("FAQCS_TEST_SEED", "20261020")
    r = subprocess.run([exe, seed, "45"], capture_output=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert b"45 files equal to zlib's" in r.stdout
