"""The deflate rules of include/faqcs_mi.h (faqcs_deflate_device / faqcs_deflate_host) without a GPU: the library's host statement -- built
from the encoder text the gfx950 kernel compiles (csrc/faqcs_deflate.h) -- against Python's zlib and gzip (deflate_cases.py), and that
encoder text under AddressSanitizer and UBSan (tools/deflate_host_fuzz.cpp)."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import inflate_cases as ic
import parse_cases as pc
from faqcs_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def test_the_encoder_core_under_the_sanitizers(tmp_path):
    """tools/deflate_host_fuzz.cpp: the shared encoder core as host C++ with AddressSanitizer and UBSan, buffers of exactly the stated sizes,
    generated texts of every shape and member size against zlib's inflate."""
    exe = str(tmp_path / "deflate_host_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "deflate_host_fuzz.cpp"), "-lz"], capture_output=True, timeout=600)
    if r.returncode != 0 and b"asan" in r.stderr.lower():
        pytest.skip("no sanitizer runtime in this image")
    assert r.returncode == 0, r.stderr.decode()
    seed = os.environ.get("FAQCS_TEST_SEED", "20261017")
    r = subprocess.run([exe, seed, "400"], capture_output=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert b"400 texts came back through zlib" in r.stdout


@pytest.mark.parametrize("shape", ic.SHAPES)
def test_format_and_round_trip(lib, shape):
    """The size grid: every member's header, stream and trailer by zlib, the whole by gzip, the index and the text by the library's own
    inflate side, info in every field, canaries around comp and member_offset."""
    n_cases = 0
    for n, mb, final in dc.grid_cases(shape):
        text = dc.grid_text(shape, n)
        rc, o = dc.deflate_host(lib, text, mb, final, with_offsets=(n_cases % 3 != 0))
        assert rc == 0
        dc.assert_deflate(lib, o, text, mb, final, what="%s n=%d mb=%d final=%d" % (shape, n, mb, final))
        n_cases += 1
    assert n_cases >= 170


def test_edge_content(lib):
    """One rule of the encoder each: the overlapping run, every byte value, no match at all, one distance code, candidates farther back
    than the format allows, the farthest distance, every length and distance code, incompressible text."""
    texts = dc.edge_texts()
    for name, text in texts.items():
        rc, o = dc.deflate_host(lib, text, 0, 1)
        assert rc == 0
        comp, ends = dc.assert_deflate(lib, o, text, 0, 1, what=name)
        toks = [dc.parse_tokens(dc.raw_stream(comp[a:b])) for a, b in zip(ends[:-2], ends[1:-1])]
        lens = [l for t in toks for l in t[0]]
        dists = [d for t in toks for d in t[1]]
        assert all(3 <= l <= 258 for l in lens) and all(1 <= d <= 32768 for d in dists), name
        if name == "one_byte_65280":
            assert set(dists) == {1} and lens.count(258) >= 250 and o["info"]["n_bytes"] < 400
        elif name == "no_repeated_trigram":
            assert not lens and (comp[18] & 7) == 5, "a dynamic block without a match"
        elif name == "single_distance":
            assert set(dists) == {2048} and (comp[18] & 7) == 5
        elif name == "far_at_32768":  # the sources 32 768 and 32 767 back are taken whole, the one 32 769 back is not
            far = {d: l for l, d in zip(lens, dists)}
            assert far.get(32768, 0) >= 40 and far.get(32767, 0) >= 40 and 32769 not in far and (comp[18] & 7) == 5, sorted(far)
        elif name == "far_only":      # every source is out of reach (the round trip above has shown that none was used)
            assert not set(dists) & {32769, 32770, 33000, 36000, 40000} and max(dists) <= 32768 and (comp[18] & 7) == 5
        elif name == "every_code":
            assert set(lens) >= set(range(3, 259)), sorted(set(range(3, 259)) - set(lens))
            assert {dc.distance_code(d) for d in dists} == set(range(30)), sorted(set(range(30)) - {dc.distance_code(d) for d in dists})
        elif name == "random":
            assert o["info"]["n_stored"] == 1 and o["info"]["n_bytes"] - 28 <= len(text) + 31


def _z(t, strategy=zlib.Z_DEFAULT_STRATEGY, level=1):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return len(co.compress(t) + co.flush())


@pytest.mark.parametrize("shape", ("illumina",) + ic.SHAPES)
def test_size_against_zlib(lib, shape):
    """The deflate streams of a file of 4 members against zlib's over the same cut: half-way between Huffman-only and level 1 where level 1
    gains something, half-way between fixed and Huffman-only codes where it does not, level 1 itself on random bytes."""
    n = 4 * dc.MAX_TEXT
    text = dc.illumina_text(n) if shape == "illumina" else ic.shape_text(np.random.Generator(np.random.PCG64([227, dc.SEED])), shape, n)
    rc, o = dc.deflate_host(lib, text, 0, 0)
    assert rc == 0 and o["info"]["n_members"] == 4
    ours = o["info"]["n_bytes"] - 4 * 26
    cut = [text[k * dc.MAX_TEXT:(k + 1) * dc.MAX_TEXT] for k in range(4)]
    z1, zh, zf, z6 = (sum(_z(c, s, lv) for c in cut) for s, lv in ((zlib.Z_DEFAULT_STRATEGY, 1), (zlib.Z_HUFFMAN_ONLY, 1), (zlib.Z_FIXED, 1), (zlib.Z_DEFAULT_STRATEGY, 6)))
    print("%s: ours %d, level 1 %d (ratio %.3f), level 6 %d (ratio %.3f), Huffman only %d, fixed %d" % (shape, ours, z1, ours / z1, z6, ours / z6, zh, zf))
    if shape in ("illumina", "repeat", "periodic"):
        assert ours <= (z1 + zh) / 2
    elif shape == "fastq":
        assert ours <= (zh + zf) / 2
    else:
        assert ours <= z1


def test_determinism(lib):
    """The same call twice, and the text at 16 different offsets in its buffer: identical bytes."""
    text = dc.illumina_text(70000, seed=3)
    want = None
    for shift in [0] + list(range(16)):
        rc, o = dc.deflate_host(lib, text, 0, 1, shift=shift)
        assert rc == 0
        got = (bytes(o["comp"]), o["member_offset"].tobytes(), o["info"])
        want = want or got
        assert got == want, shift


def test_overflow_and_arguments(lib):
    names = {"faqcs_deflate_device", "faqcs_deflate_host", "faqcs_deflate_time_ms"}
    assert names <= set(capi.declared_symbols()) and names <= set(lib._faqcs_symbols)
    assert C.sizeof(capi.DeflateInfo) == 24 and lib.faqcs_abi_version() == 2
    text = dc.illumina_text(9000, seed=5)
    rc, o = dc.deflate_host(lib, text, 4096, 1)
    assert rc == 0
    nb = o["info"]["n_bytes"]
    rc, o = dc.deflate_host(lib, text, 4096, 1, capacity=nb - 1)
    assert rc == 0 and o["info"] == {"n_bytes": nb, "n_members": 4, "overflow": 1, "n_stored": 0, "reserved": 0}
    dc.assert_nothing_written(o)
    rc, o = dc.deflate_host(lib, text, 4096, 1, capacity=nb)
    assert rc == 0
    dc.assert_deflate(lib, o, text, 4096, 1)
    tb = np.frombuffer(text, np.uint8)
    comp, moff = pc.aligned_bytes(16384), np.zeros(8, np.uint32)
    info = capi.DeflateInfo()

    def out(**kw):
        f = dict(comp=comp.ctypes.data, capacity_bytes=16000, member_offset=moff.ctypes.data, info=C.addressof(info))
        f.update(kw)
        return capi.DeflateOut(**f)

    good = out()
    # a null context is refused before any device is touched (this test runs without one)
    assert lib.faqcs_deflate_device(None, tb.ctypes.data, len(text), 0, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_deflate_time_ms(None, None, None) == capi.E_INVAL
    assert lib.faqcs_deflate_host(tb.ctypes.data, len(text), 0, 1, C.byref(good)) == 0 and info.n_members == 2
    assert lib.faqcs_deflate_host(tb.ctypes.data, 1 << 32, 0, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_deflate_host(tb.ctypes.data, len(text), 65281, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_deflate_host(tb.ctypes.data, len(text), 65280, 1, C.byref(good)) == 0
    assert lib.faqcs_deflate_host(tb.ctypes.data, (1 << 32) - 1, 1, 1, C.byref(good)) == capi.E_INVAL  # 2^32 members (refused before the text is read)
    assert lib.faqcs_deflate_host(None, len(text), 0, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_deflate_host(tb.ctypes.data, len(text), 0, 1, None) == capi.E_INVAL
    for bad in (out(comp=comp.ctypes.data + 4), out(comp=None), out(info=None)):
        assert lib.faqcs_deflate_host(tb.ctypes.data, len(text), 0, 1, C.byref(bad)) == capi.E_INVAL
        assert lib.faqcs_last_error()
    assert lib.faqcs_deflate_host(tb.ctypes.data, len(text), 0, 1, C.byref(out(member_offset=None))) == 0
    assert lib.faqcs_deflate_host(None, 0, 0, 0, C.byref(good)) == 0 and (info.n_members, info.n_bytes, info.overflow, info.n_stored) == (0, 0, 0, 0)
    assert lib.faqcs_deflate_host(None, 0, 0, 1, C.byref(good)) == 0 and (info.n_members, info.n_bytes) == (1, 28) and bytes(comp[:28]) == ic.EOF_MEMBER
