"""The dense mode of the deflate rules (include/faqcs_mi.h at faqcs_deflate_device_mode) without a GPU: faqcs_deflate_host_mode -- built from
the encoder text the gfx950 kernel compiles (csrc/faqcs_deflate.h) -- against Python's zlib and gzip, the fast mode against the bytes it
produced before the dense mode existed, texts constructed for every rule of the dense match finder (deflate_dense_cases.py), and the dense
encoder text under AddressSanitizer and UBSan (tools/deflate_host_fuzz.cpp SEED N dense)."""
import ctypes as C
import hashlib
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import deflate_dense_cases as dd
import inflate_cases as ic
import parse_cases as pc
from faqcs_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_SHAPES = ("illumina",) + ic.SHAPES

# md5 and length of comp[0 .. n_bytes) of faqcs_deflate_host, taken from the library of the commit in front of the dense mode: the five texts
# of test_deflate_model.test_size_against_zlib (4 members, final = 0) and the texts of deflate_cases.edge_texts (final = 1)
FAST_DIGESTS = {
    "size:illumina": ("c5b85dd25fd0672d1319340d3e3c4052", 76360),
    "size:fastq": ("f3882fd3be9b873fef5aebdd6dc2f04e", 149276),
    "size:random": ("1cb02cbbd78b5a903bf151f62dca9cf3", 261244),
    "size:repeat": ("7e5c6389a98abdd781a7061af5b7b436", 420),
    "size:periodic": ("5f25ac54a7cbcffd85f2fb27a5b1fbdf", 3176),
    "edge:one_byte_65280": ("b3ab4a5e22d9d0cd322294438746dccd", 133),
    "edge:all_256_values": ("42eb15fac3ae08312d3899a4c0bfac2e", 827),
    "edge:no_repeated_trigram": ("311e288fd0044fdb9796d8fc8b048a53", 2417),
    "edge:single_distance": ("e6f8442647d4216390589b4bf116270a", 2176),
    "edge:far_only": ("c29afa62c43c1079342fbfccce3daf2c", 584),
    "edge:far_at_32768": ("ec677067ee85241601b907743b5229e5", 327),
    "edge:every_code": ("015c442474a8266f5dda6459dea27795", 1318),
    "edge:random": ("9dda915e91a3d2bdf0ede65fc82ed7f6", 65339),
}


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def size_text(shape):
    n = 4 * dc.MAX_TEXT
    return dc.illumina_text(n) if shape == "illumina" else ic.shape_text(np.random.Generator(np.random.PCG64([227, dc.SEED])), shape, n)


@pytest.fixture(scope="module")
def size_texts():
    return {shape: size_text(shape) for shape in SIZE_SHAPES}


def _digest(o):
    nb = o["info"]["n_bytes"]
    return hashlib.md5(bytes(o["comp"][dc.FRONT:dc.FRONT + nb])).hexdigest(), nb


def test_fast_is_untouched(lib, size_texts):
    """faqcs_deflate_host and faqcs_deflate_host_mode(FAST) give the bytes the library gave before it had a second mode."""
    cases = [("size:" + s, t, 0) for s, t in size_texts.items()] + [("edge:" + n, t, 1) for n, t in dc.edge_texts().items()]
    assert {c[0] for c in cases} == set(FAST_DIGESTS)
    for name, text, final in cases:
        rc, o = dc.deflate_host(lib, text, 0, final)
        assert rc == 0 and _digest(o) == FAST_DIGESTS[name], name
        rc, o = dd.deflate_host_mode(lib, text, 0, final, mode=dd.FAST)
        assert rc == 0 and _digest(o) == FAST_DIGESTS[name], name + " (by faqcs_deflate_host_mode)"


@pytest.mark.parametrize("shape", ic.SHAPES)
def test_format_and_round_trip(lib, shape):
    """The size grid in dense mode through deflate_cases.assert_deflate, which asks nothing of the match finder: every member's header, BSIZE,
    stream (zlib), CRC and ISIZE, text + 31, the whole by gzip, the library's own index and inflate, info in every field, canaries."""
    n_cases = 0
    for n, mb, final in dc.grid_cases(shape):
        text = dc.grid_text(shape, n)
        rc, o = dd.deflate_host_mode(lib, text, mb, final, with_offsets=(n_cases % 3 != 0))
        assert rc == 0
        dc.assert_deflate(lib, o, text, mb, final, what="%s n=%d mb=%d final=%d" % (shape, n, mb, final))
        n_cases += 1
    assert n_cases >= 170


def test_edge_content(lib):
    """deflate_cases.edge_texts in dense mode, with what holds for any correct encoder: lengths 3 .. 258, distances 1 .. 32 768, no match where
    no three bytes repeat, no source that is out of reach, random bytes stored."""
    for name, text in dc.edge_texts().items():
        rc, o = dd.deflate_host_mode(lib, text, 0, 1)
        assert rc == 0
        comp, ends = dc.assert_deflate(lib, o, text, 0, 1, what=name)
        toks = [dc.parse_tokens(dc.raw_stream(comp[a:b])) for a, b in zip(ends[:-2], ends[1:-1])]
        lens = [l for t in toks for l in t[0]]
        dists = [d for t in toks for d in t[1]]
        assert all(3 <= l <= 258 for l in lens) and all(1 <= d <= 32768 for d in dists), name
        if name == "one_byte_65280":
            assert set(dists) == {1} and o["info"]["n_bytes"] < 400
        elif name == "no_repeated_trigram":
            assert not lens and (comp[18] & 7) == 5
        elif name == "single_distance":
            assert set(dists) == {2048}
        elif name == "far_at_32768":
            far = {d: l for l, d in zip(lens, dists)}
            assert far.get(32768, 0) >= 40 and far.get(32767, 0) >= 40 and 32769 not in far, sorted(far)
        elif name == "far_only":
            assert not set(dists) & {32769, 32770, 33000, 36000, 40000} and max(dists) <= 32768
        elif name == "random":
            assert o["info"]["n_stored"] == 1 and o["info"]["n_bytes"] - 28 <= len(text) + 31


def test_dense_edges(lib):
    """One rule of the dense match finder each, on constructed texts (deflate_dense_cases.py), the matches read back from the stream: the
    sub-tile boundaries at 255 / 256 / 257 and 1 023 / 1 024 / 1 025, a source in the position's own sub-tile, the run there, the eight-byte
    table against a decoy in the three-byte table with 7, 8 and 9 bytes to the member's end, the lazy rule inside a tile, across two tiles,
    on a rising chain of three and on equal lengths, and two sources of equal length.

    On the tie: candidates (a) and (b) of one position cannot be DIFFERENT positions with matches of equal length.  A position that shares
    eight bytes with p shares three, so (a) is never farther back than a matching (b); and where (a) is nearer than (b) it is not in the
    eight-byte table under p's hash, so it shares fewer than eight bytes while (b) shares eight at least.  What a text can hold is two
    sources of equal length, both tables naming the nearer: that one is coded."""
    for name, (text, want) in dd.dense_edge_texts().items():
        rc, o = dd.deflate_host_mode(lib, text, 0, 1)
        assert rc == 0
        comp, ends = dc.assert_deflate(lib, o, text, 0, 1, what=name)
        assert len(ends) == 3 and (comp[18] & 7) == 5, name + ": one member, a dynamic block"
        got = dc.parse_tokens(dc.raw_stream(comp[ends[0]:ends[1]]))
        assert got == want, "%s: matches %s, the rule demands %s" % (name, got, want)
    # (the fast mode sees none of this: sub_tile_257's source lies in the copy's own tile)
    text, want = dd.dense_edge_texts()["sub_tile_257"]
    rc, o = dd.deflate_host_mode(lib, text, 0, 1, mode=dd.FAST)
    assert rc == 0 and dc.parse_tokens(dc.raw_stream(bytes(o["comp"][dc.FRONT:dc.FRONT + o["info"]["n_bytes"] - 28]))) == ([], [])


def test_the_farthest_distance_by_the_eight_byte_table(lib):
    """A source exactly 32 768 back that only candidate (b) names (the three-byte table holds a decoy) is taken whole; the one 32 769 back is
    refused by itself, and the position keeps the decoy's three bytes."""
    text, where = dd.far_by_eight(np.random.Generator(np.random.PCG64([241, dc.SEED])))
    rc, o = dd.deflate_host_mode(lib, text, 0, 1)
    assert rc == 0
    comp, ends = dc.assert_deflate(lib, o, text, 0, 1)
    lens, dists = dc.parse_tokens(dc.raw_stream(comp[ends[0]:ends[1]]))
    far = [(l, d) for l, d in zip(lens, dists) if d != 1]
    assert max(dists) == 32768 and [l for l, d in far if d == 32768] == [258], far  # (the filler behind source and copy agrees too)
    assert (3, 500) in far and 32769 not in dists, far


@pytest.mark.parametrize("mb", (1, 64, 259, 4096))
def test_short_texts_and_small_members(lib, mb):
    """Texts of 1 .. 9 bytes (no position has eight bytes in front of the end, or only the first has), and an Illumina-shaped text cut into
    small members."""
    rng = np.random.Generator(np.random.PCG64([251, dc.SEED, mb]))
    texts = [bytes(rng.integers(65, 69, n, dtype=np.uint8)) for n in range(1, 10)] + [b"A" * n for n in range(1, 10)]
    texts.append(dc.illumina_text(3 * 4096 + 77 if mb > 1 else 700, seed=11))
    for k, text in enumerate(texts):
        for final in (0, 1):
            rc, o = dd.deflate_host_mode(lib, text, mb, final, with_offsets=(k % 2 == 0))
            assert rc == 0
            dc.assert_deflate(lib, o, text, mb, final, what="text %d mb=%d final=%d" % (k, mb, final))


def _z(t, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
    return len(co.compress(t) + co.flush())


def test_size(lib, size_texts):
    """Conditions on the deterministic host bytes, 4 members of 65 280: dense <= fast on every shape, dense < fast on both FASTQ shapes, and
    there dense <= zlib level 3 over the same cut."""
    for shape, text in size_texts.items():
        got = {}
        for mode in (dd.FAST, dd.DENSE):
            rc, o = dd.deflate_host_mode(lib, text, 0, 0, mode=mode)
            assert rc == 0 and o["info"]["n_members"] == 4
            got[mode] = o["info"]["n_bytes"] - 4 * 26
        cut = [text[k * dc.MAX_TEXT:(k + 1) * dc.MAX_TEXT] for k in range(4)]
        z = {lv: sum(_z(c, lv) for c in cut) for lv in (1, 3, 4, 6)}
        print("%s: fast %d, dense %d, zlib level 1 %d, 3 %d, 4 %d, 6 %d" % (shape, got[dd.FAST], got[dd.DENSE], z[1], z[3], z[4], z[6]))
        assert got[dd.DENSE] <= got[dd.FAST], shape
        if shape in ("illumina", "fastq"):
            assert got[dd.DENSE] < got[dd.FAST] and got[dd.DENSE] <= z[3], shape


def test_determinism(lib):
    """The same call twice, and the text at 16 different offsets in its buffer: identical bytes."""
    text = dc.illumina_text(70000, seed=3)
    want = None
    for shift in [0] + list(range(16)):
        rc, o = dd.deflate_host_mode(lib, text, 0, 1, shift=shift)
        assert rc == 0
        got = (bytes(o["comp"]), o["member_offset"].tobytes(), o["info"])
        want = want or got
        assert got == want, shift


def test_arguments(lib):
    names = {"faqcs_deflate_device_mode", "faqcs_deflate_host_mode"}
    assert names <= set(capi.declared_symbols()) and names <= set(lib._faqcs_symbols) and lib.faqcs_abi_version() == 2
    assert (capi.DEFLATE_FAST, capi.DEFLATE_DENSE) == (0, 1)
    text = dc.illumina_text(9000, seed=5)
    for mode in (2, -1):
        rc, o = dd.deflate_host_mode(lib, text, 4096, 1, mode=mode)
        assert rc == capi.E_INVAL and lib.faqcs_last_error()
        dc.assert_nothing_written(o)
        assert o["info"]["n_bytes"] == 0xA5A5A5A5A5A5A5A5 and o["info"]["n_members"] == 0xA5A5A5A5
    rc, whole = dd.deflate_host_mode(lib, text, 4096, 1)
    assert rc == 0
    nb = whole["info"]["n_bytes"]
    rc, o = dd.deflate_host_mode(lib, text, 4096, 1, capacity=nb - 1)
    assert rc == 0 and o["info"] == {"n_bytes": nb, "n_members": 4, "overflow": 1, "n_stored": 0, "reserved": 0}
    dc.assert_nothing_written(o)
    tb = np.frombuffer(text, np.uint8)
    comp, info = pc.aligned_bytes(16384), capi.DeflateInfo()
    good = capi.DeflateOut(comp.ctypes.data, 16000, None, C.addressof(info))
    # a null context is refused before any device is touched (this test runs without one)
    assert lib.faqcs_deflate_device_mode(None, tb.ctypes.data, len(text), 0, 1, dd.DENSE, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_deflate_host_mode(tb.ctypes.data, len(text), 65281, 1, dd.DENSE, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_deflate_host_mode(tb.ctypes.data, len(text), 0, 1, dd.DENSE, None) == capi.E_INVAL
    # the Python form
    from faqcs_amd.engine import deflate_host

    comp_d, off_d, _ = deflate_host(text, 4096, True, lib=lib, mode=capi.DEFLATE_DENSE)
    comp_f, off_f, _ = deflate_host(text, 4096, True, lib=lib)
    assert comp_d == bytes(whole["comp"][dc.FRONT:dc.FRONT + nb]) and len(comp_d) < len(comp_f) and len(off_d) == len(off_f) == 5


def test_the_dense_encoder_core_under_the_sanitizers(tmp_path):
    """tools/deflate_host_fuzz.cpp SEED N dense: the dense instantiation of the shared encoder core as host C++ with AddressSanitizer and
    UBSan, buffers of exactly the stated sizes, generated texts of every shape and member size against zlib's inflate."""
    exe = str(tmp_path / "deflate_host_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "deflate_host_fuzz.cpp"), "-lz"], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    seed = os.environ.get("FAQCS_TEST_SEED", "20261017")
    r = subprocess.run([exe, seed, "400", "dense"], capture_output=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert b"400 texts came back through zlib" in r.stdout
    fast = subprocess.run([exe, seed, "40"], capture_output=True, timeout=900)
    dense = subprocess.run([exe, seed, "40", "dense"], capture_output=True, timeout=900)
    assert fast.returncode == 0 and dense.returncode == 0 and fast.stdout != dense.stdout, "the third argument chooses the dense match finder"
