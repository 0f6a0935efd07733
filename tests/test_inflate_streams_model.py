"""faqcs_inflate_host on deflate streams zlib's encoder never writes (deflate_streams.py: codes beyond the primary tables, the dynamic
header's corners, fixed-block symbols that must be refused, hundreds of blocks in a member, a grid of matches, and one defect at a time),
without a GPU.  The yardstick comes first: Python's zlib and the writer's own LZ77 expander have to agree on every case before the
library is asked; then the writer's coverage table is held to what the catalogue promises; then the host statement, alone and as the
middle member of a file; then the same members through the decoder text under AddressSanitizer and UBSan (tools/inflate_host_fuzz.cpp
--corpus); last, every stream once more as an ordinary gzip member through faqcs_gunzip_host, whose block decoder (gz_run) is a second text of the same rules.
tests/test_gpu_inflate_streams.py sends these very bytes to the device."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_streams as ds
import gunzip_cases as gc
import gunzip_edges as ge
import inflate_cases as ic
from faqcs_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.fixture(scope="module")
def good():
    """the two sound members a case stands between"""
    rng = np.random.Generator(np.random.PCG64([223, ic.SEED]))
    ts = [ic.fastq_text(rng, 3000, 100), ic.fastq_text(rng, 1777, 60)]
    return [ic.member(ts[0], 6), ic.member(ts[1], 1)], ts


def zlib_refusal(m):
    """how Python's zlib takes the member: None (accepted, trailer right), "error", "incomplete", "leftover" or "trailer\""""
    try:
        ic.zlib_members([m])
        return None
    except zlib.error:
        return "error"
    except AssertionError:
        pass
    q = 18  # (the members of inflate_cases.member() without optional parts)
    d = zlib.decompressobj(-15)
    t = d.decompress(m[q:len(m) - 8]) + d.flush()
    if not d.eof:
        return "incomplete"
    if d.unused_data:
        return "leftover"
    assert (zlib.crc32(t) & 0xFFFFFFFF, len(t)) != tuple(int.from_bytes(m[len(m) - 8 + 4 * i:len(m) - 4 + 4 * i], "little") for i in (0, 1))
    return "trailer"


def test_the_yardstick_agrees_with_the_declarations():
    """Every valid case inflates under zlib to the expander's text; every invalid one is refused by zlib in the way the case declares.  A
    case that zlib judges otherwise is a wrong case."""
    cases = ds.catalogue()
    assert 100 <= len(cases) <= 400
    for c in cases:
        assert (c.text is None) != (c.code is None), c.name
        assert len(c.member) <= 65536
        if c.code is None:
            assert len(c.text) <= 65536 and ic.zlib_members([c.member]) == [c.text], c.name
        else:
            assert c.refusal in ("error", "incomplete", "leftover", "trailer") and zlib_refusal(c.member) == c.refusal, c.name
    assert ds.catalogue() is cases  # built once
    rebuilt = ds.catalogue.__wrapped__()
    assert [(c.name, c.member, c.text, c.code) for c in rebuilt] == [(c.name, c.member, c.text, c.code) for c in cases], "the catalogue is a function of the seed"


def test_the_coverage_table():
    """What the writer recorded while it wrote the valid cases."""
    cov = ds.coverage()
    assert cov["code_lengths"]["lit"] >= set(range(1, 16)), "literal / length codes of every length, 11 .. 15 by the canonical walk"
    assert cov["code_lengths"]["dist"] >= set(range(1, 16)), "distance codes of every length, 9 .. 15 by the canonical walk"
    assert all(cov["ranks"]["lit"][l] >= 8 for l in range(11, 16)), "several codes of each length beyond the primary table: the walk has to rank them"
    assert all(cov["ranks"]["dist"][l] >= 2 for l in range(9, 16))
    assert 7 in cov["code_lengths"]["cl"]
    assert cov["first"] == {0, 1, 2} and cov["later"] == {0, 1, 2}
    assert max(cov["blocks"].values()) >= 500
    want = {(k, ln, d) for k in ds.GRID_K for ln in ds.GRID_LEN for d in ds.GRID_DIST}
    assert len(want) == 4 * 13 * 11 and cov["grid"] == want
    assert {257, 286} <= cov["hlit"] and {1, 30} <= cov["hdist"] and {5, 19} <= cov["hclen"]  # (HCLEN = 4 states no length but 0: an invalid case)
    assert cov["cross"] == {16, 17, 18}
    assert cov["invalid_kinds"] == set(ds.INVALID_KINDS)
    assert {c.code for c in ds.invalid_cases()} == {capi.INFLATE_E_DATA, capi.INFLATE_E_LENGTH}
    assert len(ds.grid_cases()) >= 10 and all(len(c.text) <= 65536 for c in ds.grid_cases())


def test_host_statement_on_every_valid_case(lib, good):
    gm, gt = good
    for c in ds.valid_cases():
        for ms, ts in (([c.member], [c.text]), ([gm[0], c.member, gm[1]], [gt[0], c.text, gt[1]])):
            rc, o = ic.inflate_host(lib, b"".join(ms), ic.offsets_of(ms), capacity=sum(len(t) for t in ts))
            assert rc == 0
            ic.assert_inflate(o, ts, what=c.name)
    ms, ts = [c.member for c in ds.valid_cases()], [c.text for c in ds.valid_cases()]
    rc, o = ic.inflate_host(lib, b"".join(ms), ic.offsets_of(ms), capacity=sum(len(t) for t in ts))
    assert rc == 0
    ic.assert_inflate(o, ts, what="all valid cases in one file")


def test_host_statement_on_every_invalid_case(lib, good):
    """The code include/faqcs_mi.h states for the defect, n_members = the case's index, the text in front of it byte-exact, canaries."""
    gm, gt = good
    for c in ds.invalid_cases():
        for bad, ms in ((0, [c.member]), (1, [gm[0], c.member, gm[1]])):
            ts = ([gt[0]] if bad else []) + [b""] + ([gt[1]] if bad else [])
            rc, o = ic.inflate_host(lib, b"".join(ms), ic.offsets_of(ms))
            assert rc == 0
            ic.assert_inflate(o, ts, bad=bad, code=c.code, what=c.name)


def test_the_catalogue_under_the_sanitizers(tmp_path):
    """tools/inflate_host_fuzz.cpp --corpus: every member of the catalogue through the decoder text the gfx950 kernel compiles, with
    AddressSanitizer and UBSan, input and output buffers of exactly the stated sizes, verdict and text against zlib.  Only what passed
    here goes to the device."""
    exe = str(tmp_path / "inflate_host_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "inflate_host_fuzz.cpp"), "-lz"], capture_output=True, timeout=600)
    if r.returncode != 0 and b"asan" in r.stderr.lower():
        pytest.skip("no sanitizer runtime in this image")
    assert r.returncode == 0, r.stderr.decode()
    cases = ds.catalogue()
    corpus = str(tmp_path / "catalogue.bin")
    ds.write_corpus(corpus, [c.member for c in cases])
    r = subprocess.run([exe, "--corpus", corpus], capture_output=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    want = "%d corpus members: %d accepted with zlib's text, %d refused as zlib refuses them" % (len(cases), len(ds.valid_cases()), len(ds.invalid_cases()))
    assert want.encode() in r.stdout, r.stdout.decode()[-500:]


@pytest.mark.parametrize("piece", (1024, 65536))
def test_the_catalogue_through_the_gzip_entry_point(lib, piece):
    """Every stream of the catalogue alone in one gzip member (gunzip_edges.catalogue_member) through faqcs_gunzip_host: a valid one gives
    its text, an invalid one is refused with the code of gunzip_edges.CATALOGUE_CODES -- one code per kind, among those zlib's verdict
    allows -- and nothing is delivered.  The same members pass tools/gunzip_probe_check.cpp under the sanitizers
    (tests/test_gunzip_edges_model.py), and tests/test_gpu_inflate_streams.py sends them to the device."""
    allowed = ge.allowed_codes()
    for c in ds.catalogue():
        m = ge.catalogue_member(c)
        rc, info, text = gc.gunzip_host(lib, m, piece, ge.ROUNDS, 65536)
        assert rc == 0, c.name
        if c.code is None:
            gc.assert_case(gc.Case(c.name, m, (c.text,), None, 0, len(m), (piece,), ge.ROUNDS, frozenset()), info, text, c.name)
            assert (text[gc.FRONT + len(c.text):] == gc.CANARY).all(), c.name + ": bytes behind the text were written"
        else:
            code = ge.catalogue_code(c.kind)
            assert code in allowed[c.kind], c.name
            assert (info["error"], info["n_members"], info["n_bytes"], info["overflow"]) == (code, 0, 0, 0), "%s (%s): %s" % (c.name, c.kind, info)
            assert (text[:gc.FRONT] == gc.CANARY).all(), c.name + ": bytes in front of the text were written"
