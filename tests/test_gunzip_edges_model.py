"""The catalogue of tests/gunzip_edges.py without a GPU: its coverage table and its mutants, its two plain models against ds.expand() and
zlib, the library's host statement (faqcs_gunzip_host / faqcs_gunzip_stream_host, built from the text the gfx950 kernels compile) on every
case at its piece sizes, the code of every refusal against zlib's verdict on the raw stream, and tools/gunzip_probe_check.cpp -- the probe
against the decoder on every block header the catalogues know, and every case through the host passes -- under AddressSanitizer and
UBSan.  What passes here is what tests/test_gpu_gunzip_edges.py sends to the device."""
import os
import re
import subprocess

import pytest

import deflate_streams as ds
import gunzip_cases as gc
import gunzip_edges as ge
import gunzip_stream_cases as gsc
from faqcs_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the invalid kinds whose fault stands in the dynamic header itself: the probe and the decoder must both refuse the block
HEADER_FAULTS = ("first_code_length_16", "repeat_overruns", "no_end_of_block", "lit_oversubscribed", "lit_incomplete", "dist_oversubscribed", "dist_incomplete",
                 "cl_oversubscribed", "cl_incomplete", "cl_single_one_bit", "hlit_too_large", "hdist_too_large")
# (of kind dist_incomplete, but its header is sound: a set of one 1-bit code; the fault is the symbol that uses the other bit)
FAULT_BEHIND_THE_HEADER = ("one_bit_distance_code_the_other_bit",)


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def test_the_constants_are_the_header_s():
    with open(os.path.join(ROOT, "faqcs_amd", "csrc", "faqcs_gunzip.h")) as f:
        hdr = f.read()
    for name, rx in ge.CONSTANT_SOURCES.items():
        m = re.search(rx, hdr)
        assert m, "%s: faqcs_gunzip.h no longer states it as %r" % (name, rx)
        assert getattr(ge, name) == int(m.group(1)) << int(m.group(2) or 0), name
    assert ge.WIN == capi.GUNZIP_WINDOW == gsc.WIN
    assert set(ge.allowed_codes()) == set(ds.INVALID_KINDS)


def test_every_edge_is_reached_and_every_claim_holds():
    cov, lost = ge.coverage()
    assert not lost, "claims the traces do not show: %s" % lost[:5]
    assert not [e for e, v in cov.items() if not v], "edges without a case"
    assert {c.family for c in ge.cases()} == set(ge.FAMILIES)
    assert all(set(c.pieces) <= set(gc.PIECES) and len(c.comp) < 1 << 20 for c in ge.cases())
    grid = {c.pieces[0]: c for c in ge.cases_of("piece start")}
    assert sum(len(t) for t in grid[1024].texts) <= 700000 and sum(len(t) for t in grid[4096].texts) <= 500000
    want = {"k %d" % k for k in ge.GRID_K} | {"len %d" % n for n in ge.GRID_LEN} | {"dist " + d for d in ge.GRID_DIST}
    assert all(want <= c.claims for c in grid.values())      # every k, every length and every class at both piece sizes
    n_feed = len(ge.cases_of("carried window")[0].feed[0])
    assert 36 <= n_feed <= 44


def test_every_mutant_is_caught():
    assert len(ge.MUTANTS) >= 9
    for m in ge.MUTANTS:
        by = ge.caught(m)
        assert by is not None, "no case tells the mutant %r (%s) from the models" % (m, ge.MUTANTS[m])
        print("%-24s caught by %r at %d: %s" % (m, by[0], by[1], by[2]))


def test_the_models_equal_expand_and_zlib():
    """sym_model's text of every member is ds.expand()'s and zlib's, its verdict zlib's; a case's own expectation is zlib's on the file"""
    for c in ge.cases():
        texts, error, consumed = gc.zlib_model(c.comp)
        assert tuple(texts) == c.texts and error == (c.bad is not None) and consumed == c.consumed, c.name
    for c in ge.model_cases():
        for piece in c.pieces:
            texts, bad, n, seen = ge.verdict(c, piece)
            assert bad == c.bad and tuple(texts) == c.texts, "%s at %d" % (c.name, piece)
            for (s, _), t in zip(c.members, texts):
                assert t == ds.expand(s.items), c.name
        if c.bad is not None:
            with pytest.raises(ValueError):
                ds.expand(c.members[c.bad][0].items)


def test_a_refusal_s_code_follows_zlib_s_verdict():
    """the codes a refused member may state, case by case from zlib's verdict on ITS raw stream and trailer (decompressobj(-15)), are the
    catalogue's table -- which is keyed by kind and never wider than the three rows of gunzip_edges.VERDICT_CODES"""
    assert ge.VERDICT_CODES == {"raises": (ge.E_DATA,), "length": (ge.E_LENGTH,), "crc": (ge.E_CRC,), "more": (ge.E_DATA, ge.E_TRUNCATED)}
    n = 0
    for c in ge.cases_of("invalid streams"):
        raw, trailer = c.comp[c.consumed + ge.HEAD:-8], c.comp[-8:]
        v = ge.zlib_verdict(raw, trailer)
        assert v != "ok" and c.codes == ge.VERDICT_CODES[v], "%s: zlib's verdict is %r, the table allows %s" % (c.name, v, c.codes)
        if c.name.startswith("invalid: "):
            kind = next(d.kind for d in ds.invalid_cases() if "invalid: " + d.name == c.name)
            assert c.codes == ge.allowed_codes()[kind], c.name
        n += 1
    assert n == 3 * len(ds.invalid_cases())      # plain, and behind a prefix of 1 025 and of 4 097 bytes
    for c in ge.model_cases():
        if c.bad is not None:
            (s, head) = c.members[c.bad]
            assert ge.zlib_verdict(s.getvalue(), c.comp[-8:]) == "raises" and c.codes == (ge.E_DATA,), c.name


@pytest.mark.parametrize("family", [f for f in ge.FAMILIES if f != "carried window"])
def test_host_statement_on_the_catalogue(lib, family):
    """every case at its piece sizes: gc.assert_case (text, members, consumed, nothing in front of the text), the code among the allowed,
    n_pieces the chain model's, exactly text[0 .. n_bytes) written"""
    seen = set()
    for c in ge.cases_of(family):
        for piece in c.pieces:
            what = "%s at %d" % (c.name, piece)
            rc, info, text = gc.gunzip_host(lib, c.comp, piece, ge.ROUNDS, ge.capacity(c))
            assert rc == 0, what
            ge.check_info(c, piece, info, text, what)
            assert (text[gc.FRONT + info["n_bytes"]:] == gc.CANARY).all(), what + ": bytes behind the text were written"
            seen.add(info["error"])
            if c.name == "a block end on a range end":
                assert info["n_pieces"] == ge.n_pieces_model(c, piece, "strictly behind") + 1, what   # (the host tells that mutant apart by the count)
    if family == "invalid streams":
        assert {ge.E_DATA, ge.E_LENGTH, ge.E_CRC} <= seen <= {ge.E_DATA, ge.E_LENGTH, ge.E_CRC, ge.E_TRUNCATED}, seen


def test_host_statement_on_the_feeds(lib):
    """the streamed cases through faqcs_gunzip_stream_host: gsc.feed / check_calls / check_stops, every call stopped at its cut"""
    for c in ge.cases_of("carried window"):
        for piece in c.pieces:
            ge.run_feed(gsc.host_call(lib), c, piece)


def corpus(path):
    """what the sanitizer program reads: the headers of the three catalogues with their positions, every whole-file case, every feed"""
    probes = []
    for c in ds.valid_cases():
        probes.append((0, ds.raw_stream(c)[0], gc.block_starts(c.stream)[0]))
    for c in ge.model_cases():
        for s, _ in c.members:
            probes.append((0, s.getvalue(), gc.block_starts(s)[0]))
    for mode, raw, positions in list(probes):      # the final blocks too, as if another followed: BFINAL cleared
        last = positions[-1]
        cleared = bytearray(raw)
        cleared[last >> 3] &= ~(1 << (last & 7)) & 255
        probes.append((mode, bytes(cleared), [last]))
    for c in ds.invalid_cases():
        raw = ds.raw_stream(c)[0]
        mode = 0 if c.kind in HEADER_FAULTS and c.name not in FAULT_BEHIND_THE_HEADER else 1
        probes += [(mode, raw, [0]), (mode, bytes([raw[0] & 254]) + raw[1:], [0])]
    files = [(piece, int(c.bad is not None), len(c.texts), b"".join(c.texts), c.comp) for c in ge.cases() if c.feed is None for piece in c.pieces]
    # every stream of deflate_streams.catalogue() alone in a gzip member, at the piece sizes the host and the device tests run them at
    files += [(piece, int(c.code is not None), int(c.code is None), c.text or b"", ge.catalogue_member(c)) for c in ds.catalogue() for piece in (1024, 65536)]
    # (a feed that ends with an error has delivered the blocks in front of its last one, the refused one, call by call)
    feeds = [(piece, int(c.bad is not None), b"".join(c.texts) if c.bad is None else ds.expand(c.members[0][0].items[:-1]), c.feed[0], c.comp)
             for c in ge.cases() if c.feed is not None for piece in c.pieces]
    ge.write_corpus(path, probes, files, feeds)
    return len(files), len(feeds)


def test_the_probe_and_the_decoder_under_the_sanitizers(tmp_path):
    """tools/gunzip_probe_check.cpp with AddressSanitizer and UBSan: at every known block header that reads non-final dynamic,
    plausible_block() is true exactly when gz_run decodes the block (the reverse allowed only where the catalogue puts the fault behind the
    header); every case and every feed through HostBackend with buffers of exactly the stated sizes.  Nothing is loaded into Python."""
    exe = str(tmp_path / "gunzip_probe_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "gunzip_probe_check.cpp")], capture_output=True, timeout=600)
    if r.returncode != 0 and b"asan" in r.stderr.lower():
        pytest.skip("no sanitizer runtime in this image")
    assert r.returncode == 0, r.stderr.decode()
    path = str(tmp_path / "corpus.bin")
    n_files, n_feeds = corpus(path)
    r = subprocess.run([exe, path], capture_output=True, timeout=900)
    out = (r.stdout + r.stderr).decode()
    print(out[-1500:])
    assert r.returncode == 0, out[-2000:]
    assert "%d files and %d feeds as zlib has them" % (n_files, n_feeds) in out
    m = re.search(r"(\d+) headers: (\d+) taken by both, (\d+) by neither", out)
    assert m and int(m.group(1)) >= 980 and int(m.group(2)) >= 900 and int(m.group(3)) >= 20, out
