"""The inflate rules of include/faqcs_mi.h (faqcs_inflate_device / faqcs_inflate_host / faqcs_bgzf_index_host) without a GPU: the library's
host statement -- built from the decoder text the gfx950 kernel compiles (csrc/faqcs_inflate.h) -- against Python's zlib on hand-built BGZF
files (inflate_cases.py), and that decoder text under AddressSanitizer and UBSan (tools/inflate_host_fuzz.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import inflate_cases as ic
import parse_cases as pc
from faqcs_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def test_the_decoder_core_under_the_sanitizers(tmp_path):
    """tools/inflate_host_fuzz.cpp: the shared decoder core as host C++ with AddressSanitizer and UBSan, buffers of exactly the stated sizes,
    generated and damaged streams against zlib: equal texts, equal verdicts, no access out of range.  (This is what stands between a
    damaged stream and the device: the GPU tests of damaged input check a refusal that has been proven here first.)"""
    exe = str(tmp_path / "inflate_host_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "inflate_host_fuzz.cpp"), "-lz"], capture_output=True, timeout=600)
    if r.returncode != 0 and b"asan" in r.stderr.lower():
        pytest.skip("no sanitizer runtime in this image")
    assert r.returncode == 0, r.stderr.decode()
    seed = os.environ.get("FAQCS_TEST_SEED", "20261017")
    r = subprocess.run([exe, seed, "250"], capture_output=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert b"250 members equal to zlib's" in r.stdout


def test_host_statement_equals_zlib(lib):
    """A few hundred seeded files of every member shape, level, strategy and header variant: text, member_text_offset and info field by
    field, canaries around every buffer; every block type came up as a member's first block."""
    rng = np.random.Generator(np.random.PCG64([101, ic.SEED]))
    edge = ic.edge_members(rng)
    files = [([m], [t]) for m, t in edge] + [([m for m, _ in edge], [t for _, t in edge]), ([], [])]
    for k in range(280):
        files.append(ic.random_file(rng, int(rng.integers(1, 9)), max_text=65280 if k % 8 == 0 else 6000))
    seen_types, n_members = set(), 0
    for k, (ms, ts) in enumerate(files):
        assert ic.zlib_members(ms) == ts
        rc, o = ic.inflate_host(lib, b"".join(ms), ic.offsets_of(ms), capacity=sum(len(t) for t in ts), with_offsets=(k % 3 != 0))
        assert rc == 0
        ic.assert_inflate(o, ts, what="file %d" % k)
        seen_types |= {ic.first_block_type(m) for m in ms}
        n_members += len(ms)
    assert len(files) >= 300 and n_members >= 1000
    assert seen_types == {0, 1, 2}, "stored, fixed and dynamic first blocks have to come up: %s" % sorted(seen_types)


@pytest.mark.parametrize("kind", ic.DAMAGE)
def test_damaged_members(lib, kind):
    """One change to one member in the middle of a file: the stated code, n_members = the member's index, the text in front byte-exact."""
    rng = np.random.Generator(np.random.PCG64([103, ic.DAMAGE.index(kind), ic.SEED]))
    seen = set()
    for rnd in range(12 if kind == "bitflip" else 3):
        ms, ts = ic.random_file(rng, 7, max_text=5000)
        bad = int(rng.integers(1, 6))
        text = ic.shape_text(rng, "fastq", int(rng.integers(2000, 6000)))
        ms[bad] = ic.damaged(rng, kind, text)
        ts[bad] = text
        if kind not in ("no_bc", "isize_big"):  # (the yardstick refuses it too)
            with pytest.raises(Exception):
                ic.zlib_members([ms[bad]])
        rc, o = ic.inflate_host(lib, b"".join(ms), ic.offsets_of(ms))
        assert rc == 0
        ic.assert_inflate(o, ts, bad=bad, code=ic.DAMAGE_CODE[kind], what="%s round %d" % (kind, rnd))
        seen.add(o["info"]["error"])
    assert 0 not in seen
    for code in range(1, 6):
        assert lib.faqcs_inflate_error_text(code).startswith(b"bgzf: ")
    assert lib.faqcs_inflate_error_text(0) == b"" and lib.faqcs_inflate_error_text(6) is None and lib.faqcs_inflate_error_text(-1) is None


def test_every_error_code_comes_up(lib):
    rng = np.random.Generator(np.random.PCG64([105, ic.SEED]))
    seen = set()
    text = ic.shape_text(rng, "fastq", 3000)
    for kind in ic.DAMAGE:
        m = ic.damaged(rng, kind, text)
        rc, o = ic.inflate_host(lib, m, ic.offsets_of([m]))
        assert rc == 0 and o["info"]["n_members"] == 0 and o["info"]["n_bytes"] == 0
        seen.add(o["info"]["error"])
    good = ic.member(text)
    info = capi.BgzfIndexInfo()
    off = np.zeros(4, np.uint32)
    cut = np.frombuffer(good[:-5], np.uint8)
    assert lib.faqcs_bgzf_index_host(cut.ctypes.data, len(cut), 1, off.ctypes.data, 3, C.byref(info)) == 0
    seen.add(info.error)
    assert seen == {capi.INFLATE_E_HEADER, capi.INFLATE_E_LENGTH, capi.INFLATE_E_DATA, capi.INFLATE_E_CRC, capi.INFLATE_E_TRUNCATED}


def test_offsets_that_do_not_describe_members(lib):
    """Member offsets that decrease, leave the input or cut a member in two are E_HEADER of that member; nothing is read outside comp."""
    rng = np.random.Generator(np.random.PCG64([106, ic.SEED]))
    ms, ts = ic.random_file(rng, 5, max_text=3000)
    comp, moff = b"".join(ms), ic.offsets_of(ms)
    for k, v in ((2, moff[3] + 1), (3, moff[2]), (5, len(comp) + 40), (4, moff[3] + 7)):
        mo = moff.copy()
        mo[k] = v
        rc, o = ic.inflate_host(lib, comp, mo)
        assert rc == 0 and (o["info"]["error"], o["info"]["n_members"]) == (capi.INFLATE_E_HEADER, k - 1), (k, o["info"])
        n = o["info"]["n_members"]
        assert bytes(o["text"][ic.FRONT:ic.FRONT + o["info"]["n_bytes"]]) == b"".join(ts[:n])


def test_overflow_on_the_host(lib):
    """A capacity one byte short: info states what is needed and nothing else is written; the exact size is enough."""
    rng = np.random.Generator(np.random.PCG64([107, ic.SEED]))
    ms, ts = ic.random_file(rng, 9, max_text=4000)
    nb = sum(len(t) for t in ts)
    rc, o = ic.inflate_host(lib, b"".join(ms), ic.offsets_of(ms), capacity=nb - 1)
    assert rc == 0 and o["info"] == {"n_bytes": nb, "n_members": 9, "overflow": 1, "error": 0}
    ic.assert_nothing_written(o)
    rc, o = ic.inflate_host(lib, b"".join(ms), ic.offsets_of(ms), capacity=nb)
    assert rc == 0
    ic.assert_inflate(o, ts)


def index_host(lib, comp, final, capacity=None):
    buf = np.frombuffer(bytes(comp), np.uint8) if len(comp) else np.zeros(1, np.uint8)
    cap = len(comp) // 26 + 1 if capacity is None else capacity
    off = np.full(cap + 2, ic.CAN32, np.uint32)
    info = capi.BgzfIndexInfo(0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5, -1, 0xA5A5A5A5)
    assert lib.faqcs_bgzf_index_host(buf.ctypes.data, len(comp), 1 if final else 0, off.ctypes.data, cap, C.byref(info)) == 0
    assert off[cap + 1] == ic.CAN32 and (info.overflow or (off[info.n_members + 1:] == ic.CAN32).all())
    return off, {"consumed": int(info.consumed), "n_members": int(info.n_members), "overflow": int(info.overflow), "error": int(info.error)}


def test_index_chunked_walk_equals_one_call(lib):
    """At EVERY cut of a small file: the members of [0, cut) with final = 0, then the rest from `consumed` with final = 1, are the one-call
    walk.  Also: a truncated last member, trailing bytes that are not gzip, a gzip header that is not BGZF, too few offsets."""
    rng = np.random.Generator(np.random.PCG64([109, ic.SEED]))
    ms, _ = ic.random_file(rng, 6, max_text=300)
    ms.append(ic.EOF_MEMBER)
    comp, want = b"".join(ms), ic.offsets_of(ms)
    off, info = index_host(lib, comp, True)
    assert info == {"consumed": len(comp), "n_members": len(ms), "overflow": 0, "error": 0} and (off[:len(ms) + 1] == want).all()
    for cut in range(len(comp) + 1):
        o1, i1 = index_host(lib, comp[:cut], False)
        assert i1["error"] == 0 and i1["consumed"] == want[i1["n_members"]] and i1["consumed"] <= cut
        assert i1["n_members"] == int(np.searchsorted(want, cut, side="right")) - 1
        o2, i2 = index_host(lib, comp[i1["consumed"]:], True)
        got = np.concatenate([o1[:i1["n_members"] + 1], o2[1:i2["n_members"] + 1] + i1["consumed"]])
        assert i2["error"] == 0 and (got == want).all(), cut
    for cut in range(1, len(ms[-1])):  # a truncated last member
        _, i = index_host(lib, comp[:len(comp) - cut], True)
        assert i == {"consumed": int(want[-2]), "n_members": len(ms) - 1, "overflow": 0, "error": capi.INFLATE_E_TRUNCATED}
    for junk in (b"\0", b"xyz", b"\x1f\x00", b"\n" * 40):  # trailing bytes that are not gzip end the data
        _, i = index_host(lib, comp + junk, True)
        assert i == {"consumed": len(comp) + len(junk), "n_members": len(ms), "overflow": 0, "error": 0}
    import gzip
    _, i = index_host(lib, comp + gzip.compress(b"ordinary gzip"), True)
    assert i == {"consumed": len(comp), "n_members": len(ms), "overflow": 0, "error": capi.INFLATE_E_HEADER}
    off, i = index_host(lib, comp, True, capacity=len(ms) - 1)
    assert i == {"consumed": len(comp), "n_members": len(ms), "overflow": 1, "error": 0} and (off == ic.CAN32).all()
    _, i = index_host(lib, b"", True)
    assert i == {"consumed": 0, "n_members": 0, "overflow": 0, "error": 0}


def test_chunked_inflate_and_parse_equal_the_one_call_parse(lib):
    """The loop of INTEGRATION.md section 3.2 on the host: members in chunks -> inflate -> parse final = 0 -> the unparsed tail in front of
    the next inflate's text -> ... final = 1 on the last chunk: the records are those of the one-call parse of the whole text."""
    rng = np.random.Generator(np.random.PCG64([113, ic.SEED]))
    for rnd in range(8):
        text = pc.make_text(rng, rng.integers(0, 300, 400), (b"\n", b"\r\n")[rnd % 2], ("clean", "clean_open")[rnd % 2 if rnd < 6 else 0])
        cuts = sorted(set(rng.integers(0, len(text), 14).tolist()) | {0, len(text)})
        ts = [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        ms = [ic.member(t, ic.LEVELS[int(rng.integers(0, 4))]) for t in ts]
        rc, whole = pc.parse_host(lib, text, True)
        assert rc == 0
        want = [(text[a:a + l], s, q, tn) for a, l, s, q, tn in pc.records_of(whole)]
        bounds = sorted(set(rng.integers(0, len(ms) + 1, 2).tolist()) | {0, len(ms)})
        tail, got = b"", []
        for a, b in zip(bounds[:-1], bounds[1:]):
            part = ms[a:b]
            rc, o = ic.inflate_host(lib, b"".join(part), ic.offsets_of(part))
            assert rc == 0 and o["info"]["error"] == 0
            chunk = tail + bytes(o["text"][ic.FRONT:ic.FRONT + o["info"]["n_bytes"]])
            rc, p = pc.parse_host(lib, chunk, b == len(ms))
            assert rc == 0 and p["info"]["error"] == 0
            got += [(chunk[x:x + l], s, q, tn) for x, l, s, q, tn in pc.records_of(p)]
            tail = chunk[p["info"]["consumed"]:]
        assert got == want, rnd


def test_declarations_and_argument_checks(lib):
    names = {"faqcs_inflate_device", "faqcs_inflate_host", "faqcs_inflate_time_ms", "faqcs_inflate_error_text", "faqcs_bgzf_index_host"}
    assert names <= set(capi.declared_symbols()) and names <= set(lib._faqcs_symbols)
    for nm in names:
        assert getattr(lib, nm) is not None
    assert C.sizeof(capi.InflateInfo) == 24 and C.sizeof(capi.BgzfIndexInfo) == 24 and lib.faqcs_abi_version() == 2
    m = ic.member(b"@a\nAC\n+\nII\n")
    comp, moff = np.frombuffer(m, np.uint8), np.array([0, len(m)], np.uint32)
    text, mto = pc.aligned_bytes(256), np.zeros(4, np.uint32)
    info = capi.InflateInfo()

    def out(**kw):
        f = dict(text=text.ctypes.data, capacity_bytes=64, member_text_offset=mto.ctypes.data, info=C.addressof(info))
        f.update(kw)
        return capi.InflateOut(**f)

    good = out()
    # a null context is refused before any device is touched (this test runs without one)
    assert lib.faqcs_inflate_device(None, comp.ctypes.data, len(m), moff.ctypes.data, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_inflate_time_ms(None, None, None) == capi.E_INVAL
    assert lib.faqcs_inflate_host(comp.ctypes.data, len(m), moff.ctypes.data, 1, C.byref(good)) == 0 and (info.n_members, info.n_bytes, info.error) == (1, 11, 0)
    assert lib.faqcs_inflate_host(comp.ctypes.data, 1 << 32, moff.ctypes.data, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_inflate_host(comp.ctypes.data, len(m), moff.ctypes.data, 3, C.byref(good)) == capi.E_INVAL  # more members than the bytes can hold
    assert lib.faqcs_inflate_host(comp.ctypes.data, len(m), moff.ctypes.data, 1, None) == capi.E_INVAL
    assert lib.faqcs_inflate_host(None, len(m), moff.ctypes.data, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_inflate_host(comp.ctypes.data, len(m), None, 1, C.byref(good)) == capi.E_INVAL
    for bad in (out(text=text.ctypes.data + 4), out(text=None), out(info=None)):
        assert lib.faqcs_inflate_host(comp.ctypes.data, len(m), moff.ctypes.data, 1, C.byref(bad)) == capi.E_INVAL
        assert lib.faqcs_last_error()
    assert lib.faqcs_inflate_host(comp.ctypes.data, len(m), moff.ctypes.data, 1, C.byref(out(member_text_offset=None))) == 0
    assert lib.faqcs_inflate_host(None, 0, None, 0, C.byref(good)) == 0 and (info.n_members, info.n_bytes, info.error, info.overflow) == (0, 0, 0, 0)
    ii = capi.BgzfIndexInfo()
    assert lib.faqcs_bgzf_index_host(comp.ctypes.data, 1 << 32, 1, mto.ctypes.data, 3, C.byref(ii)) == capi.E_INVAL
    assert lib.faqcs_bgzf_index_host(None, 5, 1, mto.ctypes.data, 3, C.byref(ii)) == capi.E_INVAL
    assert lib.faqcs_bgzf_index_host(comp.ctypes.data, len(m), 1, None, 3, C.byref(ii)) == capi.E_INVAL
    assert lib.faqcs_bgzf_index_host(comp.ctypes.data, len(m), 1, mto.ctypes.data, 3, None) == capi.E_INVAL
