"""The streamed gunzip of include/faqcs_mi.h (faqcs_gunzip_stream_host, the host statement of faqcs_gunzip_stream_device) without a GPU:
chunked feeds of gunzip_stream_cases.py against Python's zlib -- after every call the text so far, state.crc, the valid window, the
counters --, its equality with the single call, its argument checks, and the shared text under AddressSanitizer and UBSan
(tools/gunzip_stream_host_fuzz.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gunzip_cases as gc
import gunzip_stream_cases as gs
from faqcs_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.fixture(scope="module")
def call(lib):
    return gs.host_call(lib)


def test_the_symbols_and_the_struct(lib):
    for nm in ("faqcs_gunzip_stream_device", "faqcs_gunzip_stream_host"):
        assert hasattr(lib, nm), nm
        assert nm in capi.declared_symbols()
    assert C.sizeof(capi.GunzipState) == 56 and capi.GunzipState.window.offset == 48 and capi.GunzipState.phase.offset == 24
    assert (capi.GUNZIP_BETWEEN, capi.GUNZIP_STREAM, capi.GUNZIP_TRAILER, capi.GUNZIP_WINDOW) == (0, 1, 2, 32768)


def test_every_edge_is_reached(call):
    """every targeted feed at its piece sizes: each call against zlib, the feed's own expectation, and the table"""
    seen = set()
    for f in gs.feeds():
        for piece in f.pieces:
            seen |= gs.run_feed(call, f, piece)[0]
    seen |= gs.overflow_continued(call) | gs.isize_modulo(call)
    assert not gs.unreached(seen), "edges without a feed"


@pytest.mark.parametrize("piece", gc.PIECES)
def test_a_zeroed_state_and_final_is_the_single_call(lib, call, piece):
    """the whole catalogue of gunzip_cases.py: the same text, the same info field for field, exactly text[0 .. n_bytes) written"""
    for c in gc.cases():
        if piece not in c.pieces:
            continue
        cap = sum(len(t) for t in c.texts) + (0 if c.bad is None else 400000)
        rc1, info1, text1 = gc.gunzip_host(lib, c.comp, piece, c.max_rounds, cap)
        w, addr, _ = gs.host_window()
        st = gs.new_state(addr)
        rc2, info2, text2 = call(c.comp, True, st, w, piece, c.max_rounds, cap)
        assert (rc1, rc2) == (0, 0) and info1 == info2, "%s at %d: %s, streamed %s" % (c.name, piece, info1, info2)
        nb = info1["n_bytes"]
        assert (text1[:gc.FRONT + nb] == text2[:gc.FRONT + nb]).all() and (text2[gc.FRONT + nb:] == gc.CANARY).all(), c.name
        assert (st.total_bytes, st.total_comp, st.members) == (nb, info1["consumed"], info1["n_members"]) and st.phase == gs.BETWEEN, c.name


def _cut_feeds(c, ends_list, call, what):
    for piece in c.pieces:
        for ends in ends_list:
            calls = gs.feed(call, c.comp, ends, piece, c.max_rounds)
            gs.check_calls(c.comp, calls, "%s at %d, %s %s" % (c.name, piece, what, list(ends)[:4]), code=c.code)


def test_every_single_cut_of_the_small_files(call):
    """every file of at most 4 KiB, the hand-written members among them, cut in two at every byte"""
    small = [c for c in gc.cases() if 0 < len(c.comp) <= 4096]
    assert len(small) >= 4
    for c in small:
        _cut_feeds(c, [[cut] for cut in range(1, len(c.comp))], call, "cut")
    for name, s in gs.handmade().items():
        comp = gs._member_of(s) if name != "in front of the member" else None
        if comp is not None and len(comp) <= 4096:
            for cut in range(1, len(comp)):
                gs.check_calls(comp, gs.feed(call, comp, [cut], 1024, 64), "%s cut at %d" % (name, cut))


def _large():
    # (E_SERIAL is counted per call and is no property of the data: those two cases are the single call's)
    return [c for c in gc.cases() if len(c.comp) > 4096 and c.code != gc.E_SERIAL]


def test_a_seeded_sample_of_cuts_of_the_large_files(call):
    rng = np.random.Generator(np.random.PCG64([347, gc.SEED]))
    for c in _large():
        _cut_feeds(c, [[int(rng.integers(1, len(c.comp)))] for _ in range(3)], call, "cut")


def test_three_chunks_of_the_large_files(call):
    rng = np.random.Generator(np.random.PCG64([349, gc.SEED]))
    for c in _large():
        _cut_feeds(c, [sorted(int(v) for v in rng.integers(1, len(c.comp), 2))], call, "chunks")


def test_a_dribble_of_1500_bytes(call):
    """a fixed step of 1 500 bytes: most calls find no whole block and the chunk grows until one is there"""
    for c in _large():
        calls = gs.feed(call, c.comp, range(1500, len(c.comp), 1500), c.pieces[0], c.max_rounds)
        gs.check_calls(c.comp, calls, "%s, dribble" % c.name, code=c.code)


def test_argument_checks(lib):
    c = next(c for c in gc.cases() if c.name == "shorter than one piece")
    comp = np.frombuffer(c.comp, np.uint8).copy()
    text = gc.ic.pc.aligned_bytes(1024)
    info = capi.GunzipInfo()
    out = capi.GunzipOut(text.ctypes.data, 512, C.addressof(info))
    w, addr, _ = gs.host_window()

    def run(st, n=len(comp), final=1, piece=0, o=out, p=comp.ctypes.data):
        return lib.faqcs_gunzip_stream_host(p, n, final, piece, 0, C.byref(st) if st is not None else None, C.byref(o) if o is not None else None)

    def state(**kw):
        st = gs.new_state(addr)
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    assert lib.faqcs_gunzip_stream_device(None, comp.ctypes.data, len(comp), 1, 0, 0, C.byref(state()), C.byref(out)) == capi.E_INVAL   # before any device is touched
    st = state()
    assert run(st) == 0 and (info.n_members, info.n_bytes, info.error, st.members, st.total_comp) == (1, 300, 0, 1, len(comp))
    # everything the single call refuses
    assert run(state(), piece=1023) == capi.E_INVAL and run(state(), n=1 << 32) == capi.E_INVAL and run(state(), p=None) == capi.E_INVAL and run(state(), o=None) == capi.E_INVAL
    for bad in (capi.GunzipOut(text.ctypes.data + 4, 512, C.addressof(info)), capi.GunzipOut(None, 512, C.addressof(info)), capi.GunzipOut(text.ctypes.data, 512, None)):
        assert run(state(), o=bad) == capi.E_INVAL
    # and the state's own
    assert run(None) == capi.E_INVAL and run(state(window=None)) == capi.E_INVAL
    for kw in (dict(phase=3), dict(phase=1, bit=8), dict(phase=0, bit=1), dict(phase=2, bit=3), dict(phase=1, member_bytes=100, window_bytes=99),
               dict(phase=1, member_bytes=40000, window_bytes=40000), dict(phase=1, member_bytes=40000, window_bytes=100), dict(window_bytes=1), dict(reserved=1)):
        st = state(**kw)
        before = gs.state_dict(st)
        assert run(st) == capi.E_INVAL and lib.faqcs_last_error(), kw
        assert gs.state_dict(st) == before
    assert run(state(phase=1, member_bytes=40000, window_bytes=32768), n=0, final=0, p=None) == 0
    # nothing to read: zeros and the state as it is; final = 1 with a member open is E_TRUNCATED
    for phase in (gs.BETWEEN, gs.STREAM, gs.TRAILER):
        st = state(phase=phase, member_bytes=5, window_bytes=5, crc=77, bit=3 if phase == gs.STREAM else 0) if phase else state()
        before = gs.state_dict(st)
        assert run(st, n=0, final=0, p=None) == 0 and gs.state_dict(st) == before
        assert (info.n_members, info.n_bytes, info.error, info.overflow, info.consumed, info.n_rounds) == (0, 0, 0, 0, 0, 0)
        assert run(st, n=0, final=1, p=None) == 0 and gs.state_dict(st) == before
        assert info.error == (gc.E_TRUNCATED if phase else 0) and (info.n_members, info.n_bytes, info.consumed) == (0, 0, 0)
    from faqcs_amd.engine import gunzip_state, gunzip_stream_host
    st = gunzip_state(addr)
    t1, d1 = gunzip_stream_host(c.comp[:100], False, st, w, lib=lib)
    t2, d2 = gunzip_stream_host(c.comp[d1["consumed"]:], True, st, w, lib=lib)
    assert t1 + t2 == c.texts[0] and d2["error"] == 0 and st.members == 1


def test_the_shared_text_under_the_sanitizers(tmp_path):
    """tools/gunzip_stream_host_fuzz.cpp: the streamed walk and the passes as host C++ with AddressSanitizer and UBSan, buffers of exactly
    the stated sizes, generated and damaged files at random chunk ends against zlib: equal texts, the state's crc and window by their
    definitions, an error exactly where zlib has one, no access out of range."""
    exe = str(tmp_path / "gunzip_stream_host_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "gunzip_stream_host_fuzz.cpp"), "-lz"], capture_output=True, timeout=600)
    if r.returncode != 0 and b"asan" in r.stderr.lower():
        pytest.skip("no sanitizer runtime in this image")
    assert r.returncode == 0, r.stderr.decode()
    seed = os.environ.get("FAQCS_TEST_SEED", "20261020")
    r = subprocess.run([exe, seed, "30"], capture_output=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert b"30 files equal to zlib's" in r.stdout
