"""CPU-side checks of the decisions around trim() (faqcs_detect_device / faqcs_first_error_device / faqcs_set_input_quality_offset): the host
statements (faqcs_detect_host, faqcs_first_error_host) against the numpy models (driver.detect_model, driver.first_error_model) on the
constructed catalogue (detect_cases.py), against the existing whole-buffer helpers on the golden fixtures, the argument checks, and the
statements under AddressSanitizer and UBSan as a stand-alone program (tools/detect_host_fuzz.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import detect_cases as dc
from faqcs_amd import _capi as capi
from faqcs_amd import driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    return capi.load_library()


def test_the_symbols_and_structs_are_declared(lib):
    for s in ("faqcs_detect_device", "faqcs_detect_host", "faqcs_first_error_device", "faqcs_first_error_host", "faqcs_set_input_quality_offset"):
        assert s in capi.declared_symbols() and hasattr(lib, s), s
    assert C.sizeof(capi.DetectInfo) == 24 and C.sizeof(capi.ErrorInfo) == 8
    assert lib.faqcs_abi_version() == 2
    assert (dc.T, dc.T_RESULTS) == (1024 * 16, 1024 * 2)


def test_the_catalogue_holds_what_it_claims():
    """The named placements are there, and the constructed expectations hold on the numpy model."""
    cases = dc.detect_cases()
    names = {c.name for c in cases}
    assert len(names) == len(cases)
    for where in ("0", "1", "15", "16", "17", "T-1", "T", "T+1", "last"):
        for kind in dc.KINDS:
            assert "single_%s_%s" % (where, kind) in names
    assert {int(c.offset[c.first]) for c in cases if c.name.startswith("head_")} == set(range(1, 16))
    assert sum(c.big for c in cases) == 3 and all(c.total > dc.FINISH_THREADS * dc.T for c in cases if c.big)
    for c in cases:
        m = c.model()
        for k, v in c.expect.items():
            assert m[k] == v, (c.name, k, m)
    ecases = dc.error_cases()
    assert sum(c.big for c in ecases) == 3 and all(c.n > dc.FINISH_THREADS * dc.T_RESULTS for c in ecases if c.big)
    for c in ecases:
        assert c.model() == c.expect, c.name


def test_detect_host_equals_the_model_on_every_case(lib):
    for c in dc.detect_cases():
        assert c.host(lib) == c.model(), c.name


def test_first_error_host_equals_the_model_on_every_case(lib):
    for c in dc.error_cases():
        assert c.host(lib) == c.model(), c.name


def test_the_engine_wrappers(lib):
    from faqcs_amd.engine import detect_host, first_error_host

    for c in dc.detect_cases()[::7]:
        if not c.big:
            assert detect_host(c.qual, c.offset, c.first, c.count, c.text, c.def_pos, c.def_len, lib=lib) == c.model(), c.name
    for c in dc.error_cases()[::3]:
        if not c.big:
            assert first_error_host(c.res, lib=lib) == c.model(), c.name


@pytest.mark.parametrize("fixture", ["adv", "adv64", "nextseq"])
def test_whole_buffers_equal_the_existing_helpers(lib, fixture, fixture_cache):
    """faqcs_detect_host over a whole buffer == faqcs_auto_detect_quality_offset == driver.auto_detect_quality_offset, and next_seq ==
    driver.auto_detect_next_seq, for both mates of the fixture; then the same buffer with every decisive byte replaced: undecided."""
    import golden_util
    import make_fixtures

    from faqcs_amd.engine import detect_host

    for path in golden_util.fixture_paths(fixture, fixture_cache):
        reads = make_fixtures.read_fastq(path)
        text = np.frombuffer(b"".join(d + b"\n" + s + b"\n+\n" + q + b"\n" for d, s, q in reads), np.uint8)
        seq, qual, offset, tn, dpos, dlen, consumed, error = driver.parse_model(text.tobytes(), True)
        n = len(reads)
        assert error == 0 and len(offset) - 1 == n
        offset = np.ascontiguousarray(offset, np.uint32)
        qual = np.ascontiguousarray(qual[:int(offset[-1])], np.uint8)
        d = detect_host(qual, offset, 0, n, text, dpos, dlen, lib=lib)
        assert d == driver.detect_model(qual, offset, 0, n, text, dpos, dlen)
        want = driver.auto_detect_quality_offset([r[2] for r in reads])
        assert d["quality_offset"] == want == lib.faqcs_auto_detect_quality_offset(qual.ctypes.data, offset.ctypes.data, n)
        assert want == (64 if fixture == "adv64" else 33)
        assert d["next_seq"] == int(driver.auto_detect_next_seq([r[0] for r in reads])) == int(fixture == "nextseq")
        assert bytes(reads[d["read"]][2][d["pos"]:d["pos"] + 1]) == bytes([d["byte"]])
        # the undecided buffer
        s8 = qual.view(np.int8)
        flat = np.where((s8 > 74) | (s8 < 59), np.uint8(ord("A")), qual).astype(np.uint8)
        d = detect_host(flat, offset, 0, n, lib=lib)
        assert d == dict(quality_offset=0, read=n, pos=0, byte=0, next_seq=0, reserved=0) == driver.detect_model(flat, offset, 0, n)
        assert lib.faqcs_auto_detect_quality_offset(flat.ctypes.data, offset.ctypes.data, n) == 0
        with pytest.raises(driver.FatalError):
            driver.auto_detect_quality_offset([bytes(flat[offset[i]:offset[i + 1]]) for i in range(n)])


def test_argument_checks(lib):
    E = capi.E_INVAL
    q = np.full(8, ord("A"), np.uint8)
    off = np.array([0, 4, 8], np.uint32)
    dp, dl = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    b = capi.Batch(None, q.ctypes.data, off.ctypes.data, 2, 0, None, 0, None)
    info = capi.DetectInfo()
    ia = C.addressof(info)
    H = lib.faqcs_detect_host
    assert H(C.byref(b), 0, 2, None, None, None, ia) == 0
    assert H(None, 0, 2, None, None, None, ia) == E and H(C.byref(b), 0, 2, None, None, None, None) == E
    assert H(C.byref(b), 0, 3, None, None, None, ia) == E and H(C.byref(b), 2, 1, None, None, None, ia) == E and H(C.byref(b), 3, 0, None, None, None, ia) == E
    assert H(C.byref(b), 0xFFFFFFFF, 2, None, None, None, ia) == E  # (first + count does not wrap)
    assert b"leaves the batch" in lib.faqcs_last_error()
    assert H(C.byref(b), 2, 0, None, None, None, ia) == 0 and (info.quality_offset, info.read) == (0, 2)
    t = q.ctypes.data
    for text, p, ln in ((t, None, None), (t, dp.ctypes.data, None), (t, None, dl.ctypes.data), (None, dp.ctypes.data, dl.ctypes.data), (None, dp.ctypes.data, None), (None, None, dl.ctypes.data)):
        assert H(C.byref(b), 0, 2, text, p, ln, ia) == E
    assert H(C.byref(b), 0, 2, t, dp.ctypes.data, dl.ctypes.data, ia) == 0
    for bad in (capi.Batch(None, None, off.ctypes.data, 2, 0, None, 0, None), capi.Batch(None, q.ctypes.data, None, 2, 0, None, 0, None)):
        assert H(C.byref(bad), 0, 2, None, None, None, ia) == E
        assert H(C.byref(bad), 1, 0, None, None, None, ia) == 0  # count == 0 reads nothing
    # the device forms refuse a null context at call time, before any device is touched
    assert lib.faqcs_detect_device(None, C.byref(b), 0, 2, None, None, None, ia) == E and b"null ctx" in lib.faqcs_last_error()
    einfo = capi.ErrorInfo()
    res = np.zeros(3, capi.RESULT_DTYPE)
    assert lib.faqcs_first_error_device(None, res.ctypes.data, 3, C.addressof(einfo)) == E
    assert lib.faqcs_set_input_quality_offset(None, 64) == E
    F = lib.faqcs_first_error_host
    assert F(res.ctypes.data, 3, C.addressof(einfo)) == 0 and (einfo.n_good, einfo.flags) == (3, 0)
    assert F(None, 3, C.addressof(einfo)) == E and F(res.ctypes.data, 3, None) == E
    assert F(None, 0, C.addressof(einfo)) == 0 and (einfo.n_good, einfo.flags) == (0, 0)


def test_detect_statements_under_the_sanitizers(tmp_path):
    """tools/detect_host_fuzz.cpp: the two host statements as a stand-alone program with AddressSanitizer and UBSan, random and adversarial
    inputs in buffers of exactly the stated sizes (the arena with its padding, decisive throughout), against a naive loop inside the
    program.  Nothing here is loaded into Python."""
    exe = str(tmp_path / "detect_host_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "detect_host_fuzz.cpp"), os.path.join(ROOT, "faqcs_amd", "csrc", "faqcs_host.cpp")],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run([exe, os.environ.get("FAQCS_TEST_SEED", "20261019"), "3000"], capture_output=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert r.stderr == b"", r.stderr.decode()[-2000:]
    assert b"3000 cases: ok" in r.stdout, r.stdout.decode()[-500:]
