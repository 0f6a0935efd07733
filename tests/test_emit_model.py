"""CPU-side checks of the device emission (faqcs_emit_device): the numpy model the GPU tests use as their expected value agrees with the
library's own host statement of the byte edits (faqcs_apply_edits) read by read, and the entry point is there, declared as the header says,
and refuses a null context before it touches a device."""
import ctypes as C

import numpy as np
import pytest

from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    return capi.load_library()


@pytest.mark.parametrize("args", [[], ["--replace_to_N_q", "15"], ["--out_ascii", "64"], ["--ascii", "64", "--out_ascii", "33"]])
def test_emit_model_matches_apply_edits(lib, args):
    """200 random reads with N runs at their ends, random windows, random keep: the model's packed arenas are, read by read, what the C
    host function writes for the same window."""
    rng = np.random.default_rng(5)
    opt = parse_args(["-u", "x", "-d", "y"] + args)
    in_off = 64 if "--ascii" in args else 33
    h = capi.ParamsHolder(opt, 256, in_off)
    reads = []
    for _ in range(200):
        L = int(rng.integers(1, 60))
        s = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, L)].copy()
        if rng.random() < 0.3:
            s[: rng.integers(0, 4)] = ord("N")
        if rng.random() < 0.3:
            s[L - int(rng.integers(0, 4)):] = ord("N")
        q = (rng.integers(0, 42, L) + in_off).astype(np.uint8)
        reads.append((b"@r", s.tobytes(), q.tobytes()))
    seq, qual, offset, _ = driver.pack_segments([reads])
    n = len(reads)
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    lens = np.diff(offset.astype(np.int64))
    res["start"] = rng.integers(0, lens)
    res["len"] = rng.integers(0, lens - res["start"] + 1)
    res["flags"] = rng.integers(0, 2, n) | (rng.integers(0, 8, n) << 4)  # F_VALID at random, other bits are noise
    keep = (rng.random(n) < 0.7).astype(np.uint8)
    for kp in (None, keep):
        es, eq, eoff, eidx = driver.emit_model(opt, in_off, seq, qual, offset, res, kp)
        want = [i for i in range(n) if res["flags"][i] & 1 and (kp is None or kp[i])]
        assert 20 < len(want) < n and eidx.tolist() == want
        assert eoff.dtype == np.uint32 and eidx.dtype == np.uint32
        assert eoff[0] == 0 and len(eoff) == len(want) + 1 and len(es) == len(eq) == int(eoff[-1])
        for k, i in enumerate(want):
            a, ln = int(offset[i]), int(res["len"][i])
            os_, oq = np.zeros(ln + 1, np.uint8), np.zeros(ln + 1, np.uint8)
            rc = lib.faqcs_apply_edits(C.byref(h.p), seq[a:].ctypes.data, qual[a:].ctypes.data, int(lens[i]), res[i:].ctypes.data,
                                       os_.ctypes.data, oq.ctypes.data)
            assert rc == 0
            assert int(eoff[k + 1]) - int(eoff[k]) == ln
            assert (es[eoff[k]:eoff[k + 1]] == os_[:ln]).all(), (i, args)
            assert (eq[eoff[k]:eoff[k + 1]] == oq[:ln]).all(), (i, args)


def test_emit_model_of_nothing():
    opt = parse_args(["-u", "x", "-d", "y"])
    z = np.zeros(0, np.uint8)
    es, eq, eoff, eidx = driver.emit_model(opt, 33, z, z, np.zeros(1, np.uint32), np.zeros(0, dtype=capi.RESULT_DTYPE))
    assert len(es) == len(eq) == len(eidx) == 0 and eoff.tolist() == [0]
    seq, qual, offset, _ = driver.pack_segments([[(b"@r", b"ACGT", b"IIII")]])
    res = np.zeros(1, dtype=capi.RESULT_DTYPE)  # not valid
    es, eq, eoff, eidx = driver.emit_model(opt, 33, seq, qual, offset, res)
    assert len(es) == len(eq) == len(eidx) == 0 and eoff.tolist() == [0]


def test_emit_entry_point_is_declared_and_checks_its_arguments(lib):
    assert "faqcs_emit_device" in capi.declared_symbols()
    assert hasattr(lib, "faqcs_emit_device")
    assert C.sizeof(capi.EmitInfo) == 16
    assert C.sizeof(capi.EmitOut) == 48
    b = capi.Batch(None, None, None, 0, 0, None, 0, None)
    out = capi.EmitOut(None, None, 0, None, None, None)
    # a null context is refused at call time, before any device is touched (this machine may have none)
    assert lib.faqcs_emit_device(None, C.byref(b), None, None, C.byref(out)) == capi.E_INVAL
    assert b"null ctx" in lib.faqcs_last_error()
