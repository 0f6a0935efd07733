"""faqcs_gunzip_device on the MI355X: the catalogue of gunzip_cases.py against the host statement faqcs_gunzip_host -- the text byte for
byte and info field for field, n_pieces / n_fixups / n_rounds included, which holds the probe and the chain to the same decisions on both
sides -- and the chain gunzip -> parse against the parse of the plain text.  The damaged files that go to the device here are the ones
tests/test_gunzip_model.py has put through the host statement, and the same text through the sanitizers, first: they check a refusal."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import gunzip_cases as gc
from faqcs_amd import _capi as capi
from faqcs_amd.options import parse_args

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example_1.fastq.gz")


@pytest.fixture(scope="module")
def eng():
    from faqcs_amd.engine import HipEngine

    e = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    yield e
    e.close()


def gunzip_device(eng, comp, piece_bytes, max_rounds, capacity, shift=1):
    """One faqcs_gunzip_device into canary-filled device buffers -> (info dict, the WHOLE text buffer as a host array), the layout of
    gunzip_cases.gunzip_host.  shift: the compressed bytes start that many bytes behind a 256-byte aligned address."""
    import torch

    comp = bytes(comp)
    dev = torch.device("cuda:0")
    d_comp = torch.zeros(shift + len(comp) + 1, dtype=torch.uint8, device=dev)
    if comp:
        d_comp[shift:shift + len(comp)] = torch.from_numpy(np.frombuffer(comp, np.uint8).copy()).to(dev)
    text = torch.full((gc.FRONT + capacity + 64,), gc.CANARY, dtype=torch.uint8, device=dev)
    info = torch.full((5,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert (text.data_ptr() + gc.FRONT) % 16 == 0 and d_comp.data_ptr() % 256 == 0
    out = capi.GunzipOut(text.data_ptr() + gc.FRONT, capacity, info.data_ptr())
    eng.gunzip_device(d_comp.data_ptr() + shift if comp else None, len(comp), out, piece_bytes, max_rounds)   # (the call blocks)
    p = capi.GunzipInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    return gc.info_dict(p), text.cpu().numpy()


@pytest.mark.parametrize("piece", gc.PIECES)
def test_the_catalogue_equals_the_host_statement(eng, piece):
    """every case at this piece size: the text in front of the first bad member byte for byte, info field for field, canaries in front of
    the text and behind what the call may write (the capacity; without an error the text rounded up to 16)"""
    lib = eng.lib
    for k, c in enumerate(gc.cases()):
        if piece not in c.pieces:
            continue
        cap = sum(len(t) for t in c.texts) + (0 if c.bad is None else 400000)
        rc, h_info, h_text = gc.gunzip_host(lib, c.comp, piece, c.max_rounds, cap)
        assert rc == 0
        gc.assert_case(c, h_info, h_text, "host, %s at %d" % (c.name, piece))   # (first: the verdict is the host's before it is the device's)
        d_info, d_text = gunzip_device(eng, c.comp, piece, c.max_rounds, cap, shift=k % 7)
        what = "%s at %d" % (c.name, piece)
        assert d_info == h_info, "%s: device %s host %s" % (what, d_info, h_info)
        gc.assert_case(c, d_info, d_text, what)
        nb = d_info["n_bytes"]
        assert (d_text[gc.FRONT:gc.FRONT + nb] == h_text[gc.FRONT:gc.FRONT + nb]).all(), what
        behind = (nb + 15) // 16 * 16 if c.bad is None else cap
        assert (d_text[gc.FRONT + behind:] == gc.CANARY).all(), what + ": bytes behind the text were written"


def test_overflow_writes_nothing_but_info(eng):
    c = next(c for c in gc.cases() if c.name == "three members")
    nb = sum(len(t) for t in c.texts)
    for piece in (1024, 0):
        d_info, d_text = gunzip_device(eng, c.comp, piece, 0, nb - 1)
        rc, h_info, _ = gc.gunzip_host(eng.lib, c.comp, piece, 0, nb - 1)
        assert rc == 0 and d_info == h_info and (d_info["overflow"], d_info["n_bytes"], d_info["n_members"], d_info["error"]) == (1, nb, 3, 0)
        assert (d_text == gc.CANARY).all()


def test_every_alignment_of_the_compressed_bytes(eng):
    """d_comp at every residue mod 16: the probe's eight-byte loads and the bit reader's dwords start anywhere"""
    c = next(c for c in gc.cases() if c.name == "blocks against the ranges")
    nb = len(c.texts[0])
    rc, h_info, h_text = gc.gunzip_host(eng.lib, c.comp, 1024, c.max_rounds, nb)
    assert rc == 0
    for shift in range(16):
        d_info, d_text = gunzip_device(eng, c.comp, 1024, c.max_rounds, nb, shift=shift)
        assert d_info == h_info, shift
        assert (d_text == h_text).all(), shift


def test_time_ms_and_argument_checks(eng):
    c = next(c for c in gc.cases() if c.name == "level 6")
    d_info, _ = gunzip_device(eng, c.comp, 4096, 0, len(c.texts[0]))
    assert d_info["error"] == 0
    ms = eng.gunzip_time_ms()
    assert len(ms) == 3 and all(v >= 0.0 for v in ms) and ms[0] > 0.0 and ms[1] > 0.0
    lib = eng.lib
    import torch

    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    good = capi.GunzipOut(base + 1024, 512, base + 3072)
    assert lib.faqcs_gunzip_device(eng.ctx, base, 100, 1023, 0, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_gunzip_device(eng.ctx, base, 1 << 32, 0, 0, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_gunzip_device(eng.ctx, None, 100, 0, 0, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_gunzip_device(eng.ctx, base, 100, 0, 0, C.byref(capi.GunzipOut(base + 1028, 512, base + 3072))) == capi.E_INVAL
    assert lib.faqcs_gunzip_device(eng.ctx, base, 100, 0, 0, None) == capi.E_INVAL
    assert int(buf.sum()) == 0
    assert lib.faqcs_gunzip_device(eng.ctx, None, 0, 0, 0, C.byref(good)) == 0   # no bytes: zeros
    assert not buf.cpu().numpy()[3072:3112].any()


def test_gunzipped_text_feeds_the_parse(eng):
    """the golden FASTQ file, compressed with Python's gzip here (and as it is committed: gzip's own output): gunzipped_text -> parse_device
    equals the parse of the plain text in every array"""
    import torch

    from faqcs_amd.device import gunzipped_text
    from faqcs_amd.engine import FaqcsError
    from tools.parse_bench import parse_buffers, read_info

    with open(GOLDEN, "rb") as f:
        golden = f.read()
    text = gzip.decompress(golden)
    dev = torch.device("cuda:0")
    n_reads = text.count(b"\n") // 4

    def parse(d_text):
        pout, t = parse_buffers(dev, len(text), n_reads + 8)
        torch.cuda.synchronize()
        eng.parse_device(d_text.data_ptr(), len(text), True, pout)
        eng.sync()
        info = read_info(t["info"])
        assert info["error"] == 0 and info["overflow"] == 0 and info["n_reads"] == n_reads
        nb, n = info["n_bytes"], info["n_reads"]
        return info, [t["seq"][64:64 + nb].cpu().numpy(), t["qual"][64:64 + nb].cpu().numpy(), t["offset"][:n + 1].cpu().numpy(), t["terminal_n"][:n].cpu().numpy(),
                      t["def_pos"][:n].cpu().numpy(), t["def_len"][:n].cpu().numpy()]

    plain = torch.full((64 + len(text) + 64,), 10, dtype=torch.uint8, device=dev)
    plain[64:64 + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
    want_info, want = parse(plain[64:64 + len(text)])
    for comp, piece in ((gzip.compress(text, 6), 0), (gzip.compress(text, 9), 4096), (golden, 1024)):
        d_comp = torch.from_numpy(np.frombuffer(comp, np.uint8).copy()).to(dev)
        d_text = gunzipped_text(eng, d_comp, piece_bytes=piece)
        assert int(d_text.numel()) == len(text) and d_text.data_ptr() % 16 == 0
        assert bytes(d_text.cpu().numpy()) == text
        info, got = parse(d_text)
        assert info == want_info and all((a == b).all() for a, b in zip(got, want))
    # too little room at first: the call is repeated once with what info asks for
    d_text = gunzipped_text(eng, d_comp, capacity=1000)
    assert bytes(d_text.cpu().numpy()) == text
    bad = bytearray(golden)
    bad[-6] ^= 1
    with pytest.raises(FaqcsError, match="member 0: bgzf: the CRC-32"):
        gunzipped_text(eng, torch.from_numpy(np.frombuffer(bytes(bad), np.uint8).copy()).to(dev))
