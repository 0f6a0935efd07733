"""faqcs_bgzf_index_device on the MI355X: the catalogue of bgzf_index_cases.py against the host statement faqcs_bgzf_index_host, byte for
byte -- member_offset[0 .. n_members], every field of info, the entries behind them and the canaries around both --, the argument errors,
two calls without a sync between them, the chain into faqcs_inflate_device, the retry of device.bgzf_index and a randomised round.

The compressed bytes lie between two runs of whole 28-byte members in device memory: a kernel that read in front of d_comp or behind
d_comp + n_comp would find sound headers there, and answer differently from the host, which never sees them."""
import ctypes as C

import numpy as np
import pytest

import bgzf_index_cases as bc
import inflate_cases as ic
from faqcs_amd import _capi as capi
from faqcs_amd.options import parse_args

pytestmark = pytest.mark.gpu

GUARD = 64 * len(bc.EOF_MEMBER)  # bytes of sound members on either side of the data: a multiple of 16, so `shift` is the residue


@pytest.fixture(scope="module")
def eng():
    from faqcs_amd.engine import HipEngine

    e = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    yield e
    e.close()


class DeviceIndex:
    """The device buffers of one call: the data at residue `shift` mod 16 between its guards, capacity + 1 offsets between two canaries,
    info between two canaries."""

    def __init__(self, comp, capacity, shift=0):
        import torch

        dev = torch.device("cuda:0")
        guard = np.frombuffer(bc.EOF_MEMBER * 64, np.uint8)
        host = np.concatenate([np.zeros(shift, np.uint8), guard, np.frombuffer(bytes(comp), np.uint8), guard, np.zeros(16, np.uint8)])
        self.d_comp = torch.from_numpy(host.copy()).to(dev)
        self.n, self.capacity, self.at = len(comp), capacity, shift + GUARD
        self.moff = torch.from_numpy(np.full(capacity + 3, bc.CAN32, np.uint32).view(np.int32).copy()).to(dev)
        self.info = torch.full((5,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        assert self.d_comp.data_ptr() % 256 == 0 and self.moff.data_ptr() % 16 == 0

    def enqueue(self, eng, final):
        eng.bgzf_index_device(self.d_comp.data_ptr() + self.at if self.n else None, self.n, final, self.moff.data_ptr() + 4, self.capacity, self.info.data_ptr() + 8)

    def result(self):
        """-> (info dict, the whole offset array) in the form of bgzf_index_cases.index_host"""
        h = self.info.cpu().numpy()
        assert h[0] == -1 and h[4] == -1, "info's canaries"
        p = capi.BgzfIndexInfo.from_buffer_copy(h[1:4].tobytes())
        return {f: int(getattr(p, f)) for f, _ in capi.BgzfIndexInfo._fields_}, self.moff.cpu().numpy().view(np.uint32)


def check(eng, comp, final, capacity, shift=0, what=""):
    rc, h, off = bc.index_host(eng.lib, comp, final, capacity)
    assert rc == 0, "the host refuses an input of the test: a test bug (%s)" % what
    d = DeviceIndex(comp, capacity, shift)
    d.enqueue(eng, final)
    eng.sync()
    info, moff = d.result()
    assert info == h, (what, info, h)
    assert (moff == off).all(), (what, np.flatnonzero(moff != off)[:8])
    return info


def test_every_case_equals_the_host_statement(eng):
    for k, c in enumerate(bc.cases()):
        check(eng, c.comp, c.final, c.capacity, shift=k % 3, what=c.name)
    a, b = eng.bgzf_index_time_ms()
    assert a > 0 and b > 0


def test_every_residue_mod_16(eng):
    comp = bc.residue_case()
    for shift in range(16):
        for final in (0, 1):
            info = check(eng, comp, final, 64, shift=shift, what="residue %d final %d" % (shift, final))
            assert info["n_members"] == 43 and info["error"] == (capi.INFLATE_E_TRUNCATED if final else 0)


def test_overflow_writes_nothing_but_info(eng):
    seven = [c for c in bc.cases() if c.name.startswith("seven members")]
    assert len(seven) == 8
    for c in seven:
        d = DeviceIndex(c.comp, c.capacity)
        d.enqueue(eng, c.final)
        eng.sync()
        info, moff = d.result()
        assert info["n_members"] == 7 and info["overflow"] == (1 if c.capacity < 7 else 0), c.name
        if info["overflow"]:
            assert (moff == bc.CAN32).all(), c.name
        else:
            assert moff[0] == bc.CAN32 and moff[1] == 0 and (moff[9:] == bc.CAN32).all() and (np.diff(moff[1:9].astype(np.int64)) >= 26).all(), c.name


def test_argument_errors(eng):
    import torch

    lib = eng.lib
    buf = torch.zeros(4096, dtype=torch.uint8, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    base = buf.data_ptr()
    assert lib.faqcs_bgzf_index_device(eng.ctx, base, 1 << 32, 1, base + 1024, 8, base + 2048) == capi.E_INVAL
    assert lib.faqcs_bgzf_index_device(eng.ctx, None, 5, 1, base + 1024, 8, base + 2048) == capi.E_INVAL
    assert lib.faqcs_bgzf_index_device(eng.ctx, base, 100, 1, None, 8, base + 2048) == capi.E_INVAL
    assert lib.faqcs_bgzf_index_device(eng.ctx, base, 100, 1, base + 1024, 8, None) == capi.E_INVAL
    assert lib.faqcs_bgzf_index_device(None, base, 100, 1, base + 1024, 8, base + 2048) == capi.E_INVAL
    eng.sync()
    assert int(buf.sum()) == 0
    buf[2048:2072] = 0xFF
    torch.cuda.synchronize()
    assert lib.faqcs_bgzf_index_device(eng.ctx, None, 0, 1, base + 1024, 0, base + 2048) == 0  # no bytes: zeros, as the host says
    eng.sync()
    assert int(buf.sum()) == 0


def test_two_calls_without_a_sync_between_them(eng):
    """the second call reuses the scratch of the first, on the same stream: both answer as the host does, whichever order the sizes come in"""
    rng = np.random.Generator(np.random.PCG64([223, ic.SEED]))
    pool = [c for c in bc.cases() if 0 < len(c.comp) < 200_000]
    for rnd in range(12):
        pair = [pool[int(i)] for i in rng.integers(0, len(pool), 2)]
        if rnd % 3 == 0:
            pair[1] = pair[0]
        ds = [DeviceIndex(c.comp, c.capacity, shift=int(rng.integers(0, 16))) for c in pair]
        for d, c in zip(ds, pair):
            d.enqueue(eng, c.final)
        eng.sync()
        for d, c in zip(ds, pair):
            rc, h, off = bc.index_host(eng.lib, c.comp, c.final, c.capacity)
            info, moff = d.result()
            assert rc == 0 and info == h and (moff == off).all(), (rnd, c.name)


def test_device_offsets_feed_inflate(eng):
    """a small file of members zlib takes, an impostor in a stored block among them: faqcs_inflate_device fed the device-made offsets gives
    the text of inflated_text(index="host"), and inflated_text(index="device") is that call"""
    import torch

    from faqcs_amd.device import bgzf_index, inflated_text

    rng = np.random.Generator(np.random.PCG64([227, ic.SEED]))
    ms, ts = ic.random_file(rng, 9, max_text=6000)
    trap = bc.header(3000) + ic.shape_text(rng, "random", 900)
    ms.insert(4, ic.member(trap, 0))
    ts.insert(4, trap)
    ms.append(ic.EOF_MEMBER)
    comp = torch.from_numpy(np.frombuffer(b"".join(ms), np.uint8).copy()).to(torch.device("cuda:0"))
    assert bc.impostors(b"".join(ms))[0]
    want, want_off = inflated_text(eng, comp)
    assert bytes(want.cpu().numpy()) == b"".join(ts)
    moff, n, consumed, err = bgzf_index(eng, comp)
    assert (n, consumed, err) == (len(ms), int(comp.numel()), 0) and moff.is_cuda
    assert (moff.cpu().numpy().view(np.uint32) == ic.offsets_of(ms)).all()
    got, got_off = inflated_text(eng, comp, moff)
    assert torch.equal(got, want) and torch.equal(got_off, want_off)
    got, got_off = inflated_text(eng, comp, index="device")
    assert torch.equal(got, want) and torch.equal(got_off, want_off)


def test_bgzf_index_retries_with_the_reported_count(eng):
    import torch

    from faqcs_amd.device import bgzf_index

    comp = bc.EOF_MEMBER * 500 + bc.EOF_MEMBER[:20]
    d = torch.from_numpy(np.frombuffer(comp, np.uint8).copy()).to(torch.device("cuda:0"))
    want, consumed, err = eng.bgzf_index_host(comp, True)
    for cap in (None, 3, 499, 500, 0):  # (None: 64 members for these 14 020 bytes)
        moff, n, c, e = bgzf_index(eng, d, True, capacity=cap)
        assert (n, c, e) == (500, consumed, err) == (500, 14000, capi.INFLATE_E_TRUNCATED)
        assert (moff.cpu().numpy().view(np.uint32) == want).all()
    moff, n, c, e = bgzf_index(eng, d, False, capacity=2)
    assert (n, c, e) == (500, 14000, 0)
    moff, n, c, e = bgzf_index(eng, d[:0])
    assert (n, c, e) == (0, 0, 0) and moff.cpu().numpy().tolist() == [0]


def test_randomised_round(eng):
    """a few hundred concatenations of catalogue members and impostor payloads under a seed drawn here and printed"""
    seed = int(np.random.SeedSequence().entropy % (1 << 31))
    print("test_randomised_round: seed %d" % seed)
    rng = np.random.Generator(np.random.PCG64([229, seed]))
    for k in range(300):
        comp, final, cap = bc.random_input(rng)
        check(eng, comp, final, cap, shift=int(rng.integers(0, 16)), what="seed %d input %d" % (seed, k))
