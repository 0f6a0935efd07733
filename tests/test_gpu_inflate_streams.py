"""faqcs_inflate_device on the MI355X on the catalogue of deflate_streams.py: deflate streams zlib's encoder never writes -- codes beyond the
primary tables, the dynamic header's corners, hundreds of blocks in a member, and the grid of (literals waiting, match length, distance)
that the wave's Sink (WaveSink: the part of the decoder the host never runs) has to get right.  Every byte that goes to the device here
has been through the same decoder text on the host first, under the sanitizers, against zlib (tests/test_inflate_streams_model.py): the
invalid cases check a refusal that is the host's before it is the device's.  The same streams then go through faqcs_gunzip_device as ordinary
gzip members: gz_run states the same rules a second time, and the wave's Sink is the same text with 16-bit symbols."""
import numpy as np
import pytest

import deflate_streams as ds
import gunzip_cases as gc
import gunzip_edges as ge
import inflate_cases as ic
from test_gpu_gunzip import gunzip_device
from test_gpu_inflate import eng, inflate_device  # noqa: F401  (eng: the module's engine fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def good():
    """sound members of every text length modulo 16, to stand around a case"""
    rng = np.random.Generator(np.random.PCG64([227, ic.SEED]))
    text = ic.fastq_text(rng, 3000, 100)
    ts = [text[:2900 + r] for r in range(16)]
    return [ic.member(t, (1, 6)[r % 2]) for r, t in enumerate(ts)], ts


def run_both(eng, ms, ts, what, shift=1, bad=None, code=0):
    """the file on the host statement, then on the device: both against the texts, and the device's info against the host's"""
    comp, moff = b"".join(ms), ic.offsets_of(ms)
    cap = sum(len(t) for t in ts) if bad is None else None
    rc, h = ic.inflate_host(eng.lib, comp, moff, capacity=cap)
    assert rc == 0
    ic.assert_inflate(h, ts, bad=bad, code=code, what="host " + what)
    o = inflate_device(eng, comp, moff, capacity=cap, shift=shift)
    ic.assert_inflate(o, ts, bad=bad, code=code, round16=True, what=what)
    assert o["info"] == h["info"], what
    return o


def test_all_valid_cases_in_one_file(eng):
    """The text equals the expander's and zlib's, info equals faqcs_inflate_host's in every field, canaries hold."""
    cases = ds.valid_cases()
    ms, ts = [c.member for c in cases], [c.text for c in cases]
    assert ic.zlib_members(ms) == ts
    run_both(eng, ms, ts, "all valid cases")


def test_valid_cases_alone_name_the_case_that_fails(eng):
    """Each valid case outside the grid as a file of its own: a difference names the case."""
    for i, c in enumerate(c for c in ds.valid_cases() if c.kind != "grid"):
        run_both(eng, [c.member], [c.text], c.name, shift=i % 5)


def test_grid_members_alone_at_every_alignment(eng):
    """Each member of the (k, len, dist) grid alone, the compressed bytes 0 .. 4 bytes behind an aligned address."""
    grid = ds.grid_cases()
    assert len(grid) >= 10
    for i, c in enumerate(grid):
        assert ic.zlib_members([c.member]) == [c.text]
        run_both(eng, [c.member], [c.text], c.name, shift=i % 5)


def test_invalid_cases_are_refused_as_the_host_refuses_them(eng, good):
    """[good, case, good]: the host's code, n_members = 1, member 0's text byte-exact, nothing written beyond the scanned total, info equal to
    the host statement's.  Then [good, case] with the good member's length chosen so that the scanned total -- the good text and the case's
    ISIZE -- is a multiple of 16: not ONE byte behind the case's ISIZE is written, by a literal, a match or a stored block."""
    gm, gt = good
    for c in ds.invalid_cases():
        isize = int.from_bytes(c.member[-4:], "little")
        assert isize <= 65536
        ts = [gt[0], bytes(isize), gt[5]]
        o = run_both(eng, [gm[0], c.member, gm[5]], ts, c.name, bad=1, code=c.code)
        assert o["info"]["n_members"] == 1 and o["info"]["error"] == c.code
        total = sum(len(t) for t in ts)
        assert (o["text"][ic.FRONT + (total + 15) // 16 * 16:] == ic.CANARY).all(), c.name + ": bytes behind the scanned total were written"
        r = next(r for r in range(16) if (len(gt[r]) + isize) % 16 == 0)
        o = run_both(eng, [gm[r], c.member], [gt[r], bytes(isize)], c.name + " last", bad=1, code=c.code, shift=r % 5)
        assert (o["text"][ic.FRONT + len(gt[r]) + isize:] == ic.CANARY).all(), c.name + ": bytes behind the member's ISIZE were written"


def test_the_catalogue_through_the_gzip_entry_point(eng):
    """Every stream of the catalogue as a gzip member (gunzip_edges.catalogue_member) through faqcs_gunzip_device at pieces of 1 024 bytes:
    the valid ones as one file of many members, each invalid one alone.  Verdict, info and text are the host statement's, which
    tests/test_inflate_streams_model.py holds to the texts and to gunzip_edges.CATALOGUE_CODES -- asserted here once more, so that a
    refusal is the host's before it is the device's."""
    valid = ds.valid_cases()
    comp, want = b"".join(ge.catalogue_member(c) for c in valid), b"".join(c.text for c in valid)
    rc, h_info, h_text = gc.gunzip_host(eng.lib, comp, 1024, ge.ROUNDS, len(want))
    assert rc == 0 and (h_info["error"], h_info["n_members"], h_info["n_bytes"], h_info["consumed"]) == (0, len(valid), len(want), len(comp)), h_info
    assert bytes(h_text[gc.FRONT:gc.FRONT + len(want)]) == want
    d_info, d_text = gunzip_device(eng, comp, 1024, ge.ROUNDS, len(want))
    assert d_info == h_info, "device %s host %s" % (d_info, h_info)
    assert bytes(d_text[gc.FRONT:gc.FRONT + len(want)]) == want
    assert (d_text[:gc.FRONT] == gc.CANARY).all() and (d_text[gc.FRONT + (len(want) + 15) // 16 * 16:] == gc.CANARY).all()
    for k, c in enumerate(ds.invalid_cases()):
        m, cap = ge.catalogue_member(c), 65536
        rc, h_info, _ = gc.gunzip_host(eng.lib, m, 1024, ge.ROUNDS, cap)
        assert rc == 0 and (h_info["error"], h_info["n_members"], h_info["n_bytes"]) == (ge.catalogue_code(c.kind), 0, 0), "%s: host %s" % (c.name, h_info)
        d_info, d_text = gunzip_device(eng, m, 1024, ge.ROUNDS, cap, shift=k % 7)
        assert d_info == h_info, "%s: device %s host %s" % (c.name, d_info, h_info)
        assert (d_text[:gc.FRONT] == gc.CANARY).all() and (d_text[gc.FRONT + cap:] == gc.CANARY).all(), c.name + ": bytes outside the text buffer were written"
