"""The catalogue of tests/gunzip_edges.py on the MI355X: every match shape against a piece start, markers of markers, markers either side
of the resolved region, literals that wait, member edges from a later piece, the carried window, and the two catalogues of
deflate_streams.py as gzip members -- faqcs_gunzip_device and faqcs_gunzip_stream_device against the host statement, which is checked
against zlib first.  The wave's symbol sink (WaveSink<uint16_t> of faqcs_inflate_wave.h) has no host twin: the bit-for-bit comparison is its
test, at the shapes this catalogue feeds it.

One test per family and piece size, one engine for the module.  For every case the host statement runs first and is held to zlib's text and
verdict and to the chain model's piece count (gunzip_edges.check_info); then the device call goes into canary-filled buffers, the
compressed bytes k % 7 behind a 256-byte boundary: info equals the host's field for field (n_pieces, n_fixups and n_rounds included), the
text is the host's and zlib's, nothing is written in front of it or behind (n_bytes + 15) // 16 * 16 -- behind the capacity for a refused
file.

The invalid files that go to the device are exactly those that tests/test_gunzip_edges_model.py has put through the host statement and,
in tools/gunzip_probe_check.cpp, through the same text under AddressSanitizer and UBSan, where they were refused cleanly: they check a
refusal, none is built to fault.  A failed engine call stops the module's remaining tests: nothing more is started on the device."""
import time

import pytest

import gunzip_cases as gc
import gunzip_edges as ge
import gunzip_stream_cases as gsc
from test_gpu_gunzip import eng, gunzip_device  # noqa: F401  (eng: the module's engine fixture)
from test_gpu_gunzip_stream import device_call, device_window

pytestmark = pytest.mark.gpu
ENGINE_ERRORS = []
PAIRS = [(f, p) for f in ge.FAMILIES if f != "carried window" for p in gc.PIECES if ge.cases_of(f, p)]


def on_device(what, fn, *args, **kw):
    """one engine call; its failure is remembered and ends what the module does on the device"""
    from faqcs_amd.engine import FaqcsError

    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    try:
        return fn(*args, **kw)
    except FaqcsError as x:
        ENGINE_ERRORS.append("%s: %s" % (what, x))
        raise


def host_then_device(eng, c, piece, k):
    """-> (info, the device's whole text buffer) of a case whose host run and device run both hold"""
    what = "%s at %d" % (c.name, piece)
    cap = ge.capacity(c)
    rc, h_info, h_text = gc.gunzip_host(eng.lib, c.comp, piece, ge.ROUNDS, cap)
    assert rc == 0, what
    ge.check_info(c, piece, h_info, h_text, "host, " + what)      # (first: the verdict is the host's before it is the device's)
    d_info, d_text = on_device(what, gunzip_device, eng, c.comp, piece, ge.ROUNDS, cap, shift=k % 7)
    assert d_info == h_info, "%s: device %s host %s" % (what, d_info, h_info)
    ge.check_info(c, piece, d_info, d_text, what)
    nb = d_info["n_bytes"]
    assert (d_text[gc.FRONT:gc.FRONT + nb] == h_text[gc.FRONT:gc.FRONT + nb]).all(), what + ": the text differs from the host's"
    behind = (nb + 15) // 16 * 16 if c.bad is None else cap
    assert (d_text[gc.FRONT + behind:] == gc.CANARY).all(), what + ": bytes behind the text were written"
    return d_info, d_text


@pytest.mark.parametrize("family,piece", PAIRS, ids=["%s-%d" % (f.replace(" ", "_"), p) for f, p in PAIRS])
def test_catalogue(eng, family, piece):
    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    todo = ge.cases_of(family, piece)
    t0, n = time.time(), dict(n_pieces=0, n_rounds=0, n_fixups=0)
    for k, c in enumerate(todo):
        info, _ = host_then_device(eng, c, piece, k)
        for f in n:
            n[f] += info[f]
    print("%s at %d: %d cases, %d compressed bytes, %s, host and device %.1f s" % (family, piece, len(todo), sum(len(c.comp) for c in todo), n, time.time() - t0))


@pytest.mark.parametrize("piece", (1024, 0))
def test_the_carried_window(eng, piece):
    """the streamed family through faqcs_gunzip_stream_device, call by call against the host's call: info, every state field, the text and
    the window's valid bytes; on both sides zlib's text and state, the stops at the cuts and the chain model's pieces (gunzip_edges.run_feed)"""
    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    todo = ge.cases_of("carried window", piece)
    assert todo
    for k, c in enumerate(todo):
        what = "%s at %d" % (c.name, piece)
        h = ge.run_feed(gsc.host_call(eng.lib), c, piece)
        d = on_device(what, ge.run_feed, device_call(eng, k % 7), c, piece, window=device_window(k % 5))
        assert len(h) == len(d), what
        for n, (a, b) in enumerate(zip(h, d)):
            w = "%s, call %d" % (what, n)
            assert b.info == a.info, "%s: device %s host %s" % (w, b.info, a.info)
            assert b.state == a.state, "%s: device %s host %s" % (w, b.state, a.state)
            assert b.text == a.text, "%s: the text differs" % w
            assert b.window == a.window, "%s: the window differs" % w


def test_the_grid_twice_on_one_context(eng):
    """the first family once more, every file twice in a row on the module's context: the symbol buffer, the records and the slices of the
    call in front are reused, and nothing of them shows -- both results are the host's, the second at another alignment"""
    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    for c in ge.cases_of("piece start"):
        for piece in c.pieces:
            i1, t1 = host_then_device(eng, c, piece, 3)
            i2, t2 = host_then_device(eng, c, piece, 4)
            assert i1 == i2 and (t1 == t2).all(), c.name


def test_no_case_is_left_out():
    ran = {(c.name, p) for f, p in PAIRS for c in ge.cases_of(f, p)} | {(c.name, p) for p in (1024, 0) for c in ge.cases_of("carried window", p)}
    assert ran == {(c.name, p) for c in ge.cases() for p in c.pieces}
