"""The catalogue of tests/deflate_edges.py on an MI355X: every case through HipEngine and faqcs_deflate_device_mode in both modes, into
canary-filled device buffers (test_gpu_deflate_dense.deflate_device_mode), the text `case index mod 5` bytes behind an aligned address (the index in
the whole catalogue; the second run of a call three bytes further, mod 5).  The device's info, comp[0 .. n_bytes) and member_offset are held to the plain model first (run once per module), then to the host statement
faqcs_deflate_host_mode: of the three, a difference says which stands alone.  Every call runs twice on the same engine, at the two shifts, and must give equal
bytes; the calls of the `call` family also come back through faqcs_inflate_device.  One test per family and mode."""
import ctypes as C
import time

import numpy as np
import pytest

import deflate_cases as dc
import deflate_dense_cases as dd
import deflate_edges as de
from faqcs_amd import _capi as capi
from test_gpu_deflate_dense import deflate_device_mode, eng  # noqa: F401  (the engine fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return de.all_cases()


def back_through_inflate(eng, o, text, what):
    """comp and member_offset as the device wrote them -> faqcs_inflate_device -> the text"""
    import torch

    from faqcs_amd.device import inflated_text

    nb, n = o["info"]["n_bytes"], o["info"]["n_members"]
    comp = torch.from_numpy(o["comp"][dc.FRONT:dc.FRONT + nb].copy()).to("cuda:0")
    moff = torch.from_numpy(o["member_offset"][:n + 1].view(np.int32).copy()).to("cuda:0")
    back, _ = inflated_text(eng, comp, moff)
    assert int(back.numel()) == len(text) and bytes(back.cpu().numpy()) == text, what + ": back through faqcs_inflate_device"


@pytest.mark.parametrize("mode", de.MODES, ids=[de.MODE_NAME[m] for m in de.MODES])
@pytest.mark.parametrize("family", de.FAMILIES)
def test_catalogue(eng, cases, family, mode):
    todo = de.cases_of(family, cases)
    assert todo
    t0 = time.time()
    for case in todo:
        case.expected(mode)
    t1 = time.time()
    n_calls = 0
    index_of = {c.name: k for k, c in enumerate(cases)}     # the catalogue-wide case index decides the text's shift
    for case in todo:
        index = index_of[case.name]
        v = case.view(mode)
        for k, c in enumerate(v.calls):
            what = "%s call %d (%s)" % (case.name, k, de.MODE_NAME[mode])
            mb, e = case.calls[k][1], c["out"]
            runs = []
            for turn in range(2):
                rc, o = deflate_device_mode(eng, c["text"], mb, c["final"], mode=mode, capacity=c["capacity"], shift=(index + 3 * turn) % 5)
                assert rc == 0, what
                runs.append(o)
            o = runs[0]
            nb, n = e["info"]["n_bytes"], e["info"]["n_members"]
            rc, h = dd.deflate_host_mode(eng.lib, c["text"], mb, c["final"], mode=mode, capacity=c["capacity"])
            assert rc == 0
            if e["info"]["overflow"]:
                assert o["info"] == e["info"] == h["info"], "%s: device %s, model %s, host %s" % (what, o["info"], e["info"], h["info"])
                dc.assert_nothing_written(o)
                dc.assert_nothing_written(runs[1])
                continue
            # 1. the model
            got = bytes(o["comp"][dc.FRONT:dc.FRONT + nb])
            bad = de.first_difference(case, k, mode, got, o["info"], o["member_offset"][:n + 1])
            host = bytes(h["comp"][dc.FRONT:dc.FRONT + nb])
            if bad:
                alone = "the device stands alone: the host statement equals the model" if host == e["comp"] and h["info"] == e["info"] else \
                    "the model stands alone: the device equals the host statement" if host == got and h["info"] == o["info"] else "all three differ"
                raise AssertionError("%s; %s" % (bad, alone))
            assert o["member_offset"][n + 1] == dc.CAN32, what
            assert (o["comp"][:dc.FRONT] == dc.CANARY).all() and (o["comp"][dc.FRONT + (nb + 15) // 16 * 16:] == dc.CANARY).all(), what + ": canaries"
            # 2. the host statement
            assert h["info"] == o["info"] and host == got and (h["member_offset"][:n + 1] == o["member_offset"][:n + 1]).all(), what + ": the host statement differs from device and model"
            # 3. the same call again
            assert runs[1]["info"] == o["info"] and (runs[1]["comp"] == o["comp"]).all() and (runs[1]["member_offset"] == o["member_offset"]).all(), what + ": the second run differs"
            # 4. back through the device's inflate
            if family == "call":
                back_through_inflate(eng, o, c["text"], what)
            n_calls += 1
    print("%s (%s): %d cases, %d calls, %d bytes, model %.1f s, device and host %.1f s" % (family, de.MODE_NAME[mode], len(todo), n_calls, sum(c.n_bytes() for c in todo), t1 - t0,
                                                                                     time.time() - t1))


def test_no_case_is_left_out(cases):
    assert sorted(c.name for f in de.FAMILIES for c in de.cases_of(f, cases)) == sorted(c.name for c in cases)
