"""CPU-side checks of the pair stage (faqcs_pair_device / faqcs_render_pair_device): the host statements (faqcs_pair_host,
faqcs_render_pair_host) against the numpy models written from parse_id and FaQCs.cpp:296-361, against the EXISTING rendering statement on a
joined batch, and against the reference's own files and messages (the golden cases); the statements under AddressSanitizer and UBSan as a
stand-alone program (tools/pair_host_fuzz.cpp); the entry points' argument checks."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import pair_cases as pcs
import render_cases as rc
from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    return capi.load_library()


def test_the_id_catalogue_says_what_it_claims():
    """parse_id on the catalogue: the matching entries match, the others do not, and the named cases of the rules hold."""
    for a, b in pcs.matching():
        assert driver.parse_id(a) == driver.parse_id(b), (a, b)
    for a, b, ia, ib in pcs.mismatching():
        assert ia != ib, (a, b)
    P = driver.parse_id
    assert (P(b"x/1"), P(b"x.1"), P(b"x/12"), P(b"/1"), P(b"a/1"), P(b"id comment/1"), P(b"a\tb c"), P(b""), P(b"1")) == (
        b"x", b"x", b"x/12", b"", b"a", b"id", b"a\tb", b"", b"1")
    lens = {len(a) for a, b in pcs.matching()} | {len(a) for a, b, _, _ in pcs.mismatching()}
    assert {0, 1, 2, 15, 16, 17, 31, 32, 33, 300} <= lens


PLACEMENTS = {"none": (300, 300, ()), "at_0": (300, 300, (0,)), "at_last": (300, 300, (299,)), "two_lower_wins": (300, 300, (211, 37)),
              "mate1_longer": (330, 290, ()), "mate2_longer": (280, 333, (279,)), "no_pairs": (0, 7, ()), "nothing": (0, 0, ()), "every_pair_bad": (40, 40, tuple(range(40)))}


@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_pair_host_equals_the_model(lib, name):
    """Random pairs with ids from the catalogue, mismatches placed as named, unequal counts both ways and n = 0: route and info of
    faqcs_pair_host equal driver.pair_model exactly, the canaries around route stay, and the check-only form (no results) gives the same
    verdict with zero counters and writes no route."""
    n1, n2, bad = PLACEMENTS[name]
    rng = np.random.default_rng([21, list(PLACEMENTS).index(name)])
    pc = pcs.PairCase(rng, n1, n2, bad=bad)
    n = min(n1, n2)
    want_route, want = driver.pair_model(*pc.model_mates())
    route, info = pcs.pair_host(lib, pc)
    assert info == want, name
    assert (route == want_route).all(), name
    assert info["n_pairs"] == (min(bad) if bad else n) and info["mismatch"] == (1 if bad else 0)
    assert (route[info["n_pairs"]:] == capi.ROUTE_NOWHERE).all() and (route[:info["n_pairs"]] < 4).all()
    if not bad and n:
        assert len(set(route.tolist())) == 4  # every route occurs
        assert info["paired_read_number"] == 2 * int((route == 3).sum()) > 0 and info["paired_base_length"] > 0
        assert info["n_one_valid"] == int(((route == 1) | (route == 2)).sum()) and info["n_none_valid"] == int((route == 0).sum())
    if bad:
        i = info["n_pairs"]
        ids = [bytes(c.text[c.def_pos[i]:c.def_pos[i] + ln]) for c, ln in zip(pc.m, info["id_len"])]
        assert ids == [driver.parse_id(pc.r1[i][0]), driver.parse_id(pc.r2[i][0])] and ids[0] != ids[1]
    # check only
    none_route, none_want = driver.pair_model(*pc.model_mates(with_res=False))
    for with_route in (True, False):
        r0, i0 = pcs.pair_host(lib, pc, with_res=False, with_route=with_route)
        assert r0 is None and none_route is None and i0 == none_want
    assert {k: none_want[k] for k in ("n_pairs", "mismatch", "id_len")} == {k: want[k] for k in ("n_pairs", "mismatch", "id_len")}
    assert (none_want["paired_read_number"], none_want["paired_base_length"], none_want["n_one_valid"], none_want["n_none_valid"]) == (0, 0, 0, 0)


def test_every_catalogue_entry_alone(lib):
    """Each entry of the catalogue as pair 1 of 3: the statement's verdict and id lengths are parse_id's."""
    rng = np.random.default_rng(22)
    for a, b in pcs.matching() + [x[:2] for x in pcs.mismatching()]:
        for x, y in ((a, b), (b, a)):
            pc = pcs.PairCase(rng, 3, deflines=[(b"same", b"same/2"), (x, y), (b"s", b"s")], max_len=8)
            ix, iy = driver.parse_id(x), driver.parse_id(y)
            route, info = pcs.pair_host(lib, pc)
            if ix == iy:
                assert (info["n_pairs"], info["mismatch"], info["id_len"]) == (3, 0, (0, 0)), (x, y)
            else:
                assert (info["n_pairs"], info["mismatch"], info["id_len"]) == (1, 1, (len(ix), len(iy))), (x, y)
                assert route.tolist()[1:] == [capi.ROUTE_NOWHERE] * 2


@pytest.mark.parametrize("args", rc.OPTION_SETS, ids=lambda a: " ".join(a) or "default")
def test_render_pair_host_equals_render_host_on_the_joined_batch(lib, args):
    """Two mates of 260 random reads (random F_VALID, random windows with empty ones, N runs, deflines from the catalogue), a mismatch at pair
    200 so that 60 pairs are routed nowhere: each of the four files, with rec_offset and rec_index, equals faqcs_render_host on the joined
    batch with the masks and the interleave of render_cases.file_plans -- and the numpy model.  One byte short: nothing but info is written."""
    rng = np.random.default_rng([23, rc.OPTION_SETS.index(args)])
    opt = parse_args(["-1", "a", "-2", "b", "-d", "y"] + args)
    in_off = rc.in_offset(args)
    h = capi.ParamsHolder(opt, 256, in_off)
    for bad, n1, n2 in (((200,), 260, 260), ((), 130, 150)):
        pc = pcs.PairCase(rng, n1, n2, bad=bad, in_off=in_off)
        route, info = pcs.pair_host(lib, pc)
        n = pc.n
        assert info["n_pairs"] == (200 if bad else n)
        want = pcs.joined_files(lib, h, pc, route)
        seen = np.zeros(2 * n, int)
        for f in pcs.FILES:
            assert len(want[f][2]) > 10
            for n_pairs in sorted({n, info["n_pairs"]}):  # (the pairs behind the mismatch are routed nowhere: n and n_pairs give the same file)
                for with_offset, with_index in ((True, True), (False, False)):
                    o = pcs.render_pair_host(lib, h, pc, f, route, n_pairs, with_offset=with_offset, with_index=with_index)
                    rc.assert_rendering(o, want[f], "%s file %d n_pairs %d" % (args, f, n_pairs))
            model = driver.render_pair_model(opt, in_off, f, *pc.model_mates(), route, n)
            assert model[0].tobytes() == want[f][0].tobytes() and (model[1] == want[f][1]).all() and (model[2] == want[f][2]).all()
            if f != capi.FILE_DISCARD:
                seen[want[f][2]] += 1
            else:  # the discard file does not read results
                o = pcs.render_pair_host(lib, h, pc, f, route, n, with_res=(False, False))
                rc.assert_rendering(o, want[f])
            nb, nr = len(want[f][0]), len(want[f][2])
            for cap in (nb - 1, 0):
                o = pcs.render_pair_host(lib, h, pc, f, route, n, capacity=cap)
                assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (nb, nr, 1)
                rc.assert_untouched(o, nb, nr, overflow=True)
            rc.assert_rendering(pcs.render_pair_host(lib, h, pc, f, route, n, capacity=nb), want[f])
        # a valid mate of a routed pair is in exactly one trimmed file, a mate routed nowhere in none
        valid = np.stack([(c.res["flags"][:n] & 1) != 0 for c in pc.m], axis=1).ravel()
        routed = np.repeat(route != capi.ROUTE_NOWHERE, 2)
        assert (seen == (valid & routed)).all()
        assert not np.isin(want[capi.FILE_DISCARD][2] >> 1, np.nonzero(route == capi.ROUTE_NOWHERE)[0]).any()
    # no pairs: zeros and rec_offset[0] = 0
    for f in pcs.FILES:
        o = pcs.render_pair_host(lib, h, pc, f, route, 0)
        assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (0, 0, 0) and o["rec_offset"][0] == 0
        rc.assert_untouched(o, 0, 0)


def _parse_host(lib, text):
    """faqcs_parse_host of one mate's text -> a render_cases.Case-like object (text, spans, arenas with slack, offsets)"""
    t = np.frombuffer(text, np.uint8)
    n_max = text.count(b"\n") // 4 + 1
    seq, qual = np.zeros(64 + len(t) + 64, np.uint8), np.zeros(64 + len(t) + 64, np.uint8)
    so, qo = 16 + (-(seq.ctypes.data + 16)) % 16, 16 + (-(qual.ctypes.data + 16)) % 16
    off, tn, dpos, dlen = np.zeros(n_max + 1, np.uint32), np.zeros(n_max, np.uint8), np.zeros(n_max, np.uint32), np.zeros(n_max, np.uint32)
    info = capi.ParseInfo()
    out = capi.ParseOut(seq.ctypes.data + so, qual.ctypes.data + qo, len(t), n_max, off.ctypes.data, tn.ctypes.data, dpos.ctypes.data, dlen.ctypes.data,
                        C.addressof(info))
    assert lib.faqcs_parse_host(t.ctypes.data, len(t), 1, C.byref(out)) == 0
    assert (info.error, info.overflow) == (0, 0)
    n = info.n_reads

    class Mate:
        pass

    m = Mate()
    m.n, m.text, m.def_pos, m.def_len = n, t, dpos[:n], dlen[:n]
    m.seq, m.qual, m.offset, m.tn = seq[so:], qual[qo:], off[:n + 1], tn[:n]
    m.res = None
    return m


class _Pair:
    def __init__(self, m1, m2):
        self.m, self.n = [m1, m2], min(m1.n, m2.n)


PAIRED_GOLDEN = [n for n in rc.GOLDEN if n != "adv_unpaired_only"]


@pytest.mark.parametrize("name", PAIRED_GOLDEN)
def test_pair_statements_reproduce_the_reference_files(lib, name, fixture_cache, tmp_path):
    """Every paired golden case, two texts: faqcs_parse_host per mate, the oracle's per-read results, faqcs_pair_host, four
    faqcs_render_pair_host: md5, bytes and records of each file are the reference's, and the pair counters are what driver.py's loop counts."""
    import golden_util
    from oracle_engine import OracleEngine

    case, opt, in_off, r1, r2 = rc.golden_inputs(name, fixture_cache, tmp_path)
    assert r2 is not None
    m1, m2 = _parse_host(lib, rc.fastq_text(r1)), _parse_host(lib, rc.fastq_text(r2))
    m = len(r1)
    assert m1.n == m2.n == m
    seq, qual, offset, seg = driver.pack_segments([r1, r2])
    res = OracleEngine(opt, 1024, in_off).process(seq, qual, offset, seg)
    m1.res, m2.res = np.ascontiguousarray(res[:m]), np.ascontiguousarray(res[m:])
    pc = _Pair(m1, m2)
    route, info = pcs.pair_host(lib, pc)
    assert (info["n_pairs"], info["mismatch"]) == (m, 0)
    h = capi.ParamsHolder(opt, 1024, in_off)
    for f in pcs.FILES:
        fn = capi.PAIR_FILES[f]
        o = pcs.render_pair_host(lib, h, pc, f, route, m)
        text = o["text"][o["base"]:o["base"] + o["n_bytes"]].tobytes()
        if fn in case["fastq"]:
            meta = case["fastq"][fn]
            assert (o["n_reads"], o["n_bytes"], o["overflow"]) == (meta["records"], meta["bytes"], 0), fn
            assert hashlib.md5(text).hexdigest() == meta["md5"], fn
        else:
            assert fn == "QC.discard.trimmed.fastq"  # (written only with --discard)
    assert set(case["fastq"]) <= set(capi.PAIR_FILES)
    # the counters of the host driver's own loop on the same command line
    assert golden_util.run_case(case, fixture_cache, tmp_path, lambda o, R, q: OracleEngine(o, R, q),
                                max_read_length=golden_util.case_max_read_length(case)) == []
    run = driver.run.last
    assert (info["paired_read_number"], info["paired_base_length"]) == (run.paired_read_number, run.paired_base_length)
    assert info["paired_read_number"] > 0


def test_mate_id_mismatch_as_the_reference_reports_it(lib, fixture_cache):
    """The fixture of err_mate_id_mismatch: mismatch = 1 and the two ids are the ones in the reference's message."""
    import golden_util
    import make_fixtures

    case = golden_util.load_case("err_mate_id_mismatch")
    p1, p2 = golden_util.fixture_paths(case["fixture"], fixture_cache)
    m1, m2 = (_parse_host(lib, rc.fastq_text(make_fixtures.read_fastq(p))) for p in (p1, p2))
    pc = _Pair(m1, m2)
    route, info = pcs.pair_host(lib, pc, with_res=False)
    assert route is None and info["mismatch"] == 1
    i = info["n_pairs"]
    ids = [bytes(c.text[c.def_pos[i]:c.def_pos[i] + ln]).decode() for c, ln in zip(pc.m, info["id_len"])]
    assert ids == ["@R20", "@OTHER20"]
    assert "Read one id (%s)" % ids[0] in case["stderr"] and "read two id (%s)" % ids[1] in case["stderr"]
    assert i == 20


def test_pair_statements_under_the_sanitizers(tmp_path):
    """tools/pair_host_fuzz.cpp: the two host statements as a stand-alone program with AddressSanitizer and UBSan, generated and mutated
    inputs in buffers of exactly the stated sizes, against a naive statement inside the program.  Nothing here is loaded into Python."""
    exe = str(tmp_path / "pair_host_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "pair_host_fuzz.cpp"), os.path.join(ROOT, "faqcs_amd", "csrc", "faqcs_host.cpp")],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run([exe, os.environ.get("FAQCS_TEST_SEED", "20261018"), "400"], capture_output=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert r.stderr == b"", r.stderr.decode()[-2000:]
    assert b"400 cases: ok" in r.stdout, r.stdout.decode()[-500:]


def test_pair_entry_points_are_declared_and_check_their_arguments(lib):
    for s in ("faqcs_pair_device", "faqcs_pair_host", "faqcs_render_pair_device", "faqcs_render_pair_host", "faqcs_pair_time_ms", "faqcs_render_pair_time_ms"):
        assert s in capi.declared_symbols() and hasattr(lib, s)
    assert C.sizeof(capi.PairInfo) == 40 and C.sizeof(capi.Mate) == 40
    assert (capi.ROUTE_V1, capi.ROUTE_V2, capi.ROUTE_NOWHERE) == (1, 2, 0x80)
    rng = np.random.default_rng(24)
    pc = pcs.PairCase(rng, 5)
    hm = pcs.HostMates(pc)
    a, b = hm.mates
    route = np.zeros(8, np.uint8)
    info = capi.PairInfo()
    ia = C.addressof(info)
    # a null context is refused at call time, before any device is touched
    assert lib.faqcs_pair_device(None, C.byref(a), C.byref(b), route.ctypes.data, ia) == capi.E_INVAL
    assert b"null ctx" in lib.faqcs_last_error()
    x, y = C.c_double(), C.c_double()
    assert lib.faqcs_pair_time_ms(None, C.byref(x), C.byref(y)) == capi.E_INVAL
    assert lib.faqcs_render_pair_time_ms(None, C.byref(x), C.byref(y)) == capi.E_INVAL
    assert lib.faqcs_pair_host(C.byref(a), C.byref(b), route.ctypes.data, ia) == 0
    assert lib.faqcs_pair_host(None, C.byref(b), route.ctypes.data, ia) == capi.E_INVAL
    assert lib.faqcs_pair_host(C.byref(a), None, route.ctypes.data, ia) == capi.E_INVAL
    assert lib.faqcs_pair_host(C.byref(a), C.byref(b), route.ctypes.data, None) == capi.E_INVAL
    assert lib.faqcs_pair_host(C.byref(a), C.byref(b), None, ia) == capi.E_INVAL  # results without a route
    one = pcs.HostMates(pc, (True, False)).mates
    assert lib.faqcs_pair_host(C.byref(one[0]), C.byref(one[1]), route.ctypes.data, ia) == capi.E_INVAL  # exactly one results
    one = pcs.HostMates(pc, (False, True)).mates
    assert lib.faqcs_pair_host(C.byref(one[0]), C.byref(one[1]), route.ctypes.data, ia) == capi.E_INVAL
    nobatch = capi.Mate(None, a.results, a.text, a.def_pos, a.def_len)
    assert lib.faqcs_pair_host(C.byref(nobatch), C.byref(b), route.ctypes.data, ia) == capi.E_INVAL
    for bad in (capi.Mate(a.batch, a.results, None, a.def_pos, a.def_len), capi.Mate(a.batch, a.results, a.text, None, a.def_len),
                capi.Mate(a.batch, a.results, a.text, a.def_pos, None)):
        assert lib.faqcs_pair_host(C.byref(bad), C.byref(b), route.ctypes.data, ia) == capi.E_INVAL
    big = capi.Batch(None, None, None, 1 << 31, 0, None, 0, None)
    bigm = capi.Mate(C.pointer(big), a.results, a.text, a.def_pos, a.def_len)
    assert lib.faqcs_pair_host(C.byref(bigm), C.byref(bigm), route.ctypes.data, ia) == capi.E_INVAL  # n > 2^31 - 1
    # the rendering
    opt = parse_args(["-1", "a", "-2", "b", "-d", "y"])
    h = capi.ParamsHolder(opt, 256, 33)
    rinfo = capi.RenderInfo()
    buf = np.zeros(4096, np.uint8)
    t = buf.ctypes.data + (-buf.ctypes.data) % 16
    good = capi.RenderOut(t, 2048, None, None, C.addressof(rinfo))
    P = C.byref(h.p)
    assert lib.faqcs_render_pair_device(None, 0, C.byref(a), C.byref(b), route.ctypes.data, 5, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_pair_host(P, 0, C.byref(a), C.byref(b), route.ctypes.data, 5, C.byref(good)) == 0
    for f in (-1, 4, 77):
        assert lib.faqcs_render_pair_host(P, f, C.byref(a), C.byref(b), route.ctypes.data, 5, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_pair_host(P, 0, C.byref(a), C.byref(b), route.ctypes.data, 6, C.byref(good)) == capi.E_INVAL  # more pairs than reads
    assert lib.faqcs_render_pair_host(P, 0, C.byref(a), C.byref(b), None, 5, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_pair_host(P, 0, None, C.byref(b), route.ctypes.data, 5, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_pair_host(P, 0, C.byref(a), C.byref(b), route.ctypes.data, 5, None) == capi.E_INVAL
    assert lib.faqcs_render_pair_host(P, 0, C.byref(bigm), C.byref(bigm), route.ctypes.data, 1 << 31, C.byref(good)) == capi.E_INVAL
    nores = pcs.HostMates(pc, (True, False)).mates
    assert lib.faqcs_render_pair_host(P, capi.FILE_UNPAIRED, C.byref(nores[0]), C.byref(nores[1]), route.ctypes.data, 5, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_render_pair_host(P, capi.FILE_DISCARD, C.byref(nores[0]), C.byref(nores[1]), route.ctypes.data, 5, C.byref(good)) == 0
    for bad in (capi.RenderOut(None, 64, None, None, C.addressof(rinfo)), capi.RenderOut(t, 64, None, None, None), capi.RenderOut(t + 4, 64, None, None, C.addressof(rinfo))):
        assert lib.faqcs_render_pair_host(P, 0, C.byref(a), C.byref(b), route.ctypes.data, 5, C.byref(bad)) == capi.E_INVAL
