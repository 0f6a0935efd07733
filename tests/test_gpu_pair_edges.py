"""The catalogue of tests/pair_edges.py on an MI355X: every case through faqcs_pair_device and faqcs_render_pair_device against the host
statements (faqcs_pair_host, faqcs_render_pair_host, which tests/test_pair_edges_model.py ties to the models and to the catalogue's own
expectations) -- route, info, text, rec_offset and rec_index byte for byte, canaries in front of and behind every buffer, every call twice
with identical bytes, the pair call also check-only with and without a route pointer.  One test per edge family, with the helpers of
test_gpu_pair.py and test_gpu_render.py; the big case is sized for the compute units of THIS device."""
import hashlib

import numpy as np
import pytest

import pair_cases as pcs
import pair_edges as pg
import render_cases as rc
import test_gpu_pair as gp
from faqcs_amd import _capi as capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    out = {}
    for name, args in pg.ARG_SETS.items():
        opt, e = gp.engine(args, R=capi.MAX_READ_LENGTH)
        out[name] = (e, capi.ParamsHolder(opt, capi.MAX_READ_LENGTH, rc.in_offset(args)))
    yield out
    for e, _ in out.values():
        e.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in pg.all_cases(big=False)}


@pytest.fixture(scope="module")
def big(n_cu):
    """The big case and its variants, built and uploaded once: -> {name: (case, DevicePair)}"""
    return {c.name: (c, gp.DevicePair(c)) for c in pg.big_cases(n_cu)}


def family(cases, *prefixes):
    out = [c for n, c in cases.items() if n.startswith(prefixes)]
    assert out
    return out


def tn_mates(dp, form):
    on, off = dp.mates(tn=True), dp.mates(tn=False)
    return {"both": on, "neither": off, "mate0": [on[0], off[1]], "mate1": [off[0], on[1]]}[form]


def run_pair(eng, case, dp=None):
    """Device == host statement for the pair call, twice with identical bytes; check only with and without a route pointer.
    -> (the route the rendering takes, the bytes the device wrote)"""
    import torch

    lib, n, made = eng.lib, case.n, []
    want_route, want = pcs.pair_host(lib, case, with_res=case.routed)
    if case.routed:
        m1, m2 = dp.mates()
        first = None
        for rep in range(2):
            route, info, raw = gp.pair_dev(eng, m1, m2, n)
            assert info == want, case.name
            assert (route == want_route).all(), "%s: route differs first at pair %d" % (case.name, int(np.nonzero(route != want_route)[0][0]))
            assert first is None or raw == first, "the second run's bytes differ"
            first = raw
        made.append(first)
        c1, c2 = dp.mates(with_res=(False, False), tn=False)
        _, want = pcs.pair_host(lib, case, with_res=False)
    else:  # deflines alone, back to back, in the hostile padding
        dev = torch.device("cuda:0")
        (c1, k1), (c2, k2) = gp.spans_on_device(dev, case.m[0]), gp.spans_on_device(dev, case.m[1])
    for with_route in (True, False):
        first = None
        for rep in range(2):
            r0, i0, raw = gp.pair_dev(eng, c1, c2, n, with_res=False, with_route=with_route)
            assert r0 is None and i0 == want, (case.name, i0, want)
            assert first is None or raw == first, "the second run's bytes differ"
            first = raw
        made.append(first)
    return want_route, made


def run_files(eng, holder, case, dp, route):
    """Device == host statement for each file of the case: with each form of the terminal_n pointers, with and without rec_offset / rec_index,
    twice with identical bytes; at the capacities of the overflow rule where the case asks for them.  -> the bytes the device wrote"""
    lib, made = eng.lib, []
    route = case.route if case.route is not None else route
    for f in case.files:
        full = pcs.render_pair_host(lib, holder, case, f, route, case.n_pairs, capacity=case.capacity)
        nb, nr = full["n_bytes"], full["n_reads"]
        m1, m2 = tn_mates(dp, case.tn_forms[0])
        if case.overflow:
            for cap in ((nb - 1, 0) if nb else ()) if case.overflow is True else (case.capacity,):
                want = pcs.render_pair_host(lib, holder, case, f, route, case.n_pairs, capacity=cap)
                assert want["overflow"] == 1
                o = gp.render_pair_dev(eng, dp, m1, m2, f, route, case.n_pairs, capacity=cap)
                assert (o["n_bytes"], o["n_reads"], o["overflow"]) == (want["n_bytes"], want["n_reads"], 1), (case.name, f, cap)
                rc.assert_untouched(o, nb, nr, overflow=True)
            if case.overflow == "only":
                continue
        cap = nb if case.overflow else case.capacity
        w = pcs.rendering(full)
        first = None
        for rep, form in enumerate((case.tn_forms[0],) + case.tn_forms):
            a, b = tn_mates(dp, form)
            arrays = rep < 2 or rep % 2 == 0
            o = gp.render_pair_dev(eng, dp, a, b, f, route, case.n_pairs, with_offset=arrays, with_index=arrays, capacity=cap)
            rc.assert_rendering(o, w, "%s file %d terminal_n %s" % (case.name, f, form))
            if nr == 0 and arrays:
                assert o["rec_offset"][0] == 0
            if rep < 2:
                raw = o["text"].tobytes() + o["rec_offset"].tobytes() + o["rec_index"].tobytes()
                assert first is None or raw == first, "the second run's bytes differ"
                first = raw
        made.append(hashlib.md5(first).hexdigest())
    return made


def run_case(engines, case, dp=None):
    eng, holder = engines[case.args]
    if case.routed and dp is None:
        dp = gp.DevicePair(case)
    route, made = run_pair(eng, case, dp) if case.pair else (None, [])
    if case.render:
        made += run_files(eng, holder, case, dp, route)
    return made


def test_id_length_spaces_lengths_suffixes_bytes_alignments(engines, cases):
    group = family(cases, "space_", "suffixes", "odd_byte", "every_alignment")
    assert len(group) == 18
    for case in group:
        run_case(engines, case)


@pytest.mark.parametrize("bit", ("bit0", "bit7"))
def test_ids_of_48_bytes_that_differ_in_one_byte(engines, cases, bit):
    """Each of the 48 positions, both ways round, as the last pair of a short clean base: n_pairs, mismatch and id_len."""
    group = family(cases, "one_byte_%s_at_" % bit)
    assert len(group) == 96
    eng = engines["default"][0]
    for case in group:
        run_case(engines, case)
        _, info = pcs.pair_host(eng.lib, case, with_res=False)
        assert (info["n_pairs"], info["mismatch"], info["id_len"]) == (case.n - 1, 1, (48, 48)), case.name


def test_equal_ids_with_different_bytes_behind_them(engines, cases):
    group = family(cases, "equal_ids_then_different_bytes", "suffix_against_two_id_bytes_", "two_id_bytes_against_suffix_")
    assert len(group) == 7
    eng = engines["default"][0]
    for case in group:
        run_case(engines, case)
        _, info = pcs.pair_host(eng.lib, case, with_res=False)
        assert info["mismatch"] == (0 if case.name.startswith("equal_ids") else 1) and info["n_pairs"] == case.n - info["mismatch"], case.name


def test_check_tile_sizes(engines, cases):
    group = family(cases, "check_")
    assert len(group) == 2 * len(pg.CHECK_SIZES)
    for case in group:
        run_case(engines, case)


def test_check_tile_first_mismatch_placements(engines, cases):
    group = family(cases, "bad_tile", "two_bad_", "bad_in_every_wave")
    assert len(group) == 13
    for case in group:
        run_case(engines, case)


def test_counters_beyond_24_and_32_bits(engines, cases):
    for case in family(cases, "tile_of_65535", "sum_above_2_32"):
        run_case(engines, case)


@pytest.mark.parametrize("nt", (1023, 1024, 1025))
def test_finishing_block_at_one_round_of_tiles(engines, cases, nt):
    case = cases["n_tiles_%d" % nt]
    assert case.ctx().n_tiles == nt
    run_case(engines, case)


@pytest.mark.parametrize("name", ("big_clean", "big_bad_at_3", "big_bad_beyond_round", "big_bad_last"))
def test_beyond_one_round_of_the_finishing_block_and_the_void_tail(engines, big, n_cu, name):
    """The big case, sized for THIS device: the mismatch placements of pair_finish's second round and of pair_void_tail's second stride, and
    the four files over its 2 n candidates (the one-block scan of the rendering in its second round)."""
    case, dp = big[name]
    c = case.ctx()
    E = pg.big_edges(n_cu)
    print("n_cu %d: %d pairs in %d tiles, the void tail's grid holds %d pairs" % (n_cu, case.n, c.n_tiles, n_cu * pg.VOID_BLOCKS_PER_CU * 256))
    assert case.n == pg.big_size(n_cu) > max(n_cu * pg.VOID_BLOCKS_PER_CU * 256, pg.SCAN_THREADS * 512)
    lost = [e for e in case.claims if e in E and not E[e](c)]
    assert not lost, "with %d compute units %s does not reach %s" % (n_cu, name, lost)
    run_case(engines, case, dp)


def test_route_truth_table(engines, cases):
    """route[i] = i for 256 pairs: exactly the statement's candidates appear in each file."""
    case = cases["route_truth_table"]
    run_case(engines, case)
    eng, holder = engines[case.args]
    for f in pg.FILES:
        o = pcs.render_pair_host(eng.lib, holder, case, f, case.route, 256, capacity=case.capacity)
        want = {pg.QC1: [6], pg.QC2: [7], pg.UNPAIRED: [2, 5], pg.DISCARD: [0, 1, 3, 4]}[f]
        assert o["rec_index"][:o["n_reads"]].tolist() == want, f


def test_scan_of_the_paired_rendering(engines, cases):
    group = family(cases, "render_", "fewer_pairs_than_reads", "candidate_tile", "last_of_tile_first_of_next_")
    assert len(group) == len(pg.RENDER_SIZES) + 5
    for case in group:
        run_case(engines, case)


def test_overflow_and_engine_arguments(engines, cases):
    """One byte short and exact, an empty file at capacity 0, a thread's own sum beyond 2^32; under each of the three argument sets."""
    group = family(cases, "mid_", "all_routed_3", "thread_sum_2_32")
    assert len(group) == 5 and {c.args for c in group} == set(pg.ARG_SETS)
    for case in group:
        run_case(engines, case)


def test_source_by_mate(engines, cases):
    group = family(cases, "shadow_mates", "short_against_long", "terminal_N_", "four_flagged_")
    assert len(group) == 16
    for case in group:
        run_case(engines, case)


@pytest.mark.parametrize("file", ("unpaired", "discard"))
def test_gather_across_mates(engines, cases, file):
    group = [c for c in cases.values() if c.family == "gather" and (c.name.endswith("_" + file) or (file == "discard" and c.name == "records_of_5_to_15_bytes"))]
    assert len(group) >= 20
    for case in group:
        run_case(engines, case)


def test_context_reuse(big, cases):
    """On one context: the big mismatching case, a 300-pair clean routed case, a check-only call, the big clean case -- each correct and
    byte-identical to what a fresh context writes."""
    small = pg.PairCase("clean_300", "tiles", (), *pg.tiny_mates(300))
    sequence = [big["big_bad_at_3"], (small, gp.DevicePair(small)), (cases["suffixes"], None), big["big_clean"]]

    def fresh():
        opt, e = gp.engine([], R=capi.MAX_READ_LENGTH)
        return {"default": (e, capi.ParamsHolder(opt, capi.MAX_READ_LENGTH, 33))}

    shared = fresh()
    on_one = [run_case(shared, case, dp) for case, dp in sequence]
    shared["default"][0].close()
    for (case, dp), made in zip(sequence, on_one):
        alone = fresh()
        assert run_case(alone, case, dp) == made, case.name
        alone["default"][0].close()


def test_no_case_is_left_out(cases):
    prefixes = ("space_", "suffixes", "odd_byte", "every_alignment", "one_byte_bit0_at_", "one_byte_bit7_at_", "equal_ids_then_different_bytes", "suffix_against_two_id_bytes_",
                "two_id_bytes_against_suffix_", "check_", "bad_tile", "two_bad_", "bad_in_every_wave", "tile_of_65535", "sum_above_2_32", "n_tiles_", "route_truth_table", "render_",
                "fewer_pairs_than_reads", "candidate_tile", "last_of_tile_first_of_next_", "mid_", "all_routed_3", "thread_sum_2_32", "shadow_mates", "short_against_long",
                "terminal_N_", "four_flagged_")
    assert all(c.family == "gather" or n.startswith(prefixes) for n, c in cases.items())
