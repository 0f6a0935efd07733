"""The catalogue of tests/kmer_exchange_edges.py without a GPU: its restated constants against the sources, its coverage table (every predicate
put to every case: no edge unreached, no claim that does not hold, no case outside the families), the sender's and the owner's bucket rule
against each other for every world size and bucket, the one-key-one-owner invariant in both modes, the model summed over all owners
against the oracle on the same reads in file order, and the mutants of the model, each told from the right model by a named case."""
import os
import re

import numpy as np
import pytest

import kmer_exchange_edges as kx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faqcs_amd", "csrc")


@pytest.fixture(scope="module")
def cases():
    return kx.all_cases()


def source(name):
    return open(os.path.join(CSRC, name)).read()


def test_restated_constants_equal_the_sources():
    for name, (fn, rx) in kx.CONSTANT_SOURCES.items():
        m = re.search(rx, source(fn))
        assert m, "%s: %s no longer states it as %r" % (name, fn, rx)
        assert getattr(kx, name) == int(m.group(1)), name
    skm, kmer, capi = source("faqcs_skm.h"), source("faqcs_kmer.h"), source("faqcs_capi_kmer.hip")
    # the item: 16 bytes, (k-mers - 1) in 5 bits at NK, the partition, the run / epoch
    assert re.search(r"w1 >> SKM_NK_SHIFT\) & 31u\) \+ 1u", skm) and kx.NK_BITS == 5 and kx.NK_SHIFT + kx.NK_BITS == kx.PART_SHIFT
    assert kx.PART_SHIFT + kx.PART_BITS == kx.RUN_SHIFT and kx.RUN_SHIFT + kx.RUN_BITS == 64 and "Item (16 bytes)" in skm
    assert (1 << kx.RUN_BITS) > kx.KG_EPOCH_SPAN - 1 and (1 << kx.RUN_BITS) > kx.KG_MAX_RUNS - 1
    # kmer_mix and kmer_owner
    m = re.search(r"kmer_mix\(uint64_t x\)\s*\{\s*x \^= x >> (\d+); x \*= (0x[0-9a-f]+)ull; x \^= x >> (\d+); x \*= (0x[0-9a-f]+)ull; x \^= x >> (\d+);", kmer)
    assert m and [int(m.group(i), 0) for i in range(1, 6)] == [kx.MIX_SHIFT, kx.MIX_1, kx.MIX_SHIFT, kx.MIX_2, kx.MIX_SHIFT]
    assert "return (uint32_t)(((kmer_mix(key) >> 32) * (uint64_t)world) >> 32);" in kmer
    x = 0x0123456789abcdef
    for mul in (kx.MIX_1, kx.MIX_2):  # the same on Python ints
        x ^= x >> 33
        x = (x * mul) & (2 ** 64 - 1)
    assert int(kx.kmer_mix(np.array([0x0123456789abcdef], np.uint64))[0]) == x ^ (x >> 33)
    # the direct path's threshold, the sender's rule, the owner's rule, cap1, the refusal
    assert "if (n_epochs > (uint32_t)KG_EPOCH_SPAN) c->kg.direct = true;" in capi
    assert "const uint32_t d = (i * world) >> 8;" in source("faqcs_kmer_skm_kernel.hip")
    assert "lo_b = (c->part_rank * 256u + c->part_world - 1u) / c->part_world, hi_b = ((c->part_rank + 1u) * 256u + c->part_world - 1u) / c->part_world;" in capi
    assert "d.part_lo = lo_b << 11;" in capi and "(1ull << 51) / ((uint64_t)(hi_b - lo_b) << 11)" in capi
    assert "std::max<uint64_t>(KG_MIN_CAP, 2 * ib / ((uint64_t)KG_FAN * KG_FAN) + 64)" in capi and "(w == 1 ? occ : occ * 3 / (w + 1)) + 2ull * s.n + 64" in capi
    assert all(sub.error in capi for c in kx.all_cases() for subs in c.senders for sub in subs if sub.error)
    assert kx.SMALL_GROUP == 1 << 14 and "v >= (1ull << 14)" in capi


def test_every_edge_is_reached_every_claim_holds_every_case_has_a_family(cases):
    assert len({c.name for c in cases}) == len(cases), "two cases share a name"
    table, lost, _ = kx.coverage(cases)
    assert not lost, "claims that do not hold: %s" % lost
    missing = sorted(e for e, v in table.items() if not v)
    assert not missing, "edges no case reaches: %s" % missing
    assert all(c.family in kx.FAMILIES for c in cases) and {c.family for c in cases} == set(kx.FAMILIES)
    assert all(c.claims for c in cases), "a case that claims nothing"
    assert len(table) >= 360
    assert sorted(c.world for c in cases if c.name.startswith("owners_world_") and c.k == 31) == sorted(kx.WORLDS)
    assert all(c.world <= kx.WORLD_MAX for c in cases) and set(kx.MUTANTS.values()) <= {c.name for c in cases}


def test_the_sender_rule_and_the_owner_rule_agree_for_every_world_and_bucket():
    """(b * world) >> 8 == r exactly when ceil(r * 256 / world) <= b < ceil((r + 1) * 256 / world), and the owner's map of its partitions
    onto [0, 2^19) -- ((part - part_lo) * part_mul) >> 32, part_mul = floor(2^51 / n), kg_init -- is injective and below 2^19: on Python ints"""
    for world in range(1, kx.WORLD_MAX + 1):
        for r in range(world):
            lo, hi = -(-r * 256 // world), -(-(r + 1) * 256 // world)
            assert (lo, hi) == (kx.lo_bucket(r, world), kx.lo_bucket(r + 1, world)) and hi > lo
            assert [b for b in range(256) if (b * world) >> 8 == r] == list(range(lo, hi)), (world, r)
            part_lo, n = lo << 11, (hi - lo) << 11
            mul = (1 << 51) // n
            local = ((np.arange(n, dtype=object)) * mul) >> 32 if n <= 4096 else None
            if local is None:  # (exact on uint64: (n - 1) * mul < 2^51)
                local = (np.arange(n, dtype=np.uint64) * np.uint64(mul)) >> np.uint64(32)
            local = np.asarray(local, np.int64)
            assert (np.diff(local) > 0).all() and local[0] == 0 and local[-1] < 1 << 19, (world, r)
            assert kx.part_range(r, world) == (part_lo, part_lo + n)
        assert kx.lo_bucket(world, world) == 256


def test_one_key_one_owner_in_both_modes_and_both_rules_select_the_same(cases):
    for case in cases:
        c = case.ctx()
        assert kx._one_owner(c), "%s: a canonical key with two owners" % case.name
        for (s, i), d in c.subs():
            for r in range(case.world):
                canon, _ = c.t.owned(r, s, i)
                assert np.array_equal(canon, d["canon"][d["dest"] == r]), "%s: sender %d submission %d: the owner's rule of rank %d takes other items than the sender sends it" % (case.name, s, i, r)
    # the direct mode's rule on the item twin's reads, and the item rule on the direct case's
    by = {c.name: c for c in cases}
    a, b = by["epochs_direct_env_n5"].ctx(), by["epochs_item_twin_n5"].ctx()
    assert a.t.whole() == b.t.whole() and a.t.direct and not b.t.direct
    assert [a.t.owner_state(r) for r in range(3)] != [b.t.owner_state(r) for r in range(3)]  # (two different partitions of the keys)


def test_model_summed_over_the_owners_equals_the_oracle_on_every_case(cases):
    for case in cases:
        d, t, hist = case.ctx().t.whole()
        points, totals, ohist = kx.oracle_whole(case)
        assert totals == (sum(d), sum(t)) or case.flow == "ring", case.name
        assert hist == ohist, case.name
        assert kx.points_of(case, d, t) == points, "%s: %s, the oracle's %s" % (case.name, kx.points_of(case, d, t), points)
    assert len(kx.ring_schedule({c.name: c for c in cases}["ring_curve_completes_mid_run"])[1]) == 8


@pytest.mark.parametrize("mutant", sorted(kx.MUTANTS))
def test_mutant_of_the_model_is_told_apart_by_its_case(cases, mutant):
    case = {c.name: c for c in cases}[kx.MUTANTS[mutant]]
    right, wrong = case.ctx().t.observable(), kx.Trace(case, mutant).observable()
    assert right != wrong, "%s: the case %s expects the same from the mutant" % (mutant, case.name)
    if mutant in ("floor_lo_b", "max_epoch"):  # an owner-side mutant: the outboxes are the right ones
        assert right[0] == wrong[0]
    if mutant in ("dest_rounds_up", "outbox_again"):  # a sender-side mutant
        assert right[1] == wrong[1]
