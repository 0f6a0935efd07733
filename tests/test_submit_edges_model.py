"""The catalogue of tests/submit_edges.py without a GPU: every edge is reached and no schedule is left out of the GPU test's lists; the
restated constants equal the sources; the plan trace() assumes for every submission is what tools/trim_plan_check.cpp prints (built
stand-alone with g++ under AddressSanitizer and UBSan, as tests/test_trim_plan.py builds it); the oracle's block for a schedule is the sum
of the blocks of its submissions taken alone, resets honoured -- the additivity the expectations rest on; mutated traces lose edges; and the
host arenas put decisive bytes directly around every window."""
import os
import re

import numpy as np
import pytest

import submit_edges as se
from test_trim_plan import exe, plans  # noqa: F401  (exe: the module-scoped fixture that builds tools/trim_plan_check.cpp)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def schedules():
    return se.all_schedules()


def test_every_edge_is_reached_and_no_schedule_is_left_out(schedules):
    assert len({s.name for s in schedules}) == len(schedules), "two schedules share a name"
    table, per = se.coverage(schedules)
    missing = sorted(e for e, v in table.items() if not v)
    assert not missing, "edges no schedule reaches: %s" % missing
    assert len(table) >= 90
    idle = sorted(n for n, h in per.items() if not h)
    assert not idle, "schedules that reach no edge: %s" % idle
    # the lists tests/test_gpu_submit_edges.py runs: every (family, setting) pair that has schedules, and nothing else
    ran = {s.name for f in se.FAMILIES for st in se.SETTINGS for s in se.schedules_of(f, st, schedules)}
    assert ran == {s.name for s in schedules} and {s.family for s in schedules} == set(se.FAMILIES) and {s.setting for s in schedules} == set(se.SETTINGS)
    assert all(s.setting == "single_pass" for s in se.schedules_of("single_pass", "single_pass", schedules)) and se.schedules_of("single_pass", "single_pass", schedules)
    assert not [s.name for s in schedules if s.setting == "single_pass" and s.family != "single_pass"]
    # no k-mer option anywhere (the k-mer state across submissions has catalogues of its own)
    assert not any(s.opt().kmer_rarefaction for s in schedules)


def test_sizes_and_shapes_of_the_catalogue(schedules):
    """Reads of at most 304 bases but where an edge needs more; but for the schedule under load, no batch is larger than the 65 537 reads of 30 bases"""
    for s in schedules:
        longest = max(b.longest for b in s.batches)
        assert longest <= 304 or s.name in ("aux_folder_tfa_length", "aux_folder_trim_long"), s.name
        under_load = s.name == "host_ring_under_load"  # (sized so that the device falls behind the host: sixteen times the same 200 000 reads)
        assert under_load or (max(b.n for b in s.batches) <= 65537 and s.n_reads() < 200000), s.name
        assert s.ops[-1][0] in ("finish", "expect_error")


def test_every_arm_of_the_tallies_is_predicted_somewhere(schedules):
    seen = dict.fromkeys(se.TALLIES, 0)
    for s in schedules:
        for k, v in se.trace(s).tallies.items():
            seen[k] += v
    assert all(seen.values()), seen


def test_restated_constants_equal_the_sources():
    for name, places in se.CONSTANT_SOURCES.items():
        for path, rx, value in places:
            m = re.search(rx, open(os.path.join(ROOT, path)).read())
            assert m, "%s: %s no longer states it as %r" % (name, path, rx)
            assert value(m.groups()) == getattr(se, name), (name, path, rx)
    assert set(se.CONSTANT_SOURCES) == {"RING", "N_SLOTS", "N_RECSETS", "FOLD_U", "PER_CLAIM", "CELL_MAX", "PAD_BEFORE", "PAD_AFTER", "STAGE_FRONT", "TN_SLACK",
                                        "RESERVE_DIV", "RESERVE_ADD"}
    # the FLUSH_CLAIMS formula at the folding launch of the fold_n schedules: NT = 768 threads, chunks of 3 072 records, a flush every 4 claims
    assert se.fold_geometry(se.FOLDER_NW) == (3072, 61440) and se.CELL_MAX // (3072 * se.PER_CLAIM) == 4
    # the tallies' names are the structure's fields, in order, in the header and in the ctypes view
    from faqcs_amd import _capi as capi

    hdr = open(os.path.join(ROOT, "include", "faqcs_mi.h")).read()
    body = re.search(r"typedef struct faqcs_path_tallies \{(.*?)\} faqcs_path_tallies;", hdr, re.S).group(1)
    assert tuple(re.findall(r"uint64_t (\w+);", body)) == se.TALLIES == tuple(n for n, _ in capi.PathTallies._fields_)
    assert (se.E_INVAL, se.E_QUALITY, se.F_ERR_QUALITY) == (capi.E_INVAL, capi.E_QUALITY, capi.F_ERR_QUALITY)


def test_the_plans_trace_assumes_are_the_plans_of_trim_plan(exe, schedules):  # noqa: F811
    """kernel, NW, grid, wide_records, folds_tail, records_needed (and the rest of the plan) of every submission of every schedule, with the
    fold_n the trace offers it; the folding launch of every fold_n schedule has ONE block of FOLDER_NW waves."""
    queries = [q for s in schedules for q in se.trace(s).plan_queries]
    assert len(queries) >= 250
    got = plans(exe, [q[:5] for q in queries])
    for q, g in zip(queries, got):
        assert g == q[5], q[:5]
    assert {g["kernel"] for g in got} == {"trim_lds", "trim_filter_accumulate", "trim_long"} and {g["folds_tail"] for g in got} == {0, 1}
    for s in schedules:
        if s.family == "tail_n":
            w, f = se.trace(s).subs
            assert (f["kernel"], f["grid"], f["NW"], f["fold"], f["folds_tail"]) == ("trim_lds", 1, se.FOLDER_NW, "tail", True) and f["n"] <= f["RPC"], s.name
            assert f["fold_n"] == w["n"] == se.fold_n_value(s.name[len("tail_fold_n_"):], f["NW"])
        if s.family == "tail_big":
            w, f = se.trace(s).subs
            assert f["fold"] == "tail" and f["NW"] == se.FOLDER_NW and f["grid"] >= 16 and f["n"] // f["RPC"] >= 300


@pytest.mark.parametrize("family", [f for f in se.FAMILIES if f != "error"])
def test_the_oracle_block_is_the_sum_of_the_submissions_alone(schedules, family):
    for s in [x for x in schedules if x.family == family]:
        e, alone = s.expected(), se.expected(s, alone=True)
        assert e["error"] is None and sorted(e["blocks"]) == sorted(alone["blocks"]) and e["blocks"]
        for at in e["blocks"]:
            bad = np.nonzero(e["blocks"][at] != alone["blocks"][at])[0]
            assert len(bad) == 0, "%s, operation %d: %d counters differ, first %d" % (s.name, at, len(bad), bad[0])
        for a, b in zip(e["results"], alone["results"]):
            assert (a == b).all()
        # a reset leaves nothing of what came before it: the block behind the last reset is the sum of the later submissions alone
        resets = [i for i, op in enumerate(s.ops) if op[0] == "reset"]
        if resets and not any(op[0] == "import" for op in s.ops):
            last = max(e["blocks"])
            later = [b for i, b in zip([i for i, op in enumerate(s.ops) if op[0] == "submit"], s.batches) if resets[-1] < i < last]
            n_later = sum(b.n for b in later)
            assert int(e["blocks"][last][0]) == n_later  # (FilterStat TOTAL_COUNT is the block's first word)


def test_the_error_schedule(schedules):
    (s,) = [x for x in schedules if x.family == "error"]
    e = s.expected()
    j, code = e["error"]
    assert code == se.E_QUALITY and 0 < j < 4 and all(r is not None for r in e["results"][:j]) and e["results"][j] is None
    b = s.batches[j]
    at = int(b.kind.split()[-1])
    q = b.qual[b.offset[at]:b.offset[at + 1]]
    assert q[3] == ord("~") and int((b.qual > 41 + 33).sum()) == 1  # one score above 41 in the whole schedule, in that read


@pytest.mark.parametrize("mutation,edges", [
    (dict(ring=4), ["host: ticket + 8 == n_submits", "host: 8 submissions without a wait"]),
    (dict(n_slots=1), ["host: slot 1 reused with equal size", "host: slot 1 regrown with its kernels in flight", "host: slot 1 reused with a smaller batch"]),
    (dict(pending_on=False), ["tail: fold_n = F+1, a folding launch of one chunk (grid 1)", "aux: a record set reused at k+2 while its fold may still run (the wait for `folded`)",
                              "now: the last launch's records folded by export", "dropped: reset behind an aux fold that may still run",
                              "aux: two-word records beside a launch that writes one-word ones"]),
])
def test_a_mutated_trace_loses_edges(schedules, mutation, edges):
    """The predicates look at the trace: with a ring of 4, with one slot, with a fold that is never pending, edges go unreached and the
    predicted tallies change."""
    table, _ = se.coverage(schedules)
    mutated, _ = se.coverage(schedules, **mutation)
    lost = sorted(e for e in table if table[e] and not mutated[e])
    assert lost, mutation
    if "ring" in mutation:  # (a ring of 4 moves the ticket cases: what was the boundary is a recycled event, and the ring wraps earlier)
        assert "host: ticket + 8 == n_submits" in lost or table["host: ticket + 8 == n_submits"] != mutated["host: ticket + 8 == n_submits"]
        assert sum(se.trace(s, **mutation).tallies["ticket_ring_waits"] for s in schedules) > sum(se.trace(s).tallies["ticket_ring_waits"] for s in schedules)
    else:
        assert not [e for e in edges if e not in lost], [e for e in edges if e not in lost]
    assert any(se.trace(s, **mutation).tallies != se.trace(s).tallies for s in schedules)


def test_decisive_bytes_stand_around_every_window(schedules):
    """An N and a quality above 41 directly in front of (where there is a front) and behind every window of a host arena, and around the
    arenas of a device-resident batch; the window itself is the batch."""
    for s in schedules:
        for b in s.batches:
            seq, qual, off = b.host_arenas()
            assert int(off[0]) == b.o0 and int(off[-1]) == b.o0 + b.total and len(seq) >= b.o0 + b.total + se.PAD_AFTER
            assert (seq[b.o0:b.o0 + b.total] == b.seq).all() and (qual[b.o0:b.o0 + b.total] == b.qual).all()
            assert seq[b.o0 + b.total] == se.N and qual[b.o0 + b.total] == se.HOSTILE_Q > 41 + max(33, s.in_off, 64)
            assert b.o0 == 0 or (seq[b.o0 - 1] == se.N and qual[b.o0 - 1] == se.HOSTILE_Q)
            dseq, dqual, front = b.device_arenas()
            assert front >= se.PAD_BEFORE and len(dseq) - front - b.total >= se.PAD_AFTER and dseq[front - 1] == se.N and dqual[front + b.total] == se.HOSTILE_Q
            assert (b.terminal_n() <= 3).all() and len(b.terminal_n()) == b.n
