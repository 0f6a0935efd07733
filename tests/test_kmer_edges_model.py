"""The catalogue of tests/kmer_edges.py without a GPU: its restated constants against the sources, its coverage table (every edge claimed,
every claim of a case true), its plain model against the oracle on every case -- alone on a fresh engine and as the consecutive passes
tests/test_gpu_kmer_edges.py runs --, and every window of the catalogue through the emulated extraction lanes of tests/skm_model.cpp
(file mode), which also holds the Python restatement of skm_ord / skm_part to faqcs_skm.h."""
import os
import re
import subprocess

import pytest

import kmer_edges as ke
from faqcs_amd import driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return ke.all_cases()


def test_restated_constants_equal_the_sources():
    csrc = os.path.join(ROOT, "faqcs_amd", "csrc")
    for name, (fn, rx) in ke.CONSTANT_SOURCES.items():
        m = re.search(rx, open(os.path.join(csrc, fn)).read())
        assert m, "%s: %s no longer states it as %r" % (name, fn, rx)
        v = int(m.group(1))
        assert getattr(ke, name) == (1 << v if name == "DENSE_N" else v), name
    skm = open(os.path.join(csrc, "faqcs_kmer_skm_kernel.hip")).read()
    ls, limit = re.search(r"constexpr int LS = (\d+),", skm), re.search(r"LIMIT = LS - (\d+);", skm)
    assert ls and limit and int(ls.group(1)) == ke.LDS_SLOTS and ke.LDS_SLOTS - int(limit.group(1)) == ke.LDS_ROUND_KEYS
    assert [ke.skm_geom(k) for k in (2, 15, 16, 31)] == [(2, 1), (15, 1), (15, 2), (15, 17)]


def test_every_edge_is_claimed_and_every_claim_holds(cases):
    assert len({c.name for c in cases}) == len(cases), "two cases share a name"
    table, lost = ke.coverage(cases)
    assert not lost, "claims that do not hold: %s" % lost
    missing = sorted(e for e, v in table.items() if not v)
    assert not missing, "edges no case claims: %s" % missing
    assert len(table) >= 110 and all(e in ke.EDGES for c in cases for e in c.claims)
    assert {c.family for c in cases} == set(ke.FAMILIES)
    assert sorted(c.name for r in ke.engine_runs(cases) for c in r if len(r) != 2 or r[0].name not in ke.TWO_PASSES) == sorted(c.name for c in cases)


def oracle_pass(ora, m, case):
    """One pass of a case on an oracle engine and a model engine side by side: active after every submission, points and totals where the
    case asks for them on the way, points, totals and the histogram at its end."""
    for sub in case.subs:
        res = ora.process(*driver.pack_segments(sub))
        m.submit(sub, res)
        assert ora.kmer_active() == m.active, case.name
        if case.ask:
            assert [tuple(int(x) for x in p) for p in ora.kmer_points()] == m.points and ora.kmer_totals() == m.totals(), case.name
    assert ora.kmer_totals() == m.totals(), case.name
    ora.kmer_end_table()
    m.end_table()
    assert [tuple(int(x) for x in p) for p in ora.kmer_points()] == m.points, case.name
    c, n = ora.kmer_histogram()
    assert list(zip(c.tolist(), n.tolist())) == m.histogram(), case.name
    assert ora.kmer_active() == m.active, case.name


def test_model_equals_oracle_on_every_case_alone(cases):
    from oracle_engine import OracleEngine

    for case in cases:
        ora, m = OracleEngine(case.opt(), ke.MAX_READ, ke.IN_OFF), ke.Model(case.opt())
        oracle_pass(ora, m, case)
        ora.close()
        e = case.ctx().expected  # what model(case) says: the same run
        assert (e["points"], e["hist"], e["active"]) == (m.points, m.histogram(), m.active), case.name


def test_model_equals_oracle_on_consecutive_passes_of_one_engine(cases):
    from oracle_engine import OracleEngine

    runs = [r for r in ke.engine_runs(cases) if len(r) > 1]
    assert len(runs) >= 8 and [[c.name for c in r] for r in runs[:2]] == [list(ke.TWO_PASSES), list(ke.TWO_PASSES)[::-1]]
    for run in runs:
        ora, m = OracleEngine(run[0].opt(), ke.MAX_READ, ke.IN_OFF), ke.Model(run[0].opt())
        for case in run:
            assert m.active, "%s: the curve of its engine is complete before it starts" % case.name
            oracle_pass(ora, m, case)
        ora.close()


def test_twin_cases_of_the_two_extraction_kernels_expect_the_same(cases):
    by = {c.name: c for c in cases}
    a, b = by["short_reads_16_byte_kernel"].ctx().expected, by["short_reads_general_kernel"].ctx().expected
    assert a["hist"] == b["hist"] and a["totals"] == b["totals"] and a["totals"][1] > 500


# ---- the catalogue's windows through the emulated lanes --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes(cases, tmp_path_factory):
    """-> [(case name, k, effective window, output fields of skm_model --file)] for every distinct counted window of the catalogue"""
    d = tmp_path_factory.mktemp("skm_file")
    exe, path = str(d / "skm_model"), str(d / "windows.txt")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "skm_model.cpp")])
    rows, seen = [], set()
    with open(path, "w") as f:
        for case in cases:
            c = case.ctx()
            for w in c.wins:
                s, q, a, n = w
                if (s, q, a, n, c.k, c.rq) in seen:
                    continue
                seen.add((s, q, a, n, c.k, c.rq))
                eff = c.eff(w)
                mask = "".join("1" if x != y else "0" for x, y in zip(s[a:a + n], eff))
                f.write("%s %d %d %d %s\n" % (s.hex() or "-", a, n, c.k, ("0" * a + mask + "0" * (len(s) - a - n)) if "1" in mask else "-"))
                rows.append((case.name, c.k, eff))
    out = subprocess.run([exe, "--file", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1].startswith("ok: %d reads" % len(rows))
    return [r + ([int(x) for x in ln.split()],) for r, ln in zip(rows, lines)]


def test_catalogue_windows_through_the_emulated_lanes(lanes):
    """skm_model has checked keys as a multiset, <= w k-mers per item and one partition per canonical k-mer; here: the k-mer count equals the
    model's, the partitions equal the Python restatement's for every k-mer, and skm_extract16 defers exactly the reads with a run beyond 17."""
    assert len(lanes) > 1500
    tried = 0
    for i, (name, k, eff, (line, k2, deferred, longest, total, part_sum)) in enumerate(lanes):
        assert (line, k2) == (i, k)
        assert total == len(ke.canonical_kmers([eff], k)), name
        want = sum(int(ke.skm_part(ke.min_ords(eff[s:s + n], k)).sum()) for s, n in ke.stretches(eff) if n >= k)
        assert part_sum == want, "%s: skm_ord / skm_part of tests/kmer_edges.py differ from faqcs_skm.h" % name
        run = ke.longest_run(eff, k)
        assert longest <= ke.skm_geom(k)[1] and (run == 0) == (longest == 0), name
        assert (deferred >= 0) == (k == 31 and len(eff) <= 256), name
        if deferred >= 0:
            tried += 1
            assert deferred == (run > ke.SKM_W_MAX), "%s: a longest run of %d k-mers and deferred = %d" % (name, run, deferred)
            assert deferred or longest == run, name
    assert tried > 300


@pytest.mark.parametrize("n,deferred", [(16, 0), (17, 0), (18, 1), (35, 1)])
def test_run_length_cases_are_deferred_as_claimed(lanes, n, deferred):
    got = [(f[2], f[3]) for name, k, eff, f in lanes if name == "run_of_%d_k31" % n and ke.longest_run(eff, 31) == n]
    assert got and all(d == deferred and (longest == n if not deferred else longest <= 17) for d, longest in got), got
