"""trim_plan() (faqcs_amd/csrc/faqcs_trim_plan.h), the one statement of the trim dispatch, without a GPU: tools/trim_plan_check.cpp built
with g++ under AddressSanitizer and UBSan prints the plan of every line it is given, and the plans are held to the rows the GPU suite runs
(tests/trim_dispatch_cases.py: DISPATCH_ROWS), to DESIGN.md section 4 restated in Python (expected_plan) over every length, option class and
switch, to the table's boundaries by name, to the chunk-capacity rule and to the record count.  Nothing here is loaded into the Python process."""
import os
import subprocess

import pytest

import trim_dispatch_cases as td

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_FIELDS = ("kernel", "C", "LPR", "NW", "RPC", "windowed", "ext", "wide_records", "folds_tail", "grid", "records_needed")
MI355X_CU = 256


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("trim_plan") / "trim_plan_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", path,
                        os.path.join(ROOT, "tools", "trim_plan_check.cpp")], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return path


def plans(exe, cases):
    """cases: (options, max_len, n_reads, n_cu, switches) -> the program's plan of each, as dicts."""
    text = "".join(" ".join(str(int(x)) for x in [o[f] for f in td.OPTION_FIELDS] + [max_len, n, n_cu] + [sw[f] for f in td.SWITCH_FIELDS]) + "\n"
                   for o, max_len, n, n_cu, sw in cases)
    r = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"", (r.stdout[-500:] + r.stderr[-2000:]).decode()
    out = [dict(zip(PLAN_FIELDS, [w[0]] + [int(x) for x in w[1:]])) for w in (l.split() for l in r.stdout.decode().splitlines())]
    assert len(out) == len(cases)
    return out


def test_restated_constants_are_the_headers(exe):
    r = subprocess.run([exe, "constants"], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()
    got = {k: int(v) for k, v in (l.split() for l in r.stdout.decode().splitlines())}
    assert got == {"FAQCS_FAST_READ_LENGTH": td.FAST_READ_LENGTH, "FAQCS_PARTIAL_FLUSHES": td.PARTIAL_FLUSHES, "FAQCS_TRIM_NW": td.TRIM_NW,
                   "FAQCS_TRIM_LONG_NW": td.TRIM_LONG_NW, "FAQCS_LDS16_RPC": td.LDS16_RPC}


def test_the_rows_the_gpu_suite_runs(exe):
    """test_dispatcher_picks_the_documented_trim_kernel's rows (300 reads of L bases, on an MI355X's 256 compute units): the plan names the same kernel."""
    got = plans(exe, [(td.option_fields(args), L, 300, MI355X_CU, td.DEFAULT_SWITCHES) for L, args, _ in td.DISPATCH_ROWS])
    assert [p["kernel"] for p in got] == [kernel for _, _, kernel in td.DISPATCH_ROWS]


OPTION_CLASSES = {
    "default": {}, "default, records pending": dict(fold_n=300), "--adapter": dict(has_adapters=1, fold_n=300), "--qc_only": dict(qc_only=1, fold_n=300),
    "--5trim_off": dict(protect5=1, fold_n=300), "--mode HARD": dict(mode=td.MODE_HARD, fold_n=300), "--mode BWA": dict(mode=td.MODE_BWA, fold_n=300),
    "--avg_q": dict(avgq_on=1, fold_n=300), "-n 1": dict(max_poly_n=1, fold_n=300), "--replace_to_N_q": dict(replace_q=15, fold_n=300),
    "FAQCS_DBG": dict(dbg=2, fold_n=300), "--5end": dict(trim5=3, fold_n=300), "--3end --qc_only": dict(trim3=5, qc_only=1, fold_n=300),
}
SWITCH_SETS = {"all on": {}, "FAQCS_TRIM_LONG=1": dict(force_long=1), "FAQCS_TRIM_LDS=0": dict(lds_on=0), "FAQCS_TRIM_LDS4=0": dict(lds4_on=0),
               "FAQCS_TRIM_LDS16=0": dict(lds16_on=0)}


@pytest.mark.parametrize("switches", list(SWITCH_SETS))
def test_whole_plan_against_the_restated_table(exe, switches):
    """Every longest read from 0 to 1 100 bases and 32 767, every option class: kernel, shape, both flags, wide_records, folds_tail, grid and record count."""
    sw = dict(td.DEFAULT_SWITCHES, **SWITCH_SETS[switches])
    cases = [(dict(td.DEFAULT_OPTIONS, **o), L, 300, MI355X_CU, sw) for o in OPTION_CLASSES.values() for L in list(range(1101)) + [32767]]
    names = [(name, L) for name in OPTION_CLASSES for L in list(range(1101)) + [32767]]
    for who, got, case in zip(names, plans(exe, cases), cases):
        assert got == td.expected_plan(*case), who


# DESIGN.md section 4 by its boundaries, default options, every switch on: (the two neighbouring lengths) -> (kernel, C, lanes per read) on either side
BOUNDARIES = {
    (52, 53): (("trim_lds", 13, 4), ("trim_lds", 19, 4)), (76, 77): (("trim_lds", 19, 4), ("trim_lds", 13, 8)), (104, 105): (("trim_lds", 13, 8), ("trim_lds", 19, 8)),
    (152, 153): (("trim_lds", 19, 8), ("trim_lds", 16, 16)), (252, 253): (("trim_lds", 16, 16), ("trim_lds", 19, 16)), (256, 257): (("trim_lds", 19, 16), ("trim_lds", 19, 16)),
    (304, 305): (("trim_lds", 19, 16), ("trim_filter_accumulate", 10, 32)), (320, 321): (("trim_filter_accumulate", 10, 32), ("trim_filter_accumulate", 16, 32)),
    (512, 513): (("trim_filter_accumulate", 16, 32), ("trim_filter_accumulate", 12, 64)), (768, 769): (("trim_filter_accumulate", 12, 64), ("trim_filter_accumulate", 16, 64)),
    (1024, 1025): (("trim_filter_accumulate", 16, 64), ("trim_long", 0, 0)),
}


@pytest.mark.parametrize("pair", list(BOUNDARIES), ids=lambda p: "%d/%d" % p)
def test_table_boundary(exe, pair):
    got = plans(exe, [(td.DEFAULT_OPTIONS, L, 300, MI355X_CU, td.DEFAULT_SWITCHES) for L in pair])
    assert tuple((p["kernel"], p["C"], p["LPR"]) for p in got) == BOUNDARIES[pair]
    assert [p["wide_records"] for p in got] == [int(256 < L <= 1024) for L in pair]  # (the 256/257 boundary moves nothing else)
    assert [p["records_needed"] for p in got] == [151 if L > 1024 else 600 if L > 256 else 300 for L in pair]


@pytest.mark.parametrize("n_cu", [1, 256])
@pytest.mark.parametrize("row", td.LDS_ROWS, ids=lambda r: "%d...%d" % r[:2])
def test_chunk_capacity_rule(exe, row, n_cu):
    """A block of trim_lds has 8 flush rows, one per 65 535 // RPC reads of each of its NW waves' chunks (a multiple of NW chunks), and the plan
    fills three quarters of them: the largest submission that stays with trim_lds, and one chunk more, which trim_filter_accumulate takes in the
    shape of the same length's row."""
    lo, hi, C, LPR, RPC, NW, _ = row
    limit = n_cu * 8 * (65535 // RPC // NW * NW) * 3 // 4  # chunks
    for L in (lo, hi):
        stays, moves = plans(exe, [(td.DEFAULT_OPTIONS, L, n, n_cu, td.DEFAULT_SWITCHES) for n in (limit * RPC, limit * RPC + RPC)])
        assert (stays["kernel"], stays["C"], stays["LPR"], stays["RPC"], stays["NW"], stays["grid"]) == ("trim_lds", C, LPR, RPC, NW, n_cu)
        tfa = [r for r in td.TFA_ROWS if L <= r[0]][0]
        assert (moves["kernel"], moves["C"], moves["LPR"], moves["NW"], moves["RPC"], moves["folds_tail"]) == ("trim_filter_accumulate", tfa[1], tfa[2], tfa[3], 0, 0)
        assert moves == td.expected_plan(td.DEFAULT_OPTIONS, L, limit * RPC + RPC, n_cu, td.DEFAULT_SWITCHES)


def test_records_needed(exe):
    """n // 2 + 1 words for trim_long (its scratch), two per read past 256 bases, else one."""
    ns = [1, 2, 63, 64, 65, 299, 300, 4097, 1 << 20, 100000001]
    cases = [(dict(td.DEFAULT_OPTIONS, **o), L, n, MI355X_CU, dict(td.DEFAULT_SWITCHES, **sw)) for n in ns for L in (1, 150, 256, 257, 304, 305, 1024, 1025, 32767)
             for o in ({}, dict(replace_q=15)) for sw in ({}, dict(force_long=1), dict(lds_on=0))]
    for got, (o, L, n, _, sw) in zip(plans(exe, cases), cases):
        long_reads = got["kernel"] == "trim_long"
        assert long_reads == (L > 1024 or bool(sw["force_long"]))
        assert got["wide_records"] == int(L > 256 and not long_reads)
        assert got["records_needed"] == (n // 2 + 1 if long_reads else 2 * n if got["wide_records"] else n), (L, n, o, sw)
