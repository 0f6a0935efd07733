"""The trim dispatch, stated for the tests: the (longest read, options, kernel) rows that tests/test_gpu_parity.py runs on the device and
tests/test_trim_plan.py holds trim_plan() to without one, and DESIGN.md section 4's table restated in Python -- expected_plan() -- the way
tests/pack_edges.py restates the pack constants.  Plain Python: no GPU, no ctypes, nothing of the library at import."""
from faqcs_amd.options import parse_args

# (L, command-line options, kernel): 300 reads of L bases each
DISPATCH_ROWS = [
    (150, [], "trim_lds"), (151, ["--adapter"], "trim_lds"), (100, ["--mode", "HARD", "-q", "10"], "trim_lds"), (125, ["--qc_only"], "trim_lds"),
    (128, [], "trim_lds"), (96, [], "trim_lds"), (75, [], "trim_lds"), (160, [], "trim_lds"), (157, ["--5trim_off"], "trim_lds"), (64, [], "trim_lds"), (50, ["--adapter"], "trim_lds"), (36, ["--mode", "BWA"], "trim_lds"),
    (75, ["--replace_to_N_q", "15"], "trim_filter_accumulate"),
    (150, ["--replace_to_N_q", "15"], "trim_filter_accumulate"), (128, ["--qc_only"], "trim_lds"), (192, ["--adapter"], "trim_lds"),
    (250, [], "trim_lds"), (251, ["--adapter", "--polyA"], "trim_lds"), (200, ["--mode", "BWA", "--avg_q", "20"], "trim_lds"), (161, [], "trim_lds"), (252, [], "trim_lds"),
    (253, [], "trim_lds"), (224, [], "trim_lds"), (256, [], "trim_lds"), (250, ["--replace_to_N_q", "15"], "trim_filter_accumulate"),
    (300, [], "trim_lds"), (301, ["--adapter", "--polyA"], "trim_lds"), (304, ["--mode", "HARD", "-q", "10"], "trim_lds"), (305, [], "trim_filter_accumulate"),
    (300, ["--replace_to_N_q", "15"], "trim_filter_accumulate"),
]

# ---- the constants behind the table, restated (test_trim_plan.py compares them with the header's) ------------------------------------------
FAST_READ_LENGTH = 1024     # longest read of the chunked kernels
PARTIAL_FLUSHES = 8         # flush rows of a trim_lds block
TRIM_NW = 4                 # waves per block of trim_filter_accumulate (the 1 024-wide shape: 8)
TRIM_LONG_NW = 4
LDS16_RPC = 32
MODE_HARD, MODE_BWA, MODE_BWA_PLUS = 0, 1, 2
FOLD_TABLE_DWORDS = (10001 * 6 + 1) // 2 + 512 + 8  # what a block needs to fold composition records: the table, the per-length factors, the claim words

OPTION_FIELDS = ("mode", "protect5", "qc_only", "replace_q", "avgq_on", "max_poly_n", "dbg", "has_adapters", "trim5", "trim3", "fold_n")
DEFAULT_OPTIONS = dict(mode=MODE_BWA_PLUS, protect5=0, qc_only=0, replace_q=0, avgq_on=0, max_poly_n=2, dbg=0, has_adapters=0, trim5=0, trim3=0, fold_n=0)
SWITCH_FIELDS = ("force_long", "lds_on", "lds4_on", "lds16_on")
DEFAULT_SWITCHES = dict(force_long=0, lds_on=1, lds4_on=1, lds16_on=1)

# trim_lds, DESIGN.md section 4: (first length, last length, C, lanes per read, reads per chunk, waves per block, switch that must be on)
LDS_ROWS = [(1, 52, 13, 4, 64, 12, "lds4_on"), (53, 76, 19, 4, 64, 12, "lds4_on"), (77, 104, 13, 8, 64, 12, None), (105, 152, 19, 8, 64, 12, None),
            (153, 252, 16, 16, LDS16_RPC, 12, "lds16_on"), (253, 304, 19, 16, 20, 12, "lds16_on")]
# trim_filter_accumulate: (last length, C, lanes per read, waves per block, compiled variants: 4 = every (WINDOWED, GENERIC) pair, 2 = both or neither, 1 = both)
TFA_ROWS = [(64, 16, 4, TRIM_NW, 4), (76, 19, 4, TRIM_NW, 4), (104, 13, 8, TRIM_NW, 4), (128, 16, 8, TRIM_NW, 4), (152, 19, 8, TRIM_NW, 4), (160, 20, 8, TRIM_NW, 4),
            (208, 13, 16, TRIM_NW, 4), (256, 16, 16, TRIM_NW, 4), (320, 10, 32, TRIM_NW, 4), (512, 16, 32, TRIM_NW, 2), (768, 12, 64, TRIM_NW, 1), (1024, 16, 64, 8, 1)]


def option_fields(args):
    """The TrimOptions of a command line (fold_n = 0), as faqcs_create() fills DevParams from the options."""
    o = parse_args(["-u", "x", "-d", "y"] + args)
    return dict(DEFAULT_OPTIONS, mode=o.mode, protect5=int(o.protect_5), qc_only=int(o.qc_only), replace_q=o.replace_to_N_q, avgq_on=int(o.average_quality > 0),
                max_poly_n=o.max_num_poly_N, has_adapters=int(bool(o.adapter) and o.adapters_active()), trim5=o.trim_5, trim3=o.trim_3)


def row_dwords(C, LPR, WQ=0):
    """LDS dwords of the accumulators and tables of a <C, LPR> row (RowCfg): quality matrix, base matrix, length and quality histograms, filter
    slots; then the base table, three per-length tables and the byte masks."""
    W = LPR * C
    hq = 42 * W // 2 if W > 768 else 42 * (WQ or W)
    n_zero = hq + 5 * W + (W + 2) + 3 * 42 + 32
    return ((n_zero + 256 + 3 * (W + 1) + 3) & ~3) + (4 if (C + 3) // 4 <= 4 else 8) * (C + 2)


def lds_block_dwords(C, LPR, RPC, NW):
    """LDS dwords of a trim_lds block (LdsCfg): the row, two 256 x 2 tables, the chunk queue, Q-B's rotated masks, a staging slot per wave, the tail."""
    cq = 20 if C == 19 else C
    qstride = cq + 1 if LPR == 16 else cq
    wq = (LPR * qstride + 31) // 32 * 32 if (LPR == 16 or C == 19) else 0
    nrot = 2 if LPR == 16 else (4 if C == 19 else 1)
    W, maxlen = LPR * C, lds_maxlen(C, LPR)
    o_stg = ((row_dwords(C, LPR, wq) + 3) & ~3) + 512 + 512 + 8 + (nrot * (cq + 1) * 8 if nrot > 1 else 0)
    stg_bytes = RPC * max(maxlen // 32 * 32 + 16, maxlen) + 32
    return o_stg + NW * ((stg_bytes + 15) // 16 * 4) + ((W + 64) // 4 if W + 64 > 256 else 64)


def lds_maxlen(C, LPR):
    return 252 if LPR * C == 256 else LPR * C


def lds_chunk_limit(n_cu, RPC, NW):
    """Chunks the blocks of a trim_lds launch that fills the device take between them: three quarters of 8 flush rows of 65 535 // RPC reads-per-cell each."""
    return n_cu * PARTIAL_FLUSHES * (65535 // RPC // NW * NW) * 3 // 4


def expected_plan(o, max_len, n_reads, n_cu, sw):
    """DESIGN.md section 4 as a function: the fields tools/trim_plan_check prints, as a dict."""
    ceil = lambda a, b: (a + b - 1) // b
    if max_len > FAST_READ_LENGTH or sw["force_long"]:
        return dict(kernel="trim_long", C=0, LPR=0, NW=TRIM_LONG_NW, RPC=0, windowed=0, ext=0, wide_records=0, folds_tail=0,
                    grid=min(ceil(n_reads, TRIM_LONG_NW), 8 * n_cu), records_needed=n_reads // 2 + 1)
    wide = int(max_len > 256)
    windowed = int(bool(o["has_adapters"] or ((o["trim5"] or o["trim3"]) and not o["qc_only"])))
    headline = (o["mode"] == MODE_BWA_PLUS and not o["protect5"] and not o["qc_only"] and not o["replace_q"] and not o["avgq_on"] and o["max_poly_n"] == 2
                and not o["dbg"])
    p = dict(windowed=windowed, ext=int(not headline), wide_records=wide, folds_tail=0, records_needed=n_reads * (2 if wide else 1), RPC=0)
    if sw["lds_on"] and not o["replace_q"] and not o["dbg"]:
        for lo, hi, C, LPR, RPC, NW, switch in LDS_ROWS:
            if lo <= max_len <= hi and (switch is None or sw[switch]):
                chunks = ceil(n_reads, RPC)
                grid = min(ceil(chunks, NW), n_cu)
                if chunks <= lds_chunk_limit(grid, RPC, NW):
                    folds = lds_block_dwords(C, LPR, RPC, NW) >= FOLD_TABLE_DWORDS and lds_maxlen(C, LPR) <= 256
                    return dict(p, kernel="trim_lds", C=C, LPR=LPR, NW=NW, RPC=RPC, grid=grid, folds_tail=int(folds and o["fold_n"] != 0))
    for hi, C, LPR, NW, variants in TFA_ROWS:
        if max_len <= hi:
            if variants == 2:
                p["windowed"] = p["ext"] = p["windowed"] | p["ext"]
            if variants == 1:
                p["windowed"] = p["ext"] = 1
            minwaves = 2 if (LPR == 8 or C > 10) else 3
            per_cu = max(1, min(160 * 1024 // (4 * row_dwords(C, LPR)), ceil(4 * minwaves, NW)))
            return dict(p, kernel="trim_filter_accumulate", C=C, LPR=LPR, NW=NW, grid=min(ceil(ceil(n_reads, 64), NW), n_cu * per_cu))
    raise AssertionError("no row for %d bases" % max_len)
