"""A constructed catalogue of inputs for trim_filter_accumulate and composition_histogram (faqcs_trim_kernel.hip; flush_block and flush_hq8 of
faqcs_trim_common.h), in the style of tests/trim_long_edges.py.  The plain model (Model), TCase, layout, the read helpers and the threshold
searches come from tests/trim_edges.py, whose registry, table and times stand: this catalogue has an edge registry of its own.  What only
this kernel has is aimed at here: its twelve shapes <C, LPR, NW> and their compiled (WINDOWED, GENERIC) variants, the lane borders m C - 1 |
m C of each shape's OWN C (and the DPP row borders of the 32- and 64-lane shapes), the tails of its unaligned multi-dword loads and the
prefetched next read, the register-privatised base counts in 6-bit fields with their spill schedule, the 8-bit cells of the 1 024-wide
shape, the PAST_END correction of flush_block, --replace_to_N_q, and the rounds of composition_histogram.

Every case is a named builder of submissions of segments of reads, every edge a PREDICATE over a case's reads and the model's per-read
trace, never over a case's name; coverage() puts every predicate to every case.  The builders take n_cu, the compute units the grids are
capped by; shapes, per_cu, grids and variants come from tests/trim_dispatch_cases.py (TFA_ROWS, expected_plan).

A submission of millions of reads is a Tiled one: a period of distinct reads, a number of repeats and a remainder.  The model runs on the
period and on the remainder once; every counter is a sum over reads, so the expected block is repeats x block(period) + block(remainder)
(tests/test_trim_tfa_edges_model.py states and tests that identity at a small size).

lanes(case): a second model, which restates the LANEWISE structure of the kernel for the case's shape -- per-lane Pin, E and T with its
correction for the slots past the read, the reset bits with next / prev across lanes, lane-local argmax keys with JB / PB / KEY_BIAS, the
pair logic of poly-N, cls with prev_last, the edit bits -- and, for the counters, the schedule of the 6-bit fields, the 8-bit cells, the
`shorter` correction and the rounds of composition_histogram as the largest value a field takes between two flushes.  Unmutated it equals
the plain model; MUTANTS are wrong versions of it, each told apart by a named case.

The window family -- a built-in adapter's window in front of this kernel's walk -- has OracleEngine as its reference, whole results and the whole
counter block, because the model covers no adapters.

    python -m tests.trim_tfa_edges        prints the table, the sizes per family, the mutants and the exclusions
"""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import trim_edges as te
from trim_dispatch_cases import DEFAULT_SWITCHES, FAST_READ_LENGTH, TFA_ROWS, expected_plan, option_fields
from trim_edges import (F_POLY_N_SEEN, F_QUAL_TRIMMED, F_VALID, FILT_LENGTH_PRE, FILT_LOW_COMPLEXITY, FILT_NONE, FILT_POLY_N, MODE_BWA, MODE_BWA_PLUS, MODE_HARD,
                        Model, Qs, TCase, f32, lc_thr, rb, rd)

KERNEL, COMMON, PLAN = "faqcs_amd/csrc/faqcs_trim_kernel.hip", "faqcs_amd/csrc/faqcs_trim_common.h", "faqcs_amd/csrc/faqcs_trim_plan.h"
# restated; test_trim_tfa_edges_model.py holds each to its source by regex (a tuple: the regex's groups in order)
REG_FLUSH_EVERY = {16: 3, 8: 7, 4: 15, 32: 1, 64: 1}    # iterations between two spills of the 6-bit fields, by lanes per read
MID_CHUNK_SPILL = 32                                     # LPR 64 spills in front of read t == 32 of a chunk as well
HQ8_EVERY = 16                                           # reads per wave between two flush_hq8 of the 1 024-wide shape
COMP_U, COMP_NT, COMP_FIELD = 4, 1024, 65535             # composition_histogram: records per thread and round, threads, the 16-bit table
JB, PB, KEY_BIAS = (16, 5, 4), (16, 9, 11), (16, 16, 18)  # (threshold, value above / below ...) as the sources state them
CONSTANT_SOURCES = {
    "REG_FLUSH_EVERY": (KERNEL, r"constexpr uint32_t REG_FLUSH_EVERY = LPR == (16) \? (3) : \(LPR == (8) \? (7) : \(LPR == (4) \? (15) : (1)\)\);"),
    "MID_CHUNK_SPILL": (KERNEL, r"if \(LPR == 64 && t == (\d+)\) spill_base_regs\(\);"),
    "HQ8_EVERY": (PLAN, r"static constexpr int HQ8_EVERY = (\d+);"),
    "COMP_U": (KERNEL, r"#define FAQCS_COMP_U (\d+) "),
    "COMP_NT": (KERNEL, r"constexpr int NT = (\d+);"),
    "COMP_FIELD": (KERNEL, r"constexpr uint32_t FLUSH_EVERY = (\d+)u / \(NT \* U\);"),
    "JB": (PLAN, r"static constexpr int JB = C > (\d+) \? (\d+) : (\d+);"),
    "PB": (PLAN, r"static constexpr int PB = LPR <= (\d+) \? (\d+) : (\d+);"),
    "KEY_BIAS": (PLAN, r"static constexpr int KEY_BIAS = LPR <= (\d+) \? \(1 << (\d+)\) : \(1 << (\d+)\);"),
}
STATEMENT_SOURCES = {
    "the block flush of trim_filter_accumulate: every 65535 / (NW * 64) iterations": (KERNEL, r"constexpr uint32_t FLUSH_EVERY = 65535u / \(NW \* 64\) > 0 \? 65535u / \(NW \* 64\) : 1;"),
    "composition_histogram: at most n_cu / 2 blocks per record array": (KERNEL, r"if \(per_array > \(uint32_t\)\(n_cu / 2\)\) per_array = \(uint32_t\)\(n_cu / 2\);"),
    "composition_histogram flushes after FLUSH_EVERY rounds and after the last": (KERNEL, r"if \(\(\(r \+ 1\) % FLUSH_EVERY\) == 0 \|\| r \+ 1 == rounds\)"),
    "the fields spill after REG_FLUSH_EVERY iterations and with the block": (KERNEL, r"if \(\(\(it \+ 1\) % REG_FLUSH_EVERY\) == 0 \|\| block_flush\) spill_base_regs\(\);"),
    "flush_hq8 after every HQ8_EVERY reads of a chunk": (KERNEL, r"if \(Cfg::HQ8 && \(t % Cfg::HQ8_EVERY\) == Cfg::HQ8_EVERY - 1\) flush_hq8<C, LPR, NW>"),
    "an 8-bit cell holds NW x HQ8_EVERY at most": (KERNEL, r"static_assert\(!Cfg::HQ8 \|\| NW \* Cfg::HQ8_EVERY <= 255,"),
    "the 3' stop pattern takes the next lane's bits": (KERNEL, r"const uint32_t ext = r3 \| \(RW::next\(r3\) << C\);"),
    "the 5' stop pattern takes the previous lane's bits": (KERNEL, r"const uint32_t ext5 = \(r5 << 2\) \| \(\(RW::prev\(r5\) >> \(C - 2\)\) & 3u\);"),
    "the smaller position wins a 5' tie": (KERNEL, r"\(KEY_BIAS << JB\) \| \(\(int\)JM - j\)\)"),
    "T is corrected for the slots past the read": (KERNEL, r"if \(!WINDOWED\) T -= Q \* \(LPR \* C - len\);"),
    "the edit applies to upper-case G inside the window": (KERNEL, r"repbits &= gubits & win2;"),
    "column 0 is corrected by the reads that are not longer than p": (COMMON, r"for \(uint32_t l = 0; l <= p; \+\+l\) shorter \+= hlen\[l\] & 0xffffu;"),
    "positions from R on are not flushed": (COMMON, r"if \(p < R\) \{\s+if \(pre\) atomicAdd"),
    "the prefetch loads nothing past the read": (KERNEL, r"for \(int k = 0; k < D; \+\+k\) \{ nseq\.w\[k\] = 0; nqual\.w\[k\] = 0; \}\s+if \(pbase < n_len\) \{"),
}
COMP_ROUND = COMP_NT * COMP_U                            # records of a block and round
COMP_FLUSH_EVERY = COMP_FIELD // COMP_ROUND              # 15
TFA_FLUSH_EVERY = {4: 65535 // (4 * 64), 8: 65535 // (8 * 64)}   # 255 iterations; 127 for NW = 8
LDS_LAST = te.ROW_LAST[-1]                               # 304: the last length trim_lds takes

SHAPES = []                                              # (first length, last length = W, C, LPR, NW, compiled variants)
for _hi, _C, _LPR, _NW, _v in TFA_ROWS:
    SHAPES.append(((SHAPES[-1][1] + 1) if SHAPES else 1, _hi, _C, _LPR, _NW, _v))
assert all(s[1] == s[2] * s[3] for s in SHAPES) and SHAPES[-1][1] == FAST_READ_LENGTH
LPR_CLASSES = (4, 8, 16, 32, 64)
OPTION_SETS = {"headline": [], "5end": ["--5end", "3"], "avg_q": ["--avg_q", "20"], "5end_avg_q": ["--5end", "3", "--avg_q", "20"]}
FAMILIES = ("shapes", "seams", "lengths", "ns", "transitions", "replace", "sums", "chunks", "spills", "window")
FAMILY_REFERENCE = {f: "oracle" if f == "window" else "model" for f in FAMILIES}     # the trim model covers no adapters: OracleEngine alone, whole results and counter block
PREFIX = dict(shapes="sh:", seams="sm:", lengths="ln:", ns="ns:", transitions="tr:", replace="rp:", sums="su:", chunks="ch:", spills="sp:", window="wd:")
SETTINGS = ("natural", "single_pass")
# what the catalogue leaves out, by name (the CPU test counts them)
EXCLUSIONS = {
    "flush_block:16-bit_flush_after_FLUSH_EVERY_iterations": "FLUSH_EVERY = 255 iterations (127 for NW = 8) of a full grid are 16 .. 33 million reads in one launch on 256 compute units, "
                                                             "and no switch shrinks the grid",
    "walk:final_pos_3_one_below_final_pos_5": "the closed form cannot reach it either (DESIGN.md 4.1f): sm:no_read_with_final_pos_3_one_below_final_pos_5 asserts that the seams family has no such read",
}


def shape_of(n):
    return next((s for s in SHAPES if n <= s[1]), None)


def seam_ms(shape):
    """the lane borders m C - 1 | m C of a shape that the catalogue aims at: the first, the last, and every DPP row border (lane 15|16 of RowOps<32>;
    lanes 15|16, 31|32, 47|48 of RowOps<64>)"""
    LPR = shape[3]
    return sorted({1, LPR - 1} | ({16} if LPR == 32 else {16, 32, 48} if LPR == 64 else set()))


def borders(shape):
    return [m * shape[2] for m in seam_ms(shape)]


def switches(setting):
    return dict(DEFAULT_SWITCHES, lds_on=int(setting != "single_pass"))


def plan_of(args, longest, n_reads, n_cu, setting):
    return expected_plan(option_fields(list(args)), longest, n_reads, n_cu, switches(setting))


def iteration(shape, n_cu, args=()):
    """one iteration: the reads a full grid of the shape takes at once, grid_cap x NW x 64, from expected_plan"""
    p = plan_of(args, shape[1], 1 << 30, n_cu, "single_pass")
    assert p["kernel"] == "trim_filter_accumulate" and (p["C"], p["LPR"], p["NW"]) == shape[2:5]
    return p["grid"] * p["NW"] * 64


def comp_blocks(n, n_cu):
    """blocks per record array of faqcs_launch_composition"""
    return max(1, min((n + COMP_ROUND - 1) // COMP_ROUND, n_cu // 2))


def comp_rounds(n, n_cu):
    per = comp_blocks(n, n_cu) * COMP_ROUND
    return (n + per - 1) // per


class Tiled(list):
    """A submission of one segment: `period` repeated `repeats` times, then `rest`.  As a list it holds the two once, which is what the model and the
    predicates read; arenas() and tiled_results() unfold it"""

    def __init__(self, period, repeats, rest=()):
        list.__init__(self, [list(period), list(rest)])
        self.repeats = repeats
        assert repeats >= 1 and period

    def n(self):
        return len(self[0]) * self.repeats + len(self[1])


def sub_n(sub):
    return sub.n() if isinstance(sub, Tiled) else sum(len(seg) for seg in sub)


def sub_longest(sub):
    return max([len(r[1]) for seg in sub for r in seg] or [0])


def arenas(sub):
    """-> (seq arena, qual arena, offset, segment_start) of a submission in host memory, a Tiled one unfolded by numpy"""
    from faqcs_amd import driver

    if not isinstance(sub, Tiled):
        return driver.pack_segments(sub)
    pad = np.zeros(driver.PAD, np.uint8)
    parts, lens = {1: [], 2: []}, []
    for seg, k in ((sub[0], sub.repeats), (sub[1], 1)):
        for col in (1, 2):
            parts[col].append(np.tile(np.frombuffer(b"".join(r[col] for r in seg), np.uint8), k))
        lens.append(np.tile(np.array([len(r[1]) for r in seg], np.int64), k))
    lens = np.concatenate(lens)
    offset = np.zeros(len(lens) + 1, np.uint32)
    offset[1:] = np.cumsum(lens).astype(np.uint32)
    assert int(lens.sum()) < 1 << 32
    seq, qual = (np.concatenate([pad] + parts[col] + [pad]) for col in (1, 2))
    return seq[driver.PAD:], qual[driver.PAD:], offset, np.array([0, len(lens)], np.uint32)


def run_model(case):
    """te.run_model with Tiled submissions: -> dict(results=[array per submission], counters, error, trace)"""
    o = case.opt()
    total, results, trace = None, [], []

    def one_block(segments):
        m = Model(o, case.R, case.in_off)
        r = np.zeros(sum(len(s) for s in segments), te.RESULT_DTYPE)
        try:
            for i, t in enumerate(m.submit(segments)):
                r[i] = t + (0,)
        finally:
            trace.extend(m.trace)
        return r, m.block()

    try:
        for sub in case.subs:
            if isinstance(sub, Tiled):
                r1, b1 = one_block([sub[0]])
                r2, b2 = one_block([sub[1]])
                r, b = np.concatenate([np.tile(r1, sub.repeats), r2]), b1 * np.uint64(sub.repeats) + b2
            else:
                r, b = one_block(sub)
            results.append(r)
            total = b if total is None else total + b
    except te.QualityError:
        return dict(results=None, counters=None, error=te.E_QUALITY, trace=trace)
    return dict(results=results, counters=total, error=0, trace=trace)


class FCase(TCase):
    """A TCase of this catalogue, built for n_cu compute units.  setting(): `natural` (no switch: every submission with a base has a read past 304 bases,
    or the case runs --replace_to_N_q) or `single_pass` (FAQCS_TRIM_LDS=0)"""

    def __init__(self, name, args, subs, claims, n_cu=256, R=None, hostile=False, shifts=None, adapters=(), oracle=False):
        self.adapters = list(adapters)          # extra (name, sequence) targets behind the built-in set
        TCase.__init__(self, name, args, subs, claims, R=R, hostile=hostile, shifts=shifts)
        self.n_cu, self.oracle = n_cu, oracle
        assert self.R >= self.longest and all(not isinstance(s, Tiled) for s in subs) or shifts is None

    def opt(self):
        o = TCase.opt(self)
        o.adapter.extend(self.adapters)
        return o

    def expected(self):
        if self._exp is None:
            if self.oracle:
                from trim_long_edges import run_oracle

                self._exp = run_oracle(self)
            else:
                self._exp = run_model(self)
        return self._exp

    def ctx(self):
        if self._ctx is None:
            self._ctx = FCtx(self)
        return self._ctx

    def n_reads(self):
        return sum(sub_n(sub) for sub in self.subs)

    def setting(self):
        natural = self.opt().replace_to_N_q > 0 or all(sub_longest(sub) > LDS_LAST for sub in self.subs if sub_longest(sub))
        return "natural" if natural else "single_pass"

    def kernel(self, k):
        """the kernel submission k must report (None: a batch without a base)"""
        longest = sub_longest(self.subs[k])
        return None if longest == 0 else "trim_long" if longest > FAST_READ_LENGTH else "trim_filter_accumulate"

    def plan(self, k, setting=None):
        return plan_of(self.args, sub_longest(self.subs[k]), sub_n(self.subs[k]), self.n_cu, setting or self.setting())


class FCtx(te.Ctx):
    def __init__(self, case):
        te.Ctx.__init__(self, case)
        self.n_cu = case.n_cu
        self._sc = {}
        e = case.expected()
        self.res = np.concatenate(e["results"]) if e["results"] else None      # (the window family's predicates read the oracle's results)
        # (submission index, read) and the trace, in the order the model saw them: a Tiled submission's period and remainder once
        self.by_sub, at = [], 0
        for sub in case.subs:
            n = sum(len(seg) for seg in sub)
            self.by_sub.append(self.rt[at:at + n])
            at += n

    def shapes(self):
        return [shape_of(sub_longest(sub)) for sub in self.case.subs]

    def with_shape(self):
        """[(shape of the read's submission, read, Info)]"""
        return [(sh, r, i) for sh, rows in zip(self.shapes(), self.by_sub) if sh for r, i in rows]

    def scores(self, r):
        """the clamped scores of a read after the terminal-N mask"""
        key = id(r)
        if key not in self._sc:
            _, s, q = r
            n = len(s)
            lead, trail = n - len(s.lstrip(b"N")), n - len(s.rstrip(b"N"))
            q = bytearray(q)
            q[:lead] = bytes([self.off]) * lead
            q[n - trail:] = bytes([self.off]) * min(trail, n)
            self._sc[key] = np.maximum(np.frombuffer(bytes(q), np.int8).astype(np.int64) - self.off, 0)
        return self._sc[key]


EDGES = {}


def edge(name):
    def reg(f):
        EDGES[name] = f
        return f
    return reg


def W(i):
    return i.w or {}


def all_shapes(found):
    """found: a set of (last length of the shape, ...) tuples or of last lengths -> every shape is in it"""
    return {s[1] for s in SHAPES} <= {x[0] if isinstance(x, tuple) else x for x in found}


# =====================================================================================================================================
# edges
# =====================================================================================================================================
# ---- shapes -------------------------------------------------------------------------------------------------------------------------
def _variant(c, k):
    p = c.case.plan(k, "single_pass")
    return (p["C"], p["LPR"], p["windowed"], p["ext"]) if p["kernel"] == "trim_filter_accumulate" else None


def compiled_variants():
    out = set()
    for _, _, C, LPR, _, v in SHAPES:
        out |= {(C, LPR, w, e) for w in (0, 1) for e in (0, 1) if v == 4 or (v == 2 and w == e) or (w and e)}
    return out


for _name in OPTION_SETS:
    # a batch whose longest read is the row's first length and one at its last, with shorter and empty reads, under one of the four option sets
    edge("sh:%s:first_and_last_length_of_a_shape" % _name)(lambda c, nm=_name: c.case.args[4:] == [str(a) for a in OPTION_SETS[nm]] and len(c.case.subs) == 2 and
                                                         (lambda sh: sh is not None and [sub_longest(s) for s in c.case.subs] == [sh[0], sh[1]])(shape_of(c.case.longest)) and
                                                         all(any(len(r[1]) == 0 for seg in s for r in seg) and len({len(r[1]) for seg in s for r in seg}) >= min(5, sub_longest(s) + 1) for s in c.case.subs))
edge("sh:requests_(T,F)_and_(F,T)_run_the_superset_at_512")(lambda c: shape_of(c.case.longest)[1] == 512 and option_fields(c.case.args)["trim5"] != option_fields(c.case.args)["avgq_on"] and
                                                            _variant(c, 1)[2:] == (1, 1))
edge("sh:every_request_runs_the_superset_at_768_and_1024")(lambda c: shape_of(c.case.longest)[1] in (768, 1024) and _variant(c, 1)[2:] == (1, 1) and
                                                           not (option_fields(c.case.args)["trim5"] and option_fields(c.case.args)["avgq_on"]))
edge("sh:1024|1025_hands_over_to_trim_long")(lambda c: [c.case.kernel(k) for k in range(len(c.case.subs))] == ["trim_filter_accumulate", "trim_long"] and
                                             [sub_longest(s) for s in c.case.subs] == [1024, 1025])


# ---- seams --------------------------------------------------------------------------------------------------------------------------
def _reset3(c, r, i):
    """the 3' reset bits of a read's window (the whole read: the seams cases apply no fixed cuts): reset[p] = (p > 2) & (sum of Q - score behind p >= 0)"""
    sc = c.scores(r)
    d = c.o.quality - sc
    after = np.concatenate([np.cumsum(d[::-1])[::-1][1:], [0]])
    return (np.arange(len(sc)) > 2) & (after >= 0)


def _stop3(c, r, i):
    """the position p of the stop pattern !reset[p] & !reset[p + 1] & reset[p + 2] nearest the read's end, or None"""
    rs = _reset3(c, r, i)
    hit = np.nonzero(~rs[:-2] & ~rs[1:-1] & rs[2:])[0] if len(rs) > 2 else []
    return int(hit[-1]) if len(hit) else None


def _reset5(c, r, i):
    sc = c.scores(r)
    d = c.o.quality - sc
    before = np.concatenate([[0], np.cumsum(d)[:-1]])
    return (np.arange(len(sc)) < W(i)["f3"] - 2) & (before >= 0)


def _stop5(c, r, i):
    """the position p of the 5' stop pattern reset[p - 2] & !reset[p - 1] & !reset[p] nearest the read's start, or None"""
    rs = _reset5(c, r, i)
    hit = np.nonzero(rs[:-2] & ~rs[1:-1] & ~rs[2:])[0] if len(rs) > 2 else []
    return int(hit[0]) + 2 if len(hit) else None


def _plus(c):
    return c.o.mode == MODE_BWA_PLUS and not c.o.protect_5 and not c.o.trim_5 and not c.o.trim_3


def _at_borders(c, what, deltas):
    """per shape and border b: `what(read, Info)` takes every value b + d, d in deltas"""
    got = {}
    for sh, r, i in c.with_shape():
        if i.w:
            v = what(r, i)
            if v is not None:
                got.setdefault(sh[1], set()).add(v)
    return all({b + d for b in borders(sh) for d in deltas if 0 <= b + d < sh[1]} <= got.get(sh[1], set()) for sh in SHAPES)


# the stop pattern's three positions p, p + 1, p + 2 against the border b: p = b - 3 (all below), b - 2 (the re-arming step is the first of the next lane),
# b - 1 (one non-reset step each side), b (all above)
edge("sm:bwa_plus_3:stop_pattern_at_every_placement_across_a_border")(lambda c: _plus(c) and _at_borders(c, lambda r, i: _stop3(c, r, i), (-3, -2, -1, 0)))
edge("sm:bwa_plus_3:maximum_on_either_side_of_a_border")(lambda c: _plus(c) and _at_borders(c, lambda r, i: i.w["f3"] + 1 if i.w["step3"] >= 0 else None, (-1, 0)))
edge("sm:bwa_plus_3:two_equal_maxima_one_each_side_the_larger_position_wins")(lambda c: _plus(c) and _at_borders(c, lambda r, i: i.w["f3"] + 1 if i.w["tie3"] and _tie3_other(c, r, i) else None, (0, 1)))


edge("sm:bwa_plus_3:two_equal_maxima_inside_a_lane_the_larger_position_wins")(lambda c: _plus(c) and _at_borders(c, lambda r, i: i.w["f3"] + 1 if i.w["tie3"] and _tie3_other(c, r, i) else None, (-1, 2)))
edge("sm:bwa_plus_3:new_maximum_beyond_the_stop_at_every_placement")(lambda c: _plus(c) and _at_borders(c, lambda r, i: _stop3(c, r, i) if _beyond3(c, r, i) else None, (-3, -2, -1, 0)))
edge("sm:bwa_plus_5:two_equal_maxima_inside_a_lane_the_smaller_position_wins")(lambda c: _plus(c) and _at_borders(c, lambda r, i: i.w["f5"] - 1 if i.w["tie5"] and _tie5_other(c, r, i) else None, (-3, 0)))
edge("sm:bwa_plus_5:new_maximum_beyond_the_stop_at_every_placement")(lambda c: _plus(c) and _at_borders(c, lambda r, i: _stop5(c, r, i) if _beyond5(c, r, i) else None, (-1, 0, 1, 2)))


def _beyond3(c, r, i):
    """in front of the 3' stop the sum of Q - score from a position on passes the maximum the walk found: a walk that went on would cut there"""
    d = c.o.quality - c.scores(r)
    suf = np.cumsum(d[::-1])[::-1]
    p = _stop3(c, r, i)
    return p is not None and p > 0 and i.w["step3"] >= 0 and int(suf[:p].max()) > int(suf[i.w["f3"] + 1])


def _beyond5(c, r, i):
    d = c.o.quality - c.scores(r)
    pre = np.cumsum(d)
    p = _stop5(c, r, i)
    return p is not None and i.w["step5"] >= 0 and int(pre[p + 1:i.w["f3"]].max()) > int(pre[i.w["f5"] - 1])


def _tie3_other(c, r, i):
    """the 3' walk's maximum is reached a second time, two positions further in"""
    d = c.o.quality - c.scores(r)
    p = i.w["f3"] + 1
    return p >= 2 and int(d[p:].sum()) == int(d[p - 2:].sum()) > 0


def _tie5_other(c, r, i):
    d = c.o.quality - c.scores(r)
    p = i.w["f5"] - 1
    return p + 2 < len(d) and int(d[:p + 1].sum()) == int(d[:p + 3].sum()) > 0


edge("sm:bwa_plus_5:stop_pattern_at_every_placement_across_a_border")(lambda c: _plus(c) and _at_borders(c, lambda r, i: _stop5(c, r, i), (-1, 0, 1, 2)))
edge("sm:bwa_plus_5:maximum_on_either_side_of_a_border")(lambda c: _plus(c) and _at_borders(c, lambda r, i: i.w["f5"] - 1 if i.w["step5"] >= 0 else None, (-1, 0)))
edge("sm:bwa_plus_5:two_equal_maxima_one_each_side_the_smaller_position_wins")(lambda c: _plus(c) and _at_borders(c, lambda r, i: i.w["f5"] - 1 if i.w["tie5"] and _tie5_other(c, r, i) else None, (-2, -1)))
# (the exclusion walk:final_pos_3_one_below_final_pos_5: the family that walks every placement has no such read, so the closed form never meets it)
edge("sm:no_read_with_final_pos_3_one_below_final_pos_5")(lambda c: _plus(c) and len(c.trace) > 100 and any(i.w and i.w["f3"] <= i.w["f5"] for i in c.trace) and
                                                          not any(i.w and i.w["f3"] == i.w["f5"] - 1 for i in c.trace))
edge("sm:bwa:first_failing_step_on_either_side_of_a_border")(lambda c: c.o.mode == MODE_BWA and _at_borders(c, lambda r, i: len(r[1]) - i.w["steps3"] if i.w["neg3"] >= 0 else None, (-1, 0)))
edge("sm:hard:first_good_score_from_the_end_on_either_side_of_a_border")(lambda c: c.o.mode == MODE_HARD and _at_borders(c, lambda r, i: i.w["f3"] if i.w["found3"] else None, (-1, 0)))
edge("sm:hard:first_good_score_from_the_start_on_either_side_of_a_border")(lambda c: c.o.mode == MODE_HARD and _at_borders(c, lambda r, i: i.w["f5"] if i.w["f5"] > 0 else None, (-1, 0)))
edge("sm:kept_window_starts_and_ends_on_mC-1_mC_mC+1")(lambda c: _plus(c) and _at_borders(c, lambda r, i: i.a if i.flags & F_VALID and i.a else None, (-1, 0, 1)) and
                                                       _at_borders(c, lambda r, i: i.a + i.kept - 1 if i.flags & F_VALID and i.kept < i.n0 else None, (-1, 0, 1)))
for _q, _sc in ((41, 0), (0, 41)):
    # the largest and the smallest total of Q - score at full width: the key bias and the PB / JB fields of the argmax keys
    edge("sm:score_total_extreme_q%d_all_scores_%d_at_full_width" % (_q, _sc))(lambda c, q=_q, sc=_sc: c.o.quality == q and all_shapes(
        {sh[1] for sh, r, i in c.with_shape() if len(r[1]) == sh[1] and set(c.scores(r)) == {sc}}))

# ---- lengths ------------------------------------------------------------------------------------------------------------------------
edge("ln:every_length_0..C+1")(lambda c: all(set(range(sh[2] + 2)) <= {len(r[1]) for s2, r, i in c.with_shape() if s2 == sh} for sh in SHAPES))
edge("ln:lengths_mC-1_mC_mC+1_for_the_two_widest_m_and_W-1_W")(lambda c: all(
    {m * sh[2] + d for m in (sh[3] - 2, sh[3] - 1) for d in (-1, 0, 1)} | {sh[1] - 1, sh[1]} <= {len(r[1]) for s2, r, i in c.with_shape() if s2 == sh} for sh in SHAPES))
edge("ln:every_length_mod_4_at_every_dword_count")(lambda c: all(set(range(1, sh[2] + 1)) <= {len(r[1]) - (sh[3] - 1) * sh[2] for s2, r, i in c.with_shape() if s2 == sh} for sh in SHAPES))


def _row_pairs(c):
    """{(shape's last length, length of a read, length of the read behind it in the same row of its chunk, or None where the batch ends)}: reads t and t + 1 of
    a row are batch indices 64 k + rowb + t and + 1 with t + 1 < LPR"""
    out = set()
    for sh, rows in zip(c.shapes(), c.by_sub):
        if sh:
            LPR = sh[3]
            for k, (r, i) in enumerate(rows):
                if (k % 64) % LPR != LPR - 1:
                    out.add((sh[1], len(r[1]), len(rows[k + 1][0][1]) if k + 1 < len(rows) else None))
    return out


edge("ln:full_width_read_then_an_empty_a_one_base_and_a_C_base_read_in_its_row_and_the_reverse")(lambda c: all(
    {(sh[1], sh[1], x) for x in (0, 1, sh[2])} | {(sh[1], x, sh[1]) for x in (0, 1, sh[2])} <= _row_pairs(c) for sh in SHAPES))
edge("ln:the_rows_last_read_is_absent")(lambda c: all((sh[1], sh[1], None) in _row_pairs(c) for sh in SHAPES))
# a genuine score of 0 at a position where shorter reads of the same block have ended: column 0 of that position holds both the real count and the slots past the
# shorter reads, which flush_block takes out by the length histogram
edge("ln:score_0_where_shorter_reads_have_ended")(lambda c: all(any(
    any(len(r[1]) > p and c.scores(r)[p] == 0 and r[1][p] != 78 for r, i in rows) and any(0 < len(r[1]) <= p for r, i in rows) and any(len(r[1]) == 0 for r, i in rows) and
    any(len(r[1]) == p + 1 for r, i in rows) for p in (1, sh[2], sh[1] - 2)) for sh, rows in zip(c.shapes(), c.by_sub) if sh) and all_shapes({sh[1] for sh in c.shapes() if sh}))
edge("ln:context_narrower_than_the_shape")(lambda c: all_shapes({sh[1] for sh in c.shapes() if sh}) and all(sub_longest(s) == c.case.R < shape_of(sub_longest(s))[1] for s in c.case.subs) and
                                           len({x.R for x in [c.case]}) == 1)
edge("ln:context_of_1024")(lambda c: c.case.R == 1024 and all_shapes({sh[1] for sh in c.shapes() if sh}))


# ---- ns -----------------------------------------------------------------------------------------------------------------------------
def _nrun(s, front):
    t = s if front else s[::-1]
    return len(t) - len(t.lstrip(b"N"))


def _low_inwards(c, r, front):
    """low bases inwards of the terminal run: an unmasked run (scores of 41) would stop the walk in front of them"""
    s, sc = r[1], c.scores(r)
    k = _nrun(s, front)
    return 0 < k < len(s) - 8 and all(x < c.o.quality for x in (sc[k:k + 3] if front else sc[len(s) - k - 3:len(s) - k]))


edge("ns:terminal_N_runs_of_0..C+1_at_each_end_with_low_bases_inwards")(lambda c: all(
    set(range(1, sh[2] + 2)) <= {_nrun(r[1], f) for s2, r, i in c.with_shape() if s2 == sh and _low_inwards(c, r, f) and i.flags & F_QUAL_TRIMMED} for sh in SHAPES for f in (True, False)))
edge("ns:terminal_N_runs_under_qc_only_are_masked_and_nothing_is_cut")(lambda c: c.o.qc_only and all(
    set(range(1, sh[2] + 2)) <= {_nrun(r[1], f) for s2, r, i in c.with_shape() if s2 == sh and _low_inwards(c, r, f) and i.flags & F_VALID and i.kept == i.n0} for sh in SHAPES for f in (True, False)))
edge("ns:trailing_run_starts_on_the_last_position_of_a_lane_and_on_the_first_of_the_next")(lambda c: all(
    {b - 1, b} <= {len(r[1]) - _nrun(r[1], False) for s2, r, i in c.with_shape() if s2 == sh and 0 < _nrun(r[1], False) < len(r[1])} for sh in SHAPES for b in borders(sh)))
edge("ns:leading_run_ends_on_the_last_position_of_a_lane_and_on_the_first_of_the_next")(lambda c: all(
    {b - 1, b} <= {_nrun(r[1], True) - 1 for s2, r, i in c.with_shape() if s2 == sh and 0 < _nrun(r[1], True) < len(r[1])} for sh in SHAPES for b in borders(sh)))
edge("ns:all_N_reads_of_mC_and_W_bases")(lambda c: all({sh[2], sh[2] * (sh[3] - 1), sh[1]} <= {len(r[1]) for s2, r, i in c.with_shape() if s2 == sh and r[1] and r[1] == b"N" * len(r[1])} for sh in SHAPES))
edge("ns:lower_case_n_at_an_end_is_not_masked")(lambda c: all(any(s2 == sh and r[1][-1:] == b"n" and c.scores(r)[-1] > 0 for s2, r, i in c.with_shape()) and
                                                              any(s2 == sh and r[1][:1] == b"n" and c.scores(r)[0] > 0 for s2, r, i in c.with_shape()) for sh in SHAPES))


def _runs(s):
    """[(start, length)] of the runs of upper-case N"""
    a = np.frombuffer(s, np.uint8) == 78
    d = np.diff(np.concatenate([[0], a.view(np.int8), [0]]))
    st, en = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    return list(zip(st.tolist(), (en - st).tolist()))


def _poly_edge(c, k, qc):
    """runs of k - 1, k, k + 1 (the read's only run, inside the kept window) that straddle a lane border of the shape at every offset, judged as the rule says"""
    if c.o.max_num_poly_N != k or bool(c.o.qc_only) != qc:
        return False
    for sh in SHAPES:
        b = sh[2] * (sh[3] // 2)
        got = set()
        for s2, r, i in c.with_shape():
            rs = _runs(r[1])
            if s2 == sh and len(rs) == 1 and i.npoly == rs[0][1]:
                st, ln = rs[0]
                tripped = bool(i.flags & F_POLY_N_SEEN)
                if tripped == (ln >= k) and (qc or (i.filt == FILT_POLY_N) == tripped):
                    got.add((ln, b - st))
        if not {(ln, x) for ln in (k - 1, k, k + 1) for x in range(1, ln)} <= got:
            return False
    return True


for _k in (2, 3, 7):
    for _qc in (False, True):
        edge("ns:-n_%d%s:runs_of_k-1_k_k+1_straddle_a_border_at_every_offset" % (_k, ":qc_only" if _qc else ""))(lambda c, k=_k, qc=_qc: _poly_edge(c, k, qc))
edge("ns:run_of_2C+2_spans_four_lanes_and_one_of_C+2_three")(lambda c: c.o.max_num_poly_N > 2 and all(
    any(s2 == sh and (st, ln) == (sh[2] - 1, sh[2] + 2) for s2, r, i in c.with_shape() for st, ln in _runs(r[1])) and
    any(s2 == sh and (st, ln) == (sh[2] - 1, 2 * sh[2] + 2) and i.npoly == ln for s2, r, i in c.with_shape() for st, ln in _runs(r[1])) for sh in SHAPES))
edge("ns:run_broken_by_n_on_a_lanes_first_position")(lambda c: all(any(s2 == sh and r[1][b - 2:b + 2] == b"NNnN" and i.npoly == 2 for s2, r, i in c.with_shape()) for sh in SHAPES for b in borders(sh)[:1]))

# ---- transitions --------------------------------------------------------------------------------------------------------------------
TR_LC = ("0.2", "0.4", "0.75", "0.5")


def _tr_lengths(text):
    return sorted(set(te.LC_LENGTHS[text]) | set(te.LC_DI_LENGTHS[text]))


for _lc in TR_LC:
    edge("tr:lc_%s:threshold_lengths_in_every_shape_that_has_one" % _lc)(lambda c, t=_lc: c.lc_text() == t and all(
        te._lc_edge(c, False, [n for n in te.LC_LENGTHS[t] if lc_thr(n, c.o.low_complexity_cutoff_ratio)], False) for _ in (0,)) and
        {shape_of(n)[1] for n in _tr_lengths(t)} <= {sh[1] for sh in c.shapes() if sh})


def _pairs_across(c, sh, r, i, pair=b"AT"):
    """the borders (positions b with r[b - 1 : b + 1] == pair) of the shape that a read's transitions cross"""
    return {b for b in range(sh[2], sh[1], sh[2]) if r[1][b - 1:b + 1] == pair}


edge("tr:thr2-1_and_thr2_transitions_with_exactly_one_across_each_aimed_border")(lambda c: all(
    {(b, f) for b in borders(sh) for f in (FILT_NONE, FILT_LOW_COMPLEXITY)} <=
    {(b, i.filt) for s2, r, i in c.with_shape() if s2 == sh and i.counts and len(_pairs_across(c, sh, r, i)) == 1 and i.wlen == sh[1] and
     i.dmax == lc_thr(i.wlen, c.o.low_complexity_cutoff_ratio, True) - (i.filt == FILT_NONE) and i.cmax < lc_thr(i.wlen, c.o.low_complexity_cutoff_ratio) for b in _pairs_across(c, sh, r, i)}
    for sh in SHAPES))
edge("tr:non_base_on_a_lanes_last_position_in_front_of_a_lone_base")(lambda c: all(
    any(s2 == sh and r[1][b - 1:b] == b"R" and r[1][b:b + 1] == b"T" and r[1][b - 2:b - 1] == b"A" and i.counts and i.filt == FILT_NONE and
        i.dmax == lc_thr(i.wlen, c.o.low_complexity_cutoff_ratio, True) - 1 for s2, r, i in c.with_shape()) for sh in SHAPES for b in borders(sh)[:1]))


# ---- replace ------------------------------------------------------------------------------------------------------------------------
def _rep(c, r, i):
    """positions of the read whose upper-case G has a score below --replace_to_N_q (edited where they lie inside the kept window)"""
    s, sc = np.frombuffer(r[1], np.uint8), c.scores(r)
    return set(np.nonzero((s == 71) & (sc < c.o.replace_to_N_q))[0].tolist())


for _q in (1, 15, 41):
    edge("rp:q%d:G_at_thr-1_and_thr_and_g_at_thr-1_on_either_side_of_a_border" % _q)(lambda c, q=_q: c.o.replace_to_N_q == q and all(
        {(p, ch, x) for p in (b - 1, b) for ch, x in ((71, q - 1), (71, q), (103, q - 1))} <=
        {(p, r[1][p], int(c.scores(r)[p])) for s2, r, i in c.with_shape() if s2 == sh and i.flags & F_VALID and len(r[1]) == sh[1] for p in (b - 1, b)}
        for sh in SHAPES for b in borders(sh)))
edge("rp:one_case_per_LPR_class")(lambda c: c.o.replace_to_N_q > 0 and {sh[3] for sh in c.shapes() if sh} == set(LPR_CLASSES) and any(_rep(c, r, i) for r, i in c.rt))
edge("rp:replaced_G_is_either_member_of_the_transition_that_decides_lc")(lambda c: c.o.replace_to_N_q > 0 and all(
    {(m, f) for m in (0, 1) for f in (FILT_NONE,)} <= {(m, i.filt) for s2, r, i in c.with_shape() if s2 == sh and i.counts for m in (0, 1)
                                                       if _decides(c, r, i, m)} for sh in SHAPES if sh[1] >= 64))


def _decides(c, r, i, member):
    """the read would be low-complexity by its transitions without the edit (dmax + 1 == thr2), and the one replaced G is the first / second member of such a pair"""
    rep = _rep(c, r, i)
    if len(rep) != 1 or i.filt != FILT_NONE:
        return False
    p = next(iter(rep))
    t2 = lc_thr(i.wlen, c.o.low_complexity_cutoff_ratio, True)
    pair = r[1][p:p + 2] if member == 0 else r[1][p - 1:p + 1]
    return i.dmax == t2 - 1 and pair in (b"GA", b"AG") and r[1].count(pair) == t2


edge("rp:replaced_G_outside_the_kept_window_is_not_counted")(lambda c: c.o.replace_to_N_q > 0 and all(any(
    s2 == sh and i.flags & F_VALID and any(p >= i.a + i.kept for p in _rep(c, r, i)) and any(p < i.a for p in _rep(c, r, i)) and i.bins[4] == 0 for s2, r, i in c.with_shape()) for sh in SHAPES))
edge("rp:replaced_G_next_to_a_masked_terminal_N")(lambda c: c.o.replace_to_N_q > 0 and all(any(
    s2 == sh and i.flags & F_VALID and r[1][:1] == b"N" and 1 in _rep(c, r, i) and r[1][-1:] == b"N" and len(r[1]) - 2 in _rep(c, r, i) for s2, r, i in c.with_shape()) for sh in SHAPES))
edge("rp:all_G_read_of_W_bases_all_replaced")(lambda c: c.o.replace_to_N_q > 0 and all(any(
    s2 == sh and r[1] == b"G" * sh[1] and i.flags & F_VALID and i.kept == sh[1] and len(_rep(c, r, i)) == sh[1] and i.counts == [0, 0, 0, 0] for s2, r, i in c.with_shape()) for sh in SHAPES))
edge("rp:whole_read_kept_and_only_the_edit_changes_the_counts")(lambda c: c.o.replace_to_N_q > 0 and all(any(
    s2 == sh and i.flags & F_VALID and i.a == 0 and i.kept == i.n0 == sh[1] and len(_rep(c, r, i)) == 1 and i.bins != i.pre_bin for s2, r, i in c.with_shape()) for sh in SHAPES))
# (poly-N looks at the read's own bytes: two replaced G side by side are no run of N.  The model says so, and the CPU test holds the model to the oracle)
edge("rp:-n_2_with_two_replaced_G_side_by_side")(lambda c: c.o.replace_to_N_q > 0 and c.o.max_num_poly_N == 2 and all(any(
    s2 == sh and i.flags & F_VALID and not i.flags & F_POLY_N_SEEN and any(p + 1 in _rep(c, r, i) for p in _rep(c, r, i)) and i.npoly == 0 for s2, r, i in c.with_shape()) for sh in SHAPES))

# ---- sums ---------------------------------------------------------------------------------------------------------------------------
SUM_SHAPES = (160, 768, 1024)        # C = 20 (the widest lane) and the two 64-lane shapes (the most lanes): the packed word N count << 20 | V + (1 << 12) per lane
edge("su:quality_bytes_all_0x80_under_ascii_64_at_full_width")(lambda c: c.off == 64 and all(any(s2[1] == w and len(r[1]) == w and set(r[2]) == {0x80} for s2, r, i in c.with_shape()) for w in SUM_SHAPES))
edge("su:quality_bytes_all_offset+41_at_full_width")(lambda c: all(any(s2[1] == w and len(r[1]) == w and set(r[2]) == {c.off + 41} and i.flags & F_VALID for s2, r, i in c.with_shape()) for w in SUM_SHAPES))
edge("su:W_bases_all_one_base_and_half_and_half_at_1024")(lambda c: {r[1] for s2, r, i in c.with_shape() if s2[1] == 1024 and i.flags & F_VALID} >=
                                                          {ch * 1024 for ch in (b"A", b"T", b"C", b"G")} | {b"A" * 512 + b"T" * 512, b"C" * 512 + b"G" * 512})
edge("su:V_post_through_both_branches")(lambda c: c.o.average_quality > 0 and all(
    any(s2 == sh and i.flags & F_QUAL_TRIMMED and i.flags & F_VALID and min(r[2]) >= c.off for s2, r, i in c.with_shape()) and
    any(s2 == sh and i.flags & F_QUAL_TRIMMED and i.flags & F_VALID and any(x < c.off for x in r[2][i.a:i.a + i.kept]) for s2, r, i in c.with_shape()) and
    any(s2 == sh and i.flags & F_QUAL_TRIMMED and i.flags & F_VALID and any(x < c.off for x in r[2][i.a + i.kept:]) and min(r[2][i.a:i.a + i.kept]) >= c.off for s2, r, i in c.with_shape())
    for sh in SHAPES))


# ---- chunks -------------------------------------------------------------------------------------------------------------------------
def batch_sizes(shape, n_cu):
    NW, it = shape[4], iteration(shape, n_cu)
    return sorted({1, 63, 64, 65, 64 * NW - 1, 64 * NW, 64 * NW + 1, it - 1, it, it + 1, it + 64 * NW + 1})


HQ8_SIZES = (1, 15, 16, 17, 31, 32, 33, 64, 65, 8 * 64 - 1, 8 * 64 + 1)
LPR_SHAPE = {4: 64, 8: 160, 16: 256, 32: 512, 64: 768}      # the shape that stands for an LPR class in the chunks and spills families


def _sizes(c):
    out = {}
    for sub in c.case.subs:
        sh = shape_of(sub_longest(sub))
        if sh:
            out.setdefault(sh[1], set()).add(sub_n(sub))
    return out


edge("ch:batch_sizes_of_every_LPR_class")(lambda c: all(_sizes(c).get(w, set()) >= set(batch_sizes(shape_of(w), c.n_cu)) for w in LPR_SHAPE.values()))
edge("ch:a_wave_whose_second_iteration_chunk_does_not_exist")(lambda c: all(any(
    it < n and (n + 63) // 64 - it // 64 < shape_of(w)[4] * ((it // 64) // shape_of(w)[4]) for n in _sizes(c).get(w, set()) for it in [iteration(shape_of(w), c.n_cu)]) for w in LPR_SHAPE.values()))
edge("ch:hq8:reads_of_identical_quality_at_every_flush_count")(lambda c: _sizes(c).get(1024, set()) >= set(HQ8_SIZES) and all(
    len({r[2] for seg in sub for r in seg}) == 1 for sub in c.case.subs if sub_longest(sub) > 768))
edge("ch:every_device_address_mod_16_at_the_wide_shapes")(lambda c: c.case.shifts is not None and not c.case.hostile and
                                                          {(shape_of(sub_longest(s))[1], k) for s, k in zip(c.case.subs, c.case.shifts)} >= {(w, k) for w in (320, 512, 768, 1024) for k in range(16)})
edge("ch:hostile_padding_at_the_wide_shapes")(lambda c: c.case.hostile and c.case.shifts is not None and all(
    any(shape_of(sub_longest(sub))[1] == w and len(sub[0][0][1]) > 0 and len(sub[0][-1][1]) > 0 and (sub[0][0][1][:1] == b"N") == n and (sub[0][-1][1][-1:] == b"N") == n for sub in c.case.subs)
    for w in (320, 512, 768, 1024) for n in (True, False)) and any(i.a > 0 for i in c.trace) and any(i.flags & F_VALID and i.a + i.kept < i.n0 for i in c.trace))


# ---- spills -------------------------------------------------------------------------------------------------------------------------
def _spill_edge(c, LPR):
    """one launch of REG_FLUSH_EVERY + 1 full iterations of the LPR class's shape whose reads all hold the same base at a position (LPR 64: 65 reads in one
    chunk): a field that is spilled one iteration late overflows its 6 bits"""
    sh = shape_of(LPR_SHAPE[LPR])
    for sub, rows in zip(c.case.subs, c.by_sub):
        if shape_of(sub_longest(sub)) != sh:
            continue
        same = len({r[1][:1] for r, i in rows}) == 1 and all(len(r[1]) > sh[2] for r, i in rows) and len({r[1][sh[2]:sh[2] + 1] for r, i in rows}) == 1
        if LPR == 64:
            if same and sub_n(sub) == 65:
                return True
        elif same and sub_n(sub) == (REG_FLUSH_EVERY[LPR] + 1) * iteration(sh, c.n_cu) and field_peak(LPR, sub_n(sub), iteration(sh, c.n_cu)) <= 63 < field_peak(LPR, sub_n(sub), iteration(sh, c.n_cu), late=1):
            return True
    return False


def field_peak(LPR, n_reads, it_reads, late=0, mid_chunk=True):
    """the largest value a 6-bit field of a lane takes between two spills when every read of a launch adds 1 to it: LPR reads per chunk and row, one chunk per
    wave and iteration, spilled after every REG_FLUSH_EVERY (+ late) iterations and after the last; LPR 64: in front of read 32 of a chunk as well"""
    per_chunk = LPR if LPR < 64 else (32 if mid_chunk else 64)
    n_iter = max(1, (n_reads + it_reads - 1) // it_reads)
    return min(n_iter, REG_FLUSH_EVERY[LPR] + late) * per_chunk if n_reads >= it_reads or LPR == 64 else per_chunk


for _lpr in LPR_CLASSES:
    edge("sp:lpr%d:one_launch_past_the_spill_with_reads_identical_at_a_position" % _lpr)(lambda c, l=_lpr: _spill_edge(c, l))
for _wide in (False, True):
    edge("sp:comp:%s:records_4095_4096_4097_and_the_second_round" % ("wide" if _wide else "narrow"))(lambda c, w=_wide: {sub_n(s) for s in c.case.subs if (sub_longest(s) > 256) == w} >= {
        COMP_ROUND - 1, COMP_ROUND, COMP_ROUND + 1, (c.n_cu // 2) * COMP_ROUND - 1, (c.n_cu // 2) * COMP_ROUND + 1})
    # 16 rounds of records that all fall into the same bins: 4 096 per block and round, 61 440 after 15 rounds, past 65 535 without the flush
    edge("sp:comp:%s:sixteen_rounds_into_one_bin" % ("wide" if _wide else "narrow"))(lambda c, w=_wide: any(
        (sub_longest(s) > 256) == w and comp_rounds(sub_n(s), c.n_cu) == COMP_FLUSH_EVERY + 1 and isinstance(s, Tiled) and
        {len(r[1]) for r in s[0]} == {1} and {r[1] for r in s[0]} == {b"A"} and sub_n(s) - len(s[0]) * s.repeats <= 64 for s in c.case.subs) and
        COMP_FLUSH_EVERY * COMP_ROUND <= COMP_FIELD < (COMP_FLUSH_EVERY + 1) * COMP_ROUND)

# ---- window (the oracle's results: the model has no adapters) --------------------------------------------------------------------------
F_ADAPTER = 0x20
WINDOW_LENGTHS = (310, 400, 700, 1000)
# the lane border the window starts on, in the read's first half (an adapter in the second half is a 3' adapter): the DPP row border where it lies there
WINDOW_BORDER = {310: 160, 400: 128, 700: 192, 1000: 256}


def _wd(c, pred):
    """the lengths at which a read and its oracle result meet pred(read, result)"""
    return {len(r[1]) for r, x in zip(c.reads, c.res) if pred(r, x)}


edge("wd:3'_adapter_behind_a_low_tail_that_the_walk_takes")(lambda c: c.case.oracle and _wd(c, lambda r, x: r[1].endswith(ADAPTER_3) and x["flags"] & F_ADAPTER and x["flags"] & F_VALID and
                                                                                     x["start"] == 0 and x["len"] == len(r[1]) - len(ADAPTER_3) - 30) >= set(WINDOW_LENGTHS))
edge("wd:5'_adapter_in_front_of_a_low_head_that_the_walk_takes")(lambda c: c.case.oracle and _wd(c, lambda r, x: r[1][5:5 + len(ADAPTER_3)] == ADAPTER_3 and x["flags"] & F_ADAPTER and x["flags"] & F_VALID and
                                                                                          x["start"] == 5 + len(ADAPTER_3) + 20) >= set(WINDOW_LENGTHS))
edge("wd:whole_read_masked")(lambda c: c.case.oracle and any(r[1].decode() == a[1] and not x["flags"] & F_VALID and x["flags"] & F_ADAPTER for a in c.case.adapters for r, x in zip(c.reads, c.res)))
edge("wd:window_starts_on_mC-1_and_mC")(lambda c: c.case.oracle and all({b - 1, b} <= {int(x["start"]) for r, x in zip(c.reads, c.res) if len(r[1]) == n and x["flags"] & F_ADAPTER and x["flags"] & F_VALID}
                                                                        for n, b in WINDOW_BORDER.items()) and all(b % shape_of(n)[2] == 0 for n, b in WINDOW_BORDER.items()))
edge("wd:replace_to_N_q_15_at_150_behind_an_adapter_window")(lambda c: c.case.oracle and c.o.replace_to_N_q == 15 and any(
    len(r[1]) == 150 and x["flags"] & F_ADAPTER and x["flags"] & F_VALID and x["len"] < 150 - len(ADAPTER_3) and
    any(ch == 71 and q - c.off < 15 for ch, q in zip(r[1][x["start"]:x["start"] + x["len"]], r[2][x["start"]:x["start"] + x["len"]])) for r, x in zip(c.reads, c.res)))

# =====================================================================================================================================
# builders
# =====================================================================================================================================
ADAPTER_3 = b"CTGTCTCTTATACACATCTAGATGTGTATAAGAGACAG"        # Nextera-junction-adapter-1 of the built-in set (faqcs_amd/options.py; the CPU test compares)
WINDOW_ARGS = ["--adapter", "-t", "1", "--min_L", "1", "-n", "40000", "--lc", "1", "--avg_q", "0"]
BASE = ["--min_L", "1", "--lc", "1.0", "-n", "2000"]
WALK_MODES = {"bwa_plus": [], "bwa": ["--mode", "BWA"], "hard": ["--mode", "HARD"]}


def full(sh, salt=0, good=38):
    """a good read of the shape's full width: it selects the shape"""
    return rd(rb(sh[1], salt + sh[1]), Qs([good] * sh[1]))


def q_read(n, sc, salt=0):
    return rd(rb(n, salt + n), Qs(sc))


def shapes_cases(n_cu):
    C = []
    for sh in SHAPES:
        for nm, extra in OPTION_SETS.items():
            subs = [[te.ragged(14, L, sh[1] + k) + [rd(b"")]] for k, L in enumerate((sh[0], sh[1]))]
            claims = ["sh:%s:first_and_last_length_of_a_shape" % nm]
            if sh[1] == 512 and nm in ("5end", "avg_q"):
                claims.append("sh:requests_(T,F)_and_(F,T)_run_the_superset_at_512")
            if sh[1] >= 768 and nm != "5end_avg_q":
                claims.append("sh:every_request_runs_the_superset_at_768_and_1024")
            C.append(FCase("sh_%d_%s" % (sh[1], nm), ["--min_L", "10", "--lc", "0.85"] + extra, subs, claims, n_cu))
    C.append(FCase("sh_1024_1025", ["--min_L", "10", "--lc", "0.85"], [[te.ragged(9, 1024, 1)], [te.ragged(9, 1025, 2)]], ["sh:1024|1025_hands_over_to_trim_long"], n_cu, R=4096))
    return C


def tail(n, deltas, Q, salt=0, good=38):
    """a read of n good bases whose scores from the end inwards are Q - deltas[k]"""
    sc = [good] * n
    for k, x in enumerate(deltas):
        sc[n - 1 - k] = Q - x
    return q_read(n, sc, salt)


def head(n, deltas, Q, salt=0, good=38, zeros=0):
    """... from position `zeros` on (the positions in front of it hold Q: the area stays 0 and the walk goes on)"""
    sc = [good] * n
    sc[:zeros] = [Q] * zeros
    for k, x in enumerate(deltas):
        sc[zeros + k] = Q - x
    return q_read(n, sc, salt)


def seams_cases(n_cu):
    C = []
    Q = 5
    for sh in SHAPES:
        Cc = sh[2]
        reads3, reads5, bwa, hard, wins = [full(sh)], [full(sh, 1)], [full(sh, 2)], [full(sh, 3)], [full(sh, 4)]
        for b in borders(sh):
            for p in (b - 3, b - 2, b - 1, b):
                # the last re-arming step at p + 2: a tail of t low bases behind it, a good base on it and in front of it (the area falls by 33 and stays negative)
                for t in (2, 5):
                    if p + 2 >= 3 and p + 3 + t <= sh[1]:
                        reads3.append(tail(p + 3 + t, [1] * t, Q, p))
                # ... and with a larger sum beyond the stop: a step down of 3 on p + 2, none on p + 1, bases of score 0 on p (the walk's last step) and p - 1 (which a
                # walk that misses the stop takes)
                if p >= 4 and p + 5 <= sh[1]:
                    reads3.append(tail(p + 5, [1, 1, -3, 0, 5, 5], Q, p + 1))
            for p in (b - 1, b, b + 1, b + 2):
                # the 5' mirror: the last re-arming step at p - 2, the two steps without one at p - 1 and p
                for t in (2, 5):
                    if p - 2 - t >= 0 and p + 6 <= sh[1]:
                        reads5.append(head(min(p + 40, sh[1]), [1] * t, Q, p, zeros=p - 2 - t))
                if p - 4 >= 0 and p + 8 <= sh[1]:
                    reads5.append(head(min(p + 40, sh[1]), [1, 1, -3, 0, 5, 5], Q, p + 1, zeros=p - 4))
            for m in (b - 1, b):
                # the 3' maximum on position m (final_pos_3 = m - 1)
                if m + 3 <= sh[1]:
                    reads3.append(tail(m + 3, [1, 1, 1], Q, m))
                # BWA: the first failing step (area < 0) on position m: a low tail down to m + 1, a good base on m
                if m + 4 <= sh[1]:
                    bwa.append(tail(m + 4, [1, 1, 1], Q, m))
                # ... and twice, two positions apart (the larger position wins): on m + 1 and m - 1 across the border, on m and m - 2 / m + 2 and m inside a lane
                for p in (m, m + 1 if m == b else m + 3):
                    if p + 2 <= sh[1]:
                        reads3.append(tail(p + 2, [1, 1, -1, 1], Q, p + 1))
                # the 5' maximum on position m (final_pos_5 = m + 1)
                if m >= 2 and m + 6 <= sh[1]:
                    reads5.append(head(min(m + 40, sh[1]), [1, 1, 1], Q, m, zeros=m - 2))
                # ... and twice, two positions apart (the smaller position wins): across the border and inside a lane
                for p in (m - 1, m - 2 if m == b - 1 else m):
                    if p >= 1 and p + 9 <= sh[1]:
                        reads5.append(head(min(p + 40, sh[1]), [1, 1, -1, 1], Q, p + 1, zeros=p - 1))
                # HARD: the first good score from the end on m; the first from the start on m (and another behind it for the 3' side)
                n = min(m + 20, sh[1])
                hard.append(q_read(n, [Q] * m + [Q + 1] + [Q] * (n - m - 1), m))
                if m + 7 <= sh[1]:
                    hard.append(q_read(m + 7, [Q] * m + [Q + 1] + [Q] * 3 + [Q + 1] + [Q] * 2, m + 1))
            for d in (-1, 0, 1):
                if 4 <= b + d <= sh[1] - 6:
                    n = min(b + d + 30, sh[1])
                    wins.append(q_read(n, [2] * (b + d) + [38] * (n - b - d), b + d))             # the window starts on b + d
                    n = min(b + d + 5, sh[1])
                    wins.append(q_read(n, [38] * (b + d + 1) + [2] * (n - b - d - 1), b + d + 1))  # ... ends on b + d
        reads3 += [tail(n, d, Q, 99) for n in (6, Cc + 2) for d in ([3, -2, -3], [1, -5, 3, 1, -9], [4, -9])]   # (final_pos_3 at and below final_pos_5)
        reads3 += [q_read(9, [2] * 9, 1), q_read(Cc + 1, [2] * (Cc + 1), 2)]
        C.append(FCase("sm_%d_bwa_plus_3" % sh[1], BASE, [[reads3]], [], n_cu))
        C.append(FCase("sm_%d_bwa_plus_5" % sh[1], BASE, [[reads5]], [], n_cu))
        C.append(FCase("sm_%d_windows" % sh[1], BASE, [[wins]], [], n_cu))
        C.append(FCase("sm_%d_bwa" % sh[1], BASE + WALK_MODES["bwa"], [[bwa]], [], n_cu))
        C.append(FCase("sm_%d_hard" % sh[1], BASE + WALK_MODES["hard"], [[hard]], [], n_cu))
    # one case per mode over every shape, which is what the edges ask for: the per-shape cases above are its submissions
    out = []
    for kind, args, claims in (("bwa_plus_3", BASE, ["sm:bwa_plus_3:stop_pattern_at_every_placement_across_a_border", "sm:bwa_plus_3:two_equal_maxima_inside_a_lane_the_larger_position_wins",
                                                     "sm:bwa_plus_3:new_maximum_beyond_the_stop_at_every_placement", "sm:bwa_plus_3:maximum_on_either_side_of_a_border",
                                                     "sm:bwa_plus_3:two_equal_maxima_one_each_side_the_larger_position_wins", "sm:no_read_with_final_pos_3_one_below_final_pos_5"]),
                               ("bwa_plus_5", BASE, ["sm:bwa_plus_5:stop_pattern_at_every_placement_across_a_border", "sm:bwa_plus_5:two_equal_maxima_inside_a_lane_the_smaller_position_wins",
                                                     "sm:bwa_plus_5:new_maximum_beyond_the_stop_at_every_placement", "sm:bwa_plus_5:maximum_on_either_side_of_a_border",
                                                     "sm:bwa_plus_5:two_equal_maxima_one_each_side_the_smaller_position_wins"]),
                               ("windows", BASE, ["sm:kept_window_starts_and_ends_on_mC-1_mC_mC+1"]),
                               ("bwa", BASE + WALK_MODES["bwa"], ["sm:bwa:first_failing_step_on_either_side_of_a_border"]),
                               ("hard", BASE + WALK_MODES["hard"], ["sm:hard:first_good_score_from_the_end_on_either_side_of_a_border", "sm:hard:first_good_score_from_the_start_on_either_side_of_a_border"])):
        subs = [c.subs[0] for c in C if c.name.endswith("_" + kind)]
        out.append(FCase("sm_" + kind, args, subs, claims, n_cu))
    for q, sc in ((41, 0), (0, 41)):
        out.append(FCase("sm_total_q%d" % q, BASE + ["-q", q], [[[q_read(sh[1], [sc] * sh[1], q), q_read(sh[1] // 2, [sc] * (sh[1] // 2), q), q_read(sh[1], [20] * sh[1], q + 1)]] for sh in SHAPES],
                         ["sm:score_total_extreme_q%d_all_scores_%d_at_full_width" % (q, sc)], n_cu))
    return out


def lengths_cases(n_cu):
    C = []
    subs, prefetch, shorter = [], [], []
    for sh in SHAPES:
        lo, hi, Cc, LPR = sh[:4]
        lens = sorted(set(range(Cc + 2)) | {m * Cc + d for m in (LPR - 2, LPR - 1) for d in (-1, 0, 1)} | {hi - 1, hi} | {(LPR - 1) * Cc + k for k in range(1, Cc + 1)})
        subs.append([[full(sh)] + [q_read(n, [30 + (n + j) % 9 for j in range(n)], n) for n in lens]])
        # rows of a chunk: LPR reads each.  A full-width read followed by an empty, a one-base and a C-base read, and the reverse; the batch ends inside a row behind
        # a full-width read
        row = lambda a, b: [a, b] + [q_read(7, [33] * 7, 7)] * (LPR - 2)
        small = [rd(b""), q_read(1, [33]), q_read(Cc, [35] * Cc)]
        reads = [r for x in small for r in row(full(sh, 5), x) + row(x, full(sh, 6))]
        pad = [q_read(7, [33] * 7, 7)] * ((-len(reads)) % 64)
        prefetch.append([reads + pad + [full(sh, 7)]])
        # genuine scores of 0 at p where shorter reads have ended, empty reads among them
        rs = [full(sh, 8)]
        for p in (1, Cc, hi - 2):
            sc = [30] * hi
            sc[p] = 0
            rs += [q_read(hi, sc, p), q_read(p + 1, ([30] * p + [0]), p), q_read(p, [31] * p, p), rd(b""), q_read(max(p - 1, 1), [32] * max(p - 1, 1), p)]
        shorter.append([rs])
    C.append(FCase("ln_lengths", BASE, subs, ["ln:every_length_0..C+1", "ln:lengths_mC-1_mC_mC+1_for_the_two_widest_m_and_W-1_W", "ln:every_length_mod_4_at_every_dword_count"], n_cu))
    C.append(FCase("ln_prefetch", BASE, prefetch, ["ln:full_width_read_then_an_empty_a_one_base_and_a_C_base_read_in_its_row_and_the_reverse", "ln:the_rows_last_read_is_absent"], n_cu))
    C.append(FCase("ln_score_0_past_shorter_reads", BASE + ["-q", "0"], shorter, ["ln:score_0_where_shorter_reads_have_ended"], n_cu))
    C.append(FCase("ln_score_0_past_shorter_reads_R1024", BASE + ["-q", "0"], shorter, ["ln:score_0_where_shorter_reads_have_ended", "ln:context_of_1024"], n_cu, R=1024))
    for sh in SHAPES:
        if sh[1] - sh[0] >= 2:
            L = sh[1] - 2         # the longest read is the context's R, two below the shape's width: the slots L and L + 1 are counted by every read and flushed by none
            sc = [30] * L
            sc[L - 1] = 0
            C.append(FCase("ln_context_%d_in_shape_%d" % (L, sh[1]), BASE + ["-q", "0"], [[[q_read(L, sc, 1), q_read(L - 1, [30] * (L - 1), 2), rd(b""), q_read(L, [29] * L, 3), q_read(1, [0], 4)]]],
                           [], n_cu, R=L))
    both = [c for c in C if c.name.startswith("ln_context_")]
    assert len(both) == len(SHAPES)
    for c in both:
        c.claims = ("ln:context_narrower_than_the_shape",)
    return C


LN_CONTEXT_SHAPES = None    # (every shape has a context case of its own: the edge holds per case, and the CPU test asks that the cases' shapes are all twelve)
EDGES["ln:context_narrower_than_the_shape"] = lambda c: len(c.case.subs) == 1 and sub_longest(c.case.subs[0]) == c.case.R == shape_of(c.case.R)[1] - 2 and any(
    len(r[1]) == c.case.R and c.scores(r)[-1] == 0 for r, i in c.rt) and any(len(r[1]) == 0 for r, i in c.rt)


def n_read(n, lead, trail, Q=5, salt=0, low=3, ch=b"N"):
    """a read of n bases with terminal runs of `ch` under scores of 41 and `low` low bases inwards of each"""
    s = ch * lead + rb(n - lead - trail, salt + n) + ch * trail
    sc = [41] * lead + [2] * low + [38] * (n - lead - trail - 2 * low) + [2] * low + [41] * trail
    assert len(s) == len(sc) == n
    return rd(s, Qs(sc))


def run_read(n, start, ln, salt=0, mid=None):
    s = bytearray(rb(n, salt + start))
    s[start:start + ln] = b"N" * ln
    if mid is not None:
        s[mid] = ord("n")
    return rd(bytes(s))


def ns_cases(n_cu):
    C = []
    subs, alln = [], []
    for sh in SHAPES:
        lo, hi, Cc, LPR = sh[:4]
        n = min(max(3 * Cc + 20, 40), hi)
        reads = [full(sh)] + [n_read(n, k, 0, salt=k) for k in range(1, Cc + 2)] + [n_read(n, 0, k, salt=k + 40) for k in range(1, Cc + 2)] + [n_read(n, 2, 2, ch=b"n")]
        for b in borders(sh):
            for x in (b - 1, b):
                if 6 <= x <= hi - 1:
                    reads.append(n_read(hi, 0, hi - x, salt=x))        # the trailing run starts on x
                if x + 1 <= hi - 6:
                    reads.append(n_read(hi, x + 1, 0, salt=x + 1))     # the leading run ends on x
        subs.append([reads])
        alln.append([[full(sh, 1)] + [rd(b"N" * k, Qs([30] * k)) for k in (Cc, Cc * (LPR - 1), hi)] + [rd(rb(20, 3))]])
    C.append(FCase("ns_terminal_runs", BASE, subs, ["ns:terminal_N_runs_of_0..C+1_at_each_end_with_low_bases_inwards", "ns:trailing_run_starts_on_the_last_position_of_a_lane_and_on_the_first_of_the_next",
                                                    "ns:leading_run_ends_on_the_last_position_of_a_lane_and_on_the_first_of_the_next", "ns:lower_case_n_at_an_end_is_not_masked"], n_cu))
    C.append(FCase("ns_terminal_runs_qc_only", BASE + ["--qc_only"], subs, ["ns:terminal_N_runs_under_qc_only_are_masked_and_nothing_is_cut"], n_cu))
    C.append(FCase("ns_all_N", BASE, alln, ["ns:all_N_reads_of_mC_and_W_bases"], n_cu))
    for k in (2, 3, 7):
        subs = []
        for sh in SHAPES:
            lo, hi, Cc, LPR = sh[:4]
            b = Cc * (LPR // 2)
            reads = [full(sh)]
            for ln in (k - 1, k, k + 1):
                reads += [run_read(hi, b - x, ln, x) for x in range(1, ln)]
            if k > 2:
                reads += [run_read(hi, Cc - 1, Cc + 2, 1), run_read(hi, Cc - 1, 2 * Cc + 2, 2)]
            b0 = borders(sh)[0]
            reads.append(run_read(hi, b0 - 2, 4, 3, mid=b0))
            subs.append([reads])
        for qc in (False, True):
            claims = ["ns:-n_%d%s:runs_of_k-1_k_k+1_straddle_a_border_at_every_offset" % (k, ":qc_only" if qc else "")]
            if k == 7 and not qc:
                claims += ["ns:run_of_2C+2_spans_four_lanes_and_one_of_C+2_three", "ns:run_broken_by_n_on_a_lanes_first_position"]
            C.append(FCase("ns_poly_n%d%s" % (k, "_qc_only" if qc else ""), ["--min_L", "1", "--lc", "1.0", "-n", k] + (["--qc_only"] if qc else []), subs, claims, n_cu))
    return C


def pair_read(n, k, across, pair=b"AT", gap=b"R"):
    """a read of n bases with k transitions `pair`, one of them across the position `across` (its second member on it), none across any other position that is
    a multiple of anything: the others lie in blocks pair + gap from the read's start, kept clear of `across`"""
    s = bytearray(gap * n)
    s[across - 1:across + 1] = pair
    at, left = 1, k - 1
    while left:
        if at + 2 < across - 1 or at > across + 1:
            s[at:at + 2] = pair
            left -= 1
        at += 3
        assert at + 2 < n, (n, k, across)
    return bytes(s)


def clear_of(s, sh, keep, pair=b"AT"):
    """no transition `pair` of s crosses a lane border of the shape but the one on `keep`"""
    return all(s[b - 1:b + 1] != pair or b == keep for b in range(sh[2], sh[1], sh[2]))


def transitions_cases(n_cu):
    C = []
    base = ["--mode", "BWA", "--min_L", "1", "-n", "2000"]
    for text in TR_LC:
        lc = f32(float(text))
        reads = []
        for n in _tr_lengths(text):
            for letter in range(4):
                reads += te.lc_reads(n, lc, letter)
            reads += te.di_reads(n, lc)
        subs = [[[full(sh)] + [r for r in reads if sh[0] <= len(r[1]) <= sh[1]]] for sh in SHAPES if any(sh[0] <= len(r[1]) <= sh[1] for r in reads)]
        C.append(FCase("tr_lc_%s" % text, base + ["--lc", text], subs, ["tr:lc_%s:threshold_lengths_in_every_shape_that_has_one" % text], n_cu))
    # thr2 - 1 and thr2 transitions AT at full width, exactly one of them across a lane border: lane by lane, the transition that prev_last carries decides
    lc = f32(0.4)
    subs = []
    for sh in SHAPES:
        hi, Cc = sh[1], sh[2]
        t2 = lc_thr(hi, lc, True)
        reads = [full(sh)]
        for b in borders(sh):
            for k in (t2 - 1, t2):
                s = bytearray(pair_read(hi, k, b))
                # move the blocks that fell on another border one position on
                for bb in range(Cc, hi, Cc):
                    if bb != b and bytes(s[bb - 1:bb + 1]) == b"AT":
                        s[bb - 1:bb + 2] = b"RAT" if bytes(s[bb + 1:bb + 2]) == b"R" and bytes(s[bb + 2:bb + 3]) != b"T" else s[bb - 1:bb + 2]
                assert clear_of(bytes(s), sh, b) and bytes(s).count(b"AT") == k, (sh, b, k)
                reads.append(rd(bytes(s)))
        # a lone T on a lane's first position behind a non-base on the last position of the lane before, an A in front of that: no transition, whatever prev_last
        # carries; thr2 - 1 transitions elsewhere, so one more would take the read
        b = borders(sh)[0]
        s = bytearray(b"R" * hi)
        s[b - 2:b + 1] = b"ART"
        spots = [at for at in range(0, hi - 2, 3) if at + 2 < b - 3 or at > b + 2]
        for at in spots[:t2 - 1]:
            s[at:at + 2] = b"AT"
        assert bytes(s).count(b"AT") == t2 - 1
        reads.append(rd(bytes(s)))
        subs.append([reads])
    C.append(FCase("tr_pairs_across_borders", base + ["--lc", "0.4"], subs, ["tr:thr2-1_and_thr2_transitions_with_exactly_one_across_each_aimed_border",
                                                                               "tr:non_base_on_a_lanes_last_position_in_front_of_a_lone_base"], n_cu))
    return C


def replace_cases(n_cu):
    C = []
    base = ["--min_L", "1", "-n", "2"]
    for q in (1, 15, 41):
        subs = []
        for sh in SHAPES:
            hi, Cc = sh[1], sh[2]
            reads = []
            for b in borders(sh):
                for p in (b - 1, b):
                    for ch, x in ((b"G", q - 1), (b"G", q), (b"g", q - 1)):
                        s = bytearray(rb(hi, p))
                        s[p:p + 1] = ch
                        sc = [41] * hi
                        sc[p] = x
                        reads.append(rd(bytes(s), Qs(sc)))
            subs.append([reads])
        C.append(FCase("rp_q%d_borders" % q, base + ["--lc", "1.0", "--replace_to_N_q", q, "-q", "0"], subs, ["rp:q%d:G_at_thr-1_and_thr_and_g_at_thr-1_on_either_side_of_a_border" % q], n_cu))
    q = 15
    subs, lcsubs = [], []
    for sh in SHAPES:
        hi, Cc = sh[1], sh[2]
        b = borders(sh)[-1]
        reads = []
        # outside the kept window on both sides: low heads and tails that hold a G
        s = bytearray(rb(hi, 11).replace(b"G", b"C"))
        s[1:2], s[hi - 2:hi - 1] = b"G", b"G"
        reads.append(rd(bytes(s), Qs([2] * 4 + [38] * (hi - 8) + [2] * 4)))
        # under a masked terminal N neighbour
        s = bytearray(rb(hi, 12))
        s[0:2], s[hi - 2:hi] = b"NG", b"GN"
        reads.append(rd(bytes(s), Qs([41] + [10] + [38] * (hi - 4) + [10] + [41])))
        reads.append(rd(b"G" * hi, Qs([14] * hi)))
        # the whole read kept, one edit
        s = bytearray(rb(hi, 13).replace(b"G", b"C"))
        s[b:b + 1] = b"G"
        sc = [38] * hi
        sc[b] = 14
        reads.append(rd(bytes(s), Qs(sc)))
        # two replaced G side by side across a border
        s[b - 1:b + 1] = b"GG"
        sc[b - 1] = 14
        reads.append(rd(bytes(s), Qs(sc)))
        subs.append([reads])
        if hi >= 64:
            # thr2 transitions AG (GA), the G of one of them on a border replaced: thr2 - 1 are left and the read stays
            t2 = lc_thr(hi, f32(0.4), True)
            rs = []
            for pair in (b"GA", b"AG"):
                gpos = b - 1 if pair == b"GA" else b     # (the transition crosses the border either way)
                body = bytearray(pair_read(hi, t2, b, pair=pair))
                sc = [38] * hi
                sc[gpos] = 14
                assert body[gpos:gpos + 1] == b"G"
                rs.append(rd(bytes(body), Qs(sc)))
            lcsubs.append([rs])
    C.append(FCase("rp_windows_and_neighbours", base + ["--lc", "1.0", "--replace_to_N_q", q], subs,
                   ["rp:replaced_G_outside_the_kept_window_is_not_counted", "rp:replaced_G_next_to_a_masked_terminal_N", "rp:all_G_read_of_W_bases_all_replaced",
                    "rp:whole_read_kept_and_only_the_edit_changes_the_counts", "rp:-n_2_with_two_replaced_G_side_by_side", "rp:one_case_per_LPR_class"], n_cu))
    C.append(FCase("rp_transition_members", ["--min_L", "1", "-n", "2000", "--lc", "0.4", "--replace_to_N_q", q], lcsubs, ["rp:replaced_G_is_either_member_of_the_transition_that_decides_lc"], n_cu))
    return C


def sums_cases(n_cu):
    C = []
    subs64 = [[[rd(rb(w, 1), bytes([0x80] * w)), rd(rb(w // 2, 2), bytes([0x80] * (w // 2))), rd(rb(w, 3), Qs([41] * w, 64))]] for w in SUM_SHAPES]
    C.append(FCase("su_bytes_0x80_ascii_64", BASE + ["--ascii", "64", "-q", "0"], subs64, ["su:quality_bytes_all_0x80_under_ascii_64_at_full_width", "su:quality_bytes_all_offset+41_at_full_width"], n_cu))
    C.append(FCase("su_bytes_41", BASE + ["-q", "0"], [[[rd(rb(w, 3), Qs([41] * w)), rd(rb(w - 1, 4), Qs([41] * (w - 1)))]] for w in SUM_SHAPES], ["su:quality_bytes_all_offset+41_at_full_width"], n_cu))
    reads = [rd(ch * 1024) for ch in (b"A", b"T", b"C", b"G")] + [rd(b"A" * 512 + b"T" * 512), rd(b"C" * 512 + b"G" * 512)]
    C.append(FCase("su_pair_sums_1024", BASE, [[reads]], ["su:W_bases_all_one_base_and_half_and_half_at_1024"], n_cu))
    subs = []
    for sh in SHAPES:
        hi = sh[1]
        clean = q_read(hi, [30] * (hi - 6) + [2] * 6, 1)
        inside = rd(rb(hi, 2), bytes([64 + 30] * 8 + [40] + [64 + 30] * (hi - 15) + [64 + 2] * 6))
        outside = rd(rb(hi, 3), bytes([64 + 30] * (hi - 6) + [64 + 2] * 3 + [40] + [64 + 2] * 2))
        subs.append([[rd(c[1], bytes(x - 33 + 64 for x in c[2])) for c in (clean,)] + [inside, outside]])
    C.append(FCase("su_V_post_branches", BASE + ["--ascii", "64", "--avg_q", "3"], subs, ["su:V_post_through_both_branches"], n_cu))
    return C


def mixed_period(sh, k=61):
    """k distinct short reads (0 .. C + 1 bases, low tails, an N) for a Tiled batch of the shape"""
    Cc = sh[2]
    return te.ragged(k, Cc + 1, sh[1])[1:] + [rd(rb(Cc + 1, 5))]


def sized(sh, n, salt=0):
    """a submission of n reads of the shape: one full-width read, the others short"""
    per = mixed_period(sh)
    if n <= 600:
        return [(per * (n // len(per) + 1))[:n - 1] + [full(sh, salt)]]
    return Tiled(per, (n - 1) // len(per), per[:(n - 1) % len(per)] + [full(sh, salt)])


def chunks_cases(n_cu):
    C = []
    for LPR, w in LPR_SHAPE.items():
        sh = shape_of(w)
        C.append(FCase("ch_sizes_lpr%d" % LPR, ["--min_L", "10"], [sized(sh, n, n) for n in batch_sizes(sh, n_cu)], [], n_cu))
    C.append(FCase("ch_sizes", ["--min_L", "10"], [s for c in C for s in c.subs], ["ch:batch_sizes_of_every_LPR_class", "ch:a_wave_whose_second_iteration_chunk_does_not_exist"], n_cu))
    C = C[-1:]
    sh = SHAPES[-1]
    one_q = q_read(1024, [17 + (j % 5 == 0) for j in range(1024)], 1)
    C.append(FCase("ch_hq8_identical_quality", BASE, [[[one_q] * n] for n in HQ8_SIZES], ["ch:hq8:reads_of_identical_quality_at_every_flush_count"], n_cu))
    subs, shifts = [], []
    for w in (320, 512, 768, 1024):
        for k in range(16):
            subs.append([te.ragged(6, w, k)])
            shifts.append(k)
    C.append(FCase("ch_device_addresses", ["--min_L", "1"], subs, ["ch:every_device_address_mod_16_at_the_wide_shapes"], n_cu, shifts=shifts))
    subs, shifts = [], []
    for n, hi in enumerate((320, 512, 768, 1024)):
        subs.append([[rd(rb(hi // 2 + 1, hi), Qs([2] * 3 + [38] * (hi // 2 - 2)))] + te.ragged(3, hi, 9)[::-1] + [te.low_tail(hi - 3, 3, hi)]])
        subs.append([[rd(b"NN" + rb(hi // 2, hi), Qs([41] * 2 + [2] * 3 + [38] * (hi // 2 - 3)))] + te.ragged(3, hi, 9)[::-1] +
                     [rd(rb(hi - 2, hi) + b"NN", Qs([38] * (hi - 5) + [2] * 3 + [41] * 2))]])
        shifts += [(5 * n + 3) % 16, (5 * n + 12) % 16]
    C.append(FCase("ch_hostile_padding", ["--min_L", "1"], subs, ["ch:hostile_padding_at_the_wide_shapes"], n_cu, hostile=True, shifts=shifts))
    return C


def same_at(sh, k):
    """k distinct reads of C + 1 bases that all hold A on position 0 and T on position C (the first position of lane 1), good scores"""
    Cc = sh[2]
    return [rd(b"A" + rb(Cc - 1, j).replace(b"A", b"C") + b"T", Qs([30 + (j + x) % 10 for x in range(Cc + 1)])) for j in range(k)]


def spills_cases(n_cu):
    C = []
    for LPR in (4, 8, 16, 32):
        sh = shape_of(LPR_SHAPE[LPR])
        n = (REG_FLUSH_EVERY[LPR] + 1) * iteration(sh, n_cu)
        per = same_at(sh, 7)
        wide = rd(b"A" + rb(sh[1] - 1, 1)[:sh[2] - 1] + b"T" + rb(sh[1], 2)[sh[2] + 1:])
        C.append(FCase("sp_lpr%d" % LPR, BASE, [Tiled(per, (n - 1) // 7, per[:(n - 1) % 7] + [wide])], ["sp:lpr%d:one_launch_past_the_spill_with_reads_identical_at_a_position" % LPR], n_cu))
    sh = shape_of(LPR_SHAPE[64])
    wide = rd(b"A" + rb(sh[1] - 1, 1)[:sh[2] - 1] + b"T" + rb(sh[1], 2)[sh[2] + 1:])
    C.append(FCase("sp_lpr64", BASE, [[same_at(sh, 64) + [wide]]], ["sp:lpr64:one_launch_past_the_spill_with_reads_identical_at_a_position"], n_cu))
    half = n_cu // 2
    for wide_rec in (False, True):
        long_read = rd(rb(300, 1)) if wide_rec else rd(rb(40, 1))
        per = te.ragged(60, 30, 5)[1:]
        subs = []
        for n in (COMP_ROUND - 1, COMP_ROUND, COMP_ROUND + 1, half * COMP_ROUND - 1, half * COMP_ROUND + 1):
            subs.append(Tiled(per, (n - 1) // len(per), per[:(n - 1) % len(per)] + [long_read]))
        nm = "wide" if wide_rec else "narrow"
        C.append(FCase("sp_comp_%s_rounds" % nm, BASE, subs, ["sp:comp:%s:records_4095_4096_4097_and_the_second_round" % nm], n_cu))
        n = (COMP_FLUSH_EVERY + 1) * half * COMP_ROUND
        C.append(FCase("sp_comp_%s_16_rounds" % nm, ["--mode", "BWA"] + BASE, [Tiled([rd(b"A")], n - 1, [long_read])], ["sp:comp:%s:sixteen_rounds_into_one_bin" % nm], n_cu))
    return C


def window_cases(n_cu):
    A = ADAPTER_3
    reads = []
    for n in WINDOW_LENGTHS:
        body = n - len(A)
        reads.append(rd(rb(body, n) + A, Qs([38] * (body - 30) + [2] * 30 + [38] * len(A))))                                         # 3' cut, a low tail in front of it
        reads.append(rd(rb(5, n) + A + rb(body - 5, n + 1), Qs([38] * (5 + len(A)) + [2] * 20 + [38] * (body - 45) + [2] * 20)))   # 5' cut, a low head and a low tail behind it
        b = WINDOW_BORDER[n]
        for st in (b - 1, b):                                                                                                        # the window starts on st
            reads.append(rd(rb(st - len(A), n + st) + A + rb(n - st, n + st + 1)))
    whole = rb(700, 77)
    reads.append(rd(whole))
    C = [FCase("wd_adapter_window_then_walk", WINDOW_ARGS, [[[r for r in reads if shape_of(len(r[1])) == sh]] for sh in SHAPES[8:]],
               ["wd:3'_adapter_behind_a_low_tail_that_the_walk_takes", "wd:5'_adapter_in_front_of_a_low_head_that_the_walk_takes", "wd:whole_read_masked", "wd:window_starts_on_mC-1_and_mC"],
               n_cu, adapters=[("whole-read", whole.decode())], oracle=True)]
    s = bytearray(rb(150 - len(A), 150).replace(b"G", b"C"))
    s[40:41] = b"G"
    r150 = rd(bytes(s) + A, Qs([38] * 40 + [14] + [38] * (150 - len(A) - 41 - 20) + [2] * 20 + [38] * len(A)))
    C.append(FCase("wd_replace_150", WINDOW_ARGS + ["--replace_to_N_q", "15"], [[[r150, rd(rb(150, 3))]]], ["wd:replace_to_N_q_15_at_150_behind_an_adapter_window"], n_cu, oracle=True))
    return C


_BUILDERS = dict(window=window_cases, shapes=shapes_cases, seams=seams_cases, lengths=lengths_cases, ns=ns_cases, transitions=transitions_cases, replace=replace_cases, sums=sums_cases,
                 chunks=chunks_cases, spills=spills_cases)
_CASES = {}


def family_cases(family, n_cu=256):
    if (family, n_cu) not in _CASES:
        cs = _BUILDERS[family](n_cu)
        for c in cs:
            c.family = family
        _CASES[(family, n_cu)] = cs
    return _CASES[(family, n_cu)]


def all_cases(n_cu=256):
    return [c for f in FAMILIES for c in family_cases(f, n_cu)]


def cases_of(family, setting, n_cu=256):
    return [c for c in family_cases(family, n_cu) if c.setting() == setting]


def coverage(cases=None):
    """Every predicate on every case -> ({edge: [cases that claim it and reach it]}, {case: [claims that do not hold]}, {edge: [cases that reach it without
    claiming it]}).  A predicate that cannot be put to a case it was not written for does not hold there."""
    cases = all_cases() if cases is None else cases
    table, lost, more = {e: [] for e in EDGES}, {}, {e: [] for e in EDGES}
    for c in cases:
        for e in c.claims:
            if e not in EDGES:
                lost.setdefault(c.name, []).append(e)
        for e, pred in EDGES.items():
            if e in c.claims:
                if pred(c.ctx()):
                    table[e].append(c.name)
                else:
                    lost.setdefault(c.name, []).append(e)
            else:
                try:
                    if pred(c.ctx()):
                        more[e].append(c.name)
                except (IndexError, KeyError, TypeError, ValueError, AttributeError):
                    pass
    return table, lost, more


# =====================================================================================================================================
# the lanewise model and its mutants
# =====================================================================================================================================
MUTANTS = {   # name: (what is wrong, the case that tells it apart)
    "next_dropped": ("the 3' stop pattern without the next lane's reset bits", "sm_bwa_plus_3"),
    "prev_dropped": ("the 5' stop pattern without the previous lane's reset bits", "sm_bwa_plus_5"),
    "tie3_smaller": ("the smaller position wins a 3' tie", "sm_bwa_plus_3"),
    "tie5_larger": ("the larger position wins a 5' tie", "sm_bwa_plus_5"),
    "t_uncorrected": ("T not corrected for the slots past the read", "sm_bwa_plus_3"),
    "pairs_not_carried": ("poly-N pairs not carried across a lane", "ns_poly_n2"),
    "run_not_carried": ("the exact longest run without the lanes before", "ns_poly_n7"),
    "prev_last_none": ("prev_last as `none`", "tr_pairs_across_borders"),
    "edit_g": ("the edit applied to lower-case g", "rp_q15_borders"),
    "edit_outside": ("the edit applied outside the kept window", "rp_windows_and_neighbours"),
    "edit_poly_n": ("the edit seen by poly-N", "rp_windows_and_neighbours"),
    "shorter_to_p-1": ("`shorter` summed to p - 1", "ln_score_0_past_shorter_reads"),
}
# mutants of the schedule: the largest value a field takes between two flushes passes the field's width on the named case (schedule_peak)
SCHEDULE_MUTANTS = dict(
    [("spill_late_lpr%d" % _l, ("the 6-bit fields of LPR %d spilled one iteration late" % _l, "sp_lpr%d" % _l)) for _l in (4, 8, 16, 32)] +
    [("no_mid_chunk_spill", ("the t == 32 spill missing", "sp_lpr64")), ("hq8_every_64", ("HQ8_EVERY doubled twice", "ch_hq8_identical_quality")),
     ("comp_flush_late_narrow", ("the composition_histogram flush one round late", "sp_comp_narrow_16_rounds")),
     ("comp_flush_late_wide", ("the composition_histogram flush one round late", "sp_comp_wide_16_rounds"))])
# mutants no input can tell apart, with the reason (the CPU test asserts the equality on the named family)
EQUIVALENT_MUTANTS = {
    "e_left_out_of_the_5_test": ("`pmax > 0` for `pmax + E > 0`: the first positive prefix of a read lies in a lane whose E is <= 0, so that lane's own pmax is positive too and "
                                 "__any() is true either way; a lane with pmax <= 0 < pmax + E never decides alone", "seams"),
    "stale_prefetch": ("the previous read's bytes where pbase >= n_len: the byte-mask row of vb = 0 clears those registers before anything reads them", "lengths"),
    "p_le_R": ("`p < R` as `p <= R`: at p = R every read has ended, so column 0 is n - shorter = 0, the base cells are 0, and nothing is added", "lengths"),
}
F_FILT_SHIFT = 1


def _rng(lo, hi, W_):
    m = np.zeros(W_ + 2, bool)
    lo, hi = max(lo, 0), min(hi, W_)
    if hi > lo:
        m[lo:hi] = True
    return m


def lanes_read(s, q, o, off, sh, mut=None, prev=None):
    """one read the way trim_filter_accumulate<C, LPR> computes it -> (start, len, flags | filter << 1, the N bin of the post-trim composition), the clamped scores
    of all W slots"""
    Cc, LPR = sh[2], sh[3]
    Wd = Cc * LPR
    jb, pb, bias = (JB[1] if Cc > JB[0] else JB[2]), (PB[1] if LPR <= PB[0] else PB[2]), 1 << (KEY_BIAS[1] if LPR <= KEY_BIAS[0] else KEY_BIAS[2])
    JM, PMX, FK, M32 = (1 << jb) - 1, (1 << pb) - 1, 2 * Wd, 0xFFFFFFFF
    ln = len(s)
    pos = np.arange(Wd + 2)
    lane, j = pos // Cc, pos % Cc
    ws, wq = np.zeros(Wd + 2, np.int64), np.zeros(Wd + 2, np.int64)
    if mut == "stale_prefetch" and prev is not None:      # lanes that load nothing keep the read before: what the byte mask then clears
        ws[:len(prev[0])], wq[:len(prev[0])] = np.frombuffer(prev[0], np.uint8), np.frombuffer(prev[1], np.uint8)
        keep = lane * Cc >= ln
        ws, wq = ws * keep, wq * keep
    ws[:ln], wq[:ln] = np.frombuffer(s, np.uint8), np.frombuffer(q, np.uint8)
    vb = np.clip(ln - lane * Cc, 0, Cc)                   # the byte-mask row of the lane: bytes j >= vb are cleared
    ws, wq = ws * (j < vb), wq * (j < vb)
    ws[Wd:], wq[Wd:] = 0, 0
    nu, gu = ws == 78, (ws == 71) | ((ws == 103) if mut == "edit_g" else False)
    # terminal-N mask: lead = the first non-N position (len: none), trail_start = 1 + the last
    inr = pos < ln
    non = np.nonzero(inr & ~nu)[0]
    lead, trail_start = (int(non[0]), int(non[-1]) + 1) if len(non) else (ln, 0)
    wq = np.where(inr & ((pos < lead) | (pos >= trail_start)), off, wq)
    v = np.where(wq > 127, wq - 256, wq) - off
    qq = np.maximum(v, 0)
    Q = o.quality
    a, n, flags, filt, ret = 0, ln, 0, FILT_NONE, True
    windowed = bool((o.trim_5 or o.trim_3) and not o.qc_only)
    if o.trim_5 and not o.qc_only:
        a, n = (a, 0) if o.trim_5 > n else (a + o.trim_5, n - o.trim_5)
    if o.trim_3 and not o.qc_only:
        n = 0 if o.trim_3 > n else n - o.trim_3
    if n < o.min_read_length or n == 0:
        ret, filt = False, FILT_LENGTH_PRE
    dq = Q - qq
    if windowed:
        dq = np.where((pos >= a) & (pos < a + n), dq, 0)
    dq[Wd:] = 0
    Pin = np.cumsum(dq[:Wd].reshape(LPR, Cc), axis=1)      # lane-local
    run = Pin[:, -1]
    E = np.concatenate([[0], np.cumsum(run)[:-1]])
    T = int(run.sum())
    if not windowed and mut != "t_uncorrected":
        T -= Q * (Wd - ln)
    if not o.qc_only:
        fp3, fp5 = n - 1, 0
        a5, nan2 = min(n, 5), min(n, 2)
        if o.mode == MODE_BWA_PLUS:
            TE = T - E
            Dv = TE[:, None] - Pin                          # the sum behind position (lane, j)
            r3 = np.zeros(Wd + 2, bool)
            r3[:Wd] = (Dv >= 0).ravel()
            r3 &= _rng(a + nan2 + 1, a + n, Wd)
            f5 = r3 & _rng(a + n - a5, a + n, Wd)
            # bits j + 1 and j + 2 of ext: the lane's own, or -- past its last position -- the next lane's (RW::next is 0 behind the row's last lane, where r3 is 0 too)
            e1, e2 = np.concatenate([r3[1:], [False]]), np.concatenate([r3[2:], [False, False]])
            if mut == "next_dropped":
                e1, e2 = e1 & (j + 1 < Cc), e2 & (j + 2 < Cc)
            c3 = ~r3 & ~e1 & e2 & (pos < Wd)
            hit = np.nonzero(c3)[0]
            red = int(hit[-1]) + 1 if len(hit) else 0
            pstar = red - 1 if f5.any() else a + n - a5
            vis = _rng(max(pstar, a), a + n, Wd)[:Wd].reshape(LPR, Cc)
            val = np.concatenate([TE[:, None], Dv[:, :-1]], axis=1)   # S of position (lane, j) = the sum from it on
            jj = np.arange(Cc)[None, :]
            jkey = (JM - jj) if mut == "tie3_smaller" else jj
            k = (((val.astype(np.int64) << jb) + ((bias << jb) | jkey)) & M32) * vis
            kl = k.max(axis=1)
            jdec = (JM - (kl & JM)) if mut == "tie3_smaller" else (kl & JM)
            pa = np.arange(LPR) * Cc - a
            K3 = int(np.where(kl > 0, (((kl >> jb) << pb) + (pa + jdec)) & M32, 0).max())
            if (K3 >> pb) - bias > 0:
                fp3 = (K3 & PMX) - 1
            pmax = Pin.max(axis=1)
            if not o.protect_5 and ((pmax + (0 if mut == "e_left_out_of_the_5_test" else E)) > 0).any():
                P2 = Pin + E[:, None]
                r5 = np.zeros(Wd + 2, bool)
                r5[:Wd] = np.concatenate([E[:, None], P2[:, :-1]], axis=1).ravel() >= 0
                r5 &= _rng(a, a + fp3 - nan2, Wd)
                g5 = r5 & _rng(a, a + a5, Wd)
                m1, m2 = np.concatenate([[False], r5[:-1]]), np.concatenate([[False, False], r5[:-2]])
                if mut == "prev_dropped":
                    m1, m2 = m1 & (j >= 1), m2 & (j >= 2)
                c5 = ~r5 & ~m1 & m2 & (pos < Wd)
                hit = np.nonzero(c5)[0]
                pstar5 = (int(hit[0]) if len(hit) else FK) if g5.any() else a + a5 - 1
                vis5 = _rng(a, min(pstar5 + 1, a + n), Wd)[:Wd].reshape(LPR, Cc)
                jkey = jj if mut == "tie5_larger" else (JM - jj)
                k = (((P2.astype(np.int64) << jb) + ((bias << jb) | jkey)) & M32) * vis5
                kl = k.max(axis=1)
                jdec = (kl & JM) if mut == "tie5_larger" else (JM - (kl & JM))
                K5 = int(np.where(kl > 0, (((kl >> jb) << pb) + (PMX - (pa + jdec))) & M32, 0).max())
                if (K5 >> pb) - bias > 0:
                    fp5 = PMX - (K5 & PMX) + 1
            kept = 0 if fp3 <= fp5 else fp3 - fp5 + 1
        else:
            win = [int(x) for x in qq[a:a + n]]
            fp5, kept, _ = (te.walk_bwa(win, Q) if o.mode == MODE_BWA else te.walk_hard(win, Q, o.protect_5)) if n else (0, 0, None)
        if ret:
            if kept != n:
                flags |= F_QUAL_TRIMMED
            a, n = a + fp5, kept
            if n < o.min_read_length or n == 0:
                ret, filt = False, te.FILT_LENGTH_POST
    win2 = _rng(a, a + n, Wd)
    rep = np.zeros(Wd + 2, bool)
    if o.replace_to_N_q > 0:
        rep = (qq < o.replace_to_N_q) & gu & (win2 if mut != "edit_outside" else (pos < ln))
    if ret:
        K = o.max_num_poly_N
        nw = (nu | (rep if mut == "edit_poly_n" else False)) & win2
        nxt = np.concatenate([nw[1:], [False]])
        if mut == "pairs_not_carried":
            nxt &= j + 1 < Cc
        pairs = (nw & nxt).any()
        if K <= 2:
            trip = K == 0 or bool(nw.any() if K == 1 else pairs)
        elif not pairs:
            trip = False
        else:
            best, lastnon = 0, a
            for lp in range(LPR):              # loc[] inside the lane, excl from the lanes before
                start = lastnon if mut != "run_not_carried" else a
                for p in range(lp * Cc, lp * Cc + Cc):
                    if win2[p] and not nw[p]:
                        start = lastnon = p + 1
                    elif nw[p]:
                        best = max(best, p + 1 - max(start, a))
            trip = best >= K
        if trip:
            flags |= F_POLY_N_SEEN
            if not o.qc_only:
                ret, filt = False, FILT_POLY_N
    cls = np.full(Wd + 2, 7)
    for code, (u, l) in enumerate(((65, 97), (84, 116), (67, 99), (71, 103))):
        cls[((ws == u) | (ws == l)) & win2 & ~rep] = code
    cnt = [int((cls == c).sum()) for c in range(4)]
    if ret and o.average_quality > 0 and int(v[a:a + n].sum()) < te.avg_pass_sum(n, o.average_quality, off):
        ret, filt = False, te.FILT_AVG_Q
    if ret:
        mthr, dthr = lc_thr(n, o.low_complexity_cutoff_ratio), lc_thr(n, o.low_complexity_cutoff_ratio, True)
        trip = mthr is not None and any(c >= mthr for c in cnt)
        if not trip and dthr is not None and sum(c >= dthr for c in cnt) >= 2:
            pv = np.concatenate([[7], cls[:-1]])
            if mut == "prev_last_none":
                pv[j == 0] = 7
            trip = any(x != y and cnt[x] >= dthr and cnt[y] >= dthr and int(((pv == x) & (cls == y))[:Wd].sum()) >= dthr for x in range(4) for y in range(4))
        if trip:
            ret, filt = False, FILT_LOW_COMPLEXITY
    # the post-trim count of N (and n) with the edit, as its composition bin: where the edit shows when no filter looks at it
    cn = int((((ws == 78) | (ws == 110)) & win2).sum()) + int((rep & (win2 if mut != "edit_outside" else True)).sum())
    nbin = te.comp_bin_float(n, cn) if ret else 0
    return ((a, n, flags | F_VALID, nbin) if ret else (0, 0, flags | (filt << F_FILT_SHIFT), 0)), qq


def lanes(case, mutant=None):
    """-> ([array of results per submission], [column 0 of pre_qual per submission]) computed lane by lane for the shape of each submission (a Tiled one: the
    period and the remainder once).  Column 0 the way the read loop and flush_block leave it: one for every slot of a counted read whose (masked) score is 0,
    past the read's end too, less the `shorter` reads of each position"""
    o = case.opt()
    out, col0 = [], []
    for sub in case.subs:
        sh = shape_of(sub_longest(sub))
        if sh is None or case.oracle:             # (a batch for trim_long: not this kernel's; the window family: no adapters in this model)
            out.append(None), col0.append(None)
            continue
        reads = [r for seg in sub for r in seg]
        res = np.zeros(len(reads), te.RESULT_DTYPE)
        slots = np.zeros(sh[1] + 1, np.int64)
        prev = None
        for k, (_, s, q) in enumerate(reads):
            t, qq = lanes_read(s, q, o, case.in_off, sh, mutant, prev if k % sh[3] else None)
            res[k] = t
            slots[:sh[1]] += qq[:sh[1]] == 0
            slots[(len(s) if mutant != "shorter_to_p-1" else len(s) + 1):sh[1]] -= 1     # shorter: the reads with len <= p (the mutant: len <= p - 1)
            prev = (s, q)
        out.append(res)
        col0.append(slots[:min(case.R + (mutant == "p_le_R"), sh[1])])
    return out, col0


def lanes_differ(case, got):
    """None, or the first difference between lanes() and the plain model: the per-read results, then column 0 of pre_qual (from the reads' own scores)"""
    e = case.expected()
    res, col0 = got
    at = 0
    for k, (sub, r) in enumerate(zip(case.subs, res)):
        n = sum(len(seg) for seg in sub)
        if r is None:
            at += n
            continue
        want = np.zeros(n, te.RESULT_DTYPE)
        for x, i in enumerate(e["trace"][at:at + n]):
            want[x] = (i.a, i.kept, i.flags | (i.filt << F_FILT_SHIFT), i.bins[4] if i.bins else 0)
        bad = np.nonzero(r != want)[0]
        if len(bad):
            return "submission %d read %d: lanes %s model %s" % (k, bad[0], r[bad[0]], want[bad[0]])
        ctx = case.ctx()
        ref = np.zeros(min(case.R, len(col0[k])), np.int64)
        if len(col0[k]) > len(ref) and col0[k][len(ref):].any():
            return "submission %d: pre_qual[%d][0] lanes %d, past the context's rows" % (k, len(ref), col0[k][len(ref)])
        for rd_ in (x for seg in sub for x in seg):
            sc = ctx.scores(rd_)[:len(ref)]
            ref[:len(sc)] += sc == 0
        if (ref != col0[k][:len(ref)]).any():
            p = int(np.nonzero(ref != col0[k][:len(ref)])[0][0])
            return "submission %d: pre_qual[%d][0] lanes %d model %d" % (k, p, col0[k][p], ref[p])
        at += n
    return None


def case_named(name, n_cu=256):
    return [c for c in all_cases(n_cu) if c.name == name][0]


def caught(mutant, n_cu=256):
    c = case_named(MUTANTS[mutant][1], n_cu)
    return lanes_differ(c, lanes(c, mutant))


def hq8_peak(n_reads, every, NW=8):
    """the largest value an 8-bit cell of the 1 024-wide shape takes between two flush_hq8 when every read adds 1 to it: the waves of a block that hold a chunk,
    min(reads of the chunk, every) each"""
    chunks = [min(64, n_reads - 64 * k) for k in range(min(NW, (n_reads + 63) // 64))]
    return sum(min(c, every) for c in chunks)


def schedule_peak(name, n_cu=256):
    """-> (the field's largest value under the schedule as it stands, under the mutant, the field's capacity) on the mutant's case"""
    c = case_named(SCHEDULE_MUTANTS[name][1], n_cu)
    if name.startswith("spill_late_lpr"):
        l = int(name[len("spill_late_lpr"):])
        n, it = sub_n(c.subs[0]), iteration(shape_of(LPR_SHAPE[l]), n_cu)
        return field_peak(l, n, it), field_peak(l, n, it, late=1), 63
    if name == "no_mid_chunk_spill":
        n = sub_n(c.subs[0])
        return max(min(n, 64) - MID_CHUNK_SPILL, MID_CHUNK_SPILL), min(n, 64), 63
    if name == "hq8_every_64":
        n = max(sub_n(s) for s in c.subs)
        return hq8_peak(n, HQ8_EVERY), hq8_peak(n, 4 * HQ8_EVERY), 255
    rounds = comp_rounds(sub_n(c.subs[0]), n_cu)
    return min(rounds, COMP_FLUSH_EVERY) * COMP_ROUND, min(rounds, COMP_FLUSH_EVERY + 1) * COMP_ROUND, COMP_FIELD


if __name__ == "__main__":
    t, lost, more = coverage()
    print("claimed  unclaimed  edge")
    for e, v in t.items():
        print("%7d  %9d  %s" % (len(v), len(more[e]), e))
    for f in FAMILIES:
        cs = family_cases(f)
        print("%-12s %3d cases, %9d reads (%7d for the model), %s" % (f, len(cs), sum(c.n_reads() for c in cs), sum(len(c.ctx().reads) for c in cs),
                                                                      ", ".join("%d %s" % (len([c for c in cs if c.setting() == s]), s) for s in SETTINGS)))
    print("%d cases, %d edges; claims that do not hold: %s" % (len(all_cases()), len(t), lost))
    for name, why in EXCLUSIONS.items():
        print("excluded: %s: %s" % (name, why))
    for m, (what, name) in MUTANTS.items():
        print("mutant %-20s %-58s %s: %s" % (m, what, name, caught(m)))
    for m, (what, name) in SCHEDULE_MUTANTS.items():
        print("schedule mutant %-24s %-58s %s: as it stands %d, mutated %d, the field holds %d" % ((m, what, name) + schedule_peak(m)))
    for m, (why, fam) in EQUIVALENT_MUTANTS.items():
        print("equivalent mutant %s (%s): %s" % (m, fam, why))
