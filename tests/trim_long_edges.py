"""A constructed catalogue of inputs for the long-read trim path (trim_long<NW>, long_accumulate and faqcs_launch_trim_long,
faqcs_trim_long_kernel.hip), in the style of tests/trim_edges.py, from which it takes the plain model (Model, run_model), TCase, layout, the
read helpers and the threshold searches.  What sets the two kernels apart from the chunked ones is aimed at here: the 64-position pieces
and 256-position rounds of the two streaming passes and of the walks, with what they carry from piece to piece; the 16-bit fields, which
are right because a read has at most 32 767 bases; the 512-position tiles of long_accumulate and the way its blocks deal out the reads;
what a wave keeps from one read to its next (the length histograms in run-length form); and the adapter window in front of a real walk.
Every case is a named builder of submissions of segments of reads, every edge a PREDICATE over a case's reads and the model's per-read
trace, never over a case's name; coverage() puts every predicate to every case.  The builders take n_cu, the number of compute units the
grids are capped by, and the predicates compute the grids from it.

Eight families: walk, terminal_n, poly_n, fields, transitions, tiles, waves, window.  The reference of the first seven is the plain model
of tests/trim_edges.py; the reference of `window` is OracleEngine, for whole results and the whole counter block, because the model covers
no adapters.

pieces(case): a second model, which restates the PIECEWISE structure of the kernels -- the walks piece by piece with carry, best, seen and
prev_nr, the poly-N run with run_carry, the transitions with prev_cls, the matrices position by position from the packed verdict and the
two terminal runs, the length histograms as each wave's runs -- on numpy rows of 64.  Unmutated it must equal the plain model; MUTANTS are
wrong versions of it, each told apart by a named case.

    python -m tests.trim_long_edges        prints the number of cases per edge, and the mutants
"""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import trim_edges as te
from trim_edges import (F_POLY_N_SEEN, F_QUAL_TRIMMED, F_VALID, FILT_AVG_Q, FILT_LENGTH_POST, FILT_LENGTH_PRE, FILT_LOW_COMPLEXITY, FILT_NONE, FILT_POLY_N,
                        MODE_BWA, MODE_BWA_PLUS, MODE_HARD, NBASE, NQ, Qs, TCase, f32, lc_thr, one, rb, rd)

# restated; test_trim_long_edges_model.py holds each to its source by regex
PIECE, ROUND, LA_TILE, LA_NW, TRIM_LONG_NW = 64, 256, 512, 16, 4
GRID_BLOCKS_PER_CU, LA_BLOCKS_PER_CU = 8, 1
MAX_READ_LENGTH, FAST_READ_LENGTH = 32767, 1024
CONSTANT_SOURCES = {
    "PIECE": ("faqcs_amd/csrc/faqcs_trim_long_kernel.hip", r"const int t = (\d+) \* k \+ lane, i = desc"),
    "ROUND": ("faqcs_amd/csrc/faqcs_trim_long_kernel.hip", r"for \(int cc = 0; cc < len; cc \+= (\d+)\)"),
    "LA_TILE": ("faqcs_amd/csrc/faqcs_trim_long_kernel.hip", r"constexpr int LA_TILE = (\d+),"),
    "LA_NW": ("faqcs_amd/csrc/faqcs_trim_long_kernel.hip", r"constexpr int LA_TILE = \d+, LA_NW = (\d+),"),
    "TRIM_LONG_NW": ("faqcs_amd/csrc/faqcs_trim_plan.h", r"enum \{ FAQCS_TRIM_LONG_NW = (\d+) \};"),
    "GRID_BLOCKS_PER_CU": ("faqcs_amd/csrc/faqcs_trim_plan.h", r"p\.grid = blocks\(n_reads, FAQCS_TRIM_LONG_NW, \(uint32_t\)n_cu \* (\d+)u\);"),
    "MAX_READ_LENGTH": ("include/faqcs_mi.h", r"#define FAQCS_MAX_READ_LENGTH (\d+)"),
    "FAST_READ_LENGTH": ("faqcs_amd/csrc/faqcs_trim_plan.h", r"#define FAQCS_FAST_READ_LENGTH (\d+)"),
}
# statements that hold a constant without a number of their own
STATEMENT_SOURCES = {
    "pass 1 streams four pieces per round": ("faqcs_amd/csrc/faqcs_trim_long_kernel.hip", r"for \(int c = 0; c < len0; c \+= 256\) \{ // four 64-position pieces per round"),
    "long_accumulate: at most one block per compute unit": ("faqcs_amd/csrc/faqcs_trim_long_kernel.hip",
                                                           r"uint32_t g2 = \(a\.n_reads \+ LA_NW - 1\) / LA_NW;\s+if \(g2 > \(uint32_t\)a\.n_cu\) g2 = \(uint32_t\)a\.n_cu;"),
    "long_accumulate deals the reads out by block, round and wave": ("faqcs_amd/csrc/faqcs_trim_long_kernel.hip",
                                                                    r"const uint32_t r0 = blockIdx\.x \+ k \* LA_NW \* gridDim\.x;(.|\n)*?const uint32_t r = r0 \+ wave \* gridDim\.x;"),
    "trim_long deals the reads out by wave": ("faqcs_amd/csrc/faqcs_trim_long_kernel.hip", r"for \(uint32_t r = blockIdx\.x \* NW \+ wave; r < n_reads; r \+= n_waves\)"),
}
E_QUALITY = te.E_QUALITY
F_ADAPTER = 0x20
FAMILIES = ("walk", "terminal_n", "poly_n", "fields", "transitions", "tiles", "waves", "window")
FAMILY_REFERENCE = {f: "model" for f in FAMILIES}
FAMILY_REFERENCE["window"] = "oracle"     # the trim model covers no adapters: OracleEngine alone, whole results and the whole counter block
# what the catalogue leaves out, by name (the CPU test counts them)
EXCLUSIONS = {
    "long_accumulate:flush_after_65535_increments": "`since + LA_NW > 65535` needs about 16 million long reads in one batch on 256 compute units",
    "poly_n:whole_N_piece_narrower_than_64": "only a read's last piece is narrower than 64, and run_carry is not read after it: a wrong run_carry there cannot show "
                                             "(the model's mutant and the kernel's mutation both survive, and must)",
    "walk:first_re-arm_after_step_0": "the area before step 0 is 0, so a window of more than three bases re-arms at step 0: a later first re-arm does not exist",
}


def trim_long_grid(n_reads, n_cu):
    return min((n_reads + TRIM_LONG_NW - 1) // TRIM_LONG_NW, GRID_BLOCKS_PER_CU * n_cu)


def accumulate_grid(n_reads, n_cu):
    return min((n_reads + LA_NW - 1) // LA_NW, LA_BLOCKS_PER_CU * n_cu)


def full_waves(n_cu):
    """W: the waves of a full trim_long grid"""
    return GRID_BLOCKS_PER_CU * n_cu * TRIM_LONG_NW


class LCase(TCase):
    """A TCase of this catalogue: force_long: the case's engine runs under FAQCS_TRIM_LONG=1; device_max_len: not None: every submission goes through
    faqcs_submit_device with that max_read_len (0: the context's capacity); adapters: extra (name, sequence) targets behind the built-in set; the window
    family's expected() is the oracle's"""

    def __init__(self, name, args, subs, claims, R=None, force_long=False, device_max_len=None, adapters=(), error=False, oracle=False):
        self.adapters = list(adapters)
        TCase.__init__(self, name, args, subs, claims, R=R, error=error)
        self.force_long, self.device_max_len, self.oracle = force_long, device_max_len, oracle
        assert self.R >= self.longest and self.R <= MAX_READ_LENGTH

    def opt(self):
        o = TCase.opt(self)
        o.adapter.extend(self.adapters)
        return o

    def expected(self):
        if self._exp is None:
            self._exp = run_oracle(self) if self.oracle else te.run_model(self)
        return self._exp

    def ctx(self):
        if self._ctx is None:
            self._ctx = LCtx(self)
        return self._ctx

    def max_len(self, k):
        """what the launcher is told of submission k"""
        longest = max([len(r[1]) for seg in self.subs[k] for r in seg] or [0])
        return longest if self.device_max_len is None else (self.device_max_len or self.R)

    def runs_trim_long(self, k):
        return self.force_long or self.max_len(k) > FAST_READ_LENGTH


def run_oracle(case):
    from oracle_engine import OracleEngine

    from faqcs_amd import driver
    from faqcs_amd.engine import FaqcsError

    ora = OracleEngine(case.opt(), case.R, case.in_off)
    try:
        results = [ora.process(*driver.pack_segments(sub)) for sub in case.subs]
        return dict(results=results, counters=ora.counters(), error=0, trace=[])
    except FaqcsError as x:
        return dict(results=None, counters=None, error=x.code, trace=[])
    finally:
        ora.close()


class LCtx(te.Ctx):
    def __init__(self, case):
        te.Ctx.__init__(self, case)
        self.n_cu = case.n_cu
        e = case.expected()
        self.res = np.concatenate(e["results"]) if e["results"] else None
        if case.oracle:
            self.rt = []
        self._cache = {}

    def win(self, k):
        """(scores of the window the walk of read k sees, as numpy; its first position in the read)"""
        if k not in self._cache:
            (_, s, q), i = self.rt[k]
            q = bytearray(q)
            n = len(s)
            lead = n - len(s.lstrip(b"N"))
            trail = n - len(s.rstrip(b"N"))
            q[:lead] = bytes([self.off]) * lead
            q[n - trail:] = bytes([self.off]) * min(trail, n)
            v = np.frombuffer(bytes(q), np.int8).astype(np.int64) - self.off
            a = self.o.trim_5 if self.o.trim_5 and not self.o.qc_only and self.o.trim_5 <= n else 0
            self._cache[k] = (np.maximum(v, 0)[a:a + i.pre], a)
        return self._cache[k]

    def areas(self, k, desc=True):
        """-> (area before every step, area after it) of a walk over the whole window of read k"""
        sc, _ = self.win(k)
        d = self.o.quality - (sc[::-1] if desc else sc)
        after = np.cumsum(d)
        return after - d, after

    def walked(self):
        return [k for k, (_, i) in enumerate(self.rt) if i.w]

    def sub_reads(self):
        return [[r for seg in sub for r in seg] for sub in self.case.subs]


EDGES = {}


def edge(name):
    def reg(f):
        EDGES[name] = f
        return f
    return reg


def W(i):
    return i.w or {}


# =====================================================================================================================================
# edges
# =====================================================================================================================================
# ---- walk ---------------------------------------------------------------------------------------------------------------------------
WALK_LENGTHS = (1025, 4096, 32767)
RUNS = (255, 256, 257, 4095, 4096, 4097, 16384)
MAX_STEPS = (63, 64, 65, 255, 256, 257)
SEAMS = (64, 256, 16384)
FIXED5 = (1, 63, 64, 65)
WALK_MODES = {"bwa_plus": [], "bwa_plus_5off": ["--5trim_off"], "bwa": ["--mode", "BWA"], "hard": ["--mode", "HARD"], "hard_5off": ["--mode", "HARD", "--5trim_off"]}
WALK_BASE = ["--min_L", "1", "--lc", "1.0", "-n", "40000"]


def _mode_is(c, mname):
    return (c.o.mode, bool(c.o.protect_5)) == {"bwa_plus": (MODE_BWA_PLUS, False), "bwa_plus_5off": (MODE_BWA_PLUS, True), "bwa": (MODE_BWA, False),
                                                "hard": (MODE_HARD, False), "hard_5off": (MODE_HARD, True)}[mname]


def _low_run(c, q, front):
    """the length of the run of bytes below offset + Q at the front (the end) of q"""
    t = q if front else q[::-1]
    lim = c.off + c.o.quality
    n = 0
    while n < len(t) and t[n] < lim:
        n += 1
    return n


def _tails_cut(c, fixed5):
    """{(raw length, low tail)} of the reads whose low tail, and nothing else, the walk cut"""
    return {(i.n0, _low_run(c, q, False)) for (_, s, q), i in c.rt if i.flags & F_VALID and i.a == fixed5 and i.a + i.kept == i.n0 - _low_run(c, q, False) and _low_run(c, q, False)}


def _heads_cut(c, fixed5):
    return {(i.n0, _low_run(c, q[fixed5:], True)) for (_, s, q), i in c.rt if i.flags & F_VALID and i.a + i.kept == i.n0 and i.a == fixed5 + _low_run(c, q[fixed5:], True) and i.a > fixed5}


def _want_runs(fixed5=0, lengths=WALK_LENGTHS):
    """(raw length, run) of the low tails and heads a walk can cut and leave a read: BWA_plus leaves nothing of one base, so len - 1 and len are asked of the inputs alone"""
    return {(n, t) for n in lengths for t in RUNS if t < n - fixed5 - 1}


def _want(mn, q):
    """every run at 32 767 bases under BWA_plus at -q 5; under the other modes and at -q 41 every run at 1 025 and 4 096 bases and the far one at 32 767"""
    return _want_runs() if (mn, q) == ("bwa_plus", 5) else _want_runs(0, (1025, 4096)) | {(MAX_READ_LENGTH, 16384)}


for _mn in ("bwa_plus", "bwa_plus_5off", "bwa", "hard", "hard_5off"):
    for _q in (5, 41):
        if _mn.startswith("hard") and _q == 41:
            continue        # no score exceeds 41: HARD cuts nothing (its own edge below)
        edge("walk:%s:q%d:low_tails_of_255..16384_are_cut" % (_mn, _q))(lambda c, mn=_mn, q=_q: _mode_is(c, mn) and c.o.quality == q and not c.o.trim_5 and _tails_cut(c, 0) >= _want(mn, q))
        if _q == 41:     # a good base scores 41 = Q: the area never falls, and the 3' walk crosses the whole read, 512 pieces of it, into the low head
            edge("walk:%s:q41:3'_walk_crosses_a_read_of_32767_into_its_low_head" % _mn)(lambda c, mn=_mn: _mode_is(c, mn) and c.o.quality == 41 and any(
                i.n0 == MAX_READ_LENGTH and i.w["steps3"] >= i.n0 - 3 and _low_run(c, q_, True) == 16384 and i.w["step3"] >= i.n0 - 3 for (_, s, q_), i in c.rt if i.w))
        elif _mn in ("bwa_plus", "hard"):
            edge("walk:%s:q%d:low_heads_of_255..16384_are_cut" % (_mn, _q))(lambda c, mn=_mn, q=_q: _mode_is(c, mn) and c.o.quality == q and not c.o.trim_5 and _heads_cut(c, 0) >= _want(mn, q))
        else:
            edge("walk:%s:q%d:low_heads_are_kept" % (_mn, _q))(lambda c, mn=_mn, q=_q: _mode_is(c, mn) and c.o.quality == q and not c.o.trim_5 and
                                                                {(i.n0, _low_run(c, q_, True)) for (_, s, q_), i in c.rt if i.flags & F_VALID and i.a == 0 and i.kept == i.n0} >= _want(mn, q))
edge("walk:low_tails_and_heads_of_len-1_and_len_at_1025_4096_32767")(lambda c: not c.o.trim_5 and all(
    any(len(q) == n and _low_run(c, q, front) == t for _, s, q in c.reads) for n in WALK_LENGTHS for t in (n - 1, n) for front in (False, True)))
edge("walk:hard:q41_cuts_nothing")(lambda c: c.o.mode == MODE_HARD and c.o.quality == 41 and len(c.rt) > 20 and all(i.kept == i.n0 for i in c.trace))
for _n in (1025, 32767):
    edge("walk:bwa_plus:low_throughout_at_%d:final_pos_3<=final_pos_5" % _n)(lambda c, n=_n: c.o.mode == MODE_BWA_PLUS and not c.o.protect_5 and any(
        i.n0 == n and i.pre == n and i.w and i.w["f3"] <= i.w["f5"] and i.filt == FILT_LENGTH_POST and _low_run(c, q, True) == n for (_, s, q), i in c.rt))
    edge("walk:low_throughout_at_%d:bwa_and_hard" % _n)(lambda c, n=_n: c.o.mode in (MODE_BWA, MODE_HARD) and any(
        i.n0 == n and i.w and _low_run(c, q, True) == n and i.kept == (1 if c.o.mode == MODE_BWA else n) for (_, s, q), i in c.rt))
for _st in MAX_STEPS:
    edge("walk:bwa_plus:3'_maximum_at_step_%d_of_a_walk_that_ends_pieces_later" % _st)(lambda c, st=_st: c.o.mode == MODE_BWA_PLUS and any(
        W(i).get("step3") == st and (i.w["steps3"] - 1) // PIECE > st // PIECE for i in c.trace))
    edge("walk:bwa_plus:5'_maximum_at_step_%d_of_a_walk_that_ends_pieces_later" % _st)(lambda c, st=_st: c.o.mode == MODE_BWA_PLUS and any(
        W(i).get("step5") == st and (i.w["steps5"] - 1) // PIECE > st // PIECE for i in c.trace))
    edge("walk:bwa:maximum_at_step_%d_of_a_walk_that_ends_pieces_later" % _st)(lambda c, st=_st: c.o.mode == MODE_BWA and any(
        W(i).get("step3") == st and (i.w["steps3"] - 1) // PIECE > st // PIECE for i in c.trace))


def _tie_across_pieces(c, k):
    """the largest area of read k's 3' walk is reached at visited steps of two pieces, and the cut is the first of them"""
    i = c.rt[k][1]
    _, after = c.areas(k)
    after = after[:i.w["steps3"]]
    if not len(after) or after.max() <= 0:
        return False
    at = np.nonzero(after == after.max())[0]
    return len({int(t) // PIECE for t in at}) >= 2 and i.w["step3"] == int(at[0])


edge("walk:two_equal_maxima_in_different_pieces_the_earlier_wins")(lambda c: c.o.mode in (MODE_BWA_PLUS, MODE_BWA) and any(_tie_across_pieces(c, k) for k in c.walked()))


def _rearm3(c, k):
    """R(t) of read k's 3' BWA_plus walk over every step of the window (trim.cpp:739)"""
    before, _ = c.areas(k)
    n = len(before)
    return (before >= 0) & (np.arange(n) < n - 1 - min(2, n))


def _stop_rule(c, S, kind):
    for k in c.walked():
        i = c.rt[k][1]
        if c.o.mode != MODE_BWA_PLUS or i.pre < S + 8:
            continue
        R = _rearm3(c, k)
        _, after = c.areas(k)
        if kind == "none_at_63_none_at_0":   # ends on step S, through prev_nr; the step behind it would have been a new maximum
            if R[:S - 1].all() and not R[S - 1] and not R[S] and i.w["steps3"] == S + 1 and after[S + 1] > after[:S + 1].max():
                return True
        elif kind == "rearm_at_63_then_two_without":
            if R[:S].all() and not R[S] and not R[S + 1] and i.w["steps3"] == S + 2 and i.w["step3"] == S + 1:
                return True
        elif kind == "none_at_62_rearm_at_63":
            if R[:S - 2].all() and not R[S - 2] and R[S - 1] and not R[S] and not R[S + 1] and i.w["steps3"] == S + 2:
                return True
    return False


for _S in SEAMS:
    for _kind in ("none_at_63_none_at_0", "rearm_at_63_then_two_without", "none_at_62_rearm_at_63"):
        edge("walk:bwa_plus:stop_rule_at_seam_%d:%s" % (_S, _kind))(lambda c, S=_S, kind=_kind: _stop_rule(c, S, kind))
edge("walk:bwa_plus:re-arm_at_step_0_then_thousands_of_re-arming_steps")(lambda c: c.o.mode == MODE_BWA_PLUS and any(
    c.rt[k][1].w["steps3"] >= 4000 and _rearm3(c, k)[:c.rt[k][1].w["steps3"] - 3].all() for k in c.walked() if c.rt[k][1].pre > 4003))
for _S in (64, 256):
    edge("walk:bwa:first_failing_step_at_lane_0_of_piece_%d" % (_S // PIECE))(lambda c, S=_S: c.o.mode == MODE_BWA and any(
        c.rt[k][1].w["steps3"] == S and c.rt[k][1].pre > S + 2 and c.areas(k)[1][S] > c.areas(k)[1][:S].max() for k in c.walked()))
    edge("walk:bwa:first_failing_step_at_lane_63_of_piece_%d" % (_S // PIECE - 1))(lambda c, S=_S: c.o.mode == MODE_BWA and any(
        c.rt[k][1].w["steps3"] == S - 1 and c.rt[k][1].pre > S + 2 for k in c.walked()))


def _hard_only_good(c, pos):
    """reads whose only score above Q lies at window position pos -> their Infos"""
    out = []
    for k in c.walked():
        sc, _ = c.win(k)
        hi = np.nonzero(sc > c.o.quality)[0]
        if len(hi) == 1 and hi[0] == pos:
            out.append(c.rt[k][1])
    return out


edge("walk:hard:first_good_score_at_position_1")(lambda c: c.o.mode == MODE_HARD and any(i.w["f3"] == 1 and i.pre % PIECE in (1, 12) for i in _hard_only_good(c, 1)) and
                                                 len({i.pre % PIECE for i in _hard_only_good(c, 1)}) >= 2)
edge("walk:hard:good_score_only_at_position_0_is_not_looked_at")(lambda c: c.o.mode == MODE_HARD and any(i.w["f3"] == i.pre - 1 and i.kept == i.pre for i in _hard_only_good(c, 0)))
edge("walk:hard:first_good_score_inside_the_last_piece")(lambda c: c.o.mode == MODE_HARD and any(i.w["f3"] == 5 and (i.pre - 1 - 5) // PIECE == (i.pre - 1) // PIECE for i in _hard_only_good(c, 5)))
for _S in (64, 256):
    edge("walk:hard:5'_scan_bounded_by_pos_3_on_seam_%d" % _S)(lambda c, S=_S: c.o.mode == MODE_HARD and not c.o.protect_5 and any(
        i.w["f3"] == S and i.w["f5"] == 0 and i.kept == S + 1 for i in _hard_only_good(c, S)))
for _f in FIXED5:
    edge("walk:behind_5end_%d:tails_heads_and_seams" % _f)(lambda c, f=_f: c.o.trim_5 == f and c.o.mode == MODE_BWA_PLUS and not c.o.protect_5 and
                                                           _tails_cut(c, f) >= _want_runs(f, (1025 + f, 4096 + f)) and _heads_cut(c, f) >= _want_runs(f, (1025 + f, 4096 + f)) and
                                                           all(_stop_rule(c, S, kind) for S in (64, 256) for kind in ("none_at_63_none_at_0", "rearm_at_63_then_two_without", "none_at_62_rearm_at_63")) and
                                                           any(_tie_across_pieces(c, k) for k in c.walked()))

# ---- terminal_n ---------------------------------------------------------------------------------------------------------------------
N_RUNS = (63, 64, 65, 255, 256, 257, 511, 512, 513)


def _nrun(s, ch, front):
    t = s if front else s[::-1]
    return len(t) - len(t.lstrip(ch))


# (scores of 40 under the run and low bases inwards of it: the walk crosses a masked run and takes the low bases; a run that is not masked stops it at once)
edge("tn:leading_runs_of_63..513_are_masked")(lambda c: {_nrun(s, b"N", True) for (_, s, q), i in c.rt if i.flags & F_VALID and i.a == _nrun(s, b"N", True) + 4 and q[0] == c.off + 40} >= set(N_RUNS))
edge("tn:trailing_runs_of_63..513_are_masked")(lambda c: {_nrun(s, b"N", False) for (_, s, q), i in c.rt if i.flags & F_VALID and i.n0 - i.a - i.kept == _nrun(s, b"N", False) + 4 and q[-1] == c.off + 40} >= set(N_RUNS))
for _n in (1025, 32767):
    edge("tn:runs_of_len-1_at_%d" % _n)(lambda c, n=_n: {(_nrun(s, b"N", True), _nrun(s, b"N", False)) for (_, s, _), i in c.rt if i.n0 == n} >= {(n - 1, 0), (0, n - 1)})
    edge("tn:all_N_at_%d" % _n)(lambda c, n=_n: any(i.n0 == n and s == b"N" * n and q[0] == c.off + 40 and i.qsum in (0, None) for (_, s, q), i in c.rt))
edge("tn:lead_and_trail_both_32767")(lambda c: any(s == b"N" * MAX_READ_LENGTH for _, s, _ in c.reads))
edge("tn:N..N_X_N..N")(lambda c: any(_nrun(s, b"N", True) + _nrun(s, b"N", False) == len(s) - 1 and len(s) > 1024 and _nrun(s, b"N", True) >= 512 and _nrun(s, b"N", False) >= 512 for _, s, _ in c.reads))
edge("tn:n_at_an_end_is_not_masked")(lambda c: any(s[:1] == b"n" and s[1:65] == b"N" * 64 and i.a == 0 and i.flags & F_VALID for (_, s, _), i in c.rt) and
                                     any(s[-1:] == b"n" and s[-65:-1] == b"N" * 64 and i.a + i.kept == i.n0 and i.flags & F_VALID for (_, s, _), i in c.rt))
edge("tn:n_inside_a_run_stops_it")(lambda c: any(s[:130] == b"N" * 70 + b"n" + b"N" * 59 and i.a == 70 and i.flags & F_VALID for (_, s, _), i in c.rt) and
                                   any(s[-130:] == b"N" * 59 + b"n" + b"N" * 70 and i.a + i.kept == i.n0 - 70 and i.flags & F_VALID for (_, s, _), i in c.rt))
edge("tn:score_above_41_under_a_terminal_N")(lambda c: not c.error and any(s[-70:] == b"N" * 70 and min(q[-70:]) > c.off + 41 for _, s, q in c.reads) and
                                             any(s[:70] == b"N" * 70 and min(q[:70]) > c.off + 41 for _, s, q in c.reads))
edge("tn:score_above_41_under_a_terminal_n_is_an_error")(lambda c: c.error == E_QUALITY and c.case.longest > 1024 and any(s[-1:] == b"n" and s[-2:-1] == b"N" and q[-1] > c.off + 41 for _, s, q in c.reads))

# ---- poly_n -------------------------------------------------------------------------------------------------------------------------
POLY_K = (2, 7, 64, 65, 129, 300)


def _longest_run(s):
    """(start, length) of the longest run of upper-case N (the first of them)"""
    a = np.frombuffer(s, np.uint8) == 78
    if not a.any():
        return 0, 0
    d = np.diff(np.concatenate(([0], a.view(np.int8), [0])))
    st, en = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    k = int(np.argmax(en - st))
    return int(st[k]), int(en[k] - st[k])


def poly_offsets(k):
    return tuple(range(k + 1)) if k <= 7 else (0, 1, 63, 64, 65)


def _poly_edge(c, k, qc):
    if c.o.max_num_poly_N != k or bool(c.o.qc_only) != qc:
        return False
    got = set()
    for (_, s, _), i in c.rt:
        st, ln = _longest_run(s)
        if ln and i.a == 0 and i.pre == i.n0 and i.npoly == ln and ((i.filt == FILT_POLY_N) if not qc else bool(i.flags & F_POLY_N_SEEN and i.flags & F_VALID)) == (ln >= k):
            for seam in (PIECE, ROUND):
                for m in (1, 2, 3):
                    if 0 <= m * seam - st <= 65:
                        got.add((ln - k, seam, m * seam - st))
    return got >= {(d, seam, j) for d in (-1, 0, 1) for seam in (PIECE, ROUND) for j in poly_offsets(k)}


for _k in POLY_K:
    edge("pn:-n_%d:runs_of_k-1_k_k+1_from_64m-j_and_256m-j" % _k)(lambda c, k=_k: _poly_edge(c, k, False))
    edge("pn:-n_%d:the_same_under_qc_only" % _k)(lambda c, k=_k: _poly_edge(c, k, True))


def _run_at(c, start, length, n=None):
    return any(_longest_run(s) == (start, length) and i.npoly == length and (n is None or i.n0 == n) and i.pre == i.n0 and (i.filt == FILT_POLY_N) == (length >= c.o.max_num_poly_N)
               for (_, s, _), i in c.rt)


edge("pn:run_of_one_whole_piece")(lambda c: not c.o.qc_only and c.o.max_num_poly_N == 64 and _run_at(c, 64, 64) and _run_at(c, 256, 64))
edge("pn:run_of_two_whole_pieces")(lambda c: not c.o.qc_only and c.o.max_num_poly_N == 129 and _run_at(c, 64, 128) and _run_at(c, 192, 128))
edge("pn:run_of_63+64+1_over_three_pieces")(lambda c: not c.o.qc_only and c.o.max_num_poly_N == 129 and _run_at(c, 1, 128) and _run_at(c, 193, 128))
for _w in (1, 63, 64):
    edge("pn:run_ends_at_the_window's_end_in_a_last_piece_of_%d" % _w)(lambda c, w=_w: not c.o.qc_only and any(
        _run_at(c, n - ln, ln, n) for n in (1024 + w, 1088 + w) for ln in (c.o.max_num_poly_N, c.o.max_num_poly_N - 1) if ln > 0))
edge("pn:last_piece_all_N")(lambda c: not c.o.qc_only and any(_run_at(c, n - ln, ln, n) for n in (1034,) for ln in (c.o.max_num_poly_N,) if ln >= 74))
edge("pn:run_broken_by_n")(lambda c: any(b"N" * 40 + b"n" + b"N" * 40 in s and i.npoly == 40 and s.find(b"n") % PIECE == 0 for (_, s, _), i in c.rt))
edge("pn:run_shortened_by_the_3'_and_the_5'_cut")(lambda c: c.o.max_num_poly_N >= 64 and any(
    i.flags & F_VALID and i.npoly == c.o.max_num_poly_N - 1 and _longest_run(s)[1] == c.o.max_num_poly_N and i.a + i.kept < i.n0 and i.a == 0 for (_, s, _), i in c.rt) and any(
    i.flags & F_VALID and i.npoly == c.o.max_num_poly_N - 1 and _longest_run(s)[1] == c.o.max_num_poly_N and i.a > 0 and i.a % PIECE for (_, s, _), i in c.rt))
edge("pn:terminal_runs_count_as_runs")(lambda c: not c.o.qc_only and all(any(_longest_run(s) == (0 if front else i.n0 - ln, ln) and i.filt == FILT_POLY_N and i.pre == i.n0 for (_, s, _), i in c.rt)
                                                                         for ln in (c.o.max_num_poly_N, c.o.max_num_poly_N + 1) for front in (True, False)) and
                                       any(s == b"N" * 1025 and i.filt == FILT_POLY_N for (_, s, _), i in c.rt))

# ---- fields -------------------------------------------------------------------------------------------------------------------------
M = MAX_READ_LENGTH
COMPOSITIONS = {"all_A": b"A" * M, "all_T": b"T" * M, "all_C": b"C" * M, "all_G": b"G" * M, "all_N": b"N" * M, "A_T_halves": b"A" * 16384 + b"T" * 16383,
                "C_G_halves": b"C" * 16384 + b"G" * 16383, "AT_pairs": (b"AT" * 16384)[:M], "TCTG_quads": (b"TCTG" * 8192)[:M]}


def _field_lc(c, which, di):
    """a read of 32 767 bases of composition `which` lies at the threshold (filtered) or one count below it (kept)"""
    s0 = COMPOSITIONS[which]
    out = set()
    for (_, s, _), i in c.rt:
        if s == s0 and i.counts and i.wlen == M:
            t = lc_thr(M, c.o.low_complexity_cutoff_ratio, di)
            v = i.dmax if di else i.cmax
            if True:      # (TCTG: the count of T, 16 384, and the count of TC, 8 192, give the same product: both tests sit on the threshold)
                out.add("at" if (t == v and i.filt == FILT_LOW_COMPLEXITY) else "below" if (t is None or t == v + 1) and i.flags & F_VALID else "")
    return out


for _w in ("all_A", "all_T", "all_C", "all_G", "A_T_halves", "C_G_halves"):
    for _where in ("at", "below"):
        edge("fd:%s:base_count_%s_the_threshold" % (_w, _where))(lambda c, w=_w, where=_where: where in _field_lc(c, w, False))
for _w in ("AT_pairs", "TCTG_quads"):
    for _where in ("at", "below"):
        edge("fd:%s:transition_count_%s_the_threshold" % (_w, _where))(lambda c, w=_w, where=_where: where in _field_lc(c, w, True))
edge("fd:all_N:counts_nothing_and_is_kept")(lambda c: any(s == COMPOSITIONS["all_N"] and i.flags & F_VALID and i.cmax == 0 and i.bins[4] == 10000 for (_, s, _), i in c.rt))
edge("fd:composition_bin_of_count=len_pre_and_post")(lambda c: {k for (_, s, _), i in c.rt if i.n0 == M and i.bins for k in range(5) if i.pre_bin[k] == 10000 and i.bins[k] == 10000} == set(range(5)))
edge("fd:composition_bins_of_the_16384/16383_split")(lambda c: all(any(s == COMPOSITIONS[w] and i.bins == i.pre_bin and (i.pre_bin[k], i.pre_bin[k2]) == (te.comp_bin_float(M, 16384), te.comp_bin_float(M, 16383))
                                                                       for (_, s, _), i in c.rt) for w, k, k2 in (("A_T_halves", 0, 1), ("C_G_halves", 2, 3))))
edge("fd:composition_bins_post_trim_on_a_kept_length")(lambda c: any(i.n0 == M and i.flags & F_VALID and i.kept == M - 7 and s[:i.kept] == b"A" * i.kept and i.bins[0] == 10000 and i.pre_bin[0] < 10000
                                                                     for (_, s, _), i in c.rt) and
                                                       any(i.n0 == M and i.flags & F_VALID and i.kept == M - 7 and i.bins[0] == te.comp_bin_float(M - 7, 16384) and s[:16384] == b"A" * 16384 for (_, s, _), i in c.rt))
edge("fd:quality_all_offset+41")(lambda c: any(i.n0 == M and set(q) == {c.off + 41} and i.flags & F_VALID and i.qsum == 41 * M for (_, s, q), i in c.rt))
for _b in (0x80, 0xFF):
    edge("fd:quality_all_0x%02X:negative_sum_clamped" % _b)(lambda c, b=_b: any(i.n0 == M and set(q) == {b} and i.flags & F_VALID and i.qsum == (b - 256 - c.off) * M for (_, s, q), i in c.rt))
edge("fd:ascii_64")(lambda c: c.off == 64 and any(i.n0 == M and i.flags & F_VALID and i.qsum == 41 * M for i in c.trace) and any(i.n0 == M and i.qsum < 0 for i in c.trace))
edge("fd:result_offset_32766_length_1")(lambda c: any(i.flags & F_VALID and (i.a, i.kept) == (M - 1, 1) for i in c.trace))
edge("fd:result_offset_0_length_32767")(lambda c: any(i.flags & F_VALID and (i.a, i.kept) == (0, M) for i in c.trace))

# ---- transitions --------------------------------------------------------------------------------------------------------------------
TR_LENGTHS = (1025, 4096, 32767)
_CLS = np.full(256, 4, np.int64)
for _k, _ch in enumerate(b"ATCG"):
    _CLS[_ch] = _CLS[_ch | 32] = _k


def _window_cls(c, k):
    """classes A T C G / none of the bases the low-complexity test of read k sees (--replace_to_N_q applied)"""
    (_, s, q), i = c.rt[k]
    a = i.a if i.flags & F_VALID else (c.o.trim_5 if c.o.trim_5 and not c.o.qc_only else 0)
    ws = np.frombuffer(s, np.uint8)[a:a + i.wlen].copy()
    if c.o.replace_to_N_q > 0:
        sc = np.maximum(np.frombuffer(q, np.int8).astype(np.int64)[a:a + i.wlen] - c.off, 0)
        ws[(ws == 71) & (sc < c.o.replace_to_N_q)] = 78
    return _CLS[ws]


def _seam_pair(c, n, seam, kind):
    """at window length n a read with thr2 transitions (filtered) and one with thr2 - 1 (kept); kind: "pair": both have the commonest transition across the seam;
    "no_pair": the kept one has a non-base in front of the seam and a base behind it"""
    t2 = lc_thr(n, c.o.low_complexity_cutoff_ratio, True)
    got = set()
    for k, ((_, s, q), i) in enumerate(c.rt):
        if i.counts and i.wlen == n and i.cmax < (lc_thr(n, c.o.low_complexity_cutoff_ratio) or n + 1) and i.dmax in (t2, t2 - 1) and (i.filt == FILT_LOW_COMPLEXITY) == (i.dmax == t2):
            cls = _window_cls(c, k)
            a, b = cls[seam - 1], cls[seam]
            if kind == "pair" and a != 4 and b != 4 and a != b:
                got.add(i.dmax - t2)
            if kind == "no_pair" and a == 4 and b != 4 and cls[seam + 1] == 4:
                got.add(i.dmax - t2)
    return got


def last_seam(n):
    return (n - 1) // PIECE * PIECE


for _n in TR_LENGTHS:
    for _sname, _seam in (("63|64", 64), ("255|256", 256), ("last", None)):
        edge("tr:%d:deciding_pair_on_seam_%s" % (_n, _sname))(lambda c, n=_n, seam=_seam: not c.o.trim_5 and not c.o.replace_to_N_q and
                                                               _seam_pair(c, n, seam or last_seam(n), "pair") == {0, -1})
    edge("tr:%d:non-base_at_lane_63_makes_no_pair_at_lane_0" % _n)(lambda c, n=_n: not c.o.trim_5 and -1 in _seam_pair(c, n, 64, "no_pair") and -1 in _seam_pair(c, n, 256, "no_pair") and
                                                                   any(s[63:65] == b"NG" for _, s, _ in c.reads) and any(s[255:257] == b"RG" for _, s, _ in c.reads))
    edge("tr:%d:behind_a_5'_cut_that_moves_the_seam" % _n)(lambda c, n=_n: c.o.trim_5 == 7 and _seam_pair(c, min(n, M - 7), 64, "pair") == {0, -1} and _seam_pair(c, min(n, M - 7), 256, "pair") == {0, -1} and
                                                           any(i.n0 == min(n + 7, M) for i in c.trace))


def _replaced_g(c, lane):
    """--replace_to_N_q: two reads that differ in the score of one G at window position 63 (64): 14 -> N, one transition fewer, kept; 15 -> filtered"""
    got = set()
    for k, ((_, s, q), i) in enumerate(c.rt):
        p = 63 + lane
        if i.counts and i.a == 0 and s[p:p + 1] == b"G" and q[p] - c.off in (14, 15):
            t2 = lc_thr(i.wlen, c.o.low_complexity_cutoff_ratio, True)
            got.add((q[p] - c.off, i.dmax - t2, i.filt))
    return got >= {(14, -1, FILT_NONE), (15, 0, FILT_LOW_COMPLEXITY)}


edge("tr:replace_to_N_q:G_on_lane_63_decides")(lambda c: c.o.replace_to_N_q == 15 and _replaced_g(c, 0))
edge("tr:replace_to_N_q:G_on_lane_0_decides")(lambda c: c.o.replace_to_N_q == 15 and _replaced_g(c, 1))

# ---- tiles --------------------------------------------------------------------------------------------------------------------------
TILE_LENGTHS = (511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 32256, 32767)


def phase_read(n, ph, off=33):
    """quality offset + (p + ph) % 42, base ATCGN[(p + 2 ph) % 5]: a tile that is shifted, doubled or dropped changes the four matrices"""
    p = np.arange(n)
    return (b"@p", np.frombuffer(b"ATCGN", np.uint8)[(p + 2 * ph) % 5].tobytes(), (off + (p + ph) % 42).astype(np.uint8).tobytes())


def _is_phase(r, ph=None):
    n = len(r[1])
    return n >= 5 and any(r[1:] == phase_read(n, k)[1:] for k in ((ph,) if ph is not None else (0, 17)))


for _n in TILE_LENGTHS:
    edge("tl:max_len_%d_two_phases" % _n)(lambda c, n=_n: len(c.case.subs) == 1 and c.case.max_len(0) == n and c.case.runs_trim_long(0) and c.case.R == n and
                                          sum(1 for r in c.reads if len(r[1]) == n and _is_phase(r)) >= 2 and any(len(r[1]) < n for r in c.reads) and all(i.flags & F_VALID for i in c.trace))
WINDOWS = ((512, 1024), (511, 513), (0, 512), (513, None))


def _windows(c):
    return {(i.a, i.a + i.kept if i.a + i.kept < i.n0 else None) for (r, i) in c.rt if i.flags & F_VALID and i.n0 > 1024 and (_is_phase(r) or i.w and i.flags & F_QUAL_TRIMMED)}


for _a, _b in WINDOWS:
    edge("tl:kept_window_%d_%s_by_fixed_cuts" % (_a, _b or "len"))(lambda c, a=_a, b=_b: (c.o.trim_5 or c.o.trim_3) and (a, b) in _windows(c))
    edge("tl:kept_window_%d_%s_by_a_walk" % (_a, _b or "len"))(lambda c, a=_a, b=_b: not c.o.trim_5 and not c.o.trim_3 and (a, b) in _windows(c))
edge("tl:terminal_runs_end_and_begin_on_511_512_513")(lambda c: {_nrun(s, b"N", True) for _, s, _ in c.reads} >= {511, 512, 513} and
                                                      {len(s) - _nrun(s, b"N", False) for _, s, _ in c.reads if len(s) > 1024} >= {511, 512, 513})


def _low_g(c):
    """where a G below --replace_to_N_q lies: (position, inside the kept window)"""
    out = set()
    for (_, s, q), i in c.rt:
        if i.flags & F_VALID and c.o.replace_to_N_q > 0:
            for p in (511, 512):
                if s[p:p + 1] == b"G" and q[p] - c.off < c.o.replace_to_N_q:
                    out.add((p, i.a <= p < i.a + i.kept))
    return out


edge("tl:replace_to_N_q:low_G_either_side_of_a_tile_border_inside_and_outside_the_window")(lambda c: _low_g(c) >= {(511, True), (512, True), (511, False), (512, False)})
edge("tl:R_32767_under_a_longest_read_of_1025")(lambda c: c.case.R == MAX_READ_LENGTH and c.case.longest == 1025)


def batch_sizes(n_cu):
    return (1, 15, 16, 17, LA_NW * n_cu - 1, LA_NW * n_cu, LA_NW * n_cu + 1, 2 * LA_NW * n_cu + 1)


edge("tl:batches_of_1_15_16_17_and_either_side_of_a_full_grid")(lambda c: [len(sub) for sub in c.sub_reads()] == list(batch_sizes(c.n_cu)) and
                                                               [accumulate_grid(len(sub), c.n_cu) for sub in c.sub_reads()] == [1, 1, 1, 2, c.n_cu, c.n_cu, c.n_cu, c.n_cu] and
                                                               all(max(len(r[1]) for r in sub) == 1025 and sorted(len(r[1]) for r in sub)[-2:-1] in ([], [40]) or len(sub) == 1 for sub in c.sub_reads()))
edge("tl:trim_lds_then_long_then_trim_lds_on_one_engine")(lambda c: not c.case.force_long and [c.case.runs_trim_long(k) for k in range(len(c.case.subs))] == [False, True, False])
edge("tl:long_then_trim_lds_then_long_on_one_engine")(lambda c: not c.case.force_long and [c.case.runs_trim_long(k) for k in range(len(c.case.subs))] == [True, False, True])
edge("tl:device_resident_max_read_len_0_walks_eight_tiles")(lambda c: c.case.device_max_len == 0 and c.case.R == 8 * LA_TILE and c.case.longest <= 304 and c.case.runs_trim_long(0))

# ---- waves --------------------------------------------------------------------------------------------------------------------------
def _wave_reads(c, k):
    """the (read, Info) lists of the waves of submission k, in the order each wave meets them"""
    n = len(c.sub_reads()[k])
    at = sum(len(s) for s in c.sub_reads()[:k])
    nw = trim_long_grid(n, c.n_cu) * TRIM_LONG_NW
    return [[c.rt[at + r] for r in range(w, n, nw)] for w in range(min(nw, n))]


def _is_waves(c):
    return c.case.force_long and c.case.longest <= 40 and len(c.case.subs) == 1


def wave_sizes(n_cu):
    w = full_waves(n_cu)
    return (w - 1, w, w + 1, 2 * w + 1, 3 * w + 1)


for _k, _nm in enumerate(("W-1", "W", "W+1", "2W+1", "3W+1")):
    edge("wv:batch_of_%s_reads" % _nm)(lambda c, k=_k: _is_waves(c) and len(c.reads) == wave_sizes(c.n_cu)[k] and max(len(w) for w in _wave_reads(c, 0)) == (1, 1, 2, 3, 4)[k])
edge("wv:raw_lengths_all_equal")(lambda c: _is_waves(c) and len(c.reads) >= full_waves(c.n_cu) - 1 and len({i.n0 for i in c.trace}) == 1)
edge("wv:raw_lengths_alternate_read_by_read")(lambda c: _is_waves(c) and len(c.reads) > full_waves(c.n_cu) and all(a.n0 != b.n0 for a, b in zip(c.trace, c.trace[1:])))
edge("wv:a_wave's_successive_reads_are_equal")(lambda c: _is_waves(c) and len({i.n0 for i in c.trace}) > 1 and any(len(w) >= 2 for w in _wave_reads(c, 0)) and
                                               all(len({i.n0 for _, i in w}) == 1 for w in _wave_reads(c, 0)))
edge("wv:a_wave's_successive_reads_differ")(lambda c: _is_waves(c) and any(len(w) >= 4 and all(a[1].n0 != b[1].n0 for a, b in zip(w, w[1:])) for w in _wave_reads(c, 0)))
edge("wv:lengths_change_every_4_reads")(lambda c: _is_waves(c) and len(c.reads) > full_waves(c.n_cu) and all(len({i.n0 for i in c.trace[k:k + 4]}) == 1 for k in range(0, 64, 4)) and
                                        all(c.trace[k].n0 != c.trace[k + 4].n0 for k in range(0, 64, 4)))
edge("wv:lengths_change_every_W_reads")(lambda c: _is_waves(c) and len(c.reads) > 2 * full_waves(c.n_cu) and
                                        [len({i.n0 for i in c.trace[k:k + full_waves(c.n_cu)]}) for k in range(0, len(c.trace) - 1, full_waves(c.n_cu))] == [1] * ((len(c.trace) - 1) // full_waves(c.n_cu)) and
                                        c.trace[0].n0 != c.trace[full_waves(c.n_cu)].n0)
edge("wv:kept_lengths_equal_raw_lengths_differ")(lambda c: _is_waves(c) and any(a[1].flags & b[1].flags & F_VALID and a[1].kept == b[1].kept and a[1].n0 != b[1].n0 for w in _wave_reads(c, 0) for a, b in zip(w, w[1:])))
edge("wv:raw_lengths_equal_kept_lengths_differ")(lambda c: _is_waves(c) and any(a[1].flags & b[1].flags & F_VALID and a[1].kept != b[1].kept and a[1].n0 == b[1].n0 for w in _wave_reads(c, 0) for a, b in zip(w, w[1:])))
edge("wv:filtered_read_between_two_kept_ones_of_one_length")(lambda c: _is_waves(c) and any(len(w) >= 3 and any(not b[1].flags & F_VALID and a[1].flags & F_VALID and x[1].flags & F_VALID and a[1].kept == x[1].kept
                                                                                                               for a, b, x in zip(w, w[1:], w[2:])) for w in _wave_reads(c, 0)))
for _n in (1, 3, 4, 5):
    edge("wv:batch_of_%d:bins_0_1_40_41" % _n)(lambda c, n=_n: c.case.force_long and c.case.longest <= 40 and any(
        len(sub) == n and {int(te.average_quality(te.Model(c.o, 64, c.off).read(r[1], r[2])[1], c.off)) for r in sub} >= ({0, 1, 40, 41} if n >= 4 else ({0, 40, 41} if n == 3 else {41})) for sub in c.sub_reads()))

# ---- window (the oracle's results are the trace) -----------------------------------------------------------------------------------
def _wres(c):
    return [] if not c.case.oracle or c.res is None else [(r, x) for r, x in zip(c.reads, c.res)]


edge("wd:3'_cut_and_the_walk_takes_a_low_tail_in_front_of_it")(lambda c: any(x["flags"] & F_ADAPTER and x["flags"] & F_VALID and x["flags"] & F_QUAL_TRIMMED and x["start"] == 0 and
                                                                             _low_run(c, q[:s.find(ADAPTER_3)], False) > 0 and x["len"] == s.find(ADAPTER_3) - _low_run(c, q[:s.find(ADAPTER_3)], False)
                                                                             for (_, s, q), x in _wres(c) if s.find(ADAPTER_3) > 1024))
edge("wd:5'_cut_by_no_multiple_of_64_then_a_walk")(lambda c: any(x["flags"] & F_ADAPTER and x["flags"] & F_VALID and x["flags"] & F_QUAL_TRIMMED and x["start"] % PIECE and x["start"] > len(ADAPTER_3) and
                                                                 x["start"] + x["len"] < len(s) and len(s) > 1024 and s.find(ADAPTER_3) < 64 for (_, s, q), x in _wres(c)))
edge("wd:both_cuts")(lambda c: any(x["flags"] & F_ADAPTER and x["flags"] & F_VALID and 0 <= s.find(ADAPTER_5) < x["start"] and x["start"] % PIECE and x["start"] + x["len"] <= s.rfind(ADAPTER_3) and len(s) > 1024
                                   for (_, s, q), x in _wres(c)))
edge("wd:whole_read_masked")(lambda c: any(x["flags"] & F_ADAPTER and not x["flags"] & F_VALID and (x["flags"] >> 1) & 7 == FILT_LENGTH_PRE and len(s) > 1024 for (_, s, q), x in _wres(c)))
edge("wd:lengths_1100_and_4097")(lambda c: c.case.oracle and {len(r[1]) for r in c.reads} >= {1100, 4097})


# =====================================================================================================================================
# builders
# =====================================================================================================================================
def q_read(n, sc, salt=0):
    return rd(rb(n, salt), Qs(sc))


def _special(n, deltas, Q, front=False, good=38):
    """a read of n bases: Q - score is deltas[t] at step t of the 3' walk (the 5' walk with front), `good` behind them"""
    sc = [Q - d for d in deltas] + [good] * (n - len(deltas))
    assert len(deltas) <= n and all(0 <= x <= 41 for x in sc)
    return q_read(n, sc if front else sc[::-1], len(deltas))


def stop_rule_deltas(S, kind):
    if kind == "none_at_63_none_at_0":
        return [1] + [0] * (S - 3) + [-3, 0, 0, 5]
    if kind == "rearm_at_63_then_two_without":
        return [1] + [0] * (S - 2) + [-3, 0, 5]
    return [1] + [0] * (S - 4) + [-3, 4, -5, 0, 1]


def walk_reads(Q, lengths, full):
    good, low = (38, Q - 1) if Q < 38 else (41, Q - 1)
    reads = []
    for n in lengths:
        runs = [t for t in RUNS + (n - 1, n) if t <= n and (full or n < MAX_READ_LENGTH or t in (16384, n - 1, n))]
        for t in runs:
            reads.append(q_read(n, [good] * (n - t) + [low] * t, t))
            reads.append(q_read(n, [low] * t + [good] * (n - t), t + 1))
    n = lengths[0]
    if Q < 38:
        for st in MAX_STEPS:       # the area climbs to st + 1, then falls by 1 a step: the walk goes on for st + 1 steps and more
            for front in (False, True):
                reads.append(_special(n, [1] * (st + 1) + [-1] * (st + 4), Q, front))
        reads.append(_special(n, [1] * 10 + [-1] * 5 + [0] * 80 + [1] * 5 + [-1] * 20, Q))          # 10 at step 9 and again at step 99
        reads.append(_special(n, [1] * 10 + [-1] * 5 + [0] * 300 + [1] * 5 + [-1] * 20, Q))         # ... and at step 319, a round later
        for S in SEAMS:
            for kind in ("none_at_63_none_at_0", "rearm_at_63_then_two_without", "none_at_62_rearm_at_63"):
                if S < n - 8 or full:
                    reads.append(_special(max(n, S + 9 if S < 1024 else MAX_READ_LENGTH) if S > n - 8 else n, stop_rule_deltas(S, kind), Q))
        for S in (64, 256):        # BWA: the area is 0 up to step S - 2 (S - 3) and negative from the step behind; the step it does not take would be a new maximum
            reads.append(_special(n, [1, -1] + [0] * (S - 3) + [-1, 5], Q))
            reads.append(_special(n, [1, -1] + [0] * (S - 4) + [-1, 5], Q))
    return reads


def hard_reads(Q):
    reads = []
    for n in (1025, 1100):
        for pos in (1, 0, 5):
            sc = [Q - 1] * n
            sc[pos] = 38
            reads.append(q_read(n, sc, pos))
    for S in (64, 256):
        sc = [Q - 1] * 1025
        sc[S] = 38
        reads.append(q_read(1025, sc, S))
    return reads


def walk_cases(n_cu):
    C = []
    for mname, margs in WALK_MODES.items():
        for Q in (5, 41):
            full = mname == "bwa_plus" and Q == 5
            reads = walk_reads(Q, WALK_LENGTHS, full)
            claims = ["walk:low_tails_and_heads_of_len-1_and_len_at_1025_4096_32767"]
            if not (mname.startswith("hard") and Q == 41):
                claims.append("walk:%s:q%d:low_tails_of_255..16384_are_cut" % (mname, Q))
                claims.append("walk:%s:q41:3'_walk_crosses_a_read_of_32767_into_its_low_head" % mname if Q == 41 else
                              "walk:%s:q%d:low_heads_of_255..16384_are_cut" % (mname, Q) if mname in ("bwa_plus", "hard") else "walk:%s:q%d:low_heads_are_kept" % (mname, Q))
            elif mname == "hard":
                claims.append("walk:hard:q41_cuts_nothing")
            if mname.startswith("hard") and Q == 5:
                reads += hard_reads(Q)
            if mname == "hard" and Q == 5:
                claims += ["walk:hard:first_good_score_at_position_1", "walk:hard:good_score_only_at_position_0_is_not_looked_at", "walk:hard:first_good_score_inside_the_last_piece",
                           "walk:hard:5'_scan_bounded_by_pos_3_on_seam_64", "walk:hard:5'_scan_bounded_by_pos_3_on_seam_256"]
            if Q == 5 and mname == "bwa_plus":
                claims += ["walk:bwa_plus:3'_maximum_at_step_%d_of_a_walk_that_ends_pieces_later" % st for st in MAX_STEPS]
                claims += ["walk:bwa_plus:5'_maximum_at_step_%d_of_a_walk_that_ends_pieces_later" % st for st in MAX_STEPS]
                claims += ["walk:bwa_plus:stop_rule_at_seam_%d:%s" % (S, k) for S in SEAMS for k in ("none_at_63_none_at_0", "rearm_at_63_then_two_without", "none_at_62_rearm_at_63")]
                claims += ["walk:two_equal_maxima_in_different_pieces_the_earlier_wins", "walk:bwa_plus:re-arm_at_step_0_then_thousands_of_re-arming_steps"]
                claims += ["walk:bwa_plus:low_throughout_at_%d:final_pos_3<=final_pos_5" % n for n in (1025, 32767)]
            if Q == 5 and mname == "bwa":
                claims += ["walk:bwa:maximum_at_step_%d_of_a_walk_that_ends_pieces_later" % st for st in MAX_STEPS]
                claims += ["walk:bwa:first_failing_step_at_lane_0_of_piece_%d" % k for k in (1, 4)] + ["walk:bwa:first_failing_step_at_lane_63_of_piece_%d" % k for k in (0, 3)]
            if Q == 5 and mname in ("bwa", "hard"):
                claims += ["walk:low_throughout_at_%d:bwa_and_hard" % n for n in (1025, 32767)] if mname == "bwa" else []
            C.append(LCase("walk_%s_q%d" % (mname, Q), WALK_BASE + margs + ["-q", Q], one(reads), claims, R=MAX_READ_LENGTH))
    for f in FIXED5:       # the same reads behind a fixed 5' cut: the window's pieces lie at every offset from the arena
        reads = []
        for r in walk_reads(5, (1025, 4096), False):
            reads.append((r[0], rb(f, f) + r[1], Qs([38] * f) + r[2]))
        C.append(LCase("walk_bwa_plus_behind_5end_%d" % f, WALK_BASE + ["-q", "5", "--5end", f], one(reads), ["walk:behind_5end_%d:tails_heads_and_seams" % f], R=4096 + 65))
    return C


def n_read(n, lead=0, trail=0, lead_ch=b"N", trail_ch=b"N", hot=None, salt=0):
    """N runs at the ends under scores of 40 (hot: that byte instead), four low bases inwards of each, good bases between"""
    mid = n - lead - trail
    s = lead_ch * lead + rb(mid, salt) + trail_ch * trail
    under = lambda k: bytes([hot]) * k if hot else Qs([40] * k)
    if mid >= 12:
        q = under(lead) + Qs([2] * 4 + [38] * (mid - 8) + [2] * 4) + under(trail)
    else:
        q = under(lead) + Qs([38] * mid) + under(trail)
    return rd(s, q)


def terminal_n_cases(n_cu):
    C = []
    base = ["--min_L", "1", "--lc", "1.0", "-n", "40000"]
    reads = []
    for k in N_RUNS:
        reads += [n_read(1100, lead=k, salt=k), n_read(1100, trail=k, salt=k + 1), n_read(1100, lead=k, trail=k - 60, salt=k + 2)]
    reads += [n_read(1025, lead=1024), n_read(1025, trail=1024), n_read(1025, lead=1025), n_read(1025, lead=512, trail=512)]
    reads += [rd(b"n" + b"N" * 64 + rb(1000, 1) + b"N" * 64 + b"n", Qs([40] * 65 + [38] * 1000 + [40] * 65)),
              rd(b"N" * 70 + b"n" + b"N" * 59 + rb(900, 2) + b"N" * 59 + b"n" + b"N" * 70, Qs([40] * 70 + [38] * 1020 + [40] * 70))]
    reads += [n_read(1100, lead=70, trail=70, hot=33 + 60, salt=9), n_read(1100, lead=70, trail=70, hot=0x7F, salt=10)]
    C.append(LCase("tn_runs_1100", base, one(reads), ["tn:leading_runs_of_63..513_are_masked", "tn:trailing_runs_of_63..513_are_masked", "tn:runs_of_len-1_at_1025", "tn:all_N_at_1025", "tn:N..N_X_N..N",
                                                       "tn:n_at_an_end_is_not_masked", "tn:n_inside_a_run_stops_it", "tn:score_above_41_under_a_terminal_N"]))
    reads = [n_read(M, lead=M - 1), n_read(M, trail=M - 1), n_read(M, lead=M), n_read(M, lead=16384, trail=16382), n_read(M, lead=513, trail=257, salt=3)]
    C.append(LCase("tn_runs_32767", base, one(reads), ["tn:runs_of_len-1_at_32767", "tn:all_N_at_32767", "tn:lead_and_trail_both_32767"], R=M))
    bad = rd(rb(1099, 1) + b"Nn", Qs([38] * 1099) + bytes([33 + 60, 33 + 60]))
    C.append(LCase("tn_score_above_41_under_n", base, one([q_read(1100, [38] * 1100), bad, q_read(1100, [38] * 1100, 1)]), ["tn:score_above_41_under_a_terminal_n_is_an_error"], error=True))
    return C


def run_read(n, start, ln, salt=0, ch=b"N"):
    assert 0 <= start and start + ln <= n
    return rd(rb(start, salt) + ch * ln + rb(n - start - ln, salt + 1))


def poly_n_cases(n_cu):
    C = []
    base = ["--min_L", "1", "--lc", "1.0", "-q", "0"]       # (-q 0: no walk cuts anything, the window is the read)
    for k in POLY_K:
        reads = []
        for ln in (k - 1, k, k + 1):
            for seam, m in ((PIECE, 2), (ROUND, 1), (PIECE, 3)):
                for j in poly_offsets(k):
                    if m * seam - j >= 0 and (m == 3) <= (k <= 7):
                        reads.append(run_read(1100, m * seam - j, ln, ln + j))
        # at the window's end in a last piece of 1, 63 and 64 positions, a last piece that is all N, terminal runs
        for w in (1, 63, 64):
            for n in (1024 + w, 1088 + w):
                reads += [run_read(n, n - ln, ln, w) for ln in (k - 1, k) if ln > 0]
        if k >= 64:
            reads += [run_read(1034, 1034 - k, k, 5)]
        reads += [run_read(1100, 0 if front else 1100 - ln, ln, 6) for ln in (k, k + 1) for front in (True, False)] + [rd(b"N" * 1025)]
        reads += [rd(rb(216, 7) + b"N" * 40 + b"n" + b"N" * 40 + rb(803, 8))]
        if k == 64:
            reads += [run_read(1100, 64, 64, 9), run_read(1100, 256, 64, 10)]
        if k == 129:
            reads += [run_read(1100, 64, 128, 9), run_read(1100, 192, 128, 10), run_read(1100, 1, 128, 11), run_read(1100, 193, 128, 12)]
        for qc in (False, True):
            claims = ["pn:-n_%d:%s" % (k, "the_same_under_qc_only" if qc else "runs_of_k-1_k_k+1_from_64m-j_and_256m-j")]
            if not qc:
                claims += ["pn:run_ends_at_the_window's_end_in_a_last_piece_of_%d" % w for w in (1, 63, 64)] + ["pn:terminal_runs_count_as_runs", "pn:run_broken_by_n"]
                claims += ["pn:last_piece_all_N"] if k >= 74 else []
                claims += ["pn:run_of_one_whole_piece"] if k == 64 else []
                claims += ["pn:run_of_two_whole_pieces", "pn:run_of_63+64+1_over_three_pieces"] if k == 129 else []
            C.append(LCase("pn_n%d%s" % (k, "_qc_only" if qc else ""), base + ["-n", k] + (["--qc_only"] if qc else []), one(reads), claims))
    for k in (64, 129):     # a run of k that the 3' cut (the 5' cut) shortens to k - 1: the low scores begin on the run's last (end on its first) base
        reads = [rd(rb(500, 1) + b"N" * k + rb(600 - k, 2), Qs([38] * (500 + k - 1) + [2] * (601 - k))), rd(rb(100, 3) + b"N" * k + rb(1000 - k, 4), Qs([2] * 101 + [38] * 999))]
        C.append(LCase("pn_n%d_shortened_by_a_cut" % k, ["--min_L", "1", "--lc", "1.0", "-n", k], one(reads), ["pn:run_shortened_by_the_3'_and_the_5'_cut"]))
    return C


def lc_pair(n, count, di):
    """two --lc texts: under the first a count of `count` in n bases trips the filter and count - 1 does not, under the second it is one below the threshold"""
    norm = f32(1.0 / n)
    if di:
        norm = f32(float(norm) * 2.0)
    v = f32(count) * norm
    at, below = np.nextafter(v, f32(0), dtype=f32), v
    assert lc_thr(n, at, di) == count and lc_thr(n, below, di) in (count + 1, None)
    return repr(float(at)), repr(float(below))


def fields_cases(n_cu):
    C = []
    base = ["--mode", "BWA", "--min_L", "1", "-n", "40000"]
    good = lambda s, q=38: rd(s, Qs([q]) * len(s))
    sets = (("count=len", ("all_A", "all_T", "all_C", "all_G", "all_N"), M, False), ("halves", ("A_T_halves", "C_G_halves"), 16384, False),
            ("AT_pairs", ("AT_pairs",), 16383, True), ("TCTG_quads", ("TCTG_quads",), 8192, True))
    for name, which, count, di in sets:
        for where, text in zip(("at", "below"), lc_pair(M, count, di)):
            claims = ["fd:%s:%s_count_%s_the_threshold" % (w, "transition" if di else "base", where) for w in which if w != "all_N"]
            if name == "count=len":
                claims += ["fd:all_N:counts_nothing_and_is_kept"] + (["fd:composition_bin_of_count=len_pre_and_post", "fd:result_offset_0_length_32767"] if where == "below" else [])
            if name == "halves" and where == "below":
                claims += ["fd:composition_bins_of_the_16384/16383_split"]
            C.append(LCase("fd_%s_%s_threshold" % (name, where), base + ["--lc", text], one([good(COMPOSITIONS[w]) for w in which]), claims, R=M))
    reads = [rd(b"A" * (M - 7) + b"T" * 7, Qs([38] * (M - 7) + [2] * 7)), rd(b"A" * 16384 + b"T" * 16383, Qs([38] * (M - 7) + [2] * 7))]
    C.append(LCase("fd_composition_post_trim", base + ["--lc", "1.0"], one(reads), ["fd:composition_bins_post_trim_on_a_kept_length"], R=M))
    reads = [good(rb(M, 1), 41), rd(rb(M, 2), bytes([0x80]) * M), rd(rb(M, 3), bytes([0xFF]) * M)]
    C.append(LCase("fd_quality_bytes", base + ["--lc", "1.0", "-q", "0"], one(reads), ["fd:quality_all_offset+41", "fd:quality_all_0x80:negative_sum_clamped", "fd:quality_all_0xFF:negative_sum_clamped"], R=M))
    reads = [rd(rb(M, 1), Qs([41] * M, 64)), rd(rb(M, 2), Qs([10] * M, 33)), rd(rb(M, 3), bytes([0x80]) * M)]
    C.append(LCase("fd_ascii_64", base + ["--lc", "1.0", "-q", "0", "--ascii", "64"], one(reads), ["fd:ascii_64"], R=M))
    C.append(LCase("fd_5end_32766", base + ["--lc", "1.0", "--5end", M - 1], one([good(rb(M, 4)), good(rb(M - 1, 5)), good(rb(1025, 6))]), ["fd:result_offset_32766_length_1"], R=M))
    return C


def pair_read(n, pairs, seam, kind, shift=0, pair=b"AG", lane_q=None):
    """a read whose window of n bases (behind `shift` fillers) holds `pairs` transitions of one kind, in triplets such as AGR that make no second kind; kind
    "pair": one of them across the seam; "no_pair": none there, but a non-base at seam - 1 and the pair's second base alone at the seam; lane_q: (0 | 1, score):
    the score of the G of the seam's pair, at seam - 1 (the pair is GA) or at the seam (AG)"""
    s = bytearray(b"R" * n)
    if kind == "pair":
        s[seam - 1:seam + 1] = pair
        left = pairs - 1
    else:
        s[seam - 1:seam + 1] = (b"N" if seam == 64 else b"R") + pair[1:]
        left = pairs
    p = 2
    while left:
        if not (seam - 4 <= p <= seam + 2) and p % PIECE != PIECE - 1:
            s[p:p + 2] = pair
            left -= 1
        p += 3
        assert p < n - 2
    q = bytearray(Qs([38] * n))
    if lane_q is not None:
        q[seam - 1 + lane_q[0]] = 33 + lane_q[1]
    return rd(rb(shift, 3).replace(b"A", b"C").replace(b"G", b"C") + bytes(s), Qs([38] * shift) + bytes(q))


def transitions_cases(n_cu):
    C = []
    base = ["--mode", "BWA", "--min_L", "1", "-n", "40000", "--lc", "0.2"]
    lc = f32(0.2)
    for n in TR_LENGTHS:
        for shift in (0, 7):
            wn = min(n, M - shift)          # (the window behind the cut)
            t2 = lc_thr(wn, lc, True)
            reads = []
            for seam in (64, 256) + (() if shift else (last_seam(n),)):
                reads += [pair_read(wn, k, seam, "pair", shift) for k in (t2 - 1, t2)]
                if seam <= 256 and not shift:
                    reads += [pair_read(wn, t2 - 1, seam, "no_pair")]
            claims = ["tr:%d:behind_a_5'_cut_that_moves_the_seam" % n] if shift else ["tr:%d:deciding_pair_on_seam_%s" % (n, sn) for sn in ("63|64", "255|256", "last")] + ["tr:%d:non-base_at_lane_63_makes_no_pair_at_lane_0" % n]
            C.append(LCase("tr_%d%s" % (n, "_behind_5end_7" if shift else ""), base + (["--5end", "7"] if shift else []), one(reads), claims, R=wn + shift if wn + shift > 4096 else None))
    t2 = lc_thr(1025, lc, True)
    reads = [pair_read(1025, t2, 64, "pair", pair=pr, lane_q=(lane, sc)) for lane, pr in ((0, b"GA"), (1, b"AG")) for sc in (14, 15)]
    # (every other G of these reads is good: only the G of the seam's pair is replaced)
    C.append(LCase("tr_replace_to_N_q", base + ["--replace_to_N_q", "15"], one(reads), ["tr:replace_to_N_q:G_on_lane_63_decides", "tr:replace_to_N_q:G_on_lane_0_decides"]))
    return C


def short_reads(n, salt=0, lo=30, hi=40):
    return [q_read(lo + (k * 7 + salt) % (hi - lo + 1), [38] * (lo + (k * 7 + salt) % (hi - lo + 1)), k + salt) for k in range(n)]


def tiles_cases(n_cu):
    C = []
    flat = ["--min_L", "1", "--lc", "1.0", "-n", "40000", "-q", "0"]     # nothing is cut and nothing filtered: the matrices are the reads
    for n in TILE_LENGTHS:
        reads = [phase_read(n, 0), phase_read(n - 200, 5), phase_read(n, 17), phase_read(40, 3)]
        C.append(LCase("tl_max_len_%d" % n, flat, one(reads), ["tl:max_len_%d_two_phases" % n], R=n, force_long=n <= FAST_READ_LENGTH))
    for a, b in WINDOWS:
        n = 1537
        args = (["--5end", a] if a else []) + (["--3end", n - b] if b else [])
        C.append(LCase("tl_window_%d_%s_fixed" % (a, b or "len"), flat + args, one([phase_read(n, 0), phase_read(n, 17), phase_read(1100, 4)]), ["tl:kept_window_%d_%s_by_fixed_cuts" % (a, b or "len")], R=n))
    n = 1537
    reads = [q_read(n, [4] * a + [38] * ((b or n) - a) + [4] * (n - (b or n)), a) for a, b in WINDOWS]
    C.append(LCase("tl_windows_by_bwa_plus_walks", ["--min_L", "1", "--lc", "1.0", "-n", "40000"], one(reads), ["tl:kept_window_%d_%s_by_a_walk" % (a, b or "len") for a, b in WINDOWS if (a, b) != (511, 513)], R=n))
    # (BWA_plus leaves nothing of a window of two bases: HARD keeps it)
    C.append(LCase("tl_windows_by_hard_scans", ["--mode", "HARD", "--min_L", "1", "--lc", "1.0", "-n", "40000"], one(reads), ["tl:kept_window_%d_%s_by_a_walk" % (a, b or "len") for a, b in WINDOWS], R=n))
    reads = [n_read(1100, lead=k, salt=k) for k in (511, 512, 513)] + [n_read(1100, trail=1100 - k, salt=k + 1) for k in (511, 512, 513)] + [n_read(1100, lead=512, trail=588)]
    C.append(LCase("tl_terminal_runs_on_the_tile_border", ["--min_L", "1", "--lc", "1.0", "-n", "40000"], one(reads), ["tl:terminal_runs_end_and_begin_on_511_512_513"], R=1100))
    reads = []
    for p in (511, 512):
        for inside in (True, False):
            s = bytearray(rb(1100, p).replace(b"G", b"C"))
            s[p] = 71
            sc = [38] * 1100
            sc[p] = 9
            if not inside:          # a low tail from p - 3 on (a low head up to p + 3): the G lies outside the window
                if p == 511:
                    sc[:p + 3] = [3] * (p + 3)
                else:
                    sc[p - 3:] = [3] * (1100 - p + 3)
            reads.append(rd(bytes(s), Qs(sc)))
    C.append(LCase("tl_replace_to_N_q", ["--min_L", "1", "--lc", "1.0", "-n", "40000", "--replace_to_N_q", "15"], one(reads),
                   ["tl:replace_to_N_q:low_G_either_side_of_a_tile_border_inside_and_outside_the_window"], R=1100))
    C.append(LCase("tl_R_32767_longest_1025", flat, one([phase_read(1025, 0), phase_read(700, 17), phase_read(1025, 5)]), ["tl:R_32767_under_a_longest_read_of_1025"], R=MAX_READ_LENGTH))
    subs = []
    for k, n in enumerate(batch_sizes(n_cu)):
        sh = short_reads(n - 1, k)
        subs.append([sh[:n // 2] + [phase_read(1025, k)] + sh[n // 2:]])
    C.append(LCase("tl_batch_sizes", ["--min_L", "1", "--lc", "1.0", "-n", "40000"], subs, ["tl:batches_of_1_15_16_17_and_either_side_of_a_full_grid"], R=1025))
    lds = lambda k: [te.ragged(70, 152, k)]
    lng = lambda k: [[phase_read(1537, k), q_read(1100, [38] * 1000 + [3] * 100, k), phase_read(600, k + 1)]]
    C.append(LCase("tl_lds_long_lds", ["--min_L", "10"], [lds(1), lng(2), lds(3)], ["tl:trim_lds_then_long_then_trim_lds_on_one_engine"], R=1537))
    C.append(LCase("tl_long_lds_long", ["--min_L", "10"], [lng(4), lds(5), lng(6)], ["tl:long_then_trim_lds_then_long_on_one_engine"], R=1537))
    C.append(LCase("tl_device_resident_max_read_len_0", ["--min_L", "10"], [[te.ragged(100, 304, 7)]], ["tl:device_resident_max_read_len_0_walks_eight_tiles"], R=8 * LA_TILE, device_max_len=0))
    return C


def waves_cases(n_cu):
    C = []
    Wv = full_waves(n_cu)
    sizes = wave_sizes(n_cu)
    base = ["--min_L", "1", "--lc", "1.0", "-n", "2"]
    _memo = {}

    def sr(n, tail=0, kind=0):
        """a read of n bases with a low tail; kind 1: NN inside (the poly-N filter takes it)"""
        if (n, tail, kind) not in _memo:
            s = rb(n, n + tail)
            if kind:
                s = s[:10] + b"NN" + s[12:]
            _memo[(n, tail, kind)] = rd(s, Qs([38] * (n - tail) + [2] * tail))
        return _memo[(n, tail, kind)]
    # the five batch sizes are 8 W + 2 reads in all (65 538 on 256 compute units): every other edge of the family rides on one of them
    C.append(LCase("wv_W-1_equal_lengths", base, one([sr(35)] * sizes[0]), ["wv:batch_of_W-1_reads", "wv:raw_lengths_all_equal"], force_long=True))
    C.append(LCase("wv_W_alternating", base, one([sr(30 + 5 * (k % 2)) for k in range(sizes[1])]), ["wv:batch_of_W_reads"], force_long=True))
    C.append(LCase("wv_W+1_every_4_reads", base, one([sr(30 + (k // 4) % 11) for k in range(sizes[2])]), ["wv:batch_of_W+1_reads", "wv:lengths_change_every_4_reads"], force_long=True))
    # 2 W + 1 reads whose lengths alternate read by read: W is even, so a wave's reads are all of one raw length; their low tails, and so their kept lengths, differ
    C.append(LCase("wv_2W+1_alternating", base, one([sr(30 + 5 * (k % 2), 3 * (k // Wv)) for k in range(sizes[3])]),
                   ["wv:batch_of_2W+1_reads", "wv:raw_lengths_alternate_read_by_read", "wv:a_wave's_successive_reads_are_equal", "wv:raw_lengths_equal_kept_lengths_differ"], force_long=True))
    # 3 W + 1 reads: W of 31 bases, W of 34 with a low tail of 3 (kept: 31), W of 37 that the poly-N filter takes, one of 31: a wave meets four raw lengths, two
    # kept lengths of 31, a filtered read and 31 again -- the post-trim run goes on across the filtered read
    block = [sr(31), sr(34, 3), sr(37, 0, 1), sr(31)]
    C.append(LCase("wv_3W+1_every_W_reads", base, one([block[k // Wv] for k in range(sizes[4])]),
                   ["wv:batch_of_3W+1_reads", "wv:lengths_change_every_W_reads", "wv:a_wave's_successive_reads_differ", "wv:kept_lengths_equal_raw_lengths_differ",
                    "wv:filtered_read_between_two_kept_ones_of_one_length"], force_long=True))
    bins = [q_read(40, [x] * 40, x) for x in (41, 40, 0, 1, 20)]
    C.append(LCase("wv_small_batches", ["--mode", "BWA", "--min_L", "1", "--lc", "1.0", "-q", "0"], [[bins[:n]] for n in (1, 3, 4, 5)], ["wv:batch_of_%d:bins_0_1_40_41" % n for n in (1, 3, 4, 5)], force_long=True))
    return C


ADAPTER_5 = b"GATCGGAAGAGCACACGTCTGAACTCCAGTCAC"             # Nextera-primer-adapter-1
ADAPTER_3 = b"CTGTCTCTTATACACATCTAGATGTGTATAAGAGACAG"        # Nextera-junction-adapter-1 of the built-in set (faqcs_amd/options.py; the CPU test compares)
WINDOW_ARGS = ["--adapter", "-t", "1", "--min_L", "1", "-n", "40000", "--lc", "1", "--avg_q", "0"]


def window_cases(n_cu):
    A = ADAPTER_3
    reads = []
    for n in (1100, 4097):
        body = n - len(A)
        reads.append(rd(rb(body, n) + A, Qs([38] * (body - 30) + [2] * 30 + [38] * len(A))))                       # 3' cut, a low tail in front of it
        reads.append(rd(rb(5, n) + A + rb(body - 5, n + 1), Qs([38] * (5 + len(A)) + [2] * 20 + [38] * (body - 45) + [2] * 20)))   # 5' cut by 43 bases, low head and tail behind it
        reads.append(rd(rb(3, n) + ADAPTER_5 + rb(body - len(ADAPTER_5) - 3, n + 2) + A, Qs([38] * n)))                              # both cuts
    whole = rb(1100, 77)
    reads.append(rd(whole))
    return [LCase("wd_adapter_window_then_walk", WINDOW_ARGS, one(reads), ["wd:3'_cut_and_the_walk_takes_a_low_tail_in_front_of_it", "wd:5'_cut_by_no_multiple_of_64_then_a_walk", "wd:both_cuts",
                                                                           "wd:whole_read_masked", "wd:lengths_1100_and_4097"], R=4097, adapters=[("whole-read", whole.decode())], oracle=True)]


_BUILDERS = dict(walk=walk_cases, terminal_n=terminal_n_cases, poly_n=poly_n_cases, fields=fields_cases, transitions=transitions_cases, tiles=tiles_cases, waves=waves_cases, window=window_cases)
_CASES = {}


def family_cases(family, n_cu=256):
    if (family, n_cu) not in _CASES:
        cs = _BUILDERS[family](n_cu)
        for c in cs:
            c.family, c.n_cu = family, n_cu
        _CASES[(family, n_cu)] = cs
    return _CASES[(family, n_cu)]


def all_cases(n_cu=256):
    return [c for f in FAMILIES for c in family_cases(f, n_cu)]


def coverage(cases=None):
    """Every predicate on every case -> ({edge: [cases that claim it and reach it]}, {case: [claims that do not hold]}, {edge: [cases that reach it
    without claiming it]})"""
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
# the piecewise model and its mutants
# =====================================================================================================================================
MUTANTS = {
    # mutant: (what it does, the case that tells it apart)
    "prev_nr_not_carried": ("the last lane's `no re-arm` is not handed to the next piece", "walk_bwa_plus_q5"),
    "later_piece_wins_a_tie": ("`m > best` across pieces taken as `>=`", "walk_bwa_plus_q5"),
    "carry_dropped_at_a_round": ("the walk's running area starts from 0 after every fourth piece", "walk_bwa_plus_q5"),
    "run_carry_reset_at_a_round": ("the poly-N run carried into a round is dropped", "pn_n7"),
    "prev_cls_reset_at_a_piece": ("lane 0 sees no base in front of it", "tr_1025"),
    "window_starts_one_late": ("the matrices take `p > k0`", "tl_window_512_1024_fixed"),
    "window_ends_one_late": ("the matrices take `p <= k1`", "tl_window_512_1024_fixed"),
    "leading_run_one_longer": ("the matrices mask `p <= lead`", "tl_terminal_runs_on_the_tile_border"),
    "trailing_run_one_shorter": ("the matrices mask `p > tail_from`", "tl_terminal_runs_on_the_tile_border"),
    "length_run_added_to_the_new_key": ("a wave's run of equal lengths is added to the length that ends it", "wv_3W+1_every_W_reads"),
}
# wrong versions that no input can tell apart (EXCLUSIONS names why); the CPU test asserts that they equal the model on their family
EQUIVALENT_MUTANTS = {"whole_N_piece_adds_64": ("a piece that is wholly N adds 64 to run_carry where its width is smaller", "poly_n")}
_LANE = np.arange(PIECE)


def _walk_pieces(sc, Q, desc, plus, rearm_below, mut):
    """area_walk of trim_long: the step after which the area was largest and positive, or -1"""
    n = len(sc)
    steps = sc[::-1] if desc else sc
    a0 = min(n, 5)
    carry, best, best_t, seen, prev_nr = 0, 0, -1, False, False
    for k in range((n + PIECE - 1) // PIECE):
        w = min(PIECE, n - PIECE * k)
        d = np.zeros(PIECE, np.int64)
        d[:w] = Q - steps[PIECE * k:PIECE * k + w]
        valid = _LANE < w
        incl = np.cumsum(d)
        before, after = carry + incl - d, carry + incl
        t = PIECE * k + _LANE
        stop = PIECE
        if plus:
            rm = valid & (t < rearm_below) & (before >= 0)
            nr = ~rm
            sh = np.concatenate(([False], nr[:-1]))
            cand = None
            if not seen:
                f = int(np.argmax(rm)) if rm.any() else PIECE
                if f >= a0:
                    stop = a0 - 1
                else:
                    seen = True
                    cand = nr & sh & (_LANE >= f + 2)
            else:
                sh[0] = prev_nr
                cand = nr & sh
            if cand is not None and cand.any():
                stop = int(np.argmax(cand))
            prev_nr = bool(nr[PIECE - 1]) and mut != "prev_nr_not_carried"
            visited = _LANE <= stop
        else:
            go = valid & (t < n - 1) & (before >= 0)
            ff = PIECE if go.all() else int(np.argmin(go))
            visited = _LANE < ff
            if ff < PIECE:
                stop = ff
        mine = valid & visited
        if mine.any():
            m = int(after[mine].max())
            if m > best or (mut == "later_piece_wins_a_tie" and m == best and m > 0):
                best, best_t = m, PIECE * k + int(np.argmax(mine & (after == m)))
        if stop < PIECE:
            break
        carry += int(incl[PIECE - 1])
        if mut == "carry_dropped_at_a_round" and k % (ROUND // PIECE) == ROUND // PIECE - 1:
            carry = 0
    return best_t


def _poly_pieces(ws, mut):
    isn = np.frombuffer(ws, np.uint8) == 78
    run_max = carry = 0
    for c in range(0, len(ws), PIECE):
        if mut == "run_carry_reset_at_a_round" and c % ROUND == 0:
            carry = 0
        m = isn[c:c + PIECE]
        wv = len(m)
        if m.any():
            lead1 = wv if m.all() else int(np.argmin(m))
            inner = max(len(x) for x in m.view(np.uint8).tobytes().split(b"\0"))
            run_max = max(run_max, carry + lead1, inner)
            if lead1 >= wv:
                carry += PIECE if mut == "whole_N_piece_adds_64" else wv
            else:
                carry = wv - 1 - int(np.nonzero(~m)[0][-1])
        else:
            carry = 0
    return run_max


def _piece_read(s, q, o, off, mut):
    """one read as trim_long judges it -> ((start, len, flags), lead, trail, the window (k0, k1) of a kept read or None); QualityError where it flags the read"""
    n = len(s)
    lead = n - len(s.lstrip(b"N"))
    trail = n if lead == n else n - len(s.rstrip(b"N"))
    qm = bytearray(q)
    qm[:lead] = bytes([off]) * lead
    qm[n - trail:] = bytes([off]) * min(trail, n)
    qm = bytes(qm)
    sc = np.array(te.scores_of(qm, off), np.int64)
    w0, ln, offset_5, flags, filt, ok = 0, n, 0, 0, FILT_NONE, True
    if o.trim_5 and not o.qc_only:
        if o.trim_5 > ln:
            ln = 0
        else:
            w0, ln, offset_5 = w0 + o.trim_5, ln - o.trim_5, offset_5 + o.trim_5
    if o.trim_3 and not o.qc_only:
        ln = 0 if o.trim_3 > ln else ln - o.trim_3
    if ln < o.min_read_length or ln == 0:
        ok, filt = False, FILT_LENGTH_PRE
    if not o.qc_only and ok:
        win, Q = sc[w0:w0 + ln], o.quality
        nan2 = min(ln, 2)
        if o.mode == MODE_HARD:
            cut5, kept, _ = te.walk_hard(list(win), Q, o.protect_5)
        elif o.mode == MODE_BWA:
            bt = _walk_pieces(win, Q, True, False, 0, mut)
            cut5, kept = 0, ((ln - 1 - bt) - 1 if bt >= 0 else ln - 1) + 1
        else:
            bt3 = _walk_pieces(win, Q, True, True, ln - 1 - nan2, mut)
            f3 = (ln - 1 - bt3) - 1 if bt3 >= 0 else ln - 1
            f5 = 0
            if not o.protect_5:
                bt5 = _walk_pieces(win, Q, False, True, f3 - nan2, mut)
                f5 = bt5 + 1 if bt5 >= 0 else 0
            cut5, kept = f5, (0 if f3 <= f5 else f3 - f5 + 1)
        if kept != ln:
            flags |= F_QUAL_TRIMMED
        offset_5, w0, ln = offset_5 + cut5, w0 + cut5, kept
        if ln < o.min_read_length or ln == 0:
            ok, filt = False, FILT_LENGTH_POST
    ws, wq = s[w0:w0 + ln], qm[w0:w0 + ln]
    if ok and _poly_pieces(ws, mut) >= o.max_num_poly_N:
        flags |= F_POLY_N_SEEN
        if not o.qc_only:
            ok, filt = False, FILT_POLY_N
    if ok and te.average_quality(wq, off) < f32(o.average_quality):
        ok, filt = False, FILT_AVG_Q
    if ok and ln:
        b = np.frombuffer(ws, np.uint8).copy()
        if o.replace_to_N_q > 0:
            b[(b == 71) & (sc[w0:w0 + ln] < o.replace_to_N_q)] = 78
        cls = _CLS[b]
        prev = np.concatenate(([4], cls[:-1]))
        if mut == "prev_cls_reset_at_a_piece":
            prev[::PIECE] = 4
        pair = (cls != 4) & (prev != 4) & (cls != prev)
        dc = np.bincount((prev * 4 + cls)[pair], minlength=16)
        cnt = np.bincount(cls, minlength=5)[:4]
        norm, lc = f32(1.0 / ln), f32(o.low_complexity_cutoff_ratio)
        low = any(f32(int(c)) * norm > lc for c in cnt)
        if not low:
            norm2 = f32(float(norm) * 2.0)
            low = any(f32(int(c)) * norm2 > lc for c in dc)
        if low:
            ok, filt = False, FILT_LOW_COMPLEXITY
    x = ((offset_5 & 0xffff) | (ln << 16)) if ok else 0         # the packed verdict long_accumulate reads the window from
    res = (x & 0xffff, x >> 16, flags | (F_VALID if ok else 0) | (filt << 1))
    return res, lead, trail, ((x & 0xffff, (x & 0xffff) + (x >> 16)) if ok else None)


_COL = np.full(256, -1, np.int64)
for _k, _ch in enumerate(b"ATCGN"):
    _COL[_ch] = _COL[_ch | 32] = _k


def pieces(case, mutant=None):
    """The piecewise model on a case -> dict(results, sections: the two length histograms and the four matrices, error)"""
    o, off, R, n_cu = case.opt(), case.in_off, case.R, case.n_cu
    lay = te.layout(R)
    sec = {k: np.zeros(lay[k][1], np.int64) for k in ("pre_len_hist", "post_len_hist", "pre_qual", "post_qual", "pre_base", "post_base")}
    results = []
    try:
        for k, sub in enumerate(case.subs):
            reads = [r for seg in sub for r in seg]
            limit = min(case.max_len(k), R)
            memo = {}        # (the batches of the waves family hold few distinct reads)
            verdict = [memo[(s, q)] if (s, q) in memo else memo.setdefault((s, q), _piece_read(s, q, o, off, mutant)) for _, s, q in reads]
            res = np.zeros(len(reads), te.RESULT_DTYPE)
            for j, v in enumerate(verdict):
                res[j] = v[0] + (0,)
            results.append(res)
            if not case.runs_trim_long(k):      # (a batch for the chunked kernels: the plain sums)
                for (_, s, q), (r, lead, trail, win) in zip(reads, verdict):
                    sec["pre_len_hist"][len(s)] += 1
                    if win:
                        sec["post_len_hist"][win[1] - win[0]] += 1
            else:
                nw = trim_long_grid(len(reads), n_cu) * TRIM_LONG_NW
                for w in range(min(nw, len(reads))):
                    for which, key_of in (("pre_len_hist", lambda j: len(reads[j][1])), ("post_len_hist", lambda j: verdict[j][3][1] - verdict[j][3][0] if verdict[j][3] else None)):
                        key, run = None, 0
                        for j in range(w, len(reads), nw):
                            x = key_of(j)
                            if x is None:
                                continue
                            if x != key:
                                if run:
                                    sec[which][x if mutant == "length_run_added_to_the_new_key" else key] += run
                                key, run = x, 0
                            run += 1
                        if run:
                            sec[which][key] += run
            add = {k_: [] for k_ in ("pre_qual", "post_qual", "pre_base", "post_base")}
            for (_, s, q), (r, lead, trail, win) in zip(reads, verdict):
                e = min(len(s), limit if case.runs_trim_long(k) else R)
                if not e:
                    continue
                p = np.arange(e)
                tail_from = len(s) - trail
                masked = ((p <= lead) if mutant == "leading_run_one_longer" else (p < lead)) | ((p > tail_from) if mutant == "trailing_run_one_shorter" else (p >= tail_from))
                qv = np.where(masked, off, np.frombuffer(q, np.int8)[:e].astype(np.int64))
                scv = np.minimum(np.maximum(qv - off, 0), NQ - 1)
                k0, k1 = win or (0, 0)
                inw = ((p > k0) if mutant == "window_starts_one_late" else (p >= k0)) & ((p <= k1) if mutant == "window_ends_one_late" else (p < k1))
                add["pre_qual"].append(p * NQ + scv)
                add["post_qual"].append((p * NQ + scv)[inw])
                b0 = np.frombuffer(s, np.uint8)[:e]
                col0 = _COL[b0]
                add["pre_base"].append((p * NBASE + col0)[col0 >= 0])
                b = np.where((o.replace_to_N_q > 0) & (b0 == 71) & (scv < o.replace_to_N_q), 78, b0)
                col = _COL[b]
                add["post_base"].append((p * NBASE + col)[inw & (col >= 0)])
            for k_, v in add.items():
                if v:
                    sec[k_] += np.bincount(np.concatenate(v), minlength=len(sec[k_]))
    except te.QualityError:
        return dict(results=None, sections=None, error=E_QUALITY)
    return dict(results=results, sections=sec, error=0)


def pieces_differ(case, got):
    """None when the piecewise model's output equals the case's expected(), else the first difference in words"""
    e = case.expected()
    if got["error"] != e["error"]:
        return "error %d for %d" % (got["error"], e["error"])
    if e["error"]:
        return None
    for k, (a, b) in enumerate(zip(got["results"], e["results"])):
        bad = np.nonzero(a != b)[0]
        if len(bad):
            return "submission %d read %d: %s for %s" % (k, bad[0], a[bad[0]], b[bad[0]])
    lay = te.layout(case.R)
    for name, v in got["sections"].items():
        want = e["counters"][lay[name][0]:lay[name][0] + lay[name][1]].astype(np.int64)
        bad = np.nonzero(v != want)[0]
        if len(bad):
            return "%s[%d]: %d for %d (%d cells differ)" % (name, bad[0], v[bad[0]], want[bad[0]], len(bad))
    return None


def case_named(name, n_cu=256):
    return [c for c in all_cases(n_cu) if c.name == name][0]


def caught(mutant, n_cu=256):
    """how the case MUTANTS names tells the mutant from the model, or None"""
    c = case_named(MUTANTS[mutant][1], n_cu)
    return pieces_differ(c, pieces(c, mutant))


def comp_bin_search(lo=FAST_READ_LENGTH + 1, hi=MAX_READ_LENGTH):
    """the largest trunc(bin(a)) + trunc(bin(len - a)) over every length lo .. hi and every split a: the GC bin is written without a bound check"""
    worst = 0
    for n in range(lo, hi + 1):
        norm = f32(te.NCOMP_BIN - 1) / f32(n)
        b = (norm * np.arange(n + 1, dtype=np.float32)).astype(np.int64)     # (float32 products, truncated)
        worst = max(worst, int((b + b[::-1]).max()))
    return worst


if __name__ == "__main__":
    t, lost, more = coverage()
    print("claimed  unclaimed  edge")
    for e, v in t.items():
        print("%7d  %9d  %s" % (len(v), len(more[e]), e))
    for f in FAMILIES:
        cs = family_cases(f)
        print("%-12s %3d cases %6d reads %9d bases  reference: %s" % (f, len(cs), sum(c.n_reads() for c in cs), sum(len(r[1]) for c in cs for sub in c.subs for seg in sub for r in seg), FAMILY_REFERENCE[f]))
    print("%d cases, %d edges; unreached: %s; claims that do not hold: %s" % (len(all_cases()), len(t), sorted(e for e, v in t.items() if not v), lost))
    for m in MUTANTS:
        print("mutant %-34s %s: %s" % (m, MUTANTS[m][1], caught(m)))
    for name, why in EXCLUSIONS.items():
        print("excluded %s: %s" % (name, why))
