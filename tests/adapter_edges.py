"""A constructed catalogue of inputs for the adapter / contaminant pre-pass (adapter_overlap_pair and every variant of adapter_overlap,
faqcs_adapter_kernel.hip; the group partition of faqcs_capi.hip), in the style of tests/trim_edges.py: the edges of the launcher's dispatch,
of the targets' plane-word classes, of the reads' lengths and bytes, of the aligner's tie rule over diagonals and 64-diagonal blocks, of the
three stage-1 filters, of the float32 threshold and the group of 8 it is taken from, of the stale-range state, of the mask and
find_mask_range, of the groups of a library past one launch, of the two halves of the pair kernel, and of the bytes the aligner rejects.
Every case is a named library, an option list and submissions of segments of reads (all qualities 'I'); every edge a PREDICATE over a
case's inputs and the model's per-(read, target) trace; coverage() evaluates every predicate on every case.

model: the plain reference.  trim_adapters_and_phiX (trim.cpp:961-1142) under -t 1, SeqOverlap's ungapped local alignment
(seq_overlap.cpp:46-370: M = max(M_prev, 0) + s along the diagonal, the start replaced only where M_prev < 0, the last row-major cell
among the maxima kept) and find_mask_range (trim.cpp:1144-1189), with the quirks Q1, Q3, Q4, Q5 and H2 of SURVEY.md Appendix B, on Python
ints; the DP is swept with numpy along the longer of the two sequences, one position of the shorter per step.  Only the threshold is
float32, one operation at a time.  It shares no text with oracle/ and none with the kernel or its host tables.

What the model predicts of a record: `adapter` (1 + the credited target, 0 for none), FAQCS_F_ADAPTER, and -- the options of every case
leave the trim stage behind the pre-pass nothing to decide (BASE_ARGS) -- FAQCS_F_VALID, `start` and `len` of a read that is not filtered
(trim.cpp:270-277: the window; a window without a base starts at the read's length and is filtered); and adapter_stats of the counter
block.  A read with a byte na_to_bits() rejects is flagged FAQCS_F_ERR_BASE, alone, and the submission fails with FAQCS_E_BASE.

A '-' has mask 16 (seq_overlap.h:138): it meets no base and no IUPAC code, but q & t > 0 (seq_overlap.cpp:157-161) holds for '-' against
'-', so a gap in a read matches a gap in a target.  The model follows the reference's source there.

    python -m tests.adapter_edges        prints the number of cases per edge
"""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

f32 = np.float32
# restated; test_adapter_edges_model.py compares them with faqcs_dev.h, include/faqcs_mi.h and the launcher
GROUP, TPL_CAP, SINGLE_LENGTH, BB_CAP = 64, 4096, 8192, 136
PAIR_LEN, PAIR_TARGETS, PAIR_TLEN = 160, 32, 128
WIDTHS = (256, 320, 1024, 4096, 8192, 16384, 32768)
MAX_READ_LENGTH, MAX_ADAPTER_LENGTH = 32767, 32767
CONSTANT_SOURCES = {
    "GROUP": ("faqcs_amd/csrc/faqcs_dev.h", r"#define FAQCS_ADAPTER_GROUP (\d+)"),
    "TPL_CAP": ("faqcs_amd/csrc/faqcs_dev.h", r"#define FAQCS_ADAPTER_TPL_CAP (\d+)"),
    "SINGLE_LENGTH": ("faqcs_amd/csrc/faqcs_dev.h", r"#define FAQCS_ADAPTER_SINGLE_LENGTH (\d+)"),
    "BB_CAP": ("faqcs_amd/csrc/faqcs_adapter_kernel.hip", r"constexpr int BB_CAP = (\d+);"),
    "MAX_READ_LENGTH": ("include/faqcs_mi.h", r"#define FAQCS_MAX_READ_LENGTH (\d+)"),
    "MAX_ADAPTER_LENGTH": ("include/faqcs_mi.h", r"#define FAQCS_MAX_ADAPTER_LENGTH (\d+)"),
}
# the launcher's gates as launch_adapter states them, in its order
LAUNCHER_SOURCES = (
    (r"max_len <= (\d+) && A\.n_adapters <= (\d+) && A\.longest <= (\d+) && A\.plane_dwords <= (\d+) && \(dbg & 8u\) == 0u", (PAIR_LEN, PAIR_TARGETS, PAIR_TLEN, TPL_CAP)),
    (r"if \(max_len <= (\d+)\) \{\s+constexpr int NW = 4;", (256,)),
    (r"\} else if \(max_len <= (\d+)\) \{ // MiSeq", (320,)),
    (r"\} else if \(max_len <= (\d+)\) \{\s+constexpr int NW = 8;", (1024,)),
    (r"if \(max_len <= (\d+)\) FAQCS_ADAPTER_LONG\((\d+), 5u\)", (4096, 4096)),
    (r"else if \(max_len <= (\d+)\) FAQCS_ADAPTER_LONG\((\d+), 4u\)", (8192, 8192)),
    (r"else if \(max_len <= (\d+)\) FAQCS_ADAPTER_LONG\((\d+), 2u\)", (16384, 16384)),
    (r"else FAQCS_ADAPTER_LONG\((\d+), 1u\)", (32768,)),
)
F_VALID, F_ADAPTER, F_ERR_BASE, E_BASE = 0x1, 0x20, 0x200, -4
SETTINGS = ("default", "prefilter_off", "no_pair")
# nothing for the trim stage to decide: no length filter but the empty window, no poly-N, average-quality or low-complexity filter; under --mode hard
# qualities of 'I' cut nothing (BWA_plus empties a window of one base, trim.cpp:781-786)
BASE_ARGS = ["--mode", "hard", "--min_L", "0", "-n", "100000", "--lc", "1", "--avg_q", "0"]
RESULT_DTYPE = np.dtype([("start", "<u2"), ("len", "<u2"), ("flags", "<u2"), ("adapter", "<u2")])

# seq_overlap.h:133-150 / seq_overlap.cpp:372-411, restated: A 1, C 2, G 4, T 8, the IUPAC codes their unions, '-' 16, anything else rejected
_CODES = {"A": 1, "C": 2, "G": 4, "T": 8, "M": 3, "R": 5, "S": 6, "V": 7, "W": 9, "Y": 10, "H": 11, "K": 12, "D": 13, "B": 14, "N": 15}


def _table(gap):
    t = np.zeros(256, np.uint8)
    for ch, v in _CODES.items():
        t[ord(ch)] = t[ord(ch.lower())] = v
    t[ord("-")] = gap
    return t


NA = _table(16)
MUTANTS = ("first_cell_wins_a_tie", "start_resets_at_M<=0", "threshold_in_double", "threshold_from_the_reads_own_length", "tail_group_takes_the_min",
           "stale_range_dropped", "stale_range_before_any_state", "find_mask_range_resets_at_every_masked_base", "credit_on_>=", "gap_matches_every_base",
           "gap_matches_nothing")


# =====================================================================================================================================
# the model
# =====================================================================================================================================
class Hit:
    """One (read, target): any a cell matches, score / start / stop what the aligner reports (stale: start / stop from target `src`), (i, j) the
    winning cell, diag = j - i + qlen - 1 its diagonal, block = diag // 64, cells the maximal cells (up to 64), counts the matches per diagonal,
    thr the threshold and m the length it was taken from, num_match, used: a range was there to judge, masked, credited"""
    __slots__ = ("t", "tlen", "any", "score", "start", "stop", "i", "j", "diag", "block", "cells", "counts", "thr", "m", "num_match", "stale", "src", "used", "masked",
                 "credited", "ndiag")


def align(qb, tb, mutant=None):
    """-> (any, score, start, stop, i, j, cells, counts) of the bit masks qb (read) and tb (target); seq_overlap.cpp:46-370 for one of the 8 lanes.
    Every cell depends on its diagonal neighbour only, so the sweep may run along either sequence: one position of the shorter per step."""
    n, m = len(qb), len(tb)
    match = (qb[:, None] & tb[None, :]) != 0 if n * m else np.zeros((n, m), bool)
    counts = np.bincount((np.arange(m)[None, :] - np.arange(n)[:, None] + n - 1)[match], minlength=max(n + m - 1, 0)) if n * m else np.zeros(0, np.int64)
    by_read = n <= m                       # the outer loop walks the read (rows) or the target (columns)
    outer, inner = (n, m) if by_read else (m, n)
    M = np.zeros(inner, np.int64)          # the previous step's cells; in front of the first step M = 0 everywhere (seq_overlap.cpp:85-101, :109-117)
    S = np.zeros(inner, np.int64)
    best, key, start, cells = None, None, 0, []
    pos = np.arange(inner)
    for k in range(outer):
        s = np.where(match[k, :] if by_read else match[:, k], 1, -1)
        pm = np.concatenate(([0], M[:-1]))                      # the diagonal neighbour; 0 on the border
        ps = np.concatenate(([0], S[:-1]))
        here = k if by_read else pos                            # the read index of this step's cells
        fresh = (pm <= 0) if mutant == "start_resets_at_M<=0" else (pm < 0)   # seq_overlap.cpp:255, :272-275: only below 0 (Q3)
        fresh[0] = True                                         # the first row and the first column start at their own read position
        if k == 0:
            fresh[:] = True
        S = np.where(fresh, here, ps)
        M = np.maximum(pm, 0) + s
        mx = int(M.max())
        if mx < 0 or (best is not None and mx < best):
            continue
        at = np.nonzero(M == mx)[0]
        ij = [(k, int(x)) if by_read else (int(x), k) for x in at]
        if best is None or mx > best:
            best, key, cells = mx, None, []
        cells = (cells + ij)[:64] if len(cells) < 64 else cells
        top = min(ij) if mutant == "first_cell_wins_a_tie" else max(ij)
        if key is None or ((top < key) if mutant == "first_cell_wins_a_tie" else (top > key)):
            key = top
            start = int(S[top[1] if by_read else top[0]])
    if best is None:
        return False, 0, 0, 0, 0, 0, [], counts
    return True, best, start, key[0], key[0], key[1], cells, counts


def threshold(rate, m, mutant=None):
    """trim.cpp:969, :1007-1008: float(1.0 - rate) * m in float, cut to int"""
    if mutant == "threshold_in_double":
        return int((1.0 - float(rate)) * m)                 # (on the option as it was typed)
    match_rate = f32(1.0 - float(f32(float(rate))))
    return int(f32(match_rate * f32(m)))


def find_mask_range(mask, mutant=None):
    """trim.cpp:1144-1189, literal: mask[i] True = unmasked"""
    longest_start = longest = run_start = run = 0
    for i, ok in enumerate(mask):
        if not ok:
            if run > longest:
                longest, longest_start, run = run, run_start, 0
            elif mutant == "find_mask_range_resets_at_every_masked_base":
                run = 0
        else:
            if run == 0:
                run_start = i
            run += 1
    if run > longest:
        longest, longest_start = run, run_start
    return (longest_start, longest) if longest else (0, 0)


class Info:
    """One read: qlen, bad (a rejected byte), group (index in the segment // 8), tail, len8 (the length the threshold takes its min with, None in a
    tail group), hits [Hit per target], mask, first / second the window, credit (0: none), unmasked runs"""
    __slots__ = ("seq", "qlen", "bad", "sub", "seg", "at", "index", "tail", "len8", "hits", "mask", "first", "second", "credit")


def model_read(seq, lib_bits, rate, tail, len8, mutant=None, na=NA):
    """one read against the library; len8: the length of the last read of its group of 8 (of what there is of the group, in a tail group)"""
    I = Info()
    I.seq, I.qlen, I.tail, I.len8 = seq, len(seq), tail, None if tail else len8
    qb = na[np.frombuffer(seq, np.uint8)] if seq else np.zeros(0, np.uint8)
    I.bad = bool((qb == 0).any())
    I.hits, I.first, I.second, I.credit = [], 0, len(seq), 0
    I.mask = [True] * len(seq)
    if I.bad:
        return I
    best, best_j = 0, 0
    have, rs, re, src = mutant == "stale_range_before_any_state", 0, 0, -1
    for t, tb in enumerate(lib_bits):
        h = Hit()
        h.t, h.tlen, h.ndiag = t, len(tb), len(seq) + len(tb) - 1
        h.any, h.score, a, b, h.i, h.j, h.cells, h.counts = align(qb, tb, mutant)
        h.diag = h.j - h.i + len(seq) - 1
        h.block = h.diag // 64
        own = len(seq) if mutant == "threshold_from_the_reads_own_length" else len8
        h.m = len(tb) if tail and mutant != "tail_group_takes_the_min" else min(own, len(tb))
        h.thr = threshold(rate, h.m, mutant)
        h.stale, h.used, h.masked, h.credited = False, False, False, False
        if h.any:
            have, rs, re, src = True, a, b, t
        elif have and mutant != "stale_range_dropped":
            h.stale = True                                   # H2: score 0 with the range the aligner still holds
        else:
            h.start = h.stop = h.num_match = 0
            h.src = -1
            I.hits.append(h)
            continue
        h.used, h.start, h.stop, h.src = True, rs, re, src
        h.num_match = (re - rs + 1 + h.score) // 2           # trim.cpp:1024-1025
        if h.num_match >= h.thr:
            h.masked = True
            for k in range(rs, re + 1):
                if k < len(I.mask):                          # (only the mutant that invents a range for an empty read gets here with k outside)
                    I.mask[k] = False
            if h.score > best or (mutant == "credit_on_>=" and h.score >= best and h.score > 0):
                best, best_j = h.score, t
        I.hits.append(h)
    if best > 0:
        I.first, I.second = find_mask_range(I.mask, mutant)
        I.credit = best_j + 1
        I.hits[best_j].credited = True
    return I


def run_model(case, mutant=None):
    """-> dict(results=[array per submission], stats=[reads, bases per target], error, info=[Info per read])"""
    na = _table(15) if mutant == "gap_matches_every_base" else (_table(32) if mutant == "gap_matches_nothing" else NA)
    lib_bits = [(_table(64) if mutant == "gap_matches_nothing" else na)[np.frombuffer(t.encode(), np.uint8)] for _, t in case.lib]
    rate = case.args[case.args.index("--rate") + 1] if "--rate" in case.args else "0.2"   # the option as typed; CPU test: float32 of it is the parsed option
    stats = np.zeros(2 * len(case.lib), np.uint64)
    results, info, error, index = [], [], 0, 0
    for k, sub in enumerate(case.subs):
        res = np.zeros(sum(len(seg) for seg in sub), RESULT_DTYPE)
        r = 0
        for s, seg in enumerate(sub):
            for at, seq in enumerate(seg):
                g_last = at // 8 * 8 + 7                     # Q1: the threshold of a full group of 8 comes from its LAST read, a tail group takes no min
                tail = g_last >= len(seg)
                I = model_read(seq, lib_bits, rate, tail, len(seg[min(g_last, len(seg) - 1)]), mutant, na)
                I.sub, I.seg, I.at, I.index = k, s, at, index
                index += 1
                info.append(I)
                if I.bad:
                    error = E_BASE
                    res[r] = (0, 0, F_ERR_BASE, 0)
                else:
                    flags, start, ln = 0, 0, I.qlen
                    if I.qlen != I.second:                   # trim.cpp:270-277
                        flags |= F_ADAPTER
                        start, ln = (I.qlen if I.second == 0 else I.first), I.second
                    if I.credit:
                        stats[2 * (I.credit - 1)] += 1
                        stats[2 * (I.credit - 1) + 1] += I.qlen - I.second
                    res[r] = (start, ln, flags | F_VALID, I.credit) if ln else (0, 0, flags, I.credit)
                r += 1
        results.append(res)
    return dict(results=results, stats=stats, error=error, info=info)


# ---- the dispatch, restated from launch_adapter (faqcs_adapter_kernel.hip) and the group partition of faqcs_create (faqcs_capi.hip) -------------
def plane_words(tlen):
    return (tlen + 31) // 32


def partition(tlens):
    """-> None for a set that runs in one pass, else [(first target, targets, longest, plane dwords)] of the groups"""
    if len(tlens) <= GROUP and max(tlens) <= SINGLE_LENGTH:
        return None
    out, j = [], 0
    while j < len(tlens):
        j0, words, longest = j, 0, 0
        while j < len(tlens) and j - j0 < GROUP and 4 * (words + plane_words(tlens[j])) <= TPL_CAP:
            words, longest, j = words + plane_words(tlens[j]), max(longest, tlens[j]), j + 1
        assert j > j0, "a target that fits no group"
        out.append((j0, j - j0, longest, 4 * words))
    return out


def variant(max_len, n_targets, longest, plane_dwords, grouped, pair_on=True, prefilter_on=True):
    """-> (kernel, planes cached): the kernel one launch takes -- "pair", or the width of adapter_overlap -- and whether the targets' planes fit its LDS copy"""
    cached = plane_dwords <= TPL_CAP
    if not grouped and pair_on and prefilter_on and max_len <= PAIR_LEN and n_targets <= PAIR_TARGETS and longest <= PAIR_TLEN and cached:
        return "pair", True
    for w in WIDTHS:
        if max_len <= w:
            return ("grouped_%d" if grouped else "%d") % w, cached
    raise ValueError("a read of %d bases" % max_len)


def launches(tlens, max_len, setting="default", gap=False):
    """[(kernel, cached, first target, targets)] of one submission whose longest read has max_len bases.  gap: a target of the library holds a '-';
    the base planes do not see a '-' of a read against it, so such a library runs as under prefilter_off (AdapterDev::has_gap)"""
    pair_on, pre = setting != "no_pair", setting != "prefilter_off" and not gap
    groups = partition(tlens)
    if groups is None:
        return [variant(max_len, len(tlens), max(tlens), 4 * sum(map(plane_words, tlens)), False, pair_on, pre) + (0, len(tlens))]
    return [variant(max_len, n, longest, dwords, True, pair_on, pre) + (j0, n) for j0, n, longest, dwords in groups]


def stage1_width(kernel, qlen, tlens):
    """NBR of adapter_overlap's stage 1 for one read: blocks of 64 diagonals its register windows cover (None: another kernel)"""
    w = int(kernel.split("_")[-1]) if kernel != "pair" else 0
    if w == 320:
        return 7
    if w != 256:
        return None
    short = max([t for t in tlens if t <= 128] or [0])
    return 4 if not any(t > 128 for t in tlens) and qlen + short - 1 <= 256 else 6


NB_LO = {4: 3, 6: 4, 7: 5}


# =====================================================================================================================================
# cases
# =====================================================================================================================================
class ACase:
    """name, the library [(name, sequence)], the option list behind BASE_ARGS, submissions of segments of reads (bytes), the edges it claims;
    R the engine's longest read; exclude: {setting: reason}"""

    def __init__(self, name, lib, args, subs, claims, R=None):
        self.name, self.args, self.subs, self.claims = name, [str(a) for a in args], subs, tuple(claims)
        self.lib = [(n, t) for n, t in lib]
        self.longest = max([len(r) for sub in subs for seg in sub for r in seg] or [0])
        self.R = R or next(w for w in (256, 1024, 4096, MAX_READ_LENGTH) if self.longest <= w)
        self.exclude = {}
        self._exp = self._ctx = self._opt = None
        self.in_off = 33
        self.tlens = [len(t) for _, t in self.lib]
        if "--polyA" in self.args:
            assert self.lib[-1] == ("polyA", "A" * 20), "%s: --polyA appends the polyA target" % name

    def opt(self):
        """the options of the case: --adapter with the case's library in place of the built-in set (--polyA appends its target, as options.cpp does)"""
        from faqcs_amd.options import parse_args

        o = parse_args(["-u", "x", "-d", "y", "--adapter"] + BASE_ARGS + self.args)
        o.adapter = [a for a in self.lib if a[0] != "polyA"] + [a for a in o.adapter if a[0] == "polyA"]
        assert o.adapter == self.lib and not o.print_usage, self.name
        return o

    def records(self, k):
        """submission k as segments of (id, seq, qual)"""
        return [[(b"@r", s, b"I" * len(s)) for s in seg] for seg in self.subs[k]]

    def expected(self):
        if self._exp is None:
            self._exp = run_model(self)
        return self._exp

    def n_reads(self):
        return sum(len(seg) for sub in self.subs for seg in sub)

    def launches(self, k, setting="default"):
        return launches(self.tlens, max([len(r) for seg in self.subs[k] for r in seg] or [0]), setting, any("-" in t for _, t in self.lib))

    def takes_pair(self):
        return any(l[0] == "pair" for k in range(len(self.subs)) if sum(map(len, self.subs[k])) for l in self.launches(k))

    def ctx(self):
        if self._ctx is None:
            self._ctx = Ctx(self)
        return self._ctx


class Ctx:
    """What the predicates look at: the case, the model's Info per read, and (Info, Hit) pairs with the launch that holds the target"""

    def __init__(self, case):
        self.case, self.tlens = case, case.tlens
        e = case.expected()
        self.error, self.info, self.stats = e["error"], e["info"], e["stats"]
        self.kern = [case.launches(k) for k in range(len(case.subs))]
        self.maxlen = [max([len(r) for seg in sub for r in seg] or [0]) for sub in case.subs]
        self.ih = [(i, h) for i in self.info for h in i.hits]
        self.grouped = partition(case.tlens) is not None
        self.lib = [t for _, t in case.lib]

    def launch_of(self, i, h):
        return next(l for l in self.kern[i.sub] if l[2] <= h.t < l[2] + l[3])

    def kernels(self):
        return {l[0] for ls in self.kern for l in ls}

    def by_sub(self, k):
        return [i for i in self.info if i.sub == k]


_RNG = np.random.Generator(np.random.PCG64(20261020))
_POOL = {alpha: np.frombuffer(alpha.encode(), np.uint8)[_RNG.integers(0, len(alpha), 1 << 17)].tobytes() for alpha in ("ACG", "AG", "ACGT")}


def tg(n, salt=0, alpha="ACG"):
    """a target of n bases over an alphabet without T: a different stretch of a fixed pool for every salt"""
    pool = _POOL[alpha]
    at = (salt * 7919 + 13) % (len(pool) - n)
    return pool[at:at + n].decode()


def rd(n, *plants, fill=b"T"):
    """a read of n bases of T (which no target of the catalogue holds) with pieces written over it: (position, text)"""
    s = bytearray(fill * n)
    for p, text in plants:
        text = text.encode() if isinstance(text, str) else text
        assert 0 <= p and p + len(text) <= n, (n, p, len(text))
        s[p:p + len(text)] = text
    return bytes(s)


def spoil(text, every, start=0):
    """text with every `every`-th base from `start` replaced by T: a mismatch on the diagonal"""
    s = bytearray(text.encode() if isinstance(text, str) else text)
    for k in range(start, len(s), every):
        s[k] = ord("T")
    return bytes(s)


def scatter(text):
    """two bases of every five kept, three replaced by T: two fifths of the diagonal match and no alignment is longer than two bases"""
    s = bytearray(text.encode() if isinstance(text, str) else text)
    for k in range(len(s)):
        if k % 5 >= 2:
            s[k] = ord("T")
    return bytes(s)


def one(reads):
    return [[list(reads)]]


EDGES = {}


def edge(name):
    def reg(f):
        EDGES[name] = f
        return f
    return reg


def diag_cells(i, h):
    """[(read position, target position)] of the cells of the winning alignment"""
    return [(x, x + h.j - h.i) for x in range(h.start, h.stop + 1)]


def path_touches_zero(c, i, h):
    """the running score along the winning alignment returns to exactly 0 behind its start and goes on (Q3)"""
    if not h.any or h.stale:
        return False
    qb, tb = NA[np.frombuffer(i.seq, np.uint8)], NA[np.frombuffer(c.lib[h.t].encode(), np.uint8)]
    M, seen = 0, False
    for x, y in diag_cells(i, h):
        if not 0 <= y < len(tb):
            return False
        M = max(M, 0) + (1 if qb[x] & tb[y] else -1)
        seen = seen or (M == 0 and x < h.stop)
    return seen and M == h.score


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------------
def _kernel_at(L, name):
    return lambda c: any(m == L and ls[0][0] == name for m, ls in zip(c.maxlen, c.kern))


for _L, _k in ((160, "pair"), (161, "256"), (256, "256"), (257, "320"), (320, "320"), (321, "1024"), (1024, "1024"), (1025, "4096"), (4096, "4096"), (4097, "8192")):
    edge("dispatch:longest_read_%d_takes_%s" % (_L, _k))(_kernel_at(_L, _k))
for _w in (8192, 16384, 32768):
    edge("dispatch:long_width_%d_with_a_hit" % _w)(lambda c, w=_w: any(ls[0][0] == str(w) and any(i.credit and i.qlen > w // 2 for i in c.by_sub(k)) for k, ls in enumerate(c.kern)))
edge("dispatch:32_targets_take_pair")(lambda c: len(c.tlens) == 32 and c.kernels() == {"pair"})
edge("dispatch:33_targets_take_256")(lambda c: len(c.tlens) == 33 and c.kernels() == {"256"} and max(c.maxlen) <= 160 and max(c.tlens) <= 128)
edge("dispatch:longest_target_128_takes_pair")(lambda c: max(c.tlens) == 128 and c.kernels() == {"pair"})
edge("dispatch:longest_target_129_takes_256")(lambda c: max(c.tlens) == 129 and c.kernels() == {"256"} and max(c.maxlen) <= 160 and len(c.tlens) <= 32)
edge("dispatch:64_targets_in_one_pass")(lambda c: len(c.tlens) == 64 and not c.grouped and any(i.credit == 64 for i in c.info))
edge("dispatch:65_targets_are_grouped")(lambda c: len(c.tlens) == 65 and c.grouped and any(i.credit == 65 for i in c.info))
edge("dispatch:longest_target_8192_in_one_pass")(lambda c: max(c.tlens) == 8192 and not c.grouped and any(h.masked and h.tlen == 8192 for _, h in c.ih))
edge("dispatch:longest_target_8193_is_grouped")(lambda c: max(c.tlens) == 8193 and c.grouped and any(h.masked and h.tlen == 8193 for _, h in c.ih))
for _w in ("256", "320"):
    edge("dispatch:uncached_single_pass_%s" % _w)(lambda c, w=_w: not c.grouped and any(ls[0] == (w, False) + ls[0][2:] and any(i.credit for i in c.by_sub(k)) for k, ls in enumerate(c.kern)))
    edge("dispatch:the_same_library_cut_to_the_cap_%s" % _w)(lambda c, w=_w: not c.grouped and max(c.tlens) > 6000 and any(ls[0] == (w, True) + ls[0][2:] and any(i.credit for i in c.by_sub(k)) for k, ls in enumerate(c.kern)))


def _nbr(c, i):
    return stage1_width(c.kern[i.sub][0][0], i.qlen, c.tlens)


edge("dispatch:stage1_width_4_at_256_diagonals")(lambda c: any(_nbr(c, i) == 4 and i.qlen + max(c.tlens) - 1 == 256 and i.credit for i in c.info))
edge("dispatch:stage1_width_6_at_257_diagonals")(lambda c: max(c.tlens) <= 128 and any(_nbr(c, i) == 6 and i.qlen + max(c.tlens) - 1 == 257 and i.credit for i in c.info))
edge("dispatch:stage1_width_6_by_a_long_target")(lambda c: any(_nbr(c, i) == 6 and i.qlen + max(t for t in c.tlens if t <= 128) - 1 <= 256 and i.credit for i in c.info))
for _n in (4, 6, 7):
    edge("dispatch:stage1_width_%d_blocks_at_%d_and_%d" % (_n, NB_LO[_n], NB_LO[_n] + 1))(lambda c, n=_n: {(h.ndiag + 63) // 64 for i, h in c.ih if _nbr(c, i) == n and h.tlen <= 128 and h.masked} >= {NB_LO[n], NB_LO[n] + 1})

# ---- target shapes ----------------------------------------------------------------------------------------------------------------------
TARGET_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129)
for _t in TARGET_LENGTHS:
    edge("target:%d_bases_credited" % _t)(lambda c, t=_t: any(h.credited and h.tlen == t for _, h in c.ih))
edge("target:every_class_in_one_library_out_of_class_order")(lambda c: {plane_words(t) for t in c.tlens} >= {1, 2, 3, 4, 5} and
                                                             [plane_words(t) for t in c.tlens] != sorted(plane_words(t) for t in c.tlens) and
                                                             {plane_words(h.tlen) for _, h in c.ih if h.credited} >= {1, 2, 3, 4, 5})
edge("target:iupac_codes")(lambda c: any(h.credited and set(c.lib[h.t][y] for _, y in diag_cells(i, h)) >= set("RYSWKMBDHV") for i, h in c.ih))
edge("target:lower_case")(lambda c: any(h.credited and c.lib[h.t].islower() for _, h in c.ih))
edge("target:N_matches_every_base")(lambda c: any(h.credited and "N" in c.lib[h.t][h.j - (h.stop - h.start):h.j + 1] and h.score == h.stop - h.start + 1 for _, h in c.ih))
edge("target:gap_matches_no_base")(lambda c: any(h.masked and not h.stale and "-" in c.lib[h.t][h.j - (h.stop - h.start):h.j + 1] and b"-" not in i.seq for i, h in c.ih))
edge("target:no_base_plane_shared_with_the_read")(lambda c: any(not h.any and i.qlen and set(c.lib[h.t]) <= set("ACG") and set(i.seq) <= set(b"T") for i, h in c.ih))

# ---- read shapes ------------------------------------------------------------------------------------------------------------------------
READ_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129)
for _n in READ_LENGTHS:
    edge("read:%d_bases" % _n)(lambda c, n=_n: any(i.qlen == n and (n == 0 or i.credit) for i in c.info) and any(i.qlen == n and not i.credit for i in c.info))
edge("read:only_gaps")(lambda c: any(i.qlen > 8 and set(i.seq) == set(b"-") and not i.bad and not any(h.any for h in i.hits) for i in c.info))
edge("read:a_gap_against_a_gap_in_the_target")(lambda c: any(h.masked and not h.stale and any(i.seq[x:x + 1] == b"-" and c.lib[h.t][y] == "-" for x, y in diag_cells(i, h)) for i, h in c.ih))
edge("read:N_matches_every_target_base")(lambda c: any(h.credited and i.seq[h.start:h.stop + 1].count(b"N") >= 3 and h.score == h.stop - h.start + 1 for i, h in c.ih))


def _leftover(c, step):
    """a read whose score against some target would grow if the bases of the read `step` places before it, behind its own end, were still there"""
    out = []
    for i in c.info:
        if i.at >= step and i.index % 64 >= step:
            p = c.info[i.index - step]
            if p.sub == i.sub and not p.bad and not i.bad and p.qlen >= (i.qlen + 63) // 64 * 64 + 8 and i.qlen:
                ghost = NA[np.frombuffer(i.seq + p.seq[i.qlen:], np.uint8)]
                for h in i.hits:
                    tb = NA[np.frombuffer(c.lib[h.t].encode(), np.uint8)]
                    if h.any and align(ghost, tb)[1] > h.score and h.masked:
                        out.append(i)
    return out


edge("read:short_behind_long_in_one_wave_slot")(lambda c: "pair" not in c.kernels() and len(_leftover(c, 1)) > 0)
edge("read:short_behind_long_in_either_half_of_the_pair_kernel")(lambda c: c.kernels() == {"pair"} and {i.index % 2 for i in _leftover(c, 2)} == {0, 1})


# ---- aligner ----------------------------------------------------------------------------------------------------------------------------
def _blocks(h, qlen):
    return sorted({(y - x + qlen - 1) // 64 for x, y in h.cells})


def _bounds(h):
    """per 64-diagonal block the largest match count of a diagonal: what the bound pass of align_exact orders the blocks by"""
    n = (h.ndiag + 63) // 64
    return [int(h.counts[64 * b:64 * b + 64].max()) for b in range(n)]


def _tie(c, pred):
    return any(h.masked and not h.stale and h.score > 0 and len({y - x for x, y in h.cells}) >= 2 and pred(i, h, {y - x + i.qlen - 1 for x, y in h.cells}) for i, h in c.ih)


edge("aligner:tie_on_two_diagonals_of_one_block")(lambda c: _tie(c, lambda i, h, d: len({x // 64 for x in d}) == 1))
edge("aligner:tie_on_diagonals_63_and_64")(lambda c: _tie(c, lambda i, h, d: any(x % 64 == 63 and x + 1 in d for x in d)))
edge("aligner:tie_in_blocks_far_apart")(lambda c: _tie(c, lambda i, h, d: max(d) // 64 - min(d) // 64 >= 3))
edge("aligner:tie_in_a_long_target")(lambda c: _tie(c, lambda i, h, d: h.tlen > 128 and len({x // 64 for x in d}) >= 2))
edge("aligner:the_block_visited_first_does_not_win_the_tie")(lambda c: _tie(c, lambda i, h, d: len({x // 64 for x in d}) >= 2 and _bounds(h).index(max(_bounds(h))) != h.block and
                                                                            _bounds(h).index(max(_bounds(h))) in {x // 64 for x in d}))
edge("aligner:a_block_whose_bound_equals_the_best_score_wins")(lambda c: _tie(c, lambda i, h, d: len({x // 64 for x in d}) >= 2 and _bounds(h)[h.block] == h.score and
                                                                              _bounds(h).index(max(_bounds(h))) != h.block))
edge("aligner:last_row_major_cell_larger_i")(lambda c: _tie(c, lambda i, h, d: (h.i, h.j) == max(h.cells) and len({x for x, _ in h.cells}) >= 2 and min(h.cells)[1] > h.j))
edge("aligner:last_row_major_cell_larger_j_in_one_row")(lambda c: any(h.masked and sum(1 for x, y in h.cells if x == h.i) >= 2 and h.j == max(y for x, y in h.cells if x == h.i) for _, h in c.ih))
edge("aligner:winner_on_lane_0")(lambda c: any(h.credited and h.diag % 64 == 0 and h.diag >= 64 for _, h in c.ih))
edge("aligner:winner_on_lane_63")(lambda c: any(h.credited and h.diag % 64 == 63 for _, h in c.ih))
edge("aligner:diagonals_64k")(lambda c: any(h.credited and h.ndiag % 64 == 0 and h.block == h.ndiag // 64 - 1 for _, h in c.ih) and any(h.credited and h.ndiag % 64 == 0 and h.block == 0 for _, h in c.ih))
# (the block past 64 k diagonals holds one cell; the winner lies in the last whole block)
edge("aligner:diagonals_64k+1")(lambda c: any(h.credited and h.ndiag % 64 == 1 and h.block == h.ndiag // 64 - 1 for _, h in c.ih))
edge("aligner:alignment_from_i=0_j=0")(lambda c: any(h.credited and h.start == 0 and h.j - (h.stop - h.start) == 0 for _, h in c.ih))
edge("aligner:alignment_to_the_last_base_of_both")(lambda c: any(h.credited and h.stop == i.qlen - 1 and h.j == h.tlen - 1 for i, h in c.ih))
edge("aligner:target_hangs_off_the_reads_start")(lambda c: any(h.credited and h.start == 0 and h.j - (h.stop - h.start) > 0 for _, h in c.ih))
edge("aligner:target_hangs_off_the_reads_end")(lambda c: any(h.credited and h.stop == i.qlen - 1 and h.j < h.tlen - 1 for i, h in c.ih))
edge("aligner:score_touches_0_and_the_start_survives")(lambda c: any(h.masked and path_touches_zero(c, i, h) for i, h in c.ih))
edge("aligner:best_score_in_the_last_partial_plane_word")(lambda c: any(h.credited and h.tlen % 32 and h.j // 32 == (h.tlen - 1) // 32 and h.tlen > 32 for _, h in c.ih))


# ---- filters ----------------------------------------------------------------------------------------------------------------------------
def _stage1(c, i, h):
    """which stage-1 filter meets the pair: "blocked" (register-blocked, 1 - 4 plane words), "sliding" (long target, cached), "uncached", or None"""
    k, cached = c.launch_of(i, h)[:2]
    if any("-" in t for t in c.lib):
        return None
    if k == "pair":
        return "blocked"
    w = int(k.split("_")[-1])
    if w <= 320 and cached:
        return "blocked" if h.tlen <= 128 else "sliding"
    return "uncached"


def _need_cnt(i, h):
    need = 2 * h.thr - min(i.qlen, h.tlen)
    return max(need, h.thr)


for _f in ("blocked", "sliding", "uncached"):
    edge("filters:%s:num_match=thr" % _f)(lambda c, f=_f: any(_stage1(c, i, h) == f and not h.stale and h.masked and h.num_match == h.thr > 4 for i, h in c.ih))
    edge("filters:%s:num_match=thr-1" % _f)(lambda c, f=_f: any(_stage1(c, i, h) == f and not h.stale and h.any and not h.masked and h.num_match == h.thr - 1 > 4 for i, h in c.ih))
    edge("filters:%s:count_reaches_need_cnt_and_no_alignment_reaches_thr" % _f)(lambda c, f=_f: any(
        _stage1(c, i, h) == f and h.any and not h.masked and h.thr > 4 and int(h.counts.max()) >= _need_cnt(i, h) and h.num_match < h.thr // 2 for i, h in c.ih))


def _first_word(c, i, h):
    """matches of the winning diagonal on the target's first plane word"""
    tb, qb = NA[np.frombuffer(c.lib[h.t].encode(), np.uint8)], NA[np.frombuffer(i.seq, np.uint8)]
    return sum(1 for y in range(min(32, h.tlen)) if 0 <= y - (h.j - h.i) < i.qlen and qb[y - (h.j - h.i)] & tb[y])


edge("filters:two_word_target_met_behind_its_first_word")(lambda c: any(
    32 < h.tlen <= 64 and h.credited and h.start == 0 and h.j == h.tlen - 1 and _first_word(c, i, h) == max(_need_cnt(i, h) - (h.tlen - 32), 0) < h.num_match / 2
    for i, h in c.ih))
edge("filters:polyA_16_of_20")(lambda c: "--polyA" in c.case.args and any(h.t == len(c.tlens) - 1 and h.credited and h.num_match == h.thr == 16 for _, h in c.ih) and
                               any(h.t == len(c.tlens) - 1 and h.any and not h.masked and h.num_match == 15 for _, h in c.ih))

# ---- threshold --------------------------------------------------------------------------------------------------------------------------
edge("thr:last_of_8_shorter_than_the_target")(lambda c: any(not i.tail and i.at % 8 < 7 and h.masked and not h.stale and i.len8 < h.tlen and h.num_match < threshold(0.2, h.tlen) for i, h in c.ih))
edge("thr:last_of_8_longer_than_the_target")(lambda c: any(not i.tail and i.at % 8 < 7 and h.any and not h.masked and i.qlen < h.tlen < i.len8 and h.num_match >= threshold(0.2, i.qlen) for i, h in c.ih))
edge("thr:last_of_8_empty")(lambda c: any(not i.tail and i.len8 == 0 and i.credit and sum(h.masked for h in i.hits) >= 2 and any(h.masked and h.thr == 0 and h.num_match < 3 for h in i.hits) for i in c.info))
edge("thr:tail_group_takes_no_min")(lambda c: any(i.tail and h.any and not h.masked and h.m == h.tlen > i.qlen and h.num_match >= threshold(0.2, i.qlen) for i, h in c.ih))
edge("thr:group_of_8_across_a_64_read_chunk")(lambda c: any(not i.tail and (i.index - i.at % 8 + 7) // 64 > i.index // 64 and h.masked and not h.stale and i.len8 < h.tlen and
                                                            h.num_match < threshold(0.2, h.tlen) for i, h in c.ih))
edge("thr:segments_that_are_no_multiple_of_8")(lambda c: any(len(sub) >= 3 and all(len(seg) % 8 for seg in sub if seg) and any(i.credit and i.seg == len(sub) - 1 for i in c.by_sub(k))
                                                             for k, sub in enumerate(c.case.subs)))
edge("thr:empty_segment")(lambda c: any(any(len(seg) == 0 for seg in sub[:-1]) and len(sub[-1]) == 0 and any(i.credit and i.seg > 0 for i in c.by_sub(k)) for k, sub in enumerate(c.case.subs)))
FLOAT_THR = {5: (1, 2), 10: (3, 4), 20: (7, 8), 40: (15, 16)}
for _t, (_thr, _exact) in FLOAT_THR.items():
    edge("thr:rate_0.6_against_%d_bases_is_%d" % (_t, _thr))(lambda c, t=_t, v=_thr: c.case.args == ["--rate", "0.6"] and
                                                             any(h.tlen == t and h.thr == v == h.num_match and h.masked and not h.stale for _, h in c.ih) and
                                                             any(h.tlen == t and h.thr == v == h.num_match + 1 and not h.masked and not h.stale for _, h in c.ih))
edge("thr:rate_0.35_against_180_bases_is_116")(lambda c: c.case.args == ["--rate", "0.35"] and any(h.tlen == 180 and h.thr == 116 == h.num_match and h.credited for _, h in c.ih) and
                                               any(h.tlen == 180 and h.num_match == 115 and not h.masked for _, h in c.ih))

# ---- state ------------------------------------------------------------------------------------------------------------------------------
edge("state:stale_range_after_a_target_that_aligned")(lambda c: any(h.stale and h.masked and i.hits[h.src].masked and h.src == h.t - 1 for i, h in c.ih))
edge("state:stale_range_after_a_target_that_could_not_pass")(lambda c: any(h.stale and h.masked and not i.hits[h.src].masked and int(i.hits[h.src].counts.max()) < _need_cnt(i, i.hits[h.src]) and
                                                                           i.credit and not i.mask[h.start] for i, h in c.ih))
edge("state:no_range_before_any_target")(lambda c: any(not h.any and not h.used and h.t == 0 and h.thr == 0 and i.credit for i, h in c.ih))
edge("state:score_0_masks_without_credit")(lambda c: any(h.stale and h.masked and h.score == 0 and not h.credited and i.credit and i.credit - 1 != h.src for i, h in c.ih))
edge("state:equal_best_scores_keep_the_earlier_target")(lambda c: any(i.credit and any(h.masked and h.score == i.hits[i.credit - 1].score and h.t > i.credit - 1 for h in i.hits) for i in c.info))


# ---- mask and range ---------------------------------------------------------------------------------------------------------------------
def _ranges(i):
    return [(h.start, h.stop) for h in i.hits if h.masked and not h.stale]


def _two(i, pred):
    r = _ranges(i)
    return i.credit and any(pred(a, b) for x, a in enumerate(r) for b in r[x + 1:])


def _runs(i):
    """[(start, length)] of the unmasked runs"""
    out, at = [], None
    for k, ok in enumerate(i.mask + [False]):
        if ok and at is None:
            at = k
        if not ok and at is not None:
            out.append((at, k - at))
            at = None
    return out


edge("mask:two_disjoint_ranges")(lambda c: any(_two(i, lambda a, b: a[1] + 1 < b[0] or b[1] + 1 < a[0]) for i in c.info))
edge("mask:two_overlapping_ranges")(lambda c: any(_two(i, lambda a, b: a[0] < b[0] <= a[1] < b[1] or b[0] < a[0] <= b[1] < a[1]) for i in c.info))
edge("mask:nested_ranges")(lambda c: any(_two(i, lambda a, b: (a[0] < b[0] and b[1] < a[1]) or (b[0] < a[0] and a[1] < b[1])) for i in c.info))
edge("mask:the_whole_read")(lambda c: any(i.credit and i.second == 0 and i.qlen > 8 for i in c.info))
edge("mask:a_run_that_is_no_record_is_not_reset")(lambda c: any(i.credit and (i.first, i.second) != find_mask_range(i.mask, "find_mask_range_resets_at_every_masked_base") and
                                                                i.second > max(n for _, n in _runs(i)) for i in c.info))
edge("mask:two_runs_of_equal_length_the_first_wins")(lambda c: any(i.credit and len(_runs(i)) == 2 and _runs(i)[0][1] == _runs(i)[1][1] == i.second and i.first == _runs(i)[0][0] for i in c.info))
for _p in (64, 128):
    edge("mask:changes_at_%d_%d" % (_p - 1, _p))(lambda c, p=_p: any(i.credit and i.qlen > p and not i.mask[p - 1] and i.mask[p] for i in c.info) and
                                                 any(i.credit and i.qlen > p and i.mask[p - 1] and not i.mask[p] for i in c.info))
edge("mask:read_ends_inside_an_unmasked_run")(lambda c: any(i.credit and i.mask[-1] and i.first + i.second == i.qlen and i.first > 0 for i in c.info))
edge("mask:adapter_stats_bases_are_qlen_minus_second")(lambda c: sum(i.qlen - i.second for i in c.info if i.credit) == int(c.stats[1::2].sum()) > 0 and
                                                        int(c.stats[0::2].sum()) == sum(1 for i in c.info if i.credit))


# ---- groups -----------------------------------------------------------------------------------------------------------------------------
def _groups(c):
    return partition(c.tlens) or [(0, len(c.tlens), max(c.tlens), 4 * sum(map(plane_words, c.tlens)))]


def _group_of(c, t):
    return next(k for k, g in enumerate(_groups(c)) if g[0] <= t < g[0] + g[1])


def _masking_groups(c, i):
    return {_group_of(c, h.t) for h in i.hits if h.masked}


def _reaches_stage2(c, i, g):
    """the group's launch goes to stage 2 for the read: a target without a matching cell, or one whose diagonals may reach its threshold"""
    j0, n = _groups(c)[g][:2]
    return any(not h.any or int(h.counts.max()) >= _need_cnt(i, h) for h in i.hits[j0:j0 + n])


edge("groups:closed_by_64_targets")(lambda c: any(g[1] == GROUP for g in _groups(c)) and any(i.credit > GROUP for i in c.info))
edge("groups:closed_by_the_plane_capacity")(lambda c: any(g[1] < GROUP and k + 1 < len(_groups(c)) for k, g in enumerate(_groups(c))) and
                                            any(i.credit and _group_of(c, i.credit - 1) > 0 and _groups(c)[_group_of(c, i.credit - 1) - 1][1] < GROUP for i in c.info))
edge("groups:32767_bases_alone_against_64_bases")(lambda c: any(h.tlen == 32767 and i.qlen == 64 and h.credited and _groups(c)[_group_of(c, h.t)][1] == 1 for i, h in c.ih))
edge("groups:diagonals_above_64_BB_CAP")(lambda c: any(c.grouped and h.credited and 64 * BB_CAP < h.ndiag <= 64 * BB_CAP + 2 and i.qlen <= 320 for i, h in c.ih))
edge("groups:diagonals_at_64_BB_CAP")(lambda c: any(c.grouped and h.credited and h.ndiag == 64 * BB_CAP and i.qlen <= 320 for i, h in c.ih))
edge("groups:masked_in_the_first_group_only_and_the_last_skips_stage_2")(lambda c: len(_groups(c)) >= 2 and any(
    i.credit and _masking_groups(c, i) == {0} and not _reaches_stage2(c, i, len(_groups(c)) - 1) and i.qlen > 64 for i in c.info))
edge("groups:masked_in_the_last_group_only")(lambda c: len(_groups(c)) >= 2 and any(i.credit and _masking_groups(c, i) == {len(_groups(c)) - 1} for i in c.info))
edge("groups:masked_in_two_groups")(lambda c: any(i.credit and len(_masking_groups(c, i)) >= 2 and i.qlen > 64 and len(_ranges(i)) >= 2 for i in c.info))
edge("groups:stale_range_from_an_earlier_groups_target")(lambda c: c.grouped and any(h.stale and h.masked and _group_of(c, h.src) < _group_of(c, h.t) and not i.hits[h.src].masked and
                                                                                     int(i.hits[h.src].counts.max()) < _need_cnt(i, i.hits[h.src]) and i.credit for i, h in c.ih))
edge("groups:mask_of_more_than_one_word")(lambda c: c.grouped and any(i.credit and i.qlen > 128 and len(_masking_groups(c, i)) >= 2 and not i.mask[i.qlen - 2] for i in c.info))
edge("groups:long_read")(lambda c: c.grouped and any(i.credit and i.qlen > 1024 and len(_masking_groups(c, i)) >= 2 for i in c.info))


# ---- pair kernel ------------------------------------------------------------------------------------------------------------------------
def _pairs(c):
    """[(A, B or None)] of the submissions that take the pair kernel"""
    out = []
    for k, ls in enumerate(c.kern):
        if ls[0][0] == "pair":
            r = c.by_sub(k)
            out += [(r[x], r[x + 1] if x + 1 < len(r) else None) for x in range(0, len(r), 2)]
    return out


def _stage2(i):
    return any(int(h.counts.max() if len(h.counts) else 0) >= _need_cnt(i, h) for h in i.hits) or any(not h.any for h in i.hits)


edge("pair:odd_number_of_reads")(lambda c: any(b is None and a.credit for a, b in _pairs(c)))
edge("pair:one_of_a_pair_empty")(lambda c: {(a.qlen == 0, b.qlen == 0) for a, b in _pairs(c) if b and (a.credit or b.credit)} >= {(True, False), (False, True)})
edge("pair:one_of_a_pair_rejected")(lambda c: {(a.bad, b.bad) for a, b in _pairs(c) if b and (a.credit or b.credit)} >= {(True, False), (False, True)})
edge("pair:1_and_160_bases")(lambda c: {(a.qlen, b.qlen) for a, b in _pairs(c) if b and (a.credit and b.credit)} >= {(1, 160), (160, 1)})
edge("pair:only_A_only_B_and_both_go_on")(lambda c: {(a.credit > 0, b.credit > 0) for a, b in _pairs(c) if b and set(a.seq + b.seq) != set(b"T") and
                                                    (a.credit or set(a.seq) == set(b"T")) and (b.credit or set(b.seq) == set(b"T"))} >= {(True, False), (False, True), (True, True)})
edge("pair:in_two_groups_of_8")(lambda c: any(b and a.seg == b.seg and a.at // 8 != b.at // 8 and a.credit and b.credit and a.len8 != b.len8 for a, b in _pairs(c)))
edge("pair:in_two_segments")(lambda c: any(b and a.seg != b.seg and a.credit and b.credit for a, b in _pairs(c)))

# ---- rejected bases ---------------------------------------------------------------------------------------------------------------------
REJECTED = (b"X", b"U", b"7", b"\0", b"\x80", b"\xff")
for _b in REJECTED:
    edge("rejected:%r_first_and_last" % _b)(lambda c, b=_b: c.error == E_BASE and any(i.bad and i.seq[:1] == b and i.seq.count(b) == 1 and i.qlen > 1 for i in c.info) and
                                            any(i.bad and i.seq[-1:] == b and i.seq.count(b) == 1 and i.qlen > 1 for i in c.info))
edge("rejected:the_neighbours_are_not_flagged")(lambda c: c.error == E_BASE and any(i.bad and 0 < i.index < len(c.info) - 1 and i.sub == c.info[i.index + 1].sub == c.info[i.index - 1].sub and
                                                                                    c.info[i.index - 1].credit and c.info[i.index + 1].credit and
                                                                                    i.seq[:1] in REJECTED and i.seq[-1:] in REJECTED for i in c.info))
edge("rejected:alone_in_its_read")(lambda c: c.error == E_BASE and any(i.bad and i.qlen == 1 for i in c.info))


# =====================================================================================================================================
# the cases
# =====================================================================================================================================
X40, Z30, W20, Y300, U60 = tg(40, 1), tg(30, 2), tg(20, 3), tg(300, 4), tg(60, 5)
SHORT3 = [("x40", X40), ("z30", Z30), ("w20", W20)]


def hit_read(n, target, at=None):
    """n bases with the whole target at `at` (default: the middle)"""
    at = (n - len(target)) // 2 if at is None else at
    return rd(n, (at, target))


def dispatch_cases():
    C = []
    subs = [one([rd(L, (L - 45, X40)), rd(60, (5, Z30)), rd(60), rd(50, (20, W20))]) [0] for L in (160, 161, 256, 257, 320, 321, 1024)]
    C.append(ACase("dispatch_by_the_longest_read", SHORT3, [], subs, ["dispatch:longest_read_%d_takes_%s" % p for p in ((160, "pair"), (161, "256"), (256, "256"), (257, "320"),
                                                                                                                        (320, "320"), (321, "1024"), (1024, "1024"))]))
    subs = [one([rd(60, (5, Z30)), rd(L, (L - 45, X40), (10, W20)), rd(50)])[0] for L in (1025, 4096, 4097, 8193, 16385)]
    C.append(ACase("dispatch_by_the_longest_read_long", SHORT3, [], subs, ["dispatch:longest_read_1025_takes_4096", "dispatch:longest_read_4096_takes_4096", "dispatch:longest_read_4097_takes_8192"] +
                   ["dispatch:long_width_%d_with_a_hit" % w for w in (8192, 16384, 32768)]))
    for n in (32, 33):
        lib = [("t%d" % k, tg(24 + k % 5, 100 + k)) for k in range(n)]
        reads = [hit_read(150 - k, lib[k][1], 10 + 2 * k) for k in (0, 7, 31, n - 1)] + [rd(150)]
        C.append(ACase("pair_gate_%d_targets" % n, lib, [], one(reads), ["dispatch:32_targets_take_pair" if n == 32 else "dispatch:33_targets_take_256"]))
    for n in (128, 129):
        lib = [("x40", X40), ("long", tg(n, 7))]
        reads = [hit_read(160, lib[1][1], 3), hit_read(150, X40), rd(140), hit_read(150, lib[1][1][:n - 9], 0), hit_read(150, lib[1][1][9:], 150 - n + 9)]
        C.append(ACase("pair_gate_target_of_%d" % n, lib, [], one(reads), ["dispatch:longest_target_128_takes_pair", "target:128_bases_credited"] if n == 128 else
                       ["dispatch:longest_target_129_takes_256", "dispatch:stage1_width_6_by_a_long_target", "target:129_bases_credited"]))
    for n in (64, 65):
        lib = [("t%d" % k, tg(20 + k % 7, 200 + k)) for k in range(n)]
        reads = [hit_read(150, lib[k][1], 100) for k in (0, 63, n - 1)] + [rd(150), hit_read(300, lib[n - 1][1], 250)]
        C.append(ACase("group_gate_%d_targets" % n, lib, [], one(reads), ["dispatch:64_targets_in_one_pass"] if n == 64 else ["dispatch:65_targets_are_grouped", "groups:closed_by_64_targets",
                                                                                                              "groups:masked_in_the_first_group_only_and_the_last_skips_stage_2"]))
    for n in (8192, 8193):
        lib = [("x40", X40), ("long", tg(n, 9))]
        t = lib[1][1]
        reads = [rd(300, (20, t[4000:4260])), rd(150, (0, t[n - 130:])), rd(150, (30, X40)), rd(150), rd(64, (0, t[:60])), rd(150), rd(150), rd(64)]   # (a full group of 8: the threshold comes from its last read)
        C.append(ACase("group_gate_target_of_%d" % n, lib, [], one(reads), ["dispatch:longest_target_8192_in_one_pass"] if n == 8192 else ["dispatch:longest_target_8193_is_grouped"]))
    # stage-1 width: 4 while |read| + the longest short target - 1 <= 256 and no target is longer than 128 bases, else 6; 7 in the 320 variant.  The
    # straight-line count of a class runs over NB_LO blocks when the pair's diagonals fit them, else over all
    lib = [("t33", tg(33, 11)), ("t97", tg(97, 12))]
    reads = [hit_read(160, lib[1][1], 60), hit_read(160, lib[0][1], 100), hit_read(161, lib[1][1], 60), hit_read(200, lib[0][1], 150), hit_read(200, lib[1][1], 90), rd(161)]
    C.append(ACase("stage1_width_4_and_6", lib, [], one(reads), ["dispatch:stage1_width_4_at_256_diagonals", "dispatch:stage1_width_6_at_257_diagonals", "dispatch:stage1_width_4_blocks_at_3_and_4",
                                                                 "dispatch:stage1_width_6_blocks_at_4_and_5"]))
    reads = [hit_read(288, lib[0][1], 200), hit_read(288, lib[1][1], 100), rd(288)]
    C.append(ACase("stage1_width_7", lib, [], one(reads), ["dispatch:stage1_width_7_blocks_at_5_and_6"]))
    return C


def _big5(n):
    return [("big%d" % k, tg(n, 300 + k)) for k in range(5)]


def uncached_cases():
    """five targets of 7 000 bases: 5 * 219 plane words = 4 380 dwords, past the LDS copy of a single-pass set; cut to 6 500 bases (4 080 dwords) they fit"""
    C = []
    for n, rate in ((7000, "0.2"), (6500, "0.2"), (7000, "0.6"), (6500, "0.6")):
        lib = _big5(n)
        t0, t3, t4 = lib[0][1], lib[3][1], lib[4][1]
        name, f = ("uncached", "uncached") if n == 7000 else ("cut_to_the_cap", "sliding")
        if rate == "0.2":
            short = [rd(250, (20, t0[3000:3200])), rd(250, (25, t3[100:299])), rd(250, (0, t4[n - 210:])), rd(250, (40, t0[:210])), rd(250), rd(250, (10, t3[6000:6100])),
                     rd(250, (3, t4[500:700]), (210, t0[0:40])), rd(250, (30, t3[2000:2200]))]
            wide = [rd(300, (20, t0[3000:3250])), rd(300, (25, t3[100:339])), rd(300, (0, t4[n - 260:])), rd(300), rd(300, (1, t0[4000:4240])), rd(290, (0, t3[:239])), rd(300), rd(300)]
            claims = ["filters:%s:num_match=thr" % f, "filters:%s:num_match=thr-1" % f] + (["dispatch:uncached_single_pass_256", "dispatch:uncached_single_pass_320"] if n == 7000 else
                                                                                          ["dispatch:the_same_library_cut_to_the_cap_256", "dispatch:the_same_library_cut_to_the_cap_320"])
            subs = [[short], [wide]]
        else:
            subs = [[[rd(250, (0, scatter(t0[3000:3250]))), rd(250, (0, t3[10:110])), rd(250), rd(250, (0, scatter(t4[200:450]))), rd(250, (0, t3[10:109])), rd(250), rd(250), rd(250)]]]
            claims = ["filters:%s:count_reaches_need_cnt_and_no_alignment_reaches_thr" % f]
        C.append(ACase("%s_rate_%s" % (name, rate), lib, ["--rate", rate] if rate != "0.2" else [], subs, claims))
    return C


CLASS_ORDER = (129, 97, 1, 64, 33, 128, 31, 96, 65, 32, 127, 63, 95)


def target_cases():
    C = []
    lib = [("t%d" % n, tg(n, 400 + n)) for n in CLASS_ORDER]
    reads = [hit_read(200, t, 30 + k) for k, (_, t) in enumerate(lib) if len(t) > 1] + [rd(200, (100, lib[2][1])), rd(200)]
    C.append(ACase("every_class_with_a_long_target", lib, [], one(reads), ["target:every_class_in_one_library_out_of_class_order", "target:no_base_plane_shared_with_the_read"] +
                   ["target:%d_bases_credited" % n for n in CLASS_ORDER if n != 128]))
    lib12 = [a for a in lib if len(a[1]) <= 128]
    reads = [hit_read(150, t, k) for k, (_, t) in enumerate(lib12) if len(t) > 1] + [rd(150, (100, lib[2][1])), rd(150)]
    C.append(ACase("every_class_in_the_pair_kernel", lib12, [], one(reads), ["target:%d_bases_credited" % n for n in (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127)]))
    codes = "ARCYGSAWCKGMABCDGHAVCNGA"
    lib = [("iupac", codes + tg(16, 21)), ("lower", tg(36, 22).lower()), ("with_n", tg(12, 23) + "NNNN" + tg(12, 24)), ("with_gap", tg(14, 25) + "-" + tg(14, 26) + "--" + tg(9, 27))]
    res = codes.translate(str.maketrans("RYSWKMBDHVN", "AGCAGACAAAT".replace("G", "C", 1))) + lib[0][1][len(codes):]
    reads = [rd(150, (40, res)), rd(150, (5, lib[1][1].upper())), rd(150, (60, lib[2][1].replace("NNNN", "TTTT"))), rd(150, (20, lib[3][1].replace("-", "T"))),
             rd(150, (20, lib[3][1].replace("-", "A"))), rd(150, (80, lib[1][1])), rd(150)]
    C.append(ACase("target_codes", lib, [], one(reads), ["target:gap_matches_no_base"]))
    # (a library with a '-' runs without the filters: the codes once more without it, through stage 1 and the pair kernel)
    C.append(ACase("target_codes_without_the_gap", lib[:3], [], one(reads[:3] + reads[5:]), ["target:iupac_codes", "target:lower_case", "target:N_matches_every_base"]))
    return C


def read_cases():
    C = []
    lib = [("u60", U60), ("z30", Z30), ("one", "G")]
    # every length with a hit and without one; the 1-base target's threshold is 0, so a 'G' anywhere is a hit: the reads without one hold no G
    reads = []
    for n in READ_LENGTHS:
        reads += [rd(n, (max(n - 60, 0), U60[:n][-60:])) if n else b"", rd(n)]
    reads += [b"-" * 40, rd(100, (20, U60[:10] + "NNNN" + U60[14:40] + "N" + U60[41:])), rd(100, (3, b"-" * 9))]
    C.append(ACase("read_lengths", lib, [], [[reads], [list(reversed(reads))]], ["read:%d_bases" % n for n in READ_LENGTHS] + ["read:only_gaps", "read:N_matches_every_target_base"]))
    # what a longer read leaves in the plane words behind a shorter one: the read two (pair kernel) or one place before holds, past the short read's end, what
    # would lengthen the short read's alignment
    long_a, short_a = rd(150, (64, U60[30:])), rd(64, (34, U60[:30]))
    reads = [long_a, long_a, short_a, short_a, rd(150), rd(150, (80, Z30))]
    C.append(ACase("leftover_plane_words_pair", lib[:2], ["--rate", "0.6"], one(reads), ["read:short_behind_long_in_either_half_of_the_pair_kernel"]))
    reads = [long_a, short_a, rd(161), rd(200, (128, U60[30:])), rd(128, (98, U60[:30])), rd(256, (192, U60[30:])), rd(192, (162, U60[:30]))]
    C.append(ACase("leftover_plane_words", lib[:2], ["--rate", "0.6"], one(reads), ["read:short_behind_long_in_one_wave_slot"]))
    lib = [("gapped", tg(15, 31) + "-" + tg(15, 32) + "-" + tg(8, 33)), ("z30", Z30)]
    # (the first 32 bases of the target, both gaps among them: 32 matches are the threshold, 30 without the gaps are not)
    reads = [rd(150, (30, lib[0][1])), rd(150, (60, lib[0][1][:32])), rd(150, (30, lib[0][1].replace("-", "T"))), rd(150, (100, Z30), (2, lib[0][1][10:25])), rd(150)]
    C.append(ACase("gap_against_gap", lib, [], one(reads), ["read:a_gap_against_a_gap_in_the_target"]))
    return C


T100 = tg(100, 41)


def aligner_cases():
    C = []
    # runs: 20 A, 25 G, 20 C.  A read with 20 A and, 22 bases on, 20 C meets it on two diagonals 23 apart with 20 matches each and none besides (either piece
    # faces the G of the other's diagonal): both blocks' bounds equal the best score, the lower block is visited first and the upper one holds the later cell
    runs = "A" * 20 + "G" * 25 + "C" * 20
    lib = [("t100", T100), ("y300", Y300), ("rep", tg(30, 42) + tg(8, 43) + tg(30, 42)), ("runs", runs), ("runs5", "".join(ch * 5 for ch in runs))]
    A = ["--rate", "0.9"]     # thr = 10, 30, 6, 6 and 30: a piece of 25 (40) bases masks
    rep = lib[2][1]

    def two(n, d1, d2, k=25, a1=0, a2=40, t=T100):
        """pieces t[a1 : a1 + k] and t[a2 : a2 + k] on the diagonals d1 and d2 of a read of n bases: d = a - p + n - 1"""
        return rd(n, (a1 + n - 1 - d1, t[a1:a1 + k]), (a2 + n - 1 - d2, t[a2:a2 + k]))
    reads = [two(200, 70, 90, a2=60), two(200, 63, 64, a2=30), two(200, 63, 64, a1=29, a2=1), two(200, 30, 270, a2=75), two(200, 270, 30, a1=75, a2=0),
             two(300, 100, 420, k=40, a2=230, t=Y300), two(300, 420, 100, k=40, a1=230, a2=0, t=Y300), two(300, 63, 64, k=30, a1=31, a2=0, t=Y300),
             rd(200, (50, rep[:30])), rd(200, (0, T100[:30])), rd(200, (170, T100[70:])), rd(200, (0, T100[60:])), rd(200, (165, T100[:35])),
             rd(93, (0, T100[70:])), rd(93, (60, T100[:33])), rd(94, (0, T100[70:])), rd(200, (20, spoil(T100[10:12], 2, 1).decode() + T100[12:50])),
             rd(200, (128, T100[20:50])), rd(200), rd(200, (149, "A" * 20), (171, "C" * 20)), rd(300, (45, "A" * 100), (155, "C" * 100))]
    claims = ["aligner:tie_on_two_diagonals_of_one_block", "aligner:tie_on_diagonals_63_and_64", "aligner:tie_in_blocks_far_apart", "aligner:tie_in_a_long_target",
              "aligner:the_block_visited_first_does_not_win_the_tie", "aligner:a_block_whose_bound_equals_the_best_score_wins", "aligner:last_row_major_cell_larger_i",
              "aligner:last_row_major_cell_larger_j_in_one_row", "aligner:winner_on_lane_0", "aligner:winner_on_lane_63", "aligner:diagonals_64k", "aligner:diagonals_64k+1",
              "aligner:alignment_from_i=0_j=0", "aligner:alignment_to_the_last_base_of_both", "aligner:target_hangs_off_the_reads_start", "aligner:target_hangs_off_the_reads_end",
              "aligner:score_touches_0_and_the_start_survives", "aligner:best_score_in_the_last_partial_plane_word"]
    C.append(ACase("ties_and_ends", lib, A, one(reads), claims))
    C.append(ACase("ties_and_ends_short_targets", [lib[0], lib[2]], A, one([r for r in reads if len(r) <= 160 or r.count(b"T") > 0][:5] + [r[40:] for r in reads[8:13]] + [reads[13], reads[14]]), []))
    return C


def filter_cases():
    C = []
    lib = [("x40", X40), ("w20", W20), ("y300", Y300), ("polyA", "A" * 20)]
    reads = [rd(250, (100, X40[:32])), rd(250, (100, X40[:31])), rd(250, (0, X40[8:])), rd(250, (30, "A" * 16)), rd(250, (30, "A" * 15)), rd(250, (25, Y300[50:250])),
             rd(250, (25, Y300[50:249])), rd(250, (200, W20[:16])), rd(250, (200, W20[:15])), rd(250)] + [rd(250)] * 6
    C.append(ACase("filters_default_rate", lib, ["--polyA"], one(reads), ["filters:blocked:num_match=thr", "filters:blocked:num_match=thr-1", "filters:sliding:num_match=thr",
                                                                        "filters:sliding:num_match=thr-1", "filters:polyA_16_of_20"]))
    reads = [rd(250, (100, scatter(X40))), rd(250, (0, scatter(Y300[20:270]))), rd(250, (0, X40[24:])), rd(250, (0, X40[25:])), rd(250, (60, X40[:16])), rd(250), rd(250), rd(250)]
    C.append(ACase("filters_rate_0.6", lib[:3], ["--rate", "0.6"], one(reads), ["filters:blocked:count_reaches_need_cnt_and_no_alignment_reaches_thr",
                                                                                "filters:sliding:count_reaches_need_cnt_and_no_alignment_reaches_thr", "filters:two_word_target_met_behind_its_first_word"]))
    reads = [rd(150, (100, X40[:32])), rd(150, (100, X40[:31])), rd(150, (0, X40[8:])), rd(150, (30, "A" * 16)), rd(150, (30, "A" * 15)), rd(150, (100, scatter(X40))), rd(150), rd(150)]
    C.append(ACase("filters_pair_kernel", [lib[0], lib[1], lib[3]], ["--polyA"], one(reads), []))
    return C


def threshold_cases():
    C = []
    lib = [("x40", X40), ("w20", W20)]
    part = rd(60, (10, X40[:24]))                  # 24 of 40: masks under a threshold taken from a read of 25 (20), not under the target's own (32)
    short = rd(30, (0, X40[:26]))                  # 26 of 40 in a read of 30: masks under its own length (24), not under the last read's of 60 (32)
    full = rd(60, (15, X40))
    g_short = [part, full, rd(60), part, rd(60), part, full, rd(25)]
    g_long = [short, full, rd(60), short, rd(60), rd(60), full, rd(60)]
    g_empty = [rd(60, (30, "A")), full, rd(60, (5, X40[:3]), (40, W20)), rd(60), part, rd(60, (0, W20[:2])), rd(60, (20, X40[:12])), b""]
    tail = [short, part, full]
    C.append(ACase("last_of_8", lib, [], [[g_short + g_long + g_empty + tail]], ["thr:last_of_8_shorter_than_the_target", "thr:last_of_8_longer_than_the_target", "thr:last_of_8_empty",
                                                                                "thr:tail_group_takes_no_min"]))
    # a first segment of 60 reads: the second segment's first group of 8 is reads 60 ... 67, across the 64-read chunk of a wave
    seg0 = ([full, rd(60), part] * 20)[:60]
    seg1 = [part, full, part, part, rd(60), part, full, rd(25), part, full, rd(60)]
    C.append(ACase("segments", lib, [], [[seg0, seg1, [full, part, full]], [[part, full], [], [], [full, part, rd(60), full], []]], ["thr:group_of_8_across_a_64_read_chunk", "thr:segments_that_are_no_multiple_of_8",
                                                                                                                                   "thr:empty_segment"]))
    lib = [("t%d" % n, tg(n, 500 + n)) for n in (5, 10, 20, 40)]
    reads = []
    for (_, t), n in zip(lib, (5, 10, 20, 40)):
        v = FLOAT_THR[n][0]
        reads += [rd(70, (20, t[:v])), rd(70, (20, t[:v - 1])) if v > 1 else rd(70)]
    C.append(ACase("rate_0.6", lib, ["--rate", "0.6"], one(reads + [rd(70)] * 8), ["thr:rate_0.6_against_%d_bases_is_%d" % (n, v[0]) for n, v in FLOAT_THR.items()]))
    t180 = tg(180, 51)
    C.append(ACase("rate_0.35", [("t180", t180), ("w20", W20)], ["--rate", "0.35"], one([rd(200, (10, t180[30:146])), rd(200, (10, t180[30:145])), rd(200, (50, W20)), rd(200)] + [rd(200)] * 4),
                   ["thr:rate_0.35_against_180_bases_is_116"]))
    return C


def state_cases():
    """targets over A / G and reads of A / G / T: a target of C alone has no matching cell and reports the range the aligner still holds (H2)"""
    C = []
    xa, za = tg(40, 61, "AG"), tg(30, 62, "AG")
    lib = [("c1", "C"), ("xa", xa), ("c12", "C" * 12), ("za", za), ("za_again", za), ("c12_again", "C" * 12)]
    reads = [rd(150, (10, xa), (100, za)),            # c12 behind a target that aligned and masked: the same range once more
             rd(150, (10, xa[:20]), (100, za)),       # xa matches somewhere and cannot pass: c12 masks xa's range (20 bases, 10 >= 9) without credit, za credits
             rd(150, (0, za)),                        # c1 in front of every state: threshold 0 and nothing to judge
             rd(150, (60, xa[:20])), rd(150, (100, za)),   # (a window from base 0: a range invented for c1 would cut it)
             rd(150, (5, za), (60, xa[:20])), rd(150, (10, xa)), rd(150, (1, za[:28]))]
    C.append(ACase("stale_range", lib, [], one(reads), ["state:stale_range_after_a_target_that_aligned", "state:stale_range_after_a_target_that_could_not_pass", "state:no_range_before_any_target",
                                                        "state:score_0_masks_without_credit", "state:equal_best_scores_keep_the_earlier_target"]))
    C.append(ACase("stale_range_wide", lib, [], one([r + b"T" * 50 for r in reads]), []))
    return C


def mask_cases():
    C = []
    zo = X40[30:] + tg(20, 71)                        # begins with X40's last 10 bases: behind X40 its range overlaps X40's
    lib = [("x40", X40), ("z30", Z30), ("w20", W20), ("inner", X40[10:30]), ("zo", zo)]
    reads = [rd(200, (10, X40), (100, Z30)), rd(200, (10, X40 + zo[10:])), X40.encode(), rd(70, (10, W20), (40, Z30)), rd(150, (10, W20), (40, Z30), (80, W20)),
             rd(150, (34, Z30), (74, W20)), rd(200, (34, Z30)), rd(200, (64, Z30)), rd(200, (98, Z30)), rd(200, (128, Z30)), rd(200, (150, Z30)), rd(200)]
    C.append(ACase("ranges_and_runs", lib, [], one(reads), ["mask:two_disjoint_ranges", "mask:two_overlapping_ranges", "mask:nested_ranges", "mask:the_whole_read", "mask:a_run_that_is_no_record_is_not_reset",
                                                            "mask:two_runs_of_equal_length_the_first_wins", "mask:changes_at_63_64", "mask:changes_at_127_128", "mask:read_ends_inside_an_unmasked_run",
                                                            "mask:adapter_stats_bases_are_qlen_minus_second"]))
    C.append(ACase("ranges_and_runs_pair_kernel", lib, [], one([r[:160] for r in reads]), []))
    return C


def group_cases():
    C = []
    ag = [("g%d" % k, tg(30, 600 + k, "AG")) for k in range(130)]
    lib = ag[:64] + [("c12", "C" * 12)] + ag[64:127] + ag[127:130]
    t = lambda k: lib[k][1]
    reads = [rd(150, (20, t(3))),                                  # the first group only; the last group's targets all match somewhere and none can pass
             rd(150, (100, t(129))), rd(150, (5, t(10)), (118, t(100))), rd(150, (5, t(10)), (60, t(100)), (119, t(130))),
             rd(150, (40, t(63)[:14]), (100, t(70))),              # target 63 cannot pass; c12, first of the next group, masks its range: aligned from global memory
             rd(150), rd(150, (0, t(64 + 64))), rd(64, (30, t(130)))]
    claims = ["groups:masked_in_the_last_group_only", "groups:masked_in_two_groups", "groups:stale_range_from_an_earlier_groups_target",
              "groups:mask_of_more_than_one_word"]
    C.append(ACase("three_groups", lib, [], one(reads), claims))
    C.append(ACase("three_groups_long_read", lib, [], one([rd(1100, (5, t(10)), (1060, t(100))), rd(150, (20, t(3))), rd(300, (5, t(10)), (260, t(100)))]), ["groups:long_read"]))
    # by capacity: 8 193 + 8 642 + 8 641 bases are 3 196 plane dwords, the 32 767 bases behind them 4 096 of their own
    b1, hi, lo, top = tg(8193, 81), tg(64 * BB_CAP + 2 - 64, 82), tg(64 * BB_CAP + 1 - 64, 83), tg(32767, 84)
    lib = [("b8193", b1), ("above", hi), ("at", lo), ("top", top), ("x40", X40)]
    reads = [rd(64, (0, top[20000:20060])), rd(64, (2, hi[8000:8060])), rd(64, (2, lo[8000:8060])), rd(64, (0, lo[len(lo) - 60:])), rd(64, (4, hi[len(hi) - 60:])),
             rd(150, (0, b1[100:220]), (125, hi[:25])), rd(150, (20, X40), (70, top[32700:])), rd(64)]
    C.append(ACase("groups_by_capacity", lib, [], one(reads), ["groups:closed_by_the_plane_capacity", "groups:32767_bases_alone_against_64_bases", "groups:diagonals_above_64_BB_CAP",
                                                               "groups:diagonals_at_64_BB_CAP"]))
    return C


def pair_cases():
    C = []
    lib = SHORT3
    hx, hz, hw, no = rd(150, (20, X40)), rd(150, (100, Z30)), rd(150, (60, W20)), rd(150)
    one_b = rd(1, (0, X40[:1]))
    # thr of a group whose last read has one base is 0: the 1-base read (tail group or such a group) masks with any match
    # the second group of 8 ends with a read of one base: its threshold is 0 and a read of one base masks; 17 reads: the pair (16, 17) lies in two segments
    seg0 = [hx, b"", b"", hz, hx, no, no, hw, hx, hz, rd(160, (120, X40)), one_b, one_b, rd(160, (0, Z30)), hw, one_b, hx]
    seg1 = [hz, no, no, no, hx, hw, hz, rd(100, (0, X40)), hx, hw]      # starts at read 17: its groups of 8 begin at odd reads; 27 reads in all
    C.append(ACase("pairs", lib, [], [[seg0, seg1]], ["pair:odd_number_of_reads", "pair:one_of_a_pair_empty", "pair:1_and_160_bases", "pair:only_A_only_B_and_both_go_on", "pair:in_two_groups_of_8",
                                                      "pair:in_two_segments"]))
    return C


def rejected_cases():
    C = []
    hx, hz = rd(150, (20, X40)), rd(150, (100, Z30))
    for kernel, wide in (("pair", []), ("256", [rd(200, (30, X40))])):
        reads = list(wide)
        for b in REJECTED:
            reads += [hx, b + hx[1:], hz, hz[:-1] + b, hx, b + hz[1:-1] + b, hz]
        reads += [hx, b"X", hz]
        C.append(ACase("rejected_bytes_%s" % kernel, SHORT3, [], one(reads), (["rejected:%r_first_and_last" % b for b in REJECTED] + ["rejected:the_neighbours_are_not_flagged", "rejected:alone_in_its_read"]
                                                                             if kernel == "256" else ["pair:one_of_a_pair_rejected"])))
    return C


FAMILIES = ("dispatch", "uncached", "targets", "reads", "aligner", "filters", "threshold", "state", "mask", "groups", "pair", "rejected")
_BUILDERS = dict(dispatch=dispatch_cases, uncached=uncached_cases, targets=target_cases, reads=read_cases, aligner=aligner_cases, filters=filter_cases, threshold=threshold_cases,
                 state=state_cases, mask=mask_cases, groups=group_cases, pair=pair_cases, rejected=rejected_cases)
_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        C = []
        for fam in FAMILIES:
            cs = _BUILDERS[fam]()
            for c in cs:
                c.family = fam
                if not c.takes_pair():
                    c.exclude["no_pair"] = "no submission of the case takes the pair kernel"
            C += cs
        _CASES = C
    return _CASES


def cases_of(family, setting, cases=None):
    return [c for c in (all_cases() if cases is None else cases) if c.family == family and setting not in c.exclude]


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
                except (IndexError, KeyError, TypeError, ValueError, StopIteration):
                    pass
    return table, lost, more


if __name__ == "__main__":
    t, lost, more = coverage()
    print("claimed  unclaimed  edge")
    for e, v in t.items():
        print("%7d  %9d  %s" % (len(v), len(more[e]), e))
    print("%d cases, %d reads, %d edges; claims that do not hold: %s" % (len(all_cases()), sum(c.n_reads() for c in all_cases()), len(t), lost))
