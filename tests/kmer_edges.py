"""A constructed catalogue of inputs for the k-mer rarefaction stage (faqcs_kmer_skm_kernel.hip, faqcs_kmer_kernel.hip, faqcs_capi_kmer.hip,
faqcs_skm.h, faqcs_kmer.h), in the style of tests/pair_edges.py: the edges of the kept window and of k, of the byte classification, of the
lanes and pieces of the two extraction kernels, of the runs of equal minimizers, of the three storage classes of the histogram of counts,
of the sampling points and of the partitions.  Every case is a named builder of submissions of segments of reads, every edge a PREDICATE over
a case's inputs (and, for the sampling points, the model's trace); coverage() evaluates the predicates a case claims.

model(case) is the plain reference: canonical k-mers of the kept windows from a numpy rolling word, counted in a dict of Python ints, the
sampling-point rule segment by segment (trim.cpp:157-185, FaQCs.cpp:518-537).  It shares nothing with faqcs_skm.h or with oracle/: its base
codes are A C G T = 0 1 2 3, not the kernels'.  The kept window of a read that is trimmed comes from the oracle's results (the model does
not restate trimming).  skm_ord / min_ords / skm_part below restate the minimizer of faqcs_skm.h; they construct reads and state
predicates and never produce an expected count.  tests/test_kmer_edges_model.py holds the model to the oracle and the restatement to the
header without a GPU; tests/test_gpu_kmer_edges.py sends the catalogue to the device.

    python -m tests.kmer_edges        prints the number of cases per edge
"""
import numpy as np

IN_OFF = 33
MAX_READ = 1024
KS = (2, 3, 14, 15, 16, 17, 30, 31)
SKM_PIECE, SKM_ADVANCE, SKM_W_MAX = 256, 200, 17   # restated; test_kmer_edges_model.py compares them with faqcs_skm.h
DENSE_N = 1 << 16                                  # counts below it: the dense array (faqcs_capi_kmer.hip: d.dense_n)
LDS_SLOTS = 4096                                   # slots of the counting kernel's LDS table
LDS_ROUND_KEYS = 2816                              # keys of a partition the counting kernel's LDS table takes in one round
KG_EPOCH_SPAN = KG_MAX_RUNS = 1000
CONSTANT_SOURCES = {
    "SKM_PIECE": ("faqcs_skm.h", r"SKM_PIECE = (\d+)"), "SKM_ADVANCE": ("faqcs_skm.h", r"SKM_ADVANCE = (\d+)"), "SKM_W_MAX": ("faqcs_skm.h", r"SKM_W_MAX = (\d+)"),
    "DENSE_N": ("faqcs_capi_kmer.hip", r"d\.dense_n = 1u << (\d+)"), "KG_EPOCH_SPAN": ("faqcs_kmer.h", r"KG_EPOCH_SPAN = (\d+)"),
    "KG_MAX_RUNS": ("faqcs_kmer.h", r"KG_MAX_RUNS = (\d+)"),
}
GOOD = ord("I")

# =====================================================================================================================================
# the model
# =====================================================================================================================================
_STD = np.full(256, 4, np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _STD[_ch] = _STD[_ch | 32] = _i


def canonical_kmers(windows, k):
    """The canonical k-mers (uint64, A C G T = 0 1 2 3, first base in the highest bits) of every stretch of k bases `AaCcGgTt` in each window."""
    if not windows:
        return np.zeros(0, np.uint64)
    c = _STD[np.frombuffer(b"\xff".join(windows), np.uint8)]
    n = len(c)
    if n < k:
        return np.zeros(0, np.uint64)
    m = n - k + 1
    bad = np.concatenate([[0], np.cumsum(c > 3)])
    ok = bad[k:] == bad[:m]
    cc = (c & 3).astype(np.uint64)
    fwd, rc = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
    for t in range(k):
        fwd = (fwd << np.uint64(2)) | cc[t:t + m]
        rc |= (np.uint64(3) - cc[t:t + m]) << np.uint64(2 * t)
    return np.minimum(fwd, rc)[ok]


def effective(seq, qual, replace_q):
    """--replace_to_N_q: an upper-case G whose score (the byte as a signed char minus the offset, not below 0) is under the threshold reads as N"""
    if not replace_q or not seq:
        return seq
    s = np.frombuffer(seq, np.uint8).copy()
    score = np.maximum(np.frombuffer(qual, np.int8).astype(np.int64) - IN_OFF, 0)
    s[(s == ord("G")) & (score < replace_q)] = ord("N")
    return s.tobytes()


class Model:
    """One engine's k-mer state over any number of passes: TOTAL_NUMBER, the points and the histogram go on from pass to pass, the keys do not."""

    def __init__(self, opt):
        self.k, self.split, self.n_sub, self.qc, self.replace_q = opt.kmer, opt.split_size, opt.num_subsample, opt.qc_only, opt.replace_to_N_q
        self.keys, self.points, self.hist, self.total_number, self.active, self.trace = {}, [], {}, 0, True, []

    def windows(self, segment, results):
        """[(seq, qual, a, n, counted)] of a segment's reads; results: the oracle's per-read records (not looked at under --qc_only)"""
        out = []
        for i, (_, s, q) in enumerate(segment):
            if self.qc:
                out.append((s, q, 0, len(s), True))
            else:
                r = results[i]
                valid = bool(int(r["flags"]) & 1)
                out.append((s, q, int(r["start"]) if valid else 0, int(r["len"]) if valid else 0, valid))
        return out

    def totals(self):
        return len(self.keys), sum(self.keys.values())

    def submit(self, segments, results=None):
        at = 0
        for seg in segments:
            wins = self.windows(seg, None if results is None else results[at:at + len(seg)])
            at += len(seg)
            counted = 0
            if self.active:
                eff = [effective(s[a:a + n], q[a:a + n], 0 if self.qc else self.replace_q) for s, q, a, n, c in wins if c]
                u, cnt = np.unique(canonical_kmers(eff, self.k), return_counts=True)
                for key, c in zip(u.tolist(), cnt.tolist()):
                    self.keys[key] = self.keys.get(key, 0) + c
                counted = int(cnt.sum())
            self.total_number += len(seg)
            was_active, point = self.active, False
            if self.active:
                n_points = len(self.points)
                if self.total_number // self.split > n_points and n_points < self.n_sub:
                    self.points.append((self.total_number,) + self.totals())
                    point = True
                if n_points >= self.n_sub:
                    self.active = False
            self.trace.append(dict(n=len(seg), total=self.total_number, active=was_active, point=point, kmers=counted, wins=wins))

    def end_table(self):
        for c in self.keys.values():
            self.hist[c] = self.hist.get(c, 0) + 1
        if self.active and not self.points:
            self.points.append((self.total_number,) + self.totals())
        self.last_totals = self.totals()
        self.keys = {}

    def histogram(self):
        return sorted(self.hist.items())


def oracle_results(case):
    """The oracle's per-read records of a case's submissions on a fresh engine (the kept windows; None under --qc_only)"""
    if case.opt().qc_only:
        return [None] * len(case.subs)
    if case._res is None:
        from oracle_engine import OracleEngine

        from faqcs_amd import driver

        ora = OracleEngine(case.opt(), MAX_READ, IN_OFF)
        case._res = [ora.process(*driver.pack_segments(sub)) for sub in case.subs]
        ora.close()
    return case._res


def run_model(m, case, results=None):
    """One pass of `case` on the model engine m -> {after: [(points, totals, active)] per submission, points, totals, hist, active}"""
    results = results or oracle_results(case)
    after = []
    for sub, res in zip(case.subs, results):
        m.submit(sub, res)
        after.append((list(m.points), m.totals(), m.active))
    m.end_table()
    return dict(after=after, points=list(m.points), totals=m.last_totals, hist=m.histogram(), active=m.active)


def model(case):
    return run_model(Model(case.opt()), case)


# =====================================================================================================================================
# the minimizer of faqcs_skm.h, restated (construction and predicates only)
# =====================================================================================================================================
_SKM = np.full(256, 4, np.uint8)
for _i, _ch in enumerate(b"ACTG"):
    _SKM[_ch] = _SKM[_ch | 32] = _i


def skm_geom(k):
    m = min(k, 15)
    return m, k - m + 1


def skm_ord(x, m):
    x = np.asarray(x, np.uint64)
    mask = np.uint64((1 << (2 * m)) - 1)
    x = x ^ (x >> np.uint64(m))
    x = (x * np.uint64(0x9E3779B1)) & np.uint64(0xffffffff) & mask
    return x ^ (x >> np.uint64(m - 1))


def skm_part(o):
    return ((np.asarray(o, np.uint64) * np.uint64(0x85EBCA6B)) & np.uint64(0xffffffff)) >> np.uint64(13)


def min_ords(bases, k):
    """bases: bytes of ACGTacgt only -> the smallest ord among the canonical m-mers of each k-mer (one entry per k-mer start)"""
    m, w = skm_geom(k)
    c = _SKM[np.frombuffer(bases, np.uint8)].astype(np.uint64)
    nm = len(c) - m + 1
    if len(c) < k:
        return np.zeros(0, np.uint64)
    fwd, rc = np.zeros(nm, np.uint64), np.zeros(nm, np.uint64)
    for t in range(m):
        fwd |= c[t:t + nm] << np.uint64(2 * t)
        rc |= (c[t:t + nm] ^ np.uint64(2)) << np.uint64(2 * (m - 1 - t))
    o = skm_ord(np.minimum(fwd, rc), m)
    nk = len(c) - k + 1
    mn = o[:nk].copy()
    for t in range(1, w):
        mn = np.minimum(mn, o[t:t + nk])
    return mn


def stretches(eff):
    """[(start, length)] of the maximal stretches of bases in a window"""
    v = np.concatenate([[0], (_STD[np.frombuffer(eff, np.uint8)] < 4).astype(np.int8), [0]])
    d = np.diff(v)
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]).tolist()))


_RUNS = {}


def runs(eff, k):
    """[(first k-mer start, k-mers, smallest ord)] of the maximal runs of consecutive k-mers with one minimizer in a window"""
    key = (eff, k)
    if key not in _RUNS:
        out = []
        for s, n in stretches(eff):
            if n < k:
                continue
            mo = min_ords(eff[s:s + n], k)
            cut = np.concatenate([[0], np.nonzero(np.diff(mo) != 0)[0] + 1, [len(mo)]])
            out += [(s + int(a), int(b - a), int(mo[a])) for a, b in zip(cut[:-1], cut[1:])]
        if len(_RUNS) > 20000:
            _RUNS.clear()
        _RUNS[key] = out
    return _RUNS[key]


def longest_run(eff, k):
    return max([r[1] for r in runs(eff, k)] or [0])


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return s.translate(_COMP)[::-1]


# =====================================================================================================================================
# cases
# =====================================================================================================================================
class KCase:
    """name, the option list (behind -u x -d y --kmer_rarefaction), submissions of segments of (id, seq, qual), the edges it claims, table
    slots, environment switches for the device run, fresh: an engine of its own, ask: points and totals are read after every submission
    (which sends the pass through the table), expect: what the device run's diagnostics must report ('redo', 'overflow', 'fullest'; 'flushed': a group
    goes into the table before the pass ends, under every setting)"""

    def __init__(self, name, args, subs, claims, slots=1 << 22, env=None, fresh=False, ask=False, expect=()):
        self.name, self.args, self.subs, self.claims, self.slots = name, [str(a) for a in args], subs, tuple(claims), slots
        self.env, self.fresh, self.ask, self.expect, self._res, self._ctx = dict(env or {}), fresh, ask, tuple(expect), None, None

    def opt(self):
        from faqcs_amd.options import parse_args

        return parse_args(["-u", "x", "-d", "y", "--kmer_rarefaction"] + self.args)

    def group(self):
        return (tuple(self.args), self.slots)

    def ctx(self):
        if self._ctx is None:
            self._ctx = Ctx(self)
        return self._ctx


class Ctx:
    """What the predicates look at: the options, the model's trace of a fresh engine, and per submission the windows of its reads"""

    def __init__(self, case):
        self.case, self.o = case, case.opt()
        self.k, self.qc = self.o.kmer, self.o.qc_only
        m = Model(self.o)
        self.expected = run_model(m, case)
        self.trace = m.trace
        self.sub_of = [i for i, sub in enumerate(case.subs) for _ in sub]  # submission of trace entry t
        self.wins = [(s, q, a, n) for t in self.trace for s, q, a, n, c in t["wins"] if c]  # counted windows
        self.all_wins = [w for t in self.trace for w in t["wins"]]
        self.rq = 0 if self.qc else self.o.replace_to_N_q

    def eff(self, w):
        s, q, a, n = w[:4]
        return effective(s[a:a + n], q[a:a + n], self.rq)

    def sub_max_len(self, i):
        return max([len(r[1]) for seg in self.case.subs[i] for r in seg] or [0])

    def sub_wins(self, i):
        return [(s, q, a, n) for t, si in zip(self.trace, self.sub_of) if si == i for s, q, a, n, c in t["wins"] if c]


def rb(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.Generator(np.random.PCG64([4242, seed])).integers(0, 4, n)].tobytes()


def rd(seq, qual=None):
    return (b"@r", bytes(seq), bytes([GOOD]) * len(seq) if qual is None else bytes(qual))


def one(reads):
    """one submission of one segment"""
    return [[list(reads)]]


def TR(k, *extra):
    return ["--mode", "BWA", "--lc", "1.0", "--min_L", "1", "-n", "2000", "-m", k] + list(extra)


def QC(k, *extra):
    return ["--qc_only", "-m", k] + list(extra)


def pieces(n):
    """extraction rounds skm_extract takes for a window of n bases: the piece at pc is the last unless pc + 256 < a + n"""
    p, pc = 1, 0
    while pc + SKM_PIECE < n:
        pc += SKM_ADVANCE
        p += 1
    return p


EDGES = {}


def edge(name):
    def reg(f):
        EDGES[name] = f
        return f
    return reg


def with_base_flanks(c, w, p):
    """position p of the window has k bases on either side"""
    e = c.eff(w)
    return p >= c.k and p + c.k < len(e) and all(x < 4 for x in _STD[np.frombuffer(e[p - c.k:p] + e[p + 1:p + 1 + c.k], np.uint8)])


def nonbases(c, w):
    return np.nonzero(_STD[np.frombuffer(c.eff(w), np.uint8)] > 3)[0].tolist()


# ---- window and k ---------------------------------------------------------------------------------------------------------------------
for _k in KS:
    edge("k=%d" % _k)(lambda c, k=_k: c.k == k and c.expected["totals"][1] > 0)
for _mode in ("trim", "qc"):
    for _d in (-1, 0, 1):
        edge("%s:window_len=k%+d" % (_mode, _d))(lambda c, d=_d, mode=_mode: c.qc == (mode == "qc") and any(w[3] == c.k + d for w in c.wins))
    edge("%s:window_len=0" % _mode)(lambda c, mode=_mode: c.qc == (mode == "qc") and any(w[3] == 0 for w in c.all_wins))
    edge("%s:window_len=1" % _mode)(lambda c, mode=_mode: c.qc == (mode == "qc") and any(w[3] == 1 for w in c.wins))
    edge("%s:empty_read" % _mode)(lambda c, mode=_mode: c.qc == (mode == "qc") and any(len(w[0]) == 0 for w in c.all_wins))
    edge("%s:every_arena_residue_mod_16" % _mode)(lambda c, mode=_mode: c.qc == (mode == "qc") and _residues(c) == set(range(16)))
    edge("%s:last_read_ends_the_arena_window_not_multiple_of_4" % _mode)(lambda c, mode=_mode: c.qc == (mode == "qc") and _last_read(c))
edge("trim:invalid_read_between_valid_ones")(lambda c: not c.qc and any(not a[4] and len(a[0]) and b[4] and b[3] >= c.k and z[4] and z[3] >= c.k
                                                                         for t in c.trace for b, a, z in zip(t["wins"], t["wins"][1:], t["wins"][2:])))
edge("qc:invalid_read_is_counted")(lambda c: c.qc and any(w[0] == b"N" * 40 for w in c.wins) and any(len(w[0]) == 0 for w in c.wins) and
                                   c.trace[-1]["total"] == len(c.all_wins) == len(c.wins))
for _a in range(6):
    edge("a=%d" % _a)(lambda c, a=_a: not c.qc and c.o.trim_5 == a and any(w[2] == a and w[3] >= c.k for w in c.wins))


def _residues(c):
    out = set()
    for sub in c.case.subs:
        at = 0
        for seg in sub:
            for r in seg:
                if len(r[1]) >= c.k + c.o.trim_5:
                    out.add(at % 16)
                at += len(r[1])
    return out


def _last_read(c):
    s, q, a, n, counted = c.trace[-1]["wins"][-1]
    return counted and n >= c.k and n % 4 != 0 and a + n == len(s)


# ---- bases and bytes ------------------------------------------------------------------------------------------------------------------
# (every byte value listed in the issue; none had to be dropped: the trim results and counters agree on all of them)
BYTES = list(b"acgtACGTNn@`") + [0x00, 0x01, 0x21, 0x23, 0x27, 0x34, 0x80, 0xC1, 0xE1, 0xFF] + list(b"BDEF")
edge("qc:every_confusable_byte_inside_bases")(lambda c: c.qc and all(any(len(w[0]) > 35 and w[0][35] == b and with_base_flanks(c, w, 35) for w in c.wins) for b in BYTES))
edge("nonbase_at_0..k+1_from_either_end")(lambda c: all(any(nonbases(c, w) == [j] and w[3] >= 2 * c.k + 4 for w in c.wins) and
                                                         any(nonbases(c, w) == [w[3] - 1 - j] and w[3] >= 2 * c.k + 4 for w in c.wins) for j in range(c.k + 2)))
for _d in (-1, 0, 1):
    edge("two_nonbases_k%+d_apart" % _d)(lambda c, d=_d: any(len(nb) == 2 and nb[1] - nb[0] == c.k + d and nb[0] >= c.k for w in c.wins for nb in [nonbases(c, w)]))
LANE_BORDERS = sorted({x for l in (1, 2, 5, 9, 15) for x in (16 * l - 1, 16 * l, 4 * l - 1, 4 * l)})
PIECE_BORDERS = (199, 200, 229, 230, 255, 256)
edge("nonbase_at_lane_borders")(lambda c: all(any(nonbases(c, w) == [p] and w[3] == 256 for w in c.wins) for p in LANE_BORDERS))
edge("nonbase_at_piece_borders")(lambda c: all(any(nonbases(c, w) == [p] and w[3] == 400 for w in c.wins) for p in PIECE_BORDERS))
edge("more_than_64_nonbases_in_a_piece")(lambda c: any(len([p for p in nb if p < 256]) > 64 and {p % 4 for p in nb if p < 256} == {0, 1, 2, 3} and c.expected["totals"][1] > 0
                                                       for w in c.wins for nb in [nonbases(c, w)]))


def _g2n(c, base, pred):
    return c.rq > 0 and any(s[p] == base and pred(q[p]) and with_base_flanks(c, (s, q, a, n), p - a) or False
                            for s, q, a, n in c.wins for p in range(a, a + n) if s[p] in b"Gg" and pred(q[p]))


edge("g2n:low_quality_G_replaced")(lambda c: c.rq > 0 and any(s[p] == ord("G") and IN_OFF <= q[p] < IN_OFF + c.rq and c.eff((s, q, a, n))[p - a] == ord("N") and
                                                                with_base_flanks(c, (s, q, a, n), p - a) for s, q, a, n in c.wins for p in range(a, a + n)))
edge("g2n:low_quality_g_kept")(lambda c: _g2n(c, ord("g"), lambda q: IN_OFF <= q < IN_OFF + c.rq))
edge("g2n:high_quality_G_kept")(lambda c: _g2n(c, ord("G"), lambda q: q >= IN_OFF + c.rq))
edge("g2n:quality_byte_below_the_offset")(lambda c: c.rq > 0 and any(s[p] == ord("G") and q[p] < IN_OFF and c.eff((s, q, a, n))[p - a] == ord("N")
                                                                      for s, q, a, n in c.wins for p in range(a, a + n)))

# ---- lengths and pieces ---------------------------------------------------------------------------------------------------------------
LENGTHS = (255, 256, 257, 286, 287, 456, 457, 656)
for _L in LENGTHS:
    edge("window_len=%d" % _L)(lambda c, L=_L: any(w[3] == L and w[2] == 0 for w in c.wins))
    edge("a=3:window_len=%d" % _L)(lambda c, L=_L: any(w[3] == L and w[2] == 3 for w in c.wins))
for _p in (1, 2, 3):
    edge("pieces=%d" % _p)(lambda c, p=_p: any(pieces(w[3]) == p and w[3] >= c.k for w in c.wins))
edge("last_piece_has_kmer_starts_200_and_beyond")(lambda c: any(pieces(w[3]) > 1 and w[3] - SKM_ADVANCE * (pieces(w[3]) - 1) - c.k >= SKM_ADVANCE for w in c.wins))
edge("k=31:submission_for_the_16_byte_kernel")(lambda c: c.k == 31 and any(c.sub_max_len(i) <= 256 and any(w[3] >= 31 for w in c.sub_wins(i)) for i in range(len(c.case.subs))))
edge("k=31:short_reads_through_the_general_kernel")(lambda c: c.k == 31 and any(c.sub_max_len(i) > 256 and any(31 <= w[3] and len(w[0]) <= 256 for w in c.sub_wins(i))
                                                                                  for i in range(len(c.case.subs))))
edge("k<31")(lambda c: 15 < c.k < 31)

# ---- runs -----------------------------------------------------------------------------------------------------------------------------
for _k, _n in ((31, 16), (31, 17), (31, 18), (31, 35), (16, 2), (16, 3)):
    edge("k=%d:longest_run=%d" % (_k, _n))(lambda c, k=_k, n=_n: c.k == k and any(longest_run(c.eff(w), k) == n for w in c.wins))
HOMOPOLYMERS = (31, 47, 48, 250, 600)
edge("homopolymers_of_every_base")(lambda c: all(any(c.eff(w) == bytes([b]) * n for w in c.wins) for b in b"ACGT" for n in HOMOPOLYMERS))


def _repeat(c, p):
    def rep(e):
        return len(e) >= c.k + 2 * p and e == (e[:p] * (len(e) // p + 1))[:len(e)] and len(set(e[:p])) > 1 and all(e[:p] != (e[:q] * p)[:p] for q in range(1, p))
    return any(rep(c.eff(w)) for w in c.wins)


edge("dinucleotide_repeat")(lambda c: _repeat(c, 2))
edge("trinucleotide_repeat")(lambda c: _repeat(c, 3))
edge("read_and_reverse_complement_in_one_segment")(lambda c: any(any(revcomp(c.eff(a)) == c.eff(b) and c.eff(a) != c.eff(b) and a[3] > c.k for a in ws for b in ws)
                                                                 for t in c.trace for ws in [[w for w in t["wins"] if w[4]]]))
edge("k=30:palindromic_key")(lambda c: c.k == 30 and any(c.eff(w) == revcomp(c.eff(w)) and w[3] == 30 for w in c.wins) and
                             c.expected["totals"] == (1, len(c.wins)))
edge("run_starts_at_the_last_kmer_start_of_a_piece")(lambda c: any(pieces(w[3]) > 1 and any(r[0] == SKM_ADVANCE - 1 and r[1] > 1 for r in runs(c.eff(w), c.k)) for w in c.wins))
edge("run_crosses_the_piece_limit")(lambda c: any(pieces(w[3]) > 1 and any(r[0] < SKM_ADVANCE - 2 and r[0] + r[1] > SKM_ADVANCE + 2 for r in runs(c.eff(w), c.k)) for w in c.wins))
edge("k=31:item_whose_bases_32..46_are_all_G")(lambda c: c.k == 31 and any(r[1] == 17 and e[r[0] + 32:r[0] + 47] == b"G" * 15 for w in c.wins for e in [c.eff(w)] for r in runs(e, 31)))
edge("k=31:item_of_1_kmer")(lambda c: c.k == 31 and any(w[3] == 31 and len(runs(c.eff(w), 31)) == 1 for w in c.wins))
edge("k=31:item_of_17_kmers")(lambda c: c.k == 31 and any(r[1] == 17 for w in c.wins for r in runs(c.eff(w), 31)))

# ---- counts ---------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 255, 256, 257, 65535, 65536, 65537)


def _one_key(c, n, both):
    e = {c.eff(w) for w in c.wins}
    return c.k == 31 and len(c.wins) == n and all(len(x) == 31 for x in e) and c.expected["hist"] == [(n, 1)] and \
        (len(e) == 2 and revcomp(min(e)) == max(e) if both else len(e) == 1)


for _n in COUNTS:
    edge("count=%d" % _n)(lambda c, n=_n: _one_key(c, n, False))
    if _n > 1:
        edge("count=%d_on_both_strands" % _n)(lambda c, n=_n: _one_key(c, n, True))
edge("counts_either_side_of_dense_n")(lambda c: [n for n, _ in c.expected["hist"]] == [DENSE_N - 1, DENSE_N, DENSE_N + 4])
edge("one_key_beyond_2^17_from_items_of_17")(lambda c: c.k == 31 and {c.eff(w) for w in c.wins} == {b"A" * 47} and c.expected["hist"] == [(17 * len(c.wins), 1)] and 17 * len(c.wins) > 1 << 17)

# ---- epochs and points ----------------------------------------------------------------------------------------------------------------
for _s in (1, 2, 7):
    edge("split_size=%d" % _s)(lambda c, s=_s: c.o.split_size == s and len(c.expected["points"]) > 1)
edge("cumulative_count_one_below_on_and_one_past_a_multiple")(lambda c: c.o.split_size > 2 and {t["total"] % c.o.split_size for t in c.trace if t["active"] and t["n"]} >= {c.o.split_size - 1, 0, 1})
edge("segment_crosses_three_multiples")(lambda c: any(t["active"] and t["point"] and t["total"] // c.o.split_size - (t["total"] - t["n"]) // c.o.split_size >= 3 for t in c.trace))
edge("segment_of_zero_reads")(lambda c: any(t["n"] == 0 and t["active"] for t in c.trace[1:-1]))
edge("segments_without_kmers_between_ones_with")(lambda c: any(a["kmers"] and not b["kmers"] and b["n"] and z["kmers"] for a, b, z in zip(c.trace, c.trace[1:], c.trace[2:])))


def _stop(c):
    """(index of the last segment counted, its submission) when the curve completes inside the case, else None"""
    off = [i for i, t in enumerate(c.trace) if not t["active"]]
    if not off or not c.trace[off[0] - 1]["kmers"] or not any(len(seg) for seg in sum(c.case.subs, [])[off[0]:]):
        return None
    return off[0] - 1, c.sub_of[off[0] - 1]


edge("num_subsample_reached_in_the_middle_of_a_submission")(lambda c: _stop(c) is not None and c.sub_of[_stop(c)[0] + 1] == _stop(c)[1] and c.sub_of[_stop(c)[0] - 1] == _stop(c)[1] and not c.expected["active"])
edge("last_point_at_the_end_of_a_submission")(lambda c: _stop(c) is not None and c.sub_of[_stop(c)[0] - 1] != _stop(c)[1] and c.trace[_stop(c)[0] - 1]["point"] and not c.expected["active"])
edge("key_in_epochs_e_e+1_and_the_last")(lambda c: c.o.split_size == 1 and len(c.trace) >= 5 and c.case.subs[0][1] == c.case.subs[0][2] == c.case.subs[0][-1] and
                                         c.expected["points"][2][1] == c.expected["points"][1][1] and all(t["point"] for t in c.trace))
edge("more_epochs_than_a_group_spans")(lambda c: len(c.case.subs) == 1 and sum(t["point"] for t in c.trace) > max(KG_EPOCH_SPAN, KG_MAX_RUNS) and all(t["kmers"] for t in c.trace))
edge("points_asked_for_after_each_of_three_submissions")(lambda c: c.case.ask and len(c.case.subs) == 3 and all(p for p, _, _ in c.expected["after"]))

# ---- partitions -----------------------------------------------------------------------------------------------------------------------


def _parts(c):
    """{19-bit partition: distinct canonical k-mers} over single-k-mer windows"""
    eff = sorted({c.eff(w) for w in c.wins if w[3] == c.k})
    keys = canonical_kmers(eff, c.k)
    part = [int(skm_part(min_ords(e, c.k)[0])) for e in eff]
    out = {}
    for p, key in zip(part, keys.tolist()):
        out.setdefault(p, set()).add(key)
    return out


edge("one_partition_beyond_an_LDS_round")(lambda c: max(len(v) for v in _parts(c).values()) > LDS_SLOTS > LDS_ROUND_KEYS)
edge("one_bucket_fed_200_items")(lambda c: max(sum(1 for w in c.wins if w[3] == c.k and int(skm_part(min_ords(c.eff(w), c.k)[0])) >> 11 == b) for b in {p >> 11 for p in _parts(c)}) >= 200)
edge("table_slots=2^22")(lambda c: c.case.slots == 1 << 22 and "overflow" in c.case.expect)
edge("table_slots=2^24")(lambda c: c.case.slots == 1 << 24 and "redo" in c.case.expect)


# =====================================================================================================================================
# builders
# =====================================================================================================================================
def window_case(k, a, qc):
    reads, seed = [], 1000 * k + 10 * a
    for L in (0, 1, k - 1, k, k + 1):
        reads.append(rd(rb(L + a if L else 0, seed + L)))
    reads += [rd(rb(a, seed + 50)), rd(rb(k + 5 + a, seed + 51)), rd(b"N" * 40), rd(rb(k + 9 + a, seed + 53))]
    at = sum(len(r[1]) for r in reads)
    for r in range(16):  # a read at every residue of the arena offset mod 16, behind a spacer of 1 .. 16 bases
        sp = (r - at) % 16 or 16
        reads += [rd(rb(sp, seed + 100 + r)), rd(rb(k + 7 + a, seed + 200 + r))]
        at += sp + k + 7 + a
    Lf = k + 2 if (k + 2) % 4 else k + 3
    reads.append(rd(rb(Lf + a, seed + 300)))
    mode = "qc" if qc else "trim"
    claims = ["%s:window_len=%s" % (mode, x) for x in ("k-1", "k+0", "k+1", "0", "1")] + ["%s:empty_read" % mode, "%s:every_arena_residue_mod_16" % mode,
                                                                                            "%s:last_read_ends_the_arena_window_not_multiple_of_4" % mode]
    claims += ["qc:invalid_read_is_counted"] if qc else ["trim:invalid_read_between_valid_ones", "a=%d" % a]
    if a == 0:
        claims.append("k=%d" % k)
    # (the read of 40 N: what the quality trim leaves of it is an N, and -n 1 allows none; under --qc_only it is counted like any other)
    return KCase("window_k%d_%s" % (k, "qc" if qc else "a%d" % a), QC(k) if qc else TR(k, "--5end", a, "-n", 1), one(reads), claims)


def bytes_case(k):
    reads = [rd(rb(35, 7000 + b) + bytes([b]) + rb(35, 7300 + b)) for b in BYTES]
    return KCase("bytes_k%d" % k, QC(k), one(reads), ["qc:every_confusable_byte_inside_bases"])


def _with(s, positions, byte=b"N"):
    s = bytearray(s)
    for p in positions:
        s[p:p + 1] = byte
    return bytes(s)


def nonbase_case(k, qc=True, a=0):
    short, seed = [], 9000 + k
    L = 2 * k + 10
    for j in range(k + 2):
        short += [rd(rb(a, 1) + _with(rb(L, seed + j), [j])), rd(rb(a, 2) + _with(rb(L, seed + 50 + j), [L - 1 - j], b"n"))]
    for d in (-1, 0, 1):
        short.append(rd(rb(a, 3) + _with(rb(3 * k + 10, seed + 100 + d), [k + 2, k + 2 + k + d], b".")))
    for p in LANE_BORDERS:
        short.append(rd(rb(a, 4) + _with(rb(256, seed + 200 + p), [p])))
    long_ = [rd(rb(a, 5) + _with(rb(400, seed + 500 + p), [p])) for p in PIECE_BORDERS]
    long_.append(rd(rb(a, 6) + _with(rb(400, seed + 600), range(0, 210, 3), b"N")))
    long_.append(rd(rb(a, 7) + _with(rb(400, seed + 601), [p for p in range(0, 256) if p % 5 in (0, 2)], b"-")))
    claims = ["nonbase_at_0..k+1_from_either_end", "two_nonbases_k-1_apart", "two_nonbases_k+0_apart", "two_nonbases_k+1_apart", "nonbase_at_lane_borders",
              "nonbase_at_piece_borders", "more_than_64_nonbases_in_a_piece"]
    return KCase("nonbases_k%d_%s" % (k, "qc" if qc else "a%d" % a), QC(k) if qc else TR(k, "--5end", a), [[short], [long_]], claims)


def g2n_case(k):
    reads = []
    for i, (base, q) in enumerate(((b"G", b"+"), (b"g", b"+"), (b"G", b"I"), (b"G", b" "), (b"G", b"5"), (b"g", b" "))):  # threshold 20: '5' is exactly 20
        s = _with(rb(2 * k + 21, 11000 + 10 * k + i).replace(b"G", b"C"), [k + 10], base)
        reads.append(rd(s, _with(bytes([GOOD]) * len(s), [k + 10], q)))
    claims = ["g2n:low_quality_G_replaced", "g2n:low_quality_g_kept", "g2n:high_quality_G_kept", "g2n:quality_byte_below_the_offset"]
    return KCase("replace_to_N_k%d" % k, TR(k, "--replace_to_N_q", 20, "-q", 0), one(reads), claims)


def lengths_case(k, a):
    subs = []
    for i, L in enumerate(LENGTHS):
        subs.append([[rd(rb(L + a, 13000 + 100 * k + 10 * a + i)), rd(_with(rb(L + a, 13500 + 100 * k + 10 * a + i), [L // 2])), rd(rb(L + a, 13000 + 100 * k + 10 * a + i))]])
    pre = "a=3:" if a else ""
    claims = [pre + "window_len=%d" % L for L in LENGTHS] + ["pieces=1", "pieces=2", "pieces=3", "last_piece_has_kmer_starts_200_and_beyond"]
    claims += (["k=31:submission_for_the_16_byte_kernel"] if a == 0 else []) if k == 31 else ["k<31"]
    return KCase("lengths_k%d_a%d" % (k, a), TR(k, "--5end", a), subs, claims)


def short_reads(k=31):
    return window_case(k, 0, False).subs[0][0] + nonbase_case(k).subs[0][0][:20]


def kernel_twin_cases():
    """the same short reads through skm_extract16 and -- an all-N read of 257 bases behind them -- through skm_extract: the same k-mers"""
    a = KCase("short_reads_16_byte_kernel", TR(31), one(short_reads()), ["k=31:submission_for_the_16_byte_kernel"])
    b = KCase("short_reads_general_kernel", TR(31), one(short_reads() + [rd(b"N" * 257)]), ["k=31:short_reads_through_the_general_kernel"])
    return [a, b]


def find_read(k, want, kind, seed0):
    """seeded search: the first candidate whose longest run of equal minimizers is exactly `want` k-mers"""
    for seed in range(seed0, seed0 + 20000):
        if kind == "random":
            s = rb(k + 40, seed)
        else:  # a tandem repeat between random flanks: its m-mers recur, so one minimizer holds over the whole repeat
            unit = rb(5 + seed % 4, seed)
            s = rb(20, seed + 1) + (unit * 40)[:want + k - 16 + seed % 9] + rb(20, seed + 2)
        if longest_run(s, k) == want:
            return s
    raise AssertionError("no read with a run of %d at k = %d" % (want, k))


def run_cases():
    C = []
    reads = {n: find_read(31, n, "random" if n <= 17 else "repeat", 100 * n) for n in (16, 17, 18, 35)}
    for n, s in reads.items():
        C.append(KCase("run_of_%d_k31" % n, TR(31), one([rd(s), rd(rb(60, n))]), ["k=31:longest_run=%d" % n] + (["k=31:item_of_17_kmers"] if n == 17 else [])))
    C.append(KCase("runs_of_2_and_3_k16", TR(16), one([rd(find_read(16, 2, "random", 5)), rd(find_read(16, 3, "random", 900))]), ["k=16:longest_run=2", "k=16:longest_run=3"]))
    homo = [rd(bytes([b]) * n) for b in b"ACGT" for n in HOMOPOLYMERS]
    C.append(KCase("homopolymers_k31", TR(31), [[[r for r in homo if len(r[1]) <= 256]], [[r for r in homo if len(r[1]) > 256]]], ["homopolymers_of_every_base"]))
    C.append(KCase("homopolymers_k17", TR(17), [[[r for r in homo if len(r[1]) <= 256]], [[r for r in homo if len(r[1]) > 256]]], ["homopolymers_of_every_base"]))
    for k in (31, 16):
        reps = [rd((u * 400)[:n]) for u in (b"AC", b"GT", b"AG", b"ACG", b"TTG", b"CAG") for n in (k + 6, 120, 256, 333)]
        C.append(KCase("repeats_k%d" % k, TR(k), [[[r for r in reps if len(r[1]) <= 256]], [[r for r in reps if len(r[1]) > 256]]], ["dinucleotide_repeat", "trinucleotide_repeat"]))
        s = [rb(90, 15000 + k), rb(250, 15001 + k)]
        C.append(KCase("read_and_reverse_complement_k%d" % k, TR(k), one([rd(s[0]), rd(revcomp(s[0])), rd(revcomp(s[1])), rd(s[1])]), ["read_and_reverse_complement_in_one_segment"]))
    half = rb(15, 16000)
    pal = half + revcomp(half)
    C.append(KCase("palindrome_k30", TR(30), one([rd(pal)] * 3), ["k=30:palindromic_key"]))
    for name, e, seed0 in (("run_starts_at_199", "run_starts_at_the_last_kmer_start_of_a_piece", 17000), ("run_crosses_200", "run_crosses_the_piece_limit", 17500)):
        for seed in range(seed0, seed0 + 2000):
            c = KCase(name + "_k31", TR(31), one([rd(rb(500, seed))]), [e])
            if EDGES[e](c.ctx()):
                break
        C.append(c)
    for seed in range(18000, 40000):  # an item of 17 k-mers whose bases 32 .. 46 are all G: a 47-base read with one minimizer
        s = rb(32, seed) + b"G" * 15
        if [r[:2] for r in runs(s, 31)] == [(0, 17)]:
            break
    C.append(KCase("item_high_bases_all_G", TR(31), one([rd(s), rd(s), rd(rb(31, 18))]), ["k=31:item_whose_bases_32..46_are_all_G", "k=31:item_of_17_kmers", "k=31:item_of_1_kmer"]))
    return C


def count_cases():
    C, s = [], rb(31, 19000)
    args = TR(31, "--min_L", 31)
    for n in COUNTS:
        C.append(KCase("count_%d" % n, args, one([rd(s)] * n), ["count=%d" % n]))
        if n > 1:
            C.append(KCase("count_%d_both_strands" % n, args, one([rd(s)] * (n // 2) + [rd(revcomp(s))] * (n - n // 2)), ["count=%d_on_both_strands" % n]))
    t, u = rb(31, 19001), rb(31, 19002)
    mixed = [rd(x) for i in range(DENSE_N + 4) for x in ((s,) + ((t,) if i < DENSE_N else ()) + ((u,) if i < DENSE_N - 1 else ()))]
    C.append(KCase("counts_either_side_of_dense_n", args, one(mixed), ["counts_either_side_of_dense_n"]))
    C.append(KCase("poly_A_beyond_2_17", args, one([rd(b"A" * 47)] * ((1 << 17) // 17 + 2)), ["one_key_beyond_2^17_from_items_of_17"]))
    return C


def point_cases():
    C, k = [], 16

    def segs(counts, seed, short=()):
        return [[rd(rb(k - 1 if i in short else k + 4, seed + 100 * i + j)) for j in range(n)] for i, n in enumerate(counts)]

    C.append(KCase("points_split_7", QC(k, "--split_size", 7, "--subset", 10), [segs([6, 1, 1, 5, 1, 1, 0, 22, 3], 20000), segs([2, 4, 3, 6], 20500, short=(2,))],
                   ["split_size=7", "cumulative_count_one_below_on_and_one_past_a_multiple", "segment_crosses_three_multiples", "segment_of_zero_reads",
                    "segments_without_kmers_between_ones_with"], fresh=True))
    C.append(KCase("points_split_2_curve_completes_inside_a_submission", QC(k, "--split_size", 2, "--subset", 1), [segs([2, 2, 2, 2, 2], 21000), segs([2, 2], 21500)],
                   ["split_size=2", "num_subsample_reached_in_the_middle_of_a_submission"], fresh=True))
    C.append(KCase("points_split_2_last_point_ends_a_submission", QC(k, "--split_size", 2, "--subset", 1), [segs([2, 2], 22000), segs([2, 2, 2], 22500)],
                   ["last_point_at_the_end_of_a_submission"], fresh=True))
    first = segs([1] * 7, 23000)
    first[2] = first[-1] = first[1]
    C.append(KCase("points_split_1_key_in_three_epochs", QC(k, "--split_size", 1, "--subset", 10), [first], ["split_size=1", "key_in_epochs_e_e+1_and_the_last"], fresh=True))
    C.append(KCase("points_1100_epochs", QC(k, "--split_size", 1, "--subset", 600), [segs([1] * 1100, 24000)], ["more_epochs_than_a_group_spans"], fresh=True, expect=("flushed",)))
    C.append(KCase("points_asked_after_each_submission", QC(31, "--split_size", 7, "--subset", 10), [segs([5, 4], 25000), segs([9], 25100), segs([3, 8], 25200)],
                   ["points_asked_for_after_each_of_three_submissions"], fresh=True, ask=True))
    return C


N_ONE_MINIMIZER = 4400  # more keys than the LDS table has slots (4 096): skm_combine<KS_COUNT> cannot take the partition, whatever its probe lengths


def partition_cases():
    """4 400 distinct 31-mers with one minimizer: a 15-mer core that comes early in the order between random 8-base flanks.  (3 000 keys, beyond
    the 2 816 of a KS_GROUP / KS_REDO round, still fit the 4 096 slots of KS_COUNT, whose only limit is a probe sequence of 256: measured, the
    pass was counted without a single partition redone.)"""
    for seed in range(26000, 46000):
        core = rb(15, seed)
        if int(min_ords(core, 15)[0]) < (1 << 30) // 20000:
            break
    reads = [rd(rb(8, 27000 + i) + core + rb(8, 57000 + i)) for i in range(N_ONE_MINIMIZER)]
    claims = ["one_partition_beyond_an_LDS_round", "one_bucket_fed_200_items"]
    args = TR(31, "--min_L", 31)
    # 2^22 slots, the group buffers of that table: what does not fit a region goes occurrence by occurrence into the partition's 64-slot slice
    # (dirty: KS_REDO) and from there into the overflow area.  2^24 slots with group buffers that hold all 4 400 items of the partition
    # (FAQCS_KMER_GROUP_ITEMS, as test_kmer_partition_counted_in_several_rounds sets it): more keys than the LDS table has slots.
    return [KCase("one_minimizer_slots_2_22", args, one(reads), claims + ["table_slots=2^22"], slots=1 << 22, expect=("redo", "overflow"), fresh=True),
            KCase("one_minimizer_slots_2_24", args, one(reads), claims + ["table_slots=2^24"], slots=1 << 24, env={"FAQCS_KMER_DEBUG": "1", "FAQCS_KMER_GROUP_ITEMS": str(1 << 30)},
                  expect=("redo", "fullest"), fresh=True)]


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        F = {"window": [], "bytes": [], "lengths": [], "runs": [], "counts": [], "points": [], "partitions": []}
        for k in KS:
            F["window"] += [window_case(k, 0, False), window_case(k, 3, False), window_case(k, 0, True)]
        for k in (31, 16):
            F["window"] += [window_case(k, a, False) for a in (1, 2, 4, 5)]
            F["bytes"] += [bytes_case(k), nonbase_case(k), g2n_case(k)]
        F["bytes"] += [nonbase_case(31, qc=False, a=3), nonbase_case(17)]
        F["lengths"] += [lengths_case(k, a) for k in (31, 17) for a in (0, 3)] + kernel_twin_cases()
        F["runs"], F["counts"], F["points"], F["partitions"] = run_cases(), count_cases(), point_cases(), partition_cases()
        C = []
        for fam, cs in F.items():
            for c in cs:
                c.family = fam
            C += cs
        _CASES = C
    return _CASES


FAMILIES = ("window", "bytes", "lengths", "runs", "counts", "points", "partitions")
TWO_PASSES = ("run_of_18_k31", "homopolymers_k31")  # two different cases of one option list: both orders on one engine


def engine_runs(cases=None, family=None):
    """The engines of a run of the catalogue: the cases of one option list and table size are consecutive passes on one engine (kmer_end_table
    between them; TOTAL_NUMBER, the points and the histogram go on), a `fresh` case has an engine of its own, and TWO_PASSES run in both
    orders on engines of their own.  -> [[case, ...], ...]"""
    cases = [c for c in (all_cases() if cases is None else cases) if family is None or c.family == family]
    shared, out = {}, []
    for c in cases:
        if c.fresh:
            out.append([c])
        else:
            shared.setdefault(c.group(), []).append(c)
    by_name = {c.name: c for c in cases}
    if all(n in by_name for n in TWO_PASSES):
        x, y = (by_name[n] for n in TWO_PASSES)
        assert x.group() == y.group()
        out += [[x, y], [y, x]]
    return out + list(shared.values())


def coverage(cases=None):
    """-> ({edge: [cases that claim it and reach it]}, {case: [claims that do not hold]})"""
    cases = all_cases() if cases is None else cases
    table, lost = {e: [] for e in EDGES}, {}
    for c in cases:
        for e in c.claims:
            if e in EDGES and EDGES[e](c.ctx()):
                table[e].append(c.name)
            else:
                lost.setdefault(c.name, []).append(e)
    return table, lost


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t, lost = coverage()
    for e, v in t.items():
        print("%3d  %s" % (len(v), e))
    print("%d cases, %d edges; claims that do not hold: %s" % (len(all_cases()), len(t), lost))
