"""A constructed catalogue of inputs for the trim stage (trim_lds, trim_filter_accumulate, trim_long; faqcs_trim_lds_kernel.hip,
faqcs_trim_kernel.hip, faqcs_trim_long_kernel.hip, build_tables() of faqcs_capi.hip), in the style of tests/kmer_edges.py: the edges of the
three quality walks, of the two length filters and the fixed cuts, of the terminal-N mask and the poly-N rule, of the float32 thresholds of
--lc and --avg_q and of the composition bins, of the chunks, rows and arena offsets of the chunked kernels, of the byte values a read can
hold, and of trim_long's 64-position steps.  Every case is a named builder of submissions of segments of reads, every edge a PREDICATE over
a case's inputs and the model's per-read trace; coverage() evaluates every predicate on every case.

model(case) is the plain reference: trim_read (trim.cpp:225-551) read by read on Python ints, float32 (numpy.float32, one operation at a
time) only where the reference computes in `float` -- average_quality, the two norm products of the low-complexity test and the composition
norm --, and the whole counter block laid out by capi.python_layout; only the four position matrices are filled with numpy, from the
windows the per-read walk decided.  It shares nothing with oracle/ or with the kernels' host tables.  It does not cover adapters or
k-mers.  tests/test_trim_edges_model.py holds the model to the oracle without a GPU; tests/test_gpu_trim_edges.py sends the catalogue to
the device.

    python -m tests.trim_edges        prints the number of cases per edge
"""
import itertools
import os
import sys
from fractions import Fraction

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from trim_dispatch_cases import FAST_READ_LENGTH, LDS_ROWS

NQ, NBASE, NCOMP_BIN, NCOMP_KIND = 42, 5, 10001, 6
PAD_BEFORE, PAD_AFTER = 16, 64   # restated; test_trim_edges_model.py compares them with include/faqcs_mi.h
CONSTANT_SOURCES = {"PAD_BEFORE": r"#define FAQCS_ARENA_PAD_BEFORE (\d+)", "PAD_AFTER": r"#define FAQCS_ARENA_PAD_AFTER (\d+)", "NQ": r"#define FAQCS_NQ\s+(\d+)",
                    "NBASE": r"#define FAQCS_NBASE\s+(\d+)", "NCOMP_BIN": r"#define FAQCS_NCOMP_BIN\s+(\d+)", "NCOMP_KIND": r"#define FAQCS_NCOMP_KIND\s+(\d+)"}
# FilterStat (FaQCs.h), restated: test_trim_edges_model.py compares the names' order with faqcs_amd/_capi.py
STAT = ("TOTAL_COUNT", "TOTAL_NUMBER", "TOTAL_LENGTH", "TOTAL_TRIMMED_NUMBER", "TOTAL_TRIMMED_LENGTH", "PAIRED_READ_NUMBER", "PAIRED_BASE_LENGTH", "READ_LENGTH",
        "BASE_LENGTH", "READ_NN", "BASE_NN", "READ_PHIX", "BASE_PHIX", "READ_ADAPTER", "BASE_ADAPTER", "READ_AVG_Q", "BASE_AVG_Q", "READ_QUAL_TRIM", "BASE_QUAL_TRIM",
        "READ_LOW_COMPLEXITY", "BASE_LOW_COMPLEXITY")
S = {n: i for i, n in enumerate(STAT)}
F_VALID, F_QUAL_TRIMMED, F_POLY_N_SEEN = 0x1, 0x10, 0x40
FILT_NONE, FILT_LENGTH_PRE, FILT_LENGTH_POST, FILT_POLY_N, FILT_AVG_Q, FILT_LOW_COMPLEXITY = range(6)
E_QUALITY = -3
MODE_HARD, MODE_BWA, MODE_BWA_PLUS = 0, 1, 2

ROW_FIRST = [r[0] for r in LDS_ROWS]          # 1, 53, 77, 105, 153, 253
ROW_LAST = [r[1] for r in LDS_ROWS]           # 52, 76, 104, 152, 252, 304
TFA_FIRST = ROW_LAST[-1] + 1                  # 305: the first length trim_filter_accumulate takes by itself
ROW_LENGTHS = sorted(ROW_FIRST + ROW_LAST + [TFA_FIRST])
SETTINGS = ("lds", "long", "single_pass")
f32 = np.float32


def layout(R):
    """capi.python_layout without adapters, restated (the CPU test compares the two)"""
    o, out = 0, {}
    for name, size in (("filter_stats", 32), ("pre_read_qhist", NQ), ("pre_base_qhist", NQ), ("post_read_qhist", NQ), ("post_base_qhist", NQ), ("pre_len_hist", R + 1),
                       ("post_len_hist", R + 1), ("pre_qual", R * NQ), ("post_qual", R * NQ), ("pre_base", R * NBASE), ("post_base", R * NBASE),
                       ("pre_comp", NCOMP_BIN * NCOMP_KIND), ("post_comp", NCOMP_BIN * NCOMP_KIND), ("adapter_stats", 0)):
        out[name] = (o, size)
        o += size
    out["total"] = o
    return out


# =====================================================================================================================================
# the model
# =====================================================================================================================================
class QualityError(Exception):
    pass


class Info:
    """What the model saw of one read: n0 raw length, pre the length after the fixed cuts, a / kept the window, flags, filt, w the walk's trace,
    cmax / dmax the commonest base / transition of the window, qsum the window's sum of raw - offset, npoly its longest run of N, bins the
    composition bins (pre, post or None)"""
    __slots__ = ("n0", "pre", "a", "kept", "flags", "filt", "w", "cmax", "dmax", "qsum", "npoly", "bins", "counts", "pre_bin", "wlen")


def scores_of(q, off):
    """fastq.h:17-36: the byte as a signed char minus the offset, not below 0; above 41 throws"""
    out = []
    for b in q:
        v = (b - 256 if b > 127 else b) - off
        if v > 41:
            raise QualityError()
        out.append(v if v > 0 else 0)
    return out


def raw_sum(q):
    return sum(q) - 256 * sum(1 for b in q if b > 127)


def walk_bwa_plus(sc, Q, protect5):
    """trim.cpp:714-793 -> (final_pos_5, kept, trace)"""
    n = len(sc)
    scan, after = min(5, n), min(2, n)
    p3 = n - 1
    f5, f3, area, best, step = 0, n - 1, 0, 0, 0
    w = dict(step3=-1, tie3=False, zero3=False, neg3=-1, steps3=0, step5=-1, tie5=False, steps5=0, fast3=0)
    while scan:
        scan -= 1
        if p3 > after and area >= 0:
            scan = after
        assert p3 >= 0
        before = area
        area += Q - sc[p3]
        if area > best:
            best, f3, w["step3"] = area, p3 - 1, step
        elif area == best and best > 0 and Q != sc[p3]:
            w["tie3"] = True
        if area == 0 and step > 0 and before != 0 and scan:
            w["zero3"] = True
        if area < 0 <= before and w["neg3"] < 0:
            w["neg3"] = step
        p3 -= 1
        step += 1
    w["steps3"] = step
    if not protect5:
        p5, best, area, step = 0, 0, 0, 0
        scan = min(5, n)
        while scan:
            scan -= 1
            if p5 < f3 - after and area >= 0:
                scan = after
            assert p5 < n
            area += Q - sc[p5]
            if area > best:
                best, f5, w["step5"] = area, p5 + 1, step
            elif area == best and best > 0 and Q != sc[p5]:
                w["tie5"] = True
            p5 += 1
            step += 1
        w["steps5"] = step
    w["f3"], w["f5"] = f3, f5
    return f5, (0 if f3 <= f5 else f3 - f5 + 1), w


def walk_bwa(sc, Q):
    """trim.cpp:675-709"""
    p3 = len(sc) - 1
    f3, area, best, step = p3, 0, 0, 0
    w = dict(step3=-1, tie3=False, zero3=False, neg3=-1, steps3=0, step5=-1, tie5=False, steps5=0)
    while p3 > 0 and area >= 0:
        before = area
        area += Q - sc[p3]
        if area > best:
            best, f3, w["step3"] = area, p3 - 1, step
        elif area == best and best > 0 and Q != sc[p3]:
            w["tie3"] = True
        if area == 0 and step > 0 and before != 0 and p3 > 1:
            w["zero3"] = True
        if area < 0 and w["neg3"] < 0:
            w["neg3"] = step
        p3 -= 1
        step += 1
    w["steps3"], w["f3"], w["f5"] = step, f3, 0
    return 0, f3 + 1, w


def walk_hard(sc, Q, protect5):
    """trim.cpp:629-672"""
    p3 = len(sc) - 1
    f5, f3 = 0, p3
    while p3 > 0:
        if Q < sc[p3]:
            f3 = p3
            break
        p3 -= 1
    if not protect5:
        p5 = 0
        while p5 < p3:
            if Q < sc[p5]:
                f5 = p5
                break
            p5 += 1
    return f5, f3 - f5 + 1, dict(step3=-1, tie3=False, zero3=False, neg3=-1, steps3=len(sc) - 1 - p3, step5=-1, tie5=False, steps5=0, f3=f3, f5=f5, found3=p3 > 0)


_UP = bytes(c if chr(c) in "ACGT" else (c - 32 if chr(c) in "acgt" else ord(".")) for c in range(256))
_PAIRS = [bytes(p) for p in itertools.permutations(b"ACGT", 2)]


def average_quality(q, off):
    """trim.cpp:553-576 in float32"""
    if not q:
        return f32(0)
    v = f32(raw_sum(q)) / f32(len(q)) - f32(off)
    return v if v > f32(0) else f32(0)


def comp_bins(s):
    """trim.cpp:858-875: the six bins (A, T, C, G, N, GC) of a read or window"""
    n = len(s)
    norm = f32(NCOMP_BIN - 1) / f32(n) if n else f32(0)
    a, t, c, g, x = (s.count(u) + s.count(l) for u, l in (b"Aa", b"Tt", b"Cc", b"Gg", b"Nn"))
    ia, it, ic, ig, ix = (int(norm * f32(k)) for k in (a, t, c, g, x))
    return (ia, it, ic, ig, ix, ic + ig)


class Model:
    """One engine's counter block over any number of submissions"""

    def __init__(self, opt, R, in_off):
        self.o, self.R, self.off = opt, R, in_off
        self.lay = layout(R)
        self.C = [0] * self.lay["total"]      # Python ints; the four matrices are added by numpy in block()
        self.mat = {k: np.zeros(self.lay[k][1], np.int64) for k in ("pre_qual", "post_qual", "pre_base", "post_base")}
        self.trace = []

    def add(self, name, i, v=1):
        self.C[self.lay[name][0] + i] += v

    def stat(self, name, v=1):
        self.C[self.lay["filter_stats"][0] + S[name]] += v

    def read(self, s, q):
        """-> (start, len, flags), the masked quality, the post window (a, kept, edited bases) or None"""
        o, off, I = self.o, self.off, Info()
        n = I.n0 = len(s)
        self.stat("TOTAL_COUNT"), self.stat("TOTAL_NUMBER"), self.stat("TOTAL_LENGTH", n)
        q = bytearray(q)
        i = 0
        while i < n and s[i] == 78:           # mask_quality_terminal_N, trim.cpp:1191-1216: upper-case N only
            q[i] = off
            i += 1
        i = n
        while i > 0 and s[i - 1] == 78:
            q[i - 1] = off
            i -= 1
        q = bytes(q)
        sc = scores_of(q, off)                # (throws where update_quality_matrix would, trim.cpp:247)
        I.pre_bin = comp_bins(s)
        for k, b in enumerate(I.pre_bin):
            self.add("pre_comp", b * NCOMP_KIND + k)
        self.add("pre_len_hist", n)
        qb = int(average_quality(q, off))
        self.add("pre_read_qhist", qb), self.add("pre_base_qhist", qb, n)
        a, ln, flags, filt, ok = 0, n, 0, FILT_NONE, True
        if o.trim_5 and not o.qc_only:
            if o.trim_5 > ln:
                ln = 0                        # (offset_5 is left alone, trim.cpp:286-287)
            else:
                a, ln = a + o.trim_5, ln - o.trim_5
        if o.trim_3 and not o.qc_only:
            ln = 0 if o.trim_3 > ln else ln - o.trim_3
        I.pre = ln
        if ln < o.min_read_length or ln == 0:
            self.stat("BASE_LENGTH", ln), self.stat("READ_LENGTH")
            ok, filt = False, FILT_LENGTH_PRE
        I.w = None
        if not o.qc_only and ok:
            win = sc[a:a + ln]
            if o.mode == MODE_HARD:
                c5, kept, I.w = walk_hard(win, o.quality, o.protect_5)
            elif o.mode == MODE_BWA:
                c5, kept, I.w = walk_bwa(win, o.quality)
            else:
                c5, kept, I.w = walk_bwa_plus(win, o.quality, o.protect_5)
            if kept != ln:
                self.stat("BASE_QUAL_TRIM", ln - kept), self.stat("READ_QUAL_TRIM")
                flags |= F_QUAL_TRIMMED
            a, ln = a + c5, kept
            if ln < o.min_read_length or ln == 0:
                self.stat("BASE_LENGTH", ln), self.stat("READ_LENGTH")
                ok, filt = False, FILT_LENGTH_POST
        ws, wq = s[a:a + ln], q[a:a + ln]
        I.npoly = max((len(r) for r in ws.replace(b"N", b"\0").translate(bytes(1 if c == 0 else 32 for c in range(256))).split()), default=0) if b"N" in ws else 0
        if ok and I.npoly >= o.max_num_poly_N:
            self.stat("BASE_NN", ln), self.stat("READ_NN")
            flags |= F_POLY_N_SEEN
            if not o.qc_only:
                ok, filt = False, FILT_POLY_N
        ave = average_quality(wq, off)
        I.qsum = raw_sum(wq) - off * ln
        if ok and ave < f32(o.average_quality):
            self.stat("BASE_AVG_Q", ln), self.stat("READ_AVG_Q")
            ok, filt = False, FILT_AVG_Q
        I.cmax = I.dmax = 0
        I.counts, I.wlen = None, ln
        if ok and ln:
            if o.replace_to_N_q > 0:
                ws = bytes(78 if b == 71 and x < o.replace_to_N_q else b for b, x in zip(ws, sc[a:a + ln]))
            up = ws.translate(_UP)
            I.counts = cnt = [up.count(b) for b in (b"A", b"T", b"G", b"C")]
            dc = [up.count(p) for p in _PAIRS]
            I.cmax, I.dmax = max(cnt), max(dc)
            norm, lc = f32(1.0 / ln), f32(o.low_complexity_cutoff_ratio)
            low = any(f32(c) * norm > lc for c in cnt)
            if not low:
                norm2 = f32(float(norm) * 2.0)
                low = any(f32(c) * norm2 > lc for c in dc)
            if low:
                self.stat("BASE_LOW_COMPLEXITY", ln), self.stat("READ_LOW_COMPLEXITY")
                ok, filt = False, FILT_LOW_COMPLEXITY
        I.bins = None
        if ok:
            self.stat("TOTAL_TRIMMED_LENGTH", ln), self.stat("TOTAL_TRIMMED_NUMBER")
            I.bins = comp_bins(ws)
            for k, b in enumerate(I.bins):
                self.add("post_comp", b * NCOMP_KIND + k)
            self.add("post_len_hist", ln)
            self.add("post_read_qhist", int(ave)), self.add("post_base_qhist", int(ave), ln)
        I.a, I.kept, I.flags, I.filt = (a, ln, flags | F_VALID, filt) if ok else (0, 0, flags, filt)
        self.trace.append(I)
        return (I.a, I.kept, I.flags | (filt << 1)), q, ((a, ln, ws) if ok else None)

    def submit(self, segments):
        """-> [(start, len, flags)] of the submission's reads; QualityError where the reference throws"""
        out, pre_q, pre_s, post_q, post_s, post_row = [], [], [], [], [], []
        for seg in segments:
            for _, s, q in seg:
                res, mq, post = self.read(s, q)
                out.append(res)
                pre_q.append(mq), pre_s.append(s)
                if post:
                    a, ln, ws = post
                    post_q.append(mq[a:a + ln]), post_s.append(ws), post_row.append(a)
        self._matrices("pre", pre_q, pre_s, [0] * len(pre_q))
        self._matrices("post", post_q, post_s, post_row)
        return out

    def _matrices(self, which, quals, seqs, row0):
        """update_quality_matrix / update_base_statistics (trim.cpp:795-857) for many windows at once: position = index in the window + offset_5"""
        lens = np.array([len(x) for x in quals], np.int64)
        if not lens.sum():
            return
        q = np.frombuffer(b"".join(quals), np.int8).astype(np.int64)
        s = np.frombuffer(b"".join(seqs), np.uint8)
        start = np.cumsum(lens) - lens
        pos = np.arange(len(q)) - np.repeat(start, lens) + np.repeat(np.array(row0, np.int64), lens)
        score = np.maximum(q - self.off, 0)
        assert score.max() <= NQ - 1
        ok = pos < self.R
        self.mat[which + "_qual"] += np.bincount(pos[ok] * NQ + score[ok], minlength=self.R * NQ)
        col = np.full(256, -1, np.int64)
        for k, ch in enumerate(b"ATCGN"):
            col[ch] = col[ch | 32] = k
        c = col[s]
        ok &= c >= 0
        self.mat[which + "_base"] += np.bincount(pos[ok] * NBASE + c[ok], minlength=self.R * NBASE)

    def block(self):
        out = np.array(self.C, np.uint64)
        for k, m in self.mat.items():
            out[self.lay[k][0]:self.lay[k][0] + self.lay[k][1]] = m.astype(np.uint64)
        return out


RESULT_DTYPE = np.dtype([("start", "<u2"), ("len", "<u2"), ("flags", "<u2"), ("adapter", "<u2")])


def run_model(case):
    """-> dict(results=[array per submission], counters, error, trace)"""
    m = Model(case.opt(), case.R, case.in_off)
    results = []
    try:
        for sub in case.subs:
            r = np.zeros(sum(len(seg) for seg in sub), RESULT_DTYPE)
            for i, t in enumerate(m.submit(sub)):
                r[i] = t + (0,)
            results.append(r)
    except QualityError:
        return dict(results=None, counters=None, error=E_QUALITY, trace=m.trace)
    return dict(results=results, counters=m.block(), error=0, trace=m.trace)


# ---- the float32 thresholds, for construction and predicates (the model itself judges read by read, above) ----------------------------
_THR = {}


def lc_thr(n, lc, di=False):
    """The smallest count c <= n with float32(c) * norm > lc (norm doubled for transitions), or None"""
    key = (n, float(lc), di)
    if key not in _THR:
        norm = f32(1.0 / n)
        if di:
            norm = f32(float(norm) * 2.0)
        _THR[key] = next((c for c in range(n + 1) if f32(c) * norm > f32(lc)), None)
    return _THR[key]


def lc_thr_exact(n, lc_text, di=False):
    """The smallest count with c / n (2 c / n) > lc in exact arithmetic on the option as it was typed"""
    return int(Fraction(lc_text) * n / (2 if di else 1)) + 1


def avg_pass_sum(n, avg, off):
    """The smallest V = sum(raw - offset) >= 0 with NOT(average_quality < avg) in float32"""
    ok = lambda V: not ((lambda v: v if v > 0 else f32(0))(f32(V + off * n) / f32(n) - f32(off)) < f32(avg))
    lo, hi = 0, 42 * n
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid + 1, hi)
    return lo


def comp_bin_float(n, c):
    return int(f32(NCOMP_BIN - 1) / f32(n) * f32(c))


_LOW_PAIRS = {}


def comp_low_pairs(max_len):
    """(len, count) whose float32 bin lies below floor(10000 count / len)"""
    if max_len not in _LOW_PAIRS:
        _LOW_PAIRS[max_len] = [(n, c) for n in range(1, max_len + 1) for c in range(n + 1) if comp_bin_float(n, c) < 10000 * c // n]
    return _LOW_PAIRS[max_len]


# =====================================================================================================================================
# cases
# =====================================================================================================================================
class TCase:
    """name, the option list (behind -u x -d y), submissions of segments of (id, seq, qual), the edges it claims; R the engine's longest read,
    kernels: per submission the kernel the default setting must report (None: not asserted), exclude: {setting: reason}, hostile: the arenas'
    pads are filled with bytes that must not show, shifts: per submission the device address mod 16 of the arenas' first byte; a hostile
    case and a case with shifts are submitted device-resident (faqcs_submit_device, whose caller owns the pads: device_buffers())"""

    def __init__(self, name, args, subs, claims, R=None, kernels=None, hostile=False, error=False, shifts=None):
        self.name, self.args, self.subs, self.claims = name, [str(a) for a in args], subs, tuple(claims)
        longest = max([len(r[1]) for sub in subs for seg in sub for r in seg] or [0])
        self.R = R or (FAST_READ_LENGTH if longest <= FAST_READ_LENGTH else 4096)
        self.kernels, self.exclude, self.hostile, self.error = kernels, {}, hostile, error
        self.shifts = list(shifts) if shifts is not None else ([0] * len(subs) if hostile else None)
        assert self.shifts is None or (len(self.shifts) == len(subs) and all(0 <= k < 16 for k in self.shifts))
        self._exp = self._ctx = None
        o = self.opt()
        self.in_off = 33 if o.input_quality_offset < 0 else o.input_quality_offset
        self.longest = longest

    def opt(self):
        from faqcs_amd.options import parse_args

        return parse_args(["-u", "x", "-d", "y"] + self.args)

    def expected(self):
        if self._exp is None:
            self._exp = run_model(self)
        return self._exp

    def n_reads(self):
        return sum(len(seg) for sub in self.subs for seg in sub)

    def ctx(self):
        if self._ctx is None:
            self._ctx = Ctx(self)
        return self._ctx


class Ctx:
    """What the predicates look at: the options, the reads and the model's trace, read by read"""

    def __init__(self, case):
        self.case, self.o = case, case.opt()
        self.off = case.in_off
        self.reads = [r for sub in case.subs for seg in sub for r in seg]
        e = case.expected()
        self.error, self.trace = e["error"], e["trace"]
        self.rt = list(zip(self.reads, self.trace))

    def lc_text(self):
        return self.case.args[self.case.args.index("--lc") + 1] if "--lc" in self.case.args else "0.85"


_POOL = np.frombuffer(b"ACGT", np.uint8)[np.random.Generator(np.random.PCG64(20261019)).integers(0, 4, 1 << 16)].tobytes()


def rb(n, salt=0):
    """n bases of a fixed pool: a different stretch for every salt"""
    at = (salt * 7919) % (len(_POOL) - n)
    return _POOL[at:at + n]


def Qs(scores, off=33):
    return bytes(off + x for x in scores)


def rd(seq, qual=None, off=33):
    return (b"@r", bytes(seq), Qs([38] * len(seq), off) if qual is None else bytes(qual))


def one(reads):
    return [[list(reads)]]


EDGES = {}


def edge(name):
    def reg(f):
        EDGES[name] = f
        return f
    return reg


def W(i):
    return i.w or {}


def _inner_end(q):
    """the first base of a read's low tail (the reads of the tail cases are good up to it)"""
    return len(q) - len(q.lstrip(q[:1])) if q else 0


# ---- walk -------------------------------------------------------------------------------------------------------------------------------
for _m, _mode in ((MODE_BWA_PLUS, "bwa_plus"), (MODE_BWA, "bwa"), (MODE_HARD, "hard")):
    edge("walk:%s:every_string_of_1..7_over_three_levels" % _mode)(lambda c, m=_m: c.o.mode == m and not c.o.protect_5 and len({r[2] for r in c.reads if len(r[1]) <= 7}) >= 3 ** 7)
edge("walk:bwa_plus:5trim_off_every_string")(lambda c: c.o.mode == MODE_BWA_PLUS and c.o.protect_5 and len({r[2] for r in c.reads}) >= 3 ** 7 and all(i.a == 0 for i in c.trace))
edge("walk:hard:5trim_off_every_string")(lambda c: c.o.mode == MODE_HARD and c.o.protect_5 and len({r[2] for r in c.reads}) >= 3 ** 7 and all(i.a == 0 for i in c.trace))
for _q in (0, 5, 41):
    edge("walk:q=%d" % _q)(lambda c, q=_q: c.o.quality == q and len(c.reads) >= 3 ** 7)
def _run(q, b, front):
    """the length of the run of byte b at the front (the end) of q"""
    t = q if front else q[::-1]
    return len(t) - len(t.lstrip(bytes([b])))


# (the inputs hold a tail / head of every length 0 .. L, uniformly one below the threshold, and the model cuts what the mode lets it cut of them)
edge("walk:tail_of_every_length_0..L_at_every_row")(lambda c: all(
    {_run(q, c.off + c.o.quality - 1, False) for _, s, q in c.reads if len(s) == L and set(q) <= {c.off + 38, c.off + c.o.quality - 1}} >= set(range(L + 1)) and
    {L - i.kept for (_, s, _), i in c.rt if len(s) == L and i.a == 0 and i.filt in (0, FILT_LENGTH_POST)} >= set(range(1, L - 1)) for L in ROW_LAST))
edge("walk:head_of_every_length_0..L_at_every_row")(lambda c: all(
    {_run(q, c.off + c.o.quality - 1, True) for _, s, q in c.reads if len(s) == L and set(q) <= {c.off + 38, c.off + c.o.quality - 1}} >= set(range(L + 1)) and
    {i.a for (_, s, _), i in c.rt if len(s) == L and i.flags & F_VALID} >= set(range(1, L - 3)) for L in ROW_LAST))
edge("walk:tail_at_threshold_is_not_cut")(lambda c: any(len(s) > 60 and set(q[-50:]) == {c.off + c.o.quality} and i.kept == len(s) for (_, s, q), i in c.rt))
edge("walk:good_base_inside_the_tail_at_1_2_3_64")(lambda c: all(any(len(s) == 304 and _inner_end(q) + d + 5 < 304 and q[_inner_end(q) + d] == c.off + c.o.quality + 2
                                                                      for _, s, q in c.reads) for d in (1, 2, 3, 64)))
edge("walk:two_equal_maxima_first_wins")(lambda c: any(W(i).get("tie3") and W(i)["step3"] >= 0 for i in c.trace) and any(W(i).get("tie5") for i in c.trace))
edge("walk:area_returns_to_0_and_goes_on")(lambda c: any(W(i).get("zero3") and W(i)["steps3"] > 8 for i in c.trace))
edge("walk:stops_two_after_negative")(lambda c: any(W(i).get("neg3", -1) >= 3 and W(i)["steps3"] == W(i)["neg3"] + 3 and len(s) > W(i)["steps3"] + 3 for (_, s, _), i in c.rt))
edge("walk:new_maximum_in_the_two_after_negative")(lambda c: any(0 <= W(i).get("neg3", -1) < W(i)["step3"] and W(i)["steps3"] == W(i)["neg3"] + 3 and len(s) > 20 for (_, s, _), i in c.rt))
for _st in (254, 255, 256, 300):
    edge("walk:maximum_at_step_%d_of_304" % _st)(lambda c, st=_st: c.o.mode == MODE_BWA_PLUS and any(len(s) == 304 and W(i).get("step3") == st for (_, s, _), i in c.rt))
# final_pos_3 = final_pos_5 - 1 cannot be reached: a 3' maximum at base k means a positive step at k, and the 5' walk, which takes base k
# whenever its own maximum could lie at k - 1, adds that step to its area.  What can be reached: below by two or more, equal, one above.
edge("walk:final_pos_3_below_final_pos_5")(lambda c: c.o.mode == MODE_BWA_PLUS and any(i.w and i.w["f3"] < i.w["f5"] for i in c.trace) and
                                           not any(i.w and i.w["f3"] == i.w["f5"] - 1 for i in c.trace))
for _d in (0, 1):
    edge("walk:final_pos_3=final_pos_5%+d" % _d)(lambda c, d=_d: c.o.mode == MODE_BWA_PLUS and any(i.w and i.w["f3"] - i.w["f5"] == d and i.w["f5"] > 0 for i in c.trace))
edge("walk:low_throughout_at_1..12")(lambda c: {len(s) for (_, s, q), i in c.rt if q and max(q) < c.off + c.o.quality} >= set(range(1, 13)))

# ---- ends -------------------------------------------------------------------------------------------------------------------------------
for _d in (-1, 0, 1):
    edge("ends:pre_length=min_L%+d" % _d)(lambda c, d=_d: any(i.pre == c.o.min_read_length + d and (i.filt == FILT_LENGTH_PRE) == (d < 0) for i in c.trace))
    edge("ends:post_length=min_L%+d" % _d)(lambda c, d=_d: any(i.w and i.pre > c.o.min_read_length and i.flags & F_QUAL_TRIMMED and
                                                                 ((i.filt == FILT_LENGTH_POST and d < 0 and _post_len(c, i) == c.o.min_read_length + d) or
                                                                  (d >= 0 and i.kept == c.o.min_read_length + d)) for i in c.trace))
    edge("ends:5end=len%+d" % _d)(lambda c, d=_d: c.o.trim_5 and not c.o.trim_3 and any(c.o.trim_5 == i.n0 + d for i in c.trace))
    edge("ends:3end=len%+d" % _d)(lambda c, d=_d: c.o.trim_3 and not c.o.trim_5 and any(c.o.trim_3 == i.n0 + d for i in c.trace))
    edge("ends:5end+3end=len%+d" % _d)(lambda c, d=_d: c.o.trim_3 and c.o.trim_5 and any(c.o.trim_3 + c.o.trim_5 == i.n0 + d for i in c.trace))
edge("ends:empty_read")(lambda c: any(i.n0 == 0 and i.filt == FILT_LENGTH_PRE for i in c.trace))
edge("ends:read_of_one_base")(lambda c: any(i.n0 == 1 for i in c.trace))
edge("ends:quality_trimmed_then_filtered")(lambda c: {i.filt for i in c.trace if i.flags & F_QUAL_TRIMMED and not i.flags & F_VALID and i.kept == 0} >= {FILT_LENGTH_POST, FILT_POLY_N, FILT_AVG_Q, FILT_LOW_COMPLEXITY})
edge("ends:qc_only_applies_no_ends")(lambda c: c.o.qc_only and c.o.trim_5 and c.o.trim_3 and any(i.flags & F_VALID and i.a == 0 and i.kept == i.n0 for i in c.trace))


def _post_len(c, i):
    return (i.w["f3"] - i.w["f5"] + 1) if i.w["f3"] > i.w["f5"] or c.o.mode != MODE_BWA_PLUS else 0


# ---- ns ---------------------------------------------------------------------------------------------------------------------------------
def _nrun(s, ch, front):
    t = s if front else s[::-1]
    return len(t) - len(t.lstrip(ch))


edge("ns:terminal_N_runs_of_0..5_at_each_end")(lambda c: {(_nrun(s, b"N", True), _nrun(s, b"N", False)) for _, s, _ in c.reads} >= {(a, b) for a in range(6) for b in range(6)})
edge("ns:terminal_n_runs_are_not_masked")(lambda c: {(_nrun(s, b"n", True), _nrun(s, b"n", False)) for _, s, _ in c.reads} >= {(a, b) for a in range(6) for b in range(6)} and
                                          any(i.kept == i.n0 and s[-1:] == b"n" for (_, s, _), i in c.rt))
edge("ns:all_N_read_at_every_row_length")(lambda c: {len(s) for _, s, _ in c.reads if s and s == b"N" * len(s)} >= set(ROW_LENGTHS))
edge("ns:score_above_41_under_a_terminal_N")(lambda c: not c.error and any(s[-1:] == b"N" and q[-1] > c.off + 41 for _, s, q in c.reads) and any(s[:1] == b"N" and q[0] > c.off + 41 for _, s, q in c.reads))
edge("ns:score_above_41_under_a_terminal_n_is_an_error")(lambda c: c.error == E_QUALITY and any(s[-1:] == b"n" and q[-1] > c.off + 41 for _, s, q in c.reads))
for _k in (0, 1, 2, 3, 7):
    edge("ns:-n_%d:longest_run_k-1_k_k+1" % _k)(lambda c, k=_k: c.o.max_num_poly_N == k and not c.o.qc_only and
                                                  {i.npoly for i in c.trace if i.filt in (FILT_NONE, FILT_POLY_N) and (i.filt == FILT_POLY_N) == (i.npoly >= k)} >= {x for x in (k - 1, k, k + 1) if x >= 0})
edge("ns:run_broken_by_n")(lambda c: any(b"NNnN" in s and i.npoly == 2 for (_, s, _), i in c.rt))
edge("ns:two_runs")(lambda c: any(s.count(b"ANNA") + s.count(b"CNNNG") == 2 and i.npoly == 3 for (_, s, _), i in c.rt))
edge("ns:run_shortened_by_a_cut")(lambda c: any(i.flags & F_VALID and i.npoly == c.o.max_num_poly_N - 1 and (b"N" * c.o.max_num_poly_N) in s and i.a + i.kept < i.n0 for (_, s, _), i in c.rt) and
                                  any(i.flags & F_VALID and i.npoly == c.o.max_num_poly_N - 1 and (b"N" * c.o.max_num_poly_N) in s and i.a > 0 for (_, s, _), i in c.rt))
edge("ns:run_starts_at_mC-1_and_mC_of_every_row")(lambda c: all(any(len(s) == hi and s.find(b"NN") == p for _, s, _ in c.reads) for _, hi, C, _, _, _, _ in LDS_ROWS for m in (1, 2) for p in (m * C - 1, m * C)))
edge("ns:run_starts_at_dword_borders")(lambda c: {s.find(b"NN") for _, s, _ in c.reads} >= {3, 4, 7, 8, 63, 64})
edge("ns:qc_only_poly_N_seen_and_valid")(lambda c: c.o.qc_only and any(i.flags & F_POLY_N_SEEN and i.flags & F_VALID for i in c.trace))

# ---- thresholds -------------------------------------------------------------------------------------------------------------------------
# (lengths past 304 bases: trim_filter_accumulate judges from the same tables)
LC_LENGTHS = {"0.2": (15, 30, 60, 120, 240, 255, 480, 510, 960, 1020), "0.4": (15, 30, 60, 120, 240, 255, 480, 510, 960, 1020),
              "0.75": (28, 56, 60, 112, 120, 224, 240, 252, 380, 1020), "0.5": (2, 75, 150, 151, 304)}
LC_DI_LENGTHS = {"0.2": (30, 60, 120, 240, 480, 1020), "0.4": (15, 30, 60, 120, 240, 255, 480, 1020), "0.75": (56, 112, 120, 224, 240, 448), "0.5": (75, 150, 151, 304)}
AVGQ_LENGTHS = tuple(ROW_LENGTHS) + (75, 150, 250)


def _lc_edge(c, di, lengths, need_diff):
    """reads whose commonest base (transition) occurs thr - 1 and thr times at each length; with need_diff the float32 threshold differs from the exact one"""
    lc, text = c.o.low_complexity_cutoff_ratio, c.lc_text()
    for n in lengths:
        t = lc_thr(n, lc, di)
        if t is None or (need_diff and t == lc_thr_exact(n, text, di)):
            return False
        got = {(i.dmax if di else i.cmax, i.filt) for i in c.trace if i.counts and i.wlen == n and i.filt in (FILT_NONE, FILT_LOW_COMPLEXITY)}
        if not ((t - 1, FILT_NONE) in got and (t, FILT_LOW_COMPLEXITY) in got):
            return False
    return True


edge("thr:lc_0.85:base_at_thr-1_and_thr_at_every_length_1..304")(lambda c: c.lc_text() == "0.85" and _lc_edge(c, False, range(1, 305), False))
edge("thr:lc_0.85:transition_at_thr2-1_and_thr2")(lambda c: c.lc_text() == "0.85" and _lc_edge(c, True, range(8, 305, 1), False))
for _lc in ("0.2", "0.4", "0.75"):
    edge("thr:lc_%s:base_threshold_differs_from_exact" % _lc)(lambda c, t=_lc: c.lc_text() == t and _lc_edge(c, False, LC_LENGTHS[t], True))
    edge("thr:lc_%s:transition_threshold_differs_from_exact" % _lc)(lambda c, t=_lc: c.lc_text() == t and _lc_edge(c, True, LC_DI_LENGTHS[t], True))
edge("thr:lc_0.5:base_and_transition")(lambda c: c.lc_text() == "0.5" and _lc_edge(c, False, LC_LENGTHS["0.5"], False) and _lc_edge(c, True, LC_DI_LENGTHS["0.5"], False))
# (at every length the case is about: 1 .. 304 under the default, the listed lengths under the other values)
edge("thr:lc:every_base_and_split_case")(lambda c: all(any(i.filt == filt and i.wlen == n and i.counts[k] == i.cmax == lc_thr(n, c.o.low_complexity_cutoff_ratio) - (filt == FILT_NONE) and
                                                            (s.count(lo) > 0) == split for (_, s, _), i in c.rt if i.counts)
                                                       for n in (range(1, 305) if c.lc_text() == "0.85" else LC_LENGTHS[c.lc_text()]) if (lc_thr(n, c.o.low_complexity_cutoff_ratio) or 0) >= 3  # (a count of 2 can be split)
                                                       for k, lo in enumerate((b"a", b"t", b"g", b"c"))
                                                       for split in (False, True) if not split or k == n % 4 or c.lc_text() != "0.85" for filt in (FILT_NONE, FILT_LOW_COMPLEXITY)))
edge("thr:lc:kept_length_is_not_the_raw_length")(lambda c: any(i.counts and i.flags & F_QUAL_TRIMMED and i.filt == FILT_LOW_COMPLEXITY and
                                                               i.cmax == lc_thr(i.wlen, c.o.low_complexity_cutoff_ratio) and i.wlen < i.n0 for i in c.trace) and
                                                 any(i.flags & F_QUAL_TRIMMED and i.flags & F_VALID and i.cmax == lc_thr(i.kept, c.o.low_complexity_cutoff_ratio) - 1 for i in c.trace))
AVGQ_VALUES = ("25", "12.5", "20.2", "20.1")
# the sweep of --avg_q 0.1 .. 41.0 in steps of 0.1: at 20.2 the float32 rule passes a sum one below the exact one (exact on the float32 value of
# the option) at every length that is a multiple of 5, at 20.1 it wants one more than the exact rule on the option as typed at every multiple of 10
AVGQ_DIFF = {"20.2": ("f32", (75, 105, 150, 250, 305)), "20.1": ("typed", (150, 250))}


def avg_pass_sum_exact(n, text, kind):
    ex = Fraction(text) if kind == "typed" else Fraction(float(f32(float(text))))
    return -((-ex * n) // 1)


for _a in AVGQ_DIFF:
    edge("thr:avg_q_%s:float_threshold_differs_from_exact" % _a)(lambda c, a=_a: abs(c.o.average_quality - float(a)) < 1e-5 and all(
        avg_pass_sum(n, c.o.average_quality, c.off) != avg_pass_sum_exact(n, a, AVGQ_DIFF[a][0]) and
        {(i.qsum - avg_pass_sum(n, c.o.average_quality, c.off), i.filt) for i in c.trace if i.n0 == n} >= {(-1, FILT_AVG_Q), (0, FILT_NONE)} for n in AVGQ_DIFF[a][1]))
for _a in AVGQ_VALUES:
    edge("thr:avg_q_%s:sum_one_below_and_at_the_smallest_passing" % _a)(lambda c, a=_a: abs(c.o.average_quality - float(a)) < 1e-5 and all(
        {(i.qsum - avg_pass_sum(n, c.o.average_quality, c.off), i.filt) for i in c.trace if i.n0 == n} >= {(-1, FILT_AVG_Q), (0, FILT_NONE)} for n in AVGQ_LENGTHS))
edge("thr:avg_q:negative_sum_is_filtered")(lambda c: c.o.average_quality > 0 and any(i.qsum < 0 and i.filt == FILT_AVG_Q for i in c.trace) and any(i.flags & F_VALID for i in c.trace))
edge("thr:avg_q:negative_sum_clamps_to_0")(lambda c: c.o.average_quality == 0 and sum(1 for i in c.trace if i.qsum < 0 and i.flags & F_VALID) >= 4)
edge("thr:quality_bin:sums_k_len-1_and_k_len")(lambda c: all(any(i.n0 == n and i.qsum == k * n + d and i.flags & F_VALID for i in c.trace) for n in (75, 150, 304) for k in (1, 20, 41) for d in (-1, 0)))

edge("thr:replace_to_N_q:a_replaced_G_leaves_the_count_below_thr")(lambda c: c.o.replace_to_N_q > 0 and all(
    any(i.n0 == n and i.flags & F_VALID and s.count(b"G") == lc_thr(n, c.o.low_complexity_cutoff_ratio) == i.cmax + 1 and i.bins[4] > 0 for (_, s, _), i in c.rt) and
    any(i.n0 == n and i.filt == FILT_LOW_COMPLEXITY and s.count(b"G") + s.count(b"g") == lc_thr(n, c.o.low_complexity_cutoff_ratio) == i.cmax and b"g" in s for (_, s, _), i in c.rt)
    for n in (75, 150, 304)))

# ---- composition ------------------------------------------------------------------------------------------------------------------------
edge("comp:every_count_of_A_at_every_length_1..304")(lambda c: len({(i.n0, s.count(b"A")) for (_, s, _), i in c.rt if s.count(b"A") + s.count(b"T") == i.n0}) == 46664)
edge("comp:the_70_pairs_below_the_exact_floor")(lambda c: {(i.n0, s.count(b"A")) for (_, s, _), i in c.rt} >= set(comp_low_pairs(304)) and len(comp_low_pairs(304)) == 70)
# (every one of the 70 pairs with the count on C alone and on G alone; on both at once where two such counts fit into the read)
edge("comp:low_pairs_on_C_G_and_both")(lambda c: all({(s.count(b"C"), s.count(b"G")) for (_, s, _), i in c.rt if i.n0 == n and i.flags & F_VALID} >= ({(k, 0), (0, k)} | ({(k, k)} if 2 * k <= n else set()))
                                                     for n, k in comp_low_pairs(304)) and
                                       all(any(i.n0 == n and i.pre_bin[5] == 2 * comp_bin_float(n, k) < 10000 * 2 * k // n and i.bins == i.pre_bin for i in c.trace) for n, k in comp_low_pairs(304) if 2 * k <= n))
edge("comp:low_pairs_in_the_post_table_on_a_kept_length")(lambda c: all(any(i.flags & F_VALID and i.kept == n < i.n0 and s[:n].count(b"A") == k and i.bins[0] == comp_bin_float(n, k) for (_, s, _), i in c.rt)
                                                                        for n, k in comp_low_pairs(297)))
edge("comp:one_and_two_word_records_in_both_orders")(lambda c: _record_orders(c))


def _record_orders(c):
    wide = [max(len(r[1]) for seg in sub for r in seg) > 256 for sub in c.case.subs]
    pairs = set(zip(wide, wide[1:]))
    return pairs == {(False, True), (True, False), (False, False), (True, True)} and len(c.case.subs) == 8


# ---- chunks -----------------------------------------------------------------------------------------------------------------------------
def _row_of(n):
    return next((r for r in LDS_ROWS if r[0] <= n <= r[1]), None)


def _sub_sizes(c):
    out = {}
    for sub in c.case.subs:
        reads = [r for seg in sub for r in seg]
        row = _row_of(max([len(r[1]) for r in reads] or [0]))
        if row:
            out.setdefault(row[:2], set()).add(len(reads))
    return out


def chunk_sizes(row):
    RPC, NW = row[4], row[5]
    return sorted({1, RPC - 1, RPC, RPC + 1, NW * RPC - 1, NW * RPC + 1, 12 * RPC + 1})


edge("chunks:batch_sizes_at_every_row")(lambda c: all(_sub_sizes(c).get(r[:2], set()) >= set(chunk_sizes(r)) for r in LDS_ROWS))


def _chunks(c):
    """[(row, [reads of the chunk])] of every submission"""
    for sub in c.case.subs:
        reads = [r for seg in sub for r in seg]
        row = _row_of(max([len(r[1]) for r in reads] or [0]))
        if row:
            for k in range(0, len(reads), row[4]):
                yield row, reads[k:k + row[4]]


def _rows_with(c, pred):
    return {row[:2] for row, ch in _chunks(c) if len(ch) == row[4] and pred(row, ch)}


def _padded_chunks(c):
    """[(row, [(read, Info)])] of the chunks trim_lds stages as padded rows, by the kernel's own condition (issue_loads: rows_): a full chunk whose
    reads all have the length of the first, a multiple of 32 that is not 0 and not above PADLEN = C * LPR / 32 * 32"""
    at = 0
    for sub in c.case.subs:
        n = sum(len(seg) for seg in sub)
        rt = c.rt[at:at + n]
        at += n
        row = _row_of(max([len(r[1]) for r, _ in rt] or [0]))
        if row:
            RPC, padlen = row[4], row[2] * row[3] // 32 * 32
            for k in range(0, n, RPC):
                ch = rt[k:k + RPC]
                L = len(ch[0][0][1])
                if len(ch) == RPC and L % 32 == 0 and 0 < L <= padlen and all(len(r[1]) == L for r, _ in ch):
                    yield row, ch


def _padded_rows_meet(c):
    """per row a chunk of padded rows with a walk that cuts a tail and one that cuts a head, an N, a terminal N, and reads that the poly-N rule and
    the low-complexity filter take after counting (the take-back pass)"""
    rows = set()
    for row, ch in _padded_chunks(c):
        if (any(i.flags & F_VALID and i.a == 0 and i.kept < i.n0 for _, i in ch) and any(i.flags & F_VALID and i.a > 0 for _, i in ch) and
                any(r[1][:1] == b"N" and r[1][-1:] == b"N" for r, _ in ch) and {i.filt for _, i in ch} >= {FILT_NONE, FILT_POLY_N, FILT_LOW_COMPLEXITY}):
            rows.add(row[:2])
    return rows == ALL_ROWS


ALL_ROWS = {r[:2] for r in LDS_ROWS}
edge("chunks:chunk_of_empty_reads")(lambda c: _rows_with(c, lambda row, ch: all(len(r[1]) == 0 for r in ch)) == ALL_ROWS)
edge("chunks:empty_read_first_and_last")(lambda c: _rows_with(c, lambda row, ch: len(ch[0][1]) == 0 and len(ch[-1][1]) == 0 and len(ch[1][1]) > 0) == ALL_ROWS)
edge("chunks:padded_rows_at_every_row")(_padded_rows_meet)
# (one odd read makes the chunk a span again: the chunks either side of the padded rows)
edge("chunks:odd_read_in_slot_0_of_an_equal_length_chunk")(lambda c: _rows_with(c, lambda row, ch: len({len(r[1]) for r in ch[1:]}) == 1 and len(ch[1][1]) % 32 == 0 and len(ch[0][1]) != len(ch[1][1])) == ALL_ROWS and
                                                           {row[:2] for row, _ in _padded_chunks(c)} == ALL_ROWS)
edge("chunks:odd_read_in_the_last_slot_of_an_equal_length_chunk")(lambda c: _rows_with(c, lambda row, ch: len({len(r[1]) for r in ch[:-1]}) == 1 and len(ch[0][1]) % 32 == 0 and len(ch[-1][1]) != len(ch[0][1])) == ALL_ROWS and
                                                                  {row[:2] for row, _ in _padded_chunks(c)} == ALL_ROWS)
edge("chunks:every_arena_offset_mod_16")(lambda c: c.case.shifts is None and len(c.case.subs) >= 16 * 6 and
                                         {(max(len(r[1]) for r in sub[0]), len(sub[0][0][1]) % 16) for sub in c.case.subs} >= {(hi, k) for hi in ROW_LAST for k in range(16)})
edge("chunks:every_device_address_mod_16")(lambda c: c.case.shifts is not None and
                                           {(max(len(r[1]) for r in sub[0]), k) for sub, k in zip(c.case.subs, c.case.shifts)} >= {(hi, k) for hi in ROW_LAST + [TFA_FIRST] for k in range(16)})
# (the pads are the test's own device memory: the arena's first read starts behind them and its last read ends in front of them, with a low head / tail that
# the walks enter and, in every other submission, with terminal N runs that the mask follows to the arena's edge)
edge("chunks:hostile_padding")(lambda c: c.case.hostile and c.case.shifts is not None and all(
    any(max(len(r[1]) for r in sub[0]) == hi and len(sub[0][0][1]) > 0 and len(sub[0][-1][1]) > 0 and (sub[0][0][1][:1] == b"N") == n and (sub[0][-1][1][-1:] == b"N") == n for sub in c.case.subs)
    for hi in ROW_LAST + [TFA_FIRST] for n in (True, False)) and any(i.a > 0 for i in c.trace) and any(i.flags & F_VALID and i.a + i.kept < i.n0 for i in c.trace))
edge("chunks:one_long_read_among_one_base_reads")(lambda c: c.case.kernels and [max(len(r[1]) for r in sub[0]) for sub in c.case.subs] == ROW_LENGTHS and
                                                  all(sorted(len(r[1]) for r in sub[0])[-2] == 1 for sub in c.case.subs))
edge("chunks:segment_boundaries_inside_a_chunk")(lambda c: all(any(len(sub) > 3 and _row_of(max(len(r[1]) for seg in sub for r in seg))[:2] == row and
                                                                   any(sum(len(x) for x in sub[:k]) % _row_of(max(len(r[1]) for seg in sub for r in seg))[4] for k in range(1, len(sub)))
                                                                   for sub in c.case.subs) for row in ALL_ROWS))

# ---- bytes ------------------------------------------------------------------------------------------------------------------------------
def _qbyte_places(c, b):
    """where byte b occurs as a quality: first base, last base, inside / outside the kept window"""
    out = set()
    for (_, s, q), i in c.rt:
        for p in [k for k, x in enumerate(q) if x == b]:
            if s[p] == 78:
                continue
            out.add("first" if p == 0 else "last" if p == len(q) - 1 else "")
            if i.flags & F_VALID:
                out.add("inside" if p in (i.a, i.a + i.kept - 1) else "outside" if p in (i.a - 1, i.a + i.kept) else "")
    return out


def _bad_byte_places(c, b):
    """where byte b, a score above 41, lies in the reads that hold it: on the first base, on the last, or outside the window that the walk keeps of the read
    when the byte is a score of 0 instead (and no other byte of the case is above offset + 41)"""
    out = set()
    for _, s, q in c.reads:
        if any(x < 128 and x > c.off + 41 and x != b for x in q):
            return set()
        for p in [k for k, x in enumerate(q) if x == b]:
            q0 = bytearray(q)
            q0[p] = c.off
            f5, kept, _ = walk_bwa_plus(scores_of(bytes(q0), c.off), c.o.quality, c.o.protect_5)
            out.add("first" if p == 0 else "last" if p == len(q) - 1 else "outside" if not f5 <= p < f5 + kept else "inside")
    return out


for _off in (33, 64):
    edge("bytes:ascii_%d:quality_bytes_at_the_window_edges" % _off)(lambda c, off=_off: c.off == off and all(
        _qbyte_places(c, b) >= {"first", "last", "inside", "outside"} for b in (off - 1, off, off + 41, 0x00, 0x80, 0xFF)))
for _off in (33, 64):
    edge("bytes:ascii_%d:quality_bytes_next_to_a_walked_window" % _off)(lambda c, off=_off: c.off == off and not c.o.trim_5 and all(
        _qbyte_places(c, b) >= {"first", "last", "outside"} for b in (off - 1, off, 0x00, 0x80, 0xFF)) and _qbyte_places(c, off + 41) >= {"first", "last", "inside"})
edge("bytes:out_ascii_64")(lambda c: c.o.output_quality_offset == 64 and c.off == 33 and any(i.flags & F_VALID for i in c.trace))
for _where in ("first", "last", "outside"):
    for _name in ("offset+42", "0x7F"):
        edge("bytes:%s_at_%s_is_an_error" % (_name, _where))(lambda c, w=_where, nm=_name: c.error == E_QUALITY and _bad_byte_places(c, c.off + 42 if nm == "offset+42" else 0x7F) == {w})
edge("bytes:every_byte_as_a_base")(lambda c: {s[20] for _, s, _ in c.reads if len(s) > 40} == set(range(256)))
edge("bytes:high_byte_in_the_first_and_last_read_of_a_chunk")(lambda c: any(max(ch[0][1]) >= 0x80 and max(ch[-1][1]) >= 0x80 for row, ch in _chunks(c) if len(ch) == row[4]))
edge("bytes:high_byte_in_a_read_vetoed_after_counting")(lambda c: any(max(s or b"\0") >= 0x80 and i.filt in (FILT_LOW_COMPLEXITY, FILT_AVG_Q, FILT_POLY_N) for (_, s, _), i in c.rt))

# ---- long -------------------------------------------------------------------------------------------------------------------------------
LONG_LC = {"0.2": (1920, 2040, 4080), "0.75": (1516, 1520, 1620)}        # kept lengths past 1 024 where the float32 base threshold is not the exact one (seeded search, fixed)
LONG_TAILS = (63, 64, 65, 127, 128, 129)
for _lc in LONG_LC:
    edge("long:lc_%s:base_threshold_differs_from_exact" % _lc)(lambda c, t=_lc: c.lc_text() == t and c.case.longest > 1024 and _lc_edge(c, False, LONG_LC[t], True))
edge("long:avg_q_25:sum_one_below_and_at_the_smallest_passing")(lambda c: c.case.longest > 1024 and all(
    {(i.qsum - avg_pass_sum(n, c.o.average_quality, c.off), i.filt) for i in c.trace if i.n0 == n} >= {(-1, FILT_AVG_Q), (0, FILT_NONE)} for n in (1025, 2049, 4096)))
LONG_AVGQ_DIFF = (1025, 2050, 4095)     # multiples of 5: the float32 rule of --avg_q 20.2 passes a sum one below the exact one
edge("long:avg_q_20.2:float_threshold_differs_from_exact")(lambda c: c.case.longest > 1024 and abs(c.o.average_quality - 20.2) < 1e-5 and all(
    avg_pass_sum(n, c.o.average_quality, c.off) != avg_pass_sum_exact(n, "20.2", "f32") and
    {(i.qsum - avg_pass_sum(n, c.o.average_quality, c.off), i.filt) for i in c.trace if i.n0 == n} >= {(-1, FILT_AVG_Q), (0, FILT_NONE)} for n in LONG_AVGQ_DIFF))
LONG_COMP_BELOW = ((1060, 53), (1060, 106), (1075, 215), (1075, 387), (1090, 109), (1098, 549), (1098, 1098))   # float32 bin below floor(10000 count / len) ...
LONG_COMP_ABOVE = ((1059, 989), (1201, 1057), (1207, 1007))                                                       # ... and above it (never up to 304 bases)
edge("long:composition_bins_below_the_exact_floor")(lambda c: c.case.longest > 1024 and sum(1 for (_, s, _), i in c.rt if i.n0 > 1024 and i.pre_bin[0] < 10000 * s.count(b"A") // i.n0) >= len(LONG_COMP_BELOW))
edge("long:composition_bins_above_the_exact_floor")(lambda c: c.case.longest > 1024 and sum(1 for (_, s, _), i in c.rt if i.n0 > 1024 and i.pre_bin[0] > 10000 * s.count(b"A") // i.n0) >= len(LONG_COMP_ABOVE))
edge("long:tails_of_63..129_low_bases")(lambda c: c.case.longest > 1024 and {i.n0 - i.kept for i in c.trace if i.a == 0 and i.n0 > 1024} >= set(LONG_TAILS) and
                                        {i.a for i in c.trace if i.n0 > 1024} >= set(LONG_TAILS))


# =====================================================================================================================================
# builders
# =====================================================================================================================================
WALK_MODES = {"bwa_plus": [], "bwa_plus_5off": ["--5trim_off"], "bwa": ["--mode", "BWA"], "hard": ["--mode", "HARD"], "hard_5off": ["--mode", "HARD", "--5trim_off"]}
WALK_BASE = ["--min_L", "1", "--lc", "1.0"]


def walk_cases():
    C = []
    for mname, margs in WALK_MODES.items():
        for Q in (5, 0, 41):
            levels = (max(Q - 2, 0), Q, min(Q + 2, 41))
            reads = [rd(rb(n, n), Qs(t)) for n in range(1, 8) for t in itertools.product(levels, repeat=n)]
            mode = mname.split("_5off")[0]
            claims = ["walk:q=%d" % Q]
            if Q == 5:
                claims.append("walk:%s:5trim_off_every_string" % mode if "5off" in mname else "walk:%s:every_string_of_1..7_over_three_levels" % mode)
                if mname == "bwa_plus":
                    claims += ["walk:final_pos_3_below_final_pos_5", "walk:final_pos_3=final_pos_5+0", "walk:final_pos_3=final_pos_5+1"]
            C.append(TCase("walk_all7_%s_q%d" % (mname, Q), WALK_BASE + margs + ["-q", Q], one(reads), claims))
    Q = 5
    for mname in ("bwa_plus", "bwa", "hard"):
        subs = []
        for L in ROW_LAST:
            reads = []
            for t in range(L + 1):
                for low, good in ((Q, None), (Q - 1, None), (Q - 1, 1), (Q - 1, 2), (Q - 1, 3), (Q - 1, 64)):
                    sc = [38] * (L - t) + [low] * t
                    if good is not None and t > good:
                        sc[L - t + good] = Q + 2       # one good base at distance `good` from the tail's inner end
                    reads.append(rd(rb(L, t), Qs(sc)))
            subs.append([reads])
        claims = ["walk:tail_of_every_length_0..L_at_every_row", "walk:tail_at_threshold_is_not_cut"]
        if mname == "bwa_plus":
            claims += ["walk:good_base_inside_the_tail_at_1_2_3_64"] + ["walk:maximum_at_step_%d_of_304" % s for s in (254, 255, 256, 300)]
        C.append(TCase("walk_tails_%s" % mname, WALK_BASE + WALK_MODES[mname], subs, claims))
    for mname in ("bwa_plus", "hard", "bwa_plus_5off"):
        subs = []
        for L in ROW_LAST:
            reads = []
            for t in range(L + 1):
                for low, good in ((Q, None), (Q - 1, None), (Q - 1, 1), (Q - 1, 2), (Q - 1, 3), (Q - 1, 64)):
                    sc = [low] * t + [38] * (L - t)
                    if good is not None and t > good:
                        sc[t - 1 - good] = Q + 2
                    reads.append(rd(rb(L, t + 1000), Qs(sc)))
            subs.append([reads])
        C.append(TCase("walk_heads_%s" % mname, WALK_BASE + WALK_MODES[mname], subs, ["walk:head_of_every_length_0..L_at_every_row"] if "5off" not in mname else []))
    # deltas Q - score from the read's end inwards (tail) and from its start (head); the middle is good
    special = {"two_equal_maxima": [1, -1, 1, -9], "returns_to_0_and_goes_on": [1, -1, 0, 0, 0, 0, 0, 0, 2, -9], "stops_two_after_negative": [1, 0, 0, -5, 1, 1, 5, 5, 5],
               "new_maximum_two_after_negative": [1, -2, 0, 3, -9, 5], "recovers_within_two": [2, -3, 1, 1, 4, -9]}
    for mname in ("bwa_plus", "bwa"):
        reads = []
        for L in (40, 304):
            for d in special.values():
                sc = [38] * L
                for k, x in enumerate(d):
                    sc[L - 1 - k] = Q - x
                reads.append(rd(rb(L, 7), Qs(sc)))
                sc = [38] * L
                for k, x in enumerate(d):
                    sc[k] = Q - x
                reads.append(rd(rb(L, 8), Qs(sc)))
        reads += [rd(rb(n, 9), Qs([Q - 1 - (k % 2) for k in range(n)])) for n in range(1, 13)]
        claims = ["walk:area_returns_to_0_and_goes_on", "walk:low_throughout_at_1..12"]
        claims += ["walk:stops_two_after_negative", "walk:two_equal_maxima_first_wins", "walk:new_maximum_in_the_two_after_negative"] if mname == "bwa_plus" else []
        C.append(TCase("walk_special_%s" % mname, WALK_BASE + WALK_MODES[mname], one(reads), claims))
    return C


def with_fillers(reads, salt=0):
    """the reads once per row: one submission each, behind a good read of the row's last length (and of 305 bases: trim_filter_accumulate)"""
    return [[[rd(rb(hi, salt + hi))] + list(reads)] for hi in ROW_LAST + [TFA_FIRST]]


def low_tail(n_good, n_low, salt=0, seq=None):
    return rd(seq or rb(n_good + n_low, salt), Qs([38] * n_good + [2] * n_low))


def ends_cases():
    C = []
    reads = [rd(rb(n, n)) for n in (0, 1, 9, 10, 11)] + [low_tail(k, 14 - k, k) for k in (9, 10, 11)] + [low_tail(k, 3, k) for k in (0, 1)]
    C.append(TCase("ends_min_L_10", ["--min_L", "10"], with_fillers(reads), ["ends:pre_length=min_L%+d" % d for d in (-1, 0, 1)] + ["ends:post_length=min_L%+d" % d for d in (-1, 0, 1)] +
                   ["ends:empty_read", "ends:read_of_one_base"]))
    lens = [rd(rb(n, n)) for n in (0, 1, 19, 20, 21)]
    C.append(TCase("ends_5end_20", ["--min_L", "1", "--5end", "20"], with_fillers(lens), ["ends:5end=len%+d" % d for d in (-1, 0, 1)]))
    C.append(TCase("ends_3end_20", ["--min_L", "1", "--3end", "20"], with_fillers(lens), ["ends:3end=len%+d" % d for d in (-1, 0, 1)]))
    C.append(TCase("ends_5end_8_3end_12", ["--min_L", "1", "--5end", "8", "--3end", "12"], with_fillers(lens), ["ends:5end+3end=len%+d" % d for d in (-1, 0, 1)]))
    C.append(TCase("ends_5end_8_3end_12_qc_only", ["--min_L", "1", "--5end", "8", "--3end", "12", "--qc_only"], with_fillers(lens), ["ends:qc_only_applies_no_ends"]))
    # trimmed by the walk, then taken by a later filter: the length, the poly-N run, the average (a window of scores 10 under --avg_q 11), the commonest base
    trimmed = [low_tail(5, 30, 1), low_tail(40, 9, 2, rb(20, 2) + b"NN" + rb(27, 3)), rd(rb(49, 4), Qs([10] * 40 + [2] * 9)), low_tail(40, 9, 5, b"A" * 49)]
    args = ["--min_L", "10", "--avg_q", "11"]
    C.append(TCase("ends_trimmed_then_filtered", args, with_fillers(trimmed), ["ends:quality_trimmed_then_filtered"]))
    C.append(TCase("ends_trimmed_then_filtered_qc_only", args + ["--qc_only"], with_fillers(trimmed), []))
    return C


def ns_cases():
    C = []
    Q = 5

    def ends(ch):
        # N runs of 0 .. 5 at each end under scores of 41, low bases inwards of them: masked, the walk goes through them into the low bases
        out = []
        for a in range(6):
            for b in range(6):
                s = ch * a + rb(40 - a - b, 10 * a + b) + ch * b
                out.append(rd(s, Qs([41] * a + [2] * 4 + [38] * (32 - a - b) + [2] * 4 + [41] * b)))
        return out
    for hi in (52, 152, 304):
        C.append(TCase("ns_terminal_runs_%d" % hi, ["--min_L", "1", "-n", "9"], [[[rd(rb(hi, hi))] + ends(b"N") + ends(b"n")]], ["ns:terminal_N_runs_of_0..5_at_each_end", "ns:terminal_n_runs_are_not_masked"]))
    C.append(TCase("ns_all_N", ["--min_L", "1", "-n", "2000"], [[[rd(b"N" * n, Qs([30] * n)), rd(rb(n, n)), rd(b"N" * n, Qs([30] * n))]] for n in ROW_LENGTHS], ["ns:all_N_read_at_every_row_length"]))
    hot = [rd(b"N" + rb(38, 1) + b"N", Qs([60] + [38] * 38 + [60])), rd(b"NN" + rb(37, 1) + b"N", bytes([0x7F, 0x7E]) + Qs([38] * 37) + bytes([0x7F]))]
    C.append(TCase("ns_score_above_41_under_N", ["--min_L", "1"], with_fillers(hot), ["ns:score_above_41_under_a_terminal_N"]))
    C.append(TCase("ns_score_above_41_under_n", ["--min_L", "1"], one([rd(rb(60, 1)), rd(b"N" + rb(38, 1) + b"n", Qs([60] + [38] * 38 + [60]))]), ["ns:score_above_41_under_a_terminal_n_is_an_error"], error=True))
    for k in (0, 1, 2, 3, 7):
        for qc in (False, True):
            reads = []
            for run in sorted({max(k - 1, 0), k, k + 1, 1}):
                reads.append(rd(rb(20, run) + b"N" * run + rb(20, run + 1)))
            reads += [rd(rb(10, 3) + b"NNnN" + rb(20, 4)), rd(rb(10, 5) + b"ANNA" + rb(9, 6) + b"CNNNG" + rb(9, 7))]
            if k >= 2:  # a run of k bases that the 3' walk (the 5' walk) shortens to k - 1: the cut falls inside the run, whose scores are low beyond it
                reads.append(rd(rb(30, 8) + b"N" * k + rb(9, 9), Qs([38] * (30 + k - 1) + [2] * 10)))
                reads.append(rd(rb(9, 8) + b"N" * k + rb(30, 9), Qs([2] * 10 + [38] * (30 + k - 1))))
            claims = (["ns:qc_only_poly_N_seen_and_valid"] if qc else ["ns:-n_%d:longest_run_k-1_k_k+1" % k] + (["ns:run_shortened_by_a_cut"] if k >= 2 else [])) + \
                (["ns:run_broken_by_n", "ns:two_runs"] if k == 7 else [])
            C.append(TCase("ns_poly_n%d%s" % (k, "_qc_only" if qc else ""), ["--min_L", "1", "-n", k] + (["--qc_only"] if qc else []), with_fillers(reads), claims))
    subs = []
    for _, hi, Cc, _, _, _, _ in LDS_ROWS:
        at = sorted({m * Cc - 1 for m in (1, 2)} | {m * Cc for m in (1, 2)} | {3, 4, 7, 8} | ({63, 64} if hi >= 76 else set()))
        subs.append([[rd(rb(p, p) + b"NN" + rb(hi - p - 2, p + 1)) for p in at if p + 2 < hi] + [rd(rb(70, 1)[:63] + b"NN" + rb(5, 2)), rd(rb(64, 3) + b"NN" + rb(5, 4))]])
    C.append(TCase("ns_run_positions", ["--min_L", "1", "-n", "2"], subs, ["ns:run_starts_at_mC-1_and_mC_of_every_row", "ns:run_starts_at_dword_borders"]))
    return C


def blocks_read(n, counts, letters=b"ATGC", filler=b"R", split=None):
    """A read of n bases: counts[k] copies of letters[k] in blocks (one transition between two blocks), `filler` for the rest; split: the block of
    that letter alternates upper and lower case ... in blocks too, so no transition is added"""
    s = b""
    for k, c in enumerate(counts):
        ch = letters[k:k + 1]
        s += (ch * (c - c // 2) + ch.lower() * (c // 2)) if split == k else ch * c
    assert len(s) <= n, (n, counts)
    return s + filler * (n - len(s))


def lc_reads(n, lc, letter, split=False, tail=0):
    """two reads of kept length n: the commonest base (A T G C by `letter`) thr - 1 and thr times, the others at most thr - 2 times"""
    t = lc_thr(n, lc)
    out = []
    if t is None or t < 1:
        return out
    for c in (t - 1, t):
        if c > n:
            continue
        rest, counts = n - c, [0, 0, 0, 0]
        counts[letter] = c
        for k in range(4):
            if k != letter:
                counts[k] = min(max(c - 2, 0) if c == t - 1 else max(t - 2, 0), rest, max(n // 8, 1))
                rest -= counts[k]
        s = blocks_read(n, counts, split=letter if split else None)
        out.append(rd(s + rb(tail, 1), Qs([38] * n + [2] * tail)))
    return out


def di_reads(n, lc, tail=0):
    """two reads of kept length n: the transition AT thr2 - 1 and thr2 times and no base at thr"""
    t2, t = lc_thr(n, lc, True), lc_thr(n, lc)
    out = []
    if t2 is None or t2 < 2 or t is None:
        return out
    for k in (t2 - 1, t2):
        s = b"AT" * k
        if len(s) > n or k >= t:
            continue
        rest = n - len(s)
        c = min(rest, max(min(t - 2, n // 8), 0))
        s += b"C" * c + b"R" * (rest - c)
        out.append(rd(s + rb(tail, 2), Qs([38] * n + [2] * tail)))
    return out


def threshold_cases():
    C = []
    base = ["--mode", "BWA", "--min_L", "1", "-n", "2000"]   # (BWA: BWA_plus leaves nothing of a read of one base)
    subs = []
    for lo, hi in [r[:2] for r in LDS_ROWS]:
        reads = []
        for n in range(lo, hi + 1):
            for letter in range(4):
                reads += lc_reads(n, f32(0.85), letter)
            reads += lc_reads(n, f32(0.85), n % 4, split=True) + di_reads(n, f32(0.85))
        subs.append([reads])
    C.append(TCase("thr_lc_default_every_length", base, subs, ["thr:lc_0.85:base_at_thr-1_and_thr_at_every_length_1..304", "thr:lc_0.85:transition_at_thr2-1_and_thr2", "thr:lc:every_base_and_split_case"]))
    for text in ("0.5", "0.2", "0.4", "0.75"):
        lc = f32(float(text))
        reads = []
        for n in sorted(set(LC_LENGTHS[text]) | set(LC_DI_LENGTHS[text])):
            for letter in range(4):
                reads += lc_reads(n, lc, letter) + lc_reads(n, lc, letter, split=True)
            reads += di_reads(n, lc)
            if n <= 290:
                reads += lc_reads(n, lc, 0, tail=9) + di_reads(n, lc, tail=9)
        subs = [[[r for r in reads if lo <= len(r[1]) <= hi]] for lo, hi in [r[:2] for r in LDS_ROWS] + [(TFA_FIRST, 512), (513, FAST_READ_LENGTH)]]
        claims = ["thr:lc_0.5:base_and_transition"] if text == "0.5" else ["thr:lc_%s:base_threshold_differs_from_exact" % text, "thr:lc_%s:transition_threshold_differs_from_exact" % text]
        C.append(TCase("thr_lc_%s" % text, base + ["--lc", text], [s for s in subs if s[0]], claims + ["thr:lc:kept_length_is_not_the_raw_length", "thr:lc:every_base_and_split_case"]))
    for text in AVGQ_VALUES:
        avg = float(f32(float(text)))
        subs = []
        for n in AVGQ_LENGTHS:
            V = avg_pass_sum(n, avg, 33)
            reads = []
            for v in (V - 1, V, V + 1):
                sc = [v // n + (1 if k < v % n else 0) for k in range(n)]
                reads.append(rd(rb(n, v), Qs(sc)))
            subs.append([reads])
        C.append(TCase("thr_avg_q_%s" % text, base + ["--lc", "1.0", "-q", "0", "--avg_q", text], subs, ["thr:avg_q_%s:sum_one_below_and_at_the_smallest_passing" % text] +
                       (["thr:avg_q_%s:float_threshold_differs_from_exact" % text] if text in AVGQ_DIFF else [])))
    # bytes below the offset (--ascii 64, bytes from 33 up): the trimmers clamp them to 0, the average does not; it clamps its result
    reads = [rd(rb(n, n), bytes([40] * (n - 5) + [64 + 30] * 5)) for n in (20, 75, 150, 304)] + [rd(rb(60, 1), Qs([30] * 60, 64))]
    C.append(TCase("thr_avg_q_negative_sum_filtered", base + ["-q", "0", "--ascii", "64", "--avg_q", "5"], one(reads), ["thr:avg_q:negative_sum_is_filtered"]))
    C.append(TCase("thr_avg_q_negative_sum", base + ["-q", "0", "--ascii", "64"], one(reads), ["thr:avg_q:negative_sum_clamps_to_0"]))
    # --replace_to_N_q 15: an upper-case G with a score below 15 counts as N in the low-complexity test and in the post tables, a lower-case g does not
    reads = []
    for n in (75, 150, 304):
        r = lc_reads(n, f32(0.85), 2)[1]
        at = r[1].index(b"G") + 3
        for ch, score in ((b"G", 14), (b"G", 15), (b"g", 14)):
            reads.append(rd(r[1][:at] + ch + r[1][at + 1:], Qs([38] * at + [score] + [38] * (n - at - 1))))
    C.append(TCase("thr_replace_to_N_q", base + ["--replace_to_N_q", "15"], [[[r for r in reads if len(r[1]) == n]] for n in (75, 150, 304)], ["thr:replace_to_N_q:a_replaced_G_leaves_the_count_below_thr"]))
    reads = []
    for n in (75, 150, 304):
        for k in (1, 20, 41):
            for v in (k * n - 1, k * n):
                reads.append(rd(rb(n, v), Qs([v // n + (1 if j < v % n else 0) for j in range(n)])))
    C.append(TCase("thr_quality_bin_truncation", base + ["-q", "0"], one(reads), ["thr:quality_bin:sums_k_len-1_and_k_len"]))
    return C


def composition_cases():
    C = []
    base = ["--min_L", "1", "--lc", "1.0", "-n", "2000"]
    # row by row on one engine, the 253 .. 304 row in two halves behind the first row: one-word records (reads up to 256 bases) and two-word records
    # follow each other in all four orders.  (The GPU test syncs behind every submission, and faqcs_sync folds what is pending: composition_histogram on
    # the compute stream folds every row's records, one-word or two-word, at once -- no launch folds or hands on the records of the one before it here;
    # the launches that do are the unsynced schedules of tests/submit_edges.py.)  The small last submission is one more launch behind the widest rows
    order = [LDS_ROWS[0][:2], (253, 280), (281, 304)] + [r[:2] for r in LDS_ROWS[1:5]]
    subs = [[[rd(b"A" * c + b"T" * (n - c)) for n in range(lo, hi + 1) for c in range(n + 1)]] for lo, hi in order]
    subs.append([[rd(rb(30, 1))]])
    C.append(TCase("comp_every_count_of_A", base, subs, ["comp:every_count_of_A_at_every_length_1..304", "comp:the_70_pairs_below_the_exact_floor", "comp:one_and_two_word_records_in_both_orders"]))
    low = comp_low_pairs(304)
    reads = []
    for n, k in low:
        reads += [rd(b"C" * k + b"T" * (n - k)), rd(b"G" * k + b"A" * (n - k))]
        if 2 * k <= n:
            reads.append(rd(b"C" * k + b"G" * k + b"a" * (n - 2 * k)))
    C.append(TCase("comp_low_pairs_on_C_and_G", base, [[[r for r in reads if lo <= len(r[1]) <= hi]] for lo, hi in [r[:2] for r in LDS_ROWS] if any(lo <= len(r[1]) <= hi for r in reads)] + [[[rd(rb(30, 1))]]],
                   ["comp:low_pairs_on_C_G_and_both"]))
    reads = [rd(b"A" * k + b"T" * (n - k) + rb(7, n), Qs([38] * n + [2] * 7)) for n, k in low if n + 7 <= 304]
    C.append(TCase("comp_low_pairs_post_trim", base, [[[r for r in reads if lo <= len(r[1]) <= hi]] for lo, hi in [r[:2] for r in LDS_ROWS] if any(lo <= len(r[1]) <= hi for r in reads)] + [[[rd(rb(30, 1))]]],
                   ["comp:low_pairs_in_the_post_table_on_a_kept_length"]))
    return C


def ragged(n, hi, salt):
    """n reads of 0 .. hi bases (the first of hi bases), scores with low stretches at either end"""
    out = []
    for k in range(n):
        L = hi if k == 0 else (k * 37 + salt * 11) % (hi + 1)
        sc = [20 + (j * 7 + k) % 22 for j in range(L)]
        t, h = (k * 5) % 9, (k * 3) % 7
        sc[L - t:] = [2] * len(sc[L - t:]) if t else sc[L:]
        sc[:h] = [3] * len(sc[:h])
        s = bytearray(rb(L, salt + k))
        if k % 5 == 0 and L > 4:
            s[L // 2] = 78
        out.append(rd(bytes(s), Qs(sc)))
    return out


def padded_mix(L, n):
    """n reads of L bases each for one chunk of padded rows: low tails, low heads, both, an N inside, terminal Ns over high scores and low bases inwards of
    them, a run of N for the poly-N rule and a read of one letter for the low-complexity filter (both counted first and taken back)"""
    out = []
    for k in range(n):
        s, sc = bytearray(rb(L, 40 + k)), [25 + (j * 5 + k) % 17 for j in range(L)]
        t = 1 + k % 6
        kind = k % 8
        if kind in (0, 2):
            sc[L - t:] = [2] * t
        if kind in (1, 2):
            sc[:t] = [3] * t
        if kind == 3:
            s[L // 2] = 78
        if kind == 4:
            s[:2], s[L - 1:] = b"NN", b"N"
            sc[:2], sc[L - 1:], sc[2:5], sc[L - 4:L - 1] = [41] * 2, [41], [2] * 3, [2] * 3
        if kind == 5:
            s[L // 3:L // 3 + 3] = b"NNN"
        if kind == 6:
            s = bytearray(b"C" * L)
        out.append(rd(bytes(s), Qs(sc)))
    return out


def chunk_cases():
    C = []
    base = ["--min_L", "10"]
    subs = [[ragged(n, row[1], n)] for row in LDS_ROWS for n in chunk_sizes(row)]
    C.append(TCase("chunks_sizes", base, subs, ["chunks:batch_sizes_at_every_row"], kernels=["trim_lds"] * len(subs)))
    subs = []
    for row in LDS_ROWS:
        lo, hi, Cc, LPR, RPC, NW, _ = row
        good = ragged(RPC, hi, 3)
        empty = [rd(b"")] * RPC
        subs.append([good + empty + good])                                             # a chunk of empty reads only
        subs.append([good + [rd(b"")] + ragged(RPC, hi, 4)[:RPC - 2] + [rd(b"")] + good])                  # an empty read first and last in a chunk
        L32 = hi // 32 * 32
        if L32 >= max(lo, 32):
            eq = [rd(rb(L32, k), Qs([30 + k % 9] * (L32 - k % 5) + [2] * (k % 5))) for k in range(RPC)]
            # five chunks: the odd read in slot 0, two chunks of padded rows, the odd read in the last slot, the rest
            subs.append([[rd(rb(hi, 5))] + eq[1:] + eq + padded_mix(L32, RPC) + eq[:-1] + [rd(rb(7, 6))] + [rd(rb(hi, 7))]])
    C.append(TCase("chunks_empty_and_padded_rows", base, subs, ["chunks:chunk_of_empty_reads", "chunks:empty_read_first_and_last", "chunks:padded_rows_at_every_row",
                                                                 "chunks:odd_read_in_slot_0_of_an_equal_length_chunk", "chunks:odd_read_in_the_last_slot_of_an_equal_length_chunk"]))
    subs = []
    for hi in ROW_LAST:
        for k in range(16):
            subs.append([[rd(rb(k or 16, k))] + ragged(5, hi, k)])
    C.append(TCase("chunks_arena_offsets", ["--min_L", "1"], subs, ["chunks:every_arena_offset_mod_16"]))
    subs, shifts = [], []
    for hi in ROW_LAST + [TFA_FIRST]:
        for k in range(16):
            subs.append([ragged(6, hi, k)])
            shifts.append(k)
    C.append(TCase("chunks_device_addresses", ["--min_L", "1"], subs, ["chunks:every_device_address_mod_16"], shifts=shifts))
    subs, shifts = [], []
    for n, hi in enumerate(ROW_LAST + [TFA_FIRST]):
        # the arena's first read begins with a low head, its last read ends in a low tail; then both with terminal N runs as well
        subs.append([[rd(rb(hi // 2 + 1, hi), Qs([2] * 3 + [38] * (hi // 2 - 2)))] + ragged(3, hi, 9)[::-1] + [low_tail(hi - 3, 3, hi)]])
        subs.append([[rd(b"NN" + rb(hi // 2, hi), Qs([41] * 2 + [2] * 3 + [38] * (hi // 2 - 3)))] + ragged(3, hi, 9)[::-1] +
                     [rd(rb(hi - 2, hi) + b"NN", Qs([38] * (hi - 5) + [2] * 3 + [41] * 2))]])
        shifts += [(5 * n) % 16, (5 * n + 9) % 16]
    C.append(TCase("chunks_hostile_padding", ["--min_L", "1"], subs, ["chunks:hostile_padding"], hostile=True, shifts=shifts))
    subs, kernels = [], []
    for n in ROW_LENGTHS:
        subs.append([[rd(rb(1, k)) for k in range(40)] + [rd(rb(n, n))] + [rd(rb(1, k)) for k in range(30)]])
        kernels.append("trim_lds" if n <= ROW_LAST[-1] else "trim_filter_accumulate")
    C.append(TCase("chunks_one_long_read", ["--min_L", "1", "--lc", "1.0"], subs, ["chunks:one_long_read_among_one_base_reads"], kernels=kernels))
    subs = []
    for row in LDS_ROWS:
        reads = ragged(3 * row[4] + 5, row[1], 21)
        cuts = [0, 1, row[4] - 1, row[4] + 3, 2 * row[4] + 3, 2 * row[4] + 3, len(reads)]
        subs.append([reads[a:b] for a, b in zip(cuts, cuts[1:])])
    C.append(TCase("chunks_segments", base, subs, ["chunks:segment_boundaries_inside_a_chunk"]))
    return C


def byte_cases():
    C = []
    for off, extra in ((33, []), (64, ["--ascii", "64"]), (33, ["--out_ascii", "64"])):
        reads = []
        for b in (off - 1, off, off + 41, 0x00, 0x80, 0xFF):
            for n in (40, 150):
                good = Qs([38] * n, off)
                low = Qs([2] * 6, off)
                for p in (0, n - 1):
                    q = bytearray(good)
                    q[p] = b
                    reads.append(rd(rb(n, p), bytes(q)))
                # a kept window [6, n - 6): the byte on its first and last base and on the bases next to them
                for p in (5, 6, n - 7, n - 6):
                    q = bytearray(low + good[6:n - 6] + low)
                    q[p] = b
                    reads.append(rd(rb(n, p + 1), bytes(q)))
                    q[6 if p < 10 else n - 7] = off + 41
                    reads.append(rd(rb(n, p + 2), bytes(q)))
        name = "bytes_quality_ascii_%d%s" % (off, "_out_64" if extra and extra[0] == "--out_ascii" else "")
        C.append(TCase(name, ["--min_L", "1"] + extra, with_fillers(reads)[1::2], ["bytes:out_ascii_64"] if "out" in name else ["bytes:ascii_%d:quality_bytes_next_to_a_walked_window" % off]))
        # the same reads under fixed cuts of 6 bases and a walk that cuts nothing (-q 0): every byte on the window's first and last base too
        C.append(TCase(name + "_fixed_cuts", ["--min_L", "1", "-q", "0", "--5end", "6", "--3end", "6"] + extra, with_fillers(reads)[::2],
                       [] if "out" in name else ["bytes:ascii_%d:quality_bytes_at_the_window_edges" % off]))
    for nm, b in (("offset+42", 33 + 42), ("0x7F", 0x7F)):
        for where, p in (("first", 0), ("last", 59), ("outside", 57)):
            q = bytearray(Qs([38] * 54 + [2] * 6))
            q[p] = b
            C.append(TCase("bytes_error_%s_%s" % (nm, where), ["--min_L", "1"], one([rd(rb(150, 1)), rd(rb(60, 2), bytes(q)), rd(rb(60, 3))]),
                           ["bytes:%s_at_%s_is_an_error" % (nm, where)], error=True))
    reads = [rd(rb(20, b) + bytes([b]) + rb(29, b + 1)) for b in range(256)]
    C.append(TCase("bytes_every_byte_as_a_base", ["--min_L", "1"], with_fillers(reads)[::2], ["bytes:every_byte_as_a_base"]))
    subs = []
    for row in LDS_ROWS:
        RPC, hi = row[4], row[1]
        hot = lambda k: rd(rb(hi // 2, k) + bytes([0x80 + k % 128]) + rb(hi - hi // 2 - 1, k + 1))
        vetoed = rd(b"A" * (hi // 2) + bytes([0xC1]) + b"A" * (hi - hi // 2 - 1))                      # counted, then taken by the low-complexity filter
        vetoed2 = rd(rb(hi // 2, 3) + bytes([0xE1]) + b"NN" + rb(hi - hi // 2 - 3, 4))                # ... by the poly-N rule
        subs.append([[hot(1)] + ragged(RPC - 2, hi, 5) + [hot(2), vetoed] + ragged(RPC - 2, hi, 6) + [vetoed2, hot(7)]])
    C.append(TCase("bytes_high_bytes_in_chunks", ["--min_L", "1"], subs, ["bytes:high_byte_in_the_first_and_last_read_of_a_chunk", "bytes:high_byte_in_a_read_vetoed_after_counting"]))
    return C


def long_cases():
    C = []
    base = ["--min_L", "1", "-n", "2000"]
    for text in LONG_LC:
        lc = f32(float(text))
        reads = [r for n in LONG_LC[text] for letter in (0, 3) for r in lc_reads(n, lc, letter)]
        C.append(TCase("long_lc_%s" % text, base + ["--lc", text], one(reads), ["long:lc_%s:base_threshold_differs_from_exact" % text]))
    reads = []
    for n in (1025, 2049, 4096):
        V = avg_pass_sum(n, 25.0, 33)
        for v in (V - 1, V):
            reads.append(rd((rb(4096, v) * 2)[:n], Qs([v // n + (1 if k < v % n else 0) for k in range(n)])))
    C.append(TCase("long_avg_q_25", base + ["-q", "0", "--avg_q", "25"], one(reads), ["long:avg_q_25:sum_one_below_and_at_the_smallest_passing"]))
    reads = []
    avg = float(f32(20.2))
    for n in LONG_AVGQ_DIFF:
        V = avg_pass_sum(n, avg, 33)
        for v in (V - 1, V, V + 1):
            reads.append(rd((rb(4096, v) * 2)[:n], Qs([v // n + (1 if k < v % n else 0) for k in range(n)])))
    C.append(TCase("long_avg_q_20.2", base + ["--lc", "1.0", "-q", "0", "--avg_q", "20.2"], one(reads), ["long:avg_q_20.2:float_threshold_differs_from_exact"]))
    pairs = LONG_COMP_BELOW + LONG_COMP_ABOVE
    C.append(TCase("long_composition", base + ["--lc", "1.0"], one([rd(b"A" * c + b"T" * (n - c)) for n, c in pairs] + [rd(b"C" * c + b"G" * (n - c)) for n, c in pairs]),
                   ["long:composition_bins_below_the_exact_floor", "long:composition_bins_above_the_exact_floor"]))
    reads = []
    for n in (1025, 1500):
        for t in LONG_TAILS:
            reads.append(rd(rb(n, t), Qs([38] * (n - t) + [4] * t)))
            reads.append(rd(rb(n, t + 1), Qs([4] * t + [38] * (n - t))))
            reads.append(rd(rb(n, t + 2), Qs([5] * t + [38] * (n - 2 * t) + [5] * t)))
    for mname in ("bwa_plus", "bwa"):
        C.append(TCase("long_tails_%s" % mname, WALK_BASE + WALK_MODES[mname], one(reads), ["long:tails_of_63..129_low_bases"] if mname == "bwa_plus" else []))
    return C


FAMILIES = ("walk", "ends", "ns", "thresholds", "composition", "chunks", "bytes", "long")
_BUILDERS = dict(walk=walk_cases, ends=ends_cases, ns=ns_cases, thresholds=threshold_cases, composition=composition_cases, chunks=chunk_cases, bytes=byte_cases, long=long_cases)
# why a family does not run under a setting (the cases of the family are excluded by name: cases_of())
FAMILY_SETTINGS = {"composition": ("lds", "single_pass"), "chunks": ("lds", "single_pass"), "long": ("long",)}
FAMILY_REASON = {"composition": "names the rows and records of trim_lds: trim_long writes no records", "chunks": "names the rows and chunks of trim_lds: trim_long has no chunks",
                 "long": "reads past 1 024 bases run trim_long under every setting"}
_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        C = []
        for fam in FAMILIES:
            cs = _BUILDERS[fam]()
            for c in cs:
                c.family = fam
                for s in SETTINGS:
                    if s not in FAMILY_SETTINGS.get(fam, SETTINGS):
                        c.exclude[s] = FAMILY_REASON[fam]
            C += cs
        _CASES = C
    return _CASES


def cases_of(family, setting, cases=None):
    return [c for c in (all_cases() if cases is None else cases) if c.family == family and setting not in c.exclude]


def hostile_arenas(sub, off):
    """pack_segments with pads that must not show: 0xFF and 'N' around the bases, bytes past offset + 41 around the qualities.  Host memory, for
    the oracle (test_trim_edges_model.py); the device meets such pads through device_buffers()"""
    lens = [len(r[1]) for seg in sub for r in seg]
    offset = np.zeros(len(lens) + 1, np.uint32)
    offset[1:] = np.cumsum(lens)
    seg = np.cumsum([0] + [len(s) for s in sub]).astype(np.uint32)
    pad_s = (b"\xffN" * 64)[:64]
    pad_q = bytes([off + 60, 0x7F] * 32)
    seq = np.frombuffer(pad_s + b"".join(r[1] for s in sub for r in s) + pad_s, np.uint8)
    qual = np.frombuffer(pad_q + b"".join(r[2] for s in sub for r in s) + pad_q, np.uint8)
    return seq[64:], qual[64:], offset, seg


def device_buffers(sub, off, shift=0, hostile=True):
    """-> (seq buffer, qual buffer, front, offset, segment_start): a submission for faqcs_submit_device.  The arenas begin `front` = 64 + shift bytes into
    buffers that the caller places at a 16-byte aligned device address, and at least 64 bytes follow them.  Every byte outside the arenas is one that must
    not show: 0xFF and 'N' around the bases ('N' next to the arena on either side), bytes past offset + 41 around the qualities"""
    lens = [len(r[1]) for seg in sub for r in seg]
    offset = np.zeros(len(lens) + 1, np.uint32)
    offset[1:] = np.cumsum(lens)
    seg = np.cumsum([0] + [len(s) for s in sub]).astype(np.uint32)
    front = 64 + shift
    assert front >= PAD_BEFORE and 0 <= shift < 16
    back = PAD_AFTER + (-(front + int(offset[-1]))) % 16 + 16
    fs, bs, fq, bq = ((b"\xffN" * 40)[-front:], (b"N\xff" * 48)[:back], bytes([0x7F, off + 60] * 40)[-front:], bytes([off + 42, 0xFF, 0x7F] * 32)[:back]) if hostile else \
        (bytes(front), bytes(back), bytes(front), bytes(back))
    seq = np.frombuffer(fs + b"".join(r[1] for s in sub for r in s) + bs, np.uint8).copy()
    qual = np.frombuffer(fq + b"".join(r[2] for s in sub for r in s) + bq, np.uint8).copy()
    assert len(seq) == len(qual) == front + int(offset[-1]) + back and len(seq) % 16 == 0
    return seq, qual, front, offset, seg


def coverage(cases=None):
    """Every predicate on every case -> ({edge: [cases that claim it and reach it]}, {case: [claims that do not hold]}, {edge: [cases that reach it
    without claiming it]}).  A predicate that cannot be put to a case it was not written for (it looks for a read the case does not have) does not hold there."""
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
                except (IndexError, KeyError, TypeError, ValueError):
                    pass
    return table, lost, more


if __name__ == "__main__":
    t, lost, more = coverage()
    print("claimed  unclaimed  edge")
    for e, v in t.items():
        print("%7d  %9d  %s" % (len(v), len(more[e]), e))
    print("%d cases, %d reads, %d edges; claims that do not hold: %s" % (len(all_cases()), sum(c.n_reads() for c in all_cases()), len(t), lost))
