"""A constructed catalogue of inputs for the owner-partitioned k-mer exchange (kmer_send_items / skm_outbox on the sender,
skm_items with its part_lo / part_mul remap and kg_add_items on the owner, the direct form kmer_send_pairs / kmer_extract / kmer_insert_items,
faqcs_kmer_forward with its two staging buffers, faqcs_kmer_outbox with ob_fresh, faqcs_kmer_epoch_counts), in the manner of tests/kmer_edges.py:
every case is a named builder of SENDERS of submissions of segments of reads, every segment with an epoch (or EPOCH_NONE); every edge a
PREDICATE over a case's inputs and the model's trace; coverage() puts every predicate to every case.

Trace(case) is the plain reference.  It does not call the library and reads none of the kernels' tables.  Every canonical k-mer occurrence
of a counted window (the kept windows come from the oracle's per-read results, as in kmer_edges.oracle_results) has an owner:
    item mode     (bucket * world) >> 8, bucket = skm_part(minimizer of the k-mer) >> 11 (kmer_edges.min_ords / skm_part)
    direct mode   (n_epochs > 1000 or FAQCS_KMER_DIRECT=1) kmer_owner(key, world) of faqcs_kmer.h, restated below with kmer_mix
From that it derives, per sender and submission, the outbox (per destination the multiset of (key, epoch) occurrences) and, per owner and
after any sequence of inserts, total_by_epoch, distinct_by_first_epoch (keys by their smallest epoch) and the histogram of counts.  The
owner side selects its occurrences by the OWNER's rule (buckets ceil(r * 256 / world) .. ceil((r + 1) * 256 / world)), the outbox by the
SENDER's; tests/test_kmer_exchange_edges_model.py holds the two to each other, the model to the oracle and the restated constants to the
sources, without a GPU; tests/test_gpu_kmer_exchange_edges.py sends the catalogue through several contexts on one device.

The item layout (16 bytes; NK at bit 30, PART at bit 35 with 19 bits, RUN at bit 54 with 10 bits) and the two key encodings (item_keys: what
faqcs_kmer_outbox_host lists in item mode; direct_keys: the keys of the (key, epoch) pairs) are restated to READ the library's outbox --
to cut the key list by item, to read an item's partition and epoch, to compare multisets of keys.  Expected counts never come from them
(the direct mode's owner rule, which is a function of the direct key, excepted: the issue of this catalogue asks for that restatement).

    python -m tests.kmer_exchange_edges        prints the number of cases per edge
"""
import collections

import numpy as np

try:
    import kmer_edges as ke
except ImportError:  # (python -m tests.kmer_exchange_edges)
    from tests import kmer_edges as ke

EPOCH_NONE = 0xFFFFFFFF
MAX_READ, IN_OFF = ke.MAX_READ, ke.IN_OFF
# restated; test_kmer_exchange_edges_model.py compares them with the sources
KG_EPOCH_SPAN = KG_MAX_RUNS = 1000
KG_MIN_CAP, KG_FAN, WORLD_MAX = 128, 256, 64
NK_SHIFT, NK_BITS, PART_SHIFT, PART_BITS, RUN_SHIFT, RUN_BITS = 30, 5, 35, 19, 54, 10
MIX_1, MIX_2, MIX_SHIFT = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53, 33
SMALL_GROUP = 1 << 14  # FAQCS_KMER_GROUP_ITEMS of the small_groups setting: the occurrences a group takes
CONSTANT_SOURCES = {
    "KG_EPOCH_SPAN": ("faqcs_kmer.h", r"KG_EPOCH_SPAN = (\d+)"), "KG_MAX_RUNS": ("faqcs_kmer.h", r"KG_MAX_RUNS = (\d+)"),
    "KG_MIN_CAP": ("faqcs_kmer.h", r"KG_MIN_CAP = (\d+)"), "KG_FAN": ("faqcs_kmer.h", r"KG_FAN = (\d+)"),
    "WORLD_MAX": ("faqcs_capi_kmer.hip", r"world == 0 \|\| world > (\d+)"),
    "NK_SHIFT": ("faqcs_skm.h", r"SKM_NK_SHIFT = (\d+)"), "PART_SHIFT": ("faqcs_skm.h", r"SKM_PART_SHIFT = (\d+)"), "PART_BITS": ("faqcs_skm.h", r"SKM_PART_BITS = (\d+)"),
    "RUN_SHIFT": ("faqcs_skm.h", r"SKM_RUN_SHIFT = (\d+)"), "RUN_BITS": ("faqcs_skm.h", r"SKM_RUN_BITS = (\d+)"),
}
MUTANTS = {  # a wrong model -> the case that tells it from the right one (test_kmer_exchange_edges_model.py)
    "owner_from_key_hash": "owners_world_3", "floor_lo_b": "owners_world_3", "dest_rounds_up": "owners_world_3", "max_epoch": "min_epoch_7_then_3_two_calls",
    "none_counted": "epochs_none_first_middle_last", "run_number_for_epoch": "epochs_n1000_item_path", "outbox_again": "outbox_asked_twice",
    "spill_dropped": "outbox_spill",
}
U = np.uint64


def cat(parts, dtype=np.uint64):
    return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)


# =====================================================================================================================================
# the two key encodings of the library's outbox and the direct mode's owner rule, restated
# =====================================================================================================================================
def item_keys(bases, k):
    """bases: bytes of ACGTacgt only -> what faqcs_kmer_outbox_host lists for each k-mer in item mode: base i at bits 2 i, A C T G = 0 1 2 3,
    the smaller of the k-mer and its reverse complement (faqcs_skm.h: skm_roll_key)"""
    c = ke._SKM[np.frombuffer(bases, np.uint8)].astype(U)
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, U)
    fwd, rc = np.zeros(n, U), np.zeros(n, U)
    for i in range(k):
        fwd |= c[i:i + n] << U(2 * i)
        rc |= (c[k - 1 - i:k - 1 - i + n] ^ U(2)) << U(2 * i)
    return np.minimum(fwd, rc)


def direct_keys(bases, k):
    """the key of a (key, epoch) pair (faqcs_kmer.h: kmer_chunk_key).  The kernel's codes are A T C G = 0 1 2 3; its key is two bit planes,
    the low plane (bit 0 of the code: set for T and G) in bits 0 .. 31 and the high plane (bit 1: set for C and G) in bits 32 .. 63, bit t =
    base t; the reverse complement reverses both planes and inverts the low one; the key is the smaller of the two"""
    c = ke._SKM[np.frombuffer(bases, np.uint8)].astype(U)  # (kmer_edges' table is A C T G = 0 1 2 3: T and G have ITS bit 1 set, C and G its bit 0)
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, U)
    p0, p1 = c >> U(1), c & U(1)  # the kernel's low plane (T or G), its high plane (C or G)
    w0, w1, r0, r1 = (np.zeros(n, U) for _ in range(4))
    for i in range(k):
        w0 |= p0[i:i + n] << U(i)
        w1 |= p1[i:i + n] << U(i)
        r0 |= (U(1) - p0[k - 1 - i:k - 1 - i + n]) << U(i)
        r1 |= p1[k - 1 - i:k - 1 - i + n] << U(i)
    return np.minimum((w1 << U(32)) | w0, (r1 << U(32)) | r0)


def kmer_mix(x):
    x = np.asarray(x, U).copy()
    x ^= x >> U(MIX_SHIFT)
    x *= U(MIX_1)
    x ^= x >> U(MIX_SHIFT)
    x *= U(MIX_2)
    x ^= x >> U(MIX_SHIFT)
    return x


def kmer_owner(key, world):
    return (((kmer_mix(key) >> U(32)) * U(world)) >> U(32)).astype(np.int64)


def lo_bucket(r, world, floor=False):
    """first bucket of rank r by the OWNER's rule (kg_init: lo_b)"""
    return r * 256 // world if floor else (r * 256 + world - 1) // world


def part_range(r, world):
    """the 19-bit partitions rank r owns"""
    return lo_bucket(r, world) << 11, lo_bucket(r + 1, world) << 11


def cap1_of(n_reads, n_bases, k):
    """sub-region capacity of the sender staging (kmer_send_items), restated"""
    w = ke.skm_geom(k)[1]
    ib = (n_bases if w == 1 else n_bases * 3 // (w + 1)) + 2 * n_reads + 64
    return max(KG_MIN_CAP, 2 * ib // (KG_FAN * KG_FAN) + 64)


def writing_blocks(n_reads, max_len):
    """blocks of an extraction launch over n_reads reads at most (faqcs_skm_grid16 / faqcs_skm_grid; fewer on a device with fewer CUs)"""
    per = 256 if max_len <= 256 else 64
    return max(1, min(KG_FAN, (n_reads + per - 1) // per))


_OCC = {}


def window_occ(eff, k):
    """-> (canonical key of the model, 19-bit partition, item key, direct key, 'an item starts here') of every k-mer of a window, in order"""
    key = (eff, k)
    if key not in _OCC:
        parts = [[] for _ in range(5)]
        w = ke.skm_geom(k)[1]
        for s, n in ke.stretches(eff):
            if n < k:
                continue
            seg = eff[s:s + n]
            mo = ke.min_ords(seg, k)
            idx = np.arange(len(mo))
            start = np.maximum.accumulate(np.where(np.concatenate([[True], mo[1:] != mo[:-1]]), idx, 0))
            for p, v in zip(parts, (ke.canonical_kmers([seg], k), ke.skm_part(mo), item_keys(seg, k), direct_keys(seg, k), (idx - start) % w == 0)):
                p.append(np.asarray(v, U))
        if len(_OCC) > 40000:
            _OCC.clear()
        _OCC[key] = tuple(cat(p) for p in parts)
    return _OCC[key]


# =====================================================================================================================================
# cases
# =====================================================================================================================================
class Sub:
    """one submission: segments of (epoch, reads); error: the message faqcs_submit must refuse it with"""

    def __init__(self, segs, error=None):
        self.segs, self.error = [(int(e), list(r)) for e, r in segs], error

    def buffers(self):
        return [r for _, r in self.segs]

    def epochs(self):
        return [e for e, _ in self.segs]

    def runs(self):
        """[(first segment, end segment)] of the launches (faqcs_capi_kmer.hip: for_each_epoch_run): consecutive segments of one epoch that hold reads"""
        out, s, n = [], 0, len(self.segs)
        while s < n:
            e = s + 1
            while e < n and self.segs[e][0] == self.segs[s][0]:
                e += 1
            if self.segs[s][0] != EPOCH_NONE and any(self.segs[j][1] for j in range(s, e)):
                out.append((s, e))
            s = e
        return out


class XCase:
    """name, family, k, world, n_epochs, senders (each a list of Sub), the edges it claims; direct_env: FAQCS_KMER_DIRECT=1; owner_ranks: the
    ranks whose tables the device run builds (None: all); extra: more options; flow: how the device run moves the items ('plain': kmer_outbox ->
    copy -> kmer_insert_device; 'forward' / 'forward_peer': faqcs_kmer_forward; 'ring': every context sender and owner, pipelined)"""

    def __init__(self, name, family, k, world, n_epochs, senders, claims, direct_env=False, owner_ranks=None, extra=(), flow="plain", expect=()):
        self.name, self.family, self.k, self.world, self.n_epochs, self.senders, self.claims = name, family, k, world, n_epochs, senders, tuple(claims)
        self.direct_env, self.owner_ranks, self.extra, self.flow, self.expect = direct_env, owner_ranks, [str(x) for x in extra], flow, tuple(expect)
        self._res, self._ctx = None, None

    @property
    def direct(self):
        return self.direct_env or self.n_epochs > KG_EPOCH_SPAN

    def ranks(self):
        return list(range(self.world)) if self.owner_ranks is None else sorted(set(self.owner_ranks))

    def args(self):
        return [str(a) for a in ke.TR(self.k)] + self.extra

    def opt(self):
        from faqcs_amd.options import parse_args

        return parse_args(["-u", "x", "-d", "y", "--kmer_rarefaction"] + self.args())

    def ctx(self):
        if self._ctx is None:
            self._ctx = Ctx(self)
        return self._ctx


_RES = {}


def oracle_results(case):
    """[sender][submission] -> the oracle's per-read records (the kept windows); equal submissions under equal options are computed once"""
    if case._res is None:
        from oracle_engine import OracleEngine

        from faqcs_amd import driver

        ora, out = None, []
        for subs in case.senders:
            out.append([])
            for sub in subs:
                key = (tuple(case.args()), tuple(len(b) for b in sub.buffers()), hash(tuple(r[1:] for b in sub.buffers() for r in b)))
                if key not in _RES:
                    ora = ora or OracleEngine(case.opt(), MAX_READ, IN_OFF)
                    _RES[key] = ora.process(*driver.pack_segments(sub.buffers()))
                out[-1].append(_RES[key])
        if ora:
            ora.close()
        case._res = out
    return case._res


class Trace:
    """The model of one case.  sub[(s, i)]: the counted occurrences of sender s's submission i as arrays (canon, lkey: the key the library's
    outbox shows, epoch, dest: by the sender's rule, bucket, part, first: an item starts, read) -- None for a refused submission."""

    def __init__(self, case, mutant=None):
        self.case, self.mutant, self.world, self.direct = case, mutant, case.world, case.direct
        res, rq = oracle_results(case), case.opt().replace_to_N_q
        self.sub = {}
        for s, subs in enumerate(case.senders):
            for i, sub in enumerate(subs):
                self.sub[(s, i)] = None if sub.error else self._sub(sub, res[s][i], rq)

    def _sub(self, sub, res, rq):
        k, world, mutant = self.case.k, self.world, self.mutant
        run_of = {j: n for n, (a, e) in enumerate(sub.runs()) for j in range(a, e)}
        cols, at, n_bases, max_len = [[] for _ in range(7)], 0, 0, 0
        for j, (epoch, reads) in enumerate(sub.segs):
            for r_i, (_, s, q) in enumerate(reads):
                rec = res[at + r_i]
                n_bases, max_len = n_bases + len(s), max(max_len, len(s))
                if not int(rec["flags"]) & 1 or (epoch == EPOCH_NONE and mutant != "none_counted"):
                    continue
                a, n = int(rec["start"]), int(rec["len"])
                canon, part, ikey, dkey, first = window_occ(ke.effective(s[a:a + n], q[a:a + n], rq), k)
                e = 0 if epoch == EPOCH_NONE else run_of[j] if mutant == "run_number_for_epoch" else epoch
                for c, v in zip(cols, (canon, part, ikey, dkey, first, np.full(len(canon), e, U), np.full(len(canon), at + r_i, U))):
                    c.append(v)
            at += len(reads)
        canon, part, ikey, dkey, first, epoch, read = (cat(c) for c in cols)
        bucket = (part >> U(11)).astype(np.int64)
        if self.direct or mutant == "owner_from_key_hash":
            dest = kmer_owner(dkey, world)
        elif mutant == "dest_rounds_up":
            dest = (bucket * world + world - 1) >> 8
        else:
            dest = (bucket * world) >> 8
        d = dict(canon=canon, lkey=dkey if self.direct else ikey, epoch=epoch.astype(np.int64), dest=dest, bucket=bucket, part=part.astype(np.int64),
                 first=first.astype(bool), read=read.astype(np.int64), n_runs=len(sub.runs()), n_reads=at, max_len=max_len, cap1=cap1_of(at, n_bases, k))
        if mutant == "spill_dropped" and not self.direct:  # what a sender without the spill area would send: cap1 items per (bucket, writing block)
            item = np.cumsum(d["first"]) - 1
            seen, keep_item = collections.Counter(), np.ones(int(item[-1]) + 1 if len(item) else 0, bool)
            for it in np.nonzero(d["first"])[0].tolist():
                where = (int(bucket[it]), int(d["read"][it]) // 256)
                seen[where] += 1
                keep_item[item[it]] = seen[where] <= d["cap1"]
            keep = keep_item[item]
            for name in ("canon", "lkey", "epoch", "dest", "bucket", "part", "first", "read"):
                d[name] = d[name][keep]
        return d

    # ---- the sender ----------------------------------------------------------------------------------------------------------------
    def outbox_occurrences(self, s, i, call=1):
        """occurrences per destination the call-th faqcs_kmer_outbox behind submission i reports (in direct mode: its counts)"""
        d = self.sub[(s, i)]
        if call > 1 and self.mutant != "outbox_again":
            return np.zeros(self.world, np.int64)
        return np.bincount(d["dest"], minlength=self.world)

    def outbox_keys(self, s, i):
        """{(destination, epoch): sorted keys as the library's outbox shows them}"""
        d, out = self.sub[(s, i)], {}
        for dest, e in sorted(set(zip(d["dest"].tolist(), d["epoch"].tolist()))):
            out[(dest, e)] = np.sort(d["lkey"][(d["dest"] == dest) & (d["epoch"] == e)])
        return out

    def items_to(self, s, i, dest):
        """items the model cuts for a destination (runs of one minimizer, at most w k-mers): exact where an item is one k-mer (k <= 15)"""
        d = self.sub[(s, i)]
        return int((d["first"] & (d["dest"] == dest)).sum())

    # ---- the owner -----------------------------------------------------------------------------------------------------------------
    def order(self):
        """the insert calls in the order every owner sees them: submission by submission, sender by sender"""
        n = max(len(subs) for subs in self.case.senders)
        return [(s, i) for i in range(n) for s in range(len(self.case.senders)) if i < len(self.case.senders[s]) and self.sub[(s, i)] is not None]

    def owned(self, r, s, i):
        """(canon, epoch) of submission (s, i) that rank r OWNS, by the owner's rule"""
        d = self.sub[(s, i)]
        if self.direct:
            m = d["dest"] == r
        else:
            floor = self.mutant == "floor_lo_b"
            m = (d["bucket"] >= lo_bucket(r, self.world, floor)) & (d["bucket"] < lo_bucket(r + 1, self.world, floor))
        return d["canon"][m], d["epoch"][m]

    def arrivals(self, r):
        """[((s, i), canon, epoch)] of the insert calls that bring rank r something"""
        out = []
        for s, i in self.order():
            c, e = self.owned(r, s, i)
            if len(c):
                out.append(((s, i), c, e))
        return out

    def owner_state(self, r, steps=None):
        """(distinct_by_first_epoch, total_by_epoch, histogram [(count, keys)]) of rank r after its first `steps` arrivals (None: all)"""
        arr = self.arrivals(r)[:steps]
        return self.state_of(cat([a[1] for a in arr]), cat([a[2] for a in arr], np.int64))

    def state_of(self, canon, epoch):
        n = self.case.n_epochs
        if not len(canon):
            return [0] * n, [0] * n, []
        u, inv = np.unique(canon, return_inverse=True)
        if self.mutant == "max_epoch":
            first = np.zeros(len(u), np.int64)
            np.maximum.at(first, inv, epoch)
        else:
            first = np.full(len(u), 1 << 40, np.int64)
            np.minimum.at(first, inv, epoch)
        hist = sorted(collections.Counter(np.bincount(inv).tolist()).items())
        return np.bincount(first, minlength=n).tolist(), np.bincount(epoch, minlength=n).tolist(), hist

    def whole(self):
        """every owner's state summed: (distinct_by_first_epoch, total_by_epoch, histogram)"""
        d, t, h = np.zeros(self.case.n_epochs, np.int64), np.zeros(self.case.n_epochs, np.int64), collections.Counter()
        for r in range(self.world):
            a, b, c = self.owner_state(r)
            d, t = d + np.asarray(a), t + np.asarray(b)
            h.update(dict(c))
        return d.tolist(), t.tolist(), sorted(h.items())

    def observable(self):
        """everything a device run compares, as one value (the mutants are told apart by it)"""
        subs = [(key, self.outbox_occurrences(*key).tolist(), self.outbox_occurrences(*key, call=2).tolist(),
                 [(de, v.tolist()) for de, v in self.outbox_keys(*key).items()]) for key in sorted(self.sub) if self.sub[key] is not None]
        return subs, [self.owner_state(r) for r in range(self.world)]


class Ctx:
    """what the predicates look at: the case and its trace"""

    def __init__(self, case):
        self.case, self.t, self.k, self.world, self._buckets = case, Trace(case), case.k, case.world, None

    def subs(self):
        return [(key, d) for key, d in sorted(self.t.sub.items()) if d is not None]

    def buckets(self):
        """{bucket: items} over all submissions (item mode)"""
        if self._buckets is None:
            self._buckets = collections.Counter()
            for _, d in self.subs():
                self._buckets.update(d["bucket"][d["first"]].tolist())
        return self._buckets

    def n_occ(self):
        return sum(len(d["canon"]) for _, d in self.subs())

    def first_epochs_of(self, key):
        """the first epoch of one canonical key on its owner after each of the owner's arrivals (None: not there yet), and the owner"""
        for r in range(self.world):
            arr = self.t.arrivals(r)
            if any((c == U(key)).any() for _, c, _ in arr):
                out, best = [], None
                for _, c, e in arr:
                    m = e[c == U(key)]
                    if len(m):
                        best = int(m.min()) if best is None else min(best, int(m.min()))
                    out.append(best)
                return out, r
        return [], None


def rb(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.Generator(np.random.PCG64([777, seed])).integers(0, 4, n)].tobytes()


rd = ke.rd


def reads_of(n, length, seed):
    return [rd(rb(length, 1000 * seed + i)) for i in range(n)]


EDGES = {}


def edge(name):
    def reg(f):
        EDGES[name] = f
        return f
    return reg


FAMILIES = ("owners", "epochs", "outbox", "forward", "ring")
WORLDS = (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
OWNER_WORLDS = (2, 3, 7, 8, 33, 64)
K_WORLDS = [(w, k) for w in (3, 64) for k in (3, 15, 16, 31)]


def owner_ranks(world):
    return sorted({0, 1, world // 2, world - 1})


# ---- owners ---------------------------------------------------------------------------------------------------------------------------
def _boundary(c, world, r):
    if c.world != world or c.t.direct:
        return False
    b, n = lo_bucket(r, world), c.buckets()
    return n[b - 1] > 0 and n[b] > 0 and ((b - 1) * world) >> 8 == r - 1 and (b * world) >> 8 == r


def _ends(c, world, r):
    if c.world != world or r not in c.case.ranks() or c.t.direct:
        return False
    lo, hi = part_range(r, world)
    parts = set()
    for _, d in c.subs():
        parts.update(d["part"][d["dest"] == r].tolist())
    return c.world == world and r in c.case.ranks() and lo in parts and hi - 1 in parts and all(lo <= p < hi for p in parts)


for _w in WORLDS:
    edge("world=%d:every_bucket_holds_an_item" % _w)(lambda c, w=_w: c.world == w and c.k == 31 and not c.t.direct and all(c.buckets()[b] > 0 for b in range(256)))
    for _r in range(1, _w):
        edge("world=%d:both_buckets_at_the_boundary_of_rank_%d" % (_w, _r))(lambda c, w=_w, r=_r: _boundary(c, w, r))
for _w, _k in K_WORLDS:
    edge("world=%d:k=%d" % (_w, _k))(lambda c, w=_w, k=_k: c.world == w and c.k == k and c.n_occ() > 0 and c.case.family == "owners" and not c.t.direct)
for _w in (5, 64):  # the direct form: kmer_extract's lane d counts for destination d -- at world 64 every lane of the wave
    edge("direct:world=%d:every_destination_holds_a_pair_in_both_epochs" % _w)(lambda c, w=_w: c.world == w and c.t.direct and c.case.family == "owners" and all(
        (np.bincount(d["dest"][d["epoch"] == e], minlength=w) > 0).all() for _, d in c.subs() for e in (0, 1)))
for _w in OWNER_WORLDS:
    for _r in owner_ranks(_w):
        edge("world=%d:rank_%d_receives_its_first_and_its_last_partition" % (_w, _r))(lambda c, w=_w, r=_r: _ends(c, w, r))


def _one_owner(c):
    """no canonical key with two destinations (the sender's rule) over the whole case"""
    keys = cat([d["canon"] for _, d in c.subs()])
    dest = cat([d["dest"] for _, d in c.subs()], np.int64)
    pairs = np.unique(np.stack([keys.astype(np.int64), dest]), axis=1) if len(keys) else np.zeros((2, 0), np.int64)
    return len(pairs[0]) == len(np.unique(keys))


def _both_strands(c):
    a, b = c.case.senders[0][0].buffers()[0], c.case.senders[1][0].buffers()[0]
    return len(c.case.senders) == 2 and [ke.revcomp(r[1]) for r in a] == [r[1] for r in b] and all(r[1] != ke.revcomp(r[1]) for r in a) and \
        sorted(c.t.sub[(0, 0)]["canon"].tolist()) == sorted(c.t.sub[(1, 0)]["canon"].tolist()) and c.n_occ() > 0 and _one_owner(c)


edge("both_strands_of_a_key_from_two_senders:one_owner")(lambda c: len(c.case.senders) == 2 and _both_strands(c))
edge("k=30:palindromic_key:one_owner")(lambda c: c.k == 30 and len(c.case.senders) == 2 and _one_owner(c) and
                                       all(len(np.unique(d["canon"])) == 1 and len(d["canon"]) == 3 for _, d in c.subs()) and
                                       all(r[1] == ke.revcomp(r[1]) for subs in c.case.senders for r in subs[0].buffers()[0]))


# ---- epochs ---------------------------------------------------------------------------------------------------------------------------
def _epochs_used(c):
    return sorted({e for _, d in c.subs() for e in d["epoch"].tolist()})


edge("n_epochs=1000:epochs_0_1_998_999:item_path")(lambda c: c.case.n_epochs == 1000 and not c.t.direct and _epochs_used(c) == [0, 1, 998, 999] and (1 << RUN_BITS) > 999)
edge("n_epochs=1001:epoch_1000:direct_path")(lambda c: c.case.n_epochs == 1001 and c.t.direct and not c.case.direct_env and 1000 in _epochs_used(c))
edge("FAQCS_KMER_DIRECT=1:n_epochs=5")(lambda c: c.case.direct_env and c.case.n_epochs == 5 and _epochs_used(c) == [0, 1, 2, 3, 4])
edge("item_twin_of_the_direct_case")(lambda c: not c.t.direct and c.case.n_epochs == 5 and c.case.name == "epochs_item_twin_n5" and _epochs_used(c) == [0, 1, 2, 3, 4])


def _none_at(c, where):
    for subs in c.case.senders:
        for sub in subs:
            ep = sub.epochs()
            holds = [any(len(r[1]) >= c.k for r in rs) for _, rs in sub.segs]
            idx = [j for j, e in enumerate(ep) if e == EPOCH_NONE and holds[j]]
            counted = [j for j, e in enumerate(ep) if e != EPOCH_NONE and holds[j]]
            if counted and any((where == "first" and j == 0) or (where == "last" and j == len(ep) - 1) or (where == "middle" and min(counted) < j < max(counted)) for j in idx):
                return True
    return False


for _where in ("first", "middle", "last"):
    edge("EPOCH_NONE_segment_%s" % _where)(lambda c, w=_where: _none_at(c, w))
edge("consecutive_segments_of_one_epoch_make_one_run")(lambda c: any(sum(1 for j in range(a, e) if sub.segs[j][1]) >= 2 for subs in c.case.senders for sub in subs for a, e in sub.runs()))


def _segs3(c):
    return [(x, y, z) for subs in c.case.senders for sub in subs for x, y, z in zip(sub.segs, sub.segs[1:], sub.segs[2:]) if x[1] and not y[1] and z[1]]


edge("empty_segment_inside_a_run")(lambda c: any(x[0] == y[0] == z[0] != EPOCH_NONE for x, y, z in _segs3(c)))
edge("empty_segment_of_another_epoch_between_two_of_one")(lambda c: any(x[0] == z[0] != y[0] and x[0] != EPOCH_NONE for x, y, z in _segs3(c)))
edge("empty_segment_between_two_epochs")(lambda c: any(x[0] != z[0] and EPOCH_NONE not in (x[0], z[0]) for x, y, z in _segs3(c)))
edge("runs=KG_MAX_RUNS_in_one_submission")(lambda c: any(d["n_runs"] == KG_MAX_RUNS and len(d["canon"]) > 0 for _, d in c.subs()))
edge("runs=KG_MAX_RUNS+1:refused_and_the_context_usable")(lambda c: any(sub.error and len(sub.runs()) == KG_MAX_RUNS + 1 and i + 1 < len(subs) and c.t.sub[(s, i + 1)] is not None and
                                                                          len(c.t.sub[(s, i + 1)]["canon"]) > 0 for s, subs in enumerate(c.case.senders) for i, sub in enumerate(subs)))
KEY_READ = rb(31, 31)


def _K():
    return int(ke.canonical_kmers([KEY_READ], 31)[0])


def _arrivals_of_K(c):
    """[((s, i), epochs of K in that insert call)] on K's owner"""
    if c.case.family != "epochs" or c.k != 31:
        return []
    f, r = c.first_epochs_of(_K())
    return [] if r is None else [(key, sorted(e[cn == U(_K())].tolist())) for key, cn, e in c.t.arrivals(r) if (cn == U(_K())).any()]


edge("min_epoch:7_then_3:two_insert_calls_of_one_sender")(lambda c: [(k[0], e) for k, e in _arrivals_of_K(c)] == [(0, [7]), (0, [3])])
edge("min_epoch:7_then_3:one_insert_call")(lambda c: [e for _, e in _arrivals_of_K(c)] == [[3, 7]] and
                                           [sub.epochs() for sub in c.case.senders[0]] == [[7, 3]])
edge("min_epoch:7_then_3:two_senders")(lambda c: [(k[0], e) for k, e in _arrivals_of_K(c)] == [(0, [7]), (1, [3])])
edge("min_epoch:equal_epochs_from_two_senders")(lambda c: [(k[0], e) for k, e in _arrivals_of_K(c)] == [(0, [5]), (1, [5])])


def _moves(c):
    """K's first epoch is 7 after one arrival and 3 after a later one; total_by_epoch keeps both"""
    f, r = c.first_epochs_of(_K()) if c.case.family == "epochs" and c.k == 31 else ([], None)
    if r is None or 7 not in f or f[-1] != 3:
        return False
    at7 = f.index(7)
    d7, _, _ = c.t.owner_state(r, at7 + 1)
    d, t, _ = c.t.owner_state(r)
    return d7[7] >= 1 and d[7] == d7[7] - 1 and d[3] >= 1 and t[7] >= 1 and t[3] >= 1


edge("min_epoch:first_hist_moves_from_7_to_3:total_by_epoch_keeps_both")(_moves)


def _flush_between(c):
    """between K's two arrivals its owner takes more occurrences than a group of the small_groups setting holds: under that setting the second
    arrival finds K in the table; under the default setting (groups of millions) both arrivals meet in one group"""
    f, r = c.first_epochs_of(_K()) if c.case.family == "epochs" and c.k == 31 else ([], None)
    if r is None or 7 not in f or 3 not in f:
        return False
    arr = c.t.arrivals(r)
    return sum(len(a[1]) for a in arr[f.index(7) + 1:f.index(3)]) > SMALL_GROUP


edge("min_epoch:a_group_of_2^14_flushed_between_the_arrivals")(_flush_between)
edge("min_epoch:a_group_of_2^14_flushed_between_the_arrivals:two_senders")(lambda c: _flush_between(c) and [(k[0], e) for k, e in _arrivals_of_K(c)] == [(0, [7]), (1, [3])])


def _one_call_beyond_a_group(c):
    """K with 7 and with 3 in ONE insert call that holds more occurrences than a group of the small_groups setting: the call is cut into
    several groups (whether K's two items fall into different ones cannot be read through the ABI)"""
    arr = _arrivals_of_K(c)
    if [e for _, e in arr] != [[3, 7]]:
        return False
    _, r = c.first_epochs_of(_K())
    return [len(a[1]) > SMALL_GROUP for a in c.t.arrivals(r) if a[0] == arr[0][0]] == [True] and c.case.senders[0][0].epochs() == [7, 5, 3]


edge("min_epoch:7_and_3_in_one_insert_call_beyond_a_group_of_2^14")(_one_call_beyond_a_group)


# ---- outbox ---------------------------------------------------------------------------------------------------------------------------
edge("every_read_shorter_than_k:all_counts_zero")(lambda c: all(len(r[1]) == c.k - 1 for subs in c.case.senders for sub in subs for b in sub.buffers() for r in b) and
                                                  c.n_occ() == 0 and len(c.subs()) > 0 and all(d["n_reads"] > 0 for _, d in c.subs()))
edge("second_outbox_call_returns_zeros")(lambda c: c.case.name == "outbox_asked_twice" and c.t.outbox_occurrences(0, 0).sum() > 0 and c.t.outbox_occurrences(0, 0, call=2).sum() == 0)
edge("empty_submission_behind_a_full_one")(lambda c: any(a is not None and b is not None and len(a["canon"]) > 0 and b["n_reads"] == 0
                                                         for a, b in [(c.t.sub[(0, i)], c.t.sub[(0, i + 1)]) for i in range(len(c.case.senders[0]) - 1)]))


def _dests(c, s=0, i=0):
    return np.nonzero(c.t.outbox_occurrences(s, i))[0].tolist()


POLY_A_DEST = (int(ke.skm_part(ke.min_ords(b"A" * 31, 31)[0]) >> 11) * 64) >> 8
edge("world=64:poly_A_only:one_destination_63_zero_counts")(lambda c: c.world == 64 and all(set(r[1]) == {ord("A")} for r in c.case.senders[0][0].buffers()[0]) and
                                                            _dests(c) == [POLY_A_DEST])
edge("world=64:destinations_0_and_63_zeros_between")(lambda c: c.world == 64 and _dests(c) == [0, 63])


def _spill(c):
    """pigeonhole: the items of one bucket exceed cap1 in every one of the sub-regions the submission's writing blocks can use"""
    for _, d in c.subs():
        if len(d["canon"]) and not c.t.direct:
            n = collections.Counter(d["bucket"][d["first"]].tolist()).most_common(1)[0][1]
            if n > writing_blocks(d["n_reads"], d["max_len"]) * d["cap1"] and d["cap1"] == max(KG_MIN_CAP, d["cap1"]):
                return True
    return False


edge("spill:one_sub_region_beyond_cap1")(_spill)
edge("staging:small_large_small_submissions_on_one_sender")(lambda c: len(c.case.senders) == 1 and len(c.subs()) == 3 and
                                                            c.subs()[1][1]["n_reads"] > 10 * c.subs()[2][1]["n_reads"] > 10 * c.subs()[0][1]["n_reads"] > 0)


# ---- forward --------------------------------------------------------------------------------------------------------------------------
def _bounds(c, r):
    """[(fewest, most) items rank r can get from each submission of sender 0]: an item holds 1 .. w occurrences"""
    w = ke.skm_geom(c.k)[1]
    occ = [int(c.t.outbox_occurrences(0, i)[r]) for i in range(len(c.case.senders[0]))]
    return [((n + w - 1) // w, n) for n in occ]


edge("forward:in_place")(lambda c: c.case.flow == "forward" and c.world == 3 and c.n_occ() > 0)
edge("forward:behind_an_empty_submission_nothing_moves")(lambda c: c.case.flow in ("forward", "forward_peer") and any(
    a is not None and b is not None and len(a["canon"]) > 0 and b["n_reads"] == 0 for a, b in [(c.t.sub[(0, i)], c.t.sub[(0, i + 1)]) for i in range(len(c.case.senders[0]) - 1)]))
edge("forward:peer_copy:five_forwards_to_one_owner_third_beyond_the_capacity")(lambda c: c.case.flow == "forward_peer" and any(
    len(b) == 5 and all(lo > 0 for lo, _ in b) and b[2][0] > max(b[0][1], b[1][1]) and b[3][1] < b[2][0] and b[4][0] > b[3][1] for b in [_bounds(c, r) for r in range(c.world)]))
edge("forward:peer_copy:an_owner_receives_nothing_in_a_forward")(lambda c: c.case.flow == "forward_peer" and any(
    sorted(np.nonzero(c.t.outbox_occurrences(0, i) == 0)[0].tolist()) == [2] for i in range(len(c.case.senders[0]))))
edge("forward:wrong_rank_refused")(lambda c: c.case.flow == "forward_peer" and "wrong_rank" in c.case.expect)


# ---- ring -----------------------------------------------------------------------------------------------------------------------------
def ring_schedule(case):
    """(epoch per segment in file order, num_seq of every point) of a ring case, by parallel.rarefaction_schedule over the whole input"""
    from faqcs_amd import parallel

    o = case.opt()
    return parallel.rarefaction_schedule([len(rs) for subs in case.senders for sub in subs for _, rs in sub.segs], o.split_size, o.num_subsample)


def _ring(c):
    return c.case.flow == "ring" and len(c.case.senders) == c.world == 4 and all(len(subs) == 3 for subs in c.case.senders) and \
        [e for subs in c.case.senders for sub in subs for e in sub.epochs()] == ring_schedule(c.case)[0]


edge("ring:curve_completes_mid_run")(lambda c: _ring(c) and len(ring_schedule(c.case)[1]) == c.case.opt().num_subsample and
                                     EPOCH_NONE in c.case.senders[2][2].epochs() and EPOCH_NONE not in c.case.senders[0][2].epochs() and c.case.n_epochs - 1 in _epochs_used(c))
edge("ring:no_scheduled_point")(lambda c: _ring(c) and ring_schedule(c.case)[1] == [] and _epochs_used(c) == [0])
edge("ring:a_key_from_several_senders_in_different_epochs")(lambda c: _ring(c) and _shared_key(c))


def _shared_key(c):
    seen = {}
    for (s, i), d in c.subs():
        for key, e in zip(d["canon"][:2000].tolist(), d["epoch"][:2000].tolist()):
            seen.setdefault(key, set()).add((s, e))
    return any(len({s for s, _ in v}) > 1 and len({e for _, e in v}) > 1 for v in seen.values())


# =====================================================================================================================================
# builders
# =====================================================================================================================================
BASE_READS = reads_of(200, 150, 1)  # two hundred random 150-base reads: at k = 31 every one of the 256 buckets holds an item


def _inv_ord15(o):
    """the 15-mer (30 bits, base i at bits 2 i) whose skm_ord is o"""
    mask = (1 << 30) - 1
    x = o ^ (o >> 14) ^ (o >> 28)
    x = (x * pow(0x9E3779B1, -1, 1 << 30)) & mask
    return x ^ (x >> 15)


_PARTS_OF_ORD = None


def read_in_partition(target, seed):
    """a 31-base read whose only k-mer lies in the 19-bit partition `target`: a 15-mer that comes early in the minimizer order (so that it IS the
    minimizer between random flanks) and whose ord mixes to the partition -- found by walking the orders upwards, skm_ord inverted"""
    global _PARTS_OF_ORD
    if _PARTS_OF_ORD is None:
        _PARTS_OF_ORD = ke.skm_part(np.arange(1 << 23, dtype=U)).astype(np.int32)
    for o in np.nonzero(_PARTS_OF_ORD == target)[0].tolist():
        x = _inv_ord15(o)
        core = bytes(b"ACTG"[(x >> (2 * i)) & 3] for i in range(15))
        for t in range(4):
            s = rb(8, seed + 7 * t) + core + rb(8, seed + 7 * t + 1)
            if int(ke.skm_part(ke.min_ords(s, 31)[0])) == target:
                return s
    raise AssertionError("no read for partition %d" % target)


def owners_cases():
    C = []
    for w in WORLDS:
        claims = ["world=%d:every_bucket_holds_an_item" % w] + ["world=%d:both_buckets_at_the_boundary_of_rank_%d" % (w, r) for r in range(1, w)]
        reads, ranks = list(BASE_READS), []
        if w in OWNER_WORLDS:
            ranks = owner_ranks(w)
            for r in ranks:
                lo, hi = part_range(r, w)
                reads += [rd(read_in_partition(lo, 100 * w + r)), rd(read_in_partition(hi - 1, 5000 + 100 * w + r))]
                claims.append("world=%d:rank_%d_receives_its_first_and_its_last_partition" % (w, r))
        if (w, 31) in K_WORLDS:
            claims.append("world=%d:k=31" % w)
        # (the epochs of the two segments are NOT their run numbers: an outbox that carried the run number would be told at once)
        C.append(XCase("owners_world_%d" % w, "owners", 31, w, 2, [[Sub([(1, reads[:120]), (0, reads[120:])])]], claims, owner_ranks=ranks))
    for w, k in K_WORLDS:
        if k != 31:
            C.append(XCase("owners_world_%d_k%d" % (w, k), "owners", k, w, 2, [[Sub([(1, BASE_READS[:15]), (0, BASE_READS[15:30])])]], ["world=%d:k=%d" % (w, k)],
                           owner_ranks=owner_ranks(w)))
    for w, reads in ((64, BASE_READS), (5, BASE_READS[:40])):
        C.append(XCase("owners_direct_world_%d" % w, "owners", 31, w, 2, [[Sub([(1, reads[:len(reads) // 2]), (0, reads[len(reads) // 2:])])]],
                       ["direct:world=%d:every_destination_holds_a_pair_in_both_epochs" % w], direct_env=True, owner_ranks=owner_ranks(w)))
    both = reads_of(6, 90, 2)
    C.append(XCase("owners_both_strands_two_senders", "owners", 31, 3, 2, [[Sub([(0, both)])], [Sub([(1, [rd(ke.revcomp(r[1])) for r in both])])]],
                   ["both_strands_of_a_key_from_two_senders:one_owner"]))
    half = ke.rb(15, 16000)  # (the palindromic 30-mer of kmer_edges.run_cases)
    pal = half + ke.revcomp(half)
    C.append(XCase("owners_palindrome_k30_two_senders", "owners", 30, 3, 2, [[Sub([(0, [rd(pal)] * 3)])], [Sub([(1, [rd(pal)] * 3)])]], ["k=30:palindromic_key:one_owner"]))
    return C


def epochs_cases():
    C, R = [], lambda n, seed, length=60: reads_of(n, length, seed)
    C.append(XCase("epochs_n1000_item_path", "epochs", 31, 3, 1000, [[Sub([(998, R(10, 10)), (0, R(10, 11)), (999, R(10, 12)), (1, R(10, 13) + R(3, 10))])]],
                   ["n_epochs=1000:epochs_0_1_998_999:item_path"]))
    C.append(XCase("epochs_n1001_direct_path", "epochs", 31, 3, 1001, [[Sub([(1000, R(10, 14)), (0, R(10, 15) + R(3, 14))])]], ["n_epochs=1001:epoch_1000:direct_path"]))
    five = [(e, R(8, 20 + e) + R(2, 20)) for e in (3, 0, 4, 1, 2)]
    C.append(XCase("epochs_direct_env_n5", "epochs", 31, 3, 5, [[Sub(five)], [Sub(five[::-1])]], ["FAQCS_KMER_DIRECT=1:n_epochs=5"], direct_env=True))
    C.append(XCase("epochs_item_twin_n5", "epochs", 31, 3, 5, [[Sub(five)], [Sub(five[::-1])]], ["item_twin_of_the_direct_case"]))
    C.append(XCase("epochs_none_first_middle_last", "epochs", 31, 2, 4, [[Sub([(EPOCH_NONE, R(6, 30)), (0, R(6, 31)), (EPOCH_NONE, R(6, 32)), (2, R(6, 33)), (EPOCH_NONE, R(6, 34))])]],
                   ["EPOCH_NONE_segment_first", "EPOCH_NONE_segment_middle", "EPOCH_NONE_segment_last"]))
    C.append(XCase("epochs_consecutive_segments_one_run", "epochs", 31, 2, 6, [[Sub([(2, R(5, 35)), (2, R(5, 36)), (2, R(5, 37)), (4, R(5, 38))])]],
                   ["consecutive_segments_of_one_epoch_make_one_run"]))
    C.append(XCase("epochs_empty_segments", "epochs", 31, 2, 6, [[Sub([(1, R(5, 40)), (1, []), (1, R(5, 41)), (4, []), (1, R(5, 42)), (2, []), (3, R(5, 43))])]],
                   ["empty_segment_inside_a_run", "empty_segment_of_another_epoch_between_two_of_one", "empty_segment_between_two_epochs"]))
    thousand = [(j & 1, [rd(rb(40, 50000 + j))]) for j in range(KG_MAX_RUNS + 1)]
    C.append(XCase("epochs_1000_runs", "epochs", 31, 2, 2, [[Sub(thousand[:KG_MAX_RUNS])]], ["runs=KG_MAX_RUNS_in_one_submission"]))
    C.append(XCase("epochs_1001_runs_refused", "epochs", 31, 2, 2, [[Sub(thousand, error="more than 1000 runs of segments with one epoch in a submission"), Sub([(1, R(6, 44))])]],
                   ["runs=KG_MAX_RUNS+1:refused_and_the_context_usable"]))
    K, moves = [rd(KEY_READ)], "min_epoch:first_hist_moves_from_7_to_3:total_by_epoch_keeps_both"
    C.append(XCase("min_epoch_7_then_3_two_calls", "epochs", 31, 2, 8, [[Sub([(7, K + R(4, 45))]), Sub([(3, K + R(4, 46))])]], ["min_epoch:7_then_3:two_insert_calls_of_one_sender", moves]))
    C.append(XCase("min_epoch_7_then_3_one_call", "epochs", 31, 2, 8, [[Sub([(7, K + R(4, 47)), (3, K)])]], ["min_epoch:7_then_3:one_insert_call"]))
    C.append(XCase("min_epoch_7_then_3_two_senders", "epochs", 31, 2, 8, [[Sub([(7, K + R(4, 48))])], [Sub([(3, K)])]], ["min_epoch:7_then_3:two_senders", moves]))
    C.append(XCase("min_epoch_equal_two_senders", "epochs", 31, 2, 8, [[Sub([(5, K)])], [Sub([(5, K + R(4, 49))])]], ["min_epoch:equal_epochs_from_two_senders"]))
    C.append(XCase("min_epoch_flush_between_arrivals", "epochs", 31, 1, 8, [[Sub([(7, K)]), Sub([(5, BASE_READS)]), Sub([(3, K)])]],
                   ["min_epoch:a_group_of_2^14_flushed_between_the_arrivals", moves], expect=("flushed",)))
    C.append(XCase("min_epoch_flush_between_arrivals_two_senders", "epochs", 31, 1, 8, [[Sub([(7, K)]), Sub([(5, BASE_READS)])], [Sub([(6, R(4, 51))]), Sub([(3, K)])]],
                   ["min_epoch:a_group_of_2^14_flushed_between_the_arrivals:two_senders", moves], expect=("flushed",)))
    C.append(XCase("min_epoch_one_call_beyond_a_group", "epochs", 31, 1, 8, [[Sub([(7, K), (5, BASE_READS), (3, K)])]],
                   ["min_epoch:7_and_3_in_one_insert_call_beyond_a_group_of_2^14"], expect=("flushed",)))
    return C


def single_kmer_reads(want, seed0, n_each):
    """31-base reads whose one k-mer goes to the destinations `want` = {destination: ...} of a world, n_each per destination"""
    world, dests = want
    out = {d: [] for d in dests}
    for seed in range(seed0, seed0 + 100000):
        s = rb(31, seed)
        d = ((int(ke.skm_part(ke.min_ords(s, 31)[0])) >> 11) * world) >> 8
        if d in out and len(out[d]) < n_each:
            out[d].append(rd(s))
            if all(len(v) == n_each for v in out.values()):
                return [r for d in dests for r in out[d]]
    raise AssertionError("no reads for %s" % (want,))


def outbox_cases():
    C = []
    C.append(XCase("outbox_reads_shorter_than_k", "outbox", 31, 64, 2, [[Sub([(0, reads_of(20, 30, 60)), (1, reads_of(5, 30, 61))])]], ["every_read_shorter_than_k:all_counts_zero"], owner_ranks=[]))
    C.append(XCase("outbox_asked_twice", "outbox", 31, 3, 2, [[Sub([(0, reads_of(10, 80, 62))])]], ["second_outbox_call_returns_zeros"]))
    C.append(XCase("outbox_empty_submission_behind_a_full_one", "outbox", 31, 3, 2, [[Sub([(0, reads_of(10, 80, 63))]), Sub([(1, [])]), Sub([(1, reads_of(3, 80, 64))])]],
                   ["empty_submission_behind_a_full_one"]))
    C.append(XCase("outbox_poly_A_world_64", "outbox", 31, 64, 2, [[Sub([(0, [rd(b"A" * n) for n in (31, 47, 48, 60, 150)] * 4)])]], ["world=64:poly_A_only:one_destination_63_zero_counts"],
                   owner_ranks=[POLY_A_DEST, (POLY_A_DEST + 1) % 64]))
    C.append(XCase("outbox_destinations_0_and_63", "outbox", 31, 64, 2, [[Sub([(0, single_kmer_reads((64, (0, 63)), 70000, 5))])]], ["world=64:destinations_0_and_63_zeros_between"],
                   owner_ranks=[0, 31, 63]))
    spill = ke.partition_cases()[0].subs[0][0]  # 4 400 distinct 31-mers with one minimizer: one bucket, 18 writing blocks of 256 reads
    C.append(XCase("outbox_spill", "outbox", 31, 2, 2, [[Sub([(0, spill[:2200]), (1, spill[2200:])])]], ["spill:one_sub_region_beyond_cap1"], extra=("--min_L", 31)))
    C.append(XCase("outbox_staging_small_large_small", "outbox", 31, 3, 2, [[Sub([(0, BASE_READS[:2])]), Sub([(1, BASE_READS)]), Sub([(0, BASE_READS[100:110])])]],
                   ["staging:small_large_small_submissions_on_one_sender"]))
    return C


def forward_cases():
    a, b = reads_of(150, 150, 80), reads_of(150, 150, 81)
    C = [XCase("forward_in_place", "forward", 31, 3, 4, [[Sub([(0, a[:20])]), Sub([(1, [])]), Sub([(1, a[20:60]), (2, a[:5])]), Sub([(3, a[60:70])])]],
               ["forward:in_place", "forward:behind_an_empty_submission_nothing_moves"], flow="forward")]
    few = single_kmer_reads((3, (0, 1)), 90000, 3)
    subs = [Sub([(0, reads_of(12, 40, 82))]), Sub([(1, reads_of(12, 40, 83))]), Sub([(1, a), (2, b[:20])]), Sub([(2, few)]), Sub([(3, b), (0, a[:20])])]
    C.append(XCase("forward_peer_copy", "forward", 31, 3, 4, [subs], ["forward:peer_copy:five_forwards_to_one_owner_third_beyond_the_capacity",
                                                                     "forward:peer_copy:an_owner_receives_nothing_in_a_forward", "forward:wrong_rank_refused"],
                   flow="forward_peer", expect=("wrong_rank",)))
    return C


def ring_case(name, split, claims):
    pool = reads_of(12, 100, 95)
    senders = [[Sub([(0, reads_of(26, 100, 100 + 10 * s + 2 * i + j) + pool[(s + i + j) % 3::3]) for j in range(2)]) for i in range(3)] for s in range(4)]
    case = XCase(name, "ring", 31, 4, 5, senders, claims, extra=("--split_size", split, "--subset", 4), flow="ring")
    case.n_epochs = case.opt().num_subsample + 1  # (KmerExchange: the segment behind the last point is still counted)
    epochs = iter(ring_schedule(case)[0])
    for subs in senders:
        for sub in subs:
            sub.segs = [(next(epochs), rs) for _, rs in sub.segs]
    return case


def ring_cases():
    return [ring_case("ring_curve_completes_mid_run", 50, ["ring:curve_completes_mid_run", "ring:a_key_from_several_senders_in_different_epochs"]),
            ring_case("ring_no_scheduled_point", 100000, ["ring:no_scheduled_point"])]


def oracle_whole(case):
    """OracleEngine on the counted segments of the case in file order (sender by sender; a ring case: every segment, under its own sampling
    options) -> (points, totals before the table ends, histogram)"""
    from oracle_engine import OracleEngine

    from faqcs_amd import driver
    from faqcs_amd.options import parse_args

    extra = [] if case.flow == "ring" else ["--split_size", str(1 << 30)]
    ora = OracleEngine(parse_args(["-u", "x", "-d", "y", "--kmer_rarefaction"] + case.args() + extra), MAX_READ, IN_OFF)
    for subs in case.senders:
        for sub in subs:
            keep = [] if sub.error else sub.buffers() if case.flow == "ring" else [rs for e, rs in sub.segs if e != EPOCH_NONE]
            if keep:
                ora.process(*driver.pack_segments(keep))
    totals = ora.kmer_totals()
    ora.kmer_end_table()
    points = [tuple(int(x) for x in p) for p in ora.kmer_points()]
    c, n = ora.kmer_histogram()
    ora.close()
    return points, totals, list(zip(c.tolist(), n.tolist()))


def points_of(case, d, t):
    """KmerExchange.finish's rule, restated: the sums over the owners accumulated over the epochs at the scheduled points, or -- with no
    scheduled point -- one point for the whole pass"""
    num_seq = ring_schedule(case)[1] if case.flow == "ring" else []
    d, t = np.cumsum(d), np.cumsum(t)
    total_reads = sum(len(rs) for subs in case.senders for sub in subs if not sub.error for e, rs in sub.segs if case.flow == "ring" or e != EPOCH_NONE)
    return [(int(ns), int(d[i]), int(t[i])) for i, ns in enumerate(num_seq)] or [(total_reads, int(d[-1]), int(t[-1]))]


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = owners_cases() + epochs_cases() + outbox_cases() + forward_cases() + ring_cases()
    return _CASES


def coverage(cases=None):
    """Puts EVERY predicate to EVERY case.  -> ({edge: [cases that reach it]}, {case: [claims that do not hold]}, {case: [edges reached, not claimed]})"""
    cases = all_cases() if cases is None else cases
    table, lost, silent = {e: [] for e in EDGES}, {}, {}
    for c in cases:
        for e, f in EDGES.items():
            if bool(f(c.ctx())):
                table[e].append(c.name)
                if e not in c.claims:
                    silent.setdefault(c.name, []).append(e)
            elif e in c.claims:
                lost.setdefault(c.name, []).append(e)
        for e in c.claims:
            if e not in EDGES:
                lost.setdefault(c.name, []).append(e)
    return table, lost, silent


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t, lost, silent = coverage()
    for e, v in t.items():
        print("%3d  %s" % (len(v), e))
    print("%d cases, %d edges; claims that do not hold: %s" % (len(all_cases()), len(t), lost))
