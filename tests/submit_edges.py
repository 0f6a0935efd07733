"""A constructed catalogue of SCHEDULES for the host orchestration of a context (faqcs_capi.hip: faqcs_submit_async / faqcs_wait /
faqcs_submit_device / faqcs_sync / faqcs_finish / faqcs_counters_export / _import / faqcs_reset_counters / faqcs_set_quality /
faqcs_set_input_quality_offset, and enqueue_trim's one-launch-late composition fold), in the style of tests/pair_edges.py and
tests/kmer_edges.py.  Every other catalogue drives a context as "one submission, then faqcs_sync", which folds the pending composition
records at once; here the submissions follow each other with work in flight, so that the fold of launch k's records happens in the tail
of launch k+1's blocks (comp_fold_tail) or on the aux stream beside it (composition_histogram), the staging slots and the record sets
are reused and regrown, the ticket ring wraps, and the counter block is moved or reset between launches.

A schedule is a list of operations on ONE context:
    ("submit", Batch)            via "host" (faqcs_submit_async, pinned memory, a ticket) or "device" (faqcs_submit_device)
    ("wait", k)                  faqcs_wait on the ticket of the schedule's k-th submission (k past the last one: an unknown ticket)
    ("hostile", k)               the host arenas, offsets and flags of submission k are overwritten (the command line's buffer recycling)
    ("sync",) ("finish",) ("export",) ("import",) ("reset",)
    ("set_quality", q) ("set_offset", o)
    ("tail_fold", "0" | None)    FAQCS_TAIL_FOLD for the submissions behind it (the library reads it at every submission)
    ("expect_error", code)       faqcs_sync must return this code (the error-in-flight schedule ends with it)

expected(schedule) feeds the same batches in the same order to OracleEngine (tests/oracle_engine.py): its block is zeroed at a reset,
set_quality is applied at the same point, a changed input offset is a fresh oracle that carries the block, an import puts back the block
of the last export.  Results and counters are integers: the GPU test compares them for equality, there is no tolerance anywhere.

trace(schedule) restates the HOST rules and nothing else -- record set n_enqueued & 1, slot n_submits & 1, the ticket ring of 8,
DevBuf::reserve's capacity rule, pending_fold / pending_n / pending_wide, and per submission the plan (tests/trim_dispatch_cases.py:
expected_plan, which tests/test_trim_plan.py holds to faqcs_trim_plan.h) -- and predicts the tallies of faqcs_path_tallies_get().  It never
produces an expected count.  Every edge of EDGES is a predicate over a schedule and its trace; coverage() evaluates every predicate on
every schedule.  tests/test_submit_edges_model.py holds the catalogue together without a GPU; tests/test_gpu_submit_edges.py runs it.

    python -m tests.submit_edges        prints the number of schedules per edge
"""
import os
import sys

import numpy as np

try:
    import trim_dispatch_cases as td
except ImportError:  # python -m tests.submit_edges
    from tests import trim_dispatch_cases as td

# ---- the host rules' constants, restated (test_submit_edges_model.py compares them with the sources) -----------------------------------
RING = 8                      # ticket events of a context
N_SLOTS = 2                   # staging slots of the host path
N_RECSETS = 2                 # composition record sets
FOLD_U = 4                    # records per thread and chunk of comp_fold_tail
PER_CLAIM = 5                 # chunks per claim
CELL_MAX = 65535              # what a 16-bit cell of the fold's table takes between two flushes
PAD_BEFORE, PAD_AFTER = 16, 64
STAGE_FRONT = 16              # arena bytes land this far into a staging buffer
TN_SLACK = 64                 # entries behind the n flags of a staged terminal_n
RESERVE_DIV, RESERVE_ADD = 4, 64  # DevBuf::reserve: n + n / 4 + 64

_CAPI, _CTX, _COMMON, _HDR = "faqcs_amd/csrc/faqcs_capi.hip", "faqcs_amd/csrc/faqcs_ctx.h", "faqcs_amd/csrc/faqcs_trim_common.h", "include/faqcs_mi.h"
# name -> [(file, regex, value the groups must give)]
CONSTANT_SOURCES = {
    "RING": [(_CTX, r"hipEvent_t ticket_ev\[(\d+)\]", lambda g: int(g[0])), (_CAPI, r"c->ticket_ev\[c->n_submits & (\d+)\]", lambda g: int(g[0]) + 1),
             (_CAPI, r"if \(c->n_submits >= (\d+)\) \{ HIPCHK\(hipEventSynchronize\(tk\)\)", lambda g: int(g[0])),
             (_CAPI, r"if \(ticket \+ (\d+) < c->n_submits\) return 0;", lambda g: int(g[0])), (_CAPI, r"c->ticket_ev\[ticket & (\d+)\]", lambda g: int(g[0]) + 1)],
    "N_SLOTS": [(_CTX, r"Slot slot\[(\d+)\];", lambda g: int(g[0])), (_CAPI, r"c->slot\[c->n_submits & (\d+)\]", lambda g: int(g[0]) + 1)],
    "N_RECSETS": [(_CTX, r"RecSet rec\[(\d+)\];", lambda g: int(g[0])), (_CAPI, r"const int set = \(int\)\(c->n_enqueued\+\+ & (\d+)\);", lambda g: int(g[0]) + 1)],
    "FOLD_U": [(_COMMON, r"ND = \(NE \+ 1\) / 2, U = (\d+);", lambda g: int(g[0]))],
    "PER_CLAIM": [(_COMMON, r"CHUNK = NT \* U, PER_CLAIM = (\d+), FLUSH_CLAIMS = (\d+)u / \(CHUNK \* PER_CLAIM\);", lambda g: int(g[0]))],
    "CELL_MAX": [(_COMMON, r"CHUNK = NT \* U, PER_CLAIM = (\d+), FLUSH_CLAIMS = (\d+)u / \(CHUNK \* PER_CLAIM\);", lambda g: int(g[1]))],
    "PAD_BEFORE": [(_HDR, r"#define FAQCS_ARENA_PAD_BEFORE (\d+)", lambda g: int(g[0]))],
    "PAD_AFTER": [(_HDR, r"#define FAQCS_ARENA_PAD_AFTER (\d+)", lambda g: int(g[0]))],
    "STAGE_FRONT": [(_CAPI, r"hipMemcpyAsync\(sl\.seq\.p \+ (\d+), b->seq \+ o0, bytes", lambda g: int(g[0])),
                    (_CAPI, r"hipMemcpyAsync\(sl\.qual\.p \+ (\d+), b->qual \+ o0, bytes", lambda g: int(g[0])),
                    (_CAPI, r"d_seq = sl\.seq\.p \+ (\d+) - o0, \*d_qual = sl\.qual\.p \+ (\d+) - o0;", lambda g: int(g[0]) if g[0] == g[1] else -1)],
    "TN_SLACK": [(_CAPI, r"sl\.tn\.reserve\(\(size_t\)n \+ (\d+)\)", lambda g: int(g[0])), (_CAPI, r"\(size_t\)n \+ (\d+) > sl\.tn\.cap", lambda g: int(g[0]))],
    "RESERVE_DIV": [(_CTX, r"const size_t want = n \+ n / (\d+) \+ (\d+);", lambda g: int(g[0]))],
    "RESERVE_ADD": [(_CTX, r"const size_t want = n \+ n / (\d+) \+ (\d+);", lambda g: int(g[1]))],
}
TALLIES = ("folds_tail", "folds_aux", "folds_now", "folds_dropped", "slot_stream_waits", "slot_event_syncs", "recset_fold_waits", "recset_grow_syncs",
           "ticket_ring_waits")
E_INVAL, E_QUALITY, F_ERR_QUALITY = -1, -3, 0x100
SETTINGS = ("lds", "single_pass")  # single_pass: FAQCS_TRIM_LDS=0, read once per process -- those schedules run in one child process
MI355X_CU = 256
ACGT = np.frombuffer(b"ACGT", np.uint8)
N, HOSTILE_Q = ord("N"), ord("~")


def reserve(cap, n):
    """DevBuf::reserve: the capacity behind it"""
    return cap if n <= cap else n + n // RESERVE_DIV + RESERVE_ADD


def fold_geometry(NW):
    """CHUNK, F of the issue: records per chunk of a folding block of NW waves, and records between two flushes of a block that claims alone"""
    chunk = FOLD_U * 64 * NW
    return chunk, CELL_MAX // (chunk * PER_CLAIM) * PER_CLAIM * chunk


# =====================================================================================================================================
# batches
# =====================================================================================================================================

class Batch:
    """One submission's reads as arenas (seq, qual: the window's bytes; lens) and how it is handed over."""

    def __init__(self, seq, qual, lens, via="host", o0=0, tn=False, results=True, kind=""):
        self.seq, self.qual = np.ascontiguousarray(seq, np.uint8), np.ascontiguousarray(qual, np.uint8)
        self.lens = np.asarray(lens, np.int64)
        self.n = len(self.lens)
        self.offset = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint32)
        self.total = int(self.offset[-1])
        assert len(self.seq) == len(self.qual) == self.total
        self.longest = int(self.lens.max()) if self.n else 0
        self.via, self.o0, self.tn, self.results, self.kind = via, o0, tn, results, kind
        self.seg = np.array([0, self.n], np.uint32)

    def but(self, **kw):
        import copy

        b = copy.copy(self)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def terminal_n(self):
        """faqcs_batch.terminal_n: bit 0 = the first base is an upper-case N, bit 1 = the last one is"""
        if not self.total:
            return np.zeros(self.n, np.uint8)
        off, nz = self.offset.astype(np.int64), self.lens > 0
        first = self.seq[np.minimum(off[:-1], self.total - 1)] == N
        last = self.seq[np.maximum(off[1:] - 1, 0)] == N
        return (first & nz).astype(np.uint8) | ((last & nz).astype(np.uint8) << 1)

    def n_counts(self):
        """N (upper case) per read"""
        if "_c_n_counts" not in self.__dict__:
            c = np.concatenate([[0], np.cumsum(self.seq == N)])
            self.__dict__["_c_n_counts"] = c[self.offset[1:]] - c[self.offset[:-1]]
        return self.__dict__["_c_n_counts"]

    def identical(self):
        if "_c_identical" not in self.__dict__:
            self.__dict__["_c_identical"] = self._identical()
        return self.__dict__["_c_identical"]

    def _identical(self):
        return self.n > 1 and len(set(self.lens.tolist())) == 1 and bool((self.seq.reshape(self.n, -1) == self.seq[:self.longest]).all()) and \
            bool((self.qual.reshape(self.n, -1) == self.qual[:self.longest]).all())

    def host_arenas(self):
        """What the host path is given: the batch as a WINDOW [o0, o0 + total) of a larger arena, with N and qualities above 41 -- bytes that would
        change results and raise FAQCS_E_QUALITY if they were ever interpreted -- directly in front of and behind the window.  -> seq, qual, offsets"""
        s = np.full(self.o0 + self.total + PAD_AFTER, N, np.uint8)
        q = np.full(self.o0 + self.total + PAD_AFTER, HOSTILE_Q, np.uint8)
        s[self.o0:self.o0 + self.total], q[self.o0:self.o0 + self.total] = self.seq, self.qual
        return s, q, (self.offset.astype(np.int64) + self.o0).astype(np.uint32)

    def device_arenas(self, front=64):
        """What faqcs_submit_device is given: the arenas with `front` hostile bytes before and PAD_AFTER and more behind -> seq, qual, front"""
        s = np.full(front + self.total + 2 * PAD_AFTER, N, np.uint8)
        q = np.full(front + self.total + 2 * PAD_AFTER, HOSTILE_Q, np.uint8)
        s[front:front + self.total], q[front:front + self.total] = self.seq, self.qual
        return s, q, front


def make(seed, n, L, shape="ragged", n_mode="some", qual="headline", in_off=33, plant=None, **kw):
    """n seeded reads whose longest has exactly L bases.
    shape   ragged: L - 37 ... L bases, the first read L | equal | same: one read n times
    n_mode  some: an N at 0.5 % of the bases | none | lanes: read i holds i % 64 of them (every lane of a folding wave another count)
    qual    headline: 30 ... 40 with a tail of 2 from a random point on | reject: 2 everywhere (no read survives: post-trim records without
            CR_VALID) | mixed: every other read rejected
    plant   a list of target strings: a third of the reads carry a piece of one"""
    rng = np.random.Generator(np.random.PCG64([seed, n, L]))
    if shape == "ragged":
        lens = rng.integers(max(1, L - 37), L + 1, n)
        if n:
            lens[0] = L
    else:
        lens = np.full(n, L, np.int64)
    m = 1 if shape == "same" and n else n
    lens_m = lens[:m]
    total = int(lens_m.sum())
    off = np.concatenate([[0], np.cumsum(lens_m)])
    read_of = np.repeat(np.arange(m), lens_m)
    pos = np.arange(total) - off[read_of]
    seq = ACGT[rng.integers(0, 4, total)].copy()
    if n_mode == "some":
        seq[rng.random(total) < 0.005] = N
    elif n_mode == "lanes":
        want = (np.arange(m) % 64)[read_of]
        seq[(pos < 2 * want) & (pos % 2 == 1)] = N   # every other base from the front: want N in a read of at least 2 want bases
    q = rng.integers(30, 41, total)
    brk = rng.integers(lens_m // 2, lens_m + 41)[read_of] if m else np.zeros(0, np.int64)
    q[pos >= brk] = 2
    if qual == "reject":
        q[:] = 2
    elif qual == "mixed":
        q[read_of % 2 == 1] = 2
    if plant:
        for i in range(0, m, 3):
            t = np.frombuffer(plant[int(rng.integers(0, len(plant)))].upper().encode(), np.uint8)
            t = t[np.isin(t, ACGT)][:40]
            if int(lens_m[i]) > len(t) + 8 and len(t) >= 12:
                p = int(rng.integers(4, int(lens_m[i]) - len(t)))
                seq[off[i] + p:off[i] + p + len(t)] = t
    if shape == "same" and n:
        seq, q = np.tile(seq, n), np.tile(q, n)
    return Batch(seq, (q + in_off).astype(np.uint8), lens, kind="%s/%s/%s" % (shape, n_mode, qual), **kw)


def _tests_on_path():
    """tests/ and tests/golden/ importable, as tests/conftest.py makes them (python -m tests.submit_edges has no conftest)"""
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here, os.path.join(here, "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)


def empty(**kw):
    return Batch(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.int64), kind="empty", **kw)


def error_batch(seed, n, at, **kw):
    """n reads of up to 150 bases; read `at` is the quality-above-41 read of the golden case err_quality_above_41 (tests/golden/make_fixtures.py,
    "errq": read 57 of adversarial(200, seed=31) with a '~' as its fourth quality) -- a legitimate input that the reference throws on"""
    _tests_on_path()
    import make_fixtures

    _, sq, q = make_fixtures.adversarial(200, seed=31)[0][57]
    q = q[:3] + b"~" + q[4:]
    b = make(seed, n, 150)
    lens = b.lens.copy()
    off = b.offset.astype(np.int64)
    seq = np.concatenate([b.seq[:off[at]], np.frombuffer(sq, np.uint8), b.seq[off[at + 1]:]])
    qual = np.concatenate([b.qual[:off[at]], np.frombuffer(q, np.uint8), b.qual[off[at + 1]:]])
    lens[at] = len(sq)
    return Batch(seq, qual, lens, kind="error at %d" % at, **kw)


# =====================================================================================================================================
# schedules, the trace
# =====================================================================================================================================

class Schedule:
    def __init__(self, name, family, ops, args=(), R=304, in_off=33, setting="lds", library=0):
        self.name, self.family, self.args, self.R, self.in_off, self.setting, self.library = name, family, tuple(args), R, in_off, setting, library
        ops = list(ops)
        if not any(op[0] == "expect_error" for op in ops) and ops[-1][0] != "finish":
            ops.append(("finish",))
        self.ops = ops
        self.batches = [op[1] for op in ops if op[0] == "submit"]
        self._expected = None
        assert max([b.longest for b in self.batches] or [0]) <= R

    def opt(self):
        from faqcs_amd.options import parse_args

        opt = parse_args(["-u", "x", "-d", "y"] + list(self.args))
        if self.library:
            opt.adapter = library(self.library)
        return opt

    def option_fields(self):
        o = td.option_fields(list(self.args))
        return dict(o, has_adapters=1) if self.library else o

    def switches(self):
        return dict(td.DEFAULT_SWITCHES, lds_on=0 if self.setting == "single_pass" else 1)

    def n_reads(self):
        return sum(b.n for b in self.batches)

    def expected(self):
        if self._expected is None:
            self._expected = expected(self)
        return self._expected


def library(n):
    """The smallest library that runs in groups (tests/test_gpu_adapter_library.py: more than 64 targets): its seeded 65-target one"""
    _tests_on_path()
    from test_gpu_adapter_library import random_library

    return random_library(np.random.Generator(np.random.PCG64([61, n])), n)


class Trace:
    def __init__(self):
        self.subs, self.waits, self.now, self.dropped, self.hostile = [], [], [], 0, []
        self.tallies = dict.fromkeys(TALLIES, 0)
        self.plan_queries = []  # (options, max_len, n, n_cu, switches, the plan trace() assumed): held to tools/trim_plan_check.cpp


def trace(s, ring=RING, n_slots=N_SLOTS, pending_on=True, n_cu=MI355X_CU):
    """The host rules of faqcs_capi.hip over a schedule.  ring / n_slots / pending_on are the MUTATIONS of test_submit_edges_model.py: a ring of
    4, one slot, a fold that is never pending -- each must lose edges, which shows that the predicates look at the trace."""
    T = Trace()
    t = T.tallies
    n_submits = n_enqueued = 0
    slots = [dict(seq=0, off=0, tn=0, used=False, bytes=None) for _ in range(n_slots)]
    rec = [dict(cap=0, used=False) for _ in range(N_RECSETS)]
    res_cap = 0
    pending = None    # (set, n, wide, index of the writing submission)
    tail_env = None
    synced = True     # nothing in flight since the last call that waits for the compute stream
    tickets = {}      # index of a host submission among all submissions -> its ticket
    for at, op in enumerate(s.ops):
        kind = op[0]
        if kind == "tail_fold":
            tail_env = op[1]
        elif kind == "submit":
            b = op[1]
            r = dict(index=len(T.subs), op=at, batch=b, via=b.via, n=b.n, max_len=b.longest, slot=None, slot_arm=None, ring_wait=False, res_grow=False, res_regrow=False,
                     set=None, fold=None, fold_n=0, fold_wide=False, writer=None, rec_wait=False, rec_grow=False, rec_regrow=False, kernel=None, tail_env=tail_env,
                     unsynced_behind=not synced, slot_prev_bytes=None, ticket=None)
            if b.via == "host":
                need_seq = b.total + PAD_BEFORE + PAD_AFTER
                sl = slots[n_submits % n_slots]
                r["slot"], r["slot_prev_bytes"] = n_submits % n_slots, sl["bytes"]
                if n_submits >= ring:
                    r["ring_wait"] = True
                    t["ticket_ring_waits"] += 1
                if sl["used"]:
                    if need_seq > sl["seq"] or b.n + 1 > sl["off"] or (b.tn and b.n + TN_SLACK > sl["tn"]):
                        r["slot_arm"] = "grow"
                        t["slot_event_syncs"] += 1
                    else:
                        r["slot_arm"] = "wait"
                        t["slot_stream_waits"] += 1
                else:
                    r["slot_arm"] = "first"
                sl["seq"], sl["off"] = reserve(sl["seq"], need_seq), reserve(sl["off"], b.n + 1)
                if b.tn:
                    sl["tn"] = reserve(sl["tn"], b.n + TN_SLACK)
                r["res_grow"], r["res_regrow"] = b.n + 1 > res_cap, b.n + 1 > res_cap > 0
                res_cap = reserve(res_cap, b.n + 1)
                sl["used"], sl["bytes"] = True, b.total
                r["ticket"] = tickets[r["index"]] = n_submits
                n_submits += 1
            if b.n:
                offer = pending is not None and not pending[2] and tail_env != "0"
                o = dict(s.option_fields(), fold_n=pending[1] if offer else 0)
                plan = td.expected_plan(o, b.longest, b.n, n_cu, s.switches())
                T.plan_queries.append((o, b.longest, b.n, n_cu, s.switches(), plan))
                r.update(kernel=plan["kernel"], NW=plan["NW"], LPR=plan["LPR"], RPC=plan["RPC"], grid=plan["grid"], wide=bool(plan["wide_records"]),
                         folds_tail=bool(plan["folds_tail"]), records_needed=plan["records_needed"])
                k = n_enqueued % N_RECSETS
                n_enqueued += 1
                r["set"] = k
                if rec[k]["used"]:
                    r["rec_wait"], rec[k]["used"] = True, False
                    t["recset_fold_waits"] += 1
                if plan["records_needed"] > rec[k]["cap"]:
                    r["rec_grow"], r["rec_regrow"] = True, rec[k]["cap"] > 0
                    t["recset_grow_syncs"] += 1
                rec[k]["cap"] = reserve(rec[k]["cap"], plan["records_needed"])
                if pending is not None:
                    r["fold_n"], r["fold_wide"], r["writer"] = pending[1], pending[2], pending[3]
                    if plan["folds_tail"]:
                        r["fold"] = "tail"
                        t["folds_tail"] += 1
                    else:
                        r["fold"] = "aux"
                        rec[pending[0]]["used"] = True
                        t["folds_aux"] += 1
                    pending = None
                if plan["kernel"] != "trim_long" and pending_on:
                    pending = (k, b.n, bool(plan["wide_records"]), r["index"])
                synced = False
            T.subs.append(r)
        elif kind == "wait":
            k = op[1]
            if k not in tickets:
                T.waits.append(dict(op=at, sub=k, arm="unknown", in_flight=0))
            else:
                tk = tickets[k]
                arm = "recycled" if tk + ring < n_submits else "event"
                T.waits.append(dict(op=at, sub=k, ticket=tk, arm=arm, boundary=tk + ring == n_submits, in_flight=len(T.subs) - 1 - k))
        elif kind == "hostile":
            T.hostile.append(dict(op=at, sub=op[1], later=sum(1 for o2 in s.ops[at + 1:] if o2[0] == "submit")))
        elif kind in ("sync", "finish", "export", "import", "expect_error"):
            if pending is not None:
                T.now.append(dict(op=at, by="sync" if kind == "expect_error" else kind, writer=pending[3], n=pending[1], wide=pending[2]))
                t["folds_now"] += 1
                pending = None
            synced = True
        elif kind == "reset":
            if pending is not None:
                T.dropped += 1
                t["folds_dropped"] += 1
                pending = None
        elif kind == "set_offset":
            synced = True  # (drains the three streams; what is pending stays pending)
        elif kind == "set_quality":
            pass
        else:
            raise AssertionError(kind)
    return T


# =====================================================================================================================================
# the expected values: OracleEngine, fed the same batches in the same order
# =====================================================================================================================================

def expected(s, alone=False):
    """-> dict(results=[per submission, None behind an error], blocks={op index: block at that finish / export}, error=(submission, code) or None).
    alone=True: the ADDITIVE statement instead -- every submission on a fresh oracle of its own, the blocks summed since the last reset."""
    from oracle_engine import OracleEngine

    from faqcs_amd.engine import FaqcsError

    opt = s.opt()
    in_off, quality = s.in_off, opt.quality

    def fresh():
        o = OracleEngine(opt, s.R, in_off)
        o.set_quality(quality)
        return o

    ora = fresh()
    total = np.zeros(ora.n_counters, np.uint64)
    out = dict(results=[], blocks={}, error=None)
    saved = None
    again = {}  # the same Batch object once more under the same settings: its results and what it added to the block, not computed twice
    for at, op in enumerate(s.ops):
        kind = op[0]
        if kind == "submit":
            b = op[1]
            if out["error"]:
                out["results"].append(None)
                continue
            if (id(b), in_off, quality) in again:
                res, delta = again[id(b), in_off, quality]
                out["results"].append(res)
                ora.block += delta
                total += delta
                continue
            one = fresh() if alone else ora
            before = one.block.copy()
            try:
                out["results"].append(one.process(b.seq if b.total else np.zeros(1, np.uint8), b.qual if b.total else np.zeros(1, np.uint8), b.offset, b.seg))
                again[id(b), in_off, quality] = (out["results"][-1], one.block - before)
            except FaqcsError as x:
                out["error"] = (len(out["results"]), x.code)
                out["results"].append(None)
            if alone:
                total += one.block
                one.close()
        elif kind == "set_quality":
            quality = op[1]
            ora.set_quality(quality)
        elif kind == "set_offset":
            block = ora.block.copy()
            ora.close()
            in_off = op[1]
            ora = fresh()
            ora.block[:] = block
        elif kind == "reset":
            ora.block[:] = 0
            total[:] = 0
        elif kind in ("finish", "export"):
            out["blocks"][at] = total.copy() if alone else ora.block.copy()
            if kind == "export":
                saved = out["blocks"][at]
        elif kind == "import":
            ora.block[:] = saved
            total[:] = saved
    ora.close()
    return out


# =====================================================================================================================================
# the edges: predicates over (schedule, trace)
# =====================================================================================================================================
FOLD_NS = ("1", "63", "CHUNK-1", "CHUNK", "CHUNK+1", "5CHUNK", "5CHUNK+1", "F-1", "F", "F+1", "65535", "65536", "65537")


def fold_n_value(name, NW):
    chunk, F = fold_geometry(NW)
    return {"1": 1, "63": 63, "CHUNK-1": chunk - 1, "CHUNK": chunk, "CHUNK+1": chunk + 1, "5CHUNK": 5 * chunk, "5CHUNK+1": 5 * chunk + 1, "F-1": F - 1, "F": F,
            "F+1": F + 1, "65535": 65535, "65536": 65536, "65537": 65537}[name]


def _folds(T, arm=None):
    """(writer, folder) records of the launches whose fold happened at a later launch"""
    return [(T.subs[r["writer"]], r) for r in T.subs if r["fold"] and (arm is None or r["fold"] == arm)]


def _default(s):
    return s.option_fields() == dict(td.DEFAULT_OPTIONS) and s.setting == "lds"


def _one_chunk(f):
    return f["kernel"] == "trim_lds" and f["grid"] == 1 and f["n"] <= f["RPC"]


def _writer_kind(w):
    if w["kernel"] == "trim_filter_accumulate" and not w["wide"]:
        return "tfa"
    if w["kernel"] != "trim_lds":
        return None
    return "52" if w["max_len"] <= 52 else "77-104" if 77 <= w["max_len"] <= 104 else "153-252" if 153 <= w["max_len"] <= 252 else None


def _record_shape(w, shape):
    b = w["batch"]
    if shape == "identical, past a 16-bit cell":
        return b.n > CELL_MAX and b.identical()
    if shape == "another N count in every lane":
        return b.n >= 64 and len(set(b.n_counts()[:64].tolist())) == 64
    if shape == "no N in any read":
        return b.n >= 64 and int(b.n_counts().sum()) == 0
    if shape == "records without CR_VALID":
        return b.n >= 64 and b.total > 0 and bool((b.qual == 2 + 33).all())  # (a score of 2 everywhere: nothing is kept of any read)
    raise AssertionError(shape)


RECORD_SHAPES = ("identical, past a 16-bit cell", "another N count in every lane", "no N in any read", "records without CR_VALID")


def _runs_unsynced(T, arm, length):
    """`length` launches in a row, none with a sync in front of it but the first, the later ones all folding by `arm`"""
    trims = [r for r in T.subs if r["n"]]
    for i in range(len(trims) - length + 1):
        run = trims[i:i + length]
        if all(r["fold"] == arm and r["unsynced_behind"] for r in run[1:]):
            return True
    return False


def _edges():
    E = {}
    for v in FOLD_NS:
        E["tail: fold_n = %s, a folding launch of one chunk (grid 1)" % v] = lambda s, T, v=v: _default(s) and any(
            _one_chunk(f) and f["fold_n"] == fold_n_value(v, f["NW"]) for _, f in _folds(T, "tail"))
    for v in ("F+1", "65537"):
        E["tail: fold_n = %s, a folding launch of hundreds of chunks (the halves of the grid meet)" % v] = lambda s, T, v=v: _default(s) and any(
            f["grid"] >= 16 and f["n"] >= 200 * f["RPC"] and f["fold_n"] == fold_n_value(v, f["NW"]) for _, f in _folds(T, "tail"))
    for arm in ("tail", "aux"):
        for shape in RECORD_SHAPES:
            E["%s: %s" % (arm, shape)] = lambda s, T, arm=arm, shape=shape: any(
                _record_shape(w, shape) and (arm == "tail" or f["tail_env"] == "0") and (shape != "identical, past a 16-bit cell" or arm == "aux" or _one_chunk(f))
                for w, f in _folds(T, arm))
        for wk in ("52", "77-104", "153-252"):
            E["%s: records written by trim_lds at %s bases" % (arm, wk)] = lambda s, T, arm=arm, wk=wk: any(
                _writer_kind(w) == wk and (arm == "tail" or f["tail_env"] == "0") for w, f in _folds(T, arm))
    # (with FAQCS_TRIM_LDS=0 no launch of the process is a trim_lds one: the records of trim_filter_accumulate never meet a tail that folds)
    E["aux: one-word records written by trim_filter_accumulate (FAQCS_TRIM_LDS=0)"] = lambda s, T: s.setting == "single_pass" and any(
        _writer_kind(w) == "tfa" and f["kernel"] == "trim_filter_accumulate" for w, f in _folds(T, "aux"))
    E["tail: three launches in a row without a sync (set A again at launch k+2, ordered by the compute stream alone)"] = lambda s, T: _runs_unsynced(T, "tail", 3)
    E["tail: four launches in a row without a sync"] = lambda s, T: _runs_unsynced(T, "tail", 4)
    E["tail: a record set regrown at launch k+2 with its reader in flight"] = lambda s, T: any(
        r["rec_regrow"] and r["unsynced_behind"] and r["fold"] == "tail" and r["index"] >= 2 and T.subs[r["index"] - 1]["fold"] == "tail" for r in T.subs)
    E["tail: the folder runs --adapter (the plan lets it fold)"] = lambda s, T: s.option_fields()["has_adapters"] == 1 and bool(_folds(T, "tail"))
    for lo, hi in ((105, 152), (153, 252)):  # the shapes whose blocks own the LDS the fold's table needs (faqcs_trim_plan.h: lds_tail_folds_v)
        E["tail: the folder has the shape of %d ... %d bases" % (lo, hi)] = lambda s, T, lo=lo, hi=hi: any(lo <= f["max_len"] <= hi for _, f in _folds(T, "tail"))
    for lo, hi in ((1, 52), (53, 76), (77, 104), (253, 304)):  # ... and the trim_lds shapes that cannot fold: too little LDS, or two-word records
        E["aux: one-word records offered to a folder of %d ... %d bases, which cannot fold" % (lo, hi)] = lambda s, T, lo=lo, hi=hi: any(
            f["kernel"] == "trim_lds" and lo <= f["max_len"] <= hi and not f["fold_wide"] and f["tail_env"] != "0" for _, f in _folds(T, "aux"))
    E["aux: the folder is trim_filter_accumulate by its length"] = lambda s, T: s.setting == "lds" and any(
        f["kernel"] == "trim_filter_accumulate" and f["max_len"] > 304 and f["tail_env"] != "0" for _, f in _folds(T, "aux"))
    E["aux: the folder is trim_long"] = lambda s, T: any(f["kernel"] == "trim_long" for _, f in _folds(T, "aux"))
    for ww in (False, True):
        for fw in (False, True):
            E["aux: %s-word records beside a launch that writes %s-word ones" % ("two" if ww else "one", "two" if fw else "one")] = lambda s, T, ww=ww, fw=fw: any(
                w["wide"] == ww and f["kernel"] != "trim_long" and f["wide"] == fw and (ww or f["LPR"] == 16 or f["tail_env"] == "0") for w, f in _folds(T, "aux"))
    E["aux: two-word records in front of a shape that folds one-word ones (not offered)"] = lambda s, T: any(
        f["fold_wide"] and f["kernel"] == "trim_lds" and 77 <= f["max_len"] <= 152 and f["tail_env"] != "0" for _, f in _folds(T, "aux"))
    E["aux: a record set reused at k+2 while its fold may still run (the wait for `folded`)"] = lambda s, T: any(r["rec_wait"] and r["unsynced_behind"] for r in T.subs)
    E["aux: a record set reused at k+2 behind a fold of more than 65 535 records beside a launch of one chunk (the fold outlasts the launch)"] = lambda s, T: any(
        r["rec_wait"] and r["unsynced_behind"] and r["n"] > CELL_MAX and T.subs[r["index"] - 1]["fold"] == "aux" and T.subs[r["index"] - 1]["fold_n"] > CELL_MAX
        and T.subs[r["index"] - 1]["n"] <= 64 for r in T.subs if r["index"] >= 2)
    E["aux: trim_long in the middle (no records, the record array is its scratch)"] = lambda s, T: any(
        r["kernel"] == "trim_long" and r["fold"] == "aux" and i + 1 < len(T.subs) and T.subs[i + 1]["n"] and T.subs[i + 1]["fold"] is None and T.subs[i + 1]["unsynced_behind"]
        for i, r in enumerate(T.subs))
    for by in ("sync", "finish", "export", "import"):
        E["now: the last launch's records folded by %s" % by] = lambda s, T, by=by: any(x["by"] == by for x in T.now)
    E["dropped: the last launch's records dropped by reset, launches behind it"] = lambda s, T: T.dropped > 0 and any(
        op[0] == "reset" and any(o2[0] == "submit" for o2 in s.ops[i + 1:]) for i, op in enumerate(s.ops))
    E["dropped: reset behind an aux fold that may still run"] = lambda s, T: any(
        op[0] == "reset" and [r for r in T.subs if r["op"] < i][-1:] and [r for r in T.subs if r["op"] < i][-1]["fold"] == "aux" and T.dropped for i, op in enumerate(s.ops))

    def run_of_host(s):
        """the longest run of host submissions without a wait or a sync between them"""
        best = run = 0
        for op in s.ops:
            if op[0] == "submit" and op[1].via == "host":
                run += 1
                best = max(best, run)
            elif op[0] in ("wait", "sync", "finish", "export", "import", "set_offset", "expect_error"):
                run = 0
        return best

    for k in (1, 2, 3, 8, 9, 16, 17):
        E["host: %d submissions without a wait" % k] = lambda s, T, k=k: run_of_host(s) == k and s.family == "host"
    E["host: results behind faqcs_wait alone, later submissions in flight"] = lambda s, T: any(w["arm"] == "event" and w["in_flight"] > 0 for w in T.waits)
    E["host: the arenas of a waited-for batch overwritten, submissions behind it"] = lambda s, T: any(
        h["later"] > 0 and any(w["sub"] == h["sub"] and w["op"] < h["op"] for w in T.waits) for h in T.hostile)
    E["host: ticket + 8 == n_submits"] = lambda s, T: any(w["arm"] == "event" and w["boundary"] for w in T.waits)
    E["host: ticket + 8 < n_submits (its event has been recycled)"] = lambda s, T: any(w["arm"] == "recycled" for w in T.waits)
    E["host: a recycled ticket waited for with sixteen large submissions in flight (only the ring's wait has made it true)"] = lambda s, T: any(
        w["arm"] == "recycled" and w["ticket"] >= 7 and len(T.subs) >= 16 and all(r["n"] >= 200000 and r["via"] == "host" for r in T.subs) and
        not any(o2[0] in ("wait", "sync", "finish") for o2 in s.ops[:w["op"]]) for w in T.waits)
    E["host: an unknown ticket, the context used afterwards"] = lambda s, T: any(
        w["arm"] == "unknown" and any(o2[0] == "submit" for o2 in s.ops[w["op"] + 1:]) for w in T.waits)
    E["host: the ticket ring wraps (the host waits for submission k-8)"] = lambda s, T: any(r["ring_wait"] for r in T.subs)
    for slot in range(N_SLOTS):
        E["host: slot %d reused with equal size" % slot] = lambda s, T, slot=slot: any(
            r["slot"] == slot and r["slot_arm"] == "wait" and r["slot_prev_bytes"] == r["batch"].total > 0 for r in T.subs)
        E["host: slot %d reused with a smaller batch" % slot] = lambda s, T, slot=slot: any(
            r["slot"] == slot and r["slot_arm"] == "wait" and 0 < r["batch"].total < r["slot_prev_bytes"] for r in T.subs)
        E["host: slot %d regrown with its kernels in flight" % slot] = lambda s, T, slot=slot: any(
            r["slot"] == slot and r["slot_arm"] == "grow" and r["unsynced_behind"] for r in T.subs)
    E["host: the shared result buffer regrown"] = lambda s, T: any(r["res_regrow"] and r["unsynced_behind"] for r in T.subs)
    for o0 in (0, 1, 15, 16, 17, 3000):
        E["host: offset[0] = %d" % o0] = lambda s, T, o0=o0: any(r["via"] == "host" and r["n"] and r["batch"].o0 == o0 for r in T.subs)
    E["host: terminal_n given, then not, then given"] = lambda s, T: any(
        [r["batch"].tn for r in T.subs[i:i + 3]] == [True, False, True] and all(r["via"] == "host" and r["n"] for r in T.subs[i:i + 3]) for i in range(len(T.subs) - 2))
    E["host: a submission without reads between full ones"] = lambda s, T: any(
        T.subs[i]["n"] and not T.subs[i + 1]["n"] and T.subs[i + 2]["n"] and T.subs[i + 2]["unsynced_behind"] and T.subs[i + 1]["via"] == "host" for i in range(len(T.subs) - 2))
    E["host: results == NULL"] = lambda s, T: any(r["via"] == "host" and r["n"] and not r["batch"].results for r in T.subs)
    E["host: host and device submissions interleaved"] = lambda s, T: any(
        [r["via"] for r in T.subs[i:i + 4]] in (["host", "device", "host", "device"], ["device", "host", "device", "host"]) and all(r["unsynced_behind"] for r in T.subs[i + 1:i + 4])
        for i in range(len(T.subs) - 3))

    def between_unsynced(s, T, kind):
        """an operation of `kind` with a launch in front of it and one behind it, no sync in between"""
        for i, op in enumerate(s.ops):
            if op[0] == kind:
                before = [r for r in T.subs if r["op"] < i and r["n"]]
                after = [r for r in T.subs if r["op"] > i and r["n"]]
                if before and after and (after[0]["unsynced_behind"] or kind == "set_offset") and not any(
                        o2[0] in ("sync", "finish", "export", "import") for o2 in s.ops[before[-1]["op"]:i]):
                    return len(before) if kind != "set_offset" else (2 if len(before) >= 2 and before[-1]["unsynced_behind"] else 0)
        return 0

    E["settings: set_quality between two launches that are not synced"] = lambda s, T: between_unsynced(s, T, "set_quality") >= 1
    E["settings: set_input_quality_offset behind two launches that are not synced"] = lambda s, T: between_unsynced(s, T, "set_offset") >= 2
    E["settings: --adapter --polyA, growing and shrinking submissions without a sync"] = lambda s, T: "--polyA" in s.args and not s.library and _grows_and_shrinks(T)
    E["settings: a target library that runs in groups, growing and shrinking submissions without a sync"] = lambda s, T: s.library > 64 and _grows_and_shrinks(T)
    E["error: a quality above 41 in submission j of five without a sync"] = lambda s, T: any(op[0] == "expect_error" and op[1] == E_QUALITY for op in s.ops) and \
        len(T.subs) == 5 and all(r["unsynced_behind"] for r in T.subs[1:]) and any(r["batch"].kind.startswith("error") for r in T.subs[1:4])
    return E


def _grows_and_shrinks(T):
    ns = [r["n"] for r in T.subs]
    return len(ns) >= 4 and all(r["unsynced_behind"] for r in T.subs[1:]) and any(a < b for a, b in zip(ns, ns[1:])) and any(a > b for a, b in zip(ns, ns[1:])) \
        and max(ns) > 4 * min(ns)


EDGES = _edges()


# =====================================================================================================================================
# the schedules
# =====================================================================================================================================
S = lambda b: ("submit", b)
W = lambda k: ("wait", k)
SYNC, FINISH, EXPORT, IMPORT, RESET = ("sync",), ("finish",), ("export",), ("import",), ("reset",)
NO_TAIL, TAIL = ("tail_fold", "0"), ("tail_fold", None)
FOLDER_NW = 12  # waves of a block of the 105 ... 152-base shape, the folding launch of the fold_n schedules (the trace asserts it)


def folder(seed, via="device"):
    """The folding launch of ONE chunk: 64 reads of 114 ... 150 bases"""
    return make(seed, 64, 150, via=via)


def tail_schedules():
    out = []
    for i, v in enumerate(FOLD_NS):
        n = fold_n_value(v, FOLDER_NW)
        out.append(Schedule("tail_fold_n_%s" % v, "tail_n", [S(make(100 + i, n, 30, via="device")), S(folder(200 + i))]))
    for i, v in enumerate(("F+1", "65537")):
        n = fold_n_value(v, FOLDER_NW)
        out.append(Schedule("tail_fold_n_%s_wide_grid" % v, "tail_big", [S(make(120 + i, n, 30, via="device")), S(make(220 + i, 300 * 64, 110, via="device"))]))
    return out


def record_schedules():
    out = []
    for arm, env in (("tail", TAIL), ("aux", NO_TAIL)):
        out.append(Schedule("%s_identical_65537" % arm, "records", [env, S(make(300, 65537, 30, shape="same", n_mode="none", via="device")), S(folder(301))]))
        out.append(Schedule("%s_n_count_per_lane" % arm, "records", [env, S(make(302, 640, 140, shape="equal", n_mode="lanes", via="device")), S(folder(303))]))
        out.append(Schedule("%s_no_n" % arm, "records", [env, S(make(304, 700, 100, n_mode="none", via="device")), S(folder(305))]))
        out.append(Schedule("%s_rejected" % arm, "records", [env, S(make(306, 700, 100, qual="reject", via="device")), S(make(307, 500, 120, qual="mixed", via="device")), S(folder(308))]))
        for L in (40, 100, 200):
            out.append(Schedule("%s_writer_%d" % (arm, L), "records", [env, S(make(310 + L, 700, L, via="device")), S(folder(311 + L))]))
    out.append(Schedule("aux_writer_tfa", "single_pass", [S(make(330, 700, 100, via="device")), S(make(331, 64, 150, via="host")), S(make(332, 300, 40, via="device")), S(make(333, 300, 70, via="device"))], setting="single_pass"))
    return out


def chain_schedules():
    d = lambda seed, n, L, **kw: make(seed, n, L, via="device", **kw)
    return [
        Schedule("tail_three_in_a_row", "chains", [S(d(400, 700, 150)), S(d(401, 650, 150)), S(d(402, 600, 120))]),
        Schedule("tail_four_in_a_row", "chains", [S(d(403, 700, 150)), S(d(404, 650, 120)), S(d(405, 600, 200)), S(d(406, 500, 150))]),
        Schedule("tail_set_regrown_at_k2", "chains", [S(d(407, 300, 150)), S(d(408, 300, 150)), S(d(409, 2000, 150)), S(d(410, 2100, 120))]),
        Schedule("tail_folder_with_adapters", "chains", [S(d(411, 700, 150)), S(d(412, 64, 150)), S(d(413, 300, 100))], args=["--adapter"]),
        Schedule("tail_folder_16_lanes", "chains", [S(d(420, 700, 150)), S(d(421, 300, 200)), S(d(422, 300, 250)), S(d(419, 300, 105))]),
        Schedule("aux_folder_16_lanes_304", "chains", [S(d(414, 700, 150)), S(d(415, 300, 300)), S(d(416, 300, 304)), S(d(417, 64, 150))]),
        Schedule("aux_folder_8_lanes_104", "chains", [S(d(418, 700, 150)), S(d(437, 300, 100)), S(d(438, 300, 77)), S(d(439, 64, 104))]),
        Schedule("aux_folder_4_lanes", "chains", [S(d(450, 700, 150)), S(d(451, 300, 40)), S(d(452, 300, 70)), S(d(453, 300, 52)), S(d(454, 64, 150))]),
        Schedule("aux_folder_tfa_length", "chains", [S(d(423, 700, 150)), S(d(424, 300, 320))], R=320),
        Schedule("aux_folder_trim_long", "chains", [S(d(425, 700, 150)), S(d(426, 40, 1100)), S(d(427, 500, 150)), S(d(428, 64, 150))], R=2048),
        Schedule("aux_one_and_two_words", "chains", [S(d(430, 500, 150)), S(d(431, 300, 300)), S(d(432, 280, 260)), S(d(433, 400, 150)), S(d(434, 300, 200)), NO_TAIL,
                                                    S(d(435, 300, 150)), S(d(436, 300, 100))]),
        Schedule("aux_set_reuse_at_k2", "chains", [NO_TAIL, S(d(440, 3000, 150)), S(d(441, 3000, 150)), S(d(442, 2500, 150)), S(d(443, 2800, 100)), S(d(444, 64, 150))]),
        Schedule("aux_set_reuse_behind_a_long_fold", "chains", [NO_TAIL, S(d(460, 65537, 30)), S(d(461, 64, 150)), S(d(462, 65537, 30)), S(d(463, 64, 150)), S(d(464, 65537, 30))]),
        Schedule("aux_set_reuse_at_k2_16_lanes", "chains", [S(d(445, 3000, 250)), S(d(446, 3000, 200)), S(d(447, 2500, 250)), S(d(448, 64, 160))]),
    ]


def counter_schedules():
    d = lambda seed, n, L, **kw: make(seed, n, L, via="device", **kw)
    return [
        Schedule("now_by_sync", "counters", [S(d(500, 700, 150)), S(d(501, 64, 150)), SYNC, S(d(502, 300, 100)), SYNC]),
        Schedule("now_by_export_and_import", "counters", [S(d(503, 700, 150)), S(d(504, 300, 100)), EXPORT, S(d(505, 300, 150)), S(d(506, 200, 150)), IMPORT, S(d(507, 300, 100)), FINISH,
                                                         S(d(508, 100, 150)), EXPORT]),
        Schedule("reset_drops_pending", "counters", [S(d(510, 700, 150)), S(d(511, 300, 150)), RESET, S(d(512, 300, 100)), S(d(513, 64, 150)), FINISH, S(d(514, 64, 150)), RESET]),
        Schedule("reset_behind_aux_fold", "counters", [NO_TAIL, S(d(515, 3000, 150)), S(d(516, 3000, 150)), RESET, S(d(517, 300, 150)), S(d(518, 300, 150))]),
        Schedule("reset_behind_tail_fold", "counters", [S(d(519, 3000, 150)), S(d(520, 3000, 150)), RESET, S(d(521, 300, 150))]),
    ]


def host_schedules():
    out = []
    h = lambda seed, n, L, **kw: make(seed, n, L, via="host", **kw)
    for k in (1, 2, 3, 8, 9, 16, 17):
        out.append(Schedule("host_%d_in_flight" % k, "host", [S(h(600 + 20 * k + i, 150 + 37 * ((i * 5) % 7), (150, 100, 140)[i % 3], o0=(0, 16, 5)[i % 3])) for i in range(k)]))
    out.append(Schedule("host_wait_alone", "host", [S(h(700, 400, 150)), S(h(701, 3000, 150)), S(h(702, 3000, 100)), W(0), S(h(703, 500, 150)), W(1), W(3), W(2)]))
    b = [h(710 + i, 300 + 50 * i, 150, o0=(0, 1, 15, 16, 17, 3000)[i % 6]) for i in range(12)]
    out.append(Schedule("host_recycled_buffers", "host", [S(b[0]), S(b[1]), W(0), ("hostile", 0), S(b[2]), W(1), ("hostile", 1), S(b[3]), S(b[4]), W(2), ("hostile", 2), W(3), ("hostile", 3),
                                                         S(b[5]), S(b[6]), W(4), ("hostile", 4), S(b[7]), W(5), W(6), ("hostile", 5), ("hostile", 6), S(b[8])]))
    t = [h(730 + i, 100, 120) for i in range(12)]
    out.append(Schedule("host_tickets", "host", [S(x) for x in t[:8]] + [W(0), S(t[8]), S(t[9]), W(0), W(1), W(2), W(40), S(t[10]), W(3), W(10), W(9), S(t[11])]))
    big = h(740, 200000, 150)  # (one batch sixteen times: 60 MB over the bus per submission, so that the device falls behind the host)
    out.append(Schedule("host_ring_under_load", "host", [S(big) for _ in range(16)] + [W(7), W(3), W(15)]))
    out.append(Schedule("host_slot_sizes", "host", [S(h(750, 500, 150)), S(h(751, 400, 120)), S(h(750, 500, 150)), S(h(751, 400, 120)), S(h(752, 200, 150)), S(h(753, 100, 120)),
                                                   S(h(754, 2500, 150)), S(h(755, 2600, 100)), S(h(756, 64, 150))]))
    out.append(Schedule("host_offsets", "host", [S(h(760 + i, 300, (150, 100)[i % 2], o0=o0)) for i, o0 in enumerate((0, 1, 15, 16, 17, 3000))]))
    out.append(Schedule("host_terminal_n", "host", [S(h(770, 600, 150, tn=True)), S(h(771, 700, 150)), S(h(772, 800, 150, tn=True)), S(h(773, 2000, 100, tn=True)), S(h(774, 100, 100))]))
    out.append(Schedule("host_without_reads", "host", [S(h(780, 600, 150)), S(empty(via="host")), S(h(781, 500, 150)), S(empty(via="host", o0=7)), S(empty(via="host")), S(h(782, 64, 150))]))
    out.append(Schedule("host_without_results", "host", [S(h(785, 600, 150)), S(h(786, 500, 150, results=False)), S(h(787, 300, 100)), S(h(788, 300, 100, results=False))]))
    out.append(Schedule("host_and_device", "host", [S(h(790, 600, 150)), S(make(791, 500, 150, via="device")), S(h(792, 300, 100, tn=True)), S(make(793, 64, 150, via="device")),
                                                   S(h(794, 900, 250)), S(make(795, 300, 300, via="device")), S(h(796, 300, 150))]))
    return out


def setting_schedules():
    from faqcs_amd.options import BUILTIN_ADAPTERS, POLYA

    d = lambda seed, n, L, **kw: make(seed, n, L, via="device", **kw)
    h = lambda seed, n, L, **kw: make(seed, n, L, via="host", **kw)
    plant = [a[1] for a in BUILTIN_ADAPTERS] + [POLYA[1]]
    sizes = (100, 900, 300, 1500, 50, 700)
    out = [
        Schedule("set_quality_between", "settings", [S(d(800, 700, 150)), ("set_quality", 20), S(d(801, 600, 150)), ("set_quality", 2), S(h(802, 500, 100)), ("set_quality", 30), S(d(803, 64, 150))]),
        Schedule("set_offset_behind_two", "settings", [S(d(810, 700, 150)), S(h(811, 600, 150)), ("set_offset", 64), S(d(812, 500, 150, in_off=64)), S(h(813, 300, 100, in_off=64))],
                 args=["--avg_q", "20"]),
        Schedule("adapters_grow_and_shrink", "settings", [S((h if i & 1 else d)(820 + i, n, (150, 100, 250)[i % 3], plant=plant)) for i, n in enumerate(sizes)], args=["--adapter", "--polyA"]),
    ]
    lib = [t[1] for t in library(65)]
    out.append(Schedule("library_grow_and_shrink", "settings", [S((h if i & 1 else d)(830 + i, n, (150, 100, 250)[i % 3], plant=lib[40:])) for i, n in enumerate(sizes)],
                        args=["--adapter"], library=65))
    return out


def error_schedules():
    return [Schedule("quality_error_in_flight", "error", [S(make(900, 300, 150, via="host")), S(make(901, 200, 100, via="device")), S(error_batch(902, 300, 211, via="host")),
                                                         S(make(903, 200, 150, via="device")), S(make(904, 100, 150, via="host")), ("expect_error", E_QUALITY)])]


FAMILIES = ("tail_n", "tail_big", "records", "single_pass", "chains", "counters", "host", "settings", "error")


def all_schedules():
    return tail_schedules() + record_schedules() + chain_schedules() + counter_schedules() + host_schedules() + setting_schedules() + error_schedules()


def schedules_of(family, setting, schedules=None):
    return [s for s in (all_schedules() if schedules is None else schedules) if s.family == family and s.setting == setting]


def hits(s, T=None):
    T = trace(s) if T is None else T
    return {e for e, p in EDGES.items() if p(s, T)}


def coverage(schedules=None, **mutation):
    """-> {edge: [names of the schedules that reach it]} and {schedule name: edges reached}; **mutation: trace()'s ring / n_slots / pending_on"""
    schedules = all_schedules() if schedules is None else schedules
    table, per = {e: [] for e in EDGES}, {}
    for s in schedules:
        per[s.name] = hits(s, trace(s, **mutation))
        for e in per[s.name]:
            table[e].append(s.name)
    return table, per


if __name__ == "__main__":
    _tests_on_path()
    scheds = all_schedules()
    table, _ = coverage(scheds)
    for edge, names in table.items():
        print("%-110s %3d  %s" % (edge, len(names), ", ".join(names[:3]) + (" ..." if len(names) > 3 else "")))
    total = dict.fromkeys(TALLIES, 0)
    for s in scheds:
        for k, v in trace(s).tallies.items():
            total[k] += v
    print("%d schedules, %d reads; %d edges, %d unreached; tallies over all schedules: %s" % (
        len(scheds), sum(s.n_reads() for s in scheds), len(table), sum(not v for v in table.values()), total))
