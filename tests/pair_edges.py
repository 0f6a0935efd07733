"""A constructed catalogue of inputs for the pair stage (faqcs_pair_device, faqcs_render_pair_device; faqcs_pair_kernel.hip), in the style
of tests/pack_edges.py: the edges of the check tile (256 pairs, four waves), of the finishing block and the void tail, of id_length /
equal_bits, of the scan over the 2 n candidates, of the choice of source by mate, of the route byte and of the overflow rule.  Nothing is
drawn at random: every case is a named builder of two mates, every edge a PREDICATE over a case's inputs and its expected outputs -- the ids,
the route, the counters and the rendered offsets, computed here with numpy from the rules of include/faqcs_mi.h (PairCtx), never by calling
the library.  coverage() evaluates every predicate on every case.  tests/test_pair_edges_model.py holds the catalogue against the models and
the host statements without a GPU; tests/test_gpu_pair_edges.py sends it to the device.  Plain Python and numpy: no GPU and no ctypes at
import.

    python -m tests.pair_edges        prints the number of cases per edge
"""
import numpy as np

try:
    import pack_edges as pe
except ImportError:  # python -m tests.pair_edges
    from tests import pack_edges as pe

# ---- the structure constants, restated (test_pair_edges_model.py compares them with the sources) --------------------------------------
PAIR_TILE = 256           # pairs of a tile of pair_check (PAIR_THREADS)
WAVE = 64
VEC = 16                  # bytes of a vector of id_length / equal_bits
SCAN_THREADS = 1024       # tiles per round of pair_finish's strided loops (and of the one-block scan of the rendering)
CAND_TILE = 1024          # candidates of a tile of the paired rendering's scan: 512 pairs
PAIRS_PER_THREAD = 2      # a thread of that scan holds four candidates
VOID_BLOCKS_PER_CU = 8    # blocks of 256 per compute unit beyond which pair_void_tail strides
DEFAULT_CU = 256

CONSTANT_SOURCES = {
    "PAIR_TILE": ("faqcs_pair_kernel.hip", r"constexpr uint32_t PAIR_THREADS = (\d+)"),
    "CAND_TILE": ("faqcs_pack_common.h", r"TILE_THREADS = (\d+), TILE_RPT = (\d+), TILE_ITEMS = TILE_THREADS \* TILE_RPT"),
    "SCAN_THREADS": ("faqcs_pack_common.h", r"SCAN_THREADS = (\d+)"),
    "VOID_BLOCKS_PER_CU": ("faqcs_pair_kernel.hip", r"const size_t cap = \(size_t\)\(n_cu > 0 \? n_cu : \d+\) \* (\d+), want = \(\(size_t\)n_pairs \+ 255\) / 256"),
    "DEFAULT_CU": ("faqcs_pair_kernel.hip", r"const size_t cap = \(size_t\)\(n_cu > 0 \? n_cu : (\d+)\) \* \d+, want"),
}

F_VALID, ROUTE_NOWHERE = 1, 0x80
QC1, QC2, UNPAIRED, DISCARD = 0, 1, 2, 3   # FAQCS_FILE_*
FILES = (QC1, QC2, UNPAIRED, DISCARD)
ARG_SETS = {"default": [], "replace_out64": ["--replace_to_N_q", "15", "--out_ascii", "64"], "ascii64": ["--ascii", "64"]}
HOSTILE_PAD = b"/1 a9.2x"  # what test_gpu_pair.py lays around a text of deflines alone: it would change verdicts if it were read as part of one


def _hash(i):
    i = np.asarray(i, np.int64)
    return (i * 2654435761 + (i >> 5) * 40503) >> 7


def parse_id(d):
    from faqcs_amd import driver

    return driver.parse_id(d)


# =====================================================================================================================================
# a mate and a case
# =====================================================================================================================================

class Mate:
    """One mate: the text its deflines live in with their spans, arenas (64 readable bytes either side), results.  Has the attributes the
    helpers of pair_cases.py and the device helpers of the GPU tests take of a render_cases.Case (as pack_edges.Batch has).
    lens None: no arenas (the pair call reads only results, text and spans); valid None: no results (check only)."""

    def __init__(self, text, def_pos, def_len, lens=None, start=None, wlen=None, valid=None, n_lead=None, n_trail=None, salt=0, qual_shift=0):
        self.text = np.ascontiguousarray(np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else text, np.uint8)
        self.def_pos, self.def_len = np.asarray(def_pos, np.int64).astype(np.uint32), np.asarray(def_len, np.int64).astype(np.uint32)
        self.n = n = len(self.def_pos)
        self.lens = lens = np.zeros(n, np.int64) if lens is None else np.asarray(lens, np.int64)
        self.offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        self.total = total = int(self.offset[-1])
        s, q = np.zeros(64 + total + 64, np.uint8), np.zeros(64 + total + 64, np.uint8)
        s[64:64 + total], q[64:64 + total] = pe.bases(total, salt), pe.quals(total, salt) + qual_shift
        off = self.offset.astype(np.int64)
        for arr, front in ((n_lead, True), (n_trail, False)):
            if arr is not None:
                for i in np.nonzero(np.asarray(arr))[0]:
                    r = int(arr[i])
                    a, b = (off[i], off[i] + r) if front else (off[i + 1] - r, off[i + 1])
                    s[64 + a:64 + b] = ord("N")
        self._s, self._q = s, q
        self.seq, self.qual = s[64:], q[64:]
        self.seg = np.array([0, n], np.uint32)
        if valid is None:
            self.res = None
        else:
            res = np.zeros(n, pe.RESULT_DTYPE)
            res["start"] = 0 if start is None else start
            res["len"] = (lens - res["start"]) if wlen is None else wlen
            res["flags"] = np.asarray(valid, np.int64) * F_VALID | ((np.arange(n) % 8) << 4)  # (the other flag bits are noise)
            self.res = res
        self.set_tn()

    def set_tn(self):
        n, off, s = self.n, self.offset.astype(np.int64), self._s
        if n and self.total:
            nz = self.lens > 0
            first = s[64 + np.minimum(off[:-1], self.total - 1)] == 78
            last = s[64 + np.maximum(off[1:] - 1, 0)] == 78
            self.tn = (first & nz).astype(np.uint8) | ((last & nz).astype(np.uint8) << 1)
        else:
            self.tn = np.zeros(n, np.uint8)

    def with_text(self, text):
        """The same mate (arrays shared) over another text of the same spans."""
        import copy

        m = copy.copy(self)
        m.text = np.ascontiguousarray(text, np.uint8)
        return m


def spans(deflines, sep=b""):
    """-> (text, def_pos, def_len) of deflines laid one behind the other (sep between two of them: none, so the bytes behind a defline are
    the next one, the first starts at text position 0 and the last ends at the text's last byte)"""
    lens = np.array([len(d) for d in deflines], np.int64)
    pos = np.cumsum(lens + len(sep)) - lens - len(sep)
    return sep.join(deflines), pos, lens


def id_mate(deflines):
    return Mate(*spans(deflines))


class PairCase:
    """name, family, the edges it claims, two mates, and how it runs: a route of its own (else the one the pair call makes), n_pairs of the
    rendering, the files, the engine arguments by name, whether the pair call / the rendering run at all, whether the rendering also runs
    at the capacities of the overflow rule, and with which terminal_n pointers."""
    kind = "pair"

    def __init__(self, name, family, claims, m0, m1, route=None, n_pairs=None, files=FILES, args="default", pair=True, render=True, overflow=False,
                 capacity=None, tn_forms=("both", "neither"), deflines=None):
        self.name, self.family, self.claims, self.m = name, family, tuple(claims), [m0, m1]
        self.n = min(m0.n, m1.n)
        self.routed = m0.res is not None
        self.route = None if route is None else np.asarray(route, np.uint8)
        self.n_pairs = self.n if n_pairs is None else n_pairs
        self.files, self.args, self.pair, self.overflow, self.tn_forms, self.deflines = tuple(files), args, pair, overflow, tuple(tn_forms), deflines
        self.render = render and self.routed
        self.fixed_capacity = capacity
        self._ctx = None

    @property
    def capacity(self):
        """bytes no rendering of the case exceeds (the texts hold the deflines alone)"""
        if self.fixed_capacity is not None:
            return self.fixed_capacity
        return sum(len(m.text) + 2 * m.total + 5 * m.n for m in self.m)

    def model_mates(self, with_res=True, lo=0):
        """the mates as driver.pair_model / render_pair_model take them (from pair lo on)"""
        return [dict(text=m.text, def_pos=m.def_pos[lo:], def_len=m.def_len[lo:], seq=m.seq, qual=m.qual, offset=m.offset[lo:], res=m.res[lo:] if with_res and m.res is not None else None) for m in self.m]

    def ctx(self):
        if self._ctx is None:
            self._ctx = PairCtx(self)
        return self._ctx


def id_lengths(m, n):
    """parse_id over every defline of a mate at once, from the rule of include/faqcs_mi.h: the first ' ' (or the length), less 2 when the
    two bytes in front of it are a mark and a digit"""
    t = np.concatenate([m.text, np.zeros(2, np.uint8)]).astype(np.int64)
    pos, ln = m.def_pos[:n].astype(np.int64), m.def_len[:n].astype(np.int64)
    sp = np.nonzero(m.text == 32)[0]
    if len(sp):
        k = np.searchsorted(sp, pos)
        nxt = np.where(k < len(sp), sp[np.minimum(k, len(sp) - 1)], 1 << 62)
    else:
        nxt = np.full(n, 1 << 62, np.int64)
    loc = np.where(nxt < pos + ln, nxt - pos, ln)
    digit, mark = t[np.maximum(pos + loc - 1, 0)], t[np.maximum(pos + loc - 2, 0)]
    strip = (loc > 1) & (digit >= 48) & (digit <= 57) & ((mark == 46) | (mark == 47))
    return loc - 2 * strip


def ids_equal(m0, m1, la, lb):
    n = len(la)
    same = la == lb
    L = np.where(same, la, 0)
    ends = np.cumsum(L)
    ramp = np.arange(int(ends[-1]) if n else 0, dtype=np.int64) - np.repeat(ends - L, L)
    neq = m0.text[np.repeat(m0.def_pos[:n].astype(np.int64), L) + ramp] != m1.text[np.repeat(m1.def_pos[:n].astype(np.int64), L) + ramp]
    cs = np.concatenate([[0], np.cumsum(neq)])
    return same & (cs[ends] - cs[ends - L] == 0)


class PairCtx:
    """What the predicates look at: the inputs of a case and what the rules of include/faqcs_mi.h make of them."""

    def __init__(self, case):
        self.case, self.m, self.n, self._defs = case, case.m, case.n, None
        n = self.n
        self.n_tiles = (n + PAIR_TILE - 1) // PAIR_TILE
        if case.pair:
            self.id_len = [id_lengths(m, n) for m in case.m]
            self.same = ids_equal(case.m[0], case.m[1], *self.id_len)
            self.bad = np.nonzero(~self.same)[0]
        else:
            self.id_len, self.same, self.bad = None, np.ones(n, bool), np.zeros(0, np.int64)
        self.mismatch = int(len(self.bad) > 0)
        self.n_pairs = int(self.bad[0]) if self.mismatch else n
        self.info = dict(paired_read_number=0, paired_base_length=0, n_pairs=self.n_pairs, mismatch=self.mismatch,
                         id_len=(int(self.id_len[0][self.n_pairs]), int(self.id_len[1][self.n_pairs])) if self.mismatch else (0, 0), n_one_valid=0, n_none_valid=0)
        self.pair_route = None
        if case.routed:
            v = [(m.res["flags"][:n] & F_VALID) != 0 for m in case.m]
            self.valid = v
            r = (v[0].astype(np.uint8) | (v[1].astype(np.uint8) << 1))
            self.both = r == 3
            live = np.arange(n) < self.n_pairs
            self.base_sum = case.m[0].res["len"][:n].astype(np.int64) + case.m[1].res["len"][:n].astype(np.int64)
            self.info.update(paired_read_number=2 * int((self.both & live).sum()), paired_base_length=int(self.base_sum[self.both & live].sum()),
                             n_one_valid=int((((r == 1) | (r == 2)) & live).sum()), n_none_valid=int(((r == 0) & live).sum()))
            self.pair_route = np.where(live, r, ROUTE_NOWHERE).astype(np.uint8)
        self.route = case.route if case.route is not None else self.pair_route
        self.files = {}
        if case.render:
            for f in case.files:
                self.files[f] = FileCtx(self, f)


class FileCtx:
    """One of the four files of a case: which of the 2 n_pairs candidates the statement renders, and the offsets of the output."""

    def __init__(self, c, f):
        case, npairs = c.case, c.case.n_pairs
        self.f = f
        r = np.repeat(c.route[:npairs].astype(np.int64), 2)
        s = np.tile(np.array([0, 1], np.int64), npairs)
        self.sel = {QC1: (s == 0) & (r == 3), QC2: (s == 1) & (r == 3), UNPAIRED: r == (1 << s), DISCARD: (r < 4) & ((r >> s) & 1 == 0)}[f]
        il = lambda a, b: np.stack([np.asarray(a[:npairs], np.int64), np.asarray(b[:npairs], np.int64)], axis=1).ravel()
        m0, m1 = case.m
        self.wlen = il(m0.lens, m1.lens) if f == DISCARD else il(m0.res["len"], m1.res["len"])
        self.size = il(m0.def_len, m1.def_len) + 2 * self.wlen + 5
        self.rec_index = np.nonzero(self.sel)[0]
        self.offset = np.concatenate([[0], np.cumsum(self.size[self.sel])])
        self.n_reads, self.n_bytes = len(self.rec_index), int(self.offset[-1])
        nt = (2 * npairs + CAND_TILE - 1) // CAND_TILE
        pad = np.zeros(nt * CAND_TILE, bool)
        pad[:2 * npairs] = self.sel
        self.tiles = pad.reshape(nt, CAND_TILE)
        self.tile_recs = self.tiles.sum(1)
        self.alternate = self.n_reads >= 1 and bool((np.diff(self.rec_index & 1) != 0).all())


# =====================================================================================================================================
# the edges
# =====================================================================================================================================

SPACE_AT = (0, 1, 2, 15, 16, 17, 31, 32, 33)
NO_SPACE_LEN = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49)
SUFFIX_LOC = (1, 2, 3, 16, 17, 18)
ODD_BYTES = (0x00, 0x09, 0x80, 0xA0, 0xFF)
CHECK_SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
BAD_THREADS = (0, 63, 64, 255)
RENDER_SIZES = (1, 2, 511, 512, 513, 1023, 1024, 1025)


def _loc(d):
    k = d.find(b" ")
    return len(d) if k < 0 else k


def _stripped(d):
    return len(parse_id(d)) == _loc(d) - 2


def _every_defline(c):
    """(mate, pair, defline, the bytes that lie behind it where the kernel reads them) of a case that names its deflines"""
    if c.case.deflines is None:
        return ()
    if c._defs is None:
        c._defs = []
        for s, ds in enumerate(c.case.deflines):
            behind = b"".join(ds) + HOSTILE_PAD * 8
            at = 0
            for i, d in enumerate(ds):
                at += len(d)
                c._defs.append((s, i, d, behind[at:at + 16]))
    return c._defs


def _any_defline(pred):
    return lambda c: any(pred(d, behind) for _, _, d, behind in _every_defline(c))


def _id_edges():
    E = {}
    for P in SPACE_AT:
        E["first_space_at=%d" % P] = _any_defline(lambda d, b, P=P: d.find(b" ") == P and len(d) > P + 1)
    for L in NO_SPACE_LEN:
        E["no_space_len=%d" % L] = _any_defline(lambda d, b, L=L: b" " not in d and len(d) == L)
    for r in range(1, 16):
        E["last_vector_holds=%d_space_in_the_bytes_behind" % r] = _any_defline(lambda d, b, r=r: b" " not in d and len(d) % VEC == r and b" " in b[:VEC - r])
    E["last_entry_space_in_the_padding"] = lambda c: any(b" " not in d and i == len(c.case.deflines[s]) - 1 and len(d) % VEC and b" " in b[:VEC - len(d) % VEC] for s, i, d, b in _every_defline(c))
    for K in SUFFIX_LOC:
        if K == 1:
            E["suffix_loc=1_not_stripped"] = _any_defline(lambda d, b: _loc(d) == 1 and d[:1].isdigit() and parse_id(d) == d[:1])
        else:
            E["suffix_loc=%d" % K] = _any_defline(lambda d, b, K=K: _loc(d) == K and _stripped(d) and d[K - 1:K].isdigit() and d[K - 2:K - 1] in (b".", b"/"))
    for ch in b"09":
        E["digit_%c_stripped" % ch] = _any_defline(lambda d, b, ch=ch: _stripped(d) and d[_loc(d) - 1] == ch)
    for ch, nm in ((0x2f, "slash"), (0x3a, "colon")):
        E["digit_place_%s_not_stripped" % nm] = _any_defline(lambda d, b, ch=ch: _loc(d) > 1 and d[_loc(d) - 1] == ch and d[_loc(d) - 2:_loc(d) - 1] in (b".", b"/") and not _stripped(d))
    for ch, nm in ((0x2e, "dot"), (0x2f, "slash")):
        E["mark_%s_stripped" % nm] = _any_defline(lambda d, b, ch=ch: _stripped(d) and d[_loc(d) - 2] == ch)
    for ch, nm in ((0x2d, "minus"), (0x30, "zero")):
        E["mark_place_%s_not_stripped" % nm] = _any_defline(lambda d, b, ch=ch: _loc(d) > 1 and d[_loc(d) - 2] == ch and d[_loc(d) - 1:_loc(d)].isdigit() and not _stripped(d))
    E["suffix_behind_first_space_ignored"] = _any_defline(lambda d, b: b" " in d and d[-2:-1] in (b".", b"/") and d[-1:].isdigit() and not _stripped(d) and _loc(d) > 1)
    E["double_suffix_stripped_once"] = _any_defline(lambda d, b: _stripped(d) and len(parse_id(parse_id(d))) == len(parse_id(d)) - 2)
    for v in ODD_BYTES:
        # inside the id with id bytes behind it: neither a delimiter nor an end
        E["byte_0x%02x_inside_id" % v] = _any_defline(lambda d, b, v=v: bytes([v]) in parse_id(d)[:-1] and len(parse_id(d)) > d.find(bytes([v])) + 1)
    for v in ODD_BYTES:
        E["byte_0x%02x_in_front_of_the_only_difference" % v] = lambda c, v=v: c.case.deflines is not None and c.mismatch == 1 and (
            lambda a, b: len(a) == len(b) and a[-1] != b[-1] and a[:-1] == b[:-1] and a[-4] == v)(parse_id(c.case.deflines[0][c.n_pairs]), parse_id(c.case.deflines[1][c.n_pairs]))
    for s in (0, 1):
        for v in range(16):
            E["def_pos_mod_16=%d/mate%d" % (v, s)] = lambda c, s=s, v=v: c.id_len is not None and bool(((c.id_len[s] >= 17) & (c.m[s].def_pos[:c.n] % VEC == v)).any())
    return E


def _one_byte(c, k, bit):
    """the first mismatch of the case: two ids of 48 bytes that differ in byte k alone, by `bit` alone"""
    if not c.mismatch or c.info["id_len"] != (48, 48):
        return False
    i = c.n_pairs
    a, b = (m.text[int(m.def_pos[i]):int(m.def_pos[i]) + 48] for m in c.m)
    x = a ^ b
    return int(x[k]) == bit and int(np.count_nonzero(x)) == 1


def _equal_then_differ(form):
    """a MATCHING pair with ids of la bytes whose byte la differs between the mates"""
    def pred(c, r):
        if c.case.deflines is None:
            return False
        for i, (a, b) in enumerate(zip(*c.case.deflines)):
            la = len(parse_id(a))
            if not c.same[i] or la % VEC != r:
                continue
            if form == "comment" and len(a) > la + 1 and len(b) > la + 1 and a[la] == b[la] == 32 and a[la + 1] != b[la + 1]:
                return True
            if form == "suffix" and _stripped(a) != _stripped(b):
                return True
        return False
    return pred


def _compare_edges():
    E = {}
    for bit, nm in ((1, "bit0"), (0x80, "bit7")):
        for k in range(48):
            for way in ("ab", "ba"):
                E["one_byte_%s_at=%d/%s" % (nm, k, way)] = lambda c, k=k, bit=bit, way=way: _one_byte(c, k, bit) and c.case.name.endswith(way)
    for r in range(1, 16):
        E["match_then_space_and_comments_differ_la_mod_16=%d" % r] = lambda c, r=r: _equal_then_differ("comment")(c, r)
        E["match_suffix_on_one_side_la_mod_16=%d" % r] = lambda c, r=r: _equal_then_differ("suffix")(c, r)
    E["equal_length_suffix_against_two_id_bytes_mismatches"] = lambda c: c.case.deflines is not None and c.mismatch == 1 and (
        lambda a, b: len(a) == len(b) and a[:-2] == b[:-2] and _stripped(a) and not _stripped(b) and b" " not in a + b)(c.case.deflines[0][c.n_pairs], c.case.deflines[1][c.n_pairs])
    return E


def _tiled(c):
    return c.case.family in ("tiles", "big") and c.case.routed


def _behind_bad_counts(c):
    """both-valid pairs right behind the first bad pair: in its wave, in a later wave of its tile, in the tile behind"""
    if not (_tiled(c) and c.mismatch):
        return False
    f, both = c.n_pairs, c.both
    w_end, t_end = (f // WAVE + 1) * WAVE, (f // PAIR_TILE + 1) * PAIR_TILE
    return bool(both[f + 1:w_end].any() and both[w_end:t_end].any() and both[t_end:t_end + PAIR_TILE].any())


def _tile_edges():
    E = {}
    for n in CHECK_SIZES:
        E["n=%d_clean" % n] = lambda c, n=n: _tiled(c) and c.n == n and not c.mismatch
        E["n=%d_last_pair_bad" % n] = lambda c, n=n: _tiled(c) and c.n == n and c.mismatch and c.n_pairs == n - 1
    for t in (0, 1):
        for th in BAD_THREADS:
            E["first_bad_tile%d_thread%d" % (t, th)] = lambda c, t=t, th=th: _tiled(c) and c.mismatch and c.n_pairs == t * PAIR_TILE + th and c.n > c.n_pairs + PAIR_TILE
    E["two_bad_in_a_tile_later_wave_lower_lane"] = lambda c: _tiled(c) and len(c.bad) >= 2 and c.bad[1] // PAIR_TILE == c.bad[0] // PAIR_TILE and c.bad[1] // WAVE > c.bad[0] // WAVE and c.bad[1] % WAVE < c.bad[0] % WAVE
    E["bad_in_every_wave_of_a_tile"] = lambda c: _tiled(c) and c.mismatch and len(np.unique(c.bad[c.bad // PAIR_TILE == c.bad[0] // PAIR_TILE] // WAVE)) == PAIR_TILE // WAVE
    E["two_bad_tiles_later_at_lower_position"] = lambda c: _tiled(c) and len(c.bad) >= 2 and c.bad[1] // PAIR_TILE > c.bad[0] // PAIR_TILE and c.bad[1] % PAIR_TILE < c.bad[0] % PAIR_TILE
    E["both_valid_pairs_right_behind_the_bad_pair"] = _behind_bad_counts
    E["tile_sum_above_2^24"] = lambda c: c.case.routed and c.n >= PAIR_TILE and any(int(c.base_sum[t:t + PAIR_TILE][c.both[t:t + PAIR_TILE]].sum()) > 1 << 24 for t in range(0, min(c.n_pairs, 4 * PAIR_TILE), PAIR_TILE))
    E["paired_base_length_above_2^32"] = lambda c: c.info["paired_base_length"] > 1 << 32 and c.info["n_one_valid"] > 0 and c.info["n_none_valid"] > 0
    for nt in (1023, 1024, 1025):
        E["n_tiles=%d_clean" % nt] = lambda c, nt=nt: c.case.routed and c.n_tiles == nt and not c.mismatch
    return E


def _ragged_counters(c, lo, hi):
    """the tiles lo .. hi - 1 differ among themselves in what they count"""
    live = (np.arange(c.n) < c.n_pairs) & c.both
    per = np.add.reduceat(np.where(live, c.base_sum, 0), np.arange(0, c.n, PAIR_TILE))[lo:hi]
    return len(np.unique(per)) > 8


def big_edges(n_cu=DEFAULT_CU):
    """the edges beyond one round of the finishing block and beyond the void tail's grid, for a device of n_cu compute units"""
    E = {}
    rnd = SCAN_THREADS * PAIR_TILE
    E["first_bad_beyond_scan_round"] = lambda c: c.case.routed and len(c.bad) >= 2 and c.n_pairs >= rnd
    E["later_bad_in_lower_scan_slot"] = lambda c: c.case.routed and len(c.bad) >= 2 and c.bad[0] >= rnd and bool(((c.bad[1:] // PAIR_TILE > c.bad[0] // PAIR_TILE) & (c.bad[1:] // PAIR_TILE % SCAN_THREADS < c.bad[0] // PAIR_TILE % SCAN_THREADS)).any())
    E["void_tail_second_stride"] = lambda c: c.case.routed and c.mismatch and c.n - c.n_pairs > n_cu * VOID_BLOCKS_PER_CU * 256
    E["sums_from_second_round"] = lambda c: c.case.routed and c.n_pairs > rnd + PAIR_TILE and _ragged_counters(c, SCAN_THREADS, c.n_pairs // PAIR_TILE + 1) and _ragged_counters(c, 0, SCAN_THREADS)
    E["take_is_one_tile_of_many"] = lambda c: c.case.routed and c.mismatch and c.n_pairs < PAIR_TILE and c.n_tiles > SCAN_THREADS
    E["bad_last_pair_beyond_scan_round"] = lambda c: c.case.routed and c.mismatch and c.n_pairs == c.n - 1 and c.n > rnd
    E["scan_carries_into_second_round"] = lambda c: all(f in c.files and 2 * c.case.n_pairs >= SCAN_THREADS * CAND_TILE + 1500 and len(np.unique(c.files[f].tile_recs[:SCAN_THREADS])) > 8
                                                         and len(np.unique(c.files[f].tile_recs[SCAN_THREADS:])) > 1 for f in FILES)
    return E


def _file_pred(pred, files=FILES):
    return lambda c: any(f in c.files and pred(c.files[f]) for f in files)


def _last_then_first(fc):
    return any(fc.tile_recs[t] == 1 and fc.tiles[t, -1] and fc.tile_recs[t + 1] == 1 and fc.tiles[t + 1, 0] for t in range(len(fc.tile_recs) - 1))


def _swap_changes_every_record(c):
    """Both mates share offsets and spans, and at EVERY position of the texts' deflines and of the arenas their bytes differ: a record read
    from the other mate's arrays at the same place differs in every byte it takes from them -- and every record takes one."""
    a, b = c.m
    if c.case.family != "source" or a.n != b.n or not ((a.offset == b.offset).all() and (a.def_pos == b.def_pos).all() and (a.def_len == b.def_len).all()):
        return False
    T = a.total
    differ = (a.text != b.text).all() and (a.seq[:T] != b.seq[:T]).all() and (a.qual[:T] != b.qual[:T]).all() and (a.tn != b.tn).any()
    return bool(differ) and all((fc.size[fc.sel] > 5).all() and fc.n_reads > 0 for fc in c.files.values())


def _runs(m):
    """(leading, trailing) 'N' run of every read"""
    lead, trail = np.zeros(m.n, np.int64), np.zeros(m.n, np.int64)
    for i in np.nonzero(m.tn)[0]:
        r = m.seq[int(m.offset[i]):int(m.offset[i + 1])]
        nn = np.nonzero(r != 78)[0]
        lead[i] = int(nn[0]) if len(nn) else len(r)
        trail[i] = (len(r) - 1 - int(nn[-1])) if len(nn) else len(r)
    return lead, trail


def _four_flagged(c):
    if c.case.family != "source" or c.n < 2:
        return False
    l0, l1 = _runs(c.m[0])[0], _runs(c.m[1])[0]
    return any(len({int(l0[i]), int(l0[i + 1]), int(l1[i]), int(l1[i + 1])} - {0}) == 4 for i in range(0, c.case.n_pairs - 1, 2))


def _terminal(form):
    def pred(c):
        if c.case.family != "source":
            return False
        f0, f1 = (int((m.tn != 0).sum()) for m in c.m)
        same_offsets = c.m[0].n == c.m[1].n and bool((c.m[0].offset == c.m[1].offset).all())
        if form == "mate0_only":
            return same_offsets and f0 >= 40 and f1 == 0
        if form == "mate1_only":
            return same_offsets and f1 >= 40 and f0 == 0
        return same_offsets and f0 >= 40 and f1 >= 40 and bool((np.stack(_runs(c.m[0])) != np.stack(_runs(c.m[1]))).any(0).sum() >= 20)
    return pred


def _render_edges():
    E = {}
    E["route_every_byte_value"] = lambda c: c.case.route is not None and c.case.n_pairs == 256 and bool((c.case.route[:256] == np.arange(256)).all()) and all(
        f in c.files for f in FILES) and all((m.lens[:256] > 0).all() for m in c.m)
    for n in RENDER_SIZES:
        E["render_n_pairs=%d" % n] = lambda c, n=n: c.case.render and c.case.n_pairs == n and any(fc.n_reads for fc in c.files.values())
    E["n_pairs_below_both_n_reads_n1_ne_n2"] = lambda c: c.case.render and c.case.n_pairs < min(c.m[0].n, c.m[1].n) and c.m[0].n != c.m[1].n
    E["candidate_tile_all_dropped"] = _file_pred(lambda fc: len(fc.tile_recs) >= 3 and bool(((fc.tile_recs[1:-1] == 0) & (fc.tile_recs[:-2] > 0) & (fc.tile_recs[2:] > 0)).any()))
    E["only_last_of_tile_then_only_first_of_next/UNPAIRED"] = _file_pred(_last_then_first, (UNPAIRED,))
    E["only_last_of_tile_then_only_first_of_next/DISCARD"] = _file_pred(_last_then_first, (DISCARD,))
    E["candidate_tiles_alternate_all_and_none"] = _file_pred(lambda fc: len(fc.tile_recs) >= 4 and all(fc.tile_recs[t] == (CAND_TILE if t % 2 == 0 else 0) for t in range(4)))
    E["odd_n_pairs_leaves_half_a_thread"] = lambda c: c.case.render and c.case.n_pairs % 2 == 1 and any(fc.sel[-2:].any() for fc in c.files.values())
    for f in FILES:
        E["overflow_one_byte_short/file%d" % f] = lambda c, f=f: c.case.overflow and f in c.files and c.files[f].n_bytes > 1000
    E["empty_file_at_capacity_0"] = lambda c: c.case.overflow and any(fc.n_reads == 0 for fc in c.files.values())
    E["thread_sum_passes_2^32"] = _file_pred(lambda fc: len(fc.sel) > 0 and int(np.concatenate([np.where(fc.sel, fc.size, 0), np.zeros(3, np.int64)])[:(len(fc.sel) + 3) // 4 * 4].reshape(-1, 4).sum(1).max()) >= 1 << 32)
    E["mates_share_offsets_and_differ_in_every_byte"] = _swap_changes_every_record
    E["mates_of_very_different_offsets"] = lambda c: c.case.family == "source" and c.m[0].lens.max() <= 3 and c.m[1].lens.min() >= 100 and c.m[1].lens.max() >= 250
    for form in ("mate0_only", "mate1_only", "both_different_runs"):
        E["terminal_N_" + form] = _terminal(form)
    E["four_candidates_of_a_thread_flagged_four_run_lengths"] = _four_flagged
    for form in ("both", "neither", "mate0", "mate1"):
        E["terminal_n_pointer_" + form] = lambda c, form=form: form in c.case.tn_forms and c.case.render and any((m.tn != 0).any() for m in c.m)
    for e, (p, kinds) in pe.GATHER_EDGES.items():
        if "render" in kinds:
            E["gather_across_mates:" + e] = _file_pred(lambda fc, p=p: fc.alternate and p(fc.offset))
    E["three_records_of_mates_0_1_0_in_one_piece"] = _file_pred(lambda fc: fc.alternate and bool(((fc.offset[:-3] // VEC == (fc.offset[3:] - 1) // VEC) & (fc.rec_index[:-2] % 2 == 0)).any()) if fc.n_reads >= 3 else False)
    E["deflines_at_both_ends_of_both_texts"] = lambda c: c.case.render and c.n > 0 and all(m.def_pos[0] == 0 and m.def_len[0] > 0 and int(m.def_pos[-1]) + int(m.def_len[-1]) == len(m.text) and m.def_len[-1] > 0 for m in c.m) and any(
        fc.sel[0] and fc.sel[-1] for fc in c.files.values())
    for a in ARG_SETS:
        E["args=" + a] = lambda c, a=a: c.case.render and c.case.args == a and any(f != DISCARD and fc.n_reads >= 100 for f, fc in c.files.items()) and DISCARD in c.files and c.files[DISCARD].n_reads >= 50
    return E


ID_EDGES, COMPARE_EDGES, TILE_EDGES, RENDER_EDGES = _id_edges(), _compare_edges(), _tile_edges(), _render_edges()


def edges(n_cu=DEFAULT_CU):
    E = {}
    for part in (ID_EDGES, COMPARE_EDGES, TILE_EDGES, big_edges(n_cu), RENDER_EDGES):
        E.update(part)
    return E


def required():
    """every edge has to be reached"""
    return set(edges())


# =====================================================================================================================================
# the cases
# =====================================================================================================================================

def _letters(n, salt):
    return bytes((97 + (_hash(np.arange(n) + 31 * salt) % 26)).astype(np.uint8))


CLEAN_BASE = [(b"ab", b"ab"), (b"x/1", b"x/2"), (b"", b""), (b"@id comment/1", b"@id other"), (_letters(40, 1), _letters(40, 1) + b" c"), (b"/1", b""), (b"q.7", b"q")]


def _check_case(name, claims, pairs):
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    return PairCase(name, "ids", claims, id_mate(a), id_mate(b), deflines=(a, b))


def id_cases():
    C = []
    # -- the first ' ' and the lengths without one
    ds = [_letters(P, P) + b" " + _letters(20, P + 1) for P in SPACE_AT] + [_letters(L, 50 + L) for L in NO_SPACE_LEN]
    C.append(_check_case("space_positions_and_lengths", ["first_space_at=%d" % P for P in SPACE_AT] + ["no_space_len=%d" % L for L in NO_SPACE_LEN],
                         [(d, d.split(b" ")[0] + b" other") if b" " in d else (d, d) for d in ds]))
    # -- a last vector of r bytes with a ' ' right behind the defline: the next one begins with it; the last one finds it in the padding
    # (a scan that ran over the end would take loc = len from a ' ' AT the end all the same; behind "q" it takes one byte more on one side only)
    pairs = []
    for r in range(1, 16):
        x, y = _letters(16 + r, 100 + r), _letters(32 + r, 130 + r)
        pairs += [(x, x), (b" x" + bytes([97 + r]), b" "), (y, y), (b"q x", b"q"), (x[:r], x[:r]), (b"q", b"q y")]
    C.append(_check_case("space_behind_the_last_vector", ["last_vector_holds=%d_space_in_the_bytes_behind" % r for r in range(1, 16)], pairs))
    for r in (1, 7, 13):
        x = _letters(32 + r, 200 + r)
        C.append(_check_case("space_in_the_padding_%d" % r, ["last_entry_space_in_the_padding"], CLEAN_BASE[:r % 5] + [(x, x)]))
    # -- the suffix
    # every form that is NOT stripped stands against the same bytes with a suffix that is: stripped by mistake, the pair would differ
    pairs = [(b"k/", b"k/ c"), (b"7", b"7/1"), (b"k.", b"k./3"), (b"9 c", b"9"), (b"/1", b""), (b".9 c", b" d"), (b"a/1", b"a.2"), (b"a/0 x", b"a")]
    for K in (16, 17, 18):
        x = _letters(K - 2, 300 + K)
        pairs += [(x + b"/1", x + b".2"), (x + b".0 c", x), (x, x + b"/9 zz")]
    pairs += [(b"ab/0", b"ab/9"), (b"ab//", b"ab//.1"), (b"ab/:", b"ab/:/1"), (b"ab./ c", b"ab.//7"), (b"ab.:", b"ab.:.0"), (b"ab.3", b"ab/4"), (b"ab-1", b"ab-1/2"), (b"ab01", b"ab01.5"),
              (b"ab cd/1", b"ab xy.2"), (b"ab/x c/1", b"ab/x"), (b"a/1/2", b"a/1/3"), (b"a/1/2", b"a/1.7 c"), (b"a.1.2.3", b"a.1.2/7"), (b"//", b"///1"), (b"/:", b"/:/1")]
    x = _letters(14, 5)
    pairs += [(x + b"//", x + b"///1"), (x + b"/:", x + b"/:.2"), (x + b"-1", x + b"-1/1"), (x + b"01", x + b"01/1"), (x + b"/@", x + b"/@/1"), (x + b"..", x + b"...9")]
    claims = ["suffix_loc=1_not_stripped"] + ["suffix_loc=%d" % K for K in SUFFIX_LOC[1:]] + ["digit_0_stripped", "digit_9_stripped", "digit_place_slash_not_stripped", "digit_place_colon_not_stripped",
              "mark_dot_stripped", "mark_slash_stripped", "mark_place_minus_not_stripped", "mark_place_zero_not_stripped", "suffix_behind_first_space_ignored", "double_suffix_stripped_once"]
    C.append(_check_case("suffixes", claims, pairs))
    # -- bytes that are neither delimiters nor ends
    pairs = []
    for v in ODD_BYTES:
        for at in (0, 1, 7, 15, 16, 20):
            x = _letters(at, v) + bytes([v]) + _letters(22 - at, v + 1)
            pairs += [(x, x), (x + b"/1", x + b" c"), (bytes([v]) * 19, bytes([v]) * 19 + b".2")]
    C.append(_check_case("odd_bytes", ["byte_0x%02x_inside_id" % v for v in ODD_BYTES], pairs))
    # (a byte taken for a delimiter hides what follows it on BOTH sides: only a difference behind it tells)
    for v in ODD_BYTES:
        for at in (3, 20):
            x = _letters(at, v) + bytes([v])
            C.append(_check_case("odd_byte_0x%02x_at_%d_then_differ" % (v, at), ["byte_0x%02x_in_front_of_the_only_difference" % v], CLEAN_BASE[:2 + at % 3] + [(x + b"abc", x + b"abd c")]))
    # -- every alignment of a long defline, per mate: the fillers in front put entry k at k mod 16 in mate 1's text and at 5 k + 3 in mate 2's
    pairs, at = [], [0, 0]
    filler = lambda L: b" "[:L] + _letters(max(L - 1, 0), L)  # (the empty id at every length)
    for k in range(16):
        x = _letters(17 + k % 5, 400 + k)
        f = [filler((t - p) % VEC) for t, p in zip((k, (5 * k + 3) % VEC), at)]
        pairs += [tuple(f), (x + b"/1", x)]
        at = [at[0] + len(f[0]) + len(x) + 2, at[1] + len(f[1]) + len(x)]
    C.append(_check_case("every_alignment", ["def_pos_mod_16=%d/mate%d" % (v, s) for s in (0, 1) for v in range(16)], pairs))
    return C


def compare_cases():
    C = []
    for bit, nm in ((1, "bit0"), (0x80, "bit7")):
        for k in range(48):
            x = _letters(48, 500 + k)
            y = x[:k] + bytes([x[k] ^ bit]) + x[k + 1:]
            for way, (a, b) in (("ab", (x, y)), ("ba", (y, x))):
                C.append(_check_case("one_byte_%s_at_%d_%s" % (nm, k, way), ["one_byte_%s_at=%d/%s" % (nm, k, way)], CLEAN_BASE[:1 + k % 7] + [(a + b"/1", b + b" c")]))
    pairs = []
    for r in range(1, 16):
        for la in (r, 32 + r):
            x = _letters(la, 600 + la)
            pairs += [(x + b" one", x + b" two"), (x + b"/1", x + b"/2"), (x + b".1", x), (x, x + b"/2 c")]
    C.append(_check_case("equal_ids_then_different_bytes", ["match_then_space_and_comments_differ_la_mod_16=%d" % r for r in range(1, 16)] + ["match_suffix_on_one_side_la_mod_16=%d" % r for r in range(1, 16)], pairs))
    for la in (3, 14, 30):
        x = _letters(la, 700 + la)
        for way, (a, b) in (("ab", (x + b"/1", x + b"yz")), ("ba", (x + b"yz", x + b"/1"))):
            if way == "ab":
                C.append(_check_case("suffix_against_two_id_bytes_%d" % la, ["equal_length_suffix_against_two_id_bytes_mismatches"], CLEAN_BASE[:la % 4] + [(a, b)]))
            else:
                C.append(_check_case("two_id_bytes_against_suffix_%d" % la, [], CLEAN_BASE[:la % 4] + [(a, b)]))
    return C


def tiny_ids(n, bad=()):
    """n pairs of tiny deflines laid back to back: ids of 2 - 4 letters, on either side now and then a suffix (2 - 6 bytes in all); the
    pairs of `bad` differ in bit 0 of their first byte.  -> two (text, def_pos, def_len)"""
    i = np.arange(n, dtype=np.int64)
    h = _hash(i)
    idl = 2 + h % 3
    out = []
    for s in (0, 1):
        suf = ((h >> 4) % 3 == 0) if s == 0 else ((h >> 6) % 4 == 1)
        ln = idl + 2 * suf
        pos = np.cumsum(ln) - ln
        p = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(pos, ln)
        ii = np.repeat(i, ln)
        body = (97 + _hash(ii * 7 + p * 131 + 3) % 26).astype(np.uint8)
        text = np.where(p < np.repeat(idl, ln), body, np.where(p == np.repeat(idl, ln), 47 if s == 0 else 46, 49 + s)).astype(np.uint8)
        if s == 1 and len(bad):
            text[pos[np.asarray(bad, np.int64)]] ^= 1
        out.append((text, pos, ln))
    return out


def tiny_mates(n, bad=(), n1=None, big=False, len65535=False, arenas=True, qual_shift=0):
    """Two mates of tiny deflines (tiny_ids) and tiny reads of different lengths per mate, ragged validity by a fixed hash."""
    out = []
    for s, (text, pos, ln) in enumerate(tiny_ids(max(n, n1 or 0), bad)):
        k = n if s == 0 or n1 is None else n1
        text, pos, ln = text[:int(pos[k - 1] + ln[k - 1]) if k else 0], pos[:k], ln[:k]
        i = np.arange(k, dtype=np.int64)
        h = _hash(i + 77 * s)
        lens = (h >> (2 * s)) % 4 if big else ((i * 7) % 11 if s == 0 else (i * 5) % 13 + 1)
        valid = ((h >> 3) % 4 != 0) if s == 0 else ((h >> 5) % 5 != 0)
        if len65535:
            out.append(Mate(text, pos, ln, None, 0, np.full(k, 65535), valid, salt=s))
        else:
            start = (lens > 2).astype(np.int64)
            out.append(Mate(text, pos, ln, lens if arenas else None, start if arenas else 0, (lens - start) if arenas else lens, valid,
                            n_lead=(i % 1009 == 5) * np.minimum(lens, 2) if arenas else None, salt=1000 * s + 1, qual_shift=qual_shift))
    return out


def tile_cases():
    C = []
    add = lambda name, claims, n, bad=(), **kw: C.append(PairCase(name, "tiles", claims, *tiny_mates(n, bad), **kw))
    for n in CHECK_SIZES:
        add("check_%d_clean" % n, ["n=%d_clean" % n], n)
        add("check_%d_last_bad" % n, ["n=%d_last_pair_bad" % n], n, (n - 1,))
    for t in (0, 1):
        for th in BAD_THREADS:
            add("bad_tile%d_thread%d" % (t, th), ["first_bad_tile%d_thread%d" % (t, th)] + (["both_valid_pairs_right_behind_the_bad_pair"] if th < 63 else []), 800, (t * PAIR_TILE + th,))
    add("two_bad_later_wave_lower_lane", ["two_bad_in_a_tile_later_wave_lower_lane", "both_valid_pairs_right_behind_the_bad_pair"], 600, (70, 133))
    add("two_bad_later_wave_lower_lane_tile1", ["two_bad_in_a_tile_later_wave_lower_lane"], 900, (256 + 62, 256 + 64))
    add("bad_in_every_wave", ["bad_in_every_wave_of_a_tile"], 700, (256 + 40, 256 + 64 + 30, 256 + 128 + 20, 256 + 192 + 10))
    add("two_bad_tiles_later_lower", ["two_bad_tiles_later_at_lower_position"], 900, (200, 256 + 17))
    add("two_bad_tiles_later_lower_far", ["two_bad_tiles_later_at_lower_position"], 900, (255 + 256, 512))
    # -- the counters
    m = tiny_mates(300, len65535=True)
    for x in m:
        x.res["flags"][:PAIR_TILE] |= F_VALID
    C.append(PairCase("tile_of_65535", "tiles", ["tile_sum_above_2^24"], *m, render=False))
    C.append(PairCase("sum_above_2_32", "tiles", ["paired_base_length_above_2^32"], *tiny_mates(33000 * 2, len65535=True), render=False))
    for nt in (1023, 1024, 1025):
        C.append(PairCase("n_tiles_%d" % nt, "tiles", ["n_tiles=%d_clean" % nt], *tiny_mates((nt - 1) * PAIR_TILE + (1, 256, 77)[nt - 1023], big=True, arenas=False), render=False))
    return C


def big_size(n_cu=DEFAULT_CU):
    return max(n_cu * VOID_BLOCKS_PER_CU * 256, SCAN_THREADS * 512) + 3000


def big_cases(n_cu=DEFAULT_CU):
    """One big pair of mates, built once, and its variants: the texts alone differ (bit 0 of the first byte of mate 2's defline at the bad pairs)."""
    n = big_size(n_cu)
    m0, m1 = tiny_mates(n, big=True)
    t_bad = SCAN_THREADS + 300
    variants = (("big_clean", (), ["sums_from_second_round", "scan_carries_into_second_round"]),
                ("big_bad_at_3", (3, 900), ["void_tail_second_stride", "take_is_one_tile_of_many", "both_valid_pairs_right_behind_the_bad_pair"]),
                ("big_bad_beyond_round", (t_bad * PAIR_TILE + 77, (2 * SCAN_THREADS + 5) * PAIR_TILE + 3), ["first_bad_beyond_scan_round", "later_bad_in_lower_scan_slot", "sums_from_second_round"]),
                ("big_bad_last", (n - 1,), ["bad_last_pair_beyond_scan_round", "sums_from_second_round"]))
    C = []
    for name, bad, claims in variants:
        text = m1.text.copy()
        for b in bad:
            assert b < n, (name, b, n)
            text[int(m1.def_pos[b])] ^= 1
        C.append(PairCase(name, "big", claims, m0, m1.with_text(text), args="default" if name != "big_bad_beyond_round" else "replace_out64"))
    return C


def _read_mates(n, lens, route=None, salt=0, def_len=None, valid=None, qual_shift=0, n_lead=(None, None), n_trail=(None, None), starts=None):
    """Two mates with matching ids (route None: the pair call's own route from `valid`), deflines with '\\n' between them"""
    out = []
    for s in (0, 1):
        k = len(lens[s])
        i = np.arange(k, dtype=np.int64)
        idl = 2 + (i * 3) % 5
        dl = (idl + s * (2 + i % 3)) if def_len is None else np.asarray(def_len[s], np.int64)  # mate 2: the id, ' ' and a comment
        pos = np.cumsum(dl + 1) - dl - 1
        text = np.full(max(int((dl + 1).sum()) - 1 if k else 0, 1), 10, np.uint8)  # (a text of no bytes still needs a pointer)
        p = np.arange(int(dl.sum()), dtype=np.int64) - np.repeat(np.cumsum(dl) - dl, dl)
        ii = np.repeat(i, dl)
        body = 97 + _hash(ii * 11 + p) % 26  # the same id on both sides
        if def_len is None and s:
            body = np.where(p < np.repeat(idl, dl), body, np.where(p == np.repeat(idl, dl), 32, 65 + _hash(ii * 13 + p) % 26))
        text[np.repeat(pos, dl) + p] = body
        L = np.asarray(lens[s], np.int64)
        st = ((i * 3) % 5).clip(max=L) if starts is None else np.asarray(starts[s], np.int64)
        v = np.ones(k, np.int64) if valid is None else valid[s]
        out.append(Mate(text, pos, dl, L, st, L - st - ((L - st) > 4), v, n_lead=n_lead[s], n_trail=n_trail[s], salt=salt + 5000 * s + 1, qual_shift=qual_shift))
    return out


def _valid_of(route):
    r = np.asarray(route)
    return [(r & 1), (r >> 1) & 1]


def scan_cases():
    C = []
    ragged = lambda n, s: (np.arange(n) * (5 + 2 * s)) % 9
    route_mix = lambda n: (_hash(np.arange(n)) >> 2) % 4
    # -- the truth table of the route byte
    n = 256
    C.append(PairCase("route_truth_table", "scan", ["route_every_byte_value"], *_read_mates(n, [1 + ragged(n, 0), 2 + ragged(n, 1)]), route=np.arange(256)))
    for n in RENDER_SIZES:
        r = route_mix(n)
        C.append(PairCase("render_%d_pairs" % n, "scan", ["render_n_pairs=%d" % n] + (["odd_n_pairs_leaves_half_a_thread"] if n % 2 else []), *_read_mates(n, [ragged(n, 0), ragged(n, 1)], valid=_valid_of(r))))
    r = route_mix(600)
    C.append(PairCase("fewer_pairs_than_reads", "scan", ["n_pairs_below_both_n_reads_n1_ne_n2"], *_read_mates(0, [ragged(700, 0), ragged(650, 1)], valid=[np.ones(700, np.int64), np.arange(650) % 3 != 0]), route=r, n_pairs=600))
    n = 3 * 512 + 10
    i = np.arange(n)
    r = np.where(i // 512 == 1, ROUTE_NOWHERE, route_mix(n))
    C.append(PairCase("candidate_tile_dropped", "scan", ["candidate_tile_all_dropped"], *_read_mates(n, [ragged(n, 0), ragged(n, 1)]), route=r))
    # only mate 1 of pair 511 and mate 0 of pair 512 of the first two tiles: UNPAIRED takes route 2 then 1, DISCARD route 1 then 2
    for f, (ra, rb) in ((UNPAIRED, (2, 1)), (DISCARD, (1, 2))):
        r = np.where(i < 1024, 3 if f == DISCARD else 0, route_mix(n))
        r[511], r[512] = ra, rb
        C.append(PairCase("last_of_tile_first_of_next_file%d" % f, "scan", ["only_last_of_tile_then_only_first_of_next/" + ("UNPAIRED" if f == UNPAIRED else "DISCARD")],
                          *_read_mates(n, [1 + ragged(n, 0), 1 + ragged(n, 1)]), route=r))
    n = 5 * 512
    i = np.arange(n)
    C.append(PairCase("candidate_tiles_alternate", "scan", ["candidate_tiles_alternate_all_and_none"], *_read_mates(n, [ragged(n, 0), ragged(n, 1)]), route=np.where((i // 512) % 2 == 0, 0, ROUTE_NOWHERE)))
    # -- the overflow rule on a mid-sized case, each engine argument set
    for a, shift in (("default", 0), ("replace_out64", 0), ("ascii64", 31)):
        r = np.where(np.arange(700) >= 650, 0, route_mix(700))
        C.append(PairCase("mid_" + a, "scan", ["args=" + a] + ["overflow_one_byte_short/file%d" % f for f in FILES] + ["deflines_at_both_ends_of_both_texts"],
                          *_read_mates(700, [20 + ragged(700, 0) * 9, 30 + ragged(700, 1) * 7], valid=_valid_of(r), qual_shift=shift), args=a, overflow=True))
    C.append(PairCase("all_routed_3", "scan", ["empty_file_at_capacity_0"], *_read_mates(300, [ragged(300, 0), ragged(300, 1)]), overflow=True))
    # -- a thread's own sum beyond 2^32: four deflines of 0x60000000 bytes that nobody may read (the rendering alone, the discard file)
    m = _read_mates(3, [np.array([2, 3, 1]), np.array([1, 2, 4])])
    for x in m:
        x.def_pos[:] = 0
        x.def_len[:2] = 0x60000000
    C.append(PairCase("thread_sum_2_32", "scan", ["thread_sum_passes_2^32"], *m, route=np.zeros(3, np.uint8), files=(DISCARD,), pair=False, overflow="only", capacity=4096))
    return C


def _terminal_batch():
    return [b for b in pe.batch_cases("render") if b.name == "terminal_N"][0]


def source_cases():
    C = []
    # -- equal offsets and spans, every byte different
    n = 400
    i = np.arange(n)
    lens = 6 + (i * 7) % 40
    lead, trail = (i % 5 == 0) * (1 + i % 3), (i % 7 == 3) * (1 + i % 2)
    a, b = _read_mates(n, [lens, lens], def_len=[1 + i % 6, 1 + i % 6], n_lead=(lead, None), n_trail=(trail, None), starts=[i % 3, i % 3])
    T = a.total
    rot = np.zeros(256, np.uint8)
    rot[[65, 67, 71, 84, 78]] = [67, 71, 84, 65, 65]
    b._s[64:64 + T] = rot[a.seq[:T]]
    b._q[64:64 + T] = np.where(a.qual[:T] >= 74, 35, a.qual[:T] + 1)
    b.text = np.where(a.text == 10, 13, a.text + 1).astype(np.uint8)
    off = b.offset.astype(np.int64)
    for k in np.nonzero((i % 5 == 1) | (i % 7 == 4))[0]:  # mate 2's own runs, where mate 1 has none
        if i[k] % 5 == 1:
            b._s[64 + off[k]:64 + off[k] + 2] = 78
        else:
            b._s[64 + off[k + 1] - 1] = 78
    b.set_tn()
    b.res = a.res.copy()
    r = (_hash(i) >> 2) % 4
    C.append(PairCase("shadow_mates", "source", ["mates_share_offsets_and_differ_in_every_byte"], a, b, route=r, tn_forms=("both", "neither", "mate0", "mate1")))
    C.append(PairCase("shadow_mates_replace", "source", ["mates_share_offsets_and_differ_in_every_byte"], a, b, route=r, args="replace_out64"))
    # -- very different offsets
    n = 500
    i = np.arange(n)
    C.append(PairCase("short_against_long", "source", ["mates_of_very_different_offsets"], *_read_mates(n, [(i * 3) % 4, 100 + (i * 37) % 201], valid=_valid_of((_hash(i) >> 3) % 4))))
    # -- the terminal_N batch of pack_edges.py as one mate, an N-free mate of the same offsets as the other; and both with different runs
    t = _terminal_batch()
    lead, trail = _runs(t)
    n = t.n
    spans_of = lambda salt: _read_mates(n, [t.lens, t.lens], def_len=[1 + (np.arange(n) + salt) % 4] * 2)[0]

    def twin(lead=None, trail=None, salt=9):
        m = spans_of(salt)
        x = Mate(m.text, m.def_pos, m.def_len, t.lens, t.res["start"], t.res["len"], np.ones(n, np.int64), n_lead=lead, n_trail=trail, salt=salt)
        return x

    every = ("both", "neither", "mate0", "mate1")
    for rname, route in (("3", np.full(n, 3)), ("12", 1 + np.arange(n) % 2), ("21", 2 - np.arange(n) % 2)):
        plain, t_like = twin(), twin(lead, trail, salt=3)
        moved = twin(np.roll(lead, 7) % (t.lens + 1), np.roll(trail, 5) % (t.lens + 1), salt=4)
        C.append(PairCase("terminal_N_mate0_route" + rname, "source", ["terminal_N_mate0_only"] + ["terminal_n_pointer_" + f for f in every], t_like, plain, route=route, tn_forms=every))
        C.append(PairCase("terminal_N_mate1_route" + rname, "source", ["terminal_N_mate1_only"], plain, t_like, route=route, tn_forms=every))
        C.append(PairCase("terminal_N_both_route" + rname, "source", ["terminal_N_both_different_runs"], t_like, moved, route=route, tn_forms=every, args="replace_out64" if rname == "3" else "default"))
    # -- the batch itself as a mate: a pack_edges.Batch is a mate as it stands
    C.append(PairCase("terminal_N_batch_as_mate0", "source", ["terminal_N_mate0_only"], t, twin(salt=11), route=np.full(n, 3), tn_forms=every))
    # -- four flagged candidates in one thread, four run lengths
    n = 64
    i = np.arange(n)
    lens = 80 + (i % 4) * 10
    la, lb = 1 + (i % 2) * 64 + i // 2 % 3, 3 + (i % 2) * 60 + 7 + i // 2 % 3
    for rname, route in (("3", np.full(n, 3)), ("12", 1 + i % 2), ("0", np.zeros(n, np.int64))):
        C.append(PairCase("four_flagged_route" + rname, "source", ["four_candidates_of_a_thread_flagged_four_run_lengths"],
                          *_read_mates(n, [lens, lens + 5], n_lead=(la, lb), n_trail=((i % 3 == 0) * 2, None), starts=[i % 4, (i * 3) % 70]), route=route, tn_forms=every))
    return C


def gather_cases():
    C = []
    for lay in pe.layouts():
        if "render" not in lay.kinds:
            continue
        sizes = lay.sizes.tolist()
        R = len(sizes)
        claims = ["gather_across_mates:" + e for e in lay.claims]
        # UNPAIRED: record k is mate k mod 2 of pair k
        lens, dl, st = ([], []), ([], []), ([], [])
        for k, sz in enumerate(sizes):
            d, w = pe._render_split(sz)
            for s in (0, 1):
                if s == k % 2:
                    lens[s].append(w + (k * 3) % 5 + k % 3), dl[s].append(d), st[s].append((k * 3) % 5)
                else:
                    lens[s].append(k % 7), dl[s].append(k % 4), st[s].append(0)
        m = _read_mates(R, lens, def_len=dl, starts=st, salt=R)
        for s in (0, 1):
            own = np.arange(R) % 2 == s
            m[s].res["len"] = np.where(own, [pe._render_split(sz)[1] for sz in sizes], m[s].res["len"])
        C.append(PairCase("layout_%s_unpaired" % lay.name, "gather", claims, *m, route=1 + np.arange(R) % 2, files=(UNPAIRED, QC1)))
        # DISCARD: record k is mate k mod 2 of pair k div 2 (an odd last record: the pair's second mate is valid)
        P = (R + 1) // 2
        lens, dl = ([], []), ([], [])
        for k, sz in enumerate(sizes):
            d, w = pe._render_split(sz)
            lens[k % 2].append(w), dl[k % 2].append(d)
        if R % 2:
            lens[1].append(4), dl[1].append(2)
        route = np.zeros(P, np.int64)
        route[-1] = 2 if R % 2 else 0
        C.append(PairCase("layout_%s_discard" % lay.name, "gather", claims, *_read_mates(P, lens, def_len=dl, salt=R + 1), route=route, files=(DISCARD, UNPAIRED)))
    # records of 5 - 15 bytes: empty deflines, 0 - 5 bases
    P = 300
    i = np.arange(P)
    C.append(PairCase("records_of_5_to_15_bytes", "gather", ["three_records_of_mates_0_1_0_in_one_piece"], *_read_mates(P, [(i % 7 == 3) * (i % 6), (i % 5 == 1) * ((i * 3) % 6)], def_len=[0 * i, 0 * i]),
                      route=np.zeros(P, np.int64), files=(DISCARD,)))
    return C


def all_cases(n_cu=DEFAULT_CU, big=True):
    return id_cases() + compare_cases() + tile_cases() + scan_cases() + source_cases() + gather_cases() + (big_cases(n_cu) if big else [])


def hits(case, n_cu=DEFAULT_CU):
    c = case.ctx()
    return {e for e, p in edges(n_cu).items() if p(c)}


def coverage(cases=None, n_cu=DEFAULT_CU):
    """-> {edge: [names of the cases that reach it]} over every case, and {case name: edges reached}"""
    cases = all_cases(n_cu) if cases is None else cases
    table, per_case = {e: [] for e in required()}, {}
    for case in cases:
        h = hits(case, n_cu)
        per_case[case.name] = h
        for e in h:
            table[e].append(case.name)
    return table, per_case


if __name__ == "__main__":
    table, _ = coverage()
    for edge, names in sorted(table.items()):
        print("%-64s %3d  %s" % (edge, len(names), ", ".join(names[:3]) + (" ..." if len(names) > 3 else "")))
    print("%d edges, %d unreached" % (len(table), sum(not v for v in table.values())))
