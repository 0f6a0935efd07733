"""Deflate streams written bit by bit for the inflate tests: the streams zlib's encoder never writes.  A bit writer, block builders (stored,
fixed, dynamic with explicit code lengths, explicit code-length-code operations and an explicit HCLEN), a token expander (plain LZ77 copy:
the expected text of a valid stream without any inflater) and a catalogue of named cases, valid and invalid.  Plain Python and numpy from
RFC 1951; no code of zlib, of the reference or of the library under test.  The catalogue is a pure function of inflate_cases.SEED: the
streams proven on the host are byte for byte the streams sent to the device."""
import collections
import functools
import heapq

import numpy as np

import inflate_cases as ic
from faqcs_amd import _capi as capi

E_DATA, E_LENGTH = capi.INFLATE_E_DATA, capi.INFLATE_E_LENGTH

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8   # 286 and 287 take part in the code
FIXED_DIST = [5] * 32                                     # and so do 30 and 31
PLAIN_LIT = [8] * 226 + [9] * 60                          # complete sets without a story
PLAIN_DIST = [4] * 2 + [5] * 28
# {length: codes} of complete sets with SEVERAL codes of every length the primary tables (10 and 8 bits) do not hold: the canonical walk has
# to rank them
LADDER_LIT = {7: 70, 8: 90, 9: 32, 10: 32, 11: 8, 12: 8, 13: 8, 14: 8, 15: 16}
LADDER_DIST = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 9: 2, 10: 2, 11: 2, 12: 2, 13: 2, 14: 2, 15: 4}


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, v, n):
        """n bits of v, the least significant first (header fields, extra bits)"""
        assert 0 <= v < (1 << n), (v, n)
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        """a Huffman code of n bits, the most significant first"""
        r = 0
        for _ in range(n):
            r = r << 1 | (c & 1)
            c >>= 1
        self.bits(r, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """{symbol: (code, bits)} of the canonical code of RFC 1951 section 3.2.2.  Broken sets get codes too (cut to their length): the decoder
    has to refuse them at the table, whatever follows."""
    count = collections.Counter(l for l in lens if l)
    code, nxt = 0, {}
    for b in range(1, 17):
        code = (code + count.get(b - 1, 0)) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def kraft(lens, maxbits=15):
    """the code space the set takes, in units of 2^-maxbits: 2^maxbits is a complete set"""
    return sum(1 << (maxbits - l) for l in lens if l)


def limited_lens(freqs, maxbits):
    """Code lengths <= maxbits of a COMPLETE prefix code for the symbols with a frequency (at least two): Huffman's lengths, cut at maxbits,
    the code space then repaired by lengthening the longest codes that can grow and shortening the longest that fit."""
    syms = [s for s, f in enumerate(freqs) if f > 0]
    assert len(syms) >= 2
    heap = [(freqs[s], s, (s,)) for s in syms]
    heapq.heapify(heap)
    depth = dict.fromkeys(syms, 0)
    while len(heap) > 1:
        fa, ta, a = heapq.heappop(heap)
        fb, tb, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, min(ta, tb), a + b))
    lens = {s: min(d, maxbits) for s, d in depth.items()}
    full, k = 1 << maxbits, sum(1 << (maxbits - l) for l in lens.values())
    while k > full:
        s = max((s for s in syms if lens[s] < maxbits), key=lambda s: (lens[s], -freqs[s], s))
        lens[s] += 1
        k -= 1 << (maxbits - lens[s])
    while k < full:
        s = max((s for s in syms if (1 << (maxbits - lens[s])) <= full - k), key=lambda s: (lens[s], freqs[s], -s))
        k += 1 << (maxbits - lens[s])
        lens[s] -= 1
    out = [0] * len(freqs)
    for s, l in lens.items():
        out[s] = l
    return out


def dealt_lens(rng, n, counts, must=()):
    """the lengths of `counts` ({length: codes}, a complete set) dealt at random over n symbols, those of `must` among them"""
    order = [int(v) for v in rng.permutation(n)]
    total = sum(counts.values())
    for m in must:
        if order.index(m) >= total:
            i = int(rng.integers(0, total))
            j = order.index(m)
            order[i], order[j] = order[j], order[i]
    lens, at = [0] * n, 0
    for l in sorted(counts):
        for s in order[at:at + counts[l]]:
            lens[s] = l
        at += counts[l]
    assert kraft(lens) == 1 << 15
    return lens


def chain_lens(symbols, n):
    """lengths 1, 2, ..., m - 1, m - 1 over the m <= 16 symbols in the order given (complete), 0 for the rest of the n"""
    assert 2 <= len(symbols) <= 16
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, len(symbols) - 1)
    return lens


def expand_ops(ops):
    """the code lengths a list of code-length-code operations states: an int is a length, (16, n) n times the one in front, (17, n) and
    (18, n) n zeros"""
    out = []
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        elif op[0] == 16:
            out += [out[-1] if out else 0] * op[1]
        else:
            out += [0] * op[1]
    return out


def rle_ops(lens, split=()):
    """greedy operations for `lens`: 18 for 11 .. 138 zeros, 17 for 3 .. 10, 16 for 3 .. 6 repeats; no run crosses an index in `split`"""
    ops, i, n = [], 0, len(lens)
    cuts = sorted(set(split) | {n})
    while i < n:
        stop = min(c for c in cuts if c > i)
        j = i
        while j < stop and lens[j] == lens[i]:
            j += 1
        run = j - i
        if lens[i] == 0:
            while run >= 3:
                r = min(run, 138)
                ops.append((18, r) if r >= 11 else (17, r))
                run -= r
            ops += [0] * run
        else:
            ops.append(lens[i])
            run -= 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r))
                run -= r
            ops += [lens[i]] * run
        i = j
    return ops


def length_symbol(length):
    c = max(i for i in range(29) if LEN_BASE[i] <= length)
    return 257 + c, length - LEN_BASE[c]


def distance_symbol(dist):
    d = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return d, dist - DIST_BASE[d]


def expand(items):
    """The text of a stream's blocks by plain LZ77 copy.  items: ("stored", bytes) and ("huffman", tokens); a token is a literal (int), a
    match (length, distance), or the raw pair ("L", symbol, extra), ("D", symbol, extra) -- with a fourth entry, the number of extra bits to
    write, for the symbols that have no meaning.  ValueError for what is no valid deflate."""
    out = bytearray()
    for kind, payload in items:
        if kind == "stored":
            out += payload
            continue
        pending = None
        for t in payload:
            if isinstance(t, int):
                assert pending is None
                out.append(t)
                continue
            if t[0] == "L":
                if not 257 <= t[1] <= 285:
                    raise ValueError("length symbol %d" % t[1])
                pending = LEN_BASE[t[1] - 257] + t[2]
                continue
            if t[0] == "D":
                if t[1] >= 30:
                    raise ValueError("distance symbol %d" % t[1])
                length, dist = pending, DIST_BASE[t[1]] + t[2]
                pending = None
            else:
                length, dist = t
            if dist > len(out):
                raise ValueError("distance %d at %d" % (dist, len(out)))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
        assert pending is None
    return bytes(out)


class Stream:
    """One deflate stream under construction.  It records what it emitted: the blocks for expand(), every field's bit range (for the
    truncations), and the coverage: code lengths of emitted symbols per alphabet, block types, header values, repeats across the
    literal / distance boundary."""

    def __init__(self):
        self.w = BitWriter()
        self.items, self.fields, self.block_types, self.headers, self.cross = [], [], [], [], []
        self.used = {"lit": set(), "dist": set(), "cl": set()}
        self.ranks = {"lit": set(), "dist": set()}   # (length, rank among the codes of that length) of emitted symbols
        self.grid = set()

    def _field(self, kind, start):
        self.fields.append((kind, start, self.w.bitpos))

    def _header(self, final, btype):
        a = self.w.bitpos
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)
        self._field("block_header", a)
        self.block_types.append(btype)

    def stored(self, data, final=False, length=None, nlen=None):
        """length / nlen: LEN and NLEN to state instead of the true ones"""
        data = bytes(data)
        self._header(final, 0)
        self.w.align()
        n = len(data) if length is None else length
        a = self.w.bitpos
        self.w.bits(n, 16)
        self.w.bits(n ^ 0xFFFF if nlen is None else nlen, 16)
        self._field("len_nlen", a)
        a = self.w.bitpos
        self.w.raw(data)
        if data:
            self._field("stored_data", a)
        self.items.append(("stored", data))
        return self

    def _tokens(self, tokens, lit_lens, dist_lens, eob):
        lit, dist = canonical(lit_lens), canonical(dist_lens)
        first = {"lit": {}, "dist": {}}
        for a, codes in (("lit", lit), ("dist", dist)):
            for c, l in codes.values():
                first[a][l] = min(c, first[a].get(l, c))
        w = self.w

        def put_lit(sym, extra, nbits):
            a = w.bitpos
            w.code(*lit[sym])
            self._field("symbol", a)
            self.used["lit"].add(lit[sym][1])
            self.ranks["lit"].add((lit[sym][1], lit[sym][0] - first["lit"][lit[sym][1]]))
            if nbits:
                a = w.bitpos
                w.bits(extra, nbits)
                self._field("length_extra", a)

        def put_dist(sym, extra, nbits):
            a = w.bitpos
            w.code(*dist[sym])
            self._field("distance_symbol", a)
            self.used["dist"].add(dist[sym][1])
            self.ranks["dist"].add((dist[sym][1], dist[sym][0] - first["dist"][dist[sym][1]]))
            if nbits:
                a = w.bitpos
                w.bits(extra, nbits)
                self._field("distance_extra", a)

        for t in tokens:
            if isinstance(t, int):
                put_lit(t, 0, 0)
            elif t[0] == "L":
                put_lit(t[1], t[2], t[3] if len(t) > 3 else LEN_EXTRA[t[1] - 257])
            elif t[0] == "D":
                put_dist(t[1], t[2], t[3] if len(t) > 3 else DIST_EXTRA[t[1]])
            else:
                s, e = length_symbol(t[0])
                put_lit(s, e, LEN_EXTRA[s - 257])
                s, e = distance_symbol(t[1])
                put_dist(s, e, DIST_EXTRA[s])
        if eob:
            put_lit(256, 0, 0)
        self.items.append(("huffman", list(tokens)))

    def fixed(self, tokens, final=False, eob=True):
        self._header(final, 1)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST, eob)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, ops=None, cl_lens=None, hclen=None, hlit=None, hdist=None, cross=True,
                eob=True, check=True):
        """lit_lens / dist_lens: the code lengths the tokens are written with, and (by their sizes) HLIT and HDIST unless given.  ops: the
        code-length-code operations to send (default: rle_ops, runs crossing the literal / distance boundary when `cross`); cl_lens: the 19
        lengths of the code-length code (default: a complete code of at most 7 bits for the operations); hclen: how many of them are sent
        (default: up to the last that is not 0).  check: the operations state exactly lit_lens + dist_lens (off for broken headers)."""
        w = self.w
        nlit, ndist = len(lit_lens) if hlit is None else hlit, len(dist_lens) if hdist is None else hdist
        lens = list(lit_lens) + list(dist_lens)
        if ops is None:
            ops = rle_ops(lens, () if cross else (len(lit_lens),))
        if check:
            assert expand_ops(ops) == lens and nlit == len(lit_lens) and ndist == len(dist_lens)
        syms = [op if isinstance(op, int) else op[0] for op in ops]
        if cl_lens is None:
            freq = [0] * 19
            for s in syms:
                freq[s] += 1
            if sum(1 for f in freq if f) < 2:   # (a single code of one bit is no code-length code: give it a neighbour)
                freq[1 if freq[0] else 0] += 1
            cl_lens = limited_lens(freq, 7)
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
        self._header(final, 2)
        a = w.bitpos
        w.bits(nlit - 257, 5)
        w.bits(ndist - 1, 5)
        w.bits(hclen - 4, 4)
        self._field("counts", a)
        self.headers.append((nlit, ndist, hclen))
        a = w.bitpos
        for i in range(hclen):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        self._field("cl_lens", a)
        cl = canonical(cl_lens)
        at = 0
        for op, s in zip(ops, syms):
            a = w.bitpos
            w.code(*cl[s])
            self._field("code_length", a)
            self.used["cl"].add(cl[s][1])
            rep = 1
            if s >= 16:
                rep = op[1]
                base, nb = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[s]
                a = w.bitpos
                w.bits(rep - base, nb)
                self._field("code_length_extra", a)
                if at < nlit < at + rep:
                    self.cross.append(s)
            at += rep
        self._tokens(tokens, lit_lens, dist_lens, eob)
        return self

    def getvalue(self):
        return self.w.getvalue()


Case = collections.namedtuple("Case", "name member text code kind refusal stream")
# name, member bytes, expected text (None: invalid), expected error code (None: valid); kind: the bullet of the catalogue the case stands for;
# refusal: how the yardstick refuses an invalid case -- "error" (zlib.error), "incomplete" (zlib wants more input), "leftover" (zlib ends in
# front of the trailer), "trailer" (ISIZE / CRC differ from zlib's text); stream: the Stream, for the coverage table

GRID_K = (0, 1, 31, 63)
GRID_LEN = (3, 4, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 258)
GRID_DIST = (1, 2, 3, 63, 64, 65, "len-1", "len", "len+1", 32768, "o")
INVALID_KINDS = ("first_code_length_16", "repeat_overruns", "no_end_of_block", "lit_oversubscribed", "lit_incomplete", "dist_oversubscribed",
                 "dist_incomplete", "cl_oversubscribed", "cl_incomplete", "cl_single_one_bit", "hlit_too_large", "hdist_too_large",
                 "fixed_symbol_286", "fixed_symbol_287", "fixed_distance_30", "fixed_distance_31", "len_nlen_mismatch", "stored_past_input",
                 "stored_past_isize", "match_past_isize", "literal_past_isize", "distance_in_front_fixed", "distance_in_front_dynamic",
                 "truncated_block_header", "truncated_counts", "truncated_cl_lens", "truncated_code_length", "truncated_code_length_extra",
                 "truncated_symbol", "truncated_length_extra", "truncated_distance_symbol", "truncated_distance_extra", "truncated_len_nlen",
                 "extra_byte", "no_final_block")


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _skewed(rng, n, ratio):
    """frequencies that fall by `ratio` per rank, the ranks dealt at random: a Huffman code far deeper than 15"""
    f = [max(1, int(2.0 ** 60 / ratio ** r)) for r in range(n)]
    return [f[i] for i in rng.permutation(n)]


def _sweep_tokens(rng, lit_lens, dist_lens, o):
    """every literal, length symbol and distance symbol that has a code, at least once, behind o bytes of history"""
    toks = [s for s in rng.permutation(256).tolist() if lit_lens[s]]
    o += len(toks)
    ls = [s for s in range(257, 286) if s < len(lit_lens) and lit_lens[s]]
    ds = [d for d in range(30) if d < len(dist_lens) and dist_lens[d] and DIST_BASE[d] <= o]
    for i in range(max(len(ls), len(ds)) if ls and ds else 0):
        s, d = ls[i % len(ls)], ds[i % len(ds)]
        le = int(rng.integers(0, 1 << LEN_EXTRA[s - 257]))
        de = min(int(rng.integers(0, 1 << DIST_EXTRA[d])), o - DIST_BASE[d])
        toks += [("L", s, le), ("D", d, de)]
        o += LEN_BASE[s - 257] + le
    return toks


def _grid_members(rng):
    """The (k, len, dist) grid: a stored block of random bytes (history, and the choice of o mod 64), then one Huffman block per combination
    -- k literals, the match, one literal -- alternately fixed and dynamic; in front of every other one an empty stored block, so that the
    k literals are exactly what waits (else the literal behind the match in front waits with them).  dist = 32768 lives in members with
    32 768 bytes of history and more, dist = o in members that are still shorter."""
    combos = [(k, ln, d) for d in GRID_DIST for ln in GRID_LEN for k in GRID_K]
    near = [c for c in combos if c[2] != 32768]
    far = [c for c in combos if c[2] == 32768]
    out = []

    def build(part, first, idx):
        s = Stream()
        front = _rand(rng, first)
        s.stored(front)
        o = first
        for j, (k, ln, dk) in enumerate(part):
            dist = {"len-1": ln - 1, "len": ln, "len+1": ln + 1, "o": o + k}.get(dk, dk)
            assert 1 <= dist <= o + k and dist <= 32768, (k, ln, dk, o)
            toks = rng.integers(0, 256, k).tolist() + [(ln, dist), int(rng.integers(0, 256))]
            if j % 2:
                s.stored(b"")
            if (j + idx) % 3 == 0:
                s.fixed(toks)
            else:
                s.dynamic(toks, PLAIN_LIT, PLAIN_DIST)
            s.grid.add((k, ln, dk))
            o += k + ln + 1
        s.stored(b"", final=True)
        assert o <= 65536
        out.append(s)

    per = 44
    for i in range(0, len(near), per):
        build(near[i:i + per], 260 + (i // per) * 37 % 64 + int(rng.integers(0, 64)), i // per)   # (o + 63 + 258 + 1) * 44 < 32 768
    for i in range(0, len(far), 26):
        build(far[i:i + 26], 32768 + int(rng.integers(0, 64)), i // 26)
    return out


def _valid_streams(rng):
    """[(name, kind, Stream)] of the valid cases outside the grid"""
    out = []

    def add(name, kind, s):
        out.append((name, kind, s))

    # ---- the canonical walk: codes longer than the primary tables -------------------------------------------------------------------
    lits = [65, 67, 71, 84, 10, 64, 43, 73, 78, 35]
    for name, order in (("lit_chain_eob_15_bits", lits + [257, 258, 260, 285, 33, 256]), ("lit_chain_literals_15_bits", [256, 285, 257, 270, 264, 258] + lits),
                        ("lit_chain_lengths_15_bits", [256] + lits[:6] + [65 + 100, 200, 255, 0, 257, 258, 284, 285, 270])):
        lens = chain_lens(order, 286)
        toks = [s for s in order if s < 256] * 2
        for s in order:
            if s > 256:
                toks += [("L", s, (1 << LEN_EXTRA[s - 257]) - 1), ("D", len(toks) % 4, 0), order[1] if order[1] < 256 else 65]
        add(name, "canonical_walk", Stream().dynamic(toks, lens, PLAIN_DIST, final=True))
    for name, syms, first in (("dist_chain_near", list(range(16)), 300), ("dist_chain_far", list(range(14, 30)), 32768 + 77)):
        order = [syms[i] for i in rng.permutation(16)]
        dl = chain_lens(order, 30)
        toks = []
        for rep in range(2):
            for d in order:
                ln = int(rng.integers(3, 259))
                toks += [(ln, DIST_BASE[d] + (((1 << DIST_EXTRA[d]) - 1) if rep else 0)), int(rng.integers(0, 256))]
        add(name, "canonical_walk", Stream().stored(_rand(rng, first)).dynamic(toks, PLAIN_LIT, dl, final=True))
    for i in range(3):
        if i == 0:
            ll, dl = limited_lens(_skewed(rng, 286, 1.12), 15), limited_lens(_skewed(rng, 30, 2.4), 15)
        else:
            ll, dl = dealt_lens(rng, 286, LADDER_LIT, must=(256,)), dealt_lens(rng, 30, LADDER_DIST)
        s = Stream().stored(_rand(rng, 32768 + i))
        s.dynamic(_sweep_tokens(rng, ll, dl, 32768 + i), ll, dl, final=True, hclen=19 if i == 0 else None)
        add("sweep_length_limited" if i == 0 else "sweep_many_long_codes_%d" % i, "canonical_walk", s)
    # ---- the code-length code fills its 7 bits ---------------------------------------------------------------------------------------
    ll = [0] * 10 + [6] * 32 + [7] * 16 + [8] * 64 + [9] * 63 + [0] * 71 + [9]
    cl = [0] * 19
    for i, c in enumerate([8, 9, 7, 6, 0, 18, 17, 16]):
        cl[c] = min(i + 1, 7)
    toks = [int(v) for v in rng.integers(10, 185, 400)]
    add("code_length_code_7_bits", "code_length_code", Stream().dynamic(toks, ll, [0, 0, 0, 0], final=True, cl_lens=cl))
    # ---- the dynamic header's corners -------------------------------------------------------------------------------------------------
    ll = [0] + [8] * 256
    toks = [int(v) for v in rng.integers(1, 256, 300)]
    s = Stream().dynamic(toks, ll, [0], final=True, ops=[0, 8] + [(16, 6)] * 42 + [(16, 3), 0], cl_lens=[2 if c in (0, 8) else 1 if c == 16 else 0 for c in range(19)])
    assert s.headers == [(257, 1, 5)]
    add("hlit_257_hdist_1_hclen_5_no_distance_code", "header_corners", s)
    toks = [int(v) for v in rng.integers(0, 180, 200)] + [(258, 200), (3, 1), 7]
    add("hlit_257_hdist_30", "header_corners", Stream().dynamic(toks[:200], [8] * 255 + [9, 9], PLAIN_DIST, final=True))
    add("hlit_286_hdist_1_one_bit_distance", "header_corners", Stream().dynamic(toks[:200] + [(258, 1), 6, (3, 1), 7], PLAIN_LIT, [1], final=True))
    add("hlit_286_hdist_30_hclen_19", "header_corners", Stream().dynamic(toks, PLAIN_LIT, PLAIN_DIST, final=True, hclen=19))
    add("no_distance_code_hdist_30", "header_corners", Stream().dynamic(toks[:200], PLAIN_LIT, [0] * 30, final=True))
    toks7 = [int(v) for v in rng.integers(0, 256, 40)] + [("L", 280, 9), ("D", 7, 3), 1, ("L", 257, 0), ("D", 7, 0), 2]
    add("one_bit_distance_code_symbol_7", "header_corners", Stream().dynamic(toks7, PLAIN_LIT, [0] * 7 + [1], final=True))
    add("literal_set_is_256_alone", "header_corners", Stream().stored(b"@r\nACGT\n+\nIIII\n").dynamic([], [0] * 256 + [1], [0], final=True))
    add("literal_set_is_256_alone_empty_member", "header_corners", Stream().dynamic([], [0] * 256 + [1], [0], final=True))
    for name, ll, dl in (("repeat_16_across_the_boundary", [8] * 164 + [9] * 120 + [4, 4], PLAIN_DIST),
                         ("repeat_17_across_the_boundary", [8] * 228 + [9] * 56 + [0, 0], [0, 0] + [4] * 4 + [5] * 24),
                         ("repeat_18_across_the_boundary", [8] * 234 + [9] * 44 + [0] * 8, [0] * 6 + [4] * 8 + [5] * 16)):
        tk = [int(v) for v in rng.integers(0, 200, 100)] + [(40, 100), 3, (70, 70), 5]
        s = Stream().dynamic(tk, ll, dl, final=True)
        assert len(s.cross) == 1
        add(name, "header_corners", s)
    ll = [8] * 200 + [0] * 6 + [8] * 50 + [9] * 12 + [0] * 18
    add("repeat_16_behind_17", "header_corners", Stream().dynamic(toks[:100] + [(9, 50), 4], ll, PLAIN_DIST, final=True, ops=[8] + [(16, 6)] * 32 + [(16, 4), (16, 3)] + [(17, 3), (16, 3)] +
                                                                  [8] + [(16, 6)] * 8 + [8] + [9] * 12 + [(17, 6), (16, 6), (16, 6)] + rle_ops(PLAIN_DIST)))
    ll = [8] * 180 + [0] * 26 + [8] * 76 + [0] * 4
    add("repeat_16_behind_18", "header_corners", Stream().dynamic([int(v) for v in rng.integers(0, 180, 100)] + [(9, 50), 4], ll, PLAIN_DIST, final=True,
                                                                  ops=[8] + [(16, 6)] * 29 + [(16, 5)] + [(18, 20), (16, 6)] + [8] + [(16, 6)] * 12 + [(16, 3)] + [(17, 4)] + rle_ops(PLAIN_DIST)))
    head = rle_ops(PLAIN_LIT[:226]) + [9] + [(16, 6)] * 4   # 251 lengths
    for name, mid in (("end_of_block_length_first_of_a_repeat", [(16, 5), (16, 3)] + [9] * 27), ("end_of_block_length_inside_a_repeat", [(16, 3), (16, 6)] + [9] * 26),
                      ("end_of_block_length_last_of_a_repeat", [(16, 6)] + [9] * 29)):
        add(name, "header_corners", Stream().dynamic(toks, PLAIN_LIT, PLAIN_DIST, final=True, ops=head + mid + rle_ops(PLAIN_DIST)))
    # ---- fixed blocks -------------------------------------------------------------------------------------------------------------------
    s = Stream().stored(_rand(rng, 32768 + 5))
    add("fixed_every_symbol", "fixed", s.fixed(_sweep_tokens(rng, FIXED_LIT[:286], FIXED_DIST[:30], 32768 + 5), final=True))
    add("fixed_258_as_285_and_as_284_with_31", "fixed", Stream().fixed([1, 2, 3, ("L", 285, 0), ("D", 2, 0), 4, ("L", 284, 31), ("D", 0, 0), (258, 258), 9], final=True))
    add("fixed_neighbours_of_the_refused_symbols", "fixed", Stream().stored(_rand(rng, 32768)).fixed([("L", 285, 0), ("D", 29, 8191), 0, ("L", 284, 30), ("D", 28, 8191), 255], final=True))
    # ---- the wave's literals, stored blocks and what waits in the lanes -----------------------------------------------------------------
    for front in (0, 1, 37, 63):
        for k in (0, 1, 63, 64, 65):
            s = Stream()
            if front:
                s.stored(_rand(rng, front))
            add("flush_%d_literals_waiting_at_%d" % (k, front), "wave_sink", s.fixed(rng.integers(0, 256, k).tolist(), final=True))
    for j in range(8):   # 8 n + 13 bits in front of LEN: the stored bytes start at every alignment
        s = Stream().fixed(rng.integers(0, 256, 5 + j).tolist()).stored(_rand(rng, 100 + j)).fixed([(30, 100), 1, (100, 105 + j), 2]).stored(_rand(rng, 64))
        add("stored_behind_%d_literals" % (5 + j), "wave_sink", s.dynamic([(258, 64), (4, 170), 0], PLAIN_LIT, PLAIN_DIST, final=True))
    s = Stream().stored(_rand(rng, 1000)).fixed([(258, 1000), (200, 1258), 1]).stored(_rand(rng, 333)).dynamic([(129, 333), (65, 64), (64, 1791 + 129 + 65)], PLAIN_LIT, PLAIN_DIST, final=True)
    add("matches_reach_back_into_stored_blocks", "wave_sink", s)
    # ---- many blocks per member ---------------------------------------------------------------------------------------------------------
    s = Stream()
    o = 0
    for b in range(640):
        n = 1 + b % 5
        toks = rng.integers(33, 127, n).tolist()
        if o > 70 and b % 3 != 2 and b % 4 < 2:
            toks.append((3 + b % 17, 1 + b % 70))
            o += 3 + b % 17
        o += n
        if b % 3 == 0:
            freq = [0] * 286
            for t in toks:
                freq[t if isinstance(t, int) else length_symbol(t[0])[0]] += 1 + b % 3
            freq[256] = 1
            if len(toks) > n:
                s.dynamic(toks, limited_lens(freq, 15), chain_lens([distance_symbol(toks[-1][1])[0], (b // 3) % 5 + 20], 30))
            else:
                s.dynamic(toks, limited_lens(freq, 15)[:257], [0])
        elif b % 3 == 1:
            s.fixed(toks)
        else:
            s.stored(bytes(toks))
    add("many_blocks_640_mixed", "many_blocks", s.fixed([10], final=True))
    s = Stream()
    for _ in range(40):
        s.stored(b"")
    s.fixed(list(b"@read\n"))
    for _ in range(40):
        s.stored(b"")
    s.dynamic(list(b"ACGT") + [(40, 4)], PLAIN_LIT, PLAIN_DIST)
    for _ in range(39):
        s.stored(b"")
    add("runs_of_empty_stored_blocks", "many_blocks", s.stored(b"", final=True))
    add("fixed_first_stored_later", "many_blocks", Stream().fixed([1, 2, 3]).stored(b"xyz").dynamic([(5, 6)], PLAIN_LIT, PLAIN_DIST).fixed([4], final=True))
    # ---- the limits, from inside ----------------------------------------------------------------------------------------------------------
    add("text_of_65536_ends_with_a_match", "limits", Stream().stored(_rand(rng, 4)).fixed([(258, 3)] * 253 + [(258, 258)], final=True))
    assert 4 + 254 * 258 == 65536
    add("text_of_65536_ends_with_a_stored_block", "limits", Stream().stored(_rand(rng, 1)).fixed([(258, 1)] * 253).stored(_rand(rng, 65536 - 1 - 253 * 258), final=True))
    for name, fx in (("distance_equals_o_deep_fixed", True), ("distance_equals_o_deep_dynamic", False)):
        s = Stream().stored(_rand(rng, 20000))
        tk = [7, 8, (258, 20002), 9, (3, 20261), 1]
        add(name, "limits", s.fixed(tk, final=True) if fx else s.dynamic(tk, PLAIN_LIT, PLAIN_DIST, final=True))
    return out


def _cut(s, kind):
    """the stream's bytes, ended at a byte boundary inside (or at the start of) the first field of `kind` that allows it"""
    for k, a, e in s.fields:
        n = (e - 1) // 8
        if k == kind and a <= 8 * n < e and 8 * n > 0:
            return s.getvalue()[:n]
    raise AssertionError("no field of kind %s crosses a byte boundary" % kind)


def _invalid_cases(rng):
    """[(name, kind, code, refusal, raw stream bytes, text the trailer states)]: one defect each"""
    out = []
    text = ic.fastq_text(rng, 600, 50)
    toks = list(text[:300])

    def add(name, kind, code, refusal, raw, stated=text[:300]):
        out.append((name, kind, code, refusal, raw, stated))

    def dyn(**kw):
        a = dict(tokens=toks, lit_lens=PLAIN_LIT, dist_lens=PLAIN_DIST, final=True, check=False)
        a.update(kw)
        return Stream().dynamic(**a).getvalue()

    lens = PLAIN_LIT + PLAIN_DIST
    # ---- the dynamic header ----------------------------------------------------------------------------------------------------------
    add("first_code_length_symbol_is_16", "first_code_length_16", E_DATA, "error", dyn(lit_lens=[0] * 3 + [8] * 229 + [9] * 54, ops=[(16, 3)] + rle_ops([8] * 229 + [9] * 54 + PLAIN_DIST)))   # (were it three zeros, the rest would be sound)
    add("repeat_16_overruns_the_lengths", "repeat_overruns", E_DATA, "error", dyn(ops=rle_ops(lens[:-2]) + [(16, 3)]))
    add("repeat_17_overruns_the_lengths", "repeat_overruns", E_DATA, "error", dyn(ops=rle_ops(lens[:-2]) + [(17, 3)], cl_lens=None))
    add("repeat_18_overruns_the_lengths", "repeat_overruns", E_DATA, "error", dyn(ops=rle_ops(lens[:-5]) + [(18, 11)]))
    gap = PLAIN_LIT[:250] + [0] * 10 + PLAIN_LIT[260:]
    add("zeros_of_17_cover_256", "no_end_of_block", E_DATA, "error", dyn(ops=rle_ops(PLAIN_LIT[:250]) + [(17, 10)] + rle_ops(PLAIN_LIT[260:] + PLAIN_DIST), lit_lens=gap, eob=False))
    gap = PLAIN_LIT[:240] + [0] * 30 + PLAIN_LIT[270:]
    add("zeros_of_18_cover_256", "no_end_of_block", E_DATA, "error", dyn(ops=rle_ops(PLAIN_LIT[:240]) + [(18, 30)] + rle_ops(PLAIN_LIT[270:] + PLAIN_DIST), lit_lens=gap, eob=False))
    gap = PLAIN_LIT[:250] + [0] * 9 + PLAIN_LIT[259:]
    add("zeros_of_16_behind_17_cover_256", "no_end_of_block", E_DATA, "error",
        dyn(ops=rle_ops(PLAIN_LIT[:250]) + [(17, 4), (16, 5)] + rle_ops(PLAIN_LIT[259:] + PLAIN_DIST), lit_lens=gap, eob=False))
    add("hclen_4_states_no_length_at_all", "no_end_of_block", E_DATA, "error",
        dyn(tokens=[], lit_lens=[0] * 257, dist_lens=[0], ops=[(18, 138), (18, 120)], cl_lens=[1 if c in (0, 18) else 0 for c in range(19)], hclen=4, eob=False))
    add("literal_set_oversubscribed", "lit_oversubscribed", E_DATA, "error", dyn(lit_lens=[8] * 227 + [9] * 59))
    add("literal_set_incomplete", "lit_incomplete", E_DATA, "error", dyn(lit_lens=[8] * 225 + [9] * 61))
    add("literal_set_two_codes_of_two_bits", "lit_incomplete", E_DATA, "error", dyn(tokens=[65, 65], lit_lens=[0] * 65 + [2] + [0] * 190 + [2], dist_lens=[0]))
    add("distance_set_three_codes_of_one_bit", "dist_oversubscribed", E_DATA, "error", dyn(dist_lens=[1, 1, 1]))
    add("distance_set_oversubscribed", "dist_oversubscribed", E_DATA, "error", dyn(dist_lens=[4] * 3 + [5] * 27))
    add("distance_set_two_codes_of_two_bits", "dist_incomplete", E_DATA, "error", dyn(dist_lens=[2, 2]))
    add("distance_set_incomplete", "dist_incomplete", E_DATA, "error", dyn(dist_lens=[4] * 1 + [5] * 29))
    add("distance_set_one_code_of_two_bits", "dist_incomplete", E_DATA, "error", dyn(dist_lens=[2]))
    ops = rle_ops(lens)
    used = sorted({op if isinstance(op, int) else op[0] for op in ops})
    assert used == [4, 5, 8, 9, 16]
    cl = lambda **kw: [kw.get("l%d" % c, 0) for c in range(19)]  # noqa: E731
    add("code_length_set_oversubscribed", "cl_oversubscribed", E_DATA, "error", dyn(ops=ops, cl_lens=cl(l4=2, l5=2, l8=2, l9=2, l16=2)))
    add("code_length_set_incomplete", "cl_incomplete", E_DATA, "error", dyn(ops=ops, cl_lens=cl(l4=3, l5=3, l8=2, l9=2, l16=3)))
    add("code_length_set_one_code_of_one_bit", "cl_single_one_bit", E_DATA, "error",
        dyn(tokens=[], lit_lens=[0] * 257, dist_lens=[0], ops=[(18, 138), (18, 120)], cl_lens=cl(l18=1), eob=False))
    add("hlit_287", "hlit_too_large", E_DATA, "error", dyn(lit_lens=PLAIN_LIT + [0]))
    add("hlit_288", "hlit_too_large", E_DATA, "error", dyn(lit_lens=PLAIN_LIT + [0, 0]))
    add("hdist_31", "hdist_too_large", E_DATA, "error", dyn(dist_lens=PLAIN_DIST + [0]))
    add("hdist_32", "hdist_too_large", E_DATA, "error", dyn(dist_lens=PLAIN_DIST + [0, 0]))
    add("one_bit_distance_code_the_other_bit", "dist_incomplete", E_DATA, "error",
        _other_bit(toks))
    # ---- fixed blocks -------------------------------------------------------------------------------------------------------------------
    # (what follows each is what the formulas of RFC 1951 section 3.2.5 would ask for were the symbol one more step of its table -- 6 extra
    # bits and a length of 323 / 387, 14 extra bits and a distance of 32 769 / 49 153 -- with history and ISIZE to match: a decoder that lets
    # the symbol pass reaches the CRC, and reports that instead)
    add("fixed_symbol_286", "fixed_symbol_286", E_DATA, "error", Stream().fixed(toks + [("L", 286, 0, 6), ("D", 0, 0)], final=True).getvalue(), text[:300] + bytes(323))
    add("fixed_symbol_287", "fixed_symbol_287", E_DATA, "error", Stream().fixed(toks + [("L", 287, 0, 6), ("D", 0, 0)], final=True).getvalue(), text[:300] + bytes(387))
    deep = _rand(rng, 50000)
    add("fixed_distance_30", "fixed_distance_30", E_DATA, "error", Stream().stored(deep).fixed([("L", 257, 0), ("D", 30, 0, 14)], final=True).getvalue(), deep + bytes(3))
    add("fixed_distance_31", "fixed_distance_31", E_DATA, "error", Stream().stored(deep).fixed([("L", 285, 0), ("D", 31, 0, 14)], final=True).getvalue(), deep + bytes(258))
    # ---- stored blocks ------------------------------------------------------------------------------------------------------------------
    add("len_nlen_mismatch", "len_nlen_mismatch", E_DATA, "error", Stream().fixed(toks).stored(text[300:], final=True, nlen=(300 ^ 0xFFFF) ^ 0x100).getvalue(), text)
    add("stored_length_past_the_input", "stored_past_input", E_DATA, "incomplete", Stream().fixed(toks).stored(text[300:], final=True, length=301).getvalue(), text)
    # ---- output beyond ISIZE: valid deflate, a trailer that states one byte less -----------------------------------------------------------
    for name, kind, s in (("stored_block_past_isize", "stored_past_isize", Stream().fixed(toks).stored(text[300:], final=True)),
                          ("match_past_isize", "match_past_isize", Stream().stored(text[:342]).fixed([(258, 50)], final=True)),
                          ("literal_past_isize", "literal_past_isize", Stream().stored(text[:342]).dynamic(list(text[342:]), PLAIN_LIT, PLAIN_DIST, final=True))):
        full = expand(s.items)
        assert len(full) == 600
        add(name, kind, E_LENGTH, "trailer", s.getvalue(), full[:-1])
    # ---- a distance one byte in front of the member, deep inside it ----------------------------------------------------------------------
    front = _rand(rng, 20000)
    add("distance_o_plus_1_fixed", "distance_in_front_fixed", E_DATA, "error", Stream().stored(front).fixed([1, 2, (258, 20003), 3], final=True).getvalue(), front + bytes(261))
    add("distance_o_plus_1_dynamic", "distance_in_front_dynamic", E_DATA, "error",
        Stream().stored(front).dynamic([1, 2, (258, 20003), 3], PLAIN_LIT, PLAIN_DIST, final=True).getvalue(), front + bytes(261))
    # ---- the input runs out in each field ----------------------------------------------------------------------------------------------
    ll, dl = limited_lens(_skewed(rng, 286, 1.1), 15), limited_lens(_skewed(rng, 30, 1.8), 15)
    s = Stream()
    for b in range(12):
        s.fixed(rng.integers(0, 256, 1 + b % 4).tolist())
        s.stored(_rand(rng, 3 + b))
    s.dynamic(_sweep_tokens(rng, ll, dl, len(expand(s.items))), ll, dl)
    for b in range(12):
        s.fixed(rng.integers(0, 256, 1 + b % 3).tolist() + [(20 + 9 * b, 150 + 40 * b)])
    s.stored(b"the end\n", final=True)
    full = expand(s.items)
    for field in ("block_header", "counts", "cl_lens", "code_length", "code_length_extra", "symbol", "length_extra", "distance_symbol", "distance_extra", "len_nlen"):
        add("input_ends_in_" + field, "truncated_" + field, E_DATA, "incomplete", _cut(s, field), full)
    # ---- the stream's end ------------------------------------------------------------------------------------------------------------------
    add("extra_byte_in_front_of_the_trailer", "extra_byte", E_DATA, "leftover", Stream().fixed(list(text), final=True).getvalue() + b"\0", text)
    add("final_block_never_comes_stored", "no_final_block", E_DATA, "incomplete", Stream().stored(text).getvalue(), text)
    add("final_block_never_comes_fixed", "no_final_block", E_DATA, "incomplete", Stream().fixed(list(text)).getvalue(), text)
    # ---- two defects, where the header has to say which one is reported ---------------------------------------------------------------------
    add("match_past_isize_with_a_distance_in_front", "distance_in_front_fixed", E_DATA, "error", Stream().stored(text[:100]).fixed([(258, 101)], final=True).getvalue(), text[:200])
    add("stored_block_past_isize_and_past_the_input", "stored_past_input", E_DATA, "incomplete", Stream().stored(text[:100]).stored(text[100:200], final=True, length=400).getvalue(), text[:150])
    return out


def _other_bit(toks):
    """a distance set of one 1-bit code, and a match whose distance code is the bit that code does not use"""
    s = Stream()
    s.dynamic(toks + [("L", 257, 0)], PLAIN_LIT, [1], final=True, eob=False)
    s.w.bits(1, 1)
    s.w.code(*canonical(PLAIN_LIT)[256])
    return s.getvalue()


@functools.lru_cache(maxsize=None)
def catalogue():
    """The named cases, valid ones first: a tuple of Case."""
    rng = np.random.Generator(np.random.PCG64([211, ic.SEED]))
    cases = []
    for name, kind, s in _valid_streams(rng):
        text = expand(s.items)
        cases.append(Case(name, ic.member(text, raw=s.getvalue()), text, None, kind, None, s))
    for i, s in enumerate(_grid_members(rng)):
        text = expand(s.items)
        cases.append(Case("match_grid_%02d" % i, ic.member(text, raw=s.getvalue()), text, None, "grid", None, s))
    for name, kind, code, refusal, raw, stated in _invalid_cases(rng):
        cases.append(Case(name, ic.member(stated, raw=raw), None, code, kind, refusal, None))
    assert len({c.name for c in cases}) == len(cases)
    assert all(len(c.text) <= 65536 for c in cases if c.text is not None)
    return tuple(cases)


def valid_cases():
    return [c for c in catalogue() if c.code is None]


def invalid_cases():
    return [c for c in catalogue() if c.code is not None]


def grid_cases():
    return [c for c in catalogue() if c.kind == "grid"]


def raw_stream(case):
    """-> (the raw deflate stream of a Case, the eight trailer bytes its member states): catalogue() wraps every stream with ic.member()'s
    plain BGZF header of 18 bytes"""
    assert case.member[:4] == b"\x1f\x8b\x08\x04" and case.member[10:14] == b"\x06\x00BC"
    return case.member[18:-8], case.member[-8:]


def stored_prefix(data):
    """a NON-final stored block of `data`, as bytes: it ends on a byte boundary, so stored_prefix(data) + raw is the stream `raw` with
    one more block in front, every bit of `raw` where it was within its byte"""
    return Stream().stored(data).getvalue()


def coverage():
    """What the writer emitted in the VALID cases (every symbol of a valid stream is decoded):
       code_lengths       {"lit" / "dist" / "cl": the code lengths of emitted symbols}
       ranks              {"lit" / "dist": {code length: how many different codes of that length were emitted}}
       first / later      block types (0 stored, 1 fixed, 2 dynamic) seen as a member's first block / behind it
       blocks             {case name: blocks in the member}
       grid               the (k, len, dist) combinations, dist as in GRID_DIST
       hlit, hdist, hclen the values dynamic headers stated
       cross              the repeat symbols that ran across the literal / distance boundary
       invalid_kinds      the kinds of the invalid cases"""
    cov = {"code_lengths": {"lit": set(), "dist": set(), "cl": set()}, "first": set(), "later": set(), "blocks": {}, "grid": set(), "hlit": set(), "hdist": set(),
           "hclen": set(), "cross": set(), "invalid_kinds": {c.kind for c in invalid_cases()}}
    ranks = {"lit": set(), "dist": set()}
    for c in valid_cases():
        s = c.stream
        for a in ranks:
            ranks[a] |= s.ranks[a]
        for a in cov["code_lengths"]:
            cov["code_lengths"][a] |= s.used[a]
        cov["first"].add(s.block_types[0])
        cov["later"] |= set(s.block_types[1:])
        cov["blocks"][c.name] = len(s.block_types)
        cov["grid"] |= s.grid
        for hl, hd, hc in s.headers:
            cov["hlit"].add(hl)
            cov["hdist"].add(hd)
            cov["hclen"].add(hc)
        cov["cross"] |= set(s.cross)
    cov["ranks"] = {a: dict(collections.Counter(l for l, _ in r)) for a, r in ranks.items()}
    return cov


def write_corpus(path, members):
    """the file tools/inflate_host_fuzz.cpp --corpus reads: a count, then size-prefixed members, little-endian 32-bit"""
    with open(path, "wb") as f:
        f.write(len(members).to_bytes(4, "little"))
        for m in members:
            f.write(len(m).to_bytes(4, "little"))
            f.write(m)
