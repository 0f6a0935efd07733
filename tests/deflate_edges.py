"""A constructed catalogue of inputs for the device deflate (faqcs_deflate_device / faqcs_deflate_host, csrc/faqcs_deflate.h, DESIGN.md
section 4.9), in the style of tests/trim_edges.py: the edges of the staging, of the two match finders and the pay test, of the parse across
tiles, of the three length-limited codes, of the run-length coded header, of the choice between the three block kinds, of the placement of
the tokens' bits and of a call of many members.  Every case is a named text with its member size, every edge a PREDICATE over what the
model's trace says about a member or over what read_stream() reads out of its deflate stream; coverage() puts every predicate to every case
in both modes.

Model.member(text, mode) is the plain reference: the member's exact bytes and a trace of the decisions behind them, on Python ints, written
from DESIGN.md section 4.9 and RFC 1951.  It shares nothing with the library: the match finders are dictionaries of latest positions, the
parse is a serial walk, the symbols come from the RFC's two tables, the code lengths from a two-queue Huffman construction over explicit
nodes, the three bit counts from the three blocks really built.  zlib is used for the CRC-32 alone.  Restated from the encoder and compared
with csrc/faqcs_deflate.h by tests/test_deflate_edges_model.py: the sizes (TILE, SUB, MAX_TEXT, ...), the two hash multipliers, MATCH_BASE.
tests/test_deflate_edges_model.py holds the host statement to the model without a GPU; tests/test_gpu_deflate_edges.py sends the catalogue
to the device.

    python -m tests.deflate_edges        prints the table: per edge the (case, mode) pairs that claim and reach it
"""
import os
import sys
import zlib
from bisect import bisect_right
from collections import Counter

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

FAST, DENSE = 0, 1
MODES = (FAST, DENSE)
MODE_NAME = {FAST: "fast", DENSE: "dense"}
# restated; tests/test_deflate_edges_model.py compares them with csrc/faqcs_deflate.h
MAX_TEXT, TILE, SUB, HASH_BITS, MIN_MATCH, MAX_MATCH, MAX_DIST, SURE_LENGTH, MATCH_BASE_BITS = 65280, 1024, 256, 12, 3, 258, 32768, 32, 12
HASH3_MUL, HASH8_MUL = 0x9e3779b1, 0x9e3779b97f4a7c15
CONSTANT_SOURCES = {"MAX_TEXT": r"MAX_TEXT = (\d+)", "TILE": r"\bTILE = (\d+)", "SUB": r"\bSUB = (\d+)", "HASH_BITS": r"HASH_BITS = (\d+)", "MIN_MATCH": r"MIN_MATCH = (\d+)",
                    "MAX_MATCH": r"MAX_MATCH = (\d+)", "MAX_DIST": r"MAX_DIST = (\d+)", "SURE_LENGTH": r"SURE_LENGTH = (\d+)", "MATCH_BASE_BITS": r"MATCH_BASE_BITS = (\d+)",
                    "HASH3_MUL": r"hash3\(.*?\* (0x[0-9a-f]+)u\)", "HASH8_MUL": r"hash8\(.*?\* (0x[0-9a-f]+)ull\)"}
STORED, FIXED, DYNAMIC = 0, 1, 2
KIND_NAME = {STORED: "stored", FIXED: "fixed", DYNAMIC: "dynamic"}
GZIP_HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")  # RFC 1952 with the BGZF extra field, in front of BSIZE
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# RFC 1951 section 3.2.5: the first length / distance of every code and its extra bits; 3.2.7: the order of the code-length code's lengths
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


# =====================================================================================================================================
# the model
# =====================================================================================================================================
def length_symbol(length):
    """-> (code 0 .. 28, extra bits, their value)"""
    c = bisect_right(LENGTH_BASE, length) - 1
    return c, LENGTH_EXTRA[c], length - LENGTH_BASE[c]


def distance_symbol(dist):
    c = bisect_right(DIST_BASE, dist) - 1
    return c, DIST_EXTRA[c], dist - DIST_BASE[c]


def log2_eighths(x):
    """8 log2(x) with the mantissa linear between two powers of two: the exponent, then the three bits behind x's leading one"""
    e = x.bit_length() - 1
    return 8 * e + (((x << 3) >> e) & 7)


def literal_costs(text):
    """Eighths of a bit per byte value, from the member's byte histogram: 8 log2(n / count) by log2_eighths, at least one bit"""
    n, cnt = len(text), Counter(text)
    return {b: max(8, log2_eighths(n) - log2_eighths(f)) for b, f in cnt.items()}


def hash3(text, p):
    return ((int.from_bytes(text[p:p + 3], "little") * HASH3_MUL) & 0xffffffff) >> (32 - HASH_BITS)


def hash8(text, p):
    return ((int.from_bytes(text[p:p + 8], "little") * HASH8_MUL) & 0xffffffffffffffff) >> (64 - HASH_BITS)


def common(text, p, c, most):
    """how many bytes at p and at c agree, at most `most`"""
    a, b = text[p:p + most], text[c:c + most]
    if a == b:
        return most
    lo, hi = 0, most  # a[:lo] == b[:lo], a[:hi] != b[:hi]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if a[lo:mid] == b[lo:mid]:
            lo = mid
        else:
            hi = mid
    return lo


def pay(text, cost, p, length, dist):
    """-> (eighths the literals are expected to cost, eighths the match is: 12 bits and its extra bits)"""
    return sum(cost[b] for b in text[p:p + length]), 8 * (MATCH_BASE_BITS + length_symbol(length)[1] + distance_symbol(dist)[1])


def huffman_depths(weights):
    """Minimum-redundancy code lengths of the weights (ascending), by the two-queue method: the two lightest of the unused leaves and the
    unused inner nodes are joined, a leaf before an inner node on a tie.  -> the leaves' depths, deepest first"""
    m = len(weights)
    assert m >= 2 and all(a <= b for a, b in zip(weights, weights[1:]))
    inner, parent, leaf, node = [], {}, 0, 0   # inner: weights in the order made; parent of ("l", i) / ("n", i)
    for _ in range(m - 1):
        pick = []
        for _ in range(2):
            if leaf < m and (node >= len(inner) or weights[leaf] <= inner[node]):
                pick.append(("l", leaf)); leaf += 1
            else:
                pick.append(("n", node)); node += 1
        for x in pick:
            parent[x] = len(inner)
        inner.append(sum(weights[i] if k == "l" else inner[i] for k, i in pick))
    depth_of_inner = [0] * (m - 1)
    for i in range(m - 3, -1, -1):
        depth_of_inner[i] = depth_of_inner[parent[("n", i)]] + 1
    return sorted((depth_of_inner[parent[("l", i)]] + 1 for i in range(m)), reverse=True)


def limited_lengths(weights, limit, two=False):
    """{symbol: length} of a code of at most `limit` bits for {symbol: weight > 0} inside an alphabet that starts at symbol 0, and a trace.
    No symbol: symbol 0 gets one bit.  One: it gets one bit, and with `two` the lowest other symbol does too.  Else the Huffman depths;
    leaves deeper than the limit come up to it, and while the code is over-subscribed one step takes a leaf from the deepest level above
    the limit that has one, makes it an inner node over itself and a leaf taken from the limit's level.  The rarest symbols -- by (weight,
    symbol) -- get the longest codes."""
    order = sorted(weights, key=lambda s: (weights[s], s))
    tr = {"used": len(order), "unlimited": {}, "steps": []}
    if not order:
        return {0: 1}, tr
    if len(order) == 1:
        s = order[0]
        return ({s: 1, (0 if s else 1): 1} if two else {s: 1}), tr
    depths = huffman_depths([weights[s] for s in order])
    tr["unlimited"] = dict(zip(order, depths))
    level = Counter(min(d, limit) for d in depths)
    while sum(k << (limit - l) for l, k in level.items()) > 1 << limit:
        l = max(l for l, k in level.items() if k and l < limit)
        tr["steps"].append(l)
        level[l] -= 1; level[l + 1] += 2; level[limit] -= 1
    out = sorted((l for l, k in level.items() for _ in range(k)), reverse=True)
    return dict(zip(order, out)), tr


def canonical(lengths):
    """{symbol: length} -> {symbol: (code, length)}, RFC 1951 section 3.2.2: by length, then by symbol, counting up"""
    code, out, last = 0, {}, 0
    for l, s in sorted((l, s) for s, l in lengths.items() if l):
        code <<= l - last
        out[s] = (code, l)
        code += 1; last = l
    return out


class Bits:
    """A stream that fills its bytes from bit 0"""

    def __init__(self):
        self.done, self.acc, self.n, self.at = bytearray(), 0, 0, 0

    def put(self, v, nb):
        assert 0 <= v < 1 << nb
        self.acc |= v << self.n
        self.n += nb; self.at += nb
        if self.n >= 4096:
            k = self.n // 8
            self.done += (self.acc & ((1 << 8 * k) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k; self.n -= 8 * k

    def code(self, c):
        """a Huffman code goes out from its most significant bit"""
        v, l = c
        self.put(int(format(v, "0%db" % l)[::-1], 2), l)

    def bytes(self):
        return bytes(self.done) + self.acc.to_bytes((self.n + 7) // 8, "little")


def header_tokens(seq):
    """The run-length coding of the code lengths: [(symbol, extra value)].  Zeros: 18 for 11 .. 138 of them while 11 are left, then 17 for 3 ..
    10, the rest as they are.  Another length: itself, then 16 for 3 .. 6 repeats while 3 are left, the rest as they are."""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138); out.append((18, r - 11)); run -= r
            if run >= 3:
                out.append((17, run - 3)); run = 0
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                r = min(run, 6); out.append((16, r - 3)); run -= r
        out += [(v, 0)] * run
    return out


def block(tokens, lit, dist, head=None):
    """The bits of one final block: head = None for the fixed codes, else (n_lit, n_dist, n_cl, cl lengths, header tokens).  -> (Bits, [(bit
    offset, bit length)] of the tokens)"""
    w = Bits()
    w.put(1, 1); w.put(FIXED if head is None else DYNAMIC, 2)
    if head is not None:
        n_lit, n_dist, n_cl, cl, htok = head
        w.put(n_lit - 257, 5); w.put(n_dist - 1, 5); w.put(n_cl - 4, 4)
        for s in CL_ORDER[:n_cl]:
            w.put(cl.get(s, 0), 3)
        cc = canonical(cl)
        for s, v in htok:
            w.code(cc[s])
            if s in CL_EXTRA:
                w.put(v, CL_EXTRA[s])
    lc, dc, where = canonical(lit), canonical(dist), []
    for t in tokens:
        at = w.at
        if isinstance(t, int):
            w.code(lc[t])
        else:
            (c, e, v), (d, de, dv) = length_symbol(t[0]), distance_symbol(t[1])
            w.code(lc[257 + c]); w.put(v, e); w.code(dc[d]); w.put(dv, de)
        where.append((at, w.at - at))
    w.code(lc[256])
    return w, where


class Model:
    @staticmethod
    def find_fast(text, cost, tr):
        """-> {p: (len, dist)} of the matches kept, tile by tile.  The candidate table is the latest position of an EARLIER tile with p's
        hash3; a tile's positions look up only from the tile's entry on, and all of them enter the table behind the tile."""
        n, table, kept, entry = len(text), {}, {}, 0
        for t0 in range(0, n, TILE):
            tr["entries"].append(entry)
            found = {}
            for p in range(max(t0, entry), min(t0 + TILE, n - MIN_MATCH + 1)):
                most = min(MAX_MATCH, n - p)
                cands = []
                c = table.get(hash3(text, p))
                if c is not None and p - c <= MAX_DIST:
                    cands.append(("hash", p - c, common(text, p, c, most)))
                if p:
                    cands.append(("run", 1, common(text, p, p - 1, most)))
                tr["cands"][p] = cands
                best = None
                for k, d, l in cands:   # the longer; the run candidate, which comes second, on a tie
                    if best is None or l >= best[0]:
                        best = (l, d)
                found[p] = Model.judge(text, cost, tr, p, best)
            entry = Model.walk(text, tr, t0, entry, found, kept)
            for p in range(t0, min(t0 + TILE, n - MIN_MATCH + 1)):
                table[hash3(text, p)] = p
        return kept

    @staticmethod
    def find_dense(text, cost, tr):
        """Sub-tiles of 256: the tables are the latest position of an earlier SUB-TILE with p's hash3 and with p's hash8 (positions with
        eight bytes left); the third candidate is p - 1; the longest wins, the nearest on a tie.  Then, on the tile's lengths as found, a
        match gives way to a longer one at the next position of the tile."""
        n, t3, t8, kept, entry = len(text), {}, {}, {}, 0
        for t0 in range(0, n, TILE):
            tr["entries"].append(entry)
            found = {}
            for s0 in range(t0, min(t0 + TILE, n), SUB):
                for p in range(max(s0, entry), min(s0 + SUB, n - MIN_MATCH + 1)):
                    most = min(MAX_MATCH, n - p)
                    where = [("hash", t3.get(hash3(text, p))), ("hash8", t8.get(hash8(text, p)) if p + 8 <= n else None), ("run", p - 1 if p else None)]
                    cands = [(k, p - c, common(text, p, c, most)) for k, c in where if c is not None and p - c <= MAX_DIST]
                    tr["cands"][p] = cands
                    best = None
                    for k, d, l in cands:
                        if best is None or l > best[0] or (l == best[0] and d < best[1]):
                            best = (l, d)
                    found[p] = Model.judge(text, cost, tr, p, best)
                for p in range(s0, min(s0 + SUB, n)):
                    if p + MIN_MATCH <= n:
                        t3[hash3(text, p)] = p
                    if p + 8 <= n:
                        t8[hash8(text, p)] = p
            lazy = [p for p in found if found[p] and p + 1 < t0 + TILE and found.get(p + 1) and found[p + 1][0] > found[p][0]]
            for p in lazy:
                found[p] = None
                tr["kept"][p] = "lazy"
            entry = Model.walk(text, tr, t0, entry, found, kept)
        return kept

    @staticmethod
    def judge(text, cost, tr, p, best):
        """the best candidate of p -> the match kept, or None; the reason goes into the trace"""
        if best is None or best[0] < MIN_MATCH:
            tr["kept"][p] = "short"
            return None
        if best[0] < SURE_LENGTH:
            lits, price = pay(text, cost, p, *best)
            tr["pay"][p] = (lits, price, best)
            if not lits > price:
                tr["kept"][p] = "pay"
                return None
        tr["kept"][p] = best
        return best

    @staticmethod
    def walk(text, tr, t0, entry, found, kept):
        """The greedy parse of one tile, a serial walk from the tile's entry -> the next tile's entry"""
        p, end = entry, min(t0 + TILE, len(text))
        while p < end:
            m = found.get(p)
            if m:
                kept[p] = m
            tr["starts"].append(p)
            p += m[0] if m else 1
        return p

    @staticmethod
    def member(text, mode=FAST):
        """-> (the BGZF member of text, the trace)"""
        text = bytes(text)
        n = len(text)
        assert 1 <= n <= MAX_TEXT and mode in MODES
        cost = literal_costs(text)
        tr = {"n": n, "mode": mode, "cost": cost, "cands": {}, "kept": {}, "pay": {}, "starts": [], "entries": []}
        kept = (Model.find_fast if mode == FAST else Model.find_dense)(text, cost, tr)
        tokens = [kept[p] if p in kept else text[p] for p in tr["starts"]]
        tr["tokens"] = tokens
        # the three histograms
        lit_count, dist_count = Counter({256: 1}), Counter()
        for t in tokens:
            if isinstance(t, int):
                lit_count[t] += 1
            else:
                lit_count[257 + length_symbol(t[0])[0]] += 1
                dist_count[distance_symbol(t[1])[0]] += 1
        lit, tr["lit_limit"] = limited_lengths(lit_count, 15)
        dist, tr["dist_limit"] = limited_lengths(dist_count, 15)
        n_lit, n_dist = max(257, max(lit) + 1), max(dist) + 1
        seq = [lit.get(s, 0) for s in range(n_lit)] + [dist.get(s, 0) for s in range(n_dist)]
        htok = header_tokens(seq)
        cl_count = Counter(s for s, _ in htok)
        cl, tr["cl_limit"] = limited_lengths(cl_count, 7, two=True)
        n_cl = max(4, max(i for i, s in enumerate(CL_ORDER) if cl.get(s, 0)) + 1)
        tr.update(lit_count=dict(lit_count), dist_count=dict(dist_count), cl_count=dict(cl_count), lit=lit, dist=dist, cl=cl, n_lit=n_lit, n_dist=n_dist, n_cl=n_cl,
                  header_tokens=htok)
        # the three blocks
        dyn, dyn_where = block(tokens, lit, dist, (n_lit, n_dist, n_cl, cl, htok))
        fix, fix_where = block(tokens, dict(enumerate(FIXED_LIT)), dict(enumerate(FIXED_DIST)))
        tr["bits"] = {"dynamic": dyn.at, "fixed": fix.at, "stored": 8 * (n + 5)}
        best, where, kind = (fix, fix_where, FIXED) if fix.at <= dyn.at else (dyn, dyn_where, DYNAMIC)
        if (best.at + 7) // 8 >= n + 5:
            kind, where = STORED, []
            stream = b"\x01" + n.to_bytes(2, "little") + (n ^ 0xffff).to_bytes(2, "little") + text
            tr["stream_bits"] = 8 * (n + 5)
        else:
            stream = best.bytes()
            tr["stream_bits"] = best.at
        tr["kind"], tr["where"] = kind, where
        size = len(GZIP_HEADER) + 2 + len(stream) + 8
        out = GZIP_HEADER + (size - 1).to_bytes(2, "little") + stream + (zlib.crc32(text) & 0xffffffff).to_bytes(4, "little") + n.to_bytes(4, "little")
        tr["size"] = size
        return out, tr

    @staticmethod
    def call(text, member_bytes=0, final=1, mode=FAST, capacity=None):
        """One faqcs_deflate_*_mode call -> {"members": [bytes], "traces": [...], "comp": bytes, "member_offset": [...], "info": {...}}: the text
        cut into members of member_bytes (0: 65 280), the 28-byte EOF member behind them with `final`; with a capacity below the need nothing
        is written and info says what was needed."""
        text = bytes(text)
        mb = member_bytes or MAX_TEXT
        got = [_member(text[k:k + mb], mode) for k in range(0, len(text), mb)]
        members, traces = [m for m, _ in got], [t for _, t in got]
        if final:
            members.append(EOF_MEMBER)
        ends = [0]
        for m in members:
            ends.append(ends[-1] + len(m))
        over = capacity is not None and ends[-1] > capacity
        info = {"n_bytes": ends[-1], "n_members": len(members), "overflow": int(over), "n_stored": sum(t["kind"] == STORED for t in traces), "reserved": 0}
        return {"members": members, "traces": traces, "comp": b"" if over else b"".join(members), "member_offset": None if over else ends, "info": info}


_MEMO = {}


def _member(text, mode):
    """Model.member, once per (text, mode) of a process"""
    key = (text, mode)
    if key not in _MEMO:
        _MEMO[key] = Model.member(text, mode)
    return _MEMO[key]


# =====================================================================================================================================
# the stream reader
# =====================================================================================================================================
def _decoder(lengths):
    """{symbol: length} -> (the longest length, a table by that many next bits of the stream: (symbol, length))"""
    most = max(lengths.values())
    tab = [None] * (1 << most)
    for s, (c, l) in canonical(lengths).items():
        r = int(format(c, "0%db" % l)[::-1], 2)
        for hi in range(1 << (most - l)):
            tab[r | hi << l] = (s, l)
    return most, tab


def read_stream(stream):
    """One raw deflate stream of ONE final block, by a decoder of its own -> {"kind", "n_lit", "n_dist", "n_cl", "header_tokens": [(symbol,
    extra value)], "cl" / "lit" / "dist": {symbol: length}, "tokens": [(token, bit offset, bit length)], "end": the bit behind the
    end-of-block code}; a token is a literal's byte or (length, distance).  A stored block has its text as "text" and no tokens."""
    big = bytes(stream) + bytes(8)
    pos = [0]

    def peek(nb):
        i = pos[0] >> 3
        return (int.from_bytes(big[i:i + 4], "little") >> (pos[0] & 7)) & ((1 << nb) - 1)

    def bits(nb):
        v = peek(nb)
        pos[0] += nb
        return v

    def sym(tab):
        e = tab[1][peek(tab[0])]
        assert e is not None, "no code at bit %d" % pos[0]
        pos[0] += e[1]
        return e[0]

    assert bits(1) == 1, "one final block"
    kind = bits(2)
    out = {"kind": kind, "n_lit": None, "n_dist": None, "n_cl": None, "header_tokens": [], "cl": {}, "lit": {}, "dist": {}, "tokens": []}
    if kind == STORED:
        pos[0] = (pos[0] + 7) & ~7
        n = bits(16)
        assert bits(16) == n ^ 0xffff
        out["text"] = bytes(stream[5:5 + n])
        out["end"] = 8 * (5 + n)
        return out
    assert kind in (FIXED, DYNAMIC)
    if kind == FIXED:
        lit, dist = dict(enumerate(FIXED_LIT)), dict(enumerate(FIXED_DIST))
    else:
        n_lit, n_dist, n_cl = bits(5) + 257, bits(5) + 1, bits(4) + 4
        cl = {s: l for s, l in ((s, bits(3)) for s in CL_ORDER[:n_cl]) if l}
        ct, seq = _decoder(cl), []
        while len(seq) < n_lit + n_dist:
            s = sym(ct)
            v = bits(CL_EXTRA[s]) if s in CL_EXTRA else 0
            out["header_tokens"].append((s, v))
            seq += [s] if s < 16 else [seq[-1]] * (3 + v) if s == 16 else [0] * ((3 if s == 17 else 11) + v)
        assert len(seq) == n_lit + n_dist
        lit = {s: l for s, l in enumerate(seq[:n_lit]) if l}
        dist = {s: l for s, l in enumerate(seq[n_lit:]) if l}
        out.update(n_lit=n_lit, n_dist=n_dist, n_cl=n_cl, cl=cl)
    out["lit"], out["dist"] = lit, dist
    lt, dt = _decoder(lit), _decoder(dist)
    while True:
        at = pos[0]
        s = sym(lt)
        if s == 256:
            break
        if s < 256:
            out["tokens"].append((s, at, pos[0] - at))
            continue
        c = s - 257
        length = LENGTH_BASE[c] + bits(LENGTH_EXTRA[c])
        d = sym(dt)
        out["tokens"].append(((length, DIST_BASE[d] + bits(DIST_EXTRA[d])), at, pos[0] - at))
    out["end"] = pos[0]
    return out


def explain(member, trace, bit):
    """What bit `bit` of a member (counted from the member's first byte) belongs to, by the model's trace of that member"""
    size, kind = trace["size"], trace["kind"]
    if bit < 128:
        return "the gzip header"
    if bit < 144:
        return "BSIZE"
    if bit >= 8 * (size - 8):
        return "the CRC-32" if bit < 8 * (size - 4) else "ISIZE"
    b = bit - 144
    if kind == STORED:
        return "the stored block's header" if b < 40 else "stored byte %d" % ((b - 40) // 8)
    if b < 3:
        return "the block's kind"
    if trace["where"] and b >= trace["where"][0][0]:
        k = bisect_right([w[0] for w in trace["where"]], b) - 1
        at, nb = trace["where"][k]
        if b < at + nb:
            t = trace["tokens"][k]
            return "token %d at text position %d: %s" % (k, trace["starts"][k], "literal %d" % t if isinstance(t, int) else "match of %d at distance %d" % t)
        return "the end-of-block code or the padding behind it"
    if kind == FIXED:
        return "the end-of-block code or the padding behind it"
    b -= 3
    if b < 14:
        return "n_lit" if b < 5 else "n_dist" if b < 10 else "n_cl"
    b -= 14
    if b < 3 * trace["n_cl"]:
        return "the length of code-length symbol %d" % CL_ORDER[b // 3]
    b -= 3 * trace["n_cl"]
    cc = canonical(trace["cl"])
    for k, (s, v) in enumerate(trace["header_tokens"]):
        nb = cc[s][1] + CL_EXTRA.get(s, 0)
        if b < nb:
            return "header token %d: symbol %d, extra value %d" % (k, s, v)
        b -= nb
    return "the end-of-block code or the padding behind it"


def first_difference(case, k, mode, got, info, member_offset):
    """None, or what the first difference between a call's bytes and the model's is"""
    e = case.expected(mode)[k]
    what = "%s call %d (%s)" % (case.name, k, MODE_NAME[mode])
    if info != e["info"]:
        return "%s: info %s, the model's %s" % (what, info, e["info"])
    want = e["comp"]
    if got != want:
        i = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        bit = 8 * i + (((got[i] ^ want[i]) & -(got[i] ^ want[i])).bit_length() - 1 if i < min(len(got), len(want)) else 0)
        ends = e["member_offset"]
        j = max(j for j, x in enumerate(ends[:-1]) if x <= i)
        where = "the EOF member" if j >= len(e["traces"]) else explain(e["members"][j], e["traces"][j], bit - 8 * ends[j])
        return "%s: member %d, first differing bit %d of the member (byte %d of comp): %s" % (what, j, bit - 8 * ends[j], i, where)
    if e["member_offset"] is not None and member_offset is not None and list(member_offset) != e["member_offset"]:
        return "%s: member_offset" % what
    return None


def pay_bound():
    """The pay test over every (length, distance) a match under SURE_LENGTH can have, with the cheapest literals there are (one bit each):
    -> (the longest match that can be refused, the distances at which it can).  Every longer match pays whatever its bytes cost."""
    worst = {}
    for length in range(MIN_MATCH, SURE_LENGTH):
        for c in range(30):
            price = 8 * (MATCH_BASE_BITS + length_symbol(length)[1] + DIST_EXTRA[c])
            if not 8 * length > price:
                worst.setdefault(length, []).append(c)
    longest = max(worst)
    return longest, [DIST_BASE[c] for c in worst[longest]]


# =====================================================================================================================================
# cases
# =====================================================================================================================================
class Member:
    """What a member-level predicate looks at: the member's text, the model's trace of it, and its stream as read_stream() reads it"""

    def __init__(self, text, mode):
        self.text, self.n, self.mode = text, len(text), mode
        self.bytes, self.tr = _member(text, mode)
        self._st = self._matches = None

    @property
    def st(self):
        if self._st is None:
            self._st = read_stream(self.bytes[18:-8])
        return self._st

    def seq(self):
        """the code lengths of a dynamic block as the header codes them: literal-length set, then distance set"""
        s = self.st
        return [s["lit"].get(i, 0) for i in range(s["n_lit"])] + [s["dist"].get(i, 0) for i in range(s["n_dist"])]

    def runs(self):
        """{(is zero, run length)} of the maximal runs of seq()"""
        q, out, i = self.seq(), set(), 0
        while i < len(q):
            j = i
            while j < len(q) and q[j] == q[i]:
                j += 1
            out.add((q[i] == 0, j - i))
            i = j
        return out

    def matches(self):
        if self._matches is None:
            self._matches = [(p, t) for p, t in zip(self.tr["starts"], self.tr["tokens"]) if not isinstance(t, int)]
        return self._matches


_MEMBERS = {}


def member_view(text, mode):
    key = (text, mode)
    if key not in _MEMBERS:
        _MEMBERS[key] = Member(text, mode)
    return _MEMBERS[key]


class DCase:
    """name, calls [(text, member_bytes, final, capacity or None)], the edges it claims.  A claim holds when one of the two modes reaches it."""

    def __init__(self, name, calls, claims):
        self.name, self.claims, self.family = name, tuple(claims), None
        self.calls = [tuple(c) + (None,) * (4 - len(c)) for c in ([calls] if isinstance(calls, tuple) else calls)]
        self.calls = [(bytes(t), mb, f, cap) for t, mb, f, cap in self.calls]
        assert all(0 <= mb <= MAX_TEXT and f in (0, 1) and cap in (None, "need", "need-1") for _, mb, f, cap in self.calls)
        self._views = {}

    def n_bytes(self):
        return sum(len(c[0]) for c in self.calls)

    def view(self, mode):
        if mode not in self._views:
            self._views[mode] = View(self, mode)
        return self._views[mode]

    def expected(self, mode):
        """per call Model.call's dict"""
        return self.view(mode).out


class View:
    """What a case-level predicate looks at: per call the arguments, Model.call's result and the members' views"""

    def __init__(self, case, mode):
        self.case, self.mode = case, mode
        self.out = [Model.call(t, mb, f, mode, self.capacity(t, mb, f, cap)) for t, mb, f, cap in case.calls]
        self.calls = []
        for (t, mb, f, cap), o in zip(case.calls, self.out):
            mb = mb or MAX_TEXT
            self.calls.append({"text": t, "mb": mb, "final": f, "capacity": self.capacity(t, mb, f, cap), "out": o, "members": [member_view(t[k:k + mb], mode) for k in range(0, len(t), mb)]})

    def capacity(self, t, mb, f, cap):
        """a case names a capacity by the need, which is the mode's: "need", "need-1", or None for plenty"""
        return None if cap is None else Model.call(t, mb, f, self.mode)["info"]["n_bytes"] - (1 if cap == "need-1" else 0)

    def members(self):
        seen = set()
        for c in self.calls:
            for m in c["members"]:
                if id(m) not in seen:
                    seen.add(id(m))
                    yield m


MEMBER_EDGES, CASE_EDGES, UNREACHABLE = {}, {}, {}


def medge(name):
    def reg(f):
        MEMBER_EDGES[name] = f
        return f
    return reg


def cedge(name):
    def reg(f):
        CASE_EDGES[name] = f
        return f
    return reg


def unreachable(name, why):
    """An edge no input can reach (the argument is DESIGN.md section 4.9a's): the predicate says what reaching it would look like, and the
    coverage test asserts that nothing does"""
    def reg(f):
        MEMBER_EDGES[name] = f
        UNREACHABLE[name] = why
        return f
    return reg


def dyn(m):
    return m.tr["kind"] == DYNAMIC


def hash_cand(m, p):
    return next(((d, l) for k, d, l in m.tr["cands"].get(p, ()) if k == "hash"), None)


def run_cand(m, p):
    return next(((d, l) for k, d, l in m.tr["cands"].get(p, ()) if k == "run"), None)


def kept(m, p):
    k = m.tr["kept"].get(p)
    return k if isinstance(k, tuple) else None


# ---- stage ------------------------------------------------------------------------------------------------------------------------------
def _small_shapes(v):
    got = {"one": set(), "two": set(), "distinct": set()}
    for c in v.calls:
        if len(c["members"]) == 1 and c["members"][0].n <= 40:
            t = c["text"]
            k = len(set(t))
            if k == 1: got["one"].add(len(t))
            if k == 2: got["two"].add(len(t))
            if k == len(t): got["distinct"].add(len(t))
    return got


cedge("stage:every_n_1..40_of_one_byte_value")(lambda v: _small_shapes(v)["one"] >= set(range(1, 41)))
cedge("stage:every_n_2..40_of_two_byte_values")(lambda v: _small_shapes(v)["two"] >= set(range(2, 41)))
cedge("stage:every_n_1..40_all_distinct")(lambda v: _small_shapes(v)["distinct"] >= set(range(1, 41)))
medge("stage:n=65279")(lambda m: m.n == 65279)
medge("stage:n=65280")(lambda m: m.n == 65280)
for _r in (1, 2, 3):
    cedge("stage:last_member_of_%d" % _r)(lambda v, r=_r: any(len(c["members"]) > 1 and c["members"][-1].n == r for c in v.calls))
medge("stage:one_byte_value_costs_one_bit")(lambda m: m.n > 1 and len(m.tr["cost"]) == 1 and set(m.tr["cost"].values()) == {8})


def _cost_difference(m, want):
    cnt = Counter(m.text)
    return any(log2_eighths(m.n) - log2_eighths(f) == want for f in cnt.values())


medge("stage:cost_difference_of_7_clamped_to_8")(lambda m: m.n <= 4096 and _cost_difference(m, 7))
medge("stage:cost_difference_of_8_at_the_clamp")(lambda m: m.n <= 4096 and _cost_difference(m, 8))
medge("stage:cost_difference_of_9_past_the_clamp")(lambda m: m.n <= 4096 and _cost_difference(m, 9))

# ---- find -------------------------------------------------------------------------------------------------------------------------------
medge("find:match_at_n-3_and_no_look_up_at_n-2")(lambda m: m.n >= 4 and kept(m, m.n - 3) is not None and (m.n - 2) not in m.tr["cands"] and (m.n - 3) in m.tr["starts"])
for _k in (3, 4, 5, 6, 7, 257):
    medge("find:match_to_the_last_byte_of_%d" % _k)(lambda m, k=_k: m.n > k and (kept(m, m.n - k) or (0, 0))[0] == k and (m.n - k) in m.tr["starts"] and (kept(m, m.n - k) or (0, 0))[1] > 1)


def _match_258(m, equal):
    for p, (l, d) in m.matches():
        if l == 258 and d > 1 and p + 258 < m.n and (m.text[p + 258] == m.text[p + 258 - d]) == equal:
            return True
    return False


medge("find:length_258_and_byte_259_equal")(lambda m: _match_258(m, True))
medge("find:length_258_and_byte_259_different")(lambda m: _match_258(m, False))
cedge("find:hash_matches_of_every_length_3..35")(lambda v: {l for m in v.members() for p, (l, d) in m.matches() if d > 1 and hash_cand(m, p) == (d, l)} >= set(range(3, 36)))
cedge("find:fast_hash_matches_of_every_length_3..35")(lambda v: v.mode == FAST and {l for m in v.members() for p, (l, d) in m.matches() if d > 1 and hash_cand(m, p) == (d, l)} >= set(range(3, 36)))


def _own_tile_only(m):
    """fast mode: three bytes that occur earlier in the position's own tile and in no tile in front: no candidate, no match"""
    if m.mode != FAST or m.n > 8192:
        return False
    for p in range(TILE, m.n - 2):
        t0 = p - p % TILE
        if hash_cand(m, p) is None and p in m.tr["cands"] and kept(m, p) is None:
            c = m.text.find(m.text[p:p + 3], t0, p + 2)
            if 0 <= c < p - 1 and m.text.find(m.text[p:p + 3], 0, t0 + 2) < 0 and m.text[p:p + 8] == m.text[c:c + 8]:
                return True
    return False


medge("find:fast_source_in_the_own_tile_only_is_not_seen")(_own_tile_only)
medge("find:fast_source_one_tile_earlier_is_seen")(lambda m: m.mode == FAST and any(d > 1 and (p - d) // TILE == p // TILE - 1 for p, (l, d) in m.matches()))


def _later_of_two(m):
    if m.mode != FAST or m.n > 8192:
        return False
    for p, (l, d) in m.matches():
        c = p - d
        if d > 1 and hash_cand(m, p) == (d, l):
            e = m.text.find(m.text[p:p + 3], c - c % TILE, c + 2)
            if 0 <= e < c:
                return True
    return False


medge("find:fast_the_later_of_two_positions_of_a_tile_is_the_candidate")(_later_of_two)
medge("find:another_trigram_with_the_same_hash_fails")(lambda m: any(k == "hash" and l < 3 and m.text[p:p + 3] != m.text[p - d:p - d + 3] for p, cs in m.tr["cands"].items() for k, d, l in cs))


def _tie(m):
    for p, (l, d) in m.matches():
        h, r = hash_cand(m, p), run_cand(m, p)
        if m.mode == FAST and d == 1 and h and r and h[1] == r[1] == l and h[0] > 1:
            return True
    return False


medge("find:fast_hash_and_run_of_equal_length_code_distance_1")(_tie)
medge("find:hash_candidate_longer_than_the_run")(lambda m: any((hash_cand(m, p) or (0, 0))[1] > (run_cand(m, p) or (0, 0))[1] >= 3 and kept(m, p) == (hash_cand(m, p)[1], hash_cand(m, p)[0]) for p in m.tr["cands"]))
medge("find:run_longer_than_the_hash_candidate")(lambda m: any((run_cand(m, p) or (0, 0))[1] > (hash_cand(m, p) or (0, 0))[1] >= 3 and kept(m, p) == (run_cand(m, p)[1], 1) for p in m.tr["cands"]))
medge("find:position_0_has_no_candidate")(lambda m: m.n >= 3 and m.tr["cands"].get(0) == [] and m.tr["kept"][0] == "short")


def _source_inside_a_match(m):
    starts = set(m.tr["starts"])
    return any(d > 1 and (p - d) not in starts for p, (l, d) in m.matches())


medge("find:source_inside_an_earlier_match")(_source_inside_a_match)
medge("find:distance_32767")(lambda m: any(d == 32767 for p, (l, d) in m.matches()))
medge("find:distance_32768")(lambda m: any(d == 32768 for p, (l, d) in m.matches()))


def _too_far(m):
    """a tile's first position whose 40 bytes lie 32 769 in front of it as well: refused for its distance, no other candidate"""
    for p in range(33 * TILE, m.n - 40, TILE):
        if m.text[p:p + 40] == m.text[p - 32769:p - 32769 + 40] and p in m.tr["cands"] and hash_cand(m, p) is None and kept(m, p) is None:
            return True
    return False


medge("find:distance_32769_is_refused")(_too_far)
medge("find:dense_source_in_the_own_sub_tile_is_not_seen")(lambda m: m.mode == DENSE and m.n <= 4096 and any(
    kept(m, p) is None and not [c for c in m.tr["cands"][p] if c[0] != "run"] and 0 <= m.text.find(m.text[p:p + 8], p - p % SUB, p + 7) < p - 1 and m.text.find(m.text[p:p + 3], 0, p - p % SUB + 2) < 0
    for p in m.tr["cands"] if p % SUB and p + 8 <= m.n))
medge("find:dense_eight_byte_table_names_a_farther_and_longer_source")(lambda m: m.mode == DENSE and any(
    k == "hash8" and l >= 8 and (hash_cand(m, p) or (0, 0))[1] < l and (hash_cand(m, p) or (1 << 20,))[0] < d and kept(m, p) == (l, d) for p, cs in m.tr["cands"].items() for k, d, l in cs))

# ---- pay --------------------------------------------------------------------------------------------------------------------------------
def _pay(m, length, over, de=None, le=None):
    """a candidate of `length` bytes whose literals cost `over` eighths more than the match; refused exactly when over <= 0"""
    for p, (lits, price, (l, d)) in m.tr["pay"].items():
        if l == length and lits - price == over and (de is None or distance_symbol(d)[1] == de) and (le is None or length_symbol(l)[1] == le):
            return True
    return False


for _l in range(3, 28):
    cedge("pay:%d_bytes_refused_at_the_price_and_kept_one_eighth_above" % _l)(lambda v, l=_l: any(_pay(m, l, 0) for m in v.members()) and any(_pay(m, l, 1) for m in v.members()))
for _e, _ls in ((0, range(3, 11)), (1, range(11, 19)), (2, range(19, 28))):
    cedge("pay:a_pair_with_%d_extra_length_bits" % _e)(lambda v, e=_e, ls=_ls: any(any(_pay(m, l, 0, le=e) for m in v.members()) and any(_pay(m, l, 1, le=e) for m in v.members()) for l in ls))
cedge("pay:a_pair_with_13_extra_distance_bits")(lambda v: any(any(_pay(m, l, 0, de=13) for m in v.members()) and any(_pay(m, l, 1, de=13) for m in v.members()) for l in range(3, 28)))
medge("pay:27_bytes_of_one_bit_literals_refused")(lambda m: _pay(m, 27, 0, de=13))
medge("pay:28_bytes_of_one_bit_literals_kept")(lambda m: _pay(m, 28, 8, de=13))

# ---- parse ------------------------------------------------------------------------------------------------------------------------------
def _entry(m, off, by_match=True):
    for k, e in enumerate(m.tr["entries"]):
        if k and e - k * TILE == off:
            last = max(p for p in m.tr["starts"] if p < k * TILE)
            if (kept(m, last) is not None and last in dict(m.matches())) == by_match:
                return True
    return False


medge("parse:a_match_ends_at_the_tile's_end:_entry_0")(lambda m: _entry(m, 0))
medge("parse:a_match_ends_one_beyond_the_tile:_entry_1")(lambda m: _entry(m, 1))
medge("parse:a_258_match_at_1023:_entry_257")(lambda m: _entry(m, 257) and any(p % TILE == TILE - 1 and l == 258 for p, (l, d) in m.matches()))


def _all_literals(m, off):
    starts = set(m.tr["starts"])
    return any(e - k * TILE == off and (k + 1) * TILE <= m.n and all(p in starts for p in range(e, (k + 1) * TILE)) and not any(k * TILE <= p < (k + 1) * TILE for p, _ in m.matches())
               for k, e in enumerate(m.tr["entries"]))


medge("parse:1024_literals_from_entry_0")(lambda m: _all_literals(m, 0))
medge("parse:1023_literals_from_entry_1")(lambda m: _all_literals(m, 1))
medge("parse:a_match_inside_another_match_is_not_taken")(lambda m: any(kept(m, p) and p not in set(m.tr["starts"]) for p in list(m.tr["kept"])[:20000]) if m.n <= 20000 else False)
medge("parse:a_last_tile_of_one_position")(lambda m: m.n > TILE and m.n % TILE == 1)
medge("parse:n_a_multiple_of_1024")(lambda m: m.n % TILE == 0)
medge("parse:dense_lazy_gives_way")(lambda m: any(k == "lazy" for k in m.tr["kept"].values()))
medge("parse:dense_lazy_chain_of_two")(lambda m: any(k == "lazy" and m.tr["kept"].get(p + 1) == "lazy" for p, k in m.tr["kept"].items()))
medge("parse:dense_lazy_not_across_tiles")(lambda m: m.mode == DENSE and any(  # (position 1 024 lies in front of its tile's entry and is not looked up: the longer match is the text's)
    p % TILE == TILE - 1 and kept(m, p) and p in m.tr["starts"] and 0 <= m.text.find(m.text[p + 1:p + 2 + kept(m, p)[0]], 0, p) < p - SUB for p in m.tr["kept"]))
medge("parse:dense_lazy_equal_lengths_do_not_fire")(lambda m: m.mode == DENSE and any(kept(m, p) and kept(m, p + 1) and kept(m, p + 1)[0] == kept(m, p)[0] and p in m.tr["starts"] for p in m.tr["kept"]))

# ---- codes ------------------------------------------------------------------------------------------------------------------------------
medge("codes:no_match:_one_distance_code_of_one_bit")(lambda m: dyn(m) and not m.matches() and m.st["n_dist"] == 1 and m.st["dist"] == {0: 1})
medge("codes:one_distance_code_used")(lambda m: dyn(m) and len(m.tr["dist_count"]) == 1 and list(m.st["dist"].values()) == [1])
medge("codes:two_distance_codes_used")(lambda m: dyn(m) and len(m.tr["dist_count"]) == 2 and sorted(m.st["dist"].values()) == [1, 1])
medge("codes:n_lit_257")(lambda m: dyn(m) and m.st["n_lit"] == 257)
medge("codes:n_lit_286")(lambda m: dyn(m) and m.st["n_lit"] == 286)
medge("codes:n_dist_30")(lambda m: dyn(m) and m.st["n_dist"] == 30)


def _limit(m, which, limit):
    """the dynamic block is chosen, the unlimited lengths pass the limit, the over-subscription takes several steps and one of them finds no
    leaf on the level above the last"""
    t = m.tr[which + "_limit"]
    return dyn(m) and t["unlimited"] and max(t["unlimited"].values()) > limit and len(t["steps"]) >= 2 and min(t["steps"]) < limit - 1 and max(m.st[which].values()) == limit


medge("codes:literal_lengths_pass_15")(lambda m: _limit(m, "lit", 15))
medge("codes:distance_lengths_pass_15")(lambda m: _limit(m, "dist", 15))
medge("codes:code_length_lengths_pass_7")(lambda m: _limit(m, "cl", 7))
medge("codes:equal_weights_ordered_by_symbol")(lambda m: dyn(m) and any(
    m.tr["lit_count"][s] == m.tr["lit_count"][t] and m.st["lit"][s] > m.st["lit"][t] for s in m.tr["lit_count"] for t in m.tr["lit_count"] if s < t))
medge("codes:code_length_code_of_two_symbols")(lambda m: dyn(m) and len(m.tr["cl_count"]) == 2)
unreachable("codes:code_length_code_of_one_symbol", "the end-of-block code has a length v >= 1, coded as symbol v; with a symbol unused its zero is coded too, and 257 or more used symbols cannot "
            "all have one length")(lambda m: m.tr["kind"] != STORED and len(m.tr["cl_count"]) == 1)

# ---- header -----------------------------------------------------------------------------------------------------------------------------
for _r in (1, 2, 3, 10, 11, 138, 139, 149):
    medge("header:zero_run_of_%d" % _r)(lambda m, r=_r: dyn(m) and (True, r) in m.runs())
for _r in (1, 2, 3, 4, 7, 8, 10, 11):
    medge("header:nonzero_run_of_%d" % _r)(lambda m, r=_r: dyn(m) and (False, r) in m.runs())
for _s in (16, 17, 18):
    medge("header:symbol_%d_with_its_least_and_its_greatest_value" % _s)(lambda m, s=_s: dyn(m) and {(s, 0), (s, (1 << CL_EXTRA[s]) - 1)} <= set(m.st["header_tokens"]))
medge("header:a_run_from_the_last_literal-length_length_into_the_distance_lengths")(lambda m: dyn(m) and m.seq()[m.st["n_lit"] - 1] == m.seq()[m.st["n_lit"]] != 0)
medge("header:n_cl_19_with_a_15_bit_code")(lambda m: dyn(m) and m.st["n_cl"] == 19 and 15 in list(m.st["lit"].values()) + list(m.st["dist"].values()))
medge("header:n_cl_12_the_smallest")(lambda m: dyn(m) and m.st["n_cl"] == 12)
unreachable("header:n_cl_below_12", "a distance set of fewer than 2 codes has a 1-bit code (n_cl 18), and a complete code over at most 30 symbols needs a length of 4 or less (n_cl >= 12): "
            "lengths 5 .. 11 alone sum to 30 / 32 at the most")(lambda m: dyn(m) and m.st["n_cl"] < 12)

# ---- choose -----------------------------------------------------------------------------------------------------------------------------
medge("choose:fixed_equals_dynamic:_fixed")(lambda m: m.tr["bits"]["fixed"] == m.tr["bits"]["dynamic"] and m.st["kind"] == FIXED)
medge("choose:fixed_one_above_dynamic:_dynamic")(lambda m: m.tr["bits"]["fixed"] == m.tr["bits"]["dynamic"] + 1 and m.st["kind"] == DYNAMIC)
medge("choose:bytes_equal_n+5:_stored")(lambda m: (min(m.tr["bits"]["fixed"], m.tr["bits"]["dynamic"]) + 7) // 8 == m.n + 5 and m.st["kind"] == STORED)
medge("choose:bytes_equal_n+4:_not_stored")(lambda m: (min(m.tr["bits"]["fixed"], m.tr["bits"]["dynamic"]) + 7) // 8 == m.n + 4 and m.st["kind"] != STORED)
medge("choose:a_member_of_n+31_bytes")(lambda m: len(m.bytes) == m.n + 31)
medge("choose:a_full_member_of_65311_bytes")(lambda m: len(m.bytes) == MAX_TEXT + 31)
cedge("choose:all_three_kinds_in_one_call")(lambda v: any({m.tr["kind"] for m in c["members"]} == {STORED, FIXED, DYNAMIC} for c in v.calls))

# ---- place ------------------------------------------------------------------------------------------------------------------------------
LONGEST_TOKEN = 44   # bits: the longest token of the catalogue (48 is the format's limit)


def _longest(m):
    return max([nb for _, _, nb in m.st["tokens"]] or [0]) if m.tr["kind"] != STORED else 0


medge("place:a_token_of_more_than_32_bits")(lambda m: _longest(m) > 32)
medge("place:the_longest_token_found")(lambda m: _longest(m) == LONGEST_TOKEN)
cedge("place:token_starts_at_every_bit_offset_mod_32")(lambda v: any(m.tr["kind"] != STORED and {(144 + at) % 32 for _, at, _ in m.st["tokens"]} == set(range(32)) for m in v.members()))


def _upper_part(m):
    if m.tr["kind"] == STORED:
        return False
    big = int.from_bytes(m.bytes[:4096], "little")
    for t, at, nb in m.st["tokens"]:
        o = 144 + at
        if o + nb > 8 * 4096:
            break
        if o % 32 + nb > 32 and (big >> o & ((1 << nb) - 1)) >> (32 - o % 32):
            return True
    return False


medge("place:a_token_across_a_word_boundary_with_bits_in_the_upper_word")(_upper_part)
for _r in (0, 1, 7):
    medge("place:stream_bits_mod_8_is_%d" % _r)(lambda m, r=_r: m.tr["kind"] != STORED and m.tr["stream_bits"] % 8 == r)
cedge("place:member_sizes_of_every_residue_mod_16")(lambda v: {len(m.bytes) % 16 for m in v.members()} == set(range(16)))

# ---- call -------------------------------------------------------------------------------------------------------------------------------
def _pairs(c):
    o = c["out"]["member_offset"]
    return {(a % 16, (b - a) % 16) for a, b in zip(o[:-1], o[1:])} if o else set()


cedge("call:all_256_pairs_of_start_and_size_mod_16")(lambda v: any(len(_pairs(c)) == 256 for c in v.calls))
for _k in (255, 256, 257):
    cedge("call:%d_members" % _k)(lambda v, k=_k: any(c["out"]["info"]["n_members"] == k for c in v.calls))
cedge("call:513_members_of_4096_of_three_kinds_of_text")(lambda v: any(
    c["mb"] == 4096 and len(c["members"]) >= 2 * 256 + 1 and all(c["members"][k].tr["kind"] != c["members"][k + 1].tr["kind"] or bool(c["members"][k].matches()) != bool(c["members"][k + 1].matches())
                                                                  for k in range(len(c["members"]) - 1))
    and {m.tr["kind"] for m in c["members"]} >= {STORED, DYNAMIC} and any(m.tr["kind"] == DYNAMIC and not m.matches() for m in c["members"]) for c in v.calls))
cedge("call:stored_members_among_others")(lambda v: any(0 < c["out"]["info"]["n_stored"] < len(c["members"]) for c in v.calls))
cedge("call:capacity_one_below_the_need")(lambda v: any(c["capacity"] == c["out"]["info"]["n_bytes"] - 1 and c["out"]["info"]["overflow"] == 1 for c in v.calls))
cedge("call:capacity_exactly_the_need")(lambda v: any(c["capacity"] == c["out"]["info"]["n_bytes"] and c["out"]["info"]["overflow"] == 0 for c in v.calls))


# =====================================================================================================================================
# the cases
# =====================================================================================================================================
def _rng(*key):
    return np.random.Generator(np.random.PCG64([20261020] + [int(k) for k in key]))


def _filler(rng, n):
    """n bytes of 24 letters in which no three bytes occur twice: no match but what a case places"""
    import deflate_cases as dc

    return bytearray(dc.no_repeated_trigram(rng, n, 97, 121))


def _unique(rng, n, lo=130, hi=250):
    import deflate_cases as dc

    return dc.no_repeated_trigram(rng, n, lo, hi)


def _illumina(n, seed):
    import deflate_cases as dc

    return dc.illumina_text(n, seed=seed)


def stage_cases():
    C = []
    calls = []
    for n in range(1, 41):
        calls += [(b"G" * n, 0, n & 1), (bytes(range(60, 60 + n)), 0, 1)]
        if n >= 2:
            calls.append(((b"AC" * n)[:n], 0, 0))
    C.append(DCase("stage_1_to_40", calls, ["stage:every_n_1..40_of_one_byte_value", "stage:every_n_2..40_of_two_byte_values", "stage:every_n_1..40_all_distinct",
                                           "stage:one_byte_value_costs_one_bit", "codes:code_length_code_of_two_symbols"]))
    C.append(DCase("stage_65279_one_value", (b"Q" * 65279, 0, 1), ["stage:n=65279", "header:a_run_from_the_last_literal-length_length_into_the_distance_lengths",
                                                                   "find:fast_hash_and_run_of_equal_length_code_distance_1"]))
    t = _illumina(3 * 64 + 3, 21)
    C.append(DCase("stage_last_members", [(t[:3 * 64 + r], 64, 1) for r in (1, 2, 3)], ["stage:last_member_of_1", "stage:last_member_of_2", "stage:last_member_of_3"]))
    calls = []
    for want in (7, 8, 9):
        n, f = next((n, f) for n in range(16, 200) for f in range(1, n) if log2_eighths(n) - log2_eighths(f) == want)
        calls.append((bytes(_rng(31, want).permutation(np.frombuffer(b"T" * f + b"C" * (n - f), np.uint8))), 0, 1))
    C.append(DCase("stage_clamp", calls, ["stage:cost_difference_of_7_clamped_to_8", "stage:cost_difference_of_8_at_the_clamp", "stage:cost_difference_of_9_past_the_clamp"]))
    return C


def _colliding_trigrams(rng):
    seen = {}
    while True:
        t = bytes(int(v) for v in rng.integers(130, 250, 3))
        if len(set(t)) == 3:
            h = hash3(t, 0)
            if h in seen and not set(seen[h]) & set(t):
                return seen[h], t
            seen[h] = t


def find_cases():
    import deflate_cases as dc
    import deflate_dense_cases as dd

    C = []
    for k in (3, 4, 5, 6, 7, 257):
        rng = _rng(41, k)
        n = 1400 + k
        t = _filler(rng, n)
        s = _unique(rng, k) if k > 100 else bytes(int(v) for v in rng.permutation(np.arange(130, 250))[:k])
        t[100:100 + k] = s
        t[n - k:] = s
        C.append(DCase("find_to_the_last_byte_%d" % k, (t, 0, 1), ["find:match_to_the_last_byte_of_%d" % k] + (["find:match_at_n-3_and_no_look_up_at_n-2"] if k == 3 else [])))
    rng = _rng(42)
    t = _filler(rng, 1700)
    s = _unique(rng, 520)
    t[50:308], t[308] = s[:258], 251
    t[350:608], t[608] = s[260:518], 252
    t[1030:1288], t[1288] = s[:258], 251
    t[1330:1588], t[1588] = s[260:518], 253
    C.append(DCase("find_258", (t, 0, 1), ["find:length_258_and_byte_259_equal", "find:length_258_and_byte_259_different", "header:symbol_16_with_its_least_and_its_greatest_value"]))
    calls = []
    for L in range(3, 36):               # one text per length: the source ends with tile 0, so next to nothing enters the table behind it
        for seed in range(16):           # (the first seed at which no other trigram has taken the source's place in the 12-bit table: 0 for all but one length)
            rng = _rng(43, L, seed)
            t = _filler(rng, 1100 + L)
            src = _unique(rng, L)
            t[1022 - L:1022], t[1022] = src, 251
            t[1040:1040 + L], t[1040 + L] = src, 252
            tr = _member(bytes(t), FAST)[1]
            if tr["kept"].get(1040) == (L, 18 + L) and 1040 in tr["starts"] and hash_cand(member_view(bytes(t), FAST), 1040) == (18 + L, L):
                break
        calls.append((t, 0, L & 1))
    C.append(DCase("find_lengths_3_to_35", calls, ["find:hash_matches_of_every_length_3..35", "find:fast_hash_matches_of_every_length_3..35", "find:fast_source_one_tile_earlier_is_seen"]))
    x = dd._Text(_rng(44), 2300)
    own, near, two = x.rare(12), x.rare(12), x.rare(3)
    x.place(1100, own); x.place(1300, own)
    x.place(900, near); x.place(1500, near)
    x.place(100, two + x.rare(3)); tail = x.rare(4); x.place(300, two + tail); x.place(1700, two + tail)
    C.append(DCase("find_tiles", (x.bytes(), 0, 1), ["find:fast_source_in_the_own_tile_only_is_not_seen", "find:fast_source_one_tile_earlier_is_seen",
                                                     "find:fast_the_later_of_two_positions_of_a_tile_is_the_candidate", "header:symbol_17_with_its_least_and_its_greatest_value"]))
    rng = _rng(45)
    t1, t2 = _colliding_trigrams(rng)
    t = _filler(rng, 1300)
    t[100:103], t[1100:1103] = t1, t2
    C.append(DCase("find_collision", (t, 0, 1), ["find:another_trigram_with_the_same_hash_fails"]))
    x = dd._Text(_rng(46), 2400)
    a, b, tail = x.rare(1), x.rare(1), x.rare(3)
    x.place(100, a * 4 + tail); x.place(1100, a * 4 + tail)      # at 1101 the hash candidate (101) gives 6, the run 3
    x.place(300, b * 4); x.place(1300, b * 10)                  # at 1301 the hash candidate gives 3, the run 9
    t = bytearray(x.bytes())
    t[1900:2300] = b"q" * 400                                    # at 2048 the latest qqq of the tiles in front is 2045: 258 either way
    C.append(DCase("find_run_and_hash", (t, 0, 1), ["find:hash_candidate_longer_than_the_run", "find:run_longer_than_the_hash_candidate",
                                                    "find:fast_hash_and_run_of_equal_length_code_distance_1", "find:position_0_has_no_candidate"]))
    x = dd._Text(_rng(47), 2300)
    s = x.rare(10)
    x.place(100, s); x.place(1100, s); x.place(2100, s[4:])
    C.append(DCase("find_source_inside_a_match", (x.bytes(), 0, 1), ["find:source_inside_an_earlier_match"]))
    C.append(DCase("find_far", (dc.far_repeat(_rng(48), (32768, 32769, 32767)), 0, 1), ["find:distance_32767", "find:distance_32768", "find:distance_32769_is_refused",
                                                                                      "stage:n=65280", "codes:n_dist_30"]))
    claims = {"own_sub_tile": ["find:dense_source_in_the_own_sub_tile_is_not_seen"], "eight_bytes_9": ["find:dense_eight_byte_table_names_a_farther_and_longer_source"]}
    for name, (text, want) in dd.dense_edge_texts().items():
        if not name.startswith("lazy"):
            C.append(DCase("find_dense_" + name, (text, 0, 1), claims.get(name, [])))
    return C


# ---- pay: the source at 20, G1 A B A A .. A G2, its copy P bytes on behind another guard; every other byte is a run of A, of B or of a third letter,
# so that "ABA" stands at the source and at the copy alone, and the counts of A and B are whatever the price asks for
def _pay_counts(L, de, over):
    """-> (n, count of A, count of B, distance) with (L - 1) cost(A) + cost(B) == the match's price + over"""
    le = length_symbol(L)[1]
    price = 8 * (MATCH_BASE_BITS + le + de)
    dist = DIST_BASE[2 * de + 2] + 40
    for n in range(dist + 2 * L + 200, dist + 2 * L + 4000, 7):
        by_cost = {}
        for f in range(2 * L, n):
            by_cost.setdefault(max(8, log2_eighths(n) - log2_eighths(f)), f)     # the smallest count with that cost
        for ca in sorted(by_cost):
            cb = price + over - (L - 1) * ca
            if cb in by_cost and by_cost[ca] + by_cost[cb] + 60 <= n and by_cost[ca] >= 2 * L + 8 and by_cost[cb] >= 10:
                return n, by_cost[ca], by_cost[cb], dist
    raise AssertionError("no counts for %d %d %d" % (L, de, over))


def _pay_text(L, de, over):
    n, fa, fb, dist = _pay_counts(L, de, over)
    S = b"ABA" + b"A" * (L - 3)
    src, cpy = b"\x01" + S + b"\x02", b"\x03" + S + b"\x04"
    fa -= 2 * (L - 1); fb -= 2
    t = bytearray(b"\x05" * 19 + src)
    mid = dist - L - 2                   # between the source's last guard and the copy's first: the copy's A B A stands `dist` behind the source's
    letters = bytes([65]) * fa + bytes([66]) * fb
    gap, rest = letters[:mid], letters[mid:]
    t += gap + b"\x06" * (mid - len(gap)) + cpy + rest[::-1]
    assert len(t) <= n, (L, de, over, len(t), n)
    t += b"\x07" * (n - len(t))
    assert len(t) == n and t.count(65) == fa + 2 * (L - 1) and t.count(66) == fb + 2 and t.find(b"ABA", 21) == 20 + dist
    return bytes(t)


def pay_cases():
    C = []
    for lo, hi, de in ((3, 24, 9), (24, 28, 13)):
        calls, claims = [], []
        for L in range(lo, hi):
            calls += [(_pay_text(L, de, 0), 0, 1), (_pay_text(L, de, 1), 0, 0)]
            claims.append("pay:%d_bytes_refused_at_the_price_and_kept_one_eighth_above" % L)
        if de == 9:
            claims += ["pay:a_pair_with_%d_extra_length_bits" % e for e in (0, 1, 2)]
        else:
            calls.append((_pay_text(28, 13, 8), 0, 1))
            claims += ["pay:a_pair_with_13_extra_distance_bits", "pay:27_bytes_of_one_bit_literals_refused", "pay:28_bytes_of_one_bit_literals_kept"]
        C.append(DCase("pay_pairs_de_%d" % de, calls, claims))
    return C


def parse_cases():
    import deflate_dense_cases as dd

    C = []
    rng = _rng(61)
    t = _filler(rng, 5500)
    t[1000:1024] = b"\x81" * 24          # the match ends where tile 0 ends; tile 1 is 1 024 literals
    t[3050:3073] = b"\x82" * 23          # one beyond tile 2's end; tile 3 is 1 023 literals behind an entry of 1
    t[5118:5377] = b"\x83" * 259         # a literal at 5 118, 258 bytes from 5 119, the last position of tile 4
    C.append(DCase("parse_tile_ends", (t, 0, 1), ["parse:a_match_ends_at_the_tile's_end:_entry_0", "parse:a_match_ends_one_beyond_the_tile:_entry_1", "parse:a_258_match_at_1023:_entry_257",
                                                  "parse:1024_literals_from_entry_0", "parse:1023_literals_from_entry_1", "parse:a_match_inside_another_match_is_not_taken", "codes:n_lit_286"]))
    C.append(DCase("parse_last_tile_of_one", (_filler(_rng(62), 2049), 0, 1), ["parse:a_last_tile_of_one_position"]))
    C.append(DCase("parse_two_whole_tiles", (_filler(_rng(63), 2048), 0, 0), ["parse:n_a_multiple_of_1024"]))
    claims = {"lazy_pair": [], "lazy_chain": ["parse:dense_lazy_gives_way", "parse:dense_lazy_chain_of_two"], "lazy_pair_across_tiles": ["parse:dense_lazy_not_across_tiles"],
              "lazy_equal": ["parse:dense_lazy_equal_lengths_do_not_fire"]}
    for name, (text, want) in dd.dense_edge_texts().items():
        if name.startswith("lazy"):
            C.append(DCase("parse_dense_" + name, (text, 0, 1), claims[name]))
    return C


def _chain_counts(k=18, first=(1, 5), slack=3):
    """k counts, each the sum of the two in front of it and `slack` more: Fibonacci numbers with room for the few symbols a text adds on its own (the
    end-of-block code, the length codes of chance matches), so that the Huffman tree stays one chain"""
    c = list(first)
    while len(c) < k:
        c.append(c[-1] + c[-2] + slack)
    return c


FIB = tuple(_chain_counts())


def _fibonacci_literals(rng):
    """Byte values whose counts are _chain_counts() (and the end-of-block code's 1 under them): a chain of 19 symbols, deeper than 15.  The bytes are
    shuffled."""
    raw = np.concatenate([np.full(f, 40 + 3 * k, np.uint8) for k, f in enumerate(FIB)])
    return rng.permutation(raw).tobytes()


CHAIN_ROW, CHAIN_ROWS, CHAIN_CELL = 86, 126, 6
CHAIN_HEAVY = ((2, 2584), (3, 1597), (4, 987), (6, 610), (8, 377), (12, 233), (16, 144), (24, 89))     # (rows between two occurrences, matches): codes 20 .. 27
CHAIN_NEAR = ((19, 55), (18, 34), (17, 21), (16, 13), (14, 8), (13, 5), (12, 3), (11, 2))              # (distance code, matches), copies near a tile's start
CHAIN_COUNTS = {20: 2584, 21: 1597, 22: 987, 23: 610, 24: 377, 25: 233, 26: 144, 27: 89, 19: 55, 18: 34, 17: 21, 16: 13, 14: 8, 13: 5, 12: 3, 11: 2, 28: 1, 29: 1}


def _distance_chain_text():
    """65 016 bytes in which every byte is placed: 126 rows of 86 cells of six bytes, a cell a four-byte word and two guard bytes.  A column of the
    heavy kind holds m words in turn, so a word comes back every m rows, 516 m bytes -- always in an earlier tile --; the light counts are pairs of
    cells, the copy so near its tile's start that the source lies in the tile in front.  The first three bytes of every repeated word hash to a
    slot of the 12-bit table that no other trigram of the member hashes to, so no source is ever overwritten; every other trigram at which a token can
    start occurs once in the member, so there is no chance match; no byte equals the one in front of it, so there is no run.  The distance codes
    then occur exactly CHAIN_COUNTS times: Fibonacci numbers, a chain of 18.  The one match of code 29 is 148 bytes long, 24 768 back."""
    import random

    rnd = random.Random(76)
    K, ROWS = CHAIN_ROW, CHAIN_ROWS
    reserved, others, seen = set(), set(), set()      # slots of first trigrams; hashes of every other trigram; the other trigrams themselves

    def word(n, repeated):
        while True:
            w = bytes(rnd.randrange(256) for _ in range(n))
            tri = [w[i:i + 3] for i in range(n - 2)]
            hs = [hash3(t, 0) for t in tri]
            rest = tri[1:] if repeated else tri
            if any(a == b for a, b in zip(w, w[1:])) or len(set(tri)) < len(tri) or any(t in seen for t in tri) or any(h in reserved for h in hs):
                continue
            if repeated and hs[0] in others:
                continue
            if repeated:
                reserved.add(hs[0])
                seen.add(tri[0])
            for t in rest:
                seen.add(t)
                others.add(hash3(t, 0))
            return w

    def long_word(n):
        """a repeated word of n bytes, grown byte by byte under the same rules"""
        w = bytearray(word(3, True))
        while len(w) < n:
            b = rnd.randrange(256)
            t = bytes(w[-2:]) + bytes([b])
            if b != w[-1] and t not in seen and hash3(t, 0) not in reserved:
                seen.add(t)
                others.add(hash3(t, 0))
                w.append(b)
        return bytes(w)

    cells = [None] * (K * ROWS)              # the content of every cell; a long word takes several
    col = 0
    for m, quota in CHAIN_HEAVY:
        while quota:
            q = min(quota, ROWS - m)
            ws = [word(4, True) for _ in range(m)]
            for r in range(m + q):
                cells[r * K + col] = ws[r % m]
            quota -= q
            col += 1
    first_free = col
    free = lambda c: cells[c] is None and c % K >= first_free
    # one match of code 28 and the long one of code 29, in the free columns
    a, b = 3 * K + first_free, (3 + 33) * K + first_free               # 33 rows: 17 028 bytes
    assert free(a) and free(b)
    cells[a] = cells[b] = word(4, True)
    long_cells = (148 + 2) // CHAIN_CELL
    assert K - first_free - 1 >= long_cells
    w = long_word(148)
    for r in (5, 5 + 48):                                                # 48 rows: 24 768 bytes
        c0 = r * K + first_free + 1
        assert all(free(c) for c in range(c0, c0 + long_cells))
        cells[c0] = w
        for c in range(c0 + 1, c0 + long_cells):
            cells[c] = b""
    for code, count in CHAIN_NEAR:
        lo, hi = DIST_BASE[code], DIST_BASE[code + 1] - 1
        c = 0
        while count:
            c += 1
            assert c < K * ROWS, code
            if not free(c):
                continue
            p = CHAIN_CELL * c
            for d in range((lo + 5) // 6 * 6, hi + 1, 6):
                s = c - d // 6
                if s >= 0 and free(s) and (p - d) // TILE < p // TILE:
                    cells[s] = cells[c] = word(4, True)
                    count -= 1
                    break
    for c in range(K * ROWS):
        if cells[c] is None:
            cells[c] = word(4, False)
    # the guards, each pair chosen with the two bytes behind it in view
    t = bytearray()
    order = [w for w in cells if w != b""]
    for k, w in enumerate(order):
        t += w
        nxt = order[k + 1][:2] if k + 1 < len(order) else b""
        while True:
            g = bytes((rnd.randrange(256), rnd.randrange(256)))
            s = bytes(t[-2:]) + g + nxt
            tri = [s[i:i + 3] for i in range(len(s) - 2)]
            if any(x == y for x, y in zip(s, s[1:])) or len(set(tri)) < len(tri) or any(x in seen for x in tri) or any(hash3(x, 0) in reserved for x in tri):
                continue
            seen.update(tri)
            t += g
            break
    assert len(t) == K * ROWS * CHAIN_CELL
    return bytes(t)


def _cl_limit_text():
    """A literal-length code given by its lengths: a complete code of 60 .. 180 symbols of 2 .. 10 bits, made by splitting random codes, laid over random
    byte values; a byte with a code of l bits occurs 2^(10 - l) times and the end-of-block code has 10 bits, so Huffman gives exactly these lengths, and the
    1 023 bytes are one tile.  The first such code (seeded) whose header -- the counts of the code-length symbols -- is deeper than 7 bits, needs several
    limit steps and one of them from above level 6."""
    import random

    rnd = random.Random(7)
    while True:
        lens, target = [1, 1], rnd.randint(60, 180)
        while len(lens) < target:
            i = rnd.randrange(len(lens))
            if lens[i] < 10 and (rnd.random() < 0.5 or lens[i] < 4):
                lens[i] += 1
                lens.append(lens[i])
        if 1 in lens or max(lens) != 10:
            continue
        lens.remove(10)                  # the end-of-block code
        vals = sorted(rnd.sample(range(256), len(lens)))
        rnd.shuffle(lens)
        lit = dict(zip(vals, lens))
        tr = limited_lengths(Counter(s for s, _ in header_tokens([lit.get(s, 0) for s in range(256)] + [10, 1])), 7, two=True)[1]
        if tr["unlimited"] and max(tr["unlimited"].values()) > 7 and len(tr["steps"]) >= 2 and min(tr["steps"]) < 6:
            raw = np.concatenate([np.full(1 << (10 - l), v, np.uint8) for v, l in lit.items()])
            return _rng(75, 0).permutation(raw).tobytes()


def _n_cl_12_text():
    """18 tiles of random bytes of 64 values (six bits each, so no literal-length code is longer than 11 bits) with eight bytes at the start of tiles 2 ..
    17 copied from 9, 13, 17, ... 1 537 bytes in front: 16 distance codes once each, four bits each, and no length under 4 or over 11 anywhere"""
    rng = _rng(83, 0)
    t = bytearray((32 + rng.integers(0, 64, 18 * 1024 + 100)).astype(np.uint8).tobytes())
    for k, c in enumerate(range(6, 22)):
        T, d = 1024 * (k + 2), DIST_BASE[c]
        t[T:T + 8] = t[T - d:T - d + 8]
    return bytes(t)


def codes_cases():
    import deflate_cases as dc

    C = []
    rng = _rng(71)
    C.append(DCase("codes_no_match", (_filler(rng, 3000), 0, 1), ["codes:no_match:_one_distance_code_of_one_bit", "codes:n_lit_257", "place:token_starts_at_every_bit_offset_mod_32"]))
    C.append(DCase("codes_one_distance", (dc.single_distance(rng), 0, 1), ["codes:one_distance_code_used"]))
    t = bytearray(dc.single_distance(rng))
    t[3000:3040] = b"\xfd" * 40
    C.append(DCase("codes_two_distances", (t, 0, 1), ["codes:two_distance_codes_used"]))
    C.append(DCase("codes_equal_weights", (bytes(range(64)) * 4, 0, 1), ["codes:equal_weights_ordered_by_symbol"]))
    C.append(DCase("codes_fibonacci_literals", (_fibonacci_literals(_rng(72)), 0, 1), ["codes:literal_lengths_pass_15", "header:n_cl_19_with_a_15_bit_code"]))
    C.append(DCase("codes_cl_limit", (_cl_limit_text(), 0, 1), ["codes:code_length_lengths_pass_7"]))
    C.append(DCase("codes_distance_chain", (_distance_chain_text(), 0, 1), ["codes:distance_lengths_pass_15", "place:a_token_of_more_than_32_bits", "place:the_longest_token_found"]))
    return C


def _header_runs():
    """63 byte values in groups of consecutive values -- 1, 2, 3, 4, 7, 8, 10, 11 and 5, 6, 6 more --, four bytes of each: with the end-of-block code
    64 symbols, six bits each, so every group is a run of its size; the unused values between the groups are runs of 1, 2, 3, 10, 11, 149 and 4, 5, 6, 2"""
    groups, gaps = (1, 2, 3, 4, 7, 8, 10, 11, 5, 6, 6), (1, 2, 3, 10, 11, 149, 4, 5, 6, 2)
    vals, v = [], 0
    for g, z in zip(groups, gaps + (0,)):
        vals += range(v, v + g)
        v += g + z
    assert len(vals) == 63 and v <= 256, v
    return vals


def _zero_run(k):
    """values 0 .. 20 and 21 + k .. 255 - (a few): one run of k unused values"""
    return list(range(21)) + list(range(21 + k, 21 + k + 42))


def header_cases():
    C = []
    rng = _rng(81)
    vals = np.array(_header_runs() * 4, np.uint8)
    C.append(DCase("header_runs", (rng.permutation(vals).tobytes(), 0, 1), ["header:zero_run_of_%d" % r for r in (1, 2, 3, 10, 11, 149)] + ["header:nonzero_run_of_%d" % r for r in (1, 2, 3, 4, 7, 8, 10, 11)] + ["header:symbol_18_with_its_least_and_its_greatest_value"]))
    C.append(DCase("header_n_cl_12", (_n_cl_12_text(), 0, 1), ["header:n_cl_12_the_smallest"]))
    for k in (138, 139):
        C.append(DCase("header_zero_run_%d" % k, (rng.permutation(np.array(_zero_run(k) * 4, np.uint8)).tobytes(), 0, 1), ["header:zero_run_of_%d" % k]))
    return C


# edge -> hex of a small text, found by a seeded search with the model: texts of 4 .. 69 bytes, random over 1 .. 39 neighbouring byte values or a random
# third of them repeated, the first text that reaches the edge
CHOOSE_TEXTS = {
    "choose:fixed_equals_dynamic:_fixed": "0412090613041004120906130410041209061304100412",
    "choose:fixed_one_above_dynamic:_dynamic": "907c8f8d93758b8e788b958d80859585778a86847585827d85927e91817a76858c7f7c7a738c787e918b7b95887d92787c94",
    "choose:bytes_equal_n+5:_stored": "d7dad4ced0ccdbd4d1d4c7c6d3c4c7c2c8cfdbc7dac8ccc5d1c3d5dbccda",
    "choose:bytes_equal_n+4:_not_stored": "a0988b99969ba0988b99969ba0988b99969b",
}


def choose_cases():
    C = []
    for e, h in CHOOSE_TEXTS.items():
        C.append(DCase("choose_" + e.split(":")[1].strip("_"), (bytes.fromhex(h), 0, 1), [e]))
    rng = _rng(91)
    rnd = rng.integers(0, 256, MAX_TEXT, dtype=np.uint8).tobytes()
    C.append(DCase("choose_stored_65280", (rnd, 0, 1), ["choose:a_full_member_of_65311_bytes", "choose:a_member_of_n+31_bytes"]))
    three = rnd[:300] + _illumina(300, 5) + b"ACGTTGCA"
    C.append(DCase("choose_three_kinds", (three, 300, 1), ["choose:all_three_kinds_in_one_call"]))
    return C


def _three_kinds(rng, k, n=4096):
    """member k of the long call: match-rich text, text without a match, random bytes"""
    v = k // 3 % 4
    if k % 3 == 0:
        return _illumina(n, 100 + v)
    if k % 3 == 1:
        return bytes(_filler(_rng(95, v), n))
    return _rng(96, v).integers(0, 256, n, dtype=np.uint8).tobytes()


def _mixed(rng, K):
    """K stretches of Illumina-shaped text, a few random bytes, a run, a period of four and random bases, of random lengths: small members of every size"""
    parts = []
    for k in range(K):
        parts += [_illumina(int(rng.integers(200, 900)), 30 + k), rng.integers(0, 256, int(rng.integers(5, 40)), dtype=np.uint8).tobytes(), bytes([65 + k % 4]) * int(rng.integers(5, 90)),
                  (b"ACGT" * 40)[:int(rng.integers(10, 120))], rng.integers(65, 69, int(rng.integers(10, 200)), dtype=np.uint8).tobytes()]
    return b"".join(parts)


def place_cases():
    mixed = _mixed(_rng(92, 0), 200)     # (members of 67 bytes reach the 256 pairs too, of 61 bytes 254 of them)
    return [DCase("place_pairs", (mixed, 79, 1), ["call:all_256_pairs_of_start_and_size_mod_16", "place:member_sizes_of_every_residue_mod_16",
                                                  "place:a_token_across_a_word_boundary_with_bits_in_the_upper_word", "place:stream_bits_mod_8_is_0", "place:stream_bits_mod_8_is_1",
                                                 "place:stream_bits_mod_8_is_7"])]


def call_cases():
    C = []
    rng = _rng(93)
    t = _illumina(257 * 16, 40)
    C.append(DCase("call_255_256_257", [(t[:k * 16], 16, 0) for k in (255, 256, 257)], ["call:255_members", "call:256_members", "call:257_members"]))
    long_call = b"".join(_three_kinds(rng, k) for k in range(2 * 256 + 1))
    C.append(DCase("call_513_members", (long_call, 4096, 1), ["call:513_members_of_4096_of_three_kinds_of_text", "call:stored_members_among_others"]))
    t = _illumina(9000, 41) + rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    C.append(DCase("call_capacity", [(t, 4096, 1, "need-1"), (t, 4096, 1, "need")], ["call:capacity_one_below_the_need", "call:capacity_exactly_the_need"]))
    return C


FAMILIES = ("stage", "find", "pay", "parse", "codes", "header", "choose", "place", "call")
_BUILDERS = dict(stage=stage_cases, find=find_cases, pay=pay_cases, parse=parse_cases, codes=codes_cases, header=header_cases, choose=choose_cases, place=place_cases, call=call_cases)
_CASES = None
_COVERAGE = []


def all_cases():
    global _CASES
    if _CASES is None:
        C = []
        for fam in FAMILIES:
            cs = _BUILDERS[fam]() if fam in _BUILDERS else []
            for c in cs:
                c.family = fam
            C += cs
        _CASES = C
    return _CASES


def cases_of(family, cases=None):
    return [c for c in (all_cases() if cases is None else cases) if c.family == family]


def coverage(cases=None):
    """Every predicate on every case in both modes -> ({edge: [(case, mode) that claim it and reach it]}, {case: [claims no mode reaches]}, {edge:
    [(case, mode) that reach it without a claim]}).  A member-level edge is reached by a case when one of its members reaches it."""
    cases = all_cases() if cases is None else cases
    if cases is _CASES and _COVERAGE:
        return _COVERAGE[0]
    edges = list(MEMBER_EDGES) + list(CASE_EDGES)
    table, lost, more = {e: [] for e in edges}, {}, {e: [] for e in edges}
    reached_by_member = {}
    for c in cases:
        got = set()
        for mode in MODES:
            v = c.view(mode)
            for m in v.members():
                if id(m) not in reached_by_member:
                    reached_by_member[id(m)] = {e for e, pred in MEMBER_EDGES.items() if pred(m)}
                for e in reached_by_member[id(m)]:
                    got.add((e, mode))
            for e, pred in CASE_EDGES.items():
                if pred(v):
                    got.add((e, mode))
        for e, mode in sorted(got):
            (table if e in c.claims else more)[e].append((c.name, MODE_NAME[mode]))
        for e in c.claims:
            if e not in edges or not any((e, mode) in got for mode in MODES):
                lost.setdefault(c.name, []).append(e)
    if cases is _CASES:
        _COVERAGE.append((table, lost, more))
    return table, lost, more


if __name__ == "__main__":
    t, lost, more = coverage()
    print("claimed  unclaimed  edge")
    for e, v in t.items():
        print("%7d  %9d  %s%s" % (len(v), len(more[e]), e, "   (unreachable: %s)" % UNREACHABLE[e] if e in UNREACHABLE else ""))
    cs = all_cases()
    print("%d cases in %d families, %d calls, %d bytes of text, %d edges, %d of them unreachable; claims that do not hold: %s; cases in no family: %s" % (
        len(cs), len({c.family for c in cs}), sum(len(c.calls) for c in cs), sum(c.n_bytes() for c in cs), len(t), len(UNREACHABLE), lost, [c.name for c in cs if c.family not in FAMILIES]))
    for f in FAMILIES:
        print("  %-7s %3d cases, %4d calls" % (f, len(cases_of(f)), sum(len(c.calls) for c in cases_of(f))))
