"""The edges of the piece-wise gunzip's OWN parts (csrc/faqcs_gunzip.h, faqcs_gunzip_kernel.hip; DESIGN.md sections 4.8 and 4.8a) as named
cases: the wave's symbol sink (literals batched on 64-symbol boundaries of the piece-relative offset, matches loaded 5 x 64 lanes, copied
periodically for dist < len, markers for sources in front of the piece), the marker life cycle (marker_source, resolve_piece over a piece's
last 32 768 symbols, narrow_slice over the rest in slices of 16 384, the front of 32 768 that holds the carried window) and gz_run's block
header parser beside plausible_block.  tests/gunzip_cases.py feeds these parts zlib's own output and six matches at a piece start; here the
position that matters is the PIECE start, and every match shape is put against it.

Streams are written with deflate_streams.Stream.  What a case must give is zlib's (gunzip_cases.zlib_model, gunzip_stream_cases.model), never
the library's.  Two plain models restate the scheme:

    chain_model  the pieces: a piece runs from its start to the first block end at or behind the end of the grid range that holds its start,
                 or to the final block -- from the block positions Stream.fields records.  info.n_pieces must equal it
    sym_model    the symbols: per piece 16-bit symbols (a byte, or 0x8000 | k for symbol k of the 32 768 in front of the piece; a copied
                 marker stays a marker), the last 32 768 of each piece resolved in order, everything narrowed, a marker outside the resolved
                 region looked up in front of its piece, a source in front of the member the error.  Its text must equal ds.expand() and
                 zlib's; its TRACE is what the edges are predicates of

EDGES is the coverage table: an edge counts for a case that claims it AND whose trace shows it (reached()); a test fails when an edge is
unreached or a claim does not hold.  MUTANTS are wrong versions of the two models; each must be told apart by a case: a text or a verdict
that is no longer zlib's, a piece count that is no longer the host statement's, or a claimed edge that the trace no longer shows.

    python -m tests.gunzip_edges       prints the cases per edge"""
import functools
import os
import struct
import sys
import zlib
from collections import namedtuple

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import deflate_streams as ds
import gunzip_cases as gc
import gunzip_stream_cases as gsc

WIN, SLICE, MIN_PIECE, DEFAULT_PIECE = 32768, 16384, 1024, 65536   # restated; test_gunzip_edges_model.py compares them with csrc/faqcs_gunzip.h
CONSTANT_SOURCES = {"WIN": r"\bWIN = (\d+)()", "SLICE": r"\bSLICE = (\d+)()", "MIN_PIECE": r"\bMIN_PIECE = (\d+)()", "DEFAULT_PIECE": r"\bDEFAULT_PIECE = (\d+)u << (\d+)"}
E_DATA, E_LENGTH, E_CRC, E_TRUNCATED = gc.E_DATA, gc.E_LENGTH, gc.E_CRC, gc.E_TRUNCATED
HEAD = 10                              # gz_member()'s header without optional fields
ROUNDS = 4000                          # stored and fixed blocks are starts no probe finds: a round each

GRID_K = (0, 1, 31, 63, 64, 65)
GRID_LEN = (3, 4, 63, 64, 65, 128, 129, 257, 258)
GRID_T = (1, 63, 64, 65)
GRID_DIST = ("1", "k", "k+1", "k+2", "k+len-1", "k+len", "k+len+1", "len-1", "32768", "first")
WAIT_K = (1, 63, 64, 65, 130)
WAIT_AT = (0, 1, 63)
WINDOWS = (1, 300, 32767, 32768)
FAMILIES = ("piece start", "markers of markers", "resolved or narrowed", "literals that wait", "member edges", "carried window", "valid streams", "invalid streams")

# How a refused member's code follows zlib's verdict on the raw stream (decompressobj(-15)); never wider than this:
#   zlib raises -> E_DATA;  zlib reaches the end and the trailer differs -> E_LENGTH, E_CRC when only the CRC differs;
#   zlib wants more input -> E_DATA or E_TRUNCATED (the same on host and device)
VERDICT_CODES = {"raises": (E_DATA,), "length": (E_LENGTH,), "crc": (E_CRC,), "more": (E_DATA, E_TRUNCATED)}
# the kinds of deflate_streams.INVALID_KINDS by how the yardstick refuses them (Case.refusal) -> the verdict above
REFUSAL_VERDICT = {"error": "raises", "incomplete": "more", "leftover": "length", "trailer": "length"}


def allowed_codes():
    """{kind of deflate_streams.INVALID_KINDS: the codes a refusal of it may state}"""
    out = {}
    for c in ds.invalid_cases():
        codes = VERDICT_CODES[REFUSAL_VERDICT[c.refusal]]
        assert out.setdefault(c.kind, codes) == codes, c.kind
    return out


# The ONE code faqcs_gunzip_* states for a stream of deflate_streams.invalid_cases() that stands alone in an ordinary gzip member, by the
# case's kind; every kind that is not named states E_DATA.  Recorded from the library, not designed: the table is there so that a change
# to gz_run, or one block decoder in place of gz_run and inflate_member, states what gz_run states today.  (In the "truncated" kinds that state E_DATA --
# truncated_cl_lens, truncated_counts, truncated_len_nlen -- and in no_final_block the trailer's bytes stand behind the cut: the bits go
# on, and what they say is wrong.)
CATALOGUE_CODES = {E_LENGTH: ("extra_byte", "literal_past_isize", "match_past_isize", "stored_past_isize"),
                   E_TRUNCATED: ("stored_past_input", "truncated_block_header", "truncated_code_length", "truncated_code_length_extra", "truncated_distance_extra",
                                 "truncated_distance_symbol", "truncated_length_extra", "truncated_symbol")}


def catalogue_code(kind):
    assert kind in ds.INVALID_KINDS
    return next((code for code, kinds in CATALOGUE_CODES.items() if kind in kinds), E_DATA)


def catalogue_member(c):
    """a case of deflate_streams.catalogue() as one gzip member: its raw stream and the trailer its BGZF member states"""
    raw, trailer = ds.raw_stream(c)
    crc, isize = struct.unpack("<II", trailer)
    return gc.gz_member(b"", raw=raw, crc=crc, isize=isize)


def zlib_verdict(raw, trailer):
    """zlib on a raw deflate stream and the eight bytes a gzip member states behind it -> "ok" or a key of VERDICT_CODES"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(raw) + d.flush()
    except zlib.error:
        return "raises"
    if not d.eof:
        return "more"
    tr = (d.unused_data + trailer)[:8]      # (the trailer stands in the next whole byte behind the final block)
    crc, isize = struct.unpack("<II", tr)
    return "length" if isize != len(text) & 0xFFFFFFFF else "crc" if crc != zlib.crc32(text) else "ok"


EDGES = {
    **{"k %d" % k: "%d literals of the piece's first block wait when its first match comes" % k for k in GRID_K},
    **{"len %d" % n: "that match has length %d" % n for n in GRID_LEN},
    **{"t %d" % t: "%d literals behind that match end the block" % t for t in GRID_T},
    "dist 1": "distance 1", "dist k": "the last in-piece source", "dist k+1": "the first source symbol is the last one in front of the piece: marker 32 767",
    "dist k+2": "dist < len and the period is part marker", "dist k+len-1": "every source but the last in front of the piece",
    "dist k+len": "the last source symbol is the last one in front of the piece", "dist k+len+1": "all markers, none of them the last one in front",
    "dist len-1": "the shortest period that is not the whole match", "dist 32768": "distance 32 768 from a piece start",
    "dist first": "the member's first byte exactly, from a later piece",
    "period part marker": "dist < len, its period holds markers and in-piece symbols", "all markers": "every symbol of a match is a marker",
    "source straddles": "dist >= len, the source straddles the piece start", "fixed test block": "the piece starts with a fixed block",
    "dynamic test block": "the piece starts with a dynamic block", "member shorter than 32768": "the first byte and 32 768 back differ",
    "markers copied in the block": "a match copies symbols an earlier match of the same block left as markers",
    "copied by the next piece": "the next piece copies what those markers became", "depth 3": "a byte that went through three markers, piece after piece",
    "source two pieces back": "a marker whose source lies two pieces and more in front, the pieces between shorter than 32 768",
    "narrowed at end-32768-1": "a marker at exactly end - 32 768 - 1 of its piece: narrow_slice looks it up",
    "resolved at end-32768": "a marker at exactly end - 32 768: the first that resolve_piece takes",
    "index 0 reads end-32768": "marker 0 of the next piece reads that symbol, which was a marker itself",
    "markers across a slice": "a run of narrowed markers across a multiple of 16 384", "narrowed index 0": "marker index 0, narrowed",
    "narrowed index 32767": "marker index 32 767 (0xFFFF), narrowed",
    **{"last slice %d mod 4" % r: "a piece's last slice has n = %d mod 4: the tail of narrow_slice" % r for r in (1, 2, 3)},
    **{"%d literals, then stored" % k: "%d literals end at a block end, a stored block follows" % k for k in WAIT_K},
    **{"%d literals, then Huffman" % k: "%d literals end at a block end, a Huffman block follows" % k for k in WAIT_K},
    **{"%d literals, then the end" % k: "%d literals end the member's final block: the flush at the run's end" % k for k in WAIT_K},
    **{"literals from %d mod 64" % o: "waiting literals begin at piece offset %d mod 64" % o for o in WAIT_AT},
    "block end on a range end": "a block that ends exactly on a range end, blocks behind it",
    "first byte from piece 3": "member 2: a match from its third piece or later to the member's first byte",
    "one in front from piece 3": "member 2: the same one byte further: E_DATA, the byte there is member 1's",
    **{"window %d" % w: "a call that reads a carried window of %d bytes" % w for w in WINDOWS},
    "window's first byte": "the first source is the carried window's first byte", "one in front of the window": "one byte in front of it: E_DATA, calls on",
    "period straddles the call": "dist < len, the period straddles the call boundary", "test block starts a call": "grid blocks, each the first piece of a call",
    "valid, alone": "a stream zlib never writes as the only member", "valid, concatenated": "those members in one file",
    "valid, behind a prefix": "behind a non-final stored block of piece + 1 bytes", "invalid, member 2": "an invalid stream as member 2",
    "invalid, behind a prefix": "the same behind the stored prefix",
}
# the edges that are a case's by construction (the file is built so); every other edge is a predicate of the trace
BY_CONSTRUCTION = frozenset(["valid, alone", "valid, concatenated", "valid, behind a prefix", "invalid, member 2", "invalid, behind a prefix", "test block starts a call",
                             "member shorter than 32768"] + ["window %d" % w for w in WINDOWS])

# name; family; the file; per member (Stream or None, the file byte where its deflate stream begins); the texts in front of the first bad
# member; its index (None: none); the codes it may state; consumed; piece sizes; the edges it is built for; feed: None, or (chunk ends,
# stops as gunzip_stream_cases.Feed has them, whether the LAST call must state the error and leave the state as it was)
Case = namedtuple("Case", "name family comp members texts bad codes consumed pieces claims feed")

# ---- the chain model --------------------------------------------------------------------------------------------------------------------
Block = namedtuple("Block", "start end n_out final kind")          # bits of the stream; kind: 0 stored, 1 fixed, 2 dynamic
Piece = namedtuple("Piece", "block start end pos n_out")           # first block; bits of the FILE (or chunk); text position in the member


def token_len(t):
    return 1 if isinstance(t, int) else t[0] if isinstance(t[0], int) else ds.LEN_BASE[t[1] - 257] + t[2] if t[0] == "L" else 0


def blocks_of(stream):
    starts, end = gc.block_starts(stream)
    raw = stream.getvalue()
    out = []
    for i, (kind, payload) in enumerate(stream.items):
        n = len(payload) if kind == "stored" else sum(token_len(t) for t in payload)
        out.append(Block(starts[i], starts[i + 1] if i + 1 < len(starts) else end, n, bool(raw[starts[i] >> 3] >> (starts[i] & 7) & 1), stream.block_types[i]))
    assert len(out) == len(starts) and out[-1].final and not any(b.final for b in out[:-1])
    return out


def chain_model(stream, head_bytes, piece_bytes, mutant=None, first=0, pos=0, stop_bit=None):
    """The pieces of one member whose stream begins head_bytes into the input (negative: in a call in front), from block `first` at text
    position pos.  stop_bit: the input ends there (a call with final = 0): a block that is not whole is not there, and the walk stops."""
    blocks = stream if isinstance(stream, list) else blocks_of(stream)
    P, shift = piece_bytes or DEFAULT_PIECE, 8 * head_bytes
    out, b = [], first
    while b < len(blocks):
        start = shift + blocks[b].start
        hi = 8 * (start // 8 // P + 1) * P
        e, n, cut = b, 0, False
        while e < len(blocks):
            end = shift + blocks[e].end
            if stop_bit is not None and end > stop_bit:
                cut = True
                break
            n += blocks[e].n_out
            e += 1
            if blocks[e - 1].final or (end > hi if mutant == "strictly behind" else end >= hi):
                break
        if e > b:
            out.append(Piece(b, start, shift + blocks[e - 1].end, pos, n))
        pos, b = pos + n, e
        if cut:
            break
    return out


# ---- the symbol model -------------------------------------------------------------------------------------------------------------------
# match: piece index; in the piece's first block; block kind; piece offset; length; distance; symbols that are markers of their own; copied
#        symbols that were markers; literals of the block in front of it; literals behind it when they end the block (else None)
# run:   a run of literals that ends at a block end -- piece index; piece offset of its first; length; what follows: "stored", "huffman",
#        "end" (the final block's end), "piece" (the piece's end)
# mark:  a marker that resolve_piece ("resolved") or narrow_slice ("narrowed") turned into a byte -- piece index; piece offset; index k;
#        its distance from the piece's end; pieces between it and its source; markers the byte went through; whether the source symbol was
#        a marker when the decode pass ended
Match = namedtuple("Match", "piece first kind o len dist own copied k t")
Run = namedtuple("Run", "piece o n then")
Mark = namedtuple("Mark", "how piece o k from_end back depth src_was_marker src")
Trace = namedtuple("Trace", "text bad pieces matches runs marks")
MUTANTS = {
    "no period": "i % dist dropped: the source of symbol i is i symbols behind the first, whatever the distance",
    "marker index": "marker index off by one",
    "rebased": "a copied marker re-based to the copying position",
    "resolve 32767": "resolve over the last 32 767 symbols",
    "resolve 32769": "resolve over the last 32 769 symbols",
    "narrow without look-up": "narrow without the look-up: a marker's low byte is the text",
    "member_pos + 1": "the member's first byte counts as in front of it",
    "member_pos - 1": "the byte in front of the member counts as its own",
    "literals lost": "literals lost when a run ends without a 64-boundary",
    "strictly behind": "a piece ends at the first block end strictly behind the range end",
}


def sym_model(stream, pieces, mutant=None):
    """The symbols of one member's pieces (chain_model's, of one call or of several calls in a row: the carried window is the text in front)
    -> Trace.  Member coordinates: the member's first byte is symbol 0."""
    blocks = blocks_of(stream)
    total = sum(p.n_out for p in pieces)
    assert [p.pos for p in pieces] == [sum(q.n_out for q in pieces[:i]) for i in range(len(pieces))]
    sym, depth = np.zeros(total + 1, np.int64), np.zeros(total + 1, np.int64)
    matches, runs, marks = [], [], []
    for pi, p in enumerate(pieces):
        shift = p.start - blocks[p.block].start
        out, dep = sym[p.pos:p.pos + p.n_out], depth[p.pos:p.pos + p.n_out]
        o, b, waiting = 0, p.block, 0
        while b < len(blocks) and blocks[b].end + shift <= p.end:
            kind, payload = stream.items[b]
            last = blocks[b].final or blocks[b].end + shift == p.end
            if kind == "stored":
                out[o:o + len(payload)] = np.frombuffer(payload, np.uint8)
                o += len(payload)
                b += 1
                continue
            k, pending, at = 0, None, len(matches)
            for t in payload:
                if isinstance(t, int):
                    out[o] = t
                    o, k = o + 1, k + 1
                    continue
                if t[0] == "L":
                    pending = ds.LEN_BASE[t[1] - 257] + t[2]
                    continue
                ln, dist = (pending, ds.DIST_BASE[t[1]] + t[2]) if t[0] == "D" else t
                vals, deps, own, copied = [], [], 0, 0
                for i in range(ln):      # every source is read before a symbol is written, as the wave's lanes do
                    s = o - dist + (i if dist >= ln or mutant == "no period" else i % dist)
                    if s < 0:
                        v, d, own = 0x8000 | (WIN + s + (1 if mutant == "marker index" else 0)) & 0xFFFF, 0, own + 1
                    else:
                        v, d = int(out[s]), int(dep[s])
                        if v & 0x8000:
                            copied += 1
                            if mutant == "rebased":
                                v = 0x8000 | (v + o + i - s) & 0x7FFF
                    vals.append(v)
                    deps.append(d)
                out[o:o + ln], dep[o:o + ln] = vals, deps
                if len(matches) > at:
                    matches[-1] = matches[-1]._replace(t=None)
                matches.append(Match(pi, b == p.block, blocks[b].kind, o, ln, dist, own, copied, k, 0))
                o, k = o + ln, 0
            if len(matches) > at:
                matches[-1] = matches[-1]._replace(t=k)
            if k:
                then = "end" if blocks[b].final else "piece" if last else "stored" if blocks[b + 1].kind == 0 else "huffman"
                runs.append(Run(pi, o - k, k, then))
                if last and mutant == "literals lost" and o & 63:
                    out[max(o - k, o & ~63):o] = 0
            b += 1
        assert o == p.n_out, (pi, o, p)
    was_marker = (sym & 0x8000) != 0
    lowest = {"member_pos + 1": 1, "member_pos - 1": -1}.get(mutant, 0)
    bad = False
    piece_of = np.zeros(total + 1, np.int64)
    for pi, p in enumerate(pieces):
        piece_of[p.pos:p.pos + p.n_out] = pi
    reach = {"resolve 32767": WIN - 1, "resolve 32769": WIN + 1}.get(mutant, WIN)

    def look_up(how, pi, p, i):
        nonlocal bad
        k = int(sym[i]) & 0x7FFF
        src = p.pos + k - WIN
        if src < lowest:
            bad = True
            return None
        marks.append(Mark(how, pi, i - p.pos, k, p.pos + p.n_out - i, pi - int(piece_of[src]), int(depth[src]) + 1, bool(was_marker[src]), src))
        depth[i] = depth[src] + 1
        return int(sym[src])

    for pi, p in enumerate(pieces):   # resolve: the pieces in order, the last WIN symbols of each
        end = p.pos + p.n_out
        a = end - reach if p.n_out > reach else p.pos
        for i in a + np.nonzero(sym[a:end] & 0x8000)[0]:
            v = look_up("resolved", pi, p, int(i))
            if v is not None:
                sym[i] = v
    text = sym[:total] & 255
    if mutant != "narrow without look-up":
        for pi, p in enumerate(pieces):   # narrow: what is still a marker is looked up in front of its piece
            for i in p.pos + np.nonzero(sym[p.pos:p.pos + p.n_out] & 0x8000)[0]:
                v = look_up("narrowed", pi, p, int(i))
                text[i] = 0 if v is None else v & 255
    return Trace(text.astype(np.uint8).tobytes(), bad, list(pieces), matches, runs, marks)


# ---- the edges as predicates of a member's trace ----------------------------------------------------------------------------------------
def edges_of(tr, later_member=False, feed=False):
    """the edges a member's trace shows.  later_member: the member is not the file's first (the member-edge cases); feed: the pieces are
    those of calls in a row, and the classes of the carried window are looked for in the last call's first match"""
    seen = set()
    n_out = {i: p.n_out for i, p in enumerate(tr.pieces)}
    first_match = {}
    for m in tr.matches:
        if m.first and m.piece > 0 and m.piece not in first_match:
            first_match[m.piece] = m
    for m in first_match.values():
        pos = tr.pieces[m.piece].pos
        if m.k not in GRID_K or m.len not in GRID_LEN or m.o != m.k:
            continue
        seen |= {"k %d" % m.k, "len %d" % m.len, "fixed test block" if m.kind == 1 else "dynamic test block"}
        if m.t in GRID_T:
            seen.add("t %d" % m.t)
        for name, d in (("1", 1), ("k", m.k), ("k+1", m.k + 1), ("k+2", m.k + 2), ("k+len-1", m.k + m.len - 1), ("k+len", m.k + m.len), ("k+len+1", m.k + m.len + 1),
                        ("len-1", m.len - 1), ("32768", 32768), ("first", pos + m.k)):
            if m.dist == d and (name != "k+2" or (m.dist < m.len and 0 < m.own < m.len)) and (name != "k+1" or m.own >= 1):
                seen.add("dist " + name)
        if m.dist < m.len and 0 < m.own < m.len and m.o > 0:
            seen.add("period part marker")
        if m.own == m.len:
            seen.add("all markers")
        if m.dist >= m.len and 0 < m.own < m.len:
            seen.add("source straddles")
        if m.dist == pos + m.k and m.piece >= 2:
            seen.add("first byte from piece 3" if later_member else "dist first")
    if tr.bad and later_member and len(tr.pieces) >= 3:
        seen.add("one in front from piece 3")
    if feed and tr.matches and tr.matches[-1].first:
        m = tr.matches[-1]
        if tr.pieces[m.piece].pos + m.o - m.dist == 0 and m.own:
            seen.add("window's first byte")
        if tr.pieces[m.piece].pos + m.o - m.dist == -1 and tr.bad:
            seen.add("one in front of the window")
        if m.dist < m.len and 0 < m.own < m.len:
            seen.add("period straddles the call")
    copied_in = {m.piece for m in tr.matches if m.copied}
    if copied_in:
        seen.add("markers copied in the block")
    for k in tr.marks:
        if k.back >= 1 and k.depth >= 2 and (k.piece - k.back) in copied_in:
            seen.add("copied by the next piece")
        if k.depth >= 3:
            seen.add("depth 3")
        if k.back >= 2 and all(n_out[q] < WIN for q in range(k.piece - k.back + 1, k.piece)):
            seen.add("source two pieces back")
        if k.how == "narrowed":
            if k.from_end == WIN + 1:
                seen.add("narrowed at end-32768-1")
            if k.k == 0:
                seen.add("narrowed index 0")
            if k.k == WIN - 1:
                seen.add("narrowed index 32767")
        if k.how == "resolved" and k.from_end == WIN and n_out[k.piece] > WIN:
            seen.add("resolved at end-32768")
        if k.how == "resolved" and k.k == 0 and k.src_was_marker and k.back == 1 and n_out[k.piece - 1] > WIN:
            seen.add("index 0 reads end-32768")
    narrowed = {(k.piece, k.o) for k in tr.marks if k.how == "narrowed"}
    if any((pi, o - 1) in narrowed for pi, o in narrowed if o and o % SLICE == 0):
        seen.add("markers across a slice")
    for p in tr.pieces:
        if p.n_out > WIN and p.n_out % SLICE % 4:
            seen.add("last slice %d mod 4" % (p.n_out % SLICE % 4))
    for r in tr.runs:
        if r.n in WAIT_K and r.then != "piece":
            seen.add("%d literals, then %s" % (r.n, {"stored": "stored", "huffman": "Huffman", "end": "the end"}[r.then]))
            if r.o % 64 in WAIT_AT:
                seen.add("literals from %d mod 64" % (r.o % 64))
    return seen


# ---- the builders -----------------------------------------------------------------------------------------------------------------------
def _rng(n):
    return np.random.Generator(np.random.PCG64([n, gc.SEED]))


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _lits(rng, n):
    return [int(v) for v in rng.integers(0, 256, n)]


def _huffman(s, j, toks, final=False):
    """block j of a file: alternately fixed and dynamic"""
    return s.fixed(toks, final=final) if j % 2 == 0 else s.dynamic(toks, ds.PLAIN_LIT, ds.PLAIN_DIST, final=final)


def _member(s):
    return gc.gz_member(ds.expand(s.items), raw=s.getvalue())


def _file(streams):
    """-> (the file of these members, ((Stream, where its deflate stream begins), ..), their texts)"""
    comp, members, texts = b"", [], []
    for s in streams:
        members.append((s, len(comp) + HEAD))
        texts.append(ds.expand(s.items))
        comp += gc.gz_member(texts[-1], raw=s.getvalue())
    return comp, tuple(members), tuple(texts)


def grid_combos(reduced=False):
    """(k, len, distance class) of the piece-start grid, no distance of 0; reduced: a sixth of them in which every k, len and class occurs"""
    out = [(k, n, d) for di, d in enumerate(GRID_DIST) for ni, n in enumerate(GRID_LEN) for ki, k in enumerate(GRID_K)
           if not (d == "k" and k == 0) and (not reduced or (ki + 2 * ni + di) % 6 == 0)]
    assert {c[0] for c in out} == set(GRID_K) and {c[1] for c in out} == set(GRID_LEN) and {c[2] for c in out} == set(GRID_DIST)
    return out


def _grid_streams(rng, piece, combos, front=WIN + 300):
    """The members of a piece-start grid.  A test block is k literals, the match, t literals, alternately fixed and dynamic; behind each a
    stored block of more than `piece` random bytes, so that the next test block is the first block of a piece (the chain model asserts it
    where the case is made).  One member has `front` bytes in front of its first test block: every class but "first"; the class "first"
    (the member's first byte, which must not be 32 768 back) lives in members of piece + 100 bytes of front that end before 32 768.
    -> [(Stream, [(block index, k, len, class)])]"""
    out, j = [], 0

    def member(part, first):
        nonlocal j
        s, pos, tests, made = ds.Stream(), first, [], {}
        s.stored(_bytes(rng, first))
        for n, (k, ln, dk) in enumerate(part):
            dist = {"1": 1, "k": k, "k+1": k + 1, "k+2": k + 2, "k+len-1": k + ln - 1, "k+len": k + ln, "k+len+1": k + ln + 1, "len-1": ln - 1, "32768": WIN,
                    "first": pos + k}[dk]
            assert 1 <= dist <= min(pos + k, WIN), (k, ln, dk, pos)
            if (k, ln, dist) in made:      # two classes that are one distance here: one block, both names
                b = made[(k, ln, dist)]
                tests.append((b, k, ln, dk))
                continue
            made[(k, ln, dist)] = len(s.items)
            t = GRID_T[j // 2 % 4] if j % 3 == 0 else 1
            tests.append((len(s.items), k, ln, dk))
            _huffman(s, j, _lits(rng, k) + [(ln, dist)] + _lits(rng, t))
            s.stored(_bytes(rng, piece + 64 + j % 64))
            pos += k + ln + t + piece + 64 + j % 64
            j += 1
        s.stored(b"", final=True)
        out.append((s, tests))

    member([c for c in combos if c[2] != "first"], front)
    near = [c for c in combos if c[2] == "first"]
    per = (WIN - (piece + 100) - 400) // (piece + 128 + 65 + 258 + 65)
    for i in range(0, len(near), per):
        member(near[i:i + per], piece + 100)
    return out


def _assert_tests_start_pieces(streams, members, piece):
    for (s, tests), (_, head) in zip(streams, members):
        starts = {p.block for p in chain_model(s, head, piece)}
        assert all(b in starts for b, _, _, _ in tests), "a test block is not the first block of a piece"


def _grid_claims(streams):
    claims = {"fixed test block", "dynamic test block", "member shorter than 32768", "period part marker", "all markers", "source straddles"} | {"t %d" % t for t in GRID_T}
    for _, tests in streams:
        for _, k, ln, dk in tests:
            claims |= {"k %d" % k, "len %d" % ln, "dist " + dk}
    return claims


def _align_front(front, at):
    """a front length >= `front` with which the block behind a stored block of it, the member's first, starts `at` bytes into a range of
    4 096 (and so of 1 024)"""
    return front + (at - (HEAD + 5 + front)) % 4096


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, family, comp, members, texts, claims, bad=None, codes=(), consumed=None, pieces=(1024, 4096), feed=None):
        for e in claims:
            assert e in EDGES, e
        out.append(Case(name, family, bytes(comp), tuple(members), tuple(texts), bad, tuple(codes), len(comp) if consumed is None else consumed, tuple(pieces),
                        frozenset(claims), feed))

    # ---- a match at a piece start -------------------------------------------------------------------------------------------------------
    for piece, reduced, limit in ((1024, False, 700000), (4096, True, 500000)):
        streams = _grid_streams(_rng(401 + piece), piece, grid_combos(reduced))
        comp, members, texts = _file([s for s, _ in streams])
        _assert_tests_start_pieces(streams, members, piece)
        assert sum(len(t) for t in texts) <= limit and len(comp) < 1 << 20 and len(texts[0]) > WIN + 300 and all(len(t) < WIN + piece + 400 for t in texts[1:])
        add("the grid at %d" % piece, "piece start", comp, members, texts, _grid_claims(streams), pieces=(piece,))
    # ---- markers of markers -------------------------------------------------------------------------------------------------------------
    rng = _rng(409)
    s = ds.Stream().stored(_bytes(rng, 33000))
    n1 = 2 + 50 + 20 + 40 + 4200          # piece 1: A leaves markers (three sources in front), B copies them, a filler in the same or the next piece
    s.dynamic(_lits(rng, 2) + [(50, 5), (20, 30)] + _lits(rng, 40), ds.PLAIN_LIT, ds.PLAIN_DIST).stored(_bytes(rng, 4200))
    n2 = 30 + 25 + 10 + 4300              # piece 2 copies what B wrote, and copies that again
    s.fixed([(30, n1 - 52)] + _lits(rng, 25) + [(10, 40)]).stored(_bytes(rng, 4300))
    n3 = 20 + 5 + 4400                    # piece 3 copies from piece 2
    s.dynamic([(20, n2)] + _lits(rng, 5), ds.PLAIN_LIT, ds.PLAIN_DIST).stored(_bytes(rng, 4400))
    s.fixed([(20, n3)] + _lits(rng, 3) + [(40, n3 + n2 + n1 - 60)], final=True)   # piece 4: from piece 3, and from piece 1's B over two pieces
    comp, members, texts = _file([s])
    add("markers of markers, depth 3", "markers of markers", comp, members, texts, ["markers copied in the block", "copied by the next piece", "depth 3", "source two pieces back"])
    # ---- resolved or narrowed -----------------------------------------------------------------------------------------------------------
    rng = _rng(419)

    def long_piece(name, toks_of, n_test, more, claims, behind=None):
        """front | a test block 100 bytes into a range | ONE stored block in the same piece, so long that the test block's markers at
        piece offset `more` and beyond lie inside the last 32 768 symbols and those in front of it outside | behind: tokens of a final
        block, the next piece"""
        front = _align_front(WIN + 500, 100)
        s = ds.Stream().stored(_bytes(rng, front))
        s.dynamic(toks_of(front), ds.PLAIN_LIT, ds.PLAIN_DIST)
        n = WIN + more - n_test
        s.stored(_bytes(rng, n), final=behind is None)
        if behind is not None:
            s.fixed(behind, final=True)
        comp, members, texts = _file([s])
        for piece in (1024, 4096):
            ps = chain_model(s, HEAD, piece)
            assert ps[1].block == 1 and ps[1].n_out == n_test + n, ps[:3]
        add(name, "resolved or narrowed", comp, members, texts, claims)

    # 258 markers at piece offsets 0 .. 257, the last 32 768 symbols begin at offset 103; the next piece's first symbol is 32 768 back
    long_piece("markers either side of end - 32768", lambda f: [(258, 261)] + _lits(rng, 5), 263, 103,
               ["narrowed at end-32768-1", "resolved at end-32768", "index 0 reads end-32768", "last slice 3 mod 4"], behind=[(3, WIN)] + _lits(rng, 2))
    # one literal, 63 x 258 copies of it, then 258 markers at offsets 16 255 .. 16 512: across 16 384, all outside the last 32 768
    long_piece("a marker run across a slice boundary", lambda f: _lits(rng, 1) + [(258, 1)] * 63 + [(258, 16255 + 258 + 7)] + _lits(rng, 4), 16517, 16517 + 1,
               ["markers across a slice", "last slice 2 mod 4"])
    # markers 0, 1, 2 (distance 32 768 at offset 0), a literal, then a match whose first source is the last symbol in front: 32 767
    long_piece("marker indices 0 and 32767, narrowed", lambda f: [(3, WIN)] + _lits(rng, 1) + [(6, 5)] + _lits(rng, 3), 13, 13 + 4,
               ["narrowed index 0", "narrowed index 32767", "last slice 1 mod 4"])
    # ---- literals that wait -------------------------------------------------------------------------------------------------------------
    rng = _rng(421)
    streams = []
    for k in WAIT_K:
        s, pos = ds.Stream(), 0

        def pad(at):
            """a stored block behind which the member's text stands at `at` mod 64"""
            nonlocal pos
            n = (at - pos) % 64 + 64
            s.stored(_bytes(rng, n))
            pos += n

        for at in WAIT_AT:
            pad(at)
            s.fixed(_lits(rng, k))                                              # k literals, then a stored block
            pos += k
            pad(at)
            s.dynamic(_lits(rng, k), ds.PLAIN_LIT, ds.PLAIN_DIST).fixed([(5, 70)])   # k literals, then a Huffman block
            pos += k + 5
        pad(63)
        s.dynamic(_lits(rng, k), ds.PLAIN_LIT, ds.PLAIN_DIST, final=True)       # and at the final block's end
        streams.append(s)
    comp, members, texts = _file(streams)
    # (with the default piece size every member is one piece: the offsets are the member's)
    add("five members of waiting literals", "literals that wait", comp, members, texts,
        ["%d literals, then %s" % (k, w) for k in WAIT_K for w in ("stored", "Huffman", "the end")] + ["literals from %d mod 64" % o for o in WAIT_AT], pieces=(0,))
    add("five members of waiting literals, cut by the ranges", "literals that wait", comp, members, texts, [], pieces=(1024, 4096))
    s = ds.Stream().dynamic(_lits(rng, 700), ds.PLAIN_LIT, ds.PLAIN_DIST)       # a piece from file byte 10 ...
    data_at = HEAD + (s.w.bitpos + 3 + 7) // 8 + 4
    s.stored(_bytes(rng, 4096 - data_at))                                       # ... to 4 096 exactly: the end of its range of 4 096
    assert 8 * HEAD + s.w.bitpos == 8 * 4096
    s.dynamic(_lits(rng, 4200), ds.PLAIN_LIT, ds.PLAIN_DIST)                    # a block longer than a range: a piece of its own, unless the one in front goes on
    s.fixed(_lits(rng, 65) + [(20, 30)])                                        # a piece from inside a range of 1 024 ...
    data_at = HEAD + (s.w.bitpos + 3 + 7) // 8 + 4
    s.stored(_bytes(rng, (-data_at) % 1024))                                    # ... to its end exactly
    assert (8 * HEAD + s.w.bitpos) % (8 * 1024) == 0 and 50 < (-data_at) % 1024
    s.dynamic(_lits(rng, 1100), ds.PLAIN_LIT, ds.PLAIN_DIST).stored(_bytes(rng, 5000)).fixed(_lits(rng, 1), final=True)
    comp, members, texts = _file([s])
    assert all(len(chain_model(s, HEAD, P)) == len(chain_model(s, HEAD, P, "strictly behind")) + 1 for P in (1024, 4096))
    add("a block end on a range end", "literals that wait", comp, members, texts, ["block end on a range end"])
    # ---- member edges from a later piece --------------------------------------------------------------------------------------------------
    rng = _rng(431)
    good = ds.Stream().stored(_bytes(rng, 1500)).fixed(_lits(rng, 7) + [(9, 3)] + [0x5A], final=True)   # member 1: its last byte is 0x5A
    for one_more in (0, 1):
        s = ds.Stream().stored(bytes([0xA5]) + _bytes(rng, 4199))                                       # member 2: its first byte is not
        s.dynamic(_lits(rng, 10), ds.PLAIN_LIT, ds.PLAIN_DIST).stored(_bytes(rng, 4200))
        s.fixed(_lits(rng, 1) + [(63, 4200 + 10 + 4200 + 1 + one_more)] + _lits(rng, 4), final=True)
        if one_more:
            m1 = _member(good)
            # (the trailer states what a decoder makes that reads member 1's last byte there: it reaches a CRC that agrees)
            comp = m1 + gc.gz_member(ds.expand([("stored", b"\x5a")] + s.items)[1:], raw=s.getvalue())
            add("member 2 reaches one byte in front of itself from its third piece", "member edges", comp, [(good, HEAD), (s, len(m1) + HEAD)], [ds.expand(good.items)],
                ["one in front from piece 3"], bad=1, codes=(E_DATA,), consumed=len(m1))
        else:
            comp, members, texts = _file([good, s])
            assert texts[1][-67] == 0xA5
            add("member 2 reaches its first byte from its third piece", "member edges", comp, members, texts, ["first byte from piece 3"])
    # ---- the carried window ---------------------------------------------------------------------------------------------------------------
    rng = _rng(433)
    combos = [c for i, c in enumerate(c for c in grid_combos() if c[2] != "first") if i % 12 == 5]
    assert 36 <= len(combos) <= 44
    (s, tests), = _grid_streams(rng, 1024, combos)
    comp, members, texts = _file([s])
    bl = blocks_of(s)
    ends = [HEAD + bl[b].start // 8 for b, _, _, _ in tests]
    assert all(bl[b].start % 8 == 0 for b, _, _, _ in tests)
    stops = [(c, dict(phase=gsc.STREAM, bit=0, total_comp=e, member_bytes=sum(x.n_out for x in bl[:b]))) for c, (e, (b, _, _, _)) in enumerate(zip(ends, tests))]
    claims = {"test block starts a call", "window 32768"} | {"k %d" % k for _, k, _, _ in tests} | {"len %d" % n for _, _, n, _ in tests} | {"dist " + d for _, _, _, d in tests}
    add("grid blocks, each the first piece of a call", "carried window", comp, members, texts, claims, pieces=(1024, 0), feed=(tuple(ends), tuple(stops), False))
    for w in WINDOWS:
        for cls, k, ln, more in (("window's first byte", 2, 12, 0), ("one in front of the window", 2, 12, 1), ("period straddles the call", 1, 10, None)):
            s = ds.Stream()
            halves = (w - w // 2, w // 2) if w > 1 else (1,)   # the window's bytes come in two calls
            for h in halves:
                s.stored(_bytes(rng, h))
            if more is not None:      # (no distance is above 32 768: the full window has nothing in front that a match could name)
                k = min(k, WIN - w - more)
                if k < 0:
                    continue
            dist = k + w + more if more is not None else min(3, k + w)
            _huffman(s, w, _lits(rng, k) + [(ln, dist)] + _lits(rng, 30), final=True)
            bl = blocks_of(s)
            ends = [HEAD + b.start // 8 for b in bl[1:]]
            stops = [(c, dict(phase=gsc.STREAM, bit=0, total_comp=e, member_bytes=sum(x.n_out for x in bl[:c + 1]), window_bytes=sum(x.n_out for x in bl[:c + 1])))
                     for c, e in enumerate(ends)]
            name = "%s, a window of %d" % (cls, w)
            if more:
                comp = gc.gz_member(b"stated, never made", raw=s.getvalue())
                add(name, "carried window", comp, [(s, HEAD)], [], [cls, "window %d" % w], bad=0, codes=(E_DATA,), consumed=0, pieces=(1024,), feed=(tuple(ends), tuple(stops), True))
            else:
                comp, members, texts = _file([s])
                add(name, "carried window", comp, members, texts, [cls, "window %d" % w], pieces=(1024,), feed=(tuple(ends), tuple(stops), False))
    # ---- the streams zlib never writes ----------------------------------------------------------------------------------------------------
    rng = _rng(439)
    valid = ds.valid_cases()
    assert {c.name for c in ds.grid_cases()} <= {c.name for c in valid}
    comp, members, texts = b"", [], []
    for c in valid:
        raw, trailer = ds.raw_stream(c)
        m = gc.gz_member(c.text, raw=raw)
        assert m[-8:] == trailer
        add("valid: " + c.name, "valid streams", m, [(c.stream, HEAD)], [c.text], ["valid, alone"], pieces=gc.PIECES)
        members.append((c.stream, len(comp) + HEAD))
        texts.append(c.text)
        comp += m
    assert len(comp) < 1 << 20
    add("valid: every stream in one file", "valid streams", comp, members, texts, ["valid, concatenated"], pieces=gc.PIECES)
    for piece in (1024, 4096):
        for c in valid:
            front = _bytes(rng, piece + 1)
            pre = ds.stored_prefix(front)
            blocks = [Block(0, 8 * len(pre), len(front), False, 0)] + [b._replace(start=b.start + 8 * len(pre), end=b.end + 8 * len(pre)) for b in blocks_of(c.stream)]
            add("valid behind a prefix of %d: %s" % (piece + 1, c.name), "valid streams", gc.gz_member(front + c.text, raw=pre + ds.raw_stream(c)[0]), [(blocks, HEAD)],
                [front + c.text], ["valid, behind a prefix"], pieces=(piece,))
    # ---- the invalid streams, as member 2 -----------------------------------------------------------------------------------------------
    good = ds.Stream().stored(_bytes(rng, 1500)).dynamic(_lits(rng, 200) + [(30, 100)], ds.PLAIN_LIT, ds.PLAIN_DIST, final=True)
    m1, t1 = _member(good), ds.expand(good.items)
    codes = allowed_codes()
    for c in ds.invalid_cases():
        raw, trailer = ds.raw_stream(c)
        add("invalid: " + c.name, "invalid streams", m1 + b"\x1f\x8b\x08\x00\0\0\0\0\x02\x03" + raw + trailer, [(good, HEAD), (None, len(m1) + HEAD)], [t1], ["invalid, member 2"],
            bad=1, codes=codes[c.kind], consumed=len(m1), pieces=gc.PIECES)
        for piece in (1024, 4096):
            front = _bytes(rng, piece + 1)
            # the trailer states what it stated, with the prefix in front: ISIZE grows by it, the CRC is that of the prefix and as much of
            # zlib's text as the old ISIZE covers where the old CRC was that text's, else it stays wrong
            d = zlib.decompressobj(-15)
            try:
                part = d.decompress(raw)
            except zlib.error:
                part = b""
            crc0, isize0 = struct.unpack("<II", trailer)
            crc = zlib.crc32(front + part[:isize0]) if len(part) >= isize0 and zlib.crc32(part[:isize0]) == crc0 else crc0 ^ 0x5A5A5A5A
            raw2, trailer2 = ds.stored_prefix(front) + raw, struct.pack("<II", crc, (isize0 + len(front)) & 0xFFFFFFFF)
            m2 = b"\x1f\x8b\x08\x00\0\0\0\0\x02\x03" + raw2 + trailer2
            # (the prefix is history too: a distance one byte in front of the member now has a source, and what is left is the wrong CRC.
            # So the codes here are those of zlib's verdict on THIS stream, not the kind's)
            add("invalid behind a prefix of %d: %s" % (piece + 1, c.name), "invalid streams", m1 + m2, [(good, HEAD), (None, len(m1) + HEAD)], [t1], ["invalid, behind a prefix"],
                bad=1, codes=VERDICT_CODES[zlib_verdict(raw2, trailer2)], consumed=len(m1), pieces=(piece,))
    assert len({c.name for c in out}) == len(out) and all(len(c.comp) < 1 << 20 for c in out) and {c.family for c in out} == set(FAMILIES)
    return tuple(out)


def cases_of(family, piece=None):
    return [c for c in cases() if c.family == family and (piece is None or piece in c.pieces)]


def as_gunzip_case(c):
    """the case as gunzip_cases.assert_case() takes it: one code where only one is allowed, else any error"""
    return gc.Case(c.name, c.comp, c.texts, c.bad, 0 if c.bad is None else c.codes[0] if len(c.codes) == 1 else None, c.consumed, c.pieces, ROUNDS, c.claims)


def as_feed(c):
    return gsc.Feed(c.name, c.comp, c.feed[0], c.pieces, ROUNDS, frozenset(), c.feed[1])


# ---- the models on a case -----------------------------------------------------------------------------------------------------------------
def feed_pieces(c, piece, mutant=None):
    """the chain model's pieces of every call of a feed, in the call's own bit positions.  (A feed is one member, and every call consumes
    its chunk: the stops say so.)"""
    (s, head), = c.members
    blocks, out, at, first, pos = blocks_of(s), [], 0, 0, 0
    for end in list(c.feed[0]) + [len(c.comp)]:
        ps = chain_model(blocks, head - at, piece, mutant, first, pos, None if end == len(c.comp) else 8 * (end - at))
        out.append(ps)
        if ps:
            first, pos = next(i for i, b in enumerate(blocks) if 8 * (head - at) + b.end == ps[-1].end) + 1, ps[-1].pos + ps[-1].n_out
        at = end
    return out


def member_pieces(c, piece, mutant=None):
    """-> per member with a Stream the chain model's pieces of the whole file, or of a feed's calls in a row; None for a member without"""
    if c.feed is not None:
        return [[p for ps in feed_pieces(c, piece, mutant) for p in ps]]
    return [None if s is None else chain_model(s, head, piece, mutant) for s, head in c.members]


def n_pieces_model(c, piece, mutant=None):
    """info.n_pieces of the whole-file call, None where a member has no Stream (the invalid catalogue: what the walk takes of it is the
    library's)"""
    ps = member_pieces(c, piece, mutant)
    return None if any(p is None for p in ps) else sum(len(p) for p in ps)


@functools.lru_cache(maxsize=None)
def traces(name, piece, mutant=None):
    """-> per member its Trace (None without a Stream) under the models, or under a mutant of them"""
    c = next(c for c in cases() if c.name == name)
    out = []
    for (s, head), ps in zip(c.members, member_pieces(c, piece, mutant)):
        if ps is None or isinstance(s, list):
            out.append(None)
            continue
        out.append(sym_model(s, ps, None if mutant == "strictly behind" else mutant))
    return out


def verdict(c, piece, mutant=None):
    """what the models make of a case -> (the texts of its members in front of the first refused one, the refused member or None, n_pieces
    or None, the edges the traces show)"""
    texts, bad, seen = [], None, set()
    for k, ((s, head), tr) in enumerate(zip(c.members, traces(c.name, piece, mutant))):
        if tr is None:
            if s is None:
                bad = k if bad is None else bad
            elif bad is None:
                texts.append(None)   # (a member behind a prefix: its blocks are known, its tokens are the catalogue's)
            continue
        seen |= edges_of(tr, later_member=k > 0, feed=c.feed is not None)
        if c.name == "a block end on a range end":
            ps = tr.pieces
            P = piece or DEFAULT_PIECE
            if any(p.end == 8 * P * (p.start // (8 * P) + 1) and p is not ps[-1] for p in ps):
                seen.add("block end on a range end")
        if bad is None:
            if tr.bad:
                bad = k
            else:
                texts.append(tr.text)
    return texts, bad, n_pieces_model(c, piece, mutant), seen | (c.claims & BY_CONSTRUCTION)


def reached(c, piece):
    return verdict(c, piece)[3]


def coverage():
    """{edge: the (case, piece size) that claim it and whose traces show it}, and the claims that do not hold"""
    cov, lost = {e: [] for e in EDGES}, []
    for c in cases():
        for piece in c.pieces:
            seen = reached(c, piece)
            for e in c.claims:
                if e in seen:
                    cov[e].append("%s at %d" % (c.name, piece))
                else:
                    lost.append((c.name, piece, e))
    return cov, lost


def model_cases():
    """the cases the models have something to say about: all but the two catalogues of deflate_streams.py, which are zlib's and the host's"""
    return [c for c in cases() if c.family not in ("valid streams", "invalid streams")]


def caught(mutant):
    """the first (case, piece size, why) that tells a mutant from the models: a text or a verdict that is no longer zlib's, a piece count that is no
    longer the true rule's, a claimed edge the trace no longer shows.  None: nothing does"""
    for c in model_cases():
        for piece in c.pieces:
            texts, bad, n, seen = verdict(c, piece, mutant)
            if bad != c.bad or [t for t in texts if t is not None] != list(c.texts):
                return c.name, piece, "the text or the verdict"
            if n != n_pieces_model(c, piece):
                return c.name, piece, "the piece count"
            lost = (c.claims - BY_CONSTRUCTION) - seen
            if lost:
                return c.name, piece, "the edge %r" % sorted(lost)[0]
    return None


# ---- a case against a statement of the rules: the host's, then the device's -------------------------------------------------------------------
def capacity(c):
    return sum(len(t) for t in c.texts) + (0 if c.bad is None else 400000)


def check_info(c, piece, info, text, what):
    """info and the text buffer (the layout of gunzip_cases.gunzip_host) of a whole-file call against the case: zlib's text and verdict,
    the code among those the verdict allows, the chain model's piece count"""
    gc.assert_case(as_gunzip_case(c), info, text, what)
    if c.bad is not None:
        assert info["error"] in c.codes, "%s: error %d, allowed %s" % (what, info["error"], c.codes)
    n = n_pieces_model(c, piece)
    assert n is None or info["n_pieces"] == n, "%s: %d pieces, the chain model has %d" % (what, info["n_pieces"], n)


def run_feed(call, c, piece, window=None):
    """a feed case through `call` (gunzip_stream_cases.host_call's form) -> its calls: zlib's text and state call by call (check_calls),
    every call stopped at its cut with bit = 0 (check_stops), the chain model's piece count per call, and for a feed built for it the
    error in the last call with the state as the call in front left it"""
    what = "%s at %d" % (c.name, piece)
    f = as_feed(c)
    calls = gsc.feed(call, c.comp, f.ends, piece, ROUNDS, window=window)
    gsc.check_calls(c.comp, calls, what, code=c.codes[0] if c.bad is not None else None)
    gsc.check_stops(f, calls, what)
    want = [len(ps) for ps in feed_pieces(c, piece)]
    assert len(calls) == len(want), what
    for k, (call_k, n) in enumerate(zip(calls, want)):
        assert call_k.info["n_pieces"] == n, "%s, call %d: %d pieces, the chain model has %d" % (what, k, call_k.info["n_pieces"], n)
        if not call_k.info["error"] and not call_k.final:
            assert call_k.at + call_k.info["consumed"] == call_k.end and call_k.state["bit"] == 0, "%s, call %d did not stop at its cut" % (what, k)
    last = calls[-1]
    if c.feed[2]:
        assert (last.info["error"], last.info["consumed"], last.info["n_bytes"], last.info["n_members"]) == (c.codes[0], 0, 0, 0), "%s: %s" % (what, last.info)
        assert last.state == calls[-2].state and last.window == calls[-2].window, what + ": the refused call changed the state"
    else:
        assert last.info["error"] == 0 and b"".join(k.text for k in calls) == b"".join(c.texts), what
    return calls


def write_corpus(path, probes, files, feeds):
    """The file tools/gunzip_probe_check.cpp reads, little-endian 32-bit words: a count, then per probe entry {mode, size, bytes, count, bit
    positions (64 bits each)}; a count, then per file {piece_bytes, error expected, n_members, text length, CRC-32 of the text, size,
    bytes}; a count, then per feed {piece_bytes, error expected, text length, CRC-32, count, chunk ends, size, bytes}."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(probes)))
        for mode, raw, positions in probes:
            f.write(struct.pack("<II", mode, len(raw)) + raw + struct.pack("<I", len(positions)) + b"".join(struct.pack("<Q", p) for p in positions))
        f.write(struct.pack("<I", len(files)))
        for piece, error, n_members, text, comp in files:
            f.write(struct.pack("<IIIIII", piece, error, n_members, len(text), zlib.crc32(text), len(comp)) + comp)
        f.write(struct.pack("<I", len(feeds)))
        for piece, error, text, ends, comp in feeds:
            f.write(struct.pack("<IIIII", piece, error, len(text), zlib.crc32(text), len(ends)) + b"".join(struct.pack("<I", e) for e in ends) + struct.pack("<I", len(comp)) + comp)


if __name__ == "__main__":
    cov, lost = coverage()
    print("  cases  edge")
    for e, v in cov.items():
        print("%7d  %-36s %s" % (len(v), e, v[0] if v else "UNREACHED"))
    print("%d cases in %d families, %d edges; claims that do not hold: %s" % (len(cases()), len(FAMILIES), len(EDGES), lost))
    for m in MUTANTS:
        print("mutant %-24s %s" % (m, caught(m)))
