"""A constructed catalogue of inputs for faqcs_parse_device, faqcs_emit_device and faqcs_render_device that puts record edges on every hard
edge of the machinery the three share (faqcs_pack_common.h: the block scan, the one-block scan of the tile sums, the piece walker) and of
the parse index (faqcs_parse_kernel.hip).  Nothing here is drawn at random and nothing is left to chance: every case is a named builder,
every edge a PREDICATE over the model's output for a case (offsets, line starts, counts), and coverage() evaluates every predicate on
every case.  tests/test_pack_edges_model.py holds the catalogue against the models and the host statements without a GPU;
tests/test_gpu_pack_edges.py sends it to the device.  Plain Python and numpy: no GPU and no ctypes at import.

    python -m tests.pack_edges        prints the number of cases per edge
"""
import numpy as np

# ---- the structure constants, restated (test_pack_edges_model.py compares them with the constexprs of the two sources) ---------------
PIECE = 16                # bytes a lane owns
WAVE_BYTES = 1024         # a wave step: 64 pieces
SPAN_BYTES = 8192         # SPAN_ITERS = 8 wave steps behind one binary search
TEXT_TILE = 16384         # a tile of the parse index
REC_TILE = 256            # records of a parse record tile (REC_THREADS)
TILE_ITEMS = 1024         # reads of a tile of the emit / render scan
SCAN_THREADS = 1024       # tiles per round of the one-block scans
GRID_BLOCKS_PER_CU = 8    # blocks per compute unit beyond which parse_rec_totals / parse_rec_apply and the gathers stride
DEFAULT_CU = 256          # what the launchers assume without device properties; an MI355X has 256

# where the sources state them: {name: (file under faqcs_amd/csrc, regular expression whose groups multiply to the value)}
CONSTANT_SOURCES = {
    "PIECE": ("faqcs_pack_common.h", r"WAVE_BYTES = FAQCS_WAVE \* (\d+)"),
    "WAVE_BYTES": ("faqcs_pack_common.h", r"WAVE_BYTES = FAQCS_WAVE \* (\d+)"),          # x FAQCS_WAVE (faqcs_dev.h)
    "SPAN_BYTES": ("faqcs_pack_common.h", r"SPAN_ITERS = (\d+), WAVE_BYTES = FAQCS_WAVE \* (\d+)"),  # x FAQCS_WAVE
    "TEXT_TILE": ("faqcs_parse_kernel.hip", r"TEXT_THREADS = (\d+), TEXT_PPT = (\d+), TEXT_PIECES = TEXT_THREADS \* TEXT_PPT, TEXT_TILE = TEXT_PIECES \* (\d+)"),
    "REC_TILE": ("faqcs_parse_kernel.hip", r"REC_THREADS = (\d+)"),
    "TILE_ITEMS": ("faqcs_pack_common.h", r"TILE_THREADS = (\d+), TILE_RPT = (\d+), TILE_ITEMS = TILE_THREADS \* TILE_RPT"),
    "SCAN_THREADS": ("faqcs_pack_common.h", r"SCAN_THREADS = (\d+)"),
    "GRID_BLOCKS_PER_CU": ("faqcs_parse_kernel.hip", r"const size_t cap = \(size_t\)\(n_cu > 0 \? n_cu : \d+\) \* (\d+)"),
    "DEFAULT_CU": ("faqcs_parse_kernel.hip", r"const size_t cap = \(size_t\)\(n_cu > 0 \? n_cu : (\d+)\)"),
}
WAVE_CONSTANTS = ("WAVE_BYTES", "SPAN_BYTES")  # their expressions carry a factor FAQCS_WAVE

# parse_cases.TAILS, restated for the same reason (the CPU test compares)
TAILS = ("clean", "clean_open", "blank_line", "defline_only", "defline_open", "no_plus", "no_plus_open", "plus_open", "no_quality")
_TAIL_TEXT = {"clean": b"", "clean_open": b"", "blank_line": b"\n", "defline_only": b"@tail\n", "defline_open": b"@tail", "no_plus": b"@tail\nACGT\n",
              "no_plus_open": b"@tail\nACGT", "plus_open": b"@tail\nACGT\n+", "no_quality": b"@tail\nACGT\n+\n"}

F_VALID = 1
RESULT_DTYPE = np.dtype([("start", "<u2"), ("len", "<u2"), ("flags", "<u2"), ("adapter", "<u2")])  # faqcs_read_result (_capi.RESULT_DTYPE)

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def bases(n, salt=0):
    """n bases over ACGT, a fixed hash of the position: no period that a misplaced piece, KiB or span could hide behind."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt)
    return _ACGT[((i * np.uint64(2654435761) + (i >> np.uint64(3)) * np.uint64(40503)) >> np.uint64(13)) & np.uint64(3)]


def quals(n, salt=0):
    """n quality bytes '#' .. 'J' (Phred+33 2 .. 41; never the input offset itself, so a masked position always differs)."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt)
    return (35 + (((i * np.uint64(2246822519) + (i >> np.uint64(2)) * np.uint64(3266489917)) >> np.uint64(11)) % np.uint64(40))).astype(np.uint8)


# =====================================================================================================================================
# parse texts
# =====================================================================================================================================

def record(k, n_bases, eol=b"\n", defline=None, cr_at=None, qual_extra=b""):
    """Record k: n_bases bases.  cr_at: a lone '\\r' at that position of the base AND the quality line (a shorter, valid record)."""
    s, q = bases(n_bases, 7919 * k).tobytes(), quals(n_bases, 104729 * k).tobytes()
    if cr_at is not None:
        s, q = s[:cr_at] + b"\r" + s[cr_at:], q[:cr_at] + b"\r" + q[cr_at:]
    d = (b"@r%d" % k) if defline is None else defline
    return d + eol + s + eol + b"+" + eol + q + qual_extra + eol


def sized_text(n, k0=0, eol=b"\n"):
    """Exactly n bytes (n >= 15) of whole records that end in '\\n': records of 0 .. 40 bases, the last one's defline padded to fit."""
    out, left, k = [], n, k0
    while True:
        r = record(k, (k * 11) % 41, eol)
        if left - len(r) < 120:
            break
        out.append(r)
        left -= len(r)
        k += 1
    # one or two records take exactly what is left
    if left >= 60:
        r = record(k, 7, eol, defline=b"@p")
        out.append(r)
        left -= len(r)
        k += 1
    fixed = len(record(k, 2, eol, defline=b""))
    assert left >= fixed, (n, left)
    out.append(record(k, 2, eol, defline=b"@" + b"x" * (left - fixed - 1) if left > fixed else b""))
    text = b"".join(out)
    assert len(text) == n, (len(text), n)
    return text


def tiny_records(n, bad=(), n_variant=True):
    """n records of 8 bytes (b"@\\nA\\n+\\nI\\n") with a sprinkling of 0- to 3-base ones, so that offsets are no multiple of anything; the
    records of `bad` carry one quality byte too many.  -> (text, base count per record)"""
    k = np.arange(n, dtype=np.int64)
    lens = np.where(k % 7 == 3, (k // 7 * 5) % 4, 1)
    tmpl = {}
    for L in range(4):
        for v in range(3):
            s = (b"ACG", b"NTA", b"GNN")[v][:L] if n_variant else b"ACG"[:L]
            q = (b"I5#", b"#J7", b"A?+")[v][:L]
            tmpl[(L, v, 0)] = b"@\n" + s + b"\n+\n" + q + b"\n"
            tmpl[(L, v, 1)] = b"@\n" + s + b"\n+\n" + q + b"I\n"
    bad = set(int(b) for b in bad)
    var = (k // 5) % 3
    parts = [tmpl[(L, v, 0)] for L, v in zip(lens.tolist(), var.tolist())]
    for b in bad:
        parts[b] = tmpl[(int(lens[b]), int(var[b]), 1)]
    return b"".join(parts), lens


class ParseCase:
    """name, text, the values of `final` it runs with, the edges it claims (per value of final: 'edge' or 'edge/final' 'edge/open'),
    the cuts of a chunked feed (or None)."""

    def __init__(self, name, text, claims, finals=(True, False), cuts=None):
        self.kind, self.name, self.text, self.claims, self.finals, self.cuts = "parse", name, text, tuple(claims), tuple(finals), cuts
        self._ctx = {}

    def ctx(self, final):
        if final not in self._ctx:
            self._ctx[final] = ParseCtx(self.text, final, self.cuts)
        return self._ctx[final]


class ParseCtx:
    """What the predicates look at: the line structure of a text and what the parse rules of include/faqcs_mi.h make of it -- computed here
    with numpy from the rules, independently of driver.parse_model (the CPU test compares the two)."""

    def __init__(self, text, final, cuts=None):
        t = np.frombuffer(text, np.uint8)
        self.t, self.final, self.n_text, self.cuts = t, final, len(t), cuts
        self.nl, self.cr = np.nonzero(t == 10)[0], np.nonzero(t == 13)[0]
        n_nl = len(self.nl)
        self.open = self.n_text > 0 and t[-1] != 10
        ltot = n_nl + (1 if self.open else 0)
        self.rem = ltot % 4
        self.n_cand = ltot // 4 if final else n_nl // 4
        # lines 0 .. 4 n_cand - 1: [start, end) without the '\n'
        nline = 4 * self.n_cand
        starts = np.concatenate([[0], self.nl + 1])[:nline]
        ends = np.concatenate([self.nl, [self.n_text]])[:nline]
        self.ls, self.le = starts.astype(np.int64), ends.astype(np.int64)
        ic = np.searchsorted(self.cr, self.ls)  # the first '\r' at or behind the line start
        first_cr = np.where(ic < len(self.cr), self.cr[np.minimum(ic, max(len(self.cr) - 1, 0))] if len(self.cr) else self.n_text, self.n_text + 16)
        self.first_cr = first_cr.astype(np.int64)
        self.ce = np.minimum(self.first_cr, self.le)  # content end
        clen = self.ce - self.ls
        self.slen, self.qlen = clen[1::4], clen[3::4]
        self.bad = np.nonzero(self.slen != self.qlen)[0]
        self.n_reads = int(self.bad[0]) if len(self.bad) else self.n_cand
        self.offset = np.concatenate([[0], np.cumsum(self.slen[:self.n_reads])]).astype(np.int64)
        self.n_tiles = (self.n_text + TEXT_TILE - 1) // TEXT_TILE
        self.tile_nl = np.bincount(self.nl // TEXT_TILE, minlength=self.n_tiles) if self.n_tiles else np.zeros(0, np.int64)
        self.tile_cr = np.bincount(self.cr // TEXT_TILE, minlength=self.n_tiles) if self.n_tiles else np.zeros(0, np.int64)

    def tail(self):
        """The name in TAILS of how the text ends (what lies behind its last whole record)."""
        if self.rem == 0:
            return "clean_open" if self.open else "clean"
        if self.rem == 1:
            if self.open:
                return "defline_open"
            last_start = int(self.nl[-2]) + 1 if len(self.nl) > 1 else 0
            return "blank_line" if int(self.nl[-1]) == last_start else "defline_only"
        if self.rem == 2:
            return "no_plus_open" if self.open else "no_plus"
        return "plus_open" if self.open else "no_quality"

    def chunk_lengths(self):
        """Lengths of the texts a chunked feed (parse_cases.chunked) hands over with final = 0: from where the last call's consumed ended to the cut."""
        out, start = [], 0
        for c in self.cuts or ():
            if c < start:
                continue
            out.append(c - start)
            piece = ParseCtx(self.t[start:c].tobytes(), False)
            if len(piece.bad):
                break
            start += int(piece.le[4 * piece.n_reads - 1]) + 1 if piece.n_reads else 0
        return np.asarray(out, np.int64)


def _line_kind(kind):
    return slice({"def": 0, "base": 1, "qual": 3}[kind], None, 4)


def _cr_at(kind, P):
    def pred(c):
        s, e, f = c.ls[_line_kind(kind)], c.le[_line_kind(kind)], c.first_cr[_line_kind(kind)]
        inside = f < e
        return bool((inside & ((f == e - 1) if P == "last" else (f - s == P))).any())
    return pred


def _cr_behind_end(c):
    for kind in ("base", "qual"):
        e, f = c.le[_line_kind(kind)], c.first_cr[_line_kind(kind)]
        if ((f > e) & (f <= e + 15)).any():
            return True
    return False


def _empty_line_cr_behind(c):
    for kind in ("base", "qual"):
        s, e = c.ls[_line_kind(kind)], c.le[_line_kind(kind)]
        m = (s == e) & (e + 1 < c.n_text)
        if m.any() and (c.t[np.minimum(e[m] + 1, c.n_text - 1)] == 13).any():
            return True
    return False


def _line_spans_three_tiles(c):
    return bool(len(c.ls) and (c.le // TEXT_TILE - c.ls // TEXT_TILE >= 2).any())


def _two_bad_lower_slot(c):
    if len(c.bad) < 2:
        return False
    t = c.bad // REC_TILE
    return bool(((t[1:] > t[0]) & (t[1:] % SCAN_THREADS < t[0] % SCAN_THREADS)).any())


def _framed(pred):
    return lambda c: pred(c) and c.t[0] == 64 and c.n_reads >= 2 and c.slen[0] > 0 and c.slen[c.n_reads - 1] > 0


def _sat(which):
    def pred(c):
        full = np.arange(c.n_tiles) < c.n_text // TEXT_TILE
        if which == "nl":
            return bool((full & (c.tile_nl == TEXT_TILE)).any())
        if which == "cr":
            return bool((full & (c.tile_cr == TEXT_TILE)).any())
        return bool((full & (c.tile_nl == TEXT_TILE // 2) & (c.tile_cr == TEXT_TILE // 2)).any())
    return pred


def _with_final(pred, final):
    return lambda c: c.final == final and pred(c)


def _parse_edges():
    E = {}
    for k in (1, 2, 64):
        for d in (-1, 0, 1):
            E["n_text=%d" % (16 * k + d)] = lambda c, v=16 * k + d: c.n_text == v
    for k in (1, 2):
        for d in (-1, 0, 1):
            E["n_text=%d" % (TEXT_TILE * k + d)] = lambda c, v=TEXT_TILE * k + d: c.n_text == v
    for r in range(1, 16):  # valid_mask: the last piece holds r bytes, the last of them a '\n' (and the padding behind it is hostile)
        E["tail_bytes=%d" % r] = lambda c, r=r: c.n_text % PIECE == r and not c.open
    E["nl_last_byte_of_tile"] = lambda c: bool((c.nl % TEXT_TILE == TEXT_TILE - 1).any())
    E["nl_first_byte_of_tile"] = lambda c: bool(((c.nl % TEXT_TILE == 0) & (c.nl > 0)).any())
    E["crlf_split_at_tile_edge"] = lambda c: bool(np.isin(c.cr[c.cr % TEXT_TILE == TEXT_TILE - 1] + 1, c.nl).any())
    E["crlf_split_at_piece_edge"] = lambda c: bool(np.isin(c.cr[c.cr % PIECE == PIECE - 1] + 1, c.nl).any())
    E["line_spans_three_tiles"] = _line_spans_three_tiles
    for which in ("nl", "cr", "crlf"):
        for final in (True, False):
            E["saturated_%s/%s" % (which, "final" if final else "open")] = _with_final(_sat(which), final)
            E["saturated_%s_framed/%s" % (which, "final" if final else "open")] = _with_final(_framed(_sat(which)), final)
    for kind in ("base", "qual", "def"):
        for P in (0, 1, 15, 16, 17, 31, 32, "last"):
            E["first_cr_of_%s_line_at_%s" % (kind, P)] = _cr_at(kind, P)
    E["cr_within_15_behind_a_line_without"] = _cr_behind_end
    E["empty_line_cr_right_behind"] = _empty_line_cr_behind
    E["has_cr_from_last_tile_only"] = lambda c: c.n_tiles >= 2 and len(c.cr) > 0 and bool((c.cr // TEXT_TILE == c.n_tiles - 1).all())
    E["has_cr_from_defline_only"] = lambda c: len(c.cr) > 0 and len(c.ls) > 0 and bool(np.isin(np.searchsorted(c.ls, c.cr, side="right") - 1, np.arange(0, len(c.ls), 4)).all()) and bool((c.cr < c.le[-1]).all())
    for K in (0, 255, 256, 257, 511):
        E["first_bad_record=%d" % K] = lambda c, K=K: len(c.bad) > 0 and c.n_reads == K
    E["later_bad_in_lower_scan_slot"] = _two_bad_lower_slot
    for T in TAILS:
        E["bad_last_candidate_tail_" + T] = lambda c, T=T: c.final and len(c.bad) > 0 and c.n_reads == c.n_cand - 1 and c.tail() == T
    E["first_bad_beyond_scan_round"] = lambda c: len(c.bad) >= 2 and c.n_reads > SCAN_THREADS * REC_TILE and c.bad[1] - c.bad[0] <= 200
    E["rec_tiles_beyond_grid"] = lambda c: c.n_cand > DEFAULT_CU * GRID_BLOCKS_PER_CU * REC_TILE
    E["first_bad_in_second_stride"] = lambda c: len(c.bad) > 0 and c.n_reads // REC_TILE >= DEFAULT_CU * GRID_BLOCKS_PER_CU
    E["grid_stride_clean"] = lambda c: c.n_cand > DEFAULT_CU * GRID_BLOCKS_PER_CU * REC_TILE and len(c.bad) == 0
    E["ragged_beyond_1024_text_tiles"] = lambda c: (c.n_tiles > SCAN_THREADS and len(np.unique(c.tile_nl[:SCAN_THREADS])) > 8 and len(np.unique(c.tile_nl[SCAN_THREADS:-1])) > 1
                                                     and bool(np.isin(c.cr + 1, c.nl).any()) and not bool(np.isin(c.cr + 1, c.nl).all()))
    for d in (-1, 0, 1):
        E["chunk_length=tile%+d" % d] = lambda c, d=d: c.cuts is not None and bool(((c.chunk_lengths() - d) % TEXT_TILE == 0).any())
        E["chunk_length=piece%+d" % d] = lambda c, d=d: c.cuts is not None and bool((((c.chunk_lengths() - d) % PIECE == 0) & ((c.chunk_lengths() - d) % TEXT_TILE != 0)).any())
    return E


def _chunk_cuts(text, lengths):
    """Cuts such that the pieces a chunked feed hands over have these lengths."""
    cuts, start = [], 0
    for L in lengths:
        c = start + L
        assert c < len(text)
        cuts.append(c)
        piece = ParseCtx(text[start:c], False)
        assert not len(piece.bad) and piece.n_reads
        start += int(piece.le[4 * piece.n_reads - 1]) + 1
    return cuts


def _bad_text(n, bad, tail="clean", k_cycle=10):
    """n records of 0 .. k_cycle - 1 bases, those of `bad` with a quality byte too many, and a tail."""
    recs = [record(k, (k * 7) % k_cycle, qual_extra=b"I" if k in bad else b"") for k in range(n)]
    if tail == "clean_open":
        recs[-1] = recs[-1][:-1]
    return b"".join(recs) + _TAIL_TEXT[tail]


def parse_cases(n_cu=DEFAULT_CU):
    """The parse texts.  n_cu: the compute units of the device the grid-stride cases are sized for."""
    C = []
    add = lambda *a, **kw: C.append(ParseCase(*a, **kw))
    # -- text sizes, every tail of the last piece
    for n in [16 * k + d for k in (1, 2, 64) for d in (-1, 0, 1)] + [TEXT_TILE * k + d for k in (1, 2) for d in (-1, 0, 1)] + [48 + r for r in range(2, 15)]:
        add("size_%d" % n, sized_text(n, k0=n), ["n_text=%d" % n] * (n < 48 or n > 62) + (["tail_bytes=%d" % (n % 16)] if n % 16 else []))
    # -- '\n' and "\r\n" at tile and piece edges, a line over three tiles
    add("nl_at_tile_edge", sized_text(TEXT_TILE - 4) + b"@ab\n\n+\n\n" + sized_text(500, 900), ["nl_last_byte_of_tile", "nl_first_byte_of_tile"])
    add("crlf_across_tile_edge", sized_text(TEXT_TILE - 4, eol=b"\r\n") + record(1, 9, b"\r\n", defline=b"@ab") + sized_text(300, 7, b"\r\n"),
        ["crlf_split_at_tile_edge", "first_cr_of_base_line_at_last", "first_cr_of_qual_line_at_last", "first_cr_of_def_line_at_last"])
    add("crlf_across_piece_edge", sized_text(16 * 5 + 12) + record(1, 9, b"\r\n", defline=b"@ab") + sized_text(100, 7), ["crlf_split_at_piece_edge"])
    add("line_over_three_tiles", sized_text(100) + record(5, 40000) + sized_text(77, 3), ["line_spans_three_tiles"])
    # -- saturated tiles
    front, behind = record(0, 4, defline=b"@a"), record(1, 5, defline=b"@b")
    for which, fill in (("nl", b"\n" * (3 * TEXT_TILE)), ("cr", b"\r" * (3 * TEXT_TILE)), ("crlf", b"\r\n" * (3 * TEXT_TILE // 2))):
        add("saturated_" + which, fill, ["saturated_%s/final" % which, "saturated_%s/open" % which])
        add("saturated_%s_framed" % which, front + fill + behind, ["saturated_%s_framed/final" % which, "saturated_%s_framed/open" % which])
    # -- content_len: the first '\r' of a line at the positions where its 16-byte steps turn
    for kind in ("base", "def"):
        recs = []
        for k, P in enumerate((0, 1, 15, 16, 17, 31, 32)):
            recs.append(record(k, 40, cr_at=P) if kind == "base" else record(k, 33, defline=b"@" + b"d" * (P - 1) + b"\rjunk" if P else b"\r@junk"))
            recs.append(record(100 + k, 3 + k))
        add("cr_positions_" + kind, b"".join(recs), ["first_cr_of_%s_line_at_%s" % (kk, P) for kk in (("base", "qual") if kind == "base" else ("def",)) for P in (0, 1, 15, 16, 17, 31, 32)]
            + (["has_cr_from_defline_only"] if kind == "def" else []))
    add("cr_behind_line_end", b"".join(b"@d%d\n" % L + bases(L, L).tobytes() + b"\n+\rjunk\n" + quals(L, L).tobytes() + b"\n@x\rjunk\n" + bases(L + 1, 3).tobytes() + b"\n+\n" + quals(L + 1, 3).tobytes() + b"\n"
                                        for L in (1, 2, 14, 15, 16, 17, 30, 31, 32, 33, 48)), ["cr_within_15_behind_a_line_without"])
    add("empty_lines_cr_behind", b"@e\n\n\r+junk\n\n\r@f\nAC\n+\nII\n" * 3 + b"@g\n\n\r\n\n", ["empty_line_cr_right_behind"])
    add("cr_in_last_tile_only", sized_text(2 * TEXT_TILE + 100) + b"@z\r\nACGT\rTT\r\n+\r\n" + b"IIII\rJJJ\r\n" + record(9, 5), ["has_cr_from_last_tile_only"])
    # -- record tiles: the first bad record
    for K in (0, 255, 256, 257, 511):
        add("bad_at_%d" % K, _bad_text(600, {K, K + 50}), ["first_bad_record=%d" % K])
    for T in TAILS:
        add("bad_last_tail_" + T, _bad_text(300, {299}, T), ["bad_last_candidate_tail_" + T], finals=(True, False))
    round_recs = SCAN_THREADS * REC_TILE
    add("bad_beyond_scan_round", tiny_records(round_recs + 1000, {round_recs + 300, round_recs + 400})[0], ["first_bad_beyond_scan_round"], finals=(True,))
    add("bad_in_lower_scan_slot", tiny_records(round_recs + 1000, {5 * REC_TILE + 7, (SCAN_THREADS + 2) * REC_TILE + 3})[0], ["later_bad_in_lower_scan_slot"], finals=(False,))
    grid_recs = n_cu * GRID_BLOCKS_PER_CU * REC_TILE
    add("grid_stride_bad", tiny_records(grid_recs + 300 * REC_TILE, {grid_recs + 37 * REC_TILE + 11})[0], ["rec_tiles_beyond_grid", "first_bad_in_second_stride"], finals=(False,))
    add("grid_stride_clean", tiny_records(grid_recs + 777)[0], ["rec_tiles_beyond_grid", "grid_stride_clean"], finals=(True,))
    # -- more than 1024 ragged text tiles
    pattern = (0, 1, 150, 37, 16, 15, 17, 250, 3, 1000, 64, 2, 151, 5000, 9, 33, 0, 0, 7, 301)
    recs = [record(k, L, b"\r\n" if k % 3 == 1 else b"\n", cr_at=(L // 2 if k % 5 == 2 else None)) for k, L in enumerate(pattern)]
    body = [b"".join(recs[:len(recs) - v]) for v in range(3)]  # (a block drops its last 0, 1 or 2 records: no two tiles alike)
    blocks, size, r = [], 0, 0
    while size <= (SCAN_THREADS + 3) * TEXT_TILE:
        blocks.append(b"@block%06d\n\n+\n\n" % r + body[r % 3])
        size += len(blocks[-1])
        r += 1
    add("ragged_16MiB", b"".join(blocks), ["ragged_beyond_1024_text_tiles"], finals=(True,))
    # -- chunked feed
    for eol, nm in ((b"\n", "lf"), (b"\r\n", "crlf")):
        text = b"".join(record(k, 20 + (k * 13) % 90, eol) for k in range(700))
        lengths = [TEXT_TILE - 1, TEXT_TILE, TEXT_TILE + 1, 16 * 40 - 1, 16 * 40, 16 * 40 + 1]
        add("chunked_" + nm, text, ["chunk_length=tile%+d" % d for d in (-1, 0, 1)] + ["chunk_length=piece%+d" % d for d in (-1, 0, 1)], finals=(True,), cuts=_chunk_cuts(text, lengths))
    return C


# =====================================================================================================================================
# gather layouts: the sizes of the records of an output, by which offset[] lands on the edges of the piece walker
# =====================================================================================================================================

class Layout:
    def __init__(self, name, sizes, claims, kinds=("parse", "emit", "render")):
        self.name, self.sizes, self.claims, self.kinds = name, np.asarray(sizes, np.int64), tuple(claims), kinds
        self.offset = np.concatenate([[0], np.cumsum(self.sizes)])
        assert (self.sizes >= (5 if "render" in kinds else 0)).all(), name


def _ends(ends):
    return np.diff(np.concatenate([[0], np.asarray(ends, np.int64)]))


def _interior(off):
    return off[(off > 0) & (off < off[-1])]


def _count_in(off, lo, hi):
    """how many of offset[1 ..] lie in (lo, hi]  (lo, hi: numbers or arrays)"""
    o = off[1:]
    return np.searchsorted(o, hi, side="right") - np.searchsorted(o, lo, side="right")


def _ends_in_kib(C, where):
    def pred(off):
        per_span = SPAN_BYTES // WAVE_BYTES
        ow = np.arange(0 if where == "first" else per_span - 1, (int(off[-1]) + WAVE_BYTES - 1) // WAVE_BYTES, per_span, dtype=np.int64) * WAVE_BYTES
        # The wave counts, per lane, the offsets behind kw that are <= the lane's position; lane 63 stands at ow + 1008, so the ends in
        # (ow, ow + 1008] decide between the 6-step search (up to 63) and the lane's own (64 and more).  That reading needs kw to be exact,
        # offset[kw] <= ow < offset[kw + 1]: at a span start the binary search makes it so, inside a span the wave carries the record under
        # the last byte it wrote, which is the same unless empty records sit AT ow (they are behind kw then and counted on top).  So the
        # predicate for the last KiB of a span asks for a non-empty record ACROSS ow as well.
        straddled = np.ones(len(ow), bool) if where == "first" else np.array([_one_record_covers(off, int(o) - 1, int(o) + 1) for o in ow], bool)
        ok = (_count_in(off, ow, ow + WAVE_BYTES - PIECE) == C) & (_count_in(off, ow, ow + WAVE_BYTES) == C) & straddled
        return any(_one_record_covers(off, int(o) + WAVE_BYTES, int(o) + 2 * WAVE_BYTES) for o in ow[ok])
    return pred


def _one_record_covers(off, lo, hi):
    k = int(np.searchsorted(off, lo, side="right")) - 1
    return 0 <= k < len(off) - 1 and off[k + 1] >= hi and off[k + 1] > off[k]


def _empty_runs(off):
    """(position, length, first record) of the maximal runs of empty records, as arrays"""
    z = np.concatenate([[0], (np.diff(off) == 0).astype(np.int8), [0]])
    d = np.diff(z)
    a, b = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    return off[a], b - a, a


def _empty_run(E, place):
    def pred(off):
        p, n, k = _empty_runs(off)
        at = {"start": k == 0, "span": (p > 0) & (p % SPAN_BYTES == 0), "kib": (p % WAVE_BYTES == 0) & (p % SPAN_BYTES != 0), "inside_piece": p % PIECE != 0}[place]
        return bool(((n == E) & (p < off[-1]) & at).any())
    return pred


def _covers_spans(off):
    sizes = np.diff(off)
    for k in np.nonzero(sizes >= 2 * SPAN_BYTES)[0]:
        if (off[k + 1] // SPAN_BYTES - (off[k] + SPAN_BYTES - 1) // SPAN_BYTES) >= 1 and 0 < k < len(sizes) - 1 and 0 < sizes[k - 1] <= 5 and 0 < sizes[k + 1] <= 5:
            return True
    return False


EMPTY_RUNS = (1, 63, 64, 65, 300)
CROWDS = (62, 63, 64, 65, 200)
N_BYTES = (1, 15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193)
NO_RENDER = ("parse", "emit")  # a rendered record has at least 5 bytes: no empty record, no output of one byte


def _gather_edges():
    """{edge: (predicate over offset[], kinds it has to be reached for)}"""
    E, ALL = {}, ("parse", "emit", "render")
    for r in (0, 1, 15):
        E["record_end_mod_16=%d" % r] = (lambda off, r=r: bool((_interior(off) % PIECE == r).any()), ALL)
    for unit, nm in ((WAVE_BYTES, "KiB"), (SPAN_BYTES, "span")):
        for d in (-1, 0, 1):
            E["record_end=%s%+d" % (nm, d)] = (lambda off, u=unit, d=d: bool(((_interior(off) - d) % u == 0).any()), ALL)
    for v in N_BYTES:
        E["n_bytes=%d" % v] = (lambda off, v=v: int(off[-1]) == v, NO_RENDER if v < 5 else ALL)
    for Cn in CROWDS:
        for where in ("first", "last"):
            E["%d_ends_in_%s_KiB_of_span" % (Cn, where)] = (_ends_in_kib(Cn, where), ALL)
    for En in EMPTY_RUNS:
        for place in ("start", "span", "kib", "inside_piece"):
            E["%d_empty_at_%s" % (En, place)] = (_empty_run(En, place), NO_RENDER)
    E["last_record_empty"] = (lambda off: len(off) > 2 and off[-1] == off[-2] and off[-1] > 0, NO_RENDER)
    E["all_but_one_empty"] = (lambda off: len(off) > 3 and int((np.diff(off) > 0).sum()) == 1, NO_RENDER)
    E["record_covers_spans"] = (_covers_spans, ALL)
    return E


def _split(total, lo=5):
    """total bytes as records of lo .. lo + 6 bytes (one record when total < 2 lo)"""
    out, k = [], 0
    while total >= 2 * lo + 6:
        s = lo + (k * 5) % 7
        out.append(s)
        total -= s
        k += 1
    return out + ([total] if total else [])


def layouts():
    L = []
    L.append(Layout("ends_mod_16", _ends([16, 33, 63, 80, 97, 127, 150]), ["record_end_mod_16=%d" % r for r in (0, 1, 15)]))
    L.append(Layout("ends_at_KiB", _ends([1023, 2048, 3073, 4091, 4096, 4101, 5000]), ["record_end=KiB%+d" % d for d in (-1, 0, 1)]))
    L.append(Layout("ends_at_span", _ends([8191, 16384, 24577, 32763, 32768, 32773, 33000]), ["record_end=span%+d" % d for d in (-1, 0, 1)]))
    L.append(Layout("ends_around_span", _ends([5, 8191 - 5, 8191, 8192 + 5, 16384 - 5, 16384, 16384 + 7, 24577 - 6, 24577, 24600]), ["record_end=span%+d" % d for d in (-1, 0, 1)]))
    for v in N_BYTES:
        L.append(Layout("n_bytes_%d" % v, _split(v), ["n_bytes=%d" % v], NO_RENDER if v < 5 else ("parse", "emit", "render")))
    for Cn in CROWDS:
        # the first KiB of span 0 holds Cn ends, one record covers the KiB behind it (the wave's carried record index has to hold there)
        L.append(Layout("crowd_%d_first" % Cn, [5] * Cn + [3000 - 5 * Cn, 7, 9, 40], ["%d_ends_in_first_KiB_of_span" % Cn]))
        # the last KiB of span 0 holds Cn ends (the first of a record that straddles its start), one record covers the first KiB of span 1
        L.append(Layout("crowd_%d_last" % Cn, [3000, 4165] + [5] * Cn + [9300 - 7165 - 5 * Cn, 6, 11], ["%d_ends_in_last_KiB_of_span" % Cn]))
    for En in EMPTY_RUNS:
        L.append(Layout("empty_%d_at_start" % En, [0] * En + [20, 30, 7], ["%d_empty_at_start" % En], NO_RENDER))
    for place, at in (("span", lambda i: SPAN_BYTES * (i + 1)), ("kib", lambda i: SPAN_BYTES * i + WAVE_BYTES * (i + 1)), ("inside_piece", lambda i: SPAN_BYTES * i + 2 * WAVE_BYTES + 16 * i + 5)):
        sizes, pos = [], 0
        for i, En in enumerate(EMPTY_RUNS):
            sizes += [at(i) - pos - 9, 9] + [0] * En
            pos = at(i)
        L.append(Layout("empty_runs_at_" + place, sizes + [33, 1], ["%d_empty_at_%s" % (En, place) for En in EMPTY_RUNS], NO_RENDER))
    L.append(Layout("last_record_empty", [10, 20, 0], ["last_record_empty"], NO_RENDER))
    L.append(Layout("all_but_one_empty", [0] * 70 + [37] + [0] * 70, ["all_but_one_empty"], NO_RENDER))
    L.append(Layout("record_over_spans_1", [1, 20000, 1, 3], ["record_covers_spans"], NO_RENDER))
    L.append(Layout("record_over_spans_5", [5, 20000, 5, 8], ["record_covers_spans"]))
    return L


def layout_text(lay):
    """A FASTQ text whose parse has the layout's offsets."""
    return b"".join(record(k, int(s), defline=b"@%d" % k if k % 3 else b"") for k, s in enumerate(lay.sizes))


# =====================================================================================================================================
# batches for the emit / render scan and their gathers
# =====================================================================================================================================

class Batch:
    """Reads in arenas (64 readable bytes either side), per-read results, keep / select, order, and a text that holds the deflines.  Has
    the attributes render_cases.render_host and the device helpers of the GPU tests take of a render_cases.Case."""

    def __init__(self, kind, name, claims, lens, start, wlen, valid, select=None, order=None, def_len=None, n_lead=None, n_trail=None):
        self.kind, self.name, self.claims = kind, name, tuple(claims)
        lens = np.asarray(lens, np.int64)
        self.n = n = len(lens)
        self.offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        self.total = total = int(self.offset[-1])
        s, q = np.zeros(64 + total + 64, np.uint8), np.zeros(64 + total + 64, np.uint8)
        s[64:64 + total], q[64:64 + total] = bases(total, n), quals(total, n)
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
        res = np.zeros(n, RESULT_DTYPE)
        res["start"], res["len"], res["flags"] = start, wlen, np.asarray(valid, np.int64) * F_VALID | ((np.arange(n) % 8) << 4)  # (the other flag bits are noise)
        assert (res["start"].astype(np.int64) + res["len"] <= lens).all()
        self.res = res
        self.select = None if select is None else np.asarray(select, np.uint8)
        self.keep = self.select
        self.order = None if order is None else np.asarray(order, np.uint32)
        self.def_len = np.zeros(n, np.uint32) if def_len is None else np.asarray(def_len, np.uint32)
        dl = self.def_len.astype(np.int64)
        self.def_pos = (np.concatenate([[0], np.cumsum(dl + 1)])[:n]).astype(np.uint32)
        text = np.full(int((dl + 1).sum()), 10, np.uint8)
        inside = np.ones(len(text), bool)
        inside[(self.def_pos.astype(np.int64) + dl)] = False
        text[inside] = 33 + (np.arange(int(inside.sum())) * 7) % 90
        self.text = text
        if n:
            nz = lens > 0
            first = s[64 + np.minimum(off[:-1], max(total - 1, 0))] == 78
            last = s[64 + np.maximum(off[1:] - 1, 0)] == 78
            self.tn = ((first & nz).astype(np.uint8) | ((last & nz).astype(np.uint8) << 1))
        else:
            self.tn = np.zeros(0, np.uint8)
        self.lens = lens

    @property
    def render_capacity(self):
        """bytes no rendering of the batch exceeds (the text here holds the deflines alone)"""
        return len(self.text) + 2 * self.total + 5 * self.n

    def scan_ctx(self, with_res=True):
        """(per candidate, in candidate order): rendered / emitted?, and the offsets of the output."""
        n = self.n
        cand = np.arange(n, dtype=np.int64) if self.order is None else self.order.astype(np.int64)
        ok = cand < n
        ci = np.where(ok, cand, 0)
        if self.select is not None:
            ok &= self.select[ci] != 0
        if with_res:
            ok &= (self.res["flags"][ci] & F_VALID) != 0
        wl = self.res["len"][ci].astype(np.int64) if with_res else self.lens[ci]
        size = wl if self.kind == "emit" else self.def_len[ci].astype(np.int64) + 2 * wl + 5
        return ScanCtx(self, ok, np.concatenate([[0], np.cumsum(size[ok])]), ci[ok])


class ScanCtx:
    def __init__(self, batch, sel, offset, index):
        self.b, self.sel, self.offset, self.index, self.n = batch, sel, offset, index, batch.n
        nt = (self.n + TILE_ITEMS - 1) // TILE_ITEMS
        pad = np.zeros(nt * TILE_ITEMS, bool)
        pad[:self.n] = sel
        self.tiles = pad.reshape(nt, TILE_ITEMS)
        self.tile_recs = self.tiles.sum(1)
        # the terminal 'N' runs of the emitted reads and where their windows lie
        b = batch
        self.lead, self.trail = [], []  # (run length, read length, start, len)
        for i in index[(b.tn[index] != 0)] if len(index) else ():
            a, e = int(b.offset[i]), int(b.offset[i + 1])
            r = b.seq[a:e]
            nn = np.nonzero(r != 78)[0]
            lead = int(nn[0]) if len(nn) else e - a
            trail = (e - a - 1 - int(nn[-1])) if len(nn) else e - a
            st, ln = int(b.res["start"][i]), int(b.res["len"][i])
            if lead:
                self.lead.append((lead, e - a, st, ln))
            if trail:
                self.trail.append((trail, e - a, st, ln))


def _window(run, side, rel):
    def pred(c):
        for r, L, st, ln in (c.lead if side == "lead" else c.trail):
            if r != run or r == L or ln == 0:
                continue
            lo, hi = (0, r) if side == "lead" else (L - r, L)  # the run
            if {"inside": lo <= st and st + ln <= hi, "straddles": (st < hi < st + ln) if side == "lead" else (st < lo < st + ln),
                "apart": (st >= hi) if side == "lead" else (st + ln <= lo)}[rel]:
                return True
        return False
    return pred


def _scan_edges():
    E = {}
    for v in (1023, 1024, 1025, 2047, 2048, 2049):
        E["n_reads=%d" % v] = lambda c, v=v: c.n == v
    E["tile_all_dropped"] = lambda c: len(c.tile_recs) >= 3 and bool(((c.tile_recs[1:-1] == 0) & (c.tile_recs[:-2] > 0) & (c.tile_recs[2:] > 0)).any())
    E["only_last_of_tile_then_only_first_of_next"] = lambda c: any(c.tile_recs[t] == 1 and c.tiles[t, -1] and c.tile_recs[t + 1] == 1 and c.tiles[t + 1, 0] for t in range(len(c.tile_recs) - 1))
    E["tiles_alternate_all_and_none"] = lambda c: len(c.tile_recs) >= 4 and all(c.tile_recs[t] == (TILE_ITEMS if t % 2 == 0 else 0) for t in range(4))
    E["scan_carries_into_second_round"] = lambda c: (c.n >= SCAN_THREADS * TILE_ITEMS + 1500 and len(np.unique(c.tile_recs[:SCAN_THREADS])) > 8 and len(np.unique(c.tile_recs[SCAN_THREADS:])) > 1
                                                      and len(np.unique(np.add.reduceat(np.diff(c.offset), np.concatenate([[0], np.cumsum(c.tile_recs)[:-1]]).clip(max=len(c.offset) - 2)))) > 8)
    for r in (1, 63, 64, 65, 128):
        for side in ("lead", "trail"):
            for rel in ("inside", "straddles", "apart"):
                if r == 1 and rel == "straddles":
                    continue  # (a window cannot hold a part of one base)
                E["%s_N_run_%d_window_%s" % (side, r, rel)] = _window(r, side, rel)
    E["whole_read_N"] = lambda c: any(r == L and ln > 0 for r, L, st, ln in c.lead)
    return E


def _order_edges():
    """Edges of the render scan's order[] (candidate j renders read order[j]; an entry that names no read is skipped).  Render alone takes one."""
    E = {}
    tile = lambda c: np.arange(c.n) // TILE_ITEMS
    given = lambda c: c.b.order is not None
    hole = lambda c: c.b.order >= c.n
    E["order_moves_reads_across_tiles"] = lambda c: given(c) and not hole(c).any() and len(np.unique(c.b.order)) == c.n and bool(((c.b.order // TILE_ITEMS != tile(c)) & c.sel).any())
    E["order_holes_n_and_2_32-1_and_between"] = lambda c: given(c) and all(bool(m.any()) for m in (c.b.order == c.n, c.b.order == 0xFFFFFFFF, (c.b.order > c.n) & (c.b.order < 0xFFFFFFFF)))
    E["order_hole_last_of_tile_or_first_of_next"] = lambda c: given(c) and bool((hole(c)[TILE_ITEMS - 1::TILE_ITEMS]).any()) and bool((hole(c)[TILE_ITEMS::TILE_ITEMS]).any())
    E["order_tile_of_holes_alone"] = lambda c: given(c) and any(bool(hole(c)[t * TILE_ITEMS:(t + 1) * TILE_ITEMS].all()) for t in range(c.n // TILE_ITEMS))
    E["order_holes_beyond_first_scan_round"] = lambda c: given(c) and bool(hole(c)[SCAN_THREADS * TILE_ITEMS:].any()) and bool((~hole(c))[SCAN_THREADS * TILE_ITEMS:].any())
    return E


def _coprime_step(n, start):
    a = start
    while np.gcd(a, n) != 1:
        a += 1
    return a


def ordered(b, name, claims, holes=None):
    """Batch b rendered through an order: candidate j renders read (a j + 7) mod n, and read (a j + 7) mod n takes what read j has in b, so the
    candidates -- and with them the tile pattern of the scan -- are those of b while the reads lie scattered over the arenas.  holes: a mask
    over the candidates whose entry of order[] is to name no read (n, 2^32 - 1 and values between, in turn)."""
    n = b.n
    j = np.arange(n, dtype=np.int64)
    perm = (_coprime_step(n, 1001) * j + 7) % n
    to_read = lambda a: None if a is None else _scatter(np.asarray(a), perm)
    order = perm.copy()
    if holes is not None:
        at = np.nonzero(holes)[0]
        order[at] = np.choose(np.arange(len(at)) % 3, [n, 0xFFFFFFFF, n + 1 + (at * 7919) % (0xFFFFFFFE - n)])
    lead = np.minimum(_lead_n(b), b.lens)
    out = Batch(b.kind, name, claims, to_read(b.lens), to_read(b.res["start"]), to_read(b.res["len"]), to_read(b.res["flags"] & F_VALID), to_read(b.select), order,
                to_read(b.def_len), n_lead=to_read(lead))
    assert (out.tn[perm] == b.tn).all(), name  # (the leading 'N' runs came along; b has no trailing ones of their own)
    return out


def _scatter(a, perm):
    out = np.empty_like(a)
    out[perm] = a
    return out


def _lead_n(b):
    """the leading 'N' run of every read of b that begins with one (0 elsewhere): what Batch() takes as n_lead"""
    out = np.zeros(b.n, np.int64)
    for i in np.nonzero(b.tn & 1)[0]:
        r = b.seq[int(b.offset[i]):int(b.offset[i + 1])]
        nn = np.nonzero(r != 78)[0]
        out[i] = int(nn[0]) if len(nn) else len(r)
    return out


def _render_split(size):
    """(defline length, window length) of a rendered record of `size` bytes: size = def_len + 2 len + 5"""
    ln = (size - 5) // 2
    if ln > 3 and size % 3 == 0:
        ln -= 3  # (a defline of 6 or 7 bytes now and then)
    return size - 5 - 2 * ln, ln


def batch_cases(kind):
    """kind: 'emit' (a record of the output is a kept window) or 'render' (defline, window twice and five bytes)."""
    assert kind in ("emit", "render")
    C = []
    # -- the gather layouts: every record's window lies inside a read that is a few bases longer; a dropped read now and then
    for lay in layouts():
        if kind not in lay.kinds:
            continue
        lens, start, wlen, valid, dlen = [], [], [], [], []
        for k, s in enumerate(lay.sizes.tolist()):
            d, w = (0, s) if kind == "emit" else _render_split(s)
            if k % 4 == 2:
                lens.append(k % 9), start.append(0), wlen.append(k % 9), valid.append(0), dlen.append(3)
            st = (k * 3) % 5
            lens.append(min(w + st + k % 3, 32767) if w + st <= 32767 else w), start.append(st if w + st <= 32767 else 0), wlen.append(w), valid.append(1), dlen.append(d)
        C.append(Batch(kind, "layout_" + lay.name, lay.claims, lens, start, wlen, valid, def_len=dlen))
    # -- the scan: read counts either side of a tile, tile patterns
    for n in (1023, 1024, 1025, 2047, 2048, 2049):
        k = np.arange(n)
        lens = (k * 7) % 11
        C.append(Batch(kind, "n_reads_%d" % n, ["n_reads=%d" % n], lens, lens // 3, lens - lens // 3 - (lens > 5), (k * 5) % 7 != 0, select=(k * 3) % 5 != 1, def_len=k % 4))
    k = np.arange(3 * TILE_ITEMS + 10)
    lens = (k * 5) % 9
    C.append(Batch(kind, "tile_all_dropped", ["tile_all_dropped"], lens, 0 * k, lens, (k // TILE_ITEMS != 1) & (k % 3 != 0), def_len=k % 3))
    C.append(Batch(kind, "last_of_tile_first_of_next", ["only_last_of_tile_then_only_first_of_next"], lens, 0 * k, lens,
                   (k == TILE_ITEMS - 1) | (k == TILE_ITEMS) | ((k >= 2 * TILE_ITEMS) & (k % 2 == 0)), def_len=k % 3))
    if kind == "render":
        # the same patterns over the CANDIDATES of an order: a permutation; then holes that do the dropping where the flags did it above
        C.append(ordered(C[-2], "tile_all_dropped_permuted", ["tile_all_dropped", "order_moves_reads_across_tiles"]))
        C.append(ordered(C[-2], "last_of_tile_first_of_next_permuted", ["only_last_of_tile_then_only_first_of_next", "order_moves_reads_across_tiles"]))
        every = Batch(kind, "", (), lens, 0 * k, lens, k % 3 != 0, def_len=k % 3)
        C.append(ordered(every, "tile_all_dropped_holes", ["tile_all_dropped", "order_tile_of_holes_alone", "order_holes_n_and_2_32-1_and_between"], holes=(k // TILE_ITEMS == 1) | (k % 7 == 2)))
        every = Batch(kind, "", (), lens, 0 * k, lens, 1 + 0 * k, def_len=k % 3)
        C.append(ordered(every, "last_of_tile_first_of_next_holes", ["only_last_of_tile_then_only_first_of_next", "order_holes_n_and_2_32-1_and_between"],
                         holes=~((k == TILE_ITEMS - 1) | (k == TILE_ITEMS) | ((k >= 2 * TILE_ITEMS) & (k % 2 == 0)))))
    k = np.arange(5 * TILE_ITEMS)
    lens = 1 + (k * 5) % 9
    C.append(Batch(kind, "tiles_alternate", ["tiles_alternate_all_and_none"], lens, 0 * k, lens, 1 + 0 * k, select=(k // TILE_ITEMS) % 2 == 0, def_len=k % 2))
    if kind == "render":
        C.append(ordered(C[-1], "tiles_alternate_permuted", ["tiles_alternate_all_and_none", "order_moves_reads_across_tiles"]))
        every = Batch(kind, "", (), lens, 0 * k, lens, 1 + 0 * k, select=k // TILE_ITEMS != 3, def_len=k % 2)
        C.append(ordered(every, "tiles_alternate_holes", ["tiles_alternate_all_and_none", "order_tile_of_holes_alone", "order_holes_n_and_2_32-1_and_between"], holes=k // TILE_ITEMS == 1))
    n = SCAN_THREADS * TILE_ITEMS + 1500
    k = np.arange(n, dtype=np.int64)
    h = (k * 2654435761 + (k >> 5) * 40503) >> 7
    lens = h % 4
    C.append(Batch(kind, "scan_second_round", ["scan_carries_into_second_round"], lens, (lens > 2).astype(np.int64), lens - (lens > 2), (h >> 3) % 3 != 0,
                   select=((h >> 6) % 5 != 0) & ((k >> 9) % 7 != 3), def_len=(h >> 9) % 2, n_lead=(k % 1009 == 5) * np.minimum(lens, 2)))
    if kind == "render":
        C.append(ordered(C[-1], "scan_second_round_permuted", ["scan_carries_into_second_round", "order_moves_reads_across_tiles"]))
        C.append(ordered(C[-2], "scan_second_round_holes", ["scan_carries_into_second_round", "order_holes_beyond_first_scan_round", "order_holes_n_and_2_32-1_and_between",
                                                             "order_hole_last_of_tile_or_first_of_next"], holes=((h >> 4) % 11 == 0) | (k % (3 * TILE_ITEMS) == TILE_ITEMS - 1) | (k % (5 * TILE_ITEMS) == 0)))
    # -- terminal 'N' runs: a read is  N x run + 100 bases  (or the other way round); windows inside the run, across its end, apart from it
    lens, start, wlen, lead, trail = [], [], [], [], []
    for r in (1, 63, 64, 65, 128):
        L = r + 100
        for front in (True, False):
            ws = [(0, r), (r, 50), (r + 1, 20)] + ([(0, r + 10), (r - 1, 2), (1, r - 1)] if r > 1 else [])
            for st, ln in ws:
                if not front:
                    st = L - st - ln  # mirrored
                lens.append(L), start.append(st), wlen.append(ln), lead.append(r if front else 0), trail.append(0 if front else r)
    for L in (1, 63, 64, 65, 128, 200):  # the whole read
        for st, ln in ((0, L), (L // 2, L - L // 2)):
            lens.append(L), start.append(st), wlen.append(ln), lead.append(L), trail.append(0)
    # both ends at once, and a window that holds neither
    lens += [300, 300]; start += [0, 70]; wlen += [300, 100]; lead += [65, 65]; trail += [64, 64]
    claims = ["%s_N_run_%d_window_%s" % (side, r, rel) for r in (1, 63, 64, 65, 128) for side in ("lead", "trail") for rel in ("inside", "straddles", "apart") if not (r == 1 and rel == "straddles")]
    C.append(Batch(kind, "terminal_N", claims + ["whole_read_N"], lens, start, wlen, np.ones(len(lens), np.int64), def_len=np.arange(len(lens)) % 5, n_lead=lead, n_trail=trail))
    return C


# =====================================================================================================================================
# the table
# =====================================================================================================================================

PARSE_EDGES, GATHER_EDGES, SCAN_EDGES, ORDER_EDGES = _parse_edges(), _gather_edges(), _scan_edges(), _order_edges()


def required():
    """{(kind, edge)}: what has to be reached, per entry point"""
    req = {("parse", e) for e in PARSE_EDGES}
    req |= {(k, e) for e, (_, kinds) in GATHER_EDGES.items() for k in kinds}
    req |= {(k, e) for e in SCAN_EDGES for k in ("emit", "render")}
    req |= {("render", e) for e in ORDER_EDGES}
    return req


def parse_texts(n_cu=DEFAULT_CU):
    """Every text for the parse: parse_cases() and the gather layouts as texts."""
    return parse_cases(n_cu) + [ParseCase("layout_" + lay.name, layout_text(lay), lay.claims) for lay in layouts() if "parse" in lay.kinds]


def all_cases(n_cu=DEFAULT_CU):
    """Every case of the catalogue: parse_texts(), the emit and the render batches."""
    return parse_texts(n_cu) + batch_cases("emit") + batch_cases("render")


def hits(case):
    """The edges a case reaches: {edge} (for a parse text with the value of final as 'edge' evaluates it; '/final' and '/open' edges name theirs)."""
    out = set()
    if case.kind == "parse":
        for final in case.finals:
            c = case.ctx(final)
            out |= {e for e, p in PARSE_EDGES.items() if p(c)}
            out |= {e for e, (p, _) in GATHER_EDGES.items() if p(c.offset)}
    else:
        c = case.scan_ctx()
        out |= {e for e, p in SCAN_EDGES.items() if p(c)}
        out |= {e for e, p in ORDER_EDGES.items() if case.kind == "render" and p(c)}
        out |= {e for e, (p, _) in GATHER_EDGES.items() if p(c.offset)}
    return out


def coverage(cases=None):
    """-> {(kind, edge): [names of the cases that reach it]} over every case (none is filtered out), and {case name: edges reached}"""
    cases = all_cases() if cases is None else cases
    table, per_case = {k: [] for k in required()}, {}
    for case in cases:
        h = hits(case)
        per_case[(case.kind, case.name)] = h
        for e in h:
            if (case.kind, e) in table:
                table[(case.kind, e)].append(case.name)
    return table, per_case


if __name__ == "__main__":
    table, _ = coverage()
    for (kind, edge), names in sorted(table.items()):
        print("%-7s %-48s %3d  %s" % (kind, edge, len(names), ", ".join(names[:3]) + (" ..." if len(names) > 3 else "")))
    print("%d edges, %d unreached" % (len(table), sum(not v for v in table.values())))
