"""Host driver: the FaQCs process contract (FaQCs.cpp main / process_paired / process_unpaired) around
an *engine* that stands where the reference calls ``trim()``.

Architecture differs from the reference on purpose: instead of one ``trim()`` per 32 768-read buffer the
driver packs several buffers (``segments``) into one structure-of-arrays batch and submits them together;
the segment table keeps every 32 768-granular semantic of the reference (adapter groups of 8, k-mer
rarefaction points, TOTAL_NUMBER ordering mate-1 buffer / mate-2 buffer).  Observable outputs -- the
trimmed FASTQs, ``<prefix>.stats.txt``, the --debug tables, exit codes and messages -- follow the
reference byte for byte (SURVEY.md section 8b "outer seam").

``run(argv)`` uses the HIP engine.  ``engine_factory`` exists so the tests can drive the same host logic
with the CPU checker; nothing in this package constructs any other engine.
"""
import gzip
import os
import sys

import numpy as np

from . import _capi as capi
from . import report
from .options import AUTO_DETECT_QUALITY_OFFSET, DEFAULT_NEXTSEQ_QUALITY_SCORE, Options, parse_args

BUFFER_SIZE = capi.SEGMENT_READS  # FaQCs.cpp:232
PAD = 32  # readable slack the kernels' aligned 16-byte loads may touch


class FatalError(Exception):
    """An error the reference reports as ``Caught the error <msg>`` + EXIT_FAILURE (FaQCs.cpp:136-147)."""


def parse_id(d: bytes) -> bytes:
    """trim.cpp:188-222"""
    loc = d.find(b" ")
    if loc < 0:
        loc = len(d)
    if loc > 1 and d[loc - 1:loc].isdigit() and d[loc - 2:loc - 1] in (b".", b"/"):
        loc -= 2
    return d[:loc]


def auto_detect_quality_offset(quals) -> int:
    """trim.cpp:599-617 over a buffer of quality strings (first decisive byte wins)."""
    for q in quals:
        if not q:
            continue
        a = np.frombuffer(q, dtype=np.uint8).view(np.int8)
        hit = np.nonzero((a > 74) | (a < 59))[0]
        if len(hit):
            return 64 if a[hit[0]] > 74 else 33
    raise FatalError("trim.cpp:auto_detect_quality_offset: Unknown quality format!")


def auto_detect_next_seq(defs) -> bool:
    """trim.cpp:619-626"""
    return bool(defs) and defs[0].startswith(b"@NS")


class FastqReader:
    """fastq.cpp:8-125 ``next_read`` semantics on a (possibly gzip'd) file; line terminators \\n or \\r."""

    def __init__(self, path, what):
        try:
            f = open(path, "rb")
        except OSError:
            raise FatalError("I/O error")
        magic = f.read(2)
        f.seek(0)
        self.f = gzip.open(f, "rb") if magic == b"\x1f\x8b" else f
        self.what = what

    def next_read(self):
        d = self.f.readline()
        if not d:
            return None
        s = self.f.readline()
        if not s:
            raise FatalError("fastq.cpp:next_read: Unable to read sequence")
        p = self.f.readline()
        if not p:
            raise FatalError("fastq.cpp:next_read: Unable to read '+'")
        q = self.f.readline()
        if not q and not p.endswith((b"\n", b"\r")):
            raise FatalError("fastq.cpp:next_read: Error reading '+' delimiter")
        d, s, q = (x.split(b"\n")[0].split(b"\r")[0] for x in (d, s, q))
        if len(s) != len(q):
            raise FatalError("fastq.cpp:next_read: |Sequence| != |Quality|")
        return d, s, q

    def close(self):
        self.f.close()


def parse_model(text: bytes, final: bool):
    """What faqcs_parse_device() / faqcs_parse_host() deliver, written from the rules of include/faqcs_mi.h (fastq.cpp:8-125) and not
    from the library: a line ends at '\\n', its content at its first '\\r' (or the '\\n', or the end of the text); a record is four lines;
    the first record with |bases| != |qualities| or, in a final text, with lines missing decides the error, and the records in front of
    it are delivered.  A text that is not final delivers only records whose four lines all end in '\\n'.
    -> (seq, qual, offset uint32[n + 1], terminal_n uint8[n], def_pos uint32[n], def_len uint32[n], consumed, error)"""
    text = bytes(text)
    lines = text.split(b"\n")  # n_newlines + 1 pieces; the last one is the unterminated rest (b"" when the text ends in '\n' or is empty)
    n_nl = len(lines) - 1
    open_tail = len(lines[-1]) > 0
    starts = np.zeros(len(lines) + 1, dtype=np.int64)
    starts[1:] = np.cumsum([len(x) + 1 for x in lines])
    ltot = n_nl + (1 if open_tail else 0)
    n_cand = ltot // 4 if final else n_nl // 4
    tail = capi.PARSE_OK
    if final:
        tail = (capi.PARSE_OK, capi.PARSE_E_SEQUENCE, capi.PARSE_E_PLUS,
                capi.PARSE_E_PLUS_DELIM if open_tail else capi.PARSE_E_QUALITY)[ltot % 4]

    def content(x):
        i = x.find(b"\r")
        return x if i < 0 else x[:i]

    seqs, quals, tn, dpos, dlen = [], [], [], [], []
    error, n = tail, n_cand
    for k in range(n_cand):
        d, s, q = content(lines[4 * k]), content(lines[4 * k + 1]), content(lines[4 * k + 3])
        if len(s) != len(q):
            error, n = capi.PARSE_E_LENGTH, k
            break
        seqs.append(s)
        quals.append(q)
        tn.append(((1 if s[:1] == b"N" else 0) | (2 if s[-1:] == b"N" else 0)) if s else 0)
        dpos.append(int(starts[4 * k]))
        dlen.append(len(d))
    consumed = min(int(starts[4 * n]), len(text))  # (a final text's last quality line may lack its '\n')
    offset = np.zeros(n + 1, dtype=np.uint32)
    if n:
        offset[1:] = np.cumsum([len(x) for x in seqs])
    return (np.frombuffer(b"".join(seqs), dtype=np.uint8), np.frombuffer(b"".join(quals), dtype=np.uint8), offset,
            np.asarray(tn, dtype=np.uint8), np.asarray(dpos, dtype=np.uint32), np.asarray(dlen, dtype=np.uint32), consumed, error)


def pack_segments(buffers):
    """buffers: list of lists of (def, seq, qual).  -> (seq arena, qual arena, offset, segment_start)"""
    lens, seg = [], [0]
    for b in buffers:
        lens.extend(len(r[1]) for r in b)
        seg.append(len(lens))
    offset = np.zeros(len(lens) + 1, dtype=np.uint32)
    if lens:
        offset[1:] = np.cumsum(np.asarray(lens, dtype=np.int64)).astype(np.uint32)
    pad = b"\0" * PAD
    seq = np.frombuffer(b"".join([pad] + [r[1] for b in buffers for r in b] + [pad]), dtype=np.uint8)
    qual = np.frombuffer(b"".join([pad] + [r[2] for b in buffers for r in b] + [pad]), dtype=np.uint8)
    # arenas start PAD bytes in so the aligned loads may under-read; hand the engine the shifted views
    return seq[PAD:], qual[PAD:], offset, np.asarray(seg, dtype=np.uint32)


def terminal_n_flags(seq, offset):
    """faqcs_batch.terminal_n for a packed host arena: bit 0 = a read's first base is 'N', bit 1 = its last (what
    mask_quality_terminal_N, trim.cpp:1191-1216, tests first); 0 for an empty read."""
    off = offset.astype(np.int64)
    n = len(off) - 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint8)
    nonempty = off[1:] > off[:-1]
    first = seq[np.minimum(off[:-1], max(len(seq) - 1, 0))] == ord("N")
    last = seq[np.maximum(off[1:] - 1, 0)] == ord("N")
    return ((first & nonempty).astype(np.uint8) | ((last & nonempty).astype(np.uint8) << 1))


def edited_arenas(opt, in_off, seq, qual, offset):
    """The rule-based byte edits of include/faqcs_mi.h faqcs_read_result, vectorised over a whole arena:
    terminal-N quality masking (trim.cpp:1191-1216), G->N (trim.cpp:390-403), offset re-encode
    (trim.cpp:516-525).  Only bytes inside a valid read's kept window are ever written out."""
    n = len(offset) - 1
    total = int(offset[-1])
    s = np.array(seq[:total], dtype=np.uint8)
    q = np.array(qual[:total], dtype=np.uint8)
    if n:
        lens = np.diff(offset.astype(np.int64))
        nz = lens > 0
        first = offset[:-1][nz].astype(np.int64)
        last = offset[1:][nz].astype(np.int64) - 1
        idx = np.nonzero(nz)[0]
        for i in idx[(s[first] == 78) | (s[last] == 78)]:
            a, b = int(offset[i]), int(offset[i + 1])
            k = a
            while k < b and s[k] == 78:
                q[k] = in_off & 0xFF
                k += 1
            k = b
            while k > a and s[k - 1] == 78:
                q[k - 1] = in_off & 0xFF
                k -= 1
    qs = np.maximum(q.view(np.int8).astype(np.int16) - in_off, 0)
    if opt.replace_to_N_q > 0:
        s[(s == 71) & (qs < opt.replace_to_N_q)] = 78
    if in_off != opt.output_quality_offset:
        q = (qs + opt.output_quality_offset).astype(np.uint8)
    return s, q


def emit_model(opt, in_off, seq, qual, offset, res, keep=None):
    """What faqcs_emit_device() packs, as numpy: every read with F_VALID (and keep[i] != 0 when keep is given), in input order, its
    kept window cut out of edited_arenas().  -> (seq, qual, offset uint32[n_emitted + 1], index uint32[n_emitted])"""
    offset = np.asarray(offset)
    n = len(offset) - 1
    sel = (res["flags"][:n] & capi.F_VALID) != 0
    if keep is not None:
        sel &= np.asarray(keep)[:n] != 0
    index = np.nonzero(sel)[0].astype(np.uint32)
    lens = res["len"][index].astype(np.int64)
    out_off = np.zeros(len(index) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(lens)
    total = int(out_off[-1])
    if total == 0:
        z = np.zeros(0, dtype=np.uint8)
        return z, z.copy(), out_off.astype(np.uint32), index
    es, eq = edited_arenas(opt, in_off, seq, qual, offset)
    first = offset[index].astype(np.int64) + res["start"][index].astype(np.int64)
    src = np.repeat(first - out_off[:-1], lens) + np.arange(total, dtype=np.int64)
    return es[src], eq[src], out_off.astype(np.uint32), index


def render_model(opt, in_off, text, def_pos, def_len, seq, qual, offset, res=None, select=None, order=None):
    """What faqcs_render_device() / faqcs_render_host() write, as numpy, from the rules of include/faqcs_mi.h: candidate j is read order[j]
    (j without an order; an entry >= n is skipped); it is rendered when select[i] != 0 (or no select) and, with results, F_VALID; the record
    is defline \\n S \\n+\\n Q \\n with S / Q the kept window cut out of edited_arenas() (results given: Run.write_read) or the read as it came
    (res None: the discard stream, _write_raw).  -> (text uint8, rec_offset uint32[n_rendered + 1], rec_index uint32[n_rendered])"""
    offset = np.asarray(offset)
    n = len(offset) - 1
    cand = np.arange(n, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)[:n]
    cand = cand[(cand >= 0) & (cand < n)]
    ok = np.ones(len(cand), dtype=bool)
    if select is not None:
        ok &= np.asarray(select)[cand] != 0
    if res is not None:
        ok &= (res["flags"][cand] & capi.F_VALID) != 0
    index = cand[ok]
    if res is not None:
        es, eq = edited_arenas(opt, in_off, seq, qual, offset)
        first = offset[index].astype(np.int64) + res["start"][index].astype(np.int64)
        lens = res["len"][index].astype(np.int64)
    else:
        es, eq = np.asarray(seq), np.asarray(qual)
        first = offset[index].astype(np.int64)
        lens = offset[index + 1].astype(np.int64) - first
    text = np.asarray(text)
    pieces = []
    for k, i in enumerate(index):
        a, b, d = int(first[k]), int(first[k] + lens[k]), int(def_pos[i])
        pieces += [text[d:d + int(def_len[i])].tobytes(), b"\n", es[a:b].tobytes(), b"\n+\n", eq[a:b].tobytes(), b"\n"]
    rec_offset = np.zeros(len(index) + 1, dtype=np.int64)
    rec_offset[1:] = np.cumsum(np.asarray(def_len)[index].astype(np.int64) + 2 * lens + 5)
    out = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    assert len(out) == int(rec_offset[-1])
    return out, rec_offset.astype(np.uint32), index.astype(np.uint32)


def pair_model(mate1, mate2):
    """What faqcs_pair_device() / faqcs_pair_host() deliver, written from parse_id (trim.cpp:188-222) and FaQCs.cpp:296-361,382-389: a mate
    is a dict with text (uint8), def_pos, def_len and res (the per-read results, or None for both mates: check only).  The pairs
    i < min(n1, n2) in order; the first whose ids differ stops the count and routes the rest nowhere.
    -> (route uint8[n] or None, info dict of the faqcs_pair_info fields)"""
    n = min(len(mate1["def_pos"]), len(mate2["def_pos"]))
    routed = mate1["res"] is not None
    route = np.full(n, capi.ROUTE_NOWHERE, dtype=np.uint8) if routed else None
    info = dict(paired_read_number=0, paired_base_length=0, n_pairs=n, mismatch=0, id_len=(0, 0), n_one_valid=0, n_none_valid=0)
    for i in range(n):
        ids = []
        for m in (mate1, mate2):
            a = int(m["def_pos"][i])
            ids.append(parse_id(bytes(m["text"][a:a + int(m["def_len"][i])])))
        if ids[0] != ids[1]:
            info.update(n_pairs=i, mismatch=1, id_len=(len(ids[0]), len(ids[1])))
            break
        if not routed:
            continue
        v1, v2 = (bool(m["res"]["flags"][i] & capi.F_VALID) for m in (mate1, mate2))
        route[i] = (capi.ROUTE_V1 if v1 else 0) | (capi.ROUTE_V2 if v2 else 0)
        if v1 and v2:  # FaQCs.cpp:304-308
            info["paired_read_number"] += 2
            info["paired_base_length"] += int(mate1["res"]["len"][i]) + int(mate2["res"]["len"][i])
        elif v1 or v2:
            info["n_one_valid"] += 1
        else:
            info["n_none_valid"] += 1
    return route, info


def render_pair_model(opt, in_off, file, mate1, mate2, route, n_pairs):
    """What faqcs_render_pair_device() / faqcs_render_pair_host() write for one of the four files (capi.FILE_*), from FaQCs.cpp:296-361: both
    mates to QC.1 / QC.2 when both are valid, the one valid mate to QC.unpaired, every mate that is not valid to QC.discard as it came --
    pair by pair, mate 1 first.  A mate is a dict with text, def_pos, def_len, seq, qual, offset, res.
    -> (text uint8, rec_offset uint32[n_rendered + 1], rec_index uint32[n_rendered], rec_index[k] = 2 i + s)"""
    mates = (mate1, mate2)
    trimmed = file != capi.FILE_DISCARD
    edited = [edited_arenas(opt, in_off, m["seq"], m["qual"], m["offset"]) if trimmed else (np.asarray(m["seq"]), np.asarray(m["qual"])) for m in mates]
    pieces, ends, index = [], [0], []
    for i in range(n_pairs):
        r = int(route[i])
        for s, m in enumerate(mates):
            if file == capi.FILE_QC1:
                take = s == 0 and r == 3
            elif file == capi.FILE_QC2:
                take = s == 1 and r == 3
            elif file == capi.FILE_UNPAIRED:
                take = r == (1 << s)
            else:
                take = r < 4 and not (r >> s) & 1
            if not take:
                continue
            a, b = int(m["offset"][i]), int(m["offset"][i + 1])
            if trimmed:
                a += int(m["res"]["start"][i])
                b = a + int(m["res"]["len"][i])
            d = int(m["def_pos"][i])
            rec = (np.asarray(m["text"][d:d + int(m["def_len"][i])]).tobytes() + b"\n" + edited[s][0][a:b].tobytes() + b"\n+\n"
                   + edited[s][1][a:b].tobytes() + b"\n")
            pieces.append(rec)
            ends.append(ends[-1] + len(rec))
            index.append(2 * i + s)
    return np.frombuffer(b"".join(pieces), dtype=np.uint8), np.asarray(ends, dtype=np.uint32), np.asarray(index, dtype=np.uint32)


def detect_model(qual, offset, first, count, text=None, def_pos=None, def_len=None):
    """The rules of faqcs_detect_device / faqcs_detect_host (include/faqcs_mi.h) in numpy: the lowest arena position b in
    [offset[first], offset[first + count]) whose quality byte, as a signed char, is > 74 (64) or < 59 (33); the read that owns it; and
    whether the defline content of read `first` starts with "@NS" (trim.cpp:599-626).  -> dict of the faqcs_detect_info fields."""
    offset = np.asarray(offset, dtype=np.int64)
    first, count = int(first), int(count)
    if first + count > len(offset) - 1:
        raise ValueError("the range of reads leaves the batch")
    if len({text is None, def_pos is None, def_len is None}) != 1:
        raise ValueError("text, def_pos and def_len go together")
    d = dict(quality_offset=0, read=first + count, pos=0, byte=0, next_seq=0, reserved=0)
    if count:
        a, e = int(offset[first]), int(offset[first + count])
        q = np.asarray(qual, dtype=np.uint8)[a:e].view(np.int8)
        hit = np.nonzero((q > 74) | (q < 59))[0]
        if len(hit):
            b = a + int(hit[0])
            read = int(np.searchsorted(offset[first:first + count + 1], b, side="right")) - 1 + first  # the last i with offset[i] <= b
            d.update(quality_offset=64 if q[hit[0]] > 74 else 33, read=read, pos=b - int(offset[read]), byte=int(q[hit[0]]) & 0xFF)
        if text is not None:
            p, ln = int(def_pos[first]), int(def_len[first])
            d["next_seq"] = int(ln >= 3 and bytes(bytearray(text[p:p + 3])) == b"@NS")
    return d


def first_error_model(res):
    """The rule of faqcs_first_error_device / faqcs_first_error_host in numpy: (n_good, flags) -- the index of the first result with an
    F_ERR_* bit, or len(res), and that read's two error bits."""
    f = np.asarray(res["flags"], dtype=np.uint16) & np.uint16(capi.F_ERR_QUALITY | capi.F_ERR_BASE)
    hit = np.nonzero(f)[0]
    return (int(hit[0]), int(f[hit[0]])) if len(hit) else (len(f), 0)


class Run:
    """State the reference keeps in main(): filter_stats, adapter_stats, PlotInfo, Options (FaQCs.cpp:67-69)."""

    def __init__(self, opt: Options, engine_factory, err, batch_buffers=8, max_read_length=capi.MAX_READ_LENGTH):
        self.opt = opt
        self.engine_factory = engine_factory
        self.err = err
        self.engine = None
        self.batch_buffers = batch_buffers
        self.max_read_length = max_read_length
        self.in_off = opt.input_quality_offset
        self.quality = opt.quality
        self.paired_read_number = 0
        self.paired_base_length = 0

    def say(self, msg):
        print(msg, file=self.err)

    def ensure_engine(self):
        if self.engine is None:
            self.engine = self.engine_factory(self.opt, self.max_read_length, self.in_off)
            if self.quality != self.opt.quality:
                self.engine.set_quality(self.quality)
        return self.engine

    def nextseq_check(self, defs):
        if self.quality < DEFAULT_NEXTSEQ_QUALITY_SCORE and auto_detect_next_seq(defs):
            self.say("The input looks like NextSeq data and the quality level (-q) is adjusted to %d for trimming."
                     % DEFAULT_NEXTSEQ_QUALITY_SCORE)
            self.quality = DEFAULT_NEXTSEQ_QUALITY_SCORE
            if self.engine is not None:
                self.engine.set_quality(self.quality)

    # ---- FaQCs.cpp:153-538 ----------------------------------------------------------------------
    def process_paired(self):
        opt = self.opt
        try:
            fin1 = FastqReader(opt.input_read1_file, "read one")
        except FatalError:
            self.say("Unable to open %s for loading read one sequences" % opt.input_read1_file)
            raise
        try:
            fin2 = FastqReader(opt.input_read2_file, "read two")
        except FatalError:
            self.say("Unable to open %s for loading read two sequences" % opt.input_read2_file)
            raise
        fout1 = fout2 = foutu = foutd = None
        if not opt.qc_only:
            fout1 = open(opt.trimmed_read1_file, "wb")
            fout2 = open(opt.trimmed_read2_file, "wb")
            foutu = open(opt.trimmed_unpaired_file, "wb")
            if opt.trimmed_discard_file:
                foutd = open(opt.trimmed_discard_file, "wb")
        pending = []  # list of (buffer1, buffer2)
        check_for_next_seq = True
        b1, b2 = [], []

        def flush():
            if not pending:
                return
            eng = self.ensure_engine()
            bufs = [b for pair in pending for b in pair]  # reference call order: trim(buffer1), trim(buffer2)
            seq, qual, offset, seg = pack_segments(bufs)
            res = eng.process(seq, qual, offset, seg, terminal_n_flags(seq, offset))
            es, eq = edited_arenas(opt, self.in_off, seq, qual, offset) if not opt.qc_only else (None, None)
            valid = (res["flags"] & capi.F_VALID) != 0
            for k, (x1, x2) in enumerate(pending):
                o1, o2 = int(seg[2 * k]), int(seg[2 * k + 1])
                for i in range(len(x1)):
                    i1, i2 = o1 + i, o2 + i
                    v1, v2 = valid[i1], valid[i2]
                    if v1 and v2:
                        self.paired_read_number += 2
                        self.paired_base_length += int(res["len"][i1]) + int(res["len"][i2])
                    if opt.qc_only:
                        continue
                    if v1 and v2:
                        _write(fout1, x1[i][0], es, eq, offset, res, i1)
                        _write(fout2, x2[i][0], es, eq, offset, res, i2)
                    else:
                        if v1:
                            _write(foutu, x1[i][0], es, eq, offset, res, i1)
                        elif v2:
                            _write(foutu, x2[i][0], es, eq, offset, res, i2)
                        if foutd is not None:
                            if not v1:
                                _write_raw(foutd, x1[i])
                            if not v2:
                                _write_raw(foutd, x2[i])
            pending.clear()

        while True:
            r1 = fin1.next_read()
            r2 = fin2.next_read()
            if r1 is None and r2 is None:
                if self.in_off == AUTO_DETECT_QUALITY_OFFSET:
                    self.in_off = auto_detect_quality_offset([r[2] for r in b1])
                    if self.in_off != auto_detect_quality_offset([r[2] for r in b2]):
                        self.say("Inconsistent quality offset detection between reads one and two")
                        raise FatalError("FaQCs.cpp:process_paired: I/O Error")
                flush()  # buffers trimmed with the pre-bump quality must go first
                self.nextseq_check([r[0] for r in b1])  # Q16: runs on the last partial buffer regardless
                pending.append((b1, b2))
                flush()
                break
            if (r1 is None) != (r2 is None):
                if r1 is not None:
                    self.say("Did not find a match to read one: " + r1[0].decode("latin-1"))
                else:
                    self.say("Did not find a match to read two: " + r2[0].decode("latin-1"))
                raise FatalError("FaQCs.cppI/O error")
            if parse_id(r1[0]) != parse_id(r2[0]):
                self.say("Read one id (%s)\ndoes not match\nread two id (%s)" % (
                    parse_id(r1[0]).decode("latin-1"), parse_id(r2[0]).decode("latin-1")))
                raise FatalError("FaQCs.cpp:trim: I/O error")
            b1.append(r1)
            b2.append(r2)
            if len(b1) == BUFFER_SIZE:
                if self.in_off == AUTO_DETECT_QUALITY_OFFSET:
                    self.in_off = auto_detect_quality_offset([r[2] for r in b1])
                    if self.in_off != auto_detect_quality_offset([r[2] for r in b2]):
                        self.say("Inconsistent quality offset detection between reads one and two")
                        raise FatalError("FaQCs.cpp:process_paired: I/O Error")
                if check_for_next_seq:
                    self.nextseq_check([r[0] for r in b1])
                    check_for_next_seq = False
                pending.append((b1, b2))
                b1, b2 = [], []
                if len(pending) >= self.batch_buffers:
                    flush()
        fin1.close()
        fin2.close()
        for f in (fout1, fout2, foutu, foutd):
            if f is not None:
                f.close()
        if self.engine is not None:
            self.engine.kmer_end_table()  # FaQCs.cpp:518-537

    # ---- FaQCs.cpp:540-757 ----------------------------------------------------------------------
    def process_unpaired(self):
        opt = self.opt
        try:
            fin = FastqReader(opt.input_unpaired_file, "unpaired")
        except FatalError:
            self.say("Unable to open %s for loading unpaired read sequences" % opt.input_unpaired_file)
            raise
        fout = foutd = None
        if not opt.qc_only:
            fout = open(opt.trimmed_unpaired_file, "wb")  # "wT": truncates what process_paired wrote (Q17)
            if opt.trimmed_discard_file:
                foutd = open(opt.trimmed_discard_file, "wb")
        pending, buf = [], []
        check_for_next_seq = True

        def flush():
            if not pending:
                return
            eng = self.ensure_engine()
            seq, qual, offset, seg = pack_segments(pending)
            res = eng.process(seq, qual, offset, seg, terminal_n_flags(seq, offset))
            if not opt.qc_only:
                es, eq = edited_arenas(opt, self.in_off, seq, qual, offset)
                valid = (res["flags"] & capi.F_VALID) != 0
                i = 0
                for b in pending:
                    for r in b:
                        if valid[i]:
                            _write(fout, r[0], es, eq, offset, res, i)
                        elif foutd is not None:
                            _write_raw(foutd, r)
                        i += 1
            pending.clear()

        while True:
            r = fin.next_read()
            if r is None:
                if self.in_off == AUTO_DETECT_QUALITY_OFFSET:
                    self.in_off = auto_detect_quality_offset([x[2] for x in buf])
                flush()
                self.nextseq_check([x[0] for x in buf])
                pending.append(buf)
                flush()
                break
            buf.append(r)
            if len(buf) == BUFFER_SIZE:
                if self.in_off == AUTO_DETECT_QUALITY_OFFSET:
                    self.in_off = auto_detect_quality_offset([x[2] for x in buf])
                if check_for_next_seq:
                    self.nextseq_check([x[0] for x in buf])
                    check_for_next_seq = False
                pending.append(buf)
                buf = []
                if len(pending) >= 2 * self.batch_buffers:
                    flush()
        fin.close()
        for f in (fout, foutd):
            if f is not None:
                f.close()
        if self.engine is not None:
            self.engine.kmer_end_table()

    def finish(self):
        opt = self.opt
        eng = self.ensure_engine()
        block = eng.counters()
        counters = report.Counters(block, self.max_read_length, eng.holder.n_adapters)
        fs = counters.fs.copy()
        fs[capi.PAIRED_READ_NUMBER] += self.paired_read_number
        fs[capi.PAIRED_BASE_LENGTH] += self.paired_base_length
        adapter_stats = report.merged_adapter_stats(opt, counters)
        fs = report.fold_phix_and_adapters(opt, fs, adapter_stats)
        try:
            with open(opt.stats_file, "w") as f:
                f.write(report.stats_text(opt, fs, adapter_stats, self.quality))
        except OSError:
            self.say("Unable to open %s for writing filtering statistics" % opt.stats_file)
        if not opt.trim_only and opt.debug:
            report.write_debug_tables(opt, counters, eng.kmer_histogram(), eng.kmer_points())
        self.filter_stats = fs
        self.counters = counters
        return fs


def _write(f, d, es, eq, offset, res, i):
    a = int(offset[i]) + int(res["start"][i])
    b = a + int(res["len"][i])
    f.write(d + b"\n" + es[a:b].tobytes() + b"\n+\n" + eq[a:b].tobytes() + b"\n")  # fastq.cpp:127-138


def _write_raw(f, r):
    f.write(r[0] + b"\n" + r[1] + b"\n+\n" + r[2] + b"\n")


def _remove_file(path, err):
    if path and os.path.isfile(path):  # FaQCs.cpp:1046-1053, file_util.cpp:11-20 (regular files only)
        print("The output %s file exists and will be overwritten." % path, file=err)
        os.unlink(path)


def _hip_engine(opt, max_read_length, in_off):
    from .engine import HipEngine

    return HipEngine(opt, max_read_length, in_off)


def run(argv, engine_factory=None, err=None, batch_buffers=8, max_read_length=capi.MAX_READ_LENGTH):
    """FaQCs.cpp:36-151.  Returns the process exit code (0 / 1)."""
    err = err or sys.stderr
    engine_factory = engine_factory or _hip_engine
    try:
        try:
            opt = parse_args(list(argv))
        except ValueError as e:
            raise FatalError(str(e))
        for m in opt.messages:
            print(m, file=err)
        if opt.print_usage:
            if not opt.version:
                print("FaQCs version 2.10 (MI355X engine): see the reference usage text for the flag list", file=err)
            return 1
        if not os.path.isdir(opt.output_dir):
            try:
                os.mkdir(opt.output_dir, 0o700)  # file_util.cpp:33-36
            except OSError:
                print('Unable to create requested output directory: "%s"' % opt.output_dir, file=err)
                return 1
        for p in (opt.plots_file, opt.stats_file, opt.trimmed_read1_file, opt.trimmed_read2_file,
                  opt.trimmed_unpaired_file, opt.trimmed_discard_file):
            _remove_file(p, err)
        r = Run(opt, engine_factory, err, batch_buffers, max_read_length)
        if opt.has_paired():
            r.process_paired()
        if opt.has_unpaired():
            r.process_unpaired()
        r.finish()
        run.last = r
        return 0
    except FatalError as e:
        print("Caught the error %s" % e, file=err)
        return 1
    except Exception as e:  # engine errors carry the reference's message text
        from .engine import FaqcsError

        if isinstance(e, FaqcsError):
            print("Caught the error %s" % e, file=err)
            return 1
        raise
