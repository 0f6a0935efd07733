"""HipEngine: the product engine -- a thin numpy wrapper over the C ABI of libfaqcs_mi.so.

An *engine* is what the host driver (faqcs_amd/driver.py) calls where the reference calls ``trim()``
(FaQCs.h:245-248).  ``process()`` takes a structure-of-arrays batch whose segments are the reference's
individual trim() calls.  There is exactly one engine in the product: this one.  (tests/ has an
OracleEngine with the same surface that wraps the CPU checker; it is never imported from here.)
"""
import ctypes as C

import numpy as np

from . import _capi as capi


class FaqcsError(RuntimeError):
    """Raised with the text the reference would print after ``Caught the error``."""

    def __init__(self, code, text):
        super().__init__(text)
        self.code = code


def _check(lib, rc):
    if rc != 0:
        msg = capi.ERR_TEXT.get(rc) or (lib.faqcs_last_error() or b"").decode() or "faqcs error %d" % rc
        raise FaqcsError(rc, msg)


def bgzf_index_host(comp, final=True, lib=None):
    """faqcs_bgzf_index_host (host only, no GPU): the BGZF members of `comp` (bytes or a uint8 array), walked from byte 0.
    Returns (member_offset uint32 [n_members + 1], consumed, error): member k is comp[member_offset[k] : member_offset[k + 1]], `consumed`
    is where the next chunk starts (final = False leaves an incomplete last member to the caller), error is a capi.INFLATE_* code."""
    lib = lib or capi.load_library()
    buf = np.frombuffer(comp, dtype=np.uint8) if isinstance(comp, (bytes, bytearray, memoryview)) else np.ascontiguousarray(comp, dtype=np.uint8)
    cap = len(buf) // 26 + 1
    off = np.zeros(cap + 1, dtype=np.uint32)
    info = capi.BgzfIndexInfo()
    _check(lib, lib.faqcs_bgzf_index_host(buf.ctypes.data if len(buf) else None, len(buf), 1 if final else 0, off.ctypes.data, cap, C.byref(info)))
    return off[:info.n_members + 1].copy(), int(info.consumed), int(info.error)


def gunzip_host(comp, piece_bytes=0, max_rounds=0, capacity=None, lib=None):
    """faqcs_gunzip_host (host only, no GPU): ordinary gzip `comp` (bytes or a uint8 array; one or more whole members) inflated by pieces of
    piece_bytes compressed bytes (0: the default), with at most max_rounds count rounds per member (0: the default).  capacity: bytes of text
    to make room for (default: found with a first call).  Returns (text bytes, info dict): the faqcs_gunzip_info fields -- what
    faqcs_gunzip_device states for the same bytes, field for field; with info["overflow"] the text is empty."""
    lib = lib or capi.load_library()
    buf = np.frombuffer(comp, dtype=np.uint8) if isinstance(comp, (bytes, bytearray, memoryview)) else np.ascontiguousarray(comp, dtype=np.uint8)
    info = capi.GunzipInfo()
    for cap in ([0, None] if capacity is None else [int(capacity)]):
        cap = int(info.n_bytes) if cap is None else cap
        store = np.zeros(cap + 32, dtype=np.uint8)
        shift = (-store.ctypes.data) % 16
        out = capi.GunzipOut(store.ctypes.data + shift, cap, C.addressof(info))
        _check(lib, lib.faqcs_gunzip_host(buf.ctypes.data if len(buf) else None, len(buf), int(piece_bytes), int(max_rounds), C.byref(out)))
        if not info.overflow:
            break
    d = {f: int(getattr(info, f)) for f, _ in capi.GunzipInfo._fields_}
    return (b"" if info.overflow else store[shift:shift + info.n_bytes].tobytes()), d


def gunzip_state(window):
    """A zeroed capi.GunzipState over `window`, the address of the caller's capi.GUNZIP_WINDOW bytes: what a file's first call takes."""
    st = capi.GunzipState()
    st.window = window
    return st


def gunzip_stream_host(comp, final, state, window, piece_bytes=0, max_rounds=0, capacity=None, lib=None):
    """faqcs_gunzip_stream_host (host only, no GPU): one chunk of an ordinary gzip file -- `comp` (bytes or a uint8 array) is the file from
    where the previous call's info["consumed"] left it, final says that these are its last bytes.  state: the file's capi.GunzipState
    (gunzip_state() before the first call), rewritten in place; window: the uint8 array of capi.GUNZIP_WINDOW bytes it points to (kept
    alive by the caller).  capacity: bytes of text to make room for (default: found with a first call, which leaves the state alone).
    Returns (text bytes of this call, info dict) -- what faqcs_gunzip_stream_device states for the same bytes, field for field."""
    lib = lib or capi.load_library()
    buf = np.frombuffer(comp, dtype=np.uint8) if isinstance(comp, (bytes, bytearray, memoryview)) else np.ascontiguousarray(comp, dtype=np.uint8)
    assert state.window == window.ctypes.data and window.nbytes >= capi.GUNZIP_WINDOW
    info = capi.GunzipInfo()
    for cap in ([0, None] if capacity is None else [int(capacity)]):
        cap = int(info.n_bytes) if cap is None else cap
        store = np.zeros(cap + 32, dtype=np.uint8)
        shift = (-store.ctypes.data) % 16
        out = capi.GunzipOut(store.ctypes.data + shift, cap, C.addressof(info))
        _check(lib, lib.faqcs_gunzip_stream_host(buf.ctypes.data if len(buf) else None, len(buf), 1 if final else 0, int(piece_bytes), int(max_rounds),
                                                 C.byref(state), C.byref(out)))
        if not info.overflow:
            break
    d = {f: int(getattr(info, f)) for f, _ in capi.GunzipInfo._fields_}
    return (b"" if info.overflow else store[shift:shift + info.n_bytes].tobytes()), d


def deflate_host(text, member_bytes=0, final=True, lib=None, mode=capi.DEFLATE_FAST):
    """faqcs_deflate_host_mode (host only, no GPU; mode: capi.DEFLATE_FAST, what faqcs_deflate_host does, or capi.DEFLATE_DENSE): `text` (bytes or a uint8 array) as BGZF members of member_bytes bytes of text each (0: 65 280),
    the EOF member behind them when final.  Returns (comp bytes, member_offset uint32 [n_members + 1], n_stored): the bytes
    faqcs_deflate_device_mode produces for the same arguments."""
    lib = lib or capi.load_library()
    buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
    mb = int(member_bytes) or 65280
    n = (len(buf) + mb - 1) // mb + (1 if final else 0)
    cap = len(buf) + 31 * n + 16
    store = np.zeros(cap + 16, dtype=np.uint8)
    shift = (-store.ctypes.data) % 16
    off = np.zeros(n + 1, dtype=np.uint32)
    info = capi.DeflateInfo()
    out = capi.DeflateOut(store.ctypes.data + shift, cap, off.ctypes.data, C.addressof(info))
    _check(lib, lib.faqcs_deflate_host_mode(buf.ctypes.data if len(buf) else None, len(buf), int(member_bytes), 1 if final else 0, int(mode), C.byref(out)))
    assert not info.overflow and info.n_members == n
    return store[shift:shift + info.n_bytes].tobytes(), off, int(info.n_stored)


def detect_host(qual, offset, first=0, count=None, text=None, def_pos=None, def_len=None, lib=None):
    """faqcs_detect_host (host only, no GPU): the first decisive quality byte of reads [first, first + count) of a packed batch (qual: uint8
    arena, offset: uint32 [n + 1]; count None: to the batch's end) and, with text / def_pos / def_len (all three or none), whether the
    defline of read `first` starts with "@NS".  Returns the faqcs_detect_info fields as a dict."""
    lib = lib or capi.load_library()
    qual = np.ascontiguousarray(qual, dtype=np.uint8)
    qual = qual if len(qual) else np.zeros(1, np.uint8)
    offset = np.ascontiguousarray(offset, dtype=np.uint32)
    n = len(offset) - 1
    count = n - first if count is None else count
    given = [x is not None for x in (text, def_pos, def_len)]
    if text is not None:
        text = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        text = text if len(text) else np.zeros(1, np.uint8)
    if def_pos is not None:
        def_pos = np.ascontiguousarray(np.append(def_pos, 0), dtype=np.uint32)
    if def_len is not None:
        def_len = np.ascontiguousarray(np.append(def_len, 0), dtype=np.uint32)
    b = capi.Batch(None, qual.ctypes.data, offset.ctypes.data, n, 0, None, 0, None)
    info = capi.DetectInfo()
    _check(lib, lib.faqcs_detect_host(C.byref(b), int(first), int(count), text.ctypes.data if given[0] else None,
                                      def_pos.ctypes.data if given[1] else None, def_len.ctypes.data if given[2] else None, C.byref(info)))
    return {f: int(getattr(info, f)) for f, _ in capi.DetectInfo._fields_}


def first_error_host(results, lib=None):
    """faqcs_first_error_host (host only, no GPU): (n_good, flags) of a per-read result array (capi.RESULT_DTYPE) -- the index of the first
    read with an F_ERR_* bit, or len(results), and that read's error bits."""
    lib = lib or capi.load_library()
    results = np.ascontiguousarray(results, dtype=capi.RESULT_DTYPE)
    info = capi.ErrorInfo()
    _check(lib, lib.faqcs_first_error_host(results.ctypes.data if len(results) else None, len(results), C.byref(info)))
    return int(info.n_good), int(info.flags)


class HipEngine:
    name = "hip"

    def __init__(self, opt, max_read_length, input_quality_offset=None, device=-1, kmer_table_slots=0):
        self.lib = capi.load_library()
        self.holder = capi.ParamsHolder(opt, max_read_length, input_quality_offset, kmer_table_slots)
        self.ctx = C.c_void_p()
        _check(self.lib, self.lib.faqcs_create(C.byref(self.holder.p), device, C.byref(self.ctx)))
        lay = capi.Layout()
        _check(self.lib, self.lib.faqcs_counters_layout(max_read_length, self.holder.n_adapters, C.byref(lay)))
        self.layout = lay
        self.n_counters = int(lay.total)

    # -- the trim() seam ---------------------------------------------------------------------------
    def process(self, seq, qual, offset, segment_start, terminal_n=None):
        """seq/qual: uint8 arenas (host memory: the library copies them into padded device buffers), offset: uint32[n+1],
        segment_start: uint32[n_segments+1]; terminal_n: optional uint8[n] (faqcs_batch.terminal_n, see terminal_n_flags()).
        Returns the per-read result array."""
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        segment_start = np.ascontiguousarray(segment_start, dtype=np.uint32)
        n = len(offset) - 1
        res = np.zeros(n, dtype=capi.RESULT_DTYPE)
        if terminal_n is not None:
            terminal_n = np.ascontiguousarray(terminal_n, dtype=np.uint8)
            assert len(terminal_n) >= n
        b = capi.Batch(seq.ctypes.data, qual.ctypes.data, offset.ctypes.data, n, len(segment_start) - 1,
                       segment_start.ctypes.data, 0, terminal_n.ctypes.data if terminal_n is not None and n else None)
        _check(self.lib, self.lib.faqcs_submit(self.ctx, C.byref(b), res.ctypes.data))
        _check(self.lib, self.lib.faqcs_sync(self.ctx))
        return res

    def emit_device(self, batch, d_results, out, d_keep=None):
        """faqcs_emit_device: packs the trimmed, edited reads of a device-resident batch (a capi.Batch of device pointers, as given to
        faqcs_submit_device, and its device results) into the arenas of `out` (a capi.EmitOut).  Enqueued; sync() waits."""
        _check(self.lib, self.lib.faqcs_emit_device(self.ctx, C.byref(batch), d_results, d_keep, C.byref(out)))

    def emit_time_ms(self):
        """(scan ms, gather ms) of the last emit_device() on this engine (HIP events on the compute stream); waits for it."""
        a, g = C.c_double(), C.c_double()
        _check(self.lib, self.lib.faqcs_emit_time_ms(self.ctx, C.byref(a), C.byref(g)))
        return a.value, g.value

    def parse_device(self, d_text, n_text, final, out):
        """faqcs_parse_device: FASTQ text in device memory (d_text: device address, readable ARENA_PAD_BEFORE bytes in front and
        ARENA_PAD_AFTER behind) -> the packed batch in the arrays of `out` (a capi.ParseOut of device pointers).  Enqueued; sync() waits."""
        _check(self.lib, self.lib.faqcs_parse_device(self.ctx, d_text, int(n_text), 1 if final else 0, C.byref(out)))

    def parse_time_ms(self):
        """(index + records ms, gather ms) of the last parse_device() on this engine (HIP events on the compute stream); waits for it."""
        a, g = C.c_double(), C.c_double()
        _check(self.lib, self.lib.faqcs_parse_time_ms(self.ctx, C.byref(a), C.byref(g)))
        return a.value, g.value

    def render_device(self, batch, d_results, d_text, d_def_pos, d_def_len, out, d_select=None, d_order=None):
        """faqcs_render_device: the FASTQ text of the selected reads of a device-resident batch (a capi.Batch of device pointers, as given to
        faqcs_submit_device) into the arrays of `out` (a capi.RenderOut of device pointers).  d_results: the device results (the trimmed
        records) or None (the original records: the discard stream); d_text / d_def_pos / d_def_len: the text and the defline spans
        faqcs_parse_device delivered; d_select / d_order: optional device arrays (include/faqcs_mi.h).  Enqueued; sync() waits."""
        _check(self.lib, self.lib.faqcs_render_device(self.ctx, C.byref(batch), d_results, d_text, d_def_pos, d_def_len, d_select, d_order, C.byref(out)))

    def render_time_ms(self):
        """(scan ms, gather ms) of the last render_device() on this engine (HIP events on the compute stream); waits for it."""
        a, g = C.c_double(), C.c_double()
        _check(self.lib, self.lib.faqcs_render_time_ms(self.ctx, C.byref(a), C.byref(g)))
        return a.value, g.value

    def pair_device(self, mate1, mate2, d_route, d_info):
        """faqcs_pair_device: the id check, the route and the pair counters of two device-resident mates (capi.Mate each: a host capi.Batch of
        device pointers, the device results or None, the text and the defline spans faqcs_parse_device delivered) into d_route (uint8
        [min of the two n_reads]; None with both results None: check only) and d_info (a faqcs_pair_info in device memory).  Enqueued; sync() waits."""
        _check(self.lib, self.lib.faqcs_pair_device(self.ctx, C.byref(mate1), C.byref(mate2), d_route, d_info))

    def pair_time_ms(self):
        """(check ms, finish ms) of the last pair_device() on this engine (HIP events on the compute stream); waits for it."""
        a, g = C.c_double(), C.c_double()
        _check(self.lib, self.lib.faqcs_pair_time_ms(self.ctx, C.byref(a), C.byref(g)))
        return a.value, g.value

    def render_pair_device(self, file, mate1, mate2, d_route, n_pairs, out):
        """faqcs_render_pair_device: the FASTQ text of one of the four files of a paired run (capi.FILE_*) from the two mates and the route
        pair_device() wrote, into the arrays of `out` (a capi.RenderOut of device pointers; rec_offset / rec_index hold up to 2 n_pairs
        (+ 1) entries).  Enqueued; sync() waits."""
        _check(self.lib, self.lib.faqcs_render_pair_device(self.ctx, int(file), C.byref(mate1), C.byref(mate2), d_route, int(n_pairs), C.byref(out)))

    def render_pair_time_ms(self):
        """(scan ms, gather ms) of the last render_pair_device() on this engine (HIP events on the compute stream); waits for it."""
        a, g = C.c_double(), C.c_double()
        _check(self.lib, self.lib.faqcs_render_pair_time_ms(self.ctx, C.byref(a), C.byref(g)))
        return a.value, g.value

    def inflate_device(self, d_comp, n_comp, d_member_offset, n_members, out):
        """faqcs_inflate_device: BGZF members in device memory (d_comp: device address, any alignment; d_member_offset: device uint32
        [n_members + 1], as bgzf_index_host() found them) -> their text in the arrays of `out` (a capi.InflateOut of device pointers).
        Enqueued; sync() waits."""
        _check(self.lib, self.lib.faqcs_inflate_device(self.ctx, d_comp, int(n_comp), d_member_offset, int(n_members), C.byref(out)))

    def inflate_time_ms(self):
        """(scan ms, decode ms) of the last inflate_device() on this engine (HIP events on the compute stream); waits for it."""
        a, g = C.c_double(), C.c_double()
        _check(self.lib, self.lib.faqcs_inflate_time_ms(self.ctx, C.byref(a), C.byref(g)))
        return a.value, g.value

    def deflate_device(self, d_text, n_text, member_bytes, final, out, mode=capi.DEFLATE_FAST):
        """faqcs_deflate_device_mode (mode: capi.DEFLATE_FAST, what faqcs_deflate_device does, or capi.DEFLATE_DENSE): text in device memory (d_text: device address, any alignment) -> BGZF members of member_bytes bytes of text
        each (0: 65 280) in the arrays of `out` (a capi.DeflateOut of device pointers), the EOF member behind them when final.
        Enqueued; sync() waits."""
        _check(self.lib, self.lib.faqcs_deflate_device_mode(self.ctx, d_text, int(n_text), int(member_bytes), 1 if final else 0, int(mode), C.byref(out)))

    def deflate_time_ms(self):
        """(encode ms, gather ms) of the last deflate_device() on this engine (HIP events on the compute stream); waits for it."""
        a, g = C.c_double(), C.c_double()
        _check(self.lib, self.lib.faqcs_deflate_time_ms(self.ctx, C.byref(a), C.byref(g)))
        return a.value, g.value

    def gunzip_device(self, d_comp, n_comp, out, piece_bytes=0, max_rounds=0):
        """faqcs_gunzip_device: ordinary gzip in device memory (d_comp: device address, any alignment; whole members) -> its text in the
        arrays of `out` (a capi.GunzipOut of device pointers).  Unlike the other seam calls this one BLOCKS: text and info are complete
        when it returns."""
        _check(self.lib, self.lib.faqcs_gunzip_device(self.ctx, d_comp, int(n_comp), int(piece_bytes), int(max_rounds), C.byref(out)))

    def gunzip_stream_device(self, d_comp, n_comp, final, state, out, piece_bytes=0, max_rounds=0):
        """faqcs_gunzip_stream_device: one chunk of an ordinary gzip file in device memory (d_comp: the file from where the previous call's
        consumed left it) -> this call's text in the arrays of `out`; state: the file's capi.GunzipState in host memory, its window in
        device memory.  The call BLOCKS, as gunzip_device() does."""
        _check(self.lib, self.lib.faqcs_gunzip_stream_device(self.ctx, d_comp, int(n_comp), 1 if final else 0, int(piece_bytes), int(max_rounds),
                                                             C.byref(state), C.byref(out)))

    def gunzip_time_ms(self):
        """(count ms, decode ms, resolve ms) of the last gunzip_device() or gunzip_stream_device() on this engine (HIP events on the compute stream)."""
        a, g, r = C.c_double(), C.c_double(), C.c_double()
        _check(self.lib, self.lib.faqcs_gunzip_time_ms(self.ctx, C.byref(a), C.byref(g), C.byref(r)))
        return a.value, g.value, r.value

    def gunzip_host(self, comp, piece_bytes=0, max_rounds=0, capacity=None):
        """gunzip_host() of this module on the engine's library."""
        return gunzip_host(comp, piece_bytes, max_rounds, capacity, self.lib)

    def bgzf_index_device(self, d_comp, n_comp, final, d_member_offset, capacity_members, d_info):
        """faqcs_bgzf_index_device: where the BGZF members of compressed bytes in device memory are (d_comp: device address, any alignment)
        -> d_member_offset (device uint32 [capacity_members + 1]) and d_info (a faqcs_bgzf_index_info in device memory), field for field
        what bgzf_index_host() finds.  Enqueued; sync() waits."""
        _check(self.lib, self.lib.faqcs_bgzf_index_device(self.ctx, d_comp, int(n_comp), 1 if final else 0, d_member_offset, int(capacity_members), d_info))

    def bgzf_index_time_ms(self):
        """(candidates ms, chain ms) of the last bgzf_index_device() on this engine (HIP events on the compute stream); waits for it."""
        a, g = C.c_double(), C.c_double()
        _check(self.lib, self.lib.faqcs_bgzf_index_time_ms(self.ctx, C.byref(a), C.byref(g)))
        return a.value, g.value

    def bgzf_index_host(self, comp, final=True):
        """bgzf_index_host() of this module on the engine's library."""
        return bgzf_index_host(comp, final, self.lib)

    def set_quality(self, q):
        _check(self.lib, self.lib.faqcs_set_quality(self.ctx, int(q)))

    def set_input_quality_offset(self, offset):
        """faqcs_set_input_quality_offset: the input quality offset of every LATER submission, emission and rendering (what auto-detection
        found).  Waits for the work enqueued so far, which keeps the old offset."""
        _check(self.lib, self.lib.faqcs_set_input_quality_offset(self.ctx, int(offset)))
        self.holder.p.input_quality_offset = int(offset)

    def detect_device(self, batch, first, count, d_info, d_text=None, d_def_pos=None, d_def_len=None):
        """faqcs_detect_device: the first decisive quality byte of reads [first, first + count) of a device-resident batch (a capi.Batch of
        device pointers; only qual, offset and n_reads are read) and, with d_text / d_def_pos / d_def_len (all three or none), whether the
        defline of read `first` starts with "@NS", into d_info (a faqcs_detect_info in device memory).  Enqueued; sync() waits."""
        _check(self.lib, self.lib.faqcs_detect_device(self.ctx, C.byref(batch), int(first), int(count), d_text, d_def_pos, d_def_len, d_info))

    def first_error_device(self, d_results, n, d_info):
        """faqcs_first_error_device: the first of n device results with an F_ERR_* bit into d_info (a faqcs_error_info in device memory).
        Enqueued behind the submission that fills d_results; sync() waits."""
        _check(self.lib, self.lib.faqcs_first_error_device(self.ctx, d_results, int(n), d_info))

    def sync(self):
        _check(self.lib, self.lib.faqcs_sync(self.ctx))

    # -- accumulators ------------------------------------------------------------------------------
    def counters_device(self):
        ptr, n = C.c_void_p(), C.c_uint64()
        _check(self.lib, self.lib.faqcs_counters_device(self.ctx, C.byref(ptr), C.byref(n)))
        return ptr.value, int(n.value)

    def counters_export(self, d_dst, n_u64):
        """Device-to-device copy of the block into a caller-owned buffer (the buffer the collective runs on)."""
        _check(self.lib, self.lib.faqcs_counters_export(self.ctx, d_dst, int(n_u64)))

    def counters_import(self, d_src, n_u64):
        _check(self.lib, self.lib.faqcs_counters_import(self.ctx, d_src, int(n_u64)))

    def comm_init(self, comm_id, rank, world):
        """The library's own RCCL communicator (include/faqcs_mi.h): comm_id = the FAQCS_COMM_ID_BYTES bytes rank 0 got from comm_id()."""
        buf = C.create_string_buffer(bytes(comm_id), 128)
        _check(self.lib, self.lib.faqcs_comm_init(self.ctx, buf, int(rank), int(world)))
        self.has_comm = True

    def comm_id(self):
        buf = C.create_string_buffer(128)
        _check(self.lib, self.lib.faqcs_comm_id(buf))
        return buf.raw

    def comm_allreduce_counters(self):
        """All-reduce(sum) of the counter block in place, enqueued on the context's compute stream (no copy, no host sync)."""
        _check(self.lib, self.lib.faqcs_comm_allreduce_counters(self.ctx))

    def counters(self):
        out = np.zeros(self.n_counters, dtype=np.uint64)
        _check(self.lib, self.lib.faqcs_finish(self.ctx, out.ctypes.data, self.n_counters))
        return out

    def kmer_active(self):
        return bool(self.lib.faqcs_kmer_active(self.ctx))

    def kmer_points(self):
        n = C.c_uint32()
        _check(self.lib, self.lib.faqcs_kmer_points(self.ctx, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=capi.RAREFACTION_DTYPE)
        if n.value:
            _check(self.lib, self.lib.faqcs_kmer_points(self.ctx, out.ctypes.data, n.value, C.byref(n)))
        return out

    def kmer_end_table(self):
        """process_paired / process_unpaired epilogue (FaQCs.cpp:518-537, :737-756)."""
        _check(self.lib, self.lib.faqcs_kmer_end_table(self.ctx))

    def kmer_finish_pass(self):
        """The pass is complete: its k-mers are counted (in one piece, without the device table, when they fit the group buffers)."""
        _check(self.lib, self.lib.faqcs_kmer_finish_pass(self.ctx))

    def kmer_totals(self):
        d, t = C.c_uint64(), C.c_uint64()
        _check(self.lib, self.lib.faqcs_kmer_totals(self.ctx, C.byref(d), C.byref(t)))
        return int(d.value), int(t.value)

    def kmer_histogram(self):
        n = C.c_uint64()
        _check(self.lib, self.lib.faqcs_kmer_histogram(self.ctx, None, None, 0, C.byref(n)))
        c = np.zeros(n.value, dtype=np.uint64)
        k = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            _check(self.lib, self.lib.faqcs_kmer_histogram(self.ctx, c.ctypes.data, k.ctypes.data, n.value, C.byref(n)))
        return c, k

    # -- k-mers across GPUs (owner-partitioned tables; faqcs_amd/parallel.py drives the exchange) --------------
    def kmer_partition(self, rank, world, n_epochs):
        self._part = (rank, world, n_epochs)
        _check(self.lib, self.lib.faqcs_kmer_partition(self.ctx, rank, world, n_epochs))

    def kmer_set_epochs(self, epochs):
        e = np.ascontiguousarray(epochs, dtype=np.uint32)
        _check(self.lib, self.lib.faqcs_kmer_set_epochs(self.ctx, e.ctypes.data, len(e)))

    def kmer_outbox(self):
        """(device pointer to the (key, epoch) pairs grouped by destination, pairs per destination)."""
        ptr = C.c_void_p()
        counts = np.zeros(self._part[1], dtype=np.uint64)
        _check(self.lib, self.lib.faqcs_kmer_outbox(self.ctx, C.byref(ptr), counts.ctypes.data))
        return ptr.value, counts

    def kmer_insert_device(self, d_items, n_items):
        _check(self.lib, self.lib.faqcs_kmer_insert_device(self.ctx, d_items, int(n_items)))

    def kmer_epoch_counts(self):
        n = self._part[2]
        d = np.zeros(n, dtype=np.uint64)
        t = np.zeros(n, dtype=np.uint64)
        _check(self.lib, self.lib.faqcs_kmer_epoch_counts(self.ctx, d.ctypes.data, t.ctypes.data, n))
        return d, t

    def close(self):
        if self.ctx:
            self.lib.faqcs_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
