"""ctypes view of include/faqcs_mi.h (the C ABI of libfaqcs_mi.so) and the data model shared with the
test oracle.  No torch types cross this boundary: numpy arrays / raw pointers only."""
import ctypes as C
import os

import numpy as np

ABI_VERSION = 2
NUM_STAT = 25
NQ = 42
NBASE = 5
NCOMP_BIN = 10001
NCOMP_KIND = 6
SEGMENT_READS = 32768
MAX_READ_LENGTH = 32767       # FAQCS_MAX_READ_LENGTH: longest read the library takes (batches with a read > 1 024 bases run on trim_long)
FAST_READ_LENGTH = 1024       # longest read of the chunked kernels
ARENA_PAD_BEFORE, ARENA_PAD_AFTER = 16, 64  # FAQCS_ARENA_PAD_*: readable bytes in front of / behind a device-resident batch's arenas

(TOTAL_COUNT, TOTAL_NUMBER, TOTAL_LENGTH, TOTAL_TRIMMED_NUMBER, TOTAL_TRIMMED_LENGTH, PAIRED_READ_NUMBER,
 PAIRED_BASE_LENGTH, READ_LENGTH, BASE_LENGTH, READ_NN, BASE_NN, READ_PHIX, BASE_PHIX, READ_ADAPTER,
 BASE_ADAPTER, READ_AVG_Q, BASE_AVG_Q, READ_QUAL_TRIM, BASE_QUAL_TRIM, READ_LOW_COMPLEXITY,
 BASE_LOW_COMPLEXITY, N_TO_A, N_TO_T, N_TO_G, N_TO_C) = range(NUM_STAT)

F_VALID, F_FILTER_MASK, F_FILTER_SHIFT = 0x1, 0xE, 1
F_QUAL_TRIMMED, F_ADAPTER, F_POLY_N_SEEN, F_ERR_QUALITY, F_ERR_BASE = 0x10, 0x20, 0x40, 0x100, 0x200

E_INVAL, E_NODEVICE, E_QUALITY, E_BASE, E_NOMEM, E_KMER_FULL = -1, -2, -3, -4, -5, -6
EPOCH_NONE = 0xFFFFFFFF

# the messages the reference throws at the corresponding sites (fastq.h:32, seq_overlap.cpp:409)
ERR_TEXT = {
    E_QUALITY: "fastq.h:quality_score: Found a quality score value that is greater than the maximum allowed quality score",
    E_BASE: "seq_overlap.cpp:na_to_bits: Unknown base!",
}


class Params(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("mode", C.c_int32), ("quality", C.c_int32),
        ("input_quality_offset", C.c_int32), ("output_quality_offset", C.c_int32),
        ("min_read_length", C.c_uint32), ("max_num_poly_N", C.c_uint32), ("trim_5", C.c_uint32),
        ("trim_3", C.c_uint32), ("replace_to_N_q", C.c_uint32), ("average_quality", C.c_float),
        ("low_complexity_cutoff_ratio", C.c_float), ("filterAdapterMismatchRate", C.c_float),
        ("protect_5", C.c_uint32), ("qc_only", C.c_uint32), ("kmer_rarefaction", C.c_uint32),
        ("kmer", C.c_uint32), ("split_size", C.c_uint32), ("num_subsample", C.c_uint32),
        ("max_read_length", C.c_uint32), ("n_adapters", C.c_uint32),
        ("adapter_seq", C.POINTER(C.c_char_p)), ("kmer_table_slots", C.c_uint64),
    ]


class Batch(C.Structure):
    _fields_ = [
        ("seq", C.c_void_p), ("qual", C.c_void_p), ("offset", C.c_void_p), ("n_reads", C.c_uint32),
        ("n_segments", C.c_uint32), ("segment_start", C.c_void_p), ("max_read_len", C.c_uint32),
        ("terminal_n", C.c_void_p),  # optional per-read flags (faqcs_submit_device only); None = the kernels look themselves
    ]


class EmitInfo(C.Structure):
    """faqcs_emit_info: what an emission needs (always) and whether it fitted."""
    _fields_ = [("n_bytes", C.c_uint64), ("n_reads", C.c_uint32), ("overflow", C.c_uint32)]


class EmitOut(C.Structure):
    """faqcs_emit_out: device pointers of the caller's output arenas (faqcs_emit_device)."""
    _fields_ = [("seq", C.c_void_p), ("qual", C.c_void_p), ("capacity_bytes", C.c_uint64), ("offset", C.c_void_p),
                ("index", C.c_void_p), ("info", C.c_void_p)]


class RenderInfo(C.Structure):
    """faqcs_render_info: what a rendering needs (always) and whether it fitted."""
    _fields_ = [("n_bytes", C.c_uint64), ("n_reads", C.c_uint32), ("overflow", C.c_uint32)]


class RenderOut(C.Structure):
    """faqcs_render_out: the caller's output arrays (device pointers for faqcs_render_device, host pointers for faqcs_render_host)."""
    _fields_ = [("text", C.c_void_p), ("capacity_bytes", C.c_uint64), ("rec_offset", C.c_void_p), ("rec_index", C.c_void_p), ("info", C.c_void_p)]


class Mate(C.Structure):
    """faqcs_mate: one mate's buffer as faqcs_parse_device + faqcs_submit_device left it.  `batch` points to a Batch in host memory (keep it
    alive); the other pointers are device pointers for the device forms, host pointers for the host forms."""
    _fields_ = [("batch", C.POINTER(Batch)), ("results", C.c_void_p), ("text", C.c_void_p), ("def_pos", C.c_void_p), ("def_len", C.c_void_p)]


class PairInfo(C.Structure):
    """faqcs_pair_info: the pairs routed, the first pair whose ids differ, and the two FilterStat slots that depend on both mates."""
    _fields_ = [("paired_read_number", C.c_uint64), ("paired_base_length", C.c_uint64), ("n_pairs", C.c_uint32), ("mismatch", C.c_uint32),
                ("id_len", C.c_uint32 * 2), ("n_one_valid", C.c_uint32), ("n_none_valid", C.c_uint32)]


class DetectInfo(C.Structure):
    """faqcs_detect_info: the first decisive quality byte of a range of reads (33 / 64, or 0: none), the read that owns it, and whether the
    range's first defline starts with "@NS"."""
    _fields_ = [("quality_offset", C.c_int32), ("read", C.c_uint32), ("pos", C.c_uint32), ("byte", C.c_uint32), ("next_seq", C.c_uint32),
                ("reserved", C.c_uint32)]


class ErrorInfo(C.Structure):
    """faqcs_error_info: the reads in front of the first one with an F_ERR_* bit, and that read's error bits."""
    _fields_ = [("n_good", C.c_uint32), ("flags", C.c_uint32)]


ROUTE_V1, ROUTE_V2, ROUTE_NOWHERE = 1, 2, 0x80
FILE_QC1, FILE_QC2, FILE_UNPAIRED, FILE_DISCARD = range(4)
# the reference's names of the four files of a paired run, by FAQCS_FILE_* code
PAIR_FILES = ("QC.1.trimmed.fastq", "QC.2.trimmed.fastq", "QC.unpaired.trimmed.fastq", "QC.discard.trimmed.fastq")

# FAQCS_INFLATE_*: faqcs_inflate_info.error / faqcs_bgzf_index_info.error, the error of member n_members
INFLATE_OK, INFLATE_E_HEADER, INFLATE_E_LENGTH, INFLATE_E_DATA, INFLATE_E_CRC, INFLATE_E_TRUNCATED = range(6)
INFLATE_E_SERIAL = 16  # faqcs_gunzip_info.error only: the stream does not split into pieces


class BgzfIndexInfo(C.Structure):
    """faqcs_bgzf_index_info: the whole members of a chunk of BGZF bytes and where the next chunk starts."""
    _fields_ = [("consumed", C.c_uint64), ("n_members", C.c_uint32), ("overflow", C.c_uint32), ("error", C.c_int32), ("reserved", C.c_uint32)]


class InflateInfo(C.Structure):
    """faqcs_inflate_info: what the text of the members needs (always), whether it fitted, and the first bad member."""
    _fields_ = [("n_bytes", C.c_uint64), ("n_members", C.c_uint32), ("overflow", C.c_uint32), ("error", C.c_int32), ("reserved", C.c_uint32)]


class InflateOut(C.Structure):
    """faqcs_inflate_out: the caller's output arrays (device pointers for faqcs_inflate_device, host pointers for faqcs_inflate_host)."""
    _fields_ = [("text", C.c_void_p), ("capacity_bytes", C.c_uint64), ("member_text_offset", C.c_void_p), ("info", C.c_void_p)]


class GunzipInfo(C.Structure):
    """faqcs_gunzip_info: what the text of the members needs, the bytes they cover, the first bad member, and what the speculation did."""
    _fields_ = [("n_bytes", C.c_uint64), ("consumed", C.c_uint64), ("n_members", C.c_uint32), ("overflow", C.c_uint32), ("error", C.c_int32),
                ("n_pieces", C.c_uint32), ("n_fixups", C.c_uint32), ("n_rounds", C.c_uint32)]


class GunzipOut(C.Structure):
    """faqcs_gunzip_out: the caller's output (device pointers for faqcs_gunzip_device, host pointers for faqcs_gunzip_host)."""
    _fields_ = [("text", C.c_void_p), ("capacity_bytes", C.c_uint64), ("info", C.c_void_p)]


GUNZIP_DEFAULT_PIECE, GUNZIP_DEFAULT_ROUNDS = 64 << 10, 32  # what piece_bytes = 0 and max_rounds = 0 mean

# FAQCS_GUNZIP_*: faqcs_gunzip_state.phase, what the next call's first byte is
GUNZIP_BETWEEN, GUNZIP_STREAM, GUNZIP_TRAILER = range(3)
GUNZIP_WINDOW = 32768  # bytes of faqcs_gunzip_state.window


class GunzipState(C.Structure):
    """faqcs_gunzip_state: what faqcs_gunzip_stream_device / _host carry from one call on a file to the next.  Host memory; all zero but
    `window` (device memory for _device, host memory for _host) before a file's first call."""
    _fields_ = [("member_bytes", C.c_uint64), ("total_bytes", C.c_uint64), ("total_comp", C.c_uint64), ("phase", C.c_uint32), ("bit", C.c_uint32),
                ("crc", C.c_uint32), ("window_bytes", C.c_uint32), ("members", C.c_uint32), ("reserved", C.c_uint32), ("window", C.c_void_p)]


class DeflateInfo(C.Structure):
    """faqcs_deflate_info: what the members need (always), whether they fitted, and how many of them hold a stored block."""
    _fields_ = [("n_bytes", C.c_uint64), ("n_members", C.c_uint32), ("overflow", C.c_uint32), ("n_stored", C.c_uint32), ("reserved", C.c_uint32)]


class DeflateOut(C.Structure):
    """faqcs_deflate_out: the caller's output arrays (device pointers for faqcs_deflate_device, host pointers for faqcs_deflate_host)."""
    _fields_ = [("comp", C.c_void_p), ("capacity_bytes", C.c_uint64), ("member_offset", C.c_void_p), ("info", C.c_void_p)]


DEFLATE_FAST, DEFLATE_DENSE = 0, 1  # FAQCS_DEFLATE_*: the match finder of faqcs_deflate_device_mode / faqcs_deflate_host_mode


# FAQCS_PARSE_*: faqcs_parse_info.error, the error of record n_reads
PARSE_OK, PARSE_E_SEQUENCE, PARSE_E_PLUS, PARSE_E_PLUS_DELIM, PARSE_E_QUALITY, PARSE_E_LENGTH = range(6)


class ParseInfo(C.Structure):
    """faqcs_parse_info: what the parsed records need (always), the text they cover, and whether they fitted."""
    _fields_ = [("n_bytes", C.c_uint64), ("consumed", C.c_uint64), ("n_reads", C.c_uint32), ("max_read_len", C.c_uint32),
                ("overflow", C.c_uint32), ("error", C.c_int32)]


class ParseOut(C.Structure):
    """faqcs_parse_out: the caller's output arrays (device pointers for faqcs_parse_device, host pointers for faqcs_parse_host)."""
    _fields_ = [("seq", C.c_void_p), ("qual", C.c_void_p), ("capacity_bytes", C.c_uint64), ("capacity_reads", C.c_uint32),
                ("offset", C.c_void_p), ("terminal_n", C.c_void_p), ("def_pos", C.c_void_p), ("def_len", C.c_void_p), ("info", C.c_void_p)]


class Layout(C.Structure):
    _fields_ = [("max_read_length", C.c_uint32), ("n_adapters", C.c_uint32)] + [
        (n, C.c_uint64) for n in (
            "filter_stats", "pre_read_qhist", "pre_base_qhist", "post_read_qhist", "post_base_qhist",
            "pre_len_hist", "post_len_hist", "pre_qual", "post_qual", "pre_base", "post_base", "pre_comp",
            "post_comp", "adapter_stats", "total")
    ]


class KernelTimes(C.Structure):
    _fields_ = [("trim_ms", C.c_double), ("adapter_ms", C.c_double), ("n_launches", C.c_uint64), ("trim_kernel", C.c_char_p),
                ("kmer_ms", C.c_double), ("kmer_insert_ms", C.c_double)]


class PathTallies(C.Structure):
    """faqcs_path_tallies: which arm of the host orchestration the calls on a context took (host-side counts, faqcs_path_tallies_get)."""
    _fields_ = [(n, C.c_uint64) for n in ("folds_tail", "folds_aux", "folds_now", "folds_dropped", "slot_stream_waits", "slot_event_syncs",
                                          "recset_fold_waits", "recset_grow_syncs", "ticket_ring_waits")]


RESULT_DTYPE = np.dtype([("start", "<u2"), ("len", "<u2"), ("flags", "<u2"), ("adapter", "<u2")])
RAREFACTION_DTYPE = np.dtype([("num_seq", "<u8"), ("distinct_kmer", "<u8"), ("total_kmer", "<u8")])


def python_layout(R, n_adapters):
    """Pure-python statement of the counter-block layout (tests assert the C library and the oracle agree)."""
    o, out = 0, {}
    for name, size in (
        ("filter_stats", 32), ("pre_read_qhist", NQ), ("pre_base_qhist", NQ), ("post_read_qhist", NQ),
        ("post_base_qhist", NQ), ("pre_len_hist", R + 1), ("post_len_hist", R + 1), ("pre_qual", R * NQ),
        ("post_qual", R * NQ), ("pre_base", R * NBASE), ("post_base", R * NBASE),
        ("pre_comp", NCOMP_BIN * NCOMP_KIND), ("post_comp", NCOMP_BIN * NCOMP_KIND),
        ("adapter_stats", 2 * n_adapters),
    ):
        out[name] = (o, size)
        o += size
    out["total"] = o
    return out


class ParamsHolder:
    """Keeps the ctypes Params struct and the adapter string array alive together."""

    def __init__(self, opt, max_read_length, input_quality_offset=None, kmer_table_slots=0):
        seqs = [a[1].encode() for a in opt.adapter] if opt.adapters_active() else []
        self._arr = (C.c_char_p * max(1, len(seqs)))(*seqs)
        off = opt.input_quality_offset if input_quality_offset is None else input_quality_offset
        self.p = Params(
            abi_version=ABI_VERSION, mode=opt.mode, quality=opt.quality, input_quality_offset=off,
            output_quality_offset=opt.output_quality_offset, min_read_length=opt.min_read_length,
            max_num_poly_N=opt.max_num_poly_N, trim_5=opt.trim_5, trim_3=opt.trim_3,
            replace_to_N_q=opt.replace_to_N_q, average_quality=opt.average_quality,
            low_complexity_cutoff_ratio=opt.low_complexity_cutoff_ratio,
            filterAdapterMismatchRate=opt.filterAdapterMismatchRate, protect_5=int(opt.protect_5),
            qc_only=int(opt.qc_only), kmer_rarefaction=int(opt.kmer_rarefaction), kmer=opt.kmer,
            split_size=opt.split_size, num_subsample=opt.num_subsample, max_read_length=max_read_length,
            n_adapters=len(seqs), adapter_seq=C.cast(self._arr, C.POINTER(C.c_char_p)),
            kmer_table_slots=kmer_table_slots,
        )
        self.n_adapters = len(seqs)
        self.max_read_length = max_read_length


_LIB = None


def lib_path():
    # FAQCS_MI_LIB lets a tuning run point at an alternative build of the same library
    return os.environ.get("FAQCS_MI_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfaqcs_mi.so")


def load_library():
    """Loads libfaqcs_mi.so (built in-tree by __graft_entry__.build()).  Fails loudly: there is no CPU
    fallback for the product path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            "libfaqcs_mi.so is missing (%s): build the HIP extension with `python -c 'import __graft_entry__ as g; "
            "g.build()'` -- the FaQCs MI355X hot path has no CPU fallback" % path)
    lib = C.CDLL(path)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    sig = {
        "faqcs_abi_version": (i32, []),
        "faqcs_counters_layout": (i32, [u32, u32, C.POINTER(Layout)]),
        "faqcs_counter_rows": (u32, [vp, u32, u32]),
        "faqcs_apply_edits": (i32, [C.POINTER(Params), vp, vp, u32, vp, vp, vp]),
        "faqcs_auto_detect_quality_offset": (i32, [vp, vp, u32]),
        "faqcs_last_error": (C.c_char_p, []),
        "faqcs_create": (i32, [C.POINTER(Params), i32, C.POINTER(vp)]),
        "faqcs_destroy": (None, [vp]),
        "faqcs_submit": (i32, [vp, C.POINTER(Batch), vp]),
        "faqcs_submit_device": (i32, [vp, C.POINTER(Batch), vp]),
        "faqcs_sync": (i32, [vp]),
        "faqcs_emit_device": (i32, [vp, C.POINTER(Batch), vp, vp, C.POINTER(EmitOut)]),
        "faqcs_parse_error_text": (C.c_char_p, [i32]),
        "faqcs_parse_device": (i32, [vp, vp, u64, i32, C.POINTER(ParseOut)]),
        "faqcs_parse_host": (i32, [vp, u64, i32, C.POINTER(ParseOut)]),
        "faqcs_parse_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "faqcs_render_device": (i32, [vp, C.POINTER(Batch), vp, vp, vp, vp, vp, vp, C.POINTER(RenderOut)]),
        "faqcs_render_host": (i32, [C.POINTER(Params), C.POINTER(Batch), vp, vp, vp, vp, vp, vp, C.POINTER(RenderOut)]),
        "faqcs_render_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "faqcs_pair_device": (i32, [vp, C.POINTER(Mate), C.POINTER(Mate), vp, vp]),
        "faqcs_pair_host": (i32, [C.POINTER(Mate), C.POINTER(Mate), vp, vp]),
        "faqcs_pair_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "faqcs_render_pair_device": (i32, [vp, i32, C.POINTER(Mate), C.POINTER(Mate), vp, u32, C.POINTER(RenderOut)]),
        "faqcs_render_pair_host": (i32, [C.POINTER(Params), i32, C.POINTER(Mate), C.POINTER(Mate), vp, u32, C.POINTER(RenderOut)]),
        "faqcs_render_pair_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "faqcs_inflate_error_text": (C.c_char_p, [i32]),
        "faqcs_bgzf_index_host": (i32, [vp, u64, i32, vp, u32, C.POINTER(BgzfIndexInfo)]),
        "faqcs_bgzf_index_device": (i32, [vp, vp, u64, i32, vp, u32, vp]),
        "faqcs_bgzf_index_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "faqcs_inflate_device": (i32, [vp, vp, u64, vp, u32, C.POINTER(InflateOut)]),
        "faqcs_inflate_host": (i32, [vp, u64, vp, u32, C.POINTER(InflateOut)]),
        "faqcs_inflate_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "faqcs_gunzip_device": (i32, [vp, vp, u64, u32, u32, C.POINTER(GunzipOut)]),
        "faqcs_gunzip_host": (i32, [vp, u64, u32, u32, C.POINTER(GunzipOut)]),
        "faqcs_gunzip_stream_device": (i32, [vp, vp, u64, i32, u32, u32, C.POINTER(GunzipState), C.POINTER(GunzipOut)]),
        "faqcs_gunzip_stream_host": (i32, [vp, u64, i32, u32, u32, C.POINTER(GunzipState), C.POINTER(GunzipOut)]),
        "faqcs_gunzip_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "faqcs_deflate_device": (i32, [vp, vp, u64, u32, i32, C.POINTER(DeflateOut)]),
        "faqcs_deflate_host": (i32, [vp, u64, u32, i32, C.POINTER(DeflateOut)]),
        "faqcs_deflate_device_mode": (i32, [vp, vp, u64, u32, i32, i32, C.POINTER(DeflateOut)]),
        "faqcs_deflate_host_mode": (i32, [vp, u64, u32, i32, i32, C.POINTER(DeflateOut)]),
        "faqcs_deflate_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "faqcs_submit_async": (i32, [vp, C.POINTER(Batch), vp, C.POINTER(u64)]),
        "faqcs_wait": (i32, [vp, u64]),
        "faqcs_host_alloc": (vp, [C.c_size_t]),
        "faqcs_host_free": (None, [vp]),
        "faqcs_path_tallies_get": (i32, [vp, C.POINTER(PathTallies)]),
        "faqcs_counters_device": (i32, [vp, C.POINTER(vp), C.POINTER(u64)]),
        "faqcs_counters_export": (i32, [vp, vp, u64]),
        "faqcs_counters_import": (i32, [vp, vp, u64]),
        "faqcs_finish": (i32, [vp, vp, u64]),
        "faqcs_reset_counters": (i32, [vp]),
        "faqcs_set_quality": (i32, [vp, i32]),
        "faqcs_set_input_quality_offset": (i32, [vp, i32]),
        "faqcs_detect_device": (i32, [vp, C.POINTER(Batch), u32, u32, vp, vp, vp, vp]),
        "faqcs_detect_host": (i32, [C.POINTER(Batch), u32, u32, vp, vp, vp, vp]),
        "faqcs_first_error_device": (i32, [vp, vp, u32, vp]),
        "faqcs_first_error_host": (i32, [vp, u32, vp]),
        "faqcs_kmer_points": (i32, [vp, vp, u32, C.POINTER(u32)]),
        "faqcs_kmer_histogram": (i32, [vp, vp, vp, u64, C.POINTER(u64)]),
        "faqcs_kmer_totals": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "faqcs_kmer_active": (i32, [vp]),
        "faqcs_kmer_end_table": (i32, [vp]),
        "faqcs_kmer_finish_pass": (i32, [vp]),
        "faqcs_kmer_memory_plan": (i32, [vp, u64, vp, u32]),
        "faqcs_kmer_partition": (i32, [vp, u32, u32, u32]),
        "faqcs_kmer_set_epochs": (i32, [vp, vp, u32]),
        "faqcs_kmer_outbox": (i32, [vp, C.POINTER(vp), vp]),
        "faqcs_kmer_outbox_host": (i32, [vp, vp, u64, C.POINTER(u64)]),
        "faqcs_kmer_insert_device": (i32, [vp, vp, u64]),
        "faqcs_kmer_epoch_counts": (i32, [vp, vp, vp, u32]),
        "faqcs_kmer_forward": (i32, [vp, vp, u32]),
        "faqcs_comm_id": (i32, [vp]),
        "faqcs_comm_init": (i32, [vp, vp, u32, u32]),
        "faqcs_comm_allreduce_counters": (i32, [vp]),
        "faqcs_comm_init_all": (i32, [vp, u32]),
        "faqcs_comm_allreduce_counters_all": (i32, [vp, u32]),
        "faqcs_synth_fill": (i32, [i32, vp, vp, vp, u32, u32, u64, u64, C.c_float]),
        "faqcs_synth_fill_genome": (i32, [i32, vp, vp, vp, u32, u32, u64, u64, u64]),
        "faqcs_terminal_n_flags": (i32, [i32, vp, vp, u32, vp]),
        "faqcs_emit_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "faqcs_kernel_time_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(u64)]),
        "faqcs_debug_words": (i32, [vp, vp, u32]),
        "faqcs_kernel_report": (i32, [vp, C.POINTER(KernelTimes)]),
    }
    # an alternative build named by FAQCS_MI_LIB (a tuning or checking build of the same kernels) may be older than the observation-only entry
    # points: it loads without them, and a caller that asks for one gets ctypes' AttributeError.  The product library must export them all
    observers = {"faqcs_path_tallies_get"} if os.environ.get("FAQCS_MI_LIB") else set()
    for name, (res, args) in sig.items():
        if name in observers and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError == a symbol the header declares is missing
        fn.restype = res
        fn.argtypes = args
    lib._faqcs_symbols = sorted(sig)
    _LIB = lib
    return lib


def declared_symbols():
    """Every `faqcs_*(` function include/faqcs_mi.h declares (parsed from the header itself)."""
    import re

    hdr = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "faqcs_mi.h")
    text = open(hdr).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(faqcs_[a-z0-9_]+)\s*\(", text)))
