/*
 * faqcs_mi.h -- C ABI of libfaqcs_mi.so: the MI355X (gfx950) implementation of the FaQCs per-read
 * trim / filter / accumulate hot path.
 *
 * Drop-in boundary.  The reference (LANL-Bioinformatics/FaQCs v2.10) has no FFI; the seam this
 * library replaces is the C++ function
 *
 *     void trim(std::vector<Read>&, std::vector<size_t>& filter_stats,
 *               MAP<std::string, std::pair<size_t,size_t>>& adapter_stats,
 *               MAP<Word,size_t>& kmer_table, PlotInfo&, Options&);        // FaQCs.h:245-248
 *
 * whose six call sites are FaQCs.cpp:287,290,424,427 (paired) and :628,:692 (unpaired).  One
 * reference trim() call == one *segment* of a faqcs_batch here.  integration/trim_shim.cpp is the
 * ~150-line C++ adapter a maintainer would compile in place of trim.o.
 *
 * Conventions: plain pointers and sizes only, no C++ / torch types; the caller owns every host
 * buffer; the library owns device memory and HIP streams; every entry point returns 0 or a negative
 * FAQCS_E_* code and faqcs_last_error() gives the text; no exceptions cross the boundary.
 */
#ifndef FAQCS_MI_H
#define FAQCS_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: faqcs_batch.terminal_n, faqcs_terminal_n_flags, the k-mer timers of faqcs_kernel_times.  Entry points added since then leave
 * every existing structure and call as it was, so the number stands: faqcs_kmer_forward, faqcs_comm_* (round 4).  Round 5 changes what the
 * 16-byte items of the k-mer exchange MEAN (faqcs_kmer_outbox / _insert_device / _forward: opaque to every caller in this repository, which
 * only moves them) -- a run of up to 17 consecutive k-mers each instead of one (key, epoch) pair -- and nothing about their size or the calls.
 * Round 6 adds faqcs_kmer_finish_pass, and faqcs_sync() no longer counts the k-mers that wait in the open group (see below).
 * faqcs_emit_device (the trimmed, edited reads packed on the device) is a new entry point with structures of its own, and so are
 * faqcs_parse_device / faqcs_parse_host (FASTQ text to a packed batch) and faqcs_render_device / faqcs_render_host (the FASTQ text of the
 * output files), and faqcs_inflate_device / faqcs_inflate_host / faqcs_bgzf_index_host / faqcs_bgzf_index_device (BGZF members to that text),
 * and faqcs_gunzip_device / faqcs_gunzip_host (ordinary gzip to that text; FAQCS_INFLATE_E_SERIAL is theirs alone),
 * and faqcs_deflate_device / faqcs_deflate_host (text to BGZF members), and faqcs_pair_device / faqcs_pair_host /
 * faqcs_render_pair_device / faqcs_render_pair_host (the two mates of a paired run from two batches), and faqcs_detect_device /
 * faqcs_detect_host / faqcs_first_error_device / faqcs_first_error_host / faqcs_set_input_quality_offset (the decisions around trim()), and faqcs_path_tallies_get (read-only, a structure of its own). */
#define FAQCS_ABI_VERSION 2

/* FilterStat enum order, FaQCs.h:46-75 */
enum {
    FAQCS_TOTAL_COUNT = 0, FAQCS_TOTAL_NUMBER, FAQCS_TOTAL_LENGTH, FAQCS_TOTAL_TRIMMED_NUMBER,
    FAQCS_TOTAL_TRIMMED_LENGTH, FAQCS_PAIRED_READ_NUMBER, FAQCS_PAIRED_BASE_LENGTH, FAQCS_READ_LENGTH,
    FAQCS_BASE_LENGTH, FAQCS_READ_NN, FAQCS_BASE_NN, FAQCS_READ_PHIX, FAQCS_BASE_PHIX,
    FAQCS_READ_ADAPTER, FAQCS_BASE_ADAPTER, FAQCS_READ_AVG_Q, FAQCS_BASE_AVG_Q, FAQCS_READ_QUAL_TRIM,
    FAQCS_BASE_QUAL_TRIM, FAQCS_READ_LOW_COMPLEXITY, FAQCS_BASE_LOW_COMPLEXITY, FAQCS_N_TO_A,
    FAQCS_N_TO_T, FAQCS_N_TO_G, FAQCS_N_TO_C, FAQCS_NUM_STAT
};

#define FAQCS_NQ 42            /* MAX_QUALITY_SCORE + 1, fastq.h:15 */
#define FAQCS_NBASE 5          /* A,T,C,G,N -- enum order FaQCs.h:35-42 */
#define FAQCS_NCOMP_BIN 10001  /* NUM_COMPOSITION_BIN, FaQCs.h:20 */
#define FAQCS_NCOMP_KIND 6     /* NucleotideCount fields A,T,C,G,N,GC, FaQCs.h:167-174 */
#define FAQCS_SEGMENT_READS 32768 /* buffer_size, FaQCs.cpp:232,585 */
#define FAQCS_MAX_READ_LENGTH 32767 /* longest read the HIP kernels take: the reference's aligner works in int16 (seq_overlap.h:80), and
                                       faqcs_read_result holds window coordinates in 16 bits.  Reads of up to 1 024 bases run on the
                                       chunked kernels (64 reads per wave pass); a batch with a longer read runs on trim_long /
                                       adapter_overlap<1, 32768> (one wave per read) */
#define FAQCS_ARENA_PAD_BEFORE 16 /* readable bytes required in front of / behind a batch's arenas (faqcs_batch) */
#define FAQCS_ARENA_PAD_AFTER 64
/* Adapter / contaminant library (faqcs_params.adapter_seq): up to 65 534 targets -- faqcs_read_result.adapter holds 1 + index in 16 bits
   and 0xffff marks a bad base -- of up to 32 767 bases each (the reference's aligner scores in int16, seq_overlap.h:80).  faqcs_create()
   refuses anything larger with FAQCS_E_INVAL; nothing is truncated.  Sets of at most 64 targets of at most 8 192 bases run in one pass of
   the pre-pass; larger ones in consecutive groups of targets. */
#define FAQCS_MAX_ADAPTERS 65534
#define FAQCS_MAX_ADAPTER_LENGTH 32767

enum { FAQCS_MODE_HARD = 0, FAQCS_MODE_BWA = 1, FAQCS_MODE_BWA_PLUS = 2 }; /* Options::Mode, FaQCs.h:90-95 */

/* error codes */
enum {
    FAQCS_OK = 0,
    FAQCS_E_INVAL = -1,      /* bad argument / unsupported size */
    FAQCS_E_NODEVICE = -2,   /* no HIP device or HIP runtime failure */
    FAQCS_E_QUALITY = -3,    /* a quality score > 41 after the offset (fastq.h:31-33 throws) */
    FAQCS_E_BASE = -4,       /* non-IUPAC base reached the aligner (seq_overlap.cpp:409 throws) */
    FAQCS_E_NOMEM = -5,
    FAQCS_E_KMER_FULL = -6   /* device k-mer table exhausted */
};

/* The subset of the reference's Options (FaQCs.h:77-144) the hot path reads, flattened to a POD.
 * The host resolves everything the reference resolves before/around trim(): quality-offset
 * auto-detect (trim.cpp:599-617), the NextSeq -q bump (trim.cpp:619-626, FaQCs.cpp:404-414) and the
 * adapter list (options.cpp:576-694). */
typedef struct faqcs_params {
    uint32_t abi_version;                 /* FAQCS_ABI_VERSION */
    int32_t  mode;                        /* FAQCS_MODE_* */
    int32_t  quality;                     /* -q ; Options::quality is a (signed) char */
    int32_t  input_quality_offset;        /* 33 / 64 (already auto-detected) */
    int32_t  output_quality_offset;
    uint32_t min_read_length;             /* --min_L */
    uint32_t max_num_poly_N;              /* -n */
    uint32_t trim_5;                      /* --5end */
    uint32_t trim_3;                      /* --3end */
    uint32_t replace_to_N_q;              /* --replace_to_N_q */
    float    average_quality;             /* --avg_q */
    float    low_complexity_cutoff_ratio; /* --lc  (float in the reference: FaQCs.h:115) */
    float    filterAdapterMismatchRate;   /* --rate */
    uint32_t protect_5;                   /* --5trim_off */
    uint32_t qc_only;                     /* --qc_only */
    uint32_t kmer_rarefaction;            /* --kmer_rarefaction */
    uint32_t kmer;                        /* -m, 2..31 */
    uint32_t split_size;                  /* --split_size */
    uint32_t num_subsample;               /* --subset (already doubled per options.cpp:506-523) */
    uint32_t max_read_length;             /* capacity R of the per-position matrices (<= FAQCS_MAX_READ_LENGTH); no read of a batch may be longer */
    uint32_t n_adapters;                  /* 0 == !(filter_adapter || filter_phiX) */
    const char *const *adapter_seq;       /* n_adapters NUL-terminated IUPAC strings (Options::adapter[j].second) */
    uint64_t kmer_table_slots;            /* device hash-table capacity (0 = library default 2^28; rounded up to a power of two in [2^22, 2^32]:
                                             the table is cut into 65 536 slices, one per key partition (a partition = the k-mers whose minimizer
                                             hashes to it); a key that finds the 128 slots behind its home slot taken lives in an overflow area of
                                             slots / 16 behind the table (round 5: a full slice is no longer an error), and FAQCS_E_KMER_FULL is
                                             raised when that area cannot take a key either -- size the table for <= 0.6 x slots distinct k-mers;
                                             16 bytes x 1.0625 x slots of device memory) */
} faqcs_params;

/* One submission: reads packed back to back in two byte arenas (structure of arrays).
 * Read i occupies seq[offset[i] .. offset[i+1]) and qual[offset[i] .. offset[i+1]) -- the reference
 * rejects |seq| != |qual| at parse time (fastq.cpp:117-121) so one offset array serves both.
 * PADDING CONTRACT: both arenas must be readable from 16 bytes before seq/qual + offset[0] up to 64 bytes past
 * seq/qual + offset[n] (FAQCS_ARENA_PAD_BEFORE / FAQCS_ARENA_PAD_AFTER): the kernels fetch a read with unaligned
 * multi-dword loads predicated on the read's length only (up to 19 bytes past its end) and whole 16-byte aligned
 * pieces of a 64-read span (up to 15 bytes either side); the padding bytes are never interpreted.  faqcs_submit()
 * and faqcs_submit_async() copy into padded device buffers themselves, so the contract binds faqcs_submit_device()
 * callers.  segment_start[] partitions the reads into reference
 * trim() calls (adapter groups of 8 restart at a segment start, trim.cpp:977-1071; k-mer rarefaction
 * points are taken at segment ends, trim.cpp:157-185). */
typedef struct faqcs_batch {
    const uint8_t  *seq;
    const uint8_t  *qual;
    const uint32_t *offset;         /* n_reads + 1 entries, non-decreasing */
    uint32_t        n_reads;
    uint32_t        n_segments;     /* >= 1 when n_reads > 0 */
    const uint32_t *segment_start;  /* n_segments + 1 entries; [0] = 0, [n_segments] = n_reads */
    uint32_t        max_read_len;   /* upper bound on the read lengths of this batch (selects the kernel
                                       variant); 0 = unknown: faqcs_submit() scans the offsets,
                                       faqcs_submit_device() falls back to the context capacity */
    const uint8_t  *terminal_n;     /* OPTIONAL (ABI 2): one byte per read, bit 0 = the read's first base is an upper-case 'N', bit 1 = its
                                       last base is (what mask_quality_terminal_N, trim.cpp:1191-1216, looks at first).  A host pointer for
                                       faqcs_submit() / faqcs_submit_async() (uploaded with the offsets), a device pointer for
                                       faqcs_submit_device() (e.g. from faqcs_terminal_n_flags()).  NULL = the kernels look themselves: two
                                       scattered byte loads per read into the base arena ahead of its streaming copy, +100 B/read of fabric
                                       requests.  A parser has both bytes in hand when it lays a read down. */
} faqcs_batch;

/* Per-read outcome (8 bytes).  For a valid read the reference's output record is
 *   seq  = in.seq [start, start+len)  with 'G' -> 'N' where Q < replace_to_N_q   (trim.cpp:390-403)
 *   qual = in.qual[start, start+len)  with the read's leading / trailing upper-case-'N' runs set to
 *          the input offset (trim.cpp:1191-1216) and then re-based input->output offset (trim.cpp:516-525)
 * faqcs_apply_edits() performs exactly these byte edits on the host. */
typedef struct faqcs_read_result {
    uint16_t start;   /* == offset_5 of trim_read() for a valid read */
    uint16_t len;
    uint16_t flags;   /* FAQCS_F_* */
    uint16_t adapter; /* 1 + index of the adapter credited for this read (trim.cpp:1036-1064), 0 = none */
} faqcs_read_result;

#define FAQCS_F_VALID        0x0001u
#define FAQCS_F_FILTER_MASK  0x000eu /* which filter fired first (trim_read short-circuit order) */
#define FAQCS_F_FILTER_SHIFT 1
enum { FAQCS_FILT_NONE = 0, FAQCS_FILT_LENGTH_PRE = 1, FAQCS_FILT_LENGTH_POST = 2, FAQCS_FILT_POLY_N = 3,
       FAQCS_FILT_AVG_Q = 4, FAQCS_FILT_LOW_COMPLEXITY = 5 };
#define FAQCS_F_QUAL_TRIMMED 0x0010u /* READ_QUAL_TRIM counted for this read */
#define FAQCS_F_ADAPTER      0x0020u /* start_length changed by the adapter pre-pass */
#define FAQCS_F_POLY_N_SEEN  0x0040u /* READ_NN counted (qc_only keeps the read valid, trim.cpp:368-370) */
/* The read is where the reference's trim() call throws; the submission as a whole also fails at faqcs_sync()/
 * faqcs_finish().  A driver that writes output per trim() call (the reference: per 32 768-read buffer) checks these to
 * stop before the buffer that holds such a read, as the reference does (FaQCs.cpp:287-361). */
#define FAQCS_F_ERR_QUALITY  0x0100u /* a quality above MAX_QUALITY_SCORE (fastq.h:31-33) */
#define FAQCS_F_ERR_BASE     0x0200u /* adapters active and a base na_to_bits() rejects (seq_overlap.cpp:409) */

/* Layout (in uint64 units) of the additive counter block.  Everything the reference accumulates in
 * filter_stats / PlotInfo / adapter_stats is a sum of per-read integers, so one block == one
 * all-reduce(sum).  Matrices are row-major [position][column] exactly like matrix<size_t>
 * (matrix.h:56-64); the reference's "rows grow on demand" is recovered on the host as
 * 1 + (last non-zero row) -- see faqcs_counter_rows(). */
typedef struct faqcs_layout {
    uint32_t max_read_length; /* R */
    uint32_t n_adapters;
    uint64_t filter_stats;    /* [FAQCS_NUM_STAT] */
    uint64_t pre_read_qhist, pre_base_qhist, post_read_qhist, post_base_qhist; /* [42] each */
    uint64_t pre_len_hist, post_len_hist;   /* [R+1] */
    uint64_t pre_qual, post_qual;           /* [R][42] */
    uint64_t pre_base, post_base;           /* [R][5]  */
    uint64_t pre_comp, post_comp;           /* [10001][6]  (A,T,C,G,N,GC) */
    uint64_t adapter_stats;                 /* [n_adapters][2] = (reads, bases) */
    uint64_t total;                         /* number of uint64 in the block */
} faqcs_layout;

typedef struct faqcs_rarefaction { uint64_t num_seq, distinct_kmer, total_kmer; } faqcs_rarefaction; /* FaQCs.h:194-199 */

typedef struct faqcs_ctx faqcs_ctx;

/* ---- layout / host helpers (no GPU needed) ---- */
int  faqcs_abi_version(void);
int  faqcs_counters_layout(uint32_t max_read_length, uint32_t n_adapters, faqcs_layout *out);
/* rows the reference's growing matrix<size_t> would have: 1 + last non-zero row (0 if all zero) */
uint32_t faqcs_counter_rows(const uint64_t *matrix, uint32_t max_rows, uint32_t n_cols);
/* applies the rule-based byte edits documented at faqcs_read_result; out_* need res->len bytes */
int  faqcs_apply_edits(const faqcs_params *p, const uint8_t *seq, const uint8_t *qual, uint32_t read_len,
                       const faqcs_read_result *res, uint8_t *out_seq, uint8_t *out_qual);
/* trim.cpp:599-617 -- returns 33, 64 or 0 (undecided: the reference throws) */
int  faqcs_auto_detect_quality_offset(const uint8_t *qual, const uint32_t *offset, uint32_t n_reads);
const char *faqcs_last_error(void);

/* ---- device path ---- */
/* device_id < 0 selects the current HIP device.  Copies the adapter strings. */
int  faqcs_create(const faqcs_params *params, int device_id, faqcs_ctx **out);
void faqcs_destroy(faqcs_ctx *ctx);

/* Process one batch whose arrays live in HOST memory: async H2D on the context's copy stream, kernels
 * on its compute stream, async D2H of the per-read results into `results` (n_reads entries).  Returns
 * when the work is enqueued; faqcs_sync() waits.  Counters accumulate on the device. */
int  faqcs_submit(faqcs_ctx *ctx, const faqcs_batch *batch, faqcs_read_result *results);

/* Same, but batch->seq/qual/offset and d_results are DEVICE pointers (inputs already resident in HBM:
 * the configuration bench.py times).  segment_start stays a host pointer. d_results may be NULL. */
int  faqcs_submit_device(faqcs_ctx *ctx, const faqcs_batch *batch, faqcs_read_result *d_results);

int  faqcs_sync(faqcs_ctx *ctx);

/* The output half of the device seam: the reads themselves.  Packs, on the device, the record the reference would write for every
 * selected read of a batch that went through faqcs_submit_device() -- the kept window with the byte edits documented at faqcs_read_result,
 * byte for byte what faqcs_apply_edits() writes on the host -- back to back into two arenas the caller owns.
 *   batch, d_results  what was given to faqcs_submit_device() (seq / qual / offset / terminal_n are DEVICE pointers; terminal_n, when present,
 *                     is used; segment_start is not needed and may be NULL).  The call is enqueued on the context's compute stream behind
 *                     that submission and returns at once; faqcs_sync() waits.
 *   d_keep            OPTIONAL device array, one byte per read.  Read i is emitted when d_results[i].flags & FAQCS_F_VALID and (d_keep ==
 *                     NULL or d_keep[i] != 0).  This is how a caller routes pairs the way FaQCs.cpp:296-361 does: valid1 & valid2 for the
 *                     two paired streams, valid1 ^ valid2 for the unpaired one.
 *   out               all DEVICE pointers.  Emitted reads keep input order: emitted read k occupies seq / qual [offset[k], offset[k + 1]) and
 *                     is input read index[k].  info->n_bytes and info->n_reads are ALWAYS the sizes the emission needs.  When n_bytes >
 *                     capacity_bytes (or >= 2^32: offsets are 32 bits wide, and the emission of a batch never exceeds its input bytes),
 *                     overflow = 1 and NOTHING is written to seq, qual, offset[1..] or index: no truncation, ever.  Otherwise overflow = 0.
 *                     The kernel stores whole 16-byte pieces, so bytes [n_bytes, n_bytes rounded up to 16) of seq / qual may be overwritten
 *                     with unspecified values; nothing else outside [0, n_bytes), offset[0 .. n_reads] and index[0 .. n_reads) is touched.
 *                     With FAQCS_ARENA_PAD_BEFORE readable bytes left in front of seq / qual by the caller, (seq, qual, offset, n_reads) is
 *                     thereby a valid input batch for faqcs_submit_device().
 * Parameters come from the context: input_quality_offset, output_quality_offset, replace_to_N_q.  n_reads == 0 is fine and yields zeros.
 * FAQCS_E_INVAL: a null ctx / batch / d_results / out / out->seq / qual / offset / info, out->seq or out->qual not 16-byte aligned.  Scan scratch
 * (16 bytes per read) is the library's: grown on demand, freed by faqcs_destroy(). */
typedef struct faqcs_emit_info { uint64_t n_bytes; uint32_t n_reads; uint32_t overflow; } faqcs_emit_info;
typedef struct faqcs_emit_out {
    uint8_t  *seq, *qual;             /* 16-byte aligned; capacity_bytes + FAQCS_ARENA_PAD_AFTER bytes writable */
    uint64_t  capacity_bytes;
    uint32_t *offset;                 /* batch->n_reads + 1 entries; [0] = 0, [k + 1] = end of emitted read k */
    uint32_t *index;                  /* OPTIONAL, batch->n_reads entries: input index of emitted read k (to gather ids / deflines) */
    faqcs_emit_info *info;            /* emitted reads, emitted bytes, overflow flag */
} faqcs_emit_out;
int  faqcs_emit_device(faqcs_ctx *ctx, const faqcs_batch *batch, const faqcs_read_result *d_results,
                       const uint8_t *d_keep, const faqcs_emit_out *out);

/* The input half of the device seam: FASTQ text -> the packed batch faqcs_submit_device() takes.
 * The rules are those of the reference's next_read (fastq.cpp:8-125), as the command line's parse_range states them:
 *   - a LINE ends at '\n'; its CONTENT is [line start, first '\r' or '\n', else end of text).  Bytes between a '\r' and the line's '\n'
 *     belong to nothing.
 *   - a record is four lines: defline, bases, plus line, qualities.  The defline is not checked for '@', the plus line's content is not
 *     looked at.  |bases content| != |quality content| is FAQCS_PARSE_E_LENGTH of that record.
 *   - final = 1: the text is the end of the input.  With Ltot = the number of '\n', plus 1 if the text does not end in '\n' and is not
 *     empty, Ltot / 4 records are complete (a last quality line without '\n' is accepted) and Ltot % 4 decides the tail error of record
 *     Ltot / 4: 1 E_SEQUENCE, 2 E_PLUS, 3 E_PLUS_DELIM when the third line has no '\n' and E_QUALITY when it has.  (A blank line at the
 *     end of a file is therefore E_SEQUENCE, as in the reference.)
 *   - final = 0: the text may stop anywhere.  Only records whose four lines all end in '\n' inside the text are parsed, the rest is left
 *     to the caller (info->consumed is where the next chunk starts) and there is no tail error.
 *   - errors are sequential: the first bad record in input order decides, info->n_reads is its index, and everything in front of it is
 *     parsed and delivered as if the text ended there.
 *   - there is no read-length limit here: info->max_read_len reports, faqcs_submit_device() keeps refusing what it refuses.
 * faqcs_parse_device: every pointer is a DEVICE pointer (d_text, and every pointer of *out, out->info included).  The call is enqueued on
 * the context's compute stream and returns at once; faqcs_sync() waits.
 *   d_text, n_text    the text.  It must be readable FAQCS_ARENA_PAD_BEFORE bytes in front of d_text and FAQCS_ARENA_PAD_AFTER bytes behind
 *                     d_text + n_text; those bytes are never interpreted.  No alignment is asked of it.  n_text >= 2^32 is FAQCS_E_INVAL at
 *                     call time: positions are 32 bits wide, and a caller cuts a larger file into chunks (final = 0, consumed).
 *   out               info is ALWAYS complete: the sizes the parsed records need, the text they cover, the error of record n_reads.  When
 *                     n_bytes > capacity_bytes, n_reads > capacity_reads or n_bytes >= 2^32, overflow = 1 and NOTHING but info is written:
 *                     no truncation, ever.  Otherwise the kernels touch only bytes [0, n_bytes rounded up to 16) of seq and qual (whole
 *                     16-byte pieces are stored), offset[0 .. n_reads], terminal_n[0 .. n_reads) and def_pos / def_len [0 .. n_reads).
 *                     With FAQCS_ARENA_PAD_BEFORE readable bytes left in front of seq / qual by the caller, (seq, qual, offset, terminal_n,
 *                     n_reads, max_read_len) is thereby a valid batch for faqcs_submit_device().
 * n_text == 0 yields zeros and offset[0] = 0.  FAQCS_E_INVAL: a null ctx / d_text (with n_text > 0) / out / out->seq / qual / offset /
 * terminal_n / info, out->seq or out->qual not 16-byte aligned, exactly one of def_pos and def_len given, n_text >= 2^32.
 * Scratch is the library's: grown on demand, freed by faqcs_destroy().  The number of lines of a text is known on the device only and the
 * host does not wait for it, so the scratch is sized by what n_text bytes can hold at most: 5 bytes per byte of text (a line start per
 * byte, a record length per four bytes).  A caller that minds cuts the text into smaller chunks.
 * faqcs_parse_host is the same with HOST pointers: the host statement of these rules, plain single-threaded C++ with no HIP call (no
 * padding is needed around the text, and exactly [0, n_bytes) of the arenas is written). */
enum { FAQCS_PARSE_OK = 0, FAQCS_PARSE_E_SEQUENCE, FAQCS_PARSE_E_PLUS, FAQCS_PARSE_E_PLUS_DELIM,
       FAQCS_PARSE_E_QUALITY, FAQCS_PARSE_E_LENGTH };
const char *faqcs_parse_error_text(int code);   /* the "fastq.cpp:next_read: ..." strings faqcs_mi prints; "" for FAQCS_PARSE_OK, NULL for no code */

typedef struct faqcs_parse_info {
    uint64_t n_bytes;      /* arena bytes the parsed records need (sum of their base-line contents) */
    uint64_t consumed;     /* text bytes covered by the parsed records: the next chunk starts here */
    uint32_t n_reads;      /* records parsed (== index of the bad record when error != 0) */
    uint32_t max_read_len;
    uint32_t overflow;     /* 1: n_bytes > capacity_bytes, n_reads > capacity_reads or n_bytes >= 2^32 */
    int32_t  error;        /* FAQCS_PARSE_* of record n_reads */
} faqcs_parse_info;

typedef struct faqcs_parse_out {
    uint8_t  *seq, *qual;          /* 16-byte aligned, capacity_bytes + FAQCS_ARENA_PAD_AFTER writable */
    uint64_t  capacity_bytes;
    uint32_t  capacity_reads;
    uint32_t *offset;              /* capacity_reads + 1 */
    uint8_t  *terminal_n;          /* capacity_reads; the flags of faqcs_batch.terminal_n */
    uint32_t *def_pos, *def_len;   /* OPTIONAL (both or neither): defline content of record k = text[def_pos[k] .. +def_len[k]) */
    faqcs_parse_info *info;
} faqcs_parse_out;

int  faqcs_parse_device(faqcs_ctx *ctx, const uint8_t *d_text, uint64_t n_text, int final, const faqcs_parse_out *out);
int  faqcs_parse_host(const uint8_t *text, uint64_t n_text, int final, const faqcs_parse_out *out);

/* The last step of the device seam: the records the reference writes to its files (FaQCs.cpp:296-361), as FASTQ text in device memory.
 * Bases and qualities are read straight from the batch's arenas, the deflines from the text faqcs_parse_device() indexed.
 * The rules:
 *   - which reads are rendered.  d_order (OPTIONAL) has n_reads entries: candidate j is read d_order[j]; an entry >= n_reads is skipped
 *     and never dereferenced; NULL means input order (candidate j is read j).  A candidate i is rendered when (d_select == NULL or
 *     d_select[i] != 0) and, when d_results != NULL, d_results[i].flags & FAQCS_F_VALID.  Rendered records keep candidate order.
 *   - d_results != NULL (the trimmed streams): the record is  defline '\n' S "\n+\n" Q '\n'  where S / Q are exactly what
 *     faqcs_apply_edits() writes for that read's window, with the context's input_quality_offset, output_quality_offset and replace_to_N_q
 *     (and batch->terminal_n when present): def_len + 2 len + 5 bytes, the bytes of Run::write_read.
 *   - d_results == NULL (the discard stream): the ORIGINAL record -- the whole read, no edit, no re-basing -- in the same form: the bytes
 *     of Run::write_raw.
 *   - the defline of read i is d_text[d_def_pos[i] .. + d_def_len[i]), exactly as faqcs_parse_device() delivered it.  It is not checked
 *     and may be empty.
 *   - out->info is ALWAYS complete: the bytes and the records the rendering needs.  n_bytes > capacity_bytes or n_bytes >= 2^32 (text
 *     positions are 32 bits wide) sets overflow = 1 and NOTHING but info is written: no truncation, ever.  Otherwise only
 *     text[0 .. n_bytes rounded up to 16) (whole 16-byte pieces are stored), rec_offset[0 .. n_reads] and rec_index[0 .. n_reads) are
 *     touched, with n_reads = info->n_reads.  A batch without reads, or of which nothing is rendered, yields zeros (and rec_offset[0] = 0).
 * faqcs_render_device: every pointer but ctx, batch and out is a DEVICE pointer, and so are batch->seq / qual / offset / terminal_n and every
 * pointer of *out (out->info included); batch->segment_start is not needed.  batch and d_results are what faqcs_submit_device() took and
 * filled; d_text needs the padding faqcs_parse_device() asks for (FAQCS_ARENA_PAD_BEFORE readable bytes in front of it, FAQCS_ARENA_PAD_AFTER
 * behind the last defline), the arenas that of faqcs_batch.  The call is enqueued on the context's compute stream behind the submission and
 * returns at once: the host never waits for a count; faqcs_sync() waits.  With both mates of a paired run in one batch -- read i of mate 2
 * at m + i -- the four files are four calls: QC.1 select [v1 & v2, 0], QC.2 select [0, v1 & v2], unpaired select
 * [v1 ^ v2, v1 ^ v2] in the order [0, m, 1, m + 1, ...], discard without results, select [!v1, !v2] in the same order.  (The two mates in
 * TWO batches, as two parses leave them: faqcs_pair_device / faqcs_render_pair_device below.)
 * Scratch (36 bytes per read) is the library's: grown on demand, freed by faqcs_destroy().
 * FAQCS_E_INVAL: a null ctx / batch / d_text (with reads) / batch arrays (with reads) / d_def_pos / d_def_len / out / out->text / out->info,
 * or out->text not 16-byte aligned.
 * faqcs_render_host is the same with HOST pointers: the host statement of these rules, plain single-threaded C++ with no HIP call (no
 * padding is needed anywhere, exactly [0, n_bytes) of the text is written, batch->terminal_n is not looked at; p may be NULL without
 * results; a window that leaves its read is FAQCS_E_INVAL). */
typedef struct faqcs_render_info { uint64_t n_bytes; uint32_t n_reads; uint32_t overflow; } faqcs_render_info;
typedef struct faqcs_render_out {
    uint8_t  *text;            /* 16-byte aligned; capacity_bytes + FAQCS_ARENA_PAD_AFTER writable */
    uint64_t  capacity_bytes;
    uint32_t *rec_offset;      /* OPTIONAL, batch->n_reads + 1: [0] = 0, [k + 1] = end of rendered record k */
    uint32_t *rec_index;       /* OPTIONAL, batch->n_reads: input read of rendered record k */
    faqcs_render_info *info;
} faqcs_render_out;
int  faqcs_render_device(faqcs_ctx *ctx, const faqcs_batch *batch, const faqcs_read_result *d_results,
                         const uint8_t *d_text, const uint32_t *d_def_pos, const uint32_t *d_def_len,
                         const uint8_t *d_select, const uint32_t *d_order, const faqcs_render_out *out);
int  faqcs_render_host(const faqcs_params *p, const faqcs_batch *batch, const faqcs_read_result *results,
                       const uint8_t *text, const uint32_t *def_pos, const uint32_t *def_len,
                       const uint8_t *select, const uint32_t *order, const faqcs_render_out *out);

/* The pair stage of the device seam: the two mates of a paired run (-1 r1 -2 r2) in TWO batches -- two texts, two sets of defline spans,
 * two result arrays, as two faqcs_parse_device + faqcs_submit_device calls leave them -- checked, routed and rendered without joining them.
 * A faqcs_mate is one mate's buffer: batch (seq / qual / offset / terminal_n as for faqcs_render_device; segment_start is not needed), the
 * results of its submission, the text its parse indexed (with that text's padding) and the defline spans.  The faqcs_mate structs and the
 * faqcs_batch they point to are HOST memory; for the device forms every other pointer in them is a DEVICE pointer.
 *
 * faqcs_pair_device / faqcs_pair_host: the id check of FaQCs.cpp:382-389, the routing of FaQCs.cpp:296-361 and the two FilterStat slots
 * that depend on both mates (FaQCs.cpp:304-308).
 *   - size.  n = min(m1->batch->n_reads, m2->batch->n_reads).  Unequal counts are no error: chunks of two files differ, and the caller
 *     carries the surplus.  n > 2^31 - 1 is FAQCS_E_INVAL.
 *   - the id (parse_id, trim.cpp:188-222) of a defline of len bytes is its first loc bytes: loc is the position of the first ' ', or len
 *     if there is none; loc is reduced by 2 when loc > 1, byte loc - 1 is '0'..'9' and byte loc - 2 is '.' or '/'.  A tab is no delimiter;
 *     an empty defline has the empty id.  Pair i MATCHES when both ids have the same length and the same bytes.
 *   - errors are sequential, as everywhere in the seam: the lowest i that does not match decides.  mismatch = 1, n_pairs = i and id_len[]
 *     holds the two id lengths -- the ids are text[def_pos[i] .. + id_len), for the caller to download for the reference's message.
 *     Without a mismatch n_pairs = n and id_len[] = 0.
 *   - the route.  route[i] for i < n_pairs is FAQCS_ROUTE_V1 * valid1 | FAQCS_ROUTE_V2 * valid2, valid = results[i].flags & FAQCS_F_VALID;
 *     route[i] for n_pairs <= i < n is FAQCS_ROUTE_NOWHERE.  The counters (paired_read_number, paired_base_length, n_one_valid,
 *     n_none_valid) cover i < n_pairs only.  Nothing outside route[0 .. n) and info is written.
 *   - check only.  With both results == NULL only the id check runs -- the reference's order: the check comes before trim(), so a caller can
 *     check before submitting.  route may then be NULL and is not touched; the counters and n_one_valid / n_none_valid are 0.  Exactly one
 *     results == NULL, or results without a route, is FAQCS_E_INVAL.
 *   - the bytes of info and route are a function of the inputs alone: the kernels use no atomics (per-tile partials, one finishing block).
 * faqcs_pair_device is enqueued on the context's compute stream and returns at once; d_route and d_info are DEVICE pointers.  The texts
 * need the padding faqcs_parse_device() asks for (whole 16-byte vectors are loaded at a defline's start and over its end).
 * FAQCS_E_INVAL: a null ctx / mate / batch / info, null text / def_pos / def_len with n > 0, and what is listed above.
 *
 * faqcs_render_pair_device / faqcs_render_pair_host: one of the four files of FaQCs.cpp:296-361 from the two mates and the route.  The
 * candidates are j = 0 .. 2 n_pairs - 1, pair i = j >> 1, mate s = j & 1, in that order; with r = route[i] candidate j is rendered when
 *     FAQCS_FILE_QC1       s == 0 && r == 3              the trimmed record (Run::write_read: as faqcs_render_device with results)
 *     FAQCS_FILE_QC2       s == 1 && r == 3              trimmed
 *     FAQCS_FILE_UNPAIRED  r == (1 << s)                 trimmed
 *     FAQCS_FILE_DISCARD   r < 4 && !(r >> s & 1)        the ORIGINAL record (as faqcs_render_device without results; results are not read)
 * so a pair routed FAQCS_ROUTE_NOWHERE appears in no file.  Bases, qualities, defline, result and terminal_n of a record come from mate s's
 * own arrays; rec_index[k] = 2 i + s; rec_offset / rec_index hold up to 2 n_pairs (+ 1) entries.  info, the overflow rule (nothing but
 * info is written), the touched ranges, the alignment demands and the FAQCS_E_INVAL list are those of faqcs_render_device, per mate; in
 * addition a file code outside 0 .. 3, n_pairs larger than either batch's n_reads or than 2^31 - 1, a null route with n_pairs > 0 and null
 * results for a trimmed file with n_pairs > 0 are FAQCS_E_INVAL.  n_pairs = 0 yields zeros and rec_offset[0] = 0.  The device form takes
 * its parameters from the context, is enqueued on the compute stream and returns at once; scratch (72 bytes per pair) is the library's.
 * The host forms are the host statements of these rules: plain single-threaded C++, no HIP call, no padding needed, exact write ranges. */
typedef struct faqcs_mate {
    const faqcs_batch *batch;            /* seq / qual / offset / terminal_n: as for faqcs_render_device; segment_start not needed */
    const faqcs_read_result *results;    /* n_reads entries; NULL only where stated */
    const uint8_t  *text;                /* the text the parse indexed, with its padding */
    const uint32_t *def_pos, *def_len;
} faqcs_mate;

typedef struct faqcs_pair_info {
    uint64_t paired_read_number;         /* FaQCs.cpp:306: += 2 per pair with both mates valid */
    uint64_t paired_base_length;         /* FaQCs.cpp:307: += len1 + len2 of those pairs (faqcs_read_result.len) */
    uint32_t n_pairs;                    /* pairs routed (== index of the bad pair when mismatch != 0) */
    uint32_t mismatch;                   /* 1: the ids of pair n_pairs differ */
    uint32_t id_len[2];                  /* mismatch: parse_id length of that pair's two deflines (the ids the reference prints), else 0 */
    uint32_t n_one_valid, n_none_valid;  /* pairs with exactly one / no valid mate, among the routed */
} faqcs_pair_info;

enum { FAQCS_ROUTE_V1 = 1, FAQCS_ROUTE_V2 = 2, FAQCS_ROUTE_NOWHERE = 0x80 };
enum { FAQCS_FILE_QC1 = 0, FAQCS_FILE_QC2, FAQCS_FILE_UNPAIRED, FAQCS_FILE_DISCARD };

int  faqcs_pair_device(faqcs_ctx *ctx, const faqcs_mate *m1, const faqcs_mate *m2, uint8_t *d_route, faqcs_pair_info *d_info);
int  faqcs_pair_host(const faqcs_mate *m1, const faqcs_mate *m2, uint8_t *route, faqcs_pair_info *info);
int  faqcs_render_pair_device(faqcs_ctx *ctx, int file, const faqcs_mate *m1, const faqcs_mate *m2,
                              const uint8_t *d_route, uint32_t n_pairs, const faqcs_render_out *out);
int  faqcs_render_pair_host(const faqcs_params *p, int file, const faqcs_mate *m1, const faqcs_mate *m2,
                            const uint8_t *route, uint32_t n_pairs, const faqcs_render_out *out);

/* The step in front of the device seam: compressed input.  BGZF (bgzip) members in device memory -> the FASTQ text faqcs_parse_device()
 * takes.  Ordinary gzip -- members of any size, no index -- is faqcs_gunzip_device's, below.
 * A MEMBER:
 *   - a gzip member whose header has ID1 ID2 CM = 1f 8b 08 and FLG.FEXTRA set, and whose extra field holds a 'B' 'C' subfield of length 2:
 *     BSIZE, the member's total size - 1.  The acceptance rule is that of the command line's reader (BgzfReader::member_size): subfields in
 *     front of BC are skipped, a member is at least 26 bytes.  FNAME, FCOMMENT and FHCRC are skipped as RFC 1952 defines them (FHCRC is not
 *     verified); a reserved FLG bit is refused.
 *   - behind the header one deflate stream (RFC 1951): stored, fixed and dynamic blocks.  Code sets are accepted as zlib accepts them (an
 *     over-subscribed set is invalid; an incomplete one too, except a set without any code and -- not for the code-length code -- a single
 *     code of one bit).  The stream ends in the byte in front of the trailer.
 *   - the trailer: CRC-32 of the text and ISIZE, its length.  ISIZE <= 65 536.
 *   - there is no dictionary: a back-reference that reaches in front of the member's own output is invalid.
 * faqcs_bgzf_index_host: where the members are.  Plain host C++, no HIP call: walks the BSIZE chain of comp[0 .. n_comp) from byte 0 and
 * writes member_offset[0 .. n_members] (capacity_members + 1 entries; member k is comp[member_offset[k] .. member_offset[k + 1])).
 *   final = 0   a member whose bytes are not all inside the chunk is left to the caller (info->consumed is where the next chunk starts), no error
 *   final = 1   an incomplete last member is FAQCS_INFLATE_E_TRUNCATED of member n_members
 *   Bytes behind the last member that do not start a gzip header (1f 8b) end the data without an error, as they do for zlib's gzread
 *   (DESIGN.md section 8): consumed = n_comp.  A gzip header that is not a BGZF member's is FAQCS_INFLATE_E_HEADER of member n_members, and
 *   consumed is where it starts.  n_members > capacity_members: overflow = 1, info is complete and nothing else is written.
 *   n_comp >= 2^32 or a null pointer is FAQCS_E_INVAL.  This is the right form for bytes the host has just read and is about to upload:
 *   the chain is a serial pointer chase -- each header says where the next one is -- that the host does in microseconds.
 * faqcs_bgzf_index_device: the same call for compressed bytes that are in device memory already (a peer's buffer, a tensor, an RDMA
 *   landing buffer) and would have to come back to the host only to be walked.  Every pointer but ctx is a DEVICE pointer, d_info
 *   included.  Enqueued on the context's compute stream, returns at once; faqcs_sync() waits.  No alignment is asked of d_comp and nothing
 *   outside d_comp[0 .. n_comp) is read.  The contract is faqcs_bgzf_index_host's, field for field:
 *   final         0: an incomplete last member is left to the caller and consumed says where the next chunk starts; 1: it is
 *                 FAQCS_INFLATE_E_TRUNCATED of member n_members
 *   end of data   bytes that do not start 1f 8b end the data without an error, consumed = n_comp; a gzip header that is not a BGZF
 *                 member's is FAQCS_INFLATE_E_HEADER with consumed at its start
 *   short input   the host walk looks at what there is: one byte 1f alone, 1f 8b with fewer than 4 bytes, a sound start with fewer than
 *                 18 bytes or fewer than 12 + XLEN are an incomplete member (see final); a byte that is wrong is judged as soon as it is there
 *   BC subfield   subfields in front of BC are skipped, a BC with SLEN != 2 is passed over, a BC whose six bytes overrun XLEN is not
 *                 taken; no BC, or a stated size below 26, is FAQCS_INFLATE_E_HEADER
 *   members       only what the chain from byte 0 lands on is a member: bytes inside a member that look like a header (in a stored block,
 *                 FNAME, FCOMMENT, an FEXTRA subfield) are not, whatever they state
 *   overflow      n_members > capacity_members: overflow = 1, info is complete and nothing else is written
 *   error         d_member_offset[0 .. n_members] of the members in front of the error are written, as the host writes them
 *   FAQCS_E_INVAL: n_comp >= 2^32, a null ctx, d_member_offset or d_info, a null d_comp with n_comp > 0.
 *   Scratch is the library's, grown on demand and freed by faqcs_destroy(): 6 bytes per compressed byte (18 bytes for each of the
 *   n_comp / 3 positions that can look like a member's header at the same time), so chunks of 256 MiB or less are the sensible unit.
 *   faqcs_bgzf_index_time_ms: the two stages of the context's last call (candidates: every position tested, the candidates in order;
 *   chain: the chain from byte 0 over them, info, the offsets).
 * faqcs_inflate_device: every pointer but ctx and out is a DEVICE pointer, out->info included.  Enqueued on the context's compute stream,
 * returns at once; faqcs_sync() waits.  No alignment is asked of d_comp; member k is d_comp[d_member_offset[k] .. d_member_offset[k + 1]).
 *   before decoding   every member's header and trailer are checked and the ISIZE of the members give each its position in the text and the
 *                     total (a member whose header is refused counts 0).  total > capacity_bytes or total >= 2^32: overflow = 1, n_bytes and
 *                     n_members are the totals, error = 0 and NOTHING but info is written: no truncation, ever.  A header that breaks the
 *                     rules above (or offsets that are not increasing inside n_comp) is E_HEADER of that member, ISIZE > 65 536 E_LENGTH.
 *   after decoding    a decoded length that differs from ISIZE is E_LENGTH; an invalid code or code set, block type 3, a stored block with
 *                     LEN != ~NLEN, a distance in front of the member, input that runs out or is left over is E_DATA; a CRC that differs
 *                     from the trailer is E_CRC.  Where a member has more than one of these wrong, the stream is read in order and the first
 *                     thing met decides: a token (a literal, a match, a stored block) that would carry the text beyond ISIZE is E_LENGTH
 *                     there and then -- what follows is not read -- and a stream that ends short of ISIZE is E_LENGTH only if it ends
 *                     well, in the byte in front of the trailer; input that runs out is E_DATA however much text there was.  Within one
 *                     token E_DATA goes first: a match that leaves ISIZE behind AND starts in front of the member, a stored block whose
 *                     LEN exceeds ISIZE AND the input, are E_DATA.  E_CRC is looked at last, when stream and length were sound.
 *   Errors are sequential, as in the parse: the first bad member in input order decides, info->n_members is its index, info->n_bytes the
 *   text of the members in front of it, and that text is delivered byte-exact (what lies behind it in `text` is unspecified).  Without an
 *   error n_members and n_bytes are the totals.  The kernels touch only text[0 .. scanned total rounded up to 16), member_text_offset
 *   [0 .. n_members] (all of them, error or not) and info; a member's decoder never writes outside its own [position, position + ISIZE),
 *   whatever the compressed bytes say.  n_members == 0 yields zeros.  With FAQCS_ARENA_PAD_BEFORE readable bytes left in front of text and
 *   FAQCS_ARENA_PAD_AFTER behind text + capacity_bytes by the caller, (text, n_bytes) is a valid d_text for faqcs_parse_device().
 *   FAQCS_E_INVAL: n_comp >= 2^32, more members than n_comp / 26, a null ctx / out / out->text / out->info, a null d_comp or d_member_offset
 *   with members, out->text not 16-byte aligned.  Scratch (24 bytes per member: header fields, position, status) is the library's: grown on
 *   demand, freed by faqcs_destroy().
 * faqcs_inflate_host is the same call with HOST pointers: the host statement of these rules, single-threaded, no HIP call and no zlib,
 * built from the same decoder text as the kernel (csrc/faqcs_inflate.h).  It writes exactly text[0 .. n_bytes). */
enum { FAQCS_INFLATE_OK = 0, FAQCS_INFLATE_E_HEADER, FAQCS_INFLATE_E_LENGTH, FAQCS_INFLATE_E_DATA, FAQCS_INFLATE_E_CRC, FAQCS_INFLATE_E_TRUNCATED,
       FAQCS_INFLATE_E_SERIAL = 16 /* faqcs_gunzip_device only, and no property of the data: the stream does not split (6 .. 15 are no codes) */ };
const char *faqcs_inflate_error_text(int code);   /* "" for FAQCS_INFLATE_OK, NULL for no code */

typedef struct faqcs_bgzf_index_info {
    uint64_t consumed;     /* compressed bytes covered by the indexed members: the next chunk starts here */
    uint32_t n_members;    /* whole members found (== index of the bad member when error != 0) */
    uint32_t overflow;     /* 1: n_members > capacity_members */
    int32_t  error;        /* FAQCS_INFLATE_E_HEADER / _E_TRUNCATED of member n_members */
    uint32_t reserved;
} faqcs_bgzf_index_info;
int  faqcs_bgzf_index_host(const uint8_t *comp, uint64_t n_comp, int final, uint32_t *member_offset, uint32_t capacity_members,
                           faqcs_bgzf_index_info *info);
int  faqcs_bgzf_index_device(faqcs_ctx *ctx, const uint8_t *d_comp, uint64_t n_comp, int final, uint32_t *d_member_offset,
                             uint32_t capacity_members, faqcs_bgzf_index_info *d_info);
int  faqcs_bgzf_index_time_ms(faqcs_ctx *ctx, double *candidates_ms, double *chain_ms);

typedef struct faqcs_inflate_info {
    uint64_t n_bytes;      /* text bytes of the members in front of the first bad one (all of them when error == 0) */
    uint32_t n_members;    /* members delivered (== index of the bad member when error != 0) */
    uint32_t overflow;     /* 1: the scanned total > capacity_bytes or >= 2^32 */
    int32_t  error;        /* FAQCS_INFLATE_* of member n_members */
    uint32_t reserved;     /* 0 */
} faqcs_inflate_info;
typedef struct faqcs_inflate_out {
    uint8_t  *text;                /* 16-byte aligned; capacity_bytes (+ FAQCS_ARENA_PAD_AFTER for faqcs_parse_device) */
    uint64_t  capacity_bytes;
    uint32_t *member_text_offset;  /* OPTIONAL, n_members + 1: [0] = 0, [k + 1] = end of member k's text */
    faqcs_inflate_info *info;
} faqcs_inflate_out;
int  faqcs_inflate_device(faqcs_ctx *ctx, const uint8_t *d_comp, uint64_t n_comp, const uint32_t *d_member_offset, uint32_t n_members,
                          const faqcs_inflate_out *out);
int  faqcs_inflate_host(const uint8_t *comp, uint64_t n_comp, const uint32_t *member_offset, uint32_t n_members, const faqcs_inflate_out *out);

/* Ordinary gzip in device memory -> the same text: the files users actually have (gzip, pigz, bgzip output alike), which carry no index.
 * The text is what zlib's gzread delivers.
 *   input         d_comp[0 .. n_comp) holds one or more COMPLETE RFC 1952 members, with any FLG fields: FEXTRA, FNAME and FCOMMENT are
 *                 skipped, FHCRC is skipped and not verified; a reserved FLG bit or CM != 8 is E_HEADER.  BGZF members are ordinary members
 *                 here.  A member's window starts empty: a distance that reaches in front of the member is E_DATA.  Code sets are accepted
 *                 as faqcs_inflate_device accepts them.  No alignment is asked of d_comp; nothing outside d_comp[0 .. n_comp) is read.
 *   end of data   bytes behind the last member that do not start 1f 8b end the data without an error (consumed = n_comp), as for gzread and
 *                 faqcs_bgzf_index_host.  A last member whose header, stream or trailer is incomplete is E_TRUNCATED with consumed at its
 *                 header: a member must be resident whole here (faqcs_gunzip_stream_device, below, takes chunks).
 *   errors        per member and sequential, as in faqcs_inflate_device: the first bad member in input order decides, n_members is its index,
 *                 consumed where its header starts, n_bytes the text of the members in front of it, and that text is delivered byte-exact
 *                 (what lies behind it in `text` is unspecified).  E_DATA: an invalid code or code set, block type 3, LEN != ~NLEN, a
 *                 distance in front of the member.  E_LENGTH (ISIZE is the length modulo 2^32) and then E_CRC are looked at last.
 *   capacity      the total text is known before anything is written.  total > capacity_bytes or total >= 2^32: overflow = 1; n_bytes,
 *                 n_members and consumed are those of the members whose streams were walked whole, error is what ended the walk (0, or the
 *                 E_HEADER / E_DATA / E_TRUNCATED / E_SERIAL of member n_members), and NOTHING but info is written.
 *   the scheme     the compressed bytes are cut every piece_bytes bytes (0: 65 536; at least 1 024; small values
 *                 exist so that tests cross many piece edges with little data).  A wave per piece probes its range for the first bit
 *                 position that can begin a dynamic-Huffman block and counts, without output, up to the first block end at or behind its
 *                 range end.  The host walks these records from each member's first block: a piece whose start is not where the chain arrives
 *                 is counted again from there, in a round of its own.  max_rounds (0: 32) bounds the rounds spent inside ONE member; a member
 *                 that needs more is FAQCS_INFLATE_E_SERIAL -- "this stream does not split (stored or fixed blocks only, blocks that no
 *                 probe finds); inflate it on the host" -- an error of that member like any other: defined, bounded, never a wrong text.
 *                 Then the pieces of the chain are decoded to 16-bit symbols -- a byte, or a marker for a byte of the 32 768 in front of
 *                 the piece --, the markers are resolved over the chain in order, and the symbols become text, with a CRC-32 per slice.
 *   info          n_pieces (pieces of the chain), n_fixups (starts the chain had to force inside a member) and n_rounds (count rounds) say
 *                 what the speculation did.  They are part of the contract: the host statement takes the same decisions and states the same.
 *   THE CALL BLOCKS.  Unlike the other seam calls this one is a short conversation between host and device -- a few bytes per piece come
 *   back for the walk, per round -- on the context's compute stream; when it returns, the text and info are complete.  d_comp, out->text and
 *   out->info are DEVICE pointers all the same.  out->text is 16-byte aligned; the kernels write text[0 .. total) and info, nothing else; with
 *   the arena pads the caller leaves, (text, n_bytes) is a valid d_text for faqcs_parse_device().
 *   FAQCS_E_INVAL: n_comp >= 2^32, 0 < piece_bytes < 1 024, a null ctx / out / out->text / out->info, a null d_comp with n_comp > 0, out->text
 *   not 16-byte aligned.  Scratch is the library's, grown on demand and freed by faqcs_destroy(): 2 bytes per text byte (the symbols), and
 *   32 bytes per piece + 24 bytes per 16 KiB of text (the records).
 * faqcs_gunzip_host is the same call with HOST pointers: the host statement of these rules, single-threaded, no HIP call and no zlib, built
 * from the same text as the kernels (csrc/faqcs_gunzip.h).  It writes exactly text[0 .. n_bytes). */
typedef struct faqcs_gunzip_info {
    uint64_t n_bytes;      /* text of the members in front of the first bad one (all of them when error == 0) */
    uint64_t consumed;     /* compressed bytes covered by those members (data that ends without an error: n_comp) */
    uint32_t n_members;    /* members delivered (== index of the bad member when error != 0) */
    uint32_t overflow;     /* 1: the total > capacity_bytes or >= 2^32 */
    int32_t  error;        /* FAQCS_INFLATE_* of member n_members */
    uint32_t n_pieces, n_fixups, n_rounds;   /* what the speculation did */
} faqcs_gunzip_info;
typedef struct faqcs_gunzip_out {
    uint8_t  *text;                /* 16-byte aligned; capacity_bytes (+ FAQCS_ARENA_PAD_AFTER for faqcs_parse_device) */
    uint64_t  capacity_bytes;
    faqcs_gunzip_info *info;
} faqcs_gunzip_out;
int  faqcs_gunzip_device(faqcs_ctx *ctx, const uint8_t *d_comp, uint64_t n_comp, uint32_t piece_bytes, uint32_t max_rounds, const faqcs_gunzip_out *out);
int  faqcs_gunzip_host(const uint8_t *comp, uint64_t n_comp, uint32_t piece_bytes, uint32_t max_rounds, const faqcs_gunzip_out *out);

/* The same inflate in chunks the caller chooses: a member need not be resident whole, and it may hold 4 GiB of text or more.  A chunk may end
 * anywhere -- inside a deflate block, a header or a trailer.  What goes from one call to the next is the caller's, per file: two files may
 * be fed alternately on one context.  Everything faqcs_gunzip_device states holds here unless said otherwise.
 *   input         comp[0 .. n_comp) is the file from where the previous call's `consumed` left it: the caller presents comp[consumed ..)
 *                 again with more bytes behind it.  final = 1: these are the file's last bytes.
 *   output        info->n_bytes is the text THIS call delivered, the open member's share included; consumed the bytes of this call's input
 *                 that are done with; n_members the members completed in this call; n_pieces, n_fixups and n_rounds are this call's.
 *   final = 0     the call delivers every whole deflate block that is resident and stops at the last block boundary:
 *                   in mid-stream          phase STREAM, consumed = boundary_bit >> 3, bit = boundary_bit & 7
 *                   a header cut short     phase BETWEEN, consumed at its first byte
 *                   a final block without its 8 trailer bytes
 *                                          phase TRAILER, consumed at the first trailer byte
 *                 consumed == 0 with an unchanged state: the chunk holds no whole block behind the carried position -- make it larger, as
 *                 for faqcs_parse_device.  Whether bytes behind a member are another member or the data's end is judged from the bytes at
 *                 that position alone, in the call that reaches them.
 *   final = 1     what is incomplete is E_TRUNCATED.  With a zeroed state this is faqcs_gunzip_device / _host exactly: the same text, the
 *                 same info field for field.
 *   the state     HOST memory in both forms, all zero (but `window`) before a file's first call.  After every call crc is the CRC-32 (as
 *                 zlib's crc32() states it) of the open member's text so far, window[32768 - window_bytes .. 32768) that text's last bytes,
 *                 member_bytes, members, total_bytes and total_comp the sums.  For any sequence of chunk ends the concatenated text is what
 *                 the single call, and gzread, deliver.
 *   errors        per member and sequential.  Nothing of the bad member is delivered BY THIS CALL: n_bytes and n_members are those of the
 *                 members in front of it within this call, consumed is at its header -- or 0 when it is the member that was open at entry,
 *                 and then the state is unchanged; else the state stands behind what n_bytes and consumed say.  E_LENGTH and E_CRC of a
 *                 member that began in an earlier call are reported when its trailer is read: earlier calls have handed its text on, as for
 *                 any gzread caller.  E_LENGTH compares member_bytes modulo 2^32 with ISIZE.  E_SERIAL counts max_rounds within one
 *                 member and one call.
 *   capacity      as above, with total >= 2^32 - 32 768 as the limit: overflow = 1, nothing but info is written, the state is untouched.
 *                 The remedies are a larger text buffer or a SHORTER n_comp: any prefix is a valid chunk.
 *   the scheme    the continued position is a forced start, like a member's first block; the grid of pieces lies over this call's bytes.
 *                 The symbols have a front of 32 768 that holds the carried window, so a marker of the first piece resolves into it
 *                 (DESIGN.md section 4.8a).  Scratch is 64 KiB more than the single call's.
 *   n_comp == 0   with final = 0: zeros, the state as it is; with final = 1 in phase STREAM or TRAILER: E_TRUNCATED.
 *   THE CALL BLOCKS, as the single call does; faqcs_gunzip_time_ms reports the last gunzip call of either kind.
 *   FAQCS_E_INVAL: everything the single call refuses; a null state or state->window; phase > 2; bit > 7, or bit != 0 outside STREAM;
 *   window_bytes != min(member_bytes, 32 768); reserved != 0. */
enum { FAQCS_GUNZIP_BETWEEN = 0,   /* the next byte is a member header, or the end of the data */
       FAQCS_GUNZIP_STREAM  = 1,   /* the next bit continues the open member's deflate stream at a block boundary */
       FAQCS_GUNZIP_TRAILER = 2 }; /* the open member's final block is done; its 8 trailer bytes come next */
typedef struct faqcs_gunzip_state {          /* HOST memory in both forms; all zero except `window` before a file's first call */
    uint64_t member_bytes;   /* text of the open member that the calls so far delivered */
    uint64_t total_bytes;    /* text delivered over all calls */
    uint64_t total_comp;     /* compressed bytes consumed over all calls */
    uint32_t phase;
    uint32_t bit;            /* STREAM: the stream goes on at bit `bit` (0..7, LSB first) of the next call's comp[0]; else 0 */
    uint32_t crc;            /* CRC-32, as zlib's crc32() states it, of those member_bytes bytes */
    uint32_t window_bytes;   /* min(member_bytes, 32768) */
    uint32_t members;        /* members completed so far */
    uint32_t reserved;       /* 0 */
    uint8_t *window;         /* 32 768 bytes, the caller's: DEVICE memory for _device, host memory for _host;
                                valid: window[32768 - window_bytes .. 32768), the open member's last text bytes */
} faqcs_gunzip_state;
int  faqcs_gunzip_stream_device(faqcs_ctx *ctx, const uint8_t *d_comp, uint64_t n_comp, int final, uint32_t piece_bytes, uint32_t max_rounds,
                                faqcs_gunzip_state *state, const faqcs_gunzip_out *out);
int  faqcs_gunzip_stream_host(const uint8_t *comp, uint64_t n_comp, int final, uint32_t piece_bytes, uint32_t max_rounds,
                              faqcs_gunzip_state *state, const faqcs_gunzip_out *out);

/* The step behind the device seam: compressed output.  Text in device memory (what faqcs_render_device() assembled, or any bytes) -> BGZF
 * members in device memory, so that a third of the bytes leave the card and the result is what faqcs_inflate_device() takes.
 *   - cutting the text.  The text is cut every member_bytes bytes: member k is text[k * member_bytes .. min(n_text, (k + 1) * member_bytes)).
 *     member_bytes = 0 means 65 280, as bgzip cuts; valid values are 1 .. 65 280 (the small ones exist so that tests reach every member
 *     boundary case with little data).
 *   - a member is exactly what faqcs_inflate_device documents as a MEMBER, and what bgzip, gzip -d and zlib's gzread accept: the 18-byte
 *     header  1f 8b 08 04 | 00000000 | 00 ff | 06 00 | 'B' 'C' 02 00 | BSIZE,  ONE deflate block -- dynamic, fixed or stored, whichever
 *     is smallest -- and the trailer, CRC-32 and ISIZE.  A member is never larger than its text + 31 bytes: when the coded form is not
 *     smaller than a stored block the stored block is written and info->n_stored counts the member; so BSIZE always fits 16 bits.
 *   - matches have distances 1 .. 32 768 that never reach in front of the member (a 65 280-byte member has earlier positions farther back
 *     than the format allows: they are refused) and lengths 3 .. 258.
 *   - final = 1: the 28-byte EOF member of bgzip is appended, and counted in n_members and member_offset.  final = 0: nothing is appended,
 *     so the outputs of the chunks of a file concatenate to the file.  n_text = 0 yields zeros, or the EOF member alone with final = 1.
 *   - out->info is ALWAYS complete.  n_bytes > capacity_bytes or n_bytes >= 2^32 sets overflow = 1 and NOTHING but info is written: no
 *     truncation, ever.  Otherwise only comp[0 .. n_bytes rounded up to 16), member_offset[0 .. n_members] and info are touched.
 *   - the bytes are a function of (text, member_bytes, final) alone: not of the grid, of timing or of the alignment of d_text (none is
 *     asked of it, and nothing outside d_text[0 .. n_text) is read), and faqcs_deflate_host produces the same bytes.  The match finder is
 *     defined without an order of execution (csrc/faqcs_deflate.h): the candidates of a position are the latest
 *     earlier position with its hash in a 1 024-byte tile in front of its own tile, and the position in front of it; the parse is the
 *     greedy one.
 * faqcs_deflate_device: d_text and every pointer of *out (out->info included) are DEVICE pointers.  Enqueued on the context's compute stream,
 * returns at once; faqcs_sync() waits.  (out->comp, out->member_offset, info->n_members) is what faqcs_inflate_device() takes as (d_comp,
 * d_member_offset, n_members): no host index is needed.
 * FAQCS_E_INVAL: n_text >= 2^32, member_bytes > 65 280, a null ctx / out / out->comp / out->info, a null d_text with n_text > 0, out->comp
 * not 16-byte aligned, 2^32 members or more (2^32 - 1 bytes cut every byte, and the EOF member: n_members is 32 bits wide).  Scratch is the library's, grown on demand and freed by faqcs_destroy(): per member a slot of member_bytes + 31
 * rounded up to 16 (65 312 bytes at the default cut) and 8 bytes of sizes, per compute unit 4 bytes per position of a member (255 KB).
 * faqcs_deflate_host is the same call with HOST pointers: the host statement of these rules, single-threaded, no HIP call and no zlib,
 * built from the same encoder text as the kernel.  It writes exactly comp[0 .. n_bytes). */
typedef struct faqcs_deflate_info {
    uint64_t n_bytes;      /* compressed bytes of all members */
    uint32_t n_members;    /* members, the EOF member included */
    uint32_t overflow;     /* 1: n_bytes > capacity_bytes or >= 2^32 */
    uint32_t n_stored;     /* members whose block is a stored one */
    uint32_t reserved;     /* 0 */
} faqcs_deflate_info;
typedef struct faqcs_deflate_out {
    uint8_t  *comp;            /* 16-byte aligned; capacity_bytes (+ FAQCS_ARENA_PAD_AFTER) writable */
    uint64_t  capacity_bytes;
    uint32_t *member_offset;   /* OPTIONAL, n_members + 1: [0] = 0, [k + 1] = end of member k  -- the array faqcs_inflate_device takes */
    faqcs_deflate_info *info;
} faqcs_deflate_out;
int  faqcs_deflate_device(faqcs_ctx *ctx, const uint8_t *d_text, uint64_t n_text, uint32_t member_bytes, int final, const faqcs_deflate_out *out);
int  faqcs_deflate_host(const uint8_t *text, uint64_t n_text, uint32_t member_bytes, int final, const faqcs_deflate_out *out);

/* The same two calls with a choice of match finder.  FAQCS_DEFLATE_FAST is faqcs_deflate_device / faqcs_deflate_host, byte for byte.
 * FAQCS_DEFLATE_DENSE spends more time on smaller members (zlib level 3 to 4 on FASTQ text).  Every rule above holds
 * for it: the cutting, one block per member -- the smallest of dynamic, fixed and stored --, text + 31, final and the EOF member, overflow,
 * the touched ranges, no alignment of d_text, device bytes == host bytes; the bytes are a function of (text, member_bytes, final, mode).
 * The dense match finder, again without an order of execution:
 *   - a 1 024-position tile of the member is looked up and entered in SUB-TILES of 256 positions, in order: the two tables a position sees
 *     hold exactly the positions in front of its own sub-tile.
 *   - the candidates of position p are (a) the latest of those positions whose three bytes have p's 12-bit hash, (b) the latest of them
 *     whose EIGHT bytes have p's 12-bit hash (a 64-bit multiplicative hash; only positions with p + 8 <= the member's length enter this
 *     table or look it up), (c) p - 1.  A candidate farther back than 32 768 is refused by itself; of the others the longest match wins,
 *     the nearest on a tie; the test whether a match under 32 bytes pays is the fast mode's.
 *   - the lazy step, inside a tile only: where position i < 1 023 of a tile keeps a match of length len(i) > 0 and len(i + 1) > len(i),
 *     position i becomes a literal.  The rule is evaluated on the lengths as the find left them for the whole tile, so a rising chain
 *     i, i + 1, i + 2 makes both i and i + 1 literals, and position 1 023 of a tile is never given up for position 0 of the next.
 *   - the parse over the lengths that remain is the greedy one, as in the fast mode.
 * FAQCS_E_INVAL in addition: a mode that is neither of the two (nothing is written). */
enum { FAQCS_DEFLATE_FAST = 0, FAQCS_DEFLATE_DENSE = 1 };
int  faqcs_deflate_device_mode(faqcs_ctx *ctx, const uint8_t *d_text, uint64_t n_text, uint32_t member_bytes, int final, int mode, const faqcs_deflate_out *out);
int  faqcs_deflate_host_mode(const uint8_t *text, uint64_t n_text, uint32_t member_bytes, int final, int mode, const faqcs_deflate_out *out);

/* The decisions the reference's driver takes AROUND trim(), for a caller whose reads are in device memory: each is the FIRST element of a
 * contiguous range for which a predicate holds, in input order as everywhere in the seam, and each brings back a few bytes of info.
 *
 * faqcs_detect_device / faqcs_detect_host: the quality-offset auto-detect (auto_detect_quality_offset, trim.cpp:599-617, called at
 * FaQCs.cpp:261-270, 393-402, 609-611, 669-671; the reference's default: options.cpp:122) and the look of the NextSeq check at the first
 * defline (auto_detect_next_seq, trim.cpp:619-626, called at FaQCs.cpp:272-277, 404-414).
 *   - the range.  The reference decides on ONE buffer: the first full one of FAQCS_SEGMENT_READS reads, or the last partial one at the end
 *     of the input.  A device chunk holds more or fewer reads than that, so the call takes the reads [first, first + count) of the batch;
 *     the caller keeps the budget and calls again on the next chunk while undecided and under FAQCS_SEGMENT_READS reads.
 *     first + count > batch->n_reads is FAQCS_E_INVAL.  count == 0 yields {0, first, 0, 0, 0, 0}.
 *   - the offset.  Reads are packed back to back, so "the first decisive byte in read order" is the lowest b in
 *     [offset[first], offset[first + count]) whose qual[b], read as a SIGNED char, is > 74 or < 59.  > 74 gives 64, < 59 gives 33; the
 *     bytes 0x80 ... 0xff are therefore 33.  read is the unique i with offset[i] <= b < offset[i + 1] (a read of length 0 never owns a
 *     byte), pos = b - offset[read], byte = qual[b].  Without such a byte quality_offset = 0 -- the reference throws "Unknown quality
 *     format!" --, read = first + count and pos = byte = 0.
 *   - only batch->qual, batch->offset and batch->n_reads are read; seq, segment_start and terminal_n may be NULL.  The padding contract of
 *     faqcs_batch holds for the device form: whole aligned 16-byte vectors are loaded over both ends of the range.  Bytes outside the
 *     range are never interpreted.
 *   - NextSeq.  text, def_pos and def_len (what faqcs_parse_device delivered) are all given or all NULL; anything else is FAQCS_E_INVAL.
 *     With them next_seq = count > 0 && def_len[first] >= 3 && text[def_pos[first] .. + 3) == "@NS" -- the defline content includes the
 *     '@', as Read::def does --, without them 0.  The comparison with -q, the bump (faqcs_set_quality) and the message stay with the caller.
 *   FAQCS_E_INVAL in addition: a null ctx / batch / info, a null batch->qual or batch->offset with count > 0.
 *
 * faqcs_first_error_device / faqcs_first_error_host: where trim() threw (FAQCS_F_ERR_QUALITY: fastq.h:31-33, FAQCS_F_ERR_BASE:
 * seq_overlap.cpp:409; the reference stops before the buffer that holds such a read, FaQCs.cpp:287-361).  n_good is the lowest i < n with
 * results[i].flags & (FAQCS_F_ERR_QUALITY | FAQCS_F_ERR_BASE) and flags holds that read's two error bits; without such a read the result
 * is {n, 0}, and n == 0 yields {0, 0}.  Mapping n_good to the caller's FAQCS_SEGMENT_READS-read buffers is host arithmetic on its own
 * segment_start.  FAQCS_E_INVAL: a null ctx / info, null results with n > 0.
 *
 * The device forms: every pointer but ctx and batch is a DEVICE pointer (batch->qual / offset too, as for faqcs_submit_device; d_info
 * included).  They are enqueued on the context's compute stream and return at once -- so they run behind the parse or the submission that
 * produced their input --; faqcs_sync() waits.  info is ALWAYS complete and nothing but info is written.  Its bytes are a function of the
 * inputs alone: no atomics, a partial per 16 KB tile and one finishing block, as in the pair stage.  They take no parameter from the
 * context.  Scratch (4 bytes per tile; the byte form's for the 2^32 bytes that 32-bit offsets can span, 1 MB) is the library's: grown on
 * demand, freed by faqcs_destroy().  The host forms are the host statements of these rules: plain single-threaded C++, no HIP call, no
 * padding needed. */
typedef struct faqcs_detect_info {
    int32_t  quality_offset;  /* 33, 64, or 0: no decisive byte in the range (the reference throws "Unknown quality format!") */
    uint32_t read;            /* batch index of the read that holds the decisive byte; first + count when there is none */
    uint32_t pos;             /* its position inside that read; 0 when none */
    uint32_t byte;            /* the raw byte; 0 when none */
    uint32_t next_seq;        /* 1: count > 0, deflines were given and the defline content of read `first` starts with "@NS" */
    uint32_t reserved;        /* 0 */
} faqcs_detect_info;

int  faqcs_detect_device(faqcs_ctx *ctx, const faqcs_batch *batch, uint32_t first, uint32_t count,
                         const uint8_t *d_text, const uint32_t *d_def_pos, const uint32_t *d_def_len,
                         faqcs_detect_info *d_info);
int  faqcs_detect_host(const faqcs_batch *batch, uint32_t first, uint32_t count,
                       const uint8_t *text, const uint32_t *def_pos, const uint32_t *def_len, faqcs_detect_info *info);

typedef struct faqcs_error_info { uint32_t n_good; uint32_t flags; } faqcs_error_info;
int  faqcs_first_error_device(faqcs_ctx *ctx, const faqcs_read_result *d_results, uint32_t n, faqcs_error_info *d_info);
int  faqcs_first_error_host(const faqcs_read_result *results, uint32_t n, faqcs_error_info *info);

/* Pipelined form of faqcs_submit(): returns a ticket; faqcs_wait(ticket) blocks until THAT batch's results have
 * landed in `results` (later batches may still be in flight: two input staging slots let the H2D copy of batch
 * k+1 overlap the kernels of batch k).  Host arenas / result arrays obtained from faqcs_host_alloc() are pinned,
 * which makes both copies true asynchronous DMA. */
int  faqcs_submit_async(faqcs_ctx *ctx, const faqcs_batch *batch, faqcs_read_result *results, uint64_t *ticket);
int  faqcs_wait(faqcs_ctx *ctx, uint64_t ticket);
void *faqcs_host_alloc(size_t bytes);
void faqcs_host_free(void *p);

/* Which arm of the host orchestration the calls on a context have taken since faqcs_create(): plain host-side counts, incremented where
 * the branch is taken; no kernel knows of them and nothing resets them.  Read-only, never waits, touches no stream.  They exist so that
 * a test can state which path it ran (tests/submit_edges.py predicts every one of them from the schedule of calls alone). */
typedef struct faqcs_path_tallies {
    uint64_t folds_tail;         /* composition records of launch k-1 handed to launch k's blocks (comp_fold_tail) */
    uint64_t folds_aux;          /* ... to composition_histogram on the aux stream, beside launch k */
    uint64_t folds_now;          /* ... folded on the compute stream: faqcs_sync / _finish, faqcs_counters_export / _import, the collectives */
    uint64_t folds_dropped;      /* ... dropped with the block by faqcs_reset_counters */
    uint64_t slot_stream_waits;  /* faqcs_submit_async: a staging slot reused as it is, the copy stream waits for submission k-2 */
    uint64_t slot_event_syncs;   /* ... regrown: the host waits for submission k-2 */
    uint64_t recset_fold_waits;  /* a record set reused while its aux fold may still run: the compute stream waits for `folded` */
    uint64_t recset_grow_syncs;  /* a record set regrown: the host waits for the aux and the compute stream */
    uint64_t ticket_ring_waits;  /* faqcs_submit_async: the host waits for the submission that held this ticket's event eight calls ago */
} faqcs_path_tallies;
int  faqcs_path_tallies_get(const faqcs_ctx *ctx, faqcs_path_tallies *out);

/* Options::quality is mutable during a run: the NextSeq check bumps -q to 20 (FaQCs.cpp:272-277,404-414).
 * Takes effect for batches submitted afterwards. */
int  faqcs_set_quality(faqcs_ctx *ctx, int quality);

/* faqcs_params.input_quality_offset is what the reference detects on its first buffer (trim.cpp:599-617, the default: options.cpp:122),
 * after Options exist.  Accepts what faqcs_create() accepts for that field (it checks nothing there) and rebuilds everything
 * faqcs_create() derives from it: the parameter block of the kernels and the average-quality threshold table (--avg_q).  The call WAITS
 * for the context's streams -- the table is device memory that enqueued kernels read --, so work enqueued before it sees the old offset
 * and work enqueued after it the new one; it happens once per run.  A context may thus be created with a placeholder offset, used for
 * faqcs_parse_device, the id check of faqcs_pair_device and faqcs_detect_device -- none of them reads the offset -- and set before its
 * first submission.  (Submissions, faqcs_emit_device and the renderings of trimmed records read it.) */
int  faqcs_set_input_quality_offset(faqcs_ctx *ctx, int input_quality_offset);

/* Device address + length (uint64 units) of the additive counter block, so the host can run the one
 * collective this path needs -- all-reduce(sum, uint64) over RCCL -- in place before faqcs_finish(). */
int  faqcs_counters_device(faqcs_ctx *ctx, void **d_ptr, uint64_t *n_u64);

/* The same collective on a buffer the CALLER owns (what bench.py / faqcs_amd/parallel.py do: RCCL registers its own
 * allocations for peer access, so the all-reduce runs on a torch tensor): export copies the block (device to device,
 * d_dst/d_src are device pointers of >= n_u64 words) after the work submitted so far, import stores the reduced block. */
int  faqcs_counters_export(faqcs_ctx *ctx, void *d_dst, uint64_t n_u64);
int  faqcs_counters_import(faqcs_ctx *ctx, const void *d_src, uint64_t n_u64);

/* Copies the counter block to the host (layout: faqcs_counters_layout); syncs first.
 * Raises FAQCS_E_QUALITY / FAQCS_E_BASE if any read tripped the reference's throw sites. */
int  faqcs_finish(faqcs_ctx *ctx, uint64_t *counters, uint64_t n_u64);
int  faqcs_reset_counters(faqcs_ctx *ctx);

/* The merge of the reference (trim.cpp:120-154: every OpenMP thread adds its private counters to the caller's under `omp critical`) across
 * GPUs: all-reduce(sum) of the additive counter block IN PLACE, by RCCL over xGMI, enqueued on the context's compute stream behind its
 * kernels -- no staging copy, no host round trip.  librccl.so is loaded at the first call (the library does not
 * link it); every call fails with FAQCS_E_NODEVICE and a message when it is missing or reports an error, and the caller can fall back on
 * faqcs_counters_export / _import + its own collective.
 *   one process per GPU:  rank 0 calls faqcs_comm_id() and hands the FAQCS_COMM_ID_BYTES bytes to the other ranks (any channel); every rank
 *                         calls faqcs_comm_init(ctx, id, rank, world) (collective), then faqcs_comm_allreduce_counters(ctx) per pass.
 *   one process, n GPUs:  faqcs_comm_init_all(ctxs, n) once (the contexts must sit on n different devices), then
 *                         faqcs_comm_allreduce_counters_all(ctxs, n) -- one grouped call for all of them.
 * The communicator is released by faqcs_destroy(). */
#define FAQCS_COMM_ID_BYTES 128
int  faqcs_comm_id(void *id);
int  faqcs_comm_init(faqcs_ctx *ctx, const void *id, uint32_t rank, uint32_t world);
int  faqcs_comm_allreduce_counters(faqcs_ctx *ctx);
int  faqcs_comm_init_all(faqcs_ctx *const *ctxs, uint32_t n);
int  faqcs_comm_allreduce_counters_all(faqcs_ctx *const *ctxs, uint32_t n);

/* k-mer rarefaction (trim.cpp:157-185, FaQCs.cpp:518-537).  The k-mers of a submission are extracted when it is submitted, as 16-byte runs
 * into group buffers sized from the free HBM, and are COUNTED LATER (combine-before-insert): when the pass ends
 * (faqcs_kmer_end_table / faqcs_kmer_finish_pass) -- if the whole pass fits the buffers it is then counted in one piece and its keys never
 * reach the device table --, when the buffers are full, or when one of faqcs_kmer_points / _totals / _epoch_counts asks for the curve so far
 * (the open group then goes into the table, the slower path: a caller that only wants the finished curve calls faqcs_kmer_end_table FIRST and
 * reads the points afterwards -- they keep their values).  Points are appended at segment ends during submit; their (distinct, total)
 * are filled in by these calls:  */
int  faqcs_kmer_points(faqcs_ctx *ctx, faqcs_rarefaction *out, uint32_t cap, uint32_t *n_points);
/* (count, number of keys with that count) pairs, ascending count -- PlotInfo::kmer_frequency_histogram */
int  faqcs_kmer_histogram(faqcs_ctx *ctx, uint64_t *count, uint64_t *nkeys, uint64_t cap, uint64_t *n_pairs);
/* distinct keys / sum of counts of the pass in progress (the FaQCs.cpp:523-537 fallback point); when nothing has been counted since
 * faqcs_kmer_end_table(): of the pass that call finished */
int  faqcs_kmer_totals(faqcs_ctx *ctx, uint64_t *distinct, uint64_t *total);
/* Options::kmer_rarefaction is switched off by trim() once the curve is complete (trim.cpp:180-184) */
int  faqcs_kmer_active(faqcs_ctx *ctx);
/* End of a process_paired()/process_unpaired() pass (FaQCs.cpp:518-537, :737-756): folds the table into the
 * count histogram, appends the guaranteed single rarefaction point if none was taken, and starts a fresh
 * table (each process_* owns its own MAP<Word,size_t>, FaQCs.cpp:235,588). */
int  faqcs_kmer_end_table(faqcs_ctx *ctx);
/* The counting half of faqcs_kmer_end_table() (which calls it): the pass is complete, its open group is counted and every point and epoch
 * histogram is final; submissions with k-mers are refused until faqcs_kmer_end_table() has started the next pass.  For callers that read
 * faqcs_kmer_epoch_counts() (owner ranks) or the points before they end the table.  Replaces nothing of its own in the reference: the
 * end of process_paired() / process_unpaired(), FaQCs.cpp:518-537. */
int  faqcs_kmer_finish_pass(faqcs_ctx *ctx);

/* What a kmer_rarefaction context made from `params` will allocate on a device with free_bytes of free memory, before anything is
 * allocated (host only; bench.py --config kmer prints it per rank and refuses a run that cannot fit): out[0] the table with its overflow
 * area, out[1] / out[2] the level-1 / level-2 group buffers, out[3] the k-mer occurrences one group takes -- a pass below it is counted in
 * one piece, without the table --, out[4] the small arrays.  n_out >= 5. */
int  faqcs_kmer_memory_plan(const faqcs_params *params, uint64_t free_bytes, uint64_t *out, uint32_t n_out);

/* ---- k-mers across GPUs --------------------------------------------------------------
 * The reference keeps ONE MAP<Word,size_t> per process (trim.cpp:82,133-135) and samples (distinct, total) after
 * trim() calls (trim.cpp:157-185); distinct counts are not additive over shards.  In this mode every canonical
 * k-mer has one owner rank -- the owner of the partition its MINIMIZER hashes to (csrc/faqcs_skm.h), so that consecutive k-mers of a
 * read that share their minimizer travel together: a rank turns its shard into 16-byte ITEMS (a run of up to 17 consecutive 31-mers as
 * 2-bit bases + the epoch, about 8 occurrences per item: under 2 bytes per occurrence on the wire where a (key, epoch) pair per
 * occurrence was 16), grouped by owner; the caller moves them with an all-to-all (RCCL: faqcs_amd/parallel.py), and the owner expands,
 * combines and inserts them keeping the smallest epoch per key.  The items are opaque to the caller.
 * epoch = index of the first rarefaction point that includes the segment (a host function of the GLOBAL
 * read counts only, trim.cpp:157-185); FAQCS_EPOCH_NONE = the curve was already complete.  Then
 *   distinct(point i) = sum over ranks of #{keys with first epoch <= i},  total(point i) = sum of occurrences with
 *   epoch <= i -- both additive, i.e. one all-reduce of 2 x n_epochs integers. */
#define FAQCS_EPOCH_NONE 0xffffffffu
/* First call on a fresh kmer_rarefaction context.  n_epochs = number of epoch slots (num_subsample + 1).  Up to 1 000 (an item has 10 bits
 * for its epoch) the exchange moves runs of k-mers and the owner combines them; a job with more sampling points goes through (key, epoch)
 * pairs instead -- 16 bytes per occurrence, one atomic per pair on the owner: exact, any --subset, slow. */
int  faqcs_kmer_partition(faqcs_ctx *ctx, uint32_t rank, uint32_t world, uint32_t n_epochs);
/* Epoch of every segment of the NEXT submission (which then buckets instead of inserting).  That submission is refused with FAQCS_E_INVAL
 * when the epochs do not number its segments, or -- runs of k-mers, not pairs -- when it holds more than 1 000 runs of consecutive segments
 * with one epoch (a run is one extraction launch; an item has 10 bits for it).  A refused submission is refused before any kernel of it is
 * launched: nothing of it is trimmed or counted, no k-mer launch is made (only its bytes have been copied to a staging buffer, which the
 * next submission overwrites), its reads are not in the counter block and the outbox is the one before.  The epochs given for it stay set
 * until the next faqcs_kmer_set_epochs() or accepted submission. */
int  faqcs_kmer_set_epochs(faqcs_ctx *ctx, const uint32_t *segment_epoch, uint32_t n_segments);
/* After a submission: device array of 16-byte items grouped by destination rank 0..world-1 and the number of ITEMS per destination
 * (counts[world]).  Valid until the next submission.  A second call without a submission in between reports nothing to send (all
 * counts 0): a rank of a collective loop whose part of the input was empty does not send the previous outbox again.  A submission
 * without reads EMPTIES the outbox: behind it faqcs_kmer_outbox_host lists no key and faqcs_kmer_forward moves nothing. */
int  faqcs_kmer_outbox(faqcs_ctx *ctx, void **d_items, uint64_t *counts);
/* The canonical keys of EVERY OCCURRENCE of the last submission's outbox, expanded from its items on the host (all destinations; keys ==
 * NULL or cap too small: only the count is returned).  For a caller that owns the table itself, like the reference's trim() seam (MAP<Word,size_t>,
 * trim.cpp:133-135): the key values are an injective re-encoding of the canonical k-mers, so counts and distinct counts
 * are the reference's, the key values are not. */
int  faqcs_kmer_outbox_host(faqcs_ctx *ctx, uint64_t *keys, uint64_t cap, uint64_t *n_keys);
/* Owner side: takes n_items received items (device pointer; returns when the buffer may be reused).  The items must be the ones a sender
 * partitioned over the same `world` grouped for THIS rank: bucket b (the top 8 bits of an item's partition) goes to rank (b * world) >> 8,
 * and rank r owns the buckets ceil(r * 256 / world) .. ceil((r + 1) * 256 / world) - 1 -- the same set for every world up to 64.  An item of
 * another rank's bucket is NOT detected: its partition is mapped onto this rank's table as if it were its own (modulo 2^32) and the
 * results of this rank are undefined from there on. */
int  faqcs_kmer_insert_device(faqcs_ctx *ctx, const void *d_items, uint64_t n_items);
/* (Replaces, like the calls around it, the per-call merge of thread-local k-mer tables into ONE map, trim.cpp:133-135, for a map that is
 * partitioned over devices.)  The exchange inside ONE process that drives several devices (faqcs_mi --gpus N --kmer_rarefaction): moves the last submission's
 * outbox of `from` to the owner contexts (owners[r] = the context faqcs_kmer_partition() made rank r of `world`) and inserts
 * it there; a peer copy when the owner sits on another device.  Returns when the outbox may be overwritten. */
int  faqcs_kmer_forward(faqcs_ctx *from, faqcs_ctx *const *owners, uint32_t world);
/* Owner side: keys by first epoch and occurrences by epoch of THIS rank's table ([n_epochs] each, cap >= n_epochs). */
int  faqcs_kmer_epoch_counts(faqcs_ctx *ctx, uint64_t *distinct_by_first_epoch, uint64_t *total_by_epoch, uint32_t cap);

/* ---- measurement helpers (used by bench.py; not part of the reference seam) ---- */
/* Fills device arenas with the SURVEY section-8(d) synthetic reads (counter-based PRNG keyed by
 * (seed, first_read + i)); stride == L (packed).  d_offset gets n_reads+1 entries. */
int  faqcs_synth_fill(int device_id, uint8_t *d_seq, uint8_t *d_qual, uint32_t *d_offset, uint32_t n_reads,
                      uint32_t L, uint64_t seed, uint64_t first_read, float adapter_frac);
/* terminal_n flags (faqcs_batch) of a device-resident batch, computed on the device: d_flags[i], i < n_reads */
int  faqcs_terminal_n_flags(int device_id, const uint8_t *d_seq, const uint32_t *d_offset, uint32_t n_reads, uint8_t *d_flags);
/* The k-mer configuration of SURVEY section 8(d): reads are windows of a fixed synthetic genome of genome_len bases
 * (either strand, 0.5 % substitutions, the same quality recipe), so distinct k-mers grow as on real data. */
int  faqcs_synth_fill_genome(int device_id, uint8_t *d_seq, uint8_t *d_qual, uint32_t *d_offset, uint32_t n_reads,
                             uint32_t L, uint64_t seed, uint64_t first_read, uint64_t genome_len);
/* duration (ms) of the scan and of the gather of the LAST faqcs_emit_device() on the context, measured with HIP events recorded on the
 * compute stream around them; waits for that emission */
int  faqcs_emit_time_ms(faqcs_ctx *ctx, double *scan_ms, double *gather_ms);
/* the same for the LAST faqcs_parse_device() on the context: the line index and the records (index_ms), the gather (gather_ms) */
int  faqcs_parse_time_ms(faqcs_ctx *ctx, double *index_ms, double *gather_ms);
/* the same for the LAST faqcs_render_device() on the context: the scan (scan_ms), the gather (gather_ms) */
int  faqcs_render_time_ms(faqcs_ctx *ctx, double *scan_ms, double *gather_ms);
/* the same for the LAST faqcs_pair_device() on the context: the ids, the route and the tile partials (check_ms), the finishing block (finish_ms) */
int  faqcs_pair_time_ms(faqcs_ctx *ctx, double *check_ms, double *finish_ms);
/* the same for the LAST faqcs_render_pair_device() on the context: the scan (scan_ms), the gather (gather_ms) */
int  faqcs_render_pair_time_ms(faqcs_ctx *ctx, double *scan_ms, double *gather_ms);
/* the same for the LAST faqcs_inflate_device() on the context: the scan of the headers (scan_ms), the decode with its CRC and the status (decode_ms) */
int  faqcs_inflate_time_ms(faqcs_ctx *ctx, double *scan_ms, double *decode_ms);
/* the same for the LAST faqcs_gunzip_device() or faqcs_gunzip_stream_device() on the context: every count round (count_ms), the decode pass,
 * the narrowing with its CRC and the two window kernels (decode_ms), the resolve pass -- the serial part, one step per piece -- (resolve_ms) */
int  faqcs_gunzip_time_ms(faqcs_ctx *ctx, double *count_ms, double *decode_ms, double *resolve_ms);
/* the same for the LAST faqcs_deflate_device() on the context: the members' encoding into their slots (encode_ms), sizes, positions and the gather (gather_ms) */
int  faqcs_deflate_time_ms(faqcs_ctx *ctx, double *encode_ms, double *gather_ms);
/* diagnostic builds only: section clocks accumulated by the trim kernel (16 words; read and cleared) */
int  faqcs_debug_words(faqcs_ctx *ctx, uint64_t *out, uint32_t n);
/* average duration (ms) of the dominant kernel over the launches since the last call, measured with
 * HIP events recorded on the compute stream around each launch */
int  faqcs_kernel_time_ms(faqcs_ctx *ctx, double *avg_ms, uint64_t *n_launches);
/* the same per kernel: the trim kernel (and which variant ran: "trim_lds", "trim_filter_accumulate", "trim_long") and the
 * adapter pre-pass adapter_overlap (0 without adapters; a library of several target groups: all its launches); both measured with HIP events on the compute stream */
typedef struct faqcs_kernel_times {
    double trim_ms, adapter_ms; uint64_t n_launches; const char *trim_kernel;
    double kmer_ms;        /* k-mer kernels of a submission (kmer_count; kmer_extract in the owner-partitioned mode), per submission */
    double kmer_insert_ms; /* faqcs_kmer_insert_device (owner-partitioned mode), per submission */
} faqcs_kernel_times;
int  faqcs_kernel_report(faqcs_ctx *ctx, faqcs_kernel_times *out);

#ifdef __cplusplus
}
#endif
#endif /* FAQCS_MI_H */
