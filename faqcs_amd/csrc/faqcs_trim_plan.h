// faqcs_trim_plan.h -- which trim kernel takes a submission, in which shape, and who folds the composition records: trim_plan(), the ONE
// statement of the trim dispatch.  Plain C++17 without HIP: the host side asks it once per submission
// (enqueue_trim, faqcs_capi.hip), the launchers of the three kernel files execute what it says, and tools/trim_plan_check.cpp prints it
// for tests/test_trim_plan.py.  The constexpr pieces of the kernels that the decision rests on live here and nowhere else: the length a
// shape takes, its waves per block, its LDS footprint, the chunks a trim_lds block can take between two flushes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/faqcs_mi.h"

#define FAQCS_FAST_READ_LENGTH 1024 /* longest read the chunked trim kernels and composition_histogram take; longer reads: trim_long */

// ---- tunables of the kernels that the plan depends on (a -D build has to give them to every file that includes this header) -----------
#ifndef FAQCS_TRIM_NW
#define FAQCS_TRIM_NW 4        /* trim_filter_accumulate: waves per block (A/B on MI355X: 4 waves x 3 blocks/CU beat 8 x 1 by 9 %) */
#endif
#ifndef FAQCS_TRIM_MINWAVES
#define FAQCS_TRIM_MINWAVES 3  /* trim_filter_accumulate: __launch_bounds__ 2nd argument, waves per SIMD the register allocator must allow */
#endif
// reads per chunk and waves per block of trim_lds's 16-lanes-per-read variant for 153 ... 252 bases (A/B on MI355X: DESIGN_HISTORY.md)
#ifndef FAQCS_LDS16_RPC
#define FAQCS_LDS16_RPC 32
#endif
#ifndef FAQCS_LDS16_NW
#define FAQCS_LDS16_NW 12
#endif
enum { FAQCS_TRIM_LONG_NW = 4 };     // trim_long: waves per block, a read per wave
enum { FS_SLOTS = 32 };
enum { FAQCS_PARTIAL_FLUSHES = 8 };  // flushes (rows) a trim_lds block has room for in one launch: it stops claiming chunks before it would need more

// ---- LDS layout of the accumulators (faqcs_trim_common.h: flush_block and the kernels index by it) ---------------------------------------
template <int C, int LPR, int WQ_ = 0> struct RowCfg {
    static constexpr int D = (C + 3) / 4;          // dwords per lane per arena
    static constexpr int W = LPR * C;              // positions covered by a row == columns of the LDS matrices
    static constexpr int WQ = WQ_ ? WQ_ : W;       // columns of the position x quality matrix (trim_lds: a multiple of 32, see its Q-B pass)
    // position x quality in LDS: one dword per cell (pre count lo16 / post count hi16) while that fits next to the
    // other tables (W <= 768); wider rows pack two cells per dword as 8-bit pre/post counters and the block flushes
    // them every 16 reads per wave (HQ8_EVERY x NW <= 255 increments per cell between flushes)
    static constexpr bool HQ8 = W > 768;           // (768 wide: 158 KB of the CU's 160 KB LDS, one block per CU)
    static constexpr int HQ8_EVERY = 16;
    static constexpr int HQ = HQ8 ? FAQCS_NQ * W / 2 : FAQCS_NQ * WQ;
    // |sum of (Q - q)| <= W * 168: key bias and the bit width of a position field inside the argmax keys
    static constexpr int KEY_BIAS = LPR <= 16 ? (1 << 16) : (1 << 18);
    static constexpr int PB = LPR <= 16 ? 9 : 11;
    static constexpr int FK = 2 * W;               // "first position" keys are FK - p (0 == none)
    static constexpr int HB = FAQCS_NBASE * W;
    static constexpr int O_HQ = 0;
    static constexpr int O_HB = O_HQ + HQ;
    static constexpr int O_LEN = O_HB + HB;        // [W+1] lo16 pre / hi16 post
    static constexpr int O_RQ = O_LEN + W + 2;     // [42]  lo16 pre / hi16 post
    static constexpr int O_BQPRE = O_RQ + 42;      // [42]
    static constexpr int O_BQPOST = O_BQPRE + 42;  // [42]
    static constexpr int O_FS = O_BQPOST + 42;     // [32]
    static constexpr int N_ZERO = O_FS + FS_SLOTS; // everything above is zero-initialised and flushed
    static constexpr int O_TBASE = N_ZERO;         // [256] base table
    static constexpr int O_TLC = O_TBASE + 256;    // [W+1]
    static constexpr int O_TAVGQ = O_TLC + W + 1;  // [W+1]
    static constexpr int O_TMAGIC = O_TAVGQ + W + 1;
    static constexpr int BMW = D <= 4 ? 4 : 8;     // dwords per byte-mask row (one or two ds_read_b128)
    static constexpr int O_TBM = (O_TMAGIC + W + 1 + 3) & ~3; // [C+2][BMW] byte masks "first vb bytes of the lane's dwords" (trim_lds: vb <= C + 1)
    static constexpr int LDS_DWORDS = O_TBM + BMW * (C + 2);
    static constexpr int JB = C > 16 ? 5 : 4;      // bits of a position index inside the lane-local argmax keys
};

// ---- trim_lds: what a <C, LPR, RPC> shape takes and what its block holds in LDS -------------------------------------------------------------
// Q-B's own partition of the positions (8 lanes per read, C = 19): 20 per lane instead of 19, quality rows of 160 cells.  With rows that are a
// multiple of 32 cells the bank of a cell is its position mod 32 whatever the quality; lane rl of a read starts at position 20 rl
// (banks 0, 20, 8, 28, 16, 4, 24, 12: the multiples of 4) and the four reads of a half wave walk their 20 positions ROTATED by
// 0, 1, 2, 3 bytes, so the 32 lanes of one ds_add hit 32 different banks -- and four different positions: no two adds of an
// instruction meet on a bank or on a cell (the round-2 kernel lost half of its LDS-atomic time to such conflicts).
// 16 lanes per read (C = 16, reads of 161 ... 252 bases): a lane's 16 cells are followed by one cell of padding, so lane rl starts on
// cell 17 rl -- 16 different banks in rows of 288 cells -- and the two reads of a half wave are rotated by 0 and 1 bytes
// (17 rl + 1 = 17 rl' has no solution with both lanes below 16): conflict-free as well.
// 16 lanes per read, C = 19 (reads of 253 ... 304 bases: 2x300): 20 positions per lane in Q-B as in the 8-lane variant, 21 cells per lane, rows of 352.
constexpr int lds_cq(int C, int LPR = 8) { return C == 19 ? 20 : C; }
constexpr int lds_qstride(int C, int LPR = 8) { return LPR == 16 ? lds_cq(C, LPR) + 1 : lds_cq(C, LPR); } // cells from one lane's first position to the next lane's
constexpr int lds_wq(int C, int LPR = 8) { return (LPR == 16 || C == 19) ? (LPR * lds_qstride(C, LPR) + 31) / 32 * 32 : 0; } // (8 lanes, C = 19: 160; 4 lanes: 96)
constexpr int lds_nrot(int C, int LPR = 8) { return LPR == 16 ? 2 : (C == 19 ? 4 : 1); }   // reads of a half wave = byte rotations in use
// The longest read a variant takes.  Up to 252 bases the step index of a walk lives in the low byte of the argmax keys (codes 254 - step), a
// window's start and length in a byte each, a read's N count in 8 bits; the 304-base variant (lds_wide) has nine-bit codes and fields, the
// N counts in a register of their own and two-word composition records.
constexpr int lds_maxlen(int C, int LPR = 8) { return LPR * C <= 252 ? LPR * C : (LPR * C == 256 ? 252 : LPR * C); }
constexpr bool lds_wide(int C, int LPR = 8) { return lds_maxlen(C, LPR) > 252; }
// waves per block = slots of 64 x MAXLEN bytes next to the accumulators in 160 KB: 12 x 9.8 KB + 37 KB (8 lanes per read), 6 x 16.2 KB + 63 KB (16)
constexpr int lds_waves(int C, int LPR = 8, int RPC = 64) { return LPR == 4 ? 12 : LPR == 16 ? (RPC == 64 ? 6 : (C == 19 ? 12 : FAQCS_LDS16_NW)) : (C <= 19 ? 12 : 8); }

template <int C, int NW, int LPR = 8, int RPC = 64> struct LdsCfg {
    using Row = RowCfg<C, LPR, lds_wq(C, LPR)>;
    static constexpr int CQ = lds_cq(C, LPR);                  // positions per lane in Q-B
    static constexpr int QSTRIDE = lds_qstride(C, LPR);        // cells per lane in a quality row
    static constexpr int NROT = lds_nrot(C, LPR);
    static constexpr bool ROT = NROT > 1;
    static constexpr int W = Row::W;
    static constexpr int MAXLEN = lds_maxlen(C, LPR);
    static constexpr int ND = (W + 3) / 4;                     // dwords of the longest read
    static constexpr int NP = (W + 15) / 16;                   // 16-byte pieces (the out-of-line exact passes)
    static constexpr int NWORD = (ND * 4 + 31) / 32;
    static constexpr int O_T2 = (Row::LDS_DWORDS + 3) & ~3;    // [256][2] (exact passes of rare reads) A,T,C,G one-hot in 8-bit fields ; isN(upper) | isN(any) << 1
    static constexpr int O_T3 = O_T2 + 512;                    // [256][2] S: 6-bit count fields, pre ; post (entry[b | 0x80]: b outside the kept window, pre only)
    static constexpr int O_CTR = O_T3 + 512;                   // [8] the block's chunk queue: [0] next unclaimed chunk number, [1] the block's chunk
                                                               // count once known, [4..7] ring: group number << 20 | group id
    static constexpr int O_TBQ = O_CTR + 8;                    // (ROT) [NROT][CQ + 1][8] rotated byte masks "positions < vb" of Q-B
    static constexpr int O_STG = O_TBQ + (ROT ? NROT * (CQ + 1) * 8 : 0);
    static constexpr int PADLEN = MAXLEN / 32 * 32;            // the longest read of a chunk staged as padded rows (dma_rows): L + 16 bytes each
    static constexpr int STG_BYTES = RPC * (PADLEN + 16 > MAXLEN ? PADLEN + 16 : MAXLEN) + 32; // one arena's span of a chunk (RPC reads) + 16-byte alignment slack
    static constexpr int STG_DW = (STG_BYTES + 15) / 16 * 4;
    static constexpr int TAIL_PAD = W + 64 > 256 ? (W + 64) / 4 : 64; // dwords: a lane may read W + 20 bytes from the start of the span's last read
    static constexpr int lds_dwords() { return O_STG + NW * STG_DW + TAIL_PAD; }
};
// a variant whose block owns at least the 122 KB the composition fold needs (the table of 16-bit counters, the per-length factors) folds the
// records of the launch before it when it runs out of reads (comp_fold_tail)
template <int C, int NW, int LPR, int RPC> constexpr bool lds_tail_folds_v =
    LdsCfg<C, NW, LPR, RPC>::lds_dwords() >= (FAQCS_NCOMP_BIN * FAQCS_NCOMP_KIND + 1) / 2 + 512 + 8 && lds_maxlen(C, LPR) <= 256; // (one-word records)
// chunks between two flushes of a block: the 16-bit halves of the LDS cells take FLUSH_CHUNKS x RPC <= 65535 increments in between
constexpr uint32_t lds_flush_chunks(int NW, int RPC)
{
#ifdef FAQCS_LDS_TEST_FLUSH_CHUNKS // (test build: flush every few chunks, so that a small launch goes through many flushes and fills every block's rows)
    return (uint32_t)(FAQCS_LDS_TEST_FLUSH_CHUNKS) / NW * NW;
#else
    return 65535u / RPC / NW * NW;
#endif
}
// every block can take FAQCS_PARTIAL_FLUSHES x lds_flush_chunks chunks: a launch the blocks could not take between them goes to another kernel
constexpr uint64_t lds_chunk_capacity(uint32_t grid, int NW, int RPC)
{
#ifdef FAQCS_LDS_TEST_FLUSH_CHUNKS
    return (uint64_t)grid * FAQCS_PARTIAL_FLUSHES * lds_flush_chunks(NW, RPC); // (up to the brim)
#else
    return (uint64_t)grid * FAQCS_PARTIAL_FLUSHES * lds_flush_chunks(NW, RPC) * 3 / 4;
#endif
}

// ---- the plan --------------------------------------------------------------------------------------------------------------------------
struct TrimSwitches { bool force_long, lds_on, lds4_on, lds16_on; }; // FAQCS_TRIM_LONG, FAQCS_TRIM_LDS, FAQCS_TRIM_LDS4, FAQCS_TRIM_LDS16
// the option fields the decision reads (DevParams: trim_options() in faqcs_dev.h); fold_n: composition records of the launch before this
// one that its blocks may fold (0: none)
struct TrimOptions {
    int32_t mode;
    uint32_t protect5, qc_only, replace_q, avgq_on, max_poly_n, dbg, has_adapters, trim5, trim3, fold_n;
};
enum class TrimKernel { trim_long, trim_lds, trim_filter_accumulate };
constexpr const char *trim_kernel_name(TrimKernel k) // (what faqcs_kernel_report() says)
{
    return k == TrimKernel::trim_long ? "trim_long" : k == TrimKernel::trim_lds ? "trim_lds" : "trim_filter_accumulate";
}
struct TrimPlan {
    TrimKernel kernel;
    int C, LPR, NW, RPC;     // positions per lane, lanes per read, waves per block; reads per chunk (trim_lds, else 0); trim_long: NW alone
    bool windowed;           // WINDOWED: an adapter pre-pass or --5end/--3end can move the window off [0, len)
    bool ext;                // trim_lds: EXT, trim_filter_accumulate: GENERIC -- anything but the headline option set
    bool wide_records;       // the launch writes two-word composition records (a read past 256 bases; trim_long writes none)
    bool folds_tail;         // the launch's blocks fold the fold_n records of the launch before it: no composition_histogram for them
    uint32_t grid;           // blocks
    size_t records_needed;   // entries of each record array (trim_long: its scratch of one u32 per read lives there)
};

// longest read of the batch -> <C, LPR, RPC> of trim_lds, each row from the end of the one before it.  C = 19 takes 2x125 as well: C = 16's 128-dword rows put
// every read of a half wave on the same banks (4.44 against 5.64 G reads/s).  From 153 bases on: 16 lanes per read with smaller chunks;
// equal-length chunks of a multiple of 32 bases are staged as padded rows (every lane of a lane-per-read pass would meet on one LDS bank
// otherwise).  The measurements behind this table: DESIGN_HISTORY.md.
struct TrimLdsShape { uint32_t max_len; int C, LPR, RPC, NW; bool folds_tail; };
template <int C, int LPR, int RPC> constexpr TrimLdsShape trim_lds_shape()
{
    return {(uint32_t)lds_maxlen(C, LPR), C, LPR, RPC, lds_waves(C, LPR, RPC), lds_tail_folds_v<C, lds_waves(C, LPR, RPC), LPR, RPC>};
}
constexpr TrimLdsShape TRIM_LDS_SHAPES[] = {
    trim_lds_shape<13, 4, 64>(),               //   1 ... 52    4 lanes per read: sixteen reads per step of the position-parallel passes (2x50); FAQCS_TRIM_LDS4
    trim_lds_shape<19, 4, 64>(),               //  53 ... 76    (2x75); FAQCS_TRIM_LDS4
    trim_lds_shape<13, 8, 64>(),               //  77 ... 104   8 lanes per read (2x100)
    trim_lds_shape<19, 8, 64>(),               // 105 ... 152   (2x125, 2x150)
    trim_lds_shape<16, 16, FAQCS_LDS16_RPC>(), // 153 ... 252   16 lanes per read (2x250, 2x251); FAQCS_TRIM_LDS16
    trim_lds_shape<19, 16, 20>(),              // 253 ... 304   16 lanes x 19 positions, chunks of 20 reads (2x300, 2x301: 6 KB slots, 12 waves beside a [42][352] quality matrix); FAQCS_TRIM_LDS16
};

// longest read of the batch -> <C, LPR, NW> of trim_filter_accumulate; beside each row the lengths that reach it.  The lengths trim_lds owns
// (1 ... 304) arrive here with --replace_to_N_q or a FAQCS_DBG bit (GENERIC only), with FAQCS_TRIM_LDS=0 (every option set; FAQCS_TRIM_LDS4=0:
// <= 76, FAQCS_TRIM_LDS16=0: 153 ... 304), and when a submission holds more chunks than trim_lds's blocks can take between two flushes.
// From 321 bases on there is one superset variant per width (the 512-base case keeps the default-set variant as well).
enum TrimVariants { TRIM_VARIANTS_FOUR, TRIM_VARIANTS_ALL_OR_NONE, TRIM_VARIANTS_ALL }; // the (WINDOWED, GENERIC) pairs a shape is compiled for
struct TrimTfaShape { uint32_t max_len; int C, LPR, NW; TrimVariants variants; int blocks_per_cu; };
template <int C, int LPR, int NW> constexpr TrimTfaShape trim_tfa_shape(uint32_t max_len, TrimVariants variants = TRIM_VARIANTS_FOUR)
{
    // (variants whose per-position arrays do not fit 168 VGPRs run at 2 waves/SIMD rather than spill: the kernel is issue-bound)
    constexpr int minwaves = (LPR == 8 || C > 10) ? 2 : (FAQCS_TRIM_MINWAVES > 2 ? FAQCS_TRIM_MINWAVES : 2);
    constexpr int by_waves = (4 * minwaves + NW - 1) / NW; // resident waves per CU the registers allow
    constexpr int by_lds = (160 * 1024) / (RowCfg<C, LPR>::LDS_DWORDS * 4);
    constexpr int per_cu = by_lds < by_waves ? by_lds : by_waves;
    return {max_len, C, LPR, NW, variants, per_cu < 1 ? 1 : per_cu};
}
constexpr TrimTfaShape TRIM_TFA_SHAPES[] = {
    trim_tfa_shape<16, 4, FAQCS_TRIM_NW>(64),    //   0 ... 64    4 lanes per read (2x50)
    trim_tfa_shape<19, 4, FAQCS_TRIM_NW>(76),    //  65 ... 76    (2x75)
    trim_tfa_shape<13, 8, FAQCS_TRIM_NW>(104),   //  77 ... 104   8 lanes per read (2x100)
    trim_tfa_shape<16, 8, FAQCS_TRIM_NW>(128),   // 105 ... 128
    trim_tfa_shape<19, 8, FAQCS_TRIM_NW>(152),   // 129 ... 152   (2x150: 152 position slots instead of 160)
    trim_tfa_shape<20, 8, FAQCS_TRIM_NW>(160),   // 153 ... 160
    trim_tfa_shape<13, 16, FAQCS_TRIM_NW>(208),  // 161 ... 208   16 lanes per read
    trim_tfa_shape<16, 16, FAQCS_TRIM_NW>(256),  // 209 ... 256   (2x250)
    trim_tfa_shape<10, 32, FAQCS_TRIM_NW>(320),  // 257 ... 320   two reads per wave (MiSeq 2x300); 305 ... 320 with every option set
    trim_tfa_shape<16, 32, FAQCS_TRIM_NW>(512, TRIM_VARIANTS_ALL_OR_NONE), // 321 ... 512
    trim_tfa_shape<12, 64, FAQCS_TRIM_NW>(768, TRIM_VARIANTS_ALL),         // 513 ... 768   the whole wave on one read
    trim_tfa_shape<16, 64, 8>(FAQCS_FAST_READ_LENGTH, TRIM_VARIANTS_ALL),  // 769 ... 1 024 (8 waves x 16 reads <= 255 per 8-bit cell)
};

constexpr int trim_shape_key(int C, int LPR) { return LPR * 100 + C; } // (the launchers' switch from a plan's shape to its instantiation)

inline TrimPlan trim_plan(const TrimOptions &o, const uint32_t max_len, const uint32_t n_reads, const int n_cu, const TrimSwitches &sw)
{
    const auto blocks = [](uint32_t chunks, int NW, uint32_t cap) { const uint32_t g = (chunks + NW - 1) / NW; return g > cap ? cap : g; };
    TrimPlan p{};
    // trim_long: a batch that holds a read of more than 1 024 bases; FAQCS_TRIM_LONG=1 sends every batch there (tests).  It adds the
    // composition bins itself and writes no records
    if (max_len > FAQCS_FAST_READ_LENGTH || sw.force_long) {
        p.kernel = TrimKernel::trim_long;
        p.NW = FAQCS_TRIM_LONG_NW;
        p.grid = blocks(n_reads, FAQCS_TRIM_LONG_NW, (uint32_t)n_cu * 8u); // 32 waves per CU: the passes wait on memory, not on issue slots
        p.records_needed = (size_t)n_reads / 2 + 1;
        return p;
    }
    p.wide_records = max_len > 256;
    p.records_needed = (size_t)n_reads * (p.wide_records ? 2 : 1);
    p.windowed = o.has_adapters || ((o.trim5 || o.trim3) && !o.qc_only);
    const bool plain = o.mode == FAQCS_MODE_BWA_PLUS && !o.protect5 && !o.qc_only && o.replace_q == 0 && !o.avgq_on && o.max_poly_n == 2 && o.dbg == 0;
    p.ext = !plain;
    // trim_lds: every byte from HBM once, through LDS.  Every option set except --replace_to_N_q (its G -> N edit needs base and quality of
    // a position together) and the ablation bits
    if (sw.lds_on && max_len > 0 && o.replace_q == 0 && o.dbg == 0) {
        for (const TrimLdsShape &s : TRIM_LDS_SHAPES) {
            if (max_len > s.max_len) continue;
            if ((s.LPR == 4 && !sw.lds4_on) || (s.LPR == 16 && !sw.lds16_on)) break;
            const uint32_t chunks = (n_reads + s.RPC - 1) / s.RPC;
            const uint32_t grid = blocks(chunks, s.NW, (uint32_t)n_cu); // one block per CU: its LDS holds a slot per wave
            if ((uint64_t)chunks > lds_chunk_capacity(grid, s.NW, s.RPC)) break;
            p.kernel = TrimKernel::trim_lds;
            p.C = s.C; p.LPR = s.LPR; p.NW = s.NW; p.RPC = s.RPC; p.grid = grid;
            p.folds_tail = s.folds_tail && o.fold_n != 0; // (the launch folds the records DevParams::fold_* names, all of them)
            return p;
        }
    }
    p.kernel = TrimKernel::trim_filter_accumulate;
    for (const TrimTfaShape &s : TRIM_TFA_SHAPES) {
        if (max_len > s.max_len) continue;
        if (s.variants == TRIM_VARIANTS_ALL_OR_NONE) p.windowed = p.ext = p.windowed || p.ext;
        if (s.variants == TRIM_VARIANTS_ALL) p.windowed = p.ext = true;
        p.C = s.C; p.LPR = s.LPR; p.NW = s.NW;
        p.grid = blocks((n_reads + 63) / 64, s.NW, (uint32_t)(n_cu * s.blocks_per_cu));
        break;
    }
    return p;
}
