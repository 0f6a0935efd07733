// faqcs_pack_common.h -- what the three kernels that pack bytes back to back share (faqcs_emit_kernel.hip: the edited reads as packed arenas,
// faqcs_parse_kernel.hip: FASTQ text to packed arenas, faqcs_render_kernel.hip: FASTQ text of the output files): the block scan, the one-block
// scan of the tile sums, the wave-wide scan of a read's terminal 'N' runs, the walk of an output-centric gather over the records under a
// 16-byte piece, the byte masks of a piece and the byte edits of faqcs_apply_edits() on a dword.
#pragma once
#include <cstddef>
#include "faqcs_dev.h"

namespace faqcs_pack {

constexpr uint32_t TILE_THREADS = 256, TILE_RPT = 4, TILE_ITEMS = TILE_THREADS * TILE_RPT; // a tile of the emit / render scan: 4 reads per thread
constexpr uint32_t SCAN_THREADS = 1024;
constexpr uint32_t SPAN_ITERS = 8, WAVE_BYTES = FAQCS_WAVE * 16, SPAN_BYTES = SPAN_ITERS * WAVE_BYTES;
constexpr uint32_t GATHER_THREADS = 256;

struct __attribute__((packed, aligned(1))) U128u { uint32_t w[4]; };

struct TileSum { unsigned long long bytes; uint32_t recs, pad; };    // of one tile (a defline length is 32 bits wide: 64-bit sums throughout)
struct TilePrefix { unsigned long long bytes; uint32_t recs, pad; }; // of the tiles in front of one

template <class T> __device__ __forceinline__ T wave_incl_scan(T v)
{
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// exclusive prefix of (a, b) over the threads of a block of NT threads, and the block's totals; s_a / s_b: NT / 64 entries each.
// s_b == nullptr (a constant of the call): a alone is scanned, and everything about b folds away.
template <class TA, int NT> __device__ __forceinline__ void block_excl_scan2(TA a, uint32_t b, TA *s_a, uint32_t *s_b, TA &pre_a, uint32_t &pre_b, TA &tot_a, uint32_t &tot_b)
{
    constexpr int NW = NT / 64;
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const TA ia = wave_incl_scan(a);
    const uint32_t ib = s_b ? wave_incl_scan(b) : 0u;
    __syncthreads(); // (the arrays may still be read from the previous call)
    if (lane == 63) { s_a[w] = ia; if (s_b) s_b[w] = ib; }
    __syncthreads();
    TA wa = 0, ta = 0;
    uint32_t wb = 0, tb = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const TA xa = s_a[k];
        const uint32_t xb = s_b ? s_b[k] : 0u;
        if (k < w) { wa += xa; wb += xb; }
        ta += xa; tb += xb;
    }
    pre_a = wa + ia - a; pre_b = wb + ib - b;
    tot_a = ta; tot_b = tb;
}
template <class T, int NT> __device__ __forceinline__ void block_excl_scan(T a, T *s, T &pre, T &tot)
{
    uint32_t pb, tb;
    block_excl_scan2<T, NT>(a, 0u, s, nullptr, pre, pb, tot, tb);
}

// One block: exclusive prefix of the tile sums of an emit / render scan, the totals and the overflow decision.  offs: the record offsets the
// gather searches; rec_offset: the caller's optional copy of them, untouched on overflow.
template <class Info>
__global__ __launch_bounds__(SCAN_THREADS) void scan_tile_sums(const TileSum *__restrict__ tiles, const uint32_t n_tiles, TilePrefix *__restrict__ prefix,
                                                               const unsigned long long capacity, Info *__restrict__ info, uint32_t *__restrict__ offs,
                                                               uint32_t *__restrict__ rec_offset)
{
    static_assert(offsetof(Info, n_bytes) == 0 && sizeof(Info::n_bytes) == 8 && offsetof(Info, n_reads) == 8 && offsetof(Info, overflow) == 12 && sizeof(Info) == 16,
                  "faqcs_emit_info and faqcs_render_info lead with {n_bytes, n_reads, overflow}");
    __shared__ unsigned long long s_a[SCAN_THREADS / 64];
    __shared__ uint32_t s_b[SCAN_THREADS / 64];
    unsigned long long carry_a = 0;
    uint32_t carry_b = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += SCAN_THREADS) { // (n_tiles <= 2^22)
        const uint32_t t = t0 + threadIdx.x;
        TileSum v{0, 0, 0};
        if (t < n_tiles) v = tiles[t];
        unsigned long long pa, ta;
        uint32_t pb, tb;
        block_excl_scan2<unsigned long long, SCAN_THREADS>(v.bytes, v.recs, s_a, s_b, pa, pb, ta, tb);
        if (t < n_tiles) prefix[t] = TilePrefix{carry_a + pa, carry_b + pb, 0};
        carry_a += ta; carry_b += tb;
    }
    if (threadIdx.x == 0) {
        // output positions are 32 bits wide: 2^32 bytes or more (results that do not belong to the batch) cannot be stored either
        const unsigned long long cap = capacity < 0xffffffffull ? capacity : 0xffffffffull;
        const uint32_t over = carry_a > cap ? 1u : 0u;
        info->n_bytes = carry_a;
        info->n_reads = carry_b;
        info->overflow = over;
        offs[0] = 0;
        if (!over && rec_offset) rec_offset[0] = 0;
    }
}

// which ends of the read [a, b) are 'N' (bit 0: the first base, bit 1: the last): the batch's terminal_n when given, else the two end bytes
__device__ __forceinline__ uint32_t terminal_flags(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ tn, uint32_t i, uint32_t a, uint32_t b)
{
    if (b <= a) return 0u;
    if (tn) return tn[i] & 3u;
    return (seq[a] == 'N' ? 1u : 0u) | (seq[(size_t)b - 1] == 'N' ? 2u : 0u);
}

// [lead, trail) of a read [a, b) whose first (bit 0) / last (bit 1) base is 'N': the positions that keep their quality.  Whole wave, uniform arguments.
__device__ __forceinline__ void wave_terminal_extents(const uint8_t *__restrict__ seq, uint32_t a, uint32_t b, uint32_t bits, uint32_t &lead, uint32_t &trail)
{
    const uint32_t lane = threadIdx.x & 63u, L = b - a;
    lead = 0; trail = L;
    if (bits & 1u) {
        lead = L;
        for (uint32_t p = 0; p < L; p += 64) {
            const uint32_t x = p + lane;
            const bool stop = x >= L || seq[(size_t)a + x] != 'N';
            const unsigned long long m = __ballot(stop);
            if (m) { lead = p + (uint32_t)__builtin_ctzll(m); break; }
        }
    }
    if (bits & 2u) {
        trail = 0;
        for (uint32_t p = 0; p < L; p += 64) { // x: distance from the read's last base
            const uint32_t x = p + lane;
            const bool stop = x >= L || seq[(size_t)b - 1 - x] != 'N';
            const unsigned long long m = __ballot(stop);
            if (m) { trail = L - (p + (uint32_t)__builtin_ctzll(m)); break; }
        }
    }
}

// The few reads of a thread's TILE_RPT that start or end in 'N' (bits[r] != 0; read [ra[r], rb[r]), window [start[r], start[r] + len[r]),
// record kk[r]): the wave scans their ends, one read at a time, and patches klo | khi << 16 -- window positions [klo, khi) keep their quality,
// khi <= klo: none does -- into word 3 of the record, which lies at rec + kk[r] * STRIDE.  Whole wave.
template <uint32_t STRIDE>
__device__ __forceinline__ void mark_terminal_extents(const uint8_t *__restrict__ seq, const uint32_t (&ra)[TILE_RPT], const uint32_t (&rb)[TILE_RPT], const uint32_t (&bits)[TILE_RPT],
                                                      const uint32_t (&start)[TILE_RPT], const uint32_t (&len)[TILE_RPT], const uint32_t (&kk)[TILE_RPT], uint4 *__restrict__ rec)
{
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r) {
        unsigned long long m = __ballot(bits[r] != 0);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            const uint32_t a = (uint32_t)__shfl((int)ra[r], l), b = (uint32_t)__shfl((int)rb[r], l), f = (uint32_t)__shfl((int)bits[r], l);
            uint32_t lead, trail;
            wave_terminal_extents(seq, a, b, f, lead, trail);
            if ((int)(threadIdx.x & 63u) == l) {
                const uint32_t s = start[r], e = s + len[r];
                const uint32_t lo = lead < s ? s : (lead > e ? e : lead), hi = trail < s ? s : (trail > e ? e : trail);
                reinterpret_cast<uint32_t *>(rec + STRIDE * (size_t)kk[r])[3] = (lo - s) | (hi - s) << 16;
            }
        }
    }
}

// Bytes [lo, hi) of a 16-byte piece (0 <= lo, hi <= 16) as 16 byte-enable bits, and the enable bits of dword j as a mask of 0xff bytes: 4 + 4 x 4
// vector instructions per range.
__device__ __forceinline__ uint32_t range_bits(int lo, int hi) { return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u; }
__device__ __forceinline__ uint32_t byte_mask(uint32_t bits, int j) { return ((((bits >> (4 * j)) & 15u) * 0x00204081u) & 0x01010101u) * 0xffu; }

// a with the bytes under the 0xff bytes of m taken from v: (a & ~m) | (v & m), stated as the one three-input bit operation it is (truth table 0xd8) --
// left to the compiler, the select came out as one v_bitop3_b32 or as three and / xor instructions depending on the code around it
__device__ __forceinline__ uint32_t merge_bytes(uint32_t a, uint32_t v, uint32_t m) { return __builtin_amdgcn_bitop3_b32(a, v, m, 0xd8); }

// a position relative to the piece's byte 0 (any value) as a byte position of the piece, clamped to the segment [d, e]
template <class T> __device__ __forceinline__ int piece_pos(T p, int d, int e) { return p < d ? d : (p > e ? e : (int)p); }

// faqcs_apply_edits() on the four bytes of a dword pair (quality already masked)
__device__ __forceinline__ void edit_dword(uint32_t &s, uint32_t &q, int in, int out, int replace_q)
{
    uint32_t so = 0, qo = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        uint32_t b = (s >> (8 * t)) & 0xffu;
        const int raw = (int)(int8_t)((q >> (8 * t)) & 0xffu);
        int qs = raw - in;
        qs = qs < 0 ? 0 : qs;
        if (replace_q > 0 && b == 'G' && qs < replace_q) b = 'N';
        const uint32_t qb = in != out ? (uint32_t)(qs + out) & 0xffu : (uint32_t)raw & 0xffu;
        so |= b << (8 * t);
        qo |= qb << (8 * t);
    }
    s = so; q = qo;
}

// the quality dword j of a piece with the terminal-'N' positions of its read set to the input offset: the piece bytes of keep_bits keep theirs
__device__ __forceinline__ uint32_t mask_terminal_quality(uint32_t q, uint32_t keep_bits, int j, uint32_t in4)
{
    const uint32_t km = byte_mask(keep_bits, j);
    return merge_bytes(in4, q, km);
}

// The OUTPUT-centric gather.  n_bytes (< 2^32) of output are cut into aligned 16-byte pieces; a lane owns one piece, a wave 64 consecutive ones
// (1 KiB) and SPAN_ITERS such KiB in a row (a span); the waves of the grid stride over the spans.  Record k fills the output bytes
// [offset[k], offset[k + 1]), offset[n_rec] == n_bytes; records may be empty.  For every piece, at output position o:
//     p.clear();  then, for every non-empty record k under the piece, in order:  r = p.record(k);  p.fill(r, k, o, d, e, pos);  then  p.store(o);
// r is what the kernel keeps per record, {x = offset[k], y = offset[k + 1], ...}; [d, e) are the piece bytes of record k and pos is the output
// position of byte d.  The record under a span's first byte is found by binary search in the offsets (wave-uniform); inside a span the wave
// carries the record index along and every lane finds its own record among the next 64 offsets with 6 cross-lane steps.
template <class Piece>
__device__ __forceinline__ void for_each_piece_segment(const uint32_t *__restrict__ offset, const uint32_t n_rec, const unsigned long long n_bytes, Piece &p)
{
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (GATHER_THREADS / 64) + uniu(threadIdx.x >> 6);
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (GATHER_THREADS / 64);
    for (unsigned long long span = wave; span * SPAN_BYTES < n_bytes; span += n_waves) {
        const unsigned long long o0 = span * SPAN_BYTES;
        // the record under the span's first byte: the largest k with offset[k] <= o0 (offset[n_rec] == n_bytes > o0)
        uint32_t kw = 0;
        {
            uint32_t lo = 0, hi = n_rec; // offset[lo] <= o0 < offset[hi]
            while (hi - lo > 1) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (offset[mid] <= (uint32_t)o0) lo = mid; else hi = mid;
            }
            kw = uniu(lo);
        }
        for (uint32_t it = 0; it < SPAN_ITERS; ++it) {
            const unsigned long long ow = o0 + (unsigned long long)it * WAVE_BYTES;
            if (ow >= n_bytes) break;
            const unsigned long long o = ow + lane * 16u;
            const bool active = o < n_bytes;
            const uint32_t o32 = (uint32_t)o;
            // this lane's record: kw + (how many of offset[kw + 1 ..] are <= o)
            const uint32_t jx = kw + 1u + lane;
            const uint32_t offv = offset[(jx > n_rec || jx < kw) ? n_rec : jx]; // (jx < kw: the index wrapped)
            uint32_t c = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
                const uint32_t v = (uint32_t)__shfl((int)offv, (int)(c + step - 1u));
                if (v <= o32) c += step;
            }
            uint32_t k = kw + c;
            const uint32_t v63 = (uint32_t)__builtin_amdgcn_readlane((int)offv, 63);
            if (active && c == 63u && v63 <= o32) {
                // more than 64 records end inside this wave's KiB (records of a few bytes, empty ones): a search of its own
                uint32_t lo = kw + 64u, hi = n_rec; // offset[lo] <= o < offset[hi]
                while (hi - lo > 1) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (offset[mid] <= o32) lo = mid; else hi = mid;
                }
                k = lo;
            }
            if (!active) k = kw;
            if (active) {
                const unsigned long long oend = (o + 16u < n_bytes) ? o + 16u : n_bytes;
                p.clear();
                unsigned long long pos = o;
                while (pos < oend) { // (k < n_rec while pos < n_bytes == offset[n_rec])
                    const auto r = p.record(k);
                    if ((unsigned long long)r.y > pos) {
                        const unsigned long long segend = (unsigned long long)r.y < oend ? (unsigned long long)r.y : oend;
                        p.fill(r, k, o, (int)(pos - o), (int)(segend - o), pos);
                        pos = segend;
                    }
                    if ((unsigned long long)r.y <= pos) ++k;
                }
                p.store(o);
            }
            kw = (uint32_t)__builtin_amdgcn_readlane((int)k, 63); // a lower bound for the next KiB
        }
    }
}

// blocks of GATHER_THREADS for a gather of at most most_bytes of output: a wave per span, cut to 8 blocks per compute unit (the waves stride)
inline unsigned gather_grid(unsigned long long most_bytes, int n_cu)
{
    const unsigned long long spans = (most_bytes + SPAN_BYTES - 1) / SPAN_BYTES;
    const unsigned long long grid = (spans + GATHER_THREADS / 64 - 1) / (GATHER_THREADS / 64);
    const unsigned long long cap = (unsigned long long)(n_cu > 0 ? n_cu : 256) * 8;
    return (unsigned)(grid < cap ? grid : cap);
}

} // namespace faqcs_pack
