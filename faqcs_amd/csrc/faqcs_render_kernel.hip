// faqcs_render_kernel.hip -- faqcs_render_device(): the FASTQ text of the reference's output files, assembled on the device.
//
// One rendered record is  defline '\n' S "\n+\n" Q '\n'  (fastq.cpp:127-138).  With per-read results (the trimmed streams) S / Q are the kept
// window with the byte edits of faqcs_apply_edits(); without them (the discard stream) S / Q are the read as it came.  The bytes are read
// STRAIGHT from the input: the defline from the FASTQ text faqcs_parse_device() indexed, bases and qualities from the batch's arenas.
//
// Two steps on the compute stream, in the shape of faqcs_emit_kernel.hip:
//   scan    render_tile_totals -> render_scan_tiles -> render_scan_apply.  A tile is 1 024 consecutive CANDIDATES (4 per thread); candidate j
//           is read order[j] (j without an order).  Per candidate size = rendered ? def_len + 2 len + 5 : 0, summed in 64 bits; the exclusive
//           prefix sums of (size, rendered) give every rendered record k its text range and a 32-byte descriptor
//           {begin, end, arena position of the window, kept-quality range | defline position, defline length, window length, -}.
//           Only reads whose first or last base is 'N' scan their ends: a wave per such read (wave_terminal_extents).
//   gather  render_gather<MASKED, EDIT>.  OUTPUT-centric: a lane owns one 16-byte aligned piece of the text, a wave 64 consecutive pieces (1 KiB).
//           The record under a span's first byte is found by binary search in the record offsets (wave-uniform, once per 8 KiB span); inside
//           a span the wave carries the record index along and every lane finds its own record among the next 64 offsets with 6 cross-lane
//           steps (more than 64 records ending in one KiB -- 5-byte records -- take the lane's own search).  A piece is first filled with
//           '\n' over the record's bytes, then up to three unaligned 16-byte loads per record -- defline, bases, qualities, each issued only
//           by the lanes whose piece holds such bytes, each addressed so that the bytes arrive in place -- are merged under byte masks, then
//           the '+' is placed; ONE aligned 16-byte vector store per piece.
//           EDIT = false (--replace_to_N_q 0, input offset == output offset: the default, and always for the discard stream) copies;
//           only flagged reads touch their quality.  EDIT = true with --replace_to_N_q loads the qualities under a piece's bases as well.
// The kernels use no atomics and only vector stores.
#include "faqcs_edit_common.h"

namespace {

using namespace faqcs_edit;

constexpr uint32_t TILE_THREADS = 256, TILE_RPT = 4, TILE_CAND = TILE_THREADS * TILE_RPT;
constexpr uint32_t SCAN_THREADS = 1024;
constexpr uint32_t SPAN_ITERS = 8, WAVE_BYTES = FAQCS_WAVE * 16, SPAN_BYTES = SPAN_ITERS * WAVE_BYTES;
constexpr uint32_t GATHER_THREADS = 256;

struct TileSum { unsigned long long bytes; uint32_t recs, pad; };    // of one tile (def_len is 32 bits wide: 64-bit sums throughout)
struct TilePrefix { unsigned long long bytes; uint32_t recs, pad; }; // of the tiles in front of one

// the inputs of the scan, by value
struct RenderIn {
    const uint8_t *seq;
    const uint32_t *in_off;
    const uint8_t *tn;
    const faqcs_read_result *res; // nullptr: the discard stream (whole reads, as they came)
    const uint32_t *def_pos, *def_len;
    const uint8_t *select;
    const uint32_t *order;
    uint32_t n;
};

// the four candidates of a thread: read index, window and defline length of each rendered one, and the selection bits
__device__ __forceinline__ uint32_t load_candidates(const RenderIn &I, unsigned long long j0, uint32_t (&idx)[TILE_RPT], uint32_t (&start)[TILE_RPT],
                                                    uint32_t (&len)[TILE_RPT], uint32_t (&dlen)[TILE_RPT])
{
    uint32_t sel = 0;
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r) {
        const unsigned long long j = j0 + r;
        idx[r] = start[r] = len[r] = dlen[r] = 0;
        if (j >= I.n) continue;
        const uint32_t i = I.order ? I.order[j] : (uint32_t)j;
        if (i >= I.n) continue; // (an order entry that names no read: skipped, never dereferenced)
        if (I.select && I.select[i] == 0) continue;
        uint32_t st = 0, ln;
        if (I.res) {
            const uint2 v = *reinterpret_cast<const uint2 *>(I.res + i);
            if (!(v.y & FAQCS_F_VALID)) continue;
            st = v.x & 0xffffu; ln = v.x >> 16;
        } else
            ln = I.in_off[(size_t)i + 1] - I.in_off[i];
        sel |= 1u << r;
        idx[r] = i; start[r] = st; len[r] = ln; dlen[r] = I.def_len[i];
    }
    return sel;
}

__device__ __forceinline__ unsigned long long record_bytes(uint32_t dlen, uint32_t len) { return (unsigned long long)dlen + 2ull * len + 5ull; }

__device__ __forceinline__ unsigned long long thread_bytes(uint32_t sel, const uint32_t (&len)[TILE_RPT], const uint32_t (&dlen)[TILE_RPT])
{
    unsigned long long b = 0;
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r)
        if (sel >> r & 1u) b += record_bytes(dlen[r], len[r]);
    return b;
}

__global__ __launch_bounds__(TILE_THREADS) void render_tile_totals(const RenderIn I, TileSum *__restrict__ tiles)
{
    __shared__ unsigned long long s_a[TILE_THREADS / 64];
    __shared__ uint32_t s_b[TILE_THREADS / 64];
    const unsigned long long j0 = (unsigned long long)blockIdx.x * TILE_CAND + threadIdx.x * TILE_RPT;
    uint32_t idx[TILE_RPT], start[TILE_RPT], len[TILE_RPT], dlen[TILE_RPT];
    const uint32_t sel = load_candidates(I, j0, idx, start, len, dlen);
    unsigned long long pa, ta;
    uint32_t pb, tb;
    block_excl_scan2<unsigned long long, TILE_THREADS>(thread_bytes(sel, len, dlen), (uint32_t)__popc(sel), s_a, s_b, pa, pb, ta, tb);
    if (threadIdx.x == 0) tiles[blockIdx.x] = TileSum{ta, tb, 0};
}

// one block: exclusive prefix of the tile sums, the totals and the overflow decision
__global__ __launch_bounds__(SCAN_THREADS) void render_scan_tiles(const TileSum *__restrict__ tiles, const uint32_t n_tiles, TilePrefix *__restrict__ prefix,
                                                                  const unsigned long long capacity, faqcs_render_info *__restrict__ info,
                                                                  uint32_t *__restrict__ offs, uint32_t *__restrict__ rec_offset)
{
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
        const unsigned long long cap = capacity < 0xffffffffull ? capacity : 0xffffffffull; // text positions are 32 bits wide
        const uint32_t over = carry_a > cap ? 1u : 0u;
        info->n_bytes = carry_a;
        info->n_reads = carry_b;
        info->overflow = over;
        offs[0] = 0; // (the library's scratch)
        if (!over && rec_offset) rec_offset[0] = 0;
    }
}

__global__ __launch_bounds__(TILE_THREADS) void render_scan_apply(const RenderIn I, const TilePrefix *__restrict__ prefix, const faqcs_render_info *__restrict__ info,
                                                                  uint32_t *__restrict__ offs, uint32_t *__restrict__ rec_offset, uint32_t *__restrict__ rec_index,
                                                                  uint4 *__restrict__ desc)
{
    __shared__ unsigned long long s_a[TILE_THREADS / 64];
    __shared__ uint32_t s_b[TILE_THREADS / 64];
    if (info->overflow) return; // nothing is written (uniform over the grid)
    const unsigned long long j0 = (unsigned long long)blockIdx.x * TILE_CAND + threadIdx.x * TILE_RPT;
    uint32_t idx[TILE_RPT], start[TILE_RPT], len[TILE_RPT], dlen[TILE_RPT];
    const uint32_t sel = load_candidates(I, j0, idx, start, len, dlen);
    unsigned long long pa, ta;
    uint32_t pb, tb;
    block_excl_scan2<unsigned long long, TILE_THREADS>(thread_bytes(sel, len, dlen), (uint32_t)__popc(sel), s_a, s_b, pa, pb, ta, tb);
    const TilePrefix tp = prefix[blockIdx.x];
    uint32_t ob = (uint32_t)(tp.bytes + pa), k = tp.recs + pb; // (no overflow: n_bytes < 2^32)
    uint32_t ra[TILE_RPT], rb[TILE_RPT], bits[TILE_RPT], kk[TILE_RPT];
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r) {
        ra[r] = rb[r] = bits[r] = kk[r] = 0;
        if (sel >> r & 1u) {
            const uint32_t i = idx[r];
            const uint32_t a = I.in_off[i], b = I.in_off[(size_t)i + 1];
            uint32_t f = 0;
            if (I.res) { // (the discard stream keeps every quality as it came)
                if (I.tn) f = I.tn[i] & 3u;
                else if (b > a) f = (I.seq[a] == 'N' ? 1u : 0u) | (I.seq[(size_t)b - 1] == 'N' ? 2u : 0u);
                if (b <= a) f = 0;
            }
            ra[r] = a; rb[r] = b; bits[r] = f; kk[r] = k;
            const uint32_t end = ob + (uint32_t)record_bytes(dlen[r], len[r]);
            offs[k + 1] = end;
            if (rec_offset) rec_offset[k + 1] = end;
            if (rec_index) rec_index[k] = i;
            desc[2 * (size_t)k] = make_uint4(ob, end, a + start[r], len[r] << 16); // every position of the window keeps its quality
            desc[2 * (size_t)k + 1] = make_uint4(I.def_pos[i], dlen[r], len[r], 0);
            ob = end;
            ++k;
        }
    }
    if (!I.res) return; // (uniform)
    // the few reads that start or end in 'N': the wave scans their ends, one read at a time
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r) {
        unsigned long long m = __ballot(bits[r] != 0);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            const uint32_t a = (uint32_t)__shfl((int)ra[r], l), b = (uint32_t)__shfl((int)rb[r], l), f = (uint32_t)__shfl((int)bits[r], l);
            uint32_t lead, trail;
            wave_terminal_extents(I.seq, a, b, f, lead, trail);
            if ((int)(threadIdx.x & 63u) == l) {
                const uint32_t s = start[r], e = s + len[r];
                const uint32_t lo = lead < s ? s : (lead > e ? e : lead), hi = trail < s ? s : (trail > e ? e : trail);
                // window positions [klo, khi) keep their quality (khi <= klo: none does)
                reinterpret_cast<uint32_t *>(desc + 2 * (size_t)kk[r])[3] = (lo - s) | (hi - s) << 16;
            }
        }
    }
}

// Bytes [lo, hi) of a 16-byte piece (0 <= lo, hi <= 16) as 16 byte-enable bits, and the enable bits of dword j as a mask of 0xff bytes: the
// gather is bound by vector instructions, and a range costs 4 + 4 x 4 of them this way against 4 x 12 for byte_range_mask.
__device__ __forceinline__ uint32_t range_bits(int lo, int hi) { return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u; }
__device__ __forceinline__ uint32_t byte_mask(uint32_t bits, int j) { return ((((bits >> (4 * j)) & 15u) * 0x00204081u) & 0x01010101u) * 0xffu; }

// a record position (64 bits: a defline length is 32 bits wide) as a byte position of the piece, clamped to the segment [d, e]
__device__ __forceinline__ int piece_pos(long long p, int d, int e) { return p < d ? d : (p > e ? e : (int)p); }

// MASKED: the trimmed streams (terminal-'N' quality masking applies); EDIT: G -> N and / or the quality re-base as well
template <bool MASKED, bool EDIT>
__global__ __launch_bounds__(GATHER_THREADS) void render_gather(const uint8_t *__restrict__ text, const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual,
                                                                const uint4 *__restrict__ desc, const uint32_t *__restrict__ offset,
                                                                const faqcs_render_info *__restrict__ info, uint8_t *__restrict__ out_text,
                                                                const int in, const int out, const int replace_q)
{
    if (info->overflow) return;
    const unsigned long long n_bytes = info->n_bytes; // < 2^32
    const uint32_t n_rec = info->n_reads;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (GATHER_THREADS / 64) + uniu(threadIdx.x >> 6);
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (GATHER_THREADS / 64);
    const uint32_t inb = (uint32_t)in & 0xffu, in4 = inb * 0x01010101u;
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
            const uint32_t offv = offset[(jx > n_rec || jx < kw) ? n_rec : jx];
            uint32_t c = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
                const uint32_t v = (uint32_t)__shfl((int)offv, (int)(c + step - 1u));
                if (v <= o32) c += step;
            }
            uint32_t k = kw + c;
            const uint32_t v63 = (uint32_t)__builtin_amdgcn_readlane((int)offv, 63);
            if (active && c == 63u && v63 <= o32) {
                // more than 64 records end inside this wave's KiB (empty deflines and windows): a search of its own
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
                uint32_t acc[4] = {0, 0, 0, 0};
                unsigned long long pos = o;
                while (pos < oend) {
                    const uint4 r = desc[2 * (size_t)k]; // {begin, end, arena position of the window, klo | khi << 16}
                    if ((unsigned long long)r.y > pos) {
                        const uint4 t = desc[2 * (size_t)k + 1]; // {defline position, defline length, window length, -}
                        const unsigned long long segend = (unsigned long long)r.y < oend ? (unsigned long long)r.y : oend;
                        const int d = (int)(pos - o), e = (int)(segend - o); // bytes [d, e) of the piece belong to this record
                        const long long rel0 = (long long)o - (long long)r.x; // record position of the piece's byte 0 (>= -15)
                        const long long D = t.y, len = t.z;
                        // record positions: [0, D) defline, D '\n', [D + 1, D + 1 + len) bases, "\n+\n", [D + 4 + len, D + 4 + 2 len) qualities, '\n'
                        const long long ps = D + 1 - rel0, pq = D + 4 + len - rel0; // piece positions of the first base / the first quality
                        const int d_lo = piece_pos(-rel0, d, e), d_hi = piece_pos(D - rel0, d, e);
                        const int s_lo = piece_pos(ps, d, e), s_hi = piece_pos(ps + len, d, e);
                        const int q_lo = piece_pos(pq, d, e), q_hi = piece_pos(pq + len, d, e);
                        const long long plus = ps + len + 1;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t m = (d == 0 && e == 16) ? 0xffffffffu : byte_mask(range_bits(d, e), j);
                            acc[j] = (acc[j] & ~m) | (0x0a0a0a0au & m);
                        }
                        if (d_hi > d_lo) {
                            const U128u v = *reinterpret_cast<const U128u *>(text + ((long long)t.x + rel0));
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const uint32_t m = byte_mask(range_bits(d_lo, d_hi), j);
                                acc[j] = (acc[j] & ~m) | (v.w[j] & m);
                            }
                        }
                        if (s_hi > s_lo) {
                            const long long src = (long long)r.z - ps; // piece byte x is window position x - ps
                            const U128u v = *reinterpret_cast<const U128u *>(seq + src);
                            U128u vq = v;
                            if (EDIT && replace_q > 0) vq = *reinterpret_cast<const U128u *>(qual + src);
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const uint32_t m = byte_mask(range_bits(s_lo, s_hi), j);
                                uint32_t s = v.w[j], q = vq.w[j];
                                // (a 'G' never lies in a terminal 'N' run: its quality needs no masking here)
                                if (EDIT && replace_q > 0) edit_dword(s, q, in, out, replace_q);
                                acc[j] = (acc[j] & ~m) | (s & m);
                            }
                        }
                        if (q_hi > q_lo) {
                            const long long src = (long long)r.z - pq;
                            const U128u v = *reinterpret_cast<const U128u *>(qual + src);
                            const uint32_t klo = r.w & 0xffffu, khi = r.w >> 16;
                            const bool flagged = MASKED && (klo != 0u || (long long)khi != len);
                            // piece bytes that keep their quality: window positions [klo, khi) -> piece bytes [klo + pq, khi + pq)
                            const int keep_lo = piece_pos(pq + klo, q_lo, q_hi), keep_hi = piece_pos(pq + khi, q_lo, q_hi);
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const uint32_t m = byte_mask(range_bits(q_lo, q_hi), j);
                                uint32_t s = 0, q = v.w[j];
                                if (flagged) {
                                    const uint32_t km = byte_mask(range_bits(keep_lo, keep_hi), j);
                                    q = (q & km) | (in4 & ~km);
                                }
                                if (EDIT) edit_dword(s, q, in, out, 0);
                                acc[j] = (acc[j] & ~m) | (q & m);
                            }
                        }
                        if (plus >= d && plus < e) {
                            const uint32_t pb = 1u << (int)plus;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const uint32_t m = byte_mask(pb, j);
                                acc[j] = (acc[j] & ~m) | (0x2b2b2b2bu & m); // '+'
                            }
                        }
                        pos = segend;
                    }
                    if ((unsigned long long)r.y <= pos) ++k;
                }
                *reinterpret_cast<uint4 *>(out_text + o) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
            }
            kw = (uint32_t)__builtin_amdgcn_readlane((int)k, 63); // a lower bound for the next KiB
        }
    }
}

} // namespace

size_t faqcs_render_tile_count(uint32_t n_reads) { return ((size_t)n_reads + TILE_CAND - 1) / TILE_CAND; }
// descriptors (32 bytes per read), record offsets (n_reads + 1), tile prefixes, tile sums
size_t faqcs_render_scratch_bytes(uint32_t n_reads)
{
    const size_t nt = faqcs_render_tile_count(n_reads);
    return (size_t)n_reads * 2 * sizeof(uint4) + nt * sizeof(TilePrefix) + nt * sizeof(TileSum) + ((size_t)n_reads + 1) * sizeof(uint32_t) + 64;
}

namespace {
struct Scratch { uint4 *desc; TilePrefix *prefix; TileSum *tiles; uint32_t *offs; };
Scratch carve(void *scratch, uint32_t n_reads)
{
    const size_t nt = faqcs_render_tile_count(n_reads);
    Scratch s;
    s.desc = reinterpret_cast<uint4 *>(scratch);
    s.prefix = reinterpret_cast<TilePrefix *>(s.desc + 2 * (size_t)n_reads);
    s.tiles = reinterpret_cast<TileSum *>(s.prefix + nt);
    s.offs = reinterpret_cast<uint32_t *>(s.tiles + nt);
    return s;
}
} // namespace

// scratch: faqcs_render_scratch_bytes(n_reads) bytes, 16-byte aligned.  The scan: totals, overflow decision, rec_offset / rec_index, the descriptors.
hipError_t faqcs_launch_render_scan(const faqcs_batch *b, const faqcs_read_result *res, const uint32_t *def_pos, const uint32_t *def_len,
                                    const uint8_t *select, const uint32_t *order, const faqcs_render_out *out, void *scratch, hipStream_t st)
{
    const uint32_t n = b->n_reads;
    const size_t nt = faqcs_render_tile_count(n);
    const Scratch s = carve(scratch, n);
    const RenderIn I{b->seq, b->offset, b->terminal_n, res, def_pos, def_len, select, order, n};
    if (nt) hipLaunchKernelGGL(render_tile_totals, dim3((unsigned)nt), dim3(TILE_THREADS), 0, st, I, s.tiles);
    hipLaunchKernelGGL(render_scan_tiles, dim3(1), dim3(SCAN_THREADS), 0, st, s.tiles, (uint32_t)nt, s.prefix, (unsigned long long)out->capacity_bytes, out->info, s.offs, out->rec_offset);
    if (nt) hipLaunchKernelGGL(render_scan_apply, dim3((unsigned)nt), dim3(TILE_THREADS), 0, st, I, s.prefix, out->info, s.offs, out->rec_offset, out->rec_index, s.desc);
    return hipGetLastError();
}

// The gather behind the scan (same scratch).
hipError_t faqcs_launch_render_gather(const faqcs_batch *b, bool trimmed, const uint8_t *text, const faqcs_render_out *out, const void *scratch,
                                      int in_off, int out_off, uint32_t replace_q, int n_cu, hipStream_t st)
{
    const uint32_t n = b->n_reads;
    const Scratch s = carve(const_cast<void *>(scratch), n);
    // the text cannot exceed min(capacity, 2^32 - 1) bytes; the grid is cut to that and to the device, the waves stride over the spans
    const unsigned long long most = out->capacity_bytes < 0xffffffffull ? out->capacity_bytes : 0xffffffffull;
    const unsigned long long spans = (most + SPAN_BYTES - 1) / SPAN_BYTES;
    unsigned long long grid = (spans + GATHER_THREADS / 64 - 1) / (GATHER_THREADS / 64);
    const unsigned long long cap = (unsigned long long)(n_cu > 0 ? n_cu : 256) * 8;
    if (grid > cap) grid = cap;
    if (!grid || !n) return hipSuccess;
    const bool edit = trimmed && (replace_q > 0 || in_off != out_off);
#define FAQCS_RENDER_GATHER(M, E, RQ) \
    hipLaunchKernelGGL((render_gather<M, E>), dim3((unsigned)grid), dim3(GATHER_THREADS), 0, st, text, b->seq, b->qual, s.desc, s.offs, out->info, out->text, in_off, out_off, RQ)
    if (edit) FAQCS_RENDER_GATHER(true, true, (int)replace_q);
    else if (trimmed) FAQCS_RENDER_GATHER(true, false, 0);
    else FAQCS_RENDER_GATHER(false, false, 0);
#undef FAQCS_RENDER_GATHER
    return hipGetLastError();
}
