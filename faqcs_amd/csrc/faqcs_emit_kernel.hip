// faqcs_emit_kernel.hip -- faqcs_emit_device(): the trimmed, edited reads of a device-resident batch, packed back to back on the device.
//
// What one emitted read holds is what faqcs_apply_edits() (faqcs_capi.hip) writes for it: the kept window [start, start + len) of the read,
// 'G' -> 'N' below --replace_to_N_q (trim.cpp:390-403), the quality of the read's leading / trailing upper-case 'N' runs set to the input
// offset (trim.cpp:1191-1216), the quality re-based from the input to the output offset (trim.cpp:516-525).
//
// Two steps on the compute stream:
//   scan    emit_tile_totals -> emit_scan_tiles -> emit_scan_apply.  A tile is 1 024 consecutive reads (4 per thread).  Per read
//           kept = selected ? len : 0; the exclusive prefix sums of (kept, selected) over the batch give every emitted read k its output
//           range and a 16-byte record {begin, end, source position of the window, kept-quality range}.  Bytes are summed in 64 bits.
//           Only reads whose first or last base is 'N' (faqcs_batch.terminal_n, or the two end bytes) scan their ends: a wave per such read.
//   gather  emit_gather<EDIT>.  OUTPUT-centric: a lane owns one 16-byte aligned piece of the output arenas, a wave 64 consecutive pieces
//           (1 KiB), and stores them with one aligned 16-byte vector store per arena.  The emitted read under a span's first byte is found
//           by binary search in out->offset (wave-uniform, once per 8 KiB span); inside a span the wave carries the read index along and every
//           lane finds its own read among the next 64 output offsets with 6 cross-lane steps.  A piece that lies inside one read -- nearly all of
//           them at 150 bases -- is ONE unaligned 16-byte load per arena; a piece that straddles reads takes one more load per further read,
//           addressed so that the bytes land in place (source - position inside the piece) and are merged under a byte mask.
//           EDIT = false (--replace_to_N_q 0, input offset == output offset: the default) copies; only flagged reads touch their quality.
// The kernels use no atomics and only vector stores.
#include "faqcs_edit_common.h"

namespace {

using namespace faqcs_edit; // the block scan, the terminal-'N' scan, the byte masks and the byte edits: shared with faqcs_render_kernel.hip

constexpr uint32_t TILE_THREADS = 256, TILE_RPT = 4, TILE_READS = TILE_THREADS * TILE_RPT;
constexpr uint32_t SCAN_THREADS = 1024;
constexpr uint32_t SPAN_ITERS = 8, WAVE_BYTES = FAQCS_WAVE * 16, SPAN_BYTES = SPAN_ITERS * WAVE_BYTES;
constexpr uint32_t GATHER_THREADS = 256;

struct TileSum { uint32_t bytes, reads; };                       // of one tile (<= 1 024 x 32 767 bytes)
struct TilePrefix { unsigned long long bytes; uint32_t reads, pad; }; // of the tiles in front of one

// the four reads of a thread: kept bytes of each (0 when the read is not emitted) and the selection bits
__device__ __forceinline__ uint32_t load_selection(const faqcs_read_result *__restrict__ res, const uint8_t *__restrict__ keep, uint32_t n, unsigned long long i0,
                                                   uint32_t (&start)[TILE_RPT], uint32_t (&len)[TILE_RPT])
{
    uint32_t sel = 0;
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r) {
        const unsigned long long i = i0 + r;
        start[r] = len[r] = 0;
        if (i < n) {
            const uint2 v = *reinterpret_cast<const uint2 *>(res + i);
            const bool s = (v.y & FAQCS_F_VALID) && (!keep || keep[i] != 0);
            if (s) { sel |= 1u << r; start[r] = v.x & 0xffffu; len[r] = v.x >> 16; }
        }
    }
    return sel;
}

__global__ __launch_bounds__(TILE_THREADS) void emit_tile_totals(const faqcs_read_result *__restrict__ res, const uint8_t *__restrict__ keep, const uint32_t n,
                                                                 TileSum *__restrict__ tiles)
{
    __shared__ uint32_t s_a[TILE_THREADS / 64], s_b[TILE_THREADS / 64];
    const unsigned long long i0 = (unsigned long long)blockIdx.x * TILE_READS + threadIdx.x * TILE_RPT; // (a tile may reach past 2^32)
    uint32_t start[TILE_RPT], len[TILE_RPT];
    const uint32_t sel = load_selection(res, keep, n, i0, start, len);
    const uint32_t bytes = len[0] + len[1] + len[2] + len[3];
    uint32_t pa, pb, ta, tb;
    block_excl_scan2<uint32_t, TILE_THREADS>(bytes, (uint32_t)__popc(sel), s_a, s_b, pa, pb, ta, tb);
    if (threadIdx.x == 0) tiles[blockIdx.x] = TileSum{ta, tb};
}

// one block: exclusive prefix of the tile sums, the totals and the overflow decision
__global__ __launch_bounds__(SCAN_THREADS) void emit_scan_tiles(const TileSum *__restrict__ tiles, const uint32_t n_tiles, TilePrefix *__restrict__ prefix,
                                                                const unsigned long long capacity, faqcs_emit_info *__restrict__ info, uint32_t *__restrict__ offset)
{
    __shared__ unsigned long long s_a[SCAN_THREADS / 64];
    __shared__ uint32_t s_b[SCAN_THREADS / 64];
    unsigned long long carry_a = 0;
    uint32_t carry_b = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += SCAN_THREADS) { // (n_tiles <= 2^22)
        const uint32_t t = t0 + threadIdx.x;
        TileSum v{0, 0};
        if (t < n_tiles) v = tiles[t];
        unsigned long long pa, ta;
        uint32_t pb, tb;
        block_excl_scan2<unsigned long long, SCAN_THREADS>((unsigned long long)v.bytes, v.reads, s_a, s_b, pa, pb, ta, tb);
        if (t < n_tiles) prefix[t] = TilePrefix{carry_a + pa, carry_b + pb, 0};
        carry_a += ta; carry_b += tb;
    }
    if (threadIdx.x == 0) {
        // output offsets are 32 bits wide: an emission of 2^32 bytes or more (results that do not belong to the batch) cannot be stored either
        const unsigned long long cap = capacity < 0xffffffffull ? capacity : 0xffffffffull;
        info->n_bytes = carry_a;
        info->n_reads = carry_b;
        info->overflow = carry_a > cap ? 1u : 0u;
        offset[0] = 0;
    }
}

__global__ __launch_bounds__(TILE_THREADS) void emit_scan_apply(const uint8_t *__restrict__ seq, const uint32_t *__restrict__ in_off, const uint8_t *__restrict__ tn,
                                                                const faqcs_read_result *__restrict__ res, const uint8_t *__restrict__ keep, const uint32_t n,
                                                                const TilePrefix *__restrict__ prefix, const faqcs_emit_info *__restrict__ info,
                                                                uint32_t *__restrict__ offset, uint32_t *__restrict__ index, uint4 *__restrict__ rec)
{
    __shared__ uint32_t s_a[TILE_THREADS / 64], s_b[TILE_THREADS / 64];
    if (info->overflow) return; // nothing is written (uniform over the grid)
    const unsigned long long i0 = (unsigned long long)blockIdx.x * TILE_READS + threadIdx.x * TILE_RPT; // (a tile may reach past 2^32)
    uint32_t start[TILE_RPT], len[TILE_RPT];
    const uint32_t sel = load_selection(res, keep, n, i0, start, len);
    const uint32_t bytes = len[0] + len[1] + len[2] + len[3];
    uint32_t pa, pb, ta, tb;
    block_excl_scan2<uint32_t, TILE_THREADS>(bytes, (uint32_t)__popc(sel), s_a, s_b, pa, pb, ta, tb);
    const TilePrefix tp = prefix[blockIdx.x];
    uint32_t ob = (uint32_t)(tp.bytes + pa), k = tp.reads + pb; // (no overflow: n_bytes < 2^32)
    uint32_t ra[TILE_RPT], rb[TILE_RPT], bits[TILE_RPT], kk[TILE_RPT], ext[TILE_RPT];
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r) {
        ra[r] = rb[r] = bits[r] = kk[r] = ext[r] = 0;
        if (sel >> r & 1u) {
            const uint32_t i = (uint32_t)(i0 + r);
            const uint32_t a = in_off[i], b = in_off[(size_t)i + 1];
            uint32_t f = 0;
            if (tn) f = tn[i] & 3u;
            else if (b > a) f = (seq[a] == 'N' ? 1u : 0u) | (seq[(size_t)b - 1] == 'N' ? 2u : 0u);
            if (b <= a) f = 0;
            ra[r] = a; rb[r] = b; bits[r] = f; kk[r] = k;
            ext[r] = len[r] << 16; // every position of the window keeps its quality
            offset[k + 1] = ob + len[r];
            if (index) index[k] = i;
            rec[k] = make_uint4(ob, ob + len[r], a + start[r], ext[r]);
            ob += len[r];
            ++k;
        }
    }
    // the few reads that start or end in 'N': the wave scans their ends, one read at a time
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
                // window positions [klo, khi) keep their quality (khi <= klo: none does)
                reinterpret_cast<uint32_t *>(rec + kk[r])[3] = (lo - s) | (hi - s) << 16;
            }
        }
    }
}

template <bool EDIT>
__global__ __launch_bounds__(GATHER_THREADS) void emit_gather(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual, const uint4 *__restrict__ rec,
                                                              const uint32_t *__restrict__ offset, const faqcs_emit_info *__restrict__ info,
                                                              uint8_t *__restrict__ out_seq, uint8_t *__restrict__ out_qual, const int in, const int out, const int replace_q)
{
    if (info->overflow) return;
    const unsigned long long n_bytes = info->n_bytes; // < 2^32
    const uint32_t n_emit = info->n_reads;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (GATHER_THREADS / 64) + uniu(threadIdx.x >> 6);
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (GATHER_THREADS / 64);
    const uint32_t inb = (uint32_t)in & 0xffu, in4 = inb * 0x01010101u;
    for (unsigned long long span = wave; span * SPAN_BYTES < n_bytes; span += n_waves) {
        const unsigned long long o0 = span * SPAN_BYTES;
        // the emitted read under the span's first byte: the largest k with offset[k] <= o0 (offset[n_emit] == n_bytes > o0)
        uint32_t kw = 0;
        {
            uint32_t lo = 0, hi = n_emit; // offset[lo] <= o0 < offset[hi]
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
            // this lane's read: kw + (how many of offset[kw + 1 ..] are <= o)
            const uint32_t jx = kw + 1u + lane;
            const uint32_t offv = offset[(jx > n_emit || jx < kw) ? n_emit : jx];
            uint32_t c = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
                const uint32_t v = (uint32_t)__shfl((int)offv, (int)(c + step - 1u));
                if (v <= o32) c += step;
            }
            uint32_t k = kw + c;
            const uint32_t v63 = (uint32_t)__builtin_amdgcn_readlane((int)offv, 63);
            if (active && c == 63u && v63 <= o32) {
                // more than 64 emitted reads end inside this wave's KiB (reads of a few bases, empty windows): a search of its own
                uint32_t lo = kw + 64u, hi = n_emit; // offset[lo] <= o < offset[hi]
                while (hi - lo > 1) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (offset[mid] <= o32) lo = mid; else hi = mid;
                }
                k = lo;
            }
            if (!active) k = kw;
            if (active) {
                const unsigned long long oend = (o + 16u < n_bytes) ? o + 16u : n_bytes;
                uint32_t as[4] = {0, 0, 0, 0}, aq[4] = {0, 0, 0, 0};
                unsigned long long pos = o;
                while (pos < oend) {
                    const uint4 r = rec[k]; // {begin, end, source position of the window, klo | khi << 16}
                    if ((unsigned long long)r.y > pos) {
                        const unsigned long long segend = (unsigned long long)r.y < oend ? (unsigned long long)r.y : oend;
                        const int d = (int)(pos - o), e = (int)(segend - o); // bytes [d, e) of the piece
                        const uint32_t w0 = (uint32_t)pos - r.x;             // window position of byte d
                        const size_t src = (size_t)r.z + w0;
                        const U128u vs = *reinterpret_cast<const U128u *>(seq + src - d);
                        const U128u vq = *reinterpret_cast<const U128u *>(qual + src - d);
                        const uint32_t klo = r.w & 0xffffu, khi = r.w >> 16, wlen = r.y - r.x;
                        const bool flagged = klo != 0u || khi != wlen;
                        // piece bytes that keep their quality: window positions [klo, khi) -> piece bytes [klo - w0 + d, khi - w0 + d)
                        const int keep_lo = (int)klo - (int)w0 + d, keep_hi = (int)khi - (int)w0 + d;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t m = (d == 0 && e == 16) ? 0xffffffffu : byte_range_mask(d, e, j);
                            uint32_t s = vs.w[j], q = vq.w[j];
                            if (flagged)
                                q = mask_terminal_quality(q, keep_lo < d ? d : keep_lo, keep_hi > e ? e : keep_hi, j, in4);
                            if (EDIT) edit_dword(s, q, in, out, replace_q);
                            as[j] = (as[j] & ~m) | (s & m);
                            aq[j] = (aq[j] & ~m) | (q & m);
                        }
                        pos = segend;
                    }
                    if ((unsigned long long)r.y <= pos) ++k;
                }
                *reinterpret_cast<uint4 *>(out_seq + o) = make_uint4(as[0], as[1], as[2], as[3]);
                *reinterpret_cast<uint4 *>(out_qual + o) = make_uint4(aq[0], aq[1], aq[2], aq[3]);
            }
            kw = (uint32_t)__builtin_amdgcn_readlane((int)k, 63); // a lower bound for the next KiB
        }
    }
}

} // namespace

size_t faqcs_emit_tile_count(uint32_t n_reads) { return ((size_t)n_reads + TILE_READS - 1) / TILE_READS; }
size_t faqcs_emit_scratch_bytes(uint32_t n_reads)
{
    const size_t nt = faqcs_emit_tile_count(n_reads);
    return (size_t)n_reads * sizeof(uint4) + nt * sizeof(TilePrefix) + nt * sizeof(TileSum) + 64;
}

// scratch: faqcs_emit_scratch_bytes(n_reads) bytes, 16-byte aligned.  The scan: totals, overflow decision, out->offset / index, the records.
hipError_t faqcs_launch_emit_scan(const uint8_t *seq, const uint32_t *off, const uint8_t *tn, uint32_t n_reads, const faqcs_read_result *res,
                                  const uint8_t *keep, const faqcs_emit_out *out, void *scratch, hipStream_t st)
{
    const size_t nt = faqcs_emit_tile_count(n_reads);
    uint4 *rec = reinterpret_cast<uint4 *>(scratch);
    TilePrefix *prefix = reinterpret_cast<TilePrefix *>(rec + n_reads);
    TileSum *tiles = reinterpret_cast<TileSum *>(prefix + nt);
    if (nt) hipLaunchKernelGGL(emit_tile_totals, dim3((unsigned)nt), dim3(TILE_THREADS), 0, st, res, keep, n_reads, tiles);
    hipLaunchKernelGGL(emit_scan_tiles, dim3(1), dim3(SCAN_THREADS), 0, st, tiles, (uint32_t)nt, prefix, (unsigned long long)out->capacity_bytes, out->info, out->offset);
    if (nt) hipLaunchKernelGGL(emit_scan_apply, dim3((unsigned)nt), dim3(TILE_THREADS), 0, st, seq, off, tn, res, keep, n_reads, prefix, out->info, out->offset, out->index, rec);
    return hipGetLastError();
}

// The gather behind the scan (same scratch).
hipError_t faqcs_launch_emit_gather(const uint8_t *seq, const uint8_t *qual, uint32_t n_reads, const faqcs_emit_out *out, const void *scratch,
                                    int in_off, int out_off, uint32_t replace_q, int n_cu, hipStream_t st)
{
    const uint4 *rec = reinterpret_cast<const uint4 *>(scratch);
    // the emission cannot exceed min(capacity, 2^32 - 1, 32 767 bytes per read) bytes; the grid is cut to that, the waves stride over the spans
    unsigned long long most = out->capacity_bytes < 0xffffffffull ? out->capacity_bytes : 0xffffffffull;
    if ((unsigned long long)n_reads * FAQCS_MAX_READ_LENGTH < most) most = (unsigned long long)n_reads * FAQCS_MAX_READ_LENGTH;
    const unsigned long long spans = (most + SPAN_BYTES - 1) / SPAN_BYTES;
    unsigned long long grid = (spans + GATHER_THREADS / 64 - 1) / (GATHER_THREADS / 64);
    const unsigned long long cap = (unsigned long long)(n_cu > 0 ? n_cu : 256) * 8;
    if (grid > cap) grid = cap;
    if (!grid) return hipSuccess;
    const bool edit = replace_q > 0 || in_off != out_off;
    if (edit) hipLaunchKernelGGL(emit_gather<true>, dim3((unsigned)grid), dim3(GATHER_THREADS), 0, st, seq, qual, rec, out->offset, out->info, out->seq, out->qual, in_off, out_off, (int)replace_q);
    else hipLaunchKernelGGL(emit_gather<false>, dim3((unsigned)grid), dim3(GATHER_THREADS), 0, st, seq, qual, rec, out->offset, out->info, out->seq, out->qual, in_off, out_off, 0);
    return hipGetLastError();
}
