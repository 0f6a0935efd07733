// faqcs_emit_kernel.hip -- faqcs_emit_device(): the trimmed, edited reads of a device-resident batch, packed back to back on the device.
//
// What one emitted read holds is what faqcs_apply_edits() (faqcs_host.cpp) writes for it: the kept window [start, start + len) of the read,
// 'G' -> 'N' below --replace_to_N_q (trim.cpp:390-403), the quality of the read's leading / trailing upper-case 'N' runs set to the input
// offset (trim.cpp:1191-1216), the quality re-based from the input to the output offset (trim.cpp:516-525).
//
// Two steps on the compute stream:
//   scan    emit_tile_totals -> scan_tile_sums -> emit_scan_apply.  A tile is 1 024 consecutive reads (4 per thread).  Per read
//           kept = selected ? len : 0; the exclusive prefix sums of (kept, selected) over the batch give every emitted read k its output
//           range and a 16-byte record {begin, end, source position of the window, kept-quality range}.  Bytes are summed in 64 bits.
//           Only reads whose first or last base is 'N' (faqcs_batch.terminal_n, or the two end bytes) scan their ends: a wave per such read.
//   gather  emit_gather<EDIT>: for_each_piece_segment (faqcs_pack_common.h) over out->offset with EmitPiece.  A lane owns one 16-byte
//           aligned piece of the output arenas and stores it with one aligned 16-byte vector store per arena.  A piece that lies inside one
//           read -- nearly all of them at 150 bases -- is ONE unaligned 16-byte load per arena; a piece that straddles reads takes one more
//           load per further read, addressed so that the bytes land in place (source - position inside the piece) and are merged under a
//           byte mask.  EDIT = false (--replace_to_N_q 0, input offset == output offset: the default) copies; only flagged reads touch
//           their quality.
// The kernels use no atomics and only vector stores.
#include "faqcs_pack_common.h"

namespace {

using namespace faqcs_pack; // the scans, the terminal-'N' scan, the piece walker, the byte masks and the byte edits

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
    const unsigned long long i0 = (unsigned long long)blockIdx.x * TILE_ITEMS + threadIdx.x * TILE_RPT; // (a tile may reach past 2^32)
    uint32_t start[TILE_RPT], len[TILE_RPT];
    const uint32_t sel = load_selection(res, keep, n, i0, start, len);
    const uint32_t bytes = len[0] + len[1] + len[2] + len[3]; // (<= 1 024 x 32 767 per tile)
    uint32_t pa, pb, ta, tb;
    block_excl_scan2<uint32_t, TILE_THREADS>(bytes, (uint32_t)__popc(sel), s_a, s_b, pa, pb, ta, tb);
    if (threadIdx.x == 0) tiles[blockIdx.x] = TileSum{ta, tb, 0};
}

__global__ __launch_bounds__(TILE_THREADS) void emit_scan_apply(const uint8_t *__restrict__ seq, const uint32_t *__restrict__ in_off, const uint8_t *__restrict__ tn,
                                                                const faqcs_read_result *__restrict__ res, const uint8_t *__restrict__ keep, const uint32_t n,
                                                                const TilePrefix *__restrict__ prefix, const faqcs_emit_info *__restrict__ info,
                                                                uint32_t *__restrict__ offset, uint32_t *__restrict__ index, uint4 *__restrict__ rec)
{
    __shared__ uint32_t s_a[TILE_THREADS / 64], s_b[TILE_THREADS / 64];
    if (info->overflow) return; // nothing is written (uniform over the grid)
    const unsigned long long i0 = (unsigned long long)blockIdx.x * TILE_ITEMS + threadIdx.x * TILE_RPT; // (a tile may reach past 2^32)
    uint32_t start[TILE_RPT], len[TILE_RPT];
    const uint32_t sel = load_selection(res, keep, n, i0, start, len);
    const uint32_t bytes = len[0] + len[1] + len[2] + len[3];
    uint32_t pa, pb, ta, tb;
    block_excl_scan2<uint32_t, TILE_THREADS>(bytes, (uint32_t)__popc(sel), s_a, s_b, pa, pb, ta, tb);
    const TilePrefix tp = prefix[blockIdx.x];
    uint32_t ob = (uint32_t)(tp.bytes + pa), k = tp.recs + pb; // (no overflow: n_bytes < 2^32)
    uint32_t ra[TILE_RPT], rb[TILE_RPT], bits[TILE_RPT], kk[TILE_RPT];
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r) {
        ra[r] = rb[r] = bits[r] = kk[r] = 0;
        if (sel >> r & 1u) {
            const uint32_t i = (uint32_t)(i0 + r);
            const uint32_t a = in_off[i], b = in_off[(size_t)i + 1];
            ra[r] = a; rb[r] = b; bits[r] = terminal_flags(seq, tn, i, a, b); kk[r] = k;
            offset[k + 1] = ob + len[r];
            if (index) index[k] = i;
            rec[k] = make_uint4(ob, ob + len[r], a + start[r], len[r] << 16); // every position of the window keeps its quality
            ob += len[r];
            ++k;
        }
    }
    mark_terminal_extents<1>(seq, ra, rb, bits, start, len, kk, rec);
}

// a piece of the two output arenas
template <bool EDIT> struct EmitPiece {
    const uint8_t *__restrict__ seq, *__restrict__ qual;
    const uint4 *__restrict__ rec;
    uint8_t *__restrict__ out_seq, *__restrict__ out_qual;
    int in, out, replace_q;
    uint32_t in4; // the input offset in every byte
    uint32_t as[4], aq[4];

    __device__ __forceinline__ void clear() { as[0] = as[1] = as[2] = as[3] = aq[0] = aq[1] = aq[2] = aq[3] = 0; }
    __device__ __forceinline__ uint4 record(uint32_t k) const { return rec[k]; } // {begin, end, source position of the window, klo | khi << 16}
    __device__ __forceinline__ void fill(const uint4 &r, uint32_t, unsigned long long, int d, int e, unsigned long long pos)
    {
        const uint32_t w0 = (uint32_t)pos - r.x; // window position of byte d
        const size_t src = (size_t)r.z + w0;
        const U128u vs = *reinterpret_cast<const U128u *>(seq + src - d);
        const U128u vq = *reinterpret_cast<const U128u *>(qual + src - d);
        const uint32_t klo = r.w & 0xffffu, khi = r.w >> 16, wlen = r.y - r.x;
        const bool flagged = klo != 0u || khi != wlen;
        // piece bytes that keep their quality: window positions [klo, khi) -> piece bytes [klo - w0 + d, khi - w0 + d)
        const uint32_t keep = range_bits(piece_pos((int)klo - (int)w0 + d, d, e), piece_pos((int)khi - (int)w0 + d, d, e));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t m = (d == 0 && e == 16) ? 0xffffffffu : byte_mask(range_bits(d, e), j);
            uint32_t s = vs.w[j], q = vq.w[j];
            if (flagged) q = mask_terminal_quality(q, keep, j, in4);
            if (EDIT) edit_dword(s, q, in, out, replace_q);
            as[j] = merge_bytes(as[j], s, m);
            aq[j] = merge_bytes(aq[j], q, m);
        }
    }
    __device__ __forceinline__ void store(unsigned long long o) const
    {
        *reinterpret_cast<uint4 *>(out_seq + o) = make_uint4(as[0], as[1], as[2], as[3]);
        *reinterpret_cast<uint4 *>(out_qual + o) = make_uint4(aq[0], aq[1], aq[2], aq[3]);
    }
};

template <bool EDIT>
__global__ __launch_bounds__(GATHER_THREADS) void emit_gather(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual, const uint4 *__restrict__ rec,
                                                              const uint32_t *__restrict__ offset, const faqcs_emit_info *__restrict__ info,
                                                              uint8_t *__restrict__ out_seq, uint8_t *__restrict__ out_qual, const int in, const int out, const int replace_q)
{
    if (info->overflow) return;
    EmitPiece<EDIT> p{seq, qual, rec, out_seq, out_qual, in, out, replace_q, ((uint32_t)in & 0xffu) * 0x01010101u, {}, {}};
    for_each_piece_segment(offset, info->n_reads, info->n_bytes, p);
}

} // namespace

size_t faqcs_emit_tile_count(uint32_t n_reads) { return ((size_t)n_reads + TILE_ITEMS - 1) / TILE_ITEMS; }
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
    hipLaunchKernelGGL(scan_tile_sums<faqcs_emit_info>, dim3(1), dim3(SCAN_THREADS), 0, st, tiles, (uint32_t)nt, prefix, (unsigned long long)out->capacity_bytes, out->info, out->offset, (uint32_t *)nullptr);
    if (nt) hipLaunchKernelGGL(emit_scan_apply, dim3((unsigned)nt), dim3(TILE_THREADS), 0, st, seq, off, tn, res, keep, n_reads, prefix, out->info, out->offset, out->index, rec);
    return hipGetLastError();
}

// The gather behind the scan (same scratch).
hipError_t faqcs_launch_emit_gather(const uint8_t *seq, const uint8_t *qual, uint32_t n_reads, const faqcs_emit_out *out, const void *scratch,
                                    int in_off, int out_off, uint32_t replace_q, int n_cu, hipStream_t st)
{
    const uint4 *rec = reinterpret_cast<const uint4 *>(scratch);
    // the emission cannot exceed min(capacity, 2^32 - 1, 32 767 bytes per read) bytes
    unsigned long long most = out->capacity_bytes < 0xffffffffull ? out->capacity_bytes : 0xffffffffull;
    if ((unsigned long long)n_reads * FAQCS_MAX_READ_LENGTH < most) most = (unsigned long long)n_reads * FAQCS_MAX_READ_LENGTH;
    const unsigned grid = gather_grid(most, n_cu);
    if (!grid) return hipSuccess;
    const bool edit = replace_q > 0 || in_off != out_off;
    if (edit) hipLaunchKernelGGL(emit_gather<true>, dim3(grid), dim3(GATHER_THREADS), 0, st, seq, qual, rec, out->offset, out->info, out->seq, out->qual, in_off, out_off, (int)replace_q);
    else hipLaunchKernelGGL(emit_gather<false>, dim3(grid), dim3(GATHER_THREADS), 0, st, seq, qual, rec, out->offset, out->info, out->seq, out->qual, in_off, out_off, 0);
    return hipGetLastError();
}
