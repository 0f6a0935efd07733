// faqcs_render_kernel.hip -- faqcs_render_device(): the FASTQ text of the reference's output files, assembled on the device.
//
// One rendered record is  defline '\n' S "\n+\n" Q '\n'  (fastq.cpp:127-138).  With per-read results (the trimmed streams) S / Q are the kept
// window with the byte edits of faqcs_apply_edits(); without them (the discard stream) S / Q are the read as it came.  The bytes are read
// STRAIGHT from the input: the defline from the FASTQ text faqcs_parse_device() indexed, bases and qualities from the batch's arenas.
//
// Two steps on the compute stream, in the shape of faqcs_emit_kernel.hip:
//   scan    render_tile_totals -> scan_tile_sums -> render_scan_apply.  A tile is 1 024 consecutive CANDIDATES (4 per thread); candidate j
//           is read order[j] (j without an order).  Per candidate size = rendered ? def_len + 2 len + 5 : 0, summed in 64 bits; the exclusive
//           prefix sums of (size, rendered) give every rendered record k its text range and a 32-byte descriptor
//           {begin, end, arena position of the window, kept-quality range | defline position, defline length, window length, -}.
//           Only reads whose first or last base is 'N' scan their ends: a wave per such read (mark_terminal_extents).
//   gather  render_gather<MASKED, EDIT>: for_each_piece_segment (faqcs_pack_common.h) over the record offsets with RenderPiece.  A lane owns
//           one 16-byte aligned piece of the text.  A piece is first filled with '\n' over the record's bytes, then up to three unaligned
//           16-byte loads per record -- defline, bases, qualities, each issued only by the lanes whose piece holds such bytes, each addressed
//           so that the bytes arrive in place -- are merged under byte masks, then the '+' is placed; ONE aligned 16-byte vector store per piece.
//           EDIT = false (--replace_to_N_q 0, input offset == output offset: the default, and always for the discard stream) copies;
//           only flagged reads touch their quality.  EDIT = true with --replace_to_N_q loads the qualities under a piece's bases as well.
// The kernels use no atomics and only vector stores.
#include "faqcs_render_common.h"

namespace {

using namespace faqcs_pack; // the scans, the terminal-'N' scan, the piece walker, the byte masks and the byte edits; RenderPiece (faqcs_render_common.h)

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
    const unsigned long long j0 = (unsigned long long)blockIdx.x * TILE_ITEMS + threadIdx.x * TILE_RPT;
    uint32_t idx[TILE_RPT], start[TILE_RPT], len[TILE_RPT], dlen[TILE_RPT];
    const uint32_t sel = load_candidates(I, j0, idx, start, len, dlen);
    unsigned long long pa, ta;
    uint32_t pb, tb;
    block_excl_scan2<unsigned long long, TILE_THREADS>(thread_bytes(sel, len, dlen), (uint32_t)__popc(sel), s_a, s_b, pa, pb, ta, tb);
    if (threadIdx.x == 0) tiles[blockIdx.x] = TileSum{ta, tb, 0};
}

__global__ __launch_bounds__(TILE_THREADS) void render_scan_apply(const RenderIn I, const TilePrefix *__restrict__ prefix, const faqcs_render_info *__restrict__ info,
                                                                  uint32_t *__restrict__ offs, uint32_t *__restrict__ rec_offset, uint32_t *__restrict__ rec_index,
                                                                  uint4 *__restrict__ desc)
{
    __shared__ unsigned long long s_a[TILE_THREADS / 64];
    __shared__ uint32_t s_b[TILE_THREADS / 64];
    if (info->overflow) return; // nothing is written (uniform over the grid)
    const unsigned long long j0 = (unsigned long long)blockIdx.x * TILE_ITEMS + threadIdx.x * TILE_RPT;
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
            // (the discard stream keeps every quality as it came)
            ra[r] = a; rb[r] = b; bits[r] = I.res ? terminal_flags(I.seq, I.tn, i, a, b) : 0u; kk[r] = k;
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
    mark_terminal_extents<2>(I.seq, ra, rb, bits, start, len, kk, desc);
}

template <bool MASKED, bool EDIT>
__global__ __launch_bounds__(GATHER_THREADS) void render_gather(const uint8_t *__restrict__ text, const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual,
                                                                const uint4 *__restrict__ desc, const uint32_t *__restrict__ offset,
                                                                const faqcs_render_info *__restrict__ info, uint8_t *__restrict__ out_text,
                                                                const int in, const int out, const int replace_q)
{
    if (info->overflow) return;
    RenderPiece<MASKED, EDIT> p{text, seq, qual, nullptr, nullptr, nullptr, desc, out_text, in, out, replace_q, ((uint32_t)in & 0xffu) * 0x01010101u, {}}; // (faqcs_render_common.h)
    for_each_piece_segment(offset, info->n_reads, info->n_bytes, p);
}

} // namespace

size_t faqcs_render_tile_count(uint32_t n_reads) { return render_tile_count(n_reads); }
// descriptors (32 bytes per read), record offsets (n_reads + 1), tile prefixes, tile sums
size_t faqcs_render_scratch_bytes(uint32_t n_reads) { return render_scratch_bytes(n_reads); }

// scratch: faqcs_render_scratch_bytes(n_reads) bytes, 16-byte aligned.  The scan: totals, overflow decision, rec_offset / rec_index, the descriptors.
hipError_t faqcs_launch_render_scan(const faqcs_batch *b, const faqcs_read_result *res, const uint32_t *def_pos, const uint32_t *def_len,
                                    const uint8_t *select, const uint32_t *order, const faqcs_render_out *out, void *scratch, hipStream_t st)
{
    const uint32_t n = b->n_reads;
    const size_t nt = faqcs_render_tile_count(n);
    const RenderScratch s = render_carve(scratch, n);
    const RenderIn I{b->seq, b->offset, b->terminal_n, res, def_pos, def_len, select, order, n};
    if (nt) hipLaunchKernelGGL(render_tile_totals, dim3((unsigned)nt), dim3(TILE_THREADS), 0, st, I, s.tiles);
    hipLaunchKernelGGL(scan_tile_sums<faqcs_render_info>, dim3(1), dim3(SCAN_THREADS), 0, st, s.tiles, (uint32_t)nt, s.prefix, (unsigned long long)out->capacity_bytes, out->info, s.offs, out->rec_offset);
    if (nt) hipLaunchKernelGGL(render_scan_apply, dim3((unsigned)nt), dim3(TILE_THREADS), 0, st, I, s.prefix, out->info, s.offs, out->rec_offset, out->rec_index, s.desc);
    return hipGetLastError();
}

// The gather behind the scan (same scratch).
hipError_t faqcs_launch_render_gather(const faqcs_batch *b, bool trimmed, const uint8_t *text, const faqcs_render_out *out, const void *scratch,
                                      int in_off, int out_off, uint32_t replace_q, int n_cu, hipStream_t st)
{
    const uint32_t n = b->n_reads;
    const RenderScratch s = render_carve(const_cast<void *>(scratch), n);
    // the text cannot exceed min(capacity, 2^32 - 1) bytes
    const unsigned grid = gather_grid(out->capacity_bytes < 0xffffffffull ? out->capacity_bytes : 0xffffffffull, n_cu);
    if (!grid || !n) return hipSuccess;
    const bool edit = trimmed && (replace_q > 0 || in_off != out_off);
#define FAQCS_RENDER_GATHER(M, E, RQ) \
    hipLaunchKernelGGL((render_gather<M, E>), dim3(grid), dim3(GATHER_THREADS), 0, st, text, b->seq, b->qual, s.desc, s.offs, out->info, out->text, in_off, out_off, RQ)
    if (edit) FAQCS_RENDER_GATHER(true, true, (int)replace_q);
    else if (trimmed) FAQCS_RENDER_GATHER(true, false, 0);
    else FAQCS_RENDER_GATHER(false, false, 0);
#undef FAQCS_RENDER_GATHER
    return hipGetLastError();
}
