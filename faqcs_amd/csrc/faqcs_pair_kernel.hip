// faqcs_pair_kernel.hip -- the pair stage of the device seam (include/faqcs_mi.h at faqcs_pair_device): the two mates
// of a paired run as TWO batches -- two texts, two sets of defline spans, two result arrays -- checked, routed and rendered without a join.
//
// faqcs_pair_device, three kernels on the compute stream:
//   pair_check      a lane per pair, a tile of 256 pairs per block.  The lane finds the id (parse_id, trim.cpp:188-222) of both deflines with
//                   unaligned 16-byte loads from the two texts -- the first ' ' under a byte mask, the ".1" / "/2" suffix from two bytes --
//                   and compares the ids 16 bytes at a time.  It writes route[i] and the tile's partial: its first mismatching pair with
//                   that pair's two id lengths, and the sums over the pairs IN FRONT of that pair (every pair when none mismatches).
//   pair_finish     one block: the lowest first mismatch over the tiles, then the sums of the tiles up to and including its tile -> info.
//   pair_void_tail  only when there is a mismatch: route[n_pairs .. n) = FAQCS_ROUTE_NOWHERE (tiles behind the bad one wrote theirs).
// faqcs_render_pair_device: the scan and the gather of faqcs_render_kernel.hip over the CANDIDATES j = 2 i + s (pair i, mate s), with every
// source array chosen by s.  A thread's four candidates are two whole pairs, so s is a constant of the unrolled code in the scan; the gather
// reads the mate from word 3 of a record's second descriptor and selects between two sets of text / seq / qual pointers (RenderPiece<.., PAIRED>,
// faqcs_render_common.h).
// The kernels use no atomics and only vector stores: the bytes of info, route and the texts are a function of the inputs alone.
#include "faqcs_ctx.h"
#include "faqcs_render_common.h"

namespace {

using namespace faqcs_pack;

constexpr uint32_t PAIR_THREADS = 256, NONE = 0xffffffffu;

// of one tile of PAIR_THREADS pairs: the first pair whose ids differ (NONE: none does) with its id lengths, and the sums over the pairs in front of it
struct PairPartial { uint32_t first, n_both, n_one, n_none, bases, id_len[2], pad; };
static_assert(sizeof(PairPartial) == 32, "two 16-byte words");

struct MateIds { const uint8_t *text; const uint32_t *def_pos, *def_len; const faqcs_read_result *res; };

// one bit per byte of v that equals the byte in every position of pat: bit 4 j + t is byte t of dword j
__device__ __forceinline__ uint32_t equal_bits(const U128u &v, const U128u &pat)
{
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = v.w[j] ^ pat.w[j];
        const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); // 0x80 in every byte of x that is zero, exactly
        bits |= ((((z >> 7) * 0x00204081u) >> 21) & 15u) << (4 * j);
    }
    return bits;
}
__device__ __forceinline__ uint32_t first_bits(uint32_t left) { return left < 16u ? (1u << left) - 1u : 0xffffu; } // the first min(left, 16) bytes of a vector

// parse_id: the id of the defline p[0 .. len) is its first `loc` bytes.  Loads whole vectors: up to 15 bytes behind the defline are read.
__device__ __forceinline__ uint32_t id_length(const uint8_t *__restrict__ p, uint32_t len)
{
    const U128u spaces{{0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u}};
    uint32_t loc = len;
    for (uint32_t o = 0; o < len; o += 16) {
        const uint32_t m = equal_bits(*reinterpret_cast<const U128u *>(p + o), spaces) & first_bits(len - o);
        if (m) { loc = o + (uint32_t)__builtin_ctz(m); break; }
    }
    if (loc > 1) {
        const uint32_t digit = p[loc - 1], mark = p[loc - 2];
        if (digit - '0' < 10u && (mark == '.' || mark == '/')) loc -= 2;
    }
    return loc;
}

__global__ __launch_bounds__(PAIR_THREADS) void pair_check(const MateIds A, const MateIds B, const uint32_t n, uint8_t *__restrict__ route, PairPartial *__restrict__ partial)
{
    __shared__ uint32_t s_first[PAIR_THREADS / 64], s_sum[PAIR_THREADS / 64][4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long i64 = (unsigned long long)blockIdx.x * PAIR_THREADS + threadIdx.x;
    const bool active = i64 < n;
    const uint32_t i = (uint32_t)i64;
    uint32_t la = 0, lb = 0, r = 0, bases = 0;
    bool same = true;
    if (active) {
        const uint8_t *pa = A.text + A.def_pos[i], *pb = B.text + B.def_pos[i];
        la = id_length(pa, A.def_len[i]);
        lb = id_length(pb, B.def_len[i]);
        same = la == lb;
        for (uint32_t o = 0; same && o < la; o += 16)
            same = (~equal_bits(*reinterpret_cast<const U128u *>(pa + o), *reinterpret_cast<const U128u *>(pb + o)) & first_bits(la - o)) == 0u;
        if (A.res) { // (both or neither)
            const uint2 va = *reinterpret_cast<const uint2 *>(A.res + i), vb = *reinterpret_cast<const uint2 *>(B.res + i);
            r = ((va.y & FAQCS_F_VALID) ? (uint32_t)FAQCS_ROUTE_V1 : 0u) | ((vb.y & FAQCS_F_VALID) ? (uint32_t)FAQCS_ROUTE_V2 : 0u);
            bases = (va.x >> 16) + (vb.x >> 16);
        }
    }
    // the tile's first mismatch: pairs are in thread order
    const unsigned long long bad = __ballot(active && !same);
    if (lane == 0) s_first[w] = bad ? (uint32_t)(i64 - lane) + (uint32_t)__builtin_ctzll(bad) : NONE;
    __syncthreads();
    uint32_t first = NONE;
#pragma unroll
    for (uint32_t k = 0; k < PAIR_THREADS / 64; ++k) first = first < s_first[k] ? first : s_first[k];
    const bool live = active && i < first; // (first == NONE: every pair of the tile; n <= 2^31 - 1 < NONE)
    const bool counted = live && A.res != nullptr;
    if (A.res && active) route[i] = (uint8_t)(live ? r : (uint32_t)FAQCS_ROUTE_NOWHERE);
    const uint32_t n_both = (uint32_t)__popcll(__ballot(counted && r == 3u)), n_none = (uint32_t)__popcll(__ballot(counted && r == 0u));
    const uint32_t n_one = (uint32_t)__popcll(__ballot(counted && (r == 1u || r == 2u)));
    uint32_t sum = (counted && r == 3u) ? bases : 0u; // (at most 256 x 2 x 65 535)
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d);
    if (lane == 0) { s_sum[w][0] = n_both; s_sum[w][1] = n_one; s_sum[w][2] = n_none; s_sum[w][3] = sum; }
    __syncthreads();
    uint32_t *out = reinterpret_cast<uint32_t *>(partial + blockIdx.x);
    if (threadIdx.x == 0) {
        uint32_t t[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < PAIR_THREADS / 64; ++k)
            for (int x = 0; x < 4; ++x) t[x] += s_sum[k][x];
        *reinterpret_cast<uint4 *>(out) = make_uint4(first, t[0], t[1], t[2]);
        out[4] = t[3];
        out[7] = 0;
    }
    if (first == NONE ? threadIdx.x == 0 : (active && i == first)) { out[5] = first == NONE ? 0u : la; out[6] = first == NONE ? 0u : lb; }
}

template <class T, class Op> __device__ __forceinline__ T block_reduce(T v, T *s, Op op)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d; d >>= 1) v = op(v, (T)__shfl_xor(v, d));
    __syncthreads(); // (s may still be read from the previous call)
    if (lane == 0) s[w] = v;
    __syncthreads();
    T t = s[0];
    for (uint32_t k = 1; k < SCAN_THREADS / 64; ++k) t = op(t, s[k]);
    return t;
}

__global__ __launch_bounds__(SCAN_THREADS) void pair_finish(const PairPartial *__restrict__ partial, const uint32_t n_tiles, const uint32_t n, faqcs_pair_info *__restrict__ info)
{
    __shared__ unsigned long long s64[SCAN_THREADS / 64];
    __shared__ uint32_t s32[SCAN_THREADS / 64];
    uint32_t first = NONE;
    for (uint32_t t = threadIdx.x; t < n_tiles; t += SCAN_THREADS) {
        const uint32_t f = partial[t].first;
        first = first < f ? first : f;
    }
    first = block_reduce(first, s32, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
    const uint32_t take = first == NONE ? n_tiles : first / PAIR_THREADS + 1u; // tiles behind the bad pair's count nothing
    unsigned long long both = 0, one = 0, none = 0, bases = 0;
    for (uint32_t t = threadIdx.x; t < take; t += SCAN_THREADS) {
        const uint4 v = *reinterpret_cast<const uint4 *>(partial + t);
        both += v.y; one += v.z; none += v.w; bases += partial[t].bases;
    }
    const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
    both = block_reduce(both, s64, add);
    one = block_reduce(one, s64, add);
    none = block_reduce(none, s64, add);
    bases = block_reduce(bases, s64, add);
    if (threadIdx.x == 0) {
        const bool bad = first != NONE;
        info->paired_read_number = 2ull * both;
        info->paired_base_length = bases;
        info->n_pairs = bad ? first : n;
        info->mismatch = bad ? 1u : 0u;
        info->id_len[0] = bad ? partial[first / PAIR_THREADS].id_len[0] : 0u;
        info->id_len[1] = bad ? partial[first / PAIR_THREADS].id_len[1] : 0u;
        info->n_one_valid = (uint32_t)one;
        info->n_none_valid = (uint32_t)none;
    }
}

__global__ __launch_bounds__(256) void pair_void_tail(const faqcs_pair_info *__restrict__ info, const uint32_t n, uint8_t *__restrict__ route)
{
    if (!info->mismatch) return;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)info->n_pairs + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        route[i] = (uint8_t)FAQCS_ROUTE_NOWHERE;
}

// ---- faqcs_render_pair_device ----------------------------------------------------------------------------------------------------------------

struct MateScan { const uint8_t *seq; const uint32_t *off; const uint8_t *tn; const faqcs_read_result *res; const uint32_t *def_pos, *def_len; };
struct PairRenderIn { MateScan m[2]; const uint8_t *route; uint32_t n; int file; }; // n: candidates, 2 n_pairs

// the four candidates of a thread -- two pairs: r >> 1, mate r & 1 -- pair index, window and defline length of each rendered one, and the selection bits
__device__ __forceinline__ uint32_t load_pair_candidates(const PairRenderIn &I, unsigned long long j0, uint32_t (&idx)[TILE_RPT], uint32_t (&start)[TILE_RPT],
                                                         uint32_t (&len)[TILE_RPT], uint32_t (&dlen)[TILE_RPT])
{
    uint32_t sel = 0;
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r) {
        const unsigned long long j = j0 + r; // (j0 is a multiple of 4: the mate of candidate r is r & 1)
        const uint32_t s = r & 1u;
        const MateScan &M = I.m[s];
        idx[r] = start[r] = len[r] = dlen[r] = 0;
        if (j >= I.n) continue;
        const uint32_t i = (uint32_t)(j >> 1), rt = I.route[i];
        bool take;
        if (I.file == FAQCS_FILE_QC1) take = s == 0u && rt == 3u;
        else if (I.file == FAQCS_FILE_QC2) take = s == 1u && rt == 3u;
        else if (I.file == FAQCS_FILE_UNPAIRED) take = rt == (1u << s);
        else take = rt < 4u && !(rt >> s & 1u);
        if (!take) continue;
        uint32_t st = 0, ln;
        if (I.file != FAQCS_FILE_DISCARD) {
            const uint2 v = *reinterpret_cast<const uint2 *>(M.res + i);
            st = v.x & 0xffffu; ln = v.x >> 16;
        } else
            ln = M.off[(size_t)i + 1] - M.off[i];
        sel |= 1u << r;
        idx[r] = i; start[r] = st; len[r] = ln; dlen[r] = M.def_len[i];
    }
    return sel;
}

__device__ __forceinline__ unsigned long long pair_thread_bytes(uint32_t sel, const uint32_t (&len)[TILE_RPT], const uint32_t (&dlen)[TILE_RPT])
{
    unsigned long long b = 0;
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r)
        if (sel >> r & 1u) b += record_bytes(dlen[r], len[r]);
    return b;
}

__global__ __launch_bounds__(TILE_THREADS) void pair_render_tile_totals(const PairRenderIn I, TileSum *__restrict__ tiles)
{
    __shared__ unsigned long long s_a[TILE_THREADS / 64];
    __shared__ uint32_t s_b[TILE_THREADS / 64];
    const unsigned long long j0 = (unsigned long long)blockIdx.x * TILE_ITEMS + threadIdx.x * TILE_RPT;
    uint32_t idx[TILE_RPT], start[TILE_RPT], len[TILE_RPT], dlen[TILE_RPT];
    const uint32_t sel = load_pair_candidates(I, j0, idx, start, len, dlen);
    unsigned long long pa, ta;
    uint32_t pb, tb;
    block_excl_scan2<unsigned long long, TILE_THREADS>(pair_thread_bytes(sel, len, dlen), (uint32_t)__popc(sel), s_a, s_b, pa, pb, ta, tb);
    if (threadIdx.x == 0) tiles[blockIdx.x] = TileSum{ta, tb, 0};
}

__global__ __launch_bounds__(TILE_THREADS) void pair_render_scan_apply(const PairRenderIn I, const TilePrefix *__restrict__ prefix, const faqcs_render_info *__restrict__ info,
                                                                       uint32_t *__restrict__ offs, uint32_t *__restrict__ rec_offset, uint32_t *__restrict__ rec_index,
                                                                       uint4 *__restrict__ desc)
{
    __shared__ unsigned long long s_a[TILE_THREADS / 64];
    __shared__ uint32_t s_b[TILE_THREADS / 64];
    if (info->overflow) return; // nothing is written (uniform over the grid)
    const unsigned long long j0 = (unsigned long long)blockIdx.x * TILE_ITEMS + threadIdx.x * TILE_RPT;
    uint32_t idx[TILE_RPT], start[TILE_RPT], len[TILE_RPT], dlen[TILE_RPT];
    const uint32_t sel = load_pair_candidates(I, j0, idx, start, len, dlen);
    unsigned long long pa, ta;
    uint32_t pb, tb;
    block_excl_scan2<unsigned long long, TILE_THREADS>(pair_thread_bytes(sel, len, dlen), (uint32_t)__popc(sel), s_a, s_b, pa, pb, ta, tb);
    const TilePrefix tp = prefix[blockIdx.x];
    const bool trimmed = I.file != FAQCS_FILE_DISCARD;
    uint32_t ob = (uint32_t)(tp.bytes + pa), k = tp.recs + pb; // (no overflow: n_bytes < 2^32)
    uint32_t ra[TILE_RPT], rb[TILE_RPT], bits[2][TILE_RPT], kk[TILE_RPT];
#pragma unroll
    for (uint32_t r = 0; r < TILE_RPT; ++r) {
        const uint32_t s = r & 1u;
        const MateScan &M = I.m[s];
        ra[r] = rb[r] = bits[0][r] = bits[1][r] = kk[r] = 0;
        if (sel >> r & 1u) {
            const uint32_t i = idx[r];
            const uint32_t a = M.off[i], b = M.off[(size_t)i + 1];
            // (the discard stream keeps every quality as it came)
            ra[r] = a; rb[r] = b; bits[s][r] = trimmed ? terminal_flags(M.seq, M.tn, i, a, b) : 0u; kk[r] = k;
            const uint32_t end = ob + (uint32_t)record_bytes(dlen[r], len[r]);
            offs[k + 1] = end;
            if (rec_offset) rec_offset[k + 1] = end;
            if (rec_index) rec_index[k] = (uint32_t)(j0 + r);
            desc[2 * (size_t)k] = make_uint4(ob, end, a + start[r], len[r] << 16); // every position of the window keeps its quality
            desc[2 * (size_t)k + 1] = make_uint4(M.def_pos[i], dlen[r], len[r], s);
            ob = end;
            ++k;
        }
    }
    if (!trimmed) return; // (uniform)
    // the ends of mate 0's reads lie in mate 0's arena, those of mate 1's in mate 1's: one pass of the wave over each
    mark_terminal_extents<2>(I.m[0].seq, ra, rb, bits[0], start, len, kk, desc);
    mark_terminal_extents<2>(I.m[1].seq, ra, rb, bits[1], start, len, kk, desc);
}

template <bool MASKED, bool EDIT>
__global__ __launch_bounds__(GATHER_THREADS) void pair_render_gather(const uint8_t *__restrict__ text0, const uint8_t *__restrict__ seq0, const uint8_t *__restrict__ qual0,
                                                                     const uint8_t *__restrict__ text1, const uint8_t *__restrict__ seq1, const uint8_t *__restrict__ qual1,
                                                                     const uint4 *__restrict__ desc, const uint32_t *__restrict__ offset,
                                                                     const faqcs_render_info *__restrict__ info, uint8_t *__restrict__ out_text,
                                                                     const int in, const int out, const int replace_q)
{
    if (info->overflow) return;
    RenderPiece<MASKED, EDIT, true> p{text0, seq0, qual0, text1, seq1, qual1, desc, out_text, in, out, replace_q, ((uint32_t)in & 0xffu) * 0x01010101u, {}};
    for_each_piece_segment(offset, info->n_reads, info->n_bytes, p);
}

inline size_t pair_tile_count(uint32_t n) { return ((size_t)n + PAIR_THREADS - 1) / PAIR_THREADS; }
inline MateScan scan_view(const MateDev &m) { return MateScan{m.seq, m.off, m.tn, m.res, m.def_pos, m.def_len}; }

} // namespace

// one partial per tile of pairs
size_t faqcs_pair_scratch_bytes(uint32_t n_pairs) { return (pair_tile_count(n_pairs) + 1) * sizeof(PairPartial); }

// ids, route (with results) and the tiles' partials
hipError_t faqcs_launch_pair_check(const MateDev &m1, const MateDev &m2, uint32_t n_pairs, uint8_t *route, void *scratch, hipStream_t st)
{
    const size_t nt = pair_tile_count(n_pairs);
    if (!nt) return hipSuccess;
    const MateIds A{m1.text, m1.def_pos, m1.def_len, m1.res}, B{m2.text, m2.def_pos, m2.def_len, m2.res};
    hipLaunchKernelGGL(pair_check, dim3((unsigned)nt), dim3(PAIR_THREADS), 0, st, A, B, n_pairs, route, reinterpret_cast<PairPartial *>(scratch));
    return hipGetLastError();
}

// the finishing block, and -- with a route -- the pairs behind a mismatch
hipError_t faqcs_launch_pair_finish(uint32_t n_pairs, bool routed, uint8_t *route, faqcs_pair_info *info, const void *scratch, int n_cu, hipStream_t st)
{
    const size_t nt = pair_tile_count(n_pairs);
    hipLaunchKernelGGL(pair_finish, dim3(1), dim3(SCAN_THREADS), 0, st, reinterpret_cast<const PairPartial *>(scratch), (uint32_t)nt, n_pairs, info);
    if (routed && nt) {
        const size_t cap = (size_t)(n_cu > 0 ? n_cu : 256) * 8, want = ((size_t)n_pairs + 255) / 256;
        hipLaunchKernelGGL(pair_void_tail, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, info, n_pairs, route);
    }
    return hipGetLastError();
}

// scratch: render_scratch_bytes(2 n_pairs) bytes, 16-byte aligned.  The scan over the 2 n_pairs candidates.
hipError_t faqcs_launch_render_pair_scan(int file, const MateDev &m1, const MateDev &m2, const uint8_t *route, uint32_t n_pairs, const faqcs_render_out *out,
                                         void *scratch, hipStream_t st)
{
    const uint32_t n = 2u * n_pairs; // (n_pairs <= 2^31 - 1)
    const size_t nt = render_tile_count(n);
    const RenderScratch s = render_carve(scratch, n);
    const PairRenderIn I{{scan_view(m1), scan_view(m2)}, route, n, file};
    if (nt) hipLaunchKernelGGL(pair_render_tile_totals, dim3((unsigned)nt), dim3(TILE_THREADS), 0, st, I, s.tiles);
    hipLaunchKernelGGL(scan_tile_sums<faqcs_render_info>, dim3(1), dim3(SCAN_THREADS), 0, st, s.tiles, (uint32_t)nt, s.prefix, (unsigned long long)out->capacity_bytes, out->info, s.offs, out->rec_offset);
    if (nt) hipLaunchKernelGGL(pair_render_scan_apply, dim3((unsigned)nt), dim3(TILE_THREADS), 0, st, I, s.prefix, out->info, s.offs, out->rec_offset, out->rec_index, s.desc);
    return hipGetLastError();
}

// The gather behind the scan (same scratch).
hipError_t faqcs_launch_render_pair_gather(bool trimmed, const MateDev &m1, const MateDev &m2, uint32_t n_pairs, const faqcs_render_out *out, const void *scratch,
                                           int in_off, int out_off, uint32_t replace_q, int n_cu, hipStream_t st)
{
    const uint32_t n = 2u * n_pairs;
    const RenderScratch s = render_carve(const_cast<void *>(scratch), n);
    const unsigned grid = gather_grid(out->capacity_bytes < 0xffffffffull ? out->capacity_bytes : 0xffffffffull, n_cu);
    if (!grid || !n) return hipSuccess;
    const bool edit = trimmed && (replace_q > 0 || in_off != out_off);
#define FAQCS_PAIR_GATHER(M, E, RQ) \
    hipLaunchKernelGGL((pair_render_gather<M, E>), dim3(grid), dim3(GATHER_THREADS), 0, st, m1.text, m1.seq, m1.qual, m2.text, m2.seq, m2.qual, s.desc, s.offs, out->info, out->text, in_off, out_off, RQ)
    if (edit) FAQCS_PAIR_GATHER(true, true, (int)replace_q);
    else if (trimmed) FAQCS_PAIR_GATHER(true, false, 0);
    else FAQCS_PAIR_GATHER(false, false, 0);
#undef FAQCS_PAIR_GATHER
    return hipGetLastError();
}
