// faqcs_gunzip_kernel.hip -- faqcs_gunzip_device: ordinary gzip in HBM to the FASTQ text faqcs_parse_device takes (include/faqcs_mi.h,
// DESIGN.md section 4.8).  The scheme and every function that decides something are faqcs_gunzip.h, the text the host statement and the
// sanitizer build compile too; the chain is walked on the host (gunzip_run, from faqcs_capi_seam.hip).  This file holds the wave that
// executes the shared text and the four kernels:
//
//   gunzip_count      ONE WAVE PER PIECE: the probe (64 positions a step, the lowest that passes decides) and the run that counts; in
//                     grid mode piece i is grid piece i, else the pieces are the records the host sent (a forced start).  No output but
//                     the 32-byte record
//   gunzip_decode     ONE WAVE PER CHAIN PIECE: the run again, into 16-bit symbols at the piece's position; the window of a match is the
//                     symbol buffer itself behind a fence of wavefront scope, what lies in front of the piece is a marker
//   gunzip_resolve    ONE BLOCK over the chain in order: the markers in the last 32 768 symbols of each piece, one barrier per piece
//   gunzip_narrow     one wave per slice of 16 KiB: symbols to bytes, the slice's CRC-32 carried to its member's end
// No global atomic anywhere and vector stores only: every word has one writer.
#include "faqcs_gunzip.h"
#include "faqcs_pack_common.h"

namespace gz = faqcs_gunzip;
namespace inf = faqcs_inflate;

namespace {

constexpr uint32_t BLOCKS_PER_CU = 24; // 5.4 KB of LDS each
constexpr uint32_t RESOLVE_THREADS = 1024;

__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uniu((uint32_t)v) | (uint64_t)uniu((uint32_t)(v >> 32)) << 32; }

// One wave as the Sink of faqcs_gunzip.h: WaveSink of faqcs_inflate_kernel.hip with 16-bit symbols.  Literals wait one per lane and leave
// together; a copy reads symbols that are all in memory before it starts, or stand in front of the piece and become markers.
struct WaveSymSink {
    uint16_t *out;
    uint32_t l, lo, hi, mine;
    __device__ __forceinline__ uint32_t lane() const { return l; }
    __device__ __forceinline__ uint32_t lanes() const { return 64; }
    __device__ __forceinline__ void sync() { __syncthreads(); } // (the block is this wave)
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return uniu(v); }
    __device__ __forceinline__ uint32_t umin(uint32_t v) const
    {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) v = umin_(v, (uint32_t)__shfl_xor((int)v, d));
        return uniu(v);
    }
    __device__ __forceinline__ void flush()
    {
        if (hi > lo) {
            const uint32_t a = (lo & ~63u) | l;
            if (a >= lo && a < hi) out[a] = (uint16_t)mine;
            lo = hi;
        }
    }
    __device__ __forceinline__ void lit(uint32_t o, uint32_t v)
    {
        if (hi == lo) lo = hi = o;
        if ((o & 63u) == l) mine = v;
        hi = o + 1;
        if ((hi & 63u) == 0) flush();
    }
    __device__ __forceinline__ void own_stores_visible() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
    __device__ __forceinline__ void match(uint32_t o, uint32_t len, uint32_t dist)
    {
        flush();
        own_stores_visible();
        uint16_t v[5];
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) { // (len <= 258)
            const uint32_t i = l + 64 * k;
            if (i < len) {
                const uint32_t j = o + (dist >= len ? i : i % dist); // source position + dist
                v[k] = j < dist ? (uint16_t)(0x8000u | (gz::WIN + j - dist)) : out[j - dist]; // (dist <= WIN)
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) {
            const uint32_t i = l + 64 * k;
            if (i < len) out[o + i] = v[k];
        }
    }
    __device__ __forceinline__ void stored(uint32_t o, const uint8_t *src, uint32_t len)
    {
        flush();
        for (uint32_t i = l; i < len; i += 64) out[o + i] = src[i];
    }
};

__device__ __forceinline__ WaveSymSink wave_sink(uint16_t *out)
{
    WaveSymSink S;
    S.out = out; S.l = threadIdx.x; S.lo = S.hi = 0; S.mine = 0;
    return S;
}

__global__ __launch_bounds__(64) void gunzip_count(const uint8_t *__restrict__ comp, const uint32_t n_comp, const uint32_t piece_bytes, gz::Piece *__restrict__ recs,
                                                   const uint32_t n, const int grid_mode)
{
    __shared__ inf::Tables T;
    WaveSymSink S = wave_sink(nullptr);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        gz::Piece pc{gz::NO_BIT, 0, 0, i, 0};
        if (!grid_mode) {
            pc.start_bit = uni64(recs[i].start_bit);
            pc.grid = uniu(recs[i].grid);
        }
        if ((unsigned long long)pc.grid * piece_bytes < n_comp) gz::count_piece(comp, n_comp, piece_bytes, pc, T, S); // (else: no such piece)
        else pc.state = gz::P_NO_START;
        if (S.l == 0) recs[i] = pc;
    }
}

__global__ __launch_bounds__(64) void gunzip_decode(const uint8_t *__restrict__ comp, const uint32_t n_comp, const gz::ChainPiece *__restrict__ chain, const uint32_t n,
                                                    uint16_t *sym, uint32_t *__restrict__ status)
{
    __shared__ inf::Tables T;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        gz::ChainPiece c;
        c.start_bit = uni64(chain[i].start_bit); c.end_bit = uni64(chain[i].end_bit);
        c.pos = uniu(chain[i].pos); c.n_out = uniu(chain[i].n_out); c.member_pos = uniu(chain[i].member_pos); c.member_end = uniu(chain[i].member_end);
        WaveSymSink S = wave_sink(sym + c.pos); // [pos, pos + n_out) lies inside the chain's total, which the symbol buffer holds
        const uint32_t st = gz::decode_piece(comp, n_comp, c, T, S);
        if (S.l == 0) status[i] = st;
    }
}

__global__ __launch_bounds__(RESOLVE_THREADS) void gunzip_resolve(const gz::ChainPiece *__restrict__ chain, const uint32_t n, uint16_t *sym, uint32_t *__restrict__ bad_out)
{
    __shared__ uint32_t s_bad;
    for (uint32_t k = 0; k < n; ++k) { // (n is the host's: the number of steps is fixed before the launch)
        if (threadIdx.x == 0) s_bad = 0;
        __syncthreads(); // the symbols the step in front wrote are this step's window
        if (gz::resolve_piece(sym, chain[k], threadIdx.x, RESOLVE_THREADS)) s_bad = 1;
        __syncthreads();
        if (threadIdx.x == 0) bad_out[k] = s_bad;
    }
}

__global__ __launch_bounds__(64) void gunzip_narrow(const gz::ChainPiece *__restrict__ chain, const gz::Slice *__restrict__ slices, const uint32_t n_slices,
                                                    const uint16_t *__restrict__ sym, uint8_t *text, const gz::Pow pw, gz::SliceResult *__restrict__ out)
{
    __shared__ inf::Tables T;
    WaveSymSink S = wave_sink(nullptr);
    inf::crc_init(T, S);
    for (uint32_t s = blockIdx.x; s < n_slices; s += gridDim.x) {
        const gz::Slice sl{uniu(slices[s].begin), uniu(slices[s].n), uniu(slices[s].piece), 0};
        gz::ChainPiece c;
        c.start_bit = c.end_bit = 0;
        c.pos = uniu(chain[sl.piece].pos); c.n_out = uniu(chain[sl.piece].n_out);
        c.member_pos = uniu(chain[sl.piece].member_pos); c.member_end = uniu(chain[sl.piece].member_end);
        uint32_t bad = gz::narrow_slice(sym, text, sl, c, S.l, 64);
        S.own_stores_visible();
        uint32_t crc = inf::crc_slice(T, text + sl.begin, sl.n, S.l);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { crc ^= (uint32_t)__shfl_xor((int)crc, d); bad |= (uint32_t)__shfl_xor((int)bad, d); }
        if (S.l == 0) out[s] = gz::SliceResult{inf::multmodp(gz::x8n_modp(pw, (uint64_t)c.member_end - (sl.begin + sl.n)), crc), bad};
    }
}

inline uint32_t wave_blocks(uint32_t n, int n_cu)
{
    const uint32_t cap = (uint32_t)(n_cu > 0 ? n_cu : 256) * BLOCKS_PER_CU;
    return n < cap ? n : cap;
}

} // namespace

hipError_t faqcs_launch_gunzip_count(const uint8_t *comp, uint32_t n_comp, uint32_t piece_bytes, void *recs, uint32_t n, int grid_mode, int n_cu, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(gunzip_count, dim3(wave_blocks(n, n_cu)), dim3(64), 0, st, comp, n_comp, piece_bytes, (gz::Piece *)recs, n, grid_mode);
    return hipGetLastError();
}

hipError_t faqcs_launch_gunzip_decode(const uint8_t *comp, uint32_t n_comp, const void *chain, uint32_t n, uint16_t *sym, uint32_t *status, int n_cu, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(gunzip_decode, dim3(wave_blocks(n, n_cu)), dim3(64), 0, st, comp, n_comp, (const gz::ChainPiece *)chain, n, sym, status);
    return hipGetLastError();
}

hipError_t faqcs_launch_gunzip_resolve(const void *chain, uint32_t n, uint16_t *sym, uint32_t *bad, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(gunzip_resolve, dim3(1), dim3(RESOLVE_THREADS), 0, st, (const gz::ChainPiece *)chain, n, sym, bad);
    return hipGetLastError();
}

hipError_t faqcs_launch_gunzip_narrow(const void *chain, const void *slices, uint32_t n_slices, const uint16_t *sym, uint8_t *text, void *results, int n_cu, hipStream_t st)
{
    gz::Pow pw;
    gz::pow_init(pw);
    if (n_slices) hipLaunchKernelGGL(gunzip_narrow, dim3(wave_blocks(n_slices, n_cu)), dim3(64), 0, st, (const gz::ChainPiece *)chain, (const gz::Slice *)slices, n_slices,
                                     sym, text, pw, (gz::SliceResult *)results);
    return hipGetLastError();
}
