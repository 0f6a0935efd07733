// faqcs_gunzip_kernel.hip -- faqcs_gunzip_device: ordinary gzip in HBM to the FASTQ text faqcs_parse_device takes (include/faqcs_mi.h,
// DESIGN.md section 4.8).  The scheme and every function that decides something are faqcs_gunzip.h, the text the host statement and the
// sanitizer build compile too; the chain is walked on the host (gunzip_run, from faqcs_capi_seam.hip).  The wave that executes the shared
// text is WaveSink<uint16_t> of faqcs_inflate_wave.h, the Sink of faqcs_inflate_device with 16-bit symbols; this file holds the four
// kernels of a call:
//
//   gunzip_count      ONE WAVE PER PIECE: the probe (64 positions a step, the lowest that passes decides) and the run that counts; in
//                     grid mode piece i is grid piece i, else the pieces are the records the host sent (a forced start).  No output but
//                     the 32-byte record
//   gunzip_decode     ONE WAVE PER CHAIN PIECE: the run again, into 16-bit symbols at the piece's position; the window of a match is the
//                     symbol buffer itself behind a fence of wavefront scope, what lies in front of the piece is a marker
//   gunzip_resolve    ONE BLOCK over the chain in order: the markers in the last 32 768 symbols of each piece, one barrier per piece
//   gunzip_narrow     one wave per slice of 16 KiB: symbols to bytes, the slice's CRC-32 carried to its member's end
// and, for faqcs_gunzip_stream_device, the two that move the carried window:
//   gunzip_window_load   in front of the decode pass: the caller's window into the front of the symbols, as bytes
//   gunzip_window_save   behind the narrow pass: the last 32 768 bytes of (that front ++ the open member's text of this call) into the window
// No global atomic anywhere and vector stores only: every word has one writer.
#include "faqcs_gunzip.h"
#include "faqcs_inflate_wave.h"
#include "faqcs_pack_common.h"

namespace gz = faqcs_gunzip;
namespace inf = faqcs_inflate;

namespace {

constexpr uint32_t BLOCKS_PER_CU = 24; // 5.4 KB of LDS each
constexpr uint32_t RESOLVE_THREADS = 1024;

__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uniu((uint32_t)v) | (uint64_t)uniu((uint32_t)(v >> 32)) << 32; }

__global__ __launch_bounds__(64) void gunzip_count(const uint8_t *__restrict__ comp, const uint32_t n_comp, const uint32_t piece_bytes, gz::Piece *__restrict__ recs,
                                                   const uint32_t n, const int grid_mode)
{
    __shared__ inf::Tables T;
    WaveSink<uint16_t> S = wave_sink<uint16_t>(nullptr);
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
        WaveSink<uint16_t> S = wave_sink(sym + c.pos); // [pos, pos + n_out) lies inside the chain's total, which the symbol buffer holds
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
                                                    const uint16_t *__restrict__ sym, uint8_t *text, const uint32_t front, const gz::Pow pw,
                                                    gz::SliceResult *__restrict__ out)
{
    __shared__ inf::Tables T;
    WaveSink<uint16_t> S = wave_sink<uint16_t>(nullptr);
    inf::crc_init(T, S);
    for (uint32_t s = blockIdx.x; s < n_slices; s += gridDim.x) {
        const gz::Slice sl{uniu(slices[s].begin), uniu(slices[s].n), uniu(slices[s].piece), 0};
        gz::ChainPiece c;
        c.start_bit = c.end_bit = 0;
        c.pos = uniu(chain[sl.piece].pos); c.n_out = uniu(chain[sl.piece].n_out);
        c.member_pos = uniu(chain[sl.piece].member_pos); c.member_end = uniu(chain[sl.piece].member_end);
        uint32_t bad = gz::narrow_slice(sym, text, sl, c, front, S.l, 64);
        S.own_stores_visible();
        uint32_t crc = inf::crc_slice(T, text + (sl.begin - front), sl.n, S.l);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { crc ^= (uint32_t)__shfl_xor((int)crc, d); bad |= (uint32_t)__shfl_xor((int)bad, d); }
        if (S.l == 0) out[s] = gz::SliceResult{inf::multmodp(inf::x8n_modp(pw.x2n, (uint64_t)c.member_end - (sl.begin + sl.n)), crc), bad};
    }
}

constexpr uint32_t WINDOW_THREADS = 256, WINDOW_BLOCKS = gz::WIN / 16 / WINDOW_THREADS;

// two bytes -> two symbols; eight symbols -> eight bytes
__device__ __forceinline__ uint32_t widen2(uint32_t h) { return (h & 0xffu) | (h & 0xff00u) << 8; }
__device__ __forceinline__ uint32_t narrow4(uint32_t a, uint32_t b) { return (a & 0xffu) | (a >> 8 & 0xff00u) | (b & 0xffu) << 16 | (b >> 8 & 0xff00u) << 16; }

// faqcs_gunzip_stream_device, in front of the decode pass: the carried window's valid bytes into the front of the symbols,
// sym[i] = window[i] for i in [WIN - n, WIN).  A thread has the 16 bytes at a multiple of 16 of i, whose 32 bytes of symbols are aligned:
// one 16-byte load where `window` is aligned so and the group is whole, two 16-byte stores; the group that lo cuts goes byte by byte.
__global__ __launch_bounds__(WINDOW_THREADS) void gunzip_window_load(const uint8_t *__restrict__ window, const uint32_t n, uint16_t *__restrict__ sym)
{
    const uint32_t lo = gz::WIN - n;
    const bool aligned = ((uintptr_t)window & 15u) == 0;
    for (uint32_t i = (lo & ~15u) + 16 * (blockIdx.x * WINDOW_THREADS + threadIdx.x); i < gz::WIN; i += 16 * gridDim.x * WINDOW_THREADS) {
        if (i >= lo && aligned) {
            const uint4 v = *(const uint4 *)(window + i);
            *(uint4 *)(sym + i) = make_uint4(widen2(v.x), widen2(v.x >> 16), widen2(v.y), widen2(v.y >> 16));
            *(uint4 *)(sym + i + 8) = make_uint4(widen2(v.z), widen2(v.z >> 16), widen2(v.w), widen2(v.w >> 16));
        } else
            for (uint32_t j = 0; j < 16; ++j)
                if (i + j >= lo) sym[i + j] = window[i + j];
    }
}

// Behind the narrow pass: the new window, right-aligned -- window[WIN - take_old - take_new .. WIN) = the last take_old symbols of the
// front (bytes, and no pass writes there: `window` itself is never read, so a call that adds less than WIN shifts it without a hazard),
// then text[text_end - take_new .. text_end).  A thread has the 16 bytes of `window` at a multiple of 16 of their ADDRESS: one writer per
// byte, a 16-byte store for a whole group, 16-byte loads where the group lies in one source and that source is aligned.
__global__ __launch_bounds__(WINDOW_THREADS) void gunzip_window_save(const uint16_t *__restrict__ sym, const uint8_t *__restrict__ text, const uint32_t take_old,
                                                                     const uint32_t take_new, const uint32_t text_end, uint8_t *__restrict__ window)
{
    const int32_t lo = (int32_t)(gz::WIN - take_old - take_new), skew = (int32_t)((uintptr_t)window & 15u);
    const uint16_t *old_at = sym + (gz::WIN - take_old);    // symbol k of the new window, k < take_old
    const uint8_t *new_at = text + (text_end - take_new);   // byte k - take_old of it, k >= take_old
    for (int32_t i = ((lo + skew) & ~15) - skew + 16 * (int32_t)(blockIdx.x * WINDOW_THREADS + threadIdx.x); i < (int32_t)gz::WIN; i += 16 * (int32_t)(gridDim.x * WINDOW_THREADS)) {
        const int32_t k = i - lo; // of the new window; the group is [k, k + 16)
        const bool whole = k >= 0 && i + 16 <= (int32_t)gz::WIN;
        if (whole && k >= (int32_t)take_old && ((uintptr_t)(new_at + (k - (int32_t)take_old)) & 15u) == 0) {
            *(uint4 *)(window + i) = *(const uint4 *)(new_at + (k - (int32_t)take_old));
        } else if (whole && k + 16 <= (int32_t)take_old && ((uintptr_t)(old_at + k) & 15u) == 0) {
            const uint4 a = *(const uint4 *)(old_at + k), b = *(const uint4 *)(old_at + k + 8);
            *(uint4 *)(window + i) = make_uint4(narrow4(a.x, a.y), narrow4(a.z, a.w), narrow4(b.x, b.y), narrow4(b.z, b.w));
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int32_t j = 0; j < 16; ++j) {
                const int32_t q = k + j;
                if (q >= 0 && i + j < (int32_t)gz::WIN) w[j >> 2] |= (uint32_t)(q < (int32_t)take_old ? (uint8_t)old_at[q] : new_at[q - (int32_t)take_old]) << (8 * (j & 3));
            }
            if (whole) *(uint4 *)(window + i) = make_uint4(w[0], w[1], w[2], w[3]);
            else
                for (int32_t j = 0; j < 16; ++j)
                    if (k + j >= 0 && i + j < (int32_t)gz::WIN) window[i + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
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

hipError_t faqcs_launch_gunzip_window_load(const uint8_t *window, uint32_t window_bytes, uint16_t *sym, hipStream_t st)
{
    if (window_bytes) hipLaunchKernelGGL(gunzip_window_load, dim3(WINDOW_BLOCKS), dim3(WINDOW_THREADS), 0, st, window, window_bytes, sym);
    return hipGetLastError();
}

hipError_t faqcs_launch_gunzip_window_save(const uint16_t *sym, const uint8_t *text, uint32_t take_old, uint32_t take_new, uint32_t text_end, uint8_t *window, hipStream_t st)
{
    if (take_old + take_new) hipLaunchKernelGGL(gunzip_window_save, dim3(WINDOW_BLOCKS), dim3(WINDOW_THREADS), 0, st, sym, text, take_old, take_new, text_end, window);
    return hipGetLastError();
}

hipError_t faqcs_launch_gunzip_narrow(const void *chain, const void *slices, uint32_t n_slices, const uint16_t *sym, uint8_t *text, uint32_t front, void *results, int n_cu,
                                      hipStream_t st)
{
    gz::Pow pw;
    inf::x2n_fill(pw.x2n, 36);
    if (n_slices) hipLaunchKernelGGL(gunzip_narrow, dim3(wave_blocks(n_slices, n_cu)), dim3(64), 0, st, (const gz::ChainPiece *)chain, (const gz::Slice *)slices, n_slices,
                                     sym, text, front, pw, (gz::SliceResult *)results);
    return hipGetLastError();
}
