// faqcs_detect_kernel.hip -- the decisions the reference's driver takes AROUND trim(), on the device (include/faqcs_mi.h at faqcs_detect_device;
// DESIGN.md section 4.11): the quality-offset auto-detect (trim.cpp:599-617), the NextSeq look at the first defline (trim.cpp:619-626) and the
// read at which trim() threw (the FAQCS_F_ERR_* bits).  All three are one question: the FIRST element of a contiguous device range for
// which a predicate holds.
//
// One find-first core (find_first_tiles) serves both entry points.  The range is a run of UNITS -- quality bytes, or 8-byte results -- that
// is cut into 16-byte VECTORS (16 bytes, or 2 results) and those into TILES of DETECT_TILE_VECS vectors (16 KB either way).  A source says
// which units of a vector satisfy the predicate, as a bit mask that is already cut to the range:
//   QualHits   one aligned 16-byte load.  A byte is decisive when, read as a signed char, it is > 74 or < 59: (byte - 59) mod 256 > 15.
//              The subtraction and the test run on whole dwords (four bytes at a time, no carry between them); the two ends of the range
//              are masked per byte.  Vectors are aligned by ADDRESS, so up to 15 bytes in front of the range and behind it are loaded
//              (the padding contract of faqcs_batch) and never interpreted.
//   ErrorHits  two 8-byte loads, each only when its result is inside the range (results have no padding); the predicate is the two error
//              bits of the flags.
// The tiles are strided over the grid.  A thread takes DETECT_VPT vectors of a tile, THREADS apart; a ballot per pass and a count of
// trailing zeros give the wave's first hit, the block's four waves meet in LDS, and the tile's partial -- the position of its first hit,
// or NONE -- goes to scratch.  A block that has found a hit writes NONE for its later tiles without loading them: they lie behind that hit.
// The finishing block (one block) takes the lowest partial over however many tiles there are, and one thread of it does what is left:
// the byte, the binary search of offset[] for the read that owns it and the three defline bytes, or the flags of the bad read.
// No atomics, and only vector stores: info is a function of the inputs alone.  This is not a throughput stage and nothing here was timed.
#include "faqcs_ctx.h"

namespace {

constexpr uint32_t DETECT_THREADS = 256, DETECT_VPT = 4, DETECT_TILE_VECS = DETECT_THREADS * DETECT_VPT; // 1 024 vectors: 16 384 bytes, 2 048 results
constexpr uint32_t FINISH_THREADS = 1024, NONE = 0xffffffffu;
constexpr unsigned long long MAX_BYTE_TILES = ((1ull << 32) / 16 + 1 + DETECT_TILE_VECS - 1) / DETECT_TILE_VECS + 1; // offsets are 32 bits wide

// one bit per byte of x that is decisive: bit t is byte t
__device__ __forceinline__ uint32_t decisive_bits(uint32_t x)
{
    const uint32_t H = 0x80808080u, K = 0x3b3b3b3bu;               // 59 in every byte
    const uint32_t d = ((x | H) - K) ^ ((x ^ ~K) & H);              // (byte - 59) mod 256, byte by byte
    const uint32_t t = d & 0xf0f0f0f0u;                             // not zero: the difference is above 15
    const uint32_t nz = (((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & H; // 0x80 in every byte of t that is not zero
    return (((nz >> 7) * 0x00204081u) >> 21) & 15u;
}

struct QualHits {
    static constexpr uint32_t UNITS = 16;
    const uint4 *base; // 16-byte aligned: unit u is byte u of it
    __device__ __forceinline__ uint32_t operator()(unsigned long long v, unsigned long long lo, unsigned long long hi) const
    {
        const uint4 x = base[v];
        uint32_t bits = decisive_bits(x.x) | decisive_bits(x.y) << 4 | decisive_bits(x.z) << 8 | decisive_bits(x.w) << 12;
        const unsigned long long u0 = v * UNITS;
        if (u0 < lo) bits &= 0xffffu << (uint32_t)(lo - u0);              // (the core asks for vectors that touch the range only: lo - u0 < 16)
        if (u0 + UNITS > hi) bits &= (1u << (uint32_t)(hi - u0)) - 1u;    // (hi - u0 in 1 .. 15)
        return bits;
    }
};

struct ErrorHits {
    static constexpr uint32_t UNITS = 2;
    const uint2 *res; // unit u is result u: .y holds flags (low half) and adapter
    __device__ __forceinline__ uint32_t operator()(unsigned long long v, unsigned long long lo, unsigned long long hi) const
    {
        const unsigned long long u0 = v * UNITS;
        uint32_t bits = 0;
        if (u0 >= lo && u0 < hi && (res[u0].y & (FAQCS_F_ERR_QUALITY | FAQCS_F_ERR_BASE))) bits |= 1u;
        if (u0 + 1 >= lo && u0 + 1 < hi && (res[u0 + 1].y & (FAQCS_F_ERR_QUALITY | FAQCS_F_ERR_BASE))) bits |= 2u;
        return bits;
    }
};

__host__ __device__ inline unsigned long long tile_count(unsigned long long lo, unsigned long long hi, uint32_t units)
{
    if (hi <= lo) return 0;
    const unsigned long long v0 = lo / units, v1 = (hi + units - 1) / units;
    return (v1 - v0 + DETECT_TILE_VECS - 1) / DETECT_TILE_VECS;
}

// partial[t] = the first unit of tile t of [lo, hi) that hits, minus bias, or NONE.  Tile t holds the vectors from lo / UNITS + t * DETECT_TILE_VECS.
template <class Src>
__device__ __forceinline__ void find_first_tiles(const Src &S, const unsigned long long lo, const unsigned long long hi, const uint32_t bias, uint32_t *__restrict__ partial)
{
    __shared__ uint32_t s_first[DETECT_THREADS / 64];
    const unsigned long long n_tiles = tile_count(lo, hi, Src::UNITS);
    if (!n_tiles) return;
    const unsigned long long v0 = lo / Src::UNITS, v1 = (hi + Src::UNITS - 1) / Src::UNITS;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    bool found = false; // (uniform over the block)
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        if (found) { // this tile lies behind a hit of this block
            if (threadIdx.x == 0) partial[t] = NONE;
            continue;
        }
        const unsigned long long vt = v0 + t * DETECT_TILE_VECS;
        uint32_t m[DETECT_VPT];
#pragma unroll
        for (uint32_t j = 0; j < DETECT_VPT; ++j) {
            const unsigned long long v = vt + j * DETECT_THREADS + threadIdx.x;
            m[j] = v < v1 ? S(v, lo, hi) : 0u;
        }
        uint32_t first = NONE; // the wave's: its vectors ascend with the lane inside a pass, and from pass to pass
#pragma unroll
        for (uint32_t j = 0; j < DETECT_VPT; ++j) {
            const unsigned long long any = __ballot(m[j] != 0u);
            if (any && first == NONE) {
                const uint32_t src = (uint32_t)__builtin_ctzll(any);
                const uint32_t mm = (uint32_t)__shfl((int)m[j], (int)src);
                const unsigned long long v = vt + j * DETECT_THREADS + (threadIdx.x - lane) + src;
                first = (uint32_t)(v * Src::UNITS + (uint32_t)__builtin_ctz(mm) - bias);
            }
        }
        if (lane == 0) s_first[w] = first;
        __syncthreads();
        uint32_t f = s_first[0];
#pragma unroll
        for (uint32_t k = 1; k < DETECT_THREADS / 64; ++k) f = f < s_first[k] ? f : s_first[k];
        __syncthreads(); // (s_first is written again in the next tile)
        if (threadIdx.x == 0) partial[t] = f;
        found = f != NONE;
    }
}

// the lowest of n_tiles partials, in every thread of the finishing block
__device__ __forceinline__ uint32_t lowest_partial(const uint32_t *__restrict__ partial, const unsigned long long n_tiles)
{
    __shared__ uint32_t s_low[FINISH_THREADS / 64];
    uint32_t low = NONE;
    for (unsigned long long t = threadIdx.x; t < n_tiles; t += FINISH_THREADS) {
        const uint32_t f = partial[t];
        low = low < f ? low : f;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)low, d);
        low = low < o ? low : o;
    }
    if ((threadIdx.x & 63u) == 0) s_low[threadIdx.x >> 6] = low;
    __syncthreads();
    low = s_low[0];
    for (uint32_t k = 1; k < FINISH_THREADS / 64; ++k) low = low < s_low[k] ? low : s_low[k];
    return low;
}

// the byte range of reads [first, first + count), in units of the aligned base: [lo, hi), and what to take off a unit to get the arena position
struct ByteRange { unsigned long long lo, hi; uint32_t mis; };
__device__ __forceinline__ ByteRange byte_range(const uint8_t *qual, const uint32_t *__restrict__ offset, uint32_t first, uint32_t count)
{
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(qual) & 15u);
    if (!count) return ByteRange{0, 0, mis}; // (offset is not looked at)
    return ByteRange{(unsigned long long)offset[first] + mis, (unsigned long long)offset[(size_t)first + count] + mis, mis};
}

__global__ __launch_bounds__(DETECT_THREADS) void detect_scan(const uint8_t *__restrict__ qual, const uint32_t *__restrict__ offset, const uint32_t first, const uint32_t count,
                                                              uint32_t *__restrict__ partial)
{
    const ByteRange r = byte_range(qual, offset, first, count);
    find_first_tiles(QualHits{reinterpret_cast<const uint4 *>(qual - r.mis)}, r.lo, r.hi, r.mis, partial);
}

__global__ __launch_bounds__(FINISH_THREADS) void detect_finish(const uint8_t *__restrict__ qual, const uint32_t *__restrict__ offset, const uint32_t first, const uint32_t count,
                                                                const uint8_t *__restrict__ text, const uint32_t *__restrict__ def_pos, const uint32_t *__restrict__ def_len,
                                                                const uint32_t *__restrict__ partial, faqcs_detect_info *__restrict__ info)
{
    const ByteRange r = byte_range(qual, offset, first, count);
    const uint32_t b = lowest_partial(partial, tile_count(r.lo, r.hi, QualHits::UNITS));
    if (threadIdx.x != 0) return;
    faqcs_detect_info d{0, first + count, 0u, 0u, 0u, 0u};
    if (b != NONE) {
        const uint32_t byte = qual[b];
        d.quality_offset = (int)(int8_t)byte > 74 ? 64 : 33; // (decisive: above 74 or below 59)
        uint32_t i = first, e = first + count;               // offset[i] <= b < offset[e]
        while (e - i > 1u) {
            const uint32_t mid = i + (e - i) / 2u;
            if (offset[mid] <= b) i = mid; else e = mid;
        }
        d.read = i; d.pos = b - offset[i]; d.byte = byte;
    }
    if (count && text && def_len[first] >= 3u) {
        const uint8_t *p = text + def_pos[first];
        d.next_seq = (p[0] == '@' && p[1] == 'N' && p[2] == 'S') ? 1u : 0u;
    }
    *info = d;
}

__global__ __launch_bounds__(DETECT_THREADS) void first_error_scan(const faqcs_read_result *__restrict__ res, const uint32_t n, uint32_t *__restrict__ partial)
{
    find_first_tiles(ErrorHits{reinterpret_cast<const uint2 *>(res)}, 0ull, (unsigned long long)n, 0u, partial);
}

__global__ __launch_bounds__(FINISH_THREADS) void first_error_finish(const faqcs_read_result *__restrict__ res, const uint32_t n, const uint32_t *__restrict__ partial,
                                                                     faqcs_error_info *__restrict__ info)
{
    const uint32_t i = lowest_partial(partial, tile_count(0ull, (unsigned long long)n, ErrorHits::UNITS));
    if (threadIdx.x != 0) return;
    faqcs_error_info e{n, 0u};
    if (i != NONE) { e.n_good = i; e.flags = reinterpret_cast<const uint2 *>(res)[i].y & (uint32_t)(FAQCS_F_ERR_QUALITY | FAQCS_F_ERR_BASE); }
    *info = e;
}

inline unsigned scan_grid(unsigned long long tiles, int n_cu)
{
    const unsigned long long cap = (unsigned long long)(n_cu > 0 ? n_cu : 256) * 4;
    return (unsigned)(tiles < cap ? tiles : cap);
}

} // namespace

// One partial per tile.  The byte form's range is known on the device only and the host does not wait for it, so its scratch is sized by
// what 32-bit offsets can span (1 MB); the result form's by n.
size_t faqcs_detect_scratch_bytes() { return (size_t)MAX_BYTE_TILES * sizeof(uint32_t); }
size_t faqcs_first_error_scratch_bytes(uint32_t n) { return (size_t)(tile_count(0, n, ErrorHits::UNITS) + 1) * sizeof(uint32_t); }

hipError_t faqcs_launch_detect(const uint8_t *qual, const uint32_t *off, uint32_t first, uint32_t count, const uint8_t *text, const uint32_t *def_pos,
                               const uint32_t *def_len, faqcs_detect_info *info, void *scratch, int n_cu, hipStream_t st)
{
    uint32_t *partial = reinterpret_cast<uint32_t *>(scratch);
    if (count) hipLaunchKernelGGL(detect_scan, dim3(scan_grid(MAX_BYTE_TILES, n_cu)), dim3(DETECT_THREADS), 0, st, qual, off, first, count, partial);
    hipLaunchKernelGGL(detect_finish, dim3(1), dim3(FINISH_THREADS), 0, st, qual, off, first, count, text, def_pos, def_len, partial, info);
    return hipGetLastError();
}

hipError_t faqcs_launch_first_error(const faqcs_read_result *res, uint32_t n, faqcs_error_info *info, void *scratch, int n_cu, hipStream_t st)
{
    uint32_t *partial = reinterpret_cast<uint32_t *>(scratch);
    const unsigned long long tiles = tile_count(0, n, ErrorHits::UNITS);
    if (tiles) hipLaunchKernelGGL(first_error_scan, dim3(scan_grid(tiles, n_cu)), dim3(DETECT_THREADS), 0, st, res, n, partial);
    hipLaunchKernelGGL(first_error_finish, dim3(1), dim3(FINISH_THREADS), 0, st, res, n, partial, info);
    return hipGetLastError();
}
