// faqcs_deflate_kernel.hip -- faqcs_deflate_device: FASTQ text in HBM to BGZF members (include/faqcs_mi.h).  The
// encoder itself is faqcs_deflate.h, the text the host statement and the sanitizer build compile too; this file holds the block that
// executes it and the kernels around it:
//
//   deflate_encode    ONE BLOCK PER MEMBER, members strided over the grid: the member's text, its image and every table in LDS (156 KB: one
//                     block of 1 024 threads per compute unit); the tokens wait in 4 bytes per position of the block's own scratch; the
//                     member leaves for its worst-case slot as 16-byte pieces, its size for sizes[].  Two instantiations, the fast and the
//                     dense match finder (FAQCS_DEFLATE_FAST / FAQCS_DEFLATE_DENSE); the launch picks by mode, everything behind it is shared
//   deflate_sizes     one thread per member: block scan of the sizes, a tile sum per block
//   scan_tile_sums    (faqcs_pack_common.h) one block: tile prefixes, the total, the overflow decision
//   deflate_gather    one wave per member: slot -> comp at the member's position, whole 16-byte pieces between its unaligned ends;
//                     member_offset
//   deflate_finish    one block: n_stored
// No global atomic anywhere, and nothing depends on which block takes which member.
#include "faqcs_deflate.h"
#include "faqcs_pack_common.h"
#include "faqcs_trim_common.h"

using namespace faqcs_pack;
namespace def = faqcs_deflate;

namespace {

constexpr uint32_t SCAN_TILE = 256;
constexpr uint32_t FINISH_THREADS = 1024;
constexpr uint32_t GATHER_WAVES = 4;

// the leading 16 bytes of faqcs_deflate_info under the field names scan_tile_sums asserts
struct ScanHead { unsigned long long n_bytes; uint32_t n_reads, overflow; };
static_assert(offsetof(faqcs_deflate_info, n_bytes) == 0 && offsetof(faqcs_deflate_info, n_members) == 8 && offsetof(faqcs_deflate_info, overflow) == 12 &&
              offsetof(faqcs_deflate_info, n_stored) == 16 && sizeof(faqcs_deflate_info) == 24, "faqcs_deflate_info leads with {n_bytes, n_members, overflow}, n_stored behind them");
static_assert(sizeof(def::Work) + 256 <= 160 * 1024, "the member's workspace and the scan's words fit the LDS of a compute unit");

struct Scratch {
    TileSum *tiles; TilePrefix *prefix; uint32_t *sizes, *pos, *tok; uint8_t *slots;
    size_t bytes;
};
// n: members (the EOF member included), n_data: members with text, blocks: the encode grid
inline Scratch carve(void *base, uint32_t n, uint32_t n_data, uint32_t member_bytes, uint32_t blocks)
{
    const size_t nt = ((size_t)n + SCAN_TILE - 1) / SCAN_TILE;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    Scratch s;
    uint8_t *p = (uint8_t *)base;
    s.tiles = (TileSum *)p; p += up((nt + 1) * sizeof(TileSum));
    s.prefix = (TilePrefix *)p; p += up((nt + 1) * sizeof(TilePrefix));
    s.sizes = (uint32_t *)p; p += up(((size_t)n + 1) * sizeof(uint32_t));
    s.pos = (uint32_t *)p; p += up(((size_t)n + 1) * sizeof(uint32_t));
    s.tok = (uint32_t *)p; p += up((size_t)blocks * ((member_bytes + def::TILE - 1) / def::TILE * def::TILE) * sizeof(uint32_t));
    s.slots = p; p += (size_t)n_data * def::slot_bytes(member_bytes);
    s.bytes = (size_t)(p - (uint8_t *)base);
    return s;
}

// One block as the encoder's executor.
struct BlockExec {
    uint32_t *s_scan;
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
    __device__ __forceinline__ uint32_t lanes() const { return def::TILE; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return uniu(v); }
    __device__ __forceinline__ void amax(uint32_t *p, uint32_t v) { atomicMax(p, v); }
    // a max on half a word: compare-and-swap on the word that holds it, until the half is v at least (whatever the order, the largest stays)
    __device__ __forceinline__ void amax16(uint16_t *a, uint32_t i, uint32_t v)
    {
        uint32_t *w = reinterpret_cast<uint32_t *>(a) + (i >> 1);
        const uint32_t sh = 16u * (i & 1u);
        uint32_t old = *w;
        while (((old >> sh) & 0xffffu) < v) {
            const uint32_t seen = atomicCAS(w, old, (old & ~(0xffffu << sh)) | v << sh);
            if (seen == old) break;
            old = seen;
        }
    }
    __device__ __forceinline__ void aadd(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
    __device__ __forceinline__ void aor(uint32_t *p, uint32_t v) { atomicOr(p, v); }
    __device__ __forceinline__ void axor(uint32_t *p, uint32_t v) { atomicXor(p, v); }
    __device__ __forceinline__ uint32_t excl_scan(uint32_t *a)
    {
        uint32_t pre, tot;
        const uint32_t v = a[threadIdx.x];
        block_excl_scan<uint32_t, (int)def::TILE>(v, s_scan, pre, tot);
        a[threadIdx.x] = pre; // (read back by this lane only)
        return tot;
    }
    __device__ __forceinline__ void store16(uint8_t *dst, const uint32_t *src) { *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src); }
};

template <int MODE>
__global__ __launch_bounds__(def::TILE) void deflate_encode(const uint8_t *__restrict__ text, const unsigned long long n_text, const uint32_t member_bytes, const uint32_t n_data,
                                                            uint32_t *__restrict__ tok, uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ uint32_t s_scan[def::TILE / 64];
    def::Work &W = *reinterpret_cast<def::Work *>(smem);
    BlockExec X{s_scan};
    const uint32_t slot = def::slot_bytes(member_bytes), tok_words = (member_bytes + def::TILE - 1) / def::TILE * def::TILE;
    for (uint32_t m = blockIdx.x; m < n_data; m += gridDim.x) {
        const unsigned long long a = (unsigned long long)m * member_bytes;
        const uint32_t n = (uint32_t)(n_text - a < member_bytes ? n_text - a : member_bytes); // (>= 1: m < n_data)
        const uint32_t r = def::deflate_member<MODE>(X, W, text + a, n, tok + (size_t)blockIdx.x * tok_words, slots + (size_t)m * slot);
        if (threadIdx.x == 0) sizes[m] = r;
    }
}

__global__ __launch_bounds__(SCAN_TILE) void deflate_sizes(uint32_t *__restrict__ sizes, const uint32_t n, const uint32_t n_data, uint32_t *__restrict__ pos, TileSum *__restrict__ tiles)
{
    __shared__ uint32_t s_a[SCAN_TILE / 64];
    const uint32_t first = blockIdx.x * SCAN_TILE, i = first + threadIdx.x;
    uint32_t sz = 0;
    if (i < n) {
        if (i >= n_data) sizes[i] = def::EOF_BYTES; // the EOF member
        sz = sizes[i] & 0x7fffffffu;
    }
    uint32_t pre, tot;
    block_excl_scan<uint32_t, (int)SCAN_TILE>(sz, s_a, pre, tot);
    if (i < n) pos[i + 1] = pre + sz;
    if (threadIdx.x == 0) tiles[blockIdx.x] = TileSum{tot, n - first < SCAN_TILE ? n - first : SCAN_TILE, 0};
}

// member m: comp[a .. e) = its slot.  The bytes in front of the first 16-byte boundary of comp and behind the last leave one by one, the
// pieces between them as 16 bytes from wherever they lie in the slot.
__global__ __launch_bounds__(GATHER_WAVES * 64) void deflate_gather(const uint8_t *__restrict__ slots, const uint32_t slot, const uint32_t *__restrict__ sizes, const uint32_t *__restrict__ pos,
                                                                    const TilePrefix *__restrict__ prefix, const uint32_t n, const uint32_t n_data, uint8_t *__restrict__ comp,
                                                                    uint32_t *__restrict__ member_offset, const faqcs_deflate_info *__restrict__ info)
{
    if (info->overflow) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * GATHER_WAVES;
    for (uint32_t m = blockIdx.x * GATHER_WAVES + uniu(threadIdx.x >> 6); m < n; m += n_waves) {
        const uint32_t e = uniu(pos[m + 1] + (uint32_t)prefix[m / SCAN_TILE].bytes), size = uniu(sizes[m] & 0x7fffffffu), a = e - size;
        if (member_offset && lane == 0) member_offset[m + 1] = e;
        if (m >= n_data) { // the EOF member
            if (lane < def::EOF_BYTES) comp[a + lane] = (uint8_t)def::eof_byte(lane);
            continue;
        }
        const uint8_t *src = slots + (size_t)m * slot;
        const uint32_t a16 = umin_(e, (a + 15u) & ~15u), e16 = a16 + ((e - a16) & ~15u);
        if (a + lane < a16) comp[a + lane] = src[lane];
        for (uint32_t o = a16 + 16u * lane; o < e16; o += 16u * 64u)
            *reinterpret_cast<U128u *>(comp + o) = *reinterpret_cast<const U128u *>(src + (o - a));
        if (e16 + lane < e) comp[e16 + lane] = src[e16 - a + lane];
    }
}

__global__ __launch_bounds__(FINISH_THREADS) void deflate_finish(const uint32_t *__restrict__ sizes, const uint32_t n_data, faqcs_deflate_info *__restrict__ info)
{
    __shared__ uint32_t s_n[FINISH_THREADS / 64];
    uint32_t c = 0;
    for (uint32_t i = threadIdx.x; i < n_data; i += FINISH_THREADS) c += sizes[i] >> 31;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) c += (uint32_t)__shfl_xor((int)c, d);
    if ((threadIdx.x & 63u) == 0) s_n[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        c = 0;
        for (uint32_t w = 0; w < FINISH_THREADS / 64; ++w) c += s_n[w];
        info->n_stored = c;
        info->reserved = 0;
    }
}

unsigned long long g_lds_done[2] = {0, 0}; // (by mode)

inline uint32_t encode_blocks(uint32_t n_data, int n_cu) { const uint32_t cap = (uint32_t)(n_cu > 0 ? n_cu : 256); return n_data < cap ? (n_data ? n_data : 1u) : cap; }

} // namespace

size_t faqcs_deflate_scratch_bytes(uint32_t n, uint32_t n_data, uint32_t member_bytes, int n_cu) { return carve(nullptr, n, n_data, member_bytes, encode_blocks(n_data, n_cu)).bytes; }

hipError_t faqcs_launch_deflate_encode(const uint8_t *text, unsigned long long n_text, uint32_t member_bytes, uint32_t n, uint32_t n_data, int mode, void *scratch, int n_cu, hipStream_t st)
{
    const uint32_t blocks = encode_blocks(n_data, n_cu);
    const Scratch s = carve(scratch, n, n_data, member_bytes, blocks);
    if (!n_data) return hipSuccess;
    auto *kernel = mode == def::MODE_DENSE ? deflate_encode<def::MODE_DENSE> : deflate_encode<def::MODE_FAST>;
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), sizeof(def::Work), g_lds_done[mode == def::MODE_DENSE]);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(def::TILE), sizeof(def::Work), st, text, n_text, member_bytes, n_data, s.tok, s.slots, s.sizes);
    return hipGetLastError();
}

hipError_t faqcs_launch_deflate_gather(uint32_t member_bytes, uint32_t n, uint32_t n_data, const faqcs_deflate_out *out, void *scratch, int n_cu, hipStream_t st)
{
    const Scratch s = carve(scratch, n, n_data, member_bytes, encode_blocks(n_data, n_cu));
    const uint32_t nt = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (n) hipLaunchKernelGGL(deflate_sizes, dim3(nt), dim3(SCAN_TILE), 0, st, s.sizes, n, n_data, s.pos, s.tiles);
    hipLaunchKernelGGL(scan_tile_sums<ScanHead>, dim3(1), dim3(SCAN_THREADS), 0, st, s.tiles, nt, s.prefix, (unsigned long long)out->capacity_bytes,
                       reinterpret_cast<ScanHead *>(out->info), s.pos, out->member_offset);
    hipLaunchKernelGGL(deflate_finish, dim3(1), dim3(FINISH_THREADS), 0, st, s.sizes, n_data, out->info);
    if (n) {
        const uint32_t cap = (uint32_t)(n_cu > 0 ? n_cu : 256) * 8, want = (n + GATHER_WAVES - 1) / GATHER_WAVES;
        hipLaunchKernelGGL(deflate_gather, dim3(want < cap ? want : cap), dim3(GATHER_WAVES * 64), 0, st, s.slots, def::slot_bytes(member_bytes), s.sizes, s.pos, s.prefix, n, n_data,
                           out->comp, out->member_offset, out->info);
    }
    return hipGetLastError();
}
