// faqcs_inflate_kernel.hip -- faqcs_inflate_device: BGZF members in HBM to the FASTQ text faqcs_parse_device takes (include/faqcs_mi.h,
// DESIGN.md section 4.8).  The decoder itself is faqcs_inflate.h, the text the host statement and the sanitizer build compile too, and
// the wave that executes it is WaveSink<uint8_t> of faqcs_inflate_wave.h; this file holds the kernels around them:
//
//   inflate_scan      one thread per member: header and trailer, the header rules, ISIZE; block scan of ISIZE, a tile sum per block
//   scan_tile_sums    (faqcs_pack_common.h) one block: tile prefixes, the total, the overflow decision
//   inflate_apply     one thread per member: its output position
//   inflate_decode    ONE WAVE PER MEMBER: blocks of one wave claim members by a strided loop; tables in LDS, built by the lanes over the
//                     symbols; the bit buffer is the same in every lane (scalar registers), a table look-up is one LDS address; literals
//                     collect one per lane and leave as one store per 64 bytes; a match is one load and one store per lane; the window is
//                     the output buffer itself; the CRC runs in the tail, a slice per lane
//   inflate_finish    one block: the first bad member in input order completes info
// No global atomic anywhere: every member's wave writes its own status word.
#include "faqcs_inflate_wave.h"
#include "faqcs_pack_common.h"

using namespace faqcs_pack;
namespace inf = faqcs_inflate;

namespace {

constexpr uint32_t SCAN_TILE = 256;    // members of an inflate_scan block
constexpr uint32_t FINISH_THREADS = 1024;
constexpr uint32_t DECODE_BLOCKS_PER_CU = 24; // 5.4 KB of LDS each

// the leading 16 bytes of faqcs_inflate_info under the field names scan_tile_sums asserts
struct ScanHead { unsigned long long n_bytes; uint32_t n_reads, overflow; };
static_assert(offsetof(faqcs_inflate_info, n_bytes) == 0 && offsetof(faqcs_inflate_info, n_members) == 8 && offsetof(faqcs_inflate_info, overflow) == 12 &&
              offsetof(faqcs_inflate_info, error) == 16 && sizeof(faqcs_inflate_info) == 24, "faqcs_inflate_info leads with {n_bytes, n_members, overflow}, error behind them");

struct Scratch {
    TileSum *tiles; TilePrefix *prefix; uint4 *hdr; uint32_t *pos, *status;
    size_t bytes;
};
inline Scratch carve(void *base, uint32_t n)
{
    const size_t nt = ((size_t)n + SCAN_TILE - 1) / SCAN_TILE;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    Scratch s;
    uint8_t *p = (uint8_t *)base;
    s.tiles = (TileSum *)p; p += up((nt + 1) * sizeof(TileSum));
    s.prefix = (TilePrefix *)p; p += up((nt + 1) * sizeof(TilePrefix));
    s.hdr = (uint4 *)p; p += up(((size_t)n + 1) * sizeof(uint4));
    s.pos = (uint32_t *)p; p += up(((size_t)n + 1) * sizeof(uint32_t));
    s.status = (uint32_t *)p; p += up(((size_t)n + 1) * sizeof(uint32_t));
    s.bytes = (size_t)(p - (uint8_t *)base);
    return s;
}

__global__ __launch_bounds__(SCAN_TILE) void inflate_scan(const uint8_t *__restrict__ comp, const unsigned long long n_comp, const uint32_t *__restrict__ moff, const uint32_t n,
                                                          uint4 *__restrict__ hdr, uint32_t *__restrict__ status, uint32_t *__restrict__ pos, TileSum *__restrict__ tiles)
{
    __shared__ uint32_t s_a[SCAN_TILE / 64];
    const uint32_t first = blockIdx.x * SCAN_TILE, i = first + threadIdx.x;
    uint32_t isz = 0;
    if (i < n) {
        const uint32_t a = moff[i], e = moff[i + 1];
        inf::Member m{0, 0, 0, 0};
        int st = inf::ST_E_HEADER;
        if (e > a && e <= n_comp) st = inf::parse_member(comp + a, e - a, m); // (reads inside comp[a .. e) only)
        hdr[i] = make_uint4(m.data_begin, m.data_end, m.crc, m.isize);
        status[i] = (uint32_t)st;
        isz = st ? 0u : m.isize;
    }
    uint32_t pre, tot;
    block_excl_scan<uint32_t, (int)SCAN_TILE>(isz, s_a, pre, tot); // (256 x 65 536 = 2^24)
    if (i < n) pos[i + 1] = pre + isz;
    if (threadIdx.x == 0) tiles[blockIdx.x] = TileSum{tot, n - first < SCAN_TILE ? n - first : SCAN_TILE, 0};
}

__global__ __launch_bounds__(SCAN_TILE) void inflate_apply(const TilePrefix *__restrict__ prefix, const uint32_t n, uint32_t *__restrict__ pos,
                                                           uint32_t *__restrict__ member_text_offset, const faqcs_inflate_info *__restrict__ info)
{
    const uint32_t i = blockIdx.x * SCAN_TILE + threadIdx.x;
    if (i >= n || info->overflow) return;
    const uint32_t p = pos[i + 1] + (uint32_t)prefix[blockIdx.x].bytes;
    pos[i + 1] = p;
    if (member_text_offset) member_text_offset[i + 1] = p;
}

__global__ __launch_bounds__(64) void inflate_decode(const uint8_t *__restrict__ comp, const uint32_t *__restrict__ moff, const uint32_t n, const uint4 *__restrict__ hdr,
                                                     const uint32_t *__restrict__ pos, uint32_t *__restrict__ status, uint8_t *text, const faqcs_inflate_info *__restrict__ info)
{
    __shared__ inf::Tables T;
    if (info->overflow) return;
    WaveSink<uint8_t> S = wave_sink(text);
    inf::crc_init(T, S);
    for (uint32_t m = blockIdx.x; m < n; m += gridDim.x) {
        if (uniu(status[m])) continue; // the scan refused its header
        const uint4 h = hdr[m];
        const uint32_t begin = uniu(h.x), end = uniu(h.y), crc_want = uniu(h.z), isize = uniu(h.w);
        S.out = text + uniu(pos[m]); // [pos, pos + isize) lies inside the scanned total, which fits the capacity
        S.lo = S.hi = 0;
        int st = inf::inflate_member(comp + uniu(moff[m]), begin, end, isize, T, S);
        if (!st) {
            S.own_stores_visible();
            uint32_t c = inf::crc_slice(T, S.out, isize, S.l);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) c ^= (uint32_t)__shfl_xor((int)c, d);
            if (uniu(c) != crc_want) st = inf::ST_E_CRC;
        }
        if (st && S.l == 0) status[m] = (uint32_t)st;
    }
}

__global__ __launch_bounds__(FINISH_THREADS) void inflate_finish(const uint32_t *__restrict__ status, const uint32_t *__restrict__ pos, const uint32_t n, faqcs_inflate_info *__restrict__ info)
{
    __shared__ uint32_t s_min[FINISH_THREADS / 64];
    uint32_t best = 0xffffffffu;
    if (!info->overflow)
        for (uint32_t i = threadIdx.x; i < n; i += FINISH_THREADS)
            if (status[i]) { best = i; break; }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) best = umin_(best, (uint32_t)__shfl_xor((int)best, d));
    if ((threadIdx.x & 63u) == 0) s_min[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 0; w < FINISH_THREADS / 64; ++w) best = umin_(best, s_min[w]);
        int32_t err = inf::ST_OK;
        if (best != 0xffffffffu) {
            info->n_bytes = pos[best];
            info->n_members = best;
            err = (int32_t)status[best];
        }
        info->error = err;
        info->reserved = 0;
    }
}

} // namespace

size_t faqcs_inflate_scratch_bytes(uint32_t n_members) { return carve(nullptr, n_members).bytes; }

// the scan: every member's header, its position, the total and the overflow decision
hipError_t faqcs_launch_inflate_scan(const uint8_t *comp, unsigned long long n_comp, const uint32_t *moff, uint32_t n, const faqcs_inflate_out *out, void *scratch, hipStream_t st)
{
    const Scratch s = carve(scratch, n);
    const uint32_t nt = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (n) hipLaunchKernelGGL(inflate_scan, dim3(nt), dim3(SCAN_TILE), 0, st, comp, n_comp, moff, n, s.hdr, s.status, s.pos, s.tiles);
    hipLaunchKernelGGL(scan_tile_sums<ScanHead>, dim3(1), dim3(SCAN_THREADS), 0, st, s.tiles, nt, s.prefix, (unsigned long long)out->capacity_bytes,
                       reinterpret_cast<ScanHead *>(out->info), s.pos, out->member_text_offset);
    if (n) hipLaunchKernelGGL(inflate_apply, dim3(nt), dim3(SCAN_TILE), 0, st, s.prefix, n, s.pos, out->member_text_offset, out->info);
    return hipGetLastError();
}

hipError_t faqcs_launch_inflate_decode(const uint8_t *comp, const uint32_t *moff, uint32_t n, const faqcs_inflate_out *out, void *scratch, int n_cu, hipStream_t st)
{
    const Scratch s = carve(scratch, n);
    const uint32_t cap = (uint32_t)(n_cu > 0 ? n_cu : 256) * DECODE_BLOCKS_PER_CU;
    if (n) hipLaunchKernelGGL(inflate_decode, dim3(n < cap ? n : cap), dim3(64), 0, st, comp, moff, n, s.hdr, s.pos, s.status, out->text, out->info);
    hipLaunchKernelGGL(inflate_finish, dim3(1), dim3(FINISH_THREADS), 0, st, s.status, s.pos, n, out->info);
    return hipGetLastError();
}
