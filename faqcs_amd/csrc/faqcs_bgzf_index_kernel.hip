// faqcs_bgzf_index_kernel.hip -- faqcs_bgzf_index_device: where the BGZF members of compressed bytes in HBM are (include/faqcs_mi.h,
// DESIGN.md section 4.8).  The host statement (faqcs_inflate::bgzf_index) follows the BSIZE chain from byte 0, one header after the other.
// Here every position is asked the walk's own question -- faqcs_inflate::bgzf_index_at, the text the host walk compiles -- and the chain
// is then followed by all candidates at once:
//
//   index_count      a tile of INDEX_TILE positions per block pass: unaligned 16-byte loads, the four header bytes 1f 8b 08 xx(FEXTRA)
//                    tested on every byte position of the registers; the few positions that pass are asked bgzf_index_at().  A position
//                    where it says AT_MEMBER is a CANDIDATE: the walk would go on from it, if it ever came there.  The tile's count.
//   scan_tile_sums   (faqcs_pack_common.h) one block: the candidates in front of every tile, their number C
//   index_compact    the same test again; the candidates in position order: pos[i], bsize[i]; rank[i] = NONE, but 0 for a candidate at byte 0
//   index_link       jump[i] = the candidate at pos[i] + bsize[i] + 1 (binary search among the candidates of that position's tile), or C: none
//   index_jump       round k = 0 .. R - 1: a candidate of rank r < 2^k gives its 2^k-th successor the rank r + 2^k; jump[i] = jump[jump[i]].
//                    rank is the member's index: what the chain from byte 0 never lands on keeps NONE, whatever its bytes look like.
//   index_finish     the one ranked candidate without a successor is the last member: what stands behind it (bgzf_index_at once more, with
//                    the `avail` the host walk has there) decides consumed and error; n_members = its rank + 1, overflow
//   index_write      member_offset[rank + 1] = the member's end, unless overflow
//
// BOUNDS.  A candidate's successor lies at least MIN_MEMBER bytes behind it (bgzf_index_at returns AT_MEMBER only with ms >= MIN_MEMBER):
// the successor graph has no cycle, the chain from byte 0 holds at most n / MIN_MEMBER members, and R = the bit length of n / MIN_MEMBER
// rounds rank all of them (ranks below 2^(k + 1) are known behind round k).  R is fixed by n on the host: no loop here waits for data to
// say that it is done.  Every other loop runs over tiles, candidates (C <= n / 3 + 1: a header starts 1f 8b 08, so two candidates are 3
// bytes apart or more) or the halves of a search interval.  The serial part is the R launches: logarithmic in n, whatever the members.
// No global atomic: a rank word is written once in the whole call, by the one candidate whose 2^k-th successor it is in the one round
// with 2^k <= rank < 2^(k + 1), and a reader of the same round that sees the new value takes it for what it is, not yet below 2^k.
// Nothing outside comp[0 .. n) is read: the last bytes are loaded one by one.
#include "faqcs_inflate.h"
#include "faqcs_pack_common.h"

using namespace faqcs_pack;
namespace inf = faqcs_inflate;

namespace {

constexpr uint32_t INDEX_THREADS = 256, INDEX_VPT = 4, INDEX_VEC = 16, INDEX_TILE = INDEX_THREADS * INDEX_VPT * INDEX_VEC; // 16 384 positions
constexpr uint32_t NONE = 0xffffffffu;

struct ScanHead { unsigned long long n_bytes; uint32_t n_reads, overflow; }; // n_reads: C, the number of candidates

static_assert(offsetof(faqcs_bgzf_index_info, consumed) == 0 && offsetof(faqcs_bgzf_index_info, n_members) == 8 && offsetof(faqcs_bgzf_index_info, overflow) == 12 &&
              offsetof(faqcs_bgzf_index_info, error) == 16 && sizeof(faqcs_bgzf_index_info) == 24, "faqcs_bgzf_index_info is {consumed, n_members, overflow, error, reserved}");

struct Scratch {
    TileSum *tiles; TilePrefix *prefix; ScanHead *head; uint32_t *offs;
    uint32_t *pos, *jump[2], *rank; uint16_t *bsize;
    size_t bytes;
};
inline uint32_t tile_count(unsigned long long n) { return (uint32_t)((n + INDEX_TILE - 1) / INDEX_TILE); }
inline Scratch carve(void *base, unsigned long long n)
{
    const size_t nt = tile_count(n), cmax = (size_t)(n / 3) + 2; // candidates are 3 bytes apart or more; one entry more for the node `none`
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    Scratch s;
    uint8_t *p = (uint8_t *)base;
    s.tiles = (TileSum *)p; p += up((nt + 1) * sizeof(TileSum));
    s.prefix = (TilePrefix *)p; p += up((nt + 1) * sizeof(TilePrefix));
    s.head = (ScanHead *)p; p += up(sizeof(ScanHead));
    s.offs = (uint32_t *)p; p += 16;
    s.pos = (uint32_t *)p; p += up(cmax * sizeof(uint32_t));
    s.jump[0] = (uint32_t *)p; p += up(cmax * sizeof(uint32_t));
    s.jump[1] = (uint32_t *)p; p += up(cmax * sizeof(uint32_t));
    s.rank = (uint32_t *)p; p += up(cmax * sizeof(uint32_t));
    s.bsize = (uint16_t *)p; p += up(cmax * sizeof(uint16_t));
    s.bytes = (size_t)(p - (uint8_t *)base);
    return s;
}

struct __attribute__((packed, aligned(1))) U32u { uint32_t w; };

// Bit b: the walk would take a member at position p0 + b (b < 16; p0 < n).  The 19 bytes the four-byte test of 16 positions needs are two
// loads where they all exist, single bytes (0 behind the data: no header byte is 0 in all four places) in the last 19 bytes.
__device__ __forceinline__ uint32_t member_bits(const uint8_t *__restrict__ comp, const unsigned long long n, const unsigned long long p0)
{
    uint32_t w[5];
    if (p0 + 20 <= n) {
        const U128u v = *reinterpret_cast<const U128u *>(comp + p0);
        w[0] = v.w[0]; w[1] = v.w[1]; w[2] = v.w[2]; w[3] = v.w[3];
        w[4] = reinterpret_cast<const U32u *>(comp + p0 + 16)->w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 5; ++j) {
            w[j] = 0;
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t)
                if (p0 + 4 * j + t < n) w[j] |= (uint32_t)comp[p0 + 4 * j + t] << (8 * t);
        }
    }
    uint32_t hits = 0;
#pragma unroll
    for (uint32_t b = 0; b < INDEX_VEC; ++b) {
        const uint32_t x = b & 3u ? __builtin_amdgcn_alignbyte(w[b / 4 + 1], w[b / 4], b & 3u) : w[b / 4]; // bytes p0 + b .. p0 + b + 3
        if ((x & 0x04ffffffu) == 0x04088b1fu) hits |= 1u << b;
    }
    uint32_t bits = 0;
    while (hits) { // (at most 16 turns)
        const uint32_t b = (uint32_t)__builtin_ctz(hits);
        hits &= hits - 1;
        uint32_t ms;
        if (inf::bgzf_index_at(comp, n, p0 + b, ms) == inf::AT_MEMBER) bits |= 1u << b;
    }
    return bits;
}

// The candidates of tile t, in the order of their positions: vector j * INDEX_THREADS + thread, then the bit.  bits[j]: this thread's; at[j]:
// how many candidates of the tile stand in front of them; returns the tile's count.  Whole block.
__device__ __forceinline__ uint32_t tile_candidates(const uint8_t *__restrict__ comp, const unsigned long long n, const uint32_t t, unsigned long long *s_scan,
                                                    uint32_t (&bits)[INDEX_VPT], uint32_t (&at)[INDEX_VPT])
{
    unsigned long long packed = 0; // 16 bits per j: a pass of the block holds 256 x 16 positions, at most 1 366 candidates
#pragma unroll
    for (uint32_t j = 0; j < INDEX_VPT; ++j) {
        const unsigned long long p0 = (unsigned long long)t * INDEX_TILE + (unsigned long long)(j * INDEX_THREADS + threadIdx.x) * INDEX_VEC;
        bits[j] = p0 < n ? member_bits(comp, n, p0) : 0u;
        packed |= (unsigned long long)__builtin_popcount(bits[j]) << (16 * j);
    }
    unsigned long long pre, tot;
    block_excl_scan<unsigned long long, (int)INDEX_THREADS>(packed, s_scan, pre, tot);
    uint32_t front = 0;
#pragma unroll
    for (uint32_t j = 0; j < INDEX_VPT; ++j) {
        at[j] = front + (uint32_t)(pre >> (16 * j) & 0xffffu);
        front += (uint32_t)(tot >> (16 * j) & 0xffffu);
    }
    return front;
}

__global__ __launch_bounds__(INDEX_THREADS) void index_count(const uint8_t *__restrict__ comp, const unsigned long long n, const uint32_t n_tiles, TileSum *__restrict__ tiles)
{
    __shared__ unsigned long long s_scan[INDEX_THREADS / 64];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t bits[INDEX_VPT], at[INDEX_VPT];
        const uint32_t c = tile_candidates(comp, n, t, s_scan, bits, at);
        if (threadIdx.x == 0) tiles[t] = TileSum{c, c, 0};
    }
}

__global__ __launch_bounds__(INDEX_THREADS) void index_compact(const uint8_t *__restrict__ comp, const unsigned long long n, const uint32_t n_tiles,
                                                               const TilePrefix *__restrict__ prefix, uint32_t *__restrict__ pos, uint16_t *__restrict__ bsize,
                                                               uint32_t *__restrict__ rank)
{
    __shared__ unsigned long long s_scan[INDEX_THREADS / 64];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t bits[INDEX_VPT], at[INDEX_VPT];
        (void)tile_candidates(comp, n, t, s_scan, bits, at);
        const uint32_t first = prefix[t].recs;
#pragma unroll
        for (uint32_t j = 0; j < INDEX_VPT; ++j) {
            const unsigned long long p0 = (unsigned long long)t * INDEX_TILE + (unsigned long long)(j * INDEX_THREADS + threadIdx.x) * INDEX_VEC;
            uint32_t m = bits[j], i = first + at[j];
            while (m) { // (at most 16 turns)
                const unsigned long long p = p0 + (uint32_t)__builtin_ctz(m);
                m &= m - 1;
                pos[i] = (uint32_t)p;
                bsize[i] = (uint16_t)(inf::bgzf_member_size(comp + p, n - p) - 1u); // (a candidate: MIN_MEMBER <= BSIZE + 1 <= n - p)
                rank[i] = p ? NONE : 0u; // the chain starts at byte 0
                ++i;
            }
        }
    }
}

// the candidate at position e, or C.  The candidates of a tile are pos[prefix[tile] .. prefix[tile + 1]): the interval is halved, 13 turns at most
__device__ __forceinline__ uint32_t find_candidate(const unsigned long long e, const unsigned long long n, const uint32_t n_tiles, const TilePrefix *__restrict__ prefix,
                                                   const uint32_t *__restrict__ pos, const uint32_t C)
{
    if (e >= n) return C;
    const uint32_t t = (uint32_t)(e / INDEX_TILE);
    uint32_t lo = prefix[t].recs, hi = t + 1 < n_tiles ? prefix[t + 1].recs : C;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t v = pos[mid];
        if (v == (uint32_t)e) return mid;
        if (v < (uint32_t)e) lo = mid + 1; else hi = mid;
    }
    return C;
}

__global__ __launch_bounds__(INDEX_THREADS) void index_link(const unsigned long long n, const uint32_t n_tiles, const TilePrefix *__restrict__ prefix, const ScanHead *__restrict__ head,
                                                            const uint32_t *__restrict__ pos, const uint16_t *__restrict__ bsize, uint32_t *__restrict__ jump)
{
    const uint32_t C = head->n_reads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * INDEX_THREADS + threadIdx.x; i <= C; i += (unsigned long long)gridDim.x * INDEX_THREADS)
        jump[i] = i < C ? find_candidate((unsigned long long)pos[i] + bsize[i] + 1u, n, n_tiles, prefix, pos, C) : C; // (node C, `none`, points to itself)
}

// Round k.  Behind it, rank is known wherever it is below 2^(k + 1), and out[i] is the 2^(k + 1)-th successor of i.
__global__ __launch_bounds__(INDEX_THREADS) void index_jump(const ScanHead *__restrict__ head, const uint32_t k, const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                            uint32_t *rank)
{
    const uint32_t C = head->n_reads, step = 1u << k;
    if (step >= C) return; // no member has a rank of 2^k or more: this round and all behind it have nothing to say
    for (unsigned long long i = (unsigned long long)blockIdx.x * INDEX_THREADS + threadIdx.x; i <= C; i += (unsigned long long)gridDim.x * INDEX_THREADS) {
        const uint32_t t = in[i];
        if (i < C && t < C) {
            const uint32_t r = rank[i];
            if (r < step) rank[t] = r + step; // (NONE, and a rank that this very round has written, are not below 2^k)
        }
        out[i] = in[t];
    }
}

__global__ __launch_bounds__(INDEX_THREADS) void index_finish(const uint8_t *__restrict__ comp, const unsigned long long n, const int final, const uint32_t capacity, const uint32_t n_tiles,
                                                              const TilePrefix *__restrict__ prefix, const ScanHead *__restrict__ head, const uint32_t *__restrict__ pos,
                                                              const uint16_t *__restrict__ bsize, const uint32_t *__restrict__ rank, faqcs_bgzf_index_info *__restrict__ info)
{
    const uint32_t C = head->n_reads;
    const unsigned long long g = (unsigned long long)blockIdx.x * INDEX_THREADS + threadIdx.x;
    unsigned long long e = 0; // where the walk stops
    uint32_t k = NONE;        // and how many members it has taken: exactly one thread of the grid finds out
    if (!C || pos[0]) {
        if (g == 0) k = 0; // byte 0 is no member's
    } else {
        for (unsigned long long i = g; i < C; i += (unsigned long long)gridDim.x * INDEX_THREADS) {
            const uint32_t r = rank[i];
            if (r == NONE) continue;
            const unsigned long long end = (unsigned long long)pos[i] + bsize[i] + 1u;
            if (find_candidate(end, n, n_tiles, prefix, pos, C) == C) { e = end; k = r + 1u; } // the last member
        }
    }
    if (k == NONE) return;
    uint32_t ms;
    uint64_t consumed;
    int32_t error;
    inf::bgzf_index_stop(inf::bgzf_index_at(comp, n, e, ms), n, e, final, consumed, error);
    info->consumed = consumed;
    info->n_members = k;
    info->overflow = k > capacity ? 1u : 0u;
    info->error = error;
    info->reserved = 0;
}

__global__ __launch_bounds__(INDEX_THREADS) void index_write(const ScanHead *__restrict__ head, const uint32_t *__restrict__ pos, const uint16_t *__restrict__ bsize,
                                                             const uint32_t *__restrict__ rank, const faqcs_bgzf_index_info *__restrict__ info, uint32_t *__restrict__ member_offset)
{
    if (info->overflow) return;
    const uint32_t C = head->n_reads;
    const unsigned long long g = (unsigned long long)blockIdx.x * INDEX_THREADS + threadIdx.x;
    if (g == 0) member_offset[0] = 0;
    for (unsigned long long i = g; i < C; i += (unsigned long long)gridDim.x * INDEX_THREADS) {
        const uint32_t r = rank[i];
        if (r != NONE) member_offset[(size_t)r + 1] = pos[i] + bsize[i] + 1u; // (r + 1 <= n_members <= capacity_members)
    }
}

inline unsigned grid_for(unsigned long long items, int n_cu)
{
    const unsigned long long blocks = (items + INDEX_THREADS - 1) / INDEX_THREADS, cap = (unsigned long long)(n_cu > 0 ? n_cu : 256) * 8;
    return (unsigned)(blocks < cap ? (blocks ? blocks : 1) : cap);
}

} // namespace

size_t faqcs_bgzf_index_scratch_bytes(unsigned long long n_comp) { return carve(nullptr, n_comp).bytes; }

// every position's test, and the candidates in position order
hipError_t faqcs_launch_bgzf_index_candidates(const uint8_t *comp, unsigned long long n, void *scratch, int n_cu, hipStream_t st)
{
    const Scratch s = carve(scratch, n);
    const uint32_t nt = tile_count(n);
    const unsigned grid = grid_for((unsigned long long)nt * INDEX_THREADS, n_cu);
    if (nt) hipLaunchKernelGGL(index_count, dim3(grid), dim3(INDEX_THREADS), 0, st, comp, n, nt, s.tiles);
    hipLaunchKernelGGL(scan_tile_sums<ScanHead>, dim3(1), dim3(SCAN_THREADS), 0, st, s.tiles, nt, s.prefix, ~0ull, s.head, s.offs, (uint32_t *)nullptr);
    if (nt) hipLaunchKernelGGL(index_compact, dim3(grid), dim3(INDEX_THREADS), 0, st, comp, n, nt, s.prefix, s.pos, s.bsize, s.rank);
    return hipGetLastError();
}

// the chain from byte 0 over the candidates, info and the offsets
hipError_t faqcs_launch_bgzf_index_chain(const uint8_t *comp, unsigned long long n, int final, uint32_t *member_offset, uint32_t capacity, faqcs_bgzf_index_info *info,
                                         void *scratch, int n_cu, hipStream_t st)
{
    const Scratch s = carve(scratch, n);
    const uint32_t nt = tile_count(n);
    const unsigned grid = grid_for(n / 3 + 2, n_cu);
    hipLaunchKernelGGL(index_link, dim3(grid), dim3(INDEX_THREADS), 0, st, n, nt, s.prefix, s.head, s.pos, s.bsize, s.jump[0]);
    uint32_t rounds = 0; // the bit length of the most members the chain can hold
    for (unsigned long long m = n / inf::MIN_MEMBER; m; m >>= 1) ++rounds;
    for (uint32_t k = 0; k < rounds; ++k)
        hipLaunchKernelGGL(index_jump, dim3(grid), dim3(INDEX_THREADS), 0, st, s.head, k, s.jump[k & 1u], s.jump[~k & 1u], s.rank);
    hipLaunchKernelGGL(index_finish, dim3(grid), dim3(INDEX_THREADS), 0, st, comp, n, final ? 1 : 0, capacity, nt, s.prefix, s.head, s.pos, s.bsize, s.rank, info);
    hipLaunchKernelGGL(index_write, dim3(grid), dim3(INDEX_THREADS), 0, st, s.head, s.pos, s.bsize, s.rank, info, member_offset);
    return hipGetLastError();
}
