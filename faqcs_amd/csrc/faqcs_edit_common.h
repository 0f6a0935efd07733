// faqcs_edit_common.h -- what the two kernels that write reads back out share (faqcs_emit_kernel.hip: packed arenas, faqcs_render_kernel.hip:
// FASTQ text): the block scan of their three-phase prefix sums, the wave-wide scan of a read's terminal 'N' runs, the byte masks of a
// 16-byte piece and the byte edits of faqcs_apply_edits() on a dword.
#pragma once
#include "faqcs_dev.h"

namespace faqcs_edit {

struct __attribute__((packed, aligned(1))) U128u { uint32_t w[4]; };

template <class T> __device__ __forceinline__ T wave_incl_scan(T v)
{
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// exclusive prefix of (a, b) over the threads of a block of NT threads, and the block's totals; s_a / s_b: NT / 64 entries each
template <class TA, int NT> __device__ __forceinline__ void block_excl_scan2(TA a, uint32_t b, TA *s_a, uint32_t *s_b, TA &pre_a, uint32_t &pre_b, TA &tot_a, uint32_t &tot_b)
{
    constexpr int NW = NT / 64;
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const TA ia = wave_incl_scan(a);
    const uint32_t ib = wave_incl_scan(b);
    __syncthreads(); // (the arrays may still be read from the previous call)
    if (lane == 63) { s_a[w] = ia; s_b[w] = ib; }
    __syncthreads();
    TA wa = 0, ta = 0;
    uint32_t wb = 0, tb = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const TA xa = s_a[k];
        const uint32_t xb = s_b[k];
        if (k < w) { wa += xa; wb += xb; }
        ta += xa; tb += xb;
    }
    pre_a = wa + ia - a; pre_b = wb + ib - b;
    tot_a = ta; tot_b = tb;
}

// [lead, trail) of a read [a, b) whose first (bit 0) / last (bit 1) base is 'N': the positions that keep their quality.  Whole wave, uniform arguments.
__device__ __forceinline__ void wave_terminal_extents(const uint8_t *__restrict__ seq, uint32_t a, uint32_t b, uint32_t bits, uint32_t &lead, uint32_t &trail)
{
    const uint32_t lane = threadIdx.x & 63u, L = b - a;
    lead = 0; trail = L;
    if (bits & 1u) {
        lead = L;
        for (uint32_t p = 0; p < L; p += 64) {
            const uint32_t x = p + lane;
            const bool stop = x >= L || seq[(size_t)a + x] != 'N';
            const unsigned long long m = __ballot(stop);
            if (m) { lead = p + (uint32_t)__builtin_ctzll(m); break; }
        }
    }
    if (bits & 2u) {
        trail = 0;
        for (uint32_t p = 0; p < L; p += 64) { // x: distance from the read's last base
            const uint32_t x = p + lane;
            const bool stop = x >= L || seq[(size_t)b - 1 - x] != 'N';
            const unsigned long long m = __ballot(stop);
            if (m) { trail = L - (p + (uint32_t)__builtin_ctzll(m)); break; }
        }
    }
}

// bytes [lo, hi) of a 16-byte piece that lie in its dword j, as a mask of 0xff bytes
__device__ __forceinline__ uint32_t byte_range_mask(int lo, int hi, int j)
{
    int a = lo - 4 * j, b = hi - 4 * j;
    a = a < 0 ? 0 : (a > 4 ? 4 : a);
    b = b < 0 ? 0 : (b > 4 ? 4 : b);
    if (b <= a) return 0u;
    const uint32_t mb = b == 4 ? 0xffffffffu : ((1u << (8 * b)) - 1u);
    const uint32_t ma = (1u << (8 * a)) - 1u; // a < 4 here
    return mb & ~ma;
}

// faqcs_apply_edits() on the four bytes of a dword pair (quality already masked)
__device__ __forceinline__ void edit_dword(uint32_t &s, uint32_t &q, int in, int out, int replace_q)
{
    uint32_t so = 0, qo = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        uint32_t b = (s >> (8 * t)) & 0xffu;
        const int raw = (int)(int8_t)((q >> (8 * t)) & 0xffu);
        int qs = raw - in;
        qs = qs < 0 ? 0 : qs;
        if (replace_q > 0 && b == 'G' && qs < replace_q) b = 'N';
        const uint32_t qb = in != out ? (uint32_t)(qs + out) & 0xffu : (uint32_t)raw & 0xffu;
        so |= b << (8 * t);
        qo |= qb << (8 * t);
    }
    s = so; q = qo;
}

// the quality dword j of a piece with the terminal-'N' positions of its read set to the input offset: piece bytes [keep_lo, keep_hi) keep theirs
__device__ __forceinline__ uint32_t mask_terminal_quality(uint32_t q, int keep_lo, int keep_hi, int j, uint32_t in4)
{
    const uint32_t km = byte_range_mask(keep_lo, keep_hi, j);
    return (q & km) | (in4 & ~km);
}

} // namespace faqcs_edit
