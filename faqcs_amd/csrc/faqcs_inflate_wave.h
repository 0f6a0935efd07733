// faqcs_inflate_wave.h -- one wave as the Sink of faqcs_inflate.h's decoder, for faqcs_inflate_kernel.hip (bytes) and
// faqcs_gunzip_kernel.hip (16-bit symbols).  Device code only.
#pragma once
#include "faqcs_dev.h"
#include "faqcs_inflate.h"

// Literals wait one per lane -- output o in lane o mod 64 -- and leave together when the 64 outputs' window is full or a copy needs them
// in memory.  A copy reads outputs that are all in memory before it starts (output i of a match comes from o - dist + i mod dist < o), or,
// for symbols, stand in front of output 0 and become markers; so it is one load and one store per lane and 64 outputs, with no wait
// inside it; the wave reads back its own stores behind a fence of wavefront scope.
template <class Sym> struct WaveSink { // Sym: uint8_t, or uint16_t with markers
    Sym *out;
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
            if (a >= lo && a < hi) out[a] = (Sym)mine;
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
        Sym v[5];
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) { // (len <= 258)
            const uint32_t i = l + 64 * k;
            if (i < len) {
                const uint32_t x = dist >= len ? i : i % dist, j = o + x; // the source is output j - dist
                if constexpr (sizeof(Sym) == 2) v[k] = j < dist ? (Sym)(0x8000u | (faqcs_inflate::MAX_DIST + j - dist)) : out[j - dist]; // (dist <= MAX_DIST)
                else v[k] = (out + o - dist)[x];                                                                                         // (dist <= o)
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

template <class Sym> __device__ __forceinline__ WaveSink<Sym> wave_sink(Sym *out)
{
    WaveSink<Sym> S;
    S.out = out; S.l = threadIdx.x; S.lo = S.hi = 0; S.mine = 0;
    return S;
}
