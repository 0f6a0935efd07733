// faqcs_trim_common.h -- pieces shared by the trim kernels (faqcs_trim_kernel.hip, faqcs_trim_lds_kernel.hip):
// byte / bit helpers over the LDS accumulator layout (RowCfg, faqcs_trim_plan.h), the block flush and the per-chunk epilogue.
#pragma once
#include "faqcs_dev.h"

#include <stdlib.h>

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting of a kernel: a process with contexts on several devices
// (faqcs_mi --gpus N) has to make it on each of them once.  `done` = one bit per device ordinal, owned by the caller (one per kernel).
static inline hipError_t ensure_dynamic_lds(const void *kernel, size_t bytes, unsigned long long &done)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (__atomic_load_n(&done, __ATOMIC_ACQUIRE) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) __atomic_fetch_or(&done, bit, __ATOMIC_RELEASE);
    return e;
}

namespace {

template <int D> struct __attribute__((packed, aligned(1))) PackedBytes { uint32_t w[D]; };

__device__ __forceinline__ int med3i(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// bits j in [0, C) with lo <= pbase + j < hi
template <int C> __device__ __forceinline__ uint32_t range_mask(int lo, int hi, int pbase)
{
    const int s = med3i(lo - pbase, 0, C);
    int e = med3i(hi - pbase, 0, C);
    e = e > s ? e : s;
    uint32_t m; // ((1 << (e - s)) - 1) << s in one instruction
    asm("v_bfm_b32 %0, %1, %2" : "=v"(m) : "v"(e - s), "v"(s));
    return m;
}
// 0 / -1 from bit j of mask.  Pinned to ONE v_bfe_i32: left to itself the compiler rewrites `x & -(bit)` into
// and + compare + select (3 instructions per use, ~40 uses per read in a VALU-bound kernel).
// 4 * byte K of w in ONE instruction (SDWA source select): the LDS byte offset of a base-table lookup
template <int K> __device__ __forceinline__ uint32_t byte_times4(uint32_t w, uint32_t two)
{
    uint32_t r;
    if (K == 0) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(two), "v"(w));
    else if (K == 1) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(two), "v"(w));
    else if (K == 2) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(two), "v"(w));
    else asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(two), "v"(w));
    return r;
}
// t_base_lds = LDS byte address of the table (the kernel's dynamic LDS starts at address 0, checked at kernel start): the
// lookup is then ds_read_b32 v, <4 * byte> offset:<table> with no address add at all.
typedef const __attribute__((address_space(3))) uint32_t *lds_u32_ptr;
typedef __attribute__((address_space(3))) uint32_t *lds_u32_mut;
// ds_add_u32 at an LDS BYTE offset computed in 32 bits (a generic pointer makes the compiler form the address with
// v_mad_u64_u32, a multi-pass instruction, once per base)
__device__ __forceinline__ void lds_add_u32(uint32_t byte_offset, uint32_t v)
{
    __hip_atomic_fetch_add((lds_u32_mut)(size_t)byte_offset, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// The same add as one line of assembly, for the LDS adds a wave makes WHILE ONE OF ITS LDS-DMA LOADS IS IN FLIGHT (trim_lds: the epilogue under
// the next chunk's quality DMA, the work under the base DMA).  The compiler cannot tell an LDS store or atomic from the DMA's own write to LDS and
// puts an s_waitcnt vmcnt(0) in front of the first one it sees behind a DMA, which drains the very load the work was placed under; an
// instruction inside asm it does not look at.  Nothing comes back, so there is no result to wait for; the adds of a wave reach LDS in issue
// order like every DS instruction, and the callers wait lgkmcnt(0) before a barrier hands the cells to other waves.
__device__ __forceinline__ void lds_add_u32_quiet(uint32_t byte_offset, uint32_t v)
{
    asm volatile("ds_add_u32 %0, %1" : : "v"(byte_offset), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_add_u32_quiet(uint32_t *cell, uint32_t v) { lds_add_u32_quiet((uint32_t)(size_t)(lds_u32_mut)cell, v); }
// ... with a byte offset in the instruction's offset field (16 bits; a constant after unrolling, like bit_m1's bit), for the callers that add to a
// row of cells from one address register
__device__ __forceinline__ void lds_add_u32_quiet(uint32_t byte_offset, uint32_t v, const int imm_off)
{
    asm volatile("ds_add_u32 %0, %1 offset:%2" : : "v"(byte_offset), "v"(v), "n"(imm_off) : "memory");
}
template <int C, int J> struct BaseLookup {
    static __device__ __forceinline__ void run(const uint32_t t_base_lds, const uint32_t *ws, uint32_t two, uint32_t *inc)
    {
        inc[J] = *(lds_u32_ptr)(size_t)(byte_times4<J & 3>(ws[J >> 2], two) + t_base_lds);
        BaseLookup<C, J + 1>::run(t_base_lds, ws, two, inc);
    }
};
template <int C> struct BaseLookup<C, C> {
    static __device__ __forceinline__ void run(const uint32_t, const uint32_t *, uint32_t, uint32_t *) {}
};
__device__ __forceinline__ uint32_t umax3_(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_max3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ int bit_m1(uint32_t mask, int j)
{
    int r;
    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(r) : "v"(mask), "n"(j));
    return r;
}

} // namespace

// LDS -> global u64 block.  Deliberately NOT inlined: the counter-block layout (a dozen 64-bit offsets) would
// otherwise stay live in SGPRs across the whole read loop and push the kernel into scalar-register spills.
// PAST_END: the read loop adds the "pre" 1 for every position slot of a counted read, also past its end (corrected here);
// false: the loop only counts positions inside the read (trim_lds)
template <int C, int LPR, int NW, bool PAST_END = true>
__device__ __noinline__ void flush_block(uint32_t *smem, uint64_t *counters, const uint32_t R, const int tid)
{
    using Cfg = RowCfg<C, LPR>;
    constexpr int W = Cfg::W;
    uint32_t *hq = smem + Cfg::O_HQ, *hb = smem + Cfg::O_HB, *hlen = smem + Cfg::O_LEN, *hrq = smem + Cfg::O_RQ;
    uint32_t *hbqpre = smem + Cfg::O_BQPRE, *hbqpost = smem + Cfg::O_BQPOST, *lfs = smem + Cfg::O_FS;
    // faqcs_counters_layout() restated (include/faqcs_mi.h): only R is needed for the offsets used here
    faqcs_layout L;
    {
        uint64_t o = 0;
        L.filter_stats = o;    o += 32;
        L.pre_read_qhist = o;  o += FAQCS_NQ;
        L.pre_base_qhist = o;  o += FAQCS_NQ;
        L.post_read_qhist = o; o += FAQCS_NQ;
        L.post_base_qhist = o; o += FAQCS_NQ;
        L.pre_len_hist = o;    o += (uint64_t)R + 1;
        L.post_len_hist = o;   o += (uint64_t)R + 1;
        L.pre_qual = o;        o += (uint64_t)R * FAQCS_NQ;
        L.post_qual = o;       o += (uint64_t)R * FAQCS_NQ;
        L.pre_base = o;        o += (uint64_t)R * FAQCS_NBASE;
        L.post_base = o;
    }
    __syncthreads();
    for (int i = tid; i < (Cfg::HQ8 ? 0 : Cfg::HQ); i += NW * 64) {
        const uint32_t v = hq[i];
        if (v) {
            hq[i] = 0;
            const uint32_t q = i / W, p = i % W;
            uint32_t pre = v & 0xffffu;
            if (PAST_END && q == 0) {
                // The read loop adds the "pre" 1 for EVERY position slot of a counted read, also past its end (where the
                // masked quality byte is 0): column 0 of position p is over-counted once per read with len <= p, and the
                // interval's length histogram says how many those are.
                uint32_t shorter = 0;
                for (uint32_t l = 0; l <= p; ++l) shorter += hlen[l] & 0xffffu;
                pre -= shorter;
            }
            if (p < R) {
                if (pre) atomicAdd((unsigned long long *)(counters + L.pre_qual + (uint64_t)p * FAQCS_NQ + q), (unsigned long long)pre);
                if (v >> 16) atomicAdd((unsigned long long *)(counters + L.post_qual + (uint64_t)p * FAQCS_NQ + q), (unsigned long long)(v >> 16));
            }
        }
    }
    __syncthreads(); // (the correction above reads hlen, which the loop below clears)
    for (int i = tid; i < Cfg::HB; i += NW * 64) {
        const uint32_t v = hb[i];
        if (v) {
            hb[i] = 0;
            const uint32_t c = i / W, p = i % W;
            if (p < R) {
                if (v & 0xffffu) atomicAdd((unsigned long long *)(counters + L.pre_base + (uint64_t)p * FAQCS_NBASE + c), (unsigned long long)(v & 0xffffu));
                if (v >> 16) atomicAdd((unsigned long long *)(counters + L.post_base + (uint64_t)p * FAQCS_NBASE + c), (unsigned long long)(v >> 16));
            }
        }
    }
    for (int i = tid; i <= W; i += NW * 64) {
        const uint32_t v = hlen[i];
        if (v && (uint32_t)i <= R) {
            hlen[i] = 0;
            if (v & 0xffffu) atomicAdd((unsigned long long *)(counters + L.pre_len_hist + i), (unsigned long long)(v & 0xffffu));
            if (v >> 16) atomicAdd((unsigned long long *)(counters + L.post_len_hist + i), (unsigned long long)(v >> 16));
        }
    }
    if (tid < FAQCS_NQ) {
        const uint32_t v = hrq[tid], x = hbqpre[tid], y = hbqpost[tid];
        hrq[tid] = 0; hbqpre[tid] = 0; hbqpost[tid] = 0;
        if (v & 0xffffu) atomicAdd((unsigned long long *)(counters + L.pre_read_qhist + tid), (unsigned long long)(v & 0xffffu));
        if (v >> 16) atomicAdd((unsigned long long *)(counters + L.post_read_qhist + tid), (unsigned long long)(v >> 16));
        if (x) atomicAdd((unsigned long long *)(counters + L.pre_base_qhist + tid), (unsigned long long)x);
        if (y) atomicAdd((unsigned long long *)(counters + L.post_base_qhist + tid), (unsigned long long)y);
    }
    if (tid >= 64 && tid < 64 + FAQCS_NUM_STAT) {
        const int k = tid - 64;
        const uint32_t v = lfs[k];
        if (v) { atomicAdd((unsigned long long *)(counters + L.filter_stats + k), (unsigned long long)v); lfs[k] = 0; }
    }
    __syncthreads();
}

// 8-bit packed position x quality cells (rows wider than 512) -> global u64 block; called by the whole block
template <int C, int LPR, int NW>
__device__ __noinline__ void flush_hq8(uint32_t *smem, uint64_t *counters, const uint32_t R, const int tid)
{
    using Cfg = RowCfg<C, LPR>;
    constexpr int HW = Cfg::W / 2;
    uint32_t *hq = smem + Cfg::O_HQ;
    const uint64_t pre_qual = 32 + 4 * FAQCS_NQ + 2 * ((uint64_t)R + 1), post_qual = pre_qual + (uint64_t)R * FAQCS_NQ;
    __syncthreads();
    for (int i = tid; i < Cfg::HQ; i += NW * 64) {
        const uint32_t v = hq[i];
        if (v) {
            hq[i] = 0;
            const uint32_t q = i / HW, p = 2u * (uint32_t)(i % HW);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t a = (v >> (16 * h)) & 0xffu, b = (v >> (16 * h + 8)) & 0xffu;
                if (p + h < R) {
                    if (a) atomicAdd((unsigned long long *)(counters + pre_qual + (uint64_t)(p + h) * FAQCS_NQ + q), (unsigned long long)a);
                    if (b) atomicAdd((unsigned long long *)(counters + post_qual + (uint64_t)(p + h) * FAQCS_NQ + q), (unsigned long long)b);
                }
            }
        }
    }
    __syncthreads();
}

// What depends on a read's scalars alone, done once per 64-read chunk with one read per lane: result word, composition
// records, length / average-quality histograms, FilterStat sums.
struct ReadOutcome {
    uint32_t an, fl, pAT, pCG, cAT, cCG, N; // start | kept << 16 ; flags ; base counts before / after (A|T<<16, C|G<<16, N pre | post << 16)
    int Vpre, Vpost;                       // sum(raw - offset) over the read / over the kept window
};
// FilterStat sums kept per lane over several chunks (trim_lds: folded into the block's cells every few chunks, next to the register
// spill, instead of seven wave reductions per chunk): read count << 20 | base count, at most 2^12 reads and 2^20 bases per wave
struct FsAcc { uint32_t tot = 0, trim = 0, len = 0, qt = 0; }; // (poly-N, low complexity, average quality: rare, added per chunk when they occur)
__device__ __forceinline__ void fs_acc_flush(FsAcc &f, const int lane, uint32_t *lfs)
{
    const uint32_t m = (1u << 20) - 1u;
    const uint32_t s_tot = (uint32_t)wave_sum_i32((int)f.tot), s_trim = (uint32_t)wave_sum_i32((int)f.trim), s_len = (uint32_t)wave_sum_i32((int)f.len);
    const uint32_t s_qt = (uint32_t)wave_sum_i32((int)f.qt);
    const uint32_t s_nn = 0, s_lc = 0, s_avg = 0;
    if (lane == 0) {
        if (s_tot) { lds_add_u32_quiet(&lfs[FAQCS_TOTAL_COUNT], s_tot >> 20); lds_add_u32_quiet(&lfs[FAQCS_TOTAL_NUMBER], s_tot >> 20); lds_add_u32_quiet(&lfs[FAQCS_TOTAL_LENGTH], s_tot & m); }
        if (s_trim) { lds_add_u32_quiet(&lfs[FAQCS_TOTAL_TRIMMED_NUMBER], s_trim >> 20); lds_add_u32_quiet(&lfs[FAQCS_TOTAL_TRIMMED_LENGTH], s_trim & m); }
        if (s_len) { lds_add_u32_quiet(&lfs[FAQCS_READ_LENGTH], s_len >> 20); lds_add_u32_quiet(&lfs[FAQCS_BASE_LENGTH], s_len & m); }
        if (s_nn) { lds_add_u32_quiet(&lfs[FAQCS_READ_NN], s_nn >> 20); lds_add_u32_quiet(&lfs[FAQCS_BASE_NN], s_nn & m); }
        if (s_avg) { lds_add_u32_quiet(&lfs[FAQCS_READ_AVG_Q], s_avg >> 20); lds_add_u32_quiet(&lfs[FAQCS_BASE_AVG_Q], s_avg & m); }
        if (s_qt) { lds_add_u32_quiet(&lfs[FAQCS_READ_QUAL_TRIM], s_qt >> 20); lds_add_u32_quiet(&lfs[FAQCS_BASE_QUAL_TRIM], s_qt & m); }
        if (s_lc) { lds_add_u32_quiet(&lfs[FAQCS_READ_LOW_COMPLEXITY], s_lc >> 20); lds_add_u32_quiet(&lfs[FAQCS_BASE_LOW_COMPLEXITY], s_lc & m); }
    }
    f = FsAcc();
}

// ---- (trim_lds) the six histogram adds of a chunk's epilogue, one read per lane.  64 lanes that add to ONE LDS address are serialised by the LDS
// (110-250 clocks of the CU's LDS pipe for one instruction, against 3.4-4.8 with distinct banks: DESIGN 4, the instruction table), and that is the
// common case: reads of one length, average qualities on a handful of values.  So the lanes of a wave are combined PER HISTOGRAM before they add:
//   wave_value_count   lane L's count of the lanes whose value is L (values < 64: six ballots of the value's bits, lane L keeps the lanes that
//                      agree with L in every bit): a histogram of up to 64 bins costs one add, its addresses distinct
//   peel_pairs         up to four distinct keys, two per turn: the first remaining lane's key, a ballot of the lanes that share it, one add of their
//                      count and one of their summed values by that lane; the two sums of a turn share ONE wave reduction (16-bit fields: 64 values of at most 1 023, which peel_pairs checks -- a larger value adds for itself).  Lanes left after that add for themselves.
// Every add is a quiet one (above): both halves of the epilogue run beside an LDS-DMA in flight.  Adds of zero are dropped or kept freely.
__device__ __forceinline__ uint32_t wave_value_count(const bool in, const uint32_t v, const int lane)
{
    unsigned long long b[7];
    b[6] = __builtin_amdgcn_ballot_w64(in);
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = __builtin_amdgcn_ballot_w64(in && ((v >> k) & 1u) != 0u);
    // One half of the wave after the other, one bit after the other (the empty asm pins the order): three registers at the kernel's register
    // peak.  Left to itself the compiler forms all twelve b ^ keep terms first and ORs them together: eight registers, and a spill.
    uint32_t cnt = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t m = (uint32_t)(b[6] >> (32 * h));
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            m &= ~((uint32_t)(b[k] >> (32 * h)) ^ (uint32_t)bit_m1((uint32_t)lane, k)); // (bit k of the lane number set: b, else ~b; one v_bitop3)
            asm volatile("" : "+v"(m));
        }
        cnt += (uint32_t)__popc(m);
    }
    return cnt;
}
// cnt_tab[key] += cnt_one per lane of `in`, sum_tab[key] += val (cnt_tab may be null: no counts).  Called by whole waves.
// PRECONDITION: 64 x val < 2^16 (the two sums of a turn share one register).  Its callers pass a read length of a trim_lds variant with fewer than
// 16 lanes per read (at most 152 bases; PEEL_MAX_VAL leaves room for every trim_lds length), and a value beyond the bound adds for itself.
__device__ __forceinline__ void peel_pairs(const bool in, const uint32_t key, const uint32_t val, uint32_t *cnt_tab, const uint32_t cnt_one,
                                           uint32_t *sum_tab, const int lane)
{
    constexpr uint32_t PEEL_MAX_VAL = 1023u;
    static_assert(64u * PEEL_MAX_VAL < 65536u, "two sums of 64 values share one 32-bit register");
    bool left = in && val <= PEEL_MAX_VAL;
    const bool big = in && !left;
    unsigned long long rem = __ballot(left);
#pragma unroll 1
    for (int turn = 0; turn < 2 && rem != 0ull; ++turn) {
        const int f0 = __builtin_ctzll(rem);
        const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, f0);
        const bool same0 = left && key == k0;
        const unsigned long long b0 = __ballot(same0);
        rem &= ~b0;
        const int f1 = rem != 0ull ? __builtin_ctzll(rem) : f0; // (no second key: same1 is false everywhere)
        const uint32_t k1 = (uint32_t)__builtin_amdgcn_readlane((int)key, f1);
        const bool same1 = left && !same0 && key == k1;
        const unsigned long long b1 = __ballot(same1);
        rem &= ~b1;
        const uint32_t s = (uint32_t)wave_sum_i32((int)((same0 ? val : 0u) | (same1 ? val << 16 : 0u)));
        if (lane == f0) {
            if (cnt_tab) lds_add_u32_quiet(cnt_tab + k0, (uint32_t)__popcll(b0) * cnt_one);
            lds_add_u32_quiet(sum_tab + k0, s & 0xffffu);
        }
        if (same1 && lane == f1) {
            if (cnt_tab) lds_add_u32_quiet(cnt_tab + k1, (uint32_t)__popcll(b1) * cnt_one);
            lds_add_u32_quiet(sum_tab + k1, s >> 16);
        }
        left = left && !same0 && !same1;
    }
    if (left || big) {
        if (cnt_tab) lds_add_u32_quiet(cnt_tab + key, cnt_one);
        lds_add_u32_quiet(sum_tab + key, val);
    }
}
// the length histogram: the lanes whose length is `cand` (wave-uniform: the length most of them are expected to have) in one add, the others for themselves
__device__ __forceinline__ void len_hist_add(const bool in, const uint32_t len, const uint32_t cand, const uint32_t one, uint32_t *hlen, const int lane)
{
    const bool same = in && len == cand;
    const unsigned long long b = __ballot(same);
    if (b != 0ull && lane == __builtin_ctzll(b)) lds_add_u32_quiet(hlen + cand, (uint32_t)__popcll(b) * one);
    if (in && !same) lds_add_u32_quiet(hlen + len, one);
}
#ifdef FAQCS_LDS_DIAG_EPI_NOCONFLICT // (diagnostic build, wrong results: the three adds of a lane on a cell no other lane adds to -- what the equal addresses of the epilogue's adds cost)
__device__ __forceinline__ void epi_diag_adds(const bool in, const uint32_t v, uint32_t *hrq, uint32_t *hbq, const int lane)
{
    uint32_t *c = lane < FAQCS_NQ ? hrq + lane : hbq + (lane - FAQCS_NQ);
    if (in) { lds_add_u32_quiet(c, 1u); lds_add_u32_quiet(c, 1u); lds_add_u32_quiet(c, v); }
}
#endif

// (trim_lds) The half of the deferred epilogue that depends on nothing but the read's length and its pre-trim quality sum: the pre-trim
// histogram cells and the FilterStat total.  A function of its own so that trim_lds can run it before the bases of the chunk are in LDS, while
// their DMA is in flight; chunk_epilogue calls it itself unless it is told that the caller has (pre_done).  Called by whole waves.
// The average-quality histogram is one wave_value_count (42 bins); a chunk of one length -- the common case -- adds its length once and its
// bases per quality bin as count x length from the same counts; a chunk of several lengths sums them by peel_pairs.
// COMBINE = false (the 16-lane variants: 32 or 20 reads per chunk, so the same work per chunk buys half as much or less -- 2x250 measured 41.69 -> 42.13 ms
// per step with it, profiles/lds_same_address/ab_2x250_combined.txt): the lanes that share the first lane's (length, quality bin) pair add once, the others for themselves.
template <bool COMBINE = true>
__device__ __forceinline__ void chunk_epilogue_pre(const bool mine, const bool e_err, const uint32_t e_len, const int Vpre, const int lane, uint32_t *hlen,
                                                   uint32_t *hrq, uint32_t *hbqpre, const uint32_t *t_magic, FsAcc *defer)
{
        int qb_pre = 0;
        if (mine && e_len > 0 && Vpre > 0) qb_pre = e_len == 1 ? Vpre : (int)__umulhi((uint32_t)Vpre, t_magic[e_len]);
        qb_pre = qb_pre > 41 ? 41 : qb_pre;
        const bool act = mine && !e_err;
#ifdef FAQCS_LDS_DIAG_EPI_NOCONFLICT
        epi_diag_adds(act, e_len, hrq, hbqpre, lane);
#else
        const unsigned long long actm = COMBINE ? __ballot(act) : 0ull;
        if (!COMBINE) { // (statement for statement what every variant did before per-histogram combining)
            if (act) {
                const uint32_t key = e_len | ((uint32_t)qb_pre << 16);
                const bool same = key == (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
                const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(same));
                if (same) {
                    if (lane == __ffsll((unsigned long long)__ballot(true)) - 1) {
                        lds_add_u32_quiet(hlen + e_len, cnt);
                        lds_add_u32_quiet(hrq + qb_pre, cnt);
                        if (e_len) lds_add_u32_quiet(hbqpre + qb_pre, cnt * e_len);
                    }
                } else {
                    lds_add_u32_quiet(hlen + e_len, 1u);
                    lds_add_u32_quiet(hrq + qb_pre, 1u);
                    if (e_len) lds_add_u32_quiet(hbqpre + qb_pre, e_len);
                }
            }
        } else if (actm != 0ull) { // (wave-uniform)
            const uint32_t len0 = (uint32_t)__builtin_amdgcn_readlane((int)e_len, __builtin_ctzll(actm));
            const uint32_t cnt = wave_value_count(act, (uint32_t)qb_pre, lane); // (0 in the lanes from FAQCS_NQ on: no bin has their number)
            // (bin = lane number, from a copy the compiler cannot see through: hrq + lane and hbqpre + lane would otherwise be hoisted out of the
            // chunk loop and hold two registers for the whole kernel)
            uint32_t bin = (uint32_t)lane;
            asm volatile("" : "+v"(bin));
            if (cnt) lds_add_u32_quiet(hrq + bin, cnt);
            len_hist_add(act, e_len, len0, 1u, hlen, lane);
            if (__ballot(act && e_len != len0) == 0ull) {
                if (cnt && len0) lds_add_u32_quiet(hbqpre + bin, cnt * len0);
            } else {
                peel_pairs(act && e_len != 0u, (uint32_t)qb_pre, e_len, nullptr, 0u, hbqpre, lane);
            }
        }
#endif
        const uint32_t one = 1u << 20;
        defer->tot += mine ? one | e_len : 0u;
}

template <int LPR>
__device__ __forceinline__ void chunk_epilogue(const ReadOutcome &o, const bool mine, const uint32_t my, const uint32_t v_len,
                                               const uint32_t v_hit, const int lane, uint32_t *hlen, uint32_t *hrq, uint32_t *hbqpre,
                                               uint32_t *hbqpost, uint32_t *lfs, const uint32_t *t_magic, uint2 *__restrict__ out,
                                               unsigned long long *__restrict__ rec_pre, unsigned long long *__restrict__ rec_post,
                                               const bool o_avgq_on, const uint32_t o_dbg, FsAcc *defer = nullptr, const bool wide_rt = false,
                                               const bool pre_done = false)
{
        const bool e_ret = (o.fl & FAQCS_F_VALID) != 0, e_err = (o.fl & FAQCS_F_ERR_QUALITY) != 0;
        const uint32_t e_len = v_len, e_n = o.an >> 16, e_filt = (o.fl & FAQCS_F_FILTER_MASK) >> FAQCS_F_FILTER_SHIFT;
        // int(ave_Q) == max(0, floor(V / len)), V = sum(raw - offset); floor via mulhi with a host magic
        int qb_pre = 0, qb_post = 0;
        if (!defer && mine && e_len > 0 && o.Vpre > 0) qb_pre = e_len == 1 ? o.Vpre : (int)__umulhi((uint32_t)o.Vpre, t_magic[e_len]);
        if (e_ret && o.Vpost > 0) qb_post = e_n == 1 ? o.Vpost : (int)__umulhi((uint32_t)o.Vpost, t_magic[e_n]);
        qb_pre = qb_pre > 41 ? 41 : qb_pre;
        qb_post = qb_post > 41 ? 41 : qb_post;
        if (defer) {
            // (trim_lds) the same six histogram cells, the lanes of the wave combined per histogram: the pre-trim three in chunk_epilogue_pre, here the post-trim three
            if (!pre_done) chunk_epilogue_pre<(LPR < 16)>(mine, e_err, e_len, o.Vpre, lane, hlen, hrq, hbqpre, t_magic, defer);
            // post-trim: the average quality sits on two or three values (peel_pairs: the read count and the summed kept lengths of each), the kept
            // length is spread except for the reads that keep every base (len_hist_add with the chunk's first length)
            const bool pact = mine && !e_err && e_ret;
#ifdef FAQCS_LDS_DIAG_EPI_NOCONFLICT
            epi_diag_adds(pact, e_n, hrq, hbqpost, lane);
#else
            const unsigned long long pm = LPR < 16 ? __ballot(pact) : 0ull;
            if (LPR >= 16) { // (as chunk_epilogue_pre<false>)
                if (pact) {
                    const uint32_t key = e_n | ((uint32_t)qb_post << 16);
                    const bool same = key == (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
                    const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(same));
                    if (same) {
                        if (lane == __ffsll((unsigned long long)__ballot(true)) - 1) {
                            lds_add_u32_quiet(hlen + e_n, cnt << 16);
                            lds_add_u32_quiet(hrq + qb_post, cnt << 16);
                            lds_add_u32_quiet(hbqpost + qb_post, cnt * e_n);
                        }
                    } else {
                        lds_add_u32_quiet(hlen + e_n, 0x10000u);
                        lds_add_u32_quiet(hrq + qb_post, 0x10000u);
                        lds_add_u32_quiet(hbqpost + qb_post, e_n);
                    }
                }
            } else if (pm != 0ull) { // (wave-uniform)
                peel_pairs(pact, (uint32_t)qb_post, e_n, hrq, 0x10000u, hbqpost, lane);
                len_hist_add(pact, e_n, (uint32_t)__builtin_amdgcn_readlane((int)e_len, __builtin_ctzll(pm)), 0x10000u, hlen, lane);
            }
#endif
        } else if (!(o_dbg & 2u) && mine && !e_err) { // length and int(average quality) histograms (trim.cpp:254-258,539-543,877-885)
            atomicAdd(hlen + e_len, 1u);
            atomicAdd(hrq + qb_pre, 1u);
            if (e_len) atomicAdd(hbqpre + qb_pre, e_len);
            if (e_ret) {
                atomicAdd(hlen + e_n, 0x10000u);
                atomicAdd(hrq + qb_post, 0x10000u);
                atomicAdd(hbqpost + qb_post, e_n);
            }
        }
        if (mine) {
            const bool bad_base = v_hit == 0xffffu; // set by adapter_overlap
            out[my] = make_uint2(e_ret ? o.an : 0u, (o.fl & 0x3ffu) | (bad_base ? (uint32_t)FAQCS_F_ERR_BASE : (v_hit << 16)));
            const bool pre_on = !e_err, post_on = e_ret && !e_err;
            const unsigned long long pA = o.pAT & 0xffffu, pT = o.pAT >> 16, pC = o.pCG & 0xffffu, pG = o.pCG >> 16, pn = o.N & 0xffffu;
            const unsigned long long cA = o.cAT & 0xffffu, cT = o.cAT >> 16, cC = o.cCG & 0xffffu, cG = o.cCG >> 16, cn = o.N >> 16;
            if (LPR <= 16 && !wide_rt) { // (wide_rt, wave-uniform: a 16-lane kernel whose batch holds a read of more than 256 bases)
                rec_pre[my] = pre_on ? (CR_VALID | e_len | (pA << 9) | (pT << 18) | (pC << 27) | (pG << 36) | (pn << 45)) : 0ull;
                rec_post[my] = post_on ? (CR_VALID | e_n | (cA << 9) | (cT << 18) | (cC << 27) | (cG << 36) | (cn << 45)) : 0ull;
            } else { // reads past 511 bases do not fit 9-bit fields: 11-bit fields over two words
                reinterpret_cast<ulonglong2 *>(rec_pre)[my] =
                    pre_on ? make_ulonglong2(CR_VALID | e_len | (pA << 11) | (pT << 22) | (pC << 33), pG | (pn << 11)) : make_ulonglong2(0ull, 0ull);
                reinterpret_cast<ulonglong2 *>(rec_post)[my] =
                    post_on ? make_ulonglong2(CR_VALID | e_n | (cA << 11) | (cT << 22) | (cC << 33), cG | (cn << 11)) : make_ulonglong2(0ull, 0ull);
            }
        }
        // FilterStat (trim.cpp:238-240,317-323,325-387,505-513,527-531): a read count in the high and a base
        // count in the low 20 bits, summed over the 64 reads of the chunk (64 x 1024 bases < 2^20)
        const bool e_rlen = e_filt == FAQCS_FILT_LENGTH_PRE || e_filt == FAQCS_FILT_LENGTH_POST;
        const uint32_t one = 1u << 20;
        if (defer) { // (a compile-time choice: the pointer is a constant of the inlined call)
            defer->trim += e_ret ? one | e_n : 0u; // (->tot: chunk_epilogue_pre)
            defer->len += e_rlen ? one | e_n : 0u;
            defer->qt += (o.fl & FAQCS_F_QUAL_TRIMMED) ? one | (o.fl >> 20) : 0u;
            // the rare ones at once (a wave reduction only in a chunk that has such a read)
            const uint32_t m = one - 1u;
            const bool is_nn = (o.fl & FAQCS_F_POLY_N_SEEN) != 0, is_lc = e_filt == FAQCS_FILT_LOW_COMPLEXITY, is_avg = o_avgq_on && e_filt == FAQCS_FILT_AVG_Q;
            if (__any(is_nn)) { const uint32_t v = (uint32_t)wave_sum_i32((int)(is_nn ? one | e_n : 0u)); if (lane == 0) { lds_add_u32_quiet(&lfs[FAQCS_READ_NN], v >> 20); lds_add_u32_quiet(&lfs[FAQCS_BASE_NN], v & m); } }
            if (__any(is_lc)) { const uint32_t v = (uint32_t)wave_sum_i32((int)(is_lc ? one | e_n : 0u)); if (lane == 0) { lds_add_u32_quiet(&lfs[FAQCS_READ_LOW_COMPLEXITY], v >> 20); lds_add_u32_quiet(&lfs[FAQCS_BASE_LOW_COMPLEXITY], v & m); } }
            if (__any(is_avg)) { const uint32_t v = (uint32_t)wave_sum_i32((int)(is_avg ? one | e_n : 0u)); if (lane == 0) { lds_add_u32_quiet(&lfs[FAQCS_READ_AVG_Q], v >> 20); lds_add_u32_quiet(&lfs[FAQCS_BASE_AVG_Q], v & m); } }
            return;
        }
        const uint32_t s_tot = (uint32_t)wave_sum_i32((int)(mine ? one | e_len : 0u));
        const uint32_t s_trim = (uint32_t)wave_sum_i32((int)(e_ret ? one | e_n : 0u));
        const uint32_t s_len = (uint32_t)wave_sum_i32((int)(e_rlen ? one | e_n : 0u));
        const uint32_t s_nn = (uint32_t)wave_sum_i32((int)((o.fl & FAQCS_F_POLY_N_SEEN) ? one | e_n : 0u));
        const uint32_t s_qt = (uint32_t)wave_sum_i32((int)((o.fl & FAQCS_F_QUAL_TRIMMED) ? one | (o.fl >> 20) : 0u));
        const uint32_t s_lc = (uint32_t)wave_sum_i32((int)(e_filt == FAQCS_FILT_LOW_COMPLEXITY ? one | e_n : 0u));
        uint32_t s_avg = 0;
        if (o_avgq_on) s_avg = (uint32_t)wave_sum_i32((int)(e_filt == FAQCS_FILT_AVG_Q ? one | e_n : 0u));
        if (lane == 0) {
            const uint32_t m = one - 1u;
            if (s_tot) { atomicAdd(&lfs[FAQCS_TOTAL_COUNT], s_tot >> 20); atomicAdd(&lfs[FAQCS_TOTAL_NUMBER], s_tot >> 20); atomicAdd(&lfs[FAQCS_TOTAL_LENGTH], s_tot & m); }
            if (s_trim) { atomicAdd(&lfs[FAQCS_TOTAL_TRIMMED_NUMBER], s_trim >> 20); atomicAdd(&lfs[FAQCS_TOTAL_TRIMMED_LENGTH], s_trim & m); }
            if (s_len) { atomicAdd(&lfs[FAQCS_READ_LENGTH], s_len >> 20); atomicAdd(&lfs[FAQCS_BASE_LENGTH], s_len & m); }
            if (s_nn) { atomicAdd(&lfs[FAQCS_READ_NN], s_nn >> 20); atomicAdd(&lfs[FAQCS_BASE_NN], s_nn & m); }
            if (s_avg) { atomicAdd(&lfs[FAQCS_READ_AVG_Q], s_avg >> 20); atomicAdd(&lfs[FAQCS_BASE_AVG_Q], s_avg & m); }
            if (s_qt) { atomicAdd(&lfs[FAQCS_READ_QUAL_TRIM], s_qt >> 20); atomicAdd(&lfs[FAQCS_BASE_QUAL_TRIM], s_qt & m); }
            if (s_lc) { atomicAdd(&lfs[FAQCS_READ_LOW_COMPLEXITY], s_lc >> 20); atomicAdd(&lfs[FAQCS_BASE_LOW_COMPLEXITY], s_lc & m); }
        }
}

#ifdef __HIPCC__
// ---- one composition record per lane -> the block's 10 001 x 6 table of 16-bit cells (two per dword), the arithmetic of trim.cpp:860-874.  Called
// by whole waves (the ballots below), by both fold kernels: composition_histogram (faqcs_trim_kernel.hip) and comp_fold_tail.  x (, y): the record
// (WIDE: the two-word form, 11-bit fields), 0 = none; normt: the per-length factors in LDS.
__device__ __forceinline__ void comp_cell_add(uint32_t *tab, const uint32_t e, const uint32_t v, const int lane)
{
#ifdef FAQCS_DIAG_FOLD_NOCONFLICT // (diagnostic build, wrong results: every lane of a wave on a dword of its own -- what the adds of a wave that meet on one cell or bank cost)
    constexpr uint32_t ND_ = (FAQCS_NCOMP_BIN * FAQCS_NCOMP_KIND + 1) / 2;
    uint32_t d = ((e >> 1) & ~63u) | (uint32_t)lane;
    d = d >= ND_ ? d - 64u : d;
    atomicAdd(&tab[d], v << (16 * (e & 1u)));
#else
    atomicAdd(&tab[e >> 1], v << (16 * (e & 1u)));
#endif
}
template <bool WIDE>
__device__ __forceinline__ void comp_fold_record(uint32_t *tab, const float *normt, const unsigned long long x, const unsigned long long y, const int lane)
{
    uint32_t nbin = 0xffffffffu; // this lane's N bin (none)
    if (x & CR_VALID) {
        uint32_t len, cnt[5];
        if (WIDE) {
            len = (uint32_t)(x & 2047u);
            cnt[0] = (uint32_t)(x >> 11) & 2047u; cnt[1] = (uint32_t)(x >> 22) & 2047u; cnt[2] = (uint32_t)(x >> 33) & 2047u;
            cnt[3] = (uint32_t)y & 2047u; cnt[4] = (uint32_t)(y >> 11) & 2047u;
        } else {
            len = (uint32_t)(x & 511u);
#pragma unroll
            for (int k = 0; k < 5; ++k) cnt[k] = (uint32_t)(x >> (9 + 9 * k)) & 511u;
        }
        const float norm = normt[len];
        uint32_t idx[6];
#pragma unroll
        for (int k = 0; k < 5; ++k) idx[k] = (uint32_t)__fmul_rn(norm, (float)cnt[k]); // trim.cpp:862-872
        idx[5] = idx[3] + idx[2];                                                      // :874 (G + C)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            if (k == 4) continue; // N: below
            comp_cell_add(tab, idx[k] * FAQCS_NCOMP_KIND + k, 1u, lane);
        }
        nbin = idx[4] * FAQCS_NCOMP_KIND + 4;
    }
    // The N bin is the same for nearly every read (no N at all: bin 0): 64 lanes adding to ONE LDS address serialise, and
    // that one kind cost more than the other five together.  The lanes of a wave that hit bin 0 add their count once; a read
    // with N in it adds for itself (a loop over the distinct bins of the wave was measured: 3 % of the co-running trim launch).
    constexpr uint32_t bin0 = 4u; // idx 0, kind 4
    const unsigned long long zero = __ballot(nbin == bin0);
    if (zero != 0ull && lane == __builtin_ctzll(zero)) atomicAdd(&tab[bin0 >> 1], (uint32_t)__popcll(zero) << (16 * (bin0 & 1u)));
    if (nbin != 0xffffffffu && nbin != bin0) atomicAdd(&tab[nbin >> 1], 1u << (16 * (nbin & 1u)));
}

// ---- composition records -> the 10 001 x 6 composition tables (trim.cpp:860-874), by a block that owns >= 122 KB of LDS at address `tab` ----------
// The arithmetic of composition_histogram (faqcs_trim_kernel.hip) with the records handed out dynamically: chunks of NT x 4 records from a
// global counter, five chunks per claim.  Used by the blocks of a trim_lds launch that have run out of reads (round 6): `which` = 0 / 1 takes
// the pre- / post-trim records first and the other array behind it, so that the two halves of the grid meet in the middle of the work.
// One-word records only (reads of up to 256 bases).  Every block returns when both counters are exhausted: when the LAST block of the launch
// returns, every chunk has been claimed, and the kernel does not end before its claimer is done -- the fold is complete behind the launch.
template <int NT>
__device__ __forceinline__ void comp_fold_tail(uint32_t *tab, const DevParams &P, const int tid, const uint32_t which)
{
    constexpr int NE = FAQCS_NCOMP_BIN * FAQCS_NCOMP_KIND, ND = (NE + 1) / 2, U = 4;
    constexpr uint32_t CHUNK = NT * U, PER_CLAIM = 5, FLUSH_CLAIMS = 65535u / (CHUNK * PER_CLAIM);
    static_assert(FLUSH_CLAIMS >= 1, "a claim must fit the 16-bit counters");
    float *normt = reinterpret_cast<float *>(tab + ND);
    uint32_t *s_next = tab + ND + 512;
    const uint32_t n = P.fold_n, n_chunks = (n + CHUNK - 1) / CHUNK;
    // nothing left in either array: no table to set up.  ONE thread looks at the two counters and the block takes its verdict from LDS:
    // the counters move while the waves of a block load them, and a wave that returned alone would leave its siblings at the barriers
    // below, reading an *s_next nobody wrote
    if (tid == 0)
        *s_next = (__hip_atomic_load(&P.fold_claim[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n_chunks &&
                   __hip_atomic_load(&P.fold_claim[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n_chunks) ? 1u : 0u;
    __syncthreads();
    const bool nothing_left = *s_next != 0u; // (block-uniform)
    __syncthreads();                         // (*s_next is written again by the claims below)
    if (nothing_left) return;
    for (int i = tid; i < ND; i += NT) tab[i] = 0;
    for (int i = tid; i < 512; i += NT) normt[i] = i <= FAQCS_TAB_LEN ? P.comp_norm[i] : 0.0f;
    __syncthreads();
#pragma unroll 1
    for (uint32_t pass = 0; pass < 2; ++pass) {
        const uint32_t a = which ^ pass;
        const unsigned long long *__restrict__ rec = a ? P.fold_post : P.fold_pre;
        uint64_t *__restrict__ dst = a ? P.fold_dst_post : P.fold_dst_pre;
        uint32_t since_flush = 0;
        bool dirty = false;
#pragma unroll 1
        for (;;) {
            if (tid == 0) *s_next = atomicAdd(&P.fold_claim[a], PER_CLAIM);
            __syncthreads();
            const uint32_t c0 = *s_next;
            __syncthreads();
            if (c0 >= n_chunks) break;
            dirty = true;
#pragma unroll 1
            for (uint32_t c = c0; c < c0 + PER_CLAIM && c < n_chunks; ++c) {
                unsigned long long x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) { const uint32_t i = c * CHUNK + (uint32_t)(u * NT + tid); x[u] = i < n ? rec[i] : 0ull; }
#pragma unroll
                for (int u = 0; u < U; ++u) comp_fold_record<false>(tab, normt, x[u], 0ull, tid & 63);
            }
            if (++since_flush == FLUSH_CLAIMS) {
                __syncthreads();
                for (int d = tid; d < ND; d += NT) {
                    const uint32_t v = tab[d];
                    if (v) {
                        tab[d] = 0;
                        if (v & 0xffffu) atomicAdd((unsigned long long *)(dst + 2 * d), (unsigned long long)(v & 0xffffu));
                        if (v >> 16) atomicAdd((unsigned long long *)(dst + 2 * d + 1), (unsigned long long)(v >> 16));
                    }
                }
                __syncthreads();
                since_flush = 0; dirty = false;
            }
        }
        if (dirty) { // (block-uniform)
            __syncthreads();
            for (int d = tid; d < ND; d += NT) {
                const uint32_t v = tab[d];
                if (v) {
                    tab[d] = 0;
                    if (v & 0xffffu) atomicAdd((unsigned long long *)(dst + 2 * d), (unsigned long long)(v & 0xffffu));
                    if (v >> 16) atomicAdd((unsigned long long *)(dst + 2 * d + 1), (unsigned long long)(v >> 16));
                }
            }
            __syncthreads();
        }
    }
}
#endif
