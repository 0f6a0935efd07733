// faqcs_trim_kernel.hip -- trim_filter_accumulate and composition_histogram (gfx950, wave64).
//
// Replaces trim_read() and its helpers (trim.cpp:225-551, :553-597, :629-885, :1191-1216) for every read
// of a batch.  Two kernels live in this file: trim_filter_accumulate (the single-pass trim kernel) and composition_histogram
// (folds the per-read composition records).  The trim kernels of the library share the accumulators, the flush and the per-chunk
// epilogue (faqcs_trim_common.h).  Which of them takes a submission, and in which shape, is decided in one place, trim_plan()
// (faqcs_trim_plan.h); faqcs_launch_trim_filter_accumulate at the end of this file executes a plan that names this kernel: whatever trim_lds
// (1 ... 304 bases) and trim_long (a read of more than 1 024 bases) leave.
//
// Mapping (trim_filter_accumulate).  LPR lanes share one read and lane l of the group owns the C consecutive positions [l*C, l*C+C), fetched
// with ONE unaligned global_load_dwordx{D} per arena; a wave takes chunks of 64 reads.
//   LPR =  4  reads <= 76 bases (C = 16 / 19):        sixteen reads per wave, one per DPP quad
//   LPR =  8  reads <= 160 bases (C = 13 ... 20):     eight reads per wave, two per 16-lane DPP row
//   LPR = 16  reads <= 256 bases (C = 13 / 16):       four reads per wave, one per DPP row
//   LPR = 32  reads <= 512 bases (C = 10 / 16):       two reads per wave
//   LPR = 64  reads <= 1024 bases (C = 12 / 16):      the whole wave on one read
// Every per-read scalar (length, window, cut points, filter decision) is a group-uniform VGPR value: there are no
// ballots and no scalar-ALU bit logic in the loop (round-1 profiling showed the ballot formulation was SALU-bound at
// ~900 scalar instructions per read).  Cross-lane work is DPP only (RowOps<LPR> in faqcs_dev.h): prefix scans and
// butterflies of 3-4 instructions, shared by all reads of the wave.  What depends on a read's scalars alone (FilterStat,
// small histograms, composition records, the result word) is parked in the read's owner lane and done once per
// chunk, 64 reads wide.
//
// BWA_plus (trim.cpp:714-793) in closed form from ONE prefix sum P of (Q - q[i]) over the window
// (SURVEY.md section 8 a-5):
//   3' pass: reset[i] = (i > 2) & (T - Pin[i] >= 0); the walk stops at the first i (descending) with
//            !reset[i] & !reset[i+1] & reset[i+2] (or after min(5,n) steps if no reset occurs in them);
//            final_pos_3 = argmax_{visited i} (T - Pex[i]) (largest i on ties, only if > 0) - 1
//   5' pass: mirror image with reset[i] = (i < final_pos_3 - 2) & (Pex[i] >= 0) and argmax of Pin[i].
//
// Accumulators.  position x quality: LDS [42][W] dwords, pre-trim count in the low and post-trim count in
// the high 16 bits so a base costs ONE ds_add for both (the post-trim quality of a kept base equals its
// pre-trim quality, trim.cpp:516-533).  position x base: a lane always owns the same positions, so the
// matrix is privatised in REGISTERS (6-bit fields A,T,C,G,N per position, one v_add per base) and spilled
// to LDS every <= 56 reads.  Length / average-quality histograms are small dense LDS arrays.  Composition
// bins (10 001 x 6, sparse and data dependent) are NOT accumulated here: the kernel emits one 8-byte record
// per read (length + 5 base counts, pre and post) and composition_histogram folds the records with the
// whole LDS as a 16-bit table.  A block flushes LDS to the global u64 block with atomics before a 16-bit
// field can overflow (every <= 65 535 reads per block).
//
// Float semantics of the reference are folded into integer lookup tables built on the host
// (DevParams); the only float op left is the composition-bin multiply, an exact IEEE v_mul_f32.
#include "faqcs_trim_common.h"

// WINDOWED: an adapter pre-pass or --5end/--3end can move the window off [0, len); when false (the headline
// configuration) the prefix sum runs over all positions without per-position window tests.
// GENERIC: false = the headline option set (BWA_plus, 5' trimming on, not --qc_only, no --replace_to_N_q, no
// --avg_q, -n 2) is compiled in, so those tests and their live scalars disappear from the loop.
template <int C, int LPR, int NW, bool WINDOWED, bool GENERIC>
__global__ __launch_bounds__(NW * 64, (LPR == 8 || C > 10) ? 2 : FAQCS_TRIM_MINWAVES) void trim_filter_accumulate(
    const DevParams P, const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual,
    const uint32_t *__restrict__ off, const uint32_t n_reads, const uint32_t *__restrict__ ad_sl,
    const uint16_t *__restrict__ ad_hit, uint2 *__restrict__ out, unsigned long long *__restrict__ rec_pre,
    unsigned long long *__restrict__ rec_post, uint64_t *__restrict__ counters, uint32_t *__restrict__ err)
{
    using Cfg = RowCfg<C, LPR>;
    using RW = RowOps<LPR>;
    constexpr int D = Cfg::D, W = Cfg::W, KEY_BIAS = Cfg::KEY_BIAS, PB = Cfg::PB, FK = Cfg::FK;
    constexpr uint32_t PMX = (1u << PB) - 1u;
    constexpr int JB = Cfg::JB;
    constexpr uint32_t JM = (1u << JB) - 1u;
    static_assert(!Cfg::HQ8 || NW * Cfg::HQ8_EVERY <= 255, "an 8-bit cell must not overflow between two flushes");
    constexpr uint32_t CMASK = (1u << C) - 1u;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t *hq = smem + Cfg::O_HQ, *hb = smem + Cfg::O_HB, *hlen = smem + Cfg::O_LEN, *hrq = smem + Cfg::O_RQ;
    uint32_t *hbqpre = smem + Cfg::O_BQPRE, *hbqpost = smem + Cfg::O_BQPOST, *lfs = smem + Cfg::O_FS;
    const uint32_t *t_base = smem + Cfg::O_TBASE, *t_lc = smem + Cfg::O_TLC, *t_magic = smem + Cfg::O_TMAGIC;
    const int32_t *t_avgq = (const int32_t *)(smem + Cfg::O_TAVGQ);
    const uint32_t *t_bm = smem + Cfg::O_TBM;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int rl = lane & (LPR - 1);    // lane inside the row
    const int rowb = lane & (64 - LPR); // first lane of the row
    const int wave = uni(tid >> 6);
    const int pbase = rl * C;

    for (int i = tid; i < Cfg::N_ZERO; i += NW * 64) smem[i] = 0u;
    for (int i = tid; i < 256; i += NW * 64) smem[Cfg::O_TBASE + i] = P.base_tab[i];
    for (int i = tid; i <= W; i += NW * 64) {
        smem[Cfg::O_TLC + i] = P.lc_thr[i];
        smem[Cfg::O_TAVGQ + i] = (uint32_t)P.avgq_min_v[i];
        smem[Cfg::O_TMAGIC + i] = P.div_magic[i];
    }
    for (int i = tid; i < Cfg::BMW * (C + 1); i += NW * 64) {
        const int nb = med3i((i / Cfg::BMW) - 4 * (i % Cfg::BMW), 0, 4);
        smem[Cfg::O_TBM + i] = nb >= 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u);
    }
    uint32_t two = 2u;
    asm volatile("" : "+v"(two)); // a VGPR operand for the SDWA shifts
    // the base-table lookups address LDS by offset: the kernel's only LDS object must start at LDS address 0
    if (tid == 0 && blockIdx.x == 0 && (uint32_t)(size_t)((lds_u32_ptr)smem) != 0u) atomicOr(err, 4u);
    __syncthreads();

    const uint32_t total_chunks = (n_reads + 63) >> 6;
    const uint32_t chunks_per_iter = gridDim.x * NW;
    const uint32_t n_iter = (total_chunks + chunks_per_iter - 1) / chunks_per_iter;
    constexpr uint32_t FLUSH_EVERY = 65535u / (NW * 64) > 0 ? 65535u / (NW * 64) : 1;
    // 6-bit fields: 3 chunks x 16 reads per row = 48 <= 63; a 64-lane row sees 64 reads per chunk and spills mid-chunk too
    constexpr uint32_t REG_FLUSH_EVERY = LPR == 16 ? 3 : (LPR == 8 ? 7 : (LPR == 4 ? 15 : 1)); // 32 lanes: 32 reads per chunk; 64: spills mid-chunk too

    const int in_off = P.in_off, Q = P.Q;
    const int o_mode = GENERIC ? P.mode : (int)FAQCS_MODE_BWA_PLUS;
    const bool o_protect5 = GENERIC ? P.protect5 != 0 : false;
    const bool o_qc_only = GENERIC ? P.qc_only != 0 : false;
    const uint32_t o_replace_q = GENERIC ? P.replace_q : 0u;
    const bool o_avgq_on = GENERIC ? P.avgq_on != 0 : false;
    const uint32_t o_dbg = GENERIC ? P.dbg : 0u;
    const uint32_t o_max_poly_n = GENERIC ? P.max_poly_n : 2u;
    const bool do_trim = !o_qc_only && !(o_dbg & 4u);
    uint32_t bpre[C], bpost[C];
#pragma unroll
    for (int j = 0; j < C; ++j) { bpre[j] = 0; bpost[j] = 0; }
    uint32_t any_err = 0;
    // spill of the register-privatised base matrix to LDS (before a 6-bit field can overflow)
    auto spill_base_regs = [&]() {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const uint32_t x = bpre[j], y = bpost[j];
            if (x) {
#pragma unroll
                for (int c = 0; c < FAQCS_NBASE; ++c) {
                    const uint32_t v = ((x >> BT_SHIFT(c)) & 63u) | (((y >> BT_SHIFT(c)) & 63u) << 16);
                    if (v) atomicAdd(&hb[c * W + pbase + j], v);
                }
            }
            bpre[j] = 0; bpost[j] = 0;
        }
    };

#pragma unroll 1
    for (uint32_t it = 0; it < n_iter; ++it) {
        const uint32_t chunk = (it * gridDim.x + blockIdx.x) * NW + wave;
        // (the 8-bit variant has block barriers inside the read loop: a wave without a chunk runs it with no reads)
        if (Cfg::HQ8 || chunk < total_chunks) {
            const uint32_t base = chunk << 6;
            const uint32_t my = base + lane;
            const bool mine = my < n_reads;
            const uint32_t v_off = mine ? off[my] : 0u;
            const uint32_t v_len = mine ? off[my + 1] - v_off : 0u;
            const uint32_t v_sl = (WINDOWED && ad_sl && mine) ? ad_sl[my] : (v_len << 16);
            const uint32_t v_hit = (ad_hit && mine) ? ad_hit[my] : 0u;
            // Per-read outcome, parked in the lane that owns the read (lane rowb + t): everything that is a function of
            // these scalars alone -- FilterStat sums, the small histograms, composition records, the result word -- is
            // done ONCE per chunk after the read loop, 64 reads wide, instead of 16 times per chunk on row-uniform values.
            uint32_t st_an = 0, st_fl = 0, st_pAT = 0, st_pCG = 0, st_cAT = 0, st_cCG = 0, st_N = 0;
            int st_Vpre = 0, st_Vpost = 0;

            // ---- software prefetch of the row's read 0 ---------------------------------------------------
            PackedBytes<D> nseq, nqual;
            int n_len = __shfl((int)v_len, rowb);
            {
                const uint32_t o = (uint32_t)__shfl((int)v_off, rowb);
#pragma unroll
                for (int k = 0; k < D; ++k) { nseq.w[k] = 0; nqual.w[k] = 0; }
                if (pbase < n_len) {
                    nseq = *(const PackedBytes<D> *)(seq + (size_t)o + pbase);
                    nqual = *(const PackedBytes<D> *)(qual + (size_t)o + pbase);
                }
            }

#pragma unroll 1
            for (int t = 0; t < LPR; ++t) {
                if (!Cfg::HQ8 && base + (uint32_t)t >= n_reads) break; // wave-uniform: no row has a read left
                if (LPR == 64 && t == 32) spill_base_regs();
                const int len = n_len;
                const bool act = base + (uint32_t)(rowb + t) < n_reads;
                uint32_t ws[D], wq[D];
#pragma unroll
                for (int k = 0; k < D; ++k) { ws[k] = nseq.w[k]; wq[k] = nqual.w[k]; }
                const uint32_t sl = WINDOWED ? (uint32_t)__shfl((int)v_sl, rowb + t) : 0u;
                if (t + 1 < LPR) {
                    n_len = __shfl((int)v_len, rowb + t + 1);
                    const uint32_t o = (uint32_t)__shfl((int)v_off, rowb + t + 1);
#pragma unroll
                    for (int k = 0; k < D; ++k) { nseq.w[k] = 0; nqual.w[k] = 0; }
                    if (pbase < n_len) {
                        nseq = *(const PackedBytes<D> *)(seq + (size_t)o + pbase);
                        nqual = *(const PackedBytes<D> *)(qual + (size_t)o + pbase);
                    }
                }
                // zero the bytes past the end of the read (the last dword of a lane may over-read 1..3 bytes)
                {
                    const int vb = med3i(len - pbase, 0, C);
                    const uint4 bm = *reinterpret_cast<const uint4 *>(t_bm + Cfg::BMW * vb); // one ds_read_b128
                    uint32_t m[8] = {bm.x, bm.y, bm.z, bm.w, 0u, 0u, 0u, 0u};
                    if (D > 4) {
                        const uint4 bm2 = *reinterpret_cast<const uint4 *>(t_bm + Cfg::BMW * vb + 4);
                        m[4] = bm2.x; m[5] = bm2.y; m[6] = bm2.z; m[7] = bm2.w;
                    }
#pragma unroll
                    for (int k = 0; k < D; ++k) { ws[k] &= m[k]; wq[k] &= m[k]; }
                }

                // ---- window after the adapter pre-pass and --5end/--3end (trim.cpp:270-314) --------------
                int a = 0, n = len;
                uint32_t flags = 0, filt = 0;
                if (WINDOWED && P.has_adapters) {
                    const int first = (int)(sl & 0xffffu), second = (int)(sl >> 16);
                    const bool mod = len != second;
                    a = mod ? first : 0; n = mod ? second : len;
                    flags = mod ? FAQCS_F_ADAPTER : 0u;
                }
                if (WINDOWED && P.trim5 && !o_qc_only) {
                    const bool over = (int)P.trim5 > n;
                    a = over ? a : a + (int)P.trim5;
                    n = over ? 0 : n - (int)P.trim5;
                }
                if (WINDOWED && P.trim3 && !o_qc_only) n = (int)P.trim3 > n ? 0 : n - (int)P.trim3;
                bool ret = act;
                if (ret && (n < (int)P.min_len || n == 0)) { ret = false; filt = FAQCS_FILT_LENGTH_PRE; }
                uint32_t qt_removed = 0;        // bases removed by the quality trim (BASE_QUAL_TRIM)

                // ---- pass 1 over the lane's C positions ---------------------------------------------------
                uint32_t incf[C];          // class word of the base: 6-bit count fields A,T,C,G,N; the two flag bits above them
                                           // ride along (sums only ever carry them out of the word; every reader masks)
                int q[C], Pin[C];          // clamped quality; inclusive prefix sum of (Q - q) up to this position
                int run, sumv, T, E;
                uint32_t cntpack, nubits, gubits, maxq;
                const int pa = pbase - a;
#pragma unroll 1
                for (int attempt = 0; attempt < 2; ++attempt) {
                    uint32_t inc[C];
                    BaseLookup<C, 0>::run((uint32_t)(Cfg::O_TBASE * 4), ws, two, inc);
                    run = 0; sumv = 0; cntpack = 0; nubits = 0; gubits = 0; maxq = 0;
#pragma unroll
                    for (int j = C - 1; j >= 0; --j) nubits = __builtin_amdgcn_alignbit(nubits, inc[j], 31); // bit j = BT_IS_NU of j
#pragma unroll
                    for (int j = 0; j < C; ++j) {
                        const int sq = (int)(int8_t)((wq[j >> 2] >> (8 * (j & 3))) & 0xffu);
                        const int v = sq - in_off;                              // quality_score() before the clamp
                        q[j] = v < 0 ? 0 : v;                                   // fastq.h:29
                        sumv += v;
                        maxq = umax_(maxq, (uint32_t)q[j]);
                        int dq = Q - q[j];
                        if (WINDOWED) dq = ((unsigned)(pa + j) < (unsigned)n) ? dq : 0;
                        run += dq;
                        Pin[j] = run;
                        cntpack += inc[j];
                        incf[j] = inc[j];
                        if (o_replace_q > 0) gubits |= ((inc[j] >> 30) & 1u) << j;
                    }
                    if (attempt == 1) break;
                    // mask_quality_terminal_N (trim.cpp:1191-1216): upper-case 'N' runs at either end get Q0.
                    // Rare: detect after the fact, patch the quality bytes and redo the pass.
                    const int lastj = len - 1 - pbase;
                    const bool term = ((rl == 0) && (nubits & 1u)) || ((unsigned)lastj < (unsigned)C && ((nubits >> lastj) & 1u));
                    if (!__any(term)) break;
                    const uint32_t inr = range_mask<C>(0, len, pbase);
                    const uint32_t non = inr & ~nubits;
                    const uint32_t fn_l = non ? (uint32_t)(FK - (pbase + __builtin_ctz(non))) : 0u;
                    const uint32_t ln_l = non ? (uint32_t)(pbase + (31 - __builtin_clz(non)) + 1) : 0u;
                    const uint32_t fn_m = RW::all_umax(fn_l), ln_m = RW::all_umax(ln_l);
                    const int lead = fn_m ? FK - (int)fn_m : len;   // first non-N position (len if the read is all N)
                    const int trail_start = (int)ln_m;                // 1 + last non-N position (0 if none)
#pragma unroll
                    for (int j = 0; j < C; ++j) {
                        const int p = pbase + j;
                        if (p < len && (p < lead || p >= trail_start)) {
                            const uint32_t sh = 8 * (j & 3);
                            wq[j >> 2] = (wq[j >> 2] & ~(0xffu << sh)) | (((uint32_t)in_off & 0xffu) << sh);
                        }
                    }
                }
                {
                    const int incl = RW::incl_scan_add(run);
                    E = incl - run;                                  // prefix before this lane's first position
                    T = RW::all_sum(run);
                    // without window masks the zero bytes past the read contributed (Q - 0) each
                    if (!WINDOWED) T -= Q * (LPR * C - len);
                }
                // Pin[] stays LANE-LOCAL (prefix inside the lane); E is folded into whoever needs the row-wide prefix
                const int TE = T - E;
                // whole-read sums: base counts (A,T | C,G as 16-bit pairs), N count and V = sum(raw - offset)
                uint32_t pAT, pCG, pN;
                int V_pre;
                {
                    const uint32_t c = cntpack & BT_FIELDS;
                    const uint32_t at = (c & 63u) | (((c >> 6) & 63u) << 16), cg = ((c >> 12) & 63u) | (((c >> 18) & 63u) << 16);
                    pAT = (uint32_t)RW::all_sum((int)at);
                    pCG = (uint32_t)RW::all_sum((int)cg);
                    // positions past the read contributed (0 - in_off) each: add them back
                    const int vb = med3i(len - pbase, 0, C);
                    const int both = RW::all_sum((((int)((c >> 24) & 63u)) << 20) + (sumv + in_off * (C - vb) + (1 << 12)));
                    pN = (uint32_t)both >> 20;
                    V_pre = (int)((uint32_t)both & 0xfffffu) - (LPR << 12);
                }
                const bool read_err = RW::all_umax(maxq) > 41u;

                // ---- quality trim (trim.cpp:325-360) -----------------------------------------------------
                int hi_sum = 0, lo_sum = 0;     // BWA_plus by-products: prefix sums of (Q - q) at the two cut points
                bool have_sums = false;
                if (do_trim) {
                    int fp3 = n - 1, fp5 = 0;
                    const int a5 = n < 5 ? n : 5, nan2 = n < 2 ? n : 2;
                    hi_sum = 0; lo_sum = 0;
                    if (o_mode == FAQCS_MODE_BWA_PLUS) {
                        // Pex[j] (prefix before position j) is Pin[j-1], or E for the lane's first position
                        // D[j] = T - Pin[j] = suffix sum after position j: its sign is the 3' reset flag, and D[j-1] the
                        // argmax value of position j.  Sign bits are shifted in with one v_alignbit each.
                        int Dv[C];
                        uint32_t nn = 0;
#pragma unroll
                        for (int j = C - 1; j >= 0; --j) {
                            Dv[j] = TE - Pin[j];
                            nn = __builtin_amdgcn_alignbit(nn, (uint32_t)Dv[j], 31); // (nn << 1) | (D < 0)
                        }
                        nn = ~nn;
                        const uint32_t r3 = nn & range_mask<C>(a + nan2 + 1, a + n, pbase);
                        const uint32_t f5 = r3 & range_mask<C>(a + n - a5, a + n, pbase);
                        const uint32_t ext = r3 | (RW::next(r3) << C);
                        const uint32_t c3 = ~ext & ~(ext >> 1) & (ext >> 2) & CMASK;
                        const uint32_t red = RW::all_umax((c3 ? (uint32_t)(pbase + (31 - __builtin_clz(c3)) + 1) : 0u));
                        const bool early = RW::all_or(f5) != 0u;
                        const int pstar = early ? (int)red - 1 : a + n - a5;
                        const uint32_t vis = range_mask<C>(pstar > a ? pstar : a, a + n, pbase);
                        // lane-local argmax of S = T - Pex (largest position on ties), then one row max
                        uint32_t kl = 0, kx[C];
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            const uint32_t k = ((uint32_t)(j ? Dv[j - 1] : TE) << JB) + (uint32_t)((KEY_BIAS << JB) | j);
                            kx[j] = k & (uint32_t)bit_m1(vis, j);
                        }
#pragma unroll
                        for (int j = 0; j + 1 < C; j += 2) kl = umax3_(kl, kx[j], kx[j + 1]);
                        if (C & 1) kl = umax_(kl, kx[C - 1]);
                        const uint32_t K3 = RW::all_umax(kl ? (((kl >> JB) << PB) + (uint32_t)(pa + (int)(kl & JM))) : 0u);
                        const int S3 = (int)(K3 >> PB) - KEY_BIAS;
                        fp3 = (S3 > 0) ? (int)(K3 & PMX) - 1 : n - 1;
                        hi_sum = (S3 > 0) ? T - S3 : T;                       // sum of (Q-q) over window positions <= fp3
                        // 5' pass.  Its cut is the argmax of the prefix sums over the visited positions and only counts when that
                        // maximum is positive (trim.cpp:760-790): with no positive prefix sum anywhere in any of the wave's
                        // reads -- the usual case, a read that starts at Q >= -q -- the whole pass is skipped.
                        int pmax = Pin[0];
#pragma unroll
                        for (int j = 1; j < C; ++j) pmax = pmax > Pin[j] ? pmax : Pin[j];
                        if (!o_protect5 && __any(pmax + E > 0)) {
#pragma unroll
                            for (int j = 0; j < C; ++j) Pin[j] += E; // (rare path: row-wide prefixes from here on)
                            uint32_t np = 0;
#pragma unroll
                            for (int j = C - 1; j >= 0; --j) np = __builtin_amdgcn_alignbit(np, (uint32_t)(j ? Pin[j - 1] : E), 31);
                            np = ~np; // bit j = (prefix before position j >= 0)
                            const uint32_t r5 = np & range_mask<C>(a, a + fp3 - nan2, pbase);
                            const uint32_t g5 = r5 & range_mask<C>(a, a + a5, pbase);
                            const uint32_t ext5 = (r5 << 2) | ((RW::prev(r5) >> (C - 2)) & 3u); // bit k <-> position pbase + k - 2
                            const uint32_t c5 = ~(ext5 >> 2) & ~(ext5 >> 1) & ext5 & CMASK;
                            const uint32_t red5 = RW::all_umax(c5 ? (uint32_t)(FK - (pbase + __builtin_ctz(c5))) : 0u);
                            const bool early5 = RW::all_or(g5) != 0u;
                            const int pstar5 = early5 ? FK - (int)red5 : a + a5 - 1;
                            const uint32_t vis5 = range_mask<C>(a, (pstar5 + 1 < a + n) ? pstar5 + 1 : a + n, pbase);
                            uint32_t kl5 = 0, ky[C];
#pragma unroll
                            for (int j = 0; j < C; ++j) {
                                const uint32_t k = ((uint32_t)Pin[j] << JB) + (uint32_t)((KEY_BIAS << JB) | ((int)JM - j));
                                ky[j] = k & (uint32_t)bit_m1(vis5, j);
                            }
#pragma unroll
                            for (int j = 0; j + 1 < C; j += 2) kl5 = umax3_(kl5, ky[j], ky[j + 1]);
                            if (C & 1) kl5 = umax_(kl5, ky[C - 1]);
                            const uint32_t K5 = RW::all_umax(kl5 ? (((kl5 >> JB) << PB) + (uint32_t)((int)PMX - (pa + (int)JM - (int)(kl5 & JM)))) : 0u);
                            const int S5 = (int)(K5 >> PB) - KEY_BIAS;
                            fp5 = (S5 > 0) ? (int)PMX - (int)(K5 & PMX) + 1 : 0;
                            lo_sum = (S5 > 0) ? S5 : 0;                       // sum of (Q-q) over window positions < fp5
                        }
                        have_sums = true;
                    } else if (o_mode == FAQCS_MODE_BWA) { // trim.cpp:675-709
                        uint32_t neg = 0;
#pragma unroll
                        for (int j = C - 1; j >= 0; --j) neg = (neg << 1) | (uint32_t)(Pin[j] > TE);
                        neg &= range_mask<C>(a, a + n, pbase);
                        const int pf = (int)RW::all_umax(neg ? (uint32_t)(pbase + (31 - __builtin_clz(neg)) + 1) : 0u) - 1; // -1: none
                        const int lo = (pf < a ? a : pf) + 1;
                        const uint32_t vis = range_mask<C>(lo, a + n, pbase);
                        uint32_t key = 0;
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            const uint32_t k = ((uint32_t)(TE - (j ? Pin[j - 1] : 0) + KEY_BIAS) << PB) + (uint32_t)(pa + j);
                            key = umax_(key, k & (uint32_t)bit_m1(vis, j));
                        }
                        const uint32_t K3 = RW::all_umax(key);
                        fp3 = ((int)(K3 >> PB) - KEY_BIAS > 0) ? (int)(K3 & PMX) - 1 : n - 1;
                    } else { // HARD, trim.cpp:629-672
                        uint32_t h0 = 0;
#pragma unroll
                        for (int j = C - 1; j >= 0; --j) h0 = (h0 << 1) | (uint32_t)(Q < q[j]);
                        h0 &= range_mask<C>(a, a + n, pbase);
                        const uint32_t h1 = h0 & range_mask<C>(a + 1, a + n, pbase);
                        const int h = (int)RW::all_umax(h1 ? (uint32_t)(pbase + (31 - __builtin_clz(h1)) + 1) : 0u) - 1;
                        int pos3 = 0;
                        if (h >= 0) { fp3 = h - a; pos3 = fp3; }
                        if (!o_protect5) {
                            const uint32_t lm = RW::all_umax(h0 ? (uint32_t)(FK - (pbase + __builtin_ctz(h0))) : 0u);
                            const int l = lm ? FK - (int)lm - a : 0x7fffffff;
                            if (l < pos3) fp5 = l;
                        }
                    }
                    if (ret) {
                        const int kept = (o_mode == FAQCS_MODE_BWA_PLUS && fp3 <= fp5) ? 0 : fp3 - fp5 + 1;
                        if (kept != n) { qt_removed = (uint32_t)(n - kept); flags |= FAQCS_F_QUAL_TRIMMED; }
                        a += fp5;
                        n = kept;
                        if (n < (int)P.min_len || n == 0) { ret = false; filt = FAQCS_FILT_LENGTH_POST; }
                    }
                }

                // ---- final window: poly-N, counts, sum(raw - offset) ---------------------------------------
                const uint32_t win2 = range_mask<C>(a, a + n, pbase);
                const bool whole = (a == 0 && n == len);
                if (ret && !(o_dbg & 16u)) { // poly-N filter (trim.cpp:363-371, :578-597): upper-case 'N' runs only
                    const uint32_t K = o_max_poly_n;
                    const uint32_t nw = nubits & win2;
                    bool trip;
                    if (K == 0) trip = true;
                    else {
                        const uint32_t e2 = nw | (RW::next(nw) << C);
                        const uint32_t pairs = e2 & (e2 >> 1) & CMASK;
                        const uint32_t red = RW::all_or((nw ? 1u : 0u) | (pairs ? 2u : 0u));
                        if (K == 1) trip = (red & 1u) != 0;
                        else if (K == 2) trip = (red & 2u) != 0;
                        else if (!(red & 2u)) trip = false;
                        else { // exact longest run (rare): run ending at p = p - (last non-N position <= p)
                            uint32_t loc[C], m = 0;
#pragma unroll
                            for (int j = 0; j < C; ++j) {
                                const bool isn = (nw >> j) & 1u, in = (win2 >> j) & 1u;
                                m = umax_(m, (in && !isn) ? (uint32_t)(pbase + j) + 1u : 0u);
                                loc[j] = m;
                            }
                            const uint32_t excl = RW::prev(RW::incl_scan_umax(m)); // max-scan over the lanes before this one
                            uint32_t best = 0;
#pragma unroll
                            for (int j = 0; j < C; ++j) {
                                const uint32_t lastnon = umax_(umax_(excl, loc[j]), (uint32_t)a);
                                best = umax_(best, ((nw >> j) & 1u) ? (uint32_t)(pbase + j) + 1u - lastnon : 0u);
                            }
                            trip = RW::all_umax(best) >= K;
                        }
                    }
                    if (trip) {
                        flags |= FAQCS_F_POLY_N_SEEN;
                        if (!o_qc_only) { ret = false; filt = FAQCS_FILT_POLY_N; }
                    }
                }

                // counts inside the final window, after G -> N (trim.cpp:390-403)
                uint32_t cAT = pAT, cCG = pCG, cN = pN;
                int V_post = V_pre;
                uint32_t repbits = 0;           // positions whose 'G' becomes 'N'
                if (o_replace_q > 0) {
#pragma unroll
                    for (int j = 0; j < C; ++j) repbits |= (uint32_t)(q[j] < (int)o_replace_q) << j;
                    repbits &= gubits & win2;
                }
                if (!(o_dbg & 16u) && __any(ret && (!whole || repbits))) {
                    uint32_t cp = 0;
#pragma unroll
                    for (int j = 0; j < C; ++j) {
                        const uint32_t w = ((repbits >> j) & 1u) ? (1u << BT_SHIFT(4)) : incf[j];
                        cp += w & (uint32_t)bit_m1(win2, j);
                    }
                    const uint32_t at = (cp & 63u) | (((cp >> 6) & 63u) << 16), cg = ((cp >> 12) & 63u) | (((cp >> 18) & 63u) << 16);
                    cAT = (uint32_t)RW::all_sum((int)at);
                    cCG = (uint32_t)RW::all_sum((int)cg);
                    cN = (uint32_t)RW::all_sum((int)((cp >> 24) & 63u));
                    // V_post = sum over the final window of (raw - offset).  With no raw byte below the offset it is
                    // n*Q - sum(Q - q), and BWA_plus already produced both partial sums; otherwise re-add per position.
                    const bool clean = V_pre == len * Q - (WINDOWED ? 0 : T) && !WINDOWED; // all v == q over the whole read
                    if (__all(!ret || (clean && have_sums))) {
                        V_post = n * Q - (hi_sum - lo_sum);
                    } else {
                        int sv = 0;
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            const int sq = (int)(int8_t)((wq[j >> 2] >> (8 * (j & 3))) & 0xffu);
                            sv += (sq - in_off) & bit_m1(win2, j);
                        }
                        V_post = RW::all_sum(sv);
                    }
                }
                const uint32_t cA = cAT & 0xffffu, cT = cAT >> 16, cC = cCG & 0xffffu, cG = cCG >> 16;

                // ---- average quality (trim.cpp:374-382) ----------------------------------------------------
                if (ret && o_avgq_on && V_post < t_avgq[n]) { ret = false; filt = FAQCS_FILT_AVG_Q; }

                // ---- low-complexity filter (trim.cpp:405-513) ----------------------------------------------
                if (ret && !(o_dbg & 16u)) {
                    const uint32_t thr = t_lc[n];
                    const uint32_t mthr = thr & 0xffffu, dthr = thr >> 16;
                    bool trip = cA >= mthr || cT >= mthr || cG >= mthr || cC >= mthr;
                    // dc[X->Y] <= min(count X, count Y): only pairs whose two counts both reach dthr can trip
                    const uint32_t nbig = (cA >= dthr) + (cT >= dthr) + (cC >= dthr) + (cG >= dthr);
                    if (__any(!trip && nbig >= 2)) {
                        // class index per position (0..3 = A,T,C,G inside the window, 7 = anything else)
                        uint32_t cls[C];
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            const uint32_t w = (((repbits >> j) & 1u) ? 0u : incf[j] & 0xffffffu) & (uint32_t)bit_m1(win2, j);
                            cls[j] = w ? (uint32_t)(__builtin_ctz(w) / 6) : 7u;
                        }
                        const uint32_t prev_last = RW::prev(cls[C - 1] + 1u); // 0 at the row edge
                        const uint32_t cnts[4] = {cA, cT, cC, cG};
#pragma unroll
                        for (int x = 0; x < 4; ++x)
#pragma unroll
                            for (int y = 0; y < 4; ++y)
                                if (x != y) {
                                    int dc = 0;
#pragma unroll
                                    for (int j = 0; j < C; ++j) {
                                        const uint32_t pv = j ? cls[j - 1] : prev_last - 1u; // row edge: 0xffffffff
                                        dc += (pv == (uint32_t)x && cls[j] == (uint32_t)y) ? 1 : 0;
                                    }
                                    dc = RW::all_sum(dc);
                                    trip = trip || (cnts[x] >= dthr && cnts[y] >= dthr && (uint32_t)dc >= dthr);
                                }
                    }
                    if (trip) { ret = false; filt = FAQCS_FILT_LOW_COMPLEXITY; }
                }

                // ---- accumulate: position x quality (LDS) and position x base (registers) -----------------
                if (read_err) { any_err = 1; flags |= FAQCS_F_ERR_QUALITY; }
                if (!(o_dbg & 2u)) {
                    // branch-free: a position outside the read adds 0 to a valid address
                    // (bytes past the read are zero -> class word 0 and quality column 0 with increment 0; a read with
                    //  Q > 41 aborts the whole run, fastq.h:31-33, so its row only has to stay inside the tables)
                    if (__any(read_err)) { // rare: keep the row's table indices in range, count nothing
#pragma unroll
                        for (int j = 0; j < C; ++j) { q[j] = read_err ? 0 : q[j]; incf[j] = read_err ? 0u : incf[j]; }
                    }
                    // 1024-wide rows keep exact per-position "pre" bits; the others add 1 for every slot of a counted read and
                    // let flush_block subtract the slots past the read's end
                    const uint32_t inr = Cfg::HQ8 ? ((act && !read_err) ? range_mask<C>(0, len, pbase) : 0u) : 0u;
                    const uint32_t counted = (act && !read_err) ? 1u : 0u;
                    const uint32_t pb4 = 4u * (uint32_t)pbase;
                    const uint32_t postm = ret ? (Cfg::HQ8 ? (win2 & inr) : win2) : 0u;
                    if (Cfg::HQ8) {
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            const int qq = q[j];
                            const uint32_t x = ((inr >> j) & 1u) | ((uint32_t)bit_m1(postm, j) & 0x100u); // pre -> byte 0, post -> byte 1
                            lds_add_u32(__umul24((uint32_t)qq, (uint32_t)(W / 2 * 4)) + (uint32_t)(Cfg::O_HQ * 4) + 4u * (uint32_t)((pbase + j) >> 1),
                                        x << (16 * ((pbase + j) & 1)));
                        }
                    }
                    if (o_replace_q > 0) {
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            const int qq = q[j];
                            if (!Cfg::HQ8) lds_add_u32(__umul24((uint32_t)qq, (uint32_t)(W * 4)) + pb4 + (uint32_t)(Cfg::O_HQ * 4 + 4 * j),
                                                       counted | ((uint32_t)bit_m1(postm, j) & 0x10000u));
                            bpre[j] += incf[j];
                            const uint32_t w = ((repbits >> j) & 1u) ? (1u << BT_SHIFT(4)) : incf[j];
                            bpost[j] += w & (uint32_t)bit_m1(postm, j);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            const int qq = q[j];
                            if (!Cfg::HQ8) lds_add_u32(__umul24((uint32_t)qq, (uint32_t)(W * 4)) + pb4 + (uint32_t)(Cfg::O_HQ * 4 + 4 * j),
                                                       counted | ((uint32_t)bit_m1(postm, j) & 0x10000u));
                            bpre[j] += incf[j];
                            bpost[j] += incf[j] & (uint32_t)bit_m1(postm, j);
                        }
                    }
                }

                // ---- park the read's outcome in its owner lane (see the chunk epilogue) ----------------------
                if (rl == t) {
                    st_an = (uint32_t)a | ((uint32_t)n << 16);
                    st_fl = flags | (ret ? FAQCS_F_VALID : 0u) | (filt << FAQCS_F_FILTER_SHIFT) | (qt_removed << 20);
                    st_pAT = pAT; st_pCG = pCG; st_cAT = cAT; st_cCG = cCG; st_N = pN | (cN << 16);
                    st_Vpre = V_pre; st_Vpost = V_post;
                }
                if (Cfg::HQ8 && (t % Cfg::HQ8_EVERY) == Cfg::HQ8_EVERY - 1) flush_hq8<C, LPR, NW>(smem, counters, P.R, tid);
            }

            // ---- chunk epilogue: one read per lane ----------------------------------------------------------
            if (!(o_dbg & 32u)) {
                const ReadOutcome oc{st_an, st_fl, st_pAT, st_pCG, st_cAT, st_cCG, st_N, st_Vpre, st_Vpost};
                chunk_epilogue<LPR>(oc, mine, my, v_len, v_hit, lane, smem + Cfg::O_LEN, smem + Cfg::O_RQ, smem + Cfg::O_BQPRE,
                                    smem + Cfg::O_BQPOST, smem + Cfg::O_FS, smem + Cfg::O_TMAGIC, out, rec_pre, rec_post, o_avgq_on, o_dbg);
            }
        }

        // ---- spill the register-privatised base matrix to LDS before a 6-bit field can overflow ----------
        const bool block_flush = ((it + 1) % FLUSH_EVERY) == 0 || it + 1 == n_iter;
        if (((it + 1) % REG_FLUSH_EVERY) == 0 || block_flush) spill_base_regs();

        // ---- flush LDS -> global before a 16-bit field can overflow, and at the end ----------------------
        if (block_flush && !(o_dbg & 64u)) flush_block<C, LPR, NW>(smem, counters, P.R, tid);
    }
    if (__any(any_err != 0) && lane == 0) atomicOr(err, 1u);
}

// ---------------------------------------------------------------------------------------------------------
// composition_histogram: update_base_statistics()'s composition part (trim.cpp:860-874) from the per-read
// records.  One thread per record; the block's LDS holds the whole 10 001 x 6 table as 16-bit counters
// (two per dword), flushed to the global u64 block before any of them can overflow.
// ---------------------------------------------------------------------------------------------------------
#ifndef FAQCS_COMP_U
#define FAQCS_COMP_U 4 /* records per thread and round */
#endif
template <int NT, bool WIDE>
__global__ __launch_bounds__(NT) void composition_histogram(const unsigned long long *__restrict__ rec_a, const unsigned long long *__restrict__ rec_b,
                                                            const uint32_t n, const float *__restrict__ comp_norm,
                                                            uint64_t *__restrict__ dst_a, uint64_t *__restrict__ dst_b /* counters + L.{pre,post}_comp */)
{
    constexpr int NE = FAQCS_NCOMP_BIN * FAQCS_NCOMP_KIND; // 60 006 16-bit counters
    constexpr int ND = (NE + 1) / 2;
    constexpr int U = FAQCS_COMP_U; // records per thread and round, fetched together: a round is one memory latency, not U
    extern __shared__ __attribute__((aligned(16))) uint32_t tab[];
    const int tid = threadIdx.x;
    // ONE launch folds both record arrays (pre- and post-trim): even blocks take the first, odd blocks the second (the table
    // fills the LDS of a CU, so the two cannot share one)
    const bool second = (blockIdx.x & 1u) != 0u;
    const unsigned long long *__restrict__ rec = second ? rec_b : rec_a;
    uint64_t *__restrict__ dst = second ? dst_b : dst_a;
    const uint32_t bid = blockIdx.x >> 1, nblk = gridDim.x >> 1; // (the grid is even)
    // the per-length factors behind the table, in LDS too: as a global load the factor sat between a record and its atomics,
    // a second memory latency per round (measured: 5 % of the trim launch the fold shares the GPU with)
    float *normt = reinterpret_cast<float *>(tab + ND);
    constexpr int NNORM = WIDE ? FAQCS_TAB_LEN + 1 : 512;
    for (int i = tid; i < ND; i += NT) tab[i] = 0;
    for (int i = tid; i < NNORM; i += NT) normt[i] = i <= FAQCS_TAB_LEN ? comp_norm[i] : 0.0f;
    __syncthreads();
    const uint32_t per_round = nblk * NT * U;
    const uint32_t rounds = (n + per_round - 1) / per_round;
    constexpr uint32_t FLUSH_EVERY = 65535u / (NT * U);
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t i0 = (r * nblk + bid) * (NT * U) + tid;
        unsigned long long x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = i0 + u * NT;
            x[u] = 0; y[u] = 0;
            if (i < n) {
                if (WIDE) { const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(rec)[i]; x[u] = v.x; y[u] = v.y; }
                else x[u] = rec[i];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) comp_fold_record<WIDE>(tab, normt, x[u], y[u], tid & 63);
        if (((r + 1) % FLUSH_EVERY) == 0 || r + 1 == rounds) {
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

// ---- launch wrappers ---------------------------------------------------------------------------------------
template <int C, int LPR, int NW, bool WINDOWED, bool GENERIC>
static hipError_t launch_trim_t(const TrimPlan &plan, const DevParams &P, const TrimArgs &a)
{
    constexpr size_t lds = (size_t)RowCfg<C, LPR>::LDS_DWORDS * 4;
    static unsigned long long attr_done = 0;
    auto kern = trim_filter_accumulate<C, LPR, NW, WINDOWED, GENERIC>;
    if (plan.NW != NW) return hipErrorInvalidValue;
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds, attr_done); e != hipSuccess) return e;
    if (plan.grid == 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(NW * 64), lds, a.st, P, a.seq, a.qual, a.off, a.n_reads, a.ad_sl, a.ad_hit,
                       reinterpret_cast<uint2 *>(a.out), a.rec_pre, a.rec_post, a.counters, a.err);
    return hipGetLastError();
}

using TrimLaunch = hipError_t (*)(const TrimPlan &, const DevParams &, const TrimArgs &);
// the (WINDOWED, GENERIC) variants of one <C, LPR, NW> shape: all four, or (from 321 bases on) the superset variant, at 512 bases beside the
// default-set one
template <int C, int LPR, int NW, TrimVariants V = TRIM_VARIANTS_FOUR> static TrimLaunch trim_variant(const TrimPlan &plan)
{
    if constexpr (V == TRIM_VARIANTS_FOUR)
        return plan.windowed ? (plan.ext ? launch_trim_t<C, LPR, NW, true, true> : launch_trim_t<C, LPR, NW, true, false>)
                             : (plan.ext ? launch_trim_t<C, LPR, NW, false, true> : launch_trim_t<C, LPR, NW, false, false>);
    if (plan.windowed && plan.ext) return launch_trim_t<C, LPR, NW, true, true>;
    if constexpr (V == TRIM_VARIANTS_ALL_OR_NONE) if (!plan.windowed && !plan.ext) return launch_trim_t<C, LPR, NW, false, false>;
    return nullptr;
}

// executes a plan of trim_plan() that names trim_filter_accumulate: one row of TRIM_TFA_SHAPES each
hipError_t faqcs_launch_trim_filter_accumulate(const TrimPlan &plan, const DevParams &P, const TrimArgs &a)
{
    constexpr int NW = FAQCS_TRIM_NW;
    TrimLaunch f = nullptr;
    switch (trim_shape_key(plan.C, plan.LPR)) {
    case trim_shape_key(16, 4): f = trim_variant<16, 4, NW>(plan); break;
    case trim_shape_key(19, 4): f = trim_variant<19, 4, NW>(plan); break;
    case trim_shape_key(13, 8): f = trim_variant<13, 8, NW>(plan); break;
    case trim_shape_key(16, 8): f = trim_variant<16, 8, NW>(plan); break;
    case trim_shape_key(19, 8): f = trim_variant<19, 8, NW>(plan); break;
    case trim_shape_key(20, 8): f = trim_variant<20, 8, NW>(plan); break;
    case trim_shape_key(13, 16): f = trim_variant<13, 16, NW>(plan); break;
    case trim_shape_key(16, 16): f = trim_variant<16, 16, NW>(plan); break;
    case trim_shape_key(10, 32): f = trim_variant<10, 32, NW>(plan); break;
    case trim_shape_key(16, 32): f = trim_variant<16, 32, NW, TRIM_VARIANTS_ALL_OR_NONE>(plan); break;
    case trim_shape_key(12, 64): f = trim_variant<12, 64, NW, TRIM_VARIANTS_ALL>(plan); break;
    case trim_shape_key(16, 64): f = trim_variant<16, 64, 8, TRIM_VARIANTS_ALL>(plan); break;
    }
    return f ? f(plan, P, a) : hipErrorInvalidValue; // (a shape or variant this file does not compile: a programming error)
}

// wide: the two-word records of the long-read kernels (max_len > 256).  One launch for the pre- and the post-trim records.
hipError_t faqcs_launch_composition(const unsigned long long *rec_pre, const unsigned long long *rec_post, uint32_t n, bool wide,
                                    const float *comp_norm, uint64_t *dst_pre, uint64_t *dst_post, int n_cu, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    constexpr int NT = 1024;
    constexpr size_t lds = (size_t)((FAQCS_NCOMP_BIN * FAQCS_NCOMP_KIND + 1) / 2) * 4 + (size_t)(FAQCS_TAB_LEN + 1) * 4; // table + per-length factors
    static unsigned long long attr_done_w = 0, attr_done_n = 0;
    auto kern = wide ? composition_histogram<NT, true> : composition_histogram<NT, false>;
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds, wide ? attr_done_w : attr_done_n); e != hipSuccess) return e;
    uint32_t per_array = (n + NT * FAQCS_COMP_U - 1) / (NT * FAQCS_COMP_U); // blocks one array can use
    if (per_array > (uint32_t)(n_cu / 2)) per_array = (uint32_t)(n_cu / 2); // (fewer, longer blocks are slower: 64 per array -6 %)
    if (per_array < 1) per_array = 1;
    hipLaunchKernelGGL(kern, dim3(2 * per_array), dim3(NT), lds, st, rec_pre, rec_post, n, comp_norm, dst_pre, dst_post);
    return hipGetLastError();
}
