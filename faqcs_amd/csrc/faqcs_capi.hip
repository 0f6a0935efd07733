// faqcs_capi.hip -- host side of libfaqcs_mi.so: the core of the C ABI declared in include/faqcs_mi.h -- create / destroy, submission,
// sync, the counter block, the timing reports and the synthetic-data helpers.  The context is in faqcs_ctx.h; the rest of the ABI is in
// faqcs_host.cpp (no HIP), faqcs_capi_kmer.hip, faqcs_capi_seam.hip and faqcs_capi_comm.hip.
#include "faqcs_ctx.h"

// ---------------------------------------------------------------------------------------------------------
// host-side integer tables (the reference's float32 expressions, evaluated once per length)
// ---------------------------------------------------------------------------------------------------------
static uint8_t na_to_bits_host(char c)
{
    switch (c) { // seq_overlap.cpp:372-411
    case 'A': case 'a': return 1;  case 'C': case 'c': return 2;  case 'G': case 'g': return 4;
    case 'T': case 't': return 8;  case 'M': case 'm': return 3;  case 'R': case 'r': return 5;
    case 'S': case 's': return 6;  case 'V': case 'v': return 7;  case 'W': case 'w': return 9;
    case 'Y': case 'y': return 10; case 'H': case 'h': return 11; case 'K': case 'k': return 12;
    case 'D': case 'd': return 13; case 'B': case 'b': return 14; case 'N': case 'n': return 15;
    case '-': return 16;
    }
    return 0;
}

// the average-quality thresholds: per read length, the smallest V = sum(raw - offset) >= 0 for which NOT(ave_Q < avg); ave_Q per
// trim.cpp:568-572.  (V < 0 gives ave_Q = 0 < avg, and V < table[len] is then true as well.)  The one table that depends on the input
// quality offset: faqcs_set_input_quality_offset() builds it again.
static void build_avgq(const faqcs_params &p, std::vector<int32_t> &avgq)
{
    const int N = FAQCS_TAB_LEN + 1;
    avgq.assign(N, 0);
    const volatile float avg = p.average_quality;
    if (!(avg > 0.0f)) return;
    for (int len = 1; len < N; ++len) {
        auto pass = [&](int V) {
            volatile float t = (float)(V + p.input_quality_offset * len) / (float)len;
            volatile float v = t - (float)p.input_quality_offset;
            const float a = v > 0.0f ? v : 0.0f;
            return !(a < avg);
        };
        int lo = 0, hi = 256 * len;
        if (!pass(hi)) avgq[len] = 0x7fffffff;
        else { while (lo < hi) { const int mid = (lo + hi) >> 1; if (pass(mid)) hi = mid; else lo = mid + 1; } avgq[len] = lo; }
    }
}

static void build_tables(const faqcs_params &p, std::vector<uint32_t> &lcthr, std::vector<int32_t> &avgq,
                         std::vector<float> &norm, std::vector<uint32_t> &magic, std::vector<uint32_t> &base)
{
    const int N = FAQCS_TAB_LEN + 1;
    lcthr.assign(N, 0xffffffffu); norm.assign(N, 0.f); magic.assign(N, 0);
    build_avgq(p, avgq);
    const volatile float lc = p.low_complexity_cutoff_ratio;
    for (int len = 1; len < N; ++len) {
        uint32_t mono = 0xffff, di = 0xffff;
        volatile float nrm = (float)(1.0 / (double)len);                 // trim.cpp:483
        for (int c = 0; c <= len; ++c) { volatile float v = (float)(unsigned)c * nrm; if (v > lc) { mono = (uint32_t)c; break; } }
        volatile float nrm2 = (float)((double)nrm * 2.0);                // trim.cpp:499
        for (int c = 0; c <= len; ++c) { volatile float v = (float)(unsigned)c * nrm2; if (v > lc) { di = (uint32_t)c; break; } }
        lcthr[len] = mono | (di << 16);
        norm[len] = (float)(FAQCS_NCOMP_BIN - 1) / (float)len;           // trim.cpp:860
        magic[len] = (uint32_t)((1ull << 32) / (uint64_t)len) + 1u;      // exact floor(V/len) for V < 2^16, len >= 2
    }
    // per input byte: 6-bit count fields in FaQCs enum order A,T,C,G,N (FaQCs.h:35-42), case-insensitive like
    // update_base_statistics (trim.cpp:831-857); flag bits for the case-sensitive tests (trim.cpp:396,586,1196)
    base.assign(256, 0u);
    const char *letters = "ATCGN";
    for (int k = 0; k < 5; ++k) {
        base[(unsigned char)letters[k]] = 1u << BT_SHIFT(k);
        base[(unsigned char)(letters[k] | 0x20)] = 1u << BT_SHIFT(k);
    }
    base['N'] |= BT_IS_NU;
    base['G'] |= BT_IS_GU;
}

template <class T> static hipError_t upload(T **dst, const std::vector<T> &v)
{
    hipError_t e = hipMalloc((void **)dst, v.size() * sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// ---------------------------------------------------------------------------------------------------------
// create / destroy
// ---------------------------------------------------------------------------------------------------------
extern "C" int faqcs_create(const faqcs_params *p, int device_id, faqcs_ctx **out)
{
    if (!p || !out) return fail(FAQCS_E_INVAL, "faqcs_create: null argument");
    if (p->abi_version != FAQCS_ABI_VERSION) return fail(FAQCS_E_INVAL, "faqcs_create: ABI version mismatch");
    if (p->max_read_length == 0 || p->max_read_length > FAQCS_MAX_READ_LENGTH) return fail(FAQCS_E_INVAL, "faqcs_create: max_read_length out of range");
    if (p->n_adapters > FAQCS_MAX_ADAPTERS)
        return fail(FAQCS_E_INVAL, "faqcs_create: " + std::to_string(p->n_adapters) + " adapters, at most " + std::to_string(FAQCS_MAX_ADAPTERS) + " are supported");
    if (p->mode < 0 || p->mode > 2) return fail(FAQCS_E_INVAL, "trim.cpp:trim_read: Undefined trimming mode!");
    // the argmax keys of the trim kernel hold |sum of (Q - q)| <= 1024 * (|Q| + 41) in 18 bits (16 for reads <= 256 bases)
    if (p->quality < -93 || p->quality > 93) return fail(FAQCS_E_INVAL, "faqcs_create: quality threshold outside [-93, 93]");
    if (p->kmer_rarefaction && (p->kmer < 2 || p->kmer > 31 || p->split_size == 0)) return fail(FAQCS_E_INVAL, "faqcs_create: kmer / split_size out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(FAQCS_E_NODEVICE, "faqcs_create: no HIP device (the FaQCs MI355X hot path has no CPU fallback)");
    if (device_id < 0) HIPCHK(hipGetDevice(&device_id));
    HIPCHK(hipSetDevice(device_id));
    // owned by a guard until every allocation below has succeeded: an early HIPCHK return must not leak the context
    std::unique_ptr<faqcs_ctx, void (*)(faqcs_ctx *)> guard(new faqcs_ctx(), faqcs_destroy);
    faqcs_ctx *c = guard.get();
    c->prm = *p;
    c->prm.adapter_seq = nullptr;
    c->device = device_id;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIPCHK(hipStreamCreateWithFlags(&c->compute, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
    for (auto &rs : c->rec) { HIPCHK(hipEventCreateWithFlags(&rs.trimmed, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&rs.folded, hipEventDisableTiming)); }
    HIPCHK(hipEventCreateWithFlags(&c->copied, hipEventDisableTiming));
    for (auto &sl : c->slot) HIPCHK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    for (auto &e : c->ticket_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    faqcs_counters_layout(p->max_read_length, p->n_adapters, &c->lay);

    std::vector<uint32_t> lcthr, magic, basetab; std::vector<int32_t> avgq; std::vector<float> norm;
    build_tables(*p, lcthr, avgq, norm, magic, basetab);
    HIPCHK(upload(&c->d_lcthr, lcthr)); HIPCHK(upload(&c->d_avgq, avgq)); HIPCHK(upload(&c->d_norm, norm));
    HIPCHK(upload(&c->d_magic, magic)); HIPCHK(upload(&c->d_basetab, basetab));
    HIPCHK(hipMalloc((void **)&c->d_counters, c->lay.total * sizeof(uint64_t)));
    HIPCHK(hipMemset(c->d_counters, 0, c->lay.total * sizeof(uint64_t)));
    HIPCHK(hipMalloc((void **)&c->d_err, 256)); // [0] error bits ; bytes 64.. : 16 diagnostic u64 words (FAQCS_LDS_STAMPS builds)
    HIPCHK(hipMemset(c->d_err, 0, 256));
    {   // trim_lds: one row per block and flush, then the rows each block used
        const size_t dwords = (size_t)c->n_cu * FAQCS_PARTIAL_FLUSHES * FAQCS_PARTIAL_ROW + (size_t)c->n_cu;
        HIPCHK(hipMalloc((void **)&c->d_partials, dwords * sizeof(uint32_t)));
        HIPCHK(hipMemset(c->d_partials, 0, dwords * sizeof(uint32_t)));
    }

    if (p->n_adapters) {
        std::vector<uint8_t> bits; std::vector<uint32_t> start(1, 0);
        for (uint32_t j = 0; j < p->n_adapters; ++j) {
            const char *s = p->adapter_seq[j];
            const size_t L = strlen(s);
            if (L == 0 || L > FAQCS_MAX_ADAPTER_LENGTH)
                return fail(FAQCS_E_INVAL, "faqcs_create: adapter " + std::to_string(j) + " has " + std::to_string(L) + " bases, 1 ... " +
                                               std::to_string(FAQCS_MAX_ADAPTER_LENGTH) + " are supported");
            c->adapters.emplace_back(s);
            for (size_t k = 0; k < L; ++k) {
                const uint8_t b = na_to_bits_host(s[k]);
                if (!b) return fail(FAQCS_E_BASE, "seq_overlap.cpp:na_to_bits: Unknown base!");
                if (b == 16) c->adapter_has_gap = 1u;
                bits.push_back(b);
            }
            start.push_back((uint32_t)bits.size());
        }
        // bit-planes for the prefilter: per adapter word w, 4 dwords (A,C,G,T) over bases [32w, 32w+32)
        std::vector<uint32_t> planes, wstart(1, 0);
        for (uint32_t j = 0; j < p->n_adapters; ++j) {
            const uint32_t L = start[j + 1] - start[j], nw = (L + 31) / 32;
            for (uint32_t w = 0; w < nw; ++w) {
                uint32_t pl[4] = {0, 0, 0, 0};
                for (uint32_t k = 0; k < 32 && 32 * w + k < L; ++k)
                    for (int b = 0; b < 4; ++b) pl[b] |= (uint32_t)((bits[start[j] + 32 * w + k] >> b) & 1u) << k;
                planes.insert(planes.end(), pl, pl + 4);
            }
            wstart.push_back(wstart.back() + nw);
        }
        HIPCHK(upload(&c->d_abits, bits)); HIPCHK(upload(&c->d_astart, start));
        HIPCHK(upload(&c->d_aplanes, planes)); HIPCHK(upload(&c->d_awstart, wstart));
        c->adapter_plane_dwords = (uint32_t)planes.size();
        for (uint32_t j = 0; j < p->n_adapters; ++j) c->adapter_longest = std::max(c->adapter_longest, start[j + 1] - start[j]);
        c->match_rate = (float)(1.0 - (double)p->filterAdapterMismatchRate); // trim.cpp:969
        if (p->n_adapters > FAQCS_ADAPTER_GROUP || c->adapter_longest > FAQCS_ADAPTER_SINGLE_LENGTH) {
            // consecutive groups of at most FAQCS_ADAPTER_GROUP targets whose planes fit the kernel's LDS copy (a target of 32 767 bases
            // has 1 024 plane words = FAQCS_ADAPTER_TPL_CAP dwords: every target fits a group of its own)
            std::vector<uint32_t> wgrp;
            for (uint32_t j = 0; j < p->n_adapters;) {
                faqcs_ctx::AdapterGroupHost g{j, 0, wstart[j], 0, 0};
                while (j < p->n_adapters && g.n < FAQCS_ADAPTER_GROUP && 4u * (wstart[j + 1] - g.w0) <= FAQCS_ADAPTER_TPL_CAP) {
                    g.longest = std::max(g.longest, start[j + 1] - start[j]);
                    ++g.n; ++j;
                }
                g.plane_dwords = 4u * (wstart[j] - g.w0);
                for (uint32_t k = g.j0; k <= j; ++k) wgrp.push_back(wstart[k] - g.w0);
                c->agroups.push_back(g);
            }
            HIPCHK(upload(&c->d_awstart_grp, wgrp));
        }
    }

    DevParams &d = c->dp;
    memset(&d, 0, sizeof(d));
    d.mode = p->mode; d.Q = p->quality; d.in_off = p->input_quality_offset; d.out_off = p->output_quality_offset;
    // (anything above the longest read behaves like the longest read + 1; the kernels compare these as ints)
    auto cap16 = [](uint32_t v) { return v > 65535u ? 65535u : v; };
    d.min_len = cap16(p->min_read_length); d.max_poly_n = cap16(p->max_num_poly_N); d.trim5 = cap16(p->trim_5); d.trim3 = cap16(p->trim_3);
    d.replace_q = p->replace_to_N_q; d.protect5 = p->protect_5; d.qc_only = p->qc_only;
    d.has_adapters = p->n_adapters ? 1 : 0; d.avgq_on = p->average_quality > 0.0f ? 1 : 0;
    d.R = p->max_read_length; d.n_adapters = p->n_adapters;
    d.lc_ratio = p->low_complexity_cutoff_ratio; d.avg_q = p->average_quality;
    if (const char *e = getenv("FAQCS_DBG")) d.dbg = (uint32_t)strtoul(e, nullptr, 0);
    d.lc_thr = c->d_lcthr; d.avgq_min_v = c->d_avgq; d.comp_norm = c->d_norm; d.div_magic = c->d_magic; d.base_tab = c->d_basetab;
    d.partials = c->d_partials;
    d.partial_rows = c->d_partials + (size_t)c->n_cu * FAQCS_PARTIAL_FLUSHES * FAQCS_PARTIAL_ROW;
    d.lay = c->lay;

    c->kmer_active = p->kmer_rarefaction ? 1 : 0;
    if (p->kmer_rarefaction) {
        uint64_t slots = p->kmer_table_slots ? p->kmer_table_slots : (1ull << 28);
        uint64_t pow2 = 1; while (pow2 < slots) pow2 <<= 1;
        // every partition of the combine-before-insert path owns a slice of the table (faqcs_kmer_skm_kernel.hip)
        if (pow2 < (uint64_t)KG_SLICE_MIN << 16) pow2 = (uint64_t)KG_SLICE_MIN << 16;
        if (pow2 > (uint64_t)KG_SLICE_MAX << 16) return fail(FAQCS_E_INVAL, "faqcs_create: kmer_table_slots above 2^32");
        c->kt.mask = pow2 - 1;
        { uint32_t lg = 0; while ((1ull << lg) < pow2) ++lg; if (lg > 46) return fail(FAQCS_E_INVAL, "faqcs_create: kmer_table_slots too large"); c->kt.shift = 62 - lg; }
        if (const char *e = getenv("FAQCS_KMER_DIRECT")) c->kg.direct = atoi(e) != 0;
        // the overflow area (1/16 of the table, at least 2^16 slots): keys whose probe window in their partition's slice is full
        c->kt.ovf_mask = std::max<uint64_t>(pow2 >> 4, 1ull << 16) - 1;
        // fine partitions (faqcs_kmer.h): a table that is full (0.6 keys per slot) holds about 1 200 keys per fine partition up to 2^30 slots --
        // a third of what one round of the counting kernel's LDS table takes; 2^31 slots: 2 450, 2^32: 4 900 (several rounds then)
        { const uint32_t lg = 62 - c->kt.shift;
          int f = (int)lg - 27; f = f < 0 ? 0 : (f > 3 ? 3 : f);
          if (const char *e = getenv("FAQCS_KMER_FINE_BITS")) { const int v = atoi(e); if (v >= 0 && v <= 3) f = v; } // (tests: every F on a small table)
          while (f > 0 && (pow2 >> (16 + f)) < 16) --f;                    // a slice has at least 16 slots
          while (f < 3 && (pow2 >> (16 + f)) > (uint64_t)KG_SLICE_MAX / 8) ++f; // ... and at most what the counting kernel's claim bitmap covers
          c->kt.fine = (uint32_t)f; }
        HIPCHK(hipMalloc((void **)&c->kt.dirty, (size_t)(1u << (16 + c->kt.fine)) / 8));
        HIPCHK(hipMemset(c->kt.dirty, 0, (size_t)(1u << (16 + c->kt.fine)) / 8));
        HIPCHK(hipMalloc((void **)&c->kt.slots, kmer_table_total(c->kt) * sizeof(KmerSlot)));
        HIPCHK(hipMalloc((void **)&c->kt.stats, 64));
        HIPCHK(faqcs_launch_kmer_table_init(c->kt, c->n_cu, c->compute)); // empty key, count - 1 = 0, no epoch
        HIPCHK(hipMemset(c->kt.stats, 0, 64));
        c->snap_cap = 4096;
        HIPCHK(hipMalloc((void **)&c->d_snaps, c->snap_cap * 16));
    }
    *out = guard.release();
    return 0;
}

extern "C" void faqcs_destroy(faqcs_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->compute) (void)hipStreamSynchronize(c->compute);
    if (c->copy) (void)hipStreamSynchronize(c->copy);
    if (c->aux) (void)hipStreamSynchronize(c->aux);
    for (auto &t : c->timings) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); (void)hipEventDestroy(t.p); (void)hipEventDestroy(t.k0); (void)hipEventDestroy(t.k1); }
    if (c->comm) comm_release(c->comm);
    if (c->comm_ev) (void)hipEventDestroy(c->comm_ev);
    c->emit.release(); c->parse.release(); c->render.release(); c->pair.release(); c->render_pair.release(); c->inflate.release(); c->bgzf_index.release(); c->deflate.release(); c->detect.release(); c->gunzip.release();
    if (c->ins_a) (void)hipEventDestroy(c->ins_a);
    if (c->ins_b) (void)hipEventDestroy(c->ins_b);
    for (int k = 0; k < 2; ++k) { if (c->fwd_free[k]) (void)hipEventDestroy(c->fwd_free[k]); if (c->fwd_copied[k]) (void)hipEventDestroy(c->fwd_copied[k]); c->fwd_items[k].release(); }
    void *ptrs[] = {c->d_lcthr, c->d_basetab, c->d_avgq, c->d_norm, c->d_magic, c->d_counters, c->d_err, c->d_partials, c->d_abits, c->d_astart, c->d_aplanes, c->d_awstart,
                    c->d_awstart_grp, c->kt.slots, c->kt.stats, c->kt.dirty, c->d_fold_claim, c->d_snaps, c->d_ob, c->d_tot_by_epoch, c->d_first_hist};
    for (void *q : ptrs) if (q) (void)hipFree(q);
    for (auto &sl : c->slot) { sl.seq.release(); sl.qual.release(); sl.tn.release(); sl.off.release(); if (sl.done) (void)hipEventDestroy(sl.done); }
    for (auto &e : c->ticket_ev) if (e) (void)hipEventDestroy(e);
    c->s_seg.release(); c->s_sl.release(); c->s_hit.release(); c->s_res.release(); c->s_astate.release(); c->s_amask.release();
    for (auto &rs : c->rec) { rs.pre.release(); rs.post.release(); if (rs.trimmed) (void)hipEventDestroy(rs.trimmed); if (rs.folded) (void)hipEventDestroy(rs.folded); }
    if (c->aux) (void)hipStreamDestroy(c->aux);
    c->ob_items.release(); c->ob_wave_count.release(); c->ob_wave_offset.release();
    { void *kg_ptrs[] = {c->kg.dev.l1, c->kg.dev.l2, c->kg.dev.cur1, c->kg.dev.cur2, c->kg.dev.run_epoch, c->kg.dev.first_hist, c->kg.dev.tot_by_epoch, c->kg.dev.dense, c->kg.dev.big, c->kg.dev.n_big, c->kg.dev.redo};
      for (void *q : kg_ptrs) if (q) (void)hipFree(q);
      c->kg.defer.release();
      c->ks.l1.release(); c->ks.spill.release(); c->ks.cur1.release(); c->ks.run_epoch.release(); c->ks.defer.release(); c->ks.scratch.release();
      for (auto &ev : c->kg.flush_ev) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); } }
    if (c->copied) (void)hipEventDestroy(c->copied);
    if (c->compute) (void)hipStreamDestroy(c->compute);
    if (c->copy) (void)hipStreamDestroy(c->copy);
    delete c;
}

extern "C" int faqcs_set_quality(faqcs_ctx *c, int quality)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (quality < -93 || quality > 93) return fail(FAQCS_E_INVAL, "faqcs_set_quality: quality threshold outside [-93, 93]");
    c->prm.quality = quality;
    c->dp.Q = quality;
    return 0;
}

// What faqcs_create() derives from the offset: prm, dp.in_off and the average-quality table.  The table is device memory that enqueued
// kernels read, so the context's streams are drained first: work enqueued before the call sees the old offset, work after it the new one.
extern "C" int faqcs_set_input_quality_offset(faqcs_ctx *c, int input_quality_offset)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->copy));
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipStreamSynchronize(c->aux));
    c->prm.input_quality_offset = input_quality_offset;
    c->dp.in_off = input_quality_offset;
    std::vector<int32_t> avgq;
    build_avgq(c->prm, avgq);
    HIPCHK(hipMemcpy(c->d_avgq, avgq.data(), avgq.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// submission
// ---------------------------------------------------------------------------------------------------------
// the event slot of a submission that has reads
static int take_timing(faqcs_ctx *c, Timing *&tm)
{
    if (c->timing_used == c->timings.size()) {
        Timing t; HIPCHK(hipEventCreate(&t.a)); HIPCHK(hipEventCreate(&t.b)); HIPCHK(hipEventCreate(&t.p)); HIPCHK(hipEventCreate(&t.k0)); HIPCHK(hipEventCreate(&t.k1));
        t.adapter = false; t.kmer = false; c->timings.push_back(t);
    }
    tm = &c->timings[c->timing_used++];
    tm->adapter = c->prm.n_adapters != 0;
    tm->kmer = false;
    return 0;
}

// the adapter pre-pass: every read's best hit in s_sl / s_hit
static int enqueue_adapter(faqcs_ctx *c, Timing &t, const Submission &s)
{
    const uint32_t n = s.n;
    HIPCHK(hipEventRecord(t.p, c->compute));
    HIPCHK(c->s_sl.reserve(n)); HIPCHK(c->s_hit.reserve(n)); HIPCHK(c->s_seg.reserve(s.n_seg + 1));
    HIPCHK(hipMemcpyAsync(c->s_seg.p, s.seg, (s.n_seg + 1) * 4, hipMemcpyHostToDevice, c->compute));
    auto launch = [&](const AdapterDev &A, const AdapterGroup *G) {
        return faqcs_launch_adapter(A, G, s.seq, s.off, n, s.max_len, c->s_seg.p, s.n_seg, c->s_sl.p, c->s_hit.p,
                                    c->d_counters + c->lay.adapter_stats, c->d_err, c->dp.dbg, c->n_cu, c->compute);
    };
    if (c->agroups.empty()) {
        AdapterDev A{c->d_abits, c->d_astart, c->d_aplanes, c->d_awstart, c->prm.n_adapters, c->match_rate, c->adapter_longest, c->adapter_plane_dwords,
                     c->adapter_has_gap};
        HIPCHK(launch(A, nullptr));
        return 0;
    }
    // one launch per group of targets, in library order; every read's state is carried from one to the next
    AdapterGroup G{};
    G.mask_words = (s.max_len + 63) / 64;
    HIPCHK(c->s_astate.reserve(n)); HIPCHK(c->s_amask.reserve((size_t)n * G.mask_words));
    HIPCHK(hipMemsetAsync(c->s_astate.p, 0, (size_t)n * sizeof(uint4), c->compute));
    G.state = c->s_astate.p; G.mask = c->s_amask.p; G.gstart = c->d_astart;
    for (size_t k = 0; k < c->agroups.size(); ++k) {
        const faqcs_ctx::AdapterGroupHost &g = c->agroups[k];
        AdapterDev A{c->d_abits, c->d_astart + g.j0, c->d_aplanes + 4 * (size_t)g.w0, c->d_awstart_grp + g.j0 + k, g.n, c->match_rate,
                     g.longest, g.plane_dwords, c->adapter_has_gap};
        G.j0 = g.j0; G.last = k + 1 == c->agroups.size() ? 1u : 0u;
        HIPCHK(launch(A, &G));
    }
    return 0;
}

// an environment switch that is on unless set to 0
static bool env_on(const char *name) { const char *e = getenv(name); return !e || atoi(e) != 0; }

// the trim launch: trim_plan() (faqcs_trim_plan.h) says which kernel, in which shape, how many records, and who folds.  The composition
// records of a launch are folded one launch LATE (faqcs_ctx::pending_fold): by this launch's blocks as they run out of reads, else by
// composition_histogram on the aux stream beside it.
static int enqueue_trim(faqcs_ctx *c, Timing &t, const Submission &s, const uint32_t *d_sl, const uint16_t *d_hit)
{
    const uint32_t n = s.n;
    HIPCHK(hipEventRecord(t.a, c->compute));
    // the records of the launch BEFORE this one: this launch's blocks fold them when they run out of reads, if its kernel can (trim_lds with
    // a block of at least 122 KB of LDS and one-word records: the shapes of 105 ... 152 and of 153 ... 252 bases, TrimLdsShape::folds_tail --
    // not the 4-lane shapes, not 77 ... 104, not 253 ... 304); FAQCS_TAIL_FOLD=0: never (A/B)
    const bool tail_on = env_on("FAQCS_TAIL_FOLD"); // (read at every submission, like FAQCS_TRIM_LONG below: a test runs one engine with it and one without)
    const bool offer_fold = c->pending_fold >= 0 && !c->pending_wide && tail_on;
    DevParams dp = c->dp;
    dp.fold_n = offer_fold ? c->pending_n : 0u;
    static const bool lds_on = env_on("FAQCS_TRIM_LDS"), lds4_on = env_on("FAQCS_TRIM_LDS4"), lds16_on = env_on("FAQCS_TRIM_LDS16"); // (once per process)
    const char *e_long = getenv("FAQCS_TRIM_LONG"); // (read at every submission: a test turns it on for one engine)
    const TrimPlan plan = trim_plan(trim_options(dp), s.max_len, n, c->n_cu, TrimSwitches{e_long && atoi(e_long) != 0, lds_on, lds4_on, lds16_on});
    const bool long_reads = plan.kernel == TrimKernel::trim_long; // composition bins are added by the kernel itself, no records
    dp.wide_records = plan.wide_records;
    const int set = (int)(c->n_enqueued++ & 1);
    faqcs_ctx::RecSet &rs = c->rec[set];
    if (rs.used) { HIPCHK(hipStreamWaitEvent(c->compute, rs.folded, 0)); rs.used = false; ++c->tally.recset_fold_waits; } // (a fold of the set's previous records on the aux stream)
    const size_t need = plan.records_needed;
    if (need > rs.pre.cap) { HIPCHK(hipStreamSynchronize(c->aux)); HIPCHK(hipStreamSynchronize(c->compute)); ++c->tally.recset_grow_syncs; } // (the set's old records may still be read: by the fold kernel, or by the launch before this one)
    HIPCHK(rs.pre.reserve(need)); HIPCHK(rs.post.reserve(need));
    if (offer_fold) {
        const faqcs_ctx::RecSet &ps = c->rec[c->pending_fold];
        if (!c->d_fold_claim) HIPCHK(hipMalloc((void **)&c->d_fold_claim, 8));
        HIPCHK(hipMemsetAsync(c->d_fold_claim, 0, 8, c->compute));
        dp.fold_pre = ps.pre.p; dp.fold_post = ps.post.p; dp.fold_claim = c->d_fold_claim;
        dp.fold_dst_pre = c->d_counters + c->lay.pre_comp; dp.fold_dst_post = c->d_counters + c->lay.post_comp;
    }
    const TrimArgs a{s.seq, s.qual, s.off, n, s.max_len, d_sl, d_hit, s.tn, s.res, rs.pre.p, rs.post.p, c->d_counters, c->d_err, c->n_cu, c->compute};
    HIPCHK(long_reads ? faqcs_launch_trim_long(plan, dp, a)
                      : plan.kernel == TrimKernel::trim_lds ? faqcs_launch_trim_lds(plan, dp, a) : faqcs_launch_trim_filter_accumulate(plan, dp, a));
    HIPCHK(hipEventRecord(t.b, c->compute));
    c->trim_kernel = trim_kernel_name(plan.kernel);
    if (c->pending_fold >= 0) { // ... else composition_histogram folds them on the aux stream, beside this launch
        if (!plan.folds_tail) {
            faqcs_ctx::RecSet &ps = c->rec[c->pending_fold];
            HIPCHK(hipStreamWaitEvent(c->aux, ps.trimmed, 0));
            HIPCHK(faqcs_launch_composition(ps.pre.p, ps.post.p, c->pending_n, c->pending_wide, c->d_norm, c->d_counters + c->lay.pre_comp,
                                            c->d_counters + c->lay.post_comp, c->n_cu, c->aux));
            HIPCHK(hipEventRecord(ps.folded, c->aux));
            ps.used = true;
            ++c->tally.folds_aux;
        } else ++c->tally.folds_tail;
        c->pending_fold = -1;
    }
    static const bool no_comp = [] { const char *e = getenv("FAQCS_DIAG_NO_COMPOSITION"); return e && atoi(e) != 0; }(); // (diagnostic, wrong composition tables: what the fold costs a step)
    if (!(c->dp.dbg & 1u) && !long_reads && !no_comp) {
        HIPCHK(hipEventRecord(rs.trimmed, c->compute));
        c->pending_fold = set; c->pending_n = n; c->pending_wide = plan.wide_records;
    }
    return 0;
}

// a submission on the compute stream: the adapter pre-pass, the trim launch, then its k-mers (faqcs_capi_kmer.hip)
static int enqueue(faqcs_ctx *c, const uint8_t *d_seq, const uint8_t *d_qual, const uint32_t *d_off, uint32_t n,
                   uint32_t max_len, const uint32_t *seg, uint32_t n_seg, faqcs_read_result *d_res, const uint8_t *d_tn = nullptr,
                   const uint32_t *host_off = nullptr)
{
    const Submission s{d_seq, d_qual, d_tn, d_off, seg, host_off, n, max_len, n_seg, d_res};
    if (int rc = check_kmers(c, s)) return rc;
    Timing *tm = nullptr;
    const bool adapters = s.n && c->prm.n_adapters;
    if (s.n) { if (int rc = take_timing(c, tm)) return rc; }
    if (adapters) { if (int rc = enqueue_adapter(c, *tm, s)) return rc; }
    if (s.n) { if (int rc = enqueue_trim(c, *tm, s, adapters ? c->s_sl.p : nullptr, adapters ? c->s_hit.p : nullptr)) return rc; }
    return enqueue_kmers(c, tm, s);
}

static int scan_offsets(const uint32_t *off, uint32_t n, uint32_t cap, uint32_t *max_len)
{
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return fail(FAQCS_E_INVAL, "faqcs_submit: offsets must be non-decreasing");
        const uint32_t l = off[i + 1] - off[i];
        m = l > m ? l : m;
    }
    if (m > cap) return fail(FAQCS_E_INVAL, "faqcs_submit: read longer than max_read_length");
    if (m > FAQCS_MAX_READ_LENGTH) return fail(FAQCS_E_INVAL, "faqcs_submit: reads longer than FAQCS_MAX_READ_LENGTH bases are not supported by the HIP kernels");
    *max_len = m;
    return 0;
}

static int check_segments(const faqcs_batch *b)
{
    if (!b || !b->offset) return fail(FAQCS_E_INVAL, "faqcs_submit: null batch");
    if (!b->segment_start || b->segment_start[0] != 0 || b->segment_start[b->n_segments] != b->n_reads)
        return fail(FAQCS_E_INVAL, "faqcs_submit: segment_start must span [0, n_reads]");
    for (uint32_t s = 0; s < b->n_segments; ++s)
        if (b->segment_start[s + 1] < b->segment_start[s]) return fail(FAQCS_E_INVAL, "faqcs_submit: segment_start must be non-decreasing");
    return 0;
}

extern "C" int faqcs_submit_async(faqcs_ctx *c, const faqcs_batch *b, faqcs_read_result *results, uint64_t *ticket)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = check_segments(b)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const uint32_t n = b->n_reads;
    uint32_t max_len = 0;
    if (int rc = scan_offsets(b->offset, n, c->prm.max_read_length, &max_len)) return rc;
    const uint32_t o0 = b->offset[0], o1 = b->offset[n];
    const size_t bytes = (size_t)(o1 - o0);
    faqcs_ctx::Slot &sl = c->slot[c->n_submits & 1];
    hipEvent_t tk = c->ticket_ev[c->n_submits & 7];
    if (c->n_submits >= 8) { HIPCHK(hipEventSynchronize(tk)); ++c->tally.ticket_ring_waits; } // the ticket ring is 8 deep
    // the slot may still feed the kernels of submission k-2: growing it (hipFree) needs them finished, reusing it
    // only needs the copy stream to wait for them
    if (sl.used) {
        if (bytes + FAQCS_ARENA_PAD_BEFORE + FAQCS_ARENA_PAD_AFTER > sl.seq.cap || (size_t)n + 1 > sl.off.cap || (b->terminal_n && (size_t)n + 64 > sl.tn.cap)) { HIPCHK(hipEventSynchronize(sl.done)); ++c->tally.slot_event_syncs; }
        else { HIPCHK(hipStreamWaitEvent(c->copy, sl.done, 0)); ++c->tally.slot_stream_waits; }
    }
    HIPCHK(sl.seq.reserve(bytes + FAQCS_ARENA_PAD_BEFORE + FAQCS_ARENA_PAD_AFTER)); HIPCHK(sl.qual.reserve(bytes + FAQCS_ARENA_PAD_BEFORE + FAQCS_ARENA_PAD_AFTER)); HIPCHK(sl.off.reserve((size_t)n + 1));
    if (b->terminal_n) HIPCHK(sl.tn.reserve((size_t)n + 64));
    if ((size_t)n + 1 > c->s_res.cap) HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(c->s_res.reserve((size_t)n + 1));
    // arena bytes land 16 bytes into the staging buffer; the kernels index with the ORIGINAL offsets
    if (bytes) {
        HIPCHK(hipMemcpyAsync(sl.seq.p + 16, b->seq + o0, bytes, hipMemcpyHostToDevice, c->copy));
        HIPCHK(hipMemcpyAsync(sl.qual.p + 16, b->qual + o0, bytes, hipMemcpyHostToDevice, c->copy));
    }
    HIPCHK(hipMemcpyAsync(sl.off.p, b->offset, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, c->copy));
    const uint8_t *d_tn = nullptr;
    if (b->terminal_n && n) { // the caller's parser has looked at the ends of each read: n more bytes instead of two scattered loads per read
        HIPCHK(hipMemcpyAsync(sl.tn.p, b->terminal_n, n, hipMemcpyHostToDevice, c->copy));
        d_tn = sl.tn.p;
    }
    HIPCHK(hipEventRecord(c->copied, c->copy));
    HIPCHK(hipStreamWaitEvent(c->compute, c->copied, 0));
    const uint8_t *d_seq = sl.seq.p + 16 - o0, *d_qual = sl.qual.p + 16 - o0;
    if (int rc = enqueue(c, d_seq, d_qual, sl.off.p, n, max_len, b->segment_start, b->n_segments, c->s_res.p, d_tn, b->offset)) return rc;
    if (n && results) HIPCHK(hipMemcpyAsync(results, c->s_res.p, (size_t)n * sizeof(faqcs_read_result), hipMemcpyDeviceToHost, c->compute));
    HIPCHK(hipEventRecord(sl.done, c->compute));
    HIPCHK(hipEventRecord(tk, c->compute));
    sl.used = true;
    if (ticket) *ticket = c->n_submits;
    ++c->n_submits;
    return 0;
}

extern "C" int faqcs_submit(faqcs_ctx *c, const faqcs_batch *b, faqcs_read_result *results)
{
    return faqcs_submit_async(c, b, results, nullptr);
}

extern "C" int faqcs_wait(faqcs_ctx *c, uint64_t ticket)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (ticket >= c->n_submits) return fail(FAQCS_E_INVAL, "faqcs_wait: unknown ticket");
    if (ticket + 8 < c->n_submits) return 0; // its event slot has been recycled: the submission finished long ago
    HIPCHK(hipEventSynchronize(c->ticket_ev[ticket & 7]));
    return 0;
}

extern "C" int faqcs_path_tallies_get(const faqcs_ctx *c, faqcs_path_tallies *out)
{
    if (!c || !out) return fail(FAQCS_E_INVAL, "faqcs_path_tallies_get: null argument");
    *out = c->tally;
    return 0;
}

extern "C" void *faqcs_host_alloc(size_t bytes)
{
    void *p = nullptr;
    // portable: a buffer is handed to whichever device context takes the next 32 768-read block (faqcs_mi --gpus N)
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) return nullptr;
    return p;
}

extern "C" void faqcs_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

extern "C" int faqcs_submit_device(faqcs_ctx *c, const faqcs_batch *b, faqcs_read_result *d_results)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (!b || !b->segment_start) return fail(FAQCS_E_INVAL, "faqcs_submit_device: null batch");
    HIPCHK(hipSetDevice(c->device));
    const uint32_t n = b->n_reads;
    // offsets live on the device: the caller vouches for max_read_length; pick the kernel from the ctx capacity
    uint32_t max_len = b->max_read_len ? b->max_read_len : c->prm.max_read_length;
    if (max_len > c->prm.max_read_length) return fail(FAQCS_E_INVAL, "faqcs_submit_device: max_read_len exceeds the context capacity");
    if (max_len > FAQCS_MAX_READ_LENGTH) return fail(FAQCS_E_INVAL, "faqcs_submit_device: reads longer than FAQCS_MAX_READ_LENGTH bases are not supported by the HIP kernels");
    if (!d_results) { HIPCHK(c->s_res.reserve((size_t)n + 1)); d_results = c->s_res.p; }
    return enqueue(c, b->seq, b->qual, b->offset, n, max_len, b->segment_start, b->n_segments, d_results, b->terminal_n);
}

extern "C" int faqcs_terminal_n_flags(int device_id, const uint8_t *d_seq, const uint32_t *d_offset, uint32_t n_reads, uint8_t *d_flags)
{
    if (!d_seq || !d_offset || !d_flags) return fail(FAQCS_E_INVAL, "null argument");
    if (device_id >= 0) HIPCHK(hipSetDevice(device_id));
    HIPCHK(faqcs_launch_terminal_n_flags(d_seq, d_offset, n_reads, d_flags, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

// the records of the last launch are folded now, on the compute stream (somebody is about to read, move or reset the counter block)
int fold_pending_now(faqcs_ctx *c)
{
    if (c->pending_fold < 0) return 0;
    faqcs_ctx::RecSet &ps = c->rec[c->pending_fold];
    HIPCHK(faqcs_launch_composition(ps.pre.p, ps.post.p, c->pending_n, c->pending_wide, c->d_norm, c->d_counters + c->lay.pre_comp,
                                    c->d_counters + c->lay.post_comp, c->n_cu, c->compute));
    c->pending_fold = -1;
    ++c->tally.folds_now;
    return 0;
}

extern "C" int faqcs_sync(faqcs_ctx *c)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->copy));
    if (int rc = fold_pending_now(c)) return rc;
    // (round 6: the k-mers waiting in the open group stay there -- they are counted when the pass ends, faqcs_kmer_end_table /
    // faqcs_kmer_finish_pass, or when a caller asks for the curve so far, faqcs_kmer_points / _totals / _epoch_counts: kmer_catch_up)
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipStreamSynchronize(c->aux));
    for (size_t i = 0; i < c->kg.flush_ev_used; ++i) { // group flushes (they run behind a later submission or here): part of the k-mer time
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->kg.flush_ev[i].first, c->kg.flush_ev[i].second) == hipSuccess) c->kmer_flush_ms += ms;
    }
    c->kg.flush_ev_used = 0;
    for (size_t i = 0; i < c->timing_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->timings[i].a, c->timings[i].b) == hipSuccess) { c->kernel_ms += ms; ++c->kernel_launches; }
        if (c->timings[i].kmer && hipEventElapsedTime(&ms, c->timings[i].k0, c->timings[i].k1) == hipSuccess) c->kmer_ms += ms;
        if (c->timings[i].adapter && hipEventElapsedTime(&ms, c->timings[i].p, c->timings[i].a) == hipSuccess) c->adapter_ms += ms;
    }
    c->timing_used = 0;
    if (int rc = resolve_points(c)) return rc;
    uint32_t e = 0;
    HIPCHK(hipMemcpy(&e, c->d_err, 4, hipMemcpyDeviceToHost));
    if (e & 1u) return fail(FAQCS_E_QUALITY, "fastq.h:quality_score: Found a quality score value that is greater than the maximum allowed quality score");
    if (e & 2u) return fail(FAQCS_E_BASE, "seq_overlap.cpp:na_to_bits: Unknown base!");
    if (e & 4u) return fail(FAQCS_E_INVAL, "faqcs: internal error, the trim kernel's LDS block does not start at address 0");
    if (c->kt.stats) {
        unsigned long long st[3];
        HIPCHK(hipMemcpy(st, c->kt.stats, 24, hipMemcpyDeviceToHost));
        // (bit 1: the sender staging of the multi-GPU exchange ran out of room for runs that did not fit their sub-regions -- an input whose minimizer changes
        // at almost every position makes more runs than the staging is sized for; not a full table: ADVICE r5)
        if (st[2] & 2ull) return fail(FAQCS_E_NOMEM, "faqcs: the k-mer exchange staging overflowed (more runs of k-mers per read than it is sized for): submit smaller batches");
        if (st[2]) return fail(FAQCS_E_KMER_FULL, "faqcs: device k-mer table is full (raise faqcs_params.kmer_table_slots)");
    }
    return 0;
}

extern "C" int faqcs_counters_device(faqcs_ctx *c, void **d_ptr, uint64_t *n_u64)
{
    if (!c || !d_ptr || !n_u64) return fail(FAQCS_E_INVAL, "null argument");
    *d_ptr = c->d_counters;
    *n_u64 = c->lay.total;
    return 0;
}

// The collective runs on a buffer the CALLER owns (e.g. a torch tensor that RCCL registers for IPC): export the block into it,
// all-reduce it, import the sum.  Both copies wait for the work submitted so far and return when the bytes have moved.
// (import: what is still to be folded belongs to the block that is being replaced... by its own sum: export came first)
static int counters_copy(faqcs_ctx *c, void *d_dst, const void *d_src)
{
    HIPCHK(hipSetDevice(c->device));
    if (int rc = fold_pending_now(c)) return rc;
    HIPCHK(hipStreamSynchronize(c->aux));
    HIPCHK(hipMemcpyAsync(d_dst, d_src, c->lay.total * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    return 0;
}

extern "C" int faqcs_counters_export(faqcs_ctx *c, void *d_dst, uint64_t n_u64)
{
    if (!c || !d_dst || n_u64 < c->lay.total) return fail(FAQCS_E_INVAL, "faqcs_counters_export: buffer too small");
    return counters_copy(c, d_dst, c->d_counters);
}

extern "C" int faqcs_counters_import(faqcs_ctx *c, const void *d_src, uint64_t n_u64)
{
    if (!c || !d_src || n_u64 < c->lay.total) return fail(FAQCS_E_INVAL, "faqcs_counters_import: buffer too small");
    return counters_copy(c, c->d_counters, d_src);
}

extern "C" int faqcs_finish(faqcs_ctx *c, uint64_t *counters, uint64_t n_u64)
{
    if (!c || !counters || n_u64 < c->lay.total) return fail(FAQCS_E_INVAL, "faqcs_finish: counter buffer too small");
    if (int rc = faqcs_sync(c)) return rc;
    HIPCHK(hipMemcpy(counters, c->d_counters, c->lay.total * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int faqcs_reset_counters(faqcs_ctx *c)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    // (records that are still to be folded belong to the job that ends here: they are dropped with its block -- a caller reads the block first)
    if (c->pending_fold >= 0) ++c->tally.folds_dropped;
    c->pending_fold = -1;
    HIPCHK(hipStreamSynchronize(c->aux));
    HIPCHK(hipMemsetAsync(c->d_counters, 0, c->lay.total * sizeof(uint64_t), c->compute));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// measurement helpers
// ---------------------------------------------------------------------------------------------------------
static int synth_fill_impl(int device_id, uint8_t *d_seq, uint8_t *d_qual, uint32_t *d_offset, uint32_t n_reads, uint32_t L,
                           uint64_t seed, uint64_t first_read, float adapter_frac, uint64_t genome_len)
{
    if (device_id >= 0) HIPCHK(hipSetDevice(device_id));
    if ((uint64_t)n_reads * L + L > 0xffffffffull) return fail(FAQCS_E_INVAL, "faqcs_synth_fill: arena exceeds 32-bit offsets");
    const char *at = getenv("FAQCS_SYNTH_AT"); // (A+T fraction of the synthetic bases; unset: uniform ACGT)
    HIPCHK(faqcs_launch_synth(d_seq, d_qual, d_offset, n_reads, L, seed, first_read, adapter_frac, genome_len, at ? (float)atof(at) : -1.0f, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

extern "C" int faqcs_synth_fill(int device_id, uint8_t *d_seq, uint8_t *d_qual, uint32_t *d_offset, uint32_t n_reads,
                                uint32_t L, uint64_t seed, uint64_t first_read, float adapter_frac)
{
    return synth_fill_impl(device_id, d_seq, d_qual, d_offset, n_reads, L, seed, first_read, adapter_frac, 0);
}

extern "C" int faqcs_synth_fill_genome(int device_id, uint8_t *d_seq, uint8_t *d_qual, uint32_t *d_offset, uint32_t n_reads,
                                       uint32_t L, uint64_t seed, uint64_t first_read, uint64_t genome_len)
{
    if (genome_len <= L) return fail(FAQCS_E_INVAL, "faqcs_synth_fill_genome: the genome must be longer than a read");
    return synth_fill_impl(device_id, d_seq, d_qual, d_offset, n_reads, L, seed, first_read, 0.f, genome_len);
}

// Diagnostic builds only (-DFAQCS_LDS_STAMPS): the 16 u64 words the trim kernel accumulates its section clocks in; reads and clears them.
extern "C" int faqcs_debug_words(faqcs_ctx *c, uint64_t *out, uint32_t n)
{
    if (!c || !out || n > 16) return fail(FAQCS_E_INVAL, "faqcs_debug_words: bad argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipMemcpy(out, reinterpret_cast<const uint8_t *>(c->d_err) + 64, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(reinterpret_cast<uint8_t *>(c->d_err) + 64, 0, 128));
    return 0;
}

// Per-kernel averages since the last call of this or of faqcs_kernel_time_ms(): the trim kernel (with the name of the variant
// the last submission ran) and the adapter pre-pass (0 without adapters).  Resets the sums like faqcs_kernel_time_ms().
extern "C" int faqcs_kernel_report(faqcs_ctx *c, faqcs_kernel_times *out)
{
    if (!c || !out) return fail(FAQCS_E_INVAL, "null argument");
    if (int rc = faqcs_sync(c)) return rc;
    out->n_launches = c->kernel_launches;
    out->trim_ms = c->kernel_launches ? c->kernel_ms / (double)c->kernel_launches : 0.0;
    out->adapter_ms = c->kernel_launches ? c->adapter_ms / (double)c->kernel_launches : 0.0;
    out->trim_kernel = c->trim_kernel;
    out->kmer_ms = c->kernel_launches ? (c->kmer_ms + c->kmer_flush_ms) / (double)c->kernel_launches : 0.0;
    out->kmer_insert_ms = c->kernel_launches ? c->kmer_insert_ms / (double)c->kernel_launches : 0.0;
    c->kernel_ms = 0.0; c->adapter_ms = 0.0; c->kmer_ms = 0.0; c->kmer_insert_ms = 0.0; c->kmer_flush_ms = 0.0; c->kernel_launches = 0;
    return 0;
}

extern "C" int faqcs_kernel_time_ms(faqcs_ctx *c, double *avg_ms, uint64_t *n_launches)
{
    faqcs_kernel_times t;
    if (!c || !avg_ms || !n_launches) return fail(FAQCS_E_INVAL, "null argument");
    if (int rc = faqcs_kernel_report(c, &t)) return rc;
    *n_launches = t.n_launches; *avg_ms = t.trim_ms;
    return 0;
}
