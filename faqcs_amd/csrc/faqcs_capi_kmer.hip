// faqcs_capi_kmer.hip -- the k-mer side of the host code: the groups of the combine-before-insert counting (kg_*), the k-mer tail of a
// submission (enqueue_kmers: one of three, by the context's mode) and every faqcs_kmer_* entry point of include/faqcs_mi.h.
#include "faqcs_ctx.h"

// ---------------------------------------------------------------------------------------------------------
// combine-before-insert k-mer counting: host side (kernels: faqcs_kmer_skm_kernel.hip)
// ---------------------------------------------------------------------------------------------------------
// Sizes of the group buffers for a table of `slots` slots, k-mers of k bases and `free_b` bytes of free device memory (kg_init, and
// faqcs_kmer_memory_plan for a caller that wants to know before anything is allocated).
// Either scatter level writes 65 536 sub-regions: (bucket, writing block) at level 1, partitions at level 2.  An item is 16 bytes and
// holds a run of up to w k-mers, (w + 1) / 2 on average; the buffers are sized for three items per w + 1 occurrences (the bench's reads
// make one per 8), a level-1 sub-region for 1.25 x its even share, a partition -- minimizer bins vary more than hash bins do -- for
// 1.5 x.  What overflows is counted occurrence by occurrence (exact, slow).
// The item bound of a group.  Round 6: a pass that fits ONE group never reaches the table (faqcs_kmer.h), so a group is as large as the
// table's own sizing rule makes a pass -- six occurrences per slot: 0.6 distinct keys per slot at a coverage of 10 -- and the HBM
// allows: at most 60 % of what is free (the caller's batches are resident already in every use of this library).  2^31 slots:
// groups of 12.9 G occurrences, 44 + 53 GB of buffers next to the 36.5 GB table.
struct KgPlan { uint64_t G; uint32_t cap1, cap2; size_t l1_bytes, l2_bytes; };
static KgPlan kg_plan(uint64_t slots, uint32_t kmer, size_t free_b)
{
    const uint32_t w = kmer > 15 ? kmer - 14 : 1;
    KgPlan pl{};
    auto caps = [&](uint64_t G) {
        const double G_items = w == 1 ? (double)G : (double)G * 3.0 / (w + 1);
        const double mean = G_items / (KG_FAN * KG_FAN);
        pl.cap1 = (uint32_t)(mean * 1.25 + 8.0 * std::sqrt(mean) + 64.0);
        pl.cap2 = (uint32_t)(mean * 1.5 + 8.0 * std::sqrt(mean) + 64.0);
        if (pl.cap1 < (uint32_t)KG_MIN_CAP) pl.cap1 = KG_MIN_CAP;
        if (pl.cap2 < (uint32_t)KG_MIN_CAP) pl.cap2 = KG_MIN_CAP;
        pl.cap2 = (pl.cap2 + 7u) & ~7u; // (cut 2^F ways for the fine partitions of a pass counted at its end)
        pl.l1_bytes = (size_t)pl.cap1 * KG_FAN * KG_FAN * 16; pl.l2_bytes = (size_t)pl.cap2 * KG_FAN * KG_FAN * 16;
        return pl.l1_bytes + pl.l2_bytes;
    };
    uint64_t G = slots * 6;
    if (G < (1ull << 18)) G = 1ull << 18;
    if (G > (1ull << 36)) G = 1ull << 36;
    bool fixed = false;
    if (const char *e = getenv("FAQCS_KMER_GROUP_ITEMS")) { const uint64_t v = strtoull(e, nullptr, 0); if (v >= (1ull << 14) && v <= (1ull << 36)) { G = v; fixed = true; } }
    while (!fixed && G > (1ull << 18) && caps(G) > free_b / 10 * 6) G -= G / 4;
    (void)caps(G);
    pl.G = G;
    return pl;
}

// What a kmer_rarefaction context will hold on its device: out[0] the table (with its overflow area), out[1] / out[2] the level-1 / level-2
// group buffers, out[3] the occurrences a group takes (a pass below it is counted in one piece), out[4] the small arrays.  Host only.
extern "C" int faqcs_kmer_memory_plan(const faqcs_params *p, uint64_t free_bytes, uint64_t *out, uint32_t n_out)
{
    if (!p || !out || n_out < 5) return fail(FAQCS_E_INVAL, "faqcs_kmer_memory_plan: null argument / fewer than 5 words");
    for (uint32_t i = 0; i < n_out; ++i) out[i] = 0;
    if (!p->kmer_rarefaction) return 0;
    uint64_t slots = p->kmer_table_slots ? p->kmer_table_slots : (1ull << 28);
    uint64_t pow2 = 1; while (pow2 < slots) pow2 <<= 1;
    if (pow2 < (uint64_t)KG_SLICE_MIN << 16) pow2 = (uint64_t)KG_SLICE_MIN << 16;
    const uint64_t table = (pow2 + std::max<uint64_t>(pow2 >> 4, 1ull << 16)) * sizeof(KmerSlot);
    const KgPlan pl = kg_plan(pow2, p->kmer, free_bytes > table ? (size_t)(free_bytes - table) : 0);
    out[0] = table; out[1] = pl.l1_bytes; out[2] = pl.l2_bytes; out[3] = pl.G;
    out[4] = (uint64_t)KG_FAN * KG_FAN * 4 * 18 + (1u << 16) * 8 + (1u << 20) * 8 + (1ull << 19) / 8; // cursors, redo list, histogram of counts, dirty bits
    return 0;
}

static int kg_init(faqcs_ctx *c)
{
    faqcs_ctx::KmerGroup &g = c->kg;
    if (g.ready) return 0;
    const uint64_t slots = c->kt.mask + 1;
    KmerGroupDev &d = g.dev;
    g.skm = !g.direct; // (FAQCS_KMER_DIRECT=1 on an owner-partitioned context: round 3's pairs and per-pair atomics)
    g.skm_w = c->prm.kmer > 15 ? c->prm.kmer - 14 : 1;
    const size_t item_bytes = 16;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const KgPlan pl = kg_plan(slots, c->prm.kmer, free_b);
    const uint64_t G = pl.G;
    d.cap1 = pl.cap1; d.cap2 = pl.cap2;
    g.cap_items = G;
    d.split = 1u; // (a partition's items in one piece: skm_combine fetches them by index)
    d.cap2f = d.cap2 >> c->kt.fine;
    HIPCHK(hipMalloc((void **)&d.l1, (size_t)KG_FAN * KG_FAN * d.cap1 * item_bytes));
    HIPCHK(hipMalloc((void **)&d.l2, (size_t)KG_FAN * KG_FAN * d.cap2 * item_bytes));
    HIPCHK(hipMalloc((void **)&d.cur1, (size_t)KG_FAN * KG_FAN * 4));
    HIPCHK(hipMalloc((void **)&d.cur2, (size_t)KG_FAN * KG_FAN * 8 * 4)); // (up to 2^19 fine partitions)
    HIPCHK(hipMalloc((void **)&d.run_epoch, (size_t)KG_MAX_RUNS * 4));
    // histogram of counts of a pass counted at its end (the kernels add to it; faqcs_kmer_end_table reads it and starts it again)
    d.dense_n = 1u << 16; d.big_cap = 1u << 20;
    HIPCHK(hipMalloc((void **)&d.dense, (size_t)d.dense_n * 8)); HIPCHK(hipMalloc((void **)&d.big, (size_t)d.big_cap * 8)); HIPCHK(hipMalloc((void **)&d.n_big, 8));
    HIPCHK(hipMemsetAsync(d.dense, 0, (size_t)d.dense_n * 8, c->compute)); HIPCHK(hipMemsetAsync(d.n_big, 0, 8, c->compute));
    HIPCHK(hipMalloc((void **)&d.redo, ((size_t)KG_FAN * KG_FAN * 8 + 1) * 4));
    d.n_redo = d.redo + (size_t)KG_FAN * KG_FAN * 8;
    if (g.owner && c->part_world > 1) { // the partitions this rank owns, mapped onto [0, 2^19) (faqcs_kmer.h: part_mul)
        const uint32_t lo_b = (c->part_rank * 256u + c->part_world - 1u) / c->part_world, hi_b = ((c->part_rank + 1u) * 256u + c->part_world - 1u) / c->part_world;
        d.part_lo = lo_b << 11;
        d.part_mul = hi_b > lo_b ? (1ull << 51) / ((uint64_t)(hi_b - lo_b) << 11) : 0ull;
    }
    HIPCHK(faqcs_launch_skm_reset(d, c->compute));
    g.sub_fill.assign(KG_FAN, 0);
    g.ready = true;
    return 0;
}

// first_hist / tot_by_epoch hold at least `need` epochs (grown with their contents)
static int kg_ensure_epochs(faqcs_ctx *c, uint32_t need)
{
    faqcs_ctx::KmerGroup &g = c->kg;
    if (need > g.ep_used) g.ep_used = need;
    if (need <= g.ep_cap) return 0;
    const uint32_t cap = need + need / 2 + 4096;
    unsigned long long *f = nullptr, *t = nullptr;
    HIPCHK(hipMalloc((void **)&f, (size_t)cap * 8)); HIPCHK(hipMalloc((void **)&t, (size_t)cap * 8));
    HIPCHK(hipMemsetAsync(f, 0, (size_t)cap * 8, c->compute)); HIPCHK(hipMemsetAsync(t, 0, (size_t)cap * 8, c->compute));
    if (g.ep_cap) {
        HIPCHK(hipMemcpyAsync(f, g.dev.first_hist, (size_t)g.ep_cap * 8, hipMemcpyDeviceToDevice, c->compute));
        HIPCHK(hipMemcpyAsync(t, g.dev.tot_by_epoch, (size_t)g.ep_cap * 8, hipMemcpyDeviceToDevice, c->compute));
        HIPCHK(hipStreamSynchronize(c->compute)); // (kernels in flight hold the old pointers)
        (void)hipFree(g.dev.first_hist); (void)hipFree(g.dev.tot_by_epoch);
    }
    g.dev.first_hist = f; g.dev.tot_by_epoch = t; g.dev.n_epochs = cap; g.ep_cap = cap;
    return 0;
}

// FAQCS_KMER_DEBUG=1 (diagnostics): a flush step by step with the buffers checked on the host in between -- every level-1 item sits
// in the bucket of its partition's top 8 bits, every level-2 item in its partition, no item holds more than w k-mers; prints the
// item / occurrence / distinct-key counts and the fullest partition (the host expands the items with the kernels' own faqcs_skm.h)
static int kg_debug_flush(faqcs_ctx *c, bool final)
{
    faqcs_ctx::KmerGroup &g = c->kg;
    const KmerGroupDev &d = g.dev;
    const SkmGeom geo = skm_geom(c->prm.kmer);
    HIPCHK(hipStreamSynchronize(c->compute));
    // (final: the pass is counted in one piece -- 2^(16 + F) fine partitions of cap2f items instead of 65 536 of cap2)
    const uint32_t n_parts = final ? 1u << (16 + c->kt.fine) : (uint32_t)KG_FAN * KG_FAN, pcap = final ? d.cap2f : d.cap2;
    auto part_of = [&](unsigned long long w1) { return final ? skm_item_part(w1) >> (3 - c->kt.fine) : skm_item_p16(w1); };
    auto flush_stage = [&](uint32_t st) { return final ? faqcs_launch_skm_finish(d, c->kt, c->prm.kmer, c->n_cu, c->compute, st) : faqcs_launch_skm_flush(d, c->kt, c->prm.kmer, c->compute, st); };
    std::vector<uint32_t> cur1((size_t)KG_FAN * KG_FAN), cur2((size_t)n_parts);
    HIPCHK(hipMemcpy(cur1.data(), d.cur1, cur1.size() * 4, hipMemcpyDeviceToHost));
    unsigned long long st[3];
    HIPCHK(hipMemcpy(st, c->kt.stats, 24, hipMemcpyDeviceToHost));
    uint64_t n1 = 0, occ1 = 0, bad1 = 0, long1 = 0;
    std::vector<ulonglong2> buf(d.cap1);
    for (uint32_t b = 0; b < (uint32_t)KG_FAN; ++b)
        for (uint32_t s = 0; s < (uint32_t)KG_FAN; ++s) {
            const uint32_t n = cur1[(size_t)s * KG_FAN + b];
            if (!n) continue;
            if (n > d.cap1) { fprintf(stderr, "[kmer debug] level-1 cursor %u > cap %u (bucket %u, sub %u)\n", n, d.cap1, b, s); continue; }
            HIPCHK(hipMemcpy(buf.data(), reinterpret_cast<const ulonglong2 *>(d.l1) + ((size_t)b * KG_FAN + s) * d.cap1, (size_t)n * 16, hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < n; ++i) {
                ++n1; occ1 += skm_item_kmers(buf[i].y);
                if (skm_item_bucket(buf[i].y) != b) ++bad1;
                if (skm_item_kmers(buf[i].y) > geo.w || skm_item_run(buf[i].y) >= g.run_epoch.size()) ++long1;
            }
        }
    { uint32_t nb_used = 0, first_b = 0xffffffffu, last_b = 0, ns_used = 0;
      for (uint32_t b = 0; b < (uint32_t)KG_FAN; ++b) { uint64_t t = 0; for (uint32_t s2 = 0; s2 < (uint32_t)KG_FAN; ++s2) t += cur1[(size_t)s2 * KG_FAN + b]; if (t) { ++nb_used; first_b = std::min(first_b, b); last_b = b; } }
      for (uint32_t s2 = 0; s2 < (uint32_t)KG_FAN; ++s2) { uint64_t t = 0; for (uint32_t b = 0; b < (uint32_t)KG_FAN; ++b) t += cur1[(size_t)s2 * KG_FAN + b]; if (t) ++ns_used; }
      fprintf(stderr, "[kmer debug] cap1 %u cap2 %u split %u runs %zu; buckets in use %u (%u .. %u), sub-regions in use %u\n", d.cap1, d.cap2, d.split, g.run_epoch.size(), nb_used, first_b, last_b, ns_used); }
    if (g.defer.p) { uint32_t nd = 0; HIPCHK(hipMemcpy(&nd, g.defer.p, 4, hipMemcpyDeviceToHost)); std::vector<uint32_t> dl(std::min<uint32_t>(nd, 8)); if (!dl.empty()) HIPCHK(hipMemcpy(dl.data(), g.defer.p + 1, dl.size() * 4, hipMemcpyDeviceToHost));
                     fprintf(stderr, "[kmer debug] the last 16-positions launch left %u reads to the general kernel:", nd); for (uint32_t v : dl) fprintf(stderr, " %u", v); fprintf(stderr, "\n"); }
    fprintf(stderr, "[kmer debug] before the flush: %llu level-1 items, %llu occurrences, %llu in a wrong bucket, %llu with a bad length / run; overflow flag %llu, total %llu\n",
            (unsigned long long)n1, (unsigned long long)occ1, (unsigned long long)bad1, (unsigned long long)long1, st[2], st[1]);
    HIPCHK(flush_stage(1u));
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipMemcpy(cur2.data(), d.cur2, cur2.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(st, c->kt.stats, 24, hipMemcpyDeviceToHost));
    uint64_t n2 = 0, occ2 = 0, bad2 = 0, max_keys = 0, max_items = 0, distinct = 0;
    buf.resize((size_t)pcap);
    std::vector<unsigned long long> keys;
    for (uint32_t p = 0; p < n_parts; ++p) {
        const uint32_t np = cur2[p];
        if (!np) continue;
        HIPCHK(hipMemcpy(buf.data(), reinterpret_cast<const ulonglong2 *>(d.l2) + (size_t)p * pcap, buf.size() * 16, hipMemcpyDeviceToHost));
        keys.clear();
        for (uint32_t j = 0; j < 1; ++j)
            for (uint32_t i = 0; i < np && i < pcap; ++i) {
                const ulonglong2 it = buf[i];
                ++n2; occ2 += skm_item_kmers(it.y);
                if (part_of(it.y) != p) ++bad2;
                SkmRoll r = skm_roll_begin(it.x, it.y, geo);
                for (uint32_t t = 0; t < skm_item_kmers(it.y) && t < 32; ++t) { keys.push_back(skm_mix62(skm_roll_key(r))); skm_roll_next(r, geo); }
            }
        std::sort(keys.begin(), keys.end());
        const uint64_t nd = (uint64_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
        distinct += nd;
        max_keys = std::max<uint64_t>(max_keys, nd); max_items = std::max<uint64_t>(max_items, np);
    }
    fprintf(stderr, "[kmer debug] after the split: %llu level-2 items, %llu occurrences, %llu in a wrong partition; %llu distinct keys in this group, fullest partition %llu keys / %llu items (slice: %llu slots); overflow flag %llu\n",
            (unsigned long long)n2, (unsigned long long)occ2, (unsigned long long)bad2, (unsigned long long)distinct, (unsigned long long)max_keys, (unsigned long long)max_items,
            (unsigned long long)((c->kt.mask + 1) >> (final ? 16 + c->kt.fine : 16)), st[2]);
    HIPCHK(flush_stage(2u));
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipMemcpy(st, c->kt.stats, 24, hipMemcpyDeviceToHost));
    fprintf(stderr, "[kmer debug] after the %s: overflow flag %llu\n", final ? "count (the pass in one piece)" : "combine", st[2]);
    HIPCHK(flush_stage(4u));
    return 0;
}

// the open group's items are counted: level-2 scatter, combine, cursors back to zero (all on the compute stream).
// final == false: into the table, while the pass goes on (the group buffers are full, or a caller asks for the curve so far);
// final == true: the pass ends with this group and no group of it has gone into the table -- counted in one piece, the table untouched.
// (timed: a flush outside a submission's k0 .. k1 events brings its own pair)
static int kg_flush(faqcs_ctx *c, bool timed = false, bool final = false)
{
    faqcs_ctx::KmerGroup &g = c->kg;
    if (!g.ready || g.run_epoch.empty()) return 0;
    std::vector<uint32_t> &up = g.upload[g.n_flushes++ & 1]; // (kept alive past the asynchronous copy)
    up = g.run_epoch;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    if (timed) {
        if (g.flush_ev_used == g.flush_ev.size()) {
            hipEvent_t a, b; HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
            g.flush_ev.emplace_back(a, b);
        }
        ev = g.flush_ev[g.flush_ev_used++];
        HIPCHK(hipEventRecord(ev.first, c->compute));
    }
    HIPCHK(hipMemcpyAsync(g.dev.run_epoch, up.data(), up.size() * 4, hipMemcpyHostToDevice, c->compute));
    g.dev.n_runs = (uint32_t)up.size(); g.dev.epoch_base = g.epoch_base;
    const char *dbg = getenv("FAQCS_KMER_DEBUG"); // (read at every flush: a test turns it on for one engine)
    const bool debug = dbg && atoi(dbg) != 0;
    const char *e_final = getenv("FAQCS_KMER_FINAL"); // (0: round 5's path for every group -- A/B runs, and the tests of that path; read at every flush)
    final = final && !g.table_live && !(e_final && atoi(e_final) == 0);
    if (g.skm && debug) { if (int rc = kg_debug_flush(c, final)) return rc; }
    else if (final) HIPCHK(faqcs_launch_skm_finish(g.dev, c->kt, c->prm.kmer, c->n_cu, c->compute));
    else HIPCHK(faqcs_launch_skm_flush(g.dev, c->kt, c->prm.kmer, c->compute));
    if (!final) g.table_live = true;
    if (timed) HIPCHK(hipEventRecord(ev.second, c->compute));
    g.run_epoch.clear(); g.bound_items = 0;
    std::fill(g.sub_fill.begin(), g.sub_fill.end(), 0);
    return 0;
}

// skm_extract16 -- four reads per wave and round -- takes a launch of 31-mers from reads of up to 256 bases; what it cannot take goes to
// the general kernel behind it (launch_extract).  FAQCS_KMER_EXTRACT16=0: the general kernel alone (A/B switch, latched)
static bool use_extract16(const faqcs_ctx *c, uint32_t max_len)
{
    static const bool no16 = [] { const char *e = getenv("FAQCS_KMER_EXTRACT16"); return e && atoi(e) == 0; }();
    return c->prm.kmer == 31 && max_len <= 256 && !no16;
}

// the super-k-mer items of reads [r0, r1) of a submission -- one run, one epoch -- are appended to the level-1 buffers of d.
// x16: skm_extract16 first, then skm_extract for the reads it listed in defer ([0]: how many, [1 ..]: the reads; r1 - r0 + 1 entries)
static int launch_extract(faqcs_ctx *c, const KmerGroupDev &d, bool x16, uint32_t *defer, uint32_t run, uint32_t rot, uint32_t epoch,
                          const Submission &s, uint32_t r0, uint32_t r1)
{
    if (!x16) {
        HIPCHK(faqcs_launch_skm_extract(c->dp, c->prm.kmer, d, c->kt, run, rot, epoch, s.seq, s.qual, s.off, r0, r1, s.res, c->n_cu, c->compute));
        return 0;
    }
    HIPCHK(hipMemsetAsync(defer, 0, 4, c->compute));
    HIPCHK(faqcs_launch_skm_extract16(c->dp, d, c->kt, run, rot, epoch, s.seq, s.qual, s.off, r0, r1, s.res, defer + 1, defer, c->n_cu, c->compute));
    HIPCHK(faqcs_launch_skm_extract(c->dp, c->prm.kmer, d, c->kt, run, rot, epoch, s.seq, s.qual, s.off, r0, r1, s.res, c->n_cu, c->compute,
                                    defer + 1, defer, faqcs_skm_grid16(r1 - r0, c->n_cu)));
    return 0;
}

// The sub-region rule of a group.  A launch runs on `grid` blocks; block i appends to sub-region (i + rot) % 256 of every bucket: a share
// 1 / (256 grid) of the launch's items each (hashing spreads a block's items over the buckets; the blocks take equal shares of the
// launch).  sub_fill[i] = the EXPECTED number of items in the sub-regions block slot i has written (its even share of every launch so
// far); what a sub-region may hold beyond that -- skew of the blocks' reads and of the buckets, 1/8, and the scatter of a sum of
// independent shares, eight standard deviations + a granule -- is added ONCE, to the sum (round 5 added 64 items per launch: a pass of
// 32 768-read submissions, 14 items per sub-region each, was flushed after 540 of them with its sub-regions a fifth full).  The group
// is flushed before a sub-region could overflow (an overflow would be exact too, but slow: kmer_insert_atomic).
static bool kg_over(const faqcs_ctx::KmerGroup &g, uint64_t mean) { return mean + mean / 8 + (uint64_t)(8.0 * std::sqrt((double)mean)) + 64 > g.dev.cap1; }
static uint64_t kg_share(uint32_t grid, uint64_t items) { return items / ((uint64_t)grid * KG_FAN) + 1; }

// a launch of `grid` blocks that writes at most `items` items holding at most `occ` occurrences: do its sub-regions and the group have room?
static bool kg_fits(const faqcs_ctx::KmerGroup &g, uint32_t grid, uint32_t rot, uint64_t items, uint64_t occ)
{
    for (uint32_t i = 0; i < grid; ++i) if (kg_over(g, g.sub_fill[(i + rot) % KG_FAN] + kg_share(grid, items))) return false;
    return g.bound_items + occ <= g.cap_items;
}

// ... and the launch has been issued
static void kg_account(faqcs_ctx::KmerGroup &g, uint32_t grid, uint32_t rot, uint64_t items, uint64_t occ)
{
    ++g.n_launches;
    g.bound_items += occ;
    for (uint32_t i = 0; i < grid; ++i) g.sub_fill[(i + rot) % KG_FAN] += kg_share(grid, items);
}

// the largest take in [0, n] that fits (what a take needs grows with it; the per-block share may not)
template <class N, class Fits> static N largest_prefix(N n, Fits fits)
{
    if (fits(n)) return n;
    N lo = 0, hi = n;
    while (lo < hi) { const N mid = lo + (hi - lo + 1) / 2; if (fits(mid)) lo = mid; else hi = mid - 1; }
    return lo;
}

// the k-mers of reads [r0, r1) of a submission -- one epoch -- join the open group.  The item bound is tight with the host copy of the
// offsets (an occurrence starts at a distinct base); otherwise per_read items bound every read.
static int kg_add_run(faqcs_ctx *c, const Submission &s, uint32_t r0, uint32_t r1, uint64_t per_read, uint32_t epoch)
{
    faqcs_ctx::KmerGroup &g = c->kg;
    if (g.pass_done) return fail(FAQCS_E_INVAL, "faqcs_submit: the k-mer pass has been counted (faqcs_kmer_finish_pass); faqcs_kmer_end_table starts the next one");
    if (int rc = kg_init(c)) return rc;
    if (int rc = kg_ensure_epochs(c, epoch + 1)) return rc;
    g.pass_used = true;
    if (per_read == 0) per_read = 1;
    const bool x16 = g.skm && use_extract16(c, s.max_len);
    while (r0 < r1) {
        // (round 6: an item carries its epoch RELATIVE TO THE GROUP'S FIRST directly -- the run -> epoch table of the group is the identity --, so a
        // group takes any number of extraction launches: faqcs_mi submits a launch per 32 768-read buffer, and a pass of more than 1 000 buffers
        // was cut into groups by the 10-bit run field alone.  What is left is the span of epochs an LDS histogram of the counting kernels takes.)
        if (!g.run_epoch.empty() && epoch - g.epoch_base >= (uint32_t)KG_EPOCH_SPAN) {
            if (int rc = kg_flush(c)) return rc;
        }
        const uint32_t run = g.run_epoch.empty() ? 0u : epoch - g.epoch_base, rot = (uint32_t)((g.n_launches * 37u) % KG_FAN);
        // items a launch can be expected to write at most (super-k-mers: three per w + 1 occurrences and two per read)
        auto items_of = [&](uint32_t take, uint64_t bound) { return !g.skm || g.skm_w == 1 ? bound : bound * 3 / (g.skm_w + 1) + 2ull * take; };
        auto grid_of = [&](uint32_t take) { return x16 ? faqcs_skm_grid16(take, c->n_cu) : faqcs_skm_grid(take, c->n_cu); };
        auto bound_of = [&](uint32_t take) { return s.host_off ? (uint64_t)(s.host_off[r0 + take] - s.host_off[r0]) : (uint64_t)take * per_read; };
        uint32_t take = largest_prefix(r1 - r0, [&](uint32_t t) { return kg_fits(g, grid_of(t), rot, items_of(t, bound_of(t)), bound_of(t)); });
        if (take == 0) {
            if (!g.run_epoch.empty()) { if (int rc = kg_flush(c)) return rc; continue; }
            take = 1; // (a read that no empty group has room for: whatever overflows is counted by the per-occurrence path)
        }
        if (g.run_epoch.empty()) g.epoch_base = epoch;
        if (x16 && (size_t)take + 1 > g.defer.cap) HIPCHK(g.defer.reserve((size_t)(r1 - r0) + 1));
        if (int rc = launch_extract(c, g.dev, x16, g.defer.p, run, rot, epoch, s, r0, r0 + take)) return rc;
        while (g.run_epoch.size() <= (size_t)run) g.run_epoch.push_back((uint32_t)g.run_epoch.size()); // (the identity, as long as the group's epochs span)
        kg_account(g, grid_of(take), rot, items_of(take, bound_of(take)), bound_of(take));
        r0 += take;
    }
    return 0;
}

// owner side of the multi-GPU exchange: n received items (device memory; their run fields hold absolute epochs) join the open group,
// whose run -> epoch table is the identity (at most KG_EPOCH_SPAN epochs: faqcs_kmer_partition sends a job with more through the
// (key, epoch) pairs of FAQCS_KMER_DIRECT instead)
static int kg_add_items(faqcs_ctx *c, const void *d_items, uint64_t n)
{
    faqcs_ctx::KmerGroup &g = c->kg;
    if (g.pass_done) return fail(FAQCS_E_INVAL, "faqcs_kmer_insert_device: the k-mer pass has been counted (faqcs_kmer_finish_pass); faqcs_kmer_end_table starts the next one");
    if (int rc = kg_init(c)) return rc;
    if (int rc = kg_ensure_epochs(c, c->n_epochs)) return rc;
    g.pass_used = true;
    const uint8_t *p = reinterpret_cast<const uint8_t *>(d_items);
    while (n) {
        const uint32_t rot = (uint32_t)((g.n_launches * 37u) % KG_FAN);
        // (an item holds up to skm_w occurrences: the group's bound counts occurrences, the sub-regions items)
        uint64_t take = largest_prefix(n, [&](uint64_t t) { return kg_fits(g, faqcs_skm_items_grid(t, c->n_cu), rot, t, t * g.skm_w); });
        if (take == 0) {
            if (g.bound_items) { if (int rc = kg_flush(c)) return rc; continue; }
            take = 1;
        }
        g.epoch_base = 0;
        HIPCHK(faqcs_launch_skm_items(g.dev, c->kt, c->prm.kmer, rot, p, take, c->n_cu, c->compute));
        if (g.run_epoch.empty()) { g.run_epoch.resize(c->n_epochs); for (uint32_t j = 0; j < c->n_epochs; ++j) g.run_epoch[j] = j; }
        kg_account(g, faqcs_skm_items_grid(take, c->n_cu), rot, take, take * g.skm_w);
        p += take * 16; n -= take;
    }
    return 0;
}

// (distinct, total) of the points that are not final yet, from the epoch histograms: distinct(point i) = keys whose first epoch
// is <= i, total(point i) = occurrences with epoch <= i (both arrays restart with the table, faqcs_kmer_end_table)
// the first n entries of the epoch histograms
static int kg_read_epochs(faqcs_ctx *c, size_t n, std::vector<unsigned long long> &f, std::vector<unsigned long long> &t)
{
    f.resize(n); t.resize(n);
    if (!n) return 0;
    HIPCHK(hipMemcpy(f.data(), c->kg.dev.first_hist, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(t.data(), c->kg.dev.tot_by_epoch, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

static int kg_resolve_points(faqcs_ctx *c)
{
    faqcs_ctx::KmerGroup &g = c->kg;
    if (!g.ready || c->points.size() <= g.points_final) return 0;
    std::vector<unsigned long long> f, t;
    if (int rc = kg_read_epochs(c, std::min<size_t>(c->points.size(), g.ep_used), f, t)) return rc;
    unsigned long long df = 0, dt = 0;
    for (size_t i = 0; i < c->points.size(); ++i) {
        if (i < f.size()) { df += f[i]; dt += t[i]; }
        if (i >= g.points_final) { c->points[i].distinct_kmer = df; c->points[i].total_kmer = dt; }
    }
    return 0;
}

static int kg_totals(faqcs_ctx *c, unsigned long long *distinct, unsigned long long *total)
{
    *distinct = *total = 0;
    if (!c->kg.ready) return 0;
    std::vector<unsigned long long> f, t;
    if (int rc = kg_read_epochs(c, c->kg.ep_used, f, t)) return rc;
    for (size_t i = 0; i < f.size(); ++i) { *distinct += f[i]; *total += t[i]; }
    return 0;
}

// the points whose snapshot of the table's running (distinct, total) is on the device get their values (FAQCS_KMER_DIRECT)
int resolve_points(faqcs_ctx *c)
{
    if (c->pending.empty()) return 0;
    std::vector<unsigned long long> h(c->n_snaps * 2);
    HIPCHK(hipMemcpy(h.data(), c->d_snaps, c->n_snaps * 16, hipMemcpyDeviceToHost));
    for (auto &pp : c->pending) {
        c->points[pp.point_index].distinct_kmer = h[2 * pp.snap_index];
        c->points[pp.point_index].total_kmer = h[2 * pp.snap_index + 1];
    }
    c->pending.clear();
    c->n_snaps = 0;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// the k-mer tail of a submission (behind its trim launch, on the compute stream)
// ---------------------------------------------------------------------------------------------------------
// fn(s, e) for every run of consecutive segments [s, e) with one epoch that holds reads (epoch 0xffffffff: not counted)
template <class F> static int for_each_epoch_run(const uint32_t *seg, uint32_t n_seg, const std::vector<uint32_t> &seg_epoch, F fn)
{
    for (uint32_t s = 0, e; s < n_seg; s = e) {
        for (e = s + 1; e < n_seg && seg_epoch[e] == seg_epoch[s]; ++e) {}
        if (seg_epoch[s] != 0xffffffffu && seg[e] > seg[s]) { if (int rc = fn(s, e)) return rc; }
    }
    return 0;
}

// What the k-mer tail of a submission refuses, asked BEFORE anything of the submission is enqueued: a refused submission leaves the context as
// it was -- its reads are not trimmed into the counter block, and no timing event of it is left half recorded (faqcs_sync asks for the time
// between k0 and k1: the error of an event that was never recorded stayed behind as HIP's last error and failed the NEXT submission's trim launch)
int check_kmers(faqcs_ctx *c, const Submission &s)
{
    if (!c->partitioned || !c->kmer_active || s.n == 0) return 0;
    if (c->seg_epoch.size() != s.n_seg) return fail(FAQCS_E_INVAL, "faqcs_submit: faqcs_kmer_set_epochs() must give one epoch per segment of the submission");
    if (c->kg.direct) return 0;
    size_t runs = 0;
    (void)for_each_epoch_run(s.seg, s.n_seg, c->seg_epoch, [&](uint32_t, uint32_t) -> int { ++runs; return 0; });
    if (runs > (size_t)KG_MAX_RUNS) return fail(FAQCS_E_INVAL, "faqcs_submit: more than 1000 runs of segments with one epoch in a submission");
    return 0;
}

// owner-partitioned mode: this shard's runs of k-mers (super-k-mer items) grouped by owner rank; the caller exchanges them
static int kmer_send_items(faqcs_ctx *c, Timing *tm, const Submission &s)
{
    const faqcs_params &p = c->prm;
    faqcs_ctx::KmerSend &ks = c->ks;
    const uint32_t w = p.kmer > 15 ? p.kmer - 14 : 1;
    const uint64_t occ = s.host_off ? (uint64_t)(s.host_off[s.n] - s.host_off[0]) : (uint64_t)s.n * (s.max_len >= p.kmer ? s.max_len - p.kmer + 1 : 1);
    const uint64_t ib = (w == 1 ? occ : occ * 3 / (w + 1)) + 2ull * s.n + 64; // items this submission can be expected to make at most
    // staging: a sub-region per (bucket, writing block) of twice its even share; whatever does not fit spills (room for all of it)
    const uint32_t cap1 = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(KG_MIN_CAP, 2 * ib / ((uint64_t)KG_FAN * KG_FAN) + 64), 0x7fffffffu);
    const uint32_t spill_cap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(2 * ib, occ + 64), 0x7fffffffu); // (the true bound is one run per occurrence)
    if ((size_t)KG_FAN * KG_FAN * cap1 > ks.l1.cap || spill_cap > ks.spill.cap) HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(ks.l1.reserve((size_t)KG_FAN * KG_FAN * cap1));
    HIPCHK(ks.spill.reserve(spill_cap));
    HIPCHK(ks.cur1.reserve((size_t)KG_FAN * KG_FAN + 64));
    HIPCHK(ks.run_epoch.reserve((size_t)KG_MAX_RUNS));
    HIPCHK(ks.scratch.reserve((size_t)KG_FAN * KG_FAN + 128));
    HIPCHK(ks.defer.reserve((size_t)s.n + 1));
    ks.spill_n = ks.cur1.p + (size_t)KG_FAN * KG_FAN;
    KmerGroupDev &d = ks.dev;
    d = KmerGroupDev{};
    d.l1 = reinterpret_cast<unsigned long long *>(ks.l1.p); d.cur1 = ks.cur1.p; d.run_epoch = ks.run_epoch.p; d.cap1 = cap1; d.split = 1;
    d.spill = reinterpret_cast<unsigned long long *>(ks.spill.p); d.spill_n = ks.spill_n; d.spill_cap = spill_cap;
    HIPCHK(hipMemsetAsync(ks.cur1.p, 0, ((size_t)KG_FAN * KG_FAN + 64) * 4, c->compute));
    if (tm) { HIPCHK(hipEventRecord(tm->k0, c->compute)); tm->kmer = true; }
    // one launch per run of segments with the same epoch; an item's run field (13 bits) indexes the submission's run -> epoch table
    std::vector<uint32_t> &run_epoch = c->kg.upload[c->kg.n_flushes++ & 1];
    run_epoch.clear();
    const bool x16 = use_extract16(c, s.max_len);
    if (int rc = for_each_epoch_run(s.seg, s.n_seg, c->seg_epoch, [&](uint32_t a, uint32_t e) -> int {
            if (run_epoch.size() >= (size_t)KG_MAX_RUNS) return fail(FAQCS_E_INVAL, "faqcs_submit: more than 1000 runs of segments with one epoch in a submission");
            const uint32_t run = (uint32_t)run_epoch.size(), rot = (run * 37u) % KG_FAN;
            if (int rc2 = launch_extract(c, d, x16, ks.defer.p, run, rot, c->seg_epoch[a], s, s.seg[a], s.seg[e])) return rc2;
            run_epoch.push_back(c->seg_epoch[a]);
            return 0;
        })) return rc;
    if (!run_epoch.empty()) HIPCHK(hipMemcpyAsync(ks.run_epoch.p, run_epoch.data(), run_epoch.size() * 4, hipMemcpyHostToDevice, c->compute));
    d.n_runs = (uint32_t)run_epoch.size(); d.epoch_base = 0;
    const size_t ob_need = (size_t)std::min<uint64_t>((uint64_t)KG_FAN * KG_FAN * cap1 + spill_cap, occ + 1);
    if (ob_need > c->ob_items.cap) HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(c->ob_items.reserve(ob_need));
    HIPCHK(faqcs_launch_skm_outbox(d, c->part_world, c->d_ob, ks.scratch.p, c->ob_items.p, c->compute));
    if (tm) HIPCHK(hipEventRecord(tm->k1, c->compute));
    return 0;
}

// owner-partitioned mode, FAQCS_KMER_DIRECT=1: round 3's form -- (key, epoch) pairs bucketed by owner in two passes, one atomic insert
// per pair on the owner
static int kmer_send_pairs(faqcs_ctx *c, Timing *tm, const Submission &s)
{
    const faqcs_params &p = c->prm;
    // an occurrence starts at a distinct base, so the arena size bounds the item count (host copy of the last offset
    // is not available for device-resident batches: use the per-read bound n * max_len)
    const size_t cap = (size_t)s.n * (size_t)(s.max_len > p.kmer ? s.max_len - p.kmer + 1 : 0) + 1;
    HIPCHK(c->ob_items.reserve(cap));
    // one launch per run of segments with the same epoch; the waves of all launches get consecutive rows of the
    // per-wave count / offset tables
    struct RunSpan { uint32_t s, e, wave_base; };
    std::vector<RunSpan> runs;
    uint32_t total_waves = 0;
    (void)for_each_epoch_run(s.seg, s.n_seg, c->seg_epoch, [&](uint32_t a, uint32_t e) -> int {
        runs.push_back({a, e, total_waves});
        total_waves += faqcs_kmer_extract_waves(s.seg[e] - s.seg[a], c->n_cu);
        return 0;
    });
    HIPCHK(c->ob_wave_count.reserve((size_t)total_waves * c->part_world + 1));
    HIPCHK(c->ob_wave_offset.reserve((size_t)total_waves * c->part_world + 1));
    KmerOutbox O{c->ob_items.p, c->d_ob, c->d_ob + c->part_world, c->d_ob + 2 * c->part_world, c->part_world,
                 c->ob_wave_count.p, c->ob_wave_offset.p, total_waves};
    HIPCHK(hipMemsetAsync(c->d_ob, 0, 3 * c->part_world * 8, c->compute));
    if (tm) { HIPCHK(hipEventRecord(tm->k0, c->compute)); tm->kmer = true; }
    for (int fill = 0; fill < 2; ++fill) {
        for (const RunSpan &r : runs)
            HIPCHK(faqcs_launch_kmer_extract(c->dp, p.kmer, O, fill != 0, s.seq, s.qual, s.off, s.seg[r.s], s.seg[r.e], s.res,
                                             c->seg_epoch[r.s], r.wave_base, c->n_cu, c->compute));
        if (!fill) HIPCHK(faqcs_launch_kmer_outbox_offsets(O, c->compute));
    }
    if (tm) HIPCHK(hipEventRecord(tm->k1, c->compute));
    return 0;
}

// single GPU: the rarefaction bookkeeping per reference trim() call (trim.cpp:157-185).  The k-mers of consecutive segments go to the
// device in ONE launch per run of segments that ends at a sampling point (or at the end of the batch / of the curve): only there does
// the order of insertion become observable.
static int kmer_rarefaction(faqcs_ctx *c, Timing *tm, const Submission &s)
{
    const faqcs_params &p = c->prm;
    uint32_t run_begin = s.seg[0];
    if (tm && c->kmer_active) { HIPCHK(hipEventRecord(tm->k0, c->compute)); tm->kmer = true; }
    const bool direct = c->kg.direct;
    const uint64_t per_read = s.max_len >= p.kmer ? (uint64_t)(s.max_len - p.kmer + 1) : 1;
    auto flush_run = [&](uint32_t run_end) -> int {
        if (run_end > run_begin) {
            if (direct) HIPCHK(faqcs_launch_kmer(c->dp, p.kmer, c->kt, s.seq, s.qual, s.off, run_begin, run_end, s.res, c->n_cu, c->compute));
            // the run's epoch: the index of the next sampling point (the first one that will include these occurrences)
            else if (int rc = kg_add_run(c, s, run_begin, run_end, per_read, (uint32_t)c->points.size())) return rc;
        }
        run_begin = run_end;
        return 0;
    };
    for (uint32_t k = 0; k < s.n_seg; ++k) {
        const uint32_t r0 = s.seg[k], r1 = s.seg[k + 1];
        if (!c->kmer_active) run_begin = r1; // (segments after the curve completed are not counted, trim.cpp:180-184)
        c->total_number += (r1 - r0);
        if (!c->kmer_active) continue;
        const uint64_t index = c->total_number / p.split_size;
        const size_t num_rarefaction = c->points.size();
        const bool new_point = index > num_rarefaction && num_rarefaction < p.num_subsample;
        if (k + 1 == s.n_seg || num_rarefaction >= p.num_subsample || new_point)
            if (int rc = flush_run(r1)) return rc;
        if (new_point) {
            faqcs_rarefaction pt{c->total_number, 0, 0};
            c->points.push_back(pt);
            if (direct) { // the table's running (distinct, total) in stream order
                if (c->n_snaps == c->snap_cap) { // drain the snapshots taken so far
                    HIPCHK(hipStreamSynchronize(c->compute));
                    if (int rc = resolve_points(c)) return rc;
                }
                HIPCHK(hipMemcpyAsync(c->d_snaps + 2 * c->n_snaps, c->kt.stats, 16, hipMemcpyDeviceToDevice, c->compute));
                c->pending.push_back({c->points.size() - 1, c->n_snaps});
                ++c->n_snaps;
            }
        }
        if (num_rarefaction >= p.num_subsample) c->kmer_active = 0; // trim.cpp:180-184
    }
    if (tm && tm->kmer) HIPCHK(hipEventRecord(tm->k1, c->compute));
    return 0;
}

// one of the three, by the context's mode
int enqueue_kmers(faqcs_ctx *c, Timing *tm, const Submission &s)
{
    if (!c->partitioned) return kmer_rarefaction(c, tm, s);
    if (!c->kmer_active || s.n == 0) {
        // nothing to send: the counts of the submission BEFORE this one must not be read again (faqcs_kmer_outbox_host listed its keys a second
        // time, faqcs_kmer_forward moved its items a second time)
        HIPCHK(hipMemsetAsync(c->d_ob, 0, (size_t)c->part_world * 8, c->compute));
        c->seg_epoch.clear();
        return 0;
    }
    if (c->seg_epoch.size() != s.n_seg) return fail(FAQCS_E_INVAL, "faqcs_submit: faqcs_kmer_set_epochs() must give one epoch per segment of the submission");
    if (int rc = c->kg.direct ? kmer_send_pairs(c, tm, s) : kmer_send_items(c, tm, s)) return rc;
    c->seg_epoch.clear();
    c->ob_fresh = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// k-mer rarefaction results
// ---------------------------------------------------------------------------------------------------------
extern "C" int faqcs_kmer_active(faqcs_ctx *c) { return c ? c->kmer_active : 0; }

// The curve so far: the open group is counted INTO THE TABLE (the pass goes on behind this call, so its keys have to live somewhere) and
// the points taken so far get their values.  Callers that only want the finished curve call faqcs_kmer_end_table() first -- the pass
// is then counted in one piece without the table -- and read the points afterwards.
static int kmer_catch_up(faqcs_ctx *c)
{
    if (int rc = faqcs_sync(c)) return rc;
    if (c->kg.ready && !c->kg.run_epoch.empty()) {
        if (int rc = kg_flush(c, true)) return rc;
        if (int rc = faqcs_sync(c)) return rc; // (the flush's time joins the k-mer time; the table-full flag)
    }
    return kg_resolve_points(c);
}

extern "C" int faqcs_kmer_points(faqcs_ctx *c, faqcs_rarefaction *out, uint32_t cap, uint32_t *n_points)
{
    if (!c || !n_points) return fail(FAQCS_E_INVAL, "null argument");
    if (int rc = kmer_catch_up(c)) return rc;
    *n_points = (uint32_t)c->points.size();
    for (uint32_t i = 0; out && i < cap && i < c->points.size(); ++i) out[i] = c->points[i];
    return 0;
}

// (distinct, total) of the pass in progress -- or, when nothing has been counted since faqcs_kmer_end_table(), of the pass that call finished
extern "C" int faqcs_kmer_totals(faqcs_ctx *c, uint64_t *distinct, uint64_t *total)
{
    if (!c || !distinct || !total) return fail(FAQCS_E_INVAL, "null argument");
    *distinct = *total = 0;
    if (!c->kt.stats) return 0;
    if (int rc = kmer_catch_up(c)) return rc;
    unsigned long long st[2];
    if ((c->partitioned && !c->kg.owner) || c->kg.direct) HIPCHK(hipMemcpy(st, c->kt.stats, 16, hipMemcpyDeviceToHost));
    else if (!c->kg.pass_used) { st[0] = c->kg.last_distinct; st[1] = c->kg.last_total; }
    else if (int rc = kg_totals(c, &st[0], &st[1])) return rc;
    *distinct = st[0]; *total = st[1];
    return 0;
}

// The pass ends: its open group is counted -- in one piece and without the table when no group of the pass has been flushed before
//  -- and the points get their final values.  Nothing can join the pass afterwards; faqcs_kmer_end_table()
// (which calls this) starts the next one.  Callers that read results other than the points before faqcs_kmer_end_table() -- the epoch
// histograms of an owner rank, faqcs_kmer_epoch_counts -- call it themselves.
extern "C" int faqcs_kmer_finish_pass(faqcs_ctx *c)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (!c->kt.stats) return 0;
    if (int rc = faqcs_sync(c)) return rc;
    faqcs_ctx::KmerGroup &g = c->kg;
    if (g.ready && !g.pass_done) {
        if (int rc = kg_flush(c, true, true)) return rc;
        g.pass_done = true;
        if (int rc = faqcs_sync(c)) return rc;
        // keys in the overflow area (a probe window of a slice was full) are not swept by the counting kernel
        unsigned long long st[4];
        HIPCHK(hipMemcpy(st, c->kt.stats, 32, hipMemcpyDeviceToHost));
        g.hist_in_table = g.table_live;
        g.hist_in_overflow = !g.table_live && st[3] != 0;
        const char *e_stats = getenv("FAQCS_KMER_STATS"); // (read at every pass: a test turns it on for one engine)
        if (e_stats && atoi(e_stats) != 0) { // (diagnostics: how the pass was counted)
            uint32_t n_redo = 0;
            if (g.dev.n_redo && !g.table_live) HIPCHK(hipMemcpy(&n_redo, g.dev.n_redo, 4, hipMemcpyDeviceToHost));
            fprintf(stderr, "[kmer stats] pass counted %s; %u of %u fine partitions through their table slices; %llu inserts into the overflow area; group bound %llu occurrences, cap1 %u cap2f %u\n",
                    g.table_live ? "through the table (a group was flushed before the pass ended)" : "in one piece", n_redo, 1u << (16 + c->kt.fine), st[3],
                    (unsigned long long)g.cap_items, g.dev.cap1, g.dev.cap2f);
        }
    }
    return kg_resolve_points(c);
}

extern "C" int faqcs_kmer_end_table(faqcs_ctx *c)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (!c->kt.stats) return 0;
    if (int rc = faqcs_kmer_finish_pass(c)) return rc;
    faqcs_ctx::KmerGroup &g = c->kg;
    const bool table_only = (c->partitioned && !g.owner) || g.direct; // (round 3's per-occurrence paths: everything is in the table)
    unsigned long long st[2] = {0, 0};
    if (table_only) HIPCHK(hipMemcpy(st, c->kt.stats, 16, hipMemcpyDeviceToHost));
    else if (int rc = kg_totals(c, &st[0], &st[1])) return rc;
    // ++kmer_frequency_histogram[count] for every key, FaQCs.cpp:518-521: what the counting kernel of a pass in one piece has added up
    // already (KmerGroupDev::dense / big), plus -- when keys of the pass live in the table -- a read-only pass over it
    const bool sweep = st[0] != 0 && (table_only || g.hist_in_table || g.hist_in_overflow);
    const bool ovf_only = !table_only && !g.hist_in_table; // (the slices are empty: only the area behind the table holds keys)
    if (st[0]) {
        const uint32_t DENSE = 1u << 16, BIGCAP = 1u << 20;
        unsigned long long *d_dense = g.dev.dense, *d_big = g.dev.big, *d_nbig = g.dev.n_big;
        const bool own = !d_dense; // (a context that never made a group: the per-occurrence paths)
        if (own) {
            HIPCHK(hipMalloc((void **)&d_dense, DENSE * 8)); HIPCHK(hipMalloc((void **)&d_big, (size_t)BIGCAP * 8)); HIPCHK(hipMalloc((void **)&d_nbig, 8));
            HIPCHK(hipMemsetAsync(d_dense, 0, DENSE * 8, c->compute)); HIPCHK(hipMemsetAsync(d_nbig, 0, 8, c->compute));
        }
        auto release = [&]() { if (own) { (void)hipFree(d_dense); (void)hipFree(d_big); (void)hipFree(d_nbig); } };
        // (a read-only pass, then kmer_table_init below: 13.5 ms on the bench's 2^31-slot table; one pass that also cleared the live
        // sectors -- scattered 64-byte stores between the reads -- took 17.5)
        if (sweep) HIPCHK(faqcs_launch_kmer_histogram(c->kt, d_dense, DENSE, d_big, d_nbig, BIGCAP, c->n_cu, c->compute, ovf_only));
        HIPCHK(hipStreamSynchronize(c->compute));
        std::vector<unsigned long long> dense(DENSE);
        unsigned long long nbig = 0;
        HIPCHK(hipMemcpy(dense.data(), d_dense, DENSE * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&nbig, d_nbig, 8, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < DENSE; ++i) if (dense[i]) c->kmer_hist[i] += dense[i];
        if (nbig > BIGCAP) { release(); return fail(FAQCS_E_NOMEM, "faqcs_kmer_end_table: too many k-mers with count >= 65536"); }
        if (nbig) {
            std::vector<unsigned long long> big(nbig);
            HIPCHK(hipMemcpy(big.data(), d_big, nbig * 8, hipMemcpyDeviceToHost));
            for (auto v : big) c->kmer_hist[v] += 1;
        }
        if (!own) { HIPCHK(hipMemsetAsync(d_dense, 0, DENSE * 8, c->compute)); HIPCHK(hipMemsetAsync(d_nbig, 0, 8, c->compute)); }
        release();
    }
    if (c->partitioned) { // the points belong to the driver (faqcs_kmer_epoch_counts); only the table restarts here
        HIPCHK(hipMemsetAsync(c->d_tot_by_epoch, 0, (size_t)c->n_epochs * 8, c->compute));
    } else if (c->kmer_active && c->points.empty()) { // FaQCs.cpp:523-537
        faqcs_rarefaction pt{c->total_number, st[0], st[1]};
        c->points.push_back(pt);
    }
    // the next pass starts on an empty table: a stream of stores over all of it only when this pass has put keys there
    if (sweep || (st[0] == 0 && (table_only || g.hist_in_table || g.hist_in_overflow))) HIPCHK(faqcs_launch_kmer_table_init(c->kt, c->n_cu, c->compute, ovf_only));
    HIPCHK(hipMemsetAsync(c->kt.stats, 0, 64, c->compute));
    HIPCHK(hipMemsetAsync(c->kt.dirty, 0, (size_t)(1u << (16 + c->kt.fine)) / 8, c->compute));
    g.last_distinct = st[0]; g.last_total = st[1];
    g.table_live = false; g.pass_done = false; g.pass_used = false; g.hist_in_table = false; g.hist_in_overflow = false;
    if (g.ready && g.ep_cap) { // the epoch histograms restart with the table; the points taken so far keep their values
        g.points_final = c->points.size();
        HIPCHK(hipMemsetAsync(g.dev.first_hist, 0, (size_t)g.ep_cap * 8, c->compute));
        HIPCHK(hipMemsetAsync(g.dev.tot_by_epoch, 0, (size_t)g.ep_cap * 8, c->compute));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// owner-partitioned k-mers across GPUs
// ---------------------------------------------------------------------------------------------------------
extern "C" int faqcs_kmer_partition(faqcs_ctx *c, uint32_t rank, uint32_t world, uint32_t n_epochs)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (!c->kt.slots) return fail(FAQCS_E_INVAL, "faqcs_kmer_partition: the context was created without kmer_rarefaction");
    if (world == 0 || world > 64 || rank >= world || n_epochs == 0) return fail(FAQCS_E_INVAL, "faqcs_kmer_partition: bad rank / world / n_epochs");
    if (c->n_submits || c->total_number || c->partitioned) return fail(FAQCS_E_INVAL, "faqcs_kmer_partition: must be the first call on a fresh context");
    HIPCHK(hipSetDevice(c->device));
    c->kt.partitioned = 1;
    HIPCHK(hipMalloc((void **)&c->d_ob, 3 * (size_t)world * 8));
    HIPCHK(hipMalloc((void **)&c->d_tot_by_epoch, (size_t)n_epochs * 8));
    HIPCHK(hipMalloc((void **)&c->d_first_hist, (size_t)n_epochs * 8));
    HIPCHK(hipMemset(c->d_tot_by_epoch, 0, (size_t)n_epochs * 8));
    c->partitioned = true; c->part_rank = rank; c->part_world = world; c->n_epochs = n_epochs;
    // what this rank receives -- super-k-mer items whose run field holds the absolute epoch, 13 bits -- joins the group buffers like a single
    // GPU's own runs.  FAQCS_KMER_DIRECT=1, or more sampling epochs than an item's 10-bit epoch field and a group's LDS histogram take
    // (KG_EPOCH_SPAN): round 3's (key, epoch) pairs -- 16 bytes per occurrence on the wire, one atomic per pair on the owner: exact, any --subset.
    if (n_epochs > (uint32_t)KG_EPOCH_SPAN) c->kg.direct = true;
    c->kg.owner = !c->kg.direct;
    return 0;
}

extern "C" int faqcs_kmer_set_epochs(faqcs_ctx *c, const uint32_t *segment_epoch, uint32_t n_segments)
{
    if (!c || (!segment_epoch && n_segments)) return fail(FAQCS_E_INVAL, "null argument");
    if (!c->partitioned) return fail(FAQCS_E_INVAL, "faqcs_kmer_set_epochs: call faqcs_kmer_partition first");
    for (uint32_t s = 0; s < n_segments; ++s)
        if (segment_epoch[s] != 0xffffffffu && segment_epoch[s] >= c->n_epochs) return fail(FAQCS_E_INVAL, "faqcs_kmer_set_epochs: epoch out of range");
    c->seg_epoch.assign(segment_epoch, segment_epoch + n_segments);
    return 0;
}

extern "C" int faqcs_kmer_outbox(faqcs_ctx *c, void **d_items, uint64_t *counts)
{
    if (!c || !d_items || !counts) return fail(FAQCS_E_INVAL, "null argument");
    if (!c->partitioned) return fail(FAQCS_E_INVAL, "faqcs_kmer_outbox: call faqcs_kmer_partition first");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->compute));
    std::vector<unsigned long long> h(c->part_world, 0ull);
    // (a second call without a submission in between -- a rank of a collective loop whose part of the input was empty -- has nothing to send:
    // the outbox of the submission before it has been handed out already)
    if (c->ob_fresh) HIPCHK(hipMemcpy(h.data(), c->d_ob, (size_t)c->part_world * 8, hipMemcpyDeviceToHost));
    c->ob_fresh = false;
    for (uint32_t d = 0; d < c->part_world; ++d) counts[d] = h[d];
    *d_items = c->ob_items.p;
    return 0;
}

// Host copy of the keys of the last submission's outbox (all destinations, in bucket order): what a single-process caller
// that keeps its own MAP<Word, size_t> (the reference's trim() seam, integration/trim_shim.cpp) merges per call.
extern "C" int faqcs_kmer_outbox_host(faqcs_ctx *c, uint64_t *keys, uint64_t cap, uint64_t *n_keys)
{
    if (!c || !n_keys) return fail(FAQCS_E_INVAL, "null argument");
    if (!c->partitioned) return fail(FAQCS_E_INVAL, "faqcs_kmer_outbox_host: call faqcs_kmer_partition first");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->compute));
    std::vector<unsigned long long> h(c->part_world);
    HIPCHK(hipMemcpy(h.data(), c->d_ob, (size_t)c->part_world * 8, hipMemcpyDeviceToHost));
    uint64_t n_items = 0;
    for (uint32_t d = 0; d < c->part_world; ++d) n_items += h[d];
    // the outbox holds runs of k-mers (faqcs_skm.h): the number of occurrences is the sum of their lengths, counted on the host
    uint64_t total = n_items;
    if (!c->kg.direct && n_items) {
        std::vector<unsigned long long> w1((size_t)n_items * 2);
        HIPCHK(hipMemcpy(w1.data(), c->ob_items.p, (size_t)n_items * 16, hipMemcpyDeviceToHost));
        total = 0;
        for (uint64_t i = 0; i < n_items; ++i) total += skm_item_kmers(w1[2 * i + 1]);
    }
    *n_keys = total;
    if (!keys || cap < total || total == 0) return 0;
    std::vector<unsigned long long> items((size_t)n_items * 2);
    HIPCHK(hipMemcpy(items.data(), c->ob_items.p, (size_t)n_items * 16, hipMemcpyDeviceToHost));
    if (c->kg.direct) { for (uint64_t i = 0; i < n_items; ++i) keys[i] = items[2 * i]; return 0; }
    const SkmGeom geo = skm_geom(c->prm.kmer);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n_items; ++i) {
        SkmRoll r = skm_roll_begin(items[2 * i], items[2 * i + 1], geo);
        for (uint32_t j = 0, nk = skm_item_kmers(items[2 * i + 1]); j < nk; ++j) { keys[at++] = skm_roll_key(r); skm_roll_next(r, geo); }
    }
    return 0;
}

// the received items join the owner's group buffers (or its table), enqueued on its compute stream
static int kmer_insert_enqueue(faqcs_ctx *c, const void *d_items, uint64_t n_items)
{
    if (c->kg.owner) return kg_add_items(c, d_items, n_items);
    HIPCHK(faqcs_launch_kmer_insert_items(c->kt, d_items, n_items, c->d_tot_by_epoch, c->n_epochs, c->n_cu, c->compute));
    return 0;
}

extern "C" int faqcs_kmer_insert_device(faqcs_ctx *c, const void *d_items, uint64_t n_items)
{
    if (!c || (!d_items && n_items)) return fail(FAQCS_E_INVAL, "null argument");
    if (!c->partitioned) return fail(FAQCS_E_INVAL, "faqcs_kmer_insert_device: call faqcs_kmer_partition first");
    HIPCHK(hipSetDevice(c->device));
    if (!c->ins_a) { HIPCHK(hipEventCreate(&c->ins_a)); HIPCHK(hipEventCreate(&c->ins_b)); }
    HIPCHK(hipEventRecord(c->ins_a, c->compute));
    if (int rc = kmer_insert_enqueue(c, d_items, n_items)) return rc;
    HIPCHK(hipEventRecord(c->ins_b, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute)); // the caller may recycle d_items as soon as this returns
    { float ms = 0.f; if (hipEventElapsedTime(&ms, c->ins_a, c->ins_b) == hipSuccess) c->kmer_insert_ms += ms; }
    return 0;
}

// In-process form of the exchange (one process driving several devices: faqcs_mi --gpus N --kmer_rarefaction): the last submission's
// outbox of `from` goes to the owner contexts -- owners[r] = the context of rank r -- and is inserted there.  Same device: the
// owner reads the outbox in place; another device: a peer copy into the owner's staging buffer first.
extern "C" int faqcs_kmer_forward(faqcs_ctx *from, faqcs_ctx *const *owners, uint32_t world)
{
    if (!from || !owners) return fail(FAQCS_E_INVAL, "null argument");
    if (!from->partitioned || world != from->part_world) return fail(FAQCS_E_INVAL, "faqcs_kmer_forward: the context is not partitioned over `world` ranks");
    for (uint32_t r = 0; r < world; ++r)
        if (!owners[r] || !owners[r]->partitioned || owners[r]->part_rank != r || owners[r]->part_world != world)
            return fail(FAQCS_E_INVAL, "faqcs_kmer_forward: owners[r] must be the context of rank r");
    HIPCHK(hipSetDevice(from->device));
    HIPCHK(hipStreamSynchronize(from->compute));
    std::vector<unsigned long long> cnt(world);
    HIPCHK(hipMemcpy(cnt.data(), from->d_ob, (size_t)world * 8, hipMemcpyDeviceToHost));
    // (FAQCS_KMER_FORCE_PEER_COPY=1: an owner on the SAME device is treated like one on another device -- its items go through hipMemcpyPeer into
    // its staging buffer -- so that the branch a multi-GPU node takes is exercised on a one-GPU box: tests/test_gpu_parity.py)
    const char *e_peer = getenv("FAQCS_KMER_FORCE_PEER_COPY");
    const bool force_peer = e_peer && atoi(e_peer) != 0;
    size_t at = 0;
    for (uint32_t r = 0; r < world; ++r) {
        const unsigned long long n = cnt[r];
        if (!n) continue;
        const ulonglong2 *src = from->ob_items.p + at;
        at += (size_t)n;
        faqcs_ctx *o = owners[r];
        if (o->device == from->device && !force_peer) { if (int rc = faqcs_kmer_insert_device(o, src, n)) return rc; continue; }
        HIPCHK(hipSetDevice(o->device));
        // Two staging buffers per owner.  The copy runs on the owner's COPY stream and waits (on the device) only for the insert that last read
        // this staging buffer; the owner's compute stream waits (on the device) for the copy before the insert; the host waits for the copy
        // alone -- the sender's outbox may be overwritten then --, not for what the owner's compute stream has queued (the forward
        // blocked on the owner's whole stream, one buffer late).
        const unsigned k = o->fwd_n++ & 1u;
        if (!o->fwd_free[k]) { HIPCHK(hipEventCreateWithFlags(&o->fwd_free[k], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&o->fwd_copied[k], hipEventDisableTiming)); }
        else HIPCHK(hipStreamWaitEvent(o->copy, o->fwd_free[k], 0));
        if ((size_t)n > o->fwd_items[k].cap) HIPCHK(hipEventSynchronize(o->fwd_free[k])); // (about to be reallocated: nothing may still read it)
        HIPCHK(o->fwd_items[k].reserve((size_t)n));
        HIPCHK(hipMemcpyPeerAsync(o->fwd_items[k].p, o->device, src, from->device, (size_t)n * 16, o->copy));
        HIPCHK(hipEventRecord(o->fwd_copied[k], o->copy));
        HIPCHK(hipStreamWaitEvent(o->compute, o->fwd_copied[k], 0));
        if (int rc = kmer_insert_enqueue(o, o->fwd_items[k].p, n)) return rc;
        HIPCHK(hipEventRecord(o->fwd_free[k], o->compute));
        HIPCHK(hipEventSynchronize(o->fwd_copied[k]));
        HIPCHK(hipSetDevice(from->device));
    }
    return 0;
}

extern "C" int faqcs_kmer_epoch_counts(faqcs_ctx *c, uint64_t *distinct_by_first_epoch, uint64_t *total_by_epoch, uint32_t cap)
{
    if (!c || !distinct_by_first_epoch || !total_by_epoch) return fail(FAQCS_E_INVAL, "null argument");
    if (!c->partitioned || cap < c->n_epochs) return fail(FAQCS_E_INVAL, "faqcs_kmer_epoch_counts: not partitioned / buffers too small");
    if (int rc = kmer_catch_up(c)) return rc; // (after faqcs_kmer_finish_pass: nothing is open; before it: the open group goes into the table)
    if (c->kg.owner) { // kept up to date by the combine kernel: no pass over the table
        for (uint32_t i = 0; i < c->n_epochs; ++i) { distinct_by_first_epoch[i] = 0; total_by_epoch[i] = 0; }
        if (c->kg.ready && c->kg.ep_cap) {
            HIPCHK(hipMemcpy(distinct_by_first_epoch, c->kg.dev.first_hist, (size_t)c->n_epochs * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(total_by_epoch, c->kg.dev.tot_by_epoch, (size_t)c->n_epochs * 8, hipMemcpyDeviceToHost));
        }
        return 0;
    }
    HIPCHK(hipMemsetAsync(c->d_first_hist, 0, (size_t)c->n_epochs * 8, c->compute));
    HIPCHK(faqcs_launch_kmer_first_epoch_histogram(c->kt, c->d_first_hist, c->n_epochs, c->n_cu, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    HIPCHK(hipMemcpy(distinct_by_first_epoch, c->d_first_hist, (size_t)c->n_epochs * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(total_by_epoch, c->d_tot_by_epoch, (size_t)c->n_epochs * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int faqcs_kmer_histogram(faqcs_ctx *c, uint64_t *count, uint64_t *nkeys, uint64_t cap, uint64_t *n_pairs)
{
    if (!c || !n_pairs) return fail(FAQCS_E_INVAL, "null argument");
    *n_pairs = c->kmer_hist.size();
    uint64_t i = 0;
    for (auto &kv : c->kmer_hist) {
        if (i >= cap || !count || !nkeys) break;
        count[i] = kv.first; nkeys[i] = kv.second; ++i;
    }
    return 0;
}
