// faqcs_ctx.h -- internal to the host side of libfaqcs_mi.so (never installed): the context every entry point of include/faqcs_mi.h works
// on, the launch functions of the kernel files, and the few host functions that cross the host side's translation units:
//   faqcs_host.cpp       host statements and helpers without HIP (faqcs_host.h)     faqcs_capi_seam.hip  emit / parse / render / pair / inflate / gunzip / deflate / detect
//   faqcs_capi.hip       create / destroy, submission, sync, counters, timing       faqcs_capi_comm.hip  RCCL
//   faqcs_capi_kmer.hip  k-mer groups, the k-mer tails of a submission, faqcs_kmer_*
// One faqcs_ctx == the (filter_stats, adapter_stats, PlotInfo, Options) quadruple the reference keeps in
// main() (FaQCs.cpp:67-69) plus the device state: a compute stream, a copy stream, device staging arenas,
// the additive u64 counter block, the adapter tables and the k-mer hash table.
// There is NO CPU implementation of the hot path in this library: without a HIP device faqcs_create() fails.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "faqcs_dev.h"
#include "faqcs_host.h"
#include "faqcs_kmer.h"
#include "faqcs_skm.h"

// kernels (other translation units)
struct AdapterDev { // (field by field in faqcs_adapter_kernel.hip)
    const uint8_t *bits;
    const uint32_t *start, *planes, *wstart;
    uint32_t n_adapters;
    float match_rate;
    uint32_t longest, plane_dwords, has_gap;
};
// the trim launchers, one per kernel file: each executes a TrimPlan (trim_plan(), faqcs_trim_plan.h) that names its kernel
hipError_t faqcs_launch_trim_lds(const TrimPlan &plan, const DevParams &P, const TrimArgs &a);
hipError_t faqcs_launch_trim_filter_accumulate(const TrimPlan &plan, const DevParams &P, const TrimArgs &a);
hipError_t faqcs_launch_trim_long(const TrimPlan &plan, const DevParams &P, const TrimArgs &a);
hipError_t faqcs_launch_terminal_n_flags(const uint8_t *seq, const uint32_t *off, uint32_t n_reads, uint8_t *flags, hipStream_t st);
hipError_t faqcs_launch_composition(const unsigned long long *rec_pre, const unsigned long long *rec_post, uint32_t n, bool wide,
                                    const float *comp_norm, uint64_t *dst_pre, uint64_t *dst_post, int n_cu, hipStream_t st);
hipError_t faqcs_launch_adapter(const AdapterDev &A, const AdapterGroup *G, const uint8_t *seq, const uint32_t *off, uint32_t n_reads,
                                uint32_t max_len, const uint32_t *seg_start, uint32_t n_segments, uint32_t *ad_sl,
                                uint16_t *ad_hit, uint64_t *adapter_stats, uint32_t *err, uint32_t dbg, int n_cu, hipStream_t st);
hipError_t faqcs_launch_synth(uint8_t *d_seq, uint8_t *d_qual, uint32_t *d_offset, uint32_t n_reads, uint32_t L,
                              uint64_t seed, uint64_t first_read, float adapter_frac, uint64_t genome_len, float at_frac, hipStream_t st);

size_t faqcs_emit_scratch_bytes(uint32_t n_reads);
hipError_t faqcs_launch_emit_scan(const uint8_t *seq, const uint32_t *off, const uint8_t *tn, uint32_t n_reads, const faqcs_read_result *res,
                                  const uint8_t *keep, const faqcs_emit_out *out, void *scratch, hipStream_t st);
hipError_t faqcs_launch_emit_gather(const uint8_t *seq, const uint8_t *qual, uint32_t n_reads, const faqcs_emit_out *out, const void *scratch,
                                    int in_off, int out_off, uint32_t replace_q, int n_cu, hipStream_t st);

size_t faqcs_parse_scratch_bytes(unsigned long long n_text);
hipError_t faqcs_launch_parse_index(const uint8_t *text, unsigned long long n_text, int final, void *scratch, hipStream_t st);
hipError_t faqcs_launch_parse_records(const uint8_t *text, unsigned long long n_text, const faqcs_parse_out *out, void *scratch, int n_cu, hipStream_t st);
hipError_t faqcs_launch_parse_gather(const uint8_t *text, unsigned long long n_text, const faqcs_parse_out *out, const void *scratch, int n_cu, hipStream_t st);

size_t faqcs_render_scratch_bytes(uint32_t n_reads);
hipError_t faqcs_launch_render_scan(const faqcs_batch *b, const faqcs_read_result *res, const uint32_t *def_pos, const uint32_t *def_len,
                                    const uint8_t *select, const uint32_t *order, const faqcs_render_out *out, void *scratch, hipStream_t st);
hipError_t faqcs_launch_render_gather(const faqcs_batch *b, bool trimmed, const uint8_t *text, const faqcs_render_out *out, const void *scratch,
                                      int in_off, int out_off, uint32_t replace_q, int n_cu, hipStream_t st);

// one mate of faqcs_pair_device / faqcs_render_pair_device, by value (faqcs_pair_kernel.hip)
struct MateDev {
    const uint8_t *seq, *qual, *tn, *text;
    const uint32_t *off, *def_pos, *def_len;
    const faqcs_read_result *res;
};
size_t faqcs_pair_scratch_bytes(uint32_t n_pairs);
hipError_t faqcs_launch_pair_check(const MateDev &m1, const MateDev &m2, uint32_t n_pairs, uint8_t *route, void *scratch, hipStream_t st);
hipError_t faqcs_launch_pair_finish(uint32_t n_pairs, bool routed, uint8_t *route, faqcs_pair_info *info, const void *scratch, int n_cu, hipStream_t st);
hipError_t faqcs_launch_render_pair_scan(int file, const MateDev &m1, const MateDev &m2, const uint8_t *route, uint32_t n_pairs, const faqcs_render_out *out,
                                         void *scratch, hipStream_t st);
hipError_t faqcs_launch_render_pair_gather(bool trimmed, const MateDev &m1, const MateDev &m2, uint32_t n_pairs, const faqcs_render_out *out, const void *scratch,
                                           int in_off, int out_off, uint32_t replace_q, int n_cu, hipStream_t st);

size_t faqcs_inflate_scratch_bytes(uint32_t n_members);
hipError_t faqcs_launch_inflate_scan(const uint8_t *comp, unsigned long long n_comp, const uint32_t *moff, uint32_t n, const faqcs_inflate_out *out, void *scratch, hipStream_t st);
hipError_t faqcs_launch_inflate_decode(const uint8_t *comp, const uint32_t *moff, uint32_t n, const faqcs_inflate_out *out, void *scratch, int n_cu, hipStream_t st);
hipError_t faqcs_launch_gunzip_count(const uint8_t *comp, uint32_t n_comp, uint32_t piece_bytes, void *recs, uint32_t n, int grid_mode, int n_cu, hipStream_t st);
hipError_t faqcs_launch_gunzip_decode(const uint8_t *comp, uint32_t n_comp, const void *chain, uint32_t n, uint16_t *sym, uint32_t *status, int n_cu, hipStream_t st);
hipError_t faqcs_launch_gunzip_resolve(const void *chain, uint32_t n, uint16_t *sym, uint32_t *bad, hipStream_t st);
hipError_t faqcs_launch_gunzip_narrow(const void *chain, const void *slices, uint32_t n_slices, const uint16_t *sym, uint8_t *text, uint32_t front, void *results, int n_cu,
                                      hipStream_t st);
hipError_t faqcs_launch_gunzip_window_load(const uint8_t *window, uint32_t window_bytes, uint16_t *sym, hipStream_t st);
hipError_t faqcs_launch_gunzip_window_save(const uint16_t *sym, const uint8_t *text, uint32_t take_old, uint32_t take_new, uint32_t text_end, uint8_t *window, hipStream_t st);
size_t faqcs_bgzf_index_scratch_bytes(unsigned long long n_comp);
hipError_t faqcs_launch_bgzf_index_candidates(const uint8_t *comp, unsigned long long n_comp, void *scratch, int n_cu, hipStream_t st);
hipError_t faqcs_launch_bgzf_index_chain(const uint8_t *comp, unsigned long long n_comp, int final, uint32_t *member_offset, uint32_t capacity, faqcs_bgzf_index_info *info,
                                         void *scratch, int n_cu, hipStream_t st);
size_t faqcs_deflate_scratch_bytes(uint32_t n, uint32_t n_data, uint32_t member_bytes, int n_cu);
hipError_t faqcs_launch_deflate_encode(const uint8_t *text, unsigned long long n_text, uint32_t member_bytes, uint32_t n, uint32_t n_data, int mode, void *scratch, int n_cu, hipStream_t st);
hipError_t faqcs_launch_deflate_gather(uint32_t member_bytes, uint32_t n, uint32_t n_data, const faqcs_deflate_out *out, void *scratch, int n_cu, hipStream_t st);

size_t faqcs_detect_scratch_bytes();
size_t faqcs_first_error_scratch_bytes(uint32_t n);
hipError_t faqcs_launch_detect(const uint8_t *qual, const uint32_t *off, uint32_t first, uint32_t count, const uint8_t *text, const uint32_t *def_pos,
                               const uint32_t *def_len, faqcs_detect_info *info, void *scratch, int n_cu, hipStream_t st);
hipError_t faqcs_launch_first_error(const faqcs_read_result *res, uint32_t n, faqcs_error_info *info, void *scratch, int n_cu, hipStream_t st);

#define HIPCHK(x)                                                                                         \
    do {                                                                                                  \
        hipError_t e_ = (x);                                                                              \
        if (e_ != hipSuccess)                                                                             \
            return fail(FAQCS_E_NODEVICE, std::string(#x) + ": " + hipGetErrorString(e_));                \
    } while (0)

struct faqcs_ctx;

#pragma GCC visibility push(hidden)

template <class T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0; // elements
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const size_t want = n + n / 4 + 64;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// p .. a: the adapter pre-pass (when there is one), a .. b: the trim kernel, k0 .. k1: the submission's k-mer kernels (kmer_count, or
// kmer_extract in the owner-partitioned mode)
struct Timing { hipEvent_t a, b, p, k0, k1; bool adapter, kmer; };

// What faqcs_emit_device / faqcs_parse_device / faqcs_render_device each keep on a context: the scratch of their kernels and the events
// around the two stages of the last call (faqcs_*_time_ms).  A stage is whatever is launched between two marks.
struct PackStage {
    DevBuf<uint4> scratch;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipStream_t st = nullptr;
    bool timed = false;
    int begin(faqcs_ctx *c, size_t scratch_bytes); // the scratch, and the mark in front of the first stage
    int mark(int i);                               // behind stage i (1, 2)
    int times(faqcs_ctx *c, const char *not_yet, double *first_ms, double *second_ms);
    void release();
};

// What faqcs_gunzip_device keeps on a context: the records of the pieces, the chain and the slices; one record for a forced start; the 16-bit
// symbols (2 bytes per text byte, and 64 KiB in front of them for the carried window of faqcs_gunzip_stream_device); the events around a
// pass and the three stage times of the last call of either kind (faqcs_gunzip_time_ms).
struct GunzipStage {
    DevBuf<uint4> rec, one, sym;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms[3] = {0.0, 0.0, 0.0}; // count, decode + narrow, resolve
    bool timed = false;
    void release() { rec.release(); one.release(); sym.release(); for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
};

#pragma GCC visibility pop

struct faqcs_ctx {
    faqcs_params prm;
    int device = 0, n_cu = 256;
    hipStream_t compute = nullptr, copy = nullptr;
    hipEvent_t copied = nullptr;
    DevParams dp;
    faqcs_layout lay;
    // device tables
    uint32_t *d_lcthr = nullptr, *d_magic = nullptr, *d_basetab = nullptr;
    int32_t *d_avgq = nullptr;
    float *d_norm = nullptr;
    uint64_t *d_counters = nullptr;
    uint32_t *d_err = nullptr;
    uint32_t *d_partials = nullptr;
    // adapters
    std::vector<std::string> adapters;
    uint8_t *d_abits = nullptr;
    uint32_t *d_astart = nullptr, *d_aplanes = nullptr, *d_awstart = nullptr;
    float match_rate = 0.f;
    uint32_t adapter_longest = 0, adapter_plane_dwords = 0;
    uint32_t adapter_has_gap = 0; // a target holds a '-': the base planes' counts bound nothing (AdapterDev::has_gap)
    // a library of more than FAQCS_ADAPTER_GROUP targets, or with a target of more than FAQCS_ADAPTER_SINGLE_LENGTH bases: consecutive groups
    // of targets, one adapter_overlap launch each, that carry every read's state in s_astate / s_amask (faqcs_dev.h); empty: one pass
    struct AdapterGroupHost { uint32_t j0, n, w0, longest, plane_dwords; };
    std::vector<AdapterGroupHost> agroups;
    uint32_t *d_awstart_grp = nullptr; // per group g, n + 1 word offsets rebased to the group's first plane word, from d_awstart_grp + j0 + g
    DevBuf<uint4> s_astate;
    DevBuf<uint64_t> s_amask;
    // staging for host submissions: two input slots so the H2D copy of batch k+1 overlaps the kernels of batch k
    struct Slot { DevBuf<uint8_t> seq, qual, tn; DevBuf<uint32_t> off; hipEvent_t done = nullptr; bool used = false; };
    Slot slot[2];
    uint64_t n_submits = 0;
    hipEvent_t ticket_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBuf<uint32_t> s_seg, s_sl;
    DevBuf<uint16_t> s_hit;
    DevBuf<faqcs_read_result> s_res;
    PackStage emit;   // the scan's tile sums and the 16-byte record of every emitted read | scan, gather
    PackStage parse;  // the line index, the record lengths and the two scans' tile sums | index + records, gather
    PackStage render; // the 32-byte descriptor and the text offset of every rendered record, the scan's tile sums | scan, gather
    PackStage pair;   // the partial of every tile of pairs (first mismatch, sums) | ids + route + partials, finishing block
    PackStage render_pair; // as render, over the 2 n_pairs candidates of the two mates | scan, gather
    PackStage inflate; // the header fields, the position and the status of every member, the scan's tile sums | scan, decode
    PackStage bgzf_index; // the candidates' positions, sizes, jump tables and ranks, the tiles' counts | candidates, chain
    PackStage deflate; // every member's slot, size and position, a block's tokens, the scan's tile sums | encode, gather
    GunzipStage gunzip; // faqcs_gunzip_device: see GunzipStage
    PackStage detect;  // faqcs_detect_device and faqcs_first_error_device: the partial (first hit) of every tile | only the scratch is used: the stage is not timed
    // per-read composition records (trim kernel -> composition_histogram).  Two sets: the histogram kernels of
    // submission k run on the aux stream next to the trim kernel of submission k+1 (LDS-bound next to VALU-bound).
    struct RecSet { DevBuf<unsigned long long> pre, post; hipEvent_t trimmed = nullptr, folded = nullptr; bool used = false; };
    RecSet rec[2];
    uint64_t n_enqueued = 0;
    // round 6: the records of a launch are folded one launch LATE -- by the next trim_lds launch's blocks as they run out of reads (DevParams::fold_*),
    // else by composition_histogram on the aux stream beside the next launch, or on the compute stream when somebody needs the counters
    int pending_fold = -1;         // the record set that still has to be folded (-1: none)
    uint32_t pending_n = 0;
    bool pending_wide = false;
    uint32_t *d_fold_claim = nullptr;
    hipStream_t aux = nullptr;
    // which arm of the host orchestration a call took, counted where the branch is taken (faqcs_path_tallies_get: a test asserts the arm it is about)
    faqcs_path_tallies tally{};
    // rarefaction state (trim.cpp:157-185): host-deterministic from read counts, values filled from the device
    uint64_t total_number = 0;
    int kmer_active = 0;
    std::vector<faqcs_rarefaction> points;
    struct PendingPoint { size_t point_index; size_t snap_index; };
    std::vector<PendingPoint> pending;
    KmerTable kt{nullptr, 0, nullptr, 0};
    // owner-partitioned multi-GPU k-mer mode (faqcs_kmer_partition)
    bool partitioned = false;
    uint32_t part_rank = 0, part_world = 1, n_epochs = 0;
    std::vector<uint32_t> seg_epoch;             // epochs of the NEXT submission's segments
    DevBuf<ulonglong2> ob_items;
    bool ob_fresh = false;                       // the outbox holds a submission that faqcs_kmer_outbox() has not handed out yet
    DevBuf<uint32_t> ob_wave_count;
    DevBuf<unsigned long long> ob_wave_offset;
    unsigned long long *d_ob = nullptr;          // [3 * world]: dest_count, dest_offset, dest_cursor
    unsigned long long *d_tot_by_epoch = nullptr, *d_first_hist = nullptr; // [n_epochs] each
    unsigned long long *d_snaps = nullptr; // [snap_cap][2]
    size_t snap_cap = 0, n_snaps = 0;
    std::map<uint64_t, uint64_t> kmer_hist; // PlotInfo::kmer_frequency_histogram
    // combine-before-insert k-mer counting (every context that is not owner-partitioned; faqcs_kmer_skm_kernel.hip): the
    // k-mers of a run of segments are appended to bucket buffers at submission time and reach the table group by group
    struct KmerGroup {
        bool ready = false;
        bool direct = false;          // FAQCS_KMER_DIRECT=1 (diagnostics): one atomic insert per occurrence (kmer_count), as in rounds 1-3
        bool owner = false;           // owner-partitioned context whose received pairs go through the group buffers too (n_epochs <= KG_EPOCH_SPAN)
        bool skm = false;             // 16-byte super-k-mer items (faqcs_kmer_skm_kernel.hip): every context that is not owner-partitioned
        uint32_t skm_w = 1;           // k-mers an item can hold (k - min(k, 15) + 1)
        DevBuf<uint32_t> defer;       // [0]: how many, [1 ..]: the reads skm_extract16 left to skm_extract (k = 31, reads of up to 256 bases)
        uint64_t cap_items = 0;       // item bound of a group
        uint64_t bound_items = 0;     // upper bound of the items the open group holds
        std::vector<uint32_t> run_epoch, upload[2]; // epochs (relative to epoch_base) of the open group's runs; host copies in flight
        unsigned n_flushes = 0;
        uint64_t n_launches = 0;      // (owner side) launches so far: rotates the sub-regions
        uint32_t epoch_base = 0;
        std::vector<uint64_t> sub_fill; // [256] upper bound of the items in the level-1 sub-regions written by block slot i
        KmerGroupDev dev{};           // (n_runs / epoch_base filled in at flush time)
        uint32_t ep_cap = 0;          // entries of dev.first_hist / dev.tot_by_epoch
        uint32_t ep_used = 0;         // 1 + largest epoch seen
        size_t points_final = 0;      // points whose (distinct, total) are final (resolved before the table restarted)
        std::vector<std::pair<hipEvent_t, hipEvent_t>> flush_ev; size_t flush_ev_used = 0;
        // round 6: a pass whose items fit the group buffers is counted in ONE piece when it ends (faqcs_kmer_finish_pass / faqcs_kmer_end_table)
        bool table_live = false;      // a group of this pass has been flushed into the table: its last group goes there too, and the table is swept
        bool pass_done = false;       // the pass has been counted (faqcs_kmer_finish_pass): nothing can join it; faqcs_kmer_end_table starts the next one
        bool pass_used = false;       // k-mers have joined the pass
        bool hist_in_table = false;   // the histogram of counts still has to be read off the table (table_live)
        bool hist_in_overflow = false; // ... off the overflow area behind it only (a pass counted in one piece whose slices' probe windows filled up)
        uint64_t last_distinct = 0, last_total = 0; // totals of the pass faqcs_kmer_end_table finished last
    } kg;
    // sender staging of the multi-GPU k-mer exchange (super-k-mer items of ONE submission, grouped by destination rank afterwards)
    struct KmerSend {
        KmerGroupDev dev{};
        DevBuf<ulonglong2> l1, spill;
        DevBuf<uint32_t> cur1, run_epoch, defer;
        DevBuf<unsigned long long> scratch;
        uint32_t *spill_n = nullptr;
    } ks;
    // kernel timing
    std::vector<Timing> timings;
    size_t timing_used = 0;
    double kernel_ms = 0.0, adapter_ms = 0.0, kmer_ms = 0.0, kmer_insert_ms = 0.0, kmer_flush_ms = 0.0;
    uint64_t kernel_launches = 0;
    hipEvent_t ins_a = nullptr, ins_b = nullptr;
    // faqcs_kmer_forward, owner side: two staging buffers for items that arrive by peer copy; [k]: the insert that read buffer k is done / the copy into it is
    DevBuf<ulonglong2> fwd_items[2];
    hipEvent_t fwd_free[2] = {nullptr, nullptr}, fwd_copied[2] = {nullptr, nullptr};
    unsigned fwd_n = 0;
    const char *trim_kernel = "";
    void *comm = nullptr;          // ncclComm_t (faqcs_comm_init / faqcs_comm_init_all)
    hipEvent_t comm_ev = nullptr;  // the aux stream's work (composition fold) before the collective
};

// The device view of one submission: seq / qual / off are device pointers valid for indices off[0] .. off[n], res a device result array,
// seg the host's segment starts; host_off (may be null) is the host copy of the offsets, tn (may be null) the terminal-N flags.
struct Submission {
    const uint8_t *seq, *qual, *tn;
    const uint32_t *off, *seg, *host_off;
    uint32_t n, max_len, n_seg;
    faqcs_read_result *res;
};

// host functions that cross translation units (file-local before the host side was split: none is exported)
FAQCS_HIDDEN int fold_pending_now(faqcs_ctx *c);                                   // faqcs_capi.hip
FAQCS_HIDDEN int enqueue_kmers(faqcs_ctx *c, Timing *tm, const Submission &s);     // faqcs_capi_kmer.hip: the k-mer tail of a submission
FAQCS_HIDDEN int check_kmers(faqcs_ctx *c, const Submission &s);                   // faqcs_capi_kmer.hip: what enqueue_kmers would refuse, before anything is enqueued
FAQCS_HIDDEN int resolve_points(faqcs_ctx *c);                                     // faqcs_capi_kmer.hip
FAQCS_HIDDEN void comm_release(void *comm);                                        // faqcs_capi_comm.hip (ncclCommDestroy)
