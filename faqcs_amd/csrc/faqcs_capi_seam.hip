// faqcs_capi_seam.hip -- the device seams of the C ABI (include/faqcs_mi.h): faqcs_emit_device, faqcs_parse_device, faqcs_render_device,
// faqcs_pair_device, faqcs_render_pair_device, faqcs_bgzf_index_device, faqcs_inflate_device and faqcs_deflate_device with their faqcs_*_time_ms, and the untimed
// faqcs_detect_device / faqcs_first_error_device.  Each of the timed ones is two stages of kernels between the marks of a
// PackStage; the host statements of the same rules, and the argument checks shared with them, are in faqcs_host.cpp.
// faqcs_gunzip_device is the one call that blocks: the walk of faqcs_gunzip.h runs here, on the host, between its passes.
#include "faqcs_ctx.h"
#include "faqcs_deflate.h"
#include "faqcs_gunzip.h"

int PackStage::begin(faqcs_ctx *c, size_t scratch_bytes)
{
    HIPCHK(hipSetDevice(c->device));
    st = c->compute;
    const size_t need = (scratch_bytes + sizeof(uint4) - 1) / sizeof(uint4);
    if (need > scratch.cap) HIPCHK(hipStreamSynchronize(st)); // (growing frees the scratch an earlier call may still read)
    HIPCHK(scratch.reserve(need));
    for (auto &e : ev) if (!e) HIPCHK(hipEventCreate(&e));
    return mark(0);
}

int PackStage::mark(int i)
{
    HIPCHK(hipEventRecord(ev[i], st));
    if (i == 2) timed = true;
    return 0;
}

int PackStage::times(faqcs_ctx *c, const char *not_yet, double *first_ms, double *second_ms)
{
    if (!timed) return fail(FAQCS_E_INVAL, not_yet);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(ev[2]));
    float ms[2] = {0.f, 0.f};
    for (int i = 0; i < 2; ++i) HIPCHK(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    *first_ms = ms[0]; *second_ms = ms[1];
    return 0;
}

// faqcs_*_time_ms: the two stages of the entry point's last call on the context
static int stage_times(faqcs_ctx *c, PackStage faqcs_ctx::*stage, const char *not_yet, double *first_ms, double *second_ms)
{
    if (!c || !first_ms || !second_ms) return fail(FAQCS_E_INVAL, "null argument");
    return (c->*stage).times(c, not_yet, first_ms, second_ms);
}

void PackStage::release()
{
    scratch.release();
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
}

extern "C" int faqcs_emit_device(faqcs_ctx *c, const faqcs_batch *b, const faqcs_read_result *d_results, const uint8_t *d_keep, const faqcs_emit_out *out)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (!b || !d_results || !out) return fail(FAQCS_E_INVAL, "faqcs_emit_device: null batch, results or output");
    if (!out->seq || !out->qual || !out->offset || !out->info) return fail(FAQCS_E_INVAL, "faqcs_emit_device: null output arena, offset or info");
    if (((uintptr_t)out->seq | (uintptr_t)out->qual) & 15u) return fail(FAQCS_E_INVAL, "faqcs_emit_device: the output arenas must be 16-byte aligned");
    const uint32_t n = b->n_reads;
    if (n && (!b->seq || !b->qual || !b->offset)) return fail(FAQCS_E_INVAL, "faqcs_emit_device: null batch arrays");
    if (int rc = c->emit.begin(c, faqcs_emit_scratch_bytes(n))) return rc;
    HIPCHK(faqcs_launch_emit_scan(b->seq, b->offset, b->terminal_n, n, d_results, d_keep, out, c->emit.scratch.p, c->compute));
    if (int rc = c->emit.mark(1)) return rc;
    HIPCHK(faqcs_launch_emit_gather(b->seq, b->qual, n, out, c->emit.scratch.p, c->prm.input_quality_offset, c->prm.output_quality_offset,
                                    c->prm.replace_to_N_q, c->n_cu, c->compute));
    return c->emit.mark(2);
}

extern "C" int faqcs_emit_time_ms(faqcs_ctx *c, double *scan_ms, double *gather_ms) { return stage_times(c, &faqcs_ctx::emit, "faqcs_emit_time_ms: no emission on this context yet", scan_ms, gather_ms); }

extern "C" int faqcs_parse_device(faqcs_ctx *c, const uint8_t *d_text, uint64_t n_text, int final, const faqcs_parse_out *out)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = parse_check_args("faqcs_parse_device", d_text, n_text, out)) return rc;
    if (int rc = c->parse.begin(c, faqcs_parse_scratch_bytes(n_text))) return rc;
    HIPCHK(faqcs_launch_parse_index(d_text, n_text, final ? 1 : 0, c->parse.scratch.p, c->compute));
    HIPCHK(faqcs_launch_parse_records(d_text, n_text, out, c->parse.scratch.p, c->n_cu, c->compute));
    if (int rc = c->parse.mark(1)) return rc;
    HIPCHK(faqcs_launch_parse_gather(d_text, n_text, out, c->parse.scratch.p, c->n_cu, c->compute));
    return c->parse.mark(2);
}

extern "C" int faqcs_parse_time_ms(faqcs_ctx *c, double *index_ms, double *gather_ms) { return stage_times(c, &faqcs_ctx::parse, "faqcs_parse_time_ms: no parse on this context yet", index_ms, gather_ms); }

extern "C" int faqcs_render_device(faqcs_ctx *c, const faqcs_batch *b, const faqcs_read_result *d_results, const uint8_t *d_text,
                                   const uint32_t *d_def_pos, const uint32_t *d_def_len, const uint8_t *d_select, const uint32_t *d_order,
                                   const faqcs_render_out *out)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = render_check_args("faqcs_render_device", b, d_text, d_def_pos, d_def_len, out)) return rc;
    const uint32_t n = b->n_reads;
    if (int rc = c->render.begin(c, faqcs_render_scratch_bytes(n))) return rc;
    HIPCHK(faqcs_launch_render_scan(b, d_results, d_def_pos, d_def_len, d_select, d_order, out, c->render.scratch.p, c->compute));
    if (int rc = c->render.mark(1)) return rc;
    HIPCHK(faqcs_launch_render_gather(b, d_results != nullptr, d_text, out, c->render.scratch.p, c->prm.input_quality_offset, c->prm.output_quality_offset,
                                      c->prm.replace_to_N_q, c->n_cu, c->compute));
    return c->render.mark(2);
}

extern "C" int faqcs_render_time_ms(faqcs_ctx *c, double *scan_ms, double *gather_ms) { return stage_times(c, &faqcs_ctx::render, "faqcs_render_time_ms: no rendering on this context yet", scan_ms, gather_ms); }

static MateDev device_view(const faqcs_mate *m) { const faqcs_batch *b = m->batch; return MateDev{b->seq, b->qual, b->terminal_n, m->text, b->offset, m->def_pos, m->def_len, m->results}; }

extern "C" int faqcs_pair_device(faqcs_ctx *c, const faqcs_mate *m1, const faqcs_mate *m2, uint8_t *d_route, faqcs_pair_info *d_info)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    uint32_t n = 0;
    if (int rc = pair_check_args("faqcs_pair_device", m1, m2, d_route, d_info, &n)) return rc;
    if (int rc = c->pair.begin(c, faqcs_pair_scratch_bytes(n))) return rc;
    HIPCHK(faqcs_launch_pair_check(device_view(m1), device_view(m2), n, d_route, c->pair.scratch.p, c->compute));
    if (int rc = c->pair.mark(1)) return rc;
    HIPCHK(faqcs_launch_pair_finish(n, m1->results != nullptr, d_route, d_info, c->pair.scratch.p, c->n_cu, c->compute));
    return c->pair.mark(2);
}

extern "C" int faqcs_pair_time_ms(faqcs_ctx *c, double *check_ms, double *finish_ms) { return stage_times(c, &faqcs_ctx::pair, "faqcs_pair_time_ms: no pairing on this context yet", check_ms, finish_ms); }

extern "C" int faqcs_render_pair_device(faqcs_ctx *c, int file, const faqcs_mate *m1, const faqcs_mate *m2, const uint8_t *d_route, uint32_t n_pairs,
                                        const faqcs_render_out *out)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = render_pair_check_args("faqcs_render_pair_device", file, m1, m2, d_route, n_pairs, out)) return rc;
    if (int rc = c->render_pair.begin(c, faqcs_render_scratch_bytes(2u * n_pairs))) return rc;
    const MateDev a = device_view(m1), b = device_view(m2);
    HIPCHK(faqcs_launch_render_pair_scan(file, a, b, d_route, n_pairs, out, c->render_pair.scratch.p, c->compute));
    if (int rc = c->render_pair.mark(1)) return rc;
    HIPCHK(faqcs_launch_render_pair_gather(file != FAQCS_FILE_DISCARD, a, b, n_pairs, out, c->render_pair.scratch.p, c->prm.input_quality_offset,
                                           c->prm.output_quality_offset, c->prm.replace_to_N_q, c->n_cu, c->compute));
    return c->render_pair.mark(2);
}

extern "C" int faqcs_render_pair_time_ms(faqcs_ctx *c, double *scan_ms, double *gather_ms) { return stage_times(c, &faqcs_ctx::render_pair, "faqcs_render_pair_time_ms: no paired rendering on this context yet", scan_ms, gather_ms); }

extern "C" int faqcs_bgzf_index_device(faqcs_ctx *c, const uint8_t *d_comp, uint64_t n_comp, int final, uint32_t *d_member_offset, uint32_t capacity_members,
                                       faqcs_bgzf_index_info *d_info)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = bgzf_index_check_args("faqcs_bgzf_index_device", d_comp, n_comp, d_member_offset, d_info)) return rc;
    if (int rc = c->bgzf_index.begin(c, faqcs_bgzf_index_scratch_bytes(n_comp))) return rc;
    HIPCHK(faqcs_launch_bgzf_index_candidates(d_comp, n_comp, c->bgzf_index.scratch.p, c->n_cu, c->compute));
    if (int rc = c->bgzf_index.mark(1)) return rc;
    HIPCHK(faqcs_launch_bgzf_index_chain(d_comp, n_comp, final ? 1 : 0, d_member_offset, capacity_members, d_info, c->bgzf_index.scratch.p, c->n_cu, c->compute));
    return c->bgzf_index.mark(2);
}

extern "C" int faqcs_bgzf_index_time_ms(faqcs_ctx *c, double *candidates_ms, double *chain_ms) { return stage_times(c, &faqcs_ctx::bgzf_index, "faqcs_bgzf_index_time_ms: no index on this context yet", candidates_ms, chain_ms); }

extern "C" int faqcs_inflate_device(faqcs_ctx *c, const uint8_t *d_comp, uint64_t n_comp, const uint32_t *d_member_offset, uint32_t n_members, const faqcs_inflate_out *out)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = inflate_check_args("faqcs_inflate_device", d_comp, n_comp, d_member_offset, n_members, out)) return rc;
    if (int rc = c->inflate.begin(c, faqcs_inflate_scratch_bytes(n_members))) return rc;
    HIPCHK(faqcs_launch_inflate_scan(d_comp, n_comp, d_member_offset, n_members, out, c->inflate.scratch.p, c->compute));
    if (int rc = c->inflate.mark(1)) return rc;
    HIPCHK(faqcs_launch_inflate_decode(d_comp, d_member_offset, n_members, out, c->inflate.scratch.p, c->n_cu, c->compute));
    return c->inflate.mark(2);
}

extern "C" int faqcs_inflate_time_ms(faqcs_ctx *c, double *scan_ms, double *decode_ms) { return stage_times(c, &faqcs_ctx::inflate, "faqcs_inflate_time_ms: no inflate on this context yet", scan_ms, decode_ms); }

// faqcs_gunzip_device's Backend of gunzip_run (faqcs_gunzip.h): the compressed bytes and the passes are on the device, the walk's few bytes
// per piece come back to the host.  Every step is followed by a wait, so the call blocks; a pass is timed between two events.
namespace {
struct GunzipDevice {
    faqcs_ctx *c;
    const uint8_t *comp;
    uint32_t n_comp, piece_bytes;
    uint8_t *text;
    uint8_t *window; // faqcs_gunzip_stream_device: the caller's 32 768 bytes in device memory
    int down(void *dst, const void *src, size_t n)
    {
        HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->compute));
        HIPCHK(hipStreamSynchronize(c->compute));
        return 0;
    }
    int begin() { HIPCHK(hipEventRecord(c->gunzip.ev[0], c->compute)); return 0; }
    int end(int stage)
    {
        float ms = 0.f;
        HIPCHK(hipEventRecord(c->gunzip.ev[1], c->compute));
        HIPCHK(hipEventSynchronize(c->gunzip.ev[1]));
        HIPCHK(hipEventElapsedTime(&ms, c->gunzip.ev[0], c->gunzip.ev[1]));
        c->gunzip.ms[stage] += ms;
        return 0;
    }
    int fetch(uint64_t p, uint32_t n, uint8_t *dst) { return down(dst, comp + p, n); }
    int count_grid(faqcs_gunzip::Piece *grid, uint32_t n_grid)
    {
        HIPCHK(c->gunzip.rec.reserve(2 * (size_t)n_grid));
        if (int rc = begin()) return rc;
        HIPCHK(faqcs_launch_gunzip_count(comp, n_comp, piece_bytes, c->gunzip.rec.p, n_grid, 1, c->n_cu, c->compute));
        if (int rc = end(0)) return rc;
        return down(grid, c->gunzip.rec.p, sizeof(faqcs_gunzip::Piece) * (size_t)n_grid);
    }
    int count_forced(faqcs_gunzip::Piece &pc)
    {
        HIPCHK(c->gunzip.one.reserve(2));
        HIPCHK(hipMemcpyAsync(c->gunzip.one.p, &pc, sizeof pc, hipMemcpyHostToDevice, c->compute));
        if (int rc = begin()) return rc;
        HIPCHK(faqcs_launch_gunzip_count(comp, n_comp, piece_bytes, c->gunzip.one.p, 1, 0, c->n_cu, c->compute));
        if (int rc = end(0)) return rc;
        return down(&pc, c->gunzip.one.p, sizeof pc);
    }
    int write(const std::vector<faqcs_gunzip::ChainPiece> &chain, const std::vector<faqcs_gunzip::MemberRec> &members, uint32_t front, uint32_t window_bytes,
              uint32_t total, std::vector<faqcs_gunzip::MemberResult> &res)
    {
        namespace gz = faqcs_gunzip;
        std::vector<gz::Slice> slices;
        gz::make_slices(chain, slices);
        const size_t n = chain.size(), ns = slices.size();
        auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
        const size_t o_slices = n * sizeof(gz::ChainPiece), o_dst = o_slices + ns * sizeof(gz::Slice), o_bad = o_dst + up(4 * n), o_res = o_bad + up(4 * n),
                     bytes = o_res + up(ns * sizeof(gz::SliceResult));
        HIPCHK(c->gunzip.rec.reserve(bytes / sizeof(uint4) + 1));
        HIPCHK(c->gunzip.sym.reserve((((size_t)front + total) * 2 + 15) / sizeof(uint4) + 1));
        uint8_t *base = (uint8_t *)c->gunzip.rec.p;
        uint16_t *sym = (uint16_t *)c->gunzip.sym.p;
        HIPCHK(hipMemcpyAsync(base, chain.data(), n * sizeof(gz::ChainPiece), hipMemcpyHostToDevice, c->compute));
        if (ns) HIPCHK(hipMemcpyAsync(base + o_slices, slices.data(), ns * sizeof(gz::Slice), hipMemcpyHostToDevice, c->compute));
        if (int rc = begin()) return rc;
        HIPCHK(faqcs_launch_gunzip_window_load(window, window_bytes, sym, c->compute));
        HIPCHK(faqcs_launch_gunzip_decode(comp, n_comp, base, (uint32_t)n, sym, (uint32_t *)(base + o_dst), c->n_cu, c->compute));
        if (int rc = end(1)) return rc;
        if (int rc = begin()) return rc;
        HIPCHK(faqcs_launch_gunzip_resolve(base, (uint32_t)n, sym, (uint32_t *)(base + o_bad), c->compute));
        if (int rc = end(2)) return rc;
        if (int rc = begin()) return rc;
        HIPCHK(faqcs_launch_gunzip_narrow(base, base + o_slices, (uint32_t)ns, sym, text, front, base + o_res, c->n_cu, c->compute));
        if (int rc = end(1)) return rc;
        std::vector<uint32_t> dst(n), bad(n);
        std::vector<gz::SliceResult> sres(ns + 1);
        if (int rc = down(dst.data(), base + o_dst, 4 * n)) return rc;
        if (int rc = down(bad.data(), base + o_bad, 4 * n)) return rc;
        if (ns) if (int rc = down(sres.data(), base + o_res, ns * sizeof(gz::SliceResult))) return rc;
        gz::fold_results(chain, members, slices, sres.data(), dst.data(), bad.data(), res);
        return 0;
    }
    int window_save(uint32_t take_old, uint32_t take_new, uint32_t text_end)
    {
        if (int rc = begin()) return rc;
        HIPCHK(faqcs_launch_gunzip_window_save((const uint16_t *)c->gunzip.sym.p, text, take_old, take_new, text_end, window, c->compute));
        return end(1);
    }
};
} // namespace

// both device entry points behind their argument checks; state == nullptr: the single call
static int gunzip_on_device(const char *who, faqcs_ctx *c, const uint8_t *d_comp, uint64_t n_comp, int final, uint32_t piece_bytes, uint32_t max_rounds,
                            faqcs_gunzip_state *state, const faqcs_gunzip_out *out)
{
    HIPCHK(hipSetDevice(c->device));
    for (auto &e : c->gunzip.ev) if (!e) HIPCHK(hipEventCreate(&e));
    c->gunzip.ms[0] = c->gunzip.ms[1] = c->gunzip.ms[2] = 0.0;
    c->gunzip.timed = false;
    GunzipDevice B{c, d_comp, (uint32_t)n_comp, piece_bytes ? piece_bytes : faqcs_gunzip::DEFAULT_PIECE, out->text, state ? state->window : nullptr};
    faqcs_gunzip::Info info;
    faqcs_gunzip::State st{};
    if (state) gunzip_state_in(state, &st);
    if (int rc = faqcs_gunzip::gunzip_run(B, n_comp, piece_bytes, max_rounds, out->capacity_bytes, info, state ? &st : nullptr, final != 0))
        return rc == faqcs_gunzip::E_RECORD ? fail(FAQCS_E_INVAL, std::string(who) + ": a piece record that no run produces") : rc;
    faqcs_gunzip_info h;
    gunzip_info_out(info, &h);
    HIPCHK(hipMemcpyAsync(out->info, &h, sizeof h, hipMemcpyHostToDevice, c->compute));
    HIPCHK(hipStreamSynchronize(c->compute));
    if (state) gunzip_state_out(st, state);
    c->gunzip.timed = true;
    return 0;
}

extern "C" int faqcs_gunzip_device(faqcs_ctx *c, const uint8_t *d_comp, uint64_t n_comp, uint32_t piece_bytes, uint32_t max_rounds, const faqcs_gunzip_out *out)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = gunzip_check_args("faqcs_gunzip_device", d_comp, n_comp, piece_bytes, out)) return rc;
    return gunzip_on_device("faqcs_gunzip_device", c, d_comp, n_comp, 1, piece_bytes, max_rounds, nullptr, out);
}

extern "C" int faqcs_gunzip_stream_device(faqcs_ctx *c, const uint8_t *d_comp, uint64_t n_comp, int final, uint32_t piece_bytes, uint32_t max_rounds,
                                          faqcs_gunzip_state *state, const faqcs_gunzip_out *out)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = gunzip_check_args("faqcs_gunzip_stream_device", d_comp, n_comp, piece_bytes, out)) return rc;
    if (int rc = gunzip_state_check_args("faqcs_gunzip_stream_device", state)) return rc;
    return gunzip_on_device("faqcs_gunzip_stream_device", c, d_comp, n_comp, final, piece_bytes, max_rounds, state, out);
}

extern "C" int faqcs_gunzip_time_ms(faqcs_ctx *c, double *count_ms, double *decode_ms, double *resolve_ms)
{
    if (!c || !count_ms || !decode_ms || !resolve_ms) return fail(FAQCS_E_INVAL, "null argument");
    if (!c->gunzip.timed) return fail(FAQCS_E_INVAL, "faqcs_gunzip_time_ms: no gunzip on this context yet");
    *count_ms = c->gunzip.ms[0]; *decode_ms = c->gunzip.ms[1]; *resolve_ms = c->gunzip.ms[2];
    return 0;
}

extern "C" int faqcs_deflate_device(faqcs_ctx *c, const uint8_t *d_text, uint64_t n_text, uint32_t member_bytes, int final, const faqcs_deflate_out *out)
{
    return faqcs_deflate_device_mode(c, d_text, n_text, member_bytes, final, FAQCS_DEFLATE_FAST, out);
}

extern "C" int faqcs_deflate_device_mode(faqcs_ctx *c, const uint8_t *d_text, uint64_t n_text, uint32_t member_bytes, int final, int mode, const faqcs_deflate_out *out)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = deflate_check_args("faqcs_deflate_device", d_text, n_text, member_bytes, final, mode, out)) return rc;
    const uint32_t mb = member_bytes ? member_bytes : (uint32_t)faqcs_deflate::MAX_TEXT;
    const uint32_t n_data = (uint32_t)((n_text + mb - 1) / mb), n = n_data + (final ? 1u : 0u);
    if (int rc = c->deflate.begin(c, faqcs_deflate_scratch_bytes(n, n_data, mb, c->n_cu))) return rc;
    HIPCHK(faqcs_launch_deflate_encode(d_text, n_text, mb, n, n_data, mode, c->deflate.scratch.p, c->n_cu, c->compute));
    if (int rc = c->deflate.mark(1)) return rc;
    HIPCHK(faqcs_launch_deflate_gather(mb, n, n_data, out, c->deflate.scratch.p, c->n_cu, c->compute));
    return c->deflate.mark(2);
}

extern "C" int faqcs_deflate_time_ms(faqcs_ctx *c, double *encode_ms, double *gather_ms) { return stage_times(c, &faqcs_ctx::deflate, "faqcs_deflate_time_ms: no deflate on this context yet", encode_ms, gather_ms); }

// The decisions around trim(): a scan over the tiles and the finishing block.  Not a throughput stage: no marks, no faqcs_*_time_ms.
extern "C" int faqcs_detect_device(faqcs_ctx *c, const faqcs_batch *b, uint32_t first, uint32_t count, const uint8_t *d_text, const uint32_t *d_def_pos,
                                   const uint32_t *d_def_len, faqcs_detect_info *d_info)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = detect_check_args("faqcs_detect_device", b, first, count, d_text, d_def_pos, d_def_len, d_info)) return rc;
    if (int rc = c->detect.begin(c, faqcs_detect_scratch_bytes())) return rc;
    HIPCHK(faqcs_launch_detect(b->qual, b->offset, first, count, d_text, d_def_pos, d_def_len, d_info, c->detect.scratch.p, c->n_cu, c->compute));
    return 0;
}

extern "C" int faqcs_first_error_device(faqcs_ctx *c, const faqcs_read_result *d_results, uint32_t n, faqcs_error_info *d_info)
{
    if (!c) return fail(FAQCS_E_INVAL, "null ctx");
    if (int rc = first_error_check_args("faqcs_first_error_device", d_results, n, d_info)) return rc;
    if (int rc = c->detect.begin(c, faqcs_first_error_scratch_bytes(n))) return rc;
    HIPCHK(faqcs_launch_first_error(d_results, n, d_info, c->detect.scratch.p, c->n_cu, c->compute));
    return 0;
}
