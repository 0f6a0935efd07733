// faqcs_host.cpp -- the part of libfaqcs_mi.so's C ABI (include/faqcs_mi.h) that never touches HIP: the counter layout and the host helpers,
// the host statements of the parse / render / pair / inflate / deflate rules -- what the GPU tests hold the kernels against -- with their
// error texts and argument checks, and the error sink of the whole library.  Plain C++17: it also links into a stand-alone program
// (tools/host_statements_check.cpp runs it under the sanitizers).
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "faqcs_host.h"
#include "faqcs_inflate.h"
#include "faqcs_gunzip.h"
#include "faqcs_deflate.h"

static thread_local std::string g_err;
int fail(int code, const std::string &msg) { g_err = msg; return code; }
extern "C" const char *faqcs_last_error(void) { return g_err.c_str(); }

// ---------------------------------------------------------------------------------------------------------
// layout + host helpers
// ---------------------------------------------------------------------------------------------------------
extern "C" int faqcs_abi_version(void) { return FAQCS_ABI_VERSION; }

extern "C" int faqcs_counters_layout(uint32_t R, uint32_t n_adapters, faqcs_layout *L)
{
    if (!L || R == 0 || R > FAQCS_MAX_READ_LENGTH || n_adapters > FAQCS_MAX_ADAPTERS) return fail(FAQCS_E_INVAL, "faqcs_counters_layout: bad size");
    uint64_t o = 0;
    memset(L, 0, sizeof(*L));
    L->max_read_length = R;
    L->n_adapters = n_adapters;
    L->filter_stats = o;    o += 32;
    L->pre_read_qhist = o;  o += FAQCS_NQ;
    L->pre_base_qhist = o;  o += FAQCS_NQ;
    L->post_read_qhist = o; o += FAQCS_NQ;
    L->post_base_qhist = o; o += FAQCS_NQ;
    L->pre_len_hist = o;    o += (uint64_t)R + 1;
    L->post_len_hist = o;   o += (uint64_t)R + 1;
    L->pre_qual = o;        o += (uint64_t)R * FAQCS_NQ;
    L->post_qual = o;       o += (uint64_t)R * FAQCS_NQ;
    L->pre_base = o;        o += (uint64_t)R * FAQCS_NBASE;
    L->post_base = o;       o += (uint64_t)R * FAQCS_NBASE;
    L->pre_comp = o;        o += (uint64_t)FAQCS_NCOMP_BIN * FAQCS_NCOMP_KIND;
    L->post_comp = o;       o += (uint64_t)FAQCS_NCOMP_BIN * FAQCS_NCOMP_KIND;
    L->adapter_stats = o;   o += (uint64_t)n_adapters * 2;
    L->total = o;
    return 0;
}

extern "C" uint32_t faqcs_counter_rows(const uint64_t *m, uint32_t max_rows, uint32_t n_cols)
{
    for (uint32_t r = max_rows; r > 0; --r)
        for (uint32_t c = 0; c < n_cols; ++c)
            if (m[(uint64_t)(r - 1) * n_cols + c]) return r;
    return 0;
}

extern "C" int faqcs_apply_edits(const faqcs_params *p, const uint8_t *seq, const uint8_t *qual, uint32_t read_len,
                                 const faqcs_read_result *res, uint8_t *out_seq, uint8_t *out_qual)
{
    if (!p || !res || (uint32_t)res->start + res->len > read_len) return fail(FAQCS_E_INVAL, "faqcs_apply_edits: window outside the read");
    uint32_t lead = 0, trail = read_len; // [lead, trail) keeps its quality (trim.cpp:1191-1216)
    while (lead < read_len && seq[lead] == 'N') ++lead;
    while (trail > 0 && seq[trail - 1] == 'N') --trail;
    const int in = p->input_quality_offset, out = p->output_quality_offset;
    for (uint32_t k = 0; k < res->len; ++k) {
        const uint32_t i = res->start + k;
        const int raw = (i < lead || i >= trail) ? in : (int)(int8_t)qual[i];
        int qs = raw - in;
        if (qs < 0) qs = 0;
        uint8_t b = seq[i];
        if (p->replace_to_N_q > 0 && b == 'G' && qs < (int)p->replace_to_N_q) b = 'N'; // trim.cpp:390-403
        out_seq[k] = b;
        out_qual[k] = (in != out) ? (uint8_t)(qs + out) : (uint8_t)raw;                  // trim.cpp:516-525
    }
    return 0;
}

extern "C" int faqcs_auto_detect_quality_offset(const uint8_t *qual, const uint32_t *offset, uint32_t n_reads)
{
    if (!n_reads) return 0;
    for (uint32_t i = offset[0]; i < offset[n_reads]; ++i) { // trim.cpp:599-617
        const int c = (int)(int8_t)qual[i];
        if (c > 74) return 64;
        if (c < 59) return 33;
    }
    return 0;
}

static const char *const PARSE_TEXT[] = {"", "fastq.cpp:next_read: Unable to read sequence", "fastq.cpp:next_read: Unable to read '+'",
                                         "fastq.cpp:next_read: Error reading '+' delimiter", "fastq.cpp:next_read: Unable to read quality",
                                         "fastq.cpp:next_read: |Sequence| != |Quality|"};
extern "C" const char *faqcs_parse_error_text(int code) { return code >= 0 && code <= FAQCS_PARSE_E_LENGTH ? PARSE_TEXT[code] : nullptr; }

int parse_check_args(const char *who, const uint8_t *text, uint64_t n_text, const faqcs_parse_out *out)
{
    const std::string w(who);
    if (!out || (!text && n_text)) return fail(FAQCS_E_INVAL, w + ": null text or output");
    if (!out->seq || !out->qual || !out->offset || !out->terminal_n || !out->info) return fail(FAQCS_E_INVAL, w + ": null output arena, offset, terminal_n or info");
    if (((uintptr_t)out->seq | (uintptr_t)out->qual) & 15u) return fail(FAQCS_E_INVAL, w + ": the output arenas must be 16-byte aligned");
    if ((out->def_pos == nullptr) != (out->def_len == nullptr)) return fail(FAQCS_E_INVAL, w + ": def_pos and def_len go together");
    if (n_text >= (1ull << 32)) return fail(FAQCS_E_INVAL, w + ": a text of 2^32 bytes or more must be cut into chunks (final = 0, consumed)");
    return 0;
}

// The host statement of the parse rules (include/faqcs_mi.h at faqcs_parse_device).  Two passes over the text: what the records need, then --
// when it fits -- the records.
extern "C" int faqcs_parse_host(const uint8_t *text, uint64_t n_text, int final, const faqcs_parse_out *out)
{
    if (int rc = parse_check_args("faqcs_parse_host", text, n_text, out)) return rc;
    // [content end, start of the next line, terminated?] of the line that starts at p
    auto line = [&](uint64_t p, uint64_t &content_end, uint64_t &next) -> bool {
        uint64_t x = p;
        while (x < n_text && text[x] != '\n' && text[x] != '\r') ++x;
        content_end = x;
        while (x < n_text && text[x] != '\n') ++x;
        if (x == n_text) { next = n_text; return false; }
        next = x + 1;
        return true;
    };
    faqcs_parse_info info{};
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t p = 0, o = 0;
        uint32_t k = 0;
        if (pass) out->offset[0] = 0;
        const uint32_t stop = pass ? info.n_reads : 0xffffffffu;
        while (p < n_text && k < stop) {
            uint64_t e0, e1, e2, e3, n0, n1, n2, n3;
            int err = FAQCS_PARSE_OK;
            bool complete = false; // (final = 0: a record whose lines do not all end in '\n' is not there yet)
            const bool t0 = line(p, e0, n0);
            bool t1 = false, t2 = false, t3 = false;
            if (n0 >= n_text) err = FAQCS_PARSE_E_SEQUENCE;
            else {
                t1 = line(n0, e1, n1);
                if (n1 >= n_text) err = FAQCS_PARSE_E_PLUS;
                else {
                    t2 = line(n1, e2, n2);
                    if (!t2) err = FAQCS_PARSE_E_PLUS_DELIM;
                    else if (n2 >= n_text) err = FAQCS_PARSE_E_QUALITY;
                    else {
                        t3 = line(n2, e3, n3);
                        complete = true;
                        if (e1 - n0 != e3 - n2) err = FAQCS_PARSE_E_LENGTH;
                    }
                }
            }
            if (!final && !(complete && t0 && t1 && t2 && t3)) break; // left to the caller, no error
            if (err) { info.error = err; break; }
            const uint64_t len = e1 - n0;
            if (pass) {
                memcpy(out->seq + o, text + n0, (size_t)len);
                memcpy(out->qual + o, text + n2, (size_t)len);
                out->terminal_n[k] = len ? (uint8_t)((text[n0] == 'N' ? 1 : 0) | (text[n0 + len - 1] == 'N' ? 2 : 0)) : (uint8_t)0;
                if (out->def_pos) { out->def_pos[k] = (uint32_t)p; out->def_len[k] = (uint32_t)(e0 - p); }
                out->offset[k + 1] = (uint32_t)(o + len);
            } else {
                if (len > info.max_read_len) info.max_read_len = (uint32_t)len;
                info.consumed = n3;
            }
            o += len; ++k;
            p = n3;
        }
        if (pass) break;
        info.n_bytes = o;
        info.n_reads = k;
        info.overflow = (o > out->capacity_bytes || k > out->capacity_reads || o >= (1ull << 32)) ? 1u : 0u;
        *out->info = info;
        if (info.overflow) break;
    }
    return 0;
}

int render_check_args(const char *who, const faqcs_batch *b, const uint8_t *text, const uint32_t *def_pos, const uint32_t *def_len, const faqcs_render_out *out)
{
    const std::string w(who);
    if (!b || !out) return fail(FAQCS_E_INVAL, w + ": null batch or output");
    if (!def_pos || !def_len) return fail(FAQCS_E_INVAL, w + ": null defline spans");
    if (!out->text || !out->info) return fail(FAQCS_E_INVAL, w + ": null output text or info");
    if ((uintptr_t)out->text & 15u) return fail(FAQCS_E_INVAL, w + ": the output text must be 16-byte aligned");
    if (b->n_reads && (!text || !b->seq || !b->qual || !b->offset)) return fail(FAQCS_E_INVAL, w + ": null text or batch arrays");
    return 0;
}

static const char *const INFLATE_TEXT[] = {"", "bgzf: not a BGZF member header", "bgzf: the decoded length differs from ISIZE",
                                           "bgzf: invalid deflate data", "bgzf: the CRC-32 differs from the trailer", "bgzf: the last member is incomplete"};
extern "C" const char *faqcs_inflate_error_text(int code)
{
    if (code == FAQCS_INFLATE_E_SERIAL) return "gzip: the stream does not split into pieces; inflate it on the host";
    return code >= 0 && code <= FAQCS_INFLATE_E_TRUNCATED ? INFLATE_TEXT[code] : nullptr;
}

int bgzf_index_check_args(const char *who, const uint8_t *comp, uint64_t n_comp, const uint32_t *member_offset, const faqcs_bgzf_index_info *info)
{
    const std::string w(who);
    if (!info || !member_offset || (!comp && n_comp)) return fail(FAQCS_E_INVAL, w + ": null input, offsets or info");
    if (n_comp >= (1ull << 32)) return fail(FAQCS_E_INVAL, w + ": 2^32 bytes or more must be cut into chunks (final = 0, consumed)");
    return 0;
}

extern "C" int faqcs_bgzf_index_host(const uint8_t *comp, uint64_t n_comp, int final, uint32_t *member_offset, uint32_t capacity_members, faqcs_bgzf_index_info *info)
{
    if (int rc = bgzf_index_check_args("faqcs_bgzf_index_host", comp, n_comp, member_offset, info)) return rc;
    faqcs_inflate::IndexInfo ii{};
    faqcs_inflate::bgzf_index(comp, n_comp, final, member_offset, capacity_members, ii);
    info->consumed = ii.consumed; info->n_members = ii.n_members; info->overflow = ii.overflow; info->error = ii.error; info->reserved = 0;
    return 0;
}

int inflate_check_args(const char *who, const uint8_t *comp, uint64_t n_comp, const uint32_t *member_offset, uint32_t n_members, const faqcs_inflate_out *out)
{
    const std::string w(who);
    if (!out || !out->text || !out->info) return fail(FAQCS_E_INVAL, w + ": null output, text or info");
    if (n_members && (!comp || !member_offset)) return fail(FAQCS_E_INVAL, w + ": null input or member offsets");
    if ((uintptr_t)out->text & 15u) return fail(FAQCS_E_INVAL, w + ": the output text must be 16-byte aligned");
    if (n_comp >= (1ull << 32)) return fail(FAQCS_E_INVAL, w + ": 2^32 compressed bytes or more must be cut into chunks");
    if (n_members > n_comp / faqcs_inflate::MIN_MEMBER) return fail(FAQCS_E_INVAL, w + ": more members than the input can hold");
    return 0;
}

// The host statement of the inflate rules (include/faqcs_mi.h at faqcs_inflate_device): the scan over every member's header, then -- when
// the total fits -- the members in input order up to the first bad one, each decoded into a buffer of its own first, so that exactly
// text[0 .. n_bytes) is written.
extern "C" int faqcs_inflate_host(const uint8_t *comp, uint64_t n_comp, const uint32_t *member_offset, uint32_t n_members, const faqcs_inflate_out *out)
{
    namespace inf = faqcs_inflate;
    if (int rc = inflate_check_args("faqcs_inflate_host", comp, n_comp, member_offset, n_members, out)) return rc;
    faqcs_inflate_info info{};
    auto header = [&](uint32_t k, inf::Member &m) -> int {
        const uint32_t a = member_offset[k], e = member_offset[k + 1];
        m = inf::Member{0, 0, 0, 0};
        return (e > a && e <= n_comp) ? inf::parse_member(comp + a, e - a, m) : (int)inf::ST_E_HEADER;
    };
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_members; ++k) {
        inf::Member m;
        if (!header(k, m)) total += m.isize;
    }
    info.n_bytes = total; info.n_members = n_members;
    info.overflow = (total > out->capacity_bytes || total >= (1ull << 32)) ? 1u : 0u;
    if (!info.overflow) {
        std::vector<uint8_t> one(inf::MAX_ISIZE);
        std::unique_ptr<inf::Tables> T(new inf::Tables);
        inf::HostSink<uint8_t> S{one.data()};
        inf::crc_init(*T, S);
        uint64_t pos = 0;
        bool bad = false;
        if (out->member_text_offset) out->member_text_offset[0] = 0;
        for (uint32_t k = 0; k < n_members; ++k) {
            inf::Member m;
            int st = header(k, m);
            const uint32_t isz = st ? 0u : m.isize;
            if (!bad) {
                if (!st) st = inf::inflate_member_host(comp + member_offset[k], member_offset[k + 1] - member_offset[k], *T, one.data(), m);
                if (st) { bad = true; info.n_bytes = pos; info.n_members = k; info.error = st; }
                else if (m.isize) memcpy(out->text + pos, one.data(), m.isize);
            }
            pos += isz;
            if (out->member_text_offset) out->member_text_offset[k + 1] = (uint32_t)pos;
        }
    }
    *out->info = info;
    return 0;
}

int gunzip_check_args(const char *who, const uint8_t *comp, uint64_t n_comp, uint32_t piece_bytes, const faqcs_gunzip_out *out)
{
    const std::string w(who);
    if (!out || !out->text || !out->info) return fail(FAQCS_E_INVAL, w + ": null output, text or info");
    if (!comp && n_comp) return fail(FAQCS_E_INVAL, w + ": null input");
    if ((uintptr_t)out->text & 15u) return fail(FAQCS_E_INVAL, w + ": the output text must be 16-byte aligned");
    if (n_comp >= (1ull << 32)) return fail(FAQCS_E_INVAL, w + ": 2^32 compressed bytes or more in one call");
    if (piece_bytes && piece_bytes < faqcs_gunzip::MIN_PIECE) return fail(FAQCS_E_INVAL, w + ": a piece is at least 1 024 bytes");
    return 0;
}

void gunzip_info_out(const faqcs_gunzip::Info &i, faqcs_gunzip_info *o)
{
    o->n_bytes = i.n_bytes; o->consumed = i.consumed; o->n_members = i.n_members; o->overflow = i.overflow; o->error = i.error;
    o->n_pieces = i.n_pieces; o->n_fixups = i.n_fixups; o->n_rounds = i.n_rounds;
}

// The host statement of the gunzip rules (include/faqcs_mi.h at faqcs_gunzip_device): the walk and the passes of csrc/faqcs_gunzip.h on one
// thread, into a buffer of its own first, so that exactly text[0 .. n_bytes) is written.
extern "C" int faqcs_gunzip_host(const uint8_t *comp, uint64_t n_comp, uint32_t piece_bytes, uint32_t max_rounds, const faqcs_gunzip_out *out)
{
    if (int rc = gunzip_check_args("faqcs_gunzip_host", comp, n_comp, piece_bytes, out)) return rc;
    std::unique_ptr<faqcs_gunzip::HostBackend> B(new faqcs_gunzip::HostBackend(comp, n_comp, piece_bytes));
    faqcs_gunzip::Info info;
    if (int rc = faqcs_gunzip::gunzip_run(*B, n_comp, piece_bytes, max_rounds, out->capacity_bytes, info))
        return rc == faqcs_gunzip::E_RECORD ? fail(FAQCS_E_INVAL, "faqcs_gunzip_host: a piece record that no run produces") : rc;
    if (!info.overflow && info.n_bytes) memcpy(out->text, B->text.data(), info.n_bytes);
    gunzip_info_out(info, out->info);
    return 0;
}

int gunzip_state_check_args(const char *who, const faqcs_gunzip_state *s)
{
    const std::string w(who);
    if (!s || !s->window) return fail(FAQCS_E_INVAL, w + ": null state or window");
    if (s->phase > FAQCS_GUNZIP_TRAILER) return fail(FAQCS_E_INVAL, w + ": the phase is BETWEEN, STREAM or TRAILER");
    if (s->bit > 7 || (s->bit && s->phase != FAQCS_GUNZIP_STREAM)) return fail(FAQCS_E_INVAL, w + ": bit is 0 .. 7, and 0 outside the phase STREAM");
    if (s->window_bytes != (s->member_bytes < faqcs_gunzip::WIN ? s->member_bytes : faqcs_gunzip::WIN)) return fail(FAQCS_E_INVAL, w + ": window_bytes is min(member_bytes, 32 768)");
    if (s->reserved) return fail(FAQCS_E_INVAL, w + ": reserved is 0");
    return 0;
}

void gunzip_state_in(const faqcs_gunzip_state *s, faqcs_gunzip::State *o)
{
    *o = faqcs_gunzip::State{s->member_bytes, s->total_bytes, s->total_comp, s->phase, s->bit, s->crc, s->window_bytes, s->members, 0};
}

void gunzip_state_out(const faqcs_gunzip::State &s, faqcs_gunzip_state *o)
{
    o->member_bytes = s.member_bytes; o->total_bytes = s.total_bytes; o->total_comp = s.total_comp; o->phase = s.phase; o->bit = s.bit;
    o->crc = s.crc; o->window_bytes = s.window_bytes; o->members = s.members;
}

// The host statement of faqcs_gunzip_stream_device: the same walk with the carried state, the caller's window in host memory.
extern "C" int faqcs_gunzip_stream_host(const uint8_t *comp, uint64_t n_comp, int final, uint32_t piece_bytes, uint32_t max_rounds, faqcs_gunzip_state *state,
                                        const faqcs_gunzip_out *out)
{
    if (int rc = gunzip_check_args("faqcs_gunzip_stream_host", comp, n_comp, piece_bytes, out)) return rc;
    if (int rc = gunzip_state_check_args("faqcs_gunzip_stream_host", state)) return rc;
    std::unique_ptr<faqcs_gunzip::HostBackend> B(new faqcs_gunzip::HostBackend(comp, n_comp, piece_bytes));
    B->window = state->window;
    faqcs_gunzip::Info info;
    faqcs_gunzip::State st;
    gunzip_state_in(state, &st);
    if (int rc = faqcs_gunzip::gunzip_run(*B, n_comp, piece_bytes, max_rounds, out->capacity_bytes, info, &st, final != 0))
        return rc == faqcs_gunzip::E_RECORD ? fail(FAQCS_E_INVAL, "faqcs_gunzip_stream_host: a piece record that no run produces") : rc;
    if (!info.overflow && info.n_bytes) memcpy(out->text, B->text.data(), info.n_bytes);
    gunzip_info_out(info, out->info);
    gunzip_state_out(st, state);
    return 0;
}

int deflate_check_args(const char *who, const uint8_t *text, uint64_t n_text, uint32_t member_bytes, int final, int mode, const faqcs_deflate_out *out)
{
    const std::string w(who);
    if (mode != FAQCS_DEFLATE_FAST && mode != FAQCS_DEFLATE_DENSE) return fail(FAQCS_E_INVAL, w + ": the mode is FAQCS_DEFLATE_FAST or FAQCS_DEFLATE_DENSE");
    if (!out || !out->comp || !out->info) return fail(FAQCS_E_INVAL, w + ": null output, comp or info");
    if (!text && n_text) return fail(FAQCS_E_INVAL, w + ": null text");
    if ((uintptr_t)out->comp & 15u) return fail(FAQCS_E_INVAL, w + ": the output must be 16-byte aligned");
    if (n_text >= (1ull << 32)) return fail(FAQCS_E_INVAL, w + ": 2^32 bytes of text or more must be cut into chunks (final = 0)");
    if (member_bytes > faqcs_deflate::MAX_TEXT) return fail(FAQCS_E_INVAL, w + ": a member holds at most 65 280 bytes of text");
    const uint64_t mb = member_bytes ? member_bytes : (uint64_t)faqcs_deflate::MAX_TEXT;
    if ((n_text + mb - 1) / mb + (final ? 1u : 0u) > 0xffffffffull) return fail(FAQCS_E_INVAL, w + ": 2^32 members or more (the member count is 32 bits wide)");
    return 0;
}

// The host statement of the deflate rules (include/faqcs_mi.h at faqcs_deflate_device): every member by the encoder text of the kernel into
// a slot of its own, then -- when the total fits -- the members back to back, so that exactly comp[0 .. n_bytes) is written.
extern "C" int faqcs_deflate_host(const uint8_t *text, uint64_t n_text, uint32_t member_bytes, int final, const faqcs_deflate_out *out)
{
    return faqcs_deflate_host_mode(text, n_text, member_bytes, final, FAQCS_DEFLATE_FAST, out);
}

extern "C" int faqcs_deflate_host_mode(const uint8_t *text, uint64_t n_text, uint32_t member_bytes, int final, int mode, const faqcs_deflate_out *out)
{
    namespace def = faqcs_deflate;
    static_assert(FAQCS_DEFLATE_FAST == def::MODE_FAST && FAQCS_DEFLATE_DENSE == def::MODE_DENSE, "the encoder's modes are the header's");
    if (int rc = deflate_check_args("faqcs_deflate_host", text, n_text, member_bytes, final, mode, out)) return rc;
    const uint32_t mb = member_bytes ? member_bytes : (uint32_t)def::MAX_TEXT;
    const uint32_t n_data = (uint32_t)((n_text + mb - 1) / mb), n = n_data + (final ? 1u : 0u);
    std::unique_ptr<def::Work> W(new def::Work);
    std::vector<uint32_t> tok((mb + def::TILE - 1) / def::TILE * def::TILE);
    std::vector<uint8_t> slot(def::slot_bytes(mb)), all;
    std::vector<uint32_t> ends(n);
    def::HostExec X;
    faqcs_deflate_info info{};
    for (uint32_t k = 0; k < n_data; ++k) {
        const uint64_t a = (uint64_t)k * mb;
        const uint32_t len = (uint32_t)std::min<uint64_t>(mb, n_text - a);
        const uint32_t r = mode == FAQCS_DEFLATE_DENSE ? def::deflate_member<def::MODE_DENSE>(X, *W, text + a, len, tok.data(), slot.data())
                                                       : def::deflate_member<def::MODE_FAST>(X, *W, text + a, len, tok.data(), slot.data());
        info.n_stored += r >> 31;
        all.insert(all.end(), slot.begin(), slot.begin() + (r & 0x7fffffffu));
        ends[k] = (uint32_t)all.size();
    }
    if (final) {
        for (uint32_t i = 0; i < def::EOF_BYTES; ++i) all.push_back((uint8_t)def::eof_byte(i));
        ends[n_data] = (uint32_t)all.size();
    }
    info.n_bytes = all.size(); info.n_members = n;
    info.overflow = (all.size() > out->capacity_bytes || all.size() >= (1ull << 32)) ? 1u : 0u;
    if (!info.overflow) {
        if (!all.empty()) memcpy(out->comp, all.data(), all.size());
        if (out->member_offset) {
            out->member_offset[0] = 0;
            for (uint32_t k = 0; k < n; ++k) out->member_offset[k + 1] = ends[k];
        }
    }
    *out->info = info;
    return 0;
}

// The host statement of the render rules (include/faqcs_mi.h at faqcs_render_device).  Two passes over the candidates: what the records need,
// then -- when it fits -- the records.
extern "C" int faqcs_render_host(const faqcs_params *p, const faqcs_batch *b, const faqcs_read_result *results, const uint8_t *text,
                                 const uint32_t *def_pos, const uint32_t *def_len, const uint8_t *select, const uint32_t *order,
                                 const faqcs_render_out *out)
{
    if (int rc = render_check_args("faqcs_render_host", b, text, def_pos, def_len, out)) return rc;
    if (results && !p) return fail(FAQCS_E_INVAL, "faqcs_render_host: results without parameters");
    const uint32_t n = b->n_reads;
    faqcs_render_info info{};
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t o = 0;
        uint32_t k = 0;
        if (pass && out->rec_offset) out->rec_offset[0] = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t i = order ? order[j] : j;
            if (i >= n) continue;
            if (select && !select[i]) continue;
            if (results && !(results[i].flags & FAQCS_F_VALID)) continue;
            const uint32_t a = b->offset[i], L = b->offset[i + 1] - a;
            const uint32_t start = results ? results[i].start : 0u, len = results ? results[i].len : L;
            if (start + len > L) return fail(FAQCS_E_INVAL, "faqcs_render_host: window outside the read");
            const uint64_t size = (uint64_t)def_len[i] + 2ull * len + 5ull;
            if (pass) {
                uint8_t *w = out->text + o;
                memcpy(w, text + def_pos[i], def_len[i]);
                w += def_len[i];
                *w++ = '\n';
                uint8_t *ws = w, *wq = w + len + 3;
                if (results) {
                    if (int rc = faqcs_apply_edits(p, b->seq + a, b->qual + a, L, results + i, ws, wq)) return rc;
                } else {
                    memcpy(ws, b->seq + a, len);
                    memcpy(wq, b->qual + a, len);
                }
                ws[len] = '\n'; ws[len + 1] = '+'; ws[len + 2] = '\n';
                wq[len] = '\n';
                if (out->rec_offset) out->rec_offset[k + 1] = (uint32_t)(o + size);
                if (out->rec_index) out->rec_index[k] = i;
            }
            o += size; ++k;
        }
        if (pass) break;
        info.n_bytes = o;
        info.n_reads = k;
        info.overflow = (o > out->capacity_bytes || o >= (1ull << 32)) ? 1u : 0u;
        *out->info = info;
        if (info.overflow) break;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// the pair stage (include/faqcs_mi.h at faqcs_pair_device)
// ---------------------------------------------------------------------------------------------------------
static int mate_check(const std::string &w, const faqcs_mate *m, uint32_t n)
{
    if (!m || !m->batch) return fail(FAQCS_E_INVAL, w + ": null mate or batch");
    if (n && (!m->text || !m->def_pos || !m->def_len)) return fail(FAQCS_E_INVAL, w + ": null text or defline spans");
    return 0;
}

int pair_check_args(const char *who, const faqcs_mate *m1, const faqcs_mate *m2, const uint8_t *route, const faqcs_pair_info *info, uint32_t *n)
{
    const std::string w(who);
    if (!m1 || !m2 || !m1->batch || !m2->batch) return fail(FAQCS_E_INVAL, w + ": null mate or batch");
    if (!info) return fail(FAQCS_E_INVAL, w + ": null info");
    *n = std::min(m1->batch->n_reads, m2->batch->n_reads);
    if (*n > 0x7fffffffu) return fail(FAQCS_E_INVAL, w + ": more than 2^31 - 1 pairs must be cut into chunks");
    if (int rc = mate_check(w, m1, *n)) return rc;
    if (int rc = mate_check(w, m2, *n)) return rc;
    if ((m1->results == nullptr) != (m2->results == nullptr)) return fail(FAQCS_E_INVAL, w + ": results of one mate only");
    if (m1->results && !route) return fail(FAQCS_E_INVAL, w + ": results without a route");
    return 0;
}

int render_pair_check_args(const char *who, int file, const faqcs_mate *m1, const faqcs_mate *m2, const uint8_t *route, uint32_t n_pairs, const faqcs_render_out *out)
{
    const std::string w(who);
    if (file < FAQCS_FILE_QC1 || file > FAQCS_FILE_DISCARD) return fail(FAQCS_E_INVAL, w + ": no such file");
    if (!m1 || !m2 || !m1->batch || !m2->batch || !out) return fail(FAQCS_E_INVAL, w + ": null mate, batch or output");
    if (!out->text || !out->info) return fail(FAQCS_E_INVAL, w + ": null output text or info");
    if ((uintptr_t)out->text & 15u) return fail(FAQCS_E_INVAL, w + ": the output text must be 16-byte aligned");
    if (n_pairs > 0x7fffffffu || n_pairs > m1->batch->n_reads || n_pairs > m2->batch->n_reads) return fail(FAQCS_E_INVAL, w + ": more pairs than a batch has reads, or than 2^31 - 1");
    for (const faqcs_mate *m : {m1, m2}) {
        if (!m->def_pos || !m->def_len) return fail(FAQCS_E_INVAL, w + ": null defline spans");
        if (n_pairs && (!m->text || !m->batch->seq || !m->batch->qual || !m->batch->offset)) return fail(FAQCS_E_INVAL, w + ": null text or batch arrays");
        if (n_pairs && file != FAQCS_FILE_DISCARD && !m->results) return fail(FAQCS_E_INVAL, w + ": a trimmed file without results");
    }
    if (n_pairs && !route) return fail(FAQCS_E_INVAL, w + ": null route");
    return 0;
}

// parse_id (trim.cpp:188-222): how many bytes of the defline d[0 .. len) are its id
static uint32_t id_length(const uint8_t *d, uint32_t len)
{
    uint32_t loc = 0;
    while (loc < len && d[loc] != ' ') ++loc;
    if (loc > 1 && d[loc - 1] >= '0' && d[loc - 1] <= '9' && (d[loc - 2] == '.' || d[loc - 2] == '/')) loc -= 2;
    return loc;
}

// The host statement of the pair rules: the pairs in order up to the first whose ids differ.
extern "C" int faqcs_pair_host(const faqcs_mate *m1, const faqcs_mate *m2, uint8_t *route, faqcs_pair_info *info)
{
    uint32_t n = 0;
    if (int rc = pair_check_args("faqcs_pair_host", m1, m2, route, info, &n)) return rc;
    const bool routed = m1->results != nullptr;
    faqcs_pair_info r{};
    uint32_t i = 0;
    for (; i < n; ++i) {
        const uint8_t *a = m1->text + m1->def_pos[i], *b = m2->text + m2->def_pos[i];
        const uint32_t la = id_length(a, m1->def_len[i]), lb = id_length(b, m2->def_len[i]);
        if (la != lb || (la && memcmp(a, b, la) != 0)) { r.mismatch = 1; r.id_len[0] = la; r.id_len[1] = lb; break; }
        if (!routed) continue;
        const bool v1 = m1->results[i].flags & FAQCS_F_VALID, v2 = m2->results[i].flags & FAQCS_F_VALID;
        route[i] = (uint8_t)((v1 ? FAQCS_ROUTE_V1 : 0) | (v2 ? FAQCS_ROUTE_V2 : 0));
        if (v1 && v2) { r.paired_read_number += 2; r.paired_base_length += (uint64_t)m1->results[i].len + m2->results[i].len; }
        else if (v1 || v2) ++r.n_one_valid;
        else ++r.n_none_valid;
    }
    r.n_pairs = i;
    if (routed)
        for (; i < n; ++i) route[i] = (uint8_t)FAQCS_ROUTE_NOWHERE;
    *info = r;
    return 0;
}

// The host statement of the paired rendering.  Two passes over the candidates, as faqcs_render_host.
extern "C" int faqcs_render_pair_host(const faqcs_params *p, int file, const faqcs_mate *m1, const faqcs_mate *m2, const uint8_t *route, uint32_t n_pairs,
                                      const faqcs_render_out *out)
{
    if (int rc = render_pair_check_args("faqcs_render_pair_host", file, m1, m2, route, n_pairs, out)) return rc;
    const bool trimmed = file != FAQCS_FILE_DISCARD;
    if (trimmed && n_pairs && !p) return fail(FAQCS_E_INVAL, "faqcs_render_pair_host: results without parameters");
    const faqcs_mate *const mate[2] = {m1, m2};
    faqcs_render_info info{};
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t o = 0;
        uint32_t k = 0;
        if (pass && out->rec_offset) out->rec_offset[0] = 0;
        for (uint64_t j = 0; j < 2ull * n_pairs; ++j) {
            const uint32_t i = (uint32_t)(j >> 1), s = (uint32_t)(j & 1), r = route[i];
            const bool take = file == FAQCS_FILE_QC1 ? (s == 0 && r == 3) : file == FAQCS_FILE_QC2 ? (s == 1 && r == 3)
                            : file == FAQCS_FILE_UNPAIRED ? r == (1u << s) : (r < 4 && !(r >> s & 1u));
            if (!take) continue;
            const faqcs_mate &m = *mate[s];
            const faqcs_batch *b = m.batch;
            const uint32_t a = b->offset[i], L = b->offset[i + 1] - a;
            const uint32_t start = trimmed ? m.results[i].start : 0u, len = trimmed ? m.results[i].len : L;
            if (start + len > L) return fail(FAQCS_E_INVAL, "faqcs_render_pair_host: window outside the read");
            const uint64_t size = (uint64_t)m.def_len[i] + 2ull * len + 5ull;
            if (pass) {
                uint8_t *w = out->text + o;
                memcpy(w, m.text + m.def_pos[i], m.def_len[i]);
                w += m.def_len[i];
                *w++ = '\n';
                uint8_t *ws = w, *wq = w + len + 3;
                if (trimmed) {
                    if (int rc = faqcs_apply_edits(p, b->seq + a, b->qual + a, L, m.results + i, ws, wq)) return rc;
                } else {
                    memcpy(ws, b->seq + a, len);
                    memcpy(wq, b->qual + a, len);
                }
                ws[len] = '\n'; ws[len + 1] = '+'; ws[len + 2] = '\n';
                wq[len] = '\n';
                if (out->rec_offset) out->rec_offset[k + 1] = (uint32_t)(o + size);
                if (out->rec_index) out->rec_index[k] = (uint32_t)j;
            }
            o += size; ++k;
        }
        if (pass) break;
        info.n_bytes = o;
        info.n_reads = k;
        info.overflow = (o > out->capacity_bytes || o >= (1ull << 32)) ? 1u : 0u;
        *out->info = info;
        if (info.overflow) break;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// the decisions around trim() (include/faqcs_mi.h at faqcs_detect_device)
// ---------------------------------------------------------------------------------------------------------
int detect_check_args(const char *who, const faqcs_batch *b, uint32_t first, uint32_t count, const uint8_t *text, const uint32_t *def_pos, const uint32_t *def_len, const faqcs_detect_info *info)
{
    const std::string w(who);
    if (!b || !info) return fail(FAQCS_E_INVAL, w + ": null batch or info");
    if ((uint64_t)first + count > b->n_reads) return fail(FAQCS_E_INVAL, w + ": the range of reads leaves the batch");
    if (count && (!b->qual || !b->offset)) return fail(FAQCS_E_INVAL, w + ": null batch arrays");
    if ((text == nullptr) != (def_pos == nullptr) || (text == nullptr) != (def_len == nullptr)) return fail(FAQCS_E_INVAL, w + ": text, def_pos and def_len go together");
    return 0;
}

int first_error_check_args(const char *who, const faqcs_read_result *results, uint32_t n, const faqcs_error_info *info)
{
    const std::string w(who);
    if (!info) return fail(FAQCS_E_INVAL, w + ": null info");
    if (n && !results) return fail(FAQCS_E_INVAL, w + ": null results");
    return 0;
}

// The host statement of the detect rules: the bytes of the range in order (trim.cpp:599-617), then the first defline (trim.cpp:619-626).
extern "C" int faqcs_detect_host(const faqcs_batch *b, uint32_t first, uint32_t count, const uint8_t *text, const uint32_t *def_pos, const uint32_t *def_len,
                                 faqcs_detect_info *info)
{
    if (int rc = detect_check_args("faqcs_detect_host", b, first, count, text, def_pos, def_len, info)) return rc;
    faqcs_detect_info d{0, first + count, 0u, 0u, 0u, 0u};
    for (uint32_t i = first; i < first + count && !d.quality_offset; ++i)
        for (uint32_t k = b->offset[i]; k < b->offset[i + 1]; ++k) {
            const int c = (int)(int8_t)b->qual[k];
            if (c > 74 || c < 59) {
                d.quality_offset = c > 74 ? 64 : 33;
                d.read = i; d.pos = k - b->offset[i]; d.byte = b->qual[k];
                break;
            }
        }
    if (count && text) d.next_seq = (def_len[first] >= 3 && memcmp(text + def_pos[first], "@NS", 3) == 0) ? 1u : 0u;
    *info = d;
    return 0;
}

// The host statement of where trim() threw: the results in order.
extern "C" int faqcs_first_error_host(const faqcs_read_result *results, uint32_t n, faqcs_error_info *info)
{
    if (int rc = first_error_check_args("faqcs_first_error_host", results, n, info)) return rc;
    faqcs_error_info e{n, 0u};
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t f = results[i].flags & (FAQCS_F_ERR_QUALITY | FAQCS_F_ERR_BASE);
        if (f) { e.n_good = i; e.flags = f; break; }
    }
    *info = e;
    return 0;
}
