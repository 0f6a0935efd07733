// host_statements_check.cpp -- the host statements of faqcs_amd/csrc/faqcs_host.cpp (what the GPU tests hold the kernels against) as a
// stand-alone program under AddressSanitizer and UBSan, every buffer of exactly the size the statement asked for:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o check tools/host_statements_check.cpp faqcs_amd/csrc/faqcs_host.cpp
//   ./check reads.fastq
// One-shot parse == chunked parse (final = 0, following `consumed`); render of the parsed batch == the text when the text is canonical;
// deflate -> index -> inflate gives the text back.  Prints one line of counts; exit 0 when every comparison held, 1 otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/faqcs_mi.h"

static int n_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++n_failed; fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)
#define CALL(x) do { const int rc_ = (x); if (rc_) { fprintf(stderr, "%s: error %d: %s\n", #x, rc_, faqcs_last_error()); exit(1); } } while (0)

// exactly n bytes (at least one), 16-byte aligned: the sanitizer sees the first byte past what a statement may write
template <class T> struct Exact {
    T *p = nullptr;
    explicit Exact(size_t n) { void *q = nullptr; if (posix_memalign(&q, 16, (n ? n : 1) * sizeof(T))) abort(); p = (T *)q; }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
};

struct Parsed {
    std::vector<uint8_t> seq, qual, tn;
    std::vector<uint32_t> offset{0}, def_pos, def_len;
    int error = 0;
    uint64_t consumed = 0;
    size_t n() const { return tn.size(); }
};

// text[pos .. pos + n) parsed with arenas of exactly the size a first call asks for; the records are appended to P, rebased to the whole text
static uint64_t parse_append(const uint8_t *text, uint64_t pos, uint64_t n, int final, Parsed &P)
{
    Exact<uint8_t> d_seq(0), d_qual(0), d_tn(0);
    Exact<uint32_t> d_off(1);
    faqcs_parse_info need{};
    faqcs_parse_out sizing{d_seq.p, d_qual.p, 0, 0, d_off.p, d_tn.p, nullptr, nullptr, &need};
    CALL(faqcs_parse_host(text + pos, n, final, &sizing));
    Exact<uint8_t> seq(need.n_bytes), qual(need.n_bytes), tn(need.n_reads);
    Exact<uint32_t> off((size_t)need.n_reads + 1), dp(need.n_reads), dl(need.n_reads);
    faqcs_parse_info info{};
    faqcs_parse_out out{seq.p, qual.p, need.n_bytes, need.n_reads, off.p, tn.p, dp.p, dl.p, &info};
    CALL(faqcs_parse_host(text + pos, n, final, &out));
    CHECK(!info.overflow && info.n_bytes == need.n_bytes && info.n_reads == need.n_reads && info.consumed == need.consumed && info.error == need.error,
          "the second call's info differs from the sizing call's");
    CHECK(off.p[0] == 0 && off.p[info.n_reads] == info.n_bytes, "offset[0], offset[n_reads]");
    const uint32_t base = P.offset.back();
    P.seq.insert(P.seq.end(), seq.p, seq.p + info.n_bytes);
    P.qual.insert(P.qual.end(), qual.p, qual.p + info.n_bytes);
    for (uint32_t k = 0; k < info.n_reads; ++k) {
        P.tn.push_back(tn.p[k]);
        P.offset.push_back(base + off.p[k + 1]);
        P.def_pos.push_back((uint32_t)(pos + dp.p[k]));
        P.def_len.push_back(dl.p[k]);
    }
    P.error = info.error;
    P.consumed = pos + info.consumed;
    return info.consumed;
}

// LF line ends, bare '+' lines, a final newline, whole records
static bool canonical(const std::vector<uint8_t> &t)
{
    if (t.empty()) return true;
    if (t.back() != '\n') return false;
    size_t line = 0, start = 0;
    for (size_t i = 0; i < t.size(); ++i) {
        if (t[i] == '\r') return false;
        if (t[i] != '\n') continue;
        if (line % 4 == 2 && !(i == start + 1 && t[start] == '+')) return false;
        ++line; start = i + 1;
    }
    return line % 4 == 0;
}

static void render_round_trip(const std::vector<uint8_t> &text, const Parsed &P, bool &compared)
{
    const uint32_t n = (uint32_t)P.n();
    const uint32_t seg[2] = {0, n};
    faqcs_batch b{};
    b.seq = P.seq.data(); b.qual = P.qual.data(); b.offset = P.offset.data(); b.n_reads = n; b.n_segments = 1; b.segment_start = seg;
    Exact<uint8_t> d_text(0);
    Exact<uint32_t> dp(n), dl(n);
    if (n) { memcpy(dp.p, P.def_pos.data(), (size_t)n * 4); memcpy(dl.p, P.def_len.data(), (size_t)n * 4); }
    faqcs_render_info need{};
    faqcs_render_out sizing{d_text.p, 0, nullptr, nullptr, &need};
    CALL(faqcs_render_host(nullptr, &b, nullptr, text.data(), dp.p, dl.p, nullptr, nullptr, &sizing));
    uint64_t want = 0;
    for (uint32_t k = 0; k < n; ++k) want += (uint64_t)P.def_len[k] + 2ull * (P.offset[k + 1] - P.offset[k]) + 5;
    CHECK(need.n_reads == n && need.n_bytes == want, "render: %u records, %llu bytes; expected %u, %llu", need.n_reads, (unsigned long long)need.n_bytes, n, (unsigned long long)want);
    Exact<uint8_t> out_text(need.n_bytes);
    Exact<uint32_t> rec_off((size_t)n + 1), rec_idx(n);
    faqcs_render_info info{};
    faqcs_render_out out{out_text.p, need.n_bytes, rec_off.p, rec_idx.p, &info};
    CALL(faqcs_render_host(nullptr, &b, nullptr, text.data(), dp.p, dl.p, nullptr, nullptr, &out));
    CHECK(!info.overflow && info.n_bytes == need.n_bytes && info.n_reads == n && rec_off.p[n] == need.n_bytes, "render: the second call's info");
    compared = !P.error && P.consumed == text.size() && canonical(text);
    if (compared) CHECK(info.n_bytes == text.size() && (text.empty() || !memcmp(out_text.p, text.data(), text.size())), "render: the rendered batch is not the canonical input text");
}

static void deflate_round_trip(const std::vector<uint8_t> &text, uint32_t member_bytes, uint64_t &n_members)
{
    Exact<uint8_t> d_comp(0);
    faqcs_deflate_info need{};
    faqcs_deflate_out sizing{d_comp.p, 0, nullptr, &need};
    CALL(faqcs_deflate_host(text.data(), text.size(), member_bytes, 1, &sizing));
    CHECK(need.overflow == 1 && need.n_members >= 1, "deflate: the sizing call");
    const uint32_t nm = need.n_members;
    Exact<uint8_t> comp(need.n_bytes);
    Exact<uint32_t> moff((size_t)nm + 1), moff2((size_t)nm + 1), toff((size_t)nm + 1);
    faqcs_deflate_info di{};
    faqcs_deflate_out dout{comp.p, need.n_bytes, moff.p, &di};
    CALL(faqcs_deflate_host(text.data(), text.size(), member_bytes, 1, &dout));
    CHECK(!di.overflow && di.n_bytes == need.n_bytes && di.n_members == nm && moff.p[nm] == need.n_bytes, "deflate: the second call's info");
    faqcs_bgzf_index_info xi{};
    CALL(faqcs_bgzf_index_host(comp.p, di.n_bytes, 1, moff2.p, nm, &xi));
    CHECK(!xi.overflow && !xi.error && xi.n_members == nm && xi.consumed == di.n_bytes, "index: %u members, %llu bytes, error %d", xi.n_members, (unsigned long long)xi.consumed, xi.error);
    CHECK(!memcmp(moff.p, moff2.p, ((size_t)nm + 1) * 4), "index: the member offsets differ from the encoder's");
    Exact<uint8_t> back(text.size());
    faqcs_inflate_info ii{};
    faqcs_inflate_out iout{back.p, text.size(), toff.p, &ii};
    CALL(faqcs_inflate_host(comp.p, di.n_bytes, moff.p, nm, &iout));
    CHECK(!ii.overflow && !ii.error && ii.n_members == nm && ii.n_bytes == text.size() && toff.p[nm] == text.size(), "inflate: %u members, %llu bytes, error %d", ii.n_members, (unsigned long long)ii.n_bytes, ii.error);
    CHECK(text.empty() || !memcmp(back.p, text.data(), text.size()), "inflate: the text did not come back (member_bytes %u)", member_bytes);
    n_members += nm;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s reads.fastq\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> text;
    for (uint8_t buf[65536];;) { const size_t got = fread(buf, 1, sizeof(buf), f); if (!got) break; text.insert(text.end(), buf, buf + got); }
    fclose(f);
    const uint64_t n = text.size();

    Parsed one;
    parse_append(text.data(), 0, n, 1, one);

    // the cuts: every byte offset of a small text, 97 pseudo-random ones of a larger one (in increasing order)
    std::vector<uint64_t> cuts;
    if (n < 4096) for (uint64_t c = 1; c < n; ++c) cuts.push_back(c);
    else {
        uint64_t x = 0x9e3779b97f4a7c15ull ^ n;
        std::vector<bool> taken(n, false);
        for (int i = 0; i < 97; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; taken[1 + x % (n - 1)] = true; }
        for (uint64_t c = 1; c < n; ++c) if (taken[c]) cuts.push_back(c);
    }
    Parsed chunked;
    uint64_t pos = 0;
    for (uint64_t c : cuts) {
        pos += parse_append(text.data(), pos, c - pos, 0, chunked);
        if (chunked.error) break;
    }
    if (!chunked.error) parse_append(text.data(), pos, n - pos, 1, chunked);
    CHECK(chunked.error == one.error && chunked.n() == one.n() && chunked.consumed == one.consumed, "chunked parse: %zu records, error %d; one call: %zu, %d", chunked.n(), chunked.error, one.n(), one.error);
    CHECK(chunked.seq == one.seq && chunked.qual == one.qual && chunked.offset == one.offset && chunked.tn == one.tn, "chunked parse: seq, qual, offset or terminal_n differ");
    CHECK(chunked.def_pos == one.def_pos && chunked.def_len == one.def_len, "chunked parse: the defline spans differ");

    bool compared = false;
    render_round_trip(text, one, compared);
    uint64_t n_members = 0;
    deflate_round_trip(text, 0, n_members);
    deflate_round_trip(text, 4096, n_members);
    printf("%llu bytes, %zu reads, parse error %d, %zu chunks, render %s, %llu members: %s\n", (unsigned long long)n, one.n(), one.error, cuts.size() + 1,
           compared ? "equal to the text" : "not compared (the text is not canonical)", (unsigned long long)n_members, n_failed ? "FAILED" : "ok");
    return n_failed ? 1 : 0;
}
