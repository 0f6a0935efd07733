// detect_host_fuzz.cpp -- the host statements of the decisions around trim() (faqcs_detect_host, faqcs_first_error_host in
// faqcs_amd/csrc/faqcs_host.cpp) as a stand-alone program for a build with AddressSanitizer and UBSan:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o detect_host_fuzz tools/detect_host_fuzz.cpp faqcs_amd/csrc/faqcs_host.cpp
//   usage: detect_host_fuzz SEED N
// N generated cases.  A batch of 0 .. 60 reads of 0 .. 40 bytes (runs of empty reads among them) whose quality bytes are undecided
// ('A' .. 'J') but for 0 .. 3 planted bytes of any value -- 58, 59, 74, 75, 0x7f, 0x80 and 0xff more often than the rest --; the arena has
// the padding of faqcs_batch around it (16 bytes in front, 64 behind) and that padding is DECISIVE throughout, so a statement that
// interpreted it would give another answer; offset[], the defline spans, the text and the results are of exactly the stated sizes, so the
// sanitizer sees the first byte past each.  A random range [first, first + count) -- empty ranges, whole batches, ranges that end the batch
// --, deflines from a small set around "@NS" with the defline of read `first` anywhere in the text, its end included.  Results with random
// non-error bits and 0 .. 3 reads with error bits.  Every case goes through a naive loop written here (read by read, byte by byte) and
// through the library's statement: every field of info must be equal.  The argument checks are made once.  Prints "N cases: ok"; exit 1 on
// the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/faqcs_mi.h"

static uint64_t g_state;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

static unsigned g_case;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "case %u: FAILED %s (line %d): ", g_case, #cond, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// exactly n elements (at least one): the sanitizer sees the first byte past what a statement may touch
template <class T> struct Exact {
    T *p = nullptr;
    size_t n;
    explicit Exact(size_t n_) : n(n_) { p = (T *)malloc((n ? n : 1) * sizeof(T)); if (!p) abort(); }
    Exact(const std::vector<T> &v) : Exact(v.size()) { if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
};

static uint8_t planted_byte()
{
    static const uint8_t edges[] = {58, 59, 74, 75, 0x7f, 0x80, 0xff, 0, '!', '~'};
    return below(3) ? edges[below(sizeof(edges))] : (uint8_t)below(256);
}

static void detect_case()
{
    const uint32_t n = below(4) ? below(61) : 0;
    std::vector<uint32_t> off(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + (below(4) ? below(41) : 0);
    const uint32_t total = off[n];
    std::vector<uint8_t> arena(FAQCS_ARENA_PAD_BEFORE + total + FAQCS_ARENA_PAD_AFTER);
    for (size_t k = 0; k < arena.size(); ++k) arena[k] = (k & 1) ? '!' : '~'; // the padding stays like this
    for (uint32_t k = 0; k < total; ++k) arena[FAQCS_ARENA_PAD_BEFORE + k] = (uint8_t)('A' + below(10));
    for (uint32_t k = below(4); k && total; --k) arena[FAQCS_ARENA_PAD_BEFORE + below(total)] = planted_byte();
    Exact<uint8_t> qual(arena);
    Exact<uint32_t> offset(off);
    const uint32_t first = below(n + 1);
    const uint32_t count = below(3) ? below(n - first + 1) : n - first;
    // deflines: laid down in a random rotation, so that any read's may end the text
    static const char *const defs[] = {"@NS", "@NS500:1", "@N", "", "NS500", "@ns", "x@NS", "@NS", "@", "@NT", "@MS", " @NS"};
    const bool with_text = below(4) != 0;
    std::vector<uint32_t> dpos(n), dlen(n);
    std::string text;
    const uint32_t rot = below(n ? n : 1);
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t i = (j + rot) % n;
        const std::string d = defs[below(sizeof(defs) / sizeof(defs[0]))];
        dpos[i] = (uint32_t)text.size(); dlen[i] = (uint32_t)d.size();
        text += d;
    }
    Exact<uint8_t> t(std::vector<uint8_t>(text.begin(), text.end()));
    Exact<uint32_t> def_pos(dpos), def_len(dlen);
    // the naive statement
    faqcs_detect_info want = {0, first + count, 0, 0, 0, 0};
    bool done = false;
    for (uint32_t i = first; i < first + count && !done; ++i)
        for (uint32_t k = off[i]; k < off[i + 1] && !done; ++k) {
            const signed char c = (signed char)arena[FAQCS_ARENA_PAD_BEFORE + k];
            if (c > 74 || c < 59) {
                want.quality_offset = c > 74 ? 64 : 33; want.read = i; want.pos = k - off[i]; want.byte = arena[FAQCS_ARENA_PAD_BEFORE + k];
                done = true;
            }
        }
    if (with_text && count) want.next_seq = text.compare(dpos[first], dlen[first] < 3 ? dlen[first] : 3, "@NS") == 0 ? 1u : 0u;
    // the library's (seq, segment_start and terminal_n are not read: null)
    faqcs_batch b = {nullptr, qual.p + FAQCS_ARENA_PAD_BEFORE, offset.p, n, 0, nullptr, 0, nullptr};
    faqcs_detect_info got;
    memset(&got, 0xcd, sizeof(got));
    const int rc = faqcs_detect_host(&b, first, count, with_text ? t.p : nullptr, with_text ? def_pos.p : nullptr, with_text ? def_len.p : nullptr, &got);
    CHECK(rc == 0, "%s", faqcs_last_error());
    CHECK(memcmp(&got, &want, sizeof(got)) == 0, "n %u first %u count %u: got {%d, %u, %u, %u, %u, %u}, want {%d, %u, %u, %u, %u, %u}", n, first, count,
          got.quality_offset, got.read, got.pos, got.byte, got.next_seq, got.reserved, want.quality_offset, want.read, want.pos, want.byte, want.next_seq, want.reserved);
    // whole batches: the statement agrees with the older helper
    if (first == 0 && count == n)
        CHECK(faqcs_auto_detect_quality_offset(qual.p + FAQCS_ARENA_PAD_BEFORE, offset.p, n) == want.quality_offset, "faqcs_auto_detect_quality_offset differs");
    CHECK(faqcs_detect_host(&b, first, n - first + 1, nullptr, nullptr, nullptr, &got) == FAQCS_E_INVAL, "a range that leaves the batch was taken");
}

static void error_case()
{
    const uint32_t n = below(5) ? below(200) : 0;
    std::vector<faqcs_read_result> r(n);
    const uint16_t other = (uint16_t)~(FAQCS_F_ERR_QUALITY | FAQCS_F_ERR_BASE);
    const bool all_bits = below(4) == 0;
    for (auto &x : r) { x.start = (uint16_t)rnd(); x.len = (uint16_t)rnd(); x.adapter = (uint16_t)rnd(); x.flags = all_bits ? other : (uint16_t)(rnd() & other); }
    for (uint32_t k = below(4); k && n; --k) r[below(n)].flags |= (uint16_t)((1 + below(3)) << 8);
    Exact<faqcs_read_result> res(r);
    faqcs_error_info want = {n, 0};
    for (uint32_t i = 0; i < n; ++i)
        if (r[i].flags & 0x0300u) { want.n_good = i; want.flags = r[i].flags & 0x0300u; break; }
    faqcs_error_info got;
    memset(&got, 0xcd, sizeof(got));
    const int rc = faqcs_first_error_host(n ? res.p : nullptr, n, &got);
    CHECK(rc == 0, "%s", faqcs_last_error());
    CHECK(got.n_good == want.n_good && got.flags == want.flags, "n %u: got {%u, %#x}, want {%u, %#x}", n, got.n_good, got.flags, want.n_good, want.flags);
}

static void argument_checks()
{
    uint8_t q[4] = {'A', 'A', 'A', 'A'};
    uint32_t off[2] = {0, 4}, dp[1] = {0}, dl[1] = {0};
    faqcs_batch b = {nullptr, q, off, 1, 0, nullptr, 0, nullptr};
    faqcs_detect_info d;
    faqcs_error_info e;
    CHECK(faqcs_detect_host(&b, 0, 1, nullptr, nullptr, nullptr, &d) == 0 && d.quality_offset == 0 && d.read == 1, "undecided");
    CHECK(faqcs_detect_host(nullptr, 0, 1, nullptr, nullptr, nullptr, &d) == FAQCS_E_INVAL, "null batch");
    CHECK(faqcs_detect_host(&b, 0, 1, nullptr, nullptr, nullptr, nullptr) == FAQCS_E_INVAL, "null info");
    CHECK(faqcs_detect_host(&b, 1, 1, nullptr, nullptr, nullptr, &d) == FAQCS_E_INVAL, "first + count > n_reads");
    CHECK(faqcs_detect_host(&b, 0xffffffffu, 2, nullptr, nullptr, nullptr, &d) == FAQCS_E_INVAL, "first + count wraps");
    CHECK(faqcs_detect_host(&b, 0, 1, q, nullptr, nullptr, &d) == FAQCS_E_INVAL && faqcs_detect_host(&b, 0, 1, q, dp, nullptr, &d) == FAQCS_E_INVAL &&
          faqcs_detect_host(&b, 0, 1, nullptr, dp, dl, &d) == FAQCS_E_INVAL && faqcs_detect_host(&b, 0, 1, q, nullptr, dl, &d) == FAQCS_E_INVAL, "text, def_pos, def_len: all or none");
    faqcs_batch nq = b, no = b;
    nq.qual = nullptr; no.offset = nullptr;
    CHECK(faqcs_detect_host(&nq, 0, 1, nullptr, nullptr, nullptr, &d) == FAQCS_E_INVAL && faqcs_detect_host(&no, 0, 1, nullptr, nullptr, nullptr, &d) == FAQCS_E_INVAL, "null arrays");
    CHECK(faqcs_detect_host(&nq, 1, 0, nullptr, nullptr, nullptr, &d) == 0 && d.read == 1 && d.quality_offset == 0, "count == 0 reads nothing");
    CHECK(faqcs_first_error_host(nullptr, 0, &e) == 0 && e.n_good == 0 && e.flags == 0, "n == 0");
    CHECK(faqcs_first_error_host(nullptr, 1, &e) == FAQCS_E_INVAL, "null results");
    faqcs_read_result r = {0, 0, 0, 0};
    CHECK(faqcs_first_error_host(&r, 1, nullptr) == FAQCS_E_INVAL, "null info");
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: detect_host_fuzz SEED N\n"); return 2; }
    g_state = strtoull(argv[1], nullptr, 0);
    const unsigned n = (unsigned)strtoul(argv[2], nullptr, 0);
    argument_checks();
    for (g_case = 0; g_case < n; ++g_case) { detect_case(); error_case(); }
    printf("%u cases: ok\n", n);
    return 0;
}
