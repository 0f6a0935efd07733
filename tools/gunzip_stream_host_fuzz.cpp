// gunzip_stream_host_fuzz.cpp -- the streamed gunzip of faqcs_gunzip_stream_device (faqcs_amd/csrc/faqcs_gunzip.h: gunzip_run with a
// carried State) as plain host C++ against zlib, meant for a build with AddressSanitizer and UBSan:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/gunzip_stream_host_fuzz.cpp -lz
//
// As tools/gunzip_host_fuzz.cpp does for the single call: the header is the text the gfx950 kernels compile; every chunk is a heap block of
// EXACTLY its bytes, the symbols (the front of 32 768 and the call's total) and the text heap blocks of exactly what the chain states, the
// window a heap block of exactly 32 768, and the sanitizers see any access outside them.
//   usage: gunzip_stream_host_fuzz SEED N
//   - N generated files of one to four members (texts of up to 300 KB; zlib levels 0 .. 9; all strategies; full flushes; FNAME / FCOMMENT /
//     FEXTRA / FHCRC; trailing bytes that are not gzip) at piece sizes 1 024, 4 096 and the default, each fed several times at random
//     chunk ends (none, a few, many): the concatenated text equals zlib's, and behind EVERY call state.crc is zlib's crc32 of the open
//     member's text so far, the window that text's last bytes, the counters their sums
//   - of each, damaged copies (bit flips, overwritten bytes, a changed trailer, a cut file) fed the same way: the completed members carry
//     zlib's text, the feed ends with an error exactly when zlib does, and a call that states an error of the member that was open at
//     entry leaves the state as it was
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../faqcs_amd/csrc/faqcs_gunzip.h"

namespace gz = faqcs_gunzip;
typedef std::vector<uint8_t> Bytes;

static std::mt19937_64 rng;
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0; }

static Bytes make_text(uint32_t n)
{
    Bytes t(n);
    switch (rnd(6)) {
    case 0: for (auto &b : t) b = (uint8_t)rng(); break;
    case 1: { const uint8_t v = (uint8_t)rng(); for (auto &b : t) b = v; break; }
    case 2: {
        const uint32_t p = 2 + rnd(10);
        uint8_t unit[12];
        for (auto &u : unit) u = (uint8_t)('A' + rnd(26));
        for (uint32_t i = 0; i < n; ++i) t[i] = unit[i % p];
        break;
    }
    default: { // FASTQ-like
        const char bases[] = "ACGTN";
        uint32_t i = 0, rec = 0;
        while (i < n) {
            char def[64];
            const int dl = snprintf(def, sizeof def, "@r%u len=%u\n", rec++, 100 + rnd(100));
            for (int k = 0; k < dl && i < n; ++k) t[i++] = (uint8_t)def[k];
            const uint32_t L = 20 + rnd(200);
            for (uint32_t k = 0; k < L && i < n; ++k) t[i++] = (uint8_t)bases[rnd(100) < 4 ? 4 : rnd(4)];
            const char *plus = "\n+\n";
            for (int k = 0; k < 3 && i < n; ++k) t[i++] = (uint8_t)plus[k];
            for (uint32_t k = 0; k < L && i < n; ++k) t[i++] = (uint8_t)(33 + rnd(42));
            if (i < n) t[i++] = '\n';
        }
    }
    }
    return t;
}

static Bytes deflate_raw(const Bytes &text, int level, int strategy, int mem_level, const std::vector<uint32_t> &flush_at)
{
    z_stream z{};
    if (deflateInit2(&z, level, Z_DEFLATED, -15, mem_level, strategy) != Z_OK) abort();
    Bytes out(deflateBound(&z, (uLong)text.size()) + 64 + 16 * flush_at.size());
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    uint32_t a = 0;
    for (uint32_t c : flush_at) {
        z.next_in = const_cast<uint8_t *>(text.data()) + a; z.avail_in = c - a;
        const int rc = deflate(&z, Z_FULL_FLUSH);
        if (rc != Z_OK && rc != Z_BUF_ERROR) abort();
        a = c;
    }
    z.next_in = const_cast<uint8_t *>(text.data()) + a; z.avail_in = (uInt)text.size() - a;
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

static void put16(Bytes &b, uint32_t v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
static void put32(Bytes &b, uint32_t v) { put16(b, v & 0xffffu); put16(b, v >> 16); }

static Bytes make_member(const Bytes &text, const Bytes &raw, int variant)
{
    Bytes m = {31, 139, 8, 0, 1, 2, 3, 4, 2, 3};
    if (variant == 1) { m[3] |= 4; put16(m, 7); for (char c : std::string("ZZ\3\0abc", 7)) m.push_back((uint8_t)c); }
    if (variant == 2 || variant == 5) { m[3] |= 8; for (char c : std::string("reads.fq")) m.push_back((uint8_t)c); m.push_back(0); }
    if (variant == 3 || variant == 5) { m[3] |= 16; for (char c : std::string("by hand")) m.push_back((uint8_t)c); m.push_back(0); }
    if (variant == 4) { m[3] |= 2; put16(m, (uint32_t)crc32(0, m.data(), (uInt)m.size()) & 0xffffu); }
    m.insert(m.end(), raw.begin(), raw.end());
    put32(m, (uint32_t)crc32(0, text.data(), (uInt)text.size()));
    put32(m, (uint32_t)text.size());
    return m;
}

// zlib on the same bytes, member by member as gzread goes: the texts of the members it accepts whole, and whether it ends with an error
struct Model { std::vector<Bytes> texts; bool error; size_t consumed; };
static Model zlib_model(const Bytes &f)
{
    Model md{{}, false, 0};
    size_t p = 0;
    while (p < f.size()) {
        if (f[p] != 31 || (p + 1 < f.size() && f[p + 1] != 139)) { p = f.size(); break; } // not gzip: the data ends
        z_stream z{};
        if (inflateInit2(&z, 15 + 16) != Z_OK) abort();
        Bytes text(1u << 16);
        z.next_in = const_cast<uint8_t *>(f.data()) + p; z.avail_in = (uInt)(f.size() - p);
        int rc;
        for (;;) {
            if (z.total_out == text.size()) text.resize(2 * text.size());
            z.next_out = text.data() + z.total_out; z.avail_out = (uInt)(text.size() - z.total_out);
            rc = inflate(&z, Z_NO_FLUSH);
            if (rc != Z_OK) break;
            if (z.avail_in == 0 && z.avail_out) { rc = Z_BUF_ERROR; break; }
        }
        const bool ok = rc == Z_STREAM_END;
        if (ok) { text.resize(z.total_out); md.texts.push_back(text); p = f.size() - z.avail_in; }
        inflateEnd(&z);
        if (!ok) { md.error = true; break; }
    }
    md.consumed = p;
    return md;
}

static unsigned long long n_calls = 0, n_refused = 0, n_harmless = 0, n_carried_errors = 0, seen_phase[3] = {0, 0, 0}, seen_code[8] = {0, 0, 0, 0, 0, 0, 0, 0};

#define FAIL(...) do { printf("FAIL %s (piece %u, call %zu at %zu): ", what, piece, k, at); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

// one feed of f at the chunk ends `ends` (ascending; the rest goes with final = 1)
static void feed(const Bytes &f, const Model &md, std::vector<size_t> ends, uint32_t piece, const char *what)
{
    std::unique_ptr<uint8_t[]> window(new uint8_t[gz::WIN]); // exactly the window
    memset(window.get(), 0xee, gz::WIN);
    gz::State st{0, 0, 0, gz::PH_BETWEEN, 0, 0, 0, 0, 0};
    Bytes got;
    size_t at = 0, k = 0;
    ends.push_back(f.size());
    int32_t error = 0;
    for (; k < ends.size(); ++k) {
        const size_t end = ends[k] < f.size() ? ends[k] : f.size(), n = end - at;
        const bool final = k + 1 == ends.size();
        std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]); // exactly the chunk
        memcpy(in.get(), f.data() + at, n);
        gz::HostBackend B(n ? in.get() : nullptr, n, piece);
        B.window = window.get();
        const gz::State before = st;
        Bytes wbefore(window.get(), window.get() + gz::WIN);
        gz::Info info;
        const int rc = gz::gunzip_run(B, n, piece, 4096, ~0ull >> 1, info, &st, final);
        ++n_calls;
        if (rc) FAIL("gunzip_run returned %d", rc);
        if (info.overflow) FAIL("overflow");
        if (info.consumed > n) FAIL("consumed %llu of %zu", (unsigned long long)info.consumed, n);
        got.insert(got.end(), B.text.begin(), B.text.begin() + (info.n_bytes <= B.text.size() ? info.n_bytes : B.text.size()));
        if (st.total_bytes != got.size() || st.total_comp != at + info.consumed || st.members != before.members + info.n_members || st.reserved) FAIL("the counters");
        if (st.members > md.texts.size()) FAIL("%u members, zlib %zu", st.members, md.texts.size());
        size_t done = 0;
        for (uint32_t m = 0; m < st.members; ++m) done += md.texts[m].size();
        if (done + st.member_bytes != got.size()) FAIL("member_bytes %llu", (unsigned long long)st.member_bytes);
        size_t o = 0;
        for (uint32_t m = 0; m < st.members; ++m) { // the completed members: zlib's text
            if (md.texts[m].size() && memcmp(got.data() + o, md.texts[m].data(), md.texts[m].size())) FAIL("the text of member %u differs", m);
            o += md.texts[m].size();
        }
        if (st.members < md.texts.size()) { // the open member is one that zlib accepts: a prefix of its text
            if (st.member_bytes > md.texts[st.members].size() || (st.member_bytes && memcmp(got.data() + done, md.texts[st.members].data(), st.member_bytes))) FAIL("the open member's text differs");
        }
        const uint32_t want_crc = st.phase == gz::PH_BETWEEN ? 0u : (uint32_t)crc32(0, got.data() + done, (uInt)st.member_bytes);
        if (st.crc != want_crc) FAIL("crc %08x, zlib %08x", st.crc, want_crc);
        const uint32_t wb = st.member_bytes < gz::WIN ? (uint32_t)st.member_bytes : gz::WIN;
        if (st.window_bytes != wb || (wb && memcmp(window.get() + gz::WIN - wb, got.data() + got.size() - wb, wb))) FAIL("the window");
        if (st.phase > 2 || st.bit > 7 || (st.bit && st.phase != gz::PH_STREAM) || (st.phase == gz::PH_BETWEEN && st.member_bytes)) FAIL("phase %u bit %u", st.phase, st.bit);
        ++seen_phase[st.phase];
        if (info.error) {
            if (before.phase != gz::PH_BETWEEN && info.n_members == 0) { // of the member that was open at entry
                ++n_carried_errors;
                if (info.consumed || info.n_bytes || memcmp(&before, &st, sizeof st) || memcmp(wbefore.data(), window.get(), gz::WIN)) FAIL("an error of the open member moved the state");
            }
            error = info.error;
            break;
        }
        if (!final && !info.consumed && !info.n_bytes && memcmp(&before, &st, sizeof st)) FAIL("no progress, and the state changed");
        at += info.consumed;
    }
    ++seen_code[error < 8 ? error : 7];
    if ((error != 0) != md.error) { k = ends.size(); FAIL("error %d, zlib %s behind %zu members", error, md.error ? "refuses" : "accepts", md.texts.size()); }
    if (st.members != md.texts.size()) FAIL("%u members, zlib %zu", st.members, md.texts.size());
    if (!md.error && (st.total_comp != md.consumed || st.phase != gz::PH_BETWEEN)) FAIL("consumed %llu, zlib %zu", (unsigned long long)st.total_comp, md.consumed);
}

static void check(const Bytes &f, uint32_t piece, bool pristine, const char *what)
{
    const Model md = zlib_model(f);
    if (pristine && md.error) { printf("FAIL %s: zlib refuses a generated file\n", what); exit(1); }
    if (!pristine) ++(md.error ? n_refused : n_harmless);
    const uint32_t n = (uint32_t)f.size();
    for (int round = 0; round < (pristine ? 4 : 2); ++round) {
        std::vector<size_t> ends;
        const uint32_t cuts = round == 0 ? 0 : round == 1 ? 1 + rnd(3) : round == 2 ? 8 + rnd(24) : 2;
        for (uint32_t c = 0; c < cuts && n; ++c) ends.push_back(rnd(n));
        if (round == 3 && n > 20) { ends[0] = n - 1 - rnd(12); ends[1] = rnd(20); } // around the trailer and inside the first header
        std::sort(ends.begin(), ends.end());
        feed(f, md, ends, piece, what);
    }
}

int main(int argc, char **argv)
{
    const unsigned long long seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int n = argc > 2 ? atoi(argv[2]) : 30;
    rng.seed(seed);
    const int strategies[5] = {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, Z_FILTERED};
    const uint32_t pieces[3] = {1024, 4096, 0};
    for (int made = 0; made < n; ++made) {
        Bytes file;
        const uint32_t n_members = 1 + rnd(4);
        bool fhcrc = false;
        for (uint32_t k = 0; k < n_members; ++k) {
            const uint32_t size = rnd(8) == 0 ? rnd(3) : rnd(3) ? rnd(20000) : rnd(300000);
            const Bytes text = make_text(size);
            std::vector<uint32_t> fl;
            if (size > 4 && rnd(4) == 0) { fl.push_back(rnd(size)); if (rnd(2)) fl.push_back(fl[0]); if (rnd(2)) fl.push_back(fl.back() + rnd(size - fl.back())); }
            const int variant = (int)rnd(7);
            fhcrc |= variant == 4;
            const Bytes m = make_member(text, deflate_raw(text, (made + (int)k) % 10, strategies[rnd(5)], 1 + (int)rnd(9), fl), variant);
            file.insert(file.end(), m.begin(), m.end());
        }
        if (rnd(4) == 0) for (uint32_t k = 1 + rnd(9); k; --k) file.push_back((uint8_t)(rnd(2) ? 0 : 'x' + rnd(3)));
        const uint32_t piece = pieces[made % 3];
        check(file, piece, true, "generated");
        if (fhcrc) continue; // (zlib verifies FHCRC, the contract skips it: damaged copies of such a file have two yardsticks)
        for (int d = 0; d < 4; ++d) {
            Bytes b = file;
            const uint32_t kind = rnd(5);
            if (kind <= 1) { const uint32_t flips = 1 + rnd(3); for (uint32_t f = 0; f < flips; ++f) b[rnd((uint32_t)b.size())] ^= (uint8_t)(1u << rnd(8)); }
            else if (kind == 2) b[10 + rnd((uint32_t)b.size() - 10)] = (uint8_t)rng();
            else if (kind == 3) b.resize(1 + rnd((uint32_t)b.size() - 1));
            else b[b.size() - 1 - rnd(b.size() > 40 ? 40 : (uint32_t)b.size())] ^= (uint8_t)(1u << rnd(8));
            check(b, piece, false, "damaged");
        }
    }
    for (int c : {0, 3, 4, 5}) if (!seen_code[c]) { printf("FAIL: status %d never came up\n", c); return 1; }
    for (int p = 0; p < 3; ++p) if (!seen_phase[p]) { printf("FAIL: phase %d never came up\n", p); return 1; }
    if (!n_carried_errors) { printf("FAIL: no error of a member that was open at entry\n"); return 1; }
    printf("%d files equal to zlib's over %llu calls, %llu damaged copies refused where zlib refuses them, %llu harmless, %llu errors of a carried member\n", n, n_calls,
           n_refused, n_harmless, n_carried_errors);
    return 0;
}
