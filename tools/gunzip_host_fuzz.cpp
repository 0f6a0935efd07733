// gunzip_host_fuzz.cpp -- the piece-wise gunzip of faqcs_gunzip_device (faqcs_amd/csrc/faqcs_gunzip.h) as plain host C++ against zlib, meant
// for a build with AddressSanitizer and UBSan:  g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/gunzip_host_fuzz.cpp -lz
//
// The header is the text the gfx950 kernels compile, so what holds here about its bounds holds for the device code's arithmetic: the
// compressed bytes are a heap block of EXACTLY n_comp bytes, the symbols and the text heap blocks of exactly the total the chain states,
// and the sanitizers see any access outside them.
//   usage: gunzip_host_fuzz SEED N
//   - N generated files of one to four members (FASTQ-like / random / one repeated byte / short periodic text of up to 300 KB; levels
//     0 1 6 9; all strategies; full flushes; FNAME / FCOMMENT / FEXTRA / FHCRC; trailing bytes that are not gzip) at piece sizes 1 024,
//     4 096 and the default: the text equals the input, every member is delivered, consumed is the whole input
//   - of each, damaged copies (bit flips, overwritten bytes, a changed trailer, a cut file): the members in front of the first one zlib
//     refuses are delivered with zlib's text, the call reports an error exactly when zlib does, and nothing outside the buffers is touched
#include <zlib.h>

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

static unsigned long long n_good = 0, n_refused = 0, n_harmless = 0, seen_code[8] = {0, 0, 0, 0, 0, 0, 0, 0};

static void check(const Bytes &f, uint32_t piece, bool pristine, const char *what)
{
    std::unique_ptr<uint8_t[]> in(new uint8_t[f.size() ? f.size() : 1]); // exactly the input
    memcpy(in.get(), f.data(), f.size());
    const Model md = zlib_model(f);
    gz::HostBackend B(f.size() ? in.get() : nullptr, f.size(), piece);
    gz::Info info;
    const int rc = gz::gunzip_run(B, f.size(), piece, 4096, ~0ull >> 1, info);
    if (rc) { printf("FAIL %s: gunzip_run returned %d\n", what, rc); exit(1); }
    ++seen_code[info.error < 8 ? info.error : 7];
    if (info.overflow) { printf("FAIL %s: overflow\n", what); exit(1); }
    if ((info.error != 0) != md.error || info.n_members != md.texts.size()) {
        printf("FAIL %s (piece %u): error %d of member %u, zlib %s behind %zu members\n", what, piece, info.error, info.n_members, md.error ? "refuses" : "accepts", md.texts.size());
        exit(1);
    }
    size_t at = 0;
    for (const Bytes &t : md.texts) {
        if (at + t.size() > info.n_bytes || (t.size() && memcmp(B.text.data() + at, t.data(), t.size()))) { printf("FAIL %s: the text of a delivered member differs\n", what); exit(1); }
        at += t.size();
    }
    if (at != info.n_bytes) { printf("FAIL %s: n_bytes %llu, zlib %zu\n", what, (unsigned long long)info.n_bytes, at); exit(1); }
    if (!md.error && info.consumed != md.consumed) { printf("FAIL %s: consumed %llu, zlib %zu\n", what, (unsigned long long)info.consumed, md.consumed); exit(1); }
    if (pristine) { if (md.error) { printf("FAIL %s: zlib refuses a generated file\n", what); exit(1); } ++n_good; }
    else if (md.error) ++n_refused; else ++n_harmless;
}

int main(int argc, char **argv)
{
    const unsigned long long seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int n = argc > 2 ? atoi(argv[2]) : 40;
    rng.seed(seed);
    const int levels[4] = {0, 1, 6, 9}, strategies[5] = {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, Z_FILTERED};
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
            const Bytes m = make_member(text, deflate_raw(text, levels[rnd(4)], strategies[rnd(5)], 1 + (int)rnd(9), fl), variant);
            file.insert(file.end(), m.begin(), m.end());
        }
        if (rnd(4) == 0) for (uint32_t k = 1 + rnd(9); k; --k) file.push_back((uint8_t)(rnd(2) ? 0 : 'x' + rnd(3)));
        const uint32_t piece = pieces[made % 3];
        check(file, piece, true, "generated");
        if (fhcrc) continue; // (zlib verifies FHCRC, the contract skips it: damaged copies of such a file have two yardsticks)
        for (int d = 0; d < 6; ++d) {
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
    printf("%d files equal to zlib's, %llu damaged copies refused where zlib refuses them, %llu harmless\n", n, n_refused, n_harmless);
    (void)n_good;
    return 0;
}
