// inflate_host_fuzz.cpp -- the decoder core of faqcs_inflate_device (faqcs_amd/csrc/faqcs_inflate.h) as plain host C++ against zlib, meant
// for a build with AddressSanitizer and UBSan:  g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/inflate_host_fuzz.cpp -lz
//
// The core is the text the gfx950 kernel compiles, so what holds here about its bounds holds for the device code's arithmetic: every input
// and output buffer below is a heap block of EXACTLY the size the decoder is told, and the sanitizers see any access outside it.
//   usage: inflate_host_fuzz SEED N
//   - N generated members (FASTQ-like / random / one repeated byte / short periodic text; levels 0 1 6 9; all strategies; full flushes in
//     the middle; optional FNAME / FCOMMENT / FHCRC / a subfield in front of BC; sizes 0 .. 65 536): the decoder's text equals the input,
//     its verdict is ST_OK
//   - of each, damaged copies (bit flips anywhere in the member, trailer changes, a cut deflate stream): the verdict is never ST_OK unless
//     zlib accepts the same bytes with the same text, CRC and length; whatever the bytes say, nothing outside the buffers is touched
//   - the BSIZE walk over the concatenation, cut at random places, with final = 0 / 1
//   usage: inflate_host_fuzz --corpus FILE
//   - FILE holds a count, then that many members, each behind its size (32-bit little-endian values): members written elsewhere -- the
//     catalogue of tests/deflate_streams.py, streams zlib's encoder never writes -- each through the same check as a damaged copy: the
//     verdict is ST_OK exactly when zlib accepts the bytes, then with zlib's text; nothing outside the exact-size buffers is touched
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../faqcs_amd/csrc/faqcs_inflate.h"

namespace inf = faqcs_inflate;
typedef std::vector<uint8_t> Bytes;

static std::mt19937_64 rng;
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0; }

static Bytes make_text(uint32_t n)
{
    Bytes t(n);
    switch (rnd(4)) {
    case 0: { // FASTQ-like
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
        break;
    }
    case 1: for (auto &b : t) b = (uint8_t)rng(); break;
    case 2: { const uint8_t v = (uint8_t)rng(); for (auto &b : t) b = v; break; }
    default: {
        const uint32_t p = 2 + rnd(10);
        uint8_t unit[12];
        for (auto &u : unit) u = (uint8_t)('A' + rnd(26));
        for (uint32_t i = 0; i < n; ++i) t[i] = unit[i % p];
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
        if (rc != Z_OK && rc != Z_BUF_ERROR) abort(); // (Z_BUF_ERROR: a second flush at the same place has nothing to do)
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

// empty when the member would not fit BSIZE
static Bytes make_member(const Bytes &text, const Bytes &raw, int variant)
{
    Bytes m = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255};
    Bytes front, tail;
    if (variant == 1) { front = {'Z', 'Z', 3, 0, 'a', 'b', 'c'}; }
    if (variant == 2) { m[3] |= 8; for (char c : std::string("reads.fq")) tail.push_back((uint8_t)c); tail.push_back(0); }
    if (variant == 3) { m[3] |= 16; for (char c : std::string("by hand")) tail.push_back((uint8_t)c); tail.push_back(0); }
    const bool fhcrc = variant == 4;
    if (fhcrc) m[3] |= 2;
    const size_t total = 12 + front.size() + 6 + tail.size() + (fhcrc ? 2 : 0) + raw.size() + 8;
    if (total > 65536) return Bytes();
    put16(m, (uint32_t)front.size() + 6);
    m.insert(m.end(), front.begin(), front.end());
    m.push_back('B'); m.push_back('C'); put16(m, 2); put16(m, (uint32_t)total - 1);
    m.insert(m.end(), tail.begin(), tail.end());
    if (fhcrc) put16(m, (uint32_t)crc32(0, m.data(), (uInt)m.size()) & 0xffffu);
    m.insert(m.end(), raw.begin(), raw.end());
    put32(m, (uint32_t)crc32(0, text.data(), (uInt)text.size()));
    put32(m, (uint32_t)text.size());
    return m;
}

// zlib on the same member: true and the text when it accepts stream, CRC and length (with the stream ending at the trailer)
static bool zlib_member(const uint8_t *p, size_t size, const inf::Member &mb, Bytes &text)
{
    z_stream z{};
    if (inflateInit2(&z, -15) != Z_OK) abort();
    text.assign(65536 + 1, 0);
    z.next_in = const_cast<uint8_t *>(p) + mb.data_begin; z.avail_in = mb.data_end - mb.data_begin;
    z.next_out = text.data(); z.avail_out = (uInt)text.size();
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.avail_in == 0 && z.total_out == mb.isize && (uint32_t)crc32(0, text.data(), (uInt)z.total_out) == mb.crc;
    text.resize(ok ? z.total_out : 0);
    inflateEnd(&z);
    (void)size;
    return ok;
}

static std::unique_ptr<inf::Tables> T;
static unsigned long long n_ok = 0, n_refused = 0, seen_code[6] = {0, 0, 0, 0, 0, 0};

// our verdict on exact-size heap copies; text: what was decoded when ST_OK
static int ours(const Bytes &m, Bytes &text)
{
    std::unique_ptr<uint8_t[]> in(new uint8_t[m.size() ? m.size() : 1]);
    memcpy(in.get(), m.data(), m.size());
    inf::Member mb;
    int st = inf::parse_member(in.get(), m.size(), mb);
    text.clear();
    if (st) return st;
    std::unique_ptr<uint8_t[]> out(new uint8_t[mb.isize ? mb.isize : 1]); // exactly ISIZE: a write beyond it is the sanitizer's
    st = inf::inflate_member_host(in.get(), m.size(), *T, out.get(), mb);
    if (!st) text.assign(out.get(), out.get() + mb.isize);
    return st;
}

static void check(const Bytes &m, const Bytes *want, const char *what)
{
    Bytes got, ztext;
    const int st = ours(m, got);
    ++seen_code[st];
    if (want) {
        if (st != inf::ST_OK || got != *want) { printf("FAIL %s: status %d on a good member of %zu bytes\n", what, st, m.size()); exit(1); }
        ++n_ok;
        return;
    }
    inf::Member mb;
    const bool hdr = inf::parse_member(m.data(), m.size(), mb) == inf::ST_OK;
    const bool zok = hdr && zlib_member(m.data(), m.size(), mb, ztext);
    if ((st == inf::ST_OK) != zok || (zok && got != ztext)) { printf("FAIL %s: status %d, zlib %s\n", what, st, zok ? "accepts" : "refuses"); exit(1); }
    if (st) ++n_refused; else ++n_ok;
}

static int run_corpus(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { printf("FAIL: cannot open %s\n", path); return 1; }
    uint8_t w[4];
    if (fread(w, 1, 4, f) != 4) { printf("FAIL: %s holds no count\n", path); return 1; }
    const uint32_t n = inf::le32(w);
    for (uint32_t i = 0; i < n; ++i) {
        if (fread(w, 1, 4, f) != 4) { printf("FAIL: %s ends in front of member %u\n", path, i); return 1; }
        Bytes m(inf::le32(w));
        if (m.size() > (1u << 20) || fread(m.data(), 1, m.size(), f) != m.size()) { printf("FAIL: %s ends inside member %u\n", path, i); return 1; }
        const std::string what = "corpus member " + std::to_string(i);
        check(m, nullptr, what.c_str());
    }
    fclose(f);
    printf("%u corpus members: %llu accepted with zlib's text, %llu refused as zlib refuses them\n", n, n_ok, n_refused);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 2 && !strcmp(argv[1], "--corpus")) {
        T.reset(new inf::Tables);
        inf::HostSink<uint8_t> S{nullptr};
        inf::crc_init(*T, S);
        return run_corpus(argv[2]);
    }
    const unsigned long long seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int n = argc > 2 ? atoi(argv[2]) : 100;
    rng.seed(seed);
    T.reset(new inf::Tables);
    inf::HostSink<uint8_t> S{nullptr};
    inf::crc_init(*T, S);
    const int levels[4] = {0, 1, 6, 9}, strategies[5] = {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, Z_FILTERED};
    const uint32_t sizes[6] = {0, 1, 2, 65280, 65535, 65536};
    Bytes file;
    std::vector<uint32_t> offs{0};
    int made = 0;
    while (made < n) {
        uint32_t size = rnd(10) == 0 ? sizes[rnd(6)] : rnd(3) ? rnd(4000) : rnd(65537);
        const Bytes text = make_text(size);
        std::vector<uint32_t> fl;
        if (size > 4 && rnd(4) == 0) { fl.push_back(rnd(size)); if (rnd(2)) fl.push_back(fl[0]); if (rnd(2)) fl.push_back(fl.back() + rnd(size - fl.back())); }
        const Bytes raw = deflate_raw(text, levels[rnd(4)], strategies[rnd(5)], 1 + (int)rnd(9), fl);
        const Bytes m = make_member(text, raw, (int)rnd(6));
        if (m.empty()) continue;
        ++made;
        check(m, &text, "generated");
        if (file.size() + m.size() < (1u << 22)) { file.insert(file.end(), m.begin(), m.end()); offs.push_back((uint32_t)file.size()); }
        for (int d = 0; d < 12; ++d) {
            Bytes b = m;
            const uint32_t kind = rnd(6);
            if (kind <= 2) { const uint32_t flips = 1 + rnd(3); for (uint32_t f = 0; f < flips; ++f) b[rnd((uint32_t)b.size())] ^= (uint8_t)(1u << rnd(8)); }
            else if (kind == 3) b[b.size() - 8 + rnd(8)] ^= (uint8_t)(1u << rnd(8));                        // the trailer
            else if (kind == 4 && raw.size() > 1) {                                                            // a cut stream (BSIZE made to fit)
                const uint32_t cut = 1 + rnd((uint32_t)raw.size() - 1);
                b.erase(b.end() - 8 - cut, b.end() - 8);
                for (size_t x = 12; x + 6 <= b.size(); ++x) if (b[x] == 'B' && b[x + 1] == 'C' && b[x + 2] == 2 && b[x + 3] == 0) { b[x + 4] = (uint8_t)(b.size() - 1); b[x + 5] = (uint8_t)((b.size() - 1) >> 8); break; }
            } else { const uint32_t at = 12 + rnd((uint32_t)b.size() - 12); b[at] = (uint8_t)rng(); }
            check(b, nullptr, "damaged");
        }
    }
    // the BSIZE walk: one call against cuts with final = 0 and the rest with final = 1; a truncated last member; trailing bytes
    const uint32_t nm = (uint32_t)offs.size() - 1;
    for (int round = 0; round < 200; ++round) {
        const size_t keep = round % 3 == 2 ? file.size() - 1 - rnd(20) : file.size();
        Bytes f(file.begin(), file.begin() + (long)keep);
        if (round % 3 == 1) { f.push_back('x'); f.push_back('y'); }
        std::unique_ptr<uint8_t[]> heap(new uint8_t[f.size() + 1]);
        memcpy(heap.get(), f.data(), f.size());
        std::vector<uint32_t> mo(nm + 2);
        inf::IndexInfo whole{};
        inf::bgzf_index(heap.get(), f.size(), 1, mo.data(), nm + 1, whole);
        const uint32_t want_n = round % 3 == 2 ? nm - 1 : nm;
        const int want_err = round % 3 == 2 ? inf::ST_E_TRUNCATED : inf::ST_OK;
        if (whole.n_members != want_n || whole.error != want_err || whole.overflow) { printf("FAIL index round %d: %u members, error %d\n", round, whole.n_members, whole.error); return 1; }
        for (uint32_t k = 0; k <= want_n; ++k) if (mo[k] != offs[k]) { printf("FAIL index round %d: offset %u\n", round, k); return 1; }
        size_t start = 0;
        uint32_t k = 0;
        const size_t cut = rnd((uint32_t)f.size() + 1);
        for (int part = 0; part < 2; ++part) {
            const size_t end = part ? f.size() : cut;
            if (end < start) continue;
            std::unique_ptr<uint8_t[]> piece(new uint8_t[end - start + 1]); // exactly the chunk
            memcpy(piece.get(), f.data() + start, end - start);
            std::vector<uint32_t> po(nm + 2);
            inf::IndexInfo ii{};
            inf::bgzf_index(piece.get(), end - start, part, po.data(), nm + 1, ii);
            for (uint32_t j = 0; j < ii.n_members; ++j, ++k) if (start + po[j + 1] != offs[k + 1]) { printf("FAIL chunked index round %d\n", round); return 1; }
            if (part && (ii.error != want_err || k != want_n)) { printf("FAIL chunked index round %d: %u members, error %d\n", round, k, ii.error); return 1; }
            start += ii.consumed;
        }
    }
    for (int c = 0; c < 5; ++c) if (!seen_code[c]) { printf("FAIL: status %d never came up\n", c); return 1; }
    printf("%d members equal to zlib's, %llu damaged copies refused, %llu harmless\n", made, n_refused, n_ok - (unsigned long long)made);
    return 0;
}
