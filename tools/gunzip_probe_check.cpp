// gunzip_probe_check.cpp -- the probe of the piece-wise gunzip against its decoder, and the catalogue of tests/gunzip_edges.py through the host
// passes, as plain host C++ for a build with AddressSanitizer and UBSan:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/gunzip_probe_check.cpp
//
// faqcs_gunzip.h states what a dynamic block's header may be three times: inflate_member (faqcs_inflate.h), gz_run's parser, and
// plausible_block, which decides where a grid piece may start.  A probe stricter than the decoder turns valid files into E_SERIAL, a looser
// one costs rounds; here the two are held against each other on block headers whose positions the test knows.
//   usage: gunzip_probe_check CORPUS        (the file tests/gunzip_edges.write_corpus() writes)
//   - probe entries {mode, stream, bit positions of block headers}: at every position whose three header bits read BFINAL = 0, BTYPE = 2,
//     plausible_block() against "gz_run<false> from there to the end of that block returns ST_OK".  A header the decoder takes and the
//     probe refuses fails in both modes.  The reverse fails in mode 0 (valid streams, and invalid ones whose fault is in the header);
//     mode 1 allows it: gz_run cannot be stopped at the header's end, and the fault of those streams lies behind it
//   - files {piece_bytes, verdict, members, text length and CRC-32, bytes}: gunzip_run over HostBackend, the compressed bytes a heap block of
//     exactly their size, the symbols and the text of exactly the total the chain states
//   - feeds {piece_bytes, verdict, text length and CRC-32, chunk ends, bytes}: the same through the carried State, every chunk a heap block
//     of its own, the window one of exactly 32 768 bytes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../faqcs_amd/csrc/faqcs_gunzip.h"

namespace gz = faqcs_gunzip;
namespace inf = faqcs_inflate;
typedef std::vector<uint8_t> Bytes;

static Bytes corpus;
static size_t at = 0;
static uint32_t get32()
{
    if (at + 4 > corpus.size()) { printf("FAIL: the corpus ends early\n"); exit(1); }
    uint32_t v;
    memcpy(&v, corpus.data() + at, 4);
    at += 4;
    return v;
}
static uint64_t get64() { const uint64_t lo = get32(); return lo | (uint64_t)get32() << 32; }
static std::unique_ptr<uint8_t[]> get_bytes(uint32_t n) // a heap block of exactly n bytes (one for none)
{
    if (at + n > corpus.size()) { printf("FAIL: the corpus ends early\n"); exit(1); }
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    memcpy(p.get(), corpus.data() + at, n);
    at += n;
    return p;
}

static uint32_t crc32_of(const uint8_t *p, size_t n, uint32_t crc = 0)
{
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xedb88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: gunzip_probe_check CORPUS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("FAIL: cannot open %s\n", argv[1]); return 1; }
    for (uint8_t buf[65536];;) {
        const size_t n = fread(buf, 1, sizeof buf, f);
        if (!n) break;
        corpus.insert(corpus.end(), buf, buf + n);
    }
    fclose(f);
    std::unique_ptr<inf::Tables> T(new inf::Tables);
    unsigned long long n_headers = 0, n_both = 0, n_neither = 0, n_behind = 0, n_other = 0;
    const uint32_t n_probe = get32();
    for (uint32_t e = 0; e < n_probe; ++e) {
        const uint32_t mode = get32(), n = get32();
        const std::unique_ptr<uint8_t[]> in = get_bytes(n);
        const uint32_t n_pos = get32();
        for (uint32_t k = 0; k < n_pos; ++k) {
            const uint64_t bit = get64();
            if ((bit >> 3) >= n) { printf("FAIL: entry %u: position %llu is behind the stream\n", e, (unsigned long long)bit); return 1; }
            if ((gz::peek(in.get(), n, bit) & 7u) != 4u) { ++n_other; continue; }
            ++n_headers;
            const bool probe = gz::plausible_block(in.get(), n, bit);
            inf::HostSink<uint16_t> S{nullptr};
            gz::Run r;
            gz::gz_run<false>(in.get(), n, bit, bit + 1, gz::NO_BIT, gz::NO_BIT, *T, S, r);
            const bool decoder = r.status == inf::ST_OK;
            if (decoder && !probe) { printf("FAIL: entry %u, bit %llu: the decoder takes the block, the probe refuses its header\n", e, (unsigned long long)bit); return 1; }
            if (probe && !decoder && mode == 0) {
                printf("FAIL: entry %u, bit %llu: the probe takes the header, the decoder refuses the block (status %u)\n", e, (unsigned long long)bit, r.status);
                return 1;
            }
            if (probe && decoder) ++n_both; else if (probe) ++n_behind; else ++n_neither;
        }
    }
    const uint32_t n_files = get32();
    for (uint32_t e = 0; e < n_files; ++e) {
        const uint32_t piece = get32(), error = get32(), n_members = get32(), n_text = get32(), crc = get32(), n = get32();
        const std::unique_ptr<uint8_t[]> in = get_bytes(n);
        gz::HostBackend B(n ? in.get() : nullptr, n, piece);
        gz::Info info;
        const int rc = gz::gunzip_run(B, n, piece, 4000, ~0ull >> 1, info);
        if (rc || info.overflow) { printf("FAIL: file %u at %u: gunzip_run returned %d, overflow %u\n", e, piece, rc, info.overflow); return 1; }
        if ((info.error != 0) != (error != 0) || info.n_members != n_members || info.n_bytes != n_text || crc32_of(B.text.data(), n_text) != crc) {
            printf("FAIL: file %u at %u: error %d, %u members, %llu bytes; expected %s, %u members, %u bytes, or the text differs\n", e, piece, info.error, info.n_members,
                   (unsigned long long)info.n_bytes, error ? "an error" : "none", n_members, n_text);
            return 1;
        }
    }
    const uint32_t n_feeds = get32();
    for (uint32_t e = 0; e < n_feeds; ++e) {
        const uint32_t piece = get32(), error = get32(), n_text = get32(), crc = get32(), n_ends = get32();
        std::vector<uint32_t> ends(n_ends);
        for (uint32_t &v : ends) v = get32();
        const uint32_t n = get32();
        const size_t file_at = at;
        at += n;
        ends.push_back(n);
        std::unique_ptr<uint8_t[]> window(new uint8_t[gz::WIN]);
        memset(window.get(), 0xEE, gz::WIN);
        gz::State st{0, 0, 0, gz::PH_BETWEEN, 0, 0, 0, 0, 0};
        uint32_t from = 0, got_crc = 0, last_error = 0;
        uint64_t got = 0;
        for (size_t c = 0; c < ends.size() && !last_error; ++c) {
            const uint32_t len = ends[c] - from;
            std::unique_ptr<uint8_t[]> chunk(new uint8_t[len ? len : 1]);
            memcpy(chunk.get(), corpus.data() + file_at + from, len);
            gz::HostBackend B(len ? chunk.get() : nullptr, len, piece);
            B.window = window.get();
            gz::Info info;
            const int rc = gz::gunzip_run(B, len, piece, 4000, ~0ull >> 1, info, &st, c + 1 == ends.size());
            if (rc || info.overflow) { printf("FAIL: feed %u, call %zu: gunzip_run returned %d, overflow %u\n", e, c, rc, info.overflow); return 1; }
            got_crc = crc32_of(B.text.data(), info.n_bytes, got_crc);
            got += info.n_bytes;
            from += (uint32_t)info.consumed;
            last_error = (uint32_t)info.error;
        }
        if ((last_error != 0) != (error != 0) || got != n_text || got_crc != crc) {
            printf("FAIL: feed %u at %u: error %u, %llu bytes; expected %s, %u bytes, or the text differs\n", e, piece, last_error, (unsigned long long)got, error ? "an error" : "none",
                   n_text);
            return 1;
        }
    }
    if (at != corpus.size()) { printf("FAIL: %zu bytes of the corpus are left over\n", corpus.size() - at); return 1; }
    printf("%llu headers: %llu taken by both, %llu by neither, %llu by the probe alone where the fault lies behind the header; %llu positions are no non-final dynamic block\n",
           n_headers, n_both, n_neither, n_behind, n_other);
    printf("%u files and %u feeds as zlib has them\n", n_files, n_feeds);
    return 0;
}
