// deflate_host_fuzz.cpp -- the encoder core of faqcs_deflate_device (faqcs_amd/csrc/faqcs_deflate.h) as host C++ under AddressSanitizer and
// UBSan: generated texts of every shape and member size, every buffer of exactly the stated size on the heap (so that one byte too far is
// an error), every member back through zlib's inflate and its CRC.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o deflate_host_fuzz tools/deflate_host_fuzz.cpp -lz
//   ./deflate_host_fuzz SEED N [dense]      (dense: the dense match finder, FAQCS_DEFLATE_DENSE, instead of the fast one)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
#include <zlib.h>

#include "../faqcs_amd/csrc/faqcs_deflate.h"

namespace def = faqcs_deflate;

static std::vector<uint8_t> make_text(std::mt19937_64 &rng, uint32_t shape, uint32_t n)
{
    std::vector<uint8_t> t(n);
    const uint32_t period = 2 + rng() % 700;
    for (uint32_t i = 0; i < n; ++i) {
        switch (shape) {
        case 0: t[i] = "ACGT"[rng() & 3]; break;                                   // bases
        case 1: t[i] = (uint8_t)rng(); break;                                      // random
        case 2: t[i] = 'Q'; break;                                                 // one byte
        case 3: t[i] = i < period ? (uint8_t)('A' + rng() % 26) : t[i - period]; break; // periodic
        case 4: t[i] = (i / 400) & 1 ? "FF:F,F#F"[rng() & 7] : "@A00789:123:HXYZ2DSXX:1:1101:"[i % 29]; break; // defline-like and quality-like stretches
        default: t[i] = (rng() % 10) ? (i ? t[i - 1] : 'x') : (uint8_t)rng(); break; // runs
        }
    }
    return t;
}

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    const bool dense = argc > 3 && !strcmp(argv[3], "dense");
    std::mt19937_64 rng(seed);
    std::unique_ptr<def::Work> W(new def::Work);
    def::HostExec X;
    static const uint32_t SIZES[] = {1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 260, 1023, 1024, 1025, 4096, 32768, 32769, 65279, 65280};
    unsigned long long n_stored = 0, n_bytes = 0, n_comp = 0;
    for (int r = 0; r < rounds; ++r) {
        const uint32_t n = r < 120 ? SIZES[r % 20] : (r % 5 == 0 ? 60000 + (uint32_t)(rng() % 5281) : 1 + (uint32_t)(rng() % 9000));
        const std::vector<uint8_t> text = make_text(rng, (uint32_t)(r % 6), n);
        // buffers of exactly the stated sizes: the text without padding, the tokens, the slot
        std::unique_ptr<uint8_t[]> in(new uint8_t[n]);
        memcpy(in.get(), text.data(), n);
        std::unique_ptr<uint32_t[]> tok(new uint32_t[(n + def::TILE - 1) / def::TILE * def::TILE]);
        const uint32_t slot_bytes = (n + def::SLACK + 15u) & ~15u;
        uint8_t *slot = (uint8_t *)aligned_alloc(16, slot_bytes);
        const uint32_t res = dense ? def::deflate_member<def::MODE_DENSE>(X, *W, in.get(), n, tok.get(), slot) : def::deflate_member(X, *W, in.get(), n, tok.get(), slot);
        const uint32_t size = res & 0x7fffffffu;
        if (size > n + def::SLACK || size < 26) { fprintf(stderr, "round %d: size %u for %u bytes\n", r, size, n); return 1; }
        if (faqcs_inflate::bgzf_member_size(slot, size) != size) { fprintf(stderr, "round %d: header\n", r); return 1; }
        std::vector<uint8_t> back(n + 1);
        z_stream z{};
        if (inflateInit2(&z, -15) != Z_OK) return 2;
        z.next_in = slot + 18; z.avail_in = size - 26;
        z.next_out = back.data(); z.avail_out = n + 1;
        const int rc = inflate(&z, Z_FINISH);
        const bool ok = rc == Z_STREAM_END && z.total_out == n && z.avail_in == 0 && !memcmp(back.data(), text.data(), n);
        inflateEnd(&z);
        if (!ok) { fprintf(stderr, "round %d (shape %d, %u bytes): zlib says %d, %lu bytes out, %u in left\n", r, r % 6, n, rc, z.total_out, z.avail_in); return 1; }
        if (faqcs_inflate::le32(slot + size - 8) != (uint32_t)crc32(0, text.data(), n) || faqcs_inflate::le32(slot + size - 4) != n) { fprintf(stderr, "round %d: trailer\n", r); return 1; }
        n_stored += res >> 31; n_bytes += n; n_comp += size;
        free(slot);
    }
    printf("%d texts came back through zlib (%llu bytes as %llu, %llu stored)\n", rounds, n_bytes, n_comp, n_stored);
    return 0;
}
