// faqcs_deflate.h -- the encoder core of faqcs_deflate_device / faqcs_deflate_host (include/faqcs_mi.h): one BGZF
// member from at most 65 280 bytes of text.  The SAME text compiles for the host (faqcs_host.cpp: faqcs_deflate_host;
// tools/deflate_host_fuzz.cpp under the sanitizers) and for gfx950 (faqcs_deflate_kernel.hip), the way faqcs_inflate.h does, and the bytes it
// produces are a function of the text alone: every step is either per-position work whose result does not depend on who does it, or a
// commutative update (max, add, or) of a shared word, or serial work of lane 0.  No HIP call, no zlib.
//
// The member, step by step (Work is the member's workspace: LDS on the device, the heap on the host):
//   stage      the text into Work::text (zeros behind it), its CRC-32 by the 64 slices of faqcs_inflate.h, the byte histogram and from it
//              the cost of a literal in eighths of a bit
//   per TILE   of 1 024 positions, in order:
//     find     the candidates of position p are (a) the latest position of a tile IN FRONT of p's tile whose three bytes hash as p's do
//              (head[] holds it: the positions of a tile enter head[] by max, behind a barrier, after the tile has looked its own up) and
//              (b) p - 1, the run candidate.  The longer match wins, the nearer on a tie; one that reaches farther back than 32 768 or in
//              front of the member is refused, and so is one that costs more bits than the literals it replaces are expected to.
//     parse    the greedy parse: next(p) = p + max(1, len(p)), and the token starts are the positions reachable from the tile's entry
//              (where the last token of the tile in front ended).  Reachability is marked by pointer jumping -- 10 doublings -- which
//              gives exactly the set a serial walk gives.
//     tokens   every token start writes its token to tok[p] (global scratch: 4 bytes per position) and counts its symbols
//   MODE_DENSE replaces `find` (deflate_member<MODE_DENSE>; MODE_FAST is everything above, untouched).  The tile is looked up and entered in
//   SUB-TILES of 256 positions, in order, so that the tables a position sees hold exactly the positions in front of its own sub-tile:
//     find     four lanes per position, one candidate each: (a) head16[0], the latest such position whose three bytes hash as p's do, (b)
//              head16[1], the latest whose EIGHT bytes hash as p's do (12 bits of a 64-bit multiplicative hash; only positions with p + 8 <=
//              n enter or look up), (c) p - 1; the fourth lane rests.  One farther back than 32 768 is refused by itself.  A barrier; then
//              the position keeps the longest, the nearest on a tie, if it pays (the same test), and enters both tables by a max on half
//              a word (positions + 1 fit 16 bits: two tables of 4 096 lie where head[] does).  A barrier.
//     lazy     on the lengths of the WHOLE tile as find left them: len(i) > 0, i < 1 023 and len(i + 1) > len(i) flag position i; behind a
//              barrier the flagged positions become literals (a rising chain gives way but for its last; never across two tiles)
//   and the parse goes on as above: next(p) is still a function of p.
//   codes      length-limited canonical codes (15 / 15 / 7 bits) of the literal-length, distance and code-length alphabets: a rank sort by
//              all lanes, then lane 0: the in-place minimum-redundancy lengths of Moffat and Katajainen over the sorted weights, the
//              limit by moving leaves down one level at a time until the Kraft sum fits, lengths handed out in sorted order
//   choose     the exact size of the dynamic block, of the fixed block and of the stored block; the smallest wins, the stored block on a tie
//   place      the member's IMAGE -- header, stream, trailer -- is assembled in Work::img: the bits of token k start at the exclusive prefix
//              of the token bit lengths (the executor's scan) and are ORed into the zeroed image; the image leaves as 16-byte pieces
//
// An executor X is who runs it: one host thread (lanes() == 1) or one block of TILE threads.  It supplies
//     lane(), lanes()               who I am
//     sync()                        a barrier: what any lane wrote is visible to every lane behind it
//     uni(v)                        v, known to be the same in every lane
//     amax(p, v) aadd(p, v) aor(p, v) axor(p, v)   atomic max / add / or / xor on a word of Work
//     amax16(a, i, v)               atomic max on a[i], half a word of Work (a: a 4-byte aligned array)
//     excl_scan(a)                  a[0 .. TILE) becomes its exclusive prefix sum; returns the total (barriers inside)
//     store16(dst, src)             16 bytes from Work to the member's slot
#pragma once
#include "faqcs_inflate.h"

namespace faqcs_deflate {

namespace inf = faqcs_inflate;

enum { MAX_TEXT = 65280, TILE = 1024, HASH_BITS = 12, MIN_MATCH = 3, MAX_MATCH = 258, MAX_DIST = 32768, HEADER = 18, TRAILER = 8,
       SLACK = HEADER + 5 + TRAILER, // a member is never larger than its text + 31
       N_LIT = 288, N_DIST = 32, N_CL = 19, EOF_BYTES = 28,
       MATCH_BASE_BITS = 12,         // what a match is expected to cost in front of its extra bits: a length code of 7 and a distance code of 5
       SURE_LENGTH = 32,             // a match this long always pays: a literal costs a bit at least, a match 30 at most
       SUB = 256 };                  // the dense mode looks a tile up, and enters it, in sub-tiles of this many positions
enum { MODE_FAST = 0, MODE_DENSE = 1 }; // FAQCS_DEFLATE_FAST / FAQCS_DEFLATE_DENSE of include/faqcs_mi.h
enum { KIND_STORED = 0, KIND_FIXED = 1, KIND_DYNAMIC = 2 };
constexpr uint32_t NO_TOKEN = 0xffffffffu;

// a token: a literal is its byte, a match is length << 16 | distance
struct Work {
    uint32_t text[MAX_TEXT / 4 + 2];             // the member's text, two zero words behind it (load32 reads a word ahead)
    uint32_t img[(MAX_TEXT + SLACK + 15) / 16 * 4]; // the member's image; in front of `place`, an inf::Tables for the CRC lies here
    union {
        uint32_t head[1 << HASH_BITS];           // find: position + 1 of the latest occurrence of a hash in the tiles in front, 0 = none
        uint16_t head16[2][1 << HASH_BITS];      // the dense find (position + 1 <= 65 280): [0] by three bytes, [1] by eight, the sub-tiles in front
        struct {                                 // codes, choose, place
            uint32_t weight[N_LIT];
            uint16_t sorted[N_LIT];
            uint16_t cl_token[N_LIT + N_DIST];   // the run-length coded code lengths: symbol | extra value << 8
            uint16_t lit_code[N_LIT], dist_code[N_DIST], cl_code[N_CL + 1];
        } c;
    } u;
    union {
        struct {                                 // parse
            uint32_t match[TILE];
            union { uint16_t next[2][TILE + 2]; uint32_t cand[3][SUB]; }; // (cand: the dense find's matches of a sub-tile, one row per candidate)
            uint8_t reach[TILE + 8];             // (the dense mode keeps the lazy step's flags here until the parse starts)
        } p;
        uint32_t bits[TILE];                     // place: the bit lengths of a tile's tokens, then their prefix
    } t;
    uint32_t byte_count[256];
    uint16_t lit_cost[256];                      // eighths of a bit
    uint32_t lit_count[N_LIT], dist_count[N_DIST], cl_count[N_CL + 1];
    uint8_t lit_len[N_LIT], dist_len[N_DIST], cl_len[N_CL + 1];
    uint32_t extra_bits, entry, entry_next, crc, kind, n_cl_token, n_lit, n_dist, n_cl, stream_bits, size;
};

#if defined(__HIPCC__)
#define DEF_HD __host__ __device__ __forceinline__
#else
#define DEF_HD static inline
#endif

DEF_HD uint32_t msb(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); } // x != 0
DEF_HD uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// the 4 bytes at byte position i of an array of words (little endian), whatever i's alignment: two aligned words and a shift
DEF_HD uint32_t load32(const uint32_t *w, uint32_t i)
{
    const uint64_t v = (uint64_t)w[i >> 2] | (uint64_t)w[(i >> 2) + 1] << 32;
    return (uint32_t)(v >> (8u * (i & 3u)));
}
DEF_HD uint32_t load8(const uint32_t *w, uint32_t i) { return (w[i >> 2] >> (8u * (i & 3u))) & 255u; }

DEF_HD uint32_t hash3(uint32_t w) { return ((w & 0xffffffu) * 0x9e3779b1u) >> (32 - HASH_BITS); }
DEF_HD uint32_t hash8(uint32_t lo, uint32_t hi) { return (uint32_t)((((uint64_t)hi << 32 | lo) * 0x9e3779b97f4a7c15ull) >> (64 - HASH_BITS)); }

// how many bytes at p and at c < p agree, at most `most` (p + most <= the text's length): dwords, and the first differing byte by its bit
DEF_HD uint32_t match_length(const uint32_t *text, uint32_t p, uint32_t c, uint32_t most)
{
    uint32_t l = 0;
    while (l + 4 <= most) {
        const uint32_t x = load32(text, p + l) ^ load32(text, c + l);
        if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
        l += 4;
    }
    while (l < most && load8(text, p + l) == load8(text, c + l)) ++l;
    return l;
}

// RFC 1951 section 3.2.5 as shifts, the inverse of faqcs_inflate::length_code / distance_code: symbol, extra bits and their value
DEF_HD void length_symbol(uint32_t len, uint32_t &c, uint32_t &extra, uint32_t &value)
{
    const uint32_t x = len - 3;
    if (len == 258) { c = 28; extra = 0; value = 0; }
    else if (x < 8) { c = x; extra = 0; value = 0; }
    else { extra = msb(x) - 2; c = 4 * extra + 4 + ((x >> extra) & 3u); value = x & ((1u << extra) - 1u); }
}
DEF_HD void distance_symbol(uint32_t dist, uint32_t &c, uint32_t &extra, uint32_t &value)
{
    const uint32_t x = dist - 1;
    if (x < 4) { c = x; extra = 0; value = 0; }
    else { extra = msb(x) - 1; c = 2 * extra + 2 + ((x >> extra) & 1u); value = x & ((1u << extra) - 1u); }
}

// 8 log2(x), the mantissa linear between the powers of two (x >= 1)
DEF_HD uint32_t log2_eighths(uint32_t x)
{
    const uint32_t e = msb(x);
    return 8 * e + ((e >= 3 ? x >> (e - 3) : x << (3 - e)) & 7u);
}

// does the match (len, dist) at p pay?  One under SURE_LENGTH bytes does when the literals it replaces are expected to cost more bits than it
DEF_HD bool match_pays(const uint32_t *text, const uint16_t *lit_cost, uint32_t p, uint32_t len, uint32_t dist)
{
    uint32_t lc, le, lv, dc, de, dv, lits = 0;
    length_symbol(len, lc, le, lv);
    distance_symbol(dist, dc, de, dv);
    for (uint32_t k = 0; k < len; ++k) lits += lit_cost[load8(text, p + k)];
    return lits > 8 * (MATCH_BASE_BITS + le + de);
}

DEF_HD uint32_t fixed_lit_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

DEF_HD uint32_t eof_byte(uint32_t i) // the 28-byte member bgzip ends a file with
{
    return i == 0 ? 0x1fu : i == 1 ? 0x8bu : i == 2 ? 8u : i == 3 ? 4u : i == 9 ? 0xffu : i == 10 ? 6u : i == 12 ? 'B' : i == 13 ? 'C' : i == 14 ? 2u
         : i == 16 ? 0x1bu : i == 18 ? 3u : 0u;
}

// `nb` (<= 32) bits of v at bit position `at` of the zeroed image
template <class X> DEF_HD void put_bits(X &x, uint32_t *img, uint32_t at, uint32_t v, uint32_t nb)
{
    if (!nb) return;
    const uint64_t t = (uint64_t)v << (at & 31u);
    x.aor(&img[at >> 5], (uint32_t)t);
    if (t >> 32) x.aor(&img[(at >> 5) + 1], (uint32_t)(t >> 32));
}

// The lengths of a code of at most `limit` bits for the weights w[0 .. n) (0 = unused symbol).  No used symbol: symbol 0 gets one bit (the
// distance set of a member without a match); one: it gets one bit, and with `two` a second symbol does too (the code-length code must be
// complete).  Whole block; the result is in lens[] behind the call's last barrier.
template <class X> DEF_HD void code_lengths(X &x, Work &W, const uint32_t *w, uint32_t n, uint32_t limit, uint8_t *lens, bool two)
{
    x.sync();
    for (uint32_t s = x.lane(); s < n; s += x.lanes()) {
        lens[s] = 0;
        if (w[s]) { // the rank of (w[s], s) among the used symbols
            uint32_t r = 0;
            for (uint32_t t = 0; t < n; ++t) r += (w[t] && (w[t] < w[s] || (w[t] == w[s] && t < s))) ? 1u : 0u;
            W.u.c.sorted[r] = (uint16_t)s;
        }
    }
    x.sync();
    if (x.lane() == 0) {
        uint32_t m = 0;
        for (uint32_t s = 0; s < n; ++s) m += w[s] ? 1u : 0u;
        uint32_t *A = W.u.c.weight;
        const uint16_t *S = W.u.c.sorted;
        if (m == 0) lens[0] = 1;
        else if (m == 1) { lens[S[0]] = 1; if (two) lens[S[0] ? 0 : 1] = 1; }
        else {
            for (uint32_t i = 0; i < m; ++i) A[i] = w[S[i]];
            // Moffat and Katajainen, "In-place calculation of minimum-redundancy codes": weights ascending in, code lengths out
            A[0] += A[1];
            uint32_t root = 0, leaf = 2;
            for (uint32_t next = 1; next + 1 < m; ++next) {
                if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
                if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
            }
            A[m - 2] = 0;
            for (int next = (int)m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
            int avail = 1, used = 0, rt = (int)m - 2, nx = (int)m - 1;
            uint32_t depth = 0;
            while (avail > 0) {
                while (rt >= 0 && A[rt] == depth) { ++used; --rt; }
                while (avail > used) { A[nx--] = depth; --avail; }
                avail = 2 * used; ++depth; used = 0;
            }
            // the limit: leaves deeper than it come up to it, which over-subscribes the code by `over` codes of `limit` bits; one step
            // takes one of them away: a leaf above the last level becomes an inner node over itself and a leaf taken from the last level
            uint32_t cnt[16];
            for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
            for (uint32_t i = 0; i < m; ++i) ++cnt[umin(A[i], limit)];
            uint32_t total = 0;
            for (uint32_t l = 1; l <= limit; ++l) total += cnt[l] << (limit - l);
            for (; total > (1u << limit); --total) {
                uint32_t l = limit - 1;
                while (!cnt[l]) --l;
                --cnt[l]; cnt[l + 1] += 2; --cnt[limit];
            }
            // the rarest symbols get the longest codes
            uint32_t l = limit;
            for (uint32_t i = 0; i < m; ++i) {
                while (!cnt[l]) --l;
                lens[S[i]] = (uint8_t)l; --cnt[l];
            }
        }
    }
    x.sync();
}

// the canonical code of lens[0 .. n), bit-reversed for a stream that fills bytes from bit 0.  Lane 0.
DEF_HD void canonical_codes(const uint8_t *lens, uint32_t n, uint16_t *code)
{
    uint32_t cnt[16], next[16];
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++cnt[lens[s]];
    uint32_t c = 0;
    cnt[0] = 0; next[0] = 0;
    for (uint32_t l = 1; l < 16; ++l) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
    for (uint32_t s = 0; s < n; ++s) code[s] = lens[s] ? (uint16_t)inf::bit_reverse(next[lens[s]]++, lens[s]) : (uint16_t)0;
}

// the bits of a token under the chosen codes: value (filled from bit 0) and length, at most 48
DEF_HD uint32_t token_bits(const Work &W, uint32_t tok, uint64_t &v)
{
    if (tok < 256) { v = W.u.c.lit_code[tok]; return W.lit_len[tok]; }
    uint32_t lc, le, lv, dc, de, dv;
    length_symbol(tok >> 16, lc, le, lv);
    distance_symbol(tok & 0xffffu, dc, de, dv);
    uint32_t nb = W.lit_len[257 + lc];
    v = W.u.c.lit_code[257 + lc];
    v |= (uint64_t)lv << nb; nb += le;
    v |= (uint64_t)W.u.c.dist_code[dc] << nb; nb += W.dist_len[dc];
    v |= (uint64_t)dv << nb; nb += de;
    return nb;
}

// One member: text[0 .. n) (1 <= n <= MAX_TEXT; any alignment, nothing outside it is read) -> slot[0 .. size rounded up to 16), a 16-byte
// aligned buffer of the member's own of (n + SLACK) rounded up to 16 bytes.  tok: n rounded up to TILE words of scratch.  Returns the
// member's size, bit 31 set when its block is a stored one (the same value in every lane).
template <int MODE = MODE_FAST, class X> DEF_HD uint32_t deflate_member(X &x, Work &W, const uint8_t *text, uint32_t n, uint32_t *tok, uint8_t *slot)
{
    const uint32_t lane = x.lane(), nl = x.lanes();
    inf::Tables &T = *reinterpret_cast<inf::Tables *>(W.img);
    static_assert(sizeof(inf::Tables) <= sizeof(W.img), "the CRC tables lie in the image until it is assembled");
    x.sync(); // (the workspace may still be read for the member in front)
    // ---- stage ---------------------------------------------------------------------------------------------------------------------
    // (word j of the text from the two ALIGNED words of memory it lies in, where both lie inside the text; bytes at the text's two ends)
    const uint32_t skew = (uint32_t)((uintptr_t)text & 3u);
    const uint8_t *aligned = text - skew;
    for (uint32_t j = lane; j < n / 4 + 2; j += nl) {
        uint32_t w = 0;
        if (4 * j >= skew && 4 * j + 8 - skew <= n) {
            uint32_t lo, hi = 0;
            memcpy(&lo, static_cast<const uint8_t *>(__builtin_assume_aligned(aligned + 4 * j, 4)), 4);
            if (skew) memcpy(&hi, static_cast<const uint8_t *>(__builtin_assume_aligned(aligned + 4 * j + 4, 4)), 4);
            w = (uint32_t)(((uint64_t)hi << 32 | lo) >> (8 * skew));
        } else {
            for (uint32_t k = 0; k < 4; ++k)
                if (4 * j + k < n) w |= (uint32_t)text[4 * j + k] << (8 * k);
        }
        W.text[j] = w;
    }
    for (uint32_t i = lane; i < 256; i += nl) W.byte_count[i] = 0;
    for (uint32_t i = lane; i < N_LIT; i += nl) W.lit_count[i] = 0;
    for (uint32_t i = lane; i < N_DIST; i += nl) W.dist_count[i] = 0;
    for (uint32_t i = lane; i < (1u << HASH_BITS); i += nl) W.u.head[i] = 0;
    if (lane == 0) { W.extra_bits = 0; W.entry = 0; W.crc = 0; }
    inf::crc_init(T, x); // (a barrier behind it)
    for (uint32_t l = lane; l < inf::CRC_LANES; l += nl) {
        const uint32_t c = inf::crc_slice(T, reinterpret_cast<const uint8_t *>(W.text), n, l);
        if (c) x.axor(&W.crc, c);
    }
    for (uint32_t i = lane; i < n; i += nl) x.aadd(&W.byte_count[load8(W.text, i)], 1u);
    x.sync();
    for (uint32_t i = lane; i < 256; i += nl) {
        const uint32_t f = W.byte_count[i];
        const uint32_t c = f ? log2_eighths(n) - log2_eighths(f) : 0u;
        W.lit_cost[i] = (uint16_t)(c < 8 ? 8 : c);
    }
    x.sync();
    // ---- the tiles -----------------------------------------------------------------------------------------------------------------
    const uint32_t n_tiles = (n + TILE - 1) / TILE;
    for (uint32_t t0 = 0; t0 < n_tiles * TILE; t0 += TILE) {
        const uint32_t entry = x.uni(W.entry);
        if constexpr (MODE == MODE_DENSE) {
        // find, sub-tile by sub-tile: four lanes per position, one candidate each (the fourth rests); then the position keeps the best of
        // the three and enters both tables, which therefore hold exactly the positions in front of the sub-tile that is looked up
        for (uint32_t s0 = 0; s0 < TILE; s0 += SUB) {
            for (uint32_t j = lane; j < 4 * SUB; j += nl) {
                const uint32_t i = j >> 2, c = j & 3u, p = t0 + s0 + i;
                if (c == 3) continue;
                uint32_t m = 0;
                if (p >= entry && p + MIN_MATCH <= n) {
                    uint32_t q = p; // the candidate's position + 1; (c) is p - 1
                    if (c == 0) q = W.u.head16[0][hash3(load32(W.text, p))];
                    else if (c == 1) q = p + 8 <= n ? W.u.head16[1][hash8(load32(W.text, p), load32(W.text, p + 4))] : 0u;
                    if (q && p - (q - 1) <= MAX_DIST) m = match_length(W.text, p, q - 1, umin(MAX_MATCH, n - p)) << 16 | (p - (q - 1));
                }
                W.t.p.cand[c][i] = m;
            }
            x.sync();
            for (uint32_t i = lane; i < SUB; i += nl) {
                const uint32_t p = t0 + s0 + i;
                uint32_t best = 0; // the longest, the nearest on a tie
                for (uint32_t c = 0; c < 3; ++c) {
                    const uint32_t m = W.t.p.cand[c][i];
                    if ((m >> 16) > (best >> 16) || ((m >> 16) == (best >> 16) && (m & 0xffffu) < (best & 0xffffu))) best = m;
                }
                const uint32_t len = best >> 16;
                if (len < MIN_MATCH || (len < SURE_LENGTH && !match_pays(W.text, W.lit_cost, p, len, best & 0xffffu))) best = 0;
                W.t.p.match[s0 + i] = best;
                if (p + MIN_MATCH <= n) x.amax16(W.u.head16[0], hash3(load32(W.text, p)), p + 1);
                if (p + 8 <= n) x.amax16(W.u.head16[1], hash8(load32(W.text, p), load32(W.text, p + 4)), p + 1);
            }
            x.sync();
        }
        // the lazy step, on the tile's lengths as the find left them: a match gives way to a longer one at the next position of the tile
        for (uint32_t i = lane; i < TILE; i += nl) {
            const uint32_t len = W.t.p.match[i] >> 16;
            W.t.p.reach[i] = (len && i + 1 < TILE && (W.t.p.match[i + 1] >> 16) > len) ? 1 : 0;
        }
        x.sync();
        } else {
        // find
        for (uint32_t i = lane; i < TILE; i += nl) {
            const uint32_t p = t0 + i;
            uint32_t len = 0, dist = 0;
            if (p >= entry && p + MIN_MATCH <= n) {
                const uint32_t most = umin(MAX_MATCH, n - p);
                const uint32_t c = W.u.head[hash3(load32(W.text, p))];
                if (c && p - (c - 1) <= MAX_DIST) {
                    len = match_length(W.text, p, c - 1, most);
                    dist = p - (c - 1);
                }
                if (p) {
                    const uint32_t l1 = match_length(W.text, p, p - 1, most);
                    if (l1 >= len) { len = l1; dist = 1; }
                }
                if (len >= MIN_MATCH && len < SURE_LENGTH && !match_pays(W.text, W.lit_cost, p, len, dist)) len = 0;
                if (len < MIN_MATCH) len = dist = 0;
            }
            W.t.p.match[i] = len << 16 | dist;
        }
        x.sync();
        } // (MODE_FAST)
        // the tile enters head[] (the dense mode's has, and its lazy step is applied instead); the parse's first step
        for (uint32_t i = lane; i < TILE; i += nl) {
            const uint32_t p = t0 + i;
            if constexpr (MODE == MODE_DENSE) { if (W.t.p.reach[i]) W.t.p.match[i] = 0; }
            else if (p + MIN_MATCH <= n) x.amax(&W.u.head[hash3(load32(W.text, p))], p + 1);
            const uint32_t len = W.t.p.match[i] >> 16;
            W.t.p.next[0][i] = (uint16_t)(p < n ? umin(i + (len ? len : 1u), TILE) : (uint32_t)TILE);
            W.t.p.reach[i] = (p == entry) ? 1 : 0;
        }
        if (lane == 0) { W.t.p.next[0][TILE] = W.t.p.next[1][TILE] = TILE; W.entry_next = entry; }
        x.sync();
        // parse: after round r every position within 2^(r + 1) - 1 tokens of the entry is marked
        for (uint32_t r = 0; r < 10; ++r) {
            const uint16_t *cur = W.t.p.next[r & 1u];
            uint16_t *nw = W.t.p.next[(r & 1u) ^ 1u];
            for (uint32_t i = lane; i < TILE; i += nl) {
                const uint32_t j = cur[i];
                if (W.t.p.reach[i] && j < TILE) W.t.p.reach[j] = 1;
                nw[i] = cur[j];
            }
            x.sync();
        }
        // tokens
        for (uint32_t i = lane; i < TILE; i += nl) {
            const uint32_t p = t0 + i;
            uint32_t token = NO_TOKEN;
            if (p < n && W.t.p.reach[i]) {
                const uint32_t m = W.t.p.match[i], len = m >> 16;
                if (len) {
                    uint32_t lc, le, lv, dc, de, dv;
                    length_symbol(len, lc, le, lv);
                    distance_symbol(m & 0xffffu, dc, de, dv);
                    x.aadd(&W.lit_count[257 + lc], 1u);
                    x.aadd(&W.dist_count[dc], 1u);
                    if (le + de) x.aadd(&W.extra_bits, le + de);
                    token = m;
                } else {
                    token = load8(W.text, p);
                    x.aadd(&W.lit_count[token], 1u);
                }
                if (i + (len ? len : 1u) >= TILE) W.entry_next = p + (len ? len : 1u); // (the tile's last token: one writer)
            }
            if (p < n) tok[p] = token;
        }
        x.sync();
        if (lane == 0) W.entry = W.entry_next;
        x.sync();
    }
    // ---- codes ---------------------------------------------------------------------------------------------------------------------
    if (lane == 0) W.lit_count[256] = 1;
    code_lengths(x, W, W.lit_count, 286, 15, W.lit_len, false);
    code_lengths(x, W, W.dist_count, 30, 15, W.dist_len, false);
    if (lane == 0) {
        uint32_t nlit = 286, ndist = 30;
        while (nlit > 257 && !W.lit_len[nlit - 1]) --nlit;
        while (ndist > 1 && !W.dist_len[ndist - 1]) --ndist;
        W.n_lit = nlit; W.n_dist = ndist;
        // the lengths of both sets as one sequence, run-length coded: 16 repeats the length in front 3 .. 6 times, 17 / 18 are 3 .. 10 /
        // 11 .. 138 zeros
        for (uint32_t s = 0; s <= N_CL; ++s) W.cl_count[s] = 0;
        const uint32_t total = nlit + ndist;
        uint32_t k = 0;
        auto at = [&](uint32_t i) -> uint32_t { return i < nlit ? W.lit_len[i] : W.dist_len[i - nlit]; };
        auto emit = [&](uint32_t sym, uint32_t value) { W.u.c.cl_token[k++] = (uint16_t)(sym | value << 8); ++W.cl_count[sym]; };
        for (uint32_t i = 0; i < total;) {
            const uint32_t v = at(i);
            uint32_t run = 1;
            while (i + run < total && at(i + run) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const uint32_t r = umin(run, 138); emit(18, r - 11); run -= r; }
                if (run >= 3) { emit(17, run - 3); run = 0; }
            } else {
                emit(v, 0); --run;
                while (run >= 3) { const uint32_t r = umin(run, 6); emit(16, r - 3); run -= r; }
            }
            while (run) { emit(v, 0); --run; }
        }
        W.n_cl_token = k;
    }
    code_lengths(x, W, W.cl_count, N_CL, 7, W.cl_len, true);
    // ---- choose --------------------------------------------------------------------------------------------------------------------
    if (lane == 0) {
        uint32_t ncl = N_CL;
        while (ncl > 4 && !W.cl_len[inf::cl_order(ncl - 1)]) --ncl;
        W.n_cl = ncl;
        uint32_t dyn = 3 + 5 + 5 + 4 + 3 * ncl, fix = 3;
        for (uint32_t s = 0; s < N_CL; ++s) dyn += W.cl_count[s] * (W.cl_len[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
        for (uint32_t s = 0; s < 286; ++s) { dyn += W.lit_count[s] * W.lit_len[s]; fix += W.lit_count[s] * fixed_lit_len(s); }
        for (uint32_t s = 0; s < 30; ++s) { dyn += W.dist_count[s] * W.dist_len[s]; fix += W.dist_count[s] * 5u; }
        dyn += W.extra_bits; fix += W.extra_bits;
        const uint32_t kind = fix <= dyn ? KIND_FIXED : KIND_DYNAMIC, bits = fix <= dyn ? fix : dyn;
        if ((bits + 7) / 8 >= n + 5) { W.kind = KIND_STORED; W.stream_bits = 8 * (n + 5); }
        else { W.kind = kind; W.stream_bits = bits; }
        W.size = HEADER + (W.stream_bits + 7) / 8 + TRAILER;
        if (W.kind == KIND_FIXED) {
            for (uint32_t s = 0; s < N_LIT; ++s) W.lit_len[s] = (uint8_t)fixed_lit_len(s);
            for (uint32_t s = 0; s < N_DIST; ++s) W.dist_len[s] = 5;
        }
        if (W.kind != KIND_STORED) {
            canonical_codes(W.lit_len, W.kind == KIND_FIXED ? (uint32_t)N_LIT : 286u, W.u.c.lit_code);
            canonical_codes(W.dist_len, W.kind == KIND_FIXED ? (uint32_t)N_DIST : 30u, W.u.c.dist_code);
            canonical_codes(W.cl_len, N_CL, W.u.c.cl_code);
        }
    }
    x.sync();
    const uint32_t kind = x.uni(W.kind), size = x.uni(W.size), crc = x.uni(W.crc);
    // ---- place ---------------------------------------------------------------------------------------------------------------------
    const uint32_t n16 = (size + 15) / 16;
    for (uint32_t j = lane; j < 4 * n16; j += nl) W.img[j] = 0;
    x.sync();
    uint32_t at = 8 * HEADER;
    if (lane == 0) {
        put_bits(x, W.img, 0, 0x04088b1fu, 32);   // ID1 ID2 CM FLG.FEXTRA; MTIME = 0
        put_bits(x, W.img, 64, 0x0006ff00u, 32);  // XFL = 0, OS = 255, XLEN = 6
        put_bits(x, W.img, 96, 0x00024342u, 32);  // 'B' 'C' 2 0
        put_bits(x, W.img, 128, size - 1, 16);    // BSIZE
        put_bits(x, W.img, 8 * (size - 8), crc, 32);
        put_bits(x, W.img, 8 * (size - 4), n, 32);
    }
    if (kind == KIND_STORED) {
        if (lane == 0) {
            put_bits(x, W.img, at, 1, 8);
            put_bits(x, W.img, at + 8, n, 16);
            put_bits(x, W.img, at + 24, n ^ 0xffffu, 16);
        }
        for (uint32_t i = lane; i < n; i += nl) put_bits(x, W.img, at + 40 + 8 * i, load8(W.text, i), 8);
    } else {
        if (lane == 0) {
            put_bits(x, W.img, at, 1u | (uint32_t)kind << 1, 3);
            at += 3;
            if (kind == KIND_DYNAMIC) {
                put_bits(x, W.img, at, W.n_lit - 257, 5);
                put_bits(x, W.img, at + 5, W.n_dist - 1, 5);
                put_bits(x, W.img, at + 10, W.n_cl - 4, 4);
                at += 14;
                for (uint32_t i = 0; i < W.n_cl; ++i, at += 3) put_bits(x, W.img, at, W.cl_len[inf::cl_order(i)], 3);
                for (uint32_t k = 0; k < W.n_cl_token; ++k) {
                    const uint32_t sym = W.u.c.cl_token[k] & 255u, value = W.u.c.cl_token[k] >> 8;
                    put_bits(x, W.img, at, W.u.c.cl_code[sym], W.cl_len[sym]);
                    at += W.cl_len[sym];
                    const uint32_t e = sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u;
                    put_bits(x, W.img, at, value, e);
                    at += e;
                }
            }
            W.entry = at; // (the tokens start here)
        }
        x.sync();
        at = x.uni(W.entry);
        for (uint32_t t0 = 0; t0 < n_tiles * TILE; t0 += TILE) {
            for (uint32_t i = lane; i < TILE; i += nl) {
                const uint32_t p = t0 + i, token = p < n ? tok[p] : NO_TOKEN;
                uint64_t v = 0;
                W.t.bits[i] = token == NO_TOKEN ? 0u : token_bits(W, token, v);
            }
            const uint32_t total = x.excl_scan(W.t.bits);
            for (uint32_t i = lane; i < TILE; i += nl) {
                const uint32_t p = t0 + i, token = p < n ? tok[p] : NO_TOKEN;
                if (token == NO_TOKEN) continue;
                uint64_t v = 0;
                const uint32_t nb = token_bits(W, token, v), o = at + W.t.bits[i];
                put_bits(x, W.img, o, (uint32_t)v, umin(nb, 32));
                if (nb > 32) put_bits(x, W.img, o + 32, (uint32_t)(v >> 32), nb - 32);
            }
            at += total;
            x.sync(); // (bits[] is rewritten)
        }
        if (lane == 0) put_bits(x, W.img, at, W.u.c.lit_code[256], W.lit_len[256]);
    }
    x.sync();
    for (uint32_t q = lane; q < n16; q += nl) x.store16(slot + 16 * q, &W.img[4 * q]);
    return size | (kind == KIND_STORED ? 0x80000000u : 0u);
}

// ---- the host as an executor ---------------------------------------------------------------------------------------------------------
struct HostExec {
    uint32_t lane() const { return 0; }
    uint32_t lanes() const { return 1; }
    void sync() {}
    uint32_t uni(uint32_t v) const { return v; }
    void amax(uint32_t *p, uint32_t v) { if (v > *p) *p = v; }
    void amax16(uint16_t *a, uint32_t i, uint32_t v) { if (v > a[i]) a[i] = (uint16_t)v; }
    void aadd(uint32_t *p, uint32_t v) { *p += v; }
    void aor(uint32_t *p, uint32_t v) { *p |= v; }
    void axor(uint32_t *p, uint32_t v) { *p ^= v; }
    uint32_t excl_scan(uint32_t *a)
    {
        uint32_t s = 0;
        for (uint32_t i = 0; i < TILE; ++i) { const uint32_t v = a[i]; a[i] = s; s += v; }
        return s;
    }
    void store16(uint8_t *dst, const uint32_t *src) { memcpy(dst, src, 16); }
};

DEF_HD uint32_t slot_bytes(uint32_t member_bytes) { return (member_bytes + SLACK + 15u) & ~15u; }

} // namespace faqcs_deflate
