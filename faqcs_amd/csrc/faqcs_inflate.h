// faqcs_inflate.h -- the decoder core of faqcs_inflate_device / faqcs_inflate_host and of the piece-wise gunzip (faqcs_gunzip.h): the gzip member
// header, canonical Huffman tables with zlib's acceptance rules, symbol decode, length / distance arithmetic, the block loop of a BGZF
// member (faqcs_gunzip.h's gz_run is the same loop with a piece's bounds and stops) and the CRC-32 arithmetic; at the end, the BSIZE walk of
// faqcs_bgzf_index_host and the per-position decision it shares with faqcs_bgzf_index_device's kernels.
// The SAME text compiles for the host (faqcs_host.cpp: faqcs_inflate_host; tools/inflate_host_fuzz.cpp under the sanitizers) and for
// gfx950 (faqcs_inflate_kernel.hip, faqcs_gunzip_kernel.hip), the way faqcs_skm.h does: every bound the decoder checks -- input that runs
// out, a distance in front of the member, output beyond its bound -- is checked HERE, before a Sink is asked to move a byte, so what the
// CPU tests and the sanitizers prove about the arithmetic holds for the device code.  No HIP call, no zlib.
//
// A Sink is who executes the decoder: one host thread (lanes() == 1: HostSink) or one wave (lanes() == 64, every lane runs the same
// control flow on the same values: WaveSink of faqcs_inflate_wave.h).  Its output is bytes (a BGZF member) or 16-bit symbols (a piece of
// an ordinary gzip member: a byte, or 0x8000 | k = byte k of the MAX_DIST in front of the piece, a marker).  It supplies
//     lane(), lanes()              who I am among the cooperating lanes
//     sync()                       writes of any lane to the Tables are visible to every lane behind it
//     uni(v)                       v, known to be the same in every lane (a scalar register on the device)
//     umin(v)                      the smallest v of the cooperating lanes
//     lit(o, byte)                 output o
//     match(o, len, dist)          outputs [o, o + len): output i = output o - dist + (i mod dist); bytes: dist <= o, checked here;
//                                  symbols: dist <= MAX_DIST, and a source in front of output 0 is a marker
//     stored(o, src, len)          outputs [o, o + len) = src[0 .. len)                                      (both ranges checked here)
//     flush()                      everything handed over so far is in memory
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define INF_HD __host__ __device__ __forceinline__
#else
#define INF_HD static inline
#endif

namespace faqcs_inflate {

enum { ST_OK = 0, ST_E_HEADER = 1, ST_E_LENGTH = 2, ST_E_DATA = 3, ST_E_CRC = 4, ST_E_TRUNCATED = 5 }; // == FAQCS_INFLATE_*
enum { MAX_ISIZE = 65536, MIN_MEMBER = 26, LIT_BITS = 10, DIST_BITS = 8, CL_BITS = 7, CRC_LANES = 64, MAX_DIST = 32768 };
enum { CRC_POLY = 0xedb88320u };

// What a block's decoder keeps: in LDS on the device (one per wave), on the stack on the host.  A primary table entry is
// symbol << 4 | code length, 0 = no code of at most `bits` bits ends here: longer codes (rare) and invalid ones take the canonical walk
// over cnt / sorted.
struct Tables {
    uint16_t lit[1 << LIT_BITS];
    uint16_t dist[1 << DIST_BITS];   // (first the code-length code of a dynamic block, then its distance code)
    uint16_t lit_sorted[288], dist_sorted[32];
    uint16_t lit_cnt[16], dist_cnt[16];
    uint16_t start[16], first[16], next[16], symidx[320];
    uint8_t lens[320];
    uint8_t cl[20];
    uint32_t ok;
    uint32_t crc[256];
    uint32_t x2n[20];                // x^(2^k) modulo the gzip polynomial, reflected
};

INF_HD uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
INF_HD uint32_t le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }

// BSIZE + 1 of the BGZF member whose header starts at p with `avail` bytes behind it; 0 = not a BGZF member header.  The acceptance rule
// of the command line's reader (faqcs_cli.cpp, BgzfReader::member_size), so that both accept the same headers.
INF_HD uint32_t bgzf_member_size(const uint8_t *p, uint64_t avail)
{
    if (avail < 18 || p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) return 0;
    const uint32_t xlen = le16(p + 10);
    if (avail < 12ull + xlen) return 0;
    for (uint32_t x = 0; x + 4 <= xlen;) {
        const uint8_t *f = p + 12 + x;
        const uint32_t slen = le16(f + 2);
        if (f[0] == 'B' && f[1] == 'C' && slen == 2 && x + 6 <= xlen) return le16(f + 4) + 1;
        x += 4 + slen;
    }
    return 0;
}

// ---- the member header (RFC 1952) -----------------------------------------------------------------------------------------------------
// What stands at w[0 .. have), the first bytes of a member; all: these are all the bytes there are.
//   H_OK        a header of hlen bytes, the deflate stream behind it          H_END      not gzip: the data ends here, without an error
//   H_HEADER    CM != 8 or a reserved FLG bit                                 H_PARTIAL  sound as far as it goes, and it ends early
//   H_MORE      (all = false) the header is longer than the window
enum { H_OK = 0, H_END, H_HEADER, H_PARTIAL, H_MORE };
INF_HD int gz_header(const uint8_t *w, uint64_t have, bool all, uint32_t &hlen)
{
    hlen = 0;
    const int shrt = all ? H_PARTIAL : H_MORE;
    if (!have) return shrt;
    if (w[0] != 31 || (have >= 2 && w[1] != 139)) return H_END;
    if (have >= 3 && w[2] != 8) return H_HEADER;
    if (have >= 4 && (w[3] & 0xe0u)) return H_HEADER;
    if (have < 10) return shrt;
    const uint32_t flg = w[3];
    uint64_t q = 10;
    if (flg & 4u) { // FEXTRA
        if (have < 12) return shrt;
        q = 12 + (uint64_t)le16(w + 10);
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) // FNAME, FCOMMENT: zero-terminated
        if (flg & bit) {
            while (q < have && w[q]) ++q;
            if (q >= have) return shrt;
            ++q;
        }
    if (flg & 2u) q += 2; // FHCRC: skipped, not verified
    if (q > have) return shrt;
    hlen = (uint32_t)q;
    return H_OK;
}

struct Member { uint32_t data_begin, data_end, crc, isize; }; // the deflate stream is p[data_begin .. data_end), the trailer behind it

// The BGZF member that fills p[0 .. size) exactly: the header in front of the trailer's eight bytes is all the header there is.
INF_HD int parse_member(const uint8_t *p, uint64_t size, Member &m)
{
    m.data_begin = m.data_end = m.crc = m.isize = 0;
    if (size < MIN_MEMBER || size > 65536 || bgzf_member_size(p, size) != size) return ST_E_HEADER;
    const uint32_t limit = (uint32_t)size - 8;
    if (gz_header(p, limit, true, m.data_begin) != H_OK) return ST_E_HEADER; // (FNAME, FCOMMENT, FHCRC, the reserved bits)
    m.data_end = limit;
    m.crc = le32(p + limit); m.isize = le32(p + limit + 4);
    return m.isize > MAX_ISIZE ? ST_E_LENGTH : ST_OK;
}

// ---- bits --------------------------------------------------------------------------------------------------------------------------
// in[pos ..) is loaded a dword ahead of its use (`next`), so that the load's latency lies beside the symbols in front of it; cnt counts
// real bits only: a field that needs more than there are is the input running out.
struct BitReader {
    const uint8_t *in;
    uint32_t pos, end; // pos: the byte `next` was loaded from
    uint64_t buf;
    uint32_t cnt, next, next_n;
    bool bad;
};
template <class Sink> INF_HD void br_load(BitReader &b, Sink &S)
{
    const uint32_t n = b.end - b.pos;
    uint32_t v = 0;
    if (n >= 4) { memcpy(&v, b.in + b.pos, 4); b.next_n = 4; }
    else { for (uint32_t i = 0; i < n; ++i) v |= (uint32_t)b.in[b.pos + i] << (8 * i); b.next_n = n; }
    b.next = S.uni(v);
}
template <class Sink> INF_HD void br_seek(BitReader &b, uint32_t pos, Sink &S) { b.pos = pos; b.buf = 0; b.cnt = 0; br_load(b, S); }
// at least 32 bits behind it, unless the input ends
template <class Sink> INF_HD void br_refill(BitReader &b, Sink &S)
{
    if (b.cnt < 32 && b.next_n) {
        b.buf |= (uint64_t)b.next << b.cnt;
        b.cnt += 8 * b.next_n;
        b.pos += b.next_n;
        br_load(b, S);
    }
}
INF_HD void br_drop(BitReader &b, uint32_t n) { b.buf >>= n; b.cnt -= n; }
INF_HD uint32_t br_take(BitReader &b, uint32_t n) // n <= 16
{
    if (n > b.cnt) { b.bad = true; return 0; }
    const uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
    br_drop(b, n);
    return v;
}
INF_HD uint32_t br_byte_pos(const BitReader &b) { return b.pos - (b.cnt >> 3); } // of the first byte no bit was taken from

// ---- tables ------------------------------------------------------------------------------------------------------------------------
INF_HD uint32_t bit_reverse(uint32_t v, uint32_t n) // the low n bits of v, reversed (1 <= n <= 15)
{
    v = ((v >> 1) & 0x5555u) | ((v & 0x5555u) << 1);
    v = ((v >> 2) & 0x3333u) | ((v & 0x3333u) << 2);
    v = ((v >> 4) & 0x0f0fu) | ((v & 0x0f0fu) << 4);
    v = ((v >> 8) & 0x00ffu) | ((v & 0x00ffu) << 8);
    return v >> (16 - n);
}

// The canonical code of lens[0 .. n) (0 = symbol unused).  zlib's inflate_table rules: an over-subscribed set is invalid; an incomplete
// one too, except no code at all, and -- not for the code-length code -- a single code of one bit.  Lane 0 counts and ranks (two passes
// over at most 320 symbols), the lanes fill the primary table, one symbol each.
template <class Sink>
INF_HD bool build_table(const uint8_t *lens, uint32_t n, uint16_t *tab, uint32_t bits, uint16_t *cnt, uint16_t *sorted, bool code_lengths, Tables &T, Sink &S)
{
    const uint32_t lane = S.lane(), nl = S.lanes();
    S.sync(); // (the tables may still be read)
    for (uint32_t i = lane; i < (1u << bits); i += nl) tab[i] = 0;
    if (lane == 0) {
        for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
        for (uint32_t s = 0; s < n; ++s) ++cnt[lens[s] & 15u];
        int left = 1;
        uint32_t max = 0;
        bool ok = true;
        for (uint32_t l = 1; l < 16; ++l) {
            left = 2 * left - (int)cnt[l];
            if (left < 0) { ok = false; break; }
            if (cnt[l]) max = l;
        }
        if (ok && left > 0 && !(max == 0 || (max == 1 && !code_lengths))) ok = false;
        uint32_t at = 0, code = 0;
        for (uint32_t l = 1; l < 16; ++l) {
            T.start[l] = T.next[l] = (uint16_t)at;
            T.first[l] = (uint16_t)code;
            at += cnt[l];
            code = (code + cnt[l]) << 1;
        }
        if (ok)
            for (uint32_t s = 0; s < n; ++s) {
                const uint32_t l = lens[s] & 15u;
                if (l) { const uint32_t k = T.next[l]++; sorted[k] = (uint16_t)s; T.symidx[s] = (uint16_t)k; }
            }
        T.ok = ok ? 1u : 0u;
    }
    S.sync();
    if (!S.uni(T.ok)) return false;
    for (uint32_t s = lane; s < n; s += nl) {
        const uint32_t l = lens[s] & 15u;
        if (l && l <= bits) {
            const uint32_t code = (uint32_t)T.first[l] + ((uint32_t)T.symidx[s] - (uint32_t)T.start[l]);
            for (uint32_t k = bit_reverse(code, l); k < (1u << bits); k += 1u << l) tab[k] = (uint16_t)(s << 4 | l);
        }
    }
    S.sync();
    return true;
}

// the next symbol, or -1: no code of this set starts the bits, or the input ran out
template <class Sink>
INF_HD int decode_symbol(const uint16_t *tab, uint32_t bits, const uint16_t *cnt, const uint16_t *sorted, BitReader &b, Sink &S)
{
    const uint32_t e = S.uni((uint32_t)tab[(uint32_t)b.buf & ((1u << bits) - 1u)]);
    const uint32_t l = e & 15u;
    if (l) {
        if (l > b.cnt) return -1;
        br_drop(b, l);
        return (int)(e >> 4);
    }
    uint64_t v = b.buf;
    int code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len < 16; ++len) {
        if (len > b.cnt) return -1;
        code |= (int)(v & 1u);
        v >>= 1;
        const int count = (int)S.uni((uint32_t)cnt[len]);
        if (code - count < first) {
            br_drop(b, len);
            return (int)S.uni((uint32_t)sorted[index + (code - first)]);
        }
        index += count; first += count;
        first <<= 1; code <<= 1;
    }
    return -1;
}

// length symbol c = sym - 257 (0 .. 28) and distance symbol d (0 .. 29): base value and extra bits, RFC 1951 section 3.2.5 as arithmetic
INF_HD void length_code(uint32_t c, uint32_t &base, uint32_t &extra)
{
    if (c < 8) { base = 3 + c; extra = 0; }
    else if (c == 28) { base = 258; extra = 0; }
    else { extra = (c >> 2) - 1; base = 3 + ((4 + (c & 3u)) << extra); }
}
INF_HD void distance_code(uint32_t d, uint32_t &base, uint32_t &extra)
{
    if (d < 4) { base = 1 + d; extra = 0; }
    else { extra = (d >> 1) - 1; base = 1 + ((2 + (d & 1u)) << extra); }
}
// the order the code-length code's lengths are sent in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
INF_HD uint32_t cl_order(uint32_t i)
{
    const uint64_t a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t c = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? a >> (5 * i) : c >> (5 * (i - 12))) & 31u);
}

// ---- CRC-32 ------------------------------------------------------------------------------------------------------------------------
INF_HD uint32_t multmodp(uint32_t a, uint32_t b) // a(x) b(x) modulo the gzip polynomial, reflected (bit 31 = x^0)
{
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? (uint32_t)CRC_POLY : 0u);
    }
    return p;
}
// x^(2^k) modulo the gzip polynomial, reflected, for k < n: the squaring chain
INF_HD void x2n_fill(uint32_t *x2n, uint32_t n)
{
    uint32_t p = 0x40000000u; // x^1
    for (uint32_t k = 0; k < n; ++k) { x2n[k] = p; p = multmodp(p, p); }
}
INF_HD uint32_t x8n_modp(const uint32_t *x2n, uint64_t n) // x^(8 n); x2n holds three entries more than n has bits
{
    uint32_t p = 0x80000000u;
    for (uint32_t k = 3; n; n >>= 1, ++k)
        if (n & 1u) p = multmodp(x2n[k], p);
    return p;
}
// the byte table and the powers (n <= 65 536: 20 of them): once per Tables
template <class Sink> INF_HD void crc_init(Tables &T, Sink &S)
{
    for (uint32_t i = S.lane(); i < 256; i += S.lanes()) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (uint32_t)CRC_POLY ^ (c >> 1) : c >> 1;
        T.crc[i] = c;
    }
    if (S.lane() == 0) x2n_fill(T.x2n, 20);
    S.sync();
}
// What slice `l` of CRC_LANES contiguous slices of text[0 .. n) adds to the CRC-32 of the whole: its own CRC multiplied by x^(8 x the bytes
// behind it).  The CRC of the text is the XOR over the slices.
INF_HD uint32_t crc_slice(const Tables &T, const uint8_t *text, uint32_t n, uint32_t l)
{
    const uint32_t per = (n + CRC_LANES - 1) / CRC_LANES;
    const uint32_t a = l * per < n ? l * per : n, e = a + per < n ? a + per : n;
    if (e == a) return 0;
    uint32_t c = 0xffffffffu, i = a;
    for (; i + 4 <= e; i += 4) {
        uint32_t w;
        memcpy(&w, text + i, 4);
        c ^= w;
        for (int k = 0; k < 4; ++k) c = T.crc[c & 255u] ^ (c >> 8);
    }
    for (; i < e; ++i) c = T.crc[(c ^ text[i]) & 255u] ^ (c >> 8);
    return multmodp(x8n_modp(T.x2n, n - e), ~c);
}

// ---- a member ----------------------------------------------------------------------------------------------------------------------
// The deflate stream in[begin .. end) must decode to exactly isize bytes and end in the byte in front of `end`.  ST_OK, ST_E_DATA or
// ST_E_LENGTH; output offsets handed to the Sink are always inside [0, isize).
template <class Sink>
INF_HD int inflate_member(const uint8_t *in, uint32_t begin, uint32_t end, uint32_t isize, Tables &T, Sink &S)
{
    BitReader b;
    b.in = in; b.end = end; b.bad = false;
    br_seek(b, begin, S);
    uint32_t o = 0, last;
    do {
        br_refill(b, S);
        last = br_take(b, 1);
        const uint32_t type = br_take(b, 2);
        if (b.bad || type == 3) return ST_E_DATA;
        if (type == 0) {
            br_drop(b, b.cnt & 7u);
            br_refill(b, S);
            const uint32_t len = br_take(b, 16), nlen = br_take(b, 16);
            if (b.bad || (len ^ 0xffffu) != nlen) return ST_E_DATA;
            const uint32_t sp = br_byte_pos(b);
            if (len > end - sp) return ST_E_DATA;
            if (len > isize - o) return ST_E_LENGTH;
            S.stored(o, in + sp, len);
            o += len;
            br_seek(b, sp + len, S);
            continue;
        }
        uint32_t nlit = 288, ndist = 32; // (fixed: 286, 287 and 30, 31 take part in the code and are refused when they come up)
        S.sync();
        if (type == 1) {
            for (uint32_t s = S.lane(); s < 320; s += S.lanes()) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
        } else {
            br_refill(b, S);
            nlit = br_take(b, 5) + 257; ndist = br_take(b, 5) + 1;
            const uint32_t ncl = br_take(b, 4) + 4;
            if (b.bad || nlit > 286 || ndist > 30) return ST_E_DATA;
            for (uint32_t i = S.lane(); i < 20; i += S.lanes()) T.cl[i] = 0;
            S.sync();
            for (uint32_t i = 0; i < ncl; ++i) {
                br_refill(b, S);
                const uint32_t v = br_take(b, 3);
                if (S.lane() == 0) T.cl[cl_order(i)] = (uint8_t)v;
            }
            if (b.bad) return ST_E_DATA;
            if (!build_table(T.cl, 19, T.dist, CL_BITS, T.dist_cnt, T.dist_sorted, true, T, S)) return ST_E_DATA;
            const uint32_t total = nlit + ndist;
            uint32_t i = 0, prev = 0, eob = 0;
            while (i < total) {
                br_refill(b, S);
                const int sym = decode_symbol(T.dist, CL_BITS, T.dist_cnt, T.dist_sorted, b, S);
                if (sym < 0) return ST_E_DATA;
                uint32_t rep = 1, val = (uint32_t)sym;
                if (sym == 16) { if (i == 0) return ST_E_DATA; rep = 3 + br_take(b, 2); val = prev; }
                else if (sym == 17) { rep = 3 + br_take(b, 3); val = 0; }
                else if (sym == 18) { rep = 11 + br_take(b, 7); val = 0; }
                if (b.bad || rep > total - i) return ST_E_DATA;
                if (i <= 256 && 256 < i + rep) eob = val;
                for (uint32_t k = S.lane(); k < rep; k += S.lanes()) T.lens[i + k] = (uint8_t)val;
                i += rep; prev = val;
            }
            if (!eob) return ST_E_DATA; // no end-of-block code
        }
        if (!build_table(T.lens, nlit, T.lit, LIT_BITS, T.lit_cnt, T.lit_sorted, false, T, S)) return ST_E_DATA;
        if (!build_table(T.lens + nlit, ndist, T.dist, DIST_BITS, T.dist_cnt, T.dist_sorted, false, T, S)) return ST_E_DATA;
        for (;;) {
            br_refill(b, S);
            const int sym = decode_symbol(T.lit, LIT_BITS, T.lit_cnt, T.lit_sorted, b, S);
            if (sym < 0) return ST_E_DATA;
            if (sym < 256) {
                if (o >= isize) return ST_E_LENGTH;
                S.lit(o, (uint32_t)sym);
                ++o;
                continue;
            }
            if (sym == 256) break;
            if (sym >= 286) return ST_E_DATA;
            uint32_t base, extra;
            length_code((uint32_t)sym - 257u, base, extra);
            const uint32_t len = base + br_take(b, extra);
            br_refill(b, S);
            const int ds = decode_symbol(T.dist, DIST_BITS, T.dist_cnt, T.dist_sorted, b, S);
            if (ds < 0 || ds >= 30) return ST_E_DATA;
            distance_code((uint32_t)ds, base, extra);
            const uint32_t dist = base + br_take(b, extra);
            if (b.bad || dist > o) return ST_E_DATA; // (a distance in front of the member: there is no dictionary)
            if (len > isize - o) return ST_E_LENGTH;
            S.match(o, len, dist);
            o += len;
        }
    } while (!last);
    S.flush();
    if (br_byte_pos(b) != end) return ST_E_DATA; // the stream ends where the trailer starts
    return o == isize ? ST_OK : ST_E_LENGTH;
}

// ---- the host as a Sink ------------------------------------------------------------------------------------------------------------
template <class Sym> struct HostSink { // Sym: uint8_t, or uint16_t with markers
    Sym *out;
    uint32_t lane() const { return 0; }
    uint32_t lanes() const { return 1; }
    void sync() {}
    uint32_t uni(uint32_t v) const { return v; }
    uint32_t umin(uint32_t v) const { return v; }
    void lit(uint32_t o, uint32_t v) { out[o] = (Sym)v; }
    void match(uint32_t o, uint32_t len, uint32_t dist)
    {
        for (uint32_t i = 0; i < len; ++i) {
            const uint32_t x = dist >= len ? i : i % dist; // the source is output o - dist + x
            if constexpr (sizeof(Sym) == 2) {
                const int64_t s = (int64_t)o - dist + x;
                out[o + i] = s < 0 ? (Sym)(0x8000u | (uint32_t)(MAX_DIST + s)) : out[s];
            } else out[o + i] = out[o - dist + x]; // (dist <= o)
        }
    }
    void stored(uint32_t o, const uint8_t *src, uint32_t len)
    {
        if constexpr (sizeof(Sym) == 1) { if (len) memcpy(out + o, src, len); }
        else for (uint32_t i = 0; i < len; ++i) out[o + i] = src[i];
    }
    void flush() {}
};

// One member on the host, into out[0 .. isize) (a buffer of the caller's: a bad member leaves it in an unspecified state): the scan's
// status when it is not ST_OK, else the decoder's, else the CRC's -- the CRC by the slices the device uses.
inline int inflate_member_host(const uint8_t *p, uint64_t size, Tables &T, uint8_t *out, Member &m)
{
    int st = parse_member(p, size, m);
    if (st) return st;
    HostSink<uint8_t> S{out};
    st = inflate_member(p, m.data_begin, m.data_end, m.isize, T, S);
    if (st) return st;
    uint32_t crc = 0;
    for (uint32_t l = 0; l < CRC_LANES; ++l) crc ^= crc_slice(T, out, m.isize, l);
    return crc == m.crc ? ST_OK : ST_E_CRC;
}

struct IndexInfo { uint64_t consumed; uint32_t n_members, overflow; int32_t error; };

// What the walk of the BSIZE chain decides at position p of comp[0 .. n) (p <= n), from the bytes comp[p .. n) alone.  The host walk
// (bgzf_index) and the kernels of faqcs_bgzf_index_device (faqcs_bgzf_index_kernel.hip) compile this text: a position is a member's for
// both or for neither.
//   AT_MEMBER    a whole member of ms bytes (MIN_MEMBER <= ms <= n - p): the walk goes on at p + ms
//   AT_STOP      p == n: the data ends behind a member, consumed = p
//   AT_END       not gzip: the data ends here, consumed = n
//   AT_HEADER    a gzip member that is not BGZF, no BC subfield, or a stated size below MIN_MEMBER: E_HEADER, consumed = p
//   AT_PARTIAL   what is there of a header or a member is sound, but not all of it is there: E_TRUNCATED when final, consumed = p
enum { AT_MEMBER = 0, AT_STOP, AT_END, AT_HEADER, AT_PARTIAL };
INF_HD int bgzf_index_at(const uint8_t *comp, uint64_t n, uint64_t p, uint32_t &ms)
{
    ms = 0;
    const uint64_t avail = n - p;
    if (!avail) return AT_STOP;
    if (comp[p] != 31 || (avail >= 2 && comp[p + 1] != 139)) return AT_END;
    if (avail >= 4 && (comp[p + 2] != 8 || !(comp[p + 3] & 4))) return AT_HEADER;
    bool whole = avail >= 18 && avail >= 12ull + le16(comp + p + 10);
    if (whole) {
        ms = bgzf_member_size(comp + p, avail);
        if (ms < MIN_MEMBER) return AT_HEADER; // no BC subfield
        whole = ms <= avail;
    }
    return whole ? AT_MEMBER : AT_PARTIAL;
}
// consumed and error of a walk that stops at position p with the decision `at` (not AT_MEMBER)
INF_HD void bgzf_index_stop(int at, uint64_t n, uint64_t p, int final, uint64_t &consumed, int32_t &error)
{
    consumed = at == AT_END ? n : p;
    error = at == AT_HEADER ? ST_E_HEADER : (at == AT_PARTIAL && final) ? ST_E_TRUNCATED : ST_OK;
}

// The BSIZE chain of comp[0 .. n) from byte 0: member k is comp[member_offset[k] .. member_offset[k + 1]).  See faqcs_bgzf_index_host.
inline void bgzf_index(const uint8_t *comp, uint64_t n, int final, uint32_t *member_offset, uint32_t capacity, IndexInfo &info)
{
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t p = 0;
        uint32_t k = 0, ms;
        int at;
        if (pass) member_offset[0] = 0;
        while ((at = bgzf_index_at(comp, n, p, ms)) == AT_MEMBER) {
            if (pass) member_offset[k + 1] = (uint32_t)(p + ms);
            p += ms; ++k;
        }
        if (pass) break;
        bgzf_index_stop(at, n, p, final, info.consumed, info.error);
        info.n_members = k;
        info.overflow = k > capacity ? 1u : 0u;
        if (info.overflow) break;
    }
}

} // namespace faqcs_inflate
