// faqcs_gunzip.h -- faqcs_gunzip_device / faqcs_gunzip_host (include/faqcs_mi.h): ordinary gzip -- members of any
// size, no index -- inflated by pieces.  The SAME text compiles for the host statement (faqcs_host.cpp), the sanitizer tool
// (tools/gunzip_host_fuzz.cpp) and gfx950 (faqcs_gunzip_kernel.hip), as faqcs_inflate.h does, and it builds on that file: the member header,
// BitReader, build_table, decode_symbol, the length / distance arithmetic, the CRC arithmetic and the host's Sink are that file's.  gz_run
// is inflate_member's block decoder once more, with its own bounds, statuses and stops: a rule changed in one is to be changed in the other.
//
//   pieces    the compressed bytes are cut every piece_bytes bytes (a grid over the whole input).  The wave of a grid piece PROBES its range for
//             the first bit position that can begin a non-final dynamic-Huffman block (plausible_block: the rules of faqcs_pargz.h) and whose
//             run (below) ends without an error; up to PROBE_TRIES candidates are tried, a piece may find none.
//   run       gz_run decodes block by block from a start and stops at the end of the first block that ends at or behind the piece's range
//             end, or at a final block.  The count pass (WRITE = false) produces no output -- symbol decoding needs no window -- and records
//             {start_bit, end_bit, n_out, final, status}; every loop is bounded by the input's bits, and a run from a probed start also
//             gives up SPEC_RUN bytes behind its range end.
//   chain     gunzip_run (host code, both forms) parses the member headers and walks the records from each member's first block: the piece
//             that contains end_bit(cur) must start there; if it does not, a piece WITH that start is counted in a round of its own.  The
//             first block of every member is such a forced start too.  More than max_rounds rounds inside one member: E_SERIAL.
//   sizes     the sum of n_out over the chain gives every piece its position and the overflow decision before anything is written.
//   decode    gz_run again (WRITE = true) per chain piece, into 16-bit symbols at the piece's position: a byte, or 0x8000 | k = byte k of the
//             32 768 in front of this piece.  resolve_piece, over the chain in order, turns the markers of each piece's last 32 768 symbols
//             into bytes (so the window of the next piece is bytes); narrow_slice makes text of everything and a CRC per slice.
//   chunks    faqcs_gunzip_stream_*: gunzip_run with a carried State.  The walk begins where the state says (in mid-stream: a forced start), the
//             symbols get a front of 32 768 that holds the carried window as bytes, so the first piece's markers resolve like any other's, and
//             with final = 0 the walk stops at the last block boundary that is resident; the CRC so far and this call's share are folded as
//             zlib's crc32_combine folds them.
// A Sink here is faqcs_inflate.h's with 16-bit output.
#pragma once
#include "faqcs_inflate.h"

#include <vector>

namespace faqcs_gunzip {

namespace inf = faqcs_inflate;

enum { ST_E_SERIAL = 16 };                  // == FAQCS_INFLATE_E_SERIAL
enum { P_NO_START = 100, P_GAVE_UP = 101 }; // a piece that is not a chain's: no start in its range | its run left SPEC_RUN behind
constexpr uint32_t MIN_PIECE = 1024, DEFAULT_PIECE = 64u << 10, DEFAULT_ROUNDS = 32, WIN = 32768, PROBE_TRIES = 8, SLICE = 16384;
constexpr uint64_t SPEC_RUN_BITS = 8ull << 20; // 1 MiB behind the range end: no block of zlib's is that long (its symbol buffer holds 16 384)
constexpr uint64_t NO_BIT = ~0ull;

// what the count pass records of a piece; state = status | final << 8
struct Piece { uint64_t start_bit, end_bit, n_out; uint32_t grid, state; };
// a piece of the chain for the passes that write: where its bits are, where its text is, and its member's text
struct ChainPiece { uint64_t start_bit, end_bit; uint32_t pos, n_out, member_pos, member_end; };
// at most SLICE bytes of a chain piece's text for narrow_slice
struct Slice { uint32_t begin, n, piece, pad; };
struct SliceResult { uint32_t crc, bad; }; // the slice's share of its member's CRC-32 | a marker in front of the member
struct Pow { uint32_t x2n[36]; };          // x^(2^k) modulo the gzip polynomial, reflected: 8 x 2^32 bits

static_assert(WIN == inf::MAX_DIST, "a marker's k counts from the window's first byte");
static_assert(sizeof(Piece) == 32 && sizeof(ChainPiece) == 32 && sizeof(Slice) == 16, "the records the host and the device exchange");

// ---- the probe --------------------------------------------------------------------------------------------------------------------------
INF_HD uint64_t peek(const uint8_t *in, uint64_t n, uint64_t bit) // 57 bits at `bit`; zeros behind the input
{
    const uint64_t by = bit >> 3;
    uint64_t v = 0;
    if (by + 8 <= n) memcpy(&v, in + by, 8);
    else for (uint32_t i = 0; by + i < n && i < 8; ++i) v |= (uint64_t)in[by + i] << (8 * i);
    return v >> (bit & 7u);
}

// Can a non-final dynamic-Huffman block start at `bit` of in[0 .. n)?  The rules of faqcs_pargz.h's plausible_block, which are
// build_table's: BFINAL = 0, BTYPE = 2, HLIT <= 286, HDIST <= 30, a complete code-length code, no repeat without a length in front or
// beyond the lengths, an end-of-block code, literal and distance sets that are complete, or one code of one bit, or (distances) no code.
// Straight-line and without tables: only about one position in a thousand comes past the code-length code.
INF_HD bool plausible_block(const uint8_t *in, uint64_t n, uint64_t bit)
{
    const uint64_t v = peek(in, n, bit);
    if ((v & 7u) != 4u) return false;
    const uint32_t hlit = (uint32_t)((v >> 3) & 31u) + 257, hdist = (uint32_t)((v >> 8) & 31u) + 1, hclen = (uint32_t)((v >> 13) & 15u) + 4;
    if (hlit > 286 || hdist > 30) return false;
    uint64_t at = bit + 17;
    uint64_t pv = peek(in, n, at) & ((1ull << (3 * hclen)) - 1u);
    at += 3 * hclen;
    uint64_t pl = 0; // the 19 lengths of the code-length code, three bits each
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < hclen; ++i, pv >>= 3) {
        const uint32_t l = (uint32_t)pv & 7u;
        pl |= (uint64_t)l << (3 * inf::cl_order(i));
        if (l) kraft += 128u >> l;
    }
    if (kraft != 128) return false;
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t s = 0; s < 19; ++s) ++cnt[(pl >> (3 * s)) & 7u];
    const uint32_t total = hlit + hdist;
    uint32_t i = 0, prev = 0, eob = 0;
    uint32_t sum[2] = {0, 0}, mx[2] = {0, 0}; // the code space taken in units of 2^-15 and the longest code, literals | distances
    while (i < total) {
        uint64_t w = peek(in, n, at);
        uint32_t code = 0, first = 0, len = 1, rank = 0;
        for (; len <= 7; ++len) { // the canonical walk of decode_symbol
            code |= (uint32_t)w & 1u;
            w >>= 1;
            const uint32_t c = cnt[len];
            if (code < first + c) { rank = code - first; break; }
            first = (first + c) << 1; code <<= 1;
        }
        if (len > 7) return false;
        at += len;
        uint32_t sym = 0;
        for (uint32_t r = rank; sym < 19; ++sym)
            if (((pl >> (3 * sym)) & 7u) == len) { if (!r) break; --r; }
        uint32_t rep = 1, val = sym;
        if (sym == 16) { if (!i) return false; rep = 3 + ((uint32_t)w & 3u); at += 2; val = prev; }
        else if (sym == 17) { rep = 3 + ((uint32_t)w & 7u); at += 3; val = 0; }
        else if (sym == 18) { rep = 11 + ((uint32_t)w & 127u); at += 7; val = 0; }
        if (rep > total - i) return false;
        if (val) {
            const uint32_t a = i >= hlit ? 0u : (i + rep <= hlit ? rep : hlit - i); // how many of them are literal / length codes
            if (a) { sum[0] += a * (32768u >> val); if (val > mx[0]) mx[0] = val; }
            if (rep > a) { sum[1] += (rep - a) * (32768u >> val); if (val > mx[1]) mx[1] = val; }
            if (i <= 256 && 256 < i + rep) eob = 1;
        }
        i += rep; prev = val;
    }
    if ((at >> 3) >= n || !eob) return false;
    for (uint32_t k = 0; k < 2; ++k)
        if (sum[k] > 32768u || (sum[k] < 32768u && mx[k] > 1)) return false;
    return true;
}

// the lowest position in [lo, hi) that passes, NO_BIT: none.  The lanes test neighbouring positions; the smallest of a step decides.
template <class Sink> INF_HD uint64_t probe(const uint8_t *in, uint64_t n, uint64_t lo, uint64_t hi, Sink &S)
{
    for (uint64_t base = lo; base < hi; base += S.lanes()) {
        const uint64_t c = base + S.lane();
        const uint32_t hit = S.umin(c < hi && plausible_block(in, n, c) ? S.lane() : 0xffffffffu);
        if (hit != 0xffffffffu) return base + hit;
    }
    return NO_BIT;
}

// ---- a run of blocks --------------------------------------------------------------------------------------------------------------------
struct Run { uint64_t end_bit, n_out; uint32_t final, status; };

INF_HD uint64_t br_bit_pos(const inf::BitReader &b) { return 8ull * b.pos - b.cnt; }
// why a field or a code could not be read: the input ran out (what is left of it is shorter than any code can be told by), or it is invalid
INF_HD uint32_t why(const inf::BitReader &b) { return (b.bad || (!b.next_n && b.cnt < 15)) ? (uint32_t)inf::ST_E_TRUNCATED : (uint32_t)inf::ST_E_DATA; }

// The blocks of in[0 .. n_in) from start_bit up to the end of the first block that ends at or behind limit_bit, or a final block.
// WRITE: the Sink receives output offsets relative to the run's start, all below max_out (else ST_E_DATA: a run that is repeated cannot
// differ, but no offset is handed over unchecked).  give_up_byte: a run that reads beyond it ends with P_GAVE_UP.
// r.n_out and r.end_bit are those of the last whole block; status: ST_OK, ST_E_DATA, ST_E_TRUNCATED (the input ran out), P_GAVE_UP.
template <bool WRITE, class Sink>
INF_HD void gz_run(const uint8_t *in, uint32_t n_in, uint64_t start_bit, uint64_t limit_bit, uint64_t give_up_byte, uint64_t max_out, inf::Tables &T, Sink &S, Run &r)
{
    inf::BitReader b;
    b.in = in; b.end = n_in; b.bad = false;
    r.end_bit = start_bit; r.n_out = 0; r.final = 0; r.status = inf::ST_OK;
    inf::br_seek(b, (uint32_t)(start_bit >> 3), S);
    inf::br_refill(b, S);
    if ((uint32_t)(start_bit & 7u) > b.cnt) { r.status = inf::ST_E_TRUNCATED; return; }
    inf::br_drop(b, (uint32_t)(start_bit & 7u));
    uint64_t o = 0;
    for (;;) {
        inf::br_refill(b, S);
        const uint32_t last = inf::br_take(b, 1), type = inf::br_take(b, 2);
        if (b.bad) { r.status = inf::ST_E_TRUNCATED; break; }
        if (type == 3) { r.status = inf::ST_E_DATA; break; }
        if (type == 0) {
            inf::br_drop(b, b.cnt & 7u);
            inf::br_refill(b, S);
            const uint32_t len = inf::br_take(b, 16), nlen = inf::br_take(b, 16);
            if (b.bad) { r.status = inf::ST_E_TRUNCATED; break; }
            if ((len ^ 0xffffu) != nlen) { r.status = inf::ST_E_DATA; break; }
            const uint32_t sp = inf::br_byte_pos(b);
            if (len > n_in - sp) { r.status = inf::ST_E_TRUNCATED; break; }
            if (len > max_out - o) { r.status = inf::ST_E_DATA; break; }
            if (WRITE) S.stored((uint32_t)o, in + sp, len);
            o += len;
            inf::br_seek(b, sp + len, S);
        } else {
            uint32_t nlit = 288, ndist = 32, st = inf::ST_OK;
            S.sync();
            if (type == 1) {
                for (uint32_t s = S.lane(); s < 320; s += S.lanes()) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
            } else {
                inf::br_refill(b, S);
                nlit = inf::br_take(b, 5) + 257; ndist = inf::br_take(b, 5) + 1;
                const uint32_t ncl = inf::br_take(b, 4) + 4;
                if (b.bad) { r.status = inf::ST_E_TRUNCATED; break; }
                if (nlit > 286 || ndist > 30) { r.status = inf::ST_E_DATA; break; }
                for (uint32_t i = S.lane(); i < 20; i += S.lanes()) T.cl[i] = 0;
                S.sync();
                for (uint32_t i = 0; i < ncl; ++i) {
                    inf::br_refill(b, S);
                    const uint32_t v = inf::br_take(b, 3);
                    if (S.lane() == 0) T.cl[inf::cl_order(i)] = (uint8_t)v;
                }
                if (b.bad) { r.status = inf::ST_E_TRUNCATED; break; }
                if (!inf::build_table(T.cl, 19, T.dist, inf::CL_BITS, T.dist_cnt, T.dist_sorted, true, T, S)) { r.status = inf::ST_E_DATA; break; }
                const uint32_t total = nlit + ndist;
                uint32_t i = 0, prev = 0, eob = 0;
                while (i < total) {
                    inf::br_refill(b, S);
                    const int sym = inf::decode_symbol(T.dist, inf::CL_BITS, T.dist_cnt, T.dist_sorted, b, S);
                    if (sym < 0) { st = why(b); break; }
                    uint32_t rep = 1, val = (uint32_t)sym;
                    if (sym == 16) { if (i == 0) { st = inf::ST_E_DATA; break; } rep = 3 + inf::br_take(b, 2); val = prev; }
                    else if (sym == 17) { rep = 3 + inf::br_take(b, 3); val = 0; }
                    else if (sym == 18) { rep = 11 + inf::br_take(b, 7); val = 0; }
                    if (b.bad) { st = inf::ST_E_TRUNCATED; break; }
                    if (rep > total - i) { st = inf::ST_E_DATA; break; }
                    if (i <= 256 && 256 < i + rep) eob = val;
                    for (uint32_t k = S.lane(); k < rep; k += S.lanes()) T.lens[i + k] = (uint8_t)val;
                    i += rep; prev = val;
                }
                if (!st && !eob) st = inf::ST_E_DATA; // no end-of-block code
                if (st) { r.status = st; break; }
            }
            if (!inf::build_table(T.lens, nlit, T.lit, inf::LIT_BITS, T.lit_cnt, T.lit_sorted, false, T, S) ||
                !inf::build_table(T.lens + nlit, ndist, T.dist, inf::DIST_BITS, T.dist_cnt, T.dist_sorted, false, T, S)) { r.status = inf::ST_E_DATA; break; }
            for (;;) {
                inf::br_refill(b, S);
                if (b.pos > give_up_byte) { st = P_GAVE_UP; break; }
                const int sym = inf::decode_symbol(T.lit, inf::LIT_BITS, T.lit_cnt, T.lit_sorted, b, S);
                if (sym < 0) { st = why(b); break; }
                if (sym < 256) {
                    if (o >= max_out) { st = inf::ST_E_DATA; break; }
                    if (WRITE) S.lit((uint32_t)o, (uint32_t)sym);
                    ++o;
                    continue;
                }
                if (sym == 256) break;
                if (sym >= 286) { st = inf::ST_E_DATA; break; }
                uint32_t base, extra;
                inf::length_code((uint32_t)sym - 257u, base, extra);
                const uint32_t len = base + inf::br_take(b, extra);
                inf::br_refill(b, S);
                const int ds = inf::decode_symbol(T.dist, inf::DIST_BITS, T.dist_cnt, T.dist_sorted, b, S);
                if (ds < 0) { st = why(b); break; }
                if (ds >= 30) { st = inf::ST_E_DATA; break; }
                inf::distance_code((uint32_t)ds, base, extra);
                const uint32_t dist = base + inf::br_take(b, extra);
                if (b.bad) { st = inf::ST_E_TRUNCATED; break; }
                if (len > max_out - o) { st = inf::ST_E_DATA; break; }
                if (WRITE) S.match((uint32_t)o, len, dist); // (dist <= 32 768: what lies in front of the run is a marker's business)
                o += len;
            }
            if (st) { r.status = st; break; }
        }
        r.end_bit = br_bit_pos(b); r.n_out = o;
        if (last) { r.final = 1; break; }
        if (r.end_bit >= limit_bit) break;
        if (b.pos > give_up_byte) { r.status = P_GAVE_UP; break; }
    }
    if (WRITE) S.flush();
}

// the bit range of grid piece g
INF_HD uint64_t grid_lo(uint32_t g, uint32_t piece_bytes) { return 8ull * g * piece_bytes; }
INF_HD uint64_t grid_hi(uint32_t g, uint32_t piece_bytes, uint32_t n_in)
{
    const uint64_t e = ((uint64_t)g + 1) * piece_bytes;
    return 8ull * (e < n_in ? e : (uint64_t)n_in);
}

// The count pass of one piece.  pc.start_bit given: the chain's start, run to the range end of pc.grid whatever it takes.  NO_BIT: probe
// the range of pc.grid; the start is the lowest plausible position whose run ends well (at most PROBE_TRIES are run).
template <class Sink> INF_HD void count_piece(const uint8_t *in, uint32_t n_in, uint32_t piece_bytes, Piece &pc, inf::Tables &T, Sink &S)
{
    const uint64_t hi = grid_hi(pc.grid, piece_bytes, n_in);
    Run r;
    if (pc.start_bit != NO_BIT) gz_run<false>(in, n_in, pc.start_bit, hi, NO_BIT, NO_BIT, T, S, r);
    else {
        uint64_t from = grid_lo(pc.grid, piece_bytes);
        r.end_bit = r.n_out = 0; r.final = 0; r.status = P_NO_START;
        for (uint32_t tries = 0; tries < PROBE_TRIES && from < hi; ++tries) {
            const uint64_t c = probe(in, n_in, from, hi, S);
            if (c == NO_BIT) break;
            gz_run<false>(in, n_in, c, hi, (hi + SPEC_RUN_BITS) >> 3, NO_BIT, T, S, r);
            if (r.status == inf::ST_OK) { pc.start_bit = c; break; }
            r.end_bit = r.n_out = 0; r.final = 0; r.status = P_NO_START;
            from = c + 1;
        }
    }
    pc.end_bit = r.end_bit; pc.n_out = r.n_out; pc.state = r.status | r.final << 8;
}

// The decode pass of one chain piece: its symbols at sym[c.pos .. c.pos + c.n_out) through the Sink (whose output starts at sym + c.pos).
// ST_OK, or ST_E_DATA when the run does not end where the count pass ended.
template <class Sink> INF_HD uint32_t decode_piece(const uint8_t *in, uint32_t n_in, const ChainPiece &c, inf::Tables &T, Sink &S)
{
    Run r;
    gz_run<true>(in, n_in, c.start_bit, c.end_bit, NO_BIT, c.n_out, T, S, r);
    return (r.status == inf::ST_OK && r.end_bit == c.end_bit && r.n_out == c.n_out) ? (uint32_t)inf::ST_OK : (uint32_t)inf::ST_E_DATA;
}

// the symbol a marker stands for: v = 0x8000 | k is symbol k of the WIN in front of piece c; false: in front of the member
INF_HD bool marker_source(const ChainPiece &c, uint32_t v, uint32_t &src)
{
    const uint64_t s = (uint64_t)c.pos + (v & 0x7fffu);
    src = (uint32_t)(s - WIN);
    return s >= (uint64_t)c.member_pos + WIN;
}

// The markers among the last WIN symbols of piece c become the symbols they stand for: bytes, when every piece in front has been
// resolved.  1: a marker points in front of the member's first byte.
INF_HD uint32_t resolve_piece(uint16_t *sym, const ChainPiece &c, uint32_t lane, uint32_t lanes)
{
    const uint32_t end = c.pos + c.n_out, a = c.n_out > WIN ? end - WIN : c.pos;
    uint32_t bad = 0;
    for (uint32_t i = a + lane; i < end; i += lanes) {
        const uint32_t v = sym[i];
        if (v & 0x8000u) {
            uint32_t s;
            if (marker_source(c, v, s)) sym[i] = sym[s]; else bad = 1;
        }
    }
    return bad;
}

// text[s.begin - front .. s.begin - front + s.n) from the symbols, four to a store; a marker is looked up in the piece's resolved window.
// front: the symbols in front of the call's text (0, or WIN: the carried window).  1: a marker points in front of the member's first byte.
INF_HD uint32_t narrow_slice(const uint16_t *sym, uint8_t *text, const Slice &s, const ChainPiece &c, uint32_t front, uint32_t lane, uint32_t lanes)
{
    text += s.begin - front;
    uint32_t bad = 0;
    for (uint32_t i = 4 * lane; i < s.n; i += 4 * lanes) {
        const uint32_t m = s.n - i < 4 ? s.n - i : 4;
        uint32_t w = 0;
        for (uint32_t j = 0; j < m; ++j) {
            uint32_t v = sym[s.begin + i + j];
            if (v & 0x8000u) {
                uint32_t src;
                if (marker_source(c, v, src)) v = sym[src]; else { v = 0; bad = 1; }
            }
            w |= (v & 255u) << (8 * j);
        }
        if (m == 4) memcpy(text + i, &w, 4);
        else for (uint32_t j = 0; j < m; ++j) text[i + j] = (uint8_t)(w >> (8 * j));
    }
    return bad;
}

// ---- the chain: host code of both forms -------------------------------------------------------------------------------------------------
struct Info { uint64_t n_bytes, consumed; uint32_t n_members, overflow; int32_t error; uint32_t n_pieces, n_fixups, n_rounds; };
// open: 0, or the phase in which the call leaves the member (final = 0); end_bit: where this call leaves it (open), behind its trailer (not)
struct MemberRec { uint64_t header_at, text_begin, len; uint32_t crc, isize; size_t chain_begin, chain_end; uint32_t open; uint64_t end_bit; };
struct MemberResult { uint32_t crc, bad; };
enum { E_RECORD = -100 }; // gunzip_run: a pass returned a record that no run can produce

// What faqcs_gunzip_stream_* carry from call to call (faqcs_gunzip_state of include/faqcs_mi.h without the window, which is the Backend's).
enum { PH_BETWEEN = 0, PH_STREAM = 1, PH_TRAILER = 2 };
struct State { uint64_t member_bytes, total_bytes, total_comp; uint32_t phase, bit, crc, window_bytes, members, reserved; };

// A Backend is where the compressed bytes and the passes are: the host (HostBackend) or a device (faqcs_capi_seam.hip).
//   int fetch(p, n, dst)                          comp[p .. p + n) -> dst (host memory)
//   int count_grid(grid, n_grid)                  count_piece of every grid piece (start_bit = NO_BIT, grid = its index)
//   int count_forced(pc)                          count_piece of one piece with a given start
//   int write(chain, members, front, window_bytes, total, results)
//                                                 the carried window into the symbols' front (window_bytes of it), decode, resolve, narrow: the
//                                                 text, and per member its CRC-32 and whether a marker left it
//   int window_save(take_old, take_new, text_end) the caller's window, right-aligned: the last take_old symbols of the front, then
//                                                 text[text_end - take_new .. text_end)
// Each returns 0 or a FAQCS_E_* code, which ends the call.
//
// carry == nullptr: faqcs_gunzip_device / _host -- whole members, no front.  Else faqcs_gunzip_stream_*: the walk begins where *carry says,
// the symbols have a front of WIN for the carried window (every position moves up by it; the continued member's member_pos is
// WIN - window_bytes, so a marker of its first piece resolves into the front and marker_source, resolve_piece and narrow_slice have no
// case for it), and with final = false the walk stops at the last block boundary that is resident instead of stating E_TRUNCATED: a forced
// run that the input's end cut short is taken as far as its last whole block.  *carry is rewritten only when nothing overflows, and then
// stands behind what info.n_bytes and info.consumed say.
template <class Backend>
int gunzip_run(Backend &B, uint64_t n_comp, uint32_t piece_bytes, uint32_t max_rounds, uint64_t capacity, Info &info, State *carry = nullptr, bool final = true)
{
    const uint32_t P = piece_bytes ? piece_bytes : DEFAULT_PIECE, R = max_rounds ? max_rounds : DEFAULT_ROUNDS;
    const uint32_t G = (uint32_t)((n_comp + P - 1) / P);
    const State st0 = carry ? *carry : State{0, 0, 0, PH_BETWEEN, 0, 0, 0, 0, 0};
    const uint32_t F = carry ? WIN : 0u;
    info = Info{0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<Piece> grid;
    std::vector<ChainPiece> chain;
    std::vector<MemberRec> members;
    std::vector<uint8_t> win;
    uint64_t p = 0, total = 0;
    bool walk = true;
    if (st0.phase == PH_TRAILER) { // the open member's trailer first: it completes a member that has no text in this call
        if (n_comp < 8) { if (final) info.error = (int32_t)inf::ST_E_TRUNCATED; walk = false; }
        else {
            uint8_t tr[8];
            if (int rc = B.fetch(0, 8, tr)) return rc;
            members.push_back(MemberRec{0, 0, 0, inf::le32(tr), inf::le32(tr + 4), 0, 0, 0, 64});
            p = 8;
        }
    }
    for (bool cont = st0.phase == PH_STREAM; walk; cont = false) {
        MemberRec m{p, total, 0, 0, 0, chain.size(), 0, 0, 0};
        uint64_t cur = st0.bit, next = 0;
        if (!cont) {
            uint32_t hlen = 0;
            int h = inf::H_PARTIAL;
            for (uint64_t have = 512;; have *= 8) { // the header: a window of what follows p, widened while the header is longer
                const uint64_t avail = n_comp - p, take = have < avail ? have : avail;
                if (!take) break;
                win.resize(take);
                if (int rc = B.fetch(p, (uint32_t)take, win.data())) return rc;
                h = inf::gz_header(win.data(), take, take == avail, hlen);
                if (h != inf::H_MORE) break;
            }
            if (p == n_comp || h == inf::H_END) { info.consumed = h == inf::H_END && p < n_comp ? n_comp : p; break; }
            if (h == inf::H_PARTIAL && !final) { info.consumed = p; break; } // the rest of the header comes with the next call
            if (h != inf::H_OK) { info.error = h == inf::H_HEADER ? (int32_t)inf::ST_E_HEADER : (int32_t)inf::ST_E_TRUNCATED; info.consumed = p; break; }
            cur = 8 * (p + hlen);
        }
        uint32_t rounds = 0, err = 0;
        for (bool first = true;; first = false) {
            if ((cur >> 3) >= n_comp) { if (final) err = inf::ST_E_TRUNCATED; else m.open = PH_STREAM; break; }
            const uint32_t g = (uint32_t)((cur >> 3) / P);
            Piece pc{cur, 0, 0, g, 0};
            if (!grid.empty() && grid[g].start_bit == cur) pc = grid[g];
            else {
                if (++rounds > R) { err = ST_E_SERIAL; break; }
                ++info.n_rounds;
                if (!first) ++info.n_fixups;
                if (grid.empty()) { // the first round of the call: every grid piece beside the first block
                    grid.resize(G);
                    for (uint32_t i = 0; i < G; ++i) grid[i] = Piece{NO_BIT, 0, 0, i, 0};
                    if (int rc = B.count_grid(grid.data(), G)) return rc;
                }
                if (int rc = B.count_forced(pc)) return rc;
            }
            const bool cut = !final && (pc.state & 255u) == inf::ST_E_TRUNCATED; // the input's end, not the data: the last whole block counts
            if (cut && pc.end_bit <= cur) { m.open = PH_STREAM; break; }
            if ((pc.state & 255u) && !cut) { err = pc.state & 255u; break; }
            if (pc.end_bit <= cur || pc.end_bit > 8 * n_comp) return E_RECORD; // (a record that cannot be: never follow it)
            // (32 bits: used when nothing overflows)
            chain.push_back(ChainPiece{pc.start_bit, pc.end_bit, (uint32_t)(F + total + m.len), (uint32_t)pc.n_out, cont ? F - st0.window_bytes : (uint32_t)(F + total), 0});
            m.len += pc.n_out;
            cur = pc.end_bit;
            if (cut) { m.open = PH_STREAM; break; }
            if (pc.state >> 8) { // the final block: the trailer in the next whole byte
                const uint64_t t = (pc.end_bit + 7) >> 3;
                if (t + 8 > n_comp) {
                    if (final) err = inf::ST_E_TRUNCATED; else { m.open = PH_TRAILER; cur = 8 * t; }
                    break;
                }
                uint8_t tr[8];
                if (int rc = B.fetch(t, 8, tr)) return rc;
                m.crc = inf::le32(tr); m.isize = inf::le32(tr + 4);
                next = t + 8;
                break;
            }
        }
        if (err) { chain.resize(m.chain_begin); info.error = (int32_t)err; info.consumed = p; break; }
        m.chain_end = chain.size();
        m.end_bit = m.open ? cur : 8 * next;
        total += m.len;
        members.push_back(m);
        if (m.open) { info.consumed = cur >> 3; break; }
        p = next;
    }
    const bool open_last = !members.empty() && members.back().open;
    info.n_bytes = total; info.n_members = (uint32_t)members.size() - (open_last ? 1u : 0u); info.n_pieces = (uint32_t)chain.size();
    info.overflow = (total > capacity || total >= (1ull << 32) - F) ? 1u : 0u;
    if (info.overflow || (members.empty() && !carry)) return 0;
    for (const MemberRec &m : members)
        for (size_t k = m.chain_begin; k < m.chain_end; ++k) chain[k].member_end = (uint32_t)(F + m.text_begin + m.len);
    std::vector<MemberResult> res(members.size(), MemberResult{0, 0});
    if (!chain.empty())
        if (int rc = B.write(chain, members, F, st0.phase == PH_STREAM ? st0.window_bytes : 0u, (uint32_t)total, res)) return rc;
    Pow pw;
    inf::x2n_fill(pw.x2n, 36);
    size_t n_good = members.size();
    for (size_t k = 0; k < members.size(); ++k) { // CRC and length are looked at last
        const MemberRec &m = members[k];
        const bool carried = k == 0 && st0.phase != PH_BETWEEN;
        // what zlib's crc32_combine makes of the CRC the calls in front carried and this call's share
        if (carried) res[k].crc ^= inf::multmodp(inf::x8n_modp(pw.x2n, m.len), st0.crc);
        const uint64_t len = (carried ? st0.member_bytes : 0) + m.len;
        const int32_t st = res[k].bad ? (int32_t)inf::ST_E_DATA : m.open ? 0 : (uint32_t)len != m.isize ? (int32_t)inf::ST_E_LENGTH : res[k].crc != m.crc ? (int32_t)inf::ST_E_CRC : 0;
        if (st) { info.error = st; info.n_members = (uint32_t)k; info.n_bytes = m.text_begin; info.consumed = m.header_at; n_good = k; break; }
    }
    if (!carry) return 0;
    State &s = *carry;
    for (size_t k = 0; k < n_good; ++k) {
        const MemberRec &m = members[k];
        const bool carried = k == 0 && st0.phase != PH_BETWEEN;
        if (!m.open) { ++s.members; s.member_bytes = 0; s.crc = 0; s.window_bytes = 0; s.phase = PH_BETWEEN; s.bit = 0; continue; }
        s.member_bytes = (carried ? st0.member_bytes : 0) + m.len;
        s.crc = res[k].crc;
        s.window_bytes = s.member_bytes < WIN ? (uint32_t)s.member_bytes : WIN;
        s.phase = m.open;
        s.bit = m.open == PH_STREAM ? (uint32_t)(m.end_bit & 7u) : 0u;
        if (m.len) { // (no text of it in this call: the window stands as it is)
            const uint32_t take_new = m.len < WIN ? (uint32_t)m.len : WIN;
            if (int rc = B.window_save(s.window_bytes - take_new, take_new, (uint32_t)(m.text_begin + m.len))) return rc; // (old ones: at most window_bytes of entry)
        }
    }
    s.total_bytes += info.n_bytes;
    s.total_comp += info.consumed;
    return 0;
}

// the slices of the chain's text
inline void make_slices(const std::vector<ChainPiece> &chain, std::vector<Slice> &slices)
{
    slices.clear();
    for (size_t k = 0; k < chain.size(); ++k)
        for (uint32_t a = 0; a < chain[k].n_out; a += SLICE)
            slices.push_back(Slice{chain[k].pos + a, chain[k].n_out - a < SLICE ? chain[k].n_out - a : SLICE, (uint32_t)k, 0});
}
// what the slices' results and the pieces' statuses say of every member
inline void fold_results(const std::vector<ChainPiece> &chain, const std::vector<MemberRec> &members, const std::vector<Slice> &slices, const SliceResult *sres,
                         const uint32_t *decode_status, const uint32_t *resolve_bad, std::vector<MemberResult> &res)
{
    std::vector<uint32_t> of(chain.size());
    for (size_t m = 0; m < members.size(); ++m) {
        res[m] = MemberResult{0, 0};
        for (size_t k = members[m].chain_begin; k < members[m].chain_end; ++k) { of[k] = (uint32_t)m; res[m].bad |= decode_status[k] | resolve_bad[k]; }
    }
    for (size_t s = 0; s < slices.size(); ++s) { MemberResult &r = res[of[slices[s].piece]]; r.crc ^= sres[s].crc; r.bad |= sres[s].bad; }
}

// the host statement's passes: one thread, the functions above in their order
struct HostBackend {
    const uint8_t *comp;
    uint32_t n_comp, piece_bytes;
    std::vector<uint8_t> text;
    std::vector<uint16_t> sym;
    uint8_t *window = nullptr; // faqcs_gunzip_stream_host: the caller's WIN bytes
    inf::Tables T;
    HostBackend(const uint8_t *c, uint64_t n, uint32_t pb) : comp(c), n_comp((uint32_t)n), piece_bytes(pb ? pb : DEFAULT_PIECE) { inf::HostSink<uint16_t> S{nullptr}; inf::crc_init(T, S); }
    int fetch(uint64_t p, uint32_t n, uint8_t *dst) { memcpy(dst, comp + p, n); return 0; }
    int count_grid(Piece *grid, uint32_t n_grid)
    {
        inf::HostSink<uint16_t> S{nullptr};
        for (uint32_t g = 0; g < n_grid; ++g) count_piece(comp, n_comp, piece_bytes, grid[g], T, S);
        return 0;
    }
    int count_forced(Piece &pc) { inf::HostSink<uint16_t> S{nullptr}; count_piece(comp, n_comp, piece_bytes, pc, T, S); return 0; }
    int write(const std::vector<ChainPiece> &chain, const std::vector<MemberRec> &members, uint32_t front, uint32_t window_bytes, uint32_t total,
              std::vector<MemberResult> &res)
    {
        sym.assign((size_t)front + total, 0); // (exactly: a write beyond is the sanitizers')
        for (uint32_t i = WIN - window_bytes; i < WIN && window_bytes; ++i) sym[i] = window[i];
        std::vector<uint32_t> dst(chain.size()), rbad(chain.size());
        text.assign((size_t)total, 0);
        for (size_t k = 0; k < chain.size(); ++k) { inf::HostSink<uint16_t> S{sym.data() + chain[k].pos}; dst[k] = decode_piece(comp, n_comp, chain[k], T, S); }
        for (size_t k = 0; k < chain.size(); ++k) rbad[k] = resolve_piece(sym.data(), chain[k], 0, 1);
        std::vector<Slice> slices;
        make_slices(chain, slices);
        std::vector<SliceResult> sres(slices.size());
        Pow pw;
        inf::x2n_fill(pw.x2n, 36);
        for (size_t s = 0; s < slices.size(); ++s) {
            const Slice &sl = slices[s];
            const ChainPiece &c = chain[sl.piece];
            sres[s].bad = narrow_slice(sym.data(), text.data(), sl, c, front, 0, 1);
            uint32_t crc = 0;
            for (uint32_t l = 0; l < inf::CRC_LANES; ++l) crc ^= inf::crc_slice(T, text.data() + (sl.begin - front), sl.n, l);
            sres[s].crc = inf::multmodp(inf::x8n_modp(pw.x2n, (uint64_t)c.member_end - (sl.begin + sl.n)), crc);
        }
        fold_results(chain, members, slices, sres.data(), dst.data(), rbad.data(), res);
        return 0;
    }
    int window_save(uint32_t take_old, uint32_t take_new, uint32_t text_end)
    {
        uint8_t *w = window + (WIN - take_old - take_new);
        for (uint32_t j = 0; j < take_old; ++j) w[j] = (uint8_t)sym[WIN - take_old + j]; // (the front, never `window`: w runs ahead of what it reads)
        memcpy(w + take_old, text.data() + (text_end - take_new), take_new);
        return 0;
    }
};

} // namespace faqcs_gunzip
