// faqcs_parse_kernel.hip -- faqcs_parse_device(): FASTQ text that lies in HBM -> the packed batch faqcs_submit_device() takes.
//
// The rules are those of fastq.cpp:8-125 as parse_range (faqcs_cli.cpp) states them, written out at faqcs_parse_device in
// include/faqcs_mi.h: a line ends at '\n', its content at the first '\r' or '\n'; a record is four lines; |bases| != |qualities| and the
// four tails of a text that ends inside a record are errors of that record, and the first bad record in input order decides.
//
// Three steps on the compute stream; the host never waits for a count:
//   index    parse_count_tiles -> parse_scan_tiles -> parse_write_lines.  A tile is 16 KiB of text, read as 16-byte pieces (4 per thread,
//            consecutive lanes on consecutive pieces).  '\n' and '\r' are counted per tile, one block scans the tile sums and decides how
//            many records the text can hold and which tail error it ends in, and a second pass over the tiles writes the start of every
//            line into scratch (4 B per line).
//   records  parse_rec_totals -> parse_scan_recs -> parse_rec_apply.  One thread per record reads its four line starts, takes the content
//            of the base and quality lines (the line itself when the text holds no '\r' at all; else the line is searched for its first
//            '\r', 16 bytes per step) and checks the length rule.  A tile is 256 records; its sums stop at its first bad record.  One block
//            finds the first bad record of the text, scans the tile sums in 64 bits and completes faqcs_parse_info, overflow included.
//            The last pass writes offset, terminal_n and the defline spans of the records in front of the bad one.
//   gather   parse_gather: for_each_piece_segment (faqcs_pack_common.h) over out->offset with ParsePiece.  A lane owns one aligned 16-byte
//            piece of the two arenas, loads 16 unaligned bytes from the base line and from the quality line of its record
//            (text + source - position in the piece) and merges under a byte mask where a piece straddles records.
// The kernels use no global atomics and only vector stores.
#include "faqcs_pack_common.h"

namespace {

using namespace faqcs_pack; // the block scan, the piece walker and the byte masks

constexpr uint32_t TEXT_THREADS = 256, TEXT_PPT = 4, TEXT_PIECES = TEXT_THREADS * TEXT_PPT, TEXT_TILE = TEXT_PIECES * 16; // 16 KiB
constexpr uint32_t REC_THREADS = 256;  // records of a tile, one per thread
constexpr uint32_t NONE = 0xffffffffu;

struct TextTile { uint32_t nl, cr; };
// what the index found (device side; the host sizes nothing by it)
struct Hdr { uint32_t n_nl, has_cr, n_cand, tail_err, n_rec_tiles, pad[3]; };
// of the records of one tile IN FRONT OF its first bad record
struct RecTile { unsigned long long bytes; uint32_t first_bad, max_len; };

// 0x80 in every byte of w that equals c (exact: no carry between bytes)
__device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t c4)
{
    const uint32_t x = w ^ c4;
    const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return ~(t | x | 0x7f7f7f7fu);
}

// 0x80 in the bytes of dword j of a 16-byte piece that lie in front of byte `valid` of the piece
__device__ __forceinline__ uint32_t valid_mask(uint32_t valid, int j)
{
    const int b = (int)valid - 4 * j;
    if (b >= 4) return 0x80808080u;
    if (b <= 0) return 0u;
    return 0x80808080u & ((1u << (8 * b)) - 1u);
}

// the piece q of tile `tile`: '\n' and '\r' masks of its four dwords (bytes at or behind n_text masked out).  Reads up to 15 bytes behind the text.
__device__ __forceinline__ void load_piece(const uint8_t *__restrict__ text, unsigned long long n_text, unsigned long long pos, uint32_t (&nl)[4], uint32_t (&cr)[4])
{
    nl[0] = nl[1] = nl[2] = nl[3] = 0;
    cr[0] = cr[1] = cr[2] = cr[3] = 0;
    if (pos >= n_text) return;
    const U128u v = *reinterpret_cast<const U128u *>(text + pos);
    const uint32_t valid = n_text - pos >= 16 ? 16u : (uint32_t)(n_text - pos);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t m = valid == 16 ? 0x80808080u : valid_mask(valid, j);
        nl[j] = eq_bytes(v.w[j], 0x0a0a0a0au) & m;
        cr[j] = eq_bytes(v.w[j], 0x0d0d0d0du) & m;
    }
}

__global__ __launch_bounds__(TEXT_THREADS) void parse_count_tiles(const uint8_t *__restrict__ text, const unsigned long long n_text, TextTile *__restrict__ tiles)
{
    __shared__ uint32_t s[TEXT_THREADS / 64];
    const unsigned long long base = (unsigned long long)blockIdx.x * TEXT_TILE;
    uint32_t c = 0; // '\n' in the low half, '\r' in the high half (<= 16 384 each per tile)
#pragma unroll
    for (uint32_t p = 0; p < TEXT_PPT; ++p) {
        uint32_t nl[4], cr[4];
        load_piece(text, n_text, base + (unsigned long long)(p * TEXT_THREADS + threadIdx.x) * 16u, nl, cr);
        c += (uint32_t)(__popc(nl[0]) + __popc(nl[1]) + __popc(nl[2]) + __popc(nl[3]));
        c += (uint32_t)(__popc(cr[0]) + __popc(cr[1]) + __popc(cr[2]) + __popc(cr[3])) << 16;
    }
    uint32_t pre, tot;
    block_excl_scan<uint32_t, TEXT_THREADS>(c, s, pre, tot);
    if (threadIdx.x == 0) tiles[blockIdx.x] = TextTile{tot & 0xffffu, tot >> 16};
}

// one block: exclusive prefix of the tiles' '\n' counts, and what the text as a whole can hold
__global__ __launch_bounds__(SCAN_THREADS) void parse_scan_tiles(const uint8_t *__restrict__ text, const unsigned long long n_text, const int final,
                                                                 const TextTile *__restrict__ tiles, const uint32_t n_tiles, uint32_t *__restrict__ tile_pre,
                                                                 uint32_t *__restrict__ line_start, Hdr *__restrict__ hdr)
{
    __shared__ uint32_t s[SCAN_THREADS / 64];
    __shared__ uint32_t s_cr;
    if (threadIdx.x == 0) s_cr = 0;
    uint32_t carry = 0, any_cr = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += SCAN_THREADS) { // (n_tiles <= 2^18)
        const uint32_t t = t0 + threadIdx.x;
        TextTile v{0, 0};
        if (t < n_tiles) v = tiles[t];
        uint32_t pre, tot;
        block_excl_scan<uint32_t, SCAN_THREADS>(v.nl, s, pre, tot);
        if (t < n_tiles) tile_pre[t] = carry + pre;
        carry += tot;
        any_cr |= v.cr;
    }
    if (any_cr) s_cr = 1; // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n_nl = carry;
        const bool open = n_text > 0 && text[n_text - 1] != '\n'; // the last line has no '\n'
        Hdr h{};
        h.n_nl = n_nl;
        h.has_cr = s_cr;
        if (final) {
            const unsigned long long ltot = (unsigned long long)n_nl + (open ? 1u : 0u);
            const uint32_t rem = (uint32_t)(ltot & 3u);
            h.n_cand = (uint32_t)(ltot >> 2);
            h.tail_err = rem == 0 ? FAQCS_PARSE_OK : rem == 1 ? FAQCS_PARSE_E_SEQUENCE : rem == 2 ? FAQCS_PARSE_E_PLUS
                       : open ? FAQCS_PARSE_E_PLUS_DELIM : FAQCS_PARSE_E_QUALITY;
        } else {
            h.n_cand = n_nl >> 2;
            h.tail_err = FAQCS_PARSE_OK;
        }
        h.n_rec_tiles = (h.n_cand + REC_THREADS - 1) / REC_THREADS;
        *hdr = h;
        line_start[0] = 0;
    }
}

// line_start[j + 1] = 1 + position of the text's j-th '\n'
__global__ __launch_bounds__(TEXT_THREADS) void parse_write_lines(const uint8_t *__restrict__ text, const unsigned long long n_text, const uint32_t *__restrict__ tile_pre,
                                                                  uint32_t *__restrict__ line_start)
{
    __shared__ unsigned long long s[TEXT_THREADS / 64];
    const unsigned long long base = (unsigned long long)blockIdx.x * TEXT_TILE;
    uint32_t nl[TEXT_PPT][4];
    unsigned long long c = 0; // the four pieces' counts, 16 bits each (<= 4 096 per piece row of a tile)
#pragma unroll
    for (uint32_t p = 0; p < TEXT_PPT; ++p) {
        uint32_t cr[4];
        load_piece(text, n_text, base + (unsigned long long)(p * TEXT_THREADS + threadIdx.x) * 16u, nl[p], cr);
        c |= (unsigned long long)(__popc(nl[p][0]) + __popc(nl[p][1]) + __popc(nl[p][2]) + __popc(nl[p][3])) << (16 * p);
    }
    unsigned long long pre, tot;
    block_excl_scan<unsigned long long, TEXT_THREADS>(c, s, pre, tot);
    uint32_t row = tile_pre[blockIdx.x]; // '\n' in front of piece row p of this tile
#pragma unroll
    for (uint32_t p = 0; p < TEXT_PPT; ++p) {
        uint32_t j = row + (uint32_t)((pre >> (16 * p)) & 0xffffu);
        const unsigned long long pos = base + (unsigned long long)(p * TEXT_THREADS + threadIdx.x) * 16u;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t m = nl[p][d];
            while (m) {
                const uint32_t byte = (uint32_t)__builtin_ctz(m) >> 3;
                m &= m - 1;
                line_start[(size_t)j + 1] = (uint32_t)(pos + 4u * (uint32_t)d + byte + 1u); // (j < n_nl <= n_text: inside the index)
                ++j;
            }
        }
        row += (uint32_t)((tot >> (16 * p)) & 0xffffu);
    }
}

// length of the content of the line [a, e): up to its first '\r'.  Reads up to 15 bytes behind e.
__device__ __forceinline__ uint32_t content_len(const uint8_t *__restrict__ text, uint32_t a, uint32_t e, bool has_cr)
{
    if (!has_cr) return e - a;
    for (unsigned long long p = a; p < e; p += 16) {
        const U128u v = *reinterpret_cast<const U128u *>(text + p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t m = eq_bytes(v.w[j], 0x0d0d0d0du);
            if (m) {
                const unsigned long long x = p + 4u * (uint32_t)j + ((uint32_t)__builtin_ctz(m) >> 3);
                return x < e ? (uint32_t)(x - a) : e - a;
            }
        }
    }
    return e - a;
}

// the four lines of record k: starts of the defline, the base line and the quality line, and the content lengths of the last two
__device__ __forceinline__ void record_lines(const uint8_t *__restrict__ text, const uint32_t n_text, const uint32_t *__restrict__ line_start, const Hdr &h, uint32_t k,
                                             uint4 &ls, uint32_t &slen, uint32_t &qlen)
{
    ls = reinterpret_cast<const uint4 *>(line_start)[k]; // starts of lines 4k .. 4k + 3
    const unsigned long long l4 = 4ull * k + 4u;
    const uint32_t qe = l4 <= h.n_nl ? line_start[l4] - 1u : n_text; // (the last quality line of a final text may lack its '\n')
    slen = content_len(text, ls.y, ls.z - 1u, h.has_cr != 0);
    qlen = content_len(text, ls.w, qe, h.has_cr != 0);
}

__global__ __launch_bounds__(REC_THREADS) void parse_rec_totals(const uint8_t *__restrict__ text, const uint32_t n_text, const uint32_t *__restrict__ line_start,
                                                                const Hdr *__restrict__ hdr, uint32_t *__restrict__ rec_len, RecTile *__restrict__ rec_tiles)
{
    __shared__ unsigned long long s[REC_THREADS / 64];
    __shared__ uint32_t s_bad, s_max;
    const Hdr h = *hdr;
    for (uint32_t t = blockIdx.x; t < h.n_rec_tiles; t += gridDim.x) {
        __syncthreads();
        if (threadIdx.x == 0) { s_bad = NONE; s_max = 0; }
        __syncthreads();
        const unsigned long long k64 = (unsigned long long)t * REC_THREADS + threadIdx.x;
        const bool live = k64 < h.n_cand;
        const uint32_t k = (uint32_t)k64;
        uint32_t slen = 0, qlen = 0;
        if (live) {
            uint4 ls;
            record_lines(text, n_text, line_start, h, k, ls, slen, qlen);
            rec_len[k] = slen;
            if (slen != qlen) atomicMin(&s_bad, k); // (LDS)
        }
        __syncthreads();
        const uint32_t bad = s_bad;
        const bool counts = live && k < bad;
        if (counts) atomicMax(&s_max, slen);
        unsigned long long pre, tot;
        block_excl_scan<unsigned long long, REC_THREADS>(counts ? (unsigned long long)slen : 0ull, s, pre, tot);
        if (threadIdx.x == 0) rec_tiles[t] = RecTile{tot, bad, s_max}; // (the scan's barriers lie behind every atomicMax)
    }
}

// one block: the first bad record, the byte prefix of every tile in front of it, faqcs_parse_info
__global__ __launch_bounds__(SCAN_THREADS) void parse_scan_recs(const uint32_t n_text, const uint32_t *__restrict__ line_start, const Hdr *__restrict__ hdr,
                                                                const RecTile *__restrict__ rec_tiles, unsigned long long *__restrict__ rec_pre,
                                                                const unsigned long long capacity_bytes, const uint32_t capacity_reads,
                                                                faqcs_parse_info *__restrict__ info, uint32_t *__restrict__ offset)
{
    __shared__ unsigned long long s[SCAN_THREADS / 64];
    __shared__ uint32_t s_tb, s_max;
    const Hdr h = *hdr;
    const uint32_t nt = h.n_rec_tiles;
    if (threadIdx.x == 0) { s_tb = NONE; s_max = 0; }
    __syncthreads();
    uint32_t mine = NONE;
    for (uint32_t t = threadIdx.x; t < nt; t += SCAN_THREADS)
        if (rec_tiles[t].first_bad != NONE) { mine = t; break; } // (ascending t: the thread's first)
    if (mine != NONE) atomicMin(&s_tb, mine);
    __syncthreads();
    const uint32_t tb = s_tb;                        // the tile of the first bad record
    const uint32_t last = tb != NONE ? tb + 1u : nt; // tiles [0, last) hold the parsed records
    unsigned long long carry = 0;
    uint32_t mx = 0;
    for (uint32_t t0 = 0; t0 < last; t0 += SCAN_THREADS) {
        const uint32_t t = t0 + threadIdx.x;
        RecTile v{0, NONE, 0};
        if (t < last) v = rec_tiles[t];
        unsigned long long pre, tot;
        block_excl_scan<unsigned long long, SCAN_THREADS>(v.bytes, s, pre, tot);
        if (t < last) rec_pre[t] = carry + pre;
        carry += tot;
        mx = v.max_len > mx ? v.max_len : mx;
    }
    if (mx) atomicMax(&s_max, mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n_reads = tb != NONE ? rec_tiles[tb].first_bad : h.n_cand;
        const unsigned long long l = 4ull * n_reads; // the parsed records end where line l starts
        faqcs_parse_info o;
        o.n_bytes = carry;
        o.consumed = l == 0 ? 0ull : l <= h.n_nl ? (unsigned long long)line_start[l] : (unsigned long long)n_text;
        o.n_reads = n_reads;
        o.max_read_len = s_max;
        o.overflow = (carry > capacity_bytes || n_reads > capacity_reads || carry >= (1ull << 32)) ? 1u : 0u;
        o.error = tb != NONE ? (int32_t)FAQCS_PARSE_E_LENGTH : (int32_t)h.tail_err;
        *info = o;
        if (!o.overflow) offset[0] = 0;
    }
}

__global__ __launch_bounds__(REC_THREADS) void parse_rec_apply(const uint8_t *__restrict__ text, const uint32_t n_text, const uint32_t *__restrict__ line_start,
                                                               const Hdr *__restrict__ hdr, const uint32_t *__restrict__ rec_len, const unsigned long long *__restrict__ rec_pre,
                                                               const faqcs_parse_info *__restrict__ info, uint32_t *__restrict__ offset, uint8_t *__restrict__ terminal_n,
                                                               uint32_t *__restrict__ def_pos, uint32_t *__restrict__ def_len)
{
    __shared__ uint32_t s[REC_THREADS / 64];
    if (info->overflow) return; // nothing is written (uniform over the grid)
    const uint32_t n_reads = info->n_reads;
    const bool has_cr = hdr->has_cr != 0;
    const uint32_t nt = (n_reads + REC_THREADS - 1) / REC_THREADS;
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long k64 = (unsigned long long)t * REC_THREADS + threadIdx.x;
        const bool live = k64 < n_reads;
        const uint32_t k = (uint32_t)k64;
        const uint32_t slen = live ? rec_len[k] : 0u;
        uint32_t pre, tot;
        block_excl_scan<uint32_t, REC_THREADS>(slen, s, pre, tot); // (no overflow: n_bytes < 2^32)
        if (live) {
            const uint4 ls = reinterpret_cast<const uint4 *>(line_start)[k];
            offset[(size_t)k + 1] = (uint32_t)rec_pre[t] + pre + slen;
            terminal_n[k] = slen ? (uint8_t)((text[ls.y] == 'N' ? 1u : 0u) | (text[(size_t)ls.y + slen - 1u] == 'N' ? 2u : 0u)) : (uint8_t)0;
            if (def_pos) {
                def_pos[k] = ls.x;
                def_len[k] = content_len(text, ls.x, ls.y - 1u, has_cr);
            }
        }
    }
}

// a piece of the two arenas
struct ParsePiece {
    const uint8_t *__restrict__ text;
    const uint32_t *__restrict__ line_start, *__restrict__ offset;
    uint8_t *__restrict__ out_seq, *__restrict__ out_qual;
    uint32_t as[4], aq[4];

    __device__ __forceinline__ void clear() { as[0] = as[1] = as[2] = as[3] = aq[0] = aq[1] = aq[2] = aq[3] = 0; }
    __device__ __forceinline__ uint2 record(uint32_t k) const { return make_uint2(offset[k], offset[(size_t)k + 1]); }
    __device__ __forceinline__ void fill(const uint2 &r, uint32_t k, unsigned long long, int d, int e, unsigned long long pos)
    {
        const uint4 ls = reinterpret_cast<const uint4 *>(line_start)[k];
        const uint32_t w0 = (uint32_t)pos - r.x; // position in the record of byte d
        const U128u vs = *reinterpret_cast<const U128u *>(text + ((size_t)ls.y + w0) - d);
        const U128u vq = *reinterpret_cast<const U128u *>(text + ((size_t)ls.w + w0) - d);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t m = (d == 0 && e == 16) ? 0xffffffffu : byte_mask(range_bits(d, e), j);
            as[j] = merge_bytes(as[j], vs.w[j], m);
            aq[j] = merge_bytes(aq[j], vq.w[j], m);
        }
    }
    __device__ __forceinline__ void store(unsigned long long o) const
    {
        *reinterpret_cast<uint4 *>(out_seq + o) = make_uint4(as[0], as[1], as[2], as[3]);
        *reinterpret_cast<uint4 *>(out_qual + o) = make_uint4(aq[0], aq[1], aq[2], aq[3]);
    }
};

__global__ __launch_bounds__(GATHER_THREADS) void parse_gather(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_start, const uint32_t *__restrict__ offset,
                                                               const faqcs_parse_info *__restrict__ info, uint8_t *__restrict__ out_seq, uint8_t *__restrict__ out_qual)
{
    if (info->overflow) return;
    ParsePiece p{text, line_start, offset, out_seq, out_qual, {}, {}};
    for_each_piece_segment(offset, info->n_reads, info->n_bytes, p);
}

size_t text_tiles(unsigned long long n_text) { return (size_t)((n_text + TEXT_TILE - 1) / TEXT_TILE); }
size_t max_rec_tiles(unsigned long long n_text) { return (size_t)((n_text / 4 + 1 + REC_THREADS - 1) / REC_THREADS); } // (a record takes >= 4 bytes of a non-final text, one less at the end of a final one)
size_t round16(size_t x) { return (x + 15) & ~(size_t)15; }

struct Scratch {
    uint32_t *line_start, *rec_len, *tile_pre;
    unsigned long long *rec_pre;
    RecTile *rec_tiles;
    TextTile *tiles;
    Hdr *hdr;
};
// Every array is sized by what n_text bytes can hold at most -- a line per byte, a record per four -- because the text's line count is known
// on the device only and the host does not wait for it.
Scratch carve(void *scratch, unsigned long long n_text, size_t *total)
{
    uint8_t *p = reinterpret_cast<uint8_t *>(scratch);
    const size_t tt = text_tiles(n_text), rt = max_rec_tiles(n_text);
    Scratch s;
    size_t o = 0;
    s.line_start = reinterpret_cast<uint32_t *>(p + o); o += round16(((size_t)n_text + 8) * 4); // (+ the entry behind the last '\n', + the uint4 a record thread loads)
    s.rec_len = reinterpret_cast<uint32_t *>(p + o); o += round16(((size_t)n_text / 4 + 2) * 4);
    s.rec_pre = reinterpret_cast<unsigned long long *>(p + o); o += round16(rt * 8);
    s.rec_tiles = reinterpret_cast<RecTile *>(p + o); o += round16(rt * sizeof(RecTile));
    s.tiles = reinterpret_cast<TextTile *>(p + o); o += round16(tt * sizeof(TextTile));
    s.tile_pre = reinterpret_cast<uint32_t *>(p + o); o += round16(tt * 4);
    s.hdr = reinterpret_cast<Hdr *>(p + o); o += round16(sizeof(Hdr));
    if (total) *total = o;
    return s;
}

} // namespace

size_t faqcs_parse_scratch_bytes(unsigned long long n_text)
{
    size_t total = 0;
    (void)carve(nullptr, n_text, &total);
    return total;
}

// scratch: faqcs_parse_scratch_bytes(n_text) bytes, 16-byte aligned.  The line index, the records, faqcs_parse_info, offset / terminal_n / def_*.
hipError_t faqcs_launch_parse_index(const uint8_t *text, unsigned long long n_text, int final, void *scratch, hipStream_t st)
{
    const Scratch s = carve(scratch, n_text, nullptr);
    const size_t tt = text_tiles(n_text);
    if (tt) hipLaunchKernelGGL(parse_count_tiles, dim3((unsigned)tt), dim3(TEXT_THREADS), 0, st, text, n_text, s.tiles);
    hipLaunchKernelGGL(parse_scan_tiles, dim3(1), dim3(SCAN_THREADS), 0, st, text, n_text, final, s.tiles, (uint32_t)tt, s.tile_pre, s.line_start, s.hdr);
    if (tt) hipLaunchKernelGGL(parse_write_lines, dim3((unsigned)tt), dim3(TEXT_THREADS), 0, st, text, n_text, s.tile_pre, s.line_start);
    return hipGetLastError();
}

hipError_t faqcs_launch_parse_records(const uint8_t *text, unsigned long long n_text, const faqcs_parse_out *out, void *scratch, int n_cu, hipStream_t st)
{
    const Scratch s = carve(scratch, n_text, nullptr);
    size_t grid = max_rec_tiles(n_text);
    const size_t cap = (size_t)(n_cu > 0 ? n_cu : 256) * 8;
    if (grid > cap) grid = cap; // (the blocks stride over the tiles the index found)
    hipLaunchKernelGGL(parse_rec_totals, dim3((unsigned)grid), dim3(REC_THREADS), 0, st, text, (uint32_t)n_text, s.line_start, s.hdr, s.rec_len, s.rec_tiles);
    hipLaunchKernelGGL(parse_scan_recs, dim3(1), dim3(SCAN_THREADS), 0, st, (uint32_t)n_text, s.line_start, s.hdr, s.rec_tiles, s.rec_pre,
                       (unsigned long long)out->capacity_bytes, out->capacity_reads, out->info, out->offset);
    size_t grid2 = ((size_t)out->capacity_reads + REC_THREADS - 1) / REC_THREADS; // (more records than capacity_reads: overflow, nothing to write)
    if (grid2 > grid) grid2 = grid;
    if (grid2) hipLaunchKernelGGL(parse_rec_apply, dim3((unsigned)grid2), dim3(REC_THREADS), 0, st, text, (uint32_t)n_text, s.line_start, s.hdr, s.rec_len, s.rec_pre,
                                  out->info, out->offset, out->terminal_n, out->def_pos, out->def_len);
    return hipGetLastError();
}

// The gather behind the records (same scratch).
hipError_t faqcs_launch_parse_gather(const uint8_t *text, unsigned long long n_text, const faqcs_parse_out *out, const void *scratch, int n_cu, hipStream_t st)
{
    const Scratch s = carve(const_cast<void *>(scratch), n_text, nullptr);
    // an arena cannot take more than min(capacity, half of the text) bytes
    const unsigned grid = gather_grid(out->capacity_bytes < n_text / 2 ? out->capacity_bytes : n_text / 2, n_cu);
    if (!grid) return hipSuccess;
    hipLaunchKernelGGL(parse_gather, dim3(grid), dim3(GATHER_THREADS), 0, st, text, s.line_start, out->offset, out->info, out->seq, out->qual);
    return hipGetLastError();
}
