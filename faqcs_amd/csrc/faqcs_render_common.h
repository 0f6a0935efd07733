// faqcs_render_common.h -- what the two renderings share (faqcs_render_kernel.hip: faqcs_render_device, one batch; faqcs_pair_kernel.hip:
// faqcs_render_pair_device, the two mates of a paired run): the size of a rendered record, the piece of the text the gather assembles and
// the layout of the scan's scratch (DESIGN.md sections 4.7 and 4.10).
#pragma once
#include "faqcs_pack_common.h"

namespace faqcs_pack {

__device__ __forceinline__ unsigned long long record_bytes(uint32_t dlen, uint32_t len) { return (unsigned long long)dlen + 2ull * len + 5ull; }

// A piece of the text.  MASKED: the trimmed streams (terminal-'N' quality masking applies); EDIT: G -> N and / or the quality re-base as well;
// PAIRED: a record's sources are those of mate 0 or of mate 1, by word 3 of its second descriptor (PAIRED = false: mate 0's, the word is unused)
template <bool MASKED, bool EDIT, bool PAIRED = false> struct RenderPiece {
    const uint8_t *__restrict__ text, *__restrict__ seq, *__restrict__ qual;
    const uint8_t *__restrict__ text1, *__restrict__ seq1, *__restrict__ qual1; // mate 1's (PAIRED)
    const uint4 *__restrict__ desc;
    uint8_t *__restrict__ out_text;
    int in, out, replace_q;
    uint32_t in4; // the input offset in every byte
    uint32_t acc[4];

    __device__ __forceinline__ void clear() { acc[0] = acc[1] = acc[2] = acc[3] = 0; }
    __device__ __forceinline__ void merge(uint32_t bits, int j, uint32_t v)
    {
        const uint32_t m = byte_mask(bits, j);
        acc[j] = merge_bytes(acc[j], v, m);
    }
    __device__ __forceinline__ uint4 record(uint32_t k) const { return desc[2 * (size_t)k]; } // {begin, end, arena position of the window, klo | khi << 16}
    __device__ __forceinline__ void fill(const uint4 &r, uint32_t k, unsigned long long o, int d, int e, unsigned long long)
    {
        const uint4 t = desc[2 * (size_t)k + 1]; // {defline position, defline length, window length, mate}
        const bool second = PAIRED && t.w != 0u;
        const uint8_t *const tx = second ? text1 : text, *const sq = second ? seq1 : seq, *const ql = second ? qual1 : qual;
        const long long rel0 = (long long)o - (long long)r.x; // record position of the piece's byte 0 (>= -15)
        const long long D = t.y, len = t.z;
        // record positions: [0, D) defline, D '\n', [D + 1, D + 1 + len) bases, "\n+\n", [D + 4 + len, D + 4 + 2 len) qualities, '\n'
        const long long ps = D + 1 - rel0, pq = D + 4 + len - rel0; // piece positions of the first base / the first quality
        const int d_lo = piece_pos(-rel0, d, e), d_hi = piece_pos(D - rel0, d, e);
        const int s_lo = piece_pos(ps, d, e), s_hi = piece_pos(ps + len, d, e);
        const int q_lo = piece_pos(pq, d, e), q_hi = piece_pos(pq + len, d, e);
        const long long plus = ps + len + 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t m = (d == 0 && e == 16) ? 0xffffffffu : byte_mask(range_bits(d, e), j);
            acc[j] = merge_bytes(acc[j], 0x0a0a0a0au, m);
        }
        if (d_hi > d_lo) {
            const U128u v = *reinterpret_cast<const U128u *>(tx + ((long long)t.x + rel0));
#pragma unroll
            for (int j = 0; j < 4; ++j) merge(range_bits(d_lo, d_hi), j, v.w[j]);
        }
        if (s_hi > s_lo) {
            const long long src = (long long)r.z - ps; // piece byte x is window position x - ps
            const U128u v = *reinterpret_cast<const U128u *>(sq + src);
            U128u vq = v;
            if (EDIT && replace_q > 0) vq = *reinterpret_cast<const U128u *>(ql + src);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t s = v.w[j], q = vq.w[j];
                // (a 'G' never lies in a terminal 'N' run: its quality needs no masking here)
                if (EDIT && replace_q > 0) edit_dword(s, q, in, out, replace_q);
                merge(range_bits(s_lo, s_hi), j, s);
            }
        }
        if (q_hi > q_lo) {
            const long long src = (long long)r.z - pq;
            const U128u v = *reinterpret_cast<const U128u *>(ql + src);
            const uint32_t klo = r.w & 0xffffu, khi = r.w >> 16;
            const bool flagged = MASKED && (klo != 0u || (long long)khi != len);
            // piece bytes that keep their quality: window positions [klo, khi) -> piece bytes [klo + pq, khi + pq)
            const uint32_t keep = range_bits(piece_pos(pq + klo, q_lo, q_hi), piece_pos(pq + khi, q_lo, q_hi));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t s = 0, q = v.w[j];
                if (flagged) q = mask_terminal_quality(q, keep, j, in4);
                if (EDIT) edit_dword(s, q, in, out, 0);
                merge(range_bits(q_lo, q_hi), j, q);
            }
        }
        if (plus >= d && plus < e) {
#pragma unroll
            for (int j = 0; j < 4; ++j) merge(1u << (int)plus, j, 0x2b2b2b2bu); // '+'
        }
    }
    __device__ __forceinline__ void store(unsigned long long o) const { *reinterpret_cast<uint4 *>(out_text + o) = make_uint4(acc[0], acc[1], acc[2], acc[3]); }
};

// the scratch of a rendering's scan over n candidates: descriptors (32 bytes per candidate), tile prefixes, tile sums, record offsets (n + 1)
inline size_t render_tile_count(uint32_t n) { return ((size_t)n + TILE_ITEMS - 1) / TILE_ITEMS; }
inline size_t render_scratch_bytes(uint32_t n)
{
    const size_t nt = render_tile_count(n);
    return (size_t)n * 2 * sizeof(uint4) + nt * sizeof(TilePrefix) + nt * sizeof(TileSum) + ((size_t)n + 1) * sizeof(uint32_t) + 64;
}
struct RenderScratch { uint4 *desc; TilePrefix *prefix; TileSum *tiles; uint32_t *offs; };
inline RenderScratch render_carve(void *scratch, uint32_t n)
{
    const size_t nt = render_tile_count(n);
    RenderScratch s;
    s.desc = reinterpret_cast<uint4 *>(scratch);
    s.prefix = reinterpret_cast<TilePrefix *>(s.desc + 2 * (size_t)n);
    s.tiles = reinterpret_cast<TileSum *>(s.prefix + nt);
    s.offs = reinterpret_cast<uint32_t *>(s.tiles + nt);
    return s;
}

} // namespace faqcs_pack
