// cli_parse.h -- the FASTQ line and record parser of `faqcs_mi` (fastq.cpp:8-125), stated once for the streaming and the mapped reader.
// Plain host C++: no faqcs_mi.h, no HIP.  The parser is a template on the buffer type so that tools/cli_parse_check.cpp can run it
// under the sanitizers on heap blocks of exactly the stated size; the command line's buffer is cli_input.h's RecBuf.
#pragma once
#include <immintrin.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace {
// first '\n' or '\r' in [p, end) (end if none), 32 bytes per step where the CPU has AVX2
__attribute__((target("avx2"))) const char *find_break_avx2(const char *p, const char *end)
{
    const __m256i nl = _mm256_set1_epi8('\n'), cr = _mm256_set1_epi8('\r');
    for (; p + 32 <= end; p += 32) {
        const __m256i v = _mm256_loadu_si256((const __m256i *)p);
        const unsigned m = (unsigned)_mm256_movemask_epi8(_mm256_or_si256(_mm256_cmpeq_epi8(v, nl), _mm256_cmpeq_epi8(v, cr)));
        if (m) return p + __builtin_ctz(m);
    }
    for (; p < end; ++p) if (*p == '\n' || *p == '\r') return p;
    return end;
}
const char *find_break(const char *p, const char *end)
{
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return find_break_avx2(p, end);
    for (; p < end; ++p) if (*p == '\n' || *p == '\r') return p;
    return end;
}
// [p, return) is the line content: up to the first '\n' or '\r' (strpbrk in the reference); next = behind the line's '\n' (end when
// there is none: terminated = false).  One pass over the line
inline const char *line_end(const char *p, const char *end, const char *&next, bool &terminated)
{
    const char *x = find_break(p, end);
    if (x == end) { terminated = false; next = end; return end; }
    if (*x == '\n') { terminated = true; next = x + 1; return x; }
    const char *nlp = (const char *)memchr(x, '\n', (size_t)(end - x));
    terminated = nlp != nullptr;
    next = nlp ? nlp + 1 : end;
    return x;
}

// fastq.cpp:8-125 on the text [p, end): four lines per record, a '\r' also ends a line, |bases| must equal |qualities|.  Fills the
// structure-of-arrays buffer *b (n, eof, error, seq, qual, off, tn; cap and grow() for its arena) from 32 bytes of slack on; a malformed
// record sets b->error and ends the parse with the records in front of it counted.  Deflines are position + length (dpos / dlen)
// relative to b->dbase: `base` when the text stays where it is (a mapping), else (base == nullptr: a block that is recycled) they are
// copied into b->defs, whose address is taken only when the parse is over -- it moves while it grows.
template <class Buf> void parse_range(const char *base, const char *p, const char *end, bool eof, Buf *b)
{
    b->n = 0; b->eof = eof; b->error.clear(); b->defs.clear(); b->dpos.clear(); b->dlen.clear();
    size_t o = 32; // slack in front of the first read
    b->off[0] = (uint32_t)o;
    // a record is defline + bases + '+' line + qualities, |bases| == |qualities|: an arena takes less than half of the text
    if ((size_t)(end - p) / 2 + 128 > b->cap) b->grow((size_t)(end - p) / 2 + 128);
    while (p < end) {
        const char *nx; bool term;
        const char *e = line_end(p, end, nx, term);
        const size_t dl = (size_t)(e - p);
        const uint64_t dp = base ? (uint64_t)(p - base) : (uint64_t)b->defs.size();
        if (!base) b->defs.append(p, dl);
        p = nx;
        if (p >= end) { b->error = "fastq.cpp:next_read: Unable to read sequence"; break; }
        e = line_end(p, end, nx, term);
        const size_t slen = (size_t)(e - p);
        if (o + slen + 64 > b->cap) b->grow(o + slen + 128); // (only a malformed record: a base line longer than half of the text)
        memcpy(b->seq + o, p, slen);
        p = nx;
        if (p >= end) { b->error = "fastq.cpp:next_read: Unable to read '+'"; break; }
        (void)line_end(p, end, nx, term);
        if (!term) { b->error = "fastq.cpp:next_read: Error reading '+' delimiter"; break; }
        p = nx;
        if (p >= end) { b->error = "fastq.cpp:next_read: Unable to read quality"; break; }
        e = line_end(p, end, nx, term);
        const size_t qlen = (size_t)(e - p);
        if (slen != qlen) { b->error = "fastq.cpp:next_read: |Sequence| != |Quality|"; break; }
        memcpy(b->qual + o, p, qlen);
        p = nx;
        b->tn[b->n] = slen ? (uint8_t)((b->seq[o] == 'N' ? 1 : 0) | (b->seq[o + slen - 1] == 'N' ? 2 : 0)) : (uint8_t)0;
        o += slen;
        b->dpos.push_back(dp); b->dlen.push_back((uint32_t)dl);
        ++b->n;
        b->off[b->n] = (uint32_t)o;
    }
    b->dbase = base ? base : b->defs.data();
}
} // namespace
