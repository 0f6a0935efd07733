// cli_parse_check.cpp -- the command line's FASTQ line and record parser (faqcs_amd/csrc/cli/cli_parse.h) against a plain restatement, as
// host C++ for a build with AddressSanitizer and UBSan:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/cli_parse_check.cpp
//
// The parser fills a structure-of-arrays buffer through seq, qual, off, tn, cap, grow() and the defline arrays.  Here that buffer is heap
// memory of exactly the stated sizes (seq / qual: cap + 64 bytes, off: records + 1, tn: records), and the text a heap block of exactly its
// length, so that an access out of range is the sanitizer's to report.  Every case is parsed as one range and cut in two at every record
// boundary, with the deflines left in the text (the mapped reader) and copied out (the streaming reader), and compared -- record count, off[],
// bases, qualities, tn[], every defline, the error text, the arena's final size -- with model(): lines split byte by byte, four lines per
// record (fastq.cpp:8-125), no code shared with the header.  line_end() alone is compared with its two-memchr definition on every
// placement of '\r' and '\n' in lines of 0 ... 70 bytes.  Exit status 1 at the first difference, or when a listed case was never reached.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../faqcs_amd/csrc/cli/cli_parse.h"

// ---- the buffer: heap blocks of exactly the stated sizes, the grow rule of the command line's pinned buffer ----------------------------
struct Buf {
    uint32_t n = 0;
    bool eof = false;
    std::string error, defs;
    uint8_t *seq = nullptr, *qual = nullptr, *tn = nullptr;
    uint32_t *off = nullptr;
    size_t cap = 0;
    const char *dbase = nullptr;
    std::vector<uint64_t> dpos;
    std::vector<uint32_t> dlen;
    Buf(size_t bytes, size_t records) : cap(bytes)
    {
        seq = (uint8_t *)calloc(cap + 64, 1); qual = (uint8_t *)calloc(cap + 64, 1);
        off = (uint32_t *)malloc((records + 1) * sizeof(uint32_t));
        tn = (uint8_t *)malloc(records ? records : 1);
    }
    void grow(size_t need)
    {
        size_t nc = cap * 2;
        while (nc < need) nc *= 2;
        uint8_t *s = (uint8_t *)calloc(nc + 64, 1), *q = (uint8_t *)calloc(nc + 64, 1);
        memcpy(s, seq, cap); memcpy(q, qual, cap);
        free(seq); free(qual);
        seq = s; qual = q; cap = nc;
    }
    ~Buf() { free(seq); free(qual); free(off); free(tn); }
};

// ---- what has to come up -----------------------------------------------------------------------------------------------------------------
enum Reached {
    LF, CRLF, LONE_CR_DEF, LONE_CR_SEQ, LONE_CR_QUAL, NO_FINAL_NL, END_AFTER_DEF, END_AFTER_SEQ, END_IN_PLUS, END_AFTER_PLUS, LEN_MISMATCH,
    EMPTY_READ, N_FIRST, N_LAST, N_BOTH, N_SINGLE, GROW_TEXT, GROW_LINE, LINE_31, LINE_32 = LINE_31 + 2, LINE_33 = LINE_31 + 4,
    LINE_63 = LINE_31 + 6, LINE_64 = LINE_31 + 8, LINE_65 = LINE_31 + 10, LINE_END_SWEEP = LINE_31 + 12, N_REACHED
};
static const char *const REACHED_NAME[N_REACHED] = {
    "\\n line endings", "\\r\\n line endings", "a lone \\r in a defline", "a lone \\r in a base line", "a lone \\r in a quality line",
    "no final newline", "text ends after the defline", "text ends after the bases", "text ends inside the '+' line", "text ends after the '+' line",
    "|Sequence| != |Quality|", "an empty read", "N first", "N last", "N first and last", "the single base N", "the arena grows for the text",
    "the arena grows for a base line", "31 \\n", "31 \\r\\n", "32 \\n", "32 \\r\\n", "33 \\n", "33 \\r\\n", "63 \\n", "63 \\r\\n", "64 \\n", "64 \\r\\n",
    "65 \\n", "65 \\r\\n", "the line_end sweep"};
static bool reached[N_REACHED];

[[noreturn]] static void fail(const std::string &what, const std::string &detail)
{
    printf("FAIL: %s: %s\n", what.c_str(), detail.c_str());
    exit(1);
}

// ---- the plain restatement ---------------------------------------------------------------------------------------------------------------
struct Line { size_t begin = 0, len = 0; bool terminated = false, crlf = false, lone_cr = false; };
static std::vector<Line> split_lines(const std::string &t)
{
    std::vector<Line> v;
    size_t i = 0;
    while (i < t.size()) {
        Line l;
        l.begin = i;
        bool content_over = false;
        for (; i < t.size(); ++i) {
            if (t[i] == '\n') { l.terminated = true; ++i; break; }
            if (t[i] == '\r' && !content_over) {
                content_over = true;
                if (i + 1 < t.size() && t[i + 1] == '\n') l.crlf = true; else l.lone_cr = true;
            }
            if (!content_over) ++l.len;
        }
        v.push_back(l);
    }
    return v;
}

struct Expect {
    std::vector<std::string> def, seq, qual;
    std::vector<size_t> def_at;     // where each defline starts in the text
    std::vector<size_t> record_end; // the text offset behind each whole record
    std::string error;
    size_t cap = 0;
};
static Expect model(const std::string &t, size_t cap)
{
    Expect x;
    const std::vector<Line> ln = split_lines(t);
    if (t.size() / 2 + 128 > cap) { size_t nc = cap * 2; while (nc < t.size() / 2 + 128) nc *= 2; cap = nc; reached[GROW_TEXT] = true; }
    size_t o = 32;
    for (size_t i = 0; i < ln.size(); i += 4) {
        if (i + 1 >= ln.size()) { x.error = "fastq.cpp:next_read: Unable to read sequence"; reached[END_AFTER_DEF] = true; break; }
        const size_t slen = ln[i + 1].len;
        if (o + slen + 64 > cap) { size_t nc = cap * 2; while (nc < o + slen + 128) nc *= 2; cap = nc; reached[GROW_LINE] = true; }
        if (i + 2 >= ln.size()) { x.error = "fastq.cpp:next_read: Unable to read '+'"; reached[END_AFTER_SEQ] = true; break; }
        if (!ln[i + 2].terminated) { x.error = "fastq.cpp:next_read: Error reading '+' delimiter"; reached[END_IN_PLUS] = true; break; }
        if (i + 3 >= ln.size()) { x.error = "fastq.cpp:next_read: Unable to read quality"; reached[END_AFTER_PLUS] = true; break; }
        if (ln[i + 3].len != slen) { x.error = "fastq.cpp:next_read: |Sequence| != |Quality|"; reached[LEN_MISMATCH] = true; break; }
        x.def.push_back(t.substr(ln[i].begin, ln[i].len));
        x.def_at.push_back(ln[i].begin);
        x.seq.push_back(t.substr(ln[i + 1].begin, slen));
        x.qual.push_back(t.substr(ln[i + 3].begin, slen));
        x.record_end.push_back(i + 4 < ln.size() ? ln[i + 4].begin : t.size());
        o += slen;
        // what this record shows
        for (size_t k = i; k < i + 4; ++k) {
            if (ln[k].terminated && !ln[k].crlf && !ln[k].lone_cr) reached[LF] = true;
            if (ln[k].crlf) reached[CRLF] = true;
            static const size_t edge[6] = {31, 32, 33, 63, 64, 65};
            for (int e = 0; e < 6; ++e) if (ln[k].len == edge[e] && ln[k].terminated && !ln[k].lone_cr) reached[LINE_31 + 2 * e + (ln[k].crlf ? 1 : 0)] = true;
        }
        if (ln[i].lone_cr) reached[LONE_CR_DEF] = true;
        if (ln[i + 1].lone_cr) reached[LONE_CR_SEQ] = true;
        if (ln[i + 3].lone_cr) reached[LONE_CR_QUAL] = true;
        if (!ln[i + 3].terminated) reached[NO_FINAL_NL] = true;
        const std::string &s = x.seq.back();
        if (s.empty()) reached[EMPTY_READ] = true;
        else {
            const bool nf = s[0] == 'N', nl = s[s.size() - 1] == 'N';
            if (nf && !nl) reached[N_FIRST] = true;
            if (!nf && nl) reached[N_LAST] = true;
            if (nf && nl && s.size() > 1) reached[N_BOTH] = true;
            if (nf && s.size() == 1) reached[N_SINGLE] = true;
        }
    }
    x.cap = cap;
    return x;
}

// ---- one parse against the model -------------------------------------------------------------------------------------------------------
// [c0, c1) of `text`, the arena cap0 bytes at first; in_place: the deflines stay in the text (positions from the start of the WHOLE text)
static void check_range(const std::string &what, const std::string &text, size_t c0, size_t c1, size_t cap0, bool in_place, bool eof)
{
    const std::string sub = text.substr(c0, c1 - c0);
    const Expect x = model(sub, cap0);
    char *block = (char *)malloc(text.size() ? text.size() : 1); // exactly the text: a read behind it is the sanitizer's
    memcpy(block, text.data(), text.size());
    {
        Buf b(cap0, x.seq.size());
        b.defs = "stale"; b.dpos.assign(3, 7); b.dlen.assign(3, 7); b.error = "stale"; b.n = 77; // (what an earlier parse left)
        parse_range(in_place ? block : nullptr, block + c0, block + c1, eof, &b);
        char msg[256];
        const std::string w = what + (in_place ? " (deflines in place)" : " (deflines copied)") + " [" + std::to_string(c0) + ", " + std::to_string(c1) + ")";
        if (b.error != x.error) fail(w, "error '" + b.error + "', expected '" + x.error + "'");
        if (b.n != x.seq.size()) { snprintf(msg, sizeof msg, "%u records, expected %zu", b.n, x.seq.size()); fail(w, msg); }
        if (b.eof != eof) fail(w, "eof is not what was passed");
        if (b.cap != x.cap) { snprintf(msg, sizeof msg, "arena of %zu bytes, expected %zu", b.cap, x.cap); fail(w, msg); }
        if (b.dpos.size() != b.n || b.dlen.size() != b.n) fail(w, "the defline arrays do not hold one entry per record");
        if (b.dbase != (in_place ? block : b.defs.data())) fail(w, "dbase is not the text / the copied deflines");
        size_t o = 32;
        if (b.off[0] != 32) fail(w, "off[0] is not the 32 bytes of slack");
        for (uint32_t i = 0; i < b.n; ++i) {
            const std::string &s = x.seq[i], &q = x.qual[i];
            snprintf(msg, sizeof msg, "record %u", i);
            if (b.off[i + 1] != o + s.size()) fail(w, std::string(msg) + ": off[]");
            if (memcmp(b.seq + o, s.data(), s.size()) != 0) fail(w, std::string(msg) + ": bases");
            if (memcmp(b.qual + o, q.data(), q.size()) != 0) fail(w, std::string(msg) + ": qualities");
            const uint8_t tn = s.empty() ? 0 : (uint8_t)((s[0] == 'N' ? 1 : 0) | (s[s.size() - 1] == 'N' ? 2 : 0));
            if (b.tn[i] != tn) fail(w, std::string(msg) + ": tn[]");
            if (b.dlen[i] != x.def[i].size() || memcmp(b.dbase + b.dpos[i], x.def[i].data(), x.def[i].size()) != 0) fail(w, std::string(msg) + ": defline");
            if (in_place && b.dpos[i] != c0 + x.def_at[i]) fail(w, std::string(msg) + ": the defline's position in the text");
            o += s.size();
        }
    }
    free(block);
}

// a case: as one range, and cut in two at every record boundary; cap0 == 0: an arena that does not have to grow
static void check_case(const std::string &what, const std::string &text, size_t cap0 = 0)
{
    const size_t cap = cap0 ? cap0 : text.size() / 2 + 128;
    const Expect whole = model(text, cap);
    for (int in_place = 0; in_place < 2; ++in_place) {
        check_range(what, text, 0, text.size(), cap, in_place != 0, true);
        for (size_t cut : whole.record_end) {
            check_range(what, text, 0, cut, cap, in_place != 0, false);
            check_range(what, text, cut, text.size(), cap, in_place != 0, true);
        }
    }
}

// ---- line_end against the two-memchr definition ------------------------------------------------------------------------------------------
static void check_line_end_sweep()
{
    for (int len = 0; len <= 70; ++len)
        for (int cr = -1; cr < len; ++cr)
            for (int nl = -1; nl < len; ++nl) {
                if (cr >= 0 && cr == nl) continue;
                char *t = (char *)malloc(len ? (size_t)len : 1);
                memset(t, 'A', (size_t)len);
                if (cr >= 0) t[cr] = '\r';
                if (nl >= 0) t[nl] = '\n';
                const char *end = t + len;
                // the definition: the line ends at the first '\n', its content at the first '\r' in front of that
                const char *xnl = (const char *)memchr(t, '\n', (size_t)len);
                const char *stop = xnl ? xnl : end;
                const char *xcr = (const char *)memchr(t, '\r', (size_t)(stop - t));
                const char *want_e = xcr ? xcr : stop, *want_next = xnl ? xnl + 1 : end;
                const char *next = nullptr;
                bool term = !xnl;
                const char *e = line_end(t, end, next, term);
                if (e != want_e || next != want_next || term != (xnl != nullptr)) {
                    char msg[128];
                    snprintf(msg, sizeof msg, "%d bytes, \\r at %d, \\n at %d: content %td (expected %td), next %td (%td), terminated %d", len, cr, nl, e - t,
                             want_e - t, next - t, want_next - t, (int)term);
                    fail("line_end", msg);
                }
                free(t);
            }
    reached[LINE_END_SWEEP] = true;
}

static std::string rec(const std::string &id, const std::string &s, const std::string &q, const std::string &eol = "\n")
{
    return "@" + id + eol + s + eol + "+" + eol + q + eol;
}

int main()
{
    check_line_end_sweep();
    const std::string three = rec("r1 first", "ACGTACGT", "IIIIHHHH") + rec("r2/1", "GGGTTTAAAC", "ABCDEFGHIJ") + rec("r3.2 x", "TTTT", "!!!!");
    check_case("\\n line endings", three);
    check_case("\\r\\n line endings", rec("r1", "ACGTACGT", "IIIIHHHH", "\r\n") + rec("r2", "GGG", "ABC", "\r\n") + rec("r3", "T", "!", "\r\n"));
    check_case("a lone \\r in a defline", rec("r1\rbehind it", "ACGT", "IIII") + rec("r2", "GG", "AB"));
    check_case("a lone \\r in a base line", rec("r1", "ACGT\rTT", "IIII") + rec("r2", "GG", "AB"));
    check_case("a lone \\r in a quality line", rec("r1", "ACGT", "IIII\rJJJ") + rec("r2", "GG", "AB"));
    check_case("no final newline", three.substr(0, three.size() - 1));
    check_case("the text ends after the defline", three + "@r4\n");
    check_case("the text ends after an unterminated defline", three + "@r4");
    check_case("the text ends after the bases", three + "@r4\nACGT\n");
    check_case("the text ends inside the '+' line", three + "@r4\nACGT\n+");
    check_case("the text ends inside a longer '+' line", three + "@r4\nACGT\n+r4\r");
    check_case("the text ends after the '+' line", three + "@r4\nACGT\n+\n");
    check_case("|Sequence| != |Quality|", three + rec("r4", "ACGT", "III") + rec("r5", "AC", "II"));
    check_case("|Sequence| != |Quality| in the first record", rec("r1", "ACG", "IIII") + three);
    check_case("an empty read", rec("r1", "", "") + rec("r2", "ACGT", "IIII") + rec("r3", "", "", "\r\n"));
    check_case("N at the ends", rec("a", "NACGT", "IIIII") + rec("b", "ACGTN", "IIIII") + rec("c", "NACGN", "IIIII") + rec("d", "N", "#") + rec("e", "ANA", "III") + rec("f", "NN", "##"));
    check_case("nothing", "");
    check_case("an empty line for a record", "\n");
    // the two grow rules: an arena one byte short of what the text asks for; a base line longer than half of the text (a malformed record)
    check_case("an arena just too small for the text", three, three.size() / 2 + 127);
    check_case("an arena much too small for the text", three + three + three + three + three + three + three + three, 16);
    {
        const std::string big = three + rec("long", std::string(400, 'A'), "II") + three;
        check_case("a base line longer than half of the text", big, big.size() / 2 + 128);
        const std::string tail = three + "@long\n" + std::string(900, 'C');
        check_case("a base line longer than half of the text, and nothing behind it", tail, tail.size() / 2 + 128);
        const std::string edge = "@long\n" + std::string(400, 'C'); // 32 bytes of slack + 400 bases + 64: an arena of 496 bytes is the smallest that stays
        check_case("a base line that just fits the arena", edge, 496);
        check_case("a base line one byte too long for the arena", edge, 495);
    }
    // both kinds of line break at every position around the 32-byte step of find_break's vector loop and its scalar tail
    for (size_t len : {31u, 32u, 33u, 63u, 64u, 65u})
        for (const char *eol : {"\n", "\r\n"}) {
            std::string bases(len, 'A'), quals(len, 'I'), id(len - 1, 'd'); // ('@' + id: a defline of len bytes)
            bases[len / 2] = 'G'; quals[len - 1] = '#';
            const std::string t = rec(id, bases, quals, eol) + rec("x", "AC", "II", eol) + rec(id, bases, quals, eol);
            check_case("lines of " + std::to_string(len) + " bytes", t);
            check_case("lines of " + std::to_string(len) + " bytes, no final newline", t.substr(0, t.size() - strlen(eol)));
        }
    int missing = 0;
    for (int k = 0; k < N_REACHED; ++k) if (!reached[k]) { printf("FAIL: never reached: %s\n", REACHED_NAME[k]); ++missing; }
    if (missing) return 1;
    printf("cli_parse_check: every case equal to the restatement, %d kinds of input reached\n", (int)N_REACHED);
    return 0;
}
