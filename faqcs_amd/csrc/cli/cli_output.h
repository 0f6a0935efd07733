// cli_output.h -- the output side of `faqcs_mi`: buffered output files, one surviving record as text, the mate-id rule of a pair of buffers.
#pragma once
#include "cli_input.h"

namespace {
// trim.cpp:188-222: length of the id part of a defline (up to the first space, minus a trailing ".N" / "/N")
size_t id_len(const char *d, size_t len)
{
    const char *sp = (const char *)memchr(d, ' ', len);
    size_t loc = sp ? (size_t)(sp - d) : len;
    if (loc > 1 && isdigit((unsigned char)d[loc - 1]) && (d[loc - 2] == '.' || d[loc - 2] == '/')) loc -= 2;
    return loc;
}

struct OutFile {
    FILE *f = nullptr; std::vector<char> buf; size_t n = 0;
    void open(const std::string &p) { f = fopen(p.c_str(), "wb"); if (!f) throw Fatal("I/O error"); buf.resize(8 << 20); n = 0; }
    // room for `need` more bytes at the returned address (the caller adds what it wrote to n): a record is assembled with one capacity
    // check, not one per field
    bool in_memory = false; // no file behind it: the text stays in buf[0 .. n) (the streaming path's formatters render into such)
    char *room(size_t need)
    {
        if (n + need > buf.size()) {
            if (in_memory) buf.resize(std::max(n + need, buf.size() + buf.size() / 2 + (1u << 20)));
            else { flush(); if (need > buf.size()) buf.resize(need); }
        }
        return buf.data() + n;
    }
    void put(const char *p, size_t len) { char *d = room(len); memcpy(d, p, len); n += len; }
    void flush() { if (f && n) fwrite(buf.data(), 1, n, f); n = 0; }
    void close() { flush(); if (f) fclose(f); f = nullptr; }
};

// one surviving record, with the reference's byte edits (trim.cpp:390-403,516-525,1191-1216; fastq.cpp:127-138), rendered at o:
// deflen + 2 * res.len + 5 bytes (def \n seq \n + \n qual \n); returns their end
char *render_read(const faqcs_params &prm, const RecBuf *b, uint32_t i, char *o)
{
    const faqcs_read_result &x = b->res[i];
    const uint32_t ro = b->off[i], len = b->off[i + 1] - ro;
    const uint32_t dl = b->deflen(i);
    memcpy(o, b->def(i), dl); o += dl; *o++ = '\n';
    const uint8_t *sp = b->seq + ro, *qp = b->qual + ro;
    if (prm.replace_to_N_q == 0 && prm.input_quality_offset == prm.output_quality_offset && len && sp[0] != 'N' && sp[len - 1] != 'N') {
        // no byte of this record is edited (trim.cpp:390-403,516-525,1191-1216): copy the kept window
        memcpy(o, sp + x.start, x.len); o += x.len; memcpy(o, "\n+\n", 3); o += 3;
        memcpy(o, qp + x.start, x.len); o += x.len; *o++ = '\n';
        return o;
    }
    uint8_t *so = (uint8_t *)o, *qo = (uint8_t *)o + x.len + 3;
    faqcs_apply_edits(&prm, sp, qp, len, &x, so, qo); // (the edited window straight into the record)
    memcpy(o + x.len, "\n+\n", 3);
    o += 2 * (size_t)x.len + 3; *o++ = '\n';
    return o;
}

// FaQCs.cpp:370-389 on the buffers of a pair: mate ids, then equal counts.  Returns the text of the error the reference throws (empty:
// the buffers pair up) and sets `note` to the line it prints first
std::string pair_check(const RecBuf *b1, const RecBuf *b2, std::string &note)
{
    const uint32_t n = std::min(b1->n, b2->n);
    for (uint32_t i = 0; i < n; ++i) {
        const char *d1 = b1->def(i), *d2 = b2->def(i);
        const size_t l1 = id_len(d1, b1->deflen(i)), l2 = id_len(d2, b2->deflen(i));
        if (l1 != l2 || memcmp(d1, d2, l1) != 0) {
            note = "Read one id (" + std::string(d1, l1) + ")\ndoes not match\nread two id (" + std::string(d2, l2) + ")\n";
            return "FaQCs.cpp:trim: I/O error";
        }
    }
    if (b1->n != b2->n) {
        const RecBuf *lng = b1->n > b2->n ? b1 : b2;
        note = std::string("Did not find a match to read ") + (b1->n > b2->n ? "one: " : "two: ") + std::string(lng->def(n), lng->deflen(n)) + "\n";
        return "FaQCs.cppI/O error"; // (the reference's own text)
    }
    return std::string();
}

// An output file that cannot be opened (FaQCs.cpp:188-223, :560-579): the reference's line, then the error for its catch in main()
static void open_output(OutFile &f, const std::string &path, const char *what)
{
    try { f.open(path); } catch (Fatal &) { fprintf(stderr, "Unable to open %s for writing %s\n", path.c_str(), what); throw; }
}
// The report of the reference's catch in main() and the end of the process, for the streaming path's errors in front of its loop: the input
// readers are running by then and may sit on their queues (unwinding past a Source whose threads run would end in std::terminate).
[[noreturn]] static void leave(const char *what) { fprintf(stderr, "Caught the error %s\n", what); fflush(nullptr); _exit(EXIT_FAILURE); }
static void open_output_or_leave(OutFile &f, const std::string &path, const char *what)
{
    try { open_output(f, path, what); } catch (Fatal &e) { leave(e.what()); }
}

void remove_file(const std::string &p)
{
    struct stat st;
    if (!p.empty() && stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode)) { // (file_util.cpp:11-20: regular files only)
        fprintf(stderr, "The output %s file exists and will be overwritten.\n", p.c_str());
        unlink(p.c_str());
    }
}
} // namespace
