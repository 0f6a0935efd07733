// cli_input.h -- the input side of `faqcs_mi`: record buffers, the BGZF reader, the streaming reader (Source), the mapped reader's
// file and buffer index.  The record parser both readers call is cli_parse.h's.
#pragma once
#include "cli_common.h"
#include "cli_parse.h"

namespace {
struct RecBuf {
    uint32_t n = 0;
    bool eof = false;
    std::string error;           // a parse error is reported when the buffer is consumed (keeps input order)
    uint8_t *seq = nullptr, *qual = nullptr;
    size_t cap = 0;              // bytes in seq / qual (pinned)
    uint32_t *off = nullptr;     // BUF_READS + 1 (pinned)
    faqcs_read_result *res = nullptr; // BUF_READS (pinned)
    uint8_t *tn = nullptr;       // BUF_READS (pinned): faqcs_batch.terminal_n, filled by the parser (bit 0: first base is 'N', bit 1: last)
    // defline i is dlen[i] bytes at dbase + dpos[i]; dbase is the memory-mapped input (the mapped path leaves them there) or, on the
    // streaming path, `defs`, into which the parser copies them: set by parse_range() when the buffer is parsed
    const char *dbase = nullptr;
    std::string defs;
    std::vector<uint64_t> dpos;
    std::vector<uint32_t> dlen;
    const char *def(uint32_t i) const { return dbase + dpos[i]; }
    uint32_t deflen(uint32_t i) const { return dlen[i]; }
    uint64_t ticket = 0;
    int dev = 0;                 // index of the context (device) the buffer was submitted to

    void init(size_t bytes)
    {
        cap = bytes;
        seq = (uint8_t *)faqcs_host_alloc(cap + 64); qual = (uint8_t *)faqcs_host_alloc(cap + 64);
        off = (uint32_t *)faqcs_host_alloc((BUF_READS + 1) * sizeof(uint32_t));
        res = (faqcs_read_result *)faqcs_host_alloc(BUF_READS * sizeof(faqcs_read_result));
        tn = (uint8_t *)faqcs_host_alloc(BUF_READS + 64);
        if (!seq || !qual || !off || !res || !tn) throw Fatal("faqcs_mi: unable to allocate pinned host memory");
        memset(seq, 0, cap + 64); memset(qual, 0, cap + 64);
        dpos.reserve(BUF_READS); dlen.reserve(BUF_READS);
    }
    void grow(size_t need)
    {
        size_t nc = cap * 2;
        while (nc < need) nc *= 2;
        uint8_t *s = (uint8_t *)faqcs_host_alloc(nc + 64), *q = (uint8_t *)faqcs_host_alloc(nc + 64);
        if (!s || !q) throw Fatal("faqcs_mi: unable to allocate pinned host memory");
        memset(s, 0, nc + 64); memset(q, 0, nc + 64);
        memcpy(s, seq, cap); memcpy(q, qual, cap);
        faqcs_host_free(seq); faqcs_host_free(qual);
        seq = s; qual = q; cap = nc;
    }
    void release() { faqcs_host_free(seq); faqcs_host_free(qual); faqcs_host_free(off); faqcs_host_free(res); faqcs_host_free(tn); }
};

template <class T> class Queue {
    std::mutex m; std::condition_variable cv; std::deque<T> q;
public:
    void push(T v) { { std::lock_guard<std::mutex> l(m); q.push_back(v); } cv.notify_one(); }
    T pop() { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !q.empty(); }); T v = q.front(); q.pop_front(); return v; }
};

// A block of raw FASTQ text holding up to BUF_READS records (exactly 4 lines each), cut by the I/O thread.
struct TextBlock {
    std::vector<char> text;
    uint64_t seq_no = 0;
    uint32_t n_lines = 0;
    struct RecBuf *buf = nullptr; // destination, assigned by the I/O thread IN FILE ORDER (so the oldest block always owns one)
    bool eof = false;        // last block of the file
    bool io_error = false;     // the compressed stream failed behind this block's text (not an end of file)
};

// ---------------------------------------------------------------------------------------------------------
// BGZF input (bgzip, htslib: gzip members of <= 64 KiB that carry their compressed size in a 'BC' extra field): the members
// of a memory-mapped file are found by hopping from header to header and inflated by a pool of threads, in file order
// (fastq.cpp:8-125 reads through gzread; a single-member .gz cannot be split and stays on gzread below).
// ---------------------------------------------------------------------------------------------------------
struct BgzfReader {
    struct Task { size_t begin = 0, end = 0; std::vector<char> out; size_t n_out = 0; bool done = false; bool bad = false; };
    const uint8_t *base = nullptr;
    size_t size = 0, scan = 0;
    int fd = -1;
    std::vector<Task> ring;
    uint64_t issued = 0, taken = 0; // task numbers handed to the workers / consumed by next()
    uint64_t claimed = 0;
    bool closing = false, failed = false;
    // what follows the last whole BGZF member (ordinary gzip members appended to a bgzip file): inflated by the consumer itself
    // through zlib's gzip decoder, as gzread would go on reading; a failure there fails the input; bytes that do not start
    // with the gzip magic are trailing garbage and end the data, as in zlib
    bool tail = false, tail_init = false, tail_done = false, tail_mid = false;
    z_stream tz;
    std::vector<char> tail_out;
    std::mutex m; std::condition_variable cv_work, cv_done;
    std::vector<std::thread> workers;
    static constexpr size_t TASK_BLOCKS = 64;

    // BSIZE of the member that starts at `o` (its total size), 0 = not a BGZF member header
    static size_t member_size(const uint8_t *p, size_t avail)
    {
        if (avail < 18 || p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) return 0;
        const size_t xlen = p[10] | ((size_t)p[11] << 8);
        if (avail < 12 + xlen) return 0;
        for (size_t x = 0; x + 4 <= xlen;) {
            const uint8_t *f = p + 12 + x;
            const size_t slen = f[2] | ((size_t)f[3] << 8);
            if (f[0] == 'B' && f[1] == 'C' && slen == 2 && x + 6 <= xlen) return (size_t)(f[4] | ((size_t)f[5] << 8)) + 1;
            x += 4 + slen;
        }
        return 0;
    }
    static bool looks_like_bgzf(const std::string &path)
    {
        struct stat st;
        if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 28) return false;
        uint8_t h[64];
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) return false;
        const size_t n = fread(h, 1, sizeof h, f);
        fclose(f);
        return member_size(h, n) != 0;
    }
    bool open(const std::string &path, int n_threads)
    {
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0) { ::close(fd); fd = -1; return false; }
        size = (size_t)st.st_size;
        void *mp = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (mp == MAP_FAILED) { ::close(fd); fd = -1; return false; }
        madvise(mp, size, MADV_SEQUENTIAL);
        base = (const uint8_t *)mp;
        ring.resize((size_t)(2 * n_threads + 2));
        for (int i = 0; i < n_threads; ++i) workers.emplace_back([this] { work(); });
        return true;
    }
    // (under the lock) carve the next task out of the file: up to TASK_BLOCKS whole members
    bool issue_locked()
    {
        if (scan >= size || failed) return false;
        Task &t = ring[issued % ring.size()];
        t.begin = scan; t.done = false; t.bad = false; t.n_out = 0;
        size_t nb = 0;
        while (nb < TASK_BLOCKS && scan < size) {
            const size_t ms = member_size(base + scan, size - scan);
            if (ms < 26 || scan + ms > size) { if (nb == 0) { tail = true; return false; } break; } // not BGZF from here on: the rest goes through zlib (next_tail)
            scan += ms; ++nb;
        }
        t.end = scan;
        ++issued;
        return true;
    }
    void work()
    {
        // members are inflated by the repository's own decoder (faqcs_pargz.h, byte output); FAQCS_MI_BGZF_ZLIB=1: by zlib (A/B)
        FaqcsThreadCpu cpu_note("bgzf inflate worker");
        static const bool use_zlib = [] { const char *e = getenv("FAQCS_MI_BGZF_ZLIB"); return e && atoi(e) != 0; }();
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) return;
        std::unique_ptr<ParGzReader::MarkerInflate> mi(new ParGzReader::MarkerInflate);
        for (;;) {
            Task *t;
            {
                std::unique_lock<std::mutex> l(m);
                cv_work.wait(l, [&] { return closing || claimed < issued; });
                if (claimed >= issued) break; // closing
                t = &ring[claimed % ring.size()];
                ++claimed;
            }
            if (t->out.size() < TASK_BLOCKS * 65536 + 1024) t->out.resize(TASK_BLOCKS * 65536 + 1024); // (+ the room the decoder's copies may run over a match's end)
            size_t o = t->begin, w = 0;
            bool bad = false;
            while (o < t->end && !bad) {
                const uint8_t *p = base + o;
                const size_t ms = member_size(p, t->end - o), xlen = p[10] | ((size_t)p[11] << 8);
                const size_t hdr = 12 + xlen;
                const uint32_t isize = (uint32_t)p[ms - 4] | ((uint32_t)p[ms - 3] << 8) | ((uint32_t)p[ms - 2] << 16) | ((uint32_t)p[ms - 1] << 24);
                if (hdr + 8 > ms || isize > 65536 || w + isize + 1024 > t->out.size()) { bad = true; break; }
                if (isize && !use_zlib) {
                    // block after block to the final one: exactly isize bytes, from no more than the member's own deflate data
                    mi->begin(p + hdr, ms - hdr - 8, 0);
                    uint8_t *dst = (uint8_t *)t->out.data() + w;
                    size_t pos = 0, cap = (size_t)isize + 320;
                    auto no_room = [](size_t) -> uint8_t * { return nullptr; }; // (more than ISIZE bytes: invalid)
                    do { if (!mi->decode_block(dst, pos, cap, no_room) || pos > isize) { bad = true; break; } } while (!mi->final_block);
                    if (bad || pos != isize) { bad = true; break; }
                } else if (isize) {
                    inflateReset(&z);
                    z.next_in = const_cast<Bytef *>(p + hdr); z.avail_in = (uInt)(ms - hdr - 8);
                    z.next_out = (Bytef *)t->out.data() + w; z.avail_out = (uInt)isize;
                    const int rc = inflate(&z, Z_FINISH);
                    if (rc != Z_STREAM_END || z.avail_out != 0) { bad = true; break; }
                }
                if (isize) {
                    const uint32_t crc = (uint32_t)p[ms - 8] | ((uint32_t)p[ms - 7] << 8) | ((uint32_t)p[ms - 6] << 16) | ((uint32_t)p[ms - 5] << 24);
                    if (faqcs_crc32(0, (const uint8_t *)t->out.data() + w, isize) != crc) { bad = true; break; } // (gzread checks it too)
                    w += isize;
                }
                o += ms;
            }
            {
                std::lock_guard<std::mutex> l(m);
                t->n_out = w; t->bad = bad; t->done = true;
            }
            cv_done.notify_all();
        }
        inflateEnd(&z);
    }
    // the next run of decompressed bytes in file order (valid until the following call); 0 = end of data
    size_t next(const char *&data)
    {
        std::unique_lock<std::mutex> l(m);
        for (;;) {
            while (issued - taken < ring.size() - 1 && issue_locked()) cv_work.notify_one();
            if (taken == issued) { if (tail && !failed) { l.unlock(); return next_tail(data); } return 0; }
            Task &t = ring[taken % ring.size()];
            cv_done.wait(l, [&] { return t.done; });
            ++taken;
            if (t.bad) { failed = true; return 0; } // (a corrupt member ends the input, as a failing gzread does)
            if (t.n_out == 0) continue; // empty members (the BGZF end-of-file marker)
            data = t.out.data();
            return t.n_out;
        }
    }
    // the bytes behind the last BGZF member, through zlib (gzip members, concatenated or not); 0 = end of data or failure (`failed`)
    size_t next_tail(const char *&data)
    {
        if (tail_done) return 0;
        if (!tail_init) {
            memset(&tz, 0, sizeof tz);
            if (inflateInit2(&tz, 15 + 16) != Z_OK) { failed = true; tail_done = true; return 0; }
            tz.next_in = const_cast<Bytef *>(base + scan); tz.avail_in = 0;
            tail_out.resize(8u << 20);
            tail_init = true;
        }
        for (;;) {
            if (!tail_mid) { // at the start of a member: zlib's gz_look() takes anything that does not begin with the gzip magic,
                             // behind at least one decoded member, for trailing garbage and ends the data there WITHOUT an error
                             // (gzread.c: "if we were decoding gzip before, then this is trailing garbage") -- so does the reference
                const uint8_t *q = tz.avail_in ? (const uint8_t *)tz.next_in : base + scan;
                const size_t avail = (size_t)tz.avail_in + (size - scan);
                if (avail > 0 && (avail < 2 || q[0] != 31 || q[1] != 139)) { tail_done = true; inflateEnd(&tz); return 0; }
            }
            if (tz.avail_in == 0) {
                const size_t left = size - scan;
                if (left == 0) { tail_done = true; inflateEnd(&tz); if (tail_mid) failed = true; return 0; } // (the file ends inside a member)
                const size_t take = left < (64u << 20) ? left : (64u << 20);
                tz.next_in = const_cast<Bytef *>(base + scan); tz.avail_in = (uInt)take;
                scan += take;
            }
            tz.next_out = (Bytef *)tail_out.data(); tz.avail_out = (uInt)tail_out.size();
            const int rc = inflate(&tz, Z_NO_FLUSH);
            const size_t got = tail_out.size() - tz.avail_out;
            tail_mid = rc != Z_STREAM_END;
            if (rc == Z_STREAM_END) { // one member done: another may follow (gzread reads concatenated members)
                const Bytef *ni = tz.next_in; const uInt ai = tz.avail_in;
                if (ai == 0 && scan >= size) { tail_done = true; inflateEnd(&tz); }
                else { inflateReset(&tz); tz.next_in = const_cast<Bytef *>(ni); tz.avail_in = ai; }
            } else if (rc != Z_OK && !(rc == Z_BUF_ERROR && got == 0 && tz.avail_in == 0 && scan < size)) {
                // a data error, or the stream ends in the middle of a member (Z_BUF_ERROR with nothing left to feed)
                failed = true; tail_done = true; inflateEnd(&tz);
                if (got) { data = tail_out.data(); return got; }
                return 0;
            }
            if (got) { data = tail_out.data(); return got; }
            if (tail_done) return 0;
        }
    }
    void stop_threads()
    {
        { std::lock_guard<std::mutex> l(m); closing = true; claimed = issued; }
        cv_work.notify_all();
        for (auto &w : workers) if (w.joinable()) w.join();
        workers.clear();
    }
    void close()
    {
        if (tail_init && !tail_done) { inflateEnd(&tz); tail_done = true; }
        stop_threads();
        if (base) munmap(const_cast<uint8_t *>(base), size);
        base = nullptr;
        if (fd >= 0) ::close(fd);
        fd = -1;
    }
};

// CPUs this process can actually use: the cgroup's CPU quota when there is one (a container that shows 256 hardware threads may
// be allowed 16 of them -- the GPU boxes of this project are: cpu.max = "1600000 100000"), else the hardware's count
static unsigned effective_cpus()
{
    unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    long quota = -1, period = 100000;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) { // cgroup v2: "<quota|max> <period>"
        char q[64];
        if (fscanf(f, "%63s %ld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atol(q);
        fclose(f);
    } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { // cgroup v1
        if (fscanf(g, "%ld", &quota) != 1) quota = -1;
        fclose(g);
        if (FILE *h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(h, "%ld", &period) != 1) period = 100000; fclose(h); }
    }
    if (quota > 0 && period > 0) hw = std::min<unsigned>(hw, (unsigned)std::max<long>(1, (quota + period - 1) / period));
    return hw;
}

// The byte behind the `want`-th newline of [p, end) (want >= 1), or `end` when there are fewer; taken = the newlines passed.  The reader
// threads of the streaming path cut their input into blocks of 4 x 32 768 lines with it: 32 bytes a step instead of a memchr per line.
__attribute__((target("avx2"))) static const char *skip_lines_avx2(const char *p, const char *end, uint32_t want, uint32_t &taken)
{
    uint32_t c = 0;
    const __m256i nl = _mm256_set1_epi8('\n');
    while (p + 32 <= end) {
        unsigned m = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i *)p), nl));
        const uint32_t k = (uint32_t)__builtin_popcount(m);
        if (c + k >= want) { // the newline asked for is one of these
            for (uint32_t drop = want - c; drop > 1; --drop) m &= m - 1;
            taken = want;
            return p + __builtin_ctz(m) + 1;
        }
        c += k; p += 32;
    }
    for (; p < end; ++p) if (*p == '\n' && ++c == want) { taken = c; return p + 1; }
    taken = c;
    return end;
}
static const char *skip_lines(const char *p, const char *end, uint32_t want, uint32_t &taken)
{
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return skip_lines_avx2(p, end, want, taken);
    uint32_t c = 0;
    while (p < end && c < want) {
        const char *x = (const char *)memchr(p, '\n', (size_t)(end - p));
        if (!x) { p = end; break; }
        p = x + 1; ++c;
    }
    taken = c;
    return p;
}

// One input file: an I/O thread reads (gz or plain) and cuts the byte stream into blocks of 4 * BUF_READS lines by
// counting newlines only; a small pool of parser threads turns blocks into pinned structure-of-arrays RecBufs
// (fastq.cpp:8-125 semantics: four lines per record, a '\r' also ends a line, |seq| must equal |qual|); buffers are
// handed to the consumer strictly in file order.
struct Source {
    gzFile gz = nullptr;
    BgzfReader bgzf;
    bool use_bgzf = false;
    ParGzReader pargz; // an ordinary gzip file of some size: inflated by a pool of threads (faqcs_pargz.h)
    bool use_pargz = false;
    Queue<RecBuf *> free_q;
    Queue<TextBlock *> block_free, block_full;
    std::thread io_th, alloc_th;
    std::atomic<bool> alloc_stop{false};
    bool alone = false; // no second file is read beside this one (set before start())
    std::vector<std::thread> parsers;
    int n_parsers = 0;
    std::vector<RecBuf> bufs;
    std::vector<TextBlock> blocks;
    // ordered delivery
    std::mutex om; std::condition_variable ocv; std::map<uint64_t, RecBuf *> ready; uint64_t next_out = 0;

    void start(const std::string &p, int nbuf, int nparse)
    {
        if (!getenv("FAQCS_MI_NO_BGZF") && BgzfReader::looks_like_bgzf(p)) use_bgzf = bgzf.open(p, std::max(2, nparse));
        if (!use_bgzf && !getenv("FAQCS_MI_NO_PARGZ")) {
            // threads per file: half of the CPUs the process may use (2 ... 24; two files are read at once).  While each mate file was rendered
            // and written by one thread, 6 of 16 were better than 8 (13.2 against 11.9 M reads/s, profiles/r6n/); with the formatter
            // pool behind the readers 8 are (16.2 - 17.0 against 14.7 - 15.9, profiles/r6r/).  Files under 8 MB stay on gzread
            const unsigned hw = effective_cpus();
            const char *et = getenv("FAQCS_MI_PARGZ_THREADS"), *em = getenv("FAQCS_MI_PARGZ_MIN");
            const int nt = et && atoi(et) > 0 ? atoi(et) : (int)std::min(24u, std::max(2u, alone ? hw * 3 / 4 : hw / 2)); // (unpaired input: one file at a time)
            if (ParGzReader::eligible(p, em ? (size_t)atoll(em) : (size_t)(8u << 20))) use_pargz = pargz.open(p, nt); // (false: not ASCII, ...: gzread)
        }
        if (!use_bgzf && !use_pargz) {
            gz = gzopen(p.c_str(), "r");
            if (!gz) throw Fatal("I/O error");
            gzbuffer(gz, 1 << 20);
        }
        // the pinned buffers come from a thread of their own while the readers already work: 12 x 21 MB per file to allocate and clear,
        // and the first allocation waits for the HIP runtime to come up -- 0.17 s of every run's start until round 6, during which
        // nothing was inflated
        bufs.resize(nbuf);
        alloc_th = std::thread([this] {
            try { for (size_t i = 0; i < bufs.size() && !alloc_stop; ++i) { bufs[i].init((size_t)BUF_READS * 320); free_q.push(&bufs[i]); } } // (a short file ends before they are all there)
            catch (std::exception &e) { fprintf(stderr, "Caught the error %s\n", e.what()); _exit(EXIT_FAILURE); }
        });
        blocks.resize(nparse + 2);
        for (auto &t : blocks) block_free.push(&t);
        n_parsers = nparse;
        io_th = std::thread([this] { io_run(); });
        for (int i = 0; i < nparse; ++i) parsers.emplace_back([this] { parse_run(); });
    }

    void io_run()
    {
        FaqcsThreadCpu cpu_note("streaming reader (cuts blocks of lines)");
        std::vector<char> io(16 << 20);
        uint64_t seq_no = 0;
        auto next_block = [&] { // an empty block with the next number and, taken in that order, its destination
            TextBlock *t = block_free.pop();
            t->text.clear(); t->n_lines = 0; t->eof = false; t->io_error = false; t->seq_no = seq_no++;
            t->buf = free_q.pop();
            return t;
        };
        TextBlock *cur = next_block();
        const uint32_t want = 4 * BUF_READS;
        for (;;) {
            const char *chunk = io.data();
            size_t got;
            if (use_bgzf) { got = bgzf.next(chunk); if (got == 0 && bgzf.failed) cur->io_error = true; }
            else if (use_pargz) {
                got = pargz.next(chunk);
                if (got == 0 && pargz.failed) {
                    cur->io_error = true;
                    fprintf(stderr, "faqcs_mi: the parallel inflate of a .gz input ended with an error: the file is damaged or cut short, or a stretch of it "
                                    "inflates more than 128 : 1, which this reader refuses (FAQCS_MI_NO_PARGZ=1 reads the file through zlib's gzread)\n");
                }
            }
            else {
                const int g = gzread(gz, io.data(), (unsigned)io.size());
                got = g > 0 ? (size_t)g : 0;
                // a read that fails without being at the end of the file: the reference's gzgets() returns NULL with !gzeof() there
                // and next_read() throws (fastq.cpp:34-41)
                if (g < 0 || (g == 0 && !gzeof(gz))) cur->io_error = true;
                else if (g == 0) { int en = 0; (void)gzerror(gz, &en); if (en != Z_OK && en != Z_STREAM_END) cur->io_error = true; }
            }
            if (got == 0) break;
            const char *p = chunk, *end = p + got;
            while (p < end) {
                // take whole lines until the block holds `want` of them
                uint32_t taken = 0;
                const char *q = skip_lines(p, end, want - cur->n_lines, taken);
                const uint32_t lines = cur->n_lines + taken;
                cur->text.insert(cur->text.end(), p, q);
                cur->n_lines = lines;
                p = q;
                if (lines == want) {
                    block_full.push(cur);
                    cur = next_block();
                }
            }
        }
        if (cur->io_error) { // gzgets() hands back nothing of the line it was reading when the stream failed (it returns NULL): drop the partial line
            while (!cur->text.empty() && cur->text.back() != '\n') cur->text.pop_back();
        }
        if (!cur->text.empty() && cur->text.back() != '\n') ++cur->n_lines; // (the file ended without a final newline)
        cur->eof = true;
        block_full.push(cur);
        for (int i = 1; i < n_parsers; ++i) block_full.push(nullptr); // wake the other parsers up to exit
    }

    void parse_run()
    {
        FaqcsThreadCpu cpu_note("streaming parser");
        for (;;) {
            TextBlock *t = block_full.pop();
            if (!t) return;
            RecBuf *b = t->buf;
            parse_range(nullptr, t->text.data(), t->text.data() + t->text.size(), t->eof, b); // (the block is recycled: the deflines are copied out)
            // the stream failed behind this text: where the reference's next gzgets() returns NULL without being at the end of the
            // file (fastq.cpp:34-41); a record cut short by the failure has set its own message already
            if (t->io_error && b->error.empty()) b->error = "fastq.cpp:next_read: Unable to read header";
            const uint64_t sn = t->seq_no;
            const bool last = t->eof;
            block_free.push(t);
            { std::lock_guard<std::mutex> l(om); ready[sn] = b; }
            ocv.notify_all();
            if (last) return;
        }
    }

    RecBuf *pop() // next buffer in file order
    {
        std::unique_lock<std::mutex> l(om);
        ocv.wait(l, [&] { return ready.count(next_out) != 0; });
        RecBuf *b = ready[next_out];
        ready.erase(next_out++);
        return b;
    }

    void stop()
    {
        alloc_stop = true;
        if (alloc_th.joinable()) alloc_th.join();
        if (io_th.joinable()) io_th.join();
        for (auto &t : parsers) if (t.joinable()) t.join();
        if (gz) gzclose(gz);
        // The readers' threads are gone; the input mappings and the pinned buffers are left to the end of the process, which follows at
        // once (faqcs_mi leaves through _exit): unmapping gigabytes and unpinning half a gigabyte took 0.2 s of every run's tail
        // (FAQCS_MI_TIDY=1: give everything back here, for leak checkers)
        static const bool tidy = [] { const char *e = getenv("FAQCS_MI_TIDY"); return e && atoi(e) != 0; }();
        if (use_bgzf) { if (tidy) bgzf.close(); else bgzf.stop_threads(); }
        if (use_pargz) { if (tidy) pargz.close(); else pargz.disarm(); }
        if (tidy) for (auto &b : bufs) b.release();
    }
};

// The mapped path: uncompressed regular files (what a drop-in run on a fast scratch file system or /dev/shm sees).
// The streaming path above moves every byte through one I/O thread per file (gzread -> line count -> block -> parser), which
// tops out near 1.3 GB/s per file; here the input is memory-mapped, an index of the 32 768-record buffers is built by
// counting newlines in parallel, a pool of parser threads fills pinned structure-of-arrays buffers straight from the mapping
// (deflines stay there), and a pool of formatter threads renders the survivors of finished buffers into the output files' mappings, at
// offsets the gate thread hands out in input order.  Same reference semantics, same C ABI underneath.
struct MapFile {
    const char *p = nullptr; size_t n = 0; int fd = -1;
    bool open(const std::string &path)
    {
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { ::close(fd); fd = -1; return false; }
        n = (size_t)st.st_size;
        if (n) {
            void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { ::close(fd); fd = -1; return false; }
            p = (const char *)m;
            madvise(m, n, MADV_WILLNEED);
        }
        return true;
    }
    void close() { if (p) munmap((void *)p, n); if (fd >= 0) ::close(fd); p = nullptr; fd = -1; }
};

// plain text?  (a gzip member starts 1f 8b; anything unreadable takes the streaming path, which reports the error)
bool is_plain_regular_file(const std::string &path)
{
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return false;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    unsigned char m[2] = {0, 0};
    const size_t got = fread(m, 1, 2, f);
    fclose(f);
    return !(got == 2 && m[0] == 0x1f && m[1] == 0x8b);
}

__attribute__((target("avx2"))) size_t count_newlines_avx2(const char *p, size_t n)
{
    size_t c = 0, i = 0;
    const __m256i nl = _mm256_set1_epi8('\n');
    for (; i + 32 <= n; i += 32) c += (size_t)__builtin_popcount((unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i *)(p + i)), nl)));
    for (; i < n; ++i) c += p[i] == '\n';
    return c;
}
size_t count_newlines(const char *p, size_t n)
{
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return count_newlines_avx2(p, n);
    size_t c = 0;
    for (const char *q = p, *e = p + n; q < e;) { const char *x = (const char *)memchr(q, '\n', (size_t)(e - q)); if (!x) break; ++c; q = x + 1; }
    return c;
}

// start[k] = byte offset of record k * BUF_READS, start[n_buf] = file size.  The last buffer holds the remainder (possibly
// nothing: the streaming reader also ends with an empty buffer when the record count is a multiple of BUF_READS).
std::vector<size_t> index_buffers(const MapFile &f, unsigned threads)
{
    const size_t lines_per_buf = 4ull * BUF_READS;
    const size_t slice = std::max<size_t>(8u << 20, (f.n + threads - 1) / std::max(1u, threads));
    const size_t n_slices = f.n ? (f.n + slice - 1) / slice : 0;
    std::vector<size_t> cnt(n_slices, 0);
    std::atomic<size_t> next{0};
    auto worker1 = [&] { for (size_t i; (i = next++) < n_slices;) cnt[i] = count_newlines(f.p + i * slice, std::min(slice, f.n - i * slice)); };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < threads && t < n_slices; ++t) th.emplace_back(worker1);
    worker1();
    for (auto &t : th) t.join();
    th.clear();
    std::vector<size_t> line0(n_slices + 1, 0);
    for (size_t i = 0; i < n_slices; ++i) line0[i + 1] = line0[i] + cnt[i];
    const size_t total_nl = line0[n_slices];
    const size_t n_full = total_nl / lines_per_buf;      // boundaries after newline number lines_per_buf * k, k = 1 .. n_full
    std::vector<size_t> start(n_full + 2, 0);
    start[n_full + 1] = f.n;
    next = 0;
    auto worker2 = [&] {
        for (size_t i; (i = next++) < n_slices;) {
            // boundaries whose newline (1-based index lines_per_buf * k) falls in this slice
            size_t k = line0[i] / lines_per_buf + 1;
            if (k * lines_per_buf > line0[i + 1] || k > n_full) continue;
            const char *q = f.p + i * slice, *e = q + std::min(slice, f.n - i * slice);
            size_t seen = line0[i];
            while (q < e && k <= n_full && k * lines_per_buf <= line0[i + 1]) {
                const char *x = (const char *)memchr(q, '\n', (size_t)(e - q));
                if (!x) break;
                ++seen; q = x + 1;
                if (seen == k * lines_per_buf) { start[k] = (size_t)(q - f.p); ++k; }
            }
        }
    };
    for (unsigned t = 1; t < threads && t < n_slices; ++t) th.emplace_back(worker2);
    worker2();
    for (auto &t : th) t.join();
    return start;
}
} // namespace
