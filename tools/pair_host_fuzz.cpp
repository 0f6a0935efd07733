// pair_host_fuzz.cpp -- the host statements of the pair stage (faqcs_pair_host, faqcs_render_pair_host in faqcs_amd/csrc/faqcs_host.cpp) as a
// stand-alone program for a build with AddressSanitizer and UBSan, every buffer of exactly the size the statement may touch:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o pair_host_fuzz tools/pair_host_fuzz.cpp faqcs_amd/csrc/faqcs_host.cpp
//   usage: pair_host_fuzz SEED N
// N generated cases: two mates of 0 .. 40 records (the counts differ in half of the cases), deflines built from a small alphabet rich in
// ' ', '\t', '.', '/', digits, so that every branch of parse_id is taken at random positions, and lengths around the 16-byte steps; mate 2's
// defline is a MUTATION of mate 1's (suffix swapped, a byte changed, cut, extended, comment added) or equal; in half of the cases
// the mutations are the id-preserving ones, so that whole cases are routed.  Every case goes through a
// naive statement written here (byte-at-a-time id, record-at-a-time files into std::string) and through the library's: info, route and the
// four files with rec_offset / rec_index must be equal, the overflow rule must hold one byte short, and the sanitizers see the first byte
// past every array.  Prints "N cases: ok"; exit 1 on the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/faqcs_mi.h"

static uint64_t g_state;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "case %u: FAILED %s (line %d): ", g_case, #cond, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)
static unsigned g_case;

// exactly n elements (at least one): the sanitizer sees the first byte past what a statement may touch
template <class T> struct Exact {
    T *p = nullptr;
    size_t n;
    explicit Exact(size_t n_) : n(n_) { void *q = nullptr; if (posix_memalign(&q, 16, (n ? n : 1) * sizeof(T))) abort(); p = (T *)q; }
    Exact(const std::vector<T> &v) : Exact(v.size()) { if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
};

struct Rec { std::string def, seq, qual; faqcs_read_result res; };

static std::string random_defline()
{
    static const char alphabet[] = "ab@ \t./0129:x";
    static const uint32_t lens[] = {0, 1, 2, 3, 5, 14, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 300};
    uint32_t len = lens[below(sizeof(lens) / sizeof(lens[0]))];
    if (below(4) == 0) len = below(40);
    std::string d(len, 'q');
    const bool plain = below(3) == 0; // long ids without a delimiter
    for (auto &c : d) c = plain ? (char)('a' + below(26)) : alphabet[below(sizeof(alphabet) - 1)];
    return d;
}

// gentle: only mutations that usually keep the id (so that whole cases pass the check and every pair is routed)
static std::string mutate(const std::string &d, bool gentle)
{
    static const uint32_t keeps[] = {0, 1, 2, 6};
    std::string m = d;
    switch (gentle && below(30) ? keeps[below(4)] : below(9)) {
    case 0: case 1: break; // equal
    case 2: if (m.size() >= 2 && (m[m.size() - 2] == '/' || m[m.size() - 2] == '.')) m[m.size() - 1] = (char)('0' + below(10)); else m += "/2"; break;
    case 3: if (!m.empty()) m[below((uint32_t)m.size())] ^= 1; break;
    case 4: if (!m.empty()) m[m.size() - 1] ^= 2; break;
    case 5: if (!m.empty()) m.resize(below((uint32_t)m.size())); break;
    case 6: m += " comment/1"; break;
    case 7: m += (char)('a' + below(3)); break;
    default: if (!m.empty()) m[0] ^= 4; break;
    }
    for (auto &c : m) if (c == '\n' || c == '\r') c = '_';
    return m;
}

static std::vector<Rec> random_mate(uint32_t n, const std::vector<Rec> *other, bool gentle)
{
    std::vector<Rec> v(n);
    for (uint32_t i = 0; i < n; ++i) {
        Rec &r = v[i];
        r.def = other && i < other->size() ? mutate((*other)[i].def, gentle) : random_defline();
        const uint32_t L = below(5) == 0 ? 0 : below(70);
        r.seq.resize(L); r.qual.resize(L);
        for (uint32_t k = 0; k < L; ++k) { r.seq[k] = "ACGTN"[below(5)]; r.qual[k] = (char)(33 + below(42)); }
        if (L && below(3) == 0) for (uint32_t k = 0, e = below(L + 1); k < e; ++k) r.seq[k] = 'N';
        if (L && below(3) == 0) for (uint32_t k = L - below(L + 1); k < L; ++k) r.seq[k] = 'N';
        r.res.start = (uint16_t)below(L + 1);
        r.res.len = (uint16_t)below(L - r.res.start + 1);
        r.res.flags = (uint16_t)((below(2) ? FAQCS_F_VALID : 0) | (below(8) << 4));
        r.res.adapter = (uint16_t)below(3);
    }
    return v;
}

// one mate in arrays of exactly the stated sizes (the text in its FASTQ form; the arenas back to back)
struct Mate {
    Exact<uint8_t> text, seq, qual;
    Exact<uint32_t> off, dpos, dlen;
    Exact<faqcs_read_result> res;
    faqcs_batch b{};
    faqcs_mate m{};
    static std::vector<uint8_t> bytes(const std::vector<Rec> &v, int what)
    {
        std::vector<uint8_t> o;
        for (const Rec &r : v) {
            const std::string s = what == 0 ? r.def + "\n" + r.seq + "\n+\n" + r.qual + "\n" : what == 1 ? r.seq : r.qual;
            o.insert(o.end(), s.begin(), s.end());
        }
        return o;
    }
    explicit Mate(const std::vector<Rec> &v) : text(bytes(v, 0)), seq(bytes(v, 1)), qual(bytes(v, 2)), off(v.size() + 1), dpos(v.size()), dlen(v.size()), res(v.size())
    {
        uint32_t o = 0, t = 0;
        off.p[0] = 0;
        for (size_t i = 0; i < v.size(); ++i) {
            dpos.p[i] = t; dlen.p[i] = (uint32_t)v[i].def.size();
            t += (uint32_t)(v[i].def.size() + 2 * v[i].seq.size() + 5);
            o += (uint32_t)v[i].seq.size();
            off.p[i + 1] = o;
            res.p[i] = v[i].res;
        }
        b.seq = seq.p; b.qual = qual.p; b.offset = off.p; b.n_reads = (uint32_t)v.size(); b.n_segments = 1;
        m.batch = &b; m.results = res.p; m.text = text.p; m.def_pos = dpos.p; m.def_len = dlen.p;
    }
};

// parse_id, a byte at a time (trim.cpp:188-222)
static std::string naive_id(const std::string &d)
{
    size_t loc = d.find(' ');
    if (loc == std::string::npos) loc = d.size();
    if (loc > 1 && d[loc - 1] >= '0' && d[loc - 1] <= '9' && (d[loc - 2] == '.' || d[loc - 2] == '/')) loc -= 2;
    return d.substr(0, loc);
}

static std::string naive_record(const faqcs_params &p, const Rec &r, bool trimmed)
{
    std::string s = r.seq, q = r.qual;
    if (trimmed) {
        size_t lead = 0, trail = s.size();
        while (lead < s.size() && s[lead] == 'N') ++lead;
        while (trail > 0 && s[trail - 1] == 'N') --trail;
        for (size_t i = 0; i < s.size(); ++i) {
            int raw = (i < lead || i >= trail) ? p.input_quality_offset : (int)(signed char)q[i];
            int qs = raw - p.input_quality_offset;
            if (qs < 0) qs = 0;
            if (p.replace_to_N_q > 0 && s[i] == 'G' && qs < (int)p.replace_to_N_q) s[i] = 'N';
            q[i] = (char)(p.input_quality_offset != p.output_quality_offset ? qs + p.output_quality_offset : raw);
        }
        s = s.substr(r.res.start, r.res.len);
        q = q.substr(r.res.start, r.res.len);
    }
    return r.def + "\n" + s + "\n+\n" + q + "\n";
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: pair_host_fuzz SEED N\n"); return 2; }
    g_state = strtoull(argv[1], nullptr, 10) * 2654435761ull + 12345;
    const unsigned n_cases = (unsigned)atoi(argv[2]);
    unsigned long long n_mismatch = 0, n_records = 0;
    for (g_case = 0; g_case < n_cases; ++g_case) {
        const uint32_t n1 = below(41), n2 = below(2) ? n1 : below(41), n = n1 < n2 ? n1 : n2;
        const std::vector<Rec> v1 = random_mate(n1, nullptr, false), v2 = random_mate(n2, below(8) ? &v1 : nullptr, below(2) != 0);
        const Mate A(v1), B(v2);
        faqcs_params p{};
        p.abi_version = FAQCS_ABI_VERSION;
        p.input_quality_offset = 33;
        p.output_quality_offset = below(2) ? 33 : 64;
        p.replace_to_N_q = below(2) ? 0 : 15;
        // the naive statement
        faqcs_pair_info want{};
        std::vector<uint8_t> wroute(n, (uint8_t)FAQCS_ROUTE_NOWHERE);
        uint32_t i = 0;
        for (; i < n; ++i) {
            const std::string ia = naive_id(v1[i].def), ib = naive_id(v2[i].def);
            if (ia != ib) { want.mismatch = 1; want.id_len[0] = (uint32_t)ia.size(); want.id_len[1] = (uint32_t)ib.size(); break; }
            const bool a = v1[i].res.flags & FAQCS_F_VALID, b = v2[i].res.flags & FAQCS_F_VALID;
            wroute[i] = (uint8_t)((a ? 1 : 0) | (b ? 2 : 0));
            if (a && b) { want.paired_read_number += 2; want.paired_base_length += v1[i].res.len + v2[i].res.len; }
            else if (a || b) ++want.n_one_valid;
            else ++want.n_none_valid;
        }
        want.n_pairs = i;
        n_mismatch += want.mismatch;
        // the library's, with results and check only
        Exact<uint8_t> route(n);
        faqcs_pair_info got;
        memset(&got, 0xee, sizeof got);
        CHECK(faqcs_pair_host(&A.m, &B.m, route.p, &got) == 0, "%s", faqcs_last_error());
        CHECK(memcmp(&got, &want, sizeof got) == 0, "info differs: n_pairs %u / %u, mismatch %u / %u, id_len %u %u / %u %u", got.n_pairs, want.n_pairs, got.mismatch,
              want.mismatch, got.id_len[0], got.id_len[1], want.id_len[0], want.id_len[1]);
        CHECK(n == 0 || memcmp(route.p, wroute.data(), n) == 0, "route differs");
        faqcs_mate a0 = A.m, b0 = B.m;
        a0.results = b0.results = nullptr;
        faqcs_pair_info chk;
        CHECK(faqcs_pair_host(&a0, &b0, nullptr, &chk) == 0, "%s", faqcs_last_error());
        CHECK(chk.n_pairs == want.n_pairs && chk.mismatch == want.mismatch && chk.id_len[0] == want.id_len[0] && chk.id_len[1] == want.id_len[1] &&
              chk.paired_read_number == 0 && chk.paired_base_length == 0 && chk.n_one_valid == 0 && chk.n_none_valid == 0, "check only differs");
        // the four files, over all n pairs (those behind a mismatch are routed nowhere)
        for (int file = 0; file < 4; ++file) {
            std::string text;
            std::vector<uint32_t> woff{0}, widx;
            for (uint32_t j = 0; j < 2 * n; ++j) {
                const uint32_t pi = j >> 1, s = j & 1, r = wroute[pi];
                const bool take = file == 0 ? (s == 0 && r == 3) : file == 1 ? (s == 1 && r == 3) : file == 2 ? r == (1u << s) : (r < 4 && !(r >> s & 1));
                if (!take) continue;
                text += naive_record(p, s ? v2[pi] : v1[pi], file != 3);
                woff.push_back((uint32_t)text.size());
                widx.push_back(j);
            }
            n_records += widx.size();
            faqcs_mate ma = A.m, mb = B.m;
            if (file == 3) ma.results = mb.results = nullptr; // the discard file does not read results
            for (int pass = 0; pass < 2; ++pass) { // the exact capacity, then one byte short
                if (pass && text.empty()) break;
                const size_t cap = text.size() - (size_t)pass;
                Exact<uint8_t> out(pass ? 0 : cap);
                Exact<uint32_t> roff(pass ? 0 : widx.size() + 1), ridx(pass ? 0 : widx.size());
                faqcs_render_info info;
                memset(&info, 0xee, sizeof info);
                const faqcs_render_out ro{out.p, cap, roff.p, ridx.p, &info};
                CHECK(faqcs_render_pair_host(&p, file, &ma, &mb, route.p, n, &ro) == 0, "%s", faqcs_last_error());
                CHECK(info.n_bytes == text.size() && info.n_reads == widx.size() && info.overflow == (uint32_t)pass, "file %d: info %llu %u %u, wanted %zu %zu %d", file,
                      (unsigned long long)info.n_bytes, info.n_reads, info.overflow, text.size(), widx.size(), pass);
                if (pass) continue;
                CHECK(text.empty() || memcmp(out.p, text.data(), text.size()) == 0, "file %d: text differs", file);
                CHECK(memcmp(roff.p, woff.data(), woff.size() * 4) == 0, "file %d: rec_offset differs", file);
                CHECK(widx.empty() || memcmp(ridx.p, widx.data(), widx.size() * 4) == 0, "file %d: rec_index differs", file);
            }
        }
    }
    printf("%u cases: ok (%llu with a mismatch, %llu records rendered)\n", n_cases, n_mismatch, n_records);
    return 0;
}
