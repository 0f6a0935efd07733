// cli_options.h -- the flag surface of `faqcs_mi` (options.cpp:72-774): Opt, parse_args, the PhiX174 and artifact-file helpers.
#pragma once
#include "cli_common.h"

namespace {
struct Opt {
    std::vector<int> devices; // --gpus / --gpu_ids (empty: the current device)
    bool print_usage = false, protect_5 = false, replace_N = false, kmer_rarefaction = false, discard_output = false;
    bool qc_only = false, trim_only = false, filter_adapter = false, filter_phiX = false, debug = false, version = false;
    int mode = FAQCS_MODE_BWA_PLUS;
    std::string prefix = "QC", plots_file, stats_file, in1, in2, inu, out1, out2, outu, outd, output_dir, artifact_file;
    float average_quality = 0.0f, lc = 0.85f, rate = 0.2f;
    int in_off = AUTO_OFFSET, out_off = 33, quality = 5;
    unsigned num_thread = 0, min_len = 50, max_poly_n = 2, kmer = 31, num_subsample = 10, trim_5 = 0, trim_3 = 0, split_size = 1000000,
             replace_to_N_q = 0;
    std::vector<std::pair<std::string, std::string>> adapter;
    std::vector<std::string> messages;
    bool adapters_active() const { return filter_adapter || filter_phiX; }
};

const std::pair<const char *, const char *> BUILTIN_ADAPTERS[] = { // options.cpp:583-617
    {"cre-loxp-forward", "TCGTATAACTTCGTATAATGTATGCTATACGAAGTTATTACG"},
    {"cre-loxp-reverse", "AGCATATTGAAGCATATTACATACGATATGCTTCAATAATGC"},
    {"TruSeq-adapter-1", "GGGGTAGTGTGGATCCTCCTCTAGGCAGTTGGGTTATTCTAGAAGCAGATGTGTTGGCTGTTTCTGAAACTCTGGAAAA"},
    {"TruSeq-adapter-3", "CAACAGCCGGTCAAAACATCTGGAGGGTAAGCCATAAACACCTCAACAGAAAA"},
    {"PCR-primer-1", "CGATAACTTCGTATAATGTATGCTATACGAAGTTATTACG"},
    {"PCR-primer-2", "GCATAACTTCGTATAGCATACATTATACGAAGTTATACGA"},
    {"Nextera-primer-adapter-1", "GATCGGAAGAGCACACGTCTGAACTCCAGTCAC"},
    {"Nextera-primer-adapter-2", "GATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"},
    {"Nextera-junction-adapter-1", "CTGTCTCTTATACACATCTAGATGTGTATAAGAGACAG"},
};

unsigned strtou(const std::string &s)
{
    for (char c : s) if (c < '0' || c > '9') throw Fatal("options.cpp:strtou: Invalid character");
    return s.empty() ? 0u : (unsigned)strtoull(s.c_str(), nullptr, 10);
}

std::string reverse_complement(const std::string &s) // options.cpp:894-996
{
    static const char *from = "ATGCatgcMRSVWYHKDBNmrsvwyhkdbn", *to = "TACGtacgKYSBWRDMHVNkysbwrdmhvn";
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) { const char *p = strchr(from, c); if (p && c) c = to[p - from]; }
    return r;
}

std::string exe_dir()
{
    char buf[4096];
    ssize_t n = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
    if (n <= 0) return ".";
    buf[n] = 0;
    std::string s(buf);
    return s.substr(0, s.rfind('/'));
}

std::string phix_sequence()
{
    const std::string path = exe_dir() + "/data/phix174_nc_001422.txt";
    FILE *f = fopen(path.c_str(), "r");
    if (!f) throw Fatal("Unable to open the PhiX174 sequence file " + path);
    std::string seq; char line[256];
    while (fgets(line, sizeof(line), f)) {
        if (line[0] == '#') continue;
        for (char *p = line; *p; ++p) if (*p > ' ') seq.push_back(*p);
    }
    fclose(f);
    return seq;
}

void parse_artifact_file(const std::string &path, std::vector<std::pair<std::string, std::string>> &out) // options.cpp:820-891
{
    gzFile fin = gzopen(path.c_str(), "r");
    if (!fin) { fprintf(stderr, "Unable to open %s for loading artifact sequences\n", path.c_str()); throw Fatal("I/O error"); }
    char buffer[4096];
    std::string defline, data;
    while (gzgets(fin, buffer, sizeof(buffer))) {
        char *ptr = strchr(buffer, '>');
        if (ptr) {
            if (!data.empty()) out.emplace_back(defline, data);
            data.clear();
            ++ptr;
            for (char *p = ptr; *p; ++p) if (*p == '\n' || *p == '\r') *p = 0;
            defline = ptr;
        } else {
            for (char *p = buffer; *p; ++p) if (!isspace((unsigned char)*p)) data.push_back(*p);
        }
    }
    if (!data.empty()) out.emplace_back(defline, data);
    gzclose(fin);
}

struct LongOpt { const char *name; bool arg; };
const LongOpt LONG_OPTS[] = {
    {"mode", true}, {"5end", true}, {"3end", true}, {"adapter", false}, {"rate", true}, {"polyA", false}, {"artifactFile", true},
    {"min_L", true}, {"avg_q", true}, {"lc", true}, {"phiX", false}, {"ascii", true}, {"out_ascii", true}, {"prefix", true},
    {"stats", true}, {"split_size", true}, {"qc_only", false}, {"kmer_rarefaction", false}, {"subset", true}, {"discard", false},
    {"substitute", false}, {"trim_only", false}, {"5trim_off", false}, {"debug", false}, {"version", false}, {"R1", true},
    {"R2", true}, {"Ru", false}, {"Rd", false}, {"QRpdf", false}, {"replace_to_N_q", true},
    // extensions of this command line (not in the reference): --gpus N = the first N devices, --gpu_ids a,b,... = these devices
    {"gpus", true}, {"gpu_ids", true}};

Opt parse_args(int argc, char **argv)
{
    Opt o;
    o.print_usage = argc == 1;
    bool trim_polyA = false;
    for (int i = 1; i < argc;) {
        std::string a = argv[i++];
        if (a.size() < 2 || a[0] != '-') continue;
        std::string name = a.substr(a[1] == '-' ? 2 : 1), val;
        bool has_val = false;
        const size_t eq = name.find('=');
        if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has_val = true; }
        bool need = false, known = false;
        for (const LongOpt &lo : LONG_OPTS) if (name == lo.name) { need = lo.arg; known = true; }
        const std::string shorts = "dtn12pqum";
        if (!known && name.size() == 1 && (shorts.find(name[0]) != std::string::npos || name == "h" || name == "?")) {
            known = true; need = shorts.find(name[0]) != std::string::npos;
        }
        if (!known && a[1] != '-' && name.size() > 1 && shorts.find(name[0]) != std::string::npos) { // -q5
            val = name.substr(1); name = name.substr(0, 1); has_val = true; known = true; need = true;
        }
        if (!known) { // unique abbreviation, getopt_long_only style
            const LongOpt *hit = nullptr; int nhit = 0;
            for (const LongOpt &lo : LONG_OPTS) if (std::string(lo.name).compare(0, name.size(), name) == 0) { hit = &lo; ++nhit; }
            if (nhit == 1) { name = hit->name; need = hit->arg; known = true; }
        }
        if (!known) { o.print_usage = true; continue; }
        if (need && !has_val) {
            if (i >= argc) { o.print_usage = true; break; }
            val = argv[i++];
        }
        auto fl = [&](const std::string &v) { return (float)atof(v.c_str()); };
        if (name == "mode") {
            std::string m = val; for (char &c : m) c = (char)tolower(c);
            o.mode = m == "hard" ? FAQCS_MODE_HARD : m == "bwa" ? FAQCS_MODE_BWA : m == "bwa_plus" ? FAQCS_MODE_BWA_PLUS : -1;
        } else if (name == "5end") o.trim_5 = strtou(val);
        else if (name == "3end") o.trim_3 = strtou(val);
        else if (name == "adapter") o.filter_adapter = true;
        else if (name == "rate") o.rate = fl(val);
        else if (name == "polyA") trim_polyA = true;
        else if (name == "artifactFile") { o.artifact_file = val; o.filter_adapter = true; }
        else if (name == "min_L") o.min_len = strtou(val);
        else if (name == "avg_q") o.average_quality = fl(val);
        else if (name == "lc") o.lc = fl(val);
        else if (name == "phiX") o.filter_phiX = true;
        else if (name == "ascii") o.in_off = atoi(val.c_str());
        else if (name == "out_ascii") o.out_off = atoi(val.c_str());
        else if (name == "prefix") o.prefix = val;
        else if (name == "stats") o.stats_file = val;
        else if (name == "split_size") o.split_size = strtou(val);
        else if (name == "qc_only") o.qc_only = true;
        else if (name == "kmer_rarefaction") o.kmer_rarefaction = true;
        else if (name == "subset") o.num_subsample = strtou(val);
        else if (name == "discard") o.discard_output = true;
        else if (name == "substitute") o.replace_N = true;
        else if (name == "trim_only") o.trim_only = true;
        else if (name == "5trim_off") o.protect_5 = true;
        else if (name == "debug") o.debug = true;
        else if (name == "version") o.version = true;
        else if (name == "R1" || name == "1") o.in1 = val;
        else if (name == "R2" || name == "2") o.in2 = val;
        else if (name == "replace_to_N_q") o.replace_to_N_q = strtou(val);
        else if (name == "gpus") { o.devices.clear(); for (unsigned k = 0; k < strtou(val); ++k) o.devices.push_back((int)k); }
        else if (name == "gpu_ids") { o.devices.clear(); size_t b = 0; while (b <= val.size()) { const size_t e = val.find(',', b); o.devices.push_back(atoi(val.substr(b, e == std::string::npos ? e : e - b).c_str())); if (e == std::string::npos) break; b = e + 1; } }
        else if (name == "u") o.inu = val;
        else if (name == "d") o.output_dir = val;
        else if (name == "m") o.kmer = strtou(val);
        else if (name == "n") o.max_poly_n = strtou(val);
        else if (name == "q") o.quality = atoi(val.c_str());
        else if (name == "t") o.num_thread = strtou(val);
        else if (name == "h" || name == "?") o.print_usage = true;
    }
    if (o.print_usage) return o;
    if (o.version) { o.messages.push_back(std::string("Version: ") + VERSION); o.print_usage = true; return o; }
    if (o.in1.empty() != o.in2.empty()) { o.print_usage = true; return o; }      // options.cpp:506-518
    o.num_subsample *= 2;                                                          // options.cpp:519-523 (quirk b)
    if (o.inu.empty() && o.in1.empty()) { o.print_usage = true; return o; }
    if (o.kmer < 2 || o.kmer > 31 || o.lc > 1.0f || o.lc < 0.0f || o.rate > 1.0f || o.rate < 0.0f || o.split_size == 0 || o.num_subsample == 0) {
        o.print_usage = true; return o;
    }
    if (o.replace_N) o.messages.push_back("**Warning** \"-substitue\" is not currently implemented");
    if (o.filter_adapter) for (auto &a : BUILTIN_ADAPTERS) o.adapter.emplace_back(a.first, a.second);
    if (trim_polyA) o.adapter.emplace_back("polyA", std::string(20, 'A'));
    if (o.filter_phiX) {
        const std::string px = phix_sequence();
        o.adapter.emplace_back("__PhiX174_NC_001422__", px);
        o.adapter.emplace_back("__PhiX174_NC_001422_complement__", reverse_complement(px));
    }
    if (!o.artifact_file.empty()) parse_artifact_file(o.artifact_file, o.adapter);
    const std::string d = o.output_dir + "/" + o.prefix;
    if (!o.in1.empty() && !o.in2.empty()) {
        if (o.out1.empty()) o.out1 = d + ".1.trimmed.fastq";
        if (o.out2.empty()) o.out2 = d + ".2.trimmed.fastq";
        if (o.outu.empty()) o.outu = d + ".unpaired.trimmed.fastq";
        if (o.outd.empty()) o.outd = d + ".discard.trimmed.fastq";
    }
    if (!o.inu.empty()) {
        if (o.outu.empty()) o.outu = d + ".unpaired.trimmed.fastq";
        if (o.outd.empty()) o.outd = d + ".discard.trimmed.fastq";
    }
    if (o.plots_file.empty()) o.plots_file = o.output_dir + "/" + o.prefix + "_qc_report.pdf";
    if (!o.discard_output) o.outd.clear();
    if (o.stats_file.empty()) o.stats_file = d + ".stats.txt";
    if (o.mode == -1) {
        o.mode = FAQCS_MODE_BWA_PLUS;
        if (!o.qc_only) o.messages.push_back("Not recognized mode. Bwa extension trimming algorithm is used.");
    } else if (!o.qc_only) {
        o.messages.push_back(o.mode == FAQCS_MODE_HARD ? "Hard trimming is used." : o.mode == FAQCS_MODE_BWA ? "Bwa trimming is used." : "Bwa extension trimming is used.");
    }
    return o;
}
} // namespace
