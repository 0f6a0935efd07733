// cli_process.h -- how `faqcs_mi` runs as a process: the worker-process decision, the "outputs complete" byte, the host-only self checks.
#pragma once
#include "cli_input.h"
#include "cli_report.h"

namespace {
// Whether the command runs in a forked worker (see report_done() below) or in this process.
static bool worker_process_wanted()
{
    const char *nf = getenv("FAQCS_MI_NO_FORK");
    // One process when asked for, and ALWAYS under a profiler: rocprofv3 --pmc has initialised the GPU before main() runs, a child
    // forked from such a process must not touch it, and the tool would follow the wrong process anyway.  LD_PRELOAD by
    // itself is not that sign (job launchers preload guards of their own that never touch the GPU): only a profiler's library in it.
    static const char *const tool_env[] = {"ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_FORCE_LOAD", "ROCPROF_OUTPUT_PATH",
                                           "ROCPROFILER_LIBRARY_CTOR", "HSA_TOOLS_LIB", "ROCP_METRICS"};
    bool tool = false;
    for (const char *name : tool_env) { const char *v = getenv(name); if (v && *v) tool = true; }
    if (const char *pre = getenv("LD_PRELOAD")) {
        static const char *const prof[] = {"rocprof", "roctracer", "roctx", "rocsys", "omnitrace", "rocpd"};
        for (const char *w : prof) if (strstr(pre, w)) tool = true;
    }
    return !(nf && atoi(nf) != 0) && !tool;
}

// Host-only self checks (no device is touched): `faqcs_mi --bgzf_cat <file>` writes the inflated bytes of a BGZF file to stdout
// through BgzfReader, `faqcs_mi --report_script <FaQCs options...>` prints the R script the report step would pipe,
// `faqcs_mi --process_plan` says whether a command started in this environment would run in a worker process.
int host_self_check(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "--process_plan")) { puts(worker_process_wanted() ? "worker" : "one process"); return 0; }
    if (argc >= 3 && !strcmp(argv[1], "--bgzf_cat")) {
        if (!BgzfReader::looks_like_bgzf(argv[2])) { fprintf(stderr, "not a BGZF file\n"); return 2; }
        BgzfReader r;
        if (!r.open(argv[2], 4)) { fprintf(stderr, "I/O error\n"); return 1; }
        const char *data;
        size_t n;
        while ((n = r.next(data)) != 0) fwrite(data, 1, n, stdout);
        const bool bad = r.failed;
        r.close();
        fflush(stdout);
        return bad ? 3 : 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "--pargz_cat")) { // --pargz_cat <file.gz> [threads] [piece bytes]: the parallel inflate of an ordinary gzip file to stdout
        ParGzReader r;
        const int nt = argc >= 4 ? atoi(argv[3]) : 8;
        const size_t piece = argc >= 5 ? (size_t)atoll(argv[4]) : 0;
        if (!ParGzReader::eligible(argv[2], 18)) { fprintf(stderr, "not a gzip file\n"); return 2; }
        if (const char *e = getenv("FAQCS_MI_PARGZ_REARM")) r.rearm_min = (size_t)atoll(e); // (tests: short members take the parallel reader again)
        if (!r.open(argv[2], nt, piece)) { fprintf(stderr, "not eligible (not ASCII, or the first piece does not inflate)\n"); return 4; }
        const char *data;
        size_t n;
        const char *nap = getenv("FAQCS_PARGZ_CAT_SLEEP_US"); // (tests: a consumer slower than the inflate)
        while ((n = r.next(data)) != 0) { fwrite(data, 1, n, stdout); if (nap) usleep((useconds_t)atoi(nap)); }
        const bool bad = r.failed;
        if (getenv("FAQCS_PARGZ_STATS")) {
            const size_t used = r.crc_index.size();
            fprintf(stderr, "pieces %zu (of %zu bytes), on the chain %zu, bytes out %zu, failed %d\n", r.armed_pieces, r.piece_bytes, used, r.total_out, (int)bad);
        }
        r.close();
        fflush(stdout);
        return bad ? 3 : 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "--report_script")) {
        std::vector<char *> av{argv[0]};
        for (int i = 2; i < argc; ++i) av.push_back(argv[i]);
        Opt o = parse_args((int)av.size(), av.data());
        const std::string t = report_script(o);
        fwrite(t.data(), 1, t.size(), stdout);
        return 0;
    }
    return -1;
}

// The command runs in a worker process; the process the caller started returns as soon as the worker says that every output
// file is complete (one status byte through a pipe), while the worker goes on releasing what it holds -- the HIP context, a
// gigabyte of pinned buffers, ten gigabytes of file mappings: 0.47 s of the 1.67 s an 8 M-pair run took, none of which the caller
// has any use for.  FAQCS_MI_NO_FORK=1 keeps everything in one process (debuggers, profilers that follow the first process).
static int g_done_fd = -1;
static void report_done(int status)
{
    if (g_done_fd < 0) return;
    fflush(nullptr);
    prctl(PR_SET_PDEATHSIG, 0); // (the parent exits on the byte below, as planned: the teardown is not to be cut short by its death signal)
    // From here on nobody watches this process: the release of the GPU context, the pinned buffers and the mappings gets a bounded
    // time.  A teardown that hangs ends with SIGALRM's default action instead of holding the GPU for ever (every output is complete).
    signal(SIGALRM, SIG_DFL);
    alarm(120);
    const unsigned char b = (unsigned char)status;
    if (write(g_done_fd, &b, 1) != 1) {}
    ::close(g_done_fd);
    g_done_fd = -1;
    // a caller that reads our stdout / stderr through pipes waits for their last holder: let go of them, nothing more is said
    const int nul = open("/dev/null", O_WRONLY);
    if (nul >= 0) { dup2(nul, 1); dup2(nul, 2); if (nul > 2) ::close(nul); }
}
} // namespace
