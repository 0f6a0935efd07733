// cli_common.h -- what every part of the command line uses: the system headers, the constants, Fatal, the time marks.
// The headers of this directory are parts of ONE translation unit, faqcs_cli.cpp, which includes them in order; they live here and not
// in csrc/ because csrc/*.h are sources of the GPU library (its build's dependencies, and tools/source_hash.py's identity of the kernels).
#pragma once
#include <zlib.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
#include <immintrin.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <atomic>
#include <memory>
#include <thread>
#include <vector>

#include "../../../include/faqcs_mi.h"
#include "../faqcs_pargz.h"

namespace {
const char *VERSION = "2.10";
constexpr uint32_t BUF_READS = FAQCS_SEGMENT_READS;
const int AUTO_OFFSET = -128;

struct Fatal : std::runtime_error { using std::runtime_error::runtime_error; };

// FAQCS_MI_TIMING=1: wall-clock marks of the run's stages on stderr (diagnostics; a path that has no mark for a stage passes nullptr)
double now_s() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
const double T0 = now_s();
void tmark(const char *what) { static const bool on = getenv("FAQCS_MI_TIMING") != nullptr; if (on && what) fprintf(stderr, "[faqcs_mi %8.3f s] %s\n", now_s() - T0, what); }
} // namespace
