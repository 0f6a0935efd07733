// trim_plan_check -- prints trim_plan() (faqcs_amd/csrc/faqcs_trim_plan.h) for every line of its standard input.  Host C++ only; built by
// tests/test_trim_plan.py under AddressSanitizer and UBSan, never linked into the product.
//   a line:  mode protect5 qc_only replace_q avgq_on max_poly_n dbg has_adapters trim5 trim3 fold_n   max_len n_reads n_cu
//            force_long lds_on lds4_on lds16_on                                                     (18 unsigned numbers)
//   answer:  kernel C LPR NW RPC windowed ext wide_records folds_tail grid records_needed
// "constants" as the only argument: the constants of the header that the test restates, one "name value" per line.
#include <cstdio>
#include <cstring>

#include "../faqcs_amd/csrc/faqcs_trim_plan.h"

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "constants")) {
        printf("FAQCS_FAST_READ_LENGTH %d\nFAQCS_PARTIAL_FLUSHES %d\nFAQCS_TRIM_NW %d\nFAQCS_TRIM_LONG_NW %d\nFAQCS_LDS16_RPC %d\n", (int)FAQCS_FAST_READ_LENGTH,
               (int)FAQCS_PARTIAL_FLUSHES, (int)FAQCS_TRIM_NW, (int)FAQCS_TRIM_LONG_NW, (int)FAQCS_LDS16_RPC);
        return 0;
    }
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        unsigned v[18];
        int got = 0, used = 0;
        for (const char *p = line; got < 18 && sscanf(p, "%u%n", &v[got], &used) == 1; p += used) ++got;
        if (got != 18) { fprintf(stderr, "trim_plan_check: a line needs 18 numbers, this one has %d: %s", got, line); return 2; }
        const TrimOptions o{(int32_t)v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]};
        const TrimSwitches sw{v[14] != 0, v[15] != 0, v[16] != 0, v[17] != 0};
        const TrimPlan p = trim_plan(o, v[11], v[12], (int)v[13], sw);
        printf("%s %d %d %d %d %d %d %d %d %u %zu\n", trim_kernel_name(p.kernel), p.C, p.LPR, p.NW, p.RPC, (int)p.windowed, (int)p.ext, (int)p.wide_records,
               (int)p.folds_tail, p.grid, p.records_needed);
    }
    return 0;
}
