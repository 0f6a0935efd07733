// faqcs_host.h -- what faqcs_host.cpp (plain host C++, no HIP) shares with the device side of the library (faqcs_ctx.h): the one error
// sink behind faqcs_last_error() and the argument checks that a host statement and its device entry point both make.  Internal: nothing
// declared here is exported.
#pragma once
#include <string>

#include "../../include/faqcs_mi.h"

#define FAQCS_HIDDEN __attribute__((visibility("hidden")))

// stores the calling thread's message (faqcs_last_error) and returns `code`
FAQCS_HIDDEN int fail(int code, const std::string &msg);

// `who` names the entry point in the message
FAQCS_HIDDEN int parse_check_args(const char *who, const uint8_t *text, uint64_t n_text, const faqcs_parse_out *out);
FAQCS_HIDDEN int render_check_args(const char *who, const faqcs_batch *b, const uint8_t *text, const uint32_t *def_pos, const uint32_t *def_len, const faqcs_render_out *out);
FAQCS_HIDDEN int bgzf_index_check_args(const char *who, const uint8_t *comp, uint64_t n_comp, const uint32_t *member_offset, const faqcs_bgzf_index_info *info);
FAQCS_HIDDEN int inflate_check_args(const char *who, const uint8_t *comp, uint64_t n_comp, const uint32_t *member_offset, uint32_t n_members, const faqcs_inflate_out *out);
FAQCS_HIDDEN int gunzip_check_args(const char *who, const uint8_t *comp, uint64_t n_comp, uint32_t piece_bytes, const faqcs_gunzip_out *out);
FAQCS_HIDDEN int gunzip_state_check_args(const char *who, const faqcs_gunzip_state *state);
namespace faqcs_gunzip { struct Info; struct State; }
FAQCS_HIDDEN void gunzip_info_out(const faqcs_gunzip::Info &i, faqcs_gunzip_info *o);
// the carried state without its window, in and out
FAQCS_HIDDEN void gunzip_state_in(const faqcs_gunzip_state *s, faqcs_gunzip::State *o);
FAQCS_HIDDEN void gunzip_state_out(const faqcs_gunzip::State &s, faqcs_gunzip_state *o);
FAQCS_HIDDEN int deflate_check_args(const char *who, const uint8_t *text, uint64_t n_text, uint32_t member_bytes, int final, int mode, const faqcs_deflate_out *out);
FAQCS_HIDDEN int pair_check_args(const char *who, const faqcs_mate *m1, const faqcs_mate *m2, const uint8_t *route, const faqcs_pair_info *info, uint32_t *n);
FAQCS_HIDDEN int render_pair_check_args(const char *who, int file, const faqcs_mate *m1, const faqcs_mate *m2, const uint8_t *route, uint32_t n_pairs, const faqcs_render_out *out);
FAQCS_HIDDEN int detect_check_args(const char *who, const faqcs_batch *b, uint32_t first, uint32_t count, const uint8_t *text, const uint32_t *def_pos, const uint32_t *def_len, const faqcs_detect_info *info);
FAQCS_HIDDEN int first_error_check_args(const char *who, const faqcs_read_result *results, uint32_t n, const faqcs_error_info *info);
