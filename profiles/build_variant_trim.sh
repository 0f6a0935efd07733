#!/bin/bash
# Like build_variant.sh, for faqcs_trim_kernel.hip: bash profiles/build_variant_trim.sh <name> -DFOO ...  -> profiles/microbench/libfaqcs_mi_<name>.so
# (faqcs_capi.hip under the same switches: trim_plan()'s grid of trim_filter_accumulate follows -DFAQCS_TRIM_NW and -DFAQCS_TRIM_MINWAVES)
set -e
cd "$(dirname "$0")/.."
name=$1; shift
cs=faqcs_amd/csrc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function "$@" -c $cs/faqcs_trim_kernel.hip -o /tmp/faqcs_trimk_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function "$@" -c $cs/faqcs_capi.hip -o /tmp/faqcs_capi_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o profiles/microbench/libfaqcs_mi_$name.so /tmp/faqcs_capi_$name.o /tmp/faqcs_trimk_$name.o $cs/faqcs_capi_kmer.o $cs/faqcs_capi_seam.o $cs/faqcs_capi_comm.o $cs/faqcs_host.o $cs/faqcs_trim_lds_kernel.o $cs/faqcs_trim_long_kernel.o $cs/faqcs_adapter_kernel.o $cs/faqcs_kmer_kernel.o $cs/faqcs_kmer_skm_kernel.o $cs/faqcs_synth_kernel.o $cs/faqcs_emit_kernel.o $cs/faqcs_parse_kernel.o $cs/faqcs_render_kernel.o $cs/faqcs_inflate_kernel.o $cs/faqcs_deflate_kernel.o
