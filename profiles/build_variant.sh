#!/bin/bash
# Diagnostic builds of the library with trim_lds compiled under extra -D switches (results are WRONG with the FAQCS_LDS_NO_*
# switches: they exist to attribute LDS time): bash profiles/build_variant.sh <name> -DFOO [-DBAR ...]  -> profiles/microbench/libfaqcs_mi_<name>.so
# faqcs_capi.hip is compiled under the same switches: it asks trim_plan() (faqcs_trim_plan.h), whose shapes and chunk capacity follow
# -DFAQCS_LDS16_RPC, -DFAQCS_LDS16_NW and -DFAQCS_LDS_TEST_FLUSH_CHUNKS.  The other objects: those of __graft_entry__.build() (HIP_SOURCES).
set -e
cd "$(dirname "$0")/.."
name=$1; shift
cs=faqcs_amd/csrc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function "$@" -c $cs/faqcs_trim_lds_kernel.hip -o /tmp/faqcs_lds_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function "$@" -c $cs/faqcs_capi.hip -o /tmp/faqcs_capi_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o profiles/microbench/libfaqcs_mi_$name.so /tmp/faqcs_capi_$name.o $cs/faqcs_capi_kmer.o $cs/faqcs_capi_seam.o $cs/faqcs_capi_comm.o $cs/faqcs_host.o $cs/faqcs_trim_kernel.o $cs/faqcs_trim_long_kernel.o $cs/faqcs_adapter_kernel.o $cs/faqcs_kmer_kernel.o $cs/faqcs_kmer_skm_kernel.o $cs/faqcs_synth_kernel.o $cs/faqcs_emit_kernel.o $cs/faqcs_parse_kernel.o $cs/faqcs_render_kernel.o $cs/faqcs_inflate_kernel.o $cs/faqcs_deflate_kernel.o /tmp/faqcs_lds_$name.o
