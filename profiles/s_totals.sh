#!/bin/bash
# The fixed part of trim_lds's S step: the read's totals and the gate of the adjacent-N test (profiles/s_totals/).
#   bash profiles/s_totals.sh build
#       the diagnostic library (WRONG results, never the product) from the tree's sources, next to the objects of __graft_entry__.build():
#       profiles/microbench/libfaqcs_mi_s_nonblock.so  -DFAQCS_LDS_DIAG_S_NO_NBLOCK  the adjacent-N test is never entered
#   the A/B itself: bash profiles/lds_same_address.sh ab <reps> parent=<library of the parent commit> change=faqcs_amd/libfaqcs_mi.so nonblock=profiles/microbench/libfaqcs_mi_s_nonblock.so
set -e -o pipefail
cd "$(dirname "$0")/.."
cs=faqcs_amd/csrc
hip="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function"
case "$1" in
build)
    objs=""
    for s in $(python3 -c "import __graft_entry__ as g; print(' '.join(g.HIP_SOURCES))"); do
        case $s in faqcs_trim_lds_kernel.hip) ;; *) objs="$objs $cs/${s%.*}.o" ;; esac
    done
    mkdir -p profiles/microbench
    $hip -DFAQCS_LDS_DIAG_S_NO_NBLOCK -c $cs/faqcs_trim_lds_kernel.hip -o /tmp/faqcs_lds_s_nonblock.o
    $hip -shared -o profiles/microbench/libfaqcs_mi_s_nonblock.so $objs /tmp/faqcs_lds_s_nonblock.o
    ;;
*) echo "usage: $0 build"; exit 2 ;;
esac
