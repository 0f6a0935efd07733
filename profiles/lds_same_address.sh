#!/bin/bash
# The LDS adds of trim_lds and of the composition fold that land on one address (profiles/lds_same_address/).
#   bash profiles/lds_same_address.sh build
#       the two diagnostic libraries (WRONG results, never the product) from the tree's sources, next to the objects of __graft_entry__.build():
#       profiles/microbench/libfaqcs_mi_epi_nc.so   -DFAQCS_LDS_DIAG_EPI_NOCONFLICT  the six epilogue adds of a chunk on cells of their own
#       profiles/microbench/libfaqcs_mi_fold_nc.so  -DFAQCS_DIAG_FOLD_NOCONFLICT     the fold's adds on one dword per lane (both fold kernels)
#   bash profiles/lds_same_address.sh ab <reps> <name>=<library> [<name>=<library> ...] [-- <bench.py arguments>]
#       the plain bench, the libraries alternating (FAQCS_MI_LIB), <reps> runs each; a line per run, then min / median / max per library
set -e -o pipefail
cd "$(dirname "$0")/.."
cs=faqcs_amd/csrc
hip="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function"
case "$1" in
build)
    objs=""
    for s in $(python3 -c "import __graft_entry__ as g; print(' '.join(g.HIP_SOURCES))"); do
        case $s in faqcs_trim_lds_kernel.hip|faqcs_trim_kernel.hip) ;; *) objs="$objs $cs/${s%.*}.o" ;; esac
    done
    $hip -DFAQCS_LDS_DIAG_EPI_NOCONFLICT -c $cs/faqcs_trim_lds_kernel.hip -o /tmp/faqcs_lds_epi_nc.o &
    $hip -DFAQCS_DIAG_FOLD_NOCONFLICT -c $cs/faqcs_trim_lds_kernel.hip -o /tmp/faqcs_lds_fold_nc.o &
    $hip -DFAQCS_DIAG_FOLD_NOCONFLICT -c $cs/faqcs_trim_kernel.hip -o /tmp/faqcs_trimk_fold_nc.o &
    wait
    $hip -shared -o profiles/microbench/libfaqcs_mi_epi_nc.so $objs $cs/faqcs_trim_kernel.o /tmp/faqcs_lds_epi_nc.o
    $hip -shared -o profiles/microbench/libfaqcs_mi_fold_nc.so $objs /tmp/faqcs_trimk_fold_nc.o /tmp/faqcs_lds_fold_nc.o
    ;;
ab)
    reps=$2; shift 2
    libs=(); extra=()
    while [ $# -gt 0 ]; do
        if [ "$1" = "--" ]; then shift; extra=("$@"); break; fi
        libs+=("$1"); shift
    done
    tmp=$(mktemp)
    for r in $(seq "$reps"); do
        for nl in "${libs[@]}"; do
            name=${nl%%=*}; lib=${nl#*=}
            # (a run that fails -- a fault, an abort, its time limit -- ends the script: nothing more is started on that GPU; its stderr stays visible)
            log=$(mktemp)
            FAQCS_MI_LIB=$(readlink -f "$lib") timeout -k 10 240 python3 bench.py --no-cpu-baseline --e2e-pairs 0 "${extra[@]}" > "$log" || {
                rc=$?; echo "$name run $r: bench.py ended with status $rc -- stopping" >&2; tail -5 "$log" >&2; rm -f "$log" "$tmp"; exit $rc; }
            tail -1 "$log" |
                python3 -c "import sys,json; d=json.loads(sys.stdin.read()); r=d['roofline']; print('$name run $r ms_per_step', d['ms_per_step'], 'value', d['value'], 'kernel_ms', r['kernel_ms'], 'ratio', round(7*r['kernel_ms']/d['ms_per_step'],4), 'frac', r['frac'])" | tee -a "$tmp"
            rm -f "$log"
        done
    done
    python3 - "$tmp" <<'PY'
import statistics, sys
runs = {}
for ln in open(sys.argv[1]):
    w = ln.split()
    runs.setdefault(w[0], []).append((float(w[4]), float(w[8])))
for name, v in runs.items():
    ms, k = [a for a, _ in v], [b for _, b in v]
    print(name, "ms_per_step min/med/max", min(ms), statistics.median(ms), max(ms), "kernel_ms min/med/max", min(k), statistics.median(k), max(k),
          "kernel_ms x launches / ms_per_step (median)", round(statistics.median(k) * 7 / statistics.median(ms), 4), "n", len(ms))
PY
    rm -f "$tmp"
    ;;
*) echo "usage: $0 build | ab <reps> <name>=<library> ... [-- <bench.py arguments>]"; exit 2 ;;
esac
