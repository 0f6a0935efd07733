#!/bin/bash
# trim_lds: the adjacent-N test behind the S loop (profiles/n_deferred/).  Every GPU step runs under a time limit of its own and
# the first one that fails ends the script; nothing is tried twice.
#   bash profiles/n_deferred.sh build
#       the diagnostic library (WRONG results, never the product) from the tree's sources, next to the objects of __graft_entry__.build():
#       profiles/microbench/libfaqcs_mi_s_nonblock.so  -DFAQCS_LDS_DIAG_S_NO_NBLOCK  no step is ever flagged: the pass behind the loop never runs
#       (built from the PARENT's sources the same macro gives the ceiling of this change: the test never entered inside the loop)
#   bash profiles/n_deferred.sh ab <out dir> parent=<library of the parent commit> change=<library> [ceiling=<parent's diagnostic library>]
#       the plain bench, parent and change alternating, six runs each; then the ceiling, three runs              -> ab_plain.txt, ab_ceiling.txt
#   bash profiles/n_deferred.sh shapes <out dir> parent=<library> change=<library>
#       2x100 and 2x250 with the parent's library twice (the noise floor), the adapter config; three runs each  -> ab_2x100_noise.txt, ab_2x250_noise.txt, ab_adapter.txt
#   bash profiles/n_deferred.sh outputs <out dir> <parent's library> <library>
#       bench.py --dump-outputs of both, plain and adapter, compared byte for byte                                -> outputs_byte_equal.txt
#   bash profiles/n_deferred.sh mix <out dir> <name> <library>
#       rocprofv3 --pmc (a run of its own) over profiles/microbench/trim_ab: instructions and wave cycles per read -> pmc_instruction_mix_<name>.txt
#   bash profiles/n_deferred.sh stats <out dir> <name> <library>
#       rocprofv3 --kernel-trace --stats of the plain bench                                                       -> rocprofv3_kernel_stats_plain_<name>.csv
# (build also makes profiles/microbench/trim_ab, the harness of mix and of pmc_traffic2.sh)
set -e -o pipefail
cd "$(dirname "$0")/.."
cs=faqcs_amd/csrc
hip="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function"
ab="bash profiles/lds_same_address.sh ab"
case "$1" in
build)
    objs=""
    for s in $(python3 -c "import __graft_entry__ as g; print(' '.join(g.HIP_SOURCES))"); do
        case $s in faqcs_trim_lds_kernel.hip) ;; *) objs="$objs $cs/${s%.*}.o" ;; esac
    done
    mkdir -p profiles/microbench
    $hip -DFAQCS_LDS_DIAG_S_NO_NBLOCK -c $cs/faqcs_trim_lds_kernel.hip -o /tmp/faqcs_lds_s_nonblock.o
    $hip -shared -o profiles/microbench/libfaqcs_mi_s_nonblock.so $objs /tmp/faqcs_lds_s_nonblock.o
    g++ -O2 -std=c++17 -o profiles/microbench/trim_ab profiles/microbench/trim_ab.cpp -Iinclude -ldl -L/opt/rocm/lib -lamdhip64 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
    ;;
ab)
    out=$2; shift 2; mkdir -p "$out"
    pair=(); ceiling=""
    for nl in "$@"; do case $nl in ceiling=*) ceiling=$nl ;; *) pair+=("$nl") ;; esac; done
    $ab 6 "${pair[@]}" -- --gpus 1 --steps 20 --warmup 5 | tee "$out/ab_plain.txt"
    if [ -n "$ceiling" ]; then $ab 3 "$ceiling" -- --gpus 1 --steps 20 --warmup 5 | tee "$out/ab_ceiling.txt"; fi
    ;;
shapes)
    out=$2; parent=${3#parent=}; change=${4#change=}; mkdir -p "$out"
    $ab 3 parent="$parent" change="$change" parent_again="$parent" -- --gpus 1 --steps 20 --warmup 5 --read-len 100 | tee "$out/ab_2x100_noise.txt"
    $ab 3 parent="$parent" change="$change" parent_again="$parent" -- --gpus 1 --steps 20 --warmup 5 --read-len 250 | tee "$out/ab_2x250_noise.txt"
    $ab 3 parent="$parent" change="$change" -- --gpus 1 --steps 20 --warmup 5 --config adapter | tee "$out/ab_adapter.txt"
    ;;
outputs)
    out=$2; mkdir -p "$out"; tmp=$(mktemp -d)
    for cfg in plain adapter; do
        i=0
        for lib in "$3" "$4"; do
            i=$((i + 1))
            FAQCS_MI_LIB=$(readlink -f "$lib") timeout -k 10 240 python3 bench.py --gpus 1 --steps 2 --warmup 1 --config $cfg --dump-outputs "$tmp/${cfg}_$i" > /dev/null
        done
        for f in "$tmp/${cfg}_1"/*.npy; do
            b=$(basename "$f")
            if cmp -s "$f" "$tmp/${cfg}_2/$b"; then echo "dump_$cfg $b $(stat -c %s "$f") byte-equal"; else echo "dump_$cfg $b DIFFERS"; fi
        done
    done | tee "$out/outputs_byte_equal.txt"
    rm -rf "$tmp"
    if grep -q DIFFERS "$out/outputs_byte_equal.txt"; then exit 1; fi
    ;;
mix)
    out=$2; name=$3; lib=$4; n=16777216; mkdir -p "$out"; tmp=$(mktemp -d)
    TRIM_AB_REPS=2 timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d "$tmp" -o pmc -- \
        ./profiles/microbench/trim_ab $n 150 1 "$lib" < /dev/null > "$tmp/log" 2>&1
    python3 - "$tmp" "$n" <<'PY' | tee "$out/pmc_instruction_mix_$name.txt"
import collections, csv, glob, sys
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        acc[r["Kernel_Name"].split("(")[0]][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, c in acc.items():
    if "trim_lds" not in k and "fold" not in k:
        continue
    print(k, "launches", max(len(v) for v in c.values()))
    for name in sorted(c):
        print("   %-24s %12.3f per read" % (name, sum(c[name]) / len(c[name]) / float(sys.argv[2])))
PY
    rm -rf "$tmp"
    ;;
stats)
    out=$2; name=$3; lib=$4; mkdir -p "$out"; tmp=$(mktemp -d)
    FAQCS_MI_LIB=$(readlink -f "$lib") timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$tmp" -o plain -- \
        python3 bench.py --gpus 1 --steps 20 --warmup 5 > "$tmp/log" 2>&1
    cp "$(find "$tmp" -name '*kernel_stats.csv' | head -1)" "$out/rocprofv3_kernel_stats_plain_$name.csv"
    head -4 "$out/rocprofv3_kernel_stats_plain_$name.csv"
    rm -rf "$tmp"
    ;;
*) echo "usage: $0 build | ab | shapes | outputs | mix | stats  (see the head of the script)"; exit 2 ;;
esac
