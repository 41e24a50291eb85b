#!/bin/bash
# GPU-box recipe: A/B of the headline between the product library and
# baseline libraries under abl/ (ATGPU_LIB), alternating plain bench.py runs.
#   tools/gpu_lib_ab.sh <tag> <rounds> <name>...   name: product | abl/libatgpu_<name>.so
# then, per library, in runs of their own: the search kernel alone under a
# kernel trace (bench.py --k2-profile), the live step under a kernel trace,
# and a counter pass (SQ_INSTS_VALU, SQ_WAVES) -- never combined.
# STEPS (default 30) sets the steps of a plain run, PROFILE (default: every
# name) the libraries that get the profiling passes, NO_PROFILE=1 none,
# OUT_DIR (default ab_out/ in the tree) where the results go.
# Build the baselines before the call, e.g. the parent commit's library as
# abl/libatgpu_old.so, or one with a single object file swapped.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT_DIR:-$R/ab_out}/${1:-libab}
ROUNDS=${2:-3}
shift 2
NAMES=${*:-"old product"}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
lib() { [ "$1" = product ] && echo "" || echo "$R/abl/libatgpu_$1.so"; }
die() { echo "$1 failed (rc $2)"; exit 1; }
for r in $(seq 1 "$ROUNDS"); do
    for n in $NAMES; do
        L=$(lib "$n")
        line=$(env ${L:+ATGPU_LIB=$L} timeout -k 10 240 python3 "$R/bench.py" --gpus 1 --steps "${STEPS:-30}" --warmup 2 \
               2>>"$OUT/err.log" | tail -n 1) || die "bench $n" $?
        echo "{\"lib\": \"$n\", \"round\": $r, \"result\": $line}" | tee -a "$OUT/pairs.jsonl" | cut -c 1-200
    done
done
[ -n "$NO_PROFILE" ] && exit 0
cd "$OUT"
for n in ${PROFILE:-$NAMES}; do
    L=$(lib "$n")
    env ${L:+ATGPU_LIB=$L} timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/k2_$n" -o run \
        --output-format csv -- python3 "$R/bench.py" --k2-profile --steps 20 > "$OUT/k2_$n.log" 2>&1 || die "k2 trace $n" $?
    python3 "$R/tools/prof_summary.py" "$(find "$OUT/k2_$n" -name '*kernel_stats.csv' | head -n 1)" "$OUT/k2_alone_$n.txt" | grep search
    env ${L:+ATGPU_LIB=$L} timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/live_$n" -o run \
        --output-format csv -- python3 "$R/bench.py" --gpus 1 --steps 20 --warmup 2 > "$OUT/live_$n.log" 2>&1 || die "live trace $n" $?
    python3 "$R/tools/prof_summary.py" "$(find "$OUT/live_$n" -name '*kernel_stats.csv' | head -n 1)" "$OUT/live_$n.txt" | grep -E "search|pack|md5|lpc"
    env ${L:+ATGPU_LIB=$L} timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES -d "$OUT/pmc_$n/sq" -o run \
        --output-format csv -- python3 "$R/bench.py" --gpus 1 --steps 2 --warmup 1 > "$OUT/pmc_$n.log" 2>&1 || die "pmc $n" $?
    python3 "$R/tools/pmc_summary.py" "$OUT/pmc_$n" > "$OUT/pmc_$n.json"
done
