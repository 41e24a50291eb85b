#!/bin/bash
# GPU-box recipe: ALAC decoder change check.  The ALAC and chain GPU suites,
# then two chain-only bench runs (the headline leg runs 10 steps first).
set -e -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT="$R/gpurun_out/${1:-alac}"
mkdir -p "$OUT"
cd "$R"
timeout -k 10 600 python -u -m pytest -x -q --timeout 120 --timeout-method thread -m gpu \
    tests/test_gpu_alac.py tests/test_gpu_chain.py tests/test_gpu_callers.py > "$OUT/pytest.log" 2>&1
for k in 1 2; do
    timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-host \
        --no-t2t --no-rg4 --narrow= --no-decode > "$OUT/chain$k.log" 2>&1
done
