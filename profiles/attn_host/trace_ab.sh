#!/bin/bash
# Kernel traces (rocprofv3 --kernel-trace, nothing else traced) of the attention tests and of three
# steps of each step benchmark, once with the tree's library and once with the parent's, one
# process per trace under its own time limit; the first failure stops the chain.
#   profiles/attn_host/trace_ab.sh PARENT_SO OUT_DIR [tests|bench]
# Compare with python profiles/gemm_host/trace_compare.py OUT_DIR attn.
# Together the test files launch every chunk count 1..8 under every backward form in both storage
# types, plus the row, live-row and fp8 modes.
set -eu
tree=$(cd "$(dirname "$0")/../.." && pwd)
parent=$(readlink -f "$1")
out=$2
what=${3:-all}
mkdir -p "$out"
cd "$tree"
trace() {  # name limit command...
    local name=$1 limit=$2
    shift 2
    timeout -k 10 "$limit" rocprofv3 --kernel-trace --output-format csv -d "$out/$leg.$name" \
        -o run -- "$@" > "$out/$leg.$name.log" 2>&1 < /dev/null
}
for leg in tree parent; do
    export LCCLIP_LIB="$tree/lifelong-clip_amd/lcclip/liblcclip.so"
    [ "$leg" = parent ] && export LCCLIP_LIB="$parent"
    if [ "$what" != bench ]; then
        trace attention 300 python -m pytest -q -p no:cacheprovider tests/test_attention_gpu.py
        # (-k applies to every file of a pytest run: the kernel tests get a run of their own)
        trace kernels 300 python -m pytest -q -p no:cacheprovider tests/test_kernels_gpu.py \
            -k attention
        trace rows 300 python -m pytest -q -p no:cacheprovider tests/test_attention_row_gpu.py \
            tests/test_attention_row_exact_gpu.py tests/test_fp8_gpu.py tests/test_f16_gpu.py
    fi
    if [ "$what" != tests ]; then
        trace bench 300 python bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline
        STEPS=3 WARM=1 trace mvp 300 python tools/bench_mvp.py
        for prec in bf16 fp8; do
            PREC=$prec STEPS=3 WARM=1 trace maple_$prec 300 python tools/bench_maple.py
        done
    fi
done
