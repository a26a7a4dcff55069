#!/bin/bash
# Three interleaved pairs (the tree's library, then the parent's, same checkout) of the default
# bench line, the MVP step benchmark and the MaPLe one over 100 timed steps per precision, one
# process each under its own time limit; the first failure stops the chain.
#   profiles/gemm_host/bench_ab.sh PARENT_SO OUT_DIR
set -eu
tree=$(cd "$(dirname "$0")/../.." && pwd)
parent=$(readlink -f "$1")
out=$2
mkdir -p "$out"
cd "$tree"
for i in 1 2 3; do
    for leg in tree parent; do
        export LCCLIP_LIB="$tree/lifelong-clip_amd/lcclip/liblcclip.so"
        [ "$leg" = parent ] && export LCCLIP_LIB="$parent"
        timeout -k 10 300 python -u bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline \
            > "$out/bench.$leg.$i.log" 2>&1 < /dev/null
        timeout -k 10 300 python -u tools/bench_mvp.py > "$out/mvp.$leg.$i.log" 2>&1 < /dev/null
        for prec in bf16 fp8; do
            PREC=$prec STEPS=100 WARM=10 timeout -k 10 300 python -u tools/bench_maple.py \
                > "$out/maple_$prec.$leg.$i.log" 2>&1 < /dev/null
        done
    done
done
