#!/bin/bash
# Three interleaved pairs (tree, then the parent checkout) of the default bench line and of the
# MVP and MaPLe step benchmarks, one process each under its own time limit; the first failure
# stops the chain. Both legs load the tree's liblcclip.so.
#   profiles/engine_prompts/bench_ab.sh PARENT_CHECKOUT OUT_DIR
set -eu
tree=$(cd "$(dirname "$0")/../.." && pwd)
parent=$(cd "$1" && pwd)
out=$2
mkdir -p "$out"
export LCCLIP_LIB="$tree/lifelong-clip_amd/lcclip/liblcclip.so"
for i in 1 2 3; do
    for leg in tree parent; do
        root=$parent
        [ "$leg" = tree ] && root=$tree
        cd "$root"
        timeout -k 10 300 python -u bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline \
            > "$out/bench.$leg.$i.log" 2>&1 < /dev/null
        timeout -k 10 300 python -u tools/bench_mvp.py > "$out/mvp.$leg.$i.log" 2>&1 < /dev/null
        timeout -k 10 300 python -u tools/bench_maple.py > "$out/maple.$leg.$i.log" 2>&1 < /dev/null
        cd "$tree"
    done
done
