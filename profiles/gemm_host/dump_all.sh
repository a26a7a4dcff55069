#!/bin/bash
# Every configuration of ../engine_prompts/configs.txt from this checkout: the tree's library once
# and the parent's library three times, one process per dump, each under its own time limit; the
# first failure stops the chain.
#   profiles/gemm_host/dump_all.sh PARENT_SO OUT_DIR
# Compare with python profiles/engine_prompts/compare.py OUT_DIR.
set -eu
tree=$(cd "$(dirname "$0")/../.." && pwd)
parent=$(readlink -f "$1")
out=$2
mkdir -p "$out"
for leg in tree p1 p2 p3; do
    export LCCLIP_LIB="$parent"
    [ "$leg" = tree ] && export LCCLIP_LIB="$tree/lifelong-clip_amd/lcclip/liblcclip.so"
    while IFS='|' read -r name envs args; do
        # shellcheck disable=SC2086
        env $envs timeout -k 10 120 python "$tree/tools/step_dump.py" "$out/$name.$leg" $args < /dev/null
    done < "$tree/profiles/engine_prompts/configs.txt"
done
