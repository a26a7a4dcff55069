#!/bin/bash
# Every configuration of configs.txt: the tree once and the parent checkout three times, one
# process per dump, each under its own time limit; the first failure stops the chain.
#   profiles/engine_prompts/dump_all.sh PARENT_CHECKOUT OUT_DIR
# Both legs load the tree's liblcclip.so (LCCLIP_LIB). Compare with compare.py OUT_DIR.
set -eu
here=$(cd "$(dirname "$0")" && pwd)
tree=$(cd "$here/../.." && pwd)
parent=$(cd "$1" && pwd)
out=$2
mkdir -p "$out"
export LCCLIP_LIB="$tree/lifelong-clip_amd/lcclip/liblcclip.so"
for leg in tree p1 p2 p3; do
    root=$parent
    [ "$leg" = tree ] && root=$tree
    while IFS='|' read -r name envs args; do
        # shellcheck disable=SC2086
        env $envs timeout -k 10 120 python "$root/tools/step_dump.py" "$out/$name.$leg" $args < /dev/null
    done < "$here/configs.txt"
done
