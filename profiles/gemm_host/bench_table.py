"""The raw lines of bench_ab.txt and the table of README.md from bench_ab.sh's logs:
python bench_table.py OUT_DIR. Rule: the tree's mean is accepted when it is no further above the
parent's mean than the parent's own max - min."""
import json
import os
import sys

out = sys.argv[1]


def ms(path):
    for line in reversed(open(path).read().splitlines()):
        if line.startswith("{") and "ms_per_step" in line:
            d = json.loads(line)
            return d["ms_per_step"], d.get("images_per_s", d.get("value"))
    raise SystemExit(f"no result line in {path}")


rows = []
for b in ("bench", "mvp", "maple_bf16", "maple_fp8"):
    v = {"tree": [], "parent": []}
    for i in (1, 2, 3):
        for leg in ("tree", "parent"):
            m, ips = ms(os.path.join(out, f"{b}.{leg}.{i}.log"))
            v[leg].append(m)
            print(f"{b} {leg} {i}: {m} ms, {ips} images/s")
    mt, mp = sum(v["tree"]) / 3, sum(v["parent"]) / 3
    span = max(v["parent"]) - min(v["parent"])
    rows.append(f"| {b} | {', '.join(map(str, v['tree']))} | {mt:.3f} | "
                f"{', '.join(map(str, v['parent']))} | {mp:.3f} | {span:.3f} | {mt - mp:+.3f} | "
                f"{'yes' if mt - mp <= span else 'NO'} |")
print("\n| benchmark | tree, ms per step | mean | parent, ms per step | mean | parent max - min | "
      "tree - parent | accepted |\n|---|---|---|---|---|---|---|---|")
print("\n".join(rows))
