"""The table of README.md from the dumps of dump_all.sh: python compare.py OUT_DIR.
Per configuration: the tree's trace against each of the parent's three (bytes), every saved
tensor against the parent's (bits where the parent's three runs agree, else the tree's distance
from the nearest parent run against the parent's own spread) and max_memory_allocated."""
import os
import sys

import numpy as np

out = sys.argv[1]
here = os.path.dirname(os.path.abspath(__file__))
ok = True
print("| configuration | calls | trace, tree vs 3 × parent | tensors | bit-identical over the "
      "parent runs | tree bit-identical to parent | not reproducible: parent spread / tree "
      "difference | max_memory_allocated, parent / tree |")
print("|---|---|---|---|---|---|---|---|")
for line in open(os.path.join(here, "configs.txt")):
    name = line.split("|")[0]
    legs = ("tree", "p1", "p2", "p3")
    tr = {leg: open(f"{out}/{name}.{leg}.trace.txt", "rb").read() for leg in legs}
    same = all(tr["tree"] == tr[p] for p in ("p1", "p2", "p3"))
    z = {leg: np.load(f"{out}/{name}.{leg}.npz") for leg in tr}
    keys = [k for k in z["p1"].files if k != "max_mem"]
    assert set(z["tree"].files) == set(z["p1"].files)
    stable = exact = 0
    loose = []
    for k in keys:
        ps = [z[p][k] for p in ("p1", "p2", "p3")]
        t = z["tree"][k]
        if all(np.array_equal(ps[0].view(np.uint32), p.view(np.uint32)) for p in ps[1:]):
            stable += 1
            if np.array_equal(t.view(np.uint32), ps[0].view(np.uint32)):
                exact += 1
            else:
                ok = False
                loose.append(f"{k}: DIFFERS by {np.abs(t - ps[0]).max():.3g}")
        else:
            spread = max(np.abs(a - b).max() for a in ps for b in ps)
            diff = min(np.abs(t - p).max() for p in ps)
            ok &= bool(diff <= 2 * spread)
            loose.append(f"{k}: {spread:.3g} / {diff:.3g}")
    mp = sorted({int(z[p]["max_mem"]) for p in ("p1", "p2", "p3")})
    mt = int(z["tree"]["max_mem"])
    ok &= same and mt <= max(mp)
    calls = tr["tree"].count(b"\n")
    print(f"| {name} | {calls} | {'identical' if same else 'DIFFERENT'} | "
          f"{len(keys)} | {stable} | {exact} | {'; '.join(loose) or '—'} | "
          f"{' '.join(map(str, mp))} / {mt} |")
print("\nall requirements met" if ok else "\nFAILED")
sys.exit(0 if ok else 1)
