"""Same kernels, same grids: python trace_compare.py OUT_DIR [SUBSTRING ...] (the traces of a
trace_ab.sh). Per trace: the sequence, in dispatch order, of (kernel name, grid, workgroup size,
LDS size) of every kernel whose name contains one of the substrings, as given or in lower case —
by default "gemm" or "Cijk_" (hipBLASLt's, and the Tensile GEMMs of the tests' torch references);
profiles/attn_host passes "attn" — tree against parent, line by line. Exit status 1 on any
difference."""
import csv
import glob
import os
import sys

out = sys.argv[1]
keys = sys.argv[2:] or ["gemm", "Cijk_"]
ok = True


def launches(d):
    seq = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        rows = list(csv.DictReader(open(path)))
        rows.sort(key=lambda r: int(r["Dispatch_Id"]))
        for r in rows:
            name = r["Kernel_Name"]
            if any(k in name or k in name.lower() for k in keys):
                seq.append((name,) + tuple(r[c] for c in (
                    "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X",
                    "Workgroup_Size_Y", "Workgroup_Size_Z", "LDS_Block_Size")))
    return seq


print("| trace | launches, tree | launches, parent | distinct lines | Cijk_ launches | verdict |")
print("|---|---|---|---|---|---|")
for d in sorted(glob.glob(os.path.join(out, "tree.*"))):
    if not os.path.isdir(d):
        continue
    name = os.path.basename(d)[len("tree."):]
    t, p = launches(d), launches(os.path.join(out, "parent." + name))
    same = t == p and len(t) > 0
    ok &= same
    if not same:
        for i, (a, b) in enumerate(zip(t, p)):
            if a != b:
                print(f"first difference at line {i}:\n  tree   {a}\n  parent {b}", file=sys.stderr)
                break
    blaslt = sum(1 for r in t if "Cijk_" in r[0])
    print(f"| {name} | {len(t)} | {len(p)} | {len(set(t))} | {blaslt} | "
          f"{'equal line by line' if same else 'DIFFERENT'} |")
print("\nall equal" if ok else "\nFAILED")
sys.exit(0 if ok else 1)
