#!/usr/bin/env python3
"""lc_gemm_split_plan over a sweep of shapes, workspaces and knobs, one line per cell.

usage: [LCCLIP_LIB=<other build>] tools/gemm_plan_sweep.py > cells.txt

Needs no GPU (the router plans for 256 CUs without a device). Run it once per library, each in
its own process, and diff the outputs: a host-side change of the GEMM router must leave every
cell's (return code, dp_tiles, splits) as it was. The last line counts the cells and those with
a split (S > 1).
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lifelong-clip_amd"))
from lcclip import _lib, ops  # noqa: E402

MS = (64, 770, 4095, 4096, 4293, 7700, 12763, 12800, 25216, 25600, 27776, 28160, 32768, 50395,
      50432, 65792, 75676)
NS = (64, 192, 256, 512, 768, 2304, 3072)
KS = (64, 128, 768, 1024, 2048, 2304, 3072)
KNOBS = ((0, 0), (1, 0), (0, 8))  # (stream-K mode, forced tile)


def main():
    lib = _lib.load()
    cells = split = 0
    for sk, tile in KNOBS:
        assert lib.lc_gemm_set_streamk(sk) == 0 and lib.lc_gemm_set_tile(tile) == 0
        for ws in (0, ops.SPLITK_WS_BYTES):
            for M in MS:
                for N in NS:
                    for K in KS:
                        dp, s = ctypes.c_int(-1), ctypes.c_int(-1)
                        rc = lib.lc_gemm_split_plan(M, N, K, ws, ctypes.byref(dp), ctypes.byref(s))
                        print(sk, tile, ws, M, N, K, rc, dp.value, s.value)
                        cells += 1
                        split += rc == 0 and s.value > 1
    lib.lc_gemm_set_streamk(0)
    lib.lc_gemm_set_tile(0)
    print(f"# {cells} cells, {split} with a split")


if __name__ == "__main__":
    main()
