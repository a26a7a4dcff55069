"""The GEMM router's plan query (lc_gemm_split_plan), without a GPU.

lc_gemm_nt_rows stands in for a launch at M_full rows only where the router says that launch runs
gemm8_kernel's default schedule (or a kernel without any split), and it reads the split-K plan
from the same decision. The query needs no device: without one the router plans for 256 CUs, the
MI355X's count, which the cases of tests/test_gemm_rows_gpu.py are written for. A routing change
that moves a plan or drops a refusal fails here before it reaches the GPU tests.
"""
import ctypes

from test_gemm_rows_gpu import CASES

LC_EUNSUPPORTED = -3


def plan(lib, M, N, K, ws_bytes):
    dp, s = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.lc_gemm_split_plan(M, N, K, ws_bytes, ctypes.byref(dp), ctypes.byref(s))
    return rc, dp.value, s.value


def test_plans_of_the_rows_cases():
    from lcclip import ops
    for name, (n, mul, add, N, K, tiles, tail, S) in CASES.items():
        assert ops.gemm_split_plan(n * mul, N, K) == (tiles - tail, S), name


def test_knobs_refuse_and_reset():
    from lcclip import _lib, ops
    lib = _lib.load()
    n, mul, add, N, K, tiles, tail, S = CASES["c"]
    shape = (n * mul, N, K, ops.SPLITK_WS_BYTES)
    want = (0, tiles - tail, S)
    assert plan(lib, *shape) == want
    for setter, value in ((lib.lc_gemm_set_streamk, 1), (lib.lc_gemm_set_tile, 8)):
        assert setter(value) == 0
        try:
            assert plan(lib, *shape)[0] == LC_EUNSUPPORTED, setter.__name__
        finally:
            setter(0)
        assert plan(lib, *shape) == want, setter.__name__


def test_no_workspace_no_split():
    from lcclip import _lib
    lib = _lib.load()
    for name, (n, mul, add, N, K, tiles, tail, S) in CASES.items():
        assert plan(lib, n * mul, N, K, 0) == (0, tiles, 1), name
