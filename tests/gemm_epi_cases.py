"""Cells, inputs and float64 references of the GEMM epilogue matrix
(tests/test_gemm_epilogue_matrix_gpu.py), and the helpers its assertions use. Nothing here needs
a GPU: tests/test_gemm_epilogue_ref.py checks the helpers, the cell table against gemm.hip, and
the range of the generated inputs on the CPU.

The inputs make the value entering the epilogue exact. A holds {-1, 0, 1}, B holds {-1, 0, 1} / 8,
so every product is a multiple of 1/8 and every partial sum of at most 192 of them is exact in
f32 whatever the order; alpha is 1/2 or 1 and the bias a multiple of 1/4, so pre = alpha * acc +
bias is a multiple of 1/16 known exactly. All of it is exact in bf16 and in IEEE half, so one set
of inputs serves both storage types.
"""
import functools
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_HIP = os.path.join(ROOT, "lifelong-clip_amd", "csrc", "gemm.hip")

BF = torch.bfloat16
HF = torch.float16
F32 = torch.float32

# the public epilogues (lc_gemm_nt_ws takes these and no others) and their numbers
EPI = {"BF16": 0, "F32": 1, "RESID": 2, "GELU": 3, "GELU_BWD": 4, "BF16_F32": 5, "GELU_D": 6,
       "MUL": 7, "RESID16": 14}

# The public epilogues each kernel family is instantiated for, written out here on purpose:
# test_gemm_epilogue_ref.py compares this with the `using ...Epis = EpiList<...>` lines of gemm.hip.
FAMILY_EPIS = {
    "NtEpis": ("BF16", "F32", "RESID", "RESID16", "GELU", "GELU_BWD", "BF16_F32", "GELU_D", "MUL"),
    "PpEpis": ("BF16", "F32", "RESID", "GELU", "GELU_BWD", "BF16_F32", "GELU_D", "MUL"),
    "G8Epis": ("BF16", "F32", "RESID", "RESID16", "GELU", "GELU_D", "MUL"),
    "W4Epis": ("BF16", "F32", "RESID", "GELU_D", "MUL"),
}
# forced tile (the lc_gemm_set_tile numbering) -> the family that runs it
TILE_FAMILY = {1: "NtEpis", 2: "NtEpis", 3: "NtEpis", 4: "NtEpis", 11: "NtEpis", 5: "PpEpis",
               7: "W4Epis", 8: "G8Epis"}
TILES = (1, 2, 3, 4, 5, 7, 8, 11)
STORAGE = (BF, HF)  # every family is built a second time under LC_F16


def cells():
    """(compute, refuse): lists of (storage, tile, epilogue name). A compute cell runs and is
    checked; a refuse cell names an epilogue outside the forced family's list and must raise.
    Tile 8 with an epilogue gemm8_kernel lacks runs on the ping-pong kernel, so it computes when
    that kernel has it. EPI_RESID16 takes bf16 operands only (ops.gemm_nt): no half cells."""
    compute, refuse = [], []
    for st in STORAGE:
        for tile in TILES:
            have = set(FAMILY_EPIS[TILE_FAMILY[tile]])
            if tile == 8:
                have |= set(FAMILY_EPIS["PpEpis"])
            for name in EPI:
                if name == "RESID16" and st == HF:
                    continue
                (compute if name in have else refuse).append((st, tile, name))
    return compute, refuse


CELLS, REFUSED = cells()

# N = 768: at least three column tiles for every family. K: an even count of 64-wide k-tiles, an
# odd count, a single one. M = 293: two or three row tiles, the last 37 rows ragged; M = 5: one
# tile shorter than a pass. N = 64: route_tile falls a forced 256- or 128-wide tile back to 128x64.
SHAPES = tuple((M, 768, K) for K in (128, 192, 64) for M in (293, 5)) + ((293, 64, 192),)
PRE_MAX = 16.0


def parse_epilists(path=GEMM_HIP):
    """{list name: (epilogue names without EPI_)} of every `using X = EpiList<...>;` in gemm.hip."""
    txt = open(path).read()
    out = {}
    for name, body in re.findall(r"using\s+(\w+)\s*=\s*EpiList<([^>]*)>\s*;", txt):
        out[name] = tuple(e.strip()[len("EPI_"):] for e in body.split(",") if e.strip())
    return out


# ------------------------------------------------------------------------------------- helpers
def spacing(x, dtype):
    """The distance from |x| to the next larger value of `dtype` (bf16 or half), elementwise in
    float64: 2^(e - p) for 2^e <= |x| < 2^(e+1) with p = 7 (bf16) or 10 (half) mantissa bits,
    the subnormal step below the smallest normal number (zero included)."""
    p, emin = {BF: (7, -126), HF: (10, -14)}[dtype]
    x = torch.as_tensor(x, dtype=torch.float64)
    _, e = torch.frexp(x.abs())  # |x| = m 2^e, 1/2 <= m < 1
    e = torch.where(x == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.ldexp(torch.ones_like(x), e - p)


SENTINEL = {2: 0x7FC1, 4: 0x7FC12345}  # by element size: a NaN in bf16, half and f32
_INT = {2: torch.int16, 4: torch.int32}


def as_int(t):
    """The same memory as integers of the element size (bf16 / half -> int16, f32 -> int32)."""
    return t.view(_INT[t.element_size()])


def fill_sentinel(t):
    as_int(t).fill_(SENTINEL[t.element_size()])
    return t


def untouched(t):
    """Every element of t still holds the sentinel (compared as integers: the sentinel is a NaN)."""
    return bool((as_int(t) == SENTINEL[t.element_size()]).all())


def guards_intact(buf, M, N):
    """Rows >= M and columns >= N of a sentinel-filled buffer still hold the sentinel."""
    return untouched(buf[M:, :]) and untouched(buf[:M, N:])


def exact_cast(x64, dtype):
    """x64 (float64, exactly representable in f32) rounded to nearest even in `dtype`: through f32
    so that one rounding happens, as in the kernel (its epilogue value is an f32)."""
    x32 = x64.to(F32)
    assert torch.equal(x32.double(), x64), "reference value is not exact in f32"
    return x32.to(dtype)


# -------------------------------------------------------------------------- inputs, reference
@functools.lru_cache(maxsize=None)
def inputs(M, N, K):
    """The case's inputs in float64 on the CPU (one fixed seed per shape; treat as read-only)."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    return {
        "A": ri(-1, 1, (M, K)),
        "B": ri(-1, 1, (N, K)) / 8,
        "bias": ri(-8, 8, (N,)) / 4,                  # multiples of 1/4 in [-2, 2]
        "resid": ri(-8192, 8192, (M, N)) / 1024,      # f32 residual
        # half residual: multiples of 1/1024 in [-2, 2] (exact in half), so aux + pre needs
        # rounding in half wherever the sum leaves [-2, 2]
        "resid16": ri(-2048, 2048, (M, N)) / 1024,
        # odd multiples of 1/64 (bf16: 8 significant bits) or 1/512 (half: 11) below 4, so
        # pre * aux needs rounding in the output type; the product is exact in f32
        "mul": (2 * ri(-128, 127, (M, N)) + 1) / 64,
        "mul_h": (2 * ri(-1024, 1023, (M, N)) + 1) / 512,
        "bwd": ri(-48, 48, (M, N)) / 8,               # multiples of 1/8 in [-6, 6]
    }


def alpha_of(name):
    return 1.0 if name in ("GELU", "GELU_D") else 0.5


def has_bias(name):
    return name not in ("GELU_BWD", "MUL")


def aux_of(name, storage=BF):
    """The key of the epilogue's side input in inputs(), or None (MUL: one per storage type)."""
    return {"RESID": "resid", "RESID16": "resid16", "MUL": "mul" if storage == BF else "mul_h",
            "GELU_BWD": "bwd"}.get(name)


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def quick_gelu_grad(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1 + 1.702 * x * (1 - s))


@functools.lru_cache(maxsize=None)
def reference(M, N, K, name, storage=BF):
    """float64 reference of one epilogue on inputs(M, N, K) (storage: the 16-bit type, which picks
    MUL's side input and nothing else): dict with `pre` (= alpha acc + bias),
    `v` (the exact multiplier of the bound: alpha acc for GELU_BWD, else None), `out0`, `out1`
    (None when absent) in float64, and `exact0` / `exact1`: whether the output is exact
    arithmetic (compared bit for bit after one rounding) or a transcendental (bounded)."""
    x = inputs(M, N, K)
    alpha = alpha_of(name)
    acc = x["A"] @ x["B"].t()
    pre = alpha * acc + (x["bias"] if has_bias(name) else 0.0)
    r = {"pre": pre, "v": None, "out1": None, "exact0": True, "exact1": True}
    if name in ("BF16", "F32", "BF16_F32"):
        r["out0"] = pre
        if name == "BF16_F32":
            r["out1"] = pre
    elif name == "RESID":
        r["out0"] = x["resid"] + pre
    elif name == "RESID16":
        r["out0"] = x["resid16"] + pre
    elif name == "MUL":
        r["out0"] = pre * x[aux_of(name, storage)]
    elif name == "GELU":
        r["out0"], r["out1"], r["exact1"] = pre, quick_gelu(pre), False
    elif name == "GELU_D":
        r["out0"], r["out1"] = quick_gelu_grad(pre), quick_gelu(pre)
        r["exact0"] = r["exact1"] = False
    elif name == "GELU_BWD":
        r["out0"], r["v"], r["exact0"] = pre * quick_gelu_grad(x["bwd"]), pre, False
    else:
        raise KeyError(name)
    return r


def out_dtypes(name, storage):
    """(out0 dtype, out1 dtype or None) of an epilogue at 16-bit storage type `storage`."""
    if name in ("F32", "RESID"):
        return F32, None
    if name == "RESID16":
        return HF, None
    if name == "BF16_F32":
        return storage, F32
    if name in ("GELU", "GELU_D"):
        return storage, storage
    return storage, None


def bound(ref64, v, dtype):
    """The elementwise bound of a transcendental output: one step of the output type at the
    reference plus 2^-17 max(1, |v|) (derivation: test_gemm_epilogue_matrix_gpu's docstring)."""
    scale = torch.ones_like(ref64) if v is None else v.abs().clamp_min(1.0)
    return spacing(ref64, dtype) + 2.0 ** -17 * scale
