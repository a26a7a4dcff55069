"""Inputs, float64 references and bounds of the adapter / LoRA / LayerNorm kernel matrices
(tests/test_peft_matrix_gpu.py, tests/test_layernorm_matrix_gpu.py). Nothing here needs a GPU:
tests/test_peft_cases.py checks the claims below, the references against torch autograd, the
dropout mask against a big-integer restatement, and the tables against peft.hip / norm.hip.

Exact inputs (the recipe of gemm_epi_cases). z, gout, X, dY hold {-1, 0, 1}; the adapter weights
{-1, 0, 1} / 8; the biases multiples of 1/4 in [-2, 2]; the residual multiples of 1/4 in [-8, 8];
the adapter scale is 1/4 and keep is 1 or 1/2, so 1 / keep is exact; LoRA A holds {-1, 0, 1} / 4,
B^T {-1, 0, 1} / 8, the LoRA scaling is 1/4; accumulation targets start from small multiples of
1/4. Every input is exact in bf16 and in IEEE half, every product is a multiple of a power of two,
and every partial sum stays far below 2^24 of those units, so the value entering each rounding is
the same in any summation order:

  pre  = z Wd^T + bd                a multiple of 1/8,   |pre| < 32 (asserted: PRE_MAX)
  h    = relu(pre) mask / keep      a multiple of 1/8 (keep 1) or 1/4 (keep 1/2), < 64: exact in
                                    bf16 (8 significant bits) and in half
  x_out = resid + z + (h Wu^T + bu) / 4   a multiple of 1/256 (keep 1) or 1/128: exact in f32;
                                    the cast to half rounds wherever |x_out| >= 8 (keep 1)
  dpre = (h > 0) (gout Wu) / (4 keep)     a multiple of 1/32 or 1/16, < 16: exact in bf16 / half
  dz   = gout + dpre Wd             a multiple of 1/256 or 1/128: exact in f32, rounds in bf16
  XA   = X A^T, dYB = dY B          multiples of 1/4, 1/8, < 64 / < 32: exact in bf16 (the kernel
                                    rounds them to bf16: a no-op here, kept in the reference)
  weight / LoRA gradients           sums of M such products: exact in f32 (asserted from the sum
                                    of absolute values, EXACT_F32)

The residual of the keep-1/2 half cell (`resid_fine`): x_out is a multiple of 1/128 there, which
half holds exactly below 16, so with the residual in [-8, 8] no value would round whatever its
granularity. That cell's residual is a multiple of 1/64 in [-24, 24] (exact in half: the spacing
on [16, 32) is 1/64), so the odd multiples of 1/128 beyond 16 round, and they are ties: round to
nearest even, truncation and round-half-away all differ.

LayerNorm bounds: ln_fwd_bounds / ln_bwd_bound (derivations in their docstrings).
"""
import functools
import os
import re

import numpy as np
import torch

from gemm_epi_cases import BF, F32, HF, ROOT, exact_cast, spacing  # noqa: F401  (shared helpers)

PEFT_HIP = os.path.join(ROOT, "lifelong-clip_amd", "csrc", "peft.hip")
NORM_HIP = os.path.join(ROOT, "lifelong-clip_amd", "csrc", "norm.hip")
GEMM_HIP = os.path.join(ROOT, "lifelong-clip_amd", "csrc", "gemm.hip")
F64 = torch.float64

# ------------------------------------------------------------------ tables (checked against source)
LN_V = (1, 2, 4, 8, 12, 16)                       # LC_LN_F / LC_LN_B: D / 64
LN_D = tuple(64 * v for v in LN_V)
LORA_KT_NC = ((24, 18), (24, 6), (16, 12), (16, 4))  # LC_LG(KT, NC): K = 32 KT, N = 128 NC
LORA_KN = tuple((32 * kt, 128 * nc) for kt, nc in LORA_KT_NC)
FUSED_D = (768, 512)                              # adapter_ln_fwd, adapter_bwd_fused
AD_H = 64                                         # the bottleneck width
AD_R, AD_NS = 32, 3                               # adapter backward walker: rows per block, ring
ALN_R = 16                                        # adapter + LayerNorm forward: rows per block
LORA_R = 32                                       # LoRA walker: rows per block
AD_BWD_FUSED_MIN_M = 1024                         # below: the bf16 entry takes the two-GEMM form
SEED_DEV_MUL = 0xD1B54A32D192ED03
CUS_NOMINAL = 256                                 # the MI355X; the GPU files ask the device

SCALE = 0.25
LORA_S = 0.25
SEED = 0x1234567890ABCDEF
PRE_MAX, H_MAX, DPRE_MAX, XA_MAX, DYB_MAX = 32.0, 64.0, 16.0, 64.0, 32.0
EXACT_F32 = 2.0 ** 24
EPS = float(np.float32(1e-5))                     # the kernels' 1e-5f


def walker_rows(R, cus, d):
    """Rows that give walkers 0 and 1 d blocks of R rows (walker 1's last one ragged, 5 rows) and
    every other walker d - 1."""
    return R * (cus * (d - 1) + 1) + 5


def adapter_fwd_rows(cus):
    return {"M5": 5, "full": ALN_R * cus, "w1": walker_rows(ALN_R, cus, 1),
            "w2": walker_rows(ALN_R, cus, 2), "w3": walker_rows(ALN_R, cus, 3)}


def adapter_bwd_rows(cus):
    r = {"M37": 37, "M1031": 1031, "full2": AD_R * cus * 2}
    r.update({f"w{d}": walker_rows(AD_R, cus, d) for d in (1, 2, 3, 4)})
    return r


WGRAD_ROWS = {"M37": 37, "M4133": 4096 + 37}


def lora_rows(cus):
    r = {"M1": 1, "M31": 31, "full2": LORA_R * cus * 2}
    r.update({f"w{d}": walker_rows(LORA_R, cus, d) for d in (1, 2, 3)})
    return r


def parse_tables():
    """The same tables read from the source text."""
    peft, norm, gemm = (open(p).read() for p in (PEFT_HIP, NORM_HIP, GEMM_HIP))
    ints = lambda pat, txt: [tuple(int(v) for v in m) if isinstance(m, tuple) else int(m)
                             for m in re.findall(pat, txt)]
    return {
        "ln_f": tuple(ints(r"LC_LN_F\((\d+)\)", norm)),
        "ln_b": tuple(ints(r"LC_LN_B\((\d+)\)", norm)),
        "lora": tuple(ints(r"LC_LG\((\d+),\s*(\d+)\)", peft)),
        "fused_d": [tuple(sorted(p, reverse=True)) for p in ints(r"\(D == (\d+) \|\| D == (\d+)\)", peft)],
        "ad_mt": ints(r"constexpr int AD_MT = (\d+);", peft),
        "ad_r_is_16_mt": len(re.findall(r"constexpr int AD_R = 16 \* AD_MT;", peft)),
        "ad_ns": ints(r"constexpr int AD_NS = (\d+);", peft),
        "ad_h": ints(r"constexpr int AD_H = (\d+);", peft),
        "aln_blocks": len(re.findall(r"const int nblk = \(M \+ 15\) / 16;", peft)),
        "lora_blocks": len(re.findall(r"const int nblk = \(M \+ 31\) / 32;", peft)),
        "ad_bwd_min_m": ints(r"\(D == 768 \|\| D == 512\) && M >= (\d+)", peft),
        "seed_dev_mul": [int(v, 16) for v in
                         re.findall(r"seed \+= \*(?:ep\.)?seed_dev \* 0x([0-9A-Fa-f]+)ull", peft + gemm)],
    }


# ----------------------------------------------------------------------------- the dropout mask
def _u64(v):
    return np.asarray([int(v) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)


def drop_keep(seed, rows, keep, seed_dev=None):
    """The keep mask of drop_mul (lc_common.h) as a bool array [len(rows), 64], in numpy uint64
    arithmetic (wrapping mod 2^64). rows: the dropout row ids m * row_mul + row_add. seed_dev:
    the device-side epoch, seed += epoch * 0xD1B54A32D192ED03 first."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    if np.float32(keep) >= np.float32(1.0):
        return np.ones((rows.shape[0], AD_H), dtype=bool)
    s = _u64(seed)
    if seed_dev is not None:
        s = s + _u64(seed_dev) * _u64(SEED_DEV_MUL)
    idx = rows * np.uint64(AD_H) + np.arange(AD_H, dtype=np.uint64).reshape(1, -1)
    z = s + _u64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * _u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * _u64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    hsh = z >> np.uint64(32)
    u = (hsh >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u < np.float32(keep)


def row_ids(M, rows=None):
    mul, add = (1, 0) if rows is None else rows
    return np.arange(M, dtype=np.uint64) * np.uint64(mul) + np.uint64(add)


# --------------------------------------------------------------------------------------- inputs
def _ri(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


@functools.lru_cache(maxsize=3)
def adapter_inputs(M, D):
    """The adapter case's inputs as f32 on the CPU, every value exact (treat as read-only)."""
    g = torch.Generator().manual_seed(7919 * M + D)
    return {
        "z": _ri(g, -1, 1, (M, D)),
        "gout": _ri(g, -1, 1, (M, D)),
        "Wd": _ri(g, -1, 1, (AD_H, D)) / 8,
        "Wu": _ri(g, -1, 1, (D, AD_H)) / 8,
        "bd": _ri(g, -8, 8, (AD_H,)) / 4,
        "bu": _ri(g, -8, 8, (D,)) / 4,
        "resid": _ri(g, -32, 32, (M, D)) / 4,
        "resid_fine": _ri(g, -24 * 64, 24 * 64, (M, D)) / 64,
        "gamma": torch.randn(D, generator=g).to(F32),
        "beta": torch.randn(D, generator=g).to(F32),
        # accumulation targets: multiples of 1/4 in [-2, 2]
        "dWu0": _ri(g, -8, 8, (D, AD_H)) / 4, "dbu0": _ri(g, -8, 8, (D,)) / 4,
        "dWd0": _ri(g, -8, 8, (AD_H, D)) / 4, "dbd0": _ri(g, -8, 8, (AD_H,)) / 4,
    }


@functools.lru_cache(maxsize=3)
def lora_inputs(M, K, N):
    g = torch.Generator().manual_seed(104729 * M + 13 * K + N)
    return {
        "X": _ri(g, -1, 1, (M, K)),
        "dY": _ri(g, -1, 1, (M, N)),
        "A": _ri(g, -1, 1, (4, K)) / 4,     # rows < r are used
        "Bt": _ri(g, -1, 1, (4, N)) / 8,
        "dA0": _ri(g, -8, 8, (4, K)) / 4,
        "dB0": _ri(g, -8, 8, (N, 4)) / 4,
    }


# ----------------------------------------------------------------------------------- references
def adapter_fwd_math(z, Wd, bd, Wu, bu, resid, keepmask, keep, scale=SCALE):
    """adapter.py's forward in the given dtype (float64 here, plain torch ops: autograd runs
    through it in test_peft_cases): (pre, h, x_out)."""
    pre = z @ Wd.t() + bd
    h = torch.relu(pre) * keepmask / keep
    return pre, h, resid + z + scale * (h @ Wu.t() + bu)


@functools.lru_cache(maxsize=4)
def adapter_fwd_ref(M, D, keep, fine=False, rows=None, seed_dev=None, seed=SEED):
    """float64 (pre, h, x_out, keepmask) of the adapter forward on adapter_inputs(M, D). fine:
    the residual `resid_fine`; rows: (mul, add) of the dropout row ids; seed_dev: the epoch."""
    x = {k: v.double() for k, v in adapter_inputs(M, D).items()}
    mask = torch.from_numpy(drop_keep(seed, row_ids(M, rows), keep, seed_dev))
    pre, h, xo = adapter_fwd_math(x["z"], x["Wd"], x["bd"], x["Wu"], x["bu"],
                                  x["resid_fine" if fine else "resid"], mask.double(), keep)
    assert pre.abs().max().item() < PRE_MAX and h.max().item() < H_MAX
    return pre, h, xo, mask


BWD_KEEP = 0.5


def adapter_bwd_math(gout, h, Wu, Wd, keep, scale=SCALE):
    """(dpre, dz) of adapter.py's autograd with the mask taken from h > 0 (ReLU and dropout)."""
    dpre = torch.where(h > 0, scale * (gout @ Wu) / keep, torch.zeros_like(h))
    return dpre, gout + dpre @ Wd


@functools.lru_cache(maxsize=3)
def adapter_bwd_ref(M, D):
    """float64 (h, dpre, dz): h from the reference forward with keep 1/2 (its zeros are ReLU and
    dropout zeros), dpre and dz from gout."""
    x = adapter_inputs(M, D)
    h = adapter_fwd_ref(M, D, BWD_KEEP)[1]
    dpre, dz = adapter_bwd_math(x["gout"].double(), h, x["Wu"].double(), x["Wd"].double(), BWD_KEEP)
    assert dpre.abs().max().item() < DPRE_MAX
    # the kernels form dz from dpre as stored (bf16 / half): the same value
    for dt in (BF, HF):
        assert torch.equal(dpre.to(dt).double(), dpre)
    return h, dpre, dz


@functools.lru_cache(maxsize=3)
def adapter_wgrad_ref(M, D, scale=SCALE):
    """float64 (dWu, dbu, dWd, dbd) accumulated onto the start values, and the largest sum of
    absolute terms in units of the granularity (exact in f32 while < 2^24)."""
    x = {k: v.double() for k, v in adapter_inputs(M, D).items()}
    h, dpre, _ = adapter_bwd_ref(M, D)
    g, z = x["gout"], x["z"]
    out = (x["dWu0"] + scale * (g.t() @ h), x["dbu0"] + scale * g.sum(0),
           x["dWd0"] + dpre.t() @ z, x["dbd0"] + dpre.sum(0))
    # units: h 1/4 (keep 1/2), dpre 1/16, the start values and scale exact powers of two on top
    mass = max((g.abs().t() @ h.abs()).max().item() * 4 + 8, (dpre.abs().t() @ z.abs()).max().item() * 16 + 32,
               dpre.abs().sum(0).max().item() * 16 + 32, g.abs().sum(0).max().item() + 8)
    assert mass < EXACT_F32
    return out


@functools.lru_cache(maxsize=3)
def lora_ref(M, K, N, r, s=LORA_S):
    """float64 (dA [r, K], dB [N, r]) of the one-pass LoRA gradients onto the start values; XA and
    dYB rounded to bf16 as the kernel rounds them."""
    x = {k: v.double() for k, v in lora_inputs(M, K, N).items()}
    X, dY, A, Bt = x["X"], x["dY"], x["A"][:r], x["Bt"][:r]
    xa, dyb = X @ A.t(), dY @ Bt.t()
    assert xa.abs().max().item() < XA_MAX and dyb.abs().max().item() < DYB_MAX
    xa, dyb = xa.to(BF).double(), dyb.to(BF).double()
    dB = x["dB0"][:, :r] + s * (dY.t() @ xa)
    dA = x["dA0"][:r] + s * (dyb.t() @ X)
    mass = max((dY.abs().t() @ xa.abs()).max().item() * 4, (dyb.abs().t() @ X.abs()).max().item() * 8) + 32
    assert mass < EXACT_F32
    return dA, dB


def ln_fwd_ref(x, gamma, beta):
    """float64 (mean, rstd, y) of LayerNorm over the last dimension, eps = the kernels' 1e-5f."""
    mean = x.mean(1)
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((d * d).mean(1) + EPS)
    return mean, rstd, d * rstd[:, None] * gamma + beta


def ln_bwd_ref(dy, x, mean, rstd, gamma, dres=None):
    """float64 dx (+ dres) of LayerNorm given the saved mean and rstd (taken as exact)."""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx if dres is None else dx + dres


# --------------------------------------------------------------------------- LayerNorm bounds
U = 2.0 ** -24   # unit roundoff of f32
T = 40           # see ln_fwd_bounds


def _step(ref, dtype):
    return torch.zeros_like(ref) if dtype == F32 else spacing(ref, dtype)


def ln_fwd_bounds(x, gamma, beta, ref, ydtype):
    """Elementwise / per-row bounds (b_mean [R], b_rstd [R], b_y [R, D]) of a LayerNorm forward
    computed in f32 against ln_fwd_ref on the same x (float64 of the stored values).

    u = 2^-24. An f32 sum of D terms in a tree of depth t errs by at most t u sum|x_i| (first
    order). The depths in the code: ln_fwd_kernel / ln_bwd_kernel sum V = D / 64 <= 16 terms per
    lane in sequence, then 6 butterfly levels: t = V + 6 <= 22; adapter_ln_fwd_kernel sums 4 NU
    terms per lane (NU = D / 128 <= 6), 2 shuffles, 8 waves in sequence: t = 4 NU + 10 <= 34.
    T = 40 is used for all of them; the 6 units above the deepest tree pay for the roundings
    around each sum (the terms' own roundings, the product with the rounded constant 1 / D, the
    added eps), so they are not listed again. A kernel that sums deeper than 34 must revisit T.

      mean:  |mean - mu| <= dmu = T u mean|x| + u |mu|
      rstd:  the kernel's variance is that of x about its own mean, mean((x - mu)^2) + dmu^2, with
             a relative error of at most (T + 6) u (three roundings per squared term, the tree, 1 / D
             and eps); the square root halves relative errors and rsqrtf adds at most 2 ulp = 4 u:
             |rstd / ref - 1| <= rho = ((T + 6) / 2 + 4) u + dmu^2 rstd^2 / 2
      y:     y = ((x - mean) rstd) gamma + beta: the deviation carries dmu and one rounding, the
             two products and the sum one rounding each of magnitudes <= |ref| + |beta|:
             |y - ref| <= step(ref) + |gamma| rstd (dmu + |x - mu| rho) + 4 u (|ref| + |beta|)
             step: one step of a 16-bit output type at ref (half a step of rounding, of a value
             that may sit on the other side of a rounding boundary), 0 for f32 output.
    """
    mean, rstd, y = ref
    dmu = T * U * x.abs().mean(1) + U * mean.abs()
    rho = ((T + 6) / 2 + 4) * U + 0.5 * dmu * dmu * rstd * rstd
    b_y = (_step(y, ydtype) + gamma.abs() * rstd[:, None] * (dmu[:, None] + (x - mean[:, None]).abs() * rho[:, None])
           + 4 * U * (y.abs() + beta.abs()))
    return dmu, rho * rstd, b_y


def ln_bwd_bound(dy, x, mean, rstd, gamma, ref, dxdtype):
    """Elementwise bound [R, D] of an f32 LayerNorm backward against ln_bwd_ref with the same saved
    mean and rstd (f32 values, exact inputs of both): the kernel forms xh = (x - mean) rstd
    (2 roundings), g = dy gamma (1), s1 = mean(g), s2 = mean(g xh) by the trees of ln_fwd_bounds
    (T covers the tree, the terms' <= 4 roundings and 1 / D):
        ds1 = T u mean|g|,  ds2 = T u mean|g xh|
    and out = rstd ((g - s1) - xh s2) (+ dres): with a = |g| + |s1| + |xh s2| the roundings of g,
    of xh inside the product, of the product, of the two differences and of the scaling by rstd
    are at most 5 u a together; the final sum with dres (or the scaling alone) rounds once more:
        |dx - ref| <= step(ref) + rstd (ds1 + |xh| ds2 + 5 u a) + u |ref|
    step: one step of a half dx at ref, 0 for f32."""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    ds1 = T * U * g.abs().mean(1, keepdim=True)
    ds2 = T * U * (g * xh).abs().mean(1, keepdim=True)
    a = g.abs() + s1.abs() + (xh * s2).abs()
    return _step(ref, dxdtype) + rstd[:, None] * (ds1 + xh.abs() * ds2 + 5 * U * a) + U * ref.abs()


LN_ROWS = (1, 5, 333)
LN_SPECIAL = ("mean100", "outlier", "const2", "zeros")


@functools.lru_cache(maxsize=None)
def ln_inputs(rows, D):
    """f32 inputs of a LayerNorm cell on the CPU: x [rows, D] (ordinary rows 3 randn + 1; with
    rows >= 5 the last four are a row of mean 100 and spread 1, a row of unit values with one
    outlier of 200, a constant row of 2 and a row of zeros: LN_SPECIAL, in that order), gamma,
    beta, dy, dres (f32; the tests round copies to the cell's types)."""
    g = torch.Generator().manual_seed(31 * rows + D)
    x = torch.randn(rows, D, generator=g) * 3 + 1
    if rows >= 5:
        x[-4] = 100 + torch.randn(D, generator=g)
        x[-3] = torch.randn(D, generator=g)
        x[-3, D // 3] = 200.0
        x[-2] = 2.0
        x[-1] = 0.0
    return {"x": x, "gamma": torch.randn(D, generator=g), "beta": torch.randn(D, generator=g),
            "dy": torch.randn(rows, D, generator=g), "dres": torch.randn(rows, D, generator=g) * 2}
