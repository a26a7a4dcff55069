"""Inputs, float64 references, derived bounds and wrong variants for the kernels that finish every
training step (no GPU needed): csrc/head.hip (lc_l2norm_rows, lc_clip_head, lc_head_logits,
lc_softmax_bwd_rows, lc_head_feat_grad, lc_grad_pow2_normalize, lc_add_unscaled) and the AdamW /
finite-check / counter block at the end of csrc/peft.hip. tests/test_step_tail_gpu.py runs the
kernels against this module; tests/test_tail_cases.py checks the module itself.

References are float64 restatements of the operation on the STORED f32 inputs widened to float64,
the f32-rounded hyperparameters included (lc_adamw receives `float b2`, so the reference's b2 is
float32(0.999), not 0.999).

Bounds are elementwise and come from a running error analysis (class V below): every quantity is
a pair (float64 value, absolute error bound), and each f32 operation of the kernel adds what that
operation can add. With u = 2^-24 (f32 unit roundoff) and eta = 2^-149 (the subnormal spacing: an
underflowing result is off by at most that):

  round    a correctly rounded result r~ of a value with bound e:  e + u (|r| + e) + eta
  a * b    |a| e_b + |b| e_a + e_a e_b, then round
  a +- b   e_a + e_b, then round
  a / b    (e_a + |a / b| e_b) / (|b| - e_b), then round   (IEEE division: the build has no
           fast-math flag, and hipcc's f32 division and sqrtf are correctly rounded by default)
  sqrt a   |sqrt x - sqrt y| = |x - y| / (sqrt x + sqrt y) <= min(e_a / (sqrt lo + sqrt a),
           sqrt e_a) with lo = max(a - e_a, 0), then round
  sum      of n terms at depth d (the longest chain of additions any term passes through):
           sum e_i + d u sum (|t_i| + e_i); the depths are read off the kernels:
             dots / row sums over a 64-lane wave: ceil(n / 64) strided terms per lane, then six
               butterfly levels (wave_sum): one product rounding + ceil(n / 64) - 1 + 6 additions,
               d = ceil(n / 64) + 6;
             the feature gradient's sum over Co: ceil(Co / 4) sequential terms per wave + 3 LDS
               additions on the 16-B route, ceil(Co / 8) + 7 on the scalar route, + the product:
               d = max(ceil(Co / 4) + 4, ceil(Co / 8) + 8) covers both;
             its n . dn: at most 4 terms per thread, six butterfly levels, 3 LDS additions and
               the product: d = 14;
             the loss: B atomic additions in any order, d = B.

ASSUMPTION (the one constant that cannot be derived from the project): the hardware functions.
  __expf(x) is exp2(x * log2(e)) on v_exp_f32: one rounding of x * log2(e), whose relative
  error u becomes an absolute error u |x| log2(e) of the exponent, i.e. ~|x| u relative, twice
  (the constant log2(e) is itself rounded), plus a 1-ulp (2 u) v_exp_f32 and margin for the
  multiply: EXPF_REL(x) = (2 |x| + 4) u relative. Results below 2^-126 may be flushed to zero:
  an absolute 2^-126 on top. logf: LOGF_REL = 4 u relative.
powf (the bias corrections, host libm or device) is taken as 1 ulp = 2 u of b^t, which is
K_bc(t) = 2 b^t / (1 - b^t) units of 1 - b^t; the subtraction adds one more.

Every bound comes with two CPU proofs (test_tail_cases.py): a plain f32 torch restatement of the
same formula stays inside it on every case (the bound admits a correct f32 implementation), and
each listed wrong variant leaves it, or fails an exact case, on at least one case (the bound has
teeth)."""
import functools
import math
import os
import re

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
ETA = 2.0 ** -149
FLUSH = 2.0 ** -126
LOGF_REL = 4 * U

# limits quoted from the source (test_tail_cases.py::test_constants_match_the_source)
E_MAX, C_MAX = 1024, 8192
CTR_MAX = 64
GRID_CAP, BLOCK = 4096, 256
SWEEP = GRID_CAP * BLOCK            # elements one grid sweep of finite_kernel / adamw_kernel covers
NORMALIZE_THREADS = 1024
TARGET_MAX = 100
K_MIN, K_MAX = -126, 127

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lifelong-clip_amd", "csrc")

LS_CLIP = float(np.float32(math.log(1 / 0.07)))
LS_100 = float(np.float32(math.log(100.0)))


def f32r(x):
    """The value a `float` argument receives."""
    return float(np.float32(x))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------ running error analysis
class V:
    """value (float64 tensor) +- e (float64 tensor, >= 0)."""

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=F64)
        self.e = torch.zeros_like(self.v) if e is None else torch.as_tensor(e, dtype=F64)


def _rnd(v, e):
    return V(v, e + U * (v.abs() + e) + ETA)


def vmul(a, b):
    return _rnd(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)


def vadd(a, b):
    return _rnd(a.v + b.v, a.e + b.e)


def vsub(a, b):
    return _rnd(a.v - b.v, a.e + b.e)


def vdiv(a, b):
    q = a.v / b.v
    den = b.v.abs() - b.e
    assert (den > 0).all(), "divisor not separated from zero"
    return _rnd(q, (a.e + q.abs() * b.e) / den)


def vsqrt(a):
    lo = (a.v - a.e).clamp_min(0)
    r = a.v.sqrt()
    den = lo.sqrt() + r
    e = torch.where(den > 0, torch.minimum(a.e / den.clamp_min(1e-300), a.e.sqrt()), a.e.sqrt())
    return _rnd(r, e)


def vsum(t, dim, depth, keepdim=False):
    """Sum of the terms t (products already rounded by vmul) at addition depth `depth`."""
    mass = (t.v.abs() + t.e).sum(dim, keepdim=keepdim)
    g = depth * U / (1 - depth * U)
    return V(t.v.sum(dim, keepdim=keepdim), t.e.sum(dim, keepdim=keepdim) + g * mass)


def vexpf(a):
    """__expf under the module's assumption."""
    r = a.v.exp()
    rel = torch.expm1(a.e) + (2 * (a.v.abs() + a.e) + 4) * U * a.e.exp()
    return V(r, r * rel + FLUSH)


def vlogf(a):
    assert (a.v - a.e > 0).all()
    r = a.v.log()
    return V(r, a.e / (a.v - a.e) + LOGF_REL * r.abs() + ETA)


def wave_depth(n):
    return cdiv(n, 64) + 6


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (NaN anywhere in got gives inf)."""
    got = torch.as_tensor(got).detach().cpu().to(F64)
    err = (got - ref).abs()
    if not torch.isfinite(err).all():
        return math.inf
    r = err / bound
    r = torch.where(err == 0, torch.zeros_like(r), r)
    return float(r.max()) if r.numel() else 0.0


# -------------------------------------------------------------------------------------- l2norm
def l2norm_ref(f):
    f = f.to(F64)
    n = (f * f).sum(-1).sqrt()
    return f / n[:, None], n


def l2norm_bounds(f):
    x = V(f.to(F64))
    n = vsqrt(vsum(vmul(x, x), -1, wave_depth(f.shape[1]) - 1))
    inv = vdiv(V(torch.ones_like(n.v)), n)
    out = vmul(x, V(inv.v[:, None], inv.e[:, None]))
    return out.e, n.e


def l2norm_exact_case(R, E, seed=0):
    """Rows of 4 entries +-2 (norm 4, output +-1/2) or, for E >= 16 on odd rows, 16 entries +-1/2
    (norm 2, output +-1/4); E < 4: one entry +-4 (norm 4, output +-1). The sum of squares is an
    integer <= 16, exact in any order; sqrt, 1 / norm and the product are exact."""
    g = gen(1000 + 37 * R + E + seed)
    f = torch.zeros(R, E)
    for r in range(R):
        k, val = (1, 4.0) if E < 4 else ((16, 0.5) if (E >= 16 and r % 2) else (4, 2.0))
        idx = torch.randperm(E, generator=g)
        if r == 0:                               # the last column is used
            idx = torch.cat([torch.tensor([E - 1]), idx[idx != E - 1]])
        idx = idx[:k]
        sign = torch.randint(0, 2, (k,), generator=g).float() * 2 - 1
        f[r, idx] = sign * val
    return f


# ---------------------------------------------------------------------------------------- head
def head_case(B, C, E, ls, seed=0):
    """randn rows normalised in float64 and stored as f32, with the hard elements: class rows 0
    and 1 a near-duplicate pair (C >= 2), image row 0 a near copy of class row 0 (a logit close
    to exp(ls): at ln 100 it overflows an unshifted exp); labels random with 0 and C - 1 present
    when B >= 2."""
    g = gen(2000 + 131 * B + 17 * C + E + seed)
    fi = torch.randn(B, E, generator=g, dtype=F64)
    ft = torch.randn(C, E, generator=g, dtype=F64)
    if C >= 2:
        ft[1] = ft[0] + 1e-3 * torch.randn(E, generator=g, dtype=F64)
    fi[0] = ft[0] + 0.05 * torch.randn(E, generator=g, dtype=F64)
    img_n = l2norm_ref(fi)[0].to(F32)
    txt_n = l2norm_ref(ft)[0].to(F32)
    y = torch.randint(0, C, (B,), generator=g)
    if B >= 2:
        y[0], y[-1] = 0, C - 1
    return dict(img_n=img_n, txt_n=txt_n, ls=torch.tensor([ls], dtype=F32), y=y)


def head_ref(img_n, txt_n, ls, y):
    """logits = exp(ls) I T^T; probs = softmax(logits); loss = mean CE(probs, y), the CE taking
    the probabilities as its logits (the reference project's double softmax);
    dlogits = d loss / d logits."""
    I, T = img_n.to(F64), txt_n.to(F64)
    B = I.shape[0]
    lg = ls.to(F64).exp() * (I @ T.t())
    p = torch.softmax(lg, -1)
    q = torch.softmax(p, -1)
    oh = torch.nn.functional.one_hot(y, T.shape[0]).to(F64)
    loss = (torch.logsumexp(p, -1) - (p * oh).sum(-1)).sum() / B
    dp = (q - oh) / B
    dl = p * (dp - (p * dp).sum(-1, keepdim=True))
    return dict(logits=lg, probs=p, dlogits=dl, loss=loss)


def _softmax_bound(lg):
    """probs = softmax(logits) as the kernels compute it. The logit error D = max_c e(logit)
    enters through the softmax's sensitivity, p~_c / p_c in [exp(-2 D), exp(2 D)]; the
    computation itself (shift by the exact maximum, __expf, a wave sum of positive terms, an
    IEEE division) is analysed on the exact logits and scaled by exp(2 D)."""
    C = lg.v.shape[-1]
    D = lg.e.max(-1, keepdim=True).values
    x = lg.v - lg.v.max(-1, keepdim=True).values
    ex = vexpf(V(x, U * x.abs()))
    z = vsum(ex, -1, wave_depth(C) - 1, keepdim=True)
    pc = vdiv(ex, z)
    return V(pc.v, pc.e * (2 * D).exp() + pc.v * torch.expm1(2 * D))


def head_bounds(img_n, txt_n, ls, y, calls=1):
    """Bounds of lc_clip_head's outputs (and lc_head_logits': logits, probs). calls: how often the
    kernel accumulated into *loss (the bound is then that of calls x the loss: calls B atomic
    additions)."""
    I, T = img_n.to(F64), txt_n.to(F64)
    B, E = I.shape
    C = T.shape[0]
    s = vexpf(V(ls.to(F64)))
    mass = I.abs() @ T.abs().t()
    gd = wave_depth(E) * U / (1 - wave_depth(E) * U)
    lg = vmul(V(s.v.expand(B, C), s.e.expand(B, C)), V(I @ T.t(), gd * mass))
    p = _softmax_bound(lg)
    d = wave_depth(C) - 1
    e2 = vexpf(p)
    z2 = vsum(e2, -1, d, keepdim=True)
    q = vdiv(e2, z2)
    oh = torch.nn.functional.one_hot(y, C).to(F64)
    invB = V(torch.full((B, 1), 1.0 / B, dtype=F64), torch.full((B, 1), U / B, dtype=F64))
    dp = vmul(vsub(q, V(oh)), V(invB.v.expand(B, C), invB.e.expand(B, C)))
    dot = vsum(vmul(p, dp), -1, d, keepdim=True)
    dl = vmul(p, vsub(dp, V(dot.v.expand(B, C), dot.e.expand(B, C))))
    py = V((p.v * oh).sum(-1, keepdim=True), (p.e * oh).sum(-1, keepdim=True))
    rows = vmul(vsub(vlogf(z2), py), invB)
    loss = vsum(V(rows.v.repeat(calls, 1), rows.e.repeat(calls, 1)), 0, calls * B)
    return dict(logits=lg.e, probs=p.e, dlogits=dl.e, loss=loss.e.reshape(()))


def head_f32(img_n, txt_n, ls, y, variant=None):
    """The plain f32 torch restatement (variant None) and the wrong variants of HEAD_VARIANTS."""
    I, T = img_n.float(), txt_n.float()
    B, C = I.shape[0], T.shape[0]
    s = ls.float().exp()
    if variant == "scale_twice":
        s = s * s
    lg = s * (I @ T.t())
    yy = (y + 1) % C if variant == "label_off_by_one" else y
    oh = torch.nn.functional.one_hot(yy, C).float()
    if variant == "no_max_shift":
        ex = lg.exp()
    else:
        ex = (lg - lg.max(-1, keepdim=True).values).exp()
    if variant == "lane_tail_skipped" and C % 64:
        ex = ex.clone()
        ex[:, C - C % 64:] = 0
    p = ex / ex.sum(-1, keepdim=True)
    invB = 1.0 if variant == "no_inv_b" else 1.0 / B
    if variant == "single_softmax":
        loss = (torch.logsumexp(lg, -1) - (lg * oh).sum(-1)).sum() * invB
        dl = (p - oh) * invB
    else:
        e2 = p.exp()
        q = e2 / e2.sum(-1, keepdim=True)
        loss = (e2.sum(-1).log() - (p * oh).sum(-1)).sum() * invB
        dp = (q - oh) * invB
        dl = p * (dp - (p * dp).sum(-1, keepdim=True))
    return dict(logits=lg, probs=p, dlogits=dl, loss=loss)


# the GPU matrix's shapes (test_step_tail_gpu.py); the CPU proofs run the f32 restatement on all
HEAD_B, HEAD_C, HEAD_E = (1, 3, 64), (1, 2, 63, 64, 65, 200, 256), (4, 37, 512, 768, 1024)
HEAD_LS = (LS_CLIP, LS_100)
FG_R, FG_CO = 3, (1, 3, 4, 5, 8, 9, 256)
FG_E_VEC, FG_E_SCALAR = (4, 512, 1024), (37, 510)
HEAD_VARIANTS = ("single_softmax", "no_inv_b", "label_off_by_one", "lane_tail_skipped",
                 "no_max_shift", "scale_twice")
# (B, C, E, ls): the general cases the CPU proofs run on (the GPU cells add more shapes)
HEAD_CPU_CASES = ((1, 2, 4, LS_CLIP), (3, 65, 37, LS_100), (4, 200, 512, LS_CLIP),
                  (3, 200, 64, LS_100), (64, 10, 512, LS_100))


def uniform_case(B, C, E=64, seed=0):
    """All class rows equal: every logit of a row is the same f32 number, so p = 1 / C, the second
    softmax is 1 / C again and dlogits = (1 / C) (1 / C - [c == y]) / B bit for bit (C and B
    powers of two). Labels alternate between 0 and C - 1."""
    c = head_case(B, C, E, LS_CLIP, seed)
    c["txt_n"] = c["txt_n"][:1].expand(C, E).contiguous()
    c["y"] = torch.tensor([0 if b % 2 == 0 else C - 1 for b in range(B)])
    oh = torch.nn.functional.one_hot(c["y"], C).to(F64)
    c["dlogits_exact"] = ((1.0 / C) * (1.0 / C - oh) / B).to(F32)
    c["probs_exact"] = torch.full((B, C), 1.0 / C, dtype=F32)
    return c


def saturated_case(C, E, label_hot, k=1):
    """logit_scale = ln 100, img_n = e_k, txt_n[c] = -e_k except the hot class (+e_k): logits are
    +-exp(ls), the gap of ~200 exceeds 104 (exp(-104) < 2^-149), probs is exactly one-hot and
    dlogits exactly zero, whichever class the label names."""
    hot = C // 2
    img = torch.zeros(2, E)
    img[:, k] = 1
    txt = torch.zeros(C, E)
    txt[:, k] = -1
    txt[hot, k] = 1
    y = torch.full((2,), hot if label_hot else (hot + 1) % C)
    oh = torch.nn.functional.one_hot(torch.full((2,), hot), C).float()
    return dict(img_n=img, txt_n=txt, ls=torch.tensor([LS_100], dtype=F32), y=y, probs_exact=oh,
                dlogits_exact=torch.zeros(2, C))


def pow2_entries(shape, g, lo_exp, hi_exp, zero_share=0.25):
    """Entries {-1, 0, 1} * 2^-j, j in [lo_exp, hi_exp]."""
    sgn = torch.randint(-1, 2, shape, generator=g).float()
    keep = (torch.rand(shape, generator=g) >= zero_share).float()
    j = torch.randint(lo_exp, hi_exp + 1, shape, generator=g).float()
    return sgn * keep * torch.exp2(-j)


def logits_integer_case(B, C, E, seed=0):
    """lc_head_logits with logit_scale = 0 (__expf(0) = 1): entries {-1, 0, 1} * 2^-j, j <= 3:
    every product is a multiple of 2^-6 and every partial sum stays below E, so the f32 logits
    are exact in any summation order (E 2^6 = 2^16 units << 2^24)."""
    g = gen(3000 + 7 * B + 3 * C + E + seed)
    return dict(img_n=pow2_entries((B, E), g, 0, 3), txt_n=pow2_entries((C, E), g, 0, 3),
                ls=torch.zeros(1))


def softmax_bwd_case(B, C, seed=0):
    g = gen(4000 + 5 * B + C + seed)
    p = torch.softmax(3 * torch.randn(B, C, generator=g, dtype=F64), -1).to(F32)
    dp = torch.randn(B, C, generator=g)
    dp[0, C - 1] = 1e4
    return p, dp


def softmax_bwd_integer_case(B, C, seed=0):
    """p multiples of 1/16 in [0, 1], dp in {-1, 0, 1} * 2^-j (j <= 3): products are multiples of
    2^-7 below 1, the row sum stays below C <= 8192: C 2^7 units << 2^24, exact in any order."""
    g = gen(4500 + 5 * B + C + seed)
    p = torch.randint(0, 17, (B, C), generator=g).float() / 16
    return p, pow2_entries((B, C), g, 0, 3)


def softmax_bwd_ref(p, dp):
    p, dp = p.to(F64), dp.to(F64)
    return p * (dp - (p * dp).sum(-1, keepdim=True))


def softmax_bwd_bound(p, dp):
    P, D = V(p.to(F64)), V(dp.to(F64))
    dot = vsum(vmul(P, D), -1, wave_depth(p.shape[1]) - 1, keepdim=True)
    return vmul(P, vsub(D, V(dot.v.expand_as(P.v), dot.e.expand_as(P.v)))).e


def softmax_bwd_f32(p, dp):
    return p * (dp - (p * dp).sum(-1, keepdim=True))


# ---------------------------------------------------------------------------- feature gradient
def dlog_view(dlogits, R, Co, sr, sc):
    """dlog(r, c) = dlogits.flat[r * sr + c * sc] as an [R, Co] tensor."""
    return dlogits.reshape(-1).as_strided((R, Co), (sr, sc))


def featgrad_case(R, Co, E, orient, ls=LS_CLIP, ext=True, seed=0, zero_dlog=False):
    """orient "img": the B x C dlogits read as rows (sr, sc) = (Co, 1), the image side;
    "txt": the Co x R matrix read as columns (1, R), the text side."""
    g = gen(5000 + 11 * R + 7 * Co + E + seed + (0 if orient == "img" else 1))
    self_n = l2norm_ref(torch.randn(R, E, generator=g, dtype=F64))[0].to(F32)
    other_n = l2norm_ref(torch.randn(Co, E, generator=g, dtype=F64))[0].to(F32)
    shape, sr, sc = ((R, Co), Co, 1) if orient == "img" else ((Co, R), 1, R)
    dlog = torch.randn(shape, generator=g) * 0.1
    if zero_dlog:
        dlog.zero_()
    norms = (torch.rand(R, generator=g) * 9 + 1)
    dn_ext = torch.randn(R, E, generator=g) * 0.3 if ext else None
    return dict(dlogits=dlog, sr=sr, sc=sc, other_n=other_n, self_n=self_n, norms=norms,
                ls=torch.tensor([ls], dtype=F32), dn_ext=dn_ext)


def featgrad_integer_case(R, Co, E, orient, ext=True, seed=0):
    """logit_scale = 0; dlogits {-1, 0, 1} / 4, other_n and self_n {-1, 0, 1} * 2^-j (j <= 1),
    dn_ext multiples of 1/4 in [-2, 2], norms powers of two: dn is a multiple of 1/8 below
    Co / 4 + 2 <= 66, n . dn a multiple of 1/16 below 66 E, n (n . dn) a multiple of 1/32 below
    66 E: at most 66 * 1024 * 32 < 2^22 units, every partial sum exact in f32 in any order."""
    g = gen(5500 + 11 * R + 7 * Co + E + seed + (0 if orient == "img" else 1))
    shape, sr, sc = ((R, Co), Co, 1) if orient == "img" else ((Co, R), 1, R)
    return dict(dlogits=pow2_entries(shape, g, 2, 2), sr=sr, sc=sc,
                other_n=pow2_entries((Co, E), g, 0, 1), self_n=pow2_entries((R, E), g, 0, 1),
                norms=torch.exp2(torch.randint(-2, 3, (R,), generator=g).float()),
                ls=torch.zeros(1),
                dn_ext=torch.randint(-8, 9, (R, E), generator=g).float() / 4 if ext else None)


def featgrad_ref(dlogits, sr, sc, other_n, self_n, norms, ls, dn_ext):
    """dF[r] = (dn - n (n . dn)) / norm[r], dn = exp(ls) sum_c dlog(r, c) other_n[c] + dn_ext[r]:
    the backward of f -> f / |f| followed by the logit product."""
    R, Co = self_n.shape[0], other_n.shape[0]
    d = dlog_view(dlogits, R, Co, sr, sc).to(F64)
    n = self_n.to(F64)
    dn = ls.to(F64).exp() * (d @ other_n.to(F64))
    if dn_ext is not None:
        dn = dn + dn_ext.to(F64)
    return (dn - n * (n * dn).sum(-1, keepdim=True)) / norms.to(F64)[:, None]


def featgrad_bound(dlogits, sr, sc, other_n, self_n, norms, ls, dn_ext):
    """Bound of dF for either kernel of lc_head_feat_grad (the depths of the module docstring)."""
    R, E = self_n.shape
    Co = other_n.shape[0]
    d = dlog_view(dlogits, R, Co, sr, sc).to(F64)
    o, n = other_n.to(F64), self_n.to(F64)
    depth = max(cdiv(Co, 4) + 4, cdiv(Co, 8) + 8)
    g = depth * U / (1 - depth * U)
    acc = V(d @ o, g * (d.abs() @ o.abs()) + ETA * Co)
    s = vexpf(V(ls.to(F64)))
    dn = vmul(acc, V(s.v.expand(R, E), s.e.expand(R, E)))
    if dn_ext is not None:
        dn = vadd(dn, V(dn_ext.to(F64)))
    N = V(n)
    nd = vsum(vmul(dn, N), -1, 13, keepdim=True)
    inv = vdiv(V(torch.ones(R, 1, dtype=F64)), V(norms.to(F64)[:, None]))
    out = vmul(vsub(dn, vmul(N, V(nd.v.expand(R, E), nd.e.expand(R, E)))),
               V(inv.v.expand(R, E), inv.e.expand(R, E)))
    return out.e


def featgrad_f32(dlogits, sr, sc, other_n, self_n, norms, ls, dn_ext, variant=None):
    R, Co = self_n.shape[0], other_n.shape[0]
    if variant == "strides_swapped":
        sr, sc = sc, sr
    d = dlog_view(dlogits, R, Co, sr, sc).float()
    s = ls.float().exp()
    if variant == "scale_twice":
        s = s * s
    dn = s * (d @ other_n.float())
    if dn_ext is not None and variant != "dn_ext_ignored":
        dn = dn + dn_ext.float()
    n = self_n.float()
    proj = 0 if variant == "no_projection" else n * (n * dn).sum(-1, keepdim=True)
    return (dn - proj) / norms.float()[:, None]


FEATGRAD_VARIANTS = ("dn_ext_ignored", "no_projection", "strides_swapped", "scale_twice")
# (R, Co, E, orient): square, so that swapped strides stay inside the buffer
FEATGRAD_CPU_CASES = ((5, 5, 37, "img"), (5, 5, 512, "txt"), (9, 9, 4, "img"))


# --------------------------------------------------------------------------------------- AdamW
HP = dict(lr=f32r(5e-4), b1=f32r(0.9), b2=f32r(0.999), eps=f32r(1e-8), wd=f32r(1e-2))
HP_EXACT = dict(lr=2.0 ** -10, b1=0.5, b2=0.75, eps=0.0)
ADAM_STEPS = (1, 2, 3, 10, 1000, 100000)
HARD_G = (1e-20, 1e-8, 1e-4, 1.0, 1e4, 1e18)


def adamw_ref(p, g, m, v, hp, t):
    """torch.optim.AdamW's single-tensor update as adamw_kernel writes it: decoupled weight decay,
    bias-corrected moments, denominator sqrt(v / bc2) + eps. Returns (p', m', v') in float64."""
    p, g, m, v = (x.to(F64) for x in (p, g, m, v))
    lr, b1, b2, eps, wd = (hp[k] for k in ("lr", "b1", "b2", "eps", "wd"))
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    return p - (lr / bc1) * m / ((v / bc2).sqrt() + eps), m, v


def adamw_ref_steps(p, grads, hp, m=None, v=None, t0=0):
    """The trainer's rule over several gradients, in float64 with the state ROUNDED TO F32 after
    every step (what the buffers hold): a step whose gradient is not finite changes nothing,
    neither p, m, v nor the step count. Returns (p, m, v, t)."""
    m = torch.zeros_like(p) if m is None else m
    v = torch.zeros_like(p) if v is None else v
    t = t0
    for g in grads:
        if not torch.isfinite(g).all():
            continue
        t += 1
        p, m, v = (x.to(F32) for x in adamw_ref(p, g, m, v, hp, t))
    return p, m, v, t


def k_bc(b, t):
    bt = b ** t
    return 2 * bt / (1 - bt)


def adamw_bounds(p, g, m, v, hp, t):
    """Bounds of (p', m', v'). The bias corrections 1 - powf(b, t) carry (K_bc(t) + 1) u relative
    (module docstring); the one in the denominator is halved by the square root in vsqrt."""
    sc = lambda x, e=0.0: V(torch.full_like(p, x, dtype=F64), torch.full_like(p, e, dtype=F64))
    P, G, M, Vv = (V(x.to(F64)) for x in (p, g, m, v))
    lr, b1, b2, eps, wd = (sc(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    one = sc(1.0)
    pi = vmul(P, vsub(one, vmul(lr, wd)))
    mi = vadd(vmul(b1, M), vmul(vsub(one, b1), G))
    vi = vadd(vmul(b2, Vv), vmul(vmul(vsub(one, b2), G), G))
    bc = []
    for b in (hp["b1"], hp["b2"]):
        val = 1 - b ** t
        bc.append(sc(val, (k_bc(b, t) + 1) * U * val))
    denom = vadd(vsqrt(vdiv(vi, bc[1])), eps)
    upd = vdiv(vmul(vdiv(lr, bc[0]), mi), denom)
    return vsub(pi, upd).e, mi.e, vi.e


def adamw_f32(p, g, m, v, hp, t, variant=None):
    f = lambda x: torch.tensor(x, dtype=F32)
    lr, b1, b2, eps, wd = (f(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    p, g, m, v = p.float(), g.float(), m.float(), v.float()
    if variant == "wd_coupled":
        g = g + wd * p
    else:
        p = p * (1 - lr * wd)
    m = (b2 if variant == "m_uses_b2" else b1) * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    tt = f(float(t + 1 if variant == "step_off_by_one" else t))
    bc1, bc2 = 1 - torch.pow(b1, tt), 1 - torch.pow(b2, tt)
    if variant == "eps_inside_sqrt":
        denom = (v / bc2 + eps).sqrt()
    elif variant == "bc2_outside_sqrt":
        denom = v.sqrt() / bc2 + eps
    else:
        denom = (v / bc2).sqrt() + eps
    return p - (lr / bc1) * m / denom, m, v


ADAMW_VARIANTS = ("eps_inside_sqrt", "bc2_outside_sqrt", "wd_coupled", "step_off_by_one",
                  "m_uses_b2")


@functools.lru_cache(maxsize=None)
def adamw_case(n, warm, seed=0):
    """(p, g, m, v) f32. warm: the state after three float64-reference steps on random gradients
    (rounded to f32), else zero state. Hard elements, as far as n holds them: p = 0 on the first
    min(n, 256) / 2 elements (the result IS the update); from the end backwards g = 0 on two
    elements, then |g| in HARD_G with both signs (g^2 (1 - b2) = 1e-43 is subnormal, 1e-16 sits
    at eps^2, 1e36 / bc2 is near the top of f32). The last element is always a hard one (the
    grid-stride tail). Cached: callers copy before they write."""
    g_ = gen(6000 + n + seed + (1 if warm else 0))
    p = torch.randn(n, generator=g_)
    m, v = torch.zeros(n), torch.zeros(n)
    if warm:
        p, m, v, _ = adamw_ref_steps(p, [torch.randn(n, generator=g_) for _ in range(3)], HP)
    g = torch.randn(n, generator=g_)
    p[:min(n, 256) // 2] = 0
    hard = [0.0, 0.0] + [s * a for a in HARD_G for s in (1.0, -1.0)]
    for i, val in enumerate(hard[:max(n - 1, 1)]):
        g[n - 1 - i] = val
    return p, g, m, v


def adamw_exact_case(n, wd, seed=0):
    """b1 = 1/2, b2 = 3/4, lr = 2^-10, eps = 0, m = v = 0, g = +-2^k (|k| <= 20), p multiples of
    2^-10 below 1: after step 1, m' = g / 2, v' = g^2 / 4 (powers of two), bc1 = 1/2, bc2 = 1/4,
    sqrt(v' / bc2) = |g|, (lr / bc1) m' / |g| = 2^-10 sign(g), and p (1 - lr wd) is a multiple of
    2^-23 below 1 for wd in {0, 1/8} (1 - 2^-13 has 13 bits, p at most 10), the difference a
    multiple of 2^-23 below 1 + 2^-10 < 2: every operation is exact, and
    p' = p (1 - lr wd) - 2^-10 sign(g)."""
    g_ = gen(6500 + n + seed)
    p = torch.randint(-1023, 1024, (n,), generator=g_).float() / 1024
    sgn = torch.randint(0, 2, (n,), generator=g_).float() * 2 - 1
    g = sgn * torch.exp2(torch.randint(-20, 21, (n,), generator=g_).float())
    hp = dict(HP_EXACT, wd=wd)
    want = ((p.double() * (1 - hp["lr"] * wd) - hp["lr"] * sgn.double()).to(F32),
            g / 2, g * g / 4)
    return p, g, hp, want


# ----------------------------------------------------------------------------------- loss scale
POW2_MAX = (2.0 ** -140, 2.0 ** -126, 2.0 ** -120, f32r(3e-4), 1.0, 2.0 ** 100, 1.5 * 2.0 ** 127)
POW2_N = (1, 3, 4, 5, 1023, 1024 * 4 + 3, 10 * 512)
POW2_TARGETS = (-100, 10, 100)


def floor_log2(a):
    """floor(log2 a) of a positive finite double, subnormal f32 values included."""
    mant, ex = math.frexp(a)     # a = mant 2^ex, mant in [0.5, 1)
    return ex - 1


def pow2_scale_ref(x, target):
    """s = 2^k, k = clamp(target - floor(log2 max|x|), -126, 127), the maximum over the elements
    that are not NaN; s = 1 when that maximum is 0 or infinite (or every element is NaN)."""
    a = x.to(F64).abs()
    a = a[~torch.isnan(a)]
    amax = float(a.max()) if a.numel() else 0.0
    if amax == 0.0 or math.isinf(amax):
        return 1.0
    return 2.0 ** min(max(target - floor_log2(amax), K_MIN), K_MAX)


def pow2_case(n, amax, seed=0):
    """x[i] = +-amax j_i / 512 with integers j_i in [2, 512] (a dynamic range of 2^8, so that no
    element underflows where the maximum does not: x s and the way back are exact), the maximum
    itself at the LAST index (the scalar tail when n % 4 != 0)."""
    g = gen(7000 + n + seed)
    j = torch.randint(2, 513, (n,), generator=g).double()
    j[-1] = 512
    sgn = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (sgn * j / 512 * amax).to(F32)


# ------------------------------------------------------------------------------ source constants
def parse_source():
    """The limits this module quotes, as head.hip / peft.hip state them."""
    with open(os.path.join(CSRC, "head.hip")) as f:
        head = f.read()
    with open(os.path.join(CSRC, "peft.hip")) as f:
        peft = f.read()
    ints = lambda pat, txt: [int(x) for x in re.findall(pat, txt)]
    return dict(
        c_max=ints(r"C <= (\d+)", head), e_max=ints(r"E <= (\d+)\)", head),
        lds=re.findall(r"shm = \(size_t\)\(E \+ C\) \* sizeof\(float\)", head),
        target=[int(x) for x in re.findall(r"target_exp [<>]= (-?\d+)", head)],
        normalize_threads=ints(r"grad_pow2_normalize_kernel, dim3\(1\), dim3\((\d+)\)", head),
        normalize_bounds=ints(r"__launch_bounds__\((\d+)\)\s*grad_pow2_normalize_kernel", head),
        k_clamp=[int(x) for x in re.findall(r"min\(max\(target - e, (-?\d+)\), (\d+)\)", head)[0]],
        featgrad_route=re.findall(r"const bool v4 = E % 4 == 0 && \(\(\(uintptr_t\)other_n \| "
                                  r"\(uintptr_t\)self_n \| \(uintptr_t\)dF \|\s*\(uintptr_t\)dn_ext\)"
                                  r" & 15\) == 0;", head),
        normalize_route=re.findall(r"const bool v4 = \(\(uintptr_t\)x & 15\) == 0;", head),
        ctr_max=ints(r"n > 0 && n <= (\d+) && ctr != nullptr", peft),
        grid_cap=ints(r"if \(gsz > (\d+)\) gsz = \1;", peft),
        tail_block=ints(r"(?:finite_kernel|adamw_kernel), dim3\(grid_for\(n, (\d+)\)\), dim3\(\1\)",
                        peft),
        adamw_step_rule=re.findall(r"n >= 0 && \(step >= 1 \|\| step_dev != nullptr\)", peft),
    )
