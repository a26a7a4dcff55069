"""Attention test cases and yardsticks shared by test_attention_cases.py (CPU) and
test_attention_gpu.py (the HIP kernels of csrc/attention.hip). Pure torch, importable without a
GPU; every function runs on the device of its inputs.

Layouts are the kernels': qkv = [n*L, 3*H*64] (q | k | v, head h at columns h*64), O / dO =
[n*L, H*64], lse = [n*H, L] in the log2 domain. The references return per-head tensors
[n, H, L, 64] (heads() converts a kernel output), so a "row" below is one (sequence, head, row).

  ref_attention64   fp64 forward + backward of the operation on the given (16-bit-rounded) inputs
  emulate           the same with the kernels' documented rounding points restated, nothing else
                    changed: the yardstick a kernel's distance from fp64 is measured against
  one_hot_case      inputs whose softmax is exactly one-hot in the kernels' f32 arithmetic
  uniform_case      q = 0: every allowed key weighs 1 / cnt
  row_err           worst row of got against ref

Unit roundoff u of a storage type as the bounds use it: 2^-8 bfloat16, 2^-11 float16 (one ulp of
a value in [1, 2) is 2u: |round(x) - x| <= u |x| with room to spare).
"""
import math
from collections import namedtuple

import torch

LOG2E = 1.0 / math.log(2.0)
SCALE = 0.125  # 64^-0.5
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# every tile count NQB = ceil(L / 32) = 1..8 at its first, an inner and its last length
L_SWEEP = (1, 16, 17, 32, 33, 50, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 197, 224, 225, 256)

# one_hot_case's query scale per storage type. At 16 (on-target raw score 1024) the off-target
# softmax mass is 2^-43: float16 rounds it to zero, but bfloat16 has f32's exponent range, so
# wherever the exact answer is 0 (v_pi(i) = 0, a key no query targets) even the fp64 result rounds
# to a non-zero bfloat16 of about 1e-13 and no kernel can match the integers bit for bit. At 64
# (on-target 4096, still a power of two) the off-target p is exp2(-184): zero in f32.
ONE_HOT_QSCALE = {torch.float16: 16, torch.bfloat16: 64}

Attn = namedtuple("Attn", "O lse P dq dk dv")


def heads(x, n, L, H):
    """[n*L, H*64] (rows of any stride) -> [n, H, L, 64]."""
    return x.reshape(n, L, H, 64).permute(0, 2, 1, 3)


def rows(x):
    """[n, H, L, 64] -> [n*L, H*64] contiguous."""
    n, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(n * L, H * 64).contiguous()


def split_qkv(qkv, n, L, H):
    """[n*L, 3*H*64] -> q, k, v as fp64 [n, H, L, 64]."""
    t = qkv.double().reshape(n, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def allowed(L, causal, device=None):
    """[L, L] bool: query row i may see key column j."""
    m = torch.ones(L, L, dtype=torch.bool, device=device)
    return m.tril_() if causal else m


def _softmax_parts(q, k, L, causal):
    s = (q @ k.transpose(-1, -2)) * SCALE
    s = s.masked_fill(~allowed(L, causal, s.device), float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)  # unnormalised, max 1 per row
    return m, p, p.sum(-1, keepdim=True)


def ref_attention64(qkv, dO, n, L, H, causal):
    """fp64 attention forward and backward on the inputs as given (pass the 16-bit-rounded
    tensors the kernel sees). Returns Attn(O, lse, P, dq, dk, dv): [n, H, L, 64] each, lse
    [n, H, L] in the log2 domain, P [n, H, L, L]."""
    q, k, v = split_qkv(qkv, n, L, H)
    do = heads(dO.double(), n, L, H)
    m, p, l = _softmax_parts(q, k, L, causal)
    P = p / l
    O = P @ v
    lse = ((m + torch.log(l)) * LOG2E).squeeze(-1)
    dv = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dq = (dS @ k) * SCALE
    dk = (dS.transpose(-1, -2) @ q) * SCALE
    return Attn(O, lse, P, dq, dk, dv)


def emulate(qkv, dO, n, L, H, causal, dtype):
    """ref_attention64 with the kernels' documented rounding points (csrc/attention.hip) and
    nothing else changed; every product and sum stays fp64:
      forward   the unnormalised p = exp(s - max) is rounded to the storage type for the P V
                product, the row sum is taken from the unrounded p, O is rounded when stored;
      backward  P = exp2(s c - lse) (unrounded) is rounded for P^T dO, Delta = rowsum(dO * stored
                O), dS = P (dP - Delta) is rounded for dS K and dS^T Q, dq / dk / dv are rounded
                when stored.
    A yardstick for measured bounds, not code under test."""
    def rt(x):
        return x.to(dtype).double()

    q, k, v = split_qkv(qkv, n, L, H)
    do = heads(dO.double(), n, L, H)
    m, p, l = _softmax_parts(q, k, L, causal)
    O = rt((rt(p) @ v) / l)
    lse = ((m + torch.log(l)) * LOG2E).squeeze(-1)
    P = p / l
    dv = rt(rt(P).transpose(-1, -2) @ do)
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = rt(P * (dP - delta))
    dq = rt((dS @ k) * SCALE)
    dk = rt((dS.transpose(-1, -2) @ q) * SCALE)
    return Attn(O, lse, P, dq, dk, dv)


def grads_in_chunks(fn, qkv, dO, n, L, H, causal, chunk, **kw):
    """(dq, dk, dv) of fn (ref_attention64 / emulate) evaluated `chunk` sequences at a time: the
    fp64 score tensor of a large launch does not have to exist at once."""
    D = H * 64
    out = [[], [], []]
    for s0 in range(0, n, chunk):
        s1 = min(n, s0 + chunk)
        r = fn(qkv[s0 * L:s1 * L, :3 * D], dO[s0 * L:s1 * L, :D], s1 - s0, L, H, causal, **kw)
        for acc, x in zip(out, (r.dq, r.dk, r.dv)):
            acc.append(x)
    return tuple(torch.cat(acc) for acc in out)


def fwd_bound(ref, qkv, n, L, H, dtype):
    """Per-element forward bound |O - O64| <= 2.5 u (P64 |v|) + 1e-6: one u from rounding P to
    the storage type, one u from rounding O, a quarter on top for f32 summation order and the
    hardware exp2 / log2."""
    v = split_qkv(qkv, n, L, H)[2]
    return 2.5 * UNIT_ROUNDOFF[dtype] * (ref.P @ v.abs()) + 1e-6


def row_err(got, ref):
    """max over rows of ||got_row - ref_row|| / max(||ref_row||, median row norm of ref); got and
    ref [..., 64], every leading index (sequence, head, row) a row."""
    got, ref = got.double(), ref.double()
    rn = ref.norm(dim=-1)
    return ((got - ref).norm(dim=-1) / torch.maximum(rn, rn.median())).max().item()


def ulp_diff(a, b):
    """Element-wise distance of two 16-bit float tensors of one type in units in the last place
    (integer bit patterns on the sign-magnitude line; +0 and -0 coincide)."""
    def line(x):
        i = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


def _int_rows(g, n, L, H):
    return torch.randint(-3, 4, (n * L, H * 64), generator=g).float()


def one_hot_case(L, causal, seed, n=3, H=2, qscale=16):
    """Inputs whose attention is a gather: k_j = the 8 bits of j as +-1, tiled 8 times to 64
    columns (the same in every head), q_i = qscale * k_pi(i) with pi a random permutation
    (causal: pi(i) uniform in [0, i]) drawn per (sequence, head); v and dO integers in [-3, 3],
    different per head and sequence. The raw score q_i . k_j is 64 qscale - 16 qscale hamming(
    pi(i), j): on target 64 qscale, a power of two, so score * c and the running max are exact in
    f32 and p is exactly 1; off target at most 48 qscale, i.e. 2 qscale nats below.
    Returns f32 qkv [n*L, 3*H*64], dO [n*L, H*64] (exact in either storage type) and pi [n, H, L].
    """
    assert L <= 256
    g = torch.Generator().manual_seed(seed)
    bits = ((torch.arange(L)[:, None] >> torch.arange(8)) & 1).float() * 2 - 1  # [L, 8]
    k = bits.repeat(1, 8)                                                       # [L, 64]
    if causal:
        pi = (torch.rand(n, H, L, generator=g) * torch.arange(1, L + 1)).long()
        pi = torch.minimum(pi, torch.arange(L))
    else:
        pi = torch.stack([torch.randperm(L, generator=g) for _ in range(n * H)]).reshape(n, H, L)
    q = qscale * k[pi]                                                          # [n, H, L, 64]
    kk = k.expand(n, H, L, 64)
    v = heads(_int_rows(g, n, L, H), n, L, H)
    qkv = torch.cat([rows(q), rows(kk), rows(v)], dim=1)
    return qkv, _int_rows(g, n, L, H), pi


def one_hot_expected(qkv, dO, pi):
    """(O, dv) of a one_hot_case as exact integers, [n, H, L, 64]: O_i = v_pi(i), dv_j = the sum
    of dO_i over the queries i with pi(i) = j."""
    n, H, L = pi.shape
    v = split_qkv(qkv, n, L, H)[2]
    do = heads(dO.double(), n, L, H)
    idx = pi.to(v.device)[..., None].expand(n, H, L, 64)
    return v.gather(2, idx), torch.zeros_like(do).scatter_add_(2, idx, do)


def uniform_case(L, seed, n=3, H=2):
    """q = 0 (every allowed key weighs 1 / cnt), k random, v integers in [-3, 3]: O is the mean
    of the allowed keys' v, an integer sum over a count. Returns f32 qkv [n*L, 3*H*64]."""
    g = torch.Generator().manual_seed(seed)
    D = H * 64
    k = 1.5 * torch.randn(n * L, D, generator=g)
    return torch.cat([torch.zeros(n * L, D), k, _int_rows(g, n, L, H)], dim=1)


def uniform_expected(qkv, n, L, H, causal):
    """(O, lse) of a uniform_case in fp64: the integer sum of the allowed keys' v over their count
    (an exact 0 where the sum cancels, which P @ v in fp64 is not), and log2(cnt)."""
    v = split_qkv(qkv, n, L, H)[2]
    ok = allowed(L, causal, v.device).double()
    cnt = ok.sum(-1, keepdim=True)
    return (ok @ v) / cnt, torch.log2(cnt).squeeze(-1).expand(n, H, L)


def random_case(L, seed, n, H, device=None):
    """1.5 * randn qkv and randn dO (f32; round them to the storage type under test)."""
    g = torch.Generator(device=device).manual_seed(seed)
    qkv = 1.5 * torch.randn(n * L, 3 * H * 64, generator=g, device=device)
    return qkv, torch.randn(n * L, H * 64, generator=g, device=device)
