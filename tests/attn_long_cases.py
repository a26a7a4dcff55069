"""The one-hot attention case for 257 <= L <= 512 (the long kernel family of csrc/attention.hip),
beside tests/attn_cases.py, whose one_hot_case stops at 256 keys (8 index bits). Pure torch.

Everything else of attn_cases — ref_attention64, emulate, fwd_bound, row_err, the uniform and
random cases, one_hot_expected — takes any length and is used as it is.
"""
import torch

import attn_cases as ac

# every chunk count NCH = ceil(L / 32) = 9..16 at its first length, 9's inner lengths and last
# length, MVP's 277 (257 + 20 prompt rows), and 16's last
L_SWEEP = (257, 273, 277, 288, 289, 320, 321, 353, 384, 385, 417, 449, 480, 481, 512)

# One query scale for both storage types: the on-target raw score 64 * 128 = 8192 is a power of
# two, so score * c and the running max are exact in f32 and p is exactly 1; one differing index
# bit flips 4 columns, 2 * 4 * 128 = 1024 raw = 128 nats, so the off-target p is exp2(-184.7),
# zero in f32 (and in bfloat16, which has f32's exponent range: attn_cases.ONE_HOT_QSCALE).
QSCALE = 128


def one_hot_case(L, causal, seed, n=3, H=2):
    """attn_cases.one_hot_case with 16 index bits: k_j = the 16 bits of j as +-1, tiled 4 times
    to 64 columns (the same in every head), q_i = QSCALE * k_pi(i) with pi a random permutation
    (causal: pi(i) uniform in [0, i]) drawn per (sequence, head); v and dO integers in [-3, 3].
    The raw score q_i . k_j is 64 QSCALE - 8 QSCALE hamming(pi(i), j).
    Returns f32 qkv [n*L, 3*H*64], dO [n*L, H*64] (exact in either storage type) and pi [n, H, L].
    """
    assert L <= 512
    g = torch.Generator().manual_seed(seed)
    bits = ((torch.arange(L)[:, None] >> torch.arange(16)) & 1).float() * 2 - 1  # [L, 16]
    k = bits.repeat(1, 4)                                                        # [L, 64]
    if causal:
        pi = (torch.rand(n, H, L, generator=g) * torch.arange(1, L + 1)).long()
        pi = torch.minimum(pi, torch.arange(L))
    else:
        pi = torch.stack([torch.randperm(L, generator=g) for _ in range(n * H)]).reshape(n, H, L)
    q = QSCALE * k[pi]                                                           # [n, H, L, 64]
    kk = k.expand(n, H, L, 64)
    v = ac.heads(ac._int_rows(g, n, L, H), n, L, H)
    qkv = torch.cat([ac.rows(q), ac.rows(kk), ac.rows(v)], dim=1)
    return qkv, ac._int_rows(g, n, L, H), pi
