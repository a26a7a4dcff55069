"""The conditions test_attention_long_gpu.py leans on, shown on the references alone (no GPU), as
test_attention_cases.py does for the lengths up to 256: attn_long_cases.one_hot_case really is
exact in fp64 at query scale 128 in both storage types, and the yardsticks of attn_cases hold at
the long family's lengths."""
import pytest
import torch

import attn_cases as ac
import attn_long_cases as alc

DTYPES = (torch.bfloat16, torch.float16)
N, H = 3, 2


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", alc.L_SWEEP)
def test_one_hot_off_target_mass(L, causal):
    """Per row, the fp64 softmax of the 16-bit one_hot_case leaves nothing off the target key
    that fp64 can see next to 1 (exp(-128) per key), the inputs are exact in either storage type,
    the fp64 O and dv rounded to the storage type are the exact integers v[pi] /
    index_add(pi, dO) with |dv| <= 256 (integers both types hold), lse is 8 * 128 * log2(e), and
    |dq|, |dk| stay under 2^-20."""
    qkv, dO, pi = alc.one_hot_case(L, causal, 1000 + L, N, H)
    for dtype in DTYPES:
        assert torch.equal(qkv.to(dtype).float(), qkv) and torch.equal(dO.to(dtype).float(), dO)
    if causal:
        assert (pi <= torch.arange(L)).all()
    else:
        assert torch.equal(pi.sort(-1).values, torch.arange(L).expand(N, H, L))
    r = ac.ref_attention64(qkv, dO, N, L, H, causal)
    on = r.P.gather(3, pi[..., None]).squeeze(-1)
    assert (1 - on).max().item() < 2.0 ** -36
    off = r.P.scatter(3, pi[..., None], 0.0)
    assert off.max().item() < 2.0 ** -150  # below f32's smallest denormal: p is 0 in the kernels
    want_O, want_dv = ac.one_hot_expected(qkv, dO, pi)
    assert want_dv.abs().max() <= 256
    for dtype in DTYPES:
        assert torch.equal(r.O.to(dtype), want_O.to(dtype))
        assert torch.equal(r.dv.to(dtype), want_dv.to(dtype))
    assert torch.allclose(r.lse, torch.full_like(r.lse, 8 * alc.QSCALE * ac.LOG2E),
                          rtol=1e-12, atol=0)
    assert r.dq.abs().max() <= 2.0 ** -20 and r.dk.abs().max() <= 2.0 ** -20


def test_one_hot_scores_are_exact_in_f32():
    """The on-target raw score is 8192, a power of two, and every score is a multiple of 1024
    between -8192 and 8192: exact in f32, so the kernels' max and score * c carry no rounding of
    the score itself; one differing bit costs 1024 raw = 128 nats."""
    qkv, _, pi = alc.one_hot_case(512, False, 1512, 1, 1)
    q, k, _ = ac.split_qkv(qkv, 1, 512, 1)
    s = (q @ k.transpose(-1, -2))[0, 0]
    assert torch.equal(s.float().double(), s)
    assert torch.equal(s.gather(1, pi[0, 0][:, None]).squeeze(1), torch.full((512,), 8192.0).double())
    assert torch.equal(s % 1024, torch.zeros_like(s))
    assert s.scatter(1, pi[0, 0][:, None], -1e9).max().item() == 8192 - 1024
    assert 1024 * ac.SCALE == 128


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("L,causal", [(257, False), (289, True), (512, True)])
def test_emulation_inside_forward_bound(L, causal, dtype):
    """emulate() stays inside attn_cases.fwd_bound on 1.5 * randn inputs at the long family's
    lengths too, its lse is the reference's, and the backward yardstick is a rounding-sized
    distance."""
    qkv, dO = ac.random_case(L, L, 2, 3)
    qkv, dO = qkv.to(dtype), dO.to(dtype)
    r = ac.ref_attention64(qkv, dO, 2, L, 3, causal)
    e = ac.emulate(qkv, dO, 2, L, 3, causal, dtype)
    assert ((e.O - r.O).abs() <= ac.fwd_bound(r, qkv, 2, L, 3, dtype)).all()
    assert torch.equal(e.lse, r.lse)
    for name in ("dq", "dk", "dv"):
        assert 0 < ac.row_err(getattr(e, name), getattr(r, name)) < 0.1
