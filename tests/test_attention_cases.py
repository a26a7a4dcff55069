"""The conditions test_attention_gpu.py leans on, shown on the references alone (no GPU): the
constructed cases of tests/attn_cases.py really are exact in fp64, and the derived forward bound
holds for an arithmetic that rounds where the kernels round and is otherwise exact."""
import pytest
import torch

import attn_cases as ac

DTYPES = (torch.bfloat16, torch.float16)
N, H = 3, 2


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", ac.L_SWEEP)
def test_one_hot_off_target_mass(L, causal):
    """Per row, the fp64 softmax of one_hot_case leaves less than 2^-36 off the target key
    (measured 2^-43.2 at L = 256, query scale 16), the fp64 O and dv rounded to the storage type
    are the exact integers v[pi] / index_add(pi, dO), and |dq|, |dk| stay under 2^-20 — at the
    query scale each storage type is tested with."""
    for dtype in DTYPES:
        qkv, dO, pi = ac.one_hot_case(L, causal, 1000 + L, N, H, ac.ONE_HOT_QSCALE[dtype])
        assert torch.equal(qkv.to(dtype).float(), qkv) and torch.equal(dO.to(dtype).float(), dO)
        if causal:
            assert (pi <= torch.arange(L)).all()
        else:
            assert torch.equal(pi.sort(-1).values, torch.arange(L).expand(N, H, L))
        r = ac.ref_attention64(qkv, dO, N, L, H, causal)
        on = r.P.gather(3, pi[..., None]).squeeze(-1)
        assert (1 - on).max().item() < 2.0 ** -36
        want_O, want_dv = ac.one_hot_expected(qkv, dO, pi)
        assert want_dv.abs().max() <= 256  # integers the storage types hold exactly
        assert torch.equal(r.O.to(dtype), want_O.to(dtype))
        assert torch.equal(r.dv.to(dtype), want_dv.to(dtype))
        assert torch.allclose(r.lse, torch.full_like(r.lse, 8 * ac.ONE_HOT_QSCALE[dtype] * ac.LOG2E),
                              rtol=1e-12, atol=0)
        assert r.dq.abs().max() <= 2.0 ** -20 and r.dk.abs().max() <= 2.0 ** -20


def test_one_hot_scale_16_is_not_exact_in_bfloat16():
    """Why bfloat16 runs one_hot_case at query scale 64: at 16 the fp64 result itself, rounded
    to bfloat16, differs from the integers wherever they are 0 (float16 flushes the 2^-43)."""
    qkv, dO, pi = ac.one_hot_case(50, True, 1050, N, H, 16)
    r = ac.ref_attention64(qkv, dO, N, 50, H, True)
    want_O, want_dv = ac.one_hot_expected(qkv, dO, pi)
    assert not torch.equal(r.dv.to(torch.bfloat16), want_dv.to(torch.bfloat16))
    assert torch.equal(r.dv.to(torch.float16), want_dv.to(torch.float16))
    assert torch.equal(r.O.to(torch.float16), want_O.to(torch.float16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("L,causal", [(50, False), (77, True), (130, False), (197, False),
                                      (256, True)])
def test_emulation_inside_forward_bound(L, causal, dtype):
    """emulate() — P and O rounded to the storage type, everything else exact — stays inside
    |O - O64| <= 2.5 u (P64 |v|) + 1e-6 on 1.5 * randn inputs (peak 1.32 u over these lengths),
    and its lse is the reference's."""
    qkv, dO = ac.random_case(L, L, 2, 3)
    qkv, dO = qkv.to(dtype), dO.to(dtype)
    r = ac.ref_attention64(qkv, dO, 2, L, 3, causal)
    e = ac.emulate(qkv, dO, 2, L, 3, causal, dtype)
    assert ((e.O - r.O).abs() <= ac.fwd_bound(r, qkv, 2, L, 3, dtype)).all()
    assert torch.equal(e.lse, r.lse)
    # the backward yardstick is a rounding-sized distance, not zero and not a wrong row (~1)
    for name in ("dq", "dk", "dv"):
        assert 0 < ac.row_err(getattr(e, name), getattr(r, name)) < 0.1


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", ac.L_SWEEP)
def test_uniform_mean(L, causal):
    """uniform_case: the fp64 attention output is the mean of the allowed keys' v, and rounded
    to the storage type it is within one ulp of f32(sum) * f32(1 / cnt) rounded, the kernels'
    order of operations (measured 0 ulp)."""
    qkv = ac.uniform_case(L, 2000 + L, N, H)
    r = ac.ref_attention64(qkv, torch.zeros(N * L, H * 64), N, L, H, causal)
    v = ac.split_qkv(qkv, N, L, H)[2]
    cnt = ac.allowed(L, causal).sum(-1, keepdim=True).double()
    total = ac.allowed(L, causal).double() @ v
    mean, lse = ac.uniform_expected(qkv, N, L, H, causal)
    assert torch.equal(mean, total / cnt)
    assert torch.allclose(r.O, mean, rtol=1e-14, atol=1e-14)
    assert torch.allclose(r.lse, lse, rtol=1e-13, atol=1e-13)
    for dtype in DTYPES:
        f32 = total.float() * (1.0 / cnt.float())
        assert ac.ulp_diff(mean.to(dtype), f32.to(dtype)).max().item() <= 1


def test_row_err_and_ulp_diff():
    """row_err sees one wrong row among many at full size where a whole-tensor norm does not;
    ulp_diff counts representable steps across zero."""
    torch.manual_seed(0)
    ref = torch.randn(2, 12, 197, 64)
    got = ref.clone()
    got[1, 5, 100] = torch.randn(64)
    whole = ((got - ref).norm() / ref.norm()).item()
    assert whole < 2.5e-2 and ac.row_err(got, ref) > 0.5
    assert ac.row_err(ref, ref) == 0
    small = ref.clone()
    small[0, 0, 0] = 0  # a zero reference row is measured against the median row norm
    assert ac.row_err(small + 1e-3, small) < 2e-3
    for dtype in DTYPES:
        a = torch.tensor([1.0, -0.0, 0.0, 2.0], dtype=dtype)
        b = torch.tensor([1.0, 0.0, -0.0, 2.0], dtype=dtype)
        assert ac.ulp_diff(a, b).max() == 0
        nxt = (a.view(torch.int16) + 1).view(dtype)
        assert ac.ulp_diff(a, nxt).tolist() == [1, 1, 1, 1]
