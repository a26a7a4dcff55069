"""The long attention family of csrc/attention.hip (257 <= L <= 512: attn_long_fwd_kernel,
attn_long_bwd_kv_kernel, attn_long_bwd_q_kernel, reached through ops.attn_fwd / ops.attn_bwd) on
the MI355X: the five families of test_attention_gpu.py with its helpers and bounds, the yardsticks
of tests/attn_cases.py and the 16-bit one-hot case of tests/attn_long_cases.py (premises on the
CPU: test_attention_long_cases.py). Every chunk count NCH = ceil(L / 32) = 9..16, both storage
types (torch.float16 reaches the _f16 symbols). The family has one backward form.

  A  one-hot attention: O and dv are the exact integers, no tolerance; dq, dk vanish
  B  uniform attention: an integer sum over the allowed-key count at every mask edge
  C  random data: the derived per-element forward bound, and per-row backward errors within twice
     those of an fp64 arithmetic that rounds only where the kernels round
  D  strided views inside NaN-poisoned / sentinel-filled buffers: same bits, nothing else written
  E  more workgroups than CUs: the bits of the same inputs run as two smaller launches

Measured kernel / emulation ratios of C (MI355X) are in profiles/vit_l14/README.md.
"""
import pytest
import torch

import attn_cases as ac
import attn_long_cases as alc
from test_attention_gpu import (DTYPES, HF, assert_exact, check_lse, check_rows, grads, guarded_in,
                                guarded_out, ops, run_fwd, same_bits, sentinel_intact, GUARD)  # noqa: F401

pytestmark = pytest.mark.gpu


def run_bwd(ops, qkv, O, dO, lse, n, L, H, causal):
    dqkv = torch.full((n * L, 3 * H * 64), float("nan"), device=qkv.device, dtype=qkv.dtype)
    ops.attn_bwd(qkv, O, dO, lse, dqkv, n, L, H, causal)
    return dqkv


# ----------------------------------------------------------------------- A: exact one-hot cases
@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", alc.L_SWEEP)
def test_one_hot_exact(ops, dev, dtype, L, causal):
    """attn_long_cases.one_hot_case: p is exactly 1 on the target key and exactly 0 off it
    (exp2(-184.7) in f32), so O = v[pi] and dv = index_add(pi, dO) exactly and lse = 8 * 128 *
    log2(e); dS is p (dP - Delta), 0 on target (dP and Delta are the same small integers) and 0
    off it, so |dq|, |dk| <= 2^-20 with room to spare. pi puts the dominant key in any of the
    9..16 chunks, before or after the query's: a chunk walk (w, w + 8), row / key index, swizzle,
    staging-pass, transposed-read or online-rescale error fails exactly."""
    n, H = 3, 2
    qkv, dO, pi = alc.one_hot_case(L, causal, 1000 + L, n, H)
    qkv, dO = qkv.to(dev, dtype), dO.to(dev, dtype)
    want_O, want_dv = (x.to(dtype) for x in ac.one_hot_expected(qkv, dO, pi))
    O, lse = run_fwd(ops, qkv, n, L, H, causal)
    assert_exact(ac.heads(O, n, L, H), want_O, "O")
    assert torch.allclose(lse, torch.full_like(lse, 8 * alc.QSCALE * ac.LOG2E), rtol=1e-6, atol=0)
    dq, dk, dv = grads(run_bwd(ops, qkv, O, dO, lse, n, L, H, causal), n, L, H)
    assert_exact(dv, want_dv, "dv")
    assert (dq.abs() <= 2.0 ** -20).all()
    assert (dk.abs() <= 2.0 ** -20).all()


# ----------------------------------------------------------------------- B: uniform attention
@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", alc.L_SWEEP)
def test_uniform_every_mask_edge(ops, dev, dtype, L, causal):
    """uniform_case (q = 0): O[q] within one storage ulp of the fp64 mean of the allowed keys' v
    and lse = log2(cnt) to 1e-6 (relative; absolute below 1), at every row of every chunk."""
    n, H = 3, 2
    qkv = ac.uniform_case(L, 2000 + L, n, H).to(dev, dtype)
    want_O, want_lse = ac.uniform_expected(qkv, n, L, H, causal)
    O, lse = run_fwd(ops, qkv, n, L, H, causal)
    assert ac.ulp_diff(ac.heads(O, n, L, H), want_O.to(dtype)).max().item() <= 1
    err = (lse.reshape(n, H, L).double() - want_lse).abs()
    assert (err <= 1e-6 * want_lse.clamp_min(1.0)).all()


# ------------------------------------------------------- C: per-element / per-row, random data
@DTYPES
@pytest.mark.parametrize("L,causal", [(257, False), (277, False), (289, True), (400, False),
                                      (512, True)])
def test_random_bounds(ops, dev, dtype, L, causal):
    """1.5 * randn inputs against ref_attention64 on the same rounded inputs. Forward: every
    element inside attn_cases.fwd_bound, lse to 1e-5. Backward: check_rows (kernel row error
    <= 2 x the emulation's, per tensor; the ratios are printed)."""
    n, H = 2, 3
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, 3000 + L, n, H, dev))
    ref = ac.ref_attention64(qkv, dO, n, L, H, causal)
    emu = ac.emulate(qkv, dO, n, L, H, causal, dtype)
    O, lse = run_fwd(ops, qkv, n, L, H, causal)
    over = (ac.heads(O, n, L, H).double() - ref.O).abs() / ac.fwd_bound(ref, qkv, n, L, H, dtype)
    assert over.max().item() <= 1.0  # NaN fails too
    check_lse(lse, ref, n, H, L)
    got = grads(run_bwd(ops, qkv, O, dO, lse, n, L, H, causal), n, L, H)
    check_rows(got, ref[3:], emu[3:], f"{'f16' if dtype == HF else 'bf16'} L={L} long")


# --------------------------------------------------- D: strided, poisoned and guarded buffers
@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [257, 300, 512])
def test_strided_guarded_buffers(ops, dev, dtype, L, causal):
    """qkv, O, dO, dqkv as views of row stride cols + 8 and cols + 64 with 64 guard rows before
    and after (inputs NaN there, outputs a sentinel): the contiguous call's bits (lse too), every
    sentinel intact, no NaN."""
    n, H = 3, 2
    D = H * 64
    M = n * L
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, 4000 + L, n, H, dev))
    O, lse = run_fwd(ops, qkv, n, L, H, causal)
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    base = run_bwd(ops, qkv, O, dO, lse, n, L, H, causal)
    assert torch.isfinite(base.float()).all()
    for pad in (8, 64):
        qkv_s = guarded_in(qkv, pad)
        O_buf, O_s = guarded_out(M, D, pad, dtype, dev)
        lse_buf = torch.full((n * H * L + 2 * GUARD,), -7.0, device=dev)
        lse_s = lse_buf[GUARD:GUARD + n * H * L].view(n * H, L)
        ops.attn_fwd(qkv_s, O_s, lse_s, n, L, H, causal)
        assert same_bits(O_s, O), pad
        assert torch.equal(lse_s, lse), pad
        assert sentinel_intact(O_buf, M, D), pad
        assert (lse_buf[:GUARD] == -7.0).all() and (lse_buf[-GUARD:] == -7.0).all(), pad
        O_in, dO_s = guarded_in(O, pad), guarded_in(dO, pad)
        g_buf, g_s = guarded_out(M, 3 * D, pad, dtype, dev)
        ops.attn_bwd(qkv_s, O_in, dO_s, lse_s, g_s, n, L, H, causal)
        assert same_bits(g_s, base), pad
        assert sentinel_intact(g_buf, M, 3 * D), pad


# ------------------------------------------------------------------- E: more items than CUs
@DTYPES
def test_more_workgroups_than_cus(ops, dev, dtype):
    """n = 24, H = 16, L = 257: 384 workgroups, one per CU at a time (LDS), so workgroups follow
    one another on a CU. Forward and backward give the bits of the same inputs run as two
    launches of 12 sequences."""
    n, H, L = 24, 16, 257
    assert n * H > ops.device_cu_count(dev)
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, 5000 + L, n, H, dev))
    O, lse = run_fwd(ops, qkv, n, L, H, False)
    big = run_bwd(ops, qkv, O, dO, lse, n, L, H, False)
    assert torch.isfinite(O.float()).all() and torch.isfinite(big.float()).all()
    h = n // 2
    for s0 in (0, h):
        r = slice(s0 * L, (s0 + h) * L)
        O_p, lse_p = run_fwd(ops, qkv[r], h, L, H, False)
        assert same_bits(O_p, O[r]) and torch.equal(lse_p, lse[s0 * H:(s0 + h) * H]), s0
        part = run_bwd(ops, qkv[r], O[r], dO[r], lse[s0 * H:(s0 + h) * H], h, L, H, False)
        assert same_bits(part, big[r]), s0
