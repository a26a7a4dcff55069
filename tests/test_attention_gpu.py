"""The attention kernels of csrc/attention.hip on the MI355X against the cases and yardsticks of
tests/attn_cases.py (their premises are shown on the CPU by test_attention_cases.py): every tile
count NQB = ceil(L / 32) = 1..8, every backward form, both storage types (torch.float16 reaches the
_f16 symbols), and the persistent item walk of the fused backward that the training step runs.

  A  one-hot attention: O and dv are the exact integers, no tolerance; dq, dk vanish
  B  uniform attention: an integer sum over the allowed-key count at every mask edge
  C  random data: a derived per-element forward bound, and per-row backward errors within twice
     those of an fp64 arithmetic that rounds only where the kernels round
  D  strided views inside NaN-poisoned / sentinel-filled buffers: same bits, nothing else written
  E  n_seq * H >= 4 * CUs, where a workgroup walks several items: the same bits as one item per
     workgroup, and the per-row bound of C
"""
import contextlib

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
SENTINEL = 0x5A5A  # a finite value in either storage type


@pytest.fixture(scope="module")
def ops(dev):
    from lcclip import ops as _ops
    return _ops


@contextlib.contextmanager
def bwd_form(dtype, form):
    """lc_attn_bwd_set_form[_f16](form) for the launches inside; process-wide, so restored."""
    from lcclip import _lib
    lib = _lib.load()
    set_form = lib.lc_attn_bwd_set_form_f16 if dtype == HF else lib.lc_attn_bwd_set_form
    try:
        assert set_form(form) == 0
        yield
    finally:
        set_form(0)


def forms_for(L):
    """The backward forms a length allows: the two-phase form has no 8-tile instance."""
    return (1, 2, 3) if L <= 224 else (1, 2)


def bits(x):
    return x.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def assert_exact(got, want, tag=None):
    """Every element of got is the value of want exactly (no tolerance, NaN fails). The sign of a
    zero is left free: where the exact answer is 0, a negative off-target remainder of 2^-46
    correctly rounds to -0 in float16."""
    bad = ~(got == want)
    if bad.any():
        idx = bad.nonzero()[:5].tolist()
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                             f"{idx}: got {[got[tuple(i)].item() for i in idx]}, "
                             f"want {[want[tuple(i)].item() for i in idx]}")


def run_fwd(ops, qkv, n, L, H, causal):
    O = torch.full((n * L, H * 64), float("nan"), device=qkv.device, dtype=qkv.dtype)
    lse = torch.full((n * H, L), float("nan"), device=qkv.device)
    ops.attn_fwd(qkv, O, lse, n, L, H, causal)
    return O, lse


def run_bwd(ops, qkv, O, dO, lse, n, L, H, causal, form):
    dqkv = torch.full((n * L, 3 * H * 64), float("nan"), device=qkv.device, dtype=qkv.dtype)
    with bwd_form(qkv.dtype, form):
        ops.attn_bwd(qkv, O, dO, lse, dqkv, n, L, H, causal)
    return dqkv


def grads(dqkv, n, L, H):
    """dq, dk, dv of a dqkv matrix as [n, H, L, 64]."""
    D = H * 64
    return tuple(ac.heads(dqkv[:, i * D:(i + 1) * D], n, L, H) for i in range(3))


# ----------------------------------------------------------------------- A: exact one-hot cases
@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", ac.L_SWEEP)
def test_one_hot_exact(ops, dev, dtype, L, causal):
    """one_hot_case: p is exactly 1 on the target key, so O = v[pi] and dv = index_add(pi, dO)
    exactly (assert_exact) and lse = on-target score * log2(e), in the forward and every backward
    form, at the query scale of the storage type (attn_cases.ONE_HOT_QSCALE). On
    target dS = p (dP - Delta) is exactly 0 (dP and Delta are the same small integers); off
    target it is at most 2^-43 * 1152 * 255 * 16 * 0.125 ~ 2^-24 (query scale 16; nothing at
    64), so |dq|, |dk| <= 2^-20. pi puts the dominant key in an earlier or later 32-key block at
    random: a row / key index, swizzle, transposed-read or online-rescale error fails exactly."""
    n, H = 3, 2
    qs = ac.ONE_HOT_QSCALE[dtype]
    qkv, dO, pi = ac.one_hot_case(L, causal, 1000 + L, n, H, qs)
    qkv, dO = qkv.to(dev, dtype), dO.to(dev, dtype)
    want_O, want_dv = (x.to(dtype) for x in ac.one_hot_expected(qkv, dO, pi))
    O, lse = run_fwd(ops, qkv, n, L, H, causal)
    assert_exact(ac.heads(O, n, L, H), want_O, "O")
    assert torch.allclose(lse, torch.full_like(lse, 8 * qs * ac.LOG2E), rtol=1e-6, atol=0)
    for form in forms_for(L):
        dq, dk, dv = grads(run_bwd(ops, qkv, O, dO, lse, n, L, H, causal, form), n, L, H)
        assert_exact(dv, want_dv, f"dv form {form}")
        assert (dq.abs() <= 2.0 ** -20).all(), form
        assert (dk.abs() <= 2.0 ** -20).all(), form


# ----------------------------------------------------------------------- B: uniform attention
@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", ac.L_SWEEP)
def test_uniform_every_mask_edge(ops, dev, dtype, L, causal):
    """uniform_case (q = 0): O[q] within one storage ulp of the fp64 mean of the allowed keys' v
    (integer bit patterns compared) and lse = log2(cnt) to 1e-6 (relative; absolute below 1). One
    key wrongly included or excluded, at any row, changes an integer sum and the count."""
    n, H = 3, 2
    qkv = ac.uniform_case(L, 2000 + L, n, H).to(dev, dtype)
    want_O, want_lse = ac.uniform_expected(qkv, n, L, H, causal)
    O, lse = run_fwd(ops, qkv, n, L, H, causal)
    assert ac.ulp_diff(ac.heads(O, n, L, H), want_O.to(dtype)).max().item() <= 1
    err = (lse.reshape(n, H, L).double() - want_lse).abs()
    assert (err <= 1e-6 * want_lse.clamp_min(1.0)).all()


# ------------------------------------------------------- C: per-element / per-row, random data
def check_lse(lse, ref, n, H, L):
    """1e-5 relative per element; the kernels form lse = max * c + log2(sum) in f32, two terms of
    magnitude >= 1 in general, so a value below 1 is held to 1e-5 absolute."""
    err = (lse.reshape(n, H, L).double() - ref.lse).abs()
    assert (err <= 1e-5 * ref.lse.abs().clamp_min(1.0)).all(), err.max().item()


def check_rows(got, ref, emu, tag):
    """row_err(kernel, fp64) <= 2 row_err(emulate, fp64) per tensor: the factor 2 covers f32
    summation order and storage roundings that flip; a wrong row is ~60 times over. Prints each
    figure before it asserts."""
    for name, g, r, e in zip(("dq", "dk", "dv"), got, ref, emu):
        k_err, e_err = ac.row_err(g, r), ac.row_err(e, r)
        print(f"ATTN_ROW_ERR {tag} {name} kernel {k_err:.3e} emulate {e_err:.3e} "
              f"ratio {k_err / e_err:.3f}")
        assert k_err <= 2 * e_err, (tag, name, k_err, e_err)


@DTYPES
@pytest.mark.parametrize("L,causal", [(33, False), (50, False), (64, False), (129, False),
                                      (160, False), (161, False), (192, False), (77, True),
                                      (197, False), (256, True)])
def test_random_bounds(ops, dev, dtype, L, causal):
    """1.5 * randn inputs at the tile counts no other test launches (NQB = 2, 5, 6) and the
    towers' own lengths, against ref_attention64 on the same rounded inputs. Forward: every
    element inside 2.5 u (P64 |v|) + 1e-6 (attn_cases.fwd_bound), lse to 1e-5. Backward, every
    form: check_rows. Measured kernel / emulation ratios (MI355X), the same in every form, both
    storage types alike: dq 0.78 .. 1.00, dk 0.96 .. 1.20, dv 1.00."""
    n, H = 2, 3
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, 3000 + L, n, H, dev))
    ref = ac.ref_attention64(qkv, dO, n, L, H, causal)
    emu = ac.emulate(qkv, dO, n, L, H, causal, dtype)
    O, lse = run_fwd(ops, qkv, n, L, H, causal)
    over = (ac.heads(O, n, L, H).double() - ref.O).abs() / ac.fwd_bound(ref, qkv, n, L, H, dtype)
    assert over.max().item() <= 1.0  # NaN fails too
    check_lse(lse, ref, n, H, L)
    for form in forms_for(L):
        got = grads(run_bwd(ops, qkv, O, dO, lse, n, L, H, causal, form), n, L, H)
        check_rows(got, ref[3:], emu[3:], f"{'f16' if dtype == HF else 'bf16'} L={L} form={form}")


# --------------------------------------------------- D: strided, poisoned and guarded buffers
GUARD = 64


def guarded_in(x, pad):
    """x [rows, cols] as a view of row stride cols + pad inside a NaN-filled buffer with GUARD
    rows before and after."""
    rows_, cols = x.shape
    buf = torch.full((rows_ + 2 * GUARD, cols + pad), float("nan"), device=x.device, dtype=x.dtype)
    view = buf[GUARD:GUARD + rows_, :cols]
    view.copy_(x)
    return view


def guarded_out(rows_, cols, pad, dtype, dev):
    """(buffer, view [rows, cols] of row stride cols + pad): every 16-bit word the sentinel."""
    buf = torch.full((rows_ + 2 * GUARD, cols + pad), SENTINEL, device=dev, dtype=torch.int16).view(dtype)
    return buf, buf[GUARD:GUARD + rows_, :cols]


def sentinel_intact(buf, rows_, cols):
    chk = buf.view(torch.int16).clone()
    chk[GUARD:GUARD + rows_, :cols] = SENTINEL
    return bool((chk == SENTINEL).all())


@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [50, 130, 197, 250])
def test_strided_guarded_buffers(ops, dev, dtype, L, causal):
    """qkv, O, dO, dqkv as views of row stride cols + 8 and cols + 64 with 64 guard rows before
    and after: input padding / guards NaN, output padding / guards a sentinel bit pattern. The
    forward and every backward form give the contiguous call's bits (lse too), leave every
    sentinel intact and produce no NaN: a read of a neighbouring sequence's rows or of the
    padding, or a store past a sequence's rows, shows."""
    n, H = 3, 2
    D = H * 64
    M = n * L
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, 4000 + L, n, H, dev))
    O, lse = run_fwd(ops, qkv, n, L, H, causal)
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    base = {form: run_bwd(ops, qkv, O, dO, lse, n, L, H, causal, form) for form in forms_for(L)}
    for form, dqkv in base.items():
        assert torch.isfinite(dqkv.float()).all(), form
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
        for form in forms_for(L):
            g_buf, g_s = guarded_out(M, 3 * D, pad, dtype, dev)
            with bwd_form(dtype, form):
                ops.attn_bwd(qkv_s, O_in, dO_s, lse_s, g_s, n, L, H, causal)
            assert same_bits(g_s, base[form]), (pad, form)
            assert sentinel_intact(g_buf, M, 3 * D), (pad, form)


# ------------------------------------------------------------------- E: the persistent walk
@DTYPES
@pytest.mark.parametrize("n,L,H", [(89, 197, 12), (531, 130, 2)])
def test_persistent_walk(ops, dev, dtype, n, L, H):
    """The fused backward with several items per workgroup (persistent_grid: n_seq * H >= 4 * CUs
    at one workgroup per CU; 1068 items, ragged over 256 workgroups, and 1062 at NQB = 5), forms 0
    (automatic) and 1. The big launch's dqkv, NaN-filled before, equals bit for bit the same
    inputs run in sequence chunks below that threshold — the same template at one item per
    workgroup — so contamination between items (prefetch registers, a deferred dQ landing in
    another item, the last item's dQ dropped) shows; and it meets check_rows against
    ref_attention64 evaluated in sequence chunks."""
    cus = ops.device_cu_count(dev)
    assert n * H >= 4 * cus, "too few items to make a workgroup walk on this part"
    D = H * 64
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, 5000 + L, n, H, dev))
    O, lse = run_fwd(ops, qkv, n, L, H, False)
    step = (4 * cus - 1) // H  # sequences per launch that stay at one item per workgroup
    assert 0 < step * H < 4 * cus
    ref = ac.grads_in_chunks(ac.ref_attention64, qkv, dO, n, L, H, False, max(1, 96 // H))
    emu = ac.grads_in_chunks(ac.emulate, qkv, dO, n, L, H, False, max(1, 96 // H), dtype=dtype)
    for form in (0, 1):
        big = run_bwd(ops, qkv, O, dO, lse, n, L, H, False, form)
        assert torch.isfinite(big.float()).all(), form
        parts = torch.full_like(big, float("nan"))
        with bwd_form(dtype, form):
            for s0 in range(0, n, step):
                s1 = min(n, s0 + step)
                r = slice(s0 * L, s1 * L)
                ops.attn_bwd(qkv[r], O[r], dO[r], lse[s0 * H:s1 * H], parts[r], s1 - s0, L, H, False)
        assert same_bits(big, parts), form
        check_rows(grads(big, n, L, H), ref, emu,
                   f"{'f16' if dtype == HF else 'bf16'} walk n={n} L={L} H={H} form={form}")
