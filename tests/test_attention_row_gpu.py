"""The single-query-row attention kernels (lc_attn_row_fwd / lc_attn_row_bwd, csrc/attention.hip)
on the MI355X against the cases and yardsticks of tests/attn_cases.py: the image tower's last
block runs them on its CLS row (row 0), here every row position, mask and storage type.

  exact    one-hot attention: O_row and dv are the exact integers, no tolerance
  random   the per-element forward bound of test_attention_gpu's case C at the chosen row; the
           backward against ref_attention64 with dO zero off the row, per-row error at most twice
           emulate's on the same inputs (emulate's stored O among them)
  dead     dq off the row exactly zero; causal: dk, dv beyond the row exactly zero
  strided  ldo / lddq larger than needed inside NaN- / sentinel-filled buffers: same bits,
           nothing else written
(One workgroup per (sequence, head) and no item walk: no walk case.)
"""
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
LS = (1, 17, 32, 33, 64, 65, 197, 256)
SENTINEL = 0x5A5A
GUARD = 8
N, H = 3, 2
D = H * 64


@pytest.fixture(scope="module")
def ops(dev):
    from lcclip import ops as _ops
    return _ops


def rows_of(L):
    """row 0, an inner row, the last row (distinct ones)."""
    return sorted({0, (2 * L) // 3, L - 1})


def bits(x):
    return x.contiguous().view(torch.int16)


def assert_exact(got, want, tag):
    bad = ~(got == want)
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ"


def run_fwd(ops, qkv, L, row, causal):
    O = torch.full((N, D), float("nan"), device=qkv.device, dtype=qkv.dtype)
    lse = torch.full((N * H,), float("nan"), device=qkv.device)
    ops.attn_row_fwd(qkv, O, lse, N, L, H, row, causal)
    return O, lse


def run_bwd(ops, qkv, O, dO, lse, L, row, causal):
    dqkv = torch.full((N * L, 3 * D), float("nan"), device=qkv.device, dtype=qkv.dtype)
    ops.attn_row_bwd(qkv, O, dO, lse, dqkv, N, L, H, row, causal)
    return dqkv


def grads(dqkv, L):
    return tuple(ac.heads(dqkv[:, i * D:(i + 1) * D], N, L, H) for i in range(3))


def row_only(dO, L, row):
    """dO [N*L, D] with every row but `row` of each sequence zeroed, and its compact rows."""
    z = torch.zeros_like(dO).view(N, L, D)
    z[:, row] = dO.view(N, L, D)[:, row]
    return z.view(N * L, D), z[:, row].contiguous()


def check_dead(dq, dk, dv, L, row, causal):
    off = torch.ones(L, dtype=torch.bool, device=dq.device)
    off[row] = False
    assert (dq[:, :, off] == 0).all()
    if causal:
        assert (dk[:, :, row + 1:] == 0).all() and (dv[:, :, row + 1:] == 0).all()


@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", LS)
def test_row_one_hot_exact(ops, dev, dtype, L, causal):
    """one_hot_case: p is exactly 1 on the row's target key, so O_row = v[pi(row)] and dv =
    dO_row at key pi(row), zero elsewhere, exactly; lse_row = on-target score * log2(e); dq, dk
    at most 2^-20 (test_attention_gpu.test_one_hot_exact's derivation)."""
    qs = ac.ONE_HOT_QSCALE[dtype]
    qkv, dO, pi = ac.one_hot_case(L, causal, 1000 + L, N, H, qs)
    qkv, dO = qkv.to(dev, dtype), dO.to(dev, dtype)
    for row in rows_of(L):
        dO_full, dO_row = row_only(dO, L, row)
        want_O, want_dv = (x.to(dtype) for x in ac.one_hot_expected(qkv, dO_full, pi))
        O, lse = run_fwd(ops, qkv, L, row, causal)
        assert_exact(O.view(N, H, 64), want_O[:, :, row], f"O row {row}")
        assert torch.allclose(lse, torch.full_like(lse, 8 * qs * ac.LOG2E), rtol=1e-6, atol=0)
        dq, dk, dv = grads(run_bwd(ops, qkv, O, dO_row, lse, L, row, causal), L)
        assert_exact(dv, want_dv, f"dv row {row}")
        assert (dq.abs() <= 2.0 ** -20).all() and (dk.abs() <= 2.0 ** -20).all()
        check_dead(dq, dk, dv, L, row, causal)


@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", LS)
def test_row_forward_is_the_full_forward_row(ops, dev, dtype, L, causal):
    """O_row and lse_row are bit for bit row `row` of attn_fwd's O and lse (the forward runs the
    same instructions on the same operands for the wave that owns the row)."""
    qkv, _ = (x.to(dtype) for x in ac.random_case(L, 6000 + L, N, H, dev))
    O_full = torch.empty(N * L, D, device=dev, dtype=dtype)
    lse_full = torch.empty(N * H, L, device=dev)
    ops.attn_fwd(qkv, O_full, lse_full, N, L, H, causal)
    for row in rows_of(L):
        O, lse = run_fwd(ops, qkv, L, row, causal)
        assert torch.equal(bits(O), bits(O_full.view(N, L, D)[:, row])), row
        assert torch.equal(lse, lse_full[:, row]), row


@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", LS)
def test_row_random_bounds(ops, dev, dtype, L, causal):
    """1.5 * randn inputs against ref_attention64 on the same rounded inputs. Forward: every
    element of O_row inside attn_cases.fwd_bound at that row, lse to 1e-5. Backward (dO zero off
    the row): row_err(kernel, fp64) <= 2 row_err(emulate, fp64) per tensor, each figure printed
    first; the dead rows exactly zero."""
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, 3000 + L, N, H, dev))
    for row in rows_of(L):
        dO_full, dO_row = row_only(dO, L, row)
        ref = ac.ref_attention64(qkv, dO_full, N, L, H, causal)
        emu = ac.emulate(qkv, dO_full, N, L, H, causal, dtype)
        O, lse = run_fwd(ops, qkv, L, row, causal)
        bound = ac.fwd_bound(ref, qkv, N, L, H, dtype)[:, :, row]
        over = (O.view(N, H, 64).double() - ref.O[:, :, row]).abs() / bound
        assert over.max().item() <= 1.0  # NaN fails too
        err = (lse.view(N, H).double() - ref.lse[:, :, row]).abs()
        assert (err <= 1e-5 * ref.lse[:, :, row].abs().clamp_min(1.0)).all(), err.max().item()
        # the backward on emulate's inputs: its stored O (the P V product of a rounded P, which
        # the row kernel does not round; inside the forward bound like the kernel's own) —
        # Delta = rowsum(dO * stored O) is one number per (sequence, head), so with two
        # different roundings of O the worst-row ratio would compare two draws of 6 samples
        O_emu = emu.O[:, :, row].reshape(N, D).to(dtype)
        assert ((O_emu.view(N, H, 64).double() - ref.O[:, :, row]).abs() <= bound).all()
        got = grads(run_bwd(ops, qkv, O_emu, dO_row, lse, L, row, causal), L)
        check_dead(*got, L, row, causal)
        check_dead(*grads(run_bwd(ops, qkv, O, dO_row, lse, L, row, causal), L), L, row, causal)
        # the rows that are exactly zero in the reference too (checked above) are left out of
        # row_err: its denominator, max(row norm, median row norm), is 0 on them
        keys = slice(0, row + 1) if causal else slice(0, L)
        live = (slice(row, row + 1), keys, keys)
        for name, g, r, e, sl in zip(("dq", "dk", "dv"), got, ref[3:], emu[3:], live):
            if not r[:, :, sl].any():
                # one visible key (L = 1, or causal at row 0): P = 1 and dP = Delta, so dS, dq
                # and dk are exact zeros in fp64 and in emulate; twice a zero error is zero
                assert (L == 1 or (causal and row == 0)) and name != "dv"
                assert not e[:, :, sl].any() and (g[:, :, sl] == 0).all(), name
                continue
            k_err, e_err = ac.row_err(g[:, :, sl], r[:, :, sl]), ac.row_err(e[:, :, sl], r[:, :, sl])
            print(f"ATTN_ROW1_ERR {'f16' if dtype == HF else 'bf16'} L={L} row={row} "
                  f"causal={causal} {name} kernel {k_err:.3e} emulate {e_err:.3e}")
            assert k_err <= 2 * e_err, (name, row, k_err, e_err)


@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [17, 197, 256])
def test_row_strided_guarded(ops, dev, dtype, L, causal):
    """qkv, O_row, dO_row and dqkv as views of a wider row stride inside NaN-filled (inputs) or
    sentinel-filled (outputs) buffers with guard rows before and after: the contiguous call's
    bits, every sentinel intact, no NaN."""
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, 4000 + L, N, H, dev))
    row = (2 * L) // 3
    dO_row = row_only(dO, L, row)[1]
    O, lse = run_fwd(ops, qkv, L, row, causal)
    base = run_bwd(ops, qkv, O, dO_row, lse, L, row, causal)
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    assert torch.isfinite(base.float()).all()

    def guarded_in(x, pad):
        r, c = x.shape
        buf = torch.full((r + 2 * GUARD, c + pad), float("nan"), device=dev, dtype=dtype)
        buf[GUARD:GUARD + r, :c] = x
        return buf[GUARD:GUARD + r, :c]

    def guarded_out(r, c, pad):
        buf = torch.full((r + 2 * GUARD, c + pad), SENTINEL, device=dev, dtype=torch.int16).view(dtype)
        return buf, buf[GUARD:GUARD + r, :c]

    def intact(buf, r, c):
        chk = buf.view(torch.int16).clone()
        chk[GUARD:GUARD + r, :c] = SENTINEL
        return bool((chk == SENTINEL).all())

    for pad in (8, 64):
        qkv_s = guarded_in(qkv, pad)
        O_buf, O_s = guarded_out(N, D, pad)
        lse_buf = torch.full((N * H + 2 * GUARD,), -7.0, device=dev)
        lse_s = lse_buf[GUARD:GUARD + N * H]
        ops.attn_row_fwd(qkv_s, O_s, lse_s, N, L, H, row, causal)
        assert torch.equal(bits(O_s), bits(O)) and torch.equal(lse_s, lse), pad
        assert intact(O_buf, N, D), pad
        assert (lse_buf[:GUARD] == -7.0).all() and (lse_buf[-GUARD:] == -7.0).all(), pad
        g_buf, g_s = guarded_out(N * L, 3 * D, pad)
        ops.attn_row_bwd(qkv_s, guarded_in(O, pad), guarded_in(dO_row, pad), lse_s, g_s, N, L, H,
                         row, causal)
        assert torch.equal(bits(g_s), bits(base)), pad
        assert intact(g_buf, N * L, 3 * D), pad


def test_row_argument_checks(ops, dev):
    """row outside [0, L) and L > 256 are refused on the host (nothing is launched)."""
    from lcclip._lib import LcError
    L = 8
    qkv = torch.zeros(N * L, 3 * D, device=dev, dtype=BF)
    O = torch.zeros(N, D, device=dev, dtype=BF)
    lse = torch.zeros(N * H, device=dev)
    for row in (-1, L):
        with pytest.raises(LcError):
            ops.attn_row_fwd(qkv, O, lse, N, L, H, row, False)
        with pytest.raises(LcError):
            ops.attn_row_bwd(qkv, O, O, lse, torch.zeros_like(qkv), N, L, H, row, False)
    big = torch.zeros(N * 257, 3 * D, device=dev, dtype=BF)
    with pytest.raises(LcError):
        ops.attn_row_fwd(big, O, lse, N, 257, H, 0, False)
