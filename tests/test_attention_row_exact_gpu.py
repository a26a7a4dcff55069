"""ops.attn_bwd_live_row (lc_attn_bwd_live_row: the MFMA attention backward's single-row mode)
against the launch it replaces: ops.attn_bwd on full-size operands blanked off the live row the
way engine.py builds them (O and dO zero, lse = 1e30 there). The whole dqkv is compared with ==,
so a +0 may stand where the full kernel wrote -0; nothing else may differ.

L in {17, 50, 129, 197, 256}: NQB 1, 2, the first persistent count (5), the step's (7) and the
largest (8, where the full path is the key-major + query-major pair). Rows 0, L - 1 and 40.
24 sequences x 12 heads are 288 items on 256 CUs, so some persistent workgroups walk two items.
Causal masks are supported and tested.
"""
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
SENTINEL = 0x5A5A
GUARD = 8


@pytest.fixture(scope="module")
def ops(dev):
    from lcclip import ops as _ops
    return _ops


def rows_of(L):
    return sorted({0, L - 1} | ({40} if L > 40 else set()))


def compact(ops, qkv, dO, n, L, H, row, causal):
    """The compact operands of the row: O_row, lse_row from the row forward, dO_row."""
    D = H * 64
    O = torch.empty(n, D, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(n * H, device=qkv.device)
    ops.attn_row_fwd(qkv, O, lse, n, L, H, row, causal)
    return O, dO.view(n, L, D)[:, row].contiguous(), lse


def blanked_reference(ops, qkv, O_row, dO_row, lse_row, n, L, H, row, causal):
    """engine.py's blanked launch: the full kernel on O, dO zero and lse = 1e30 off the row."""
    D = H * 64
    Of = torch.zeros(n * L, D, device=qkv.device, dtype=qkv.dtype)
    dOf = torch.zeros_like(Of)
    lsef = torch.full((n * H, L), 1e30, dtype=torch.float32, device=qkv.device)
    Of.view(n, L, D)[:, row] = O_row
    dOf.view(n, L, D)[:, row] = dO_row
    lsef[:, row] = lse_row
    want = torch.full((n * L, 3 * D), float("nan"), device=qkv.device, dtype=qkv.dtype)
    ops.attn_bwd(qkv, Of, dOf, lsef, want, n, L, H, causal)
    return want


def check(ops, dev, dtype, n, H, L, causal, seed):
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, seed, n, H, dev))
    for row in rows_of(L):
        O_row, dO_row, lse_row = compact(ops, qkv, dO, n, L, H, row, causal)
        want = blanked_reference(ops, qkv, O_row, dO_row, lse_row, n, L, H, row, causal)
        got = torch.full_like(want, float("nan"))
        assert ops.attn_bwd_live_row(qkv, O_row, dO_row, lse_row, got, n, L, H, row, causal)
        bad = ~(got == want)
        assert not bad.any(), (f"L={L} row={row} causal={causal}: {int(bad.sum())} of "
                               f"{bad.numel()} elements differ")
        # the compared values are not trivially zero (dv of the keys the row sees never is)
        assert want.view(n, L, -1)[:, 0, 2 * H * 64:].any()


@DTYPES
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [17, 50, 129, 197, 256])
def test_live_row_equals_blanked_full_launch(ops, dev, dtype, L, causal):
    check(ops, dev, dtype, 24, 12, L, causal, 7000 + L)


@DTYPES
@pytest.mark.parametrize("causal", [False, True])
def test_live_row_small(ops, dev, dtype, causal):
    for L in (17, 197):
        check(ops, dev, dtype, 2, 2, L, causal, 7500 + L)


@DTYPES
def test_live_row_strided_guarded(ops, dev, dtype):
    """Operands and dqkv as views of a wider row stride inside NaN- (inputs) or sentinel-filled
    (output) buffers with guard rows around them: the contiguous call's result, bands intact."""
    n, H, L, row, causal = 3, 2, 197, 131, False
    D = H * 64
    qkv, dO = (x.to(dtype) for x in ac.random_case(L, 7900, n, H, dev))
    O_row, dO_row, lse_row = compact(ops, qkv, dO, n, L, H, row, causal)
    base = torch.full((n * L, 3 * D), float("nan"), device=dev, dtype=dtype)
    assert ops.attn_bwd_live_row(qkv, O_row, dO_row, lse_row, base, n, L, H, row, causal)
    assert torch.isfinite(base.float()).all()

    def guarded_in(x, pad):
        r, c = x.shape
        buf = torch.full((r + 2 * GUARD, c + pad), float("nan"), device=dev, dtype=dtype)
        buf[GUARD:GUARD + r, :c] = x
        return buf[GUARD:GUARD + r, :c]

    for pad in (8, 64):
        buf = torch.full((n * L + 2 * GUARD, 3 * D + pad), SENTINEL, device=dev,
                         dtype=torch.int16).view(dtype)
        g_s = buf[GUARD:GUARD + n * L, :3 * D]
        assert ops.attn_bwd_live_row(guarded_in(qkv, pad), guarded_in(O_row, pad),
                                     guarded_in(dO_row, pad), lse_row, g_s, n, L, H, row, causal)
        assert torch.equal(g_s.contiguous().view(torch.int16), base.view(torch.int16)), pad
        chk = buf.view(torch.int16).clone()
        chk[GUARD:GUARD + n * L, :3 * D] = SENTINEL
        assert bool((chk == SENTINEL).all()), pad


def test_live_row_refused_under_another_form(ops, dev):
    """lc_attn_bwd_set_form(2 or 3) changes what the full launch computes: the row mode then
    returns the error and writes nothing."""
    from lcclip import _lib
    lib = _lib.load()
    n, H, L = 2, 2, 50
    qkv, dO = (x.to(BF) for x in ac.random_case(L, 7950, n, H, dev))
    O_row, dO_row, lse_row = compact(ops, qkv, dO, n, L, H, 0, False)
    out = torch.full((n * L, 3 * H * 64), 7.0, device=dev, dtype=BF)
    assert lib.lc_attn_bwd_set_form(2) == 0
    try:
        assert not ops.attn_bwd_live_row(qkv, O_row, dO_row, lse_row, out, n, L, H, 0, False)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    finally:
        lib.lc_attn_bwd_set_form(0)
