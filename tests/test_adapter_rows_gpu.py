"""The _rows forms of the adapter forwards (lc_adapter_ln_fwd_rows[_x16|_f16], lc_adapter_fwd_rows
[_f16]): rows gathered from a larger launch, run with the dropout row id m * mul + add, give the
bits those rows had in the full launch (the arithmetic is row-local; only the dropout mask knows
the row number). The image tower's last block runs them on its CLS rows, mul = L.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
D, N, L, KEEP, SEED = 768, 4, 17, 0.9, 24681357


@pytest.fixture(scope="module")
def ops(dev):
    from lcclip import ops as _ops
    return _ops


def make(dev, dt, xdt):
    torch.manual_seed(5)
    M = N * L
    z = torch.randn(M, D, device=dev).to(dt)
    Wd = (torch.randn(64, D, device=dev) * D ** -0.5).to(dt)
    Wu = (torch.randn(D, 64, device=dev) * 0.125).to(dt)
    bd = torch.randn(64, device=dev) * 0.1
    bu = torch.randn(D, device=dev) * 0.1
    x = (torch.randn(M, D, device=dev) * 2).to(xdt)
    gam, bet = torch.randn(D, device=dev), torch.randn(D, device=dev)
    return z, Wd, bd, Wu, bu, x, gam, bet


def run_ln(ops, z, Wd, bd, Wu, bu, x, gam, bet, rows=None):
    M = z.shape[0]
    dev = z.device
    xo = torch.full((M, D), float("nan"), device=dev, dtype=x.dtype)
    h = torch.full((M, 64), float("nan"), device=dev, dtype=z.dtype)
    y = torch.full((M, D), float("nan"), device=dev, dtype=z.dtype)
    m, r = torch.full((M,), float("nan"), device=dev), torch.full((M,), float("nan"), device=dev)
    ops.adapter_ln_fwd(z, Wd, bd, Wu, bu, 0.1, KEEP, SEED, x, xo, h, gam, bet, y, m, r, rows=rows)
    return h, xo, y, m, r


@pytest.mark.parametrize("dt,xdt", [(BF, F32), (BF, HF), (HF, F32)], ids=["bf16", "x16", "f16"])
def test_adapter_ln_fwd_rows_bits(ops, dev, dt, xdt):
    """h, x_out, y, mean and rstd of the 4 gathered CLS rows (rows = (L, 0)) are bit-identical
    to rows 0, L, 2L, 3L of the full 68-row launch; with the plain row ids the dropout mask
    differs (the case has teeth); an offset (add) selects another row of every sequence."""
    z, Wd, bd, Wu, bu, x, gam, bet = make(dev, dt, xdt)
    full = run_ln(ops, z, Wd, bd, Wu, bu, x, gam, bet)
    for add in (0, 5):
        idx = torch.arange(N, device=dev) * L + add
        got = run_ln(ops, z[idx].contiguous(), Wd, bd, Wu, bu, x[idx].contiguous(), gam, bet,
                     rows=(L, add))
        for name, g, f in zip(("h", "x_out", "y", "mean", "rstd"), got, full):
            assert torch.equal(g, f[idx]), (name, add)
    idx = torch.arange(N, device=dev) * L
    plain = run_ln(ops, z[idx].contiguous(), Wd, bd, Wu, bu, x[idx].contiguous(), gam, bet)
    assert torch.equal(plain[0][0], full[0][0])           # row 0 has id 0 either way
    assert not torch.equal(plain[0][1:] == 0, full[0][idx][1:] == 0)
    assert not torch.isnan(full[0].float()).any() and not torch.isnan(got[0].float()).any()


@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "f16"])
def test_adapter_fwd_rows_bits(ops, dev, dt):
    """The unfused pair (the EPI_AD_DOWN GEMM epilogue's mask): h and x_out of the gathered rows
    are bit-identical to those rows of the full launch."""
    z, Wd, bd, Wu, bu, x, _, _ = make(dev, dt, F32)
    M = N * L

    def run(zz, xx, rows=None):
        xo = torch.full(tuple(xx.shape), float("nan"), device=dev)
        h = torch.full((zz.shape[0], 64), float("nan"), device=dev, dtype=dt)
        ops.adapter_fwd(zz, Wd, bd, Wu, bu, 0.1, KEEP, SEED, xx, xo, h, rows=rows)
        return h, xo

    h_full, xo_full = run(z, x)
    assert ((h_full == 0).float().mean() > 0.05)  # dropout and ReLU zeros are there
    for add in (0, 5):
        idx = torch.arange(N, device=dev) * L + add
        h, xo = run(z[idx].contiguous(), x[idx].contiguous(), rows=(L, add))
        assert torch.equal(h, h_full[idx]) and torch.equal(xo, xo_full[idx]), add
    idx = torch.arange(N, device=dev) * L
    h_plain, _ = run(z[idx].contiguous(), x[idx].contiguous())
    assert not torch.equal(h_plain[1:] == 0, h_full[idx][1:] == 0)
    assert M == 68


def test_rows_argument_checks(ops, dev):
    z, Wd, bd, Wu, bu, x, gam, bet = make(dev, BF, F32)
    with pytest.raises(ValueError):
        run_ln(ops, z, Wd, bd, Wu, bu, x, gam, bet, rows=(0, 0))
    with pytest.raises(ValueError):
        run_ln(ops, z, Wd, bd, Wu, bu, x, gam, bet, rows=(L, -1))
