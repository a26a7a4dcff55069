"""ln_fwd_kernel / ln_bwd_kernel (norm.hip) at every instantiated width, on the MI355X, against a
float64 reference of the same rounded inputs, element by element and row by row.

A cell is (D, rows, variant); the variant names the types (x, y, dy, dx / dres):
    f32      f32   f32   f32   f32
    bf16     f32   bf16  bf16  f32    (+ the bf16 copy of dx)
    x16      half  bf16  bf16  f32    (+ copy)     lc_layernorm_*_x16
    x16-f32  half  f32   f32   f32                 lc_layernorm_*_x16
    g16      half  bf16  bf16  half   (+ copy)     lc_layernorm_bwd_g16
    g16-f32  half  f32   f32   half                lc_layernorm_bwd_g16
    f16      f32   half  half  f32    (+ half copy) the IEEE-half build, lc_layernorm_*_f16
A half gradient with an f32 x does not exist (ops.layernorm_bwd raises ValueError: asserted
once). Every cell runs contiguous and strided (views of buffers with 8 more rows and 24 / 40 / 56
more columns, NaN input padding, sentinel-filled outputs whose guards are compared as integers),
plain and row-gathered (row_idx), and the backward with and without dres in both; ops.layernorm_bwd
accepts every such combination. dx, dres and the 16-bit copy share one row stride (the kernel has
one), so they get the same padding.

With rows >= 5 the input's last four rows are the hard ones of peft_cases.ln_inputs: mean 100 with
spread 1, one outlier of 200, a constant 2 (mean == 2 and y == cast(beta) bit for bit: every
partial sum is exact; rstd within 2 ulp of float32(1 / sqrt(1e-5))), and zeros. The constant row
found ln_fwd_kernel taking its deviations about another mean than the one it saves at D = 768:
the compiler had fused x - sum * (1 / 768) into one fma on the unrounded product, so the row gave
y = beta - 1.9e-5 gamma (2 - 1536 fl(1 / 768) = -2^-24, times rstd = 316); the kernel now
subtracts the saved mean (norm.hip).

mean, rstd and every element of y and dx lie within peft_cases.ln_fwd_bounds / ln_bwd_bound
(derived there from the summation trees, not measured); the backward gets the reference's mean
and rstd rounded to f32. max(err / bound) per cell is recorded (test_mvp_gpu.record).
"""
import pytest
import torch

import gemm_epi_cases as C
import peft_cases as P
from test_peft_matrix_gpu import PAD_A, PAD_B, PAD_C, _guard1d, _guard2d, _in, _out, _out1d, _within, record

pytestmark = pytest.mark.gpu

BF, HF, F32 = C.BF, C.HF, C.F32
# variant -> (x, y, dy, dx / dres, 16-bit copy or None)
VARIANTS = {"f32": (F32, F32, F32, F32, None), "bf16": (F32, BF, BF, F32, BF),
            "x16": (HF, BF, BF, F32, BF), "x16-f32": (HF, F32, F32, F32, None),
            "g16": (HF, BF, BF, HF, BF), "g16-f32": (HF, F32, F32, HF, None),
            "f16": (F32, HF, HF, F32, HF)}
CELLS = [(D, rows, v) for D in P.LN_D for rows in P.LN_ROWS for v in VARIANTS]
GATHER = {1: [0], 5: [4, 1, 3, 2], 333: [0, 17, 34, 200, 329, 330, 331, 332]}


@pytest.fixture(scope="module")
def ops(dev):
    from lcclip import ops as _ops
    return _ops


def _id(c):
    return f"D{c[0]}-rows{c[1]}-{c[2]}"


def _ulp32(v):
    return C.as_int(torch.tensor([v], dtype=F32)).item()


def _forward(ops, dev, x, gam, bet, ydt, idx, strided):
    n = x.shape[0] if idx is None else idx.numel()
    y = _out(n, x.shape[1], ydt, dev, strided, PAD_B)
    mean, rstd = _out1d(n, dev), _out1d(n, dev)
    ops.layernorm_fwd(x, gam, bet, y[1], mean[1], rstd[1], row_idx=idx)
    torch.cuda.synchronize(dev)
    return y, mean, rstd


def _backward(ops, dev, dy, x, mean, rstd, gam, gdt, cdt, dres, idx, strided):
    R, D = x.shape
    dx = _out(R, D, gdt, dev, strided, PAD_B)
    dxb = _out(R, D, cdt, dev, strided, PAD_B) if cdt is not None else None
    ops.layernorm_bwd(dy, x, mean, rstd, gam, dx[1], dxb[1] if dxb else None, dres=dres, row_idx=idx)
    torch.cuda.synchronize(dev)
    return dx, dxb


@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_layernorm_cell(ops, dev, cell):
    D, rows, var = cell
    xdt, ydt, dydt, gdt, cdt = VARIANTS[var]
    c = P.ln_inputs(rows, D)
    x_cpu, dres_cpu = c["x"].to(xdt), c["dres"].to(gdt)
    x64, gam64, bet64 = x_cpu.double(), c["gamma"].double(), c["beta"].double()
    gam, bet = c["gamma"].to(dev), c["beta"].to(dev)
    full = P.ln_fwd_ref(x64, gam64, bet64)
    worst_f, worst_b = 0.0, 0.0
    for strided in (False, True):
        x = _in(x_cpu, xdt, dev, strided, PAD_A)
        for gathered in (False, True):
            where = f"{_id(cell)} strided={strided} gathered={gathered}"
            sel = torch.tensor(GATHER[rows]) if gathered else torch.arange(rows)
            idx = sel.to(dev).to(torch.int32) if gathered else None
            n = sel.numel()
            ref = tuple(t[sel] for t in full)
            # ---- forward
            y, mean, rstd = _forward(ops, dev, x, gam, bet, ydt, idx, strided)
            _guard2d(y[0], n, D, "y", where)
            _guard1d(mean[0], n, "mean", where)
            _guard1d(rstd[0], n, "rstd", where)
            b_mean, b_rstd, b_y = P.ln_fwd_bounds(x64[sel], gam64, bet64, ref, ydt)
            got_y, got_m, got_r = y[1].cpu(), mean[1].cpu(), rstd[1].cpu()
            worst_f = max(worst_f, _within(got_m.double(), ref[0], b_mean, "mean", where),
                          _within(got_r.double(), ref[1], b_rstd, "rstd", where),
                          _within(got_y.double(), ref[2], b_y, "y", where))
            if rows >= 5:
                k = (sel == rows - 2).nonzero().item()   # the constant row
                assert got_m[k].item() == 2.0, f"{where}: mean of the constant row"
                assert torch.equal(got_y[k], c["beta"].to(ydt)), f"{where}: y of the constant row is not beta"
                assert abs(_ulp32(got_r[k].item()) - _ulp32(1e-5 ** -0.5)) <= 2, f"{where}: rstd of the constant row"
                k0 = (sel == rows - 1).nonzero().item()  # the row of zeros
                assert got_m[k0].item() == 0.0 and torch.equal(got_y[k0], c["beta"].to(ydt))
            # ---- backward on the reference's statistics rounded to f32
            m32, r32 = ref[0].float(), ref[1].float()
            dy_cpu = c["dy"][:n].to(dydt)
            dy = _in(dy_cpu, dydt, dev, strided, PAD_C)
            for with_dres in (True, False):
                wh = f"{where} dres={with_dres}"
                dres = _in(dres_cpu, gdt, dev, strided, PAD_B) if with_dres else None
                dx, dxb = _backward(ops, dev, dy, x, m32.to(dev), r32.to(dev), gam, gdt, cdt, dres, idx, strided)
                dref = P.ln_bwd_ref(dy_cpu.double(), x64[sel], m32.double(), r32.double(), gam64,
                                    dres_cpu.double()[sel] if with_dres else None)
                lim = P.ln_bwd_bound(dy_cpu.double(), x64[sel], m32.double(), r32.double(), gam64, dref, gdt)
                _guard2d(dx[0], rows, D, "dx", wh)
                got = dx[1].cpu()
                worst_b = max(worst_b, _within(got[sel].double(), dref, lim, "dx", wh))
                rest = torch.ones(rows, dtype=torch.bool)
                rest[sel] = False
                assert C.untouched(got[rest]), f"{wh}: dx written in a row outside row_idx"
                if dxb is not None:
                    _guard2d(dxb[0], rows, D, "dx copy", wh)
                    cp = dxb[1].cpu()
                    # the copy is the stored dx rounded once more (half dx: the half value)
                    assert torch.equal(cp[sel], got[sel].float().to(cdt)), f"{wh}: the 16-bit copy of dx"
                    assert C.untouched(cp[rest]), f"{wh}: dx copy written in a row outside row_idx"
                if gdt == HF:
                    # the half dx is the f32 kernel's dx rounded to half
                    d32, _ = _backward(ops, dev, dy, x, m32.to(dev), r32.to(dev), gam, F32, None,
                                       dres.float() if with_dres else None, idx, False)
                    assert torch.equal(got[sel], d32[1].cpu()[sel].to(HF)), f"{wh}: half dx is not the f32 dx rounded"
    record(test="layernorm_matrix", kernel="ln_fwd", cell=_id(cell), max_err_over_bound=worst_f)
    record(test="layernorm_matrix", kernel="ln_bwd", cell=_id(cell), max_err_over_bound=worst_b)


def test_half_gradient_needs_a_half_x(ops, dev):
    c = P.ln_inputs(5, 256)
    x, dy = c["x"].to(dev), c["dy"].to(dev)
    m, r = torch.zeros(5, device=dev), torch.ones(5, device=dev)
    dx = C.fill_sentinel(torch.empty(5, 256, dtype=HF, device=dev))
    with pytest.raises(ValueError):
        ops.layernorm_bwd(dy, x, m, r, c["gamma"].to(dev), dx, None, dres=None)
    torch.cuda.synchronize(dev)
    assert C.untouched(dx)
