"""Every GEMM kernel family x every public epilogue of lc_gemm_nt, on the MI355X: exact, ragged
and strided.

A cell forces one tile (lc_gemm_set_tile, or lc_gemm_set_tile_f16 for the IEEE-half build), runs
one epilogue through ops.gemm_nt at every shape of gemm_epi_cases.SHAPES, contiguous and strided,
and compares with a float64 reference of the same rounded inputs (gemm_epi_cases.reference). The
inputs make the value entering the epilogue exact in any summation order (gemm_epi_cases), so:

* Exact epilogues (BF16, F32, RESID, RESID16, BF16_F32, MUL, out0 of GELU) must equal the
  reference after its one round-to-nearest-even cast to the output type. The MUL and RESID16 side
  inputs are chosen so that the cast does round: truncation or another rounding mode fails.
* Transcendental outputs (out1 of GELU, both outputs of GELU_D, GELU_BWD) are bounded elementwise:
      |out - ref64| <= s(ref64) + 2^-17 max(1, |v|)
  with s the spacing of the output type at the reference (one bf16 or half step) and v the exact
  multiplier (alpha acc for GELU_BWD, 1 otherwise). Derivation: the f32 formula (sigmoid through
  exp2 and rcp, then QuickGELU or its derivative) makes three roundings of at most 2^-24 relative
  each on magnitudes of at most 1 + 1.702 * 16 < 32 (|pre| <= 16 is asserted from the reference),
  i.e. at most 3 * 2^-24 * 32 < 2^-17 absolute per unit of v, and the output cast adds at most
  half a step on top of a value that may sit that far from the reference, hence one whole step.
  QuickGELU' has a zero near x = -0.75, where a purely relative bound cannot hold: the absolute
  term covers it.
* Strided pass: out0, out1 and aux are views [:M, :N] of buffers with 8 more rows and 24 / 40 / 56
  more columns (row strides multiples of 8 that differ per buffer, ldo1 > ldo0), A and B views
  with lda = K + 64, ldb = K + 8. Output buffers are filled with a NaN bit pattern first and their
  guard rows and columns compared as integers afterwards; the padding of A, B and aux is NaN, so a
  read of a wrong row or a padding column poisons the result.
* Cells outside a family's EpiList raise LcError and leave a sentinel-filled out0 untouched.
* For one epilogue and one input, every family that has it gives bit-identical outputs (the
  value entering the epilogue is identical and store_tile's arithmetic is shared).

What each family's main loop assumes about the number of k-tiles was read before the first run:
the launch_nt rings stage min(STAGES - 1, nk) tiles and wait for all of them when nk is short; the
ping-pong and 4-wave kernels count 32-deep halves, always an even number, and guard every DMA of
half h + 3 and every wait by the halves left; gemm8_kernel's prologue and phase waits branch on
nt > 1 and on t + 1 < nt, t + 2 < nt. All of them take K = 64 and odd counts, so no routing
fallback is needed (or tested) for K.
"""
import pytest
import torch

import gemm_epi_cases as C
from gemm_epi_cases import CELLS, REFUSED, SHAPES  # noqa: F401  (the cell table lives there)

pytestmark = pytest.mark.gpu

PAD_ROWS = 8
PAD0, PAD1, PADX = 24, 40, 56  # extra columns of out0, out1, aux


@pytest.fixture(scope="module")
def ops(dev):
    from lcclip import ops as _ops
    return _ops


def _name(st):
    return "bf16" if st == C.BF else "f16"


def _id(cell):
    st, tile, name = cell
    return f"{_name(st)}-t{tile}-{name}"


def _set_tile(st, tile):
    from lcclip import _lib
    lib = _lib.load()
    fn = lib.lc_gemm_set_tile if st == C.BF else lib.lc_gemm_set_tile_f16
    assert fn(tile) == 0


def _padded(x64, dtype, dev, rows, cols):
    """x64 as a [:M, :N] view of a NaN-filled device buffer with `rows` / `cols` more."""
    M, N = x64.shape
    buf = torch.full((M + rows, N + cols), float("nan"), dtype=dtype, device=dev)
    buf[:M, :N] = x64.to(dev).to(dtype)
    return buf[:M, :N]


def _out(M, N, dtype, dev, rows, cols):
    buf = C.fill_sentinel(torch.empty(M + rows, N + cols, dtype=dtype, device=dev))
    return buf, buf[:M, :N]


def _launch(ops, dev, st, name, M, N, K, strided):
    """One ops.gemm_nt call of epilogue `name`; returns [(buffer, view)] of its outputs."""
    x = C.inputs(M, N, K)
    pr = PAD_ROWS if strided else 0
    A = _padded(x["A"], st, dev, 0, 64 if strided else 0)
    B = _padded(x["B"], st, dev, 0, 8 if strided else 0)
    bias = x["bias"].to(dev).float() if C.has_bias(name) else None
    d0, d1 = C.out_dtypes(name, st)
    outs = [_out(M, N, d0, dev, pr, PAD0 if strided else 0)]
    if d1 is not None:
        outs.append(_out(M, N, d1, dev, pr, PAD1 if strided else 0))
    aux = None
    if C.aux_of(name):
        adt = {"RESID": C.F32, "RESID16": C.HF}.get(name, st)
        aux = _padded(x[C.aux_of(name, st)], adt, dev, pr, PADX if strided else 0)
    ops.gemm_nt(A, B, C.EPI[name], outs[0][1], bias=bias, alpha=C.alpha_of(name),
                out1=outs[1][1] if d1 is not None else None, aux=aux)
    return outs


def _check(outs, st, name, M, N, K, where):
    ref = C.reference(M, N, K, name, st)
    assert ref["pre"].abs().max().item() <= C.PRE_MAX
    for i, (buf, view) in enumerate(outs):
        assert C.guards_intact(buf, M, N), f"{where}: out{i} written outside [:M, :N]"
        got = view.cpu()
        r64 = ref[f"out{i}"]
        if ref[f"exact{i}"]:
            want = C.exact_cast(r64, got.dtype)
            bad = (got != want).nonzero()
            assert bad.numel() == 0, (f"{where}: out{i} differs at {bad.shape[0]} elements, first "
                                      f"(m, n) = {bad[0].tolist()}")
        else:
            err = (got.double() - r64).abs()
            lim = C.bound(r64, ref["v"], got.dtype)
            bad = (~(err <= lim)).nonzero()  # a NaN fails
            assert bad.numel() == 0, (f"{where}: out{i} off the bound at {bad.shape[0]} elements, "
                                      f"first (m, n) = {bad[0].tolist()}, max err / bound = "
                                      f"{(err / lim).max().item():.3g}")


@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_cell(ops, dev, cell):
    """One (storage, forced tile, epilogue) cell at every shape, contiguous and strided."""
    st, tile, name = cell
    for M, N, K in SHAPES:
        for strided in (False, True):
            try:
                _set_tile(st, tile)
                outs = _launch(ops, dev, st, name, M, N, K, strided)
            finally:
                _set_tile(st, 0)
            _check(outs, st, name, M, N, K, f"{_id(cell)} M={M} N={N} K={K} strided={strided}")


@pytest.mark.parametrize("cell", REFUSED, ids=_id)
def test_cell_outside_the_family_list_is_refused(ops, dev, cell):
    """A forced family without the epilogue: LcError, nothing launched, out0 untouched."""
    from lcclip._lib import LcError
    st, tile, name = cell
    M, N, K = SHAPES[0]
    x = C.inputs(M, N, K)
    A, B = x["A"].to(dev).to(st), x["B"].to(dev).to(st)
    bias = x["bias"].to(dev).float() if C.has_bias(name) else None
    d0, d1 = C.out_dtypes(name, st)
    out0 = C.fill_sentinel(torch.empty(M, N, dtype=d0, device=dev))
    out1 = C.fill_sentinel(torch.empty(M, N, dtype=d1, device=dev)) if d1 is not None else None
    aux = None
    if C.aux_of(name):
        aux = x[C.aux_of(name, st)].to(dev).to({"RESID": C.F32, "RESID16": C.HF}.get(name, st))
    try:
        _set_tile(st, tile)
        with pytest.raises(LcError):
            ops.gemm_nt(A, B, C.EPI[name], out0, bias=bias, alpha=C.alpha_of(name), out1=out1,
                        aux=aux)
    finally:
        _set_tile(st, 0)
    torch.cuda.synchronize(dev)
    assert C.untouched(out0)
    assert out1 is None or C.untouched(out1)


AGREE = sorted({(st, name) for st, _, name in CELLS}, key=lambda c: (_name(c[0]), c[1]))


@pytest.mark.parametrize("st,name", AGREE, ids=lambda v: v if isinstance(v, str) else _name(v))
def test_families_agree_bit_for_bit(ops, dev, st, name):
    """One epilogue, one input (M = 293, K = 192, contiguous): every forced tile that has the
    epilogue gives the same bits, transcendental outputs included."""
    M, N, K = 293, 768, 192
    first = None
    for tile in C.TILES:
        if (st, tile, name) not in CELLS:
            continue
        try:
            _set_tile(st, tile)
            outs = _launch(ops, dev, st, name, M, N, K, False)
        finally:
            _set_tile(st, 0)
        bits = [C.as_int(v).cpu() for _, v in outs]
        if first is None:
            first = (tile, bits)
            continue
        for i, (a, b) in enumerate(zip(first[1], bits)):
            bad = (a != b).nonzero()
            assert bad.numel() == 0, (f"{_name(st)} {name} out{i}: tile {tile} differs from tile "
                                      f"{first[0]} at {bad.shape[0]} elements, first (m, n) = "
                                      f"{bad[0].tolist()}")
