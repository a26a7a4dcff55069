"""The adapter and LoRA kernels of peft.hip (and the two GEMM epilogues of the separate adapter
forward / backward) on the MI355X against float64 references: exact, every walker depth, strided.

The inputs (peft_cases) make every value that enters a rounding exact in any summation order, so
h, x_out, dpre, dz, the four adapter weight gradients and the LoRA gradients must equal the
float64 reference after its one round-to-nearest-even cast to the output type, bit for bit. The
casts of x_out to half and of dz to bf16 do round at a share of the elements (asserted on the CPU,
test_peft_cases), so truncation fails. The dropout mask is compared with peft_cases.drop_keep, an
integer restatement of drop_mul, element by element.

Row counts: peft_cases.walker_rows gives walkers 0 and 1 d blocks (walker 1's last one ragged, 5
rows) and every other walker d - 1, for d up to the ring depth + 1: the ramp-up and drain cases
of the counted vmcnt waits. The CU count is the device's.

Passes: every cell runs contiguous and strided. Strided operands are views [:M, :D] of buffers
with 8 more rows and 24 / 40 / 56 more columns; input padding is NaN, output buffers hold a NaN
bit pattern first and their guard rows and columns are compared as integers afterwards (1-D and
dense outputs carry guard elements behind them).

What was read in the code before the first run of the new depths (2 to 4 of the adapter backward,
2 and 3 of the LoRA walker): adapter_bwd_fused_kernel waits vmcnt(min(P - 1, n - 1 - i) LP +
min(i, P) SP) for block i's DMA; per wave the memory operations issued after that DMA are the
DMAs of the blocks issued since (min(n, i + P) - i - 1 of them) and the stores of the min(i, P)
blocks stored since, which is the formula; the only conditional stores are those of the ragged
block, always a walker's last. lora_grad1p_kernel waits for X_i with two ring pieces behind it and
for chunk c with the next chunk's piece (if one exists) and, for c < 2, X_{i+1} behind it; both
counts hold for every number of blocks. Every DMA row is clamped to M - 1 and every store masked
by m < M.

Left out: the separate forward (ops.adapter_fwd) has no half-residual form (ops.py sends a half
residual stream through adapter_ln_fwd), so x16 cells exist for the fused form only.
"""
import pytest
import torch

import gemm_epi_cases as C
import peft_cases as P
from test_mvp_gpu import record   # one line per measured margin, in the file the model tests use

pytestmark = pytest.mark.gpu

BF, HF, F32 = C.BF, C.HF, C.F32
PAD_ROWS = 8
PAD_A, PAD_B, PAD_C = 24, 40, 56
ROW_IDS = (197, 3)   # the last block's CLS rows: row m draws the mask of row 197 m + 3
EPOCH = 5


@pytest.fixture(scope="module")
def ops(dev):
    from lcclip import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cus(ops, dev):
    return ops.device_cu_count(dev)


# ------------------------------------------------------------------------------------- helpers
def _in(x, dtype, dev, strided, cols):
    """x (CPU, exact) as `dtype` on the device: contiguous, or a [:M, :N] view of a NaN-filled
    buffer with PAD_ROWS more rows and `cols` more columns."""
    x = x.to(dtype)
    if not strided:
        return x.to(dev)
    M, N = x.shape
    buf = torch.full((M + PAD_ROWS, N + cols), float("nan"), dtype=dtype, device=dev)
    buf[:M, :N] = x.to(dev)
    return buf[:M, :N]


def _out(M, N, dtype, dev, strided, cols):
    """(buffer, view [:M, :N]) of a sentinel-filled output; guard rows always, columns if strided."""
    buf = C.fill_sentinel(torch.empty(M + PAD_ROWS, N + (cols if strided else 0), dtype=dtype, device=dev))
    return buf, buf[:M, :N]


def _out1d(M, dev):
    buf = C.fill_sentinel(torch.empty(M + PAD_ROWS, dtype=F32, device=dev))
    return buf, buf[:M]


def _acc(start, dev):
    """(buffer, dense view) of an accumulation target holding `start`, 64 guard elements behind."""
    n = start.numel()
    buf = C.fill_sentinel(torch.empty(n + 64, dtype=F32, device=dev))
    view = buf[:n].view(start.shape)
    view.copy_(start.to(dev))
    return buf, view


def _guard2d(buf, M, N, what, where):
    assert C.guards_intact(buf, M, N), f"{where}: {what} written outside [:M, :N]"


def _guard1d(buf, n, what, where):
    assert C.untouched(buf[n:]), f"{where}: {what} written past its end"


def _same(got, want, what, where):
    """got (device) equals want (CPU, same dtype) element for element; a NaN (the sentinel) fails."""
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (f"{where}: {what} differs at {bad.shape[0]} elements, first index "
                              f"{bad[0].tolist()}: got {got[tuple(bad[0])].item()!r}, want "
                              f"{want[tuple(bad[0])].item()!r}")


def _within(got64, ref64, lim, what, where):
    err = (got64 - ref64).abs()
    bad = (~(err <= lim)).nonzero()   # a NaN fails
    ratio = torch.where(lim > 0, err / lim, (err > 0).double() * float("inf")).max().item()
    assert bad.numel() == 0, (f"{where}: {what} off the bound at {bad.shape[0]} elements, first index "
                              f"{bad[0].tolist()}, max err / bound = {ratio:.3g}")
    return ratio


# ------------------------------------------------------------------------------ adapter forward
STORAGE = {"bf16": (BF, F32), "x16": (BF, HF), "f16": (HF, F32)}   # (16-bit type, residual type)


def _fwd_cells():
    cells = []
    for D in P.FUSED_D:
        for m in ("M5", "full", "w1", "w2", "w3"):
            for form in ("gemm", "fused"):
                for st in (("bf16", "f16") if form == "gemm" else ("bf16", "x16", "f16")):
                    for keep in (1.0, 0.5):
                        cells.append((form, D, st, keep, m))
    return cells


FWD_CELLS = _fwd_cells()


def _run_fwd(ops, dev, form, D, st, keep, M, strided, rows=None, epoch=None):
    """One forward launch; returns the output (buffer, view) pairs by name."""
    t16, tx = STORAGE[st]
    x = P.adapter_inputs(M, D)
    fine = tx == HF and keep == 0.5   # the residual that makes this cell's half cast round
    z = _in(x["z"], t16, dev, strided, PAD_A)
    Wd, Wu = x["Wd"].to(t16).to(dev), x["Wu"].to(t16).to(dev)
    bd, bu = x["bd"].to(dev), x["bu"].to(dev)
    resid = _in(x["resid_fine" if fine else "resid"], tx, dev, strided, PAD_B)
    o = {"xout": _out(M, D, tx, dev, strided, PAD_B), "h": _out(M, P.AD_H, t16, dev, False, 0)}
    if strided:  # resid and x_out: one stride (ops.py)
        assert resid.stride() == o["xout"][1].stride()
    else:        # contiguous x_out: guard rows only, resid dense
        assert o["xout"][1].is_contiguous()
    sd = None if epoch is None else torch.tensor([epoch], dtype=torch.int64, device=dev)
    if form == "gemm":
        ops.adapter_fwd(z, Wd, bd, Wu, bu, P.SCALE, keep, P.SEED, resid, o["xout"][1], o["h"][1],
                        seed_dev=sd, rows=rows)
    else:
        o["y"] = _out(M, D, t16, dev, strided, PAD_C)
        o["mean"], o["rstd"] = _out1d(M, dev), _out1d(M, dev)
        ops.adapter_ln_fwd(z, Wd, bd, Wu, bu, P.SCALE, keep, P.SEED, resid, o["xout"][1], o["h"][1],
                           x["gamma"].to(dev), x["beta"].to(dev), o["y"][1], o["mean"][1],
                           o["rstd"][1], seed_dev=sd, rows=rows)
    torch.cuda.synchronize(dev)
    return o, fine


def _check_fwd(o, fine, form, D, st, keep, M, where, rows=None, epoch=None, exact=True):
    t16, tx = STORAGE[st]
    pre, h, xo, mask = P.adapter_fwd_ref(M, D, keep, fine, rows, epoch)
    _guard2d(o["xout"][0], M, D, "x_out", where)
    _guard2d(o["h"][0], M, P.AD_H, "h", where)
    got_h = o["h"][1].cpu()
    live = pre > 0
    badm = (((got_h != 0) != mask) & live).nonzero()
    assert badm.numel() == 0, (f"{where}: dropout mask differs from drop_mul at {badm.shape[0]} elements, "
                               f"first (row, j) = {badm[0].tolist()}")
    assert not (got_h.double()[~live] != 0).any(), f"{where}: h nonzero where pre <= 0"
    if not exact:
        return None
    _same(o["h"][1], C.exact_cast(h, t16), "h", where)
    _same(o["xout"][1], C.exact_cast(xo, tx), "x_out", where)
    if form != "fused":
        return None
    for k, n in (("y", D),):
        _guard2d(o[k][0], M, n, k, where)
    _guard1d(o["mean"][0], M, "mean", where)
    _guard1d(o["rstd"][0], M, "rstd", where)
    x = P.adapter_inputs(M, D)
    gam, bet = x["gamma"].double(), x["beta"].double()
    stored = o["xout"][1].cpu().double()       # the LayerNorm reads x_out as stored
    ref = P.ln_fwd_ref(stored, gam, bet)
    b_mean, b_rstd, b_y = P.ln_fwd_bounds(stored, gam, bet, ref, t16)
    return max(_within(o["mean"][1].cpu().double(), ref[0], b_mean, "mean", where),
               _within(o["rstd"][1].cpu().double(), ref[1], b_rstd, "rstd", where),
               _within(o["y"][1].cpu().double(), ref[2], b_y, "y", where))


def _fwd_id(c):
    form, D, st, keep, m = c
    return f"{form}-D{D}-{st}-keep{keep:g}-{m}"


@pytest.mark.parametrize("cell", FWD_CELLS, ids=_fwd_id)
def test_adapter_fwd(ops, dev, cus, cell):
    form, D, st, keep, m = cell
    M = P.adapter_fwd_rows(cus)[m]
    ratios = []
    for strided in (False, True):
        o, fine = _run_fwd(ops, dev, form, D, st, keep, M, strided)
        ratios.append(_check_fwd(o, fine, form, D, st, keep, M,
                                 f"{_fwd_id(cell)} M={M} strided={strided}"))
    if form == "fused":
        record(test="peft_matrix", kernel="adapter_ln_fwd", cell=_fwd_id(cell), M=M,
               max_err_over_bound=max(ratios))


@pytest.mark.parametrize("form", ("gemm", "fused"))
def test_adapter_fwd_row_ids(ops, dev, cus, form):
    """rows = (mul, add): row m draws the mask of row m mul + add (the _rows entry points)."""
    D, st, keep = 768, "bf16", 0.5
    M = P.adapter_fwd_rows(cus)["w2"]
    for strided in (False, True):
        o, fine = _run_fwd(ops, dev, form, D, st, keep, M, strided, rows=ROW_IDS)
        _check_fwd(o, fine, form, D, st, keep, M, f"{form} rows={ROW_IDS} M={M} strided={strided}",
                   rows=ROW_IDS)
    other = P.adapter_fwd_ref(M, D, keep)[3]
    assert (P.adapter_fwd_ref(M, D, keep, False, ROW_IDS)[3] != other).any()


@pytest.mark.parametrize("form", ("gemm", "fused"))
def test_adapter_fwd_seed_dev(ops, dev, cus, form):
    """The device-side epoch: seed += epoch * 0xD1B54A32D192ED03 in gemm.hip's EPI_AD_DOWN and in
    peft.hip's fused forward alike, against drop_keep(..., seed_dev=epoch)."""
    D, st, keep = 768, "bf16", 0.5
    M = P.adapter_fwd_rows(cus)["w2"]
    for strided in (False, True):
        o, fine = _run_fwd(ops, dev, form, D, st, keep, M, strided, epoch=EPOCH)
        _check_fwd(o, fine, form, D, st, keep, M, f"{form} seed_dev={EPOCH} M={M} strided={strided}",
                   epoch=EPOCH)
    m0, m5 = P.adapter_fwd_ref(M, D, keep)[3], P.adapter_fwd_ref(M, D, keep, False, None, EPOCH)[3]
    assert (m0 != m5).float().mean().item() > 0.4   # another epoch, another mask
    # epoch 0 on the device is the plain seed
    o, fine = _run_fwd(ops, dev, form, D, st, keep, M, False, epoch=0)
    _check_fwd(o, fine, form, D, st, keep, M, f"{form} seed_dev=0 M={M}")


@pytest.mark.parametrize("form", ("gemm", "fused"))
def test_adapter_fwd_keep_09_mask(ops, dev, cus, form):
    """keep = 0.9: 1 / keep is not exact, so only the mask is pinned (bit for bit) and the guards."""
    D, st, keep = 512, "bf16", 0.9
    M = P.adapter_fwd_rows(cus)["w2"]
    for strided in (False, True):
        o, fine = _run_fwd(ops, dev, form, D, st, keep, M, strided)
        _check_fwd(o, fine, form, D, st, keep, M, f"{form} keep=0.9 M={M} strided={strided}", exact=False)
    mask = P.adapter_fwd_ref(M, D, keep)[3]
    assert 0.88 < mask.float().mean().item() < 0.92


# ----------------------------------------------------------------------------- adapter backward
def _bwd_cells():
    cells = []
    for D in P.FUSED_D:
        for m in ("M37", "M1031", "full2", "w1", "w2", "w3", "w4"):
            for form in ("fused", "gemm", "g16"):
                for with_dz in (True, False):
                    cells.append((form, D, with_dz, m, "bf16"))
            cells.append(("fused", D, True, m, "f16"))
    return cells


BWD_CELLS = _bwd_cells()


def _set_form(st, fused):
    from lcclip import _lib
    lib = _lib.load()
    fn = lib.lc_adapter_bwd_set_form if st == "bf16" else lib.lc_adapter_bwd_set_form_f16
    assert fn(int(fused)) == 0


def _run_bwd(ops, dev, form, D, with_dz, M, st, strided):
    t16 = STORAGE[st][0]
    x = P.adapter_inputs(M, D)
    h = P.adapter_bwd_ref(M, D)[0]
    gout = _in(x["gout"], HF if form == "g16" else t16, dev, strided, PAD_A)
    hd = C.exact_cast(h, t16).to(dev)
    WuT = x["Wu"].t().contiguous().to(t16).to(dev)   # [64, D]
    WdT = x["Wd"].t().contiguous().to(t16).to(dev)   # [D, 64]
    dpre = _out(M, P.AD_H, t16, dev, False, 0)
    dz = _out(M, D, t16, dev, strided, PAD_B) if with_dz else None
    try:
        _set_form(st, form != "gemm")
        ops.adapter_bwd(gout, hd, WuT, WdT, P.SCALE, P.BWD_KEEP, dpre[1], dz[1] if with_dz else None)
        torch.cuda.synchronize(dev)
    finally:
        _set_form(st, True)   # process-wide: restored even if the launch raised
    return dpre, dz


def _bwd_id(c):
    form, D, with_dz, m, st = c
    return f"{form}-D{D}-{'dz' if with_dz else 'dpre'}-{m}-{st}"


@pytest.mark.parametrize("cell", BWD_CELLS, ids=_bwd_id)
def test_adapter_bwd(ops, dev, cus, cell):
    form, D, with_dz, m, st = cell
    M = P.adapter_bwd_rows(cus)[m]
    t16 = STORAGE[st][0]
    _, dpre64, dz64 = P.adapter_bwd_ref(M, D)
    for strided in (False, True):
        where = f"{_bwd_id(cell)} M={M} strided={strided}"
        dpre, dz = _run_bwd(ops, dev, form, D, with_dz, M, st, strided)
        _guard2d(dpre[0], M, P.AD_H, "dpre", where)
        _same(dpre[1], C.exact_cast(dpre64, t16), "dpre", where)
        if with_dz:
            _guard2d(dz[0], M, D, "dz", where)
            _same(dz[1], C.exact_cast(dz64, t16), "dz", where)


@pytest.mark.parametrize("D", P.FUSED_D)
@pytest.mark.parametrize("m", ("M1031", "full2", "w1", "w2", "w3", "w4"))
def test_adapter_bwd_forms_agree(ops, dev, cus, D, m):
    """The one-pass walker and the two-GEMM form give the same bits (both equal the reference
    above; compared with each other as well, as the existing tests do)."""
    M = P.adapter_bwd_rows(cus)[m]
    a = _run_bwd(ops, dev, "fused", D, True, M, "bf16", False)
    b = _run_bwd(ops, dev, "gemm", D, True, M, "bf16", False)
    for (_, x), (_, y), what in ((a[0], b[0], "dpre"), (a[1], b[1], "dz")):
        bad = (C.as_int(x) != C.as_int(y)).nonzero()
        assert bad.numel() == 0, f"D={D} M={M}: {what} of the two forms differs first at {bad[0].tolist()}"


# ----------------------------------------------------------------------- adapter weight gradients
WGRAD_FORMS = ("ws", "atomic", "gscale", "g16", "ws-f16")
GSCALE = 2.0 ** 12


@pytest.mark.parametrize("D", P.FUSED_D)
@pytest.mark.parametrize("m", tuple(P.WGRAD_ROWS))
@pytest.mark.parametrize("form", WGRAD_FORMS)
def test_adapter_wgrad(ops, dev, form, m, D):
    """dWu, dbu, dWd, dbd from nonzero start values: the workspace form, the atomic form, the
    forms that divide a power-of-two scale out again (bf16 and half gout), the IEEE-half build."""
    M = P.WGRAD_ROWS[m]
    t16 = HF if form == "ws-f16" else BF
    x = P.adapter_inputs(M, D)
    h64, dpre64, _ = P.adapter_bwd_ref(M, D)
    want = [t.to(F32) for t in P.adapter_wgrad_ref(M, D)]
    for t, w in zip(P.adapter_wgrad_ref(M, D), want):
        assert torch.equal(w.double(), t)
    s = GSCALE if form in ("gscale", "g16") else 1.0
    h, dpre = C.exact_cast(h64, t16).to(dev), C.exact_cast(dpre64 * s, t16).to(dev)
    for strided in (False, True):
        where = f"wgrad {form} D={D} M={M} strided={strided}"
        gout = _in(x["gout"] * s, HF if form == "g16" else t16, dev, strided, PAD_A)
        z = _in(x["z"], t16, dev, strided, PAD_C)
        outs = [_acc(x[k], dev) for k in ("dWu0", "dbu0", "dWd0", "dbd0")]
        views = [v for _, v in outs]
        if form == "atomic":
            from lcclip._lib import call, ptr, stream_of
            call("lc_adapter_wgrad", stream_of(gout), M, D, ptr(gout), gout.stride(0), ptr(h), ptr(z),
                 z.stride(0), ptr(dpre), P.SCALE, *[ptr(t) for t in views])
        else:
            gs = torch.full((1,), GSCALE, device=dev) if s != 1.0 else None
            ops.adapter_wgrad(gout, h, z, dpre, P.SCALE, *views, gscale=gs)
        torch.cuda.synchronize(dev)
        for (buf, view), w, name in zip(outs, want, ("dWu", "dbu", "dWd", "dbd")):
            _guard1d(buf, view.numel(), name, where)
            _same(view, w, name, where)


# --------------------------------------------------------------------------------- LoRA one-pass
def _lora_cells():
    cells = []
    for K, N in P.LORA_KN:
        for m in ("M1", "M31", "w1", "w2", "w3", "full2"):
            cells.append((K, N, 4, m))
            if (K, N) == P.LORA_KN[1] and m in ("M31", "w1", "w2"):
                cells += [(K, N, r, m) for r in (1, 2, 3)]
    return cells


LORA_CELLS = _lora_cells()


def _run_lora(ops, dev, K, N, r, M, strided, t16=BF, gscale=None):
    x = P.lora_inputs(M, K, N)
    s = 1.0 if gscale is None else gscale
    dY = _in(x["dY"] * s, t16, dev, strided, PAD_C)
    X = _in(x["X"], t16, dev, strided, PAD_A)
    a, bt = torch.zeros(16, K), torch.zeros(16, N)   # rows >= r zero: the caller's invariant
    a[:r], bt[:r] = x["A"][:r], x["Bt"][:r]
    a_pad, bt_pad = _in(a, t16, dev, strided, PAD_A), _in(bt, t16, dev, strided, PAD_B)
    dA, dB = _acc(x["dA0"][:r].contiguous(), dev), _acc(x["dB0"][:, :r].contiguous(), dev)
    gs = None if gscale is None else torch.full((1,), gscale, device=dev)
    ops.lora_grad_1p(dY, X, a_pad, bt_pad, r, P.LORA_S, dA[1], dB[1], gscale=gs)
    torch.cuda.synchronize(dev)
    return dA, dB


def _check_lora(dA, dB, K, N, r, M, where):
    wA, wB = P.lora_ref(M, K, N, r)
    # dA is [r, K] and dB [N, r] dense: rows >= r / columns >= r do not exist, and what follows
    # the arrays in memory is untouched
    assert tuple(dA[1].shape) == (r, K) and tuple(dB[1].shape) == (N, r)
    _guard1d(dA[0], r * K, "dA", where)
    _guard1d(dB[0], N * r, "dB", where)
    _same(dA[1], C.exact_cast(wA, F32), "dA", where)
    _same(dB[1], C.exact_cast(wB, F32), "dB", where)


def _lora_id(c):
    K, N, r, m = c
    return f"K{K}-N{N}-r{r}-{m}"


@pytest.mark.parametrize("cell", LORA_CELLS, ids=_lora_id)
def test_lora_grad_1p(ops, dev, cus, cell):
    K, N, r, m = cell
    M = P.lora_rows(cus)[m]
    for strided in (False, True):
        dA, dB = _run_lora(ops, dev, K, N, r, M, strided)
        _check_lora(dA, dB, K, N, r, M, f"{_lora_id(cell)} M={M} strided={strided}")


@pytest.mark.parametrize("variant", ("gscale", "f16"))
def test_lora_grad_1p_variants(ops, dev, cus, variant):
    """lc_lora_grad_ws_unscaled (dY carries 2^12, divided out again) and the IEEE-half build."""
    K, N, r = (P.LORA_KN[3] + (4,)) if variant == "f16" else (P.LORA_KN[1] + (3,))
    M = P.lora_rows(cus)["w2"]
    for strided in (False, True):
        dA, dB = _run_lora(ops, dev, K, N, r, M, strided, HF if variant == "f16" else BF,
                           GSCALE if variant == "gscale" else None)
        _check_lora(dA, dB, K, N, r, M, f"lora {variant} K={K} N={N} r={r} M={M} strided={strided}")
