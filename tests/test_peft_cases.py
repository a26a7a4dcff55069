"""No-GPU checks of the adapter / LoRA / LayerNorm matrices (tests/test_peft_matrix_gpu.py,
tests/test_layernorm_matrix_gpu.py): the exactness claims of peft_cases at every shape the GPU
files use (at the MI355X's 256 CUs), the float64 references against torch autograd, the dropout
mask against a big-integer restatement, the LayerNorm bounds on an f32 computation, and the tables
against peft.hip / norm.hip / gemm.hip."""
import numpy as np
import pytest
import torch

import peft_cases as P

BF, HF, F32 = P.BF, P.HF, P.F32
CUS = P.CUS_NOMINAL


def exact_in(x64, *dtypes):
    return all(torch.equal(x64.to(dt).double(), x64) for dt in dtypes)


def share_rounding(x64, dtype):
    return (x64.to(dtype).double() != x64).double().mean().item()


# ----------------------------------------------------------------------------- exactness claims
def test_row_counts():
    assert P.walker_rows(16, 256, 1) == 21 and P.walker_rows(32, 256, 4) == 24613
    assert P.walker_rows(32, 256, 3) == 16421
    for R, rows in ((P.ALN_R, P.adapter_fwd_rows(CUS)), (P.AD_R, P.adapter_bwd_rows(CUS)),
                    (P.LORA_R, P.lora_rows(CUS))):
        for name, M in rows.items():
            if not name.startswith("w"):
                continue
            d, nb = int(name[1:]), -(-M // R)
            per = [(nb - 1 - w) // CUS + 1 if w < nb else 0 for w in range(CUS)]
            # walkers 0 and 1 walk d blocks, every other one d - 1; the last block has 5 rows
            assert per[:2] == [d, d] and set(per[2:]) == {d - 1} and M - (nb - 1) * R == 5
            assert (nb - 1) % CUS == 1  # the ragged block is walker 1's
    assert max(P.adapter_bwd_rows(CUS).values()) == 24613 and max(P.lora_rows(CUS).values()) == 16421
    # the bf16 entry's threshold between the two-GEMM and the one-pass backward lies inside the set
    assert sorted(P.adapter_bwd_rows(CUS).values())[0] < P.AD_BWD_FUSED_MIN_M < 1031


@pytest.mark.parametrize("D", P.FUSED_D)
def test_adapter_inputs_and_forward_are_exact(D):
    for M in sorted(set(P.adapter_fwd_rows(CUS).values()) | set(P.adapter_bwd_rows(CUS).values())
                    | set(P.WGRAD_ROWS.values())):
        x = {k: v.double() for k, v in P.adapter_inputs(M, D).items()}
        for k in ("z", "gout", "Wd", "Wu", "resid", "resid_fine"):
            assert exact_in(x[k], BF, HF) or k.startswith("resid"), k
        assert exact_in(x["resid"], HF, F32) and exact_in(x["resid_fine"], HF, F32)
        for k in ("z", "gout"):
            assert set(x[k].unique().tolist()) <= {-1.0, 0.0, 1.0}
        for k in ("Wd", "Wu"):
            assert set((8 * x[k]).unique().tolist()) <= {-1.0, 0.0, 1.0}
        for k in ("bd", "bu", "dWu0", "dbu0", "dWd0", "dbd0"):
            assert x[k].abs().max() <= 2 and torch.equal((4 * x[k]).round(), 4 * x[k]), k
        assert x["resid"].abs().max() <= 8 and torch.equal((4 * x["resid"]).round(), 4 * x["resid"])
        assert x["resid_fine"].abs().max() <= 24
        assert torch.equal((64 * x["resid_fine"]).round(), 64 * x["resid_fine"])
        if M not in P.adapter_fwd_rows(CUS).values():
            continue
        for keep in (1.0, 0.5):
            for fine in (False, True):
                pre, h, xo, mask = P.adapter_fwd_ref(M, D, keep, fine)
                assert pre.abs().max() < P.PRE_MAX and h.max() < P.H_MAX
                assert exact_in(h, BF, HF) and exact_in(xo, F32)
                assert torch.equal((h == 0) | (pre <= 0), ~mask | (pre <= 0))
            # the cells' half x_out does round: keep 1 on the plain residual, keep 1/2 on the fine one
            xo = P.adapter_fwd_ref(M, D, keep, keep < 1)[2]
            if M * D >= 1000:
                assert share_rounding(xo, HF) > 0.01, (M, D, keep)
        # at keep 1/2 the plain residual would leave the half cast untested (see peft_cases)
        assert share_rounding(P.adapter_fwd_ref(M, D, 0.5, False)[2], HF) == 0


@pytest.mark.parametrize("D", P.FUSED_D)
def test_adapter_backward_and_wgrad_are_exact(D):
    for M in sorted(set(P.adapter_bwd_rows(CUS).values()) | set(P.WGRAD_ROWS.values())):
        h, dpre, dz = P.adapter_bwd_ref(M, D)
        assert dpre.abs().max() < P.DPRE_MAX and exact_in(dpre, BF, HF) and exact_in(dz, F32)
        assert ((h == 0) <= (dpre == 0)).all()
        if M >= 1000:
            assert share_rounding(dz, BF) > 1e-4, (M, D)   # the bf16 cast of dz does round
    for M in P.WGRAD_ROWS.values():
        for t in P.adapter_wgrad_ref(M, D):               # asserts the f32 mass itself
            assert exact_in(t, F32)
        x = P.adapter_inputs(M, D)
        assert not (x["dWu0"] == 0).all() and not (x["dbd0"] == 0).all()


@pytest.mark.parametrize("K,N", P.LORA_KN)
def test_lora_is_exact(K, N):
    for M in sorted(P.lora_rows(CUS).values()):
        x = {k: v.double() for k, v in P.lora_inputs(M, K, N).items()}
        assert exact_in(x["X"], BF, HF) and exact_in(x["dY"], BF, HF)
        assert set((4 * x["A"]).unique().tolist()) <= {-1.0, 0.0, 1.0} and exact_in(x["A"], BF, HF)
        assert set((8 * x["Bt"]).unique().tolist()) <= {-1.0, 0.0, 1.0} and exact_in(x["Bt"], BF, HF)
        for r in ((1, 2, 3, 4) if (K, N) == P.LORA_KN[1] and M < 10000 else (4,)):
            dA, dB = P.lora_ref(M, K, N, r)                # asserts |XA|, |dYB| and the f32 mass
            assert tuple(dA.shape) == (r, K) and tuple(dB.shape) == (N, r)
            assert exact_in(dA, F32) and exact_in(dB, F32)
            xa = x["X"] @ x["A"][:r].t()
            assert exact_in(xa, BF) and exact_in(x["dY"] @ x["Bt"][:r].t(), BF)


# ------------------------------------------------------------------- references against autograd
def test_adapter_reference_is_autograd():
    M, D, keep = 37, 512, 0.5
    x = {k: v.double() for k, v in P.adapter_inputs(M, D).items()}
    pre, h, xo, mask = P.adapter_fwd_ref(M, D, keep)
    leaves = {k: x[k].clone().requires_grad_(True) for k in ("z", "Wd", "bd", "Wu", "bu")}
    # adapter.py: down, ReLU, dropout, up, scale, plus the block's residual and the adapter's input
    down = torch.nn.functional.linear(leaves["z"], leaves["Wd"], leaves["bd"])
    hh = torch.relu(down) * mask.double() / keep
    out = x["resid"] + leaves["z"] + P.SCALE * torch.nn.functional.linear(hh, leaves["Wu"], leaves["bu"])
    assert torch.equal(hh.detach(), h) and torch.equal(out.detach(), xo)
    down.retain_grad()
    out.backward(x["gout"])
    h2, dpre, dz = P.adapter_bwd_ref(M, D)
    assert torch.equal(h2, h)
    assert torch.equal(down.grad, dpre) and torch.equal(leaves["z"].grad, dz)
    dWu, dbu, dWd, dbd = P.adapter_wgrad_ref(M, D)
    assert torch.equal(leaves["Wu"].grad + x["dWu0"], dWu) and torch.equal(leaves["bu"].grad + x["dbu0"], dbu)
    assert torch.equal(leaves["Wd"].grad + x["dWd0"], dWd) and torch.equal(leaves["bd"].grad + x["dbd0"], dbd)


@pytest.mark.parametrize("r", (1, 4))
def test_lora_reference_is_autograd(r):
    M, K, N = 31, 512, 512
    x = {k: v.double() for k, v in P.lora_inputs(M, K, N).items()}
    A = x["A"][:r].clone().requires_grad_(True)
    B = x["Bt"][:r].t().clone().requires_grad_(True)       # [N, r]
    y = P.LORA_S * (x["X"] @ A.t()) @ B.t()                # lora.py: x A^T B^T scaling
    y.backward(x["dY"])
    dA, dB = P.lora_ref(M, K, N, r)
    assert torch.equal(A.grad + x["dA0"][:r], dA) and torch.equal(B.grad + x["dB0"][:, :r], dB)


@pytest.mark.parametrize("D", (64, 768))
def test_layernorm_reference_is_autograd(D):
    c = {k: v.double() for k, v in P.ln_inputs(5, D).items()}
    x = c["x"].clone().requires_grad_(True)
    want = torch.nn.functional.layer_norm(x, (D,), c["gamma"], c["beta"], P.EPS)
    mean, rstd, y = P.ln_fwd_ref(c["x"], c["gamma"], c["beta"])
    assert torch.allclose(y, want.detach(), rtol=1e-12, atol=1e-12)
    want.backward(c["dy"])
    dx = P.ln_bwd_ref(c["dy"], c["x"], mean, rstd, c["gamma"], c["dres"])
    # (the constant and the zero row divide by sqrt(eps): 1e-9 absolute of values up to ~1e3)
    assert torch.allclose(dx, x.grad + c["dres"], rtol=1e-10, atol=1e-9)
    assert P.EPS == float(np.float32(1e-5)) and abs(P.EPS - 1e-5) < 1e-12
    # the special rows are what the docstring says
    assert torch.equal(c["x"][-2], torch.full((D,), 2.0, dtype=torch.float64)) and not c["x"][-1].any()
    assert abs(c["x"][-4].mean().item() - 100) < 1 and c["x"][-3].max().item() == 200


@pytest.mark.parametrize("D", P.LN_D)
def test_layernorm_bounds_hold_for_an_f32_computation(D):
    """A plain f32 LayerNorm (torch's, another summation order) lies inside the bounds, and the
    bounds are tight enough to mean something: a relative error of 2^-12 of y (half a bf16 step
    in an f32 output) or 2^-16 of rstd lies outside."""
    c = P.ln_inputs(333, D)
    x, gam, bet = c["x"].double(), c["gamma"].double(), c["beta"].double()
    ref = P.ln_fwd_ref(x, gam, bet)
    b_mean, b_rstd, b_y = P.ln_fwd_bounds(x, gam, bet, ref, F32)
    y32 = torch.nn.functional.layer_norm(c["x"], (D,), c["gamma"], c["beta"], 1e-5).double()
    assert ((y32 - ref[2]).abs() <= b_y).all()
    m32 = c["x"].mean(1).double()
    assert ((m32 - ref[0]).abs() <= b_mean).all()
    ordinary = slice(0, 329)
    assert not ((ref[2] * 2.0 ** -12).abs() <= b_y)[ordinary].all()
    assert (b_rstd / ref[1] < 2.0 ** -16)[ordinary].all() and (b_mean[ordinary] < 1e-4).all()
    # backward: torch f32 autograd against the reference on the f32 statistics
    mean32, rstd32 = ref[0].float().double(), ref[1].float().double()
    dy = c["dy"].double()
    dref = P.ln_bwd_ref(dy, x, mean32, rstd32, gam)
    b_dx = P.ln_bwd_bound(dy, x, mean32, rstd32, gam, dref, F32)
    xr = c["x"].clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (D,), c["gamma"], c["beta"], 1e-5).backward(c["dy"])
    # torch recomputes its own statistics: only rows whose f32 statistics it reproduces to a few
    # ulp are comparable, and the bound has no term for that; the ordinary rows are within 16 x
    assert ((xr.grad.double() - dref).abs() <= 16 * b_dx)[ordinary].all()
    assert not ((dref * 2.0 ** -12).abs() <= b_dx)[ordinary].all()


# ------------------------------------------------------------------------------- the dropout mask
def _hash_py(seed, idx):
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return z >> 32


def _keep_py(seed, row, j, keep, epoch=None):
    m = (1 << 64) - 1
    if epoch is not None:
        seed = (seed + epoch * 0xD1B54A32D192ED03) & m
    u = np.float32(_hash_py(seed & m, (row * 64 + j) & m) >> 8) * np.float32(1.0 / 16777216.0)
    return bool(u < np.float32(keep))


def test_drop_keep_equals_big_integer_restatement():
    rows = [0, 1, 15, 16, 17, 31, 32, 4095, 4096, 50431, 50 * 197 + 3, (1 << 31) + 5]
    for seed in (0, 1234, P.SEED, (1 << 64) - 1):
        for keep in (0.9, 0.5):
            for epoch in (None, 0, 1, 77, (1 << 63) + 12345):
                got = P.drop_keep(seed, rows, keep, epoch)
                want = [[_keep_py(seed, r, j, keep, epoch) for j in range(64)] for r in rows]
                assert got.tolist() == want, (seed, keep, epoch)
    assert P.drop_keep(P.SEED, rows, 1.0).all() and P.drop_keep(P.SEED, rows, 1.0).shape == (12, 64)
    # epoch 0 is the plain seed, another epoch another mask; the row ids are what is hashed
    assert (P.drop_keep(P.SEED, rows, 0.5, 0) == P.drop_keep(P.SEED, rows, 0.5)).all()
    assert (P.drop_keep(P.SEED, rows, 0.5, 3) != P.drop_keep(P.SEED, rows, 0.5)).any()
    assert (P.drop_keep(P.SEED, P.row_ids(8, (197, 3)), 0.5)
            == P.drop_keep(P.SEED, [3 + 197 * m for m in range(8)], 0.5)).all()
    assert P.SEED_DEV_MUL == 0xD1B54A32D192ED03


@pytest.mark.parametrize("keep", (0.9, 0.5))
def test_drop_keep_rate_per_column(keep):
    n = 20000
    m = P.drop_keep(P.SEED, np.arange(n), keep)
    rate = m.mean(0)
    sd = (keep * (1 - keep) / n) ** 0.5
    assert (np.abs(rate - keep) < 4 * sd).all(), np.abs(rate - keep).max() / sd
    # no period of one row block: rows 16 (32) apart do not share their mask
    for step in (16, 32):
        assert (m[:-step] != m[step:]).mean() > 0.1


# ------------------------------------------------------------------------ tables against the source
def test_tables_match_the_source():
    t = P.parse_tables()
    assert t["ln_f"] == P.LN_V and t["ln_b"] == P.LN_V and P.LN_D == (64, 128, 256, 512, 768, 1024)
    assert t["lora"] == P.LORA_KT_NC
    assert P.LORA_KN == ((768, 2304), (768, 768), (512, 1536), (512, 512))
    # the fused forward, the half-gradient backward and the bf16 backward's route
    assert len(t["fused_d"]) == 3 and all(d == P.FUSED_D for d in t["fused_d"])
    assert t["ad_mt"] == [P.AD_R // 16] and t["ad_r_is_16_mt"] == 1 and t["ad_ns"] == [P.AD_NS]
    assert t["ad_h"] == [P.AD_H]
    # the 16-row block of adapter_ln_fwd_kernel and the 32-row block of lora_grad1p_kernel: once
    # in the kernel, once in its launcher
    assert t["aln_blocks"] == 2 and P.ALN_R == 16
    assert t["lora_blocks"] == 2 and P.LORA_R == 32
    assert t["ad_bwd_min_m"] == [P.AD_BWD_FUSED_MIN_M]
    # gemm.hip's EPI_AD_DOWN and peft.hip's fused forward advance the seed alike
    assert t["seed_dev_mul"] == [P.SEED_DEV_MUL, P.SEED_DEV_MUL]


def test_gpu_matrix_cells_cover_the_tables():
    import test_layernorm_matrix_gpu as L
    import test_peft_matrix_gpu as G
    assert {c[1] for c in G.FWD_CELLS} == set(P.FUSED_D) and {c[0] for c in G.FWD_CELLS} == {"gemm", "fused"}
    assert {c[2] for c in G.FWD_CELLS if c[0] == "fused"} == {"bf16", "x16", "f16"}
    assert {c[4] for c in G.FWD_CELLS} == set(P.adapter_fwd_rows(CUS))
    assert {c[3] for c in G.BWD_CELLS} == set(P.adapter_bwd_rows(CUS))
    assert {(K, N) for K, N, r, m in G.LORA_CELLS} == set(P.LORA_KN)
    assert {r for K, N, r, m in G.LORA_CELLS} == {1, 2, 3, 4}
    assert {m for K, N, r, m in G.LORA_CELLS} == set(P.lora_rows(CUS))
    assert {c[0] for c in L.CELLS} == set(P.LN_D) and {c[1] for c in L.CELLS} == set(P.LN_ROWS)
