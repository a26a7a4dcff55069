"""No-GPU checks of tests/tail_cases.py (the step-tail kernel matrix, tests/test_step_tail_gpu.py):
the premises of the exact cases in f32 arithmetic, the float64 references against torch autograd
and torch.optim.AdamW in float64, every bound against a plain f32 restatement (it must admit one)
and against the wrong variants (it must reject each on some case), and the quoted limits against
the text of head.hip / peft.hip."""
import math

import numpy as np
import pytest
import torch

import tail_cases as T

F32, F64 = T.F32, T.F64
f32 = np.float32


def inside(got, ref, bound):
    return T.ratio(got, ref, bound) <= 1.0


# ------------------------------------------------------------------ premises of the exact cases
def wave_sum_f32(terms):
    """wave_sum of a 64-lane strided f32 sum, in the kernels' order: lane l adds terms l, l + 64,
    ... one after the other, then six xor-butterfly levels."""
    lanes = np.zeros(64, dtype=f32)
    for c, t in enumerate(terms):
        lanes[c % 64] = f32(lanes[c % 64] + f32(t))
    for o in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[np.arange(64) ^ o]).astype(f32)
    assert (lanes == lanes[0]).all()
    return lanes[0]


@pytest.mark.parametrize("C", (2, 64, 128, 256))
def test_uniform_rows_premise(C):
    """Equal logits: exp(0) = 1 and the sum of C ones give p = 1 / C; C equal terms exp(1 / C) sum
    to exactly C times the term in the kernels' order, for any value of the term (three values
    tried: a correct exp and its two neighbours), so the second softmax is 1 / C too; the dot
    product of p and dp is exactly zero and dlogits is (1 / C)(1 / C - [c == y]) / B."""
    assert wave_sum_f32([1.0] * C) == f32(C) and f32(1) / f32(C) == f32(1.0 / C)
    p = f32(1.0 / C)
    e = np.exp(p).astype(f32)
    for term in (e, np.nextafter(e, f32(0)), np.nextafter(e, f32(4))):
        z2 = wave_sum_f32([term] * C)
        assert float(z2) == float(term) * C and f32(term / z2) == p
    for B in (1, 4, 64):
        invB = f32(1) / f32(B)
        for y in (0, C - 1):
            dp = [f32(f32(p - f32(c == y)) * invB) for c in range(C)]
            assert all(float(d) == (1.0 / C - (c == y)) / B for c, d in enumerate(dp))
            dot = wave_sum_f32([f32(p * d) for d in dp])
            assert dot == 0
            if y == 0:      # row 0 of the case carries label 0
                want = T.uniform_case(B, C)["dlogits_exact"][0]
                assert want.tolist() == [float(f32(p * d)) for d in dp]
    c = T.uniform_case(4, C)
    assert c["y"].tolist() == [0, C - 1, 0, C - 1]
    got = T.head_f32(c["img_n"], c["txt_n"], c["ls"], c["y"])
    assert torch.equal(got["probs"], c["probs_exact"])
    ref = T.head_ref(c["img_n"], c["txt_n"], c["ls"], c["y"])
    assert (ref["dlogits"] - c["dlogits_exact"].double()).abs().max() < 1e-15


@pytest.mark.parametrize("label_hot", (True, False))
def test_saturated_rows_premise(label_hot):
    s = float(np.exp(f32(T.LS_100)))
    assert 2 * s * (1 - 20 * T.U) > 104 and math.exp(-104) < 2.0 ** -150
    assert np.exp(f32(-2 * s * (1 - 20 * T.U))) == 0
    c = T.saturated_case(65, 37, label_hot)
    got = T.head_f32(c["img_n"], c["txt_n"], c["ls"], c["y"])
    assert torch.equal(got["probs"], c["probs_exact"])
    assert torch.equal(got["dlogits"], c["dlogits_exact"]) and torch.isfinite(got["loss"])
    ref = T.head_ref(c["img_n"], c["txt_n"], c["ls"], c["y"])
    assert ref["dlogits"].abs().max() < 1e-80
    assert (ref["probs"] - c["probs_exact"]).abs().max() < 1e-80
    assert (c["y"] == 32).all() == label_hot


def units(x, unit):
    """x / unit as integers (asserted), for the exactness premises."""
    q = x.double() / unit
    assert torch.equal(q, q.round())
    return q


def test_integer_cases_premise():
    """Every sum's mass (sum of |terms|) stays below 2^24 units of its grid: exact in any order."""
    for B, C, E in ((3, 65, 37), (2, 8192, 1024)):
        c = T.logits_integer_case(B, C, E)
        mass = c["img_n"].double().abs() @ c["txt_n"].double().abs().t()
        units(c["img_n"], 2.0 ** -3), units(c["txt_n"], 2.0 ** -3)
        assert mass.max() / 2.0 ** -6 < 2 ** 24 and c["img_n"].any() and c["txt_n"].any()
        want = c["img_n"].double() @ c["txt_n"].double().t()
        y0 = torch.zeros(B, dtype=torch.int64)
        assert torch.equal(T.head_ref(c["img_n"], c["txt_n"], c["ls"], y0)["logits"], want)
        assert torch.equal(want.float().double(), want)
    p, dp = T.softmax_bwd_integer_case(3, 8192)
    units(p, 1 / 16), units(dp, 1 / 8)
    assert (p * dp.abs()).double().sum(-1).max() / 2.0 ** -7 < 2 ** 24
    ref = T.softmax_bwd_ref(p, dp)
    assert torch.equal(ref.float().double(), ref)
    assert torch.equal(T.softmax_bwd_f32(p, dp).double(), ref)
    for orient in ("img", "txt"):
        for R, Co, E in ((3, 256, 1024), (5, 9, 37)):
            c = T.featgrad_integer_case(R, Co, E, orient)
            d = T.dlog_view(c["dlogits"], R, Co, c["sr"], c["sc"]).double()
            o, n = c["other_n"].double(), c["self_n"].double()
            dn_mass = d.abs() @ o.abs() + c["dn_ext"].double().abs()
            assert dn_mass.max() <= Co / 4 + 2 and dn_mass.max() / 2.0 ** -3 < 2 ** 24
            nd_mass = (dn_mass * n.abs()).sum(-1)
            assert nd_mass.max() / 2.0 ** -4 < 2 ** 24
            assert (dn_mass + n.abs() * nd_mass[:, None]).max() / 2.0 ** -5 < 2 ** 22
            assert set(np.log2(c["norms"].numpy()).tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
            ref = T.featgrad_ref(**c)
            assert torch.equal(ref.float().double(), ref) and ref.any()
            assert torch.equal(T.featgrad_f32(**c).double(), ref)


@pytest.mark.parametrize("E", (1, 37, 64, 100, 512, 1024))
def test_l2norm_exact_premise(E):
    f = T.l2norm_exact_case(6, E)
    out, n = T.l2norm_ref(f)
    assert set(n.tolist()) <= {4.0, 2.0} and f[0, E - 1] != 0
    assert set(out.abs().unique().tolist()) <= {0.0, 0.25, 0.5, 1.0}
    if E >= 16:
        assert set(n.tolist()) == {4.0, 2.0}


@pytest.mark.parametrize("wd", (0.0, 0.125))
def test_adamw_exact_premise(wd):
    p, g, hp, want = T.adamw_exact_case(255, wd)
    z = torch.zeros_like(p)
    for got in (T.adamw_f32(p, g, z, z, hp, 1), T.adamw_ref(p, g, z, z, hp, 1)):
        for a, b in zip(got, want):
            assert torch.equal(a.double(), b.double())
    # powf(b, 1) = b, and 1 - b is exact: the host-step and the device-step path agree bit for bit
    assert f32(1) - np.power(f32(0.5), f32(1)) == f32(0.5) and f32(1) - f32(0.75) == f32(0.25)
    assert not torch.equal(want[0], p) and (g.abs().log2().abs() <= 20).all()


def test_pow2_cases_premise():
    """x s is representable, and the way back returns x, for every (max, target) of the matrix; the
    subnormal maximum's floor(log2) is the true one; both clamps of k are reached."""
    ks = set()
    for amax in T.POW2_MAX:
        for target in T.POW2_TARGETS:
            x = T.pow2_case(1023, amax)
            assert float(x.abs().max()) == amax == float(x[-1].abs())
            assert float(x.abs().min()) >= amax / 256
            s = T.pow2_scale_ref(x, target)
            k = round(math.log2(s))
            assert s == 2.0 ** k and T.K_MIN <= k <= T.K_MAX
            ks.add(k)
            assert k == min(max(target - math.floor(math.log2(amax)), -126), 127)
            xs = x.double() * s
            assert torch.equal(xs.float().double(), xs) and torch.isfinite(xs.float()).all()
            if k < T.K_MAX and k > T.K_MIN:      # unclamped: the maximum lands in [2^t, 2^(t+1))
                assert 2.0 ** target <= float(xs.abs().max()) < 2.0 ** (target + 1)
    assert T.K_MIN in ks and T.K_MAX in ks
    assert T.floor_log2(2.0 ** -140) == -140 and T.floor_log2(1.5 * 2.0 ** 127) == 127
    assert T.floor_log2(3 * 2.0 ** -149) == -148
    nan = torch.tensor([float("nan"), 3.0, -5.0])
    assert T.pow2_scale_ref(nan, 10) == 2.0 ** 8
    assert T.pow2_scale_ref(torch.tensor([1.0, float("inf")]), 10) == 1.0
    assert T.pow2_scale_ref(torch.zeros(4), 10) == 1.0
    assert T.pow2_scale_ref(torch.full((3,), float("nan")), 10) == 1.0


# ------------------------------------------------------------------ references against autograd
@pytest.mark.parametrize("B,C,E,ls", T.HEAD_CPU_CASES[:4])
def test_head_reference_is_autograd(B, C, E, ls):
    g = T.gen(B + C + E)
    fi = torch.randn(B, E, generator=g, dtype=F64, requires_grad=True)
    ft = torch.randn(C, E, generator=g, dtype=F64, requires_grad=True)
    ext_i = torch.randn(B, E, generator=g, dtype=F64)
    y = torch.randint(0, C, (B,), generator=g)
    lsv = torch.tensor([ls], dtype=F64)
    i_n, t_n = fi / fi.norm(dim=-1, keepdim=True), ft / ft.norm(dim=-1, keepdim=True)
    logits = lsv.exp() * i_n @ t_n.t()
    logits.retain_grad()
    probs = logits.softmax(-1)
    loss = torch.nn.functional.cross_entropy(probs, y)
    (loss + (i_n * ext_i).sum()).backward()
    ni, ti = T.l2norm_ref(fi.detach())
    nt, tt = T.l2norm_ref(ft.detach())
    assert torch.allclose(ni, i_n.detach(), rtol=1e-14, atol=0)
    ref = T.head_ref(ni, nt, lsv, y)
    for k, want in (("logits", logits), ("probs", probs), ("loss", loss), ("dlogits", logits.grad)):
        assert torch.allclose(ref[k], want.detach(), rtol=1e-11, atol=1e-15), k
    dl = ref["dlogits"]
    di = T.featgrad_ref(dl, C, 1, nt, ni, ti, lsv, ext_i)
    dt = T.featgrad_ref(dl, 1, C, ni, nt, tt, lsv, None)
    assert torch.allclose(di, fi.grad, rtol=1e-9, atol=1e-14)
    assert torch.allclose(dt, ft.grad, rtol=1e-9, atol=1e-14)
    # softmax backward is the vector-Jacobian product of softmax
    p, dp = T.softmax_bwd_case(B, C)
    x = torch.randn(B, C, generator=g, dtype=F64, requires_grad=True)
    sm = x.softmax(-1)
    sm.backward(dp.double())
    assert torch.allclose(T.softmax_bwd_ref(sm.detach(), dp), x.grad, rtol=1e-11, atol=1e-15)


def test_adamw_reference_is_torch_adamw():
    """With the same double hyperparameters the float64 reference is torch.optim.AdamW in float64;
    with the f32-rounded ones the kernel receives it is off by the price of `float b2`."""
    n = 999
    hp64 = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)
    g_ = T.gen(5)
    p0 = torch.randn(n, generator=g_, dtype=F64)
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([q], lr=hp64["lr"], betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    p32, m32, v32 = p.clone(), m.clone(), v.clone()
    worst = 0.0
    for t in range(1, 11):
        g = torch.randn(n, generator=g_, dtype=F64)
        q.grad = g.clone()
        before = q.detach().clone()
        opt.step()
        p, m, v = T.adamw_ref(p, g, m, v, hp64, t)
        assert torch.allclose(p, q.detach(), rtol=1e-13, atol=1e-16), t
        new = T.adamw_ref(before, g, m32, v32, T.HP, t)
        upd64 = q.detach() - before * (1 - hp64["lr"] * hp64["wd"])
        upd32 = new[0] - before * (1 - T.HP["lr"] * T.HP["wd"])
        big = upd64.abs() > 1e-5
        worst = max(worst, ((upd32 - upd64).abs() / upd64.abs())[big].max().item())
        m32, v32 = new[1], new[2]
    # the f32 hyperparameters move the update by parts in 1e5 at most, and by more than f32 rounding
    assert 1e-7 < worst < 1e-4, worst
    assert abs((1 - T.HP["b2"] ** 2) / (1 - 0.999 ** 2) - 1) > 1e-5


def test_skip_rule_keeps_state_and_count():
    p = torch.randn(50, generator=T.gen(1))
    gs = [torch.randn(50, generator=T.gen(2 + i)) for i in range(5)]
    bad = [g.clone() for g in gs]
    bad[2][7] = float("inf")
    a = T.adamw_ref_steps(p, bad, T.HP)
    b = T.adamw_ref_steps(p, gs[:2] + gs[3:], T.HP)
    assert a[3] == 4 and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert torch.isfinite(a[2]).all()


# -------------------------------------------------- bounds: admit f32, reject the wrong variants
def head_cases():
    return [T.head_case(*c) for c in T.HEAD_CPU_CASES]


def test_head_bounds_admit_f32():
    for c in head_cases():
        ref, bnd = T.head_ref(**c), T.head_bounds(**c)
        got = T.head_f32(**c)
        for k in ("logits", "probs", "dlogits", "loss"):
            assert inside(got[k], ref[k], bnd[k]), (k, T.ratio(got[k], ref[k], bnd[k]))
        # and mean something: the relative bound of the largest probability of each row stays
        # below 1e-3 even at exp(ls) = 100
        top = ref["probs"].max(-1)
        assert (bnd["probs"].gather(1, top.indices[:, None])[:, 0] / top.values).max() < 1e-3


def test_bounds_admit_f32_on_the_whole_gpu_matrix():
    """Every general cell of test_step_tail_gpu.py's head and feature-gradient matrices."""
    for C in T.HEAD_C:
        for E in T.HEAD_E:
            for B in T.HEAD_B:
                for ls in T.HEAD_LS:
                    c = T.head_case(B, C, E, ls)
                    ref, bnd, got = T.head_ref(**c), T.head_bounds(**c), T.head_f32(**c)
                    for k in ("logits", "probs", "dlogits", "loss"):
                        assert inside(got[k], ref[k], bnd[k]), (B, C, E, ls, k)
    for orient in ("img", "txt"):
        for E in T.FG_E_VEC + T.FG_E_SCALAR:
            for Co in T.FG_CO:
                for ext in (True, False):
                    for ls in T.HEAD_LS:
                        c = T.featgrad_case(T.FG_R, Co, E, orient, ls=ls, ext=ext)
                        assert inside(T.featgrad_f32(**c), T.featgrad_ref(**c),
                                      T.featgrad_bound(**c)), (orient, Co, E, ext, ls)


@pytest.mark.parametrize("variant", T.HEAD_VARIANTS)
def test_head_bounds_reject(variant):
    caught = set()
    for c in head_cases():
        ref, bnd = T.head_ref(**c), T.head_bounds(**c)
        got = T.head_f32(**c, variant=variant)
        caught |= {k for k in ("logits", "probs", "dlogits", "loss")
                   if not inside(got[k], ref[k], bnd[k])}
    must = {"single_softmax": {"dlogits", "loss"}, "no_inv_b": {"dlogits", "loss"},
            "label_off_by_one": {"dlogits", "loss"}, "lane_tail_skipped": {"probs", "dlogits"},
            "no_max_shift": {"probs", "dlogits"}, "scale_twice": {"logits", "probs", "dlogits"}}
    assert must[variant] <= caught, (variant, caught)


def test_exact_cases_reject_head_variants():
    """The exact cases on their own catch the index slips: 1 / B, the label, the lane tail."""
    c = T.uniform_case(4, 128)
    for variant in ("no_inv_b", "label_off_by_one", "single_softmax"):
        got = T.head_f32(c["img_n"], c["txt_n"], c["ls"], c["y"], variant=variant)
        assert not torch.equal(got["dlogits"], c["dlogits_exact"]), variant


def test_softmax_bwd_bound():
    for B, C in ((1, 1), (3, 65), (4, 200), (2, 8192)):
        p, dp = T.softmax_bwd_case(B, C)
        ref, bnd = T.softmax_bwd_ref(p, dp), T.softmax_bwd_bound(p, dp)
        assert inside(T.softmax_bwd_f32(p, dp), ref, bnd)
        if C > 1:
            assert not inside(p * dp, ref, bnd)                         # the projection dropped
            skipped = p * (dp - (p[:, :C - 1] * dp[:, :C - 1]).sum(-1, keepdim=True))
            assert not inside(skipped, ref, bnd)                        # the last class not summed


def featgrad_cases():
    out = []
    for R, Co, E, orient in T.FEATGRAD_CPU_CASES:
        for ls in (T.LS_CLIP, T.LS_100):
            out.append(T.featgrad_case(R, Co, E, orient, ls=ls))
    return out


def test_featgrad_bound_admits_f32():
    for c in featgrad_cases() + [T.featgrad_case(3, 256, 1024, "txt"),
                                 T.featgrad_case(2, 1, 512, "img", zero_dlog=True),
                                 T.featgrad_case(4, 7, 510, "img", ext=False)]:
        ref, bnd = T.featgrad_ref(**c), T.featgrad_bound(**c)
        assert inside(T.featgrad_f32(**c), ref, bnd), T.ratio(T.featgrad_f32(**c), ref, bnd)
        assert (bnd < 1e-3 * ref.abs().max()).all()


@pytest.mark.parametrize("variant", T.FEATGRAD_VARIANTS)
def test_featgrad_bound_rejects(variant):
    n = 0
    for c in featgrad_cases():
        got = T.featgrad_f32(**c, variant=variant)
        n += not inside(got, T.featgrad_ref(**c), T.featgrad_bound(**c))
    assert n == len(featgrad_cases()), (variant, n)
    # and so does the exact case
    c = T.featgrad_integer_case(5, 5, 37, "img")
    assert not torch.equal(T.featgrad_f32(**c, variant=variant).double(), T.featgrad_ref(**c)) \
        or variant == "scale_twice"          # exp(0)^2 = 1: the integer case cannot see that one


def test_l2norm_bound_admits_f32():
    f = torch.randn(7, 100, generator=T.gen(3)) * 3
    out, n = T.l2norm_ref(f)
    b_out, b_n = T.l2norm_bounds(f)
    nn = f.norm(dim=-1)
    assert inside(nn, n, b_n) and inside(f / nn[:, None], out, b_out)
    assert (b_n / n).max() < 16 * T.U
    assert not inside(f / (f * f).sum(-1, keepdim=True), out, b_out)    # the root dropped


def adamw_cells():
    for n in (1, 255, 10007):
        for warm in (False, True):
            for t in T.ADAM_STEPS:
                yield n, warm, t


def test_adamw_bounds_admit_f32():
    worst = 0.0
    for n, warm, t in adamw_cells():
        p, g, m, v = T.adamw_case(n, warm)
        ref, bnd = T.adamw_ref(p, g, m, v, T.HP, t), T.adamw_bounds(p, g, m, v, T.HP, t)
        got = T.adamw_f32(p, g, m, v, T.HP, t)
        for a, r, b in zip(got, ref, bnd):
            worst = max(worst, T.ratio(a, r, b))
    assert worst <= 1.0, worst
    # teeth in numbers: where p = 0 the bound is a relative bound of the update itself, about
    # (K_bc2 / 2 + K_bc1) u at step 1 (1017 u = 6.1e-5) and a dozen u late (the median element:
    # one whose b1 m and (1 - b1) g cancel has a larger relative bound, as it must)
    p, g, m, v = T.adamw_case(10007, True)
    for t, lim in ((1, 7e-5), (1000, 1e-6)):
        ref, bnd = T.adamw_ref(p, g, m, v, T.HP, t), T.adamw_bounds(p, g, m, v, T.HP, t)
        assert (p[:128] == 0).all() and (bnd[0] / ref[0].abs())[:128].median() < lim
    assert abs(T.k_bc(T.HP["b2"], 1) / 2 + T.k_bc(T.HP["b1"], 1) - 1017) < 2


@pytest.mark.parametrize("variant", T.ADAMW_VARIANTS)
def test_adamw_bounds_reject(variant):
    caught = 0
    for n, warm, t in adamw_cells():
        p, g, m, v = T.adamw_case(n, warm)
        ref, bnd = T.adamw_ref(p, g, m, v, T.HP, t), T.adamw_bounds(p, g, m, v, T.HP, t)
        got = T.adamw_f32(p, g, m, v, T.HP, t, variant=variant)
        caught += not all(inside(a, r, b) for a, r, b in zip(got, ref, bnd))
    assert caught >= 6, (variant, caught)
    p, g, hp, want = T.adamw_exact_case(255, 0.125)
    z = torch.zeros_like(p)
    got = T.adamw_f32(p, g, z, z, hp, 1, variant=variant)
    # (the exact case has eps = 0 and m = 0: those two slips it cannot see)
    assert (not all(torch.equal(a, b) for a, b in zip(got, want))
            or variant in ("eps_inside_sqrt", "m_uses_b2"))


def test_adamw_case_holds_its_hard_elements():
    p, g, m, v = T.adamw_case(10007, True)
    assert (p[:128] == 0).all() and (g[-2:] == 0).all() and (v >= 0).all() and m.any()
    assert sorted(set(g[-14:-2].abs().tolist())) == sorted(float(f32(a)) for a in T.HARD_G)
    assert 0 < float(f32(1e-20) * f32(1e-20) * f32(1e-3)) < 2.0 ** -126      # subnormal, not zero
    assert T.adamw_case(1, False)[1].tolist() == [0.0]


# ------------------------------------------------------------------------------ source constants
def test_constants_match_the_source():
    s = T.parse_source()
    assert s["c_max"] == [T.C_MAX] * 2 and s["e_max"] == [T.E_MAX] * 3 and len(s["lds"]) == 2
    assert (T.E_MAX + T.C_MAX) * 4 <= 64 * 1024
    assert s["target"] == [-T.TARGET_MAX, T.TARGET_MAX]
    assert s["normalize_threads"] == [T.NORMALIZE_THREADS] == s["normalize_bounds"]
    assert s["k_clamp"] == [T.K_MIN, T.K_MAX]
    assert len(s["featgrad_route"]) == 1 and len(s["normalize_route"]) == 1
    assert s["ctr_max"] == [T.CTR_MAX] and s["grid_cap"] == [T.GRID_CAP]
    assert s["tail_block"] == [T.BLOCK, T.BLOCK] and T.SWEEP == 4096 * 256
    assert len(s["adamw_step_rule"]) == 1
