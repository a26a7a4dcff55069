"""The step-tail kernel matrix on the MI355X: csrc/head.hip (normalise, logit head, softmax backward,
feature gradient, loss scale) and the AdamW / finite-check / counter block of csrc/peft.hip, each
cell elementwise against the float64 references and derived bounds of tests/tail_cases.py, or bit
for bit on its exact cases. Every bounded cell asserts error / bound <= 1; each test appends its
worst ratio per kernel to the suite's parity_metrics.jsonl (kernel, cell, ratio) through
test_mvp_gpu.py's record().

Route -> cell, checked against the dispatch conditions in the launchers:

  lc_head_feat_grad   v4 = E % 4 == 0 && (other_n | self_n | dF | dn_ext) 16-B aligned
    head_feat_grad4_kernel      test_feat_grad[*-4|512|1024-aligned], with and without dn_ext
    head_feat_grad_kernel       E % 4 != 0: test_feat_grad[*-37|510-aligned]
                                one pointer off 16 B: test_feat_grad[*-512-dF|self_n|other_n|dn_ext]
    dn_ext == NULL / given      the `ext` loop of every test_feat_grad cell
    (sr, sc) = (Co, 1), (1, R)  orient img / txt of every test_feat_grad cell
    Co = 1, zero dlogits        test_feat_grad_dn_ext_alone (the module path's normalisation backward)
  lc_clip_head        one kernel; y outside [0, C): test_head_label_out_of_range
                      dynamic LDS (E + C) * 4 at its maximum: test_head_lds_maximum
                      C < 64, = 64, > 64 (lane tail), C = 1: test_head[C-E]
  lc_head_logits      probs given: test_head; probs == NULL: test_head_logits_exact
  lc_l2norm_rows      ldf = E and ldf = E + 8: test_l2norm[E]
  lc_grad_pow2_normalize   v4 = x 16-B aligned, n4 = n / 4, scalar tail 4 n4 .. n
    16-B loop + tail            test_loss_scale[*] n in {5, 1023, 4099} (n % 4 != 0), aligned
    16-B loop alone             n in {4, 5120}
    tail alone (n < 4)          n in {1, 3}
    unaligned, all scalar       the `[1:]` views of test_loss_scale[*]
    k clamped at 127 / -126     max 2^-140 .. 2^-120 at target 10 / 100; max 2^100, 1.5 2^127 at -100
    subnormal maximum           max 2^-140 (unclamped at target -100: the exponent must be the true one)
    s = 1                       test_loss_scale_zero_inf_nan
  lc_adamw            bias corrections from `step` (host) or *step_dev (device); *skip != 0 returns
    host step                   test_adamw[n-warm-t] (its "host" pass), test_adamw_exact[*]
    step_dev                    test_adamw[n-warm-t] (its "dev" pass), test_adamw_exact[*],
                                test_update_sequence_*
    skip                        test_adamw_skip_is_boolean, test_update_sequence_*
    more than one grid sweep    n = 4096 * 256 + 77 in test_adamw, test_check_finite
  lc_add_unscaled     1 .. 20 blocks: the way back of every test_loss_scale cell; past the 1024-block
                      grid cap: test_loss_scale_past_one_grid_sweep
  lc_counter_add / lc_adam_step_advance     test_counters
"""
import math

import pytest
import torch

import tail_cases as T
from test_mvp_gpu import record

pytestmark = pytest.mark.gpu
F32, F64 = T.F32, T.F64
NAN = float("nan")


@pytest.fixture
def worst(request):
    """kernel -> (worst error / bound ratio of this test, its cell); recorded when the test ends,
    whether it passed or not."""
    w = {}
    yield w
    for kernel, (r, cell, rn) in sorted(w.items()):
        record(test="step_tail", item=request.node.name, kernel=kernel, ratio=r, cell=cell,
               ratio_normal=rn)


def bounded(worst, kernel, cell, got, ref, bound):
    """Asserts max |got - ref| / bound <= 1. Recorded with it: the same maximum over the elements
    with |ref| >= 2^-100 only (ratio_normal), since an element whose exp the hardware flushes to
    zero just below 2^-126 sits at ratio ~1 by construction of the bound's absolute floor."""
    r = T.ratio(got, ref, bound)
    got = torch.as_tensor(got).detach().cpu()
    big = ref.abs() >= 2.0 ** -100
    rn = T.ratio(got[big], ref[big], bound[big]) if big.any() else 0.0
    old = worst.get(kernel, (0.0, "", 0.0))
    worst[kernel] = (max(r, old[0]), str(cell) if r >= old[0] else old[1], max(rn, old[2]))
    assert r <= 1.0, (kernel, cell, r)


@pytest.fixture(scope="module")
def ops(dev):
    from lcclip import ops as _ops
    return _ops


def off16(t, dev):
    """A copy of t on the device that starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---------------------------------------------------------------------------------------- head
def run_head(ops, dev, c, cell):
    img, txt, ls, y = (c[k].to(dev) for k in ("img_n", "txt_n", "ls", "y"))
    B, C = img.shape[0], txt.shape[0]
    probs = torch.full((B, C), NAN, device=dev)
    dlog = torch.full((B, C), NAN, device=dev)
    loss = torch.zeros(1, device=dev)
    ops.clip_head(img, txt, ls, y, probs, dlog, loss)
    one = loss.clone()
    ops.clip_head(img, txt, ls, y, probs, dlog, loss)          # *loss accumulates
    lg = torch.full((B, C), NAN, device=dev)
    pr = torch.full((B, C), NAN, device=dev)
    ops.head_logits(img, txt, ls, lg, pr)
    return dict(probs=probs, dlogits=dlog, loss=one[0], loss2=loss[0], logits=lg, probs_m=pr)


@pytest.mark.parametrize("E", T.HEAD_E)
@pytest.mark.parametrize("C", T.HEAD_C)
def test_head(ops, dev, worst, C, E):
    for B in T.HEAD_B:
        for ls in T.HEAD_LS:
            c = T.head_case(B, C, E, ls)
            cell = (B, C, E, round(ls, 2))
            got = run_head(ops, dev, c, cell)
            ref, bnd = T.head_ref(**c), T.head_bounds(**c)
            bounded(worst, "head_rows.probs", cell, got["probs"], ref["probs"], bnd["probs"])
            bounded(worst, "head_rows.dlogits", cell, got["dlogits"], ref["dlogits"],
                    bnd["dlogits"])
            bounded(worst, "head_rows.loss", cell, got["loss"], ref["loss"], bnd["loss"])
            bounded(worst, "head_rows.loss_twice", cell, got["loss2"], 2 * ref["loss"],
                    T.head_bounds(**c, calls=2)["loss"])
            bounded(worst, "head_logits.logits", cell, got["logits"], ref["logits"], bnd["logits"])
            bounded(worst, "head_logits.probs", cell, got["probs_m"], ref["probs"], bnd["probs"])
    # softmax backward on stored probabilities and a random upstream gradient
    for B in T.HEAD_B:
        p, dp = T.softmax_bwd_case(B, C)
        dl = torch.full((B, C), NAN, device=dev)
        ops.softmax_bwd_rows(p.to(dev), dp.to(dev), dl)
        bounded(worst, "softmax_bwd", (B, C), dl, T.softmax_bwd_ref(p, dp),
                T.softmax_bwd_bound(p, dp))
        p, dp = T.softmax_bwd_integer_case(B, C)
        ops.softmax_bwd_rows(p.to(dev), dp.to(dev), dl)
        assert torch.equal(dl.cpu().double(), T.softmax_bwd_ref(p, dp)), (B, C)


def test_head_lds_maximum(ops, dev, worst):
    """C = 8192, E = 1024: the dynamic LDS request (E + C) * 4 = 36 864 B, 128 classes per lane."""
    c = T.head_case(2, T.C_MAX, T.E_MAX, T.LS_100)
    got = run_head(ops, dev, c, "max")
    ref, bnd = T.head_ref(**c), T.head_bounds(**c)
    for k, name in (("probs", "head_rows.probs"), ("dlogits", "head_rows.dlogits"),
                    ("loss", "head_rows.loss"), ("logits", "head_logits.logits"),
                    ("probs_m", "head_logits.probs")):
        r = "probs" if k == "probs_m" else k
        bounded(worst, name, (2, T.C_MAX, T.E_MAX), got[k], ref[r], bnd[r])
    c = T.logits_integer_case(2, T.C_MAX, T.E_MAX)
    lg = torch.full((2, T.C_MAX), NAN, device=dev)
    ops.head_logits(c["img_n"].to(dev), c["txt_n"].to(dev), c["ls"].to(dev), lg, None)
    assert torch.equal(lg.cpu().double(), c["img_n"].double() @ c["txt_n"].double().t())
    p, dp = T.softmax_bwd_integer_case(3, T.C_MAX)
    dl = torch.full((3, T.C_MAX), NAN, device=dev)
    ops.softmax_bwd_rows(p.to(dev), dp.to(dev), dl)
    assert torch.equal(dl.cpu().double(), T.softmax_bwd_ref(p, dp))


def test_head_label_out_of_range(ops, dev, worst):
    """Labels -1 and C: that row of dlogits and the loss are NaN; probs of every row and the
    other rows of dlogits are untouched by it and inside their bounds."""
    B, C, E = 4, 65, 37
    c = T.head_case(B, C, E, T.LS_CLIP)
    good = dict(c)
    bad_y = c["y"].clone()
    bad_y[1], bad_y[3] = -1, C
    c["y"] = bad_y
    got = run_head(ops, dev, c, "bad-label")
    ref, bnd = T.head_ref(**good), T.head_bounds(**good)
    assert torch.isnan(got["loss"]) and torch.isnan(got["loss2"])
    assert torch.isnan(got["dlogits"][[1, 3]]).all()
    bounded(worst, "head_rows.probs", "bad-label", got["probs"], ref["probs"], bnd["probs"])
    keep = [0, 2]
    bounded(worst, "head_rows.dlogits", "bad-label", got["dlogits"][keep], ref["dlogits"][keep],
            bnd["dlogits"][keep])
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.check_finite(got["dlogits"], flag)
    assert flag.item() == 1


@pytest.mark.parametrize("C", (2, 64, 128, 256))
def test_head_uniform_rows_exact(ops, dev, C):
    for B in (1, 4, 64):
        c = T.uniform_case(B, C)
        got = run_head(ops, dev, c, "uniform")
        assert torch.equal(got["probs"].cpu(), c["probs_exact"]), (B, C)
        assert torch.equal(got["probs_m"].cpu(), c["probs_exact"]), (B, C)
        assert torch.equal(got["dlogits"].cpu(), c["dlogits_exact"]), (B, C)


@pytest.mark.parametrize("label_hot", (True, False))
def test_head_saturated_rows_exact(ops, dev, label_hot):
    for C, E in ((2, 4), (65, 37), (256, 512)):
        c = T.saturated_case(C, E, label_hot)
        got = run_head(ops, dev, c, "saturated")
        assert torch.equal(got["probs"].cpu(), c["probs_exact"]), (C, E)
        assert torch.equal(got["dlogits"].cpu(), c["dlogits_exact"]), (C, E)
        assert torch.isfinite(got["loss"]) and torch.isfinite(got["logits"]).all()


def test_head_logits_exact(ops, dev):
    """Integer data, logit_scale = 0, probs == NULL (the logits-only route)."""
    for B, C, E in ((1, 1, 4), (3, 65, 37), (64, 200, 512), (3, 256, 1024)):
        c = T.logits_integer_case(B, C, E)
        lg = torch.full((B, C), NAN, device=dev)
        ops.head_logits(c["img_n"].to(dev), c["txt_n"].to(dev), c["ls"].to(dev), lg, None)
        assert torch.equal(lg.cpu().double(), c["img_n"].double() @ c["txt_n"].double().t())


# ---------------------------------------------------------------------------- feature gradient
def run_feat_grad(ops, dev, c, misalign=None):
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
    R, E = c["self_n"].shape
    dF = torch.full((R, E), NAN, device=dev)
    if misalign == "dF":
        dF = off16(dF, dev)
    elif misalign is not None:
        t[misalign] = off16(c[misalign], dev)
    ptrs = [t["other_n"], t["self_n"], dF] + ([t["dn_ext"]] if t["dn_ext"] is not None else [])
    route = "v4" if E % 4 == 0 and all(x.data_ptr() % 16 == 0 for x in ptrs) else "scalar"
    ops.head_feat_grad(t["dlogits"], c["sr"], c["sc"], t["other_n"], t["self_n"], t["norms"],
                       t["ls"], dF, dn_ext=t["dn_ext"])
    return dF, route


FG_CELLS = [(E, None) for E in T.FG_E_VEC + T.FG_E_SCALAR] + \
           [(512, m) for m in ("dF", "self_n", "other_n", "dn_ext")]


@pytest.mark.parametrize("E,misalign", FG_CELLS, ids=lambda v: str(v) if v else "aligned")
@pytest.mark.parametrize("orient", ("img", "txt"))
def test_feat_grad(ops, dev, worst, orient, E, misalign):
    R = T.FG_R
    want_route = "v4" if (E % 4 == 0 and misalign is None) else "scalar"
    for Co in T.FG_CO:
        for ext in (True, False):
            if misalign == "dn_ext" and not ext:
                continue
            cell = (orient, R, Co, E, misalign or "aligned", "ext" if ext else "noext")
            c = T.featgrad_integer_case(R, Co, E, orient, ext=ext)
            dF, route = run_feat_grad(ops, dev, c, misalign)
            assert route == want_route, cell
            assert torch.equal(dF.cpu().double(), T.featgrad_ref(**c)), cell
            for ls in T.HEAD_LS:
                c = T.featgrad_case(R, Co, E, orient, ls=ls, ext=ext)
                dF, route = run_feat_grad(ops, dev, c, misalign)
                assert route == want_route, cell
                bounded(worst, "head_feat_grad." + route, cell + (round(ls, 2),), dF,
                        T.featgrad_ref(**c), T.featgrad_bound(**c))


def test_feat_grad_dn_ext_alone(ops, dev, worst):
    """Co = 1 with zero dlogits: dF = (dn_ext - n (n . dn_ext)) / norm, the normalisation's
    backward on the module path."""
    for E in (512, 37):
        c = T.featgrad_case(5, 1, E, "img", zero_dlog=True)
        dF, _ = run_feat_grad(ops, dev, c)
        n, e = c["self_n"].double(), c["dn_ext"].double()
        want = (e - n * (n * e).sum(-1, keepdim=True)) / c["norms"].double()[:, None]
        assert torch.equal(want, T.featgrad_ref(**c))
        bounded(worst, "head_feat_grad.dn_ext_alone", E, dF, want, T.featgrad_bound(**c))


# -------------------------------------------------------------------------------------- l2norm
@pytest.mark.parametrize("E", (1, 37, 64, 100, 512, 1024))
def test_l2norm(ops, dev, worst, E):
    R = 6
    for pad in (0, 8):
        f = T.l2norm_exact_case(R, E)
        f[2] = 0                                    # a zero row: norm 0 and a NaN row
        buf = torch.full((R, E + pad), 7.0, device=dev)
        buf[:, :E] = f.to(dev)
        src = buf[:, :E]
        assert src.stride(0) == E + pad
        out = torch.full((R, E), 3.0, device=dev)
        norms = torch.full((R,), 3.0, device=dev)
        ops.l2norm_rows(src, out, norms)
        want_out, want_n = T.l2norm_ref(f)
        rows = [0, 1, 3, 4, 5]
        assert torch.equal(norms.cpu().double()[rows], want_n[rows]), (E, pad)
        assert torch.equal(out.cpu().double()[rows], want_out[rows]), (E, pad)
        assert norms[2].item() == 0 and torch.isnan(out[2]).all()
        # random rows inside the bound
        g = torch.randn(R, E, generator=T.gen(E + pad)) * 3
        buf[:, :E] = g.to(dev)
        ops.l2norm_rows(src, out, norms)
        ref_out, ref_n = T.l2norm_ref(g)
        b_out, b_n = T.l2norm_bounds(g)
        bounded(worst, "l2norm.out", (E, pad), out, ref_out, b_out)
        bounded(worst, "l2norm.norms", (E, pad), norms, ref_n, b_n)


# -------------------------------------------------------------------------------- finite check
@pytest.mark.parametrize("n", (1, 63, 257, T.SWEEP + 77))
def test_check_finite(ops, dev, n):
    g = torch.randn(n, generator=T.gen(n)).to(dev)
    g[0], g[n - 1] = 3.4e38, -3.4e38
    if n > 4:
        g[1], g[2] = 2.0 ** -149, -(2.0 ** -130)     # subnormals are finite
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.check_finite(g, flag)
    assert flag.item() == 0
    spots = sorted({0, n - 1} | ({T.SWEEP + 5} if n > T.SWEEP else set()))
    for bad in (float("inf"), float("-inf"), NAN):
        for i in spots:
            h = g.clone()
            h[i] = bad
            flag.zero_()
            ops.check_finite(h, flag)
            assert flag.item() == 1, (n, i, bad)
            ops.check_finite(g, flag)                # OR-ed: a clean vector leaves it set
            assert flag.item() == 1, (n, i, bad)
    flag.zero_()
    ops.check_finite(g, flag)
    assert flag.item() == 0


# --------------------------------------------------------------------------------------- AdamW
def adamw_cells():
    for n in (1, 255, 10007, T.SWEEP + 77):
        for warm in (False, True):
            for t in T.ADAM_STEPS:
                yield n, warm, t


def run_adamw(ops, dev, p, g, m, v, hp, t, path, skip=None):
    p, g, m, v = (x.clone().to(dev) for x in (p, g, m, v))
    if path == "host":
        ops.adamw(p, g, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, skip)
    else:
        ctr = torch.tensor([t], dtype=torch.int64, device=dev)
        ops.adamw(p, g, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], 1, skip,
                  step_dev=ctr)
    return p, m, v


@pytest.mark.parametrize("n,warm,t", list(adamw_cells()))
def test_adamw(ops, dev, worst, n, warm, t):
    p, g, m, v = T.adamw_case(n, warm)
    ref, bnd = T.adamw_ref(p, g, m, v, T.HP, t), T.adamw_bounds(p, g, m, v, T.HP, t)
    for path in ("host", "dev"):
        got = run_adamw(ops, dev, p, g, m, v, T.HP, t, path)
        for name, a, r, b in zip("pmv", got, ref, bnd):
            bounded(worst, f"adamw.{name}.{path}", (n, "warm" if warm else "zero", t), a, r, b)


@pytest.mark.parametrize("wd", (0.0, 0.125))
def test_adamw_exact(ops, dev, wd):
    for n in (1, 255, 10007):
        p, g, hp, want = T.adamw_exact_case(n, wd)
        z = torch.zeros(n)
        host = run_adamw(ops, dev, p, g, z, z, hp, 1, "host")
        devp = run_adamw(ops, dev, p, g, z, z, hp, 1, "dev")
        for a, b, w in zip(host, devp, want):
            assert torch.equal(a.cpu(), w) and torch.equal(b, a), (n, wd)


def test_adamw_skip_is_boolean(ops, dev):
    p, g, m, v = T.adamw_case(10007, True)
    for val in (1, 2, -1):
        skip = torch.tensor([val], dtype=torch.int32, device=dev)
        for path in ("host", "dev"):
            got = run_adamw(ops, dev, p, g, m, v, T.HP, 3, path, skip)
            for a, b in zip(got, (p, m, v)):
                assert torch.equal(a.cpu(), b), (val, path)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    assert not torch.equal(run_adamw(ops, dev, p, g, m, v, T.HP, 3, "host", zero)[0].cpu(), p)


def _update(ops, st):
    """Trainer._update's launches."""
    st["skip"].zero_()
    ops.check_finite(st["g"], st["skip"])
    ops.adam_step_advance(st["ctr"], st["skip"])
    hp = T.HP
    ops.adamw(st["p"], st["g"], st["m"], st["v"], hp["lr"], hp["b1"], hp["b2"], hp["eps"],
              hp["wd"], 1, st["skip"], step_dev=st["ctr"])


def _sequence_inputs(n):
    p0 = torch.randn(n, generator=T.gen(91))
    grads = [torch.randn(n, generator=T.gen(92 + i)) for i in range(5)]
    grads[2][n // 2] = float("inf")
    return p0, grads


def _fresh_state(dev, p0):
    n = p0.numel()
    return dict(p=p0.clone().to(dev), g=torch.zeros(n, device=dev), m=torch.zeros(n, device=dev),
                v=torch.zeros(n, device=dev), skip=torch.zeros(1, dtype=torch.int32, device=dev),
                ctr=torch.zeros(1, dtype=torch.int64, device=dev))


def _eager_sequence(ops, dev, n, worst=None):
    check = worst is not None
    p0, grads = _sequence_inputs(n)
    st = _fresh_state(dev, p0)
    t = 0
    for i, g in enumerate(grads):
        before = [st[k].clone().cpu() for k in "pmv"]
        st["g"].copy_(g)
        _update(ops, st)
        if not check:
            continue
        if i == 2:      # the non-finite gradient: nothing moves, the count included
            assert st["skip"].item() == 1 and st["ctr"].item() == t
            assert all(torch.equal(st[k].cpu(), b) for k, b in zip("pmv", before))
            continue
        t += 1
        assert st["skip"].item() == 0 and st["ctr"].item() == t
        # one step from the state the buffers held, at the step count the reference rule gives
        ref, bnd = T.adamw_ref(*before[:1], g, *before[1:], T.HP, t), \
            T.adamw_bounds(*before[:1], g, *before[1:], T.HP, t)
        for name, r, b in zip("pmv", ref, bnd):
            bounded(worst, f"adamw.{name}.sequence", (n, i), st[name], r, b)
        if i == 3:      # teeth: a count that had advanced on the skipped step lies outside
            assert T.ratio(st["p"], T.adamw_ref(*before[:1], g, *before[1:], T.HP, t + 1)[0],
                           bnd[0]) > 1
    return st


def test_update_sequence_skips_and_counts(ops, dev, worst):
    n = 10007
    st = _eager_sequence(ops, dev, n, worst)
    assert st["ctr"].item() == 4 and torch.isfinite(st["v"]).all() and torch.isfinite(st["m"]).all()
    assert T.adamw_ref_steps(*_sequence_inputs(n), T.HP)[3] == 4


def test_update_sequence_as_graph(ops, dev):
    """The same five steps as a captured graph of the single-stream chain (no branches), warmed up
    on a side stream and its state restored as Trainer.enable_graph does, replayed with the
    gradient buffer rewritten between replays: bit-identical to the eager run."""
    n = 10007
    eager = _eager_sequence(ops, dev, n)
    p0, grads = _sequence_inputs(n)
    st = _fresh_state(dev, p0)
    st["g"].copy_(grads[0])
    keys = ("p", "m", "v", "ctr")
    snap = [st[k].clone() for k in keys]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _update(ops, st)
    torch.cuda.current_stream(dev).wait_stream(side)
    for k, c in zip(keys, snap):
        st[k].copy_(c)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _update(ops, st)
    for k, c in zip(keys, snap):                    # capture launched nothing
        assert torch.equal(st[k], c)
    for i, g in enumerate(grads):
        st["g"].copy_(g)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert st["skip"].item() == (1 if i == 2 else 0)
    assert st["ctr"].item() == 4
    for k in "pmv":
        assert torch.equal(st[k], eager[k]), k


# ------------------------------------------------------------------------------------ counters
def test_counters(ops, dev):
    base = torch.arange(66, dtype=torch.int64) * 1000 - 7
    base[1] = 2 ** 32 - 1
    base[64] = -(2 ** 32)
    for n in (1, 64):
        for delta in (1, -5, 2 ** 33 + 3):
            ctr = base.clone().to(dev)
            ops.counter_add(ctr[1:1 + n], delta)
            want = base.clone()
            want[1:1 + n] += delta
            assert torch.equal(ctr.cpu(), want), (n, delta)
    assert base[1] + 1 == 2 ** 32
    with pytest.raises(Exception):
        ops.counter_add(torch.zeros(65, dtype=torch.int64, device=dev), 1)
    ctr = torch.tensor([2 ** 32 - 1], dtype=torch.int64, device=dev)
    skip = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.adam_step_advance(ctr, None)
    assert ctr.item() == 2 ** 32
    ops.adam_step_advance(ctr, skip)
    assert ctr.item() == 2 ** 32 + 1
    for val in (1, 2, -1):
        skip.fill_(val)
        ops.adam_step_advance(ctr, skip)
        assert ctr.item() == 2 ** 32 + 1


# ----------------------------------------------------------------------------------- loss scale
def _on_device(x, dev, unaligned):
    return off16(x, dev) if unaligned else x.clone().to(dev)


@pytest.mark.parametrize("amax", T.POW2_MAX, ids=lambda a: f"{a:.3g}")
def test_loss_scale(ops, dev, amax):
    s_dev = torch.empty(1, device=dev)
    for n in T.POW2_N:
        orig = T.pow2_case(n, amax)
        for target in T.POW2_TARGETS:
            for unaligned in (False, True):
                cell = (amax, n, target, unaligned)
                x = _on_device(orig, dev, unaligned)
                assert (x.data_ptr() % 16 == 0) != unaligned
                ops.grad_pow2_normalize(x, s_dev, target)
                s = T.pow2_scale_ref(orig, target)
                assert s_dev.item() == s, cell
                assert torch.equal(x.cpu().double(), orig.double() * s), cell
                y = torch.zeros(n, device=dev)
                ops.add_unscaled(y, x, s_dev)
                assert torch.equal(y.cpu(), orig), cell


def test_loss_scale_past_one_grid_sweep(ops, dev):
    """n = 1024 * 256 + 77: lc_add_unscaled's grid is capped at 1024 blocks of 256, so the last 77
    elements are a second sweep; the normalise kernel's single workgroup walks 65 float4 per thread
    and a one-element tail. y accumulates: two calls give twice the gradient, exactly."""
    n = 1024 * 256 + 77
    orig = T.pow2_case(n, 1.0)
    x = orig.clone().to(dev)
    s = torch.empty(1, device=dev)
    ops.grad_pow2_normalize(x, s, 10)
    assert s.item() == T.pow2_scale_ref(orig, 10) == 1024.0
    assert torch.equal(x.cpu(), orig * 1024)
    y = torch.zeros(n, device=dev)
    ops.add_unscaled(y, x, s)
    assert torch.equal(y.cpu(), orig)
    ops.add_unscaled(y, x, s)
    assert torch.equal(y.cpu(), 2 * orig)


def test_loss_scale_zero_inf_nan(ops, dev):
    s = torch.empty(1, device=dev)
    for n in (1, 5, 1023):
        z = torch.zeros(n, device=dev)
        ops.grad_pow2_normalize(z, s, 10)
        assert s.item() == 1.0 and not z.any()
        for bad in (float("inf"), float("-inf")):
            orig = T.pow2_case(n, T.POW2_MAX[3])
            orig[n // 2] = bad
            x = orig.clone().to(dev)
            ops.grad_pow2_normalize(x, s, 10)
            assert s.item() == 1.0 and torch.equal(x.cpu(), orig), (n, bad)
        nan = torch.full((n,), NAN, device=dev)
        ops.grad_pow2_normalize(nan, s, 10)
        assert s.item() == 1.0 and torch.isnan(nan).all()
    # a NaN beside finite values: it stays (the finite check still trips), s is the finite power of
    # two of the others, and every finite element goes there and back exactly
    for n, where in ((5, 4), (1023, 0), (1023, 1022), (4099, 2048)):
        for unaligned in (False, True):
            orig = T.pow2_case(n, T.POW2_MAX[3])
            orig[where] = NAN
            x = _on_device(orig, dev, unaligned)
            ops.grad_pow2_normalize(x, s, 10)
            want = T.pow2_scale_ref(orig, 10)
            assert s.item() == want and want == 2.0 ** round(math.log2(want)) and want > 1
            fin = torch.isfinite(orig)
            assert torch.isnan(x[where]).item() and fin.sum() == n - 1
            assert torch.equal(x.cpu()[fin].double(), orig[fin].double() * want)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            ops.check_finite(x, flag)
            assert flag.item() == 1
            y = torch.zeros(n, device=dev)
            ops.add_unscaled(y, x, s)
            assert torch.equal(y.cpu()[fin], orig[fin]) and torch.isnan(y[where]).item()
