"""MVP-CLIP training method on the MI355X: the mvp.hip kernels against the float64 restatements
of tests/mvp_method_ref.py on identical f32 inputs, the pool_kernels switch of CLIP_MVP against
the torch path, MVPTrainer.step against the restatement composed from the oracle's forward, the
config-3 shape, and the data-parallel exchange.

Tolerance rule: each checked quantity is also computed by the same restatement in float32 on the
CPU; its error against float64 is e32, and the kernel passes when its own error is
<= 8 * e32 + 1e-6 (absolute for scores and losses, relative-norm for gradients). Measured values
are appended to the suite's parity metrics file through tests/test_mvp_gpu.py's `record`."""
import functools
import math
import os
import socket
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mvp_method_ref as R
from parity import GRAD_REL
from test_mvp_gpu import record

from oracle import clip_oracle as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("key", "mask", "g_prompts", "e_prompts")


def abs_err(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def within_rule(err, e32):
    return err <= 8 * e32 + 1e-6


# ---------------------------------------------------------------- selection + similarity loss
SELECT_SHAPES = [(1, 1, 128, 1), (3, 10, 128, 1), (65, 10, 768, 2), (5, 64, 132, 8)]


@functools.lru_cache(maxsize=None)
def select_case(B, P, W, k, with_count):
    """Seeded inputs whose float64 selection is well separated: the k-th and (k+1)-th scaled
    distances of every row differ by more than 1e-3 (the condition the test asserts), and the
    selected ones among themselves by more than 1e-4 (their order is compared too)."""
    for seed in range(4000):
        g = torch.Generator().manual_seed(1000 * B + seed)
        q = torch.randn(B, W, generator=g)
        key = torch.randn(P, W, generator=g)
        count = torch.randint(0, 5, (P,), generator=g).float() if with_count else None
        sc = R.select(q.double(), key.double(), None if count is None else count.double(), k)[2]
        s = sc.sort(dim=1).values[:, :k + 1]
        gaps = s[:, 1:] - s[:, :-1]
        if P == k or (gaps[:, k - 1].min() > 1e-3 and (k == 1 or gaps[:, :k - 1].min() > 1e-4)):
            return q, key, count
    raise AssertionError("no separated seed found")


def run_select(dev, q, key, count, k, hist=True):
    from lcclip import ops
    B, P = q.shape[0], key.shape[0]
    idx = torch.empty(B, k, dtype=torch.int64, device=dev)
    dist_ = torch.empty(B, k, device=dev)
    qn, kn = torch.empty(B, device=dev), torch.empty(P, device=dev)
    num = torch.zeros(P, dtype=torch.int64, device=dev) if hist else None
    ops.mvp_select(q.to(dev), key.to(dev), None if count is None else count.to(dev), k, idx,
                   dist_, qn, kn, num)
    torch.cuda.synchronize()
    return idx.cpu(), dist_.cpu(), None if num is None else num.cpu()


@pytest.mark.parametrize("with_count", [False, True])
@pytest.mark.parametrize("B,P,W,k", SELECT_SHAPES)
def test_select(dev, B, P, W, k, with_count):
    q, key, count = select_case(B, P, W, k, with_count)
    c64 = None if count is None else count.double()
    topk, sel, scaled, num = R.select(q.double(), key.double(), c64, k)
    if P > k:
        s = scaled.sort(dim=1).values
        assert (s[:, k] - s[:, k - 1]).min() > 1e-3
    sel32 = R.select(q, key, count, k)[1]
    e32 = abs_err(sel32, sel)
    idx, d, hist = run_select(dev, q, key, count, k)
    err = abs_err(d, sel)
    record(test="mvp_select", shape=[B, P, W, k], count=with_count, dist_err=err, e32=e32)
    assert torch.equal(idx, topk)
    assert within_rule(err, e32), (err, e32)
    assert torch.equal(hist, num)
    idx2, d2, _ = run_select(dev, q, key, count, k, hist=False)
    assert torch.equal(idx2, idx) and torch.equal(d2, d)


def test_select_rejects_unsupported_shapes(dev):
    from lcclip import LcError
    g = torch.Generator().manual_seed(0)
    for B, P, W, k in [(2, 65, 16, 1), (2, 10, 16, 9), (2, 4, 16, 5)]:
        with pytest.raises(LcError):
            run_select(dev, torch.randn(B, W, generator=g), torch.randn(P, W, generator=g), None, k)


def simloss_ref(q, key, count, k, contrastiv, dtype):
    q, key = q.to(dtype), key.detach().to(dtype).requires_grad_(True)
    c = None if count is None else count.to(dtype)
    topk, sel, _, _ = R.select(q, key, c if contrastiv else None, k)
    loss = R.simloss(key, c, topk, sel, contrastiv)
    (2.5 * loss).backward()
    return loss.detach(), key.grad


@pytest.mark.parametrize("count_kind", ["zero", "random"])
@pytest.mark.parametrize("contrastiv", [False, True])
@pytest.mark.parametrize("B,P,W,k", SELECT_SHAPES)
def test_simloss_and_dkey(dev, B, P, W, k, contrastiv, count_kind):
    from lcclip import LcError
    from lcclip import autograd as A
    # the count scales the selection only under use_contrastiv (models/mvp_clip.py:226-229)
    q, key, count = select_case(B, P, W, k, contrastiv and count_kind == "random")
    if count is None:
        count = torch.zeros(P) if count_kind == "zero" else torch.arange(P).float() % 4
    if contrastiv and k > 1:
        # models/mvp_clip.py:240-246 does not broadcast at selection sizes above 1 for a general
        # batch: the restatement raises as the reference would, and the kernel rejects the shape
        with pytest.raises(RuntimeError):
            simloss_ref(q, key, count, k, True, torch.float64)
        with pytest.raises(LcError):
            A.mvp_select_apply(key.to(dev).requires_grad_(True), q.to(dev), count.to(dev), k, True)
        return
    l64, g64 = simloss_ref(q, key, count, k, contrastiv, torch.float64)
    l32, g32 = simloss_ref(q, key, count, k, contrastiv, torch.float32)
    e_l, e_g = abs_err(l32, l64), rel_err(g32, g64)
    out = []
    for _ in range(2):
        kd = key.to(dev).requires_grad_(True)
        loss, idx, _ = A.mvp_select_apply(kd, q.to(dev), count.to(dev), k, contrastiv)
        (2.5 * loss).backward()  # the upstream scalar is read from device memory
        torch.cuda.synchronize()
        out.append((loss.detach().cpu(), kd.grad.cpu(), idx.cpu()))
    (loss, dkey, idx), again = out
    err_l, err_g = abs_err(loss, l64), rel_err(dkey, g64)
    record(test="mvp_simloss", shape=[B, P, W, k], contrastiv=contrastiv, count=count_kind,
           loss_err=err_l, loss_e32=e_l, dkey_rel=err_g, dkey_e32=e_g)
    assert within_rule(err_l, e_l), (err_l, e_l)
    assert within_rule(err_g, e_g), (err_g, e_g)
    if not contrastiv:  # unselected keys: exact zeros
        for p in range(P):
            if p not in set(idx.flatten().tolist()):
                assert dkey[p].abs().max().item() == 0.0
    assert torch.equal(again[0], loss) and torch.equal(again[1], dkey)


# ---------------------------------------------------------------- pool gather
@pytest.mark.parametrize("pattern", ["same", "never"])
@pytest.mark.parametrize("B,k,P,R_", [(5, 1, 3, 7), (5, 2, 10, 60 * 128), (128, 1, 10, 60 * 768)])
def test_pool_gather_and_backward(dev, B, k, P, R_, pattern):
    from lcclip import ops
    g = torch.Generator().manual_seed(B + R_)
    table = torch.randn(P, R_, generator=g)
    if pattern == "same" and k == 1:
        idx = torch.full((B, k), 1, dtype=torch.int64)
    elif pattern == "same":  # every image picks the same k entries
        idx = torch.tensor([1, 4]).repeat(B, 1)
    else:  # entry 0 is never picked
        idx = torch.randint(1, P, (B, k), generator=g)
    never = [p for p in range(P) if p not in set(idx.flatten().tolist())]
    assert never
    grad = torch.randn(B * k, R_, generator=g)
    td, idd, gd = table.to(dev), idx.to(dev), grad.to(dev)
    out = torch.empty(B * k, R_, device=dev)
    ops.pool_gather(td, idd, out)
    outm = torch.empty(B, R_, device=dev)
    ops.pool_gather(td, idd, outm, mean=True)
    assert torch.equal(out.cpu(), table[idx.reshape(-1)])
    assert rel_err(outm, table.double()[idx].mean(1)) < 1e-6
    ref = R.gather_bwd(idx, grad.double(), P)
    e32 = rel_err(R.gather_bwd(idx, grad, P), ref)
    res = []
    for _ in range(2):
        dt = torch.full((P, R_), float("nan"), device=dev)
        ops.pool_gather_bwd(idd, gd, dt)
        torch.cuda.synchronize()
        res.append(dt.cpu())
    err = rel_err(res[0], ref)
    # the backward of the mean: every selection of image b reads g[b], scaled by 1/k
    gm = torch.randn(B, R_, generator=g)
    dtm = torch.empty(P, R_, device=dev)
    ops.pool_gather_bwd(idd, gm.to(dev), dtm, alpha=1.0 / k, shared_s=True)
    refm = R.gather_bwd(idx, gm.double().repeat_interleave(k, 0), P, 1.0 / k)
    e32m = rel_err(R.gather_bwd(idx, gm.repeat_interleave(k, 0), P, 1.0 / k), refm)
    errm = rel_err(dtm, refm)
    record(test="mvp_pool_gather_bwd", shape=[B, k, P, R_], pattern=pattern, rel=err, e32=e32,
           rel_mean=errm, e32_mean=e32m)
    assert within_rule(err, e32), (err, e32)
    assert within_rule(errm, e32m), (errm, e32m)
    for p in never:
        assert res[0][p].abs().max().item() == 0.0
    assert torch.equal(res[0], res[1])


# ---------------------------------------------------------------- head + scores + backward
def head_case(B, C, E, exposed, seed, neg_row=False):
    g = torch.Generator().manual_seed(seed)
    i = torch.randn(B, E, generator=g)
    t = torch.randn(C, E, generator=g)
    mp_ = -1.0 + 0.5 * torch.randn(B, C + 3, generator=g)  # rows wider than C, as the pool's are
    y = torch.randint(0, exposed - 1, (B,), generator=g)     # class exposed-1 has no sample
    y[1] = y[0]
    if neg_row:  # image 2 lies on its class's text feature: cps = margin there
        i[2] = 3.0 * t[y[2]] + 0.01 * torch.randn(E, generator=g)
    cmask = torch.full((C,), float("-inf"))
    cmask[:exposed] = 0
    ls = torch.tensor(100.0).log()
    return i, t, mp_, y, cmask, ls


def head_ref(case, dtype, C, **kw):
    i, t, mp_, y, cmask, ls = case
    iv = i.detach().clone().to(dtype).requires_grad_(True)
    mv = mp_.detach().clone().to(dtype).requires_grad_(True)
    loss, ign, cps = R.method_loss(iv, t.to(dtype), mv[:, :C], cmask.to(dtype), y, ls.to(dtype),
                                   **kw)
    loss.backward()
    return loss.detach(), ign.detach(), cps.detach(), iv.grad, mv.grad


HEAD_SHAPES = [(5, 4, 64, 3), (7, 6, 64, 6), (33, 70, 512, 60)]


@pytest.mark.parametrize("mode", ["gsf_afs", "afs", "gsf", "scores_only", "afs_negative_cps"])
@pytest.mark.parametrize("B,C,E,exposed", HEAD_SHAPES)
def test_head_scores_and_backward(dev, B, C, E, exposed, mode):
    from lcclip import autograd as A
    neg = mode == "afs_negative_cps"
    kw = dict(use_afs="afs" in mode, use_gsf="gsf" in mode, alpha=0.5, gamma=2.0,
              margin=-0.5 if neg else 0.5)
    case = head_case(B, C, E, exposed, seed=B + 7, neg_row=neg)
    i, t, mp_, y, cmask, ls = case
    l64, ign64, cps64, gi64, gm64 = head_ref(case, torch.float64, C, **kw)
    l32, ign32, cps32, gi32, gm32 = head_ref(case, torch.float32, C, **kw)
    if neg:
        assert cps64[2] < 0 and (cps64[torch.arange(B) != 2] > 0).all()
    else:
        assert (cps64 > 0).all()
    st = A.MvpHeadState(compute_scores=True, **kw)
    iv = i.detach().to(dev).requires_grad_(True)
    mv = mp_.detach().to(dev).requires_grad_(True)
    loss, logits = A.mvp_head_apply(iv, mv, t.to(dev), ls.to(dev), cmask.to(dev), y.to(dev), st)
    loss.backward()
    torch.cuda.synchronize()
    met = dict(ign=abs_err(st.ign, ign64), ign_e32=abs_err(ign32, ign64),
               cps=abs_err(st.cps, cps64), cps_e32=abs_err(cps32, cps64),
               loss=abs_err(loss, l64), loss_e32=abs_err(l32, l64),
               dimg=rel_err(iv.grad, gi64), dimg_e32=rel_err(gi32, gi64),
               dmask=rel_err(mv.grad, gm64), dmask_e32=rel_err(gm32, gm64))
    record(test="mvp_head", shape=[B, C, E, exposed], mode=mode, **met)
    for k in ("ign", "cps", "loss", "dimg", "dmask"):
        assert within_rule(met[k], met[k + "_e32"]), (k, met)
    # the caller's predictions: the masked logits, unexposed columns at -inf
    if exposed < C:
        assert torch.isinf(logits[:, exposed:]).all()
    assert torch.isfinite(logits[:, :exposed]).all()
    assert mv.grad[:, C:].abs().max().item() == 0.0


def test_head_label_on_unexposed_column_poisons_loss(dev):
    from lcclip import autograd as A
    i, t, mp_, y, cmask, ls = head_case(5, 4, 64, 3, seed=3)
    for bad in (3, 4, -1):  # on the -inf column; outside [0, C)
        yb = y.clone()
        yb[0] = bad
        st = A.MvpHeadState(use_gsf=True)
        iv = i.detach().to(dev).requires_grad_(True)
        loss, _ = A.mvp_head_apply(iv, mp_.to(dev), t.to(dev), ls.to(dev), cmask.to(dev),
                                   yb.to(dev), st)
        loss.backward()
        assert not math.isfinite(loss.item())
        assert not torch.isfinite(iv.grad).all()


# ---------------------------------------------------------------- steps on TINY_MVP
def tiny_setup(seed_sd=21, seed_mv=3):
    cfg = o.TINY_MVP
    sd = o.synthetic_state_dict(cfg, seed=seed_sd)
    mv = o.mvp_params(cfg, seed=seed_mv)
    img = o.synthetic_images(4, cfg.image_resolution, seed=5)
    tok = o.synthetic_tokens(4, cfg.context_length, seed=5, vocab=cfg.vocab_size)
    return cfg, sd, mv, img, tok


def build(sd, mv, dev, **kw):
    from lcclip.mvp_clip import CLIP_MVP
    m = CLIP_MVP.from_state_dict(sd, device=dev, num_classes=mv["mask"].shape[1],
                                 task_num=mv["key"].shape[0], **kw)
    with torch.no_grad():
        for k in NAMES:
            getattr(m, k).copy_(mv[k])
    return m


@pytest.mark.parametrize("contrastiv", [False, True])
def test_pool_kernels_switch_matches_torch_path(dev, contrastiv):
    cfg, sd, mv, img, tok = tiny_setup()
    y = torch.tensor([0, 3, 1, 1], device=dev)
    out = []
    for pk in (False, True):
        m = build(sd, mv, dev, use_last_layer=False, use_contrastiv=contrastiv, pool_kernels=pk)
        m.count += torch.tensor([0., 2, 1, 0, 0, 3, 0, 0, 1, 0], device=dev)
        m.train()
        m.text_tokens = tok.to(dev)
        logits = m(img.to(dev), tok.to(dev))
        m.loss_fn(logits, y).backward()
        torch.cuda.synchronize()
        out.append((logits.detach().cpu(), m.last_topk.cpu(), m.count.cpu(),
                    m.similarity_loss.detach().cpu(), {k: getattr(m, k).grad.cpu() for k in NAMES}))
    (l0, t0, c0, s0, g0), (l1, t1, c1, s1, g1) = out
    ls = math.exp(sd["logit_scale"].item())
    met = dict(logit_cos=abs_err(l1, l0) / ls, sim=abs_err(s1, s0),
               **{f"grad_{k}": rel_err(g1[k], g0[k]) for k in NAMES})
    record(test="mvp_pool_kernels_switch", contrastiv=contrastiv, **met)
    assert torch.equal(t1, t0) and torch.equal(c1, c0)
    assert met["logit_cos"] <= 1e-6 and met["sim"] <= 1e-6, met
    for k in NAMES:
        assert met[f"grad_{k}"] < 1e-5, (k, met)


def step_reference(cfg, sd, mv, img, tok, y, C, exposed, query, contrastiv, gsf, **rounding):
    """The method's loss and the four gradients, composed from the oracle's forward (features,
    mask selection) and the restatement of the loss."""
    mvg = {k: v.clone().requires_grad_(True) for k, v in mv.items()}
    _, sim, img_f, txt_f, _, topk = o.mvp_forward(img, tok, sd, cfg, mvg, use_last_layer=False,
                                                  **rounding)
    mask_pre = mvg["mask"][topk].mean(1)[:, :C]
    cmask = torch.full((C,), float("-inf"))
    cmask[:exposed] = 0
    if contrastiv:  # float64 similarity loss on the query the module recorded
        k64 = mvg["key"].double()
        tk, sel, _, _ = R.select(query.double(), k64, torch.zeros(k64.shape[0]).double(), 1)
        assert torch.equal(tk, topk)
        sim = R.simloss(k64, torch.zeros(k64.shape[0]).double(), tk, sel, True).float()
    loss, ign, cps = R.method_loss(img_f, txt_f.detach(), mask_pre, cmask, y, sd["logit_scale"],
                                   use_afs=True, use_gsf=gsf)
    total = loss + sim
    total.backward()
    return total.detach(), {k: v.grad for k, v in mvg.items()}


@pytest.mark.parametrize("gsf", [False, True])
@pytest.mark.parametrize("contrastiv", [False, True])
def test_trainer_step_vs_restatement(dev, contrastiv, gsf):
    """The labels are tests/test_mvp_gpu.py's [0, 3, 1] plus a repeat, with all four prompt columns
    exposed. The bounds (loss 5e-3, GRAD_REL) are those of the bf16 image tower against the fp32
    oracle, and they need a case where bf16 storage alone stays inside them, which the test
    asserts from the oracle's two rounding modes alone: with column 3 closed (it holds p = 0.7-0.9
    of every row) the remaining softmax is so flat that the oracle's bf16-rounding mode is already
    3.2e-2 from fp32 on the mask gradient (0.6e-2 with the column open) and 8e-3 on the loss. The
    closed column is covered by the head tests above and by
    test_trainer_skips_update_on_unexposed_label."""
    from lcclip.mvp_trainer import MVPTrainer
    cfg, sd, mv, img, tok = tiny_setup()
    m = build(sd, mv, dev)
    tr = MVPTrainer(m, use_mask=True, use_contrastiv=contrastiv, use_last_layer=False,
                    use_afs=True, use_gsf=gsf, lr=1e-4)
    tr.add_new_class(torch.tensor([7, 2, 5, 9]))
    y = torch.tensor([0, 3, 1, 1])  # already remapped: columns of the four prompts
    assert (tr.class_mask[:4] == 0).all() and torch.isinf(tr.class_mask[4:]).all()
    p0 = tr.flat_p.detach().cpu().clone()
    loss, logits = tr.step(img.to(dev), y, tok.to(dev))
    torch.cuda.synchronize()
    ref_loss, ref_g = step_reference(cfg, sd, mv, img, tok, y, 4, 4, m.features, contrastiv, gsf)
    l16, g16 = step_reference(cfg, sd, mv, img, tok, y, 4, 4, m.features, contrastiv, gsf,
                              rt=o.round_bf16, rt_text=o.round_f16)
    assert abs(l16.item() - ref_loss.item()) < 4e-3
    for k in NAMES:  # the case is well conditioned: bf16 storage alone uses under half the bound
        assert rel_err(g16[k], ref_g[k]) < GRAD_REL / 2, k
    met = dict(loss_abs=abs(loss.item() - ref_loss.item()))
    for k in NAMES:
        met[f"grad_{k}_rel"] = rel_err(getattr(m, k).grad, ref_g[k])
    # ign against the restatement on the GPU's own features
    img_f, txt_f, mrows = (t.cpu() for t in tr.head.inputs)
    cmask = tr.class_mask[:4].cpu()
    ls = sd["logit_scale"]
    ign64, _ = R.scores(img_f.double(), txt_f.double(), y, torch.sigmoid(mrows[:, :4].double()) * 2,
                        cmask.double(), ls.double(), 0.5)
    ign32, _ = R.scores(img_f, txt_f, y, torch.sigmoid(mrows[:, :4]) * 2, cmask, ls, 0.5)
    met["ign"], met["ign_e32"] = abs_err(tr.last_scores[0], ign64), abs_err(ign32, ign64)
    record(test="mvp_trainer_step", contrastiv=contrastiv, gsf=gsf, **met)
    assert met["loss_abs"] < 5e-3, met
    for k in NAMES:
        assert met[f"grad_{k}_rel"] < GRAD_REL, (k, met)
    assert within_rule(met["ign"], met["ign_e32"]), met
    assert torch.isfinite(logits).all()
    assert m.count.sum().item() == 4
    # the update is Adam(lr, weight_decay=0) on the trainer's own gradient
    p = p0.clone().requires_grad_(True)
    p.grad = tr.flat_g.detach().cpu().clone()
    torch.optim.Adam([p], lr=1e-4, weight_decay=0).step()
    torch.testing.assert_close(tr.flat_p.detach().cpu(), p.detach(), rtol=1e-5, atol=1e-7)
    assert not torch.equal(tr.flat_p.cpu(), p0)


def test_trainer_skips_update_on_unexposed_label(dev):
    from lcclip.mvp_trainer import MVPTrainer
    cfg, sd, mv, img, tok = tiny_setup()
    m = build(sd, mv, dev)
    tr = MVPTrainer(m, use_last_layer=False, use_afs=True, use_gsf=True)
    tr.add_new_class(torch.tensor([7, 2, 5, 7]))
    p0 = tr.flat_p.clone()
    loss, _ = tr.step(img.to(dev), torch.tensor([0, 3, 2, 0]), tok.to(dev))  # column 3 is -inf
    torch.cuda.synchronize()
    assert not math.isfinite(loss.item())
    assert torch.equal(tr.flat_p, p0) and tr.adam_step.item() == 0
    loss, _ = tr.step(img.to(dev), torch.tensor([0, 1, 2, 0]), tok.to(dev))
    assert math.isfinite(loss.item()) and tr.adam_step.item() == 1
    assert not torch.equal(tr.flat_p, p0)


def test_trainer_config3_shape(dev):
    """ViT-B/16, B = 128, C = 200, use_mask, use_contrastiv, GSF: one step."""
    from lcclip.mvp_trainer import MVPTrainer
    cfg = o.VIT_B16
    sd = o.synthetic_state_dict(cfg, seed=33)
    B, C = 128, 200
    mv = o.mvp_params(cfg, n_classes=C, seed=5)
    m = build(sd, mv, dev)
    tr = MVPTrainer(m, use_mask=True, use_contrastiv=True, use_last_layer=False, use_afs=True,
                    use_gsf=True, visible_classes="all")
    tr.add_new_class(torch.arange(C))
    img = o.synthetic_images(B, 224, seed=6).to(dev)
    tok = o.synthetic_tokens(C, 77, seed=7).to(dev)
    loss, logits = tr.step(img, torch.arange(B) % C, tok)
    torch.cuda.synchronize()
    assert math.isfinite(loss.item()) and logits.shape == (B, C)
    for k in NAMES:
        g = getattr(m, k).grad
        assert torch.isfinite(g).all() and g.abs().sum() > 0, k
    assert m.count.sum().item() == B
    assert torch.isfinite(tr.last_scores[0]).all() and (tr.last_scores[1] > 0).all()


# ---------------------------------------------------------------- data parallelism
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_trainer(dev, distributed, seed_mv=3):
    from lcclip.mvp_trainer import MVPTrainer
    cfg, sd, mv, img, tok = tiny_setup(seed_mv=seed_mv)
    m = build(sd, mv, dev)
    tr = MVPTrainer(m, use_last_layer=False, use_gsf=True, distributed=distributed)
    return tr, img.to(dev), tok.to(dev), torch.tensor([0, 3, 1, 2])


def _dp_worker(rank, world, port, tmpdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    for p in (ROOT, os.path.join(ROOT, "lifelong-clip_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    # rank 1 starts from other prompt parameters, which the replication overwrites
    tr, img, tok, y = _dp_trainer(dev, True, seed_mv=3 + rank)
    per = img.shape[0] // world
    sl = slice(rank * per, (rank + 1) * per)
    tr.add_new_class(y[sl])
    assert tr.book.exposed_classes == [0, 3, 1, 2]
    tr.step(img[sl], y[sl], tok)
    torch.cuda.synchronize()
    torch.save({"g": tr.flat_g.cpu(), "p": tr.flat_p.cpu(), "ign": tr.last_scores[0].cpu(),
                "count": tr.model.count.cpu()}, os.path.join(tmpdir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_trainer_dp_matches_global_batch(dev):
    tr, img, tok, y = _dp_trainer(dev, False)
    tr.add_new_class(y)
    tr.forward_backward(img, y, tok)
    torch.cuda.synchronize()
    ref_g, ref_ign = tr.flat_g.cpu(), tr.last_scores[0].cpu()
    img_f, txt_f, mrows = (t.cpu() for t in tr.head.inputs)
    cm = tr.class_mask[:4].cpu()
    ls = tr.model.backbone.logit_scale.detach().cpu()
    ign64, _ = R.scores(img_f.double(), txt_f.double(), y, torch.sigmoid(mrows[:, :4].double()) * 2,
                        cm.double(), ls.double(), 0.5)
    ign32, _ = R.scores(img_f, txt_f, y, torch.sigmoid(mrows[:, :4]) * 2, cm, ls.float(), 0.5)
    e32 = abs_err(ign32, ign64)
    world = 2
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_dp_worker, args=(world, _free_port(), tmp), nprocs=world, join=True)
        outs = [torch.load(os.path.join(tmp, f"r{r}.pt"), weights_only=True) for r in range(world)]
    assert torch.equal(outs[0]["g"], outs[1]["g"])
    assert torch.equal(outs[0]["p"], outs[1]["p"])
    rel = rel_err(outs[0]["g"], ref_g)
    ign = torch.cat([outs[0]["ign"], outs[1]["ign"]])
    err = abs_err(ign, ref_ign)
    record(test="mvp_trainer_dp", grad_rel=rel, ign_err=err, ign_e32=e32)
    print(f"mvp dp: grad rel {rel:.3e}, ign err {err:.3e}, e32 {e32:.3e}")
    assert rel < 2e-2
    assert within_rule(err, e32), (err, e32)
    assert torch.equal(outs[0]["count"], tr.model.count.cpu())
