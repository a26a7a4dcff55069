"""Torch restatements of the MVP-CLIP training method (methods/mvp_clip.py and the pool glue of
models/mvp_clip.py of qcNPU/LifeLong-CLIP), the references of tests/test_mvp_method*.py. They
run in the dtype of their inputs: float64 is the reference, the same code in float32 gives the
error a float32 implementation of the same formulas has (`e32`, the tolerance rule's yardstick).
Nothing here calls lcclip.

Tolerance rule (tests/test_mvp_method_gpu.py): a kernel passes when its error against float64
is <= 8 * e32 + 1e-6, absolute for scores and losses, relative-norm for gradients; the factor 8
allows for another summation order and the hardware exponential.
"""
import torch
import torch.nn.functional as F


def select(query, key, count, k):
    """models/mvp_clip.py:224-235, 253 -> (topk [B,k], selected distances [B,k], scaled distance
    [B,P], bincount [P]). count None: use_contrastiv off (mass 1)."""
    distance = 1 - F.cosine_similarity(query.unsqueeze(1), key, dim=-1)          # :224-225
    mass = (count + 1) if count is not None else 1.0                             # :226-229
    scaled = distance * mass
    topk = scaled.topk(k, dim=1, largest=False)[1]                               # :231-232
    rows = torch.arange(topk.size(0)).unsqueeze(1).repeat(1, k)
    sel = distance[rows, topk]                                                   # :233-235
    num = topk.view(-1).bincount(minlength=key.size(0))                          # :253
    return topk, sel, scaled, num


def simloss(key, count, topk, sel, use_contrastiv):
    """models/mvp_clip.py:239-248 as written, its squeeze() and broadcasting included: at
    selection size 1 key_wise_distance[topk] is [B,1,P] and mass[topk] [B,1], whose quotient
    broadcasts to [B,B,P]; at larger sizes the shapes do not broadcast for a general batch and
    torch raises, as the reference would."""
    distance = sel.squeeze()
    if not use_contrastiv:
        return distance.mean()                                                   # :248
    mass = count + 1
    kwd = 1 - F.cosine_similarity(key.unsqueeze(1), key, dim=-1)                 # :239
    a = (kwd[topk] / mass[topk]).exp().mean()                                    # :240-246
    d = (distance / mass[topk]).exp().mean()
    return -(a / (d + a) + 1e-6).log()


def gather_bwd(idx, g, pool, alpha=1.0):
    """The pool gather's backward as one GEMM: alpha * one_hot(idx)^T @ g, g [B*k, R]."""
    onehot = F.one_hot(idx.reshape(-1), pool).to(g.dtype)
    return alpha * (onehot.t() @ g)


def masked_logits(i_feat, t_feat, logit_scale, mask, cmask):
    """forward_head (models/mvp_clip.py:266-280) + methods/mvp_clip.py:269-274: normalise,
    s * i t^T, times the (sigmoid * 2) mask when given, plus the 0 / -inf class mask."""
    t = t_feat / t_feat.norm(dim=-1, keepdim=True)
    i = i_feat / i_feat.norm(dim=-1, keepdim=True)
    logit = logit_scale.exp() * i @ t.t()
    if mask is not None:
        logit = logit * mask
    return logit + cmask


def grads_loop(i_feat, t_feat, y, mask, cmask, logit_scale):
    """_compute_grads (methods/mvp_clip.py:204-238) literally: one backward per sample for
    d loss_b / d t[y_b], then one for the batch-mean loss -> (sample_grad [B,E], batch_grad
    [B,E])."""
    t = (t_feat / t_feat.norm(dim=-1, keepdim=True)).detach().requires_grad_(True)
    i = (i_feat / i_feat.norm(dim=-1, keepdim=True)).detach().requires_grad_(True)
    logit = logit_scale.detach().exp() * i @ t.t()
    if mask is not None:
        logit = logit * mask.detach()
    logit = logit + cmask
    sample_loss = F.cross_entropy(logit, y, reduction="none")
    sample_grad = []
    for b in range(len(y)):
        (g,) = torch.autograd.grad(sample_loss[b], t, retain_graph=True)
        sample_grad.append(g[y[b]].clone())
    sample_grad = torch.stack(sample_grad)
    (total,) = torch.autograd.grad(F.cross_entropy(logit, y, reduction="mean"), t)
    return sample_grad, total[y]


def grads_closed(i_feat, t_feat, y, mask, cmask, logit_scale, n_global=None):
    """The same in closed form (no backward pass): with z the masked logits and p = softmax(z),
    sample_grad_b = s m[b,y_b] (p[b,y_b] - 1) i^_b and G = (s/B) (m (p - onehot))^T i^.
    1 - p[b,y] is summed from the other classes (no cancellation at a peaky softmax).
    -> (sample_grad, batch_grad = G[y], G)."""
    i = i_feat / i_feat.norm(dim=-1, keepdim=True)
    z = masked_logits(i_feat, t_feat, logit_scale, mask, cmask)
    B, C = z.shape
    e = (z - z.max(dim=1, keepdim=True).values).exp()
    p = e / e.sum(1, keepdim=True)
    onehot = F.one_hot(y, C).bool()
    q1 = e.masked_fill(onehot, 0).sum(1) / e.sum(1)
    pm = torch.where(onehot, -q1.unsqueeze(1), p)
    m = mask if mask is not None else torch.ones_like(z)
    s = logit_scale.exp()
    sample_grad = (s * m[torch.arange(B), y] * -q1).unsqueeze(1) * i
    G = (s / (n_global or B)) * (m * pm).t() @ i
    return sample_grad, G[y], G


def scores(i_feat, t_feat, y, mask, cmask, logit_scale, margin, closed=True, G=None):
    """_get_score (methods/mvp_clip.py:240-254) -> (ign [B], cps [B]). G: a batch gradient
    computed elsewhere (the global batch's, under data parallelism)."""
    if closed:
        sg, bg, _ = grads_closed(i_feat, t_feat, y, mask, cmask, logit_scale)
        if G is not None:
            bg = G[y]
    else:
        sg, bg = grads_loop(i_feat, t_feat, y, mask, cmask, logit_scale)
    ign = 1.0 - torch.cosine_similarity(sg, bg, dim=1)
    cps = 1.0 - torch.cosine_similarity(t_feat[y], i_feat, dim=1) + margin
    return ign, cps


def method_loss(i_feat, t_feat, mask_pre, cmask, y, logit_scale, use_afs=False, use_gsf=False,
                alpha=0.5, gamma=2.0, margin=0.5, closed=True, ign=None):
    """loss_fn without the similarity term (methods/mvp_clip.py:256-280) -> (loss, ign, cps).
    mask_pre: the selected pre-sigmoid mask rows [B,C] or None (use_mask off); differentiable in
    i_feat and mask_pre. ign: scores computed elsewhere (the kernel's own, or a global batch's)."""
    mask = torch.sigmoid(mask_pre) * 2.0 if mask_pre is not None else None   # models/mvp_clip.py:263
    ign_, cps = scores(i_feat.detach(), t_feat.detach(), y,
                       None if mask is None else mask.detach(), cmask, logit_scale.detach(),
                       margin, closed)
    if ign is None:
        ign = ign_
    feat = i_feat / cps.unsqueeze(1) if use_afs else i_feat                  # :264-268
    logit = masked_logits(feat, t_feat, logit_scale, mask, cmask)
    loss = F.nll_loss(F.log_softmax(logit, dim=1), y)                        # :275-276
    if use_gsf:
        loss = (1 - alpha) * loss + alpha * (ign.detach() ** gamma) * loss   # :277-279
    return loss.mean(), ign, cps
