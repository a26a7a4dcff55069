"""MVP-CLIP as a training method: methods/mvp_clip.py of qcNPU/LifeLong-CLIP (BASELINE config 3)
around lcclip.mvp_clip.CLIP_MVP, on the mvp.hip kernels.

One step (online_train, methods/mvp_clip.py:73-132, with loss_fn, :256-280, and _get_score,
:204-254):

  forward_features (no-grad key query, selection, count, similarity loss, the e-prompt / mask
  gathers, the prompt-tuned tower) -> normalise -> [scores] -> [AFS] -> masked logits + the
  -inf exposed-class mask -> mean NLL x GSF weight + similarity loss -> backward through the head,
  the prompt tower and the pool kernels -> gradient sync -> non-finite check -> Adam.

The reference's per-sample gradient loop (B backward(retain_graph=True) calls) is computed in
closed form: with z = s m (i^ t^T) + cmask, p = softmax(z),
  sample_grad_b = s m[b,y_b] (p[b,y_b] - 1) i^_b,   G = (s/B) (m (p - onehot))^T i^,
  ign_b = 1 - cos(sample_grad_b, G[y_b]),           cps_b = 1 - cos(t[y_b], i_b) + margin,
and with use_gsf loss = Lbar ((1 - alpha) + alpha mean_b ign_b^gamma). use_afs divides the image
feature by cps before forward_head normalises it, which is the identity for cps > 0 (margin 0.5
keeps it there) and a sign flip (NaN at 0) otherwise; it is implemented as the reference writes
it. The reference computes the scores on every step; here they are skipped when neither flag
consumes them (compute_scores=True forces them).

Documented deviation: under AMP the reference's score GEMM runs in fp16; here it is fp32.

All four trainable tensors (key, mask, g_prompts, e_prompts) are views into one flat fp32
buffer, and so are their gradients and the Adam moments (the OnlineTrainer layout): the
optimizer is one launch and the data-parallel exchange one all-reduce. weight_decay = 0 makes
lc_adamw the reference's Adam (opt_name 'adam', lr 1e-4).

Data parallelism (one rank per GPU, lcclip.dp.ModuleDataParallel): the reference computes its
loss on the gathered global batch, so G and sum_b ign_b^gamma are summed over ranks (G scaled by
the global batch size) before ign and the GSF weight are formed; each rank then backpropagates
Lbar_rank x w_global and the flat gradient is averaged.
"""
from __future__ import annotations

import torch

from . import autograd as lc_autograd
from . import ops
from .dp import ModuleDataParallel
from .ops import F32
from .stream import ClassBook

PARAM_NAMES = ("key", "mask", "g_prompts", "e_prompts")


class MVPTrainer:
    def __init__(self, model, class_names=None, use_mask=True, use_contrastiv=False,
                 use_last_layer=True, use_afs=False, use_gsf=False, alpha=0.5, gamma=2.0,
                 margin=0.5, visible_classes="batch", lr=1e-4, weight_decay=0.0,
                 betas=(0.9, 0.999), eps=1e-8, process_group=None, distributed=None,
                 pool_kernels=True, compute_scores=False, memory_size=0):
        self.model = model
        # methods/mvp_clip.py:294-298 (setup_distributed_model)
        model.use_mask = bool(use_mask)
        model.use_contrastiv = bool(use_contrastiv)
        model.use_last_layer = bool(use_last_layer)
        model.pool_kernels = bool(pool_kernels)
        self.use_mask = bool(use_mask)
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.n_classes = model.class_num
        if class_names is None:
            class_names = [str(i) for i in range(self.n_classes)]
        self.book = ClassBook(class_names, memory_size=memory_size, visible=visible_classes)
        self.visible_classes = visible_classes
        dev = model.key.device
        # methods/mvp_clip.py:47: every class unexposed until add_new_class
        self.class_mask = torch.full((self.n_classes,), float("-inf"), dtype=F32, device=dev)
        params = [getattr(model, k) for k in PARAM_NAMES]
        n = sum(p.numel() for p in params)
        self.numel = n
        self.flat_p = torch.empty(n, dtype=F32, device=dev)
        self.flat_g = torch.zeros(n, dtype=F32, device=dev)
        self.m = torch.zeros(n, dtype=F32, device=dev)
        self.v = torch.zeros(n, dtype=F32, device=dev)
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                self.flat_p[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[off:off + k].view_as(p)
                p.grad = self.flat_g[off:off + k].view_as(p)
                off += k
        self.params = params
        # replicas: rank 0's parameters (through the flat buffer's views) and buffers, once
        self.ddp = ModuleDataParallel(model, process_group, distributed)
        self.head = lc_autograd.MvpHeadState(use_afs, use_gsf, alpha, gamma, margin,
                                             compute_scores, self.ddp)
        self.skip = torch.zeros(1, dtype=torch.int32, device=dev)
        self.adam_step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.step_count = 0
        self.last_scores = None

    # ------------------------------------------------------------------ class bookkeeping
    def add_new_class(self, labels):
        """methods/mvp_clip.py:319-328: exposed classes in first-seen order, the class mask's first
        len(exposed) entries opened, the batch-visible list rebuilt (merged over ranks under
        data parallelism, :300-313)."""
        self.book.add_new_class(labels)
        if self.ddp.active:
            self.book.exposed_classes = self.ddp.exposed_classes(self.book.exposed_classes)
            if self.book.memory_size > 0:
                self.book.batch_exposed_classes = self.book.exposed_classes
            else:
                self.book.batch_exposed_classes = self.ddp.exposed_classes(
                    self.book.batch_exposed_classes)
        self.class_mask[:len(self.book.exposed_classes)] = 0
        if self.model._tokenizer is not None:
            self.model.set_exposed_classes(self.book.exposed_classes_names)
        else:
            self.model.exposed_classes = len(self.book.exposed_classes)

    def train_classes(self):
        """(class ids, class names) of the logit columns (visible_classes 'batch' | 'all')."""
        return self.book.train_classes()

    def remap(self, labels):
        return self.book.remap(labels)

    def reset_optimizer(self):
        """reset_opt (methods/mvp_clip.py:198-202): a fresh Adam."""
        self.m.zero_()
        self.v.zero_()
        self.step_count = 0
        self.adam_step.zero_()

    # ------------------------------------------------------------------ the step
    def forward_backward(self, images, labels, tokens):
        """Everything but the gradient sync and the update -> (loss [1], masked logits [B, C]).
        labels index the rows of `tokens` (already remapped).

        Mask columns: the reference takes mask[:, y.unique()] and self.mask[y.unique()] in 'batch'
        mode; here columns 0..C-1 are used. The two are equal whenever every listed class occurs
        in the batch, which the reference's single-process bookkeeping guarantees (the batch list
        is the batch's distinct labels). With 'all' the columns are [:len(exposed)]."""
        m = self.model
        m.train()
        self.flat_g.zero_()
        dev = self.flat_p.device
        C = tokens.shape[0]
        B = images.shape[0]
        x, txt, maskraw, _ = m._features(images, tokens)
        maskrows = maskraw.reshape(B, -1) if self.use_mask else None
        cmask = self.class_mask[:C].contiguous()
        labels = labels.to(dev, torch.int64).contiguous()
        loss_h, logits = lc_autograd.mvp_head_apply(x, maskrows, txt, m.backbone.logit_scale,
                                                    cmask, labels, self.head)
        loss = loss_h + m.similarity_loss
        loss.backward()
        if self.head.scoring:
            self.last_scores = (self.head.ign, self.head.cps)
        return loss.detach().reshape(1), logits

    def sync_grads(self):
        """Average the flat gradient over ranks (one all-reduce)."""
        dp = self.ddp.dp
        dp.launch_bucket(self.flat_g, 0, self.numel)
        dp.finish_buckets(self.flat_g)

    def _update(self):
        """Non-finite check -> Adam step counter (unless skipped) -> fused AdamW, all on the
        device (the OnlineTrainer._update sequence)."""
        self.skip.zero_()
        ops.check_finite(self.flat_g, self.skip)
        ops.adam_step_advance(self.adam_step, self.skip)
        b1, b2 = self.betas
        ops.adamw(self.flat_p, self.flat_g, self.m, self.v, self.lr, b1, b2, self.eps, self.wd, 1,
                  self.skip, step_dev=self.adam_step)

    def optimizer_step(self):
        self.step_count += 1
        self._update()

    def step(self, images, labels, tokens):
        """One training step (methods/mvp_clip.py:96-125) -> (loss [1], logits [B, C])."""
        loss, logits = self.forward_backward(images, labels, tokens)
        self.sync_grads()
        self.optimizer_step()
        return loss, logits

    def online_train(self, x, y):
        """methods/mvp_clip.py:73-132 for one batch of raw labels: remap them into the training
        class list, tokenise its names, step."""
        _, names = self.train_classes()
        yy = self.remap(y)
        tokens = self.model.labels_tokenize(names)
        return self.step(x, yy, tokens)

    @torch.no_grad()
    def evaluate_logits(self, x):
        """online_evaluate's logits (methods/mvp_clip.py:150-151): model(x) + class_mask[:exposed]."""
        self.model.eval()
        logits = self.model(x)
        return logits + self.class_mask[:len(self.book.exposed_classes)]
