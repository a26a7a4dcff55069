"""ViT-L/14's routes in a whole training step on the MI355X, against the CPU oracle: patch-14
embedding (lc_patchify_pad, conv1 at K = 640), 257-token attention (the long kernel family),
the width-1024 routes, and a last block that keeps every row (the compact last block needs the
one-row attention forms, L <= 256).

Two 2-layer configs, both with L = 257:
  SMALL  width 128 (H = 2), patch 14 at 224 px, text 64 / 1 head: patch embedding and the long
         attention inside a step
  WIDE2  oracle.VIT_L14 cut to 2 + 2 layers: width 1024, H = 16, embed 768, text 768 / 12

OnlineTrainer.forward_backward against oracle.train_step in fp32 and with the path's rounding
(bf16 image tower, IEEE-half text tower). Bounds are the project's (test_model_gpu.py,
tests/parity.py): probs abs < 4e-3 vs the rounding oracle and < 1e-2 vs fp32, loss < 1e-2,
check_logits, flat PEFT gradient rel-norm vs fp32 < GRAD_REL and every tensor's cosine >= 0.99.
Per-tensor rel-norms are recorded (test_model_gpu.record's metrics file), not asserted, as is the
logit distance from the rounding oracle: as in test_model_gpu.py's train-step tests, check_logits
gets the distances from fp32 only. parity.MAX_VS_BF16 (8e-4, "what remains is accumulation
order") does not apply to SMALL: the rounding oracle evaluated with fp32 and with fp64
accumulation — the same rounding points, nothing else changed (the method of
tools/summation_floor.py) — is already 6.4e-4 max / 3.5e-4 RMS apart in logits on the SMALL
adapter case (64-dimensional features; WIDE2 adapter 1.8e-4, LoRA 1.5e-4 / 0.7e-4), so two
accumulation orders of that arithmetic sit up to ~9e-4 apart (measured here: 9.1e-4).

The seeds are chosen so that the reference alone sits well inside those bounds (rounding oracle
vs fp32 oracle on the CPU: gradient flat rel 0.44e-2 .. 1.65e-2, cosine min >= 0.9996). Seed 21
must not be used for the adapter case: with B = 4 its oracle-only cosine is 0.971 (SMALL).
"""
import dataclasses
import math

import pytest
import torch
from parity import GRAD_REL, check_logits, logit_errors, logit_metrics
from test_model_gpu import make_wrapper, record, rel

from oracle import clip_oracle as o

pytestmark = pytest.mark.gpu

SMALL = o.ClipConfig(embed_dim=64, image_resolution=224, vision_layers=2, vision_width=128,
                     vision_patch_size=14, vocab_size=512, transformer_width=64,
                     transformer_heads=1, transformer_layers=2)
WIDE2 = dataclasses.replace(o.VIT_L14, vision_layers=2, transformer_layers=2)
CONFIGS = {"small": SMALL, "wide2": WIDE2}
# method: (B, C, weight seed, image seed, token seed)
RUNS = {"adapter": (4, 4, 31, 32, 33), "lora": (2, 3, 21, 22, 23)}


def cs(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()


@pytest.mark.parametrize("method", ["adapter", "lora"])
@pytest.mark.parametrize("cfg_name", ["small", "wide2"])
def test_step_vs_oracle(dev, cfg_name, method):
    from lcclip import OnlineTrainer
    cfg = CONFIGS[cfg_name]
    B, C, s_w, s_i, s_t = RUNS[method]
    assert cfg.grid ** 2 + 1 == 257
    sd = o.synthetic_state_dict(cfg, method, "both", seed=s_w)
    img = o.synthetic_images(B, cfg.image_resolution, seed=s_i)
    tok = o.synthetic_tokens(C, cfg.context_length, seed=s_t, vocab=cfg.vocab_size)
    y = torch.arange(B) % C
    loss32, p32, i32, t32, g32, _ = o.train_step(img, tok, y, sd, cfg, method, "both")
    _, p16, i16, t16, g16, _ = o.train_step(img, tok, y, sd, cfg, method, "both",
                                            rt=o.round_bf16, rt_text=o.round_f16)
    w = make_wrapper(sd, method, "both", dev)
    with torch.no_grad():
        _, fi, ft = w(img.to(dev), tok.to(dev))
    tr = OnlineTrainer(w)
    loss, probs = tr.forward_backward(img.to(dev), y.to(dev), tok.to(dev))
    torch.cuda.synchronize()
    ls = math.exp(sd["logit_scale"].item())
    named = dict(w.model.named_parameters())
    gg = {n: tr.grads[named[n]].float().cpu() for n in g32}
    e32 = {n: rel(gg[n], g) for n, g in g32.items()}
    cos = {n: cs(gg[n], g32[n]) for n in g32}
    cat = lambda d: torch.cat([d[n].flatten() for n in g32])  # noqa: E731
    m = dict(probs_abs_vs_bf16=(probs.cpu() - p16).abs().max().item(),
             probs_abs_vs_fp32=(probs.cpu() - p32).abs().max().item(),
             loss_abs=abs(loss.item() - loss32.item()),
             grad_flat_rel_vs_fp32=rel(cat(gg), cat(g32)), grad_cos_min=min(cos.values()),
             oracle_bf16_grad_flat_rel=rel(cat(g16), cat(g32)),
             oracle_bf16_grad_cos_min=min(cs(g16[n], g32[n]) for n in g32), n_grads=len(g32),
             logit_max_vs_rounding_oracle=logit_errors(ls * fi.cpu() @ ft.cpu().t(),
                                                       ls * i16 @ t16.t(), ls)[0],
             **logit_metrics(ls * fi.cpu() @ ft.cpu().t(), ls * i32 @ t32.t(), None, ls))
    record(test=f"vit_l14_{cfg_name}_step", method=method, B=B, C=C, grad_rel=e32, **m)
    print(f"VIT_L14_STEP {cfg_name} {method} {m}")
    assert m["n_grads"] > 0
    assert m["probs_abs_vs_bf16"] < 4e-3 and m["probs_abs_vs_fp32"] < 1e-2, m
    assert m["loss_abs"] < 1e-2, m
    check_logits(m, tiny=cfg_name == "small")
    assert m["grad_flat_rel_vs_fp32"] < GRAD_REL, m
    for n in g32:
        assert cos[n] >= 0.99, (n, cos[n], e32[n])
    if method == "adapter":
        # the adapter tower's compact last block is off at 257 tokens: every row kept
        with torch.no_grad():
            _, ctx = tr.img.forward(img.to(dev), save=True, training=False)
        assert not ctx["rows"] and ctx["x"].shape[0] == B * 257
        assert tr.img.stack.rows_ok()
        x0 = torch.zeros(B * 257, cfg.vision_width, device=dev)
        with pytest.raises(ValueError, match="last_rows"):
            tr.img.stack.forward(x0, B, 257, save=False, last_rows=True)


def test_patch_row_input_is_refused(dev):
    """The 2-D "already patch rows" input (the train transform's layout="patches") stays a
    patch % 8 feature: a patch-14 model refuses it by name."""
    sd = o.synthetic_state_dict(SMALL, "adapter", "both", seed=31)
    w = make_wrapper(sd, "adapter", "both", dev)
    rows = torch.zeros(256, 588, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="patch"):
        w.model.visual.tower.forward(rows, save=False)
