"""The image tower's last block on its CLS rows only (ImageTower.LAST_ROWS, engine.py) against the
full-row path it replaces, from identical dropout seeds: the skipped rows feed nothing
(model.py:782 reads row 0 of each image) and their gradient is zero, so loss, probs and every PEFT
gradient stay what they were up to 16-bit rounding.

Bounds. Loss and probs: 4e-3, the bound of test_golden_trainer_step against the rounding oracle.
Gradients, per tensor: rel(on, off) <= rel(off, fp32 oracle) at dropout 0 — the change stays inside
the old path's own distance from the reference (with dropout on, the same per-tensor bound: the
oracle cannot draw the kernels' mask, and a wrong mask moves a gradient by order 1, far outside).
Models: the tiny golden config (width 128: the unfused adapter launches, f32 residual stream) and a
2-layer width-768 224/16 tower (the fused adapter + LayerNorm launches, half residual stream).
Measured (MI355X): rel(on, off) is exactly 0 in every default case (the compact path executes the
full path's arithmetic on the live rows); the bounds are what the issue set.
"""
import itertools
import os

import numpy as np
import pytest
import torch

from oracle import clip_oracle as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiny_clip.npz")
W768 = o.ClipConfig(vision_layers=2, transformer_layers=2)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def wrapper(sd, dev, dropout, prec):
    from lcclip.adapter_clip import AdapterCLIP, set_adapter_dropout
    w = AdapterCLIP.from_state_dict(sd, "adapter", "both", device=dev, image_precision=prec)
    return set_adapter_dropout(w, dropout)


def set_path(monkeypatch, rows):
    """LAST_ROWS on / off and the dropout seed counter back at its start."""
    from lcclip import engine
    monkeypatch.setattr(engine.ImageTower, "LAST_ROWS", rows)
    monkeypatch.setattr(engine, "_seed_counter", itertools.count(1))


def trainer_step(case, dev, monkeypatch, rows, dropout, prec):
    from lcclip import OnlineTrainer
    sd, img, tok, y, _ = case
    set_path(monkeypatch, rows)
    w = wrapper(sd, dev, dropout, prec)
    tr = OnlineTrainer(w)
    loss, probs = tr.forward_backward(img.to(dev), y.to(dev), tok.to(dev))
    torch.cuda.synchronize()
    grads = {n: tr.grads[p].float().cpu().clone() for n, p in w.model.named_parameters()
             if p.requires_grad}
    return loss.item(), probs.float().cpu(), grads


@pytest.fixture(scope="module")
def cases():
    """name -> (state dict, images, tokens, labels, fp32 oracle gradients)."""
    d = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")}
    sd = {k: sd[k] for k in o.param_shapes(o.TINY, "adapter", "both")}
    g = {k[len("adapter/grad/"):]: torch.from_numpy(d[k]) for k in d.files
         if k.startswith("adapter/grad/")}
    tiny = (sd, torch.from_numpy(d["images"]), torch.from_numpy(d["tokens"]),
            torch.from_numpy(d["labels"]), g)
    sd7 = o.synthetic_state_dict(W768, "adapter", "both", seed=17)
    img = o.synthetic_images(2, 224, seed=18)
    tok = o.synthetic_tokens(4, 77, seed=19)
    y = torch.arange(2) % 4
    g7 = o.train_step(img, tok, y, sd7, W768, "adapter", "both")[4]
    return {"tiny": tiny, "w768": (sd7, img, tok, y, g7)}


_off0 = {}


def off_at_p0(cases, dev, monkeypatch, model, prec):
    """The full-row path at dropout 0 (computed once per model and precision): its per-tensor
    distance from the fp32 oracle is the bound."""
    key = (model, prec)
    if key not in _off0:
        _off0[key] = trainer_step(cases[model], dev, monkeypatch, False, 0.0, prec)
    return _off0[key]


def check(on, off, bound_run, g32, tag):
    (l1, p1, g1), (l0, p0, g0) = on, off
    assert abs(l1 - l0) < 4e-3 and (p1 - p0).abs().max().item() < 4e-3, tag
    assert set(g1) == set(g0) and set(g32) <= set(g0)
    for n in g32:
        r, b = rel(g1[n], g0[n]), rel(bound_run[2][n], g32[n])
        print(f"LAST_ROWS {tag} {n} rel(on, off) {r:.3e} bound rel(off, fp32) {b:.3e}")
        assert r <= b, (tag, n, r, b)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("model", ["tiny", "w768"])
def test_last_rows_trainer_step(cases, dev, monkeypatch, model, dropout, prec):
    """OnlineTrainer.forward_backward with LAST_ROWS on and off from identical seeds."""
    base = off_at_p0(cases, dev, monkeypatch, model, prec)
    off = base if dropout == 0.0 else trainer_step(cases[model], dev, monkeypatch, False, dropout,
                                                   prec)
    on = trainer_step(cases[model], dev, monkeypatch, True, dropout, prec)
    check(on, off, base, cases[model][4], f"{model} p={dropout} {prec}")
    if dropout:
        # the mask matters at this size: without it the gradients leave the bound
        moved = max(rel(off[2][n], base[2][n]) / rel(base[2][n], g) for n, g in cases[model][4].items()
                    if "adaptmlp" in n and n.startswith("visual"))
        assert moved > 3.0, moved


def test_last_rows_row_backward_knob(cases, dev, monkeypatch):
    """BlockStack.ROW_BWD (LCCLIP_ROW_BWD=1): the compact block's attention backward on
    ops.attn_row_bwd instead of the full kernel on blanked operands; the same bounds."""
    from lcclip import engine
    model, prec = "w768", "bf16"
    base = off_at_p0(cases, dev, monkeypatch, model, prec)
    off = trainer_step(cases[model], dev, monkeypatch, False, 0.1, prec)
    monkeypatch.setattr(engine.BlockStack, "ROW_BWD", True)
    on = trainer_step(cases[model], dev, monkeypatch, True, 0.1, prec)
    check(on, off, base, cases[model][4], "w768 p=0.1 bf16 row-bwd")


def test_last_rows_module_path(cases, dev, monkeypatch):
    """AdapterCLIP.forward + cross-entropy on probs + autograd (autograd.py goes through
    ImageTower) with LAST_ROWS on, against the trainer's full-row step."""
    from lcclip import freeze_backbone
    model = "w768"
    sd, img, tok, y, g32 = cases[model]
    base = off_at_p0(cases, dev, monkeypatch, model, "bf16")
    set_path(monkeypatch, True)
    w = wrapper(sd, dev, 0.0, "bf16")
    freeze_backbone(w)
    w.train()
    w.set_token(tok.to(dev))
    probs, _, _ = w(img.to(dev))
    loss = torch.nn.functional.cross_entropy(probs, y.to(dev))
    loss.backward()
    grads = {n: p.grad.float().cpu() for n, p in w.model.named_parameters() if p.requires_grad}
    check((loss.item(), probs.detach().float().cpu(), grads), base, base, g32, "module w768")


def test_last_rows_input_gradient(cases, dev, monkeypatch):
    """need_dx=True: the tower's stack-input gradient with LAST_ROWS on against off, both
    precisions. Bound: the full-row path's own distance between its bf16 and fp16 towers (the
    16-bit budget of that gradient; test_fp16_image_tower_module_path_and_input_grad holds it to
    2e-2)."""
    sd, img, _, _, _ = cases["tiny"]
    gx = {}
    for prec in ("bf16", "fp16"):
        for rows in (False, True):
            set_path(monkeypatch, rows)
            tower = wrapper(sd, dev, 0.1, prec).model.visual.tower
            f, ctx = tower.forward(img.to(dev), save=True, training=True)
            df = torch.randn(f.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
            grads = {p: torch.zeros(p.shape, device=dev) for p in tower.stack.trainable_params()}
            gx[prec, rows] = tower.backward(ctx, df * 1e-6, grads, need_dx=True).float().cpu()
            assert ctx["rows"] == rows
    bound = rel(gx["fp16", False], gx["bf16", False])
    for prec in ("bf16", "fp16"):
        r = rel(gx[prec, True], gx[prec, False])
        print(f"LAST_ROWS input gradient {prec} rel(on, off) {r:.3e} bound {bound:.3e}")
        assert gx[prec, True].abs().sum() > 0 and r <= bound, (prec, r, bound)


def test_last_rows_scope(cases, dev, monkeypatch):
    """The knob touches the adapter image tower only: LoRA keeps every row; inference (save=False)
    takes the compact path too and gives the full path's features within 16-bit rounding."""
    sd, img, _, _, _ = cases["w768"]
    feats = {}
    for rows in (False, True):
        set_path(monkeypatch, rows)
        tower = wrapper(sd, dev, 0.0, "bf16").model.visual.tower
        with torch.no_grad():
            feats[rows], ctx = tower.forward(img.to(dev), save=False)
        assert ctx is None
    assert rel(feats[True], feats[False]) < 4e-3
    from lcclip.adapter_clip import AdapterCLIP
    sdl = o.synthetic_state_dict(o.TINY, "lora", "both", seed=3)
    set_path(monkeypatch, True)
    tower = AdapterCLIP.from_state_dict(sdl, "lora", "both", device=dev).model.visual.tower
    _, ctx = tower.forward(cases["tiny"][1].to(dev), save=True, training=True)
    assert ctx["rows"] is False and ctx["x"].shape[0] == ctx["n"] * ctx["L"]
