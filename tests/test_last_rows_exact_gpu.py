"""The compact last block on its exact compact kernels (BlockStack.ROWS_EXACT: ops.gemm_nt_rows
for c_proj / c_fc dX, ops.attn_bwd_live_row for the attention backward) against the two paths it
must not move by a bit: the same block on full-size launches over blanked operands
(LCCLIP_ROWS_EXACT=0) and the full-row path (LCCLIP_LAST_ROWS=0). One forward_backward of the
tiny and the width-768 models of tests/test_last_rows_gpu.py at 4 images, dropout 0.1, identical
seeds: probs and every PEFT gradient bit-equal in the three configurations, and the new
entry points really ran (calls through ops counted). Split-K tails do not occur at this size;
tests/test_gemm_rows_gpu.py pins those.
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


@pytest.fixture(scope="module")
def cases():
    d = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")}
    sd = {k: sd[k] for k in o.param_shapes(o.TINY, "adapter", "both")}
    tok_t = torch.from_numpy(d["tokens"])
    tiny = (sd, o.synthetic_images(4, o.TINY.image_resolution, seed=28), tok_t,
            torch.arange(4) % tok_t.shape[0])
    sd7 = o.synthetic_state_dict(W768, "adapter", "both", seed=17)
    w768 = (sd7, o.synthetic_images(4, 224, seed=18), o.synthetic_tokens(4, 77, seed=19),
            torch.arange(4) % 4)
    return {"tiny": tiny, "w768": w768}


def step(case, dev, monkeypatch, last_rows, exact):
    from lcclip import OnlineTrainer, engine, ops
    from lcclip.adapter_clip import AdapterCLIP, set_adapter_dropout
    sd, img, tok, y = case
    monkeypatch.setattr(engine.ImageTower, "LAST_ROWS", last_rows)
    monkeypatch.setattr(engine.BlockStack, "ROWS_EXACT", exact)
    monkeypatch.setattr(engine, "_seed_counter", itertools.count(1))
    calls = {"gemm_nt_rows": 0, "attn_bwd_live_row": 0}

    def counted(name):
        fn = getattr(ops, name)

        def wrapper(*a, **kw):
            done = fn(*a, **kw)
            calls[name] += bool(done)
            return done
        return wrapper
    for name in calls:
        monkeypatch.setattr(ops, name, counted(name))
    w = set_adapter_dropout(AdapterCLIP.from_state_dict(sd, "adapter", "both", device=dev), 0.1)
    tr = OnlineTrainer(w)
    loss, probs = tr.forward_backward(img.to(dev), y.to(dev), tok.to(dev))
    torch.cuda.synchronize()
    grads = {n: tr.grads[p].detach().clone() for n, p in w.model.named_parameters()
             if p.requires_grad}
    return loss.detach().clone(), probs.detach().clone(), grads, calls


@pytest.mark.parametrize("model", ["tiny", "w768"])
def test_exact_rows_keep_every_bit(cases, dev, monkeypatch, model):
    new = step(cases[model], dev, monkeypatch, True, True)
    blanked = step(cases[model], dev, monkeypatch, True, False)
    full = step(cases[model], dev, monkeypatch, False, True)
    # c_proj forward and c_fc dX of the last block; its attention backward
    assert new[3] == {"gemm_nt_rows": 2, "attn_bwd_live_row": 1}, new[3]
    assert blanked[3] == {"gemm_nt_rows": 0, "attn_bwd_live_row": 0}, blanked[3]
    assert full[3] == {"gemm_nt_rows": 0, "attn_bwd_live_row": 0}, full[3]
    for tag, other in (("knob off", blanked), ("LAST_ROWS off", full)):
        # (the scalar loss is a mean whose last bit varies from run to run of one configuration
        # on the tiny model, full-row path included: held to 1e-6, not to the bit)
        assert torch.equal(new[1], other[1]), (model, tag)
        assert abs(new[0].item() - other[0].item()) <= 1e-6 * abs(other[0].item()), (model, tag)
        assert set(new[2]) == set(other[2])
        for n in new[2]:
            assert torch.equal(new[2][n], other[2][n]), (model, tag, n)
    assert any(g.any() for n, g in new[2].items() if n.startswith("visual"))
