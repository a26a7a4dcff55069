"""ViT-L/14, the reference adapter script's model (scripts/adapter_clip.sh:30), on the public
surface, without a GPU: the architecture table, the script's spelling of the name, and the
reference's logged parameter counts (nohup.out:8,29)."""
import pytest
import torch

from oracle import clip_oracle as o

TOTAL, TRAINABLE = 431_977_985, 4_361_472


@pytest.mark.parametrize("name", ["ViT-L/14", "ViT-L-14"])
def test_vit_l14_surface_counts(name):
    from lcclip import AdapterCLIP, freeze_backbone
    m = AdapterCLIP(name, "adapter", "both")
    assert sum(p.numel() for p in m.parameters()) == TOTAL
    freeze_backbone(m)
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == TRAINABLE
    got = {k[len("model."):]: tuple(v.shape) for k, v in m.named_parameters()}
    want = {k: tuple(v) for k, v in o.param_shapes(o.VIT_L14, "adapter", "both").items()}
    assert got == want


def test_architecture_table():
    from lcclip import available_models, clip_loader
    names = available_models()
    assert "ViT-B/16" in names and "ViT-B/32" in names and "ViT-L/14" in names
    a = clip_loader.ARCHITECTURES["ViT-L/14"]
    assert (a["embed_dim"], a["vision_layers"], a["vision_width"], a["vision_patch_size"]) == \
        (768, 24, 1024, 14)
    assert (a["transformer_width"], a["transformer_heads"], a["transformer_layers"]) == (768, 12, 12)
    with pytest.raises(RuntimeError, match="not found"):
        clip_loader.load("ViT-L/15")


def test_attention_routing_limit():
    """ops.attn_fwd / attn_bwd refuse more than 512 tokens by name, before the library is asked."""
    from lcclip import ops
    assert (ops.ATTN_ROW_MAX_L, ops.ATTN_MAX_L) == (256, 512)
    t = torch.zeros(513, 192, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="512"):
        ops.attn_fwd(t, t[:, :64], torch.zeros(1, 513), 1, 513, 1, False)
    with pytest.raises(ValueError, match="512"):
        ops.attn_bwd(t, t[:, :64], t[:, :64], torch.zeros(1, 513), t.clone(), 1, 513, 1, False)
