"""lc_patchify_pad on the MI355X: conv1's im2col rows for any patch size at a padded row stride
(ViT-L/14: patch 14, 588 -> 640 columns), against the oracle's patchify, bit for bit, in both
storage types; the pad columns zero; nothing written outside `out`; lc_patchify's bits where
both apply."""
import pytest
import torch

from oracle import clip_oracle as o

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A
GUARD = 64


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("n,res,P,ldo", [(2, 28, 14, 640), (1, 224, 14, 640), (2, 64, 16, 768),
                                         (1, 64, 32, 3072)])
def test_patchify_pad(dev, dtype, n, res, P, ldo):
    from lcclip import ops
    img = o.synthetic_images(n, res, seed=7)
    g = res // P
    rows, cols = n * g * g, 3 * P * P
    want = o.patchify(img, P).reshape(rows, cols).to(dtype)
    buf = torch.full((rows + 2 * GUARD, ldo), SENTINEL, device=dev, dtype=torch.int16).view(dtype)
    out = buf[GUARD:GUARD + rows]
    ops.patchify_pad(img.to(dev), P, out)
    got = out.cpu()
    assert torch.equal(got[:, :cols].view(torch.int16), want.view(torch.int16))
    assert (got[:, cols:].view(torch.int16) == 0).all()
    guard = buf.view(torch.int16)
    assert (guard[:GUARD] == SENTINEL).all() and (guard[GUARD + rows:] == SENTINEL).all()
    if P % 8 == 0 and ldo == cols:
        plain = torch.empty((rows, cols), device=dev, dtype=dtype)
        ops.patchify(img.to(dev), P, plain)
        assert torch.equal(plain.view(torch.int16), out.view(torch.int16))
