"""MVP-CLIP training method, the parts that need no GPU: the float64 restatements check
themselves (the literal loop of backward passes against the closed form, AFS on against off),
MVPTrainer's bookkeeping on a CPU-constructed TINY CLIP_MVP (no kernel is called), and the
cross-compile of mvp.hip (no spills, no private segment)."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import mvp_method_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "lifelong-clip_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TINY_ARCH = dict(embed_dim=64, image_resolution=64, vision_layers=2, vision_width=128,
                 vision_patch_size=16, context_length=77, vocab_size=512, transformer_width=64,
                 transformer_heads=1, transformer_layers=2)


def head_case(B, C, E, exposed, seed, dtype=torch.float64, scale=100.0):
    """Features, labels (repeats; at least one exposed class without a sample), pre-sigmoid mask
    rows and the 0 / -inf class mask of one head problem."""
    g = torch.Generator().manual_seed(seed)
    i = torch.randn(B, E, generator=g, dtype=torch.float64)
    t = torch.randn(C, E, generator=g, dtype=torch.float64)
    mp = -1.0 + 0.5 * torch.randn(B, C, generator=g, dtype=torch.float64)
    y = torch.randint(0, exposed - 1, (B,), generator=g)  # class exposed-1 never sampled
    y[1] = y[0]
    cmask = torch.full((C,), float("-inf"), dtype=torch.float64)
    cmask[:exposed] = 0
    ls = torch.tensor(scale, dtype=torch.float64).log()
    return [v.to(dtype) if v.is_floating_point() else v for v in (i, t, mp, y, cmask, ls)]


@pytest.mark.parametrize("B,C,E,exposed", [(5, 4, 64, 3), (7, 6, 64, 6)])
@pytest.mark.parametrize("scale", [100.0, 20.0])
def test_closed_form_matches_loop_of_backwards(B, C, E, exposed, scale):
    i, t, mp, y, cmask, ls = head_case(B, C, E, exposed, seed=B, scale=scale)
    mask = torch.sigmoid(mp) * 2
    sg_l, bg_l = R.grads_loop(i, t, y, mask, cmask, ls)
    sg_c, bg_c, _ = R.grads_closed(i, t, y, mask, cmask, ls)
    assert (sg_l - sg_c).abs().max() < 1e-12 * max(1.0, sg_l.abs().max().item())
    assert (bg_l - bg_c).abs().max() < 1e-12 * max(1.0, bg_l.abs().max().item())
    ign_l, cps_l = R.scores(i, t, y, mask, cmask, ls, 0.5, closed=False)
    ign_c, cps_c = R.scores(i, t, y, mask, cmask, ls, 0.5, closed=True)
    assert (ign_l - ign_c).abs().max() < 1e-12
    assert torch.equal(cps_l, cps_c)


@pytest.mark.parametrize("B,C,E,exposed", [(5, 4, 64, 3), (7, 6, 64, 6)])
def test_afs_is_identity_for_positive_cps(B, C, E, exposed):
    i, t, mp, y, cmask, ls = head_case(B, C, E, exposed, seed=10 + B)
    out = []
    for afs in (False, True):
        iv = i.clone().requires_grad_(True)
        loss, _, cps = R.method_loss(iv, t, mp, cmask, y, ls, use_afs=afs, use_gsf=True)
        loss.backward()
        out.append((loss.detach(), iv.grad))
        assert (cps > 0).all()
    assert abs(out[0][0] - out[1][0]) < 1e-12 * max(1.0, abs(out[0][0].item()))
    assert (out[0][1] - out[1][1]).norm() < 1e-12 * out[0][1].norm()


def tiny_mvp(**kw):
    from lcclip.mvp_clip import CLIP_MVP
    torch.manual_seed(0)
    return CLIP_MVP(model_name="tiny", arch_overrides=TINY_ARCH, device=None, num_classes=12,
                    task_num=4, **kw)


def test_pool_kernels_defaults_off():
    m = tiny_mvp()
    assert m.pool_kernels is False
    assert tiny_mvp(pool_kernels=True).pool_kernels is True


def test_trainer_bookkeeping_cpu():
    from lcclip.mvp_trainer import MVPTrainer
    m = tiny_mvp()
    before = {k: getattr(m, k).detach().clone() for k in ("key", "mask", "g_prompts", "e_prompts")}
    names = [f"c{i}" for i in range(12)]
    tr = MVPTrainer(m, class_names=names, use_mask=True, use_contrastiv=True,
                    use_last_layer=False, use_afs=True, use_gsf=True)
    # the flags reach the module (methods/mvp_clip.py:294-298); the trainer turns the kernels on
    assert m.use_mask and m.use_contrastiv and not m.use_last_layer and m.pool_kernels
    assert MVPTrainer(tiny_mvp(), pool_kernels=False).model.pool_kernels is False
    # flat_p aliases the four parameters (values kept), flat_g their gradients
    off = 0
    for k in ("key", "mask", "g_prompts", "e_prompts"):
        p = getattr(m, k)
        assert torch.equal(p.detach(), before[k])
        assert p.data_ptr() == tr.flat_p[off:].data_ptr()
        assert p.grad.data_ptr() == tr.flat_g[off:].data_ptr()
        off += p.numel()
    assert off == tr.numel == tr.flat_p.numel() == tr.m.numel() == tr.v.numel()
    tr.flat_p[0] = 7.0
    assert m.key.detach().reshape(-1)[0] == 7.0
    # class mask: -inf until exposed (methods/mvp_clip.py:47, 319-321)
    assert torch.isinf(tr.class_mask).all() and tr.class_mask.shape == (12,)
    tr.add_new_class(torch.tensor([5, 2, 5, 9]))
    assert tr.book.exposed_classes == [5, 2, 9]
    assert tr.class_mask[:3].tolist() == [0, 0, 0] and torch.isinf(tr.class_mask[3:]).all()
    assert m.exposed_classes == 3
    assert tr.train_classes() == ([5, 2, 9], ["c5", "c2", "c9"])
    assert tr.remap(torch.tensor([5, 2, 5, 9])).tolist() == [0, 1, 0, 2]
    # the next batch: the batch-visible list is that batch's classes, the exposed list grows
    tr.add_new_class(torch.tensor([9, 1]))
    assert tr.book.exposed_classes == [5, 2, 9, 1]
    assert tr.train_classes()[0] == [9, 1]
    assert tr.remap(torch.tensor([1, 9, 9])).tolist() == [1, 0, 0]
    assert tr.class_mask[:4].tolist() == [0, 0, 0, 0] and torch.isinf(tr.class_mask[4:]).all()
    # visible_classes 'all': the exposed list
    tr_all = MVPTrainer(tiny_mvp(), class_names=names, visible_classes="all")
    tr_all.add_new_class(torch.tensor([3, 4]))
    tr_all.add_new_class(torch.tensor([8]))
    assert tr_all.train_classes()[0] == [3, 4, 8]
    # reset_optimizer zeroes the Adam state
    tr.m.fill_(1.0)
    tr.v.fill_(2.0)
    tr.adam_step.fill_(5)
    tr.step_count = 5
    tr.reset_optimizer()
    assert tr.m.abs().sum() == 0 and tr.v.abs().sum() == 0
    assert tr.adam_step.item() == 0 and tr.step_count == 0


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_mvp_hip_cross_compiles_without_spills(tmp_path):
    src = os.path.join(ROOT, "lifelong-clip_amd", "csrc", "mvp.hip")
    out = tmp_path / "mvp.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only",
                    "-S", "-I", os.path.join(ROOT, "include"), src, "-o", str(out)], check=True)
    text = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*mvp_\S+)", text)
    assert len(set(kernels)) >= 14, kernels
    for field in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        vals = [int(v) for v in re.findall(rf"\.{field}:\s+(\d+)", text)]
        assert vals and all(v == 0 for v in vals), (field, vals)
