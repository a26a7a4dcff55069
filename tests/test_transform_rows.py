"""CPU side of the padded patch-row path: the row-width rule shared by the transforms and the
image tower, the new entry point's host-side refusals, and OnlineLoop.evaluate's use of an
evaluation transform (stub wrapper, tokenizer and transform: no kernels)."""
import ctypes

import pytest
import torch

ARCH14 = dict(embed_dim=64, image_resolution=28, vision_layers=2, vision_width=128,
              vision_patch_size=14, context_length=77, vocab_size=512, transformer_width=64,
              transformer_heads=1, transformer_layers=2)


def test_patch_row_width():
    from lcclip.transforms import patch_row_width
    assert [patch_row_width(p) for p in (14, 16, 32)] == [640, 768, 3072]
    assert patch_row_width(14, channels=1) == 256 and patch_row_width(16, 1) == 256
    assert patch_row_width(2) == 64


@pytest.mark.parametrize("patch,res", [(14, 28), (16, 32)])
def test_image_tower_stages_conv1_at_that_width(monkeypatch, patch, res):
    """ImageTower._stage asks transforms.patch_row_width for conv_k: the attribute follows
    whatever that function says."""
    from lcclip import AdapterCLIP, engine, transforms
    assert engine.patch_row_width is transforms.patch_row_width
    m = AdapterCLIP("tiny", peft_method="adapter", peft_encoder="both",
                    arch_overrides=dict(ARCH14, vision_patch_size=patch, image_resolution=res))
    tower = m.model.visual.tower
    monkeypatch.setattr(engine.ops, "merge_weight", lambda *a, **k: None)  # the one GPU call
    seen = []

    def rule(p, channels=3):
        seen.append((p, channels))
        return transforms.patch_row_width(p, channels) + 64
    monkeypatch.setattr(engine, "patch_row_width", rule)
    tower._stage()
    assert seen == [(patch, 3)]
    assert tower.conv_k == transforms.patch_row_width(patch) + 64
    if patch == 14:  # padded K: the weight's pad columns are zero
        assert tower.conv_w.shape == (128, 704)
        assert not tower.conv_w[:, 588:].any() and tower.conv_w[:, :588].any()


def test_rows_entry_refuses_on_the_host():
    """LC_EINVAL before any launch, so these need no GPU (the pointers are never read)."""
    from lcclip import _lib
    lib = _lib.load()
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    s = (ctypes.c_float * 3)(0.2, 0.2, 0.2)
    x, out = ctypes.c_void_p(4096), ctypes.c_void_p(4096)

    def rc(R=224, patch=14, ldo=640, o=out, std=s, crop=0):
        return lib.lc_train_transform_rows(None, 2, 3, 32, 32, x, R, 4, crop, 0, 0,
                                           ctypes.cast(m, ctypes.c_void_p),
                                           ctypes.cast(std, ctypes.c_void_p), 1, patch, ldo, o)
    assert rc(ldo=584) == -1            # ldo < 3 * 14^2
    assert rc(ldo=644) == -1            # ldo % 8
    assert rc(patch=7) == -1            # odd patch
    assert rc(patch=0) == -1
    assert rc(R=210) == -1              # R % 4
    assert rc(R=220) == -1              # R % patch
    assert rc(o=ctypes.c_void_p(4104)) == -1   # out not 16-B aligned
    assert rc(o=None) == -1
    assert rc(crop=9) == -1             # lc_train_transform's own checks
    assert rc(std=(ctypes.c_float * 3)(0.2, 0.0, 0.2)) == -1
    assert rc(patch=16, ldo=760) == -1


def test_transform_python_refusals():
    from lcclip.transforms import EvalTransform, TrainTransform
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="multiple of the patch"):
        TrainTransform((0.5,) * 3, (0.2,) * 3, inp_size=224, patch=12)(x, params=(0, 0, False),
                                                                      layout="patches")
    with pytest.raises(ValueError, match="multiple of the patch"):
        EvalTransform((0.5,) * 3, (0.2,) * 3, inp_size=224, patch=12)(x, layout="patches")
    with pytest.raises(ValueError, match="layout"):
        EvalTransform((0.5,) * 3, (0.2,) * 3)(x, layout="rows")
    with pytest.raises(ValueError, match="channels"):
        EvalTransform((0.5,), (0.2,))(x)


# ------------------------------------------------------------------------- OnlineLoop.evaluate
class StubWrapper:
    training = False

    def __init__(self):
        self.seen, self.tokens = [], None

    def set_token(self, t):
        self.tokens = t

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def __call__(self, x):
        self.seen.append(x)
        n = x.shape[0] if x.dim() == 4 else x.shape[0] // 4
        return torch.zeros(n, 4)


class StubEval:
    def __init__(self):
        self.calls = []

    def __call__(self, x, layout="nchw"):
        self.calls.append((x, layout))
        return torch.full((x.shape[0] * 4, 64), float(len(self.calls)))


def make_loop(eval_transform):
    from types import SimpleNamespace

    from lcclip.online import OnlineLoop
    from lcclip.stream import ClassBook
    wrapper = StubWrapper()
    trainer = SimpleNamespace(wrapper=wrapper, flat_p=torch.zeros(1))
    book = ClassBook([f"class{i}" for i in range(4)])
    book.add_new_class(torch.tensor([0, 1, 2, 3]))
    test_x = torch.arange(6 * 3 * 2 * 2, dtype=torch.float32).reshape(6, 3, 2, 2)
    test_y = torch.tensor([0, 1, 2, 3, 0, 1])
    loop = OnlineLoop(trainer, SimpleNamespace(num_tasks=2), book, test_x[:0], test_y[:0], test_x,
                      test_y, lambda names: torch.zeros(len(names), 77, dtype=torch.long),
                      test_batch=4, eval_transform=eval_transform)
    return loop, wrapper, test_x


def test_evaluate_applies_the_eval_transform_per_batch():
    ev = StubEval()
    loop, wrapper, test_x = make_loop(ev)
    res = loop.evaluate(4)
    assert wrapper.tokens.shape == (4, 77)
    assert [lay for _, lay in ev.calls] == ["patches", "patches"]      # 6 samples, batches of 4
    assert torch.equal(ev.calls[0][0], test_x[:4]) and torch.equal(ev.calls[1][0], test_x[4:])
    assert [tuple(x.shape) for x in wrapper.seen] == [(16, 64), (8, 64)]
    assert wrapper.seen[0][0, 0] == 1.0 and wrapper.seen[1][0, 0] == 2.0
    assert 0.0 <= res["avg_acc"] <= 1.0


def test_evaluate_without_eval_transform_hands_batches_over_unchanged():
    loop, wrapper, test_x = make_loop(None)
    loop.evaluate(4)
    assert len(wrapper.seen) == 2
    assert torch.equal(wrapper.seen[0], test_x[:4]) and torch.equal(wrapper.seen[1], test_x[4:])
