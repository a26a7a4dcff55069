"""The argument checks of the step-tail entry points (csrc/head.hip, the AdamW / counter block of
csrc/peft.hip), without a GPU, as test_attn_long_args.py does for the long attention.

Every call carries one argument that the check rejects, so it returns LC_EINVAL before any launch,
through ctypes on the built library; the two calls that are valid (n = 0) return LC_OK before any
launch as well. The buffer is never read or written.
"""
import ctypes

import pytest

import tail_cases as T

LC_OK, LC_EINVAL = 0, -1

ORDER = {
    "lc_l2norm_rows": "st R E p_f ldf p_out p_norms",
    "lc_clip_head": "st B C E p_img p_txt p_ls p_labels p_probs p_dlogits p_loss",
    "lc_head_logits": "st B C E p_img p_txt p_ls p_logits p_probs",
    "lc_softmax_bwd_rows": "st B C p_probs p_dprobs p_dlogits",
    "lc_head_feat_grad": "st R Co E p_dlogits sr sc p_other p_self p_norms p_ls p_ext p_dF",
    "lc_grad_pow2_normalize": "st n p_x p_scale target",
    "lc_add_unscaled": "st n p_y p_x p_scale",
    "lc_check_finite": "st n p_g p_flag",
    "lc_adamw": "st n p_p p_g p_m p_v lr b1 b2 eps wd step p_skip p_stepdev",
    "lc_counter_add": "st n p_ctr delta",
    "lc_adam_step_advance": "st p_ctr p_skip",
}
VALID = dict(st=None, R=2, B=2, C=3, Co=3, E=8, ldf=8, sr=3, sc=1, n=4, target=10, step=1, delta=1,
             lr=5e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)
HEAD_SHAPE = [dict(B=0), dict(C=0), dict(E=0), dict(E=T.E_MAX + 1), dict(C=T.C_MAX + 1), dict(B=-1)]
REJECTED = {
    "lc_l2norm_rows": [dict(R=0), dict(E=0), dict(ldf=7), dict(E=T.E_MAX, ldf=T.E_MAX - 1)],
    "lc_clip_head": HEAD_SHAPE,
    "lc_head_logits": HEAD_SHAPE,
    "lc_softmax_bwd_rows": [dict(B=0), dict(C=0)],
    "lc_head_feat_grad": [dict(R=0), dict(Co=0), dict(E=0), dict(E=T.E_MAX + 1)],
    "lc_grad_pow2_normalize": [dict(n=0), dict(p_x=None), dict(p_scale=None),
                               dict(target=T.TARGET_MAX + 1), dict(target=-T.TARGET_MAX - 1)],
    "lc_add_unscaled": [dict(n=0), dict(p_y=None), dict(p_x=None), dict(p_scale=None)],
    "lc_check_finite": [dict(n=-1)],
    "lc_adamw": [dict(n=-1), dict(step=0, p_stepdev=None), dict(step=-3, p_stepdev=None),
                 dict(n=0, step=0, p_stepdev=None)],
    "lc_counter_add": [dict(n=0), dict(n=T.CTR_MAX + 1), dict(p_ctr=None)],
    "lc_adam_step_advance": [dict(p_ctr=None)],
}
# valid without a launch: nothing to do
ACCEPTED = {"lc_check_finite": [dict(n=0)],
            "lc_adamw": [dict(n=0), dict(n=0, step=0)]}


@pytest.fixture(scope="module")
def lib():
    from lcclip import _lib
    return _lib.load()


def _args(order, case, base):
    args = []
    for key in order.split():
        if key.startswith("p_"):
            args.append(ctypes.c_void_p(base) if case.get(key, "ok") is not None else None)
        else:
            args.append(case.get(key, VALID.get(key)))
    return args


def test_every_check_rejects(lib):
    buf = ctypes.create_string_buffer(4096 + 256)
    base = (ctypes.addressof(buf) + 255) & ~255
    made = 0
    for name, order in ORDER.items():
        for case in REJECTED[name]:
            assert getattr(lib, name)(*_args(order, case, base)) == LC_EINVAL, (name, case)
            made += 1
    assert made == 4 + 6 + 6 + 2 + 4 + 5 + 4 + 1 + 4 + 3 + 1


def test_empty_vectors_return_ok_without_a_launch(lib):
    buf = ctypes.create_string_buffer(4096 + 256)
    base = (ctypes.addressof(buf) + 255) & ~255
    for name, cases in ACCEPTED.items():
        for case in cases:
            assert getattr(lib, name)(*_args(ORDER[name], case, base)) == LC_OK, (name, case)
    assert bytes(buf) == bytes(len(buf))
