"""The attention entry points' argument check (csrc/attention.hip: check()), without a GPU.

Every call here carries one argument that the check rejects, so it returns LC_EINVAL before any
launch: the calls of tools/attn_host_check.cpp (which runs them under a sanitizer), through ctypes
on the built library, for the bf16 and the IEEE-half symbols. No call has valid arguments: that
would launch. The buffer is never read or written.

The 32-bit-offset bound is one bound on the row strides (ld < 2^22 elements; the fp8 form's
lddq, in bytes, < 2^23) and holds in all six launching entry points.
"""
import ctypes

import pytest

LC_EINVAL = -1
BIG22, BIG23 = 1 << 22, 1 << 23

# argument order of each entry point (include/lc_clip.h); `p_*` are pointers
ORDER = {
    "lc_attn_fwd": "st n_seq L H p_qkv ldq p_O ldo p_lse causal",
    "lc_attn_bwd": "st n_seq L H p_qkv ldq p_O p_dO ldo p_lse p_dqkv lddq causal",
    "lc_attn_bwd_fp8": "st n_seq L H p_qkv ldq p_O p_dO ldo p_lse p_dqkv lddq p_qs q_rows causal",
    "lc_attn_row_fwd": "st n_seq L H p_qkv ldq row p_O ldo p_lse causal",
    "lc_attn_row_bwd": "st n_seq L H p_qkv ldq row p_O p_dO ldo p_lse p_dqkv lddq causal",
    "lc_attn_bwd_live_row": "st n_seq L H p_qkv ldq row p_O p_dO ldo p_lse p_dqkv lddq causal",
}
# 2 sequences of 64 tokens, 2 heads: D = 128, qkv / dqkv rows of 384, O rows of 128
VALID = dict(st=None, n_seq=2, L=64, H=2, ldq=384, ldo=128, lddq=384, row=0, q_rows=256, causal=0)

SHAPE = [dict(n_seq=0), dict(L=0), dict(L=257), dict(H=0), dict(ldq=376), dict(ldq=388),
         dict(ldo=120), dict(ldo=132)]
BOUND_IN = [dict(L=256, ldq=BIG22), dict(ldq=BIG22), dict(ldo=BIG22)]
GRAD = [dict(lddq=376), dict(lddq=388), dict(p_dqkv="odd"), dict(L=256, lddq=BIG22),
        dict(lddq=BIG22)]
ROW = [dict(row=-1), dict(row=64), dict(p_O="odd")]
REJECTED = {
    "lc_attn_fwd": SHAPE + BOUND_IN + [dict(p_O="odd")],
    "lc_attn_bwd": SHAPE + BOUND_IN + GRAD,
    "lc_attn_bwd_fp8": [c for c in SHAPE if c != dict(L=257)] + BOUND_IN + [
        dict(L=225, q_rows=512), dict(lddq=368), dict(lddq=392), dict(p_dqkv="odd"),
        dict(p_qs=None), dict(q_rows=128), dict(q_rows=0), dict(lddq=BIG23)],
    "lc_attn_row_fwd": SHAPE + BOUND_IN + ROW,
    "lc_attn_row_bwd": SHAPE + BOUND_IN + GRAD + ROW + [dict(p_dO="odd")],
    "lc_attn_bwd_live_row": SHAPE + BOUND_IN + GRAD + ROW + [dict(p_dO="odd")],
}


@pytest.fixture(scope="module")
def lib():
    from lcclip import _lib
    return _lib.load()


@pytest.mark.parametrize("suffix", ["", "_f16"])
def test_every_check_rejects(lib, suffix):
    buf = ctypes.create_string_buffer(4096 + 256)
    base = (ctypes.addressof(buf) + 255) & ~255
    made = 0
    for name, order in ORDER.items():
        if suffix and name == "lc_attn_bwd_fp8":  # bf16 in, fp8 out: no IEEE-half form is bound
            continue
        fn = getattr(lib, name + suffix)
        for case in REJECTED[name]:
            args = []
            for key in order.split():
                v = case.get(key, VALID.get(key, "ok"))
                if key.startswith("p_"):
                    v = None if v is None else ctypes.c_void_p(base + (8 if v == "odd" else 0))
                args.append(v)
            assert fn(*args) == LC_EINVAL, (name + suffix, case)
            made += 1
    assert made == (82 if suffix else 100)


@pytest.mark.parametrize("suffix", ["", "_f16"])
def test_set_form_range(lib, suffix):
    set_form = getattr(lib, "lc_attn_bwd_set_form" + suffix)
    try:
        for form in (0, 1, 2, 3):
            assert set_form(form) == 0, form
        for form in (-1, 4):
            assert set_form(form) == LC_EINVAL, form
    finally:
        assert set_form(0) == 0
