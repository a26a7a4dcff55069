"""The long attention entry points' argument check (csrc/attention.hip: check(), E_LONG_FWD /
E_LONG_BWD), without a GPU, as test_attn_args.py does for the six entry points up to 256 tokens.

Every call carries one argument that the check rejects, so it returns LC_EINVAL before any launch,
through ctypes on the built library, for the bf16 and the IEEE-half symbols. No call has valid
arguments: that would launch. The buffer is never read or written.

257 <= L <= 512: L = 256 belongs to lc_attn_fwd / lc_attn_bwd and is refused here, so every length
has one home. The 32-bit-offset bound is ld < 2^21 elements (512 padded rows, half the stride of
the 256-row families).
"""
import ctypes

import pytest

LC_EINVAL = -1
BIG21 = 1 << 21

ORDER = {
    "lc_attn_long_fwd": "st n_seq L H p_qkv ldq p_O ldo p_lse causal",
    "lc_attn_long_bwd": "st n_seq L H p_qkv ldq p_O p_dO ldo p_lse p_dqkv lddq causal",
}
# 2 sequences of 257 tokens, 2 heads: D = 128, qkv / dqkv rows of 384, O rows of 128
VALID = dict(st=None, n_seq=2, L=257, H=2, ldq=384, ldo=128, lddq=384, causal=0)

SHAPE = [dict(n_seq=0), dict(L=256), dict(L=513), dict(H=0), dict(ldq=376), dict(ldq=388),
         dict(ldo=120), dict(ldo=132)]
BOUND_IN = [dict(ldq=BIG21), dict(L=512, ldq=BIG21), dict(ldo=BIG21)]
REJECTED = {
    "lc_attn_long_fwd": SHAPE + BOUND_IN + [dict(p_O="odd")],
    "lc_attn_long_bwd": SHAPE + BOUND_IN + [dict(lddq=376), dict(lddq=388), dict(p_dqkv="odd"),
                                            dict(lddq=BIG21), dict(L=512, lddq=BIG21)],
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
        fn = getattr(lib, name + suffix)
        for case in REJECTED[name]:
            args = []
            for key in order.split():
                v = case.get(key, VALID.get(key, "ok"))
                if key.startswith("p_"):
                    v = ctypes.c_void_p(base + (8 if v == "odd" else 0))
                args.append(v)
            assert fn(*args) == LC_EINVAL, (name + suffix, case)
            made += 1
    assert made == 12 + 16


@pytest.mark.parametrize("suffix", ["", "_f16"])
def test_short_entry_points_still_refuse_long_lengths(lib, suffix):
    """The other half of "one home per length": 257 stays LC_EINVAL in lc_attn_fwd / lc_attn_bwd."""
    buf = ctypes.create_string_buffer(4096 + 256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    assert getattr(lib, "lc_attn_fwd" + suffix)(None, 2, 257, 2, p, 384, p, 128, p, 0) == LC_EINVAL
    assert getattr(lib, "lc_attn_bwd" + suffix)(None, 2, 257, 2, p, 384, p, p, 128, p, p, 384,
                                                0) == LC_EINVAL
