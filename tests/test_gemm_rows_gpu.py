"""ops.gemm_nt_rows (lc_gemm_nt_rows): a few rows of a large GEMM launch, from the compact operand,
bit for bit what the full launch writes to them.

Reference: ops.gemm_nt at M_full rows on an A that is zero off the live rows i * mul + add; the
live rows of both outputs are compared as integers (int16 / int32 views). Inputs are random normal
bf16, A at unit scale, B x 0.02.

The full launch sums a row of its split-K tail tiles slice by slice (gemm8_kernel: S slices of
nt / S k-tiles, added in slice order), another f32 order than a launch at n rows. The cases are
written for 256 CUs and each asserts, through ops.gemm_split_plan, that the launch it stands in
for has the stated S:

  a  M_full 514 x 128 = 65 792, N 256, K 1024: 257 tiles, 1 tail tile, S = 2 (the smallest split)
  b  M_full 128 x 200 = 25 600, N 768, K 2048: 300 tiles, 44 tail, S = 4; panel 85 holds column
     tile 0 whole and tiles 1, 2 split (live rows 21 800 and 22 000 lie in it)
  c  M_full 128 x 220 = 28 160, N 768, K 3072: 330 tiles, 74 tail, S = 3 (the step's 3 x 16
     k-tiles); also with add = 7
  d  as c at K = 768: no split, the launch at n rows alone has to match

Teeth (f32 output, cases a - c): the plain launch at n rows differs from the reference in more
than 25 % of the tail-tile elements (a CPU model of chunked f32 accumulation gives 70 - 84 % for
these K and S), so a fix-up that did nothing, or missed tiles, fails the comparison.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPI_BF16, EPI_F32, EPI_GELU = 0, 1, 3
CASES = {  # name: (n, mul, add, N, K, tiles, tail tiles, S)
    "a": (514, 128, 0, 256, 1024, 257, 1, 2),
    "b": (128, 200, 0, 768, 2048, 300, 44, 4),
    "c": (128, 220, 0, 768, 3072, 330, 74, 3),
    "c7": (128, 220, 7, 768, 3072, 330, 74, 3),
    "d": (128, 220, 0, 768, 768, 330, 0, 1),
}
FORMS = {"bf16_bias": (EPI_BF16, True), "bf16": (EPI_BF16, False), "f32": (EPI_F32, False)}


@pytest.fixture(scope="module")
def ops(dev):
    from lcclip import ops as _ops
    return _ops


_data = {}


def case_data(ops, dev, name):
    """Operands and the three full-launch references of one case, computed once: (A compact, B,
    bias, live row index, {form: reference rows})."""
    if name in _data:
        return _data[name]
    n, mul, add, N, K = CASES[name][:5]
    M_full = n * mul
    g = torch.Generator(device=dev).manual_seed(sum(map(ord, name)) + K)
    A = torch.randn(n, K, device=dev, generator=g).to(torch.bfloat16)
    B = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g)
    live = torch.arange(n, device=dev) * mul + add
    Af = torch.zeros(M_full, K, dtype=torch.bfloat16, device=dev)
    Af[live] = A
    ref = {}
    for form, (epi, with_bias) in FORMS.items():
        out = torch.empty(M_full, N, dtype=torch.float32 if epi == EPI_F32 else torch.bfloat16,
                          device=dev)
        ops.gemm_nt(Af, B, epi, out, bias=bias if with_bias else None)
        ref[form] = out[live].clone()
    del Af, out
    _data[name] = (A, B, bias, live, ref)
    return _data[name]


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_plan(ops, name):
    n, mul, add, N, K, tiles, tail, S = CASES[name]
    M_full = n * mul
    assert ((M_full + 255) // 256) * (N // 256) == tiles
    dp, s = ops.gemm_split_plan(M_full, N, K)
    assert (dp, s) == (tiles - tail, S), (name, dp, s)
    return dp


def tail_mask(name, dp, live, dev):
    """[n, N] bool: the elements whose full-launch tile (row-major raster: N < 2304) is split."""
    N = CASES[name][3]
    tiles_n = N // 256
    tile = (live // 256)[:, None] * tiles_n + (torch.arange(N, device=dev) // 256)[None, :]
    return tile >= dp


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_rows_match_full_launch(ops, dev, name, form):
    n, mul, add, N, K = CASES[name][:5]
    dp = check_plan(ops, name)
    A, B, bias, live, ref = case_data(ops, dev, name)
    epi, with_bias = FORMS[form]
    out = torch.empty(n, N, dtype=ref[form].dtype, device=dev)
    assert ops.gemm_nt_rows(A, B, epi, out, n * mul, mul, add, bias=bias if with_bias else None)
    assert torch.equal(bits(out), bits(ref[form])), (name, form)
    if form == "f32" and CASES[name][7] > 1:
        plain = torch.empty_like(out)
        ops.gemm_nt(A, B, epi, plain)
        tail = tail_mask(name, dp, live, dev)
        differs = (bits(plain) != bits(ref[form])) & tail
        frac = differs.sum().item() / tail.sum().item()
        print(f"gemm_nt_rows case {name}: plain launch differs in {frac:.3f} of the tail elements")
        assert frac > 0.25, (name, frac)
        # and nowhere else: the whole tiles need no fix-up
        assert torch.equal(bits(plain)[~tail], bits(ref[form])[~tail])


def test_rows_refusals(ops, dev):
    """Outside its scope the entry point returns the error and writes nothing."""
    from lcclip import _lib
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(3)

    def refused(n, mul, N, K, epi=EPI_BF16):
        A = torch.randn(n, K, device=dev, generator=g).to(torch.bfloat16)
        B = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        out = torch.full((n, N), 7.0, dtype=torch.bfloat16, device=dev)
        done = ops.gemm_nt_rows(A, B, epi, out, n * mul, mul, 0)
        torch.cuda.synchronize()
        return (not done) and bool((out == 7.0).all())

    assert refused(128, 220, 768, 3072, epi=EPI_GELU)  # an epilogue outside the scope
    assert refused(256, 128, 768, 2304)                # the hipBLASLt shape (M_full 32 768)
    assert lib.lc_gemm_set_streamk(1) == 0
    try:
        assert refused(128, 220, 768, 3072)            # a stream-K mode switched on
    finally:
        lib.lc_gemm_set_streamk(0)
    assert not refused(128, 220, 768, 3072)            # the same call is served otherwise
