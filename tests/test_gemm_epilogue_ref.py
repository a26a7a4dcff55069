"""No-GPU checks of the GEMM epilogue matrix (tests/test_gemm_epilogue_matrix_gpu.py): the
reference helpers on fixed cases, the cell table against the EpiList lines of gemm.hip, and the
range of the generated inputs."""
import torch

import gemm_epi_cases as C
import test_gemm_epilogue_matrix_gpu as G

BF, HF = C.BF, C.HF


def sp(x, dtype):
    return C.spacing(torch.tensor(x, dtype=torch.float64), dtype).item()


def test_spacing_fixed_cases():
    # at and around powers of two: the step doubles at 2^e, not before
    assert sp(1.0, BF) == 2.0 ** -7 and sp(1.0, HF) == 2.0 ** -10
    assert sp(2.0, BF) == 2.0 ** -6 and sp(2.0, HF) == 2.0 ** -9
    assert sp(2.0 - 2.0 ** -30, BF) == 2.0 ** -7 and sp(2.0 - 2.0 ** -30, HF) == 2.0 ** -10
    assert sp(0.5, BF) == 2.0 ** -8 and sp(0.5 - 2.0 ** -30, BF) == 2.0 ** -9
    assert sp(0.25, HF) == 2.0 ** -12 and sp(0.25 - 2.0 ** -30, HF) == 2.0 ** -13
    # negative values: the spacing of the magnitude
    assert sp(-1.0, BF) == 2.0 ** -7 and sp(-3.5, HF) == 2.0 ** -9 and sp(-0.75, BF) == 2.0 ** -8
    # zero and the subnormal range: the smallest subnormal
    assert sp(0.0, HF) == 2.0 ** -24 and sp(0.0, BF) == 2.0 ** -133
    assert sp(2.0 ** -14, HF) == 2.0 ** -24 and sp(2.0 ** -20, HF) == 2.0 ** -24
    assert sp(2.0 ** -13, HF) == 2.0 ** -23
    # the largest finite half
    assert sp(65504.0, HF) == 32.0 and sp(-65504.0, HF) == 32.0


def test_spacing_is_the_step_to_the_next_value():
    """Against the types themselves: x + spacing(x) is the next representable value."""
    for dtype in (BF, HF):
        x = torch.tensor([1.0, 1.5, 2.0, 3.0, 0.0625, 5.75, -1.0, -6.0, 2.0 ** -14], dtype=dtype)
        step = C.spacing(x.double(), dtype)
        up = (x.double().abs() + step).to(dtype)
        assert torch.equal(up.double(), x.double().abs() + step)  # representable
        between = (x.double().abs() + step / 2)
        assert (between.to(dtype).double() != between).all()  # and nothing in between


def test_guard_comparison_is_on_integers():
    for dtype in (BF, HF, torch.float32):
        buf = C.fill_sentinel(torch.empty(6, 10, dtype=dtype))
        assert torch.isnan(buf).all()  # the sentinel is a NaN: a float compare could never pass
        assert C.untouched(buf) and C.guards_intact(buf, 4, 8)
        buf[:4, :8] = 1.0
        assert C.guards_intact(buf, 4, 8) and not C.untouched(buf)
        for m, n in ((4, 0), (5, 9), (0, 8), (3, 9)):  # a guard row, a guard column
            b = buf.clone()
            b[m, n] = 0.0
            assert not C.guards_intact(b, 4, 8), (dtype, m, n)
        # another NaN is not the sentinel
        b = buf.clone()
        b[5, 5] = float("nan")
        assert not C.guards_intact(b, 4, 8)
        # no guards: a contiguous [M, N] buffer
        assert C.guards_intact(buf, 6, 10)


def test_exact_cast_rounds_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20,
                      -(1.0 + 2.0 ** -8)], dtype=torch.float64)
    got = C.exact_cast(x, BF).double()
    # ties go to the even neighbour (down, up), above the tie up; truncation would give 1, 1 + 2^-7
    assert got.tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0]
    h = C.exact_cast(torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], dtype=torch.float64), HF)
    assert h.double().tolist() == [1.0, 1.0 + 2.0 ** -9]


def test_cell_table_matches_gemm_hip():
    """The table of the GPU file equals the EpiList lines of gemm.hip on the public epilogues: an
    epilogue added to (or taken from) a family without its cell fails here."""
    lists = C.parse_epilists()
    assert {"NtEpis", "PpEpis", "G8Epis", "G8SkEpis", "W4Epis"} <= set(lists)
    for fam, names in C.FAMILY_EPIS.items():
        public = tuple(n for n in lists[fam] if n in C.EPI)
        assert sorted(public) == sorted(names), fam
    # every family list that is not stream-K's is in the table, every forced tile has a family
    assert set(lists) - {"G8SkEpis"} == set(C.FAMILY_EPIS)
    assert set(C.TILE_FAMILY) == set(C.TILES) == {1, 2, 3, 4, 5, 7, 8, 11}
    # the GPU file runs exactly the cells the lists give
    want, refuse = set(), set()
    for st in (BF, HF):
        for tile in C.TILES:
            have = {n for n in lists[C.TILE_FAMILY[tile]] if n in C.EPI}
            if tile == 8:  # the others of tile 8 run on the ping-pong kernel
                have |= {n for n in lists["PpEpis"] if n in C.EPI}
            for n in C.EPI:
                if n == "RESID16" and st == HF:
                    continue
                (want if n in have else refuse).add((st, tile, n))
    assert set(G.CELLS) == want and len(G.CELLS) == len(want)
    assert set(G.REFUSED) == refuse and len(G.REFUSED) == len(refuse)
    assert (BF, 7, "GELU") in refuse and (BF, 5, "RESID16") in refuse
    assert (BF, 8, "GELU_BWD") in want and (HF, 8, "BF16_F32") in want
    # ops numbers the epilogues as the table does
    from lcclip import ops
    for n, v in C.EPI.items():
        assert getattr(ops, "EPI_" + n) == v


def test_shapes_of_the_matrix():
    assert {(M, K) for M, N, K in G.SHAPES if N == 768} == {(m, k) for m in (293, 5)
                                                            for k in (128, 192, 64)}
    assert [s for s in G.SHAPES if s[1] != 768] == [(293, 64, 192)]


def test_inputs_are_exact_and_in_range():
    """Every (M, N, K) of the matrix: the inputs are exact in bf16 and half, max |pre| <= 16 for
    every epilogue, exact outputs are exact in f32, and the MUL / RESID16 products and sums do need
    rounding in the output type (else the cells could not tell truncation from rounding)."""
    for M, N, K in G.SHAPES:
        x = C.inputs(M, N, K)
        for key in ("A", "B", "mul", "bwd"):
            for dtype in (BF, HF):
                assert torch.equal(x[key].to(dtype).double(), x[key]), key
        assert torch.equal(x["mul_h"].to(HF).double(), x["mul_h"])
        assert torch.equal(x["resid16"].to(HF).double(), x["resid16"])
        assert torch.equal(x["resid"].float().double(), x["resid"])
        assert set(x["A"].unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert set((8 * x["B"]).unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert x["bias"].abs().max() <= 2 and torch.equal((4 * x["bias"]).round(), 4 * x["bias"])
        assert x["bwd"].abs().max() <= 6 and torch.equal((8 * x["bwd"]).round(), 8 * x["bwd"])
        for name in C.EPI:
            r = C.reference(M, N, K, name)
            assert r["pre"].abs().max().item() <= C.PRE_MAX, (M, N, K, name)
            assert torch.equal((16 * r["pre"]).round(), 16 * r["pre"])  # a multiple of 1/16
            for st in (BF, HF):
                r = C.reference(M, N, K, name, st)
                for i in (0, 1):
                    if r[f"out{i}"] is not None and r[f"exact{i}"]:
                        assert torch.equal(r[f"out{i}"].float().double(), r[f"out{i}"])
        if M * N >= 1000:
            for dtype in (BF, HF):
                mul = C.reference(M, N, K, "MUL", dtype)["out0"]
                assert (mul.to(dtype).double() != mul).float().mean() > 0.1, dtype
            r16 = C.reference(M, N, K, "RESID16")["out0"]
            assert (r16.to(HF).double() != r16).float().mean() > 0.1
