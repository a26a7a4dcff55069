"""BlockStack._spread / _gather (lcclip.engine, "the compact last block"): compact row i at row
i * L of a buffer that holds `fill` elsewhere, and back. Plain torch indexing, checked on CPU
tensors at n_seq = 3, L = 5, W = 8 against results built row by row: a fresh destination, a
destination that starts with the source (the clone), a caller-zeroed destination whose other rows
are not written, the lse shape, and the gather in place."""
import pytest
import torch

from lcclip.engine import BlockStack

N, L, W = 3, 5, 8


def numbered(rows, cols=W, start=1.0):
    """Distinct non-zero values."""
    return torch.arange(rows * cols, dtype=torch.float32).view(rows, cols) + start


def expected(src, n, seq, fill):
    want = torch.full((n * seq, src.shape[1]), fill, dtype=src.dtype)
    for i in range(n):
        want[i * seq] = src[i]
    return want


@pytest.mark.parametrize("fill", [0, 1e30])
def test_fresh_destination(fill):
    src = numbered(N)
    out = BlockStack._spread(src, N, L, fill=fill)
    assert out.shape == (N * L, W) and out.dtype == src.dtype
    assert torch.equal(out, expected(src, N, L, fill))
    assert torch.equal(src, numbered(N))


def test_destination_that_starts_with_the_source():
    buf = numbered(N * L + 2)
    before = buf.clone()
    out = BlockStack._spread(buf[:N], N, L, dst=buf[:N * L])
    assert out.data_ptr() == buf.data_ptr() and out.shape == (N * L, W)
    # (without the clone rows 0 and 2 * L would be read after the fill)
    assert torch.equal(buf[:N * L], expected(before[:N], N, L, 0))
    assert torch.equal(buf[N * L:], before[N * L:])


def test_live_rows_only_into_a_callers_buffer():
    src = numbered(N)
    dst = torch.full((N * L, W), -7.0)
    out = BlockStack._spread(src, N, L, dst=dst, fill=None)
    assert out is dst
    assert torch.equal(dst, expected(src, N, L, -7.0))


def test_callers_buffer_is_refilled():
    src = numbered(N)
    dst = torch.full((N * L + 1, W), -7.0)
    BlockStack._spread(src, N, L, dst=dst[:N * L])
    assert torch.equal(dst[:N * L], expected(src, N, L, 0))
    assert torch.equal(dst[N * L:], torch.full((1, W), -7.0))


def test_lse_shape():
    H = 2
    lse = numbered(N * H, 1).view(-1)
    out = BlockStack._spread(lse.view(-1, 1), N * H, L, fill=1e30).view(N * H, L)
    want = torch.full((N * H, L), 1e30)
    want[:, 0] = lse
    assert torch.equal(out, want)


@pytest.mark.parametrize("n,seq", [(N, L), (7, 3)])  # (7, 3): rows 3 and 6 are read and written
def test_gather_in_place_and_into_another_buffer(n, seq):
    buf = numbered(n * seq + 2)
    before = buf.clone()
    want = torch.stack([before[i * seq] for i in range(n)])
    out = torch.zeros(n, W)
    BlockStack._gather(buf[:n * seq], n, seq, out)
    assert torch.equal(out, want) and torch.equal(buf, before)
    BlockStack._gather(buf[:n * seq], n, seq, buf[:n])
    assert torch.equal(buf[:n], want)
    assert torch.equal(buf[n:], before[n:])


def test_round_trip():
    src = numbered(N)
    out = torch.empty(N, W)
    BlockStack._gather(BlockStack._spread(src, N, L), N, L, out)
    assert torch.equal(out, src)
