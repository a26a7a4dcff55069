"""The prompt-row machinery of lcclip.engine ("prompt rows"): BlockStack.row_plan, the forward
helpers _rows_in / _rows_out and backward's _GradBufs, on CPU tensors at n = 2, L = 3, D = 4
against a literal restatement of the reference's rule — cat the prompts, run the block, take
x[:, :L] (models/mvp_clip.py:158-175) — and of MaPLe's row replacement. Small integers in
float32 / bfloat16, so every comparison is exact."""
import pytest
import torch

from lcclip.engine import BlockStack, _GradBufs, _Rows

N, L, D = 2, 3, 4

# (appended rows per layer, {layer: (row, count)} replaced, stop)
PATTERNS = {
    "runs": ([2, 2, 0, 3, 3, 3, 0], {}, None),
    "prompt_first": ([2, 0, 1], {}, None),
    "prompt_last": ([0, 0, 3], {}, None),
    "different_counts": ([2, 3, 3, 1], {}, None),
    "replace_first": ([0, 0, 0], {0: (1, 2)}, None),
    "replace_after_prompt": ([2, 2, 2], {1: (1, 1)}, None),
    "stop_cuts_run": ([3, 3, 3, 3], {}, 2),
    "replace_in_plain": ([0, 2, 0, 0], {2: (0, 2), 3: (2, 1)}, None),
}
# the plan with PROMPT_KEEP on: (P, inherit, keep, R) per layer that runs
EXPECTED = {
    "runs": [(2, False, True, None), (2, True, False, None), (0, False, False, None),
             (3, False, True, None), (3, True, True, None), (3, True, False, None),
             (0, False, False, None)],
    "prompt_first": [(2, False, False, None), (0, False, False, None), (1, False, False, None)],
    "prompt_last": [(0, False, False, None), (0, False, False, None), (3, False, False, None)],
    "different_counts": [(2, False, False, None), (3, False, True, None), (3, True, False, None),
                         (1, False, False, None)],
    "replace_first": [(0, False, False, (1, 2)), (0, False, False, None), (0, False, False, None)],
    "replace_after_prompt": [(2, False, False, None), (2, False, True, (1, 1)),
                             (2, True, False, None)],
    "stop_cuts_run": [(3, False, True, None), (3, True, False, None)],
    "replace_in_plain": [(0, False, False, None), (2, False, False, None),
                         (0, False, False, (0, 2)), (0, False, False, (2, 1))],
}


def plan_of(name, keep):
    P, R, stop = PATTERNS[name]
    P_of = {i: p for i, p in enumerate(P) if p}
    return BlockStack.row_plan(len(P), P_of, R, stop, keep)


def numbered(*shape, start=1, dtype=torch.float32):
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, dtype=torch.float32) + start).view(*shape).to(dtype)


def tensors(name):
    """{layer: prompts [N, P, D]} and {layer: (row, rows [N, count, D])}, distinct values."""
    P, R, _ = PATTERNS[name]
    prompts = {i: numbered(N, p, D, start=100 * (i + 1)) for i, p in enumerate(P) if p}
    replace = {i: (r0, numbered(N, c, D, start=1000 * (i + 1))) for i, (r0, c) in R.items()}
    return prompts, replace


# ----------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_plan(name):
    P, R, stop = PATTERNS[name]
    plan = plan_of(name, True)
    assert [tuple(p) for p in plan] == EXPECTED[name]
    assert all(isinstance(p, _Rows) for p in plan)
    assert len(plan) == (len(P) if stop is None else min(stop, len(P)))
    for i, p in enumerate(plan):
        # the layer runs at L + P rows whatever is kept; rows are inherited exactly when the
        # previous layer kept the same count, and a replacing layer never inherits
        assert p.P == P[i] and p.R == R.get(i)
        assert p.inherit == (i > 0 and plan[i - 1].keep)
        assert not (p.inherit and p.R is not None)
        if p.keep:
            assert i + 1 < len(plan) and P[i + 1] == p.P > 0
        assert p.plain == (not P[i] and i not in R)
    assert not plan[-1].keep


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_plan_without_keeping(name):
    on, off = plan_of(name, True), plan_of(name, False)
    assert [(p.P, p.R) for p in on] == [(p.P, p.R) for p in off]
    assert not any(p.keep or p.inherit for p in off)


# ----------------------------------------------------------------------------- rows in / out
def block(x, layer):
    """Stand-in block on [N, Lx, D]: every output row is distinct, depends on the layer, its row
    and — like attention — every row of its sequence (the appended ones included)."""
    rows = torch.arange(x.shape[1], dtype=x.dtype).view(1, -1, 1)
    return x + 1000 * (layer + 1) + 10 * rows + x.sum(dim=1, keepdim=True)


def reference_forward(x0, name):
    P, R, stop = PATTERNS[name]
    prompts, replace = tensors(name)
    x = x0.view(N, L, D).clone()
    for i in range(len(P) if stop is None else min(stop, len(P))):
        if i in replace:
            r0, pr = replace[i]
            x = x.clone()
            x[:, r0:r0 + pr.shape[1]] = pr
        if P[i]:
            x = torch.cat([x, prompts[i]], dim=1)
        x = block(x, i)[:, :L]
    return x.reshape(N * L, D)


def engine_forward(x0, name, keep):
    prompts, replace = tensors(name)
    x = x0
    for idx, p in enumerate(plan_of(name, keep)):
        x = BlockStack._rows_in(x, p, idx, N, L, prompts, replace)
        assert x.shape == (N * (L + p.P), D)
        x_out = block(x.view(N, L + p.P, D), idx).reshape(N * (L + p.P), D)
        x = BlockStack._rows_out(x_out, p, N, L)
    return x


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_rows_in_and_out(name):
    x0 = numbered(N * L, D)
    before = x0.clone()
    want = reference_forward(x0, name)
    kept = engine_forward(x0, name, True)
    copied = engine_forward(x0, name, False)
    assert torch.equal(x0, before)  # the caller's input is never written
    # (a run cut by stop still ends with its rows dropped: the last planned layer keeps none)
    assert kept.shape == (N * L, D)
    assert torch.equal(kept, copied)
    assert torch.equal(kept, want)


# ----------------------------------------------------------------------------- _GradBufs
def reference_backward(g_out, plan):
    """By rows: the dropped rows of a prompt layer's output carry zero gradient, the layer's
    backward is the identity plus li + 1, an appended row's input gradient is its prompt's, a
    replaced row's is reported and stops."""
    g, pg = g_out.view(N, L, D).clone(), {}
    for li in range(len(plan) - 1, -1, -1):
        p = plan[li]
        if p.P:
            g = torch.cat([g, torch.zeros(N, p.P, D)], dim=1)
        g = g + (li + 1)
        if p.R is not None:
            r0, c = p.R
            pg[("R", li)] = g[:, r0:r0 + c].clone()
            g[:, r0:r0 + c] = 0
        if p.P:
            pg[li] = g[:, L:].clone()
            g = g[:, :L]
    return g.reshape(N * L, D), pg


def bufs_backward(plan, dx, dxb, keep_input):
    """BlockStack.backward's use of _GradBufs with the stand-in layer."""
    Mmax = N * (L + max(p.P for p in plan))
    bufs = _GradBufs(dx, dxb, N, L, Mmax, None if dxb is None else dxb.dtype, keep_input, None)
    pg, stopped = {}, []  # stopped: (row, count) replaced in the layer above
    for li in range(len(plan) - 1, -1, -1):
        p = plan[li]
        Lx = L + p.P
        if p.P and not p.pkeep:
            bufs.expand(p.P)
        gx, gxb = bufs.current(N * Lx)
        assert gx.shape == (N * Lx, D) and (gxb is None) == (dxb is None)
        for g in (gx, gxb):
            if g is not None:
                v = g.view(N, Lx, D).float()
                assert not p.P or v[:, L:].abs().max() == 0  # dropped or inherited rows
                for r0, c in stopped:
                    assert v[:, r0:r0 + c].abs().max() == 0
        ox, oxb = bufs.output(p.P)
        assert ox.shape == (N * Lx, D) and ox.data_ptr() != gx.data_ptr()
        ox.copy_(gx + (li + 1))
        if oxb is not None:
            oxb.copy_(gxb + (li + 1))
        bufs.take_replaced(li, p.R, pg)
        bufs.advance(li, p.P, p.inherit, None, pg)
        stopped = [p.R] if p.R is not None else []
    return bufs.result(), pg


class _P:
    """The plan entry as backward reads it from a layer's record (pkeep for keep)."""

    def __init__(self, rows):
        self.P, self.inherit, self.pkeep, self.R = rows


@pytest.mark.parametrize("half_copy", [True, False])
@pytest.mark.parametrize("keep_input", [True, False])
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_grad_bufs(name, keep, keep_input, half_copy):
    plan = plan_of(name, keep)
    dx = numbered(N * L, D)
    dxb = dx.to(torch.bfloat16) if half_copy else None
    before = dx.clone(), None if dxb is None else dxb.clone()
    want, want_pg = reference_backward(dx, plan)
    (gx, gxb), pg = bufs_backward([_P(p) for p in plan], dx, dxb, keep_input)
    assert torch.equal(gx, want)
    assert (gxb is None) == (dxb is None)
    if gxb is not None:
        assert gxb.dtype == torch.bfloat16 and torch.equal(gxb.float(), want)
    assert set(pg) == set(want_pg)
    for k, t in want_pg.items():
        assert torch.equal(pg[k], t), k
    if keep_input:
        assert torch.equal(dx, before[0])
        assert dxb is None or torch.equal(dxb, before[1])
