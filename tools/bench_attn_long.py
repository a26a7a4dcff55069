"""Attention fwd/bwd microbenchmark of the long kernel family (257..512 tokens) at ViT-L/14's
shape (dev tool; sibling of bench_attn.py). n = 64 sequences, H = 16, bf16, not causal:

  L = 257, 512   the long family (lc_attn_long_fwd / lc_attn_long_bwd through ops.attn_*)
  L = 256        the one-wave-per-chunk kernels at the nearest length they run (yardstick)
  L = 257        torch.nn.functional.scaled_dot_product_attention forward + backward (yardstick)

One line per launch: average us over REPS launches after one warm-up, and algorithmic TFLOP/s
(unpadded L: fwd 2 matmuls, bwd 5 matmuls of L x L x 64 per (sequence, head))."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lifelong-clip_amd")]
import torch  # noqa: E402

from lcclip import ops  # noqa: E402

REPS = int(os.environ.get("REPS", 20))
N = int(os.environ.get("N", 64))
H = 16
dev = torch.device("cuda:0")


def timed(f):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def report(name, tag, L, ms, matmuls):
    flops = matmuls * 2.0 * N * H * L * L * 64
    print(f"{name:6s} {tag:7s} n={N} L={L} H={H}: {ms * 1e3:8.1f} us  {flops / ms / 1e9:7.1f} TFLOP/s",
          flush=True)


def run(name, L):
    D = H * 64
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(N * L, 3 * D, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    O = torch.empty(N * L, D, device=dev, dtype=torch.bfloat16)
    dO = (torch.randn(N * L, D, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    lse = torch.empty(N * H, L, device=dev)
    dqkv = torch.empty_like(qkv)
    report(name, "fwd", L, timed(lambda: ops.attn_fwd(qkv, O, lse, N, L, H, False)), 2)
    report(name, "bwd", L, timed(lambda: ops.attn_bwd(qkv, O, dO, lse, dqkv, N, L, H, False)), 5)


def run_sdpa(L):
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v = ((torch.randn(N, H, L, 64, device=dev, generator=g) * 0.5).to(torch.bfloat16)
               .requires_grad_() for _ in range(3))
    dO = (torch.randn(N, H, L, 64, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    sdpa = torch.nn.functional.scaled_dot_product_attention
    with torch.no_grad():
        report("sdpa", "fwd", L, timed(lambda: sdpa(q, k, v)), 2)

    def both():
        o = sdpa(q, k, v)
        torch.autograd.grad(o, (q, k, v), dO)
    report("sdpa", "fwd+bwd", L, timed(both), 7)


run("long", 257)
run("long", 512)
run("short", 256)
run_sdpa(257)
