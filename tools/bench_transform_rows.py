"""Patch-14 train transform microbenchmark (dev tool): n = 64 CIFAR-shaped images -> 224, patch
14 (the reference adapter script's batch), into conv1's bf16 rows [64 * 256, 640]:

  (a) rows   lc_train_transform_rows, one launch;
  (b) pair   lc_train_transform layout 0 (f32 NCHW batch) + lc_patchify_pad at ldo = 640, what a
             ViT-L/14 loop needed before the rows entry existed.

Both in one process on preallocated buffers, after warm-up, --reps (5) interleaved repetitions
a, b, a, b, ... Each repetition is timed two ways with HIP events on the stream:
  graph   --iters calls captured once into a HIP graph and replayed: device time per call, free
          of the host's launch cost (a call here is ~10 us of kernel, the size of one ctypes
          launch);
  eager   --iters calls issued from Python: what a loop that launches them one by one waits for.
Prints one JSON line per repetition and a summary line: the medians, each side's spread
(max - min over the repetitions) and whether (a) beats (b) by more than the larger spread.
Outputs are compared bit for bit before anything is timed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lifelong-clip_amd")]
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transform_rows needs the GPU (no CPU timing)")
    from lcclip import ops
    from lcclip.transforms import TrainTransform, patch_row_width
    dev = torch.device("cuda:0")
    n, R, P = args.n, 224, 14
    g = R // P
    ldo = patch_row_width(P)
    gen = torch.Generator().manual_seed(0)
    x = (torch.randint(0, 256, (n, 3, 32, 32), generator=gen).float() / 255).to(dev)
    tf = TrainTransform.for_dataset("cifar100", patch=P)
    prm = (4, 4, True)
    rows_a = torch.empty(n * g * g, ldo, dtype=torch.bfloat16, device=dev)
    rows_b = torch.empty_like(rows_a)
    img = torch.empty(n, 3, R, R, dtype=torch.float32, device=dev)

    def a():
        tf(x, params=prm, layout="patches", out=rows_a)

    def b():
        tf(x, params=prm, layout="nchw", out=img)
        ops.patchify_pad(img, P, rows_b)

    for _ in range(20):  # warm-up: code objects, clocks
        a()
        b()
    torch.cuda.synchronize()
    if not torch.equal(rows_a, rows_b):
        raise SystemExit("the two forms disagree: nothing timed")

    def graph_of(fn):
        gr = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            fn()
            with torch.cuda.graph(gr, stream=s):
                for _ in range(args.iters):
                    fn()
        torch.cuda.current_stream(dev).wait_stream(s)
        gr.replay()
        torch.cuda.synchronize()
        return gr

    def timed(run):
        st = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        run()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters * 1e3  # us per call

    def eager(fn):
        def run():
            for _ in range(args.iters):
                fn()
        return run

    ga, gb = graph_of(a), graph_of(b)
    lines = []
    for r in range(args.reps):
        rec = {"rep": r,
               "rows_graph_us": round(timed(ga.replay), 2), "pair_graph_us": round(timed(gb.replay), 2),
               "rows_eager_us": round(timed(eager(a)), 2), "pair_eager_us": round(timed(eager(b)), 2)}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    out_bytes = rows_a.numel() * 2
    summary = {"n": n, "iters": args.iters, "reps": args.reps, "rows_bytes_written": out_bytes,
               "pair_bytes_moved": img.numel() * 4 * 2 + out_bytes}
    for mode in ("graph", "eager"):
        ta = [l[f"rows_{mode}_us"] for l in lines]
        tb = [l[f"pair_{mode}_us"] for l in lines]
        spread = max(max(ta) - min(ta), max(tb) - min(tb))
        summary[mode] = {"rows_median_us": statistics.median(ta), "rows_spread_us": round(max(ta) - min(ta), 2),
                         "pair_median_us": statistics.median(tb), "pair_spread_us": round(max(tb) - min(tb), 2),
                         "rows_faster_in_every_rep": all(p > q for p, q in zip(tb, ta)),
                         "rows_faster_beyond_spread": statistics.median(tb) - statistics.median(ta) > spread}
    summary["rows_GBps_graph"] = round(out_bytes / (summary["graph"]["rows_median_us"] * 1e-6) / 1e9, 1)
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for l in lines + [summary]:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
