"""One OnlineTrainer.forward_backward with every lcclip.ops call recorded (dev tool): for
comparing two checkouts that must issue the same launches and compute the same bits.

  python tools/step_dump.py OUT [--model tiny|w768] [--method adapter|lora]
                                [--image-precision bf16|fp16]

The models of tests/test_last_rows_exact_gpu.py (the tiny golden model, or 2 layers at width 768;
4 images, dropout 0.1, the dropout seed counter at its start); the LCCLIP_* knobs come from the
environment. Writes OUT.trace.txt, one line per call through a public function of lcclip.ops —
name, tensor arguments as dtype[shape], scalar arguments, and the stream it was issued on (main:
the one current at the start; side1, side2, ...: the others in order of appearance) — and
OUT.npz: loss, probs and every trainable parameter's gradient."""
import argparse
import inspect
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lifelong-clip_amd")]
from lcclip import OnlineTrainer, engine, ops  # noqa: E402
from lcclip.adapter_clip import AdapterCLIP, set_adapter_dropout  # noqa: E402
from oracle import clip_oracle as o  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--model", default="tiny", choices=["tiny", "w768"])
ap.add_argument("--method", default="adapter", choices=["adapter", "lora"])
ap.add_argument("--image-precision", default="bf16", choices=["bf16", "fp16"])
a = ap.parse_args()

dev = torch.device("cuda:0")
if a.model == "tiny":
    d = np.load(os.path.join(ROOT, "tests", "golden", "tiny_clip.npz"))
    sd = {k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")}
    sd = {k: sd[k] for k in o.param_shapes(o.TINY, "adapter", "both")}
    if a.method == "lora":
        sd = o.synthetic_state_dict(o.TINY, "lora", "both", seed=3)
    img = o.synthetic_images(4, o.TINY.image_resolution, seed=28)
    tok = torch.from_numpy(d["tokens"])
else:
    cfg = o.ClipConfig(vision_layers=2, transformer_layers=2)
    sd = o.synthetic_state_dict(cfg, a.method, "both", seed=17)
    img, tok = o.synthetic_images(4, 224, seed=18), o.synthetic_tokens(4, 77, seed=19)
y = torch.arange(4) % tok.shape[0]

trace, streams = [], {torch.cuda.current_stream(dev).cuda_stream: "main"}


def show(v):
    if isinstance(v, torch.Tensor):
        return f"{str(v.dtype)[6:]}{list(v.shape)}"
    if isinstance(v, (list, tuple)):
        return "(" + ", ".join(show(x) for x in v) + ")"
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    return type(v).__name__


def recorded(name, fn):
    def wrapper(*args, **kw):
        sid = torch.cuda.current_stream(dev).cuda_stream
        tag = streams.setdefault(sid, f"side{len(streams)}")
        shown = [show(v) for v in args] + [f"{k}={show(v)}" for k, v in sorted(kw.items())]
        trace.append(f"{tag:6s}{name}({', '.join(shown)})")
        return fn(*args, **kw)
    return wrapper


for name, fn in inspect.getmembers(ops, inspect.isfunction):
    if fn.__module__ == ops.__name__ and not name.startswith("_"):
        setattr(ops, name, recorded(name, fn))

engine._seed_counter = itertools.count(1)
w = AdapterCLIP.from_state_dict(sd, a.method, "both", device=dev,
                                image_precision=a.image_precision)
tr = OnlineTrainer(set_adapter_dropout(w, 0.1))
loss, probs = tr.forward_backward(img.to(dev), y.to(dev), tok.to(dev))
torch.cuda.synchronize()
out = {"loss": loss, "probs": probs}
out.update({"grad/" + n: tr.grads[p] for n, p in w.model.named_parameters() if p.requires_grad})
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
np.savez(a.out + ".npz", **{k: v.detach().float().cpu().numpy() for k, v in out.items()})
with open(a.out + ".trace.txt", "w") as f:
    f.write("\n".join(trace) + "\n")
print(f"{a.out}: {len(trace)} calls, loss {loss.item():.9g}, streams {sorted(streams.values())}")
