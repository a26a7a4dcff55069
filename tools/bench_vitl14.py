"""ViT-L/14 adapter step throughput on one MI355X: the reference adapter script's model and batch
(scripts/adapter_clip.sh:30: MODEL_NAME="ViT-L-14", batch 64), AdapterCLIP("ViT-L/14", "adapter",
"both"), C = 10 prompts, one full online step (transform-free: synthetic normalised 224 x 224
inputs; forward, CE on probs, backward, AdamW), random-init weights. 257 image tokens: patch-14
embedding at K = 640, the long attention family, the width-1024 general routes, the last block on
every row. Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lifelong-clip_amd")]
import torch  # noqa: E402

B = int(os.environ.get("B", 64))
C = int(os.environ.get("C", 10))
STEPS = int(os.environ.get("STEPS", 5))
WARM = int(os.environ.get("WARM", 2))


def main():
    from lcclip import AdapterCLIP, OnlineTrainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    w = AdapterCLIP("ViT-L/14", "adapter", "both", device=dev)
    tr = OnlineTrainer(w)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, 3, 224, 224, device=dev, generator=g)
    tok = torch.zeros(C, 77, dtype=torch.long, device=dev)
    tok[:, 0] = 49406
    tok[:, 1:9] = torch.randint(256, 49405, (C, 8), device=dev, generator=g)
    tok[:, 9] = 49407
    y = torch.randint(0, C, (B,), device=dev, generator=g)
    for _ in range(WARM):
        loss, _ = tr.step(x, y, tok)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        loss, _ = tr.step(x, y, tok)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / STEPS
    print(json.dumps({"workload": "adapter_clip ViT-L/14 online step (adapter on both towers)",
                      "per_gpu_batch": B, "classes": C, "image_tokens": 257,
                      "ms_per_step": round(dt * 1e3, 3), "images_per_s": round(B / dt, 1),
                      "loss": round(float(loss), 5), "dtype": "bf16 image / fp16 text",
                      "data": "synthetic"}), flush=True)


if __name__ == "__main__":
    main()
