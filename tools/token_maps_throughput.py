"""Prompt-token maps (ca_token_maps): kernel and pipeline, one JSON line per measurement; nothing here is a gate.

``kernel``: one captured layer at the real geometry: L = 4096 image rows, T = 256 and 512 text rows (all of them asked for),
24 heads, 1 and 5 problems, q and k as column slices of one [T + L, 3 x 3072] bf16 buffer per item, every problem with its
accumulator and its per-layer row.  HIP events around the calls, 3 warm-ups, the median of 20.  Beside ``token_maps``:
  * ``torch``: what a user would otherwise write on the device: per head softmax(q k^T) over all keys, the text columns,
    the mean over the heads (the q rows carry the scale, so exp2);
  * ``attention``: ops.attention on the same rows (image queries against [text | image] keys and values): the floor of a
    QK^T-plus-PV pass over these rows.
TFLOP/s on 2 L (T + L) 128 heads per problem (109.5 GFLOP at T = 256), the work of the pass over all keys.

``loop``: the pipeline of tools/frontend_throughput.py (real geometries, synthetic weights) at 1024 x 1024, layers 15-18:
``generate_images(batch=5)`` and ``encode_images(batch=5)`` with and without ``token_maps=True``, ms per image; a host
clock around each call, which ends in a device synchronise, one warm-up and the median of three.  On a commit without
``ops.token_maps`` only the without-figures are taken: that is how a commit is measured against its parent in one job.
    python tools/token_maps_throughput.py            # both steps, each a process of its own under a time limit
    python tools/token_maps_throughput.py kernel     # one step: kernel | loop
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

L_IMG, HEADS, N_ITEMS = 4096, 24, 5
WORDS = ["cat", "dog", "sheep", "bus", "car", "bird"]


def _median_us(fn, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(sorted(ms)[10] * 1e3, 1)


def kernel():
    import torch
    from conceptattention_amd import ops
    W = HEADS * 128
    g = torch.Generator().manual_seed(0)
    for T in (256, 512):
        # rows of unit variance, the q columns scaled as the model's (softmax_scale log2 e): logits of about 1 nat
        qkv = [torch.randn(T + L_IMG, 3 * W, generator=g).to("cuda", torch.bfloat16) for _ in range(N_ITEMS)]
        for b in qkv:
            b[:, :W] *= 1.4426950408889634 / 128 ** 0.5
        acc = [torch.zeros(T, L_IMG, device="cuda") for _ in range(N_ITEMS)]
        tab = [torch.zeros(T, L_IMG, device="cuda") for _ in range(N_ITEMS)]
        out = [torch.empty(L_IMG, W, device="cuda", dtype=torch.bfloat16) for _ in range(N_ITEMS)]
        for n in (1, N_ITEMS):
            flop = n * 2 * L_IMG * (T + L_IMG) * 128 * HEADS
            line = {"T": T, "L": L_IMG, "heads": HEADS, "problems": n, "GFLOP": round(flop / 1e9, 1)}
            routes = []
            if hasattr(ops, "token_maps"):
                probs = [ops.TokenMaps(qkv[i][T:, :W], qkv[i][:T, W:2 * W], qkv[i][T:, W:2 * W], T, acc=acc[i], weight=0.25,
                                       acc2=tab[i], weight2=1.0) for i in range(n)]
                routes.append(("token_maps", lambda: ops.token_maps(probs, HEADS, 1.0)))

            def torch_route():
                for i in range(n):
                    q = qkv[i][T:, :W].view(L_IMG, HEADS, 128).transpose(0, 1)
                    k = qkv[i][:, W:2 * W].view(T + L_IMG, HEADS, 128).transpose(0, 1)
                    total = None
                    for h in range(HEADS):                        # (per head: all heads at once are 1.7 GB of scores)
                        s = (q[h] @ k[h].T).float() * 0.6931471805599453
                        p = torch.softmax(s, -1)[:, :T]
                        total = p if total is None else total + p
                    m = (total / HEADS).T
                    acc[i].add_(m, alpha=0.25)
                    tab[i].add_(m)
            attn = [ops.Attn(qkv[i][T:, :W], out[i], qkv[i][:T, W:2 * W], qkv[i][:T, 2 * W:], qkv[i][T:, W:2 * W],
                             qkv[i][T:, 2 * W:]) for i in range(n)]
            routes += [("torch", torch_route), ("attention", lambda: ops.attention(attn, HEADS, q_prescaled=True))]
            for name, fn in routes:
                us = _median_us(fn, torch)
                line[name] = {"us": us, "TFLOP_per_s": round(flop / us / 1e6, 1)}
            print(json.dumps(line), flush=True)


def loop():
    import numpy as np
    import PIL.Image
    import torch
    from frontend_throughput import build_pipeline
    from conceptattention_amd import ops
    pipe = build_pipeline()
    side = 1024
    images = [PIL.Image.fromarray(np.random.default_rng(i).integers(0, 256, (side, side, 3), dtype=np.uint8))
              for i in range(N_ITEMS)]
    prompts = [f"a {WORDS[i]} and a {WORDS[i + 1]}" for i in range(N_ITEMS)]
    concepts = WORDS[:4]

    def med(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(sorted(ms)[1] / N_ITEMS, 2)
    modes = [("without", {})] + ([("token_maps", {"token_maps": True})] if hasattr(ops, "token_maps") else [])
    for name, kw in modes:
        line = {"route": name, "tokens": [len(p) for p in prompts] if kw else None}
        line["generate_images_ms_per_image"] = med(lambda: pipe.generate_images(
            prompts, concepts, batch=N_ITEMS, return_pil_heatmaps=False, **kw))
        line["encode_images_ms_per_image"] = med(lambda: pipe.encode_images(
            images, concepts, prompts, batch=N_ITEMS, return_pil_heatmaps=False, **kw))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args == ["kernel"]:
        kernel()
    elif args == ["loop"]:
        loop()
    else:
        for step, limit in (("kernel", 300), ("loop", 600)):
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step]).returncode
            if rc:
                sys.exit(rc)
