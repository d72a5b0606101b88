"""Per-head concept maps (ca_head_maps): kernel and pipeline, one JSON line per measurement; nothing here is a gate.

``kernel``: one captured layer at the real geometry: L = 4096 image rows, hidden 3072 = 24 heads, 5 items x the three
spaces = 15 problems in ONE launch (fp32 rows for "output" and "cross", the bf16 v third of a [C + L, 3 x 3072] buffer for
"value"), C = 4 / 12 / 32 concepts, each norm, every problem with its head-resolved tensor and its mean.  HIP events around
the calls, 3 warm-ups, the median of 20.  MB read (every image and concept row once) and written (the two outputs, read
and written), and GB/s on their sum.  Beside ``head_maps``:
  * ``torch``: what a user would otherwise write on the device: reshape to heads, einsum, the norm over the concepts
    (softmax; the sparse norms have no torch form and are left out), the mean over the heads, added to both outputs;
  * ``heatmap_many``: ops.heatmap_many on the same rows (full-width logits, its own norms): the floor of one pass over
    them.

``loop``: the pipeline of tools/frontend_throughput.py (real geometries, synthetic weights) at 1024 x 1024, layers 15-18:
``generate_images(batch=5)`` and ``encode_images(batch=5)`` with and without ``head_maps=("output", "cross", "value")``, ms
per image; a host clock around each call, which ends in a device synchronise, one warm-up and the median of three.  On a
commit without ``ops.head_maps`` only the without-figures are taken: that is how a commit is measured against its parent
in one job.
    python tools/head_maps_throughput.py            # both steps, each a process of its own under a time limit
    python tools/head_maps_throughput.py kernel     # one step: kernel | loop
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
SPACES = ("output", "cross", "value")


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
    from conceptattention_amd import _lib as L
    from conceptattention_amd import ops
    W = HEADS * 128
    g = torch.Generator().manual_seed(0)
    norms = {"none": getattr(L, "NORM_NONE", None), **L.NORMS}
    for C in (4, 12, 32):
        rows = []   # per item and space: (image rows, concept rows)
        for _ in range(N_ITEMS):
            qkv = (torch.randn(C + L_IMG, 3 * W, generator=g) * 0.1).to("cuda", torch.bfloat16)
            for space in SPACES:
                if space == "value":
                    rows.append((qkv[C:, 2 * W:], qkv[:C, 2 * W:]))
                else:
                    x = (torch.randn(C + L_IMG, W, generator=g) * 0.1).to("cuda")
                    rows.append((x[C:], x[:C]))
        n = len(rows)
        heads = [torch.zeros(HEADS, C, L_IMG, device="cuda") for _ in range(n)]
        acc = [torch.zeros(C, L_IMG, device="cuda") for _ in range(n)]
        read = sum((i.shape[0] + c.shape[0]) * W * i.element_size() for i, c in rows)
        for name, norm in norms.items():
            line = {"L": L_IMG, "heads": HEADS, "C": C, "problems": n, "norm": name, "MB_read": round(read / 1e6, 1)}
            routes = []
            if hasattr(ops, "head_maps"):
                probs = [ops.HeadMaps(i, c, heads=heads[k], weight_h=0.25, acc=acc[k], weight=0.25)
                         for k, (i, c) in enumerate(rows)]
                routes.append(("head_maps", lambda: ops.head_maps(probs, HEADS, norm),
                               2 * sum(h.numel() + a.numel() for h, a in zip(heads, acc)) * 4))

            def torch_route():
                for k, (i, c) in enumerate(rows):
                    z = torch.einsum("chd,phd->hcp", c.float().view(C, HEADS, 128), i.float().view(L_IMG, HEADS, 128))
                    w = torch.softmax(z, 1) if name == "softmax" else z
                    heads[k].add_(w, alpha=0.25)
                    acc[k].add_(w.mean(0), alpha=0.25)
            if name in ("none", "softmax"):
                routes.append(("torch", torch_route, 2 * sum(h.numel() + a.numel() for h, a in zip(heads, acc)) * 4))
            if name != "none":
                many = [ops.Heatmap(i, c if c.dtype == torch.float32 or i.dtype != torch.float32 else c.float(), acc=acc[k],
                                    weight=0.25) for k, (i, c) in enumerate(rows)]
                routes.append(("heatmap_many", lambda: ops.heatmap_many(many, L.NORMS[name]),
                               2 * sum(a.numel() for a in acc) * 4))
            for route, fn, written in routes:
                us = _median_us(fn, torch)
                line[route] = {"us": us, "MB_written": round(written / 1e6, 1),
                               "GB_per_s": round((read + written) / us / 1e3, 1)}
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
    modes = [("without", {})] + ([("head_maps", {"head_maps": SPACES})] if hasattr(ops, "head_maps") else [])
    for name, kw in modes:
        line = {"route": name}
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
