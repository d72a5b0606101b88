"""Propagated maps (ca_propagate_maps): kernel and pipeline, one JSON line per measurement; nothing here is a gate.

``kernel``: ``--layers`` captured layers at the real geometry: L = 4096 image rows as queries and as keys (n0 = 0),
``--heads`` heads (24: hidden 3072), q and k as column slices of a [rows, 3 x heads x 128] buffer per item (the model's
QKV), C = 4 / 12 / 32 map rows, 1 item and 5 items per launch.  HIP events around the calls, 3 warm-ups, the median of 20.
GFLOP of the QK^T pass (2 L L 128 heads) and of P.V at C padded to 16 or 32, and TFLOP/s on their sum.  Beside
``propagate_maps``:
  * ``torch``: what a user would otherwise write on the device: per head softmax(q k^T) @ v^T, the mean over the heads,
    added to the accumulator (the L x L matrix of every head is materialised);
  * ``attention``: ops.attention on the same rows (the keys as values): the floor of one flash pass with a bf16 P.V.
On a commit without ``ops.propagate_maps`` only the other two are taken: that is how a commit is measured against its
parent in one job (their columns then show the box).

``loop``: the pipeline of tools/frontend_throughput.py (real geometries, synthetic weights) at 1024 x 1024, layers 15-18:
``generate_images(batch=5)`` and ``encode_images(batch=5)`` with and without ``propagate=("output", "cross")``, ms per
image; a host clock around each call, which ends in a device synchronise, one warm-up and the median of three.

``--parent DIR``: a built checkout of the parent commit: its ``loop`` and ``python bench.py --gpus 1 --steps 4 --warmup 2``
run in the same job, after this tree's, each a process of its own under a time limit.
    python tools/propagate_throughput.py                      # kernel, loop and bench.py, each a process of its own
    python tools/propagate_throughput.py kernel --heads 24 --layers 1
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

# (CA_TREE: the tree whose package and tools are measured -- how ``--parent`` runs this file over the parent's checkout)
ROOT = os.environ.get("CA_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

L_IMG = 4096
WORDS = ["cat", "dog", "sheep", "bus", "car", "bird"]
CONCEPTS = (4, 12, 32)


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


def kernel(heads: int, layers: int):
    import torch
    from conceptattention_amd import ops
    W = heads * 128
    g = torch.Generator().manual_seed(0)
    scale_log2 = 1.4426950408889634 / math.sqrt(128.0)
    for C in CONCEPTS:
        for items in (1, 5):
            bufs = [(torch.randn(L_IMG, 3 * W, generator=g)).to("cuda", torch.bfloat16) for _ in range(items)]
            rows = [(b[:, :W], b[:, W:2 * W]) for b in bufs]                         # q, image keys
            v = [torch.softmax(torch.randn(C, L_IMG, generator=g), 0).to("cuda") for _ in range(items)]
            acc = [torch.zeros(C, L_IMG, device="cuda") for _ in range(items)]
            qk = items * 2.0 * L_IMG * L_IMG * 128 * heads
            pv = items * 2.0 * L_IMG * L_IMG * (16 if C <= 16 else 32) * heads
            line = {"C": C, "L": L_IMG, "heads": heads, "items": items, "layers": layers,
                    "GFLOP_qk": round(layers * qk / 1e9, 1), "GFLOP_pv_fp32": round(layers * pv / 1e9, 1)}
            routes = []
            if hasattr(ops, "propagate_maps"):
                probs = [ops.PropagateMaps(q, None, k, v[i], acc=acc[i], weight=0.25) for i, (q, k) in enumerate(rows)]
                ws = torch.empty(ops.propagate_maps_workspace_bytes(probs, heads), dtype=torch.uint8, device="cuda")
                line["workspace_MB"] = round(ws.numel() / 1e6, 1)

                def prop_route():
                    for _ in range(layers):
                        ops.propagate_maps(probs, heads, scale_log2, workspace=ws)
                routes.append(("propagate_maps", prop_route))

            def torch_route():
                for _ in range(layers):
                    for i, (q, k) in enumerate(rows):
                        qh = q.float().view(L_IMG, heads, 128).permute(1, 0, 2)
                        kh = k.float().view(L_IMG, heads, 128).permute(1, 2, 0)
                        p = torch.softmax((qh @ kh) * (scale_log2 / 1.4426950408889634), -1)
                        acc[i].add_((p @ v[i].T).mean(0).T, alpha=0.25)
            routes.append(("torch", torch_route))
            out = [torch.empty(L_IMG, W, device="cuda", dtype=torch.bfloat16) for _ in range(items)]
            attn = [ops.Attn(q, out[i], k, k) for i, (q, k) in enumerate(rows)]

            def attn_route():
                for _ in range(layers):
                    ops.attention(attn, heads)
            routes.append(("attention", attn_route))
            for route, fn in routes:
                us = _median_us(fn, torch)
                line[route] = {"us": us, "TFLOP_per_s": round(layers * (qk + (pv if route == "propagate_maps" else 0)) / us / 1e6, 1)}
            print(json.dumps(line), flush=True)


def loop():
    import numpy as np
    import PIL.Image
    import torch
    from frontend_throughput import build_pipeline
    from conceptattention_amd import ops
    pipe = build_pipeline()
    side, n = 1024, 5
    images = [PIL.Image.fromarray(np.random.default_rng(i).integers(0, 256, (side, side, 3), dtype=np.uint8)) for i in range(n)]
    prompts = [f"a {WORDS[i]} and a {WORDS[i + 1]}" for i in range(n)]
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
        return round(sorted(ms)[1] / n, 2)
    modes = [("without", {})]
    if hasattr(ops, "propagate_maps"):
        modes.append(("propagate", {"propagate": ("output", "cross")}))
        modes.append(("propagate_2_steps", {"propagate": ("output", "cross"), "propagate_steps": 2}))
    for name, kw in modes:
        line = {"route": name, "tree": ROOT}
        line["generate_images_ms_per_image"] = med(lambda: pipe.generate_images(
            prompts, concepts, batch=n, return_pil_heatmaps=False, **kw))
        line["encode_images_ms_per_image"] = med(lambda: pipe.encode_images(
            images, concepts, prompts, batch=n, return_pil_heatmaps=False, **kw))
        print(json.dumps(line), flush=True)


def _child(cmd, limit, tree) -> int:
    return subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=tree, env=dict(os.environ, CA_TREE=tree)).returncode


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", choices=("kernel", "loop"))
    ap.add_argument("--heads", type=int, default=24)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, measured in the same job")
    a = ap.parse_args()
    if a.step == "kernel":
        kernel(a.heads, a.layers)
    elif a.step == "loop":
        loop()
    else:
        me = os.path.abspath(__file__)
        bench = [sys.executable, "bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"]
        steps = [([sys.executable, me, "kernel", "--heads", str(a.heads), "--layers", str(a.layers)], 300, ROOT),
                 ([sys.executable, me, "loop"], 600, ROOT), (bench, 600, ROOT)]
        if a.parent:   # (a tree without ops.propagate_maps takes the other routes only)
            parent = os.path.abspath(a.parent)
            steps += [([sys.executable, me, "loop"], 600, parent), (bench, 600, parent)]
        for cmd, limit, tree in steps:
            rc = _child(cmd, limit, tree)
            if rc:
                sys.exit(rc)
