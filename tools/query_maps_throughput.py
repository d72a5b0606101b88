"""Query-row maps (ca_query_maps): kernel and pipeline, one JSON line per measurement; nothing here is a gate.

``kernel``: ``--layers`` captured layers at the real geometry: L = 4096 image rows, T = 512 text rows, ``--heads`` heads
(24: hidden 3072), q and k as column slices of a [rows, 3 x heads x 128] buffer per item (the model's QKV), 1 item and 5
items per launch; the text rows' maps with nq = 16 and nq = 512 against [text | image], the concept rows' with nq = 4 and
nq = 32 against [concept | image].  HIP events around the calls, 3 warm-ups, the median of 20.  MB read once (every q and
key row of the problems) and the accumulators read and written, and GB/s on their sum.  Beside ``query_maps``:
  * ``torch``: what a user would otherwise write on the device: per head softmax(q k^T), the emitted slice, the mean over
    the heads, added to the accumulator;
  * ``attention``: ops.attention on the same q rows and key rows (the keys as values): the floor of one QK^T pass.
On a commit without ``ops.query_maps`` only the other two are taken: that is how a commit is measured against its parent in
one job (their columns then show the box).

``loop``: the pipeline of tools/frontend_throughput.py (real geometries, synthetic weights) at 1024 x 1024, layers 15-18:
``generate_images(batch=5)`` and ``encode_images(batch=5)`` with and without ``query_maps=("tokens", "concepts")`` (with
``token_maps=True`` in both, which "tokens" needs), ms per image; a host clock around each call, which ends in a device
synchronise, one warm-up and the median of three.
    python tools/query_maps_throughput.py                      # both steps, each a process of its own under a time limit
    python tools/query_maps_throughput.py kernel --heads 24 --layers 1
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

L_IMG, T_TXT = 4096, 512
WORDS = ["cat", "dog", "sheep", "bus", "car", "bird"]
SHAPES = (("tokens", 16), ("tokens", 512), ("concepts", 4), ("concepts", 32))


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
    for kind, nq in SHAPES:
        for items in (1, 5):
            n0 = T_TXT if kind == "tokens" else nq
            bufs = [(torch.randn(n0 + L_IMG, 3 * W, generator=g)).to("cuda", torch.bfloat16) for _ in range(items)]
            rows = [(b[:nq, :W], b[:n0, W:2 * W], b[n0:, W:2 * W]) for b in bufs]      # q, leading keys, image keys
            acc = [torch.zeros(nq, L_IMG, device="cuda") for _ in range(items)]
            read = items * (nq + n0 + L_IMG) * W * 2
            written = 2 * sum(a.numel() for a in acc) * 4
            line = {"kind": kind, "nq": nq, "n0": n0, "L": L_IMG, "heads": heads, "items": items, "layers": layers,
                    "MB_read": round(layers * read / 1e6, 1), "MB_acc": round(layers * written / 1e6, 1)}
            routes = []
            if hasattr(ops, "query_maps"):
                probs = [ops.QueryMaps(q, k0, k1, acc=acc[i], weight=0.25) for i, (q, k0, k1) in enumerate(rows)]
                ws = torch.empty(ops.query_maps_workspace_bytes(probs, heads), dtype=torch.uint8, device="cuda")

                def query_route():
                    for _ in range(layers):
                        ops.query_maps(probs, heads, scale_log2, workspace=ws)
                routes.append(("query_maps", query_route))

            def torch_route():
                for _ in range(layers):
                    for i, (q, k0, k1) in enumerate(rows):
                        qh = q.float().view(nq, heads, 128).permute(1, 0, 2)
                        kh = torch.cat([k0, k1]).float().view(n0 + L_IMG, heads, 128).permute(1, 2, 0)
                        p = torch.softmax((qh @ kh) * (scale_log2 / 1.4426950408889634), -1)
                        acc[i].add_(p[:, :, n0:].mean(0), alpha=0.25)
            routes.append(("torch", torch_route))
            out = [torch.empty(nq, W, device="cuda", dtype=torch.bfloat16) for _ in range(items)]
            attn = [ops.Attn(q, out[i], k0, k0, k1, k1) for i, (q, k0, k1) in enumerate(rows)]

            def attn_route():
                for _ in range(layers):
                    ops.attention(attn, heads)
            routes.append(("attention", attn_route))
            for route, fn in routes:
                us = _median_us(fn, torch)
                line[route] = {"us": us, "GB_per_s": round(layers * (read + (written if route != "attention" else 0)) / us / 1e3, 1)}
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
    modes = [("without", {}), ("token_maps", {"token_maps": True})]
    if hasattr(ops, "query_maps"):
        modes.append(("token_maps+query_maps", {"token_maps": True, "query_maps": ("tokens", "concepts")}))
    for name, kw in modes:
        line = {"route": name}
        line["generate_images_ms_per_image"] = med(lambda: pipe.generate_images(
            prompts, concepts, batch=n, return_pil_heatmaps=False, **kw))
        line["encode_images_ms_per_image"] = med(lambda: pipe.encode_images(
            images, concepts, prompts, batch=n, return_pil_heatmaps=False, **kw))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", choices=("kernel", "loop"))
    ap.add_argument("--heads", type=int, default=24)
    ap.add_argument("--layers", type=int, default=1)
    a = ap.parse_args()
    if a.step == "kernel":
        kernel(a.heads, a.layers)
    elif a.step == "loop":
        loop()
    else:
        for step, limit in (("kernel", 300), ("loop", 600)):
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step,
                                 "--heads", str(a.heads), "--layers", str(a.layers)]).returncode
            if rc:
                sys.exit(rc)
