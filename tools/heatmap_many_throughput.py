"""Heat maps for more than 8 concepts: the three-launch form against ca_heatmap_many, kernel and pipeline.

``kernel``: the real geometry of one captured layer of a 5-item forward: L = 4096 patches, dim 3072, 5 items x 2 spaces =
10 problems, fp32 image and concept vectors (the rows the model hands over beyond 8 concepts), every problem with its
running accumulator and its per-layer table row.  C = 8, 9, 12, 16, 21, 32.  Per C:
  * ``three_launch``: per problem ops.heatmap_logits (ceil(C / 4) launches, each a pass over the image rows) and two
    weighting launches (ops.heatmap_norm_accumulate);
  * ``many``: one ops.heatmap_many;
  * ``fused`` (C = 8 only, for scale): one ops.heatmap_fused.
HIP events around the calls, 3 warm-ups, the median of 20; bytes moved (counted from the launches: every read and write
of vectors, logits and accumulators) and GB/s.  Softmax; ``--norm sparsemax`` times the sparse weighting instead.

``loop``: the pipeline of tools/frontend_throughput.py (real geometries, synthetic weights) at C = 12 and C = 21:
``generate_images(batch=5)`` and ``encode_images(batch=5)`` of 5 items, per image, and one ``layer_noise_sweep`` of 5 noise
levels over all 19 layers of one image, per level; a host clock around each call, which ends in a device synchronise, one
warm-up and the median of three.

The tool runs on a commit without ca_heatmap_many as well: it then times the three-launch route only (``many`` absent
from the lines), which is how a commit is measured against its parent in one job.  One JSON line per measurement; nothing
here is a gate.
    python tools/heatmap_many_throughput.py            # both steps, each a process of its own under a time limit
    python tools/heatmap_many_throughput.py kernel     # one step: kernel | loop
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

L_IMG, DIM, N_ITEMS = 4096, 3072, 5
CONCEPTS = (8, 9, 12, 16, 21, 32)
WORDS = ["cat", "dog", "sheep", "bus", "car", "bird", "boat", "cow", "person", "train", "sofa", "chair", "horse", "tree",
         "sky", "grass", "floor", "road", "wall", "lamp", "cup"]


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


def kernel(norm_name="softmax"):
    import torch
    from conceptattention_amd import _lib as L
    from conceptattention_amd import ops
    norm = L.NORMS[norm_name]
    n = 2 * N_ITEMS
    g = torch.Generator().manual_seed(0)
    img = [torch.randn(L_IMG, DIM, generator=g).to("cuda") for _ in range(n)]
    has_many = hasattr(ops, "heatmap_many")
    accumulate = getattr(ops, "heatmap_norm_accumulate", ops.heatmap_softmax_accumulate)   # (sparse norms up to 32 | 16)
    for C in CONCEPTS:
        if norm != L.NORM_SOFTMAX and C > 16 and not has_many:
            continue                                       # (the sparse norms stop at 16 concepts there)
        con = [(torch.randn(C, DIM, generator=g) * 1.5 / DIM ** 0.5).to("cuda") for _ in range(n)]
        acc = [torch.zeros(C, L_IMG, device="cuda") for _ in range(n)]
        tab = [torch.zeros(C, L_IMG, device="cuda") for _ in range(n)]
        logits = torch.empty(C, L_IMG, device="cuda")
        probs = [ops.Heatmap(img[i], con[i], acc[i], 0.25, tab[i], 1.0) for i in range(n)]

        def three_launch():
            for i in range(n):
                ops.heatmap_logits(img[i], con[i], logits)
                accumulate(logits, acc[i], 0.25, norm)
                accumulate(logits, tab[i], 1.0, norm)
        vec, plane = L_IMG * DIM * 4, C * L_IMG * 4
        passes = -(-C // 4)
        moved = {"three_launch": n * (passes * (vec + 4 * DIM * 4) + plane + 2 * 3 * plane),
                 "many": n * (vec + C * DIM * 4 + 2 * 2 * plane)}
        moved["fused"] = moved["many"]
        line = {"C": C, "norm": norm_name, "problems": n, "L": L_IMG, "dim": DIM,
                "launches": {"three_launch": n * (passes + 2), "many": 1}}
        routes = [("three_launch", three_launch)]
        if has_many:
            routes.append(("many", lambda: ops.heatmap_many(probs, norm)))
        if C <= 8:
            routes.append(("fused", lambda: ops.heatmap_fused(probs, norm)))
        for name, fn in routes:
            us = _median_us(fn, torch)
            line[name] = {"us": us, "MB": round(moved[name] / 1e6, 1), "GB_per_s": round(moved[name] / us / 1e3, 1)}
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

    def med(fn, per):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(sorted(ms)[1] / per, 2)
    for C in (12, 21):
        concepts = WORDS[:C]
        line = {"C": C, "route": "heatmap_many" if hasattr(ops, "heatmap_many") else "three_launch"}
        line["generate_images_ms_per_image"] = med(lambda: pipe.generate_images(
            prompts, concepts, batch=N_ITEMS, return_pil_heatmaps=False), N_ITEMS)
        line["encode_images_ms_per_image"] = med(lambda: pipe.encode_images(
            images, concepts, prompts, batch=N_ITEMS, return_pil_heatmaps=False), N_ITEMS)
        line["layer_noise_sweep_ms_per_level"] = med(lambda: pipe.layer_noise_sweep(
            images[0], concepts, prompts[0], noise_levels=[10, 20, 30, 40, 45], num_steps=50, batch=N_ITEMS), 5)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    norm = sys.argv[sys.argv.index("--norm") + 1] if "--norm" in sys.argv else "softmax"
    args = [a for a in args if a != norm]
    if args == ["kernel"]:
        kernel(norm)
    elif args == ["loop"]:
        loop()
    else:
        for step, limit in (("kernel", 300), ("loop", 840)):
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step,
                                 "--norm", norm]).returncode
            if rc:
                sys.exit(rc)
