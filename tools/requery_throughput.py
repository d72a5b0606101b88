"""Concept re-query against the full calls it replaces, one JSON line per measurement; nothing here is a gate.

The pipeline of tools/frontend_throughput.py (real geometries, synthetic weights) at 1024 x 1024, layers 15-18, 4 steps:
  (a) ``full``:    generate_image, generate_images(batch=5), encode_images(batch=5) with 4 concepts, ms per image;
  (b) ``tracing``: the same calls with keep_trace=True (every step / noise sample traced), and the bytes a trace holds;
  (c) ``requery``: pipe.requery on the traces of (b) with C' = 4 and 21 new words, 1 and 5 images per call, ms per image --
      for a generate trace (4 traced steps) and an encode trace (1 noise sample);
  (d) ``split``:   one re-query step (B = 1, C' = 4) with HIP events around every GEMM and attention launch (ops hooks):
      where the device time of a step goes.  The events serialise nothing (one stream), but the hooks add host time, so
      the total of (c) is the figure to quote.
A host clock between two device synchronises, one warm-up, the median of three.  On a commit without ``requery`` only (a)
is taken: that is how a commit is measured against its parent in one job.
    python tools/requery_throughput.py
"""
import inspect
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_ITEMS, SIDE = 5, 1024
WORDS = ["cat", "dog", "sheep", "bus", "car", "bird"]
NEW = {4: ["tree", "sky", "road", "grass"],
       21: ["tree", "sky", "road", "grass"] + [f"thing {i}" for i in range(17)]}


def main():
    import numpy as np
    import PIL.Image
    import torch
    from frontend_throughput import build_pipeline
    from conceptattention_amd import ops
    pipe = build_pipeline()
    images = [PIL.Image.fromarray(np.random.default_rng(i).integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8))
              for i in range(N_ITEMS)]
    prompts = [f"a {WORDS[i]} and a {WORDS[i + 1]}" for i in range(N_ITEMS)]
    concepts = WORDS[:4]
    raw = dict(return_pil_heatmaps=False)

    def med(fn, per=1):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(sorted(ms)[1] / per, 2)

    def calls(**kw):
        return {"generate_image_ms": med(lambda: pipe.generate_image(prompts[0], concepts, **raw, **kw)),
                "generate_images_b5_ms_per_image": med(lambda: pipe.generate_images(prompts, concepts, batch=N_ITEMS, **raw,
                                                                                    **kw), N_ITEMS),
                "encode_images_b5_ms_per_image": med(lambda: pipe.encode_images(images, concepts, prompts, batch=N_ITEMS,
                                                                                **raw, **kw), N_ITEMS)}
    print(json.dumps({"route": "full", **calls()}), flush=True)
    if "keep_trace" not in inspect.signature(pipe.generate_image).parameters:
        return
    print(json.dumps({"route": "tracing", **calls(keep_trace=True)}), flush=True)
    gen = pipe.generate_images(prompts, concepts, batch=N_ITEMS, keep_trace=True, **raw)
    enc = pipe.encode_images(images, concepts, prompts, batch=N_ITEMS, keep_trace=True, **raw)
    torch.cuda.synchronize()
    print(json.dumps({"route": "trace_bytes", "generate_trace_GB_per_image": round(gen[0].trace.nbytes / 1e9, 3),
                      "encode_trace_GB_per_image": round(enc[0].trace.nbytes / 1e9, 3),
                      "allocated_GB": round(torch.cuda.memory_allocated() / 1e9, 1)}), flush=True)
    for name, outs in (("generate", gen), ("encode", enc)):
        traces = [o.trace for o in outs]
        for C, words in NEW.items():
            pipe.requery(traces, words, **raw)        # (the words' embeddings are cached from here on)
            print(json.dumps({"route": "requery", "trace": name, "steps": len(traces[0].timesteps), "concepts": C,
                              "b1_ms_per_image": med(lambda: pipe.requery(traces[0], words, **raw)),
                              "b5_ms_per_image": med(lambda: pipe.requery(traces, words, **raw), N_ITEMS)}), flush=True)
    # (d) the device time of one step, by launch kind
    spans = []

    def timed(kind):
        def hook(arr, _, launch):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            spans.append((kind, a, b))
        return hook
    step = gen[0].trace.timesteps[:1]
    pipe.requery(gen[0].trace, NEW[4], timesteps=step, **raw)
    torch.cuda.synchronize()
    ops.set_gemm_hook(timed("gemm"))
    ops.set_attn_hook(timed("attention"))
    try:
        t0 = time.perf_counter()
        pipe.requery(gen[0].trace, NEW[4], timesteps=step, **raw)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
    finally:
        ops.set_gemm_hook(None)
        ops.set_attn_hook(None)
    line = {"route": "split", "step_total_ms_with_hooks": round(total, 2)}
    for kind in ("gemm", "attention"):
        us = [a.elapsed_time(b) * 1e3 for k, a, b in spans if k == kind]
        line[kind] = {"launches": len(us), "ms": round(sum(us) / 1e3, 3)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
