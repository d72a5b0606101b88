"""Time per image of scoring a per-layer x per-noise-level sweep, three routes over the same device tables.

1024 x 1024 image, 4 concepts, 50 noise levels x 19 layers, both spaces, labels at 224 x 224, the pipeline of
tools/frontend_throughput.py (real geometries, synthetic weights).  The routes:

* ``host``:      ``layer_noise_sweep``, both tables to the host, then per map the mean-threshold mask,
                 ``prepare_for_scoring`` and ``SweepScores.update`` -- what a user of the sweep had to do;
* ``device``:    ``ConceptAttentionSegmentationModel.score_sweep`` with a ``DeviceSweepScores`` and its ``result()`` (one
                 ``ops.segtab_score`` call per space, one download of the records);
* ``seg_score``: the same device tables through ``ops.seg_score`` in launches of 16, then the one download: the route that
                 needs no new kernel, the yardstick for ``ops.segtab_score``.

One warm-up call, then the median of three (SWEEP_REPEATS), per image: ``wall_ms`` is a host clock around the whole call,
ending in a device synchronise; ``score_ms`` the part after the tables exist (bracketed by device synchronises).  ``kernel``
times the scoring launches alone by HIP events (median of 20 after 3): one ``ops.segtab_score`` call on 950 maps of 64 x 64
inside a [950, 4, 64, 64] table, and the 60 ``ops.seg_score`` launches for the same maps.  One JSON line per measurement;
nothing here is a gate.
    python tools/sweep_score_throughput.py            # both steps, each a process of its own under a time limit
    python tools/sweep_score_throughput.py kernel     # one step: kernel | routes
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIDE, SIZE, LEVELS, NUM_STEPS, WARMUP = 1024, 224, 50, 50, 1
REPEATS = int(os.environ.get("SWEEP_REPEATS", 3))
CONCEPTS = ["object", "background", "grass", "sky"]


def _label():
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(100)
    return (torch.nn.functional.interpolate(torch.rand(1, 1, 7, 7, generator=g), size=(SIZE, SIZE))[0, 0] > 0.5) \
        .numpy().astype(np.uint8)


def _median(v):
    return round(sorted(v)[len(v) // 2], 3)


def _seg_score_table(ops, table, target, label, records):
    """Every [h, w] plane ``target`` of a [M, C, h, w] table through ops.seg_score (launches of 16 inside)."""
    ops.seg_score([table[m, target] for m in range(table.shape[0])], [label] * table.shape[0], records)


def kernel():
    import torch
    from conceptattention_amd import ops
    M = 950
    table = torch.rand(M, 4, 64, 64, device="cuda") ** 2
    label = torch.from_numpy(_label()).to("cuda")
    rec = torch.zeros(M, ops.SEG_RECORD_BYTES, dtype=torch.uint8, device="cuda")
    cells = ops.segtab_cells(64, 64, "cuda")

    def med(fn):
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
        return round(sorted(ms)[10], 3)
    line = {"call": "950 maps of 64 x 64 (plane 0 of 4) against one 224 x 224 label",
            "segtab_score_ms": med(lambda: ops.segtab_score(table, 0, label, rec, cells)),
            "segtab_score_raw_blur_downscale_ms": med(lambda: ops.segtab_score(
                table, 0, label, rec, cells, downscale_for_eval=True, blur_weights=ops.seg_blur_weights(), normalize=False)),
            "seg_score_60_launches_ms": med(lambda: _seg_score_table(ops, table, 0, label, rec))}
    print(json.dumps(line), flush=True)


def routes():
    import numpy as np
    import PIL.Image
    import torch
    from frontend_throughput import build_pipeline
    from conceptattention_amd import ops
    from conceptattention_amd import segmentation as S
    pipe = build_pipeline()
    seg = S.ConceptAttentionSegmentationModel(pipe)
    depth = pipe.params.depth
    image = PIL.Image.fromarray(np.random.default_rng(0).integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8))
    prompt = "a photo of an object"
    vae_noise = torch.randn(1, 16, SIDE // 8, SIDE // 8, generator=torch.Generator().manual_seed(30))
    label = _label()
    levels = list(range(LEVELS))
    kw = dict(num_steps=NUM_STEPS, width=SIDE, height=SIDE, batch=5)
    clock = {"score": 0.0}
    sweep = pipe.layer_noise_sweep

    def tables():
        t = sweep(image, CONCEPTS, prompt, levels, vae_noise=vae_noise, **kw)
        torch.cuda.synchronize()
        clock["t"] = time.perf_counter()
        return t

    def done():
        torch.cuda.synchronize()
        clock["score"] = (time.perf_counter() - clock["t"]) * 1e3

    def host():
        scores = S.SweepScores(LEVELS, depth)
        for space, table in zip(S.SWEEP_SPACES, tables()):
            planes = table[:, :, 0].cpu()
            for lv in range(LEVELS):
                for col in range(depth):
                    x = planes[lv, col]
                    c, m = S.prepare_for_scoring(x.numpy(), (x > x.mean()).numpy(), size=SIZE)
                    scores.update(space, lv, col, m, c, label.astype(bool))
        done()
        return scores.result("output")

    def device():
        dev = S.DeviceSweepScores(LEVELS, depth, "cuda:0")
        pipe.layer_noise_sweep = lambda *a, **k: tables()       # (the same call, with the clock behind it)
        try:
            seg.score_sweep([image], ["object"], CONCEPTS, [prompt], [label], dev, levels, size=SIZE, vae_noise=[vae_noise], **kw)
        finally:
            del pipe.layer_noise_sweep
        out = dev.result("output")
        done()
        return out

    def seg_score():
        dev = S.DeviceSweepScores(LEVELS, depth, "cuda:0")
        y = torch.from_numpy(label).to("cuda:0")
        for space, table in zip(S.SWEEP_SPACES, tables()):
            _seg_score_table(ops, table.reshape(-1, *table.shape[2:]), 0, y, dev.reserve(space, SIZE * SIZE))
        out = dev.result("output")
        done()
        return out

    results = {}
    with torch.no_grad():
        for name, fn in (("device", device), ("seg_score", seg_score), ("host", host)):
            for _ in range(WARMUP):
                results[name] = fn()
            wall, score = [], []
            for _ in range(REPEATS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                score.append(clock["score"])
            print(json.dumps({"route": name, "per_image": {"wall_ms": _median(wall), "score_ms": _median(score)},
                              "maps": 2 * LEVELS * depth, "repeats": REPEATS}), flush=True)
    diff = {n: max(float(np.abs(results[n][k] - results["device"][k]).max()) for k in ("pixAcc", "mIoU", "mAP"))
            for n in ("host", "seg_score")}
    print(json.dumps({"largest difference of pixAcc / mIoU / mAP from the device route": diff}), flush=True)


if __name__ == "__main__":
    steps = {"kernel": kernel, "routes": routes}
    if len(sys.argv) == 2:
        steps[sys.argv[1]]()
    else:
        for what in steps:
            rc = subprocess.call(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), what])
            if rc != 0:
                sys.exit(f"step {what} ended with {rc}")   # nothing more is started on the GPU
