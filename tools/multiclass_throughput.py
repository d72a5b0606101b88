"""Time per image of the multi-class (Pascal VOC) eval loop, scores on the host against scores on the device.

1024 x 1024 images, labels at 64 x 64 (the harness's size) and at 224 x 224, the pipeline of tools/frontend_throughput.py
(real geometries, synthetic weights), 5 images per call, 5 background concepts + 3 present classes per image.  Two routes
over the same images and labels:

* ``host``:   ``segment_multiclass`` (``encode_images(batch=5)``, argmax on the downloaded maps), then per image
              ``map_predictions_to_class_indices``, the nearest resize to the label and ``MultiClassScores.update``;
* ``device``: ``ConceptAttentionSegmentationModel.score_multiclass_images`` with a ``DeviceMultiClassScores`` and its
              ``result()`` (the one download of the count rows).
Both routes get the same diffusion and autoencoder noise, so their counters must agree (the last line printed per size).

Two warm-up calls, then the median of five, per image (the call's time / 5): ``wall_ms`` is a host clock around the whole
call, which ends in a device synchronise; ``score_ms`` comes from a second set of runs in which the scoring part is
bracketed by device synchronises and a host clock (host: argmax + lookup + resize + update of the 5 images; device: the
``ops.mseg_score`` launches and ``result()``).  ``kernel`` times ``ops.mseg_score`` alone for 5 items of 8 maps of 64 x 64
by HIP events (median of 20 launches after 3).  One JSON line per measurement; nothing here is a gate.
    python tools/multiclass_throughput.py            # both steps, each a process of its own under a time limit
    python tools/multiclass_throughput.py kernel     # one step: kernel | loop
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_ITEMS, SIDE, SIZES, WARMUP, REPEATS = 5, 1024, (64, 224), 2, 5
NAMES = ["background", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable",
         "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]
BACKGROUND = ["background", "floor", "grass", "tree", "sky"]
TARGETS = [["cat", "dog", "sheep"], ["bus", "car", "person"], ["bird", "boat", "cow"], ["chair", "sofa", "tvmonitor"],
           ["horse", "person", "dog"]]
IGNORE = 255


def _labels(size):
    import numpy as np
    import torch
    out = []
    for i in range(N_ITEMS):
        g = torch.Generator().manual_seed(100 + i)
        ids = torch.tensor([0] + [NAMES.index(c) for c in TARGETS[i]])
        coarse = ids[torch.randint(0, len(ids), (7, 7), generator=g)]
        y = torch.nn.functional.interpolate(coarse[None, None].float(), size=(size, size))[0, 0].numpy().astype(np.uint8)
        t = max(1, size // 32)
        y[:t], y[-t:], y[:, :t], y[:, -t:] = 255, 255, 255, 255
        out.append(y)
    return out


def _median_per_image(v):
    return round(sorted(v)[len(v) // 2] / N_ITEMS, 3)


def kernel():
    import torch
    from conceptattention_amd import ops
    K, nclass = len(BACKGROUND) + 3, len(NAMES)
    maps = torch.rand(N_ITEMS, K, 64, 64, device="cuda") ** 2
    tables = [[0] * len(BACKGROUND) + [NAMES.index(c) for c in t] for t in TARGETS]
    counts = torch.zeros(N_ITEMS, 2 + 2 * nclass, dtype=torch.int32, device="cuda")

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
        return round(sorted(ms)[10] * 1e3, 1)
    for size in SIZES:
        labels = torch.stack([torch.from_numpy(y) for y in _labels(size)]).to("cuda")
        line = {"call": f"mseg_score, 5 items of {K} maps 64 x 64 against {size} x {size} labels, one launch",
                "launch_us": med(lambda: ops.mseg_score(maps, labels, counts, tables, nclass, ignore_index=IGNORE)),
                "launch_blur_us": med(lambda: ops.mseg_score(maps, labels, counts, tables, nclass, ignore_index=IGNORE,
                                                             blur_weights=ops.seg_blur_weights()))}
        line["per_image_us"] = round(line["launch_us"] / N_ITEMS, 1)
        print(json.dumps(line), flush=True)


def loop():
    import numpy as np
    import PIL.Image
    import torch
    from frontend_throughput import build_pipeline
    from conceptattention_amd import ops
    from conceptattention_amd import segmentation as S
    pipe = build_pipeline()
    seg = S.ConceptAttentionSegmentationModel(pipe)
    images = [PIL.Image.fromarray(np.random.default_rng(i).integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8))
              for i in range(N_ITEMS)]
    prompts = [",".join(f"a {c}" for c in t) for t in TARGETS]
    lat = (1, 16, SIDE // 8, SIDE // 8)
    noise = [[torch.randn(*lat, generator=torch.Generator().manual_seed(10 + i))] for i in range(N_ITEMS)]
    vae_noise = [torch.randn(*lat, generator=torch.Generator().manual_seed(30 + i)) for i in range(N_ITEMS)]
    tables = [S.multiclass_table(BACKGROUND, t, NAMES) for t in TARGETS]
    kw = dict(batch=5, noise=noise, vae_noise=vae_noise, width=SIDE, height=SIDE)
    staged = {"on": False, "ms": 0.0}

    def bracket(fn):
        def f(*a, **k):
            if not staged["on"]:
                return fn(*a, **k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            staged["ms"] += (time.perf_counter() - t0) * 1e3
            return out
        return f

    ops.mseg_score = bracket(ops.mseg_score)     # (score_multiclass_images looks it up at call time)
    device_result = bracket(lambda dev: dev.to_host())
    # the host route's scoring part starts at the argmax: segment_multiclass is encode_images + argmax, so the route is
    # spelt out here to bracket everything behind the download of the maps
    for size in SIZES:
        labels = _labels(size)

        def score_on_host(outs):
            scores = S.MultiClassScores(len(NAMES))
            for o, y, table in zip(outs, labels, tables):
                maps = torch.as_tensor(np.asarray(o.concept_heatmaps), dtype=torch.float32)
                klass = S.map_predictions_to_class_indices(maps.argmax(dim=0), table)
                up = torch.nn.functional.interpolate(klass[None, None].float(), size=y.shape, mode="nearest")[0, 0]
                scores.update(up, y, ignore_index=IGNORE)
            return scores
        score_on_host = bracket(score_on_host)

        def host():
            outs = pipe.encode_images(images, [BACKGROUND + t for t in TARGETS], prompts, return_pil_heatmaps=False, **kw)
            return score_on_host(outs)

        def device():
            dev = S.DeviceMultiClassScores(len(NAMES), "cuda:0")
            seg.score_multiclass_images(images, prompts, BACKGROUND, TARGETS, NAMES, labels, dev, ignore_index=IGNORE, **kw)
            return device_result(dev)

        results = {}
        with torch.no_grad():
            for name, fn in (("host", host), ("device", device)):
                for _ in range(WARMUP):
                    results[name] = fn()
                torch.cuda.synchronize()
                wall, score = [], []
                for _ in range(REPEATS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                staged["on"] = True
                for _ in range(REPEATS):
                    staged["ms"] = 0.0
                    fn()
                    score.append(staged["ms"])
                staged["on"] = False
                r = results[name].result()
                print(json.dumps({"route": name, "labels": f"{size} x {size}",
                                  "per_image": {"wall_ms": _median_per_image(wall), "score_ms": _median_per_image(score)},
                                  "result": {"pixAcc": r["pixAcc"], "mIoU": r["mIoU"], "n": r["n"]}}), flush=True)
        h, d = results["host"], results["device"]
        same = (h.correct, h.labelled, h.inter.tolist(), h.union.tolist()) == (d.correct, d.labelled, d.inter.tolist(),
                                                                                d.union.tolist())
        print(json.dumps({"labels": f"{size} x {size}", "every counter of the two routes equal": same}), flush=True)


if __name__ == "__main__":
    steps = {"kernel": kernel, "loop": loop}
    if len(sys.argv) == 2:
        steps[sys.argv[1]]()
    else:
        for what in steps:
            rc = subprocess.call(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), what])
            if rc != 0:
                sys.exit(f"step {what} ended with {rc}")   # nothing more is started on the GPU
