"""Time per image of the segmentation eval loop, scores on the host against scores on the device.

1024 x 1024 images, labels at 224 x 224, the pipeline of tools/frontend_throughput.py (real geometries, synthetic weights),
5 images per call, the concept list of the harness.  Two routes over the same images and labels:

* ``host``:   ``encode_images(batch=5)``, then per image the mean-threshold mask, ``prepare_for_scoring`` and
              ``SegmentationScores.update`` on the downloaded maps -- the route of examples/segmentation_eval.py;
* ``device``: ``ConceptAttentionSegmentationModel.score_images`` with a ``DeviceSegmentationScores`` and its ``result()``
              (the one download of the records).
Both routes get the same diffusion and autoencoder noise, so their scores must agree (the last line printed).

Two warm-up calls, then the median of five, per image (the call's time / 5): ``wall_ms`` is a host clock around the whole
call, which ends in a device synchronise; ``score_ms`` comes from a second set of runs in which the scoring part is
bracketed by device synchronises and a host clock (host: mask + prepare_for_scoring + update of the 5 images; device: the
``ops.seg_score`` launches and ``result()``).  ``kernel`` times ``ops.seg_score`` alone for 5 maps of 64 x 64 against
224 x 224 labels by HIP events (median of 20 launches after 3).  One JSON line per measurement; nothing here is a gate.
    python tools/segmentation_throughput.py            # both steps, each a process of its own under a time limit
    python tools/segmentation_throughput.py kernel     # one step: kernel | loop
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_ITEMS, SIDE, SIZE, WARMUP, REPEATS = 5, 1024, 224, 2, 5
CONCEPTS = ["object", "background", "floor", "grass", "tree", "sky"]


def _labels():
    import numpy as np
    import torch
    out = []
    for i in range(N_ITEMS):
        g = torch.Generator().manual_seed(100 + i)
        y = torch.nn.functional.interpolate(torch.rand(1, 1, 7, 7, generator=g), size=(SIZE, SIZE))[0, 0] > 0.5
        out.append(y.numpy().astype(np.uint8))
    return out


def _median_per_image(v):
    return round(sorted(v)[len(v) // 2] / N_ITEMS, 3)


def kernel():
    import torch
    from conceptattention_amd import ops
    maps = torch.rand(N_ITEMS, 64, 64, device="cuda") ** 2
    labels = torch.stack([torch.from_numpy(y) for y in _labels()]).to("cuda")
    res = torch.zeros(N_ITEMS, ops.SEG_RECORD_BYTES, dtype=torch.uint8, device="cuda")

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
    line = {"call": "seg_score, 5 maps 64 x 64 against 224 x 224 labels, one launch",
            "launch_us": med(lambda: ops.seg_score(list(maps), list(labels), res)),
            "launch_blur_downscale_us": med(lambda: ops.seg_score(list(maps), list(labels), res, downscale_for_eval=True,
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
    prompts = [f"a photo of object number {i}" for i in range(N_ITEMS)]
    lat = (1, 16, SIDE // 8, SIDE // 8)
    noise = [[torch.randn(*lat, generator=torch.Generator().manual_seed(10 + i))] for i in range(N_ITEMS)]
    vae_noise = [torch.randn(*lat, generator=torch.Generator().manual_seed(30 + i)) for i in range(N_ITEMS)]
    labels = _labels()
    targets = ["object"] * N_ITEMS
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

    def score_on_host(outs):
        scores = S.SegmentationScores()
        for o, y in zip(outs, labels):
            coeff = torch.as_tensor(np.asarray(o.concept_heatmaps), dtype=torch.float32)
            mask = S.target_mask(coeff, 0)
            c, m = S.prepare_for_scoring(coeff[0].numpy(), mask.numpy(), size=SIZE)
            scores.update(m, c, y.astype(bool))
        return scores.result()
    score_on_host = bracket(score_on_host)
    ops.seg_score = bracket(ops.seg_score)     # (score_images looks it up at call time)
    device_result = bracket(lambda dev: dev.result())

    def host():
        outs = pipe.encode_images(images, CONCEPTS, prompts, batch=5, noise=noise, vae_noise=vae_noise, width=SIDE,
                                  height=SIDE, return_pil_heatmaps=False)
        return score_on_host(outs)

    def device():
        dev = S.DeviceSegmentationScores("cuda:0")
        seg.score_images(images, targets, CONCEPTS, prompts, labels, dev, size=SIZE, batch=5, noise=noise, vae_noise=vae_noise,
                         width=SIDE, height=SIDE)
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
            print(json.dumps({"route": name, "per_image": {"wall_ms": _median_per_image(wall),
                                                           "score_ms": _median_per_image(score)},
                              "result": results[name]}), flush=True)
    diff = max(abs(results["host"][k] - results["device"][k]) for k in ("pixAcc", "mIoU", "mAP"))
    print(json.dumps({"largest difference of pixAcc / mIoU / mAP between the routes": diff}), flush=True)


if __name__ == "__main__":
    steps = {"kernel": kernel, "loop": loop}
    if len(sys.argv) == 2:
        steps[sys.argv[1]]()
    else:
        for what in steps:
            rc = subprocess.call(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), what])
            if rc != 0:
                sys.exit(f"step {what} ended with {rc}")   # nothing more is started on the GPU
