"""Time per image of the front end, one item at a time against five per launch: a loop of ``encode_image`` against
``encode_images(batch=5)`` on PIL images, and a loop of ``generate_image`` against ``generate_images(batch=5)``.

1024 x 1024, the real geometries (flux-schnell DiT, the Flux autoencoder, T5-v1.1-xxl at 256 tokens, CLIP ViT-L/14 text at
77) on synthetic weights behind the toy tokenizers; 5 items, the concept list of the segmentation harness.  Two warm-up
calls, then the median of five, per image (the call's time / 5):

* ``wall_ms``: host clock around the whole call, which ends in a device synchronise -- what a user waits for;
* ``device_ms``: HIP events around the call on the current stream -- without the host work before the first launch;
* the stages, from a second set of runs in which every stage is bracketed by device synchronises and a host clock
  (so their sum exceeds ``wall_ms`` by the overlap the synchronises remove): VAE encode (with the upload of the bytes
  on the pixel route), T5, CLIP, DiT, VAE decode (with the download), and ``other`` = the rest of the call: the image
  conversion on the host (and, on the route before the pixel kernels, the upload of the fp32 image and its resize),
  tokenizers, noise, glue.  ``other`` + ``vae_encode`` is therefore "host conversion + upload + VAE" on every commit.

The same file runs on a commit that has no batched calls (it then times the loops alone), so the loop of an older
commit can serve as the yardstick.  One JSON line per measured call; nothing printed here is a gate.
    python tools/frontend_throughput.py            # every step, each a process of its own under a time limit
    python tools/frontend_throughput.py encode     # one step: encode | generate | kernels
``kernels`` times the two pixel kernels alone at 1024 x 1024 (HIP events, median of 20 launches after 3) beside the torch
operations they replace on the device.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_ITEMS, SIDE, WARMUP, REPEATS = 5, 1024, 2, 5
CONCEPTS = ["object", "background", "floor", "grass", "tree", "sky"]


def build_pipeline():
    import torch  # noqa: F401
    from t5_throughput import device_encoder
    from conceptattention_amd import ConceptAttentionFluxPipeline
    from conceptattention_amd.clip import HipClipEmbedder, ToyClipTokenizer, load_clip
    from conceptattention_amd.params import clip_params, t5_params
    from conceptattention_amd.t5 import HipTextEncoder, ToyByteTokenizer
    clip = HipClipEmbedder(load_clip(clip_params["clip-vit-large-patch14"], "cuda", "synthetic"), ToyClipTokenizer(), 77)
    text = HipTextEncoder(device_encoder(t5_params["t5-v1_1-xxl"]), ToyByteTokenizer(), 256, clip=clip)
    return ConceptAttentionFluxPipeline("flux-schnell", device="cuda:0", weights="synthetic", autoencoder="synthetic",
                                        text_encoder=text)


class Stages:
    """Brackets the stage functions of a pipeline with device synchronises and a host clock while ``on``."""

    def __init__(self, pipe):
        import torch
        self.ms, self.on, self._torch = {}, False, torch
        ae, te = pipe.autoencoder, pipe.text_encoder
        targets = [(ae, "encode", "vae_encode"), (ae, "encode_pixels", "vae_encode"), (ae, "decode", "vae_decode"),
                   (ae, "decode_pixels", "vae_decode"), (te.encoder, "encode_ids", "t5"),
                   (te.clip_embedder.encoder, "encode_ids", "clip"), (pipe, "_encode_maps", "dit"),
                   (pipe, "generate_on_device", "dit")]
        for obj, name, stage in targets:
            if hasattr(obj, name):
                setattr(obj, name, self._wrap(getattr(obj, name), stage))
        # the download of the decoded image belongs to the decode stage on both routes
        gen = pipe.flux_generator
        for name in ("decode_many", "decode"):
            if hasattr(gen, name):
                setattr(gen, name, self._wrap(getattr(gen, name), "vae_decode", outer=True))
                break

    def _wrap(self, fn, stage, outer=False):
        depth = [0]

        def f(*a, **k):
            if not self.on or (depth[0] and not outer):
                return fn(*a, **k)
            self._torch.cuda.synchronize()
            t0 = time.perf_counter()
            inner_before = self.ms.get(stage, 0.0) if outer else None
            depth[0] += 1
            try:
                out = fn(*a, **k)
            finally:
                depth[0] -= 1
            self._torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if outer:      # replaces what the stage's inner function added during this call
                self.ms[stage] = inner_before + dt
            else:
                self.ms[stage] = self.ms.get(stage, 0.0) + dt
            return out
        return f


def measure(name, fn, stages, cold=None):
    """``cold``: called before each of three further staged runs (it empties the concept cache); their median T5 stage is
    reported as ``t5_cold_cache_ms`` beside the steady-state figures, in which the cache is hot after the warm-up."""
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    per_stage = {}
    stages.on = True
    try:
        for _ in range(REPEATS):
            stages.ms = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
            stages.ms["other"] = total - sum(stages.ms.values())
            for k, v in stages.ms.items():
                per_stage.setdefault(k, []).append(v)
        cold_t5 = []
        for _ in range(3 if cold is not None else 0):
            cold()
            stages.ms = {}
            fn()
            cold_t5.append(stages.ms.get("t5", 0.0))
    finally:
        stages.on = False

    def med(v):
        return round(sorted(v)[len(v) // 2] / N_ITEMS, 2)
    line = {"call": name, "per_image": {"wall_ms": med(wall), "device_ms": med(dev),
                                        "stages_ms": {k: med(v) for k, v in sorted(per_stage.items())}}}
    if cold_t5:
        line["concept_cache"] = "hot in the figures above (filled by the warm-up calls)"
        line["per_image"]["t5_cold_cache_ms"] = med(cold_t5)
    print(json.dumps(line), flush=True)


def kernels():
    import torch
    from conceptattention_amd import ops
    if not hasattr(ops, "pixels_to_nhwc32"):
        return
    src = torch.randint(0, 256, (SIDE, SIDE, 3), dtype=torch.uint8, device="cuda")
    plane = torch.zeros(SIDE, SIDE, 32, dtype=torch.bfloat16, device="cuda")
    img = torch.rand(1, SIDE, SIDE, 3, device="cuda") * 2.4 - 1.2
    out = torch.empty(1, SIDE, SIDE, 3, dtype=torch.uint8, device="cuda")
    f32 = src.permute(2, 0, 1).float()[None]

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
    res = {"u8_to_nhwc32_us": med(lambda: ops.pixels_to_nhwc32(src, plane)),
           # what it replaces on the device, given the fp32 image already uploaded: layout copy + cast into the plane
           "torch_permute_cast_us": med(lambda: plane[:, :, :3].copy_(f32[0].permute(1, 2, 0))),
           "f32_to_u8_us": med(lambda: ops.nhwc_to_pixels(img, out)),
           "torch_clamp_scale_byte_us": med(lambda: (127.5 * (img.clamp(-1, 1) + 1.0)).byte()),
           "bytes_moved": {"u8_to_nhwc32": 3 * SIDE * SIDE + 64 * SIDE * SIDE, "f32_to_u8": 15 * SIDE * SIDE}}
    print(json.dumps({"call": "pixel kernels at 1024 x 1024", **res}), flush=True)


def step(what):
    import numpy as np
    import PIL.Image
    import torch
    if what == "kernels":
        return kernels()
    pipe = build_pipeline()
    stages = Stages(pipe)

    def cold():
        pipe.flux_generator.concept_cache.bind(None)
    prompts = [f"a photo of object number {i}" for i in range(N_ITEMS)]
    lat = (1, 16, SIDE // 8, SIDE // 8)
    with torch.no_grad():
        if what == "encode":
            images = [PIL.Image.fromarray(np.random.default_rng(i).integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8))
                      for i in range(N_ITEMS)]
            noise = [[torch.randn(*lat, generator=torch.Generator().manual_seed(10 + i))] for i in range(N_ITEMS)]
            kw = dict(width=SIDE, height=SIDE, return_pil_heatmaps=False)
            measure("encode_image x 5 (loop)", lambda: [pipe.encode_image(images[i], CONCEPTS, prompt=prompts[i],
                                                                          noise=noise[i], **kw) for i in range(N_ITEMS)], stages)
            if hasattr(pipe, "encode_images"):
                measure("encode_images(batch=5)", lambda: pipe.encode_images(images, CONCEPTS, prompts, batch=5, noise=noise,
                                                                             **kw), stages, cold)
        else:
            latents = [torch.randn(*lat, generator=torch.Generator().manual_seed(20 + i)) for i in range(N_ITEMS)]
            kw = dict(width=SIDE, height=SIDE, return_pil_heatmaps=False)
            measure("generate_image x 5 (loop)", lambda: [pipe.generate_image(prompts[i], CONCEPTS, latent=latents[i], **kw)
                                                          for i in range(N_ITEMS)], stages)
            if hasattr(pipe, "generate_images"):
                measure("generate_images(batch=5)", lambda: pipe.generate_images(prompts, CONCEPTS, latents=latents, batch=5,
                                                                                 **kw), stages, cold)


if __name__ == "__main__":
    if len(sys.argv) == 2:
        step(sys.argv[1])
    else:
        for what in ("kernels", "encode", "generate"):
            rc = subprocess.call(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), what])
            if rc != 0:
                sys.exit(f"step {what} ended with {rc}")   # nothing more is started on the GPU
