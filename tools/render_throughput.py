"""Time per image of the heat-map pictures: what ``_finish`` costs on the host against ops.heatmap_render on the device.

The pipeline of tools/frontend_throughput.py (the real geometries on synthetic weights) makes one image at 1024 x 1024 with 4
concepts; its two fp32 accumulators [1, 4, 64, 64] and the decoded picture's bytes stay on the device and every route below
turns them into the two lists of 4 PIL pictures.  Two warm-up calls, then the median of five, host clock around the route
with a device synchronise on either side:

  a  host          ``_finish`` as it is without the feature: download the maps, colorize_heatmaps (64 x 64 pictures)
  b  device        ``_finish_device``: the same 64 x 64 pictures from one launch, one download of bytes
  c  device overlays   bilinear to 1024 x 1024 blended over the picture with alpha 0.5, one launch, one download
  d  host overlays     the same from downloaded maps: F.interpolate on the CPU, matplotlib, a numpy blend
  e  torch overlays    the same with torch operations on the device and one download: the route that needs no kernel

and the call alone (``ops.heatmap_render``: its two to four launches, without download) by HIP events (median of 20 calls
after 3) at 64 -> 64 and 64 -> 1024 for the 8 planes, with the bytes it writes per second; the gaps between the small launches
are in that figure, a kernel trace separates them.  One JSON line per row; nothing printed here is a gate.
    python tools/render_throughput.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIDE, WARMUP, REPEATS, ALPHA = 1024, 2, 5, 0.5
CONCEPTS = ["cat", "grass", "sky", "tree"]


def timed(name, fn, extra=None):
    import torch
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"route": name, "per_image_ms": round(sorted(ms)[REPEATS // 2], 3), **(extra or {})}), flush=True)


def main():
    import matplotlib.pyplot as plt
    import numpy as np
    import PIL.Image
    import torch
    import torch.nn.functional as F
    from frontend_throughput import build_pipeline
    from conceptattention_amd import ops
    pipe = build_pipeline()
    with torch.no_grad():
        txt, vec, con, _, _ = pipe._embed("A cat in a park on the grass by a tree", CONCEPTS)
        latent = torch.randn(1, 16, SIDE // 8, SIDE // 8, generator=torch.Generator().manual_seed(0))
        img, ho, hc = pipe.generate_on_device(latent, txt, vec, con)
        pix = pipe.flux_generator.decode_pixels(img, SIDE, SIDE)
    image = PIL.Image.fromarray(pix[0].cpu().numpy())
    cmap = plt.get_cmap("plasma")
    lut = ops.colormap_lut("plasma", pipe.device)
    lut_f = lut[:256].float()

    def host_overlays():
        picture = pix[0].cpu().numpy().astype(np.float32)
        out = []
        for t in (ho, hc):
            maps = t[0].cpu()
            lo, hi = maps.min(), maps.max()
            up = F.interpolate(maps[None], size=(SIDE, SIDE), mode="bilinear", align_corners=False)[0]
            for m in ((up - lo) / (hi - lo)).numpy():
                rgb = cmap(m)[:, :, :3] * 255
                out.append(PIL.Image.fromarray((rgb * ALPHA + picture * (1 - ALPHA) + 0.5).astype(np.uint8)))
        return out

    def torch_overlays():
        picture = pix[0].float()
        planes = []
        for t in (ho, hc):
            lo, hi = torch.aminmax(t[0])
            up = F.interpolate(t, size=(SIDE, SIDE), mode="bilinear", align_corners=False)[0]
            rows = (((up - lo) / (hi - lo)) * 256).clamp_(0, 255).long()
            planes.append((lut_f[rows] * ALPHA + picture * (1 - ALPHA) + 0.5).to(torch.uint8))
        host = torch.stack(planes).cpu().numpy()
        return [PIL.Image.fromarray(p) for p in host.reshape(-1, SIDE, SIDE, 3)]

    with torch.no_grad():
        timed("a host (_finish, 64 x 64)", lambda: pipe._finish(image, ho, hc, True, "plasma"))
        timed("b device (64 x 64)", lambda: pipe._finish_device([image], ho, hc, "plasma"))
        timed("c device overlays (bilinear, 1024 x 1024)",
              lambda: pipe._finish_device([image], ho, hc, "plasma", None, "bilinear", ALPHA, pix))
        timed("d host overlays (F.interpolate + matplotlib + numpy)", host_overlays)
        timed("e torch overlays on the device", torch_overlays)

        def events(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            us = []
            for _ in range(20):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                us.append(a.elapsed_time(b) * 1e3)
            return sorted(us)[10]
        groups = [ho[0], hc[0]]
        for side, kw in ((64, {}), (SIDE, dict(bilinear=True)), (SIDE, dict(bilinear=True, images=pix[0], alpha=ALPHA))):
            out = [torch.empty(4, side, side, 3, dtype=torch.uint8, device=pipe.device) for _ in groups]
            us = events(lambda: ops.heatmap_render(groups, lut, size=side, out=out, **kw))
            nbytes = 8 * 3 * side * side
            print(json.dumps({"call": f"ops.heatmap_render 64 -> {side}, 8 planes" + (", blend" if "images" in kw else ""),
                              "us": round(us, 1), "bytes_written": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1),
                              "beside": "ca_nhwc_f32_to_pixels_u8 at 1.1 TB/s"}), flush=True)


if __name__ == "__main__":
    main()
