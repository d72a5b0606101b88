"""Concept heat maps laid over the generated picture -- the reference's plotting.overlay_heatmap_on_image (bilinear upscale
to the image size, a colour map, alpha = 0.5) without leaving the device: the decoded picture's bytes and the fp32
accumulators are already there, ``heatmap_renderer="device"`` blends them in one launch and downloads the bytes once.

Runs on seeded random-init weights (no checkpoint can be fetched here), so the pictures are noise; the call sequence,
shapes and outputs are the real ones.  CA_TINY=1 runs the tiny geometry at 256 x 256 (seconds instead of minutes)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conceptattention_amd import ConceptAttentionFluxPipeline, tiny_params

tiny = os.environ.get("CA_TINY") == "1"
side = 256 if tiny else 1024
# the overlays need the picture's bytes on the device: the HIP autoencoder
pipeline = ConceptAttentionFluxPipeline(model_name="flux-schnell", device="cuda:0", autoencoder="synthetic",
                                        text_encoder=os.environ.get("CA_TEXT_ENCODER"),
                                        **(dict(params=tiny_params(), n_text_tokens=64) if tiny else {}))

prompt = "A cat in a park on the grass by a tree"
concepts = ["cat", "grass", "sky", "tree"]

out = pipeline.generate_image(prompt=prompt, concepts=concepts, width=side, height=side,
                              **(dict(layer_indices=[0, 1], num_inference_steps=2) if tiny else {}),
                              heatmap_renderer="device", heatmap_interpolation="bilinear", overlay_alpha=0.5)

out_dir = sys.argv[1] if len(sys.argv) > 1 else "results"
os.makedirs(out_dir, exist_ok=True)
out.image.save(os.path.join(out_dir, "image.png"))
for concept, overlay in zip(concepts, out.concept_heatmaps):
    assert overlay.size == out.image.size
    overlay.save(os.path.join(out_dir, f"overlay_{concept}.png"))
for concept, overlay in zip(concepts, out.cross_attention_maps):
    overlay.save(os.path.join(out_dir, f"overlay_cross_attention_{concept}.png"))
print("wrote the image and", len(concepts) * 2, "overlays of", out.image.size, "to", out_dir)
