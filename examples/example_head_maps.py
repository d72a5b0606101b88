"""Per-head concept maps and the raw-space baselines next to the concept maps of the same run: for every attention head,
the logits of the concept rows against the image rows in the attention-output, cross-attention (q) and value spaces,
weighted across the concepts per head (``head_maps=``; ops.head_maps / ca_head_maps), and their mean over the heads: the
reference's RawOutputSpace / RawCrossAttention / RawValueSpace baselines (conceptattention_amd/baselines.py).

Runs on seeded random-init weights (no checkpoint can be fetched here), so the pictures are noise; the call sequence,
shapes and outputs are the real ones.  CA_TINY=1 runs the tiny geometry at 256 x 256 (seconds instead of minutes)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conceptattention_amd import ConceptAttentionFluxPipeline, tiny_params
from conceptattention_amd.baselines import RawValueSpaceSegmentationModel
from conceptattention_amd.pipeline import colorize_heatmaps

tiny = os.environ.get("CA_TINY") == "1"
side = 256 if tiny else 1024
pipeline = ConceptAttentionFluxPipeline(model_name="flux-schnell", device="cuda:0",
                                        **(dict(params=tiny_params(), n_text_tokens=8) if tiny else {}))

prompt = "A cat on the grass"
concepts = ["cat", "grass", "sky"]
small = dict(layer_indices=[0, 1], num_inference_steps=2) if tiny else {}

out = pipeline.generate_image(prompt=prompt, concepts=concepts, width=side, height=side,
                              head_maps=("output", "cross", "value"), head_norm="softmax", **small)
heads = out.head_maps["output"]                       # fp32 device tensor (num_heads, C, h, w)
num_heads = heads.shape[0]
assert out.raw_heatmaps["output"].shape == heads.shape[1:]

# which heads localise a concept: the spatial contrast of every head's map of concept 0, largest first
contrast = heads[:, 0].flatten(1).std(1)
order = torch.argsort(contrast, descending=True).tolist()
print(f"heads by the contrast of their '{concepts[0]}' map (output space):", order[:8], "...")

out_dir = sys.argv[1] if len(sys.argv) > 1 else "results"
os.makedirs(out_dir, exist_ok=True)
for space, maps in out.raw_heatmaps.items():          # the baselines' maps of this run, one picture per concept
    for concept, picture in zip(concepts, colorize_heatmaps(maps.cpu().numpy())):
        picture.save(os.path.join(out_dir, f"raw_{space}_{concept}.png"))
for h in order[:4]:                                   # the four most contrasted heads of concept 0
    colorize_heatmaps(heads[h, :1].cpu().numpy())[0].save(os.path.join(out_dir, f"head_{h:02d}_{concepts[0]}.png"))

# the baseline class, as the reference's segmentation harness calls it: a latent (or, with an autoencoder, a PIL image)
latent = torch.randn(1, 16, side // 8, side // 8, generator=torch.Generator().manual_seed(0))
model = RawValueSpaceSegmentationModel(pipeline)
maps, _ = model.segment_individual_image(latent, concepts, prompt, height=side, width=side,
                                         **(dict(num_steps=2, noise_timestep=1) if tiny else {}))
assert maps.shape == (len(concepts), side // 16, side // 16) and np.isfinite(maps.cpu().numpy()).all()
print("wrote the raw maps of 3 spaces and 4 head maps of", tuple(heads.shape[2:]), "to", out_dir, "-", num_heads, "heads")
