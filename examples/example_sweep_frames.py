"""The frames of a concept-attention video from a noise-level sweep -- concept_attention/video/video_utils.py
(make_individual_videos: one frame per timestep, the range taken over all frames of a concept) with the frames made on the
device: ``layer_noise_sweep`` leaves its table [levels, layers, C, side, side] there, ``concept_attention_frames`` colours a
permuted view of it (no copy) and only bytes come back.  Written as one GIF per concept through PIL; no ffmpeg.

Runs on seeded random-init weights, so the pictures are noise.  CA_TINY=1 runs the tiny geometry at 256 x 256."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conceptattention_amd import ConceptAttentionFluxPipeline, concept_attention_frames, tiny_params

tiny = os.environ.get("CA_TINY") == "1"
side = 256 if tiny else 1024
pipeline = ConceptAttentionFluxPipeline(model_name="flux-schnell", device="cuda:0",
                                        text_encoder=os.environ.get("CA_TEXT_ENCODER"),
                                        **(dict(params=tiny_params(), n_text_tokens=64) if tiny else {}))

concepts = ["cat", "grass", "sky", "tree"]
steps = 4 if tiny else 50
levels = list(range(steps)) if tiny else list(range(0, steps, 5))
latent = torch.randn(1, 16, side // 8, side // 8, generator=torch.Generator().manual_seed(0))
table, _ = pipeline.layer_noise_sweep(latent, concepts, "A cat in a park on the grass by a tree", levels, num_steps=steps,
                                      width=side, height=side)
layer = table.shape[1] - 1                                        # the last double block
frames = concept_attention_frames(table[:, layer].permute(1, 0, 2, 3), cmap="inferno", per_concept=True, size=256)
host = frames.cpu().numpy()                                       # (concepts, frames, 256, 256, 3): the one download

import PIL.Image  # noqa: E402
out_dir = sys.argv[1] if len(sys.argv) > 1 else "results"
os.makedirs(out_dir, exist_ok=True)
for c, concept in enumerate(concepts):
    pictures = [PIL.Image.fromarray(f) for f in host[c]]
    pictures[0].save(os.path.join(out_dir, f"sweep_{concept}.gif"), save_all=True, append_images=pictures[1:], duration=200,
                     loop=0)
print("wrote", len(concepts), "GIFs of", host.shape[1], "frames to", out_dir)
