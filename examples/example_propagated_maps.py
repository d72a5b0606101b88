"""Propagated concept maps: every captured layer's concept map carried through the image rows' OWN attention -- each
patch's concept scores replaced by the attention-weighted mean of the scores of the patches it attends to, mean over heads,
layers and steps (``propagate=("output", "cross")``; ops.propagate_maps / ca_propagate_maps).  The self-attention
refinement step of attention-map segmentation, applied without ever storing the patches x patches matrix.
``propagate_steps=2`` applies the layer's attention twice.

Runs on seeded random-init weights behind the toy byte tokenizer (no checkpoint or vocabulary can be fetched here), so the
pictures are noise; the call sequence, shapes and outputs are the real ones.  CA_TINY=1 runs the tiny geometry at
256 x 256 (seconds instead of minutes)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conceptattention_amd import ConceptAttentionFluxPipeline, tiny_params

tiny = os.environ.get("CA_TINY") == "1"
side = 256 if tiny else 1024
pipeline = ConceptAttentionFluxPipeline(model_name="flux-schnell", device="cuda:0", text_encoder="synthetic-t5-clip",
                                        **(dict(params=tiny_params(), n_text_tokens=64) if tiny else {}))

prompt = "A cat on the grass"
concepts = ["cat", "grass", "sky"]

out = pipeline.generate_image(prompt=prompt, concepts=concepts, width=side, height=side, propagate=("output", "cross"),
                              propagate_steps=2, **(dict(layer_indices=[0, 1], num_inference_steps=2) if tiny else {}))

out_dir = sys.argv[1] if len(sys.argv) > 1 else "results"
os.makedirs(out_dir, exist_ok=True)
assert set(out.propagated_heatmaps) == {"output", "cross"}
for space, plain in (("output", out.concept_heatmaps), ("cross", out.cross_attention_maps)):
    assert len(out.propagated_heatmaps[space]) == len(concepts)
    for concept, picture, before in zip(concepts, out.propagated_heatmaps[space], plain):
        picture.save(os.path.join(out_dir, f"{space}_{concept}_propagated.png"))
        before.save(os.path.join(out_dir, f"{space}_{concept}.png"))
print("wrote", 2 * len(concepts), "propagated maps and the maps they start from,", out.concept_heatmaps[0].size, "to", out_dir)
