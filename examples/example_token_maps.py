"""Prompt-token attention maps (DAAM for Flux) next to the concept maps of the same run: for every token of the prompt, the
attention the image tokens give that token's key in the captured double blocks, mean over heads, layers and steps
(``token_maps=True``; ops.token_maps / ca_token_maps).  One picture per token.

Runs on seeded random-init weights behind the toy byte tokenizer (no checkpoint or vocabulary can be fetched here), so the
tokens are the prompt's bytes and the pictures are noise; the call sequence, shapes and outputs are the real ones.
CA_TINY=1 runs the tiny geometry at 256 x 256 (seconds instead of minutes)."""
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

out = pipeline.generate_image(prompt=prompt, concepts=concepts, width=side, height=side, token_maps=True,
                              **(dict(layer_indices=[0, 1], num_inference_steps=2) if tiny else {}))

out_dir = sys.argv[1] if len(sys.argv) > 1 else "results"
os.makedirs(out_dir, exist_ok=True)
assert len(out.token_heatmaps) == len(out.tokens) == len(prompt.encode("utf-8"))
for i, (token, picture) in enumerate(zip(out.tokens, out.token_heatmaps)):
    name = token if token.isalnum() else f"0x{ord(token):02x}"
    picture.save(os.path.join(out_dir, f"token_{i:02d}_{name}.png"))
for concept, picture in zip(concepts, out.concept_heatmaps):
    picture.save(os.path.join(out_dir, f"concept_{concept}.png"))
print("wrote", len(out.tokens), "token maps and", len(concepts), "concept maps of", out.token_heatmaps[0].size, "to", out_dir)
