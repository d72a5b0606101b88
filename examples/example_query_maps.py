"""Query-row attention maps: where each word of the prompt, and each concept token, LOOKS in the image -- the softmax
probability its own query row puts on every image key in the captured double blocks, mean over heads, layers and steps
(``query_maps=("tokens", "concepts")``; ops.query_maps / ca_query_maps).  The other direction of ``token_maps``, which is
asked for as well here: it names the tokens, and its maps (what the image rows give a word's key) are written beside.

Runs on seeded random-init weights behind the toy byte tokenizer (no checkpoint or vocabulary can be fetched here), so the
tokens are the prompt's bytes, the words split at its spaces and the pictures are noise; the call sequence, shapes and
outputs are the real ones.  CA_TINY=1 runs the tiny geometry at 256 x 256 (seconds instead of minutes)."""
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
                              query_maps=("tokens", "concepts"),
                              **(dict(layer_indices=[0, 1], num_inference_steps=2) if tiny else {}))

out_dir = sys.argv[1] if len(sys.argv) > 1 else "results"
os.makedirs(out_dir, exist_ok=True)
assert out.words == prompt.split() and set(out.query_heatmaps) == {"tokens", "concepts", "words"}
assert len(out.query_heatmaps["words"]) == len(out.word_heatmaps) == len(out.words)
for i, word in enumerate(out.words):
    out.query_heatmaps["words"][i].save(os.path.join(out_dir, f"word_{i:02d}_{word}_looks_at.png"))
    out.word_heatmaps[i].save(os.path.join(out_dir, f"word_{i:02d}_{word}_is_looked_at.png"))
for concept, looks, picture in zip(concepts, out.query_heatmaps["concepts"], out.concept_heatmaps):
    looks.save(os.path.join(out_dir, f"concept_{concept}_looks_at.png"))
    picture.save(os.path.join(out_dir, f"concept_{concept}.png"))
print("wrote", len(out.words), "word maps in both directions and", len(concepts), "concept query maps of",
      out.word_heatmaps[0].size, "to", out_dir)
