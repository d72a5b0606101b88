"""Concept re-query: generate one picture with ``keep_trace=True``, then ask it about other word lists without running the
image pass again (``pipeline.requery``).  Each re-query costs the concept rows' own stream through the double blocks; the
trace holds the image keys, values and map operands of the traced steps until ``release()``.

Runs on seeded random-init weights behind the toy byte tokenizer (no checkpoint or vocabulary can be fetched here), so the
pictures are noise; the call sequence, shapes and outputs are the real ones.  CA_TINY=1 runs the tiny geometry at 256 x 256
(seconds instead of minutes)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conceptattention_amd import ConceptAttentionFluxPipeline, tiny_params

tiny = os.environ.get("CA_TINY") == "1"
side = 256 if tiny else 1024
pipeline = ConceptAttentionFluxPipeline(model_name="flux-schnell", device="cuda:0", text_encoder="synthetic-t5-clip",
                                        autoencoder="synthetic",
                                        **(dict(params=tiny_params(), n_text_tokens=64) if tiny else {}))
settings = dict(layer_indices=[0, 1], num_inference_steps=2) if tiny else {}

out = pipeline.generate_image(prompt="A cat on the grass", concepts=["cat", "grass", "sky"], width=side, height=side,
                              keep_trace=True, **settings)
trace = out.trace
print(f"the trace holds {trace.nbytes / 1e9:.3f} GB: steps {trace.timesteps}, layers {trace.layer_indices}")

out_dir = sys.argv[1] if len(sys.argv) > 1 else "results"
os.makedirs(out_dir, exist_ok=True)
out.image.save(os.path.join(out_dir, "image.png"))
word_lists = {"first": ["cat", "grass", "sky"],
              "background": ["tree", "road", "cloud", "wall", "water"],
              "classes": [f"class {i}" for i in range(21)]}          # 9 .. 32 concepts: one ca_heatmap_many launch per layer
for name, words in word_lists.items():
    again = pipeline.requery(trace, words)
    assert again.image is out.image and again.token_heatmaps is None
    for word, picture in zip(words, again.concept_heatmaps):
        picture.save(os.path.join(out_dir, f"{name}_{word.replace(' ', '_')}.png"))
    print("re-queried", len(words), "concepts:", name)
last_layer = pipeline.requery(trace, word_lists["background"], layer_indices=trace.layer_indices[-1:])   # any subset
trace.release()
print("wrote the pictures to", out_dir)
