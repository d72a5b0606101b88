"""Concept re-query, what holds without a device: the new keywords' defaults, the grouping of re-query items, the memory
arithmetic of a trace, the concept side of the text embedding alone, and the property the feature rests on -- the image
rows never see a concept row -- on the fp32 oracle."""
import inspect

import pytest
import torch

from conceptattention_amd.flux_dit import HipFluxDiT, StepTrace, modulation_rows, step_trace_nbytes
from conceptattention_amd.image_generator import ConceptCache, FluxGenerator
from conceptattention_amd.params import configs, tiny_params
from conceptattention_amd.pipeline import (MAX_ITEMS_PER_FORWARD, ConceptAttentionFluxPipeline,
                                           ConceptAttentionPipelineOutput, ImageTrace, plan_batches, plan_requery,
                                           trace_nbytes)

P = ConceptAttentionFluxPipeline


# ---------------------------------------------------------------------------------------------------------- 10. keywords
@pytest.mark.parametrize("method", [P.generate_image, P.generate_images, P.encode_image, P.encode_images],
                         ids=lambda m: m.__name__)
def test_keep_trace_is_off_by_default(method):
    assert inspect.signature(method).parameters["keep_trace"].default is False


def test_the_output_has_no_trace_unless_asked():
    out = ConceptAttentionPipelineOutput(image=None, concept_heatmaps=[], cross_attention_maps=[])
    assert out.trace is None and out.token_heatmaps is None
    assert inspect.signature(HipFluxDiT.__call__).parameters["trace"].default is None


def test_requery_signature():
    params = inspect.signature(P.requery).parameters
    assert list(params)[:3] == ["self", "trace", "concepts"]
    want = dict(layer_indices=None, timesteps=None, softmax=True, attention_norm="sparsemax", cmap="plasma",
                return_pil_heatmaps=True, heatmap_renderer="host", heatmap_size=None, heatmap_interpolation="nearest",
                overlay_alpha=None)
    assert {k: params[k].default for k in want} == want
    # the presentation keywords are generate_image's, with its defaults
    gen = inspect.signature(P.generate_image).parameters
    for k in ("softmax", "attention_norm", "cmap", "return_pil_heatmaps", "heatmap_renderer", "heatmap_size",
              "heatmap_interpolation", "overlay_alpha"):
        assert params[k].default == gen[k].default, k
    assert list(inspect.signature(HipFluxDiT.requery).parameters) == ["self", "step_traces", "concepts", "concept_ids",
                                                                      "heatmaps"]


# ---------------------------------------------------------------------------------------------------------- 11. grouping
def test_requery_items_are_grouped_by_geometry_and_concept_count():
    assert MAX_ITEMS_PER_FORWARD == 5
    g, h = ("1024", (15, 16)), ("512", (15, 16))
    # seven items of one geometry and count: 5 + 2, in order
    assert plan_requery([g] * 7, [4] * 7) == [[0, 1, 2, 3, 4], [5, 6]]
    # another concept count or another geometry starts a group of its own; groups in the order of their first item
    assert plan_requery([g, g, h, g, h], [4, 9, 4, 4, 4]) == [[0, 3], [1], [2, 4]]
    assert plan_requery([], []) == []
    assert plan_requery([g, g], [1, 1]) == plan_batches([(g, 1), (g, 1)], 5) == [[0, 1]]
    with pytest.raises(ValueError):
        plan_requery([g], [1, 2])


# ---------------------------------------------------------------------------------------------------------- 12. memory
def test_trace_memory_arithmetic():
    tiny = tiny_params(depth=2, depth_single_blocks=2)          # H = 256
    assert modulation_rows(tiny) == (12 * 2 + 3 * 2 + 2) * 256 == 8192
    # C = 3, T = 8, L = 256 -> 267 rows; blocks 0 .. 1, both captured
    slabs = 2 * 267 * 768 * 2                                   # bf16 [267, 3H] per block
    rows32 = 2 * (264 * 256 * 4 + 267 * 256 * 4)                # fp32 [T+L, H] attention rows + fp32 [n, H] q rows per layer
    assert step_trace_nbytes(tiny, 3, 8, 256, 2, 2) == slabs + rows32 + 8192 * 4 == 1940480
    assert trace_nbytes(tiny, 3, 8, 256, [0, 1], 1) == 1940480
    assert trace_nbytes(tiny, 3, 8, 256, [1], 2) == 2 * (slabs + rows32 // 2 + 8192 * 4)   # layer 1 alone still keeps block 0
    assert trace_nbytes(tiny, 3, 8, 256, [], 3) == 3 * 8192 * 4
    full = configs["flux-schnell"]                              # H = 3072, 19 + 38 blocks
    assert modulation_rows(full) == (12 * 19 + 3 * 38 + 2) * 3072 == 1056768
    # 1024 x 1024, C = 4, T = 256: 4356 rows; layers 15 .. 18 -> blocks 0 .. 18
    per_step = 19 * 4356 * 9216 * 2 + 4 * (4352 * 3072 * 4 + 4356 * 3072 * 4) + 1056768 * 4
    assert per_step == 1525506048 + 428015616 + 4227072 == 1957748736            # 1.96 GB
    assert trace_nbytes(full, 4, 256, 4096, range(15, 19), 4) == 4 * per_step == 7830994944   # 7.8 GB per item
    # an unfilled or released trace holds nothing
    assert StepTrace().nbytes == 0
    t = ImageTrace({}, {}, None)
    assert t.nbytes == 0 and t.layer_indices == [] and t.timesteps == []
    t.release()
    assert t.released


# ---------------------------------------------------------------------------------------------------------- embedding
class FakeEncoder:
    D = 8

    def __init__(self):
        self.calls = []

    @staticmethod
    def _code(text):
        return float(sum(map(ord, text)) % 97)

    def t5_many(self, texts):
        self.calls.append(list(texts))
        return torch.stack([torch.full((4, self.D), self._code(t), dtype=torch.bfloat16) for t in texts])

    def t5(self, text):
        return self.t5_many([text])

    def clip(self, text):
        return torch.full((1, 6), self._code(text) + 0.5, dtype=torch.bfloat16)


def _generator(enc):
    gen = object.__new__(FluxGenerator)      # the host logic alone: no model, no device
    gen.text_encoder, gen.t5, gen.clip = enc, enc.t5, enc.clip
    gen.concept_cache, gen.t5_sequences_encoded = ConceptCache(), 0
    return gen


def test_concepts_alone_are_embedded_as_embed_many_embeds_them():
    enc = FakeEncoder()
    gen = _generator(enc)
    many = gen.embed_many(["p", "q"], [["cat", "sky"], ["sea"]])
    enc.calls.clear()
    got = gen.embed_concepts_many([["sky", "sea", "dog"], ["cat"]])
    assert enc.calls == [["dog"]]                                 # no prompt; only what the cache does not hold
    assert tuple(got[0][0].shape) == (1, 3, FakeEncoder.D) and tuple(got[0][1].shape) == (1, 3, 3) and not got[0][1].any()
    assert torch.equal(got[1][0], many[0][2][:, :1]) and torch.equal(got[0][0][:, 1], many[1][2][:, 0])
    enc.calls.clear()
    gen.embed_concepts_many([["cat", "dog"]])
    assert enc.calls == []                                        # nothing to encode: no call at all

    class Plain:
        def t5(self, text):
            return torch.full((1, 4, 8), FakeEncoder._code(text), dtype=torch.bfloat16)

        def clip(self, text):
            return torch.zeros(1, 6, dtype=torch.bfloat16)
    plain = _generator(Plain())
    assert torch.equal(plain.embed_concepts_many([["a", "b"]])[0][0], plain.embed("p", ["a", "b"])[2])


# ---------------------------------------------------------------------------------------------------------- 13. the oracle
def test_the_oracles_prediction_does_not_depend_on_the_concept_set():
    """The image and text rows never see a concept row (modified_double_stream_block.py:105-119): in fp32 the prediction
    and the image-side vectors of two forwards with different concept sets (and counts) are the same numbers exactly."""
    from conceptattention_amd.weights import synthetic_inputs, synthetic_state_dict
    from oracle import flux_oracle as O
    p = tiny_params(depth=2, depth_single_blocks=2)
    sd = synthetic_state_dict(p, seed=1)
    a = synthetic_inputs(p, 256, 256, n_txt=8, n_concepts=3, seed=2)
    b = synthetic_inputs(p, 256, 256, n_txt=8, n_concepts=5, seed=11)
    outs = []
    with torch.no_grad():
        for con in (a, b):
            outs.append(O.dit_forward(sd, p, O.patchify(a["latent"]), a["img_ids"], a["txt"], a["txt_ids"], con["concepts"],
                                      con["concept_ids"], a["concept_vec"], torch.tensor([0.5]), a["vec"]))
    assert torch.equal(outs[0][0], outs[1][0])
    for k in ("output_space_image_vectors", "cross_attention_image_vectors"):
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k
    assert outs[0][1]["output_space_concept_vectors"].shape[-2] == 3 and outs[1][1]["output_space_concept_vectors"].shape[-2] == 5
