"""CPU checks of the batched front end's host logic: the grouping plan of ``encode_images`` / ``generate_images`` and the
concept cache of ``FluxGenerator.embed_many`` (with a fake text encoder: no GPU, no kernels)."""
import inspect
from dataclasses import fields

import numpy as np
import pytest
import torch

from conceptattention_amd import segmentation as S
from conceptattention_amd.image_generator import ConceptCache, FluxGenerator
from conceptattention_amd.pipeline import (MAX_ITEMS_PER_FORWARD, ConceptAttentionFluxPipeline, EncodeSettings, _per_item,
                                           plan_batches)


# ---------------------------------------------------------------------------------------------------------- the plan
def test_plan_keeps_order_and_bounds_the_chunks():
    assert MAX_ITEMS_PER_FORWARD == 5
    plan = plan_batches(["a"] * 12, 5)
    assert plan == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11]]
    assert plan_batches(["a"] * 12, 64) == plan                       # never more than the launches take
    assert plan_batches(["a"] * 3, 1) == [[0], [1], [2]] == plan_batches(["a"] * 3, 0)
    assert plan_batches([], 5) == []


def test_plan_groups_mixed_shapes_and_concept_counts():
    k2, k3, big = ((16, 32, 32), 2, 64), ((16, 32, 32), 3, 64), ((16, 64, 64), 2, 64)
    keys = [k2, k3, k2, big, k2, k2, k3, k2, k2, big]
    plan = plan_batches(keys, 5)
    assert plan == [[0, 2, 4, 5, 7], [8], [1, 6], [3, 9]]               # groups in the order of their first item
    assert sorted(i for c in plan for i in c) == list(range(len(keys)))  # every item exactly once
    for chunk in plan:
        assert chunk == sorted(chunk) and len({keys[i] for i in chunk}) == 1 and 1 <= len(chunk) <= 5
    # the seven-image case of the GPU test: two of them carry a third concept
    assert plan_batches([k3 if i in (1, 4) else k2 for i in range(7)], 5) == [[0, 2, 3, 5, 6], [1, 4]]


def test_one_concept_list_for_all_items_or_one_per_item():
    assert _per_item(["cat", "sky"], 3, "x") == [["cat", "sky"]] * 3
    assert _per_item([["cat"], ["sky", "sea"]], 2, "x") == [["cat"], ["sky", "sea"]]
    with pytest.raises(ValueError):
        _per_item([["cat"], ["sky"]], 3, "x")


# ---------------------------------------------------------------------------------------------------------- the settings
@pytest.mark.parametrize("method", [ConceptAttentionFluxPipeline.encode_image, ConceptAttentionFluxPipeline.encode_images,
                                    ConceptAttentionFluxPipeline.encode_many_on_device,
                                    S.ConceptAttentionSegmentationModel.segment_images,
                                    S.ConceptAttentionSegmentationModel.segment_individual_image],
                         ids=lambda m: m.__name__)
def test_the_public_defaults_are_the_settings_records(method):
    """Every parameter of a public encode call that is a field of the record (``layers``: the harness's name of
    layer_indices) has the record's default.  The one exception is ``batch`` of ``encode_many_on_device``: the throughput
    call's own argument, public with the default 1 (one item per forward unless the caller asks) since before the record."""
    record, params, seen = EncodeSettings(), inspect.signature(method).parameters, set()
    for f in fields(EncodeSettings):
        name = "layers" if f.name == "layer_indices" and "layers" in params else f.name
        if name not in params or (method.__name__, name) == ("encode_many_on_device", "batch"):
            continue
        assert params[name].default == getattr(record, f.name), (method.__name__, name)
        seen.add(f.name)
    assert {"layer_indices", "num_samples", "num_steps", "noise_timestep", "seed"} <= seen


def test_harness_keywords_become_the_settings_record():
    assert S.encode_settings({}) == EncodeSettings()
    with pytest.raises(TypeError, match=r"^score_images: unexpected arguments \['layer'\]$"):
        S.encode_settings({"layer": 1, "seed": 0}, "score_images")
    values = {"layers": [0, 1], "num_samples": 2, "num_steps": 3, "noise_timestep": 1, "seed": 7, "height": 256, "width": 256,
              "batch": 2, "joint_attention_kwargs": {"concept_self_attention": False}, "noise": [None], "vae_noise": [None],
              "attention_norm": "entmax15", "softmax": False}
    assert set(values) == S._ENCODE_KEYS
    for key, value in values.items():
        got = S.encode_settings({key: value, **({"width": 256} if key == "height" else {"height": 256} if key == "width" else {})})
        if key not in ("noise", "vae_noise"):                          # (per-call data: no field of the record)
            assert getattr(got, "layer_indices" if key == "layers" else key) == value
    full = S.encode_settings(values)
    assert (full.layer_indices, full.batch, full.norm, full.stop_after_multi_modal_attentions) == ([0, 1], 2, 2, True)
    assert full.keywords()["layer_indices"] == [0, 1] and "norm" not in full.keywords()


def test_the_settings_record_makes_the_checks_of_an_encode_call():
    assert EncodeSettings(layer_indices=[0, 18], depth=19).norm == 0      # softmax=True wins over the name
    for bad in ([19], [-1], [0, 2]):
        with pytest.raises(AssertionError, match="Invalid layer index"):
            EncodeSettings(layer_indices=bad, depth=2 if bad == [0, 2] else 19)
    with pytest.raises(AssertionError, match="Height and width"):
        EncodeSettings(height=512)
    with pytest.raises(ValueError, match="Unknown attention_norm=softmin"):
        EncodeSettings(attention_norm="softmin", softmax=False)
    assert EncodeSettings(attention_norm="softmin").norm == 0             # (as the reference: never looked at with softmax)
    with pytest.raises(ValueError, match=r"33 concepts.*at most 32"):
        EncodeSettings(softmax=False, n_concepts=33)
    assert EncodeSettings(n_concepts=33).norm == 0                        # the softmax has no limit
    with pytest.raises(Exception):                                        # frozen
        EncodeSettings().seed = 1


# ---------------------------------------------------------------------------------------------------------- scoring inputs
def test_scoring_inputs_from_one_concept_list_or_one_per_item():
    labels = [np.zeros((8, 8), dtype=np.uint8), np.ones((8, 8), dtype=bool)]
    per_item, target, lab, blur = S._scoring_inputs(["cat", "sky"], ["sky", "cat"], labels, 8, False)
    assert per_item == [["cat", "sky"]] * 2 and target == [1, 0] and blur is None
    assert [y.dtype for y in lab] == [np.uint8, np.uint8] and lab[1].all() and not lab[0].any()
    per_item, target, _, _ = S._scoring_inputs([["cat", "sky"], ["sea", "sky", "cat"]], ["sky", "cat"], labels, 8, False)
    assert per_item == [["cat", "sky"], ["sea", "sky", "cat"]] and target == [1, 2]
    with pytest.raises(ValueError, match="unicorn"):
        S._scoring_inputs(["cat", "sky"], ["sky", "unicorn"], labels, 8, False)
    with pytest.raises(ValueError, match=r"^labels\[1\]: expected a uint8 / bool array \(8, 8\), got uint8 \(8, 4\)$"):
        S._scoring_inputs(["cat", "sky"], ["sky", "cat"], [labels[0], np.zeros((8, 4), dtype=np.uint8)], 8, False)
    with pytest.raises(ValueError, match=r"^labels\[0\]: .*got int64 \(8, 8\)$"):
        S._scoring_inputs(["cat", "sky"], ["sky", "cat"], [np.zeros((8, 8), dtype=np.int64), labels[1]], 8, False)


# ---------------------------------------------------------------------------------------------------------- the cache
class FakeEncoder:
    """t5_many / clip with the shapes of the real ones; the value of a row names the string it came from."""
    T, D, V = 4, 8, 6

    def __init__(self):
        self.calls = []

    @staticmethod
    def _code(text):
        return float(sum(text.encode()) % 251)

    def t5_many(self, texts):
        self.calls.append(list(texts))
        out = torch.zeros(len(texts), self.T, self.D, dtype=torch.bfloat16)
        for i, t in enumerate(texts):
            out[i] = self._code(t)
            out[i, 1:] += 1            # only token 0 is the concept's vector
        return out

    def clip(self, text):
        return torch.full((1, self.V), self._code(text) + 0.5, dtype=torch.bfloat16)


def _generator(enc, max_entries=4096):
    gen = object.__new__(FluxGenerator)      # the host logic alone: no model, no device
    gen.text_encoder, gen.t5, gen.clip = enc, getattr(enc, "t5", None), enc.clip
    gen.concept_cache, gen.t5_sequences_encoded = ConceptCache(max_entries), 0
    return gen


def test_embed_many_equals_embed_and_counts_what_it_encodes():
    enc = FakeEncoder()
    gen = _generator(enc)
    prompts, concepts = ["p one", "p two", "p one"], [["cat", "sky"], ["sky", "sea", "cat"], ["sea"]]
    many = gen.embed_many(prompts, concepts)
    assert enc.calls == [["p one", "p two", "cat", "sky", "sea"]] and gen.t5_sequences_encoded == 5   # ONE call, distinct strings
    for item, p, c in zip(many, prompts, concepts):
        for a, b in zip(item, gen.embed(p, c)):
            assert a.shape == b.shape and torch.equal(a, b)
    assert tuple(many[1][2].shape) == (1, 3, FakeEncoder.D) and tuple(many[1][3].shape) == (1, 3, 3)
    assert not many[0][4].any()                                       # the concepts' pooled vector is zero
    enc.calls.clear()
    gen.embed_many(["p three"], [["cat", "sea"]])
    assert enc.calls == [["p three"]] and gen.t5_sequences_encoded == 6   # the concepts came from the cache
    with pytest.raises(ValueError):
        gen.embed_many(["a", "b"], [["cat"]])


def test_the_cache_is_bounded_lru_and_dropped_with_its_encoder():
    enc = FakeEncoder()
    gen = _generator(enc, max_entries=3)
    gen.embed_many(["p"], [["a", "b", "c"]])
    assert len(gen.concept_cache) == 3
    gen.embed_many(["p"], [["a"]])                 # touches "a": "b" is now the oldest
    gen.embed_many(["p"], [["d"]])
    assert len(gen.concept_cache) == 3 and "b" not in gen.concept_cache and "a" in gen.concept_cache
    enc.calls.clear()
    out = gen.embed_many(["p"], [["a", "b", "c", "d", "e"]])      # more concepts than entries: still every vector right
    assert enc.calls == [["p", "b", "e"]] and len(gen.concept_cache) == 3
    assert [float(v) for v in out[0][2][0, :, 0]] == [FakeEncoder._code(c) for c in "abcde"]
    other = FakeEncoder()
    gen.text_encoder, gen.clip = other, other.clip                 # another encoder object: nothing of the old one survives
    gen.embed_many(["p"], [["a"]])
    assert other.calls == [["p", "a"]] and len(gen.concept_cache) == 1
    with pytest.raises(ValueError):
        ConceptCache(0)


def test_an_encoder_without_t5_many_goes_through_embed_per_item():
    class Plain:
        def __init__(self):
            self.n = 0

        def t5(self, text):
            self.n += 1
            return torch.full((1, 4, 8), FakeEncoder._code(text), dtype=torch.bfloat16)

        def clip(self, text):
            return torch.full((1, 6), FakeEncoder._code(text) + 0.5, dtype=torch.bfloat16)
    enc = Plain()
    gen = _generator(enc)
    out = gen.embed_many(["p", "q"], [["a", "b"], ["a"]])
    assert enc.n == 5 and gen.t5_sequences_encoded == 0 and len(gen.concept_cache) == 0
    assert torch.equal(out[1][2], gen.embed("q", ["a"])[2])
