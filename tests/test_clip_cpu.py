"""CPU checks of the CLIP text encoder's host side: the fp64 restatement against the goldens transformers made, the
state-dict layout with and without the ``text_model.`` prefix, the real geometry, load_state_dict semantics, both
pooling rules, the toy tokenizer and the embedder's contract.  No GPU: the encoder objects here are built on the CPU
device and never run a kernel."""
import os

import numpy as np
import pytest
import torch

import clip_ref
from conceptattention_amd.clip import (PREFIX, ClipTextEncoder, HipClipEmbedder, ToyClipTokenizer, clip_state_dict_spec,
                                       pooled_positions, synthetic_clip_state_dict)
from conceptattention_amd.params import ClipTextParams, clip_params, tiny_clip_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _case(name):
    geo = clip_ref.CASES[name][0]
    return tiny_clip_params(**geo), np.load(os.path.join(GOLDEN, f"clip_{name}.npz"))


@pytest.mark.parametrize("name", list(clip_ref.CASES))
def test_restatement_matches_the_golden(name):
    """2e-5 is the margin of the other restatements here; measured: 2.0e-6 max-abs on outputs of magnitude <= 4.6, i.e.
    transformers' fp32 accumulation needs no more."""
    p, g = _case(name)
    _, length, eos_pos, eos_token_id, _ = clip_ref.CASES[name]
    ids = clip_ref.case_ids(name)
    assert np.array_equal(ids.numpy(), g["ids"]) and tuple(ids.shape) == (8, 77)
    assert list(g["pooled"]) == list(eos_pos) == clip_ref.pooled_positions(ids, eos_token_id)
    assert list(g["rows"]) == clip_ref.kept_rows(length, eos_pos) and set(eos_pos) <= set(g["rows"])
    with torch.no_grad():
        last, pooled = clip_ref.text_model(synthetic_clip_state_dict(p, 0), ids, p.num_attention_heads,
                                           p.num_hidden_layers, eos_token_id)
    assert tuple(last.shape) == (8, length, p.hidden_size) and tuple(pooled.shape) == (8, p.hidden_size)
    assert np.abs(last[:, g["rows"]].numpy() - g["hidden_f32"]).max() <= 2e-5
    assert np.abs(pooled.numpy() - g["pooler_f32"]).max() <= 2e-5
    assert 1e-3 < g["bf16_err"][0] < 2e-2 and 1e-3 < g["bf16_err"][1] < 2e-2     # the reference's own bf16 run


def test_the_goldens_cover_the_empty_prompt_the_tile_boundary_and_the_truncated_prompt():
    for name, (_, length, eos_pos, eos_token_id, (bos, eos, pad)) in clip_ref.CASES.items():
        ids = clip_ref.case_ids(name)
        assert {1, 63, 64, 65, 76} <= set(eos_pos) and len(eos_pos) == 8
        for r, e in enumerate(eos_pos):
            assert ids[r, 0] == bos and ids[r, e] == eos and (ids[r, e + 1:] == pad).all()
            assert (ids[r, 1:e] < bos).all() and (ids[r, 1:e] > 0).all()
    assert clip_ref.CASES["tiny"][3] == 2 and clip_ref.CASES["tiny"][4][1] == clip_ref.CASES["tiny"][4][2]   # arg-max rule, pad = eos
    assert clip_ref.CASES["eos"][3] == clip_ref.CASES["eos"][4][1] != clip_ref.CASES["eos"][4][2]           # first match, pad differs


def test_both_pooling_rules():
    ids = torch.tensor([[7, 3, 9, 9, 1], [2, 8, 2, 0, 0], [4, 4, 4, 4, 4]])
    assert pooled_positions(ids, 2).tolist() == [2, 1, 0] == clip_ref.pooled_positions(ids, 2)       # first arg-max
    assert pooled_positions(ids, 9).tolist() == [2, 0, 0] == clip_ref.pooled_positions(ids, 9)       # first match, 0 if none
    assert pooled_positions(ids, 4).tolist() == [0, 0, 0]
    for name in clip_ref.CASES:                    # neither rule is "the last row" on the goldens' ids
        _, length, eos_pos, eos_token_id, _ = clip_ref.CASES[name]
        got = pooled_positions(clip_ref.case_ids(name), eos_token_id).tolist()
        assert got == list(eos_pos) and got[:-1] != [length - 1] * 7


@pytest.mark.parametrize("name", list(clip_ref.CASES))
def test_spec_equals_the_goldens_keys_and_shapes_with_and_without_the_prefix(name):
    p, g = _case(name)
    theirs = {k: tuple(int(x) for x in s.split(",")) for k, s in zip(g["keys"], g["shapes"])}
    ours = dict(clip_state_dict_spec(p))
    assert {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v for k, v in theirs.items()} == ours
    sd = synthetic_clip_state_dict(p, 0)
    assert list(sd) == [k for k, _ in clip_state_dict_spec(p)] == [k[len(PREFIX):] if k.startswith(PREFIX) else k for k in g["keys"]]
    plain, prefixed = ClipTextEncoder(p, "cpu"), ClipTextEncoder(p, "cpu")
    assert plain.load_state_dict(sd) == ([], [])
    assert prefixed.load_state_dict({PREFIX + k: v for k, v in sd.items()}) == ([], [])
    assert all(torch.equal(plain.w[k], prefixed.w[k]) for k in plain.w) and set(plain.w) == set(prefixed.w)
    assert list(plain.state_dict()) == list(sd)


def test_real_geometry_is_clip_vit_large_patch14():
    p = clip_params["clip-vit-large-patch14"]
    assert p == ClipTextParams()
    assert (p.vocab_size, p.hidden_size, p.num_attention_heads, p.intermediate_size, p.num_hidden_layers) == (49408, 768, 12, 3072, 12)
    assert (p.max_position_embeddings, p.layer_norm_eps, p.eos_token_id, p.head_dim) == (77, 1e-5, 2, 64)
    spec = dict(clip_state_dict_spec(p))
    assert len(spec) == 2 + 12 * 16 + 2
    assert sum(int(np.prod(s)) for s in spec.values()) == 123_060_480          # the text model's parameter count
    ClipTextEncoder(p, "cpu")                                                  # the geometry meets the kernels' rules
    t = tiny_clip_params()
    assert (t.vocab_size, t.hidden_size, t.num_attention_heads, t.intermediate_size, t.num_hidden_layers) == (512, 256, 4, 512, 2)


def test_synthetic_weights_are_bf16_values_with_the_stated_scales():
    p = tiny_clip_params()
    sd = synthetic_clip_state_dict(p, 0)
    for k, v in sd.items():
        assert v.dtype == torch.float32 and torch.equal(v, v.to(torch.bfloat16).float()), k
    b = "encoder.layers.0"
    q = sd[f"{b}.self_attn.q_proj.weight"]
    assert abs(float(q.std()) - (2.0 / p.hidden_size) ** 0.5) < 0.1 * (2.0 / p.hidden_size) ** 0.5      # q of variance 2
    f1, b1 = sd[f"{b}.mlp.fc1.weight"], sd[f"{b}.mlp.fc1.bias"]
    assert abs(float(f1.var()) * p.hidden_size + float(b1.var()) - 1.0) < 0.1                            # unit variance
    for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2",
              "layer_norm1", "layer_norm2"):
        assert float(sd[f"{b}.{n}.bias"].abs().max()) > 0.05, n                                          # non-trivial
    assert float(sd["embeddings.position_embedding.weight"].std()) > 0.2
    assert not torch.equal(sd["final_layer_norm.bias"], synthetic_clip_state_dict(p, 1)["final_layer_norm.bias"])
    assert torch.equal(sd["final_layer_norm.bias"], synthetic_clip_state_dict(p, 0)["final_layer_norm.bias"])
    # the logits of the first layer spread over a few nats AFTER the 1 / 8 scale
    ids = clip_ref.case_ids("tiny")[-1:]
    w = {k: v.double() for k, v in sd.items()}
    x = clip_ref.embed(w["embeddings.token_embedding.weight"], w["embeddings.position_embedding.weight"], ids.reshape(-1), 77)
    h = clip_ref.layernorm(x, w[f"{b}.layer_norm1.weight"], w[f"{b}.layer_norm1.bias"])
    qq = h @ w[f"{b}.self_attn.q_proj.weight"].t() + w[f"{b}.self_attn.q_proj.bias"]
    kk = h @ w[f"{b}.self_attn.k_proj.weight"].t() + w[f"{b}.self_attn.k_proj.bias"]
    s = (qq[:, :64] @ kk[:, :64].t()) * 0.125
    assert 1.0 < float(s.std()) < 4.0


def test_load_state_dict_ignored_missing_unexpected_and_wrong_shape():
    p = tiny_clip_params()
    sd = synthetic_clip_state_dict(p, 0)
    enc = ClipTextEncoder(p, "cpu")
    assert enc.load_state_dict(sd) == ([], []) and enc.loaded
    d = p.hidden_size
    assert enc.w["0.qkv"].shape == (3 * d, d) and enc.w["0.qkv"].dtype == torch.bfloat16
    assert torch.equal(enc.w["1.qkv"][d:2 * d].float(), sd["encoder.layers.1.self_attn.k_proj.weight"])
    assert torch.equal(enc.w["1.qkv.b"][2 * d:].float(), sd["encoder.layers.1.self_attn.v_proj.bias"])
    assert enc.w["0.ln1.b"].dtype == torch.float32 and enc.w["0.fc1.b"].dtype == torch.bfloat16
    full = {PREFIX + k: v for k, v in sd.items()}            # a full CLIP checkpoint's other members
    full.update({"text_model.embeddings.position_ids": torch.arange(77)[None], "logit_scale": torch.tensor(4.6),
                 "vision_model.post_layernorm.weight": torch.ones(8), "text_projection.weight": torch.ones(4, d),
                 "visual_projection.weight": torch.ones(4, 8)})
    assert ClipTextEncoder(p, "cpu").load_state_dict(full) == ([], [])
    less = {k: v for k, v in sd.items() if k != "final_layer_norm.bias"}
    more = dict(sd, **{"encoder.layers.2.mlp.fc1.bias": torch.ones(8)})
    e3 = ClipTextEncoder(p, "cpu")
    with pytest.raises(RuntimeError):
        e3.load_state_dict(less)
    with pytest.raises(RuntimeError):
        e3.load_state_dict(more)
    assert e3.load_state_dict(less, strict=False) == (["final_layer_norm.bias"], []) and not e3.loaded
    assert e3.load_state_dict(more, strict=False) == ([], ["encoder.layers.2.mlp.fc1.bias"]) and e3.loaded
    bad = dict(sd)
    bad["encoder.layers.0.mlp.fc2.weight"] = torch.zeros(d, p.intermediate_size + 1)
    with pytest.raises(RuntimeError, match="shape"):
        ClipTextEncoder(p, "cpu").load_state_dict(bad, strict=False)
    with pytest.raises(RuntimeError):
        ClipTextEncoder(p, "cpu").encode_ids(torch.zeros(1, 77, dtype=torch.long))   # nothing loaded


def test_geometry_and_id_checks_need_no_gpu():
    with pytest.raises(ValueError):
        ClipTextEncoder(tiny_clip_params(num_attention_heads=2), "cpu")      # head dim 128
    with pytest.raises(ValueError):
        ClipTextEncoder(tiny_clip_params(intermediate_size=320), "cpu")      # not a multiple of the GEMM tile
    with pytest.raises(ValueError):
        ClipTextEncoder(tiny_clip_params(max_position_embeddings=129), "cpu")
    enc = ClipTextEncoder(tiny_clip_params(), "cpu")
    enc.load_state_dict(synthetic_clip_state_dict(enc.params, 0))
    for ids in (torch.zeros(1, 78, dtype=torch.long), torch.zeros(1, 0, dtype=torch.long), torch.zeros(77, dtype=torch.long),
                torch.full((1, 77), 512), torch.full((1, 77), -1), torch.zeros(1, 77)):
        with pytest.raises(ValueError):
            enc.encode_ids(ids)
        with pytest.raises(ValueError):
            enc.hidden_states(ids)


def test_toy_tokenizer_has_the_hf_call_contract():
    tok = ToyClipTokenizer()
    assert tok.eos_token_id == tok.pad_token_id == tok.vocab_size - 1 > tok.bos_token_id > 255      # EOS is the highest id
    out = tok(["cat", "é", ""], truncation=True, max_length=8, padding="max_length", return_tensors="pt", return_length=False)
    e, b = tok.eos_token_id, tok.bos_token_id
    assert out["input_ids"].tolist() == [[b, 99, 97, 116, e, e, e, e], [b, 0xC3, 0xA9, e, e, e, e, e], [b, e, e, e, e, e, e, e]]
    assert out["input_ids"].dtype == torch.long
    empty = tok("")["input_ids"]                                              # the default length is CLIP's 77
    assert tuple(empty.shape) == (1, 77) and empty[0, :2].tolist() == [b, e] and (empty[0, 2:] == e).all()
    assert pooled_positions(empty, 2).tolist() == [1] == pooled_positions(empty, e).tolist()
    long = tok("x" * 200)["input_ids"]                                        # truncated at 77, still terminated
    assert tuple(long.shape) == (1, 77) and long[0, 0] == b and long[0, 76] == e and (long[0, 1:76] == ord("x")).all()
    assert pooled_positions(long, 2).tolist() == [76]
    assert int(tok("\xff" * 3, max_length=8)["input_ids"].max()) < tok.vocab_size


class _StubEncoder:
    device = torch.device("cpu")
    params = tiny_clip_params()

    def __init__(self):
        self.calls = []

    def encode_ids(self, ids):
        self.calls.append(ids.clone())
        return ids[:, :4].to(torch.bfloat16)


def test_embedder_cuts_and_pads_what_the_tokenizer_returns_and_plugs_into_the_text_encoder():
    seen = {}

    def tokenizer(texts, **kw):       # an HF-shaped callable that ignores max_length
        seen.update(kw, texts=texts)
        return {"input_ids": torch.arange(100)[None].repeat(len(texts), 1)}
    stub = _StubEncoder()
    emb = HipClipEmbedder(stub, tokenizer, max_length=77)
    ids = emb.token_ids(["a", "b"])
    assert tuple(ids.shape) == (2, 77) and ids[1].tolist() == list(range(77)) and ids.dtype == torch.long
    assert seen["max_length"] == 77 and seen["padding"] == "max_length" and seen["truncation"] is True
    assert seen["return_tensors"] == "pt" and seen["texts"] == ["a", "b"]
    short = HipClipEmbedder(stub, ToyClipTokenizer(), max_length=16)
    assert short.token_ids([""])[0].tolist() == [256] + [257] * 15
    padded = HipClipEmbedder(stub, type("T", (), {"pad_token_id": 9, "__call__": lambda s, t, **k: {"input_ids": [[5, 6]]}})(), 8)
    assert padded.token_ids(["x"])[0].tolist() == [5, 6, 9, 9, 9, 9, 9, 9]
    with pytest.raises(ValueError):
        HipClipEmbedder(stub, lambda t, **k: {"input_ids": [[5, 6]]}, 8).token_ids(["x"])      # too short, no pad id
    with pytest.raises(ValueError):
        HipClipEmbedder(stub, tokenizer, max_length=78)
    assert tuple(emb.clip("a").shape) == (1, 4) and tuple(emb.clip_many(["a", "b", "c"]).shape) == (3, 4)
    assert len(stub.calls) == 2
    from conceptattention_amd.t5 import HipTextEncoder
    from conceptattention_amd.params import tiny_t5_params
    t5 = type("E", (), {"device": torch.device("cpu"), "params": tiny_t5_params()})()
    te = HipTextEncoder(t5, lambda t, **k: None, max_length=64, clip=emb)          # the embedder object itself
    assert te.clip_embedder is emb and tuple(te.clip("a").shape) == (1, 4)
    te = HipTextEncoder(t5, lambda t, **k: None, max_length=64, clip=lambda s: "clip:" + s)   # a bare callable, as before
    assert te.clip_embedder is None and te.clip("x") == "clip:x"


def test_unknown_text_encoder_names_are_rejected_with_both_names_in_the_text():
    import inspect
    from conceptattention_amd import image_generator
    src = inspect.getsource(image_generator.FluxGenerator.__init__)
    assert '"synthetic-t5", "synthetic-t5-clip"' in src and "unknown name" in src
