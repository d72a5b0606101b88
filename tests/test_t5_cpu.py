"""CPU checks of the T5 encoder's host side: the fp64 restatement against the goldens transformers made, the state-dict
layout, the bias table, the real geometry, load_state_dict semantics, the text front end and FluxGenerator.embed's two
routes.  No GPU: the encoder objects here are built on the CPU device and never run a kernel."""
import os

import numpy as np
import pytest
import torch

import t5_ref
from conceptattention_amd.params import T5_TOKENS, T5Params, t5_params, tiny_t5_params
from conceptattention_amd.t5 import (TIED_EMBEDDING, HipTextEncoder, T5Encoder, ToyByteTokenizer, relative_bias_table,
                                     relative_position_bucket, synthetic_t5_state_dict, t5_state_dict_spec)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _case(name):
    geo, length, real = t5_ref.CASES[name]
    return tiny_t5_params(**geo), length, np.load(os.path.join(GOLDEN, f"t5_{name}.npz"))


@pytest.mark.parametrize("name", list(t5_ref.CASES))
def test_restatement_matches_the_golden(name):
    """2e-5 is the autoencoder restatement's margin; measured here: 7.7e-6 (tiny), 5.9e-6 (long) max-abs on outputs of
    magnitude <= 3.6, i.e. transformers' fp32 accumulation needs no more."""
    p, length, g = _case(name)
    ids = t5_ref.case_ids(name)
    assert np.array_equal(ids.numpy(), g["ids"])
    assert list(g["rows"]) == t5_ref.kept_rows(length) and g["rows"][0] == 0
    with torch.no_grad():
        out = t5_ref.encoder(synthetic_t5_state_dict(p, 0), ids, p.num_heads, p.num_layers)
    assert tuple(out.shape) == (ids.shape[0], length, p.d_model)
    assert np.abs(out[:, g["rows"]].numpy() - g["out_f32"]).max() <= 2e-5
    assert 1e-3 < g["bf16_err"][0] < 2e-2 and 1e-3 < g["bf16_err"][1] < 2e-2     # the reference's own bf16 run


def test_ids_are_padded_sequences_with_few_real_tokens():
    geo, length, real = t5_ref.CASES["tiny"]
    ids = t5_ref.case_ids("tiny")
    assert tuple(ids.shape) == (3, 256) and real == (7, 3, 2)
    for r, n in enumerate(real):
        assert (ids[r, :n] != 0).all() and (ids[r, n:] == 0).all() and ids[r, n - 1] == 1


@pytest.mark.parametrize("name", list(t5_ref.CASES))
def test_spec_equals_the_goldens_keys_and_shapes(name):
    p, _, g = _case(name)
    theirs = {k: tuple(int(x) for x in s.split(",")) for k, s in zip(g["keys"], g["shapes"])}
    ours = dict(t5_state_dict_spec(p))
    assert theirs.pop(TIED_EMBEDDING) == ours["shared.weight"]      # the tied twin transformers lists as well
    assert theirs == ours
    assert list(synthetic_t5_state_dict(p, 0)) == [k for k, _ in t5_state_dict_spec(p)]


def test_bucket_and_bias_table_equal_transformers_at_all_1023_offsets():
    _, _, g = _case("tiny")
    off = torch.arange(-511, 512)
    ours = relative_position_bucket(off)
    assert np.array_equal(ours.numpy(), g["buckets"])
    assert [t5_ref.bucket_exact(int(o)) for o in off] == list(g["buckets"])     # fp32 log == exact arithmetic here
    assert ours.min() == 0 and ours.max() == 31 and ours[511] == 0 and ours[511 + 1] == 17 and ours[511 - 1] == 1
    assert ours[511 + 90] == 30 and ours[511 + 91] == 31 and ours[511 + 128] == 31 and ours[0] == 15   # last bucket: 8 * 16^(7/8) = 90.5 on
    w = torch.arange(32 * 4, dtype=torch.float32).reshape(32, 4)
    tab = relative_bias_table(w, 512)
    assert tuple(tab.shape) == (4, 1023) and tab.dtype == torch.float32
    assert torch.equal(tab, w[torch.from_numpy(g["buckets"]).long()].t())
    assert torch.equal(relative_bias_table(w, 256), tab[:, 256:1023 - 256])      # a shorter table is the middle
    assert torch.equal(tab.double(), t5_ref.bias_table(w.double(), 512))


def test_real_geometry_is_t5_v1_1_xxl():
    p = t5_params["t5-v1_1-xxl"]
    assert p == T5Params()
    assert (p.num_layers, p.d_model, p.num_heads, p.d_kv, p.d_ff) == (24, 4096, 64, 64, 10240)
    assert (p.relative_attention_num_buckets, p.relative_attention_max_distance, p.layer_norm_epsilon) == (32, 128, 1e-6)
    assert p.vocab_size == 32128 and p.inner_dim == 4096
    spec = dict(t5_state_dict_spec(p))
    assert len(spec) == 1 + 24 * 9 + 1 + 1 and not any(k.endswith(".bias") for k in spec)
    assert sum(int(np.prod(s)) for s in spec.values()) == 4_762_310_656       # the encoder's parameter count
    assert spec["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"] == (32, 64)
    assert "encoder.block.1.layer.0.SelfAttention.relative_attention_bias.weight" not in spec
    assert T5_TOKENS == {"flux-schnell": 256, "flux-dev": 512}
    T5Encoder(p, "cpu")                                                       # the geometry meets the kernels' rules


def test_synthetic_weights_are_bf16_values_with_the_stated_scales():
    p = tiny_t5_params()
    sd = synthetic_t5_state_dict(p, 0)
    for k, v in sd.items():
        assert v.dtype == torch.float32 and torch.equal(v, v.to(torch.bfloat16).float()), k
    rb = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    assert rb.max() > 3 and rb.min() < -3 and rb.abs().max() <= 4                     # several nats
    q = sd["encoder.block.0.layer.0.SelfAttention.q.weight"]
    assert abs(float(q.std()) - (0.25 / p.d_model) ** 0.5) < 0.1 * (0.25 / p.d_model) ** 0.5
    assert not torch.equal(sd["shared.weight"], synthetic_t5_state_dict(p, 1)["shared.weight"])
    assert torch.equal(sd["shared.weight"], synthetic_t5_state_dict(p, 0)["shared.weight"])


def test_load_state_dict_tied_key_missing_unexpected_and_wrong_shape():
    p = tiny_t5_params()
    sd = synthetic_t5_state_dict(p, 0)
    enc = T5Encoder(p, "cpu")
    assert enc.load_state_dict(sd) == ([], []) and enc.loaded
    assert enc.w["0.qkv"].shape == (3 * p.inner_dim, p.d_model) and enc.w["0.qkv"].dtype == torch.bfloat16
    assert enc.w["1.wi"].shape == (2 * p.d_ff, p.d_model)
    assert torch.equal(enc.w["1.wi"][: p.d_ff].float(), sd["encoder.block.1.layer.1.DenseReluDense.wi_1.weight"])
    assert torch.equal(enc.bias_table(256), relative_bias_table(
        sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], 256))
    tied = dict(sd)
    tied[TIED_EMBEDDING] = tied.pop("shared.weight")                           # only the twin
    e2 = T5Encoder(p, "cpu")
    assert e2.load_state_dict(tied) == ([], []) and torch.equal(e2.w["shared"], enc.w["shared"])
    both = dict(sd)
    both[TIED_EMBEDDING] = sd["shared.weight"]
    assert T5Encoder(p, "cpu").load_state_dict(both) == ([], [])
    less = {k: v for k, v in sd.items() if k != "encoder.final_layer_norm.weight"}
    more = dict(sd, **{"decoder.final_layer_norm.weight": torch.ones(p.d_model)})
    e3 = T5Encoder(p, "cpu")
    with pytest.raises(RuntimeError):
        e3.load_state_dict(less)
    with pytest.raises(RuntimeError):
        e3.load_state_dict(more)
    assert e3.load_state_dict(less, strict=False) == (["encoder.final_layer_norm.weight"], []) and not e3.loaded
    assert e3.load_state_dict(more, strict=False) == ([], ["decoder.final_layer_norm.weight"]) and e3.loaded
    bad = dict(sd)
    bad["encoder.block.0.layer.0.SelfAttention.o.weight"] = torch.zeros(p.d_model, p.inner_dim + 1)
    with pytest.raises(RuntimeError, match="shape"):
        T5Encoder(p, "cpu").load_state_dict(bad, strict=False)
    with pytest.raises(RuntimeError):
        T5Encoder(p, "cpu").encode_ids(torch.zeros(1, 64, dtype=torch.long))   # nothing loaded


def test_geometry_and_id_checks_need_no_gpu():
    with pytest.raises(ValueError):
        T5Encoder(tiny_t5_params(d_kv=128), "cpu")
    with pytest.raises(ValueError):
        T5Encoder(tiny_t5_params(d_ff=320), "cpu")          # not a multiple of the SPLIT_GELU tile
    enc = T5Encoder(tiny_t5_params(), "cpu")
    enc.load_state_dict(synthetic_t5_state_dict(enc.params, 0))
    for ids in (torch.zeros(1, 96, dtype=torch.long), torch.zeros(1, 576, dtype=torch.long), torch.zeros(64, dtype=torch.long),
                torch.full((1, 64), 512), torch.full((1, 64), -1), torch.zeros(1, 64)):
        with pytest.raises(ValueError):
            enc.encode_ids(ids)
    assert enc.sequences_per_pass(256) == 32 and enc.sequences_per_pass(512) == 16 and enc.sequences_per_pass(192) == 1


class _StubEncoder:
    device = torch.device("cpu")
    params = tiny_t5_params()

    def __init__(self):
        self.calls = []

    def encode_ids(self, ids):
        self.calls.append(ids.clone())
        return ids[..., None].expand(*ids.shape, 4).to(torch.bfloat16)


def test_text_encoder_pads_and_truncates_to_max_length_with_a_stub_tokenizer():
    seen = {}

    def tokenizer(texts, **kw):       # an HF-shaped callable that ignores max_length: 3 and 100 tokens
        seen.update(kw, texts=texts)
        return {"input_ids": torch.tensor([[5, 6, 1] + [0] * 97, list(range(2, 101)) + [1]][: len(texts)])}
    stub = _StubEncoder()
    te = HipTextEncoder(stub, tokenizer, max_length=64, clip=lambda s: "clip:" + s)
    ids = te.token_ids(["a", "b"])
    assert tuple(ids.shape) == (2, 64) and ids.dtype == torch.long
    assert ids[0].tolist() == [5, 6, 1] + [0] * 61 and ids[1].tolist() == list(range(2, 66))
    assert seen["max_length"] == 64 and seen["padding"] == "max_length" and seen["truncation"] is True
    assert seen["return_tensors"] == "pt" and seen["texts"] == ["a", "b"]
    short = HipTextEncoder(stub, lambda texts, **kw: {"input_ids": [[7, 1]]}, max_length=128)
    assert short.token_ids(["x"])[0].tolist() == [7, 1] + [0] * 126                       # padded up
    assert tuple(te.t5("a").shape) == (1, 64, 4) and tuple(te.t5_many(["a", "b"]).shape) == (2, 64, 4)
    assert len(stub.calls) == 2 and te.clip("x") == "clip:x"
    with pytest.raises(ValueError):
        HipTextEncoder(stub, tokenizer, max_length=100)
    v = short.clip("a cat")                                                               # the stand-in, keyed by the text
    assert tuple(v.shape) == (1, 768) and torch.equal(v, short.clip("a cat")) and not torch.equal(v, short.clip("a dog"))


def test_toy_tokenizer_is_deterministic_and_has_the_hf_call_contract():
    tok = ToyByteTokenizer()
    out = tok(["cat", "é"], truncation=True, max_length=8, padding="max_length", return_tensors="pt", return_length=False)
    assert out["input_ids"].tolist() == [[3 + 99, 3 + 97, 3 + 116, 1, 0, 0, 0, 0], [3 + 0xC3, 3 + 0xA9, 1, 0, 0, 0, 0, 0]]
    assert tok("abcdefghijkl", max_length=4)["input_ids"].tolist() == [[100, 101, 102, 1]]   # truncated, still terminated
    assert int(tok("\xff" * 3, max_length=8)["input_ids"].max()) < tok.vocab_size


class _Counting:
    def __init__(self, many):
        self.t5_calls, self.many_calls = [], []
        if many:
            self.t5_many = self._many

    def _emb(self, text):
        return torch.full((1, 4, 6), float(len(text)))

    def t5(self, text):
        self.t5_calls.append(text)
        return self._emb(text)

    def _many(self, texts):
        self.many_calls.append(list(texts))
        return torch.cat([self._emb(t) for t in texts])

    def clip(self, text):
        return torch.zeros(1, 3)


@pytest.mark.parametrize("many", [True, False])
def test_embed_takes_the_one_call_route_with_t5_many_and_the_old_route_without(many):
    from conceptattention_amd.image_generator import FluxGenerator
    gen = FluxGenerator.__new__(FluxGenerator)          # embed() alone: no model, no device
    enc = _Counting(many)
    gen.text_encoder, gen.t5, gen.clip = enc, enc.t5, enc.clip
    txt, vec, con, con_ids, con_vec = gen.embed("a prompt", ["cat", "grass"])
    if many:
        assert enc.many_calls == [["a prompt", "cat", "grass"]] and enc.t5_calls == []
    else:
        assert enc.t5_calls == ["a prompt", "cat", "grass"] and enc.many_calls == []
    assert tuple(txt.shape) == (1, 4, 6) and float(txt[0, 0, 0]) == 8.0
    assert tuple(con.shape) == (1, 2, 6) and con[0, :, 0].tolist() == [3.0, 5.0]
    assert tuple(con_ids.shape) == (1, 2, 3) and not con_vec.any()
