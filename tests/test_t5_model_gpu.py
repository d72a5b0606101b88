"""``T5Encoder`` on the GPU against the goldens made by transformers' own T5EncoderModel.

Gate (the project's usual one): relative-rms distance from the reference's fp32 output, over all kept rows and over the
token-0 rows (the concept embeddings), no larger than the distance of the reference's own bf16 run, stored in the same
golden.  Measured on an MI355X (ours / the reference's bf16 run): see README, "Text encoder"."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import t5_ref  # noqa: E402
from conceptattention_amd.params import tiny_t5_params  # noqa: E402
from conceptattention_amd.t5 import HipTextEncoder, T5Encoder, ToyByteTokenizer, load_t5, synthetic_t5_state_dict  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
_ENC = {}


def _enc(name):
    if name not in _ENC:
        p = tiny_t5_params(**t5_ref.CASES[name][0])
        enc = T5Encoder(p, DEV)
        enc.load_state_dict(synthetic_t5_state_dict(p, 0))
        _ENC[name] = enc
    return _ENC[name]


def _rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


@pytest.mark.parametrize("name", list(t5_ref.CASES))
def test_encoder_against_the_golden(name):
    g = np.load(os.path.join(GOLDEN, f"t5_{name}.npz"))
    enc = _enc(name)
    ids = torch.from_numpy(g["ids"])
    out = enc.encode_ids(ids)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (ids.shape[0], ids.shape[1], enc.params.d_model)
    got = out.float().cpu().numpy()[:, g["rows"]]
    assert np.isfinite(got).all()
    ours, ours0 = _rel_rms(got, g["out_f32"]), _rel_rms(got[:, 0], g["out_f32"][:, 0])
    ref, ref0 = g["bf16_err"]
    print(f"t5 {name}: rel-rms {ours:.3e} (reference bf16 {ref:.3e}, ratio {ours / ref:.3f}); token 0 {ours0:.3e} "
          f"(reference bf16 {ref0:.3e}, ratio {ours0 / ref0:.3f})")
    assert ours <= ref and ours0 <= ref0


def test_five_sequences_in_one_forward_equal_five_single_calls_and_a_second_call_repeats_the_bits():
    enc = _enc("tiny")
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(0, enc.params.vocab_size, (5, 256), generator=gen)
    ids[:, 20:] = 0
    both = enc.encode_ids(ids)
    ws = enc._ws
    again = enc.encode_ids(ids)
    assert enc._ws is ws and torch.equal(again, both)                  # the workspace is reused, the bits repeat
    for i in range(5):
        assert torch.equal(enc.encode_ids(ids[i:i + 1]), both[i:i + 1]), i
    assert enc._ws is ws
    assert not torch.equal(both[0], both[1])


def test_a_batch_split_into_passes_equals_one_pass_and_other_lengths_run_alone(monkeypatch):
    enc = _enc("tiny")
    gen = torch.Generator().manual_seed(4)
    ids = torch.randint(0, enc.params.vocab_size, (3, 256), generator=gen)
    one = enc.encode_ids(ids)
    monkeypatch.setattr(enc, "MAX_ROWS", 512)                          # two sequences per pass
    assert enc.sequences_per_pass(256) == 2 and torch.equal(enc.encode_ids(ids), one)
    monkeypatch.undo()
    short = torch.randint(0, enc.params.vocab_size, (3, 64), generator=gen)   # L = 64: one sequence per pass
    out = enc.encode_ids(short)
    ref = t5_ref.encoder(synthetic_t5_state_dict(enc.params, 0), short, enc.params.num_heads, enc.params.num_layers)
    assert _rel_rms(out.float().cpu().numpy(), ref.numpy()) < 1e-2
    assert torch.equal(enc.encode_ids(short[1:2]), out[1:2])


def test_safetensors_file_shard_directory_and_environment_variable_load_the_same_weights(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    p = tiny_t5_params(num_layers=1)
    sd = synthetic_t5_state_dict(p, seed=5)
    ids = t5_ref.case_ids("tiny")[:1, :64].contiguous()
    ref = load_t5(p, DEV, weights=sd).encode_ids(ids)
    path = str(tmp_path / "t5.safetensors")
    save_file(dict(sd, **{"decoder.final_layer_norm.weight": torch.ones(p.d_model)}), path)   # a full checkpoint's extras
    assert torch.equal(load_t5(p, DEV, weights=path).encode_ids(ids), ref)
    shards = tmp_path / "shards"
    shards.mkdir()
    names = list(sd)
    save_file({k: sd[k] for k in names[:5]}, str(shards / "model-00001-of-00002.safetensors"))
    save_file({k: sd[k] for k in names[5:]}, str(shards / "model-00002-of-00002.safetensors"))
    assert torch.equal(load_t5(p, DEV, weights=str(shards)).encode_ids(ids), ref)
    monkeypatch.setenv("T5", path)
    assert torch.equal(load_t5(p, DEV).encode_ids(ids), ref)
    monkeypatch.delenv("T5")
    assert not torch.equal(load_t5(p, DEV, seed=0).encode_ids(ids), ref)
    save_file({k: sd[k] for k in names[:5]}, path)
    with pytest.raises(RuntimeError):
        load_t5(p, DEV, weights=path)


def test_text_encoder_on_the_device():
    te = HipTextEncoder(_enc("tiny"), ToyByteTokenizer(), max_length=256)
    many = te.t5_many(["a cat on the grass", "cat", "grass"])
    assert tuple(many.shape) == (3, 256, 256) and many.dtype == torch.bfloat16 and torch.isfinite(many.float()).all()
    assert torch.equal(te.t5("cat"), many[1:2])
    assert tuple(te.clip("cat").shape) == (1, 768)


def test_pipeline_with_the_synthetic_t5_text_encoder():
    from conceptattention_amd import ConceptAttentionFluxPipeline, tiny_params
    from conceptattention_amd.t5 import HipTextEncoder as H
    pipe = ConceptAttentionFluxPipeline("flux-schnell", device=DEV, params=tiny_params(), n_text_tokens=64,
                                        text_encoder="synthetic-t5")
    assert isinstance(pipe.text_encoder, H) and pipe.text_encoder.encoder.params.d_model == pipe.params.context_in_dim
    kw = dict(width=128, height=128, layer_indices=[0, 1], num_inference_steps=2, return_pil_heatmaps=False)
    out = pipe.generate_image("a cat on the grass", ["cat", "grass"], **kw)
    assert out.concept_heatmaps.shape == (2, 8, 8) and np.isfinite(out.concept_heatmaps).all()
    assert np.isfinite(out.cross_attention_maps).all()
    txt, vec, con, con_ids, con_vec = pipe._embed("a cat on the grass", ["cat", "grass"])
    assert tuple(txt.shape) == (1, 64, pipe.params.context_in_dim) and tuple(con.shape) == (1, 2, pipe.params.context_in_dim)
    assert torch.isfinite(txt.float()).all()
    assert torch.equal(con[0, 0], pipe.text_encoder.t5("cat")[0, 0])            # a concept = token 0 of its own encoding
    assert torch.equal(pipe._embed("a cat on the grass", ["cat", "grass"])[0], txt)      # the same prompt: equal bits
    assert not torch.equal(pipe._embed("a dog in the snow", ["cat", "grass"])[0], txt)   # another prompt: another txt
    again = pipe.generate_image("a cat on the grass", ["cat", "grass"], **kw)
    assert np.array_equal(again.concept_heatmaps, out.concept_heatmaps)
