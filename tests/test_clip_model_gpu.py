"""``ClipTextEncoder`` on the GPU against the goldens made by transformers' own CLIPTextModel.

Gate (the project's usual one): relative-rms distance from the reference's fp32 output -- ``hidden_states`` over the kept
rows, ``encode_ids`` over the pooled rows -- no larger than the distance of the reference's own bf16 run, stored in the
same golden.  Measured on an MI355X (ours / the reference's bf16 run): see README, "Text encoder"."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_cases as T  # noqa: E402
import clip_ref  # noqa: E402
from conceptattention_amd.clip import (PREFIX, ClipTextEncoder, HipClipEmbedder, ToyClipTokenizer, load_clip,  # noqa: E402
                                       pooled_positions, synthetic_clip_state_dict)
from conceptattention_amd.params import tiny_clip_params  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
_ENC = {}


def _enc(name):
    if name not in _ENC:
        p = tiny_clip_params(**clip_ref.CASES[name][0])
        enc = ClipTextEncoder(p, DEV)
        enc.load_state_dict(synthetic_clip_state_dict(p, 0))
        _ENC[name] = enc
    return _ENC[name]


@pytest.mark.parametrize("name", list(clip_ref.CASES))
def test_encoder_against_the_golden(name):
    g = np.load(os.path.join(GOLDEN, f"clip_{name}.npz"))
    enc = _enc(name)
    ids = torch.from_numpy(g["ids"]).long()
    hidden, pooled = enc.hidden_states(ids), enc.encode_ids(ids)
    d = enc.params.hidden_size
    assert hidden.dtype == torch.bfloat16 and tuple(hidden.shape) == (ids.shape[0], ids.shape[1], d)
    assert pooled.dtype == torch.bfloat16 and tuple(pooled.shape) == (ids.shape[0], d)
    got_h, got_p = hidden.float().cpu().numpy()[:, g["rows"]], pooled.float().cpu().numpy()
    assert np.isfinite(got_h).all() and np.isfinite(got_p).all()
    ours_h, ours_p = clip_ref.rel_rms(got_h, g["hidden_f32"]), clip_ref.rel_rms(got_p, g["pooler_f32"])
    ref_h, ref_p = g["bf16_err"]
    print(f"clip {name}: hidden rel-rms {ours_h:.3e} (reference bf16 {ref_h:.3e}, ratio {ours_h / ref_h:.3f}); pooled "
          f"{ours_p:.3e} (reference bf16 {ref_p:.3e}, ratio {ours_p / ref_p:.3f})")
    assert ours_h <= ref_h and ours_p <= ref_p
    # the pooled rows are rows of the hidden states
    assert torch.equal(hidden[torch.arange(ids.shape[0]), torch.from_numpy(g["pooled"]).long()], pooled)


def test_five_sequences_in_one_call_equal_five_single_calls_and_a_second_call_repeats_the_bits():
    enc = _enc("tiny")
    ids = clip_ref.case_ids("tiny")[[0, 2, 4, 6, 7]]
    both = enc.encode_ids(ids)
    ws = enc._ws
    assert ws is not None and enc.workspace_bytes() > 0
    again = enc.encode_ids(ids)
    assert enc._ws is ws and torch.equal(again, both)                  # the workspace is reused, the bits repeat
    for i in range(5):
        assert torch.equal(enc.encode_ids(ids[i:i + 1]), both[i:i + 1]), i
    assert torch.equal(enc.encode_ids(ids.flip(0)), both.flip(0))      # nor does the order matter
    assert enc._ws is ws
    assert not torch.equal(both[0], both[1])
    hidden = enc.hidden_states(ids)
    assert enc._ws is ws
    assert torch.equal(hidden[torch.arange(5), pooled_positions(ids, enc.params.eos_token_id)], both)
    assert torch.equal(enc.hidden_states(ids[3:4]), hidden[3:4])


def test_a_short_length_runs_and_agrees_with_the_restatement():
    enc = _enc("eos")
    p = enc.params
    ids = clip_ref.case_ids("eos")[:4, :20].contiguous()
    ids[:, 19] = 511                                                    # ends with the end-of-text token, as a tokenizer's cut does
    hidden, pooled = enc.hidden_states(ids), enc.encode_ids(ids)
    with torch.no_grad():
        ref_h, ref_p = clip_ref.text_model(synthetic_clip_state_dict(p, 0), ids, p.num_attention_heads, p.num_hidden_layers,
                                           p.eos_token_id)
    eh, ep = clip_ref.rel_rms(hidden.float().cpu().numpy(), ref_h.numpy()), clip_ref.rel_rms(pooled.float().cpu().numpy(), ref_p.numpy())
    print(f"clip L=20: hidden rel-rms {eh:.3e}, pooled {ep:.3e} (bound {T.MODEL_REL_RMS:.1e})")
    assert eh <= T.MODEL_REL_RMS and ep <= T.MODEL_REL_RMS
    assert clip_ref.pooled_positions(ids, p.eos_token_id) == [1, 5, 19, 19]
    one = enc.encode_ids(ids[:1, :1])                                   # L = 1: a single key
    assert tuple(one.shape) == (1, p.hidden_size) and torch.isfinite(one.float()).all()


def test_safetensors_file_shard_directory_and_environment_variable_load_the_same_weights(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    p = tiny_clip_params(num_hidden_layers=1)
    sd = synthetic_clip_state_dict(p, seed=5)
    ids = clip_ref.case_ids("tiny")[1:3]
    ref = load_clip(p, DEV, weights=sd).encode_ids(ids)
    path = str(tmp_path / "clip.safetensors")
    full = {PREFIX + k: v for k, v in sd.items()}                        # a published checkpoint: prefixed, with the rest of CLIP
    full.update({"text_model.embeddings.position_ids": torch.arange(77)[None], "logit_scale": torch.tensor(4.6),
                 "vision_model.post_layernorm.weight": torch.ones(8), "text_projection.weight": torch.ones(4, p.hidden_size),
                 "visual_projection.weight": torch.ones(4, 8)})
    save_file(full, path)
    assert torch.equal(load_clip(p, DEV, weights=path).encode_ids(ids), ref)
    shards = tmp_path / "shards"
    shards.mkdir()
    names = list(sd)
    save_file({k: sd[k] for k in names[:5]}, str(shards / "model-00001-of-00002.safetensors"))
    save_file({PREFIX + k: sd[k] for k in names[5:]}, str(shards / "model-00002-of-00002.safetensors"))
    assert torch.equal(load_clip(p, DEV, weights=str(shards)).encode_ids(ids), ref)
    monkeypatch.setenv("CLIP", path)
    assert torch.equal(load_clip(p, DEV).encode_ids(ids), ref)
    monkeypatch.delenv("CLIP")
    assert not torch.equal(load_clip(p, DEV, seed=0).encode_ids(ids), ref)
    save_file({k: sd[k] for k in names[:5]}, path)
    with pytest.raises(RuntimeError):
        load_clip(p, DEV, weights=path)


def test_embedder_on_the_device():
    emb = HipClipEmbedder(_enc("tiny"), ToyClipTokenizer(), max_length=77)
    many = emb.clip_many(["a cat on the grass", "cat", ""])
    assert tuple(many.shape) == (3, 256) and many.dtype == torch.bfloat16 and torch.isfinite(many.float()).all()
    assert torch.equal(emb.clip("cat"), many[1:2]) and torch.equal(emb.clip(""), many[2:3])
    assert not torch.equal(many[0], many[1])


def test_pipeline_with_the_synthetic_t5_and_clip_text_encoders():
    from conceptattention_amd import ConceptAttentionFluxPipeline, tiny_params
    from conceptattention_amd.t5 import HipTextEncoder
    pipe = ConceptAttentionFluxPipeline("flux-schnell", device=DEV, params=tiny_params(), n_text_tokens=64,
                                        text_encoder="synthetic-t5-clip")
    te = pipe.text_encoder
    assert isinstance(te, HipTextEncoder) and isinstance(te.clip_embedder, HipClipEmbedder)
    clip = te.clip_embedder
    assert clip.encoder.params.hidden_size == pipe.params.vec_in_dim and clip.encoder.params.num_hidden_layers == 2
    assert clip.max_length == 77 and isinstance(clip.tokenizer, ToyClipTokenizer)
    prompt = "a cat on the grass"
    txt, vec, con, con_ids, con_vec = pipe._embed(prompt, ["cat", "grass"])
    assert tuple(vec.shape) == (1, pipe.params.vec_in_dim) and vec.dtype == torch.bfloat16 and torch.isfinite(vec.float()).all()
    assert torch.equal(pipe._embed(prompt, ["cat", "grass"])[1], vec)                       # the same prompt: equal bits
    assert not torch.equal(pipe._embed("a dog in the snow", ["cat", "grass"])[1], vec)      # another prompt: another vec
    ids = clip.tokenizer([prompt], max_length=77)["input_ids"]
    assert torch.equal(vec, clip.encoder.encode_ids(ids))
    assert pooled_positions(ids, clip.encoder.params.eos_token_id).tolist() == [1 + len(prompt)]
    empty = te.clip("")                                                                     # restrict_clip_guidance's string
    assert tuple(empty.shape) == (1, pipe.params.vec_in_dim) and torch.isfinite(empty.float()).all()
    assert pooled_positions(clip.token_ids([""]), clip.encoder.params.eos_token_id).tolist() == [1]
    kw = dict(width=128, height=128, layer_indices=[0, 1], num_inference_steps=2, return_pil_heatmaps=False)
    out = pipe.generate_image(prompt, ["cat", "grass"], **kw)
    assert out.concept_heatmaps.shape == (2, 8, 8) and np.isfinite(out.concept_heatmaps).all()
    again = pipe.generate_image(prompt, ["cat", "grass"], **kw)
    assert np.array_equal(again.concept_heatmaps, out.concept_heatmaps)
    img, maps = pipe.flux_generator.generate_image(128, 128, 2, 0.0, 0, prompt, ["cat", "grass"], restrict_clip_guidance=True)
    assert np.isfinite(np.asarray(img, dtype=np.float64)).all()
    with pytest.raises(ValueError, match="synthetic-t5-clip"):
        ConceptAttentionFluxPipeline("flux-schnell", device=DEV, params=tiny_params(), n_text_tokens=64, text_encoder="clip")
