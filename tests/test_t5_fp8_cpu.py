"""CPU checks of the host side of the T5 encoder's fp8 mode: precision and projection-name validation, e4m3fn checkpoint
tensors recognised one by one with their bytes reaching the packed operands, the refusal of per-tensor-scaled files, a
safetensors round trip, and the keyword plumbing.  No GPU: the encoders here are built on the CPU device and never run a
kernel (an e4m3 tensor is packed without one; any other tensor of an fp8 projection needs the quantiser, hence a GPU)."""
import pytest
import torch

import t5_fp8_cases as F
from conceptattention_amd.image_generator import ConceptCache
from conceptattention_amd.params import tiny_t5_params
from conceptattention_amd.t5 import (FP8_PROJECTIONS, HipTextEncoder, T5Encoder, ToyByteTokenizer, load_t5,
                                     synthetic_t5_state_dict)

E4M3 = torch.float8_e4m3fn


def _sd(p=None, seed=0):
    p = p or tiny_t5_params()
    return p, synthetic_t5_state_dict(p, seed)


def test_precision_and_projection_names_are_validated():
    p = tiny_t5_params()
    assert FP8_PROJECTIONS == ("qkv", "o", "wi", "wo")
    enc = T5Encoder(p, "cpu")
    assert enc.precision == "bf16" and enc.fp8 == frozenset()
    assert T5Encoder(p, "cpu", precision="bf16", fp8_projections=("o",)).fp8 == frozenset()     # the list needs fp8 mode
    assert T5Encoder(p, "cpu", precision="fp8").fp8 == frozenset(FP8_PROJECTIONS)
    assert T5Encoder(p, "cpu", precision="fp8", fp8_projections=["qkv", "o", "wi"]).fp8 == {"qkv", "o", "wi"}
    for bad in ("fp16", "FP8", "", None, "e4m3"):
        with pytest.raises(ValueError, match="precision"):
            T5Encoder(p, "cpu", precision=bad)
        with pytest.raises(ValueError, match="precision"):
            load_t5(p, "cpu", precision=bad)
    for bad in ((), [], ("q",), ("qkv", "w0"), ("qkv", ""), "qk"):
        for precision in ("bf16", "fp8"):
            with pytest.raises(ValueError, match="fp8_projections"):
                T5Encoder(p, "cpu", precision=precision, fp8_projections=bad)
        with pytest.raises(ValueError, match="fp8_projections"):
            load_t5(p, "cpu", precision="fp8", fp8_projections=bad)


def test_an_e4m3_state_dict_is_recognised_tensor_by_tensor_and_its_bytes_reach_the_packed_operands():
    p, sd = _sd()
    sd8 = F.e4m3_state_dict(sd)
    proj = [k for k in sd if k.endswith(F.PROJECTION_KEYS)]
    assert len(proj) == 7 * p.num_layers and all(sd8[k].dtype == E4M3 for k in proj)
    enc = T5Encoder(p, "cpu", precision="fp8")
    assert enc.load_state_dict(sd8) == ([], []) and enc.loaded and enc.e4m3 == set(proj)
    for k in proj:                                   # the host copy is the exact widening
        assert torch.equal(enc.tensors[k], sd8[k].float())
    by = lambda k: sd8[k].view(torch.uint8)   # noqa: E731
    for i in range(p.num_layers):
        a, f = f"encoder.block.{i}.layer.0.SelfAttention", f"encoder.block.{i}.layer.1.DenseReluDense"
        want = {"qkv": torch.cat([by(f"{a}.{n}.weight") for n in "qkv"]), "o": by(f"{a}.o.weight"),
                "wi": torch.cat([by(f"{f}.wi_1.weight"), by(f"{f}.wi_0.weight")]), "wo": by(f"{f}.wo.weight")}
        for name, b in want.items():
            w, s = enc.w[f"{i}.{name}"], enc.w[f"{i}.{name}.scale"]
            assert w.dtype == torch.uint8 and torch.equal(w, b), (i, name)          # byte for byte
            assert s.dtype == torch.float32 and tuple(s.shape) == (b.shape[0],) and bool((s == 1).all())
    assert enc.w["shared"].dtype == torch.bfloat16 and enc.w["0.ln0"].dtype == torch.float32    # unchanged
    # a mixed checkpoint: only o arrives as e4m3 and only o is an fp8 projection -> still no kernel needed
    mixed = dict(sd)
    for i in range(p.num_layers):
        k = f"encoder.block.{i}.layer.0.SelfAttention.o.weight"
        mixed[k] = sd8[k]
    e2 = T5Encoder(p, "cpu", precision="fp8", fp8_projections=("o",))
    e2.load_state_dict(mixed)
    assert e2.e4m3 == {f"encoder.block.{i}.layer.0.SelfAttention.o.weight" for i in range(p.num_layers)}
    assert e2.w["0.o"].dtype == torch.uint8 and "0.o.scale" in e2.w
    assert e2.w["0.qkv"].dtype == torch.bfloat16 and "0.qkv.scale" not in e2.w
    # loading fp32 tensors over e4m3 ones forgets the mark
    e2.load_state_dict(sd8)
    assert len(e2.e4m3) == 7 * p.num_layers
    e3 = T5Encoder(p, "cpu")
    e3.load_state_dict(sd8)
    e3.load_state_dict(sd)
    assert e3.e4m3 == set()


def test_e4m3_weights_in_bf16_mode_are_widened_exactly():
    p, sd = _sd()
    sd8 = F.e4m3_state_dict(sd)
    a, b = T5Encoder(p, "cpu"), T5Encoder(p, "cpu")
    a.load_state_dict(sd8)
    b.load_state_dict({k: v.float() for k, v in sd8.items()})
    assert set(a.w) == set(b.w) and all(a.w[k].dtype == b.w[k].dtype and torch.equal(a.w[k], b.w[k]) for k in a.w)
    assert a.w["0.qkv"].dtype == torch.bfloat16 and not any(k.endswith(".scale") for k in a.w)
    assert a.weight_bytes() == b.weight_bytes() > a.weight_bytes(embedding=False) > 0


def test_weight_bytes_of_the_fp8_operands_are_about_half():
    p, sd = _sd()
    sd8 = F.e4m3_state_dict(sd)
    bf, f8 = T5Encoder(p, "cpu"), T5Encoder(p, "cpu", precision="fp8")
    bf.load_state_dict(sd8), f8.load_state_dict(sd8)
    assert f8.weight_bytes(embedding=False) < 0.55 * bf.weight_bytes(embedding=False)
    assert bf.weight_bytes() - bf.weight_bytes(False) == f8.weight_bytes() - f8.weight_bytes(False) == p.vocab_size * p.d_model * 2


@pytest.mark.parametrize("suffix", [".scale_weight", ".weight_scale"])
def test_per_tensor_scale_keys_next_to_e4m3_weights_are_refused_in_fp8_mode(suffix):
    p, sd = _sd()
    sd8 = F.e4m3_state_dict(sd)
    key = "encoder.block.1.layer.1.DenseReluDense.wo" + suffix
    scaled = dict(sd8, **{key: torch.tensor(0.5)})
    for strict in (True, False):
        with pytest.raises(RuntimeError, match=key.replace(".", r"\.")):
            T5Encoder(p, "cpu", precision="fp8").load_state_dict(scaled, strict=strict)
    with pytest.raises(RuntimeError, match=key.replace(".", r"\.")):
        load_t5(p, "cpu", weights=scaled, precision="fp8")
    # bf16 mode: an unexpected key like any other
    with pytest.raises(RuntimeError):
        T5Encoder(p, "cpu").load_state_dict(scaled)
    assert T5Encoder(p, "cpu").load_state_dict(scaled, strict=False) == ([], [key])


def test_safetensors_round_trip_keeps_e4m3_tensors_and_load_t5_reads_them(tmp_path):
    from safetensors.torch import load_file, save_file
    p, sd = _sd(tiny_t5_params(num_layers=1))
    sd8 = F.e4m3_state_dict(sd)
    path = str(tmp_path / "t5_e4m3.safetensors")
    save_file({k: v.contiguous() for k, v in sd8.items()}, path)
    back = load_file(path, device="cpu")
    for k, v in sd8.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k].view(torch.uint8) if v.dtype == E4M3 else back[k],
                                                        v.view(torch.uint8) if v.dtype == E4M3 else v), k
    enc = load_t5(p, "cpu", weights=path, precision="fp8")
    ref = T5Encoder(p, "cpu", precision="fp8")
    ref.load_state_dict(sd8)
    assert enc.e4m3 == ref.e4m3 and len(enc.e4m3) == 7
    assert all(torch.equal(enc.w[k], ref.w[k]) for k in ref.w) and set(enc.w) == set(ref.w)
    save_file({**{k: v.contiguous() for k, v in sd8.items()},
               "encoder.block.0.layer.0.SelfAttention.q.scale_weight": torch.ones(1)}, path)
    with pytest.raises(RuntimeError, match="scale_weight"):
        load_t5(p, "cpu", weights=path, precision="fp8")


def test_keywords_reach_the_encoder_and_a_cache_never_serves_two_encoders():
    from conceptattention_amd.image_generator import FluxGenerator
    from conceptattention_amd.pipeline import ConceptAttentionFluxPipeline
    import inspect
    for fn in (FluxGenerator.__init__, ConceptAttentionFluxPipeline.__init__):
        assert inspect.signature(fn).parameters["t5_precision"].default == "bf16"
    from conceptattention_amd.t5 import synthetic_text_encoder
    assert inspect.signature(synthetic_text_encoder).parameters["t5_precision"].default == "bf16"
    assert inspect.signature(load_t5).parameters["precision"].default == "bf16"
    assert inspect.signature(T5Encoder.__init__).parameters["precision"].default == "bf16"
    # ConceptCache belongs to one encoder OBJECT; an fp8 and a bf16 encoder are two objects whatever their weights
    p = tiny_t5_params()
    te_bf = HipTextEncoder(T5Encoder(p, "cpu"), ToyByteTokenizer(), 64, clip=lambda s: s)
    te_f8 = HipTextEncoder(T5Encoder(p, "cpu", precision="fp8"), ToyByteTokenizer(), 64, clip=lambda s: s)
    cache = ConceptCache()
    cache.bind(te_bf)
    cache.put("cat", torch.zeros(4))
    cache.bind(te_bf)
    assert "cat" in cache
    cache.bind(te_f8)
    assert "cat" not in cache and len(cache) == 0
    cache.put("cat", torch.ones(4))
    cache.bind(te_bf)
    assert len(cache) == 0
    assert te_f8.encoder.precision == "fp8" and te_bf.encoder.precision == "bf16"
