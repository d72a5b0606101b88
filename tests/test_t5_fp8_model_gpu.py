"""``T5Encoder(precision="fp8")`` on the GPU against the goldens made by transformers' own T5EncoderModel
(tests/golden/t5_tiny.npz: L = 256, two blocks; t5_long.npz: L = 512, one block; reference ``out_f32``).

(a) The parity gate fixes no tolerance in advance.  The yardstick is ``t5_fp8_cases.encoder_fp8_emulated``: the fp64
restatement with the fp8 mode's quantisation points (weight rows and the activation rows in front of qkv, o, wi, wo
through torch's float8_e4m3fn cast under the kernels' scale rule) and exact arithmetic between them.  The GPU's
relative-rms distance from the golden may be at most 1.5 x the emulation's (the project's usual margin; fp32
accumulation order and the bf16 roundings between the quantisation points flip individual e4m3 roundings).

Measured on an MI355X, relative rms against ``out_f32`` (all kept rows / token-0 rows), synthetic weights:

                         GPU fp8              emulated fp8         our bf16             transformers' bf16
  tiny (L 256, 2 blocks) 5.85e-2 / 5.87e-2    5.76e-2 / 5.80e-2    3.93e-3 / 3.84e-3    6.34e-3 / 6.25e-3
  long (L 512, 1 block)  4.42e-2 / 4.53e-2    4.41e-2 / 4.54e-2    3.32e-3 / 3.07e-3    4.82e-3 / 5.02e-3

GPU / emulation: 1.016 / 1.014 (tiny), 1.003 / 0.998 (long).  That is 13 to 15 times the bf16 path: what three mantissa
bits on both operands of every projection give.  With ``wo`` kept in bf16 (tiny): 5.27e-2 / 5.32e-2.  Weight bytes of
the tiny geometry without the embedding: 1335296 against 2627584 (0.508).  Real-weight accuracy is unmeasured."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import t5_fp8_cases as F  # noqa: E402
import t5_ref  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from conceptattention_amd.params import tiny_t5_params  # noqa: E402
from conceptattention_amd.t5 import FP8_PROJECTIONS, T5Encoder, load_t5, synthetic_t5_state_dict  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
MARGIN = 1.5
_ENC, _EMU = {}, {}


def _params(name):
    return tiny_t5_params(**t5_ref.CASES[name][0])


def _enc(name, precision="fp8", projections=FP8_PROJECTIONS):
    key = (name, precision, tuple(projections))
    if key not in _ENC:
        p = _params(name)
        _ENC[key] = load_t5(p, DEV, weights=synthetic_t5_state_dict(p, 0), precision=precision, fp8_projections=projections)
    return _ENC[key]


def _rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


def _errors(got, g):
    """(all kept rows, token-0 rows) relative rms of [n_seq, kept rows, d_model] against the golden."""
    return _rel_rms(got, g["out_f32"]), _rel_rms(got[:, 0], g["out_f32"][:, 0])


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"t5_{name}.npz"))


def _emulation_errors(name):
    if name not in _EMU:     # computed once per golden, on the CPU in fp64
        g, p = _golden(name), _params(name)
        out = F.encoder_fp8_emulated(synthetic_t5_state_dict(p, 0), torch.from_numpy(g["ids"]), p.num_heads, p.num_layers)
        _EMU[name] = _errors(out.numpy()[:, g["rows"]], g)
    return _EMU[name]


def _gpu_errors(name, precision="fp8", projections=FP8_PROJECTIONS):
    g = _golden(name)
    out = _enc(name, precision, projections).encode_ids(torch.from_numpy(g["ids"]))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (*g["ids"].shape, _params(name).d_model)
    got = out.float().cpu().numpy()[:, g["rows"]]
    assert np.isfinite(got).all()
    return _errors(got, g)


@pytest.mark.parametrize("name", list(t5_ref.CASES))
def test_a_parity_with_the_golden_within_the_margin_of_the_emulated_fp8_forward(name):
    gpu, emu, bf = _gpu_errors(name), _emulation_errors(name), _gpu_errors(name, "bf16")
    ref = tuple(_golden(name)["bf16_err"])
    for what, i in (("all rows", 0), ("token 0", 1)):
        print(f"t5 fp8 {name} {what}: GPU fp8 {gpu[i]:.3e}, emulated fp8 {emu[i]:.3e} (ratio {gpu[i] / emu[i]:.3f}), "
              f"our bf16 {bf[i]:.3e}, transformers bf16 {ref[i]:.3e}")
    assert gpu[0] <= MARGIN * emu[0] and gpu[1] <= MARGIN * emu[1], (gpu, emu)


def test_b_five_sequences_in_one_forward_equal_five_single_calls_and_a_second_call_repeats_the_bits():
    enc = _enc("tiny")
    ids = torch.randint(0, enc.params.vocab_size, (5, 256), generator=torch.Generator().manual_seed(3))
    ids[:, 20:] = 0
    both = enc.encode_ids(ids)
    ws = enc._ws
    assert torch.equal(enc.encode_ids(ids), both) and enc._ws is ws
    for i in range(5):
        assert torch.equal(enc.encode_ids(ids[i:i + 1]), both[i:i + 1]), i
    assert not torch.equal(both[0], both[1])
    assert "hn" not in ws and {"hn8", "hn8.scale", "ao8", "ao8.scale", "p8", "p8.scale"} <= set(ws)   # the fp8 planes
    assert ws["hn8"].dtype == torch.uint8 and ws["p8"].shape[1] == enc.params.d_ff


def _set_operands(enc, sd8):
    """Overwrite the packed fp8 operands of ``enc`` with the e4m3 bytes of ``sd8`` and unit scales."""
    by = lambda k: sd8[k].view(torch.uint8).to(DEV)   # noqa: E731
    for i in range(enc.params.num_layers):
        a, f = f"encoder.block.{i}.layer.0.SelfAttention", f"encoder.block.{i}.layer.1.DenseReluDense"
        for name, b in (("qkv", torch.cat([by(f"{a}.{n}.weight") for n in "qkv"])), ("o", by(f"{a}.o.weight")),
                        ("wi", torch.cat([by(f"{f}.wi_1.weight"), by(f"{f}.wi_0.weight")])), ("wo", by(f"{f}.wo.weight"))):
            assert enc.w[f"{i}.{name}"].shape == b.shape and enc.w[f"{i}.{name}"].dtype == torch.uint8
            enc.w[f"{i}.{name}"] = b.contiguous()
            enc.w[f"{i}.{name}.scale"] = torch.ones(b.shape[0], device=DEV)


def test_c_an_e4m3_checkpoint_in_fp8_mode_runs_on_its_own_bytes_with_unit_scales():
    p = _params("tiny")
    sd = synthetic_t5_state_dict(p, 0)
    sd8 = F.e4m3_state_dict(sd)
    ids = t5_ref.case_ids("tiny")
    loaded = load_t5(p, DEV, weights=sd8, precision="fp8")
    by_hand = load_t5(p, DEV, weights={k: v.float() for k, v in sd8.items()}, precision="fp8")   # re-quantised ...
    assert not bool((by_hand.w["0.qkv.scale"] == 1).all())
    _set_operands(by_hand, sd8)                                                                  # ... then overwritten
    out = loaded.encode_ids(ids)
    assert torch.equal(out, by_hand.encode_ids(ids)) and torch.isfinite(out.float()).all()
    assert all(bool((loaded.w[f"{i}.{n}.scale"] == 1).all()) for i in range(p.num_layers) for n in FP8_PROJECTIONS)


def test_d_an_e4m3_checkpoint_in_bf16_mode_equals_its_widened_fp32_values():
    p = _params("tiny")
    sd8 = F.e4m3_state_dict(synthetic_t5_state_dict(p, 0))
    ids = t5_ref.case_ids("tiny")
    a = load_t5(p, DEV, weights=sd8).encode_ids(ids)
    b = load_t5(p, DEV, weights={k: v.float() for k, v in sd8.items()}).encode_ids(ids)
    assert torch.equal(a, b) and torch.isfinite(a.float()).all()


def test_e_a_partial_projection_list_runs_and_is_no_worse_than_all_four():
    part = ("qkv", "o", "wi")
    enc = _enc("tiny", "fp8", part)
    some, full = _gpu_errors("tiny", "fp8", part), _gpu_errors("tiny")
    print(f"t5 fp8 tiny, wo kept in bf16: {some[0]:.3e} / token 0 {some[1]:.3e} (all four: {full[0]:.3e} / {full[1]:.3e})")
    assert some[0] <= MARGIN * full[0] and some[1] <= MARGIN * full[1]
    assert enc.w["0.wo"].dtype == torch.bfloat16 and "0.wo.scale" not in enc.w and enc.w["0.wi"].dtype == torch.uint8
    assert "p8" not in enc._ws and "hn" not in enc._ws and "ao8" in enc._ws
    one = _enc("tiny", "fp8", ("wo",))                # the other way round: only wo in e4m3, the bf16 norm plane is back
    err = _gpu_errors("tiny", "fp8", ("wo",))
    assert err[0] <= MARGIN * full[0] and "hn" in one._ws and "hn8" not in one._ws and "p8" in one._ws


def test_f_the_bf16_mode_is_untouched_and_the_fp8_weights_are_half(monkeypatch):
    p = _params("tiny")
    ids = t5_ref.case_ids("tiny")
    first = T5Encoder(p, DEV)
    first.load_state_dict(synthetic_t5_state_dict(p, 0))
    second = load_t5(p, DEV, weights=synthetic_t5_state_dict(p, 0), precision="bf16")

    def never(*a, **k):
        raise AssertionError("an fp8 kernel ran in bf16 mode")
    for name in ("t5_rmsnorm_fp8", "gated_mul_fp8", "quantize_rows_fp8"):
        monkeypatch.setattr(ops, name, never)
    out = first.encode_ids(ids)
    assert torch.equal(out, second.encode_ids(ids))
    assert set(first._ws) == {"rows", "x", "hn", "qkv", "ao", "u", "g"}                     # today's workspace
    assert all(v.dtype != torch.uint8 for v in first.w.values()) and not any(k.endswith(".scale") for k in first.w)
    monkeypatch.undo()
    g = _golden("tiny")                                       # and still inside the gate of tests/test_t5_model_gpu.py
    ours = _errors(out.float().cpu().numpy()[:, g["rows"]], g)
    assert ours[0] <= g["bf16_err"][0] and ours[1] <= g["bf16_err"][1]
    f8 = _enc("tiny")
    ratio = f8.weight_bytes(embedding=False) / first.weight_bytes(embedding=False)
    print(f"t5 tiny weight bytes without the embedding: fp8 {f8.weight_bytes(False)}, bf16 {first.weight_bytes(False)}, "
          f"ratio {ratio:.3f}")
    assert ratio < 0.55
    assert f8.workspace_bytes() > 0 and first.workspace_bytes() > 0


def test_g_pipeline_with_the_synthetic_t5_text_encoder_in_fp8():
    from conceptattention_amd import ConceptAttentionFluxPipeline, tiny_params
    kw = dict(width=128, height=128, layer_indices=[0, 1], num_inference_steps=2, return_pil_heatmaps=False)
    pipe = ConceptAttentionFluxPipeline("flux-schnell", device=DEV, params=tiny_params(), n_text_tokens=64,
                                        text_encoder="synthetic-t5", t5_precision="fp8")
    enc = pipe.text_encoder.encoder
    assert enc.precision == "fp8" and enc.fp8 == frozenset(FP8_PROJECTIONS) and enc.w["0.qkv"].dtype == torch.uint8
    out = pipe.generate_image("a cat on the grass", ["cat", "grass"], **kw)
    assert out.concept_heatmaps.shape == (2, 8, 8) and np.isfinite(out.concept_heatmaps).all()
    assert np.isfinite(out.cross_attention_maps).all()
    txt = pipe._embed("a cat on the grass", ["cat", "grass"])[0]
    assert torch.isfinite(txt.float()).all() and torch.equal(pipe._embed("a cat on the grass", ["cat", "grass"])[0], txt)
    with pytest.raises(ValueError):
        ConceptAttentionFluxPipeline("flux-schnell", device=DEV, params=tiny_params(), n_text_tokens=64,
                                     text_encoder="synthetic-t5", t5_precision="fp4")
