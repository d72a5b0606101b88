"""``AutoEncoder`` on the GPU against the goldens made by the reference's own class.

Gate: max-abs and relative-rms distance from the reference's fp32 values <= the reference's own distance under
``torch.autocast(bfloat16)``, stored in the same golden.  Absolute bound: 1.5 x the value measured on an MI355X
(DESIGN.md section 2), the project's margin for box-to-box rounding differences."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vae_ref  # noqa: E402
from conceptattention_amd import AutoEncoderParams  # noqa: E402
from conceptattention_amd.vae import AutoEncoder, load_ae, synthetic_ae_state_dict  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
# (max-abs, relative rms) measured on an MI355X, per golden and output
MEASURED = {
    ("tiny", "dec"): (1.081e-2, 1.038e-2), ("tiny", "mom"): (1.065e-2, 9.502e-3),
    ("rect", "dec"): (8.638e-3, 9.485e-3), ("rect", "mom"): (1.219e-2, 8.711e-3),
    ("real", "dec"): (7.405e-3, 8.270e-3), ("real", "mom"): (1.402e-2, 9.220e-3),
    ("full_decode", "dec"): (6.669e-3, 8.289e-3), ("full_encode", "mom"): (1.095e-2, 9.083e-3),
}
_AE = {}


def _ae(ch):
    if ch not in _AE:
        ae = AutoEncoder(AutoEncoderParams(ch=ch), DEV)
        ae.load_state_dict(synthetic_ae_state_dict(ae.params, 0))
        _AE[ch] = ae
    return _AE[ch]


def _gate(name, key, got, g):
    ma, rr = vae_ref.errors(got, g[key + "_f32"])
    ref_ma, ref_rr = g[key + "_bf16_err"]
    print(f"vae {name} {key}: max-abs {ma:.3e} (reference bf16 {ref_ma:.3e}), rel-rms {rr:.3e} (reference bf16 {ref_rr:.3e})")
    assert np.isfinite(got).all()
    assert ma <= ref_ma and rr <= ref_rr
    assert ma <= 1.5 * MEASURED[(name, key)][0] and rr <= 1.5 * MEASURED[(name, key)][1]


@pytest.mark.parametrize("name", list(vae_ref.CASES))
def test_decode_and_moments_against_the_golden(name):
    ch, B, h, w, step = vae_ref.CASES[name]
    g = np.load(os.path.join(GOLDEN, f"vae_{name}.npz"))
    z, x = vae_ref.case_inputs(name, ch, B, h, w)
    ae = _ae(ch)
    dec = ae.decode(z.to(DEV))
    assert dec.dtype == torch.float32 and tuple(dec.shape) == (B, 3, 8 * h, 8 * w)
    _gate(name, "dec", dec.cpu().numpy(), g)
    mom = ae.encoder_moments(x.to(DEV))
    assert tuple(mom.shape) == (B, 32, h, w)
    _gate(name, "mom", mom.cpu().numpy(), g)


@pytest.mark.parametrize("part", ["decode", "encode"])
def test_full_size_against_the_golden(part):
    ch, B, h, w, step = vae_ref.FULL[part]
    g = np.load(os.path.join(GOLDEN, f"vae_full_{part}.npz"))
    z, x = vae_ref.case_inputs("full_" + part, ch, B, h, w)
    ae = _ae(ch)
    if part == "decode":
        _gate("full_decode", "dec", vae_ref.subsample(ae.decode(z.to(DEV)).cpu().numpy(), step), g)
    else:
        _gate("full_encode", "mom", vae_ref.subsample(ae.encoder_moments(x.to(DEV)).cpu().numpy(), step), g)


def test_batch_of_two_equals_two_single_calls_bit_for_bit():
    ch, B, h, w, _ = vae_ref.CASES["real"]
    z, x = vae_ref.case_inputs("real", ch, B, h, w)
    ae = _ae(ch)
    both = ae.decode(z.to(DEV))
    mom = ae.encoder_moments(x.to(DEV))
    for b in range(B):
        assert torch.equal(both[b:b + 1], ae.decode(z[b:b + 1].to(DEV)))
        assert torch.equal(mom[b:b + 1], ae.encoder_moments(x[b:b + 1].to(DEV)))


def test_encode_is_moments_plus_noise_arithmetic():
    ch, B, h, w, _ = vae_ref.CASES["rect"]
    _, x = vae_ref.case_inputs("rect", ch, B, h, w)
    ae = _ae(ch)
    mom = ae.encoder_moments(x.to(DEV)).double().cpu()
    mean, logvar = mom[:, :16], mom[:, 16:]
    noise = torch.randn(B, 16, h, w, generator=torch.Generator().manual_seed(1))
    s, sh = ae.params.scale_factor, ae.params.shift_factor
    got = ae.encode(x.to(DEV), sample=True, noise=noise.to(DEV)).double().cpu()
    ref = s * (mean + torch.exp(0.5 * logvar) * noise.double() - sh)
    # fp32 arithmetic of four operations on values of magnitude |ref| + s |shift|, and the fast exp (2 ulp)
    tol = 8 * 2.0 ** -24 * (ref.abs() + s * (mean.abs() + sh) + s * (torch.exp(0.5 * logvar) * noise.double()).abs() * 4)
    assert tuple(got.shape) == (B, 16, h, w) and ((got - ref).abs() <= tol).all()
    got0 = ae.encode(x.to(DEV), sample=False).double().cpu()
    ref0 = s * (mean - sh)
    assert ((got0 - ref0).abs() <= 4 * 2.0 ** -24 * (ref0.abs() + s * (mean.abs() + sh))).all()
    assert tuple(ae.encode(x.to(DEV)).shape) == (B, 16, h, w)      # noise drawn on the device


def test_safetensors_path_and_environment_variable_load_the_same_weights(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from conceptattention_amd import ae_params
    sd = synthetic_ae_state_dict(ae_params["flux-schnell"], seed=5)
    path = str(tmp_path / "ae.safetensors")
    save_file(sd, path)
    z = vae_ref.case_inputs("tiny", 128, 1, 4, 4)[0].to(DEV)
    ref = load_ae("flux-schnell", DEV, weights=sd).decode(z)
    assert torch.equal(load_ae("flux-schnell", DEV, weights=path).decode(z), ref)
    monkeypatch.setenv("AE", path)
    assert torch.equal(load_ae("flux-schnell", DEV).decode(z), ref)
    monkeypatch.delenv("AE")
    assert not torch.equal(load_ae("flux-schnell", DEV, seed=0).decode(z), ref)


def test_pipeline_returns_a_pil_image_and_encodes_one():
    import PIL.Image
    from conceptattention_amd import ConceptAttentionFluxPipeline, tiny_params
    pipe = ConceptAttentionFluxPipeline("flux-schnell", device=DEV, params=tiny_params(), n_text_tokens=16,
                                        autoencoder="synthetic")
    out = pipe.generate_image("a cat on the grass", ["cat", "grass"], width=128, height=128, layer_indices=[0, 1],
                              num_inference_steps=2)
    assert isinstance(out.image, PIL.Image.Image) and out.image.size == (128, 128)
    enc = pipe.encode_image(out.image, ["cat", "grass"], prompt="a cat", width=128, height=128, layer_indices=[0, 1],
                            num_samples=1)
    assert len(enc.concept_heatmaps) == 2


def test_a_batch_split_into_passes_equals_the_batch_in_one_pass(monkeypatch):
    ch, B, h, w, _ = vae_ref.CASES["real"]
    z, x = vae_ref.case_inputs("real", ch, B, h, w)
    ae = _ae(ch)
    dec, mom = ae.decode(z.to(DEV)), ae.encoder_moments(x.to(DEV))
    monkeypatch.setattr(ae, "MAX_PIXELS", 8 * h * 8 * w)            # one image per pass
    assert torch.equal(ae.decode(z.to(DEV)), dec) and torch.equal(ae.encoder_moments(x.to(DEV)), mom)
    assert tuple(ae.encode(x.to(DEV), sample=False).shape) == (B, 16, h, w)
    monkeypatch.setattr(ae, "MAX_PIXELS", 8 * h * 8 * w - 1)
    with pytest.raises(ValueError):
        ae.decode(z.to(DEV))
