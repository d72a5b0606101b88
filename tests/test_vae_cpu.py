"""CPU checks of the autoencoder: the torch restatement against the reference's goldens, the state-dict contract of
``AutoEncoder``, the weight packer against an im2col in numpy, and argument rejection of the new entry points."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as entry
import vae_ref
from conceptattention_amd import AutoEncoderParams, ae_params, ops
from conceptattention_amd import _lib as L
from conceptattention_amd.vae import AutoEncoder, ae_state_dict_spec, synthetic_ae_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL = dict(vae_ref.CASES, **{"full_" + k: v for k, v in vae_ref.FULL.items()})


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"vae_{name}.npz"))


@pytest.mark.parametrize("name", list(vae_ref.CASES))
def test_restatement_matches_the_reference_goldens(name):
    ch, B, h, w, step = vae_ref.CASES[name]
    g = _golden(name)
    sd = synthetic_ae_state_dict(AutoEncoderParams(ch=ch))
    z, x = vae_ref.case_inputs(name, ch, B, h, w)
    np.testing.assert_allclose(vae_ref.checksum(z), g["z_checksum"], rtol=1e-12)
    np.testing.assert_allclose(vae_ref.checksum(x), g["x_checksum"], rtol=1e-12)
    with torch.no_grad():
        dec, mom = vae_ref.decode(sd, z).numpy(), vae_ref.encoder(sd, x).numpy()
    assert np.abs(dec - g["dec_f32"]).max() <= 2e-5
    assert np.abs(mom - g["mom_f32"]).max() <= 2e-5


def test_restatement_matches_the_full_size_encode_golden():
    ch, B, h, w, step = vae_ref.FULL["encode"]
    g = _golden("full_encode")
    sd = synthetic_ae_state_dict(AutoEncoderParams(ch=ch))
    _, x = vae_ref.case_inputs("full_encode", ch, B, h, w)
    np.testing.assert_allclose(vae_ref.checksum(x), g["x_checksum"], rtol=1e-12)
    with torch.no_grad():
        mom = vae_ref.subsample(vae_ref.encoder(sd, x).numpy(), step)
    assert np.abs(mom - g["mom_f32"]).max() <= 2e-5


def test_restatement_matches_the_full_size_decode_golden():
    """The 1024 x 1024 decode: the 16 384-token attention and the every-8th-pixel storage of the decoder's output."""
    ch, B, h, w, step = vae_ref.FULL["decode"]
    g = _golden("full_decode")
    sd = synthetic_ae_state_dict(AutoEncoderParams(ch=ch))
    z, _ = vae_ref.case_inputs("full_decode", ch, B, h, w)
    np.testing.assert_allclose(vae_ref.checksum(z), g["z_checksum"], rtol=1e-12)
    with torch.no_grad():
        dec = vae_ref.subsample(vae_ref.decode(sd, z).numpy(), step)
    assert dec.shape == g["dec_f32"].shape == (B, 3, 129, 129)
    assert np.abs(dec - g["dec_f32"]).max() <= 2e-5


@pytest.mark.parametrize("name", list(ALL))
def test_accepted_keys_and_shapes_are_the_references(name):
    g = _golden(name)
    spec = ae_state_dict_spec(AutoEncoderParams(ch=int(g["geometry"][0])))
    assert [k for k, _ in spec] == list(g["keys"])
    assert [",".join(map(str, s)) for _, s in spec] == list(g["shapes"])


def test_real_params_are_the_references():
    for name in ("flux-schnell", "flux-dev"):
        p = ae_params[name]
        assert (p.resolution, p.in_channels, p.ch, p.out_ch, tuple(p.ch_mult), p.num_res_blocks, p.z_channels,
                p.scale_factor, p.shift_factor) == (256, 3, 128, 3, (1, 2, 4, 4), 2, 16, 0.3611, 0.1159)


def test_load_state_dict_strict_missing_unexpected_and_shape_mismatch():
    p = AutoEncoderParams(ch=32)
    sd = synthetic_ae_state_dict(p)
    ae = AutoEncoder(p, "cpu")
    assert ae.load_state_dict(sd, strict=True) == ([], []) and ae.loaded
    part = dict(sd)
    del part["decoder.up.3.block.0.norm1.weight"]
    part["extra.key"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        AutoEncoder(p, "cpu").load_state_dict(part, strict=True)
    ae2 = AutoEncoder(p, "cpu")
    assert ae2.load_state_dict(part, strict=False) == (["decoder.up.3.block.0.norm1.weight"], ["extra.key"])
    assert not ae2.loaded
    with pytest.raises(RuntimeError):
        ae2.decode(torch.zeros(1, 16, 4, 4))
    bad = dict(sd)
    bad["encoder.conv_in.weight"] = torch.zeros(32, 4, 3, 3)
    with pytest.raises(RuntimeError, match="encoder.conv_in.weight"):
        AutoEncoder(p, "cpu").load_state_dict(bad, strict=False)


def test_synthetic_weights_are_seeded_and_bf16_representable():
    p = AutoEncoderParams(ch=32)
    a, b, c = synthetic_ae_state_dict(p, 0), synthetic_ae_state_dict(p, 0), synthetic_ae_state_dict(p, 1)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["decoder.conv_in.weight"], c["decoder.conv_in.weight"])
    assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in a.values())


@pytest.mark.parametrize("mode", ["s1", "s2", "up", "k1"])
def test_packed_weight_times_im2col_is_conv2d(mode):
    """The packer's layout, emulated in numpy with the kernel's own index arithmetic: out[p, n] =
    sum_k im2col[p, k] * packed[n, k], k = (ky * ksize + kx) * cin_pad + c, padding by predicate, stride 2 with the
    (0,1,0,1) padding, the upsample as (iy >> 1, ix >> 1).  A padded channel count (Cin 3 -> 32, Cout 5 -> 16)."""
    g = torch.Generator().manual_seed(3)
    B, H, W, cin, cout, k = 2, 5, 6, 3, 5, 1 if mode == "k1" else 3
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64).to(torch.bfloat16).double()
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64).to(torch.bfloat16).double()
    packed = ops.pack_conv_weight(w.float()).double().numpy()
    cin_pad = 32
    assert packed.shape == (16, k * k * cin_pad)
    stride, up, pad = (2 if mode == "s2" else 1), mode == "up", (1 if mode in ("s1", "up") else 0)
    Ho, Wo = ops.conv_out_hw(H, W, k, stride, up)
    Hv, Wv = (2 * H, 2 * W) if up else (H, W)
    xn = np.zeros((B, H, W, cin_pad))
    xn[..., :cin] = x.permute(0, 2, 3, 1).numpy()
    col = np.zeros((B, Ho, Wo, k * k * cin_pad))
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(k):
                for kx in range(k):
                    iy, ix = oy * stride + ky - pad, ox * stride + kx - pad
                    if 0 <= iy < Hv and 0 <= ix < Wv:
                        sy, sx = (iy >> 1, ix >> 1) if up else (iy, ix)
                        t = ky * k + kx
                        col[:, oy, ox, t * cin_pad:(t + 1) * cin_pad] = xn[:, sy, sx]
    got = (col @ packed.T)[..., :cout]
    if mode == "s2":
        ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    elif mode == "up":
        ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, padding=1)
    else:
        ref = F.conv2d(x, w, padding=pad)
    assert (col @ packed.T)[..., cout:].any() == False  # noqa: E712  (padding rows are zeros)
    np.testing.assert_allclose(got, ref.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    entry.build()
    lib = L.load()
    one = 4096   # a non-null, aligned "pointer": rejected calls never dereference
    conv = lambda *a: lib.ca_conv3x3_nhwc(*a)  # noqa: E731
    ok = [one, one, one, None, one, 1, 4, 4, 32, 16, 32, 16, 16, 3, 1, 0, 1, None]
    for i, v in ((0, None), (1, None), (4, None), (5, 0), (8, 16), (8, 48), (9, 0), (10, 16), (12, 8), (13, 2), (14, 3),
                 (0, one + 2)):
        args = list(ok)
        args[i] = v
        assert conv(*args) == -1, (i, v)
        assert b"ca_conv3x3_nhwc" in lib.ca_last_error()
    assert conv(*(ok[:14] + [2, 1, 1, None])) == -1          # stride 2 with the upsample
    assert conv(*(ok[:6] + [1, 4] + ok[8:14] + [2, 0, 1, None])) == -1   # stride 2 needs two input rows
    gn_ok = [one, 1, 32, one, one, one, 32, 1, 16, 32, 1e-6, 1, one, 1, None]
    for i, v in ((0, None), (3, None), (5, None), (12, None), (7, 0), (8, 0), (9, 48), (9, 16), (2, 16), (13, 0), (10, 0.0)):
        args = list(gn_ok)
        args[i] = v
        assert lib.ca_groupnorm_nhwc(*args) == -1, (i, v)
        assert b"ca_groupnorm_nhwc" in lib.ca_last_error()
    sm_ok = [one, 64, one, 64, 1, 64, 0.1, None]
    for i, v in ((0, None), (2, None), (4, 0), (5, 0), (5, 65), (6, 0.0)):
        args = list(sm_ok)
        args[i] = v
        assert lib.ca_softmax_rows_f32(*args) == -1, (i, v)
        assert b"ca_softmax_rows_f32" in lib.ca_last_error()
    af_ok = [one, 16, None, 0, None, 0, one, 16, 1, 4, 16, 1.0, 0.0, None]
    for i, v in ((0, None), (6, None), (9, 0), (10, 0), (10, 17), (2, one)):
        args = list(af_ok)
        args[i] = v
        assert lib.ca_affine_rows_f32(*args) == -1, (i, v)
        assert b"ca_affine_rows_f32" in lib.ca_last_error()
