"""Functional, state-dict-driven torch restatement of the Flux autoencoder's encoder and decoder
(flux/modules/autoencoder.py:25-312) in the dtype of the tensors it is given (fp32 / fp64).  Test infrastructure: pinned
to tests/golden/vae_*.npz on the CPU and used as the reference for shapes that have no golden; the package never
imports it."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

CASES = {   # name -> (ch, B, latent h, latent w, subsample step of the stored arrays)
    "tiny": (32, 1, 4, 4, 1),
    "rect": (64, 1, 6, 8, 1),
    "real": (128, 2, 16, 16, 1),
}
FULL = {"decode": (128, 1, 128, 128, 8), "encode": (128, 1, 64, 64, 8)}   # 1024^2 decode, 512^2 encode


def gn(sd, name, x, swish):
    y = F.group_norm(x, 32, sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype), eps=1e-6)
    return y * torch.sigmoid(y) if swish else y


def conv(sd, name, x, stride=1, padding=1):
    return F.conv2d(x, sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype), stride=stride, padding=padding)


def resnet(sd, name, x):
    h = conv(sd, name + ".conv1", gn(sd, name + ".norm1", x, True))
    h = conv(sd, name + ".conv2", gn(sd, name + ".norm2", h, True))
    if name + ".nin_shortcut.weight" in sd:
        x = conv(sd, name + ".nin_shortcut", x, padding=0)
    return x + h


def attn(sd, name, x):
    B, C, H, W = x.shape
    h = gn(sd, name + ".norm", x, False)
    q, k, v = (conv(sd, f"{name}.{n}", h, padding=0).reshape(B, C, H * W).transpose(1, 2) for n in "qkv")
    p = torch.softmax(q @ k.transpose(1, 2) / C ** 0.5, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(B, C, H, W)
    return x + conv(sd, name + ".proj_out", o, padding=0)


def _mid(sd, side, h):
    h = resnet(sd, f"{side}.mid.block_1", h)
    h = attn(sd, f"{side}.mid.attn_1", h)
    return resnet(sd, f"{side}.mid.block_2", h)


def encoder(sd, x, levels=4, num_res_blocks=2):
    h = conv(sd, "encoder.conv_in", x)
    for lv in range(levels):
        for i in range(num_res_blocks):
            h = resnet(sd, f"encoder.down.{lv}.block.{i}", h)
        if lv != levels - 1:
            h = conv(sd, f"encoder.down.{lv}.downsample.conv", F.pad(h, (0, 1, 0, 1)), stride=2, padding=0)
    h = _mid(sd, "encoder", h)
    return conv(sd, "encoder.conv_out", gn(sd, "encoder.norm_out", h, True))


def decoder(sd, z, levels=4, num_res_blocks=2):
    h = conv(sd, "decoder.conv_in", z)
    h = _mid(sd, "decoder", h)
    for lv in reversed(range(levels)):
        for i in range(num_res_blocks + 1):
            h = resnet(sd, f"decoder.up.{lv}.block.{i}", h)
        if lv != 0:
            h = conv(sd, f"decoder.up.{lv}.upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"))
    return conv(sd, "decoder.conv_out", gn(sd, "decoder.norm_out", h, True))


def decode(sd, z, scale=0.3611, shift=0.1159):
    return decoder(sd, z / scale + shift)


def case_inputs(name, ch, B, h, w, seed=0):
    """(z [B,16,h,w], x [B,3,8h,8w]): seeded, bf16-representable."""
    def g(tag):
        gen = torch.Generator(device="cpu")
        gen.manual_seed(zlib.crc32(f"vae.{name}.{tag}".encode()) + seed)
        return gen
    z = torch.randn(B, 16, h, w, generator=g("z")).to(torch.bfloat16).float()
    x = (torch.rand(B, 3, 8 * h, 8 * w, generator=g("x")) * 2 - 1).to(torch.bfloat16).float()
    return z, x


def subsample(a, step):
    """Every step-th row and column plus the last ones of the two trailing dimensions."""
    if step == 1:
        return a
    iy = sorted(set(range(0, a.shape[-2], step)) | {a.shape[-2] - 1})
    ix = sorted(set(range(0, a.shape[-1], step)) | {a.shape[-1] - 1})
    return a[..., iy, :][..., ix]


def checksum(t):
    return np.array([float(t.double().sum()), float(t.double().abs().sum())])


def errors(got, ref):
    """(max-abs, relative rms) distance of two arrays."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()), float(np.sqrt(((got - ref) ** 2).mean() / (ref ** 2).mean()))
