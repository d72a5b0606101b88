"""The Flux autoencoder on the GPU: ``AutoEncoder.encode`` / ``decode`` with the reference's contract
(concept_attention/flux/src/flux/modules/autoencoder.py:277-312) on the HIP kernels of ca_vae.hip.

Layout and precision.  Activations are NHWC.  The residual stream ``h`` is fp32; every convolution and GEMM operand is
bf16 (written by the GroupNorm that precedes it), every accumulation, statistic and softmax fp32.  torch allocates the
buffers and permutes the 16-channel latent and the 3-channel image between NCHW and NHWC; everything else is a kernel.

Mid-block attention (one head, d = C).  q, k and ``proj_out`` are GEMMs over the token rows.  Two rules of the GEMM have
to be met without changing the arithmetic:

* K % 64 and N % 64: the token count T is padded to a multiple of 64 in the buffers.  The padding rows of the normed
  input and of k are zeros, the softmax writes exact zeros into the padding columns of P, so the padding contributes
  exact zeros to every sum.
* a per-column bias only, where V^T ([C, T], the operand P @ V needs) wants a per-row one: V^T is produced directly as
  W_v @ H^T without its bias, and, softmax rows summing to 1, ``b_v`` is folded into ``proj_out``'s bias on the host:
  b' = b_proj + W_proj @ b_v, formed in fp64.  The GEMM takes its bias as bf16, so b' is rounded to bf16 once (2^-9
  relative on the bias term), as b_q and b_k are.

``nin_shortcut`` (a 1x1 convolution whose channel counts may be below the GEMM's 64) runs through the convolution
kernel with ksize = 1.
"""
from __future__ import annotations

import math
import os
import warnings
from typing import Optional

import torch

from . import _lib as L
from . import ops
from .params import AutoEncoderParams, ae_params
from .weights import _gen

__all__ = ["AutoEncoder", "AutoEncoderParams", "load_ae", "synthetic_ae_state_dict", "ae_state_dict_spec"]

GN_EPS = 1e-6
SCORE_ROWS = 2048   # query rows per score chunk: 2048 x 16 384 fp32 = 128 MB at the 1024 x 1024 geometry


# ---------------------------------------------------------------------------------------------------------- layout
def _resnet(spec, name, cin, cout):
    spec += [(f"{name}.norm1.weight", (cin,)), (f"{name}.norm1.bias", (cin,)),
             (f"{name}.conv1.weight", (cout, cin, 3, 3)), (f"{name}.conv1.bias", (cout,)),
             (f"{name}.norm2.weight", (cout,)), (f"{name}.norm2.bias", (cout,)),
             (f"{name}.conv2.weight", (cout, cout, 3, 3)), (f"{name}.conv2.bias", (cout,))]
    if cin != cout:
        spec += [(f"{name}.nin_shortcut.weight", (cout, cin, 1, 1)), (f"{name}.nin_shortcut.bias", (cout,))]


def _attn(spec, name, c):
    spec += [(f"{name}.norm.weight", (c,)), (f"{name}.norm.bias", (c,))]
    for n in ("q", "k", "v", "proj_out"):
        spec += [(f"{name}.{n}.weight", (c, c, 1, 1)), (f"{name}.{n}.bias", (c,))]


def _mid_spec(spec, side, c):
    _resnet(spec, f"{side}.mid.block_1", c, c)
    _attn(spec, f"{side}.mid.attn_1", c)
    _resnet(spec, f"{side}.mid.block_2", c, c)


def ae_state_dict_spec(p: AutoEncoderParams) -> list:
    """[(name, shape)] under the reference's key names (nn.Module order of AutoEncoder, autoencoder.py:109-259)."""
    spec: list = []
    nres = len(p.ch_mult)
    spec += [("encoder.conv_in.weight", (p.ch, p.in_channels, 3, 3)), ("encoder.conv_in.bias", (p.ch,))]
    in_mult = (1,) + tuple(p.ch_mult)
    c = p.ch
    for lv in range(nres):
        c, cout = p.ch * in_mult[lv], p.ch * p.ch_mult[lv]
        for i in range(p.num_res_blocks):
            _resnet(spec, f"encoder.down.{lv}.block.{i}", c, cout)
            c = cout
        if lv != nres - 1:
            spec += [(f"encoder.down.{lv}.downsample.conv.weight", (c, c, 3, 3)),
                     (f"encoder.down.{lv}.downsample.conv.bias", (c,))]
    _mid_spec(spec, "encoder", c)
    spec += [("encoder.norm_out.weight", (c,)), ("encoder.norm_out.bias", (c,)),
             ("encoder.conv_out.weight", (2 * p.z_channels, c, 3, 3)), ("encoder.conv_out.bias", (2 * p.z_channels,))]
    c = p.ch * p.ch_mult[-1]
    spec += [("decoder.conv_in.weight", (c, p.z_channels, 3, 3)), ("decoder.conv_in.bias", (c,))]
    _mid_spec(spec, "decoder", c)
    ups = []
    for lv in reversed(range(nres)):
        lvl: list = []
        cout = p.ch * p.ch_mult[lv]
        for i in range(p.num_res_blocks + 1):
            _resnet(lvl, f"decoder.up.{lv}.block.{i}", c, cout)
            c = cout
        if lv != 0:
            lvl += [(f"decoder.up.{lv}.upsample.conv.weight", (c, c, 3, 3)), (f"decoder.up.{lv}.upsample.conv.bias", (c,))]
        ups.insert(0, lvl)
    for lvl in ups:
        spec += lvl
    spec += [("decoder.norm_out.weight", (c,)), ("decoder.norm_out.bias", (c,)),
             ("decoder.conv_out.weight", (p.out_ch, c, 3, 3)), ("decoder.conv_out.bias", (p.out_ch,))]
    return spec


def synthetic_ae_state_dict(p: AutoEncoderParams, seed: int = 0) -> dict:
    """Seeded on the CPU generator (one generator per tensor name, so the values do not depend on the order), every value
    bf16-representable.  Convolutions: U(-b, b) with PyTorch's default bound b = 1 / sqrt(fan_in); norms: weight
    1 +- 0.1, bias +- 0.1.  ``decoder.conv_out`` is halved: with the default bound the decoded image spans about +-1.7
    and the [-1, 1] clamp of the image conversion would saturate; halved it uses the range without reaching it."""
    sd, shapes = {}, dict(ae_state_dict_spec(p))
    for name, shape in shapes.items():
        u = torch.rand(shape, generator=_gen("ae." + name, seed, "cpu"), dtype=torch.float32) * 2 - 1
        base = name.rsplit(".", 1)[0]
        if ".norm" in name:
            t = 1 + 0.1 * u if name.endswith(".weight") else 0.1 * u
        else:
            wshape = shape if name.endswith(".weight") else shapes[base + ".weight"]
            t = u / math.sqrt(wshape[1] * wshape[2] * wshape[3])
            if base == "decoder.conv_out":
                t = t * 0.5
        sd[name] = t.to(torch.bfloat16).to(torch.float32)
    return sd


def attention_workspace(T: int, c: int, device) -> dict:
    """Buffers of ``attention_block`` for T tokens of c channels; the token count is padded to a multiple of 64."""
    Tp = (T + 63) // 64 * 64
    R = min(SCORE_ROWS, T)
    return {"T": T, "Tp": Tp,
            "part": torch.empty(128 * 96, device=device, dtype=torch.float32),
            "hn": torch.zeros(Tp, c, device=device, dtype=torch.bfloat16),      # padding rows stay zero
            "q": torch.empty(T, c, device=device, dtype=torch.bfloat16),
            "k": torch.zeros(Tp, c, device=device, dtype=torch.bfloat16),       # padding rows stay zero
            "vt": torch.empty(c, Tp, device=device, dtype=torch.bfloat16),
            "o": torch.empty(T, c, device=device, dtype=torch.bfloat16),
            "s": torch.empty(R, Tp, device=device, dtype=torch.float32),
            "p": torch.empty(R, Tp, device=device, dtype=torch.bfloat16)}


def pack_attention(t: dict, a: str, device) -> dict:
    """Device operands of AttnBlock ``a`` from fp32 host tensors under the reference's names."""
    w = {}
    c = t[f"{a}.q.weight"].shape[0]
    for n in ("q", "k", "v", "proj_out"):
        w[f"{a}.{n}.weight"] = t[f"{a}.{n}.weight"].reshape(c, c).to(device, torch.bfloat16).contiguous()
    for n in ("q", "k"):
        w[f"{a}.{n}.bias"] = t[f"{a}.{n}.bias"].to(device, torch.bfloat16)
    # softmax rows sum to 1: P (V + 1 b_v^T) W^T = P V W^T + W b_v
    folded = t[f"{a}.proj_out.bias"].double() + t[f"{a}.proj_out.weight"].reshape(c, c).double() @ t[f"{a}.v.bias"].double()
    w[f"{a}.proj_out.bias"] = folded.to(torch.float32).to(device, torch.bfloat16)
    w[f"{a}.ones"] = torch.ones(c, device=device, dtype=torch.float32)
    for n in ("weight", "bias"):
        w[f"{a}.norm.{n}"] = t[f"{a}.norm.{n}"].to(device, torch.float32)
    return w


def attention_block(x: torch.Tensor, w: dict, name: str, ws: dict) -> None:
    """x fp32 [B,H,W,C] += proj_out(softmax(q k^T / sqrt(C)) v) of GroupNorm(x), in place (AttnBlock, :25-52)."""
    B, H, W, C = x.shape
    T = ws["T"]
    if T != H * W:
        raise ValueError("attention_block: workspace made for another token count")
    scale = 1.0 / math.sqrt(C)
    for b in range(B):
        xb = x[b].view(1, T, C)
        ops.groupnorm_nhwc(xb, w[name + ".norm.weight"], w[name + ".norm.bias"], ws["hn"][:T].view(1, T, C), False,
                           GN_EPS, ws["part"])
        hn = ws["hn"][:T]
        ops.gemm([ops.Gemm(hn, w[name + ".q.weight"], w[name + ".q.bias"], ws["q"])])
        ops.gemm([ops.Gemm(hn, w[name + ".k.weight"], w[name + ".k.bias"], ws["k"][:T])])
        ops.gemm([ops.Gemm(w[name + ".v.weight"], ws["hn"], None, ws["vt"])])     # V^T = W_v H^T, bias folded away
        R = ws["s"].shape[0]
        for r0 in range(0, T, R):
            r1 = min(T, r0 + R)
            ops.gemm([ops.Gemm(ws["q"][r0:r1], ws["k"], None, ws["s"][: r1 - r0])])
            ops.softmax_rows(ws["s"][: r1 - r0], ws["p"][: r1 - r0], T, scale)
            ops.gemm([ops.Gemm(ws["p"][: r1 - r0], ws["vt"], None, ws["o"][r0:r1])])
        xr = x[b].view(T, C)
        ops.gemm([ops.Gemm(ws["o"], w[name + ".proj_out.weight"], w[name + ".proj_out.bias"], xr,
                           epilogue=L.EPI_GATE_RESIDUAL, resid=xr, gate=w[name + ".ones"])])


# ---------------------------------------------------------------------------------------------------------- the model
class AutoEncoder:
    """``encode(x[B,3,H,W]) -> [B,16,H/8,W/8]``, ``decode(z) -> [B,3,H,W]`` fp32; H and W multiples of 8 (of 2^(levels-1))."""

    def __init__(self, params: AutoEncoderParams, device="cuda"):
        if params.ch % 32 or params.ch & (params.ch - 1):
            raise ValueError("AutoEncoder: ch must be a power of two >= 32 (GroupNorm(32) over power-of-two channel counts)")
        self.params = params
        self.device = torch.device(device)
        self.scale_factor, self.shift_factor = params.scale_factor, params.shift_factor
        self.spec = dict(ae_state_dict_spec(params))
        self.tensors: dict = {}      # name -> fp32 host copy as loaded
        self.w: dict = {}            # packed device operands
        self._ws: dict = {}
        self.loaded = False

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd, strict: bool = True, assign: bool = False):
        """Same (missing, unexpected) semantics as nn.Module.load_state_dict; a shape mismatch always raises.  The
        operands are packed here, once.  ``assign`` is accepted because the reference's loaders pass it
        (image_generator.py:44); the tensors are always copied into packed operands, so it changes nothing."""
        missing = [k for k in self.spec if k not in sd]
        unexpected = [k for k in sd if k not in self.spec]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:4]}.. unexpected {unexpected[:4]}..")
        for k, shape in self.spec.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(shape):
                    raise RuntimeError(f"load_state_dict: {k} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
                self.tensors[k] = sd[k].detach().to("cpu", torch.float32)
        if not missing:
            self._pack()
        return missing, unexpected

    def state_dict(self):
        return dict(self.tensors)

    def _pack(self):
        dev, t, w = self.device, self.tensors, {}
        for name, shape in self.spec.items():
            base, leaf = name.rsplit(".", 1)
            attn_lin = ".attn_1." in name and ".norm." not in name
            if leaf == "weight" and len(shape) == 4 and not attn_lin:
                w[name] = ops.pack_conv_weight(t[name]).to(dev)
            elif not attn_lin:
                w[name] = t[name].to(dev)                                   # conv bias, norm weight / bias: fp32
        for side in ("encoder", "decoder"):
            w.update(pack_attention(t, f"{side}.mid.attn_1", dev))
        self.w = w
        self.loaded = True

    # ------------------------------------------------------------------ workspace
    def _workspace(self, B: int, H: int, W: int):
        """Resident buffers for images of H x W pixels, sized on first use: three fp32 planes for the residual stream and
        two bf16 operand planes, each as large as the widest activation of the net at that size; the zero-padded
        32-channel input planes and the NHWC outputs of both directions are added on their first use."""
        key = (B, H, W)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        p, dev = self.params, self.device
        n = len(p.ch_mult)
        elems = 0
        for lv in range(n):                      # widest pixels x channels over the levels (either direction)
            hw = (H >> lv) * (W >> lv)
            elems = max(elems, hw * p.ch * max(p.ch_mult[max(lv - 1, 0)], p.ch_mult[lv], p.ch_mult[min(lv + 1, n - 1)]), hw * 32)
        elems *= B
        ws = attention_workspace((H >> (n - 1)) * (W >> (n - 1)), p.ch * p.ch_mult[-1], dev)
        ws.update({"f": [torch.empty(elems, device=dev, dtype=torch.float32) for _ in range(3)],
                   "h": [torch.empty(elems, device=dev, dtype=torch.bfloat16) for _ in range(2)],
                   "part": torch.empty(B * 128 * 96, device=dev, dtype=torch.float32)})
        if len(self._ws) >= 3:
            self._ws.pop(next(iter(self._ws)))
        self._ws[key] = ws
        return ws

    # ------------------------------------------------------------------ blocks
    @staticmethod
    def _view(buf, B, H, W, C):
        return buf[: B * H * W * C].view(B, H, W, C)

    def _gn(self, ws, x, name, swish, out_buf=0):
        y = self._view(ws["h"][out_buf], *x.shape)
        ops.groupnorm_nhwc(x, self.w[name + ".weight"], self.w[name + ".bias"], y, swish, GN_EPS, ws["part"])
        return y

    def _conv(self, x, name, out, **kw):
        cout = self.spec[name + ".weight"][0]
        ops.conv2d_nhwc(x, self.w[name + ".weight"], self.w[name + ".bias"], out, cout, **kw)
        return out

    def _resnet(self, ws, f, name, x):
        """x fp32 [B,H,W,Cin] in plane f[0]; returns the block's output, f[0] again naming the plane that holds it."""
        B, H, W, cin = x.shape
        cout = self.spec[name + ".conv1.weight"][0]
        t = self._gn(ws, x, name + ".norm1", True)
        h1 = self._conv(t, name + ".conv1", self._view(ws["f"][f[1]], B, H, W, cout))
        t = self._gn(ws, h1, name + ".norm2", True)
        if cin == cout:
            return self._conv(t, name + ".conv2", x, resid=x)                        # in place: x + h
        xb = self._cast(ws, x, 1)                                                    # the shortcut's bf16 operand
        sc = self._conv(xb, name + ".nin_shortcut", self._view(ws["f"][f[2]], B, H, W, cout), ksize=1)
        f[0], f[1] = f[1], f[0]
        return self._conv(t, name + ".conv2", self._view(ws["f"][f[0]], B, H, W, cout), resid=sc)

    def _cast(self, ws, x, buf):
        """The fp32 stream as a bf16 convolution operand in operand plane ``buf``."""
        c = x.shape[-1]
        xb = self._view(ws["h"][buf], *x.shape)
        ops.affine_rows(x.view(-1, c), xb.view(-1, c))
        return xb

    def _resample(self, ws, f, name, x, **kw):
        """Downsample / Upsample: the convolution ``name`` of the cast stream into the next plane."""
        B, H, W, c = x.shape
        Ho, Wo = ops.conv_out_hw(H, W, 3, kw.get("stride", 1), kw.get("upsample", False))
        f[0], f[1] = f[1], f[0]
        return self._conv(self._cast(ws, x, 0), name, self._view(ws["f"][f[0]], B, Ho, Wo, c), **kw)

    def _mid(self, ws, f, side, x):
        x = self._resnet(ws, f, f"{side}.mid.block_1", x)
        attention_block(x, self.w, f"{side}.mid.attn_1", ws)
        return self._resnet(ws, f, f"{side}.mid.block_2", x)

    @staticmethod
    def _resident(ws, key, shape, dtype, device, zero=False):
        """A buffer of the workspace allocated on first use (zeroed once if asked: its padding stays zero)."""
        if key not in ws:
            ws[key] = (torch.zeros if zero else torch.empty)(shape, device=device, dtype=dtype)
        return ws[key]

    def _check(self, t, channels, what):
        if not self.loaded:
            raise RuntimeError("AutoEncoder: no weights loaded")
        m = 2 ** (len(self.params.ch_mult) - 1)
        if t.dim() != 4 or t.shape[1] != channels:
            raise ValueError(f"{what}: expected [B,{channels},H,W], got {tuple(t.shape)}")
        return m

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def encoder_moments(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 2 z, H/8, W/8] fp32: mean | logvar, the encoder's output before DiagonalGaussian."""
        return self._moments_nhwc(x)[0].permute(0, 3, 1, 2).contiguous()   # (a copy: the NHWC buffer is reused)

    MAX_PIXELS = 1024 * 1024   # full-resolution pixels of one pass through the net: the extent verified on the GPU

    def _items_per_pass(self, H, W, what):
        """A batch runs in passes of at most MAX_PIXELS full-resolution pixels, so the workspace stays bounded and no
        launch is larger than those of one 1024 x 1024 image; a single larger image needs tiling (not built)."""
        if H * W > self.MAX_PIXELS:
            raise ValueError(f"{what}: {H} x {W} pixels exceed {self.MAX_PIXELS} (tiled decoding is not built)")
        return max(1, self.MAX_PIXELS // (H * W))

    def _moments_nhwc(self, x):
        """fp32 NHWC moments [B, H/8, W/8, 2 z] (the workspace's buffer when the batch fits one pass) and their dims."""
        self._check(x, self.params.in_channels, "encode")
        n = self._items_per_pass(x.shape[2], x.shape[3], "encode")
        if x.shape[0] <= n:
            return self._moments_pass(x)
        parts = [self._moments_pass(x[i:i + n])[0].clone() for i in range(0, x.shape[0], n)]
        mom = torch.cat(parts)
        return mom, tuple(mom.shape[:3])

    def _moments_pass(self, x):
        p = self.params
        m = self._check(x, p.in_channels, "encode")
        B, _, H, W = x.shape
        if H % m or W % m:
            raise ValueError(f"encode: H and W must be multiples of {m}")
        ws = self._workspace(B, H, W)
        xin = x.to(self.device, torch.float32).permute(0, 2, 3, 1).contiguous()
        xb = self._resident(ws, "x32", (B, H, W, 32), torch.bfloat16, self.device, zero=True)   # channels 3.. stay zero
        ops.affine_rows(xin.view(-1, p.in_channels), xb.view(-1, 32), cols=p.in_channels)
        return self._moments_net(ws, xb)

    def _moments_net(self, ws, xb):
        """The encoder from its zero-padded bf16 input plane ``xb`` [B, H, W, 32] (the workspace's "x32") on."""
        p = self.params
        B, H, W, _ = xb.shape
        f = [0, 1, 2]
        h = self._conv(xb, "encoder.conv_in", self._view(ws["f"][f[0]], B, H, W, p.ch))
        n = len(p.ch_mult)
        for lv in range(n):
            for i in range(p.num_res_blocks):
                h = self._resnet(ws, f, f"encoder.down.{lv}.block.{i}", h)
            if lv != n - 1:
                h = self._resample(ws, f, f"encoder.down.{lv}.downsample.conv", h, stride=2)
        h = self._mid(ws, f, "encoder", h)
        t = self._gn(ws, h, "encoder.norm_out", True)
        _, hh, ww, _ = t.shape
        mom = self._resident(ws, "mom", (B, hh, ww, 2 * p.z_channels), torch.float32, self.device)
        self._conv(t, "encoder.conv_out", mom)
        return mom, (B, hh, ww)

    @torch.no_grad()
    def encode(self, x: torch.Tensor, sample: bool = True, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """scale * (mean + exp(0.5 logvar) * noise - shift) (autoencoder.py:262-305); ``sample=False``: the scaled mean.
        ``noise`` [B, z, H/8, W/8] is drawn with torch.randn on the device when not given."""
        mom, dims = self._moments_nhwc(x)
        return self._latent(mom, dims, sample, noise)

    def _latent(self, mom, dims, sample, noise):
        """DiagonalGaussian and the scale / shift on the NHWC moments; the caller's own NCHW tensor."""
        z = self.params.z_channels
        B, h, w_ = dims
        out = torch.empty(B, h, w_, z, device=self.device, dtype=torch.float32)
        m2 = mom.view(-1, 2 * z)
        a, b = self.scale_factor, -self.scale_factor * self.shift_factor
        if sample:
            if noise is None:
                noise = torch.randn(B, z, h, w_, device=self.device, dtype=torch.float32)
            nz = noise.to(self.device, torch.float32).permute(0, 2, 3, 1).contiguous().view(-1, z)
            ops.affine_rows(m2[:, :z], out.view(-1, z), a, b, logvar=m2[:, z:], noise=nz)
        else:
            ops.affine_rows(m2[:, :z], out.view(-1, z), a, b)
        return out.permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def encode_pixels(self, images, height: int, width: int, sample: bool = True,
                      noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``encode`` from image bytes: ``images`` is a list of uint8 [H0, W0, 3] tensors or arrays of any sizes.  Each is
        uploaded as bytes and written by ``ops.pixels_to_nhwc32`` (nearest resize to height x width, 2 x / 255 - 1, bf16)
        straight into its slot of the zero-padded input plane: no fp32 image, no layout copy, no cast launch.  The result
        is bit for bit ``encode(x)`` of x = interpolate(2 * (img.float() / 255) - 1, (height, width)) with the same
        ``noise``; the batch runs in the same passes of at most MAX_PIXELS pixels."""
        if not self.loaded:
            raise RuntimeError("AutoEncoder: no weights loaded")
        m = 2 ** (len(self.params.ch_mult) - 1)
        if height % m or width % m:
            raise ValueError(f"encode_pixels: height and width must be multiples of {m}")
        srcs = []
        for im in images:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)      # a read-only array (a PIL image's buffer) is only read here
                t = torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError(f"encode_pixels: every image must be uint8 [H0, W0, 3], got {t.dtype} {tuple(t.shape)}")
            srcs.append(t.contiguous().to(self.device))
        if not srcs:
            raise ValueError("encode_pixels: no images")
        n = self._items_per_pass(height, width, "encode_pixels")
        parts, dims = [], None
        for i in range(0, len(srcs), n):
            chunk = srcs[i:i + n]
            ws = self._workspace(len(chunk), height, width)
            xb = self._resident(ws, "x32", (len(chunk), height, width, 32), torch.bfloat16, self.device, zero=True)
            for j, src in enumerate(chunk):
                ops.pixels_to_nhwc32(src, xb[j])
            mom, dims = self._moments_net(ws, xb)
            parts.append(mom if len(srcs) <= n else mom.clone())      # (the NHWC buffer is reused by the next pass)
        if len(parts) > 1:
            mom = torch.cat(parts)
            dims = tuple(mom.shape[:3])
        return self._latent(mom, dims, sample, noise)

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        m = self._check(z, self.params.z_channels, "decode")
        n = self._items_per_pass(z.shape[2] * m, z.shape[3] * m, "decode")
        parts = [self._decode_pass(z[i:i + n], m).permute(0, 3, 1, 2).contiguous()   # the caller's own NCHW tensor:
                 for i in range(0, z.shape[0], n)]                                    # the NHWC buffer is reused
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    @torch.no_grad()
    def decode_pixels(self, z: torch.Tensor) -> torch.Tensor:
        """uint8 [B, H, W, 3] on the device, made from the decoder's NHWC buffer by ``ops.nhwc_to_pixels``: bit for bit
        ``(127.5 * (decode(z).clamp(-1, 1) + 1.0)).byte()`` in HWC order, with no fp32 image leaving the workspace."""
        m = self._check(z, self.params.z_channels, "decode_pixels")
        n = self._items_per_pass(z.shape[2] * m, z.shape[3] * m, "decode_pixels")
        if self.params.out_ch != 3:
            raise ValueError("decode_pixels: the byte image has 3 channels")
        out = torch.empty(z.shape[0], z.shape[2] * m, z.shape[3] * m, 3, device=self.device, dtype=torch.uint8)
        for i in range(0, z.shape[0], n):
            ops.nhwc_to_pixels(self._decode_pass(z[i:i + n], m), out[i:i + n])
        return out

    def _decode_pass(self, z, m):
        """One pass of the decoder; returns the workspace's fp32 NHWC image buffer [B, H, W, out_ch]."""
        p = self.params
        B, _, h, w_ = z.shape
        ws = self._workspace(B, h * m, w_ * m)
        f = [0, 1, 2]
        zin = z.to(self.device, torch.float32).permute(0, 2, 3, 1).contiguous()
        zb = self._resident(ws, "z32", (B, h, w_, 32), torch.bfloat16, self.device, zero=True)   # channels 16.. stay zero
        ops.affine_rows(zin.view(-1, p.z_channels), zb.view(-1, 32), 1.0 / self.scale_factor, self.shift_factor,
                        cols=p.z_channels)
        x = self._conv(zb, "decoder.conv_in", self._view(ws["f"][f[0]], B, h, w_, p.ch * p.ch_mult[-1]))
        x = self._mid(ws, f, "decoder", x)
        for lv in reversed(range(len(p.ch_mult))):
            for i in range(p.num_res_blocks + 1):
                x = self._resnet(ws, f, f"decoder.up.{lv}.block.{i}", x)
            if lv != 0:
                x = self._resample(ws, f, f"decoder.up.{lv}.upsample.conv", x, upsample=True)
        t = self._gn(ws, x, "decoder.norm_out", True)
        _, H, W, _ = t.shape
        img = self._resident(ws, "img", (B, H, W, p.out_ch), torch.float32, self.device)
        self._conv(t, "decoder.conv_out", img)
        return img

    # the reference's callers move the module around and switch modes; resident here
    def to(self, *a, **k):
        return self

    def eval(self):
        return self


def load_ae(name: str = "flux-schnell", device="cuda", weights="synthetic", seed: int = 0) -> AutoEncoder:
    """``weights``: "synthetic", a ``.safetensors`` path, or a state dict.  As in flux/util.py:165-184 the ``AE``
    environment variable names the checkpoint when the caller gives none ("synthetic"); nothing is downloaded."""
    ae = AutoEncoder(ae_params[name], device)
    if isinstance(weights, str) and weights == "synthetic" and os.environ.get("AE"):
        weights = os.environ["AE"]
    if isinstance(weights, dict):
        sd = weights
    elif weights == "synthetic":
        sd = synthetic_ae_state_dict(ae.params, seed)
    else:
        from safetensors.torch import load_file
        sd = load_file(str(weights), device="cpu")
    ae.load_state_dict(sd, strict=True)
    return ae
