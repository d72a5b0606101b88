"""Launch forms of the autoencoder kernels (conceptattention_amd/csrc/ca_vae.hip), their fp64 references, derived
bounds, a faithful fp32 emulation on the CPU and the named kernel slips the bounds must reject.

Imported by tests/test_vae_routes_gpu.py (the GPU cases, through the C entry points), by tests/test_vae_cases_cpu.py
(coverage of every launch form and entry point by a case, the edges the table must hit, the discrimination checks) and
by the address-range files.  Nothing here touches torch.cuda at import time; a reference runs on the device its `dev`
argument names.

A case names its C entry point and the kernel instantiation(s) that entry point launches for its arguments, spelled as
where ca_vae.hip launches them; a GroupNorm case names both of its launches, joined by " + ".  make_inputs returns the
host buffers exactly as the kernel sees them: 2-D [rows, row stride], the columns between width and stride filled with
junk for an input (JUNK, finite and non-zero: a kernel that reads them is wrong by a lot) and with a finite canary
for an output (CANARY), the written range of an output with NaN.  reference returns, per output,
(fp64 value, bound before the output's rounding, kind); the canary columns are an output of kind "exact".

Bounds (elementwise, u = 2^-24):
  convolution   bf16 x bf16 products are exact in fp32, so before the epilogue only the accumulation errs: K additions
                within u of a partial sum of at most A = conv(|x|, |w|); 4 sqrt(K) u A.  Bias and residual: two
                roundings, 2 u (|y| + |bias| + |resid|).  An fp32 store is exact (kind "f32" adds nothing).
  bf16 store    of any kernel: half a bf16 ulp of the fp64 value (round to nearest even) on top of the bound before
                the store (kind "bf16").
  GroupNorm     16 u max|x| rstd |gamma| + GN_ABS (the Welford mean and the subtraction, a few ulps of max|x| seen
                through rstd gamma); swish: |d swish / dy| <= 1.1 and 4 u |y| for the exp and the divide.
  softmax       relative 2 u (|scale (s - max)| + sqrt(n) + 4) (the exp2 argument's rounding, the sum, the
                reciprocal and the product), 1e-38 absolute; after the half-ulp store never below 2^-133, bf16's
                smallest subnormal (kind "prob").
  affine        t = exp(h) noise, h = 0.5 logvar (exact): relative (5 |h| + EXP_ULPS) u for the one __expf (the
                exponent's rounding is amplified by |h|) and 2 u per remaining fp32 operation of its running
                magnitude: the product, x + t, a v, + b.  With a = 1, b = 0 and no logvar the kernel is a copy or a
                cast: kind "exact" against x, or against x.to(torch.bfloat16).

The softmax scores are unrounded fp32 (they are a GEMM's fp32 output in the model); every other input is
bf16-representable except the mean-1000 GroupNorm case, which needs unrounded fp32 values to tell a one-pass variance
from a stable one.

Measured on MI355X: see the comment under the constants.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace

import torch
import torch.nn.functional as F

import gemm_route_cases as G
import rowop_cases as R

U = 2.0 ** -24
EXP_ULPS = R.EXP_ULPS
GN_ABS = 1e-6
GN_EPS = 1e-6
CANARY = 123.0
JUNK = -77.0
NAN = float("nan")

# Measured on MI355X, tests/test_vae_routes_gpu.py (the printed max err / bound, largest per family and output kind):
#   convolution fp32 out 0.041, bf16 out 0.997 (the half-ulp store); GroupNorm 1.000 (the half-ulp store: the bound
#   before it is a few 1e-6, so a value next to a rounding tie uses all of it; no element over); softmax 0.999;
#   affine fp32 out 0.250, bf16 out 1.000 (the half-ulp store again), the casts and copies, the 71M-element one among
#   them, bit for bit.
#   Bit for bit as well: every canary column and every input; the bf16 store of all 13 bf16 convolution cases against
#   RNE of the same launch's fp32 store; the scalar epilogue of the three ldo / ldr cases against their contiguous
#   twins; ops.conv2d_nhwc, groupnorm_nhwc, softmax_rows and affine_rows against the entry points on every case they
#   can express.  The faithful fp32 emulation on the CPU (tests/test_vae_cases_cpu.py) gives the same picture:
#   convolution 0.048 / 0.997, GroupNorm 0.9996, softmax 0.999, affine 0.371 / 0.9995.
#   No constant was widened: every bound above is as derived.


# --------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    entry: str          # the C entry point (include/conceptattn.h)
    kernel: str         # the instantiation(s) it launches, spelled as where ca_vae.hip launches them
    op: str             # conv | gn | softmax | affine
    shape: dict = field(default_factory=dict, hash=False, compare=False)
    seed: int = 0

    @property
    def id(self):
        return self.name

    @property
    def kernels(self):
        return [k.strip() for k in self.kernel.split("+")]


def ceil_to(v, m):
    return (v + m - 1) // m * m


def conv_geometry(s):
    """(ksize, stride, upsample, Ho, Wo, M) of a convolution case."""
    k = 1 if s["mode"] == "k1" else 3
    stride, up = (2 if s["mode"] == "s2" else 1), s["mode"] == "up"
    if up:
        Ho, Wo = 2 * s["H"], 2 * s["W"]
    elif stride == 2:
        Ho, Wo = (s["H"] - 2) // 2 + 1, (s["W"] - 2) // 2 + 1
    else:
        Ho, Wo = s["H"], s["W"]
    return k, stride, up, Ho, Wo, s["B"] * Ho * Wo


def conv_vector_epilogue(s) -> bool:
    """Whether the kernel stores four channels at a time: Cout, ldo and ldr (4 without a residual) multiples of 4."""
    ldr = s["ldr"] if s["resid"] == "separate" else s["ldo"] if s["resid"] == "in place" else 4
    return s["cout"] % 4 == 0 and s["ldo"] % 4 == 0 and ldr % 4 == 0


_SEED = [0]


def _cv(name, H, W, cin, cout, mode, bias=True, resid="none", out="f32", ldx=None, ldo=None, ldr=None, B=2):
    _SEED[0] += 1
    kernel = "ca_conv_kernel<1>" if ceil_to(cout, 16) <= 32 else "ca_conv_kernel<4>"
    s = dict(H=H, W=W, cin=cin, cout=cout, mode=mode, bias=bias, resid=resid, out=out, ldx=ldx or ceil_to(cin, 32),
             ldo=ldo or cout, ldr=(ldr or cout) if resid == "separate" else None, B=B)
    assert resid in ("none", "separate", "in place") and (resid != "in place" or out == "f32")
    return Case(name, "ca_conv3x3_nhwc", kernel, "conv", s, 1000 + _SEED[0])


# the 16 parameter sets of tests/test_vae_kernels_gpu.py CONV_CASES: H, W, Cin, Cout, mode, resid, out_f32
LEGACY_CONV = [
    (1, 1, 32, 16, "s1", False, True), (5, 7, 96, 48, "s1", True, True), (16, 16, 512, 160, "s1", False, False),
    (33, 17, 32, 160, "s1", True, False), (33, 17, 96, 16, "s1", False, True), (5, 7, 32, 48, "s2", False, True),
    (16, 16, 96, 160, "s2", True, True), (33, 17, 512, 16, "s2", False, False), (5, 7, 96, 160, "up", False, True),
    (16, 16, 32, 48, "up", True, False), (1, 1, 32, 16, "up", False, True), (5, 7, 3, 48, "s1", False, True),
    (16, 16, 16, 160, "s1", True, True), (16, 16, 32, 3, "s1", False, True), (33, 17, 96, 3, "s1", False, False),
    (33, 17, 96, 160, "k1", True, True),
]
CASES = [_cv(f"conv_{H}x{W}_c{ci}_o{co}_{m}{'_resid' if r else ''}_{'f32' if f else 'bf16'}", H, W, ci, co, m,
             resid="separate" if r else "none", out="f32" if f else "bf16") for H, W, ci, co, m, r, f in LEGACY_CONV]
CASES += [
    # <1>: Cout 20 and 32 make both wave columns live (CoutPad = 32); 20 ends inside a fragment under the vector store
    _cv("conv1_o20_vec_tail_bf16", 5, 7, 32, 20, "s1", out="bf16"),
    _cv("conv1_o32_in_place", 8, 8, 32, 32, "s1", resid="in place"),                       # M == 128 exactly
    _cv("conv1_o16_ldx40_junk", 5, 7, 32, 16, "s1", ldx=40, ldo=20),
    _cv("conv1_o3_ldo8_bf16", 3, 3, 32, 3, "s2", out="bf16", ldo=8),                        # s2 on 3 x 3
    # <4>
    _cv("conv4_o35_scalar_tail", 5, 7, 32, 35, "s1", resid="separate", ldr=37, ldo=36),
    _cv("conv4_o36_partial_fragment_bf16", 5, 7, 32, 36, "s1", out="bf16", ldo=40),
    _cv("conv4_o48_no_bias", 5, 7, 32, 48, "s1", bias=False),                               # wave column 1: no MFMA
    _cv("conv4_o80_no_bias_resid", 5, 7, 32, 80, "up", bias=False, resid="separate", ldr=88, ldo=84),
    _cv("conv4_o130_scalar_second_block", 2, 2, 32, 130, "s2", out="bf16"),                 # s2 on 2 x 2
    _cv("conv4_o132_vector_second_block", 5, 7, 32, 132, "s1", resid="in place", ldo=136),
    _cv("conv4_o160_B3_boundary_in_tile", 5, 7, 64, 160, "s1", B=3, out="bf16", resid="separate"),
    # the scalar epilogue with Cout % 4 == 0, and the contiguous twins the GPU file compares them with
    _cv("conv4_o48_scalar_by_ldo", 5, 7, 32, 48, "s1", resid="separate", ldo=50, ldr=48),
    _cv("conv4_o48_scalar_by_ldr", 5, 7, 32, 48, "s1", resid="separate", ldo=48, ldr=50, out="bf16"),
    _cv("conv1_o16_scalar_by_ldo_bf16", 5, 7, 32, 16, "s1", out="bf16", ldo=18),
    # K walk: one step in all, one step per tap
    _cv("conv1_k1_c32_one_step", 5, 7, 32, 32, "k1"),
    _cv("conv4_k1_c64_bf16", 5, 7, 64, 48, "k1", out="bf16", ldo=52),
    # pixel extents
    _cv("conv1_33x1", 33, 1, 32, 16, "s1"),
    _cv("conv4_1x17", 1, 17, 32, 48, "s1", resid="separate"),
    _cv("conv1_M129", 43, 3, 32, 16, "s1", B=1),
]
_SCALAR_TWINS = ["conv4_o48_scalar_by_ldo", "conv4_o48_scalar_by_ldr", "conv1_o16_scalar_by_ldo_bf16"]


def _gn(name, C, HW, xdt, swish, B=2, mean=0.0, std=1.0, n_chunks=None, ldx=None, ldy=None, const=False):
    _SEED[0] += 1
    t = "float" if xdt == "f32" else "bf16"
    s = dict(C=C, HW=HW, B=B, xdt=xdt, swish=swish, mean=mean, std=std, n_chunks=n_chunks, ldx=ldx or C, ldy=ldy or C,
             const=const)
    return Case(name, "ca_groupnorm_nhwc", f"ca_gn_stats_kernel<{t}> + ca_gn_apply_kernel<{t}>", "gn", s,
                2000 + _SEED[0])


def groupnorm_chunks(hw: int) -> int:
    """The wrapper's choice (ops.groupnorm_chunks); tests/test_vae_cases_cpu.py holds the two together."""
    return max(1, min(128, hw // 512))


CASES += [
    _gn("gn_C32_hw1_f32_swish", 32, 1, "f32", True),
    _gn("gn_C32_hw7_bf16_B3", 32, 7, "bf16", False, B=3),
    _gn("gn_C64_hw7_f32", 64, 7, "f32", False),
    _gn("gn_C64_hw511_bf16_swish", 64, 511, "bf16", True, mean=0.5, std=2.0),
    _gn("gn_C128_hw512_f32_swish", 128, 512, "f32", True),
    _gn("gn_C128_hw1023_bf16_B1", 128, 1023, "bf16", False, B=1),
    _gn("gn_C256_hw1024_f32", 256, 1024, "f32", False),
    _gn("gn_C256_hw1025_bf16_swish", 256, 1025, "bf16", True),
    _gn("gn_C512_hw4096_f32_B1", 512, 4096, "f32", False, B=1),
    _gn("gn_C512_hw7_bf16_swish", 512, 7, "bf16", True),
    _gn("gn_C1024_hw7_f32_swish", 1024, 7, "f32", True),
    _gn("gn_C1024_hw1025_bf16", 1024, 1025, "bf16", False, B=1),
    _gn("gn_C32_hw1025_f32", 32, 1025, "f32", False),                    # HW % rstep = 1; two chunks of 513 and 512
    _gn("gn_C32_hw70000_f32_swish", 32, 70000, "f32", True),
    _gn("gn_C64_hw4096_one_chunk", 64, 4096, "f32", True, n_chunks=1),
    _gn("gn_C128_hw1000_1024_chunks", 128, 1000, "bf16", False, n_chunks=1024),     # 24 empty chunks
    _gn("gn_C32_hw5_7_chunks", 32, 5, "f32", False, n_chunks=7),
    _gn("gn_C1024_hw40000_apply_grid_cap", 1024, 40000, "f32", True, B=1),          # 5000 > 4096 apply blocks
    _gn("gn_C64_hw33_f32_strided", 64, 33, "f32", True, ldx=68, ldy=72),
    _gn("gn_C128_hw33_bf16_strided", 128, 33, "bf16", False, ldx=136, ldy=132),
    _gn("gn_C128_hw600_constant", 128, 600, "f32", True, const=True),
    _gn("gn_C64_hw4096_mean100", 64, 4096, "f32", False, mean=100.0),
    _gn("gn_C64_hw4096_mean1000_unrounded", 64, 4096, "f32", False, mean=1000.0),
]


def _sm(name, rows, n, lds, ldp, scale=0.125):
    _SEED[0] += 1
    return Case(name, "ca_softmax_rows_f32", "ca_softmax_rows_kernel", "softmax",
                dict(rows=rows, n=n, lds=lds, ldp=ldp, scale=scale), 3000 + _SEED[0])


CASES += [
    _sm("softmax_n1_row1", 1, 1, 1, 1),
    _sm("softmax_n63", 5, 63, 66, 128),
    _sm("softmax_n64", 5, 64, 64, 64, scale=512 ** -0.5),
    _sm("softmax_n65_pad300", 5, 65, 67, 365),
    _sm("softmax_n255", 5, 255, 256, 320),
    _sm("softmax_n256", 5, 256, 259, 256, scale=512 ** -0.5),
    _sm("softmax_n257", 5, 257, 257, 264),
    _sm("softmax_n1000", 5, 1000, 1003, 1088),
]


def _af(name, rows, C, out, lv, ldx=None, ldo=None, ldl=None, ldn=None, a=1.0, b=0.0, view=False, big=False):
    _SEED[0] += 1
    s = dict(rows=rows, C=C, out=out, lv=lv, ldx=ldx or C, ldo=ldo or C, ldl=ldl or C, ldn=ldn or C, a=a, b=b,
             view=view, big=big)
    return Case(name, "ca_affine_rows_f32", "ca_affine_rows_kernel", "affine", s, 4000 + _SEED[0])


SCALE_FACTOR, SHIFT_FACTOR = 0.3611, 0.1159       # the Flux autoencoder's latent scale and shift
CASES += [
    _af("affine_cast_bf16_padded", 5, 16, "bf16", False, ldx=20, ldo=32),                     # the conv operand's cast
    _af("affine_copy_f32_padded", 5, 16, "f32", False, ldx=20, ldo=24),
    _af("affine_decode_f32", 7, 16, "f32", False, ldo=20, a=1 / SCALE_FACTOR, b=SHIFT_FACTOR),
    _af("affine_decode_bf16", 70, 16, "bf16", False, ldx=24, ldo=32, a=1 / SCALE_FACTOR, b=SHIFT_FACTOR),
    _af("affine_sample_bf16_moments_view", 35, 16, "bf16", True, ldo=32, ldn=16, a=SCALE_FACTOR,
        b=-SCALE_FACTOR * SHIFT_FACTOR, view=True),
    _af("affine_sample_f32", 9, 12, "f32", True, ldx=14, ldl=16, ldn=13, ldo=15, a=SCALE_FACTOR,
        b=-SCALE_FACTOR * SHIFT_FACTOR),
    _af("affine_1_element", 1, 1, "bf16", False, ldo=2),
    _af("affine_255_elements", 15, 17, "f32", True, a=1.5, b=-0.25),
    _af("affine_257_elements", 257, 1, "bf16", False, ldx=3, a=-2.0, b=0.5),
    _af("affine_grid_stride_71M", 2 ** 22 + 3, 17, "bf16", False, big=True),                  # > 65536 x 1024 elements
]
BY_ID = {c.id: c for c in CASES}
SCALAR_TWINS = {cid: replace(BY_ID[cid], name=cid + "_contiguous_twin",
                             shape=dict(BY_ID[cid].shape, ldo=BY_ID[cid].shape["cout"],
                                        ldr=BY_ID[cid].shape["cout"] if BY_ID[cid].shape["ldr"] else None))
                for cid in _SCALAR_TWINS}


# --------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(shape, g, scale=1.0, shift=0.0):
    """fp32 values that are exact in bf16."""
    return (torch.randn(shape, generator=g) * scale + shift).to(torch.bfloat16).float()


def _padded(vals, ld, fill, dtype=None):
    out = torch.full((vals.shape[0], ld), fill, dtype=dtype or vals.dtype)
    out[:, :vals.shape[1]] = vals.to(out.dtype)
    return out


def make_inputs(case: Case) -> dict:
    """Host (CPU) buffers of one case, as the kernel sees them; keys with a leading underscore are the same values in
    the layout the reference wants."""
    s, g = case.shape, _gen(case.seed)
    if case.op == "conv":
        k, _, _, Ho, Wo, M = conv_geometry(s)
        B, H, W, cin, cout = s["B"], s["H"], s["W"], s["cin"], s["cout"]
        cin_pad = ceil_to(cin, 32)
        x = _bf((B, cin, H, W), g)
        w = _bf((cout, cin, k, k), g, 1.0 / math.sqrt(cin * k * k))
        b = _bf((cout,), g, 0.1)
        r = _bf((B, cout, Ho, Wo), g)
        xr = torch.zeros(B * H * W, cin_pad)
        xr[:, :cin] = x.permute(0, 2, 3, 1).reshape(-1, cin)
        wp = torch.zeros(ceil_to(cout, 16), k * k, cin_pad)
        wp[:cout, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, k * k, cin)
        odt = torch.float32 if s["out"] == "f32" else torch.bfloat16
        rr = r.permute(0, 2, 3, 1).reshape(M, cout)
        out0 = _padded(torch.full((M, cout), NAN), s["ldo"], CANARY, odt)
        inp = dict(x=_padded(xr, s["ldx"], JUNK, torch.bfloat16), w=wp.reshape(wp.shape[0], -1).bfloat16(), out0=out0,
                   _x=x, _w=w)
        if s["bias"]:
            inp["bias"] = b
        if s["resid"] == "separate":
            inp["resid"] = _padded(rr, s["ldr"], JUNK)
        elif s["resid"] == "in place":
            out0[:, :cout] = rr
        if s["resid"] != "none":
            inp["_r"] = r
        return inp
    if case.op == "gn":
        B, HW, C = s["B"], s["HW"], s["C"]
        if s["const"]:
            x = torch.full((B, HW, C), 0.75)
        elif s["mean"] >= 1000:
            x = torch.randn((B, HW, C), generator=g) * s["std"] + s["mean"]
        else:
            x = _bf((B, HW, C), g, s["std"], s["mean"])
        gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        xdt = torch.float32 if s["xdt"] == "f32" else torch.bfloat16
        return dict(x=_padded(x.reshape(B * HW, C), s["ldx"], JUNK, xdt), gamma=gamma, beta=beta,
                    y0=_padded(torch.full((B * HW, C), NAN), s["ldy"], CANARY, torch.bfloat16))
    if case.op == "softmax":
        rows, n = s["rows"], s["n"]
        sc = torch.randn(rows, n, generator=g) * 8
        if rows >= 5:
            sc[1] = 3.0                                                   # equal scores
            sc[2, n // 2] = sc[2].max() + 60 / s["scale"]                 # one score 60 nats above the rest
            sc[3] = -1e4 + torch.randn(n, generator=g)                    # all near -1e4
        return dict(s=_padded(sc, s["lds"], NAN), p0=torch.full((rows, s["ldp"]), NAN, dtype=torch.bfloat16))
    if case.op == "affine":
        rows, C = s["rows"], s["C"]
        odt = torch.float32 if s["out"] == "f32" else torch.bfloat16
        if s["big"]:
            return dict(x=torch.randn(rows, C, generator=g), out0=torch.full((rows, s["ldo"]), NAN, dtype=odt))
        inp = dict(out0=_padded(torch.full((rows, C), NAN), s["ldo"], CANARY, odt))
        x = _bf((rows, C), g, 2.0)
        x[0, 0] = 0.0
        if not s["lv"]:
            inp["x"] = _padded(x, s["ldx"], JUNK)
            return inp
        lv = _bf((rows, C), g, 2.0, -3.0)
        inp["noise"] = _padded(_bf((rows, C), g), s["ldn"], JUNK)
        if s["view"]:                                                      # x = m[:, :z], logvar = m[:, z:]
            inp["moments"] = torch.cat((x, lv), 1)
        else:
            inp["x"], inp["logvar"] = _padded(x, s["ldx"], JUNK), _padded(lv, s["ldl"], JUNK)
        return inp
    raise KeyError(case.op)


def affine_operands(case, inp):
    """(x, logvar, noise) [rows, C] views of the affine case's buffers (logvar / noise None without them)."""
    s = case.shape
    C = s["C"]
    if not s["lv"]:
        return inp["x"][:, :C], None, None
    if s["view"]:
        return inp["moments"][:, :C], inp["moments"][:, C:2 * C], inp["noise"][:, :C]
    return inp["x"][:, :C], inp["logvar"][:, :C], inp["noise"][:, :C]


# --------------------------------------------------------------------------------------------------- reference
def _conv_nchw(x, w, b, mode):
    if mode == "s2":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
    if mode == "up":
        return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    if mode == "k1":
        return F.conv2d(x, w, b)
    return F.conv2d(x, w, b, padding=1)


def _rows(t):
    """[B, C, H, W] -> [B H W, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _pad_output(out0, width, dev):
    """The canary columns of an output buffer, as an output of kind "exact"."""
    return {"pad": (out0[:, width:].to(dev).double(), None, "exact")} if out0.shape[1] > width else {}


def conv_reference(case, inp, dev="cpu"):
    s = case.shape
    k = conv_geometry(s)[0]
    x, w = inp["_x"].to(dev).double(), inp["_w"].to(dev).double()
    b = inp["bias"].to(dev).double() if s["bias"] else None
    y = _rows(_conv_nchw(x, w, b, s["mode"]))
    A = _rows(_conv_nchw(x.abs(), w.abs(), None, s["mode"]))
    mag = 0.0
    if s["resid"] != "none":
        r = _rows(inp["_r"].to(dev).double())
        y, mag = y + r, r.abs()
    if b is not None:
        mag = mag + b.abs()[None]
    pre = 4 * math.sqrt(k * k * s["cin"]) * U * A + 2 * U * (y.abs() + mag)
    return {"out": (y, pre, s["out"]), **_pad_output(inp["out0"], s["cout"], dev)}


def gn_values(case, inp, dev="cpu"):
    s = case.shape
    return inp["x"].to(dev)[:, :s["C"]].reshape(s["B"], s["HW"], 32, s["C"] // 32)


def gn_reference(case, inp, dev="cpu"):
    s = case.shape
    B, HW, C = s["B"], s["HW"], s["C"]
    x = gn_values(case, inp, dev).double()
    mean = x.mean((1, 3), keepdim=True)
    var = ((x - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    gamma, beta = (inp[k].to(dev).double().reshape(1, 1, 32, C // 32) for k in ("gamma", "beta"))
    y = (x - mean) * rstd * gamma + beta
    pre = 16 * U * x.abs().max() * rstd * gamma.abs() + GN_ABS + torch.zeros_like(y)
    if s["swish"]:
        pre = pre * 1.1 + 4 * U * y.abs()
        y = y * torch.sigmoid(y)
    return {"y": (y.reshape(B * HW, C), pre.reshape(B * HW, C), "bf16"), **_pad_output(inp["y0"], C, dev)}


def softmax_reference(case, inp, dev="cpu"):
    s = case.shape
    n = s["n"]
    sc = inp["s"].to(dev)[:, :n].double()
    scale = float(torch.tensor(s["scale"], dtype=torch.float32))
    p = torch.softmax(sc * scale, 1)
    arg = (sc - sc.amax(1, keepdim=True)).abs() * scale
    pre = p * 2 * U * (arg + math.sqrt(n) + 4) + 1e-38
    out = {"p": (p, pre, "prob")}
    if s["ldp"] > n:
        out["pad"] = (torch.zeros(s["rows"], s["ldp"] - n, dtype=torch.float64, device=dev), None, "exact")
    return out


def affine_reference(case, inp, dev="cpu"):
    s = case.shape
    C = s["C"]
    a, b = (float(torch.tensor(v, dtype=torch.float32)) for v in (s["a"], s["b"]))
    x, lv, nz = affine_operands(case, {k: v.to(dev) for k, v in inp.items() if k != "out0"})
    if not s["lv"] and a == 1.0 and b == 0.0:
        ref = x if s["out"] == "f32" else x.to(torch.bfloat16)
        return {"out": (ref.double(), None, "exact"), **_pad_output(inp["out0"], C, dev)}
    x = x.double()
    v, e = x, torch.zeros_like(x)
    if s["lv"]:
        h = 0.5 * lv.double()
        t = torch.exp(h) * nz.double()
        v = x + t
        e = t.abs() * ((5 * h.abs() + EXP_ULPS) * U + 2 * U) + 2 * U * v.abs()
    o = a * v + b
    e = abs(a) * e + 2 * U * (a * v).abs() + 2 * U * o.abs()
    return {"out": (o, e, s["out"]), **_pad_output(inp["out0"], C, dev)}


REFERENCES = {"conv": conv_reference, "gn": gn_reference, "softmax": softmax_reference, "affine": affine_reference}


def reference(case, inp, dev="cpu") -> dict:
    """fp64 reference of every output of the case: name -> (ref, bound before the output rounding, kind)."""
    return REFERENCES[case.op](case, inp, dev)


# --------------------------------------------------------------------------------------------------- bounds
def bound(ref, pre, kind):
    if kind == "f32":
        return pre
    b = pre + 0.5 * G.ulp(ref, "bf16")
    if kind == "prob":
        b = b.clamp(min=2.0 ** -133)
    return b


def excess(got: torch.Tensor, ref: torch.Tensor, pre, kind: str):
    """(max |got - ref| / bound, number of elements NOT within the bound).  NaN / inf (an output element the kernel
    never wrote keeps its NaN) counts as over the bound.  Kind "exact": 0 or inf, and the unequal elements."""
    got = got.to(ref.device).double()
    if not ref.numel():
        return 0.0, 0
    if kind == "exact":
        same = got == ref
        return (0.0 if bool(same.all()) else math.inf), int((~same).sum().item())
    ratio = (got - ref).abs() / bound(ref, pre, kind)
    return ratio.max().item(), int((~(ratio <= 1)).sum().item())


def trunc_bf16(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (the slip of a store without rounding)."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def rounded_like_output(t: torch.Tensor, kind: str, trunc=False) -> torch.Tensor:
    """An fp32 value stored as the kernel stores it: round to nearest even to bf16, or as it is."""
    if kind in ("f32", "exact"):
        return t.float()
    return trunc_bf16(t) if trunc else t.float().to(torch.bfloat16)


# ----------------------------------------------------------------------------------- fp32 emulation (CPU)
def _conv_taps(case, inp, slip):
    """The kernel's own walk in fp32: tap by tap over the padded channel rows, padding by predicate, nearest-2x
    upsampling by index; with the named slip.  [M, Cout] before the epilogue."""
    s = case.shape
    k, stride, up, Ho, Wo, M = conv_geometry(s)
    B, H, W, cout = s["B"], s["H"], s["W"], s["cout"]
    cin_pad = ceil_to(s["cin"], 32)
    x = inp["x"][:, :cin_pad].float().reshape(B, H, W, cin_pad)
    w = inp["w"][:cout].float().reshape(cout, k, k, cin_pad)
    pad = 1 if k == 3 and (stride == 1 or slip == "s2_pad_leading_edge") else 0
    Hv, Wv = (2 * H, 2 * W) if up else (H, W)
    oy, ox = torch.arange(Ho), torch.arange(Wo)
    acc = torch.zeros(B, Ho, Wo, cout)
    for ky in range(k):
        for kx in range(k):
            iy, ix = oy * stride + ky - pad, ox * stride + kx - pad
            ok = ((iy >= 0) & (iy < Hv))[:, None] & ((ix >= 0) & (ix < Wv))[None, :]
            if up:
                sy, sx = ((iy + 1) >> 1, (ix + 1) >> 1) if slip == "up_parity" else (iy >> 1, ix >> 1)
            else:
                sy, sx = iy, ix
            gath = x[:, sy.clamp(0, H - 1)][:, :, sx.clamp(0, W - 1)] * ok[None, :, :, None]
            wt = w[:, kx, ky] if slip == "taps_transposed" else w[:, ky, kx]
            if slip == "last_k_step_dropped" and (ky, kx) == (k - 1, k - 1):
                gath, wt = gath[..., :-32], wt[:, :-32]
            acc += gath @ wt.T
    return acc.reshape(M, cout)


def conv_emulate(case, inp, slip=None):
    """slip None: torch's fp32 convolution of the bf16-exact operands; "taps" or a named slip: the kernel's walk."""
    s = case.shape
    cout, M = s["cout"], conv_geometry(s)[5]
    y = _rows(_conv_nchw(inp["_x"], inp["_w"], None, s["mode"])) if slip is None else _conv_taps(case, inp, slip)
    if s["bias"]:
        b = inp["bias"].clone()
        if slip == "bias_missing_in_scalar_tail":
            b[cout // 4 * 4:] = 0.0
        y = y + b[None]
    if s["resid"] != "none":
        r = inp["resid"] if s["resid"] == "separate" else inp["out0"]
        if slip == "resid_read_with_ldo":
            idx = torch.arange(M)[:, None] * s["ldo"] + torch.arange(cout)[None]
            y = y + r.reshape(-1)[idx]
        else:
            y = y + r[:, :cout]
    out = {"out": rounded_like_output(y, s["out"], slip == "bf16_store_truncates")}
    if s["ldo"] > cout:
        out["pad"] = inp["out0"][:, cout:]
    return out


def _chan_merge(a, b, guard=True):
    """Chan's merge of (count, mean, M2) triples per group, as chan_merge of ca_vae.hip; guard False: the slip of a
    count-0 partial merged as 0 / 0."""
    (n, mean, m2), (nb, meanb, m2b) = a, b
    if guard and nb == 0:
        return a
    nt = n + nb
    d, f = meanb - mean, torch.tensor(float(nb)) / torch.tensor(float(nt))      # 0 / 0 = NaN, as on the device
    return nt, mean + d * f, m2 + m2b + d * d * n * f


def gn_emulate(case, inp, slip=None):
    s = case.shape
    B, HW, C = s["B"], s["HW"], s["C"]
    cpg = C // 32
    x = gn_values(case, inp).float()
    n_chunks = s["n_chunks"] or groupnorm_chunks(HW)
    per = -(-HW // n_chunks)
    xs = x
    if slip == "last_chunk_rows_dropped":          # the statistics miss the rows of the last chunk that has any
        xs = x[:, :per * ((HW - 1) // per)]
    cnt = xs.shape[1] * cpg

    def flat(v):                                   # [B, 32, pixels * cpg], a group's values contiguous: torch then
        return v.permute(0, 2, 1, 3).reshape(B, 32, -1)    # sums them pairwise, to a few fp32 ulps like Welford

    def wide(v):
        return v.reshape(B, 1, 32, 1)

    if slip == "empty_chunk_merged":
        st = (0, torch.zeros(B, 32), torch.zeros(B, 32))
        for c in range(n_chunks):
            xc = flat(x[:, c * per:min(HW, (c + 1) * per)])
            if xc.shape[2]:
                m = xc.mean(2)
                part = (xc.shape[2], m, ((xc - m[:, :, None]) ** 2).sum(2))
            else:                                  # what the statistics launch leaves for a chunk without pixels
                part = (0, torch.full((B, 32), NAN), torch.full((B, 32), NAN))
            st = _chan_merge(st, part, guard=False)
        mean, var = wide(st[1]), wide(st[2] / st[0])
    else:
        xf = flat(xs)
        mean = xf.mean(2, keepdim=True)
        if slip == "one_pass_variance":
            var = (xf * xf).mean(2, keepdim=True) - mean * mean
        else:
            var = ((xf - mean) ** 2).sum(2, keepdim=True) / (cnt - 1 if slip == "unbiased_variance" else cnt)
        mean, var = wide(mean), wide(var)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(GN_EPS))
    if slip == "group_index_ignores_cpg":          # channel c takes the statistics of group c (mod 32), not c / cpg
        grp = torch.arange(C) % 32
        mean, rstd = (t.reshape(B, 1, 32)[:, :, grp].reshape(B, 1, 32, cpg) for t in (mean, rstd))
    gamma, beta = (inp[k].reshape(1, 1, 32, cpg) for k in ("gamma", "beta"))
    sc = rstd * gamma
    y = x * sc + (beta - mean * sc)                # the apply launch's form
    if s["swish"]:
        y = y / (1.0 + torch.exp(-y))
    out = {"y": rounded_like_output(y.reshape(B * HW, C), "bf16", slip == "bf16_store_truncates")}
    if s["ldy"] > C:
        out["pad"] = inp["y0"][:, C:]
    return out


def softmax_emulate(case, inp, slip=None):
    s = case.shape
    n = s["n"]
    sc = inp["s"][:, :n]
    scale = torch.tensor(s["scale"], dtype=torch.float32)
    mx = torch.zeros(s["rows"], 1) if slip == "no_max_subtraction" else sc.amax(1, keepdim=True)
    k = scale if slip == "log2e_missing" else scale * torch.tensor(1.4426950409, dtype=torch.float32)
    t = torch.exp2((sc - mx) * k)
    p = t * (1.0 / t.sum(1, keepdim=True))
    out = {"p": p.to(torch.bfloat16)}
    if s["ldp"] > n:
        out["pad"] = inp["p0"][:, n:] if slip == "padding_not_zeroed" else torch.zeros(s["rows"], s["ldp"] - n)
    return out


def affine_emulate(case, inp, slip=None):
    s = case.shape
    C = s["C"]
    a, b = (torch.tensor(v, dtype=torch.float32) for v in (s["a"], s["b"]))
    x, lv, nz = affine_operands(case, inp)
    v = x
    if s["lv"]:
        v = x + torch.exp((1.0 if slip == "std_is_exp_logvar" else 0.5) * lv) * nz
    v = a * (v + b) if slip == "shift_before_scale" else a * v + b
    out = {"out": rounded_like_output(v, s["out"])}
    if s["ldo"] > C:
        out["pad"] = torch.zeros_like(inp["out0"][:, C:]) if slip == "padding_columns_written" else inp["out0"][:, C:]
    return out


EMULATE = {"conv": conv_emulate, "gn": gn_emulate, "softmax": softmax_emulate, "affine": affine_emulate}


def emulate(case, inp, slip=None) -> dict:
    """The case's operation in fp32 on the CPU, stored as the kernel stores it; with a named slip of SLIPS."""
    return EMULATE[case.op](case, inp, slip)


# ----------------------------------------------------------------------------------- discrimination (CPU)
SLIPS = {
    # name: (case, the slip emulate() applies, output that must expose it)
    "conv: s2_pad_leading_edge": ("conv_5x7_c32_o48_s2_f32", "s2_pad_leading_edge", "out"),
    "conv: up_parity": ("conv_5x7_c96_o160_up_f32", "up_parity", "out"),
    "conv: taps_transposed": ("conv_5x7_c96_o48_s1_resid_f32", "taps_transposed", "out"),
    "conv: last_k_step_dropped": ("conv_16x16_c512_o160_s1_bf16", "last_k_step_dropped", "out"),
    "conv: last_k_step_dropped (one step)": ("conv1_k1_c32_one_step", "last_k_step_dropped", "out"),
    "conv: bias_missing_in_scalar_tail": ("conv4_o35_scalar_tail", "bias_missing_in_scalar_tail", "out"),
    "conv: resid_read_with_ldo": ("conv4_o80_no_bias_resid", "resid_read_with_ldo", "out"),
    "conv: bf16_store_truncates": ("conv4_o36_partial_fragment_bf16", "bf16_store_truncates", "out"),
    "gn: one_pass_variance": ("gn_C64_hw4096_mean1000_unrounded", "one_pass_variance", "y"),
    "gn: unbiased_variance": ("gn_C64_hw7_f32", "unbiased_variance", "y"),
    "gn: last_chunk_rows_dropped": ("gn_C32_hw1025_f32", "last_chunk_rows_dropped", "y"),
    "gn: empty_chunk_merged": ("gn_C32_hw5_7_chunks", "empty_chunk_merged", "y"),
    "gn: empty_chunk_merged (1024 chunks)": ("gn_C128_hw1000_1024_chunks", "empty_chunk_merged", "y"),
    "gn: group_index_ignores_cpg": ("gn_C64_hw7_f32", "group_index_ignores_cpg", "y"),
    "gn: bf16_store_truncates": ("gn_C128_hw512_f32_swish", "bf16_store_truncates", "y"),
    "softmax: no_max_subtraction": ("softmax_n257", "no_max_subtraction", "p"),
    "softmax: log2e_missing": ("softmax_n63", "log2e_missing", "p"),
    "softmax: padding_not_zeroed": ("softmax_n65_pad300", "padding_not_zeroed", "pad"),
    "affine: std_is_exp_logvar": ("affine_sample_bf16_moments_view", "std_is_exp_logvar", "out"),
    "affine: shift_before_scale": ("affine_decode_f32", "shift_before_scale", "out"),
    "affine: padding_columns_written": ("affine_cast_bf16_padded", "padding_columns_written", "pad"),
}


def over_bounds(case, inp, got: dict, ref: dict = None) -> dict:
    """Elements over the bound per output of the case."""
    ref = ref or reference(case, inp)
    assert set(ref) == set(got), (case.id, set(ref) ^ set(got))
    return {k: excess(got[k], r, pre, kind)[1] for k, (r, pre, kind) in ref.items()}


def discrimination(name: str):
    """On the CPU: the faithful fp32 emulation passes every bound of the slip's case; the same emulation with the
    named slip puts elements of the output that carries it over the bound.  Returns (the faithful emulation passes,
    elements over the bound with the slip)."""
    cid, slip, which = SLIPS[name]
    case = BY_ID[cid]
    inp = make_inputs(case)
    ref = reference(case, inp)
    faithful = "taps" if case.op == "conv" else None       # the walk the slip is applied to, without the slip
    ok = not any(over_bounds(case, inp, emulate(case, inp, faithful), ref).values())
    return ok, over_bounds(case, inp, emulate(case, inp, slip), ref)[which]
