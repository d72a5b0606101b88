"""Each autoencoder kernel against fp64 torch on the CPU, on bf16-representable inputs (one GroupNorm case excepted,
which needs unrounded fp32 values to tell a one-pass variance from a stable one).

Bounds are derived, not tuned:

* convolution: operands are exact in bf16 and a bf16 x bf16 product is exact in fp32, so the only error before the
  epilogue is the fp32 accumulation: K additions, each within 2^-24 of a partial sum that is at most
  A = sum |x| |w| -- sqrt(K) 2^-24 A for roundings of random sign, taken 4 x.  Bias and residual add two roundings
  (2^-23 of |y| + |resid|), a bf16 output one more (1 ulp = 2^-8 |y|).
* GroupNorm: y is rounded to bf16 (2^-8 |y|); x - mean carries a few fp32 ulps of max|x| (the Welford mean and the
  subtraction), scaled by rstd |gamma|: 16 x 2^-24 max|x| rstd |gamma|.
* softmax: one bf16 rounding of p (2^-8 p) plus the exp2 argument's rounding, 2^-23 |scale s| relative.
* attention block: six bf16 rounding points (the normed input, q / k, V^T, P, the attention output, the folded bias),
  each 2^-8 relative; a score error d changes a probability by at most 2 d p.  To first order the update is within
  2^-8 (6 + 2 max|scale s|) of its magnitude.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conceptattention_amd import ops, vae  # noqa: E402

DEV = "cuda"
U8, U24 = 2.0 ** -8, 2.0 ** -24


def _bf(shape, gen, scale=1.0, shift=0.0):
    return ((torch.randn(shape, generator=gen) * scale + shift).to(torch.bfloat16)).float()


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _conv_ref(x, w, b, mode):
    """x [B,Cin,H,W], w [Cout,Cin,k,k] fp64."""
    if mode == "s2":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
    if mode == "up":
        return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    if mode == "k1":
        return F.conv2d(x, w, b)
    return F.conv2d(x, w, b, padding=1)


CONV_CASES = [
    # H, W, Cin, Cout, mode, resid, out_f32
    (1, 1, 32, 16, "s1", False, True),
    (5, 7, 96, 48, "s1", True, True),
    (16, 16, 512, 160, "s1", False, False),
    (33, 17, 32, 160, "s1", True, False),
    (33, 17, 96, 16, "s1", False, True),
    (5, 7, 32, 48, "s2", False, True),
    (16, 16, 96, 160, "s2", True, True),
    (33, 17, 512, 16, "s2", False, False),
    (5, 7, 96, 160, "up", False, True),
    (16, 16, 32, 48, "up", True, False),
    (1, 1, 32, 16, "up", False, True),
    (5, 7, 3, 48, "s1", False, True),       # a padded Cin (3 real channels in a 32-wide row)
    (16, 16, 16, 160, "s1", True, True),    # the decoder's conv_in
    (16, 16, 32, 3, "s1", False, True),     # a padded Cout (the scalar store path)
    (33, 17, 96, 3, "s1", False, False),
    (33, 17, 96, 160, "k1", True, True),    # nin_shortcut
]


@pytest.mark.parametrize("H,W,cin,cout,mode,resid,out_f32", CONV_CASES)
def test_conv_against_fp64(H, W, cin, cout, mode, resid, out_f32):
    B, k = 2, 1 if mode == "k1" else 3
    g = _gen(H * 1000 + cin + cout)
    x = _bf((B, cin, H, W), g)
    w = _bf((cout, cin, k, k), g, 1.0 / math.sqrt(cin * k * k))
    b = _bf((cout,), g, 0.1)
    ref = _conv_ref(x.double(), w.double(), b.double(), mode)
    A = _conv_ref(x.double().abs(), w.double().abs(), None, mode)
    Ho, Wo = ref.shape[2], ref.shape[3]
    assert (Ho, Wo) == ops.conv_out_hw(H, W, k, 2 if mode == "s2" else 1, mode == "up")
    r = _bf((B, cout, Ho, Wo), g) if resid else None
    if resid:
        ref = ref + r.double()
    cin_pad = (cin + 31) // 32 * 32
    xd = torch.zeros(B, H, W, cin_pad, dtype=torch.bfloat16, device=DEV)
    xd[..., :cin] = x.permute(0, 2, 3, 1).to(DEV, torch.bfloat16)
    out = torch.full((B, Ho, Wo, cout), float("nan"), device=DEV, dtype=torch.float32 if out_f32 else torch.bfloat16)
    rd = r.permute(0, 2, 3, 1).contiguous().to(DEV) if resid else None
    ops.conv2d_nhwc(xd, ops.pack_conv_weight(w).to(DEV), b.to(DEV), out, cout, ksize=k, stride=2 if mode == "s2" else 1,
                    upsample=mode == "up", resid=rd)
    got = out.double().cpu().permute(0, 3, 1, 2)
    K = k * k * cin
    tol = 4 * math.sqrt(K) * U24 * A + 2 * U24 * (ref.abs() + (r.double().abs() if resid else 0) + b.double().abs()[None, :, None, None])
    if not out_f32:
        tol = tol + U8 * ref.abs()
    err = (got - ref).abs()
    print("conv", (H, W, cin, cout, mode), "max err", err.max().item(), "worst err/tol", (err / tol).max().item())
    assert torch.isfinite(got).all()
    assert (err <= tol).all()


GN_CASES = [
    # C, pixels, x fp32, swish, mean, std
    (32, 1, True, True, 0.0, 1.0),
    (64, 7, True, False, 0.0, 1.0),
    (512, 7, False, True, 0.0, 1.0),
    (32, 4096, True, True, 0.0, 1.0),
    (64, 4096, False, True, 0.5, 2.0),
    (512, 4096, True, False, 0.0, 1.0),
    (32, 70000, True, True, 0.0, 1.0),
    (512, 70000, True, True, 0.0, 1.0),
    (64, 4096, True, False, 100.0, 1.0),    # a large mean; on bf16-representable values (steps of 0.5 at 100)
    # fp32 values that are NOT rounded to bf16, mean 1000, std 1: E[x^2] ~ 1e6 has an fp32 ulp of 0.06, so the
    # E[x^2] - E[x]^2 form gets a variance of 1 wrong by several percent -- tens of times the bound below
    (64, 4096, True, False, 1000.0, 1.0),
]


@pytest.mark.parametrize("C,hw,x_f32,swish,mean,std", GN_CASES)
def test_groupnorm_against_fp64(C, hw, x_f32, swish, mean, std):
    B = 2
    g = _gen(C + hw)
    x = _bf((B, hw, C), g, std, mean) if mean < 1000 else torch.randn((B, hw, C), generator=g) * std + mean
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    xd = x.double().transpose(1, 2)                                     # [B, C, hw]
    ref = F.group_norm(xd, 32, gamma.double(), beta.double(), eps=1e-6).transpose(1, 2)
    rstd = 1.0 / torch.sqrt(xd.reshape(B, 32, -1).var(dim=2, unbiased=False) + 1e-6)      # [B, 32]
    rstd_c = rstd.repeat_interleave(C // 32, dim=1)[:, None, :]
    tol = 16 * U24 * x.abs().max().item() * rstd_c * gamma.double().abs() + 1e-6
    pre = ref
    if swish:
        ref = ref * torch.sigmoid(ref)          # |d swish / dy| <= 1.1
        tol = tol * 1.1 + 4 * U24 * pre.abs()   # the exp / divide of the sigmoid
    tol = tol + U8 * ref.abs()
    out = torch.full((B, hw, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.groupnorm_nhwc(x.to(DEV, torch.float32 if x_f32 else torch.bfloat16), gamma.to(DEV), beta.to(DEV), out, swish)
    got = out.double().cpu()
    err = (got - ref).abs()
    print("groupnorm", (C, hw, x_f32, swish, mean), "max err", err.max().item(), "worst err/tol", (err / tol).max().item())
    assert torch.isfinite(got).all()
    assert (err <= tol).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_softmax_rows_against_fp64(n):
    rows, ld, scale = 5, (n + 63) // 64 * 64 + 64, 0.125
    g = _gen(n)
    s = torch.randn(rows, n, generator=g) * 8
    s[2, n // 2] = s[2].max() + 60 / scale                      # one score 60 nats above the rest
    sd = torch.full((rows, ld), float("nan"), device=DEV)
    sd[:, :n] = s.to(DEV)
    p = torch.full((rows, ld), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.softmax_rows(sd, p, n, scale)
    got = p.double().cpu()
    ref = torch.softmax(s.double() * scale, dim=1)
    assert (got[:, n:] == 0).all()
    arg = (s.double() - s.double().max(dim=1, keepdim=True).values).abs() * scale
    tol = ref * (U8 + 2 * U24 * (arg + n ** 0.5 + 4)) + 1e-38
    tol = torch.maximum(tol, torch.full_like(tol, 2.0 ** -133))     # bf16's smallest subnormal: tinier values flush
    err = (got[:, :n] - ref).abs()
    print("softmax", n, "max err", err.max().item(), "worst err/tol", (err / tol).max().item())
    assert (err <= tol).all()
    assert got[2, n // 2] == pytest.approx(1.0, abs=U8)


def _attn_weights(C, g):
    t = {}
    for n in ("q", "k", "v", "proj_out"):
        t[f"a.{n}.weight"] = _bf((C, C, 1, 1), g, 1.0 / math.sqrt(C))
        t[f"a.{n}.bias"] = _bf((C,), g, 0.1)
    t["a.norm.weight"] = 1 + 0.1 * torch.randn(C, generator=g)
    t["a.norm.bias"] = 0.1 * torch.randn(C, generator=g)
    return t


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("hw", [(2, 2), (10, 10), (64, 64)])
def test_attention_block_against_fp64(C, hw):
    H, W = hw
    B, T = 2, H * W
    g = _gen(C + T)
    t = _attn_weights(C, g)
    x = _bf((B, H, W, C), g)
    xd = x.to(DEV).clone()
    vae.attention_block(xd, vae.pack_attention(t, "a", DEV), "a", vae.attention_workspace(T, C, DEV))
    got = xd.double().cpu()
    d = {k: v.double() for k, v in t.items()}
    xr = x.double().reshape(B, T, C)
    hn = F.group_norm(xr.transpose(1, 2), 32, d["a.norm.weight"], d["a.norm.bias"], eps=1e-6).transpose(1, 2)
    q, k, v = (hn @ d[f"a.{n}.weight"].reshape(C, C).T + d[f"a.{n}.bias"] for n in "qkv")
    s = q @ k.transpose(1, 2) / math.sqrt(C)
    upd = torch.softmax(s, dim=-1) @ v @ d["a.proj_out.weight"].reshape(C, C).T + d["a.proj_out.bias"]
    ref = (xr + upd).reshape(B, H, W, C)
    tol = U8 * (6 + 2 * s.abs().max().item()) * upd.abs().max().item() + 4 * U24 * ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print("attention", (C, T), "max err", err, "tol", tol, "max |scale s|", s.abs().max().item())
    assert torch.isfinite(got).all()
    assert err <= tol


def test_conv_output_past_4gib_is_addressed_in_64_bits():
    """32 -> 32 channels, fp32 output of 5800 x 5800 pixels = 4.3 GB; sampled pixels, the very last among them, against
    fp64 on the CPU for those pixels only."""
    H = W = 5800
    g = _gen(7)
    w, b = _bf((32, 32, 3, 3), g, 1.0 / math.sqrt(288)), _bf((32,), g, 0.1)
    x = torch.empty(1, H, W, 32, device=DEV, dtype=torch.bfloat16)
    x.view(-1).copy_((torch.arange(H * W * 32, device=DEV) * 0.6180339887 % 2.0 - 1.0).to(torch.bfloat16))
    out = torch.empty(1, H, W, 32, device=DEV, dtype=torch.float32)
    assert out.numel() * 4 > 2 ** 32
    ops.conv2d_nhwc(x, ops.pack_conv_weight(w).to(DEV), b.to(DEV), out, 32)
    pts = [(0, 0), (H - 1, W - 1), (H - 1, 0), (0, W - 1), (H // 2, W // 2), (4628, 1000), (4629, 0), (H - 2, W - 3)]
    for y, xx in pts:
        patch = torch.zeros(3, 3, 32, dtype=torch.float64)
        for ky in range(3):
            for kx in range(3):
                iy, ix = y + ky - 1, xx + kx - 1
                if 0 <= iy < H and 0 <= ix < W:
                    patch[ky, kx] = x[0, iy, ix].double().cpu()
        wd = w.double().permute(0, 2, 3, 1)                         # [Cout, ky, kx, Cin]
        ref = (wd * patch[None]).sum(dim=(1, 2, 3)) + b.double()
        A = (wd.abs() * patch[None].abs()).sum(dim=(1, 2, 3))
        tol = 4 * math.sqrt(288) * U24 * A + 2 * U24 * (ref.abs() + b.double().abs())
        got = out[0, y, xx].double().cpu()
        assert ((got - ref).abs() <= tol).all(), (y, xx)
