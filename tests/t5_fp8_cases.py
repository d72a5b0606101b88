"""Launch cases of the two e4m3 producers of the T5 encoder's fp8 mode (ca_t5_rmsnorm_f32in_fp8, ca_gated_mul_fp8), their
inputs, a faithful fp32 emulation of each with the named slips, derived bounds against fp64, and the CPU emulation of
the whole fp8 forward that is the yardstick of tests/test_t5_fp8_model_gpu.py.

Imported by tests/test_t5_fp8_kernels_gpu.py, tests/test_t5_fp8_model_gpu.py and tests/test_t5_fp8_cases_cpu.py (the
emulation sits inside every bound, every slip leaves it).  Nothing here touches torch.cuda.

What a producer computes.  With y the fp32 row (the norm's x * rsqrt(mean(x^2) + eps) * w, never rounded to bf16; the
exact product float(g) * float(u)):  amax = max |y|;  scale = amax * fl(1 / 448) if amax > 0 else 1;
inv = 1 / scale;  byte = e4m3fn(clamp(y * inv, -448, 448)), round to nearest even.

Bounds (u = 2^-24, every fp32 operation charged 2 u of its running magnitude, as in t5_cases.py; second-order terms
are covered by 1 + 2^-6):

  y (rmsnorm)    the sum of squares: a thread adds 8 squares per pass over the row (a square, three levels of a tree,
                 one accumulation: 5 roundings in sequence per 2048 columns), then 6 exchanges in the wave and 2 across
                 the waves: SUMSQ_OPS(H) = 5 ceil(H / 2048) + 8 roundings of 2 u on a quantity whose inverse square
                 root is taken (half of it): u SUMSQ_OPS(H).  / H, + eps, sqrt, 1 / x and the two products:
                 2 u (NORM_ULPS + 2), as t5_cases.py charges ca_t5_rmsnorm_f32in.  Y_REL(H) = their sum.
  y (gated mul)  bf16 x bf16 has 16 significant bits: exact in fp32.  Y_REL = 0.
  scale          amax inherits Y_REL; the rounded constant 1 / 448 and the product: 4 u.
                 |scale - amax64 / 448| <= (Y_REL + 4 u) amax64 / 448.
  value          byte * scale against the fp64 y.  z = y * inv carries Y_REL and two more operations (1 / scale, the
                 product): F = Y_REL + 4 u, relative to |y|.  The e4m3 rounding of z moves it by half a step: in the
                 normal range (|z| >= 2^-6; three mantissa bits) at most 2^-4 |z|, in the subnormal range (step 2^-9)
                 2^-10.  An fp32 error that flips a rounding decision adds what it moved z by, which F covers.
                 |byte * scale - y| <= (2^-4 + F) |y|            where |y| / scale >= 2^-6
                                       scale 2^-10 + F |y|       below.
  A zero row: scale 1, every byte +-0, nothing non-finite.

Slips.  ``scale_from_bf16``: the row passes through bf16 before the maximum is taken (2^-9 on the scale, against a few
u).  ``amax_over_240``: the e4m3fnuz range instead of e4m3fn's 448.  ``truncate``: the e4m3 mantissa cut instead of
rounded (an error of up to a whole step).  ``no_saturation``: the clamp to +-448 missing.  With the kernel's own scale
the largest |z| of a finite row is 448 (1 + 3 u), which rounds to 448 with or without the clamp, so that slip cannot
show on any row whose maximum the kernel has found; it shows where the scale is too small for the row, which is what a
maximum taken over only part of the row gives.  ``pack_row`` therefore takes an optional ``scale_of`` -- the columns
the maximum is taken over -- and the saturation check runs on the outlier family with the outlier left out of it: a
saturating store then holds +-448 scale there (finite, wrong, visible in the value bound), a non-saturating one NaN.
"""
from __future__ import annotations

import math
import zlib

import torch

import gemm_route_cases as G
import t5_ref

U = G.U
NORM_ULPS = G.NORM_ULPS
SECOND_ORDER = 1 + 2.0 ** -6
EPS = 1e-6
E4M3_MAX = 448.0
E4M3_MIN_NORMAL = 2.0 ** -6
HALF_STEP_REL = 2.0 ** -4        # half an e4m3 step relative to the value, normal range
HALF_STEP_SUB = 2.0 ** -10       # half an e4m3 step in the subnormal range (times the scale)

# Measured on MI355X, tests/test_t5_fp8_kernels_gpu.py (largest printed error / bound): rmsnorm scale 0.112, value 0.985;
# gated product scale 0.398, value 0.985 (an e4m3 tie: half a step, under the second-order factor).  No constant above was
# changed after a measurement.
# With the later cases: the grid wrap (65541 x 264) rmsnorm scale 0.147, value 0.985 (4 of 17 302 824 bytes differ from the
# CPU emulation, inside the bound), gated product scale 0.422, value 0.985 (no byte differs); widths 2056 and 8: scale at
# most 0.420, value at most 0.984.

RMS_CASES = [(H, rows, strided) for H in (256, 4096) for rows in (1, 5, 257) for strided in (False, True)]
GATE_CASES = [(C, rows) for C in (512, 10240) for rows in (1, 3, 130)]
# the column loops step 2048 elements per pass: 2056 is one whole pass and a second one that thread 0 alone enters; 8 is
# the entry points' minimum width (one thread works, 255 bring 0 to the reductions)
RMS_CASES += [(H, rows, strided) for H in (2056, 8) for rows in (1, 7) for strided in (False, True)]
GATE_CASES += [(C, rows) for C in (2056, 8) for rows in (1, 7)]
# grid wrap: both producers launch one workgroup per row up to 65536 (`rows < 65536 ? rows : 65536`, tx_row_blocks) and
# walk the rest with the grid's stride, with the 4-float `red` array of tx_block_sum / tx_block_max reused
ROW_GRID_CAP = 65536
WRAP_ROWS, WRAP_WIDTH = ROW_GRID_CAP + 5, 264
WRAP_CASES = {"t5_rmsnorm_fp8": (WRAP_ROWS, ROW_GRID_CAP, 1, dict(H=WRAP_WIDTH, rows=WRAP_ROWS)),
              "gated_mul_fp8": (WRAP_ROWS, ROW_GRID_CAP, 1, dict(C=WRAP_WIDTH, rows=WRAP_ROWS))}
FAMILIES = ("normal", "zero", "outlier")   # row r belongs to FAMILIES[r % 3]; a one-row case runs once per family
OUTLIER = 1e4
SLIPS = ("scale_from_bf16", "amax_over_240", "truncate")


def _gen(tag: str) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(zlib.crc32(tag.encode()))
    return g


def bf16r(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def row_families(rows: int, first: int = 0):
    return [FAMILIES[(first + r) % 3] for r in range(rows)]


def outlier_columns(rows: int, cols: int, tag: str) -> torch.Tensor:
    """One seeded column per row: where an ``outlier`` row has its large element."""
    return torch.randint(0, cols, (rows,), generator=_gen(f"t5fp8.outlier.{tag}.{rows}.{cols}"))


def rms_inputs(H: int, rows: int, first: int = 0):
    """(x fp32 [rows, H], w fp32 [H] around 1, families).  ``normal``: unit normal; ``zero``: all zero; ``outlier``:
    one element 1e4 times the rest.  The norm keeps that ratio, so on the e4m3 grid the maximum sits at 448 and the rest
    at 448 / 1e4 = 0.045 times a unit normal: around the smallest normal (2^-6 = 0.0156), a good part of it in the
    subnormals (step 2^-9 = 0.002) or rounded to zero."""
    g = _gen(f"t5fp8.rms.{H}.{rows}.{first}")
    x = torch.randn(rows, H, generator=g)
    w = 1 + 0.25 * (torch.rand(H, generator=g) * 2 - 1)
    fam = row_families(rows, first)
    col = outlier_columns(rows, H, "rms")
    for r, f in enumerate(fam):
        if f == "zero":
            x[r] = 0
        elif f == "outlier":
            x[r] *= 0.01
            x[r, col[r]] = 0.01 * OUTLIER * (1 if r % 2 else -1)
    return x.to(torch.float32), w.to(torch.float32), fam


def gate_inputs(C: int, rows: int, first: int = 0):
    """(g, u bf16 values as fp32 [rows, C], families); an ``outlier`` row has one product 1e4 times the rest."""
    gen = _gen(f"t5fp8.gate.{C}.{rows}.{first}")
    g, u = torch.randn(rows, C, generator=gen), torch.randn(rows, C, generator=gen)
    fam = row_families(rows, first)
    col = outlier_columns(rows, C, "gate")
    for r, f in enumerate(fam):
        if f == "zero":
            (g if r % 2 else u)[r] = 0          # one factor zero is enough (the other keeps its signs: -0 products)
        elif f == "outlier":
            g[r, col[r]], u[r, col[r]] = 100.0, 100.0 * (1 if r % 2 else -1)
    return bf16r(g), bf16r(u), fam


# ---------------------------------------------------------------------------------------------------------- references
def sumsq_ops(H: int) -> int:
    return 5 * math.ceil(H / 2048) + 8


def y_rel_rmsnorm(H: int) -> float:
    return U * sumsq_ops(H) + 2 * U * (NORM_ULPS + 2)


def rmsnorm_y64(x, w, eps=EPS):
    return t5_ref.rmsnorm(x.double(), w.double(), eps)


def gated_y64(g, u):
    return g.double() * u.double()


def fp8_reference(y64: torch.Tensor, y_rel: float):
    """(scale64 [rows], scale bound [rows], value bound [rows, cols]) of a producer whose fp32 row is within y_rel of
    the fp64 row ``y64``."""
    amax = y64.abs().amax(-1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    scale_bound = (y_rel + 4 * U) * scale * SECOND_ORDER
    f = y_rel + 4 * U
    a = y64.abs()
    normal = a / scale[:, None] >= E4M3_MIN_NORMAL
    bound = torch.where(normal, (HALF_STEP_REL + f) * a, scale[:, None] * HALF_STEP_SUB + f * a) * SECOND_ORDER
    return scale, scale_bound, bound


def dequant(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes [rows, cols] and fp32 scales [rows] -> fp64 values (decoded by torch on the CPU)."""
    return q.cpu().contiguous().view(torch.float8_e4m3fn).double() * scale.cpu().double()[:, None]


def ratios(q, scale, y64, y_rel):
    """(scale error / bound, value error / bound) maxima; inf where a byte decodes to a non-finite value."""
    ref_scale, scale_bound, bound = fp8_reference(y64, y_rel)
    got = dequant(q, scale)
    if not torch.isfinite(got).all() or not torch.isfinite(scale).all():
        return math.inf, math.inf
    rs = float(((scale.cpu().double() - ref_scale).abs() / scale_bound).max())
    tiny = torch.finfo(torch.float64).tiny
    rv = float(((got - y64).abs() / bound.clamp_min(tiny)).max())     # (a zero element has a zero bound: 0 / tiny = 0)
    return rs, rv


# ---------------------------------------------------------------------------------------------------------- emulations
def _e4m3_truncated(z: torch.Tensor) -> torch.Tensor:
    """e4m3 with the mantissa cut toward zero, as fp32 values (exact: powers of two and small integers)."""
    a = z.abs().double().clamp(max=E4M3_MAX)
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -40))).clamp_min(-6.0)
    step = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 3)
    return (torch.sign(z).double() * torch.floor(a / step) * step).to(torch.float32)


def pack_row(y: torch.Tensor, slip=None, scale_of=None):
    """The shared tail of both kernels on fp32 rows y [rows, cols]: (bytes uint8, scale fp32 [rows]).  ``scale_of``: a
    boolean mask [rows, cols] of the elements the maximum is taken over (None: all of them, as the kernels do)."""
    f = torch.float32
    y = y.to(f)
    src = bf16r(y) if slip == "scale_from_bf16" else y
    if scale_of is not None:
        src = torch.where(scale_of, src, torch.zeros_like(src))
    amax = src.abs().amax(-1)
    k = torch.tensor(1.0 / 240.0 if slip == "amax_over_240" else 1.0 / E4M3_MAX, dtype=f)
    scale = torch.where(amax > 0, amax * k, torch.ones_like(amax))
    z = y * (1.0 / scale)[:, None]
    if slip != "no_saturation":
        z = z.clamp(-E4M3_MAX, E4M3_MAX)
    if slip == "truncate":
        q = _e4m3_truncated(z).to(torch.float8_e4m3fn)        # representable: the cast is exact
    else:
        q = z.to(torch.float8_e4m3fn)                         # round to nearest even; beyond 464 it gives NaN
    return q.view(torch.uint8), scale


def rmsnorm_y32(x, w, eps=EPS):
    f = torch.float32
    x = x.to(f)
    rs = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / x.shape[1] + torch.tensor(eps, dtype=f))
    return x * rs * w.to(f)


def rmsnorm_fp8_emulated(x, w, eps=EPS, slip=None, scale_of=None):
    return pack_row(rmsnorm_y32(x, w, eps), slip, scale_of)


def gated_mul_fp8_emulated(g, u, slip=None, scale_of=None):
    return pack_row(g.to(torch.float32) * u.to(torch.float32), slip, scale_of)


# ---------------------------------------------------------------------------------------------------------- the model
def quantise_rows64(t: torch.Tensor) -> torch.Tensor:
    """An fp64 matrix through the row quantiser and back: the scale rule in fp32 as the kernels form it, torch's
    float8_e4m3fn cast, the dequantised values in fp64."""
    q, scale = pack_row(t.to(torch.float32))
    return q.view(torch.float8_e4m3fn).double() * scale.double()[:, None]


def encoder_fp8_emulated(sd, ids, num_heads, num_layers, fp8=("qkv", "o", "wi", "wo"), eps=EPS):
    """t5_ref.encoder with the fp8 mode's quantisation points and nothing else: the weight rows and the activation rows
    in front of every projection named in ``fp8`` pass through e4m3 with one scale per row; all arithmetic between them
    is exact fp64 (no bf16 rounding of the GEMM outputs, the attention output or the stream).  Not the code under test:
    it shares nothing with conceptattention_amd/t5.py."""
    d = torch.float64
    w = {k: v.to(d) for k, v in sd.items()}
    n_seq, length = ids.shape

    def lin(name, a, *keys):
        m = torch.cat([w[k] for k in keys])
        if name in fp8:
            a, m = quantise_rows64(a), quantise_rows64(m)
        return a @ m.t()
    x = w["shared.weight"][ids.reshape(-1)]
    bias = t5_ref.bias_table(w["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], length)
    for i in range(num_layers):
        a, f = f"encoder.block.{i}.layer.0", f"encoder.block.{i}.layer.1"
        h = t5_ref.rmsnorm(x, w[f"{a}.layer_norm.weight"], eps)
        q, k, v = lin("qkv", h, *(f"{a}.SelfAttention.{n}.weight" for n in "qkv")).chunk(3, -1)
        x = x + lin("o", t5_ref.attention(q, k, v, bias, n_seq, num_heads), f"{a}.SelfAttention.o.weight")
        h = t5_ref.rmsnorm(x, w[f"{f}.layer_norm.weight"], eps)
        u, g = lin("wi", h, f"{f}.DenseReluDense.wi_1.weight", f"{f}.DenseReluDense.wi_0.weight").chunk(2, -1)
        x = x + lin("wo", t5_ref.gelu_tanh(g) * u, f"{f}.DenseReluDense.wo.weight")
    return t5_ref.rmsnorm(x, w["encoder.final_layer_norm.weight"], eps).reshape(n_seq, length, -1)


PROJECTION_KEYS = ("SelfAttention.q.weight", "SelfAttention.k.weight", "SelfAttention.v.weight", "SelfAttention.o.weight",
                   "DenseReluDense.wi_0.weight", "DenseReluDense.wi_1.weight", "DenseReluDense.wo.weight")


def e4m3_state_dict(sd: dict) -> dict:
    """``sd`` with every projection weight cast to torch.float8_e4m3fn (a plain cast, no scale: what an unscaled e4m3fn
    checkpoint holds); the embedding, the norms and the bias table stay as they are."""
    return {k: (v.to(torch.float8_e4m3fn) if k.endswith(PROJECTION_KEYS) else v) for k, v in sd.items()}
