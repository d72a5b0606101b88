"""The value-range edges of the five e4m3 producers (ca_ln_modulate_fp8, ca_ln_modulate_f32in_fp8, ca_quantize_rows_fp8,
ca_t5_rmsnorm_f32in_fp8, ca_gated_mul_fp8): the case table, an fp32 emulation of each with the named slips, and the
contract of include/conceptattn.h ("e4m3 value range") as a checker that the CPU test runs on the emulation and the GPU
test on what the kernels wrote.  Extends t5_fp8_cases.py and rowop_cases.py, whose families hold finite rows only.
Imported by tests/test_fp8_edge_cases_cpu.py and tests/test_fp8_edges_gpu.py.  Nothing here touches torch.cuda.

The contract, with y the fp32 row a producer quantises (t5_fp8_cases.py):
  P1  finite rows with amax * fl(1 / 448) >= 2^-126: bytes and scales as before the contract was stated (the existing
      tests and tests/golden/text_parent_records.npz hold them).
  P2  y[c] NaN (any sign, any payload, quiet or signalling)  ->  byte[c] is an e4m3 NaN (0x7F or 0xFF).
  P3  the scale is taken over the non-NaN elements: the scale and every other byte of the row are those of the same row
      with its NaN elements set to 0, bit for bit; an all-NaN row has scale 1.
  P4  a row with +-inf in y: scale +inf, NaN bytes at the infinite positions (inf * (1 / inf) = NaN), +-0 with the
      element's sign at the finite ones.
  P5  a finite non-zero row: scale finite, positive and normal, every byte finite, |byte * scale - y| inside the value
      bound of t5_fp8_cases.py computed with the kernel's own scale; the scale inside its bound where amax / 448 >= 2^-126
      and in [amax / 448, 2^-126] below (the floor that keeps 1 / scale finite).
  rows  a special row changes no other row (one workgroup holds four rows, or walks many through one `red` array).

How the statements are checked.  Every case is launched twice: on its inputs, and on the same inputs with every special
cell replaced by a value that makes its y zero (``replaced``).  P3 and ``rows`` compare the two launches by bits; P2 and
P4 are statements about the first alone.  A NaN row whose other elements are all zero (a NaN in the x of a norm makes
the whole row NaN; an inf in the x of the RMS norm leaves inf * 0 = NaN in its column and x * 0 elsewhere) has no
replaced twin: there P3 is stated directly (scale 1, +-0 with the element's sign).

Row families.  ``plain``, ``zero``, ``nan_q`` (0x7FC0), ``nan_s`` (0x7F81, signalling), ``nan_neg`` (0xFFC0), ``pinf``,
``ninf``, ``tiny``, ``all_nan``.  The special cells of a row sit at column 0, the last column and the first column of the
kernel's second pass over the row (512 for the one-wave-per-row kernels of ca_rowops.hip, 2048 for the workgroup-per-row
kernels of ca_t5.hip).  ``tiny`` elements come from {0, +-2^-125 .. +-2^-120}, at least a third zeros: all normal numbers,
so the case does not depend on whether a kernel keeps fp32 subnormals; amax / 448 < 2^-126 for every such row.
  quantize_rows   the families are rows of x.
  gated product   the families are rows of g (u plain); ``pinf`` / ``ninf`` rows hold an infinite g at column 0 and finite
                  operands whose product overflows fp32 (+-2^100 * 2^100) at the other special cells; ``zero`` rows a zero
                  g and, at the special cells, operands whose product underflows to exact zero (2^-100 * 2^-100); ``tiny``
                  rows a tiny g under u in {1, -1, 1.5}.
  RMS norm        the families are rows of x: a NaN makes the whole row NaN, an inf leaves one NaN.  The weight is
                  2^-10 (1 +- 0.25), so that a tiny x (times 1 / sqrt(eps) = 1000) gives a tiny y; per-row scales make
                  that harmless for the other rows.  Variants ``w_nan`` / ``w_inf``: one NaN (inf) column of the weight,
                  which is a NaN (inf) element in every row.
  LayerNorm       four segments of rows: 0-3 and 4-7 plain modulation, 8-9 shift 0 and scale -1 (y = 0 * t + 0: zero rows),
                  10-11 scale -1 and a shift drawn from the tiny set (y = shift).  A NaN or inf in x makes the whole row
                  NaN.  Variant ``mod``: +-inf in two columns of segment 0's shift, a NaN in one column of segment 1's shift
                  and one of its scale: NaN bytes in those columns for those rows only.

Bounds.  P5's value bound is t5_fp8_cases.fp8_reference's with the kernel's own scale: half an e4m3 step (2^-4 |y| where
|y| / scale >= 2^-6, scale 2^-10 below) plus the fp32 error of y and 4 u |y| (1 / scale and the product), times 1 + 2^-6.
The error of y: 0 for the exact producers, Y_REL |y| for the RMS norm (t5_fp8_cases.y_rel_rmsnorm), the elementwise e_y
of rowop_cases.ln_reference for the LayerNorm forms.  Nothing is new here.

Measured on MI355X, tests/test_fp8_edges_gpu.py (largest printed error / bound per producer over its cases; scale, value):
ln_fp8 0.061, 0.926; ln_f32in_fp8 0.110, 0.926; quantize_rows 0.358, 0.927; t5_rmsnorm_fp8 0.010, 0.940; gated_mul_fp8
0.356, 0.965 (the value figures are e4m3 ties: half a step, under the second-order factor).  Every NaN byte the device
wrote was 0xFF, for either sign of the NaN.  No constant above was changed after a measurement.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import torch

import rowop_cases as R
import t5_fp8_cases as F8

U = F8.U
FLT_MIN = 2.0 ** -126
INF, NAN = float("inf"), float("nan")
PRODUCERS = ("ln_fp8", "ln_f32in_fp8", "quantize_rows", "t5_rmsnorm_fp8", "gated_mul_fp8")
ENTRY = {"ln_fp8": "ca_ln_modulate_fp8", "ln_f32in_fp8": "ca_ln_modulate_f32in_fp8",
         "quantize_rows": "ca_quantize_rows_fp8", "t5_rmsnorm_fp8": "ca_t5_rmsnorm_f32in_fp8",
         "gated_mul_fp8": "ca_gated_mul_fp8"}
FAMILIES = ("plain", "zero", "nan_q", "nan_s", "nan_neg", "pinf", "ninf", "tiny", "all_nan")
NAN_BITS = {"nan_q": 0x7FC0, "nan_s": 0x7F81, "nan_neg": 0xFFC0, "all_nan": 0x7FC0}      # the upper 16 bits
# special rows between plain ones inside one four-row workgroup of ca_rowops.hip
ROWS = ("plain", "nan_q", "plain", "pinf", "zero", "nan_s", "tiny", "ninf", "nan_neg", "all_nan", "plain", "tiny")
LN_ROWS = ("plain", "nan_q", "plain", "pinf", "plain", "nan_s", "ninf", "nan_neg", "zero", "all_nan", "tiny", "tiny")
LN_SEGS = [4, 8, 10, 12]
N_ROWS = 12
WIDTHS = (8, 264, 2056, 4096)      # the minimum; one ragged chunk; one pass and a single-thread pass; 8 LayerNorm chunks
PASS = {"ln_fp8": 512, "ln_f32in_fp8": 512, "quantize_rows": 512, "t5_rmsnorm_fp8": 2048, "gated_mul_fp8": 2048}
VARIANTS = {"ln_fp8": ("x", "mod"), "ln_f32in_fp8": ("x", "mod"), "quantize_rows": ("x",),
            "t5_rmsnorm_fp8": ("x", "w_nan", "w_inf"), "gated_mul_fp8": ("x",)}
SLIPS = {"launder": "P2", "no_floor": "P5", "nan_scale": "P3", "inf_to_max": "P4", "leak": "rows"}
WRAP_SPECIAL_ROWS = (2, 3)                                   # a NaN row and an inf row of the grid-wrap cases ...
WRAP_SAME_WORKGROUP = (2 + F8.ROW_GRID_CAP, 3 + F8.ROW_GRID_CAP)   # ... and the rows the same workgroups walk next


@dataclass(frozen=True)
class Case:
    producer: str
    width: int
    strided: bool
    variant: str = "x"

    @property
    def id(self):
        return f"{self.producer}-{self.width}-{'strided' if self.strided else 'contiguous'}-{self.variant}"

    @property
    def families(self):
        return LN_ROWS if self.producer.startswith("ln") else ROWS


CASES = [Case(p, w, s, v) for p in PRODUCERS for w in WIDTHS for s in (False, True) for v in VARIANTS[p]]


def special_columns(producer: str, width: int):
    return sorted({0, width - 1} | ({PASS[producer]} if width > PASS[producer] else set()))


def _gen(tag: str) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(tag.encode()))


def set_bits(t: torch.Tensor, r, c, upper16: int) -> None:
    """t[r, c] <- the float whose upper 16 bits are ``upper16`` (bf16 or fp32 t), without passing through a conversion
    that would quiet a signalling NaN."""
    if t.dtype == torch.bfloat16:
        t.view(torch.int16)[r, c] = upper16 - (1 << 16 if upper16 >= 1 << 15 else 0)
    else:
        bits = upper16 << 16
        t.view(torch.int32)[r, c] = bits - (1 << 32 if bits >= 1 << 31 else 0)


def tiny_values(shape, tag: str) -> torch.Tensor:
    """fp32 elements from {0, +-2^-125 .. +-2^-120}, a third of them zero; element 1 of every row non-zero, element 2 zero."""
    g = _gen("fp8edge.tiny." + tag)
    pick = torch.randint(0, 18, shape, generator=g)
    val = torch.pow(torch.tensor(2.0, dtype=torch.float64), (-125 + pick % 6).double()) * torch.where(pick < 12, 1.0, -1.0)
    val = torch.where(torch.rand(shape, generator=g) < 1 / 3, torch.zeros_like(val), val)
    val[..., 1], val[..., 2] = 2.0 ** -122, 0.0
    return val.to(torch.float32)


def _family_rows(x: torch.Tensor, fams, cols, tag: str) -> torch.Tensor:
    """Rows of x (bf16 or fp32, plain values in) turned into their families, special cells at ``cols``."""
    for r, f in enumerate(fams):
        if f == "zero":
            x[r] = 0
        elif f == "tiny":
            x[r] = tiny_values((x.shape[1],), f"{tag}.{r}").to(x.dtype)
        elif f in ("pinf", "ninf"):
            x[r, cols] = INF if f == "pinf" else -INF
        elif f == "all_nan":
            set_bits(x, r, slice(None), NAN_BITS[f])
        elif f in NAN_BITS:
            set_bits(x, r, cols, NAN_BITS[f])
    return x


def make_inputs(case: Case) -> dict:
    """Host tensors of one case in the kernel's own dtypes, [rows, width] contiguous (the GPU test lays them out)."""
    p, W = case.producer, case.width
    g = _gen(f"fp8edge.{p}.{W}.{case.variant}")
    cols = special_columns(p, W)
    fams = case.families
    if p == "quantize_rows":
        x = (torch.randn(N_ROWS, W, generator=g) * 3).to(torch.bfloat16)
        return dict(x=_family_rows(x, fams, cols, case.id))
    if p == "gated_mul_fp8":
        gg = (torch.randn(N_ROWS, W, generator=g) * 2).to(torch.bfloat16)
        u = (torch.randn(N_ROWS, W, generator=g) * 2).to(torch.bfloat16)
        _family_rows(gg, fams, cols, case.id)
        for r, f in enumerate(fams):
            if f == "tiny":
                u[r] = torch.tensor([1.0, -1.0, 1.5])[torch.randint(0, 3, (W,), generator=g)].to(torch.bfloat16)
            elif f in ("pinf", "ninf"):           # column 0 keeps its infinite g; the other cells overflow in the product
                u[r, cols[0]] = 1.5
                gg[r, cols[1:]] = 2.0 ** 100 * (1 if f == "pinf" else -1)
                u[r, cols[1:]] = 2.0 ** 100
            elif f == "zero":                     # 0 * u = +-0, and products below the smallest subnormal
                gg[r, cols], u[r, cols] = 2.0 ** -100, -2.0 ** -100
        return dict(g=gg, u=u)
    if p == "t5_rmsnorm_fp8":
        x = _family_rows(torch.randn(N_ROWS, W, generator=g), fams, cols, case.id)
        w = (2.0 ** -10 * (1 + 0.25 * (torch.rand(W, generator=g) * 2 - 1))).to(torch.float32)
        if case.variant == "w_nan":
            set_bits(w[None], 0, cols[-1], NAN_BITS["nan_s"])
        elif case.variant == "w_inf":
            w[cols[-1]] = -INF
        return dict(x=x, w=w)
    xdt = torch.float32 if p == "ln_f32in_fp8" else torch.bfloat16
    x = _family_rows((torch.randn(N_ROWS, W, generator=g) * 2 + 0.3).to(xdt), [f if f not in ("zero", "tiny") else "plain"
                                                                            for f in fams], cols, case.id)
    shift = [torch.randn(W, generator=g), torch.randn(W, generator=g), torch.zeros(W), tiny_values((W,), case.id + ".shift")]
    scale = [torch.randn(W, generator=g) * 0.3, torch.randn(W, generator=g) * 0.3, -torch.ones(W), -torch.ones(W)]
    if case.variant == "mod":
        shift[0][cols[0]], shift[0][cols[-1]] = INF, -INF
        set_bits(shift[1][None], 0, cols[0], NAN_BITS["nan_s"])
        set_bits(scale[1][None], 0, cols[-1], NAN_BITS["nan_neg"])
    return dict(x=x, shift=shift, scale=scale)


def replaced(case: Case, inp: dict) -> dict:
    """The inputs with every special cell replaced by what makes its y zero: a non-finite x, g, u or weight by 0, a
    LayerNorm column with a non-finite shift or scale by shift 0 and scale -1 (1 + scale = 0), and the g of a product
    that overflows fp32 by 0."""
    def fix(t, value=0.0):
        return torch.where(torch.isfinite(t), t, torch.full_like(t, value))
    if case.producer == "gated_mul_fp8":
        over = torch.isinf(inp["g"].float() * inp["u"].float())
        return dict(g=torch.where(over, torch.zeros_like(inp["g"]), fix(inp["g"])), u=fix(inp["u"]))
    if case.producer.startswith("ln"):        # (y = (1 + scale) t + shift is zero where both are replaced)
        bad = [~(torch.isfinite(a) & torch.isfinite(b)) for a, b in zip(inp["shift"], inp["scale"])]
        return dict(x=fix(inp["x"]), shift=[torch.where(m, torch.zeros_like(t), t) for m, t in zip(bad, inp["shift"])],
                    scale=[torch.where(m, -torch.ones_like(t), t) for m, t in zip(bad, inp["scale"])])
    return {k: fix(v) for k, v in inp.items()}


# ---------------------------------------------------------------------------------------------------------- emulation
def ln_y32(x, shift, scale, eps=R.EPS):
    f = torch.float32
    x = x.to(f)
    idx = R.seg_index(x.shape[0], LN_SEGS, "cpu")
    mean = x.sum(-1, keepdim=True) / x.shape[1]
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / x.shape[1] + torch.tensor(eps, dtype=f))
    return (1.0 + torch.stack(scale)[idx]) * (d * rstd) + torch.stack(shift)[idx]


def y32(case: Case, inp: dict) -> torch.Tensor:
    """The fp32 row the producer quantises, formed as the kernel forms it (summation order apart)."""
    p = case.producer
    if p == "quantize_rows":
        return inp["x"].float()
    if p == "gated_mul_fp8":
        return inp["g"].float() * inp["u"].float()
    if p == "t5_rmsnorm_fp8":
        return F8.rmsnorm_y32(inp["x"], inp["w"])
    return ln_y32(inp["x"], inp["shift"], inp["scale"])


def pack_rows(y: torch.Tensor, slip=None):
    """The shared tail of the five kernels on fp32 rows: (bytes uint8, scale fp32 [rows]).  amax with fmaxf (a NaN is
    dropped); scale = max(amax * fl(1 / 448), FLT_MIN), 1 where amax is 0; byte = e4m3(clamp(y * (1 / scale))) with a clamp
    that keeps NaN.  Slips: ``launder`` the clamp fminf(fmaxf(z, -448), 448), which turns NaN into -448; ``no_floor``;
    ``nan_scale`` a NaN reaches the maximum; ``inf_to_max`` an infinite element counts as the largest float; ``leak`` the
    maximum of a special row reaches the row behind it."""
    f = torch.float32
    y = y.to(f)
    if slip == "inf_to_max":
        y = y.clamp(-torch.finfo(f).max, torch.finfo(f).max)
    nan = torch.isnan(y)
    amax = torch.where(nan, torch.zeros_like(y), y).abs().amax(-1)
    if slip == "nan_scale":
        amax = torch.where(nan.any(-1), torch.full_like(amax, NAN), amax)
    if slip == "leak":
        raw = torch.where(nan, torch.full_like(y, INF), y).abs().amax(-1)
        special = ~torch.isfinite(raw)
        amax = amax.clone()
        amax[1:] = torch.where(special[:-1], torch.maximum(amax[1:], raw[:-1]), amax[1:])
    sc = amax * torch.tensor(1.0 / 448.0, dtype=f)
    if slip != "no_floor":
        sc = torch.where(sc < FLT_MIN, torch.full_like(sc, FLT_MIN), sc)
    scale = torch.where(amax > 0, sc, torch.ones_like(sc))
    scale = torch.where(torch.isnan(amax), amax, scale)
    z = y * (1.0 / scale)[:, None]
    c = z.clamp(-448.0, 448.0)                                  # (torch's clamp keeps NaN)
    if slip == "launder":
        c = torch.where(torch.isnan(z), torch.full_like(z, -448.0), c)
    return c.to(torch.float8_e4m3fn).view(torch.uint8), scale


def emulate(case: Case, inp: dict, slip=None):
    return pack_rows(y32(case, inp), slip)


# ---------------------------------------------------------------------------------------------------------- the contract
def is_nan_byte(q: torch.Tensor) -> torch.Tensor:
    return (q & 0x7F) == 0x7F


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def row_kinds(y: torch.Tensor):
    """(inf rows, NaN rows whose other elements are all zero, NaN rows with a replaced twin, clean rows) of fp32 rows y."""
    nan, inf = torch.isnan(y), torch.isinf(y)
    row_inf = inf.any(-1)
    row_nan = nan.any(-1) & ~row_inf
    rest_zero = row_nan & ((y == 0) | nan).all(-1)
    return row_inf, rest_zero, row_nan & ~rest_zero, ~(row_inf | row_nan)


def violations(y: torch.Tensor, got, twin) -> set:
    """The clauses that (bytes, scales) ``got`` of rows y break; ``twin``: the same launch on the replaced inputs.  CPU
    tensors; y is the emulation's fp32 row, used only for where it is NaN, infinite, zero, and its signs."""
    (q, s), (q2, s2) = got, twin
    bad = set()
    nan, inf = torch.isnan(y), torch.isinf(y)
    fin = ~(nan | inf)
    nanb = is_nan_byte(q)
    zero_byte = torch.where(torch.signbit(y), 0x80, 0).to(torch.uint8)
    row_inf, rest_zero, elementwise, clean = row_kinds(y)
    if not nanb[nan].all():
        bad.add("P2")
    r = row_inf
    if not ((s[r] == INF).all() and nanb[r][inf[r]].all() and (q[r][fin[r]] == zero_byte[r][fin[r]]).all()):
        bad.add("P4")
    r = rest_zero
    if not ((_bits(s[r]) == _bits(torch.ones_like(s[r]))).all() and (q[r][fin[r]] == zero_byte[r][fin[r]]).all()):
        bad.add("P3")
    r = elementwise
    if not ((_bits(s[r]) == _bits(s2[r])).all() and (q[r] == q2[r])[fin[r]].all()):
        bad.add("P3")
    r = clean
    if not ((_bits(s[r]) == _bits(s2[r])).all() and (q[r] == q2[r]).all()):
        bad.add("rows")
    r = clean & (y != 0).any(-1)
    if not ((torch.isfinite(s[r]) & (s[r] >= FLT_MIN)).all() and not nanb[r].any()):
        bad.add("P5")
    return bad


def y64_and_error(case: Case, inp: dict):
    """(fp64 y, the bound of the kernel's fp32 y against it, elementwise); meaningful on finite rows only."""
    p = case.producer
    if p == "quantize_rows":
        y = inp["x"].double()
        return y, torch.zeros_like(y)
    if p == "gated_mul_fp8":
        y = inp["g"].double() * inp["u"].double()
        return y, torch.zeros_like(y)
    if p == "t5_rmsnorm_fp8":
        y = F8.rmsnorm_y64(inp["x"], inp["w"])
        return y, F8.y_rel_rmsnorm(case.width) * y.abs()
    ln = R.Case(case.id, ENTRY[p], "", "ln", dict(M=N_ROWS, H=case.width, segs=LN_SEGS, out="bf16"))
    y, e_y, _ = R.ln_reference(ln, inp)["out"]
    return y, e_y


def p5_ratios(case: Case, inp: dict, q: torch.Tensor, s: torch.Tensor):
    """(scale error / bound, value error / bound) maxima over the finite non-zero rows of the case, with the kernel's own
    scale; inf where a scale is not finite, positive and normal, a byte not finite, or a scale under the floor rule is
    outside [amax / 448, 2^-126]."""
    y, e_y = y64_and_error(case, inp)
    yf = y32(case, inp)
    rows = torch.isfinite(yf).all(-1) & (yf != 0).any(-1)
    if not rows.any():                      # (a NaN or inf column of the weight: no finite row in the case)
        return 0.0, 0.0
    y, e_y, q, s = y[rows], e_y[rows], q[rows], s[rows].double()
    if not ((torch.isfinite(s) & (s >= FLT_MIN)).all() and not is_nan_byte(q).any()):
        return math.inf, math.inf
    a = y.abs()
    amax, arg = a.max(-1)
    ref = amax / 448.0
    e_s = (e_y.gather(1, arg[:, None])[:, 0] / 448.0 + 4 * U * ref) * F8.SECOND_ORDER
    above = ref >= FLT_MIN * (1 + 2.0 ** -10)
    floored = (s <= FLT_MIN) & (s >= ref * (1 - 2.0 ** -10))
    rs = torch.where(above, (s - ref).abs() / e_s, torch.where(floored, 0.0, math.inf))
    normal = a / s[:, None] >= F8.E4M3_MIN_NORMAL
    half = torch.where(normal, F8.HALF_STEP_REL * a, s[:, None] * F8.HALF_STEP_SUB)
    bound = (half + e_y + 4 * U * a) * F8.SECOND_ORDER
    err = (q.view(torch.float8_e4m3fn).double() * s[:, None] - y).abs()
    rv = err / bound.clamp_min(torch.finfo(torch.float64).tiny)
    return float(rs.max()), float(rv.max())


# ---------------------------------------------------------------------------------------------------------- grid wrap
def wrap_inputs(producer: str):
    """The WRAP_CASES inputs of t5_fp8_cases (65541 x 264) and the same with a NaN at (2, 5) and an inf at (3, 7) of x / g."""
    c = F8.WRAP_CASES[producer][3]
    if producer == "t5_rmsnorm_fp8":
        a, b, _ = F8.rms_inputs(c["H"], c["rows"])
    else:
        a, b, _ = F8.gate_inputs(c["C"], c["rows"])
        a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    special = a.clone()
    special[WRAP_SPECIAL_ROWS[0], 5], special[WRAP_SPECIAL_ROWS[1], 7] = NAN, INF
    return a, special, b
