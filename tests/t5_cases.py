"""Launch cases of the T5 kernels (ca_t5.hip), their inputs, a faithful emulation of each kernel's numerics with the
named slips, and derived error bounds against the fp64 statements of tests/t5_ref.py.

Imported by tests/test_t5_kernels_gpu.py (the GPU cases) and tests/test_t5_cases_cpu.py (the emulation sits inside every
bound, every slip leaves it).  Nothing here touches torch.cuda; everything runs on the CPU in fp64 / fp32.

Bounds (elementwise, first order; u = 2^-24, every fp32 operation charged 2 u of its running magnitude and the
transcendentals EXP_ULPS / GELU_ULPS, as in gemm_route_cases.py, rowop_cases.py and attn_cases.py; a bf16 rounding is
BF16_U = 2^-8 relative; second-order terms -- products of relative errors <= 2^-7 -- are covered by 1 + 2^-6):

ca_t5_attn_bf16.  q, k, v and the bias are the kernel's inputs, exact on both sides.
  score          64 products in 2 MFMA updates of 32, then + bias: delta_i = 2 u (SCORE_C max_j sum_d |q_id| |k_jd| +
                 max_j |s_ij|), SCORE_C = 64 / 32 + log2 32 + 2.
  exp            the exponent (s - m) log2 e: a subtraction, a product and the fp32 constant, 5 u R_i in nats with
                 R_i = max_j s_ij - min_j s_ij; the errors of s_ij and of m: 2 delta_i; v_exp_f32: EXP_ULPS u.
                 eps_i = 2 delta_i + 5 u R_i + EXP_ULPS u, relative, on every p.
  P              rounded to bf16 on the P v side only (BF16_U); the sum runs over the fp32 values.
  O^T            one MFMA update per 32 keys: 2 u (L / 32 + log2 32 + 2) sum_j P_ij |v_jd|.
  sum            L / 4 additions per lane, two exchanges: 2 u (L / 4 + 2), relative on the output.
  finish         1 / sum, the product: 2 u FIN_ULPS |o|; the bf16 store: BF16_U |o|.
  out error      (BF16_U + eps_i + O^T) A_id + (BF16_U + eps_i + sum + finish) |o_id|,  A = sum_j P_ij |v_jd|.
ca_t5_rmsnorm_f32in.  sum of H squares (H / 1024 per thread, a 64-lane and a 4-wave reduction; charged as H / 256 + 8
  sequential additions), / H, + eps, sqrt, 1 / x (NORM_ULPS), two products, the bf16 store:
  |o| (BF16_U + u (H / 256 + 8) + 2 u (NORM_ULPS + 2)).
ca_gated_mul_bf16.  The product of two bf16 values is exact in fp32; the store: BF16_U |o| (+ the smallest bf16
  subnormal, 2^-133).
the gate path (GEMM epilogue + ca_gated_mul_bf16 on fp32 pre-activations a0, a1): g = bf16(gelu(a0)) with ca_gelu_tanh
  (GELU_ULPS u relative, plus 8 u ln 2 |a0 (K0 + K1 a0^2)| on the sigmoid: the three fp32 operations and the two
  rounded constants that form the exponent), u' = bf16(a1), the product's
  store: |o| (3 BF16_U + gelu terms).
ca_embed_rows_f32.  A bf16 value widened to fp32: exact.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import torch

import gemm_route_cases as G
import rowop_cases as R
import t5_ref

U = G.U
BF16_U = 2.0 ** -8
EXP_ULPS = R.EXP_ULPS
GELU_ULPS = G.GELU_ULPS
NORM_ULPS = G.NORM_ULPS
SCORE_C = 64 / 32 + math.log2(32) + 2
FIN_ULPS = 3
SECOND_ORDER = 1 + 2.0 ** -6
EPS = 1e-6

# Measured on MI355X, tests/test_t5_kernels_gpu.py (largest printed max err / bound per kernel): attention 0.750 (std8),
# 0.696 (far), 0.562 (std1); rmsnorm 0.980 and gated_mul 0.988 (both the bf16 store's half ulp next to a power of two);
# embed exact.  No constant above was changed after a measurement.
# With the later cases (same file, largest per kernel): attention 0.811 (2x3x192 std8), 0.804 (L = 320), 0.793 (L = 448);
# rmsnorm 0.980 (65541 x 264, the grid wrap), 0.975 (H = 1032), 0.808 (H = 4); gated_mul 0.988 (13108 x 10240, the grid
# wrap, and C = 2056); embed exact, the 32769 x 4096 wrap included.  The same cases at bit 31, across a 2^32 line and with
# far rows (tests/test_address_range_gpu.py) give the bits of the plain run.


def _gen(tag: str) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(zlib.crc32(tag.encode()))
    return g


def bf16r(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (RNE) and widen again, in t's dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


# ---------------------------------------------------------------------------------------------------------- attention
@dataclass(frozen=True)
class AttnCase:
    n_seq: int
    heads: int
    L: int
    layout: str      # contig | sliced: q, k, v as column slices of one [rows, 3 heads 64] buffer, out in a wider one
    family: str      # std1 | std8: logit standard deviation in nats; far: one far key dominates rows 0 and L - 1

    @property
    def name(self):
        return f"{self.n_seq}x{self.heads}x{self.L}-{self.layout}-{self.family}"


ATTN_SHAPES = [(1, 1, 64),      # one tile
               (1, 2, 128),
               (2, 3, 192),     # odd head count, L no power of two
               (1, 64, 64),     # the real head count
               (5, 4, 256),
               (1, 2, 320),     # NT = 20, 24, 28: with 64 .. 256 and 512 every instantiation of ca_t5_attn_kernel<NT>, each
               (2, 1, 384),     # with its own LDS carve (rows of L + 16), score-register count and unroll
               (1, 3, 448),
               (1, 2, 512)]     # the maximum: offsets beyond the 128 clamp on both sides
ATTN_CASES = [AttnCase(n, h, L, layout, fam) for (n, h, L) in ATTN_SHAPES for layout in ("contig", "sliced")
              for fam in ("std1", "std8", "far")]
FAR_LOGIT = 60.0


def attn_inputs(c: AttnCase):
    """(q, k, v [n_seq L, heads 64] fp32 holding bf16 values, bias fp32 [heads, 2 L - 1])."""
    rows, width = c.n_seq * c.L, c.heads * 64
    g = _gen(f"t5attn.{c.n_seq}.{c.heads}.{c.L}.{c.family}")
    std = 8.0 if c.family == "std8" else 1.0
    a = math.sqrt(std / 8.0)                      # q . k over 64 dimensions: std 8 a^2
    q = bf16r(torch.randn(rows, width, generator=g) * a)
    k = bf16r(torch.randn(rows, width, generator=g) * a)
    v = bf16r(torch.randn(rows, width, generator=g))
    if c.family == "far":
        for s in range(c.n_seq):
            for h in range(c.heads):
                cols = slice(h * 64, h * 64 + 64)
                for qr, kr in ((0, c.L - 1), (c.L - 1, 0)):      # the farthest key on either side
                    qv = q[s * c.L + qr, cols]
                    k[s * c.L + kr, cols] = bf16r(qv * (FAR_LOGIT / float(qv @ qv)))
    weight = bf16r((torch.rand(32, c.heads, generator=g) * 2 - 1) * 4)
    bias = t5_ref.bias_table(weight, c.L).to(torch.float32)
    return q, k, v, bias, weight


def _heads(t, n_seq, L, heads):
    return t.reshape(n_seq, L, heads, 64).permute(0, 2, 1, 3)


def _rel(L):
    idx = torch.arange(L)
    return idx[None, :] - idx[:, None] + L - 1          # [query, key]


def attn_reference(q, k, v, bias, n_seq, heads):
    """fp64 (out, bound), both [rows, heads 64]."""
    rows = q.shape[0]
    L = rows // n_seq
    qh, kh, vh = (_heads(t.double(), n_seq, L, heads) for t in (q, k, v))
    b = bias.double()[:, _rel(L)][None]
    s = qh @ kh.transpose(-1, -2) + b
    p = torch.softmax(s, -1)
    out, A = p @ vh, p @ vh.abs()
    mag = (qh.abs() @ kh.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    delta = 2 * U * (SCORE_C * mag + s.abs().amax(-1, keepdim=True))
    spread = s.amax(-1, keepdim=True) - s.amin(-1, keepdim=True)
    eps = 2 * delta + 5 * U * spread + EXP_ULPS * U
    chain = 2 * U * (L / 32 + math.log2(32) + 2)
    total = 2 * U * (L / 4 + 2)
    bound = ((BF16_U + eps + chain) * A + (BF16_U + eps + total + 2 * U * FIN_ULPS) * out.abs()) * SECOND_ORDER

    def merge(t):
        return t.permute(0, 2, 1, 3).reshape(rows, heads * 64)
    return merge(out), merge(bound)


ATTN_SLIPS = ("bucket_off_by_one", "bias_transposed", "scaled", "padding_masked", "head_stride_128")


def attn_emulated(q, k, v, bias, n_seq, heads, slip=None, weight=None, n_real=None):
    """The kernel's arithmetic in fp32 / bf16: fp32 scores + bias, exact two-pass softmax, P rounded to bf16
    (unnormalised) for P v only, the fp32 sum, the bf16 store.  ``slip``: one of ATTN_SLIPS (``weight``: the
    [32, heads] bucket weights for bucket_off_by_one; ``n_real``: keys >= n_real count as padding for padding_masked;
    head_stride_128: head h reads the q and k columns of head 2 h, wrapped into the row; needs heads >= 2)."""
    rows = q.shape[0]
    L = rows // n_seq
    f = torch.float32
    nh = heads
    qh, kh, vh = (_heads(t.to(f), n_seq, L, heads) for t in (q, k, v))
    if slip == "head_stride_128":
        src = [(2 * h) % heads for h in range(heads)]
        qh, kh = qh[:, src], kh[:, src]
    b = bias.to(f)
    if slip == "bucket_off_by_one":
        off = torch.arange(-(L - 1), L)
        bk = torch.tensor([min(31, t5_ref.bucket_exact(int(o)) + 1) for o in off])
        b = weight.to(f)[bk].t().contiguous()
    rel = _rel(L).t() if slip == "bias_transposed" else _rel(L)
    s = qh @ kh.transpose(-1, -2)
    if slip == "scaled":
        s = s * torch.tensor(0.125, dtype=f)     # 1 / sqrt(64)
    s = s + b[:nh][:, rel][None]
    if slip == "padding_masked":
        s[..., n_real:] = -torch.inf
    m = s.amax(-1, keepdim=True)
    p = torch.exp2((s - m) * torch.tensor(1.4426950409, dtype=f))
    o = (bf16r(p) @ vh) * (1.0 / p.sum(-1, keepdim=True))
    return bf16r(o).permute(0, 2, 1, 3).reshape(rows, nh * 64)


# ---------------------------------------------------------------------------------------------------------- row kernels
ROW_H = (256, 4096)
ROW_ROWS = (1, 7, 1280)
EMBED_CASES = [(H, rows, strided) for H in ROW_H for rows in ROW_ROWS for strided in (False, True)]
# the column loops step 1024 elements per pass (2048 in the e4m3 producers, t5_fp8_cases.py): 1032 and 2056 are one whole
# pass and a second one that two (one) of the 256 threads enter; 4 and 8 are the entry points' minimum widths
WIDTH_ROWS = (1, 7)
ROW_CASES = EMBED_CASES + [(H, rows, strided) for H in (1032, 4) for rows in WIDTH_ROWS for strided in (False, True)]
EMBED_CASES = EMBED_CASES + [(8, rows, strided) for rows in WIDTH_ROWS for strided in (False, True)]
GATE_CASES = [(C, rows, strided) for C in (512, 10240) for rows in ROW_ROWS for strided in (False, True)] + \
             [(C, rows, strided) for C in (2056, 8) for rows in WIDTH_ROWS for strided in (False, True)]
# ---- grid wrap: the capped grids of ca_t5.hip, restated.  A case that exceeds its cap sends workgroups through a second
# iteration of the kernel's stride loop (in the row kernels with the 4-float `red` array reused across iterations).
ROW_GRID_CAP = 65536                 # workgroups, one row each: `rows < 65536 ? rows : 65536` (tx_row_blocks)
ELEM_GRID_CAP = 65536 * 256          # threads, 8 elements each: `if (blocks > 65536) blocks = 65536` (tx_walk8_blocks)
WRAP_ROWS, WRAP_H = ROW_GRID_CAP + 5, 264
# op -> (units of work: rows or threads, the cap in the same units, units per workgroup, the case itself)
WRAP_CASES = {
    "t5_rmsnorm": (WRAP_ROWS, ROW_GRID_CAP, 1, dict(H=WRAP_H, rows=WRAP_ROWS)),
    "gated_mul": (13108 * (10240 // 8), ELEM_GRID_CAP, 256, dict(C=10240, rows=13108)),
    "embed_rows": (32769 * (4096 // 8), ELEM_GRID_CAP, 256, dict(H=4096, rows=32769)),
}
ROW_MAGNITUDES = (1.0, 1e-2, 1e4, 3.0)    # row r is scaled by ROW_MAGNITUDES[r % 4]: 1e-2 makes eps matter, 1e4 is large


def row_inputs(H, rows, tag="rms"):
    """(x fp32 [rows, H] with a mean of about half its spread, w fp32 [H] around 1)."""
    g = _gen(f"t5row.{tag}.{H}.{rows}")
    x = torch.randn(rows, H, generator=g) + 0.5
    x = x * torch.tensor([ROW_MAGNITUDES[r % 4] for r in range(rows)])[:, None]
    w = 1 + 0.25 * (torch.rand(H, generator=g) * 2 - 1)
    return x.to(torch.float32), w.to(torch.float32)


def rmsnorm_reference(x, w, eps=EPS):
    out = t5_ref.rmsnorm(x.double(), w.double(), eps)
    H = x.shape[1]
    return out, out.abs() * (BF16_U + U * (H / 256 + 8) + 2 * U * (NORM_ULPS + 2)) * SECOND_ORDER + 2.0 ** -133


RMS_SLIPS = ("mean_subtracted", "eps_1e-5")


def rmsnorm_emulated(x, w, eps=EPS, slip=None):
    f = torch.float32
    x = x.to(f)
    if slip == "mean_subtracted":
        x = x - x.mean(-1, keepdim=True)
    if slip == "eps_1e-5":
        eps = 1e-5
    rs = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / x.shape[1] + torch.tensor(eps, dtype=f))
    return bf16r(x * rs * w.to(f))


def gate_inputs(C, rows):
    """(g, u): bf16 values as fp32 [rows, C]."""
    gen = _gen(f"t5gate.{C}.{rows}")
    return bf16r(torch.randn(rows, C, generator=gen) * 2), bf16r(torch.randn(rows, C, generator=gen) * 2)


def gated_mul_reference(g, u):
    out = g.double() * u.double()
    return out, out.abs() * BF16_U + 2.0 ** -133


def gated_mul_emulated(g, u):
    return bf16r(g.to(torch.float32) * u.to(torch.float32))


def gate_path_reference(a0, a1):
    """gelu_tanh(a0) * a1 in fp64 from the fp32 pre-activations, and the bound of the epilogue + product path."""
    a0, a1 = a0.double(), a1.double()
    out = t5_ref.gelu_tanh(a0) * a1
    arg = (a0 * (G.K0 + G.K1 * a0 * a0)).abs()
    rel = 3 * BF16_U + GELU_ULPS * U + 8 * U * math.log(2.0) * arg
    return out, out.abs() * rel * SECOND_ORDER + 2.0 ** -133


GATE_SLIPS = ("erf_gelu",)


def gate_path_emulated(a0, a1, slip=None):
    f = torch.float32
    a0, a1 = a0.to(f), a1.to(f)
    if slip == "erf_gelu":
        gl = torch.nn.functional.gelu(a0)
    else:   # ca_gelu_tanh: x / (1 + exp2(x (K0 + K1 x^2)))
        gl = a0 / (1.0 + torch.exp2(a0 * (torch.tensor(G.K0, dtype=f) + torch.tensor(G.K1, dtype=f) * a0 * a0)))
    return bf16r(bf16r(gl) * bf16r(a1))


def embed_inputs(H, rows, vocab=512):
    """(table bf16 values as fp32 [vocab, H], ids int32 [rows] with 0 and vocab - 1 among them)."""
    gen = _gen(f"t5embed.{H}.{rows}")
    table = bf16r(torch.randn(vocab, H, generator=gen))
    ids = torch.randint(0, vocab, (rows,), generator=gen, dtype=torch.int32)
    ids[0] = vocab - 1
    ids[-1] = 0
    if rows > 2:
        ids[1] = 0
    return table, ids
