"""Launch cases of the CLIP text encoder's kernels (ca_clip.hip), their inputs, a faithful emulation of each kernel's
numerics with the named slips, and derived error bounds against the fp64 statements of tests/clip_ref.py.

Imported by tests/test_clip_kernels_gpu.py (the GPU cases) and tests/test_clip_cases_cpu.py (the emulation sits inside
every bound, every slip leaves it).  Nothing here touches torch.cuda; everything runs on the CPU in fp64 / fp32.

Bounds (elementwise, first order; u = 2^-24, every fp32 operation charged 2 u of its running magnitude and the
transcendentals EXP_ULPS / NORM_ULPS, as in t5_cases.py and the tables it follows; a bf16 rounding is BF16_U = 2^-8
relative; second-order terms are covered by 1 + 2^-6):

ca_clip_attn_bf16.  q, k, v are the kernel's inputs, exact on both sides.  "Keys" are the keys j <= i a query i sees.
  score          64 products in 2 MFMA updates of 32, then the product with the scale:
                 delta_i = 2 u (SCORE_C scale max_j sum_d |q_id| |k_jd| + max_j |s_ij|), SCORE_C = 64 / 32 + log2 32 + 2.
  exp            the exponent (s - m) log2 e: 5 u R_i in nats with R_i = max_j s_ij - min_j s_ij; the errors of s_ij and
                 of m: 2 delta_i; v_exp_f32: EXP_ULPS u.  eps_i = 2 delta_i + 5 u R_i + EXP_ULPS u, relative, on every
                 p.  A masked score is -inf exactly and its p is 0 exactly.
  P              rounded to bf16 on the P v side only (BF16_U); the sum runs over the fp32 values.
  O^T            one MFMA update per 32 keys of the padded length LP = 32 ceil(L / 32): 2 u (LP / 32 + log2 32 + 2)
                 sum_j P_ij |v_jd|.
  sum            LP / 4 additions per lane (the masked ones add 0), two exchanges: 2 u (LP / 4 + 2), relative.
  finish         1 / sum, the product: 2 u FIN_ULPS |o|; the bf16 store: BF16_U |o|.
  out error      (BF16_U + eps_i + O^T) A_id + (BF16_U + eps_i + sum + finish) |o_id|,  A = sum_j P_ij |v_jd|.
ca_layernorm_f32in.  With d = x - mean, sigma^2 = var + eps, a = mean_i |x_i|:
  mean           H additions (H / 1024 per thread, a 64-lane and a 4-wave reduction; charged as H / 256 + 8 sequential
                 ones) and the division: dm = u (H / 256 + 9) a, absolute.
  d              one subtraction: u |d_i| + dm.
  var            sum (d_i - dm)^2 = sum d_i^2 + H dm^2 (the first-order term vanishes: sum d_i = 0), so the error of the
                 mean enters as (dm / sigma)^2 only; the squares and the sum: u (H / 256 + 11); + eps, sqrt, 1 / x:
                 2 u (NORM_ULPS + 2).  r = half of the variance's relative error plus the last term.
  out            (d rs) w + b: |d rs w| (r + 4 u) + dm rs |w|, the addition u |o|, the bf16 store BF16_U |o|.
  A row whose mean is 100 times its spread has dm = 1e-5 sigma: visible against nothing.  The one-pass form
  sum x^2 / H - mean^2 would lose 1e4 u = 6e-4 of the variance there; it is not what the kernel does.
ca_quick_gelu_bf16.  x / (1 + exp2(-K x)), K = 1.702 log2 e: the rounded constant and the product put 2 u |K x| into
  the exponent, 2 u ln 2 |K x| relative on exp2 (times e / (1 + e) <= 1); v_exp_f32 EXP_ULPS u; 1 + e, v_rcp_f32 and
  the product: 5 u; the bf16 store: BF16_U.  Plus the smallest bf16 subnormal, 2^-133.  |x| <= 40 keeps every
  intermediate inside fp32's normal range (exp2(98)).
ca_clip_embed_f32.  Two bf16 values widened and added once: u |o|.
the model.  Relative rms of the bf16 output against fp64: MODEL_REL_RMS = 1e-2.  A bf16 rounding has a relative rms of
  2^-9 / sqrt 3 = 1.1e-3; per layer about 16 of them meet a value's path (hn, q, k, v, P, the attention output, hn
  again, fc1's output, quick_gelu's, and the six weights and their biases), two layers and the final store make 33
  independent ones: sqrt(33) 1.1e-3 = 6.5e-3 if nothing amplifies; the LayerNorms keep the stream at unit scale.
  transformers' own bf16 run of the same network is at 5.4e-3 (tests/golden/clip_*.npz), inside it as well.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import torch

import clip_ref
import gemm_route_cases as G
import rowop_cases as R

U = G.U
BF16_U = 2.0 ** -8
EXP_ULPS = R.EXP_ULPS
NORM_ULPS = G.NORM_ULPS
SCORE_C = 64 / 32 + math.log2(32) + 2
FIN_ULPS = 3
SECOND_ORDER = 1 + 2.0 ** -6
EPS = 1e-5
SCALE = 0.125
QG_K = 1.702 * 1.4426950408889634
MODEL_REL_RMS = 1e-2

# Measured on MI355X, tests/test_clip_kernels_gpu.py (largest printed max err / bound per kernel): attention 0.713
# (L = 15), 0.702 (L = 64), 0.689 (L = 77); layernorm 0.965 and quick_gelu 0.981 (both the bf16 store's half ulp next to a
# power of two); embed exact.  No constant above was changed after a measurement.
# With the later cases: layernorm 0.980 (65541 x 264, the grid wrap, row by row and gathered), 0.975 (H = 1032); quick_gelu
# 0.981 (43692 x 3072, the grid wrap, and C = 2056); embed exact, H = 8 and the 174790 x 768 wrap included; attention
# unchanged at 0.713.


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
    layout: str      # sliced: q, k, v column slices of one qkv buffer, out in a wider one; apart: four buffers, four strides

    @property
    def name(self):
        return f"{self.n_seq}x{self.heads}x{self.L}-{self.layout}"


ATTN_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 77, 128)   # one key; around the 16-key tile; around the 64-query workgroup; CLIP; the maximum
ATTN_CASES = [AttnCase(3, 2, L, "sliced") for L in ATTN_LENGTHS] + [AttnCase(3, 2, 77, "apart")]


def attn_inputs(c: AttnCase):
    """(q, k, v [n_seq L, heads 64] fp32 holding bf16 values): scale q . k has a standard deviation of 2 nats; v is drawn
    per row, so every sequence has its own."""
    rows, width = c.n_seq * c.L, c.heads * 64
    g = _gen(f"clipattn.{c.n_seq}.{c.heads}.{c.L}")
    a = math.sqrt(2.0)                            # q . k over 64 dimensions: std 8 a^2, times 1 / 8
    q = bf16r(torch.randn(rows, width, generator=g) * a)
    k = bf16r(torch.randn(rows, width, generator=g) * a)
    v = bf16r(torch.randn(rows, width, generator=g) + torch.arange(rows)[:, None] % 3 - 1.0)
    return q, k, v


def _heads(t, n_seq, L, heads):
    return t.reshape(n_seq, L, heads, 64).permute(0, 2, 1, 3)


def _visible(L, shift=0):
    idx = torch.arange(L)
    return idx[None, :] <= idx[:, None] + shift          # [query, key]


def attn_reference(q, k, v, n_seq, heads, scale=SCALE):
    """fp64 (out, bound), both [rows, heads 64]."""
    rows = q.shape[0]
    L = rows // n_seq
    LP = 32 * ((L + 31) // 32)
    qh, kh, vh = (_heads(t.double(), n_seq, L, heads) for t in (q, k, v))
    vis = _visible(L)
    s = qh @ kh.transpose(-1, -2) * scale
    p = torch.softmax(s.masked_fill(~vis, -torch.inf), -1)
    out, A = p @ vh, p @ vh.abs()
    mag = (qh.abs() @ kh.abs().transpose(-1, -2) * scale).masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    smax = s.abs().masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    delta = 2 * U * (SCORE_C * mag + smax)
    spread = s.masked_fill(~vis, -torch.inf).amax(-1, keepdim=True) - s.masked_fill(~vis, torch.inf).amin(-1, keepdim=True)
    eps = 2 * delta + 5 * U * spread + EXP_ULPS * U
    chain = 2 * U * (LP / 32 + math.log2(32) + 2)
    total = 2 * U * (LP / 4 + 2)
    bound = ((BF16_U + eps + chain) * A + (BF16_U + eps + total + 2 * U * FIN_ULPS) * out.abs()) * SECOND_ORDER

    def merge(t):
        return t.permute(0, 2, 1, 3).reshape(rows, heads * 64)
    return merge(out), merge(bound)


ATTN_SLIPS = ("mask_plus_one", "no_mask", "no_scale", "padded_keys_counted")


def attn_emulated(q, k, v, n_seq, heads, scale=SCALE, slip=None):
    """The kernel's arithmetic in fp32 / bf16: fp32 scores times the scale, -inf above the diagonal, exact two-pass
    softmax, P rounded to bf16 (unnormalised) for P v only, the fp32 sum, the bf16 store.  ``slip``: one of ATTN_SLIPS --
    mask_plus_one: key <= query + 1; no_mask; no_scale; padded_keys_counted: the rows that follow the sequence up to the
    32-key step (the next sequence's, zeros after the last) are keys and values every query sees."""
    rows = q.shape[0]
    L = rows // n_seq
    f = torch.float32
    qh, kh, vh = (_heads(t.to(f), n_seq, L, heads) for t in (q, k, v))
    vis = _visible(L, 1 if slip == "mask_plus_one" else 0)
    if slip == "no_mask":
        vis = torch.ones(L, L, dtype=torch.bool)
    if slip == "padded_keys_counted":
        pad = 32 * ((L + 31) // 32) - L

        def tail(t):        # [n_seq, heads, pad, 64]: the rows behind each sequence in the buffer, zeros behind the last
            ext = torch.cat([t.to(f), torch.zeros(pad, t.shape[1], dtype=f)])
            idx = (torch.arange(n_seq)[:, None] + 1) * L + torch.arange(pad)[None, :]
            return ext[idx].reshape(n_seq, pad, heads, 64).permute(0, 2, 1, 3)
        kh, vh = torch.cat([kh, tail(k)], 2), torch.cat([vh, tail(v)], 2)
        vis = torch.cat([vis, torch.ones(L, pad, dtype=torch.bool)], 1)
    s = qh @ kh.transpose(-1, -2)
    if slip != "no_scale":
        s = s * torch.tensor(scale, dtype=f)
    s = s.masked_fill(~vis, -torch.inf)
    m = s.amax(-1, keepdim=True)
    p = torch.exp2((s - m) * torch.tensor(1.4426950409, dtype=f))
    o = (bf16r(p) @ vh) * (1.0 / p.sum(-1, keepdim=True))
    return bf16r(o).permute(0, 2, 1, 3).reshape(rows, heads * 64)


# ---------------------------------------------------------------------------------------------------------- LayerNorm
LN_H = (64, 256, 768)
LN_ROWS = 9
# (H, rows, strided).  The column loop steps 1024 elements per pass: 1032 is one whole pass and a second one that two of
# the 256 threads enter; 4 is the entry point's minimum width (one thread works, 255 bring 0 to the reductions)
WIDTH_ROWS = (1, 7)
LN_CASES = [(H, LN_ROWS, strided) for H in LN_H for strided in (False, True)] + \
           [(H, rows, strided) for H in (1032, 4) for rows in WIDTH_ROWS for strided in (False, True)]
LN_GATHER = (5, 0, 8, 5, 2, 2)     # out of order and repeated


def ln_id(case) -> str:
    H, rows, strided = case
    return f"{H}-{strided}" if rows == LN_ROWS else f"{H}-{rows}-{strided}"


def ln_gather(rows: int) -> tuple:
    """Rows of x to read, out of order and repeated, the last row among them."""
    return tuple(min(i, rows - 1) for i in LN_GATHER)


# ---- grid wrap: the capped grids of ca_clip.hip, restated
ROW_GRID_CAP = 65536                 # workgroups, one row each: `rows < 65536 ? rows : 65536` (tx_row_blocks)
ELEM_GRID_CAP = 65536 * 256          # threads, 8 elements each: `if (blocks > 65536) blocks = 65536` (tx_walk8_blocks)
WRAP_ROWS, WRAP_H = ROW_GRID_CAP + 5, 264
# op -> (units of work: rows or threads, the cap in the same units, units per workgroup, the case itself)
WRAP_CASES = {
    "layernorm": (WRAP_ROWS, ROW_GRID_CAP, 1, dict(H=WRAP_H, rows=WRAP_ROWS)),
    "quick_gelu": (43692 * (3072 // 8), ELEM_GRID_CAP, 256, dict(C=3072, rows=43692)),
    "clip_embed": (77 * 2270 * (768 // 8), ELEM_GRID_CAP, 256, dict(H=768, rows=77 * 2270)),   # rows a multiple of 77
}


def ln_inputs(H, rows=LN_ROWS):
    """(x fp32 [rows, H], w, b fp32 [H]).  Row r has the spread (1, 1e-2, 30)[r % 3]; the odd rows have a mean of 100
    times their spread, where sum x^2 / H - mean^2 cancels."""
    g = _gen(f"clipln.{H}.{rows}")
    x = torch.randn(rows, H, generator=g)
    std = torch.tensor([(1.0, 1e-2, 30.0)[r % 3] for r in range(rows)])[:, None]
    mean = torch.tensor([100.0 if r % 2 else 0.3 for r in range(rows)])[:, None]
    x = (x + mean) * std
    w = 1 + 0.25 * (torch.rand(H, generator=g) * 2 - 1)
    b = 0.5 * (torch.rand(H, generator=g) * 2 - 1)
    return x.to(torch.float32), w.to(torch.float32), b.to(torch.float32)


def layernorm_reference(x, w, b, eps=EPS):
    """fp64 (out, bound)."""
    x, w, b = x.double(), w.double(), b.double()
    H = x.shape[1]
    out = clip_ref.layernorm(x, w, b, eps)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    sigma = torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    dm = U * (H / 256 + 9) * x.abs().mean(-1, keepdim=True)
    r = 0.5 * (U * (H / 256 + 11) + (dm / sigma) ** 2) + 2 * U * (NORM_ULPS + 2)
    core = (d / sigma * w).abs()
    bound = core * (r + 4 * U) + dm / sigma * w.abs() + out.abs() * (U + BF16_U)
    return out, bound * SECOND_ORDER + 2.0 ** -133


LN_SLIPS = ("no_mean", "no_bias")


def layernorm_emulated(x, w, b, eps=EPS, slip=None):
    """fp32: the mean, the sum of squares about it, 1 / sqrt, the product and the addition, the bf16 store.  no_mean: the
    T5 form (no mean subtraction anywhere); no_bias: b dropped."""
    f = torch.float32
    x, w, b = x.to(f), w.to(f), b.to(f)
    H = x.shape[1]
    mean = torch.zeros(x.shape[0], 1, dtype=f) if slip == "no_mean" else x.sum(-1, keepdim=True) / H
    d = x - mean
    rs = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / H + torch.tensor(eps, dtype=f))
    o = d * rs * w
    return bf16r(o if slip == "no_bias" else o + b)


# ---------------------------------------------------------------------------------------------------------- quick_gelu
QG_CASES = [(C, rows, strided) for (C, rows) in ((512, 7), (3072, 3)) for strided in (False, True)]
# 8 elements per thread: 2056 is 257 threads' worth per row (no multiple of the wave), 8 the entry point's minimum width
QG_CASES += [(C, rows, strided) for C in (2056, 8) for rows in WIDTH_ROWS for strided in (False, True)]


def quick_gelu_inputs(C, rows):
    """bf16 values as fp32 [rows, C] spanning +-40 (row 0 a ramp over the whole span, the others N(0, 2): the curved part)."""
    g = _gen(f"clipqg.{C}.{rows}")
    x = torch.randn(rows, C, generator=g) * 2
    x[0] = torch.linspace(-40, 40, C)
    x[-1, :4] = torch.tensor([-40.0, 40.0, 0.0, -0.0])
    return bf16r(x)


def quick_gelu_reference(x):
    x = x.double()
    out = clip_ref.quick_gelu(x)
    rel = BF16_U + U * (EXP_ULPS + 5) + 2 * U * math.log(2.0) * QG_K * x.abs()
    return out, out.abs() * rel * SECOND_ORDER + 2.0 ** -133


QG_SLIPS = ("gelu_tanh",)


def quick_gelu_emulated(x, slip=None):
    f = torch.float32
    x = x.to(f)
    if slip == "gelu_tanh":
        return bf16r(clip_ref.gelu_tanh(x))
    return bf16r(x * (1.0 / (1.0 + torch.exp2(torch.tensor(-QG_K, dtype=f) * x))))


# ---------------------------------------------------------------------------------------------------------- embedding
EMBED_L, EMBED_SEQ = 77, 3
EMBED_H = (64, 256, 8)             # 8: the entry point's minimum width


def embed_inputs(H, vocab=512, L=EMBED_L, n_seq=EMBED_SEQ):
    """(tok [vocab, H], pos [L, H] bf16 values as fp32, ids int32 [n_seq L] with 0 and vocab - 1 among them)."""
    g = _gen(f"clipembed.{H}")
    tok = bf16r(torch.randn(vocab, H, generator=g))
    pos = bf16r(torch.randn(L, H, generator=g) * 0.5)
    ids = torch.randint(0, vocab, (n_seq * L,), generator=g, dtype=torch.int32)
    ids[0], ids[1], ids[-1] = vocab - 1, 0, 0
    return tok, pos, ids


def embed_reference(tok, pos, ids, L=EMBED_L):
    out = clip_ref.embed(tok.double(), pos.double(), ids, L)
    return out, out.abs() * U + 2.0 ** -149


EMBED_SLIPS = ("position_of_the_global_row",)


def embed_emulated(tok, pos, ids, L=EMBED_L, slip=None):
    f = torch.float32
    r = torch.arange(ids.shape[0])
    p = torch.clamp(r, max=pos.shape[0] - 1) if slip == "position_of_the_global_row" else r % L   # (clamped to the table)
    return tok.to(f)[ids.long()] + pos.to(f)[p]
