"""Launch forms of the row kernels (conceptattention_amd/csrc/ca_rowops.hip), their fp64 reference and derived bounds.

Imported by tests/test_rowop_routes_gpu.py (the GPU cases) and by tests/test_rowop_cases_cpu.py (coverage of every
launch form of ca_rowops.hip by a case, and the discrimination checks that show each bound rejects a named kernel
slip).  Nothing here touches torch.cuda at import time; the reference and the bounds run on whatever device their
inputs live on.

Every case names the C entry point it calls and the kernel instantiation that entry point launches for its
arguments, spelled as where ca_rowops.hip launches it (CASES; `kernel`).  A reference returns, per output,
(fp64 value, bound before the output's own rounding, kind); `bound` adds the rounding of the kind.

Bounds (elementwise, u = 2^-24 = fp32 unit roundoff; every fp32 operation is charged 2 u of its running magnitude, one
ulp, so a truncating adder is covered as well as a rounding one, as in tests/gemm_route_cases.py):
  sums           a lane sums its n_lane terms in order, then a 64-lane butterfly adds 6 more levels (16-lane groups:
                 4): e = 2 (n_lane + levels + 1) u sum|terms|.  LayerNorm: n_lane = 8 per 512-column chunk; gemv:
                 K / 64 fmas; heat-map logits: dim / 64 fmas; QK norm: 8 products; qpre finish: 8 fmas.
  LayerNorm      mean error e_m = 2 (n_lane + 7) u mean|x|.  The variance is stationary in the mean (sum d = 0), so a
                 mean error enters it only squared: e_var = 2 (n_lane + 10) u var + e_m^2.  rstd = rsqrt(var + eps):
                 relative error e_var / (2 (var + eps)) + RSQ_ULPS u.  t = (x - mean) rstd: rstd (e_m + 2u|d|) +
                 |t| (rel rstd + 2 u).  y = fma(1 + scale, t, shift): |1 + scale| e_t + 2 u |1 + scale| |t| + 2 u |y|.
                 Low plane: hi + lo carries y to 2^-16 (|lo| <= half a bf16 ulp of y, rounded to bf16 itself), and
                 to bf16's subnormal spacing 2^-133 where lo is that small.
  fp8 packs      (ln_modulate_fp8 / quantize_rows_fp8) scale = absmax / 448: e_y(argmax) / 448 + 2 u s.  Bytes: the
                 kernel's own y / s, RNE to e4m3 (v_cvt_pk_fp8_f32, saturated at 448); the test accepts any RNE
                 value of r in [r - e, r + e], e = e_y / s + 4 u |r| (1 / s and the product), so a byte may differ
                 from RNE(y / s) only where y / s lies within e of a rounding tie.  quantize_rows_fp8 has an exact y:
                 its bytes and scales are checked bit for bit against the fp32 formula.
  RMS norm       rrms = rsqrt(mean(x^2) + 1e-6): relative error e_ss / 2 + NORM_ULPS u (rsqrt, the eps add, the two
                 products with rrms and the scale), as in gemm_route_cases.py.
  RoPE           z = (cos y0 - sin y1, sin y0 + cos y1): |cos| E_y0 + |sin| E_y1 + 4 u (|cos y0| + |sin y1|).
  silu           ca_silu = x rcp(1 + exp2(-x log2 e)) with v_exp_f32 / v_rcp_f32: (SILU_ULPS + 2 |x|) u |silu(x)|
                 (the exponent's rounding is amplified by |argument|), plus UNDERFLOW where the rcp may flush.
  softmax        __expf(z - max) = v_exp_f32((z - max) log2 e): each term relative (5 |z - max| + EXP_ULPS) u; the sum
                 over C adds 2 C u; p = term * (w / sum) adds 4 u.  Underflowed terms (|z - max| > 87) are 0 in fp32:
                 an absolute UNDERFLOW |w| is charged.  acc += w p adds 2 u |acc|.
  sparsemax      with z shifted to max 0, tau in [-1, 0) and every support logit in [-1, 0]: the prefix sum and the
                 division give e_tau <= 2 (C + 3) u, the shift z - max 2 u, the clamp 2 u |p|: e_p = 2 (C + 6) u.
                 The support decision is continuous (at a flip both candidate taus agree), so no extra term.
  1.5-entmax     x = (z - max) / 2, support x in [-1, 0]: the mean e_M = 2 (k + 2) u, ss = k (mean sq - M^2)
                 e_ss = 4 (k + 4) k u, a = (1 - ss) / k: e_a = (e_ss + 2 u) / k + 2 u a; sqrt: min(sqrt(e_a),
                 e_a / (2 sqrt(a))) (Hoelder where a ~ 0) + 2 u sqrt(a); p = (x - tau)^2: 2 |x - tau| e_tau + 2 u p.
  trig           timestep embedding: the kernel's argument and the fp32 argument of the reference's formula both carry
                 the fp32 rounding of (log, mul, div, exp, two products): relative (6 |x| + 8) u each, x the exponent
                 (|x| <= ln max_period); cos / sin (ocml) TRIG_ULPS ulps of the result.
  exact          axpy (one fma, rounded once), ca_split_bf16 and ca_modulation_combine_f32 ((h + b) + l, the order its
                 comment states): bit for bit against the same fp32 formula.

Deliberate difference from the model's reference: its RMSNorm rounds x * rrms to the activations' dtype before the
scale (flux/modules/layers.py:72); the kernels do not.  The fp64 reference here is the unrounded formula, as in
oracle/flux_oracle.py:69.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

import gemm_route_cases as G

U = 2.0 ** -24
F32_ULPS = G.F32_ULPS
NORM_ULPS = G.NORM_ULPS
RSQ_ULPS = 2      # v_rsq_f32: 1 ulp, charged 2 u
SILU_ULPS = 8     # v_exp_f32, v_rcp_f32, the add of 1, two products, the fp32 log2(e)
EXP_ULPS = 4      # v_exp_f32 and the fp32 log2(e)
TRIG_ULPS = 4     # ocml cosf / sinf
UNDERFLOW = 2.0 ** -120
Q_SCALE = G.Q_SCALE
EPS = 1e-6

# Measured on MI355X, tests/test_rowop_routes_gpu.py (the printed max err / bound, largest per family):
#   LayerNorm bf16 out 0.500 (the half-ulp store), hi + lo 0.467, fp8 scale 0.043 and bytes within the tie rule;
#   QK norm + RoPE 0.500; q finish fp32 x 0.113, q 0.500 (bf16 and f16); gemv 0.125; silu_split hi 0.500, hi + lo
#   0.473; heat-map logits 0.049 (fused: 0.117), softmax / sparse weighting 0.094; timestep embedding 0.062.
#   Bit for bit: quantize_rows_fp8, ca_split_bf16, ca_modulation_combine_f32, both axpy kernels, the v third.
#   No constant needed widening: every bound above is as derived.


# --------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    entry: str          # the C entry point (include/conceptattn.h)
    kernel: str         # the instantiation it launches, spelled as where ca_rowops.hip launches it
    op: str             # reference family
    shape: dict = field(default_factory=dict, hash=False, compare=False)
    seed: int = 0

    @property
    def id(self):
        return self.name


SEG15 = [0, 3, 3, 12, 13, 21, 100, 101, 250, 250, 400, 555, 556, 700, 777]   # M = 777: empty segments, boundaries
SEG16 = SEG15 + [777]                                                          # inside one wave's 8-row walk
QSEG16 = [0, 1, 3, 3, 5, 8, 13, 17, 20, 25, 30, 30, 37, 41, 49, 50]           # M = 50


def _ln(name, entry, kernel, xdt, out, M, H, segs, ldx=None, ldo=None, ldlo=None, rows="mix", seed=0):
    return Case(name, entry, kernel, "ln", dict(xdt=xdt, out=out, M=M, H=H, segs=segs, ldx=ldx or H, ldo=ldo or H,
                                                 ldlo=ldlo or H, rows=rows), seed)


_R6T, _R6F = "ca_ln_modulate_rows_kernel<6,true>", "ca_ln_modulate_rows_kernel<6,false>"
_LB, _LF = "ca_ln_modulate_kernel<false,bf16>", "ca_ln_modulate_kernel<false,float>"
_LBQ, _LFQ, _LFS = "ca_ln_modulate_kernel<true,bf16>", "ca_ln_modulate_kernel<true,float>", \
    "ca_ln_modulate_kernel<false,float,true>"
CASES = [
    _ln("ln_rows6_split_seg15", "ca_ln_modulate_f32in_split", _R6T, "f32", "split", 777, 3072, SEG15, 3080, 3088, 3104),
    _ln("ln_rows6_seg16", "ca_ln_modulate_f32in", _R6F, "f32", "bf16", 777, 3072, SEG16, 3076, 3080, seed=1),
    _ln("ln_rows6_M9", "ca_ln_modulate_f32in", _R6F, "f32", "bf16", 9, 3072, [2, 2, 9], seed=2),
    _ln("ln_bf16_H8_M7", "ca_ln_modulate_bf16", _LB, "bf16", "bf16", 7, 8, [7], 16, 24, seed=3),
    _ln("ln_bf16_H264_M8", "ca_ln_modulate_bf16", _LB, "bf16", "bf16", 8, 264, [3, 5, 8], seed=4),
    _ln("ln_bf16_H4096_seg15", "ca_ln_modulate_bf16", _LB, "bf16", "bf16", 777, 4096, SEG15, 4104, 4112, seed=5),
    _ln("ln_f32_H264_M1", "ca_ln_modulate_f32in", _LF, "f32", "bf16", 1, 264, [1], 268, seed=6),
    _ln("ln_f32_H4096_M9", "ca_ln_modulate_f32in", _LF, "f32", "bf16", 9, 4096, [2, 2, 9], seed=7),
    _ln("ln_split_H264_M9", "ca_ln_modulate_f32in_split", _LFS, "f32", "split", 9, 264, [4, 9], 272, 280, 296, seed=8),
    _ln("ln_split_H4096_seg16", "ca_ln_modulate_f32in_split", _LFS, "f32", "split", 777, 4096, SEG16, seed=9),
    _ln("ln_fp8_bf16_H3072_M7", "ca_ln_modulate_fp8", _LBQ, "bf16", "fp8", 7, 3072, [3, 7], 3080, 3088, seed=10),
    _ln("ln_fp8_bf16_H8_M9", "ca_ln_modulate_fp8", _LBQ, "bf16", "fp8", 9, 8, [9], ldo=16, seed=11),
    _ln("ln_fp8_f32_H4096_seg15", "ca_ln_modulate_f32in_fp8", _LFQ, "f32", "fp8", 777, 4096, SEG15, 4100, 4112,
        seed=12),
    _ln("ln_fp8_f32_H264_zero_rows", "ca_ln_modulate_f32in_fp8", _LFQ, "f32", "fp8", 9, 264, [9], ldo=272, rows="zero",
        seed=13),

    Case("quant_K520_strided", "ca_quantize_rows_fp8", "ca_quantize_rows_fp8_kernel", "quant",
         dict(M=9, K=520, ldx=536, ldo=528), 20),
    Case("quant_K3072_ties", "ca_quantize_rows_fp8", "ca_quantize_rows_fp8_kernel", "quant",
         dict(M=8, K=3072, ldx=3072, ldo=3072, ties=True), 21),

    Case("qk_h1_M37", "ca_qknorm_rope_bf16", "ca_qknorm_rope_kernel", "qk",
         dict(M=37, heads=1, segs=[37], ld=3 * 128 + 8, pre=False), 30),
    Case("qk_h3_seg16_pre", "ca_qknorm_rope_bf16", "ca_qknorm_rope_kernel", "qk",
         dict(M=50, heads=3, segs=QSEG16, ld=3 * 3 * 128 + 24, pre=True, ldp=3 * 128 + 16), 31),
    Case("qk_h24_M9_pre", "ca_qknorm_rope_bf16", "ca_qknorm_rope_kernel", "qk",
         dict(M=9, heads=24, segs=[4, 9], ld=3 * 24 * 128, pre=True, ldp=24 * 128), 32),

    Case("qpre_h1_no_d", "ca_qpre_finish_f32", "ca_qpre_finish_kernel", "qpre",
         dict(M=33, heads=1, d=False, ldx=136, rope=False), 40),
    Case("qpre_h24_d", "ca_qpre_finish_f32", "ca_qpre_finish_kernel", "qpre",
         dict(M=5, heads=24, d=True, ldx=24 * 128 + 4, ldd=24 * 128 + 8, rope=False), 41),
    Case("qpre_rope_h24_d_bf16_qscale", "ca_qpre_finish_rope_f32", "ca_qpre_finish_kernel", "qpre",
         dict(M=9, heads=24, d=True, ldx=24 * 128 + 4, ldd=24 * 128, rope=True, f16=False, qos=Q_SCALE,
              ldq=24 * 128 + 16), 42),
    Case("qpre_rope_h1_d_f16_noscale", "ca_qpre_finish_rope_f32", "ca_qpre_finish_kernel", "qpre",
         dict(M=17, heads=1, d=True, ldx=128, ldd=132, rope=True, f16=True, qos=0.0, ldq=136), 43),
    Case("qpre_rope_h24_no_d_f16_qscale", "ca_qpre_finish_rope_f32", "ca_qpre_finish_kernel", "qpre",
         dict(M=5, heads=24, d=False, ldx=24 * 128, rope=True, f16=True, qos=Q_SCALE, ldq=24 * 128), 44),
]

_GEMV = [  # nv, K, N, silu, bias, accumulate, ldx, ldo
    (1, 8, 70001, False, False, False, 8, 70001 + 7),       # N > 65 536: the grid-stride loop; no bias
    (2, 264, 1000, True, True, False, 272, 1000),
    (3, 2056, 77, False, True, True, 2056, 80),
    (4, 4096, 300, True, True, True, 4100, 300),
    (5, 4096, 100, True, True, False, 4096, 104),           # 80 KB of LDS: the >64 KB opt-in
    (6, 264, 66001, True, False, True, 264, 66001),         # grid-stride loop, accumulating
    (7, 4096, 33, True, True, True, 4096, 33),
    (8, 3072, 129, False, True, False, 3080, 136),
]
CASES += [Case(f"gemv_nv{nv}_K{K}_N{N}", "ca_gemv_bf16", f"ca_gemv_kernel<{nv}>", "gemv",
               dict(nv=nv, K=K, N=N, silu=s, bias=b, acc=a, ldx=lx, ldo=lo), 50 + nv)
          for nv, K, N, s, b, a, lx, lo in _GEMV]

CASES += [
    Case("silu_split_K12_strided", "ca_silu_split_bf16", "ca_silu_split_kernel<true>", "split",
         dict(silu=True, rows=3, K=12, ldx=20, ldo=16), 60),
    Case("silu_split_grid_stride", "ca_silu_split_bf16", "ca_silu_split_kernel<true>", "split",
         dict(silu=True, rows=300, K=3600, ldx=3604, ldo=3608), 61),          # rows K = 1.08 M > 2^20
    Case("split_K20_strided", "ca_split_bf16", "ca_silu_split_kernel<false>", "split",
         dict(silu=False, rows=5, K=20, ldx=24, ldo=28), 62),
    Case("split_grid_stride", "ca_split_bf16", "ca_silu_split_kernel<false>", "split",
         dict(silu=False, rows=1100, K=1000, ldx=1000, ldo=1004), 63),        # 1.1 M > 2^20
    Case("combine_nv3_N12_no_bias", "ca_modulation_combine_f32", "ca_modulation_combine_kernel", "combine",
         dict(nv=3, N=12, bias=False, ldp=16, ldo=20), 64),
    Case("combine_grid_stride", "ca_modulation_combine_f32", "ca_modulation_combine_kernel", "combine",
         dict(nv=300, N=7204, bias=True, ldp=7208, ldo=7204), 65),            # nv N = 2.16 M > 2^21

    Case("logits_bf16_C5_L4352", "ca_heatmap_logits_bf16", "ca_heatmap_logits_kernel<4,bf16>", "logits",
         dict(img="bf16", con="bf16", C=5, L=4352, dim=3072, ldi=3080, ldc=3076), 70),   # L > 4096: grid-stride
    Case("logits_bf16_C1_L2_dim8", "ca_heatmap_logits_bf16", "ca_heatmap_logits_kernel<4,bf16>", "logits",
         dict(img="bf16", con="bf16", C=1, L=2, dim=8, ldi=8, ldc=8), 71),
    Case("logits_f32con_C3_L257", "ca_heatmap_logits_bf16", "ca_heatmap_logits_kernel<4,float>", "logits",
         dict(img="bf16", con="f32", C=3, L=257, dim=264, ldi=264, ldc=268), 72),
    Case("logits_f32_C11_L1_dim8", "ca_heatmap_logits_bf16", "ca_heatmap_logits_kernel<4,float,float>", "logits",
         dict(img="f32", con="f32", C=11, L=1, dim=8, ldi=16, ldc=8), 73),
    Case("logits_f32_C8_L257_dim4096", "ca_heatmap_logits_bf16", "ca_heatmap_logits_kernel<4,float,float>", "logits",
         dict(img="f32", con="f32", C=8, L=257, dim=4096, ldi=4104, ldc=4100), 74),

    Case("softmax_C1", "ca_heatmap_softmax_accumulate", "ca_heatmap_softmax_kernel", "norm",
         dict(norm="softmax", C=1, L=300, w=0.7), 80),
    Case("softmax_C9_spread300", "ca_heatmap_norm_accumulate", "ca_heatmap_softmax_kernel", "norm",
         dict(norm="softmax", C=9, L=257, w=0.7), 81),
    Case("sparsemax_C8", "ca_heatmap_norm_accumulate", "ca_heatmap_sparse_kernel<8,false>", "norm",
         dict(norm="sparsemax", C=8, L=300, w=0.7), 82),
    Case("sparsemax_C9", "ca_heatmap_norm_accumulate", "ca_heatmap_sparse_kernel<16,false>", "norm",
         dict(norm="sparsemax", C=9, L=257, w=1.3), 83),
    Case("entmax_C1", "ca_heatmap_norm_accumulate", "ca_heatmap_sparse_kernel<8,true>", "norm",
         dict(norm="entmax15", C=1, L=40, w=0.7), 84),
    Case("entmax_C8", "ca_heatmap_norm_accumulate", "ca_heatmap_sparse_kernel<8,true>", "norm",
         dict(norm="entmax15", C=8, L=300, w=0.7), 85),
    Case("entmax_C16", "ca_heatmap_norm_accumulate", "ca_heatmap_sparse_kernel<16,true>", "norm",
         dict(norm="entmax15", C=16, L=257, w=1.3), 86),

    Case("fused4_part_softmax", "ca_heatmap_fused", "ca_heatmap_fused_kernel<4>", "fused",
         dict(form="part", C=3, L=300, heads=24, norm="softmax"), 90),
    Case("fused8_part_sparsemax", "ca_heatmap_fused", "ca_heatmap_fused_kernel<8>", "fused",
         dict(form="part", C=8, L=257, heads=5, norm="sparsemax"), 91),
    Case("fused4_bf16_vectors", "ca_heatmap_fused", "ca_heatmap_fused_kernel<4>", "fused",
         dict(form="bf16", C=4, L=101, dim=264, norm="softmax"), 92),
    Case("fused8_f32_vectors", "ca_heatmap_fused", "ca_heatmap_fused_kernel<8>", "fused",
         dict(form="f32", C=6, L=65, dim=3072, norm="entmax15"), 93),

    Case("axpy_n5", "ca_axpy_bf16", "ca_axpy_kernel", "axpy", dict(y="bf16x", n=5, a=-0.37), 100),
    Case("axpy_n1003", "ca_axpy_bf16", "ca_axpy_kernel", "axpy", dict(y="bf16x", n=1003, a=0.61), 101),
    Case("axpy_f32_bf16y_n7", "ca_axpy_f32", "ca_axpy_f32_kernel<bf16>", "axpy", dict(y="bf16", n=7, a=-0.37), 102),
    Case("axpy_f32_bf16y_n1003", "ca_axpy_f32", "ca_axpy_f32_kernel<bf16>", "axpy",
         dict(y="bf16", n=1003, a=0.61), 103),
    Case("axpy_f32_f32y_n4099", "ca_axpy_f32", "ca_axpy_f32_kernel<float>", "axpy", dict(y="f32", n=4099, a=-0.0123),
         104),

    Case("temb_dim2_t", "ca_timestep_embedding_f32", "ca_timestep_embedding_kernel", "temb",
         dict(nt=3, dim=2, tmax=1.0, tf=1000.0), 110),
    Case("temb_dim256_t", "ca_timestep_embedding_f32", "ca_timestep_embedding_kernel", "temb",
         dict(nt=7, dim=256, tmax=1.0, tf=1000.0), 111),
    Case("temb_dim256_guidance", "ca_timestep_embedding_f32", "ca_timestep_embedding_kernel", "temb",
         dict(nt=5, dim=256, tmax=3.5, tf=1000.0), 112),
    Case("temb_grid_stride", "ca_timestep_embedding_f32", "ca_timestep_embedding_kernel", "temb",
         dict(nt=8200, dim=256, tmax=1.0, tf=1000.0), 113),                    # nt dim / 2 = 1.05 M > 4096 x 256 threads
]
BY_ID = {c.id: c for c in CASES}


# --------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed), dtype=torch.float64) * scale


def _padded(vals: torch.Tensor, ld: int, fill=float("nan")) -> torch.Tensor:
    """[rows, ld] with vals in the first columns and `fill` in the padding (what a kernel must not read or write)."""
    out = torch.full((vals.shape[0], ld), fill, dtype=vals.dtype)
    out[:, :vals.shape[1]] = vals
    return out


def make_inputs(case: Case) -> dict:
    """Host (CPU) tensors of one case; row-strided operands carry NaN in their padding columns."""
    s, sd = case.shape, case.seed
    if case.op == "ln":
        M, H = s["M"], s["H"]
        X = _randn((M, H), sd, 2.0) + 0.3
        if s["rows"] == "zero":
            X[2], X[5] = 0.0, 0.0
        else:
            r = torch.arange(M)
            big = (r % 11 == 3)
            X[big] = 1000.0 + _randn((int(big.sum()), H), sd + 1)          # mean ~1e3, std ~1
            X[r % 13 == 5] = 0.75                                          # constant rows: var = 0
            X[r % 13 == 9] = -2.5
        xdt = torch.float32 if s["xdt"] == "f32" else torch.bfloat16
        n = len(s["segs"])
        shift = [_randn((H,), sd + 100 + i).float() for i in range(n)]
        if s["rows"] == "zero":
            shift = [torch.zeros(H) for _ in range(n)]
        scale = [(_randn((H,), sd + 200 + i, 0.3)).float() for i in range(n)]
        return dict(x=_padded(X.to(xdt), s["ldx"]), shift=shift, scale=scale)
    if case.op == "quant":
        M, K = s["M"], s["K"]
        X = _randn((M, K), sd, 3.0)
        X[3] = 0.0                                                         # zero row: scale 1, bytes 0
        if s.get("ties"):
            # rows of absmax 448 (scale exactly 1): values on e4m3 rounding ties, both parities
            mant = torch.randint(0, 8, (M, K), generator=_gen(sd + 1)).double()
            ex = torch.randint(-6, 8, (M, K), generator=_gen(sd + 2)).double()
            sign = torch.randint(0, 2, (M, K), generator=_gen(sd + 3)).double() * 2 - 1
            ties = sign * (1 + (mant + 0.5) / 8) * torch.pow(2.0, ex)
            X[::2] = ties[::2]
            X[::2, 7] = 448.0
        return dict(x=_padded(X.bfloat16(), s["ldx"]))
    if case.op == "qk":
        M, nh = s["M"], s["heads"]
        X = _randn((M, 3 * nh * 128), sd, 2.0)
        X[:, :nh * 128] += _randn((1, nh * 128), sd + 1, 0.5)           # uneven rows: norms differ per head
        n = len(s["segs"])
        qs = [(0.5 + torch.rand(128, generator=_gen(sd + 10 + i))).bfloat16() for i in range(n)]
        ks = [(0.5 + torch.rand(128, generator=_gen(sd + 40 + i))).bfloat16() for i in range(n)]
        return dict(qkv=_padded(X.bfloat16(), s["ld"]), q_scale=qs, k_scale=ks, rope=G.rope_table(M, sd + 2))
    if case.op == "qpre":
        M, W = s["M"], s["heads"] * 128
        out = dict(x=_padded(_randn((M, W), sd, 1.5).float(), s["ldx"]),
                   scale=(0.5 + torch.rand(128, generator=_gen(sd + 1))).bfloat16())
        if s["d"]:
            out["d"] = _padded(_randn((M, W), sd + 2, 0.01).float(), s["ldd"])
        if s["rope"]:
            out["rope"] = G.rope_table(M, sd + 3)
        return out
    if case.op == "gemv":
        nv, K, N = s["nv"], s["K"], s["N"]
        out = dict(x=_padded(_randn((nv, K), sd, 1.5).float(), s["ldx"]),
                   w=(_randn((N, K), sd + 1) / math.sqrt(K)).bfloat16())
        if s["bias"]:
            out["bias"] = _randn((N,), sd + 2, 0.5).bfloat16()
        if s["acc"]:
            out["out0"] = _randn((nv, N), sd + 3).float()
        return out
    if case.op == "split":
        X = _randn((s["rows"], s["K"]), sd, 3.0).float()
        X[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -87.0])
        return dict(x=_padded(X, s["ldx"]))
    if case.op == "combine":
        nv, N = s["nv"], s["N"]
        out = dict(pair=_padded(_randn((2 * nv, N), sd, 1.0).float(), s["ldp"]))
        out["pair"][nv:, :N] *= 1e-3                                       # the low plane's products: small
        if s["bias"]:
            out["bias"] = _randn((N,), sd + 1, 0.5).bfloat16()
        return out
    if case.op == "logits":
        C, Lp, dim = s["C"], s["L"], s["dim"]
        img = _randn((Lp, dim), sd)
        con = _randn((C, dim), sd + 1, 0.05)
        return dict(img=_padded(img.float() if s["img"] == "f32" else img.bfloat16(), s["ldi"]),
                    con=_padded(con.float() if s["con"] == "f32" else con.bfloat16(), s["ldc"]))
    if case.op == "norm":
        return dict(logits=norm_logits(s["C"], s["L"], sd), acc0=_randn((s["C"], s["L"]), sd + 5, 0.5).float())
    if case.op == "fused":
        C, Lp = s["C"], s["L"]
        out = dict(acc0=_randn((C, Lp), sd + 5, 0.5).float())
        if s["form"] == "part":
            out["part"] = (_randn((s["heads"], Lp, 8), sd, 0.4)).float()
        else:
            dt = torch.float32 if s["form"] == "f32" else torch.bfloat16
            out["img"] = _randn((Lp, s["dim"]), sd).to(dt)
            out["con"] = _randn((C, s["dim"]), sd + 1, 2.0 / math.sqrt(s["dim"])).to(dt)
        return out
    if case.op == "axpy":
        n = s["n"]
        xdt = torch.bfloat16 if s["y"] == "bf16x" else torch.float32
        ydt = torch.float32 if s["y"] == "f32" else torch.bfloat16
        return dict(x=_randn((n,), sd).to(xdt), y=_randn((n,), sd + 1).to(ydt))
    if case.op == "temb":
        t = torch.rand(s["nt"], generator=_gen(sd), dtype=torch.float64) * s["tmax"]
        t[0] = 0.0
        t[-1] = s["tmax"]
        return dict(t=t.float())
    raise KeyError(case.op)


def norm_logits(C: int, Lp: int, seed: int) -> torch.Tensor:
    """[C, L] fp32 logits: unit-scale columns, tied columns, columns of spread +-300, one large shared offset."""
    z = _randn((C, Lp), seed, 1.5)
    p = torch.arange(Lp)
    z[:, p % 7 == 1] = 0.625                                           # all C tied
    z[:, p % 7 == 2] = z[:, p % 7 == 2].round()                        # partial ties
    sp = p % 7 == 3
    z[:, sp] = torch.rand(C, int(sp.sum()), generator=_gen(seed + 1), dtype=torch.float64) * 600 - 300
    z[:, p % 7 == 4] += 250.0
    return z.float()


# --------------------------------------------------------------------------------------------------- reference
def seg_index(M: int, row_ends, dev, late=False) -> torch.Tensor:
    """The segment of every row, as the kernels pick it: the number of s < n - 1 with row_end[s] <= row."""
    rows = torch.arange(M, device=dev)
    if late:                                        # slip: the segment of the row before
        rows = (rows - 1).clamp(min=0)
    ends = torch.tensor(row_ends[:-1], device=dev, dtype=torch.int64)
    return (ends[None] <= rows[:, None]).sum(1)


def _rowsum(t):
    return t.sum(-1, keepdim=True)


def ln_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    mutate = mutate or {}
    s = case.shape
    M, H = s["M"], s["H"]
    X = inp["x"].to(dev)[:, :H].double()
    idx = seg_index(M, s["segs"], dev, late=mutate.get("seg_late", False))
    SH = torch.stack([t.to(dev).double() for t in inp["shift"]])[idx]
    SC = torch.stack([t.to(dev).double() for t in inp["scale"]])[idx]
    Xs, Hs = X, H
    if "drop_last_chunk" in mutate:                 # slip: the last 512-column chunk left out of the row statistics
        Hs = 512 * ((H - 1) // 512)
        Xs = X[:, :Hs]
    mean = _rowsum(Xs) / Hs
    d = X - mean
    var = _rowsum((Xs - mean) ** 2) / (Hs - 1 if mutate.get("var_h1") else Hs)
    eps = 0.0 if mutate.get("no_eps") else EPS
    rstd = 1.0 / torch.sqrt(var + eps)
    t = d * rstd
    sc1 = 1.0 + SC
    y = sc1 * t + SH
    nl = 8 * -(-H // 512)
    e_m = 2 * (nl + 7) * U * _rowsum(X.abs()) / H
    var0 = _rowsum(d ** 2) / H
    rel_r = (2 * (nl + 10) * U * var0 + e_m ** 2) / (2 * (var0 + EPS)) + RSQ_ULPS * U
    e_t = rstd * (e_m + 2 * U * d.abs()) + t.abs() * (rel_r + 2 * U)
    e_y = sc1.abs() * e_t + 2 * U * sc1.abs() * t.abs() + 2 * U * y.abs()
    if s["out"] == "bf16":
        return {"out": (y, e_y, "bf16")}
    if s["out"] == "split":
        return {"out": (y, e_y, "bf16"), "hi+lo": (y, e_y, "hilo")}
    return fp8_outputs(y, e_y, scale_got)


def fp8_outputs(y, e_y, scale_got):
    amax = y.abs().amax(-1, keepdim=True)
    s_ref = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    e_s = torch.gather(e_y, 1, y.abs().argmax(-1, keepdim=True)) / 448.0 + 2 * U * s_ref
    s_k = s_ref.float().double() if scale_got is None else scale_got.to(y.device).double().reshape(-1, 1)
    r = y / s_k
    return {"scale": (s_ref.reshape(-1), e_s.reshape(-1), "f32"), "q": (r, e_y / s_k + 4 * U * r.abs(), "fp8")}


def quant_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    """Exact: scale = fp32(amax * fp32(1/448)) (1 if amax = 0), bytes = RNE_e4m3(clamp(fp32(x * fp32(1 / scale))))."""
    s = case.shape
    X = inp["x"].to(dev)[:, :s["K"]].float()
    amax = X.abs().amax(-1, keepdim=True)
    sc = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32, device=dev), torch.ones_like(amax))
    inv = (1.0 / sc.double()).float()
    r = (X * inv).clamp(-448, 448)
    return {"scale": (sc.reshape(-1).double(), None, "exact"), "q": (r.double(), None, "fp8exact")}


def _rope_apply(y, rope, mutate, e_y):
    """z = (cos y0 - sin y1, sin y0 + cos y1) per pair and its bound; y / e_y [M, heads, 128], rope [M, 64, 2]."""
    cs, sn = rope[:, None, :, 0], rope[:, None, :, 1]
    y0, y1 = y[..., 0::2], y[..., 1::2]
    if "rope_swap" in mutate:                       # slip: the two elements of pair p exchanged
        p = mutate["rope_swap"]
        y0, y1 = y0.clone(), y1.clone()
        y0[..., p], y1[..., p] = y[..., 2 * p + 1], y[..., 2 * p]
    sgn = -1.0 if mutate.get("sin_sign") else 1.0  # slip: the sine's sign flipped
    z = torch.stack((cs * y0 - sgn * sn * y1, sgn * sn * y0 + cs * y1), -1).reshape(y.shape)
    e0, e1 = e_y[..., 0::2], e_y[..., 1::2]
    ez0 = cs.abs() * e0 + sn.abs() * e1 + 4 * U * ((cs * y0).abs() + (sn * y1).abs())
    ez1 = sn.abs() * e0 + cs.abs() * e1 + 4 * U * ((sn * y0).abs() + (cs * y1).abs())
    return z, torch.stack((ez0, ez1), -1).reshape(y.shape)


def _rms(x, ncols, e_rel_ss):
    """x * rsqrt(mean(x^2) + eps) over the last axis (ncols of 128 counted: slip) and the relative error of rrms."""
    rr = 1.0 / torch.sqrt((x[..., :ncols] ** 2).sum(-1, keepdim=True) / ncols + EPS)
    return rr, e_rel_ss / 2 + NORM_ULPS * U


def qk_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    mutate = mutate or {}
    s = case.shape
    M, nh = s["M"], s["heads"]
    X = inp["qkv"].to(dev)[:, :3 * nh * 128].double().reshape(M, 3, nh, 128)
    idx = seg_index(M, s["segs"], dev)
    rope = inp["rope"].to(dev).double()
    out = {}
    for which, name in ((0, "q"), (1, "k")):
        sc = torch.stack([t.to(dev).double() for t in inp["q_scale" if which == 0 else "k_scale"]])[idx][:, None]
        x = X[:, which]
        rr, rel = _rms(x, mutate.get("norm_cols", 128), 2 * (8 + 4 + 1) * U)
        y = x * rr * sc
        e_y = rel * y.abs()
        z, e_z = _rope_apply(y, rope, mutate, e_y)
        out[name] = (z.reshape(M, -1), e_z.reshape(M, -1), "bf16")
        if which == 0 and s["pre"]:
            out["q_prerope"] = (y.reshape(M, -1), e_y.reshape(M, -1), "bf16")
    out["v"] = (X[:, 2].reshape(M, -1), None, "exact")
    return out


def qpre_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    mutate = mutate or {}
    s = case.shape
    M, nh = s["M"], s["heads"]
    W = nh * 128
    x = inp["x"].to(dev)[:, :W].double()
    a = x + inp["d"].to(dev)[:, :W].double() if s["d"] else x
    a = a.reshape(M, nh, 128)
    rr, rel = _rms(a, mutate.get("norm_cols", 128), 2 * (8 + 4 + 2) * U)
    sc = inp["scale"].to(dev).double()
    y = a * rr * sc
    e_y = (rel + (4 * U if s["d"] else 0.0)) * y.abs()   # (the x + d add: 2 u relative, seen through the norm twice)
    out = {"x": (y.reshape(M, -1), e_y.reshape(M, -1), "f32")}
    if s["rope"]:
        z, e_z = _rope_apply(y, inp["rope"].to(dev).double(), mutate, e_y)
        qos = s["qos"] if s["qos"] else 1.0
        z, e_z = z * qos, e_z * qos + 2 * U * (z * qos).abs()
        out["q"] = (z.reshape(M, -1), e_z.reshape(M, -1), "f16" if s["f16"] else "bf16")
    return out


def silu_and_bound(x):
    sil = x / (1 + torch.exp(-x))
    return sil, (SILU_ULPS + 2 * x.abs()) * U * sil.abs() + UNDERFLOW   # (v_rcp_f32 may flush a subnormal result)


def gemv_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    mutate = mutate or {}
    s = case.shape
    nv, K, N = s["nv"], s["K"], s["N"]
    x = inp["x"].to(dev)[:, :K].double()
    f, e_f = silu_and_bound(x) if s["silu"] else (x, torch.zeros_like(x))
    w = inp["w"].to(dev).double()
    acc = f @ w.T
    S = f.abs() @ w.abs().T
    E = e_f @ w.abs().T
    if "bias" in inp:
        b = inp["bias"].to(dev).double()
        acc, S = acc + b, S + b.abs()
    if "out0" in inp:
        o0 = inp["out0"].to(dev).double()
        acc, S = acc + o0, S + o0.abs()
    c = 2 * (K / 64 + 6 + 2)
    if "skip_rows" in mutate:                       # slip: rows past the first n never written
        acc = acc.clone()
        acc[:, mutate["skip_rows"]:] = float("nan")
    return {"out": (acc, c * U * S + E, "f32")}


def split_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    s = case.shape
    X = inp["x"].to(dev)[:, :s["K"]]
    if not s["silu"]:                               # exact: hi = bf16(x), lo = bf16(x - hi) (the difference is exact)
        hi = X.float().bfloat16()
        lo = (X.float() - hi.float()).bfloat16()
        return {"hi": (hi.double(), None, "exact"), "lo": (lo.double(), None, "exact")}
    sil, e = silu_and_bound(X.double())
    return {"hi": (sil, e, "bf16"), "hi+lo": (sil, e, "hilo")}


def combine_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    """Exact: out = (h + float(bias)) + l in fp32, in that order."""
    s = case.shape
    nv, N = s["nv"], s["N"]
    P = inp["pair"].to(dev)[:, :N].float()
    b = inp["bias"].to(dev).float() if "bias" in inp else torch.zeros(N, device=dev)
    o = ((P[:nv] + b[None]) + P[nv:]).double()
    if "unwritten" in (mutate or {}):
        o = o.clone()
        o[mutate["unwritten"]] = float("nan")
    return {"out": (o, None, "exact")}


def logits_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    mutate = mutate or {}
    s = case.shape
    dim = s["dim"]
    img = inp["img"].to(dev)[:, :dim].double()
    con = inp["con"].to(dev)[:, :dim].double()
    z = con @ img.T
    S = con.abs() @ img.abs().T
    if mutate.get("drop_last_chunk"):               # slip: the launch of the last 4-concept chunk left out
        z = z.clone()
        z[4 * ((s["C"] - 1) // 4):] = float("nan")
    c = 2 * (dim / 64 + 6 + 1)
    return {"logits": (z, c * U * S, "f32")}


def _softmax_terms(z, e_z, mutate):
    """fp64 softmax over axis 0 of z [C, L] and its pre-rounding relative bound, e_z the logits' own bound."""
    C = z.shape[0]
    mx = z.amax(0, keepdim=True)
    if mutate.get("no_max_sub"):                    # slip: exp(z) in fp32 without the max subtraction
        e = torch.exp(z.float()).double()
        return e / e.sum(0, keepdim=True), None
    p = torch.softmax(z, 0)
    rel = (5 * (z - mx).abs() + EXP_ULPS) * U
    rel_p = rel + (p * rel).sum(0, keepdim=True) + (2 * C + 4) * U
    if e_z is not None:                             # first order: d log p_c = dz_c - sum_j p_j dz_j
        ez = e_z.amax(0, keepdim=True)
        rel_p = rel_p + 2 * ez
    return p, rel_p


def sparse_terms(z, norm, mutate=None):
    """fp64 sparsemax / 1.5-entmax over axis 0 (oracle/sparse_norms.py), with the slip of a support off by one."""
    from oracle import sparse_norms as SN
    mutate = mutate or {}
    zz = z.detach().cpu().double().numpy()
    if norm == "sparsemax" and mutate.get("support_off_by_one"):
        import numpy as np
        zs = zz - zz.max(0, keepdims=True)
        srt = -np.sort(-zs, axis=0)
        cs = np.cumsum(srt, 0)
        rho = np.arange(1, zs.shape[0] + 1)[:, None]
        k = (1 + rho * srt > cs).sum(0, keepdims=True)
        k = np.minimum(k + 1, zs.shape[0])
        tau = (np.take_along_axis(cs, k - 1, 0) - 1) / k
        p = np.maximum(zs - tau, 0)
    else:
        p = (SN.sparsemax if norm == "sparsemax" else SN.entmax15)(zz, axis=0)
    return torch.from_numpy(p).to(z.device)


def sparse_bound(z, p, norm):
    """Absolute pre-rounding bound of each p (see the module docstring)."""
    C = z.shape[0]
    if norm == "sparsemax":
        return torch.full_like(p, 2 * (C + 6) * U)
    x = (z - z.amax(0, keepdim=True)) / 2
    sup = p > 0
    k = sup.sum(0, keepdim=True).double()
    tau = torch.where(sup, x - torch.sqrt(p), torch.full_like(p, -1e300)).amax(0, keepdim=True)
    M = torch.where(sup, x, torch.zeros_like(x)).sum(0, keepdim=True) / k
    sq = (M - tau).clamp(min=0)                     # sqrt(a)
    e_M = 2 * (k + 2) * U
    e_a = (4 * (k + 4) * k * U + 2 * U) / k + 2 * U * sq ** 2
    e_sqrt = torch.minimum(torch.sqrt(e_a), e_a / (2 * sq).clamp(min=1e-300)) + 2 * U * sq
    e_tau = e_M + e_sqrt + 2 * U
    return 2 * (x - tau).abs() * e_tau * sup + 2 * U * p + 2 * e_tau ** 2


def weighted(z, e_z, norm, w, acc0, mutate=None):
    """acc0 + w * norm_c(z) in fp64 and its bound before the fp32 store (e_z: the bound of the logits, or None)."""
    mutate = mutate or {}
    if norm == "softmax":
        p, rel_p = _softmax_terms(z, e_z, mutate)
        e_p = p * rel_p + UNDERFLOW if rel_p is not None else None
    else:
        p = sparse_terms(z, norm, mutate)
        e_p = sparse_bound(z, p, norm)
        if e_z is not None:                         # both maps are 1-Lipschitz (sparsemax) / 2-Lipschitz in z
            e_p = e_p + 2 * e_z.amax(0, keepdim=True)
    o = acc0 + w * p
    pre = None if e_p is None else abs(w) * e_p + 2 * U * (w * p).abs() + 2 * U * o.abs()
    if pre is None:
        pre = torch.zeros_like(o)
    return o, pre


def norm_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    s = case.shape
    z = inp["logits"].to(dev).double()
    o, pre = weighted(z, None, s["norm"], s["w"], inp["acc0"].to(dev).double(), mutate)
    return {"acc": (o, pre, "f32")}


def fused_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    s = case.shape
    if s["form"] == "part":
        part = inp["part"].to(dev).double()[..., :s["C"]]              # [heads, L, C]
        z = part.sum(0).T
        e_z = 2 * s["heads"] * U * part.abs().sum(0).T
    else:
        img, con = inp["img"].to(dev).double(), inp["con"].to(dev).double()
        z = con @ img.T
        e_z = 2 * (s["dim"] / 64 + 6 + 1) * U * (con.abs() @ img.abs().T)
    o, pre = weighted(z, e_z, s["norm"], FUSED_W, inp["acc0"].to(dev).double(), mutate)
    return {"logits": (z, e_z, "f32"), "acc": (o, pre, "f32")}


FUSED_W = 0.45


def axpy_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    """Exact: fp32 fma(a, y, x) (a * y exact in fp64, the sum rounded once to fp32), then bf16 for a bf16 x."""
    s = case.shape
    a = torch.tensor(s["a"], dtype=torch.float32).double().item()
    x, y = inp["x"].to(dev), inp["y"].to(dev)
    r = (a * y.double() + x.double()).float()
    if x.dtype == torch.bfloat16:
        r = r.bfloat16()
    return {"x": (r.double(), None, "exact")}


def temb_reference(case, inp, dev="cpu", mutate=None, scale_got=None):
    """cos / sin in fp64 of the argument the model's reference forms in fp32 (flux/modules/layers.py:28-49:
    t = tf * t; freqs = exp(-ln(max_period) * arange(half) / half); args = t * freqs)."""
    mutate = mutate or {}
    s = case.shape
    half = s["dim"] // 2
    t = inp["t"].to(dev).float()
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=dev) / half)
    arg = ((s["tf"] * t)[:, None] * freqs[None]).double()
    xk = math.log(10000.0) * torch.arange(half, dtype=torch.float64, device=dev) / half
    e_arg = 2 * (6 * xk + 8)[None] * U * arg.abs()     # both fp32 chains
    c, sn = torch.cos(arg), torch.sin(arg)
    if mutate.get("swap_halves"):                   # slip: sin first, cos second
        c, sn = sn, c
    e_c = sn.abs() * e_arg + TRIG_ULPS * G.ulp(torch.cos(arg), "f32")
    e_s = c.abs() * e_arg + TRIG_ULPS * G.ulp(torch.sin(arg), "f32")
    if mutate.get("swap_halves"):
        e_c, e_s = e_s, e_c
    return {"out": (torch.cat((c, sn), 1), torch.cat((e_c, e_s), 1), "f32")}


REFERENCES = {"ln": ln_reference, "quant": quant_reference, "qk": qk_reference, "qpre": qpre_reference,
              "gemv": gemv_reference, "split": split_reference, "combine": combine_reference,
              "logits": logits_reference, "norm": norm_reference, "fused": fused_reference, "axpy": axpy_reference,
              "temb": temb_reference}


def reference(case, inp, dev="cpu", mutate=None, scale_got=None) -> dict:
    """fp64 reference of every output of the case: name -> (ref, bound before the output rounding, kind)."""
    return REFERENCES[case.op](case, inp, dev, mutate, scale_got)


# --------------------------------------------------------------------------------------------------- bounds
def e4m3(v: torch.Tensor) -> torch.Tensor:
    """RNE to OCP e4m3 (saturated at +-448), as fp64."""
    return v.clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn).double()


def bound(ref, pre, kind):
    if kind == "hilo":
        return pre + 2.0 ** -16 * ref.abs() + 2.0 ** -133 + F32_ULPS * G.ulp(ref, "f32")   # (lo: bf16 subnormals)
    if kind == "f32":
        return pre + F32_ULPS * G.ulp(ref, "f32")
    return pre + G.ulp(ref, kind)


def excess(got: torch.Tensor, ref: torch.Tensor, pre, kind: str):
    """(max |got - ref| / bound, number of elements NOT within the bound).  NaN / inf (an output the kernel never
    wrote keeps the NaN or 0xFF it was filled with) counts as over the bound.  `got` for fp8 kinds: decoded bytes."""
    got = got.to(ref.device).double()
    if not ref.numel():
        return 0.0, 0
    if kind == "exact":
        same = got == ref
        return (0.0 if bool(same.all()) else math.inf), int((~same).sum().item())
    if kind == "fp8exact":
        want = e4m3(ref)
        same = got == want
        return (0.0 if bool(same.all()) else math.inf), int((~same).sum().item())
    if kind == "fp8":
        lo, hi = e4m3(ref - pre), e4m3(ref + pre)
        ok = (got >= lo) & (got <= hi)
        spacing = (hi - lo).clamp(min=0)
        half = (e4m3(ref) - ref).abs()
        ratio = ((got - ref).abs() - half) / (pre + spacing).clamp(min=1e-300)
        return max(0.0, ratio.max().item()) if bool(ok.all()) else math.inf, int((~ok).sum().item())
    err = (got - ref).abs()
    ratio = err / bound(ref, pre, kind)
    return ratio.max().item(), int((~(ratio <= 1)).sum().item())


def rounded_like_output(t: torch.Tensor, kind: str) -> torch.Tensor:
    """A reference value stored as the kernel stores it (the discrimination checks' emulation of a correct kernel)."""
    if kind in ("exact", "fp8exact"):
        return t.clone() if kind == "exact" else e4m3(t)
    if kind == "fp8":
        return e4m3(t)
    if kind == "hilo":
        y = t.float()
        hi = y.bfloat16().float()
        return hi.double() + (y - hi).bfloat16().double()
    return G.rounded_like_output(t, kind)


# ----------------------------------------------------------------------------------- discrimination (CPU)
SLIPS = {
    # name: (case, mutate, output that must expose it)
    "variance over H - 1": ("ln_split_H264_M9", {"var_h1": True}, "hi+lo"),
    "variance over H - 1 (H = 8)": ("ln_bf16_H8_M7", {"var_h1": True}, "out"),
    "eps omitted (constant rows)": ("ln_rows6_split_seg15", {"no_eps": True}, "out"),
    "segment chosen one row late": ("ln_rows6_seg16", {"seg_late": True}, "out"),
    "segment chosen one row late (fp8)": ("ln_fp8_f32_H4096_seg15", {"seg_late": True}, "q"),
    "last 512-column chunk dropped": ("ln_rows6_M9", {"drop_last_chunk": True}, "out"),
    "last 512-column chunk dropped (H % 512 != 0)": ("ln_split_H4096_seg16", {"drop_last_chunk": True}, "hi+lo"),
    "RoPE pair order swapped": ("qk_h3_seg16_pre", {"rope_swap": 9}, "k"),
    "RoPE sin sign swapped": ("qk_h1_M37", {"sin_sign": True}, "q"),
    "RoPE sin sign swapped in the q finish": ("qpre_rope_h1_d_f16_noscale", {"sin_sign": True}, "q"),
    "RMS over 64 rather than 128 columns": ("qk_h24_M9_pre", {"norm_cols": 64}, "q_prerope"),
    "RMS over 64 columns in the fp32 q finish": ("qpre_h24_d", {"norm_cols": 64}, "x"),
    "gemv skips rows past the first 65 536": ("gemv_nv1_K8_N70001", {"skip_rows": 65536}, "out"),
    "last concept chunk dropped in the logits": ("logits_bf16_C5_L4352", {"drop_last_chunk": True}, "logits"),
    "softmax without max-subtraction": ("softmax_C9_spread300", {"no_max_sub": True}, "acc"),
    "sparsemax support off by one": ("sparsemax_C9", {"support_off_by_one": True}, "acc"),
    "cos / sin halves swapped": ("temb_dim256_t", {"swap_halves": True}, "out"),
    "truncating fp8 pack": ("ln_fp8_bf16_H3072_M7", {"trunc_fp8": True}, "q"),
    "truncating fp8 pack (quantize)": ("quant_K520_strided", {"trunc_fp8": True}, "q"),
    "one output element never written": ("combine_nv3_N12_no_bias", {"unwritten": (1, 5)}, "out"),
}


def trunc_e4m3(v: torch.Tensor) -> torch.Tensor:
    """e4m3 by truncation toward zero of the fp32 mantissa to 3 bits (normal range), saturated at 448."""
    f = v.clamp(-448.0, 448.0).float()
    bits = f.view(torch.int32) & ~((1 << 20) - 1)
    return bits.view(torch.float32).to(torch.float8_e4m3fn).double()


def discrimination(name: str):
    """On the CPU: the fp64 reference, stored as the kernel stores it, passes every bound of its case; the same
    computation with the named slip fails the bound of the output that carries it.  Returns (the faithful emulation
    passes, elements over the bound with the slip)."""
    cid, mutate, which = SLIPS[name]
    case = BY_ID[cid]
    inp = make_inputs(case)
    good = reference(case, inp)
    ok = True
    for k, (ref, pre, kind) in good.items():
        _, n_over = excess(rounded_like_output(ref, kind), ref, pre, kind)
        ok &= n_over == 0
    ref, pre, kind = good[which]
    if "trunc_fp8" in mutate:
        got = trunc_e4m3(ref)
    else:
        bad = reference(case, inp, mutate=mutate)
        got = rounded_like_output(bad[which][0], kind)
    _, n_bad = excess(got, ref, pre, kind)
    return ok, n_bad
