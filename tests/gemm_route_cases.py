"""Route x epilogue x precision matrix of the grouped GEMM, and its fp64 reference with derived error bounds.

Imported by tests/test_gemm_routes_gpu.py (the GPU cases) and by tests/test_gemm_plan_cpu.py (route coverage of the
model's launch table, and the discrimination checks that show each bound rejects a realistic kernel slip).  Nothing
here touches torch.cuda at import time; the reference and the bounds run on whatever device their inputs live on.

Routes (ca_gemm_plan decides them, the shapes are searched so that the plan says what the case name claims):
  classic_<w>         ca_gemm_kernel, 256 x w tiles, one workgroup per tile
  pp<w>[_persist]     the ping-pong kernel, 256 x w tiles, one tile per workgroup / persistent walk
  pp256_thin_walk     256 x 256 ping-pong walk whose last row tile (1..128 rows) rides at the end of the walk
  thin_<MF>x<NW>      the same thin part in its own launch of ca_gemm_thin_kernel<MF, NW>, main tiles present
  fp8[_persist|_thin_walk]  the fp8 ping-pong kernel (thin tiles always ride in its walk)

Bounds (all elementwise, u = 2^-24 = fp32 unit roundoff):
  accumulation   e_acc = c * u * S,  S = |A| @ |W|^T (+ |bias|, + |raw q| for qpre_add; times a_scale * w_scale for
                 fp8).  bf16: c = 2 * (K / 32 + log2(32) + 4): one accumulator update per MFMA (32 products),
                 log2(32) additions inside one MFMA's product sum, 4 for the fp32 epilogue operations before the first
                 non-linear step (bias, raw q), each charged 2 u (one ulp, so a truncating adder is covered as well as
                 a rounding one) of the running magnitude <= S.
                 fp8: c = FP8_SUM_C + 2 * (K / 128 + 4): the e4m3 MFMA (128 products per instruction) does NOT sum its
                 products to fp32 accuracy.  Measured on MI355X with one K tile (K = 128), largest on the fp32 output
                 of fp8_persist-bias_f32-K128 (9.8 M elements): |err| = 731 u S, i.e. 2^-14.5 of the absolute sum,
                 where a faithful fp32 sum would be charged 2 * (K/128 + log2(128) + 4) = 24 u S.  (The test prints
                 max err / accumulation term: 0.355 of c = 2^11 + 10 = 2058 there.  With c = 24 the same output had
                 err/bound 28.1; with c = 2^10 + 10 = 1034, 0.706.)  Each
                 instruction's sum is charged 2^-13 of its own absolute sum (FP8_SUM_C = 2^11 u: 2.8x the largest
                 measured error); over the K / 128 instructions these add up to 2^-13 S.  At K = 3072 the errors
                 average out and the same outputs stay well inside the bound.
  rounding       bf16 / fp16 output: 1 ulp of the reference (round to nearest is 1/2 ulp of the stored value, which
                 may sit one binade up); fp32 output: F32_ULPS ulps of the reference.
  GELU           gelu(x) = x / (1 + exp2(x p(x))) with v_exp_f32 / v_rcp_f32: e_acc * 1.13 (max |gelu'|) +
                 (GELU_ULPS + |x p(x)|) * u * |gelu(x)| (the exponent's rounding is amplified by |argument|).
  RMS norm       y = x * rsqrt(mean(x^2) + 1e-6) * s: first-order propagation of e_acc through the norm
                 (rel_rms = sum|x| e_acc / sum x^2) + NORM_ULPS * u * |y| for rsqrt and the products.
  RoPE           z = (cos y0 - sin y1, sin y0 + cos y1): |cos| E_y0 + |sin| E_y1 + 4 u (|cos y0| + |sin y1|).
"""
from __future__ import annotations

import ctypes
import functools
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

from conceptattention_amd import _lib as L

U = 2.0 ** -24
F32_ULPS = 4      # fp32 outputs: a few ulps for the final fp32 operations (bias add, fma with the residual)
GELU_ULPS = 8     # ca_gelu_tanh: v_exp_f32 (1 ulp), v_rcp_f32 (1 ulp), 3 mul / fma, the fp32 constants
NORM_ULPS = 8     # v_rsq_f32 (1 ulp), the fma of the mean, two products with rrms and the bf16 scale
GELU_DERIV = 1.13  # max |d gelu_tanh / dx|
K0, K1 = -2.3022082, -0.10294323   # gelu_tanh(x) = x / (1 + exp2(x (K0 + K1 x^2)))
EPS = 1e-6
Q_SCALE = 0.088388347648 * 1.4426950408889634   # softmax_scale * log2(e): the model's q_out_scale

TILE_W = {L.TILE_256x64: 64, L.TILE_256x128: 128, L.TILE_256x192: 192, L.TILE_256x256: 256,
          L.TILE_PP_256x128: 128, L.TILE_PP_256x192: 192, L.TILE_PP_256x256: 256}


FP8_SUM_C = 2.0 ** 11   # the e4m3 MFMA's product sum: charged 2^-13 of its absolute sum (measured 2^-14.5, see above)
# Measured on MI355X, tests/test_gemm_routes_gpu.py, every route and epilogue (the printed max err / bound per output):
#   bf16 operands: 0.50 on every bf16 and fp16 output (the half-ulp rounding: GELU, the RMS norm and RoPE add nothing
#     visible), 0.083 on fp32 outputs, 0.068 on the fp32 q_prerope.  GELU_ULPS and NORM_ULPS stay as derived: no extra
#     ulp was needed.
#   fp8 operands (FP8_SUM_C = 2^11): 0.50 on bf16 outputs, 0.25 on fp16 q / k, 0.355 on fp32 outputs (fp8_persist,
#     K = 128: 731 u S), 0.26 on the fp32 q_prerope.


def acc_c(K: int, fp8: bool) -> float:
    if fp8:
        return FP8_SUM_C + 2.0 * (K / 128 + 4)
    return 2.0 * (K / 32 + math.log2(32) + 4)


# --------------------------------------------------------------------------------------------------- routes
@dataclass(frozen=True)
class Route:
    tile: int
    kernel: int
    persistent: bool
    thin: object          # None: no thin part; "walk": thin tiles in the tile walk; (MF, NW): the thin-row kernel
    rem: int              # M % 256 of the searched shape
    fp8: bool = False


_P, _C, _F = L.GEMM_KERNEL_PP, L.GEMM_KERNEL_CLASSIC, L.GEMM_KERNEL_PP_FP8
ROUTES = {
    "classic_64": Route(L.TILE_256x64, _C, False, None, 77),
    "classic_128": Route(L.TILE_256x128, _C, False, None, 20),
    "classic_192": Route(L.TILE_256x192, _C, False, None, 200),
    "classic_256": Route(L.TILE_256x256, _C, False, None, 131),
    "pp128": Route(L.TILE_PP_256x128, _P, False, None, 200),
    "pp128_persist": Route(L.TILE_PP_256x128, _P, True, None, 150),
    "pp192": Route(L.TILE_PP_256x192, _P, False, None, 140),
    "pp192_persist": Route(L.TILE_PP_256x192, _P, True, "walk", 36),
    "pp256": Route(L.TILE_PP_256x256, _P, False, None, 200),
    "pp256_persist": Route(L.TILE_PP_256x256, _P, True, None, 160),
    "pp256_thin_walk": Route(L.TILE_PP_256x256, _P, False, "walk", 20),
    "thin_2x1": Route(L.TILE_PP_256x256, _P, False, (2, 1), 20),
    "thin_2x4": Route(L.TILE_PP_256x256, _P, False, (2, 4), 9),
    "thin_4x1": Route(L.TILE_PP_256x256, _P, False, (4, 1), 100),
    "thin_4x4": Route(L.TILE_PP_256x256, _P, False, (4, 4), 44),
    "fp8": Route(L.TILE_PP_256x256, _F, False, None, 200, fp8=True),
    "fp8_persist": Route(L.TILE_PP_256x256, _F, True, "walk", 40, fp8=True),
    "fp8_thin_walk": Route(L.TILE_PP_256x256, _F, False, "walk", 20, fp8=True),
}

# epilogue variants: (epilogue, out dtype, options)
EPIS = {
    "bias_bf16": dict(epi=L.EPI_BIAS, f32=False),
    "bias_f32": dict(epi=L.EPI_BIAS, f32=True),
    "gelu": dict(epi=L.EPI_GELU_TANH, f32=False),
    "gate_rows_bf16": dict(epi=L.EPI_GATE_RESIDUAL, f32=False, gates="rows_tile"),
    "gate_rows_f32": dict(epi=L.EPI_GATE_RESIDUAL, f32=True, gates="rows_thin"),
    "gate_items_bf16": dict(epi=L.EPI_GATE_RESIDUAL, f32=False, gates="items_tile"),
    "gate_items_f32": dict(epi=L.EPI_GATE_RESIDUAL, f32=True, gates="items_thin"),
    "split_gelu": dict(epi=L.EPI_SPLIT_GELU, f32=False),
    # fused QK-norm + RoPE: qpre = q_prerope mode (None, 0 bf16, 1 fp32, 2 raw fp32, 3 add), form = double / single
    # (out2 GELU tail) / qonly (N = n_split / 3)
    "qkv_double_qpre_bf16": dict(epi=L.EPI_QKV_NORM_ROPE, f32=False, form="double", qpre=0, qos=Q_SCALE),
    "qkv_single_qpre_f32_f16": dict(epi=L.EPI_QKV_NORM_ROPE, f32=False, form="single", qpre=1, qos=Q_SCALE, f16=True),
    "qkv_double_qpre_raw": dict(epi=L.EPI_QKV_NORM_ROPE, f32=False, form="double", qpre=2, qos=0.0),
    "qkv_qonly_qpre_add": dict(epi=L.EPI_QKV_NORM_ROPE, f32=False, form="qonly", qpre=3, qos=Q_SCALE, f16=True),
}


def compatible(route: str, epi: str) -> bool:
    r, e = ROUTES[route], EPIS[epi]
    if e["epi"] == L.EPI_QKV_NORM_ROPE:
        if r.tile != L.TILE_PP_256x256:
            return False
        if isinstance(r.thin, tuple) and r.thin[1] == 1:
            return False              # the fused norm needs a head's 128 columns in one workgroup: always NW = 4
        if r.fp8 and e["qpre"] == 3:
            return False              # rejected for fp8 (gemm_impl)
    return True


@dataclass(frozen=True)
class Case:
    route: str
    epi: str
    K: int = 128

    @property
    def id(self):
        return f"{self.route}-{self.epi}-K{self.K}"


CASES = [Case(r, e) for r in ROUTES for e in EPIS if compatible(r, e)]
# one long-K case per kernel family (classic, ping-pong, thin-row kernel both widths, fp8)
CASES += [Case("classic_128", "gate_items_bf16", 3072), Case("pp256_persist", "qkv_single_qpre_f32_f16", 3072),
          Case("thin_2x1", "gate_items_f32", 3072), Case("thin_4x4", "qkv_double_qpre_bf16", 3072),
          Case("fp8_thin_walk", "qkv_single_qpre_f32_f16", 3072)]


# --------------------------------------------------------------------------------------------------- planning
_FAKE = 0x100000   # a 16-byte aligned address: the plan checks pointers, it never dereferences them


def _raw_problem(p, M, N, K, epi, n_split=0, f32=False, fp8=False, qpre=None):
    p.A = p.W = p.out = _FAKE
    p.M, p.N, p.K, p.lda, p.ldw, p.ldc, p.epilogue = M, N, K, K, K, N, epi
    p.gate_rows, p.out_f32 = M, int(f32)
    if fp8:
        p.a_scale = p.w_scale = _FAKE
    if epi == L.EPI_GATE_RESIDUAL:
        p.resid = p.gate = _FAKE
        p.ldr = N
    elif epi == L.EPI_SPLIT_GELU:
        p.out2, p.ld2, p.n_split = _FAKE, N, n_split
    elif epi == L.EPI_QKV_NORM_ROPE:
        p.norm_q = p.norm_k = p.rope = _FAKE
        p.n_split = n_split
        if N > n_split:
            p.out2, p.ld2 = _FAKE, N
        if qpre is not None:
            p.q_prerope, p.ldp, p.qpre_f32 = _FAKE, n_split, qpre


def plan_raw(shapes, tile, fp8, n_cu):
    """ca_gemm_plan of problems given as dicts of _raw_problem's arguments (fake pointers: no GPU, no memory)."""
    from conceptattention_amd import ops
    arr = (L.GemmProblem * len(shapes))()
    for i, s in enumerate(shapes):
        _raw_problem(arr[i], fp8=fp8, **s)
    return ops.gemm_plan(arr, tile=tile, n_cu=n_cu, fp8=fp8)


def route_matches(info: dict, r: Route) -> bool:
    if info["tile"] != r.tile or info["kernel"] != r.kernel or bool(info["persistent"]) != r.persistent:
        return False
    if r.kernel == _C:
        return True
    if r.thin is None:
        return info["thin_tiles"] == 0 and info["thin_mf"] == 0
    if r.thin == "walk":
        return info["thin_tiles"] > 0 and info["thin_mf"] == 0
    return (info["thin_tiles"] == 0 and (info["thin_mf"], info["thin_nw"]) == r.thin and info["main_tiles"] > 0)


def n_split_of(epi: str, N: int, bn: int) -> Optional[int]:
    """n_split for an N of this epilogue variant, or None if that N does not fit it."""
    e = EPIS[epi]
    if e["epi"] == L.EPI_SPLIT_GELU:
        return bn * (N // bn // 2) if N >= 2 * bn else None
    if e["epi"] == L.EPI_QKV_NORM_ROPE:
        if e["form"] == "double":
            return N if N % 768 == 0 else None
        if e["form"] == "single":
            ns = 768 * ((N - 256) // 768)
            return ns if ns >= 768 and (N - ns) % 256 == 0 else None
        return 3 * N if N % 256 == 0 else None
    return 0


@functools.lru_cache(maxsize=None)
def find_shape(route: str, epi: str, K: int, n_cu: int):
    """Smallest (M, N, n_split) with M % 256 == route.rem whose plan at n_cu CUs is the route; None if the route
    cannot be reached on such a device."""
    r, e = ROUTES[route], EPIS[epi]
    bn = TILE_W[r.tile]
    # (m >= 1: full row tiles beside the remainder, so the route carries main tiles too)
    cands = sorted(((256 * m + r.rem) * bn * nt, m, nt) for m in range(1, 24) for nt in range(1, 300))
    for _, m, nt in cands:
        M, N = 256 * m + r.rem, bn * nt
        ns = n_split_of(epi, N, bn)
        if ns is None:
            continue
        qpre = e.get("qpre")
        try:
            info = plan_raw([dict(M=M, N=N, K=K, epi=e["epi"], n_split=ns, f32=e["f32"], qpre=qpre)], r.tile, r.fp8,
                            n_cu)
        except ValueError:
            continue
        if route_matches(info, r):
            return M, N, ns
    return None


# --------------------------------------------------------------------------------------------------- inputs
def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rope_table(M: int, seed: int) -> torch.Tensor:
    """[M, 64, 2] (cos, sin) with a distinct angle per row and pair (float32)."""
    g = torch.Generator().manual_seed(seed)
    freq = torch.rand(64, generator=g, dtype=torch.float64) * 0.5 + 0.01
    phase = torch.rand(64, generator=g, dtype=torch.float64) * 6.283
    ang = torch.arange(M, dtype=torch.float64)[:, None] * freq[None] + phase[None]
    return torch.stack((ang.cos(), ang.sin()), -1).float().contiguous()


def gate_layout(kind: str, M: int, rem: int):
    """(gate_rows, gate_stride?, gate_item_rows, gate2_item_rows): 'rows_tile' boundary inside the first row tile,
    'rows_thin' inside the last (thin) part, 'items_*' per-item gates: 4-row items (concept rows) then 37-row items
    (text rows), the boundary inside the first tile ('items_tile') or inside the last part ('items_thin')."""
    last = M - max(rem, 1) // 2 if rem > 1 else M - 1
    if kind == "rows_tile":
        return min(100, M - 1), False, 0, 0
    if kind == "rows_thin":
        return last, False, 0, 0
    if kind == "items_tile":
        return min(20, 4 * ((M - 1) // 4)), True, 4, 37
    return 4 * (last // 4), True, 4, 37


@dataclass
class Inputs:
    """Host (CPU) tensors of one problem: operands, epilogue data and the options."""
    M: int
    N: int
    K: int
    n_split: int
    epi: str
    fp8: bool
    a: torch.Tensor = None        # bf16 [M, K], or e4m3 bytes (uint8)
    w: torch.Tensor = None
    a_scale: torch.Tensor = None
    w_scale: torch.Tensor = None
    bias: torch.Tensor = None
    resid: torch.Tensor = None
    gate: torch.Tensor = None
    gate2: torch.Tensor = None
    gate_rows: int = 0
    gate_stride: int = 0
    gate_item_rows: int = 0
    gate2_item_rows: int = 0
    rope: torch.Tensor = None
    norm_q: torch.Tensor = None
    norm_k: torch.Tensor = None
    qraw: torch.Tensor = None     # qpre_add: the raw projection q_prerope holds on entry (fp32 [M, n_split / 3])
    extra: dict = field(default_factory=dict)


def make_inputs(epi: str, M: int, N: int, K: int, n_split: int, fp8: bool, rem: int, seed: int = 0,
                layout_M: Optional[int] = None) -> Inputs:
    """Row-wise generated: the first M rows of make_inputs(M', layout_M=M) equal make_inputs(M) for M < M' <= M + 256
    (the gate layout is that of layout_M rows), so that a shorter problem is a row prefix of a longer one."""
    layout_M = layout_M or M
    e = EPIS[epi]
    x = Inputs(M, N, K, n_split, epi, fp8)
    rows = lambda seed_, cols, scale=1.0: torch.cat(
        [_randn((1, cols), seed_ * 1000003 + i, scale) for i in range(M)]) if M else torch.zeros(0, cols)
    if fp8:
        x.a = rows(seed + 1, K).clamp(-440, 440).to(torch.float8_e4m3fn).view(torch.uint8)
        x.w = _randn((N, K), seed + 2).clamp(-440, 440).to(torch.float8_e4m3fn).view(torch.uint8)
        x.a_scale = torch.cat([0.01 * (1 + torch.rand(1, generator=torch.Generator().manual_seed(seed * 7 + i)))
                               for i in range(M)]).float()
        x.w_scale = (0.5 + torch.rand(N, generator=torch.Generator().manual_seed(seed + 3))) / math.sqrt(K) * 100
        x.w_scale = x.w_scale.float()
    else:
        x.a = rows(seed + 1, K).bfloat16()
        x.w = _randn((N, K), seed + 2, 1.0 / math.sqrt(K)).bfloat16()
    x.bias = _randn((N,), seed + 4, 0.5).bfloat16()
    if e["epi"] == L.EPI_GATE_RESIDUAL:
        gr, items, r1, r2 = gate_layout(e["gates"], layout_M, rem)
        x.gate_rows = gr
        x.resid = rows(seed + 5, N)
        x.resid = x.resid if e["f32"] else x.resid.bfloat16()
        if items:
            stride = N + 12                  # not a multiple of the tile width: the vectors do not line up with N
            x.gate_stride, x.gate_item_rows, x.gate2_item_rows = stride, r1, r2
            n1, n2 = -(-gr // r1) + 1, -(-(layout_M + 256 - gr) // r2) + 1
            x.gate = _randn((n1 * stride,), seed + 6).float()
            x.gate2 = _randn((n2 * stride,), seed + 7).float()
        else:
            x.gate, x.gate2 = _randn((N,), seed + 6).float(), _randn((N,), seed + 7).float()
    if e["epi"] == L.EPI_QKV_NORM_ROPE:
        x.rope = rope_table(M, seed + 8)
        x.norm_q = (0.5 + torch.rand(128, generator=torch.Generator().manual_seed(seed + 9))).bfloat16()
        x.norm_k = (0.5 + torch.rand(128, generator=torch.Generator().manual_seed(seed + 10))).bfloat16()
        if e["qpre"] == 3:
            x.qraw = rows(seed + 11, n_split // 3, 0.5)
    return x


# --------------------------------------------------------------------------------------------------- reference
def _deq(t: torch.Tensor, fp8: bool) -> torch.Tensor:
    return t.view(torch.float8_e4m3fn).double() if fp8 else t.double()


def gate_rows_of(x: Inputs, dev) -> tuple:
    """Per-row gate vectors [M, N] (fp64) as ca_gate_of picks them."""
    m = torch.arange(x.M, device=dev)
    first = m < x.gate_rows
    g1, g2 = x.gate.to(dev).double(), x.gate2.to(dev).double()
    if x.gate_stride:
        i1 = (m // x.gate_item_rows).clamp(max=g1.numel() // x.gate_stride - 1)
        i2 = ((m - x.gate_rows).clamp(min=0) // x.gate2_item_rows).clamp(max=g2.numel() // x.gate_stride - 1)
        col = torch.arange(x.N, device=dev)
        v1 = g1[i1[:, None] * x.gate_stride + col[None]]
        v2 = g2[i2[:, None] * x.gate_stride + col[None]]
    else:
        v1, v2 = g1[None].expand(x.M, x.N), g2[None].expand(x.M, x.N)
    return torch.where(first[:, None], v1, v2)


def gelu_ref(v: torch.Tensor, e: torch.Tensor):
    """tanh-GELU in fp64 and its pre-rounding bound given the input bound e."""
    y = 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))
    arg = (v * (K0 + K1 * v * v)).abs()
    return y, GELU_DERIV * e + (GELU_ULPS + arg) * U * y.abs()


def select_rows(x: Inputs, idx: torch.Tensor) -> Inputs:
    """The same problem on rows `idx` of x (row data moves with its row; not for per-row gates)."""
    y = Inputs(**{k: getattr(x, k) for k in x.__dataclass_fields__})
    y.M = len(idx)
    for k in ("a", "a_scale", "resid", "rope", "qraw"):
        if getattr(x, k) is not None:
            setattr(y, k, getattr(x, k)[idx].contiguous())
    return y


def reference(x: Inputs, dev="cpu", mutate=None) -> dict:
    """fp64 reference of every output of the problem: name -> (ref, bound before the output rounding, kind),
    kind in {bf16, f16, f32}.  `mutate` (discrimination checks): a dict of deliberate slips to emulate."""
    mutate = mutate or {}
    e = EPIS[x.epi]
    A, W = _deq(x.a.to(dev), x.fp8), _deq(x.w.to(dev), x.fp8)
    acc = A @ W.T
    S = A.abs() @ W.abs().T
    if "drop_k" in mutate:                          # one 32-wide K step of the MFMA loop left out
        k0, kw = mutate["drop_k"], mutate.get("drop_w", 32)
        acc = acc - A[:, k0:k0 + kw] @ W[:, k0:k0 + kw].T
    if x.fp8:
        sa, sw = x.a_scale.to(dev).double(), x.w_scale.to(dev).double()
        if "a_scale_shift" in mutate:               # row m takes the scale of row m + 1
            m = mutate["a_scale_shift"]
            sa = sa.clone()
            sa[m] = sa[m + 1]
        acc = acc * sa[:, None] * sw[None]
        S = S * sa[:, None].abs() * sw[None].abs()
    bias = x.bias.to(dev).double()
    v = acc + bias
    S = S + bias.abs()
    c = acc_c(x.K, x.fp8)
    out = {}
    if e["epi"] == L.EPI_QKV_NORM_ROPE:
        hd = x.n_split // 3
        nq = min(x.N, 2 * hd) // 128                 # q and k heads present in this problem
        if e["qpre"] == 3:
            qraw = x.qraw.to(dev).double()
            v = v.clone()
            v[:, :hd] = v[:, :hd] + qraw
            S = S.clone()
            S[:, :hd] = S[:, :hd] + qraw.abs()
        eacc = c * U * S
        xh = v[:, :nq * 128].reshape(x.M, nq, 128)
        eh = eacc[:, :nq * 128].reshape(x.M, nq, 128)
        ncols = mutate.get("norm_cols", 128)
        ss = (xh[..., :ncols] ** 2).sum(-1, keepdim=True)
        rr = 1.0 / torch.sqrt(ss / ncols + EPS)
        rel = (xh.abs() * eh).sum(-1, keepdim=True) / (xh ** 2).sum(-1, keepdim=True).add(128 * EPS)
        scale = torch.stack([x.norm_q.to(dev).double() if h < hd // 128 else x.norm_k.to(dev).double()
                             for h in range(nq)])[None]
        y = xh * rr * scale
        ey = rr * scale.abs() * (eh + xh.abs() * rel) + NORM_ULPS * U * y.abs()
        rope = x.rope.to(dev).double()[:, None]            # [M, 1, 64, 2]
        cs, sn = rope[..., 0], rope[..., 1]
        y0, y1 = y[..., 0::2], y[..., 1::2]
        if "rope_swap" in mutate:                   # the two elements of pair p exchanged
            p = mutate["rope_swap"]
            y0, y1 = y0.clone(), y1.clone()
            y0[..., p], y1[..., p] = y[..., 2 * p + 1], y[..., 2 * p]
        z = torch.stack((cs * y0 - sn * y1, sn * y0 + cs * y1), -1).reshape(x.M, nq, 128)
        e0, e1 = ey[..., 0::2], ey[..., 1::2]
        ez0 = cs.abs() * e0 + sn.abs() * e1 + 4 * U * ((cs * y0).abs() + (sn * y1).abs())
        ez1 = sn.abs() * e0 + cs.abs() * e1 + 4 * U * ((sn * y0).abs() + (cs * y1).abs())
        ez = torch.stack((ez0, ez1), -1).reshape(x.M, nq, 128)
        qos = e["qos"] if e["qos"] else 1.0
        hs = torch.ones(nq, dtype=torch.float64, device=dev)
        hs[:hd // 128] = qos
        if mutate.get("qos_on_k"):
            hs[hd // 128:] = qos
        z = z * hs[None, :, None]
        ez = ez * hs[None, :, None] + U * z.abs()
        qk_kind = "f16" if e.get("f16") else "bf16"
        out["q"] = (z[:, :hd // 128].reshape(x.M, -1), ez[:, :hd // 128].reshape(x.M, -1), qk_kind)
        if nq > hd // 128:
            out["k"] = (z[:, hd // 128:].reshape(x.M, -1), ez[:, hd // 128:].reshape(x.M, -1), qk_kind)
        if x.N >= x.n_split:
            out["v"] = (v[:, 2 * hd:3 * hd], eacc[:, 2 * hd:3 * hd], "bf16")
        if x.N > x.n_split:
            out["out2"] = (*gelu_ref(v[:, x.n_split:], eacc[:, x.n_split:]), "bf16")
        if e["qpre"] is not None:
            yq = y[:, :hd // 128].reshape(x.M, -1)
            eyq = ey[:, :hd // 128].reshape(x.M, -1)
            if e["qpre"] == 0:
                out["q_prerope"] = (yq, eyq, "bf16")
            elif e["qpre"] == 2:
                out["q_prerope"] = (v[:, :hd], eacc[:, :hd], "f32")
            else:
                out["q_prerope"] = (yq, eyq, "f32")
        return out
    eacc = c * U * S
    kind = "f32" if e["f32"] else "bf16"
    if e["epi"] == L.EPI_BIAS:
        out["out"] = (v, eacc, kind)
    elif e["epi"] == L.EPI_GELU_TANH:
        out["out"] = (*gelu_ref(v, eacc), kind)
    elif e["epi"] == L.EPI_SPLIT_GELU:
        out["out"] = (v[:, :x.n_split], eacc[:, :x.n_split], "bf16")
        out["out2"] = (*gelu_ref(v[:, x.n_split:], eacc[:, x.n_split:]), "bf16")
    else:
        g = gate_rows_of(x, dev)
        if "gate_neighbour" in mutate:              # row m takes the gate vector of the next item
            m = mutate["gate_neighbour"]
            g = g.clone()
            if x.gate_stride:
                first = m < x.gate_rows
                base = x.gate if first else x.gate2
                item = (m if first else m - x.gate_rows) // (x.gate_item_rows if first else x.gate2_item_rows)
                g[m] = base.to(dev).double()[(item + 1) * x.gate_stride:(item + 1) * x.gate_stride + x.N]
        r = x.resid.to(dev).double()
        o = r + g * v
        out["out"] = (o, g.abs() * eacc + F32_ULPS * U * (r.abs() + (g * v).abs()), kind)
    return out


def ulp(ref: torch.Tensor, kind: str) -> torch.Tensor:
    """One ulp of |ref| in the output format (subnormal spacing below the normal range)."""
    mant, lo = {"bf16": (7, -133), "f16": (10, -24), "f32": (23, -149)}[kind]
    _, ex = torch.frexp(ref.abs().clamp(min=2.0 ** -140).float() if kind != "f32" else ref.abs().clamp(min=1e-300))
    return torch.ldexp(torch.ones_like(ref), (ex.to(torch.int64) - 1 - mant).clamp(min=lo).to(ex.dtype)).to(ref.dtype)


def bound(ref: torch.Tensor, pre: torch.Tensor, kind: str) -> torch.Tensor:
    if kind == "f32":
        return pre + F32_ULPS * ulp(ref, "f32")
    return pre + ulp(ref, kind)


def excess(got: torch.Tensor, ref: torch.Tensor, pre: torch.Tensor, kind: str):
    """(max |got - ref| / bound, number of elements NOT within the bound).  An element that is NaN or infinite -- an
    output the kernel never wrote keeps the NaN it was filled with -- counts as over the bound."""
    err = (got.double() - ref).abs()
    b = bound(ref, pre, kind)
    ratio = err / b
    return ratio.max().item() if ratio.numel() else 0.0, int((~(ratio <= 1)).sum().item())


def rounded_like_output(t: torch.Tensor, kind: str) -> torch.Tensor:
    """A reference value rounded as the kernel stores it (the discrimination checks' emulation of a correct kernel)."""
    return t.to({"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[kind]).double()


# ----------------------------------------------------------------------------------- discrimination (CPU)
SLIPS = {
    # name: (epilogue variant, fp8, mutate, output that must expose it)
    "one 32-wide K step dropped": ("bias_bf16", False, {"drop_k": 64}, "out"),
    "one 32-wide K step dropped (fp32 stream)": ("gate_items_f32", False, {"drop_k": 192}, "out"),
    "neighbouring item's gate vector for one row": ("gate_items_bf16", False, {"gate_neighbour": 30}, "out"),
    "one 128-wide fp8 K step dropped": ("gate_rows_f32", True, {"drop_k": 128, "drop_w": 128}, "out"),
    "a_scale of row m + 1": ("bias_bf16", True, {"a_scale_shift": 17}, "out"),
    "a_scale of row m + 1 in the QKV epilogue": ("qkv_double_qpre_bf16", True, {"a_scale_shift": 17}, "v"),
    "two RoPE pair elements swapped": ("qkv_double_qpre_bf16", False, {"rope_swap": 5}, "q"),
    "norm over 64 instead of 128 columns": ("qkv_single_qpre_f32_f16", False, {"norm_cols": 64}, "k"),
    "norm over 64 columns, seen in the fp32 q_prerope": ("qkv_single_qpre_f32_f16", False, {"norm_cols": 64},
                                                          "q_prerope"),
    "rows past the first round of a persistent walk never written": ("bias_bf16", False, {"unwritten_rows": 32},
                                                                      "out"),
    "one output element never written (fp32 stream)": ("bias_f32", False, {"unwritten": (5, 77)}, "out"),
    "one q element never written": ("qkv_single_qpre_f32_f16", True, {"unwritten": (40, 3)}, "q"),
    "q_out_scale applied to k": ("qkv_double_qpre_bf16", False, {"qos_on_k": True}, "k"),
}


def discrimination(name: str):
    """On the CPU: the fp64 reference, rounded as the kernel stores it, passes its bound; the same computation with
    the named slip fails it.  Returns (passes of the faithful emulation, elements over the bound with the slip)."""
    epi, fp8, mutate, which = SLIPS[name]
    M, K = 64, 256
    e = EPIS[epi]
    N = {"double": 768, "single": 1024}.get(e.get("form"), 512)
    ns = n_split_of(epi, N, 256) or 0
    x = make_inputs(epi, M, N, K, ns, fp8, rem=M, seed=11)
    good = reference(x)
    bad = reference(x, mutate=mutate)
    ok = True
    for k, (ref, pre, kind) in good.items():
        _, n_over = excess(rounded_like_output(ref, kind), ref, pre, kind)
        ok &= n_over == 0
    ref, pre, kind = good[which]
    got = rounded_like_output(bad[which][0], kind)
    if "unwritten_rows" in mutate:              # rows the kernel never stored keep the NaN the test filled in
        got = got.clone()
        got[mutate["unwritten_rows"]:] = float("nan")
    if "unwritten" in mutate:
        got = got.clone()
        got[mutate["unwritten"]] = float("nan")
    _, n_bad = excess(got, ref, pre, kind)
    return ok, n_bad
