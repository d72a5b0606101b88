"""Tensor-level wrappers over the C ABI (include/conceptattn.h).

PyTorch is used only for device memory and the stream; every operator below runs a hand-written
gfx950 kernel from libconceptattn.so.  Arguments are validated here for dtype/device and in the
library for shapes/alignment (ValueError on a rejected argument, nothing is launched).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib as L


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk_host(t, dtype, name: str) -> torch.Tensor:
    """_chk without the device: heatmap_render checks everything else first, so that its checks run without one."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")
    return t


def _chk(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA(HIP) tensor")
    return _chk_host(t, dtype, name)


def host_values(values, device, dtype=torch.float32) -> torch.Tensor:
    """A few host numbers (timesteps, guidance) as a device tensor WITHOUT blocking the host: ``torch.tensor(list,
    device=...)`` copies from pageable memory, which waits for everything queued on the stream before it -- in a loop of
    forwards the host then cannot run ahead and the GPU idles while each forward's first launches are enqueued.  A pinned
    staging tensor and a stream-ordered copy keep the queue full (the caching host allocator recycles the staging block
    only after the copy has run)."""
    t = torch.as_tensor(values, dtype=dtype)
    if t.device.type != "cpu":
        return t.to(device)
    return t.reshape(-1).pin_memory().to(device, non_blocking=True).reshape(t.shape)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


INT32_MAX = 2 ** 31 - 1


def _i32(value, name: str) -> int:
    """A stride or size on its way to an ``int32_t`` parameter or struct field of the library.  ctypes keeps the low 32
    bits of a larger integer without a word (2^32 + 256 arrives as 256, which passes every ``ld >= H`` check and makes the
    kernel read and write other rows), so every such value goes through here: ValueError naming the argument when it is
    not in 0 .. 2^31 - 1."""
    v = int(value)
    if not 0 <= v <= INT32_MAX:
        raise ValueError(f"{name} = {v} does not fit the library's int32_t argument (0 .. 2^31 - 1)")
    return v


@dataclass
class Gemm:
    """One problem of a grouped GEMM launch: out = epi(a @ w.T + bias)."""
    a: torch.Tensor                      # [M,K] bf16 (row stride free)
    w: torch.Tensor                      # [N,K] bf16
    bias: Optional[torch.Tensor]         # [N] bf16
    out: torch.Tensor                    # [M,N] bf16 (row stride free)
    epilogue: int = L.EPI_BIAS
    resid: Optional[torch.Tensor] = None  # [M,N] bf16, may be `out`
    gate: Optional[torch.Tensor] = None   # [N] fp32
    gate2: Optional[torch.Tensor] = None  # [N] fp32 for rows >= gate_rows
    gate_rows: Optional[int] = None
    out2: Optional[torch.Tensor] = None   # SPLIT_GELU / QKV_NORM_ROPE second output [M,N-n_split]
    n_split: int = 0
    norm_q: Optional[torch.Tensor] = None  # QKV_NORM_ROPE: bf16 [128] scales, fp32 [M,64,2] rope table,
    norm_k: Optional[torch.Tensor] = None  # optional bf16 [M, heads*128] pre-RoPE q output
    rope: Optional[torch.Tensor] = None
    q_prerope: Optional[torch.Tensor] = None   # bf16 or fp32 [M, heads*128]
    q_out_scale: float = 0.0                   # QKV_NORM_ROPE: rotated q times this before rounding (0 = 1)
    qpre_raw: bool = False                     # fp32 q_prerope receives the projection BEFORE its norm (qpre_finish)
    qpre_add: bool = False                     # fp32 q_prerope HOLDS such a raw projection: added before the norm, then
                                               # overwritten with the normalised vector (qpre_f32 = 3; N = n_split / 3)
    qk_f16: bool = False                       # QKV_NORM_ROPE: rotated q / k stored as fp16 bits (attention(qk_f16=True))
    a_scale: Optional[torch.Tensor] = None  # fp8 mode: a, w are uint8 (e4m3 bytes) with fp32 row scales
    w_scale: Optional[torch.Tensor] = None  # ([M] and [N]); the launch then goes to ca_gemm_fp8
    # (there a NaN byte, 0x7F / 0xFF, in a makes its output row NaN, one in w its column -- its head under QKV_NORM_ROPE;
    # an infinite a_scale[m] leaves row m without a finite element; a result beyond bf16 is stored as +-inf.
    # acc * a_scale is formed before * w_scale and may overflow on its own: include/conceptattn.h, G1 .. G4)
    # batched forward: rows < gate_rows are items of gate_item_rows rows, the others items of gate2_item_rows rows;
    # item i of a range uses gate (gate2) + i * gate_stride floats.  gate_stride = 0: one vector per range.
    gate_stride: int = 0
    gate_item_rows: int = 0
    gate2_item_rows: int = 0


def _gemm_problems(problems: Sequence[Gemm]):
    """The ca_gemm_problem array of a grouped launch and whether its operands are fp8."""
    arr = (L.GemmProblem * len(problems))()
    fp8 = problems[0].a.dtype == torch.uint8
    op_dtype = torch.uint8 if fp8 else torch.bfloat16
    for i, g in enumerate(problems):
        f32o = g.out.dtype == torch.float32  # the fp32 residual stream (BIAS / GATE_RESIDUAL epilogues)
        a, w, out = _chk(g.a, op_dtype, "a"), _chk(g.w, op_dtype, "w"), _chk(g.out, g.out.dtype if f32o else torch.bfloat16, "out")
        if fp8:
            if g.a_scale is None or g.w_scale is None:
                raise ValueError(f"gemm[{i}]: fp8 operands need a_scale and w_scale")
            sa, sw = _chk(g.a_scale, torch.float32, "a_scale"), _chk(g.w_scale, torch.float32, "w_scale")
            if sa.numel() != a.shape[0] or sw.numel() != w.shape[0] or not (sa.is_contiguous() and sw.is_contiguous()):
                raise ValueError(f"gemm[{i}]: a_scale must be contiguous [M], w_scale contiguous [N]")
            arr[i].a_scale, arr[i].w_scale = sa.data_ptr(), sw.data_ptr()
        if a.dim() != 2 or w.dim() != 2 or out.dim() != 2 or a.shape[1] != w.shape[1] or a.shape[0] != out.shape[0]:
            raise ValueError(f"gemm[{i}]: shape mismatch a{tuple(a.shape)} w{tuple(w.shape)} out{tuple(out.shape)}")
        p = arr[i]
        p.A, p.W, p.out = a.data_ptr(), w.data_ptr(), out.data_ptr()
        p.bias = _ptr(None if g.bias is None else _chk(g.bias, torch.bfloat16, "bias"))
        p.M, p.N, p.K = _i32(a.shape[0], "M"), _i32(w.shape[0], "N"), _i32(a.shape[1], "K")
        p.lda, p.ldw, p.ldc = _i32(a.stride(0), "lda"), _i32(w.stride(0), "ldw"), _i32(out.stride(0), "ldc")
        p.epilogue = g.epilogue
        p.out_f32 = int(f32o)
        p.gate_rows = p.M if g.gate_rows is None else _i32(g.gate_rows, "gate_rows")
        if g.epilogue == L.EPI_GATE_RESIDUAL:
            if g.resid is None or g.gate is None:
                raise ValueError(f"gemm[{i}]: GATE_RESIDUAL needs resid and gate")
            p.resid, p.ldr = _chk(g.resid, out.dtype, "resid").data_ptr(), _i32(g.resid.stride(0), "ldr")
            p.gate = _chk(g.gate, torch.float32, "gate").data_ptr()
            p.gate2 = _ptr(None if g.gate2 is None else _chk(g.gate2, torch.float32, "gate2"))
            p.gate_stride, p.gate_item_rows = _i32(g.gate_stride, "gate_stride"), _i32(g.gate_item_rows, "gate_item_rows")
            p.gate2_item_rows = _i32(g.gate2_item_rows, "gate2_item_rows")
        elif g.epilogue == L.EPI_QKV_NORM_ROPE:
            if g.norm_q is None or g.norm_k is None or g.rope is None:
                raise ValueError(f"gemm[{i}]: QKV_NORM_ROPE needs norm_q, norm_k, rope")
            p.norm_q = _chk(g.norm_q, torch.bfloat16, "norm_q").data_ptr()
            p.norm_k = _chk(g.norm_k, torch.bfloat16, "norm_k").data_ptr()
            rope = _chk(g.rope, torch.float32, "rope")
            if tuple(rope.shape) != (p.M, 64, 2) or not rope.is_contiguous():
                raise ValueError(f"gemm[{i}]: rope must be contiguous [M,64,2]")
            p.rope, p.n_split = rope.data_ptr(), _i32(g.n_split, "n_split")
            p.q_out_scale = float(g.q_out_scale)
            p.qk_f16 = int(bool(g.qk_f16))
            if g.q_prerope is not None:
                if g.q_prerope.dtype not in (torch.bfloat16, torch.float32):
                    raise ValueError(f"gemm[{i}]: q_prerope must be bf16 or fp32")
                p.q_prerope = _chk(g.q_prerope, g.q_prerope.dtype, "q_prerope").data_ptr()
                p.ldp = _i32(g.q_prerope.stride(0), "ldp")
                p.qpre_f32 = int(g.q_prerope.dtype == torch.float32)
                if g.qpre_raw or g.qpre_add:
                    if not p.qpre_f32 or (g.qpre_raw and g.qpre_add):
                        raise ValueError(f"gemm[{i}]: qpre_raw / qpre_add (one of them) need an fp32 q_prerope")
                    p.qpre_f32 = 2 if g.qpre_raw else 3
            if g.out2 is not None:
                p.out2, p.ld2 = _chk(g.out2, torch.bfloat16, "out2").data_ptr(), _i32(g.out2.stride(0), "ld2")
        elif g.epilogue == L.EPI_SPLIT_GELU:
            if g.out2 is None:
                raise ValueError(f"gemm[{i}]: SPLIT_GELU needs out2")
            p.out2, p.ld2 = _chk(g.out2, torch.bfloat16, "out2").data_ptr(), _i32(g.out2.stride(0), "ld2")
            p.n_split = _i32(g.n_split, "n_split")
    return arr, fp8


def gemm(problems: Sequence[Gemm], tile: int = L.TILE_AUTO) -> None:
    lib = L.load()
    arr, fp8 = _gemm_problems(problems)
    if fp8:
        if tile not in (L.TILE_AUTO, L.TILE_PP_256x256):
            raise ValueError("gemm: fp8 operands run on the 256x256 ping-pong tile only")
        if _gemm_hook is not None:
            _gemm_hook(arr, L.TILE_PP_256x256,
                       lambda: L.check(lib.ca_gemm_fp8(arr, len(problems), _stream()), "ca_gemm_fp8"))
            return
        L.check(lib.ca_gemm_fp8(arr, len(problems), _stream()), "ca_gemm_fp8")
        return
    if _gemm_hook is not None:
        if tile == L.TILE_AUTO:
            tile = lib.ca_gemm_auto_tile(arr, len(problems))
            if tile <= 0:
                L.check(tile, "ca_gemm_auto_tile")
        _gemm_hook(arr, tile, lambda: L.check(lib.ca_gemm_bf16(arr, len(problems), tile, _stream()), "ca_gemm_bf16"))
        return
    L.check(lib.ca_gemm_bf16(arr, len(problems), tile, _stream()), "ca_gemm_bf16")


def gemm_plan(problems, tile: int = L.TILE_AUTO, n_cu: int = 0, fp8: Optional[bool] = None) -> dict:
    """What ``gemm(problems, tile)`` would launch on a device with ``n_cu`` CUs (0: the current device's), as a dict of
    ca_gemm_plan_info's fields; nothing is launched.  ``problems``: Gemm problems (fp8 from their dtype), or a ctypes
    array of L.GemmProblem together with ``fp8`` (no tensors, no GPU needed when n_cu > 0).  ValueError where the
    launch would reject the arguments."""
    lib = L.load()
    if isinstance(problems, C.Array):
        arr = problems
        if fp8 is None:
            raise ValueError("gemm_plan: a raw problem array needs fp8=True / False")
    else:
        arr, dt_fp8 = _gemm_problems(problems)
        fp8 = dt_fp8 if fp8 is None else fp8
    info = L.GemmPlanInfo()
    L.check(lib.ca_gemm_plan(arr, len(arr), tile, int(bool(fp8)), n_cu, C.byref(info)), "ca_gemm_plan")
    return {name: getattr(info, name) for name, _ in L.GemmPlanInfo._fields_ if not name.startswith("_")}


# Optional instrumentation used by bench.py: hook(problem_array, tile, launch) must call launch().
_gemm_hook = None


def set_gemm_hook(hook) -> None:
    global _gemm_hook
    _gemm_hook = hook


def linear(a, w, bias, out=None, epilogue=L.EPI_BIAS, tile=L.TILE_AUTO, **kw):
    if out is None:
        out = torch.empty(a.shape[0], w.shape[0], device=a.device, dtype=torch.bfloat16)
    gemm([Gemm(a, w, bias, out, epilogue, **kw)], tile)
    return out


@dataclass
class Attn:
    """out = softmax(q k^T * scale) v per head; keys/values = rows of (k0,v0) then rows of (k1,v1).
    q/k/v are 2-D views [rows, num_heads*128] (row stride free), head h at columns h*128.."""
    q: torch.Tensor
    out: torch.Tensor
    k0: torch.Tensor
    v0: torch.Tensor
    k1: Optional[torch.Tensor] = None
    v1: Optional[torch.Tensor] = None
    out_f32: Optional[torch.Tensor] = None  # optional fp32 copy of the output rows
    q1: Optional[torch.Tensor] = None       # second query-row segment (its rows follow q's) and its output rows
    out1: Optional[torch.Tensor] = None
    # per-head partial heat-map logits of the second segment's rows (q_prescaled kernels): hm_con fp32 [C <= 8, heads*128]
    # = the concept rows' attention outputs (complete before this launch), hm_part fp32 [heads, rows of q1, 8]
    hm_con: Optional[torch.Tensor] = None
    hm_part: Optional[torch.Tensor] = None


def attention(problems: Sequence[Attn], num_heads: int, scale: Optional[float] = None,
              q_prescaled: bool = False, qk_f16: bool = False) -> None:
    """``q_prescaled``: the q rows already carry softmax_scale * log2(e) (Gemm.q_out_scale; CA_ATTN_Q_PRESCALED).
    ``qk_f16`` (with q_prescaled): the q and k rows hold IEEE half bits in their bf16-typed tensors (Gemm.qk_f16)."""
    lib = L.load()
    arr = (L.AttnProblem * len(problems))()
    for i, a in enumerate(problems):
        for n in ("q", "out", "k0", "v0"):
            _chk(getattr(a, n), torch.bfloat16, n)
        for n in ("q", "out", "k0", "v0", "k1", "v1", "q1", "out1", "out_f32"):
            t = getattr(a, n)
            if t is not None and (t.dim() != 2 or t.shape[1] != num_heads * 128):
                raise ValueError(f"attention[{i}]: {n} must be 2-D with num_heads*128 = {num_heads * 128} columns, "
                                 f"got {tuple(t.shape)}")
        p = arr[i]
        p.q, p.out, p.k0, p.v0 = a.q.data_ptr(), a.out.data_ptr(), a.k0.data_ptr(), a.v0.data_ptr()
        p.nq, p.n0 = _i32(a.q.shape[0], "nq"), _i32(a.k0.shape[0], "n0")
        p.ldq, p.ldo, p.ldkv = _i32(a.q.stride(0), "ldq"), _i32(a.out.stride(0), "ldo"), _i32(a.k0.stride(0), "ldkv")
        if a.v0.stride(0) != p.ldkv or a.v0.shape[0] != p.n0 or a.out.shape[0] != p.nq:
            raise ValueError(f"attention[{i}]: k0/v0/out row mismatch")
        p.nq0 = p.nq
        if a.q1 is not None and a.q1.shape[0] > 0:
            _chk(a.q1, torch.bfloat16, "q1"), _chk(a.out1, torch.bfloat16, "out1")
            if a.q1.stride(0) != p.ldq or a.out1.stride(0) != p.ldo or a.out1.shape[0] != a.q1.shape[0]:
                raise ValueError(f"attention[{i}]: both query / output segments must share one row stride")
            p.q1, p.out1 = a.q1.data_ptr(), a.out1.data_ptr()
            p.nq = _i32(p.nq0 + a.q1.shape[0], "nq")
        if a.k1 is not None and a.k1.shape[0] > 0:
            _chk(a.k1, torch.bfloat16, "k1"), _chk(a.v1, torch.bfloat16, "v1")
            if a.k1.stride(0) != p.ldkv or a.v1.stride(0) != p.ldkv or a.v1.shape[0] != a.k1.shape[0]:
                raise ValueError(f"attention[{i}]: both key/value segments must share one row stride")
            p.k1, p.v1, p.n1 = a.k1.data_ptr(), a.v1.data_ptr(), _i32(a.k1.shape[0], "n1")
        if a.hm_con is not None or a.hm_part is not None:
            if a.hm_con is None or a.hm_part is None or a.q1 is None:
                raise ValueError(f"attention[{i}]: hm_con, hm_part and a second query segment go together")
            _chk(a.hm_con, torch.float32, "hm_con"), _chk(a.hm_part, torch.float32, "hm_part")
            if a.hm_con.dim() != 2 or a.hm_con.shape[1] != num_heads * 128 or not 1 <= a.hm_con.shape[0] <= 8 or \
                    tuple(a.hm_part.shape) != (num_heads, a.q1.shape[0], 8) or not a.hm_part.is_contiguous():
                raise ValueError(f"attention[{i}]: hm_con must be fp32 [C <= 8, heads*128], hm_part contiguous fp32 "
                                 "[heads, rows of q1, 8]")
            p.hm_con, p.hm_part = a.hm_con.data_ptr(), a.hm_part.data_ptr()
            p.hm_C, p.ldhc = a.hm_con.shape[0], _i32(a.hm_con.stride(0), "ldhc")
        if a.out_f32 is not None:
            _chk(a.out_f32, torch.float32, "out_f32")
            if a.out_f32.shape[0] != p.nq:
                raise ValueError(f"attention[{i}]: out_f32 row mismatch")
            p.out_f32, p.ldo32 = a.out_f32.data_ptr(), _i32(a.out_f32.stride(0), "ldo32")
    if qk_f16 and not q_prescaled:
        raise ValueError("attention: qk_f16 needs q_prescaled (ca_attn_fwd_qk16)")
    if q_prescaled:
        if scale is not None:
            raise ValueError("attention: give either scale or q_prescaled")
        scale = L.ATTN_Q_PRESCALED
    elif scale is None:
        scale = 1.0 / math.sqrt(128.0)
    elif not scale > 0:
        raise ValueError("attention: scale must be > 0")
    num_heads = _i32(num_heads, "num_heads")
    if qk_f16:
        def launch():
            L.check(lib.ca_attn_fwd_qk16(arr, len(problems), num_heads, _stream()), "ca_attn_fwd_qk16")
    else:
        def launch():
            L.check(lib.ca_attn_fwd_bf16(arr, len(problems), num_heads, scale, _stream()), "ca_attn_fwd_bf16")
    if _attn_hook is not None:
        _attn_hook(arr, num_heads, launch)
        return
    launch()


def attention_stats(reset: bool = False) -> dict:
    """Counters of ca_attn4_kernel's rare softmax paths on the current device (blocking copy; diagnostics only)."""
    c = (C.c_ulonglong * 2)()
    L.check(L.load().ca_attn_stats(c, int(reset)), "ca_attn_stats")
    return {"recomputed_workgroups": int(c[0]), "rereference_events": int(c[1])}


# Optional instrumentation used by bench.py: hook(problem_array, num_heads, launch) must call launch().
_attn_hook = None


def set_attn_hook(hook) -> None:
    global _attn_hook
    _attn_hook = hook


def ln_modulate(x, out, segments, eps: float = 1e-6, out_scale=None, out_lo=None) -> None:
    """segments: [(row_end, shift fp32[H], scale fp32[H]), ...] covering all rows of x.
    With ``out`` uint8 and ``out_scale`` fp32 [M] the result is quantised to e4m3 per row (ca_ln_modulate_fp8), under
    the value-range rules of ``quantize_rows_fp8``: a NaN or inf in x gives a row of NaN bytes with scale 1, a NaN in a
    column of a segment's shift or scale a NaN byte in that column of the segment's rows.
    ``out_lo`` (bf16, fp32 input only): second plane bf16(y - float(bf16(y))) (ca_ln_modulate_f32in_split)."""
    lib = L.load()
    fp8 = out.dtype == torch.uint8
    x32 = x.dtype == torch.float32   # fp32 residual stream
    _chk(x, torch.float32 if x32 else torch.bfloat16, "x"), _chk(out, torch.uint8 if fp8 else torch.bfloat16, "out")
    if fp8 and (out_scale is None or out_scale.dtype != torch.float32 or out_scale.numel() != x.shape[0]
                or not out_scale.is_contiguous()):
        raise ValueError("ln_modulate: fp8 output needs a contiguous fp32 out_scale [M]")
    if len(segments) > L.MAX_SEGMENTS:
        raise ValueError("ln_modulate: too many segments")
    arr = (L.ModSegment * len(segments))()
    for i, (row_end, shift, scale) in enumerate(segments):
        arr[i].row_end = _i32(row_end, "row_end")
        arr[i].shift = _chk(shift, torch.float32, "shift").data_ptr()
        arr[i].scale = _chk(scale, torch.float32, "scale").data_ptr()
    if out_lo is not None and not fp8:
        if not x32:
            raise ValueError("ln_modulate: out_lo needs an fp32 input")
        _chk(out_lo, torch.bfloat16, "out_lo")
        if out_lo.shape != out.shape:
            raise ValueError("ln_modulate: out_lo must have out's shape")
        name, extra = "ca_ln_modulate_f32in_split", (out_lo.data_ptr(), _i32(out_lo.stride(0), "ld_lo"))
    elif fp8:
        name, extra = "ca_ln_modulate_f32in_fp8" if x32 else "ca_ln_modulate_fp8", (out_scale.data_ptr(),)
    else:
        name, extra = "ca_ln_modulate_f32in" if x32 else "ca_ln_modulate_bf16", ()
    L.check(getattr(lib, name)(x.data_ptr(), _i32(x.stride(0), "ldx"), out.data_ptr(), _i32(out.stride(0), "ldo"), *extra,
                               _i32(x.shape[0], "M"), _i32(x.shape[1], "H"), arr, len(segments), eps, _stream()), name)


def qpre_finish(x, d, norm_scale, num_heads: int, rope=None, q_out=None, q_out_scale: float = 0.0,
                q_f16: bool = False) -> None:
    """x <- RMSNorm_128(x + d) * norm_scale per (row, head), in place; x, d fp32 [M, heads*128] (d may be None).
    With ``rope`` (fp32 [M,64,2]) and ``q_out`` (bf16-typed [M, heads*128] view, row stride free) the result is also
    rotated, multiplied by ``q_out_scale`` and stored there as the attention's q (IEEE half bits with ``q_f16``)."""
    lib = L.load()
    _chk(x, torch.float32, "x"), _chk(norm_scale, torch.bfloat16, "norm_scale")
    if d is not None:
        _chk(d, torch.float32, "d")
        if d.shape != x.shape:
            raise ValueError("qpre_finish: d must have x's shape")
    if x.dim() != 2 or x.shape[1] != num_heads * 128 or norm_scale.numel() != 128:
        raise ValueError("qpre_finish: x must be [M, heads*128], norm_scale [128]")
    if q_out is None:
        L.check(lib.ca_qpre_finish_f32(x.data_ptr(), _i32(x.stride(0), "ldx"), _ptr(d),
                                       0 if d is None else _i32(d.stride(0), "ldd"), norm_scale.data_ptr(),
                                       _i32(x.shape[0], "M"), _i32(num_heads, "num_heads"), _stream()), "ca_qpre_finish_f32")
        return
    _chk(q_out, torch.bfloat16, "q_out"), _chk(rope, torch.float32, "rope")
    if tuple(q_out.shape) != tuple(x.shape) or tuple(rope.shape) != (x.shape[0], 64, 2) or not rope.is_contiguous():
        raise ValueError("qpre_finish: q_out must have x's shape, rope must be contiguous [M,64,2]")
    L.check(lib.ca_qpre_finish_rope_f32(x.data_ptr(), _i32(x.stride(0), "ldx"), _ptr(d),
                                        0 if d is None else _i32(d.stride(0), "ldd"), norm_scale.data_ptr(),
                                        rope.data_ptr(), q_out.data_ptr(), _i32(q_out.stride(0), "ldq"),
                                        float(q_out_scale), int(bool(q_f16)), _i32(x.shape[0], "M"),
                                        _i32(num_heads, "num_heads"), _stream()),
            "ca_qpre_finish_rope_f32")


def quantize_rows_fp8(x, out=None, out_scale=None):
    """Row-wise absmax quantisation bf16 [M,K] -> (uint8 e4m3 [M,K], fp32 scale [M]).  scale = max|x| / 448 over the
    row's non-NaN elements, never below 2^-126, and 1 for a zero or all-NaN row.  A NaN element (quiet or signalling)
    becomes a NaN byte (0x7F / 0xFF) and changes nothing else in its row; a row with +-inf has scale inf, NaN bytes at
    the infinities and +-0 elsewhere; a finite non-zero row, however small, has finite bytes and a finite normal scale
    (include/conceptattn.h, "e4m3 value range", P1 .. P5; the other e4m3 producers follow the same rules)."""
    lib = L.load()
    _chk(x, torch.bfloat16, "x")
    if x.dim() != 2:
        raise ValueError("quantize_rows_fp8: expected a 2-D tensor")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    if out_scale is None:
        out_scale = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    _chk(out, torch.uint8, "out"), _chk(out_scale, torch.float32, "out_scale")
    if tuple(out.shape) != tuple(x.shape) or out_scale.numel() != x.shape[0] or not out_scale.is_contiguous():
        raise ValueError("quantize_rows_fp8: out must match x, out_scale must be contiguous [M]")
    L.check(lib.ca_quantize_rows_fp8(x.data_ptr(), _i32(x.stride(0), "ldx"), out.data_ptr(), _i32(out.stride(0), "ldo"),
                                     out_scale.data_ptr(), _i32(x.shape[0], "M"), _i32(x.shape[1], "K"), _stream()),
            "ca_quantize_rows_fp8")
    return out, out_scale


def qknorm_rope(qkv, num_heads, segments, rope_cos_sin, q_prerope=None) -> None:
    """In place on the q,k thirds of qkv [M, 3*num_heads*128].
    segments: [(row_end, q_scale bf16[128], k_scale bf16[128])]; rope_cos_sin fp32 [M,64,2]."""
    lib = L.load()
    _chk(qkv, torch.bfloat16, "qkv"), _chk(rope_cos_sin, torch.float32, "rope_cos_sin")
    M = qkv.shape[0]
    if tuple(rope_cos_sin.shape) != (M, 64, 2) or not rope_cos_sin.is_contiguous():
        raise ValueError(f"qknorm_rope: rope table must be contiguous [M,64,2], got {tuple(rope_cos_sin.shape)}")
    arr = (L.NormSegment * len(segments))()
    for i, (row_end, qs, ks) in enumerate(segments):
        arr[i].row_end = _i32(row_end, "row_end")
        arr[i].q_scale = _chk(qs, torch.bfloat16, "q_scale").data_ptr()
        arr[i].k_scale = _chk(ks, torch.bfloat16, "k_scale").data_ptr()
    pp, ldp = (None, 0) if q_prerope is None else (_chk(q_prerope, torch.bfloat16, "q_prerope").data_ptr(),
                                                   _i32(q_prerope.stride(0), "ldp"))
    L.check(lib.ca_qknorm_rope_bf16(qkv.data_ptr(), _i32(qkv.stride(0), "ld"), _i32(M, "M"), _i32(num_heads, "num_heads"),
                                    arr, len(segments),
                                    rope_cos_sin.data_ptr(), pp, ldp, _stream()), "ca_qknorm_rope_bf16")


def gemv(x, w, bias, out, silu_input=False, accumulate=False) -> None:
    """out[v,:] (+)= f(x[v,:]) @ w.T + bias; x fp32 [nv,K] (nv<=8), w bf16 [N,K], out fp32 [nv,N]."""
    lib = L.load()
    _chk(x, torch.float32, "x"), _chk(w, torch.bfloat16, "w"), _chk(out, torch.float32, "out")
    if not w.is_contiguous():
        raise ValueError("gemv: w must be contiguous")
    b = _ptr(None if bias is None else _chk(bias, torch.bfloat16, "bias"))
    L.check(lib.ca_gemv_bf16(x.data_ptr(), _i32(x.shape[0], "nv"), _i32(x.stride(0), "ldx"), w.data_ptr(), b, out.data_ptr(),
                             _i32(out.stride(0), "ldo"), _i32(w.shape[0], "N"), _i32(w.shape[1], "K"), int(silu_input),
                             int(accumulate), _stream()), "ca_gemv_bf16")


def _split(what: str, symbol: str, x, hi, lo) -> None:
    lib = L.load()
    _chk(x, torch.float32, "x"), _chk(hi, torch.bfloat16, "hi"), _chk(lo, torch.bfloat16, "lo")
    if x.dim() != 2 or hi.shape != x.shape or lo.shape != x.shape or hi.stride(0) != lo.stride(0):
        raise ValueError(f"{what}: x, hi, lo must be [rows,K] of one shape (hi / lo of one row stride)")
    L.check(getattr(lib, symbol)(x.data_ptr(), _i32(x.stride(0), "ldx"), hi.data_ptr(), lo.data_ptr(),
                                 _i32(hi.stride(0), "ldo"), _i32(x.shape[0], "rows"), _i32(x.shape[1], "K"), _stream()),
            symbol)


def silu_split(x, hi, lo) -> None:
    """hi + lo = silu(x) to ~16 mantissa bits, as two bf16 planes (x fp32 [rows,K]; hi, lo bf16 [rows,K])."""
    _split("silu_split", "ca_silu_split_bf16", x, hi, lo)


def split_planes(x, hi, lo) -> None:
    """hi = bf16(x), lo = bf16(x - hi): x fp32 [rows,K] as two bf16 planes (~16 mantissa bits)."""
    _split("split_planes", "ca_split_bf16", x, hi, lo)


def modulation_gemm(vecs, w, bias, out, ones) -> bool:
    """out[v,:] = silu(vecs[v,:]) @ w.T + bias for any number of vectors through the thin-row GEMM kernel (ca_gemv
    streams the weights once per 4 vectors): silu(vecs) as two bf16 planes hi + lo.  Up to 32 vectors: ONE weight pass
    over the stacked rows [hi; lo] (64 rows per workgroup), the two planes' products folded by ca_modulation_combine;
    more: two passes, the second plane accumulating into the fp32 output (gate = ones).  Both forms round alike
    ((hi.w + bias) + lo.w), so a vector's result does not depend on the count.  vecs fp32 [nv,K], w bf16 [N,K], bias
    bf16 [N], out fp32 [nv,N], ones fp32 [N].  Returns False (nothing launched) when the shape does not fit that kernel
    (N % 256, K % 64): the caller then uses gemv."""
    nv, K = vecs.shape
    N = w.shape[0]
    if N % 256 or K % 64 or nv < 1 or not w.is_contiguous():
        return False
    if nv > 128:  # the thin-row kernel takes at most 128 rows per problem: 128 vectors per pair of weight passes
        for r0 in range(0, nv, 128):
            modulation_gemm(vecs[r0:r0 + 128], w, bias, out[r0:r0 + 128], ones)
        return True
    lib = L.load()
    planes = torch.empty(2 * nv, K, device=vecs.device, dtype=torch.bfloat16)
    hi, lo = planes[:nv], planes[nv:]
    silu_split(vecs, hi, lo)
    # column chunks of fewer than 2^32 weight bytes (the GEMM's 32-bit operand offsets), multiples of 256 columns
    n_chunks = -(-N * K * 2 // ((1 << 32) - 1))
    step = -(-(N // 256) // n_chunks) * 256
    pair = torch.empty(2 * nv, N, device=vecs.device, dtype=torch.float32) if nv <= 32 else None
    for c0 in range(0, N, step):
        c1 = min(c0 + step, N)
        if pair is not None:
            gemm([Gemm(planes, w[c0:c1], None, pair[:, c0:c1], L.EPI_BIAS)], L.TILE_PP_256x256)
            continue
        o = out[:, c0:c1]
        gemm([Gemm(hi, w[c0:c1], None if bias is None else bias[c0:c1], o, L.EPI_BIAS)], L.TILE_PP_256x256)
        gemm([Gemm(lo, w[c0:c1], None, o, L.EPI_GATE_RESIDUAL, resid=o, gate=ones[c0:c1])], L.TILE_PP_256x256)
    if pair is not None:
        _chk(out, torch.float32, "out")
        L.check(lib.ca_modulation_combine_f32(pair.data_ptr(), _i32(pair.stride(0), "ldp"), _ptr(bias), out.data_ptr(),
                                              _i32(out.stride(0), "ldo"), _i32(nv, "nv"), _i32(N, "N"), _stream()),
                "ca_modulation_combine_f32")
    return True


def heatmap_logits(img_vec, con_vec, logits) -> None:
    """logits[c,p] = <img_vec[p,:], con_vec[c,:]>; img bf16|fp32 [L,dim], con bf16|fp32 [C,dim] -> fp32 [C,L]
    (fp32 image vectors go with fp32 concept vectors)."""
    lib = L.load()
    if img_vec.dtype not in (torch.bfloat16, torch.float32) or con_vec.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("heatmap_logits: img_vec and con_vec must be bf16 or fp32")
    _chk(img_vec, img_vec.dtype, "img_vec")
    _chk(con_vec, con_vec.dtype, "con_vec")
    _chk(logits, torch.float32, "logits")
    Lp, dim, Cc = img_vec.shape[0], img_vec.shape[1], con_vec.shape[0]
    if tuple(logits.shape) != (Cc, Lp) or not logits.is_contiguous() or con_vec.shape[1] != dim:
        raise ValueError("heatmap_logits: shape mismatch")
    L.check(lib.ca_heatmap_logits_bf16(img_vec.data_ptr(), _i32(img_vec.stride(0), "ldi"), con_vec.data_ptr(),
                                       _i32(con_vec.stride(0), "ldc"),
                                       int(con_vec.dtype == torch.float32) | 2 * int(img_vec.dtype == torch.float32),
                                       _i32(Lp, "L"), _i32(Cc, "C"), _i32(dim, "dim"), logits.data_ptr(),
                                       _stream()), "ca_heatmap_logits_bf16")


def heatmap_softmax_accumulate(logits, acc, weight: float, norm: int = L.NORM_SOFTMAX) -> None:
    """acc += weight * norm_over_concepts(logits); norm: L.NORM_SOFTMAX | NORM_SPARSEMAX | NORM_ENTMAX15.  The sparse norms
    with at most 16 concepts, as ever (a ValueError beyond); ``heatmap_norm_accumulate`` takes them up to 32."""
    if norm != L.NORM_SOFTMAX and isinstance(logits, torch.Tensor) and logits.dim() == 2 and \
            logits.shape[0] > L.HEATMAP_SPARSE_MAX_3LAUNCH:
        raise ValueError(f"heatmap_softmax_accumulate: C = {logits.shape[0]}; the sparse norms need C <= "
                         f"{L.HEATMAP_SPARSE_MAX_3LAUNCH} here (heatmap_norm_accumulate: C <= {L.HEATMAP_MAX_CONCEPTS})")
    heatmap_norm_accumulate(logits, acc, weight, norm)


def heatmap_norm_accumulate(logits, acc, weight: float, norm: int = L.NORM_SOFTMAX) -> None:
    """acc += weight * norm_over_concepts(logits), the weighting launch of the three-launch form: the softmax for any number
    of concepts, the sparse norms for up to L.HEATMAP_MAX_CONCEPTS = 32 (ca_heatmap_norm_accumulate)."""
    lib = L.load()
    _chk(logits, torch.float32, "logits"), _chk(acc, torch.float32, "acc")
    if logits.shape != acc.shape or not logits.is_contiguous() or not acc.is_contiguous():
        raise ValueError("heatmap_softmax_accumulate: logits/acc must be contiguous [C,L]")
    if norm == L.NORM_SOFTMAX:
        L.check(lib.ca_heatmap_softmax_accumulate(logits.data_ptr(), _i32(logits.shape[0], "C"),
                                                  _i32(logits.shape[1], "L"), weight,
                                                  acc.data_ptr(), _stream()), "ca_heatmap_softmax_accumulate")
        return
    L.check(lib.ca_heatmap_norm_accumulate(logits.data_ptr(), _i32(logits.shape[0], "C"), _i32(logits.shape[1], "L"),
                                           int(norm), weight,
                                           acc.data_ptr(), _stream()), "ca_heatmap_norm_accumulate")


@dataclass
class Heatmap:
    """One (work item, space) problem of a fused heat-map launch: logits = img_vec @ con_vec.T per patch, then
    acc += weight * norm_c(logits) and / or acc2 += weight2 * norm_c(logits); ``logits`` (optional) receives the raw
    logits.  img_vec bf16|fp32 [L,dim], con_vec bf16|fp32 [C,dim], acc / acc2 / logits fp32 [C,L] contiguous."""
    img_vec: Optional[torch.Tensor]
    con_vec: Optional[torch.Tensor]
    acc: Optional[torch.Tensor] = None
    weight: float = 0.0
    acc2: Optional[torch.Tensor] = None
    weight2: float = 0.0
    logits: Optional[torch.Tensor] = None
    # instead of the two vector sets: fp32 [heads, L, 8] per-head partial logits (Attn.hm_part): logits = their sum over
    # the heads, in head order
    part: Optional[torch.Tensor] = None


def heatmap_fused_fits(C: int, dim: int) -> bool:
    """Does ca_heatmap_fused take this geometry (all C concept vectors of a problem as fp32 in LDS)?"""
    return 1 <= C <= 8 and dim % 8 == 0 and 8 <= dim <= 4096


def _heatmap_launch(FN: str, problems: Sequence[Heatmap], norm: int, parts: bool) -> None:
    """The argument checks and the launch of heatmap_fused / heatmap_many (``parts``: Heatmap.part is accepted)."""
    lib = L.load()
    if not 1 <= len(problems) <= L.HEATMAP_MAX_PROBLEMS:
        raise ValueError(f"{FN}: 1..{L.HEATMAP_MAX_PROBLEMS} problems per launch")
    arr = (L.HeatmapProblem * len(problems))()
    some = next((t for h in problems for t in (h.acc, h.acc2, h.logits) if t is not None), None)
    if some is None:
        raise ValueError(f"{FN}: every problem needs acc, acc2 or logits")
    Cc, Lp = some.shape
    vec = next((h for h in problems if h.part is None), None)
    dim = 8 if vec is None else vec.img_vec.shape[1]
    for i, h in enumerate(problems):
        p = arr[i]
        if h.part is not None:
            if not parts:
                raise ValueError(f"{FN}[{i}]: per-head partial logits (part) have 8 slots: heatmap_fused takes them")
            _chk(h.part, torch.float32, "part")
            if h.part.dim() != 3 or tuple(h.part.shape[1:]) != (Lp, 8) or not h.part.is_contiguous():
                raise ValueError(f"{FN}[{i}]: part must be contiguous fp32 [heads, L, 8]")
            p.img_vec, p.ldi, p.img_f32 = h.part.data_ptr(), _i32(h.part.shape[0], "heads"), 2
        else:
            if h.img_vec.dtype not in (torch.bfloat16, torch.float32) or h.con_vec.dtype not in (torch.bfloat16, torch.float32):
                raise ValueError(f"{FN}[{i}]: img_vec and con_vec must be bf16 or fp32")
            _chk(h.img_vec, h.img_vec.dtype, "img_vec"), _chk(h.con_vec, h.con_vec.dtype, "con_vec")
            if tuple(h.img_vec.shape) != (Lp, dim) or tuple(h.con_vec.shape) != (Cc, dim):
                raise ValueError(f"{FN}[{i}]: all problems of a launch share L, C and dim")
            p.img_vec, p.con_vec = h.img_vec.data_ptr(), h.con_vec.data_ptr()
            p.ldi, p.ldc = _i32(h.img_vec.stride(0), "ldi"), _i32(h.con_vec.stride(0), "ldc")
            p.img_f32, p.con_f32 = int(h.img_vec.dtype == torch.float32), int(h.con_vec.dtype == torch.float32)
        for name in ("acc", "acc2", "logits"):
            t = getattr(h, name)
            if t is not None:
                _chk(t, torch.float32, name)
                if tuple(t.shape) != (Cc, Lp) or not t.is_contiguous():
                    raise ValueError(f"{FN}[{i}]: {name} must be contiguous fp32 [C,L]")
                setattr(p, name, t.data_ptr())
        p.weight, p.weight2 = float(h.weight), float(h.weight2)
    entry = getattr(lib, "ca_" + FN)
    L.check(entry(arr, len(problems), _i32(Lp, "L"), _i32(Cc, "C"), _i32(dim, "dim"), int(norm), _stream()), "ca_" + FN)


def heatmap_fused(problems: Sequence[Heatmap], norm: int = L.NORM_SOFTMAX) -> None:
    """All heat-map updates of one layer in ONE launch (ca_heatmap_fused): bit-identical to heatmap_logits followed by
    heatmap_softmax_accumulate per problem and accumulator."""
    _heatmap_launch("heatmap_fused", problems, norm, parts=True)


def heatmap_many_fits(C: int, dim: int) -> bool:
    """Does ca_heatmap_many take this geometry (the concept vectors through LDS in chunks of at most 8 rows)?"""
    return 1 <= C <= L.HEATMAP_MAX_CONCEPTS and dim % 8 == 0 and 8 <= dim <= 4096


def heatmap_many(problems: Sequence[Heatmap], norm: int = L.NORM_SOFTMAX) -> None:
    """heatmap_fused for up to L.HEATMAP_MAX_CONCEPTS concepts, still ONE launch per layer (ca_heatmap_many): bit-identical
    to heatmap_logits followed by heatmap_norm_accumulate per problem and accumulator, and to heatmap_fused at C <= 8.
    Vector problems only (no Heatmap.part)."""
    _heatmap_launch("heatmap_many", problems, norm, parts=False)


@dataclass
class TokenMaps:
    """One problem of a prompt-token map launch (ca_token_maps): the probability that the joint softmax over the keys
    [k0 | k1] of every query row of ``q`` gives to the first ``n_tok`` rows of ``k0``, averaged over the heads:
    acc += weight * map and / or acc2 += weight2 * map.  q / k0 / k1 bf16 2-D views [rows, num_heads*128] (row stride free,
    k0 and k1 share theirs), acc / acc2 fp32 [n_tok, nq] contiguous, ``lse`` (optional output) fp32 [num_heads, nq]
    contiguous: the natural-log sum of exponentials of every head's row."""
    q: torch.Tensor
    k0: torch.Tensor
    k1: Optional[torch.Tensor] = None
    n_tok: Optional[int] = None             # None: all rows of k0
    acc: Optional[torch.Tensor] = None
    weight: float = 0.0
    acc2: Optional[torch.Tensor] = None
    weight2: float = 0.0
    lse: Optional[torch.Tensor] = None


def _qk_maps_array(FN: str, struct, problems, num_heads: int, optional: str, missing: Optional[str], sizes,
                   one_row_strides: bool):
    """The argument checks of ops.token_maps, ops.query_maps and ops.propagate_maps (no device needed for the shape rules) and their problem
    array of ``struct``.  What differs between the two is data.  ``optional``: the key segment, "k0" or "k1", that may be
    None or empty; the other one is required, and ``missing`` is the text for it being None (None: left to _chk).
    ``sizes(t, nq, n0, n1)``: the op's size rule: the accumulators' shape, the (name, value) struct fields only this op
    has, and its own text when the sizes are refused.  ``one_row_strides``: the row stride of a one-row tensor, which is free in
    torch, is not held against the other segment's and is replaced by one the library takes."""
    width = num_heads * 128
    required = "k1" if optional == "k0" else "k0"
    arr = (struct * len(problems))()
    seen = {}
    for i, t in enumerate(problems):    # (this loop is host time of every launch: the texts are formed only when raised)
        k = {"k0": t.k0, "k1": t.k1}
        if k[required] is None and missing:
            raise ValueError(f"{FN}[{i}]: {missing}")
        _chk(t.q, torch.bfloat16, "q"), _chk(k[required], torch.bfloat16, required)
        if k[optional] is not None and k[optional].shape[0] == 0:
            k[optional] = None
        if k[optional] is not None:
            _chk(k[optional], torch.bfloat16, optional)
        k0, k1 = k["k0"], k["k1"]
        for n, x in (("q", t.q), ("k0", k0), ("k1", k1)):
            if x is not None and (x.dim() != 2 or x.shape[1] != width):
                raise ValueError(f"{FN}[{i}]: {n} must be 2-D with num_heads*128 = {width} columns, got {tuple(x.shape)}")
        nq, n0, n1 = t.q.shape[0], 0 if k0 is None else k0.shape[0], 0 if k1 is None else k1.shape[0]
        # the row strides: of the key segments, those that have one (under one_row_strides a one-row segment has none)
        ldq = _i32(t.q.stride(0), "ldq")
        ld0 = None if k0 is None or (one_row_strides and n0 <= 1) else _i32(k0.stride(0), "ldk")
        ld1 = None if k1 is None or (one_row_strides and n1 <= 1) else _i32(k1.stride(0), "ldk")
        if ld0 is not None and ld1 is not None and ld0 != ld1:
            raise ValueError(f"{FN}[{i}]: both key segments must share one row stride")
        # (neither has one: the library wants at least the width)
        ldk = ld0 if ld0 is not None else ld1 if ld1 is not None else max(_i32(k[required].stride(0), "ldk"), width)
        if one_row_strides and nq == 1:
            ldq = max(ldq, width)
        acc_shape, own_fields, complaint = sizes(t, nq, n0, n1)
        if complaint:
            raise ValueError(f"{FN}[{i}]: {complaint}")
        if t.acc is None and t.acc2 is None:
            raise ValueError(f"{FN}[{i}]: every problem needs acc or acc2")
        p = arr[i]
        for name, shape in (("acc", acc_shape), ("acc2", acc_shape), ("lse", (num_heads, nq))):
            x = getattr(t, name, None)    # (ops.PropagateMaps has no lse)
            if x is None:
                continue
            _chk(x, torch.float32, name)
            if tuple(x.shape) != shape or not x.is_contiguous():
                raise ValueError(f"{FN}[{i}]: {name} must be contiguous fp32 {list(shape)}, got {tuple(x.shape)}")
            if name != "lse":
                if x.data_ptr() in seen:
                    raise ValueError(f"{FN}[{i}]: {name} is also an accumulator of problem {seen[x.data_ptr()]} of this "
                                     "call (their updates would race)")
                seen[x.data_ptr()] = i
            setattr(p, name, x.data_ptr())
        p.q, p.k0, p.k1 = t.q.data_ptr(), _ptr(k0), _ptr(k1)
        p.nq, p.n0, p.n1 = _i32(nq, "nq"), _i32(n0, "n0"), _i32(n1, "n1")
        for name, value in own_fields:
            setattr(p, name, value)
        p.ldq, p.ldk = ldq, ldk
        p.weight, p.weight2 = float(t.weight), float(t.weight2)
    return arr


def _launch_slices(arr, struct, limit: int):
    """(sub-array, its length) of every launch of a problem array: at most ``limit`` problems each, in order."""
    for s in range(0, len(arr), limit):
        n = min(limit, len(arr) - s)
        yield (struct * n).from_buffer(arr, s * C.sizeof(struct)), n


def _maps_workspace_bytes(entry: str, arr, struct, limit: int, num_heads: int) -> int:
    """The largest workspace any launch of ``arr`` needs, as the library's ``entry`` says."""
    query = getattr(L.load(), entry)
    need = 0
    for sub, n in _launch_slices(arr, struct, limit):
        rc = query(sub, n, _i32(num_heads, "num_heads"))
        if rc < 0:
            L.check(int(rc), entry)
        need = max(need, int(rc))
    return need


def _maps_workspace_arg(FN: str, workspace: torch.Tensor):
    """(pointer, bytes) of a caller's workspace tensor."""
    _chk(workspace, torch.uint8, "workspace")
    if not workspace.is_contiguous():
        raise ValueError(f"{FN}: workspace must be contiguous")
    return workspace.data_ptr(), workspace.numel()


def _token_sizes(t: TokenMaps, nq: int, n0: int, n1: int):
    n_tok = n0 if t.n_tok is None else int(t.n_tok)
    bad = nq < 1 or not 1 <= n_tok <= n0 <= L.TOKMAP_MAX_TEXT
    return (n_tok, nq), (("n_tok", n_tok),), bad and (f"need nq >= 1 and 1 <= n_tok <= n0 <= {L.TOKMAP_MAX_TEXT}, got "
                                                      f"nq = {nq}, n_tok = {n_tok}, n0 = {n0}")


def _token_maps_array(problems: Sequence[TokenMaps], num_heads: int):
    """ops.token_maps' argument checks (no device needed for the shape rules) and the problem array."""
    return _qk_maps_array("token_maps", L.TokmapProblem, problems, num_heads, optional="k1", missing=None,
                          sizes=_token_sizes, one_row_strides=False)


def token_maps_workspace_bytes(problems: Sequence[TokenMaps], num_heads: int) -> int:
    """The scratch memory one ops.token_maps call over these problems needs (the largest of its launches)."""
    return _maps_workspace_bytes("ca_token_maps_workspace_bytes", _token_maps_array(problems, num_heads), L.TokmapProblem,
                                 L.TOKMAP_MAX_PROBLEMS, num_heads)


def token_maps(problems: Sequence[TokenMaps], num_heads: int, scale_log2: float = 1.0, qk_f16: bool = False,
               workspace: Optional[torch.Tensor] = None) -> None:
    """Prompt-token attention maps (ca_token_maps), up to L.TOKMAP_MAX_PROBLEMS problems per launch (longer lists are
    split, in order).  ``scale_log2``: 1.0 for q rows that already carry softmax_scale * log2(e) (the model's), otherwise
    softmax_scale * log2(e).  ``qk_f16``: the q and k rows hold IEEE half bits in their bf16-typed tensors (Gemm.qk_f16).
    ``workspace``: a uint8 device tensor of at least token_maps_workspace_bytes() bytes (None when that is 0)."""
    lib = L.load()
    if len(problems) < 1:
        raise ValueError("token_maps: at least one problem")
    if not num_heads >= 1:
        raise ValueError("token_maps: num_heads must be >= 1")
    if not math.isfinite(scale_log2):
        raise ValueError("token_maps: scale_log2 must be finite")
    arr = _token_maps_array(problems, num_heads)
    ws_ptr, ws_bytes = (None, 0) if workspace is None else _maps_workspace_arg("token_maps", workspace)
    flags = L.TOKMAP_QK_F16 if qk_f16 else 0
    for sub, n in _launch_slices(arr, L.TokmapProblem, L.TOKMAP_MAX_PROBLEMS):
        L.check(lib.ca_token_maps(sub, n, _i32(num_heads, "num_heads"), float(scale_log2), flags, ws_ptr, ws_bytes,
                                  _stream()), "ca_token_maps")


@dataclass
class QueryMaps:
    """One problem of a query-row map launch (ca_query_maps): the probability that the softmax of every row of ``q`` over
    the keys [k0 | k1] gives to each row of ``k1``, averaged over the heads: acc += weight * map and / or
    acc2 += weight2 * map.  q / k0 / k1 bf16 2-D views [rows, num_heads*128] (row stride free, k0 and k1 share theirs; k0
    may be None: no leading keys), acc / acc2 fp32 [nq, n1] contiguous, ``lse`` (optional output) fp32 [num_heads, nq]
    contiguous: the natural-log sum of exponentials of every head's row."""
    q: torch.Tensor
    k0: Optional[torch.Tensor] = None
    k1: Optional[torch.Tensor] = None
    acc: Optional[torch.Tensor] = None
    weight: float = 0.0
    acc2: Optional[torch.Tensor] = None
    weight2: float = 0.0
    lse: Optional[torch.Tensor] = None


def _query_sizes(t: QueryMaps, nq: int, n0: int, n1: int):
    bad = not 1 <= nq <= L.QUERYMAP_MAX_QUERIES or n1 < 1 or n0 + n1 > L.QUERYMAP_MAX_ROWS
    return (nq, n1), (), bad and (f"need 1 <= nq <= {L.QUERYMAP_MAX_QUERIES}, n1 >= 1 and n0 + n1 <= "
                                  f"{L.QUERYMAP_MAX_ROWS}, got nq = {nq}, n0 = {n0}, n1 = {n1}")


def _query_maps_array(problems: Sequence[QueryMaps], num_heads: int):
    """ops.query_maps' argument checks (no device needed for the shape rules) and the problem array."""
    return _qk_maps_array("query_maps", L.QuerymapProblem, problems, num_heads, optional="k0",
                          missing="k1, the emitted key rows, is required", sizes=_query_sizes, one_row_strides=True)


def _query_maps_need(arr, num_heads: int) -> int:
    return _maps_workspace_bytes("ca_query_maps_workspace_bytes", arr, L.QuerymapProblem, L.QUERYMAP_MAX_PROBLEMS, num_heads)


def query_maps_workspace_bytes(problems: Sequence[QueryMaps], num_heads: int) -> int:
    """The scratch memory one ops.query_maps call over these problems needs (the largest of its launches): 8 bytes per
    (head, query row)."""
    L.load()
    if len(problems) < 1:
        raise ValueError("query_maps_workspace_bytes: at least one problem")
    return _query_maps_need(_query_maps_array(problems, num_heads), num_heads)


def query_maps(problems: Sequence[QueryMaps], num_heads: int, scale_log2: float = 1.0, qk_f16: bool = False,
               workspace: Optional[torch.Tensor] = None) -> None:
    """Query-row attention maps (ca_query_maps), up to L.QUERYMAP_MAX_PROBLEMS problems per launch pair (longer lists are
    split, in order; the launches of one call share the workspace, which stream order makes safe).  ``scale_log2``: 1.0
    for q rows that already carry softmax_scale * log2(e) (the model's), otherwise softmax_scale * log2(e).  ``qk_f16``:
    the q and k rows hold IEEE half bits in their bf16-typed tensors (Gemm.qk_f16).  ``workspace``: a uint8 device tensor
    of at least query_maps_workspace_bytes() bytes, 16-byte aligned; None: one is allocated from torch's caching allocator
    (not under graph capture: pass one there)."""
    lib = L.load()
    if len(problems) < 1:
        raise ValueError("query_maps: at least one problem")
    if not num_heads >= 1:
        raise ValueError("query_maps: num_heads must be >= 1")
    if not math.isfinite(scale_log2):
        raise ValueError("query_maps: scale_log2 must be finite")
    arr = _query_maps_array(problems, num_heads)
    if workspace is None:
        workspace = torch.empty(_query_maps_need(arr, num_heads), dtype=torch.uint8, device=problems[0].q.device)
    ws_ptr, ws_bytes = _maps_workspace_arg("query_maps", workspace)
    flags = L.QUERYMAP_QK_F16 if qk_f16 else 0
    for sub, n in _launch_slices(arr, L.QuerymapProblem, L.QUERYMAP_MAX_PROBLEMS):
        L.check(lib.ca_query_maps(sub, n, _i32(num_heads, "num_heads"), float(scale_log2), flags, ws_ptr, ws_bytes,
                                  _stream()), "ca_query_maps")


@dataclass
class PropagateMaps:
    """One problem of a map propagation launch (ca_propagate_maps): the rows of ``v`` (fp32 [C, n1], one value per row of
    ``k1``) carried through the attention of the rows of ``q`` over the keys [k0 | k1], averaged over the heads:
    out[c, i] = mean_h sum_j softmax_j(<q_h[i], k_h[j]>)[n0 + j] * v[c, j], then acc += weight * out and / or
    acc2 += weight2 * out.  q / k0 / k1 bf16 2-D views [rows, num_heads*128] (row stride free, k0 and k1 share theirs; k0
    may be None: no leading keys, and the weights of a row then sum to 1), v fp32 [C, n1] (row stride free, at least n1),
    acc / acc2 fp32 [C, nq] contiguous.  v may not overlap an accumulator of any problem of the call."""
    q: torch.Tensor
    k0: Optional[torch.Tensor] = None
    k1: Optional[torch.Tensor] = None
    v: Optional[torch.Tensor] = None
    acc: Optional[torch.Tensor] = None
    weight: float = 0.0
    acc2: Optional[torch.Tensor] = None
    weight2: float = 0.0


def _propagate_sizes(t: PropagateMaps, nq: int, n0: int, n1: int):
    if t.v is None:
        return (0, nq), (), "v, the map rows to propagate, is required"
    _chk(t.v, torch.float32, "v")
    if t.v.dim() != 2 or t.v.shape[1] != n1:
        return (0, nq), (), f"v must be 2-D fp32 [C, n1 = {n1}], got {tuple(t.v.shape)}"
    Cc = t.v.shape[0]
    if not 1 <= Cc <= L.PROPMAP_MAX_CONCEPTS or nq < 1 or n1 < 1 or n0 + n1 > L.PROPMAP_MAX_ROWS:
        return (Cc, nq), (), (f"need 1 <= C <= {L.PROPMAP_MAX_CONCEPTS}, nq >= 1, n1 >= 1 and n0 + n1 <= {L.PROPMAP_MAX_ROWS}, "
                              f"got C = {Cc}, nq = {nq}, n0 = {n0}, n1 = {n1}")
    ldv = _i32(t.v.stride(0), "ldv")
    if Cc == 1:                     # (the row stride of a one-row tensor is free in torch)
        ldv = max(ldv, n1)
    if ldv < n1:
        return (Cc, nq), (), f"v's row stride {ldv} is below n1 = {n1}"
    if t.v.data_ptr() % 4:
        return (Cc, nq), (), "v must be 4-byte aligned"
    return (Cc, nq), (("v", t.v.data_ptr()), ("C", Cc), ("ldv", ldv)), False


def _propagate_maps_array(problems: Sequence[PropagateMaps], num_heads: int):
    """ops.propagate_maps' argument checks (no device needed for the shape rules) and the problem array."""
    arr = _qk_maps_array("propagate_maps", L.PropmapProblem, problems, num_heads, optional="k0",
                         missing="k1, the valued key rows, is required", sizes=_propagate_sizes, one_row_strides=True)
    # the kernel reads v while cells are written: no v may overlap an accumulator of the call
    outs = [(x.data_ptr(), x.data_ptr() + 4 * x.numel(), j, name) for j, t in enumerate(problems)
            for name, x in (("acc", t.acc), ("acc2", t.acc2)) if x is not None]
    for i, (t, p) in enumerate(zip(problems, arr)):
        lo, hi = t.v.data_ptr(), t.v.data_ptr() + 4 * ((p.C - 1) * p.ldv + p.n1)
        for a, b, j, name in outs:
            if lo < b and a < hi:
                raise ValueError(f"propagate_maps[{i}]: v overlaps {name} of problem {j} of this call (the kernel reads v "
                                 "while the cells are written)")
    return arr


def _propagate_maps_need(arr, num_heads: int) -> int:
    return _maps_workspace_bytes("ca_propagate_maps_workspace_bytes", arr, L.PropmapProblem, L.PROPMAP_MAX_PROBLEMS, num_heads)


def propagate_maps_workspace_bytes(problems: Sequence[PropagateMaps], num_heads: int) -> int:
    """The scratch memory one ops.propagate_maps call over these problems needs (the largest of its launches): 4 bytes
    per (head, map row, query row)."""
    L.load()
    if len(problems) < 1:
        raise ValueError("propagate_maps_workspace_bytes: at least one problem")
    return _propagate_maps_need(_propagate_maps_array(problems, num_heads), num_heads)


def propagate_maps(problems: Sequence[PropagateMaps], num_heads: int, scale_log2: float = 1.0, qk_f16: bool = False,
                   workspace: Optional[torch.Tensor] = None) -> None:
    """Map rows propagated through the query rows' attention (ca_propagate_maps), up to L.PROPMAP_MAX_PROBLEMS problems per
    launch pair (longer lists are split, in order; the launches of one call share the workspace, which stream order makes
    safe).  ``scale_log2``: 1.0 for q rows that already carry softmax_scale * log2(e) (the model's), otherwise
    softmax_scale * log2(e).  ``qk_f16``: the q and k rows hold IEEE half bits in their bf16-typed tensors (Gemm.qk_f16).
    ``workspace``: a uint8 device tensor of at least propagate_maps_workspace_bytes() bytes, 16-byte aligned; None: one is
    allocated from torch's caching allocator (not under graph capture: pass one there)."""
    lib = L.load()
    if len(problems) < 1:
        raise ValueError("propagate_maps: at least one problem")
    if not num_heads >= 1:
        raise ValueError("propagate_maps: num_heads must be >= 1")
    if not math.isfinite(scale_log2):
        raise ValueError("propagate_maps: scale_log2 must be finite")
    arr = _propagate_maps_array(problems, num_heads)
    if workspace is None:
        workspace = torch.empty(_propagate_maps_need(arr, num_heads), dtype=torch.uint8, device=problems[0].q.device)
    ws_ptr, ws_bytes = _maps_workspace_arg("propagate_maps", workspace)
    flags = L.PROPMAP_QK_F16 if qk_f16 else 0
    for sub, n in _launch_slices(arr, L.PropmapProblem, L.PROPMAP_MAX_PROBLEMS):
        L.check(lib.ca_propagate_maps(sub, n, _i32(num_heads, "num_heads"), float(scale_log2), flags, ws_ptr, ws_bytes,
                                      _stream()), "ca_propagate_maps")


@dataclass
class HeadMaps:
    """One problem of a per-head concept map launch (ca_head_maps): per head of 128 columns the logits of the C rows of
    ``con`` against the L rows of ``img``, weighted across the concepts per head; then heads += weight_h * w,
    acc += weight * mean_h(w) and / or acc2 += weight2 * mean_h(w).  img / con bf16|fp32 2-D views [rows, num_heads*128]
    (row stride free), heads fp32 [num_heads, C, L] contiguous, acc / acc2 fp32 [C, L] contiguous."""
    img: torch.Tensor
    con: torch.Tensor
    heads: Optional[torch.Tensor] = None
    weight_h: float = 0.0
    acc: Optional[torch.Tensor] = None
    weight: float = 0.0
    acc2: Optional[torch.Tensor] = None
    weight2: float = 0.0


HEADMAP_NORMS = (L.NORM_NONE, L.NORM_SOFTMAX, L.NORM_SPARSEMAX, L.NORM_ENTMAX15)


def _head_maps_array(problems: Sequence[HeadMaps], num_heads: int):
    """ops.head_maps' argument checks (no device needed for the shape rules) and the problem array; returns
    (array, L, C)."""
    FN = "head_maps"
    width = num_heads * 128
    arr = (L.HeadmapProblem * len(problems))()
    seen = {}
    Lp = Cc = None
    for i, t in enumerate(problems):
        p = arr[i]
        for n, x in (("img", t.img), ("con", t.con)):
            if not isinstance(x, torch.Tensor) or x.dtype not in (torch.bfloat16, torch.float32):
                raise ValueError(f"{FN}[{i}]: {n}: expected dtype bf16 or fp32")
            _chk(x, x.dtype, n)
            if x.dim() != 2 or x.shape[1] != width:
                raise ValueError(f"{FN}[{i}]: {n} must be 2-D with num_heads*128 = {width} columns (hidden % 128 == 0), "
                                 f"got {tuple(x.shape)}")
            ld = _i32(x.stride(0), "ldi" if n == "img" else "ldc")
            if x.shape[0] == 1 and ld < width:   # (a one-row tensor's stride is free in torch; the library wants the width)
                ld = width
            if ld < width:
                raise ValueError(f"{FN}[{i}]: {n} row stride {ld} is below the width num_heads*128 = {width}")
            per16 = 8 if x.dtype == torch.bfloat16 else 4
            if x.data_ptr() % 16 or ld % per16:
                raise ValueError(f"{FN}[{i}]: {n} rows must be 16-byte aligned (row stride a multiple of {per16} elements), "
                                 f"got stride {ld}")
            if n == "img":
                p.ldi = ld
            else:
                p.ldc = ld
        if Lp is None:
            Lp, Cc = t.img.shape[0], t.con.shape[0]
        if (t.img.shape[0], t.con.shape[0]) != (Lp, Cc):
            raise ValueError(f"{FN}[{i}]: all problems of a call share L and C")
        if Lp < 1 or not 1 <= Cc <= L.HEATMAP_MAX_CONCEPTS:
            raise ValueError(f"{FN}[{i}]: need L >= 1 and 1 <= C <= {L.HEATMAP_MAX_CONCEPTS}, got L = {Lp}, C = {Cc}")
        if t.heads is None and t.acc is None and t.acc2 is None:
            raise ValueError(f"{FN}[{i}]: every problem needs heads, acc or acc2")
        for name, shape in (("heads", (num_heads, Cc, Lp)), ("acc", (Cc, Lp)), ("acc2", (Cc, Lp))):
            x = getattr(t, name)
            if x is None:
                continue
            _chk(x, torch.float32, name)
            if tuple(x.shape) != shape or not x.is_contiguous():
                raise ValueError(f"{FN}[{i}]: {name} must be contiguous fp32 {list(shape)}, got {tuple(x.shape)}")
            if x.data_ptr() in seen:
                raise ValueError(f"{FN}[{i}]: {name} is also an accumulator of problem {seen[x.data_ptr()]} of this call "
                                 "(their updates would race)")
            seen[x.data_ptr()] = i
            setattr(p, name, x.data_ptr())
        p.img, p.con = t.img.data_ptr(), t.con.data_ptr()
        p.img_f32, p.con_f32 = int(t.img.dtype == torch.float32), int(t.con.dtype == torch.float32)
        p.weight_h, p.weight, p.weight2 = float(t.weight_h), float(t.weight), float(t.weight2)
    return arr, Lp, Cc


def head_maps(problems: Sequence[HeadMaps], num_heads: int, norm: int = L.NORM_NONE) -> None:
    """Per-head concept maps (ca_head_maps), up to L.HEATMAP_MAX_PROBLEMS problems per launch (longer lists are split, in
    order).  ``norm``: L.NORM_NONE (the logits themselves), NORM_SOFTMAX, NORM_SPARSEMAX or NORM_ENTMAX15, across the
    concepts per head and patch."""
    if len(problems) < 1:
        raise ValueError("head_maps: at least one problem")
    if not 1 <= num_heads <= L.HEADMAP_MAX_HEADS:
        raise ValueError(f"head_maps: num_heads must be in 1 .. {L.HEADMAP_MAX_HEADS}")
    if norm not in HEADMAP_NORMS:
        raise ValueError(f"head_maps: norm must be one of L.NORM_NONE / NORM_SOFTMAX / NORM_SPARSEMAX / NORM_ENTMAX15, got {norm}")
    arr, Lp, Cc = _head_maps_array(problems, num_heads)
    lib = L.load()
    for sub, n in _launch_slices(arr, L.HeadmapProblem, L.HEATMAP_MAX_PROBLEMS):
        L.check(lib.ca_head_maps(sub, n, _i32(Lp, "L"), _i32(Cc, "C"), _i32(num_heads, "num_heads"), int(norm), _stream()),
                "ca_head_maps")


def axpy(x, y, a: float) -> None:
    """x += a*y (bf16, fp32 math)."""
    lib = L.load()
    _chk(x, torch.bfloat16, "x"), _chk(y, torch.bfloat16, "y")
    if not (x.is_contiguous() and y.is_contiguous()) or x.numel() != y.numel():
        raise ValueError("axpy: x,y must be contiguous with equal sizes")
    L.check(lib.ca_axpy_bf16(x.data_ptr(), y.data_ptr(), float(a), x.numel(), _stream()), "ca_axpy_bf16")


def axpy_f32(x, y, a: float) -> None:
    """x (fp32) += a*y (bf16 or fp32): the Euler update with the latent kept in fp32 between the steps."""
    lib = L.load()
    _chk(x, torch.float32, "x")
    if y.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("axpy_f32: y must be bf16 or fp32")
    _chk(y, y.dtype, "y")
    if not (x.is_contiguous() and y.is_contiguous()) or x.numel() != y.numel():
        raise ValueError("axpy_f32: x,y must be contiguous with equal sizes")
    L.check(lib.ca_axpy_f32(x.data_ptr(), y.data_ptr(), int(y.dtype == torch.float32), float(a), x.numel(), _stream()),
            "ca_axpy_f32")


def timestep_embedding(t, out, time_factor: float = 1000.0, max_period: float = 10000.0) -> None:
    """out[v,:] = [cos(tf*t[v]*f), sin(tf*t[v]*f)]; t fp32 [nt], out fp32 [nt, dim] contiguous."""
    lib = L.load()
    _chk(t, torch.float32, "t"), _chk(out, torch.float32, "out")
    if out.dim() != 2 or out.shape[0] != t.shape[0] or not out.is_contiguous():
        raise ValueError("timestep_embedding: out must be contiguous [nt, dim]")
    L.check(lib.ca_timestep_embedding_f32(t.data_ptr(), _i32(t.shape[0], "nt"), out.data_ptr(),
                                          _i32(out.shape[1], "dim"), time_factor,
                                          max_period, _stream()), "ca_timestep_embedding_f32")


# ---------------------------------------------------------------------------------------------------------------------
# Autoencoder kernels (ca_vae.hip).  Activations are NHWC tensors whose last dimension is the channel row.

def conv_out_hw(h: int, w: int, ksize: int = 3, stride: int = 1, upsample: bool = False):
    """Output height and width of ``conv2d_nhwc`` (stride 2 = the (0,1,0,1) padding of the reference's Downsample)."""
    if upsample:
        return 2 * h, 2 * w
    if stride == 2:
        return (h - 2) // 2 + 1, (w - 2) // 2 + 1
    return h, w


def pack_conv_weight(w: torch.Tensor, cin_pad: Optional[int] = None) -> torch.Tensor:
    """nn.Conv2d weight [Cout, Cin, k, k] -> the kernel's operand: bf16 [ceil16(Cout), k*k*cin_pad], tap-major and
    K-contiguous (column (ky*k + kx) * cin_pad + c), zeros in the padding rows and columns."""
    cout, cin, k, _ = w.shape
    cin_pad = cin_pad or (cin + 31) // 32 * 32
    out = torch.zeros((cout + 15) // 16 * 16, k * k, cin_pad, dtype=torch.bfloat16, device=w.device)
    out[:cout, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, k * k, cin).to(torch.bfloat16)
    return out.reshape(out.shape[0], k * k * cin_pad)


def conv2d_nhwc(x, w_packed, bias, out, cout: int, ksize: int = 3, stride: int = 1, upsample: bool = False,
                resid=None, cin: Optional[int] = None) -> None:
    """x bf16 [B,H,W,>=cin] -> out fp32 / bf16 [B,Ho,Wo,>=cout]; bias fp32 [cout]; resid fp32 like out (may be out)."""
    _chk(x, torch.bfloat16, "x"), _chk(w_packed, torch.bfloat16, "w")
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("conv2d_nhwc: out must be fp32 or bf16")
    _chk(out, out.dtype, "out")
    B, H, W = x.shape[0], x.shape[1], x.shape[2]
    cin = cin or w_packed.shape[1] // (ksize * ksize)
    if x.dim() != 4 or out.dim() != 4 or not x.is_contiguous() or not out.is_contiguous() or \
            w_packed.shape != ((cout + 15) // 16 * 16, ksize * ksize * cin) or not w_packed.is_contiguous():
        raise ValueError(f"conv2d_nhwc: x{tuple(x.shape)} / out{tuple(out.shape)} must be contiguous NHWC, w "
                         f"{tuple(w_packed.shape)} the packed [ceil16(cout), k*k*cin]")
    if tuple(out.shape[:3]) != (B,) + conv_out_hw(H, W, ksize, stride, upsample):
        raise ValueError(f"conv2d_nhwc: out{tuple(out.shape)} does not match the output size of x{tuple(x.shape)}")
    if bias is not None and (_chk(bias, torch.float32, "bias").numel() != cout or not bias.is_contiguous()):
        raise ValueError("conv2d_nhwc: bias must be contiguous fp32 [cout]")
    if resid is not None and (_chk(resid, torch.float32, "resid").shape != out.shape or not resid.is_contiguous()):
        raise ValueError("conv2d_nhwc: resid must be contiguous fp32 of out's shape")
    L.check(L.load().ca_conv3x3_nhwc(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(resid), out.data_ptr(),
                                     _i32(B, "B"), _i32(H, "H"), _i32(W, "W"), _i32(cin, "cin"), _i32(cout, "cout"),
                                     _i32(x.shape[3], "ldx"), _i32(out.shape[3], "ldo"), _i32(out.shape[3], "ldr"),
                                     _i32(ksize, "ksize"), _i32(stride, "stride"), int(upsample),
                                     int(out.dtype == torch.float32), _stream()), "ca_conv3x3_nhwc")


def groupnorm_chunks(hw: int) -> int:
    return max(1, min(128, hw // 512))


def groupnorm_nhwc(x, gamma, beta, out, swish: bool, eps: float = 1e-6, part=None) -> None:
    """x fp32 / bf16 [B, HW, C] (or [B,H,W,C]) -> out bf16 of the same shape; gamma / beta fp32 [C]; 32 groups."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("groupnorm_nhwc: x must be fp32 or bf16")
    _chk(x, x.dtype, "x"), _chk(out, torch.bfloat16, "out")
    _chk(gamma, torch.float32, "gamma"), _chk(beta, torch.float32, "beta")
    C_ = x.shape[-1]
    if not x.is_contiguous() or not out.is_contiguous() or out.shape != x.shape or gamma.numel() != C_ or beta.numel() != C_:
        raise ValueError("groupnorm_nhwc: x and out must be contiguous and alike, gamma / beta [C]")
    B, hw = x.shape[0], x.numel() // (x.shape[0] * C_)
    n_chunks = groupnorm_chunks(hw)
    if part is None:
        part = torch.empty(B * n_chunks * 96, device=x.device, dtype=torch.float32)
    if _chk(part, torch.float32, "part").numel() < B * n_chunks * 96:
        raise ValueError("groupnorm_nhwc: part needs B * groupnorm_chunks(HW) * 96 floats")
    C_ = _i32(C_, "C")
    L.check(L.load().ca_groupnorm_nhwc(x.data_ptr(), int(x.dtype == torch.float32), C_, gamma.data_ptr(), beta.data_ptr(),
                                       out.data_ptr(), C_, _i32(B, "B"), hw, C_, eps, int(swish), part.data_ptr(), n_chunks,
                                       _stream()), "ca_groupnorm_nhwc")


def softmax_rows(s, p, n: int, scale: float) -> None:
    """s fp32 [rows, >=n] -> p bf16 [rows, >=n]: p[:, :n] = softmax(scale * s[:, :n]), p[:, n:] = 0."""
    _chk(s, torch.float32, "s"), _chk(p, torch.bfloat16, "p")
    if s.dim() != 2 or p.dim() != 2 or s.shape[0] != p.shape[0]:
        raise ValueError("softmax_rows: s and p must be 2-D with the same rows")
    L.check(L.load().ca_softmax_rows_f32(s.data_ptr(), _i32(s.stride(0), "lds"), p.data_ptr(), _i32(p.stride(0), "ldp"),
                                         _i32(s.shape[0], "rows"), _i32(n, "n"), scale,
                                         _stream()), "ca_softmax_rows_f32")


def affine_rows(x, out, a: float = 1.0, b: float = 0.0, logvar=None, noise=None, cols: Optional[int] = None) -> None:
    """out[:, :cols] = a * (x + exp(0.5 logvar) * noise) + b over 2-D row views (fp32 in, fp32 or bf16 out)."""
    _chk(x, torch.float32, "x"), _chk(out, out.dtype, "out")
    if out.dtype not in (torch.float32, torch.bfloat16) or x.dim() != 2 or out.dim() != 2 or x.shape[0] != out.shape[0]:
        raise ValueError("affine_rows: 2-D fp32 x, 2-D fp32 / bf16 out with the same rows")
    cols = cols or x.shape[1]
    for t in (logvar, noise):
        if t is not None and (_chk(t, torch.float32, "logvar/noise").dim() != 2 or t.shape[0] != x.shape[0]):
            raise ValueError("affine_rows: logvar / noise must be 2-D fp32 with x's rows")
    L.check(L.load().ca_affine_rows_f32(x.data_ptr(), _i32(x.stride(0), "ldx"), _ptr(logvar),
                                        0 if logvar is None else _i32(logvar.stride(0), "ldl"), _ptr(noise),
                                        0 if noise is None else _i32(noise.stride(0), "ldn"), out.data_ptr(),
                                        _i32(out.stride(0), "ldo"), int(out.dtype == torch.float32), x.shape[0],
                                        _i32(cols, "cols"), a, b,
                                        _stream()), "ca_affine_rows_f32")


# ---------------------------------------------------------------------------------------------------------------------
# Pixel I/O kernels (ca_pixels.hip): image bytes into the autoencoder's input plane, its output plane to bytes.

def pixels_to_nhwc32(src, dst) -> None:
    """dst[y, x, :3] = bf16(2 * (src[sy, sx] / 255) - 1) at the nearest source pixel of torch's interpolate, dst[y, x, 3:]
    = 0: src uint8 [H0, W0, 3] on the device (row stride free, the pixel's 3 bytes adjacent), dst bf16 [H, W, 32]
    contiguous -- one image slot of the zero-padded input plane."""
    _chk(src, torch.uint8, "src"), _chk(dst, torch.bfloat16, "dst")
    if src.dim() != 3 or src.shape[2] != 3 or src.stride(2) != 1 or src.stride(1) != 3 or dst.dim() != 3 or dst.shape[2] != 32 or \
            not dst.is_contiguous() or src.device != dst.device:
        raise ValueError(f"pixels_to_nhwc32: src{tuple(src.shape)} must be uint8 [H0, W0, 3] with adjacent pixels, dst"
                         f"{tuple(dst.shape)} contiguous bf16 [H, W, 32] on the same device")
    src_stride = int(src.stride(0))   # bytes, an int64_t of the entry point: the only stride that is not an int32_t
    L.check(L.load().ca_pixels_u8_to_nhwc32_bf16(src.data_ptr(), src_stride, dst.data_ptr(), _i32(src.shape[0], "H0"),
                                                 _i32(src.shape[1], "W0"), _i32(dst.shape[0], "H"), _i32(dst.shape[1], "W"),
                                                 _stream()), "ca_pixels_u8_to_nhwc32_bf16")


def nhwc_to_pixels(src, dst) -> None:
    """dst = (127.5 * (src[..., :3].clamp(-1, 1) + 1.0)).byte(): src fp32 [..., ld >= 3] contiguous (NHWC), dst uint8
    [..., 3] contiguous with the same leading dimensions.  A NaN gives 0."""
    _chk(src, torch.float32, "src"), _chk(dst, torch.uint8, "dst")
    if src.dim() < 2 or src.shape[-1] < 3 or dst.shape[-1] != 3 or tuple(src.shape[:-1]) != tuple(dst.shape[:-1]) or \
            not src.is_contiguous() or not dst.is_contiguous() or src.device != dst.device:
        raise ValueError(f"nhwc_to_pixels: src{tuple(src.shape)} must be contiguous fp32 [..., ld >= 3], dst"
                         f"{tuple(dst.shape)} contiguous uint8 [..., 3] of the same pixels on the same device")
    L.check(L.load().ca_nhwc_f32_to_pixels_u8(src.data_ptr(), _i32(src.shape[-1], "ld"), dst.data_ptr(), dst.numel() // 3,
                                              _stream()),
            "ca_nhwc_f32_to_pixels_u8")


# ---------------------------------------------------------------------------------------------------------------------
# Segmentation scoring (ca_seg.hip): heat maps against label images, one workgroup per item.

SEG_RECORD_BYTES = C.sizeof(L.SegRecord)   # 40


def seg_blur_weights(sigma: float = 1.0) -> list:
    """The nine fp32 weights of segmentation.gaussian_blur3 in row-major order, formed as it forms them."""
    k = torch.exp(-0.5 * (torch.tensor([-1.0, 0.0, 1.0]) / sigma) ** 2)
    k = k / k.sum()
    return [float(v) for v in (k[:, None] * k[None, :]).reshape(-1)]


def _seg_blur_array(fn: str, blur_weights):
    """``blur_weights`` of the scoring entry ``fn`` as the nine floats the library takes; None stays None (no blur)."""
    if blur_weights is None:
        return None
    blur_weights = [float(v) for v in blur_weights]
    if len(blur_weights) != 9:
        raise ValueError(f"{fn}: blur_weights are the nine weights of the 3x3 blur")
    return (C.c_float * 9)(*blur_weights)


def _seg_check_sizes(fn: str, maps: str, h: int, w: int, max_cells: int, host_route: str, Hl: int, Wl: int,
                     max_pixels: int) -> None:
    """The cell and label-pixel ranges of the scoring entry ``fn`` (ca_<fn>); ``maps``: its word for what it scores."""
    if not 1 <= h * w <= max_cells:
        raise ValueError(f"{fn}: {maps} of {h} x {w} cells; ca_{fn} takes 1..{max_cells} (larger maps are scored on the "
                         f"host: segmentation.{host_route})")
    if not 1 <= Hl * Wl <= max_pixels:
        raise ValueError(f"{fn}: a label of {Hl} x {Wl} pixels; ca_{fn} takes 1..2^24")


def seg_score(maps, labels, results, mean_value_threshold: bool = True, downscale_for_eval: bool = False,
              blur_weights=None, mask_out=None, coeff_out=None) -> None:
    """Score n heat maps against n label images (ca_seg_score; include/conceptattn.h states the arithmetic).
    maps: n fp32 [h, w] contiguous tensors (a list, or one [n, h, w] tensor), h * w <= 4096; labels: n uint8 [Hl, Wl]
    contiguous tensors, nonzero = positive, Hl * Wl <= 2^24; results: uint8 [n, 40] contiguous, one ca_seg_record per
    item (L.SegRecord); mask_out: optional uint8 [n, h, w], coeff_out: optional fp32 [n, h, w], both at map resolution.
    ``blur_weights``: nine numbers (seg_blur_weights) to blur the map first, None for no blur.  More than
    L.SEG_MAX_PROBLEMS items go in several launches."""
    lib = L.load()
    maps, labels = list(maps), list(labels)
    n = len(maps)
    if n < 1 or len(labels) != n:
        raise ValueError(f"seg_score: {n} maps and {len(labels)} labels; need the same number, at least 1")
    _chk(results, torch.uint8, "results")
    if tuple(results.shape) != (n, SEG_RECORD_BYTES) or not results.is_contiguous():
        raise ValueError(f"seg_score: results{tuple(results.shape)} must be contiguous uint8 [{n}, {SEG_RECORD_BYTES}]")
    h, w = (int(v) for v in maps[0].shape) if maps[0].dim() == 2 else (0, 0)
    Hl, Wl = (int(v) for v in labels[0].shape) if labels[0].dim() == 2 else (0, 0)
    for i in range(n):
        _chk(maps[i], torch.float32, "maps"), _chk(labels[i], torch.uint8, "labels")
        if tuple(maps[i].shape) != (h, w) or not maps[i].is_contiguous() or tuple(labels[i].shape) != (Hl, Wl) or \
                not labels[i].is_contiguous() or maps[i].device != results.device or labels[i].device != results.device:
            raise ValueError(f"seg_score[{i}]: maps are contiguous fp32 [h, w] and labels contiguous uint8 [Hl, Wl], all "
                             "items of one shape and on the device of results")
    for name, t, dt in (("mask_out", mask_out, torch.uint8), ("coeff_out", coeff_out, torch.float32)):
        if t is not None:
            _chk(t, dt, name)
            if tuple(t.shape) != (n, h, w) or not t.is_contiguous() or t.device != results.device:
                raise ValueError(f"seg_score: {name}{tuple(t.shape)} must be contiguous [{n}, {h}, {w}] on the same device")
    _seg_check_sizes("seg_score", "a map", h, w, L.SEG_MAX_CELLS, "SegmentationScores", Hl, Wl, L.SEG_MAX_LABEL_PIXELS)
    flags = (L.SEG_MEAN_THRESHOLD if mean_value_threshold else 0) | (L.SEG_DOWNSCALE if downscale_for_eval else 0)
    bw = _seg_blur_array("seg_score", blur_weights)      # (the library checks h >= 2 and w >= 2 for this entry)
    if bw is not None:
        flags |= L.SEG_BLUR
    for c0 in range(0, n, L.SEG_MAX_PROBLEMS):
        m = min(L.SEG_MAX_PROBLEMS, n - c0)
        arr = (L.SegProblem * m)()
        for k in range(m):
            p, i = arr[k], c0 + k
            p.map, p.label, p.result = maps[i].data_ptr(), labels[i].data_ptr(), results[i].data_ptr()
            p.mask_out = None if mask_out is None else mask_out[i].data_ptr()
            p.coeff_out = None if coeff_out is None else coeff_out[i].data_ptr()
        L.check(lib.ca_seg_score(arr, m, h, w, Hl, Wl, flags, bw, _stream()), "ca_seg_score")


# ---------------------------------------------------------------------------------------------------------------------
# Sweep scoring (ca_segtab.hip): a table of maps of one geometry against one label image, one workgroup per map.

def segtab_cells(h: int, w: int, device) -> torch.Tensor:
    """The workspace of segtab_score for h x w maps: uint32 [4, (h w + 3) & ~3] (torch has no uint32 arithmetic the
    caller needs; int32 holds the same bits).  The entry zeroes it on every call."""
    return torch.empty(4, (h * w + 3) & ~3, dtype=torch.int32, device=device)


def segtab_score(maps, target, label, records, cells=None, mean_value_threshold: bool = True,
                 downscale_for_eval: bool = False, blur_weights=None, normalize: bool = True) -> None:
    """Score the M maps of one concept against ONE label image (ca_segtab_score; include/conceptattn.h states the
    arithmetic).  maps: fp32 [M, C, h, w] contiguous with ``target`` the concept plane that is scored (the other planes
    are never read), or fp32 [M, h, w] contiguous (``target`` 0 or None); h * w <= 4096.  label: uint8 [Hl, Wl]
    contiguous, nonzero = positive, Hl * Wl <= 2^24.  records: uint8 [M, 40] contiguous, one ca_seg_record per map
    (L.SegRecord).  cells: the int32 [4, (h w + 3) & ~3] workspace (segtab_cells), allocated when not given.
    ``blur_weights``: nine numbers (seg_blur_weights) to blur every map first, None for no blur; ``normalize=False``
    scores the raw map values instead of their min-max coefficient.  More than L.SEGTAB_MAX_MAPS maps go in several
    calls."""
    lib = L.load()
    _chk(maps, torch.float32, "maps"), _chk(label, torch.uint8, "label"), _chk(records, torch.uint8, "records")
    if maps.dim() not in (3, 4) or not maps.is_contiguous() or maps.shape[0] < 1:
        raise ValueError(f"segtab_score: maps{tuple(maps.shape)} must be contiguous fp32 [M, C, h, w] or [M, h, w], M >= 1")
    M, Cc = int(maps.shape[0]), (int(maps.shape[1]) if maps.dim() == 4 else 1)
    h, w = int(maps.shape[-2]), int(maps.shape[-1])
    k = 0 if target is None else int(target)
    if not 0 <= k < Cc:
        raise ValueError(f"segtab_score: target = {target} with {Cc} concept planes")
    if label.dim() != 2 or not label.is_contiguous() or label.device != maps.device:
        raise ValueError(f"segtab_score: label{tuple(label.shape)} must be contiguous uint8 [Hl, Wl] on the device of maps")
    Hl, Wl = int(label.shape[0]), int(label.shape[1])
    if tuple(records.shape) != (M, SEG_RECORD_BYTES) or not records.is_contiguous() or records.device != maps.device:
        raise ValueError(f"segtab_score: records{tuple(records.shape)} must be contiguous uint8 [{M}, {SEG_RECORD_BYTES}] on "
                         "the device of maps")
    _seg_check_sizes("segtab_score", "maps", h, w, L.SEG_MAX_CELLS, "SweepScores.update", Hl, Wl,
                     L.SEG_MAX_LABEL_PIXELS)
    hw4 = (h * w + 3) & ~3
    if cells is None:
        cells = segtab_cells(h, w, maps.device)
    _chk(cells, torch.int32, "cells")
    if tuple(cells.shape) != (4, hw4) or not cells.is_contiguous() or cells.device != maps.device or cells.data_ptr() % 16:
        raise ValueError(f"segtab_score: cells{tuple(cells.shape)} must be contiguous int32 [4, {hw4}], 16-byte aligned, on "
                         "the device of maps")
    flags = (L.SEGTAB_MEAN_THRESHOLD if mean_value_threshold else 0) | (L.SEGTAB_DOWNSCALE if downscale_for_eval else 0) | \
        (0 if normalize else L.SEGTAB_RAW)
    bw = _seg_blur_array("segtab_score", blur_weights)
    if bw is not None:
        if h < 2 or w < 2:
            raise ValueError(f"segtab_score: blur_weights with maps of {h} x {w} cells; the blur's reflect padding needs "
                             "h >= 2 and w >= 2")
        flags |= L.SEGTAB_BLUR
    stride = Cc * h * w                      # elements between two scored maps: an int64_t of the entry
    base = maps.data_ptr() + 4 * k * h * w
    for m0 in range(0, M, L.SEGTAB_MAX_MAPS):
        n = min(L.SEGTAB_MAX_MAPS, M - m0)
        L.check(lib.ca_segtab_score(C.cast(base + 4 * m0 * stride, C.POINTER(C.c_float)), stride, _i32(n, "n_maps"),
                                    label.data_ptr(), records[m0:m0 + n].data_ptr(), cells.data_ptr(), _i32(h, "h"),
                                    _i32(w, "w"), _i32(Hl, "Hl"), _i32(Wl, "Wl"), flags, bw, _stream()),
                "ca_segtab_score")


# ---------------------------------------------------------------------------------------------------------------------
# Heat-map pictures (ca_render.hip): fp32 map planes to RGB bytes: range, colour map, upscale, blend.

_LUT_CACHE: dict = {}


def colormap_lut(cmap, device) -> torch.Tensor:
    """The look-up table of ca_heatmap_render on ``device``: uint8 [259, 3], rows 0..255
    ``(cmap(np.arange(256))[:, :3] * 255).astype(uint8)``, then the under, over and bad colours.  ``cmap``: a matplotlib
    name (cached per name and device; matplotlib is imported on the first use of a name), a matplotlib colour map, or
    the table itself as a uint8 [259, 3] array or tensor."""
    import numpy as np
    device = torch.device(device)
    if isinstance(cmap, str):
        key = (cmap, str(device))
        if key not in _LUT_CACHE:
            import matplotlib.pyplot as plt
            _LUT_CACHE[key] = colormap_lut(plt.get_cmap(cmap), device)
        return _LUT_CACHE[key]
    if callable(cmap) and hasattr(cmap, "N"):
        if int(cmap.N) != 256:
            raise ValueError(f"colormap_lut: a colour map of {cmap.N} entries; ca_heatmap_render's table has 256")
        rows = [np.asarray(cmap(np.arange(256)))[:, :3]]
        rows += [np.asarray(cmap(v), dtype=np.float64).reshape(1, 4)[:, :3] for v in (-np.inf, np.inf, np.nan)]
        cmap = (np.concatenate(rows) * 255).astype(np.uint8)
    t = torch.as_tensor(cmap)
    if t.dtype != torch.uint8 or tuple(t.shape) != (L.RENDER_LUT_ROWS, 3):
        raise ValueError(f"colormap_lut: a table must be uint8 [{L.RENDER_LUT_ROWS}, 3], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous().to(device)


def _plane_step(t: torch.Tensor) -> int:
    """Bytes from plane 0 to plane 1 of a view [n, ...] (0 for n = 1), taken from the two addresses: the plane steps of
    ca_render_problem are int64_t fields and may pass 2^31."""
    return int(t[1].data_ptr() - t[0].data_ptr()) if t.shape[0] > 1 else 0


def heatmap_render(groups, lut, size=None, bilinear: bool = False, images=None, alpha: Optional[float] = None,
                   ranges=None, out=None):
    """Colour groups of heat maps into RGB bytes (ca_heatmap_render; include/conceptattn.h states the arithmetic).
    groups: fp32 tensor views [n, h, w], each plane contiguous and the planes equally spaced (a slice ``table[:, k]`` of a
    contiguous [n, C, h, w] table is one); all groups share h, w, h * w <= 16384; the planes of a group share one range.
    lut: ``colormap_lut``.  size: None (h, w), an int or (H, W), each 1..4096; bilinear: torch's align_corners=False
    rule instead of the nearest one.  images: None, or one uint8 [H, W, 3] picture for all groups or one per group (row
    stride free, a pixel's bytes adjacent) that the colours are blended over with weight ``alpha`` in [0, 1].  ranges:
    None (every group's own min / max), or fp32 [2] for all groups or [groups, 2] on the device: {lo, hi} as given.
    out: one uint8 view [n, H, W, 3] per group (planes contiguous, equally spaced, at least 3 H W bytes apart), allocated
    when not given.  Returns (the list of out, fp32 [groups, 2] with the ranges used).  More than L.RENDER_MAX_PROBLEMS
    groups go in several launches."""
    groups = list(groups)
    G = len(groups)
    if G < 1:
        raise ValueError("heatmap_render: no groups")
    _chk_host(lut, torch.uint8, "lut")
    dev = lut.device
    if tuple(lut.shape) != (L.RENDER_LUT_ROWS, 3) or not lut.is_contiguous():
        raise ValueError(f"heatmap_render: lut{tuple(lut.shape)} must be contiguous uint8 [{L.RENDER_LUT_ROWS}, 3]")
    h, w = (int(v) for v in groups[0].shape[1:]) if isinstance(groups[0], torch.Tensor) and groups[0].dim() == 3 else (0, 0)
    for i, g in enumerate(groups):
        _chk_host(g, torch.float32, f"groups[{i}]")
        if g.dim() != 3 or tuple(g.shape[1:]) != (h, w) or g.device != dev:
            raise ValueError(f"heatmap_render: groups[{i}]{tuple(g.shape)} must be fp32 [n, {h}, {w}] on the device of lut")
        n = int(g.shape[0])
        if not 1 <= n <= L.RENDER_MAX_MAPS:
            raise ValueError(f"heatmap_render: groups[{i}] has {n} planes; ca_heatmap_render takes 1..{L.RENDER_MAX_MAPS}")
        if (h > 1 and g.stride(1) != w) or (n > 1 and g.stride(0) < h * w):
            raise ValueError(f"heatmap_render: groups[{i}]: every plane contiguous [h, w], the planes equally spaced and "
                             "at least h * w elements apart")
    if not 1 <= h * w <= L.RENDER_MAX_CELLS:
        raise ValueError(f"heatmap_render: maps of {h} x {w} cells; ca_heatmap_render takes 1..{L.RENDER_MAX_CELLS}")
    if size is None:
        H, W = h, w
    elif isinstance(size, int):
        H, W = size, size
    else:
        H, W = (int(v) for v in size)
    if not (1 <= H <= L.RENDER_MAX_SIDE and 1 <= W <= L.RENDER_MAX_SIDE):
        raise ValueError(f"heatmap_render: pictures of {H} x {W}; ca_heatmap_render takes sides of 1..{L.RENDER_MAX_SIDE}")
    flags = L.RENDER_BILINEAR if bilinear else 0
    if (images is None) != (alpha is None):
        raise ValueError("heatmap_render: images and alpha come together")
    if images is not None:
        alpha = float(alpha)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"heatmap_render: alpha = {alpha} outside 0..1")
        images = [images] * G if isinstance(images, torch.Tensor) else list(images)
        if len(images) != G:
            raise ValueError(f"heatmap_render: {len(images)} images for {G} groups")
        for i, im in enumerate(images):
            _chk_host(im, torch.uint8, f"images[{i}]")
            if tuple(im.shape) != (H, W, 3) or (W > 1 and im.stride(1) != 3) or (H > 1 and im.stride(0) < 3 * W) or \
                    im.device != dev:
                raise ValueError(f"heatmap_render: images[{i}]{tuple(im.shape)} must be uint8 [{H}, {W}, 3] with adjacent "
                                 "pixels on the device of lut")
        flags |= L.RENDER_BLEND
    if ranges is not None:
        _chk_host(ranges, torch.float32, "ranges")
        if tuple(ranges.shape) == (2,):
            ranges = ranges.expand(G, 2)
        if tuple(ranges.shape) != (G, 2) or ranges.device != dev:
            raise ValueError(f"heatmap_render: ranges{tuple(ranges.shape)} must be fp32 [2] or [{G}, 2] on the device of lut")
    if out is not None:
        out = list(out)
        if len(out) != G:
            raise ValueError(f"heatmap_render: {len(out)} out tensors for {G} groups")
        for i, o in enumerate(out):
            _chk_host(o, torch.uint8, f"out[{i}]")
            n = int(groups[i].shape[0])
            if tuple(o.shape) != (n, H, W, 3) or o.device != dev or (W > 1 and o.stride(2) != 3) or \
                    (H > 1 and o.stride(1) != 3 * W) or (n > 1 and o.stride(0) < 3 * H * W):
                raise ValueError(f"heatmap_render: out[{i}]{tuple(o.shape)} must be uint8 [{n}, {H}, {W}, 3], every plane "
                                 "contiguous, the planes equally spaced and at least 3 H W bytes apart, on the device of lut")
    if dev.type != "cuda":
        raise ValueError("heatmap_render: expected CUDA(HIP) tensors")
    if out is None:
        out = [torch.empty(int(g.shape[0]), H, W, 3, dtype=torch.uint8, device=dev) for g in groups]
    lib = L.load()
    used = torch.empty(G, 2, dtype=torch.float32, device=dev)
    for g0 in range(0, G, L.RENDER_MAX_PROBLEMS):
        m = min(L.RENDER_MAX_PROBLEMS, G - g0)
        arr = (L.RenderProblem * m)()
        for k in range(m):
            p, i = arr[k], g0 + k
            p.maps, p.map_stride, p.n_maps = groups[i].data_ptr(), _plane_step(groups[i]) // 4, int(groups[i].shape[0])
            p.range_in = None if ranges is None else ranges[i].data_ptr()
            p.range_out = used[i].data_ptr()
            if images is not None:
                p.image, p.image_stride = images[i].data_ptr(), _plane_step(images[i])
            p.out, p.out_stride = out[i].data_ptr(), _plane_step(out[i])
        L.check(lib.ca_heatmap_render(arr, m, _i32(h, "h"), _i32(w, "w"), _i32(H, "H"), _i32(W, "W"), lut.data_ptr(),
                                      0.0 if alpha is None else alpha, flags, _stream()), "ca_heatmap_render")
    return out, used


# ---------------------------------------------------------------------------------------------------------------------
# Multi-class segmentation scoring (ca_mseg.hip): an item's K maps against a label image of class ids.

def mseg_score(maps, labels, counts, class_of, nclass: int, ignore_index: Optional[int] = None, scale=None,
               blur_weights=None, class_out=None, index_out=None) -> None:
    """Argmax over every item's K maps, the winning concept's class, and its counts against a label image of class ids
    (ca_mseg_score; include/conceptattn.h states the arithmetic).
    maps: n fp32 [K, h, w] contiguous tensors (a list, or one [n, K, h, w] tensor), K <= 32, h * w <= 16384; labels: n
    uint8 [Hl, Wl] contiguous tensors of class ids, Hl * Wl <= 2^24; counts: int32 [n, 2 + 2 nclass] contiguous, per item
    correct, labelled, inter[nclass], union[nclass]; class_of: per item the K class ids of its concepts (host integers,
    each below nclass <= 256); ignore_index: the label value that is skipped, None for none; scale: K host numbers that
    multiply the planes before the argmax, None for none; blur_weights: nine numbers (seg_blur_weights) to blur the
    planes first, None for no blur; class_out / index_out: optional uint8 [n, h, w], the class and the winning concept
    per map cell.  More than L.MSEG_MAX_PROBLEMS items go in several launches."""
    lib = L.load()
    maps, labels = list(maps), list(labels)
    n = len(maps)
    if n < 1 or len(labels) != n:
        raise ValueError(f"mseg_score: {n} maps and {len(labels)} labels; need the same number, at least 1")
    nclass = int(nclass)
    if not 1 <= nclass <= L.MSEG_MAX_CLASSES:
        raise ValueError(f"mseg_score: nclass = {nclass}; ca_mseg_score takes 1..{L.MSEG_MAX_CLASSES}")
    _chk(counts, torch.int32, "counts")
    if tuple(counts.shape) != (n, 2 + 2 * nclass) or not counts.is_contiguous():
        raise ValueError(f"mseg_score: counts{tuple(counts.shape)} must be contiguous int32 [{n}, {2 + 2 * nclass}]")
    K, h, w = (int(v) for v in maps[0].shape) if maps[0].dim() == 3 else (0, 0, 0)
    Hl, Wl = (int(v) for v in labels[0].shape) if labels[0].dim() == 2 else (0, 0)
    for i in range(n):
        _chk(maps[i], torch.float32, "maps"), _chk(labels[i], torch.uint8, "labels")
        if tuple(maps[i].shape) != (K, h, w) or not maps[i].is_contiguous() or tuple(labels[i].shape) != (Hl, Wl) or \
                not labels[i].is_contiguous() or maps[i].device != counts.device or labels[i].device != counts.device:
            raise ValueError(f"mseg_score[{i}]: maps are contiguous fp32 [K, h, w] and labels contiguous uint8 [Hl, Wl], "
                             "all items of one shape and on the device of counts")
    for name, t in (("class_out", class_out), ("index_out", index_out)):
        if t is not None:
            _chk(t, torch.uint8, name)
            if tuple(t.shape) != (n, h, w) or not t.is_contiguous() or t.device != counts.device:
                raise ValueError(f"mseg_score: {name}{tuple(t.shape)} must be contiguous [{n}, {h}, {w}] on the same device")
    if not 1 <= K <= L.MSEG_MAX_CONCEPTS:
        raise ValueError(f"mseg_score: maps of K = {K} concepts; ca_mseg_score takes 1..{L.MSEG_MAX_CONCEPTS}")
    _seg_check_sizes("mseg_score", "maps", h, w, L.MSEG_MAX_CELLS, "MultiClassScores", Hl, Wl, L.MSEG_MAX_LABEL_PIXELS)
    ignore = -1 if ignore_index is None else int(ignore_index)
    if not -1 <= ignore <= 255:
        raise ValueError(f"mseg_score: ignore_index = {ignore_index}; a label value 0..255, or None")
    table = [[int(c) for c in row] for row in class_of]
    if len(table) != n or any(len(row) != K for row in table):
        raise ValueError(f"mseg_score: class_of holds one row of K = {K} class ids per item ({n} items)")
    if any(not 0 <= c < nclass for row in table for c in row):
        raise ValueError(f"mseg_score: every class_of entry must be in 0..{nclass - 1} (nclass = {nclass})")
    sc = None
    if scale is not None:
        scale = [float(v) for v in scale]
        if len(scale) != K:
            raise ValueError(f"mseg_score: scale holds one number per concept (K = {K})")
        sc = (C.c_float * K)(*scale)
    flags, bw = 0, _seg_blur_array("mseg_score", blur_weights)
    if bw is not None:
        if h < 2 or w < 2:
            raise ValueError(f"mseg_score: blur_weights with maps of {h} x {w} cells; the blur's reflect padding needs "
                             "h >= 2 and w >= 2")
        flags |= L.MSEG_BLUR
    for c0 in range(0, n, L.MSEG_MAX_PROBLEMS):
        m = min(L.MSEG_MAX_PROBLEMS, n - c0)
        arr = (L.MsegProblem * m)()
        cof = (C.c_uint8 * (m * K))(*[c for row in table[c0:c0 + m] for c in row])
        for k in range(m):
            p, i = arr[k], c0 + k
            p.maps, p.label, p.counts = maps[i].data_ptr(), labels[i].data_ptr(), counts[i].data_ptr()
            p.class_out = None if class_out is None else class_out[i].data_ptr()
            p.index_out = None if index_out is None else index_out[i].data_ptr()
        L.check(lib.ca_mseg_score(arr, m, K, h, w, Hl, Wl, nclass, ignore, flags, cof, sc, bw, _stream()), "ca_mseg_score")


# ---------------------------------------------------------------------------------------------------------------------
# T5 encoder kernels (ca_t5.hip).  Rows are tokens; q / k / v are 2-D views with free row strides.  The two checks in
# front serve the CLIP wrappers below as well.

def _attn_views(fn: str, q, k, v, out, n_seq: int, num_heads: int) -> int:
    """The four bf16 [n_seq * L, num_heads * 64] views of a text-encoder attention call (row strides free); returns L."""
    for n, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _chk(t, torch.bfloat16, n)
        if t.dim() != 2 or t.shape[1] != num_heads * 64 or t.shape[0] != q.shape[0]:
            raise ValueError(f"{fn}: {n} must be 2-D [n_seq * L, num_heads*64 = {num_heads * 64}], got {tuple(t.shape)}")
    if n_seq < 1 or q.shape[0] % n_seq:
        raise ValueError(f"{fn}: {q.shape[0]} rows are not n_seq = {n_seq} sequences of one length")
    return q.shape[0] // n_seq


def _vocab_ids(fn: str, ids, table, shapes: str, shapes_ok) -> torch.Tensor:
    """The int32 [rows] token ids (host or device) of a gather from ``table`` [vocab, H], on the table's device: their form,
    the caller's shapes, then every id in [0, vocab) -- the kernel cannot check it -- before anything is launched."""
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError(f"{fn}: ids must be a contiguous 1-D int32 tensor")
    if not shapes_ok():
        raise ValueError(f"{fn}: {shapes}")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= table.shape[0]:
        raise ValueError(f"{fn}: ids span [{lo}, {hi}], outside the vocabulary [0, {table.shape[0]})")
    return ids.to(table.device)


def t5_attention(q, k, v, bias, out, n_seq: int, num_heads: int) -> None:
    """out = softmax(q k^T + bias) v per (sequence, head); head dim 64, no 1/sqrt(d) scale, no mask.  q, k, v, out bf16
    [n_seq * L, num_heads * 64] views (row stride free, e.g. column slices of one projection output); bias fp32
    [num_heads, 2 L - 1] contiguous, indexed by key_pos - query_pos + L - 1."""
    Lq = _attn_views("t5_attention", q, k, v, out, n_seq, num_heads)
    if tuple(_chk(bias, torch.float32, "bias").shape) != (num_heads, 2 * Lq - 1) or not bias.is_contiguous():
        raise ValueError(f"t5_attention: bias must be contiguous fp32 [num_heads, 2 L - 1] = [{num_heads}, {2 * Lq - 1}], "
                         f"got {tuple(bias.shape)}")
    L.check(L.load().ca_t5_attn_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                     _i32(q.stride(0), "ldq"), _i32(k.stride(0), "ldk"), _i32(v.stride(0), "ldv"),
                                     _i32(out.stride(0), "ldo"), _i32(n_seq, "n_seq"), _i32(num_heads, "num_heads"),
                                     _i32(Lq, "L"), _stream()), "ca_t5_attn_bf16")


def t5_rmsnorm(x, weight, out, eps: float = 1e-6) -> None:
    """out = bf16(x * rsqrt(mean(x^2) + eps) * weight): x fp32 [rows, H], weight fp32 [H], out bf16 [rows, H]."""
    _chk(x, torch.float32, "x"), _chk(weight, torch.float32, "weight"), _chk(out, torch.bfloat16, "out")
    if x.dim() != 2 or out.shape != x.shape or weight.numel() != x.shape[1] or not weight.is_contiguous():
        raise ValueError("t5_rmsnorm: x and out must be 2-D of one shape, weight contiguous [H]")
    L.check(L.load().ca_t5_rmsnorm_f32in(x.data_ptr(), _i32(x.stride(0), "ldx"), weight.data_ptr(), out.data_ptr(),
                                         _i32(out.stride(0), "ldo"), x.shape[0], _i32(x.shape[1], "H"), eps, _stream()),
            "ca_t5_rmsnorm_f32in")


def gated_mul(g, u, out) -> None:
    """out = bf16(float(g) * float(u)) over 2-D bf16 row views of one shape."""
    _chk(g, torch.bfloat16, "g"), _chk(u, torch.bfloat16, "u"), _chk(out, torch.bfloat16, "out")
    if g.dim() != 2 or u.shape != g.shape or out.shape != g.shape:
        raise ValueError("gated_mul: g, u and out must be 2-D of one shape")
    L.check(L.load().ca_gated_mul_bf16(g.data_ptr(), _i32(g.stride(0), "ldg"), u.data_ptr(), _i32(u.stride(0), "ldu"),
                                       out.data_ptr(), _i32(out.stride(0), "ldo"), g.shape[0], _i32(g.shape[1], "C"),
                                       _stream()), "ca_gated_mul_bf16")


def _chk_fp8_out(what: str, out, out_scale, shape) -> None:
    """The e4m3 plane and the scale vector of an fp8 producer: uint8 of ``shape``, contiguous fp32 [rows]."""
    _chk(out, torch.uint8, "out"), _chk(out_scale, torch.float32, "out_scale")
    if tuple(out.shape) != tuple(shape) or out_scale.dim() != 1 or out_scale.numel() != shape[0] or \
            not out_scale.is_contiguous():
        raise ValueError(f"{what}: out must be uint8 {tuple(shape)}, out_scale contiguous fp32 [{shape[0]}]")


def t5_rmsnorm_fp8(x, weight, out, out_scale, eps: float = 1e-6) -> None:
    """t5_rmsnorm written as an fp8 GEMM operand: with y = x * rsqrt(mean(x^2) + eps) * weight in fp32 (never rounded to
    bf16), out_scale[r] = max|y[r]| / 448 (1 for a zero row) and out[r] = e4m3(y[r] / out_scale[r]).  x fp32 [rows, H],
    weight fp32 [H], out uint8 [rows, H] (row stride free), out_scale fp32 [rows] contiguous.  Value range as for
    ``quantize_rows_fp8``: a NaN in x gives a row of NaN bytes with scale 1, an inf in x one NaN byte (inf * 0) in a
    row of zeros; the scale of a vanishing row stops at 2^-126."""
    _chk(x, torch.float32, "x"), _chk(weight, torch.float32, "weight")
    if x.dim() != 2 or weight.numel() != x.shape[1] or not weight.is_contiguous():
        raise ValueError("t5_rmsnorm_fp8: x must be 2-D, weight contiguous [H]")
    _chk_fp8_out("t5_rmsnorm_fp8", out, out_scale, x.shape)
    L.check(L.load().ca_t5_rmsnorm_f32in_fp8(x.data_ptr(), _i32(x.stride(0), "ldx"), weight.data_ptr(), out.data_ptr(),
                                             _i32(out.stride(0), "ldo"), out_scale.data_ptr(), x.shape[0],
                                             _i32(x.shape[1], "H"), eps, _stream()),
            "ca_t5_rmsnorm_f32in_fp8")


def gated_mul_fp8(g, u, out, out_scale) -> None:
    """gated_mul written as an fp8 GEMM operand: y = float(g) * float(u) (exact), out_scale[r] = max|y[r]| / 448 (1 for
    a zero row), out[r] = e4m3(y[r] / out_scale[r]).  g, u bf16 [rows, C] row views, out uint8 [rows, C] (row stride
    free), out_scale fp32 [rows] contiguous.  Value range as for ``quantize_rows_fp8``: a NaN product is a NaN byte, an
    infinite product (an infinite factor, or an overflow of fp32) an infinite scale, a product that underflows to 0 a
    zero."""
    _chk(g, torch.bfloat16, "g"), _chk(u, torch.bfloat16, "u")
    if g.dim() != 2 or u.shape != g.shape:
        raise ValueError("gated_mul_fp8: g and u must be 2-D of one shape")
    _chk_fp8_out("gated_mul_fp8", out, out_scale, g.shape)
    L.check(L.load().ca_gated_mul_fp8(g.data_ptr(), _i32(g.stride(0), "ldg"), u.data_ptr(), _i32(u.stride(0), "ldu"),
                                      out.data_ptr(), _i32(out.stride(0), "ldo"), out_scale.data_ptr(), g.shape[0],
                                      _i32(g.shape[1], "C"), _stream()), "ca_gated_mul_fp8")


def embed_rows(table, ids, out) -> None:
    """out[r, :] = float(table[ids[r], :]): table bf16 [vocab, H], ids int32 [rows] (host or device), out fp32 [rows, H].
    An id outside [0, vocab) is a ValueError here, before anything is launched (the kernel cannot check it)."""
    _chk(table, torch.bfloat16, "table"), _chk(out, torch.float32, "out")
    ids = _vocab_ids("embed_rows", ids, table, "table [vocab, H], ids [rows >= 1], out [rows, H]", lambda: table.dim() == 2 and
                     out.dim() == 2 and ids.numel() >= 1 and out.shape[0] == ids.shape[0] and out.shape[1] == table.shape[1])
    L.check(L.load().ca_embed_rows_f32(table.data_ptr(), _i32(table.stride(0), "ldt"), ids.data_ptr(), out.data_ptr(),
                                       _i32(out.stride(0), "ldo"), ids.shape[0], _i32(table.shape[1], "H"), _stream()),
            "ca_embed_rows_f32")


# ---------------------------------------------------------------------------------------------------------------------
# CLIP text encoder kernels (ca_clip.hip).  Rows are tokens; q / k / v are 2-D views with free row strides.

def clip_attention(q, k, v, out, n_seq: int, num_heads: int, scale: float = 0.125) -> None:
    """out = softmax(scale q k^T + causal mask) v per (sequence, head); head dim 64.  q, k, v, out bf16
    [n_seq * L, num_heads * 64] views (row stride free), L = rows / n_seq any value in 1..128; a query at position i
    sees keys 0..i of its own sequence."""
    Lq = _attn_views("clip_attention", q, k, v, out, n_seq, num_heads)
    L.check(L.load().ca_clip_attn_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _i32(q.stride(0), "ldq"),
                                       _i32(k.stride(0), "ldk"), _i32(v.stride(0), "ldv"), _i32(out.stride(0), "ldo"),
                                       _i32(n_seq, "n_seq"), _i32(num_heads, "num_heads"), _i32(Lq, "L"),
                                       float(scale), _stream()), "ca_clip_attn_bf16")


def layernorm(x, weight, bias, out, eps: float = 1e-5, row_idx=None) -> None:
    """out[r] = bf16((x[src] - mean) * rsqrt(var + eps) * weight + bias), src = row_idx[r] or r: x fp32 [n, H], weight and
    bias fp32 [H], out bf16 [rows, H]; ``row_idx`` an int32 tensor [rows] (host or device) of rows of x, checked here."""
    _chk(x, torch.float32, "x"), _chk(weight, torch.float32, "weight"), _chk(bias, torch.float32, "bias")
    _chk(out, torch.bfloat16, "out")
    if x.dim() != 2 or out.dim() != 2 or out.shape[1] != x.shape[1] or weight.numel() != x.shape[1] or \
            bias.numel() != x.shape[1] or not weight.is_contiguous() or not bias.is_contiguous():
        raise ValueError("layernorm: x [n, H], out [rows, H], weight and bias contiguous [H]")
    idx = None
    if row_idx is None:
        if out.shape[0] != x.shape[0]:
            raise ValueError("layernorm: without row_idx, out has as many rows as x")
    else:
        if not isinstance(row_idx, torch.Tensor) or row_idx.dtype != torch.int32 or row_idx.dim() != 1 or \
                not row_idx.is_contiguous() or row_idx.shape[0] != out.shape[0] or row_idx.numel() < 1:
            raise ValueError("layernorm: row_idx must be a contiguous int32 tensor with one entry per row of out")
        lo, hi = int(row_idx.min()), int(row_idx.max())
        if lo < 0 or hi >= x.shape[0]:
            raise ValueError(f"layernorm: row_idx spans [{lo}, {hi}], outside the rows of x [0, {x.shape[0]})")
        idx = row_idx.to(x.device)
    L.check(L.load().ca_layernorm_f32in(x.data_ptr(), _i32(x.stride(0), "ldx"), _ptr(idx), weight.data_ptr(),
                                        bias.data_ptr(), out.data_ptr(), _i32(out.stride(0), "ldo"), out.shape[0],
                                        _i32(x.shape[1], "H"), eps, _stream()),
            "ca_layernorm_f32in")


def quick_gelu(x, out) -> None:
    """out = bf16(x * sigmoid(1.702 x)) over 2-D bf16 row views of one shape; out may be x."""
    _chk(x, torch.bfloat16, "x"), _chk(out, torch.bfloat16, "out")
    if x.dim() != 2 or out.shape != x.shape:
        raise ValueError("quick_gelu: x and out must be 2-D of one shape")
    L.check(L.load().ca_quick_gelu_bf16(x.data_ptr(), _i32(x.stride(0), "ldx"), out.data_ptr(), _i32(out.stride(0), "ldo"),
                                        x.shape[0], _i32(x.shape[1], "C"), _stream()), "ca_quick_gelu_bf16")


def clip_embed(tok, pos, ids, out, length: int) -> None:
    """out[r, :] = float(tok[ids[r], :]) + float(pos[r % length, :]): tok bf16 [vocab, H], pos bf16 [>= length, H], ids
    int32 [rows] (host or device), out fp32 [rows, H].  An id outside [0, vocab) is a ValueError here, before anything is
    launched (the kernel cannot check it)."""
    _chk(tok, torch.bfloat16, "tok"), _chk(pos, torch.bfloat16, "pos"), _chk(out, torch.float32, "out")
    ids = _vocab_ids("clip_embed", ids, tok, "tok [vocab, H], pos [>= length, H], ids [rows >= 1], out [rows, H]",
                     lambda: tok.dim() == 2 and pos.dim() == 2 and out.dim() == 2 and ids.numel() >= 1 and out.shape[0] == ids.shape[0]
                     and out.shape[1] == tok.shape[1] and pos.shape[1] == tok.shape[1] and 1 <= length <= pos.shape[0])
    L.check(L.load().ca_clip_embed_f32(tok.data_ptr(), _i32(tok.stride(0), "ldt"), pos.data_ptr(),
                                       _i32(pos.stride(0), "ldp"), ids.data_ptr(), out.data_ptr(),
                                       _i32(out.stride(0), "ldo"), ids.shape[0],
                                       _i32(length, "length"), _i32(tok.shape[1], "H"), _stream()),
            "ca_clip_embed_f32")
