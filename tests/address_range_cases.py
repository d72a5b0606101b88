"""The placement, far-row and limit cases of tests/test_address_range_gpu.py, and a numpy uint32 emulation of the
32-bit address expressions DESIGN.md ("Address arithmetic") lists for the guarded kernels.  Nothing here needs a GPU:
tests/test_address_range_cpu.py checks the coverage, the limits and that named slips move the emulated addresses."""
from __future__ import annotations

import numpy as np

import clip_cases as CL
import gemm_route_cases as G
import t5_cases as T5
import vae_cases as V
from conceptattention_amd import _lib as L

LINE = 1 << 32

# ---- a. placement: one case of attn_cases.py per attention kernel, with every operand role the kernel has
ATTN_PLACEMENT = {
    "ca_attn_kernel<8>": "scale_nk145_ragged_straddle_tail",
    "ca_attn4_kernel": "pre_hm_C1",
    "ca_attn4_qk16_kernel": "qk16_hm_C1",
}
_QKV = ["q", "q1", "k0/v0", "k1/v1", "out", "out1", "out_f32"]
ATTN_ROLES = {
    "ca_attn_kernel<8>": _QKV,                        # (hm_con / hm_part: refused for this kernel by the validator)
    "ca_attn4_kernel": _QKV + ["hm_con", "hm_part"],
    "ca_attn4_qk16_kernel": _QKV + ["hm_con", "hm_part"],
}

# GEMM: per launch route the epilogues that between them use every operand role the route's kernel can take
GEMM_EPIS = ["gate_items_bf16", "gate_rows_f32", "split_gelu", "qkv_single_qpre_f32_f16"]
GEMM_INPUT_FIELD = {"A": "a", "W": "w", "bias": "bias", "scales": "a_scale", "w_scale": "w_scale", "gates": "gate",
                    "gate2": "gate2", "rope": "rope", "norm_q": "norm_q", "norm_k": "norm_k"}
GEMM_ISSUE_ROLES = {"A", "W", "bias", "out", "resid", "out2", "q_prerope", "rope", "gates", "scales"}


def gemm_roles(epi: str, fp8: bool) -> list:
    """The operand roles of one GEMM placement case (the buffers test_gemm_routes_gpu.build names), in the order run."""
    e = G.EPIS[epi]["epi"]
    roles = ["A", "W", "bias", "out"] + (["scales", "w_scale"] if fp8 else [])
    if e == L.EPI_GATE_RESIDUAL:
        roles += ["resid", "gates", "gate2"]
    elif e == L.EPI_SPLIT_GELU:
        roles += ["out2"]
    elif e == L.EPI_QKV_NORM_ROPE:
        roles += ["norm_q", "norm_k", "rope", "out2", "q_prerope"]
    return roles


def rowop_roles(case) -> list:
    """The input and output planes of one row-op case (the buffers the run helpers of test_rowop_routes_gpu name)."""
    s, op = case.shape, case.op
    if op == "ln":
        return ["x", "shift", "scale", "out"] + {"split": ["out_lo"], "fp8": ["out_scale"]}.get(s["out"], [])
    if op == "qk":
        return ["qkv", "q_scale", "k_scale", "rope"] + (["q_prerope"] if s["pre"] else [])
    if op == "qpre":
        return ["x", "scale"] + (["d"] if s["d"] else []) + (["rope", "q_out"] if s["rope"] else [])
    if op == "gemv":
        return ["x", "w", "out"] + (["bias"] if s["bias"] else [])
    if op == "combine":
        return ["pair", "out"] + (["bias"] if s["bias"] else [])
    if op == "fused":
        return ["acc", "logits"] + (["part"] if s["form"] == "part" else ["img", "con"])
    return {"quant": ["x", "out", "out_scale"], "split": ["x", "hi", "lo"], "logits": ["img", "con", "logits"],
            "norm": ["logits", "acc"], "axpy": ["x", "y"], "temb": ["t", "out"]}[op]


# ---- b. far rows.  GEMM: A alone, then W alone, per launch route, at 3 GiB and at the largest accepted extent
GEMM_FAR_EPI = "bias_bf16"
GEMM_FAR = [(role, name, ext) for role in ("A", "W") for name, ext in (("3GiB", 3 << 30), ("max", (1 << 32) - 1))]
# one real modulation_gemm chunk (ops.modulation_gemm): thin-row kernel, the stacked planes of 8 vectors, K = 3072, W rows
# contiguous over just under 4 GiB; checked rows: the first, the middle and the last 256
MOD_CHUNK = dict(M=16, K=3072, N=((1 << 32) - 1) // (3072 * 2) // 256 * 256)
# operands the audit calls 64-bit clean: one case each with the last row more than 4 GiB from the base
PAST_4GIB = 5 << 30
GEMM_PAST = [("pp256", "bias_bf16", "out"), ("pp256", "bias_f32", "out"), ("pp256", "gate_items_bf16", "resid"),
             ("pp256", "split_gelu", "out2"), ("pp256", "qkv_single_qpre_f32_f16", "q_prerope"),
             ("thin_4x4", "bias_f32", "out"), ("thin_4x4", "qkv_single_qpre_f32_f16", "q_prerope"),
             ("classic_128", "gate_items_bf16", "resid"), ("fp8", "split_gelu", "out2")]
ATTN_PAST = ["q", "out", "out_f32"]
ROWOP_PAST = [("ln_rows6_split_seg15", "x"), ("ln_rows6_split_seg15", "out"), ("ln_rows6_split_seg15", "out_lo"),
              ("ln_split_H264_M9", "x"), ("ln_split_H264_M9", "out"), ("ln_split_H264_M9", "out_lo"),
              ("ln_bf16_H264_M8", "x"), ("ln_bf16_H264_M8", "out"), ("ln_fp8_f32_H4096_seg15", "out"),
              ("qk_h3_seg16_pre", "qkv"), ("logits_bf16_C5_L4352", "img"), ("logits_f32_C8_L257_dim4096", "img"),
              ("fused4_bf16_vectors", "img"), ("fused8_f32_vectors", "img")]

# the autoencoder kernels (ca_vae.hip): one case of vae_cases.py per entry point in which every operand role exists
VAE_PLACEMENT = {"ca_conv3x3_nhwc": "conv_5x7_c96_o48_s1_resid_f32", "ca_groupnorm_nhwc": "gn_C32_hw1025_f32",
                 "ca_softmax_rows_f32": "softmax_n257", "ca_affine_rows_f32": "affine_sample_f32"}
VAE_ROLES = {"ca_conv3x3_nhwc": ["x", "w", "bias", "resid", "out"],
             "ca_groupnorm_nhwc": ["x", "gamma", "beta", "y", "part"],
             "ca_softmax_rows_f32": ["s", "p"], "ca_affine_rows_f32": ["x", "logvar", "noise", "out"]}
# one operand at a time with its last row more than 4 GiB from its base: conv on 5 x 7, B = 2 (out once fp32, once
# bf16), GroupNorm with HW = 7, B = 2, softmax with 5 rows, affine with 70 rows.  The softmax p is run by a test of
# its own: the kernel zeroes p[r, n:ldp], so a far ldp makes it write the whole extent.
VAE_PAST = [("conv_5x7_c96_o48_s1_resid_f32", "x"), ("conv_5x7_c96_o48_s1_resid_f32", "resid"),
            ("conv_5x7_c96_o48_s1_resid_f32", "out"), ("conv4_o36_partial_fragment_bf16", "out"),
            ("gn_C64_hw7_f32", "x"), ("gn_C64_hw7_f32", "y"), ("softmax_n63", "s"), ("softmax_n63", "p"),
            ("affine_decode_bf16", "x"), ("affine_decode_bf16", "out")]
VAE_PAST_OWN_TEST = ("softmax_n63", "p")


# the text, pixel and scoring kernels (ca_t5.hip, ca_clip.hip, ca_pixels.hip, ca_seg.hip): per entry point one small case
# of its case table in which every operand role is present, as the argument of the run helper of its kernel test file
# (tests/test_address_range_gpu.TEXT_RUN), and the roles that helper names
TEXT_PLACEMENT = {
    "ca_t5_attn_bf16": T5.AttnCase(2, 3, 192, "contig", "std8"),
    "ca_t5_rmsnorm_f32in": (256, 7, True),
    "ca_t5_rmsnorm_f32in_fp8": (256, 5, True),
    "ca_gated_mul_bf16": (512, 7, True),
    "ca_gated_mul_fp8": (512, 3),
    "ca_embed_rows_f32": (256, 7, True),
    "ca_clip_attn_bf16": CL.AttnCase(3, 2, 77, "apart"),
    "ca_layernorm_f32in": (256, CL.LN_ROWS, True),          # run with the row_idx gather
    "ca_quick_gelu_bf16": (512, 7, True),
    "ca_clip_embed_f32": 256,
    "ca_pixels_u8_to_nhwc32_bf16": (5, 7, 16, 24),
    "ca_nhwc_f32_to_pixels_u8": (2, 3, 5, 32),
    "ca_seg_score": "map16x16-label64x64",
}
TEXT_ROLES = {
    "ca_t5_attn_bf16": ["q", "k", "v", "bias", "out"],
    "ca_t5_rmsnorm_f32in": ["x", "w", "out"],
    "ca_t5_rmsnorm_f32in_fp8": ["x", "w", "out", "out_scale"],
    "ca_gated_mul_bf16": ["g", "u", "out"],
    "ca_gated_mul_fp8": ["g", "u", "out", "out_scale"],     # (g and u: the two halves of one SPLIT_GELU buffer)
    "ca_embed_rows_f32": ["table", "ids", "out"],
    "ca_clip_attn_bf16": ["q", "k", "v", "out"],
    "ca_layernorm_f32in": ["x", "row_idx", "w", "b", "out"],
    "ca_quick_gelu_bf16": ["x", "out"],
    "ca_clip_embed_f32": ["tok", "pos", "ids", "out"],
    "ca_pixels_u8_to_nhwc32_bf16": ["src", "dst"],
    "ca_nhwc_f32_to_pixels_u8": ["src", "dst"],
    "ca_seg_score": ["map", "label", "result", "mask_out", "coeff_out"],
}
# the operands with a free row stride, each run once with its last row more than 4 GiB from its base:
# (entry point, the run helper's case, role, rows of the far buffer, bytes per element).  64 rows for the attention
# kernels (one tile of T5's, L = 64 of CLIP's; no guard rows), 5 to 9 elsewhere (tok: a vocabulary of 8, pos: its 77 rows)
T5_FAR_ATTN, CLIP_FAR_ATTN = T5.AttnCase(1, 1, 64, "contig", "std1"), CL.AttnCase(1, 2, 64, "apart")
TEXT_PAST = [("ca_t5_attn_bf16", T5_FAR_ATTN, role, 64, 2) for role in ("q", "k", "v", "out")] + \
            [("ca_clip_attn_bf16", CLIP_FAR_ATTN, role, 64, 2) for role in ("q", "k", "v", "out")] + [
    ("ca_t5_rmsnorm_f32in", (256, 7, True), "x", 7, 4), ("ca_t5_rmsnorm_f32in", (256, 7, True), "out", 7, 2),
    ("ca_t5_rmsnorm_f32in_fp8", (256, 5, True), "x", 5, 4), ("ca_t5_rmsnorm_f32in_fp8", (256, 5, True), "out", 5, 1),
    ("ca_gated_mul_bf16", (512, 7, True), "g", 7, 2), ("ca_gated_mul_bf16", (512, 7, True), "u", 7, 2),
    ("ca_gated_mul_bf16", (512, 7, True), "out", 7, 2),
    ("ca_gated_mul_fp8", (512, 7), "g", 7, 2), ("ca_gated_mul_fp8", (512, 7), "out", 7, 1),
    ("ca_embed_rows_f32", (256, 7, True), "table", 8, 2), ("ca_embed_rows_f32", (256, 7, True), "out", 7, 4),
    ("ca_layernorm_f32in", (256, CL.LN_ROWS, True), "x", 9, 4), ("ca_layernorm_f32in", (256, CL.LN_ROWS, True), "out", 6, 2),
    ("ca_layernorm_f32in", (256, CL.LN_ROWS, False), "x", 9, 4),         # row by row, without the gather
    ("ca_layernorm_f32in", (256, CL.LN_ROWS, False), "out", 9, 2),
    ("ca_quick_gelu_bf16", (512, 7, True), "x", 7, 2), ("ca_quick_gelu_bf16", (512, 7, True), "out", 7, 2),
    ("ca_clip_embed_f32", 256, "tok", 8, 2), ("ca_clip_embed_f32", 256, "pos", 77, 2),
    ("ca_clip_embed_f32", 256, "out", 231, 4),
]
# the operands of these entry points that have a free row stride (the others are contiguous by contract: bias, weights,
# ids, row_idx, out_scale, the pixel planes, everything of ca_seg_score).  The src of ca_pixels_u8_to_nhwc32_bf16 has a
# free BYTE stride (an int64_t) over a 3-D buffer: a test of its own.
TEXT_FREE_STRIDES = {
    "ca_t5_attn_bf16": {"q", "k", "v", "out"}, "ca_clip_attn_bf16": {"q", "k", "v", "out"},
    "ca_t5_rmsnorm_f32in": {"x", "out"}, "ca_t5_rmsnorm_f32in_fp8": {"x", "out"},
    "ca_gated_mul_bf16": {"g", "u", "out"}, "ca_gated_mul_fp8": {"g", "out"},      # (g: the buffer that holds g and u)
    "ca_embed_rows_f32": {"table", "out"}, "ca_layernorm_f32in": {"x", "out"}, "ca_quick_gelu_bf16": {"x", "out"},
    "ca_clip_embed_f32": {"tok", "pos", "out"}, "ca_pixels_u8_to_nhwc32_bf16": {"src"},
    "ca_nhwc_f32_to_pixels_u8": set(), "ca_seg_score": set(),
}
TEXT_PAST_OWN_TEST = ("ca_pixels_u8_to_nhwc32_bf16", "src")
PIXEL_FAR = (5, 7, 16, 24)              # five source rows, their byte stride from far_ld(5, 1, PAST_4GIB)
BAD_STRIDE = (1 << 32) + 256            # a row stride whose low 32 bits pass `ld >= H`: ops._i32 refuses it


def vae_roles(case) -> list:
    """The operand roles of one autoencoder case (the buffers the run helpers of test_vae_routes_gpu name)."""
    s = case.shape
    if case.op == "conv":
        return ["x", "w", "out"] + (["bias"] if s["bias"] else []) + (["resid"] if s["resid"] == "separate" else [])
    if case.op == "affine":
        return ["x", "out"] + (["logvar", "noise"] if s["lv"] else [])
    return {"gn": ["x", "gamma", "beta", "y", "part"], "softmax": ["s", "p"]}[case.op]


def vae_far_rows(cid: str, role: str):
    """(rows, bytes per element) of the 2-D buffer that carries `role` in case cid."""
    case = V.BY_ID[cid]
    inp = V.make_inputs(case)
    buf = inp[{"out": "out0", "y": "y0", "p": "p0"}.get(role, role)]
    assert buf.dim() == 2, (cid, role)
    return buf.shape[0], buf.element_size()


def far_ld(rows: int, itemsize: int, extent: int) -> int:
    """The largest row stride (a multiple of 64 elements) with rows * ld * itemsize <= extent."""
    return extent // (rows * itemsize) // 64 * 64


def gemm_epis_for(route: str) -> list:
    return [e for e in GEMM_EPIS if G.compatible(route, e)]


def gemm_kernel_of(route: str) -> str:
    """The kernel instantiation a route of gemm_route_cases.ROUTES launches for its main or thin part."""
    r = G.ROUTES[route]
    if isinstance(r.thin, tuple):
        return f"ca_gemm_thin_kernel<{r.thin[0]},{r.thin[1]}>"
    fam = {L.GEMM_KERNEL_CLASSIC: "ca_gemm_kernel", L.GEMM_KERNEL_PP: "ca_gemm_pp_kernel",
           L.GEMM_KERNEL_PP_FP8: "ca_gemm_pp_fp8_kernel"}[r.kernel]
    return f"{fam}<{G.TILE_W[r.tile]}>" + ("+thin tiles" if r.thin == "walk" else "")


# ---- b. far rows (attention): (nq, n0, n1, nq0), the value of (n0 + n1) * ldkv * 2 aimed at
ATTN_FAR = {
    "seg0_3GiB": ((70, 389, 0, 30), 3 << 30),
    "seg0_max": ((70, 389, 0, 30), LINE - 1),
    "seg1_3GiB": ((70, 100, 289, 30), 3 << 30),      # tile 1 straddles the segments, tile 6 is ragged
    "seg1_max": ((70, 100, 289, 30), LINE - 1),
}
# ---- c. limits: name -> (keys, the smallest ldkv the validator refuses)
ATTN_LIMITS = {
    "(n0 + n1) * ldkv * 2 < 2^32": (512, 1 << 22),
    "64 * ldkv * 2 < 2^32": (32, 1 << 25),
}


def far_ldkv(nk: int, extent: int) -> int:
    """The largest row stride (a multiple of 8 elements) with nk * ldkv * 2 <= extent."""
    return extent // (2 * nk) // 8 * 8


def attn_accepts(n0: int, n1: int, ldkv: int) -> bool:
    """The extent check of ca_attn_fwd_impl."""
    return (n0 + n1) * ldkv * 2 < LINE and 64 * ldkv * 2 < LINE


# ---- emulation of the 32-bit expressions (ca_attn.hip:94-95, ca_attn4_kernel.inc:60-61, 106, 128)
def attn_offsets_u32(n0: int, n1: int, ldkv: int, slip=None):
    """For every 16-byte K access of the fast path of ca_attn4_kernel (full tiles inside one segment): the kernel's
    32-bit arithmetic (scalar offset SO = tile * 64 * ldkv * 2 in uint32 plus lane offset koff = (r * ldkv + chunk * 8)
    * 2 in uint32, added to the descriptor base in 64 bits) and the exact 64-bit byte offset from key 0.
    Returns (emulated uint64 array, exact uint64 array).  slip: None | "sign_extend" (the scalar offset sign-extended) |
    "row_ld_i32" (row * ldkv as a signed 32-bit product).  (SO + koff stays below 2^32 for every accepted extent, so
    adding the two in 32 bits is no slip; the dropped carry into bit 32 is a slip of the base: base_address_slips.)"""
    nk = n0 + n1
    nt_full = nk // 64
    t_str = n0 // 64 if (n0 % 64 and n0 < nk) else -1
    tiles = np.array([t for t in range(nt_full) if t != t_str], dtype=np.uint64)
    r = np.arange(64, dtype=np.uint64)
    chunk = np.uint64(15)                                       # the highest 16-byte chunk of a 256-byte head row
    exact = ((tiles[:, None] * np.uint64(64) + r[None, :]) * np.uint64(ldkv) + chunk * np.uint64(8)) * np.uint64(2)
    with np.errstate(over="ignore"):
        so = (tiles.astype(np.uint32) * np.uint32(64)) * np.uint32(ldkv) * np.uint32(2)
        koff = (r.astype(np.uint32) * np.uint32(ldkv) + np.uint32(15 * 8)) * np.uint32(2)
        if slip == "row_ld_i32":
            key = (tiles[:, None] * np.uint64(64) + r[None, :]).astype(np.int64)
            prod = (key * ldkv * 2 + 240).astype(np.int32)     # one signed 32-bit product for the whole offset
            return prod.astype(np.int64).astype(np.uint64).ravel(), exact.ravel()
        emu = so[:, None].astype(np.uint64) + koff[None, :].astype(np.uint64)
        if slip == "sign_extend":
            emu = (so[:, None].astype(np.int32).astype(np.int64) + koff[None, :].astype(np.uint64).astype(np.int64)
                   ).astype(np.uint64)
    return emu.ravel(), exact.ravel()


def base_address_slips(start: int, nbytes: int, step: int = 16):
    """The absolute addresses of a buffer's 16-byte accesses, and the same with the low half sign-extended / the carry
    into bit 32 dropped (base halves rebuilt wrongly from two readfirstlanes)."""
    a = np.arange(start, start + nbytes, step, dtype=np.uint64)
    lo = (a & np.uint64(0xffffffff)).astype(np.uint32)
    hi = a >> np.uint64(32)
    sign = ((hi.astype(np.int64) << 32) + lo.astype(np.int32).astype(np.int64)).astype(np.uint64)
    base_hi = np.uint64(start >> 32)
    nocarry = (base_hi << np.uint64(32)) | lo.astype(np.uint64)
    return a, sign, nocarry
