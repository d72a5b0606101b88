"""ctypes binding of libconceptattn.so (the C ABI declared in include/conceptattn.h).

The library is the product path: there is no Python/PyTorch fallback.  If the shared object is
missing or does not export a symbol, loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CA_LIB_PATH: another build of the same library (an A/B against another source tree); still no fallback
LIB_PATH = os.environ.get("CA_LIB_PATH") or os.path.join(_HERE, "libconceptattn.so")

CA_VERSION = 137
EPI_BIAS, EPI_GELU_TANH, EPI_GATE_RESIDUAL, EPI_SPLIT_GELU, EPI_QKV_NORM_ROPE = 0, 1, 2, 3, 4
TILE_AUTO, TILE_256x256, TILE_256x192, TILE_256x128, TILE_256x64 = 0, 1, 2, 3, 4
TILE_PP_256x256, TILE_PP_256x128, TILE_PP_256x192 = 5, 6, 7
GEMM_KERNEL_NONE, GEMM_KERNEL_CLASSIC, GEMM_KERNEL_PP, GEMM_KERNEL_PP_FP8 = 0, 1, 2, 3
NORM_SOFTMAX, NORM_SPARSEMAX, NORM_ENTMAX15 = 0, 1, 2
NORMS = {"softmax": NORM_SOFTMAX, "sparsemax": NORM_SPARSEMAX, "entmax15": NORM_ENTMAX15}
NORM_NONE = 3                        # ca_head_maps only (csrc/ca_headmap.h): the weights are the logits themselves
MAX_SEGMENTS = 16
GEMM_MAX_PROBLEMS = 2
ATTN_MAX_PROBLEMS = 16
HEATMAP_MAX_PROBLEMS = 16
HEATMAP_MAX_CONCEPTS = 32            # ca_heatmap_many, and the sparse norms of ca_heatmap_norm_accumulate
HEATMAP_SPARSE_MAX_3LAUNCH = 16      # what ops.heatmap_softmax_accumulate takes with a sparse norm (ops.heatmap_norm_accumulate: 32)
SEG_MAX_PROBLEMS = 16
SEG_MAX_CELLS = 4096                # ca_seg_score: h * w of the map
SEG_MAX_LABEL_PIXELS = 1 << 24      # ca_seg_score: Hl * Wl of the label
SEG_MEAN_THRESHOLD, SEG_DOWNSCALE, SEG_BLUR = 1, 2, 4
MSEG_MAX_PROBLEMS = 16
MSEG_MAX_CONCEPTS = 32              # ca_mseg_score: K, the maps of an item
MSEG_MAX_CLASSES = 256              # ca_mseg_score: nclass
MSEG_MAX_CELLS = 16384              # ca_mseg_score: h * w of the maps
MSEG_MAX_LABEL_PIXELS = 1 << 24     # ca_mseg_score: Hl * Wl of the label
MSEG_BLUR = 4
SEGTAB_MAX_MAPS = 65536              # ca_segtab_score: maps of one call
SEGTAB_MEAN_THRESHOLD, SEGTAB_DOWNSCALE, SEGTAB_BLUR, SEGTAB_RAW = 1, 2, 4, 8
RENDER_MAX_PROBLEMS = 16             # ca_heatmap_render: groups of one launch
RENDER_MAX_MAPS = 65536              # ca_heatmap_render: planes of one group
RENDER_MAX_CELLS = 16384             # ca_heatmap_render: h * w of the maps
RENDER_MAX_SIDE = 4096               # ca_heatmap_render: H and W of the pictures
RENDER_LUT_ROWS = 259                # 256 colours, then under, over, bad
RENDER_BILINEAR, RENDER_BLEND = 1, 2
TOKMAP_MAX_PROBLEMS = 16             # ca_token_maps: problems of one launch (ops.token_maps splits longer lists)
TOKMAP_MAX_TEXT = 512                # ca_token_maps: n0, the text key rows of a problem
TOKMAP_QK_F16 = 1                    # ca_token_maps flags: IEEE half bits in the bf16-typed q / k rows
QUERYMAP_MAX_PROBLEMS = 16           # ca_query_maps: problems of one launch (ops.query_maps splits longer lists)
QUERYMAP_MAX_QUERIES = 512           # ca_query_maps: nq, the query rows of a problem
QUERYMAP_MAX_ROWS = 2 ** 31 - 128    # ca_query_maps: n0 + n1, the key rows of a problem
QUERYMAP_QK_F16 = 1                  # ca_query_maps flags: IEEE half bits in the bf16-typed q / k rows
PROPMAP_MAX_PROBLEMS = 16            # ca_propagate_maps: problems of one launch (ops.propagate_maps splits longer lists)
PROPMAP_MAX_CONCEPTS = 32            # ca_propagate_maps: C, the map rows of a problem
PROPMAP_MAX_ROWS = 2 ** 31 - 128     # ca_propagate_maps: n0 + n1, the key rows of a problem
PROPMAP_MAX_HEADS = 65535            # ca_propagate_maps: num_heads
PROPMAP_QK_F16 = 1                   # ca_propagate_maps flags: IEEE half bits in the bf16-typed q / k rows
HEADMAP_MAX_HEADS = 65536            # ca_head_maps: num_heads (heads of 128 columns)
ATTN_Q_PRESCALED = 0.0   # ca_attn_fwd_bf16(scale=...): the q rows already carry softmax_scale * log2(e)


class GemmProblem(C.Structure):
    _fields_ = [("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
                ("resid", C.c_void_p), ("gate", C.c_void_p), ("gate2", C.c_void_p), ("out2", C.c_void_p),
                ("norm_q", C.c_void_p), ("norm_k", C.c_void_p), ("rope", C.c_void_p), ("q_prerope", C.c_void_p),
                ("a_scale", C.c_void_p), ("w_scale", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("lda", C.c_int32), ("ldw", C.c_int32), ("ldc", C.c_int32), ("ldr", C.c_int32),
                ("ld2", C.c_int32), ("n_split", C.c_int32), ("gate_rows", C.c_int32),
                ("epilogue", C.c_int32), ("ldp", C.c_int32), ("out_f32", C.c_int32), ("gate_stride", C.c_int32),
                ("gate_item_rows", C.c_int32), ("gate2_item_rows", C.c_int32),
                ("qpre_f32", C.c_int32), ("q_out_scale", C.c_float), ("qk_f16", C.c_int32), ("_pad", C.c_int32)]


class GemmPlanInfo(C.Structure):
    _fields_ = [("tile", C.c_int32), ("kernel", C.c_int32), ("grid", C.c_int32), ("persistent", C.c_int32),
                ("main_tiles", C.c_int32), ("thin_tiles", C.c_int32), ("thin_mf", C.c_int32), ("thin_nw", C.c_int32),
                ("thin_groups", C.c_int32), ("thin_grid_x", C.c_int32), ("n_cu", C.c_int32), ("_pad", C.c_int32)]


class AttnProblem(C.Structure):
    _fields_ = [("q", C.c_void_p), ("out", C.c_void_p), ("k0", C.c_void_p), ("v0", C.c_void_p),
                ("k1", C.c_void_p), ("v1", C.c_void_p), ("out_f32", C.c_void_p),
                ("q1", C.c_void_p), ("out1", C.c_void_p), ("hm_con", C.c_void_p), ("hm_part", C.c_void_p),
                ("nq", C.c_int32), ("n0", C.c_int32), ("n1", C.c_int32),
                ("ldq", C.c_int32), ("ldo", C.c_int32), ("ldkv", C.c_int32), ("ldo32", C.c_int32),
                ("nq0", C.c_int32), ("hm_C", C.c_int32), ("ldhc", C.c_int32), ("_pad", C.c_int32)]


class HeatmapProblem(C.Structure):
    _fields_ = [("img_vec", C.c_void_p), ("con_vec", C.c_void_p), ("acc", C.c_void_p), ("acc2", C.c_void_p),
                ("logits", C.c_void_p), ("ldi", C.c_int32), ("ldc", C.c_int32), ("img_f32", C.c_int32),
                ("con_f32", C.c_int32), ("weight", C.c_float), ("weight2", C.c_float)]


class TokmapProblem(C.Structure):    # ca_tokmap_problem (csrc/ca_tokmap.h), field for field
    _fields_ = [("q", C.c_void_p), ("k0", C.c_void_p), ("k1", C.c_void_p), ("acc", C.c_void_p), ("acc2", C.c_void_p),
                ("lse", C.c_void_p), ("nq", C.c_int32), ("ldq", C.c_int32), ("n0", C.c_int32), ("n1", C.c_int32),
                ("ldk", C.c_int32), ("n_tok", C.c_int32), ("weight", C.c_float), ("weight2", C.c_float)]


class QuerymapProblem(C.Structure):  # ca_querymap_problem (csrc/ca_querymap.h), field for field
    _fields_ = [("q", C.c_void_p), ("k0", C.c_void_p), ("k1", C.c_void_p), ("acc", C.c_void_p), ("acc2", C.c_void_p),
                ("lse", C.c_void_p), ("nq", C.c_int32), ("ldq", C.c_int32), ("n0", C.c_int32), ("n1", C.c_int32),
                ("ldk", C.c_int32), ("_pad", C.c_int32), ("weight", C.c_float), ("weight2", C.c_float)]


class PropmapProblem(C.Structure):   # ca_propmap_problem (csrc/ca_propmap.h), field for field
    _fields_ = [("q", C.c_void_p), ("k0", C.c_void_p), ("k1", C.c_void_p), ("v", C.c_void_p), ("acc", C.c_void_p),
                ("acc2", C.c_void_p), ("nq", C.c_int32), ("ldq", C.c_int32), ("n0", C.c_int32), ("n1", C.c_int32),
                ("ldk", C.c_int32), ("C", C.c_int32), ("ldv", C.c_int32), ("_pad", C.c_int32), ("weight", C.c_float),
                ("weight2", C.c_float)]


class HeadmapProblem(C.Structure):   # ca_headmap_problem (csrc/ca_headmap.h), field for field
    _fields_ = [("img", C.c_void_p), ("con", C.c_void_p), ("heads", C.c_void_p), ("acc", C.c_void_p), ("acc2", C.c_void_p),
                ("ldi", C.c_int32), ("ldc", C.c_int32), ("img_f32", C.c_int32), ("con_f32", C.c_int32),
                ("weight_h", C.c_float), ("weight", C.c_float), ("weight2", C.c_float), ("_pad", C.c_int32)]


class SegProblem(C.Structure):
    _fields_ = [("map", C.c_void_p), ("label", C.c_void_p), ("result", C.c_void_p), ("mask_out", C.c_void_p),
                ("coeff_out", C.c_void_p)]


class SegRecord(C.Structure):
    _fields_ = [("n11", C.c_int32), ("n10", C.c_int32), ("n01", C.c_int32), ("n00", C.c_int32), ("ap", C.c_double),
                ("mean", C.c_float), ("lo", C.c_float), ("hi", C.c_float), ("thresholds", C.c_int32)]


class MsegProblem(C.Structure):
    _fields_ = [("maps", C.c_void_p), ("label", C.c_void_p), ("counts", C.c_void_p), ("class_out", C.c_void_p),
                ("index_out", C.c_void_p)]


class RenderProblem(C.Structure):
    _fields_ = [("maps", C.c_void_p), ("map_stride", C.c_int64), ("n_maps", C.c_int32), ("range_in", C.c_void_p),
                ("range_out", C.c_void_p), ("image", C.c_void_p), ("image_stride", C.c_int64), ("out", C.c_void_p),
                ("out_stride", C.c_int64)]


class ModSegment(C.Structure):
    _fields_ = [("row_end", C.c_int32), ("_pad", C.c_int32), ("shift", C.c_void_p), ("scale", C.c_void_p)]


class NormSegment(C.Structure):
    _fields_ = [("row_end", C.c_int32), ("_pad", C.c_int32), ("q_scale", C.c_void_p), ("k_scale", C.c_void_p)]


# name -> (restype, argtypes); every symbol include/conceptattn.h declares
SIGNATURES = {
    "ca_version": (C.c_int, []),
    "ca_last_error": (C.c_char_p, []),
    "ca_check_device": (C.c_int, []),
    "ca_gemm_bf16": (C.c_int, [C.POINTER(GemmProblem), C.c_int32, C.c_int32, C.c_void_p]),
    "ca_gemm_auto_tile": (C.c_int, [C.POINTER(GemmProblem), C.c_int32]),
    "ca_gemm_fp8": (C.c_int, [C.POINTER(GemmProblem), C.c_int32, C.c_void_p]),
    "ca_gemm_plan": (C.c_int, [C.POINTER(GemmProblem), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.POINTER(GemmPlanInfo)]),
    "ca_attn_fwd_bf16": (C.c_int, [C.POINTER(AttnProblem), C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "ca_attn_fwd_qk16": (C.c_int, [C.POINTER(AttnProblem), C.c_int32, C.c_int32, C.c_void_p]),
    "ca_attn_stats": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int32]),
    "ca_ln_modulate_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(ModSegment), C.c_int32, C.c_float, C.c_void_p]),
    "ca_ln_modulate_fp8": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                     C.POINTER(ModSegment), C.c_int32, C.c_float, C.c_void_p]),
    "ca_ln_modulate_f32in": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(ModSegment), C.c_int32, C.c_float, C.c_void_p]),
    "ca_ln_modulate_f32in_fp8": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_int32, C.POINTER(ModSegment), C.c_int32, C.c_float, C.c_void_p]),
    "ca_ln_modulate_f32in_split": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                             C.c_int32, C.c_int32, C.POINTER(ModSegment), C.c_int32, C.c_float,
                                             C.c_void_p]),
    "ca_qpre_finish_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_void_p]),
    "ca_qpre_finish_rope_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_quantize_rows_fp8": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_void_p]),
    "ca_qknorm_rope_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(NormSegment),
                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "ca_gemv_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                               C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_heatmap_logits_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ca_heatmap_softmax_accumulate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                                C.c_void_p]),
    "ca_heatmap_norm_accumulate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                             C.c_void_p]),
    "ca_heatmap_fused": (C.c_int, [C.POINTER(HeatmapProblem), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_void_p]),
    "ca_timestep_embedding_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_float,
                                            C.c_void_p]),
    "ca_axpy_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_void_p]),
    "ca_silu_split_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p]),
    "ca_axpy_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int64, C.c_void_p]),
    "ca_split_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                C.c_void_p]),
    "ca_modulation_combine_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_void_p]),
    "ca_conv3x3_nhwc": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 12 + [C.c_void_p]),
    "ca_groupnorm_nhwc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_int32,
                                    C.c_void_p]),
    "ca_softmax_rows_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                      C.c_void_p]),
    "ca_affine_rows_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_void_p]),
    "ca_t5_attn_bf16": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 7 + [C.c_void_p]),
    "ca_t5_rmsnorm_f32in": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                      C.c_float, C.c_void_p]),
    "ca_gated_mul_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64,
                                    C.c_int32, C.c_void_p]),
    "ca_t5_rmsnorm_f32in_fp8": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                          C.c_int32, C.c_float, C.c_void_p]),
    "ca_gated_mul_fp8": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_int64, C.c_int32, C.c_void_p]),
    "ca_embed_rows_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                    C.c_void_p]),
    "ca_clip_attn_bf16": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 7 + [C.c_float, C.c_void_p]),
    "ca_layernorm_f32in": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_int64, C.c_int32, C.c_float, C.c_void_p]),
    "ca_quick_gelu_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]),
    "ca_clip_embed_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_pixels_u8_to_nhwc32_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_void_p]),
    "ca_nhwc_f32_to_pixels_u8": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "ca_seg_score": (C.c_int, [C.POINTER(SegProblem), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.POINTER(C.c_float), C.c_void_p]),
    "ca_mseg_score": (C.c_int, [C.POINTER(MsegProblem), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                C.c_void_p]),
    "ca_segtab_score": (C.c_int, [C.POINTER(C.c_float), C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                  C.c_void_p]),
    "ca_heatmap_render": (C.c_int, [C.POINTER(RenderProblem), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_float, C.c_int32, C.c_void_p]),
}

# exported by the library and bound here, not declared in include/conceptattn.h yet (csrc/ca_heatmap_core.h,
# csrc/ca_tokmap.h, csrc/ca_headmap.h, csrc/ca_querymap.h and csrc/ca_propmap.h declare them)
INTERNAL_SIGNATURES = {
    "ca_heatmap_many": (C.c_int, [C.POINTER(HeatmapProblem), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_void_p]),
    "ca_token_maps": (C.c_int, [C.POINTER(TokmapProblem), C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                C.c_int64, C.c_void_p]),
    "ca_token_maps_workspace_bytes": (C.c_int64, [C.POINTER(TokmapProblem), C.c_int32, C.c_int32]),
    "ca_head_maps": (C.c_int, [C.POINTER(HeadmapProblem), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_void_p]),
    "ca_query_maps": (C.c_int, [C.POINTER(QuerymapProblem), C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                C.c_int64, C.c_void_p]),
    "ca_query_maps_workspace_bytes": (C.c_int64, [C.POINTER(QuerymapProblem), C.c_int32, C.c_int32]),
    "ca_propagate_maps": (C.c_int, [C.POINTER(PropmapProblem), C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                    C.c_int64, C.c_void_p]),
    "ca_propagate_maps_workspace_bytes": (C.c_int64, [C.POINTER(PropmapProblem), C.c_int32, C.c_int32]),
}

_lib = None


class ConceptAttnError(RuntimeError):
    pass


def load() -> C.CDLL:
    """dlopen libconceptattn.so and bind every entry point; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch ships its own libamdhip64; whichever HIP runtime is mapped first serves the whole process.  Import
    # torch before the dlopen so that the tensors' runtime is also the one the kernels are launched through
    # (the other order leaves this library on /opt/rocm's runtime, which then reports "no ROCm-capable device").
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ConceptAttnError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **INTERNAL_SIGNATURES}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ConceptAttnError(f"{LIB_PATH} does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    if lib.ca_version() != CA_VERSION:
        raise ConceptAttnError(f"libconceptattn version {lib.ca_version()} != binding {CA_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().ca_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise ConceptAttnError(f"{what}: rc={rc}: {msg}")
