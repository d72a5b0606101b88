/*
 * conceptattn.h -- C ABI of libconceptattn.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * ConceptAttention inference hot path.
 *
 * The reference (manuragkhullar/ConceptAttention) is pure PyTorch and has no FFI; what this
 * library replaces are the PyTorch op sequences on the path.  Each
 * entry point cites the reference lines (relative to the reference root) whose arithmetic it
 * implements.  The reference-side binding a maintainer would add is the ctypes stub shown in
 * INTEGRATION.md; conceptattention_amd/_lib.py is that stub.
 *
 * Contract (all entry points):
 *   - plain C types only; every pointer is a DEVICE pointer borrowed from the caller (PyTorch
 *     tensors); the library never allocates, frees or retains device memory;
 *   - every call is asynchronous on the hipStream_t passed as `stream` (a void* here) and does
 *     no host synchronisation, so calls may be captured into a hipGraph;
 *   - returns 0 on success, a negative CA_ERR_* code on a rejected argument (nothing is
 *     launched in that case); ca_last_error() gives a thread-local message;
 *   - activations and weights are bf16 row-major; modulation vectors, RoPE tables, logits and
 *     heat-map accumulators are fp32; matrix products accumulate in fp32 (MFMA).
 *   - head_dim is fixed at 128 (Flux geometry: concept_attention/flux/src/flux/util.py:34-47).
 */
#ifndef CONCEPTATTN_H
#define CONCEPTATTN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CA_VERSION 137 /* 0.1.2: ca_gemm_problem.qpre_f32 / q_out_scale, fp32 image vectors in ca_heatmap_logits_bf16,
                          CA_ATTN_Q_PRESCALED; .1: ca_axpy_f32, ca_split_bf16; .2: ca_attn_stats; .3: ca_gemm_problem.qk_f16,
                          ca_attn_fwd_qk16; .4: ca_qpre_finish_rope_f32; .5: ca_heatmap_fused; .6: ca_gemm_plan;
                          .7: the autoencoder kernels (conv3x3_nhwc, groupnorm_nhwc, softmax_rows_f32, affine_rows_f32);
                          128: the T5 encoder kernels (t5_attn_bf16, t5_rmsnorm_f32in, gated_mul_bf16, embed_rows_f32);
                          129: the CLIP text encoder kernels (clip_attn_bf16, layernorm_f32in, quick_gelu_bf16,
                          clip_embed_f32); 130: the pixel I/O kernels (pixels_u8_to_nhwc32_bf16, nhwc_f32_to_pixels_u8);
                          131: the T5 encoder's e4m3 producers (t5_rmsnorm_f32in_fp8, gated_mul_fp8);
                          132: segmentation scoring on the device (seg_score);
                          133: multi-class segmentation scoring on the device (mseg_score);
                          134: sweep tables of maps scored against one label on the device (segtab_score);
                          135: heat-map pictures on the device (heatmap_render);
                          136: sparse norms of heatmap_norm_accumulate up to C = 32 (CA_HEATMAP_MAX_CONCEPTS);
                          137: per-head concept maps (head_maps, declared in csrc/ca_headmap.h) */

#define CA_OK 0
#define CA_ERR_ARG (-1)    /* bad shape / null pointer / misalignment */
#define CA_ERR_LAUNCH (-2) /* hip launch failure */
#define CA_ERR_ARCH (-3)   /* device is not gfx950 */

typedef void *ca_stream_t; /* hipStream_t */

int ca_version(void);
const char *ca_last_error(void);
/* 0 if the current device is gfx950, CA_ERR_ARCH otherwise. */
int ca_check_device(void);

/* ------------------------------------------------------------------------------------------
 * Grouped GEMM with fused epilogue:  out[m,n] = epi( sum_k A[m,k] * W[n,k] + bias[n] )
 * Replaces nn.Linear on the path: qkv / proj / mlp of ModifiedDoubleStreamBlock
 * (concept_attention/modified_double_stream_block.py:90,96,102,194-202), linear1 / linear2 of
 * ModifiedSingleStreamBlock (concept_attention/modified_single_stream_block.py:49-54), img_in /
 * txt_in / final_layer.linear (concept_attention/modified_flux_dit.py:98,105,120,159).
 * Up to CA_GEMM_MAX_PROBLEMS problems share one launch (image stream + text/concept stream of a
 * double block), so the grid fills all 256 CUs.
 * Requirements: K % 64 == 0, N % tile_n == 0, lda/ldw/ldc/ldr/ld2 % 8 == 0, 16-byte aligned
 * pointers.  M is arbitrary (rows are masked) up to the extent limit: the A and W operands are addressed with
 * unsigned 32-bit byte offsets from their base, so M * lda * elem_size and N * ldw * elem_size must each stay below
 * 2^32 (CA_ERR_ARG "operand larger than 4 GiB" otherwise); out, resid, out2, q_prerope, rope and the gate vectors
 * are addressed in 64 bits and have no limit.  A call is one kernel launch on `stream`, or two:
 * under the 256x256 ping-pong tile a problem's last row tile with at most 128 rows (M % 256 in
 * [1, 128]: the concept rows a [concept | text] stream carries past its full row tiles) runs as
 * 32 x 128 tiles of a second kernel queued right behind the first (bit-identical results).
 */
enum {
  CA_EPI_BIAS = 0,          /* out = acc + bias */
  CA_EPI_GELU_TANH = 1,     /* out = gelu_tanh(acc + bias)          (mlp.0, :196)          */
  CA_EPI_GATE_RESIDUAL = 2, /* out = resid + gate[n]*(acc + bias)   (:194-202)             */
  CA_EPI_SPLIT_GELU = 3,    /* n <  n_split: out  = acc + bias                             */
                            /* n >= n_split: out2 = gelu_tanh(acc+bias), column n-n_split  */
                            /* (single block linear1 -> qkv | mlp, single_stream_block:49) */
  CA_EPI_QKV_NORM_ROPE = 4  /* qkv projection with QKNorm + RoPE fused (256x256 ping-pong tile only):      */
                            /* columns [0, n_split) are q|k|v thirds of heads*128 columns each (or, with    */
                            /* N = n_split / 3, the q third alone);                                          */
                            /* q, k: out = rope(rmsnorm(acc+bias) * norm_{q,k}), optional q_prerope store;   */
                            /* v: out = acc + bias; columns >= n_split: out2 = gelu_tanh(acc+bias)           */
                            /* (flux/modules/layers.py:63-84, flux/math.py:25-30, double_stream_block:189)  */
};

/* tile = block tile M x N; the PP ("ping-pong") kernels are the pipelined fast path */
enum { CA_TILE_AUTO = 0, CA_TILE_256x256 = 1, CA_TILE_256x192 = 2, CA_TILE_256x128 = 3, CA_TILE_256x64 = 4,
       CA_TILE_PP_256x256 = 5, CA_TILE_PP_256x128 = 6, CA_TILE_PP_256x192 = 7 };

#define CA_GEMM_MAX_PROBLEMS 2

typedef struct {
  const void *A;     /* bf16 [M,K], row stride lda (elements) */
  const void *W;     /* bf16 [N,K], row stride ldw: nn.Linear weight (out,in) */
  const void *bias;  /* bf16 [N] or NULL */
  void *out;         /* bf16 [M,N] (or [M,n_split] for SPLIT_GELU), row stride ldc */
  const void *resid; /* bf16 [M,N], row stride ldr; GATE_RESIDUAL only; may alias out */
  const float *gate; /* fp32 [N]; GATE_RESIDUAL: gate for rows <  gate_rows */
  const float *gate2;/* fp32 [N]; GATE_RESIDUAL: gate for rows >= gate_rows (may be NULL if gate_rows >= M) */
  void *out2;        /* bf16 [M,N-n_split], row stride ld2; SPLIT_GELU / QKV_NORM_ROPE tail */
  const void *norm_q;/* bf16 [128] query_norm.scale; QKV_NORM_ROPE only */
  const void *norm_k;/* bf16 [128] key_norm.scale */
  const float *rope; /* fp32 [M,64,2] (cos,sin) for this problem's rows */
  void *q_prerope;   /* optional [M, heads*128], row stride ldp: normalised pre-RoPE q; bf16, or fp32 if qpre_f32 */
  const float *a_scale; /* ca_gemm_fp8 only: fp32 [M], dequantisation scale of each row of A */
  const float *w_scale; /* ca_gemm_fp8 only: fp32 [N], dequantisation scale of each row of W */
  int32_t M, N, K;
  int32_t lda, ldw, ldc, ldr, ld2;
  int32_t n_split;   /* SPLIT_GELU: multiple of the tile width; QKV_NORM_ROPE: 3*heads*128 */
  int32_t gate_rows;
  int32_t epilogue;  /* CA_EPI_* */
  int32_t ldp;       /* row stride of q_prerope */
  int32_t out_f32;   /* 1: `out` (and `resid`) hold fp32 elements (ldc/ldr still in elements, % 4 == 0); BIAS and
                        GATE_RESIDUAL only.  The fp32 residual stream: img_in / txt_in write it, the attention-
                        and MLP-output projections update it in place; 0: bf16 as above */
  int32_t gate_stride;     /* GATE_RESIDUAL, batched forward: 0 = one gate vector per row range (above); else the */
  int32_t gate_item_rows;  /* rows < gate_rows are consecutive work items of gate_item_rows rows, the others of     */
  int32_t gate2_item_rows; /* gate2_item_rows rows, and item i of a range uses its base vector + i * gate_stride   */
                           /* floats (gate_stride % 4 == 0): every item of a batch has its own adaLN gates         */
  int32_t qpre_f32;        /* QKV_NORM_ROPE: 1 = q_prerope holds fp32 elements (ldp in elements, % 4 == 0): the    */
                           /* cross-attention-space vectors of modified_double_stream_block.py:189-190 without     */
                           /* their bf16 rounding (the heat-map logits are then formed from fp32 q on both sides); */
                           /* 2 = fp32 too, but the q projection (acc + bias) BEFORE its RMS norm: the caller adds */
                           /* a correction and normalises with ca_qpre_finish_f32;                                 */
                           /* 3 = (round 5) that correction fused: q_prerope holds such a raw projection on ENTRY, */
                           /* it is added to acc + bias before the norm and overwritten with the normalised vector */
                           /* -- the low-plane q projection of a captured layer (N = n_split / 3: the q third      */
                           /* alone, `out` = the attention's q rows): one launch instead of GEMM + finish kernel   */
  float q_out_scale;       /* QKV_NORM_ROPE: the rotated q is multiplied by this in fp32 before its ONE rounding   */
                           /* to bf16 (0 = 1.0; k, v and q_prerope are not scaled).  With softmax_scale * log2(e)  */
                           /* here, ca_attn_fwd_bf16(scale = CA_ATTN_Q_PRESCALED) needs no per-score multiply      */
  int32_t qk_f16;          /* QKV_NORM_ROPE: 1 = the rotated q and k are stored as IEEE half (fp16, 11-bit         */
                           /* mantissa; |values| stay far below 65504 behind an RMS norm) in the same 2-byte       */
                           /* elements of `out`; v stays bf16.  Read by ca_attn_fwd_qk16.  0 = bf16                */
  int32_t _pad;
} ca_gemm_problem;

int ca_gemm_bf16(const ca_gemm_problem *problems, int32_t n_problems, int32_t tile, ca_stream_t stream);
/* The CA_TILE_* value CA_TILE_AUTO resolves to for these problems (> 0), or CA_ERR_ARG. No launch. */
int ca_gemm_auto_tile(const ca_gemm_problem *problems, int32_t n_problems);

/* The same grouped GEMM and epilogues on OCP fp8 (e4m3fn) operands, for the reduced-precision sweep mode
 * (BASELINE.json configs[4]; no counterpart in the reference, which is bf16 throughout -- SURVEY.md 8f-2):
 *   out[m,n] = epi( a_scale[m] * w_scale[n] * sum_k A8[m,k] * W8[n,k] + bias[n] )
 * A8/W8 are e4m3 bytes produced by ca_quantize_rows_fp8 (absmax per row), lda/ldw in elements (= bytes),
 * K % 128 == 0, lda/ldw % 16 == 0; the accumulation is fp32 (v_mfma_scale_f32_16x16x128_f8f6f4 with unit
 * block scales), out/resid/bias/gates stay bf16/fp32 as above.  256x256 ping-pong tile only (N % 256 == 0).
 * e4m3 value range (the consumer's side; the producers' side is at ca_quantize_rows_fp8).  Bytes 0x7F and 0xFF are NaN.
 *   G1  a NaN byte at A8[m, k]: row m is NaN in every column the launch writes (out2 and q_prerope included); every
 *       other row has the bits of the launch with that byte 0.
 *   G2  a NaN byte at W8[n, k]: column n, and the columns the epilogue couples with it (QKV_NORM_ROPE: the 128 columns
 *       of n's head in q or k, and in a normalised q_prerope), are NaN in every row; every other column has those bits.
 *   G3  a_scale[m] = +inf: row m holds no finite element, and NaN where its accumulator is 0; the other rows keep
 *       their bits.
 *   G4  an epilogue result beyond the bf16 range is stored as +-inf (round to nearest even, as torch's fp32 -> bf16
 *       cast), never as NaN or as the largest finite bf16.
 * Limit: the epilogue multiplies the accumulator by a_scale[m] first and by w_scale[n] second, each product rounded to
 * fp32: acc * a_scale[m] can overflow to +-inf where acc * a_scale[m] * w_scale[n] would be finite (a large row scale
 * against a small column scale).  The result is then +-inf, not the finite value.
 */
int ca_gemm_fp8(const ca_gemm_problem *problems, int32_t n_problems, ca_stream_t stream);

/* The launch plan of ca_gemm_bf16 (fp8 = 0, `tile` as there) or ca_gemm_fp8 (fp8 = 1, tile AUTO or PP_256x256) for
 * these problems on a device with n_cu CUs (0 = the current device's, as the launch uses): which kernels run, on which
 * grids.  Same argument checks and return codes as the launch (the pointers are checked, never dereferenced); no
 * launch, and no GPU needed when n_cu > 0.  The launch itself plans through the same code. */
enum { CA_GEMM_KERNEL_NONE = 0,     /* no tile launch: every tile is a thin-row tile */
       CA_GEMM_KERNEL_CLASSIC = 1,  /* ca_gemm_kernel, one workgroup per tile (the CA_TILE_256x* tiles) */
       CA_GEMM_KERNEL_PP = 2,       /* the bf16 ping-pong kernel (the CA_TILE_PP_* tiles) */
       CA_GEMM_KERNEL_PP_FP8 = 3 }; /* its fp8 instantiation */

typedef struct {
  int32_t tile;        /* CA_TILE_* of the launch (AUTO resolved) */
  int32_t kernel;      /* CA_GEMM_KERNEL_* */
  int32_t grid;        /* workgroups of the tile launch (0: none) */
  int32_t persistent;  /* 1: those workgroups walk main_tiles + thin_tiles tiles with a stride of the grid */
  int32_t main_tiles;  /* full-K-loop tiles of the tile launch */
  int32_t thin_tiles;  /* thin last-row tiles walked by the tile launch (at its end, the thin copy of the K loop) */
  int32_t thin_mf;     /* thin-row kernel launched behind it: 16-row fragments per workgroup (2 or 4), 0 = none */
  int32_t thin_nw;     /* its waves per workgroup (1 or 4) */
  int32_t thin_groups; /* its grid rows (grid y) */
  int32_t thin_grid_x; /* its grid columns */
  int32_t n_cu;        /* the CU count the plan was made for (-1: unknown, no persistent walk) */
  int32_t _pad;
} ca_gemm_plan_info;

int ca_gemm_plan(const ca_gemm_problem *problems, int32_t n_problems, int32_t tile, int32_t fp8, int32_t n_cu,
                 ca_gemm_plan_info *out);

/* ------------------------------------------------------------------------------------------
 * Flash attention forward, head_dim 128, no mask:  out = softmax(q k^T * scale) v  per head.
 * Replaces F.scaled_dot_product_attention at modified_double_stream_block.py:112-116 (text+image
 * rows) and :162-168 (concept rows; only the C concept query rows are evaluated, which equals
 * rows [:C] of the reference's (C+L)x(C+L) product), and flux/math.py:6-12 for the single blocks.
 * q/k/v are read in place from a [rows, >=3*H*128] projection buffer: head h of a row lives at
 * column h*128 of the pointer given; the output is written head-concatenated ("B H L D -> B L (H D)",
 * modified_double_stream_block.py:170-176).  The key/value set of a problem is the concatenation
 * of two row segments (segment 1 may be empty), e.g. [concept rows ; image rows].
 * Up to CA_ATTN_MAX_PROBLEMS problems share one launch (per work item of a batch: its text+image rows, and its
 * concept rows); their workgroups are laid out in the order given (put the small concept problems first).
 * The query rows of a problem (and the output rows with them) may themselves come in two row segments: rows
 * [0, nq0) at q / out, rows [nq0, nq) at q1 / out1 -- in a batched forward an item's text rows and image rows are
 * not adjacent.  nq0 = 0 or nq0 = nq: one segment (q1 / out1 unused).
 * Extent limit: the kernels address the key / value rows with unsigned 32-bit byte offsets counted from key 0 over
 * both segments, so (n0 + n1) * ldkv * 2 and 64 * ldkv * 2 must each stay below 2^32 (CA_ERR_ARG "keys larger than
 * 4 GiB" otherwise, nothing is launched).  q, out, out_f32, hm_con and hm_part are addressed in 64 bits: no limit.
 */
#define CA_ATTN_MAX_PROBLEMS 16
typedef struct {
  const void *q; /* bf16, row stride ldq */
  void *out;     /* bf16, row stride ldo */
  const void *k0, *v0; /* segment 0: n0 rows, row stride ldkv */
  const void *k1, *v1; /* segment 1: n1 rows, row stride ldkv */
  float *out_f32; /* optional fp32 copy of the output rows [nq, heads*128] (row stride ldo32; indexed by the
                     problem's row number, also with two query segments), or NULL: used for the C concept rows and,
                     in the layers whose maps are requested, for the image rows, so that the heat-map products
                     (concept_attention_pipeline.py:57-62) see neither side's bf16 rounding */
  const void *q1; /* second query segment (rows nq0..nq-1), row stride ldq; or NULL */
  void *out1;     /* its output rows, row stride ldo */
  const float *hm_con; /* (round 5; pre-scaled-q kernels only) optional fp32 [hm_C, heads*128], row stride ldhc: the C   */
                       /* concept rows' attention outputs of this work item, complete BEFORE this launch starts        */
  float *hm_part;      /* with hm_con: fp32 [heads][nq - nq0][8] -- per head the partial output-space heat-map logits  */
                       /* of the second query segment's rows (the image rows):                                         */
                       /*   hm_part[(head * (nq - nq0) + r) * 8 + c] = <out row nq0 + r of that head, in fp32 before   */
                       /*   its rounding to bf16, hm_con[c, head*128 ..]>                                              */
                       /* i.e. the dot products of concept_attention_pipeline.py:57-61 split by head, formed from the  */
                       /* accumulators instead of an fp32 copy of every row (out_f32: 53 MB per item); summed over the */
                       /* heads and weighted by ca_heatmap_fused (img_f32 = 2)                                         */
  int32_t nq, n0, n1;
  int32_t ldq, ldo, ldkv, ldo32;
  int32_t nq0;    /* query rows in the first segment; 0 or nq = all */
  int32_t hm_C;   /* concepts in hm_con (1..8) */
  int32_t ldhc;   /* row stride of hm_con (elements, % 4 == 0) */
  int32_t _pad;
} ca_attn_problem;

/* scale = the softmax scale (1/sqrt(128) at the reference's call sites), or CA_ATTN_Q_PRESCALED when the q rows were
 * written with softmax_scale * log2(e) already folded in (ca_gemm_problem.q_out_scale): p = exp2(q.k - reference)
 * then costs no multiply per score. */
#define CA_ATTN_Q_PRESCALED 0.0f
int ca_attn_fwd_bf16(const ca_attn_problem *problems, int32_t n_problems, int32_t num_heads,
                     float scale, ca_stream_t stream);
/* ca_attn_fwd_bf16(scale = CA_ATTN_Q_PRESCALED) for q and k rows that hold IEEE half (fp16) instead of bf16 -- written
 * so by the qkv epilogue with ca_gemm_problem.qk_f16 = 1; v, the probabilities and the outputs stay bf16 / fp32.  Used
 * for the layers whose heat maps are requested: the bf16 rounding of the rotated q and k is what bounds the output-
 * space maps (modified_double_stream_block.py:185-191 on :112-116), and an 11-bit mantissa costs the MFMA nothing. */
int ca_attn_fwd_qk16(const ca_attn_problem *problems, int32_t n_problems, int32_t num_heads, ca_stream_t stream);
/* Diagnostics of the pre-scaled-q kernel's two rare paths on the current device, since the last reset:
 * counters[0] = workgroups whose rows were recomputed with a running maximum (a row sum passed 2^100 or
 * overflowed: a score > 100 octaves above its row's first-tile maximum with no check in between, or inf / NaN inputs),
 * counters[1] = in-place re-reference events (per wave: a running row sum passed 2^64 and the reference was moved up).  Both are 0 on the data the
 * reference's synthetic weights produce.  A blocking device-to-host copy: not for the hot path; reset != 0 zeroes them. */
int ca_attn_stats(unsigned long long *counters, int32_t reset);

/* ------------------------------------------------------------------------------------------
 * LayerNorm (no affine, eps) followed by adaLN modulation:  out = (1 + scale) * LN(x) + shift
 * modified_double_stream_block.py:88-89,94-95,100-101,196,199,202; single_stream_block:48;
 * LastLayer flux/modules/layers.py:250-251.  Row ranges may use different modulation vectors
 * (concept rows / text rows / image rows): segment i covers rows [row_end[i-1], row_end[i]).
 */
#define CA_MAX_SEGMENTS 16
typedef struct {
  int32_t row_end;
  int32_t _pad;
  const float *shift; /* fp32 [H] */
  const float *scale; /* fp32 [H] */
} ca_mod_segment;

int ca_ln_modulate_bf16(const void *x, int32_t ldx, void *out, int32_t ldo, int32_t M, int32_t H,
                        const ca_mod_segment *segs, int32_t n_segs, float eps, ca_stream_t stream);
/* The same two with an fp32 input x (row stride ldx elements, % 4 == 0): the residual stream kept in fp32
 * (its per-block bf16 rounding is what makes the heat-map error grow with depth). */
int ca_ln_modulate_f32in(const float *x, int32_t ldx, void *out, int32_t ldo, int32_t M, int32_t H,
                         const ca_mod_segment *segs, int32_t n_segs, float eps, ca_stream_t stream);
/* ca_ln_modulate_fp8 (below) with the fp32 input: the same e4m3 output, scale rule and value range (P1 .. P5 at
 * ca_quantize_rows_fp8), y being the modulated row in fp32. */
int ca_ln_modulate_f32in_fp8(const float *x, int32_t ldx, void *out8, int32_t ldo, float *out_scale, int32_t M,
                             int32_t H, const ca_mod_segment *segs, int32_t n_segs, float eps, ca_stream_t stream);
/* ca_ln_modulate_f32in with a second bf16 plane out_lo = bf16(y - float(bf16(y))) (row stride ldlo): what the bf16
 * rounding of the modulated row y drops.  out + out_lo carry y to ~16 mantissa bits. */
int ca_ln_modulate_f32in_split(const float *x, int32_t ldx, void *out, int32_t ldo, void *out_lo, int32_t ldlo,
                               int32_t M, int32_t H, const ca_mod_segment *segs, int32_t n_segs, float eps,
                               ca_stream_t stream);
/* Same, with the result quantised for ca_gemm_fp8: out8 = e4m3 bytes (row stride ldo bytes, % 16),
 * out_scale[row] = absmax(row) / 448 (fp32 [M]).  Value range: P1 .. P5 at ca_quantize_rows_fp8, with y the modulated
 * row (1 + scale) * LayerNorm(x) + shift in fp32.  A NaN or an infinity in x makes the whole row NaN (bytes NaN, scale
 * 1); a NaN in one column of a segment's shift or scale is a NaN byte in that column of that segment's rows only. */
int ca_ln_modulate_fp8(const void *x, int32_t ldx, void *out8, int32_t ldo, float *out_scale, int32_t M,
                       int32_t H, const ca_mod_segment *segs, int32_t n_segs, float eps, ca_stream_t stream);
/* Row-wise absmax quantisation bf16 [M,K] -> e4m3 [M,K] + fp32 scale per row (weights once per model;
 * activations between two fp8 GEMMs).
 * e4m3 value range, for this entry and the four other e4m3 producers (ca_ln_modulate_fp8, ca_ln_modulate_f32in_fp8,
 * ca_t5_rmsnorm_f32in_fp8, ca_gated_mul_fp8).  y is the fp32 row the producer quantises (here: x), amax the largest |y|
 * over the row's non-NaN elements, out_scale = max(amax * fl(1 / 448), 2^-126), or 1 where amax is 0, and
 * out8[c] = e4m3(clamp(y[c] * (1 / out_scale), +-448)), round to nearest even.
 *   P1  a finite row with amax * fl(1 / 448) >= 2^-126: as stated, the bytes and scales the entries have always written.
 *   P2  y[c] NaN (either sign, any payload, quiet or signalling): out8[c] is an e4m3 NaN (0x7F or 0xFF), never a
 *       finite byte.
 *   P3  the scale ignores NaN elements: out_scale and every other byte of the row are those of the same row with its NaN
 *       elements set to 0, bit for bit; a row that is all NaN has scale 1.
 *   P4  a row with +-inf in y: out_scale = +inf, NaN bytes at the infinite positions (inf * (1 / inf)), +-0 with the
 *       element's sign at the finite ones.  This covers a gated product that overflows fp32.
 *   P5  a finite non-zero row: out_scale is finite, positive and normal and every byte is finite, however small the
 *       row; below amax / 448 = 2^-126 the scale is 2^-126 (1 / out_scale stays finite; without the floor it was inf,
 *       every non-zero element +-448 and every zero 0 * inf).
 * A special row changes no other row. */
int ca_quantize_rows_fp8(const void *x, int32_t ldx, void *out8, int32_t ldo, float *out_scale, int32_t M,
                         int32_t K, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * QK-RMSNorm + RoPE, in place on the q and k thirds of a [M, 3*H*128] projection buffer.
 * QKNorm: flux/modules/layers.py:63-84 (fp32, eps 1e-6, per-head scale[128]);
 * apply_rope: flux/math.py:25-30 (interleaved pairs (2i,2i+1)); rope table [M,64,2] fp32 =
 * (cos,sin) of rope() flux/math.py:15-22 computed by the host in float64.
 * Optionally stores the normalised, PRE-RoPE q (what the reference captures as
 * cross_attention_{image,concept}_vectors, modified_double_stream_block.py:189-190) to q_prerope.
 */
typedef struct {
  int32_t row_end;
  int32_t _pad;
  const void *q_scale; /* bf16 [128] */
  const void *k_scale; /* bf16 [128] */
} ca_norm_segment;

int ca_qknorm_rope_bf16(void *qkv, int32_t ld, int32_t M, int32_t num_heads,
                        const ca_norm_segment *segs, int32_t n_segs, const float *rope_cos_sin,
                        void *q_prerope, int32_t ldp, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Small-batch matrix-vector products (weight streaming, HBM-bound):
 *   out[v,n] (+)= sum_k f(x[v,k]) * W[n,k] + bias[n],  v < nv <= 8,  f = SiLU or identity.
 * Modulation (flux/modules/layers.py:113-126), MLPEmbedder (:52-60), LastLayer.adaLN (:246,249).
 */
int ca_gemv_bf16(const float *x, int32_t nv, int32_t ldx, const void *W, const void *bias, float *out,
                 int32_t ldo, int32_t N, int32_t K, int32_t silu_input, int32_t accumulate,
                 ca_stream_t stream);

/* Cross-attention-space query vectors (post-QKNorm, pre-RoPE q; modified_double_stream_block.py:189-190) from the
 * UNROUNDED LayerNorm output: x fp32 [M, heads*128] = the q projection of bf16(y) before its norm (ca_gemm_problem
 * qpre_f32 = 2), d fp32 (or NULL) = the same weights applied to the low plane of ca_ln_modulate_f32in_split;
 * in place  x <- RMSNorm_128(x + d) * norm_scale  per head (flux/modules/layers.py:63-72).  The rounding of the
 * GEMM operand is ~90 % of the cross-space heat-map error of a bf16 MFMA path. */
int ca_qpre_finish_f32(float *x, int32_t ldx, const float *d, int32_t ldd, const void *norm_scale, int32_t M,
                       int32_t heads, ca_stream_t stream);
/* The same, and with q_out != NULL the normalised vector is also rotated (rope fp32 [M,64,2] for these rows:
 * apply_rope, flux/math.py:25-30), multiplied by q_out_scale (0 = 1) and stored as 2-byte elements (bf16, or IEEE half
 * with q_f16 = 1; row stride ldq elements) -- i.e. it REPLACES the attention's q rows that the qkv epilogue formed from
 * bf16(y) by the ones formed from the unrounded y.  The bf16 rounding of that GEMM operand, through q, is what bounds a
 * single output-space heat map (modified_double_stream_block.py:112-116 feeding :185-188): 7.7e-4 of 7.8e-4. */
int ca_qpre_finish_rope_f32(float *x, int32_t ldx, const float *d, int32_t ldd, const void *norm_scale,
                            const float *rope, void *q_out, int32_t ldq, float q_out_scale, int32_t q_f16,
                            int32_t M, int32_t heads, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Concept heat maps, one (timestep, layer) at a time (compute_heatmaps_from_vectors,
 * concept_attention/concept_attention_pipeline.py:29-91, softmax branch):
 *   logits[c,p] = <img_vec[p,:], con_vec[c,:]>                                   (:57-61)
 *   acc[c,p]   += weight * softmax_c(logits[:,p])        (weight = 1/(|timesteps|*|layers|), :64-82)
 * fp32 accumulation (the reference does this in bf16; see DESIGN.md "tolerance").
 */
/* con_is_f32 is a bit set: bit 0 = con_vec is fp32 [C,dim] (else bf16), bit 1 = img_vec is fp32 [L,dim] (else bf16;
 * needs bit 0 as well); ldi / ldc in elements, multiples of 8 / 4. */
int ca_heatmap_logits_bf16(const void *img_vec, int32_t ldi, const void *con_vec, int32_t ldc,
                           int32_t con_is_f32, int32_t L, int32_t C, int32_t dim, float *logits,
                           ca_stream_t stream);
int ca_heatmap_softmax_accumulate(const float *logits, int32_t C, int32_t L, float weight, float *acc,
                                  ca_stream_t stream);
/* The same accumulation with the other two weightings across concepts the reference offers
 * (`attention_norm`, concept_attention_pipeline.py:33,64-71): norm = CA_NORM_SOFTMAX (as above),
 * CA_NORM_SPARSEMAX or CA_NORM_ENTMAX15.  The reference takes the latter two from the third-party `entmax`
 * package, which it neither pins nor vendors: they are implemented here from the published algorithms
 * (Martins & Astudillo 2016; Peters, Niculae & Martins 2019) and their parity with that package is UNPINNED.
 * The sparse norms need C <= CA_HEATMAP_MAX_CONCEPTS. */
#define CA_NORM_SOFTMAX 0
#define CA_NORM_SPARSEMAX 1
#define CA_NORM_ENTMAX15 2
int ca_heatmap_norm_accumulate(const float *logits, int32_t C, int32_t L, int32_t norm, float weight, float *acc,
                               ca_stream_t stream);

/* The three steps above for up to CA_HEATMAP_MAX_PROBLEMS (work item, space) pairs of one layer in ONE launch
 * (round 5): per problem  logits[c,p] = <img_vec[p,:], con_vec[c,:]>  for all C concepts of a patch in one pass over
 * the image vectors, then  acc[c,p] += weight * norm_c(logits[:,p])  and, if acc2 != NULL,
 * acc2[c,p] += weight2 * norm_c(logits[:,p])  (the per-layer table row of the per-layer x noise-level sweep,
 * experiments/per_layer_segmentation/test_segmentations_per_layer.py:104-114); the logits never reach memory unless
 * `logits` != NULL.  Per patch and concept the arithmetic is that of ca_heatmap_logits_bf16 followed by
 * ca_heatmap_norm_accumulate (same k order, same expressions): the results are bit-identical to the three-launch form.
 * All problems of a call share L, C, dim and norm, and no two of them may name the same accumulator (the updates are
 * plain read-modify-writes by different workgroups).  Needs C <= 8 and C * dim * 4 bytes of LDS (<= 96 KB);
 * CA_ERR_ARG otherwise (the caller then uses the three-launch form). */
#define CA_HEATMAP_MAX_PROBLEMS 16
typedef struct {
  const void *img_vec; /* [L, dim] bf16, or fp32 if img_f32 = 1; row stride ldi elements (% 8 bf16, % 4 fp32).        */
                       /* img_f32 = 2: instead fp32 [ldi heads][L][8], the per-head partial logits an attention       */
                       /* launch left in ca_attn_problem.hm_part: logits[c,p] = their sum over the heads in head      */
                       /* order; con_vec is then unused (may be NULL)                                                 */
  const void *con_vec; /* [C, dim] bf16, or fp32 if con_f32; row stride ldc elements */
  float *acc;          /* fp32 [C, L] contiguous, or NULL */
  float *acc2;         /* fp32 [C, L] contiguous, or NULL */
  float *logits;       /* fp32 [C, L] contiguous, or NULL: the raw logits as well */
  int32_t ldi, ldc;
  int32_t img_f32, con_f32;
  float weight, weight2;
} ca_heatmap_problem;
int ca_heatmap_fused(const ca_heatmap_problem *problems, int32_t n_problems, int32_t L, int32_t C, int32_t dim,
                     int32_t norm, ca_stream_t stream);

/* Most concepts of one patch the heat-map kernels weight: the sparse norms of ca_heatmap_norm_accumulate, and the
 * library's one-launch-per-layer form for more than 8 concepts (exported and bound by conceptattention_amd/_lib.py, declared
 * in conceptattention_amd/csrc/ca_heatmap_core.h; not part of this header yet). */
#define CA_HEATMAP_MAX_CONCEPTS 32

/* Sinusoidal timestep embedding (timestep_embedding, flux/modules/layers.py:28-49):
 * out[v, 0:dim/2] = cos(time_factor*t[v]*f_i), out[v, dim/2:] = sin(...), f_i = max_period^(-i/(dim/2)). */
/* (nt * dim / 2 is formed in 64 bits: no limit below int32 nt and dim) */
int ca_timestep_embedding_f32(const float *t, int32_t nt, float *out, int32_t dim, float time_factor,
                              float max_period, ca_stream_t stream);

/* Euler step of denoise(): x = x + a*y  (flux/sampling.py:141), bf16 in/out, fp32 math. */
int ca_axpy_bf16(void *x, const void *y, float a, int64_t n, ca_stream_t stream);
/* The same update with the latent kept in fp32 between the steps: x fp32 [n] += a * y (y bf16 [n], or fp32 [n] if
 * y_is_f32: the model's prediction unrounded).  The reference's loop (flux/sampling.py:141 on bf16 tensors) re-rounds
 * the running latent after every step -- 2^-9 relative each time, accumulating; on this path the model's img_in then
 * takes the fp32 value as two bf16 planes (ca_split_bf16). */
int ca_axpy_f32(float *x, const void *y, int32_t y_is_f32, float a, int64_t n, ca_stream_t stream);
/* x fp32 [rows, K] (row stride ldx) -> hi = bf16(x), lo = bf16(x - hi) (row stride ldo), K % 4 == 0: the two planes of
 * a GEMM operand that must not lose its low bits (ca_silu_split_bf16 without the silu): the latent into img_in
 * (modified_flux_dit.py:98). */
int ca_split_bf16(const float *x, int32_t ldx, void *hi, void *lo, int32_t ldo, int32_t rows, int32_t K, ca_stream_t stream);

/* silu(x) of the conditioning vectors (Modulation: lin(silu(vec)), flux/modules/layers.py:113-126) split into two
 * bf16 planes, hi = bf16(s), lo = bf16(s - hi): hi + lo carries s to ~16 mantissa bits, so that the adaLN modulation
 * of every block -- [2 * items * steps, H] x [sum N, H]^T, the weights streamed ONCE -- can run as two bf16 MFMA GEMMs
 * (ca_gemm_bf16, the second one accumulating) instead of one weight pass per 4 vectors (ca_gemv_bf16).
 * x fp32 [rows, K] (row stride ldx), hi / lo bf16 [rows, K] (row stride ldo), K % 4 == 0.  Element indices and row
 * offsets are 64-bit in both split entry points: no limit below int32 rows, K and strides. */
int ca_silu_split_bf16(const float *x, int32_t ldx, void *hi, void *lo, int32_t ldo, int32_t rows, int32_t K,
                       ca_stream_t stream);

/* The two planes' products of a single-pass modulation GEMM ([hi; lo] stacked as 2*nv rows, no bias) folded into the
 * modulation: out[v,n] = (pair[v,n] + bias[n]) + pair[nv + v,n] -- the roundings of the two-launch form (first GEMM
 * with bias, second one accumulating), so both forms give the same bits.  pair fp32 [2*nv, N] (row stride ldp),
 * bias bf16 [N] or NULL, out fp32 [nv, N] (row stride ldo), N % 4 == 0. */
int ca_modulation_combine_f32(const float *pair, int32_t ldp, const void *bias, float *out, int32_t ldo, int32_t nv,
                              int32_t N, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Flux autoencoder (concept_attention/flux/src/flux/modules/autoencoder.py).  Activations are NHWC: a pixel is a row of
 * channels with a free row stride; every element offset is formed in 64 bits (a 1024 x 1024 fp32 activation of 256
 * channels is 1 GiB).
 *
 * Implicit-GEMM convolution on v_mfma_f32_16x16x32_bf16, fp32 accumulation:
 *   out[b, oy, ox, n] = bias[n] + sum_{ky, kx, c} x[b, sy, sx, c] * w[n, (ky * ksize + kx) * Cin + c]  (+ resid)
 * One kernel for every nn.Conv2d of the encoder and decoder:
 *   ksize 3, stride 1            padding 1 (ResnetBlock :63-65, conv_in / conv_out :126,157,208,235)
 *   ksize 3, stride 2            the (0,1,0,1) zero padding of Downsample (:85-95): Ho = (Hin - 2) / 2 + 1
 *   ksize 3, stride 1, upsample  the nearest 2x of Upsample (:98-106) folded into the index: (sy, sx) = (iy >> 1,
 *                                ix >> 1), Ho = 2 Hin; no upsampled tensor exists
 *   ksize 1                      nin_shortcut (:66-67)
 * Padding pixels are zeros by predicate.  x: bf16 [B, Hin, Win, ldx], Cin % 32 == 0 channels read per pixel (a
 * narrower tensor -- the 16-channel latent, the 3-channel image -- sits in a zero-padded row: ldx >= Cin, ldx % 8 == 0).
 * w: bf16 [ceil16(Cout), ksize * ksize * Cin], tap-major and K-contiguous, zero rows / columns for the padding.
 * bias: fp32 [Cout] or NULL.  resid: fp32 [pixels, ldr] or NULL, added in the epilogue; may alias an fp32 out.
 * out: fp32 (out_f32) or bf16 [pixels, ldo], Cout channels stored per pixel.
 */
int ca_conv3x3_nhwc(const void *x, const void *w, const float *bias, const float *resid, void *out, int32_t B,
                    int32_t Hin, int32_t Win, int32_t Cin, int32_t Cout, int32_t ldx, int32_t ldr, int32_t ldo,
                    int32_t ksize, int32_t stride, int32_t upsample, int32_t out_f32, ca_stream_t stream);

/* nn.GroupNorm(32, C, eps, affine) with optional swish (autoencoder.py:21-22,30,62,64,156,234): x fp32 (x_f32) or bf16
 * [B, HW, ldx], y bf16 [B, HW, ldy], gamma / beta fp32 [C]; C a power of two in 32..1024.  Two launches: per-chunk
 * (count, mean, M2) of every group by Welford / Chan into part (fp32 [B, n_chunks, 32, 3], caller's scratch), then the
 * merge and the apply.  The variance is never formed as a difference of two large sums. */
int ca_groupnorm_nhwc(const void *x, int32_t x_f32, int32_t ldx, const float *gamma, const float *beta, void *y,
                      int32_t ldy, int32_t B, int64_t HW, int32_t C, float eps, int32_t swish, float *part,
                      int32_t n_chunks, ca_stream_t stream);

/* p[r, 0:n] = softmax(scale * s[r, 0:n]) as bf16, p[r, n:ldp] = 0: the probabilities of the one-head attention of
 * AttnBlock (autoencoder.py:47) between its two GEMMs; any n. */
int ca_softmax_rows_f32(const float *s, int32_t lds, void *p, int32_t ldp, int32_t rows, int32_t n, float scale,
                        ca_stream_t stream);

/* out[r, c] = a * (x[r, c] + exp(0.5 * logvar[r, c]) * noise[r, c]) + b for c < C; logvar and noise both given or both
 * NULL.  DiagonalGaussian and the scale / shift of AutoEncoder (autoencoder.py:262-309); with a = 1, b = 0 the cast of an
 * fp32 tensor to a bf16 convolution operand.  out fp32 (out_f32) or bf16, row stride ldo; columns >= C are not written. */
int ca_affine_rows_f32(const float *x, int32_t ldx, const float *logvar, int32_t ldl, const float *noise, int32_t ldn,
                       void *out, int32_t ldo, int32_t out_f32, int64_t rows, int32_t C, float a, float b,
                       ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * T5 encoder (transformers' modeling_t5.py, encoder side, as flux/modules/conditioner.py:6-38 loads and calls it:
 * every string padded to max_length, attention_mask = None, so padding tokens take part in attention).  The q / k / v /
 * o and wi / wo projections run on ca_gemm_bf16; the kernels below are the rest of a block.
 *
 * T5Attention.forward: scores = q k^T (NO 1 / sqrt(d) scale) + position_bias; softmax in fp32; out = P v.
 * q, k, v: bf16 [n_seq * L, heads * 64] views with free row strides (column slices of one fused projection output);
 * head h at columns h * 64.  bias: fp32 [heads, 2 L - 1], bias[h, key_pos - query_pos + L - 1] =
 * relative_attention_bias[bucket(key_pos - query_pos), h], built by the caller.  out: bf16, same form.  Scores, softmax
 * and the P v accumulation are fp32; P is rounded to bf16 (unnormalised, in (0, 1]) only as an MFMA operand.
 * L % 64 == 0, 64 <= L <= 512, heads >= 1, n_seq >= 1, n_seq * heads * L / 64 workgroups < 2^31; row strides % 8;
 * q, k, v, out 16-byte aligned.  One launch. */
int ca_t5_attn_bf16(const void *q, const void *k, const void *v, const float *bias, void *out, int32_t ldq, int32_t ldk,
                    int32_t ldv, int32_t ldo, int32_t n_seq, int32_t heads, int32_t L, ca_stream_t stream);

/* T5LayerNorm.forward: out[r, :] = bf16(x[r, :] * rsqrt(mean(x[r, :]^2) + eps) * w[:]) -- no mean subtraction, no bias.
 * x fp32 [rows, ldx] (the residual stream), w fp32 [H], out bf16 [rows, ldo]; H % 4 == 0, ldx / ldo >= H and % 4. */
int ca_t5_rmsnorm_f32in(const float *x, int32_t ldx, const float *w, void *out, int32_t ldo, int64_t rows, int32_t H,
                        float eps, ca_stream_t stream);

/* T5DenseGatedActDense.forward: out = bf16(float(g) * float(u)) with g = gelu_new(wi_0 x) (the out2 of a
 * CA_EPI_SPLIT_GELU launch on the stacked [wi_1 ; wi_0] weight) and u = wi_1 x.  bf16 rows of C columns, C % 8 == 0,
 * row strides >= C and % 8, 16-byte aligned. */
int ca_gated_mul_bf16(const void *g, int32_t ldg, const void *u, int32_t ldu, void *out, int32_t ldo, int64_t rows,
                      int32_t C, ca_stream_t stream);

/* The two above as producers of ca_gemm_fp8's A operand (the T5 encoder's fp8 mode): the fp32 row y (the norm's
 * x * rsqrt(mean(x^2) + eps) * w, not rounded to bf16; the exact product float(g) * float(u)) leaves as OCP e4m3 bytes
 * and one fp32 scale per row: out_scale[r] = max|y| / 448, or 1 for an all-zero row (which stores zero bytes);
 * out8[r, :] = e4m3(y / out_scale[r]), round-to-nearest-even, saturating at +-448 -- the rule of ca_quantize_rows_fp8,
 * with its value range (P1 .. P5 there).  ca_t5_rmsnorm_f32in_fp8: a NaN in x makes the whole row NaN (bytes NaN, scale
 * 1); an inf in x makes rsqrt(...) 0, so y is inf * 0 = NaN in that column and x * 0 elsewhere (scale 1); a NaN or inf
 * in w[c] is a NaN or inf y[c] in every row.  ca_gated_mul_fp8: a NaN factor is a NaN y[c]; an infinite factor, or
 * finite factors whose product overflows fp32, an infinite y[c] (P4); a product that underflows to 0 counts as 0.
 * out8 uint8 [rows, ldo] with ldo in bytes, >= the row length and % 8 (ca_gemm_fp8 itself wants lda % 16), 8-byte
 * aligned; out_scale fp32 [rows] contiguous.  H % 8 == 0 / C % 8 == 0; inputs as for the bf16 forms (x, w, g, u
 * 16-byte aligned, ldx % 4, ldg / ldu % 8).  One workgroup owns a row. */
int ca_t5_rmsnorm_f32in_fp8(const float *x, int32_t ldx, const float *w, void *out8, int32_t ldo, float *out_scale,
                            int64_t rows, int32_t H, float eps, ca_stream_t stream);
int ca_gated_mul_fp8(const void *g, int32_t ldg, const void *u, int32_t ldu, void *out8, int32_t ldo, float *out_scale,
                     int64_t rows, int32_t C, ca_stream_t stream);

/* nn.Embedding into the fp32 residual stream: out[r, :] = float(table[ids[r], :]).  table bf16 [vocab, ldt], ids int32
 * [rows] on the device, out fp32 [rows, ldo]; H % 8 == 0.  The library cannot see the ids: the caller guarantees
 * 0 <= ids[r] < vocab (the Python wrapper checks before the launch). */
int ca_embed_rows_f32(const void *table, int32_t ldt, const int32_t *ids, float *out, int32_t ldo, int64_t rows,
                      int32_t H, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CLIP text encoder (transformers' modeling_clip.py, CLIPTextModel, as flux/modules/conditioner.py loads and calls it:
 * every string padded to 77 tokens, attention_mask = None, so the mask is causal only and padding tokens are keys like
 * any other).  The q|k|v, out_proj, fc1 and fc2 projections run on ca_gemm_bf16; the kernels below are the rest.
 *
 * CLIPAttention.forward: out = softmax(scale * q k^T + causal mask) v per (sequence, head), head dim 64.  q, k, v, out:
 * bf16 [n_seq * L, heads * 64] views with free row strides (column slices of one fused projection output); head h at
 * columns h * 64; sequence s owns rows s * L .. s * L + L - 1; a query at position i sees keys 0 .. i.  Scores, softmax
 * and the P v accumulation are fp32; P is rounded to bf16 (unnormalised, in [0, 1]) only as an MFMA operand.
 * 1 <= L <= 128, any value: a sequence need not fill a tile.  No row at or beyond n_seq * L is read or written (the
 * places of such rows in the last tile hold zeros).  heads >= 1, n_seq >= 1, scale > 0 and finite; row strides
 * >= heads * 64 and % 8; q, k, v, out 16-byte aligned.  One launch. */
int ca_clip_attn_bf16(const void *q, const void *k, const void *v, void *out, int32_t ldq, int32_t ldk, int32_t ldv,
                      int32_t ldo, int32_t n_seq, int32_t heads, int32_t L, float scale, ca_stream_t stream);

/* nn.LayerNorm on the fp32 stream: out[r, :] = bf16((x[src, :] - mean) * rsqrt(var + eps) * w[:] + b[:]), var the biased
 * variance about the mean, statistics in fp32; src = row_idx ? row_idx[r] : r (int32 on the device; the caller
 * guarantees 0 <= row_idx[r] < the rows of x).  x fp32 [*, ldx], w and b fp32 [H], out bf16 [rows, ldo]; H % 4 == 0,
 * ldx / ldo >= H and % 4. */
int ca_layernorm_f32in(const float *x, int32_t ldx, const int32_t *row_idx, const float *w, const float *b, void *out,
                       int32_t ldo, int64_t rows, int32_t H, float eps, ca_stream_t stream);

/* quick_gelu: out = bf16(x * sigmoid(1.702 x)), computed in fp32; bf16 rows of C columns, C % 8 == 0, row strides >= C
 * and % 8, 16-byte aligned; out may be x.  Finite for every finite x; -inf gives -0, +inf gives +inf, NaN stays NaN. */
int ca_quick_gelu_bf16(const void *x, int32_t ldx, void *out, int32_t ldo, int64_t rows, int32_t C, ca_stream_t stream);

/* CLIPTextEmbeddings: out[r, :] = float(tok[ids[r], :]) + float(pos[r % L, :]), one fp32 addition.  tok bf16
 * [vocab, ldt], pos bf16 [>= L, ldp], ids int32 [rows] on the device, out fp32 [rows, ldo]; H % 8 == 0, 1 <= L <= 128.
 * The library cannot see the ids: the caller guarantees 0 <= ids[r] < vocab (the Python wrapper checks). */
int ca_clip_embed_f32(const void *tok, int32_t ldt, const void *pos, int32_t ldp, const int32_t *ids, float *out,
                      int32_t ldo, int64_t rows, int32_t L, int32_t H, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pixel I/O of the autoencoder: image bytes in, image bytes out, with no fp32 image tensor in between.
 *
 * One image into one slot of the zero-padded input plane of encoder.conv_in, resized with the index rule of
 * torch.nn.functional.interpolate(mode="nearest"):
 *   dst[y, x, c] = bf16_rne(2.0f * (float(src[sy, sx, c]) / 255.0f) - 1.0f) for c < 3, dst[y, x, 3..31] = 0,
 *   sy = min((int)floorf(y * ((float)H0 / H)), H0 - 1), sx likewise; the division by 255 correctly rounded.
 * src: uint8 [H0, W0, 3], rows src_stride BYTES apart (>= 3 W0; unused when H0 = 1); dst: bf16 [H, W, 32], 16-byte aligned.  Bit-identical
 * to float() / 255, 2 x - 1, interpolate and the bf16 cast of ca_affine_rows_f32.  One launch per image. */
int ca_pixels_u8_to_nhwc32_bf16(const void *src, int64_t src_stride, void *dst, int32_t H0, int32_t W0, int32_t H,
                                int32_t W, ca_stream_t stream);

/* The decoder's NHWC output to bytes: dst[p, c] = (uint8)truncf(127.5f * (min(max(src[p, c], -1), 1) + 1.0f)) for c < 3,
 * the sum and the product rounded separately: (127.5 * (img.clamp(-1, 1) + 1.0)).byte().  A NaN gives 0.  src: fp32
 * [pixels, ld >= 3]; dst: uint8 [pixels, 3], 16-byte aligned; pixels counts every pixel of the batch. */
int ca_nhwc_f32_to_pixels_u8(const float *src, int32_t ld, void *dst, int64_t pixels, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation scoring (experiments/imagenet_segmentation/run_experiment.py:166-222 with batch_pix_accuracy,
 * batch_intersection_union and get_ap_scores of concept_attention/utils.py:48-108; the mean-threshold mask of
 * concept_attention/segmentation.py:55-81): one workgroup per item scores the target concept's heat map against a
 * label image without leaving the device.  Per item, every step one fp32 rounding unless it says fp64:
 *   x     = map, or with CA_SEG_BLUR its 3x3 blur with reflect padding: the nine products blur_weights[3 i + j] *
 *           map[y + i - 1, x + j - 1], each rounded, added in row-major order
 *   lo, hi = min x, max x;  mean = (float)(fp64 sum of x / (h w))   (a fixed summation tree)
 *   mask  = x > mean  with CA_SEG_MEAN_THRESHOLD, else x > 0
 *   c     = (x - lo) / (hi - lo), the division correctly rounded; a constant map gives NaN, as on the host
 *   label pixel (Y, X) reads the mask at cell (near(Y; Hl, h), near(X; Wl, w)) and the coefficient at the same cell,
 *   or with CA_SEG_DOWNSCALE at (near(near(Y; Hl, 14); 14, h), near(near(X; Wl, 14); 14, w));
 *   near(i; n_out, n_in) = min((int)floorf(i * ((float)n_in / (float)n_out)), n_in - 1), the rule of
 *   torch.nn.functional.interpolate(mode="nearest")
 *   n11, n10, n01, n00 = pixels by (mask, label != 0)
 *   ap    = the average precision of the 2 Hl Wl stacked scores (1 - c, c) (NaN -> 0) against the one-hot label:
 *           sum over the distinct scores, descending, of (R_k - R_{k-1}) P_k with P_k = tp_k / n_k and
 *           R_k = tp_k / (Hl Wl) in fp64, tp_k and n_k exact integers; the sum over a fixed tree (the same bits
 *           every run)
 * All problems of a call share h, w, Hl, Wl and flags.  Limits: 1 <= h w <= 4096, 1 <= Hl Wl <= 2^24,
 * 1 <= n_problems <= CA_SEG_MAX_PROBLEMS, CA_SEG_BLUR needs h, w >= 2 and blur_weights (nine floats on the HOST, read
 * during the call; unused and may be NULL otherwise); CA_ERR_ARG otherwise.  Needs up to 112.5 KB of LDS. */
#define CA_SEG_MAX_PROBLEMS 16
#define CA_SEG_MEAN_THRESHOLD 1
#define CA_SEG_DOWNSCALE 2
#define CA_SEG_BLUR 4
typedef struct {
  const float *map;   /* fp32 [h, w] contiguous: the target concept's accumulated heat map                             */
  const void *label;  /* uint8 [Hl, Wl] contiguous: nonzero = positive                                                 */
  void *result;       /* one ca_seg_record, 40 bytes, 8-byte aligned                                                    */
  void *mask_out;     /* uint8 [h, w], or NULL: the mask at map resolution (0 / 1)                                     */
  float *coeff_out;   /* fp32 [h, w], or NULL: c at map resolution                                                     */
} ca_seg_problem;
typedef struct {
  int32_t n11, n10, n01, n00;
  double ap;
  float mean, lo, hi;
  int32_t thresholds; /* the number of distinct scores among the pixels */
} ca_seg_record;
int ca_seg_score(const ca_seg_problem *problems, int32_t n_problems, int32_t h, int32_t w, int32_t Hl, int32_t Wl,
                 int32_t flags, const float *blur_weights, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-class segmentation scoring (experiments/pascal_voc_segmentation/multi_class_segmentation.py:58-79 and
 * run_multi_class_seg_experiment.py:25-37, 194-233): one workgroup per item takes the argmax over the item's K
 * accumulated maps, maps the winning concept to its class and counts the class map against a label image of class ids,
 * without leaving the device.  Per item, every step one fp32 rounding:
 *   x_k   = plane k, or with CA_MSEG_BLUR its 3x3 blur with reflect padding exactly as seg_score forms it: the nine
 *           products blur_weights[3 i + j] * plane[y + i - 1, x + j - 1], each rounded, added in row-major order
 *   s_k   = scale[k] * x_k when scale is given, else x_k        (the harness's unimplemented concept_scale_values)
 *   index[cell] = torch.argmax over k: plane k replaces the running best iff s_k > best, or s_k is NaN and best is
 *           not; so the first index of the maximum wins, -0.0 == 0.0, and the first NaN beats every number
 *   class[cell] = class_of[item][index[cell]]
 *   label pixel (Y, X) reads cell (near(Y; Hl, h), near(X; Wl, w)), the near of seg_score
 *   over the label pixels with label != ignore_index (ignore_index = -1: none are skipped):
 *     labelled = their number;  correct = those with class == label;
 *     inter[c] = pixels with class == label == c;  union[c] = pixels with class == c or label == c, for c < nclass
 *   a label value >= nclass that is not ignored counts as labelled, is never correct and enters only the union of the
 *   predicted class (VOC's 255 border in lines 207-222 of the harness).  All counts are exact integers.
 * All problems of a call share K, h, w, Hl, Wl, nclass, ignore_index, flags and scale.  class_of: uint8
 * [n_problems][K], the class id of every concept of every item, required, every entry < nclass; scale: float [K] or
 * NULL; blur_weights: float [9], required with CA_MSEG_BLUR.  All three are HOST arrays, read during the call; nothing
 * is uploaded, allocated or retained.  Limits: 1 <= K <= 32, 1 <= h w <= 16384, 1 <= Hl Wl <= 2^24, 1 <= nclass <= 256,
 * -1 <= ignore_index <= 255, 1 <= n_problems <= 16, CA_MSEG_BLUR needs h, w >= 2, no other flag bit; CA_ERR_ARG
 * otherwise, before any launch.  Needs 18 KB of LDS. */
#define CA_MSEG_MAX_PROBLEMS 16
#define CA_MSEG_MAX_CONCEPTS 32
#define CA_MSEG_MAX_CLASSES 256
#define CA_MSEG_MAX_CELLS 16384
#define CA_MSEG_BLUR 4
typedef struct {
  const float *maps;  /* fp32 [K, h, w] contiguous: the item's accumulated maps, concept-major            */
  const void *label;  /* uint8 [Hl, Wl] contiguous: class ids                                              */
  void *counts;       /* int32 [2 + 2 nclass], 8-byte aligned: correct, labelled, inter[nclass], union[..] */
  void *class_out;    /* uint8 [h, w] or NULL: the predicted class per map cell                            */
  void *index_out;    /* uint8 [h, w] or NULL: the winning concept index per map cell                      */
} ca_mseg_problem;
int ca_mseg_score(const ca_mseg_problem *problems, int32_t n_problems, int32_t K, int32_t h, int32_t w,
                  int32_t Hl, int32_t Wl, int32_t nclass, int32_t ignore_index, int32_t flags,
                  const void *class_of, const float *scale, const float *blur_weights, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation scoring of a TABLE of maps against one label (the per-layer and per-timestep sweeps:
 * experiments/per_layer_segmentation/test_segmentations_per_layer.py:164-243 and
 * experiments/per_timestep_segmentation/test_segmentations_per_time.py:75-174): n_maps heat maps of one geometry, one
 * ca_seg_record each, from two launches.  A label pass counts once, per map cell, the label pixels that read the cell
 * and the positive ones among them, for the mask's pixel -> cell mapping and for the coefficient's; a map pass, one
 * workgroup per map, forms the record from the map and those tables and never reads the label.  Per map, every step
 * one fp32 rounding unless it says fp64, all of it as seg_score states it:
 *   x     = map, or with CA_SEGTAB_BLUR its 3x3 blur with reflect padding (nine rounded products, row-major order)
 *   lo, hi = min x, max x (NaN cells are skipped);  mean = (float)(fp64 sum of x / (h w)), seg_score's fixed tree
 *   mask  = x > mean  with CA_SEGTAB_MEAN_THRESHOLD, else x > 0
 *   c     = (x - lo) / (hi - lo), the division correctly rounded; with CA_SEGTAB_RAW c = x (the per-layer script
 *           scores the raw coefficients, lines 209-215)
 *   label pixel (Y, X) reads the mask at cell (near(Y; Hl, h), near(X; Wl, w)) and the coefficient at the same cell,
 *   or with CA_SEGTAB_DOWNSCALE at (near(near(Y; Hl, 14); 14, h), near(near(X; Wl, 14); 14, w)); near as above
 *   n11, n10, n01, n00 = pixels by (mask, label != 0): sums over the cells of the mask's tables, exact integers
 *   ap    = the average precision of the 2 Hl Wl stacked scores (float32(1 - c), c) against the one-hot label, both
 *           scores through np.nan_to_num (NaN -> 0, +-inf -> +-FLT_MAX), -0.0 and 0.0 one threshold: the sum over the
 *           distinct scores, descending, of (R_k - R_{k-1}) P_k with P_k = tp_k / n_k and R_k = tp_k / (Hl Wl) in
 *           fp64, tp_k and n_k exact integers; the sum over a fixed tree (the same bits every run)
 * maps: map m is fp32 [h, w] contiguous at maps + m * map_stride (elements, >= h w; what lies between two maps is
 * never read: with [levels, layers, C, h w] tables concept k is maps = table + k h w, map_stride = C h w,
 * n_maps = levels * layers).  label: uint8 [Hl, Wl], nonzero = positive, shared by all maps.  records: n_maps
 * contiguous ca_seg_record, 8-byte aligned.  cells: device workspace uint32 [4, (h w + 3) & ~3], 16-byte aligned: the
 * mask's tot / pos and the coefficient's tot / pos per cell; the call zeroes it itself, in a kernel on the stream.
 * blur_weights: nine floats on the HOST, read during the call, required with CA_SEGTAB_BLUR.  Nothing is allocated,
 * uploaded or retained.  Limits: 1 <= h w <= 4096, 1 <= Hl Wl <= 2^24, 1 <= n_maps <= CA_SEGTAB_MAX_MAPS,
 * map_stride >= h w, CA_SEGTAB_BLUR needs h, w >= 2, no other flag bit; CA_ERR_ARG otherwise, before any launch.
 * Needs up to 112.5 KB of LDS. */
#define CA_SEGTAB_MAX_MAPS 65536
#define CA_SEGTAB_MEAN_THRESHOLD 1
#define CA_SEGTAB_DOWNSCALE 2
#define CA_SEGTAB_BLUR 4
#define CA_SEGTAB_RAW 8
int ca_segtab_score(const float *maps, int64_t map_stride, int32_t n_maps, const void *label, void *records,
                    void *cells, int32_t h, int32_t w, int32_t Hl, int32_t Wl, int32_t flags,
                    const float *blur_weights, ca_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Heat-map pictures (the colouring of concept_attention/concept_attention_pipeline.py:174-196, the overlays of
 * concept_attention/plotting.py::overlay_heatmap_on_image, the frames of concept_attention/video/video_utils.py): fp32
 * map planes [h, w] become RGB bytes [H, W, 3] without leaving the device.  A problem is a GROUP: the n_maps planes that
 * share one range ("global min-max over ALL concepts" of an item and space; all frames of a concept).  Every
 * floating-point operation is fp32 and rounds on its own, except the bilinear source coordinate (below).
 *   Range.  With range_in == NULL, lo / hi are the minimum / maximum over all n_maps h w cells of the group; if any cell
 *     is NaN both are NaN, as ndarray.min() gives.  Otherwise range_in = {lo, hi} is used as given, lo >= hi included.
 *     range_out is always written; range_in may be the range_out of an earlier call or the problem's own, not that of
 *     another problem of the same call.  The range is taken over the SOURCE cells under bilinear upscaling too (imshow
 *     autoscales over the upscaled plane: a stated difference).
 *   Value v at output pixel (y, x).
 *     nearest (default): v = map[sy, sx], sy = min((int)floorf(y * ((float)h / H)), h - 1), sx likewise: the rule of
 *       torch.nn.functional.interpolate(mode="nearest") as ca_pixels_u8_to_nhwc32_bf16 uses it;
 *     CA_RENDER_BILINEAR: torch's align_corners=False rule: fy = fmaf((float)h / H, y + 0.5f, -0.5f), clamped below at 0
 *       (the one fused operation of the entry: torch's builds contract this expression, and with the product rounded
 *       first a coordinate near 60 moves by 2^-19, a value by up to 43 x 2^-24 of the largest cell at 64 -> 224),
 *       y0 = (int)fy, y1 = min(y0 + 1, h - 1), ly = fy - y0, the same for x, and
 *       v = (1 - ly) * ((1 - lx) * a00 + lx * a01) + ly * ((1 - lx) * a10 + lx * a11) in exactly that order (so
 *       0 * inf is NaN, as in torch).
 *   Colour: matplotlib's rule for a float array (Colormap._get_rgba_and_mask): t = (v - lo) / (hi - lo), the division
 *     correctly rounded; xa = t * 256.0f; LUT row 258 if xa is NaN, else 256 if xa < 0, else 255 if xa == 256, else 257
 *     if xa >= 256, else (int)xa.  -0.0 is row 0; hi == lo gives NaN everywhere.
 *     lut: uint8 [259, 3] on the device, made by the caller: rows 0..255 (cmap(arange(256))[:, :3] * 255) as bytes, then
 *     the under, over and bad colours.
 *   Blend (CA_RENDER_BLEND): out_c = (uint8)(int)((float)col_c * alpha + (float)img_c * (1.0f - alpha) + 0.5f) with
 *     1 - alpha formed once; a pixel whose row is 258 keeps the picture's bytes (matplotlib's bad colour is
 *     transparent).  This is round-half-up on the blended value, not Agg's compositing: a stated difference.
 * All problems of a call share h, w, H, W, lut, alpha and flags.  Limits: 1 <= n_problems <= CA_RENDER_MAX_PROBLEMS,
 * 1 <= h w <= CA_RENDER_MAX_CELLS, 1 <= H, W <= CA_RENDER_MAX_SIDE, 1 <= n_maps <= CA_RENDER_MAX_MAPS, map_stride >= h w
 * and out_stride >= 3 H W when n_maps > 1, no other flag bit; with CA_RENDER_BLEND 0 <= alpha <= 1 and every problem has
 * an image with image_stride >= 3 W (unused when H = 1); without it alpha and image are ignored.  CA_ERR_ARG otherwise,
 * before any launch.  Two to four launches on the stream, no host synchronisation, no float atomics (the range is
 * folded with integer atomics on order keys held in range_out, so the bits do not depend on the arrival order); nothing
 * depends on what range_out or out held before.  Planes of out may start at any byte. */
#define CA_RENDER_MAX_PROBLEMS 16
#define CA_RENDER_MAX_MAPS 65536
#define CA_RENDER_MAX_CELLS 16384
#define CA_RENDER_MAX_SIDE 4096
#define CA_RENDER_BILINEAR 1
#define CA_RENDER_BLEND 2
typedef struct {
  const float *maps;      /* fp32 planes [h, w], each contiguous, map_stride ELEMENTS apart (>= h*w; unused when n_maps = 1) */
  int64_t map_stride;
  int32_t n_maps;         /* 1 .. CA_RENDER_MAX_MAPS (65536) */
  const float *range_in;  /* device fp32 [2] = {lo, hi}, or NULL: the range of all cells of the group's n_maps planes */
  float *range_out;       /* device fp32 [2]: the {lo, hi} that was used; never NULL */
  const void *image;      /* uint8 [H, W, 3], rows image_stride BYTES apart, or NULL: no blend */
  int64_t image_stride;
  void *out;              /* uint8, n_maps planes [H, W, 3] contiguous, out_stride BYTES apart (>= 3*H*W, any value) */
  int64_t out_stride;
} ca_render_problem;
int ca_heatmap_render(const ca_render_problem *problems, int32_t n_problems, int32_t h, int32_t w, int32_t H, int32_t W,
                      const void *lut /* uint8 [259, 3], device */, float alpha, int32_t flags, ca_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CONCEPTATTN_H */
