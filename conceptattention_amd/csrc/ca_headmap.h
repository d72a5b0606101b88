// ca_head_maps: per-head concept maps and the raw-space baselines.  The logits of C concept rows against L image rows
// head by head (heads of 128 columns), weighted across the concepts PER HEAD, then the head-resolved tensor and / or the
// mean over the heads added into fp32 accumulators.  Exported and bound (conceptattention_amd/_lib.py,
// INTERNAL_SIGNATURES); not declared in include/conceptattn.h, whose CA_VERSION counts this entry point as 137.
#pragma once
#include <stdint.h>

#include "../../include/conceptattn.h"

#define CA_NORM_NONE 3              /* the weights are the logits themselves (next to CA_NORM_SOFTMAX / SPARSEMAX / ENTMAX15) */
#define CA_HEADMAP_MAX_HEADS 65536

// One problem: L image rows (img, row stride ldi elements) and C concept rows (con, row stride ldc), num_heads heads of
// 128, head h at columns 128 h .. 128 h + 127 of every row.  Per head h, concept c and patch p:
//   z[h, c, p] = sum_{d < 128} con[c, 128 h + d] * img[p, 128 h + d]     (fp32; the order is ca_headmap.hip's header)
//   w[h, :, p] = norm(z[h, :, p])                                         across the C concepts
//   heads[h, c, p] += weight_h * w[h, c, p]                               fp32 [num_heads, C, L] contiguous, optional
//   acc  [c, p]    += weight  * (1 / num_heads) * sum_h w[h, c, p]        fp32 [C, L] contiguous, optional
//   acc2 [c, p]    += weight2 * (1 / num_heads) * sum_h w[h, c, p]        the same, optional; at least one of the three
typedef struct ca_headmap_problem {
  const void *img;   /* bf16 or fp32 [L, >= num_heads*128], 16-byte aligned */
  const void *con;   /* bf16 or fp32 [C, >= num_heads*128], 16-byte aligned */
  float *heads;
  float *acc;
  float *acc2;
  int32_t ldi, ldc;            /* row strides in elements: a multiple of 8 (bf16) or 4 (fp32) */
  int32_t img_f32, con_f32;    /* 0: bf16 rows, 1: fp32 rows */
  float weight_h, weight, weight2;
  int32_t _pad;
} ca_headmap_problem;

#ifdef __cplusplus
extern "C" {
#endif

// Up to CA_HEATMAP_MAX_PROBLEMS problems that share L, C, num_heads and the norm in ONE launch; 1 <= C <=
// CA_HEATMAP_MAX_CONCEPTS for every norm, 1 <= num_heads <= CA_HEADMAP_MAX_HEADS, L >= 1.
// norm: CA_NORM_NONE, CA_NORM_SOFTMAX, CA_NORM_SPARSEMAX or CA_NORM_ENTMAX15.
// Two problems of a launch must not name the same accumulator.  All pointers are borrowed device pointers; nothing is
// allocated; stream-ordered, no host wait, replayable under graph capture; deterministic (no atomics: a patch's update is
// owned by one wave), and a patch's bits depend on its own rows only, not on its position, the other problems or the grid.
// Returns 0, or a negative code with ca_last_error() text beginning "ca_head_maps: ".
int ca_head_maps(const ca_headmap_problem *problems, int32_t n_problems, int32_t L, int32_t C, int32_t num_heads,
                 int32_t norm, ca_stream_t stream);

#ifdef __cplusplus
}
#endif
