// ca_token_maps: prompt-token attention maps (DAAM for Flux).  The attention probability that image-token queries give to
// the prompt's text-token keys in a double block's joint [text | image] softmax, averaged over the heads and added into
// fp32 accumulators.  Exported and bound (conceptattention_amd/_lib.py, INTERNAL_SIGNATURES); not part of
// include/conceptattn.h yet, so the ABI version stays.
#pragma once
#include <stdint.h>

#include "../../include/conceptattn.h"

#define CA_TOKMAP_MAX_PROBLEMS 16
#define CA_TOKMAP_MAX_TEXT 512      /* n0: text key rows of a problem */
#define CA_TOKMAP_MAX_ROWS 2147483520   /* nq, and n0 + n1: 2^31 - 128, whole blocks of 64 rows stay below 2^31 */
#define CA_TOKMAP_QK_F16 1          /* flags: the q and k rows hold IEEE half bits in their bf16-typed tensors */

// One problem: nq image query rows (q, row stride ldq elements), n0 text key rows (k0) followed by n1 image key rows (k1),
// both with row stride ldk; num_heads heads of 128, head h at columns h*128.. of every row.  Per head h and query row i:
//   s_h[i, j] = scale_log2 * <q_h[i], k_h[j]>   over all n0 + n1 keys (products exact, fp32 accumulation)
//   m_h[i]    = max_j s_h[i, j]
//   l_h[i]    = sum_j exp2(s_h[i, j] - m_h[i])
// and for the first n_tok <= n0 text keys t:
//   map[t, i]   = (1 / num_heads) * sum_h exp2(s_h[i, t] - m_h[i]) / l_h[i]     (heads summed in head order)
//   acc [t, i] += weight  * map[t, i]        fp32 [n_tok, nq] contiguous, optional
//   acc2[t, i] += weight2 * map[t, i]        the same, optional; at least one of the two
//   lse [h, i]  = (m_h[i] + log2 l_h[i]) * ln 2    fp32 [num_heads, nq] contiguous, optional output
// A NaN in a q row makes that row's cells NaN; a NaN in a key row makes every cell NaN.  n1 = 0 is legal (k1 is then not
// read): the softmax runs over the text keys alone.
typedef struct ca_tokmap_problem {
  const void *q;    /* bf16 (or half bits) [nq, >= num_heads*128], 16-byte aligned */
  const void *k0;   /* [n0, ...] */
  const void *k1;   /* [n1, ...] or NULL with n1 = 0 */
  float *acc;
  float *acc2;
  float *lse;
  int32_t nq, ldq;
  int32_t n0, n1, ldk;
  int32_t n_tok;
  float weight, weight2;
} ca_tokmap_problem;

#ifdef __cplusplus
extern "C" {
#endif

// Scratch memory ca_token_maps needs for these problems, in bytes.  The head sum is carried in LDS by the one workgroup
// that owns a block of 64 query rows, so this is 0 for every geometry (a negative value: an argument error).
int64_t ca_token_maps_workspace_bytes(const ca_tokmap_problem *problems, int32_t n_problems, int32_t num_heads);

// Up to CA_TOKMAP_MAX_PROBLEMS problems in ONE launch; 1 <= n_tok <= n0 <= CA_TOKMAP_MAX_TEXT, n1 >= 0, nq >= 1; nq and
// n0 + n1 at most CA_TOKMAP_MAX_ROWS.
// scale_log2: 1.0 when the q rows already carry softmax_scale * log2(e) (the model's Q_OUT_SCALE), softmax_scale * log2(e)
// for plain rows.  flags: 0 or CA_TOKMAP_QK_F16.  workspace / workspace_bytes: at least ca_token_maps_workspace_bytes()
// bytes of device memory (may be NULL when that is 0); never written outside that size.
// All pointers are borrowed device pointers; nothing is allocated; stream-ordered, no host wait, replayable under graph
// capture; deterministic (no atomics) and a problem's bits do not depend on what else is in the launch.
// Returns 0, or a negative code with ca_last_error() text beginning "ca_token_maps: ".
int ca_token_maps(const ca_tokmap_problem *problems, int32_t n_problems, int32_t num_heads, float scale_log2, int32_t flags,
                  void *workspace, int64_t workspace_bytes, ca_stream_t stream);

#ifdef __cplusplus
}
#endif
