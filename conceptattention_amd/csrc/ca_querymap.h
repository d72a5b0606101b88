// ca_query_maps: query-row attention maps.  Where a few query rows (a prompt's text tokens, or the concept tokens) look
// among the image keys: the softmax probability each query row puts on every emitted key row, in the attention the model
// ran, averaged over the heads and added into fp32 accumulators.  The transpose of ca_token_maps' problem (few queries,
// thousands of emitted keys).  Exported and bound (conceptattention_amd/_lib.py, INTERNAL_SIGNATURES); not part of
// include/conceptattn.h yet, so the ABI version stays.
#pragma once
#include <stdint.h>

#include "../../include/conceptattn.h"

#define CA_QUERYMAP_MAX_PROBLEMS 16
#define CA_QUERYMAP_MAX_QUERIES 512      /* nq: query rows of a problem */
#define CA_QUERYMAP_MAX_ROWS 2147483520  /* n0 + n1: 2^31 - 128, whole blocks of 128 keys stay below 2^31 */
#define CA_QUERYMAP_QK_F16 1             /* flags: the q and k rows hold IEEE half bits in their bf16-typed tensors */

// One problem: nq query rows (q, row stride ldq elements), n0 leading key rows (k0: in the softmax, not emitted) followed
// by n1 emitted key rows (k1), both with row stride ldk; num_heads heads of 128, head h at columns h*128.. of every row.
// Per head h and query row i, over all n0 + n1 keys j:
//   s_h[i, j] = scale_log2 * <q_h[i], k_h[j]>   (products exact, fp32 accumulation)
//   m_h[i]    = max_j s_h[i, j]
//   l_h[i]    = sum_j exp2(s_h[i, j] - m_h[i])
// and for the n1 emitted keys j:
//   map[i, j]   = (1 / num_heads) * sum_h exp2(s_h[i, n0 + j] - m_h[i]) / l_h[i]     (heads summed in head order)
//   acc [i, j] += weight  * map[i, j]        fp32 [nq, n1] contiguous, optional
//   acc2[i, j] += weight2 * map[i, j]        the same, optional; at least one of the two
//   lse [h, i]  = (m_h[i] + log2 l_h[i]) * ln 2    fp32 [num_heads, nq] contiguous, optional output
// A NaN in a q row makes that row's cells NaN; a NaN in a key row makes every cell NaN.  n0 = 0 is legal (k0 is then not
// read): every row of map sums to 1.
typedef struct ca_querymap_problem {
  const void *q;    /* bf16 (or half bits) [nq, >= num_heads*128], 16-byte aligned */
  const void *k0;   /* [n0, ...] or NULL with n0 = 0 */
  const void *k1;   /* [n1, ...] */
  float *acc;
  float *acc2;
  float *lse;
  int32_t nq, ldq;
  int32_t n0, n1, ldk;
  int32_t _pad;
  float weight, weight2;
} ca_querymap_problem;

#ifdef __cplusplus
extern "C" {
#endif

// Scratch memory ca_query_maps needs for these problems, in bytes: the (m, l) pair of every (head, query row) of every
// problem, which the statistics pass hands to the emit pass: the sum over the problems of num_heads * nq * 8, each rounded
// up to 16 (a negative value: an argument error).
int64_t ca_query_maps_workspace_bytes(const ca_querymap_problem *problems, int32_t n_problems, int32_t num_heads);

// Up to CA_QUERYMAP_MAX_PROBLEMS problems in TWO launches (statistics, then emit); 1 <= nq <= CA_QUERYMAP_MAX_QUERIES,
// n0 >= 0, n1 >= 1, n0 + n1 at most CA_QUERYMAP_MAX_ROWS.
// scale_log2: 1.0 when the q rows already carry softmax_scale * log2(e) (the model's Q_OUT_SCALE), softmax_scale * log2(e)
// for plain rows.  flags: 0 or CA_QUERYMAP_QK_F16.  workspace / workspace_bytes: at least
// ca_query_maps_workspace_bytes() bytes of device memory, 16-byte aligned; never written outside that size, and the call
// needs nothing of what an earlier call left there.
// All pointers are borrowed device pointers; nothing is allocated; stream-ordered, no host wait, replayable under graph
// capture; deterministic (no atomics): a problem's bits depend neither on what else is in the launch nor on where in the
// grid a cell lands.
// Returns 0, or a negative code with ca_last_error() text beginning "ca_query_maps: ".
int ca_query_maps(const ca_querymap_problem *problems, int32_t n_problems, int32_t num_heads, float scale_log2, int32_t flags,
                  void *workspace, int64_t workspace_bytes, ca_stream_t stream);

#ifdef __cplusplus
}
#endif
