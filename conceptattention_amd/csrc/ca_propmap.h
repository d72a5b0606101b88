// ca_propagate_maps: a few fp32 map rows propagated through the attention of the query rows: every query row's value is
// replaced by the softmax-weighted mean of the values at the keys it attends to, averaged over the heads and added into
// fp32 accumulators.  A flash-attention pass whose value operand is the C map rows instead of v; the [nq, n0 + n1]
// probability matrix is never stored.  Exported and bound (conceptattention_amd/_lib.py, INTERNAL_SIGNATURES); not part of
// include/conceptattn.h yet, so the ABI version stays.
#pragma once
#include <stdint.h>

#include "../../include/conceptattn.h"

#define CA_PROPMAP_MAX_PROBLEMS 16
#define CA_PROPMAP_MAX_CONCEPTS 32      /* C: the map rows of a problem (CA_HEATMAP_MAX_CONCEPTS) */
#define CA_PROPMAP_MAX_ROWS 2147483520  /* n0 + n1: 2^31 - 128, whole tiles of keys stay below 2^31 */
#define CA_PROPMAP_MAX_HEADS 65535      /* num_heads: one grid row per head */
#define CA_PROPMAP_QK_F16 1             /* flags: the q and k rows hold IEEE half bits in their bf16-typed tensors */

// One problem: nq query rows (q, row stride ldq elements), n0 leading key rows (k0: in the softmax, they carry no value)
// followed by n1 valued key rows (k1), both with row stride ldk; num_heads heads of 128, head h at columns h*128.. of
// every row; C map rows v[c, j] (fp32, row stride ldv >= n1 elements), one value per valued key.
// Per head h and query row i, over all n0 + n1 keys j:
//   s_h[i, j] = scale_log2 * <q_h[i], k_h[j]>   (products exact, fp32 accumulation)
//   m_h[i]    = max_j s_h[i, j]
//   l_h[i]    = sum_j exp2(s_h[i, j] - m_h[i])
//   o_h[c, i] = sum_{j < n1} exp2(s_h[i, n0 + j] - m_h[i]) * v[c, j] / l_h[i]      (p and v enter the product as fp32)
//   out[c, i] = (1 / num_heads) * sum_h o_h[c, i]                                  (heads summed in head order)
//   acc [c, i] += weight  * out[c, i]        fp32 [C, nq] contiguous, optional
//   acc2[c, i] += weight2 * out[c, i]        the same, optional; at least one of the two
// A NaN in a q row makes that query's cells NaN in every row c; a NaN in a key row makes every cell NaN; a NaN in v[c, j]
// makes row c NaN and leaves the other rows finite.  Any other non-finite v (an infinity) is unspecified: it meets
// probabilities that are exactly zero.  With n0 = 0 (k0 is then not read) the weights of a query row sum to 1: a
// constant row of v stays that constant.  v must not overlap acc or acc2 of any problem of the call.
typedef struct ca_propmap_problem {
  const void *q;    /* bf16 (or half bits) [nq, >= num_heads*128], 16-byte aligned */
  const void *k0;   /* [n0, ...] or NULL with n0 = 0 */
  const void *k1;   /* [n1, ...] */
  const float *v;   /* fp32 [C, n1], row stride ldv, 4-byte aligned */
  float *acc;
  float *acc2;
  int32_t nq, ldq;
  int32_t n0, n1, ldk;
  int32_t C, ldv;
  int32_t _pad;
  float weight, weight2;
} ca_propmap_problem;

#ifdef __cplusplus
extern "C" {
#endif

// Scratch memory ca_propagate_maps needs for these problems, in bytes: o_h[c, i] of every head of every problem, which the
// attention pass hands to the head sum: the sum over the problems of num_heads * C * nq * 4, each rounded up to 16 (a
// negative value: an argument error).
int64_t ca_propagate_maps_workspace_bytes(const ca_propmap_problem *problems, int32_t n_problems, int32_t num_heads);

// Up to CA_PROPMAP_MAX_PROBLEMS problems in TWO launches (attention per head, then the head sum); 1 <= C <=
// CA_PROPMAP_MAX_CONCEPTS, nq >= 1, n0 >= 0, n1 >= 1, n0 + n1 at most CA_PROPMAP_MAX_ROWS, num_heads at most
// CA_PROPMAP_MAX_HEADS.
// scale_log2: 1.0 when the q rows already carry softmax_scale * log2(e) (the model's Q_OUT_SCALE), softmax_scale * log2(e)
// for plain rows.  flags: 0 or CA_PROPMAP_QK_F16.  workspace / workspace_bytes: at least
// ca_propagate_maps_workspace_bytes() bytes of device memory, 16-byte aligned; never written outside that size, and the
// call needs nothing of what an earlier call left there.
// All pointers are borrowed device pointers; nothing is allocated; stream-ordered, no host wait, replayable under graph
// capture; deterministic (no atomics): a problem's bits depend neither on what else is in the launch nor on where in the
// grid a cell lands.
// Returns 0, or a negative code with ca_last_error() text beginning "ca_propagate_maps: ".
int ca_propagate_maps(const ca_propmap_problem *problems, int32_t n_problems, int32_t num_heads, float scale_log2,
                      int32_t flags, void *workspace, int64_t workspace_bytes, ca_stream_t stream);

#ifdef __cplusplus
}
#endif
