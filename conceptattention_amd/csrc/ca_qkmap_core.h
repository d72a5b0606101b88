// What the two q.k map units (ca_tokmap.hip, ca_querymap.hip) share, stated once: the MFMA fragments of a head's 128
// columns, the key rows of [k0 | k1], the register-fragment score, the accumulators' write-out, and the entry rules that
// do not depend on the unit.  Each unit keeps its own tiling and summation order (its bounds and its emulation in
// tests/tokmap_cases.py / tests/querymap_cases.py are derived from them), its size rule and its launches.  Device
// functions are __forceinline__ and run in the including kernel; nothing here is a kernel or a translation unit of its
// own.  `Problem` is ca_tokmap_problem or ca_querymap_problem: the fields used here have one name and one meaning in both.
#pragma once
#include <math.h>

#include "ca_common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------- device
// S^T += K Q^T on v_mfma_f32_16x16x32: the key on the accumulator's row, the query on its column
template <bool F16>
__device__ __forceinline__ f32x4 qk_mfma(u32x4 k, u32x4 q, f32x4 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, k), __builtin_bit_cast(f16x8, q), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, k), __builtin_bit_cast(bf16x8, q), c, 0, 0, 0);
}

// the address of key row j (0 <= j < n0 + n1) of a problem, head columns not included
template <class Problem>
__device__ __forceinline__ const uint16_t *qk_key_row(const Problem &P, int j) {
  return j < P.n0 ? (const uint16_t *)P.k0 + (size_t)j * (size_t)P.ldk
                  : (const uint16_t *)P.k1 + (size_t)(j - P.n0) * (size_t)P.ldk;
}

// a lane's fragment of 16 rows, head h: row (lane & 15) of the 16, columns 8 (lane >> 4) + 32 ks .. of the head
__device__ __forceinline__ void qk_frag_load(const uint16_t *row, int h, u32x4 (&f)[4]) {
  const uint16_t *p = row + (size_t)h * 128 + ((threadIdx.x & 63) >> 4) * 8;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) f[ks] = *(const u32x4 *)(p + ks * 32);
}

// the scores of 16 keys against 16 queries: lane l gets keys 4 (l >> 4) + 0..3 of query l & 15, times scale_log2
template <bool F16>
__device__ __forceinline__ f32x4 qk_scores(const u32x4 (&kf)[4], const u32x4 (&qf)[4], float scale_log2) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) s = qk_mfma<F16>(kf[ks], qf[ks], s);
  return s * scale_log2;
}

// cell o of whichever accumulators the problem has: one read-modify-write each, by the cell's only writer
template <class Problem>
__device__ __forceinline__ void qk_accumulate(const Problem &P, size_t o, float v) {
  if (P.acc) P.acc[o] = __builtin_fmaf(P.weight, v, P.acc[o]);
  if (P.acc2) P.acc2[o] = __builtin_fmaf(P.weight2, v, P.acc2[o]);
}

// ------------------------------------------------------------------------------------------------------------ host
// The argument rules of an entry and of its workspace query; 0 or CA_ERR_ARG with the text under FN.  Per problem, in this
// order: the unit's `sizes_ok(FN, i, p)` (which sets its own text), the rows, the outputs.  `k0_optional`: with n0 = 0, k0
// may be null (otherwise: with n1 = 0, k1 may); `rows_need`: the unit's words for that.
template <class Problem, class SizeRule>
static int qk_check(const char *FN, const Problem *problems, int32_t n_problems, int32_t num_heads, int32_t max_problems,
                    bool k0_optional, const char *rows_need, SizeRule sizes_ok) {
  if (!problems || n_problems < 1 || n_problems > max_problems || num_heads < 1 || num_heads > (1 << 16)) {
    ca_set_error("%s: bad arguments (n_problems=%d num_heads=%d; need 1 <= n_problems <= %d, 1 <= num_heads <= 65536)", FN,
                 n_problems, num_heads, max_problems);
    return CA_ERR_ARG;
  }
  const int64_t width = (int64_t)num_heads * 128;
  for (int i = 0; i < n_problems; ++i) {
    const Problem &p = problems[i];
    if (!sizes_ok(FN, i, p)) return CA_ERR_ARG;
    const bool missing = k0_optional ? (!p.k1 || (p.n0 > 0 && !p.k0)) : (!p.k0 || (p.n1 > 0 && !p.k1));
    if (!p.q || missing || (((uintptr_t)p.q | (uintptr_t)p.k0 | (uintptr_t)p.k1) & 15) || p.ldq < width || p.ldk < width ||
        p.ldq % 8 || p.ldk % 8) {
      ca_set_error("%s: problem %d rows invalid (ldq=%d ldk=%d; %s non-null and 16-byte aligned, row strides >= "
                   "num_heads*128 = %lld and a multiple of 8)", FN, i, p.ldq, p.ldk, rows_need, (long long)width);
      return CA_ERR_ARG;
    }
    if ((!p.acc && !p.acc2) || (((uintptr_t)p.acc | (uintptr_t)p.acc2 | (uintptr_t)p.lse) & 3)) {
      ca_set_error("%s: problem %d outputs invalid (at least one of acc / acc2; acc, acc2 and lse 4-byte aligned)", FN, i);
      return CA_ERR_ARG;
    }
  }
  return CA_OK;
}

// `qk_f16`: the entry's one flag bit
static int qk_check_scale_flags(const char *FN, float scale_log2, int32_t flags, int32_t qk_f16) {
  if (isfinite(scale_log2) && !(flags & ~qk_f16)) return CA_OK;
  ca_set_error("%s: bad arguments (scale_log2=%g flags=%d; need a finite scale_log2, flags 0 or %d)", FN, (double)scale_log2,
               flags, qk_f16);
  return CA_ERR_ARG;
}
