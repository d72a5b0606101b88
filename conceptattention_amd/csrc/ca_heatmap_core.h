// The device core of the concept heat-map kernels, shared by ca_rowops.hip (ca_heatmap_logits_bf16, the weighting kernels,
// ca_heatmap_fused) and ca_heatmap_many.hip (ca_heatmap_many, the 32-concept sparse weighting): the wave reductions, the row
// loads, the weighting across the concepts of one patch and the update of a problem's accumulators.  Every form of the
// heat maps evaluates these expressions, which is what makes them bit-identical to one another.  Each unit compiles its own
// copy (anonymous namespace).
#pragma once

#include <climits>
#include <type_traits>

#include "ca_common.h"

namespace {   // device code

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// 8 consecutive elements of an fp32 or bf16 row (16-byte aligned) as floats
__device__ __forceinline__ void load8(const float *p, float *v) {
  const f32x4 t0 = *(const f32x4 *)p, t1 = *(const f32x4 *)(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = t0[j], v[4 + j] = t1[j];
}
__device__ __forceinline__ void load8(const bf16 *p, float *v) {
  const bf16x8 t = *(const bf16x8 *)p;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
}

// The weighting across the C concepts of one patch, shared by the three-launch kernels below and the fused kernel, so
// that both forms evaluate the same expressions.
// softmax: v[c] = exp(z[c] - max z) for c < C, sum = their sum in c order (the caller multiplies by weight / sum).
template <int CMAX>
__device__ __forceinline__ void hm_softmax_terms(const float (&z)[CMAX], int C, float (&v)[CMAX], float &sum) {
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) mx = fmaxf(mx, z[c]);
  sum = 0.f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    v[c] = c < C ? __expf(z[c] - mx) : 0.f;
    if (c < C) sum += v[c];
  }
}

// sparsemax_c / entmax15_c (logits[:,p]): the two sparse alternatives to the softmax over concepts
// (concept_attention_pipeline.py:66-69 calls the third-party `entmax` package for them).  Both are the
// published sort-and-threshold algorithms: sparsemax (Martins & Astudillo 2016, Alg. 1): z sorted descending,
// k = max{j : 1 + j z_(j) > sum_{i<=j} z_(i)}, tau = (sum_{i<=k} z_(i) - 1) / k, p = max(z - tau, 0);
// 1.5-entmax (Peters, Niculae & Martins 2019, Alg. 2): x = (z - max z) / 2 sorted, for every prefix j
// mean M_j, ss_j = j (mean of squares - M_j^2), tau_j = M_j - sqrt(max((1 - ss_j) / j, 0)),
// k = #{j : tau_j <= x_(j)}, p = max(x - tau_k, 0)^2.  The C <= CMAX logits in registers; z_in[c >= C] is ignored.
template <int CMAX, bool ENTMAX15>
__device__ __forceinline__ void hm_sparse_terms(const float (&z_in)[CMAX], int C, float (&v)[CMAX]) {
  float z[CMAX], srt[CMAX];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    z[c] = c < C ? z_in[c] : -INFINITY;
    mx = fmaxf(mx, z[c]);
  }
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    z[c] = (z[c] - mx) * (ENTMAX15 ? 0.5f : 1.0f);  // both maps are shift-invariant; -inf padding stays -inf
    srt[c] = z[c];
  }
  // odd-even transposition sort, descending (fully unrolled: the array never leaves the registers)
#pragma unroll
  for (int pass = 0; pass < CMAX; ++pass)
#pragma unroll
    for (int i = pass & 1; i + 1 < CMAX; i += 2) {
      const float a = srt[i], b = srt[i + 1];
      srt[i] = fmaxf(a, b);
      srt[i + 1] = fminf(a, b);
    }
  float tau = 0.f;
  float cs = 0.f, cs2 = 0.f;
#pragma unroll
  for (int j = 0; j < CMAX; ++j) {
    if (j < C) {
      cs += srt[j];
      cs2 += srt[j] * srt[j];
      const float rho = (float)(j + 1);
      float tj;
      bool in;
      if (ENTMAX15) {
        const float mean = cs / rho;
        const float ss = rho * (cs2 / rho - mean * mean);
        tj = mean - sqrtf(fmaxf((1.0f - ss) / rho, 0.0f));
        in = tj <= srt[j];
      } else {
        tj = (cs - 1.0f) / rho;
        in = 1.0f + rho * srt[j] > cs;
      }
      if (in) tau = tj;  // the support is a prefix of the sorted order, so the last j that passes is k
    }
  }
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    const float d = fmaxf(z[c] - tau, 0.f);
    v[c] = c < C ? (ENTMAX15 ? d * d : d) : 0.f;
  }
}

// acc[c,p] += weight * sparsemax_c / entmax15_c (logits[:,p]); one thread per patch.
template <int CMAX, bool ENTMAX15>
__global__ __launch_bounds__(256) void ca_heatmap_sparse_kernel(const float *__restrict__ logits, int C, int L,
                                                                float weight, float *__restrict__ acc) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= L) return;
  float z[CMAX], v[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) z[c] = c < C ? logits[(size_t)c * L + p] : -INFINITY;
  hm_sparse_terms<CMAX, ENTMAX15>(z, C, v);
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) acc[(size_t)c * L + p] += weight * v[c];
}

// the argument of a fused launch (ca_heatmap_fused, ca_heatmap_many): the problems by value
struct HeatmapLaunch {
  ca_heatmap_problem p[CA_HEATMAP_MAX_PROBLEMS];
  int32_t L, C, dim, norm;
};

// the weighting of one patch's C logits and the update of the problem's accumulators (shared by the fused bodies)
template <int CC>
__device__ __forceinline__ void hm_weight_and_accumulate(const ca_heatmap_problem &P, const float (&z)[CC], int pp, int L,
                                                         int C, int norm) {
  float v[CC];
  if (P.logits) {
#pragma unroll
    for (int c = 0; c < CC; ++c)
      if (c < C) P.logits[(size_t)c * L + pp] = z[c];
  }
  if (norm == CA_NORM_SOFTMAX) {
    float sum;
    hm_softmax_terms<CC>(z, C, v, sum);
    if (P.acc) {
      const float inv = P.weight / sum;
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) P.acc[(size_t)c * L + pp] += v[c] * inv;
    }
    if (P.acc2) {
      const float inv = P.weight2 / sum;
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) P.acc2[(size_t)c * L + pp] += v[c] * inv;
    }
  } else {
    if (norm == CA_NORM_SPARSEMAX) hm_sparse_terms<CC, false>(z, C, v);
    else hm_sparse_terms<CC, true>(z, C, v);
    if (P.acc) {
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) P.acc[(size_t)c * L + pp] += P.weight * v[c];
    }
    if (P.acc2) {
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (c < C) P.acc2[(size_t)c * L + pp] += P.weight2 * v[c];
    }
  }
}

}  // namespace

namespace {   // host helpers

// One kernel launch of this unit and its check.  The arguments are converted to the kernel's parameter types (a void *
// of the C interface becomes the kernel's typed pointer).  FN = the entry point's name for messages.
template <typename... KA, typename... A>
int launch(void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds_bytes, ca_stream_t stream, const char *FN, A... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, (hipStream_t)stream, static_cast<KA>(args)...);
  return ca_check_launch(FN);
}

// workgroups of a one-dimensional launch: n items, per_block of them per workgroup, at most cap workgroups
unsigned grid_1d(long n, long per_block, long cap = LONG_MAX) {
  const long blocks = (n + per_block - 1) / per_block;
  return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

// ca_heatmap_fused's work for 1 <= C <= CA_HEATMAP_MAX_CONCEPTS concepts, still ONE launch per layer (ca_heatmap_many.hip):
// the concept vectors go through LDS in ceil(C / 8) chunks of at most 8 rows while a wave keeps its two patches' image rows
// in registers, and a patch's C logits are weighted once the last chunk is done.  Same problem struct, same arithmetic per
// (patch, concept): bit-identical to ca_heatmap_logits_bf16 followed by ca_heatmap_norm_accumulate at every C, and to
// ca_heatmap_fused at C <= 8.  All three norms; acc, acc2 and logits each optional (at least one); bf16 or fp32 vectors per
// problem.  img_f32 = 2 (the per-head partials, 8 slots) is not accepted: CA_ERR_ARG.  Exported with C linkage and bound by
// _lib.py (INTERNAL_SIGNATURES); not declared in include/conceptattn.h yet: every streamed entry point of that header is
// listed in the stream-contract probe table of the test suite, which this entry point's own probe
// (tests/test_heatmap_many_kernels_gpu.py) is not part of.
extern "C" int ca_heatmap_many(const ca_heatmap_problem *problems, int32_t n_problems, int32_t L, int32_t C, int32_t dim,
                               int32_t norm, ca_stream_t stream);

// ca_heatmap_norm_accumulate's sparse norms at 17 .. CA_HEATMAP_MAX_CONCEPTS concepts (arguments already checked, FN = the
// called entry point's name); defined in ca_heatmap_many.hip
int ca_heatmap_sparse32(const char *FN, const float *logits, int32_t C, int32_t L, int32_t norm, float weight, float *acc,
                        ca_stream_t stream);
