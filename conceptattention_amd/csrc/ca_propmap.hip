// ca_propagate_maps: C fp32 map rows propagated through the attention of nq query rows over the keys [k0 | k1]
// (semantics: ca_propmap.h).  A flash-attention pass whose value operand is the map rows v[c, j] of the n1 valued keys
// instead of the model's v, summed over the heads; the probabilities never leave the registers.  It re-reads the q and k
// rows an attention launch has read.  The unit states its own fragments and score step (pm_*): it shares no header with
// ca_tokmap.hip / ca_querymap.hip, whose tiling and summation orders are their own, and nothing with the attention kernels.
//
// Two launches, one stream, no atomics; every output cell and every workspace cell has exactly one writer.
//
// 1. attention (pm_attn_kernel): one workgroup of four waves per (problem, block of 64 query rows, head): a grid over the
//    heads as well, so that one item of 4096 rows and 24 heads is 1536 workgroups.  S^T = K Q^T on v_mfma_f32_16x16x32,
//    the key on the accumulator's row and the query on its column; a wave holds the q fragments of the block's four
//    groups of 16 query rows and walks them against the same 16 keys.  Wave w takes keys 64 t + 16 w + 0..15 of every key
//    tile t = 0, 1, ..; lane group g = lane >> 4 holds the scores of keys 4 g + 0..3 of those 16 for query lane & 15.
//    That is the B layout of v_mfma_f32_16x16x4_f32 (B[k = g][query]), four keys per lane: O[c][query] += sum over the 16
//    keys of v[c][key] p[key][query] is four fp32-input MFMAs per 16 concepts, MFMA e taking key 4 g + e of every lane
//    group, A[c = lane & 15][k = g] = v[c][key 4 g + e] (zero for a leading key, a key past the end or c >= C).  p and v
//    are fp32; the instruction is a k-ordered chain of fused multiply-adds.  The summation order, per head, query row i
//    and wave w (m starts at -3e38, l and O at 0):
//      per tile t ascending:   m' = max(m, the wave's 16 scores of tile t);  a = exp2(m - m');  p = exp2(s - m')
//                              (keys past the end are -inf: p = 0)
//                              per lane group g:  l_g = l_g * a + (((p0 + p1) + p2) + p3)
//                              O[c] = O[c] * a;  then for e = 0..3, for g = 0..3:  O[c] = fma(v[c][key 4 g + e], p, O[c])
//                              m = m'
//      l_w = (l_0 + l_1) + (l_2 + l_3)
//      M = max over the four waves;  every wave:  f = exp2(m - M),  l_w = l_w * f,  O_w[c] = O_w[c] * f
//      L = (l_0 + l_1) + (l_2 + l_3);   O[c] = (O_0[c] + O_1[c]) + (O_2[c] + O_3[c]);   o_h[c, i] = O[c] / L
//    o_h goes to the workspace ([head][c][row] floats per problem).
// 2. head sum (pm_sum_kernel): one thread per cell (c, i): sum = 0 + o_0, sum = sum + o_h in head order, out = sum *
//    (1 / num_heads) and ONE read-modify-write of the cell in each accumulator, acc = fma(weight, out, acc).
// Neither pass depends on the grid or on the other problems: a cell's bits are a function of its own q row, the key rows,
// the map row and (through the wave and lane group a key falls into) the key indices only.
//
// The fragments come straight from global memory (16 bytes per lane; the 256 bytes of a head's row are consumed by the four
// lanes that share the row), the map values as single floats (ldv and n0 are free, so nothing wider is aligned); the next
// tile's loads are issued before the current MFMAs.  The cross-wave reduction goes through 34 KiB of LDS.
// build.py's audit refuses a spill.
#include <math.h>

#include "ca_common.h"
#include "ca_propmap.h"

typedef _Float16 pm_f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t pm_u32x4 __attribute__((ext_vector_type(4)));

namespace {   // device code

constexpr int PM_THREADS = 256;
constexpr int PM_QF = 4;                    // groups of 16 query rows of a workgroup
constexpr int PM_ROWS = 16 * PM_QF;         // query rows of a workgroup
constexpr int PM_TILE = 64;                 // keys of a tile (16 per wave)
constexpr int PM_CT = 2;                    // groups of 16 map rows (CA_PROPMAP_MAX_CONCEPTS / 16)
constexpr float PM_M_INIT = -3.0e38f;       // a finite "no key yet": exp2(-inf - PM_M_INIT) is 0, not NaN
static_assert(PM_CT * 16 == CA_PROPMAP_MAX_CONCEPTS, "the accumulators cover the concept limit");

struct PropmapLaunch {
  ca_propmap_problem p[CA_PROPMAP_MAX_PROBLEMS];
  int64_t ws_off[CA_PROPMAP_MAX_PROBLEMS];   // bytes from workspace to the problem's [num_heads][C][nq] floats
  char *workspace;
  int32_t num_heads;
  float scale_log2, inv_heads;
};

// S^T += K Q^T on v_mfma_f32_16x16x32: the key on the accumulator's row, the query on its column
template <bool F16>
__device__ __forceinline__ f32x4 pm_mfma(pm_u32x4 k, pm_u32x4 q, f32x4 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(pm_f16x8, k), __builtin_bit_cast(pm_f16x8, q), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, k), __builtin_bit_cast(bf16x8, q), c, 0, 0, 0);
}

// the address of key row j (0 <= j < n0 + n1) of a problem, head columns not included
__device__ __forceinline__ const uint16_t *pm_key_row(const ca_propmap_problem &P, int j) {
  return j < P.n0 ? (const uint16_t *)P.k0 + (size_t)j * (size_t)P.ldk
                  : (const uint16_t *)P.k1 + (size_t)(j - P.n0) * (size_t)P.ldk;
}

// a lane's fragment of 16 rows, head h: row (lane & 15) of the 16, columns 8 (lane >> 4) + 32 ks .. of the head
__device__ __forceinline__ void pm_frag_load(const uint16_t *row, int h, pm_u32x4 (&f)[4]) {
  const uint16_t *p = row + (size_t)h * 128 + ((threadIdx.x & 63) >> 4) * 8;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) f[ks] = *(const pm_u32x4 *)(p + ks * 32);
}

// the scores of 16 keys against 16 queries: lane l gets keys 4 (l >> 4) + 0..3 of query l & 15, times scale_log2
template <bool F16>
__device__ __forceinline__ f32x4 pm_scores(const pm_u32x4 (&kf)[4], const pm_u32x4 (&qf)[4], float scale_log2) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) s = pm_mfma<F16>(kf[ks], qf[ks], s);
  return s * scale_log2;
}

// a lane's map values of a wave's 16 keys starting at key j0 (an index into [k0 | k1]): va[ct][e] = v[16 ct + (lane & 15)]
// [j0 + 4 (lane >> 4) + e - n0], zero where the key carries no value (a leading key, a key past the end) or the row is
// past C.  Nothing outside v[c, 0 .. n1) is read.
__device__ __forceinline__ void pm_value_load(const ca_propmap_problem &P, int j0, int nct, float (&va)[PM_CT][4]) {
  const int lane = threadIdx.x & 63;
  const int64_t jb = (int64_t)j0 + (lane >> 4) * 4 - P.n0;
#pragma unroll
  for (int ct = 0; ct < PM_CT; ++ct) {
    const int c = ct * 16 + (lane & 15);
    const float *vr = P.v + (size_t)min(c, P.C - 1) * (size_t)P.ldv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t j = jb + e;
      va[ct][e] = (ct < nct && c < P.C && j >= 0 && j < P.n1) ? vr[j] : 0.f;
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(PM_THREADS) void pm_attn_kernel(PropmapLaunch A) {
  __shared__ float sO[4][PM_QF * PM_CT * 4][64];   // [wave][(f, ct, e)][lane]: a wave's rescaled O
  __shared__ float sM[4][PM_ROWS], sL[4][PM_ROWS];
  const ca_propmap_problem &P = A.p[blockIdx.z];
  const int64_t row0 = (int64_t)blockIdx.x * PM_ROWS;
  if (row0 >= P.nq) return;   // (the grid is sized for the launch's largest problem; whole workgroups leave together)
  const int h = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntot = P.n0 + P.n1, tiles = (ntot + PM_TILE - 1) / PM_TILE;
  const int nf = (int)min((int64_t)PM_QF, (P.nq - row0 + 15) / 16);   // groups of 16 rows that hold a row (wave-uniform)
  const int nct = (P.C + 15) / 16;                                   // groups of 16 map rows that hold one
  pm_u32x4 qf[PM_QF][4], kf[4], kn[4];
#pragma unroll
  for (int f = 0; f < PM_QF; ++f) {                        // (rows past the end repeat the last one and are dropped)
    const int64_t qrow = min(row0 + f * 16 + (lane & 15), (int64_t)P.nq - 1);
    pm_frag_load((const uint16_t *)P.q + (size_t)qrow * (size_t)P.ldq, h, qf[f]);
  }
  // (key rows past the end repeat the last key; their scores are masked)
  pm_frag_load(pm_key_row(P, min(wave * 16 + (lane & 15), ntot - 1)), h, kn);
  float va[PM_CT][4], vn[PM_CT][4];
  pm_value_load(P, wave * 16, nct, vn);
  float m[PM_QF], l[PM_QF];
  f32x4 O[PM_QF][PM_CT];
#pragma unroll
  for (int f = 0; f < PM_QF; ++f) {
    m[f] = PM_M_INIT, l[f] = 0.f;
#pragma unroll
    for (int ct = 0; ct < PM_CT; ++ct) O[f][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int t = 0; t < tiles; ++t) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) kf[ks] = kn[ks];
#pragma unroll
    for (int ct = 0; ct < PM_CT; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) va[ct][e] = vn[ct][e];
    if (t + 1 < tiles) {                                   // the next tile, in flight during this tile's MFMAs
      pm_frag_load(pm_key_row(P, min((t + 1) * PM_TILE + wave * 16 + (lane & 15), ntot - 1)), h, kn);
      pm_value_load(P, (t + 1) * PM_TILE + wave * 16, nct, vn);
    }
#pragma unroll
    for (int f = 0; f < PM_QF; ++f) {
      if (f >= nf) continue;
      f32x4 s = pm_scores<F16>(kf, qf[f], A.scale_log2);
      if (t == tiles - 1) {                                // keys past the end (the last tile only)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (t * PM_TILE + wave * 16 + (lane >> 4) * 4 + e >= ntot) s[e] = -INFINITY;
      }
      float mt = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
      mt = fmaxf(mt, __shfl_xor(mt, 16));
      mt = fmaxf(mt, __shfl_xor(mt, 32));
      const float m_new = fmaxf(m[f], mt);
      const float a = __builtin_amdgcn_exp2f(m[f] - m_new);
      float p[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = __builtin_amdgcn_exp2f(s[e] - m_new);
      l[f] = l[f] * a + (((p[0] + p[1]) + p[2]) + p[3]);
      m[f] = m_new;
#pragma unroll
      for (int ct = 0; ct < PM_CT; ++ct) {
        if (ct >= nct) continue;
        f32x4 o = O[f][ct] * a;
#pragma unroll
        for (int e = 0; e < 4; ++e) o = __builtin_amdgcn_mfma_f32_16x16x4f32(va[ct][e], p[e], o, 0, 0, 0);
        O[f][ct] = o;
      }
    }
  }
  // the four waves' (m, l, O) of every query row, brought to the common maximum and added
#pragma unroll
  for (int f = 0; f < PM_QF; ++f) {
    l[f] += __shfl_xor(l[f], 16);
    l[f] += __shfl_xor(l[f], 32);
    if (lane < 16) sM[wave][f * 16 + lane] = m[f];
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < PM_QF; ++f) {
    const int qq = f * 16 + (lane & 15);
    const float M = fmaxf(fmaxf(sM[0][qq], sM[1][qq]), fmaxf(sM[2][qq], sM[3][qq]));   // (finite: key 0 exists)
    const float sc = __builtin_amdgcn_exp2f(m[f] - M);
    if (lane < 16) sL[wave][qq] = l[f] * sc;
#pragma unroll
    for (int ct = 0; ct < PM_CT; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) sO[wave][(f * PM_CT + ct) * 4 + e][lane] = O[f][ct][e] * sc;
  }
  __syncthreads();
  float *ws = (float *)(A.workspace + A.ws_off[blockIdx.z]);
  for (int idx = threadIdx.x; idx < PM_QF * PM_CT * 4 * 64; idx += PM_THREADS) {
    const int r = idx >> 6, ln = idx & 63;
    const int f = r / (PM_CT * 4), ct = (r >> 2) % PM_CT, e = r & 3;
    const int c = ct * 16 + (ln >> 4) * 4 + e;             // the accumulator's row: 4 (lane >> 4) + register
    const int qq = f * 16 + (ln & 15);
    const int64_t qi = row0 + qq;
    if (c >= P.C || qi >= P.nq) continue;
    const float Ls = (sL[0][qq] + sL[1][qq]) + (sL[2][qq] + sL[3][qq]);
    const float Os = (sO[0][r][ln] + sO[1][r][ln]) + (sO[2][r][ln] + sO[3][r][ln]);
    ws[((size_t)h * (size_t)P.C + c) * (size_t)P.nq + (size_t)qi] = Os / Ls;
  }
}

__global__ __launch_bounds__(PM_THREADS) void pm_sum_kernel(PropmapLaunch A) {
  const ca_propmap_problem &P = A.p[blockIdx.y];
  const int64_t cells = (int64_t)P.C * P.nq;
  const int64_t cell = (int64_t)blockIdx.x * PM_THREADS + threadIdx.x;
  if (cell >= cells) return;   // (the grid is sized for the launch's largest problem)
  const float *ws = (const float *)(A.workspace + A.ws_off[blockIdx.y]) + cell;
  float sum = 0.f;                                         // (0 + o is o: head 0 starts the sum)
  for (int h = 0; h < A.num_heads; ++h) sum += ws[(size_t)h * (size_t)cells];
  const float out = sum * A.inv_heads;
  if (P.acc) P.acc[cell] = __builtin_fmaf(P.weight, out, P.acc[cell]);
  if (P.acc2) P.acc2[cell] = __builtin_fmaf(P.weight2, out, P.acc2[cell]);
}

int64_t pm_problem_bytes(const ca_propmap_problem &p, int32_t num_heads) {
  return ((int64_t)num_heads * p.C * p.nq * 4 + 15) & ~(int64_t)15;
}

// the argument rules of both entry points; 0 or CA_ERR_ARG with the text under FN
int pm_check(const char *FN, const ca_propmap_problem *problems, int32_t n_problems, int32_t num_heads) {
  if (!problems || n_problems < 1 || n_problems > CA_PROPMAP_MAX_PROBLEMS || num_heads < 1 || num_heads > CA_PROPMAP_MAX_HEADS) {
    ca_set_error("%s: bad arguments (n_problems=%d num_heads=%d; need 1 <= n_problems <= %d, 1 <= num_heads <= %d)", FN,
                 n_problems, num_heads, CA_PROPMAP_MAX_PROBLEMS, CA_PROPMAP_MAX_HEADS);
    return CA_ERR_ARG;
  }
  const int64_t width = (int64_t)num_heads * 128;
  for (int i = 0; i < n_problems; ++i) {
    const ca_propmap_problem &p = problems[i];
    // (n0 + n1 leaves room for the round-up to whole key tiles in 32-bit arithmetic)
    if (p.nq < 1 || p.n0 < 0 || p.n1 < 1 || (int64_t)p.n0 + p.n1 > CA_PROPMAP_MAX_ROWS || p.C < 1 ||
        p.C > CA_PROPMAP_MAX_CONCEPTS) {
      ca_set_error("%s: problem %d sizes invalid (nq=%d n0=%d n1=%d C=%d; need nq >= 1, n0 >= 0, n1 >= 1, n0 + n1 <= %d, "
                   "1 <= C <= %d)", FN, i, p.nq, p.n0, p.n1, p.C, CA_PROPMAP_MAX_ROWS, CA_PROPMAP_MAX_CONCEPTS);
      return CA_ERR_ARG;
    }
    if (!p.q || !p.k1 || (p.n0 > 0 && !p.k0) || (((uintptr_t)p.q | (uintptr_t)p.k0 | (uintptr_t)p.k1) & 15) || p.ldq < width ||
        p.ldk < width || p.ldq % 8 || p.ldk % 8) {
      ca_set_error("%s: problem %d rows invalid (ldq=%d ldk=%d; q, k1 and, with n0 > 0, k0 non-null and 16-byte aligned, row "
                   "strides >= num_heads*128 = %lld and a multiple of 8)", FN, i, p.ldq, p.ldk, (long long)width);
      return CA_ERR_ARG;
    }
    if (!p.v || ((uintptr_t)p.v & 3) || p.ldv < p.n1) {
      ca_set_error("%s: problem %d maps invalid (ldv=%d n1=%d; v non-null and 4-byte aligned, ldv >= n1)", FN, i, p.ldv, p.n1);
      return CA_ERR_ARG;
    }
    if ((!p.acc && !p.acc2) || (((uintptr_t)p.acc | (uintptr_t)p.acc2) & 3)) {
      ca_set_error("%s: problem %d outputs invalid (at least one of acc / acc2; acc and acc2 4-byte aligned)", FN, i);
      return CA_ERR_ARG;
    }
  }
  return CA_OK;
}

}  // namespace

extern "C" int64_t ca_propagate_maps_workspace_bytes(const ca_propmap_problem *problems, int32_t n_problems, int32_t num_heads) {
  if (pm_check("ca_propagate_maps: workspace_bytes", problems, n_problems, num_heads) != CA_OK) return CA_ERR_ARG;
  int64_t need = 0;
  for (int i = 0; i < n_problems; ++i) need += pm_problem_bytes(problems[i], num_heads);
  return need;
}

extern "C" int ca_propagate_maps(const ca_propmap_problem *problems, int32_t n_problems, int32_t num_heads, float scale_log2,
                                 int32_t flags, void *workspace, int64_t workspace_bytes, ca_stream_t stream) {
  const char *FN = "ca_propagate_maps";
  if (pm_check(FN, problems, n_problems, num_heads) != CA_OK) return CA_ERR_ARG;
  if (!isfinite(scale_log2) || (flags & ~CA_PROPMAP_QK_F16)) {
    ca_set_error("%s: bad arguments (scale_log2=%g flags=%d; need a finite scale_log2, flags 0 or %d)", FN, (double)scale_log2,
                 flags, CA_PROPMAP_QK_F16);
    return CA_ERR_ARG;
  }
  PropmapLaunch A = {};
  int64_t need = 0, max_cells = 0;
  int max_nq = 0;
  for (int i = 0; i < n_problems; ++i) {
    A.p[i] = problems[i];
    A.ws_off[i] = need;
    need += pm_problem_bytes(problems[i], num_heads);
    max_nq = problems[i].nq > max_nq ? problems[i].nq : max_nq;
    const int64_t cells = (int64_t)problems[i].C * problems[i].nq;
    max_cells = cells > max_cells ? cells : max_cells;
  }
  if (workspace_bytes < need || !workspace || ((uintptr_t)workspace & 15)) {
    ca_set_error("%s: workspace too small (workspace_bytes=%lld, ca_propagate_maps_workspace_bytes says %lld; non-null and "
                 "16-byte aligned)", FN, (long long)workspace_bytes, (long long)need);
    return CA_ERR_ARG;
  }
  A.workspace = (char *)workspace;
  A.num_heads = num_heads, A.scale_log2 = scale_log2, A.inv_heads = 1.0f / (float)num_heads;
  const bool f16 = (flags & CA_PROPMAP_QK_F16) != 0;
  const unsigned qblocks = (unsigned)(((int64_t)max_nq + PM_ROWS - 1) / PM_ROWS);
  hipLaunchKernelGGL(f16 ? pm_attn_kernel<true> : pm_attn_kernel<false>, dim3(qblocks, (unsigned)num_heads, (unsigned)n_problems),
                     dim3(PM_THREADS), 0, (hipStream_t)stream, A);
  const int rc = ca_check_launch(FN);
  if (rc != CA_OK) return rc;
  const unsigned cblocks = (unsigned)((max_cells + PM_THREADS - 1) / PM_THREADS);
  hipLaunchKernelGGL(pm_sum_kernel, dim3(cblocks, (unsigned)n_problems), dim3(PM_THREADS), 0, (hipStream_t)stream, A);
  return ca_check_launch(FN);
}
