// ca_heatmap_many: the heat maps of one layer for up to CA_HEATMAP_MAX_CONCEPTS (32) concepts in ONE launch, and the sparse
// weighting kernels of the three-launch form at 17 .. 32 concepts.  The arithmetic is ca_heatmap_core.h's, shared with
// ca_rowops.hip: bit-identical to ca_heatmap_logits_bf16 + ca_heatmap_norm_accumulate, and to ca_heatmap_fused at C <= 8.
#include <atomic>

#include "ca_common.h"
#include "ca_heatmap_core.h"

namespace {   // device code

// ------------------------------------------------------------------------------------------
// Heat maps of one layer for up to CA_HEATMAP_MAX_CONCEPTS concepts (ca_heatmap_many): ca_heatmap_fused's work with the
// concept vectors going through LDS in ceil(C / 8) chunks of equal height (C = 9: 5 + 4 rows, C = 32: 4 x 8).  Eight
// waves take 16 patches per pass, two each; a wave reads its two image rows ONCE per pass and keeps them in registers
// as floats (2 x dim / 64 VGPRs) while the chunks go by, so the image rows cross the memory system once whatever C is.
// Per chunk: the workgroup fills LDS, then every wave forms one (patch, concept) chain at a time, ca_heatmap_logits_kernel's
// (lane l: k = 8 l + 512 i in i order, then the wave sum), and lanes 0 / 1 park their patch's logit in a 2 KB LDS table.
// After the last chunk those two lanes take their patch's C logits out of the table and weight them with the three-launch
// kernels' expressions (hm_weight_and_accumulate<CW>, CW = 8 / 16 / 32 as ca_heatmap_norm_accumulate picks it).  With one
// chunk (C <= 8) LDS is filled once per workgroup, as in ca_heatmap_fused.  LDS: the table, eight zeros, the chunk.
constexpr int HM_MANY_THREADS = 512;
constexpr int HM_MANY_TABLE = HM_MANY_THREADS / 64 * 2 * CA_HEATMAP_MAX_CONCEPTS;   // floats: [wave][patch][concept]

// a wave's two image rows as floats, NP pieces of 8 per lane; a lane's pieces past the end of the row are zeros (read
// from the start of the row and discarded), so that the chains below need no branch per piece
template <int NP, typename IT>
__device__ __forceinline__ void hm_many_rows(const IT *ir0, const IT *ir1, int lane, int dim, float (&x0)[NP][8],
                                             float (&x1)[NP][8]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const bool valid = lane * 8 + 512 * i < dim;
    const int k = valid ? lane * 8 + 512 * i : 0;
    load8(ir0 + k, x0[i]);
    load8(ir1 + k, x1[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x0[i][j] = valid ? x0[i][j] : 0.f;
      x1[i][j] = valid ? x1[i][j] : 0.f;
    }
  }
}

template <int CW, int NP>
__device__ __forceinline__ void heatmap_many_body(const ca_heatmap_problem &P, int L, int C, int dim, int norm,
                                                  float *zl, float *cs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (C + 7) / 8, h = (C + nch - 1) / nch;   // chunks and their height (the last one may be lower)
  float *zw = zl + (wave * 2 + (lane & 1)) * CA_HEATMAP_MAX_CONCEPTS;   // lanes 0 / 1: their patch's logits
  const float *zero8 = zl + HM_MANY_TABLE;                               // eight zeros: what a piece past the row reads
  if (threadIdx.x < 8) zl[HM_MANY_TABLE + threadIdx.x] = 0.f;           // (visible after the first fill's barriers)
  const int p_first = blockIdx.x * (HM_MANY_THREADS / 64 * 2);
  // (the trip count is the same for all eight waves: they meet at the barriers around every LDS fill)
  for (int p0 = p_first; p0 < L; p0 += gridDim.x * (HM_MANY_THREADS / 64 * 2)) {
    const int p = p0 + wave * 2;   // (a wave past the end repeats patch L - 1 and drops the result: no branch around
                                   // the row registers)
    const size_t r0 = (size_t)min(p, L - 1) * P.ldi, r1 = (size_t)min(p + 1, L - 1) * P.ldi;
    float x0[NP][8], x1[NP][8];
    if (P.img_f32) hm_many_rows<NP>((const float *)P.img_vec + r0, (const float *)P.img_vec + r1, lane, dim, x0, x1);
    else hm_many_rows<NP>((const bf16 *)P.img_vec + r0, (const bf16 *)P.img_vec + r1, lane, dim, x0, x1);
    for (int ch = 0; ch < nch; ++ch) {
      const int c0 = ch * h, hc = min(h, C - c0);
      if (nch > 1 || p0 == p_first) {
        __syncthreads();   // (the previous chunk's readers are done)
        for (int c = 0; c < hc; ++c) {
          for (int k = threadIdx.x * 4; k < dim; k += HM_MANY_THREADS * 4) {
            f32x4 v;
            if (P.con_f32) {
              v = *(const f32x4 *)((const float *)P.con_vec + (size_t)(c0 + c) * P.ldc + k);
            } else {
              const bf16x4 t = *(const bf16x4 *)((const bf16 *)P.con_vec + (size_t)(c0 + c) * P.ldc + k);
              v = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
            }
            *(f32x4 *)(cs + c * dim + k) = v;
          }
        }
        __syncthreads();
      }
      // one chain per (patch, concept), a concept at a time (rows past the chunk's height are skipped, wave-uniformly).
      // A piece past the end of the row multiplies zeros by zeros: fma(0, 0, a) = a, bit for bit (a is never -0).
      for (int c = 0; c < hc; ++c) {
        const float *cr = cs + c * dim + lane * 8;
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const float *bp = lane * 8 + 512 * i < dim ? cr + 512 * i : zero8;
          const f32x4 b0 = *(const f32x4 *)bp, b1 = *(const f32x4 *)(bp + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {   // (ca_heatmap_logits_kernel's order)
            a0 = fmaf(x0[i][j], b0[j], a0);
            a0 = fmaf(x0[i][4 + j], b1[j], a0);
            a1 = fmaf(x1[i][j], b0[j], a1);
            a1 = fmaf(x1[i][4 + j], b1[j], a1);
          }
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        if (lane < 2) zw[c0 + c] = lane ? a1 : a0;
      }
    }
    const int pp = p + lane;
    if (lane < 2 && pp < L) {
      float z[CW];
#pragma unroll
      for (int c = 0; c < CW; ++c) z[c] = c < C ? zw[c] : 0.f;   // (what this lane wrote itself)
      hm_weight_and_accumulate<CW>(P, z, pp, L, C, norm);
    }
  }
}

template <int CW>
__global__ __launch_bounds__(HM_MANY_THREADS) void ca_heatmap_many_kernel(HeatmapLaunch A) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float *zl = (float *)smem_raw;            // [8 waves][2 patches][32 concepts], then eight zeros
  float *cs = zl + HM_MANY_TABLE + 8;       // [chunk height][dim]
  const ca_heatmap_problem &P = A.p[blockIdx.y];
  if (A.dim <= 3072) heatmap_many_body<CW, 6>(P, A.L, A.C, A.dim, A.norm, zl, cs);   // (the model's dim: 6 pieces of 512)
  else heatmap_many_body<CW, 8>(P, A.L, A.C, A.dim, A.norm, zl, cs);
}

}  // namespace

int ca_heatmap_sparse32(const char *FN, const float *logits, int32_t C, int32_t L, int32_t norm, float weight, float *acc,
                        ca_stream_t stream) {
  return launch(norm == CA_NORM_ENTMAX15 ? ca_heatmap_sparse_kernel<32, true> : ca_heatmap_sparse_kernel<32, false>,
                grid_1d(L, 256), 256, 0, stream, FN, logits, C, L, weight, acc);
}

extern "C" int ca_heatmap_many(const ca_heatmap_problem *problems, int32_t n_problems, int32_t L, int32_t C,
                               int32_t dim, int32_t norm, ca_stream_t stream) {
  if (!problems || n_problems < 1 || n_problems > CA_HEATMAP_MAX_PROBLEMS || L < 1 || C < 1 ||
      C > CA_HEATMAP_MAX_CONCEPTS || dim < 8 || dim % 8 || dim > 4096 ||
      (norm != CA_NORM_SOFTMAX && norm != CA_NORM_SPARSEMAX && norm != CA_NORM_ENTMAX15)) {
    ca_set_error("ca_heatmap_many: bad arguments (n_problems=%d L=%d C=%d dim=%d norm=%d; need n_problems <= %d, C <= %d, "
                 "dim %% 8 == 0, dim <= 4096)", n_problems, L, C, dim, norm, CA_HEATMAP_MAX_PROBLEMS,
                 CA_HEATMAP_MAX_CONCEPTS);
    return CA_ERR_ARG;
  }
  HeatmapLaunch A = {};
  A.L = L, A.C = C, A.dim = dim, A.norm = norm;
  for (int i = 0; i < n_problems; ++i) {
    const ca_heatmap_problem &p = problems[i];
    if (!p.img_vec || !p.con_vec || (!p.acc && !p.acc2 && !p.logits) ||
        (((uintptr_t)p.img_vec | (uintptr_t)p.con_vec) & 15) ||
        (((uintptr_t)p.acc | (uintptr_t)p.acc2 | (uintptr_t)p.logits) & 3) || (p.img_f32 & ~1) || (p.con_f32 & ~1) ||
        p.ldi < dim || p.ldc < dim || p.ldi % (p.img_f32 ? 4 : 8) || p.ldc % 4) {
      ca_set_error("ca_heatmap_many: problem %d invalid (ldi=%d ldc=%d img_f32=%d con_f32=%d; vectors 16-byte aligned, "
                   "img_f32 0 or 1 (no per-head partials), at least one of acc / acc2 / logits)", i, p.ldi, p.ldc,
                   p.img_f32, p.con_f32);
      return CA_ERR_ARG;
    }
    A.p[i] = p;
  }
  const int nch = (C + 7) / 8, h = (C + nch - 1) / nch;
  const size_t lds = ((size_t)HM_MANY_TABLE + 8 + (size_t)h * dim) * sizeof(float);
  if (lds > 64 * 1024) {   // 6 or more rows per chunk at the model's dim: above the default dynamic LDS limit
    static std::atomic<unsigned long long> attr_done{0};
    const int rc = ca_raise_lds_limit({(const void *)ca_heatmap_many_kernel<8>, (const void *)ca_heatmap_many_kernel<16>,
                                       (const void *)ca_heatmap_many_kernel<32>},
                                      (HM_MANY_TABLE + 8 + 8 * 4096) * (int)sizeof(float), attr_done, "ca_heatmap_many");
    if (rc != CA_OK) return rc;
  }
  // workgroups per problem: 16 patches per pass; about 2 workgroups per CU in all, as in ca_heatmap_fused
  const int n_cu = ca_cu_count() > 0 ? ca_cu_count() : 256;
  const unsigned gx = grid_1d(L, HM_MANY_THREADS / 64 * 2, (2 * n_cu + n_problems - 1) / n_problems);
  const auto kernel = C <= 8 ? ca_heatmap_many_kernel<8> : C <= 16 ? ca_heatmap_many_kernel<16> : ca_heatmap_many_kernel<32>;
  return launch(kernel, dim3(gx, n_problems), HM_MANY_THREADS, lds, stream, "ca_heatmap_many", A);
}
