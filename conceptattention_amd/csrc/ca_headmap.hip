// ca_head_maps: per-head concept maps (semantics: ca_headmap.h).  One translation unit of its own; it reads rows a forward
// has already written and shares ca_heatmap_core.h's weighting (hm_softmax_terms / hm_sparse_terms, called as they stand)
// with the other heat-map forms.
//
// Layout.  A workgroup of eight waves (four above 16 concepts) takes two consecutive patches per wave and pass.  The
// hidden width is walked in chunks of 512 columns = 4 heads, chunk loop OUTERMOST: per chunk the workgroup puts all C
// concept rows' 512 columns into LDS as floats (C x 2 KB, 64 KB at C = 32), and every wave reads its two patches' 512
// columns with one load8 per lane (lane l: columns 8 l .. 8 l + 7 of the chunk).  A head is then the 16 consecutive lanes
// g = l >> 4 of a wave, and chunk j holds heads 4 j + g.  Every image row crosses the memory system once.  Per patch only
// the chunk's 8 values, z[C], w[C] and the running head sum m[C] live in registers.
//
// The summation order, fixed (the CPU emulation of tests/headmap_cases.py follows it):
//   z      lane t = l & 15 of a head: a = 0; a = fma(img[k], con[k], a) for k = 8 t .. 8 t + 7 in that order; then the
//          butterfly a += shfl_xor(a, 1), (a, 2), (a, 4), (a, 8): all 16 lanes end with the same bits
//   w      hm_softmax_terms then w = v * (1 / sum);  hm_sparse_terms as is;  CA_NORM_NONE: w = z
//   heads  heads[h, c, p] = fma(weight_h, w, heads[h, c, p])
//   mean   lane group g: m = 0; m += w of head 4 j + g for j = 0, 1, .. (heads past the last one add nothing); then
//          m += shfl_xor(m, 16), m += shfl_xor(m, 32), i.e. (G0 + G1) + (G2 + G3); mean = m * (1.0f / num_heads)
//   acc    acc[c, p] = fma(weight, mean, acc[c, p]);  acc2 the same with weight2
// A lane group whose head lies past the last one (a ragged last chunk) re-reads the chunk's first head and drops the
// result, so nothing past a row's width is ever read.  A wave whose patch lies past L repeats patch L - 1 and stores
// nothing.  No atomics: a patch belongs to one wave.  All row and output offsets are formed in 64 bits.
#include "ca_common.h"
#include "ca_heatmap_core.h"
#include "ca_headmap.h"

namespace {   // device code

// threads of a workgroup: 512 up to 16 concepts; 256 beyond, where z, w, the sort's two copies and two patches' head sums
// (6 x 32 floats) need more than the 256 registers a wave of a 512-thread workgroup can have
template <int CW> constexpr int HD_THREADS = CW <= 16 ? 512 : 256;
constexpr int HD_CHUNK = 512;                     // columns of a chunk: 4 heads of 128

struct HeadmapLaunch {
  ca_headmap_problem p[CA_HEATMAP_MAX_PROBLEMS];
  int32_t L, C, num_heads, norm;
  float inv_heads;
};

// the weights of one head's C logits across the concepts
template <int CW>
__device__ __forceinline__ void hd_weights(const float (&z)[CW], int C, int norm, float (&w)[CW]) {
  if (norm == CA_NORM_NONE) {
#pragma unroll
    for (int c = 0; c < CW; ++c) w[c] = z[c];
  } else if (norm == CA_NORM_SOFTMAX) {
    float sum;
    hm_softmax_terms<CW>(z, C, w, sum);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int c = 0; c < CW; ++c) w[c] *= inv;
  } else if (norm == CA_NORM_SPARSEMAX) {
    hm_sparse_terms<CW, false>(z, C, w);
  } else {
    hm_sparse_terms<CW, true>(z, C, w);
  }
}

// lane t (0 .. 15) takes concepts t and t + 16 out of a register array every lane of its group holds alike
template <int CW>
__device__ __forceinline__ void hd_pick(const float (&w)[CW], int t, float &lo, float &hi) {
  lo = hi = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    if (c < CW) lo = t == c ? w[c] : lo;
    if (c + 16 < CW) hi = t == c ? w[c + 16] : hi;
  }
}

// one patch's share of one chunk: the logits of the lane group's head against the C concept rows in LDS, their weights, the
// head-resolved update and the running head sum
template <int CW>
__device__ __forceinline__ void hd_patch(const ca_headmap_problem &P, const float (&x)[8], const float *cr, int C, int norm,
                                         bool live, int h, int t, int64_t p, bool store, int64_t L, float (&m)[CW]) {
#pragma clang fp contract(off)   // (every product below that is meant to be fused is written as fmaf)
  float z[CW], w[CW];
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    float a = 0.f;
    if (c < C) {   // (wave-uniform)
      const f32x4 b0 = *(const f32x4 *)(cr + c * HD_CHUNK), b1 = *(const f32x4 *)(cr + c * HD_CHUNK + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) a = __builtin_fmaf(x[k], b0[k], a);
#pragma unroll
      for (int k = 0; k < 4; ++k) a = __builtin_fmaf(x[4 + k], b1[k], a);
#pragma unroll
      for (int o = 1; o <= 8; o <<= 1) a += __shfl_xor(a, o);
    }
    z[c] = a;
  }
  hd_weights<CW>(z, C, norm, w);
#pragma unroll
  for (int c = 0; c < CW; ++c) m[c] = live ? m[c] + w[c] : m[c];
  if (P.heads && live && store) {
    float lo, hi;
    hd_pick<CW>(w, t, lo, hi);
    float *o = P.heads + ((size_t)h * (size_t)C + (size_t)t) * (size_t)L + (size_t)p;
    if (t < C) *o = __builtin_fmaf(P.weight_h, lo, *o);
    if (CW > 16 && t + 16 < C) {
      o += (size_t)16 * (size_t)L;
      *o = __builtin_fmaf(P.weight_h, hi, *o);
    }
  }
}

// the end of a patch: the four lane groups' head sums, the mean, and the update of acc / acc2 by lanes 0 .. 15
template <int CW>
__device__ __forceinline__ void hd_finish(const ca_headmap_problem &P, float (&m)[CW], int C, float inv_heads, int lane,
                                          int64_t p, bool store, int64_t L) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    m[c] += __shfl_xor(m[c], 16);
    m[c] += __shfl_xor(m[c], 32);
  }
  if (lane < 16 && store) {
    float lo, hi;
    hd_pick<CW>(m, lane, lo, hi);
    lo *= inv_heads, hi *= inv_heads;
    const size_t o = (size_t)lane * (size_t)L + (size_t)p, o16 = o + (size_t)16 * (size_t)L;
    if (lane < C) {
      if (P.acc) P.acc[o] = __builtin_fmaf(P.weight, lo, P.acc[o]);
      if (P.acc2) P.acc2[o] = __builtin_fmaf(P.weight2, lo, P.acc2[o]);
    }
    if (CW > 16 && lane + 16 < C) {
      if (P.acc) P.acc[o16] = __builtin_fmaf(P.weight, hi, P.acc[o16]);
      if (P.acc2) P.acc2[o16] = __builtin_fmaf(P.weight2, hi, P.acc2[o16]);
    }
  }
}

template <typename T>
__device__ __forceinline__ void hd_row8(const void *base, int64_t row, int32_t ld, int col, float (&x)[8]) {
  load8((const T *)base + (size_t)row * (size_t)ld + (size_t)col, x);
}

template <int CW>
__global__ __launch_bounds__(HD_THREADS<CW>) void ca_headmap_kernel(HeadmapLaunch A) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float *cs = (float *)smem_raw;   // [C][512]: the chunk of every concept row
  const ca_headmap_problem &P = A.p[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int C = A.C, NH = A.num_heads, norm = A.norm;
  const int64_t L = A.L;
  const int nchunks = (NH + 3) / 4;
  constexpr int NT = HD_THREADS<CW>, HD_PATCHES = NT / 64 * 2;   // patches of a workgroup per pass
  // (the trip count is the same for all waves: they meet at the barriers around every LDS fill)
  for (int64_t p0 = (int64_t)blockIdx.x * HD_PATCHES; p0 < L; p0 += (int64_t)gridDim.x * HD_PATCHES) {
    const int64_t pa = p0 + wave * 2, pb = pa + 1;
    const int64_t ra = pa < L ? pa : L - 1, rb = pb < L ? pb : L - 1;
    float m0[CW], m1[CW];
#pragma unroll
    for (int c = 0; c < CW; ++c) m0[c] = m1[c] = 0.f;
    for (int j = 0; j < nchunks; ++j) {
      const int h = 4 * j + g;
      const bool live = h < NH;
      const int col = (live ? h : 4 * j) * 128 + t * 8;
      float x0[8], x1[8];   // in flight while the chunk is filled
      if (P.img_f32) hd_row8<float>(P.img, ra, P.ldi, col, x0), hd_row8<float>(P.img, rb, P.ldi, col, x1);
      else hd_row8<bf16>(P.img, ra, P.ldi, col, x0), hd_row8<bf16>(P.img, rb, P.ldi, col, x1);
      __syncthreads();   // (the previous chunk's readers are done)
      {
        const int valid = min(HD_CHUNK, NH * 128 - j * HD_CHUNK);   // columns of this chunk inside the width
        const int k = (threadIdx.x & 127) * 4;
        if (k < valid) {
          for (int c = threadIdx.x >> 7; c < C; c += NT / 128) {
            const size_t at = (size_t)c * (size_t)P.ldc + (size_t)j * HD_CHUNK + (size_t)k;
            f32x4 v;
            if (P.con_f32) {
              v = *(const f32x4 *)((const float *)P.con + at);
            } else {
              const bf16x4 b = *(const bf16x4 *)((const bf16 *)P.con + at);
              v = f32x4{(float)b[0], (float)b[1], (float)b[2], (float)b[3]};
            }
            *(f32x4 *)(cs + c * HD_CHUNK + k) = v;
          }
        }
      }
      __syncthreads();
      const float *cr = cs + (live ? lane : t) * 8;
      hd_patch<CW>(P, x0, cr, C, norm, live, h, t, pa, pa < L, L, m0);
      hd_patch<CW>(P, x1, cr, C, norm, live, h, t, pb, pb < L, L, m1);
    }
    if (P.acc || P.acc2) {
      hd_finish<CW>(P, m0, C, A.inv_heads, lane, pa, pa < L, L);
      hd_finish<CW>(P, m1, C, A.inv_heads, lane, pb, pb < L, L);
    }
  }
}

}  // namespace

extern "C" int ca_head_maps(const ca_headmap_problem *problems, int32_t n_problems, int32_t L, int32_t C, int32_t num_heads,
                            int32_t norm, ca_stream_t stream) {
  const char *FN = "ca_head_maps";
  if (!problems || n_problems < 1 || n_problems > CA_HEATMAP_MAX_PROBLEMS || L < 1 || C < 1 || C > CA_HEATMAP_MAX_CONCEPTS ||
      num_heads < 1 || num_heads > CA_HEADMAP_MAX_HEADS ||
      (norm != CA_NORM_NONE && norm != CA_NORM_SOFTMAX && norm != CA_NORM_SPARSEMAX && norm != CA_NORM_ENTMAX15)) {
    ca_set_error("%s: bad arguments (n_problems=%d L=%d C=%d num_heads=%d norm=%d; need 1 <= n_problems <= %d, L >= 1, "
                 "1 <= C <= %d, 1 <= num_heads <= %d, norm 0 .. 3)", FN, n_problems, L, C, num_heads, norm,
                 CA_HEATMAP_MAX_PROBLEMS, CA_HEATMAP_MAX_CONCEPTS, CA_HEADMAP_MAX_HEADS);
    return CA_ERR_ARG;
  }
  const int64_t width = (int64_t)num_heads * 128;
  HeadmapLaunch A = {};
  A.L = L, A.C = C, A.num_heads = num_heads, A.norm = norm, A.inv_heads = 1.0f / (float)num_heads;
  for (int i = 0; i < n_problems; ++i) {
    const ca_headmap_problem &p = problems[i];
    if (!p.img || !p.con || (((uintptr_t)p.img | (uintptr_t)p.con) & 15) || (p.img_f32 & ~1) || (p.con_f32 & ~1) ||
        p.ldi < width || p.ldc < width || p.ldi % (p.img_f32 ? 4 : 8) || p.ldc % (p.con_f32 ? 4 : 8)) {
      ca_set_error("%s: problem %d rows invalid (ldi=%d ldc=%d img_f32=%d con_f32=%d; img and con non-null and 16-byte "
                   "aligned, img_f32 / con_f32 0 or 1, row strides >= num_heads*128 = %lld and a multiple of 8 (bf16) or "
                   "4 (fp32))", FN, i, p.ldi, p.ldc, p.img_f32, p.con_f32, (long long)width);
      return CA_ERR_ARG;
    }
    if ((!p.heads && !p.acc && !p.acc2) || (((uintptr_t)p.heads | (uintptr_t)p.acc | (uintptr_t)p.acc2) & 3)) {
      ca_set_error("%s: problem %d outputs invalid (at least one of heads / acc / acc2; all three 4-byte aligned)", FN, i);
      return CA_ERR_ARG;
    }
    for (int k = 0; k < i; ++k) {
      const ca_headmap_problem &q = problems[k];
      for (const float *a : {p.heads, p.acc, p.acc2})
        if (a && (a == q.heads || a == q.acc || a == q.acc2)) {
          ca_set_error("%s: problem %d shares an accumulator with problem %d (their updates would race)", FN, i, k);
          return CA_ERR_ARG;
        }
    }
    if ((p.acc && (p.acc == p.acc2 || p.acc == p.heads)) || (p.acc2 && p.acc2 == p.heads)) {
      ca_set_error("%s: problem %d names one accumulator twice", FN, i);
      return CA_ERR_ARG;
    }
    A.p[i] = p;
  }
  const size_t lds = (size_t)C * HD_CHUNK * sizeof(float);   // (at most 64 KB: inside the default dynamic LDS limit)
  // workgroups per problem: two patches per wave and pass; about 2 workgroups per CU in all, as in ca_heatmap_many
  const int n_cu = ca_cu_count() > 0 ? ca_cu_count() : 256;
  const int threads = C <= 8 ? HD_THREADS<8> : C <= 16 ? HD_THREADS<16> : HD_THREADS<32>;
  const unsigned gx = grid_1d(L, threads / 64 * 2, (2 * n_cu + n_problems - 1) / n_problems);
  const auto kernel = C <= 8 ? ca_headmap_kernel<8> : C <= 16 ? ca_headmap_kernel<16> : ca_headmap_kernel<32>;
  return launch(kernel, dim3(gx, n_problems), threads, lds, stream, FN, A);
}
