// What the two text-encoder units (ca_t5.hip, ca_clip.hip) share, stated once: the tile and the steps of their attention
// kernels, the 4-wave row reductions, the walk of the elementwise kernels, the two launch-size rules and the row-scale
// step of the e4m3 producers.  Device functions are __forceinline__ and run in the including kernel; nothing here is a
// kernel or a launch.  Every value is formed by the operations, and in the order, written here: the summation tree of
// tx_block_sum and the key permutation of tx_pv decide bits (tests/test_text_parent_records_gpu.py pins them).
#pragma once
#include "ca_common.h"

// ------------------------------------------------------------------------------------------------------------------
// The attention tile: out = softmax(f(q k^T)) v per (sequence, head) with f the including kernel's (T5: + bias; CLIP:
// scale and causal mask).
//
// A workgroup of 4 waves owns 64 query rows of one (sequence, head); a wave owns 16 of them.  K of the head sits in LDS
// row-major ([key][64], rows of 72 bf16 so that the 16 rows of a ds_read_b128 fragment read fall on 16 distinct 16-byte
// slots), V transposed ([d][key], rows of LP + 16 bf16 for LP staged keys) because P V contracts over the keys and an MFMA
// operand wants its 8 contraction elements contiguous in a lane.
//
// Scores are computed transposed, S^T = K Q^T: with K as the MFMA's A operand and Q as B, a lane ends up with ONE query
// (lane & 15) and keys 16 t + 4 (lane >> 4) + 0..3 of every 16-key tile t.  All scores of the wave's 16 queries are
// held in registers (LP / 4 floats per lane), so the softmax is the exact two-pass one: row maximum, then exp and sum,
// each finished by two cross-lane exchanges over the 4 lanes of a query.  The same registers, rounded to bf16, are the
// B operand of O^T = V^T P^T: the contraction slot (g, e) of 32-key step u stands for key 32 u + 4 g + e (e < 4) or
// 32 u + 16 + 4 g + e - 4 (e >= 4), and the V^T fragment is read from LDS under the same permutation.  The lane's
// query is the same in both products, so 1 / sum is a per-lane scalar.  P is rounded to bf16 unnormalised (in [0, 1]);
// the sum is taken over the fp32 values.
#define TX_D 64      // the head dim
#define TX_LDK 72    // bf16 per K row in LDS (the bank-slot reason above)

// K [LP][TX_LDK], then V^T [64][LP + 16]; returns what follows them (T5: the bias row)
__device__ __forceinline__ void *tx_carve(int LP, bf16 *&sK, bf16 *&sV) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tx_smem[];
  sK = (bf16 *)tx_smem;
  sV = sK + LP * TX_LDK;
  return sV + TX_D * (LP + 16);
}

static int tx_attn_lds_bytes(int LP, int extra_floats) { return LP * TX_LDK * 2 + TX_D * (LP + 16) * 2 + extra_floats * 4; }

// K and V^T of keys 0 .. nkeys - 1 (a multiple of 32) into LDS; positions >= limit are zeros and touch no memory (a
// masked probability of 0 times a NaN in V would be NaN).  With limit >= nkeys known at compile time the tests fold away.
template <int LDV>   // bf16 per V^T row in LDS
__device__ __forceinline__ void tx_stage_kv(const bf16 *k, const bf16 *v, long row0, long col, long ldk, long ldv, bf16 *sK,
                                            bf16 *sV, int nkeys, int limit) {
  const int tid = threadIdx.x, c = tid & 7;
#pragma unroll 4
  for (int r = tid >> 3; r < nkeys; r += 32) {
    uint4 x = {0u, 0u, 0u, 0u};
    if (r < limit) x = *(const uint4 *)(k + (row0 + r) * ldk + col + c * 8);
    *(uint4 *)(sK + r * TX_LDK + c * 8) = x;
  }
  const int kp0 = tid & 31, cv = tid >> 5;           // key pair within a 64-key slab, 8-column chunk
#pragma unroll 2
  for (int kp = kp0; kp < nkeys / 2; kp += 32) {
    bf16x8 a, b;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = b[i] = (bf16)0.f;
    if (2 * kp < limit) a = *(const bf16x8 *)(v + (row0 + 2 * kp) * ldv + col + cv * 8);
    if (2 * kp + 1 < limit) b = *(const bf16x8 *)(v + (row0 + 2 * kp + 1) * ldv + col + cv * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      bf16x2 pr = {a[i], b[i]};
      *(bf16x2 *)(sV + (cv * 8 + i) * LDV + 2 * kp) = pr;
    }
  }
}

// the lane's query row (g = lane >> 4 picks its 8-element pieces) as the B operand of S^T = K Q^T.  The position must
// exist: a kernel with positions >= L (CLIP) keeps zeros there itself, because T5's test would not fold away.
__device__ __forceinline__ void tx_load_q(const bf16 *q, long row0, int qpos, long ldq, long col, int g, bf16x8 (&qf)[2]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) qf[kk] = *(const bf16x8 *)(q + (row0 + qpos) * ldq + col + kk * 32 + g * 8);
}

// the scores of query j = lane & 15 against keys 16 t + 4 g + 0..3: two MFMAs over the 64 dimensions
__device__ __forceinline__ f32x4 tx_score_tile(const bf16 *sK, int t, int j, int g, const bf16x8 (&qf)[2]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const bf16x8 kf = *(const bf16x8 *)(sK + (t * 16 + j) * TX_LDK + kk * 32 + g * 8);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], acc, 0, 0, 0);
  }
  return acc;
}

// s -> exp(s - row maximum) in place, from the lane's own maximum mx; returns the row's sum
template <int NT>
__device__ __forceinline__ float tx_softmax(f32x4 (&s)[NT], float mx) {
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[t][r] = __builtin_amdgcn_exp2f((s[t][r] - mx) * 1.4426950409f);
      sum += s[t][r];
    }
  }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  return sum;
}

// O^T = V^T P^T over the 32-key steps that hold a key <= last_key (wave-uniform: beyond it every probability is 0); the
// lane ends up with columns 16 dt + 4 g + 0..3 of query j
template <int LDV, int NT>
__device__ __forceinline__ void tx_pv(const bf16 *sV, const f32x4 (&s)[NT], int j, int g, int last_key, f32x4 (&o)[4]) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NT / 2; ++u) {
    if (u * 32 <= last_key) {
      bf16x8 pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[r] = (bf16)s[2 * u][r];
        pf[4 + r] = (bf16)s[2 * u + 1][r];
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16 *vr = sV + (dt * 16 + j) * LDV + u * 32 + g * 4;
        const bf16x4 lo = *(const bf16x4 *)vr, hi = *(const bf16x4 *)(vr + 16);
        const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
      }
    }
  }
}

// out row (row0 + qpos), columns col + 16 dt + 4 g + 0..3 = bf16(o / sum)
__device__ __forceinline__ void tx_store_o(bf16 *out, long row0, int qpos, long ldo, long col, int g, const f32x4 (&o)[4],
                                           float sum) {
  const float inv = 1.0f / sum;
  bf16 *orow = out + (row0 + qpos) * ldo + col + g * 4;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const uint2 w = {ca_pack2(o[dt][0] * inv, o[dt][1] * inv), ca_pack2(o[dt][2] * inv, o[dt][3] * inv)};
    *(uint2 *)(orow + dt * 16) = w;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Row kernels: a workgroup of 256 threads per row, rows walked with the grid's stride.  The reductions over the row: 64
// lanes by exchanges, then the 4 waves through `red` in a fixed tree.  The first barrier lets a second reduction (or the
// next row) reuse `red`.
__device__ __forceinline__ float tx_block_sum(float v, float *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float tx_block_max(float v, float *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// the row's e4m3 scale from the thread's |y| maximum: amax / 448, or 1 for a zero row (the rule of
// ca_quantize_rows_fp8_kernel); thread 0 writes it; returns its inverse, the factor of the store pass
__device__ __forceinline__ float tx_fp8_row_scale(float amax, float *red, float *out_scale) {
  amax = tx_block_max(amax, red);
  const float sc = ca_fp8_row_scale(amax);
  const float inv = 1.0f / sc;
  if (threadIdx.x == 0) *out_scale = sc;
  return inv;
}

static unsigned tx_row_blocks(long rows) { return (unsigned)(rows < 65536 ? rows : 65536); }

// ------------------------------------------------------------------------------------------------------------------
// Elementwise kernels: f(row, first column) once per chunk of 8 columns of a rows x C problem, 256 threads per
// workgroup, the chunk index in 64 bits, chunks walked with the grid's stride.
template <class F>
__device__ __forceinline__ void tx_walk8(long rows, int C, F f) {
  const int cq = C / 8;
  const long total = rows * cq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / cq;
    f(r, (int)(i - r * cq) * 8);
  }
}

static unsigned tx_walk8_blocks(long rows, int C) {
  long blocks = (rows * (C / 8) + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  return (unsigned)blocks;
}
