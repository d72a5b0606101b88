// Kernels of the T5 encoder (transformers' T5Stack, encoder side): self-attention with the relative-position bias on
// v_mfma_f32_16x16x32_bf16, the RMS layer norm of the fp32 residual stream, the gated-GELU product (each also as a
// producer of e4m3 rows with one scale per row, for the fp8 mode) and the embedding gather.  The projections run on
// the grouped GEMM of ca_gemm.hip.  Every element offset is formed in 64 bits.
#include "ca_text_core.h"

// ------------------------------------------------------------------------------------------------------------------
// out = softmax(q k^T + bias) v per (sequence, head); head dim 64, no 1/sqrt(d) scale, no mask.  The tile and its steps
// are ca_text_core.h's; here L = 16 NT is a compile-time constant, every position exists, and the head's bias row
// (2L - 1 floats) sits in LDS behind K and V^T.
template <int NT>   // NT = L / 16 key tiles
__global__ __launch_bounds__(256) void ca_t5_attn_kernel(const bf16 *q, const bf16 *k, const bf16 *v, const float *bias,
                                                          bf16 *out, long ldq, long ldk, long ldv, long ldo, int heads) {
  constexpr int L = NT * 16;
  constexpr int LDV = L + 16;
  bf16 *sK, *sV;
  float *sB = (float *)tx_carve(L, sK, sV);          // [2 L] (2 L - 1 used)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int QT = L / 64;
  const long blk = blockIdx.x;
  const int qt = (int)(blk % QT);
  const long sh = blk / QT;
  const int h = (int)(sh % heads);
  const long seq = sh / heads;
  const long row0 = seq * L;                         // first token row of the sequence
  const long col = (long)h * TX_D;

  tx_stage_kv<LDV>(k, v, row0, col, ldk, ldv, sK, sV, L, L);
  const float *bh = bias + (long)h * (2 * L - 1);
  for (int i = tid; i < 2 * L - 1; i += 256) sB[i] = bh[i];

  const int j = lane & 15, g = lane >> 4;
  const int qpos = qt * 64 + wave * 16 + j;
  bf16x8 qf[2];
  tx_load_q(q, row0, qpos, ldq, col, g, qf);
  __syncthreads();

  f32x4 s[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) s[t] = tx_score_tile(sK, t, j, g, qf);

  // ---- + bias[key - query + L - 1], row maximum
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int b0 = t * 16 + g * 4 - qpos + L - 1;    // in [0, 2 L - 5]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[t][r] += sB[b0 + r];
      mx = fmaxf(mx, s[t][r]);
    }
  }
  const float sum = tx_softmax(s, mx);

  f32x4 o[4];
  tx_pv<LDV>(sV, s, j, g, L - 1, o);
  tx_store_o(out, row0, qpos, ldo, col, g, o, sum);
}

template <int NT>
static int t5_attn_launch(const bf16 *q, const bf16 *k, const bf16 *v, const float *bias, bf16 *out, long ldq, long ldk,
                          long ldv, long ldo, int heads, long blocks, hipStream_t st, const char *FN) {
  static std::atomic<unsigned long long> raised{0};
  const int lds = tx_attn_lds_bytes(NT * 16, 2 * NT * 16);
  const int rc = ca_raise_lds_limit({(const void *)ca_t5_attn_kernel<NT>}, lds, raised, FN);
  if (rc != CA_OK) return rc;
  hipLaunchKernelGGL(ca_t5_attn_kernel<NT>, dim3((unsigned)blocks), dim3(256), lds, st, q, k, v, bias, out, ldq, ldk, ldv,
                     ldo, heads);
  return ca_check_launch(FN);
}

extern "C" int ca_t5_attn_bf16(const void *q, const void *k, const void *v, const float *bias, void *out, int32_t ldq,
                               int32_t ldk, int32_t ldv, int32_t ldo, int32_t n_seq, int32_t heads, int32_t L,
                               ca_stream_t stream) {
  const char *FN = "ca_t5_attn_bf16";
  if (!q || !k || !v || !bias || !out) {
    ca_set_error("%s: null pointer", FN);
    return CA_ERR_ARG;
  }
  const long width = (long)heads * TX_D;
  if (n_seq < 1 || heads < 1 || L < 64 || L > 512 || L % 64 || ldq < width || ldk < width || ldv < width || ldo < width ||
      ldq % 8 || ldk % 8 || ldv % 8 || ldo % 8) {
    ca_set_error("%s: bad sizes (n_seq=%d heads=%d L=%d [64..512, %% 64] ldq=%d ldk=%d ldv=%d ldo=%d [>= heads*64, %% 8])",
                 FN, n_seq, heads, L, ldq, ldk, ldv, ldo);
    return CA_ERR_ARG;
  }
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) || ((uintptr_t)bias & 3)) {
    ca_set_error("%s: q, k, v and out must be 16-byte aligned, bias 4-byte", FN);
    return CA_ERR_ARG;
  }
  const long blocks = (long)n_seq * heads * (L / 64);
  if (blocks > 0x7fffffffL) {
    ca_set_error("%s: %ld workgroups exceed the grid", FN, blocks);
    return CA_ERR_ARG;
  }
  const bf16 *qp = (const bf16 *)q, *kp = (const bf16 *)k, *vp = (const bf16 *)v;
  bf16 *op = (bf16 *)out;
  hipStream_t st = (hipStream_t)stream;
  switch (L / 64) {
#define T5_CASE(n) \
  case n: return t5_attn_launch<4 * n>(qp, kp, vp, bias, op, ldq, ldk, ldv, ldo, heads, blocks, st, FN);
    T5_CASE(1) T5_CASE(2) T5_CASE(3) T5_CASE(4) T5_CASE(5) T5_CASE(6) T5_CASE(7) T5_CASE(8)
#undef T5_CASE
  }
  ca_set_error("%s: L=%d", FN, L);
  return CA_ERR_ARG;
}

// ------------------------------------------------------------------------------------------------------------------
// T5LayerNorm: out[r, :] = bf16(x[r, :] * rsqrt(mean(x[r, :]^2) + eps) * w[:]); no mean subtraction, no bias.  A
// workgroup per row (rows walked with the grid's stride), two passes over the row (the second hits the cache).
__global__ __launch_bounds__(256) void ca_t5_rmsnorm_kernel(const float *x, long ldx, const float *w, bf16 *out, long ldo,
                                                             long rows, int H, float eps) {
  __shared__ float red[4];
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const float *xr = x + r * ldx;
    bf16 *orow = out + r * ldo;
    float ss = 0.f;
    for (int i = threadIdx.x * 4; i < H; i += 1024) {
      const f32x4 a = *(const f32x4 *)(xr + i);
      ss += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
    }
    ss = tx_block_sum(ss, red);
    const float rs = 1.0f / sqrtf(ss / (float)H + eps);
    for (int i = threadIdx.x * 4; i < H; i += 1024) {
      const f32x4 a = *(const f32x4 *)(xr + i), g = *(const f32x4 *)(w + i);
      const uint2 o = {ca_pack2(a[0] * rs * g[0], a[1] * rs * g[1]), ca_pack2(a[2] * rs * g[2], a[3] * rs * g[3])};
      *(uint2 *)(orow + i) = o;
    }
  }
}

extern "C" int ca_t5_rmsnorm_f32in(const float *x, int32_t ldx, const float *w, void *out, int32_t ldo, int64_t rows,
                                   int32_t H, float eps, ca_stream_t stream) {
  const char *FN = "ca_t5_rmsnorm_f32in";
  if (!x || !w || !out || rows < 1 || H < 4 || H % 4 || ldx < H || ldo < H || ldx % 4 || ldo % 4 || !(eps > 0.f)) {
    ca_set_error("%s: bad arguments (rows=%lld H=%d [%% 4] ldx=%d ldo=%d [>= H, %% 4] eps=%g [> 0])", FN, (long long)rows,
                 H, ldx, ldo, (double)eps);
    return CA_ERR_ARG;
  }
  if ((((uintptr_t)x | (uintptr_t)w) & 15) || ((uintptr_t)out & 7)) {
    ca_set_error("%s: x and w must be 16-byte aligned, out 8-byte", FN);
    return CA_ERR_ARG;
  }
  hipLaunchKernelGGL(ca_t5_rmsnorm_kernel, dim3(tx_row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, w,
                     (bf16 *)out, (long)ldo, (long)rows, H, eps);
  return ca_check_launch(FN);
}

// ------------------------------------------------------------------------------------------------------------------
// The e4m3 producers of the fp8 mode: a row leaves as e4m3 bytes plus one fp32 scale (amax / 448, or 1 for a zero row;
// the rule of ca_quantize_rows_fp8_kernel), the A operand of ca_gemm_fp8.  A workgroup owns a whole row, so the row
// maximum is known before the store and the row never exists in bf16.
// y[0..8) = x[i..i+8) * rs * w[i..i+8): products only, so the pass that takes the maximum and the pass that stores
// form the same bits
__device__ __forceinline__ void t5_norm8(const float *xr, const float *w, int i, float rs, float *y) {
  const f32x4 a0 = *(const f32x4 *)(xr + i), a1 = *(const f32x4 *)(xr + i + 4);
  const f32x4 g0 = *(const f32x4 *)(w + i), g1 = *(const f32x4 *)(w + i + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    y[j] = a0[j] * rs * g0[j];
    y[4 + j] = a1[j] * rs * g1[j];
  }
}

// T5LayerNorm into e4m3: three passes over the row (sum of squares, maximum, store; the last two hit the cache).
__global__ __launch_bounds__(256) void ca_t5_rmsnorm_fp8_kernel(const float *x, long ldx, const float *w, uint8_t *out,
                                                                 long ldo, float *out_scale, long rows, int H,
                                                                 float eps) {
  __shared__ float red[4];
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const float *xr = x + r * ldx;
    uint8_t *orow = out + r * ldo;
    float ss = 0.f;
    for (int i = threadIdx.x * 8; i < H; i += 2048) {
      const f32x4 a = *(const f32x4 *)(xr + i), b = *(const f32x4 *)(xr + i + 4);
      ss += ((a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3])) +
            ((b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]));
    }
    ss = tx_block_sum(ss, red);
    const float rs = 1.0f / sqrtf(ss / (float)H + eps);
    float amax = 0.f;
    for (int i = threadIdx.x * 8; i < H; i += 2048) {
      float y[8];
      t5_norm8(xr, w, i, rs, y);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(y[j]));
    }
    const float inv = tx_fp8_row_scale(amax, red, out_scale + r);
    for (int i = threadIdx.x * 8; i < H; i += 2048) {
      float y[8];
      t5_norm8(xr, w, i, rs, y);
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] *= inv;
      *(uint2 *)(orow + i) = ca_pack_fp8x8(y);
    }
  }
}

extern "C" int ca_t5_rmsnorm_f32in_fp8(const float *x, int32_t ldx, const float *w, void *out8, int32_t ldo,
                                       float *out_scale, int64_t rows, int32_t H, float eps, ca_stream_t stream) {
  const char *FN = "ca_t5_rmsnorm_f32in_fp8";
  if (!x || !w || !out8 || !out_scale || rows < 1 || H < 8 || H % 8 || ldx < H || ldo < H || ldx % 4 || ldo % 8 ||
      !(eps > 0.f)) {
    ca_set_error("%s: bad arguments (rows=%lld H=%d [%% 8] ldx=%d [>= H, %% 4] ldo=%d [>= H, %% 8] eps=%g [> 0])", FN,
                 (long long)rows, H, ldx, ldo, (double)eps);
    return CA_ERR_ARG;
  }
  if ((((uintptr_t)x | (uintptr_t)w) & 15) || ((uintptr_t)out8 & 7) || ((uintptr_t)out_scale & 3)) {
    ca_set_error("%s: x and w must be 16-byte aligned, out8 8-byte, out_scale 4-byte", FN);
    return CA_ERR_ARG;
  }
  hipLaunchKernelGGL(ca_t5_rmsnorm_fp8_kernel, dim3(tx_row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, w,
                     (uint8_t *)out8, (long)ldo, out_scale, (long)rows, H, eps);
  return ca_check_launch(FN);
}

// ------------------------------------------------------------------------------------------------------------------
// out = bf16(float(g) * float(u)): the gelu(wi_0 x) * (wi_1 x) product of T5DenseGatedActDense, 8 elements per thread.
__global__ __launch_bounds__(256) void ca_gated_mul_kernel(const bf16 *g, long ldg, const bf16 *u, long ldu, bf16 *out,
                                                            long ldo, long rows, int C) {
  tx_walk8(rows, C, [&](long r, int c) {
    const bf16x8 a = *(const bf16x8 *)(g + r * ldg + c), b = *(const bf16x8 *)(u + r * ldu + c);
    uint4 o;
    o.x = ca_pack2((float)a[0] * (float)b[0], (float)a[1] * (float)b[1]);
    o.y = ca_pack2((float)a[2] * (float)b[2], (float)a[3] * (float)b[3]);
    o.z = ca_pack2((float)a[4] * (float)b[4], (float)a[5] * (float)b[5]);
    o.w = ca_pack2((float)a[6] * (float)b[6], (float)a[7] * (float)b[7]);
    *(uint4 *)(out + r * ldo + c) = o;
  });
}

extern "C" int ca_gated_mul_bf16(const void *g, int32_t ldg, const void *u, int32_t ldu, void *out, int32_t ldo,
                                 int64_t rows, int32_t C, ca_stream_t stream) {
  const char *FN = "ca_gated_mul_bf16";
  if (!g || !u || !out || rows < 1 || C < 8 || C % 8 || ldg < C || ldu < C || ldo < C || ldg % 8 || ldu % 8 || ldo % 8 ||
      (((uintptr_t)g | (uintptr_t)u | (uintptr_t)out) & 15)) {
    ca_set_error("%s: bad arguments (rows=%lld C=%d [%% 8] ldg=%d ldu=%d ldo=%d [>= C, %% 8]; 16-byte aligned pointers)",
                 FN, (long long)rows, C, ldg, ldu, ldo);
    return CA_ERR_ARG;
  }
  hipLaunchKernelGGL(ca_gated_mul_kernel, dim3(tx_walk8_blocks(rows, C)), dim3(256), 0, (hipStream_t)stream, (const bf16 *)g,
                     (long)ldg, (const bf16 *)u, (long)ldu, (bf16 *)out, (long)ldo, (long)rows, C);
  return ca_check_launch(FN);
}

// The gate product into e4m3: y = float(g) * float(u) is exact in fp32, so the two passes over a row (maximum, store;
// the second hits the cache) see the same values.  A workgroup per row, rows walked with the grid's stride.
__global__ __launch_bounds__(256) void ca_gated_mul_fp8_kernel(const bf16 *g, long ldg, const bf16 *u, long ldu,
                                                                uint8_t *out, long ldo, float *out_scale, long rows,
                                                                int C) {
  __shared__ float red[4];
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const bf16 *gr = g + r * ldg, *ur = u + r * ldu;
    uint8_t *orow = out + r * ldo;
    float amax = 0.f;
    for (int i = threadIdx.x * 8; i < C; i += 2048) {
      const bf16x8 a = *(const bf16x8 *)(gr + i), b = *(const bf16x8 *)(ur + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)a[j] * (float)b[j]));
    }
    const float inv = tx_fp8_row_scale(amax, red, out_scale + r);
    for (int i = threadIdx.x * 8; i < C; i += 2048) {
      const bf16x8 a = *(const bf16x8 *)(gr + i), b = *(const bf16x8 *)(ur + i);
      float y[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = (float)a[j] * (float)b[j] * inv;
      *(uint2 *)(orow + i) = ca_pack_fp8x8(y);
    }
  }
}

extern "C" int ca_gated_mul_fp8(const void *g, int32_t ldg, const void *u, int32_t ldu, void *out8, int32_t ldo,
                                float *out_scale, int64_t rows, int32_t C, ca_stream_t stream) {
  const char *FN = "ca_gated_mul_fp8";
  if (!g || !u || !out8 || !out_scale || rows < 1 || C < 8 || C % 8 || ldg < C || ldu < C || ldo < C || ldg % 8 ||
      ldu % 8 || ldo % 8) {
    ca_set_error("%s: bad arguments (rows=%lld C=%d [%% 8] ldg=%d ldu=%d ldo=%d [>= C, %% 8])", FN, (long long)rows, C,
                 ldg, ldu, ldo);
    return CA_ERR_ARG;
  }
  if ((((uintptr_t)g | (uintptr_t)u) & 15) || ((uintptr_t)out8 & 7) || ((uintptr_t)out_scale & 3)) {
    ca_set_error("%s: g and u must be 16-byte aligned, out8 8-byte, out_scale 4-byte", FN);
    return CA_ERR_ARG;
  }
  hipLaunchKernelGGL(ca_gated_mul_fp8_kernel, dim3(tx_row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, (const bf16 *)g,
                     (long)ldg, (const bf16 *)u, (long)ldu, (uint8_t *)out8, (long)ldo, out_scale, (long)rows, C);
  return ca_check_launch(FN);
}

// ------------------------------------------------------------------------------------------------------------------
// out[r, :] = float(table[ids[r], :]): the token embedding into the fp32 residual stream.  The ids are the caller's
// responsibility (the Python wrapper rejects any outside [0, vocab) before the launch).
__global__ __launch_bounds__(256) void ca_embed_rows_kernel(const bf16 *table, long ldt, const int32_t *ids, float *out,
                                                             long ldo, long rows, int H) {
  tx_walk8(rows, H, [&](long r, int c) {
    const bf16x8 a = *(const bf16x8 *)(table + (long)ids[r] * ldt + c);
    float *o = out + r * ldo + c;
    *(f32x4 *)o = f32x4{(float)a[0], (float)a[1], (float)a[2], (float)a[3]};
    *(f32x4 *)(o + 4) = f32x4{(float)a[4], (float)a[5], (float)a[6], (float)a[7]};
  });
}

extern "C" int ca_embed_rows_f32(const void *table, int32_t ldt, const int32_t *ids, float *out, int32_t ldo, int64_t rows,
                                 int32_t H, ca_stream_t stream) {
  const char *FN = "ca_embed_rows_f32";
  if (!table || !ids || !out || rows < 1 || H < 8 || H % 8 || ldt < H || ldo < H || ldt % 8 || ldo % 4 ||
      (((uintptr_t)table | (uintptr_t)out) & 15) || ((uintptr_t)ids & 3)) {
    ca_set_error("%s: bad arguments (rows=%lld H=%d [%% 8] ldt=%d [>= H, %% 8] ldo=%d [>= H, %% 4]; table and out 16-byte "
                 "aligned, ids 4-byte)", FN, (long long)rows, H, ldt, ldo);
    return CA_ERR_ARG;
  }
  hipLaunchKernelGGL(ca_embed_rows_kernel, dim3(tx_walk8_blocks(rows, H)), dim3(256), 0, (hipStream_t)stream, (const bf16 *)table,
                     (long)ldt, ids, out, (long)ldo, (long)rows, H);
  return ca_check_launch(FN);
}
