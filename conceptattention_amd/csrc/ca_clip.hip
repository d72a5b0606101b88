// Kernels of the CLIP text encoder (transformers' CLIPTextModel): causal self-attention on v_mfma_f32_16x16x32_bf16 for
// sequences that fill no tile, the LayerNorm of the fp32 residual stream (with a row gather for the pooled read-out),
// quick_gelu and the token + position embedding.  The projections run on the grouped GEMM of ca_gemm.hip.  Every element
// offset is formed in 64 bits.
#include "ca_text_core.h"

// ------------------------------------------------------------------------------------------------------------------
// out = softmax(scale q k^T + causal mask) v per (sequence, head); head dim 64; L any value in 1..128.  The tile and its
// steps are ca_text_core.h's.
//
// What is this kernel's own.  LP = 32 NU >= L is the padded key count (P V contracts 32 keys per MFMA).  Positions >= L of
// the last tile belong to the next sequence, or past the last sequence to nobody: they are never loaded -- K rows, V
// columns and query fragments of such positions are ZEROS -- and such query rows are never stored.  A query at position i
// sees keys 0..i: the other scores become -inf before the maximum (key 0 is visible to everyone, so the maximum is finite
// and exp2(-inf) = 0).  For a query < L every key <= i is < L, so the zero rows are always masked.  A workgroup stages only
// the keys its 64 queries can see, a wave skips the key tiles that lie wholly above its 16 queries, and a wave whose
// queries are all >= L leaves after the barrier.
template <int NU>   // NU = LP / 32 key steps of P V, 2 NU key tiles of 16
__global__ __launch_bounds__(256) void ca_clip_attn_kernel(const bf16 *q, const bf16 *k, const bf16 *v, bf16 *out, long ldq,
                                                            long ldk, long ldv, long ldo, int heads, int L, float scale) {
  constexpr int NT = 2 * NU, LP = 32 * NU, LDV = LP + 16;
  bf16 *sK, *sV;
  tx_carve(LP, sK, sV);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int QT = (L + 63) / 64;
  const long blk = blockIdx.x;
  const int qt = (int)(blk % QT);
  const long sh = blk / QT;
  const int h = (int)(sh % heads);
  const long seq = sh / heads;
  const long row0 = seq * L;                         // first token row of the sequence
  const long col = (long)h * TX_D;
  const int nkeys = LP < qt * 64 + 64 ? LP : qt * 64 + 64;   // keys the workgroup's queries can see (a multiple of 32)

  tx_stage_kv<LDV>(k, v, row0, col, ldk, ldv, sK, sV, nkeys, L);
  const int j = lane & 15, g = lane >> 4;
  const int qbase = qt * 64 + wave * 16;             // wave-uniform
  const int qpos = qbase + j;
  bf16x8 qf[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) qf[0][i] = qf[1][i] = (bf16)0.f;
  if (qpos < L) tx_load_q(q, row0, qpos, ldq, col, g, qf);
  __syncthreads();
  if (qbase >= L) return;                            // no query of this wave exists (no barrier follows)

  // ---- scores, scale, causal mask, row maximum
  f32x4 s[NT];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t * 16 <= qbase + 15) {                      // wave-uniform: some query of the wave sees some key of the tile
      const f32x4 acc = tx_score_tile(sK, t, j, g, qf);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = t * 16 + g * 4 + r <= qpos ? acc[r] * scale : -INFINITY;
        mx = fmaxf(mx, s[t][r]);
      }
    } else {
      s[t] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    }
  }
  const float sum = tx_softmax(s, mx);

  f32x4 o[4];
  tx_pv<LDV>(sV, s, j, g, qbase + 15, o);
  if (qpos < L) tx_store_o(out, row0, qpos, ldo, col, g, o, sum);
}

template <int NU>
static int clip_attn_launch(const bf16 *q, const bf16 *k, const bf16 *v, bf16 *out, long ldq, long ldk, long ldv, long ldo,
                            int heads, int L, float scale, long blocks, hipStream_t st, const char *FN) {
  const int lds = tx_attn_lds_bytes(32 * NU, 0);   // at most 36864 bytes: below the default limit
  hipLaunchKernelGGL(ca_clip_attn_kernel<NU>, dim3((unsigned)blocks), dim3(256), lds, st, q, k, v, out, ldq, ldk, ldv, ldo,
                     heads, L, scale);
  return ca_check_launch(FN);
}

extern "C" int ca_clip_attn_bf16(const void *q, const void *k, const void *v, void *out, int32_t ldq, int32_t ldk,
                                 int32_t ldv, int32_t ldo, int32_t n_seq, int32_t heads, int32_t L, float scale,
                                 ca_stream_t stream) {
  const char *FN = "ca_clip_attn_bf16";
  if (!q || !k || !v || !out) {
    ca_set_error("%s: null pointer", FN);
    return CA_ERR_ARG;
  }
  const long width = (long)heads * TX_D;
  if (n_seq < 1 || heads < 1 || L < 1 || L > 128 || ldq < width || ldk < width || ldv < width || ldo < width || ldq % 8 ||
      ldk % 8 || ldv % 8 || ldo % 8 || !(scale > 0.f) || !(scale < INFINITY)) {
    ca_set_error("%s: bad sizes (n_seq=%d heads=%d L=%d [1..128] ldq=%d ldk=%d ldv=%d ldo=%d [>= heads*64, %% 8] scale=%g "
                 "[> 0, finite])", FN, n_seq, heads, L, ldq, ldk, ldv, ldo, (double)scale);
    return CA_ERR_ARG;
  }
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) {
    ca_set_error("%s: q, k, v and out must be 16-byte aligned", FN);
    return CA_ERR_ARG;
  }
  const long blocks = (long)n_seq * heads * ((L + 63) / 64);
  if (blocks > 0x7fffffffL) {
    ca_set_error("%s: %ld workgroups exceed the grid", FN, blocks);
    return CA_ERR_ARG;
  }
  const bf16 *qp = (const bf16 *)q, *kp = (const bf16 *)k, *vp = (const bf16 *)v;
  bf16 *op = (bf16 *)out;
  hipStream_t st = (hipStream_t)stream;
  switch ((L + 31) / 32) {
#define CLIP_CASE(n) \
  case n: return clip_attn_launch<n>(qp, kp, vp, op, ldq, ldk, ldv, ldo, heads, L, scale, blocks, st, FN);
    CLIP_CASE(1) CLIP_CASE(2) CLIP_CASE(3) CLIP_CASE(4)
#undef CLIP_CASE
  }
  ca_set_error("%s: L=%d", FN, L);
  return CA_ERR_ARG;
}

// ------------------------------------------------------------------------------------------------------------------
// nn.LayerNorm on the fp32 stream: out[r, :] = bf16((x[src, :] - mean) * rsqrt(var + eps) * w[:] + b[:]) with
// src = row_idx ? row_idx[r] : r and var the biased variance ABOUT the mean (a second pass over the row: the one-pass
// form sum x^2 / H - mean^2 cancels when the mean is large against the spread).  A workgroup per output row, three
// passes over the source row (the later ones hit the cache).
__global__ __launch_bounds__(256) void ca_layernorm_kernel(const float *x, long ldx, const int32_t *row_idx, const float *w,
                                                            const float *b, bf16 *out, long ldo, long rows, int H, float eps) {
  __shared__ float red[4];
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const long src = row_idx ? (long)row_idx[r] : r;
    const float *xr = x + src * ldx;
    bf16 *orow = out + r * ldo;
    float sm = 0.f;
    for (int i = threadIdx.x * 4; i < H; i += 1024) {
      const f32x4 a = *(const f32x4 *)(xr + i);
      sm += (a[0] + a[1]) + (a[2] + a[3]);
    }
    const float mean = tx_block_sum(sm, red) / (float)H;
    float ss = 0.f;
    for (int i = threadIdx.x * 4; i < H; i += 1024) {
      const f32x4 a = *(const f32x4 *)(xr + i);
      const float d0 = a[0] - mean, d1 = a[1] - mean, d2 = a[2] - mean, d3 = a[3] - mean;
      ss += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    ss = tx_block_sum(ss, red);
    const float rs = 1.0f / sqrtf(ss / (float)H + eps);
    for (int i = threadIdx.x * 4; i < H; i += 1024) {
      const f32x4 a = *(const f32x4 *)(xr + i), g = *(const f32x4 *)(w + i), c = *(const f32x4 *)(b + i);
      const uint2 o = {ca_pack2((a[0] - mean) * rs * g[0] + c[0], (a[1] - mean) * rs * g[1] + c[1]),
                       ca_pack2((a[2] - mean) * rs * g[2] + c[2], (a[3] - mean) * rs * g[3] + c[3])};
      *(uint2 *)(orow + i) = o;
    }
  }
}

extern "C" int ca_layernorm_f32in(const float *x, int32_t ldx, const int32_t *row_idx, const float *w, const float *b,
                                  void *out, int32_t ldo, int64_t rows, int32_t H, float eps, ca_stream_t stream) {
  const char *FN = "ca_layernorm_f32in";
  if (!x || !w || !b || !out || rows < 1 || H < 4 || H % 4 || ldx < H || ldo < H || ldx % 4 || ldo % 4 || !(eps > 0.f)) {
    ca_set_error("%s: bad arguments (rows=%lld H=%d [%% 4] ldx=%d ldo=%d [>= H, %% 4] eps=%g [> 0]; x, w, b, out non-null)",
                 FN, (long long)rows, H, ldx, ldo, (double)eps);
    return CA_ERR_ARG;
  }
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)b) & 15) || ((uintptr_t)out & 7) || ((uintptr_t)row_idx & 3)) {
    ca_set_error("%s: x, w and b must be 16-byte aligned, out 8-byte, row_idx 4-byte", FN);
    return CA_ERR_ARG;
  }
  hipLaunchKernelGGL(ca_layernorm_kernel, dim3(tx_row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, row_idx,
                     w, b, (bf16 *)out, (long)ldo, (long)rows, H, eps);
  return ca_check_launch(FN);
}

// ------------------------------------------------------------------------------------------------------------------
// quick_gelu: out = bf16(x * sigmoid(1.702 x)) = x / (1 + exp2(-1.702 log2(e) x)), in fp32, 8 elements per thread.
// x >> 0: exp2 -> 0, the quotient -> x (+inf stays +inf).  x << 0: exp2 -> +inf, 1 / inf = 0, x * 0 = -0; that product
// would be NaN at x = -inf, so x is first raised to -128, where the function (1e-93) is far below the smallest fp32
// number already.  The comparison is false for a NaN, which therefore passes through.
__device__ __forceinline__ float clip_quick_gelu(float x) {
  const float xc = x < -128.f ? -128.f : x;
  return xc * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.4554669595f * xc));
}

__global__ __launch_bounds__(256) void ca_quick_gelu_kernel(const bf16 *x, long ldx, bf16 *out, long ldo, long rows, int C) {
  tx_walk8(rows, C, [&](long r, int c) {
    const bf16x8 a = *(const bf16x8 *)(x + r * ldx + c);
    uint4 o;
    o.x = ca_pack2(clip_quick_gelu((float)a[0]), clip_quick_gelu((float)a[1]));
    o.y = ca_pack2(clip_quick_gelu((float)a[2]), clip_quick_gelu((float)a[3]));
    o.z = ca_pack2(clip_quick_gelu((float)a[4]), clip_quick_gelu((float)a[5]));
    o.w = ca_pack2(clip_quick_gelu((float)a[6]), clip_quick_gelu((float)a[7]));
    *(uint4 *)(out + r * ldo + c) = o;
  });
}

extern "C" int ca_quick_gelu_bf16(const void *x, int32_t ldx, void *out, int32_t ldo, int64_t rows, int32_t C,
                                  ca_stream_t stream) {
  const char *FN = "ca_quick_gelu_bf16";
  if (!x || !out || rows < 1 || C < 8 || C % 8 || ldx < C || ldo < C || ldx % 8 || ldo % 8 ||
      (((uintptr_t)x | (uintptr_t)out) & 15)) {
    ca_set_error("%s: bad arguments (rows=%lld C=%d [%% 8] ldx=%d ldo=%d [>= C, %% 8]; 16-byte aligned non-null pointers)",
                 FN, (long long)rows, C, ldx, ldo);
    return CA_ERR_ARG;
  }
  hipLaunchKernelGGL(ca_quick_gelu_kernel, dim3(tx_walk8_blocks(rows, C)), dim3(256), 0, (hipStream_t)stream, (const bf16 *)x,
                     (long)ldx, (bf16 *)out, (long)ldo, (long)rows, C);
  return ca_check_launch(FN);
}

// ------------------------------------------------------------------------------------------------------------------
// CLIPTextEmbeddings: out[r, :] = float(tok[ids[r], :]) + float(pos[r % L, :]) into the fp32 stream, one fp32 addition.
// The ids are the caller's responsibility (the Python wrapper rejects any outside [0, vocab) before the launch).
__global__ __launch_bounds__(256) void ca_clip_embed_kernel(const bf16 *tok, long ldt, const bf16 *pos, long ldp,
                                                             const int32_t *ids, float *out, long ldo, long rows, int L,
                                                             int H) {
  tx_walk8(rows, H, [&](long r, int c) {
    const bf16x8 a = *(const bf16x8 *)(tok + (long)ids[r] * ldt + c);
    const bf16x8 p = *(const bf16x8 *)(pos + (r % L) * ldp + c);
    float *o = out + r * ldo + c;
    *(f32x4 *)o = f32x4{(float)a[0] + (float)p[0], (float)a[1] + (float)p[1], (float)a[2] + (float)p[2],
                        (float)a[3] + (float)p[3]};
    *(f32x4 *)(o + 4) = f32x4{(float)a[4] + (float)p[4], (float)a[5] + (float)p[5], (float)a[6] + (float)p[6],
                              (float)a[7] + (float)p[7]};
  });
}

extern "C" int ca_clip_embed_f32(const void *tok, int32_t ldt, const void *pos, int32_t ldp, const int32_t *ids, float *out,
                                 int32_t ldo, int64_t rows, int32_t L, int32_t H, ca_stream_t stream) {
  const char *FN = "ca_clip_embed_f32";
  if (!tok || !pos || !ids || !out || rows < 1 || L < 1 || L > 128 || H < 8 || H % 8 || ldt < H || ldp < H || ldo < H ||
      ldt % 8 || ldp % 8 || ldo % 4 || (((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)out) & 15) || ((uintptr_t)ids & 3)) {
    ca_set_error("%s: bad arguments (rows=%lld L=%d [1..128] H=%d [%% 8] ldt=%d ldp=%d [>= H, %% 8] ldo=%d [>= H, %% 4]; tok, "
                 "pos and out 16-byte aligned, ids 4-byte, all non-null)", FN, (long long)rows, L, H, ldt, ldp, ldo);
    return CA_ERR_ARG;
  }
  hipLaunchKernelGGL(ca_clip_embed_kernel, dim3(tx_walk8_blocks(rows, H)), dim3(256), 0, (hipStream_t)stream, (const bf16 *)tok,
                     (long)ldt, (const bf16 *)pos, (long)ldp, ids, out, (long)ldo, (long)rows, L, H);
  return ca_check_launch(FN);
}
