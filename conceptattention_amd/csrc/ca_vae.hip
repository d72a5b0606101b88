// Kernels of the Flux autoencoder (flux/modules/autoencoder.py): implicit-GEMM 3x3 / 1x1 convolution on
// v_mfma_f32_16x16x32_bf16, GroupNorm(32) + swish, the row softmax of the one-head mid-block attention and the latent /
// image affine.  Activations are NHWC: a pixel is a row of C channels.  Every element offset is formed in 64 bits.
#include "ca_common.h"

// ------------------------------------------------------------------------------------------------------------------
// Convolution.  out[p, n] = bias[n] + sum_{tap, c} x[src(p, tap), c] * w[n, tap * Cin + c]  (+ resid[p, n])
// M = B*Ho*Wo output pixels, N = Cout, K = taps * Cin walked tap by tap in steps of 32 channels.  A workgroup of 4 waves
// owns a 128-pixel x (32 * NJ)-channel tile; the waves sit 2 x 2 on it, each 64 pixels x (16 * NJ) channels.  Pixel
// rows are gathered global -> registers -> LDS with the padding predicate (a padding pixel is a zero row, no padded
// copy exists); the weight tile takes the same road.  Two LDS stages: the loads of step s + 1 are in flight while the
// MFMAs of step s run, one barrier per step.
#define CV_BM 128
#define CV_BK 32
// 80-byte LDS rows: the 16 rows a ds_read_b128 fragment read touches fall on 16 distinct 16-byte slots of the 256-byte
// bank line (80 r mod 256 is a permutation of the multiples of 16 for r = 0..15)
#define CV_LD 40

struct ConvArgs {
  const bf16 *x, *w;
  const float *bias, *resid;
  void *out;
  long M;
  int Hin, Win, Cin, Cout, CoutPad, Ho, Wo;
  int ldx, ldr, ldo, ksize, stride, up, out_f32;
};

template <int NJ>
__global__ __launch_bounds__(256) void ca_conv_kernel(const ConvArgs a) {
  constexpr int BN = 32 * NJ;
  constexpr int WCH = (BN * 4 + 255) / 256;   // 16-byte weight chunks per thread and step
  __shared__ __attribute__((aligned(16))) bf16 sA[2][CV_BM * CV_LD];
  __shared__ __attribute__((aligned(16))) bf16 sW[2][BN * CV_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const long m0 = (long)blockIdx.x * CV_BM;
  const int n0 = blockIdx.y * BN;
  const int kc = tid & 3;                      // which 8-channel chunk of the 32-channel step this thread moves
  const int pad = (a.ksize == 3 && a.stride == 1) ? 1 : 0;
  const int Hv = a.up ? 2 * a.Hin : a.Hin, Wv = a.up ? 2 * a.Win : a.Win;   // the (virtual) input the taps walk
  // the two pixel rows of the tile this thread gathers: tile rows tid >> 2 and 64 + (tid >> 2)
  long pixbase[2];
  int oy[2], ox[2];
  bool rowok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long m = m0 + (tid >> 2) + 64 * i;
    rowok[i] = m < a.M;
    const long mm = rowok[i] ? m : 0;
    const long hw = (long)a.Ho * a.Wo;
    const long b = mm / hw;
    const int r = (int)(mm - b * hw);
    oy[i] = r / a.Wo;
    ox[i] = r - oy[i] * a.Wo;
    pixbase[i] = b * a.Hin * a.Win;
  }
  const int kpt = a.Cin / CV_BK;               // steps per tap
  const int steps = a.ksize * a.ksize * kpt;
  const long ldw = (long)a.ksize * a.ksize * a.Cin;

  uint4 ra[2], rw[WCH];
  auto fetch = [&](int s) {
    const int tap = s / kpt, c0 = (s - tap * kpt) * CV_BK + kc * 8;
    const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int iy = oy[i] * a.stride + ky - pad, ix = ox[i] * a.stride + kx - pad;
      const bool ok = rowok[i] && iy >= 0 && iy < Hv && ix >= 0 && ix < Wv;
      ra[i] = make_uint4(0, 0, 0, 0);
      if (ok) {
        const int sy = a.up ? iy >> 1 : iy, sx = a.up ? ix >> 1 : ix;
        ra[i] = *(const uint4 *)(a.x + (pixbase[i] + (long)sy * a.Win + sx) * a.ldx + c0);
      }
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int id = tid + 256 * i, n = n0 + (id >> 2);
      rw[i] = make_uint4(0, 0, 0, 0);
      if (id < BN * 4 && n < a.CoutPad) rw[i] = *(const uint4 *)(a.w + (long)n * ldw + (long)s * CV_BK + kc * 8);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *(uint4 *)(&sA[buf][((tid >> 2) + 64 * i) * CV_LD + kc * 8]) = ra[i];
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int id = tid + 256 * i;
      if (id < BN * 4) *(uint4 *)(&sW[buf][(id >> 2) * CV_LD + kc * 8]) = rw[i];
    }
  };

  f32x4 acc[4][NJ];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stash(0);
  __syncthreads();
  const int frow = lane & 15, fk = (lane >> 4) * 8;
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    if (s + 1 < steps) fetch(s + 1);
    bf16x8 af[4], wf[NJ];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) af[mi] = *(const bf16x8 *)(&sA[buf][(wm * 64 + mi * 16 + frow) * CV_LD + fk]);
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) wf[nj] = *(const bf16x8 *)(&sW[buf][(wn * NJ * 16 + nj * 16 + frow) * CV_LD + fk]);
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      if (n0 + wn * NJ * 16 + nj * 16 < a.CoutPad) {   // wave-uniform: no MFMA on fragments past the padded Cout
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nj], af[mi], acc[mi][nj], 0, 0, 0);
      }
    }
    if (s + 1 < steps) stash(buf ^ 1);
    __syncthreads();
  }

  // D = W-fragment x pixel-fragment: a lane holds channels (lane >> 4) * 4 + 0..3 of pixel lane & 15
  const bool vec = (a.Cout % 4 == 0) && (a.ldo % 4 == 0) && (a.ldr % 4 == 0);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const long m = m0 + wm * 64 + mi * 16 + (lane & 15);
    if (m >= a.M) continue;
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      const int n = n0 + wn * NJ * 16 + nj * 16 + (lane >> 4) * 4;
      if (n >= a.Cout) continue;
      f32x4 v = acc[mi][nj];
      if (vec) {
        if (a.bias) v += *(const f32x4 *)(a.bias + n);
        if (a.resid) v += *(const f32x4 *)(a.resid + m * a.ldr + n);
        if (a.out_f32) {
          *(f32x4 *)((float *)a.out + m * a.ldo + n) = v;
        } else {
          uint2 o = {ca_pack2(v[0], v[1]), ca_pack2(v[2], v[3])};
          *(uint2 *)((bf16 *)a.out + m * a.ldo + n) = o;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (n + i >= a.Cout) break;
          float y = v[i];
          if (a.bias) y += a.bias[n + i];
          if (a.resid) y += a.resid[m * a.ldr + n + i];
          if (a.out_f32) ((float *)a.out)[m * a.ldo + n + i] = y;
          else ((bf16 *)a.out)[m * a.ldo + n + i] = (bf16)y;
        }
      }
    }
  }
}

static int conv_out_dim(int in, int ksize, int stride, int up) {
  if (up) return 2 * in;
  if (stride == 2) return (in + 1 - 3) / 2 + 1;   // (0,1,0,1) zero padding, no padding on the leading edge
  (void)ksize;
  return in;
}

extern "C" int ca_conv3x3_nhwc(const void *x, const void *w, const float *bias, const float *resid, void *out,
                               int32_t B, int32_t Hin, int32_t Win, int32_t Cin, int32_t Cout, int32_t ldx, int32_t ldr,
                               int32_t ldo, int32_t ksize, int32_t stride, int32_t upsample, int32_t out_f32,
                               ca_stream_t stream) {
  const char *FN = "ca_conv3x3_nhwc";
  if (!x || !w || !out) {
    ca_set_error("%s: null pointer", FN);
    return CA_ERR_ARG;
  }
  if (B < 1 || Hin < 1 || Win < 1 || Cin < CV_BK || Cin % CV_BK || Cout < 1 || ldx < Cin || ldx % 8 || ldo < Cout ||
      (resid && ldr < Cout) || (ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) ||
      (stride == 2 && (ksize != 3 || upsample || Hin < 2 || Win < 2)) || (upsample && ksize != 3)) {
    ca_set_error("%s: bad sizes (B=%d Hin=%d Win=%d Cin=%d [%% 32] Cout=%d ldx=%d [>= Cin, %% 8] ldr=%d ldo=%d ksize=%d "
                 "stride=%d upsample=%d)", FN, B, Hin, Win, Cin, Cout, ldx, ldr, ldo, ksize, stride, upsample);
    return CA_ERR_ARG;
  }
  if ((((uintptr_t)x | (uintptr_t)w) & 15) || ((uintptr_t)out & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)resid & 3)) {
    ca_set_error("%s: x and w must be 16-byte aligned, out / bias / resid 4-byte", FN);
    return CA_ERR_ARG;
  }
  ConvArgs a;
  a.x = (const bf16 *)x, a.w = (const bf16 *)w, a.bias = bias, a.resid = resid, a.out = out;
  a.Hin = Hin, a.Win = Win, a.Cin = Cin, a.Cout = Cout, a.CoutPad = (Cout + 15) / 16 * 16;
  a.Ho = conv_out_dim(Hin, ksize, stride, upsample), a.Wo = conv_out_dim(Win, ksize, stride, upsample);
  a.M = (long)B * a.Ho * a.Wo;
  a.ldx = ldx, a.ldr = resid ? ldr : 4, a.ldo = ldo, a.ksize = ksize, a.stride = stride, a.up = upsample ? 1 : 0;
  a.out_f32 = out_f32 ? 1 : 0;
  const bool vec = Cout % 4 == 0 && ldo % 4 == 0 && a.ldr % 4 == 0;
  if (vec && ((((uintptr_t)out) & (out_f32 ? 15 : 7)) || ((uintptr_t)bias & 15) || ((uintptr_t)resid & 15))) {
    ca_set_error("%s: with Cout, ldo and ldr multiples of 4 the out / bias / resid pointers must be 16-byte aligned", FN);
    return CA_ERR_ARG;
  }
  const long mt = (a.M + CV_BM - 1) / CV_BM;
  if (mt > 0x7fffffffL) {
    ca_set_error("%s: %ld output pixels exceed the grid", FN, a.M);
    return CA_ERR_ARG;
  }
  if (a.CoutPad <= 32)
    hipLaunchKernelGGL(ca_conv_kernel<1>, dim3((unsigned)mt, 1), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ca_conv_kernel<4>, dim3((unsigned)mt, (a.CoutPad + 127) / 128), dim3(256), 0, (hipStream_t)stream, a);
  return ca_check_launch(FN);
}

// ------------------------------------------------------------------------------------------------------------------
// GroupNorm(32 groups, affine) + optional swish.  Launch 1: every workgroup reduces a chunk of an image's pixels over
// all C channels to (count, mean, M2) per group -- Welford per thread and channel, Chan's merge across threads -- and
// writes them to part[b][chunk][group][3].  Launch 2 merges the chunks of its image (in a fixed order, so the result
// does not depend on the launch) and applies (x - mean) * rstd * gamma + beta.  No E[x^2] - E[x]^2 anywhere.
// Traffic per element: fp32 in: 4 + 4 bytes read, 2 written; bf16 in: 2 + 2 read, 2 written.
__device__ __forceinline__ void chan_merge(float &n, float &mean, float &m2, float nb, float meanb, float m2b) {
  if (nb == 0.f) return;
  const float nt = n + nb, d = meanb - mean, f = nb / nt;
  mean += d * f;
  m2 += m2b + d * d * n * f;
  n = nt;
}

template <typename T>
__device__ __forceinline__ f32x4 load4(const T *p);
template <>
__device__ __forceinline__ f32x4 load4<float>(const float *p) { return *(const f32x4 *)p; }
template <>
__device__ __forceinline__ f32x4 load4<bf16>(const bf16 *p) {
  const bf16x4 v = *(const bf16x4 *)p;
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

template <typename T>
__global__ __launch_bounds__(256) void ca_gn_stats_kernel(const T *x, long ldx, long HW, int C, int n_chunks, float *part) {
  __shared__ float red[256 * 4 * 3];
  const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
  const int cq = C / 4;                        // column quads; a power of two <= 256
  const int q = tid % cq, r0 = tid / cq, rstep = 256 / cq;
  const long per = (HW + n_chunks - 1) / n_chunks;
  const long p0 = (long)chunk * per, p1 = p0 + per < HW ? p0 + per : HW;
  const T *xb = x + (long)b * HW * ldx + q * 4;
  f32x4 mean = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
  float n = 0.f;
  for (long p = p0 + r0; p < p1; p += rstep) {
    const f32x4 v = load4<T>(xb + p * ldx);
    n += 1.f;
    const float inv = 1.f / n;
    const f32x4 d = v - mean;
    mean += d * inv;
    m2 += d * (v - mean);
  }
  // [row slot][channel] so that a group's entries of one row slot are contiguous
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float *e = red + ((long)r0 * C + q * 4 + i) * 3;
    e[0] = n, e[1] = mean[i], e[2] = m2[i];
  }
  __syncthreads();
  if (tid < 32) {
    const int cpg = C / 32;
    float gn = 0.f, gmean = 0.f, gm2 = 0.f;
    for (int r = 0; r < rstep; ++r)
      for (int c = 0; c < cpg; ++c) {
        const float *e = red + ((long)r * C + tid * cpg + c) * 3;
        chan_merge(gn, gmean, gm2, e[0], e[1], e[2]);
      }
    float *o = part + (((long)b * n_chunks + chunk) * 32 + tid) * 3;
    o[0] = gn, o[1] = gmean, o[2] = gm2;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ca_gn_apply_kernel(const T *x, long ldx, long HW, int C, int n_chunks,
                                                          const float *part, const float *gamma, const float *beta,
                                                          float eps, int swish, bf16 *y, long ldy) {
  __shared__ float s_mean[32], s_rstd[32];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (tid < 32) {
    float gn = 0.f, gmean = 0.f, gm2 = 0.f;
    for (int c = 0; c < n_chunks; ++c) {
      const float *e = part + (((long)b * n_chunks + c) * 32 + tid) * 3;
      chan_merge(gn, gmean, gm2, e[0], e[1], e[2]);
    }
    s_mean[tid] = gmean;
    s_rstd[tid] = 1.0f / sqrtf(gm2 / gn + eps);
  }
  __syncthreads();
  const int cq = C / 4, q = tid % cq, r0 = tid / cq, rstep = 256 / cq, cpg = C / 32;
  const f32x4 g = *(const f32x4 *)(gamma + q * 4), be = *(const f32x4 *)(beta + q * 4);
  f32x4 sc, sh;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int grp = (q * 4 + i) / cpg;
    sc[i] = s_rstd[grp] * g[i];
    sh[i] = be[i] - s_mean[grp] * sc[i];
  }
  const T *xb = x + (long)b * HW * ldx + q * 4;
  bf16 *yb = y + (long)b * HW * ldy + q * 4;
  for (long p = (long)blockIdx.x * rstep + r0; p < HW; p += (long)gridDim.x * rstep) {
    f32x4 v = load4<T>(xb + p * ldx) * sc + sh;
    if (swish) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = v[i] / (1.0f + __expf(-v[i]));
    }
    uint2 o = {ca_pack2(v[0], v[1]), ca_pack2(v[2], v[3])};
    *(uint2 *)(yb + p * ldy) = o;
  }
}

extern "C" int ca_groupnorm_nhwc(const void *x, int32_t x_f32, int32_t ldx, const float *gamma, const float *beta,
                                 void *y, int32_t ldy, int32_t B, int64_t HW, int32_t C, float eps, int32_t swish,
                                 float *part, int32_t n_chunks, ca_stream_t stream) {
  const char *FN = "ca_groupnorm_nhwc";
  if (!x || !gamma || !beta || !y || !part) {
    ca_set_error("%s: null pointer", FN);
    return CA_ERR_ARG;
  }
  if (B < 1 || B > 65535 || HW < 1 || C < 32 || C > 1024 || (C & (C - 1)) || ldx < C || ldx % 4 || ldy < C || ldy % 4 ||
      n_chunks < 1 || n_chunks > 1024 || !(eps > 0.f)) {
    ca_set_error("%s: bad sizes (B=%d HW=%lld C=%d [a power of two in 32..1024] ldx=%d ldy=%d [>= C, %% 4] n_chunks=%d "
                 "[1..1024] eps=%g)", FN, B, (long long)HW, C, ldx, ldy, n_chunks, (double)eps);
    return CA_ERR_ARG;
  }
  if ((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) & 15) || ((uintptr_t)y & 7) || ((uintptr_t)part & 3) ||
      (!x_f32 && ldx % 8)) {
    ca_set_error("%s: x, gamma and beta must be 16-byte aligned (a bf16 x: ldx %% 8), y 8-byte", FN);
    return CA_ERR_ARG;
  }
  const int rstep = 256 / (C / 4);
  long ab = (HW + (long)rstep * 8 - 1) / ((long)rstep * 8);   // about 8 rows per thread of the apply launch
  if (ab > 4096) ab = 4096;
  hipStream_t st = (hipStream_t)stream;
  if (x_f32) {
    hipLaunchKernelGGL(ca_gn_stats_kernel<float>, dim3(n_chunks, B), dim3(256), 0, st, (const float *)x, (long)ldx,
                       (long)HW, C, n_chunks, part);
    hipLaunchKernelGGL(ca_gn_apply_kernel<float>, dim3((unsigned)ab, B), dim3(256), 0, st, (const float *)x, (long)ldx,
                       (long)HW, C, n_chunks, (const float *)part, gamma, beta, eps, swish, (bf16 *)y, (long)ldy);
  } else {
    hipLaunchKernelGGL(ca_gn_stats_kernel<bf16>, dim3(n_chunks, B), dim3(256), 0, st, (const bf16 *)x, (long)ldx,
                       (long)HW, C, n_chunks, part);
    hipLaunchKernelGGL(ca_gn_apply_kernel<bf16>, dim3((unsigned)ab, B), dim3(256), 0, st, (const bf16 *)x, (long)ldx,
                       (long)HW, C, n_chunks, (const float *)part, gamma, beta, eps, swish, (bf16 *)y, (long)ldy);
  }
  return ca_check_launch(FN);
}

// ------------------------------------------------------------------------------------------------------------------
// p[r, 0:n] = softmax(scale * s[r, 0:n]) as bf16, p[r, n:ldp] = 0.  One workgroup per row, three passes over the row
// (max, sum, write); the second and third hit the cache for any row the mid-block attention produces.
__device__ __forceinline__ float block_reduce(float v, bool is_max, float *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float t = __shfl_xor(v, o);
    v = is_max ? fmaxf(v, t) : v + t;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < 4; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  return r;
}

__global__ __launch_bounds__(256) void ca_softmax_rows_kernel(const float *s, long lds, bf16 *p, long ldp, int n, float scale) {
  __shared__ float red[4];
  const float *sr = s + (long)blockIdx.x * lds;
  bf16 *pr = p + (long)blockIdx.x * ldp;
  const int tid = threadIdx.x;
  float mx = -INFINITY;
  for (int i = tid; i < n; i += 256) mx = fmaxf(mx, sr[i]);
  mx = block_reduce(mx, true, red);
  const float k = scale * 1.4426950409f;
  float sum = 0.f;
  for (int i = tid; i < n; i += 256) sum += __builtin_amdgcn_exp2f((sr[i] - mx) * k);
  sum = block_reduce(sum, false, red);
  const float inv = 1.0f / sum;
  for (int i = tid; i < (int)ldp; i += 256) pr[i] = i < n ? (bf16)(__builtin_amdgcn_exp2f((sr[i] - mx) * k) * inv) : (bf16)0.f;
}

extern "C" int ca_softmax_rows_f32(const float *s, int32_t lds, void *p, int32_t ldp, int32_t rows, int32_t n, float scale,
                                   ca_stream_t stream) {
  const char *FN = "ca_softmax_rows_f32";
  if (!s || !p || rows < 1 || n < 1 || lds < n || ldp < n || !(scale > 0.f) || ((uintptr_t)s & 3) || ((uintptr_t)p & 1)) {
    ca_set_error("%s: bad arguments (rows=%d n=%d lds=%d ldp=%d [>= n] scale=%g [> 0])", FN, rows, n, lds, ldp, (double)scale);
    return CA_ERR_ARG;
  }
  hipLaunchKernelGGL(ca_softmax_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, s, (long)lds, (bf16 *)p,
                     (long)ldp, n, scale);
  return ca_check_launch(FN);
}

// ------------------------------------------------------------------------------------------------------------------
// out[r, c] = a * (x[r, c] + exp(0.5 * logvar[r, c]) * noise[r, c]) + b, c < C; logvar / noise optional (both or none).
// The latent's affine at both ends of the autoencoder and the DiagonalGaussian sample between them; with a = 1, b = 0
// the fp32 -> bf16 cast of a convolution operand.  Columns C..ldo of a bf16 output are left as they are (the caller's
// zero padding).
__global__ __launch_bounds__(256) void ca_affine_rows_kernel(const float *x, long ldx, const float *logvar, long ldl,
                                                             const float *noise, long ldn, void *out, long ldo,
                                                             int out_f32, long rows, int C, float a, float b) {
  const long total = rows * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    float v = x[r * ldx + c];
    if (logvar) v += __expf(0.5f * logvar[r * ldl + c]) * noise[r * ldn + c];
    v = a * v + b;
    if (out_f32) ((float *)out)[r * ldo + c] = v;
    else ((bf16 *)out)[r * ldo + c] = (bf16)v;
  }
}

extern "C" int ca_affine_rows_f32(const float *x, int32_t ldx, const float *logvar, int32_t ldl, const float *noise,
                                  int32_t ldn, void *out, int32_t ldo, int32_t out_f32, int64_t rows, int32_t C, float a,
                                  float b, ca_stream_t stream) {
  const char *FN = "ca_affine_rows_f32";
  if (!x || !out || rows < 1 || C < 1 || ldx < C || ldo < C || (!logvar) != (!noise) || (logvar && (ldl < C || ldn < C)) ||
      (((uintptr_t)x | (uintptr_t)logvar | (uintptr_t)noise) & 3) || ((uintptr_t)out & (out_f32 ? 3 : 1))) {
    ca_set_error("%s: bad arguments (rows=%lld C=%d ldx=%d ldl=%d ldn=%d ldo=%d; logvar and noise go together)", FN,
                 (long long)rows, C, ldx, ldl, ldn, ldo);
    return CA_ERR_ARG;
  }
  long blocks = (rows * C + 1023) / 1024;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(ca_affine_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, logvar,
                     (long)ldl, noise, (long)ldn, out, (long)ldo, out_f32, (long)rows, C, a, b);
  return ca_check_launch(FN);
}
