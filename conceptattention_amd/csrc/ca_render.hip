// Heat-map pictures: fp32 map planes [h, w] to RGB bytes [H, W, 3] (the colouring of concept_attention_pipeline.py:174-196,
// the overlays of concept_attention/plotting.py::overlay_heatmap_on_image and the frames of
// concept_attention/video/video_utils.py): the range of a GROUP of planes, the normalisation, matplotlib's look-up rule for a
// float array, an optional nearest or bilinear upscale and an optional blend over an RGB8 picture, in one call.
//
// A call is two to four launches on the stream, none of which waits for the host:
//   prep    one wave per group: range_out = range_in when it is given, else the identities of the integer reduction;
//   range   (only when a group has no range_in) blocks of 256 threads walk the group's planes and fold their cells into
//           range_out with atomicMin / atomicMax on ORDER KEYS (unsigned integers of the floats' order): integer atomics,
//           so any arrival order gives the same bits; a NaN cell sends both keys to the ends no number reaches;
//   decode  (the same condition) one wave per group turns the two keys into floats, both NaN if a NaN was seen;
//   colour  the store stream.  The unit of work is one 16-byte aligned SLOT of output addresses: consecutive lanes own
//           consecutive slots, a wave writes 1 KiB of contiguous bytes per store instruction.  A plane may start at any
//           byte, so a plane's first and last slot can be partial: those are written byte by byte, every other slot with
//           one 16-byte store.  A slot holds the bytes of 6 pixels at the most (16 bytes from channel c0 of the first one);
//           their colours are packed into five words and shifted by c0 bytes (v_alignbyte_b32).
// The look-up table is read into LDS once per block; the maps (64 KiB at the most per plane) are read through the caches.
//
// The unit is compiled with -ffp-contract=off: every operation below rounds on its own, except the bilinear source
// coordinate, which is one explicit fmaf (tests/render_cases.py holds the numpy statement).  Every plane offset is formed
// in 64 bits; offsets inside a plane fit 32 bits (3 H W <= 3 * 2^24).
#include "ca_common.h"

#define RENDER_THREADS 256
#define RENDER_MAX_BLOCKS 4096     // colour pass: 256 CUs x 8 workgroups x 2, divided among the groups; the rest is strided
#define RENDER_RANGE_BLOCKS 256    // range pass: blocks per group at the most, one plane at a time each
#define RENDER_MAX_CELLS 16384
#define RENDER_MAX_SIDE 4096
#define RENDER_ROW_UNDER 256
#define RENDER_ROW_OVER 257
#define RENDER_ROW_BAD 258
#define RENDER_LUT_ROWS 259

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // (one 16-byte store)

struct RenderGroup {
  const float *maps;
  const float *range_in;
  float *range_out;
  const uint8_t *image;
  uint8_t *out;
  int64_t map_stride, image_stride, out_stride;
  int32_t n_maps, pad;
};

struct RenderLaunch {
  RenderGroup g[CA_RENDER_MAX_PROBLEMS];
  const uint8_t *lut;
  int32_t h, w, H, W;
  uint32_t cpp;            // chunks of 256 slots per plane
  float alpha, beta;       // beta = 1 - alpha, formed once on the host
  float sy, sx;            // (float)h / H, (float)w / W: IEEE divisions on the host
};

// a float as an unsigned key of the same order.  No number maps to 0 or to 0xffffffff (those are NaN patterns): the two
// ends mark "a NaN was seen"
__device__ __forceinline__ uint32_t render_ordkey(float s) {
  const uint32_t b = __builtin_bit_cast(uint32_t, s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float render_unkey(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// ---- prep: the given range, or the identities of min and max over the keys
__global__ __launch_bounds__(CA_WAVE) void ca_render_prep_kernel(RenderLaunch A) {
  const RenderGroup &G = A.g[blockIdx.x];
  if (threadIdx.x != 0) return;
  uint32_t *r = (uint32_t *)G.range_out;
  if (G.range_in) {
    const float lo = G.range_in[0], hi = G.range_in[1];   // (both read before either is written: range_in may be range_out)
    G.range_out[0] = lo, G.range_out[1] = hi;
  } else {
    r[0] = 0xffffffffu, r[1] = 0u;
  }
}

// ---- range: a block folds planes blockIdx.x, + gridDim.x, ... of group blockIdx.y.  Aligned quads as 16-byte loads, the
// cells in front of the first aligned address and behind the last quad one by one.
__global__ __launch_bounds__(RENDER_THREADS) void ca_render_range_kernel(RenderLaunch A) {
  __shared__ float s_lo[RENDER_THREADS / CA_WAVE], s_hi[RENDER_THREADS / CA_WAVE];
  __shared__ int s_nan[RENDER_THREADS / CA_WAVE];
  const RenderGroup &G = A.g[blockIdx.y];
  if (G.range_in || (int)blockIdx.x >= G.n_maps) return;      // (uniform over the block)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hw = A.h * A.w;
  float lo = INFINITY, hi = -INFINITY;
  int nan = 0;
  for (int plane = blockIdx.x; plane < G.n_maps; plane += gridDim.x) {
    const float *m = G.maps + (int64_t)plane * G.map_stride;
    int head = (int)((16u - (uint32_t)((uintptr_t)m & 15)) & 15) >> 2;
    head = head < hw ? head : hw;
    const int quads = (hw - head) >> 2, tail0 = head + quads * 4;
    if (tid < head) {
      const float v = m[tid];
      lo = fminf(lo, v), hi = fmaxf(hi, v), nan |= !(v == v);
    }
    const f32x4 *mq = (const f32x4 *)(m + head);
    for (int q = tid; q < quads; q += RENDER_THREADS) {
      const f32x4 v = mq[q];
#pragma unroll
      for (int k = 0; k < 4; ++k) lo = fminf(lo, v[k]), hi = fmaxf(hi, v[k]), nan |= !(v[k] == v[k]);
    }
    if (tid < hw - tail0) {
      const float v = m[tail0 + tid];
      lo = fminf(lo, v), hi = fmaxf(hi, v), nan |= !(v == v);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off));
    hi = fmaxf(hi, __shfl_xor(hi, off));
    nan |= __shfl_xor(nan, off);
  }
  if (lane == 0) s_lo[wave] = lo, s_hi[wave] = hi, s_nan[wave] = nan;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < RENDER_THREADS / CA_WAVE; ++i) lo = fminf(lo, s_lo[i]), hi = fmaxf(hi, s_hi[i]), nan |= s_nan[i];
    uint32_t *r = (uint32_t *)G.range_out;
    atomicMin(&r[0], nan ? 0u : render_ordkey(lo));
    atomicMax(&r[1], nan ? 0xffffffffu : render_ordkey(hi));
  }
}

// ---- decode: keys to floats; ndarray.min() and .max() of an array with a NaN are both NaN
__global__ __launch_bounds__(CA_WAVE) void ca_render_decode_kernel(RenderLaunch A) {
  const RenderGroup &G = A.g[blockIdx.x];
  if (threadIdx.x != 0 || G.range_in) return;
  uint32_t *r = (uint32_t *)G.range_out;
  const uint32_t klo = r[0], khi = r[1];
  const bool nan = klo == 0u || khi == 0xffffffffu;
  G.range_out[0] = nan ? __builtin_nanf("") : render_unkey(klo);
  G.range_out[1] = nan ? __builtin_nanf("") : render_unkey(khi);
}

// ---- colour.  The three bytes of output pixel (y, x) in the low 24 bits, R lowest.
template <bool BILINEAR, bool BLEND>
__device__ __forceinline__ uint32_t render_pixel(const RenderLaunch &A, const float *map, const uint8_t *image,
                                                 int64_t image_stride, const uint32_t *lut, float lo, float span, int y, int x) {
  const int h = A.h, w = A.w;
  float v;
  if (BILINEAR) {
    // torch's align_corners=False source index, clamped below at 0; y0 <= h - 1 follows from fy < h - 0.5 (the min is a guard).
    // The product and the subtraction are ONE fused operation, stated as such (the unit's -ffp-contract=off fuses nothing on
    // its own): torch's builds contract scale * (y + 0.5) - 0.5, and a product near 60 rounded first moves ly by 2^-19
    float fy = __builtin_fmaf(A.sy, (float)y + 0.5f, -0.5f), fx = __builtin_fmaf(A.sx, (float)x + 0.5f, -0.5f);
    fy = fy < 0.0f ? 0.0f : fy, fx = fx < 0.0f ? 0.0f : fx;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 < h - 1 ? y0 : h - 1, x0 = x0 < w - 1 ? x0 : w - 1;
    const int y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1, x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1;
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float a00 = map[y0 * w + x0], a01 = map[y0 * w + x1], a10 = map[y1 * w + x0], a11 = map[y1 * w + x1];
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    v = hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11);
  } else {
    int sy = (int)floorf((float)y * A.sy), sx = (int)floorf((float)x * A.sx);
    sy = sy < h - 1 ? sy : h - 1, sx = sx < w - 1 ? sx : w - 1;
    v = map[sy * w + sx];
  }
  // Colormap._get_rgba_and_mask for a float array: xa = t * N, xa == N -> N - 1, then under / over / bad
  const float xa = __fdiv_rn(v - lo, span) * 256.0f;
  int row;
  if (!(xa == xa)) row = RENDER_ROW_BAD;
  else if (xa < 0.0f) row = RENDER_ROW_UNDER;
  else if (xa == 256.0f) row = 255;
  else if (xa >= 256.0f) row = RENDER_ROW_OVER;
  else row = (int)xa;
  const uint32_t col = lut[row];
  if (!BLEND) return col;
  const uint8_t *px = image + (int64_t)y * image_stride + x * 3;
  const uint32_t img = (uint32_t)px[0] | (uint32_t)px[1] << 8 | (uint32_t)px[2] << 16;
  if (row == RENDER_ROW_BAD) return img;      // matplotlib's bad colour is transparent: the picture shows
  uint32_t o = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float f = (float)((col >> (8 * c)) & 255u) * A.alpha + (float)((img >> (8 * c)) & 255u) * A.beta + 0.5f;
    o |= (uint32_t)(int)f << (8 * c);
  }
  return o;
}

template <bool BILINEAR, bool BLEND>
__global__ __launch_bounds__(RENDER_THREADS) void ca_render_colour_kernel(RenderLaunch A) {
  __shared__ uint32_t lut[RENDER_LUT_ROWS + 1];
  const RenderGroup &G = A.g[blockIdx.y];
  const int tid = threadIdx.x;
  for (int i = tid; i < RENDER_LUT_ROWS; i += RENDER_THREADS) {
    const uint8_t *r = A.lut + i * 3;
    lut[i] = (uint32_t)r[0] | (uint32_t)r[1] << 8 | (uint32_t)r[2] << 16;
  }
  __syncthreads();
  const float lo = G.range_out[0], hi = G.range_out[1];
  const float span = hi - lo;
  const int W = A.W, nbytes = A.H * W * 3;
  const uint32_t items = (uint32_t)G.n_maps * A.cpp;          // (<= 65536 * 12289: below 2^31, checked by the entry)
  for (uint32_t it = blockIdx.x; it < items; it += gridDim.x) {
    const uint32_t plane = it / A.cpp, chunk = it - plane * A.cpp;
    const float *map = G.maps + (int64_t)plane * G.map_stride;
    uint8_t *dst = G.out + (int64_t)plane * G.out_stride;
    const int mis = (int)((uintptr_t)dst & 15);
    const int b0 = (int)(chunk * RENDER_THREADS + tid) * 16 - mis;   // the slot's first byte, as an offset into the plane
    if (b0 >= nbytes) continue;
    if (b0 >= 0 && b0 + 16 <= nbytes) {
      const int p0 = b0 / 3, c0 = b0 - p0 * 3;
      int y = p0 / W, x = p0 - y * W;
      uint32_t col[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {                             // pixel p0 + 5 holds byte b0 + 15 for every c0
        col[j] = render_pixel<BILINEAR, BLEND>(A, map, G.image, G.image_stride, lut, lo, span, y, x);
        if (++x == W) x = 0, ++y;
      }
      const uint32_t s0 = col[0] | col[1] << 24, s1 = col[1] >> 8 | col[2] << 16, s2 = col[2] >> 16 | col[3] << 8;
      const uint32_t s3 = col[4] | col[5] << 24, s4 = col[5] >> 8;
      u32x4 o;
      o[0] = __builtin_amdgcn_alignbyte(s1, s0, (uint32_t)c0);
      o[1] = __builtin_amdgcn_alignbyte(s2, s1, (uint32_t)c0);
      o[2] = __builtin_amdgcn_alignbyte(s3, s2, (uint32_t)c0);
      o[3] = __builtin_amdgcn_alignbyte(s4, s3, (uint32_t)c0);
      *(u32x4 *)(dst + b0) = o;
    } else {                                                    // a plane's ragged first or last slot: byte by byte
      const int bs = b0 > 0 ? b0 : 0, be = b0 + 16 < nbytes ? b0 + 16 : nbytes;
      for (int b = bs; b < be; ++b) {
        const int p = b / 3, y = p / W;
        const uint32_t c = render_pixel<BILINEAR, BLEND>(A, map, G.image, G.image_stride, lut, lo, span, y, p - y * W);
        dst[b] = (uint8_t)(c >> (8 * (b - p * 3)));
      }
    }
  }
}

extern "C" int ca_heatmap_render(const ca_render_problem *problems, int32_t n_problems, int32_t h, int32_t w, int32_t H,
                                 int32_t W, const void *lut, float alpha, int32_t flags, ca_stream_t stream) {
  const char *FN = "ca_heatmap_render";
  if (!problems || n_problems < 1 || n_problems > CA_RENDER_MAX_PROBLEMS) {
    ca_set_error("%s: n_problems=%d outside 1..%d (or problems is NULL)", FN, n_problems, CA_RENDER_MAX_PROBLEMS);
    return CA_ERR_ARG;
  }
  if (h < 1 || w < 1 || (int64_t)h * w > RENDER_MAX_CELLS) {
    ca_set_error("%s: map %d x %d: h * w must be in 1..%d", FN, h, w, RENDER_MAX_CELLS);
    return CA_ERR_ARG;
  }
  if (H < 1 || W < 1 || H > RENDER_MAX_SIDE || W > RENDER_MAX_SIDE) {
    ca_set_error("%s: output %d x %d: H and W must be in 1..%d", FN, H, W, RENDER_MAX_SIDE);
    return CA_ERR_ARG;
  }
  if (flags & ~(CA_RENDER_BILINEAR | CA_RENDER_BLEND)) {
    ca_set_error("%s: flags=%d has bits outside CA_RENDER_BILINEAR | CA_RENDER_BLEND (1 | 2)", FN, flags);
    return CA_ERR_ARG;
  }
  const bool blend = flags & CA_RENDER_BLEND;
  if (blend && !(alpha >= 0.0f && alpha <= 1.0f)) {
    ca_set_error("%s: alpha=%g outside 0..1", FN, (double)alpha);
    return CA_ERR_ARG;
  }
  if (!lut) {
    ca_set_error("%s: lut is NULL (uint8 [259, 3] on the device)", FN);
    return CA_ERR_ARG;
  }
  RenderLaunch A = {};
  const int64_t hw = (int64_t)h * w, plane_bytes = (int64_t)H * W * 3;
  int max_maps = 0;
  bool need_range = false;
  for (int i = 0; i < n_problems; ++i) {
    const ca_render_problem &p = problems[i];
    if (p.n_maps < 1 || p.n_maps > CA_RENDER_MAX_MAPS) {
      ca_set_error("%s: problem %d: n_maps=%d outside 1..%d", FN, i, p.n_maps, CA_RENDER_MAX_MAPS);
      return CA_ERR_ARG;
    }
    if (p.n_maps > 1 && p.map_stride < hw) {
      ca_set_error("%s: problem %d: map_stride=%lld below h * w = %lld", FN, i, (long long)p.map_stride, (long long)hw);
      return CA_ERR_ARG;
    }
    if (p.n_maps > 1 && p.out_stride < plane_bytes) {
      ca_set_error("%s: problem %d: out_stride=%lld below 3 H W = %lld", FN, i, (long long)p.out_stride,
                   (long long)plane_bytes);
      return CA_ERR_ARG;
    }
    if (!p.maps || !p.range_out || !p.out || ((uintptr_t)p.maps & 3) || ((uintptr_t)p.range_out & 3) ||
        ((uintptr_t)p.range_in & 3)) {
      ca_set_error("%s: problem %d: maps, range_out and out non-null; maps, range_in and range_out 4-byte aligned", FN, i);
      return CA_ERR_ARG;
    }
    if (blend && (!p.image || (H > 1 && p.image_stride < (int64_t)W * 3))) {
      ca_set_error("%s: problem %d: CA_RENDER_BLEND needs an image with image_stride=%lld >= 3 W = %d bytes", FN, i,
                   (long long)p.image_stride, W * 3);
      return CA_ERR_ARG;
    }
    RenderGroup &g = A.g[i];
    g.maps = p.maps, g.range_in = p.range_in, g.range_out = p.range_out;
    g.image = blend ? (const uint8_t *)p.image : nullptr, g.out = (uint8_t *)p.out;
    g.map_stride = p.n_maps > 1 ? p.map_stride : 0, g.out_stride = p.n_maps > 1 ? p.out_stride : 0;
    g.image_stride = H > 1 ? p.image_stride : 0;
    g.n_maps = p.n_maps;
    max_maps = p.n_maps > max_maps ? p.n_maps : max_maps;
    need_range |= !p.range_in;
  }
  A.lut = (const uint8_t *)lut;
  A.h = h, A.w = w, A.H = H, A.W = W;
  A.alpha = alpha, A.beta = 1.0f - alpha;
  A.sy = (float)h / (float)H, A.sx = (float)w / (float)W;
  const int64_t slots = (plane_bytes + 15 + 15) / 16;          // a plane that starts 15 bytes into its first slot
  A.cpp = (uint32_t)((slots + RENDER_THREADS - 1) / RENDER_THREADS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ca_render_prep_kernel, dim3((unsigned)n_problems), dim3(CA_WAVE), 0, st, A);
  int rc = ca_check_launch(FN);
  if (rc != CA_OK) return rc;
  if (need_range) {
    const int gx = max_maps < RENDER_RANGE_BLOCKS ? max_maps : RENDER_RANGE_BLOCKS;
    hipLaunchKernelGGL(ca_render_range_kernel, dim3((unsigned)gx, (unsigned)n_problems), dim3(RENDER_THREADS), 0, st, A);
    if ((rc = ca_check_launch(FN)) != CA_OK) return rc;
    hipLaunchKernelGGL(ca_render_decode_kernel, dim3((unsigned)n_problems), dim3(CA_WAVE), 0, st, A);
    if ((rc = ca_check_launch(FN)) != CA_OK) return rc;
  }
  int64_t gx = (int64_t)max_maps * A.cpp;
  const int64_t cap = RENDER_MAX_BLOCKS / n_problems;
  gx = gx < cap ? gx : cap;
  const dim3 grid((unsigned)gx, (unsigned)n_problems), block(RENDER_THREADS);
  const bool bil = flags & CA_RENDER_BILINEAR;
  if (bil && blend) hipLaunchKernelGGL((ca_render_colour_kernel<true, true>), grid, block, 0, st, A);
  else if (bil) hipLaunchKernelGGL((ca_render_colour_kernel<true, false>), grid, block, 0, st, A);
  else if (blend) hipLaunchKernelGGL((ca_render_colour_kernel<false, true>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((ca_render_colour_kernel<false, false>), grid, block, 0, st, A);
  return ca_check_launch(FN);
}
