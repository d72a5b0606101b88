// Pixel I/O of the autoencoder: the bytes of an image straight into the zero-padded bf16 input plane of conv_in (resize,
// [-1, 1] scaling and cast in one pass), and the decoder's fp32 NHWC output straight to bytes.  Both are element-wise
// and bound by memory traffic: 16-byte stores, a grid capped at 2048 workgroups that strides over the rest, every
// element offset formed in 64 bits.  The unit is compiled with -ffp-contract=off: every operation below rounds on its
// own, as the torch expressions they restate do.
#include "ca_common.h"

#define PIX_MAX_BLOCKS 2048   // 256 CUs x 8 workgroups of 256 threads
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // (one 16-byte store: hipcc splits a uint4 struct with constant halves)

// ------------------------------------------------------------------------------------------------------------------
// dst[y, x, 0:3] = bf16_rne(2 * (float(src[sy, sx, c]) / 255) - 1), dst[y, x, 3:32] = 0, with the source pixel of
// torch's interpolate(mode="nearest"): sy = min((int)floorf(y * scale_y), H0 - 1), scale_y = (float)H0 / (float)H formed
// on the host (an IEEE division), the product in fp32.  The division by 255 is the correctly rounded one (a reciprocal
// multiply differs in the last bit for some of the 256 byte values).  Four threads per pixel, one 16-byte store each: a
// wave writes 1 KiB of contiguous plane per store instruction; the thread of channels 0..7 reads the 3 bytes.
__global__ __launch_bounds__(256) void ca_pixels_u8_to_nhwc32_kernel(const uint8_t *src, long src_stride, bf16 *dst, int H0,
                                                                      int W0, int H, int W, float scale_y, float scale_x) {
  const long total = (long)H * W * 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    u32x4 o = {0u, 0u, 0u, 0u};
    if ((i & 3) == 0) {
      const long p = i >> 2;
      const int y = (int)(p / W), x = (int)(p - (long)y * W);
      int sy = (int)floorf((float)y * scale_y), sx = (int)floorf((float)x * scale_x);
      sy = sy < H0 - 1 ? sy : H0 - 1;
      sx = sx < W0 - 1 ? sx : W0 - 1;
      const uint8_t *s = src + (long)sy * src_stride + (long)sx * 3;
      const float r = 2.0f * __fdiv_rn((float)s[0], 255.0f) - 1.0f;
      const float g = 2.0f * __fdiv_rn((float)s[1], 255.0f) - 1.0f;
      const float b = 2.0f * __fdiv_rn((float)s[2], 255.0f) - 1.0f;
      o.x = ca_pack2(r, g);
      o.y = ca_pack2(b, 0.f);
    }
    *(u32x4 *)(dst + i * 8) = o;
  }
}

extern "C" int ca_pixels_u8_to_nhwc32_bf16(const void *src, int64_t src_stride, void *dst, int32_t H0, int32_t W0, int32_t H,
                                           int32_t W, ca_stream_t stream) {
  const char *FN = "ca_pixels_u8_to_nhwc32_bf16";
  if (!src || !dst || H0 < 1 || W0 < 1 || H < 1 || W < 1 || (H0 > 1 && src_stride < (int64_t)W0 * 3) || ((uintptr_t)dst & 15)) {
    ca_set_error("%s: bad arguments (source %d x %d [>= 1], destination %d x %d [>= 1], src_stride=%lld bytes [>= 3 W0 when H0 > 1]; "
                 "src and dst non-null, dst 16-byte aligned)", FN, H0, W0, H, W, (long long)src_stride);
    return CA_ERR_ARG;
  }
  // the nearest index is exact in fp32 only while y and x are: far above any image (the conv kernel stops at 2^31 rows)
  if (H > (1 << 24) || W > (1 << 24) || H0 > (1 << 24) || W0 > (1 << 24)) {
    ca_set_error("%s: sizes above 2^24 are not representable in the fp32 index rule", FN);
    return CA_ERR_ARG;
  }
  const long total = (long)H * W * 4;
  long blocks = (total + 255) / 256;
  if (blocks > PIX_MAX_BLOCKS) blocks = PIX_MAX_BLOCKS;
  const float scale_y = (float)H0 / (float)H, scale_x = (float)W0 / (float)W;
  hipLaunchKernelGGL(ca_pixels_u8_to_nhwc32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t *)src, (long)src_stride, (bf16 *)dst, H0, W0, H, W, scale_y, scale_x);
  return ca_check_launch(FN);
}

// ------------------------------------------------------------------------------------------------------------------
// dst[p, c] = (uint8)truncf(127.5f * (min(max(src[p, c], -1), 1) + 1.0f)) for c < 3: the sum and the product are two
// roundings, exactly (127.5 * (img.clamp(-1, 1) + 1.0)).byte().  fmaxf / fminf return the other operand for a NaN, so
// a NaN becomes -1 and then 0 (torch leaves that conversion undefined).
//
// The unit of work is 16 OUTPUT BYTES, one 16-byte store, and consecutive lanes own consecutive units: a wave writes
// 1 KiB of contiguous bytes per store instruction.  Byte b of the image is channel b % 3 of pixel b / 3.  With ld == 3
// (the decoder's buffer) byte b comes from float b: a lane reads its 16 floats as four 16-byte loads and a wave reads 4 KiB
// of contiguous floats (PACKED; src 16-byte aligned).  Any other ld walks the 16 floats pixel by pixel.  The bytes behind
// the last full unit (pixels * 3 is no multiple of 16 for most sizes) are written one by one by one thread.
__device__ __forceinline__ uint32_t pix_byte(float x) {
  const float v = fminf(fmaxf(x, -1.0f), 1.0f);
  return (uint32_t)(int)truncf(127.5f * (v + 1.0f));
}

template <bool PACKED>
__global__ __launch_bounds__(256) void ca_nhwc_f32_to_pixels_kernel(const float *src, long ld, uint8_t *dst, long nbytes) {
  const long units = (nbytes + 15) / 16;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < units; i += (long)gridDim.x * 256) {
    const long b0 = i * 16;
    if (b0 + 16 <= nbytes) {
      float v[16];
      if (PACKED) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 a = *(const f32x4 *)(src + b0 + q * 4);
          v[q * 4] = a[0], v[q * 4 + 1] = a[1], v[q * 4 + 2] = a[2], v[q * 4 + 3] = a[3];
        }
      } else {
        const long p = b0 / 3;
        int c = (int)(b0 - p * 3);
        const float *s = src + p * ld + c;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          v[k] = *s;
          s += c == 2 ? ld - 2 : 1;          // the next channel, or channel 0 of the next pixel
          c = c == 2 ? 0 : c + 1;
        }
      }
      u32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        o[q] = pix_byte(v[q * 4]) | pix_byte(v[q * 4 + 1]) << 8 | pix_byte(v[q * 4 + 2]) << 16 | pix_byte(v[q * 4 + 3]) << 24;
      *(u32x4 *)(dst + b0) = o;
    } else {
      for (long b = b0; b < nbytes; ++b) {
        const long p = b / 3;
        dst[b] = (uint8_t)pix_byte(src[p * ld + (b - p * 3)]);
      }
    }
  }
}

extern "C" int ca_nhwc_f32_to_pixels_u8(const float *src, int32_t ld, void *dst, int64_t pixels, ca_stream_t stream) {
  const char *FN = "ca_nhwc_f32_to_pixels_u8";
  if (!src || !dst || pixels < 1 || ld < 3 || ((uintptr_t)src & 3) || ((uintptr_t)dst & 15) ||
      pixels > (int64_t)1 << 40) {
    ca_set_error("%s: bad arguments (pixels=%lld [1..2^40] ld=%d [>= 3]; src and dst non-null, src 4-byte and dst 16-byte "
                 "aligned)", FN, (long long)pixels, ld);
    return CA_ERR_ARG;
  }
  const long nbytes = (long)pixels * 3;
  long blocks = ((nbytes + 15) / 16 + 255) / 256;
  if (blocks > PIX_MAX_BLOCKS) blocks = PIX_MAX_BLOCKS;
  if (ld == 3 && !((uintptr_t)src & 15))
    hipLaunchKernelGGL(ca_nhwc_f32_to_pixels_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src,
                       (long)ld, (uint8_t *)dst, nbytes);
  else
    hipLaunchKernelGGL(ca_nhwc_f32_to_pixels_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src,
                       (long)ld, (uint8_t *)dst, nbytes);
  return ca_check_launch(FN);
}
