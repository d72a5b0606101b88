// Scoring of the zero-shot segmentation on the device: the target concept's heat map against a label
// image -> the mask, the min-max coefficient, the confusion counts of mask against label and the EXACT average precision
// of the stacked scores (1 - c, c) against the one-hot label, one workgroup per item, nothing sorted per pixel.
//
// What makes it cheap: after the nearest resize the Hl x Wl scores take at most h w distinct values per class, and the
// AP depends only on how many pixels and how many positives share each value.  A workgroup therefore counts, per map
// cell, the label pixels that read it (tot) and the positive ones among them (pos), sorts the at most 2 h w
// (score, cell, class) entries in LDS and walks the sorted thresholds once.
//
// The arithmetic restates conceptattention_amd/segmentation.py (target_mask, prepare_for_scoring, SegmentationScores.
// update / get_ap_scores / average_precision) one rounding at a time; tests/seg_cases.py holds the same statement in
// numpy.  The unit is compiled with -ffp-contract=off: every operation below rounds on its own.
//
// LDS (dynamic, one carve): sort entries u64 [npad] | x fp32 [hw4] | tot u32 [hw4] | pos u32 [hw4] | scratch;
// npad = the power of two >= 2 h w, hw4 = h w rounded up to 4: 112.5 KB at 64 x 64.
#include "ca_common.h"

#define SEG_THREADS 1024
#define SEG_WAVES (SEG_THREADS / CA_WAVE)
#define SEG_MAX_CELLS 4096
#define SEG_SCRATCH_BYTES 512

struct SegLaunch {
  ca_seg_problem p[CA_SEG_MAX_PROBLEMS];
  int32_t h, w, Hl, Wl, flags, npad;
  float sy, sx;            // (float)h / Hl, (float)w / Wl: the nearest rule's scales, formed on the host
  float sy14, sx14;        // 14.0f / Hl, 14.0f / Wl           (downscale_for_eval: label pixel -> 14 x 14)
  float s14y, s14x;        // (float)h / 14.0f, (float)w / 14.0f (14 x 14 -> map cell)
  float blur[9];
};

struct SegRecord {          // ca_seg_record of the header, 40 bytes
  int32_t n11, n10, n01, n00;
  double ap;
  float mean, lo, hi;
  int32_t thresholds;
};
static_assert(sizeof(SegRecord) == 40, "ca_seg_record is 40 bytes");

// torch's interpolate(mode="nearest") source index (the rule of ca_pixels.hip): the product in fp32
__device__ __forceinline__ int seg_near(int i, float scale, int n_in) {
  const int s = (int)floorf((float)i * scale);
  return s < n_in - 1 ? s : n_in - 1;
}

__device__ __forceinline__ int seg_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// a float as an unsigned key of the same order; -0.0 and NaN were removed before
__device__ __forceinline__ uint32_t seg_ordkey(float s) {
  const uint32_t b = __builtin_bit_cast(uint32_t, s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// exclusive scan over the workgroup's threads in thread order (sum, or max: 0 is the identity of both on unsigned)
template <bool MAX>
__device__ __forceinline__ uint32_t seg_scan_excl(uint32_t v, uint32_t *wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(inc, off);
    if (lane >= off) inc = MAX ? (inc > u ? inc : u) : inc + u;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int i = 0; i < wave; ++i) base = MAX ? (base > wsum[i] ? base : wsum[i]) : base + wsum[i];
  __syncthreads();          // (wsum is free again)
  uint32_t prev = __shfl_up(inc, 1);
  if (lane == 0) prev = 0;
  return MAX ? (base > prev ? base : prev) : base + prev;
}

__global__ __launch_bounds__(SEG_THREADS) void ca_seg_score_kernel(SegLaunch A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char seg_lds[];
  const ca_seg_problem P = A.p[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = A.h, w = A.w, hw = h * w, hw4 = (hw + 3) & ~3, npad = A.npad;
  unsigned long long *ent = (unsigned long long *)seg_lds;
  float *x = (float *)(seg_lds + (size_t)npad * 8);
  uint32_t *tot = (uint32_t *)(x + hw4);
  uint32_t *pos = tot + hw4;
  unsigned char *scratch = (unsigned char *)(pos + hw4);
  double *dsum = (double *)scratch;                 // [16]
  uint32_t *wsum = (uint32_t *)(scratch + 128);     // [16]
  float *fmin_w = (float *)(scratch + 192);         // [16]
  float *fmax_w = (float *)(scratch + 256);         // [16]
  int32_t *cnt = (int32_t *)(scratch + 320);        // n11, n10, n01, n00, valid entries, thresholds
  const float *map = P.map;

  // ---- 1. x = the map, or its 3x3 blur with reflect padding (nine rounded products, summed in row-major order)
  for (int c = tid; c < hw; c += SEG_THREADS) {
    float v;
    if (A.flags & CA_SEG_BLUR) {
      const int y = c / w, xx = c - y * w;
      v = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const long o = (long)seg_reflect(y + i - 1, h) * w + seg_reflect(xx + j - 1, w);
          const float prod = A.blur[i * 3 + j] * map[o];
          v = (i | j) ? v + prod : prod;
        }
    } else {
      v = map[(long)c];
    }
    x[c] = v;
    tot[c] = 0, pos[c] = 0;
  }
  if (tid < 6) cnt[tid] = 0;
  __syncthreads();

  // ---- 2. lo, hi (order-free) and the fp64 sum over a fixed tree: thread t adds cells t, t + 1024, ... in that order,
  // a wave adds its lanes as a butterfly (32, 16, ..., 1), the 16 wave sums are added in wave order
  float lo = INFINITY, hi = -INFINITY;
  double s = 0.0;
  for (int c = tid; c < hw; c += SEG_THREADS) {
    const float v = x[c];
    lo = fminf(lo, v), hi = fmaxf(hi, v);
    s += (double)v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off));
    hi = fmaxf(hi, __shfl_xor(hi, off));
    s += __shfl_xor(s, off);
  }
  if (lane == 0) dsum[wave] = s, fmin_w[wave] = lo, fmax_w[wave] = hi;
  __syncthreads();
  s = 0.0;
  for (int i = 0; i < SEG_WAVES; ++i) {
    s += dsum[i];
    lo = i ? fminf(lo, fmin_w[i]) : fmin_w[0];
    hi = i ? fmaxf(hi, fmax_w[i]) : fmax_w[0];
  }
  const float mean = (float)(s / (double)hw);
  const float thr = (A.flags & CA_SEG_MEAN_THRESHOLD) ? mean : 0.0f;
  const float range = hi - lo;
  __syncthreads();          // (dsum is free again)

  // ---- 3 / 4. the optional outputs at map resolution
  if (P.mask_out || P.coeff_out)
    for (int c = tid; c < hw; c += SEG_THREADS) {
      const float v = x[c];
      if (P.mask_out) ((uint8_t *)P.mask_out)[(long)c] = v > thr ? 1 : 0;
      if (P.coeff_out) P.coeff_out[(long)c] = __fdiv_rn(v - lo, range);
    }

  // ---- 5. every label pixel: the confusion counts and the two tables of its coefficient cell
  {
    const uint8_t *label = (const uint8_t *)P.label;
    const long N = (long)A.Hl * A.Wl;
    const bool down = A.flags & CA_SEG_DOWNSCALE;
    int n11 = 0, n10 = 0, n01 = 0, n00 = 0;
    for (long i = tid; i < N; i += SEG_THREADS) {
      const int Y = (int)(i / A.Wl), X = (int)(i - (long)Y * A.Wl);
      const int my = seg_near(Y, A.sy, h), mx = seg_near(X, A.sx, w);
      int cy = my, cx = mx;
      if (down) {
        cy = seg_near(seg_near(Y, A.sy14, 14), A.s14y, h);
        cx = seg_near(seg_near(X, A.sx14, 14), A.s14x, w);
      }
      const bool m = x[my * w + mx] > thr;
      const bool l = label[i] != 0;
      n11 += m & l, n10 += m & !l, n01 += !m & l, n00 += !m & !l;
      const int cell = cy * w + cx;
      atomicAdd(&tot[cell], 1u);
      if (l) atomicAdd(&pos[cell], 1u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      n11 += __shfl_xor(n11, off), n10 += __shfl_xor(n10, off);
      n01 += __shfl_xor(n01, off), n00 += __shfl_xor(n00, off);
    }
    if (lane == 0) atomicAdd(&cnt[0], n11), atomicAdd(&cnt[1], n10), atomicAdd(&cnt[2], n01), atomicAdd(&cnt[3], n00);
  }
  __syncthreads();

  // ---- 6. the entries: class 1 of a cell scores c, class 0 float32(1 - c); NaN -> 0; cells no pixel reads are dropped.
  // entry = ordered score key << 32 | cell * 2 + class, 0 = no entry (every real key is above 0)
  {
    int valid = 0;
    for (int e = tid; e < npad; e += SEG_THREADS) {
      unsigned long long v = 0;
      const int cell = e >> 1;
      if (cell < hw && tot[cell] != 0) {
        const float c = __fdiv_rn(x[cell] - lo, range);
        float sc = (e & 1) ? c : 1.0f - c;
        if (!(sc == sc) || sc == 0.0f) sc = 0.0f;      // nan_to_num; -0.0 == 0.0 is one threshold
        v = (unsigned long long)seg_ordkey(sc) << 32 | (uint32_t)e;
        ++valid;
      }
      ent[e] = v;
    }
    if (valid) atomicAdd(&cnt[4], valid);
  }
  __syncthreads();
  // bitonic sort, descending: the entries are distinct, so the order is unique
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (npad >> 1); i += SEG_THREADS) {
        const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
        const unsigned long long u = ent[a], v = ent[b];
        if ((u < v) == ((a & k) == 0)) ent[a] = v, ent[b] = u;
      }
      __syncthreads();
    }

  // ---- thresholds: thread t owns E consecutive sorted entries; prefix sums of pixels and positives in integers
  const int m = cnt[4];
  const int E = (npad + SEG_THREADS - 1) / SEG_THREADS;
  const int k0 = tid * E < m ? tid * E : m, k1 = k0 + E < m ? k0 + E : m;
  uint32_t sum_n = 0, sum_p = 0, last_end = 0;      // last_end: positives up to the thread's last threshold (relative)
  bool has_end = false;
  for (int k = k0; k < k1; ++k) {
    const unsigned long long e = ent[k];
    const uint32_t cell = ((uint32_t)e) >> 1, t = tot[cell], p = pos[cell];
    sum_n += t, sum_p += (e & 1) ? p : t - p;
    if (k == m - 1 || (uint32_t)(ent[k + 1] >> 32) != (uint32_t)(e >> 32)) has_end = true, last_end = sum_p;
  }
  const uint32_t ex_n = seg_scan_excl<false>(sum_n, wsum);
  const uint32_t ex_p = seg_scan_excl<false>(sum_p, wsum);
  // positives at the last threshold before the thread's entries: the running counts never fall, so a max scan finds it
  uint32_t prev = seg_scan_excl<true>(has_end ? ex_p + last_end : 0u, wsum);
  const double n_pos = (double)((long)A.Hl * A.Wl);   // every pixel is a positive of exactly one class
  double ap = 0.0;
  int nthr = 0;
  uint32_t cum_n = ex_n, cum_p = ex_p;
  for (int k = k0; k < k1; ++k) {
    const unsigned long long e = ent[k];
    const uint32_t cell = ((uint32_t)e) >> 1, t = tot[cell], p = pos[cell];
    cum_n += t, cum_p += (e & 1) ? p : t - p;
    if (k == m - 1 || (uint32_t)(ent[k + 1] >> 32) != (uint32_t)(e >> 32)) {
      const double prec = (double)cum_p / (double)cum_n;
      const double rec = (double)cum_p / n_pos, rec_prev = (double)prev / n_pos;
      ap += (rec - rec_prev) * prec;
      prev = cum_p;
      ++nthr;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ap += __shfl_xor(ap, off);
    nthr += __shfl_xor(nthr, off);
  }
  if (lane == 0) dsum[wave] = ap, atomicAdd(&cnt[5], nthr);
  __syncthreads();
  if (tid == 0) {
    ap = 0.0;
    for (int i = 0; i < SEG_WAVES; ++i) ap += dsum[i];
    SegRecord r;
    r.n11 = cnt[0], r.n10 = cnt[1], r.n01 = cnt[2], r.n00 = cnt[3];
    r.ap = ap;
    r.mean = mean, r.lo = lo, r.hi = hi;
    r.thresholds = cnt[5];
    *(SegRecord *)P.result = r;
  }
}

extern "C" int ca_seg_score(const ca_seg_problem *problems, int32_t n_problems, int32_t h, int32_t w, int32_t Hl, int32_t Wl,
                            int32_t flags, const float *blur_weights, ca_stream_t stream) {
  const char *FN = "ca_seg_score";
  if (!problems || n_problems < 1 || n_problems > CA_SEG_MAX_PROBLEMS) {
    ca_set_error("%s: n_problems=%d outside 1..%d, or problems is null", FN, n_problems, CA_SEG_MAX_PROBLEMS);
    return CA_ERR_ARG;
  }
  if (h < 1 || w < 1 || (int64_t)h * w > SEG_MAX_CELLS) {
    ca_set_error("%s: map %d x %d: h * w must be in 1..%d (larger maps are scored on the host)", FN, h, w, SEG_MAX_CELLS);
    return CA_ERR_ARG;
  }
  if (Hl < 1 || Wl < 1 || (int64_t)Hl * Wl > ((int64_t)1 << 24)) {
    ca_set_error("%s: label %d x %d: Hl * Wl must be in 1..2^24", FN, Hl, Wl);
    return CA_ERR_ARG;
  }
  if (flags & ~(CA_SEG_MEAN_THRESHOLD | CA_SEG_DOWNSCALE | CA_SEG_BLUR)) {
    ca_set_error("%s: flags=%d has bits outside CA_SEG_MEAN_THRESHOLD | CA_SEG_DOWNSCALE | CA_SEG_BLUR", FN, flags);
    return CA_ERR_ARG;
  }
  if ((flags & CA_SEG_BLUR) && (h < 2 || w < 2 || !blur_weights)) {
    ca_set_error("%s: the blur's reflect padding needs h >= 2 and w >= 2 (map %d x %d) and nine blur_weights", FN, h, w);
    return CA_ERR_ARG;
  }
  SegLaunch A = {};
  for (int i = 0; i < n_problems; ++i) {
    const ca_seg_problem &p = problems[i];
    if (!p.map || !p.label || !p.result || ((uintptr_t)p.map & 3) || ((uintptr_t)p.result & 7) || ((uintptr_t)p.coeff_out & 3)) {
      ca_set_error("%s: problem %d invalid (map, label and result non-null; map and coeff_out 4-byte, result 8-byte aligned)",
                   FN, i);
      return CA_ERR_ARG;
    }
    A.p[i] = p;
  }
  const int hw = h * w;
  int npad = 2;
  while (npad < 2 * hw) npad <<= 1;
  A.h = h, A.w = w, A.Hl = Hl, A.Wl = Wl, A.flags = flags, A.npad = npad;
  A.sy = (float)h / (float)Hl, A.sx = (float)w / (float)Wl;
  A.sy14 = 14.0f / (float)Hl, A.sx14 = 14.0f / (float)Wl;
  A.s14y = (float)h / 14.0f, A.s14x = (float)w / 14.0f;
  if (flags & CA_SEG_BLUR)
    for (int i = 0; i < 9; ++i) A.blur[i] = blur_weights[i];
  const size_t lds = (size_t)npad * 8 + (size_t)((hw + 3) & ~3) * 12 + SEG_SCRATCH_BYTES;
  if (lds > 64 * 1024) {   // above 2048 cells (npad 8192: 57 856 -> 90 672 bytes): above the default dynamic LDS limit
    static std::atomic<unsigned long long> attr_done{0};
    const int rc = ca_raise_lds_limit({(const void *)ca_seg_score_kernel},
                                      SEG_MAX_CELLS * 2 * 8 + SEG_MAX_CELLS * 12 + SEG_SCRATCH_BYTES, attr_done, FN);
    if (rc != CA_OK) return rc;
  }
  hipLaunchKernelGGL(ca_seg_score_kernel, dim3((unsigned)n_problems), dim3(SEG_THREADS), lds, (hipStream_t)stream, A);
  return ca_check_launch(FN);
}
