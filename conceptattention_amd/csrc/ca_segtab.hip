// Scoring of a TABLE of heat maps against one label image (the per-layer x per-noise-level sweep of SURVEY.md §8f-3;
// experiments/per_layer_segmentation/test_segmentations_per_layer.py:164-243 and
// experiments/per_timestep_segmentation/test_segmentations_per_time.py:75-174): every (level, layer) map of the target
// concept gets the record ca_seg.hip writes for a single map, from two launches for the whole table.
//
// What the table shares: which label pixels read which map cell depends on the geometry alone, never on the map.  The
// label pass therefore counts ONCE, per map cell, the label pixels that read it (tot) and the positive ones among them
// (pos), for the mask's pixel -> cell mapping and for the coefficient's (they differ only under CA_SEGTAB_DOWNSCALE),
// into the caller's `cells` workspace.  The map pass, one workgroup per map, never touches the label: the confusion
// counts are sums over cells of the mask tables, and the exact average precision comes from the sorted
// (score, cell, class) entries and the coefficient tables, as in ca_seg.hip.
//
// The arithmetic per map is ca_seg.hip's, one rounding at a time (tests/segtab_cases.py holds the numpy statement); with
// CA_SEGTAB_RAW the coefficient is the map value itself.  The unit is compiled with -ffp-contract=off.
//
// LDS of the map pass (dynamic, one carve): sort entries u64 [npad] | x fp32 [hw4] | tot u32 [hw4] | pos u32 [hw4] |
// scratch; npad = the power of two >= 2 h w, hw4 = h w rounded up to 4: 112.5 KB at 64 x 64.
#include "ca_common.h"

#define SEGTAB_THREADS 1024
#define SEGTAB_WAVES (SEGTAB_THREADS / CA_WAVE)
#define SEGTAB_MAX_CELLS 4096
#define SEGTAB_SCRATCH_BYTES 512
#define SEGTAB_LABEL_THREADS 256
#define SEGTAB_ROWS_MAX 65535      // label rows in gridDim.x at most; a block walks rows blockIdx.x, + gridDim.x, ...

struct SegtabLaunch {
  const float *maps;
  const uint8_t *label;
  void *records;
  uint32_t *cells;         // [4][hw4]: mask tot, mask pos, coefficient tot, coefficient pos
  int64_t map_stride;
  int32_t h, w, Hl, Wl, flags, npad;
  float sy, sx;            // (float)h / Hl, (float)w / Wl: the nearest rule's scales, formed on the host
  float sy14, sx14;        // 14.0f / Hl, 14.0f / Wl           (downscale: label pixel -> 14 x 14)
  float s14y, s14x;        // (float)h / 14.0f, (float)w / 14.0f (14 x 14 -> map cell)
  float blur[9];
};

struct SegtabRecord {       // ca_seg_record of the header, 40 bytes
  int32_t n11, n10, n01, n00;
  double ap;
  float mean, lo, hi;
  int32_t thresholds;
};
static_assert(sizeof(SegtabRecord) == 40, "ca_seg_record is 40 bytes");

// torch's interpolate(mode="nearest") source index (the rule of ca_pixels.hip): the product in fp32
__device__ __forceinline__ int segtab_near(int i, float scale, int n_in) {
  const int s = (int)floorf((float)i * scale);
  return s < n_in - 1 ? s : n_in - 1;
}

__device__ __forceinline__ int segtab_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// a float as an unsigned key of the same order; -0.0 and NaN were removed before
__device__ __forceinline__ uint32_t segtab_ordkey(float s) {
  const uint32_t b = __builtin_bit_cast(uint32_t, s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// np.nan_to_num on fp32, and one zero: NaN -> 0, +-inf -> +-FLT_MAX, -0.0 -> 0.0
__device__ __forceinline__ float segtab_score(float s) {
  if (!(s == s) || s == 0.0f) return 0.0f;
  if (s == INFINITY) return 3.402823466e+38f;
  if (s == -INFINITY) return -3.402823466e+38f;
  return s;
}

// exclusive scan over the workgroup's threads in thread order (sum, or max: 0 is the identity of both on unsigned)
template <bool MAX>
__device__ __forceinline__ uint32_t segtab_scan_excl(uint32_t v, uint32_t *wsum) {
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

__global__ __launch_bounds__(SEGTAB_LABEL_THREADS) void ca_segtab_zero_kernel(uint32_t *cells, int n) {
  const int i = blockIdx.x * SEGTAB_LABEL_THREADS + threadIdx.x;
  if (i < n) cells[i] = 0u;
}

// ---- the label pass.  A label row reads ONE row of cells under either mapping, so a workgroup counts its row in LDS
// (four tables of w bins) and adds the non-empty bins to the workspace: integer sums, any order gives the same bits.
__global__ __launch_bounds__(SEGTAB_LABEL_THREADS) void ca_segtab_label_kernel(SegtabLaunch A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char segtab_lds[];
  uint32_t *bins = (uint32_t *)segtab_lds;               // [4][w]
  const int tid = threadIdx.x, h = A.h, w = A.w, hw4 = (h * w + 3) & ~3;
  const bool down = A.flags & CA_SEGTAB_DOWNSCALE;
  for (int Y = blockIdx.x; Y < A.Hl; Y += gridDim.x) {
    for (int i = tid; i < 4 * w; i += SEGTAB_LABEL_THREADS) bins[i] = 0u;
    __syncthreads();
    const int my = segtab_near(Y, A.sy, h);
    const int cy = down ? segtab_near(segtab_near(Y, A.sy14, 14), A.s14y, h) : my;
    const uint8_t *row = A.label + (long)Y * A.Wl;
    for (int X = tid; X < A.Wl; X += SEGTAB_LABEL_THREADS) {
      const int mx = segtab_near(X, A.sx, w);
      const int cx = down ? segtab_near(segtab_near(X, A.sx14, 14), A.s14x, w) : mx;
      const bool l = row[X] != 0;
      atomicAdd(&bins[mx], 1u);
      atomicAdd(&bins[2 * w + cx], 1u);
      if (l) atomicAdd(&bins[w + mx], 1u), atomicAdd(&bins[3 * w + cx], 1u);
    }
    __syncthreads();
    for (int i = tid; i < 4 * w; i += SEGTAB_LABEL_THREADS) {
      const uint32_t v = bins[i];
      if (v) {
        const int t = i / w, xx = i - t * w;
        atomicAdd(&A.cells[(long)t * hw4 + (t < 2 ? my : cy) * w + xx], v);
      }
    }
    __syncthreads();
  }
}

// ---- the map pass: ca_seg_score_kernel step by step, the label loop replaced by sums over the tables
__global__ __launch_bounds__(SEGTAB_THREADS) void ca_segtab_map_kernel(SegtabLaunch A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char segtab_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = A.h, w = A.w, hw = h * w, hw4 = (hw + 3) & ~3, npad = A.npad;
  unsigned long long *ent = (unsigned long long *)segtab_lds;
  float *x = (float *)(segtab_lds + (size_t)npad * 8);
  uint32_t *tot = (uint32_t *)(x + hw4);
  uint32_t *pos = tot + hw4;
  unsigned char *scratch = (unsigned char *)(pos + hw4);
  double *dsum = (double *)scratch;                 // [16]
  uint32_t *wsum = (uint32_t *)(scratch + 128);     // [16]
  float *fmin_w = (float *)(scratch + 192);         // [16]
  float *fmax_w = (float *)(scratch + 256);         // [16]
  int32_t *cnt = (int32_t *)(scratch + 320);        // n11, n10, n01, n00, valid entries, thresholds
  const float *map = A.maps + (int64_t)blockIdx.x * A.map_stride;
  const uint32_t *mtot = A.cells, *mpos = A.cells + hw4;
  const bool raw = A.flags & CA_SEGTAB_RAW;

  // ---- 1. x = the map, or its 3x3 blur with reflect padding (nine rounded products, summed in row-major order); the
  // coefficient's tables come into LDS
  for (int c = tid; c < hw; c += SEGTAB_THREADS) {
    float v;
    if (A.flags & CA_SEGTAB_BLUR) {
      const int y = c / w, xx = c - y * w;
      v = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const long o = (long)segtab_reflect(y + i - 1, h) * w + segtab_reflect(xx + j - 1, w);
          const float prod = A.blur[i * 3 + j] * map[o];
          v = (i | j) ? v + prod : prod;
        }
    } else {
      v = map[(long)c];
    }
    x[c] = v;
    tot[c] = A.cells[2 * (long)hw4 + c], pos[c] = A.cells[3 * (long)hw4 + c];
  }
  if (tid < 6) cnt[tid] = 0;
  __syncthreads();

  // ---- 2. lo, hi (order-free) and the fp64 sum over a fixed tree: thread t adds cells t, t + 1024, ... in that order,
  // a wave adds its lanes as a butterfly (32, 16, ..., 1), the 16 wave sums are added in wave order
  float lo = INFINITY, hi = -INFINITY;
  double s = 0.0;
  for (int c = tid; c < hw; c += SEGTAB_THREADS) {
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
  for (int i = 0; i < SEGTAB_WAVES; ++i) {
    s += dsum[i];
    lo = i ? fminf(lo, fmin_w[i]) : fmin_w[0];
    hi = i ? fmaxf(hi, fmax_w[i]) : fmax_w[0];
  }
  const float mean = (float)(s / (double)hw);
  const float thr = (A.flags & CA_SEGTAB_MEAN_THRESHOLD) ? mean : 0.0f;
  const float range = hi - lo;
  __syncthreads();          // (dsum is free again)

  // ---- 5. the confusion counts: every cell hands its mask bit to the label pixels that read it
  {
    int n11 = 0, n10 = 0, n01 = 0, n00 = 0;
    for (int c = tid; c < hw; c += SEGTAB_THREADS) {
      const int t = (int)mtot[c], p = (int)mpos[c];
      if (x[c] > thr) n11 += p, n10 += t - p;
      else n01 += p, n00 += t - p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      n11 += __shfl_xor(n11, off), n10 += __shfl_xor(n10, off);
      n01 += __shfl_xor(n01, off), n00 += __shfl_xor(n00, off);
    }
    if (lane == 0) atomicAdd(&cnt[0], n11), atomicAdd(&cnt[1], n10), atomicAdd(&cnt[2], n01), atomicAdd(&cnt[3], n00);
  }

  // ---- 6. the entries: class 1 of a cell scores c, class 0 float32(1 - c), both through nan_to_num; cells no pixel
  // reads are dropped.  entry = ordered score key << 32 | cell * 2 + class, 0 = no entry (every real key is above 0)
  {
    int valid = 0;
    for (int e = tid; e < npad; e += SEGTAB_THREADS) {
      unsigned long long v = 0;
      const int cell = e >> 1;
      if (cell < hw && tot[cell] != 0) {
        const float c = raw ? x[cell] : __fdiv_rn(x[cell] - lo, range);
        const float sc = segtab_score((e & 1) ? c : 1.0f - c);
        v = (unsigned long long)segtab_ordkey(sc) << 32 | (uint32_t)e;
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
      for (int i = tid; i < (npad >> 1); i += SEGTAB_THREADS) {
        const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
        const unsigned long long u = ent[a], v = ent[b];
        if ((u < v) == ((a & k) == 0)) ent[a] = v, ent[b] = u;
      }
      __syncthreads();
    }

  // ---- thresholds: thread t owns E consecutive sorted entries; prefix sums of pixels and positives in integers
  const int m = cnt[4];
  const int E = (npad + SEGTAB_THREADS - 1) / SEGTAB_THREADS;
  const int k0 = tid * E < m ? tid * E : m, k1 = k0 + E < m ? k0 + E : m;
  uint32_t sum_n = 0, sum_p = 0, last_end = 0;      // last_end: positives up to the thread's last threshold (relative)
  bool has_end = false;
  for (int k = k0; k < k1; ++k) {
    const unsigned long long e = ent[k];
    const uint32_t cell = ((uint32_t)e) >> 1, t = tot[cell], p = pos[cell];
    sum_n += t, sum_p += (e & 1) ? p : t - p;
    if (k == m - 1 || (uint32_t)(ent[k + 1] >> 32) != (uint32_t)(e >> 32)) has_end = true, last_end = sum_p;
  }
  const uint32_t ex_n = segtab_scan_excl<false>(sum_n, wsum);
  const uint32_t ex_p = segtab_scan_excl<false>(sum_p, wsum);
  // positives at the last threshold before the thread's entries: the running counts never fall, so a max scan finds it
  uint32_t prev = segtab_scan_excl<true>(has_end ? ex_p + last_end : 0u, wsum);
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
    for (int i = 0; i < SEGTAB_WAVES; ++i) ap += dsum[i];
    SegtabRecord r;
    r.n11 = cnt[0], r.n10 = cnt[1], r.n01 = cnt[2], r.n00 = cnt[3];
    r.ap = ap;
    r.mean = mean, r.lo = lo, r.hi = hi;
    r.thresholds = cnt[5];
    ((SegtabRecord *)A.records)[blockIdx.x] = r;
  }
}

extern "C" int ca_segtab_score(const float *maps, int64_t map_stride, int32_t n_maps, const void *label, void *records,
                               void *cells, int32_t h, int32_t w, int32_t Hl, int32_t Wl, int32_t flags,
                               const float *blur_weights, ca_stream_t stream) {
  const char *FN = "ca_segtab_score";
  if (h < 1 || w < 1 || (int64_t)h * w > SEGTAB_MAX_CELLS) {
    ca_set_error("%s: map %d x %d: h * w must be in 1..%d (larger maps are scored on the host)", FN, h, w, SEGTAB_MAX_CELLS);
    return CA_ERR_ARG;
  }
  if (Hl < 1 || Wl < 1 || (int64_t)Hl * Wl > ((int64_t)1 << 24)) {
    ca_set_error("%s: label %d x %d: Hl * Wl must be in 1..2^24", FN, Hl, Wl);
    return CA_ERR_ARG;
  }
  if (n_maps < 1 || n_maps > CA_SEGTAB_MAX_MAPS) {
    ca_set_error("%s: n_maps=%d outside 1..%d", FN, n_maps, CA_SEGTAB_MAX_MAPS);
    return CA_ERR_ARG;
  }
  if (map_stride < (int64_t)h * w) {
    ca_set_error("%s: map_stride=%lld below h * w = %d", FN, (long long)map_stride, h * w);
    return CA_ERR_ARG;
  }
  if (!maps || !label || !records || !cells || ((uintptr_t)maps & 3) || ((uintptr_t)records & 7) || ((uintptr_t)cells & 15)) {
    ca_set_error("%s: maps, label, records and cells non-null; maps 4-byte, records 8-byte, cells 16-byte aligned", FN);
    return CA_ERR_ARG;
  }
  if (flags & ~(CA_SEGTAB_MEAN_THRESHOLD | CA_SEGTAB_DOWNSCALE | CA_SEGTAB_BLUR | CA_SEGTAB_RAW)) {
    ca_set_error("%s: flags=%d has bits outside CA_SEGTAB_MEAN_THRESHOLD | CA_SEGTAB_DOWNSCALE | CA_SEGTAB_BLUR | "
                 "CA_SEGTAB_RAW (1 | 2 | 4 | 8)", FN, flags);
    return CA_ERR_ARG;
  }
  if ((flags & CA_SEGTAB_BLUR) && (h < 2 || w < 2 || !blur_weights)) {
    ca_set_error("%s: the blur's reflect padding needs h >= 2 and w >= 2 (map %d x %d) and nine blur_weights", FN, h, w);
    return CA_ERR_ARG;
  }
  SegtabLaunch A = {};
  const int hw = h * w, hw4 = (hw + 3) & ~3;
  int npad = 2;
  while (npad < 2 * hw) npad <<= 1;
  A.maps = maps, A.label = (const uint8_t *)label, A.records = records, A.cells = (uint32_t *)cells;
  A.map_stride = map_stride;
  A.h = h, A.w = w, A.Hl = Hl, A.Wl = Wl, A.flags = flags, A.npad = npad;
  A.sy = (float)h / (float)Hl, A.sx = (float)w / (float)Wl;
  A.sy14 = 14.0f / (float)Hl, A.sx14 = 14.0f / (float)Wl;
  A.s14y = (float)h / 14.0f, A.s14x = (float)w / 14.0f;
  if (flags & CA_SEGTAB_BLUR)
    for (int i = 0; i < 9; ++i) A.blur[i] = blur_weights[i];
  const size_t lds = (size_t)npad * 8 + (size_t)hw4 * 12 + SEGTAB_SCRATCH_BYTES;
  if (lds > 64 * 1024) {   // above 2048 cells (npad 8192: 57 856 -> 90 672 bytes): above the default dynamic LDS limit
    static std::atomic<unsigned long long> attr_done{0};
    const int rc = ca_raise_lds_limit({(const void *)ca_segtab_map_kernel},
                                      SEGTAB_MAX_CELLS * 2 * 8 + SEGTAB_MAX_CELLS * 12 + SEGTAB_SCRATCH_BYTES, attr_done, FN);
    if (rc != CA_OK) return rc;
  }
  const int nz = 4 * hw4;
  hipLaunchKernelGGL(ca_segtab_zero_kernel, dim3((unsigned)((nz + SEGTAB_LABEL_THREADS - 1) / SEGTAB_LABEL_THREADS)),
                     dim3(SEGTAB_LABEL_THREADS), 0, (hipStream_t)stream, A.cells, nz);
  int rc = ca_check_launch(FN);
  if (rc != CA_OK) return rc;
  hipLaunchKernelGGL(ca_segtab_label_kernel, dim3((unsigned)(Hl < SEGTAB_ROWS_MAX ? Hl : SEGTAB_ROWS_MAX)),
                     dim3(SEGTAB_LABEL_THREADS), (size_t)w * 16, (hipStream_t)stream, A);   // (w <= 4096: at most 64 KiB)
  rc = ca_check_launch(FN);
  if (rc != CA_OK) return rc;
  hipLaunchKernelGGL(ca_segtab_map_kernel, dim3((unsigned)n_maps), dim3(SEGTAB_THREADS), lds, (hipStream_t)stream, A);
  return ca_check_launch(FN);
}
