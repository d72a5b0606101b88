// What the three scoring units (ca_seg.hip, ca_segtab.hip, ca_mseg.hip) share, stated once: the nearest rule and the
// label pixel -> cell mappings, the 3x3 blur, and for the two units that score a map against a binary label the record,
// the LDS carve and the steps of the map pass (load, fixed-tree mean / lo / hi, entries, sort, threshold walk, record),
// with the host's geometry and blur checks and the dynamic-LDS request.  Device functions are __forceinline__ and run in
// the including kernel; nothing here is a kernel or a translation unit of its own.
//
// Every operation rounds on its own (the including units are compiled with -ffp-contract=off), and the ORDER in which a
// thread performs them is part of the contract: the fp64 sum tree, the scan order and the sort network decide the bits of
// `mean` and `ap`.  tests/seg_cases.py and tests/segtab_cases.py hold the same statement in numpy.
#pragma once
#include "ca_common.h"

#define SEG_THREADS 1024
#define SEG_WAVES (SEG_THREADS / CA_WAVE)
#define SEG_MAX_CELLS 4096
#define SEG_SCRATCH_BYTES 512
// one flag test serves the three entries
static_assert(CA_SEGTAB_MEAN_THRESHOLD == CA_SEG_MEAN_THRESHOLD && CA_SEGTAB_DOWNSCALE == CA_SEG_DOWNSCALE &&
              CA_SEGTAB_BLUR == CA_SEG_BLUR && CA_MSEG_BLUR == CA_SEG_BLUR, "the scoring entries share their flag bits");

struct SegGeom {
  int32_t h, w, Hl, Wl;
  float sy, sx;            // (float)h / Hl, (float)w / Wl: the nearest rule's scales, formed on the host
  float sy14, sx14;        // 14.0f / Hl, 14.0f / Wl           (downscale_for_eval: label pixel -> 14 x 14)
  float s14y, s14x;        // (float)h / 14.0f, (float)w / 14.0f (14 x 14 -> map cell)
};

struct SegRecord {          // ca_seg_record of the header, 40 bytes
  int32_t n11, n10, n01, n00;
  double ap;
  float mean, lo, hi;
  int32_t thresholds;
};
static_assert(sizeof(SegRecord) == 40, "ca_seg_record is 40 bytes");

// ---------------------------------------------------------------------------------------------------------- device
// torch's interpolate(mode="nearest") source index (the rule of ca_pixels.hip): the product in fp32
__device__ __forceinline__ int seg_near(int i, float scale, int n_in) {
  const int s = (int)floorf((float)i * scale);
  return s < n_in - 1 ? s : n_in - 1;
}

// label row Y / column X -> the map cell row / column the MASK is read at
__device__ __forceinline__ int seg_mask_row(const SegGeom &G, int Y) { return seg_near(Y, G.sy, G.h); }
__device__ __forceinline__ int seg_mask_col(const SegGeom &G, int X) { return seg_near(X, G.sx, G.w); }
// ... and, under downscale_for_eval, the COEFFICIENT is read at: the round trip through 14 x 14 (otherwise the mask's cell).
// The caller branches on the flag, once for both coordinates where it maps both in one loop.
__device__ __forceinline__ int seg_coeff_row(const SegGeom &G, int Y) { return seg_near(seg_near(Y, G.sy14, 14), G.s14y, G.h); }
__device__ __forceinline__ int seg_coeff_col(const SegGeom &G, int X) { return seg_near(seg_near(X, G.sx14, 14), G.s14x, G.w); }

__device__ __forceinline__ int seg_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// cell (y, x) of the 3x3 blur with reflect padding: nine rounded products, summed in row-major order
__device__ __forceinline__ float seg_blur_tap(const float *map, int y, int x, int h, int w, const float (&blur)[9]) {
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const long o = (long)seg_reflect(y + i - 1, h) * w + seg_reflect(x + j - 1, w);
      const float prod = blur[i * 3 + j] * map[o];
      v = (i | j) ? v + prod : prod;
    }
  return v;
}

// step 1 of a map pass, per cell: x = the map, or its blur
__device__ __forceinline__ float seg_load_x(const float *map, int c, int h, int w, bool blurred, const float (&blur)[9]) {
  if (!blurred) return map[(long)c];
  const int y = c / w;
  return seg_blur_tap(map, y, c - y * w, h, w, blur);
}

// a float as an unsigned key of the same order; -0.0 and NaN were removed before
__device__ __forceinline__ uint32_t seg_ordkey(float s) {
  const uint32_t b = __builtin_bit_cast(uint32_t, s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// np.nan_to_num on fp32, and one zero: NaN -> 0, +-inf -> +-FLT_MAX, -0.0 -> 0.0 (-0.0 == 0.0 is one threshold).
// Only a RAW score reaches the two infinity branches.  A min-max coefficient is (x - lo) / (hi - lo) with
// lo <= x <= hi: x - lo <= hi - lo in fp32 as in the reals (rounding is monotonic), so the quotient lies in [0, 1], or
// is NaN (0 / 0, inf / inf, a NaN cell), and so does 1 - c.  This is reasoned, not measured; the non-finite records of
// tests/golden/scoring_parent_records.npz, written when ca_seg.hip had no such branches, are what confirms it.
__device__ __forceinline__ float seg_clean_score(float s) {
  s = (!(s == s) || s == 0.0f) ? 0.0f : s;          // (three selects: no branch in the entry loop)
  s = s == INFINITY ? 3.402823466e+38f : s;
  return s == -INFINITY ? -3.402823466e+38f : s;
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

// ---- the LDS of a map pass (dynamic, one carve): sort entries u64 [npad] | x fp32 [hw4] | tot u32 [hw4] | pos u32 [hw4]
// | scratch; npad = the power of two >= 2 h w, hw4 = h w rounded up to 4: 112.5 KB at 64 x 64
enum { SEG_N11, SEG_N10, SEG_N01, SEG_N00, SEG_VALID, SEG_NTHR, SEG_COUNTERS };
struct SegScratch {
  double dsum[SEG_WAVES];
  uint32_t wsum[SEG_WAVES];
  float fmin_w[SEG_WAVES], fmax_w[SEG_WAVES];
  int32_t cnt[SEG_COUNTERS];            // the four confusion counts, valid entries, thresholds
};
static_assert(sizeof(SegScratch) <= SEG_SCRATCH_BYTES, "the scratch part of the carve");

struct SegLds {
  unsigned long long *ent;  // [npad]
  float *x;                 // [hw4]
  uint32_t *tot, *pos;      // [hw4] each: per coefficient cell the label pixels that read it, and the positive ones
  SegScratch *s;
};

__device__ __forceinline__ SegLds seg_carve(unsigned char *base, int npad, int hw4) {
  SegLds L;
  L.ent = (unsigned long long *)base;
  L.x = (float *)(base + (size_t)npad * 8);
  L.tot = (uint32_t *)(L.x + hw4);
  L.pos = L.tot + hw4;
  L.s = (SegScratch *)(L.pos + hw4);
  return L;
}

// ---- step 2: lo, hi (order-free) and the fp64 sum over a fixed tree: thread t adds cells t, t + 1024, ... in that
// order, a wave adds its lanes as a butterfly (32, 16, ..., 1), the 16 wave sums are added in wave order
struct SegStats {
  float mean, lo, hi;
};

__device__ __forceinline__ SegStats seg_mean_lo_hi(const SegLds &L, int hw) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float lo = INFINITY, hi = -INFINITY;
  double s = 0.0;
  for (int c = tid; c < hw; c += SEG_THREADS) {
    const float v = L.x[c];
    lo = fminf(lo, v), hi = fmaxf(hi, v);
    s += (double)v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off));
    hi = fmaxf(hi, __shfl_xor(hi, off));
    s += __shfl_xor(s, off);
  }
  if (lane == 0) L.s->dsum[wave] = s, L.s->fmin_w[wave] = lo, L.s->fmax_w[wave] = hi;
  __syncthreads();
  s = 0.0;
  // two rounds of eight partials, in the same order.  Unrolled whole, the compiler reads all 16 doubles and 32 floats
  // ahead and the kernel takes a 65th VGPR: up to 2048 cells (57 856 bytes of LDS) two workgroups of 16 waves share a
  // CU, which needs 8 waves per SIMD, 64 VGPRs at the most
#pragma unroll 8
  for (int i = 0; i < SEG_WAVES; ++i) {
    s += L.s->dsum[i];
    lo = i ? fminf(lo, L.s->fmin_w[i]) : L.s->fmin_w[0];
    hi = i ? fmaxf(hi, L.s->fmax_w[i]) : L.s->fmax_w[0];
  }
  const SegStats S = {(float)(s / (double)hw), lo, hi};
  __syncthreads();          // (dsum is free again)
  return S;
}

// a thread's four confusion counts into cnt[SEG_N11 .. SEG_N00]
__device__ __forceinline__ void seg_add_confusion(const SegLds &L, int n11, int n10, int n01, int n00) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n11 += __shfl_xor(n11, off), n10 += __shfl_xor(n10, off);
    n01 += __shfl_xor(n01, off), n00 += __shfl_xor(n00, off);
  }
  if ((threadIdx.x & 63) == 0)
    atomicAdd(&L.s->cnt[SEG_N11], n11), atomicAdd(&L.s->cnt[SEG_N10], n10), atomicAdd(&L.s->cnt[SEG_N01], n01),
        atomicAdd(&L.s->cnt[SEG_N00], n00);
}

// ---- step 6: the entries.  Class 1 of a cell scores c, class 0 float32(1 - c), both through seg_clean_score; c is the
// min-max coefficient, or with `raw` the cell's value; cells no pixel reads are dropped.
// entry = ordered score key << 32 | cell * 2 + class, 0 = no entry (every real key is above 0)
__device__ __forceinline__ void seg_build_entries(const SegLds &L, int hw, int npad, float lo, float range, bool raw) {
  int valid = 0;
  for (int e = threadIdx.x; e < npad; e += SEG_THREADS) {
    unsigned long long v = 0;
    const int cell = e >> 1;
    if (cell < hw && L.tot[cell] != 0) {
      const float c = raw ? L.x[cell] : __fdiv_rn(L.x[cell] - lo, range);
      const float sc = seg_clean_score((e & 1) ? c : 1.0f - c);
      v = (unsigned long long)seg_ordkey(sc) << 32 | (uint32_t)e;
      ++valid;
    }
    L.ent[e] = v;
  }
  if (valid) atomicAdd(&L.s->cnt[SEG_VALID], valid);
  __syncthreads();
}

// bitonic sort, descending: the entries are distinct, so the order is unique
__device__ __forceinline__ void seg_sort_entries(unsigned long long *ent, int npad) {
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (npad >> 1); i += SEG_THREADS) {
        const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
        const unsigned long long u = ent[a], v = ent[b];
        if ((u < v) == ((a & k) == 0)) ent[a] = v, ent[b] = u;
      }
      __syncthreads();
    }
}

// ---- the thresholds: thread t owns E consecutive sorted entries; prefix sums of pixels and positives in integers, a
// term per threshold in fp64, the terms added over the same tree as the mean.  n_pos: the label's pixels (every pixel
// is a positive of exactly one class).  The result is thread 0's.
struct SegWalk {
  double ap;
  int32_t thresholds;
};

__device__ __forceinline__ SegWalk seg_walk_thresholds(const SegLds &L, int npad, double n_pos) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long *ent = L.ent;
  const uint32_t *tot = L.tot, *pos = L.pos;
  uint32_t *wsum = L.s->wsum;
  const int m = L.s->cnt[SEG_VALID];
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
  if (lane == 0) L.s->dsum[wave] = ap, atomicAdd(&L.s->cnt[SEG_NTHR], nthr);
  __syncthreads();
  SegWalk W = {0.0, 0};
  if (tid == 0) {
    for (int i = 0; i < SEG_WAVES; ++i) W.ap += L.s->dsum[i];
    W.thresholds = L.s->cnt[SEG_NTHR];
  }
  return W;
}

// thread 0, after seg_walk_thresholds
__device__ __forceinline__ void seg_write_record(void *dst, const SegLds &L, const SegStats &S, const SegWalk &W) {
  SegRecord r;
  r.n11 = L.s->cnt[SEG_N11], r.n10 = L.s->cnt[SEG_N10], r.n01 = L.s->cnt[SEG_N01], r.n00 = L.s->cnt[SEG_N00];
  r.ap = W.ap;
  r.mean = S.mean, r.lo = S.lo, r.hi = S.hi;
  r.thresholds = W.thresholds;
  *(SegRecord *)dst = r;
}

// ------------------------------------------------------------------------------------------------------------ host
// `what`: "map" or "maps", the entry's own word in its texts
static bool seg_check_geometry(const char *FN, const char *what, int32_t h, int32_t w, int32_t max_cells, int32_t Hl,
                               int32_t Wl) {
  if (h < 1 || w < 1 || (int64_t)h * w > max_cells) {
    ca_set_error("%s: %s %d x %d: h * w must be in 1..%d (larger maps are scored on the host)", FN, what, h, w, max_cells);
    return false;
  }
  if (Hl < 1 || Wl < 1 || (int64_t)Hl * Wl > ((int64_t)1 << 24)) {
    ca_set_error("%s: label %d x %d: Hl * Wl must be in 1..2^24", FN, Hl, Wl);
    return false;
  }
  return true;
}

static bool seg_check_blur(const char *FN, const char *what, int32_t flags, int32_t h, int32_t w, const float *blur_weights) {
  if ((flags & CA_SEG_BLUR) && (h < 2 || w < 2 || !blur_weights)) {
    ca_set_error("%s: the blur's reflect padding needs h >= 2 and w >= 2 (%s %d x %d) and nine blur_weights", FN, what, h, w);
    return false;
  }
  return true;
}

static void seg_fill_blur(float (&blur)[9], int32_t flags, const float *blur_weights) {
  if (flags & CA_SEG_BLUR)
    for (int i = 0; i < 9; ++i) blur[i] = blur_weights[i];
}

static SegGeom seg_fill_geom(int32_t h, int32_t w, int32_t Hl, int32_t Wl) {
  SegGeom G;
  G.h = h, G.w = w, G.Hl = Hl, G.Wl = Wl;
  G.sy = (float)h / (float)Hl, G.sx = (float)w / (float)Wl;
  G.sy14 = 14.0f / (float)Hl, G.sx14 = 14.0f / (float)Wl;
  G.s14y = (float)h / 14.0f, G.s14x = (float)w / 14.0f;
  return G;
}

// the padded sort size of hw cells: the power of two >= 2 hw
static int seg_npad(int hw) {
  int npad = 2;
  while (npad < 2 * hw) npad <<= 1;
  return npad;
}

// the dynamic LDS of a map pass on hw cells sorted in npad slots: what seg_carve lays out
static size_t seg_lds_bytes(int hw, int npad) {
  return (size_t)npad * 8 + (size_t)((hw + 3) & ~3) * 12 + SEG_SCRATCH_BYTES;
}

// above 2048 cells (npad 8192: 57 856 -> 90 672 bytes) a launch asks for more than the default dynamic LDS limit: raise
// the kernel's limit to what SEG_MAX_CELLS need.  `done`: the call site's own flag word (ca_raise_lds_limit)
static int seg_raise_lds_limit(const void *kernel, size_t lds, std::atomic<unsigned long long> &done, const char *FN) {
  if (lds > 64 * 1024) return ca_raise_lds_limit({kernel}, (int)seg_lds_bytes(SEG_MAX_CELLS, seg_npad(SEG_MAX_CELLS)), done, FN);
  return CA_OK;
}
