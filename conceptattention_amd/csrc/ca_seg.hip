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
// numpy.  The unit is compiled with -ffp-contract=off: every operation rounds on its own.
//
// ca_seg_core.h holds the arithmetic this unit shares with ca_segtab.hip and ca_mseg.hip: the nearest rule, the blur, the
// LDS carve and every step of the map pass but the label loop.  What is here is the label loop (per label pixel, with LDS
// atomics) and the optional outputs at map resolution.
#include "ca_seg_core.h"

struct SegLaunch {
  ca_seg_problem p[CA_SEG_MAX_PROBLEMS];
  SegGeom g;
  int32_t flags, npad;
  float blur[9];
};

__global__ __launch_bounds__(SEG_THREADS) void ca_seg_score_kernel(SegLaunch A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char seg_lds[];
  const ca_seg_problem P = A.p[blockIdx.x];
  const SegGeom &G = A.g;
  const int tid = threadIdx.x;
  const int h = G.h, w = G.w, hw = h * w, npad = A.npad;
  const SegLds L = seg_carve(seg_lds, npad, (hw + 3) & ~3);

  // ---- 1. x = the map or its blur; the coefficient's tables start empty
  for (int c = tid; c < hw; c += SEG_THREADS) {
    L.x[c] = seg_load_x(P.map, c, h, w, A.flags & CA_SEG_BLUR, A.blur);
    L.tot[c] = 0, L.pos[c] = 0;
  }
  if (tid < SEG_COUNTERS) L.s->cnt[tid] = 0;
  __syncthreads();

  // ---- 2. mean, lo, hi
  const SegStats S = seg_mean_lo_hi(L, hw);
  const float lo = S.lo, thr = (A.flags & CA_SEG_MEAN_THRESHOLD) ? S.mean : 0.0f;
  const float range = S.hi - lo;

  // ---- 3 / 4. the optional outputs at map resolution
  if (P.mask_out || P.coeff_out)
    for (int c = tid; c < hw; c += SEG_THREADS) {
      const float v = L.x[c];
      if (P.mask_out) ((uint8_t *)P.mask_out)[(long)c] = v > thr ? 1 : 0;
      if (P.coeff_out) P.coeff_out[(long)c] = __fdiv_rn(v - lo, range);
    }

  // ---- 5. every label pixel: the confusion counts and the two tables of its coefficient cell
  {
    const uint8_t *label = (const uint8_t *)P.label;
    const long N = (long)G.Hl * G.Wl;
    const bool down = A.flags & CA_SEG_DOWNSCALE;
    int n11 = 0, n10 = 0, n01 = 0, n00 = 0;
    for (long i = tid; i < N; i += SEG_THREADS) {
      const int Y = (int)(i / G.Wl), X = (int)(i - (long)Y * G.Wl);
      const int my = seg_mask_row(G, Y), mx = seg_mask_col(G, X);
      int cy = my, cx = mx;
      if (down) cy = seg_coeff_row(G, Y), cx = seg_coeff_col(G, X);
      const bool m = L.x[my * w + mx] > thr;
      const bool l = label[i] != 0;
      n11 += m & l, n10 += m & !l, n01 += !m & l, n00 += !m & !l;
      const int cell = cy * w + cx;
      atomicAdd(&L.tot[cell], 1u);
      if (l) atomicAdd(&L.pos[cell], 1u);
    }
    seg_add_confusion(L, n11, n10, n01, n00);
  }
  __syncthreads();

  // ---- 6. the entries, their sort, the thresholds, the record
  seg_build_entries(L, hw, npad, lo, range, false);
  seg_sort_entries(L.ent, npad);
  const SegWalk W = seg_walk_thresholds(L, npad, (double)((long)G.Hl * G.Wl));
  if (tid == 0) seg_write_record(P.result, L, S, W);
}

extern "C" int ca_seg_score(const ca_seg_problem *problems, int32_t n_problems, int32_t h, int32_t w, int32_t Hl, int32_t Wl,
                            int32_t flags, const float *blur_weights, ca_stream_t stream) {
  const char *FN = "ca_seg_score";
  if (!problems || n_problems < 1 || n_problems > CA_SEG_MAX_PROBLEMS) {
    ca_set_error("%s: n_problems=%d outside 1..%d, or problems is null", FN, n_problems, CA_SEG_MAX_PROBLEMS);
    return CA_ERR_ARG;
  }
  if (!seg_check_geometry(FN, "map", h, w, SEG_MAX_CELLS, Hl, Wl)) return CA_ERR_ARG;
  if (flags & ~(CA_SEG_MEAN_THRESHOLD | CA_SEG_DOWNSCALE | CA_SEG_BLUR)) {
    ca_set_error("%s: flags=%d has bits outside CA_SEG_MEAN_THRESHOLD | CA_SEG_DOWNSCALE | CA_SEG_BLUR", FN, flags);
    return CA_ERR_ARG;
  }
  if (!seg_check_blur(FN, "map", flags, h, w, blur_weights)) return CA_ERR_ARG;
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
  A.g = seg_fill_geom(h, w, Hl, Wl), A.flags = flags, A.npad = seg_npad(h * w);
  seg_fill_blur(A.blur, flags, blur_weights);
  const size_t lds = seg_lds_bytes(h * w, A.npad);
  static std::atomic<unsigned long long> attr_done{0};
  const int rc = seg_raise_lds_limit((const void *)ca_seg_score_kernel, lds, attr_done, FN);
  if (rc != CA_OK) return rc;
  hipLaunchKernelGGL(ca_seg_score_kernel, dim3((unsigned)n_problems), dim3(SEG_THREADS), lds, (hipStream_t)stream, A);
  return ca_check_launch(FN);
}
