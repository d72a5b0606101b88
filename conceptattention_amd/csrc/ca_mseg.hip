// Multi-class scoring of the zero-shot segmentation on the device (experiments/pascal_voc_segmentation of the reference:
// multi_class_segmentation.py:58-79, run_multi_class_seg_experiment.py:25-37 and 194-233): an item's K accumulated maps
// -> the winning concept per map cell (torch.argmax's rule), its class through the item's table, and against a label
// image of class ids the exact counts correct, labelled, inter[nclass], union[nclass].  One workgroup per item.
//
// What makes it cheap: the class map has at most 16384 cells and stays in LDS as bytes; a label pixel then costs one
// nearest index, one LDS byte and, where its (class, label) pair differs from the thread's previous pixel, two integer
// LDS atomics (whose result does not depend on their order).  No floating-point value is ever added up.
//
// The arithmetic is stated in include/conceptattn.h and restated in numpy by tests/mseg_cases.py.  The unit is compiled
// with -ffp-contract=off: the blur's products and sums and the scale product round on their own.  The nearest rule, the
// blur and the host's geometry and blur checks are ca_seg_core.h's, shared with ca_seg.hip and ca_segtab.hip; what is
// here is the argmax and the run-length walk over the label.
//
// LDS (static): class bytes [16384] | inter int32 [256] | union int32 [256] | correct, labelled: 18.0 KB.
#include "ca_seg_core.h"

#define MSEG_THREADS 1024
#define MSEG_PIXELS_PER_THREAD 4     // consecutive label pixels of one thread per round: mostly one (class, label) run

struct MsegLaunch {
  ca_mseg_problem p[CA_MSEG_MAX_PROBLEMS];
  uint8_t class_of[CA_MSEG_MAX_PROBLEMS][CA_MSEG_MAX_CONCEPTS];
  float scale[CA_MSEG_MAX_CONCEPTS];
  float blur[9];
  int32_t K, nclass, ignore_index, flags, has_scale;
  SegGeom g;               // (the class map is read at the mask's cells: h, w, Hl, Wl, sy, sx)
};

__global__ __launch_bounds__(MSEG_THREADS) void ca_mseg_score_kernel(MsegLaunch A) {
  __shared__ uint8_t cls[CA_MSEG_MAX_CELLS];
  __shared__ int32_t inter[CA_MSEG_MAX_CLASSES];
  __shared__ int32_t uni[CA_MSEG_MAX_CLASSES];
  __shared__ int32_t cnt[2];          // correct, labelled
  const int item = blockIdx.x;
  const ca_mseg_problem P = A.p[item];
  const int tid = threadIdx.x, lane = tid & 63;
  const SegGeom &G = A.g;
  const int K = A.K, h = G.h, w = G.w, hw = h * w, nclass = A.nclass;
  const float *maps = P.maps;

  if (tid < CA_MSEG_MAX_CLASSES) inter[tid] = 0, uni[tid] = 0;
  if (tid < 2) cnt[tid] = 0;

  // ---- 1. per cell: x_k = plane k or its 3x3 blur with reflect padding (nine rounded products, summed in row-major
  // order), s_k = scale[k] * x_k, and torch.argmax over k: plane k replaces the running best iff s_k > best, or s_k is
  // NaN and best is not (the first maximum wins, -0.0 == 0.0, the first NaN beats every number)
  for (int c = tid; c < hw; c += MSEG_THREADS) {
    const int y = c / w, xx = c - y * w;
    float best = 0.f;
    int index = 0, klass = 0;
    for (int k = 0; k < K; ++k) {
      const float *map = maps + (long)k * hw;
      float v = (A.flags & CA_MSEG_BLUR) ? seg_blur_tap(map, y, xx, h, w, A.blur) : map[(long)c];
      if (A.has_scale) v = A.scale[k] * v;
      const int ck = A.class_of[item][k];
      const bool take = k == 0 || v > best || (!(v == v) && best == best);
      if (take) best = v, index = k, klass = ck;
    }
    cls[c] = (uint8_t)klass;
    if (P.class_out) ((uint8_t *)P.class_out)[(long)c] = (uint8_t)klass;
    if (P.index_out) ((uint8_t *)P.index_out)[(long)c] = (uint8_t)index;
  }
  __syncthreads();

  // ---- 2. every label pixel that is not ignored: a thread walks MSEG_PIXELS_PER_THREAD consecutive pixels per round
  // and adds a run of equal (class, label) pairs to the tables at once
  {
    const uint8_t *label = (const uint8_t *)P.label;
    const int N = G.Hl * G.Wl, Wl = G.Wl, ignore = A.ignore_index;
    int correct = 0, labelled = 0;
    int run_p = 0, run_l = 0, run_n = 0;
    for (int i0 = tid * MSEG_PIXELS_PER_THREAD; i0 < N; i0 += MSEG_THREADS * MSEG_PIXELS_PER_THREAD) {
      int Y = (int)((unsigned)i0 / (unsigned)Wl), X = i0 - Y * Wl;
      int my = seg_mask_row(G, Y);
      const int n_here = N - i0 < MSEG_PIXELS_PER_THREAD ? N - i0 : MSEG_PIXELS_PER_THREAD;
      for (int u = 0; u < n_here; ++u) {
        const int l = label[(long)i0 + u];
        const int p = cls[my * w + seg_mask_col(G, X)];
        if (++X == Wl) X = 0, ++Y, my = seg_mask_row(G, Y);
        if (l == ignore) continue;
        if (run_n && p == run_p && l == run_l) {
          ++run_n;
          continue;
        }
        if (run_n) {
          labelled += run_n;
          atomicAdd(&uni[run_p], run_n);
          if (run_l == run_p) correct += run_n, atomicAdd(&inter[run_p], run_n);
          else if (run_l < nclass) atomicAdd(&uni[run_l], run_n);
        }
        run_p = p, run_l = l, run_n = 1;
      }
    }
    if (run_n) {
      labelled += run_n;
      atomicAdd(&uni[run_p], run_n);
      if (run_l == run_p) correct += run_n, atomicAdd(&inter[run_p], run_n);
      else if (run_l < nclass) atomicAdd(&uni[run_l], run_n);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) correct += __shfl_xor(correct, off), labelled += __shfl_xor(labelled, off);
    if (lane == 0) atomicAdd(&cnt[0], correct), atomicAdd(&cnt[1], labelled);
  }
  __syncthreads();

  // ---- 3. the counts: correct, labelled, inter[nclass], union[nclass]
  int32_t *out = (int32_t *)P.counts;
  if (tid < 2) out[tid] = cnt[tid];
  if (tid < nclass) out[2 + tid] = inter[tid], out[2 + nclass + tid] = uni[tid];
}

extern "C" int ca_mseg_score(const ca_mseg_problem *problems, int32_t n_problems, int32_t K, int32_t h, int32_t w,
                             int32_t Hl, int32_t Wl, int32_t nclass, int32_t ignore_index, int32_t flags,
                             const void *class_of, const float *scale, const float *blur_weights, ca_stream_t stream) {
  const char *FN = "ca_mseg_score";
  if (!problems || n_problems < 1 || n_problems > CA_MSEG_MAX_PROBLEMS) {
    ca_set_error("%s: n_problems=%d outside 1..%d, or problems is null", FN, n_problems, CA_MSEG_MAX_PROBLEMS);
    return CA_ERR_ARG;
  }
  if (K < 1 || K > CA_MSEG_MAX_CONCEPTS) {
    ca_set_error("%s: K=%d concepts outside 1..%d", FN, K, CA_MSEG_MAX_CONCEPTS);
    return CA_ERR_ARG;
  }
  if (!seg_check_geometry(FN, "maps", h, w, CA_MSEG_MAX_CELLS, Hl, Wl)) return CA_ERR_ARG;
  if (nclass < 1 || nclass > CA_MSEG_MAX_CLASSES) {
    ca_set_error("%s: nclass=%d outside 1..%d", FN, nclass, CA_MSEG_MAX_CLASSES);
    return CA_ERR_ARG;
  }
  if (ignore_index < -1 || ignore_index > 255) {
    ca_set_error("%s: ignore_index=%d outside -1..255 (-1: no label value is ignored)", FN, ignore_index);
    return CA_ERR_ARG;
  }
  if (flags & ~CA_MSEG_BLUR) {
    ca_set_error("%s: flags=%d has bits outside CA_MSEG_BLUR", FN, flags);
    return CA_ERR_ARG;
  }
  if (!seg_check_blur(FN, "maps", flags, h, w, blur_weights)) return CA_ERR_ARG;
  if (!class_of) {
    ca_set_error("%s: class_of is null (uint8 [n_problems][K] on the host, every entry below nclass)", FN);
    return CA_ERR_ARG;
  }
  MsegLaunch A = {};
  for (int i = 0; i < n_problems; ++i) {
    const ca_mseg_problem &p = problems[i];
    if (!p.maps || !p.label || !p.counts || ((uintptr_t)p.maps & 3) || ((uintptr_t)p.counts & 7)) {
      ca_set_error("%s: problem %d invalid (maps, label and counts non-null; maps 4-byte, counts 8-byte aligned)", FN, i);
      return CA_ERR_ARG;
    }
    A.p[i] = p;
    for (int k = 0; k < K; ++k) {
      const int c = ((const uint8_t *)class_of)[(size_t)i * K + k];
      if (c >= nclass) {
        ca_set_error("%s: class_of[%d][%d]=%d must be below nclass=%d", FN, i, k, c, nclass);
        return CA_ERR_ARG;
      }
      A.class_of[i][k] = (uint8_t)c;
    }
  }
  A.K = K, A.nclass = nclass, A.ignore_index = ignore_index, A.flags = flags;
  A.has_scale = scale != nullptr;
  A.g = seg_fill_geom(h, w, Hl, Wl);
  if (scale)
    for (int k = 0; k < K; ++k) A.scale[k] = scale[k];
  seg_fill_blur(A.blur, flags, blur_weights);
  hipLaunchKernelGGL(ca_mseg_score_kernel, dim3((unsigned)n_problems), dim3(MSEG_THREADS), 0, (hipStream_t)stream, A);
  return ca_check_launch(FN);
}
