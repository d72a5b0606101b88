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
// (score, cell, class) entries and the coefficient tables.
//
// ca_seg_core.h holds the arithmetic per map, the one ca_seg.hip runs (tests/segtab_cases.py holds the numpy statement):
// the nearest rule, the blur, the LDS carve and every step of the map pass.  What is here is the zero and label kernels,
// the sums over the tables, CA_SEGTAB_RAW (the coefficient is the map value itself) and the table's stride.  The unit is
// compiled with -ffp-contract=off.
#include "ca_seg_core.h"

#define SEGTAB_LABEL_THREADS 256
#define SEGTAB_ROWS_MAX 65535      // label rows in gridDim.x at most; a block walks rows blockIdx.x, + gridDim.x, ...

struct SegtabLaunch {
  const float *maps;
  const uint8_t *label;
  void *records;
  uint32_t *cells;         // [4][hw4]: mask tot, mask pos, coefficient tot, coefficient pos
  int64_t map_stride;
  SegGeom g;
  int32_t flags, npad;
  float blur[9];
};

__global__ __launch_bounds__(SEGTAB_LABEL_THREADS) void ca_segtab_zero_kernel(uint32_t *cells, int n) {
  const int i = blockIdx.x * SEGTAB_LABEL_THREADS + threadIdx.x;
  if (i < n) cells[i] = 0u;
}

// ---- the label pass.  A label row reads ONE row of cells under either mapping, so a workgroup counts its row in LDS
// (four tables of w bins) and adds the non-empty bins to the workspace: integer sums, any order gives the same bits.
__global__ __launch_bounds__(SEGTAB_LABEL_THREADS) void ca_segtab_label_kernel(SegtabLaunch A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char segtab_lds[];
  uint32_t *bins = (uint32_t *)segtab_lds;               // [4][w]
  const SegGeom &G = A.g;
  const int tid = threadIdx.x, w = G.w, hw4 = (G.h * w + 3) & ~3;
  const bool down = A.flags & CA_SEGTAB_DOWNSCALE;
  for (int Y = blockIdx.x; Y < G.Hl; Y += gridDim.x) {
    for (int i = tid; i < 4 * w; i += SEGTAB_LABEL_THREADS) bins[i] = 0u;
    __syncthreads();
    const int my = seg_mask_row(G, Y);
    const int cy = down ? seg_coeff_row(G, Y) : my;
    const uint8_t *row = A.label + (long)Y * G.Wl;
    for (int X = tid; X < G.Wl; X += SEGTAB_LABEL_THREADS) {
      const int mx = seg_mask_col(G, X);
      const int cx = down ? seg_coeff_col(G, X) : mx;
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

// ---- the map pass: the label loop of ca_seg.hip is sums over the tables here
__global__ __launch_bounds__(SEG_THREADS) void ca_segtab_map_kernel(SegtabLaunch A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char segtab_lds[];
  const SegGeom &G = A.g;
  const int tid = threadIdx.x;
  const int h = G.h, w = G.w, hw = h * w, hw4 = (hw + 3) & ~3, npad = A.npad;
  const SegLds L = seg_carve(segtab_lds, npad, hw4);
  const float *map = A.maps + (int64_t)blockIdx.x * A.map_stride;
  const uint32_t *mtot = A.cells, *mpos = A.cells + hw4;

  // ---- 1. x = the map or its blur; the coefficient's tables come into LDS
  for (int c = tid; c < hw; c += SEG_THREADS) {
    L.x[c] = seg_load_x(map, c, h, w, A.flags & CA_SEGTAB_BLUR, A.blur);
    L.tot[c] = A.cells[2 * (long)hw4 + c], L.pos[c] = A.cells[3 * (long)hw4 + c];
  }
  if (tid < SEG_COUNTERS) L.s->cnt[tid] = 0;
  __syncthreads();

  // ---- 2. mean, lo, hi
  const SegStats S = seg_mean_lo_hi(L, hw);
  const float thr = (A.flags & CA_SEGTAB_MEAN_THRESHOLD) ? S.mean : 0.0f;

  // ---- 5. the confusion counts: every cell hands its mask bit to the label pixels that read it
  {
    int n11 = 0, n10 = 0, n01 = 0, n00 = 0;
    for (int c = tid; c < hw; c += SEG_THREADS) {
      const int t = (int)mtot[c], p = (int)mpos[c];
      if (L.x[c] > thr) n11 += p, n10 += t - p;
      else n01 += p, n00 += t - p;
    }
    seg_add_confusion(L, n11, n10, n01, n00);
  }

  // ---- 6. the entries, their sort, the thresholds, the record
  seg_build_entries(L, hw, npad, S.lo, S.hi - S.lo, A.flags & CA_SEGTAB_RAW);
  seg_sort_entries(L.ent, npad);
  const SegWalk W = seg_walk_thresholds(L, npad, (double)((long)G.Hl * G.Wl));
  if (tid == 0) seg_write_record((SegRecord *)A.records + blockIdx.x, L, S, W);
}

extern "C" int ca_segtab_score(const float *maps, int64_t map_stride, int32_t n_maps, const void *label, void *records,
                               void *cells, int32_t h, int32_t w, int32_t Hl, int32_t Wl, int32_t flags,
                               const float *blur_weights, ca_stream_t stream) {
  const char *FN = "ca_segtab_score";
  if (!seg_check_geometry(FN, "map", h, w, SEG_MAX_CELLS, Hl, Wl)) return CA_ERR_ARG;
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
  if (!seg_check_blur(FN, "map", flags, h, w, blur_weights)) return CA_ERR_ARG;
  SegtabLaunch A = {};
  A.maps = maps, A.label = (const uint8_t *)label, A.records = records, A.cells = (uint32_t *)cells;
  A.map_stride = map_stride;
  A.g = seg_fill_geom(h, w, Hl, Wl), A.flags = flags, A.npad = seg_npad(h * w);
  seg_fill_blur(A.blur, flags, blur_weights);
  const size_t lds = seg_lds_bytes(h * w, A.npad);
  static std::atomic<unsigned long long> attr_done{0};
  int rc = seg_raise_lds_limit((const void *)ca_segtab_map_kernel, lds, attr_done, FN);
  if (rc != CA_OK) return rc;
  const int nz = 4 * ((h * w + 3) & ~3);
  hipLaunchKernelGGL(ca_segtab_zero_kernel, dim3((unsigned)((nz + SEGTAB_LABEL_THREADS - 1) / SEGTAB_LABEL_THREADS)),
                     dim3(SEGTAB_LABEL_THREADS), 0, (hipStream_t)stream, A.cells, nz);
  rc = ca_check_launch(FN);
  if (rc != CA_OK) return rc;
  hipLaunchKernelGGL(ca_segtab_label_kernel, dim3((unsigned)(Hl < SEGTAB_ROWS_MAX ? Hl : SEGTAB_ROWS_MAX)),
                     dim3(SEGTAB_LABEL_THREADS), (size_t)w * 16, (hipStream_t)stream, A);   // (w <= 4096: at most 64 KiB)
  rc = ca_check_launch(FN);
  if (rc != CA_OK) return rc;
  hipLaunchKernelGGL(ca_segtab_map_kernel, dim3((unsigned)n_maps), dim3(SEG_THREADS), lds, (hipStream_t)stream, A);
  return ca_check_launch(FN);
}
