// ca_token_maps: prompt-token attention maps.  For every image query row, the probability its joint [text | image] softmax
// gives to each of the first n_tok text keys, averaged over the heads (semantics: ca_tokmap.h).  It re-reads the q
// and k rows an attention launch has read; the fragments, the key rows, the accumulators' write-out and the common entry
// rules are ca_qkmap_core.h's, shared with ca_querymap.hip; nothing is shared with the attention kernels.
//
// One workgroup of four waves owns 64 query rows (16 per wave) of one problem and walks ALL heads, so that the sum over
// the heads stays inside the workgroup: every (token, row) cell lives in LDS, is added to by one lane only, in head
// order, and is written out once.  No atomics, no workspace, and nothing depends on the grid or on the other problems.
// Per head:
//   pass A  all key tiles (64 rows x 128, through LDS, shared by the four waves): S^T = K Q^T on v_mfma_f32_16x16x32, the
//           key on the accumulator's row and the query on its column, so a lane holds 4 keys x 1 query per MFMA group and
//           the online (m, l) of that query is lane-local; m is made common to the four lane groups of a query per tile
//           (two shuffles), l is summed across them once at the end of the pass.
//   pass B  the text tiles again (ceil(n_tok / 64) of them): exp2(s - m) / l into the LDS cells.
// The next tile's global loads are issued before the current tile's MFMAs (registers -> LDS at the top of the next round).
#include "ca_qkmap_core.h"
#include "ca_tokmap.h"

namespace {   // device code

constexpr int TM_THREADS = 256;
constexpr int TM_ROWS = 64;                 // query rows of a workgroup
constexpr int TM_TILE = 64;                 // key rows of a tile
constexpr int TM_PITCH = 272;               // bytes of a tile row in LDS: 256 + 16, so that the 16 rows of a fragment read
                                            // (ds_read_b128, one row per lane) start 4 banks apart
constexpr int TM_TILE_BYTES = TM_TILE * TM_PITCH;

struct TokmapLaunch {
  ca_tokmap_problem p[CA_TOKMAP_MAX_PROBLEMS];
  int32_t num_heads;
  float scale_log2, inv_heads;
};

// a thread's four 16-byte pieces of key tile `tile`, head h: piece i = tile row (tid >> 4) + 16 i, columns 8 (tid & 15)..;
// rows past the last key repeat the last key (their scores are masked)
__device__ __forceinline__ void tm_tile_load(const ca_tokmap_problem &P, int ntot, int tile, int h, u32x4 (&st)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = min(tile * TM_TILE + (int)(threadIdx.x >> 4) + 16 * i, ntot - 1);
    st[i] = *(const u32x4 *)(qk_key_row(P, j) + (size_t)h * 128 + (threadIdx.x & 15) * 8);
  }
}

__device__ __forceinline__ void tm_tile_store(char *tile_lds, const u32x4 (&st)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *(u32x4 *)(tile_lds + ((threadIdx.x >> 4) + 16 * i) * TM_PITCH + (threadIdx.x & 15) * 16) = st[i];
}

// the scores of key group g (16 keys) of the tile in LDS against the wave's 16 queries: lane l gets keys
// 16 g + 4 (l >> 4) + 0..3 of query l & 15, times scale_log2
template <bool F16>
__device__ __forceinline__ f32x4 tm_scores(const char *tile_lds, int g, const u32x4 (&qf)[4], float scale_log2) {
  const int lane = threadIdx.x & 63;
  const char *row = tile_lds + (g * 16 + (lane & 15)) * TM_PITCH + (lane >> 4) * 16;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) s = qk_mfma<F16>(*(const u32x4 *)(row + ks * 64), qf[ks], s);
  return s * scale_log2;
}

template <bool F16>
__global__ __launch_bounds__(TM_THREADS) void ca_tokmap_kernel(TokmapLaunch A) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const ca_tokmap_problem &P = A.p[blockIdx.y];
  const int row0 = blockIdx.x * TM_ROWS;
  if (row0 >= P.nq) return;   // (the grid is sized for the launch's largest problem; whole workgroups leave together)
  char *tile_lds = smem_raw;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntot = P.n0 + P.n1;
  const int nA = (ntot + TM_TILE - 1) / TM_TILE, nB = (P.n_tok + TM_TILE - 1) / TM_TILE;
  const int ngroups = (P.n_tok + 15) / 16;                 // 16-token groups that hold a cell
  // the wave's cells: [token group][token & 3][(token >> 2) & 3][query & 15]: a lane's four stores of a group go to four
  // runs of 64 consecutive floats, one float per lane
  float *cells = (float *)(smem_raw + TM_TILE_BYTES) + (size_t)wave * ngroups * 256;
  float *mine = cells + (lane >> 4) * 16 + (lane & 15);
  const int qi = row0 + wave * 16 + (lane & 15);           // this lane's query row
  const int qrow = min(qi, P.nq - 1);                      // (rows past the end repeat the last one and are dropped)

  const int per_head = nA + nB, rounds = A.num_heads * per_head;
  u32x4 st[4], qf[4], qn[4];
  // (the row's address is formed at each load: kept in a variable it changes hipcc's code for the whole kernel)
  qk_frag_load((const uint16_t *)P.q + (size_t)qrow * (size_t)P.ldq, 0, qn);
  tm_tile_load(P, ntot, 0, 0, st);
  float m = -INFINITY, l = 0.f;
  int h = 0, r = 0;                                        // round -> (head, tile job of the head)
  for (int round = 0; round < rounds; ++round) {
    __syncthreads();                                       // (the previous tile's readers are done)
    tm_tile_store(tile_lds, st);
    __syncthreads();
    if (r == 0) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
      if (h + 1 < A.num_heads) qk_frag_load((const uint16_t *)P.q + (size_t)qrow * (size_t)P.ldq, h + 1, qn);
      m = -INFINITY, l = 0.f;
    }
    {                                                      // the next round's tile, in flight during this round's MFMAs
      int r1 = r + 1, h1 = h;
      if (r1 == per_head) r1 = 0, ++h1;
      if (h1 < A.num_heads) tm_tile_load(P, ntot, r1 < nA ? r1 : r1 - nA, h1, st);
    }
    if (r < nA) {   // ---- pass A: the online maximum and sum of this lane's keys
      f32x4 s[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) s[g] = tm_scores<F16>(tile_lds, g, qf, A.scale_log2);
      if (r == nA - 1) {                                   // keys past the end (the last tile only)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (r * TM_TILE + g * 16 + (lane >> 4) * 4 + e >= ntot) s[g][e] = -INFINITY;
      }
      float tmax = -INFINITY;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) tmax = fmaxf(tmax, s[g][e]);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      const float m_new = fmaxf(m, tmax);                  // (finite from the first tile on: key 0 is in it)
      float sum = 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum += __builtin_amdgcn_exp2f(s[g][e] - m_new);
      l = l * __builtin_amdgcn_exp2f(m - m_new) + sum;
      m = m_new;
      if (r == nA - 1) {                                   // the query's sum: its four lane groups, the same order in each
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        if (P.lse && lane < 16 && qi < P.nq)
          P.lse[(size_t)h * (size_t)P.nq + qi] = (m + __builtin_amdgcn_logf(l)) * 0.69314718055994531f;
      }
    } else {        // ---- pass B: the text cells
      const int tile = r - nA;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int G = tile * 4 + g;
        if (G < ngroups) {
          const f32x4 s = tm_scores<F16>(tile_lds, g, qf, A.scale_log2);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float p = __builtin_amdgcn_exp2f(s[e] - m) / l;
            float *c = mine + (G * 4 + e) * 64;
            *c = h == 0 ? p : *c + p;
          }
        }
      }
    }
    if (++r == per_head) r = 0, ++h;
  }
  __syncthreads();   // all four waves' cells are complete
  const float *all = (const float *)(smem_raw + TM_TILE_BYTES);
  for (int idx = threadIdx.x; idx < P.n_tok * TM_ROWS; idx += TM_THREADS) {
    const int t = idx >> 6, row = idx & 63, i = row0 + row;
    if (i >= P.nq) continue;
    const float v = all[(size_t)(row >> 4) * ngroups * 256 + (((t >> 4) * 4 + (t & 3)) * 4 + ((t >> 2) & 3)) * 16 + (row & 15)] *
                    A.inv_heads;
    qk_accumulate(P, (size_t)t * (size_t)P.nq + i, v);
  }
}

size_t tm_lds_bytes(int n_tok) { return (size_t)TM_TILE_BYTES + (size_t)((n_tok + 15) / 16) * 256 * 4 * sizeof(float); }

// the unit's size rule (nq and n0 + n1 leave room for the round-up to whole row blocks / key tiles in 32-bit arithmetic)
bool tm_sizes_ok(const char *FN, int i, const ca_tokmap_problem &p) {
  if (p.nq >= 1 && p.nq <= CA_TOKMAP_MAX_ROWS && p.n0 >= 1 && p.n0 <= CA_TOKMAP_MAX_TEXT && p.n_tok >= 1 && p.n_tok <= p.n0 &&
      p.n1 >= 0 && (int64_t)p.n0 + p.n1 <= CA_TOKMAP_MAX_ROWS)
    return true;
  ca_set_error("%s: problem %d sizes invalid (nq=%d n0=%d n1=%d n_tok=%d; need 1 <= nq <= %d, 1 <= n_tok <= n0 <= %d, "
               "n1 >= 0, n0 + n1 <= %d)", FN, i, p.nq, p.n0, p.n1, p.n_tok, CA_TOKMAP_MAX_ROWS, CA_TOKMAP_MAX_TEXT,
               CA_TOKMAP_MAX_ROWS);
  return false;
}

// the argument rules of both entry points; 0 or CA_ERR_ARG with the text under FN
int tm_check(const char *FN, const ca_tokmap_problem *problems, int32_t n_problems, int32_t num_heads) {
  return qk_check(FN, problems, n_problems, num_heads, CA_TOKMAP_MAX_PROBLEMS, false, "q, k0 and, with n1 > 0, k1", tm_sizes_ok);
}

}  // namespace

extern "C" int64_t ca_token_maps_workspace_bytes(const ca_tokmap_problem *problems, int32_t n_problems, int32_t num_heads) {
  if (tm_check("ca_token_maps_workspace_bytes", problems, n_problems, num_heads) != CA_OK) return CA_ERR_ARG;
  return 0;   // (the head sum lives in LDS)
}

extern "C" int ca_token_maps(const ca_tokmap_problem *problems, int32_t n_problems, int32_t num_heads, float scale_log2,
                             int32_t flags, void *workspace, int64_t workspace_bytes, ca_stream_t stream) {
  const char *FN = "ca_token_maps";
  if (tm_check(FN, problems, n_problems, num_heads) != CA_OK) return CA_ERR_ARG;
  if (qk_check_scale_flags(FN, scale_log2, flags, CA_TOKMAP_QK_F16) != CA_OK) return CA_ERR_ARG;
  const int64_t need = ca_token_maps_workspace_bytes(problems, n_problems, num_heads);
  if (workspace_bytes < need || (need > 0 && !workspace)) {
    ca_set_error("%s: workspace too small (workspace_bytes=%lld, ca_token_maps_workspace_bytes says %lld)", FN,
                 (long long)workspace_bytes, (long long)need);
    return CA_ERR_ARG;
  }
  TokmapLaunch A = {};
  A.num_heads = num_heads, A.scale_log2 = scale_log2, A.inv_heads = 1.0f / (float)num_heads;
  int max_nq = 0, max_tok = 0;
  for (int i = 0; i < n_problems; ++i) {
    A.p[i] = problems[i];
    max_nq = problems[i].nq > max_nq ? problems[i].nq : max_nq;
    max_tok = problems[i].n_tok > max_tok ? problems[i].n_tok : max_tok;
  }
  const size_t lds = tm_lds_bytes(max_tok);   // (at most 17 KB + 128 KB of gfx950's 160 KB)
  if (lds > 64 * 1024) {
    static std::atomic<unsigned long long> attr_done{0};
    const int rc = ca_raise_lds_limit({(const void *)ca_tokmap_kernel<false>, (const void *)ca_tokmap_kernel<true>},
                                      (int)tm_lds_bytes(CA_TOKMAP_MAX_TEXT), attr_done, FN);
    if (rc != CA_OK) return rc;
  }
  const dim3 grid((unsigned)((max_nq + TM_ROWS - 1) / TM_ROWS), (unsigned)n_problems);
  const auto kernel = (flags & CA_TOKMAP_QK_F16) ? ca_tokmap_kernel<true> : ca_tokmap_kernel<false>;
  hipLaunchKernelGGL(kernel, grid, dim3(TM_THREADS), lds, (hipStream_t)stream, A);
  return ca_check_launch(FN);
}
