// ca_query_maps: query-row attention maps.  For each of a few query rows (text tokens or concept tokens), the probability
// its softmax over the keys [k0 | k1] gives to every one of the n1 emitted keys, averaged over the heads (semantics:
// ca_querymap.h).  The transpose of ca_token_maps' problem: at most 512 query rows against thousands of emitted keys, so
// the [nq, n1] output cannot live in LDS and the grid tiles the emitted keys as well as the query rows.  It re-reads the q
// and k rows an attention launch has read; the fragments, the key rows, the score step, the accumulators' write-out and the
// common entry rules are ca_qkmap_core.h's, shared with ca_tokmap.hip; nothing is shared with the attention kernels.
//
// Two launches, one stream, no atomics; every output cell and every workspace cell has exactly one writer.
//
// 1. statistics (qm_stats_kernel): one workgroup of four waves per (problem, block of 16 query rows, head).  S^T = K Q^T
//    on v_mfma_f32_16x16x32, the key on the accumulator's row and the query on its column.  Wave w of the workgroup takes
//    keys 64 t + 16 w + 0..15 of every key tile t = 0, 1, ..; lane group g = lane >> 4 holds keys 4 g + 0..3 of those 16 for
//    query lane & 15.  So the 16 "lane chains" (w, g) of a query row partition the keys by (j mod 64) / 4, and which chain
//    a key belongs to depends on its index j alone.  The summation order, per head and query row:
//      per chain, t ascending:   m' = max(m, the chain's four scores of tile t)                (m starts at -3e38)
//                                l  = l * exp2(m - m') + (((e0 + e1) + e2) + e3),  e = exp2(s - m');   m = m'
//                                (keys past the end are -inf: e = 0)
//      M = max over the 16 chains;  every chain:  l = l * exp2(m - M)
//      per wave  L_w = (l_g0 + l_g1) + (l_g2 + l_g3);     L = (L_0 + L_1) + (L_2 + L_3)
//    (M, L) go to the workspace ([head][row] pairs of floats per problem), lse = (M + log2 L) ln 2 to P.lse.
// 2. emit (qm_emit_kernel): one workgroup of four waves per (problem, block of 16 query rows, block of 128 emitted keys);
//    a wave owns 16 rows x 32 keys, a lane 1 row x 8 keys.  It walks the heads in order: p = exp2(s - M) / L on the MFMA
//    accumulators (s is the same instruction over the same operands as in pass 1), sum = 0 + p for head 0, sum = sum + p after;
//    then map = sum * (1 / num_heads) and ONE read-modify-write of the lane's own cells,  acc = fma(weight, map, acc).
// Neither pass depends on the grid or on the other problems: a cell's bits are a function of its own q row, the key rows
// and (through the chain a key falls into) the key indices only.
//
// The fragments come straight from global memory (16 bytes per lane, the 256 bytes of a head's row are consumed by the four
// lanes that share the row); the next tile's / head's loads are issued before the current MFMAs.  No LDS tiles.
// Resources (hipcc, gfx950, both storage types alike): statistics 64 VGPRs, 0 scratch, 512 bytes of LDS (the two
// cross-wave reductions); emit 128 VGPRs, 0 scratch, no LDS.  build.py's audit refuses a spill.
#include "ca_qkmap_core.h"
#include "ca_querymap.h"

namespace {   // device code

constexpr int QM_THREADS = 256;
constexpr int QM_ROWS = 16;                 // query rows of a workgroup
constexpr int QM_TILE = 64;                 // statistics: keys of a tile (16 per wave)
constexpr int QM_EMIT_KEYS = 128;           // emit: keys of a workgroup (32 per wave)
constexpr float QM_M_INIT = -3.0e38f;       // a finite "no key yet": exp2(-inf - QM_M_INIT) is 0, not NaN

struct QuerymapLaunch {
  ca_querymap_problem p[CA_QUERYMAP_MAX_PROBLEMS];
  int64_t ws_off[CA_QUERYMAP_MAX_PROBLEMS];   // bytes from workspace to the problem's [num_heads][nq] (M, L) pairs
  char *workspace;
  int32_t num_heads;
  float scale_log2, inv_heads;
};

template <bool F16>
__global__ __launch_bounds__(QM_THREADS) void qm_stats_kernel(QuerymapLaunch A) {
  __shared__ float red[2][4][QM_ROWS];
  const ca_querymap_problem &P = A.p[blockIdx.z];
  const int row0 = blockIdx.y * QM_ROWS;
  if (row0 >= P.nq) return;   // (the grid is sized for the launch's largest problem; whole workgroups leave together)
  const int h = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntot = P.n0 + P.n1, tiles = (ntot + QM_TILE - 1) / QM_TILE;
  const int qi = row0 + (lane & 15);                       // this lane's query row
  const int qrow = min(qi, P.nq - 1);                      // (rows past the end repeat the last one and are dropped)
  u32x4 qf[4], kf[4], kn[4];
  qk_frag_load((const uint16_t *)P.q + (size_t)qrow * (size_t)P.ldq, h, qf);
  // (key rows past the end repeat the last key; their scores are masked)
  qk_frag_load(qk_key_row(P, min(wave * 16 + (lane & 15), ntot - 1)), h, kn);
  float m = QM_M_INIT, l = 0.f;
  for (int t = 0; t < tiles; ++t) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) kf[ks] = kn[ks];
    if (t + 1 < tiles) qk_frag_load(qk_key_row(P, min((t + 1) * QM_TILE + wave * 16 + (lane & 15), ntot - 1)), h, kn);
    f32x4 s = qk_scores<F16>(kf, qf, A.scale_log2);
    if (t == tiles - 1) {                                  // keys past the end (the last tile only)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (t * QM_TILE + wave * 16 + (lane >> 4) * 4 + e >= ntot) s[e] = -INFINITY;
    }
    const float m_new = fmaxf(fmaxf(m, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
    float sum = __builtin_amdgcn_exp2f(s[0] - m_new);
#pragma unroll
    for (int e = 1; e < 4; ++e) sum += __builtin_amdgcn_exp2f(s[e] - m_new);
    l = l * __builtin_amdgcn_exp2f(m - m_new) + sum;
    m = m_new;
  }
  float wm = fmaxf(m, __shfl_xor(m, 16));
  wm = fmaxf(wm, __shfl_xor(wm, 32));
  if (lane < QM_ROWS) red[0][wave][lane] = wm;
  __syncthreads();
  const int c = lane & 15;
  const float M = fmaxf(fmaxf(red[0][0][c], red[0][1][c]), fmaxf(red[0][2][c], red[0][3][c]));   // (finite: key 0 exists)
  l = l * __builtin_amdgcn_exp2f(m - M);
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (lane < QM_ROWS) red[1][wave][lane] = l;
  __syncthreads();
  if (wave == 0 && lane < QM_ROWS && qi < P.nq) {
    const float Ls = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
    const size_t cell = (size_t)h * (size_t)P.nq + qi;
    float *st = (float *)(A.workspace + A.ws_off[blockIdx.z]) + cell * 2;
    st[0] = M, st[1] = Ls;
    if (P.lse) P.lse[cell] = (M + __builtin_amdgcn_logf(Ls)) * 0.69314718055994531f;
  }
}

template <bool F16>
__global__ __launch_bounds__(QM_THREADS) void qm_emit_kernel(QuerymapLaunch A) {
  const ca_querymap_problem &P = A.p[blockIdx.z];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.y * QM_ROWS;
  // (the grid is sized for the launch's largest problem; no barrier in this kernel, so waves leave on their own.
  // n1 <= 2^31 - 128 keeps blockIdx.x * 128 + 127 below 2^31)
  if (row0 >= P.nq || (int64_t)blockIdx.x * QM_EMIT_KEYS + wave * 32 >= P.n1) return;
  const int key0 = (int)blockIdx.x * QM_EMIT_KEYS + wave * 32;
  const int qi = row0 + (lane & 15);
  const int qrow = min(qi, P.nq - 1);                      // (rows past the end repeat the last one and are dropped)
  const uint16_t *qp = (const uint16_t *)P.q + (size_t)qrow * (size_t)P.ldq;
  const uint16_t *kp[2];
#pragma unroll
  for (int g = 0; g < 2; ++g)                              // (keys past the end repeat the last one and are dropped)
    kp[g] = (const uint16_t *)P.k1 + (size_t)min(key0 + g * 16 + (lane & 15), P.n1 - 1) * (size_t)P.ldk;
  const float2 *stat = (const float2 *)(A.workspace + A.ws_off[blockIdx.z]) + qrow;
  u32x4 qf[4], qn[4], kf[2][4], kn[2][4];
  qk_frag_load(qp, 0, qn);
  qk_frag_load(kp[0], 0, kn[0]);
  qk_frag_load(kp[1], 0, kn[1]);
  float2 mn = stat[0];
  f32x4 sum[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // (0 + p is p: head 0 starts the sum)
  for (int h = 0; h < A.num_heads; ++h) {
    const float2 ml = mn;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks], kf[0][ks] = kn[0][ks], kf[1][ks] = kn[1][ks];
    if (h + 1 < A.num_heads) {                             // the next head, in flight during this head's MFMAs
      qk_frag_load(qp, h + 1, qn);
      qk_frag_load(kp[0], h + 1, kn[0]);
      qk_frag_load(kp[1], h + 1, kn[1]);
      mn = stat[(size_t)(h + 1) * (size_t)P.nq];
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const f32x4 s = qk_scores<F16>(kf[g], qf, A.scale_log2);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = __builtin_amdgcn_exp2f(s[e] - ml.x) / ml.y;
        sum[g][e] += p;
      }
    }
  }
  if (qi >= P.nq) return;
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = key0 + g * 16 + (lane >> 4) * 4 + e;
      if (j >= P.n1) continue;
      qk_accumulate(P, (size_t)qi * (size_t)P.n1 + j, sum[g][e] * A.inv_heads);
    }
}

int64_t qm_problem_bytes(const ca_querymap_problem &p, int32_t num_heads) {
  return ((int64_t)num_heads * p.nq * 8 + 15) & ~(int64_t)15;
}

// the unit's size rule (n0 + n1 leaves room for the round-up to whole key tiles / key blocks in 32-bit arithmetic)
bool qm_sizes_ok(const char *FN, int i, const ca_querymap_problem &p) {
  if (p.nq >= 1 && p.nq <= CA_QUERYMAP_MAX_QUERIES && p.n0 >= 0 && p.n1 >= 1 && (int64_t)p.n0 + p.n1 <= CA_QUERYMAP_MAX_ROWS)
    return true;
  ca_set_error("%s: problem %d sizes invalid (nq=%d n0=%d n1=%d; need 1 <= nq <= %d, n0 >= 0, n1 >= 1, n0 + n1 <= %d)",
               FN, i, p.nq, p.n0, p.n1, CA_QUERYMAP_MAX_QUERIES, CA_QUERYMAP_MAX_ROWS);
  return false;
}

// the argument rules of both entry points; 0 or CA_ERR_ARG with the text under FN
int qm_check(const char *FN, const ca_querymap_problem *problems, int32_t n_problems, int32_t num_heads) {
  return qk_check(FN, problems, n_problems, num_heads, CA_QUERYMAP_MAX_PROBLEMS, true, "q, k1 and, with n0 > 0, k0", qm_sizes_ok);
}

}  // namespace

extern "C" int64_t ca_query_maps_workspace_bytes(const ca_querymap_problem *problems, int32_t n_problems, int32_t num_heads) {
  if (qm_check("ca_query_maps_workspace_bytes", problems, n_problems, num_heads) != CA_OK) return CA_ERR_ARG;
  int64_t need = 0;
  for (int i = 0; i < n_problems; ++i) need += qm_problem_bytes(problems[i], num_heads);
  return need;
}

extern "C" int ca_query_maps(const ca_querymap_problem *problems, int32_t n_problems, int32_t num_heads, float scale_log2,
                             int32_t flags, void *workspace, int64_t workspace_bytes, ca_stream_t stream) {
  const char *FN = "ca_query_maps";
  if (qm_check(FN, problems, n_problems, num_heads) != CA_OK) return CA_ERR_ARG;
  if (qk_check_scale_flags(FN, scale_log2, flags, CA_QUERYMAP_QK_F16) != CA_OK) return CA_ERR_ARG;
  QuerymapLaunch A = {};
  int64_t need = 0;
  int max_nq = 0, max_n1 = 0;
  for (int i = 0; i < n_problems; ++i) {
    A.p[i] = problems[i];
    A.ws_off[i] = need;
    need += qm_problem_bytes(problems[i], num_heads);
    max_nq = problems[i].nq > max_nq ? problems[i].nq : max_nq;
    max_n1 = problems[i].n1 > max_n1 ? problems[i].n1 : max_n1;
  }
  if (workspace_bytes < need || !workspace || ((uintptr_t)workspace & 15)) {
    ca_set_error("%s: workspace too small (workspace_bytes=%lld, ca_query_maps_workspace_bytes says %lld; non-null and "
                 "16-byte aligned)", FN, (long long)workspace_bytes, (long long)need);
    return CA_ERR_ARG;
  }
  A.workspace = (char *)workspace;
  A.num_heads = num_heads, A.scale_log2 = scale_log2, A.inv_heads = 1.0f / (float)num_heads;
  const bool f16 = (flags & CA_QUERYMAP_QK_F16) != 0;
  const unsigned qblocks = (unsigned)((max_nq + QM_ROWS - 1) / QM_ROWS);
  hipLaunchKernelGGL(f16 ? qm_stats_kernel<true> : qm_stats_kernel<false>, dim3((unsigned)num_heads, qblocks, (unsigned)n_problems),
                     dim3(QM_THREADS), 0, (hipStream_t)stream, A);
  const int rc = ca_check_launch(FN);
  if (rc != CA_OK) return rc;
  const unsigned kblocks = (unsigned)(((int64_t)max_n1 + QM_EMIT_KEYS - 1) / QM_EMIT_KEYS);
  hipLaunchKernelGGL(f16 ? qm_emit_kernel<true> : qm_emit_kernel<false>, dim3(kblocks, qblocks, (unsigned)n_problems),
                     dim3(QM_THREADS), 0, (hipStream_t)stream, A);
  return ca_check_launch(FN);
}
