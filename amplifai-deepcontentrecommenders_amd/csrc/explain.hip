// Explanations of served lists: for every pick of the lists dcue_topk leaves in device
// memory, the songs of the user's history nearest to it -- "because you played X". The definitions are
// include/dcue.h's (dcue_list_explain).
//
//   k_rank_normalize  (rank.hip) the whole candidate table x / max(||x||, 1e-8), zero-padded to DP, into
//                     the workspace: the rows dcue_topk multiplies, bit for bit
//   k_list_explain    one 256-thread workgroup per list. The list goes through in passes of 64 rows (a
//                     list of 128 picks and a history tile do not fit a CU's LDS together at d = 256):
//                     the pass's rows are gathered into LDS once, then the history row of the CSR streams
//                     through a second LDS tile, 64 entries at a time -- each entry range-checked, then
//                     looked up in the mask, before it addresses a row. Scores as k_topk_scores computes
//                     them with the pick as the query and the history song as the candidate:
//                     v_mfma_f32_16x16x4_f32, lane group g owns k = g*DP/4 + j, j ascending -- the bits
//                     of an item-to-item dcue_topk call, whatever the tiling. The 64 x 64 score tile goes
//                     to LDS; thread (row, quarter) scans 16 of the row's columns and keeps its best 8
//                     keys, sorted, in registers across all tiles. After the last tile a row's four
//                     sorted runs are merged by one thread and the first m keys decoded.
// Key = ord(sim) << 32 | ~index (topk.hip's): unsigned order is similarity descending, then index
// ascending, a total order, so a row's result depends on the set of usable history songs alone -- not on
// tile boundaries, the row's offset in hist_idx, or the launch. NaN similarities are never keyed.
#include "dcue_internal.h"
#include "explain.h"

namespace dcue {

static_assert(kExpReasons == DCUE_EXPLAIN_MAX_REASONS, "a thread keeps DCUE_EXPLAIN_MAX_REASONS keys");
static_assert(2 * kExpRows == DCUE_TOPK_MAX_K, "two passes cover the longest list");
static_assert(exp_dp(100) == rank_dp(100) && exp_dp(256) == rank_dp(256), "exp_dp is rank_dp");

struct ExplainArgs {
  const int32_t* idx;  // [n_lists][k]
  const int32_t* count;
  int k, m;
  const int32_t* queries;
  const int64_t* hist_ptr;
  const int32_t* hist_idx;
  long long n_query_rows;
  const uint8_t* mask;
  const float* cn;  // [n_cand][dp] unit rows
  int n_cand, dp;
  int32_t* out_idx;  // [n_lists][k][m]
  float* out_sim;
  int32_t* out_flags;
};

// keeps b descending
__device__ __forceinline__ void exp_insert(unsigned long long (&b)[kExpReasons], unsigned long long key) {
  if (key <= b[kExpReasons - 1]) return;
#pragma unroll
  for (int i = kExpReasons - 1; i >= 0; --i)
    if (key > b[i]) {
      if (i < kExpReasons - 1) b[i + 1] = b[i];
      b[i] = key;
    }
}

// The MFMA loop restates k_topk_scores' (topk.hip) with the list's rows as its queries and the history
// tile as its candidates, and must stay in step with it: a reason's similarity is similar_songs' score.
__global__ __launch_bounds__(256) void k_list_explain(ExplainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dp = a.dp, st = dp + 4, dp4 = dp >> 2;
  float* As = lds;                  // the pass's list rows [64][st]
  float* Bs = As + kExpRows * st;   // the history tile [64][st]
  float* S = Bs + kExpTile * st;    // the score tile [64][65]; then the merge keys [4][8][64]
  unsigned long long* K = reinterpret_cast<unsigned long long*>(S);
  int* hcol = reinterpret_cast<int*>(reinterpret_cast<char*>(S) + exp_score_bytes());  // the tile's candidates, -1: none
  int* lidx = hcol + kExpTile;
  int* misc = lidx + kExpRows;  // [0] bad index, [1] non-finite, [2] the history has a usable entry
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, l16 = lane & 15;
  const int q = blockIdx.x, k = a.k, m = a.m;
  const int32_t* list = a.idx + (size_t)q * k;
  int32_t* oi = a.out_idx + (size_t)q * k * m;
  float* os = a.out_sim + (size_t)q * k * m;
  int c = a.count[q];
  c = c < 0 ? 0 : c > k ? k : c;
  if (tid < 4) misc[tid] = 0;
  __syncthreads();
  // entries at j >= c are never read; every index is range-checked before it addresses anything
  const int u = a.queries[q];
  const bool bad_u = u < 0 || u >= a.n_query_rows;
  if (tid == 0 && bad_u) misc[0] = DCUE_LIST_FLAG_BAD_INDEX;
  if (tid < c) {
    const int v = list[tid];
    if (v < 0 || v >= a.n_cand) atomicOr(&misc[0], DCUE_LIST_FLAG_BAD_INDEX);
  }
  __syncthreads();
  if (misc[0]) {  // (uniform) nothing was gathered: the list is all padding
    for (int e = tid; e < k * m; e += 256) {
      oi[e] = -1;
      os[e] = -__builtin_inff();
    }
    if (tid == 0) a.out_flags[q] = DCUE_LIST_FLAG_BAD_INDEX;
    return;
  }
  const long long hb = a.hist_ptr[u], he = a.hist_ptr[u + 1];
  const int kq = dp >> 2;  // k range per lane group
  bool nonfinite = false;

  for (int p0 = 0; p0 == 0 || p0 < c; p0 += kExpRows) {  // (c == 0: one pass, for the history's flags)
    const int nrows = c - p0 < kExpRows ? c - p0 : kExpRows;
    const int mt = (nrows + 15) >> 4;
    __syncthreads();  // the previous pass's merge
    if (tid < kExpRows) lidx[tid] = tid < nrows ? list[p0 + tid] : -1;
    __syncthreads();
    for (int e = tid; e < 16 * mt * dp4; e += 256) {  // rows nrows .. 16 mt - 1 are zero
      const int r = e / dp4, k4 = e - r * dp4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < nrows) v = ld4(a.cn + (size_t)lidx[r] * dp + 4 * k4);
      st4(&As[r * st + 4 * k4], v);
    }
    unsigned long long best[kExpReasons];
#pragma unroll
    for (int i = 0; i < kExpReasons; ++i) best[i] = 0ull;  // below every real key

    for (long long t0 = hb; t0 < he; t0 += kExpTile) {
      __syncthreads();  // the previous tile's reads of Bs, S and hcol
      if (tid < kExpTile) {
        int col = -1;
        if (t0 + tid < he) {
          const int v = a.hist_idx[t0 + tid];
          if (v < 0 || v >= a.n_cand) {
            atomicOr(&misc[0], DCUE_LIST_FLAG_BAD_INDEX);
          } else if (!a.mask || a.mask[v]) {
            col = v;
            misc[2] = 1;  // (every writer stores the same value)
          }
        }
        hcol[tid] = col;
      }
      __syncthreads();
      if (mt) {
        for (int e = tid; e < kExpTile * dp4; e += 256) {  // rows without a usable entry are zero
          const int r = e / dp4, k4 = e - r * dp4;
          const int v = hcol[r];
          float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
          if (v >= 0) x = ld4(a.cn + (size_t)v * dp + 4 * k4);
          st4(&Bs[r * st + 4 * k4], x);
        }
      }
      __syncthreads();
      if (mt) {
        // wave w owns history columns 16w .. 16w+15 of the tile
        f32x4 acc[4];
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) acc[mm] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* brow = &Bs[(16 * w + l16) * st + g * kq];
        for (int j = 0; j < kq; j += 4) {
          const float4 b = ld4(brow + j);
#pragma unroll
          for (int mm = 0; mm < 4; ++mm)
            if (mm < mt) {
              const float4 x = ld4(&As[(16 * mm + l16) * st + g * kq + j]);
              acc[mm] = mfma4(x.x, b.x, acc[mm]);
              acc[mm] = mfma4(x.y, b.y, acc[mm]);
              acc[mm] = mfma4(x.z, b.z, acc[mm]);
              acc[mm] = mfma4(x.w, b.w, acc[mm]);
            }
        }
        // the lane holds column 16w + l16's scores for list rows 16 mm + 4g + r
#pragma unroll
        for (int mm = 0; mm < 4; ++mm)
          if (mm < mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(16 * mm + 4 * g + r) * kExpPitch + 16 * w + l16] = acc[mm][r];
          }
      }
      __syncthreads();
      // thread (row = lane, quarter = w): 16 columns of its row against its sorted best
      if (lane < nrows) {
#pragma unroll 4
        for (int cc = 0; cc < 16; ++cc) {
          const int col = 16 * w + cc;
          const int v = hcol[col];
          if (v < 0) continue;
          const float s = S[lane * kExpPitch + col] + 0.f;  // -0 -> +0: one key per value
          if (!(fabsf(s) < __builtin_inff())) nonfinite = true;
          if (s == s) exp_insert(best, ((unsigned long long)ord_key(s) << 32) | (unsigned)~(unsigned)v);
        }
      }
    }
    __syncthreads();  // the last tile's reads of S: the merge keys take its place
#pragma unroll
    for (int i = 0; i < kExpReasons; ++i) K[(w * kExpReasons + i) * kExpRows + lane] = best[i];
    __syncthreads();
    if (tid < nrows) {  // (wave 0) the row's four sorted runs -> its best m
      const bool bad = misc[0] != 0;  // a history entry out of range: final after the first pass's scan
#pragma unroll
      for (int i = 0; i < kExpReasons; ++i) best[i] = K[i * kExpRows + tid];
      for (int e = kExpReasons; e < kExpQuarters * kExpReasons; ++e) exp_insert(best, K[e * kExpRows + tid]);
      const size_t o = (size_t)(p0 + tid) * m;
#pragma unroll
      for (int i = 0; i < kExpReasons; ++i)
        if (i < m) {
          const unsigned long long key = bad ? 0ull : best[i];
          oi[o + i] = key ? (int32_t)~(unsigned)key : -1;
          os[o + i] = key ? ord_value((unsigned)(key >> 32)) : -__builtin_inff();
        }
    }
  }
  for (int e = c * m + tid; e < k * m; e += 256) {  // rows j >= c are all padding
    oi[e] = -1;
    os[e] = -__builtin_inff();
  }
  if (nonfinite) atomicOr(&misc[1], DCUE_LIST_FLAG_NONFINITE);
  __syncthreads();
  if (tid == 0)
    a.out_flags[q] = misc[0] ? DCUE_LIST_FLAG_BAD_INDEX : (misc[2] ? 0 : DCUE_EXPLAIN_FLAG_NO_HISTORY) | misc[1];
}

static int explain_check(int64_t n_cand, int32_t d, int32_t n_lists, int32_t k, int32_t m) {
  if (n_lists < 0 || k < 1 || k > DCUE_TOPK_MAX_K || m < 1 || m > DCUE_EXPLAIN_MAX_REASONS || n_cand <= 0 || d <= 0)
    return DCUE_ERR_INVALID;
  if (d > 256 || n_cand > INT32_MAX - 64) return DCUE_ERR_UNSUPPORTED;  // dcue_topk's bounds
  return DCUE_OK;
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_list_explain_workspace_bytes(int64_t n_cand, int32_t d, int32_t n_lists, int32_t k, int32_t m,
                                      size_t* bytes) {
  if (!bytes) return DCUE_ERR_INVALID;
  TRY(explain_check(n_cand, d, n_lists, k, m));
  // the candidate table's unit rows [n_cand][rank_dp(d)] floats (k_rank_normalize's output, as dcue_topk
  // keeps it); the lists' and histories' rows are gathered from it, everything else lives in LDS
  *bytes = (size_t)n_cand * rank_dp(d) * sizeof(float);
  return DCUE_OK;
}

int dcue_list_explain(const int32_t* idx, const int32_t* count, int32_t n_lists, int32_t k, const int32_t* queries,
                      const int64_t* hist_ptr, const int32_t* hist_idx, int64_t n_query_rows,
                      const uint8_t* hist_mask, const float* cand_feat, int64_t n_cand, int32_t d, int32_t m,
                      void* ws, size_t ws_bytes, int32_t* out_idx, float* out_sim, int32_t* out_flags,
                      void* stream) {
  if (!idx || !count || !queries || !hist_ptr || !hist_idx || !cand_feat || !out_idx || !out_sim || !out_flags ||
      n_query_rows <= 0)
    return DCUE_ERR_INVALID;
  TRY(explain_check(n_cand, d, n_lists, k, m));
  size_t need = 0;
  TRY(dcue_list_explain_workspace_bytes(n_cand, d, n_lists, k, m, &need));
  if (need > ws_bytes || !ws) return DCUE_ERR_WORKSPACE;
  if (n_lists == 0) return DCUE_OK;
  hipStream_t s = (hipStream_t)stream;
  static bool attr = false;
  if (!attr) {
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_list_explain, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kExpLdsBudget));
    attr = true;
  }
  const int dp = rank_dp(d);
  float* cn = static_cast<float*>(ws);
  TRY(launch_rank_normalize(cand_feat, nullptr, n_cand, d, dp, cn, s));
  ExplainArgs a;
  a.idx = idx;
  a.count = count;
  a.k = k;
  a.m = m;
  a.queries = queries;
  a.hist_ptr = hist_ptr;
  a.hist_idx = hist_idx;
  a.n_query_rows = n_query_rows;
  a.mask = hist_mask;
  a.cn = cn;
  a.n_cand = (int)n_cand;
  a.dp = dp;
  a.out_idx = out_idx;
  a.out_sim = out_sim;
  a.out_flags = out_flags;
  DCUE_LAUNCH(k_list_explain, dim3((unsigned)n_lists), dim3(256), exp_lds_bytes(d), s, a);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

}  // extern "C"
