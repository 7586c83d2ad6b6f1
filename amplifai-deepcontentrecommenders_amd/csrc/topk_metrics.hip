// Top-K ranking metrics: Precision / Recall / NDCG / MAP / MRR / HitRate at up to
// eight cutoffs for the lists dcue_topk leaves in device memory, against held-out truth rows in
// dcue_topk's exclusion CSR format, plus the exposure counts catalogue coverage is read from. The
// definitions are include/dcue.h's (dcue_topk_metrics); all arithmetic is fp64.
//
//   k_topk_metrics_table  the discounts 1 / log2(j + 2), j < 128, and their prefix sums (the ideal
//                         DCG of min(cutoff, truth size) hits) into one device table, once per call
//   k_topk_metrics        one wave64 per query, four per workgroup, no LDS. Lane l owns list positions
//                         l and l + 64: range check, then both looked up in the query's truth row by
//                         binary searches that advance in step. The hit bits of the wave are two
//                         ballots; every hit count (prefix or up to a cutoff) is a popcount of them.
//                         DCG and the AP numerator are butterfly sums over the wave, whose order is
//                         fixed, so a query's numbers depend on its list and truth row alone. Lanes
//                         0 .. 6m-1 write the query's [m][6] block. Exposure: position j of an
//                         evaluated query adds 1 (integer atomic) to exposure[i][L[j]], i the first
//                         cutoff with j < cutoff_i.
//   k_topk_metrics_mean   ONE workgroup (the ABI carries no workspace for cross-workgroup partials, and
//                         floating-point atomics would make the sum depend on arrival order): thread
//                         (g, column) sums the rows g, g + G, g + 2G, ... of its column in that order,
//                         G = 1024 / 6m row groups; a column's G partials are then added in ascending
//                         g (colmean.h col_means, shared with k_list_ild_mean). The order depends on
//                         n_queries and m only. Then coverage: one pass over
//                         the candidates, integer counts of those whose exposure up to cutoff i is
//                         non-zero and of the mask's non-zero bytes.
#include "dcue_internal.h"
#include "colmean.h"

namespace dcue {

constexpr int kTmPos = DCUE_TOPK_MAX_K;  // list positions: two per lane
constexpr int kTmMeanThreads = kColMeanThreads;
static_assert(kTmPos == 128, "k_topk_metrics gives each lane of a wave64 two list positions");
static_assert(6 * DCUE_TOPK_METRICS_MAX_CUTOFFS <= 64, "one lane per output of a query");

struct TmCutoffs {
  int m;
  int k[DCUE_TOPK_METRICS_MAX_CUTOFFS];
};

// Written by k_topk_metrics_table at the start of every dcue_topk_metrics call, on the call's stream:
// calls on other streams write the same bits.
static __device__ double g_tm_disc[kTmPos];  // 1 / log2(j + 2)
static __device__ double g_tm_idcg[kTmPos];  // sum of g_tm_disc[0..j]

__global__ __launch_bounds__(kTmPos) void k_topk_metrics_table(int n) {
  __shared__ double d[kTmPos];
  const int j = threadIdx.x;
  d[j] = 1.0 / log2((double)(j + 2));
  g_tm_disc[j] = d[j];
  __syncthreads();
  if (j == 0) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
      s += d[i];
      g_tm_idcg[i] = s;
    }
  }
}

// the same bits in every lane: a + b and b + a round alike
__device__ __forceinline__ double tm_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned long long tm_low_mask(int n) {  // bits 0 .. n-1
  return n <= 0 ? 0ull : n >= 64 ? ~0ull : (1ull << n) - 1ull;
}

__global__ __launch_bounds__(256) void k_topk_metrics(const int32_t* __restrict__ idx,
                                                      const int32_t* __restrict__ count, int nq, int k,
                                                      const int32_t* __restrict__ queries,
                                                      const int64_t* __restrict__ truth_ptr,
                                                      const int32_t* __restrict__ truth_idx, int n_rows, int n_cand,
                                                      TmCutoffs cut, double* __restrict__ out,
                                                      int32_t* __restrict__ flags, int32_t* __restrict__ exposure) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;  // (whole waves: no barrier follows)
  const int m6 = 6 * cut.m;
  const int row = queries[q];
  const bool row_ok = row >= 0 && row < n_rows;
  long long tb = 0, te = 0;
  if (row_ok) {
    tb = truth_ptr[row];
    te = truth_ptr[row + 1];
  }
  const long long t = te - tb;
  int c = count[q];
  c = c < 0 ? 0 : c > k ? k : c;
  const int32_t* L = idx + (size_t)q * k;
  // entries at j >= c are never read; an entry is range-checked before it addresses anything
  int v[2];
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = lane + 64 * i;
    v[i] = p < c ? L[p] : -1;
    bad |= p < c && (v[i] < 0 || v[i] >= n_cand);
  }
  const int f = (t <= 0 ? 1 : 0) | ((__ballot(bad) != 0ull || !row_ok) ? 2 : 0);
  if (f) {  // (wave-uniform) left out of every mean and of the exposure counts
    if (lane < m6) out[(size_t)q * m6 + lane] = 0.0;
    if (lane == 0) flags[q] = f;
    return;
  }
  const double d0 = g_tm_disc[lane], d1 = g_tm_disc[lane + 64];

  // membership: the lane's two binary searches advance in step so their loads overlap
  long long lo[2], hi[2];
  bool h[2] = {false, false};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    lo[i] = tb;
    hi[i] = lane + 64 * i < c ? te : tb;
  }
  for (bool more = true; more;) {
    more = false;
    int w[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (lo[i] < hi[i]) w[i] = truth_idx[(lo[i] + hi[i]) >> 1];
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (lo[i] < hi[i]) {
        const long long mid = (lo[i] + hi[i]) >> 1;
        if (w[i] == v[i]) {
          h[i] = true;
          lo[i] = hi[i];
        } else if (w[i] < v[i]) {
          lo[i] = mid + 1;
        } else {
          hi[i] = mid;
        }
        more |= lo[i] < hi[i];
      }
  }
  const unsigned long long m0 = __ballot(h[0]), m1 = __ballot(h[1]);
  const unsigned long long le = (2ull << lane) - 1ull;  // bits 0 .. lane (lane 63: all)
  const int n0 = __popcll(m0);
  const int H0 = __popcll(m0 & le), H1 = n0 + __popcll(m1 & le);  // hits at positions <= the lane's
  const double g0 = h[0] ? d0 : 0.0, g1 = h[1] ? d1 : 0.0;
  const double a0 = h[0] ? (double)H0 / (double)(lane + 1) : 0.0;
  const double a1 = h[1] ? (double)H1 / (double)(lane + 65) : 0.0;
  const int first = m0 ? __ffsll((long long)m0) - 1 : m1 ? 63 + __ffsll((long long)m1) : kTmPos;

  double mine = 0.0;
#pragma unroll
  for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i) {
    if (i < cut.m) {
      const int kap = cut.k[i];
      const int Hk = __popcll(m0 & tm_low_mask(kap)) + __popcll(m1 & tm_low_mask(kap - 64));
      const double dcg = tm_wave_sum((lane < kap ? g0 : 0.0) + (lane + 64 < kap ? g1 : 0.0));
      const double apn = tm_wave_sum((lane < kap ? a0 : 0.0) + (lane + 64 < kap ? a1 : 0.0));
      const int nt = t < (long long)kap ? (int)t : kap;  // 1 .. 128
      const double val[DCUE_TOPK_N_METRICS] = {(double)Hk / (double)kap,
                                               (double)Hk / (double)t,
                                               dcg / g_tm_idcg[nt - 1],
                                               apn / (double)nt,
                                               first < kap ? 1.0 / (double)(first + 1) : 0.0,
                                               Hk > 0 ? 1.0 : 0.0};
#pragma unroll
      for (int s = 0; s < DCUE_TOPK_N_METRICS; ++s)
        if (lane == 6 * i + s) mine = val[s];
    }
  }
  if (lane < m6) out[(size_t)q * m6 + lane] = mine;
  if (lane == 0) flags[q] = 0;

  if (exposure) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = lane + 64 * i;
      int slot = -1;
#pragma unroll
      for (int j = DCUE_TOPK_METRICS_MAX_CUTOFFS - 1; j >= 0; --j)
        if (j < cut.m && p < cut.k[j]) slot = j;  // the first cutoff past p
      if (p < c && slot >= 0) atomicAdd(&exposure[(size_t)slot * n_cand + v[i]], 1);
    }
  }
}

__global__ __launch_bounds__(kTmMeanThreads) void k_topk_metrics_mean(
    const double* __restrict__ metrics, const int32_t* __restrict__ flags, int nq, int m,
    const int32_t* __restrict__ exposure, const uint8_t* __restrict__ mask, int n_cand, double* __restrict__ out_mean,
    double* __restrict__ out_cov, int32_t* __restrict__ out_n) {
  __shared__ double part[kTmMeanThreads];
  __shared__ int cnt[2 + DCUE_TOPK_METRICS_MAX_CUTOFFS];  // evaluated, mask bytes set, covered[i]
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 2 + DCUE_TOPK_METRICS_MAX_CUTOFFS) cnt[tid] = 0;
  __syncthreads();
  col_means(metrics, flags, nq, 6 * m, part, &cnt[0], out_mean, out_n);
  if (!exposure) return;  // (uniform)

  int cov[DCUE_TOPK_METRICS_MAX_CUTOFFS], set = 0;
#pragma unroll
  for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i) cov[i] = 0;
  for (int c = tid; c < n_cand; c += kTmMeanThreads) {
    set += mask ? mask[c] != 0 : 1;
    int seen = 0;
#pragma unroll
    for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i)
      if (i < m) {
        seen |= exposure[(size_t)i * n_cand + c] != 0;
        cov[i] += seen;
      }
  }
  set = wave_sum_int(set);
  if (lane == 0 && set) atomicAdd(&cnt[1], set);
#pragma unroll
  for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i)
    if (i < m) {
      const int v = wave_sum_int(cov[i]);
      if (lane == 0 && v) atomicAdd(&cnt[2 + i], v);
    }
  __syncthreads();
  if (tid < m) out_cov[tid] = cnt[1] > 0 ? (double)cnt[2 + tid] / (double)cnt[1] : 0.0;
}

static int tm_check_common(int32_t n_queries, int32_t n_cutoffs, int64_t n_cand) {
  if (n_queries < 0 || n_cutoffs < 1 || n_cutoffs > DCUE_TOPK_METRICS_MAX_CUTOFFS || n_cand <= 0)
    return DCUE_ERR_INVALID;
  if (n_cand > INT32_MAX - 64) return DCUE_ERR_UNSUPPORTED;  // dcue_topk's bound: indices are int32
  return DCUE_OK;
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_topk_metrics(const int32_t* idx, const int32_t* count, int32_t n_queries, int32_t k, const int32_t* queries,
                      const int64_t* truth_ptr, const int32_t* truth_idx, int64_t n_query_rows, int64_t n_cand,
                      const int32_t* cutoffs_host, int32_t n_cutoffs, double* out_metrics, int32_t* out_flags,
                      int32_t* exposure, void* stream) {
  if (!idx || !count || !queries || !truth_ptr || !truth_idx || !cutoffs_host || !out_metrics || !out_flags ||
      k < 1 || k > DCUE_TOPK_MAX_K || n_query_rows <= 0)
    return DCUE_ERR_INVALID;
  TRY(tm_check_common(n_queries, n_cutoffs, n_cand));
  if (n_query_rows > INT32_MAX) return DCUE_ERR_UNSUPPORTED;
  TmCutoffs cut;
  cut.m = n_cutoffs;
  for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i) cut.k[i] = 0;
  for (int i = 0; i < n_cutoffs; ++i) {
    const int32_t c = cutoffs_host[i];
    if (c < 1 || c > k || (i > 0 && c <= cutoffs_host[i - 1])) return DCUE_ERR_INVALID;
    cut.k[i] = c;
  }
  if (n_queries == 0) return DCUE_OK;
  hipStream_t s = (hipStream_t)stream;
  DCUE_LAUNCH(k_topk_metrics_table, dim3(1), dim3(kTmPos), 0, s, (int)kTmPos);
  DCUE_LAUNCH_CHECK();
  DCUE_LAUNCH(k_topk_metrics, dim3((unsigned)((n_queries + 3) / 4)), dim3(256), 0, s, idx, count, (int)n_queries,
              (int)k, queries, truth_ptr, truth_idx, (int)n_query_rows, (int)n_cand, cut, out_metrics, out_flags,
              exposure);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

int dcue_topk_metrics_mean(const double* metrics, const int32_t* flags, int32_t n_queries, int32_t n_cutoffs,
                           const int32_t* exposure, const uint8_t* cand_mask, int64_t n_cand, double* out_mean,
                           double* out_coverage, int32_t* out_n_evaluated, void* stream) {
  if (!metrics || !flags || !out_mean || !out_n_evaluated || (exposure == nullptr) != (out_coverage == nullptr))
    return DCUE_ERR_INVALID;
  TRY(tm_check_common(n_queries, n_cutoffs, n_cand));
  DCUE_LAUNCH(k_topk_metrics_mean, dim3(1), dim3(kTmMeanThreads), 0, (hipStream_t)stream, metrics, flags,
              (int)n_queries, (int)n_cutoffs, exposure, cand_mask, (int)n_cand, out_mean, out_coverage,
              out_n_evaluated);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

}  // extern "C"
