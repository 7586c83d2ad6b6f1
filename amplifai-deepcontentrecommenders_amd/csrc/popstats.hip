// Popularity-bias statistics of served lists: per-list item statistics (novelty = mean
// self-information, long-tail share) on the lists dcue_topk* / dcue_list_mmr / dcue_list_group_cap leave in
// device memory, and the Gini index of the exposure counts dcue_topk_metrics accumulates. The definitions
// are include/dcue.h's (dcue_list_item_stats / dcue_exposure_gini).
//
//   k_list_item_stats       one wave64 per list, four per workgroup (k_topk_metrics' layout), no LDS: lane l
//                           owns list positions l and l + 64. Range check, then the two fp64 values and the
//                           two tail bytes. The value sum runs over the positions in ascending order -- every
//                           lane adds the same broadcast value (a lane read) at a time, so the bits are a
//                           sequential loop's -- and is divided once per cutoff. The tail counts are
//                           popcounts of two ballots.
//   k_list_item_stats_mean  ONE workgroup: colmean.h col_means over the [n][2m] matrix, the order
//                           k_topk_metrics_mean and k_list_ild_mean use.
//   k_gini_hist             one thread per candidate: the exposure cumulated over the cutoffs, and for every
//                           cutoff one integer atomic on the histogram bin of that value. Zeros are not
//                           counted (most of a catalogue is never served; their number is n minus the rest).
//                           A value outside the histogram marks the cutoff instead of addressing anything.
//   k_gini_scan             one workgroup per cutoff: threads own contiguous runs of bins, a block scan of
//                           the runs' counts gives every run its first rank, and a value v of multiplicity m
//                           at ranks r+1..r+m adds v m (2r + m - n) to an int64 sum. One fp64 division.
// Integer arithmetic only, up to the final divisions: nothing depends on launch shape or arrival order.
#include <cstdio>

#include "dcue_internal.h"
#include "colmean.h"

namespace dcue {

constexpr int kPopPos = DCUE_TOPK_MAX_K;  // list positions: two per lane
static_assert(kPopPos == 128, "k_list_item_stats gives each lane of a wave64 two list positions");
static_assert(2 * DCUE_TOPK_METRICS_MAX_CUTOFFS <= 64, "one lane per output of a list");
constexpr int kGiniThreads = 1024;
constexpr size_t kGiniHeader = 64;                  // int32 n, int32 bad[8], padding
constexpr long long kPopExact = 1ll << 53;          // integers below it are fp64 values

struct PopCutoffs {
  int m;
  int k[DCUE_TOPK_METRICS_MAX_CUTOFFS];
};

__device__ __forceinline__ unsigned long long pop_low_mask(int n) {  // bits 0 .. n-1
  return n <= 0 ? 0ull : n >= 64 ? ~0ull : (1ull << n) - 1ull;
}

__global__ __launch_bounds__(256) void k_list_item_stats(const int32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ count, int n_lists, int k,
                                                         const double* __restrict__ item_value,
                                                         const uint8_t* __restrict__ item_tail, int n_cand,
                                                         PopCutoffs cut, double* __restrict__ out,
                                                         int32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_lists) return;  // (whole waves: no barrier follows)
  const int m2 = 2 * cut.m;
  int c = count[q];
  c = c < 0 ? 0 : c > k ? k : c;
  const int32_t* L = idx + (size_t)q * k;
  // entries at j >= c are never read; an entry is range-checked before it addresses anything
  double val[2] = {0.0, 0.0};
  bool tail[2] = {false, false};
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = lane + 64 * i;
    const int v = p < c ? L[p] : -1;
    const bool ok = p < c && v >= 0 && v < n_cand;
    bad |= p < c && !ok;
    if (ok && item_value) val[i] = item_value[v];
    if (ok && item_tail) tail[i] = item_tail[v] != 0;
  }
  const int f = (c == 0 ? 1 : 0) | (__ballot(bad) != 0ull ? DCUE_LIST_FLAG_BAD_INDEX : 0);
  if (f) {  // (wave-uniform) left out of the means
    if (lane < m2) out[(size_t)q * m2 + lane] = 0.0;
    if (lane == 0) flags[q] = f;
    return;
  }
  const unsigned long long t0 = __ballot(tail[0]), t1 = __ballot(tail[1]);
  double s = 0.0, mine = 0.0;  // s: the same bits in every lane
  int j = 0;
#pragma unroll
  for (int t = 0; t < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++t) {
    if (t < cut.m) {
      const int nk = cut.k[t] < c ? cut.k[t] : c;  // >= 1
      for (; j < nk; ++j) s += __shfl(j < 64 ? val[0] : val[1], j & 63, 64);
      const int nt = __popcll(t0 & pop_low_mask(nk)) + __popcll(t1 & pop_low_mask(nk - 64));
      if (lane == 2 * t) mine = s / (double)nk;
      if (lane == 2 * t + 1) mine = (double)nt / (double)nk;
    }
  }
  if (lane < m2) out[(size_t)q * m2 + lane] = mine;
  if (lane == 0) flags[q] = 0;
}

__global__ __launch_bounds__(kColMeanThreads) void k_list_item_stats_mean(const double* __restrict__ stats,
                                                                          const int32_t* __restrict__ flags, int n,
                                                                          int m, double* __restrict__ out_mean,
                                                                          int32_t* __restrict__ out_n) {
  __shared__ double part[kColMeanThreads];
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  col_means(stats, flags, n, 2 * m, part, &cnt, out_mean, out_n);
}

struct GiniWs {
  int32_t* n;      // candidates the mask admits
  int32_t* bad;    // [8] a value of the cutoff fell outside the histogram
  uint32_t* hist;  // [m][bins]; bin 0 is not used
};

__host__ __device__ inline GiniWs gini_carve(void* ws) {
  GiniWs w;
  w.n = reinterpret_cast<int32_t*>(ws);
  w.bad = w.n + 1;
  w.hist = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + kGiniHeader);
  return w;
}

__global__ __launch_bounds__(256) void k_gini_hist(const int32_t* __restrict__ exposure,
                                                   const uint8_t* __restrict__ mask, int n_cand, int m,
                                                   long long bins, void* ws) {
  const GiniWs w = gini_carve(ws);
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool in = c < n_cand && (mask ? mask[c] != 0 : true);
  if (in) {
    long long x = 0;
    bool neg = false;
#pragma unroll
    for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i)
      if (i < m) {
        const int e = exposure[(size_t)i * n_cand + c];
        neg |= e < 0;
        x += e;
        if (neg || x >= bins) w.bad[i] = 1;  // (every writer stores the same value)
        else if (x > 0) atomicAdd(&w.hist[(size_t)i * bins + x], 1u);
      }
  }
  const int cnt = wave_sum_int(in ? 1 : 0);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(w.n, cnt);
}

__device__ __forceinline__ long long gini_wave_scan(long long v, int lane) {  // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

__global__ __launch_bounds__(kGiniThreads) void k_gini_scan(long long bins, void* ws, double* __restrict__ out_gini,
                                                            long long* __restrict__ out_total) {
  __shared__ long long wtot[kGiniThreads / 64];
  __shared__ unsigned long long acc[2];  // numerator (two's complement), total
  const GiniWs w = gini_carve(ws);
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t* h = w.hist + (size_t)i * bins;
  const long long n = *w.n;
  if (tid < 2) acc[tid] = 0ull;
  const long long per = (bins + kGiniThreads - 1) / kGiniThreads;
  long long b0 = tid * per, b1 = b0 + per;
  b0 = b0 < 1 ? 1 : b0;  // bin 0 holds nothing: the zeros are the candidates no other bin counts
  b1 = b1 < bins ? b1 : bins;
  long long mine = 0;
  for (long long v = b0; v < b1; ++v) mine += h[v];
  const long long inc = gini_wave_scan(mine, lane);
  if (lane == 63) wtot[wv] = inc;
  __syncthreads();
  long long before = inc - mine, positive = 0;
  for (int u = 0; u < kGiniThreads / 64; ++u) {
    before += u < wv ? wtot[u] : 0;
    positive += wtot[u];
  }
  // ranks: the n - positive zeros first, then the bins in ascending value. Unsigned arithmetic: where
  // n * total is beyond 2^53 a term may wrap, and the result is then refused below.
  unsigned long long r = (unsigned long long)(n - positive + before), num = 0ull, tot = 0ull;
  for (long long v = b0; v < b1; ++v) {
    const unsigned long long mv = h[v];
    if (mv) {
      num += (unsigned long long)v * mv * (2ull * r + mv - (unsigned long long)n);
      tot += (unsigned long long)v * mv;
      r += mv;
    }
  }
  if (num) atomicAdd(&acc[0], num);
  if (tot) atomicAdd(&acc[1], tot);
  __syncthreads();
  if (tid == 0) {
    const long long total = (long long)acc[1];
    // every run's total is below bins * n: 2^53 / DCUE_TOPK_MAX_K by the host's refusal
    const bool exact = n == 0 || total <= (kPopExact - 1) / n;
    if (w.bad[i] || !exact) {
      out_gini[i] = 0.0;
      out_total[i] = -1;
    } else {
      out_gini[i] = (n == 0 || total == 0) ? 0.0 : (double)(long long)acc[0] / (double)(n * total);
      out_total[i] = total;
    }
  }
}

static int pop_fail(int code, const char* why) {
  set_last_message(why);
  return code;
}

static int pop_check(const char* fn, int32_t n_lists, int32_t n_cutoffs) {
  char msg[160];
  const char* why = nullptr;
  if (n_lists < 0) why = "n_lists must not be negative";
  else if (n_cutoffs < 1 || n_cutoffs > DCUE_TOPK_METRICS_MAX_CUTOFFS) why = "n_cutoffs must be in 1..8";
  if (!why) return DCUE_OK;
  snprintf(msg, sizeof(msg), "%s: %s", fn, why);
  return pop_fail(DCUE_ERR_INVALID, msg);
}

static int gini_check(const char* fn, int64_t n_cand, int32_t n_cutoffs) {
  char msg[160];
  if (n_cand <= 0) {
    snprintf(msg, sizeof(msg), "%s: n_cand must be positive", fn);
    return pop_fail(DCUE_ERR_INVALID, msg);
  }
  if (n_cutoffs < 1 || n_cutoffs > DCUE_TOPK_METRICS_MAX_CUTOFFS) {
    snprintf(msg, sizeof(msg), "%s: n_cutoffs must be in 1..8", fn);
    return pop_fail(DCUE_ERR_INVALID, msg);
  }
  if (n_cand > INT32_MAX - 64) {  // dcue_topk's bound: indices are int32
    snprintf(msg, sizeof(msg), "%s: n_cand is beyond dcue_topk's bound", fn);
    return pop_fail(DCUE_ERR_UNSUPPORTED, msg);
  }
  return DCUE_OK;
}

// n_cand * (bins - 1) * DCUE_TOPK_MAX_K must stay below 2^53 (bins - 1 = the lists the histogram is sized for)
static bool gini_exact(int64_t n_cand, long long bins) {
  return (bins - 1) <= (kPopExact - 1) / DCUE_TOPK_MAX_K / n_cand;
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_list_item_stats(const int32_t* idx, const int32_t* count, int32_t n_lists, int32_t k,
                         const double* item_value, const uint8_t* item_tail, int64_t n_cand,
                         const int32_t* cutoffs_host, int32_t n_cutoffs, double* out_stats, int32_t* out_flags,
                         void* stream) {
  if (!idx || !count || !cutoffs_host || !out_stats || !out_flags)
    return pop_fail(DCUE_ERR_INVALID, "dcue_list_item_stats: null pointer");
  TRY(pop_check("dcue_list_item_stats", n_lists, n_cutoffs));
  if (k < 1 || k > DCUE_TOPK_MAX_K) return pop_fail(DCUE_ERR_INVALID, "dcue_list_item_stats: k must be in 1..128");
  if (n_cand <= 0) return pop_fail(DCUE_ERR_INVALID, "dcue_list_item_stats: n_cand must be positive");
  if (n_cand > INT32_MAX - 64)
    return pop_fail(DCUE_ERR_UNSUPPORTED, "dcue_list_item_stats: n_cand is beyond dcue_topk's bound");
  PopCutoffs cut;
  cut.m = n_cutoffs;
  for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i) cut.k[i] = 0;
  for (int i = 0; i < n_cutoffs; ++i) {
    const int32_t c = cutoffs_host[i];
    if (c < 1 || c > k || (i > 0 && c <= cutoffs_host[i - 1]))
      return pop_fail(DCUE_ERR_INVALID, "dcue_list_item_stats: cutoffs must be strictly ascending within 1..k");
    cut.k[i] = c;
  }
  if (n_lists == 0) return DCUE_OK;
  DCUE_LAUNCH(k_list_item_stats, dim3((unsigned)((n_lists + 3) / 4)), dim3(256), 0, (hipStream_t)stream, idx, count,
              (int)n_lists, (int)k, item_value, item_tail, (int)n_cand, cut, out_stats, out_flags);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

int dcue_list_item_stats_mean(const double* stats, const int32_t* flags, int32_t n_lists, int32_t n_cutoffs,
                              double* out_mean, int32_t* out_n_evaluated, void* stream) {
  if (!stats || !flags || !out_mean || !out_n_evaluated)
    return pop_fail(DCUE_ERR_INVALID, "dcue_list_item_stats_mean: null pointer");
  TRY(pop_check("dcue_list_item_stats_mean", n_lists, n_cutoffs));
  DCUE_LAUNCH(k_list_item_stats_mean, dim3(1), dim3(kColMeanThreads), 0, (hipStream_t)stream, stats, flags,
              (int)n_lists, (int)n_cutoffs, out_mean, out_n_evaluated);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

int dcue_exposure_gini_workspace_bytes(int64_t n_cand, int32_t n_cutoffs, int64_t n_lists_max, size_t* bytes) {
  if (!bytes) return pop_fail(DCUE_ERR_INVALID, "dcue_exposure_gini_workspace_bytes: null pointer");
  TRY(gini_check("dcue_exposure_gini_workspace_bytes", n_cand, n_cutoffs));
  if (n_lists_max < 0)
    return pop_fail(DCUE_ERR_INVALID, "dcue_exposure_gini_workspace_bytes: n_lists_max must not be negative");
  if (n_lists_max >= kPopExact || !gini_exact(n_cand, n_lists_max + 1))
    return pop_fail(DCUE_ERR_UNSUPPORTED,
                    "dcue_exposure_gini_workspace_bytes: n_cand * n_lists_max * 128 reaches 2^53");
  *bytes = kGiniHeader + (size_t)n_cutoffs * (size_t)(n_lists_max + 1) * sizeof(uint32_t);
  return DCUE_OK;
}

int dcue_exposure_gini(const int32_t* exposure, const uint8_t* cand_mask, int64_t n_cand, int32_t n_cutoffs, void* ws,
                       size_t ws_bytes, double* out_gini, int64_t* out_total, void* stream) {
  if (!exposure || !ws || !out_gini || !out_total)
    return pop_fail(DCUE_ERR_INVALID, "dcue_exposure_gini: null pointer");
  TRY(gini_check("dcue_exposure_gini", n_cand, n_cutoffs));
  if (ws_bytes < kGiniHeader + (size_t)n_cutoffs * 2 * sizeof(uint32_t))
    return pop_fail(DCUE_ERR_WORKSPACE, "dcue_exposure_gini: the workspace holds no histogram bin");
  const long long bins = (long long)((ws_bytes - kGiniHeader) / sizeof(uint32_t) / (size_t)n_cutoffs);
  if (!gini_exact(n_cand, bins))
    return pop_fail(DCUE_ERR_UNSUPPORTED, "dcue_exposure_gini: n_cand * (lists the workspace is sized for) * 128 "
                                          "reaches 2^53");
  hipStream_t s = (hipStream_t)stream;
  DCUE_HIP_CHECK(hipMemsetAsync(ws, 0, kGiniHeader + (size_t)n_cutoffs * (size_t)bins * sizeof(uint32_t), s));
  DCUE_LAUNCH(k_gini_hist, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, s, exposure, cand_mask, (int)n_cand,
              (int)n_cutoffs, bins, ws);
  DCUE_LAUNCH_CHECK();
  DCUE_LAUNCH(k_gini_scan, dim3((unsigned)n_cutoffs), dim3(kGiniThreads), 0, s, bins, ws, out_gini,
              (long long*)out_total);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

}  // extern "C"
