// Group-aware serving: a cap of `cap` entries per group (artist, album, label) on the
// ranked lists dcue_topk / dcue_list_mmr leave in device memory, and the lists' group-level statistics.
// The definitions are include/dcue.h's (dcue_list_group_cap / dcue_list_group_stats).
//
//   k_list_group_cap         one wave64 per list, four per workgroup (k_topk_metrics' layout): lane l owns
//                            pool positions l and l + 64 and carried entries l and l + 64. Range check,
//                            then the group ids go to the wave's LDS slice -- carried groups in slots
//                            0..127, the pool's in 128..255. r_j = the carried slots and the pool slots
//                            before j that hold j's group: every lane reads the same slot at a time (an
//                            LDS broadcast), at most 255 compares per position. The survivors are two
//                            ballots; an entry's place in the output is the carry count plus a popcount
//                            below it. Index and score bits are copied.
//   k_list_group_stats       the same layout, the pool slots only: one pass over the slots in ascending
//                            order keeps, per lane position, the equal ids before it (first occurrence)
//                            and the equal ids before the running cutoff (the group's size at it).
//   k_list_group_stats_mean  ONE workgroup: int64 column sums of the unflagged rows (integer adds: any
//                            order gives the same sum), one fp64 division each; then one pass over the
//                            groups for the coverage counts.
// No floating-point arithmetic outside the mean's divisions, no workspace, no cross-workgroup
// communication; the only global atomics are the integer exposure adds.
#include <cstdio>

#include "dcue_internal.h"
#include "colmean.h"

namespace dcue {

constexpr int kGrpPos = DCUE_TOPK_MAX_K;  // pool positions / carried entries: two per lane
static_assert(kGrpPos == 128, "the kernels give each lane of a wave64 two positions");
static_assert(2 * DCUE_TOPK_METRICS_MAX_CUTOFFS <= 64, "one lane per cutoff of a list");

struct GrpCutoffs {
  int m;
  int k[DCUE_TOPK_METRICS_MAX_CUTOFFS];
};

__device__ __forceinline__ unsigned long long grp_below(int lane) { return (1ull << lane) - 1ull; }  // bits 0 .. lane-1

__device__ __forceinline__ unsigned long long grp_low_mask(int n) {  // bits 0 .. n-1
  return n <= 0 ? 0ull : n >= 64 ? ~0ull : (1ull << n) - 1ull;
}

__device__ __forceinline__ int grp_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(256) void k_list_group_cap(
    const int32_t* __restrict__ idx, const float* __restrict__ score, const int32_t* __restrict__ count, int n_lists,
    int pool, const int32_t* __restrict__ group_of, int n_cand, int n_groups, int cap, int k_out,
    const int32_t* __restrict__ carry_idx, const float* __restrict__ carry_score,
    const int32_t* __restrict__ carry_count, int32_t* __restrict__ out_idx, float* __restrict__ out_score,
    int32_t* __restrict__ out_count, int32_t* __restrict__ out_dropped, int32_t* __restrict__ out_flags) {
  __shared__ int gl[4][2 * kGrpPos];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + w;
  const bool live = q < n_lists;  // (wave-uniform; every wave reaches the barrier)
  int c = 0, kc = 0;
  if (live) {
    c = count[q];
    c = c < 0 ? 0 : c > pool ? pool : c;
    if (carry_idx) {
      kc = carry_count[q];
      kc = kc < 0 ? 0 : kc > k_out ? k_out : kc;
    }
  }
  // entries at j >= c (carried: j >= kc) are never read; an entry is range-checked before it addresses
  // anything
  int v[2], cv[2], g[2], cg[2];
  float sc[2], cs[2];
  bool bad = false, badg = false;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = lane + 64 * i;
    v[i] = cv[i] = g[i] = cg[i] = -1;
    sc[i] = cs[i] = -__builtin_inff();
    if (p < c) {
      v[i] = idx[(size_t)q * pool + p];
      sc[i] = score[(size_t)q * pool + p];
    }
    if (p < kc) {
      cv[i] = carry_idx[(size_t)q * k_out + p];
      cs[i] = carry_score[(size_t)q * k_out + p];
    }
    const bool ok = p < c && v[i] >= 0 && v[i] < n_cand, cok = p < kc && cv[i] >= 0 && cv[i] < n_cand;
    bad |= (p < c && !ok) || (p < kc && !cok);
    if (ok) g[i] = group_of[v[i]];
    if (cok) cg[i] = group_of[cv[i]];
    badg |= g[i] < -1 || g[i] >= n_groups || cg[i] < -1 || cg[i] >= n_groups;
    gl[w][p] = cg[i];
    gl[w][kGrpPos + p] = g[i];
  }
  __syncthreads();
  if (!live) return;  // (no barrier follows)
  const int f = (__ballot(bad) != 0ull ? DCUE_LIST_FLAG_BAD_INDEX : 0) |
                (__ballot(badg) != 0ull ? DCUE_GROUP_FLAG_BAD_GROUP : 0);
  const size_t o = (size_t)q * k_out;
  if (f) {  // (wave-uniform) count 0 and all padding
    for (int j = lane; j < k_out; j += 64) {
      out_idx[o + j] = -1;
      out_score[o + j] = -__builtin_inff();
    }
    if (lane == 0) {
      out_count[q] = 0;
      out_flags[q] = f;
      if (out_dropped) out_dropped[q] = 0;
    }
    return;
  }
  // r_j: carried entries of the position's group, then the pool positions before it
  int r[2] = {0, 0};
  for (int i = 0; i < kc; ++i) {
    const int x = gl[w][i];
    r[0] += x == g[0];
    r[1] += x == g[1];
  }
  for (int i = 0; i < c; ++i) {
    const int x = gl[w][kGrpPos + i];
    r[0] += i < lane && x == g[0];
    r[1] += i < lane + 64 && x == g[1];
  }
  const bool in0 = lane < c, in1 = lane + 64 < c;
  const bool keep0 = in0 && (g[0] < 0 || r[0] < cap), keep1 = in1 && (g[1] < 0 || r[1] < cap);
  const unsigned long long b0 = __ballot(keep0), b1 = __ballot(keep1);
  const int n0 = __popcll(b0);
  const int at0 = kc + __popcll(b0 & grp_below(lane));       // output entries ahead of the position
  const int at1 = kc + n0 + __popcll(b1 & grp_below(lane));
  const int total = kc + n0 + __popcll(b1), n_out = total < k_out ? total : k_out;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = lane + 64 * i;
    if (p < kc) {  // kc <= k_out: the carry goes first, unchanged
      out_idx[o + p] = cv[i];
      out_score[o + p] = cs[i];
    }
  }
  if (keep0 && at0 < k_out) {
    out_idx[o + at0] = v[0];
    out_score[o + at0] = sc[0];
  }
  if (keep1 && at1 < k_out) {
    out_idx[o + at1] = v[1];
    out_score[o + at1] = sc[1];
  }
  for (int j = n_out + lane; j < k_out; j += 64) {
    out_idx[o + j] = -1;
    out_score[o + j] = -__builtin_inff();
  }
  // positions the cap removed while the list was not full yet (the sequential walk stops at k_out)
  const unsigned long long d0 = __ballot(in0 && !keep0 && at0 < k_out), d1 = __ballot(in1 && !keep1 && at1 < k_out);
  if (lane == 0) {
    out_count[q] = n_out;
    out_flags[q] = n_out < k_out ? DCUE_GROUP_FLAG_SHORT : 0;
    if (out_dropped) out_dropped[q] = __popcll(d0) + __popcll(d1);
  }
}

__global__ __launch_bounds__(256) void k_list_group_stats(const int32_t* __restrict__ idx,
                                                          const int32_t* __restrict__ count, int n_lists, int k,
                                                          const int32_t* __restrict__ group_of, int n_cand,
                                                          int n_groups, GrpCutoffs cut, int32_t* __restrict__ out,
                                                          int32_t* __restrict__ out_flags,
                                                          int32_t* __restrict__ exposure) {
  __shared__ int gl[4][kGrpPos];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + w;
  const bool live = q < n_lists;  // (wave-uniform; every wave reaches the barrier)
  int c = 0;
  if (live) {
    c = count[q];
    c = c < 0 ? 0 : c > k ? k : c;
  }
  int g[2];
  bool bad = false, badg = false;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = lane + 64 * i;
    const int v = p < c ? idx[(size_t)q * k + p] : -1;
    const bool ok = p < c && v >= 0 && v < n_cand;
    bad |= p < c && !ok;
    g[i] = ok ? group_of[v] : -1;
    badg |= g[i] < -1 || g[i] >= n_groups;
    gl[w][p] = g[i];
  }
  __syncthreads();
  if (!live) return;  // (no barrier follows)
  const int f = (__ballot(bad) != 0ull ? DCUE_LIST_FLAG_BAD_INDEX : 0) |
                (__ballot(badg) != 0ull ? DCUE_GROUP_FLAG_BAD_GROUP : 0);
  const int m2 = 2 * cut.m;
  if (f) {  // (wave-uniform) left out of the means and of the exposure counts
    if (lane < m2) out[(size_t)q * m2 + lane] = 0;
    if (lane == 0) out_flags[q] = f;
    return;
  }
  // one ascending pass over the slots: e = equal ids before the position, s = equal ids before the
  // running cutoff
  int e[2] = {0, 0}, s[2] = {0, 0}, mine = 0, i = 0;
  unsigned long long first0 = 0ull, first1 = 0ull;
#pragma unroll
  for (int t = 0; t < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++t) {
    if (t < cut.m) {
      const int nk = cut.k[t] < c ? cut.k[t] : c;
      for (; i < nk; ++i) {
        const int x = gl[w][i];
        const bool q0 = x == g[0], q1 = x == g[1];
        s[0] += q0;
        s[1] += q1;
        e[0] += q0 && i < lane;
        e[1] += q1 && i < lane + 64;
      }
      // (positions below nk have every earlier slot counted in e by now)
      first0 = __ballot(lane < nk && (g[0] < 0 || e[0] == 0));
      first1 = __ballot(lane + 64 < nk && (g[1] < 0 || e[1] == 0));
      const int distinct = __popcll(first0) + __popcll(first1);
      const int t0 = lane < nk ? (g[0] < 0 ? 1 : s[0]) : 0, t1 = lane + 64 < nk ? (g[1] < 0 ? 1 : s[1]) : 0;
      const int top = grp_wave_max(t0 > t1 ? t0 : t1);
      if (lane == 2 * t) mine = distinct;
      if (lane == 2 * t + 1) mine = top;
    }
  }
  if (lane < m2) out[(size_t)q * m2 + lane] = mine;
  if (lane == 0) out_flags[q] = 0;

  if (exposure) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int p = lane + 64 * a;
      int slot = -1;
#pragma unroll
      for (int j = DCUE_TOPK_METRICS_MAX_CUTOFFS - 1; j >= 0; --j)
        if (j < cut.m && p < cut.k[j]) slot = j;  // the first cutoff past p
      if (p < c && slot >= 0 && g[a] >= 0) atomicAdd(&exposure[(size_t)slot * n_groups + g[a]], 1);
    }
  }
}

__global__ __launch_bounds__(kColMeanThreads) void k_list_group_stats_mean(
    const int32_t* __restrict__ stats, const int32_t* __restrict__ flags, int n, int m,
    const int32_t* __restrict__ exposure, const uint8_t* __restrict__ present, int n_groups,
    double* __restrict__ out_mean, double* __restrict__ out_cov, int32_t* __restrict__ out_n) {
  __shared__ unsigned long long sum[2 * DCUE_TOPK_METRICS_MAX_CUTOFFS];
  __shared__ int cnt[2 + DCUE_TOPK_METRICS_MAX_CUTOFFS];  // evaluated, groups present, covered[i]
  const int tid = threadIdx.x, lane = tid & 63, cols = 2 * m;
  if (tid < 2 * DCUE_TOPK_METRICS_MAX_CUTOFFS) sum[tid] = 0ull;
  if (tid < 2 + DCUE_TOPK_METRICS_MAX_CUTOFFS) cnt[tid] = 0;
  __syncthreads();
  const int G = kColMeanThreads / cols;
  if (tid < G * cols) {
    const int col = tid % cols;
    unsigned long long sv = 0ull;  // the values are >= 0
    for (int r = tid / cols; r < n; r += G)
      if (flags[r] == 0) sv += (unsigned long long)stats[(size_t)r * cols + col];
    if (sv) atomicAdd(&sum[col], sv);
  }
  int ne = 0;
  for (int r = tid; r < n; r += kColMeanThreads) ne += flags[r] == 0;
  ne = wave_sum_int(ne);
  if (lane == 0 && ne) atomicAdd(&cnt[0], ne);
  __syncthreads();
  if (tid < cols) out_mean[tid] = cnt[0] > 0 ? (double)(long long)sum[tid] / (double)cnt[0] : 0.0;
  if (tid == 0) *out_n = cnt[0];
  if (!exposure) return;  // (uniform)

  int cov[DCUE_TOPK_METRICS_MAX_CUTOFFS], set = 0;
#pragma unroll
  for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i) cov[i] = 0;
  for (int gi = tid; gi < n_groups; gi += kColMeanThreads) {
    set += present ? present[gi] != 0 : 1;
    int seen = 0;
#pragma unroll
    for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i)
      if (i < m) {
        seen |= exposure[(size_t)i * n_groups + gi] != 0;
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

static int grp_fail(int code, const char* why) {
  set_last_message(why);
  return code;
}

// n_lists, the list width (pool or k), n_cand and n_groups of every entry point
static int grp_check(const char* fn, int32_t n_lists, int32_t width, int64_t n_cand, int32_t n_groups) {
  char msg[160];
  const char* why = nullptr;
  int code = DCUE_ERR_INVALID;
  if (n_lists < 0) why = "n_lists must not be negative";
  else if (width < 1 || width > DCUE_TOPK_MAX_K) why = "the list width (pool / k) must be in 1..128";
  else if (n_cand <= 0) why = "n_cand must be positive";
  else if (n_groups < 0) why = "n_groups must not be negative";
  else if (n_cand > INT32_MAX - 64) {  // dcue_topk's bound: indices are int32
    why = "n_cand is beyond dcue_topk's bound";
    code = DCUE_ERR_UNSUPPORTED;
  }
  if (!why) return DCUE_OK;
  snprintf(msg, sizeof(msg), "%s: %s", fn, why);
  return grp_fail(code, msg);
}

static int grp_cutoffs(const char* fn, const int32_t* cutoffs_host, int32_t n_cutoffs, int32_t k, GrpCutoffs* cut) {
  char msg[160];
  if (n_cutoffs < 1 || n_cutoffs > DCUE_TOPK_METRICS_MAX_CUTOFFS) {
    snprintf(msg, sizeof(msg), "%s: n_cutoffs must be in 1..%d", fn, DCUE_TOPK_METRICS_MAX_CUTOFFS);
    return grp_fail(DCUE_ERR_INVALID, msg);
  }
  cut->m = n_cutoffs;
  for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i) cut->k[i] = 0;
  for (int i = 0; i < n_cutoffs; ++i) {
    const int32_t c = cutoffs_host[i];
    if (c < 1 || c > k || (i > 0 && c <= cutoffs_host[i - 1])) {
      snprintf(msg, sizeof(msg), "%s: cutoffs must be strictly ascending within 1..k", fn);
      return grp_fail(DCUE_ERR_INVALID, msg);
    }
    cut->k[i] = c;
  }
  return DCUE_OK;
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_list_group_cap(const int32_t* idx, const float* score, const int32_t* count, int32_t n_lists, int32_t pool,
                        const int32_t* group_of, int64_t n_cand, int32_t n_groups, int32_t cap, int32_t k_out,
                        const int32_t* carry_idx, const float* carry_score, const int32_t* carry_count,
                        int32_t* out_idx, float* out_score, int32_t* out_count, int32_t* out_dropped,
                        int32_t* out_flags, void* stream) {
  if (!idx || !score || !count || !group_of || !out_idx || !out_score || !out_count || !out_flags)
    return grp_fail(DCUE_ERR_INVALID, "dcue_list_group_cap: null pointer");
  TRY(grp_check("dcue_list_group_cap", n_lists, pool, n_cand, n_groups));
  if (cap < 1) return grp_fail(DCUE_ERR_INVALID, "dcue_list_group_cap: cap must be at least 1");
  if (k_out < 1 || k_out > DCUE_TOPK_MAX_K)
    return grp_fail(DCUE_ERR_INVALID, "dcue_list_group_cap: k_out must be in 1..128");
  const int given = (carry_idx != nullptr) + (carry_score != nullptr) + (carry_count != nullptr);
  if (given != 0 && given != 3)
    return grp_fail(DCUE_ERR_INVALID, "dcue_list_group_cap: carry_idx, carry_score and carry_count go together");
  if (n_lists == 0) return DCUE_OK;
  DCUE_LAUNCH(k_list_group_cap, dim3((unsigned)((n_lists + 3) / 4)), dim3(256), 0, (hipStream_t)stream, idx, score,
              count, (int)n_lists, (int)pool, group_of, (int)n_cand, (int)n_groups, (int)cap, (int)k_out, carry_idx,
              carry_score, carry_count, out_idx, out_score, out_count, out_dropped, out_flags);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

int dcue_list_group_stats(const int32_t* idx, const int32_t* count, int32_t n_lists, int32_t k,
                          const int32_t* group_of, int64_t n_cand, int32_t n_groups, const int32_t* cutoffs_host,
                          int32_t n_cutoffs, int32_t* out_stats, int32_t* out_flags, int32_t* group_exposure,
                          void* stream) {
  if (!idx || !count || !group_of || !cutoffs_host || !out_stats || !out_flags)
    return grp_fail(DCUE_ERR_INVALID, "dcue_list_group_stats: null pointer");
  TRY(grp_check("dcue_list_group_stats", n_lists, k, n_cand, n_groups));
  GrpCutoffs cut;
  TRY(grp_cutoffs("dcue_list_group_stats", cutoffs_host, n_cutoffs, k, &cut));
  if (n_lists == 0) return DCUE_OK;
  DCUE_LAUNCH(k_list_group_stats, dim3((unsigned)((n_lists + 3) / 4)), dim3(256), 0, (hipStream_t)stream, idx, count,
              (int)n_lists, (int)k, group_of, (int)n_cand, (int)n_groups, cut, out_stats, out_flags, group_exposure);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

int dcue_list_group_stats_mean(const int32_t* stats, const int32_t* flags, int32_t n_lists, int32_t n_cutoffs,
                               const int32_t* group_exposure, const uint8_t* group_present, int32_t n_groups,
                               double* out_mean, double* out_coverage, int32_t* out_n_evaluated, void* stream) {
  if (!stats || !flags || !out_mean || !out_n_evaluated)
    return grp_fail(DCUE_ERR_INVALID, "dcue_list_group_stats_mean: null pointer");
  if ((group_exposure == nullptr) != (out_coverage == nullptr))
    return grp_fail(DCUE_ERR_INVALID, "dcue_list_group_stats_mean: group_exposure and out_coverage go together");
  if (n_lists < 0 || n_groups < 0)
    return grp_fail(DCUE_ERR_INVALID, "dcue_list_group_stats_mean: n_lists and n_groups must not be negative");
  if (n_cutoffs < 1 || n_cutoffs > DCUE_TOPK_METRICS_MAX_CUTOFFS)
    return grp_fail(DCUE_ERR_INVALID, "dcue_list_group_stats_mean: n_cutoffs must be in 1..8");
  DCUE_LAUNCH(k_list_group_stats_mean, dim3(1), dim3(kColMeanThreads), 0, (hipStream_t)stream, stats, flags,
              (int)n_lists, (int)n_cutoffs, group_exposure, group_present, (int)n_groups, out_mean, out_coverage,
              out_n_evaluated);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

}  // extern "C"
