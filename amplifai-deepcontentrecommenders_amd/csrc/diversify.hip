// Diversity-aware serving: Maximal Marginal Relevance re-ranking of the lists dcue_topk
// leaves in device memory, and their intra-list diversity. The definitions are include/dcue.h's
// (dcue_list_mmr / dcue_list_ild).
//
//   div_similarity   (device function, shared by both kernels) one 256-thread workgroup per list: range
//                    check of the entries, then the pool's rows gathered into LDS in column chunks of at
//                    most 128 and their P x P Gram matrix on v_mfma_f32_16x16x4_f32 -- wave w owns tile
//                    rows w and w + 4, so the whole Gram lives in at most sixteen 16 x 16 accumulator
//                    tiles per wave across the chunks. The finished Gram goes to LDS once (odd pitch, over
//                    the row tile, which is dead by then), the reciprocal clamped norms come from its
//                    diagonal, and G[a][b] * (inv[a] * inv[b]) is the cosine: symmetric bit for bit.
//   k_list_mmr       the greedy loop on wave 0 alone, two pool positions per lane (k_topk_metrics'
//                    layout): a step is f for the lane's positions, a butterfly maximum over the key
//                    ord(f) << 32 | (127 - position) -- f descending, then position ascending, a total
//                    order -- and one row of the similarity matrix folded into m by max. No workgroup
//                    barrier inside the loop.
//   k_list_ild       thread b sums 1 - sim(a, b) over a < b in ascending a (fp64); thread i then adds the
//                    column sums b < n_K of cutoff i in ascending b.
//   k_list_ild_mean  ONE workgroup, k_topk_metrics_mean's column sums (colmean.h col_means): thread
//                    (g, column) sums rows g, g + G, ... in that order, a column's G partials are added
//                    in ascending g.
// A list's outputs depend on the list and the rows it names alone; the Gram's summation order on d alone.
#include "dcue_internal.h"
#include "diversify.h"
#include "colmean.h"

namespace dcue {

static_assert(kDivPos == DCUE_TOPK_MAX_K && kDivPos == 128, "the selecting wave64 gives each lane two pool positions");
static_assert(div_dp(100) == rank_dp(100) && div_dp(256) == rank_dp(256), "div_dp is rank_dp");

struct DivLds {
  float* tile;  // the row tile, then the similarity matrix
  double* colsum;
  int* idx;
  float *rel, *inv;
  int *order, *misc;
};

__device__ __forceinline__ DivLds div_carve(float* lds, int pool, int d) {
  DivLds L;
  L.tile = lds;
  L.colsum = reinterpret_cast<double*>(lds + ((div_tile_floats(pool, d) + 3) & ~(size_t)3));
  L.idx = reinterpret_cast<int*>(L.colsum + kDivPos);
  L.rel = reinterpret_cast<float*>(L.idx + kDivPos);
  L.inv = L.rel + kDivPos;
  L.order = reinterpret_cast<int*>(L.inv + kDivPos);
  L.misc = L.order + kDivPos;
  return L;
}

// The cosine matrix of list positions 0 .. c-1 into L.tile at pitch p16 + 1 (entries at positions >= c
// are not written and must not be read); L.idx holds the entries, L.rel the relevances (rel != null).
// Returns the list's flags, the same value in every thread: DCUE_LIST_FLAG_BAD_INDEX (nothing was
// gathered) or DCUE_LIST_FLAG_NONFINITE, 0 otherwise. All 256 threads call it; ends on a barrier.
__device__ int div_similarity(const DivLds& L, const int32_t* __restrict__ list, const float* __restrict__ rel, int c,
                              const float* __restrict__ cand_feat, int n_cand, int d, int p16, bool vec) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, l16 = lane & 15;
  const int pitch = p16 + 1;
  const int c16 = (c + 15) & ~15, T = c16 >> 4;
  if (tid < 2) L.misc[tid] = 0;
  __syncthreads();
  // entries at j >= c are never read; an entry is range-checked before it addresses anything
  if (tid < c) {
    const int v = list[tid];
    L.idx[tid] = v;
    if (v < 0 || v >= n_cand) atomicOr(&L.misc[0], DCUE_LIST_FLAG_BAD_INDEX);
    if (rel) {
      const float r = rel[tid];
      L.rel[tid] = r;
      if (!(fabsf(r) < __builtin_inff())) atomicOr(&L.misc[1], DCUE_LIST_FLAG_NONFINITE);
    }
  }
  __syncthreads();
  if (L.misc[0]) return L.misc[0];

  f32x4 acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int dp = rank_dp(d);
  for (int c0 = 0; c0 < dp; c0 += kDivChunk) {
    const int kc = dp - c0 < kDivChunk ? dp - c0 : kDivChunk, st = kc + 4;
    if (c0) __syncthreads();  // the previous chunk's reads
    // rows c .. c16-1 and columns d .. dp-1 are zero
    if (vec) {
      const int kc4 = kc >> 2;
      for (int e = tid; e < c16 * kc4; e += 256) {
        const int r = e / kc4, col = 4 * (e - r * kc4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < c && c0 + col < d) v = ld4(cand_feat + (size_t)L.idx[r] * d + c0 + col);
        st4(&L.tile[r * st + col], v);
      }
    } else {
      for (int e = tid; e < c16 * kc; e += 256) {
        const int r = e / kc, col = e - r * kc;
        L.tile[r * st + col] = (r < c && c0 + col < d) ? cand_feat[(size_t)L.idx[r] * d + c0 + col] : 0.f;
      }
    }
    __syncthreads();
    const int kq = kc >> 2;  // k range per lane group
    for (int j = 0; j < kq; j += 4) {
      float4 a[2];
#pragma unroll
      for (int rr = 0; rr < 2; ++rr)
        if (w + 4 * rr < T) a[rr] = ld4(&L.tile[(16 * (w + 4 * rr) + l16) * st + g * kq + j]);
#pragma unroll
      for (int tc = 0; tc < 8; ++tc)
        if (tc < T) {
          const float4 b = ld4(&L.tile[(16 * tc + l16) * st + g * kq + j]);
#pragma unroll
          for (int rr = 0; rr < 2; ++rr)
            if (w + 4 * rr < T) {
              f32x4 x = acc[8 * rr + tc];
              x = mfma4(a[rr].x, b.x, x);
              x = mfma4(a[rr].y, b.y, x);
              x = mfma4(a[rr].z, b.z, x);
              x = mfma4(a[rr].w, b.w, x);
              acc[8 * rr + tc] = x;
            }
        }
    }
  }
  __syncthreads();  // the row tile is dead: the Gram takes its place
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int tc = 0; tc < 8; ++tc)
      if (w + 4 * rr < T && tc < T) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          L.tile[(16 * (w + 4 * rr) + 4 * g + r) * pitch + 16 * tc + l16] = acc[8 * rr + tc][r];
      }
  __syncthreads();
  if (tid < c) {
    const float n2 = L.tile[tid * pitch + tid];  // >= 0, or not finite: a NaN / infinite row, or its square overflowed
    L.inv[tid] = 1.f / fmaxf(sqrtf(n2), 1e-8f);
    if (!(n2 < __builtin_inff())) atomicOr(&L.misc[1], DCUE_LIST_FLAG_NONFINITE);
  }
  __syncthreads();
  if (L.misc[1]) return L.misc[1];
  for (int e = tid; e < c * kDivPos; e += 256) {
    const int a = e >> 7, b = e & (kDivPos - 1);
    if (b < c) L.tile[a * pitch + b] *= L.inv[a] * L.inv[b];  // (a, b) and (b, a): the same bits
  }
  __syncthreads();
  return 0;
}

// lam * r - oml * m, each operation rounded on its own
__device__ __forceinline__ float mmr_value(float lam, float oml, float r, float m) {
#pragma clang fp contract(off)
  const float x = lam * r, y = oml * m;
  return (x - y) + 0.f;  // -0 -> +0: one key per value
}

__device__ __forceinline__ unsigned long long div_wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(256) void k_list_mmr(const int32_t* __restrict__ idx, const float* __restrict__ score,
                                                  const int32_t* __restrict__ count, int pool,
                                                  const float* __restrict__ cand_feat, int n_cand, int d, bool vec,
                                                  float lam, int rel_mode, int k_out, int32_t* __restrict__ out_idx,
                                                  float* __restrict__ out_score, int32_t* __restrict__ out_count,
                                                  int32_t* __restrict__ out_flags) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DivLds L = div_carve(lds, pool, d);
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int p16 = div_p16(pool), pitch = p16 + 1;
  int c = count[q];
  c = c < 0 ? 0 : c > pool ? pool : c;
  const int f = div_similarity(L, idx + (size_t)q * pool, score + (size_t)q * pool, c, cand_feat, n_cand, d, p16, vec);
  if (tid >= 64) return;  // (whole waves: no barrier follows)
  const int n_sel = f ? 0 : (k_out < c ? k_out : c);
  const int p[2] = {lane, lane + 64};
  float r[2], m[2] = {0.f, 0.f};
  bool open[2];  // a real, unselected position
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    open[i] = p[i] < c && n_sel > 0;
    r[i] = open[i] ? L.rel[p[i]] : 0.f;
  }
  if (rel_mode == DCUE_MMR_REL_MINMAX && n_sel > 0) {
    float lo = fminf(open[0] ? r[0] : __builtin_inff(), open[1] ? r[1] : __builtin_inff());
    float hi = fmaxf(open[0] ? r[0] : -__builtin_inff(), open[1] ? r[1] : -__builtin_inff());
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, o, 64));
      hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    const float span = hi - lo;
#pragma unroll
    for (int i = 0; i < 2; ++i) r[i] = hi == lo ? 0.f : (r[i] - lo) / span;
  }
  const float oml = 1.f - lam;
  for (int t = 0; t < n_sel; ++t) {
    unsigned long long key = 0ull;  // below every real key
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned long long ki =
          ((unsigned long long)ord_key(mmr_value(lam, oml, r[i], m[i])) << 32) | (unsigned)(kDivPos - 1 - p[i]);
      if (open[i] && ki > key) key = ki;
    }
    // t < c: at least one position is open, so the maximum is a real key (the min only bounds the row read)
    const int s = min(kDivPos - 1 - (int)(unsigned)div_wave_max(key), c - 1);
    if (lane == 0) L.order[t] = s;
    const float* row = L.tile + s * pitch;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (p[i] == s) open[i] = false;
      if (p[i] < c) m[i] = t == 0 ? row[p[i]] : fmaxf(m[i], row[p[i]]);
    }
  }
  // (one wave: its own LDS stores are visible to it in program order)
  const size_t o = (size_t)q * k_out;
  for (int j = lane; j < k_out; j += 64) {
    const int s = j < n_sel ? L.order[j] : 0;
    out_idx[o + j] = j < n_sel ? L.idx[s] : -1;
    out_score[o + j] = j < n_sel ? L.rel[s] : -__builtin_inff();
  }
  if (lane == 0) {
    out_count[q] = n_sel;
    out_flags[q] = f;
  }
}

struct IldCutoffs {
  int m;
  int k[DCUE_TOPK_METRICS_MAX_CUTOFFS];
};

__global__ __launch_bounds__(256) void k_list_ild(const int32_t* __restrict__ idx, const int32_t* __restrict__ count,
                                                  int k, const float* __restrict__ cand_feat, int n_cand, int d,
                                                  bool vec, IldCutoffs cut, double* __restrict__ out,
                                                  int32_t* __restrict__ out_flags) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DivLds L = div_carve(lds, k, d);
  const int q = blockIdx.x, tid = threadIdx.x;
  const int p16 = div_p16(k), pitch = p16 + 1;
  int c = count[q];
  c = c < 0 ? 0 : c > k ? k : c;
  int f = div_similarity(L, idx + (size_t)q * k, nullptr, c, cand_feat, n_cand, d, p16, vec);
  if (f) {  // (uniform)
    if (tid < cut.m) out[(size_t)q * cut.m + tid] = 0.0;
    if (tid == 0) out_flags[q] = f;
    return;
  }
  if (tid < c) {
    double s = 0.0;
    for (int a = 0; a < tid; ++a) s += 1.0 - (double)L.tile[a * pitch + tid];
    L.colsum[tid] = s;
  }
  __syncthreads();
  if (tid < cut.m) {
    int kap = 0;
#pragma unroll
    for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i)
      if (tid == i) kap = cut.k[i];
    const int nk = kap < c ? kap : c;
    double s = 0.0;
    for (int b = 0; b < nk; ++b) s += L.colsum[b];
    out[(size_t)q * cut.m + tid] = nk < 2 ? 0.0 : 2.0 / ((double)nk * (double)(nk - 1)) * s;
  }
  if (tid == 0) out_flags[q] = (cut.k[0] < c ? cut.k[0] : c) < 2 ? DCUE_LIST_FLAG_NO_PAIR : 0;  // ascending cutoffs
}

__global__ __launch_bounds__(kColMeanThreads) void k_list_ild_mean(const double* __restrict__ ild,
                                                                   const int32_t* __restrict__ flags, int n, int m,
                                                                   double* __restrict__ out_mean,
                                                                   int32_t* __restrict__ out_n) {
  __shared__ double part[kColMeanThreads];
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  col_means(ild, flags, n, m, part, &cnt, out_mean, out_n);
}

static int div_check(int32_t n_lists, int32_t pool, int64_t n_cand, int32_t d) {
  if (n_lists < 0 || pool < 1 || pool > DCUE_TOPK_MAX_K || n_cand <= 0 || d <= 0) return DCUE_ERR_INVALID;
  if (d > 256 || n_cand > INT32_MAX - 64) return DCUE_ERR_UNSUPPORTED;  // dcue_topk's bounds
  return DCUE_OK;
}

// rows of whole float4: every row start and every 4-column group of it is 16-byte aligned
static bool div_vec(const float* cand_feat, int d) { return (d & 3) == 0 && ((uintptr_t)cand_feat & 15) == 0; }

static int div_lds_attr() {
  static bool attr = false;
  if (!attr) {
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_list_mmr, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kDivLdsBudget));
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_list_ild, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kDivLdsBudget));
    attr = true;
  }
  return DCUE_OK;
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_list_mmr_workspace_bytes(int32_t pool, int32_t d, int32_t n_lists, size_t* bytes) {
  if (!bytes) return DCUE_ERR_INVALID;
  TRY(div_check(n_lists, pool, 1, d));
  *bytes = 0;  // the kernels keep everything in LDS
  return DCUE_OK;
}

int dcue_list_mmr(const int32_t* idx, const float* score, const int32_t* count, int32_t n_lists, int32_t pool,
                  const float* cand_feat, int64_t n_cand, int32_t d, float lambda, int32_t rel_mode, int32_t k_out,
                  void* ws, size_t ws_bytes, int32_t* out_idx, float* out_score, int32_t* out_count,
                  int32_t* out_flags, void* stream) {
  if (!idx || !score || !count || !cand_feat || !out_idx || !out_score || !out_count || !out_flags)
    return DCUE_ERR_INVALID;
  TRY(div_check(n_lists, pool, n_cand, d));
  if (k_out < 1 || k_out > pool || !(lambda >= 0.f && lambda <= 1.f) ||
      (rel_mode != DCUE_MMR_REL_RAW && rel_mode != DCUE_MMR_REL_MINMAX))
    return DCUE_ERR_INVALID;
  size_t need = 0;
  TRY(dcue_list_mmr_workspace_bytes(pool, d, n_lists, &need));
  if (need > ws_bytes || (need && !ws)) return DCUE_ERR_WORKSPACE;
  if (n_lists == 0) return DCUE_OK;
  TRY(div_lds_attr());
  DCUE_LAUNCH(k_list_mmr, dim3((unsigned)n_lists), dim3(256), div_lds_bytes(pool, d), (hipStream_t)stream, idx, score,
              count, (int)pool, cand_feat, (int)n_cand, (int)d, div_vec(cand_feat, d), lambda, (int)rel_mode,
              (int)k_out, out_idx, out_score, out_count, out_flags);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

int dcue_list_ild(const int32_t* idx, const int32_t* count, int32_t n_lists, int32_t k, const float* cand_feat,
                  int64_t n_cand, int32_t d, const int32_t* cutoffs_host, int32_t n_cutoffs, void* ws,
                  size_t ws_bytes, double* out_ild, int32_t* out_flags, void* stream) {
  if (!idx || !count || !cand_feat || !cutoffs_host || !out_ild || !out_flags || n_cutoffs < 1 ||
      n_cutoffs > DCUE_TOPK_METRICS_MAX_CUTOFFS)
    return DCUE_ERR_INVALID;
  TRY(div_check(n_lists, k, n_cand, d));
  IldCutoffs cut;
  cut.m = n_cutoffs;
  for (int i = 0; i < DCUE_TOPK_METRICS_MAX_CUTOFFS; ++i) cut.k[i] = 0;
  for (int i = 0; i < n_cutoffs; ++i) {
    const int32_t c = cutoffs_host[i];
    if (c < 1 || c > k || (i > 0 && c <= cutoffs_host[i - 1])) return DCUE_ERR_INVALID;
    cut.k[i] = c;
  }
  size_t need = 0;
  TRY(dcue_list_mmr_workspace_bytes(k, d, n_lists, &need));
  if (need > ws_bytes || (need && !ws)) return DCUE_ERR_WORKSPACE;
  if (n_lists == 0) return DCUE_OK;
  TRY(div_lds_attr());
  DCUE_LAUNCH(k_list_ild, dim3((unsigned)n_lists), dim3(256), div_lds_bytes(k, d), (hipStream_t)stream, idx, count,
              (int)k, cand_feat, (int)n_cand, (int)d, div_vec(cand_feat, d), cut, out_ild, out_flags);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

int dcue_list_ild_mean(const double* ild, const int32_t* flags, int32_t n_lists, int32_t n_cutoffs, double* out_mean,
                       int32_t* out_n_evaluated, void* stream) {
  if (!ild || !flags || !out_mean || !out_n_evaluated || n_lists < 0 || n_cutoffs < 1 ||
      n_cutoffs > DCUE_TOPK_METRICS_MAX_CUTOFFS)
    return DCUE_ERR_INVALID;
  DCUE_LAUNCH(k_list_ild_mean, dim3(1), dim3(kColMeanThreads), 0, (hipStream_t)stream, ild, flags, (int)n_lists,
              (int)n_cutoffs, out_mean, out_n_evaluated);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

}  // extern "C"
