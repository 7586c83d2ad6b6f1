// Top-K recommendation: for a batch of query rows, the K candidates with the
// largest nn.CosineSimilarity among those a mask admits and the query's exclusion list (a CSR row,
// the items a user already played) does not name. The [queries][candidates] score matrix is never
// written: the scores of a 64-candidate tile live in the MFMA accumulators and only the few that
// beat the query's current K-th best leave them.
//
//   k_rank_normalize  (rank.hip) x / max(||x||, 1e-8), zero-padded to DP, both sides; under
//                     DCUE_SCORE_DOT (dcue_topk_scored) k_rank_pad instead: the raw rows, zero-padded
//                     -- the score is then the inner product, and everything below is unchanged
//   k_topk_scores     grid (query tiles, candidate splits). The workgroup keeps its query tile in LDS
//                     and streams its candidate chunk through one LDS slab (the next tile's global
//                     loads are in flight during the MFMA loop). Scores as k_rank_scores computes
//                     them: v_mfma_f32_16x16x4_f32, lane group g owns k = g*DP/4 + j -- the same bits
//                     as the evaluator's, whatever the tiling. Selection per query in LDS: `top`, its
//                     best KP (K rounded up to a power of two) keys so far in descending order, a
//                     threshold (the K-th of them) and a 32-slot append buffer. A score whose
//                     candidate the mask admits and which reaches the threshold's score (one float
//                     compare per score, thresholds read four at a time) is keyed, and a key that
//                     beats the threshold is appended (LDS
//                     atomics only: no global load on this path); when a buffer overflows the
//                     workgroup folds every buffer into `top` -- each appended candidate looked up
//                     in its query's exclusion row (binary searches in step, 8 per thread), bitonic
//                     sort of the 32, max against the reversed tail of `top`, bitonic merge -- and the
//                     lanes whose append found no slot try again against the raised threshold. Each workgroup
//                     leaves its K keys per query.
//   k_topk_merge      one workgroup per query: bitonic sort of the splits' partial keys, the first K
//                     decoded into (index, score), count and flags.
// Key = ord(score) << 32 | ~index: unsigned order is score descending, then index ascending, a total
// order, so the result does not depend on tiling, splits or the arrival order of LDS atomics. Key 0
// (below the key of -inf) marks an empty slot. NaN scores are never keyed.
#include "dcue_internal.h"
#include "rank_sort.h"

namespace dcue {

constexpr int kTopkApp = 32;                // append slots per query
constexpr int kTopkMaxSplit = 32;           // k_topk_merge sorts at most 32 * 128 keys in LDS
constexpr int kTopkLdsBudget = 160 * 1024;  // one workgroup per CU may take the CU's whole LDS
constexpr int kTopkFillWgs = 256;           // auto split: workgroups to aim for (the chip's CUs)

struct TopkArgs {
  const float* qn;  // [>= QT-padded nq][dp], zero rows past nq
  int nq;
  const float* cn;  // [64-padded nc][dp], zero rows past nc
  int nc, dp;
  const int32_t* queries;  // this batch's query rows (exclusion rows)
  const int64_t* excl_ptr;
  const int32_t* excl_idx;
  const uint8_t* mask;
  int k, lkp;  // KP = 1 << lkp
  int tiles_per_split, n_tiles;
  int S;
  unsigned long long* parts;  // [nq][S][k]
  int32_t* pflags;            // [nq][S]
  const float* prior;         // [nc] added to every score of the candidate (dcue_topk_prior), or null
};

__host__ __device__ constexpr size_t topk_lds_bytes(int dp, int kp, int qt) {
  return (size_t)(qt + 64) * (dp + 4) * 4 + (size_t)qt * (kp + kTopkApp) * 8 + (size_t)qt * (8 + 8 + 8 + 4 + 4 + 4) + 16;
}

struct TopkLds {
  float *As, *Bs;
  unsigned long long *top, *app, *thr;
  long long *eb, *ee;
  int *cnt, *flg, *over;
  float* thrf;  // the threshold's score (-inf: none yet; +inf: no such query), the scan's first test
};

// Folds every query's append buffer into its sorted best-KP list, dropping the candidates the query
// excludes, and raises the thresholds. All 256 threads call it; ends on a barrier.
template <int QT>
__device__ void topk_compact(const TopkLds& L, int k, int lkp, int n_valid, const int32_t* __restrict__ excl_idx) {
  const int tid = threadIdx.x;
  const int kp = 1 << lkp;
  // empty slots -> 0, and the exclusion test: every appended candidate against its query's sorted
  // exclusion row, the thread's NE binary searches in step so their loads overlap
  constexpr int NE = QT * kTopkApp / 256;
  unsigned long long key[NE];
  long long lo[NE], hi[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = tid + 256 * i, ql = e / kTopkApp;
    key[i] = (e % kTopkApp) < L.cnt[ql] ? L.app[e] : 0ull;
    const bool search = excl_idx && key[i];
    lo[i] = search ? L.eb[ql] : 0;
    hi[i] = search ? L.ee[ql] : 0;
  }
  for (bool more = true; more;) {
    more = false;
    int v[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i)
      if (lo[i] < hi[i]) v[i] = excl_idx[(lo[i] + hi[i]) >> 1];
#pragma unroll
    for (int i = 0; i < NE; ++i)
      if (lo[i] < hi[i]) {
        const long long mid = (lo[i] + hi[i]) >> 1;
        const int c = (int)~(unsigned)key[i];
        if (v[i] == c) {
          key[i] = 0ull;
          lo[i] = hi[i];
        } else if (v[i] < c) {
          lo[i] = mid + 1;
        } else {
          hi[i] = mid;
        }
        more |= lo[i] < hi[i];
      }
  }
#pragma unroll
  for (int i = 0; i < NE; ++i) L.app[tid + 256 * i] = key[i];
  __syncthreads();
  // bitonic sort of each 32-slot buffer, descending: the QT buffers side by side in one pass per
  // stage (block_bitonic_sort would take QT passes, each with its own barriers)
  for (int size = 2; size <= kTopkApp; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < QT * (kTopkApp / 2); t += 256)
        bitonic_cx<true>(L.app + t / (kTopkApp / 2) * kTopkApp, t % (kTopkApp / 2), size, stride);
      __syncthreads();
    }
  }
  // top (descending) against the buffer reversed: the elementwise maximum holds the best KP of
  // both, as a bitonic sequence
  const int lnf = lkp < 5 ? lkp : 5, nf = 1 << lnf;
  for (int e = tid; e < (QT << lnf); e += 256) {
    const int ql = e >> lnf, i = e & (nf - 1);
    unsigned long long* t = L.top + (ql << lkp) + (kp - 1 - i);
    const unsigned long long y = L.app[ql * kTopkApp + i];
    if (y > *t) *t = y;
  }
  __syncthreads();
  // (written out, not bitonic_cx: through the helper this kernel compiles to another instruction
  // order, and its speed moved with it)
  for (int stride = kp >> 1; stride > 0; stride >>= 1) {
    for (int t = tid; t < (QT << lkp) / 2; t += 256) {
      const int ql = t >> (lkp - 1), tt = t & ((kp >> 1) - 1);
      const int lo = 2 * tt - (tt & (stride - 1)), hi = lo + stride;
      unsigned long long* b = L.top + (ql << lkp);
      const unsigned long long x = b[lo], y = b[hi];
      if (x < y) {
        b[lo] = y;
        b[hi] = x;
      }
    }
    __syncthreads();
  }
  if (tid < QT) {
    const unsigned long long kth = L.top[(tid << lkp) + k - 1];
    L.thr[tid] = kth;  // 0 while fewer than K are held: everything passes
    L.thrf[tid] = tid >= n_valid ? __builtin_inff() : kth ? ord_value((unsigned)(kth >> 32)) : -__builtin_inff();
    L.cnt[tid] = 0;
  }
  if (tid == 0) *L.over = 0;
  __syncthreads();
}

__device__ __forceinline__ bool topk_eligible(const TopkArgs& a, const TopkLds& L, int c, int ql) {
  if (a.mask && !a.mask[c]) return false;
  if (!a.excl_ptr) return true;
  long long lo = L.eb[ql], hi = L.ee[ql];
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    const int v = a.excl_idx[mid];
    if (v == c) return false;
    if (v < c) lo = mid + 1; else hi = mid;
  }
  return true;
}

// MT 16-query row tiles per workgroup (QT = 16 MT queries); wave w owns candidate columns 16w..16w+15
// of each 64-candidate tile
// The MFMA loop restates k_rank_scores' (rank.hip) and must stay in step with it: recommend-versus-score
// parity rests on the two loops' k order. A shared forceinline loop was tried; it changed how the
// compiler keeps the accumulators in both kernels, and top-K ran 1 % to 5 % slower by the variant.
// PRIOR (dcue_topk_prior): s = fl32(s0 + prior[c]), one addition on the final accumulator, -0 folded
// again; the lane's prior is prefetched with its mask byte. The PRIOR = false instances are the plain
// calls' and hold none of it.
template <int MT, bool PRIOR>
__global__ __launch_bounds__(256) void k_topk_scores(TopkArgs a) {
  constexpr int QT = 16 * MT;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dp = a.dp, st = dp + 4;
  const int kp = 1 << a.lkp;
  TopkLds L;
  L.As = lds;
  L.Bs = lds + QT * st;
  L.top = reinterpret_cast<unsigned long long*>(L.Bs + 64 * st);
  L.app = L.top + QT * kp;
  L.thr = L.app + QT * kTopkApp;
  L.eb = reinterpret_cast<long long*>(L.thr + QT);
  L.ee = L.eb + QT;
  L.cnt = reinterpret_cast<int*>(L.ee + QT);
  L.flg = L.cnt + QT;
  L.over = L.flg + QT;
  L.thrf = reinterpret_cast<float*>(L.over + 4);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, l16 = lane & 15;
  const int q0 = blockIdx.x * QT;
  const int split = blockIdx.y;
  const int dp4 = dp >> 2, u = dp >> 4;  // float4 per row; float4 per thread of a 64-row tile
  const int t_begin = split * a.tiles_per_split;
  const int t_end = min(t_begin + a.tiles_per_split, a.n_tiles);

  // this thread's float4 slots of a candidate tile: flat index tid + 256 i (coalesced), LDS offset
  int boff[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = tid + 256 * i;
    const int r = e / dp4;
    boff[i] = r * st + 4 * (e - r * dp4);
  }
  float4 pre[16];
  int mcur = 0, mnext = 0;  // this lane's candidate's mask byte, current and prefetched tile
  float pcur = 0.f, pnext = 0.f;  // (PRIOR) and its prior
  if (t_begin < t_end) {
    const float* src = a.cn + (size_t)t_begin * 64 * dp;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < u) pre[i] = ld4(src + 4 * (tid + 256 * i));
    const int c = t_begin * 64 + 16 * w + l16;
    mcur = c < a.nc ? (a.mask ? a.mask[c] : 1) : 0;
    if constexpr (PRIOR) pcur = c < a.nc ? a.prior[c] : 0.f;
  }
  for (int e = tid; e < QT * dp4; e += 256) {
    const int r = e / dp4, k4 = e - r * dp4;
    st4(&L.As[r * st + 4 * k4], ld4(a.qn + (size_t)(q0 + r) * dp + 4 * k4));
  }
  for (int e = tid; e < QT * kp; e += 256) L.top[e] = 0ull;
  if (tid < QT) {
    L.thr[tid] = 0ull;
    L.thrf[tid] = q0 + tid < a.nq ? -__builtin_inff() : __builtin_inff();
    L.cnt[tid] = 0;
    L.flg[tid] = 0;
    long long b = 0, e = 0;
    if (a.excl_ptr && q0 + tid < a.nq) {
      const int row = a.queries[q0 + tid];
      b = a.excl_ptr[row];
      e = a.excl_ptr[row + 1];
    }
    L.eb[tid] = b;
    L.ee[tid] = e;
  }
  if (tid == 0) *L.over = 0;

  const int kq = dp >> 2;  // k range per lane group
  for (int t = t_begin; t < t_end; ++t) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < u) st4(&L.Bs[boff[i]], pre[i]);
    __syncthreads();
    if (t + 1 < t_end) {
      const float* src = a.cn + (size_t)(t + 1) * 64 * dp;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < u) pre[i] = ld4(src + 4 * (tid + 256 * i));
      const int cn1 = (t + 1) * 64 + 16 * w + l16;
      mnext = cn1 < a.nc ? (a.mask ? a.mask[cn1] : 1) : 0;
      if constexpr (PRIOR) pnext = cn1 < a.nc ? a.prior[cn1] : 0.f;
    }
    f32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* brow = &L.Bs[(16 * w + l16) * st + g * kq];
    for (int j = 0; j < kq; j += 4) {
      const float4 b = ld4(brow + j);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const float4 x = ld4(&L.As[(16 * m + l16) * st + g * kq + j]);
        acc[m] = mfma4(x.x, b.x, acc[m]);
        acc[m] = mfma4(x.y, b.y, acc[m]);
        acc[m] = mfma4(x.z, b.z, acc[m]);
        acc[m] = mfma4(x.w, b.w, acc[m]);
      }
    }
    // selection: lane holds candidate c's scores for queries 16m + 4g + r. A finite score only needs
    // the (prefetched) mask byte and the threshold here; its exclusion test waits for the compaction.
    const int c = t * 64 + 16 * w + l16;
    const unsigned long long low = (unsigned)~(unsigned)c;
    unsigned pend = 0;
    float mag = 0.f;  // finite unless one of the lane's scores is NaN / inf
#pragma unroll
    for (int m = 0; m < MT; ++m) mag += (fabsf(acc[m][0]) + fabsf(acc[m][1])) + (fabsf(acc[m][2]) + fabsf(acc[m][3]));
    // (PRIOR) |s0| + |p| >= |s0 + p| and rounding is monotone: a NaN / inf sum makes mag NaN / inf
    if constexpr (PRIOR) mag += fabsf(pcur);
    const bool odd = !(mag < __builtin_inff());
    if (c < a.nc && (mcur || odd)) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const float4 tf = ld4(&L.thrf[16 * m + 4 * g]);
        const float tfr[4] = {tf.x, tf.y, tf.z, tf.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = acc[m][r] + 0.f;  // -0 -> +0: one key per value
          if constexpr (PRIOR) s = (s + pcur) + 0.f;
          if (odd && !(fabsf(s) < __builtin_inff())) {  // NaN / inf: flagged where the candidate is eligible
            const int ql = 16 * m + 4 * g + r;
            if (q0 + ql < a.nq && topk_eligible(a, L, c, ql)) {
              atomicOr(&L.flg[ql], 2);
              if (s == s) pend |= 1u << (4 * m + r);
            }
          } else if (mcur && s >= tfr[r]) {  // (equal scores: the key decides below)
            pend |= 1u << (4 * m + r);
          }
        }
      }
    }
    mcur = mnext;
    const float padd = pcur;  // (PRIOR) the pending scores' prior: this tile's
    if constexpr (PRIOR) pcur = pnext;
    for (;;) {
      for (unsigned p = pend; p;) {
        const int b = __ffs(p) - 1;
        p &= p - 1;
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (b == 4 * m + r) s = acc[m][r] + 0.f;
        if constexpr (PRIOR) s = (s + padd) + 0.f;
        const int ql = 16 * (b >> 2) + 4 * g + (b & 3);
        const unsigned long long key = ((unsigned long long)ord_key(s) << 32) | low;
        if (key > L.thr[ql]) {
          const int slot = atomicAdd(&L.cnt[ql], 1);
          if (slot < kTopkApp) {
            L.app[ql * kTopkApp + slot] = key;
            pend &= ~(1u << b);
          } else {
            L.cnt[ql] = kTopkApp;  // (every writer stores the same value)
            *L.over = 1;
          }
        } else {
          pend &= ~(1u << b);
        }
      }
      __syncthreads();
      const int ov = *L.over;
      __syncthreads();
      if (!ov) break;
      topk_compact<QT>(L, a.k, a.lkp, a.nq - q0, a.excl_ptr ? a.excl_idx : nullptr);
    }
  }
  __syncthreads();
  topk_compact<QT>(L, a.k, a.lkp, a.nq - q0, a.excl_ptr ? a.excl_idx : nullptr);
  for (int e = tid; e < QT * a.k; e += 256) {
    const int ql = e / a.k, j = e - ql * a.k;
    if (q0 + ql < a.nq) a.parts[((size_t)(q0 + ql) * a.S + split) * a.k + j] = L.top[(ql << a.lkp) + j];
  }
  if (tid < QT && q0 + tid < a.nq) a.pflags[(size_t)(q0 + tid) * a.S + split] = L.flg[tid];
}

// one workgroup per query of the batch
__global__ __launch_bounds__(256) void k_topk_merge(const unsigned long long* __restrict__ parts,
                                                    const int32_t* __restrict__ pflags, int S, int k, int q_offset,
                                                    int32_t* __restrict__ out_idx, float* __restrict__ out_score,
                                                    int32_t* __restrict__ out_count, int32_t* __restrict__ out_flags) {
  __shared__ uint64_t key[kTopkMaxSplit * DCUE_TOPK_MAX_K];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int n = S * k;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int e = tid; e < np2; e += 256) key[e] = e < n ? parts[(size_t)i * n + e] : 0ull;
  __syncthreads();
  block_bitonic_sort<true>(key, np2);  // descending
  const size_t o = (size_t)(q_offset + i) * k;
  for (int j = tid; j < k; j += 256) {
    const unsigned long long v = key[j];
    out_idx[o + j] = v ? (int32_t)~(unsigned)v : -1;
    out_score[o + j] = v ? ord_value((unsigned)(v >> 32)) : -__builtin_inff();
    if (v && (j == k - 1 || key[j + 1] == 0ull)) out_count[q_offset + i] = j + 1;
  }
  if (tid == 0) {
    if (key[0] == 0ull) out_count[q_offset + i] = 0;
    int f = 0;
    for (int s = 0; s < S; ++s) f |= pflags[(size_t)i * S + s];
    out_flags[q_offset + i] = f;
  }
}

static int topk_query_tile(int dp, int kp) { return topk_lds_bytes(dp, kp, 64) <= (size_t)kTopkLdsBudget ? 64 : 32; }

static int topk_auto_split(int nq) {
  const int tiles = (nq + 63) / 64;
  const int s = (kTopkFillWgs + tiles - 1) / tiles;
  return s < 1 ? 1 : s > kTopkMaxSplit ? kTopkMaxSplit : s;
}

struct TopkWs {
  float *cn, *qn;
  unsigned long long* parts;
  int32_t* pflags;
};

// part_rows: (query, split) pairs the partials hold
static size_t topk_carve(int64_t n_cand, int32_t d, int32_t qb, int32_t k, size_t part_rows, void* base,
                         TopkWs* w) {
  Arena ar{reinterpret_cast<char*>(base), 0, 0};
  const int dp = rank_dp(d);
  w->cn = ar.take<float>((size_t)((n_cand + 63) / 64 * 64) * dp);
  w->qn = ar.take<float>((size_t)((qb + 63) / 64 * 64) * dp);
  w->parts = ar.take<unsigned long long>(part_rows * k);
  w->pflags = ar.take<int32_t>(part_rows);
  return ar.used;
}

static int topk_check(int64_t n_cand, int32_t d, int32_t query_batch, int32_t k, int32_t cand_split) {
  if (k < 1 || k > DCUE_TOPK_MAX_K || n_cand < 1 || query_batch < 1 || cand_split < 0 || d <= 0)
    return DCUE_ERR_INVALID;
  if (d > 256 || n_cand > INT32_MAX - 64) return DCUE_ERR_UNSUPPORTED;
  return DCUE_OK;
}

// dcue_topk_scored (cand_prior null) and dcue_topk_prior
static int topk_run(int32_t score, const float* query_feat, int64_t n_query_rows, const float* cand_feat,
                    int64_t n_cand, int32_t d, const int32_t* queries, int32_t n_queries, const int64_t* excl_ptr,
                    const int32_t* excl_idx, const uint8_t* cand_mask, const float* cand_prior, int32_t k,
                    int32_t query_batch, int32_t cand_split, void* ws, size_t ws_bytes, int32_t* out_idx,
                    float* out_score, int32_t* out_count, int32_t* out_flags, void* stream) {
  if (score != DCUE_SCORE_COSINE && score != DCUE_SCORE_DOT) return DCUE_ERR_INVALID;
  // the prep pass of both sides: unit rows (cosine) or the raw rows (inner product), zero-padded to dp
  const auto prep = score == DCUE_SCORE_DOT ? launch_rank_pad : launch_rank_normalize;
  if (!query_feat || !cand_feat || !queries || !ws || !out_idx || !out_score || !out_count || !out_flags ||
      n_query_rows <= 0 || n_queries < 0 || (excl_ptr == nullptr) != (excl_idx == nullptr))
    return DCUE_ERR_INVALID;
  TRY(topk_check(n_cand, d, query_batch, k, cand_split));
  if (n_queries == 0) return DCUE_OK;
  const int qb = n_queries < query_batch ? n_queries : query_batch;
  const int dp = rank_dp(d);
  int lkp = 0;
  while ((1 << lkp) < k) ++lkp;
  const int qt = topk_query_tile(dp, 1 << lkp);
  const int n_tiles = (int)((n_cand + 63) / 64);
  int S = cand_split > 0 ? (cand_split < kTopkMaxSplit ? cand_split : kTopkMaxSplit) : topk_auto_split(qb);
  if (S > n_tiles) S = n_tiles;
  const int tiles_per_split = (n_tiles + S - 1) / S;
  TopkWs w;
  if (topk_carve(n_cand, d, qb, k, (size_t)qb * S, nullptr, &w) > ws_bytes) return DCUE_ERR_WORKSPACE;
  topk_carve(n_cand, d, qb, k, (size_t)qb * S, ws, &w);
  hipStream_t s = (hipStream_t)stream;
  static bool attr = false;
  if (!attr) {
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_topk_scores<4, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kTopkLdsBudget));
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_topk_scores<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kTopkLdsBudget));
    attr = true;
  }
  static bool attr_prior = false;
  if (cand_prior && !attr_prior) {
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_topk_scores<4, true>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kTopkLdsBudget));
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_topk_scores<2, true>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kTopkLdsBudget));
    attr_prior = true;
  }
  const size_t lds = topk_lds_bytes(dp, 1 << lkp, qt);
  // zero rows past the last candidate / query of a tile: the kernels load whole tiles
  const int64_t cand_pad = (int64_t)n_tiles * 64 - n_cand;
  if (cand_pad) DCUE_HIP_CHECK(hipMemsetAsync(w.cn + (size_t)n_cand * dp, 0, (size_t)cand_pad * dp * sizeof(float), s));
  TRY(prep(cand_feat, nullptr, n_cand, d, dp, w.cn, s));
  for (int32_t q0 = 0; q0 < n_queries; q0 += qb) {
    const int nq = n_queries - q0 < qb ? n_queries - q0 : qb;
    const int q_pad = (nq + 63) / 64 * 64 - nq;
    if (q_pad) DCUE_HIP_CHECK(hipMemsetAsync(w.qn + (size_t)nq * dp, 0, (size_t)q_pad * dp * sizeof(float), s));
    TRY(prep(query_feat, queries + q0, nq, d, dp, w.qn, s));
    TopkArgs a;
    a.qn = w.qn;
    a.nq = nq;
    a.cn = w.cn;
    a.nc = (int)n_cand;
    a.dp = dp;
    a.queries = queries + q0;
    a.excl_ptr = excl_ptr;
    a.excl_idx = excl_idx;
    a.mask = cand_mask;
    a.k = k;
    a.lkp = lkp;
    a.tiles_per_split = tiles_per_split;
    a.n_tiles = n_tiles;
    a.S = S;
    a.parts = w.parts;
    a.pflags = w.pflags;
    a.prior = cand_prior;
    const dim3 grid((unsigned)((nq + qt - 1) / qt), (unsigned)S);
    if (cand_prior) {
      if (qt == 64)
        DCUE_LAUNCH((k_topk_scores<4, true>), grid, dim3(256), lds, s, a);
      else
        DCUE_LAUNCH((k_topk_scores<2, true>), grid, dim3(256), lds, s, a);
    } else if (qt == 64) {
      DCUE_LAUNCH((k_topk_scores<4, false>), grid, dim3(256), lds, s, a);
    } else {
      DCUE_LAUNCH((k_topk_scores<2, false>), grid, dim3(256), lds, s, a);
    }
    DCUE_LAUNCH_CHECK();
    DCUE_LAUNCH(k_topk_merge, dim3((unsigned)nq), dim3(256), 0, s, (const unsigned long long*)w.parts,
                (const int32_t*)w.pflags, S, (int)k, (int)q0, out_idx, out_score, out_count, out_flags);
    DCUE_LAUNCH_CHECK();
  }
  DCUE_HIP_CHECK(hipStreamSynchronize(s));
  return DCUE_OK;
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_topk_workspace_bytes(int64_t n_cand, int32_t d, int32_t query_batch, int32_t k, int32_t cand_split,
                              size_t* bytes) {
  if (!bytes) return DCUE_ERR_INVALID;
  TRY(topk_check(n_cand, d, query_batch, k, cand_split));
  // auto: the split follows the number of queries of a pass (at most query_batch); q * split(q) is
  // below 64 * kTopkFillWgs + q + 64 and below 32 q
  const size_t qb = (size_t)query_batch;
  const size_t bound = (size_t)64 * kTopkFillWgs + qb + 64;
  const size_t rows = cand_split > 0 ? qb * (size_t)(cand_split < kTopkMaxSplit ? cand_split : kTopkMaxSplit)
                                     : (qb * kTopkMaxSplit < bound ? qb * kTopkMaxSplit : bound);
  TopkWs w;
  *bytes = topk_carve(n_cand, d, query_batch, k, rows, nullptr, &w);
  return DCUE_OK;
}

int dcue_topk_scored(int32_t score, const float* query_feat, int64_t n_query_rows, const float* cand_feat,
                     int64_t n_cand, int32_t d, const int32_t* queries, int32_t n_queries, const int64_t* excl_ptr,
                     const int32_t* excl_idx, const uint8_t* cand_mask, int32_t k, int32_t query_batch,
                     int32_t cand_split, void* ws, size_t ws_bytes, int32_t* out_idx, float* out_score,
                     int32_t* out_count, int32_t* out_flags, void* stream) {
  return topk_run(score, query_feat, n_query_rows, cand_feat, n_cand, d, queries, n_queries, excl_ptr, excl_idx,
                  cand_mask, nullptr, k, query_batch, cand_split, ws, ws_bytes, out_idx, out_score, out_count,
                  out_flags, stream);
}

int dcue_topk_prior(int32_t score, const float* query_feat, int64_t n_query_rows, const float* cand_feat,
                    int64_t n_cand, int32_t d, const int32_t* queries, int32_t n_queries, const int64_t* excl_ptr,
                    const int32_t* excl_idx, const uint8_t* cand_mask, const float* cand_prior, int32_t k,
                    int32_t query_batch, int32_t cand_split, void* ws, size_t ws_bytes, int32_t* out_idx,
                    float* out_score, int32_t* out_count, int32_t* out_flags, void* stream) {
  const int st = topk_run(score, query_feat, n_query_rows, cand_feat, n_cand, d, queries, n_queries, excl_ptr,
                          excl_idx, cand_mask, cand_prior, k, query_batch, cand_split, ws, ws_bytes, out_idx,
                          out_score, out_count, out_flags, stream);
  // (the refusals are host checks made before the first device call; a HIP failure keeps its own text)
  if (st == DCUE_ERR_INVALID)
    set_last_message("dcue_topk_prior: a null required pointer, an unknown score, excl_ptr without excl_idx or the "
                     "reverse, or k / n_cand / d / query_batch / cand_split / a count out of range");
  else if (st == DCUE_ERR_UNSUPPORTED)
    set_last_message("dcue_topk_prior: d above 256 or n_cand beyond dcue_topk's bound");
  else if (st == DCUE_ERR_WORKSPACE)
    set_last_message("dcue_topk_prior: the workspace is smaller than dcue_topk_workspace_bytes says");
  return st;
}

int dcue_topk(const float* query_feat, int64_t n_query_rows, const float* cand_feat, int64_t n_cand, int32_t d,
              const int32_t* queries, int32_t n_queries, const int64_t* excl_ptr, const int32_t* excl_idx,
              const uint8_t* cand_mask, int32_t k, int32_t query_batch, int32_t cand_split, void* ws,
              size_t ws_bytes, int32_t* out_idx, float* out_score, int32_t* out_count, int32_t* out_flags,
              void* stream) {
  return dcue_topk_scored(DCUE_SCORE_COSINE, query_feat, n_query_rows, cand_feat, n_cand, d, queries, n_queries,
                          excl_ptr, excl_idx, cand_mask, k, query_batch, cand_split, ws, ws_bytes, out_idx,
                          out_score, out_count, out_flags, stream);
}

}  // extern "C"
