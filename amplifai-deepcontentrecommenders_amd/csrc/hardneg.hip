// Hard negatives: dcue_select_negatives (include/dcue.h has the contract).
//
// Out of a pool of P sampled candidates per row, keep the H the current factors score highest for the
// row's user and fill the row up to N with the pool's leading other draws. One workgroup per row:
//   A  the row's pool ids -> LDS;
//   B  the cosines: a 16-lane group per candidate, kSelAhead candidates in flight per group, lane l of
//      the group over elements l, l + 16, ... in ascending order (fmaf), then a 16-lane xor butterfly.
//      The order depends on d alone, so a score is a function of the two rows' values: the same bits
//      whatever the position, the row, P or the batch, and an exact tie between equal item rows;
//   C  first occurrences, by a scan of the ids before each position, and the 64-bit keys
//      (score descending, position ascending) of the eligible positions;
//   D  each position's rank among the keys, by counting: hard = eligible and rank < H;
//   E  compaction in pool order by ballot + prefix: the hard ids, then the first N - h others.
// Steps C and D read every LDS word as a broadcast, P words per thread. No scratch, no workspace, no
// transcendental beyond sqrt and divide; the call never waits for its stream.
//
// Every float multiply feeding a float add is an explicit fmaf (tgemm.h's rule), so the scores do not
// depend on -ffp-contract.
#include "dcue_internal.h"

namespace dcue {

constexpr int kSelThreads = 256;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelLanes = 16;                       // lanes per candidate
constexpr int kSelGroups = kSelThreads / kSelLanes;
constexpr int kSelAhead = 4;                        // candidates of one group in flight together
constexpr int kSelMaxPool = DCUE_SELECT_MAX_POOL;
constexpr int kSelPer = kSelMaxPool / kSelThreads;  // positions per thread in steps C to E
constexpr float kSelEps = 1e-8f;                    // nn.CosineSimilarity's eps

static_assert(kSelPer * kSelThreads == kSelMaxPool, "every pool position has a thread slot");

struct SelectArgs {
  const float* user_feat;
  const float* item_feat;
  const int64_t* users;
  const int64_t* pool;
  int64_t* out;
  int32_t* out_hard;
  int32_t* out_flags;
  int64_t n_users, n_items;
  int d, P, N, H;
};

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = kSelLanes / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kSelLanes);
  return v;
}

// float bits -> unsigned, monotonic over the non-NaN floats; at least 0x007fffff (-inf), never 0
__device__ __forceinline__ uint32_t score_order(float s) {
  const uint32_t b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// NK = the elements per lane: d <= 16 * NK. Elements past d count as zeros.
template <int NK>
__global__ __launch_bounds__(kSelThreads) void k_select_negatives(SelectArgs a) {
  __shared__ int64_t s_id[kSelMaxPool];
  __shared__ uint64_t s_key[kSelMaxPool];
  __shared__ float s_score[kSelMaxPool];
  __shared__ int s_wcnt[kSelPer * kSelWaves];
  __shared__ int s_flags;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t b = blockIdx.x;
  const int d = a.d, P = a.P, N = a.N;
  const int64_t* pool = a.pool + b * P;
  int64_t* out = a.out + b * N;
  const int64_t u = a.users[b];
  if (u < 0 || u >= a.n_users) {  // no row to score against: the plain draws
    for (int j = t; j < N; j += kSelThreads) out[j] = pool[j];
    if (t == 0) {
      a.out_hard[b] = 0;
      a.out_flags[b] = DCUE_SELECT_FLAG_BAD_ID;
    }
    return;
  }

  // ---- A
  if (t == 0) s_flags = 0;
  if (t < kSelPer * kSelWaves) s_wcnt[t] = 0;
  for (int p = t; p < P; p += kSelThreads) s_id[p] = pool[p];
  __syncthreads();

  // ---- B
  {
    const int sub = t & (kSelLanes - 1), grp = t / kSelLanes;
    const float* urow = a.user_feat + u * d;
    float uv[NK];
    float uu = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int e = k * kSelLanes + sub;
      const float v = urow[e < d ? e : d - 1];
      uv[k] = e < d ? v : 0.f;
      uu = fmaf(uv[k], uv[k], uu);
    }
    const float un = fmaxf(sqrtf(group_sum(uu)), kSelEps);
    for (int p0 = grp * kSelAhead; p0 < P; p0 += kSelGroups * kSelAhead) {
      float cv[kSelAhead][NK];
      bool ok[kSelAhead];
#pragma unroll
      for (int j = 0; j < kSelAhead; ++j) {
        const int p = p0 + j;
        const int64_t id = s_id[p < P ? p : P - 1];
        ok[j] = p < P && id >= 0 && id < a.n_items;
        const float* crow = a.item_feat + (ok[j] ? id : 0) * d;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const int e = k * kSelLanes + sub;
          cv[j][k] = ok[j] ? crow[e < d ? e : d - 1] : 0.f;  // an id outside the table addresses nothing
        }
      }
#pragma unroll
      for (int j = 0; j < kSelAhead; ++j) {
        float dot = 0.f, cc = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const float c = k * kSelLanes + sub < d ? cv[j][k] : 0.f;
          dot = fmaf(uv[k], c, dot);
          cc = fmaf(c, c, cc);
        }
        dot = group_sum(dot);
        cc = group_sum(cc);
        float s = dot / (un * fmaxf(sqrtf(cc), kSelEps));
        if (s == 0.f) s = 0.f;  // -0 and +0 are one score
        if (sub == 0 && ok[j]) s_score[p0 + j] = s;
      }
    }
  }
  __syncthreads();

  // ---- C
  int64_t id[kSelPer];
  uint64_t key[kSelPer];
  bool first[kSelPer];
#pragma unroll
  for (int i = 0; i < kSelPer; ++i) {
    const int p = t + i * kSelThreads;
    id[i] = p < P ? s_id[p] : -1;
    first[i] = true;
  }
  for (int q = 0; q < P; ++q) {
    const int64_t v = s_id[q];
#pragma unroll
    for (int i = 0; i < kSelPer; ++i)
      if (q < t + i * kSelThreads && v == id[i]) first[i] = false;
  }
  int flags = 0;
#pragma unroll
  for (int i = 0; i < kSelPer; ++i) {
    const int p = t + i * kSelThreads;
    key[i] = 0;
    if (p < P) {
      if (id[i] < 0 || id[i] >= a.n_items) {
        flags |= DCUE_SELECT_FLAG_BAD_ID;
      } else {
        const float s = s_score[p];
        if (s != s || fabsf(s) == INFINITY) flags |= DCUE_SELECT_FLAG_NONFINITE;
        if (first[i] && s == s) key[i] = ((uint64_t)score_order(s) << 32) | (uint32_t)(kSelMaxPool - p);
      }
      s_key[p] = key[i];
    }
  }
  if (flags) atomicOr(&s_flags, flags);
  __syncthreads();

  // ---- D
  int rank[kSelPer];
#pragma unroll
  for (int i = 0; i < kSelPer; ++i) rank[i] = 0;
  for (int q = 0; q < P; ++q) {
    const uint64_t v = s_key[q];
#pragma unroll
    for (int i = 0; i < kSelPer; ++i) rank[i] += v > key[i] ? 1 : 0;
  }

  // ---- E
  bool hard[kSelPer];
  int before[kSelPer];  // hard positions ahead of this one inside its wave's 64
#pragma unroll
  for (int i = 0; i < kSelPer; ++i) {
    hard[i] = key[i] != 0 && rank[i] < a.H;
    const unsigned long long m = __ballot(hard[i]);
    before[i] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcnt[i * kSelWaves + wave] = __popcll(m);
  }
  __syncthreads();
  int h = 0;
  int base[kSelPer];
#pragma unroll
  for (int i = 0; i < kSelPer; ++i) {
#pragma unroll
    for (int w = 0; w < kSelWaves; ++w) {
      if (w == wave) base[i] = h;
      h += s_wcnt[i * kSelWaves + w];
    }
  }
#pragma unroll
  for (int i = 0; i < kSelPer; ++i) {
    const int p = t + i * kSelThreads;
    if (p >= P) continue;
    const int hb = base[i] + before[i];
    if (hard[i]) {
      out[hb] = id[i];
    } else if (p - hb < N - h) {
      out[h + p - hb] = id[i];
    }
  }
  if (t == 0) {
    a.out_hard[b] = h;
    a.out_flags[b] = s_flags;
  }
}

}  // namespace dcue

using namespace dcue;

extern "C" int dcue_select_negatives(const float* user_feat, int64_t n_users, const float* item_feat,
                                     int64_t n_items, int32_t d, const int64_t* users, const int64_t* pool,
                                     int32_t n_samples, int32_t P, int32_t N, int32_t H, int64_t* out,
                                     int32_t* out_hard, int32_t* out_flags, void* stream) {
  if (!user_feat || !item_feat || !users || !pool || !out || !out_hard || !out_flags) return DCUE_ERR_INVALID;
  if (n_users < 0 || n_items < 0 || d < 1 || n_samples < 0) return DCUE_ERR_INVALID;
  if (N < 1 || P < N || P > DCUE_SELECT_MAX_POOL || H < 0 || H > N) return DCUE_ERR_INVALID;
  if (d > 256) return DCUE_ERR_UNSUPPORTED;
  if (n_samples == 0) return DCUE_OK;
  const SelectArgs a = {user_feat, item_feat, users, pool, out, out_hard, out_flags, n_users, n_items, d, P, N, H};
  const dim3 grid((unsigned)n_samples), block(kSelThreads);
  const hipStream_t s = (hipStream_t)stream;
  if (d <= 32)
    DCUE_LAUNCH(k_select_negatives<2>, grid, block, 0, s, a);
  else if (d <= 64)
    DCUE_LAUNCH(k_select_negatives<4>, grid, block, 0, s, a);
  else if (d <= 128)
    DCUE_LAUNCH(k_select_negatives<8>, grid, block, 0, s, a);
  else
    DCUE_LAUNCH(k_select_negatives<16>, grid, block, 0, s, a);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}
