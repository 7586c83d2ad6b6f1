// Fold-in of unseen users (include/dcue.h dcue_user_foldin): with the model frozen,
// one fresh embedding row per new user is learned against the trained towers with the training loss
// itself (cosine hinge, N sampled negatives per positive) and Adam on that row alone. New users do
// not depend on each other, so a workgroup keeps a tile of 16 users (tgemm's row block) for ALL steps
// of one launch: no host round trip between steps, no [users][candidates] matrix, no gathered copies
// of factor rows.
//
//   k_rank_normalize    (rank.hip) the candidates x / max(||x||, 1e-8), zero-padded to DP, once per call
//   k_foldin            1024 threads = 16 waves per tile. Per step:
//                         GEMM 1/2  h1 = relu(e) W1^T + b1, uf = relu(h1) W2^T + b2 on
//                                   v_mfma_f32_16x16x4_f32: the activations are the A operand (LDS), the
//                                   weights stream from L2 straight into the B registers (a lane reads
//                                   a contiguous quarter of one weight row); a wave owns 16 columns
//                         score     wave w owns user w: the step's positives in turn, each with its N
//                                   negatives drawn on the spot (splitmix64, rejection against the mask
//                                   and the history held in LDS), their normalised rows read once, eight
//                                   at a time, and kept in registers from the cosines to the weighted sum
//                         GEMM 3/4  d h1 = (d uf W2) [h1 > 0], d e = (d h1 W1) [e > 0]
//                         Adam      adam_elem on e, m, v (adam_replay.h: the trainer's element update)
//                       then the tower of the final rows. A user's arithmetic does not depend on which
//                       users share its tile or its call: results are bit-identical under any batching.
//   k_foldin_negatives  the sampler alone (tests, and the torch comparison of profiles/foldin_bench.py)
// e, m, v, h1 and d h1 live in LDS where E allows (tier 0: E <= 384 at d_s = 256 .. 432 at d_s = 32), m
// and v in the workspace up to E <= 656 .. 720 (tier 1), all five in the workspace beyond (tier 2,
// E <= 1024): a workgroup's slice is written and read by its own waves only, ordered by the block barrier.
// This file is compiled with -ffp-contract=off (Makefile), as adam.hip is.
#include <vector>

#include "dcue_internal.h"
#include "bn0adam.h"
#include "mix64.h"

namespace dcue {

constexpr int kFiThreads = 1024;
constexpr int kFiWaves = kFiThreads / 64;
constexpr int kFiTile = 16;              // users per workgroup
constexpr int kFiHist = 256;             // history entries per user held in LDS (longer ones: global)
constexpr int kFiLdsBudget = 156 * 1024; // one workgroup per CU; 4 KB left for the static arrays
constexpr int kFiMaxSteps = 4096, kFiMaxNeg = 256, kFiMaxPos = 1024;

__host__ __device__ constexpr int fi_pad16(int v) { return (v + 15) & ~15; }
__host__ __device__ constexpr int fi_pitch(int v) { return fi_pad16(v) + 4; }
__host__ __device__ constexpr size_t fi_act_floats(int E) { return (size_t)kFiTile * fi_pitch(E); }
__host__ __device__ constexpr size_t fi_lds_bytes(int E, int D, int tier) {
  return ((size_t)kFiTile * fi_pitch(D) + (size_t)kFiTile * kFiHist + (tier == 0 ? 5 : tier == 1 ? 3 : 0) * fi_act_floats(E)) * 4;
}
static int fi_tier(int E, int D) {
  return fi_lds_bytes(E, D, 0) <= (size_t)kFiLdsBudget ? 0 : fi_lds_bytes(E, D, 1) <= (size_t)kFiLdsBudget ? 1 : 2;
}
static int fi_ws_acts(int tier) { return tier == 0 ? 0 : tier == 1 ? 2 : 5; }

__host__ __device__ __forceinline__ unsigned long long fi_mix(unsigned long long z) { return mix64(z); }
__host__ __device__ __forceinline__ unsigned long long fi_row_key(unsigned long long seed, long long r) {
  return fi_mix(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(r + 1));
}

// negative (t, i, j) of the row with key z0: the first of eight draws the mask admits and the sorted
// history H[0 .. hlen) does not hold; -1 when all eight are rejected
__device__ __forceinline__ int fi_sample(unsigned long long z0, int t, int i, int j, unsigned long long n_cand,
                                         const uint8_t* __restrict__ mask, const int32_t* H, int hlen) {
  const unsigned long long base = ((unsigned long long)t << 40) | ((unsigned long long)i << 24) | ((unsigned long long)j << 8);
  for (int a = 0; a < 8; ++a) {
    const unsigned long long x = fi_mix(z0 ^ (base | (unsigned long long)a));
    const int c = (int)(((x >> 32) * n_cand) >> 32);
    if (mask && !mask[c]) continue;
    int lo = 0, hi = hlen;
    bool found = false;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const int v = H[mid];
      if (v == c) { found = true; break; }
      if (v < c) lo = mid + 1; else hi = mid;
    }
    if (!found) return c;
  }
  return -1;
}

struct FoldArgs {
  const float *W1, *b1, *W2, *b2;  // the user tower (read only)
  int E, D, d, dp;                 // D: storage width of d (rows of W2; zero past d)
  const float* cn;                 // [n_cand][dp] normalised candidates
  long long n_cand;
  const uint8_t* mask;
  const int64_t* hist_ptr;
  const int32_t* hist_idx;
  int n_users;
  long long row0;
  int steps, n_neg, max_pos;
  float margin;
  unsigned long long seed;
  const AdamScalars* sc;  // [steps]
  float *emb, *out_feat, *out_loss, *out_grad;
  int32_t* out_flags;
  float* act;  // tiers 1 / 2: [tiles][2 or 5][16][pitch(E)]
};

// C[16][N] = relu(A)[16][K] W^T + bias, W row-major [N][K]. A: zero past K up to pad16(K). Lane group g
// owns k = g * pad16(K)/4 + j: it reads a contiguous quarter of W's row n0 + l16.
__device__ __forceinline__ void fi_gemm_nt(const float* A, int lda, int K, const float* __restrict__ W, int N,
                                           const float* __restrict__ bias, float* C, int ldc, int wave, int lane) {
  const int l16 = lane & 15, g = lane >> 4;
  const int kq = fi_pad16(K) >> 2;
  const bool vec = (K & 3) == 0;
  for (int n0 = 16 * wave; n0 < N; n0 += 16 * kFiWaves) {
    const int n = n0 + l16, nc = min(n, N - 1);
    const float* wr = W + (size_t)nc * K;
    const float* ar = A + l16 * lda + g * kq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < kq; j += 4) {
      const int k = g * kq + j;
      float4 b;
      if (vec) {
        b = k < K ? ld4(wr + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        b.x = k < K ? wr[k] : 0.f;
        b.y = k + 1 < K ? wr[k + 1] : 0.f;
        b.z = k + 2 < K ? wr[k + 2] : 0.f;
        b.w = k + 3 < K ? wr[k + 3] : 0.f;
      }
      const float4 a = ld4(ar + j);
      acc = mfma4(fmaxf(a.x, 0.f), b.x, acc);
      acc = mfma4(fmaxf(a.y, 0.f), b.y, acc);
      acc = mfma4(fmaxf(a.z, 0.f), b.z, acc);
      acc = mfma4(fmaxf(a.w, 0.f), b.w, acc);
    }
    if (n < N) {
      const float bn = bias[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) C[(4 * g + r) * ldc + n] = acc[r] + bn;
    }
  }
}

// C[16][K] = (A[16][R] W) [mask > 0], W row-major [R][K]. A: zero past R up to pad16(R). Lane group g
// owns the reduction rows g * pad16(R)/4 + j; the 16 lanes of a group read 16 consecutive columns.
__device__ __forceinline__ void fi_gemm_nn(const float* A, int lda, int R, const float* __restrict__ W, int K,
                                           const float* M, int ldm, float* C, int ldc, int wave, int lane) {
  const int l16 = lane & 15, g = lane >> 4;
  const int rq = fi_pad16(R) >> 2;
  for (int k0 = 16 * wave; k0 < K; k0 += 16 * kFiWaves) {
    const int k = k0 + l16, kc = min(k, K - 1);
    const float* ar = A + l16 * lda + g * rq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < rq; j += 4) {
      const int r = g * rq + j;
      float b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float w = W[(size_t)min(r + i, R - 1) * K + kc];
        b[i] = r + i < R ? w : 0.f;
      }
      const float4 a = ld4(ar + j);
      acc = mfma4(a.x, b[0], acc);
      acc = mfma4(a.y, b[1], acc);
      acc = mfma4(a.z, b[2], acc);
      acc = mfma4(a.w, b[3], acc);
    }
    if (k < K) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        C[row * ldc + k] = M[row * ldm + k] > 0.f ? acc[r] : 0.f;
      }
    }
  }
}

template <int TIER>
__global__ __launch_bounds__(kFiThreads) void k_foldin(FoldArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ long long hbeg_s[kFiTile];
  __shared__ int hlen_s[kFiTile], flag_s[kFiTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, D = a.D, EP = fi_pitch(E), DU = fi_pitch(D);
  const size_t AB = fi_act_floats(E);
  float* uf = lds;
  int32_t* hist_l = reinterpret_cast<int32_t*>(uf + kFiTile * DU);
  float* lact = reinterpret_cast<float*>(hist_l + kFiTile * kFiHist);
  float *e, *h1, *gh, *m, *v;
  if constexpr (TIER == 0) {
    e = lact; h1 = lact + AB; gh = lact + 2 * AB; m = lact + 3 * AB; v = lact + 4 * AB;
  } else if constexpr (TIER == 1) {
    e = lact; h1 = lact + AB; gh = lact + 2 * AB;
    m = a.act + (size_t)blockIdx.x * 2 * AB; v = m + AB;
  } else {
    e = a.act + (size_t)blockIdx.x * 5 * AB; h1 = e + AB; gh = e + 2 * AB; m = e + 3 * AB; v = e + 4 * AB;
  }
  const int u0 = blockIdx.x * kFiTile;
  const int nr = min(kFiTile, a.n_users - u0);

  if (tid < kFiTile) {
    long long b = 0;
    int len = 0;
    if (tid < nr) {
      b = a.hist_ptr[a.row0 + u0 + tid];
      const long long en = a.hist_ptr[a.row0 + u0 + tid + 1];
      len = (int)(en - b);
    }
    hbeg_s[tid] = b;
    hlen_s[tid] = len;
    flag_s[tid] = (tid < nr && len <= 0) ? 1 : 0;
  }
  for (size_t i = tid; i < AB; i += kFiThreads) {
    e[i] = 0.f; h1[i] = 0.f; gh[i] = 0.f; m[i] = 0.f; v[i] = 0.f;
  }
  for (int i = tid; i < kFiTile * DU; i += kFiThreads) uf[i] = 0.f;
  __syncthreads();
  for (int i = tid; i < nr * E; i += kFiThreads) {
    const int r = i / E, k = i - r * E;
    e[r * EP + k] = a.emb[(size_t)(u0 + r) * E + k];
  }
  // wave w owns user w in the score phase: its history (if it fits) into LDS
  const int hlen = hlen_s[wave] > 0 ? hlen_s[wave] : 0;
  const bool active = wave < nr && hlen > 0;
  const int32_t* H = a.hist_idx + hbeg_s[wave];
  if (active && hlen <= kFiHist) {
    for (int i = lane; i < hlen; i += 64) hist_l[wave * kFiHist + i] = H[i];
    H = hist_l + wave * kFiHist;
  }
  const unsigned long long z0 = fi_row_key(a.seed, a.row0 + u0 + wave);
  const int P = min(hlen, a.max_pos);
  const int N = a.n_neg, dp = a.dp, d = a.d;
  int wflags = 0;
  __syncthreads();

  for (int t = 0; t <= a.steps; ++t) {
    fi_gemm_nt(e, EP, E, a.W1, E, a.b1, h1, EP, wave, lane);
    __syncthreads();
    fi_gemm_nt(h1, EP, E, a.W2, D, a.b2, uf, DU, wave, lane);
    __syncthreads();
    if (t == a.steps) break;
    // ---- score: loss of step t and d loss / d uf of this wave's user, written over uf
    {
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      float loss = 0.f;
      if (active) {
        float u[4], un[4];
        float su = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = lane + 64 * q;
          u[q] = k < d ? uf[wave * DU + k] : 0.f;
          su += u[q] * u[q];
        }
        const float du = fmaxf(sqrtf(wave_sum(su)), 1e-8f);
#pragma unroll
        for (int q = 0; q < 4; ++q) un[q] = u[q] / du;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        float sc = 0.f;  // sum of weight * cosine (negatives +, positives -)
        for (int i = 0; i < P; ++i) {
          const int pi = H[(int)(((long long)t * a.max_pos + i) % hlen)];
          if ((unsigned long long)pi >= (unsigned long long)a.n_cand) {  // not a candidate: no row to read
            wflags |= 2;
            continue;
          }
          float xp[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int k = lane + 64 * q;
            xp[q] = k < dp ? a.cn[(size_t)pi * dp + k] : 0.f;
          }
          float dpos = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q) dpos += un[q] * xp[q];
          const float cpos = wave_sum(dpos);
          float wpos = 0.f, li = 0.f;
          for (int jb = 0; jb < N; jb += 64) {
            const int cnt = min(64, N - jb);
            int mine = -1;
            if (lane < cnt) {
              mine = fi_sample(z0, t, i, jb + lane, (unsigned long long)a.n_cand, a.mask, H, hlen);
              if (mine < 0) wflags |= 4;
            }
            for (int c0 = 0; c0 < cnt; c0 += 8) {
              int ci[8];
              float x[8][4], dot[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                const int idx = __shfl(mine, (c0 + q) & 63, 64);
                ci[q] = c0 + q < cnt ? idx : -1;
              }
#pragma unroll
              for (int q = 0; q < 8; ++q)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                  const int k = lane + 64 * s;
                  x[q][s] = (ci[q] >= 0 && k < dp) ? a.cn[(size_t)ci[q] * dp + k] : 0.f;
                }
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) s += un[r] * x[q][r];
                dot[q] = s;
              }
#pragma unroll
              for (int off = 32; off > 0; off >>= 1)
#pragma unroll
                for (int q = 0; q < 8; ++q) dot[q] += __shfl_xor(dot[q], off, 64);
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                if (ci[q] < 0) continue;
                const float h = a.margin - (cpos - dot[q]);
                const float w = h > 0.f ? 1.f : (h == 0.f ? 0.5f : 0.f);  // a tie passes half, as the trainer
                li += h > 0.f ? h : (h == h ? 0.f : h);
                sc += w * dot[q];
                wpos += w;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] += w * x[q][r];
              }
            }
          }
          sc -= wpos * cpos;
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] -= wpos * xp[r];
          loss += li;
        }
        // d cos / d uf = (c^ - cos u^) / |uf|, mean over the P positives
        const float invp = 1.f / (float)P;
        const float scale = invp / du;
        loss *= invp;
#pragma unroll
        for (int r = 0; r < 4; ++r) g[r] = (acc[r] - un[r] * sc) * scale;
        if (!(fabsf(loss) < __builtin_inff())) wflags |= 2;
      }
      if (wave < nr) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = lane + 64 * q;
          if (k < D) uf[wave * DU + k] = k < d ? g[q] : 0.f;
        }
        if (lane == 0 && a.out_loss) a.out_loss[(size_t)(u0 + wave) * a.steps + t] = loss;
      }
    }
    __syncthreads();
    fi_gemm_nn(uf, DU, D, a.W2, E, h1, EP, gh, EP, wave, lane);
    __syncthreads();
    fi_gemm_nn(gh, EP, E, a.W1, E, e, EP, h1, EP, wave, lane);  // d e into the h1 buffer
    __syncthreads();
    {
      const AdamScalars s = a.sc[t];
      const bool last = a.out_grad && t == a.steps - 1;
      for (int i = tid; i < nr * E; i += kFiThreads) {
        const int r = i / E, k = i - r * E;
        const bool on = hlen_s[r] > 0;
        const float ge = on ? h1[r * EP + k] : 0.f;
        if (last) a.out_grad[(size_t)(u0 + r) * E + k] = ge;
        if (on) {
          float pp = e[r * EP + k], mm = m[r * EP + k], vv = v[r * EP + k];
          adam_elem(pp, ge, mm, vv, s);
          e[r * EP + k] = pp; m[r * EP + k] = mm; v[r * EP + k] = vv;
        }
      }
    }
    __syncthreads();
  }
  // uf = tower(final e)
  for (int i = tid; i < nr * E; i += kFiThreads) {
    const int r = i / E, k = i - r * E;
    if (hlen_s[r] > 0) a.emb[(size_t)(u0 + r) * E + k] = e[r * EP + k];
  }
  if (wave < nr) {
    float mag = 0.f;
    for (int k = lane; k < d; k += 64) {
      const float f = uf[wave * DU + k];
      a.out_feat[(size_t)(u0 + wave) * d + k] = f;
      mag += fabsf(f);
    }
    mag = wave_sum(mag);
    if (!(mag < __builtin_inff())) wflags |= 2;
    wflags |= __shfl_xor(wflags, 32, 64);
    wflags |= __shfl_xor(wflags, 16, 64);
    wflags |= __shfl_xor(wflags, 8, 64);
    wflags |= __shfl_xor(wflags, 4, 64);
    wflags |= __shfl_xor(wflags, 2, 64);
    wflags |= __shfl_xor(wflags, 1, 64);
    if (lane == 0) a.out_flags[u0 + wave] = flag_s[wave] | wflags;
  }
}

// out[u][i][j] for i < max_pos, j < n_neg: the step's negative, -1 for a dropped slot or i >= P
__global__ __launch_bounds__(256) void k_foldin_negatives(long long n_cand, const uint8_t* __restrict__ mask,
                                                          const int64_t* __restrict__ hist_ptr,
                                                          const int32_t* __restrict__ hist_idx, long long row0,
                                                          int max_pos, int n_neg, unsigned long long seed, int step,
                                                          int32_t* __restrict__ out) {
  const long long r = row0 + blockIdx.x;
  const long long hb = hist_ptr[r];
  const long long hl = hist_ptr[r + 1] - hb;
  const int hlen = hl > 0 ? (int)hl : 0;
  const int P = min(hlen, max_pos);
  const unsigned long long z0 = fi_row_key(seed, r);
  const int tot = max_pos * n_neg;
  for (int e = threadIdx.x; e < tot; e += 256) {
    const int i = e / n_neg, j = e - i * n_neg;
    out[(size_t)blockIdx.x * tot + e] =
        i < P ? fi_sample(z0, step, i, j, (unsigned long long)n_cand, mask, hist_idx + hb, hlen) : -1;
  }
}

struct FoldWs {
  float* cn;
  AdamScalars* sc;
  float* act;
};

static size_t foldin_carve(int E, int D, int d, int64_t n_cand, int32_t n_users, void* base, FoldWs* w) {
  Arena ar{reinterpret_cast<char*>(base), 0, 0};
  w->cn = ar.take<float>((size_t)n_cand * rank_dp(d));
  w->sc = ar.take<AdamScalars>(kFiMaxSteps);
  const size_t tiles = ((size_t)n_users + kFiTile - 1) / kFiTile;
  w->act = ar.take<float>(tiles * fi_ws_acts(fi_tier(E, D)) * fi_act_floats(E));
  return ar.used;
}

static int foldin_check_sampling(int64_t n_cand, int32_t n_users, int64_t row0, int32_t n_neg, int32_t max_pos) {
  if (n_cand <= 0 || n_users < 0 || row0 < 0 || n_neg < 1 || n_neg > kFiMaxNeg || max_pos < 1 || max_pos > kFiMaxPos)
    return DCUE_ERR_INVALID;
  if (n_cand > INT32_MAX - 64) return DCUE_ERR_UNSUPPORTED;
  return DCUE_OK;
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_foldin_workspace_bytes(const dcue_dims* dims, int64_t n_cand, int32_t n_users, int32_t max_pos,
                                int32_t n_neg, size_t* bytes_host) {
  if (!dims || !bytes_host) return DCUE_ERR_INVALID;
  int64_t poff[DCUE_N_DENSE_SEGMENTS + 1];
  TRY(dcue_param_layout(dims, poff));  // (the dims' own checks: d > 256, E > 1024 unsupported)
  TRY(foldin_check_sampling(n_cand, n_users, 0, n_neg, max_pos));
  FoldWs w;
  *bytes_host = foldin_carve(dims->user_embdim, st_feature(dims), dims->feature_dim, n_cand, n_users, nullptr, &w);
  return DCUE_OK;
}

int dcue_user_foldin(const dcue_model* m, const float* cand_feat, int64_t n_cand, const uint8_t* cand_mask,
                     const int64_t* hist_ptr, const int32_t* hist_idx, int32_t n_users, int64_t row0,
                     const dcue_foldin_config* cfg, float* emb, void* ws, size_t ws_bytes, float* out_feat,
                     float* out_loss, float* out_grad, int32_t* out_flags, void* stream) {
  if (!m || !cand_feat || !hist_ptr || !hist_idx || !cfg || !emb || !ws || !out_feat || !out_flags || !m->params)
    return DCUE_ERR_INVALID;
  if (cfg->steps < 0 || cfg->steps > kFiMaxSteps) return DCUE_ERR_INVALID;
  TRY(foldin_check_sampling(n_cand, n_users, row0, cfg->n_neg, cfg->max_pos));
  int64_t poff[DCUE_N_DENSE_SEGMENTS + 1];
  TRY(dcue_param_layout(&m->dims, poff));
  if (n_users == 0) return DCUE_OK;
  const int E = m->dims.user_embdim, D = st_feature(&m->dims), d = m->dims.feature_dim;
  FoldWs w;
  if (foldin_carve(E, D, d, n_cand, n_users, nullptr, &w) > ws_bytes) return DCUE_ERR_WORKSPACE;
  foldin_carve(E, D, d, n_cand, n_users, ws, &w);
  hipStream_t s = (hipStream_t)stream;
  TRY(join_user_stream(s));  // a plan's last Adam step may still be writing the tower's parameters
  const int tier = fi_tier(E, D);
  static bool attr = false;
  if (!attr) {
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_foldin<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kFiLdsBudget));
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_foldin<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kFiLdsBudget));
    DCUE_HIP_CHECK(hipFuncSetAttribute((const void*)k_foldin<2>, hipFuncAttributeMaxDynamicSharedMemorySize, kFiLdsBudget));
    attr = true;
  }
  // per-step scalars as torch.optim.Adam forms them (step count t + 1, constant lr)
  std::vector<AdamScalars> sc((size_t)cfg->steps);
  for (int t = 0; t < cfg->steps; ++t) {
    dcue_adam_args aa = {};
    aa.lr = cfg->lr; aa.beta1 = cfg->beta1; aa.beta2 = cfg->beta2; aa.eps = cfg->eps;
    aa.weight_decay = cfg->weight_decay;
    aa.step = t + 1;
    sc[(size_t)t] = form_scalars(&aa);
  }
  if (cfg->steps)
    DCUE_HIP_CHECK(hipMemcpyAsync(w.sc, sc.data(), sizeof(AdamScalars) * (size_t)cfg->steps, hipMemcpyHostToDevice, s));
  const int dp = rank_dp(d);
  TRY(launch_rank_normalize(cand_feat, nullptr, n_cand, d, dp, w.cn, s));
  FoldArgs a;
  a.W1 = m->params + poff[SEG_L1_W]; a.b1 = m->params + poff[SEG_L1_B];
  a.W2 = m->params + poff[SEG_L2_W]; a.b2 = m->params + poff[SEG_L2_B];
  a.E = E; a.D = D; a.d = d; a.dp = dp;
  a.cn = w.cn; a.n_cand = n_cand; a.mask = cand_mask;
  a.hist_ptr = hist_ptr; a.hist_idx = hist_idx;
  a.n_users = n_users; a.row0 = row0;
  a.steps = cfg->steps; a.n_neg = cfg->n_neg; a.max_pos = cfg->max_pos;
  a.margin = cfg->margin; a.seed = cfg->seed;
  a.sc = w.sc;
  a.emb = emb; a.out_feat = out_feat; a.out_loss = out_loss; a.out_grad = out_grad; a.out_flags = out_flags;
  a.act = w.act;
  const dim3 grid((unsigned)((n_users + kFiTile - 1) / kFiTile));
  const size_t lds = fi_lds_bytes(E, D, tier);
  if (tier == 0)
    DCUE_LAUNCH(k_foldin<0>, grid, dim3(kFiThreads), lds, s, a);
  else if (tier == 1)
    DCUE_LAUNCH(k_foldin<1>, grid, dim3(kFiThreads), lds, s, a);
  else
    DCUE_LAUNCH(k_foldin<2>, grid, dim3(kFiThreads), lds, s, a);
  DCUE_LAUNCH_CHECK();
  DCUE_HIP_CHECK(hipStreamSynchronize(s));  // (the scalars' host copy stays alive until here)
  return DCUE_OK;
}

int dcue_foldin_negatives(int64_t n_cand, const uint8_t* cand_mask, const int64_t* hist_ptr,
                          const int32_t* hist_idx, int32_t n_users, int64_t row0, const dcue_foldin_config* cfg,
                          int32_t step, int32_t* out_neg, void* stream) {
  if (!hist_ptr || !hist_idx || !cfg || !out_neg || step < 0 || step >= kFiMaxSteps) return DCUE_ERR_INVALID;
  TRY(foldin_check_sampling(n_cand, n_users, row0, cfg->n_neg, cfg->max_pos));
  if (n_users == 0) return DCUE_OK;
  DCUE_LAUNCH(k_foldin_negatives, dim3((unsigned)n_users), dim3(256), 0, (hipStream_t)stream, (long long)n_cand,
              cand_mask, hist_ptr, hist_idx, (long long)row0, (int)cfg->max_pos, (int)cfg->n_neg,
              (unsigned long long)cfg->seed, (int)step, out_neg);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

}  // extern "C"
