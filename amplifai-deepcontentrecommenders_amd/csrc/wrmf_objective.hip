// The WRMF objective without the dense [users][items] matrix -- gfx950.
//
// With s_ui = x_u . y_i, p_ui = 1 and c_ui = 1 + alpha v_ui on the observed pairs, p = 0 and c = 1 elsewhere:
//   L = sum_{u,i} c_ui (p_ui - s_ui)^2 + lambda (|X|^2 + |Y|^2)
//     = sum_{observed} [c_ui (1 - s_ui)^2 - s_ui^2] + sum_{a,b} (X^T X)_ab (Y^T Y)_ab + lambda (tr X^T X + tr Y^T Y)
// because sum over ALL pairs of s_ui^2 is the Frobenius inner product of the two Gram matrices. fp64
// throughout, from the fp32 factors: near a fit the observed term is negative and cancels most of the
// all-pairs term, and the sums run over millions of pairs.
//
// Kernels:
//   k_wrmf_gram_mfma / k_wrmf_gram_reduce  (wrmf.hip, launch_wrmf_gram) both Grams, in the ALS solver's order
//   k_wrmf_obj_pairs   the observed term's row sums: one wave per user row, x_u in registers for the
//                      row; a 16-lane group per pair, so one load instruction of the wave fetches four
//                      y_i rows (16 B per lane where dim is a multiple of 4) and two batches -- eight
//                      rows -- are in flight per wave; the pair's fp64 dot product is eight in-lane FMAs
//                      and a 4-step xor butterfly inside the group (a fixed tree: every lane ends with
//                      the same bits), and the row's terms are added in pair order into one fp64 partial
//   k_wrmf_obj_reduce  the row partials, 4096 per workgroup (16 per thread in index order, then a tree
//                      over the 256 threads), applied until one value is left: a tree whose shape
//                      depends on n_users alone
//   k_wrmf_obj_final   sum_{a,b} GX_ab GY_ab and the traces in the same fixed order, and out[0..3]
// No atomics anywhere: two calls give the same bits.
#include "dcue_internal.h"

namespace dcue {

constexpr int kObjMaxDim = 128;
constexpr int kObjRed = 4096;        // row partials per k_wrmf_obj_reduce workgroup
constexpr long kObjMaxBlocks = 16384;  // k_wrmf_obj_pairs workgroups (4 rows each per sweep)

__device__ __forceinline__ double obj_readlane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// sum over the 16 lanes of a group, the same bits in each of them
__device__ __forceinline__ double obj_group_sum(double v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// VEC (dim % 4 == 0: every row is 16-byte aligned): lane j of a group holds elements 4j..4j+3 and
// 64+4j..64+4j+3; otherwise elements j + 16 e, e = 0..7 (4-byte loads, 64 contiguous bytes per group)
template <bool VEC>
struct ObjRow {
  float v[8];
  __device__ __forceinline__ void load(const float* __restrict__ row, int j, int dim) {
    if (VEC) {
      // (the loads are unconditional at a clamped offset, their values selected)
      const bool a = 4 * j < dim, b = 64 + 4 * j < dim;
      const float4 lo = ld4(row + (a ? 4 * j : 0)), hi = ld4(row + (b ? 64 + 4 * j : 0));
      v[0] = a ? lo.x : 0.f; v[1] = a ? lo.y : 0.f; v[2] = a ? lo.z : 0.f; v[3] = a ? lo.w : 0.f;
      v[4] = b ? hi.x : 0.f; v[5] = b ? hi.y : 0.f; v[6] = b ? hi.z : 0.f; v[7] = b ? hi.w : 0.f;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = j + 16 * e;
        const float x = row[k < dim ? k : 0];
        v[e] = k < dim ? x : 0.f;
      }
    }
  }
};

template <bool VEC>
__global__ __launch_bounds__(256) void k_wrmf_obj_pairs(const float* __restrict__ X, const float* __restrict__ Y,
                                                        long n_users, long n_items, int dim,
                                                        const int64_t* __restrict__ indptr,
                                                        const int32_t* __restrict__ indices,
                                                        const float* __restrict__ values, double alpha,
                                                        double* __restrict__ rowpart) {
  const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long)gridDim.x * 4;
  for (long u = wave; u < n_users; u += n_waves) {
    const long p0 = indptr[u], p1 = indptr[u + 1];
    double acc = 0.0;  // (the same value in every lane)
    if (p1 > p0) {
      ObjRow<VEC> x;
      x.load(X + u * dim, j, dim);
      for (long pb = p0; pb < p1; pb += 8) {
        // two batches of four pairs: group g takes pairs pb + g and pb + 4 + g; a slot past the row
        // repeats the row's last pair (a valid address) and contributes 0
        const long pa = pb + g, pc = pb + 4 + g;
        const bool va = pa < p1, vc = pc < p1;
        const long qa = va ? pa : p1 - 1, qc = vc ? pc : p1 - 1;
        const int ia = indices[qa], ic = indices[qc];
        const float wa = values ? values[qa] : 1.f, wc = values ? values[qc] : 1.f;
        // an index outside the table is not dereferenced: row 0 is read and the term made NaN
        const bool oka = ia >= 0 && ia < n_items, okc = ic >= 0 && ic < n_items;
        ObjRow<VEC> ya, yc;
        ya.load(Y + (long)(oka ? ia : 0) * dim, j, dim);
        yc.load(Y + (long)(okc ? ic : 0) * dim, j, dim);
        double da = 0.0, dc = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          da = fma((double)x.v[e], (double)ya.v[e], da);
          dc = fma((double)x.v[e], (double)yc.v[e], dc);
        }
        const double sa = obj_group_sum(da), sc = obj_group_sum(dc);
        const double ca = 1.0 + alpha * (double)wa, cc = 1.0 + alpha * (double)wc;
        double ta = ca * (1.0 - sa) * (1.0 - sa) - sa * sa, tc = cc * (1.0 - sc) * (1.0 - sc) - sc * sc;
        ta = !va ? 0.0 : oka ? ta : __builtin_nan("");
        tc = !vc ? 0.0 : okc ? tc : __builtin_nan("");
        // pair order: pb, pb + 1, ..., pb + 7
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += obj_readlane(ta, 16 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += obj_readlane(tc, 16 * q);
      }
    }
    if (lane == 0) rowpart[u] = acc;
  }
}

// sums of 256 doubles held one per thread, thread 0 returns the total (a fixed tree)
__device__ __forceinline__ double obj_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// out[b] = the sum of in[b * kObjRed .. min(n, (b + 1) * kObjRed))
__global__ __launch_bounds__(256) void k_wrmf_obj_reduce(const double* __restrict__ in, long n,
                                                         double* __restrict__ out) {
  __shared__ double red[256];
  const long base = (long)blockIdx.x * kObjRed;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kObjRed / 256; ++i) {
    const long e = base + threadIdx.x + 256 * i;
    s += e < n ? in[e] : 0.0;
  }
  const double r = obj_block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// one workgroup: the all-pairs term and the traces from the two Grams ([D16][D16], zero past dim);
// obs: the observed term (null: 0)
__global__ __launch_bounds__(256) void k_wrmf_obj_final(const double* __restrict__ GX, const double* __restrict__ GY,
                                                        int dim, double lambda, const double* __restrict__ obs,
                                                        double* __restrict__ out) {
  __shared__ double red[256];
  const int D16 = (dim + 15) & ~15;
  double ap = 0.0, tr = 0.0;
  for (int e = threadIdx.x; e < D16 * D16; e += 256) {
    ap = fma(GX[e], GY[e], ap);
    if (e / D16 == e % D16) tr += GX[e] + GY[e];
  }
  const double all_pairs = obj_block_sum(ap, red);
  const double trace = obj_block_sum(tr, red);
  if (threadIdx.x == 0) {
    const double observed = obs ? *obs : 0.0, reg = lambda * trace;
    out[0] = observed + all_pairs + reg;
    out[1] = observed;
    out[2] = all_pairs;
    out[3] = reg;
  }
}

struct ObjWs {
  double *part, *GX, *GY, *rowpart, *ra, *rb;
};

static long obj_red_blocks(long n) { return (n + kObjRed - 1) / kObjRed; }

static size_t obj_carve(int64_t n_users, int64_t n_items, int32_t dim, void* base, ObjWs* w) {
  Arena ar{reinterpret_cast<char*>(base), 0, 0};
  const long nu = n_users < 1 ? 1 : (long)n_users, ni = n_items < 1 ? 1 : (long)n_items;
  const long cu = wrmf_gram_chunks(nu), ci = wrmf_gram_chunks(ni);
  const size_t d16 = (size_t)((dim + 15) & ~15);
  w->part = ar.take<double>((size_t)(cu > ci ? cu : ci) * dim * dim);  // one Gram at a time
  w->GX = ar.take<double>(d16 * d16);
  w->GY = ar.take<double>(d16 * d16);
  w->rowpart = ar.take<double>((size_t)nu);
  w->ra = ar.take<double>((size_t)obj_red_blocks(nu));
  w->rb = ar.take<double>((size_t)obj_red_blocks(obj_red_blocks(nu)));
  return ar.used + 256;  // (the base is aligned up to 256 bytes)
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_wrmf_objective_workspace_bytes(int64_t n_users, int64_t n_items, int32_t dim, size_t* bytes_host) {
  if (!bytes_host || dim <= 0 || dim > kObjMaxDim || n_users < 0 || n_items < 0) return DCUE_ERR_INVALID;
  ObjWs w;
  *bytes_host = obj_carve(n_users, n_items, dim, nullptr, &w);
  return DCUE_OK;
}

int dcue_wrmf_objective(const float* X, int64_t n_users, const float* Y, int64_t n_items, int32_t dim,
                        const int64_t* indptr, const int32_t* indices, const float* values, double alpha,
                        double lambda, void* ws, size_t ws_bytes, double* out, void* stream) {
  if (!X || !Y || !indptr || !out || !ws || n_users < 0 || n_items < 0 || (!indices && n_users > 0) || dim <= 0 ||
      dim > kObjMaxDim || !(lambda > 0.0))
    return DCUE_ERR_INVALID;
  ObjWs w;
  if (obj_carve(n_users, n_items, dim, nullptr, &w) > ws_bytes) return DCUE_ERR_WORKSPACE;
  obj_carve(n_users, n_items, dim, reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255)),
            &w);
  hipStream_t s = (hipStream_t)stream;
  const size_t d16 = (size_t)((dim + 15) & ~15);
  // the Grams, one after the other through the same partials (an empty side: G = 0)
  if (n_users > 0)
    TRY(launch_wrmf_gram(X, (long)n_users, (int)dim, w.part, w.GX, s));
  else
    DCUE_HIP_CHECK(hipMemsetAsync(w.GX, 0, d16 * d16 * sizeof(double), s));
  if (n_items > 0)
    TRY(launch_wrmf_gram(Y, (long)n_items, (int)dim, w.part, w.GY, s));
  else
    DCUE_HIP_CHECK(hipMemsetAsync(w.GY, 0, d16 * d16 * sizeof(double), s));
  const double* obs = nullptr;
  if (n_users > 0) {
    const long blocks = (n_users + 3) / 4 < kObjMaxBlocks ? (long)((n_users + 3) / 4) : kObjMaxBlocks;
    // 16-byte row loads where every row of both tables is 16-byte aligned
    if (dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 15) == 0)
      DCUE_LAUNCH(k_wrmf_obj_pairs<true>, dim3((unsigned)blocks), dim3(256), 0, s, X, Y, (long)n_users, (long)n_items,
                  (int)dim, indptr, indices, values, alpha, w.rowpart);
    else
      DCUE_LAUNCH(k_wrmf_obj_pairs<false>, dim3((unsigned)blocks), dim3(256), 0, s, X, Y, (long)n_users, (long)n_items,
                  (int)dim, indptr, indices, values, alpha, w.rowpart);
    DCUE_LAUNCH_CHECK();
    // the rows' tree: levels of kObjRed, alternating between the two level buffers
    const double* in = w.rowpart;
    double* dst = w.ra;
    long n = (long)n_users;
    do {
      const long nb = obj_red_blocks(n);
      DCUE_LAUNCH(k_wrmf_obj_reduce, dim3((unsigned)nb), dim3(256), 0, s, in, n, dst);
      DCUE_LAUNCH_CHECK();
      in = dst;
      dst = dst == w.ra ? w.rb : w.ra;
      n = nb;
    } while (n > 1);
    obs = in;
  }
  DCUE_LAUNCH(k_wrmf_obj_final, dim3(1), dim3(256), 0, s, (const double*)w.GX, (const double*)w.GY, (int)dim, lambda,
              obs, out);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

}  // extern "C"
