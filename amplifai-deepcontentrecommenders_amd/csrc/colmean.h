// Fixed-order column means of a [n][cols] fp64 matrix over its unflagged rows, for ONE workgroup of
// kColMeanThreads threads (k_topk_metrics_mean, k_list_ild_mean): no workspace for cross-workgroup
// partials, no floating-point atomics, so the sum's order depends on n and cols only and the means are
// bit-identical however the matrix was filled.
#pragma once

#include "dcue_common.h"

namespace dcue {

constexpr int kColMeanThreads = 1024;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Thread (g, column) sums the rows g, g + G, g + 2G, ... of its column in that order, G =
// kColMeanThreads / cols row groups; a column's G partials are then added in ascending g. A flagged
// row adds +0. out_mean[cols] = the sums over *cnt, the number of rows with flags == 0 (0 where it is
// 0), which also goes to *out_n. part: kColMeanThreads doubles of LDS; cnt: an LDS int the caller
// zeroed before a barrier. All threads call it; it ends after a barrier, with *cnt final.
__device__ __forceinline__ void col_means(const double* __restrict__ v, const int32_t* __restrict__ flags, int n,
                                          int cols, double* part, int* cnt, double* __restrict__ out_mean,
                                          int32_t* __restrict__ out_n) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int G = kColMeanThreads / cols;
  double s = 0.0;
  if (tid < G * cols) {
    const int col = tid % cols;
    int r = tid / cols;
    for (; r + 3 * G < n; r += 4 * G) {  // four rows' loads in flight, added in row order
      const int f0 = flags[r], f1 = flags[r + G], f2 = flags[r + 2 * G], f3 = flags[r + 3 * G];
      const double x0 = v[(size_t)r * cols + col], x1 = v[(size_t)(r + G) * cols + col];
      const double x2 = v[(size_t)(r + 2 * G) * cols + col], x3 = v[(size_t)(r + 3 * G) * cols + col];
      s += f0 ? 0.0 : x0;
      s += f1 ? 0.0 : x1;
      s += f2 ? 0.0 : x2;
      s += f3 ? 0.0 : x3;
    }
    for (; r < n; r += G) s += flags[r] ? 0.0 : v[(size_t)r * cols + col];
  }
  part[tid] = s;
  int ne = 0;
  for (int r = tid; r < n; r += kColMeanThreads) ne += flags[r] == 0;
  ne = wave_sum_int(ne);
  if (lane == 0 && ne) atomicAdd(cnt, ne);
  __syncthreads();
  if (tid < cols) {
    double tot = 0.0;
    for (int g = 0; g < G; ++g) tot += part[g * cols + tid];
    out_mean[tid] = *cnt > 0 ? tot / (double)*cnt : 0.0;
  }
  if (tid == 0) *out_n = *cnt;
}

}  // namespace dcue
