// Bitonic sorting of 64-bit keys in LDS, shared by the evaluator (rank.hip) and top-K (topk.hip).
// Integer compares and moves only: nothing here depends on the including file's -ffp-contract
// setting. Anything added must keep to tgemm.h's rule: no float multiply feeding a float add unless
// it is written as an explicit fmaf.
#pragma once
#include "dcue_internal.h"

namespace dcue {

// Compare-exchange t of the (size, stride) stage of a bitonic network over b[]
template <bool DESC, typename K>
__device__ __forceinline__ void bitonic_cx(K* b, int t, int size, int stride) {
  const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
  const bool fwd = (lo & size) == 0;
  const K x = b[lo], y = b[hi];
  if ((DESC ? x < y : x > y) == fwd) {
    b[lo] = y;
    b[hi] = x;
  }
}

// Bitonic sort of key[0 .. np2) in LDS (np2 a power of two), by a workgroup of 256 threads; the
// caller's stores to key[] need a barrier before the call, and the sort ends on one.
template <bool DESC>
__device__ __forceinline__ void block_bitonic_sort(uint64_t* key, int np2) {
  for (int size = 2; size <= np2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < np2 / 2; t += 256) bitonic_cx<DESC>(key, t, size, stride);
      __syncthreads();
    }
  }
}

}  // namespace dcue
