// The splitmix64 finaliser and the 64 x 64 -> high 64 multiply behind the library's counter-based
// draws (fold-in negatives, foldin.hip; crop starts, crop.hip). Host and device run the same integers.
#pragma once

#include <hip/hip_runtime.h>

namespace dcue {

constexpr unsigned long long kGolden64 = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// floor(a * b / 2^64): a uniform 64-bit a gives a value in [0, b)
__host__ __device__ __forceinline__ unsigned long long mulhi64(unsigned long long a, unsigned long long b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umul64hi(a, b);
#else
  return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}

}  // namespace dcue
