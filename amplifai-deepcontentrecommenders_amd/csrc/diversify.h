// LDS layout sizes of the diversity kernels (diversify.hip), as constexpr functions of (pool, d) so that
// the launcher, the kernels and a host-only test (tests/test_mmr_cpu.py compiles this header alone)
// agree. Self-contained: no HIP header is needed.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define DIV_HD __host__ __device__
#else
#define DIV_HD
#endif

namespace dcue {

constexpr int kDivPos = 128;    // pool positions (DCUE_TOPK_MAX_K): two per lane of the selecting wave
constexpr int kDivChunk = 128;  // columns of the row tile per pass
constexpr int kDivLdsBudget = 160 * 1024;  // a CU's LDS

DIV_HD constexpr int div_p16(int pool) { return (pool + 15) & ~15; }
DIV_HD constexpr int div_dp(int d) { return (d + 15) & ~15; }  // rank_dp: the MFMA k split
DIV_HD constexpr int div_chunk(int d) { return div_dp(d) < kDivChunk ? div_dp(d) : kDivChunk; }
// floats of the region the row tile [p16][chunk + 4] and, after it, the Gram [p16][p16 + 1] share
DIV_HD constexpr size_t div_tile_floats(int pool, int d) {
  return (size_t)div_p16(pool) * (div_chunk(d) + 4) > (size_t)div_p16(pool) * (div_p16(pool) + 1)
             ? (size_t)div_p16(pool) * (div_chunk(d) + 4)
             : (size_t)div_p16(pool) * (div_p16(pool) + 1);
}
// the shared region (rounded to 16 bytes), colsum [128] doubles, idx / rel / inv / order [128] words each,
// 4 words of flags
DIV_HD constexpr size_t div_lds_bytes(int pool, int d) {
  return ((div_tile_floats(pool, d) + 3) & ~(size_t)3) * 4 + (size_t)kDivPos * 8 + 4 * (size_t)kDivPos * 4 + 16;
}
static_assert(2 * div_lds_bytes(128, 256) <= (size_t)kDivLdsBudget, "two workgroups per CU at the worst case");

}  // namespace dcue
