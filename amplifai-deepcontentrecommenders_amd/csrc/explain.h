// LDS layout sizes of the explanation kernel (explain.hip), as constexpr functions of d so that the
// launcher, the kernel and a host-only test (tests/test_explain_cpu.py compiles this header alone)
// agree. Self-contained: no HIP header is needed.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define EXP_HD __host__ __device__
#else
#define EXP_HD
#endif

namespace dcue {

constexpr int kExpRows = 64;      // list rows per pass: a list of up to 128 picks takes two passes
constexpr int kExpTile = 64;      // history entries per tile
constexpr int kExpReasons = 8;    // DCUE_EXPLAIN_MAX_REASONS: keys a thread keeps in registers
constexpr int kExpQuarters = 4;   // threads per list row in the selection, 16 tile columns each
constexpr int kExpPitch = kExpTile + 1;    // the score tile's row pitch (odd: a column read is conflict-free)
constexpr int kExpLdsBudget = 160 * 1024;  // a CU's LDS

EXP_HD constexpr int exp_dp(int d) { return (d + 15) & ~15; }  // rank_dp: the MFMA k split
// floats of one row tile: [64][dp + 4], the pitch k_topk_scores stages its operands at
EXP_HD constexpr size_t exp_rows_floats(int d) { return (size_t)kExpRows * (exp_dp(d) + 4); }
// bytes of the region the score tile [64][65] floats and, after the last history tile, the
// [64][4][8] merge keys share
EXP_HD constexpr size_t exp_score_bytes() {
  return (size_t)kExpRows * kExpPitch * 4 > (size_t)kExpRows * kExpQuarters * kExpReasons * 8
             ? (size_t)kExpRows * kExpPitch * 4
             : (size_t)kExpRows * kExpQuarters * kExpReasons * 8;
}
// the list rows' tile, the history tile, the score tile / merge keys, the tile's candidate per column
// [64] and the pass's list entries [64] as words, 4 words of flags
EXP_HD constexpr size_t exp_lds_bytes(int d) {
  return 2 * exp_rows_floats(d) * 4 + exp_score_bytes() + (size_t)kExpTile * 4 + (size_t)kExpRows * 4 + 16;
}
static_assert(exp_score_bytes() % 16 == 0, "the words after the score tile stay 16-byte aligned");
static_assert(exp_lds_bytes(256) <= (size_t)kExpLdsBudget, "one workgroup per CU at the worst case");

}  // namespace dcue
