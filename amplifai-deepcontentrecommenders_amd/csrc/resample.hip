// Sample-rate conversion (include/dcue.h, dcue_resample): a rational polyphase resampler with a
// Kaiser-windowed sinc evaluated exactly per phase. Every tap is computed on the host in double precision
// (the Bessel function by its power series) and rounded once, so the kernel calls no device
// transcendental. No scratch, no workspace; zero extension is index arithmetic.
//
// The work is y[m] = sum_k tab[p_m][k] x[q_m - Kh + 1 + k]: every output has its own phase row and its own
// window, so the reuse lies across clips (one row serves output m of every clip) and across neighbouring
// outputs (their windows overlap). That is a GEMM on v_mfma_f32_16x16x4_f32 with a Toeplitz A operand:
//   rows     16 consecutive outputs of a wave; row i holds its phase row shifted by q_i - q_0 columns,
//            zero elsewhere (K + floor(15 M / L) + 1 columns, rounded to the 4-wide MFMA step);
//   columns  16 clips, four times per wave (four independent accumulators share one A register);
//   k        the input samples of the rows' common window, ascending.
// A workgroup (4 waves) owns kResampleTile = 64 consecutive outputs, counted from out0, of kResampleClips
// = 64 clips. The window is staged through LDS kResampleChunk samples at a time (row stride = 2 mod 32
// words: the B reads are conflict-free), so the LDS use does not depend on K. The A operand streams from
// the table (L2-resident: 341 KB at most for the rates in use) straight into registers, a chunk's 32
// steps at once.
//
// Summation order. The MFMA accumulates k in order, each product exact and added with one rounding: output
// m is the chain acc = fmaf(tab[p][k], x[q - Kh + 1 + k], acc) over k = 0 .. K-1 from acc = +0. The zero
// columns of the Toeplitz operand before and after a row's taps add +-0 to the chain, which leaves it as
// it is (the chain starts at +0 and so is never -0). An output's bits are therefore a function of its K
// samples and its phase row alone: not of its place in the tile, of out0 / n_out, of n_clips or of the
// clip's place in the batch.
//
// Non-finite samples. 0 * NaN is NaN, so a NaN under a zero column would reach outputs whose support does
// not cover it. The staging pass therefore stores 0 for a non-finite sample and raises a workgroup flag;
// in such a workgroup (and only there) each lane then scans the K samples of the outputs it is about to
// store, and an output whose support holds a non-finite sample is recomputed with the same fmaf chain
// over its own K samples, which propagates it by IEEE rules. The others keep their bits.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dcue_common.h"
#include "dcue_internal.h"

namespace dcue {

constexpr int kResampleTile = 64;    // outputs per workgroup, counted from out0: 4 waves x 16 rows
constexpr int kResampleBlocks = 4;   // MFMA column blocks (16 clips each) per wave
constexpr int kResampleClips = 16 * kResampleBlocks;  // clips per workgroup
constexpr int kResampleChunk = 128;  // window samples per clip staged at a time
constexpr int kResampleStride = kResampleChunk + 2;
constexpr int kResampleSteps = kResampleChunk / 4;  // MFMA steps (4 window columns each) per chunk
constexpr int kResampleMagic = 0x50534552;
constexpr int kResampleHeaderBytes = 32;
constexpr size_t kResampleTableCap = (size_t)DCUE_RESAMPLE_MAX_TABLE_BYTES;

// gcd-reduced rates and the filter's shape, all derived on the host
struct ResampleShape {
  int L, M, K, Kh;
  double s;
  size_t bytes;
};

// raw buffer descriptors (stride 0): an offset at or past num_records reads as 0
constexpr int kBufferFlags = 0x00020000;
constexpr unsigned kBufferOut = 0xfffffff0u;
template <typename R>
__device__ __forceinline__ float buffer_load_f32(R rsrc, unsigned byte_offset) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, byte_offset, 0, 0));
}

struct ResampleLaunch {
  const char* table;
  const float* wave;
  float* out;
  long long n_in, out0, n_out, n_clips, tiles;
  int L, M, K, Kh;
};

__global__ __launch_bounds__(256) void k_resample(const ResampleLaunch a) {
  __shared__ float s_x[kResampleClips * kResampleStride];
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform, and the compiler knows it
  const int L = a.L, M = a.M, K = a.K, Kh = a.Kh;
  const int* hdr = reinterpret_cast<const int*>(a.table);
  const float* tab = reinterpret_cast<const float*>(a.table + kResampleHeaderBytes);
  const long long tile = blockIdx.x % a.tiles;
  const long long clip0 = (blockIdx.x / a.tiles) * kResampleClips;
  const long long m_end = a.out0 + a.n_out;
  const long long m_wg = a.out0 + tile * kResampleTile;  // 64-bit from here: m M passes 2^32
  const long long m_w = m_wg + 16 * wv;
  const int col = lane & 15, kk = lane >> 4;

  // a table of another configuration (or one never initialised): every output of the launch is NaN
  if (hdr[0] != kResampleMagic || hdr[1] != L || hdr[2] != M || hdr[3] != K || hdr[4] != Kh) {
#pragma unroll
    for (int h = 0; h < kResampleBlocks; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long m = m_w + 4 * kk + r, clip = clip0 + col + 16 * h;
        if (m < m_end && clip < a.n_clips) a.out[clip * a.n_out + (m - a.out0)] = __int_as_float(0x7fc00000);
      }
    return;
  }

  const long long q_wg = (m_wg * M) / L;
  const long long X0 = q_wg - Kh + 1;  // the workgroup's window starts at sample X0 (may be negative)
  const int w_wg = ((int)(((m_wg + kResampleTile - 1) * M) / L - q_wg) + K + 3) & ~3;
  // this wave's 16 rows in window columns: origin dw (a multiple of the MFMA step), width w_w
  const int dw = (int)((m_w * M) / L - q_wg) & ~3;
  const int w_w = ((int)(((m_w + 15) * M) / L - q_wg) - dw + K + 3) & ~3;
  // this lane's A row: output m_w + col, its phase row and the column of its first tap
  const long long mm = (m_w + col) * M;
  const int row = (int)(mm % L) * K;  // in floats from tab: the table is below 16 MiB
  const int d_i = (int)(mm / L - q_wg) - dw;
  const auto rt = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(tab), 0, L * K * 4, kBufferFlags);
  // the clips' descriptors start at the window's first sample inside the clip and end with the clip
  const long long base = max(X0, 0LL);
  const int x_bytes = (int)min((a.n_in - base) * 4, (long long)INT32_MAX);

  if (tid == 0) s_bad = 0;
  f32x4 acc[kResampleBlocks];
#pragma unroll
  for (int h = 0; h < kResampleBlocks; ++h) acc[h] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < w_wg; c0 += kResampleChunk) {
    const int cw = min(kResampleChunk, w_wg - c0);
    const int lo = max(c0, dw), hi = min(c0 + cw, dw + w_w);  // this wave's columns of the chunk: multiples of 4
    // Every load of the chunk is issued before anything waits: the wave's share of the window (16 clips x
    // 2 samples per lane) and the lane's A values of the chunk's 32 steps -- one round trip to L2 per
    // chunk instead of one per few steps. They are buffer loads: an element that is not there (a sample
    // before the clip or past its end, a clip past the batch, a column outside the row's taps) gets an
    // offset beyond the descriptor's range and the hardware returns 0 -- no branch on a lane's value sits
    // between two loads. What no lane of the wave needs (columns past the chunk's end, steps outside the
    // wave's columns) is skipped by a scalar branch.
    float xv[kResampleClips / 4][kResampleChunk / 64];
#pragma unroll
    for (int j = 0; j < kResampleClips / 4; ++j) {
      const long long clip = clip0 + wv + 4 * j;
      const bool on = clip < a.n_clips;
      const float* x = a.wave + (on ? clip * a.n_in + base : 0);
      const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, on ? x_bytes : 0, kBufferFlags);
#pragma unroll
      for (int e = 0; e < kResampleChunk / 64; ++e) {
        const int c = lane + 64 * e;
        const long long rel = X0 + c0 + c - base;  // < 0: before the clip; the range check finds its end
        xv[j][e] = 0.f;
        if (64 * e < cw) xv[j][e] = buffer_load_f32(rx, (c < cw && rel >= 0) ? (unsigned)rel * 4u : kBufferOut);
      }
    }
    float av[kResampleSteps];
#pragma unroll
    for (int g = 0; g < kResampleSteps / 8; ++g) {
      const bool need = c0 + 32 * g + 32 > lo && c0 + 32 * g < hi;
#pragma unroll
      for (int s = 8 * g; s < 8 * g + 8; ++s) {
        const int c = c0 + 4 * s, t = c - dw + kk - d_i;
        av[s] = 0.f;
        if (need) av[s] = buffer_load_f32(rt, (c >= lo && c < hi && t >= 0 && t < K) ? (unsigned)(row + t) * 4u : kBufferOut);
      }
    }
    __syncthreads();  // the previous chunk has been read (first pass: s_bad is clear)
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kResampleClips / 4; ++j)
#pragma unroll
      for (int e = 0; e < kResampleChunk / 64; ++e) {
        float v = xv[j][e];
        if (!isfinite(v)) {
          bad = true;
          v = 0.f;
        }
        s_x[(wv + 4 * j) * kResampleStride + lane + 64 * e] = v;
      }
    if (bad) s_bad = 1;
    __syncthreads();
    const float* b = s_x + col * kResampleStride + kk;
    // groups of 8 steps, skipped where the wave has no column; inside a group the steps outside [lo, hi)
    // run with A = 0 over staged, finite samples: +-0 added to the chain
#pragma unroll
    for (int g = 0; g < kResampleSteps / 8; ++g) {
      if (c0 + 32 * g + 32 > lo && c0 + 32 * g < hi) {
#pragma unroll
        for (int s = 8 * g; s < 8 * g + 8; ++s)
#pragma unroll
          for (int h = 0; h < kResampleBlocks; ++h) acc[h] = mfma4(av[s], b[4 * s + 16 * h * kResampleStride], acc[h]);
      }
    }
  }
  const bool fix = s_bad != 0;  // written before the last barrier
#pragma unroll
  for (int h = 0; h < kResampleBlocks; ++h) {
    const long long clip = clip0 + col + 16 * h;
    if (clip >= a.n_clips) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long m = m_w + 4 * kk + r;
      if (m >= m_end) continue;
      float v = acc[h][r];
      if (fix) {
        const float* x = a.wave + clip * a.n_in;
        const long long mq = m * M, first = mq / L - Kh + 1;
        const float* tr = tab + (mq % L) * K;
        const int k0 = (int)max(0LL, -first), k1 = (int)min((long long)K, a.n_in - first);
        bool covered = false;
        for (int k = k0; k < k1; ++k) covered |= !isfinite(x[first + k]);
        if (covered) {
          v = 0.f;
          for (int k = k0; k < k1; ++k) v = fmaf(tr[k], x[first + k], v);  // the samples outside are zeros: +-0 added
        }
      }
      a.out[clip * a.n_out + (m - a.out0)] = v;
    }
  }
}

static int resample_fail(const char* why) {
  set_last_message(why);
  return DCUE_ERR_INVALID;
}

static int resample_shape(const dcue_resample_config* c, ResampleShape* sh) {
  if (!c) return resample_fail("dcue_resample: null config");
  if (c->rate_in < 1 || c->rate_out < 1) return resample_fail("dcue_resample: rate_in and rate_out must be positive");
  if (c->rate_in == c->rate_out) return resample_fail("dcue_resample: equal rates: nothing to resample");
  if (c->zeros < 1) return resample_fail("dcue_resample: zeros must be >= 1");
  if (!(c->rolloff > 0.0) || !(c->rolloff <= 1.0)) return resample_fail("dcue_resample: rolloff must be in (0, 1]");
  if (!(c->beta >= 0.0) || !isfinite(c->beta)) return resample_fail("dcue_resample: beta must be >= 0");
  long long g = c->rate_in, r = c->rate_out;
  while (r) {
    const long long t = g % r;
    g = r;
    r = t;
  }
  const long long L = c->rate_out / g, M = c->rate_in / g;
  const double s = c->rolloff * (L < M ? (double)L / (double)M : 1.0);
  const double kh = ceil((double)c->zeros / s);
  const double bytes = (double)kResampleHeaderBytes + 4.0 * (double)L * 2.0 * kh;
  if (bytes > (double)kResampleTableCap) {
    set_last_message("dcue_resample: the phase table exceeds DCUE_RESAMPLE_MAX_TABLE_BYTES (near-coprime rates)");
    return DCUE_ERR_UNSUPPORTED;
  }
  sh->L = (int)L;
  sh->M = (int)M;
  sh->Kh = (int)kh;
  sh->K = 2 * sh->Kh;
  sh->s = s;
  sh->bytes = (size_t)kResampleHeaderBytes + 4u * (size_t)L * (size_t)sh->K;
  return DCUE_OK;
}

// I0 by its power series sum_j ((x/2)^j / j!)^2, every term positive: converges to double precision
static double bessel_i0(double x) {
  const double h = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int j = 1; j < 1000; ++j) {
    term *= h / ((double)j * (double)j);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_resample_length(const dcue_resample_config* cfg, int64_t n_in, int64_t* n_out_host) {
  ResampleShape sh;
  TRY(resample_shape(cfg, &sh));
  if (!n_out_host) return resample_fail("dcue_resample_length: null output");
  if (n_in < 0) return resample_fail("dcue_resample: negative n_in");
  if (n_in > INT32_MAX) {
    set_last_message("dcue_resample: n_in beyond 2^31 - 1");
    return DCUE_ERR_UNSUPPORTED;
  }
  *n_out_host = (n_in * sh.L + sh.M - 1) / sh.M;
  return DCUE_OK;
}

int dcue_resample_table_bytes(const dcue_resample_config* cfg, size_t* bytes_host) {
  ResampleShape sh;
  TRY(resample_shape(cfg, &sh));
  if (!bytes_host) return resample_fail("dcue_resample_table_bytes: null output");
  *bytes_host = sh.bytes;
  return DCUE_OK;
}

int dcue_resample_table_fill_host(const dcue_resample_config* cfg, void* table_host, size_t bytes) {
  ResampleShape sh;
  TRY(resample_shape(cfg, &sh));
  if (!table_host) return resample_fail("dcue_resample_table_fill_host: null pointer");
  if (bytes != sh.bytes) return resample_fail("dcue_resample_table_fill_host: the table size differs from dcue_resample_table_bytes");
  char* base = static_cast<char*>(table_host);
  int32_t* hdr = reinterpret_cast<int32_t*>(base);
  float* tab = reinterpret_cast<float*>(base + kResampleHeaderBytes);
  const double zeros = (double)cfg->zeros, i0b = bessel_i0(cfg->beta);
  for (int p = 0; p < sh.L; ++p)
    for (int k = 0; k < sh.K; ++k) {
      const double u = sh.s * ((double)p / (double)sh.L - (double)(k - sh.Kh + 1));
      double v = 0.0;
      if (fabs(u) < zeros) {
        const double pu = M_PI * u, r = u / zeros;
        const double sinc = u == 0.0 ? 1.0 : sin(pu) / pu;
        v = sh.s * sinc * (bessel_i0(cfg->beta * sqrt(1.0 - r * r)) / i0b);
      }
      tab[(size_t)p * sh.K + k] = (float)v;
    }
  hdr[0] = kResampleMagic;
  hdr[1] = sh.L;
  hdr[2] = sh.M;
  hdr[3] = sh.K;
  hdr[4] = sh.Kh;
  hdr[5] = cfg->zeros;
  hdr[6] = cfg->rate_in;
  hdr[7] = cfg->rate_out;
  return DCUE_OK;
}

int dcue_resample_table_init(const dcue_resample_config* cfg, void* table_dev, size_t bytes, void* stream) {
  ResampleShape sh;
  TRY(resample_shape(cfg, &sh));
  if (!table_dev) return resample_fail("dcue_resample_table_init: null pointer");
  if (bytes != sh.bytes) return resample_fail("dcue_resample_table_init: the table size differs from dcue_resample_table_bytes");
  std::vector<char> host(sh.bytes);
  TRY(dcue_resample_table_fill_host(cfg, host.data(), sh.bytes));
  // the staging vector dies with this call: wait for the copy
  DCUE_HIP_CHECK(hipMemcpyAsync(table_dev, host.data(), sh.bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  DCUE_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return DCUE_OK;
}

int dcue_resample(const dcue_resample_config* cfg, const void* table_dev, const float* wave, int64_t n_clips,
                  int64_t n_in, int64_t out0, int64_t n_out, float* out, void* stream) {
  ResampleShape sh;
  TRY(resample_shape(cfg, &sh));
  if (n_clips < 0 || n_in < 0 || out0 < 0 || n_out < 0) return resample_fail("dcue_resample: negative n_clips, n_in, out0 or n_out");
  int64_t total = 0;
  TRY(dcue_resample_length(cfg, n_in, &total));
  if (out0 > total || n_out > total - out0)
    return resample_fail("dcue_resample: the output range reaches past the clip's resampled length");
  if (n_clips == 0 || n_out == 0) return DCUE_OK;
  if (!table_dev || !wave || !out) return resample_fail("dcue_resample: null pointer");
  const int64_t tiles = (n_out + kResampleTile - 1) / kResampleTile;
  const int64_t cblocks = (n_clips + kResampleClips - 1) / kResampleClips;
  if (cblocks > (int64_t)INT32_MAX / tiles) {
    set_last_message("dcue_resample: n_clips * output tiles beyond the grid limit");
    return DCUE_ERR_UNSUPPORTED;
  }
  ResampleLaunch a;
  a.table = static_cast<const char*>(table_dev);
  a.wave = wave;
  a.out = out;
  a.n_in = n_in;
  a.out0 = out0;
  a.n_out = n_out;
  a.n_clips = n_clips;
  a.tiles = tiles;
  a.L = sh.L;
  a.M = sh.M;
  a.K = sh.K;
  a.Kh = sh.Kh;
  const dim3 grid((unsigned)(tiles * cblocks)), block(256);
  DCUE_LAUNCH(k_resample, grid, block, 0, (hipStream_t)stream, a);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

}  // extern "C"
