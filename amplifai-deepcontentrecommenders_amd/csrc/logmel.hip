// Audio front end (include/dcue.h, dcue_logmel): waveform -> log-mel track-table rows in one launch.
// Framing with the reflection in the index arithmetic, periodic Hann window, a real FFT as an
// n_fft/2-point complex Stockham FFT in LDS plus the real-input split pass, power, the Slaney mel
// filterbank as per-bin runs of FFT bins, compression, and the [frame][128] row store. No spectrum
// goes to HBM and there is no workspace. Every table entry (window, twiddles, filter weights) is
// computed on the host in double precision and rounded once, so the kernel calls no sinf / cosf.
//
// One workgroup (4 waves) owns kLogmelFramesPerWg consecutive frames of one clip; a wave takes a frame
// at a time and keeps it in its own LDS buffer, so the only workgroup barrier is the one after the
// tables are staged. Inside a wave the butterfly stages exchange through LDS in place: every lane
// reads its inputs into registers, the wave synchronises, every lane writes its outputs. A frame's
// row is a function of that frame's samples and the table alone -- it does not depend on the clip's
// position, on frame0, or on what else shares the launch.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dcue_common.h"
#include "dcue_internal.h"

namespace dcue {

constexpr int kLogmelFramesPerWg = 16;
constexpr int kLogmelMagic = 0x4c4d454c;
constexpr int kLogmelHeaderBytes = 32;

// table: int32 header[8] {magic, n_fft, n_weights, 0...}; float window[N]; float2 twm[M] = exp(-2 pi i t / M);
// float2 twn[M/2 + 1] = exp(-2 pi i k / N); int32 first[128], count[128], offset[128]; float weights[N + 2]
// (M = N / 2). A bin of the spectrum lies under at most two triangles, so N + 2 weights always suffice.
__host__ __device__ constexpr size_t logmel_table_size(int N) {
  return (size_t)kLogmelHeaderBytes + 4u * N + 8u * (N / 2) + 8u * (N / 4 + 1) + 3u * 4u * DCUE_N_MELS + 4u * (N + 2);
}

// LDS traffic of one wave only: the hardware serves a wave's LDS instructions in order, the fences
// and the barrier keep the compiler from moving an access across the exchange point.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}

// Stockham radix-2 stage with Ns = 1 (no twiddles): out[2j + r] = in[j] +- in[j + M/2]
template <int M>
__device__ __forceinline__ void fft_stage2(float2* buf, int lane) {
  constexpr int Q = M / 2, PER = Q / 64;
  float2 a[PER], b[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = lane + 64 * i;
    a[i] = buf[j];
    b[i] = buf[j + Q];
  }
  wave_sync();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = lane + 64 * i;
    buf[2 * j] = make_float2(a[i].x + b[i].x, a[i].y + b[i].y);
    buf[2 * j + 1] = make_float2(a[i].x - b[i].x, a[i].y - b[i].y);
  }
  wave_sync();
}

// Stockham radix-4 stage: butterfly j reads in[j + r M/4], turns input r by exp(-2 pi i r k / (4 Ns)),
// k = j mod Ns, and writes out[(j - k) 4 + k + r Ns]
template <int M, int Ns>
__device__ __forceinline__ void fft_stage4(float2* buf, const float2* tw, int lane) {
  constexpr int Q = M / 4, PER = Q >= 64 ? Q / 64 : 1;
  const bool on = Q >= 64 || lane < Q;
  float2 v[PER][4];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = lane + 64 * i;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[i][r] = on ? buf[j + r * Q] : make_float2(0.f, 0.f);
  }
  wave_sync();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = lane + 64 * i;
    const int k = j & (Ns - 1);
    float2 v0 = v[i][0], v1 = v[i][1], v2 = v[i][2], v3 = v[i][3];
    if (Ns > 1 && on) {
      const int t = k * (M / (4 * Ns));
      v1 = cmul(v1, tw[t]);
      v2 = cmul(v2, tw[2 * t]);
      v3 = cmul(v3, tw[3 * t]);
    }
    const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y), a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
    const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y);
    const float2 a3 = make_float2(v1.y - v3.y, v3.x - v1.x);  // -i (v1 - v3)
    const int j0 = ((j - k) << 2) + k;
    if (on) {
      buf[j0] = make_float2(a0.x + a2.x, a0.y + a2.y);
      buf[j0 + Ns] = make_float2(a1.x + a3.x, a1.y + a3.y);
      buf[j0 + 2 * Ns] = make_float2(a0.x - a2.x, a0.y - a2.y);
      buf[j0 + 3 * Ns] = make_float2(a1.x - a3.x, a1.y - a3.y);
    }
  }
  wave_sync();
}

template <int M, int Ns>
__device__ __forceinline__ void fft_stages4(float2* buf, const float2* tw, int lane) {
  if constexpr (Ns < M) {
    fft_stage4<M, Ns>(buf, tw, lane);
    fft_stages4<M, Ns * 4>(buf, tw, lane);
  }
}

// M-point forward FFT of buf, in place, natural order in and out
template <int M>
__device__ __forceinline__ void fft_forward(float2* buf, const float2* tw, int lane) {
  if constexpr (M == 128 || M == 512) {  // 2 * 4^a: the odd stage first, where it needs no twiddle
    fft_stage2<M>(buf, lane);
    fft_stages4<M, 2>(buf, tw, lane);
  } else {
    fft_stages4<M, 1>(buf, tw, lane);
  }
}

// Z = FFT of z[m] = x[2m] + i x[2m+1] in buf -> the power |X[k]|^2, k = 0..M, of the N-point real FFT as
// floats in the same buffer: X[k] = E + W^k O, X[M-k] = conj(E - W^k O), E = (Z[k] + conj Z[M-k]) / 2,
// O = -i (Z[k] - conj Z[M-k]) / 2, W = exp(-2 pi i / N)
template <int M>
__device__ __forceinline__ void real_split_power(float2* buf, const float2* twn, int lane) {
  constexpr int PER = M / 128;
  float2 zk[PER], zm[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = lane + 64 * i;
    zk[i] = buf[k];
    zm[i] = buf[(M - k) & (M - 1)];
  }
  const float2 zh = buf[M / 2];
  wave_sync();
  float* P = reinterpret_cast<float*>(buf);
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = lane + 64 * i;
    const float2 e = make_float2(0.5f * (zk[i].x + zm[i].x), 0.5f * (zk[i].y - zm[i].y));
    const float2 o = make_float2(0.5f * (zk[i].y + zm[i].y), 0.5f * (zm[i].x - zk[i].x));
    const float2 t = cmul(twn[k], o);
    const float2 xa = make_float2(e.x + t.x, e.y + t.y), xb = make_float2(e.x - t.x, e.y - t.y);
    P[k] = fmaf(xa.x, xa.x, xa.y * xa.y);
    P[M - k] = fmaf(xb.x, xb.x, xb.y * xb.y);
  }
  if (lane == 0) P[M / 2] = fmaf(zh.x, zh.x, zh.y * zh.y);  // W^(M/2) = -i: |X[M/2]| = |Z[M/2]|
  wave_sync();
}

struct LogmelLaunch {
  const char* table;
  const float* wave;
  void* out;
  int32_t* flags;
  long long n_samples;
  int runs, frame0, n_frames, hop, pad, compress, out_f32;
  float amin, floor_db, log_scale;
};

template <int N>
__global__ __launch_bounds__(256) void k_logmel(const LogmelLaunch a) {
  constexpr int M = N / 2, H = M / 2 + 1, WCAP = N + 2;
  __shared__ float2 s_twm[M];
  __shared__ float2 s_twn[H];
  __shared__ float s_w[WCAP];
  __shared__ float2 s_buf[4][M];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float2* win = reinterpret_cast<const float2*>(a.table + kLogmelHeaderBytes);
  const float2* twm = win + M;
  const float2* twn = twm + M;
  const int* rng = reinterpret_cast<const int*>(twn + H);
  const float* wts = reinterpret_cast<const float*>(rng + 3 * DCUE_N_MELS);
  for (int i = tid; i < M; i += 256) s_twm[i] = twm[i];
  for (int i = tid; i < H; i += 256) s_twn[i] = twn[i];
  for (int i = tid; i < WCAP; i += 256) s_w[i] = wts[i];
  __syncthreads();

  const long long clip = blockIdx.x / a.runs;
  const int run = blockIdx.x % a.runs;
  // this lane's two mel bins; a table that was never initialised cannot send a read outside the LDS
  int mf[2], mc[2], mo[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int bin = lane + 64 * h;
    mf[h] = rng[bin];
    mc[h] = rng[DCUE_N_MELS + bin];
    mo[h] = rng[2 * DCUE_N_MELS + bin];
    if (mf[h] < 0 || mc[h] < 0 || mo[h] < 0 || mf[h] + mc[h] > M + 1 || mo[h] + mc[h] > WCAP) mf[h] = mc[h] = mo[h] = 0;
  }
  const float* x = a.wave + clip * a.n_samples;
  const int ns = (int)a.n_samples;
  float2* buf = s_buf[wv];
  const float* P = reinterpret_cast<const float*>(buf);
  bool bad = false;
  const int end = min(a.n_frames, (run + 1) * kLogmelFramesPerWg);
  for (int fr = run * kLogmelFramesPerWg + wv; fr < end; fr += 4) {
    const int start = (a.frame0 + fr) * a.hop - a.pad;
#pragma unroll
    for (int i = 0; i < M / 64; ++i) {
      const int m = lane + 64 * i;
      int i0 = start + 2 * m, i1 = i0 + 1;
      // reflect-pad: sample -i is sample i, sample ns - 1 + i is sample ns - 1 - i (one fold is enough:
      // the host checked pad < ns)
      i0 = i0 < 0 ? -i0 : i0;
      i1 = i1 < 0 ? -i1 : i1;
      i0 = i0 >= ns ? 2 * (ns - 1) - i0 : i0;
      i1 = i1 >= ns ? 2 * (ns - 1) - i1 : i1;
      const float s0 = x[i0], s1 = x[i1];
      bad |= !(isfinite(s0) && isfinite(s1));
      const float2 w = win[m];
      buf[m] = make_float2(s0 * w.x, s1 * w.y);
    }
    wave_sync();
    fft_forward<M>(buf, s_twm, lane);
    real_split_power<M>(buf, s_twn, lane);
    const long long row = ((clip * a.n_frames + fr) << 7);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float acc = 0.f;
      for (int i = 0; i < mc[h]; ++i) acc = fmaf(s_w[mo[h] + i], P[mf[h] + i], acc);  // ascending: one fixed order
      float v = acc;
      if (a.compress == DCUE_LOGMEL_DB)
        v = acc <= a.amin ? a.floor_db : 10.f * log10f(acc);
      else if (a.compress == DCUE_LOGMEL_LOG1P)
        v = log1pf(a.log_scale * sqrtf(acc));
      const long long o = row + lane + 64 * h;
      if (a.out_f32)
        static_cast<float*>(a.out)[o] = v;
      else
        static_cast<__half*>(a.out)[o] = __float2half(v);
    }
    wave_sync();  // the next frame's samples overwrite the power
  }
  if (bad) atomicOr(&a.flags[clip], DCUE_LOGMEL_FLAG_NONFINITE);
}

static int logmel_fail(const char* why) {
  set_last_message(why);
  return DCUE_ERR_INVALID;
}

static int logmel_check(const dcue_logmel_config* c) {
  if (!c) return logmel_fail("dcue_logmel: null config");
  if (c->n_fft != 256 && c->n_fft != 512 && c->n_fft != 1024 && c->n_fft != 2048)
    return logmel_fail("dcue_logmel: n_fft must be 256, 512, 1024 or 2048");
  if (c->hop < 1 || c->hop > c->n_fft) return logmel_fail("dcue_logmel: hop must be in 1..n_fft");
  if (c->sample_rate < 1) return logmel_fail("dcue_logmel: sample_rate must be positive");
  if (c->center != 0 && c->center != 1) return logmel_fail("dcue_logmel: center must be 0 or 1");
  if (!(c->fmin >= 0.f) || !(c->fmax <= 0.5f * (float)c->sample_rate) || !(c->fmin < c->fmax))
    return logmel_fail("dcue_logmel: need 0 <= fmin < fmax <= sample_rate / 2");
  if (c->compress != DCUE_LOGMEL_POWER && c->compress != DCUE_LOGMEL_DB && c->compress != DCUE_LOGMEL_LOG1P)
    return logmel_fail("dcue_logmel: unknown compress mode");
  if (c->compress == DCUE_LOGMEL_DB && !(c->amin > 0.f)) return logmel_fail("dcue_logmel: amin must be > 0 for DB");
  if (c->compress == DCUE_LOGMEL_LOG1P && !(c->log_scale >= 0.f) )
    return logmel_fail("dcue_logmel: log_scale must be >= 0 for LOG1P");
  if (c->out_dtype != 0 && c->out_dtype != 1) return logmel_fail("dcue_logmel: out_dtype must be 0 (fp16) or 1 (fp32)");
  return DCUE_OK;
}

static double hz_to_mel(double f) {
  const double f_sp = 200.0 / 3.0;
  if (f < 1000.0) return f / f_sp;
  return 1000.0 / f_sp + log(f / 1000.0) / (log(6.4) / 27.0);
}

static double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3.0, min_log_mel = 1000.0 / f_sp;
  if (m < min_log_mel) return f_sp * m;
  return 1000.0 * exp((log(6.4) / 27.0) * (m - min_log_mel));
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_logmel_frames(const dcue_logmel_config* cfg, int64_t n_samples, int64_t* n_frames_host) {
  TRY(logmel_check(cfg));
  if (!n_frames_host) return logmel_fail("dcue_logmel_frames: null output");
  const int64_t pad = cfg->center ? cfg->n_fft / 2 : 0;
  if (cfg->center ? n_samples <= pad : n_samples < cfg->n_fft)
    return logmel_fail(cfg->center ? "dcue_logmel: center = 1 needs n_samples > n_fft / 2 (the reflection)"
                                   : "dcue_logmel: center = 0 needs n_samples >= n_fft");
  *n_frames_host = 1 + (n_samples + 2 * pad - cfg->n_fft) / cfg->hop;
  return DCUE_OK;
}

int dcue_logmel_table_bytes(const dcue_logmel_config* cfg, size_t* bytes_host) {
  TRY(logmel_check(cfg));
  if (!bytes_host) return logmel_fail("dcue_logmel_table_bytes: null output");
  *bytes_host = logmel_table_size(cfg->n_fft);
  return DCUE_OK;
}

int dcue_logmel_table_fill_host(const dcue_logmel_config* cfg, void* table_host, size_t bytes) {
  TRY(logmel_check(cfg));
  const int N = cfg->n_fft, M = N / 2, H = M / 2 + 1;
  if (!table_host || bytes < logmel_table_size(N)) return logmel_fail("dcue_logmel_table_fill_host: table too small");
  char* base = static_cast<char*>(table_host);
  memset(base, 0, logmel_table_size(N));
  int32_t* hdr = reinterpret_cast<int32_t*>(base);
  float* win = reinterpret_cast<float*>(base + kLogmelHeaderBytes);
  float* twm = win + N;
  float* twn = twm + 2 * M;
  int32_t* rng = reinterpret_cast<int32_t*>(twn + 2 * H);
  float* wts = reinterpret_cast<float*>(rng + 3 * DCUE_N_MELS);
  const double two_pi = 2.0 * M_PI;
  for (int n = 0; n < N; ++n) win[n] = (float)(0.5 - 0.5 * cos(two_pi * n / N));
  for (int t = 0; t < M; ++t) {
    twm[2 * t] = (float)cos(two_pi * t / M);
    twm[2 * t + 1] = (float)-sin(two_pi * t / M);
  }
  for (int k = 0; k < H; ++k) {
    twn[2 * k] = (float)cos(two_pi * k / N);
    twn[2 * k + 1] = (float)-sin(two_pi * k / N);
  }
  // Slaney mel scale, triangles with area normalisation (librosa's defaults)
  double f[DCUE_N_MELS + 2];
  const double m0 = hz_to_mel((double)cfg->fmin), m1 = hz_to_mel((double)cfg->fmax);
  const double step = (m1 - m0) / (DCUE_N_MELS + 1);
  for (int i = 0; i < DCUE_N_MELS + 2; ++i) f[i] = mel_to_hz(m0 + i * step);
  int nw = 0;
  for (int i = 0; i < DCUE_N_MELS; ++i) {
    const double norm = 2.0 / (f[i + 2] - f[i]);
    int first = 0, count = 0;
    for (int k = 0; k <= M; ++k) {
      const double fk = (double)k * (double)cfg->sample_rate / N;
      const double lower = (fk - f[i]) / (f[i + 1] - f[i]), upper = (f[i + 2] - fk) / (f[i + 2] - f[i + 1]);
      const double w = fmax(0.0, fmin(lower, upper)) * norm;
      if (w > 0.0) {
        if (!count) first = k;
        if (nw >= N + 2) return logmel_fail("dcue_logmel_table_fill_host: filter weights exceed the table");
        wts[nw++] = (float)w;
        ++count;
      }
    }
    rng[i] = first;
    rng[DCUE_N_MELS + i] = count;
    rng[2 * DCUE_N_MELS + i] = nw - count;
  }
  hdr[0] = kLogmelMagic;
  hdr[1] = N;
  hdr[2] = nw;
  return DCUE_OK;
}

int dcue_logmel_table_init(const dcue_logmel_config* cfg, void* table_dev, size_t bytes, void* stream) {
  TRY(logmel_check(cfg));
  const size_t need = logmel_table_size(cfg->n_fft);
  if (!table_dev || bytes < need) return logmel_fail("dcue_logmel_table_init: table too small");
  std::vector<char> host(need);
  TRY(dcue_logmel_table_fill_host(cfg, host.data(), need));
  // the staging vector dies with this call: wait for the copy
  DCUE_HIP_CHECK(hipMemcpyAsync(table_dev, host.data(), need, hipMemcpyHostToDevice, (hipStream_t)stream));
  DCUE_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return DCUE_OK;
}

int dcue_logmel(const dcue_logmel_config* cfg, const void* table_dev, const float* wave, int64_t n_clips,
                int64_t n_samples, int64_t frame0, int32_t n_frames, void* out, int32_t* flags, void* stream) {
  int64_t total = 0;
  TRY(dcue_logmel_frames(cfg, n_samples, &total));
  if (n_clips < 0 || n_frames < 0 || frame0 < 0) return logmel_fail("dcue_logmel: negative n_clips, n_frames or frame0");
  if (frame0 + (int64_t)n_frames > total)
    return logmel_fail("dcue_logmel: the frame range reaches past the clip's frame count (no silent padding)");
  if (n_samples > INT32_MAX - 4 * (int64_t)cfg->n_fft) {
    set_last_message("dcue_logmel: n_samples beyond the 32-bit sample index");
    return DCUE_ERR_UNSUPPORTED;
  }
  if (n_clips == 0) return DCUE_OK;
  if (!flags) return logmel_fail("dcue_logmel: null pointer");
  if (n_frames == 0) {  // nothing to write, but the flags are this call's
    DCUE_HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)n_clips, (hipStream_t)stream));
    return DCUE_OK;
  }
  if (!table_dev || !wave || !out) return logmel_fail("dcue_logmel: null pointer");
  const int runs = (n_frames + kLogmelFramesPerWg - 1) / kLogmelFramesPerWg;
  if (n_clips > (int64_t)INT32_MAX / runs) {
    set_last_message("dcue_logmel: n_clips * frame runs beyond the grid limit");
    return DCUE_ERR_UNSUPPORTED;
  }
  DCUE_HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)n_clips, (hipStream_t)stream));
  LogmelLaunch a;
  a.table = static_cast<const char*>(table_dev);
  a.wave = wave;
  a.out = out;
  a.flags = flags;
  a.n_samples = n_samples;
  a.runs = runs;
  a.frame0 = (int)frame0;
  a.n_frames = n_frames;
  a.hop = cfg->hop;
  a.pad = cfg->center ? cfg->n_fft / 2 : 0;
  a.compress = cfg->compress;
  a.out_f32 = cfg->out_dtype;
  a.amin = cfg->amin;
  a.floor_db = cfg->compress == DCUE_LOGMEL_DB ? (float)(10.0 * log10((double)cfg->amin)) : 0.f;
  a.log_scale = cfg->log_scale;
  const dim3 grid((unsigned)(n_clips * runs)), block(256);
  switch (cfg->n_fft) {
    case 256: DCUE_LAUNCH(k_logmel<256>, grid, block, 0, (hipStream_t)stream, a); break;
    case 512: DCUE_LAUNCH(k_logmel<512>, grid, block, 0, (hipStream_t)stream, a); break;
    case 1024: DCUE_LAUNCH(k_logmel<1024>, grid, block, 0, (hipStream_t)stream, a); break;
    default: DCUE_LAUNCH(k_logmel<2048>, grid, block, 0, (hipStream_t)stream, a); break;
  }
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

}  // extern "C"
