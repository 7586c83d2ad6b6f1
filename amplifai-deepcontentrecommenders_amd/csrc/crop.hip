// Window crops of full-length tracks (include/dcue.h, dcue_crop_tracks): a ragged store
// [total_frames][128] plus frame_ptr -> a [n_out][131][128] track table, one window per track by a
// counter-based rule. Source and destination of a crop are each one contiguous span of 131 * 128
// elements, so this is a batched, offset, zero-tailed copy: 16-byte loads and stores, no LDS, no
// workspace, nothing but the store and the table touched.
//
// A unit of work is one part of one output row; a workgroup takes units blockIdx.x, blockIdx.x +
// gridDim.x, ... Everything that places a unit (rows[i], the two frame_ptr entries, the hash, the
// start) depends on the unit alone, so it is uniform over the workgroup: the compiler keeps it in
// scalar registers and no lane repeats it. The host cuts a row into `parts` so that a few dozen rows
// still give every CU a workgroup, and caps the grid so that 200,000 rows run as 2,048 resident
// workgroups striding over the table.
#include <stdio.h>

#include <cmath>

#include "dcue_common.h"
#include "dcue_internal.h"
#include "mix64.h"

namespace dcue {

constexpr int kCropChunk = 8;                                   // elements a lane moves at a time
constexpr int kCropChunks = kFrames * kMels / kCropChunk;       // 2,096 per row
constexpr int kCropChunksPerFrame = kMels / kCropChunk;         // 16
constexpr int kCropMaxParts = 16;
constexpr long long kCropTargetUnits = 1024;                    // 4 workgroups on each of 256 CUs
constexpr unsigned kCropMaxGrid = 2048;                         // 8 x 256 lanes on each CU: full occupancy

// The window rule of include/dcue.h for a track of L > W frames at index t of the store.
__host__ __device__ __forceinline__ long long crop_start(const dcue_crop_config& c, long long L, long long t) {
  const long long span = L - kFrames;
  if (span <= 0) return 0;
  switch (c.mode) {
    case DCUE_CROP_CENTER: return span / 2;
    case DCUE_CROP_GRID: return c.grid_n == 1 ? span / 2 : (long long)c.grid_j * span / (c.grid_n - 1);
    case DCUE_CROP_RANDOM: {
      const unsigned long long z0 = mix64(c.seed + kGolden64 * (unsigned long long)(t + 1));
      const unsigned long long h = mix64(z0 + kGolden64 * (c.draw + 1));
      return (long long)mulhi64(h, (unsigned long long)span);
    }
    default: return 0;  // DCUE_CROP_FIRST
  }
}

struct CropArgs {
  dcue_crop_config cfg;
  const void* data;
  void* out;
  int32_t* starts;
  int32_t* flags;
  long long n_tracks, total_frames, units;
  int parts;
};

// kCropChunk elements as 16-byte vectors: one uint4 of fp16, two float4 of fp32
template <typename T>
struct Chunk;
template <>
struct Chunk<__half> {
  uint4 v;
  static __device__ __forceinline__ Chunk load(const __half* p) { return {*reinterpret_cast<const uint4*>(p)}; }
  __device__ __forceinline__ void store(__half* p) const { *reinterpret_cast<uint4*>(p) = v; }
  static __device__ __forceinline__ Chunk zero() { return {make_uint4(0u, 0u, 0u, 0u)}; }
};
template <>
struct Chunk<float> {
  float4 lo, hi;
  static __device__ __forceinline__ Chunk load(const float* p) {
    return {reinterpret_cast<const float4*>(p)[0], reinterpret_cast<const float4*>(p)[1]};
  }
  __device__ __forceinline__ void store(float* p) const {
    reinterpret_cast<float4*>(p)[0] = lo;
    reinterpret_cast<float4*>(p)[1] = hi;
  }
  static __device__ __forceinline__ Chunk zero() { return {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)}; }
};

__device__ __forceinline__ Chunk<__half> crop_convert(const Chunk<__half>& s, const __half*) { return s; }
__device__ __forceinline__ Chunk<float> crop_convert(const Chunk<float>& s, const float*) { return s; }
__device__ __forceinline__ Chunk<float> crop_convert(const Chunk<__half>& s, const float*) {  // exact
  const __half2 h0 = *reinterpret_cast<const __half2*>(&s.v.x), h1 = *reinterpret_cast<const __half2*>(&s.v.y);
  const __half2 h2 = *reinterpret_cast<const __half2*>(&s.v.z), h3 = *reinterpret_cast<const __half2*>(&s.v.w);
  const float2 a = __half22float2(h0), b = __half22float2(h1), c = __half22float2(h2), e = __half22float2(h3);
  return {make_float4(a.x, a.y, b.x, b.y), make_float4(c.x, c.y, e.x, e.y)};
}
__device__ __forceinline__ unsigned crop_pack(float x, float y) {  // round to nearest even
  const __half2 h = __floats2half2_rn(x, y);
  return *reinterpret_cast<const unsigned*>(&h);
}
__device__ __forceinline__ Chunk<__half> crop_convert(const Chunk<float>& s, const __half*) {
  return {make_uint4(crop_pack(s.lo.x, s.lo.y), crop_pack(s.lo.z, s.lo.w), crop_pack(s.hi.x, s.hi.y),
                     crop_pack(s.hi.z, s.hi.w))};
}

// frame_ptr and rows are kernel arguments of their own: as restrict-qualified read-only pointers their
// loads (uniform addresses) go through the scalar cache, once per wave instead of once per lane
template <typename S, typename D>
__global__ __launch_bounds__(256) void k_crop_tracks(const CropArgs a, const long long* __restrict__ fp,
                                                     const int32_t* __restrict__ rows) {
  for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
    const long long i = u / a.parts;
    const int part = (int)(u - i * a.parts);
    const long long t = rows ? (long long)rows[i] : i;
    int bits = 0;
    long long lo = 0, L = 0;
    if (t < 0 || t >= a.n_tracks) {
      bits = DCUE_CROP_FLAG_BAD_ROW;
    } else {
      lo = fp[t];
      const long long hi = fp[t + 1];
      if (lo < 0 || hi < lo || hi > a.total_frames)
        bits = DCUE_CROP_FLAG_BAD_EXTENT;
      else
        L = hi - lo;
    }
    if (bits) lo = 0;  // a flagged row has L = 0: nothing is read, the whole row is the zero tail
    const long long start = crop_start(a.cfg, L, t);
    const int valid = (int)(L < kFrames ? L : kFrames) * kCropChunksPerFrame;  // chunks that hold data
    const S* __restrict__ src = static_cast<const S*>(a.data) + (lo + start) * kMels;
    D* __restrict__ dst = static_cast<D*>(a.out) + i * (long long)(kFrames * kMels);
    const int c0 = kCropChunks * part / a.parts, c1 = kCropChunks * (part + 1) / a.parts;
#pragma unroll 4
    for (int c = c0 + (int)threadIdx.x; c < c1; c += 256) {
      const Chunk<D> d = c < valid ? crop_convert(Chunk<S>::load(src + c * kCropChunk), dst) : Chunk<D>::zero();
      d.store(dst + c * kCropChunk);
    }
    if (part == 0 && threadIdx.x == 0) {
      a.flags[i] = bits;
      if (a.starts) a.starts[i] = (int32_t)start;
    }
  }
}

// ---------------------------------------------------------------------------------- augmentation
// dcue_crop_tracks_augmented (include/dcue.h has the rule): the same units, with a mask, a gain and a
// fill applied between the load and the store. What the rule gives a track -- the gain, the masks'
// places and widths -- is uniform over the workgroup like the start, and stays in scalar registers.
//
// The MEAN fill needs the row's sum before the first masked element can be written. When a row is one
// unit (parts == 1) a lane keeps its 8-9 chunks in registers while the workgroup reduces the sum, so
// the row is still read once; when a row is cut into parts (few rows, traffic irrelevant) every part
// sums the whole window and then loads its own share again. The sum is an int64 in units of 2^-24,
// the spacing of fp16's subnormals, so it is exact and the same for any split or reduction tree.
constexpr int kAugHeld = (kCropChunks + 255) / 256;  // 9 chunks a lane, the last one on 48 lanes

struct AugTrack {  // what the rule gives one track
  float gain;
  int fp[DCUE_AUG_MAX_MASKS], fw[DCUE_AUG_MAX_MASKS];  // frequency masks: bins [fp, fp + fw)
  int tp[DCUE_AUG_MAX_MASKS], tw[DCUE_AUG_MAX_MASKS];  // time masks: frames [tp, tp + tw)
};

__host__ __device__ __forceinline__ unsigned long long crop_hash(const dcue_crop_config& c, long long t) {
  const unsigned long long z0 = mix64(c.seed + kGolden64 * (unsigned long long)(t + 1));
  return mix64(z0 + kGolden64 * (c.draw + 1));
}

__host__ __device__ __forceinline__ unsigned long long aug_r(unsigned long long h, int i) {
  return mix64(h + kGolden64 * (unsigned long long)(i + 1));
}

// every fp32 operation of the rule rounds on its own: no fma may form from the gain's product and the
// element's add, whatever -ffp-contract the file is built with
__host__ __device__ __forceinline__ float aug_gain(float gain_db, unsigned long long r0) {
#pragma clang fp contract(off)
  const float u = (float)(unsigned)(r0 >> 40) * 0x1p-23f;  // exact
  const float c = u - 1.0f;                                // exact
  return gain_db * c;
}
__host__ __device__ __forceinline__ float aug_add(float x, float g) {
#pragma clang fp contract(off)
  return x + g;
}

// n: the valid frames of the row, min(L, 131)
__host__ __device__ __forceinline__ AugTrack aug_track(const dcue_augment_config& g, unsigned long long h, int n) {
  AugTrack a;
  a.gain = aug_gain(g.gain_db, aug_r(h, 0));
#pragma unroll
  for (int j = 0; j < DCUE_AUG_MAX_MASKS; ++j) {
    a.fp[j] = a.fw[j] = a.tp[j] = a.tw[j] = 0;
    if (j < g.n_freq) {
      a.fw[j] = (int)mulhi64(aug_r(h, 1 + 2 * j), (unsigned long long)(g.freq_width + 1));
      a.fp[j] = (int)mulhi64(aug_r(h, 2 + 2 * j), (unsigned long long)(kMels - a.fw[j] + 1));
    }
    if (j < g.n_time) {
      const int w = (int)mulhi64(aug_r(h, 1 + 2 * DCUE_AUG_MAX_MASKS + 2 * j), (unsigned long long)(g.time_width + 1));
      a.tw[j] = w < n ? w : n;
      a.tp[j] = (int)mulhi64(aug_r(h, 2 + 2 * DCUE_AUG_MAX_MASKS + 2 * j), (unsigned long long)(n - a.tw[j] + 1));
    }
  }
  return a;
}

// bits [a, b) of a 64-bit word, for a and b anywhere
__device__ __forceinline__ unsigned long long aug_bits(int a, int b) {
  a = a < 0 ? 0 : a;
  b = b > 64 ? 64 : b;
  if (b <= a) return 0ull;
  const unsigned long long upto = b == 64 ? ~0ull : (1ull << b) - 1ull;
  return upto & ~((1ull << a) - 1ull);
}

struct AugRow {  // a track's parameters as the element loop uses them
  unsigned long long fm0, fm1;  // the union of the frequency masks, a bit per mel bin
  int tp[DCUE_AUG_MAX_MASKS], tw[DCUE_AUG_MAX_MASKS];
  float gain, fill;
  unsigned fill_h2;  // the fill as two fp16
  bool gain_on;
};

// the fp16 value of bit pattern hb in units of 2^-24, added to acc; bad if it is not finite
__device__ __forceinline__ void aug_sum_half(unsigned hb, long long& acc, int& bad) {
  const int e = (int)(hb >> 10) & 31;
  const long long m = (long long)(hb & 1023u);
  const long long v = e ? (1024 + m) << (e - 1) : m;
  bad |= e == 31;
  acc += (hb & 0x8000u) ? -v : v;
}
__device__ __forceinline__ void aug_sum(const Chunk<__half>& s, long long& acc, int& bad) {
  const unsigned w[4] = {s.v.x, s.v.y, s.v.z, s.v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    aug_sum_half(w[k] & 0xFFFFu, acc, bad);
    aug_sum_half(w[k] >> 16, acc, bad);
  }
}
__device__ __forceinline__ void aug_sum(const Chunk<float>& s, long long& acc, int& bad) {  // rounded to fp16 first
  aug_sum(crop_convert(s, static_cast<const __half*>(nullptr)), acc, bad);
}

__device__ __forceinline__ void aug_fill(Chunk<__half>& d, unsigned m8, const AugRow& r) {
  unsigned* w[4] = {&d.v.x, &d.v.y, &d.v.z, &d.v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned sel = ((m8 >> (2 * k)) & 1u ? 0xFFFFu : 0u) | ((m8 >> (2 * k + 1)) & 1u ? 0xFFFF0000u : 0u);
    *w[k] = (*w[k] & ~sel) | (r.fill_h2 & sel);
  }
}
__device__ __forceinline__ void aug_fill(Chunk<float>& d, unsigned m8, const AugRow& r) {
  float* f[8] = {&d.lo.x, &d.lo.y, &d.lo.z, &d.lo.w, &d.hi.x, &d.hi.y, &d.hi.z, &d.hi.w};
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if ((m8 >> k) & 1u) *f[k] = r.fill;
}

// chunk c of a row (c below the row's valid chunks): gain, then the masks
template <typename S, typename D>
__device__ __forceinline__ Chunk<D> aug_chunk(const Chunk<S>& s, int c, const AugRow& r, const D* tag) {
  Chunk<D> d;
  if (r.gain_on) {
    Chunk<float> f = crop_convert(s, static_cast<const float*>(nullptr));
    f.lo.x = aug_add(f.lo.x, r.gain); f.lo.y = aug_add(f.lo.y, r.gain);
    f.lo.z = aug_add(f.lo.z, r.gain); f.lo.w = aug_add(f.lo.w, r.gain);
    f.hi.x = aug_add(f.hi.x, r.gain); f.hi.y = aug_add(f.hi.y, r.gain);
    f.hi.z = aug_add(f.hi.z, r.gain); f.hi.w = aug_add(f.hi.w, r.gain);
    d = crop_convert(f, tag);
  } else {
    d = crop_convert(s, tag);
  }
  const int frame = c / kCropChunksPerFrame, q = c % kCropChunksPerFrame;  // q: which 8 bins of the frame
  unsigned m8 = (unsigned)((q < 8 ? r.fm0 : r.fm1) >> ((q & 7) * kCropChunk)) & 0xFFu;
#pragma unroll
  for (int j = 0; j < DCUE_AUG_MAX_MASKS; ++j)
    if ((unsigned)(frame - r.tp[j]) < (unsigned)r.tw[j]) m8 = 0xFFu;
  if (m8) aug_fill(d, m8, r);
  return d;
}

struct AugArgs {
  CropArgs c;
  dcue_augment_config aug;
};

// kMean: the fill is the row's mean and a mask is on, so the sum is needed
template <typename S, typename D, bool kMean>
__global__ __launch_bounds__(256) void k_augment_tracks(const AugArgs a, const long long* __restrict__ fp,
                                                        const int32_t* __restrict__ rows) {
  __shared__ long long s_sum[4];
  __shared__ int s_bad[4];
  const int tid = (int)threadIdx.x;
  for (long long u = blockIdx.x; u < a.c.units; u += gridDim.x) {
    const long long i = u / a.c.parts;
    const int part = (int)(u - i * a.c.parts);
    const long long t = rows ? (long long)rows[i] : i;
    int bits = 0;
    long long lo = 0, L = 0;
    if (t < 0 || t >= a.c.n_tracks) {
      bits = DCUE_CROP_FLAG_BAD_ROW;
    } else {
      lo = fp[t];
      const long long hi = fp[t + 1];
      if (lo < 0 || hi < lo || hi > a.c.total_frames)
        bits = DCUE_CROP_FLAG_BAD_EXTENT;
      else
        L = hi - lo;
    }
    if (bits) lo = 0;  // a flagged row has L = 0: nothing is read, the whole row is the zero tail
    const long long start = crop_start(a.c.cfg, L, t);
    const int n = (int)(L < kFrames ? L : kFrames);
    const int valid = n * kCropChunksPerFrame;  // chunks that hold data
    const S* __restrict__ src = static_cast<const S*>(a.c.data) + (lo + start) * kMels;
    D* __restrict__ dst = static_cast<D*>(a.c.out) + i * (long long)(kFrames * kMels);

    const AugTrack tr = aug_track(a.aug, crop_hash(a.c.cfg, t), n);
    AugRow r;
    r.fm0 = r.fm1 = 0ull;
#pragma unroll
    for (int j = 0; j < DCUE_AUG_MAX_MASKS; ++j) {
      r.fm0 |= aug_bits(tr.fp[j], tr.fp[j] + tr.fw[j]);
      r.fm1 |= aug_bits(tr.fp[j] - 64, tr.fp[j] + tr.fw[j] - 64);
      r.tp[j] = tr.tp[j];
      r.tw[j] = tr.tw[j];
    }
    r.gain = tr.gain;
    r.gain_on = a.aug.gain_db != 0.f;
    r.fill = a.aug.fill_value;

    const bool held = kMean && a.c.parts == 1;
    Chunk<S> keep[kAugHeld];
    if (kMean) {
      long long acc = 0;
      int bad = 0;
      if (held) {
#pragma unroll
        for (int k = 0; k < kAugHeld; ++k) {
          const int c = tid + 256 * k;
          keep[k] = Chunk<S>::zero();
          if (c < valid) {
            keep[k] = Chunk<S>::load(src + c * kCropChunk);
            aug_sum(keep[k], acc, bad);
          }
        }
      } else {
        for (int c = tid; c < valid; c += 256) aug_sum(Chunk<S>::load(src + c * kCropChunk), acc, bad);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o);
        bad |= __shfl_xor(bad, o);
      }
      if ((tid & 63) == 0) {
        s_sum[tid >> 6] = acc;
        s_bad[tid >> 6] = bad;
      }
      __syncthreads();
      const long long sum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
      bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
      __syncthreads();  // the next unit writes them again
      float m = 0.f;
      if (n > 0) m = (float)((double)sum * 0x1p-24 / (double)(n * kMels));
      if (bad) m = __builtin_nanf("");
      r.fill = r.gain_on ? aug_add(m, r.gain) : m;
    }
    r.fill_h2 = crop_pack(r.fill, r.fill);

    if (held) {
#pragma unroll
      for (int k = 0; k < kAugHeld; ++k) {
        const int c = tid + 256 * k;
        if (c < kCropChunks) {
          const Chunk<D> d = c < valid ? aug_chunk(keep[k], c, r, dst) : Chunk<D>::zero();
          d.store(dst + c * kCropChunk);
        }
      }
    } else {
      const int c0 = kCropChunks * part / a.c.parts, c1 = kCropChunks * (part + 1) / a.c.parts;
#pragma unroll 2
      for (int c = c0 + tid; c < c1; c += 256) {
        const Chunk<D> d = c < valid ? aug_chunk(Chunk<S>::load(src + c * kCropChunk), c, r, dst) : Chunk<D>::zero();
        d.store(dst + c * kCropChunk);
      }
    }
    if (part == 0 && tid == 0) {
      a.c.flags[i] = bits;
      if (a.c.starts) a.c.starts[i] = (int32_t)start;
    }
  }
}

static int crop_fail(const char* why) {
  set_last_message(why);
  return DCUE_ERR_INVALID;
}

static bool aug_off(const dcue_augment_config* g) {
  return !g || (g->n_freq * g->freq_width == 0 && g->n_time * g->time_width == 0 && g->gain_db == 0.f);
}

static int aug_check(const dcue_augment_config* g) {
  if (g->n_freq < 0 || g->n_freq > DCUE_AUG_MAX_MASKS || g->n_time < 0 || g->n_time > DCUE_AUG_MAX_MASKS)
    return crop_fail("dcue_augment: n_freq and n_time must be in 0..4");
  if (g->freq_width < 0 || g->freq_width > kMels) return crop_fail("dcue_augment: freq_width must be in 0..128");
  if (g->time_width < 0 || g->time_width > kFrames) return crop_fail("dcue_augment: time_width must be in 0..131");
  if (!(g->gain_db >= 0.f) || !std::isfinite(g->gain_db))
    return crop_fail("dcue_augment: gain_db must be finite and not negative");
  if (g->fill_mode != DCUE_AUG_FILL_MEAN && g->fill_mode != DCUE_AUG_FILL_CONST)
    return crop_fail("dcue_augment: unknown fill_mode");
  if (!std::isfinite(g->fill_value)) return crop_fail("dcue_augment: fill_value must be finite");
  if (g->reserved != 0) return crop_fail("dcue_augment: reserved must be zero");
  return DCUE_OK;
}

static int crop_check(const dcue_crop_config* c) {
  if (!c) return crop_fail("dcue_crop: null config");
  if (c->mode != DCUE_CROP_FIRST && c->mode != DCUE_CROP_CENTER && c->mode != DCUE_CROP_GRID && c->mode != DCUE_CROP_RANDOM)
    return crop_fail("dcue_crop: unknown mode");
  if (c->mode == DCUE_CROP_GRID && (c->grid_n < 1 || c->grid_j < 0 || c->grid_j >= c->grid_n))
    return crop_fail("dcue_crop: GRID needs grid_n >= 1 and 0 <= grid_j < grid_n");
  return DCUE_OK;
}

static bool crop_dtype_ok(int32_t d) { return d == 0 || d == 1; }
static size_t crop_esize(int32_t d) { return d == 0 ? 2 : 4; }

template <bool kMean>
static void aug_launch(int32_t sd, int32_t od, dim3 grid, hipStream_t s, const AugArgs& a, const long long* fp,
                       const int32_t* rows) {
  const dim3 block(256);
  if (sd == 0 && od == 0)
    DCUE_LAUNCH((k_augment_tracks<__half, __half, kMean>), grid, block, 0, s, a, fp, rows);
  else if (sd == 0)
    DCUE_LAUNCH((k_augment_tracks<__half, float, kMean>), grid, block, 0, s, a, fp, rows);
  else if (od == 0)
    DCUE_LAUNCH((k_augment_tracks<float, __half, kMean>), grid, block, 0, s, a, fp, rows);
  else
    DCUE_LAUNCH((k_augment_tracks<float, float, kMean>), grid, block, 0, s, a, fp, rows);
}

}  // namespace dcue

using namespace dcue;

extern "C" {

int dcue_crop_starts_host(const dcue_crop_config* cfg, const int64_t* lengths_host, const int64_t* track_ids_host,
                          int64_t n, int64_t* starts_host) {
  TRY(crop_check(cfg));
  if (n < 0) return crop_fail("dcue_crop_starts_host: negative n");
  if (n == 0) return DCUE_OK;
  if (!lengths_host || !starts_host) return crop_fail("dcue_crop_starts_host: null pointer");
  for (int64_t i = 0; i < n; ++i) {
    if (lengths_host[i] < 0) return crop_fail("dcue_crop_starts_host: negative length");
    starts_host[i] = crop_start(*cfg, lengths_host[i], track_ids_host ? track_ids_host[i] : i);
  }
  return DCUE_OK;
}

// Everything dcue_crop_tracks refuses, then the launch shape: a->units stays 0 when there is nothing to do.
static int crop_prepare(const dcue_track_store* store, const dcue_crop_config* cfg, int64_t n_out, void* out,
                        int32_t out_dtype, int32_t* starts, int32_t* flags, CropArgs* a, dim3* grid) {
  a->units = 0;
  if (!store) return crop_fail("dcue_crop_tracks: null store");
  TRY(crop_check(cfg));
  if (store->n_tracks < 0 || store->total_frames < 0 || n_out < 0)
    return crop_fail("dcue_crop_tracks: negative n_tracks, total_frames or n_out");
  if (!crop_dtype_ok(store->dtype) || !crop_dtype_ok(out_dtype))
    return crop_fail("dcue_crop_tracks: dtype must be 0 (fp16) or 1 (fp32)");
  if (store->total_frames > (int64_t)INT32_MAX) {
    set_last_message("dcue_crop_tracks: total_frames beyond the 32-bit start index");
    return DCUE_ERR_UNSUPPORTED;
  }
  if (!out || !flags) return crop_fail("dcue_crop_tracks: null out or flags");
  if (n_out == 0) return DCUE_OK;
  if (!store->frame_ptr || (!store->data && store->total_frames > 0))
    return crop_fail("dcue_crop_tracks: null store data or frame_ptr");
  const uintptr_t src = reinterpret_cast<uintptr_t>(store->data), dst = reinterpret_cast<uintptr_t>(out);
  if ((src | dst) & 15) return crop_fail("dcue_crop_tracks: store data and out must be 16-byte aligned");
  const uintptr_t src_bytes = (uintptr_t)store->total_frames * kMels * crop_esize(store->dtype);
  const uintptr_t dst_bytes = (uintptr_t)n_out * kFrames * kMels * crop_esize(out_dtype);
  if (src < dst + dst_bytes && dst < src + src_bytes) return crop_fail("dcue_crop_tracks: out overlaps the store's data");

  int parts = 1;
  while (parts < kCropMaxParts && n_out * parts < kCropTargetUnits) parts *= 2;
  a->cfg = *cfg;
  a->data = store->data;
  a->out = out;
  a->starts = starts;
  a->flags = flags;
  a->n_tracks = store->n_tracks;
  a->total_frames = store->total_frames;
  a->units = n_out * parts;
  a->parts = parts;
  *grid = dim3((unsigned)(a->units < (long long)kCropMaxGrid ? a->units : (long long)kCropMaxGrid));
  return DCUE_OK;
}

int dcue_crop_tracks(const dcue_track_store* store, const dcue_crop_config* cfg, const int32_t* rows, int64_t n_out,
                     void* out, int32_t out_dtype, int32_t* starts, int32_t* flags, void* stream) {
  CropArgs a;
  dim3 grid;
  TRY(crop_prepare(store, cfg, n_out, out, out_dtype, starts, flags, &a, &grid));
  if (a.units == 0) return DCUE_OK;
  const dim3 block(256);
  const hipStream_t s = (hipStream_t)stream;
  const long long* fp = reinterpret_cast<const long long*>(store->frame_ptr);
  if (store->dtype == 0 && out_dtype == 0)
    DCUE_LAUNCH((k_crop_tracks<__half, __half>), grid, block, 0, s, a, fp, rows);
  else if (store->dtype == 0)
    DCUE_LAUNCH((k_crop_tracks<__half, float>), grid, block, 0, s, a, fp, rows);
  else if (out_dtype == 0)
    DCUE_LAUNCH((k_crop_tracks<float, __half>), grid, block, 0, s, a, fp, rows);
  else
    DCUE_LAUNCH((k_crop_tracks<float, float>), grid, block, 0, s, a, fp, rows);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

int dcue_crop_tracks_augmented(const dcue_track_store* store, const dcue_crop_config* cfg,
                               const dcue_augment_config* aug, const int32_t* rows, int64_t n_out, void* out,
                               int32_t out_dtype, int32_t* starts, int32_t* flags, void* stream) {
  if (aug) TRY(aug_check(aug));
  if (aug_off(aug)) return dcue_crop_tracks(store, cfg, rows, n_out, out, out_dtype, starts, flags, stream);
  AugArgs a;
  dim3 grid;
  TRY(crop_prepare(store, cfg, n_out, out, out_dtype, starts, flags, &a.c, &grid));
  if (a.c.units == 0) return DCUE_OK;
  a.aug = *aug;
  if (a.aug.freq_width == 0) a.aug.n_freq = 0;  // masks of width 0 cover nothing
  if (a.aug.time_width == 0) a.aug.n_time = 0;
  const bool masks = a.aug.n_freq > 0 || a.aug.n_time > 0;
  const long long* fp = reinterpret_cast<const long long*>(store->frame_ptr);
  if (masks && a.aug.fill_mode == DCUE_AUG_FILL_MEAN)
    aug_launch<true>(store->dtype, out_dtype, grid, (hipStream_t)stream, a, fp, rows);
  else
    aug_launch<false>(store->dtype, out_dtype, grid, (hipStream_t)stream, a, fp, rows);
  DCUE_LAUNCH_CHECK();
  return DCUE_OK;
}

int dcue_augment_params_host(const dcue_crop_config* cfg, const dcue_augment_config* aug, const int64_t* lengths_host,
                             const int64_t* track_ids_host, int64_t n, float* gain_host, int32_t* freq_pw_host,
                             int32_t* time_pw_host) {
  TRY(crop_check(cfg));
  if (!aug) return crop_fail("dcue_augment_params_host: null augment config");
  TRY(aug_check(aug));
  if (n < 0) return crop_fail("dcue_augment_params_host: negative n");
  if (n == 0) return DCUE_OK;
  if (!lengths_host) return crop_fail("dcue_augment_params_host: null lengths");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t L = lengths_host[i];
    if (L < 0) return crop_fail("dcue_augment_params_host: negative length");
    const AugTrack tr = aug_track(*aug, crop_hash(*cfg, track_ids_host ? track_ids_host[i] : i),
                                  (int)(L < kFrames ? L : kFrames));
    if (gain_host) gain_host[i] = tr.gain;
    for (int j = 0; j < DCUE_AUG_MAX_MASKS; ++j) {
      const int64_t k = (i * DCUE_AUG_MAX_MASKS + j) * 2;
      if (freq_pw_host) freq_pw_host[k] = tr.fp[j], freq_pw_host[k + 1] = tr.fw[j];
      if (time_pw_host) time_pw_host[k] = tr.tp[j], time_pw_host[k + 1] = tr.tw[j];
    }
  }
  return DCUE_OK;
}

}  // extern "C"
