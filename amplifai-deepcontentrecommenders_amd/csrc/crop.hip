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

static int crop_fail(const char* why) {
  set_last_message(why);
  return DCUE_ERR_INVALID;
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

int dcue_crop_tracks(const dcue_track_store* store, const dcue_crop_config* cfg, const int32_t* rows, int64_t n_out,
                     void* out, int32_t out_dtype, int32_t* starts, int32_t* flags, void* stream) {
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
  CropArgs a;
  a.cfg = *cfg;
  a.data = store->data;
  a.out = out;
  a.starts = starts;
  a.flags = flags;
  a.n_tracks = store->n_tracks;
  a.total_frames = store->total_frames;
  a.units = n_out * parts;
  a.parts = parts;
  const dim3 grid((unsigned)(a.units < (long long)kCropMaxGrid ? a.units : (long long)kCropMaxGrid)), block(256);
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

}  // extern "C"
