// What the frame kernels share around their own arithmetic (multiscale_crop.hip, frame_resize.hip, spatial_sample.hip and
// frames_to_clip of randaug.hip): the normalisation they take, the tile a workgroup owns, the writers of a thread's four neighbouring
// outputs, and the host-side checks of their tables.  The resampling itself is each file's own.
//
// Output path.  A workgroup of FRAME_THREADS threads owns FRAME_TR x FRAME_TC outputs of one frame; a thread owns four neighbouring
// columns of one row (`valid` of them inside the frame: the last tile of a row is ragged) for all three channels.  They leave as
//   store_clip_f32x4    the f32 clip [B, 3, T, S_h, S_w]: one 16-byte store per channel plane where the thread has all four columns
//                       and the plane address allows it (a clip at any 4-byte aligned base: a view, a ring slot), else scalar stores
//   store_frames_u8x4   uint8 frames [B, T, S_h, S_w, 3]: twelve bytes as three word stores where the address allows it (S_w * 3 and a
//                       slice of a frame store break every alignment), else byte stores
// and nothing is written past `valid` columns.  The crop and the resize state the f32 values with frame_norm8 (frames_to_clip's value
// of a byte) in front of store_clip_f32x4; the spatial sampling hands it its blends.
#pragma once
#include "common.h"
#include <math.h>

TAD_NAMESPACE_BEGIN

// per-channel mean and std of normalize_u8 (common.h); a kernel argument: 24 bytes, mean first
struct ClipNorm {
  float mean[3], sd[3];
};

constexpr int FRAME_THREADS = 256;
constexpr int FRAME_TR = 32, FRAME_TC = 32;  // output rows x columns of a tile
constexpr int FRAME_CG = FRAME_TC / 4;       // column groups of four per tile row: one thread each
static_assert(FRAME_TR * FRAME_CG == FRAME_THREADS, "tile shape");

__device__ __forceinline__ int frame_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the byte of a 22-bit fixed-point sum (the rounding constant 1 << 21 is in it already)
__device__ __forceinline__ uint32_t frame_clip8(int ss) { return (uint32_t)frame_clamp(ss >> 22, 0, 255); }

// v[ch][0 .. valid) to o + ch * plane: `o` is the thread's first column in the plane of channel 0, `plane` = T * S_h * S_w
__device__ __forceinline__ void store_clip_f32x4(float* o, int64_t plane, const float (&v)[3][4], int valid) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* oc = o + ch * plane;
    if (valid == 4 && (reinterpret_cast<uintptr_t>(oc) & 15) == 0) {
      *reinterpret_cast<float4*>(oc) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < valid) oc[q] = v[ch][q];
    }
  }
}

// frames_to_clip's value (normalize_u8) of the byte of a 22-bit sum: what the crop and the resize hand to store_clip_f32x4
__device__ __forceinline__ float frame_norm8(int ss, float mean, float sd) { return normalize_u8((float)frame_clip8(ss), mean, sd); }

// the bytes of the 22-bit sums acc[ch][0 .. valid) as RGB pixels from `o`, the thread's first pixel
__device__ __forceinline__ void store_frames_u8x4(uint8_t* o, const int (&acc)[3][4], int valid) {
  uint32_t pk[3] = {0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) pk[(3 * q + ch) >> 2] |= frame_clip8(acc[ch][q]) << (((3 * q + ch) & 3) * 8);
  if (valid == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) reinterpret_cast<uint32_t*>(o)[i] = pk[i];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < 3 * valid) o[i] = (uint8_t)(pk[i >> 2] >> ((i & 3) * 8));
  }
}

// ---------------------------------------------------------------- host side: `who` is the entry point's name in its messages
// the tiles of an S_h x S_w output: blockIdx.x of a launch, tile (blockIdx.x / tiles_x, blockIdx.x % tiles_x)
static inline unsigned frame_tile_grid(int Sh, int Sw, int* tiles_x) {
  *tiles_x = (Sw + FRAME_TC - 1) / FRAME_TC;
  return (unsigned)(*tiles_x * ((Sh + FRAME_TR - 1) / FRAME_TR));
}

// mean and std of the three channels into nm: finite, and no std of zero
static inline int clip_norm_from(const char* who, const float* mean, const float* std_, ClipNorm* nm) {
  for (int c = 0; c < 3; ++c) {
    TAD_REQUIRE(std::isfinite(mean[c]) && std::isfinite(std_[c]) && std_[c] != 0.0f, "%s: mean / std of channel %d", who, c);
    nm->mean[c] = mean[c], nm->sd[c] = std_[c];
  }
  return TAD_OK;
}
constexpr ClipNorm CLIP_NORM_IDENTITY = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};

static inline int frame_extent_ok(const char* who, int H, int W) {
  TAD_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 28), "%s: H=%d W=%d: a frame must have 1 .. 2^28 pixels", who, H, W);
  return TAD_OK;
}

// the table a launch reads is its workspace: int32 words, `need` bytes of them (non-null is the caller's to say)
static inline int table_workspace_ok(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
  TAD_REQUIRE_ALIGNED(who, workspace, 4);
  TAD_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, need);
  return TAD_OK;
}

// "every sample has one row" of a plan check: the samples met so far, of at most 65 535 (the bound on B, or B * T, of every table)
struct SeenSamples {
  uint64_t seen[1024] = {0};
  bool twice(int sample) {  // (0 <= sample <= 65535 is the caller's to check first)
    const bool was = seen[sample >> 6] >> (sample & 63) & 1;
    seen[sample >> 6] |= (uint64_t)1 << (sample & 63);
    return was;
  }
};

TAD_NAMESPACE_END
