// The spatial sampling of the class fine-tuning recipe on the device (kinetics.py / ssv2.py of the reference: spatial_sampling =
// random_resized_crop, random_resized_crop_with_shift or random_short_side_scale_jitter + random_crop, then horizontal_flip; with
// spatial_idx 0 / 1 / 2 the jitter + uniform_crop of the three test-time views).  Every route is a window of the source frame, a
// bilinear resize of it (torch.nn.functional.interpolate, align_corners=False, no antialiasing: four taps per output whatever the
// scale), an S x S window of the resized grid and an optional flip.  The host draws the windows (simple_tad_amd/spatial_sampling.py);
// this file carries them out in ONE launch on the f32 clips [B, 3, T, H, W] or on uint8 frames [B, T, H, W, 3], into the f32 clips
// [B, 3, T, S, S].
//
// Table (int32, include/tad_mi355x.h documents the words): one row per (clip, frame),
//   {sample, i, j, h, w, rh, rw, oy, ox, flip, scale_y, scale_x}
// The table is only read.  The host states the scales (f32 bit patterns, (float)h / (float)rh and (float)w / (float)rw): the device
// never divides for a coordinate.
//
// Arithmetic (the contract of include/tad_mi355x.h): per axis, in f32, every product and sum rounded on its own (the file is compiled
// without floating-point contraction, build.py)
//   src = max(scale * (d + 0.5f) - 0.5f, 0);  i0 = min((int)src, n_in - 1);  i1 = min(i0 + 1, n_in - 1);  l1 = src - (float)i0;  l0 = 1 - l1
//   value = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)
// A uint8 tap first becomes frames_to_clip's normalize_u8 (common.h) of the byte; a workgroup states those 3 x 256 values once, in LDS.
//
// Shape: a gather without reuse beyond the two rows and two columns of a tap, bound by memory traffic.  A workgroup owns FRAME_TR x
// FRAME_TC outputs of one frame (frame_io.h) for all three channels; a thread owns four neighbouring output columns of one row: it
// states its row's and its four columns' (i0, i1, l1) in registers (nine multiplications: cheaper than a trip through LDS and a barrier), loads the
// 2 x 2 taps of each output (neighbouring lanes read neighbouring or equal addresses: the lines are shared in the vector cache) and
// hands them to the clip writer of frame_io.h, which describes the output path.
#include "frame_io.h"
#include <string.h>

TAD_NAMESPACE_BEGIN

struct SsAxis {
  int i0, i1;
  float l0, l1;
};

// the taps of index d of the resized grid over n_in source samples.  Whatever `scale` holds (NaN and infinities included), i0 and i1
// lie in [0, n_in): the comparison is false for a NaN and n_in - 1 is taken.
__device__ __forceinline__ SsAxis ss_axis(float scale, int d, int n_in) {
  const float src = fmaxf(__fsub_rn(__fmul_rn(scale, __fadd_rn((float)d, 0.5f)), 0.5f), 0.0f);
  SsAxis a;
  a.i0 = src < (float)(n_in - 1) ? (int)src : n_in - 1;
  a.i1 = a.i0 + 1 < n_in ? a.i0 + 1 : n_in - 1;
  a.l1 = __fsub_rn(src, (float)a.i0);
  a.l0 = __fsub_rn(1.0f, a.l1);
  return a;
}

__device__ __forceinline__ float ss_blend(const SsAxis& y, const SsAxis& x, float a, float b, float c, float d) {
  const float top = __fadd_rn(__fmul_rn(x.l0, a), __fmul_rn(x.l1, b));
  const float bot = __fadd_rn(__fmul_rn(x.l0, c), __fmul_rn(x.l1, d));
  return __fadd_rn(__fmul_rn(y.l0, top), __fmul_rn(y.l1, bot));
}

template <bool U8>
__global__ __launch_bounds__(FRAME_THREADS) void spatial_sample_kernel(const void* __restrict__ xv, float* __restrict__ out,
                                                                   const int32_t* __restrict__ tab, ClipNorm nm, int B, int T, int H, int W, int S,
                                                                   int tiles_x) {
  __shared__ float lut[U8 ? 3 * 256 : 1];
  const int tid = threadIdx.x;
  if (U8) {
    // frames_to_clip's value of every byte, per channel: 768 entries, three per thread
    for (int e = tid; e < 3 * 256; e += FRAME_THREADS) {
      const int ch = e >> 8;
      lut[e] = normalize_u8((float)(e & 255), nm.mean[ch], nm.sd[ch]);
    }
    __syncthreads();
  }
  const int32_t* r = tab + (int64_t)blockIdx.y * TAD_SS_ROW_WORDS;
  const int sample = r[0];
  if (sample < 0 || sample >= B * T) return;  // (the same for every thread of the workgroup, and after the only barrier)
  const int clip = sample / T, t = sample - clip * T;
  // the window cut to the source: whatever the row says, every address below lies inside frame (clip, t) of x
  const int wi = frame_clamp(r[1], 0, H - 1), wj = frame_clamp(r[2], 0, W - 1);
  const int wh = frame_clamp(r[3], 1, H - wi), ww = frame_clamp(r[4], 1, W - wj);
  const int oy = r[7], ox = r[8];
  const bool flip = r[9] != 0;
  const float sy = __int_as_float(r[10]), sx = __int_as_float(r[11]);

  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int orow = ty * FRAME_TR + tid / FRAME_CG, col = tx * FRAME_TC + (tid % FRAME_CG) * 4;
  const int valid = S - col < 4 ? S - col : 4;
  if (orow >= S || valid <= 0) return;

  // (a wild offset wraps in the int sum below instead of overflowing: the sum is made unsigned)
  const SsAxis ay = ss_axis(sy, (int)((unsigned)oy + (unsigned)orow), wh);
  SsAxis ax[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = col + q < S ? col + q : S - 1;
    const int d = flip ? S - 1 - c : c;  // a flip reads column S - 1 - x of the unflipped result
    ax[q] = ss_axis(sx, (int)((unsigned)ox + (unsigned)d), ww);
  }

  float v[3][4];
  if (U8) {
    const uint8_t* x = static_cast<const uint8_t*>(xv) + ((((int64_t)clip * T + t) * H + wi) * W + wj) * 3;
    const uint8_t* r0 = x + (int64_t)ay.i0 * W * 3;
    const uint8_t* r1 = x + (int64_t)ay.i1 * W * 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c0 = ax[q].i0 * 3, c1 = ax[q].i1 * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        v[ch][q] = ss_blend(ay, ax[q], lut[ch * 256 + r0[c0 + ch]], lut[ch * 256 + r0[c1 + ch]], lut[ch * 256 + r1[c0 + ch]],
                            lut[ch * 256 + r1[c1 + ch]]);
    }
  } else {
    const int64_t plane = (int64_t)T * H * W;
    const float* x = static_cast<const float*>(xv) + (((int64_t)clip * 3 * T + t) * H + wi) * W + wj;  // channel ch: + ch * plane
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* r0 = x + ch * plane + (int64_t)ay.i0 * W;
      const float* r1 = x + ch * plane + (int64_t)ay.i1 * W;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[ch][q] = ss_blend(ay, ax[q], r0[ax[q].i0], r0[ax[q].i1], r1[ax[q].i0], r1[ax[q].i1]);
    }
  }

  const int64_t oplane = (int64_t)T * S * S;
  store_clip_f32x4(out + (((int64_t)clip * 3 * T + t) * S + orow) * S + col, oplane, v, valid);
}

TAD_NAMESPACE_END

using namespace tad;

static int ss_shape_ok(int B, int T, int H, int W, int S, const char* who) {
  TAD_REQUIRE(B > 0 && T > 0 && (int64_t)B * T <= 65535, "%s: B=%d T=%d: B * T must be in [1, 65535]", who, B, T);
  if (int rc = frame_extent_ok(who, H, W)) return rc;
  TAD_REQUIRE(S > 0 && S <= 16384, "%s: S=%d must be in [1, 16384]", who, S);
  return TAD_OK;
}

extern "C" size_t tad_spatial_sample_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return (size_t)B * T * TAD_SS_ROW_WORDS * 4;
}

extern "C" int tad_spatial_sample_plan_check(const int32_t* table_host, int64_t n_words, int B, int T, int H, int W, int S) {
  TAD_REQUIRE(table_host, "spatial_sample_plan_check: null pointer");
  if (int rc = ss_shape_ok(B, T, H, W, S, "spatial_sample_plan_check")) return rc;
  const int n = B * T;
  TAD_REQUIRE(n_words == (int64_t)n * TAD_SS_ROW_WORDS, "spatial_sample_plan_check: %lld words, expected B * T * %d = %lld",
              (long long)n_words, TAD_SS_ROW_WORDS, (long long)n * TAD_SS_ROW_WORDS);
  SeenSamples seen;  // (B * T <= 65535)
  for (int k = 0; k < n; ++k) {
    const int32_t* r = table_host + (int64_t)k * TAD_SS_ROW_WORDS;
    const int sample = r[0], i = r[1], j = r[2], h = r[3], w = r[4], rh = r[5], rw = r[6], oy = r[7], ox = r[8], flip = r[9];
    TAD_REQUIRE(0 <= sample && sample < n, "spatial_sample_plan_check: row %d: sample=%d outside the B * T = %d frames", k, sample, n);
    TAD_REQUIRE(!seen.twice(sample), "spatial_sample_plan_check: row %d: sample=%d has two rows", k, sample);
    TAD_REQUIRE(i >= 0 && j >= 0 && h >= 1 && w >= 1 && (int64_t)i + h <= H && (int64_t)j + w <= W,
                "spatial_sample_plan_check: row %d: window i=%d j=%d h=%d w=%d is not inside the %d x %d source", k, i, j, h, w, H, W);
    TAD_REQUIRE(rh >= 1 && rw >= 1 && oy >= 0 && ox >= 0 && (int64_t)oy + S <= rh && (int64_t)ox + S <= rw,
                "spatial_sample_plan_check: row %d: output window oy=%d ox=%d of %d x %d is not inside the %d x %d resized grid", k, oy, ox, S,
                S, rh, rw);
    TAD_REQUIRE(flip == 0 || flip == 1, "spatial_sample_plan_check: row %d: flip=%d must be 0 or 1", k, flip);
    float sy, sx;
    memcpy(&sy, r + 10, 4);
    memcpy(&sx, r + 11, 4);
    TAD_REQUIRE(std::isfinite(sy) && std::isfinite(sx) && sy > 0.0f && sx > 0.0f,
                "spatial_sample_plan_check: row %d: the scales %g, %g must be positive and finite", k, (double)sy, (double)sx);
  }
  return TAD_OK;
}

extern "C" int tad_spatial_sample(const void* x, int x_u8, float* out, const float* mean, const float* std_, const void* workspace,
                                  size_t workspace_bytes, int B, int T, int H, int W, int S, tad_stream_t stream) {
  TAD_REQUIRE(x && out && workspace, "spatial_sample: null pointer");
  if (int rc = ss_shape_ok(B, T, H, W, S, "spatial_sample")) return rc;
  if (int rc = table_workspace_ok("spatial_sample", workspace, workspace_bytes, tad_spatial_sample_workspace_bytes(B, T))) return rc;
  TAD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "spatial_sample: out must be 4-byte aligned");
  ClipNorm nm = CLIP_NORM_IDENTITY;
  if (x_u8) {
    TAD_REQUIRE(mean && std_, "spatial_sample: uint8 frames need mean and std");
    if (int rc = clip_norm_from("spatial_sample", mean, std_, &nm)) return rc;
  } else {
    TAD_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0, "spatial_sample: f32 clips must be 4-byte aligned");
  }
  int tiles_x;
  const dim3 grid(frame_tile_grid(S, S, &tiles_x), (unsigned)(B * T));
  const int32_t* tab = static_cast<const int32_t*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  if (x_u8)
    hipLaunchKernelGGL(spatial_sample_kernel<true>, grid, dim3(FRAME_THREADS), 0, s, x, out, tab, nm, B, T, H, W, S, tiles_x);
  else
    hipLaunchKernelGGL(spatial_sample_kernel<false>, grid, dim3(FRAME_THREADS), 0, s, x, out, tab, nm, B, T, H, W, S, tiles_x);
  return check_launch("spatial_sample");
}
