// The MAE pre-training crop on the device (transforms.py of the reference: GroupMultiScaleCrop, a multi-scale crop followed by PIL's
// antialiased BILINEAR resize of every frame; then Stack, ToTorchFormatTensor and GroupNormalize).  The host draws the crops and
// states the coefficient sets (simple_tad_amd/transforms.py); this file carries them out on uint8 frames [B, T, Hs, Ws, 3] in ONE
// launch, into uint8 frames [B, T, S_h, S_w, 3] or straight into the normalised f32 clip [B, 3, T, S_h, S_w].
//
// Table (int32, include/tad_mi355x.h documents the words): B rows {sample, x0, y0, w, h, hset, vset, 0}, then n_hsets horizontal and
// n_vsets vertical coefficient sets, each {in, out, ksize, 0}, bounds[out][2] = (xmin, count), kk[out][ksize], in a slot sized for
// ksize = TAD_MSC_MAX_KSIZE.  The table is only read.
//
// Arithmetic: Pillow's 8-bit resample (ImagingResampleHorizontal_8bpc, then ImagingResampleVertical_8bpc over its bytes), in int32:
//   ss = 1 << 21;  ss += pixel * k over the `count` taps from xmin;  byte = clip(ss >> 22, 0, 255)
// All double arithmetic (the triangle weights, their normalisation and the rounding to 22 bits) stays on the host.  The fused f32
// value is frames_to_clip's: normalize_u8 (common.h) of the byte, IEEE division and subtraction; the file is compiled without
// floating-point contraction (build.py) as randaug.hip is.
//
// Shape: a workgroup owns FRAME_TR x FRAME_TC outputs of one frame (frame_io.h).  It resamples, horizontally, the input rows its
// vertical taps span into LDS (one byte plane per channel, four columns to a word), then runs the vertical pass out of LDS; the row
// halo is recomputed per tile.  Source bytes are loaded one by one (Ws * 3 and the crop offset break every alignment); the outputs of
// a thread are four neighbouring columns, written by the clip and frame writers of frame_io.h, which describes the output path.
#include "frame_io.h"

TAD_NAMESPACE_BEGIN

constexpr int MC_K = TAD_MSC_MAX_KSIZE;
// input rows under the vertical taps of a tile: the centres of FRAME_TR rows lie (FRAME_TR - 1) * scale apart, the taps reach `support`
// to either side, scale = support <= 8: (FRAME_TR - 1) * 8 + 2 * 8 + 1 = 265.  An LDS row holds FRAME_CG words: four columns each
constexpr int MC_ROWS = 272;
static_assert((FRAME_TR - 1) * 8 + MC_K <= MC_ROWS, "tile shape");

__host__ __device__ __forceinline__ int64_t mc_slot_words(int out) { return TAD_MSC_SET_HEAD + (int64_t)out * (2 + MC_K); }
__host__ __device__ __forceinline__ int64_t mc_table_words(int B, int nh, int nv, int Sh, int Sw) {
  return (int64_t)B * TAD_MSC_ROW_WORDS + nh * mc_slot_words(Sw) + nv * mc_slot_words(Sh);
}

// the coefficients of `n` outputs from output `o0` of a set, staged in LDS with the bounds cut to the crop extent `extent` (a
// malformed table is never an address: xmin in [0, extent), count in [0, min(ksize, extent - xmin)])
__device__ __forceinline__ void mc_stage(const int32_t* __restrict__ set, int out_size, int extent, int o0, int n, int (*kk)[MC_K],
                                         int (*bounds)[2], int slots) {
  const int ksize = frame_clamp(set[2], 1, MC_K);
  const int32_t* b = set + TAD_MSC_SET_HEAD;
  const int32_t* k = b + 2 * (int64_t)out_size;
  for (int i = threadIdx.x; i < slots * MC_K; i += FRAME_THREADS) {
    const int o = i / MC_K, j = i - o * MC_K;
    kk[o][j] = (o < n && j < ksize) ? k[(int64_t)(o0 + o) * ksize + j] : 0;
  }
  for (int o = threadIdx.x; o < slots; o += FRAME_THREADS) {
    int xmin = 0, count = 0;
    if (o < n) {
      xmin = frame_clamp(b[2 * (o0 + o)], 0, extent - 1);
      const int most = ksize < extent - xmin ? ksize : extent - xmin;
      count = frame_clamp(b[2 * (o0 + o) + 1], 0, most);
    }
    bounds[o][0] = xmin, bounds[o][1] = count;
  }
}

template <bool F32>
__global__ __launch_bounds__(FRAME_THREADS) void multiscale_crop_kernel(const uint8_t* __restrict__ x, void* __restrict__ out,
                                                                    const int32_t* __restrict__ tab, ClipNorm nm, int B, int T, int Hs, int Ws,
                                                                    int Sh, int Sw, int nh, int nv, int tiles_x) {
  __shared__ uint32_t rows[3][MC_ROWS][FRAME_CG];
  __shared__ int hk[FRAME_TC][MC_K], vk[FRAME_TR][MC_K], hb[FRAME_TC][2], vb[FRAME_TR][2];
  const int32_t* r = tab + (int64_t)blockIdx.z * TAD_MSC_ROW_WORDS;
  const int sample = r[0];
  if (sample < 0 || sample >= B) return;  // (the same for every thread of the workgroup)
  const int t = blockIdx.y, tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  // the crop cut to the source, the set indices to the sets
  const int x0 = frame_clamp(r[1], 0, Ws - 1), y0 = frame_clamp(r[2], 0, Hs - 1);
  const int w = frame_clamp(r[3], 1, Ws - x0), h = frame_clamp(r[4], 1, Hs - y0);
  const int32_t* sets = tab + (int64_t)B * TAD_MSC_ROW_WORDS;
  const int32_t* hset = sets + frame_clamp(r[5], 0, nh - 1) * mc_slot_words(Sw);
  const int32_t* vset = sets + nh * mc_slot_words(Sw) + frame_clamp(r[6], 0, nv - 1) * mc_slot_words(Sh);
  const int c0 = tx * FRAME_TC, o0 = ty * FRAME_TR;
  const int nc = Sw - c0 < FRAME_TC ? Sw - c0 : FRAME_TC, nr = Sh - o0 < FRAME_TR ? Sh - o0 : FRAME_TR;
  mc_stage(hset, Sw, w, c0, nc, hk, hb, FRAME_TC);
  mc_stage(vset, Sh, h, o0, nr, vk, vb, FRAME_TR);
  __syncthreads();

  // the input rows under the tile's vertical taps: [lo, lo + n_in) of the crop
  int lo = h, hi = 0;
  for (int i = 0; i < nr; ++i) {
    const int a = vb[i][0], b = a + vb[i][1];
    if (vb[i][1] > 0) lo = a < lo ? a : lo, hi = b > hi ? b : hi;
  }
  int n_in = hi - lo;
  n_in = n_in < 0 ? 0 : (n_in > MC_ROWS ? MC_ROWS : n_in);

  // horizontal pass: an item is four columns of one channel of one input row, one word of LDS
  const uint8_t* src = x + (((int64_t)sample * T + t) * Hs + (y0 + lo)) * Ws * 3 + (int64_t)x0 * 3;
  // (only the column groups the tile has: a ragged last tile does not pay for the columns past the frame)
  const int ncg = (nc + 3) / 4;
  for (int it = tid; it < n_in * 3 * ncg; it += FRAME_THREADS) {
    const int cg = it % ncg, rc = it / ncg, ch = rc % 3, rr = rc / 3;
    const uint8_t* p = src + (int64_t)rr * Ws * 3 + ch;
    uint32_t pk = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = cg * 4 + q, xmin = hb[c][0], count = hb[c][1];
      int ss = 1 << 21;
      for (int j = 0; j < count; ++j) ss += (int)p[(xmin + j) * 3] * hk[c][j];
      pk |= frame_clip8(ss) << (8 * q);
    }
    rows[ch][rr][cg] = pk;
  }
  __syncthreads();

  // vertical pass: a thread owns four columns of one output row, all three channels
  const int orow = tid / FRAME_CG, cg = tid - orow * FRAME_CG;
  const int col = c0 + cg * 4, valid = Sw - col < 4 ? Sw - col : 4;
  if (orow >= nr || valid <= 0) return;
  int acc[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[ch][q] = 1 << 21;
  const int first = vb[orow][0] - lo, count = vb[orow][1];
  for (int j = 0; j < count; ++j) {
    const int rr = first + j;
    if (rr < 0 || rr >= n_in) break;
    const int k = vk[orow][j];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint32_t u = rows[ch][rr][cg];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[ch][q] += (int)((u >> (8 * q)) & 255u) * k;
    }
  }
  const int oy = o0 + orow;
  if (F32) {
    float* o = static_cast<float*>(out) + (((int64_t)sample * 3 * T + t) * Sh + oy) * Sw + col;  // channel ch: + ch * T * Sh * Sw
    const int64_t plane = (int64_t)T * Sh * Sw;
    float v[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int q = 0; q < 4; ++q) v[ch][q] = frame_norm8(acc[ch][q], nm.mean[ch], nm.sd[ch]);
    store_clip_f32x4(o, plane, v, valid);
  } else {
    store_frames_u8x4(static_cast<uint8_t*>(out) + ((((int64_t)sample * T + t) * Sh + oy) * Sw + col) * 3, acc, valid);
  }
}

TAD_NAMESPACE_END

using namespace tad;

static int mc_shape_ok(int B, int nh, int nv, int Hs, int Ws, int Sh, int Sw, const char* who) {
  TAD_REQUIRE(B > 0 && B <= 65535, "%s: B=%d must be in [1, 65535]", who, B);
  TAD_REQUIRE(nh > 0 && nh <= TAD_MSC_MAX_SETS && nv > 0 && nv <= TAD_MSC_MAX_SETS, "%s: n_hsets=%d n_vsets=%d must be in [1, %d]", who, nh,
              nv, TAD_MSC_MAX_SETS);
  TAD_REQUIRE(Hs > 0 && Ws > 0 && (int64_t)Hs * Ws <= ((int64_t)1 << 28), "%s: Hs=%d Ws=%d: a frame must have 1 .. 2^28 pixels", who, Hs, Ws);
  TAD_REQUIRE(Sh > 0 && Sw > 0 && Sh <= 16384 && Sw <= 16384, "%s: S_h=%d S_w=%d must be in [1, 16384]", who, Sh, Sw);
  return TAD_OK;
}

extern "C" size_t tad_multiscale_crop_workspace_bytes(int B, int n_hsets, int n_vsets, int S_h, int S_w) {
  if (B <= 0 || n_hsets <= 0 || n_vsets <= 0 || S_h <= 0 || S_w <= 0) return 0;
  return (size_t)mc_table_words(B, n_hsets, n_vsets, S_h, S_w) * 4;
}

static int mc_check_set(const int32_t* set, int out_size, int limit, const char* axis, int index) {
  const int in = set[0], ksize = set[2];
  TAD_REQUIRE(in >= 1 && in <= limit, "multiscale_crop_plan_check: %s set %d: input extent %d outside the source (%d)", axis, index, in,
              limit);
  TAD_REQUIRE(set[1] == out_size, "multiscale_crop_plan_check: %s set %d: output extent %d, expected %d", axis, index, set[1], out_size);
  TAD_REQUIRE((int64_t)in <= (int64_t)8 * out_size, "multiscale_crop_plan_check: %s set %d: %d -> %d samples is a filter scale above 8",
              axis, index, in, out_size);
  TAD_REQUIRE(ksize >= 1 && ksize <= TAD_MSC_MAX_KSIZE, "multiscale_crop_plan_check: %s set %d: ksize=%d must be in [1, %d]", axis, index,
              ksize, TAD_MSC_MAX_KSIZE);
  const int32_t* b = set + TAD_MSC_SET_HEAD;
  for (int o = 0; o < out_size; ++o) {
    const int xmin = b[2 * o], count = b[2 * o + 1];
    TAD_REQUIRE(count >= 0 && count <= ksize, "multiscale_crop_plan_check: %s set %d: output %d has %d taps, ksize is %d", axis, index, o,
                count, ksize);
    TAD_REQUIRE(xmin >= 0 && (int64_t)xmin + count <= in, "multiscale_crop_plan_check: %s set %d: output %d reads [%d, %d + %d) of %d samples",
                axis, index, o, xmin, xmin, count, in);
  }
  return TAD_OK;
}

extern "C" int tad_multiscale_crop_plan_check(const int32_t* table_host, int64_t n_words, int B, int n_hsets, int n_vsets, int Hs, int Ws,
                                              int S_h, int S_w) {
  TAD_REQUIRE(table_host, "multiscale_crop_plan_check: null pointer");
  if (int rc = mc_shape_ok(B, n_hsets, n_vsets, Hs, Ws, S_h, S_w, "multiscale_crop_plan_check")) return rc;
  const int64_t want = mc_table_words(B, n_hsets, n_vsets, S_h, S_w);
  TAD_REQUIRE(n_words == want, "multiscale_crop_plan_check: %lld words, expected B * %d + the sets = %lld", (long long)n_words,
              TAD_MSC_ROW_WORDS, (long long)want);
  const int32_t* sets = table_host + (int64_t)B * TAD_MSC_ROW_WORDS;
  for (int i = 0; i < n_hsets; ++i)
    if (int rc = mc_check_set(sets + i * mc_slot_words(S_w), S_w, Ws, "horizontal", i)) return rc;
  const int32_t* vsets = sets + n_hsets * mc_slot_words(S_w);
  for (int i = 0; i < n_vsets; ++i)
    if (int rc = mc_check_set(vsets + i * mc_slot_words(S_h), S_h, Hs, "vertical", i)) return rc;
  SeenSamples seen;  // (B <= 65535)
  for (int k = 0; k < B; ++k) {
    const int32_t* r = table_host + (int64_t)k * TAD_MSC_ROW_WORDS;
    const int sample = r[0], x0 = r[1], y0 = r[2], w = r[3], h = r[4], hs = r[5], vs = r[6];
    TAD_REQUIRE(0 <= sample && sample < B, "multiscale_crop_plan_check: row %d: sample=%d outside the batch B=%d", k, sample, B);
    TAD_REQUIRE(!seen.twice(sample), "multiscale_crop_plan_check: row %d: sample=%d has two rows", k, sample);
    TAD_REQUIRE(x0 >= 0 && y0 >= 0 && w >= 1 && h >= 1 && (int64_t)x0 + w <= Ws && (int64_t)y0 + h <= Hs,
                "multiscale_crop_plan_check: row %d: crop x0=%d y0=%d w=%d h=%d is not inside the %d x %d source", k, x0, y0, w, h, Ws, Hs);
    TAD_REQUIRE(0 <= hs && hs < n_hsets && 0 <= vs && vs < n_vsets, "multiscale_crop_plan_check: row %d: set indices %d, %d outside [0, %d) / [0, %d)",
                k, hs, vs, n_hsets, n_vsets);
    TAD_REQUIRE(sets[hs * mc_slot_words(S_w)] == w && vsets[vs * mc_slot_words(S_h)] == h,
                "multiscale_crop_plan_check: row %d: the sets are stated for %d x %d samples, the crop has %d x %d", k,
                sets[hs * mc_slot_words(S_w)], vsets[vs * mc_slot_words(S_h)], w, h);
  }
  return TAD_OK;
}

extern "C" int tad_multiscale_crop(const uint8_t* x, void* out, int out_f32, const float* mean, const float* std_, const void* workspace,
                                   size_t workspace_bytes, int B, int T, int Hs, int Ws, int S_h, int S_w, int n_hsets, int n_vsets,
                                   tad_stream_t stream) {
  TAD_REQUIRE(x && out && workspace, "multiscale_crop: null pointer");
  if (int rc = mc_shape_ok(B, n_hsets, n_vsets, Hs, Ws, S_h, S_w, "multiscale_crop")) return rc;
  TAD_REQUIRE(T > 0 && T <= 65535, "multiscale_crop: T=%d must be in [1, 65535]", T);
  if (int rc = table_workspace_ok("multiscale_crop", workspace, workspace_bytes, tad_multiscale_crop_workspace_bytes(B, n_hsets, n_vsets, S_h, S_w)))
    return rc;
  ClipNorm nm = CLIP_NORM_IDENTITY;
  if (out_f32) {
    TAD_REQUIRE(mean && std_, "multiscale_crop: the f32 output needs mean and std");
    TAD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "multiscale_crop: an f32 out must be 4-byte aligned");
    if (int rc = clip_norm_from("multiscale_crop", mean, std_, &nm)) return rc;
  }
  int tiles_x;
  const dim3 grid(frame_tile_grid(S_h, S_w, &tiles_x), (unsigned)T, (unsigned)B);
  const int32_t* tab = static_cast<const int32_t*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  if (out_f32)
    hipLaunchKernelGGL(multiscale_crop_kernel<true>, grid, dim3(FRAME_THREADS), 0, s, x, out, tab, nm, B, T, Hs, Ws, S_h, S_w, n_hsets, n_vsets,
                       tiles_x);
  else
    hipLaunchKernelGGL(multiscale_crop_kernel<false>, grid, dim3(FRAME_THREADS), 0, s, x, out, tab, nm, B, T, Hs, Ws, S_h, S_w, n_hsets, n_vsets,
                       tiles_x);
  return check_launch("multiscale_crop");
}
