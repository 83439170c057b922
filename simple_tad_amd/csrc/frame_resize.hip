// The loader resize of the fine-tune and inference paths on the device: cv2.resize(frame, (S_w, S_h), INTER_CUBIC) of every decoded
// frame (run_inference.py:76,91; dota.py:347-348; dada.py:309-310), and video_transforms.pad_wide_clips (:1301-1337), which pads a wide
// frame at top and bottom before that resize.  The host states the per-axis taps and coefficients (simple_tad_amd/frame_resize.py);
// this file carries them out on uint8 frames [B, T, H, W, 3] in ONE launch, into uint8 frames [B, T, S_h, S_w, 3] (any alignment: a
// slot of a ring, a slice of a frame store) or straight into the normalised f32 clip [B, 3, T, S_h, S_w].
//
// Table (int32, include/tad_mi355x.h documents the words): B rows {sample, mode, pad_top, pad_bottom, alpha bits, packed colour, vset,
// 0}, one horizontal set and n_vsets vertical sets, each {in, out, 0, 0}, first[out], k[out][4].  The table is only read.
//
// Arithmetic -- the contract: OpenCV's GENERIC INTEGER formulation of the 8-bit cubic resize, not the bytes of one OpenCV build (the
// vector path of a build finishes the vertical pass in float and can differ from this by one grey level): the two int32 passes of
// cubic_resize.h, which also describes the tile, its LDS and the vertical pass.  All float work (the sample positions, Keys' weights
// with A = -0.75, their rounding) stays on the host.
//
// Padding is a VIRTUAL source of pad_top + H + pad_bottom rows that the vertical taps index; no padded frame exists.  The horizontal
// pass -- this file's own -- maps each virtual row it needs to a frame row (reflect, replicate), or to the band's colour.  A reflected
// band byte is faded towards black: rint((float)p * alpha), the product on its own -- cv2.addWeighted(reflect, a, black, 1 - a, 0) in
// float; the file is compiled without floating-point contraction (build.py).  The four pixels under an output's horizontal taps are 12
// contiguous bytes at no particular alignment (W * 3 breaks every one): cubic_load12; where a tap clamps at a border, byte by byte.  The
// fused f32 value is frames_to_clip's: frame_norm8 in front of store_clip_f32x4 (frame_io.h).
#include "cubic_resize.h"
#include <string.h>
#include <type_traits>

TAD_NAMESPACE_BEGIN

__host__ __device__ __forceinline__ int64_t fr_table_words(int B, int nv, int Sh, int Sw) {
  return (int64_t)B * TAD_FR_ROW_WORDS + cubic_set_words(Sw) + nv * cubic_set_words(Sh);
}

// a reflected band byte faded towards black: rint((float)p * alpha), the product on its own, cut to a byte
__device__ __forceinline__ int fr_fade(int b, float alpha) { return frame_clamp(__float2int_rn(__fmul_rn((float)b, alpha)), 0, 255); }

template <bool F32>
__global__ __launch_bounds__(FRAME_THREADS) void frame_resize_kernel(const uint8_t* __restrict__ x, void* __restrict__ out,
                                                                 const int32_t* __restrict__ tab, ClipNorm nm, int B, int T, int H, int W, int Sh,
                                                                 int Sw, int nv, int tiles_x) {
  CUBIC_TILE_LDS;
  const int32_t* r = tab + (int64_t)blockIdx.z * TAD_FR_ROW_WORDS;
  const int sample = r[0];
  if (sample < 0 || sample >= B) return;  // (the same for every thread of the workgroup)
  const int t = blockIdx.y, tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  // mode and pads cut to what the frame allows, the set index to the sets: a malformed table is never an address
  const int mode = frame_clamp(r[1], TAD_FR_NONE, TAD_FR_REPLICATE);
  const int pt = mode == TAD_FR_NONE ? 0 : frame_clamp(r[2], 0, H), pb = mode == TAD_FR_NONE ? 0 : frame_clamp(r[3], 0, H);
  const float alpha = __int_as_float(r[4]);
  const uint32_t colour = (uint32_t)r[5];
  const int Hv = pt + H + pb;
  const int32_t* hset = tab + (int64_t)B * TAD_FR_ROW_WORDS;
  const int32_t* vset = hset + cubic_set_words(Sw) + frame_clamp(r[6], 0, nv - 1) * cubic_set_words(Sh);
  const int c0 = tx * FRAME_TC, o0 = ty * FRAME_TR;
  const int nc = Sw - c0 < FRAME_TC ? Sw - c0 : FRAME_TC, nr = Sh - o0 < FRAME_TR ? Sh - o0 : FRAME_TR;
  cubic_stage(hset, Sw, c0, nc, W, hf, hk, FRAME_TC);
  cubic_stage(vset, Sh, o0, nr, Hv, vf, vk, FRAME_TR);
  __syncthreads();
  const CubicSpan span = cubic_span(vf, nr, Hv);  // (of virtual rows)

  // horizontal pass: an item is one column of one virtual row, all three channels; a thread keeps its column and walks the rows.  The
  // fade of a reflected band is compiled into the pass of the clips that reflect alone (the mode is the workgroup's)
  const uint8_t* frame = x + ((int64_t)sample * T + t) * H * W * 3;
  auto hpass = [&](auto reflect) {
    constexpr bool REFLECT = decltype(reflect)::value;
    const int c = tid & (FRAME_TC - 1);
    if (c >= nc) return;
    for (int slot = tid / FRAME_TC; slot < span.nslots; slot += FRAME_THREADS / FRAME_TC) {
      const int v = cubic_slot_row(span, vf, slot, Hv);
      // the row map: inside the frame the row itself; in a band its mirror image (faded), the edge row, or the colour
      int fr = v - pt;
      bool band = false;
      if (v < pt) {
        band = true;
        fr = REFLECT ? pt - 1 - v : 0;
      } else if (v >= pt + H) {
        band = true;
        fr = REFLECT ? H - 1 - (v - pt - H) : H - 1;
      }
      fr = frame_clamp(fr, 0, H - 1);
      const bool constant = band && mode == TAD_FR_CONST, fade = REFLECT && band;
      const uint8_t* row = frame + (int64_t)fr * W * 3;
      int acc[3] = {0, 0, 0};
      const int f0 = hf[c];
      if (!constant && f0 >= 0 && f0 + 3 <= W - 1) {  // no tap clamps: the four pixels are 12 contiguous bytes
        uint32_t w[3];
        cubic_load12(row + (int64_t)f0 * 3, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = hk[c][j];
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            int b = (int)((w[(3 * j + ch) >> 2] >> (((3 * j + ch) & 3) * 8)) & 255u);
            if (fade) b = fr_fade(b, alpha);
            acc[ch] += b * k;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = hk[c][j];
          const uint8_t* p = row + (int64_t)frame_clamp(f0 + j, 0, W - 1) * 3;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            int b = constant ? (int)((colour >> (8 * ch)) & 255u) : (int)p[ch];
            if (fade) b = fr_fade(b, alpha);
            acc[ch] += b * k;
          }
        }
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) hp[slot][ch][c] = acc[ch];
    }
  };
  if (mode == TAD_FR_REFLECT)
    hpass(std::true_type{});
  else
    hpass(std::false_type{});
  __syncthreads();

  CubicOut at;
  int acc[3][4];
  if (!cubic_vpass(hp, vf, vk, span, Hv, c0, nr, Sw, false, at, acc)) return;
  const int oy = o0 + at.orow, col = at.col, valid = at.valid;
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

static int fr_shape_ok(int B, int nv, int H, int W, int Sh, int Sw, const char* who) {
  TAD_REQUIRE(B > 0 && B <= 65535, "%s: B=%d must be in [1, 65535]", who, B);
  TAD_REQUIRE(nv > 0 && nv <= TAD_FR_MAX_SETS, "%s: n_vsets=%d must be in [1, %d]", who, nv, TAD_FR_MAX_SETS);
  if (int rc = frame_extent_ok(who, H, W)) return rc;
  TAD_REQUIRE(Sh > 0 && Sw > 0 && Sh <= 16384 && Sw <= 16384, "%s: S_h=%d S_w=%d must be in [1, 16384]", who, Sh, Sw);
  return TAD_OK;
}

extern "C" size_t tad_frame_resize_workspace_bytes(int B, int n_vsets, int S_h, int S_w) {
  if (B <= 0 || n_vsets <= 0 || S_h <= 0 || S_w <= 0) return 0;
  return (size_t)fr_table_words(B, n_vsets, S_h, S_w) * 4;
}

extern "C" int tad_frame_resize_plan_check(const int32_t* table_host, int64_t n_words, int B, int n_vsets, int H, int W, int S_h, int S_w) {
  TAD_REQUIRE(table_host, "frame_resize_plan_check: null pointer");
  if (int rc = fr_shape_ok(B, n_vsets, H, W, S_h, S_w, "frame_resize_plan_check")) return rc;
  const int64_t want = fr_table_words(B, n_vsets, S_h, S_w);
  TAD_REQUIRE(n_words == want, "frame_resize_plan_check: %lld words, expected B * %d + the sets = %lld", (long long)n_words, TAD_FR_ROW_WORDS,
              (long long)want);
  const int32_t* hset = table_host + (int64_t)B * TAD_FR_ROW_WORDS;
  TAD_REQUIRE(hset[0] == W, "frame_resize_plan_check: horizontal set: input extent %d, the source has %d columns", hset[0], W);
  // (a set's input extent is checked here, against the frame, under this check's own words: W, and H plus two pads of at most H)
  if (int rc = cubic_check_set("frame_resize_plan_check", hset, S_w, "horizontal", 0, W)) return rc;
  const int32_t* vsets = hset + cubic_set_words(S_w);
  for (int i = 0; i < n_vsets; ++i) {
    const int32_t* set = vsets + i * cubic_set_words(S_h);
    TAD_REQUIRE(set[0] >= H && (int64_t)set[0] <= (int64_t)3 * H,
                "frame_resize_plan_check: vertical set %d: virtual height %d is not the %d rows of the source plus two pads of at most %d", i, set[0], H, H);
    if (int rc = cubic_check_set("frame_resize_plan_check", set, S_h, "vertical", i, 3 * H)) return rc;
  }
  SeenSamples seen;  // (B <= 65535)
  for (int k = 0; k < B; ++k) {
    const int32_t* r = table_host + (int64_t)k * TAD_FR_ROW_WORDS;
    const int sample = r[0], mode = r[1], pt = r[2], pb = r[3], vs = r[6];
    TAD_REQUIRE(0 <= sample && sample < B, "frame_resize_plan_check: row %d: sample=%d outside the batch B=%d", k, sample, B);
    TAD_REQUIRE(!seen.twice(sample), "frame_resize_plan_check: row %d: sample=%d has two rows", k, sample);
    TAD_REQUIRE(mode >= TAD_FR_NONE && mode <= TAD_FR_REPLICATE, "frame_resize_plan_check: row %d: unknown mode %d", k, mode);
    TAD_REQUIRE(pt >= 0 && pb >= 0, "frame_resize_plan_check: row %d: negative pad (%d, %d)", k, pt, pb);
    TAD_REQUIRE(pt <= H && pb <= H, "frame_resize_plan_check: row %d: pad (%d, %d) is greater than H=%d (a second reflection is not built)", k, pt, pb, H);
    TAD_REQUIRE(mode != TAD_FR_NONE || (pt == 0 && pb == 0), "frame_resize_plan_check: row %d: mode none with pads (%d, %d)", k, pt, pb);
    if (mode == TAD_FR_REFLECT) {
      float a;
      memcpy(&a, &r[4], 4);
      TAD_REQUIRE(std::isfinite(a) && a >= 0.0f && a <= 1.0f, "frame_resize_plan_check: row %d: alpha=%g must be in [0, 1]", k, (double)a);
    }
    TAD_REQUIRE((r[5] & ~0xffffff) == 0, "frame_resize_plan_check: row %d: colour word 0x%x holds more than three bytes", k, (unsigned)r[5]);
    TAD_REQUIRE(0 <= vs && vs < n_vsets, "frame_resize_plan_check: row %d: vertical set %d outside [0, %d)", k, vs, n_vsets);
    TAD_REQUIRE(vsets[vs * cubic_set_words(S_h)] == pt + H + pb, "frame_resize_plan_check: row %d: its vertical set is stated for %d rows, the padded frame has %d",
                k, vsets[vs * cubic_set_words(S_h)], pt + H + pb);
  }
  return TAD_OK;
}

extern "C" int tad_frame_resize(const uint8_t* x, void* out, int out_f32, const float* mean, const float* std_, const void* workspace,
                                size_t workspace_bytes, int B, int T, int H, int W, int S_h, int S_w, int n_vsets, tad_stream_t stream) {
  TAD_REQUIRE(x && out && workspace, "frame_resize: null pointer");
  if (int rc = fr_shape_ok(B, n_vsets, H, W, S_h, S_w, "frame_resize")) return rc;
  TAD_REQUIRE(T > 0 && T <= 65535, "frame_resize: T=%d must be in [1, 65535]", T);
  if (int rc = table_workspace_ok("frame_resize", workspace, workspace_bytes, tad_frame_resize_workspace_bytes(B, n_vsets, S_h, S_w))) return rc;
  ClipNorm nm = CLIP_NORM_IDENTITY;
  if (out_f32) {
    TAD_REQUIRE(mean && std_, "frame_resize: the f32 output needs mean and std");
    TAD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "frame_resize: an f32 out must be 4-byte aligned");
    if (int rc = clip_norm_from("frame_resize", mean, std_, &nm)) return rc;
  }
  int tiles_x;
  const dim3 grid(frame_tile_grid(S_h, S_w, &tiles_x), (unsigned)T, (unsigned)B);
  const int32_t* tab = static_cast<const int32_t*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  if (out_f32)
    hipLaunchKernelGGL(frame_resize_kernel<true>, grid, dim3(FRAME_THREADS), 0, s, x, out, tab, nm, B, T, H, W, S_h, S_w, n_vsets, tiles_x);
  else
    hipLaunchKernelGGL(frame_resize_kernel<false>, grid, dim3(FRAME_THREADS), 0, s, x, out, tab, nm, B, T, H, W, S_h, S_w, n_vsets, tiles_x);
  return check_launch("frame_resize");
}
