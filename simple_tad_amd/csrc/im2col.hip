// The patch matrix of the tubelet embedding (Conv3d k = s = (tub, p, p) as a GEMM), every way the library builds it:
//   tad_im2col_tubelets (+ _f16)     f32 clip  [B,C,T,H,W]                      -> 16-bit cols
//   tad_im2col_tubelets_f32          f32 clip  [B,C,T,H,W]                      -> f32 cols (precise mode)
//   tad_im2col_tubelets_16           16-bit clip [B,C,T,H,W] (either format)    -> the same 16-bit words in cols (a move: no cast, no twin)
//   tad_im2col_tubelets_u8 (+ _f16)  uint8 clips [B,T,H,W,3], a ring per clip   -> normalised 16-bit cols
//   tad_im2col_frame_windows         uint8 store [F,H,W,3] + slot table [B,T]   -> normalised 16-bit cols
// cols [B*N, ldk]: pixel (b, t, h, w) of channel c lands in row n = ((b T' + t') H' + h') W' + w' (t' = t / tub, ...) at column
// k = ((c tub + kt) p + kh) p + kw (kt = t % tub, ...) -- PatchGrid below is the one statement of that layout.  ldk = K = C tub p p for
// patch sizes that are multiples of 8; other even sizes (ViT-L/14: K = 1176) get rows of stride tad_patch_embed_ldk (K rounded up to the
// GEMM's K-tile, 1216) whose padding columns are zero, so the padded matrix times a zero-padded weight is the un-padded product exactly.
//
// Two work decompositions, the same for every source: "wide" items of 8 consecutive w (4 for f32 -> f32) with 16-byte stores for patch
// sizes that are multiples of 8, else "pairs" of 2 consecutive w (a pair never straddles a patch: p and w are even) where the thread
// that owns k = 0 of a token zeroes the row's padding.  All are streaming kernels: threads walk the source in memory order, 256 per block,
// grid capped with a grid-stride loop beyond.
//
// The uint8 sources are the decoder / cv2 layout; a value is normalize_u8 (common.h) of the byte and then the same round-to-nearest-even
// cast as the f32 route, so cols is bit-identical to tad_im2col_tubelets on the normalised f32 clip (run_inference.py:22-32
// prepare_image; dota.py:443-460 tensor_normalize) while reading 4x fewer bytes and skipping the f32 clip entirely.  ``bgr``: the channel
// in memory is 2 - c (cv2 frames; the reference converts with cv2.cvtColor(BGR2RGB)).  Where frame t of clip b lives is a slot policy:
// RingSlots for the sliding window of run_inference.py:86-93 kept as a ring instead of shifting the frames, TableSlots for the windows
// of a whole video uploaded once (the reference decodes, resizes and uploads all T frames of every test window again, dota.py:274-284
// load_images: at view_step 1 every frame travels T times).
//
// Compiled ONCE: the output format is a template argument (both casts exist in one translation unit), not a second pass over the file.
#include "common.h"

namespace tad {
namespace im2col {

template <int FMT>
using out_t = std::conditional_t<FMT == TAD_F32, float, uint16_t>;

struct Cell {
  int64_t n;       // row of cols
  int kt, kh, kw;  // position inside the patch
};
struct PatchGrid {
  int tub, p, Tp, Hp, Wp;
  __device__ __forceinline__ PatchGrid(int T, int H, int W, int tub_, int p_) : tub(tub_), p(p_), Tp(T / tub_), Hp(H / p_), Wp(W / p_) {}
  __device__ __forceinline__ Cell cell(int b, int t, int h, int w) const {
    const int tp = t / tub, hp = h / p, wp = w / p;
    return {((int64_t)(b * Tp + tp) * Hp + hp) * Wp + wp, t - tp * tub, h - hp * p, w - wp * p};
  }
  __device__ __forceinline__ int k(const Cell& q, int c) const { return ((c * tub + q.kt) * p + q.kh) * p + q.kw; }
};

// next (fastest remaining) coordinate of a flat work-item index
__device__ __forceinline__ int peel(int64_t& r, int extent) {
  const int v = (int)(r % extent);
  r /= extent;
  return v;
}

template <int FMT>
__device__ __forceinline__ void zero_padding(out_t<FMT>* row, int K, int ldk) {
  for (int z = K; z < ldk; z += 2) {
    if constexpr (FMT == TAD_F32) *reinterpret_cast<float2*>(row + z) = make_float2(0.f, 0.f);
    else *reinterpret_cast<uint32_t*>(row + z) = 0u;
  }
}

// ---------------------------------------------------------------- f32 clip
// One item = PER consecutive w of one (b, c, t, h) row: 32 B in, 16 B out for the 16-bit formats; 16 B in and out for f32.
template <int FMT>
__global__ void f32_wide_kernel(const float* __restrict__ x, out_t<FMT>* __restrict__ cols, int B, int C, int T, int H, int W, int tub,
                                int p) {
  constexpr int PER = FMT == TAD_F32 ? 4 : 8;
  const int Wn = W / PER;
  const int64_t total = (int64_t)B * C * T * H * Wn;
  const PatchGrid g(T, H, W, tub, p);
  const int K = C * tub * p * p;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t r = i;
    const int w = peel(r, Wn) * PER, h = peel(r, H), t = peel(r, T), c = peel(r, C), b = (int)r;
    const float4* src = reinterpret_cast<const float4*>(x) + (PER / 4) * i;
    const float4 a0 = src[0], a1 = PER == 8 ? src[1] : a0;
    const Cell q = g.cell(b, t, h, w);
    out_t<FMT>* dst = cols + q.n * K + g.k(q, c);
    if constexpr (FMT == TAD_F32)
      *reinterpret_cast<float4*>(dst) = a0;
    else
      *reinterpret_cast<uint4*>(dst) =
          make_uint4(pack16x2<FMT>(a0.x, a0.y), pack16x2<FMT>(a0.z, a0.w), pack16x2<FMT>(a1.x, a1.y), pack16x2<FMT>(a1.z, a1.w));
  }
}

template <int FMT>
__global__ void f32_pairs_kernel(const float* __restrict__ x, out_t<FMT>* __restrict__ cols, int B, int C, int T, int H, int W, int tub,
                                 int p, int ldk) {
  const int W2 = W >> 1;
  const int64_t total = (int64_t)B * C * T * H * W2;
  const PatchGrid g(T, H, W, tub, p);
  const int K = C * tub * p * p;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t r = i;
    const int w = peel(r, W2) * 2, h = peel(r, H), t = peel(r, T), c = peel(r, C), b = (int)r;
    const float2 a = reinterpret_cast<const float2*>(x)[i];
    const Cell q = g.cell(b, t, h, w);
    const int k = g.k(q, c);
    out_t<FMT>* row = cols + q.n * ldk;
    if constexpr (FMT == TAD_F32) *reinterpret_cast<float2*>(row + k) = a;
    else *reinterpret_cast<uint32_t*>(row + k) = pack16x2<FMT>(a.x, a.y);
    if (k == 0) zero_padding<FMT>(row, K, ldk);
  }
}

// ---------------------------------------------------------------- 16-bit clip
// The clip already is in the operand format (a loader's wire format, prefetch.ClipPrefetcher wire="operand"): the patch matrix is a permutation
// of its 16-bit words, so nothing here knows the format -- NaN payloads and subnormals pass as they are.  One item = 8 consecutive w of one
// (b, c, t, h) row: one 16-byte load, one 16-byte store (item i is bytes [16 i, 16 i + 16) of the clip; the 8 words stay inside one patch row
// because p % 8 == 0, so the store is 16-byte aligned in a row of K = C tub p p words, K % 64 == 0).
__global__ void w16_wide_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ cols, int B, int C, int T, int H, int W, int tub, int p) {
  const int W8 = W >> 3;
  const int64_t total = (int64_t)B * C * T * H * W8;
  const PatchGrid g(T, H, W, tub, p);
  const int K = C * tub * p * p;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t r = i;
    const int w = peel(r, W8) * 8, h = peel(r, H), t = peel(r, T), c = peel(r, C), b = (int)r;
    const uint4 a = reinterpret_cast<const uint4*>(x)[i];
    const Cell q = g.cell(b, t, h, w);
    *reinterpret_cast<uint4*>(cols + q.n * K + g.k(q, c)) = a;
  }
}

// One item = 2 consecutive w = one 4-byte word in and out.
__global__ void w16_pairs_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ cols, int B, int C, int T, int H, int W, int tub, int p,
                                 int ldk) {
  const int W2 = W >> 1;
  const int64_t total = (int64_t)B * C * T * H * W2;
  const PatchGrid g(T, H, W, tub, p);
  const int K = C * tub * p * p;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t r = i;
    const int w = peel(r, W2) * 2, h = peel(r, H), t = peel(r, T), c = peel(r, C), b = (int)r;
    const uint32_t a = reinterpret_cast<const uint32_t*>(x)[i];
    const Cell q = g.cell(b, t, h, w);
    const int k = g.k(q, c);
    uint16_t* row = cols + q.n * ldk;
    *reinterpret_cast<uint32_t*>(row + k) = a;
    if (k == 0) zero_padding<TAD_BF16>(row, K, ldk);  // (zero words: the same in both 16-bit formats)
  }
}

// ---------------------------------------------------------------- uint8 frames
// Where frame t of clip b lives, as an index into a flat array of [H,W,3] frames.
struct RingSlots {  // clips [B,T,H,W,3]: slot (t + t_offset) % T of clip b, 0 <= t_offset < T
  int t_offset;
  __device__ __forceinline__ int64_t frame(int b, int t, int T) const {
    int slot = t + t_offset;
    slot = slot >= T ? slot - T : slot;
    return (int64_t)b * T + slot;
  }
};
// store [F,H,W,3]: slot idx[b*T + t].  The table lives on the device, so the entry point cannot check it: callers validate 0 <= idx < F on
// the host (frame_store.py does), and as a defence a slot is clamped into [0, F-1] -- a bad table yields a wrong frame, never an address
// outside the store.
struct TableSlots {
  const int32_t* idx;
  int64_t F;
  __device__ __forceinline__ int64_t frame(int b, int t, int T) const {
    const int64_t s = idx[(int64_t)b * T + t];
    return s < 0 ? 0 : (s >= F ? F - 1 : s);
  }
};
// The argument list (six scalar constants, the policy last) and the 64-bit form of the pixel offset in the source address are the
// ones the compiler was seen to allocate registers for as it did for the kernels these templates replace: with the policy in front,
// the constants in a struct or the offset multiplied in 32 bits, the ring-policy wide instance takes 39-40 VGPRs instead of 31 and
// keeps its 48 channel selects' condition in an SGPR pair (and measured 1.1-1.5 % slower on frames a copy had just written).

// One item = 8 consecutive pixels of one row = 24 contiguous bytes in, three 16-byte chunks out (one per channel).
template <int FMT, typename Slots>
__global__ void u8_wide_kernel(const uint8_t* __restrict__ frames, uint16_t* __restrict__ cols, int B, int T, int H, int W, int tub, int p,
                               float m0, float m1, float m2, float s0, float s1, float s2, int bgr, Slots slots) {
  const int W8 = W >> 3;
  const int64_t total = (int64_t)B * T * H * W8;
  const PatchGrid g(T, H, W, tub, p);
  const int K = 3 * tub * p * p;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t r = i;
    const int w8 = peel(r, W8), h = peel(r, H), t = peel(r, T), b = (int)r;
    const uint8_t* src = frames + ((slots.frame(b, t, T) * H + h) * W + (int64_t)w8 * 8) * 3;
    uint32_t raw[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) raw[j] = reinterpret_cast<const uint32_t*>(src)[j];  // (W*3*8) % 4 == 0: 4-byte aligned
    const Cell q = g.cell(b, t, h, w8 * 8);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int cm = bgr ? 2 - c : c;  // channel position in memory
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int byte = e * 3 + cm;
        v[e] = normalize_u8((float)((raw[byte >> 2] >> ((byte & 3) * 8)) & 0xffu), mean[c], sd[c]);
      }
      *reinterpret_cast<uint4*>(cols + q.n * K + g.k(q, c)) =
          make_uint4(pack16x2<FMT>(v[0], v[1]), pack16x2<FMT>(v[2], v[3]), pack16x2<FMT>(v[4], v[5]), pack16x2<FMT>(v[6], v[7]));
    }
  }
}

// One item = 2 pixels = 6 contiguous bytes in (2-byte aligned), three 4-byte pairs out.
template <int FMT, typename Slots>
__global__ void u8_pairs_kernel(const uint8_t* __restrict__ frames, uint16_t* __restrict__ cols, int B, int T, int H, int W, int tub, int p,
                                int ldk, float m0, float m1, float m2, float s0, float s1, float s2, int bgr, Slots slots) {
  const int W2 = W >> 1;
  const int64_t total = (int64_t)B * T * H * W2;
  const PatchGrid g(T, H, W, tub, p);
  const int K = 3 * tub * p * p;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t r = i;
    const int w2 = peel(r, W2), h = peel(r, H), t = peel(r, T), b = (int)r;
    const uint16_t* src = reinterpret_cast<const uint16_t*>(frames + ((slots.frame(b, t, T) * H + h) * W + (int64_t)w2 * 2) * 3);
    const uint32_t lo = (uint32_t)src[0] | ((uint32_t)src[1] << 16), hi = (uint32_t)src[2];  // bytes 0..3, 4..5
    const Cell q = g.cell(b, t, h, w2 * 2);
    uint16_t* row = cols + q.n * ldk;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int cm = bgr ? 2 - c : c;
      const int b0 = cm, b1 = 3 + cm;  // byte positions of the two pixels' channel
      const float u0 = (float)((lo >> (b0 * 8)) & 0xffu);
      const float u1 = (float)(((b1 < 4 ? lo >> (b1 * 8) : hi >> ((b1 - 4) * 8))) & 0xffu);
      *reinterpret_cast<uint32_t*>(row + g.k(q, c)) = pack16x2<FMT>(normalize_u8(u0, mean[c], sd[c]), normalize_u8(u1, mean[c], sd[c]));
    }
    if (q.kt == 0 && q.kh == 0 && q.kw == 0) zero_padding<FMT>(row, K, ldk);  // (k = 0 of channel 0)
  }
}

// ---------------------------------------------------------------- host side
// The one argument check of the family; `who` is the name the entry point's messages carry.  The uint8 entry points (mean3 / std3
// given) also answer for their normalisation constants and for the alignment their 4-byte loads and 16-byte stores need (`src_name`: what
// the entry point calls its source).
static int check_args(const char* who, const void* src, const void* cols, int B, int C, int T, int H, int W, int tubelet, int patch,
                      bool u8 = false, const float* mean3 = nullptr, const float* std3 = nullptr, const char* src_name = "x") {
  TAD_REQUIRE(src && cols && (!u8 || (mean3 && std3)), "%s: null pointer", who);
  TAD_REQUIRE(B > 0 && C > 0 && tubelet > 0 && patch > 0 && T % tubelet == 0 && H % patch == 0 && W % patch == 0,
              "%s: T/H/W must be multiples of tubelet/patch (got B=%d T=%d H=%d W=%d tub=%d p=%d)", who, B, T, H, W, tubelet, patch);
  TAD_REQUIRE(patch % 2 == 0, "%s: patch size must be even (got %d)", who, patch);
  if (u8) {
    TAD_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "%s: zero std", who);
    TAD_REQUIRE_ALIGNED_AS(who, src, 4, src_name);
    TAD_REQUIRE_ALIGNED(who, cols, 16);
  }
  return TAD_OK;
}

template <int FMT>
static int from_f32(const char* who, const float* x, void* cols, int B, int C, int T, int H, int W, int tubelet, int patch,
                    tad_stream_t stream) {
  if (int rc = check_args(who, x, cols, B, C, T, H, W, tubelet, patch)) return rc;
  // wide items: float4 loads, 16-byte stores; pairs: float2 loads, one 4-byte word (16-bit formats) or a float2 (f32) per store
  TAD_REQUIRE_ALIGNED(who, x, patch % 8 ? 8 : 16);
  TAD_REQUIRE_ALIGNED(who, cols, patch % 8 ? (FMT == TAD_F32 ? 8 : 4) : 16);
  const int64_t pixels = (int64_t)B * C * T * H * W;  // (W is a multiple of every item width used: W % patch == 0)
  if (patch % 8)
    hipLaunchKernelGGL(f32_pairs_kernel<FMT>, dim3(capped_grid(pixels / 2, 256)), dim3(256), 0, (hipStream_t)stream, x, (out_t<FMT>*)cols, B,
                       C, T, H, W, tubelet, patch, tad_patch_embed_ldk(C, tubelet, patch));
  else
    hipLaunchKernelGGL(f32_wide_kernel<FMT>, dim3(capped_grid(pixels / (FMT == TAD_F32 ? 4 : 8), 256)), dim3(256), 0, (hipStream_t)stream,
                       x, (out_t<FMT>*)cols, B, C, T, H, W, tubelet, patch);
  return check_launch(who);
}

static int from_16(const char* who, const uint16_t* x, uint16_t* cols, int B, int C, int T, int H, int W, int tubelet, int patch,
                   tad_stream_t stream) {
  if (int rc = check_args(who, x, cols, B, C, T, H, W, tubelet, patch)) return rc;
  TAD_REQUIRE_ALIGNED(who, x, patch % 8 ? 4 : 16);  // pairs move 4-byte words, wide items 16-byte chunks
  TAD_REQUIRE_ALIGNED(who, cols, patch % 8 ? 4 : 16);
  const int64_t pixels = (int64_t)B * C * T * H * W;
  if (patch % 8)
    hipLaunchKernelGGL(w16_pairs_kernel, dim3(capped_grid(pixels / 2, 256)), dim3(256), 0, (hipStream_t)stream, x, cols, B, C, T, H, W, tubelet,
                       patch, tad_patch_embed_ldk(C, tubelet, patch));
  else
    hipLaunchKernelGGL(w16_wide_kernel, dim3(capped_grid(pixels / 8, 256)), dim3(256), 0, (hipStream_t)stream, x, cols, B, C, T, H, W, tubelet,
                       patch);
  return check_launch(who);
}

// (the caller has checked its arguments)
template <int FMT, typename Slots>
static int from_u8(const char* who, const uint8_t* frames, Slots slots, uint16_t* cols, int B, int T, int H, int W, int tubelet, int patch,
                   const float* m, const float* s, int bgr, tad_stream_t stream) {
  const int64_t pixels = (int64_t)B * T * H * W;
  if (patch % 8)
    hipLaunchKernelGGL((u8_pairs_kernel<FMT, Slots>), dim3(capped_grid(pixels / 2, 256)), dim3(256), 0, (hipStream_t)stream, frames, cols, B,
                       T, H, W, tubelet, patch, tad_patch_embed_ldk(3, tubelet, patch), m[0], m[1], m[2], s[0], s[1], s[2], bgr ? 1 : 0, slots);
  else
    hipLaunchKernelGGL((u8_wide_kernel<FMT, Slots>), dim3(capped_grid(pixels / 8, 256)), dim3(256), 0, (hipStream_t)stream, frames, cols, B,
                       T, H, W, tubelet, patch, m[0], m[1], m[2], s[0], s[1], s[2], bgr ? 1 : 0, slots);
  return check_launch(who);
}

template <int FMT>
static int from_ring(const uint8_t* frames, uint16_t* cols, int B, int T, int H, int W, int tubelet, int patch, const float* mean3,
                     const float* std3, int bgr, int t_offset, tad_stream_t stream) {
  if (int rc = check_args("im2col_u8", frames, cols, B, 3, T, H, W, tubelet, patch, true, mean3, std3, "frames")) return rc;
  TAD_REQUIRE(t_offset >= 0 && t_offset < T, "im2col_u8: t_offset=%d outside [0, %d)", t_offset, T);
  return from_u8<FMT>("im2col_u8", frames, RingSlots{t_offset}, cols, B, T, H, W, tubelet, patch, mean3, std3, bgr, stream);
}

}  // namespace im2col
}  // namespace tad

using namespace tad;
using namespace tad::im2col;

extern "C" {

int tad_im2col_tubelets(const float* x, uint16_t* cols, int B, int C, int T, int H, int W, int tubelet, int patch, tad_stream_t stream) {
  return from_f32<TAD_BF16>("im2col", x, cols, B, C, T, H, W, tubelet, patch, stream);
}
int tad_im2col_tubelets_f16(const float* x, uint16_t* cols, int B, int C, int T, int H, int W, int tubelet, int patch, tad_stream_t stream) {
  return from_f32<TAD_F16>("im2col", x, cols, B, C, T, H, W, tubelet, patch, stream);
}
int tad_im2col_tubelets_f32(const float* x, float* cols, int B, int C, int T, int H, int W, int tubelet, int patch, tad_stream_t stream) {
  return from_f32<TAD_F32>("im2col_f32", x, cols, B, C, T, H, W, tubelet, patch, stream);
}

int tad_im2col_tubelets_16(const uint16_t* x, uint16_t* cols, int B, int C, int T, int H, int W, int tubelet, int patch, tad_stream_t stream) {
  return from_16("im2col_16", x, cols, B, C, T, H, W, tubelet, patch, stream);
}

int tad_im2col_tubelets_u8(const uint8_t* frames, uint16_t* cols, int B, int T, int H, int W, int tubelet, int patch, const float* mean3,
                           const float* std3, int bgr, int t_offset, tad_stream_t stream) {
  return from_ring<TAD_BF16>(frames, cols, B, T, H, W, tubelet, patch, mean3, std3, bgr, t_offset, stream);
}
int tad_im2col_tubelets_u8_f16(const uint8_t* frames, uint16_t* cols, int B, int T, int H, int W, int tubelet, int patch, const float* mean3,
                               const float* std3, int bgr, int t_offset, tad_stream_t stream) {
  return from_ring<TAD_F16>(frames, cols, B, T, H, W, tubelet, patch, mean3, std3, bgr, t_offset, stream);
}

int tad_im2col_frame_windows(const uint8_t* store, int64_t F, const int32_t* idx, void* cols, int cols_dtype, int B, int T, int H, int W,
                             int tubelet, int patch, const float* mean3, const float* std3, int bgr, tad_stream_t stream) {
  const char* who = "im2col_frame_windows";
  TAD_REQUIRE(idx, "%s: null pointer", who);
  TAD_REQUIRE(F > 0, "%s: the store holds F=%lld frames (must be positive)", who, (long long)F);
  TAD_REQUIRE(cols_dtype == TAD_BF16 || cols_dtype == TAD_F16, "%s: cols_dtype=%d must be TAD_BF16 or TAD_F16", who, cols_dtype);
  TAD_REQUIRE(T > 0 && H > 0 && W > 0, "%s: T/H/W must be multiples of tubelet/patch (got T=%d H=%d W=%d)", who, T, H, W);
  if (int rc = check_args(who, store, cols, B, 3, T, H, W, tubelet, patch, true, mean3, std3, "store")) return rc;
  TAD_REQUIRE_ALIGNED(who, idx, 4);
  const TableSlots slots = {idx, F};
  if (cols_dtype == TAD_F16) return from_u8<TAD_F16>(who, store, slots, (uint16_t*)cols, B, T, H, W, tubelet, patch, mean3, std3, bgr, stream);
  return from_u8<TAD_BF16>(who, store, slots, (uint16_t*)cols, B, T, H, W, tubelet, patch, mean3, std3, bgr, stream);
}

}  // extern "C"
