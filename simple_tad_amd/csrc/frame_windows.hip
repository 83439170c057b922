// Batched input stage for overlapping windows: the patch matrix of B windows read from ONE device-resident frame store.
//   store [F,H,W,3] uint8 (decoder / cv2 layout), idx [B,T] int32 on the device: frame t of window b is slot idx[b*T + t] of the store
//   cols  [B*N, ldk] in the 16-bit operand format the caller names (TAD_BF16 / TAD_F16)
// The reference decodes, resizes and uploads all T frames of every test window again (dota.py:274-284 load_images): at view_step 1 every frame
// travels T times.  Here a video is uploaded once and its windows are a table of slots.
//
// These are the two kernels of tad_im2col_tubelets_u8 (elementwise.hip) with ONE change in the address: slot = idx[b*T + t] and the base
// store + slot*H*W*3 in place of (t + t_offset) % T inside clip b.  Same work decomposition (one thread = 8 pixels of a row for patch sizes that
// are multiples of 8, else 2 pixels with the padding columns zeroed by the owner of k = 0), same grid-stride form and cap, same arithmetic
//   v = (float(u8) / 255.0f - mean[c]) / std[c]      two IEEE divisions and one subtraction: nothing a contraction could fuse
// and the same round-to-nearest-even cast, so cols is bit-identical to tad_im2col_tubelets_u8 on the materialised clip store[idx].
// Compiled ONCE: the operand format is a template argument (both casts exist in one translation unit), not a second pass over the file.
//
// The index table lives on the device, so the entry point cannot check it: callers validate 0 <= idx < F on the host (frame_store.py does), and
// as a defence the kernels clamp a slot into [0, F-1] -- a bad table yields a wrong frame, never an address outside the store.
#include "common.h"

namespace tad {
namespace frame_windows {

static inline int capped_grid(int64_t work_items, int block) {  // = elementwise.hip's: at most 2048 blocks, grid-stride beyond
  int64_t g = (work_items + block - 1) / block;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

template <int FMT>
__device__ __forceinline__ uint32_t pack16x2(float lo, float hi) {
  if constexpr (FMT == TAD_F16) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    h2 v;
    v[0] = (_Float16)lo;
    v[1] = (_Float16)hi;
    return __builtin_bit_cast(uint32_t, v);
  } else {
    typedef __attribute__((ext_vector_type(2))) __bf16 b2;
    b2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(uint32_t, v);
  }
}

__device__ __forceinline__ int64_t clamped_slot(const int32_t* __restrict__ idx, int64_t at, int64_t F) {
  const int64_t s = idx[at];
  return s < 0 ? 0 : (s >= F ? F - 1 : s);
}

// One thread: 8 consecutive pixels of one row = 24 contiguous bytes in, three 16-byte chunks out (one per channel).
template <int FMT>
__global__ void im2col_frame_windows_kernel(const uint8_t* __restrict__ store, int64_t F, const int32_t* __restrict__ idx,
                                            uint16_t* __restrict__ cols, int B, int T, int H, int W, int tub, int p, float m0, float m1, float m2,
                                            float s0, float s1, float s2, int bgr) {
  const int W8 = W >> 3;
  const int64_t total = (int64_t)B * T * H * W8;
  const int Hp = H / p, Wp = W / p, Tp = T / tub;
  const int K = 3 * tub * p * p;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t r = i;
    const int w8 = (int)(r % W8); r /= W8;
    const int h = (int)(r % H); r /= H;
    const int t = (int)(r % T); r /= T;  // frame index inside the window
    const int b = (int)r;
    const int64_t slot = clamped_slot(idx, (int64_t)b * T + t, F);
    const uint8_t* src = store + ((slot * H + h) * W + (int64_t)w8 * 8) * 3;
    uint32_t raw[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) raw[q] = reinterpret_cast<const uint32_t*>(src)[q];  // (W*3*8) % 4 == 0: 4-byte aligned
    const int w = w8 * 8;
    const int tp = t / tub, kt = t - tp * tub, hp = h / p, kh = h - hp * p, wp = w / p, kw = w - wp * p;
    const int64_t n = ((int64_t)b * Tp + tp) * Hp * Wp + (int64_t)hp * Wp + wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int cm = bgr ? 2 - c : c;  // channel position in memory
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int byte = e * 3 + cm;
        const float u = (float)((raw[byte >> 2] >> ((byte & 3) * 8)) & 0xffu);
        v[e] = (u / 255.0f - mean[c]) / sd[c];
      }
      const int k = ((c * tub + kt) * p + kh) * p + kw;
      *reinterpret_cast<uint4*>(cols + n * K + k) =
          make_uint4(pack16x2<FMT>(v[0], v[1]), pack16x2<FMT>(v[2], v[3]), pack16x2<FMT>(v[4], v[5]), pack16x2<FMT>(v[6], v[7]));
    }
  }
}

// Even patch sizes that are not multiples of 8 (/14): one thread = 2 pixels = 6 contiguous bytes in, three 4-byte pairs out (a pair never
// straddles a patch: p and w are even); rows have stride ldk = K rounded up to 64 and the thread that owns k = 0 of a token zeroes the padding.
template <int FMT>
__global__ void im2col_frame_windows_pairs_kernel(const uint8_t* __restrict__ store, int64_t F, const int32_t* __restrict__ idx,
                                                  uint16_t* __restrict__ cols, int B, int T, int H, int W, int tub, int p, int ldk, float m0,
                                                  float m1, float m2, float s0, float s1, float s2, int bgr) {
  const int W2 = W >> 1;
  const int64_t total = (int64_t)B * T * H * W2;
  const int Hp = H / p, Wp = W / p, Tp = T / tub;
  const int K = 3 * tub * p * p;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t r = i;
    const int w2 = (int)(r % W2); r /= W2;
    const int h = (int)(r % H); r /= H;
    const int t = (int)(r % T); r /= T;
    const int b = (int)r;
    const int64_t slot = clamped_slot(idx, (int64_t)b * T + t, F);
    const uint8_t* src = store + ((slot * H + h) * W + (int64_t)w2 * 2) * 3;  // 6 bytes, 2-byte aligned
    const uint16_t* s2p = reinterpret_cast<const uint16_t*>(src);
    const uint32_t lo = (uint32_t)s2p[0] | ((uint32_t)s2p[1] << 16);  // bytes 0..3
    const uint32_t hi = (uint32_t)s2p[2];                             // bytes 4..5
    const int w = w2 * 2;
    const int tp = t / tub, kt = t - tp * tub, hp = h / p, kh = h - hp * p, wp = w / p, kw = w - wp * p;
    const int64_t n = ((int64_t)b * Tp + tp) * Hp * Wp + (int64_t)hp * Wp + wp;
    uint16_t* row = cols + n * ldk;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int cm = bgr ? 2 - c : c;
      const int b0 = cm, b1 = 3 + cm;  // byte positions of the two pixels' channel
      const float u0 = (float)((lo >> (b0 * 8)) & 0xffu);
      const float u1 = (float)(((b1 < 4 ? lo >> (b1 * 8) : hi >> ((b1 - 4) * 8))) & 0xffu);
      const int k = ((c * tub + kt) * p + kh) * p + kw;
      *reinterpret_cast<uint32_t*>(row + k) = pack16x2<FMT>((u0 / 255.0f - mean[c]) / sd[c], (u1 / 255.0f - mean[c]) / sd[c]);
    }
    if (kt == 0 && kh == 0 && kw == 0)  // (k = 0 of channel 0)
      for (int z = K; z < ldk; z += 2) *reinterpret_cast<uint32_t*>(row + z) = 0u;
  }
}

template <int FMT>
static void launch(const uint8_t* store, int64_t F, const int32_t* idx, uint16_t* cols, int B, int T, int H, int W, int tubelet, int patch,
                   const float* m, const float* s, int bgr, hipStream_t st) {
  if (patch % 8) {  // rows of stride tad_patch_embed_ldk, zero-padded (ViT-L/14: K = 1176 -> 1216)
    const int ldk = tad_patch_embed_ldk(3, tubelet, patch);
    const int64_t pairs = (int64_t)B * T * H * (W / 2);
    hipLaunchKernelGGL(im2col_frame_windows_pairs_kernel<FMT>, dim3(capped_grid(pairs, 256)), dim3(256), 0, st, store, F, idx, cols, B, T, H, W,
                       tubelet, patch, ldk, m[0], m[1], m[2], s[0], s[1], s[2], bgr ? 1 : 0);
    return;
  }
  const int64_t total = (int64_t)B * T * H * (W / 8);
  hipLaunchKernelGGL(im2col_frame_windows_kernel<FMT>, dim3(capped_grid(total, 256)), dim3(256), 0, st, store, F, idx, cols, B, T, H, W, tubelet,
                     patch, m[0], m[1], m[2], s[0], s[1], s[2], bgr ? 1 : 0);
}

}  // namespace frame_windows
}  // namespace tad

using namespace tad;

extern "C" int tad_im2col_frame_windows(const uint8_t* store, int64_t F, const int32_t* idx, void* cols, int cols_dtype, int B, int T, int H, int W,
                                        int tubelet, int patch, const float* mean3, const float* std3, int bgr, tad_stream_t stream) {
  TAD_REQUIRE(store && idx && cols && mean3 && std3, "im2col_frame_windows: null pointer");
  TAD_REQUIRE(F > 0, "im2col_frame_windows: the store holds F=%lld frames (must be positive)", (long long)F);
  TAD_REQUIRE(cols_dtype == TAD_BF16 || cols_dtype == TAD_F16, "im2col_frame_windows: cols_dtype=%d must be TAD_BF16 or TAD_F16", cols_dtype);
  TAD_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && tubelet > 0 && patch > 0 && T % tubelet == 0 && H % patch == 0 && W % patch == 0,
              "im2col_frame_windows: T/H/W must be multiples of tubelet/patch (got B=%d T=%d H=%d W=%d tub=%d p=%d)", B, T, H, W, tubelet, patch);
  TAD_REQUIRE(patch % 2 == 0, "im2col_frame_windows: patch size must be even (got %d)", patch);
  TAD_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "im2col_frame_windows: zero std");
  TAD_REQUIRE((((uintptr_t)store | (uintptr_t)idx) & 3) == 0 && (((uintptr_t)cols) & 15) == 0,
              "im2col_frame_windows: misaligned buffers (store and idx 4 bytes, cols 16 bytes)");
  if (cols_dtype == TAD_F16)
    frame_windows::launch<TAD_F16>(store, F, idx, (uint16_t*)cols, B, T, H, W, tubelet, patch, mean3, std3, bgr, (hipStream_t)stream);
  else
    frame_windows::launch<TAD_BF16>(store, F, idx, (uint16_t*)cols, B, T, H, W, tubelet, patch, mean3, std3, bgr, (hipStream_t)stream);
  return check_launch("im2col_frame_windows");
}
