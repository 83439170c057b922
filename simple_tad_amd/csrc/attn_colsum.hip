// Weighted column sum of the softmax matrix, recomputed flash-style (no N x N tensor), head_dim 64 / 80, gfx950:
//   out[b,h,j] = sum_{i<N} w[b,i] * exp(scale * q_{b,h,i} . k_{b,h,j} - lse[b,h,i])
// The step of attention rollout when only one row vector is propagated (simple_tad_amd/explain.py); with
// w = 1/N the attention each token receives, with a one-hot w one row of P.
//
// The data flow of attn_bwd_dkv_kernel (attn_bwd.hip) with neither V nor dO: one workgroup = 128 keys of one (b, h) (32 per wave, K
// fragments pinned in registers), loops over 64-row query tiles staged by LDS-DMA (same swizzled image), the row constants lse and w
// (raw, 4 bytes per lane) staged next to them.  S = Q K^T with the key on the lane; one exp2 turns the accumulators into P; each lane
// sums w_i P_ij over its 16 rows of a half tile into four f32 chains (one per group of four accumulator registers), the chains and the
// two lane halves are added at the end.  P and the sums stay f32: nothing is rounded to 16 bits.  No atomics, no cross-workgroup
// reduction, one fixed summation order: bit-reproducible.
// Compiled once: the operand format is a template argument (the only difference is the MFMA opcode), as in im2col.hip.
#include <type_traits>
#include "common.h"

TAD_NAMESPACE_BEGIN

namespace colsum {

constexpr float LOG2E = 1.44269504088896340736f;

// 16-byte chunk swizzle of the 128-byte tile rows (attn_bwd.hip: sw_dual)
__device__ __forceinline__ int sw_dual(int row) {
  return ((row >> 1) & 1) | (((row >> 2) & 1) << 1) | ((((row >> 1) ^ (row >> 3)) & 1) << 2);
}

template <int FMT>
__device__ __forceinline__ f32x16 mfma_32x32x16(const i32x4& a, const i32x4& b, const f32x16& c) {
  if constexpr (FMT == TAD_F16) {
    typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
  } else {
    typedef __attribute__((ext_vector_type(8))) __bf16 b16x8;
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b16x8, a), __builtin_bit_cast(b16x8, b), c, 0, 0, 0);
  }
}

// QS: the q third of qkv carries scale * log2(e) (see attn_fwd.hip): the scores are in log2 units; else the factor is applied to the f32 scores.
// HD: 64, or 80 as 64 + 16 (dims 64..79 of the Q tile travel in a side image of 32-byte rows, the score product gets a fifth k-step).
template <int HD, int FMT, bool QS>
__global__ __launch_bounds__(256, 2) void attn_colsum_kernel(const uint16_t* __restrict__ qkv, const float* __restrict__ lse,
                                                             const float* __restrict__ w, float* __restrict__ out, int N, int H, float scale) {
  static_assert(HD == 64 || HD == 80, "head dim");
  constexpr bool X = HD == 80;
  constexpr int NKS = HD / 16;
  constexpr int TILE_BYTES = 64 * 128;
  constexpr int RC_OFF = TILE_BYTES;        // 64 x lse, then 64 x w
  constexpr int SIDE_OFF = TILE_BYTES + 512;
  constexpr int SIDE_BYTES = X ? 64 * 32 : 0;
  constexpr int STAGE = SIDE_OFF + SIDE_BYTES;
  constexpr int NST = 2;
  __shared__ __attribute__((aligned(1024))) char lds[NST * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nblk = (N + 127) / 128;  // 1-D XCD-aware grid: the key blocks of one (batch, head) pair share their Q tiles in an L2
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int head = (lin / nblk) % H, b = lin / nblk / H;
  const int key0 = (lin % nblk) * 128 + wave * 32;
  const int kl_ = lane & 31, h5 = lane >> 5;
  const int64_t tok = (int64_t)3 * H * HD;
  const uint16_t* kbase = qkv + (int64_t)b * N * tok + (int64_t)H * HD + head * HD;
  const float c = scale * LOG2E;

  int krow = key0 + kl_;
  const bool kvalid = krow < N;
  const bool wave_live = key0 < N;  // wave-uniform
  if (!kvalid) krow = N - 1;        // (a key of this clip: computed, never stored)
  i32x4 kfr[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) kfr[ks] = *reinterpret_cast<const i32x4*>(kbase + (int64_t)krow * tok + 16 * ks + 8 * h5);

  // Q tiles go global -> LDS by LDS-DMA (1-KiB piece = 8 rows x 128 B, wave w moves pieces w and w+4; swizzle on the per-lane SOURCE
  // chunk).  Every descriptor ends with the rows of this workgroup's clip (lse: of its head): rows >= N read as zero, never the next
  // clip's; they are excluded by selection below as well.
  const uint32_t qkv_bytes = (uint32_t)(b + 1) * (uint32_t)N * (uint32_t)tok * 2u;
  const auto rs_qkv = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(qkv), 0, (int)qkv_bytes, 0x00020000);
  uint32_t dma_q[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wave + 4 * i) * 8 + (lane >> 3);
    dma_q[i] = (uint32_t)(((int64_t)b * N + row) * tok * 2) + (uint32_t)(head * HD * 2) + (uint32_t)(((lane & 7) ^ sw_dual(row)) << 4);
  }
  const uint32_t q_step = (uint32_t)(tok * 2);
  // side image (HD 80): waves 2 / 3 move its two halves (32 rows x 32 B each)
  const uint32_t dma_s = (uint32_t)(((int64_t)b * N + 32 * (wave & 1) + (lane >> 1)) * tok * 2) + (uint32_t)(head * HD * 2) + 128u + (uint32_t)((lane & 1) << 4);
  // row constants: wave 0 moves the tile's 64 lse values, wave 1 its 64 w values (4 bytes per lane)
  const int64_t bh = (int64_t)b * H + head;
  const auto rs_lse = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(lse), 0, (int)((bh + 1) * N * 4), 0x00020000);
  const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(w), 0, (int)(((int64_t)b + 1) * N * 4), 0x00020000);
  const uint32_t lse_off = (uint32_t)((bh * N + lane) * 4), w_off = (uint32_t)(((int64_t)b * N + lane) * 4);
#define LOAD_Q(buf, q0)                                                                                                                     \
  {                                                                                                                                         \
    char* ql_ = lds + (buf) * STAGE;                                                                                                        \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                                           \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_qkv, LDS_PTR(ql_ + (wave + 4 * i) * 1024), 16, dma_q[i] + (uint32_t)(q0) * q_step, 0, 0, 0); \
    if (wave == 0) /* wave-uniform */                                                                                                       \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_lse, LDS_PTR(ql_ + RC_OFF), 4, lse_off + (uint32_t)(q0) * 4u, 0, 0, 0);                   \
    if (wave == 1)                                                                                                                          \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, LDS_PTR(ql_ + RC_OFF + 256), 4, w_off + (uint32_t)(q0) * 4u, 0, 0, 0);                 \
    if constexpr (X) {                                                                                                                      \
      if (wave >= 2)                                                                                                                        \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_qkv, LDS_PTR(ql_ + SIDE_OFF + (wave & 1) * 1024), 16, dma_s + (uint32_t)(q0) * q_step, 0, 0, 0); \
    }                                                                                                                                       \
  }

  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // one chain per group of four accumulator registers

  const int nt = (N + 63) / 64;
  LOAD_Q(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // the tile loop runs in pairs so that the ring slot is a literal in each copy of the body (as in attn_bwd.hip)
  auto tile = [&](auto BUFC, int t) {
    constexpr int BUF = decltype(BUFC)::value;
    if (t + 1 < nt) LOAD_Q(BUF ^ 1, (t + 1) * 64);  // (its last reader passed the barrier that ended tile t - 1)
    const char* ql = lds + BUF * STAGE;
    if (wave_live) {  // (waves whose 32 keys all lie past the sequence only stage tiles)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int row0 = t * 64 + 32 * qt;
        if (row0 >= N) break;  // half tile of query rows past the sequence
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        const int qrow = qt * 32 + kl_;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          s = mfma_32x32x16<FMT>(*reinterpret_cast<const i32x4*>(ql + qrow * 128 + (((2 * ks + h5) ^ sw_dual(qrow)) << 4)), kfr[ks], s);
        if constexpr (X) s = mfma_32x32x16<FMT>(*reinterpret_cast<const i32x4*>(ql + SIDE_OFF + qrow * 32 + h5 * 16), kfr[NKS - 1], s);
        // accumulator register r <-> row (r & 3) + 8 (r >> 2) + 4 h5 of the half tile: its constants are four floats at [8 r4 + 4 h5]
        f32x4 l4[4], w4[4];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          l4[r4] = *reinterpret_cast<const f32x4*>(ql + RC_OFF + (qt * 32 + 8 * r4 + 4 * h5) * 4);
          w4[r4] = *reinterpret_cast<const f32x4*>(ql + RC_OFF + 256 + (qt * 32 + 8 * r4 + 4 * h5) * 4);
        }
        f32x16 p;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float lse2 = l4[r >> 2][r & 3] * LOG2E;
          p[r] = fast_exp2(QS ? s[r] - lse2 : fmaf(s[r], c, -lse2));
        }
        if (row0 + 32 > N) {  // ragged half tile: rows >= N are excluded by SELECTION (their P may be anything, NaN included)
          int lim = N - row0 - 4 * h5;
          asm volatile("" : "+v"(lim));  // (one lane value against 16 literals: see attn_bwd_dkv_kernel)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if ((r & 3) + 8 * (r >> 2) >= lim) { p[r] = 0.f; w4[r >> 2][r & 3] = 0.f; }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r >> 2] = fmaf(w4[r >> 2][r & 3], p[r], acc[r >> 2]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  for (int t = 0; t < nt; t += 2) {
    tile(std::integral_constant<int, 0>{}, t);
    if (t + 1 < nt) tile(std::integral_constant<int, 1>{}, t + 1);
  }
#undef LOAD_Q

  if (wave_live) {
    const float mine = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine), __float_as_uint(mine), false, false);
    const float total = __uint_as_float(r[0]) + __uint_as_float(r[1]);  // the two lane halves (16 rows of every half tile each)
    if (kvalid && h5 == 0) out[bh * N + krow] = total;
  }
}

typedef void (*ColsumKernel)(const uint16_t*, const float*, const float*, float*, int, int, float);
template <int FMT>
static ColsumKernel pick(int d, int qs) {
  if (d == 80) return qs ? attn_colsum_kernel<80, FMT, true> : attn_colsum_kernel<80, FMT, false>;
  return qs ? attn_colsum_kernel<64, FMT, true> : attn_colsum_kernel<64, FMT, false>;
}

}  // namespace colsum

TAD_NAMESPACE_END

using namespace tad;

extern "C" int tad_attn_colsum(const uint16_t* qkv, int op_dtype, const float* lse, const float* w, float* out, int B, int N, int H, int d,
                               float scale, int q_prescaled, tad_stream_t stream) {
  TAD_REQUIRE(qkv && lse && w && out, "attn_colsum: null pointer");
  TAD_REQUIRE_ALIGNED("attn_colsum", qkv, 16);  // (16-byte LDS-DMA pieces and fragment loads; lse, w and out move as single floats)
  TAD_REQUIRE(d == 64 || d == 80, "attn_colsum: head_dim must be 64 or 80 (got %d)", d);
  TAD_REQUIRE(op_dtype == TAD_BF16 || op_dtype == TAD_F16, "attn_colsum: op_dtype must be TAD_BF16 or TAD_F16");
  TAD_REQUIRE(B > 0 && N > 0 && H > 0 && H <= 65535 && B <= 65535, "attn_colsum: bad shape B=%d N=%d H=%d", B, N, H);
  TAD_REQUIRE(scale > 0.f, "attn_colsum: scale must be positive");
  // qkv, lse and w are addressed through buffer descriptors with 32-bit byte offsets (staging by LDS-DMA)
  TAD_REQUIRE((int64_t)B * N * 3 * H * d * 2 < (1ll << 32), "attn_colsum: qkv exceeds the 4 GiB buffer descriptor (B=%d N=%d H=%d)", B, N, H);
  TAD_REQUIRE((int64_t)B * H * N * 4 < (1ll << 31), "attn_colsum: B*H*N too large for the row-constant descriptor");
  const int64_t grid = (int64_t)((N + 127) / 128) * H * B;
  TAD_REQUIRE(grid < (1ll << 31), "attn_colsum: grid too large");
  const colsum::ColsumKernel k = op_dtype == TAD_F16 ? colsum::pick<TAD_F16>(d, q_prescaled != 0) : colsum::pick<TAD_BF16>(d, q_prescaled != 0);
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, qkv, lse, w, out, N, H, scale);
  return check_launch("attn_colsum_kernel");
}
