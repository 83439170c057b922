// What the row-norm kernels (layernorm.hip, rmsnorm.hip) have in common.  Their shape: HBM-bound, one wave per row of D f32 elements
// (D % 4 == 0, D <= 2048), the row held in registers as NV float4 per lane (one per 256 columns) and read once; in the backward a block
// owns a contiguous chunk of rows, each wave walks it with stride 4 and keeps per-lane column partials of the parameter gradients, the
// block's 4 waves are combined in LDS into one partial row per block and quantity, and launch_reduce_cols adds the blocks in a fixed
// order (no atomics).  The decisions both files must take identically live here, once: which instance serves a width, how rows are dealt
// to blocks, the partial layout, and the float4 / 16-bit helpers.
#pragma once
#include "common.h"

TAD_NAMESPACE_BEGIN

constexpr int ROWNORM_MAX_V = 8;                      // float4 per lane
constexpr int ROWNORM_MAX_D = 64 * 4 * ROWNORM_MAX_V;  // 2048

static inline bool rownorm_width_ok(int D) { return D > 0 && D % 4 == 0 && D <= ROWNORM_MAX_D; }
// float4 per lane of a row of D columns: the kernels' NV
static inline int rownorm_nv(int D) { return (D / 4 + 63) / 64; }

// One instance per float4 count, and NV is ALWAYS rownorm_nv(D): a backward's FULL variant drops the per-lane column guard on the strength
// of D == 256 * NV, so a launcher tests exactly that, on the NV of the case it stands in (nv = 7, D = 1792: an NV = 8 instance would run
// its eighth chunk into the next row).  A width rownorm_width_ok() accepts has one of these eight cases.
#define ROWNORM_SWITCH_NV(nv, M_) \
  switch (nv) {                   \
    case 1: M_(1); break;         \
    case 2: M_(2); break;         \
    case 3: M_(3); break;         \
    case 4: M_(4); break;         \
    case 5: M_(5); break;         \
    case 6: M_(6); break;         \
    case 7: M_(7); break;         \
    case 8: M_(8); break;         \
  }

// Backward geometry for nq column quantities: blocks of >= 32 rows (at most 1024 of them), the f32 partials [nq][blocks][D] in the
// workspace and the LDS of the cross-wave combine [4][nq][D].
struct RowNormBwd {
  int blocks, rows_per_block;
  size_t partial_floats, smem_bytes;
};
static inline int rownorm_bwd_blocks(int64_t rows) {
  int64_t b = (rows + 31) / 32;
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  return (int)b;
}
static inline RowNormBwd rownorm_bwd_plan(int64_t rows, int D, int nq) {
  const int blocks = rownorm_bwd_blocks(rows);
  return {blocks, (int)((rows + blocks - 1) / blocks), (size_t)nq * blocks * (size_t)D, (size_t)4 * nq * D * sizeof(float)};
}

int launch_reduce_cols(const float* partial, float* out0, float* out1, float* out2, int nq, int splits, int n, int accumulate,
                       hipStream_t st);

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 mul4(const float4& a, const float4& b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 scale4(const float4& a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ void acc4(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ float sumsq4(const float4& v) { return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
// four packed 16-bit values of format FMT <-> f32; down: round-to-nearest-even, a NaN stays a NaN (pack16x2, common.h)
template <int FMT>
__device__ __forceinline__ float4 unpack16x4(const uint2& p) {
  return make_float4(lo16_f32<FMT>(p.x), hi16_f32<FMT>(p.x), lo16_f32<FMT>(p.y), hi16_f32<FMT>(p.y));
}
template <int FMT>
__device__ __forceinline__ uint2 pack16x4(const float4& o) {
  uint2 p;
  p.x = pack16x2<FMT>(o.x, o.y);
  p.y = pack16x2<FMT>(o.z, o.w);
  return p;
}

// The cross-wave combine that ends a backward kernel.  Each wave stages its NQ register sets (`sets`: NQ arrays float4[NV], in the order of
// the partial rows) in LDS as [wave][NQ][D4]; then the block's threads walk the first nq_written quantities, add waves 1..3 to wave 0 in
// that order and write partial[q][gridDim.x][D]: one row per block and quantity, so launch_reduce_cols reduces each quantity on its own.
// `wave` is the caller's (wave-uniform) wave index.  The sets come as separate arrays, not as one float4[NQ][NV]: the kernels' registers
// then are what they were when each kernel wrote this out itself.
template <int NV, typename... Sets>
__device__ __forceinline__ void rownorm_combine(float* partial, int D, int nq_written, int wave, const Sets&... sets) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // the block's dynamic LDS: [4][NQ][D], rownorm_bwd_plan's smem_bytes
  constexpr int NQ = sizeof...(Sets);
  const int lane = threadIdx.x & 63;
  const int D4 = D >> 2;
  float4* sm = reinterpret_cast<float4*>(smem);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) {
      int q = 0;
      ((sm[(wave * NQ + q++) * D4 + c] = sets[i]), ...);
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < nq_written * D4; idx += 256) {
    const int q = NQ == 1 ? 0 : idx / D4, c = idx - q * D4;
    float4 a = sm[q * D4 + c];
#pragma unroll
    for (int w = 1; w < 4; ++w) acc4(a, sm[(w * NQ + q) * D4 + c]);
    reinterpret_cast<float4*>(partial + ((int64_t)q * gridDim.x + blockIdx.x) * D)[c] = a;
  }
}

TAD_NAMESPACE_END
