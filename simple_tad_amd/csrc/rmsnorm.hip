// RMSNorm forward / backward for rows of D f32 elements (D % 4 == 0, D <= 2048), and the RMS normalisation of the q and k thirds of a
// qkv row over their full H*d width (InternVideo2's qk_normalization): the extension ABI of include/tad_mi355x_ext.h (tadx_*).
// Same shape as layernorm.hip: HBM-bound, one wave per row, the row lives in registers (float4 per lane per 256 columns) and is read
// once, wave reductions by cross-lane steps, per-block column partials of the gamma gradients reduced in a fixed order (no atomics).
// Compiled ONCE: the 16-bit format of an operand is a run-time argument (TAD_BF16 / TAD_F16) that selects a template instance, so there
// are no _f16 twins.
#include "common.h"
#include "../../include/tad_mi355x_ext.h"

TAD_NAMESPACE_BEGIN

constexpr int RMS_MAX_V = 8;  // float4 per lane -> D <= 64*4*8 = 2048

int launch_reduce_cols(const float* partial, float* out0, float* out1, float* out2, int nq, int splits, int n, int accumulate,
                       hipStream_t st);

// a packed pair of 16-bit values of format FMT -> f32 (the run-time-format counterparts of op16_lo_f32 / op16_hi_f32)
template <int FMT>
__device__ __forceinline__ float lo16_f32(uint32_t w) {
  if constexpr (FMT == TAD_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
  else return __uint_as_float(w << 16);
}
template <int FMT>
__device__ __forceinline__ float hi16_f32(uint32_t w) {
  if constexpr (FMT == TAD_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
  else return __uint_as_float(w & 0xffff0000u);
}
template <int FMT>
__device__ __forceinline__ float4 unpack16x4(const uint2& p) {
  return make_float4(lo16_f32<FMT>(p.x), hi16_f32<FMT>(p.x), lo16_f32<FMT>(p.y), hi16_f32<FMT>(p.y));
}
// round-to-nearest-even, a NaN stays a NaN (pack16x2, common.h)
template <int FMT>
__device__ __forceinline__ uint2 pack16x4(const float4& o) {
  uint2 p;
  p.x = pack16x2<FMT>(o.x, o.y);
  p.y = pack16x2<FMT>(o.z, o.w);
  return p;
}
__device__ __forceinline__ float sumsq4(const float4& v) { return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ float4 mul4(const float4& a, const float4& b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 scale4(const float4& a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ void acc4(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// y = x * rsqrt(mean(x^2) + eps) * gamma.  YFMT: TAD_F32 / TAD_BF16 / TAD_F16.  Four rows per block, one per wave.
template <int NV, int YFMT>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, void* __restrict__ y,
                                                          float* __restrict__ rrms, int64_t rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int D4 = D >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x + row * D);
  float4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    v[i] = (c < D4) ? ldg_f4<false>(xr + c) : zero4();
    s += sumsq4(v[i]);
  }
  const float rr = rsqrtf(wave_sum(s) / (float)D + eps);
  if (lane == 0 && rrms) rrms[row] = rr;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) {
      const float4 o = mul4(scale4(v[i], rr), reinterpret_cast<const float4*>(gamma)[c]);
      if constexpr (YFMT == TAD_F32) stg_f4<false>(reinterpret_cast<float4*>((float*)y + row * D) + c, o);
      else stg_u2<false>(reinterpret_cast<uint2*>((uint16_t*)y + row * D) + c, pack16x4<YFMT>(o));
    }
  }
}

// Backward.  The layout of layernorm_bwd_kernel: each block owns a contiguous chunk of rows, each wave walks the chunk with stride 4 and
// keeps per-lane column partials of dgamma in registers; the block's 4 waves are combined in LDS and written as one partial row per
// block.  Everything a row needs is requested in one batch at the top (the load-batching and vmcnt notes of layernorm.hip apply
// unchanged); without a residual gradient the row of x is read a second time and multiplied by 0 so that the loads stay one block.
//   xh = x * rrms, t = dy * gamma:  dx = rrms * (t - xh * mean(t * xh)) (+ dres),  dgamma = sum_rows dy * xh
// An all-zero row: xh = 0, so dx = rrms * dy * gamma, finite.
template <int NV, int DYFMT, bool FULL>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const void* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ gamma, const float* __restrict__ rrms,
                                                          const float* __restrict__ dres, float* __restrict__ dx,
                                                          uint16_t* __restrict__ dx16, int dx16_fmt, float* __restrict__ partial /*[grid][D]*/,
                                                          int64_t rows, int D, int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [4][D]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int D4 = D >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(rows, r0 + rows_per_block);
  float4 g[NV], dg[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    g[i] = (c < D4) ? reinterpret_cast<const float4*>(gamma)[c] : zero4();
    dg[i] = zero4();
  }
  const float* const rsrc = dres ? dres : x;
  const float rmul = dres ? 1.f : 0.f;
  for (int64_t row = r0 + wave; row < r1; row += 4) {
    float4 xv[NV], dyv[NV], rv[NV];
    uint2 dyp[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (FULL || c < D4) {
        xv[i] = ldg_f4<false>(reinterpret_cast<const float4*>(x + row * D) + c);
        if constexpr (DYFMT == TAD_F32) dyv[i] = ldg_f4<false>(reinterpret_cast<const float4*>((const float*)dy + row * D) + c);
        else dyp[i] = ldg_u2<false>(reinterpret_cast<const uint2*>((const uint16_t*)dy + row * D) + c);
        rv[i] = ldg_f4<false>(reinterpret_cast<const float4*>(rsrc + row * D) + c);
      }
    }
    const float rr = rrms[row];
    __builtin_amdgcn_sched_barrier(0);  // the whole batch of loads stays above the arithmetic
    float4 xh[NV], t[NV];
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (FULL || c < D4) {
        if constexpr (DYFMT != TAD_F32) dyv[i] = unpack16x4<DYFMT>(dyp[i]);
        xh[i] = scale4(xv[i], rr);
        t[i] = mul4(dyv[i], g[i]);
        s2 += dot4(t[i], xh[i]);
        acc4(dg[i], mul4(dyv[i], xh[i]));
      } else {
        xh[i] = t[i] = rv[i] = zero4();
      }
    }
    const float c2 = wave_sum_dpp(s2) / (float)D;
    float4 o[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      o[i].x = fmaf(rv[i].x, rmul, rr * (t[i].x - xh[i].x * c2));
      o[i].y = fmaf(rv[i].y, rmul, rr * (t[i].y - xh[i].y * c2));
      o[i].z = fmaf(rv[i].z, rmul, rr * (t[i].z - xh[i].z * c2));
      o[i].w = fmaf(rv[i].w, rmul, rr * (t[i].w - xh[i].w * c2));
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (FULL || c < D4) stg_f4<false>(reinterpret_cast<float4*>(dx + row * D) + c, o[i]);
    }
    if (dx16) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (FULL || c < D4)
          stg_u2<false>(reinterpret_cast<uint2*>(dx16 + row * D) + c, dx16_fmt == TAD_F16 ? pack16x4<TAD_F16>(o[i]) : pack16x4<TAD_BF16>(o[i]));
      }
    }
  }
  // cross-wave combine, one partial row per block
  float4* sm = reinterpret_cast<float4*>(smem);  // [wave][D4]
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) sm[wave * D4 + c] = dg[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D4; c += 256) {
    float4 a = sm[c];
#pragma unroll
    for (int w = 1; w < 4; ++w) acc4(a, sm[w * D4 + c]);
    reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * D)[c] = a;
  }
}

// One pass over a qkv row [3A] f32: q third -> q * rq * gq * q_out_scale, k third -> k * rk * gk, v third cast; all rounded once to FMT.
// rq / rk = rsqrt(mean over the A columns of the third + eps).  Four rows per block, one per wave; the three thirds are requested together.
template <int NV, int FMT>
__global__ __launch_bounds__(256) void qk_rmsnorm_fwd_kernel(const float* __restrict__ qkv32, const float* __restrict__ gq,
                                                             const float* __restrict__ gk, uint16_t* __restrict__ qkv16,
                                                             float* __restrict__ rr, float q_out_scale, int64_t M, int A, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int A4 = A >> 2;
  const float4* src = reinterpret_cast<const float4*>(qkv32 + row * 3 * A);
  uint2* dst = reinterpret_cast<uint2*>(qkv16 + row * 3 * A);
  float4 q[NV], k[NV], v[NV];
  float sq = 0.f, sk = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < A4) {
      q[i] = ldg_f4<false>(src + c);
      k[i] = ldg_f4<false>(src + A4 + c);
      v[i] = ldg_f4<false>(src + 2 * A4 + c);
    } else {
      q[i] = k[i] = v[i] = zero4();
    }
    sq += sumsq4(q[i]);
    sk += sumsq4(k[i]);
  }
  const float rq = rsqrtf(wave_sum(sq) / (float)A + eps);
  const float rk = rsqrtf(wave_sum(sk) / (float)A + eps);
  if (lane == 0 && rr) {
    rr[2 * row] = rq;
    rr[2 * row + 1] = rk;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < A4) {
      const float4 oq = scale4(mul4(scale4(q[i], rq), reinterpret_cast<const float4*>(gq)[c]), q_out_scale);
      const float4 ok = mul4(scale4(k[i], rk), reinterpret_cast<const float4*>(gk)[c]);
      stg_u2<false>(dst + c, pack16x4<FMT>(oq));
      stg_u2<false>(dst + A4 + c, pack16x4<FMT>(ok));
      stg_u2<false>(dst + 2 * A4 + c, pack16x4<FMT>(v[i]));
    }
  }
}

// The way back: dqkv16 (tad_attn_bwd's output: the q third is the gradient of the normalised q BEFORE q_out_scale, see the header) through
// the two norms; the v third is copied.  Column partials of dgq and dgk per block: partial[q][grid][A].
template <int NV, int FMT>
__global__ __launch_bounds__(256) void qk_rmsnorm_bwd_kernel(const uint16_t* __restrict__ dqkv16, const float* __restrict__ qkv32,
                                                             const float* __restrict__ gq, const float* __restrict__ gk,
                                                             const float* __restrict__ rr, uint16_t* __restrict__ dpre16,
                                                             float* __restrict__ partial, int64_t M, int A, int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [4][2][A]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int A4 = A >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  float4 g0[NV], g1[NV], d0[NV], d1[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    g0[i] = (c < A4) ? reinterpret_cast<const float4*>(gq)[c] : zero4();
    g1[i] = (c < A4) ? reinterpret_cast<const float4*>(gk)[c] : zero4();
    d0[i] = d1[i] = zero4();
  }
  for (int64_t row = r0 + wave; row < r1; row += 4) {
    const float4* src = reinterpret_cast<const float4*>(qkv32 + row * 3 * A);
    const uint2* gsrc = reinterpret_cast<const uint2*>(dqkv16 + row * 3 * A);
    uint2* dst = reinterpret_cast<uint2*>(dpre16 + row * 3 * A);
    float4 q[NV], k[NV];
    uint2 pq[NV], pk[NV], pv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < A4) {
        q[i] = ldg_f4<false>(src + c);
        k[i] = ldg_f4<false>(src + A4 + c);
        pq[i] = ldg_u2<false>(gsrc + c);
        pk[i] = ldg_u2<false>(gsrc + A4 + c);
        pv[i] = ldg_u2<false>(gsrc + 2 * A4 + c);
      }
    }
    const float rq = rr[2 * row], rk = rr[2 * row + 1];
    __builtin_amdgcn_sched_barrier(0);
    float4 tq[NV], tk[NV];
    float sq = 0.f, sk = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < A4) {
        const float4 dq = unpack16x4<FMT>(pq[i]), dk = unpack16x4<FMT>(pk[i]);
        q[i] = scale4(q[i], rq);  // xh
        k[i] = scale4(k[i], rk);
        tq[i] = mul4(dq, g0[i]);
        tk[i] = mul4(dk, g1[i]);
        sq += dot4(tq[i], q[i]);
        sk += dot4(tk[i], k[i]);
        acc4(d0[i], mul4(dq, q[i]));
        acc4(d1[i], mul4(dk, k[i]));
      } else {
        q[i] = k[i] = tq[i] = tk[i] = zero4();
      }
    }
    const float cq = wave_sum_dpp(sq) / (float)A;
    const float ck = wave_sum_dpp(sk) / (float)A;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < A4) {
        const float4 oq = make_float4(rq * (tq[i].x - q[i].x * cq), rq * (tq[i].y - q[i].y * cq), rq * (tq[i].z - q[i].z * cq),
                                      rq * (tq[i].w - q[i].w * cq));
        const float4 ok = make_float4(rk * (tk[i].x - k[i].x * ck), rk * (tk[i].y - k[i].y * ck), rk * (tk[i].z - k[i].z * ck),
                                      rk * (tk[i].w - k[i].w * ck));
        stg_u2<false>(dst + c, pack16x4<FMT>(oq));
        stg_u2<false>(dst + A4 + c, pack16x4<FMT>(ok));
        stg_u2<false>(dst + 2 * A4 + c, pv[i]);
      }
    }
  }
  float4* sm = reinterpret_cast<float4*>(smem);  // [wave][2][A4]
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < A4) {
      sm[(wave * 2 + 0) * A4 + c] = d0[i];
      sm[(wave * 2 + 1) * A4 + c] = d1[i];
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 2 * A4; idx += 256) {
    const int qn = idx / A4, c = idx - qn * A4;
    float4 a = sm[qn * A4 + c];
#pragma unroll
    for (int w = 1; w < 4; ++w) acc4(a, sm[(w * 2 + qn) * A4 + c]);
    // partial layout: [q][grid][A], one quantity per reduce_cols row block
    reinterpret_cast<float4*>(partial + ((int64_t)qn * gridDim.x + blockIdx.x) * A)[c] = a;
  }
}

static inline int rms_bwd_blocks(int64_t rows) {
  int64_t b = (rows + 31) / 32;  // >= 32 rows per block
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  return (int)b;
}
static inline bool is_op16(int fmt) { return fmt == TAD_BF16 || fmt == TAD_F16; }

TAD_NAMESPACE_END

using namespace tad;

// One instance per float4 count: the kernels' NV must be the row's own (D / 256 rounded up), because the backward's FULL variant drops the
// column guard on the strength of D == 256 * NV.  (nv = 7, D = 1792: an NV = 8 instance would run its eighth chunk into the next row.)
#define RMS_SWITCH_NV(nv, M_) \
  switch (nv) {               \
    case 1: M_(1); break;     \
    case 2: M_(2); break;     \
    case 3: M_(3); break;     \
    case 4: M_(4); break;     \
    case 5: M_(5); break;     \
    case 6: M_(6); break;     \
    case 7: M_(7); break;     \
    default: M_(8); break;    \
  }

extern "C" {

int tadx_abi_version(void) { return TADX_ABI_VERSION; }

int tadx_rmsnorm_fwd(const float* x, const float* gamma, void* y, int y_dtype, float* rrms, int64_t rows, int D, float eps,
                     tad_stream_t stream) {
  TAD_REQUIRE(x && gamma && y, "rmsnorm_fwd: null pointer");
  TAD_REQUIRE(rows > 0 && D > 0 && D % 4 == 0 && D <= 64 * 4 * RMS_MAX_V, "rmsnorm_fwd: D=%d must be a multiple of 4 and <= %d", D,
              64 * 4 * RMS_MAX_V);
  TAD_REQUIRE(y_dtype == TAD_F32 || is_op16(y_dtype), "rmsnorm_fwd: bad y_dtype %d", y_dtype);
  // float4 loads of x and gamma; y: float4 stores (f32) or 8-byte packed stores (16-bit); rrms is written float by float
  TAD_REQUIRE_ALIGNED("rmsnorm_fwd", x, 16);
  TAD_REQUIRE_ALIGNED("rmsnorm_fwd", gamma, 16);
  TAD_REQUIRE_ALIGNED("rmsnorm_fwd", y, y_dtype == TAD_F32 ? 16 : 8);
  const int nv = (D / 4 + 63) / 64;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define RMS_FWD_(NV, F) hipLaunchKernelGGL((rmsnorm_fwd_kernel<NV, F>), grid, block, 0, st, x, gamma, y, rrms, rows, D, eps)
#define RMS_FWD(NV)                                 \
  if (y_dtype == TAD_F32) RMS_FWD_(NV, TAD_F32);    \
  else if (y_dtype == TAD_F16) RMS_FWD_(NV, TAD_F16); \
  else RMS_FWD_(NV, TAD_BF16);
  RMS_SWITCH_NV(nv, RMS_FWD)
#undef RMS_FWD
#undef RMS_FWD_
  return check_launch("rmsnorm_fwd");
}

size_t tadx_rmsnorm_bwd_workspace_bytes(int64_t rows, int D) { return (size_t)rms_bwd_blocks(rows) * (size_t)D * sizeof(float); }

int tadx_rmsnorm_bwd(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* rrms, const float* dres, float* dx,
                     uint16_t* dx16, int dx16_fmt, float* dgamma, int accumulate, void* ws, size_t ws_bytes, int64_t rows, int D,
                     tad_stream_t stream) {
  TAD_REQUIRE(dy && x && gamma && rrms && dx && dgamma && ws, "rmsnorm_bwd: null pointer");
  TAD_REQUIRE(rows > 0 && D > 0 && D % 4 == 0 && D <= 64 * 4 * RMS_MAX_V, "rmsnorm_bwd: D=%d must be a multiple of 4 and <= %d", D,
              64 * 4 * RMS_MAX_V);
  TAD_REQUIRE(dy_dtype == TAD_F32 || is_op16(dy_dtype), "rmsnorm_bwd: bad dy_dtype %d", dy_dtype);
  TAD_REQUIRE(!dx16 || is_op16(dx16_fmt), "rmsnorm_bwd: bad dx16_fmt %d", dx16_fmt);
  // float4 accesses to every f32 row operand, the partials in ws and (in the reduction) dgamma; 8-byte pieces of the 16-bit tensors;
  // rrms is read float by float
  TAD_REQUIRE_ALIGNED("rmsnorm_bwd", dy, dy_dtype == TAD_F32 ? 16 : 8);
  TAD_REQUIRE_ALIGNED("rmsnorm_bwd", x, 16);
  TAD_REQUIRE_ALIGNED("rmsnorm_bwd", gamma, 16);
  TAD_REQUIRE_ALIGNED("rmsnorm_bwd", dres, 16);
  TAD_REQUIRE_ALIGNED("rmsnorm_bwd", dx, 16);
  TAD_REQUIRE_ALIGNED("rmsnorm_bwd", dx16, 8);
  TAD_REQUIRE_ALIGNED("rmsnorm_bwd", dgamma, 16);
  TAD_REQUIRE_ALIGNED("rmsnorm_bwd", ws, 16);
  const int blocks = rms_bwd_blocks(rows);
  if (ws_bytes < (size_t)blocks * D * sizeof(float)) { set_error("rmsnorm_bwd: workspace too small"); return TAD_ENOSPACE; }
  const int rows_per_block = (int)((rows + blocks - 1) / blocks);
  const int nv = (D / 4 + 63) / 64;
  const size_t smem = (size_t)4 * D * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)ws;
  const bool full = (D == 256 * nv);
#define RMS_BWD_(NV, F, FULL_)                                                                                                    \
  hipLaunchKernelGGL((rmsnorm_bwd_kernel<NV, F, FULL_>), dim3(blocks), dim3(256), smem, st, dy, x, gamma, rrms, dres, dx, dx16, dx16_fmt, \
                     partial, rows, D, rows_per_block)
#define RMS_BWD_F(NV, F) \
  if (full) RMS_BWD_(NV, F, true); else RMS_BWD_(NV, F, false)
#define RMS_BWD(NV)                                     \
  if (dy_dtype == TAD_F32) { RMS_BWD_F(NV, TAD_F32); }  \
  else if (dy_dtype == TAD_F16) { RMS_BWD_F(NV, TAD_F16); } \
  else { RMS_BWD_F(NV, TAD_BF16); }
  RMS_SWITCH_NV(nv, RMS_BWD)
#undef RMS_BWD
#undef RMS_BWD_F
#undef RMS_BWD_
  int rc = check_launch("rmsnorm_bwd");
  if (rc) return rc;
  return launch_reduce_cols(partial, dgamma, nullptr, nullptr, 1, blocks, D, accumulate ? 1 : 0, st);
}

int tadx_qk_rmsnorm_fwd(const float* qkv32, const float* gq, const float* gk, uint16_t* qkv16, int fmt, float* rr, float q_out_scale,
                        int64_t M, int A, float eps, tad_stream_t stream) {
  TAD_REQUIRE(qkv32 && gq && gk && qkv16, "qk_rmsnorm_fwd: null pointer");
  TAD_REQUIRE(M > 0 && A > 0 && A % 4 == 0 && A <= 64 * 4 * RMS_MAX_V, "qk_rmsnorm_fwd: A=%d must be a multiple of 4 and <= %d", A,
              64 * 4 * RMS_MAX_V);
  TAD_REQUIRE(is_op16(fmt), "qk_rmsnorm_fwd: bad fmt %d", fmt);
  TAD_REQUIRE(q_out_scale > 0.f, "qk_rmsnorm_fwd: q_out_scale must be positive");
  // float4 loads of qkv32 (row stride 3A floats), gq and gk; 8-byte packed stores to qkv16; rr is written float by float
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_fwd", qkv32, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_fwd", gq, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_fwd", gk, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_fwd", qkv16, 8);
  const int nv = (A / 4 + 63) / 64;
  const dim3 grid((unsigned)((M + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define QK_FWD_(NV, F) hipLaunchKernelGGL((qk_rmsnorm_fwd_kernel<NV, F>), grid, block, 0, st, qkv32, gq, gk, qkv16, rr, q_out_scale, M, A, eps)
#define QK_FWD(NV) \
  if (fmt == TAD_F16) QK_FWD_(NV, TAD_F16); else QK_FWD_(NV, TAD_BF16);
  RMS_SWITCH_NV(nv, QK_FWD)
#undef QK_FWD
#undef QK_FWD_
  return check_launch("qk_rmsnorm_fwd");
}

size_t tadx_qk_rmsnorm_bwd_workspace_bytes(int64_t M, int A) { return (size_t)2 * rms_bwd_blocks(M) * (size_t)A * sizeof(float); }

int tadx_qk_rmsnorm_bwd(const uint16_t* dqkv16, int fmt, const float* qkv32, const float* gq, const float* gk, const float* rr,
                        float q_out_scale, uint16_t* dqkv_pre16, float* dgq, float* dgk, int accumulate, void* ws, size_t ws_bytes,
                        int64_t M, int A, tad_stream_t stream) {
  TAD_REQUIRE(dqkv16 && qkv32 && gq && gk && rr && dqkv_pre16 && dgq && dgk && ws, "qk_rmsnorm_bwd: null pointer");
  TAD_REQUIRE(M > 0 && A > 0 && A % 4 == 0 && A <= 64 * 4 * RMS_MAX_V, "qk_rmsnorm_bwd: A=%d must be a multiple of 4 and <= %d", A,
              64 * 4 * RMS_MAX_V);
  TAD_REQUIRE(is_op16(fmt), "qk_rmsnorm_bwd: bad fmt %d", fmt);
  // the factor itself does not enter the gradient (the header says why); it is checked so that a forward / backward pair agrees on it
  TAD_REQUIRE(q_out_scale > 0.f, "qk_rmsnorm_bwd: q_out_scale must be positive");
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_bwd", dqkv16, 8);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_bwd", qkv32, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_bwd", gq, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_bwd", gk, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_bwd", dqkv_pre16, 8);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_bwd", dgq, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_bwd", dgk, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_bwd", ws, 16);
  const int blocks = rms_bwd_blocks(M);
  if (ws_bytes < (size_t)2 * blocks * A * sizeof(float)) { set_error("qk_rmsnorm_bwd: workspace too small"); return TAD_ENOSPACE; }
  const int rows_per_block = (int)((M + blocks - 1) / blocks);
  const int nv = (A / 4 + 63) / 64;
  const size_t smem = (size_t)4 * 2 * A * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)ws;
#define QK_BWD_(NV, F)                                                                                                          \
  hipLaunchKernelGGL((qk_rmsnorm_bwd_kernel<NV, F>), dim3(blocks), dim3(256), smem, st, dqkv16, qkv32, gq, gk, rr, dqkv_pre16, partial, M, \
                     A, rows_per_block)
#define QK_BWD(NV) \
  if (fmt == TAD_F16) QK_BWD_(NV, TAD_F16); else QK_BWD_(NV, TAD_BF16);
  RMS_SWITCH_NV(nv, QK_BWD)
#undef QK_BWD
#undef QK_BWD_
  int rc = check_launch("qk_rmsnorm_bwd");
  if (rc) return rc;
  return launch_reduce_cols(partial, dgq, dgk, nullptr, 2, blocks, A, accumulate ? 1 : 0, st);
}

}  // extern "C"
