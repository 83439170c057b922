// RMSNorm forward / backward for rows of D f32 elements (D % 4 == 0, D <= 2048), and the RMS normalisation of the q and k thirds of a
// qkv row over their full H*d width (InternVideo2's qk_normalization): the extension ABI of include/tad_mi355x_ext.h (tadx_*).
// Same shape as layernorm.hip, and what the two share is one copy in rownorm.h: the instance per row width (ROWNORM_SWITCH_NV), the
// dealing of rows to backward blocks, the cross-wave combine into per-block column partials and the float4 / 16-bit helpers.
// Compiled ONCE: the 16-bit format of an operand is a run-time argument (TAD_BF16 / TAD_F16) that selects a template instance, so there
// are no _f16 twins.
#include "rownorm.h"
#include "../../include/tad_mi355x_ext.h"

TAD_NAMESPACE_BEGIN

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
// One float4 chunk of that gradient, on either side of the wave sum of s; both backward kernels are made of these two.  The first half
// takes one norm (rmsnorm_bwd_kernel) or two (q and k) and walks them stage by stage, the order in which the q / k kernel has always
// interleaved its two chains: the compiler's choice of which product of a sum it fuses follows the statement order, and with it the bits.
struct RmsChunk {
  float4& xh;       // out: x * r (may be x itself)
  float4& t;        // out: dy * g
  const float4& x;
  const float4& dy;
  const float4& g;
  float r;          // the row's rrms
  float& s;         // += t . xh
  float4& dg;       // += dy * xh
};
template <typename... C>
__device__ __forceinline__ void rms_grad_chunk(const C&... n) {
  ((n.xh = scale4(n.x, n.r)), ...);
  ((n.t = mul4(n.dy, n.g)), ...);
  ((n.s += dot4(n.t, n.xh)), ...);
  (acc4(n.dg, mul4(n.dy, n.xh)), ...);
}
__device__ __forceinline__ float rms_grad_dx(float t, float xh, float r, float c /* mean(t * xh) */) { return r * (t - xh * c); }

template <int NV, int DYFMT, bool FULL>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const void* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ gamma, const float* __restrict__ rrms,
                                                          const float* __restrict__ dres, float* __restrict__ dx,
                                                          uint16_t* __restrict__ dx16, int dx16_fmt, float* __restrict__ partial /*[grid][D]*/,
                                                          int64_t rows, int D, int rows_per_block) {
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
        rms_grad_chunk(RmsChunk{xh[i], t[i], xv[i], dyv[i], g[i], rr, s2, dg[i]});
      } else {
        xh[i] = t[i] = rv[i] = zero4();
      }
    }
    const float c2 = wave_sum_dpp(s2) / (float)D;
    float4 o[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      o[i].x = fmaf(rv[i].x, rmul, rms_grad_dx(t[i].x, xh[i].x, rr, c2));
      o[i].y = fmaf(rv[i].y, rmul, rms_grad_dx(t[i].y, xh[i].y, rr, c2));
      o[i].z = fmaf(rv[i].z, rmul, rms_grad_dx(t[i].z, xh[i].z, rr, c2));
      o[i].w = fmaf(rv[i].w, rmul, rms_grad_dx(t[i].w, xh[i].w, rr, c2));
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
  rownorm_combine<NV>(partial, D, 1, wave, dg);
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
        rms_grad_chunk(RmsChunk{q[i], tq[i], q[i], dq, g0[i], rq, sq, d0[i]}, RmsChunk{k[i], tk[i], k[i], dk, g1[i], rk, sk, d1[i]});  // q, k become xh
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
        const float4 oq = make_float4(rms_grad_dx(tq[i].x, q[i].x, rq, cq), rms_grad_dx(tq[i].y, q[i].y, rq, cq),
                                      rms_grad_dx(tq[i].z, q[i].z, rq, cq), rms_grad_dx(tq[i].w, q[i].w, rq, cq));
        const float4 ok = make_float4(rms_grad_dx(tk[i].x, k[i].x, rk, ck), rms_grad_dx(tk[i].y, k[i].y, rk, ck),
                                      rms_grad_dx(tk[i].z, k[i].z, rk, ck), rms_grad_dx(tk[i].w, k[i].w, rk, ck));
        stg_u2<false>(dst + c, pack16x4<FMT>(oq));
        stg_u2<false>(dst + A4 + c, pack16x4<FMT>(ok));
        stg_u2<false>(dst + 2 * A4 + c, pv[i]);
      }
    }
  }
  rownorm_combine<NV>(partial, A, 2, wave, d0, d1);
}

static inline bool is_op16(int fmt) { return fmt == TAD_BF16 || fmt == TAD_F16; }

TAD_NAMESPACE_END

using namespace tad;

extern "C" {

int tadx_abi_version(void) { return TADX_ABI_VERSION; }

int tadx_rmsnorm_fwd(const float* x, const float* gamma, void* y, int y_dtype, float* rrms, int64_t rows, int D, float eps,
                     tad_stream_t stream) {
  TAD_REQUIRE(x && gamma && y, "rmsnorm_fwd: null pointer");
  TAD_REQUIRE(rows > 0 && rownorm_width_ok(D), "rmsnorm_fwd: D=%d must be a multiple of 4 and <= %d", D, ROWNORM_MAX_D);
  TAD_REQUIRE(y_dtype == TAD_F32 || is_op16(y_dtype), "rmsnorm_fwd: bad y_dtype %d", y_dtype);
  // float4 loads of x and gamma; y: float4 stores (f32) or 8-byte packed stores (16-bit); rrms is written float by float
  TAD_REQUIRE_ALIGNED("rmsnorm_fwd", x, 16);
  TAD_REQUIRE_ALIGNED("rmsnorm_fwd", gamma, 16);
  TAD_REQUIRE_ALIGNED("rmsnorm_fwd", y, y_dtype == TAD_F32 ? 16 : 8);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define RMS_FWD_(NV, F) hipLaunchKernelGGL((rmsnorm_fwd_kernel<NV, F>), grid, block, 0, st, x, gamma, y, rrms, rows, D, eps)
#define RMS_FWD(NV)                                 \
  if (y_dtype == TAD_F32) RMS_FWD_(NV, TAD_F32);    \
  else if (y_dtype == TAD_F16) RMS_FWD_(NV, TAD_F16); \
  else RMS_FWD_(NV, TAD_BF16);
  ROWNORM_SWITCH_NV(rownorm_nv(D), RMS_FWD)
#undef RMS_FWD
#undef RMS_FWD_
  return check_launch("rmsnorm_fwd");
}

size_t tadx_rmsnorm_bwd_workspace_bytes(int64_t rows, int D) { return rownorm_bwd_plan(rows, D, 1).partial_floats * sizeof(float); }

int tadx_rmsnorm_bwd(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* rrms, const float* dres, float* dx,
                     uint16_t* dx16, int dx16_fmt, float* dgamma, int accumulate, void* ws, size_t ws_bytes, int64_t rows, int D,
                     tad_stream_t stream) {
  TAD_REQUIRE(dy && x && gamma && rrms && dx && dgamma && ws, "rmsnorm_bwd: null pointer");
  TAD_REQUIRE(rows > 0 && rownorm_width_ok(D), "rmsnorm_bwd: D=%d must be a multiple of 4 and <= %d", D, ROWNORM_MAX_D);
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
  const RowNormBwd p = rownorm_bwd_plan(rows, D, 1);
  if (ws_bytes < p.partial_floats * sizeof(float)) { set_error("rmsnorm_bwd: workspace too small"); return TAD_ENOSPACE; }
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)ws;
#define RMS_BWD_(NV, F, FULL_)                                                                                                      \
  hipLaunchKernelGGL((rmsnorm_bwd_kernel<NV, F, FULL_>), dim3(p.blocks), dim3(256), p.smem_bytes, st, dy, x, gamma, rrms, dres, dx, dx16, \
                     dx16_fmt, partial, rows, D, p.rows_per_block)
#define RMS_BWD_F(NV, F) \
  if (D == 256 * NV) RMS_BWD_(NV, F, true); else RMS_BWD_(NV, F, false)
#define RMS_BWD(NV)                                     \
  if (dy_dtype == TAD_F32) { RMS_BWD_F(NV, TAD_F32); }  \
  else if (dy_dtype == TAD_F16) { RMS_BWD_F(NV, TAD_F16); } \
  else { RMS_BWD_F(NV, TAD_BF16); }
  ROWNORM_SWITCH_NV(rownorm_nv(D), RMS_BWD)
#undef RMS_BWD
#undef RMS_BWD_F
#undef RMS_BWD_
  int rc = check_launch("rmsnorm_bwd");
  if (rc) return rc;
  return launch_reduce_cols(partial, dgamma, nullptr, nullptr, 1, p.blocks, D, accumulate ? 1 : 0, st);
}

int tadx_qk_rmsnorm_fwd(const float* qkv32, const float* gq, const float* gk, uint16_t* qkv16, int fmt, float* rr, float q_out_scale,
                        int64_t M, int A, float eps, tad_stream_t stream) {
  TAD_REQUIRE(qkv32 && gq && gk && qkv16, "qk_rmsnorm_fwd: null pointer");
  TAD_REQUIRE(M > 0 && rownorm_width_ok(A), "qk_rmsnorm_fwd: A=%d must be a multiple of 4 and <= %d", A, ROWNORM_MAX_D);
  TAD_REQUIRE(is_op16(fmt), "qk_rmsnorm_fwd: bad fmt %d", fmt);
  TAD_REQUIRE(q_out_scale > 0.f, "qk_rmsnorm_fwd: q_out_scale must be positive");
  // float4 loads of qkv32 (row stride 3A floats), gq and gk; 8-byte packed stores to qkv16; rr is written float by float
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_fwd", qkv32, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_fwd", gq, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_fwd", gk, 16);
  TAD_REQUIRE_ALIGNED("qk_rmsnorm_fwd", qkv16, 8);
  const dim3 grid((unsigned)((M + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define QK_FWD_(NV, F) hipLaunchKernelGGL((qk_rmsnorm_fwd_kernel<NV, F>), grid, block, 0, st, qkv32, gq, gk, qkv16, rr, q_out_scale, M, A, eps)
#define QK_FWD(NV) \
  if (fmt == TAD_F16) QK_FWD_(NV, TAD_F16); else QK_FWD_(NV, TAD_BF16);
  ROWNORM_SWITCH_NV(rownorm_nv(A), QK_FWD)
#undef QK_FWD
#undef QK_FWD_
  return check_launch("qk_rmsnorm_fwd");
}

size_t tadx_qk_rmsnorm_bwd_workspace_bytes(int64_t M, int A) { return rownorm_bwd_plan(M, A, 2).partial_floats * sizeof(float); }

int tadx_qk_rmsnorm_bwd(const uint16_t* dqkv16, int fmt, const float* qkv32, const float* gq, const float* gk, const float* rr,
                        float q_out_scale, uint16_t* dqkv_pre16, float* dgq, float* dgk, int accumulate, void* ws, size_t ws_bytes,
                        int64_t M, int A, tad_stream_t stream) {
  TAD_REQUIRE(dqkv16 && qkv32 && gq && gk && rr && dqkv_pre16 && dgq && dgk && ws, "qk_rmsnorm_bwd: null pointer");
  TAD_REQUIRE(M > 0 && rownorm_width_ok(A), "qk_rmsnorm_bwd: A=%d must be a multiple of 4 and <= %d", A, ROWNORM_MAX_D);
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
  const RowNormBwd p = rownorm_bwd_plan(M, A, 2);
  if (ws_bytes < p.partial_floats * sizeof(float)) { set_error("qk_rmsnorm_bwd: workspace too small"); return TAD_ENOSPACE; }
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)ws;
#define QK_BWD_(NV, F)                                                                                                               \
  hipLaunchKernelGGL((qk_rmsnorm_bwd_kernel<NV, F>), dim3(p.blocks), dim3(256), p.smem_bytes, st, dqkv16, qkv32, gq, gk, rr, dqkv_pre16, \
                     partial, M, A, p.rows_per_block)
#define QK_BWD(NV) \
  if (fmt == TAD_F16) QK_BWD_(NV, TAD_F16); else QK_BWD_(NV, TAD_BF16);
  ROWNORM_SWITCH_NV(rownorm_nv(A), QK_BWD)
#undef QK_BWD
#undef QK_BWD_
  int rc = check_launch("qk_rmsnorm_bwd");
  if (rc) return rc;
  return launch_reduce_cols(partial, dgq, dgk, nullptr, 2, p.blocks, A, accumulate ? 1 : 0, st);
}

}  // extern "C"
