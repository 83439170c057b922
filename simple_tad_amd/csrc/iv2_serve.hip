// Serving the InternVideo2 family: the serving ABI of include/tad_mi355x_serve.h (tads_*), the ONE source of libtad_mi355x_serve.so.
//   class_token_entry   `cat((cls_token.expand(B,-1,-1), x), 1) + pos_embed` in one pass, and on the way back the patch rows' gradient
//                       and the table's / the class token's gradient (a sum over the clips in the order b = 0, 1, ...) in one launch
//                       without atomics: row movers of the shape of visible_tokens.hip, one float4 per thread and step.
//   residual_rmsnorm    x_out = x + y * ls_gamma and the RMSNorm of x_out as the next Linear's 16-bit operand, one pass: the shape and the
//                       order of operations of rmsnorm_fwd_kernel (rmsnorm.hip) -- one wave per row, the row held in registers as NV float4
//                       per lane and read once, four rows per block, the instance chosen by ROWNORM_SWITCH_NV over rownorm_nv(D).  The
//                       loads of a row (x, y and the two gammas) are requested in one batch before any arithmetic (layernorm.hip's notes
//                       on load batching).  Evaluation only: no statistics are kept.
// The library is self-contained (side_library.h) and exports the tads_* entry points alone.  Compiled ONCE: the 16-bit format is a
// run-time argument that selects a template instance.
#include "side_library.h"
#include "rownorm.h"
#pragma GCC visibility push(default)
#include "../../include/tad_mi355x_serve.h"
#pragma GCC visibility pop

TAD_NAMESPACE_BEGIN

__device__ __forceinline__ float4 cte_add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// One thread per float4 of the output: item = r * D4 + c, r = b * (N + 1) + t.  Only adds: nothing here can be contracted.
__global__ __launch_bounds__(256) void class_token_entry_fwd_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                                    const float* __restrict__ pos, float* __restrict__ out, int64_t items,
                                                                    int N, int D4) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int64_t r = it / D4;
    const int c = (int)(it - r * D4);
    const int64_t b = r / (N + 1);
    const int t = (int)(r - b * (N + 1));
    const float4* src = t == 0 ? reinterpret_cast<const float4*>(cls) + c : reinterpret_cast<const float4*>(patch) + (b * N + (t - 1)) * D4 + c;
    const float4 u = ldg_f4<false>(src);
    const float4 v = ldg_f4<false>(reinterpret_cast<const float4*>(pos) + (int64_t)t * D4 + c);
    stg_f4<false>(reinterpret_cast<float4*>(out) + it, cte_add4(u, v));
  }
}

// One thread per float4 column group of one token: item = t * D4 + c.  It walks the clips in order.  DPATCH: the patch rows' gradient is
// written; DSUM: dpos and / or dcls exist (which of the two: a uniform test of the pointers).
template <bool DPATCH, bool DSUM>
__global__ __launch_bounds__(256) void class_token_entry_bwd_kernel(const float* __restrict__ g, float* __restrict__ dpatch,
                                                                    float* __restrict__ dpos, float* __restrict__ dcls, int accumulate,
                                                                    int64_t items, int B, int N, int D4) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int64_t t = it / D4;
    const int c = (int)(it - t * D4);
    if (!DSUM && t == 0) continue;                   // the class token's row is wanted by the sums alone
    if (DSUM && !DPATCH && !dpos && t != 0) continue;  // dcls alone: the first row is all there is to sum
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int b = 0; b < B; ++b) {
      const float4 v = ldg_f4<false>(reinterpret_cast<const float4*>(g) + ((int64_t)b * (N + 1) + t) * D4 + c);
      if constexpr (DPATCH) {
        if (t != 0) stg_f4<false>(reinterpret_cast<float4*>(dpatch) + ((int64_t)b * N + (t - 1)) * D4 + c, v);
      }
      if constexpr (DSUM) acc = b == 0 ? v : cte_add4(acc, v);
    }
    if constexpr (DSUM) {
      if (dpos) {
        float4* d = reinterpret_cast<float4*>(dpos) + it;
        stg_f4<false>(d, accumulate ? cte_add4(ldg_f4<false>(d), acc) : acc);
      }
      if (dcls && t == 0) {
        float4* d = reinterpret_cast<float4*>(dcls) + c;
        stg_f4<false>(d, accumulate ? cte_add4(ldg_f4<false>(d), acc) : acc);
      }
    }
  }
}

// x + y * g with the product and the sum each rounded on their own, whatever the contraction flag says: torch's `x + y * gamma`.
// __fmul_rn / __fadd_rn state the intent, but in this toolchain they are the plain operators (the OCML rounded forms are behind a macro),
// and under -ffp-contract=fast the code generator fused the pair into v_pk_fma_f32 all the same (seen in the ISA; D = 260 then differed
// from torch in the last bit).  So the product passes through an empty asm statement that names its register: no instruction, but nothing
// can be contracted across it.
__device__ __forceinline__ float mul_rounded(float a, float b) {
  float p = __fmul_rn(a, b);
  asm volatile("" : "+v"(p));
  return p;
}
__device__ __forceinline__ float4 res_scaled4(const float4& x, const float4& y, const float4& g) {
  return make_float4(__fadd_rn(x.x, mul_rounded(y.x, g.x)), __fadd_rn(x.y, mul_rounded(y.y, g.y)), __fadd_rn(x.z, mul_rounded(y.z, g.z)),
                     __fadd_rn(x.w, mul_rounded(y.w, g.w)));
}
__device__ __forceinline__ float4 res_plain4(const float4& x, const float4& y) {
  return make_float4(__fadd_rn(x.x, y.x), __fadd_rn(x.y, y.y), __fadd_rn(x.z, y.z), __fadd_rn(x.w, y.w));
}

// XFMT: TAD_BF16 / TAD_F16, or TAD_F32 for "no norm behind it" (xn and norm_gamma absent).  LS: ls_gamma exists.  Four rows per block,
// one per wave.  x and x_out may be one buffer (no __restrict__ on either): a lane reads its own elements before it writes them and
// no other lane touches them.
template <int NV, int XFMT, bool LS>
__global__ __launch_bounds__(256) void residual_rmsnorm_fwd_kernel(const float* x, const float* __restrict__ y,
                                                                   const float* __restrict__ ls_gamma, const float* __restrict__ norm_gamma,
                                                                   float* x_out, uint16_t* __restrict__ xn, int64_t rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int D4 = D >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x + row * D);
  const float4* yr = reinterpret_cast<const float4*>(y + row * D);
  float4 v[NV], u[NV], ls[NV], ng[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) {
      v[i] = ldg_f4<false>(xr + c);
      u[i] = ldg_f4<false>(yr + c);
      if constexpr (LS) ls[i] = reinterpret_cast<const float4*>(ls_gamma)[c];
      if constexpr (XFMT != TAD_F32) ng[i] = reinterpret_cast<const float4*>(norm_gamma)[c];
    } else {
      v[i] = u[i] = ls[i] = ng[i] = zero4();
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // the whole batch of loads stays above the arithmetic
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if constexpr (LS) v[i] = res_scaled4(v[i], u[i], ls[i]);
    else v[i] = res_plain4(v[i], u[i]);
    if (c < D4) stg_f4<false>(reinterpret_cast<float4*>(x_out + row * D) + c, v[i]);
    if constexpr (XFMT != TAD_F32) s += sumsq4(v[i]);
  }
  if constexpr (XFMT != TAD_F32) {
    const float rr = rsqrtf(wave_sum(s) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < D4) stg_u2<false>(reinterpret_cast<uint2*>(xn + row * D) + c, pack16x4<XFMT>(mul4(scale4(v[i], rr), ng[i])));
    }
  }
}

TAD_NAMESPACE_END

using namespace tad;

#pragma GCC visibility push(default)
extern "C" {

int tads_abi_version(void) { return TADS_ABI_VERSION; }

const char* tads_last_error_string(void) { return tad::side_last_error(); }

int tads_class_token_entry_fwd(const float* patch, const float* cls, const float* pos, float* out, int B, int N, int D,
                               tad_stream_t stream) {
  TAD_REQUIRE(patch && cls && pos && out, "class_token_entry_fwd: null pointer");
  TAD_REQUIRE(B > 0 && N > 0 && D > 0, "class_token_entry_fwd: B=%d, N=%d, D=%d must all be positive", B, N, D);
  TAD_REQUIRE(D % 4 == 0, "class_token_entry_fwd: D=%d must be a multiple of 4", D);
  // float4 loads of patch, cls and pos, float4 stores to out
  TAD_REQUIRE_ALIGNED("class_token_entry_fwd", patch, 16);
  TAD_REQUIRE_ALIGNED("class_token_entry_fwd", cls, 16);
  TAD_REQUIRE_ALIGNED("class_token_entry_fwd", pos, 16);
  TAD_REQUIRE_ALIGNED("class_token_entry_fwd", out, 16);
  const int64_t items = (int64_t)B * (N + 1) * (D / 4);
  hipLaunchKernelGGL(class_token_entry_fwd_kernel, dim3(capped_grid(items, 256)), dim3(256), 0, (hipStream_t)stream, patch, cls, pos, out,
                     items, N, D / 4);
  return check_launch("class_token_entry_fwd");
}

int tads_class_token_entry_bwd(const float* g, float* dpatch, float* dpos, float* dcls, int accumulate, int B, int N, int D,
                               tad_stream_t stream) {
  TAD_REQUIRE(g, "class_token_entry_bwd: null pointer");
  TAD_REQUIRE(dpatch || dpos || dcls, "class_token_entry_bwd: dpatch, dpos and dcls are all null: nothing to compute");
  TAD_REQUIRE(B > 0 && N > 0 && D > 0, "class_token_entry_bwd: B=%d, N=%d, D=%d must all be positive", B, N, D);
  TAD_REQUIRE(D % 4 == 0, "class_token_entry_bwd: D=%d must be a multiple of 4", D);
  // float4 loads of g, float4 stores to dpatch, float4 loads (accumulate) and stores of dpos and dcls
  TAD_REQUIRE_ALIGNED("class_token_entry_bwd", g, 16);
  TAD_REQUIRE_ALIGNED("class_token_entry_bwd", dpatch, 16);
  TAD_REQUIRE_ALIGNED("class_token_entry_bwd", dpos, 16);
  TAD_REQUIRE_ALIGNED("class_token_entry_bwd", dcls, 16);
  const int64_t items = (int64_t)(N + 1) * (D / 4);
  const dim3 grid(capped_grid(items, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define CTE_BWD(DP_, DS_) \
  hipLaunchKernelGGL((class_token_entry_bwd_kernel<DP_, DS_>), grid, block, 0, st, g, dpatch, dpos, dcls, accumulate ? 1 : 0, items, B, N, D / 4)
  const bool sums = dpos || dcls;
  if (dpatch && sums) CTE_BWD(true, true);
  else if (dpatch) CTE_BWD(true, false);
  else CTE_BWD(false, true);
#undef CTE_BWD
  return check_launch("class_token_entry_bwd");
}

int tads_residual_rmsnorm_fwd(const float* x, const float* y, const float* ls_gamma, const float* norm_gamma, float* x_out, void* xn,
                              int xn_fmt, int64_t rows, int D, float eps, tad_stream_t stream) {
  TAD_REQUIRE(x && y && x_out, "residual_rmsnorm_fwd: null pointer");
  TAD_REQUIRE(rows > 0, "residual_rmsnorm_fwd: rows=%lld must be positive", (long long)rows);
  TAD_REQUIRE(rownorm_width_ok(D), "residual_rmsnorm_fwd: D=%d must be a multiple of 4 and <= %d", D, ROWNORM_MAX_D);
  TAD_REQUIRE(!norm_gamma || xn, "residual_rmsnorm_fwd: norm_gamma without xn: the norm has nowhere to go");
  TAD_REQUIRE(!xn || norm_gamma, "residual_rmsnorm_fwd: xn without norm_gamma: there is no norm to write");
  TAD_REQUIRE(!xn || xn_fmt == TAD_BF16 || xn_fmt == TAD_F16, "residual_rmsnorm_fwd: bad xn_fmt %d", xn_fmt);
  TAD_REQUIRE((const void*)x_out != (const void*)y, "residual_rmsnorm_fwd: x_out may be x, it may not be y");
  // float4 loads of x, y and the two gammas, float4 stores to x_out, 8-byte packed stores to xn
  TAD_REQUIRE_ALIGNED("residual_rmsnorm_fwd", x, 16);
  TAD_REQUIRE_ALIGNED("residual_rmsnorm_fwd", y, 16);
  TAD_REQUIRE_ALIGNED("residual_rmsnorm_fwd", ls_gamma, 16);
  TAD_REQUIRE_ALIGNED("residual_rmsnorm_fwd", norm_gamma, 16);
  TAD_REQUIRE_ALIGNED("residual_rmsnorm_fwd", x_out, 16);
  TAD_REQUIRE_ALIGNED("residual_rmsnorm_fwd", xn, 8);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int fmt = xn ? xn_fmt : TAD_F32;
#define RR_FWD_(NV, F, LS_) \
  hipLaunchKernelGGL((residual_rmsnorm_fwd_kernel<NV, F, LS_>), grid, block, 0, st, x, y, ls_gamma, norm_gamma, x_out, (uint16_t*)xn, rows, D, eps)
#define RR_FWD_F(NV, F) \
  if (ls_gamma) RR_FWD_(NV, F, true); else RR_FWD_(NV, F, false)
#define RR_FWD(NV)                                  \
  if (fmt == TAD_F32) { RR_FWD_F(NV, TAD_F32); }    \
  else if (fmt == TAD_F16) { RR_FWD_F(NV, TAD_F16); } \
  else { RR_FWD_F(NV, TAD_BF16); }
  ROWNORM_SWITCH_NV(rownorm_nv(D), RR_FWD)
#undef RR_FWD
#undef RR_FWD_F
#undef RR_FWD_
  return check_launch("residual_rmsnorm_fwd");
}

}  // extern "C"
#pragma GCC visibility pop
