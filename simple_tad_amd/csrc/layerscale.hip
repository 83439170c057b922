// Layer-scale (gamma_1 / gamma_2) and proj / MLP dropout of the fused Block variants (ops.BlockVariantFn).
//
// A branch y = res + s[b] gamma[c] keep[m,c] / (1 - p) u, u = a W^T + bias.  With gb = op16(s keep / (1 - p) g) -- no gamma in it -- the
// backward needs no pass over an [M, D] tensor for gamma:
//   d a    = gb (diag(gamma) W)            tad_rowscale_transpose_cast writes that operand,
//   T      = gb^T a, cs = colsum(gb)       one tad_linear_bwd_weight,
//   dW     = gamma[n] T[n,:],  dbias = gamma cs,  dgamma[n] = sum_k T[n,k] W[n,k] + bias[n] cs[n]     tad_layerscale_grads.
// The mask is the counter-based one of attention dropout (common.h: Drop / drop_keep) with row = m, key = c.
#include "common.h"

TAD_NAMESPACE_BEGIN

// ---------------------------------------------------------------- out [C,R] = op16(gamma[r] * src[r,c]): transpose_cast_kernel's tiling
__global__ void rowscale_transpose_cast_kernel(const float* __restrict__ src, const float* __restrict__ gamma, uint16_t* __restrict__ dst,
                                               int R, int C) {
  __shared__ float tile[64][65];
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 256 threads: 4 rows per pass
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < R && c < C) ? gamma[r] * src[(int64_t)r * C + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, r = r0 + tx;
    if (c < C && r < R) dst[(int64_t)c * R + r] = f32_to_op16(tile[tx][i]);
  }
}

// ---------------------------------------------------------------- y = op16(rowscale * keep / (1 - p) * g)
// The factor of a row is ONE f32 value, f = rowscale[m / rows_per_scale] * inv_keep; a kept element is op16(g * f), a dropped one and
// every element of a row whose rowscale is 0 is +0 (a select: a non-finite g does not leak).
// The product g * f is an f32 value of its own before it is rounded to 16 bits (the contract: op16(fl32(g f)), what torch's cast of the f32
// product gives).  Under -ffp-contract=fast the half pass folds product and conversion into one v_fma_mixlo_f16 otherwise, whose bits
// differed from that; the empty asm pins the product in a register.
__device__ __forceinline__ float own_f32(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
template <bool VEC>
__global__ void branch_dropout_cast_kernel(const float* __restrict__ g, uint16_t* __restrict__ y, const float* __restrict__ rowscale,
                                           int rows_per_scale, Drop drop, int64_t M, int D) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    const int D4 = D >> 2;
    const int64_t total = M * D4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int64_t m = i / D4;
      const uint32_t c = (uint32_t)(i - m * D4) * 4u;
      const float s = rowscale ? rowscale[m / rows_per_scale] : 1.f;
      const float f = s * drop.inv_keep;
      const float4 v = reinterpret_cast<const float4*>(g)[i];
      const bool live = s != 0.f;
      const float a = (live && drop_keep(drop, (uint32_t)m, c)) ? own_f32(v.x * f) : 0.f;
      const float b = (live && drop_keep(drop, (uint32_t)m, c + 1)) ? own_f32(v.y * f) : 0.f;
      const float cc = (live && drop_keep(drop, (uint32_t)m, c + 2)) ? own_f32(v.z * f) : 0.f;
      const float d = (live && drop_keep(drop, (uint32_t)m, c + 3)) ? own_f32(v.w * f) : 0.f;
      uint2 o;
      o.x = pack_op16x2(a, b);
      o.y = pack_op16x2(cc, d);
      reinterpret_cast<uint2*>(y)[i] = o;
    }
  } else {
    const int64_t total = M * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int64_t m = i / D;
      const uint32_t c = (uint32_t)(i - m * D);
      const float s = rowscale ? rowscale[m / rows_per_scale] : 1.f;
      const float f = s * drop.inv_keep;
      y[i] = f32_to_op16((s != 0.f && drop_keep(drop, (uint32_t)m, c)) ? own_f32(g[i] * f) : 0.f);
    }
  }
}

#ifndef TAD_OPND_F16  // f32 in, f32 out: nothing below depends on the operand format (compiled in the bfloat16 pass only)
// ---------------------------------------------------------------- out = res + rowscale * gamma * keep / (1 - p) * u
// The factor of an element is f[c] = gamma[c] * (rowscale * inv_keep) (two f32 products); a dropped element and every element of a row whose
// rowscale is 0 is res itself, bit for bit.
template <bool VEC>
__global__ void branch_dropout_fwd_kernel(const float* __restrict__ u, const float* __restrict__ res, float* __restrict__ out,
                                          const float* __restrict__ gamma, const float* __restrict__ rowscale, int rows_per_scale, Drop drop,
                                          int64_t M, int D) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    const int D4 = D >> 2;
    const int64_t total = M * D4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int64_t m = i / D4;
      const int c4 = (int)(i - m * D4);
      const uint32_t c = (uint32_t)c4 * 4u;
      const float s = rowscale ? rowscale[m / rows_per_scale] : 1.f;
      const float f = s * drop.inv_keep;
      float4 r = reinterpret_cast<const float4*>(res)[i];
      if (s != 0.f) {
        const float4 v = reinterpret_cast<const float4*>(u)[i];
        float4 gm = make_float4(1.f, 1.f, 1.f, 1.f);
        if (gamma) gm = reinterpret_cast<const float4*>(gamma)[c4];
        if (drop_keep(drop, (uint32_t)m, c)) r.x += v.x * (gamma ? gm.x * f : f);
        if (drop_keep(drop, (uint32_t)m, c + 1)) r.y += v.y * (gamma ? gm.y * f : f);
        if (drop_keep(drop, (uint32_t)m, c + 2)) r.z += v.z * (gamma ? gm.z * f : f);
        if (drop_keep(drop, (uint32_t)m, c + 3)) r.w += v.w * (gamma ? gm.w * f : f);
      }
      reinterpret_cast<float4*>(out)[i] = r;
    }
  } else {
    const int64_t total = M * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int64_t m = i / D;
      const int c = (int)(i - m * D);
      const float s = rowscale ? rowscale[m / rows_per_scale] : 1.f;
      const float f = s * drop.inv_keep;
      float r = res[i];
      if (s != 0.f && drop_keep(drop, (uint32_t)m, (uint32_t)c)) r += u[i] * (gamma ? gamma[c] * f : f);
      out[i] = r;
    }
  }
}

// ---------------------------------------------------------------- dW = gamma[n] T[n,:], dbias = gamma cs, dgamma[n] = <T[n,:], W[n,:]> + bias[n] cs[n]
// One workgroup of 256 lanes per row n.  Lane t adds its products in ascending k (k = t, t + 256, ... or, vectorised, the four lanes of its
// 16-byte pieces); the 256 partial sums meet in a fixed tree (wave_sum inside each wave, then wave 0 .. 3 in order): no atomics, the same bits
// every run.
constexpr int LSG_BLOCK = 256;
// four consecutive floats as one 16-byte access (VEC: p is 16-byte aligned) or one float at a time
template <bool VEC>
__device__ __forceinline__ void lsg_load4(const float* p, float (&v)[4]) {
  if constexpr (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = p[e];
  }
}
template <bool VEC>
__device__ __forceinline__ void lsg_store4(float* p, const float (&v)[4]) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = v[e];
  }
}
template <bool VEC>
__global__ __launch_bounds__(LSG_BLOCK) void layerscale_grads_kernel(const float* __restrict__ T, const float* __restrict__ W,
                                                                     const float* __restrict__ bias, const float* __restrict__ cs,
                                                                     const float* __restrict__ gamma, float* __restrict__ dW,
                                                                     float* __restrict__ dbias, float* __restrict__ dgamma, int K,
                                                                     int accumulate) {
  __shared__ float part[LSG_BLOCK / WAVE];
  const int n = blockIdx.x;
  const float gm = gamma[n];
  const int64_t base = (int64_t)n * K;
  float acc = 0.f;
  if (VEC || (K & 3) == 0) {
    // Lane t owns the four-element pieces t, t + 256, ... of the row and keeps one partial sum per position inside a piece.  ONE loop body
    // for both access widths (lsg_load4 / lsg_store4: a float4, or four floats when T, W or dW is not on 16 bytes), so that dgamma has the
    // same bits wherever the tensors lie.
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = threadIdx.x; k < (K >> 2); k += LSG_BLOCK) {
      const int64_t at = base + 4 * (int64_t)k;
      float t[4], w[4], o[4];
      lsg_load4<VEC>(T + at, t);
      lsg_load4<VEC>(W + at, w);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = gm * t[e];
      if (accumulate) {
        float p[4];
        lsg_load4<VEC>(dW + at, p);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += p[e];
      }
      lsg_store4<VEC>(dW + at, o);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += t[e] * w[e];
    }
    acc = (a[0] + a[1]) + (a[2] + a[3]);
  } else {
    for (int k = threadIdx.x; k < K; k += LSG_BLOCK) {
      const float t = T[base + k];
      float o = gm * t;
      if (accumulate) o += dW[base + k];
      dW[base + k] = o;
      acc += t * W[base + k];
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float dg = part[0];
#pragma unroll
    for (int w = 1; w < LSG_BLOCK / WAVE; ++w) dg += part[w];
    const float c = cs ? cs[n] : 0.f;
    if (bias) dg += bias[n] * c;
    dgamma[n] = accumulate ? dgamma[n] + dg : dg;
    if (dbias) {
      const float db = gm * c;
      dbias[n] = accumulate ? dbias[n] + db : db;
    }
  }
}
#endif  // !TAD_OPND_F16

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

TAD_NAMESPACE_END

using namespace tad;

extern "C" {

int tad_rowscale_transpose_cast(const float* w, const float* gamma, uint16_t* out, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(w && gamma && out && N > 0 && K > 0, "rowscale_transpose_cast: bad args");
  hipLaunchKernelGGL(rowscale_transpose_cast_kernel, dim3((K + 63) / 64, (N + 63) / 64), dim3(256), 0, (hipStream_t)stream, w, gamma, out, N,
                     K);
  return check_launch("rowscale_transpose_cast");
}

int tad_branch_dropout_cast(const float* g, uint16_t* y, const float* rowscale, int rows_per_scale, float p, uint32_t seed, int64_t M, int D,
                            tad_stream_t stream) {
  TAD_REQUIRE(g && y && M > 0 && D > 0 && M <= 0xffffffffLL, "branch_dropout_cast: bad args");
  TAD_REQUIRE(!rowscale || rows_per_scale > 0, "branch_dropout_cast: rows_per_scale must be > 0");
  Drop drop;
  TAD_REQUIRE(make_drop(p, seed, &drop), "branch_dropout_cast: p must be in [0, 1)");
  const bool vec = D % 4 == 0 && aligned16(g) && (reinterpret_cast<uintptr_t>(y) & 7u) == 0;
  if (vec)
    hipLaunchKernelGGL(branch_dropout_cast_kernel<true>, dim3(capped_grid(M * (D / 4), 256)), dim3(256), 0, (hipStream_t)stream, g, y,
                       rowscale, rows_per_scale, drop, M, D);
  else
    hipLaunchKernelGGL(branch_dropout_cast_kernel<false>, dim3(capped_grid(M * D, 256)), dim3(256), 0, (hipStream_t)stream, g, y, rowscale,
                       rows_per_scale, drop, M, D);
  return check_launch("branch_dropout_cast");
}

#ifndef TAD_OPND_F16
int tad_branch_dropout_fwd(const float* u, const float* res, float* out, const float* gamma, const float* rowscale, int rows_per_scale,
                           float p, uint32_t seed, int64_t M, int D, tad_stream_t stream) {
  TAD_REQUIRE(u && res && out && M > 0 && D > 0 && M <= 0xffffffffLL, "branch_dropout_fwd: bad args");
  TAD_REQUIRE(!rowscale || rows_per_scale > 0, "branch_dropout_fwd: rows_per_scale must be > 0");
  Drop drop;
  TAD_REQUIRE(make_drop(p, seed, &drop), "branch_dropout_fwd: p must be in [0, 1)");
  const bool vec = D % 4 == 0 && aligned16(u) && aligned16(res) && aligned16(out) && (!gamma || aligned16(gamma));
  if (vec)
    hipLaunchKernelGGL(branch_dropout_fwd_kernel<true>, dim3(capped_grid(M * (D / 4), 256)), dim3(256), 0, (hipStream_t)stream, u, res, out,
                       gamma, rowscale, rows_per_scale, drop, M, D);
  else
    hipLaunchKernelGGL(branch_dropout_fwd_kernel<false>, dim3(capped_grid(M * D, 256)), dim3(256), 0, (hipStream_t)stream, u, res, out, gamma,
                       rowscale, rows_per_scale, drop, M, D);
  return check_launch("branch_dropout_fwd");
}

int tad_layerscale_grads(const float* T, const float* W, const float* bias, const float* cs, const float* gamma, float* dW, float* dbias,
                         float* dgamma, int accumulate, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(T && W && gamma && dW && dgamma && N > 0 && K > 0, "layerscale_grads: bad args");
  TAD_REQUIRE((!bias && !dbias) || cs, "layerscale_grads: bias / dbias need the column sums cs");
  const bool vec = K % 4 == 0 && aligned16(T) && aligned16(W) && aligned16(dW);
  if (vec)
    hipLaunchKernelGGL(layerscale_grads_kernel<true>, dim3(N), dim3(LSG_BLOCK), 0, (hipStream_t)stream, T, W, bias, cs, gamma, dW, dbias, dgamma,
                       K, accumulate);
  else
    hipLaunchKernelGGL(layerscale_grads_kernel<false>, dim3(N), dim3(LSG_BLOCK), 0, (hipStream_t)stream, T, W, bias, cs, gamma, dW, dbias,
                       dgamma, K, accumulate);
  return check_launch("layerscale_grads");
}
#endif  // !TAD_OPND_F16

}  // extern "C"
