// LayerNorm forward / backward for rows of D f32 elements (D % 4 == 0, D <= 2048).
// HBM-bound: one wave per row, the row lives in registers (float4 per lane per 256 columns),
// two-pass mean / variance in registers (same numerics as torch: biased variance around the mean),
// wave reductions by cross-lane shuffles -- no LDS on the forward path.  What this shape shares with rmsnorm.hip (the instance per row
// width, the dealing of rows to backward blocks, the cross-wave combine, the float4 / 16-bit helpers) is rownorm.h.
#include "rownorm.h"

TAD_NAMESPACE_BEGIN

template <int NV, bool OUT_BF16>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, void* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd,
                                                            int64_t rows, int D, float eps) {
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
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float mu = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) {
      const float a = v[i].x - mu, b = v[i].y - mu, cc = v[i].z - mu, d = v[i].w - mu;
      q += (a * a + b * b) + (cc * cc + d * d);
    }
  }
  const float rs = rsqrtf(wave_sum(q) / (float)D + eps);
  if (lane == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) {
      const float4 g = reinterpret_cast<const float4*>(gamma)[c];
      const float4 b = reinterpret_cast<const float4*>(beta)[c];
      float4 o;
      o.x = (v[i].x - mu) * rs * g.x + b.x;
      o.y = (v[i].y - mu) * rs * g.y + b.y;
      o.z = (v[i].z - mu) * rs * g.z + b.z;
      o.w = (v[i].w - mu) * rs * g.w + b.w;
      if (OUT_BF16) {
        const uint2 p = pack16x4<TAD_OP16>(o);
        stg_u2<false>(reinterpret_cast<uint2*>((uint16_t*)y + row * D) + c, p);
      } else {
        stg_f4<false>(reinterpret_cast<float4*>((float*)y + row * D) + c, o);
      }
    }
  }
}

// Backward.  Each block owns a contiguous chunk of rows; each wave walks rows of the chunk with stride 4 and keeps
// per-lane column partials of dgamma, dbeta and (optionally) colsum(dx) in registers; they are combined across the
// block's 4 waves in LDS and written as one partial row per block and quantity (rownorm_combine) -> reduced by launch_reduce_cols.
// FULL: D == 256 * NV (768, 1024, 1280, 512 ...): no per-lane column guard, so the row loop is one basic block up to the optional bf16
// store (the guards split every chunk into its own exec-masked region with its own waits).
__device__ const float ln_one = 1.0f;
template <int NV, bool DY_BF16, bool FULL>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const void* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ gamma, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const float* __restrict__ dres,
                                                            float* __restrict__ dx, uint16_t* __restrict__ dxb,
                                                            float* __restrict__ partial /*[grid][3][D]*/, int64_t rows, int D,
                                                            int rows_per_block, int want_colsum,
                                                            const float* __restrict__ rowscale, int rows_per_scale) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int D4 = D >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(rows, r0 + rows_per_block);
  float4 g[NV], dg[NV], db[NV], cs[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    g[i] = (c < D4) ? reinterpret_cast<const float4*>(gamma)[c] : zero4();
    dg[i] = db[i] = cs[i] = zero4();
  }
  // One row per wave and iteration.  Everything the row needs (x, dy, the residual gradient, its statistics and its drop-path scale) is
  // requested in ONE batch at the top -- the first version waited for each 256-column chunk on its own and fetched `dres` only behind
  // the two reductions, six dependent HBM round trips per row, and its `s_waitcnt vmcnt(0)` in front of every chunk's store also drained
  // the stores issued before it (CDNA4 counts stores in vmcnt) -- and the two row sums go through DPP / permlane steps instead of
  // twelve ds_bpermute round trips (wave_sum_dpp, common.h).  Optional operands are made unconditional so that the loads stay in one
  // block: without a residual gradient the row of x is read a second time and multiplied by 0, without row scales the scale comes from a
  // constant.
  const float* const rsrc = dres ? dres : x;
  const float rmul = dres ? 1.f : 0.f;
  const float* const scp = rowscale ? rowscale : &ln_one;
  // index of the row's drop-path scale, kept incrementally (one division per wave instead of one 64-bit division per row and chunk)
  int sidx = 0, srem = 0;
  if (rowscale) {
    sidx = (int)((r0 + wave) / rows_per_scale);
    srem = (int)((r0 + wave) - (int64_t)sidx * rows_per_scale);
  }
  for (int64_t row = r0 + wave; row < r1; row += 4) {
    float4 xv[NV], dyv[NV], rv[NV];
    uint2 dyp[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (FULL || c < D4) {
        xv[i] = ldg_f4<false>(reinterpret_cast<const float4*>(x + row * D) + c);
        if (DY_BF16) dyp[i] = ldg_u2<false>(reinterpret_cast<const uint2*>((const uint16_t*)dy + row * D) + c);
        else dyv[i] = ldg_f4<false>(reinterpret_cast<const float4*>((const float*)dy + row * D) + c);
        rv[i] = ldg_f4<false>(reinterpret_cast<const float4*>(rsrc + row * D) + c);
      }
    }
    const float mu = mean[row], rs = rstd[row];
    const float sc = scp[sidx];
    if (rowscale) {
      srem += 4;
      while (srem >= rows_per_scale) { srem -= rows_per_scale; ++sidx; }
    }
    // keep the whole batch of loads above the arithmetic: the scheduler otherwise sinks them chunk by chunk (one exposed round trip each)
    __builtin_amdgcn_sched_barrier(0);
    float4 xh[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (FULL || c < D4) {
        if (DY_BF16) dyv[i] = unpack16x4<TAD_OP16>(dyp[i]);
        xh[i] = make_float4((xv[i].x - mu) * rs, (xv[i].y - mu) * rs, (xv[i].z - mu) * rs, (xv[i].w - mu) * rs);
        const float4 t = mul4(dyv[i], g[i]);
        s1 += (t.x + t.y) + (t.z + t.w);
        s2 += dot4(t, xh[i]);
        acc4(dg[i], mul4(dyv[i], xh[i]));
        acc4(db[i], dyv[i]);
      } else {
        xh[i] = dyv[i] = rv[i] = zero4();
      }
    }
    const float c1 = wave_sum_dpp(s1) / (float)D;
    const float c2 = wave_sum_dpp(s2) / (float)D;
    float4 o[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      o[i].x = fmaf(rv[i].x, rmul, rs * (dyv[i].x * g[i].x - c1 - xh[i].x * c2));
      o[i].y = fmaf(rv[i].y, rmul, rs * (dyv[i].y * g[i].y - c1 - xh[i].y * c2));
      o[i].z = fmaf(rv[i].z, rmul, rs * (dyv[i].z * g[i].z - c1 - xh[i].z * c2));
      o[i].w = fmaf(rv[i].w, rmul, rs * (dyv[i].w * g[i].w - c1 - xh[i].w * c2));
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (FULL || c < D4) stg_f4<false>(reinterpret_cast<float4*>(dx + row * D) + c, o[i]);
      // the bf16 copy and the column sums feed the branch Linear, whose output was scaled per sample (drop-path)
      o[i] = scale4(o[i], sc);
      if (FULL || c < D4) acc4(cs[i], o[i]);
    }
    if (dxb) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (FULL || c < D4) {
          const uint2 p = pack16x4<TAD_OP16>(o[i]);
          stg_u2<false>(reinterpret_cast<uint2*>(dxb + row * D) + c, p);
        }
      }
    }
  }
  rownorm_combine<NV>(partial, D, want_colsum ? 3 : 2, wave, dg, db, cs);
}

TAD_NAMESPACE_END

using namespace tad;

extern "C" {

int tad_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_dtype, float* mean, float* rstd,
                      int64_t rows, int D, float eps, tad_stream_t stream) {
  TAD_REQUIRE(x && gamma && beta && y, "layernorm_fwd: null pointer");
  TAD_REQUIRE(rows > 0 && rownorm_width_ok(D), "layernorm_fwd: D=%d must be a multiple of 4 and <= %d", D, ROWNORM_MAX_D);
  TAD_REQUIRE(y_dtype == TAD_F32 || y_dtype == TAD_OP16, "layernorm_fwd: bad y_dtype %d", y_dtype);
  // float4 loads of x, gamma and beta; y: float4 stores (f32) or 8-byte packed stores (16-bit); mean and rstd are written float by float
  TAD_REQUIRE_ALIGNED("layernorm_fwd", x, 16);
  TAD_REQUIRE_ALIGNED("layernorm_fwd", gamma, 16);
  TAD_REQUIRE_ALIGNED("layernorm_fwd", beta, 16);
  TAD_REQUIRE_ALIGNED("layernorm_fwd", y, y_dtype == TAD_F32 ? 16 : 8);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define LN_FWD(NV)                                                                                                          \
  if (y_dtype == TAD_OP16)                                                                                                  \
    hipLaunchKernelGGL((layernorm_fwd_kernel<NV, true>), grid, block, 0, st, x, gamma, beta, y, mean, rstd, rows, D, eps); \
  else                                                                                                                      \
    hipLaunchKernelGGL((layernorm_fwd_kernel<NV, false>), grid, block, 0, st, x, gamma, beta, y, mean, rstd, rows, D, eps);
  ROWNORM_SWITCH_NV(rownorm_nv(D), LN_FWD)
#undef LN_FWD
  return check_launch("layernorm_fwd");
}

#ifndef TAD_OPND_F16  // format-independent: one copy for the library (bf16 pass)
size_t tad_layernorm_bwd_workspace_bytes(int64_t rows, int D) { return rownorm_bwd_plan(rows, D, 3).partial_floats * sizeof(float); }
#endif

int tad_layernorm_bwd(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean, const float* rstd,
                      const float* dres, float* dx, uint16_t* dx_bf16, float* dgamma, float* dbeta, float* colsum_dx,
                      const float* rowscale, int rows_per_scale, int accumulate, void* ws, size_t ws_bytes, int64_t rows, int D,
                      tad_stream_t stream) {
  TAD_REQUIRE(dy && x && gamma && mean && rstd && dx && dgamma && dbeta && ws, "layernorm_bwd: null pointer");
  TAD_REQUIRE(rows > 0 && rownorm_width_ok(D), "layernorm_bwd: unsupported D=%d", D);
  TAD_REQUIRE(dy_dtype == TAD_F32 || dy_dtype == TAD_OP16, "layernorm_bwd: bad dy_dtype %d", dy_dtype);
  TAD_REQUIRE(!rowscale || rows_per_scale > 0, "layernorm_bwd: rows_per_scale must be positive");
  // float4 accesses to every row operand, the partials in ws and (in the reduction) dgamma / dbeta / colsum_dx; 8-byte pieces of the 16-bit
  // tensors; mean, rstd and rowscale are read float by float
  TAD_REQUIRE_ALIGNED("layernorm_bwd", dy, dy_dtype == TAD_F32 ? 16 : 8);
  TAD_REQUIRE_ALIGNED("layernorm_bwd", x, 16);
  TAD_REQUIRE_ALIGNED("layernorm_bwd", gamma, 16);
  TAD_REQUIRE_ALIGNED("layernorm_bwd", dres, 16);
  TAD_REQUIRE_ALIGNED("layernorm_bwd", dx, 16);
  TAD_REQUIRE_ALIGNED("layernorm_bwd", dx_bf16, 8);
  TAD_REQUIRE_ALIGNED("layernorm_bwd", dgamma, 16);
  TAD_REQUIRE_ALIGNED("layernorm_bwd", dbeta, 16);
  TAD_REQUIRE_ALIGNED("layernorm_bwd", colsum_dx, 16);
  TAD_REQUIRE_ALIGNED("layernorm_bwd", ws, 16);
  const RowNormBwd p = rownorm_bwd_plan(rows, D, 3);
  if (ws_bytes < p.partial_floats * sizeof(float)) { set_error("layernorm_bwd: workspace too small"); return TAD_ENOSPACE; }
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)ws;
  const int want_cs = colsum_dx != nullptr;
#define LN_BWD_(NV, BF, FULL_)                                                                                                        \
  hipLaunchKernelGGL((layernorm_bwd_kernel<NV, BF, FULL_>), dim3(p.blocks), dim3(256), p.smem_bytes, st, dy, x, gamma, mean, rstd, dres, \
                     dx, dx_bf16, partial, rows, D, p.rows_per_block, want_cs, rowscale, rows_per_scale)
#define LN_BWD_F(NV, BF) \
  if (D == 256 * NV) LN_BWD_(NV, BF, true); else LN_BWD_(NV, BF, false)
#define LN_BWD(NV) \
  if (dy_dtype == TAD_OP16) { LN_BWD_F(NV, true); } else { LN_BWD_F(NV, false); }
  ROWNORM_SWITCH_NV(rownorm_nv(D), LN_BWD)
#undef LN_BWD
#undef LN_BWD_F
#undef LN_BWD_
  int rc = check_launch("layernorm_bwd");
  if (rc) return rc;
  return launch_reduce_cols(partial, dgamma, dbeta, colsum_dx, colsum_dx ? 3 : 2, p.blocks, D, accumulate ? 1 : 0, st);
}

}  // extern "C"
