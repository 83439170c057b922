// The entry of the InternVideo2 MAE encoder (internvideo2_pretrain_videomae.py, forward_features): `x = patch_embed(x) + pos_embed;
// x_vis = x[~mask].reshape(B, -1, C)` with a TRAINABLE position table -- the pre-training ABI of include/tad_mi355x_pretrain.h (tadp_*).
// Forward: the add and the selection in one pass over the visible rows alone.  Backward: the scatter of the gradient to [B,N,D] (every row
// written, so no zero fill) and the table's gradient, a sum over the clips in the order b = 0, 1, ..., in one launch without atomics.
// HBM-bound row movers; every row is D f32 with D % 4 == 0 (one float4 per thread and step).  Compiled ONCE: f32 only, no _f16 twin.
// Only adds: nothing here can be contracted into an FMA.
#include "common.h"
#include "../../include/tad_mi355x_pretrain.h"

TAD_NAMESPACE_BEGIN

__device__ __forceinline__ float4 vt_add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// One thread per float4 of the output: item = r * D4 + c, r = b * Nv + i.  Stores never depend on an index.
__global__ __launch_bounds__(256) void visible_tokens_fwd_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                                 const int32_t* __restrict__ tok, float* __restrict__ out, int64_t items,
                                                                 int N, int Nv, int D4) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int64_t r = it / D4;
    const int c = (int)(it - r * D4);
    const int64_t b = r / Nv;
    const int64_t t = tok[r];
    const float4 u = ldg_f4<false>(reinterpret_cast<const float4*>(x) + (b * N + t) * D4 + c);
    const float4 v = ldg_f4<false>(reinterpret_cast<const float4*>(pos) + t * D4 + c);
    stg_f4<false>(reinterpret_cast<float4*>(out) + it, vt_add4(u, v));
  }
}

// One thread per float4 column group of one token: item = n * D4 + c.  It walks the clips in order; what it reads from g is chosen by
// slot, what it writes (dx[b, n], dpos[n]) is not.  DX / DPOS: which outputs exist (the host picks the instance).
template <bool DX, bool DPOS>
__global__ __launch_bounds__(256) void visible_tokens_bwd_kernel(const float* __restrict__ g, const int32_t* __restrict__ slot,
                                                                 float* __restrict__ dx, float* __restrict__ dpos, int accumulate,
                                                                 int64_t items, int B, int N, int Nv, int D4) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int64_t n = it / D4;
    const int c = (int)(it - n * D4);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int b = 0; b < B; ++b) {
      const int s = slot[(int64_t)b * N + n];
      const bool vis = s >= 0 && s < Nv;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (vis) v = ldg_f4<false>(reinterpret_cast<const float4*>(g) + ((int64_t)b * Nv + s) * D4 + c);
      if constexpr (DX) stg_f4<false>(reinterpret_cast<float4*>(dx) + ((int64_t)b * N + n) * D4 + c, v);
      if constexpr (DPOS) {
        if (vis) acc = vt_add4(acc, v);
      }
    }
    if constexpr (DPOS) {
      float4* d = reinterpret_cast<float4*>(dpos) + it;
      if (accumulate) acc = vt_add4(ldg_f4<false>(d), acc);
      stg_f4<false>(d, acc);
    }
  }
}

TAD_NAMESPACE_END

using namespace tad;

extern "C" {

int tadp_abi_version(void) { return TADP_ABI_VERSION; }

int tadp_visible_tokens_fwd(const float* x, const float* pos, const int32_t* tok, float* out, int B, int N, int Nv, int D,
                            tad_stream_t stream) {
  TAD_REQUIRE(x && pos && tok && out, "visible_tokens_fwd: null pointer");
  TAD_REQUIRE(B > 0 && N > 0 && Nv > 0 && D > 0, "visible_tokens_fwd: B=%d, N=%d, Nv=%d, D=%d must all be positive", B, N, Nv, D);
  TAD_REQUIRE(Nv <= N, "visible_tokens_fwd: Nv=%d exceeds N=%d", Nv, N);
  TAD_REQUIRE(D % 4 == 0, "visible_tokens_fwd: D=%d must be a multiple of 4", D);
  // float4 loads of x and pos, float4 stores to out; tok is read int by int
  TAD_REQUIRE_ALIGNED("visible_tokens_fwd", x, 16);
  TAD_REQUIRE_ALIGNED("visible_tokens_fwd", pos, 16);
  TAD_REQUIRE_ALIGNED("visible_tokens_fwd", out, 16);
  const int64_t items = (int64_t)B * Nv * (D / 4);
  hipLaunchKernelGGL(visible_tokens_fwd_kernel, dim3(capped_grid(items, 256)), dim3(256), 0, (hipStream_t)stream, x, pos, tok, out, items, N,
                     Nv, D / 4);
  return check_launch("visible_tokens_fwd");
}

int tadp_visible_tokens_bwd(const float* g, const int32_t* slot, float* dx, float* dpos, int accumulate, int B, int N, int Nv, int D,
                            tad_stream_t stream) {
  TAD_REQUIRE(g && slot, "visible_tokens_bwd: null pointer");
  TAD_REQUIRE(dx || dpos, "visible_tokens_bwd: dx and dpos are both null: nothing to compute");
  TAD_REQUIRE(B > 0 && N > 0 && Nv > 0 && D > 0, "visible_tokens_bwd: B=%d, N=%d, Nv=%d, D=%d must all be positive", B, N, Nv, D);
  TAD_REQUIRE(Nv <= N, "visible_tokens_bwd: Nv=%d exceeds N=%d", Nv, N);
  TAD_REQUIRE(D % 4 == 0, "visible_tokens_bwd: D=%d must be a multiple of 4", D);
  // float4 loads of g, float4 stores to dx, float4 loads (accumulate) and stores of dpos; slot is read int by int
  TAD_REQUIRE_ALIGNED("visible_tokens_bwd", g, 16);
  TAD_REQUIRE_ALIGNED("visible_tokens_bwd", dx, 16);
  TAD_REQUIRE_ALIGNED("visible_tokens_bwd", dpos, 16);
  const int64_t items = (int64_t)N * (D / 4);
  const dim3 grid(capped_grid(items, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define VT_BWD(DX_, DPOS_) \
  hipLaunchKernelGGL((visible_tokens_bwd_kernel<DX_, DPOS_>), grid, block, 0, st, g, slot, dx, dpos, accumulate ? 1 : 0, items, B, N, Nv, D / 4)
  if (dx && dpos) VT_BWD(true, true);
  else if (dx) VT_BWD(true, false);
  else VT_BWD(false, true);
#undef VT_BWD
  return check_launch("visible_tokens_bwd");
}

}  // extern "C"
