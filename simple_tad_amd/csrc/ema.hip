// Multi-tensor weight EMA (timm.utils.ModelEma.update, called after every optimizer step by engine_for_finetuning.py:98-99 and
// engine_for_frame_finetuning.py:156-175): ONE launch updates every f32 tensor pair of the model, one streaming pass of 12 B per
// element (read ema, read model, write ema) instead of ~4 torch launches and ~36 B per element per tensor.
//
// Arithmetic = the reference's `ema_v.copy_(ema_v * decay + (1. - decay) * model_v)` on f32 tensors with a Python-float decay:
// three roundings, e' = fl( fl(e * (float)d) + fl(m * (float)(1.0 - d)) ), where 1.0 - d is taken in double by the caller.  An FMA
// would round once less and differ in the last bit of about a quarter of the values at d = 0.9999, so this file is compiled with
// -ffp-contract=off (simple_tad_amd/build.py, NO_FP_CONTRACT) instead of the library's -ffp-contract=fast, under which the code
// generator fuses an fmul + fadd pair whatever the source says; the pragma below only documents the intent.
#include "common.h"
#include <math.h>

TAD_NAMESPACE_BEGIN

typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
constexpr int EMA_THREADS = 256;
constexpr int EMA_VEC_ITERS = TAD_EMA_CHUNK / (EMA_THREADS * 4);
static_assert(EMA_VEC_ITERS * EMA_THREADS * 4 == TAD_EMA_CHUNK, "a chunk is a whole number of float4 sweeps of the workgroup");

__device__ __forceinline__ float ema_blend(float e, float m, float d, float omd) {
#pragma clang fp contract(off)
  return e * d + m * omd;
}

__device__ __forceinline__ f32x4 ema_blend4(f32x4 e, f32x4 m, float d, float omd) {
  return f32x4{ema_blend(e.x, m.x, d, omd), ema_blend(e.y, m.y, d, omd), ema_blend(e.z, m.z, d, omd), ema_blend(e.w, m.w, d, omd)};
}

// One workgroup per chunk of TAD_EMA_CHUNK elements of one tensor: chunks[b] = {tensor index, chunk index within the tensor};
// tensors[t] = {ema address, model address, numel, 0}.  A chunk starts at a multiple of TAD_EMA_CHUNK elements, so it keeps the
// 16-byte alignment of its tensor: float4 loads and stores when both pointers are 16-byte aligned, scalar ones otherwise.
__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(const int64_t* __restrict__ tensors, int n_tensors,
                                                                 const int2* __restrict__ chunks, float decay, float omd) {
  const int2 c = chunks[blockIdx.x];
  if (c.x < 0 || c.x >= n_tensors || c.y < 0) return;  // (the host builds the table; a malformed entry is never dereferenced)
  const int64_t* t = tensors + 4 * (int64_t)c.x;
  const int64_t numel = t[2], start = (int64_t)c.y * TAD_EMA_CHUNK;
  if (start >= numel) return;
  // (addresses read from a table: spelled as global-memory pointers so that the compiler emits global_ rather than flat_ accesses)
  gfloat* e = (gfloat*)(uintptr_t)t[0] + start;
  const gfloat* m = (const gfloat*)(uintptr_t)t[1] + start;
  const int cnt = (int)(numel - start < TAD_EMA_CHUNK ? numel - start : TAD_EMA_CHUNK);
  const int tid = threadIdx.x;
  int scalar_from = 0;
  if ((((uintptr_t)e | (uintptr_t)m) & 15) == 0) {
    const gf32x4* e4 = (const gf32x4*)e;
    const gf32x4* m4 = (const gf32x4*)m;
    gf32x4* o4 = (gf32x4*)e;
    const int n4 = cnt >> 2;
    if (n4 == EMA_VEC_ITERS * EMA_THREADS) {  // a whole chunk: every load of the thread in flight before the first store
      f32x4 ev[EMA_VEC_ITERS], mv[EMA_VEC_ITERS];
#pragma unroll
      for (int k = 0; k < EMA_VEC_ITERS; ++k) {
        ev[k] = e4[k * EMA_THREADS + tid];
        mv[k] = m4[k * EMA_THREADS + tid];
      }
#pragma unroll
      for (int k = 0; k < EMA_VEC_ITERS; ++k) o4[k * EMA_THREADS + tid] = ema_blend4(ev[k], mv[k], decay, omd);
    } else {  // the last chunk of a tensor
#pragma unroll 1
      for (int i = tid; i < n4; i += EMA_THREADS) o4[i] = ema_blend4(e4[i], m4[i], decay, omd);
    }
    scalar_from = n4 << 2;
  }
#pragma unroll 1
  for (int i = scalar_from + tid; i < cnt; i += EMA_THREADS) e[i] = ema_blend(e[i], m[i], decay, omd);
}

TAD_NAMESPACE_END

using namespace tad;

extern "C" int tad_ema_update(const int64_t* tensors, int n_tensors, const int32_t* chunks, int n_chunks, float decay,
                              float one_minus_decay, tad_stream_t stream) {
  TAD_REQUIRE(tensors && chunks, "ema_update: null pointer");
  TAD_REQUIRE(n_tensors > 0 && n_chunks > 0, "ema_update: n_tensors=%d / n_chunks=%d must be positive", n_tensors, n_chunks);
  TAD_REQUIRE(isfinite(decay) && isfinite(one_minus_decay) && decay >= 0.f && decay <= 1.f && one_minus_decay >= 0.f &&
                  one_minus_decay <= 1.f,
              "ema_update: decay=%g / one_minus_decay=%g must be finite and in [0, 1]", (double)decay, (double)one_minus_decay);
  TAD_REQUIRE_ALIGNED("ema_update", tensors, 8);
  TAD_REQUIRE_ALIGNED("ema_update", chunks, 8);
  hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)n_chunks), dim3(EMA_THREADS), 0, (hipStream_t)stream, tensors, n_tensors,
                     reinterpret_cast<const int2*>(chunks), decay, one_minus_decay);
  return check_launch("ema_update");
}
