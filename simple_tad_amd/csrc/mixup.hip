// Mixup / CutMix on the device and the soft-target cross entropy that goes with them (mixup.py:159-218 of the reference, applied to the
// f32 clip batch at engine_for_finetuning.py:59-60; timm.loss.SoftTargetCrossEntropy / LabelSmoothingCrossEntropy,
// run_class_finetuning.py:467-473).
//
// tad_mixup_clips mixes a contiguous f32 clip batch [B, C, T, H, W] IN PLACE, one launch: the thread that owns an offset of sample i also
// owns the same offset of its partner j = B-1-i, loads both ORIGINAL values, then stores both results.  So the per-sample modes of the
// reference ('elem': sample i and sample j follow different plans) need no copy of the batch, and a blend moves 2 x 4 B in and 2 x 4 B out
// per element pair where `x.flip(0).mul_(1-lam); x.mul_(lam).add_(x_flipped)` makes nine passes and a temporary of the clip's size.
//
// Arithmetic of a blend = the reference's, three roundings: x' = fl( fl(x_i * w_self) + fl(x_j * w_other) ).  An FMA rounds once less, so
// this file is compiled with -ffp-contract=off like ema.hip (simple_tad_amd/build.py, NO_FP_CONTRACT); the pragmas only document it.
#include "common.h"
#include <math.h>

TAD_NAMESPACE_BEGIN

constexpr int MIX_THREADS = 256;
constexpr int MIX_MAX_BLOCKS = 256 * 8;  // Guideline 11: a memory-bound kernel gets a capped grid (8 workgroups per CU) and strides
constexpr int CE_WAVES = 16;

struct MixPlan {  // one row of the plan table (TAD_MIXUP_PLAN_WORDS int32)
  int kind;
  float w_self, w_other;
  int t0, t1, y0, y1, x0, x1;
  float lam, one_minus_lam;
  int pad;
};
static_assert(sizeof(MixPlan) == 4 * TAD_MIXUP_PLAN_WORDS, "plan row layout");

__device__ __forceinline__ float mix_blend(float a, float b, float wa, float wb) {
#pragma clang fp contract(off)
  return a * wa + b * wb;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the row as the kernel uses it: an unknown kind is a keep, a box is cut to the clip (a malformed table is never an address)
__device__ __forceinline__ MixPlan load_plan(const int32_t* plan, int s, int T, int H, int W) {
  MixPlan p = *reinterpret_cast<const MixPlan*>(plan + (int64_t)s * TAD_MIXUP_PLAN_WORDS);
  if (p.kind != TAD_MIX_BLEND && p.kind != TAD_MIX_PASTE) p.kind = TAD_MIX_KEEP;
  p.t0 = clampi(p.t0, 0, T), p.t1 = clampi(p.t1, p.t0, T);
  p.y0 = clampi(p.y0, 0, H), p.y1 = clampi(p.y1, p.y0, H);
  p.x0 = clampi(p.x0, 0, W), p.x1 = clampi(p.x1, p.x0, W);
  if (p.kind == TAD_MIX_PASTE && (p.t0 == p.t1 || p.y0 == p.y1 || p.x0 == p.x1)) p.kind = TAD_MIX_KEEP;  // an empty box
  return p;
}

template <int V>
struct Vec;
template <>
struct Vec<1> {
  typedef float type;
};
template <>
struct Vec<4> {
  typedef f32x4 type;
};

template <int V>
__device__ __forceinline__ float comp(const typename Vec<V>::type& v, int k) {
  if constexpr (V == 1) return v;
  else return v[k];
}
template <int V>
__device__ __forceinline__ void set_comp(typename Vec<V>::type& v, int k, float f) {
  if constexpr (V == 1) v = f;
  else v[k] = f;
}

// What sample `self` becomes at (t, y, x .. x+V-1) and the store of it: a blend writes the whole vector, a paste the components inside
// its box (one vector store when all V are, scalar stores at a box edge that falls inside the vector), a keep nothing.
template <int V>
__device__ __forceinline__ void mix_store(float* dst, const MixPlan& p, const typename Vec<V>::type& self,
                                          const typename Vec<V>::type& other, int t, int y, int x) {
  typedef typename Vec<V>::type vec_t;
  if (p.kind == TAD_MIX_BLEND) {
    vec_t r;
#pragma unroll
    for (int k = 0; k < V; ++k) set_comp<V>(r, k, mix_blend(comp<V>(self, k), comp<V>(other, k), p.w_self, p.w_other));
    *reinterpret_cast<vec_t*>(dst) = r;
  } else if (p.kind == TAD_MIX_PASTE) {
    if (t < p.t0 || t >= p.t1 || y < p.y0 || y >= p.y1 || x + V <= p.x0 || x >= p.x1) return;
    if (x >= p.x0 && x + V <= p.x1) {
      *reinterpret_cast<vec_t*>(dst) = other;
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (x + k >= p.x0 && x + k < p.x1) dst[k] = comp<V>(other, k);
    }
  }
}

// blockIdx.y = pair (i, B-1-i); the workgroups of a pair stride over its work items (vectors of V floats along W).
//  * no paste in the pair: the items are the flat vectors of a sample -- no coordinates, four pairs of loads in flight per thread;
//  * otherwise the items cover [t_lo, t_hi) x [y_lo, y_hi) x [xv_lo, xv_hi) of every channel: the whole sample when one side blends,
//    the union of the two boxes when both sides paste (or keep), so that a CutMix touches the bytes of its box and no others.
template <int V>
__global__ __launch_bounds__(MIX_THREADS) void mixup_clips_kernel(float* __restrict__ x, const int32_t* __restrict__ plan, int B, int C,
                                                                  int T, int H, int W) {
  typedef typename Vec<V>::type vec_t;
  const int i = blockIdx.y, j = B - 1 - i;
  const MixPlan pi = load_plan(plan, i, T, H, W), pj = load_plan(plan, j, T, H, W);
  if (pi.kind == TAD_MIX_KEEP && pj.kind == TAD_MIX_KEEP) return;
  const int64_t n = (int64_t)C * T * H * W;  // (elements of a sample; the host checks n < 2^31)
  float* xi = x + (int64_t)i * n;
  float* xj = x + (int64_t)j * n;
  const int stride = gridDim.x * MIX_THREADS;
  const int first = blockIdx.x * MIX_THREADS + threadIdx.x;
  if (pi.kind != TAD_MIX_PASTE && pj.kind != TAD_MIX_PASTE) {
    const int nv = (int)(n / V);
    int64_t w = first;
    for (; w + 3 * (int64_t)stride < nv; w += 4 * (int64_t)stride) {
      vec_t a[4], b[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k] = *reinterpret_cast<const vec_t*>(xi + (w + (int64_t)k * stride) * V);
        b[k] = *reinterpret_cast<const vec_t*>(xj + (w + (int64_t)k * stride) * V);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        mix_store<V>(xi + (w + (int64_t)k * stride) * V, pi, a[k], b[k], 0, 0, 0);
        mix_store<V>(xj + (w + (int64_t)k * stride) * V, pj, b[k], a[k], 0, 0, 0);
      }
    }
    for (; w < nv; w += stride) {
      const vec_t a = *reinterpret_cast<const vec_t*>(xi + w * V);
      const vec_t b = *reinterpret_cast<const vec_t*>(xj + w * V);
      mix_store<V>(xi + w * V, pi, a, b, 0, 0, 0);
      mix_store<V>(xj + w * V, pj, b, a, 0, 0, 0);
    }
    return;
  }
  int t_lo = 0, t_hi = T, y_lo = 0, y_hi = H, x_lo = 0, x_hi = W;
  if (pi.kind != TAD_MIX_BLEND && pj.kind != TAD_MIX_BLEND) {
    const bool ei = pi.kind == TAD_MIX_KEEP, ej = pj.kind == TAD_MIX_KEEP;  // (at most one of them: an empty box is a keep)
    t_lo = ei ? pj.t0 : ej ? pi.t0 : min(pi.t0, pj.t0), t_hi = ei ? pj.t1 : ej ? pi.t1 : max(pi.t1, pj.t1);
    y_lo = ei ? pj.y0 : ej ? pi.y0 : min(pi.y0, pj.y0), y_hi = ei ? pj.y1 : ej ? pi.y1 : max(pi.y1, pj.y1);
    x_lo = ei ? pj.x0 : ej ? pi.x0 : min(pi.x0, pj.x0), x_hi = ei ? pj.x1 : ej ? pi.x1 : max(pi.x1, pj.x1);
  }
  const int xv_lo = x_lo / V, dxv = (x_hi + V - 1) / V - xv_lo, dy = y_hi - y_lo, dt = t_hi - t_lo;
  const int64_t items = (int64_t)C * dt * dy * dxv;  // (<= n / V < 2^31)
  for (int64_t w64 = first; w64 < items; w64 += stride) {
    const int w = (int)w64;
    const int xv = w % dxv, r = w / dxv;
    const int y = y_lo + r % dy, r2 = r / dy;
    const int t = t_lo + r2 % dt, c = r2 / dt;
    const int xx = (xv_lo + xv) * V;
    const int64_t off = (((int64_t)c * T + t) * H + y) * W + xx;
    const vec_t a = *reinterpret_cast<const vec_t*>(xi + off);
    const vec_t b = *reinterpret_cast<const vec_t*>(xj + off);
    mix_store<V>(xi + off, pi, a, b, t, y, xx);
    mix_store<V>(xj + off, pj, b, a, t, y, xx);
  }
}

// mixup_target (mixup.py:22-27): out[b][c] = fl( fl(y1 * lam_b) + fl(y2 * (1 - lam)_b) ), y1 / y2 = the smoothed one-hot rows of
// labels[b] / labels[B-1-b]; lam and 1 - lam per sample from the plan table, as the host rounded them.
__global__ __launch_bounds__(MIX_THREADS) void mixup_target_kernel(const int32_t* __restrict__ plan, const int64_t* __restrict__ labels,
                                                                   float* __restrict__ out, int B, int classes, float on, float off) {
  const int64_t total = (int64_t)B * classes;
  for (int64_t e = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * MIX_THREADS) {
    const int b = (int)(e / classes), c = (int)(e - (int64_t)b * classes);
    const MixPlan* p = reinterpret_cast<const MixPlan*>(plan + (int64_t)b * TAD_MIXUP_PLAN_WORDS);
    const float y1 = labels[b] == c ? on : off, y2 = labels[B - 1 - b] == c ? on : off;
    out[e] = mix_blend(y1, y2, p->lam, p->one_minus_lam);
  }
}

// Soft-target cross entropy, a wave per row: loss = (1/B) sum_b sum_c -t[b][c] * log_softmax(z[b])[c] and, in the same launch,
// dlogits = (softmax(z[b]) * sum_c t[b][c] - t[b]) / B.  The target row is read (target != nullptr) or formed from a hard label with
// smoothing s: t[c] = s / classes + (c == label ? 1 - s : 0) (timm's LabelSmoothingCrossEntropy written as one weighted sum).
// One workgroup of CE_WAVES waves walks the rows, so the batch mean is a fixed-order sum inside the launch (no atomics, no second
// launch): a loss batch is at most a few hundred rows of at most a few thousand logits, a latency-bound problem either way.  The row
// losses are added up in double (a handful of additions per wave): in f32 the running sum over the rows, B times a row's size, would
// lose more to its own roundings than all the f32 work inside the rows does.
__global__ __launch_bounds__(CE_WAVES * WAVE) void soft_target_ce_kernel(const float* __restrict__ z, const float* __restrict__ target,
                                                                         const int64_t* __restrict__ labels, float smoothing,
                                                                         float* __restrict__ loss, float* __restrict__ dz, int B,
                                                                         int classes) {
  __shared__ double part[CE_WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const float inv_b = 1.f / (float)B, t_off = smoothing / (float)classes, t_on = 1.f - smoothing;
  double acc = 0.0;
  for (int b = wave; b < B; b += CE_WAVES) {
    const float* zr = z + (int64_t)b * classes;
    const float* tr = target ? target + (int64_t)b * classes : nullptr;
    const int64_t label = tr ? -1 : labels[b];
    float m = -INFINITY;
    for (int c = lane; c < classes; c += WAVE) m = fmaxf(m, zr[c]);
    m = wave_max(m);
    float se = 0.f, st = 0.f;
    for (int c = lane; c < classes; c += WAVE) {
      se += expf(zr[c] - m);
      st += tr ? tr[c] : t_off + (c == label ? t_on : 0.f);
    }
    se = wave_sum(se), st = wave_sum(st);
    const float lse = logf(se), inv_se = 1.f / se;
    float row = 0.f;
    for (int c = lane; c < classes; c += WAVE) {
      const float d = zr[c] - m, t = tr ? tr[c] : t_off + (c == label ? t_on : 0.f);
      row -= t * (d - lse);
      dz[(int64_t)b * classes + c] = (expf(d) * inv_se * st - t) * inv_b;
    }
    acc += (double)wave_sum(row);
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < CE_WAVES; ++k) s += part[k];
    *loss = (float)(s / (double)B);
  }
}

TAD_NAMESPACE_END

using namespace tad;

static int mix_shape_ok(int B, int C, int T, int H, int W, const char* who) {
  TAD_REQUIRE(B > 0 && B % 2 == 0, "%s: B=%d must be even and positive (sample i is mixed with sample B-1-i)", who, B);
  TAD_REQUIRE(C > 0 && T > 0 && H > 0 && W > 0, "%s: C=%d T=%d H=%d W=%d must be positive", who, C, T, H, W);
  TAD_REQUIRE((int64_t)C * T * H * W < ((int64_t)1 << 31), "%s: a sample of C*T*H*W=%lld elements exceeds 2^31-1", who,
              (long long)((int64_t)C * T * H * W));
  return TAD_OK;
}

extern "C" int tad_mixup_plan_check(const int32_t* plan_host, int B, int T, int H, int W) {
  TAD_REQUIRE(plan_host, "mixup_plan_check: null pointer");
  if (int rc = mix_shape_ok(B, 1, T, H, W, "mixup_plan_check")) return rc;
  for (int s = 0; s < B; ++s) {
    const MixPlan* p = reinterpret_cast<const MixPlan*>(plan_host + (int64_t)s * TAD_MIXUP_PLAN_WORDS);
    TAD_REQUIRE(p->kind == TAD_MIX_KEEP || p->kind == TAD_MIX_BLEND || p->kind == TAD_MIX_PASTE, "mixup_plan_check: sample %d: kind=%d", s,
                p->kind);
    TAD_REQUIRE(isfinite(p->w_self) && isfinite(p->w_other) && isfinite(p->lam) && isfinite(p->one_minus_lam),
                "mixup_plan_check: sample %d: non-finite coefficient (w_self=%g w_other=%g lam=%g one_minus_lam=%g)", s, (double)p->w_self,
                (double)p->w_other, (double)p->lam, (double)p->one_minus_lam);
    TAD_REQUIRE(0 <= p->t0 && p->t0 <= p->t1 && p->t1 <= T && 0 <= p->y0 && p->y0 <= p->y1 && p->y1 <= H && 0 <= p->x0 && p->x0 <= p->x1 &&
                    p->x1 <= W,
                "mixup_plan_check: sample %d: box t[%d,%d) y[%d,%d) x[%d,%d) outside the clip T=%d H=%d W=%d", s, p->t0, p->t1, p->y0,
                p->y1, p->x0, p->x1, T, H, W);
  }
  return TAD_OK;
}

extern "C" int tad_mixup_clips(float* x, const int32_t* plan, int B, int C, int T, int H, int W, tad_stream_t stream) {
  TAD_REQUIRE(x && plan, "mixup_clips: null pointer");
  if (int rc = mix_shape_ok(B, C, T, H, W, "mixup_clips")) return rc;
  TAD_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(plan) & 3) == 0,
              "mixup_clips: x and plan must be 4-byte aligned");
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && W % 4 == 0;  // (then every sample and every row starts on 16 bytes)
  const int64_t items = (int64_t)C * T * H * W / (vec ? 4 : 1);
  const int pairs = B / 2;
  int64_t gx = (items + MIX_THREADS - 1) / MIX_THREADS;
  const int64_t cap = pairs >= MIX_MAX_BLOCKS ? 1 : MIX_MAX_BLOCKS / pairs;
  if (gx > cap) gx = cap;
  TAD_REQUIRE(pairs <= 65535, "mixup_clips: B=%d exceeds the grid's 65535 pairs", B);
  const dim3 grid((unsigned)gx, (unsigned)pairs);
  if (vec)
    hipLaunchKernelGGL(mixup_clips_kernel<4>, grid, dim3(MIX_THREADS), 0, (hipStream_t)stream, x, plan, B, C, T, H, W);
  else
    hipLaunchKernelGGL(mixup_clips_kernel<1>, grid, dim3(MIX_THREADS), 0, (hipStream_t)stream, x, plan, B, C, T, H, W);
  return check_launch("mixup_clips");
}

extern "C" int tad_mixup_target(const int32_t* plan, const int64_t* labels, float* out, int B, int num_classes, float on_value,
                                float off_value, tad_stream_t stream) {
  TAD_REQUIRE(plan && labels && out, "mixup_target: null pointer");
  TAD_REQUIRE(B > 0 && B % 2 == 0, "mixup_target: B=%d must be even and positive", B);
  TAD_REQUIRE(num_classes > 0, "mixup_target: num_classes=%d must be positive", num_classes);
  TAD_REQUIRE(isfinite(on_value) && isfinite(off_value), "mixup_target: on_value=%g / off_value=%g must be finite", (double)on_value,
              (double)off_value);
  TAD_REQUIRE((reinterpret_cast<uintptr_t>(labels) & 7) == 0 && ((reinterpret_cast<uintptr_t>(plan) | reinterpret_cast<uintptr_t>(out)) & 3) == 0,
              "mixup_target: labels must be 8-byte, plan and out 4-byte aligned");
  int64_t blocks = ((int64_t)B * num_classes + MIX_THREADS - 1) / MIX_THREADS;
  if (blocks > MIX_MAX_BLOCKS) blocks = MIX_MAX_BLOCKS;
  hipLaunchKernelGGL(mixup_target_kernel, dim3((unsigned)blocks), dim3(MIX_THREADS), 0, (hipStream_t)stream, plan, labels, out, B,
                     num_classes, on_value, off_value);
  return check_launch("mixup_target");
}

extern "C" int tad_soft_target_ce(const float* logits, const float* target, const int64_t* labels, float smoothing, float* loss,
                                  float* dlogits, int B, int num_classes, tad_stream_t stream) {
  TAD_REQUIRE(logits && loss && dlogits, "soft_target_ce: null pointer");
  TAD_REQUIRE((target != nullptr) != (labels != nullptr), "soft_target_ce: exactly one of target (soft rows) and labels (hard) is given");
  TAD_REQUIRE(B > 0 && num_classes >= 2, "soft_target_ce: B=%d must be positive and num_classes=%d at least 2", B, num_classes);
  TAD_REQUIRE(isfinite(smoothing) && smoothing >= 0.f && smoothing < 1.f, "soft_target_ce: smoothing=%g must be in [0, 1)", (double)smoothing);
  TAD_REQUIRE(((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(loss) |
                reinterpret_cast<uintptr_t>(dlogits)) & 3) == 0 && (reinterpret_cast<uintptr_t>(labels) & 7) == 0,
              "soft_target_ce: f32 operands must be 4-byte, labels 8-byte aligned");
  hipLaunchKernelGGL(soft_target_ce_kernel, dim3(1), dim3(CE_WAVES * WAVE), 0, (hipStream_t)stream, logits, target, labels, smoothing,
                     loss, dlogits, B, num_classes);
  return check_launch("soft_target_ce");
}
