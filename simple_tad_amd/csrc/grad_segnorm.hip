// Per-head gradient-norm diagnostics (utils.collect_grad_norms / collect_grad_norms_pretrain of the reference: one .norm().item() per
// attention head and per large tensor after every step) as ONE segmented sum-of-squares pass over the flat gradient buffer of
// flat.FlatSpace.  A head's slice of qkv.weight.grad.view(3, H, hd, D)[i, h] is hd * D contiguous floats of that buffer, and so is every
// other tensor the reference looks at: the whole table is a list of (offset, length, slot) segments, built once per model by the host
// (simple_tad_amd/grad_norms.py), and nothing is read back per step -- the results accumulate on the device over the epoch.
//
// Tables (device memory, only read; tad_grad_segnorm_plan_check validates HOST copies of them once, when they are created):
//   segments  tad_segnorm_seg  {int64 offset, int64 length, int32 slot, int32 first_work}   nseg rows
//   work      tad_segnorm_work {int64 offset, int64 length}                                 nwork rows
// Segment lengths run from one head's bias slice (64 floats) to a whole fc1 weight (4 D D), so the host cuts every segment into work
// items of at most TAD_SEGNORM_WORK_MAX floats, in order; a segment's items are work[first_work .. first_work of the next segment).
//
// Two launches, reduce then finish:
//   reduce   one workgroup per work item -> partial[item] (f32, in the workspace)
//   finish   one wave per segment: its partials added in f64 in a fixed order, the root, the coefficient, then last / acc / counters
// Two launches and not one with an integer ticket: stream order is the dependency, so no workgroup spins on or fences for another one,
// the finish is a few microseconds behind a pass that is bound by HBM, and the reduce kernel stays the plain streaming loop of
// sumsq_kernel (elementwise.hip).  No floating-point atomics anywhere: the result is bit-identical from run to run (elementwise.hip,
// "sum of squares", records why).  The only atomic is an integer add on the nonfinite_values counter.
//
// depth = 17: the longest chain of f32 additions that one element's square passes through, for this chunking (256 lanes, work items of
// at most 16384 floats = 4096 float4 = 16 per lane, four accumulators per lane):
//    2   inside a float4: (x^2 + y^2) + (z^2 + w^2)
//    5   lane-serial: an accumulator takes at most 4 of the lane's 16 float4 sums, and one scalar head or tail element
//    2   the lane's four accumulators: (s0 + s1) + (s2 + s3)
//    6   the wave's butterfly over 64 lanes
//    2   the workgroup's four waves: (r0 + r1) + (r2 + r3)
//    0   finish: the partials of a slot are added in f64 (53 bits under sums of at most a few thousand f32 values: no f32 rounding)
// Every term is non-negative, so the relative error of the f32 sum is at most (depth + 1) * 2^-24 (the + 1: the rounding of the square
// itself); the root halves it, and the conversion of the f64 root to f32 and the product with the coefficient add one rounding each.
// tests/test_grad_norms_gpu.py takes its tolerance (depth + 2) * 2^-24 from this number.
#include "common.h"
#include <math.h>
#include <vector>

TAD_NAMESPACE_BEGIN

constexpr int SEGNORM_THREADS = 256;
static_assert(TAD_SEGNORM_WORK_MAX % 4 == 0 && TAD_SEGNORM_WORK_MAX / 4 == 16 * SEGNORM_THREADS, "depth above assumes 16 float4 per lane");

__device__ __forceinline__ float sq4(const float4& a) { return (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w); }

// partial[item] = sum of squares of grad[offset, offset + length).  16-byte loads from the first 16-byte boundary on; the `head` floats in
// front of it and the (length - head) % 4 behind the last whole float4 go to single lanes.  An item that does not lie inside [0, n) or
// is longer than the maximum (the plan check refuses such a table; the device copy is not trusted with addresses) reads nothing and
// leaves 0.
__global__ __launch_bounds__(SEGNORM_THREADS) void segnorm_reduce_kernel(const float* __restrict__ grad, int64_t n,
                                                                        const tad_segnorm_work* __restrict__ work,
                                                                        float* __restrict__ partial) {
  __shared__ float red[SEGNORM_THREADS / WAVE];
  const int64_t off = work[blockIdx.x].offset, len = work[blockIdx.x].length;
  const int tid = threadIdx.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (off >= 0 && len > 0 && len <= TAD_SEGNORM_WORK_MAX && off <= n - len) {
    const float* __restrict__ x = grad + off;
    const int head = (int)min<int64_t>(len, (int64_t)((16 - ((uintptr_t)x & 15)) & 15) / 4);
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x + head);
    const int n4 = (int)((len - head) >> 2);  // <= 4096: at most four rounds of the unrolled loop, or three and three single steps
    constexpr int S = SEGNORM_THREADS;
    int i = tid;
    for (; i + 3 * S < n4; i += 4 * S) {
      const float4 a = x4[i], b = x4[i + S], c = x4[i + 2 * S], d = x4[i + 3 * S];
      s0 += sq4(a);
      s1 += sq4(b);
      s2 += sq4(c);
      s3 += sq4(d);
    }
    // (the k-th leftover float4 of a lane goes to accumulator k: no accumulator takes more than four float4 sums)
    if (i < n4) s0 += sq4(x4[i]);
    if (i + S < n4) s1 += sq4(x4[i + S]);
    if (i + 2 * S < n4) s2 += sq4(x4[i + 2 * S]);
    const int tail0 = head + (n4 << 2);
    if (tid < head) s3 += x[tid] * x[tid];
    if (tail0 + tid < len) s2 += x[tail0 + tid] * x[tail0 + tid];
  }
  const float s = wave_sum((s0 + s1) + (s2 + s3));
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per segment.  Lane l adds the segment's partials l, l + 64, ... in f64, then the butterfly: a fixed order.
//   c = coef ? *coef : 1;  c == 0: the loss scaler skipped this step on the device -- last[slot] = 0, nothing is added, steps_skipped + 1
//   else v = c * (float)sqrt(sum); v not finite: last[slot] = 0, nonfinite_values + 1; else last[slot] = v, acc[slot] += (double)v
// counters = {steps_added, steps_skipped, nonfinite_values}; the first two are written by lane 0 of wave 0 of workgroup 0 alone.
__global__ __launch_bounds__(SEGNORM_THREADS) void segnorm_finish_kernel(const tad_segnorm_seg* __restrict__ seg, int nseg, int nwork,
                                                                        const float* __restrict__ partial, const float* __restrict__ coef,
                                                                        double* __restrict__ acc, float* __restrict__ last,
                                                                        int32_t* __restrict__ counters, int nslots) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * (SEGNORM_THREADS / WAVE) + (threadIdx.x >> 6);
  const float c = coef ? *coef : 1.0f;
  const bool skipped = c == 0.0f;
  if (s == 0 && lane == 0) counters[skipped ? 1 : 0] += 1;
  if (s >= nseg) return;  // (whole waves: no barrier follows)
  const int slot = seg[s].slot;
  int w0 = seg[s].first_work, w1 = s + 1 < nseg ? seg[s + 1].first_work : nwork;
  w0 = w0 < 0 ? 0 : w0;
  w1 = w1 > nwork ? nwork : w1;
  if (slot < 0 || slot >= nslots) return;
  double sum = 0.0;
  if (!skipped)
    for (int i = w0 + lane; i < w1; i += WAVE) sum += (double)partial[i];
  sum = wave_sum_f64(sum);
  if (lane != 0) return;
  if (skipped) {
    last[slot] = 0.0f;
    return;
  }
  const float v = c * (float)sqrt(sum);
  if (!(fabsf(v) < INFINITY)) {  // inf or NaN
    last[slot] = 0.0f;
    atomicAdd(&counters[2], 1);
  } else {
    last[slot] = v;
    acc[slot] += (double)v;
  }
}

TAD_NAMESPACE_END

using namespace tad;

extern "C" size_t tad_grad_segnorm_workspace_bytes(int nwork) { return nwork > 0 ? (size_t)nwork * sizeof(float) : 0; }

extern "C" int tad_grad_segnorm_plan_check(const tad_segnorm_seg* table_host, int nseg, const tad_segnorm_work* work_host, int nwork, int64_t n,
                                           int nslots) {
  const char* who = "grad_segnorm_plan_check";
  TAD_REQUIRE(table_host && work_host, "%s: null pointer", who);
  TAD_REQUIRE(nseg > 0 && nwork >= nseg && n > 0 && nslots > 0, "%s: nseg=%d nwork=%d n=%lld nslots=%d: need 1 <= nseg <= nwork, n > 0, nslots > 0",
              who, nseg, nwork, (long long)n, nslots);
  std::vector<bool> used((size_t)nslots, false);
  int w = 0;
  for (int s = 0; s < nseg; ++s) {
    const tad_segnorm_seg& g = table_host[s];
    TAD_REQUIRE(g.length > 0, "%s: segment %d: length %lld must be positive", who, s, (long long)g.length);
    TAD_REQUIRE(g.offset >= 0 && g.offset <= n - g.length, "%s: segment %d: [%lld, %lld + %lld) is not inside the buffer of %lld floats", who, s,
                (long long)g.offset, (long long)g.offset, (long long)g.length, (long long)n);
    TAD_REQUIRE(g.slot >= 0 && g.slot < nslots, "%s: segment %d: slot %d outside [0, %d)", who, s, g.slot, nslots);
    TAD_REQUIRE(!used[(size_t)g.slot], "%s: segment %d: slot %d has two segments", who, s, g.slot);
    used[(size_t)g.slot] = true;
    TAD_REQUIRE(g.first_work == w, "%s: segment %d: first_work %d, but the work items before it end at %d (items tile the segments in order)",
                who, s, g.first_work, w);
    int64_t at = g.offset;
    const int64_t end = g.offset + g.length;
    while (at < end) {
      TAD_REQUIRE(w < nwork, "%s: segment %d: the work list ends at float %lld of it, %lld short", who, s, (long long)(at - g.offset),
                  (long long)(end - at));
      const tad_segnorm_work& k = work_host[w];
      TAD_REQUIRE(k.length > 0 && k.length <= TAD_SEGNORM_WORK_MAX, "%s: work item %d: length %lld must be in [1, %d]", who, w,
                  (long long)k.length, TAD_SEGNORM_WORK_MAX);
      TAD_REQUIRE(k.offset == at, "%s: work item %d: starts at %lld, expected %lld (items tile segment %d exactly once, in order)", who, w,
                  (long long)k.offset, (long long)at, s);
      TAD_REQUIRE(k.length <= end - at, "%s: work item %d: ends %lld floats behind segment %d", who, w, (long long)(k.length - (end - at)), s);
      at += k.length;
      ++w;
    }
  }
  TAD_REQUIRE(w == nwork, "%s: %d work items behind the last segment", who, nwork - w);
  return TAD_OK;
}

extern "C" int tad_grad_segnorm(const float* grad, int64_t n, const tad_segnorm_seg* table, int nseg, const tad_segnorm_work* work, int nwork,
                                const float* coef, double* acc, float* last, int32_t* counters, int nslots, void* ws, size_t ws_bytes,
                                tad_stream_t stream) {
  TAD_REQUIRE(grad && table && work && acc && last && counters && ws, "grad_segnorm: null pointer");
  TAD_REQUIRE(n > 0 && nseg > 0 && nwork >= nseg && nslots > 0, "grad_segnorm: n=%lld nseg=%d nwork=%d nslots=%d", (long long)n, nseg, nwork,
              nslots);
  TAD_REQUIRE(ws_bytes >= tad_grad_segnorm_workspace_bytes(nwork), "grad_segnorm: workspace of %zu bytes, need %zu", ws_bytes,
              tad_grad_segnorm_workspace_bytes(nwork));
  TAD_REQUIRE_ALIGNED("grad_segnorm", grad, 4);
  TAD_REQUIRE_ALIGNED("grad_segnorm", ws, 4);
  TAD_REQUIRE_ALIGNED("grad_segnorm", last, 4);
  TAD_REQUIRE_ALIGNED("grad_segnorm", counters, 4);
  TAD_REQUIRE_ALIGNED("grad_segnorm", table, 8);
  TAD_REQUIRE_ALIGNED("grad_segnorm", work, 8);
  TAD_REQUIRE_ALIGNED("grad_segnorm", acc, 8);
  hipStream_t st = (hipStream_t)stream;
  float* partial = static_cast<float*>(ws);
  hipLaunchKernelGGL(segnorm_reduce_kernel, dim3((unsigned)nwork), dim3(SEGNORM_THREADS), 0, st, grad, n, work, partial);
  constexpr int per = SEGNORM_THREADS / WAVE;
  hipLaunchKernelGGL(segnorm_finish_kernel, dim3((unsigned)((nseg + per - 1) / per)), dim3(SEGNORM_THREADS), 0, st, table, nseg, nwork,
                     (const float*)partial, coef, acc, last, counters, nslots);
  return check_launch("grad_segnorm");
}
