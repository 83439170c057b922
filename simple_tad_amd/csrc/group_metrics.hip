// Grouped evaluation report (anaysis/metrics_dota.py, metrics_dada.py, metrics_by_categories.py): the counting behind the metrics of up
// to 64 sample groups (TOTAL, accident categories, ego / non-ego, night / day ...) in one pass each.  Sample i carries a bit mask
// member[i]: bit g set = the sample belongs to group g.
//   tad_group_threshold_histogram   metrics.hip's histogram of k(p) = #{t : p >= thr[t]} per label, kept per group: every thresholded
//                                   metric of every group follows from hist[G][2][T+1].
//   tad_group_rank_stats            over the samples in descending score order: P, N, the integer 2 P N AUROC and the fp64 average
//                                   precision of every group (scikit-learn's definitions, tied scores grouped).
// Integer results are exact; the only floating-point sum (AP) runs in a fixed order.  No floating-point atomics anywhere.
#include "common.h"

TAD_NAMESPACE_BEGIN

constexpr int GM_MAX_THR = 255;
constexpr int GM_MAX_GROUPS = 64;
constexpr int GM_GROUP_TILE = 16;     // groups whose counters one block keeps in LDS: 16 x 2 x 256 x 4 B = 32 KiB (all 64: 128 KiB,
                                      // more than a static array may hold) -- the groups are tiled over grid.y
constexpr int GM_CHUNK = 1 << 16;     // samples per block

__global__ __launch_bounds__(256) void group_threshold_hist_kernel(const float* __restrict__ probs, const int32_t* __restrict__ labels,
                                                                   const unsigned long long* __restrict__ member, int G,
                                                                   const float* __restrict__ thr, int T, int64_t n,
                                                                   unsigned long long* __restrict__ hist /*[G][2][T+1]*/) {
  __shared__ float sthr[GM_MAX_THR];
  __shared__ unsigned int sh[GM_GROUP_TILE * 2 * (GM_MAX_THR + 1)];
  const int g0 = blockIdx.y * GM_GROUP_TILE, ng = min(GM_GROUP_TILE, G - g0), row = T + 1;
  for (int i = threadIdx.x; i < T; i += 256) sthr[i] = thr[i];
  for (int i = threadIdx.x; i < ng * 2 * row; i += 256) sh[i] = 0u;
  __syncthreads();
  // a block handles at most GM_CHUNK = 2^16 samples, and a sample adds 1 to at most one counter per group: the 32-bit LDS counters
  // cannot overflow (bounded, not flushed -- as threshold_hist_kernel bounds its blocks)
  const int64_t lo = (int64_t)blockIdx.x * GM_CHUNK, hi = min(n, lo + GM_CHUNK);
  const unsigned int tile_mask = (1u << ng) - 1u;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    unsigned int m = (unsigned int)(member[i] >> g0) & tile_mask;
    if (!m) continue;
    const float p = probs[i];
    int a = 0, b = T;  // first index with thr > p (NaN compares false everywhere: k = 0); found once, used for every group of the sample
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (p >= sthr[mid]) a = mid + 1; else b = mid;
    }
    const int slot = (labels[i] != 0 ? row : 0) + a;
    while (m) {
      const int g = __ffs(m) - 1;
      m &= m - 1;
      atomicAdd(&sh[g * 2 * row + slot], 1u);
    }
  }
  __syncthreads();
  unsigned long long* out = hist + (int64_t)g0 * 2 * row;
  for (int i = threadIdx.x; i < ng * 2 * row; i += 256)
    if (sh[i]) atomicAdd(&out[i], (unsigned long long)sh[i]);
}

// ---- rank statistics: one workgroup per group walks the sorted samples in tiles of GM_RANK_TILE.
// With T(i), F(i) the group's positives / negatives among samples 0..i, and e the run ends (last sample of every run of equal scores):
//   U2 = sum_e (F_e - F_s)(T_e + T_s)          = 2 P N AUROC (trapezoids of the ROC curve, an integer)
//   AP = sum_e (T_e - T_s) / P * T_e / (T_e + F_e)
// where s is the run end before e (T_s = F_s = 0 for the first).  A run in which the group has no member adds 0 to both.
// (T, F) travel packed as T << 32 | F: n < 2^31 keeps the halves apart, a sum of packed values is the packed sum, and since T and F
// never decrease along the array the pair at the LAST run end before a position is the MAXIMUM of the packed pairs at all run ends
// before it -- so "the previous run end" is a block max-scan carried from tile to tile, next to the sum-scan of the counts.
constexpr int GM_RANK_THREADS = 512;
constexpr int GM_RANK_ITEMS = 8;
constexpr int GM_RANK_TILE = GM_RANK_THREADS * GM_RANK_ITEMS;
constexpr int GM_RANK_WAVES = GM_RANK_THREADS / WAVE;
typedef unsigned long long u64;

__device__ __forceinline__ u64 shfl_up_u64(u64 v, int d) {
  const unsigned int lo = __shfl_up((unsigned int)v, d, 64), hi = __shfl_up((unsigned int)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_down_u64(u64 v, int d) {
  const unsigned int lo = __shfl_down((unsigned int)v, d, 64), hi = __shfl_down((unsigned int)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}
// exclusive scan of non-negative values over the block's threads (sum or max; identity 0), `total` = over all threads.
// Two barriers; swave is free again on return.
template <bool MAX>
__device__ __forceinline__ u64 block_scan_exclusive(u64 v, u64* swave, u64& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = shfl_up_u64(inc, d);
    if (lane >= d) inc = MAX ? max(inc, o) : inc + o;
  }
  if (lane == 63) swave[w] = inc;
  __syncthreads();
  u64 base = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < GM_RANK_WAVES; ++k) {
    const u64 s = swave[k];
    if (k < w) base = MAX ? max(base, s) : base + s;
    total = MAX ? max(total, s) : total + s;
  }
  __syncthreads();
  u64 exc = shfl_up_u64(inc, 1);
  if (lane == 0) exc = 0;
  return MAX ? max(base, exc) : base + exc;
}

__global__ __launch_bounds__(GM_RANK_THREADS) void group_rank_stats_kernel(const int32_t* __restrict__ labels, const u64* __restrict__ member,
                                                                           const uint8_t* __restrict__ run_end, int64_t n,
                                                                           long long* __restrict__ out_int /*[G][3]*/,
                                                                           double* __restrict__ out_ap /*[G]*/) {
  __shared__ u64 swave[GM_RANK_WAVES];
  __shared__ double sap[GM_RANK_WAVES];
  const int g = blockIdx.x, tid = threadIdx.x;
  u64 carry = 0;     // (T, F) over all earlier tiles
  u64 prev_end = 0;  // (T, F) at the last run end of all earlier tiles
  long long u2 = 0;  // this thread's share of U2 (an integer sum: any order)
  double ap = 0.0;   // this thread's share of P * AP: its run ends in array order; the shares are added in a fixed tree at the end
  for (int64_t base = 0; base < n; base += GM_RANK_TILE) {
    const int64_t i0 = base + (int64_t)tid * GM_RANK_ITEMS;
    unsigned int pos = 0, neg = 0, ends = 0;  // bit j: item i0 + j is a positive / negative member of the group / a run end
#pragma unroll
    for (int j = 0; j < GM_RANK_ITEMS; ++j) {
      const int64_t i = i0 + j;
      if (i < n) {
        const unsigned int m = (unsigned int)((member[i] >> g) & 1ull), y = labels[i] != 0;
        pos |= (m & y) << j;
        neg |= (m & (y ^ 1u)) << j;
        ends |= (unsigned int)(run_end[i] != 0) << j;
      }
    }
    u64 total, total_end;
    const u64 mine = ((u64)__popc(pos) << 32) | (u64)__popc(neg);
    const u64 before = carry + block_scan_exclusive<false>(mine, swave, total);
    // (T, F) at this thread's last run end (0: none)
    u64 c = before, last_end = 0;
#pragma unroll
    for (int j = 0; j < GM_RANK_ITEMS; ++j) {
      c += ((u64)((pos >> j) & 1u) << 32) | (u64)((neg >> j) & 1u);
      if ((ends >> j) & 1u) last_end = c;
    }
    u64 s = max(prev_end, block_scan_exclusive<true>(last_end, swave, total_end));
    c = before;
#pragma unroll
    for (int j = 0; j < GM_RANK_ITEMS; ++j) {
      c += ((u64)((pos >> j) & 1u) << 32) | (u64)((neg >> j) & 1u);
      if ((ends >> j) & 1u) {
        const long long te = (long long)(c >> 32), fe = (long long)(c & 0xffffffffull);
        const long long ts = (long long)(s >> 32), fs = (long long)(s & 0xffffffffull);
        u2 += (fe - fs) * (te + ts);
        if (te > ts) ap += (double)(te - ts) * (double)te / (double)(te + fe);  // (te - ts) te < 2^62: the product rounds once
        s = c;
      }
    }
    carry += total;
    prev_end = max(prev_end, total_end);
  }
  // block sums: down-shuffle trees inside the waves, then the waves in order
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    u2 += (long long)shfl_down_u64((u64)u2, d);
    ap += __builtin_bit_cast(double, shfl_down_u64(__builtin_bit_cast(u64, ap), d));
  }
  if ((tid & 63) == 0) {
    swave[tid >> 6] = (u64)u2;
    sap[tid >> 6] = ap;
  }
  __syncthreads();
  if (tid == 0) {
    long long u = 0;
    double a = 0.0;
    for (int k = 0; k < GM_RANK_WAVES; ++k) {
      u += (long long)swave[k];
      a += sap[k];
    }
    const long long P = (long long)(carry >> 32), N = (long long)(carry & 0xffffffffull);
    out_int[g * 3 + 0] = P;
    out_int[g * 3 + 1] = N;
    out_int[g * 3 + 2] = u;
    out_ap[g] = P > 0 ? a / (double)P : 0.0;
  }
}

TAD_NAMESPACE_END

using namespace tad;

extern "C" int tad_group_threshold_histogram(const float* probs, const int32_t* labels, const uint64_t* member, int n_groups,
                                             const float* thresholds, int n_thresholds, int64_t n, int64_t* hist, tad_stream_t stream) {
  TAD_REQUIRE(probs && labels && member && thresholds && hist, "group_threshold_histogram: null pointer");
  TAD_REQUIRE(n_groups >= 1 && n_groups <= GM_MAX_GROUPS, "group_threshold_histogram: n_groups=%d, need 1..%d", n_groups, GM_MAX_GROUPS);
  TAD_REQUIRE(n > 0 && n_thresholds > 0 && n_thresholds <= GM_MAX_THR, "group_threshold_histogram: need n > 0 and 1..%d thresholds", GM_MAX_THR);
  const int64_t blocks = (n + GM_CHUNK - 1) / GM_CHUNK;
  TAD_REQUIRE(blocks <= 0x7fffffff, "group_threshold_histogram: n=%lld is too large", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, sizeof(int64_t) * n_groups * 2 * (n_thresholds + 1), st) != hipSuccess) {
    set_error("group_threshold_histogram: memset failed");
    return TAD_EINVAL;
  }
  const dim3 grid((unsigned)blocks, (unsigned)((n_groups + GM_GROUP_TILE - 1) / GM_GROUP_TILE));
  hipLaunchKernelGGL(group_threshold_hist_kernel, grid, dim3(256), 0, st, probs, labels, reinterpret_cast<const unsigned long long*>(member),
                     n_groups, thresholds, n_thresholds, n, reinterpret_cast<unsigned long long*>(hist));
  return check_launch("group_threshold_histogram");
}

static_assert(GM_RANK_TILE == TAD_GROUP_RANK_TILE, "the header states the tile");

extern "C" int tad_group_rank_stats(const int32_t* labels_sorted, const uint64_t* member_sorted, const uint8_t* run_end, int n_groups, int64_t n,
                                    int64_t* out_int, double* out_ap, tad_stream_t stream) {
  TAD_REQUIRE(labels_sorted && member_sorted && run_end && out_int && out_ap, "group_rank_stats: null pointer");
  TAD_REQUIRE(n_groups >= 1 && n_groups <= GM_MAX_GROUPS, "group_rank_stats: n_groups=%d, need 1..%d", n_groups, GM_MAX_GROUPS);
  TAD_REQUIRE(n > 0 && n < ((int64_t)1 << 31), "group_rank_stats: n=%lld, need 1 <= n < 2^31", (long long)n);
  hipLaunchKernelGGL(group_rank_stats_kernel, dim3((unsigned)n_groups), dim3(GM_RANK_THREADS), 0, (hipStream_t)stream, labels_sorted,
                     reinterpret_cast<const u64*>(member_sorted), run_end, n, reinterpret_cast<long long*>(out_int), out_ap);
  return check_launch("group_rank_stats");
}
