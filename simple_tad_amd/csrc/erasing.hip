// RandomErasing on the device (random_erasing.py:109-173 of the reference; the datasets apply it to every normalised clip with
// --reprob 0.25 --remode pixel --recount 1 and max_area 0.1: one box per clip, shared by its frames, fresh normal noise per frame).
//
// tad_erase_clips erases the boxes of a host-drawn table from a contiguous f32 clip batch [B, C, T, H, W] IN PLACE, one launch:
// blockIdx.y = box (a table row), the workgroups of a box stride over its items.  The kernel stores the elements inside the boxes and
// loads nothing of x.  An item is a group of four floats at a 16-byte-aligned ADDRESS of one box row (c, t, y): a group that lies
// inside [x0, x1) is one 16-byte store, a group cut by a box edge (or by a later box, below) 4-byte stores of its inside components.
// Groups follow the address, not W, so a clip whose rows start at any alignment (W % 4 != 0, a base offset by one float) takes the
// same path; a value is a function of its coordinates alone, so both kinds of store write the same bits.
//
// Overlap.  The reference writes the boxes of a clip one after the other, so where two overlap the LAST one's values stay.  A box here
// leaves out every element that a later valid row of the same sample covers: each element is written once, by one thread, whatever
// the grid.  The later rows that intersect a box are found once per workgroup (for the recipe's one box per clip: none).
//
// Noise: THE definition (include/tad_mi355x.h carries the same text; tests/erasing_recipe.py restates it in float64).  The reference
// draws torch.empty((C, h, w)).normal_() on the CPU once per frame; that stream cannot be reproduced here, so the value of an element
// is a counter-based function of (seed, sample, box, c, t, dy, dx), box = the row's index in the table, dy = y - y0, dx = x - x0
// (y0, x0 after the cut to the clip), built on hash32 of common.h (the hash of the attention dropout mask):
//   k  = hash32(dy, dx, hash32(c, t, hash32(sample, box, seed)))       pixel: one value per element
//   k  = hash32(0, 0, hash32(c, t, hash32(sample, box, seed)))         rand: one value per (box, frame, channel)
//   k2 = hash32(0, 0, k + 0x6A09E667)
//   u1 = ((k >> 8) + 1) * 2^-24 in (0, 1],  u2 = (k2 >> 8) * 2^-24 in [0, 1)
//   value = sqrtf(-2 * logf(u1)) * cospif(2 * u2)                      Box-Muller with the accurate functions; |value| <= 5.77
//   const: 0.0f.
#include "common.h"
#include <math.h>

TAD_NAMESPACE_BEGIN

constexpr int ERASE_THREADS = 256;
constexpr int ERASE_MAX_BLOCKS = 256 * 8;  // Guideline 11: a capped grid (8 workgroups per CU) that strides, as MIX_MAX_BLOCKS

struct EraseBox {  // one row of the box table (TAD_ERASE_BOX_WORDS int32)
  int sample, mode;
  int t0, t1, y0, y1, x0, x1;
};
static_assert(sizeof(EraseBox) == 4 * TAD_ERASE_BOX_WORDS, "box row layout");

__host__ __device__ __forceinline__ int erase_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the row as the kernel uses it: cut to the clip; an unknown mode, a sample outside the batch or an empty box gives mode -1 = nothing to
// do (a malformed table is never an address)
__device__ __forceinline__ EraseBox load_box(const int32_t* boxes, int k, int B, int T, int H, int W) {
  EraseBox b = *reinterpret_cast<const EraseBox*>(boxes + (int64_t)k * TAD_ERASE_BOX_WORDS);
  b.t0 = erase_clamp(b.t0, 0, T), b.t1 = erase_clamp(b.t1, b.t0, T);
  b.y0 = erase_clamp(b.y0, 0, H), b.y1 = erase_clamp(b.y1, b.y0, H);
  b.x0 = erase_clamp(b.x0, 0, W), b.x1 = erase_clamp(b.x1, b.x0, W);
  const bool known = b.mode == TAD_ERASE_CONST || b.mode == TAD_ERASE_RAND || b.mode == TAD_ERASE_PIXEL;
  if (!known || b.sample < 0 || b.sample >= B || b.t0 == b.t1 || b.y0 == b.y1 || b.x0 == b.x1) b.mode = -1;
  return b;
}

__device__ __forceinline__ float erase_normal(uint32_t k) {
  const uint32_t k2 = hash32(0u, 0u, k + 0x6A09E667u);
  const float u1 = (float)((k >> 8) + 1u) * 0x1p-24f, u2 = (float)(k2 >> 8) * 0x1p-24f;
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

__global__ __launch_bounds__(ERASE_THREADS) void erase_clips_kernel(float* __restrict__ x, const int32_t* __restrict__ boxes, int n_boxes,
                                                                    uint32_t seed, int B, int C, int T, int H, int W) {
  const int box = blockIdx.y;
  const EraseBox b = load_box(boxes, box, B, T, H, W);
  if (b.mode < 0) return;  // (the same for every thread of the workgroup)
  // later rows of the same sample that intersect this box: [later_lo, later_hi) holds them all (and, in a table that is not sorted by
  // sample, rows of other samples, which the per-element test skips)
  __shared__ int later_lo, later_hi;
  if (threadIdx.x == 0) later_lo = n_boxes, later_hi = 0;
  __syncthreads();
  for (int k = box + 1 + threadIdx.x; k < n_boxes; k += ERASE_THREADS) {
    const EraseBox l = load_box(boxes, k, B, T, H, W);
    if (l.mode >= 0 && l.sample == b.sample && l.t0 < b.t1 && b.t0 < l.t1 && l.y0 < b.y1 && b.y0 < l.y1 && l.x0 < b.x1 && b.x0 < l.x1) {
      atomicMin(&later_lo, k);
      atomicMax(&later_hi, k + 1);
    }
  }
  __syncthreads();
  const int k_lo = later_lo, k_hi = later_hi;

  const int64_t n = (int64_t)C * T * H * W;  // (elements of a sample; the host checks n < 2^31)
  float* xs = x + (int64_t)b.sample * n;
  const int dt = b.t1 - b.t0, dy = b.y1 - b.y0, w = b.x1 - b.x0;
  const uint32_t groups = (uint32_t)(w + 3) / 4u + 1u;  // 16-byte groups a row of w floats can touch at any alignment
  const uint32_t rows = (uint32_t)C * dt * dy;
  const uint64_t items = (uint64_t)rows * groups;       // (<= C * T * H * max(W, 2) < 2^32)
  const uint32_t key_box = hash32((uint32_t)b.sample, (uint32_t)box, seed);
  const uint64_t stride = (uint64_t)gridDim.x * ERASE_THREADS;
  for (uint64_t it = (uint64_t)blockIdx.x * ERASE_THREADS + threadIdx.x; it < items; it += stride) {
    const uint32_t i = (uint32_t)it;
    const uint32_t g = i % groups, r = i / groups;
    const int yy = (int)(r % (uint32_t)dy), r2 = (int)(r / (uint32_t)dy);
    const int tt = r2 % dt, c = r2 / dt;
    const int t = b.t0 + tt, y = b.y0 + yy;
    float* row = xs + (((int64_t)c * T + t) * H + y) * W;  // element (c, t, y, 0)
    // first element of group g: the 16-byte-aligned address at or below row + x0, plus 4 g floats
    const int lead = (int)((reinterpret_cast<uintptr_t>(row + b.x0) >> 2) & 3);
    const int xg = b.x0 - lead + 4 * (int)g;
    if (xg >= b.x1) continue;  // (the spare group of a row that needs one fewer)
    const uint32_t key_row = hash32((uint32_t)c, (uint32_t)t, key_box);
    const float flat = b.mode == TAD_ERASE_RAND ? erase_normal(hash32(0u, 0u, key_row)) : 0.0f;
    f32x4 v;
    bool inside[4];
    bool all = true;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int xx = xg + e;
      bool in = xx >= b.x0 && xx < b.x1;
      for (int k = k_lo; in && k < k_hi; ++k) {  // last box wins: a later row of this sample that covers the element writes it
        const EraseBox l = load_box(boxes, k, B, T, H, W);
        if (l.mode >= 0 && l.sample == b.sample && t >= l.t0 && t < l.t1 && y >= l.y0 && y < l.y1 && xx >= l.x0 && xx < l.x1) in = false;
      }
      inside[e] = in;
      all = all && in;
      v[e] = (in && b.mode == TAD_ERASE_PIXEL) ? erase_normal(hash32((uint32_t)yy, (uint32_t)(xx - b.x0), key_row)) : flat;
    }
    if (all) {
      *reinterpret_cast<f32x4*>(row + xg) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (inside[e]) row[xg + e] = v[e];
    }
  }
}

TAD_NAMESPACE_END

using namespace tad;

static int erase_shape_ok(int n_boxes, int B, int C, int T, int H, int W, const char* who) {
  TAD_REQUIRE(n_boxes >= 0 && n_boxes <= TAD_ERASE_MAX_BOXES, "%s: n_boxes=%d must be in [0, %d]", who, n_boxes, TAD_ERASE_MAX_BOXES);
  TAD_REQUIRE(B > 0 && C > 0 && T > 0 && H > 0 && W > 0, "%s: B=%d C=%d T=%d H=%d W=%d must be positive", who, B, C, T, H, W);
  TAD_REQUIRE((int64_t)C * T * H * W < ((int64_t)1 << 31), "%s: a sample of C*T*H*W=%lld elements exceeds 2^31-1", who,
              (long long)((int64_t)C * T * H * W));
  return TAD_OK;
}

extern "C" int tad_erase_plan_check(const int32_t* boxes_host, int n_boxes, int B, int T, int H, int W) {
  TAD_REQUIRE(boxes_host, "erase_plan_check: null pointer");
  if (int rc = erase_shape_ok(n_boxes, B, 1, T, H, W, "erase_plan_check")) return rc;
  for (int k = 0; k < n_boxes; ++k) {
    const EraseBox* b = reinterpret_cast<const EraseBox*>(boxes_host + (int64_t)k * TAD_ERASE_BOX_WORDS);
    TAD_REQUIRE(b->mode == TAD_ERASE_CONST || b->mode == TAD_ERASE_RAND || b->mode == TAD_ERASE_PIXEL, "erase_plan_check: box %d: mode=%d", k,
                b->mode);
    TAD_REQUIRE(0 <= b->sample && b->sample < B, "erase_plan_check: box %d: sample=%d outside the batch B=%d", k, b->sample, B);
    TAD_REQUIRE(0 <= b->t0 && b->t0 <= b->t1 && b->t1 <= T && 0 <= b->y0 && b->y0 <= b->y1 && b->y1 <= H && 0 <= b->x0 && b->x0 <= b->x1 &&
                    b->x1 <= W,
                "erase_plan_check: box %d: t[%d,%d) y[%d,%d) x[%d,%d) outside the clip T=%d H=%d W=%d", k, b->t0, b->t1, b->y0, b->y1, b->x0,
                b->x1, T, H, W);
  }
  return TAD_OK;
}

extern "C" int tad_erase_clips(float* x, const int32_t* boxes, int n_boxes, uint32_t seed, int B, int C, int T, int H, int W,
                               tad_stream_t stream) {
  TAD_REQUIRE(x && boxes, "erase_clips: null pointer");
  if (int rc = erase_shape_ok(n_boxes, B, C, T, H, W, "erase_clips")) return rc;
  TAD_REQUIRE(n_boxes >= 1, "erase_clips: n_boxes=%d: a batch without a box launches nothing and is not passed here", n_boxes);
  TAD_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(boxes) & 3) == 0,
              "erase_clips: x and boxes must be 4-byte aligned");
  // the table is on the device, so the grid is sized for the largest box there can be (the whole clip); workgroups past a box's items
  // find nothing to do
  const int64_t groups = (int64_t)C * T * H * ((W + 3) / 4 + 1);
  int64_t gx = (groups + ERASE_THREADS - 1) / ERASE_THREADS;
  const int64_t cap = n_boxes >= ERASE_MAX_BLOCKS ? 1 : ERASE_MAX_BLOCKS / n_boxes;
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL(erase_clips_kernel, dim3((unsigned)gx, (unsigned)n_boxes), dim3(ERASE_THREADS), 0, (hipStream_t)stream, x, boxes,
                     n_boxes, seed, B, C, T, H, W);
  return check_launch("erase_clips");
}
