// The two-pass 8-bit cubic resize that frame_resize.hip, stream_bank.hip and yuv_ingest.hip share: everything around a kernel's own
// horizontal tap source and its writer.  Nothing here knows which of them includes it.
//
// Arithmetic -- the contract: OpenCV's GENERIC INTEGER formulation of the 8-bit cubic resize.  Per output four taps first .. first + 3,
// each clamped to the source (replicate border), 11-bit coefficients that are NOT renormalised; two passes in int32 with no rounding in
// between:
//   h[row][d] = sum_j src[row][tap_j] * kx[d][j];      byte = clip((sum_j h[tap_j][d] * ky[r][j] + (1 << 21)) >> 22, 0, 255)
// 255 * 2818 * 2818 + 2^21 < 2^31 (sum |k| <= 2818 per output, which cubic_check_set holds a table to).  All of it is integer: the bits
// are the same whatever the compiler does with floating point.
//
// A set (int32 words): {in, out, 0, 0}, first[out], k[out][4] -- cubic_set_words(out) of them.
//
// Shape: a workgroup of FRAME_THREADS threads owns FRAME_TR x FRAME_TC outputs of one frame (frame_io.h) and declares CUBIC_TILE_LDS.
// It stages the tile's taps and coefficients (cubic_stage), finds the source rows under the tile's vertical taps (cubic_span), runs ITS OWN horizontal pass over those rows into the int32 planes hp (one per row and channel), and after a barrier the vertical pass
// out of LDS (cubic_vpass), whose sums it hands to a writer of frame_io.h.  The rows are held densely (slot = row - lowest row) when
// the tile's taps span at most four rows per output row -- upscales and shrinks up to 4 -- and as four slots per output row otherwise,
// so only rows under taps are ever read.  A malformed table is never an address: `first` is cut to [-4, in] when it is staged, so
// first + 3 cannot overflow, and every tap is clamped into [0, in - 1] where it is used.
#pragma once
#include "frame_io.h"
#include <stdlib.h>

TAD_NAMESPACE_BEGIN

constexpr int CUBIC_SLOTS = 4 * FRAME_TR;  // source rows a tile can need: four taps per output row

// a kernel's LDS: the planes hp (read back four columns at a time), and first tap and coefficients of the tile's columns (hf, hk) and
// rows (vf, vk).  Five arrays, not one struct: with one LDS symbol for all five the compiler allocates the registers of every
// kernel differently, to no gain (the code objects were compared both ways)
#define CUBIC_TILE_LDS                                                      \
  __shared__ __attribute__((aligned(16))) int hp[CUBIC_SLOTS][3][FRAME_TC]; \
  __shared__ int hf[FRAME_TC], hk[FRAME_TC][4], vf[FRAME_TR], vk[FRAME_TR][4]
static_assert(CUBIC_SLOTS * 3 * FRAME_TC * 4 + (FRAME_TC + FRAME_TR) * 5 * 4 <= 64 * 1024, "static LDS stays at or below 64 KB");

__host__ __device__ __forceinline__ int64_t cubic_set_words(int out) { return TAD_FR_SET_HEAD + (int64_t)out * 5; }

// first tap and coefficients of `n` outputs from output `o0` of a set, staged in LDS (slots past n: tap 0, coefficients 0).  `in` is the
// extent the taps are later clamped into: with first > in every tap clamps to in - 1, with first < -4 to 0, so the cut changes no byte
__device__ __forceinline__ void cubic_stage(const int32_t* __restrict__ set, int out_size, int o0, int n, int in, int* first, int (*kk)[4],
                                            int slots) {
  const int32_t* f = set + TAD_FR_SET_HEAD;
  const int32_t* k = f + out_size;
  for (int i = threadIdx.x; i < slots * 5; i += FRAME_THREADS) {
    const int o = i / 5, j = i - o * 5;
    if (j == 4)
      first[o] = o < n ? frame_clamp(f[o0 + o], -4, in) : 0;
    else
      kk[o][j] = o < n ? k[(int64_t)(o0 + o) * 4 + j] : 0;
  }
}

// the 12 bytes from p (any alignment) as three words: aligned 4-byte loads and a funnel shift.  Only the aligned words that hold one of
// the 12 bytes are loaded -- three when p is aligned, else four -- so no load leaves the pages of the bytes asked for; the up to three
// bytes to either side that share a word with them are shifted out
__device__ __forceinline__ void cubic_load12(const uint8_t* p, uint32_t w[3]) {
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
  const uint32_t* q = static_cast<const uint32_t*>(__builtin_assume_aligned(p - sh, 4));  // (derived from p: stays a global pointer)
  const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = sh ? q[3] : 0u;
  w[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
  w[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
  w[2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
}

// the source rows [lo, hi] under the vertical taps of the tile's nr output rows (of a source of `in` rows), and how hp holds them
struct CubicSpan {
  int lo, hi, nslots;
  bool dense;
};

__device__ __forceinline__ CubicSpan cubic_span(const int* vf, int nr, int in) {
  int lo = in - 1, hi = 0;
  for (int i = 0; i < nr; ++i) {
    const int a = frame_clamp(vf[i], 0, in - 1), b = frame_clamp(vf[i] + 3, 0, in - 1);
    lo = a < lo ? a : lo, hi = b > hi ? b : hi;
  }
  const bool dense = hi - lo + 1 <= 4 * nr;
  return {lo, hi, dense ? hi - lo + 1 : 4 * nr, dense};
}

// horizontal pass: the source row that slot < nslots of hp holds (0 <= row <= in - 1)
__device__ __forceinline__ int cubic_slot_row(const CubicSpan& sp, const int* vf, int slot, int in) {
  return sp.dense ? sp.lo + slot : frame_clamp(vf[slot >> 2] + (slot & 3), 0, in - 1);
}

// vertical pass: the slot of hp under tap j of output row orow
__device__ __forceinline__ int cubic_tap_slot(const CubicSpan& sp, const int* vf, int orow, int j, int in) {
  const int v = frame_clamp(vf[orow] + j, 0, in - 1);
  return frame_clamp(sp.dense ? v - sp.lo : orow * 4 + j, 0, CUBIC_SLOTS - 1);
}

// the thread's place in the vertical pass: four neighbouring columns from `col` (`valid` of them inside the frame) of tile row orow
struct CubicOut {
  int orow, cg, col, valid;
};

// vertical pass of the tile at column c0 with nr rows: a thread owns four columns of one output row, all three channels.  acc: the
// 22-bit sums, the rounding constant in them; `swap` (the workgroup's) exchanges channels 0 and 2.  False: the thread has no output
__device__ __forceinline__ bool cubic_vpass(const int (*hp)[3][FRAME_TC], const int* vf, const int (*vk)[4], const CubicSpan& sp, int in, int c0,
                                            int nr, int Sw, bool swap, CubicOut& o, int (&acc)[3][4]) {
  const int tid = threadIdx.x;
  o.orow = tid / FRAME_CG, o.cg = tid - o.orow * FRAME_CG;
  o.col = c0 + o.cg * 4, o.valid = Sw - o.col < 4 ? Sw - o.col : 4;
  if (o.orow >= nr || o.valid <= 0) return false;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[ch][q] = 1 << 21;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int slot = cubic_tap_slot(sp, vf, o.orow, j, in);
    const int k = vk[o.orow][j];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int4 h = *reinterpret_cast<const int4*>(&hp[slot][ch][o.cg * 4]);
      acc[ch][0] += h.x * k, acc[ch][1] += h.y * k, acc[ch][2] += h.z * k, acc[ch][3] += h.w * k;
    }
  }
  if (swap) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int s = acc[0][q];
      acc[0][q] = acc[2][q], acc[2][q] = s;
    }
  }
  return true;
}

// ---------------------------------------------------------------- host side: `who` is the plan check's name in its messages
// a set towards out_size outputs: an input extent in [1, max_in], taps next to their source, coefficients the int32 passes can take
static inline int cubic_check_set(const char* who, const int32_t* set, int out_size, const char* axis, int index, int max_in) {
  const int in = set[0];
  TAD_REQUIRE(in >= 1 && in <= max_in, "%s: %s set %d: input extent %d outside [1, %d]", who, axis, index, in, max_in);
  TAD_REQUIRE(set[1] == out_size, "%s: %s set %d: output extent %d, expected %d", who, axis, index, set[1], out_size);
  const int32_t* f = set + TAD_FR_SET_HEAD;
  const int32_t* k = f + out_size;
  for (int o = 0; o < out_size; ++o) {
    // s = first + 1 = floor of a sample position that lies within half a source step of the source: s in [-1, in - 1]
    TAD_REQUIRE(f[o] >= -2 && f[o] <= in - 2, "%s: %s set %d: output %d has its first tap at %d, outside the %d samples of the source (a first tap lies in [-2, %d])",
                who, axis, index, o, f[o], in, in - 2);
    int64_t mag = 0;
    for (int j = 0; j < 4; ++j) mag += k[4 * o + j] < 0 ? -(int64_t)k[4 * o + j] : (int64_t)k[4 * o + j];
    TAD_REQUIRE(mag <= TAD_FR_MAX_ABS_SUM, "%s: %s set %d: output %d: sum |k| = %lld is above %d (the int32 passes would overflow)", who, axis, index, o,
                (long long)mag, TAD_FR_MAX_ABS_SUM);
  }
  return TAD_OK;
}

// The ragged launches (stream_bank.hip, yuv_ingest.hip): K frames of K sizes into K slots of a store [F, S_h, S_w, 3].  Their headers
// state the same limits under their own names; each source asserts that its names say these
constexpr int RAGGED_MAX_FRAMES = 4096, RAGGED_MAX_SETS = 64, RAGGED_MAX_EXTENT = 32768;

static inline int ragged_shape_ok(const char* who, int K, int nh, int nv, int64_t src_bytes, int64_t F, int Sh, int Sw) {
  TAD_REQUIRE(K >= 1 && K <= RAGGED_MAX_FRAMES, "%s: K=%d must be in [1, %d]", who, K, RAGGED_MAX_FRAMES);
  TAD_REQUIRE(nh >= 1 && nh <= RAGGED_MAX_SETS, "%s: n_hsets=%d must be in [1, %d]", who, nh, RAGGED_MAX_SETS);
  TAD_REQUIRE(nv >= 1 && nv <= RAGGED_MAX_SETS, "%s: n_vsets=%d must be in [1, %d]", who, nv, RAGGED_MAX_SETS);
  TAD_REQUIRE(Sh >= 1 && Sh <= 16384, "%s: S_h=%d must be in [1, 16384]", who, Sh);
  TAD_REQUIRE(Sw >= 1 && Sw <= 16384, "%s: S_w=%d must be in [1, 16384]", who, Sw);
  TAD_REQUIRE(F >= 1 && F <= ((int64_t)1 << 31), "%s: F=%lld must be in [1, 2^31]", who, (long long)F);
  TAD_REQUIRE(src_bytes >= 1, "%s: src_bytes=%lld must be positive", who, (long long)src_bytes);
  return TAD_OK;
}

static inline int ragged_cmp_i64(const void* a, const void* b) {
  const int64_t x = *static_cast<const int64_t*>(a), y = *static_cast<const int64_t*>(b);
  return x < y ? -1 : (x > y ? 1 : 0);
}

// "every slot is named once": slots[k] is the slot of row k < K (overwritten).  Sorted as slot * RAGGED_MAX_FRAMES + row, two rows of
// one slot end up next to each other
static inline int ragged_slots_once(const char* who, int64_t* slots, int K) {
  for (int k = 0; k < K; ++k) slots[k] = slots[k] * RAGGED_MAX_FRAMES + k;
  qsort(slots, (size_t)K, sizeof(int64_t), ragged_cmp_i64);  // (C's: a std::sort would put its template instances into the export table)
  for (int k = 1; k < K; ++k)
    TAD_REQUIRE(slots[k] / RAGGED_MAX_FRAMES != slots[k - 1] / RAGGED_MAX_FRAMES, "%s: row %d: slot=%lld is already named by row %d", who,
                (int)(slots[k] % RAGGED_MAX_FRAMES), (long long)(slots[k] / RAGGED_MAX_FRAMES), (int)(slots[k - 1] % RAGGED_MAX_FRAMES));
  return TAD_OK;
}

TAD_NAMESPACE_END
