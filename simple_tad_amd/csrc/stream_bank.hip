// Ragged ingest for a bank of camera streams: the stream-bank ABI of include/tad_mi355x_bank.h (tadb_*), the ONE source of
// libtad_mi355x_bank.so.
//   ingest_frames   K decoded uint8 frames of K different sizes, packed in one buffer, each resized to S_h x S_w (the loader's
//                   cv2.resize(frame, (S_w, S_h), INTER_CUBIC), run_inference.py:76,91) and written to a slot of its own in a frame store
//                   [F, S_h, S_w, 3] -- one launch for a tick of a whole fleet, where tad_frame_resize takes one source size and writes
//                   one contiguous output per call.
// The arithmetic is tad_frame_resize's under TAD_FR_NONE, restated here (frame_resize.hip and its object are not touched): host-stated
// taps and 11-bit coefficients, taps clamped to the source, two int32 passes with nothing rounded in between,
//   h[row][d] = sum_j src[row][tap_j] * kx[d][j];      byte = clip((sum_j h[tap_j][d] * ky[r][j] + (1 << 21)) >> 22, 0, 255)
// All of it is integer: the bits are the same whatever the compiler does with floating point.
//
// Shape: that kernel's, with everything that was the call's now the row's.  A workgroup of 256 threads owns FRAME_TR x FRAME_TC outputs
// of one frame (frame_io.h): blockIdx.y is the frame, blockIdx.x the tile -- every frame has the same S_h x S_w outputs, so the grid is
// rectangular although the sources are not.  The workgroup reads its row of the table once (one address: scalar loads), stages the
// tile's taps and coefficients in LDS, runs the horizontal pass over the source rows under the tile's vertical taps into int32 LDS planes
// and the vertical pass out of LDS.  The source rows are held densely (slot = row - lowest row) when the tile's taps span at most four
// rows per output row, and as four slots per output row otherwise, so only rows under taps are ever read.  The four pixels under an
// output's horizontal taps are 12 contiguous bytes at no particular alignment: they come in as the aligned words that hold them and a
// funnel shift; where a tap clamps at a border, byte by byte.  Frames start on multiples of 4 in a 4-byte aligned buffer, so those words
// never begin before their frame, and end at most 3 bytes behind it (the header's slack); what they hold beyond the 12 bytes is shifted
// out.  A thread's outputs in the vertical pass are four neighbouring columns, written by store_frames_u8x4 (frame_io.h).
//
// A malformed table is never an address: the row's extents and its frame's place in src are checked by the workgroup before anything is
// loaded (a row that fails is skipped), the slot is clamped into the store, the set indices into the sets, `first` into a range that
// cannot overflow, and every tap into the row's own w or h.
//
// The library is self-contained: built with -fvisibility=hidden (simple_tad_amd/build.py), it defines the error text and the launch
// check that common.h declares for itself and exports the tadb_* entry points alone.
#include <stdarg.h>
#include <stdlib.h>
#include "frame_io.h"
#pragma GCC visibility push(default)
#include "../../include/tad_mi355x_bank.h"
#pragma GCC visibility pop

namespace tad {

static thread_local char g_bank_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_bank_err, sizeof(g_bank_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return TAD_ELAUNCH;
  }
  return TAD_OK;
}

}  // namespace tad

TAD_NAMESPACE_BEGIN

constexpr int SB_SLOTS = 4 * FRAME_TR;  // source rows a tile can need: four taps per output row
static_assert(SB_SLOTS * 3 * FRAME_TC * 4 + (FRAME_TC + FRAME_TR) * 5 * 4 <= 64 * 1024, "static LDS stays at or below 64 KB");

__host__ __device__ __forceinline__ int64_t sb_set_words(int out) { return TAD_FR_SET_HEAD + (int64_t)out * 5; }
__host__ __device__ __forceinline__ int64_t sb_table_words(int K, int nh, int nv, int Sh, int Sw) {
  return (int64_t)K * TADB_ROW_WORDS + nh * sb_set_words(Sw) + nv * sb_set_words(Sh);
}

// the 12 bytes from p (any alignment) as three words: aligned 4-byte loads and a funnel shift.  Only the aligned words that hold one of
// the 12 bytes are loaded -- three when p is aligned, else four
__device__ __forceinline__ void sb_load12(const uint8_t* p, uint32_t w[3]) {
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
  const uint32_t* q = static_cast<const uint32_t*>(__builtin_assume_aligned(p - sh, 4));  // (derived from p: stays a global pointer)
  const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = sh ? q[3] : 0u;
  w[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
  w[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
  w[2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
}

// first tap and coefficients of `n` outputs from output `o0` of a set, staged in LDS (slots past n: tap 0, coefficients 0).  `first`
// is cut to [-4, TADB_MAX_EXTENT]: first + 3 cannot overflow, and a stated tap range is [-2, in - 2], far inside
__device__ __forceinline__ void sb_stage(const int32_t* __restrict__ set, int out_size, int o0, int n, int* first, int (*kk)[4], int slots) {
  const int32_t* f = set + TAD_FR_SET_HEAD;
  const int32_t* k = f + out_size;
  for (int i = threadIdx.x; i < slots * 5; i += FRAME_THREADS) {
    const int o = i / 5, j = i - o * 5;
    if (j == 4)
      first[o] = o < n ? frame_clamp(f[o0 + o], -4, TADB_MAX_EXTENT) : 0;
    else
      kk[o][j] = o < n ? k[(int64_t)(o0 + o) * 4 + j] : 0;
  }
}

__global__ __launch_bounds__(FRAME_THREADS) void ingest_frames_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                  uint8_t* __restrict__ store, int64_t F,
                                                                  const int32_t* __restrict__ tab, int K, int nh, int nv, int Sh, int Sw,
                                                                  int tiles_x) {
  __shared__ __attribute__((aligned(16))) int hp[SB_SLOTS][3][FRAME_TC];  // (read back four columns at a time)
  __shared__ int hf[FRAME_TC], hk[FRAME_TC][4], vf[FRAME_TR], vk[FRAME_TR][4];
  // the row, read once per workgroup (blockIdx.y < K: the launcher's grid)
  const int32_t* r = tab + (int64_t)blockIdx.y * TADB_ROW_WORDS;
  const int64_t off = (int64_t)r[0];
  const int H = r[1], W = r[2];
  // a row that is no frame inside src is skipped (the same for every thread of the workgroup): nothing below forms an address from it
  if (H < 1 || W < 1 || H > TADB_MAX_EXTENT || W > TADB_MAX_EXTENT || off < 0) return;
  if (off > src_bytes || (int64_t)H * W * 3 > src_bytes - off) return;
  const int64_t slot = r[3] < 0 ? 0 : ((int64_t)r[3] >= F ? F - 1 : (int64_t)r[3]);
  const int32_t* hset = tab + (int64_t)K * TADB_ROW_WORDS + frame_clamp(r[4], 0, nh - 1) * sb_set_words(Sw);
  const int32_t* vset = tab + (int64_t)K * TADB_ROW_WORDS + nh * sb_set_words(Sw) + frame_clamp(r[5], 0, nv - 1) * sb_set_words(Sh);
  const bool swap = (r[6] & TADB_SWAP_RB) != 0;
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int c0 = tx * FRAME_TC, o0 = ty * FRAME_TR;
  const int nc = Sw - c0 < FRAME_TC ? Sw - c0 : FRAME_TC, nr = Sh - o0 < FRAME_TR ? Sh - o0 : FRAME_TR;
  sb_stage(hset, Sw, c0, nc, hf, hk, FRAME_TC);
  sb_stage(vset, Sh, o0, nr, vf, vk, FRAME_TR);
  __syncthreads();

  // the source rows under the tile's vertical taps: [lo, hi], held densely when that is no more rows than four per output row
  int lo = H - 1, hi = 0;
  for (int i = 0; i < nr; ++i) {
    const int a = frame_clamp(vf[i], 0, H - 1), b = frame_clamp(vf[i] + 3, 0, H - 1);
    lo = a < lo ? a : lo, hi = b > hi ? b : hi;
  }
  const bool dense = hi - lo + 1 <= 4 * nr;
  const int nslots = dense ? hi - lo + 1 : 4 * nr;

  // horizontal pass: an item is one column of one source row, all three channels; a thread keeps its column and walks the rows
  const uint8_t* frame = src + off;
  {
    const int c = tid & (FRAME_TC - 1);
    if (c < nc) {
      const int f0 = hf[c];
      const int kq[4] = {hk[c][0], hk[c][1], hk[c][2], hk[c][3]};
      const bool inside = f0 >= 0 && f0 + 3 <= W - 1;  // no tap clamps: the four pixels are 12 contiguous bytes of the row
      for (int s = tid / FRAME_TC; s < nslots; s += FRAME_THREADS / FRAME_TC) {
        const int v = dense ? lo + s : frame_clamp(vf[s >> 2] + (s & 3), 0, H - 1);
        const uint8_t* row = frame + (int64_t)v * W * 3;  // (lo .. hi and the clamp: 0 <= v <= H - 1)
        int acc[3] = {0, 0, 0};
        if (inside) {
          uint32_t w[3];
          sb_load12(row + (int64_t)f0 * 3, w);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] += (int)((w[(3 * j + ch) >> 2] >> (((3 * j + ch) & 3) * 8)) & 255u) * kq[j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint8_t* p = row + (int64_t)frame_clamp(f0 + j, 0, W - 1) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] += (int)p[ch] * kq[j];
          }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) hp[s][ch][c] = acc[ch];
      }
    }
  }
  __syncthreads();

  // vertical pass: a thread owns four columns of one output row, all three channels
  const int orow = tid / FRAME_CG, cg = tid - orow * FRAME_CG;
  const int col = c0 + cg * 4, valid = Sw - col < 4 ? Sw - col : 4;
  if (orow >= nr || valid <= 0) return;
  int acc[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[ch][q] = 1 << 21;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int v = frame_clamp(vf[orow] + j, 0, H - 1);
    const int s = frame_clamp(dense ? v - lo : orow * 4 + j, 0, SB_SLOTS - 1);
    const int k = vk[orow][j];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int4 h = *reinterpret_cast<const int4*>(&hp[s][ch][cg * 4]);
      acc[ch][0] += h.x * k, acc[ch][1] += h.y * k, acc[ch][2] += h.z * k, acc[ch][3] += h.w * k;
    }
  }
  if (swap) {  // the stored channel order: a swapped row puts source channel 2 where channel 0 goes (the flag is the workgroup's)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = acc[0][q];
      acc[0][q] = acc[2][q], acc[2][q] = t;
    }
  }
  const int oy = o0 + orow;
  store_frames_u8x4(store + (((int64_t)slot * Sh + oy) * Sw + col) * 3, acc, valid);
}

TAD_NAMESPACE_END

using namespace tad;

static int sb_shape_ok(const char* who, int K, int nh, int nv, int64_t src_bytes, int64_t F, int Sh, int Sw) {
  TAD_REQUIRE(K >= 1 && K <= TADB_MAX_FRAMES, "%s: K=%d must be in [1, %d]", who, K, TADB_MAX_FRAMES);
  TAD_REQUIRE(nh >= 1 && nh <= TADB_MAX_SETS, "%s: n_hsets=%d must be in [1, %d]", who, nh, TADB_MAX_SETS);
  TAD_REQUIRE(nv >= 1 && nv <= TADB_MAX_SETS, "%s: n_vsets=%d must be in [1, %d]", who, nv, TADB_MAX_SETS);
  TAD_REQUIRE(Sh >= 1 && Sh <= 16384, "%s: S_h=%d must be in [1, 16384]", who, Sh);
  TAD_REQUIRE(Sw >= 1 && Sw <= 16384, "%s: S_w=%d must be in [1, 16384]", who, Sw);
  TAD_REQUIRE(F >= 1 && F <= ((int64_t)1 << 31), "%s: F=%lld must be in [1, 2^31]", who, (long long)F);
  TAD_REQUIRE(src_bytes >= 1, "%s: src_bytes=%lld must be positive", who, (long long)src_bytes);
  return TAD_OK;
}

static int sb_cmp_i64(const void* a, const void* b) {
  const int64_t x = *static_cast<const int64_t*>(a), y = *static_cast<const int64_t*>(b);
  return x < y ? -1 : (x > y ? 1 : 0);
}

static int sb_check_set(const int32_t* set, int out_size, const char* axis, int index) {
  const int in = set[0];
  TAD_REQUIRE(in >= 1 && in <= TADB_MAX_EXTENT, "ingest_plan_check: %s set %d: input extent %d outside [1, %d]", axis, index, in, TADB_MAX_EXTENT);
  TAD_REQUIRE(set[1] == out_size, "ingest_plan_check: %s set %d: output extent %d, expected %d", axis, index, set[1], out_size);
  const int32_t* f = set + TAD_FR_SET_HEAD;
  const int32_t* k = f + out_size;
  for (int o = 0; o < out_size; ++o) {
    TAD_REQUIRE(f[o] >= -2 && f[o] <= in - 2, "ingest_plan_check: %s set %d: output %d has its first tap at %d, outside [-2, %d] (the %d samples of the source)",
                axis, index, o, f[o], in - 2, in);
    int64_t mag = 0;
    for (int j = 0; j < 4; ++j) mag += k[4 * o + j] < 0 ? -(int64_t)k[4 * o + j] : (int64_t)k[4 * o + j];
    TAD_REQUIRE(mag <= TAD_FR_MAX_ABS_SUM, "ingest_plan_check: %s set %d: output %d: sum |k| = %lld is above %d (the int32 passes would overflow)",
                axis, index, o, (long long)mag, TAD_FR_MAX_ABS_SUM);
  }
  return TAD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int tadb_abi_version(void) { return TADB_ABI_VERSION; }

const char* tadb_last_error_string(void) { return tad::g_bank_err; }

int tadb_ingest_plan_check(const int32_t* table_host, int64_t n_words, int K, int n_hsets, int n_vsets, int64_t src_bytes, int64_t F,
                           int S_h, int S_w) {
  TAD_REQUIRE(table_host, "ingest_plan_check: table_host is null");
  if (int rc = sb_shape_ok("ingest_plan_check", K, n_hsets, n_vsets, src_bytes, F, S_h, S_w)) return rc;
  const int64_t want = sb_table_words(K, n_hsets, n_vsets, S_h, S_w);
  TAD_REQUIRE(n_words == want, "ingest_plan_check: n_words=%lld, expected K * %d + the sets = %lld", (long long)n_words, TADB_ROW_WORDS,
              (long long)want);
  const int32_t* hsets = table_host + (int64_t)K * TADB_ROW_WORDS;
  const int32_t* vsets = hsets + n_hsets * sb_set_words(S_w);
  for (int i = 0; i < n_hsets; ++i)
    if (int rc = sb_check_set(hsets + i * sb_set_words(S_w), S_w, "horizontal", i)) return rc;
  for (int i = 0; i < n_vsets; ++i)
    if (int rc = sb_check_set(vsets + i * sb_set_words(S_h), S_h, "vertical", i)) return rc;
  int64_t slots[TADB_MAX_FRAMES];  // slot * TADB_MAX_FRAMES + row, sorted below: two rows of one slot end up next to each other (32 KB of stack)
  for (int k = 0; k < K; ++k) {
    const int32_t* r = table_host + (int64_t)k * TADB_ROW_WORDS;
    const int64_t off = r[0];
    const int h = r[1], w = r[2], slot = r[3], hs = r[4], vs = r[5];
    TAD_REQUIRE(h >= 1 && h <= TADB_MAX_EXTENT, "ingest_plan_check: row %d: h=%d outside [1, %d]", k, h, TADB_MAX_EXTENT);
    TAD_REQUIRE(w >= 1 && w <= TADB_MAX_EXTENT, "ingest_plan_check: row %d: w=%d outside [1, %d]", k, w, TADB_MAX_EXTENT);
    TAD_REQUIRE(off >= 0 && (off & 3) == 0, "ingest_plan_check: row %d: src_off=%lld must be a non-negative multiple of 4", k, (long long)off);
    TAD_REQUIRE(off <= src_bytes && (int64_t)h * w * 3 <= src_bytes - off,
                "ingest_plan_check: row %d: the frame's bytes [%lld, %lld) are not inside src_bytes=%lld", k, (long long)off,
                (long long)(off + (int64_t)h * w * 3), (long long)src_bytes);
    TAD_REQUIRE(slot >= 0 && (int64_t)slot < F, "ingest_plan_check: row %d: slot=%d outside the store [0, F=%lld)", k, slot, (long long)F);
    TAD_REQUIRE(hs >= 0 && hs < n_hsets, "ingest_plan_check: row %d: hset=%d outside [0, %d)", k, hs, n_hsets);
    TAD_REQUIRE(vs >= 0 && vs < n_vsets, "ingest_plan_check: row %d: vset=%d outside [0, %d)", k, vs, n_vsets);
    TAD_REQUIRE(hsets[hs * sb_set_words(S_w)] == w, "ingest_plan_check: row %d: its hset %d is stated for %d columns, the frame has w=%d", k, hs,
                hsets[hs * sb_set_words(S_w)], w);
    TAD_REQUIRE(vsets[vs * sb_set_words(S_h)] == h, "ingest_plan_check: row %d: its vset %d is stated for %d rows, the frame has h=%d", k, vs,
                vsets[vs * sb_set_words(S_h)], h);
    TAD_REQUIRE((r[6] & ~TADB_SWAP_RB) == 0, "ingest_plan_check: row %d: flags=0x%x holds unknown bits", k, (unsigned)r[6]);
    TAD_REQUIRE(r[7] == 0, "ingest_plan_check: row %d: word 7 is %d, it must be 0", k, r[7]);
    slots[k] = (int64_t)slot * TADB_MAX_FRAMES + k;
  }
  qsort(slots, (size_t)K, sizeof(int64_t), sb_cmp_i64);  // (C's: a std::sort would put its template instances into the export table)
  for (int k = 1; k < K; ++k)
    TAD_REQUIRE(slots[k] / TADB_MAX_FRAMES != slots[k - 1] / TADB_MAX_FRAMES, "ingest_plan_check: row %d: slot=%lld is already named by row %d",
                (int)(slots[k] % TADB_MAX_FRAMES), (long long)(slots[k] / TADB_MAX_FRAMES), (int)(slots[k - 1] % TADB_MAX_FRAMES));
  return TAD_OK;
}

int tadb_ingest_frames(const uint8_t* src, int64_t src_bytes, uint8_t* store, int64_t F, const int32_t* table, int64_t n_words, int K,
                       int n_hsets, int n_vsets, int S_h, int S_w, tad_stream_t stream) {
  TAD_REQUIRE(src, "ingest_frames: src is null");
  TAD_REQUIRE(store, "ingest_frames: store is null");
  TAD_REQUIRE(table, "ingest_frames: table is null");
  if (int rc = sb_shape_ok("ingest_frames", K, n_hsets, n_vsets, src_bytes, F, S_h, S_w)) return rc;
  const int64_t want = sb_table_words(K, n_hsets, n_vsets, S_h, S_w);
  TAD_REQUIRE(n_words == want, "ingest_frames: n_words=%lld, expected K * %d + the sets = %lld", (long long)n_words, TADB_ROW_WORDS, (long long)want);
  TAD_REQUIRE_ALIGNED("ingest_frames", src, 4);
  TAD_REQUIRE_ALIGNED("ingest_frames", table, 4);  // (store: any address)
  int tiles_x;
  const dim3 grid(frame_tile_grid(S_h, S_w, &tiles_x), (unsigned)K);
  hipLaunchKernelGGL(ingest_frames_kernel, grid, dim3(FRAME_THREADS), 0, (hipStream_t)stream, src, src_bytes, store, F, table, K, n_hsets, n_vsets,
                     S_h, S_w, tiles_x);
  return check_launch("ingest_frames");
}

}  // extern "C"
#pragma GCC visibility pop
