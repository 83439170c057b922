// Ragged ingest of 4:2:0 YUV camera surfaces: the YUV-ingest ABI of include/tad_mi355x_yuv.h (tady_*), the ONE source of
// libtad_mi355x_yuv.so.
//   ingest_yuv   K pitched NV12 / NV21 / I420 frames of K different sizes, packed in one buffer; each tapped source pixel converted to
//                8-bit RGB by the header's integer formula and resized by tadb_ingest_frames' arithmetic (stream_bank.hip, restated here:
//                that file and its object are not touched) into a slot of its own in a frame store [F, S_h, S_w, 3] -- one launch, no
//                RGB frame in memory in between.
// All of it is integer: the bits are the same whatever the compiler does with floating point.
//
// Shape: ingest_frames_kernel's.  A workgroup of 256 threads owns FRAME_TR x FRAME_TC outputs of one frame (frame_io.h): blockIdx.y is
// the frame, blockIdx.x the tile.  The workgroup reads its row of the table and its colour set once (one address: scalar loads), stages
// the tile's taps and coefficients in LDS, runs the horizontal pass over the source rows under the tile's vertical taps into int32 LDS
// planes (dense rows when the tile's taps span at most four rows per output row, four slots per output row otherwise) and the vertical
// pass out of LDS through store_frames_u8x4.
//
// The conversion is made PER TAP, in the horizontal pass, in registers: an item (one source row, one output column) needs four luma
// samples and the two or three chroma pairs under them, and its neighbours in the tile need other ones unless the frame is up-scaled --
// a converted row segment in LDS would convert every pixel of the segment (up to 4.8 x the tapped ones at 1080p -> 224) and cost a
// second barrier and LDS the planes already take.  What depends on the chroma pair alone (the three chroma sums) is worked out once per
// pair, so a tap adds one max, one multiply, three adds, three shifts and three clips.  When no tap clamps, the four luma samples are 4
// contiguous bytes and the chroma samples at most 5: each comes in as the one or two aligned words that hold it and a 64-bit shift; where
// a tap clamps at a border, byte by byte.  src is 4-byte aligned, so a word that holds a live byte never begins in front of src and
// never ends behind src_bytes rounded up to 4 (the header's slack); what it holds beside the live bytes is shifted or masked out.
//
// A malformed table is never an address: the row's extents, step, pitches and the place of its three planes in src are checked by the
// workgroup before anything is loaded (a row that fails is skipped), the slot is clamped into the store, the set indices into the sets,
// `first` into a range that cannot overflow, and every tap into the row's own w or h.
//
// The library is self-contained: built with -fvisibility=hidden (simple_tad_amd/build.py), it defines the error text and the launch
// check that common.h declares for itself and exports the tady_* entry points alone.
#include <stdarg.h>
#include <stdlib.h>
#include "frame_io.h"
#pragma GCC visibility push(default)
#include "../../include/tad_mi355x_yuv.h"
#pragma GCC visibility pop

namespace tad {

static thread_local char g_yuv_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_yuv_err, sizeof(g_yuv_err), fmt, ap);
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

constexpr int YI_SLOTS = 4 * FRAME_TR;  // source rows a tile can need: four taps per output row
static_assert(YI_SLOTS * 3 * FRAME_TC * 4 + (FRAME_TC + FRAME_TR) * 5 * 4 <= 64 * 1024, "static LDS stays at or below 64 KB");

__host__ __device__ __forceinline__ int64_t yi_set_words(int out) { return TAD_FR_SET_HEAD + (int64_t)out * 5; }
__host__ __device__ __forceinline__ int64_t yi_table_words(int K, int nh, int nv, int nc, int Sh, int Sw) {
  return (int64_t)K * TADY_ROW_WORDS + nh * yi_set_words(Sw) + nv * yi_set_words(Sh) + (int64_t)nc * TADY_CSET_WORDS;
}

// does the plane of `rows` rows of `pitch` bytes, the last of them `live` bytes long, lie inside [0, src_bytes)?  (rows, live >= 1)
__host__ __device__ __forceinline__ bool yi_plane_inside(int64_t off, int64_t pitch, int rows, int64_t live, int64_t src_bytes) {
  return off >= 0 && pitch >= 0 && off <= src_bytes && (int64_t)(rows - 1) * pitch + live <= src_bytes - off;
}

// the bytes p[0 .. last] (any alignment, last <= 4) in the low bytes of a 64-bit word: aligned 4-byte loads and a shift.  Only the
// aligned words that hold one of those bytes are loaded -- one or two
__device__ __forceinline__ uint64_t yi_load_bytes(const uint8_t* p, int last) {
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
  const uint32_t* q = static_cast<const uint32_t*>(__builtin_assume_aligned(p - sh, 4));  // (derived from p: stays a global pointer)
  const uint32_t d0 = q[0], d1 = (int)sh + last >= 4 ? q[1] : 0u;
  return (((uint64_t)d1 << 32) | d0) >> (sh * 8);
}

// a colour set, in scalar registers
struct YiColour {
  int y_off, cy, cvr, cug, cvg, cub;
};

// the three chroma sums of one chroma pair, the rounding constant in them
__device__ __forceinline__ void yi_chroma(const YiColour& cs, int U, int V, int (&c)[3]) {
  c[0] = cs.cvr * (V - 128) + (1 << 19);
  c[1] = cs.cvg * (V - 128) + cs.cug * (U - 128) + (1 << 19);
  c[2] = cs.cub * (U - 128) + (1 << 19);
}

// acc[ch] += k * the 8-bit channel ch of luma sample Y under the chroma sums c
__device__ __forceinline__ void yi_tap(const YiColour& cs, int Y, const int (&c)[3], int k, int (&acc)[3]) {
  const int d = Y - cs.y_off;
  const int yy = (d < 0 ? 0 : d) * cs.cy;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) acc[ch] += frame_clamp((yy + c[ch]) >> 20, 0, 255) * k;
}

// first tap and coefficients of `n` outputs from output `o0` of a set, staged in LDS (slots past n: tap 0, coefficients 0).  `first`
// is cut to [-4, TADY_MAX_EXTENT]: first + 3 cannot overflow, and a stated tap range is [-2, in - 2], far inside
__device__ __forceinline__ void yi_stage(const int32_t* __restrict__ set, int out_size, int o0, int n, int* first, int (*kk)[4], int slots) {
  const int32_t* f = set + TAD_FR_SET_HEAD;
  const int32_t* k = f + out_size;
  for (int i = threadIdx.x; i < slots * 5; i += FRAME_THREADS) {
    const int o = i / 5, j = i - o * 5;
    if (j == 4)
      first[o] = o < n ? frame_clamp(f[o0 + o], -4, TADY_MAX_EXTENT) : 0;
    else
      kk[o][j] = o < n ? k[(int64_t)(o0 + o) * 4 + j] : 0;
  }
}

__global__ __launch_bounds__(FRAME_THREADS) void ingest_yuv_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                               uint8_t* __restrict__ store, int64_t F,
                                                               const int32_t* __restrict__ tab, int K, int nh, int nv, int nc, int Sh, int Sw,
                                                               int tiles_x) {
  __shared__ __attribute__((aligned(16))) int hp[YI_SLOTS][3][FRAME_TC];  // (read back four columns at a time)
  __shared__ int hf[FRAME_TC], hk[FRAME_TC][4], vf[FRAME_TR], vk[FRAME_TR][4];
  // the row, read once per workgroup (blockIdx.y < K: the launcher's grid)
  const int32_t* r = tab + (int64_t)blockIdx.y * TADY_ROW_WORDS;
  const int64_t y_off = r[0], y_pitch = r[1], u_off = r[2], v_off = r[3], c_pitch = r[4];
  const int c_step = r[5], H = r[6], W = r[7];
  // a row that is no frame inside src is skipped (the same for every thread of the workgroup): nothing below forms an address from it
  if (H < 1 || W < 1 || H > TADY_MAX_EXTENT || W > TADY_MAX_EXTENT || (c_step != 1 && c_step != 2)) return;
  const int CH = (H + 1) >> 1, CW = (W + 1) >> 1;
  if (y_pitch < W || c_pitch < (int64_t)CW * c_step) return;
  if (!yi_plane_inside(y_off, y_pitch, H, W, src_bytes) || !yi_plane_inside(u_off, c_pitch, CH, (int64_t)(CW - 1) * c_step + 1, src_bytes) ||
      !yi_plane_inside(v_off, c_pitch, CH, (int64_t)(CW - 1) * c_step + 1, src_bytes))
    return;
  const int64_t slot = r[8] < 0 ? 0 : ((int64_t)r[8] >= F ? F - 1 : (int64_t)r[8]);
  const int32_t* sets = tab + (int64_t)K * TADY_ROW_WORDS;
  const int32_t* hset = sets + frame_clamp(r[9], 0, nh - 1) * yi_set_words(Sw);
  const int32_t* vset = sets + nh * yi_set_words(Sw) + frame_clamp(r[10], 0, nv - 1) * yi_set_words(Sh);
  const int32_t* cset = sets + nh * yi_set_words(Sw) + nv * yi_set_words(Sh) + (int64_t)frame_clamp(r[11], 0, nc - 1) * TADY_CSET_WORDS;
  const YiColour cs = {cset[0], cset[1], cset[2], cset[3], cset[4], cset[5]};
  const bool bgr = (r[12] & TADY_BGR) != 0;
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int c0 = tx * FRAME_TC, o0 = ty * FRAME_TR;
  const int ncol = Sw - c0 < FRAME_TC ? Sw - c0 : FRAME_TC, nr = Sh - o0 < FRAME_TR ? Sh - o0 : FRAME_TR;
  yi_stage(hset, Sw, c0, ncol, hf, hk, FRAME_TC);
  yi_stage(vset, Sh, o0, nr, vf, vk, FRAME_TR);
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
  {
    const int c = tid & (FRAME_TC - 1);
    if (c < ncol) {
      const int f0 = hf[c];
      const int kq[4] = {hk[c][0], hk[c][1], hk[c][2], hk[c][3]};
      const bool inside = f0 >= 0 && f0 + 3 <= W - 1;  // no tap clamps: four contiguous luma bytes over the chroma pairs cx0 .. cx0 + np - 1
      const int cx0 = f0 >> 1, np = 2 + (f0 & 1);      // (used when inside: f0 >= 0, and cx0 + np - 1 = (f0 + 3) >> 1 <= (W - 1) >> 1)
      for (int s = tid / FRAME_TC; s < nslots; s += FRAME_THREADS / FRAME_TC) {
        const int v = dense ? lo + s : frame_clamp(vf[s >> 2] + (s & 3), 0, H - 1);  // (lo .. hi and the clamp: 0 <= v <= H - 1)
        const uint8_t* yrow = src + y_off + (int64_t)v * y_pitch;
        const uint8_t* urow = src + u_off + (int64_t)(v >> 1) * c_pitch;             // (v >> 1 <= (H - 1) >> 1 = CH - 1)
        const uint8_t* vrow = src + v_off + (int64_t)(v >> 1) * c_pitch;
        int acc[3] = {0, 0, 0};
        if (inside) {
          const uint32_t yw = (uint32_t)yi_load_bytes(yrow + f0, 3);
          const uint64_t uw = yi_load_bytes(urow + (int64_t)cx0 * c_step, (np - 1) * c_step);
          const uint64_t vw = yi_load_bytes(vrow + (int64_t)cx0 * c_step, (np - 1) * c_step);
          int cc[3][3];
#pragma unroll
          for (int i = 0; i < 3; ++i)  // (pair 2 is read from the zero bits above the loaded bytes when np = 2, and not used)
            yi_chroma(cs, (int)((uw >> (i * c_step * 8)) & 255u), (int)((vw >> (i * c_step * 8)) & 255u), cc[i]);
          const int odd = f0 & 1;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int Y = (int)((yw >> (j * 8)) & 255u);
            // tap j lies over pair (j + odd) >> 1: pairs 0 0 1 1 from an even first tap, 0 1 1 2 from an odd one
            if (j == 0)
              yi_tap(cs, Y, cc[0], kq[j], acc);
            else if (j == 3)
              yi_tap(cs, Y, odd ? cc[2] : cc[1], kq[j], acc);
            else if (j == 1)
              yi_tap(cs, Y, odd ? cc[1] : cc[0], kq[j], acc);
            else
              yi_tap(cs, Y, cc[1], kq[j], acc);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int x = frame_clamp(f0 + j, 0, W - 1);
            int cc[3];
            yi_chroma(cs, (int)urow[(int64_t)(x >> 1) * c_step], (int)vrow[(int64_t)(x >> 1) * c_step], cc);
            yi_tap(cs, (int)yrow[x], cc, kq[j], acc);
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
    const int s = frame_clamp(dense ? v - lo : orow * 4 + j, 0, YI_SLOTS - 1);
    const int k = vk[orow][j];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int4 h = *reinterpret_cast<const int4*>(&hp[s][ch][cg * 4]);
      acc[ch][0] += h.x * k, acc[ch][1] += h.y * k, acc[ch][2] += h.z * k, acc[ch][3] += h.w * k;
    }
  }
  if (bgr) {  // the stored channel order: B first (the flag is the workgroup's)
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

static int yi_shape_ok(const char* who, int K, int nh, int nv, int nc, int64_t src_bytes, int64_t F, int Sh, int Sw) {
  TAD_REQUIRE(K >= 1 && K <= TADY_MAX_FRAMES, "%s: K=%d must be in [1, %d]", who, K, TADY_MAX_FRAMES);
  TAD_REQUIRE(nh >= 1 && nh <= TADY_MAX_SETS, "%s: n_hsets=%d must be in [1, %d]", who, nh, TADY_MAX_SETS);
  TAD_REQUIRE(nv >= 1 && nv <= TADY_MAX_SETS, "%s: n_vsets=%d must be in [1, %d]", who, nv, TADY_MAX_SETS);
  TAD_REQUIRE(nc >= 1 && nc <= TADY_MAX_CSETS, "%s: n_csets=%d must be in [1, %d]", who, nc, TADY_MAX_CSETS);
  TAD_REQUIRE(Sh >= 1 && Sh <= 16384, "%s: S_h=%d must be in [1, 16384]", who, Sh);
  TAD_REQUIRE(Sw >= 1 && Sw <= 16384, "%s: S_w=%d must be in [1, 16384]", who, Sw);
  TAD_REQUIRE(F >= 1 && F <= ((int64_t)1 << 31), "%s: F=%lld must be in [1, 2^31]", who, (long long)F);
  TAD_REQUIRE(src_bytes >= 1, "%s: src_bytes=%lld must be positive", who, (long long)src_bytes);
  return TAD_OK;
}

static int yi_cmp_i64(const void* a, const void* b) {
  const int64_t x = *static_cast<const int64_t*>(a), y = *static_cast<const int64_t*>(b);
  return x < y ? -1 : (x > y ? 1 : 0);
}

static int yi_check_set(const int32_t* set, int out_size, const char* axis, int index) {
  const int in = set[0];
  TAD_REQUIRE(in >= 1 && in <= TADY_MAX_EXTENT, "ingest_plan_check: %s set %d: input extent %d outside [1, %d]", axis, index, in, TADY_MAX_EXTENT);
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

static int64_t yi_abs(int64_t v) { return v < 0 ? -v : v; }

static int yi_check_cset(const int32_t* c, int index) {
  TAD_REQUIRE(c[0] >= 0 && c[0] <= 255, "ingest_plan_check: colour set %d: y_off=%d outside [0, 255]", index, c[0]);
  TAD_REQUIRE(c[1] >= 0, "ingest_plan_check: colour set %d: cy=%d is negative", index, c[1]);
  int64_t m = yi_abs(c[2]);  // |cvr|, |cub|, |cug| + |cvg|: the largest chroma sum of a channel is 128 times that
  m = yi_abs(c[5]) > m ? yi_abs(c[5]) : m;
  m = yi_abs(c[3]) + yi_abs(c[4]) > m ? yi_abs(c[3]) + yi_abs(c[4]) : m;
  const int64_t bound = 255 * (int64_t)c[1] + 128 * m + ((int64_t)1 << 19);
  TAD_REQUIRE(bound < ((int64_t)1 << 31), "ingest_plan_check: colour set %d: 255 * cy + 128 * max|c| + 2^19 = %lld reaches 2^31 (the int32 sums would overflow)",
              index, (long long)bound);
  TAD_REQUIRE(c[6] == 0 && c[7] == 0, "ingest_plan_check: colour set %d: words 6 and 7 are %d and %d, they must be 0", index, c[6], c[7]);
  return TAD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int tady_abi_version(void) { return TADY_ABI_VERSION; }

const char* tady_last_error_string(void) { return tad::g_yuv_err; }

int tady_ingest_plan_check(const int32_t* table_host, int64_t n_words, int K, int n_hsets, int n_vsets, int n_csets, int64_t src_bytes,
                           int64_t F, int S_h, int S_w) {
  TAD_REQUIRE(table_host, "ingest_plan_check: table_host is null");
  if (int rc = yi_shape_ok("ingest_plan_check", K, n_hsets, n_vsets, n_csets, src_bytes, F, S_h, S_w)) return rc;
  const int64_t want = yi_table_words(K, n_hsets, n_vsets, n_csets, S_h, S_w);
  TAD_REQUIRE(n_words == want, "ingest_plan_check: n_words=%lld, expected K * %d + the sets = %lld", (long long)n_words, TADY_ROW_WORDS,
              (long long)want);
  const int32_t* hsets = table_host + (int64_t)K * TADY_ROW_WORDS;
  const int32_t* vsets = hsets + n_hsets * yi_set_words(S_w);
  const int32_t* csets = vsets + n_vsets * yi_set_words(S_h);
  for (int i = 0; i < n_hsets; ++i)
    if (int rc = yi_check_set(hsets + i * yi_set_words(S_w), S_w, "horizontal", i)) return rc;
  for (int i = 0; i < n_vsets; ++i)
    if (int rc = yi_check_set(vsets + i * yi_set_words(S_h), S_h, "vertical", i)) return rc;
  for (int i = 0; i < n_csets; ++i)
    if (int rc = yi_check_cset(csets + i * TADY_CSET_WORDS, i)) return rc;
  int64_t slots[TADY_MAX_FRAMES];  // slot * TADY_MAX_FRAMES + row, sorted below: two rows of one slot end up next to each other (32 KB of stack)
  for (int k = 0; k < K; ++k) {
    const int32_t* r = table_host + (int64_t)k * TADY_ROW_WORDS;
    const int64_t y_off = r[0], y_pitch = r[1], u_off = r[2], v_off = r[3], c_pitch = r[4];
    const int c_step = r[5], h = r[6], w = r[7], slot = r[8], hs = r[9], vs = r[10], cs = r[11];
    TAD_REQUIRE(h >= 1 && h <= TADY_MAX_EXTENT, "ingest_plan_check: row %d: h=%d outside [1, %d]", k, h, TADY_MAX_EXTENT);
    TAD_REQUIRE(w >= 1 && w <= TADY_MAX_EXTENT, "ingest_plan_check: row %d: w=%d outside [1, %d]", k, w, TADY_MAX_EXTENT);
    TAD_REQUIRE(c_step == 1 || c_step == 2, "ingest_plan_check: row %d: c_step=%d must be 1 (planar chroma) or 2 (interleaved)", k, c_step);
    const int ch = (h + 1) / 2, cw = (w + 1) / 2;
    TAD_REQUIRE(y_pitch >= w, "ingest_plan_check: row %d: y_pitch=%lld is below the %d live bytes of a luma row", k, (long long)y_pitch, w);
    TAD_REQUIRE(c_pitch >= (int64_t)cw * c_step, "ingest_plan_check: row %d: c_pitch=%lld is below the %d live bytes of a chroma row", k,
                (long long)c_pitch, cw * c_step);
    TAD_REQUIRE(yi_plane_inside(y_off, y_pitch, h, w, src_bytes), "ingest_plan_check: row %d: the luma plane's bytes [%lld, %lld) are not inside src_bytes=%lld",
                k, (long long)y_off, (long long)(y_off + (int64_t)(h - 1) * y_pitch + w), (long long)src_bytes);
    const int64_t clive = (int64_t)(cw - 1) * c_step + 1;
    TAD_REQUIRE(yi_plane_inside(u_off, c_pitch, ch, clive, src_bytes), "ingest_plan_check: row %d: the U plane's bytes [%lld, %lld) are not inside src_bytes=%lld",
                k, (long long)u_off, (long long)(u_off + (int64_t)(ch - 1) * c_pitch + clive), (long long)src_bytes);
    TAD_REQUIRE(yi_plane_inside(v_off, c_pitch, ch, clive, src_bytes), "ingest_plan_check: row %d: the V plane's bytes [%lld, %lld) are not inside src_bytes=%lld",
                k, (long long)v_off, (long long)(v_off + (int64_t)(ch - 1) * c_pitch + clive), (long long)src_bytes);
    TAD_REQUIRE(c_step == 1 || u_off - v_off == 1 || v_off - u_off == 1,
                "ingest_plan_check: row %d: interleaved chroma (c_step=2) with u_off=%lld and v_off=%lld not next to each other", k, (long long)u_off,
                (long long)v_off);
    TAD_REQUIRE(slot >= 0 && (int64_t)slot < F, "ingest_plan_check: row %d: slot=%d outside the store [0, F=%lld)", k, slot, (long long)F);
    TAD_REQUIRE(hs >= 0 && hs < n_hsets, "ingest_plan_check: row %d: hset=%d outside [0, %d)", k, hs, n_hsets);
    TAD_REQUIRE(vs >= 0 && vs < n_vsets, "ingest_plan_check: row %d: vset=%d outside [0, %d)", k, vs, n_vsets);
    TAD_REQUIRE(cs >= 0 && cs < n_csets, "ingest_plan_check: row %d: cset=%d outside [0, %d)", k, cs, n_csets);
    TAD_REQUIRE(hsets[hs * yi_set_words(S_w)] == w, "ingest_plan_check: row %d: its hset %d is stated for %d columns, the frame has w=%d", k, hs,
                hsets[hs * yi_set_words(S_w)], w);
    TAD_REQUIRE(vsets[vs * yi_set_words(S_h)] == h, "ingest_plan_check: row %d: its vset %d is stated for %d rows, the frame has h=%d", k, vs,
                vsets[vs * yi_set_words(S_h)], h);
    TAD_REQUIRE((r[12] & ~TADY_BGR) == 0, "ingest_plan_check: row %d: flags=0x%x holds unknown bits", k, (unsigned)r[12]);
    for (int i = 13; i < TADY_ROW_WORDS; ++i) TAD_REQUIRE(r[i] == 0, "ingest_plan_check: row %d: word %d is %d, it must be 0", k, i, r[i]);
    slots[k] = (int64_t)slot * TADY_MAX_FRAMES + k;
  }
  qsort(slots, (size_t)K, sizeof(int64_t), yi_cmp_i64);  // (C's: a std::sort would put its template instances into the export table)
  for (int k = 1; k < K; ++k)
    TAD_REQUIRE(slots[k] / TADY_MAX_FRAMES != slots[k - 1] / TADY_MAX_FRAMES, "ingest_plan_check: row %d: slot=%lld is already named by row %d",
                (int)(slots[k] % TADY_MAX_FRAMES), (long long)(slots[k] / TADY_MAX_FRAMES), (int)(slots[k - 1] % TADY_MAX_FRAMES));
  return TAD_OK;
}

int tady_ingest_yuv(const uint8_t* src, int64_t src_bytes, uint8_t* store, int64_t F, const int32_t* table, int64_t n_words, int K,
                    int n_hsets, int n_vsets, int n_csets, int S_h, int S_w, tad_stream_t stream) {
  TAD_REQUIRE(src, "ingest_yuv: src is null");
  TAD_REQUIRE(store, "ingest_yuv: store is null");
  TAD_REQUIRE(table, "ingest_yuv: table is null");
  if (int rc = yi_shape_ok("ingest_yuv", K, n_hsets, n_vsets, n_csets, src_bytes, F, S_h, S_w)) return rc;
  const int64_t want = yi_table_words(K, n_hsets, n_vsets, n_csets, S_h, S_w);
  TAD_REQUIRE(n_words == want, "ingest_yuv: n_words=%lld, expected K * %d + the sets = %lld", (long long)n_words, TADY_ROW_WORDS, (long long)want);
  TAD_REQUIRE_ALIGNED("ingest_yuv", src, 4);
  TAD_REQUIRE_ALIGNED("ingest_yuv", table, 4);  // (store: any address)
  int tiles_x;
  const dim3 grid(frame_tile_grid(S_h, S_w, &tiles_x), (unsigned)K);
  hipLaunchKernelGGL(ingest_yuv_kernel, grid, dim3(FRAME_THREADS), 0, (hipStream_t)stream, src, src_bytes, store, F, table, K, n_hsets, n_vsets,
                     n_csets, S_h, S_w, tiles_x);
  return check_launch("ingest_yuv");
}

}  // extern "C"
#pragma GCC visibility pop
