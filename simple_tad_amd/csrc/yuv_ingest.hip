// Ragged ingest of 4:2:0 YUV camera surfaces: the YUV-ingest ABI of include/tad_mi355x_yuv.h (tady_*), the ONE source of
// libtad_mi355x_yuv.so.
//   ingest_yuv   K pitched NV12 / NV21 / I420 frames of K different sizes, packed in one buffer; each tapped source pixel converted to
//                8-bit RGB by the header's integer formula and resized by the arithmetic of cubic_resize.h (tadb_ingest_frames') into a
//                slot of its own in a frame store [F, S_h, S_w, 3] -- one launch, no RGB frame in memory in between.
// All of it is integer: the bits are the same whatever the compiler does with floating point.
//
// Shape: ingest_frames_kernel's (stream_bank.hip): blockIdx.y is the frame, blockIdx.x the tile of cubic_resize.h.  The workgroup reads
// its row of the table and its colour set once (one address: scalar loads).
//
// The horizontal pass is this file's own.  The conversion is made PER TAP, in registers: an item (one source row, one output column)
// needs four luma samples and the two or three chroma pairs under them, and its neighbours in the tile need other ones unless the frame
// is up-scaled -- a converted row segment in LDS would convert every pixel of the segment (up to 4.8 x the tapped ones at 1080p -> 224)
// and cost a second barrier and LDS the planes already take.  What depends on the chroma pair alone (the three chroma sums) is worked
// out once per pair, so a tap adds one max, one multiply, three adds, three shifts and three clips.  When no tap clamps, the four luma
// samples are 4 contiguous bytes and the chroma samples at most 5: each comes in as the one or two aligned words that hold it and a
// 64-bit shift; where a tap clamps at a border, byte by byte.  src is 4-byte aligned, so a word that holds a live byte never begins in
// front of src and never ends behind src_bytes rounded up to 4 (the header's slack); what it holds beside the live bytes is shifted or
// masked out.
//
// A malformed table is never an address: the row's extents, step, pitches and the place of its three planes in src are checked by the
// workgroup before anything is loaded (a row that fails is skipped), the slot is clamped into the store, the set indices into the sets,
// and every tap into the row's own w or h (cubic_resize.h).
//
// The library is self-contained (side_library.h) and exports the tady_* entry points alone.
#include "side_library.h"
#include "frame_io.h"
#include "cubic_resize.h"
#pragma GCC visibility push(default)
#include "../../include/tad_mi355x_yuv.h"
#pragma GCC visibility pop

TAD_NAMESPACE_BEGIN

static_assert(TADY_MAX_FRAMES == RAGGED_MAX_FRAMES && TADY_MAX_SETS == RAGGED_MAX_SETS && TADY_MAX_EXTENT == RAGGED_MAX_EXTENT, "the header's limits");

__host__ __device__ __forceinline__ int64_t yi_table_words(int K, int nh, int nv, int nc, int Sh, int Sw) {
  return (int64_t)K * TADY_ROW_WORDS + nh * cubic_set_words(Sw) + nv * cubic_set_words(Sh) + (int64_t)nc * TADY_CSET_WORDS;
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

__global__ __launch_bounds__(FRAME_THREADS) void ingest_yuv_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                               uint8_t* __restrict__ store, int64_t F,
                                                               const int32_t* __restrict__ tab, int K, int nh, int nv, int nc, int Sh, int Sw,
                                                               int tiles_x) {
  CUBIC_TILE_LDS;
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
  const int32_t* hset = sets + frame_clamp(r[9], 0, nh - 1) * cubic_set_words(Sw);
  const int32_t* vset = sets + nh * cubic_set_words(Sw) + frame_clamp(r[10], 0, nv - 1) * cubic_set_words(Sh);
  const int32_t* cset = sets + nh * cubic_set_words(Sw) + nv * cubic_set_words(Sh) + (int64_t)frame_clamp(r[11], 0, nc - 1) * TADY_CSET_WORDS;
  const YiColour cs = {cset[0], cset[1], cset[2], cset[3], cset[4], cset[5]};
  const bool bgr = (r[12] & TADY_BGR) != 0;  // the stored channel order: B first
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int c0 = tx * FRAME_TC, o0 = ty * FRAME_TR;
  const int ncol = Sw - c0 < FRAME_TC ? Sw - c0 : FRAME_TC, nr = Sh - o0 < FRAME_TR ? Sh - o0 : FRAME_TR;
  cubic_stage(hset, Sw, c0, ncol, W, hf, hk, FRAME_TC);
  cubic_stage(vset, Sh, o0, nr, H, vf, vk, FRAME_TR);
  __syncthreads();
  const CubicSpan span = cubic_span(vf, nr, H);

  // horizontal pass: an item is one column of one source row, all three channels; a thread keeps its column and walks the rows
  {
    const int c = tid & (FRAME_TC - 1);
    if (c < ncol) {
      const int f0 = hf[c];
      const int kq[4] = {hk[c][0], hk[c][1], hk[c][2], hk[c][3]};
      const bool inside = f0 >= 0 && f0 + 3 <= W - 1;  // no tap clamps: four contiguous luma bytes over the chroma pairs cx0 .. cx0 + np - 1
      const int cx0 = f0 >> 1, np = 2 + (f0 & 1);      // (used when inside: f0 >= 0, and cx0 + np - 1 = (f0 + 3) >> 1 <= (W - 1) >> 1)
      for (int s = tid / FRAME_TC; s < span.nslots; s += FRAME_THREADS / FRAME_TC) {
        const int v = cubic_slot_row(span, vf, s, H);  // (0 <= v <= H - 1)
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

  CubicOut at;
  int acc[3][4];
  if (!cubic_vpass(hp, vf, vk, span, H, c0, nr, Sw, bgr, at, acc)) return;
  const int oy = o0 + at.orow;
  store_frames_u8x4(store + (((int64_t)slot * Sh + oy) * Sw + at.col) * 3, acc, at.valid);
}

TAD_NAMESPACE_END

using namespace tad;

static int yi_shape_ok(const char* who, int K, int nh, int nv, int nc, int64_t src_bytes, int64_t F, int Sh, int Sw) {
  if (int rc = ragged_shape_ok(who, K, nh, nv, src_bytes, F, Sh, Sw)) return rc;
  TAD_REQUIRE(nc >= 1 && nc <= TADY_MAX_CSETS, "%s: n_csets=%d must be in [1, %d]", who, nc, TADY_MAX_CSETS);
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

const char* tady_last_error_string(void) { return tad::side_last_error(); }

int tady_ingest_plan_check(const int32_t* table_host, int64_t n_words, int K, int n_hsets, int n_vsets, int n_csets, int64_t src_bytes,
                           int64_t F, int S_h, int S_w) {
  TAD_REQUIRE(table_host, "ingest_plan_check: table_host is null");
  if (int rc = yi_shape_ok("ingest_plan_check", K, n_hsets, n_vsets, n_csets, src_bytes, F, S_h, S_w)) return rc;
  const int64_t want = yi_table_words(K, n_hsets, n_vsets, n_csets, S_h, S_w);
  TAD_REQUIRE(n_words == want, "ingest_plan_check: n_words=%lld, expected K * %d + the sets = %lld", (long long)n_words, TADY_ROW_WORDS,
              (long long)want);
  const int32_t* hsets = table_host + (int64_t)K * TADY_ROW_WORDS;
  const int32_t* vsets = hsets + n_hsets * cubic_set_words(S_w);
  const int32_t* csets = vsets + n_vsets * cubic_set_words(S_h);
  for (int i = 0; i < n_hsets; ++i)
    if (int rc = cubic_check_set("ingest_plan_check", hsets + i * cubic_set_words(S_w), S_w, "horizontal", i, TADY_MAX_EXTENT)) return rc;
  for (int i = 0; i < n_vsets; ++i)
    if (int rc = cubic_check_set("ingest_plan_check", vsets + i * cubic_set_words(S_h), S_h, "vertical", i, TADY_MAX_EXTENT)) return rc;
  for (int i = 0; i < n_csets; ++i)
    if (int rc = yi_check_cset(csets + i * TADY_CSET_WORDS, i)) return rc;
  int64_t slots[TADY_MAX_FRAMES];  // (32 KB of stack)
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
    TAD_REQUIRE(hsets[hs * cubic_set_words(S_w)] == w, "ingest_plan_check: row %d: its hset %d is stated for %d columns, the frame has w=%d", k, hs,
                hsets[hs * cubic_set_words(S_w)], w);
    TAD_REQUIRE(vsets[vs * cubic_set_words(S_h)] == h, "ingest_plan_check: row %d: its vset %d is stated for %d rows, the frame has h=%d", k, vs,
                vsets[vs * cubic_set_words(S_h)], h);
    TAD_REQUIRE((r[12] & ~TADY_BGR) == 0, "ingest_plan_check: row %d: flags=0x%x holds unknown bits", k, (unsigned)r[12]);
    for (int i = 13; i < TADY_ROW_WORDS; ++i) TAD_REQUIRE(r[i] == 0, "ingest_plan_check: row %d: word %d is %d, it must be 0", k, i, r[i]);
    slots[k] = slot;
  }
  return ragged_slots_once("ingest_plan_check", slots, K);
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
