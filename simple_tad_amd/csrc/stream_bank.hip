// Ragged ingest for a bank of camera streams: the stream-bank ABI of include/tad_mi355x_bank.h (tadb_*), the ONE source of
// libtad_mi355x_bank.so.
//   ingest_frames   K decoded uint8 frames of K different sizes, packed in one buffer, each resized to S_h x S_w (the loader's
//                   cv2.resize(frame, (S_w, S_h), INTER_CUBIC), run_inference.py:76,91) and written to a slot of its own in a frame store
//                   [F, S_h, S_w, 3] -- one launch for a tick of a whole fleet, where tad_frame_resize takes one source size and writes
//                   one contiguous output per call.
// The arithmetic, the tile and the vertical pass are cubic_resize.h's (tad_frame_resize's under TAD_FR_NONE), with everything that was
// the call's now the row's: blockIdx.y is the frame, blockIdx.x the tile -- every frame has the same S_h x S_w outputs, so the grid is
// rectangular although the sources are not.  The workgroup reads its row of the table once (one address: scalar loads).
//
// The horizontal pass is this file's own: the four pixels under an output's taps are 12 contiguous bytes of a packed RGB row
// (cubic_load12); where a tap clamps at a border, byte by byte.  Frames start on multiples of 4 in a 4-byte aligned buffer, so those
// words never begin before their frame, and end at most 3 bytes behind it (the header's slack); what they hold beyond the 12 bytes is
// shifted out.
//
// A malformed table is never an address: the row's extents and its frame's place in src are checked by the workgroup before anything is
// loaded (a row that fails is skipped), the slot is clamped into the store, the set indices into the sets, and every tap into the row's
// own w or h (cubic_resize.h).
//
// The library is self-contained (side_library.h) and exports the tadb_* entry points alone.
#include "side_library.h"
#include "cubic_resize.h"
#pragma GCC visibility push(default)
#include "../../include/tad_mi355x_bank.h"
#pragma GCC visibility pop

TAD_NAMESPACE_BEGIN

static_assert(TADB_MAX_FRAMES == RAGGED_MAX_FRAMES && TADB_MAX_SETS == RAGGED_MAX_SETS && TADB_MAX_EXTENT == RAGGED_MAX_EXTENT, "the header's limits");

__host__ __device__ __forceinline__ int64_t sb_table_words(int K, int nh, int nv, int Sh, int Sw) {
  return (int64_t)K * TADB_ROW_WORDS + nh * cubic_set_words(Sw) + nv * cubic_set_words(Sh);
}

__global__ __launch_bounds__(FRAME_THREADS) void ingest_frames_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                  uint8_t* __restrict__ store, int64_t F,
                                                                  const int32_t* __restrict__ tab, int K, int nh, int nv, int Sh, int Sw,
                                                                  int tiles_x) {
  CUBIC_TILE_LDS;
  // the row, read once per workgroup (blockIdx.y < K: the launcher's grid)
  const int32_t* r = tab + (int64_t)blockIdx.y * TADB_ROW_WORDS;
  const int64_t off = (int64_t)r[0];
  const int H = r[1], W = r[2];
  // a row that is no frame inside src is skipped (the same for every thread of the workgroup): nothing below forms an address from it
  if (H < 1 || W < 1 || H > TADB_MAX_EXTENT || W > TADB_MAX_EXTENT || off < 0) return;
  if (off > src_bytes || (int64_t)H * W * 3 > src_bytes - off) return;
  const int64_t slot = r[3] < 0 ? 0 : ((int64_t)r[3] >= F ? F - 1 : (int64_t)r[3]);
  const int32_t* hset = tab + (int64_t)K * TADB_ROW_WORDS + frame_clamp(r[4], 0, nh - 1) * cubic_set_words(Sw);
  const int32_t* vset = tab + (int64_t)K * TADB_ROW_WORDS + nh * cubic_set_words(Sw) + frame_clamp(r[5], 0, nv - 1) * cubic_set_words(Sh);
  const bool swap = (r[6] & TADB_SWAP_RB) != 0;  // the stored channel order: a swapped row puts source channel 2 where channel 0 goes
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int c0 = tx * FRAME_TC, o0 = ty * FRAME_TR;
  const int nc = Sw - c0 < FRAME_TC ? Sw - c0 : FRAME_TC, nr = Sh - o0 < FRAME_TR ? Sh - o0 : FRAME_TR;
  cubic_stage(hset, Sw, c0, nc, W, hf, hk, FRAME_TC);
  cubic_stage(vset, Sh, o0, nr, H, vf, vk, FRAME_TR);
  __syncthreads();
  const CubicSpan span = cubic_span(vf, nr, H);

  // horizontal pass: an item is one column of one source row, all three channels; a thread keeps its column and walks the rows
  const uint8_t* frame = src + off;
  {
    const int c = tid & (FRAME_TC - 1);
    if (c < nc) {
      const int f0 = hf[c];
      const int kq[4] = {hk[c][0], hk[c][1], hk[c][2], hk[c][3]};
      const bool inside = f0 >= 0 && f0 + 3 <= W - 1;  // no tap clamps: the four pixels are 12 contiguous bytes of the row
      for (int s = tid / FRAME_TC; s < span.nslots; s += FRAME_THREADS / FRAME_TC) {
        const uint8_t* row = frame + (int64_t)cubic_slot_row(span, vf, s, H) * W * 3;
        int acc[3] = {0, 0, 0};
        if (inside) {
          uint32_t w[3];
          cubic_load12(row + (int64_t)f0 * 3, w);
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

  CubicOut at;
  int acc[3][4];
  if (!cubic_vpass(hp, vf, vk, span, H, c0, nr, Sw, swap, at, acc)) return;
  const int oy = o0 + at.orow;
  store_frames_u8x4(store + (((int64_t)slot * Sh + oy) * Sw + at.col) * 3, acc, at.valid);
}

TAD_NAMESPACE_END

using namespace tad;

#pragma GCC visibility push(default)
extern "C" {

int tadb_abi_version(void) { return TADB_ABI_VERSION; }

const char* tadb_last_error_string(void) { return tad::side_last_error(); }

int tadb_ingest_plan_check(const int32_t* table_host, int64_t n_words, int K, int n_hsets, int n_vsets, int64_t src_bytes, int64_t F,
                           int S_h, int S_w) {
  TAD_REQUIRE(table_host, "ingest_plan_check: table_host is null");
  if (int rc = ragged_shape_ok("ingest_plan_check", K, n_hsets, n_vsets, src_bytes, F, S_h, S_w)) return rc;
  const int64_t want = sb_table_words(K, n_hsets, n_vsets, S_h, S_w);
  TAD_REQUIRE(n_words == want, "ingest_plan_check: n_words=%lld, expected K * %d + the sets = %lld", (long long)n_words, TADB_ROW_WORDS,
              (long long)want);
  const int32_t* hsets = table_host + (int64_t)K * TADB_ROW_WORDS;
  const int32_t* vsets = hsets + n_hsets * cubic_set_words(S_w);
  for (int i = 0; i < n_hsets; ++i)
    if (int rc = cubic_check_set("ingest_plan_check", hsets + i * cubic_set_words(S_w), S_w, "horizontal", i, TADB_MAX_EXTENT)) return rc;
  for (int i = 0; i < n_vsets; ++i)
    if (int rc = cubic_check_set("ingest_plan_check", vsets + i * cubic_set_words(S_h), S_h, "vertical", i, TADB_MAX_EXTENT)) return rc;
  int64_t slots[TADB_MAX_FRAMES];  // (32 KB of stack)
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
    TAD_REQUIRE(hsets[hs * cubic_set_words(S_w)] == w, "ingest_plan_check: row %d: its hset %d is stated for %d columns, the frame has w=%d", k, hs,
                hsets[hs * cubic_set_words(S_w)], w);
    TAD_REQUIRE(vsets[vs * cubic_set_words(S_h)] == h, "ingest_plan_check: row %d: its vset %d is stated for %d rows, the frame has h=%d", k, vs,
                vsets[vs * cubic_set_words(S_h)], h);
    TAD_REQUIRE((r[6] & ~TADB_SWAP_RB) == 0, "ingest_plan_check: row %d: flags=0x%x holds unknown bits", k, (unsigned)r[6]);
    TAD_REQUIRE(r[7] == 0, "ingest_plan_check: row %d: word 7 is %d, it must be 0", k, r[7]);
    slots[k] = slot;
  }
  return ragged_slots_once("ingest_plan_check", slots, K);
}

int tadb_ingest_frames(const uint8_t* src, int64_t src_bytes, uint8_t* store, int64_t F, const int32_t* table, int64_t n_words, int K,
                       int n_hsets, int n_vsets, int S_h, int S_w, tad_stream_t stream) {
  TAD_REQUIRE(src, "ingest_frames: src is null");
  TAD_REQUIRE(store, "ingest_frames: store is null");
  TAD_REQUIRE(table, "ingest_frames: table is null");
  if (int rc = ragged_shape_ok("ingest_frames", K, n_hsets, n_vsets, src_bytes, F, S_h, S_w)) return rc;
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
