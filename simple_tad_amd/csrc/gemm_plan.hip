// Launch planner of the Linear GEMMs and the process-wide state that goes with it (see gemm_plan.h).  Host code only: compiled once, for
// both operand formats.  The executors of the plans are in gemm.hip.
#include <limits.h>
#include <string.h>
#include "common.h"
#include "gemm_plan.h"
#include "knob.h"

namespace tad {

// ---- the knobs: ONE table for the initial values (environment), tad_linear_tuning and tad_linear_tuning_get
namespace knobs {
int gemm_debug;  // ablation bits (GemmNT::debug); only ablation builds look at them
int nt_persist;
int nt_direct;
int nt_split;
int nt_sk_defer;  // 1 = split-K tails leave their partial tiles in front of the whole-round launch and are combined behind it; 0 = combined inside one launch
int nt_splitk;    // 1 = the tail launch of the split plan may split its tiles along K (needs a workspace); 0 = never; 2 = whenever eligible
int nt_variant;   // 0 = planned per shape (nt_plan), else the tile configuration for every launch
int nt_group_m_knob;  // 0 = per-shape choice (nt_group_m)
int tn_variant;
// > 0: bias-only Linears with K >= this run their whole rounds on the four-wave kernel.  Measured (tools/exp_w4_plain.py, planned launches at M = 50176):
// qkv forward 176.9 / 177.2 us (eight / four waves), dX(proj) 78.0 / 73.9, dX(qkv) 159.0 / 148.4, dX(fc1) 225.4 / 208.5 -- on by default
int nt_w4_plain;  // K_min of the Linears whose whole rounds of 256 x 256 tiles run on the four-wave kernel (0 = none): below ~640 its epilogue costs more than its K loop gains (tools/exp_w4_plain.py --D 384 / 512)
// bit mask: which other epilogues' whole rounds take the four-wave kernel (see nt_main_variant).  Measured (tools/exp_gemm_knobs.py --configs
// "w4_epilogues=0;w4_epilogues=14", eight / four waves): proj + residual 96.0 / 96.9 us, fc2 + residual 250.4 / 241.1, fc1 GELU 278.1 / 282.1, dX(fc2) GELU backward
// 291.2 / 338.8 -- the residual epilogue (bit 2) is on by default, the vector-heavy GELU ones stay on eight waves
int nt_w4_epilogues;
int tn_pair;      // 1: tad_linear_bwd_weight_pair runs its two problems as one launch when they fit (TnPlan::fits); 0: always two launches
int nt_short_k;   // 1: the short-K plan of nt_plan (K <= 512: tiles that put two workgroups on a CU)
int nt_tail_192;  // 1: tails of the split plan may run as 192 x 128 tiles (nt_tail_variant)
int tn_w4;        // 1: the 256 x 256 weight-gradient GEMM runs as four waves of 128 x 128 (gemm_w4.hip)
int tn_pdeep;     // 1: gemm_tn 256 x 256 with the P operand two reduction tiles ahead (see PDEEP); measured null (round 4), off
unsigned long long* nt_stamps = nullptr;
long long nt_launches = 0;
}  // namespace knobs
using namespace knobs;

namespace {
const Knob KNOBS[] = {
    {"debug", &gemm_debug, INT_MIN, INT_MAX, "TAD_GEMM_DEBUG", 0, 0},  // (settable, but no part of the documented defaults: timing experiments on ablation builds)
    {"persistent", &nt_persist, INT_MIN, INT_MAX, "TAD_GEMM_NO_PERSIST", 1, KNOB_BOOL | KNOB_ENV_INVERTED},
    {"direct_epilogue", &nt_direct, 0, 2, "TAD_GEMM_DIRECT_EPI", 1, 0},
    {"split_tail", &nt_split, 0, 2, "TAD_GEMM_SPLIT_TAIL", 1, 0},
    {"splitk_defer", &nt_sk_defer, 0, 1, "TAD_GEMM_SPLITK_DEFER", 1, 0},
    {"splitk_tail", &nt_splitk, 0, 2, "TAD_GEMM_SPLITK_TAIL", 1, 0},
    {"variant", &nt_variant, 0, 9, "TAD_GEMM_NT_VARIANT", 0, 0},  // (6 is refused: tad_linear_tuning)
    {"group_m", &nt_group_m_knob, 0, 1024, "TAD_GEMM_GROUP_M", 0, 0},
    {nullptr, &knobs::tn_variant, 0, 0, "TAD_GEMM_TN_VARIANT", 0, 0},
    {"w4_plain", &nt_w4_plain, 0, INT_MAX, "TAD_GEMM_W4_PLAIN", 640, 0},
    {"w4_epilogues", &nt_w4_epilogues, 0, 15, "TAD_GEMM_W4_EPILOGUES", 4, 0},
    {"tn_pair", &tn_pair, 0, 1, "TAD_GEMM_TN_PAIR", 1, 0},
    {"short_k", &nt_short_k, 0, 1, "TAD_GEMM_SHORT_K", 1, 0},
    {"tail_192", &nt_tail_192, 0, 1, "TAD_GEMM_TAIL_192", 1, 0},
    {"tn_w4", &tn_w4, 0, 1, "TAD_GEMM_TN_W4", 1, 0},
    {"tn_pdeep", &tn_pdeep, 0, 1, "TAD_GEMM_TN_PDEEP", 0, 0},
};
const bool knobs_initialised = knobs_from_env(KNOBS);
}  // namespace

// ---- the machine, named once
constexpr int CU_FALLBACK = 256;  // without a device (plan queries on a build machine): the MI355X's count
static int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = CU_FALLBACK;
    return v;
  }();
  return n;
}
// grid of a persistent launch: one workgroup per CU, a multiple of the 8 XCDs
static int persistent_grid() { return cu_count() & ~7; }

// Row panels per column-panel group of the tile raster.  The ~32 workgroups resident on an XCD (private 4 MiB L2) walk consecutive
// tile ids, so at any time they touch GROUP_M A-panels and ~32 / GROUP_M W-panels; each panel streams K-tile by K-tile, and a
// panel's K-tile is fetched from beyond L2 once per group of tiles that share it while they run together.  Per group of
// GROUP_M x tiles_n tiles that is GROUP_M A-panel loads (algorithmic) + tiles_n W-panel loads (overhead, amortised over GROUP_M).
// Measured (tools/exp_gemm_knobs.py --knob group_m, the eight Linear shapes of a ViT-B block, with the non-temporal output stores in): 2 / 4 / 8 are
// within 0.5 % of each other in sum; the long reductions (K = 2304 / 3072: an A panel of 256 rows is 1.2 - 1.5 MB) are 1 - 4 % faster with 4 (fc2 241
// vs 246 us, dX(fc1) 220 vs 222), the K = 768 shapes with 8 (qkv 166 vs 169).
static int nt_group_m(int K) {
  if (nt_group_m_knob > 0) return nt_group_m_knob;
  return K >= 2048 ? 4 : 8;
}

// ---- the split-K error word
// The in-launch combine (mode 0) waits for the other shares of its tile with a bounded spin; a share that never arrives (the grid was
// not co-resident: a side stream or another process held CUs) leaves stale partial sums in the output.  The kernel then sets this word,
// which lives in pinned, device-mapped host memory so that the host can see it without a synchronisation: every later Linear launch
// checks it first and returns TAD_ELAUNCH (the word used to sit in the workspace, where nobody read it).
static bool sk_error_pending_armed = false;  // (the word exists only once a mode-0 launch has been made)
unsigned* sk_error_word(unsigned** dev_ptr) {
  static unsigned* host = nullptr;
  static unsigned* dev = nullptr;
  if (!host) {
    void* h = nullptr;
    void* d = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess) return nullptr;
    host = (unsigned*)h;
    dev = (unsigned*)d;
    *host = 0u;
  }
  if (dev_ptr) { *dev_ptr = dev; sk_error_pending_armed = true; }
  return host;
}
int sk_check_pending_error() {
  if (!sk_error_pending_armed) return TAD_OK;
  unsigned* host = sk_error_word(nullptr);
  if (host && __atomic_load_n(host, __ATOMIC_RELAXED)) {
    __atomic_store_n(host, 0u, __ATOMIC_RELAXED);
    set_error("gemm_nt: an earlier in-launch split-K combine (tad_linear_tuning(\"splitk_defer\", 0)) gave up waiting for a share of its tile -- "
              "its grid was not co-resident (another stream or process held CUs); the output of that Linear is INVALID.  Use the default "
              "deferred plan (splitk_defer = 1), which has no residency requirement");
    return TAD_ELAUNCH;
  }
  return TAD_OK;
}

// ---- geometry of the split plan, ONE copy for nt_plan, nt_splitk_plan and tad_linear_workspace_bytes (the workspace query
// used to restate it, and any drift made the split-K tail drop out without a diagnostic)
// Largest row count one launch may cover (32-bit operand offsets, see nt_plan); esz = bytes of the widest element the epilogue touches
static int64_t nt_max_rows(int N, int K, int64_t esz) {
  int64_t max_rows = ((1ll << 31) - 1) / ((int64_t)N * esz) - 256;
  const int64_t a_rows = ((1ll << 32) - 1) / ((int64_t)K * 2);
  if (a_rows < max_rows) max_rows = a_rows;
  return max_rows / 256 * 256;
}
// Rows that fill whole rounds of one 256 x 256 tile per CU (0: the split plan does not apply); *tail_tiles = the 256 x 256 tiles left behind them
static int nt_main_rows(int64_t M, int N, int64_t* tail_tiles) {
  const int grid = persistent_grid();
  const int64_t tiles_n = (N + 255) / 256, tiles_m = (M + 255) / 256;
  const int64_t rounds = grid > 0 ? tiles_m * tiles_n / grid : 0;
  const int64_t panels = rounds > 0 ? rounds * grid / tiles_n : 0;
  if (!(panels > 0 && panels < tiles_m)) return 0;
  if (tail_tiles) *tail_tiles = (tiles_m - panels) * tiles_n;
  return (int)(panels * 256);
}
// Shares per tile of a split-K tail of `tiles` tiles with nk K-tiles each (0: it does not split): every share needs at least two K-tiles and all
// shares must be resident at once
static int nt_splitk_shares(int64_t tiles, int nk) {
  const int cus = cu_count();
  if (!nt_splitk || tiles <= 0 || tiles > cus / 2 || tiles > 1008) return 0;
  // measured (tools/exp_splitk.py, round 4): the 78-tile tails of ViT-B's N = 768 Linears (30 % of the CUs busy for one K loop) do NOT
  // gain -- three shares of 16 K-tiles + the combine take as long as one 256 x 128 K loop of 48 -- while the 16-tile tails of ViT-L's
  // N = 1024 Linears (6 % of the CUs) do: auto mode takes tails of at most a quarter of the CUs whose K loop is long enough
  if (nt_splitk == 1 && (tiles > cus / 4 || nk < 64)) return 0;  // (K = 3072 at 16 tiles: 289 -> 297 us; K = 4096: 424 -> 392, 387 -> 376)
  int64_t s = cus / tiles;
  if (s > nk / 2) s = nk / 2;
  if (s > 8) s = 8;
  return s < 2 ? 0 : (int)s;
}
static size_t nt_splitk_ws_bytes(int64_t tiles, int shares) { return SK_HEADER_BYTES + (size_t)(tiles * shares) * SK_TILE_BYTES; }

// rows [.., .. + rows) of the problem as a problem of its own (every range of a problem has the problem's operands and epilogue)
static NtDesc row_range(const NtDesc& p, int64_t rows) {
  NtDesc q = p;
  q.M = rows;
  return q;
}

// splits for a tail of `tiles` 256 x 256 tiles with nk K-tiles each, or 0: the combine pass costs ~14 us (partial tiles written and read back,
// arrival wait), so short reductions gain nothing.  *ws_short: the bytes a split needs where the workspace on offer is smaller.
static int nt_splitk_plan(const NtDesc& t, double* cost_us, size_t* ws_short) {
  const int tiles = (int)((t.M + 255) / 256) * ((t.N + 255) / 256), nk = t.K / BK;
  // Deferred plan (nt_sk_defer, nt_plan): the partial tiles are left by a launch IN FRONT of the whole-round launch and combined by a
  // launch BEHIND it, so their way through memory (58 MB each way for 76 tiles x 3 shares) runs beside two rounds of matrix work instead of
  // at the end of a 26 us kernel.  Measured (kernel trace, ViT-B dX(fc1), 76 tiles x 3 shares): partial-tile launch 54 us with write-through
  // stores, whole rounds 190, combine 15 -- against 190 + 47 for the 256 x 128 tail: the 58 MB of partial tiles cost what the balanced
  // K loop saves, so the rule for WHICH tails split stays what it was; the deferred form is the better way to run those that do
  // (ViT-L fc2 421 -> 388 us against 392 combined in the launch, dX(fc1) 387 -> 364 against 376).
  if (!((t.epi == EPI_PLAIN) || (t.epi == EPI_RESIDUAL && !t.out16 && t.res_mod <= 0))) return 0;
  if (t.rowscale && t.rows_per_scale < 256) return 0;
  if (t.colscale_cols > 0) return 0;
  const int s = nt_splitk_shares(tiles, nk);
  if (!s) return 0;
  // (a workspace was handed in but is smaller than tad_linear_workspace_bytes says for this shape under the current knobs: the executor says so
  //  once, nt_warn_ws_short, instead of silently running the unsplit tail)
  if (t.ws_bytes < nt_splitk_ws_bytes(tiles, s)) { *ws_short = nt_splitk_ws_bytes(tiles, s); return 0; }
  *cost_us = nt_sk_defer ? (double)((nk + s - 1) / s) * 1.45 + 10.0 + 16.0 : (double)((nk + s - 1) / s) * 1.65 + 14.0 + 3.0;
  return s;
}
void nt_warn_ws_short(const NtDesc& d, const NtPlan& plan) {
  static bool warned = false;
  if (warned || !plan.ws_short) return;
  warned = true;
  fprintf(stderr, "[tad] gemm_nt: split-K workspace of %zu bytes < the %zu a tail of M=%lld N=%d K=%d needs; running it unsplit\n", d.ws_bytes, plan.ws_short,
          (long long)d.M, d.N, d.K);
}

// Rough cost (us) of one launch on MI355X, from the in-kernel timelines (tools/exp_timeline.py): K-tile of a 256 x 256 tile
// 1.65 us, of a 256 x 128 tile 1.06 us; epilogue per tile by kind.  Only used to rank plans.
static double nt_cost(int v, int epi, int64_t M, int N, int K) {
  const int cus = cu_count();
  const double nk = K / 64;
  if (v == 1) {
    const double epi_us = (epi == EPI_GELU || epi == EPI_DGELU) ? 9.0 : (epi == EPI_RESIDUAL ? 12.5 : 4.5);
    const int64_t tiles = (int64_t)((M + 255) / 256) * ((N + 255) / 256);
    return (double)((tiles + cus - 1) / cus) * (nk * 1.65 + epi_us) + 3.0;
  }
  if (v == 3) {
    const double epi_us = (epi == EPI_GELU || epi == EPI_DGELU) ? 5.5 : (epi == EPI_RESIDUAL ? 6.5 : 3.0);
    const int64_t tiles = (int64_t)((M + 255) / 256) * ((N + 127) / 128);
    return (double)((tiles + cus - 1) / cus) * (nk * 1.06 + epi_us) + 3.0;
  }
  if (v == 8) {  // 192 x 128: 7 / 8 of the 256 x 128 tile's time per K-tile for 3 / 4 of its rows (tools/exp_tail_tile.py)
    const double epi_us = (epi == EPI_GELU || epi == EPI_DGELU) ? 4.5 : (epi == EPI_RESIDUAL ? 5.5 : 2.5);
    const int64_t tiles = (int64_t)((M + 191) / 192) * ((N + 127) / 128);
    return (double)((tiles + cus - 1) / cus) * (nk * 0.93 + epi_us) + 3.0;
  }
  const int64_t tiles = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
  return (double)((tiles + 2 * cus - 1) / (2 * cus)) * (nk * 1.3 + 5.0) + 3.0;
}
// The tile of a tail launch of the split plan (a problem of at least 2048 rows that fills less than a round of 256 x 256 tiles): 256 x 256,
// 256 x 128, or -- tad_linear_tuning("tail_192", 1), default -- 192 x 128 where that puts more CUs to work (ViT-B's N = 768 Linears:
// 6656 rows = 156 tiles of 256 x 128 on 256 CUs, or 210 of 192 x 128: the five tails of a block 146.4 -> 132.9 us, bit-identical)
static int nt_tail_variant(const NtDesc& t) {
  const double c1 = nt_cost(1, t.epi, t.M, t.N, t.K), c3 = nt_cost(3, t.epi, t.M, t.N, t.K);
  const double c8 = nt_tail_192 ? nt_cost(8, t.epi, t.M, t.N, t.K) : 1e300;
  const bool v1_ok = !(t.epi == EPI_RESIDUAL && (t.out16 || t.res_mod > 0));
  if (c8 < c3 && (c8 < c1 || !v1_ok)) return 8;
  return (c1 < c3 && v1_ok) ? 1 : 3;
}

// Which 256 x 256 kernel runs the whole rounds of a planned launch: the eight-wave one (1), or -- tad_linear_tuning("w4_plain", K_min): for
// bias-only epilogues whose reduction is at least K_min long -- the four-wave one (7), whose faster K loop outweighs its slower epilogue only
// on long reductions (csrc/gemm_w4.hip; bit-identical either way)
static int nt_main_variant(const NtDesc& p) {
  if (p.K < 2 * BK) return 1;
  if (p.epi == EPI_PLAIN) return (nt_w4_plain > 0 && p.K >= nt_w4_plain) ? 7 : 1;
  // the other epilogues: tad_linear_tuning("w4_epilogues", mask) -- bit 1 GELU, 2 residual (f32 output), 3 GELU backward
  const int bit = p.epi == EPI_GELU ? 1 : (p.epi == EPI_RESIDUAL && !p.out16 && p.res_mod <= 0) ? 2 : p.epi == EPI_DGELU ? 3 : -1;
  return (bit > 0 && ((nt_w4_epilogues >> bit) & 1) && nt_w4_plain > 0 && p.K >= nt_w4_plain) ? 7 : 1;
}

// Tile configurations.  1 = 256x256 (2x4 waves) 2 stages; 2 = 128x128 (2x2) 2 stages, 2 workgroups/CU; 3 = 256x128 (4x2) 3 stages; 4 = 128x64,
// 5 = 64x64 (2x2 waves, 2 stages: small problems); 7 = 256x256 as four waves (gemm_w4.hip); 8 = 192x128 (4x2 waves, 3 stages); 9 = 192x128 as four
// waves (2x2 of 96x64, 2 stages of 40 KiB: two workgroups per CU).  The epilogue kind and output type are compile-time (the epilogue is VALU-bound).
// Variants 1, 3 and 7 run as persistent kernels (one workgroup per CU walks a tile list) once there are more than 1.5 tiles per CU.
// The launch of rows [r0, r0 + p.M) of a problem with tile configuration v wished for: what is instantiated and legal for this epilogue decides.
static NtStep nt_step(const NtDesc& p, int64_t r0, int v) {
  const int epi = (p.epi == EPI_RESIDUAL && p.residual && p.res_mod > 0) ? EPI_RESMOD : p.epi;
  const int M = (int)p.M;
  auto tiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((p.N + bn - 1) / bn); };
  if (((epi == EPI_RESIDUAL && p.out16) || epi == EPI_RESMOD) && (v == 1 || v == 7)) v = 3;  // (not instantiated: no registers / never needed)
  if (v != 2 && v != 4 && v != 5 && p.rowscale && p.rows_per_scale < 256) v = 2;  // the 256-row tiles take at most two row-scale groups per tile
  const int grid_p = persistent_grid();
  auto persists = [&](int bn) { return nt_persist && grid_p >= 8 && tiles(256, bn) > grid_p + grid_p / 2; };
  NtStep s{};
  s.r0 = (int)r0;
  s.rows = M;
  s.kernel = v;
  s.group_m = nt_group_m(p.K);
  s.epi = epi;
  // measured per shape (tools/exp_epilogue.py): storing straight from the MFMA layout wins only for the bias-only bf16 epilogue
  // (nothing to fetch, no arithmetic); the others keep the LDS transposition.  nt_direct: 0 = never, 1 = auto, 2 = always.
  s.direct = nt_direct == 2 || (nt_direct == 1 && epi == EPI_PLAIN && p.out16);
  s.block = 512;
  switch (v) {
    case 1: s.persist = persists(256); s.grid = s.persist ? grid_p : tiles(256, 256); break;
    case 3: s.persist = persists(128); s.grid = s.persist ? grid_p : tiles(256, 128); break;
    case 7:  // the four-wave 256 x 256 kernels never store directly; their K loop is written for >= 2 K-tiles: a single one runs on the eight-wave kernel
      s.direct = 0;
      if (p.K < 2 * BK) { s.kernel = 1; s.grid = tiles(256, 256); break; }
      s.persist = persists(256); s.grid = s.persist ? grid_p : tiles(256, 256); s.block = 256;
      break;
    case 8: s.grid = tiles(192, 128); break;  // tails of the split plan whose 256 x 128 tiles would leave > a third of the CUs idle
    case 9: s.grid = tiles(192, 128); s.block = 256; break;  // the short-K plan
    case 4: s.grid = tiles(128, 64); s.block = 256; break;
    case 5: s.grid = tiles(64, 64); s.block = 256; break;
    default: s.kernel = 2; s.grid = tiles(128, 128); s.block = 256; break;
  }
  return s;
}
// Split-K launch of a (small) problem: tiles x splits workgroups, all resident (nt_splitk_shares checked tiles * splits <= CUs)
static NtStep nt_splitk_step(const NtDesc& t, int64_t r0, int splits, int mode) {
  NtStep s{};
  s.r0 = (int)r0;
  s.rows = (int)t.M;
  s.kernel = NT_SPLITK;
  s.grid = (int)((t.M + 255) / 256) * ((t.N + 255) / 256) * splits;
  s.block = 512;
  s.group_m = nt_group_m(t.K);
  s.sk_splits = splits;
  s.sk_mode = mode;
  s.epi = t.epi;
  return s;
}

int nt_validate(const NtDesc& p) {
  if (!(p.M > 0 && p.N > 0 && p.K > 0)) { set_error("gemm_nt: empty problem"); return TAD_EINVAL; }
  if (p.K % BK) { set_error("gemm_nt: K=%d must be a multiple of %d", p.K, BK); return TAD_EINVAL; }
  if (p.N % 4) { set_error("gemm_nt: N=%d must be a multiple of 4", p.N); return TAD_EINVAL; }
  if ((int64_t)p.N * p.K * 2 >= (1ll << 32)) { set_error("gemm_nt: weight operand exceeds 4 GiB"); return TAD_EINVAL; }
  if (nt_max_rows(p.N, p.K, (p.out16 && !p.residual) ? 2 : 4) <= 0) { set_error("gemm_nt: N=%d / K=%d too wide for the 32-bit operand offsets", p.N, p.K); return TAD_EINVAL; }
  return TAD_OK;
}

NtPlan nt_plan(const NtDesc& d, int64_t r0) {
  // The kernel addresses A through a buffer descriptor with 32-bit byte offsets (< 4 GiB), and C -- with the residual / pre-activation
  // operands, which have C's shape -- through descriptors whose out-of-range lanes get offset 0x80000000, so every real offset,
  // including the rows of the last, partly filled tile, must stay below 2^31: (M + 256) * N * element size < 2 GiB with the element
  // size of the widest operand the epilogue touches (4 for an f32 output or an f32 residual, else 2).  Rows are independent, so a
  // taller problem runs as row ranges that fit (ViT-B fc1, N = 3072 bf16: 222 clips of 1568 tokens per range; the f32 cap used to
  // apply to bf16 outputs too and refused B > 111).
  const int64_t max_rows = nt_max_rows(d.N, d.K, (d.out16 && !d.residual) ? 2 : 4);
  const NtDesc p = row_range(d, (d.M - r0) < max_rows ? (d.M - r0) : max_rows);
  NtPlan plan{};
  plan.next = r0 + p.M;
  auto one = [&](int v) { plan.step[plan.n++] = nt_step(p, r0, v); return plan; };
  if (nt_variant) return one(nt_variant);
  if (p.M < 2048 || p.N < 128) {
    // small problems (batch-1 inference: 1568 or 784 rows): 128 x 128 tiles, or 128 x 64 when those would leave more than half of the
    // CUs without a workgroup (ViT-B proj / fc2 at 1568 rows: 78 tiles of 128 x 128)
    const int64_t t128 = (int64_t)((p.M + 127) / 128) * ((p.N + 127) / 128);
    const int64_t t64 = (int64_t)((p.M + 127) / 128) * ((p.N + 63) / 64);
    if (t128 * 2 > cu_count() || p.N < 64) return one(2);
    return one((t64 * 4 <= 3 * cu_count() && p.M >= 64) ? 5 : 4);  // 64 x 64 while even 128 x 64 fills < 3/4 of the CUs
  }
  // Short reductions (ViT-S: K = 384; the MAE decoder: K = 512): the epilogue is as long as the K loop, and tiles that put TWO workgroups on a CU
  // let one's epilogue run beside the other's K loop: 192 x 128 as four waves of 96 x 64 (variant 9: 80 KiB of LDS, <= 210 registers) or
  // 128 x 128 (variant 2).  Measured (tools/exp_gemm_knobs.py --D 384 / 512 --configs "variant=0;variant=9;variant=2"), us, planned 256 x 256 /
  // variant 9 / variant 2 -- K = 512: fc1 + GELU 171 / 152 / 161, dX(fc2) GELU' 165 / 151 / 159, the bias-only and residual shapes 1-7 % slower on
  // either; K = 384: qkv 60.0 / 58.5 / 62, fc1 + GELU 102 / 98.6 / 100, dX(fc2) 99 / 97 / 100.5, dX(proj) 28.5 / 25.0 / 24.8, proj + residual
  // 41.0 / 38 / 36 (N = 384 is 1.5 tiles of 256 columns).  From K = 768 the 256 x 256 tile wins everywhere (fc1 274 / 277 / 290)
  if (nt_short_k && p.K <= 512 && !(p.rowscale && p.rows_per_scale < 256)) {
    const bool act = p.epi == EPI_GELU || p.epi == EPI_DGELU;
    if (p.epi == EPI_RESIDUAL && p.K < 512) return one(2);
    if (act || (p.epi == EPI_PLAIN && p.K < 512)) return one(9);
  }
  const bool v1_ok = !(p.epi == EPI_RESIDUAL && (p.out16 || p.res_mod > 0));  // (those instantiations do not exist)
  // Plans: (a) 256 x 128 tiles, (b) 256 x 256 tiles, (c) 256 x 256 tiles for as many row panels as fill whole rounds of one
  // workgroup per CU, the remaining rows as a second launch with whatever suits that smaller problem.  (c) is what lets the
  // N = 768 Linears of ViT-B use the (27 % faster per flop) 256 x 256 tile: 196 x 3 tiles are 2.3 rounds of 256 workgroups.
  const double cost_a = nt_cost(3, p.epi, p.M, p.N, p.K);
  const double cost_b = v1_ok ? nt_cost(1, p.epi, p.M, p.N, p.K) : 1e300;
  double cost_c = 1e300;
  int main_rows = 0, tail_splits = 0;
  if (v1_ok && nt_split) {
    main_rows = nt_main_rows(p.M, p.N, nullptr);
    if (main_rows > 0) {
      const NtDesc t = row_range(p, p.M - main_rows);
      double tail_cost = t.M < 2048 ? nt_cost(2, p.epi, t.M, p.N, p.K) : nt_cost(nt_tail_variant(t), p.epi, t.M, p.N, p.K);
      // (d) the tail's tiles split along K over all CUs (SPLITK kernels): 78 tiles of the N = 768 Linears of ViT-B run as 3 shares
      // each on 234 CUs instead of one K loop on 156
      if (p.ws_bytes) {
        double sk_cost = 1e300;
        const int s = nt_splitk_plan(t, &sk_cost, &plan.ws_short);
        if (s && (sk_cost < tail_cost || nt_splitk == 2)) { tail_splits = s; tail_cost = sk_cost; }
      }
      cost_c = nt_cost(1, p.epi, main_rows, p.N, p.K) + tail_cost;
    }
  }
  if (nt_split == 2 && main_rows > 0) cost_c = 0.0;  // forced (experiments)
  if (!(cost_c < cost_a && cost_c < cost_b)) return one(cost_b < cost_a ? nt_main_variant(p) : 3);
  const NtDesc t = row_range(p, p.M - main_rows);
  const NtStep main = nt_step(row_range(p, main_rows), r0, nt_main_variant(p));
  const int64_t rt = r0 + main_rows;
  if (tail_splits && nt_sk_defer) {  // partial tiles of the tail | whole rounds | combine + epilogue of the tail
    plan.step[plan.n++] = nt_splitk_step(t, rt, tail_splits, 1);
    plan.step[plan.n++] = main;
    plan.step[plan.n++] = nt_splitk_step(t, rt, tail_splits, 2);
    return plan;
  }
  plan.step[plan.n++] = main;
  if (tail_splits) plan.step[plan.n++] = nt_splitk_step(t, rt, tail_splits, 0);
  else plan.step[plan.n++] = nt_step(t, rt, t.M < 2048 ? 2 : nt_tail_variant(t));
  return plan;
}

// ---- gemm_tn.  Tiles: 1 = 256x256 (2x4) 2 stages; 3 = 256x128 (4x2) 3 stages.  Splits over the reduction dim target ~1 workgroup per CU.
// TAD_GEMM_TN_VARIANT forces one; by default the 128-wide tile serves shapes whose K the 256-wide one would pad by a third or more
// (K = 384 = 1.5 tiles: ViT-S -- the weight gradients of its qkv / proj / fc1 Linears computed 2 x 256 columns for 384)
static int tn_variant_of(int K) {
  if (knobs::tn_variant) return knobs::tn_variant;
  const int pad256 = (K + 255) / 256 * 256, pad128 = (K + 127) / 128 * 128;
  return (K > 0 && pad256 * 3 >= pad128 * 4) ? 3 : 1;
}
// One workgroup per CU is resident (128 KiB of LDS), so the grid runs in rounds of cu_count() workgroups and a grid of
// cu_count() + 1 costs two full rounds.  Pick the split count that minimises rounds x (reduction tiles per split + epilogue)
// plus the slab-reduce pass, all in units of one reduction tile (~2 us on MI355X).
TnPlan tn_plan(int64_t Mr, int N, int K, int N1, size_t ws_bytes) {
  TnPlan t{};
  const int variant = tn_variant_of(K);
  t.bn = variant != 3 ? 256 : 128;
  t.tiles_k = (K + t.bn - 1) / t.bn;
  t.tiles = ((N + 255) / 256) * t.tiles_k;
  const int64_t ktiles = (Mr + BK - 1) / BK;
  const int cus = cu_count();
  const double epi_units = 6.0;                                            // accumulator store of one workgroup
  const double reduce_units = (double)N * (double)K * 8.0 / 4.0e12 / 2.0e-6;  // slab write + read per split
  int best = 1;
  double best_cost = 1e300;
  for (int s = 1; s <= 64 && s <= ktiles; ++s) {
    const int64_t per = (ktiles + s - 1) / s;
    const int s_eff = (int)((ktiles + per - 1) / per);
    if (s_eff != s) continue;
    const int64_t rounds = ((int64_t)t.tiles * s + cus - 1) / cus;
    const double cost = (double)rounds * ((double)per + epi_units) + (s > 1 ? s * reduce_units : 0.0);
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  t.splits = best;
  t.rows_per_split = (int)((ktiles + best - 1) / best * BK);
  t.ws_bytes = (size_t)t.splits * ((size_t)N * (size_t)K + (size_t)t.tiles_k * (size_t)N) * sizeof(float);
  // 256 x 256 tiles: the four-wave kernel (gemm_w4.hip; bit-identical results) unless switched off (tad_linear_tuning("tn_w4", 0)); its loop
  // is written for at least two reduction tiles per workgroup
  if (variant == 1 && knobs::tn_w4 && !knobs::tn_pdeep && t.rows_per_split >= 2 * BK && !gemm_debug) t.kernel = TN_W4;
  else if (variant == 1) t.kernel = knobs::tn_pdeep ? TN_PDEEP : TN_W8;
  else t.kernel = TN_W8_128;
  t.grid = t.tiles * t.splits;
  t.block = t.kernel == TN_W4 ? 256 : 512;
  // a pair fits the one kernel that takes it when no tile straddles the two problems, its operands stay within the 32-bit offsets and the
  // workspace holds the slabs of both
  t.fits = N1 > 0 && knobs::tn_pair && t.kernel == TN_W4 && N1 % 256 == 0 && Mr * (int64_t)N * 2 < (1ll << 32) && Mr * (int64_t)K * 2 < (1ll << 32) &&
           ws_bytes >= t.ws_bytes;
  return t;
}

}  // namespace tad

using namespace tad;

extern "C" {

int tad_linear_tuning(const char* key, int value) {
  TAD_REQUIRE(!(key && !strcmp(key, "variant") && value == 6), "linear_tuning: variant=%d not one of 0..5, 7, 8, 9", value);
  return knob_set(KNOBS, "linear_tuning", key, value);
}

int tad_linear_tuning_get(const char* key, int* value) { return knob_get(KNOBS, "linear_tuning_get", key, value); }

long long tad_linear_kernel_launches(void) { return nt_launches; }

int tad_linear_debug_stamps(void* buf) {
#ifndef TAD_GEMM_ABLATION
  if (buf) { set_error("linear_debug_stamps: timeline stamps need an ablation build (TAD_BUILD_ABLATION=1 python -m simple_tad_amd.build --force)"); return TAD_EINVAL; }
#endif
  nt_stamps = (unsigned long long*)buf;
  return TAD_OK;
}

size_t tad_linear_workspace_bytes(int64_t M, int N, int K) {
  // What nt_plan's split plan hands to nt_splitk_plan for this shape (same helpers: nt_max_rows, nt_main_rows, nt_splitk_shares; the
  // epilogue kind is not known here: assumed eligible, and both element sizes of the row-range rule are covered), or 0 when no tail of this
  // shape splits along K -- every Linear of ViT-B under the default knobs (64 MB used to stay resident per stream for nothing)
  if (M < 4096 || N < 128 || K <= 0 || K % BK || !nt_split || !nt_splitk) return 0;
  size_t need = 0;
  for (int64_t esz = 2; esz <= 4; esz += 2) {
    const int64_t max_rows = nt_max_rows(N, K, esz);
    if (max_rows <= 0) continue;
    for (int64_t r0 = 0; r0 < M; r0 += max_rows) {  // the row ranges a taller problem is cut into (two distinct sizes at most)
      const int64_t rows = (M - r0) < max_rows ? (M - r0) : max_rows;
      if (r0 > 0 && rows == max_rows) continue;
      int64_t tiles = 0;
      if (rows < 2048 || !nt_main_rows(rows, N, &tiles)) continue;
      const int s = nt_splitk_shares(tiles, K / BK);
      if (s && nt_splitk_ws_bytes(tiles, s) > need) need = nt_splitk_ws_bytes(tiles, s);
    }
  }
  return need;
}

size_t tad_linear_bwd_weight_workspace_bytes(int64_t M, int N, int K) { return tn_plan(M, N, K).ws_bytes; }
size_t tad_patch_embed_bwd_workspace_bytes(int64_t M, int D, int K) { return tad_linear_bwd_weight_workspace_bytes(M, D, K); }

int tad_linear_plan(int64_t M, int N, int K, int epilogue, int out_16bit, int has_residual, int res_mod, int has_rowscale, int rows_per_scale,
                    int colscale_cols, size_t ws_bytes, int32_t* steps, int capacity) {
  TAD_REQUIRE(steps || capacity <= 0, "linear_plan: null buffer");
  TAD_REQUIRE(epilogue >= EPI_PLAIN && epilogue <= EPI_DGELU, "linear_plan: bad epilogue %d", epilogue);
  TAD_REQUIRE(M > 0 && M < (1ll << 31), "linear_plan: bad M");
  const NtDesc d{M, N, K, epilogue, out_16bit != 0, has_residual != 0, res_mod, has_rowscale != 0, rows_per_scale > 0 ? rows_per_scale : 1, colscale_cols, ws_bytes};
  if (const int rc = nt_validate(d)) return rc;
  int n = 0;
  for (int64_t r0 = 0; r0 < d.M;) {
    const NtPlan plan = nt_plan(d, r0);
    for (int i = 0; i < plan.n; ++i, ++n)
      if (n < capacity) memcpy(steps + (size_t)n * NT_STEP_WORDS, &plan.step[i], sizeof(NtStep));
    r0 = plan.next;
  }
  if (n > capacity) { set_error("linear_plan: %d steps, room for %d", n, capacity); return TAD_ENOSPACE; }
  return n;
}

int tad_linear_bwd_weight_plan(int64_t M, int N1, int N2, int K, size_t ws_bytes, int32_t* launches, int capacity) {
  TAD_REQUIRE(launches || capacity <= 0, "linear_bwd_weight_plan: null buffer");
  TAD_REQUIRE(M > 0 && N1 > 0 && N2 >= 0 && K > 0, "linear_bwd_weight_plan: empty problem");
  TAD_REQUIRE(N1 % 8 == 0 && N2 % 8 == 0 && K % 8 == 0, "linear_bwd_weight_plan: N1=%d, N2=%d and K=%d must be multiples of 8", N1, N2, K);
  TnPlan t[2];
  int n = 1;
  t[0] = tn_plan(M, N1 + N2, K, N2 ? N1 : 0, ws_bytes);
  if (N2 && !t[0].fits) { t[0] = tn_plan(M, N1, K); t[1] = tn_plan(M, N2, K); n = 2; }
  if (n > capacity) { set_error("linear_bwd_weight_plan: %d launches, room for %d", n, capacity); return TAD_ENOSPACE; }
  for (int i = 0; i < n; ++i) {
    const int N = n == 2 ? (i ? N2 : N1) : N1 + N2;
    const int32_t row[TAD_LINEAR_BWD_WEIGHT_PLAN_WORDS] = {N, t[i].bn, t[i].tiles, t[i].tiles_k, t[i].splits, t[i].rows_per_split, t[i].kernel, t[i].grid, t[i].block,
                                                           t[i].fits, (int32_t)(t[i].ws_bytes & 0x7fffffff), (int32_t)(t[i].ws_bytes >> 31)};
    memcpy(launches + (size_t)i * TAD_LINEAR_BWD_WEIGHT_PLAN_WORDS, row, sizeof(row));
  }
  return n;
}

}  // extern "C"
