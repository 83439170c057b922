// Host half of the 16-bit-operand GEMMs: the launch planner, the launchers and the C ABI of the Linear layers.  The kernel templates and
// their parameter blocks are in gemm_kernels.h (shared with gemm_w4.hip, the four-wave instantiations).
#include <math.h>
#include <stdlib.h>
#include <string>
#include "gemm_kernels.h"

// Scheduling knobs and counters of the Linear GEMMs (tad_linear_tuning; initial values from the environment).  One copy for the whole
// library: defined by the bf16 compilation pass, shared by the half pass.
namespace tad { namespace knobs {
#ifndef TAD_OPND_F16
static int env_int(const char* name) {
  const char* v = getenv(name);
  return v ? atoi(v) : 0;
}
int gemm_debug = env_int("TAD_GEMM_DEBUG");  // ablation bits (GemmNT::debug); only ablation builds look at them
int nt_persist = !env_int("TAD_GEMM_NO_PERSIST");
int nt_direct = getenv("TAD_GEMM_DIRECT_EPI") ? env_int("TAD_GEMM_DIRECT_EPI") : 1;
int nt_split = getenv("TAD_GEMM_SPLIT_TAIL") ? env_int("TAD_GEMM_SPLIT_TAIL") : 1;
int nt_sk_defer = getenv("TAD_GEMM_SPLITK_DEFER") ? env_int("TAD_GEMM_SPLITK_DEFER") : 1;  // 1 = split-K tails leave their partial tiles in front of the whole-round launch and are combined behind it; 0 = combined inside one launch
int nt_splitk = getenv("TAD_GEMM_SPLITK_TAIL") ? env_int("TAD_GEMM_SPLITK_TAIL") : 1;  // 1 = the tail launch of the split plan may split its tiles along K (needs a workspace); 0 = never; 2 = whenever eligible
int nt_variant = env_int("TAD_GEMM_NT_VARIANT");  // 0 = planned per shape (launch_gemm_nt), else the tile configuration for every launch
int nt_group_m_knob = getenv("TAD_GEMM_GROUP_M") ? env_int("TAD_GEMM_GROUP_M") : 0;  // 0 = per-shape choice (nt_group_m)
int tn_variant = env_int("TAD_GEMM_TN_VARIANT");
// > 0: bias-only Linears with K >= this run their whole rounds on the four-wave kernel.  Measured (tools/exp_w4_plain.py, planned launches at M = 50176):
// qkv forward 176.9 / 177.2 us (eight / four waves), dX(proj) 78.0 / 73.9, dX(qkv) 159.0 / 148.4, dX(fc1) 225.4 / 208.5 -- on by default
int nt_w4_plain = getenv("TAD_GEMM_W4_PLAIN") ? env_int("TAD_GEMM_W4_PLAIN") : 640;  // K_min of the Linears whose whole rounds of 256 x 256 tiles run on the four-wave kernel (0 = none): below ~640 its epilogue costs more than its K loop gains (tools/exp_w4_plain.py --D 384 / 512)
// bit mask: which other epilogues' whole rounds take the four-wave kernel (see nt_main_variant).  Measured (tools/exp_gemm_knobs.py --configs
// "w4_epilogues=0;w4_epilogues=14", eight / four waves): proj + residual 96.0 / 96.9 us, fc2 + residual 250.4 / 241.1, fc1 GELU 278.1 / 282.1, dX(fc2) GELU backward
// 291.2 / 338.8 -- the residual epilogue (bit 2) is on by default, the vector-heavy GELU ones stay on eight waves
int nt_w4_epilogues = getenv("TAD_GEMM_W4_EPILOGUES") ? env_int("TAD_GEMM_W4_EPILOGUES") : 4;
int tn_pair = getenv("TAD_GEMM_TN_PAIR") ? env_int("TAD_GEMM_TN_PAIR") : 1;  // 1: tad_linear_bwd_weight_pair runs its two problems as one launch when they fit (launch_gemm_tn_pair); 0: always two launches
int nt_short_k = getenv("TAD_GEMM_SHORT_K") ? env_int("TAD_GEMM_SHORT_K") : 1;  // 1: the short-K plan of launch_gemm_nt (K <= 512: tiles that put two workgroups on a CU)
int nt_tail_192 = getenv("TAD_GEMM_TAIL_192") ? env_int("TAD_GEMM_TAIL_192") : 1;  // 1: tails of the split plan may run as 192 x 128 tiles (nt_tail_variant)
int tn_w4 = getenv("TAD_GEMM_TN_W4") ? env_int("TAD_GEMM_TN_W4") : 1;  // 1: the 256 x 256 weight-gradient GEMM runs as four waves of 128 x 128 (gemm_w4.hip)
int tn_pdeep = env_int("TAD_GEMM_TN_PDEEP");  // 1: gemm_tn 256 x 256 with the P operand two reduction tiles ahead (see PDEEP); measured null (round 4), off
unsigned long long* nt_stamps = nullptr;
long long nt_launches = 0;  // gemm_nt kernel launches so far (tad_linear_kernel_launches)
#else
extern int gemm_debug, nt_persist, nt_direct, nt_split, nt_splitk, nt_variant, nt_group_m_knob, tn_variant, tn_pdeep, nt_sk_defer, tn_w4, nt_w4_plain, nt_w4_epilogues, nt_tail_192, nt_short_k, tn_pair;
extern unsigned long long* nt_stamps;
extern long long nt_launches;
#endif
}}  // namespace tad::knobs
TAD_NAMESPACE_BEGIN
using namespace knobs;

static int cu_count();

// Row panels per column-panel group of the tile raster.  The ~32 workgroups resident on an XCD (private 4 MiB L2) walk consecutive
// tile ids, so at any time they touch GROUP_M A-panels and ~32 / GROUP_M W-panels; each panel streams K-tile by K-tile, and a
// panel's K-tile is fetched from beyond L2 once per group of tiles that share it while they run together.  Per group of
// GROUP_M x tiles_n tiles that is GROUP_M A-panel loads (algorithmic) + tiles_n W-panel loads (overhead, amortised over GROUP_M).
// Measured (tools/exp_gemm_knobs.py --knob group_m, the eight Linear shapes of a ViT-B block, with the non-temporal output stores in): 2 / 4 / 8 are
// within 0.5 % of each other in sum; the long reductions (K = 2304 / 3072: an A panel of 256 rows is 1.2 - 1.5 MB) are 1 - 4 % faster with 4 (fc2 241
// vs 246 us, dX(fc1) 220 vs 222), the K = 768 shapes with 8 (qkv 166 vs 169).
static int nt_group_m(int tiles_m, int tiles_n, int K) {
  if (nt_group_m_knob > 0) return nt_group_m_knob;
  return K >= 2048 ? 4 : 8;
}


// Tile configurations.  NT: 1 = 256x256 (2x4 waves) 2 stages; 2 = 128x128 (2x2) 2 stages, 2 workgroups/CU;
// 3 = 256x128 (4x2) 3 stages; 4 = 128x64, 5 = 64x64 (2x2 waves, 2 stages: small problems).  0 = auto.  The epilogue kind and output type are compile-time (the epilogue is VALU-bound).
// Variants 1 and 3 run as persistent kernels (one workgroup per CU walks a tile list) once there are more than 1.5 tiles per CU.
template <int EPI, bool OUT_BF16>
static void launch_nt_variant(int v, GemmNT& p, hipStream_t st) {
  auto tiles = [&](int bm, int bn) { return ((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); };
  const int no_persist = !nt_persist;
  if (((EPI == EPI_RESIDUAL && OUT_BF16) || EPI == EPI_RESMOD) && (v == 1 || v == 7)) v = 3;  // (not instantiated: no registers / never needed)
  if (v != 2 && v != 4 && v != 5 && p.rowscale && p.rows_per_scale < 256) v = 2;  // the 256-row tiles take at most two row-scale groups per tile
  const int grid_p = cu_count() & ~7;
  const int bn = v == 1 ? 256 : 128;
  const bool persist = !no_persist && (v == 1 || v == 3) && grid_p >= 8 && tiles(256, bn) > grid_p + grid_p / 2;
  p.group_m = nt_group_m((p.M + 255) / 256, (p.N + bn - 1) / bn, p.K);
#define NT_LAUNCH(BM_, BN_, WM_, WN_, ST_, PER_, DIR_, GRID_, THREADS_)                                                              \
  hipLaunchKernelGGL((gemm_nt_kernel<BM_, BN_, WM_, WN_, ST_, EPI, OUT_BF16, PER_, DIR_>), dim3(GRID_), dim3(THREADS_), 0, st, p)
  // measured per shape (tools/exp_epilogue.py): storing straight from the MFMA layout wins only for the bias-only bf16 epilogue
  // (nothing to fetch, no arithmetic); the others keep the LDS transposition.  nt_direct: 0 = never, 1 = auto, 2 = always.
  const bool direct = nt_direct == 2 || (nt_direct == 1 && EPI == EPI_PLAIN && OUT_BF16);
  switch (v) {
    case 1:
      if constexpr (!(EPI == EPI_RESIDUAL && OUT_BF16) && EPI != EPI_RESMOD) {
        if (persist) { if (direct) NT_LAUNCH(256, 256, 2, 4, 2, true, true, grid_p, 512); else NT_LAUNCH(256, 256, 2, 4, 2, true, false, grid_p, 512); }
        else { if (direct) NT_LAUNCH(256, 256, 2, 4, 2, false, true, tiles(256, 256), 512); else NT_LAUNCH(256, 256, 2, 4, 2, false, false, tiles(256, 256), 512); }
      }
      break;
    case 3:
      if (persist) { if (direct) NT_LAUNCH(256, 128, 4, 2, 3, true, true, grid_p, 512); else NT_LAUNCH(256, 128, 4, 2, 3, true, false, grid_p, 512); }
      else { if (direct) NT_LAUNCH(256, 128, 4, 2, 3, false, true, tiles(256, 128), 512); else NT_LAUNCH(256, 128, 4, 2, 3, false, false, tiles(256, 128), 512); }
      break;
    case 7: {  // the four-wave 256 x 256 kernels (gemm_w4.hip); persistent under the same rule as variant 1
      if (p.K < 2 * BK) { NT_LAUNCH(256, 256, 2, 4, 2, false, false, tiles(256, 256), 512); break; }  // (its K loop is written for >= 2 K-tiles)
      const bool per7 = !no_persist && grid_p >= 8 && tiles(256, 256) > grid_p + grid_p / 2;
      (void)launch_gemm_nt_w4(p, per7 ? grid_p : 0, st);
      break;
    }
    case 8:  // 192 x 128 (4 x 2 waves, 3 stages): tails of the split plan whose 256 x 128 tiles would leave > a third of the CUs idle
      if (direct) NT_LAUNCH(192, 128, 4, 2, 3, false, true, tiles(192, 128), 512); else NT_LAUNCH(192, 128, 4, 2, 3, false, false, tiles(192, 128), 512);
      break;
    case 9:  // 192 x 128 as FOUR waves (2 x 2 of 96 x 64), 2 stages of 40 KiB: two workgroups per CU (the short-K plan of launch_gemm_nt)
      if (direct) NT_LAUNCH(192, 128, 2, 2, 2, false, true, tiles(192, 128), 256); else NT_LAUNCH(192, 128, 2, 2, 2, false, false, tiles(192, 128), 256);
      break;
    case 4:
      if (direct) NT_LAUNCH(128, 64, 2, 2, 2, false, true, tiles(128, 64), 256); else NT_LAUNCH(128, 64, 2, 2, 2, false, false, tiles(128, 64), 256);
      break;
    case 5:
      if (direct) NT_LAUNCH(64, 64, 2, 2, 2, false, true, tiles(64, 64), 256); else NT_LAUNCH(64, 64, 2, 2, 2, false, false, tiles(64, 64), 256);
      break;
    default:
      if (direct) NT_LAUNCH(128, 128, 2, 2, 2, false, true, tiles(128, 128), 256); else NT_LAUNCH(128, 128, 2, 2, 2, false, false, tiles(128, 128), 256);
      break;
  }
#undef NT_LAUNCH
}

// Split-K launch of a (small) problem: tiles x splits workgroups, all resident (the caller checked tiles * splits <= CUs).  Workspace:
// [arrival counters, one per tile | error word][partial tiles].  The counters are zeroed on the stream in front of the launch.
constexpr size_t SK_HEADER_BYTES = 4096;  // counters (<= 1008 tiles)
constexpr size_t SK_TILE_BYTES = 256 * 256 * sizeof(float);
// The in-launch combine (mode 0) waits for the other shares of its tile with a bounded spin; a share that never arrives (the grid was
// not co-resident: a side stream or another process held CUs) leaves stale partial sums in the output.  The kernel then sets this word,
// which lives in pinned, device-mapped host memory so that the host can see it without a synchronisation: every later gemm_nt launch
// checks it first and returns TAD_ELAUNCH (the word used to sit in the workspace, where nobody read it).
static unsigned* sk_error_word(unsigned** dev_ptr) {
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
  if (dev_ptr) *dev_ptr = dev;
  return host;
}
static bool sk_error_pending_armed = false;  // (the word exists only once a mode-0 launch has been made)
static int sk_check_pending_error() {
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

static int launch_gemm_nt_splitk(GemmNT p, int splits, void* ws, hipStream_t st, int mode = 0) {
  ++nt_launches;
  const int tiles = ((p.M + 255) / 256) * ((p.N + 255) / 256);
  p.sk_splits = splits;
  p.sk_mode = mode;
  p.sk_cnt = (unsigned*)ws;
  p.sk_err = nullptr;
  if (mode == 0) {
    if (!sk_error_word(&p.sk_err)) { set_error("gemm_nt: split-K error word allocation failed"); return TAD_ELAUNCH; }
    sk_error_pending_armed = true;
  }
  p.sk_ws = (float*)((char*)ws + SK_HEADER_BYTES);
  p.group_m = nt_group_m((p.M + 255) / 256, (p.N + 255) / 256, p.K);
  if (mode == 0 && hipMemsetAsync(ws, 0, SK_HEADER_BYTES, st) != hipSuccess) { set_error("gemm_nt: split-K counter reset failed"); return TAD_ELAUNCH; }
  const dim3 grid(tiles * splits), block(512);
  if (p.epi == EPI_PLAIN && p.c_bf16) hipLaunchKernelGGL((gemm_nt_kernel<256, 256, 2, 4, 2, EPI_PLAIN, true, false, false, true>), grid, block, 0, st, p);
  else if (p.epi == EPI_PLAIN) hipLaunchKernelGGL((gemm_nt_kernel<256, 256, 2, 4, 2, EPI_PLAIN, false, false, false, true>), grid, block, 0, st, p);
  else if (p.epi == EPI_RESIDUAL && !p.c_bf16) hipLaunchKernelGGL((gemm_nt_kernel<256, 256, 2, 4, 2, EPI_RESIDUAL, false, false, false, true>), grid, block, 0, st, p);
  else { set_error("gemm_nt: no split-K kernel for epilogue %d", p.epi); return TAD_EINVAL; }
  return check_launch("gemm_nt_splitk");
}
// ---- geometry of the split plan, ONE copy for launch_gemm_nt, nt_splitk_plan and tad_linear_workspace_bytes (the workspace query
// used to restate it, and any drift made the split-K tail drop out without a diagnostic)
// Largest row count one launch may cover (32-bit operand offsets, see launch_gemm_nt); esz = bytes of the widest element the epilogue touches
static int64_t nt_max_rows(int N, int K, int64_t esz) {
  int64_t max_rows = ((1ll << 31) - 1) / ((int64_t)N * esz) - 256;
  const int64_t a_rows = ((1ll << 32) - 1) / ((int64_t)K * 2);
  if (a_rows < max_rows) max_rows = a_rows;
  return max_rows / 256 * 256;
}
// Rows that fill whole rounds of one 256 x 256 tile per CU (0: the split plan does not apply); *tail_tiles = the 256 x 256 tiles left behind them
static int nt_main_rows(int64_t M, int N, int64_t* tail_tiles) {
  const int grid = cu_count() & ~7;
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

// splits for a tail of `tiles` 256 x 256 tiles with nk K-tiles each, or 0: the combine pass costs ~14 us (partial tiles written and read back,
// arrival wait), so short reductions gain nothing
static int nt_splitk_plan(const GemmNT& t, size_t ws_bytes, double* cost_us) {
  const int tiles = ((t.M + 255) / 256) * ((t.N + 255) / 256), nk = t.K / BK;
  // Deferred plan (nt_sk_defer, launch_gemm_nt): the partial tiles are left by a launch IN FRONT of the whole-round launch and combined by a
  // launch BEHIND it, so their way through memory (58 MB each way for 76 tiles x 3 shares) runs beside two rounds of matrix work instead of
  // at the end of a 26 us kernel.  Measured (kernel trace, ViT-B dX(fc1), 76 tiles x 3 shares): partial-tile launch 54 us with write-through
  // stores, whole rounds 190, combine 15 -- against 190 + 47 for the 256 x 128 tail: the 58 MB of partial tiles cost what the balanced
  // K loop saves, so the rule for WHICH tails split stays what it was; the deferred form is the better way to run those that do
  // (ViT-L fc2 421 -> 388 us against 392 combined in the launch, dX(fc1) 387 -> 364 against 376).
  if (!((t.epi == EPI_PLAIN) || (t.epi == EPI_RESIDUAL && !t.c_bf16 && t.res_mod <= 0))) return 0;
  if (t.rowscale && t.rows_per_scale < 256) return 0;
  if (t.colscale_cols > 0) return 0;
  const int s = nt_splitk_shares(tiles, nk);
  if (!s) return 0;
  if (ws_bytes < nt_splitk_ws_bytes(tiles, s)) {
    // (a workspace was handed in but is smaller than tad_linear_workspace_bytes says for this shape under the current knobs: say so once instead
    //  of silently running the unsplit tail)
    static bool warned = false;
    if (!warned) { warned = true; fprintf(stderr, "[tad] gemm_nt: split-K workspace of %zu bytes < the %zu the tail of M=%d N=%d K=%d needs; running it unsplit\n", ws_bytes, nt_splitk_ws_bytes(tiles, s), t.M, t.N, t.K); }
    return 0;
  }
  *cost_us = nt_sk_defer ? (double)((nk + s - 1) / s) * 1.45 + 10.0 + 16.0 : (double)((nk + s - 1) / s) * 1.65 + 14.0 + 3.0;
  return s;
}

static int launch_gemm_nt_one(GemmNT p, int v, hipStream_t st) {
  ++nt_launches;
  if (p.epi == EPI_RESIDUAL && p.residual && p.res_mod > 0) p.epi = EPI_RESMOD;
#define NT_CASE(E)                                                       \
  case E:                                                                \
    if (p.c_bf16) launch_nt_variant<E, true>(v, p, st);                  \
    else launch_nt_variant<E, false>(v, p, st);                          \
    break;
  switch (p.epi) {
    NT_CASE(EPI_PLAIN)
    NT_CASE(EPI_GELU)
    NT_CASE(EPI_RESIDUAL)
    NT_CASE(EPI_DGELU)
    NT_CASE(EPI_RESMOD)
    default: set_error("gemm_nt: bad epilogue %d", p.epi); return TAD_EINVAL;
  }
#undef NT_CASE
  return check_launch("gemm_nt");
}

// rows [r0, r0 + rows) of the problem as a problem of its own
static GemmNT row_range(const GemmNT& p, int r0, int rows) {
  GemmNT q = p;
  const size_t esz = p.c_bf16 ? 2 : 4;
  q.M = rows;
  q.row_base = p.row_base + r0;
  q.A = p.A + (size_t)r0 * p.K;
  q.C = (char*)p.C + (size_t)r0 * p.N * esz;
  if (p.residual && p.res_mod <= 0) q.residual = p.residual + (size_t)r0 * p.N;
  if (p.preact) q.preact = p.preact + (size_t)r0 * p.N;
  if (p.dgelu_h) q.dgelu_h = p.dgelu_h + (size_t)r0 * p.N;
  return q;
}

// Rough cost (us) of one launch on MI355X, from the in-kernel timelines (tools/exp_timeline.py): K-tile of a 256 x 256 tile
// 1.65 us, of a 256 x 128 tile 1.06 us; epilogue per tile by kind.  Only used to rank plans.
static double nt_cost(int v, int epi, int c_bf16, int M, int N, int K) {
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
static int nt_tail_variant(const GemmNT& t) {
  const double c1 = nt_cost(1, t.epi, t.c_bf16, t.M, t.N, t.K), c3 = nt_cost(3, t.epi, t.c_bf16, t.M, t.N, t.K);
  const double c8 = nt_tail_192 ? nt_cost(8, t.epi, t.c_bf16, t.M, t.N, t.K) : 1e300;
  const bool v1_ok = !(t.epi == EPI_RESIDUAL && (t.c_bf16 || t.res_mod > 0));
  if (c8 < c3 && (c8 < c1 || !v1_ok)) return 8;
  return (c1 < c3 && v1_ok) ? 1 : 3;
}

// Which 256 x 256 kernel runs the whole rounds of a planned launch: the eight-wave one (1), or -- tad_linear_tuning("w4_plain", K_min): for
// bias-only epilogues whose reduction is at least K_min long -- the four-wave one (7), whose faster K loop outweighs its slower epilogue only
// on long reductions (csrc/gemm_w4.hip; bit-identical either way)
static int nt_main_variant(const GemmNT& p) {
  if (p.K < 2 * BK) return 1;
  if (p.epi == EPI_PLAIN) return (nt_w4_plain > 0 && p.K >= nt_w4_plain) ? 7 : 1;
  // the other epilogues: tad_linear_tuning("w4_epilogues", mask) -- bit 1 GELU, 2 residual (f32 output), 3 GELU backward
  const int bit = p.epi == EPI_GELU ? 1 : (p.epi == EPI_RESIDUAL && !p.c_bf16 && p.res_mod <= 0) ? 2 : p.epi == EPI_DGELU ? 3 : -1;
  return (bit > 0 && ((nt_w4_epilogues >> bit) & 1) && nt_w4_plain > 0 && p.K >= nt_w4_plain) ? 7 : 1;
}

int launch_gemm_nt(const GemmNT& p_in, hipStream_t st, void* ws = nullptr, size_t ws_bytes = 0) {
  GemmNT p = p_in;
  if (const int rc = sk_check_pending_error()) return rc;
  if (!(p.M > 0 && p.N > 0 && p.K > 0)) { set_error("gemm_nt: empty problem"); return TAD_EINVAL; }
  if (p.K % BK) { set_error("gemm_nt: K=%d must be a multiple of %d", p.K, BK); return TAD_EINVAL; }
  if (p.N % 4) { set_error("gemm_nt: N=%d must be a multiple of 4", p.N); return TAD_EINVAL; }
  if ((int64_t)p.N * p.K * 2 >= (1ll << 32)) { set_error("gemm_nt: weight operand exceeds 4 GiB"); return TAD_EINVAL; }
  // The kernel addresses A through a buffer descriptor with 32-bit byte offsets (< 4 GiB), and C -- with the residual / pre-activation
  // operands, which have C's shape -- through descriptors whose out-of-range lanes get offset 0x80000000, so every real offset,
  // including the rows of the last, partly filled tile, must stay below 2^31: (M + 256) * N * element size < 2 GiB with the element
  // size of the widest operand the epilogue touches (4 for an f32 output or an f32 residual, else 2).  Rows are independent, so a
  // taller problem runs as row ranges that fit (ViT-B fc1, N = 3072 bf16: 222 clips of 1568 tokens per range; the f32 cap used to
  // apply to bf16 outputs too and refused B > 111).
  {
    const int64_t max_rows = nt_max_rows(p.N, p.K, (p.c_bf16 && !p.residual) ? 2 : 4);
    if (max_rows <= 0) { set_error("gemm_nt: N=%d / K=%d too wide for the 32-bit operand offsets", p.N, p.K); return TAD_EINVAL; }
    if (p.M > max_rows) {
      for (int64_t r0 = 0; r0 < p.M; r0 += max_rows) {
        const int rows = (int)((p.M - r0) < max_rows ? (p.M - r0) : max_rows);
        const int rc = launch_gemm_nt(row_range(p, (int)r0, rows), st, ws, ws_bytes);
        if (rc) return rc;
      }
      return TAD_OK;
    }
  }
  const int forced = nt_variant;
  p.debug = gemm_debug;
  p.stamps = nt_stamps;
  if (forced) return launch_gemm_nt_one(p, forced, st);
  if (p.M < 2048 || p.N < 128) {
    // small problems (batch-1 inference: 1568 or 784 rows): 128 x 128 tiles, or 128 x 64 when those would leave more than half of the
    // CUs without a workgroup (ViT-B proj / fc2 at 1568 rows: 78 tiles of 128 x 128)
    const int64_t t128 = (int64_t)((p.M + 127) / 128) * ((p.N + 127) / 128);
    const int64_t t64 = (int64_t)((p.M + 127) / 128) * ((p.N + 63) / 64);
    if (t128 * 2 > cu_count() || p.N < 64) return launch_gemm_nt_one(p, 2, st);
    return launch_gemm_nt_one(p, (t64 * 4 <= 3 * cu_count() && p.M >= 64) ? 5 : 4, st);  // 64 x 64 while even 128 x 64 fills < 3/4 of the CUs
  }
  // Short reductions (ViT-S: K = 384; the MAE decoder: K = 512): the epilogue is as long as the K loop, and tiles that put TWO workgroups on a CU
  // let one's epilogue run beside the other's K loop: 192 x 128 as four waves of 96 x 64 (variant 9: 80 KiB of LDS, <= 210 registers) or
  // 128 x 128 (variant 2).  Measured (tools/exp_gemm_knobs.py --D 384 / 512 --configs "variant=0;variant=9;variant=2"), us, planned 256 x 256 /
  // variant 9 / variant 2 -- K = 512: fc1 + GELU 171 / 152 / 161, dX(fc2) GELU' 165 / 151 / 159, the bias-only and residual shapes 1-7 % slower on
  // either; K = 384: qkv 60.0 / 58.5 / 62, fc1 + GELU 102 / 98.6 / 100, dX(fc2) 99 / 97 / 100.5, dX(proj) 28.5 / 25.0 / 24.8, proj + residual
  // 41.0 / 38 / 36 (N = 384 is 1.5 tiles of 256 columns).  From K = 768 the 256 x 256 tile wins everywhere (fc1 274 / 277 / 290)
  if (nt_short_k && p.K <= 512 && !(p.rowscale && p.rows_per_scale < 256)) {
    const bool act = p.epi == EPI_GELU || p.epi == EPI_DGELU;
    if (p.epi == EPI_RESIDUAL && p.K < 512) return launch_gemm_nt_one(p, 2, st);
    if (act || (p.epi == EPI_PLAIN && p.K < 512)) return launch_gemm_nt_one(p, 9, st);
  }
  const bool v1_ok = !(p.epi == EPI_RESIDUAL && (p.c_bf16 || p.res_mod > 0));  // (those instantiations do not exist)
  // Plans: (a) 256 x 128 tiles, (b) 256 x 256 tiles, (c) 256 x 256 tiles for as many row panels as fill whole rounds of one
  // workgroup per CU, the remaining rows as a second launch with whatever suits that smaller problem.  (c) is what lets the
  // N = 768 Linears of ViT-B use the (27 % faster per flop) 256 x 256 tile: 196 x 3 tiles are 2.3 rounds of 256 workgroups.
  const double cost_a = nt_cost(3, p.epi, p.c_bf16, p.M, p.N, p.K);
  const double cost_b = v1_ok ? nt_cost(1, p.epi, p.c_bf16, p.M, p.N, p.K) : 1e300;
  double cost_c = 1e300;
  int main_rows = 0, tail_splits = 0;
  if (v1_ok && nt_split) {
    main_rows = nt_main_rows(p.M, p.N, nullptr);
    if (main_rows > 0) {
      const int tail = p.M - main_rows;
      double tail_cost = tail < 2048 ? nt_cost(2, p.epi, p.c_bf16, tail, p.N, p.K)
                                     : nt_cost(nt_tail_variant(row_range(p, main_rows, tail)), p.epi, p.c_bf16, tail, p.N, p.K);
      // (d) the tail's tiles split along K over all CUs (SPLITK kernels): 78 tiles of the N = 768 Linears of ViT-B run as 3 shares
      // each on 234 CUs instead of one K loop on 156
      if (ws) {
        double sk_cost = 1e300;
        const int s = nt_splitk_plan(row_range(p, main_rows, tail), ws_bytes, &sk_cost);
        if (s && (sk_cost < tail_cost || nt_splitk == 2)) { tail_splits = s; tail_cost = sk_cost; }
      }
      cost_c = nt_cost(1, p.epi, p.c_bf16, main_rows, p.N, p.K) + tail_cost;
    }
  }
  if (nt_split == 2 && main_rows > 0) cost_c = 0.0;  // forced (experiments)
  if (cost_c < cost_a && cost_c < cost_b) {
    const GemmNT t = row_range(p, main_rows, p.M - main_rows);
    if (tail_splits && nt_sk_defer) {  // partial tiles of the tail | whole rounds | combine + epilogue of the tail
      int rc = launch_gemm_nt_splitk(t, tail_splits, ws, st, 1);
      if (rc) return rc;
      rc = launch_gemm_nt_one(row_range(p, 0, main_rows), nt_main_variant(p), st);
      if (rc) return rc;
      return launch_gemm_nt_splitk(t, tail_splits, ws, st, 2);
    }
    int rc = launch_gemm_nt_one(row_range(p, 0, main_rows), nt_main_variant(p), st);
    if (rc) return rc;
    if (tail_splits) return launch_gemm_nt_splitk(t, tail_splits, ws, st);
    if (t.M < 2048) return launch_gemm_nt_one(t, 2, st);
    return launch_gemm_nt_one(t, nt_tail_variant(t), st);
  }
  return launch_gemm_nt_one(p, cost_b < cost_a ? nt_main_variant(p) : 3, st);
}

// TN: 1 = 256x256 (2x4) 2 stages; 3 = 256x128 (4x2) 3 stages.  Splits over the reduction dim target ~1 workgroup per CU.
// TAD_GEMM_TN_VARIANT forces one; by default the 128-wide tile serves shapes whose K the 256-wide one would pad by a third or more
// (K = 384 = 1.5 tiles: ViT-S -- the weight gradients of its qkv / proj / fc1 Linears computed 2 x 256 columns for 384)
static int tn_variant(int K = 0) {
  if (knobs::tn_variant) return knobs::tn_variant;
  const int pad256 = (K + 255) / 256 * 256, pad128 = (K + 127) / 128 * 128;
  return (K > 0 && pad256 * 3 >= pad128 * 4) ? 3 : 1;
}
static int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    return v;
  }();
  return n;
}
// One workgroup per CU is resident (128 KiB of LDS), so the grid runs in rounds of cu_count() workgroups and a grid of
// cu_count() + 1 costs two full rounds.  Pick the split count that minimises rounds x (reduction tiles per split + epilogue)
// plus the slab-reduce pass, all in units of one reduction tile (~2 us on MI355X).
static int tn_plan(int64_t Mr, int N, int K, int* splits, int* rows_per_split) {
  const int bn = tn_variant(K) != 3 ? 256 : 128;
  const int tiles = ((N + 255) / 256) * ((K + bn - 1) / bn);
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
    const int64_t rounds = ((int64_t)tiles * s + cus - 1) / cus;
    const double cost = (double)rounds * ((double)per + epi_units) + (s > 1 ? s * reduce_units : 0.0);
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  const int64_t per = (ktiles + best - 1) / best;
  *splits = best;
  *rows_per_split = (int)(per * BK);
  return tiles;
}

size_t gemm_tn_workspace_bytes(int64_t Mr, int N, int K) {
  int s, r;
  tn_plan(Mr, N, K, &s, &r);
  const int bn = tn_variant(K) != 3 ? 256 : 128;
  return (size_t)s * ((size_t)N * (size_t)K + (size_t)((K + bn - 1) / bn) * (size_t)N) * sizeof(float);
}

// bias_out2 != null: the column sums of the first third of the columns go to bias_out, those of the last third to bias_out2 and the
// middle third is dropped (the qkv Linear: q_bias / no k bias / v_bias, modeling_finetune.py:69-76, 89-92)
int launch_gemm_tn(const uint16_t* P, const uint16_t* Q, float* out, float* bias_out, float* bias_out2, int accumulate, void* ws,
                   size_t ws_bytes, int64_t Mr, int N, int K, hipStream_t st) {
  if (const int rc = sk_check_pending_error()) return rc;  // (a failed in-launch split-K combine is reported by the NEXT tad_linear_* call, whichever it is)
  if (!(Mr > 0 && N > 0 && K > 0)) { set_error("gemm_tn: empty problem"); return TAD_EINVAL; }
  if (N % 8 || K % 8) { set_error("gemm_tn: N=%d and K=%d must be multiples of 8", N, K); return TAD_EINVAL; }
  if (Mr * (int64_t)N * 2 >= (1ll << 32) || Mr * (int64_t)K * 2 >= (1ll << 32)) { set_error("gemm_tn: operand exceeds 4 GiB"); return TAD_EINVAL; }
  GemmTN p{};
  p.P = P; p.Q = Q; p.slab = (float*)ws; p.Mr = (int)Mr; p.N = N; p.K = K;
  p.debug = gemm_debug;
  int splits;
  const int tiles = tn_plan(Mr, N, K, &splits, &p.rows_per_split);
  const int tiles_k = (K + (tn_variant(K) != 3 ? 256 : 128) - 1) / (tn_variant(K) != 3 ? 256 : 128);
  if (ws_bytes < (size_t)splits * ((size_t)N * K + (size_t)tiles_k * N) * sizeof(float)) { set_error("gemm_tn: workspace too small"); return TAD_ENOSPACE; }
  p.bias_slab = bias_out ? p.slab + (size_t)splits * N * K : nullptr;
  // 256 x 256 tiles: the four-wave kernel (gemm_w4.hip; bit-identical results) unless switched off (tad_linear_tuning("tn_w4", 0)); its loop
  // is written for at least two reduction tiles per workgroup
  if (tn_variant(K) == 1 && knobs::tn_w4 && !knobs::tn_pdeep && p.rows_per_split >= 2 * BK && !p.debug) {
    const int rc = launch_gemm_tn_w4(p, tiles * splits, st);
    if (rc) return rc;
  } else if (tn_variant(K) == 1 && knobs::tn_pdeep)
    hipLaunchKernelGGL((gemm_tn_kernel<256, 256, 2, 4, 2, true>), dim3(tiles * splits), dim3(512), 0, st, p);
  else if (tn_variant(K) == 1)
    hipLaunchKernelGGL((gemm_tn_kernel<256, 256, 2, 4, 2>), dim3(tiles * splits), dim3(512), 0, st, p);
  else
    hipLaunchKernelGGL((gemm_tn_kernel<256, 128, 4, 2, 3>), dim3(tiles * splits), dim3(512), 0, st, p);
  int rc = check_launch("gemm_tn");
  if (rc) return rc;
  if (!bias_out) return launch_reduce_partials(p.slab, out, splits, (int64_t)N * K, accumulate, st);
  // slab reduction and bias column sums in one launch (N * K % 4 == 0 and N % 4 == 0 hold: N, K are multiples of 8)
  if (bias_out2) return launch_reduce_dw(p.slab, out, splits, (int64_t)N * K, accumulate, p.bias_slab, splits * tiles_k, N, bias_out, bias_out2, N / 3, 2 * (N / 3), st);
  return launch_reduce_dw(p.slab, out, splits, (int64_t)N * K, accumulate, p.bias_slab, splits * tiles_k, N, bias_out, nullptr, N, 0, st);
}

// Two weight gradients over the same rows with the same K as ONE launch of the four-wave kernel (GemmTN::N1): out1 [N1, K] = P1^T Q1 with its
// bias column sums (bias_out1, or split into bias_out1 / bias_out1b as for the qkv Linear), out2 [N2, K] = P2^T Q2.  A small problem pays for
// filling the chip with many splits -- the 768 x 768 proj gradient of ViT-B runs 9 tiles x 28 splits: 28 slabs to write and sum, an epilogue per
// 28 reduction tiles -- where the pair (36 tiles x 7 splits: the shape of the fc1 gradient) pays once: qkv + proj 160.8 + 71.7 us apart, ~197 as a
// pair.  Falls back to two launches when the pair does not fit the kernel (K not on 256-wide tiles, N1 not a multiple of 256, four-wave kernel off).
// The summation order over the rows differs from the single launches' (another split count), as between any two batch sizes.
int launch_gemm_tn_pair(const uint16_t* P1, const uint16_t* Q1, float* out1, float* bias_out1, float* bias_out1b, int N1, const uint16_t* P2,
                        const uint16_t* Q2, float* out2, int N2, int accumulate, void* ws, size_t ws_bytes, int64_t Mr, int K, hipStream_t st) {
  if (const int rc = sk_check_pending_error()) return rc;
  if (!(Mr > 0 && N1 > 0 && N2 > 0 && K > 0)) { set_error("gemm_tn_pair: empty problem"); return TAD_EINVAL; }
  if (N1 % 8 || N2 % 8 || K % 8) { set_error("gemm_tn_pair: N1=%d, N2=%d and K=%d must be multiples of 8", N1, N2, K); return TAD_EINVAL; }
  const int N = N1 + N2;
  int splits = 0, rows_per_split = 0;
  const int tiles = tn_plan(Mr, N, K, &splits, &rows_per_split);
  const int tiles_k = (K + 255) / 256;
  const bool fits = tn_pair && tn_variant(K) == 1 && knobs::tn_w4 && !knobs::tn_pdeep && !gemm_debug && N1 % 256 == 0 && rows_per_split >= 2 * BK &&
                    Mr * (int64_t)N * 2 < (1ll << 32) && Mr * (int64_t)K * 2 < (1ll << 32) &&
                    ws_bytes >= (size_t)splits * ((size_t)N * K + (size_t)tiles_k * N) * sizeof(float);
  if (!fits) {
    const int rc = launch_gemm_tn(P1, Q1, out1, bias_out1, bias_out1b, accumulate, ws, ws_bytes, Mr, N1, K, st);
    if (rc) return rc;
    return launch_gemm_tn(P2, Q2, out2, nullptr, nullptr, accumulate, ws, ws_bytes, Mr, N2, K, st);
  }
  GemmTN p{};
  p.P = P1; p.Q = Q1; p.P2 = P2; p.Q2 = Q2; p.N1 = N1;
  p.slab = (float*)ws; p.Mr = (int)Mr; p.N = N; p.K = K; p.rows_per_split = rows_per_split;
  p.bias_slab = bias_out1 ? p.slab + (size_t)splits * N * K : nullptr;
  int rc = launch_gemm_tn_w4(p, tiles * splits, st);
  if (rc) return rc;
  // slabs [splits][N][K]: rows [0, N1) -> out1, rows [N1, N) -> out2, both in one launch (with the bias column sums of the first problem)
  const int64_t n1 = (int64_t)N1 * K, n = (int64_t)N * K;
  if (!bias_out1) return launch_reduce_dw_pair(p.slab, out1, out2, n1, splits, n, accumulate, nullptr, 0, 0, nullptr, nullptr, 0, 0, st);
  if (bias_out1b) return launch_reduce_dw_pair(p.slab, out1, out2, n1, splits, n, accumulate, p.bias_slab, splits * tiles_k, N, bias_out1, bias_out1b, N1 / 3, 2 * (N1 / 3), st);
  return launch_reduce_dw_pair(p.slab, out1, out2, n1, splits, n, accumulate, p.bias_slab, splits * tiles_k, N, bias_out1, nullptr, N1, 0, st);
}

TAD_NAMESPACE_END

using namespace tad;

extern "C" {

int tad_linear_fwd(const uint16_t* x, const uint16_t* w, const float* bias, void* y, int y_dtype, int epilogue, uint16_t* preact,
                   const float* residual, const float* gamma, const float* rowscale, int rows_per_scale, void* ws, size_t ws_bytes,
                   int64_t M, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(x && w && y, "linear_fwd: null pointer");
  TAD_REQUIRE(y_dtype == TAD_F32 || y_dtype == TAD_OP16, "linear_fwd: bad y_dtype %d", y_dtype);
  TAD_REQUIRE(epilogue >= TAD_EPI_BIAS && epilogue <= TAD_EPI_BIAS_RESIDUAL, "linear_fwd: bad epilogue %d", epilogue);
  TAD_REQUIRE(!rowscale || rows_per_scale > 0, "linear_fwd: rows_per_scale must be positive");
  TAD_REQUIRE(M > 0 && M < (1ll << 31), "linear_fwd: bad M");
  GemmNT p{};
  p.A = x; p.B = w; p.C = y; p.bias = bias; p.c_bf16 = (y_dtype == TAD_OP16);
  p.M = (int)M; p.N = N; p.K = K;
  p.rows_per_scale = rows_per_scale > 0 ? rows_per_scale : 1;
  if (epilogue == TAD_EPI_BIAS_GELU) { p.epi = EPI_GELU; p.preact = preact; }
  else if (epilogue == TAD_EPI_BIAS_RESIDUAL) { p.epi = EPI_RESIDUAL; p.residual = residual; p.gamma = gamma; p.rowscale = rowscale; }
  else p.epi = EPI_PLAIN;
  return launch_gemm_nt(p, (hipStream_t)stream, ws, ws ? ws_bytes : 0);
}

#ifndef TAD_OPND_F16
size_t tad_linear_workspace_bytes(int64_t M, int N, int K) {
  // What launch_gemm_nt's split plan hands to nt_splitk_plan for this shape (same helpers: nt_max_rows, nt_main_rows, nt_splitk_shares; the
  // epilogue kind is not known here: assumed eligible, and both element sizes of the row-range rule are covered), or 0 when no tail of this
  // shape splits along K -- every Linear of ViT-B under the default knobs (64 MB used to stay resident per stream for nothing)
  if (M < 4096 || N < 128 || K <= 0 || K % BK || !nt_split || !nt_splitk) return 0;
  size_t need = 0;
  for (int64_t esz = 2; esz <= 4; esz += 2) {
    const int64_t max_rows = nt_max_rows(N, K, esz);
    if (max_rows <= 0) continue;
    for (int64_t r0 = 0; r0 < M; r0 += max_rows) {  // the row ranges launch_gemm_nt cuts a taller problem into (two distinct sizes at most)
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
#endif

int tad_linear_fwd_qkv(const uint16_t* x, const uint16_t* w, const float* q_bias, const float* v_bias, void* y, int y_dtype, float q_prescale,
                       int64_t M, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(x && w && y, "linear_fwd_qkv: null pointer");
  TAD_REQUIRE((q_bias == nullptr) == (v_bias == nullptr), "linear_fwd_qkv: q_bias and v_bias come together");
  TAD_REQUIRE(y_dtype == TAD_F32 || y_dtype == TAD_OP16, "linear_fwd_qkv: bad y_dtype %d", y_dtype);
  TAD_REQUIRE(N > 0 && N % 12 == 0, "linear_fwd_qkv: N=%d must be 3 x a multiple of 4", N);
  TAD_REQUIRE(M > 0 && M < (1ll << 31), "linear_fwd_qkv: bad M");
  TAD_REQUIRE(q_prescale > 0.f, "linear_fwd_qkv: q_prescale must be positive (1 = plain)");
  TAD_REQUIRE(q_prescale == 1.f || N % 24 == 0, "linear_fwd_qkv: q_prescale needs N/3 = %d to be a multiple of 8", N / 3);
  GemmNT p{};
  p.A = x; p.B = w; p.C = y; p.c_bf16 = (y_dtype == TAD_OP16);
  p.bias = q_bias; p.bias2 = v_bias; p.bias_seg = q_bias ? N / 3 : 0;
  if (q_prescale != 1.f) { p.colscale = q_prescale; p.colscale_cols = N / 3; }
  p.M = (int)M; p.N = N; p.K = K;
  p.rows_per_scale = 1;
  p.epi = EPI_PLAIN;
  return launch_gemm_nt(p, (hipStream_t)stream);
}

int tad_linear_bwd_weight_qkv(const uint16_t* dy, const uint16_t* x, float* dW, float* dq_bias, float* dv_bias, int accumulate, void* ws,
                              size_t ws_bytes, int64_t M, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(dy && x && dW && ws && dq_bias && dv_bias, "linear_bwd_weight_qkv: null pointer");
  TAD_REQUIRE(N > 0 && N % 12 == 0, "linear_bwd_weight_qkv: N=%d must be 3 x a multiple of 4", N);
  return launch_gemm_tn(dy, x, dW, dq_bias, dv_bias, accumulate, ws, ws_bytes, M, N, K, (hipStream_t)stream);
}

int tad_linear_bwd_weight_pair(const uint16_t* dy1, const uint16_t* x1, float* dW1, float* db1, float* db1b, int N1, const uint16_t* dy2,
                               const uint16_t* x2, float* dW2, int N2, int accumulate, void* ws, size_t ws_bytes, int64_t M, int K, tad_stream_t stream) {
  TAD_REQUIRE(dy1 && x1 && dW1 && dy2 && x2 && dW2 && ws, "linear_bwd_weight_pair: null pointer");
  TAD_REQUIRE(!db1b || db1, "linear_bwd_weight_pair: db1b (the v_bias third) comes with db1 (the q_bias third)");
  TAD_REQUIRE(!db1b || (N1 > 0 && N1 % 12 == 0), "linear_bwd_weight_pair: N1=%d must be 3 x a multiple of 4 for the split bias sums", N1);
  // the slab reduction reads and writes float4s through every output (dW2 is usually a view into the flat gradient buffer)
  TAD_REQUIRE(((uintptr_t)dW1 | (uintptr_t)dW2 | (uintptr_t)db1 | (uintptr_t)db1b) % 16 == 0, "linear_bwd_weight_pair: dW1, dW2, db1 and db1b must be 16-byte aligned");
  return launch_gemm_tn_pair(dy1, x1, dW1, db1, db1b, N1, dy2, x2, dW2, N2, accumulate, ws, ws_bytes, M, K, (hipStream_t)stream);
}

#ifndef TAD_OPND_F16  // process-wide knobs / counters: one copy for the library (bf16 pass)
int tad_linear_tuning(const char* key, int value) {
  TAD_REQUIRE(key, "linear_tuning: null key");
  const std::string k(key);
  if (k == "splitk_tail") { TAD_REQUIRE(value >= 0 && value <= 2, "linear_tuning: splitk_tail=%d not in {0, 1, 2}", value); nt_splitk = value; return TAD_OK; }
  if (k == "persistent") nt_persist = value != 0;
  else if (k == "direct_epilogue") { TAD_REQUIRE(value >= 0 && value <= 2, "linear_tuning: direct_epilogue=%d not in 0..2", value); nt_direct = value; }
  else if (k == "debug") gemm_debug = value;  // ablation bits (timing experiments; ignored by production builds)
  else if (k == "group_m") { TAD_REQUIRE(value >= 0 && value <= 1024, "linear_tuning: group_m=%d out of range", value); nt_group_m_knob = value; }
  else if (k == "variant") { TAD_REQUIRE(value >= 0 && value <= 9 && value != 6, "linear_tuning: variant=%d not one of 0..5, 7, 8, 9", value); nt_variant = value; }
  else if (k == "splitk_defer") { TAD_REQUIRE(value == 0 || value == 1, "linear_tuning: splitk_defer=%d not in {0, 1}", value); nt_sk_defer = value; }
  else if (k == "tn_pair") { TAD_REQUIRE(value == 0 || value == 1, "linear_tuning: tn_pair=%d not in {0, 1}", value); tn_pair = value; }
  else if (k == "short_k") { TAD_REQUIRE(value == 0 || value == 1, "linear_tuning: short_k=%d not in {0, 1}", value); nt_short_k = value; }
  else if (k == "tail_192") { TAD_REQUIRE(value == 0 || value == 1, "linear_tuning: tail_192=%d not in {0, 1}", value); nt_tail_192 = value; }
  else if (k == "w4_epilogues") { TAD_REQUIRE(value >= 0 && value < 16, "linear_tuning: w4_epilogues=%d not a mask of bits 1..3", value); nt_w4_epilogues = value; }
  else if (k == "w4_plain") { TAD_REQUIRE(value >= 0, "linear_tuning: w4_plain=%d must be >= 0", value); nt_w4_plain = value; }
  else if (k == "tn_w4") { TAD_REQUIRE(value == 0 || value == 1, "linear_tuning: tn_w4=%d not in {0, 1}", value); tn_w4 = value; }
  else if (k == "tn_pdeep") { TAD_REQUIRE(value == 0 || value == 1, "linear_tuning: tn_pdeep=%d not in {0, 1}", value); tn_pdeep = value; }
  else if (k == "split_tail") { TAD_REQUIRE(value >= 0 && value <= 2, "linear_tuning: split_tail=%d not in 0..2", value); nt_split = value; }
  else { set_error("linear_tuning: unknown key '%s'", key); return TAD_EINVAL; }
  return TAD_OK;
}

int tad_linear_tuning_get(const char* key, int* value) {
  TAD_REQUIRE(key && value, "linear_tuning_get: null pointer");
  const std::string k(key);
  const struct { const char* name; const int* v; } table[] = {
      {"splitk_tail", &nt_splitk}, {"persistent", &nt_persist}, {"direct_epilogue", &nt_direct}, {"debug", &gemm_debug}, {"group_m", &nt_group_m_knob},
      {"variant", &nt_variant}, {"splitk_defer", &nt_sk_defer}, {"tn_pair", &tn_pair}, {"short_k", &nt_short_k}, {"tail_192", &nt_tail_192},
      {"w4_epilogues", &nt_w4_epilogues}, {"w4_plain", &nt_w4_plain}, {"tn_w4", &tn_w4}, {"tn_pdeep", &tn_pdeep}, {"split_tail", &nt_split}};
  for (const auto& e : table)
    if (k == e.name) { *value = *e.v; return TAD_OK; }
  set_error("linear_tuning_get: unknown key '%s'", key);
  return TAD_EINVAL;
}

long long tad_linear_kernel_launches(void) { return nt_launches; }

int tad_linear_debug_stamps(void* buf) {
#ifndef TAD_GEMM_ABLATION
  if (buf) { set_error("linear_debug_stamps: timeline stamps need an ablation build (TAD_BUILD_ABLATION=1 python -m simple_tad_amd.build --force)"); return TAD_EINVAL; }
#endif
  nt_stamps = (unsigned long long*)buf;
  return TAD_OK;
}
#endif

int tad_linear_bwd_input(const uint16_t* dy, const uint16_t* wT, void* dx, int dx_dtype, const uint16_t* gelu_preact, void* ws, size_t ws_bytes,
                         int64_t M, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(dy && wT && dx, "linear_bwd_input: null pointer");
  TAD_REQUIRE(dx_dtype == TAD_F32 || dx_dtype == TAD_OP16, "linear_bwd_input: bad dx_dtype %d", dx_dtype);
  TAD_REQUIRE(M > 0 && M < (1ll << 31), "linear_bwd_input: bad M");
  GemmNT p{};
  p.A = dy; p.B = wT; p.C = dx; p.c_bf16 = (dx_dtype == TAD_OP16);
  p.M = (int)M; p.N = K; p.K = N;  // dx[M,K] = dy[M,N] * (wT[K,N])^T
  p.rows_per_scale = 1;
  p.epi = gelu_preact ? EPI_DGELU : EPI_PLAIN;
  p.dgelu_h = gelu_preact;
  return launch_gemm_nt(p, (hipStream_t)stream, ws, ws ? ws_bytes : 0);
}

#ifndef TAD_OPND_F16
size_t tad_linear_bwd_weight_workspace_bytes(int64_t M, int N, int K) {
  return gemm_tn_workspace_bytes(M, N, K);
}
#endif

int tad_linear_bwd_weight(const uint16_t* dy, const uint16_t* x, float* dW, float* db, int accumulate, void* ws, size_t ws_bytes,
                          int64_t M, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(dy && x && dW && ws, "linear_bwd_weight: null pointer");
  return launch_gemm_tn(dy, x, dW, db, nullptr, accumulate, ws, ws_bytes, M, N, K, (hipStream_t)stream);
}

// ---- PatchEmbed = im2col + NT GEMM with bias and broadcast pos_embed in the epilogue
int tad_patch_embed_fwd(const float* x, const uint16_t* w_bf16, const float* bias, const float* pos, float* out, uint16_t* cols, int B,
                        int C, int T, int H, int W, int tubelet, int patch, int D, tad_stream_t stream) {
  TAD_REQUIRE(x && w_bf16 && out && cols, "patch_embed_fwd: null pointer");
  int rc = tad_im2col_tubelets(x, cols, B, C, T, H, W, tubelet, patch, stream);
  if (rc) return rc;
  const int ntok = (T / tubelet) * (H / patch) * (W / patch);
  GemmNT p{};
  p.A = cols; p.B = w_bf16; p.C = out; p.bias = bias; p.c_bf16 = 0;
  p.M = B * ntok; p.N = D; p.K = tad_patch_embed_ldk(C, tubelet, patch);  // cols / w_bf16 row stride (= K unless the patch is /14-like)
  p.rows_per_scale = 1;
  p.epi = EPI_RESIDUAL;
  p.residual = pos;
  p.res_mod = ntok;
  return launch_gemm_nt(p, (hipStream_t)stream);
}

int tad_patch_embed_gemm(const uint16_t* cols, const uint16_t* w_bf16, const float* bias, const float* pos, float* out, int64_t M, int ntok,
                         int D, int K, tad_stream_t stream) {
  TAD_REQUIRE(cols && w_bf16 && out, "patch_embed_gemm: null pointer");
  TAD_REQUIRE(M > 0 && M < (1ll << 31) && ntok > 0 && M % ntok == 0, "patch_embed_gemm: M=%lld must be a positive multiple of ntok=%d",
              (long long)M, ntok);
  GemmNT p{};
  p.A = cols; p.B = w_bf16; p.C = out; p.bias = bias; p.c_bf16 = 0;
  p.M = (int)M; p.N = D; p.K = K;
  p.rows_per_scale = 1;
  p.epi = EPI_RESIDUAL;
  p.residual = pos;
  p.res_mod = ntok;
  return launch_gemm_nt(p, (hipStream_t)stream);
}

#ifndef TAD_OPND_F16
size_t tad_patch_embed_bwd_workspace_bytes(int64_t M, int D, int K) { return tad_linear_bwd_weight_workspace_bytes(M, D, K); }
#endif

int tad_patch_embed_bwd(const uint16_t* dy_bf16, const uint16_t* cols, float* dW, float* db, void* ws, size_t ws_bytes, int64_t M, int D,
                        int K, tad_stream_t stream) {
  return tad_linear_bwd_weight(dy_bf16, cols, dW, db, 0, ws, ws_bytes, M, D, K, stream);
}

}  // extern "C"
