// Launch planner of the Linear GEMMs (csrc/gemm_plan.hip): WHAT a problem runs as, as data.  Host-only and compiled once -- nothing in a plan
// depends on the 16-bit operand format -- so it lives in namespace tad outside the per-format inline namespace, together with the process-wide
// state of the Linears (knobs, counters, the split-K error word).  csrc/gemm.hip, compiled per format, executes the steps; tad_linear_plan /
// tad_linear_bwd_weight_plan (include/tad_mi355x.h) return them without launching anything.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tad {

// EPI_RESMOD = EPI_RESIDUAL with the residual row taken modulo res_mod ("+ pos_embed" of the patch embedding): a variant of its
// own so that the integer division stays out of the Linear kernels
enum { EPI_PLAIN = 0, EPI_GELU = 1, EPI_RESIDUAL = 2, EPI_DGELU = 3, EPI_RESMOD = 4 };
constexpr int BK = 64;  // K-tile depth (bf16 elements) -> 128-byte LDS rows

// Scheduling knobs and counters of the Linear GEMMs (tad_linear_tuning; initial values from the environment): one copy for the whole library.
// The table that names, bounds and initialises the knobs is in gemm_plan.hip (KNOBS).
namespace knobs {
extern int gemm_debug, nt_persist, nt_direct, nt_split, nt_splitk, nt_variant, nt_group_m_knob, tn_variant, tn_pdeep, nt_sk_defer, tn_w4, nt_w4_plain,
    nt_w4_epilogues, nt_tail_192, nt_short_k, tn_pair;
extern unsigned long long* nt_stamps;
extern long long nt_launches;  // gemm_nt kernel launches so far (tad_linear_kernel_launches)
}  // namespace knobs

// ---- gemm_nt
// A Linear problem as the planner sees it: no pointers (GemmNT, with them, is per format)
struct NtDesc {
  int64_t M;
  int N, K;
  int epi;       // EPI_PLAIN / GELU / RESIDUAL / DGELU as the entry point poses it (RESIDUAL + res_mod becomes RESMOD in the steps)
  int out16;     // output in the 16-bit operand format (else f32)
  int residual;  // a residual operand is present
  int res_mod;
  int rowscale;  // a row-scale operand is present
  int rows_per_scale;
  int colscale_cols;
  size_t ws_bytes;  // split-K workspace on offer (0: none)
};
constexpr int NT_SPLITK = 10;  // NtStep::kernel of the split-K launches (the tile configurations are 1 2 3 4 5 7 8 9)
// One kernel launch: everything the executor needs and nothing it has to decide again
struct NtStep {
  int r0, rows;  // the rows of the problem this launch covers
  int kernel;    // tile configuration actually launched (1 2 3 4 5 7 8 9, see launch_nt_step) or NT_SPLITK
  int persist;   // one workgroup per CU walks the tile list (else one per tile)
  int direct;    // epilogue stores straight from the MFMA layout
  int grid, block;
  int group_m;
  int sk_splits, sk_mode;  // NT_SPLITK: shares per tile; 0 combine inside the launch, 1 leave partial tiles, 2 combine what a mode-1 launch left
  int epi;                 // the epilogue instantiation (EPI_RESMOD where the problem's residual is taken modulo res_mod)
};
constexpr int NT_STEP_WORDS = 11;  // = TAD_LINEAR_PLAN_STEP_WORDS: an NtStep is that many ints, in the order of tad_linear_plan's rows
static_assert(sizeof(NtStep) == NT_STEP_WORDS * sizeof(int), "tad_linear_plan copies steps out as rows of int32");
// The plan of ONE row range of a problem.  A problem taller than the 32-bit operand offsets allow runs as consecutive row ranges (nt_max_rows);
// the caller walks them:  for (int64_t r0 = 0; r0 < d.M; r0 = plan.next) { plan = nt_plan(d, r0); ... plan.step[0 .. plan.n) ... }
struct NtPlan {
  int n;
  NtStep step[3];   // at most: partial tiles of the tail | whole rounds | combine of the tail
  int64_t next;     // first row of the next range (= M: done)
  size_t ws_short;  // != 0: a workspace was on offer but is smaller than these many bytes, which the split-K tail of this range needs: it runs unsplit
};
int nt_validate(const NtDesc& d);  // TAD_OK, or the error (set_error) that refuses the problem
NtPlan nt_plan(const NtDesc& d, int64_t r0);
void nt_warn_ws_short(const NtDesc& d, const NtPlan& plan);  // says so on stderr, once per process

// Split-K workspace layout: [arrival counters, one per tile | error word][partial tiles].  The counters are zeroed on the stream in front of a mode-0 launch.
constexpr size_t SK_HEADER_BYTES = 4096;  // counters (<= 1008 tiles)
constexpr size_t SK_TILE_BYTES = 256 * 256 * sizeof(float);
unsigned* sk_error_word(unsigned** dev_ptr);  // the word a mode-0 launch reports a lost share in (pinned host memory); arms sk_check_pending_error
int sk_check_pending_error();                 // TAD_ELAUNCH once after an in-launch combine gave up, whichever format's launch it was

// ---- gemm_tn (weight gradients)
enum { TN_W4 = 0, TN_PDEEP = 1, TN_W8 = 2, TN_W8_128 = 3 };  // four waves 256 x 256 | eight waves, deep P ring | eight waves 256 x 256 | 256 x 128
struct TnPlan {
  int bn;  // tile width along K (256 or 128)
  int tiles, tiles_k;
  int splits, rows_per_split;
  size_t ws_bytes;  // slabs + bias column-sum slabs
  int kernel;
  int grid, block;
  bool fits;  // asked with N1 > 0 (N = N1 + N2 of a pair): the two problems run as ONE launch of the four-wave kernel
};
TnPlan tn_plan(int64_t Mr, int N, int K, int N1 = 0, size_t ws_bytes = 0);

}  // namespace tad
