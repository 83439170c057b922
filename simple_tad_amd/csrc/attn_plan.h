// Launch selector of the 16-bit attention kernels (csrc/attn_plan.hip): WHICH kernel instantiation a tad_attn_fwd / tad_attn_bwd call runs, as
// data.  Host-only and compiled once -- nothing in a record depends on the operand format -- together with the knobs of the attention kernels.
// attn_fwd.hip / attn_bwd.hip, compiled per format, look the record up in their table of instantiations and launch it; tad_attn_plan
// (include/tad_mi355x.h) returns the records without launching anything.
#pragma once
#include <stdint.h>

namespace tad {

// Knobs of the attention kernels (tad_attn_tuning; initial values from the environment): one copy for the library.  The table that names,
// bounds and initialises them is in attn_plan.hip (KNOBS).
namespace knobs {
extern int attn_dma_mode;   // 2 / 3: timing-only ablations (ablation builds)
extern int attn_fwd_q64;    // 1: the forward with 64 query rows per wave (attn_fwd_q64_kernel; experiment, round 6)
extern int attn_drop_skip;  // 0: clips dropped by stochastic depth are computed like the others (A/B runs)
extern unsigned long long* attn_stamps;  // diagnostic (tad_attn_debug_stamps)
}  // namespace knobs

// A call as the selector sees it: no pointers, only whether the nullable operands are there
struct AttnCall {
  int B, N, H, d;
  int out_dtype, op16_dtype;  // forward: the output type asked for | the TAD_* tag of the calling pass's 16-bit operand format
  int q_prescaled;
  float scale, dropout_p;
  int clip_scale, out_lo;  // operand present
};
enum { ATTN_FWD = 0, ATTN_FWD_Q64 = 1, ATTN_BWD_DQ = 2, ATTN_BWD_DKV = 3 };
// One kernel launch: the kernel family, its template arguments, the geometry.  The launchers execute it and decide nothing again.
struct AttnLaunch {
  int kernel;        // ATTN_*
  int hd;            // HD: 64 | 80
  int out16;         // OUT_BF16 of the forward: the output has the 16-bit operand format (the backward kernels': always, dqkv)
  int qs, drop;      // QS, DROP
  int dma_mode;      // DMA_MODE: 0, or the ablation a build with them runs
  int skip;          // SKIP: the launch gets the clip scale and fills the clips it drops; 0: the kernel gets a null scale
  int has_lo;        // HAS_LO of attn_fwd_q64_kernel (0 for the other families: they test the pointer)
  int grid, block;
};
constexpr int ATTN_LAUNCH_WORDS = 10;  // = TAD_ATTN_PLAN_WORDS: an AttnLaunch is that many ints, in the order of tad_attn_plan's rows
static_assert(sizeof(AttnLaunch) == ATTN_LAUNCH_WORDS * sizeof(int), "tad_attn_plan copies launches out as rows of int32");

// TAD_OK and the launch(es), or the error (set_error) that refuses the call: every shape and limit check of the entry points is here
int attn_plan_fwd(const AttnCall& c, AttnLaunch* l);
int attn_plan_bwd(const AttnCall& c, AttnLaunch (&l)[2]);  // dQ, then dK/dV
inline const char* attn_kernel_name(int kernel) { return kernel == ATTN_FWD ? "attn_fwd" : kernel == ATTN_FWD_Q64 ? "attn_fwd_q64" : kernel == ATTN_BWD_DQ ? "attn_bwd_dq" : "attn_bwd_dkv"; }

}  // namespace tad
