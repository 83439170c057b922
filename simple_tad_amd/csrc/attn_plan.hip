// Launch selector of the 16-bit attention kernels and the process-wide state that goes with it (see attn_plan.h).  Host code only: compiled
// once, for both operand formats.  The executors of the records are tad_attn_fwd (attn_fwd.hip) and tad_attn_bwd (attn_bwd.hip).
#include <string.h>
#include "common.h"
#include "attn_plan.h"
#include "knob.h"

namespace tad {

// ---- the knobs: ONE table for the initial values (environment), tad_attn_tuning and tad_attn_tuning_get
namespace knobs {
int attn_dma_mode, attn_fwd_q64, attn_drop_skip;
unsigned long long* attn_stamps = nullptr;
}  // namespace knobs
using namespace knobs;

namespace {
#ifdef TAD_GEMM_ABLATION
constexpr int DMA_MODE_MAX = 3;  // (1 is refused: tad_attn_tuning)
#else
constexpr int DMA_MODE_MAX = 0;  // 2 / 3 are timing-only ablations
#endif
const Knob KNOBS[] = {
    {"dma_mode", &attn_dma_mode, 0, DMA_MODE_MAX, "TAD_ATTN_DMA_MODE", 0, 0},
    {"fwd_q64", &attn_fwd_q64, 0, 1, "TAD_ATTN_FWD_Q64", 0, 0},
    {"drop_skip", &attn_drop_skip, 0, 1, "TAD_DROP_SKIP", 1, KNOB_BOOL},
};
const bool knobs_initialised = knobs_from_env(KNOBS);

constexpr int Q_BLOCK = 128;  // query rows (dQ, forward) or keys (dK/dV) per workgroup

// DMA_MODE of a launch: the ablation the knob asks for where this build has it (the forward has no mode 3), else production
int dma_mode_of(int highest) {
#ifdef TAD_GEMM_ABLATION
  if (attn_dma_mode == 2 || (attn_dma_mode == 3 && highest == 3)) return attn_dma_mode;
#endif
  (void)highest;
  return 0;
}
// Clips dropped by stochastic depth fill instead of compute: the production contract of the training step only (any other one computes them)
bool fills_dropped_clips(const AttnCall& c) {
  return c.clip_scale && attn_drop_skip && c.d == 64 && c.q_prescaled && c.dropout_p == 0.f && attn_dma_mode == 0;
}
}  // namespace

int attn_plan_fwd(const AttnCall& c, AttnLaunch* l) {
  const int B = c.B, N = c.N, H = c.H;
  TAD_REQUIRE(!c.out_lo || c.out_dtype == c.op16_dtype, "attn_fwd: out_lo (the rounding residual) goes with a 16-bit output");
  TAD_REQUIRE(c.d == 64 || c.d == 80, "attn_fwd: head_dim must be 64 or 80 (got %d)", c.d);
  TAD_REQUIRE(B > 0 && N > 0 && H > 0 && H <= 65535 && B <= 65535, "attn_fwd: bad shape B=%d N=%d H=%d", B, N, H);
  TAD_REQUIRE(c.out_dtype == TAD_F32 || c.out_dtype == c.op16_dtype, "attn_fwd: bad out_dtype %d", c.out_dtype);
  TAD_REQUIRE(c.scale > 0.f, "attn_fwd: scale must be positive");
  Drop drop;
  TAD_REQUIRE(make_drop(c.dropout_p, 0, &drop), "attn_fwd: dropout_p=%g outside [0, 1)", (double)c.dropout_p);
  TAD_REQUIRE(c.dropout_p == 0.f || (int64_t)B * H * N < (1ll << 32), "attn_fwd: B*H*N too large for the dropout mask's row index");
  // the kernel addresses qkv through ONE buffer descriptor with 32-bit byte offsets (K/V staging by LDS-DMA)
  TAD_REQUIRE((int64_t)B * N * 3 * H * c.d * 2 < (1ll << 32), "attn_fwd: qkv of %lld bytes exceeds the 4 GiB buffer descriptor (B=%d N=%d H=%d)",
              (long long)B * N * 3 * H * c.d * 2, B, N, H);
  TAD_REQUIRE((int64_t)((N + Q_BLOCK - 1) / Q_BLOCK) * H * B < (1ll << 31), "attn_fwd: grid too large");
  const int grid = ((N + Q_BLOCK - 1) / Q_BLOCK) * H * B;
  const int out16 = c.out_dtype == c.op16_dtype;
  // (experiment) sixty-four query rows per wave: same grid, 128 threads -- only the production contract of the training step, whose dropped
  // clips it computes like the others
  if (attn_fwd_q64 && c.d == 64 && c.q_prescaled && c.dropout_p == 0.f && out16) *l = AttnLaunch{ATTN_FWD_Q64, 64, 1, 1, 0, 0, 0, c.out_lo != 0, grid, 128};
  else if (fills_dropped_clips(c) && out16) *l = AttnLaunch{ATTN_FWD, 64, 1, 1, 0, 0, 1, 0, grid, 256};
  else *l = AttnLaunch{ATTN_FWD, c.d, out16, c.q_prescaled != 0, c.dropout_p > 0.f, dma_mode_of(2), 0, 0, grid, 256};
  return TAD_OK;
}

int attn_plan_bwd(const AttnCall& c, AttnLaunch (&l)[2]) {
  const int B = c.B, N = c.N, H = c.H;
  TAD_REQUIRE(c.d == 64 || c.d == 80, "attn_bwd: head_dim must be 64 or 80 (got %d)", c.d);
  TAD_REQUIRE(B > 0 && N > 0 && H > 0 && H <= 65535 && B <= 65535, "attn_bwd: bad shape");
  TAD_REQUIRE(c.scale > 0.f, "attn_bwd: scale must be positive");
  Drop drop;
  TAD_REQUIRE(make_drop(c.dropout_p, 0, &drop), "attn_bwd: dropout_p=%g outside [0, 1)", (double)c.dropout_p);
  TAD_REQUIRE((int64_t)B * H * N * 8 < (1ll << 31), "attn_bwd: B*H*N too large for the row-constant descriptor");
  TAD_REQUIRE((int64_t)B * N * 3 * H * c.d * 2 < (1ll << 32), "attn_bwd: qkv exceeds the 4 GiB buffer descriptor (B=%d N=%d H=%d)", B, N, H);
  const int grid = ((N + Q_BLOCK - 1) / Q_BLOCK) * H * B;
  if (fills_dropped_clips(c)) l[0] = AttnLaunch{ATTN_BWD_DQ, 64, 1, 1, 0, 0, 1, 0, grid, 256};
  else l[0] = AttnLaunch{ATTN_BWD_DQ, c.d, 1, c.q_prescaled != 0, c.dropout_p > 0.f, dma_mode_of(3), 0, 0, grid, 256};  // (mode 3, dQ kernel: as mode 0)
  l[1] = l[0];
  l[1].kernel = ATTN_BWD_DKV;
  return TAD_OK;
}

}  // namespace tad

using namespace tad;

extern "C" {

int tad_attn_tuning(const char* key, int value) {
  TAD_REQUIRE(!(DMA_MODE_MAX == 3 && key && !strcmp(key, "dma_mode") && value == 1), "attn_tuning: dma_mode=%d not in {0, 2, 3}", value);
  return knob_set(KNOBS, "attn_tuning", key, value);
}

int tad_attn_tuning_get(const char* key, int* value) { return knob_get(KNOBS, "attn_tuning_get", key, value); }

// Diagnostic (ablation builds only, like tad_linear_debug_stamps): while buf (device memory, 32 bytes per workgroup of the dK/dV grid)
// is set, workgroup w records {s_memrealtime, s_memtime} at the start and at the end of its tile loop in buf[4w .. 4w+3].
int tad_attn_debug_stamps(void* buf) {
#ifndef TAD_GEMM_ABLATION
  if (buf) { set_error("attn_debug_stamps: needs an ablation build (TAD_BUILD_ABLATION=1 python -m simple_tad_amd.build --force)"); return TAD_EINVAL; }
#endif
  attn_stamps = (unsigned long long*)buf;
  return TAD_OK;
}

size_t tad_attn_bwd_scratch_bytes(int B, int N, int H) {
  if (B <= 0 || N <= 0 || H <= 0) return 0;
  return (size_t)2 * B * H * N * sizeof(float);
}

int tad_attn_plan(int backward, int B, int N, int H, int d, int out_16bit, int q_prescaled, float dropout_p, int has_clip_scale, int has_out_lo,
                  int32_t* launches, int capacity) {
  TAD_REQUIRE(launches || capacity <= 0, "attn_plan: null buffer");
  const AttnCall c{B, N, H, d, out_16bit ? TAD_BF16 : TAD_F32, TAD_BF16, q_prescaled, 1.f, dropout_p, has_clip_scale, has_out_lo};
  AttnLaunch l[2];
  const int n = backward ? 2 : 1;
  if (const int rc = backward ? attn_plan_bwd(c, l) : attn_plan_fwd(c, l)) return rc;
  if (n > capacity) { set_error("attn_plan: %d launches, room for %d", n, capacity); return TAD_ENOSPACE; }
  memcpy(launches, l, (size_t)n * sizeof(AttnLaunch));
  return n;
}

}  // extern "C"
