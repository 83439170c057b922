// Host half of the 16-bit-operand GEMMs, per operand format: the executors of the launch plans and the C ABI of the Linear layers.  WHAT a problem
// runs as is decided in gemm_plan.hip (compiled once; tad_linear_plan returns it as data); the kernel templates and their parameter blocks are
// in gemm_kernels.h (shared with gemm_w4.hip, the four-wave instantiations).
#include "gemm_kernels.h"

TAD_NAMESPACE_BEGIN
using namespace knobs;

// One step of an NT plan: the instantiation it names, on the grid it names.  Nothing is decided here.
template <int EPI, bool OUT_BF16, bool DIRECT>
static int launch_nt_step(const NtStep& s, const GemmNT& p, hipStream_t st) {
#define NT_LAUNCH(BM_, BN_, WM_, WN_, ST_, PER_) \
  hipLaunchKernelGGL((gemm_nt_kernel<BM_, BN_, WM_, WN_, ST_, EPI, OUT_BF16, PER_, DIRECT>), dim3(s.grid), dim3(s.block), 0, st, p)
  constexpr bool HAS_256 = !(EPI == EPI_RESIDUAL && OUT_BF16) && EPI != EPI_RESMOD;  // (else not instantiated: no registers / never needed; never planned)
  switch (s.kernel) {
    case 1:
      if constexpr (HAS_256) { if (s.persist) NT_LAUNCH(256, 256, 2, 4, 2, true); else NT_LAUNCH(256, 256, 2, 4, 2, false); }
      else if constexpr (!DIRECT) NT_LAUNCH(256, 256, 2, 4, 2, false);  // (unreachable; keeps the library's kernel list what it was)
      break;
    case 3: if (s.persist) NT_LAUNCH(256, 128, 4, 2, 3, true); else NT_LAUNCH(256, 128, 4, 2, 3, false); break;
    case 7: return launch_gemm_nt_w4(p, s.persist ? s.grid : 0, st);  // the four-wave 256 x 256 kernels (gemm_w4.hip)
    case 8: NT_LAUNCH(192, 128, 4, 2, 3, false); break;
    case 9: NT_LAUNCH(192, 128, 2, 2, 2, false); break;
    case 4: NT_LAUNCH(128, 64, 2, 2, 2, false); break;
    case 5: NT_LAUNCH(64, 64, 2, 2, 2, false); break;
    case 2: NT_LAUNCH(128, 128, 2, 2, 2, false); break;
    default: set_error("gemm_nt: no kernel %d", s.kernel); return TAD_EINVAL;
  }
#undef NT_LAUNCH
  return check_launch("gemm_nt");
}

// Split-K step.  Workspace: [arrival counters, one per tile | error word][partial tiles] (gemm_plan.h)
static int launch_nt_splitk_step(const NtStep& s, GemmNT p, void* ws, hipStream_t st) {
  p.sk_splits = s.sk_splits;
  p.sk_mode = s.sk_mode;
  p.sk_cnt = (unsigned*)ws;
  p.sk_err = nullptr;
  if (s.sk_mode == 0 && !sk_error_word(&p.sk_err)) { set_error("gemm_nt: split-K error word allocation failed"); return TAD_ELAUNCH; }
  p.sk_ws = (float*)((char*)ws + SK_HEADER_BYTES);
  if (s.sk_mode == 0 && hipMemsetAsync(ws, 0, SK_HEADER_BYTES, st) != hipSuccess) { set_error("gemm_nt: split-K counter reset failed"); return TAD_ELAUNCH; }
  const dim3 grid(s.grid), block(s.block);
  if (p.epi == EPI_PLAIN && p.c_bf16) hipLaunchKernelGGL((gemm_nt_kernel<256, 256, 2, 4, 2, EPI_PLAIN, true, false, false, true>), grid, block, 0, st, p);
  else if (p.epi == EPI_PLAIN) hipLaunchKernelGGL((gemm_nt_kernel<256, 256, 2, 4, 2, EPI_PLAIN, false, false, false, true>), grid, block, 0, st, p);
  else if (p.epi == EPI_RESIDUAL && !p.c_bf16) hipLaunchKernelGGL((gemm_nt_kernel<256, 256, 2, 4, 2, EPI_RESIDUAL, false, false, false, true>), grid, block, 0, st, p);
  else { set_error("gemm_nt: no split-K kernel for epilogue %d", p.epi); return TAD_EINVAL; }
  return check_launch("gemm_nt_splitk");
}

// rows [s.r0, s.r0 + s.rows) of the problem as the parameter block of the step's launch
static GemmNT step_params(const GemmNT& p, const NtStep& s) {
  GemmNT q = p;
  const size_t esz = p.c_bf16 ? 2 : 4, r0 = (size_t)s.r0;
  q.M = s.rows;
  q.row_base = p.row_base + s.r0;
  q.A = p.A + r0 * p.K;
  q.C = (char*)p.C + r0 * p.N * esz;
  if (p.residual && p.res_mod <= 0) q.residual = p.residual + r0 * p.N;
  if (p.preact) q.preact = p.preact + r0 * p.N;
  if (p.dgelu_h) q.dgelu_h = p.dgelu_h + r0 * p.N;
  q.epi = s.epi;
  q.group_m = s.group_m;
  return q;
}

static int launch_nt_one(const NtStep& s, const GemmNT& p, void* ws, hipStream_t st) {
  ++nt_launches;
  const GemmNT q = step_params(p, s);
  if (s.kernel == NT_SPLITK) return launch_nt_splitk_step(s, q, ws, st);
#define NT_CASE(E)                                                                              \
  case E:                                                                                       \
    if (q.c_bf16) return s.direct ? launch_nt_step<E, true, true>(s, q, st) : launch_nt_step<E, true, false>(s, q, st);  \
    return s.direct ? launch_nt_step<E, false, true>(s, q, st) : launch_nt_step<E, false, false>(s, q, st);
  switch (s.epi) {
    NT_CASE(EPI_PLAIN)
    NT_CASE(EPI_GELU)
    NT_CASE(EPI_RESIDUAL)
    NT_CASE(EPI_DGELU)
    NT_CASE(EPI_RESMOD)
    default: set_error("gemm_nt: bad epilogue %d", s.epi); return TAD_EINVAL;
  }
#undef NT_CASE
}

static int launch_gemm_nt(const GemmNT& p_in, hipStream_t st, void* ws = nullptr, size_t ws_bytes = 0) {
  if (const int rc = sk_check_pending_error()) return rc;
  GemmNT p = p_in;
  p.debug = gemm_debug;
  p.stamps = nt_stamps;
  const NtDesc d{p.M, p.N, p.K, p.epi, p.c_bf16, p.residual != nullptr, p.res_mod, p.rowscale != nullptr, p.rows_per_scale, p.colscale_cols, ws ? ws_bytes : 0};
  if (const int rc = nt_validate(d)) return rc;
  for (int64_t r0 = 0; r0 < d.M;) {
    const NtPlan plan = nt_plan(d, r0);
    nt_warn_ws_short(d, plan);
    for (int i = 0; i < plan.n; ++i)
      if (const int rc = launch_nt_one(plan.step[i], p, ws, st)) return rc;
    r0 = plan.next;
  }
  return TAD_OK;
}

static int launch_gemm_tn_kernel(const TnPlan& t, const GemmTN& p, hipStream_t st) {
  const dim3 grid(t.grid), block(t.block);
  switch (t.kernel) {
    case TN_W4: return launch_gemm_tn_w4(p, t.grid, st);
    case TN_PDEEP: hipLaunchKernelGGL((gemm_tn_kernel<256, 256, 2, 4, 2, true>), grid, block, 0, st, p); break;
    case TN_W8: hipLaunchKernelGGL((gemm_tn_kernel<256, 256, 2, 4, 2>), grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL((gemm_tn_kernel<256, 128, 4, 2, 3>), grid, block, 0, st, p); break;
  }
  return check_launch("gemm_tn");
}

// bias_out2 != null: the column sums of the first third of the columns go to bias_out, those of the last third to bias_out2 and the
// middle third is dropped (the qkv Linear: q_bias / no k bias / v_bias, modeling_finetune.py:69-76, 89-92)
static int launch_gemm_tn(const uint16_t* P, const uint16_t* Q, float* out, float* bias_out, float* bias_out2, int accumulate, void* ws,
                          size_t ws_bytes, int64_t Mr, int N, int K, hipStream_t st) {
  if (const int rc = sk_check_pending_error()) return rc;  // (a failed in-launch split-K combine is reported by the NEXT tad_linear_* call, whichever it is)
  if (!(Mr > 0 && N > 0 && K > 0)) { set_error("gemm_tn: empty problem"); return TAD_EINVAL; }
  if (N % 8 || K % 8) { set_error("gemm_tn: N=%d and K=%d must be multiples of 8", N, K); return TAD_EINVAL; }
  if (Mr * (int64_t)N * 2 >= (1ll << 32) || Mr * (int64_t)K * 2 >= (1ll << 32)) { set_error("gemm_tn: operand exceeds 4 GiB"); return TAD_EINVAL; }
  const TnPlan t = tn_plan(Mr, N, K);
  if (ws_bytes < t.ws_bytes) { set_error("gemm_tn: workspace too small"); return TAD_ENOSPACE; }
  GemmTN p{};
  p.P = P; p.Q = Q; p.slab = (float*)ws; p.Mr = (int)Mr; p.N = N; p.K = K;
  p.debug = gemm_debug;
  p.rows_per_split = t.rows_per_split;
  p.bias_slab = bias_out ? p.slab + (size_t)t.splits * N * K : nullptr;
  if (const int rc = launch_gemm_tn_kernel(t, p, st)) return rc;
  if (!bias_out) return launch_reduce_partials(p.slab, out, t.splits, (int64_t)N * K, accumulate, st);
  // slab reduction and bias column sums in one launch (N * K % 4 == 0 and N % 4 == 0 hold: N, K are multiples of 8)
  if (bias_out2) return launch_reduce_dw(p.slab, out, t.splits, (int64_t)N * K, accumulate, p.bias_slab, t.splits * t.tiles_k, N, bias_out, bias_out2, N / 3, 2 * (N / 3), st);
  return launch_reduce_dw(p.slab, out, t.splits, (int64_t)N * K, accumulate, p.bias_slab, t.splits * t.tiles_k, N, bias_out, nullptr, N, 0, st);
}

// Two weight gradients over the same rows with the same K as ONE launch of the four-wave kernel (GemmTN::N1): out1 [N1, K] = P1^T Q1 with its
// bias column sums (bias_out1, or split into bias_out1 / bias_out1b as for the qkv Linear), out2 [N2, K] = P2^T Q2.  A small problem pays for
// filling the chip with many splits -- the 768 x 768 proj gradient of ViT-B runs 9 tiles x 28 splits: 28 slabs to write and sum, an epilogue per
// 28 reduction tiles -- where the pair (36 tiles x 7 splits: the shape of the fc1 gradient) pays once: qkv + proj 160.8 + 71.7 us apart, ~197 as a
// pair.  Falls back to two launches when the pair does not fit the kernel (TnPlan::fits: K not on 256-wide tiles, N1 not a multiple of 256, four-wave kernel off).
// The summation order over the rows differs from the single launches' (another split count), as between any two batch sizes.
static int launch_gemm_tn_pair(const uint16_t* P1, const uint16_t* Q1, float* out1, float* bias_out1, float* bias_out1b, int N1, const uint16_t* P2,
                               const uint16_t* Q2, float* out2, int N2, int accumulate, void* ws, size_t ws_bytes, int64_t Mr, int K, hipStream_t st) {
  if (const int rc = sk_check_pending_error()) return rc;
  if (!(Mr > 0 && N1 > 0 && N2 > 0 && K > 0)) { set_error("gemm_tn_pair: empty problem"); return TAD_EINVAL; }
  if (N1 % 8 || N2 % 8 || K % 8) { set_error("gemm_tn_pair: N1=%d, N2=%d and K=%d must be multiples of 8", N1, N2, K); return TAD_EINVAL; }
  const int N = N1 + N2;
  const TnPlan t = tn_plan(Mr, N, K, N1, ws_bytes);
  if (!t.fits) {
    const int rc = launch_gemm_tn(P1, Q1, out1, bias_out1, bias_out1b, accumulate, ws, ws_bytes, Mr, N1, K, st);
    if (rc) return rc;
    return launch_gemm_tn(P2, Q2, out2, nullptr, nullptr, accumulate, ws, ws_bytes, Mr, N2, K, st);
  }
  GemmTN p{};
  p.P = P1; p.Q = Q1; p.P2 = P2; p.Q2 = Q2; p.N1 = N1;
  p.slab = (float*)ws; p.Mr = (int)Mr; p.N = N; p.K = K; p.rows_per_split = t.rows_per_split;
  p.bias_slab = bias_out1 ? p.slab + (size_t)t.splits * N * K : nullptr;
  if (const int rc = launch_gemm_tn_kernel(t, p, st)) return rc;
  // slabs [splits][N][K]: rows [0, N1) -> out1, rows [N1, N) -> out2, both in one launch (with the bias column sums of the first problem)
  const int64_t n1 = (int64_t)N1 * K, n = (int64_t)N * K;
  if (!bias_out1) return launch_reduce_dw_pair(p.slab, out1, out2, n1, t.splits, n, accumulate, nullptr, 0, 0, nullptr, nullptr, 0, 0, st);
  if (bias_out1b) return launch_reduce_dw_pair(p.slab, out1, out2, n1, t.splits, n, accumulate, p.bias_slab, t.splits * t.tiles_k, N, bias_out1, bias_out1b, N1 / 3, 2 * (N1 / 3), st);
  return launch_reduce_dw_pair(p.slab, out1, out2, n1, t.splits, n, accumulate, p.bias_slab, t.splits * t.tiles_k, N, bias_out1, nullptr, N1, 0, st);
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
  // x, w: 16-byte LDS-DMA pieces; bias, y, preact, residual: 16-byte epilogue accesses; ws: 16-byte partial tiles; gamma, rowscale: scalar reads
  TAD_REQUIRE_ALIGNED("linear_fwd", x, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd", w, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd", bias, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd", y, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd", preact, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd", residual, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd", ws, 16);
  GemmNT p{};
  p.A = x; p.B = w; p.C = y; p.bias = bias; p.c_bf16 = (y_dtype == TAD_OP16);
  p.M = (int)M; p.N = N; p.K = K;
  p.rows_per_scale = rows_per_scale > 0 ? rows_per_scale : 1;
  if (epilogue == TAD_EPI_BIAS_GELU) { p.epi = EPI_GELU; p.preact = preact; }
  else if (epilogue == TAD_EPI_BIAS_RESIDUAL) { p.epi = EPI_RESIDUAL; p.residual = residual; p.gamma = gamma; p.rowscale = rowscale; }
  else p.epi = EPI_PLAIN;
  return launch_gemm_nt(p, (hipStream_t)stream, ws, ws ? ws_bytes : 0);
}

int tad_linear_fwd_qkv(const uint16_t* x, const uint16_t* w, const float* q_bias, const float* v_bias, void* y, int y_dtype, float q_prescale,
                       int64_t M, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(x && w && y, "linear_fwd_qkv: null pointer");
  TAD_REQUIRE((q_bias == nullptr) == (v_bias == nullptr), "linear_fwd_qkv: q_bias and v_bias come together");
  TAD_REQUIRE(y_dtype == TAD_F32 || y_dtype == TAD_OP16, "linear_fwd_qkv: bad y_dtype %d", y_dtype);
  TAD_REQUIRE(N > 0 && N % 12 == 0, "linear_fwd_qkv: N=%d must be 3 x a multiple of 4", N);
  TAD_REQUIRE(M > 0 && M < (1ll << 31), "linear_fwd_qkv: bad M");
  TAD_REQUIRE(q_prescale > 0.f, "linear_fwd_qkv: q_prescale must be positive (1 = plain)");
  TAD_REQUIRE(q_prescale == 1.f || N % 24 == 0, "linear_fwd_qkv: q_prescale needs N/3 = %d to be a multiple of 8", N / 3);
  TAD_REQUIRE_ALIGNED("linear_fwd_qkv", x, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd_qkv", w, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd_qkv", q_bias, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd_qkv", v_bias, 16);
  TAD_REQUIRE_ALIGNED("linear_fwd_qkv", y, 16);
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
  // dy, x: 16-byte LDS-DMA pieces; the slab reduction reads ws and reads / writes every output as float4
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_qkv", dy, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_qkv", x, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_qkv", dW, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_qkv", dq_bias, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_qkv", dv_bias, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_qkv", ws, 16);
  return launch_gemm_tn(dy, x, dW, dq_bias, dv_bias, accumulate, ws, ws_bytes, M, N, K, (hipStream_t)stream);
}

int tad_linear_bwd_weight_pair(const uint16_t* dy1, const uint16_t* x1, float* dW1, float* db1, float* db1b, int N1, const uint16_t* dy2,
                               const uint16_t* x2, float* dW2, int N2, int accumulate, void* ws, size_t ws_bytes, int64_t M, int K, tad_stream_t stream) {
  TAD_REQUIRE(dy1 && x1 && dW1 && dy2 && x2 && dW2 && ws, "linear_bwd_weight_pair: null pointer");
  TAD_REQUIRE(!db1b || db1, "linear_bwd_weight_pair: db1b (the v_bias third) comes with db1 (the q_bias third)");
  TAD_REQUIRE(!db1b || (N1 > 0 && N1 % 12 == 0), "linear_bwd_weight_pair: N1=%d must be 3 x a multiple of 4 for the split bias sums", N1);
  // the slab reduction reads and writes float4s through every output (dW2 is usually a view into the flat gradient buffer)
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_pair", dW1, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_pair", dW2, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_pair", db1, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_pair", db1b, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_pair", dy1, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_pair", x1, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_pair", dy2, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_pair", x2, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight_pair", ws, 16);
  return launch_gemm_tn_pair(dy1, x1, dW1, db1, db1b, N1, dy2, x2, dW2, N2, accumulate, ws, ws_bytes, M, K, (hipStream_t)stream);
}

int tad_linear_bwd_input(const uint16_t* dy, const uint16_t* wT, void* dx, int dx_dtype, const uint16_t* gelu_preact, void* ws, size_t ws_bytes,
                         int64_t M, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(dy && wT && dx, "linear_bwd_input: null pointer");
  TAD_REQUIRE(dx_dtype == TAD_F32 || dx_dtype == TAD_OP16, "linear_bwd_input: bad dx_dtype %d", dx_dtype);
  TAD_REQUIRE(M > 0 && M < (1ll << 31), "linear_bwd_input: bad M");
  TAD_REQUIRE_ALIGNED("linear_bwd_input", dy, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_input", wT, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_input", dx, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_input", gelu_preact, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_input", ws, 16);
  GemmNT p{};
  p.A = dy; p.B = wT; p.C = dx; p.c_bf16 = (dx_dtype == TAD_OP16);
  p.M = (int)M; p.N = K; p.K = N;  // dx[M,K] = dy[M,N] * (wT[K,N])^T
  p.rows_per_scale = 1;
  p.epi = gelu_preact ? EPI_DGELU : EPI_PLAIN;
  p.dgelu_h = gelu_preact;
  return launch_gemm_nt(p, (hipStream_t)stream, ws, ws ? ws_bytes : 0);
}

int tad_linear_bwd_weight(const uint16_t* dy, const uint16_t* x, float* dW, float* db, int accumulate, void* ws, size_t ws_bytes,
                          int64_t M, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(dy && x && dW && ws, "linear_bwd_weight: null pointer");
  TAD_REQUIRE_ALIGNED("linear_bwd_weight", dy, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight", x, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight", dW, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight", db, 16);
  TAD_REQUIRE_ALIGNED("linear_bwd_weight", ws, 16);
  return launch_gemm_tn(dy, x, dW, db, nullptr, accumulate, ws, ws_bytes, M, N, K, (hipStream_t)stream);
}

// ---- PatchEmbed = im2col + NT GEMM with bias and broadcast pos_embed in the epilogue
int tad_patch_embed_fwd(const float* x, const uint16_t* w_bf16, const float* bias, const float* pos, float* out, uint16_t* cols, int B,
                        int C, int T, int H, int W, int tubelet, int patch, int D, tad_stream_t stream) {
  TAD_REQUIRE(x && w_bf16 && out && cols, "patch_embed_fwd: null pointer");
  // (x: tad_im2col_tubelets answers for it; cols is also the GEMM's x operand: 16-byte LDS-DMA pieces whatever the patch size)
  TAD_REQUIRE_ALIGNED("patch_embed_fwd", cols, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_fwd", w_bf16, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_fwd", bias, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_fwd", pos, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_fwd", out, 16);
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
  TAD_REQUIRE_ALIGNED("patch_embed_gemm", cols, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_gemm", w_bf16, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_gemm", bias, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_gemm", pos, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_gemm", out, 16);
  GemmNT p{};
  p.A = cols; p.B = w_bf16; p.C = out; p.bias = bias; p.c_bf16 = 0;
  p.M = (int)M; p.N = D; p.K = K;
  p.rows_per_scale = 1;
  p.epi = EPI_RESIDUAL;
  p.residual = pos;
  p.res_mod = ntok;
  return launch_gemm_nt(p, (hipStream_t)stream);
}

int tad_patch_embed_bwd(const uint16_t* dy_bf16, const uint16_t* cols, float* dW, float* db, void* ws, size_t ws_bytes, int64_t M, int D,
                        int K, tad_stream_t stream) {
  TAD_REQUIRE(dy_bf16 && cols && dW && ws, "patch_embed_bwd: null pointer");
  TAD_REQUIRE_ALIGNED("patch_embed_bwd", dy_bf16, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_bwd", cols, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_bwd", dW, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_bwd", db, 16);
  TAD_REQUIRE_ALIGNED("patch_embed_bwd", ws, 16);
  return tad_linear_bwd_weight(dy_bf16, cols, dW, db, 0, ws, ws_bytes, M, D, K, stream);
}

}  // extern "C"
