/*
 * tad_mi355x_ext.h -- the EXTENSION ABI of libtad_mi355x.so: entry points added after the core ABI (tad_mi355x.h, TAD_ABI_VERSION 5)
 * was frozen.  They live in the same shared library, are named tadx_*, carry a version of their own (tadx_abi_version) and follow
 * every convention of the core header: plain C, device pointers and explicit sizes, `stream` a hipStream_t passed as void*, 0 or a
 * negative TAD_E* code, the text of the last error from tad_last_error_string(), no allocation, no synchronisation, scratch memory
 * from the caller with its size from a *_workspace_bytes() query, row-major contiguous operands.
 *
 * The 16-bit operand format of a call is a RUN-TIME argument here (TAD_BF16 or TAD_F16, as in tad_attn_colsum): one entry point
 * serves both formats and there are no _f16 twins.  Every 16-bit value is rounded once, to nearest even; a NaN stays a NaN.
 *
 * Version 1: RMSNorm and the q / k RMS normalisation of the InternVideo2 family (csrc/rmsnorm.hip;
 * other_models/InternVideo2_single_modality/models/internvideo2.py: RMSNorm, Attention.qk_normalization).
 *
 * Pointer alignment (checked on the host before anything is launched, refused with TAD_EINVAL and
 * "<entry point>: <argument> is misaligned: it must be N-byte aligned"; NULL for an optional argument passes):
 *   - f32 row operands, the gammas, the gamma gradients and the workspaces are moved as float4:        16 bytes
 *   - 16-bit row operands are moved as packed groups of four:                                          8 bytes
 *   - a y / dy whose type is selectable owes 16 bytes as f32 and 8 bytes as a 16-bit tensor
 *   - the row statistics (rrms, rr) are read and written one float at a time:                          any
 * tests/alignment_contract_ext.py holds this as a table.
 */
#ifndef TAD_MI355X_EXT_H
#define TAD_MI355X_EXT_H

#include "tad_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TADX_ABI_VERSION 1

int tadx_abi_version(void);

/* ---- RMSNorm: y = x * rsqrt(mean(x^2) + eps) * gamma over rows of D f32 elements (D % 4 == 0, D <= 2048).
 * x [rows,D] f32 (read once), gamma [D] f32, y [rows,D] in y_dtype (TAD_F32, TAD_BF16 or TAD_F16), rrms [rows] f32 (nullable) =
 * rsqrt(mean(x^2) + eps), what the backward needs.  An all-zero row gives y = 0 and rrms = rsqrt(eps). */
/* Alignment: x, gamma: 16 bytes; y: 16 bytes (f32) or 8 bytes (16-bit); rrms: any. */
int tadx_rmsnorm_fwd(const float* x, const float* gamma, void* y, int y_dtype, float* rrms, int64_t rows, int D, float eps,
                     tad_stream_t stream);
/* With xh = x * rrms and t = dy * gamma:
 *   dx = rrms * (t - xh * mean(t * xh)) (+ dres),   dgamma (+)= sum over rows of dy * xh.
 * dy [rows,D] in dy_dtype (TAD_F32, TAD_BF16 or TAD_F16); dres [rows,D] f32 (nullable): a gradient that reaches x by another way (the
 * residual); dx [rows,D] f32; dx16 [rows,D] (nullable): the same values rounded to dx16_fmt (TAD_BF16 / TAD_F16; ignored without dx16);
 * dgamma [D] f32, overwritten, or added to when accumulate != 0.  ws: tadx_rmsnorm_bwd_workspace_bytes(rows, D) bytes (TAD_ENOSPACE
 * if smaller).  Per-block column partials reduced in a fixed order, no atomics: two calls give the same bits. */
size_t tadx_rmsnorm_bwd_workspace_bytes(int64_t rows, int D);
/* Alignment: dy: 16 bytes (f32) or 8 bytes (16-bit); x, gamma, dres, dx, dgamma, ws: 16 bytes; dx16: 8 bytes; rrms: any. */
int tadx_rmsnorm_bwd(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* rrms, const float* dres, float* dx,
                     uint16_t* dx16, int dx16_fmt, float* dgamma, int accumulate, void* ws, size_t ws_bytes, int64_t rows, int D,
                     tad_stream_t stream);

/* ---- q / k RMS normalisation over the full H*d width, between the qkv Linear and tad_attn_fwd (Attention.forward with
 * qk_normalization: q_norm / k_norm on the flattened heads).  One pass per row of the f32 qkv [M,3A] (A = H*d, A % 4 == 0, A <= 2048,
 * column order [3][H][d]):
 *   q third -> q * rq * gq * q_out_scale,   k third -> k * rk * gk,   v third -> v,      each rounded once to fmt (TAD_BF16 / TAD_F16)
 * with rq / rk = rsqrt(mean over the third's A columns + eps), kept in rr [M,2] f32 (nullable) as (rq, rk).  The v third has the bits
 * of tad_cast_f32_bf16 / _f16.  qkv16 [M,3A] is what tad_attn_fwd reads: q_out_scale (> 0) carries its q contract, scale * log2(e)
 * for q_prescaled != 0 and 1 for plain q -- the factor cannot ride in the qkv Linear's epilogue here, the norm comes after it. */
/* Alignment: qkv32, gq, gk: 16 bytes; qkv16: 8 bytes; rr: any. */
int tadx_qk_rmsnorm_fwd(const float* qkv32, const float* gq, const float* gk, uint16_t* qkv16, int fmt, float* rr, float q_out_scale,
                        int64_t M, int A, float eps, tad_stream_t stream);
/* The way back: dqkv16 [M,3A] (fmt) is tad_attn_bwd's output, qkv32 / gq / gk / rr the forward's operands.
 *   dqkv_pre16 [M,3A] (fmt): the gradient of the qkv Linear's output (ready for tad_linear_bwd_input / _bwd_weight); its v third is a copy
 *   dgq, dgk [A] f32: the gamma gradients, overwritten, or added to when accumulate != 0.
 * Which q the incoming dq refers to: the q slot of tad_attn_bwd's dqkv is the gradient of the PLAIN q under either q contract
 * (tad_mi355x.h), i.e. of the stored q third divided by the factor tad_attn_fwd was told it carries.  With q_out_scale equal to that
 * factor -- the only consistent use -- dq already is the gradient of the normalised q, q * rq * gq, so q_out_scale is NOT applied to
 * it: neither as a factor (the gradient of the stored values, which tad_attn_bwd does not produce) nor as a divisor.  The argument is
 * validated (> 0) so that a call mirrors its forward; it does not enter the arithmetic.
 * ws: tadx_qk_rmsnorm_bwd_workspace_bytes(M, A) bytes.  Fixed-order reduction, no atomics. */
size_t tadx_qk_rmsnorm_bwd_workspace_bytes(int64_t M, int A);
/* Alignment: dqkv16, dqkv_pre16: 8 bytes; qkv32, gq, gk, dgq, dgk, ws: 16 bytes; rr: any. */
int tadx_qk_rmsnorm_bwd(const uint16_t* dqkv16, int fmt, const float* qkv32, const float* gq, const float* gk, const float* rr,
                        float q_out_scale, uint16_t* dqkv_pre16, float* dgq, float* dgk, int accumulate, void* ws, size_t ws_bytes,
                        int64_t M, int A, tad_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TAD_MI355X_EXT_H */
