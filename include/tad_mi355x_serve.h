/*
 * tad_mi355x_serve.h -- the SERVING ABI: the fourth surface of this package, tads_*, TADS_ABI_VERSION 1, and the only one that lives in
 * a shared library of its own, libtad_mi355x_serve.so (csrc/iv2_serve.hip).  libtad_mi355x.so is held at its three surfaces (the core
 * ABI tad_*, the extension ABI tadx_* at seven entry points, the pre-training ABI tadp_* at three), so what serving the InternVideo2
 * family adds is linked apart.  That library is self-contained: it is compiled with hidden visibility, exports these entry points and
 * nothing else, and keeps an error text of its own behind tads_last_error_string() -- NOT behind tad_last_error_string().
 *
 * Every other convention is the core header's: plain C, device pointers and explicit sizes, `stream` a hipStream_t passed as void*,
 * 0 or a negative TAD_E* code, no allocation, no synchronisation, row-major contiguous operands, every check made on the host before
 * anything is launched.  Nothing here takes a workspace.  The 16-bit format of an output is an argument (TAD_BF16 / TAD_F16): no twins.
 *
 * Pointer alignment (refused with TAD_EINVAL and "<entry point>: <argument> is misaligned: it must be N-byte aligned"; NULL for an
 * optional argument passes):
 *   - every f32 operand is moved as float4:                                                                 16 bytes
 *   - the 16-bit output xn is stored four values (8 bytes) at a time:                                         8 bytes
 * tests/test_iv2_serve_abi_cpu.py holds this as a table.
 */
#ifndef TAD_MI355X_SERVE_H
#define TAD_MI355X_SERVE_H

#include "tad_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TADS_ABI_VERSION 1

int tads_abi_version(void);
/* the text of the last error of a tads_* call on this thread */
const char* tads_last_error_string(void);

/* ---- The entry of the InternVideo2 encoder (internvideo2.py, forward: `x = cat((cls_token.expand(B,-1,-1), x), 1) + pos_embed`), one pass:
 *   out[b, 0, :]     = cls + pos[0]
 *   out[b, 1 + n, :] = patch[b, n, :] + pos[1 + n]
 * patch [B,N,D] f32, cls [D] f32, pos [N+1,D] f32, out [B,N+1,D] f32.  B, N, D > 0, D % 4 == 0.  One f32 add per element: the bits of
 * the torch expression. */
/* Alignment: patch, cls, pos, out: 16 bytes. */
int tads_class_token_entry_fwd(const float* patch, const float* cls, const float* pos, float* out, int B, int N, int D,
                               tad_stream_t stream);
/* The way back, one launch.  g [B,N+1,D] f32 is the gradient of out.
 *   dpatch [B,N,D] f32 (nullable): g[b, 1 + n, :]; EVERY row is written.
 *   dpos   [N+1,D] f32 (nullable): per (t, column) the f32 sum of g[b, t] over b = 0, 1, ..., B-1 IN THAT ORDER (it starts from g[0, t]).
 *   dcls   [D]     f32 (nullable): that same sum for t = 0.
 * With accumulate != 0 the finished sums are added to what dpos / dcls held (one more add each), else they overwrite; dpatch is always
 * overwritten.  Each output may be NULL, not all three.  One thread owns a float4 column group of one token and walks the clips: no
 * atomics, no workspace, two calls give the same bits. */
/* Alignment: g, dpatch, dpos, dcls: 16 bytes. */
int tads_class_token_entry_bwd(const float* g, float* dpatch, float* dpos, float* dcls, int accumulate, int B, int N, int D,
                               tad_stream_t stream);

/* ---- The evaluation-only tail of a half block and the norm behind it, one pass over the rows:
 *   x_out = x + y * ls_gamma             (ls_gamma NULL: x + y); the product and the sum are each rounded on their own
 *   xn    = x_out * rsqrt(mean(x_out^2) + eps) * norm_gamma, rounded once to xn_fmt (TAD_BF16 / TAD_F16)
 * x, y, x_out [rows,D] f32; ls_gamma, norm_gamma [D] f32; xn [rows,D] 16-bit.  rows > 0, D % 4 == 0, D <= 2048.
 * norm_gamma and xn come together or not at all (after the last block: the residual alone; xn_fmt is not looked at then).
 * x_out may be x itself (in place); it may not be y.  No statistics are kept: there is no backward. */
/* Alignment: x, y, ls_gamma, norm_gamma, x_out: 16 bytes; xn: 8 bytes. */
int tads_residual_rmsnorm_fwd(const float* x, const float* y, const float* ls_gamma, const float* norm_gamma, float* x_out, void* xn,
                              int xn_fmt, int64_t rows, int D, float eps, tad_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TAD_MI355X_SERVE_H */
