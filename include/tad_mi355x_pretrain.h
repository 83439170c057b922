/*
 * tad_mi355x_pretrain.h -- the PRE-TRAINING ABI of libtad_mi355x.so: the third surface of the library, beside the frozen core ABI
 * (tad_mi355x.h, tad_*, TAD_ABI_VERSION 5) and the extension ABI (tad_mi355x_ext.h, tadx_*, TADX_ABI_VERSION 1, held at its seven
 * entry points).  Its entry points live in the same shared library, are named tadp_*, carry a version of their own (tadp_abi_version)
 * and follow every convention of the core header: plain C, device pointers and explicit sizes, `stream` a hipStream_t passed as void*,
 * 0 or a negative TAD_E* code, the text of the last error from tad_last_error_string(), no allocation, no synchronisation, row-major
 * contiguous operands.  Nothing here takes a workspace, and nothing here has a 16-bit operand: every value is f32.
 *
 * Version 1: the entry of the InternVideo2 MAE encoder (csrc/visible_tokens.hip;
 * other_models/InternVideo2_single_modality/models/internvideo2_pretrain_videomae.py, forward_features:
 * `x = patch_embed(x) + pos_embed; x_vis = x[~mask].reshape(B, -1, C)`) with a TRAINABLE position table: the add and the selection of
 * the visible tokens in one pass over the visible rows, and on the way back the scatter of the gradient and the table's gradient in
 * one launch with a fixed summation order.
 *
 * Pointer alignment (checked on the host before anything is launched, refused with TAD_EINVAL and
 * "<entry point>: <argument> is misaligned: it must be N-byte aligned"; NULL for an optional argument passes):
 *   - every f32 operand (x, pos, out, g, dx, dpos) is moved as float4:                                   16 bytes
 *   - the index tables (tok, slot) are read one int at a time:                                           any
 * tests/test_visible_tokens_abi_cpu.py holds this as a table.
 */
#ifndef TAD_MI355X_PRETRAIN_H
#define TAD_MI355X_PRETRAIN_H

#include "tad_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TADP_ABI_VERSION 1

int tadp_abi_version(void);

/* ---- Visible tokens: out[b*Nv + i, :] = x[b*N + tok[b,i], :] + pos[tok[b,i], :]   (one f32 add per element)
 * x [B*N,D] f32, pos [N,D] f32, tok [B,Nv] int32 (the visible tokens of each clip, in the order the output keeps), out [B*Nv,D] f32.
 * B, N, Nv, D > 0, Nv <= N, D % 4 == 0.  Rows of x that no tok names are never read.
 * The indices are device data and cannot be checked on the host.  The caller owes: every tok value lies in [0, N) (a value outside
 * reads outside x and pos); the values of one clip are distinct -- the forward is still defined when they repeat (the row is delivered
 * twice), its backward below is not. */
/* Alignment: x, pos, out: 16 bytes; tok: any. */
int tadp_visible_tokens_fwd(const float* x, const float* pos, const int32_t* tok, float* out, int B, int N, int Nv, int D,
                            tad_stream_t stream);
/* The way back, one launch.  g [B*Nv,D] f32 is the gradient of out; slot [B,N] int32 is the inverse of tok: slot[b,n] = the position of
 * token n among clip b's visible tokens (tok[b, slot[b,n]] == n), or -1 where clip b does not see token n.
 *   dx   [B*N,D] f32 (nullable): g[b*Nv + slot[b,n], :] where slot[b,n] >= 0, +0 elsewhere.  EVERY row is written: no zero fill is owed.
 *   dpos [N,D]   f32 (nullable): per (n, column) the f32 sum of those g values over b = 0, 1, ..., B-1 IN THAT ORDER, starting from +0.
 *                With accumulate != 0 the finished sum is added to what dpos held (one more add), else it overwrites.
 * dx and dpos may each be NULL, not both.  One thread owns a float4 column group of one token and walks the clips: no atomics, no
 * workspace, two calls give the same bits.
 * A slot value outside [-1, Nv) is treated as -1.  Where slot is not the inverse of a tok with distinct values per clip (two tokens of a
 * clip share a slot, or a visible row has none) the result is the gradient of no forward: defined memory-wise, meaningless otherwise. */
/* Alignment: g, dx, dpos: 16 bytes; slot: any. */
int tadp_visible_tokens_bwd(const float* g, const int32_t* slot, float* dx, float* dpos, int accumulate, int B, int N, int Nv, int D,
                            tad_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TAD_MI355X_PRETRAIN_H */
