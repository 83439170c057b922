/*
 * tad_mi355x_recon.h -- the RECONSTRUCTION ABI: the fifth surface of this package, tadr_*, TADR_ABI_VERSION 1, in a shared library of
 * its own, libtad_mi355x_recon.so (csrc/mae_reconstruct.hip).  libtad_mi355x.so is held at its three surfaces (tad_*, tadx_*, tadp_*)
 * and libtad_mi355x_serve.so at its one (tads_*, from the single source iv2_serve.hip), so what turning an MAE prediction back into
 * frames adds is linked apart, the way the serving surface was.  The library is self-contained: it is compiled with hidden visibility,
 * exports these entry points and nothing else, and keeps an error text of its own behind tadr_last_error_string().
 *
 * Every other convention is the core header's: plain C, device pointers and explicit sizes, `stream` a hipStream_t passed as void*,
 * 0 or a negative TAD_E* code, no allocation, no synchronisation, row-major contiguous operands, every check made on the host before
 * anything is launched.  Nothing here takes a workspace and nothing uses atomics: two calls give the same bits.
 *
 * Pointer alignment (refused with TAD_EINVAL and "<entry point>: <argument> is misaligned: it must be N-byte aligned"; NULL for an
 * optional argument passes):
 *   - videos, pred, slot, err are read and written one 4-byte element at a time:                             4 bytes
 *   - frames may be ANY address: rows of bytes leave as whole 4-byte words where the row's own address allows and as single bytes at
 *     its two ends; the bytes written are the same at every address.
 * tests/test_reconstruct_abi_cpu.py holds this as a table.
 */
#ifndef TAD_MI355X_RECON_H
#define TAD_MI355X_RECON_H

#include "tad_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TADR_ABI_VERSION 1

int tadr_abi_version(void);
/* the text of the last error of a tadr_* call on this thread */
const char* tadr_last_error_string(void);

/* ---- MAE reconstruction: the inverse of the target arithmetic of tad_mae_target (engine_for_pretraining.py:51-66), one pass, one
 * workgroup per token.  A masked clip comes back as uint8 frames -- visible patches from the clip, masked patches from the prediction --
 * together with the per-token reconstruction error.
 *   videos [B,3,T,H,W] f32, the normalised clip;  pred [B*n_mask, tubelet*patch*patch*3] f32 in the layout 'n (p0 p1 p2) c' of
 *   tad_mae_target's labels (NULL iff n_mask == 0);  slot [B,N] int32: the row of pred inside the clip's n_mask rows that predicts the
 *   token, -1 = the token is visible;  frames [B,T,H,W,3] uint8 RGB (nullable);  err [B,N] f32 (nullable; not both NULL).
 *   N = (T/tubelet)(H/patch)(W/patch), tokens in PatchEmbed's order (t, h, w).  mean3 / std3: HOST arrays of three floats.
 * For every token, per (patch, channel) over its tubelet*patch*patch pixels: v = fma(videos, std, mean) (ONE rounding), and -- where needed --
 * the statistics exactly as tad_mae_target takes them: the mean as two floats m = mu + corr, the UNBIASED variance of the residuals,
 * s = sqrt(var) + 1e-6 and inv = 1 / s.
 *   visible token (slot < 0, or slot >= n_mask: a value outside [-1, n_mask) counts as -1):
 *     byte = clamp(rint(g * v), 0, 255) with g = 255 * visible_gain rounded to f32 once;  err = 0.
 *   masked token, normalize_target != 0:  r = pred * s + m,  target = (v - mu - corr) * inv  (tad_mae_target's label),
 *     byte = clamp(rint(255 * r), 0, 255);  err[b, tok] = the mean over the tubelet*patch*patch*3 entries of (pred - target)^2.
 *   masked token, normalize_target == 0:  r = pred, target = v.
 * rint rounds halves to even.  Non-finite values: NaN gives byte 0, +inf gives 255, -inf gives 0; err carries them as they come.
 * The squares of a token are summed in a fixed order (per lane in pixel order, the 64 lanes by a butterfly, then (R + G) + B).
 * EVERY byte of frames and EVERY float of err is written exactly once (the caller does not zero-fill); no store address depends on
 * slot -- slot only chooses what is read -- and a clip reads no row of pred but its own n_mask.
 * Refused before any launch, each naming its argument: T % tubelet, H % patch, W % patch; tubelet*patch*patch outside [2, 1024]
 * (tad_mae_target's range: the unbiased variance needs two pixels); B < 1; n_mask outside [0, N]; pred NULL with n_mask > 0; both
 * outputs NULL; visible_gain outside [0, 1] or NaN; a std3 entry <= 0; B * N above 2^31 - 1. */
/* Alignment: videos, pred, slot, err: 4 bytes; frames: any address. */
int tadr_mae_reconstruct(const float* videos, const float* pred, const int32_t* slot, uint8_t* frames, float* err, int B, int n_mask,
                         int T, int H, int W, int tubelet, int patch, const float* mean3, const float* std3, int normalize_target,
                         float visible_gain, tad_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TAD_MI355X_RECON_H */
