/*
 * tad_mi355x.h -- C ABI of libtad_mi355x.so: the MI355X (gfx950) kernels behind
 * simple-tad's Video-ViT forward/backward path.
 *
 * The reference (tue-mps/simple-tad) has no FFI of its own: its hot path is the
 * Python nn.Module surface of modeling_finetune.py, whose arithmetic runs inside
 * third-party wheels (ATen / cuDNN / cuBLAS / flash-attn).  Each entry point below
 * names the reference call site whose native arithmetic it replaces.  The nearest
 * existing analogue of a C-level boundary in the reference is
 *   flash_attn_varlen_qkvpacked_func(qkv, cu_seqlens, max_s, dropout_p, softmax_scale, causal)
 * (flash_attention_class.py:47-50).
 *
 * Conventions (all entry points):
 *   - plain C: device pointers + explicit sizes; no torch / C++ types.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).
 *   - return 0 on success, a negative TAD_E* code otherwise; never throw; the text of
 *     the last error on the calling thread is available from tad_last_error_string().
 *   - never allocate device memory, never synchronise the device, re-entrant per stream.
 *     Scratch memory is passed in by the caller; sizes come from the *_workspace_bytes()
 *     queries.
 *   - "bf16" = bfloat16 stored as uint16_t; "f32" = IEEE float.  Every uint16_t operand below is bf16 in the tad_* entry points and
 *     IEEE half in their tad_*_f16 twins (same kernels compiled for the other operand format; see the end of this header).
 *   - row-major everywhere; leading dimension == number of columns unless stated.
 *
 * Pointer alignment (what the caller owes for every device pointer; checked on the host before anything is launched):
 *   - The general rule: a device pointer must be 16-byte aligned.  The kernels move tensors as 16-byte pieces (float4 / uint4 loads and
 *     stores, 16-byte global -> LDS transfers).  A pointer that breaks its requirement is refused with TAD_EINVAL and a message
 *     "<entry point>: <argument> is misaligned: it must be N-byte aligned"; nothing is launched and no output is touched.  NULL for an
 *     optional argument passes.  Fresh allocations (hipMalloc, torch) are 256-byte aligned; what breaks the rule is a view that starts
 *     inside one, e.g. buf + 1.
 *   - Exceptions are stated where they apply, as "Alignment:" lines at the entry points below:
 *       "N bytes"  a narrower requirement (the widest access through that pointer is N bytes), enforced the same way;
 *       "any"      every address that is a multiple of the element size works and gives the same bits as an aligned one (the pointer
 *                  is read or written one element at a time, or the kernel has a narrower path for it).  The three gradient-norm
 *                  reductions (tad_sumsq_f32, tad_grad_norm_coef, tad_grad_segnorm) peel the head of x up to a 16-byte boundary: their
 *                  result is the same sum taken in another order.
 *   - Host arrays (mean3 / std3, group_lr ..., every *_host table) and handles (tad_comm_t, RCCL ids and buffers, debug buffers) are
 *     outside the rule.
 *   - The _f16 twins owe what their bf16 entry points owe.  tests/alignment_contract.py holds the whole contract as a table.
 */
#ifndef TAD_MI355X_H
#define TAD_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAD_ABI_VERSION 5

enum tad_status {
  TAD_OK = 0,
  TAD_EINVAL = -1,   /* bad argument / unsupported shape */
  TAD_ELAUNCH = -2,  /* hipLaunch / runtime error         */
  TAD_ENOSPACE = -3  /* workspace too small               */
};

/* Element types.  TAD_BF16 / TAD_F16 name the 16-bit OPERAND FORMAT of a call: the entry points below take bfloat16 operands and accept
 * TAD_F32 or TAD_BF16 where an output type is selectable; their IEEE-half twins (tad_*_f16, end of this header) take half operands
 * and accept TAD_F32 or TAD_F16. */
enum tad_dtype { TAD_F32 = 0, TAD_BF16 = 1, TAD_F16 = 2 };

/* Linear-layer epilogues (tad_linear_fwd). */
enum tad_epilogue {
  TAD_EPI_BIAS = 0,          /* y = x W^T + b                                  (F.linear)            */
  TAD_EPI_BIAS_GELU = 1,     /* y = gelu_erf(x W^T + b); optional pre-activation copy (Mlp.fc1+act)  */
  TAD_EPI_BIAS_RESIDUAL = 2  /* y = res + rowscale[m/rows_per_scale] * gamma[n] * (x W^T + b)       */
};

typedef void* tad_stream_t;

int tad_abi_version(void);
const char* tad_last_error_string(void);

/* ---- weight preparation -------------------------------------------------------------
 * fp32 master weights stay owned by the caller (torch nn.Parameter); the kernels consume
 * bf16 copies: W [N,K] for forward, W^T [K,N] for the input-gradient GEMM. */
int tad_cast_f32_bf16(const float* src, uint16_t* dst, int64_t n, tad_stream_t stream);
/* Alignment: src, dst: any. */
int tad_transpose_cast_f32_bf16(const float* src /*[R,C]*/, uint16_t* dst /*[C,R]*/, int R, int C,
                                tad_stream_t stream);

/* ---- PatchEmbed: nn.Conv3d(3,D,k=s=(tub,p,p)) + flatten(2).transpose(1,2)
 *      (modeling_finetune.py:181-183,190) fused with "+ pos_embed" (:312-313).
 * x [B,C,T,H,W] f32 contiguous.  cols [B*N, C*tub*p*p] bf16 is the tubelet patch matrix
 * (token n = t'*H'*W' + h'*W' + w', k = ((c*tub+kt)*p+kh)*p+kw) -- kept for backward.
 * w_bf16 [D,K], bias [D] f32 (nullable), pos [N,D] f32 (nullable), out [B*N,D] f32. */
/* Row stride (elements) of the patch matrix and of the bf16 weight the patch-embed GEMM reads: K = C*tubelet*patch^2 rounded up to
 * the GEMM's K-tile of 64.  Equal to K for patch sizes that are multiples of 8 (/16: 1536); for even patch sizes that are not
 * (ViT-L/14: K = 1176 -> 1216) tad_im2col_tubelets writes rows of that stride with zeros in the padding columns and the caller
 * passes a zero-padded weight [D, ldk] -- the product is the un-padded one exactly, and /14 is a pure configuration change. */
int tad_patch_embed_ldk(int C, int tubelet, int patch);
/* Alignment: patch sizes that are not multiples of 8 move pairs: x 8 bytes, cols 4 bytes (tad_im2col_tubelets_f32: cols 8 bytes); so does x of
 * tad_patch_embed_fwd (its cols stay at 16 bytes: the GEMM reads them). */
int tad_im2col_tubelets(const float* x, uint16_t* cols, int B, int C, int T, int H, int W, int tubelet,
                        int patch, tad_stream_t stream);
int tad_patch_embed_fwd(const float* x, const uint16_t* w_bf16, const float* bias, const float* pos,
                        float* out, uint16_t* cols, int B, int C, int T, int H, int W, int tubelet,
                        int patch, int D, tad_stream_t stream);
/* The same patch matrix from a clip that already is in the 16-bit operand format (a loader that ships bf16 / half clips): x [B,C,T,H,W]
 * 16-bit contiguous -> cols [B*N, tad_patch_embed_ldk(C, tubelet, patch)], word (b, c, t, h, w) at row n = ((b T' + t') H' + h') W' + w',
 * column k = ((c*tub+kt)*p+kh)*p+kw, padding columns zero.  A MOVE of 16-bit words: no cast, every bit pattern (NaN payloads, subnormals)
 * arrives unchanged, so one entry point serves both formats (there is no _f16 twin) and cols is bit-identical to tad_im2col_tubelets(_f16)
 * on the upcast clip.  Patch sizes that are multiples of 8 move 16-byte chunks: x and cols 16-byte aligned; other even sizes move 4-byte
 * words: x and cols 4-byte aligned (TAD_EINVAL otherwise). */
int tad_im2col_tubelets_16(const uint16_t* x, uint16_t* cols, int B, int C, int T, int H, int W, int tubelet, int patch,
                           tad_stream_t stream);
/* The same forward as an IMPLICIT GEMM: the x operand is read straight from the f32 clip (register-staged, rounded to the
 * operand format as tad_im2col_tubelets rounds it), no patch matrix is written -- for forwards that keep nothing for a backward pass (eval,
 * no_grad, inference); the training step uses tad_patch_embed_fwd, whose patch matrix the weight gradient reads again.  Bit-identical to
 * tad_patch_embed_fwd.  patch must be 16 (TAD_EINVAL otherwise: callers fall back to the explicit form); clip and weight < 2 GiB each. */
int tad_patch_embed_fwd_implicit(const float* x, const uint16_t* w_bf16, const float* bias, const float* pos,
                                 float* out, int B, int C, int T, int H, int W, int tubelet, int patch, int D,
                                 tad_stream_t stream);
/* Input stage: the same patch matrix straight from uint8 frames [B,T,H,W,3] (decoder / cv2 layout) with the
 * reference's normalisation v = (u8/255 - mean[c]) / std[c] in f32 (run_inference.py:15-34 prepare_image; dota.py:443-460
 * tensor_normalize) -- bit-identical to tad_im2col_tubelets on the normalised f32 clip.  mean3 / std3: HOST arrays in RGB order;
 * bgr != 0: channel c is stored at position 2-c (cv2 frames, replaces cv2.cvtColor(BGR2RGB)); t_offset: frame t of the clip is
 * slot (t + t_offset) % T of the buffer (ring buffer for the sliding window of run_inference.py:86-93).  Any even patch size: rows have
 * the stride tad_patch_embed_ldk(3, tubelet, patch) (= K for multiples of 8; /14: 1216, padding columns zeroed). */
/* Alignment: frames: 4 bytes. */
int tad_im2col_tubelets_u8(const uint8_t* frames, uint16_t* cols, int B, int T, int H, int W, int tubelet, int patch,
                           const float* mean3, const float* std3, int bgr, int t_offset, tad_stream_t stream);
/* Patch matrix of B windows read from ONE frame store [F,H,W,3] uint8: frame t of window b is slot idx[b*T+t].
 * Same arithmetic, row order, row stride (tad_patch_embed_ldk) and padding columns as tad_im2col_tubelets_u8
 * on the clip store[idx] -- bit-identical to it.
 * cols_dtype: TAD_BF16 or TAD_F16.  idx: DEVICE int32.  mean3/std3: HOST, RGB order.
 * One entry point for both operand formats (the format is an argument: there is no _f16 twin).  store and idx must be 4-byte aligned,
 * cols 16-byte aligned.  The index table is on the device, so this call cannot check it: the CALLER guarantees 0 <= idx < F.  As a
 * defence the kernels clamp every slot into [0, F-1]: an index outside the store reads the first / last frame instead of memory outside
 * the store -- a wrong result, never a wild address.  Do not rely on the clamp as padding. */
/* Alignment: store: 4 bytes; idx: any. */
int tad_im2col_frame_windows(const uint8_t* store, int64_t F, const int32_t* idx, void* cols, int cols_dtype,
                             int B, int T, int H, int W, int tubelet, int patch,
                             const float* mean3, const float* std3, int bgr, tad_stream_t stream);
/* GEMM part of tad_patch_embed_fwd on an existing patch matrix: out = cols * w^T + bias (+ pos broadcast over the batch) */
int tad_patch_embed_gemm(const uint16_t* cols, const uint16_t* w_bf16, const float* bias, const float* pos, float* out,
                         int64_t M, int ntok, int D, int K, tad_stream_t stream);
/* dW [D,K] f32 (overwritten), db [D] f32 (overwritten, nullable) from dy [B*N,D] bf16 and cols. */
size_t tad_patch_embed_bwd_workspace_bytes(int64_t M, int D, int K);
int tad_patch_embed_bwd(const uint16_t* dy_bf16, const uint16_t* cols, float* dW, float* db, void* ws,
                        size_t ws_bytes, int64_t M, int D, int K, tad_stream_t stream);

/* ---- nn.LayerNorm(D, eps) (modeling_finetune.py:143,149,270; eps=1e-6 at :342) -------
 * x [rows,D] f32; y [rows,D] in y_dtype; mean/rstd [rows] f32 saved for backward (nullable). */
/* Alignment: a 16-bit y: 8 bytes; mean, rstd: any. */
int tad_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_dtype,
                      float* mean, float* rstd, int64_t rows, int D, float eps, tad_stream_t stream);
/* dx = (dres ? dres : 0) + LN'(dy).  Optional outputs: dx_bf16 (copy of dx), colsum_dx [D]
 * (sum over rows of dx: the bias gradient of the Linear that produced x's residual branch).
 * rowscale (nullable, [ceil(rows / rows_per_scale)]): dx_bf16 and colsum_dx are taken of rowscale[row / rows_per_scale] * dx --
 * the gradient entering a residual branch whose output was scaled per sample (DropPath, modeling_finetune.py:23-34, 159-163).
 * accumulate != 0: dgamma, dbeta and colsum_dx are added to (gradient accumulation in place), else overwritten.
 * ws: tad_layernorm_bwd_workspace_bytes(rows, D). */
size_t tad_layernorm_bwd_workspace_bytes(int64_t rows, int D);
/* Alignment: a 16-bit dy and dx_bf16: 8 bytes; mean, rstd, rowscale: any. */
int tad_layernorm_bwd(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean,
                      const float* rstd, const float* dres, float* dx, uint16_t* dx_bf16, float* dgamma,
                      float* dbeta, float* colsum_dx, const float* rowscale, int rows_per_scale, int accumulate,
                      void* ws, size_t ws_bytes, int64_t rows, int D, tad_stream_t stream);

/* ---- Linear: F.linear(x, W, b) with fused epilogues ---------------------------------
 * replaces qkv (modeling_finetune.py:88-92), proj (:104), fc1+GELU (:48-49), fc2 (:52) and the
 * residual adds of Block.forward (:161-162, incl. gamma_1/2 and per-sample drop-path scale).
 * x [M,K] bf16, w [N,K] bf16, bias [N] f32 (nullable), y [M,N] y_dtype.
 * preact [M,N] bf16 (nullable): x W^T + b before GELU (saved for backward).
 * residual [M,N] f32, gamma [N] f32 (nullable), rowscale f32 [ceil(M/rows_per_scale)] (nullable). */
/* ws (nullable; tad_linear_workspace_bytes(M, N, K) bytes, private to the call's stream until the launches have run): scratch for the
 * split-K form of an under-filled last round of tiles -- a Linear whose 256 x 256 tiles do not fill whole rounds of one workgroup per
 * CU may run its last tiles as several shares of their K-tiles each, whose f32 partial tiles travel through this buffer.  Two plans:
 * the default (tad_linear_tuning("splitk_defer", 1)) is THREE launches -- partial tiles, the whole rounds, combine + epilogue -- ordered
 * by kernel boundaries, with no residency requirement: safe beside other kernels (an overlapped RCCL exchange, side streams).  The
 * in-launch combine ("splitk_defer", 0; experiments) waits for the other shares of a tile inside ONE launch and needs its whole grid
 * resident at once: if a share never arrives the kernel gives up, flags it in host-visible memory, and the NEXT tad_linear_* call on
 * the process returns TAD_ELAUNCH (the output of the affected Linear is invalid).  Results differ from the ws == NULL plan only in the
 * summation order over K.  tad_linear_workspace_bytes returns 0 for shapes whose plan never splits along K under the current
 * tad_linear_tuning knobs (every Linear of ViT-B by default; ViT-L's fc2 / dX(fc1) tails: 16 tiles x 8 shares = 33.5 MB). */
size_t tad_linear_workspace_bytes(int64_t M, int N, int K);
/* Alignment: gamma, rowscale: any (read one float at a time; bias is read as float4). */
int tad_linear_fwd(const uint16_t* x, const uint16_t* w, const float* bias, void* y, int y_dtype,
                   int epilogue, uint16_t* preact, const float* residual, const float* gamma,
                   const float* rowscale, int rows_per_scale, void* ws, size_t ws_bytes, int64_t M, int N, int K,
                   tad_stream_t stream);
/* Input gradient: dx [M,K] = (dy [M,N] @ W)  using wT [K,N] bf16.
 * If gelu_preact [M,K] is given, dx *= gelu'(preact) (backward through the GELU that fed this Linear).
 * colscale [N] / rowscale are applied to dy on the fly is NOT supported; scale dy beforehand. */
int tad_linear_bwd_input(const uint16_t* dy, const uint16_t* wT, void* dx, int dx_dtype,
                         const uint16_t* gelu_preact, void* ws, size_t ws_bytes, int64_t M, int N, int K, tad_stream_t stream);
/* The qkv Linear of Attention (modeling_finetune.py:64-76, 89-92): bias = cat(q_bias, zeros, v_bias) without materialising it.
 * N = 3 * all_head_dim; q_bias / v_bias [N/3] f32 (both or neither).  Forward: y = x W^T + bias.  Weight gradient: as
 * tad_linear_bwd_weight, with the column sums of the first / last third of dy going to dq_bias / dv_bias (workspace: the same
 * tad_linear_bwd_weight_workspace_bytes). */
/* q_prescale (> 0; 1 = the plain Linear): the q third of y (columns [0, N/3)) is multiplied by it before the one rounding to
 * y_dtype.  With q_prescale = scale * log2(e) the attention kernels (q_prescaled != 0 below) get their scores from the matrix pipe
 * in log2 units and spend no vector instruction on the softmax scale (modeling_finetune.py:96: `q = q * self.scale`, done here). */
int tad_linear_fwd_qkv(const uint16_t* x, const uint16_t* w, const float* q_bias, const float* v_bias, void* y,
                       int y_dtype, float q_prescale, int64_t M, int N, int K, tad_stream_t stream);
int tad_linear_bwd_weight_qkv(const uint16_t* dy, const uint16_t* x, float* dW, float* dq_bias, float* dv_bias,
                              int accumulate, void* ws, size_t ws_bytes, int64_t M, int N, int K,
                              tad_stream_t stream);
/* TWO weight gradients over the same M rows with the same K in one call -- the qkv and proj Linears of a Block (modeling_finetune.py:89-92,
 * 104): dW1 [N1, K] (+)= dy1^T x1 with its bias column sums (db1 [N1], or -- db1b != NULL -- the first / last third of them to db1 / db1b
 * [N1/3] as in tad_linear_bwd_weight_qkv; db1 NULL: none), dW2 [N2, K] (+)= dy2^T x2 (no bias sums).  When N1 is a multiple of 256 and K
 * runs on the 256-wide tiles both run as ONE kernel launch (a small problem alone pays for filling the chip with many reduction shares:
 * ViT-B's proj gradient is 9 tiles x 28 shares; the pair is 36 tiles x 7), otherwise as two; tad_linear_tuning("tn_pair", 0) forces two.
 * ws: at least the largest of tad_linear_bwd_weight_workspace_bytes(M, N1, K), (M, N2, K) and (M, N1 + N2, K).  The sums over the M rows
 * are taken in another order than the single calls take them (a different share count), deterministic for a given shape. */
int tad_linear_bwd_weight_pair(const uint16_t* dy1, const uint16_t* x1, float* dW1, float* db1, float* db1b, int N1,
                               const uint16_t* dy2, const uint16_t* x2, float* dW2, int N2, int accumulate, void* ws,
                               size_t ws_bytes, int64_t M, int K, tad_stream_t stream);
/* Scheduling knobs of the Linear GEMMs (process-wide; results never depend on them, only timing): tad_linear_tuning(key, value).
 *   "persistent"      1 = one workgroup per CU walks the tile list (default), 0 = one workgroup per tile
 *   "direct_epilogue" 2 = epilogue on the accumulator registers, stores straight from the MFMA layout; 0 = accumulators
 *                     transposed through the LDS first (whole rows per store instruction); 1 = per epilogue kind (default)
 *   "split_tail"      1 = a Linear whose 256 x 256 tiles do not fill whole rounds of one workgroup per CU may run as two
 *                     launches (whole rounds + remaining rows) when the cost model says so (default); 0 = never; 2 = always
 *   "splitk_tail"     1 = with a workspace, the second of those launches may split its tiles along K (default); 0 = never;
 *                     2 = whenever eligible (this one changes the summation order over K of the rows it covers)
 *   "splitk_defer"    1 = a split-K tail runs as three launches -- its partial tiles, the whole rounds, its combine + epilogue -- so
 *                     that the partial tiles travel through memory beside the whole rounds (default); 0 = one launch that combines inside
 *   "variant"         0 = tile configuration planned per shape (default); 1 / 3 / 2 / 4 / 5 = 256 x 256, 256 x 128, 128 x 128, 128 x 64,
 *                     64 x 64 tiles for every launch; 7 = the four-wave 256 x 256 kernels (128 x 128 outputs per wave, one wave per SIMD;
 *                     csrc/gemm_w4.hip); 8 / 9 = 192 x 128 as eight / four waves -- all bit-identical
 *   "short_k"         1 = Linears with K <= 512, whose epilogue is as long as their K loop, run on tiles that put two workgroups on a CU so
 *                     that one's epilogue runs beside the other's K loop: 192 x 128 as four waves (variant 9) for the GELU / GELU' Linears and,
 *                     at K < 512, the bias-only ones; 128 x 128 for the residual ones at K < 512 (default: the MAE decoder's fc1 / dX(fc2) -11 %,
 *                     ViT-S 2-12 % per shape); 0 = planned as the rest
 *   "tail_192"        1 = the second launch of the split plan may use 192 x 128 tiles where they put more CUs to work than 256 x 128
 *                     (default: ViT-B's 6656-row tails run 210 workgroups instead of 156, 9 % faster); 0 = 256 x 128 / 256 x 256 only
 *   "w4_plain"        K_min > 0: Linears whose reduction is at least K_min long run their whole rounds of 256 x 256 tiles on the
 *                     four-wave kernel (default 640: bit-identical, 5-8 % faster on the input-gradient Linears of ViT-B / L; at K = 384 / 512
 *                     its slower epilogue costs what its K loop gains); 0 = eight waves.  Applies to bias-only epilogues and to those of
 *   "w4_epilogues"    bit mask of the other epilogues whose whole rounds take the four-wave kernel: bit 1 GELU, 2 residual with f32 output
 *                     (default: 4), 3 GELU backward
 *   "tn_pair"         1 = tad_linear_bwd_weight_pair runs its two problems as one launch when they fit (default); 0 = always two launches
 *   "tn_w4"           1 = the 256 x 256 weight-gradient GEMM runs as four waves of 128 x 128 outputs (default; bit-identical, 8 % faster);
 *                     0 = eight waves of 128 x 64
 *   "tn_pdeep"        1 = the weight-gradient GEMM requests its dy operand two reduction tiles ahead (three-slot ring, the whole
 *                     160 KiB of LDS); 0 = two-stage ring (default: measured equal) */
int tad_linear_tuning(const char* key, int value);
/* Current value of a tad_linear_tuning knob (what a scoped change has to put back: simple_tad_amd.kernels.TuningScope). */
int tad_linear_tuning_get(const char* key, int* value);
/* What a Linear problem WOULD run as under the current knobs -- the launch plan the entry points above execute, as data.  Launches nothing
 * and needs no device (without one the plan is made for 256 CUs, the MI355X's count): plans can be inspected, compared and tested on a
 * build machine (simple_tad_amd.kernels.linear_plan; tests/test_linear_plan_cpu.py).  The problem is y [M,N] = x [M,K] w^T in the GEMM's own
 * terms (tad_linear_bwd_input(M, N, K) is the problem (M, K, N)) with
 *   epilogue        0 bias only, 1 bias + GELU, 2 bias + residual, 3 GELU backward (tad_linear_bwd_input with gelu_preact)
 *   out_16bit       the output has the 16-bit operand format (else f32)
 *   has_residual, res_mod         a residual operand is given; res_mod > 0: its row is taken modulo res_mod (tad_patch_embed_gemm's ntok)
 *   has_rowscale, rows_per_scale  as tad_linear_fwd's;  colscale_cols: N / 3 for tad_linear_fwd_qkv with q_prescale != 1, else 0
 *   ws_bytes        the split-K workspace on offer (0: none)
 * Writes one row of TAD_LINEAR_PLAN_STEP_WORDS int32 per kernel launch, in launch order, and returns their number (> 0), TAD_ENOSPACE when
 * there are more than `capacity` rows, or the error the entry point would refuse the shape with.  A row is
 *   r0, rows        the rows of the problem the launch covers (taller problems than 32-bit operand offsets allow run as row ranges)
 *   kernel          the tile configuration of tad_linear_tuning("variant") that is launched (1 2 3 4 5 7 8 9), or 10 = the split-K kernel
 *   persistent, direct, grid, block, group_m    one workgroup per CU walks the tiles | stores straight from the MFMA layout | launch geometry | raster
 *   sk_splits, sk_mode   split-K launches: shares per tile; 0 combine in the launch, 1 leave the partial tiles, 2 combine what a mode-1 launch left
 *   epilogue        the epilogue instantiation: as above, or 4 = residual modulo res_mod */
#define TAD_LINEAR_PLAN_STEP_WORDS 11
int tad_linear_plan(int64_t M, int N, int K, int epilogue, int out_16bit, int has_residual, int res_mod, int has_rowscale,
                    int rows_per_scale, int colscale_cols, size_t ws_bytes, int32_t* steps, int capacity);
/* The same for the weight gradients: tad_linear_bwd_weight(M, N1, K) with N2 == 0, tad_linear_bwd_weight_pair(M, N1, N2, K) otherwise, given a
 * workspace of ws_bytes.  One row of TAD_LINEAR_BWD_WEIGHT_PLAN_WORDS int32 per GEMM launch (a pair is ONE row when it fits one launch, else two):
 *   N, tile_k       output rows of the launch (N1 + N2 for a pair launch); tile width along K (256 or 128)
 *   tiles, tiles_k, splits, rows_per_split, kernel, grid, block    kernel: 0 four waves 256 x 256, 1 eight waves with the deep P ring ("tn_pdeep"),
 *                   2 eight waves 256 x 256, 3 256 x 128
 *   pair            1 = this launch computes both gradients
 *   ws_lo, ws_hi    workspace the launch needs: ws_hi * 2^31 + ws_lo bytes (= tad_linear_bwd_weight_workspace_bytes(M, N, K)) */
#define TAD_LINEAR_BWD_WEIGHT_PLAN_WORDS 12
int tad_linear_bwd_weight_plan(int64_t M, int N1, int N2, int K, size_t ws_bytes, int32_t* launches, int capacity);
/* Number of gemm_nt kernel launches issued so far by tad_linear_fwd* / tad_linear_bwd_input / tad_patch_embed_* (a call is one
 * launch, or two when the split-tail plan is taken): lets a profiler attribute event time to kernel launches. */
long long tad_linear_kernel_launches(void);
/* Debug timeline of the Linear GEMM kernels: while buf (device memory, >= gridDim * 64 * 32 * 8 bytes, caller-owned) is set,
 * every workgroup records s_memrealtime (100 MHz) for each of its first 64 tiles: slot 0 tile start, 1 K-loop end, 2 epilogue
 * issued, 3 stores acknowledged, 4 + 2q / 5 + 2q epilogue chunk q transposed / stored.  NULL switches it off (default).  Costs a store drain per tile: never leave it on.  Only libraries built with
 * -DTAD_GEMM_ABLATION (TAD_BUILD_ABLATION=1) carry the stamps; others return TAD_EINVAL for a non-NULL buffer. */
int tad_linear_debug_stamps(void* buf);
/* Weight gradient: dW [N,K] f32 = dy^T [N,M] @ x [M,K]; db [N] f32 = column sums of dy (nullable).
 * Outputs are overwritten (accumulate==0) or added to (accumulate!=0). */
size_t tad_linear_bwd_weight_workspace_bytes(int64_t M, int N, int K);
int tad_linear_bwd_weight(const uint16_t* dy, const uint16_t* x, float* dW, float* db, int accumulate,
                          void* ws, size_t ws_bytes, int64_t M, int N, int K, tad_stream_t stream);

/* ---- Space-time attention: softmax(q k^T * scale) v, non-causal, no mask --------------
 * replaces Attention._naive_attn's q@k^T/softmax/attn@v (modeling_finetune.py:96-103) and
 * FlashAttention.forward -> flash_attn_varlen_qkvpacked_func (flash_attention_class.py:47-50)
 * with equal-length sequences (cu_seqlens = arange(0,(B+1)N,N)).
 * qkv [B,N,3,H,d] bf16 packed (the qkv Linear's output, column order [3][H][d]); d = 64 or 80 (the `d` argument).
 * out [B,N,H,d] in out_dtype; lse [B,H,N] f32 = log(sum_j exp(scale * q.k_j)) (natural log).
 * out_lo (nullable, 16-bit outputs only): [B,N,H,d] = what the rounding of out dropped (out + out_lo carries 16 / 22 significant
 * bits), for tad_attn_bwd's delta.
 * q_prescaled != 0: the q third of qkv already carries the factor scale * log2(e) (tad_linear_fwd_qkv's q_prescale); `scale` is
 * still the softmax scale.  0: plain q, as flash_attn_varlen_qkvpacked_func takes it (the kernels then scale their Q fragments
 * themselves: on the f32 scores).
 * dropout_p in [0, 1), seed: attention dropout (nn.Dropout on the softmax matrix, modeling_finetune.py:99-101; dropout_p of
 * flash_attn_varlen_qkvpacked_func, flash_attention_class.py:56-61): element (b, h, query, key) is kept iff
 * hash((b H + h) N + query, key, seed) >= dropout_p * 2^32 (csrc/common.h: drop_keep; oracle/vit_oracle.py:
 * attention_dropout_keep regenerates the mask) and kept probabilities are scaled by 1 / (1 - dropout_p); lse is that of the full
 * softmax.  tad_attn_bwd must be given the same dropout_p and seed.  0 = no dropout (evaluation).
 * clip_scale (nullable; tad_attn_fwd and tad_attn_bwd, either operand type): stochastic depth (DropPath around the attention branch,
 * modeling_finetune.py:159-163).  [B] f32 in device memory, ONE scale per clip (mask / keep_prob): the scale by which the residual epilogue
 * behind the attention multiplies the branch -- the rowscale of tad_linear_fwd's TAD_EPI_BIAS_RESIDUAL with rows_per_scale = N.  A clip whose
 * scale is exactly 0 reaches the result neither forward (0 x branch) nor backward (its dout rows are exact zeros), so the kernels do not
 * compute it: the forward writes zeros to its rows of out / out_lo and a finite placeholder to lse, the backward zeros to its rows of dqkv --
 * what the computation would have stored there in the backward's case, and values that only ever meet a zero factor in the forward's.  The
 * scale is read on the device (no host copy, no synchronisation).  head_dim 64 with pre-scaled q, 16-bit output and no attention dropout
 * takes the path; every other contract, and every call without a clip_scale, computes all clips (which kernel a call takes: tad_attn_plan). */
/* Alignment: lse, clip_scale: any. */
int tad_attn_fwd(const uint16_t* qkv, void* out, int out_dtype, uint16_t* out_lo, float* lse, const float* clip_scale, int B, int N, int H,
                 int d, float scale, int q_prescaled, float dropout_p, uint32_t seed, tad_stream_t stream);
/* dqkv [B,N,3,H,d] bf16 (fully overwritten).  delta: scratch of tad_attn_bwd_scratch_bytes(B, N, H) bytes = 2*B*H*N floats (the
 * first kernel leaves -rowsum(dout*out) in [0, BHN) and -lse/scale (-lse*log2(e) with q_prescaled) in [BHN, 2 BHN) for the second
 * one, which takes them as the initial values of its accumulators).  The q slot of dqkv is the gradient of the PLAIN q in either case. */
/* Knobs of the three attention kernels (one table, csrc/attn_plan.hip; the environment variable gives the initial value):
 *   "dma_mode"   TAD_ATTN_DMA_MODE   0 = production; 2 / 3 = timing-only ablations (wrong results) that only ablation builds
 *                                    (TAD_BUILD_ABLATION=1) accept
 *   "fwd_q64"    TAD_ATTN_FWD_Q64    1 = the forward of the production contract runs with 64 query rows per wave (experiment, bit-identical);
 *                                    0 (default)
 *   "drop_skip"  TAD_DROP_SKIP       1 (default) = calls with a clip_scale fill the clips it marks as dropped instead of computing them;
 *                                    0 = they compute every clip (A/B runs; every result the training step consumes is bit-identical either way) */
int tad_attn_tuning(const char* key, int value);
/* Current value of a tad_attn_tuning knob (what a temporary change has to put back). */
int tad_attn_tuning_get(const char* key, int* value);
/* Which kernels a tad_attn_fwd (backward == 0) or tad_attn_bwd call WOULD launch under the current knobs -- the records the entry points
 * execute, as data; both operand formats select alike.  Launches nothing and needs no device (simple_tad_amd.kernels.attn_plan;
 * tests/test_attn_plan_cpu.py).  out_16bit: the forward's output has the 16-bit operand format (else f32); has_clip_scale / has_out_lo: the
 * nullable operand is given (the backward ignores out_16bit and has_out_lo).  The rule:
 *   forward   with "fwd_q64" on, head_dim 64 + pre-scaled q + no dropout + 16-bit output runs the 64-row kernel, whether or not there is a
 *             clip scale; else a call with a clip scale, "drop_skip" on, "dma_mode" 0 and that same contract runs the general kernel with
 *             SKIP (it fills dropped clips); every other call runs the general kernel for its (d, output type, q_prescaled, dropout > 0),
 *             which never looks at a clip scale
 *   backward  two launches, dQ then dK/dV, with the same arguments: SKIP under the forward's conditions except the output type, else general
 * Writes one row of TAD_ATTN_PLAN_WORDS int32 per launch and returns their number (1 or 2), TAD_ENOSPACE when `capacity` is smaller, or the
 * error the entry point would refuse the shape with.  A row is
 *   kernel          0 attn_fwd_kernel, 1 attn_fwd_q64_kernel, 2 attn_bwd_dq_kernel, 3 attn_bwd_dkv_kernel
 *   hd, out16, qs, drop, dma_mode, skip    the template arguments HD, OUT_BF16 (backward: 1), QS, DROP, DMA_MODE, SKIP
 *   has_lo          HAS_LO of the 64-row kernel (0 elsewhere)
 *   grid, block     ceil(N / 128) * H * B workgroups of 256 threads (128 for the 64-row kernel) */
#define TAD_ATTN_PLAN_WORDS 10
int tad_attn_plan(int backward, int B, int N, int H, int d, int out_16bit, int q_prescaled, float dropout_p, int has_clip_scale,
                  int has_out_lo, int32_t* launches, int capacity);
size_t tad_attn_bwd_scratch_bytes(int B, int N, int H);
/* Diagnostic, ablation builds only (see tad_linear_debug_stamps): while buf (device memory, 32 bytes per workgroup of the dK/dV grid
 * = ceil(N/128)*H*B workgroups) is set, every dK/dV workgroup records {s_memrealtime, s_memtime} at the start and at the end of its
 * tile loop: (d memtime / d memrealtime) x 100 MHz = the clock held inside the loop.  NULL switches it off. */
int tad_attn_debug_stamps(void* buf);
/* out_lo (nullable): the forward's rounding residual; with it delta = rowsum(dout * (out + out_lo)), i.e. of the unrounded output, which
 * is what cancels against the dP the kernels recompute (without it the q / k gradients of near-uniform attention rows carry the
 * rounding of out amplified by |delta| / |dP - delta|). */
/* Alignment: lse, clip_scale, delta: any. */
int tad_attn_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* out_lo, const uint16_t* dout, const float* lse,
                 const float* clip_scale, uint16_t* dqkv, float* delta, int B, int N, int H, int d, float scale, int q_prescaled,
                 float dropout_p, uint32_t seed, tad_stream_t stream);
/* Weighted column sum of the softmax matrix, recomputed from qkv and lse with no N x N tensor (csrc/attn_colsum.hip):
 *   out[b,h,j] = sum_{i<N} w[b,i] * exp(scale * q_{b,h,i} . k_{b,h,j} - lse[b,h,i])
 * -- one step of attention rollout when only a row vector is propagated (simple_tad_amd/explain.py); w = 1/N gives the attention each
 * token receives, a one-hot w one row of P.  qkv [B,N,3,H,d], d = 64 or 80, and q_prescaled exactly as tad_attn_fwd takes them (the v
 * third is not read).  One entry point for both operand formats: op_dtype is TAD_BF16 or TAD_F16 (there is no _f16 twin).
 * lse [B,H,N] f32 is used AS HANDED (tad_attn_fwd's, natural log); it is not recomputed.  w [B,N] f32, any sign.  out [B,H,N] f32, fully
 * overwritten.  P and the sums stay f32 (no 16-bit rounding of P); fixed summation order, no atomics: bit-reproducible.  A clip is computed
 * from its own rows of qkv, lse and w alone: nothing behind them is read, and a non-finite value in another clip cannot reach it.
 * TAD_EINVAL: null pointer, d not 64 / 80, unknown op_dtype, B, N or H < 1, scale <= 0, qkv of 4 GiB or more. */
/* Alignment: lse, w, out: any. */
int tad_attn_colsum(const uint16_t* qkv, int op_dtype, const float* lse, const float* w, float* out, int B, int N, int H, int d,
                    float scale, int q_prescaled, tad_stream_t stream);

/* ---- token mean-pool x.mean(1) (modeling_finetune.py:325-326) -------------------------
 * x [B,N,D] f32 -> y [B,D] f32.  ws: B*TAD_POOL_SPLIT*D floats. */
#define TAD_POOL_SPLIT 8
/* Alignment: y: any. */
int tad_meanpool_fwd(const float* x, float* y, float* ws, int B, int N, int D, tad_stream_t stream);
/* dx[b,n,:] = dy[b,:]/N  (f32, plus optional bf16 copy) */
/* Alignment: dx_bf16: 8 bytes. */
int tad_meanpool_bwd(const float* dy, float* dx, uint16_t* dx_bf16, int B, int N, int D,
                     tad_stream_t stream);

/* ---- pooled tail: the last block when only the token mean of its output is read (csrc/pooled_tail.hip) ----
 * x2 = x1 + dp2 (a W2^T + b2) is linear in a, so mean_n(x2) needs only the per-clip column sums of a, and every token of a clip
 * receives the same gradient dy[b]/N: one accumulator row t[b] = gb[b] W2 per clip serves all N rows of the fc2 input gradient.
 * One entry point each for both operand formats: op_dtype is TAD_BF16 or TAD_F16 (there is no _f16 twin).
 *
 * S[b,:] = sum_{n<N} a[b*N+n,:]: a [B*N,K] 16-bit, S [B,K] f32.  f32 accumulation in a fixed order (two stages, no atomics).
 * ws: B*TAD_POOL_SPLIT*K floats (ws_bytes is checked: TAD_ENOSPACE).  K % 8 == 0 and a, S, ws 16-byte aligned, else TAD_EINVAL:
 * callers fall back to the general path. */
int tad_colsum_segments(const uint16_t* a, int op_dtype, float* S, void* ws, size_t ws_bytes, int B, int N, int K,
                        tad_stream_t stream);
/* The pooled fc2: out[b,:] = xbar[b,:] + rowscale[b] ((S[b,:] W^T) / N + bias).  S [B,K] f32 (tad_colsum_segments), w [D,K] 16-bit,
 * bias [D] (nullable), rowscale [B] (nullable), xbar and out [B,D] f32 (out must not alias xbar).  The B*D dot products run on the
 * f32 sums (the pooled operand is not rounded to 16 bits) with f64 accumulation and one rounding to f32 at the end.
 * K % 8 == 0 and S, w 16-byte aligned, else TAD_EINVAL. */
/* Alignment: bias, rowscale, xbar, out: any. */
int tad_pooled_linear(const float* S, const uint16_t* w, int op_dtype, const float* bias, const float* rowscale, const float* xbar,
                      float* out, int B, int N, int D, int K, tad_stream_t stream);
/* dh[b*N+n,:] = op16(t[b,:] * gelu'(h[b*N+n,:])): t [B,K] f32, h and dh [B*N,K] 16-bit.  The arithmetic and the rounding are those
 * of tad_linear_bwd_input's gelu_preact epilogue on an accumulator row t[b]: bit-identical to it.
 * K % 8 == 0 and t, h, dh 16-byte aligned, else TAD_EINVAL. */
int tad_gelu_grad_bcast(const float* t, const uint16_t* h, uint16_t* dh, int op_dtype, int B, int N, int K,
                        tad_stream_t stream);

/* ---- small helpers used by the training step ------------------------------------------
 * column sums of a bf16 [M,N] matrix into f32 [N] (bias gradients: q_bias/v_bias/fc1.bias). */
size_t tad_colsum_workspace_bytes(int64_t M, int N);
/* Column sums over a row window of an f32 [B, R, N] tensor: out[n] (+)= sum_b sum_{r0 <= r < r0 + rc} a[b, r, n] (workspace:
 * tad_colsum_workspace_bytes(B * rc, N)).  The mask-token gradient of the MAE decoder input. */
int tad_colsum_window_f32(const float* a, float* out, int accumulate, void* ws, size_t ws_bytes, int B, int R, int N,
                          int r0, int rc, tad_stream_t stream);
int tad_colsum_bf16(const uint16_t* a, float* out, int accumulate, void* ws, size_t ws_bytes, int64_t M,
                    int N, tad_stream_t stream);
/* y_bf16 = bf16(rowscale[m/rows_per_scale] * gamma[n] * x_f32)  (backward of the residual-branch scale) */
/* Alignment: y: 8 bytes; rowscale: any. */
int tad_scale_cast_bf16(const float* x, uint16_t* y, const float* gamma, const float* rowscale,
                        int rows_per_scale, int64_t M, int N, tad_stream_t stream);

/* ---- fused Block variants: layer-scale (gamma_1 / gamma_2) and proj / MLP dropout (csrc/layerscale.hip) -------------------------------
 * A branch y = res + s[b] gamma[c] keep[m,c] / (1 - p) u with u = a W^T + bias (modeling_finetune.py:159-166: proj_drop / Mlp.drop, then
 * gamma, then drop path, then the residual add).  Its backward carries gamma in the WEIGHT operand: with gb = op16(s keep / (1 - p) g),
 *   d a = gb (diag(gamma) W),   T = gb^T a,  cs = colsum(gb)   (one tad_linear_bwd_weight),
 *   dW = gamma[n] T[n,:],   dbias = gamma cs,   dgamma[n] = sum_k T[n,k] W[n,k] + bias[n] cs[n]      -- u is never stored or recomputed.
 *
 * tad_rowscale_transpose_cast: w [N,K] f32, gamma [N] f32 -> out [K,N] 16-bit, out[k,n] = op16(fl32(gamma[n] w[n,k])) (the product rounded
 * to f32, then to the operand format, nearest even): the scaled twin of tad_transpose_cast_f32_bf16, the wT operand of tad_linear_bwd_input.
 * Any N, K > 0. */
/* Alignment: w, gamma, out: any. */
int tad_rowscale_transpose_cast(const float* w, const float* gamma, uint16_t* out, int N, int K, tad_stream_t stream);
/* tad_layerscale_grads: T, W [N,K] f32; bias (nullable), cs (nullable unless bias or dbias is given), gamma [N] f32.
 *   dW[n,k] (+)= fl32(gamma[n] T[n,k]);  dbias[n] (+)= fl32(gamma[n] cs[n]) (dbias nullable);  dgamma[n] (+)= sum_k T[n,k] W[n,k] + bias[n] cs[n].
 * accumulate = 0 writes, 1 adds to what dW / dbias / dgamma hold (gradient sinks).  One workgroup per row; the k reduction runs in a fixed
 * order without atomics: the same inputs give the same bits.  Any N, K > 0; 16-byte accesses when K % 4 == 0 and T, W, dW are 16-byte
 * aligned.  dW must not alias T or W. */
/* Alignment: every pointer: any (the element-wise path keeps the vector path's order of additions: dgamma has the same bits). */
int tad_layerscale_grads(const float* T, const float* W, const float* bias, const float* cs, const float* gamma, float* dW, float* dbias,
                         float* dgamma, int accumulate, int N, int K, tad_stream_t stream);
/* The dropout mask of a branch output [M,D]: element (m, c) is kept iff hash32(m, c, seed) >= p * 2^32 (csrc/common.h: Drop / drop_keep
 * with row = m, key = c -- the contract of attention dropout), kept values are scaled by inv_keep = 1.f / (1.f - p).  p in [0, 1); M < 2^32.
 * rowscale (nullable) f32 [ceil(M / rows_per_scale)]: the per-clip drop-path scale.
 * tad_branch_dropout_fwd:  out[m,c] = res[m,c] + u[m,c] * f,  f = fl32(gamma[c] * fl32(rowscale * inv_keep)) (gamma nullable: f = fl32(rowscale *
 *   inv_keep)), for kept elements of rows whose rowscale is not 0; every other element is res[m,c] bit for bit (a select, not a product with 0:
 *   a non-finite u does not leak, as in TAD_EPI_BIAS_RESIDUAL).  u comes from tad_linear_fwd with TAD_EPI_BIAS and f32 output.  out must
 *   not alias res or u.
 * tad_branch_dropout_cast: y[m,c] = op16(fl32(g[m,c] * fl32(rowscale * inv_keep))) for the same elements, +0 for every other one: the masked
 *   twin of tad_scale_cast_bf16 (no gamma: it is folded into the weights, see above).
 * Streaming, grid-stride; 16-byte accesses when D % 4 == 0 and the f32 tensors are 16-byte aligned (y: 8), element-wise otherwise. */
/* Alignment: every pointer of tad_branch_dropout_fwd and tad_branch_dropout_cast: any. */
int tad_branch_dropout_fwd(const float* u, const float* res, float* out, const float* gamma, const float* rowscale, int rows_per_scale,
                           float p, uint32_t seed, int64_t M, int D, tad_stream_t stream);
int tad_branch_dropout_cast(const float* g, uint16_t* y, const float* rowscale, int rows_per_scale, float p, uint32_t seed, int64_t M, int D,
                            tad_stream_t stream);

/* sum of squares of an f32 vector, accumulated into *out (f32, device) -- get_grad_norm_ (utils.py:415-427).  Deterministic: block
 * partials in ws (tad_sumsq_workspace_bytes()), added in a fixed order; no atomics. */
size_t tad_sumsq_workspace_bytes(void);
/* Alignment: x, out: any (see the general rule for the order of the sum); ws: 4 bytes. */
int tad_sumsq_f32(const float* x, int64_t n, float* out, void* ws, size_t ws_bytes, tad_stream_t stream);
/* NativeScalerWithGradNormCount's unscale + clip + overflow decision (utils.py:386-412: GradScaler.unscale_, clip_grad_norm_, the
 * "found inf" skip) as two launches on the flat gradient buffer, nothing read back by the host:
 *   out3[0] = ||x||_2 * inv_scale                                  (the gradient norm with the loss scale removed)
 *   out3[1] = inv_scale * min(1, max_norm / (out3[0] + 1e-6))       (max_norm <= 0: inv_scale) -- tad_adamw_step's grad_scale operand;
 *             0 when the norm is inf / NaN: the optimizer kernel then skips the step
 *   out3[2] = 1 when the norm is inf / NaN, else 0                  (read by the host one step late)
 * ws: tad_sumsq_workspace_bytes().  Deterministic (fixed order, no atomics). */
/* Alignment: x, out3: any; ws: 4 bytes. */
int tad_grad_norm_coef(const float* x, int64_t n, float inv_scale, float max_norm, float* out3, void* ws, size_t ws_bytes,
                       tad_stream_t stream);

/* Per-head gradient-norm diagnostics (utils.collect_grad_norms / collect_grad_norms_pretrain, utils.py:813-1011): the L2 norm of every
 * segment of the flat f32 gradient buffer, one segment per slot of the result tables, in two launches (reduce, finish) and without a
 * host synchronisation; the results accumulate on the device.
 *   table  nseg rows {offset, length, slot, first_work}: grad[offset, offset + length) belongs to `slot`; its work items are
 *          work[first_work .. first_work of the next row) (.. nwork for the last row)
 *   work   nwork rows {offset, length}: every segment cut, in order, into items of at most TAD_SEGNORM_WORK_MAX floats
 *   coef   device pointer to one f32, or NULL = 1.0 (tad_grad_norm_coef's out3 + 1: the unscale-and-clip coefficient)
 *   acc [nslots] f64, last [nslots] f32, counters int32 {steps_added, steps_skipped, nonfinite_values}
 * For every slot with a segment: last[slot] = coef * sqrt(sum x^2), acc[slot] += (double)last[slot], steps_added + 1.  *coef == 0 (the
 * loss scaler skipped the step on the device): every such last[slot] = 0, nothing is added, steps_skipped + 1.  A value that is inf or
 * NaN although *coef != 0 adds 0, leaves last[slot] = 0 and counts in nonfinite_values (the reference's nan_to_num keeps NaN -> 0; its
 * inf -> 1.8e308 is not reproduced).  A slot without a segment is never written.  Bit-identical from run to run: fixed summation order,
 * no floating-point atomics; 17 f32 additions at most between an element's square and the sum (csrc/grad_segnorm.hip, "depth").
 * ws: tad_grad_segnorm_workspace_bytes(nwork); a smaller one is refused.
 * tad_grad_segnorm_plan_check: host-side check of HOST copies of the two tables against a buffer of n floats (no GPU needed): every
 * segment inside [0, n), lengths > 0, slots in [0, nslots), at most one segment per slot, the work items tile every segment exactly
 * once and in order, none longer than the maximum, first_work consistent.  The device copies are not re-checked per call; the kernels
 * skip an item or slot that is out of range instead of following it. */
#define TAD_SEGNORM_WORK_MAX 16384
typedef struct { int64_t offset, length; int32_t slot, first_work; } tad_segnorm_seg;
typedef struct { int64_t offset, length; } tad_segnorm_work;
size_t tad_grad_segnorm_workspace_bytes(int nwork);
int tad_grad_segnorm_plan_check(const tad_segnorm_seg* table_host, int nseg, const tad_segnorm_work* work_host, int nwork, int64_t n,
                                int nslots);
/* Alignment: table, work: 8 bytes; ws: 4 bytes; grad, coef, acc, last, counters: any. */
int tad_grad_segnorm(const float* grad, int64_t n, const tad_segnorm_seg* table, int nseg, const tad_segnorm_work* work, int nwork,
                     const float* coef, double* acc, float* last, int32_t* counters, int nslots, void* ws, size_t ws_bytes,
                     tad_stream_t stream);

/* Batched bf16 transpose: every [R,C] matrix of a flat buffer -> [C,R] at the same offset of a second flat buffer, one launch (the
 * transposed operand copies W^T that the input-gradient GEMMs of all Linear layers read; refreshed once per optimizer step).
 * table (device, int32 [n_tiles][8]): per 64x64 tile {src offset, dst offset, C, R, valid rows, valid cols, 0, 0} in elements,
 * offsets < 2^32; R % 8 == C % 8 == 0 and 16-byte aligned matrices. */
int tad_transpose_bf16_batched(const uint16_t* src, uint16_t* dst, const int32_t* table, int n_tiles, tad_stream_t stream);

/* ---- optimizer tail -------------------------------------------------------------------------------------------
 * Fused multi-tensor AdamW over FLAT buffers: replaces torch.optim.AdamW as configured by optim_factory.create_optimizer
 * (optim_factory.py:91-127) with the layer-decay parameter groups of optim_factory.get_parameter_groups (:49-88) and the per-step
 * lr / weight-decay assignment of engine_for_finetuning.train_one_epoch (:49-54); the sum of g^2 that utils.get_grad_norm_
 * (utils.py:415-427) needs comes out of the same pass.
 * param / grad / exp_avg / exp_avg_sq: f32 [n], one shared layout in which every tensor starts on a TAD_ADAMW_CHUNK boundary.
 * chunk_group[c] (device, uint8, ceil(n / CHUNK) entries) = parameter-group index of chunk c, or 255 = leave the chunk untouched.
 * group_lr / group_wd / group_step: HOST arrays [n_groups] (this step's lr and weight decay; the 1-based count of updates the
 * group's tensors will have received after this call -- torch keeps it per parameter).  Update rule = torch.optim.AdamW:
 *   p *= 1 - lr*wd;  m += (1-b1)(g-m);  v = b2 v + (1-b2) g^2;  p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * grad_scale (device scalar or NULL): g is multiplied by *grad_scale first (gradient clipping and loss-scale removal without a host
 *   sync).  *grad_scale == 0 or not finite SKIPS the update (parameters, moments and the operand copy stay untouched; sumsq_partials
 *   is still written): the device-side form of GradScaler's "found inf -> skip the step" (utils.py:386-412).
 * param_bf16 (or NULL): receives bf16(p_new) -- the operand copy the next forward's GEMMs read.
 * sumsq_partials (or NULL): [ceil(n / CHUNK)] per-chunk sums of the UNSCALED g^2 (deterministic order). */
#define TAD_ADAMW_CHUNK 4096
#define TAD_ADAMW_MAX_GROUPS 128
/* Alignment: param_bf16: 8 bytes; chunk_group, grad_scale, sumsq_partials: any. */
int tad_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint16_t* param_bf16,
                   const uint8_t* chunk_group, int64_t n, const float* group_lr, const float* group_wd, int n_groups,
                   const int32_t* group_step, float beta1, float beta2, float eps, const float* grad_scale,
                   float* sumsq_partials, tad_stream_t stream);

/* Weight EMA over any number of f32 tensor pairs in ONE launch (timm.utils.ModelEma.update, engine_for_finetuning.py:98-99):
 *   ema[i] = fl( fl(ema[i] * decay) + fl(model[i] * one_minus_decay) )        (no FMA contraction: bit-exact with the reference's
 *   `ema_v * decay + (1. - decay) * model_v`, whose 1 - decay is taken in double; the caller passes both as floats).
 * tensors (device, int64 [n_tensors][4]): {ema address, model address, numel, 0} per pair; numel >= 1, 4-byte aligned addresses
 *   (float4 path where both are 16-byte aligned, scalar path otherwise).
 * chunks (device, int32 [n_chunks][2]): {tensor index, chunk index within the tensor}, one workgroup per TAD_EMA_CHUNK elements;
 *   every chunk of every tensor listed once.  The tables are host-built and reused while the addresses stay the same. */
#define TAD_EMA_CHUNK 8192
/* Alignment: tensors: any (8-byte rows); chunks: 8 bytes; the addresses inside the table: see above. */
int tad_ema_update(const int64_t* tensors, int n_tensors, const int32_t* chunks, int n_chunks, float decay, float one_minus_decay,
                   tad_stream_t stream);

/* Mixup / CutMix of the fine-tune loop on the device (mixup.py:159-218; applied at engine_for_finetuning.py:59-60 to the f32 clip batch).
 * plan: int32 [B][TAD_MIXUP_PLAN_WORDS], one row per sample i (partner j = B-1-i):
 *   {kind, w_self (f32 bits), w_other (f32 bits), t0, t1, y0, y1, x0, x1, lam (f32 bits), one_minus_lam (f32 bits), 0}
 *   kind TAD_MIX_KEEP:  x[i] untouched (mixup.py:166 / :183 / :198, lam == 1)
 *   kind TAD_MIX_BLEND: x[i] = fl( fl(x[i] * w_self) + fl(x[j] * w_other) )    (mixup.py:173, :191-192, :205-206; no FMA contraction)
 *   kind TAD_MIX_PASTE: x[i][:, t0:t1, y0:y1, x0:x1] = x[j][same box]          (mixup.py:170, :187-188, :203; pair mode cuts T and H)
 *   every right-hand side is the value BEFORE the call; lam / one_minus_lam are the soft target's coefficients of the sample.
 * tad_mixup_plan_check: host-side check of a HOST copy of the table (kinds, finite coefficients, boxes inside the clip); no launch.
 * tad_mixup_clips: x = contiguous f32 [B,C,T,H,W] on the device, B even, mixed in place in ONE launch (float4 accesses when x is
 *   16-byte aligned and W % 4 == 0, scalar otherwise); plan on the device.  A box is cut to the clip on the device as well.
 * tad_mixup_target: out f32 [B,num_classes] = mixup_target (mixup.py:22-27): fl( fl(y1 * lam) + fl(y2 * one_minus_lam) ) with
 *   y1 / y2 the rows of labels[b] / labels[B-1-b] (int64) holding on_value at the label and off_value elsewhere. */
#define TAD_MIXUP_PLAN_WORDS 12
#define TAD_MIX_KEEP 0
#define TAD_MIX_BLEND 1
#define TAD_MIX_PASTE 2
int tad_mixup_plan_check(const int32_t* plan_host, int B, int T, int H, int W);
/* Alignment: every pointer of tad_mixup_clips, tad_mixup_target, tad_soft_target_ce and tad_frame_loss: any. */
int tad_mixup_clips(float* x, const int32_t* plan, int B, int C, int T, int H, int W, tad_stream_t stream);
int tad_mixup_target(const int32_t* plan, const int64_t* labels, float* out, int B, int num_classes, float on_value, float off_value,
                     tad_stream_t stream);
/* Soft-target cross entropy (timm.loss.SoftTargetCrossEntropy / LabelSmoothingCrossEntropy, the criteria of
 * run_class_finetuning.py:467-473), forward and gradient in ONE launch, a wave per row of f32 logits [B,num_classes]:
 *   loss[0]  = (1/B) sum_b sum_c -t[b][c] * log_softmax(logits[b])[c]
 *   dlogits  = (softmax(logits[b]) * sum_c t[b][c] - t[b]) / B                 (the backward pass scales it by the incoming gradient)
 * t = target (f32 [B,num_classes]) when given; else t[b][c] = smoothing / num_classes + (c == labels[b] ? 1 - smoothing : 0) from
 * int64 labels.  Exactly one of target / labels is non-NULL; smoothing in [0, 1) (ignored with target). */
int tad_soft_target_ce(const float* logits, const float* target, const int64_t* labels, float smoothing, float* loss, float* dlogits,
                       int B, int num_classes, tad_stream_t stream);
/* The losses of the frame fine-tuning recipe (run_frame_finetuning.py:571-586: utils.FocalLoss / FocalLoss2 / TemporalExponentialLoss /
 * DoubleBCELoss / SmoothAPLoss), forward and gradient in ONE launch of one workgroup, a wave per row of f32 logits [B,num_classes]:
 *   loss[0] = the criterion's value (mean reduction), dlogits [B,num_classes] = d loss / d logits (the backward pass scales it).
 * With ce_b = logsumexp(logits[b]) - logits[b][labels[b]] and pt_b = exp(-ce_b):
 *   TAD_FRAME_LOSS_FOCAL        mean_b multiplier * alpha * (1 - pt_b)^gamma * ce_b
 *   TAD_FRAME_LOSS_FOCAL2       the same with class_alpha[labels[b]] (f32 [num_classes]; NULL: weight 1) in place of alpha
 *   TAD_FRAME_LOSS_EXPONENTIAL  mean_b w_b * ce_b, w_b = min(1, t < 0 ? exp(alpha_pre * t) : t > 0 ? exp(-alpha_post * t) : 1), t = ttc[b]
 *                               (f32 [B]; a NaN t gives weight 1, as the reference's masks do)
 *   TAD_FRAME_LOSS_BCE2         mean_b sum_{c in 0,1} bce_with_logits(logits[b][c], soft[b][c])        (soft f32 [B,2]; num_classes == 2)
 *   TAD_FRAME_LOSS_SMOOTHAP     (1 / max(P,1)) sum_{i: labels[i] == 1} sum_{j: labels[j] == 0} relu(p_j - p_i + delta), p = softmax(logits)[1],
 *                               P = number of rows with label 1 (num_classes == 2; no positive row: loss 0 and dlogits 0)
 * Each kind takes exactly its operands, the others NULL: labels (int64 [B]) for every kind but BCE2, soft for BCE2, ttc for EXPONENTIAL,
 * class_alpha optionally for FOCAL2.  gamma >= 1 for the focal kinds (below 1 the derivative is unbounded at pt = 1); gamma, multiplier and
 * delta finite and non-negative.  A label outside [0, num_classes) is the caller's error, as for tad_soft_target_ce: it is not checked,
 * and under FOCAL2 it indexes class_alpha. */
#define TAD_FRAME_LOSS_FOCAL 0
#define TAD_FRAME_LOSS_FOCAL2 1
#define TAD_FRAME_LOSS_EXPONENTIAL 2
#define TAD_FRAME_LOSS_BCE2 3
#define TAD_FRAME_LOSS_SMOOTHAP 4
int tad_frame_loss(int kind, const float* logits, const int64_t* labels, const float* soft, const float* ttc, const float* class_alpha,
                   float alpha, float gamma, float multiplier, float alpha_pre, float alpha_post, float delta, float* loss, float* dlogits,
                   int B, int num_classes, tad_stream_t stream);

/* RandomErasing of the fine-tune recipe on the device (random_erasing.py:151-173, applied by the datasets to every normalised clip
 * with --reprob 0.25 --remode pixel --recount 1, max_area 0.1, one box per clip shared by its frames).
 * boxes: int32 [n_boxes][TAD_ERASE_BOX_WORDS], one row per box in the order the reference writes them:
 *   {sample, mode, t0, t1, y0, y1, x0, x1}:  x[sample][:, t0:t1, y0:y1, x0:x1] = noise of `mode`
 *   Where boxes of one sample overlap, an element ends with the value of the LAST row that covers it (the reference's write order):
 *   a row leaves out every element that a later valid row of the same sample covers, so the result does not depend on the grid.
 * Noise (the one definition; csrc/erasing.hip implements it, tests/erasing_recipe.py restates it in float64).  With uint32 arithmetic,
 *   hash32(a, b, s) = fin(a * 0x9E3779B1 + b * 0x85EBCA77 + s),
 *   fin(v): v ^= v >> 16; v *= 0x7FEB352D; v ^= v >> 15; v *= 0x846CA68B; v ^= v >> 16   (the hash of the attention dropout mask),
 * and box = the row's index in the table, c = channel, t = frame, dy = y - y0, dx = x - x0 (y0, x0 after the cut to the clip):
 *   k  = hash32(dy, dx, hash32(c, t, hash32(sample, box, seed)))         TAD_ERASE_PIXEL: one value per element
 *   k  = hash32(0, 0, hash32(c, t, hash32(sample, box, seed)))           TAD_ERASE_RAND: one value per (box, frame, channel)
 *   k2 = hash32(0, 0, k + 0x6A09E667)
 *   u1 = ((k >> 8) + 1) * 2^-24 in (0, 1],  u2 = (k2 >> 8) * 2^-24 in [0, 1)
 *   value = sqrtf(-2 * logf(u1)) * cospif(2 * u2)                        Box-Muller, the accurate f32 functions; |value| <= 5.77
 *   TAD_ERASE_CONST: 0.0f.
 *   A value depends on (seed, sample, box, c, t, dy, dx) alone: not on the grid, the vector width or the alignment of x.
 * tad_erase_plan_check: host-side check of a HOST copy of the table (modes, 0 <= sample < B, boxes inside the clip); no launch.
 * tad_erase_clips: x = contiguous f32 [B,C,T,H,W] on the device, erased in place in ONE launch that writes the elements inside the
 *   boxes and reads nothing of x (16-byte stores on the aligned interior of a box row, 4-byte stores at its edges; same bits either
 *   way); boxes on the device.  On the device a box is cut to the clip and a row with an unknown mode or sample is ignored. */
#define TAD_ERASE_BOX_WORDS 8
#define TAD_ERASE_CONST 0
#define TAD_ERASE_RAND 1
#define TAD_ERASE_PIXEL 2
#define TAD_ERASE_MAX_BOXES 65535
int tad_erase_plan_check(const int32_t* boxes_host, int n_boxes, int B, int T, int H, int W);
/* Alignment: x, boxes: any. */
int tad_erase_clips(float* x, const int32_t* boxes, int n_boxes, uint32_t seed, int B, int C, int T, int H, int W, tad_stream_t stream);

/* RandAugment of the fine-tune recipe on the device (rand_augment.py of the reference: --aa rand-m6-n3-mstd0.5-inc1, applied by the
 * datasets to the PIL frames of every training clip), on uint8 frames [B,T,H,W,3], and the conversion to normalised f32 clips.
 * table: int32 [n_layers][B][TAD_RANDAUG_ROW_WORDS], per layer one row per clip (every sample exactly once):
 *   {sample, op, iarg, fill, bicubic_lo, bicubic_hi, farg, 0, a0 .. a5}
 *   op      TAD_RA_*: COPY (the layer's coin failed, or the operator is the identity), the lookup-table operators (iarg: Posterize's
 *           bits to keep 0..8, Solarize's threshold 0..256, SolarizeAdd's addend 0..255), the ImageEnhance operators (farg: the
 *           factor, f32 bits) and AFFINE (Rotate, ShearX/Y, TranslateX/YRel: a0..a5 = the coefficients PIL's Image.transform(AFFINE)
 *           receives, six doubles each as low word, high word; fill = R | G << 8 | B << 16 where no source pixel maps; bit t of
 *           bicubic_lo / bicubic_hi (t >= 32) set = frame t is resampled BICUBIC, clear = BILINEAR).
 *   All frames of a clip share op and argument; AutoContrast, Equalize and Contrast take their statistics per frame.
 *   csrc/randaug.hip states each operator's arithmetic (PIL's: integers, C float for ImageEnhance, C double for the affine map).
 * tad_randaug_plan_check: host-side check of a HOST copy of the table (n_words = its length, which must be n_layers * B * ROW_WORDS;
 *   known ops, 0 <= sample < B once per layer, argument ranges, finite factors and coefficients); no launch.
 * tad_randaug_apply: x -> out (two buffers of B*T*H*W*3 bytes, any alignment; x is only read), table on the device.  Per layer ONE
 *   apply launch, preceded by ONE statistics launch iff bit `layer` of stats_layers is set (the caller sets it when a row of the layer is
 *   AUTOCONTRAST, EQUALIZE or CONTRAST); layers alternate between out and a second buffer in the workspace (256-byte aligned,
 *   tad_randaug_workspace_bytes).  n_layers == 0 copies.  On the device a row with an unknown op copies its clip; a row whose sample
 *   is outside the batch is ignored, and a clip that no row of a layer names is left unwritten by that layer: its bytes in out are
 *   undefined (tad_randaug_plan_check refuses such tables).
 * tad_frames_to_clip: out f32 [B,3,T,H,W] = ((float)x / 255 - mean[c]) / std[c] of x uint8 [B,T,H,W,3], IEEE division and
 *   subtraction in f32 (torchvision's ToTensor, the reference's tensor_normalize, permute: dota.py:308-316); mean / std: 3 host floats. */
#define TAD_RANDAUG_ROW_WORDS 20
#define TAD_RANDAUG_MAX_LAYERS 32
#define TAD_RANDAUG_STAT_BYTES 1024
#define TAD_RA_COPY 0
#define TAD_RA_INVERT 1
#define TAD_RA_POSTERIZE 2
#define TAD_RA_SOLARIZE 3
#define TAD_RA_SOLARIZE_ADD 4
#define TAD_RA_AUTOCONTRAST 5
#define TAD_RA_EQUALIZE 6
#define TAD_RA_BRIGHTNESS 7
#define TAD_RA_COLOR 8
#define TAD_RA_CONTRAST 9
#define TAD_RA_SHARPNESS 10
#define TAD_RA_AFFINE 11
int tad_randaug_plan_check(const int32_t* table_host, int64_t n_words, int n_layers, int B, int T);
size_t tad_randaug_workspace_bytes(int n_layers, int B, int T, int H, int W);
/* Alignment: x, out, table: any; workspace: 256 bytes.  tad_frames_to_clip: x, out: any. */
int tad_randaug_apply(const uint8_t* x, uint8_t* out, const int32_t* table, int n_layers, uint32_t stats_layers, void* workspace,
                      size_t workspace_bytes, int B, int T, int H, int W, tad_stream_t stream);
int tad_frames_to_clip(const uint8_t* x, float* out, const float* mean, const float* std_, int B, int T, int H, int W, tad_stream_t stream);

/* The MAE pre-training crop on the device (transforms.py of the reference: GroupMultiScaleCrop = a multi-scale crop, then PIL's
 * antialiased BILINEAR resize of every frame; DataAugmentationForVideoMAE chains Stack, ToTorchFormatTensor and GroupNormalize
 * behind it), on uint8 frames [B,T,Hs,Ws,3]; all clips of a call share one source size.
 * table: int32, three parts in this order:
 *   rows    [B][TAD_MSC_ROW_WORDS], one per clip (every sample exactly once): {sample, x0, y0, w, h, hset, vset, 0}: the crop
 *           x[sample][:, y0:y0+h, x0:x0+w] and the indices of its horizontal (w -> S_w) and vertical (h -> S_h) coefficient set
 *   hsets   [n_hsets] slots of TAD_MSC_SET_HEAD + S_w * (2 + TAD_MSC_MAX_KSIZE) words
 *   vsets   [n_vsets] slots of TAD_MSC_SET_HEAD + S_h * (2 + TAD_MSC_MAX_KSIZE) words
 *   a set = {in, out, ksize, 0}, bounds[out][2] = (xmin, count), kk[out][ksize]; the rest of its slot is unused.  The host states the
 *   sets as Pillow's precompute_coeffs and normalize_coeffs_8bpc do (doubles, rounded to 22-bit integers); one set per distinct
 *   (crop extent -> output extent) of a call.  in <= 8 * out (filter scale <= 8, ksize <= 17).
 * Arithmetic on the device, Pillow's, in int32: the horizontal pass gives a rounded byte, the vertical pass runs over those bytes;
 *   each pass is ss = 1 << 21; ss += pixel * k over the `count` taps from xmin; byte = clip(ss >> 22, 0, 255).
 * tad_multiscale_crop_workspace_bytes: the size of the table = of the workspace, which holds nothing else and is only read.
 * tad_multiscale_crop_plan_check: host-side check of a HOST copy of the table (n_words = its length, which must be the sum of the
 *   three parts; 0 <= sample < B exactly once; crops inside the source; set indices in range and sets stated for the crop's
 *   extents; in <= 8 * out; 1 <= ksize <= TAD_MSC_MAX_KSIZE; 0 <= count <= ksize and xmin + count <= in); no launch.
 * tad_multiscale_crop: ONE launch, no host synchronisation; x is only read.  out_f32 == 0: out = uint8 [B,T,S_h,S_w,3], any
 *   alignment; mean / std_ are ignored.  out_f32 != 0: out = f32 [B,3,T,S_h,S_w] = ((float)byte / 255 - mean[c]) / std_[c], the
 *   bits tad_frames_to_clip gives on the uint8 result; mean / std_: 3 host floats.  workspace = the table on the device.  On the
 *   device a crop is cut to the source, a set index to the sets, bounds to the crop and to ksize, and a row whose sample is outside
 *   the batch is ignored (a malformed table is never an address); a clip that no row names is left unwritten. */
#define TAD_MSC_ROW_WORDS 8
#define TAD_MSC_SET_HEAD 4
#define TAD_MSC_MAX_KSIZE 17
#define TAD_MSC_MAX_SETS 64
size_t tad_multiscale_crop_workspace_bytes(int B, int n_hsets, int n_vsets, int S_h, int S_w);
int tad_multiscale_crop_plan_check(const int32_t* table_host, int64_t n_words, int B, int n_hsets, int n_vsets, int Hs, int Ws, int S_h,
                                   int S_w);
/* Alignment: x, out: any; workspace: 4 bytes. */
int tad_multiscale_crop(const uint8_t* x, void* out, int out_f32, const float* mean, const float* std_, const void* workspace,
                        size_t workspace_bytes, int B, int T, int Hs, int Ws, int S_h, int S_w, int n_hsets, int n_vsets, tad_stream_t stream);

/* The loader resize of the fine-tune and inference paths on the device: cv2.resize(frame, (S_w, S_h), INTER_CUBIC) of every decoded
 * frame (run_inference.py:76,91; dota.py:347-348; dada.py:309-310), optionally behind video_transforms.pad_wide_clips (:1301-1337),
 * on uint8 frames [B,T,H,W,3]; all clips of a call share one source size.
 * THE CONTRACT is OpenCV's generic integer formulation of the 8-bit cubic resize as stated here, not the bytes of a particular OpenCV
 * build: a build's vector path finishes the vertical pass in float, its scalar path in integers, the two can differ by one grey
 * level, and which bytes take which path depends on the build and the row width.  The tests hold the kernel to a CPU restatement of
 * this text bit for bit, and that restatement to an independent float64 bicubic within one grey level.
 * Per axis, on the HOST (numpy float32 / float64; the device sees integers only), source extent n_src, output extent n_dst:
 *   scale = n_src / n_dst                           a double
 *   f = float32((d + 0.5) * scale - 0.5)            the double expression, rounded once
 *   s = floor(f);  x = float32(f - s)
 *   Keys' cubic weights, A = -0.75f, every operation in float32:
 *     c0 = ((A*(x+1) - 5A)*(x+1) + 8A)*(x+1) - 4A;   c1 = ((A+2)*x - (A+3))*x*x + 1
 *     c2 = ((A+2)*(1-x) - (A+3))*(1-x)*(1-x) + 1;    c3 = 1 - c0 - c1 - c2
 *   k[j] = saturate_int16(rint(c_j * 2048f)), ties to even.  The four k are NOT renormalised: their sum is 2047, 2048 or 2049, and
 *   sum |k| <= TAD_FR_MAX_ABS_SUM.  first = s - 1; the taps are source indices first .. first + 3, each clamped to [0, n_src - 1]
 *   (replicate border) ON THE DEVICE: first lies in [-2, n_src - 2].  Equal extents give k = (0, 2048, 0, 0): output == input.
 * On the device, two passes in int32 with no rounding in between:
 *   h[row][d] = sum_j src[row][tap_j] * kx[d][j]
 *   byte      = clip((sum_j h[tap_j][d] * ky[r][j] + (1 << 21)) >> 22, 0, 255)        arithmetic shift
 *   (255 * 2818 * 2818 + 2^21 < 2^31)
 * Wide-clip padding is a VIRTUAL source of pad_top + H + pad_bottom rows that the vertical pass indexes; no padded frame exists.
 * Virtual row v inside the frame (pad_top <= v < pad_top + H) is the frame's row in every mode; a band row is, per mode:
 *   TAD_FR_CONST      every byte of stored channel c is (colour >> 8c) & 255 (black: colour = 0)
 *   TAD_FR_REPLICATE  frame row 0 (top band) or H - 1 (bottom band)
 *   TAD_FR_REFLECT    top band row v = frame row pad_top - 1 - v, the j-th row of the bottom band = frame row H - 1 - j (cv2's
 *                     BORDER_REFLECT: the edge row doubled), each byte faded to rint((float)p * alpha), ties to even, the product
 *                     on its own: cv2.addWeighted(reflect, a, black, 1 - a, 0), which inside the frame returns the byte itself
 *   A pad above H would need a second reflection and is refused.
 * table: int32, three parts in this order:
 *   rows    [B][TAD_FR_ROW_WORDS], one per clip (every sample exactly once):
 *           {sample, mode, pad_top, pad_bottom, alpha (f32 bits), colour (c0 | c1 << 8 | c2 << 16), vset, 0}
 *   hset    ONE horizontal set of TAD_FR_SET_HEAD + S_w * 5 words (W -> S_w)
 *   vsets   [n_vsets] vertical sets of TAD_FR_SET_HEAD + S_h * 5 words, one per distinct virtual height (pad_top + H + pad_bottom -> S_h)
 *   a set = {in, out, 0, 0}, first[out], k[out][4]
 * tad_frame_resize_workspace_bytes: the size of the table = of the workspace, which holds nothing else and is only read.
 * tad_frame_resize_plan_check: host-side check of a HOST copy of the table (n_words = its length, which must be the sum of the three
 *   parts; 0 <= sample < B exactly once; a known mode; 0 <= pad <= H, both 0 under TAD_FR_NONE; alpha in [0, 1] under REFLECT; vset in
 *   range and stated for the row's virtual height; the horizontal set stated for W; first in [-2, in - 2]; sum |k| <=
 *   TAD_FR_MAX_ABS_SUM); no launch.
 * tad_frame_resize: ONE launch, no host synchronisation; x is only read.  out_f32 == 0: out = uint8 [B,T,S_h,S_w,3], any alignment
 *   (a slot of a ring buffer, a slice of a frame store); mean / std_ are ignored.  out_f32 != 0: out = f32 [B,3,T,S_h,S_w] =
 *   ((float)byte / 255 - mean[c]) / std_[c], the bits tad_frames_to_clip gives on the uint8 result; mean / std_: 3 host floats.
 *   workspace = the table on the device.  On the device the mode is cut to the known modes, a pad to [0, H], a set index to the sets,
 *   every tap to its source, a faded byte to [0, 255], and a row whose sample is outside the batch is ignored (a malformed table is
 *   never an address); a clip that no row names is left unwritten.  Source pixels are loaded as the aligned 4-byte words that hold
 *   them: up to three bytes to either side of x share a word with its first / last pixel and are loaded and dropped. */
#define TAD_FR_ROW_WORDS 8
#define TAD_FR_SET_HEAD 4
#define TAD_FR_MAX_SETS 64
#define TAD_FR_MAX_ABS_SUM 2818
#define TAD_FR_NONE 0
#define TAD_FR_CONST 1
#define TAD_FR_REFLECT 2
#define TAD_FR_REPLICATE 3
size_t tad_frame_resize_workspace_bytes(int B, int n_vsets, int S_h, int S_w);
int tad_frame_resize_plan_check(const int32_t* table_host, int64_t n_words, int B, int n_vsets, int H, int W, int S_h, int S_w);
/* Alignment: x, out: any; workspace: 4 bytes. */
int tad_frame_resize(const uint8_t* x, void* out, int out_f32, const float* mean, const float* std_, const void* workspace,
                     size_t workspace_bytes, int B, int T, int H, int W, int S_h, int S_w, int n_vsets, tad_stream_t stream);

/* The spatial sampling of the class fine-tuning recipe on the device (kinetics.py / ssv2.py of the reference: spatial_sampling, i.e.
 * video_transforms.random_resized_crop, random_resized_crop_with_shift, or random_short_side_scale_jitter + random_crop, then
 * horizontal_flip; with spatial_idx 0 / 1 / 2 the jitter + uniform_crop).  Every route is: a window of the source frame, a bilinear
 * resize of the window (torch.nn.functional.interpolate, mode="bilinear", align_corners=False, no antialiasing) to a grid, an S x S
 * window of that grid, an optional horizontal flip.  x is the f32 clips [B,3,T,H,W] or the uint8 frames [B,T,H,W,3]; out is the f32
 * clips [B,3,T,S,S]; all clips of a call share one source size.
 * table: int32 [B * T][TAD_SS_ROW_WORDS], one row per (clip, frame), every frame exactly once:
 *   {sample, i, j, h, w, rh, rw, oy, ox, flip, scale_y, scale_x}
 *   sample   clip * T + frame
 *   i, j     origin (row, column) of the source window; h, w its extent: x[clip][.., frame, i:i+h, j:j+w]
 *   rh, rw   the grid the window is resized to
 *   oy, ox   origin of the S x S output inside that grid: output (y, x) is grid (oy + y, ox + x)
 *   flip     1: output column x holds column S - 1 - x of the unflipped result
 *   scale_y, scale_x   f32 bit patterns of (float)h / (float)rh and (float)w / (float)rw, stated by the host (the device never divides
 *            for a coordinate)
 *   Crop + resize to S x S: window = the box, grid = S x S, offset 0.  Resize of the whole frame + crop: window = the frame, grid = the
 *   resized frame, offset = the crop's.
 * Arithmetic on the device -- the contract: per axis, in f32, every product, sum and difference rounded on its own (no contraction),
 *   with d the index in the resized grid and n_in the window's extent along the axis:
 *     src = max(scale * (d + 0.5f) - 0.5f, 0)
 *     i0  = min((int)src, n_in - 1);   i1 = min(i0 + 1, n_in - 1)
 *     l1  = src - (float)i0;           l0 = 1 - l1
 *   value = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d), evaluated in that order, with a = (i0y, i0x), b = (i0y, i1x),
 *   c = (i1y, i0x), d = (i1y, i1x) of the window.  From uint8 frames each of the four taps first becomes
 *   ((float)byte / 255 - mean[c]) / std_[c], tad_frames_to_clip's value: the result has the bits of the f32 route on
 *   tad_frames_to_clip(x).
 * tad_spatial_sample_workspace_bytes: the size of the table = of the workspace, which holds nothing else and is only read.
 * tad_spatial_sample_plan_check: host-side check of a HOST copy of the table (n_words = its length, which must be B * T *
 *   TAD_SS_ROW_WORDS; 0 <= sample < B * T exactly once; source windows inside the H x W source; output windows inside the resized
 *   grid; flip 0 or 1; scales positive and finite); no launch.
 * tad_spatial_sample: ONE launch, no host synchronisation; x is only read.  x_u8 == 0: x = f32 clips, mean / std_ are ignored;
 *   x_u8 != 0: x = uint8 frames (any alignment), mean / std_: 3 host floats.  out: 4-byte aligned (16-byte stores are used where the
 *   address allows them).  workspace = the table on the device.  On the device a source window is cut to the source, the tap indices
 *   to the window whatever the scales and offsets hold, and a row whose sample is outside the batch is ignored (a malformed table is
 *   never an address); a frame that no row names is left unwritten. */
#define TAD_SS_ROW_WORDS 12
size_t tad_spatial_sample_workspace_bytes(int B, int T);
int tad_spatial_sample_plan_check(const int32_t* table_host, int64_t n_words, int B, int T, int H, int W, int S);
/* Alignment: x, out: any; workspace: 4 bytes. */
int tad_spatial_sample(const void* x, int x_u8, float* out, const float* mean, const float* std_, const void* workspace,
                       size_t workspace_bytes, int B, int T, int H, int W, int S, tad_stream_t stream);

/* ---- MAE pre-training path: what modeling_pretrain.py / engine_for_pretraining.py add around the Block stack ----
 * Rows are D f32, D % 4 == 0.  idx arrays are int32 on the device. */
/* out[r] = src[idx[r]], r < n_out: x[~mask].reshape(B,-1,C) (modeling_pretrain.py:98) with idx = b*N + visible token */
/* Alignment: idx (here and in tad_scatter_rows_f32), vis_idx, mask_idx: any. */
int tad_gather_rows_f32(const float* src, const int32_t* idx, float* out, int64_t n_out, int D, tad_stream_t stream);
/* out[idx[r]] = src[r], r < n_in (unique indices; the caller zero-fills out): backward of the gather */
int tad_scatter_rows_f32(const float* src, const int32_t* idx, float* out, int64_t n_in, int D, tad_stream_t stream);
/* decoder input (modeling_pretrain.py:283-288): out [B, n_vis+n_mask, D] = cat(x_vis + pos[vis_idx], mask_token + pos[mask_idx]);
 * x_vis [B*n_vis, D], mask_token [D], pos [N, D], vis_idx [B*n_vis] / mask_idx [B*n_mask] = token index inside the clip */
int tad_mae_assemble(const float* x_vis, const float* mask_token, const float* pos, const int32_t* vis_idx, const int32_t* mask_idx,
                     float* out, int B, int n_vis, int n_mask, int D, tad_stream_t stream);
/* reconstruction target (engine_for_pretraining.py:51-66): videos [B,3,T,H,W] f32 (normalised clip) -> labels [B*n_mask,
 * tub*p*p*3] for the masked tokens: v = x*std + mean, patch layout 'b n (p0 p1 p2) c', and with normalize_target each
 * (patch, channel) is standardised over its pixels: (v - mean) / (sqrt(unbiased var) + 1e-6).  The mean is refined by the mean of
 * the residuals, so a constant (patch, channel) gives exactly 0 (the fp64 value), not f32 rounding noise.  mean3 / std3: HOST arrays. */
/* Alignment: videos, mask_idx, labels: any. */
int tad_mae_target(const float* videos, const int32_t* mask_idx, float* labels, int B, int n_mask, int T, int H, int W, int tubelet,
                   int patch, const float* mean3, const float* std3, int normalize_target, tad_stream_t stream);
/* nn.MSELoss() (engine_for_pretraining.py:27,70): partials[tad_mse_loss_blocks(n)] = block sums of (pred-target)^2 (the loss is
 * their sum / n); grad (nullable) = 2 (pred - target) / n */
int tad_mse_loss_blocks(int64_t n);
/* Alignment: partials: any. */
int tad_mse_loss(const float* pred, const float* target, int64_t n, float* partials, float* grad, tad_stream_t stream);

/* ---- evaluation path -----------------------------------------------------------------------------------------
 * Exact integer counts behind every thresholded metric of engine_for_frame_finetuning.calculate_metrics (:593-636) and
 * anaysis/metrics.calculate_MORE_metrics (:127-208), which test `pred >= t` for t in np.arange(0, 1.001, 0.01).
 * thresholds: ascending f32 [n_thresholds <= 255] (device); labels int32 (non-zero = positive);
 * hist int64 [2][n_thresholds+1] (device, overwritten): hist[l][k] = number of samples with label l and k = #{t : p >= t}.
 * The confusion matrix at threshold index i is then  TP = sum_{k>i} hist[1][k], FN = sum_{k<=i} hist[1][k], FP / TN likewise. */
/* Alignment: every pointer of tad_threshold_histogram, tad_group_threshold_histogram and tad_group_rank_stats: any. */
int tad_threshold_histogram(const float* probs, const int32_t* labels, const float* thresholds, int n_thresholds, int64_t n,
                            int64_t* hist, tad_stream_t stream);

/* ---- grouped evaluation report (anaysis/metrics_dota.py, metrics_dada.py, metrics_by_categories.py) ---------------------------
 * The same counts for up to 64 sample groups at once (TOTAL, accident categories, ego / non-ego, night / day ...): bit g of
 * member[i] says that sample i belongs to group g; a sample may belong to any number of groups, also to none.
 * tad_group_threshold_histogram: hist int64 [n_groups][2][n_thresholds+1] (device, overwritten): hist[g] is tad_threshold_histogram's
 * table over the members of group g (same comparison in f32, NaN gives k = 0, ascending thresholds, exact counts; n_groups = 1 with
 * every mask = 1 gives that table bit for bit).  1 <= n_groups <= 64, 1 <= n_thresholds <= 255. */
int tad_group_threshold_histogram(const float* probs, const int32_t* labels, const uint64_t* member, int n_groups,
                                  const float* thresholds, int n_thresholds, int64_t n, int64_t* hist, tad_stream_t stream);
/* tad_group_rank_stats: scikit-learn's roc_auc_score / average_precision_score of every group from ONE ordering of all samples.
 * labels_sorted / member_sorted: the samples in DESCENDING score order; run_end[i] = 1 where score[i] != score[i+1] (compared in f32:
 * -0.0 and 0.0 tie) or i == n - 1, else 0.  A run of tied scores counts for a group only through the group's members in it, so the
 * runs of the whole array are the right runs for every group.  With T, F the group's positives / negatives up to a run end e and
 * (T_s, F_s) those at the run end before it (0, 0 at the start):
 *   out_int[g] = {P, N, U2},  U2 = sum_e (F_e - F_s)(T_e + T_s) = 2 P N AUROC, an exact integer (AUROC = U2 / (2 P N) on the host)
 *   out_ap[g]  = sum_e (T_e - T_s) T_e / (T_e + F_e) / P in fp64; 0 when P == 0 (scikit-learn's value for a group without positives)
 * One workgroup per group walks the array in tiles of TAD_GROUP_RANK_TILE samples; the fp64 sum runs in a fixed order (no
 * floating-point atomics): two calls give the same bits.  No workspace.  1 <= n_groups <= 64, 1 <= n < 2^31. */
#define TAD_GROUP_RANK_TILE 4096
int tad_group_rank_stats(const int32_t* labels_sorted, const uint64_t* member_sorted, const uint8_t* run_end, int n_groups, int64_t n,
                         int64_t* out_int, double* out_ap, tad_stream_t stream);

/* ---- "precise" mode (parity gate, not throughput): f32-accurate Linear via split-bf16 operands, f32 attention ----------
 * x = hi + lo (bf16 each).  concat mode: out [M,3K] = [hi|hi|lo] (role_b=0) or [hi|lo|hi] (role_b=1); stack mode: out [3M,K]
 * with the three parts stacked along rows.  Feeding tad_linear_* with both operands split this way (K or M tripled) gives the
 * f32 product to ~2^-17 using the same MFMA kernels. */
/* Alignment: out: 8 bytes. */
int tad_split_bf16x3(const float* x, uint16_t* out, int64_t M, int K, int role_b, int stack, tad_stream_t stream);
int tad_im2col_tubelets_f32(const float* x, float* cols, int B, int C, int T, int H, int W, int tubelet, int patch,
                            tad_stream_t stream);
/* f32 attention on the matrix pipe (exact-f32 MFMA), head dim d = 64 or 80: qkv [B,N,3,H,d] f32 -> out [B,N,H,d] f32, lse [B,H,N]
 * (nullable).  dropout_p in [0, 1): nn.Dropout on the softmax matrix (modeling_finetune.py:99-101; flash_attention_class.py:59-61) --
 * element (b, h, query, key) is kept iff lowbias32(row * 0x9E3779B1 + key * 0x85EBCA77 + seed) >= dropout_p * 2^32 with
 * row = (b H + h) N + query, kept probabilities scaled by 1 / (1 - dropout_p); the backward regenerates the same bits from (p, seed). */
/* Alignment: lse: any. */
int tad_attn_fwd_f32(const float* qkv, float* out, float* lse, int B, int N, int H, int d, float scale, float dropout_p, uint32_t seed,
                     tad_stream_t stream);

/* precise-mode backward pieces: f32 attention backward (dqkv [B,N,3,H,64] f32 fully overwritten; delta [B,H,N] scratch),
 * erf-GELU forward / backward on f32, column sums of an f32 matrix (bias gradients). */
/* Alignment: lse, delta: any. */
int tad_attn_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* delta,
                     int B, int N, int H, int d, float scale, float dropout_p, uint32_t seed, tad_stream_t stream);
/* Alignment: every pointer of tad_gelu_f32 and tad_gelu_bwd_f32: any. */
int tad_gelu_f32(const float* h, float* a, int64_t n, tad_stream_t stream);
int tad_gelu_bwd_f32(const float* dy, const float* h, float* dh, int64_t n, tad_stream_t stream);
/* Alignment: a: any when N % 4 != 0 (16 bytes otherwise); out: any. */
int tad_colsum_f32(const float* a, float* out, int64_t M, int N, tad_stream_t stream);

/* ---- device info ------------------------------------------------------------------------ */
int tad_device_info(int* cu_count, int* clock_khz, int* lds_bytes_per_cu, char* name, int name_len);

/* ---- gradient exchange over RCCL / xGMI for C hosts --------------------------------------------------------------------------
 * Replaces, for a host without torch, the two collectives of the reference's data-parallel wrap: DistributedDataParallel's
 * gradient all-reduce (run_class_finetuning.py:446-448; process group from utils.init_distributed_mode, utils.py:283-333,
 * backend 'nccl' at :325) and its initial parameter broadcast.  The Python host keeps torch.distributed (whose "nccl" backend is
 * RCCL on ROCm): parallel.DataParallel.  One communicator per process, one process per GPU; rank 0 creates the 128-byte id with
 * tad_rccl_unique_id and hands it to the other ranks by any host channel (file, environment, socket); every rank then calls
 * tad_rccl_init with the device it will use already current (hipSetDevice).  All-reduce and broadcast are in place and ordered on
 * `stream`; `average` != 0 divides by the number of ranks (ncclAvg).  librccl.so.1 is opened on first use (no link-time
 * dependency): on a host without it these calls return TAD_ELAUNCH and the rest of the library is unaffected. */
#define TAD_RCCL_UNIQUE_ID_BYTES 128
typedef void* tad_comm_t;
int tad_rccl_unique_id(void* id128);
int tad_rccl_init(const void* id128, int nranks, int rank, tad_comm_t* comm);
int tad_rccl_world_size(tad_comm_t comm, int* nranks);
int tad_rccl_allreduce(tad_comm_t comm, void* buf, size_t count, int dtype, int average, tad_stream_t stream);
int tad_rccl_broadcast(tad_comm_t comm, void* buf, size_t count, int dtype, int root, tad_stream_t stream);
int tad_rccl_destroy(tad_comm_t comm);

/* ---- IEEE half operand twins ------------------------------------------------------------------------------------------------------
 * The reference trains under torch.cuda.amp.autocast() -- float16 on CUDA -- with a GradScaler (engine_for_finetuning.py:67,
 * utils.py:386-412).  Every entry point above that takes or produces 16-bit GEMM / attention operands therefore exists a second
 * time with IEEE half in place of bfloat16: identical signature, semantics, kernels and schedules (the sources are compiled twice,
 * csrc/common.h), TAD_F16 in place of TAD_BF16 wherever a dtype argument selects the 16-bit type.  Half carries 11 significant bits
 * against bfloat16's 8 (operand rounding 2^-12 instead of 2^-9) at the same MFMA rate, and a narrower range (6e-8 .. 65504): the
 * backward pass runs on loss-scaled gradients exactly as in the reference (engine.NativeScalerWithGradNormCount; the scale is removed,
 * and an overflowed step skipped, inside tad_adamw_step_f16 through its grad_scale argument). */
int tad_cast_f32_f16(const float* src, uint16_t* dst, int64_t n, tad_stream_t stream);
int tad_transpose_cast_f32_f16(const float* src /*[R,C]*/, uint16_t* dst /*[C,R]*/, int R, int C, tad_stream_t stream);
int tad_scale_cast_f16(const float* x, uint16_t* y, const float* gamma, const float* rowscale, int rows_per_scale, int64_t M, int N,
                       tad_stream_t stream);
int tad_colsum_f16(const uint16_t* a, float* out, int accumulate, void* ws, size_t ws_bytes, int64_t M, int N, tad_stream_t stream);
int tad_split_f16x3(const float* x, uint16_t* out, int64_t M, int K, int role_b, int stack, tad_stream_t stream);
int tad_im2col_tubelets_f16(const float* x, uint16_t* cols, int B, int C, int T, int H, int W, int tubelet, int patch,
                            tad_stream_t stream);
int tad_im2col_tubelets_u8_f16(const uint8_t* frames, uint16_t* cols, int B, int T, int H, int W, int tubelet, int patch,
                               const float* mean3, const float* std3, int bgr, int t_offset, tad_stream_t stream);
int tad_patch_embed_fwd_f16(const float* x, const uint16_t* w_f16, const float* bias, const float* pos, float* out, uint16_t* cols,
                            int B, int C, int T, int H, int W, int tubelet, int patch, int D, tad_stream_t stream);
int tad_patch_embed_fwd_implicit_f16(const float* x, const uint16_t* w_f16, const float* bias, const float* pos, float* out, int B, int C,
                                     int T, int H, int W, int tubelet, int patch, int D, tad_stream_t stream);
int tad_patch_embed_gemm_f16(const uint16_t* cols, const uint16_t* w_f16, const float* bias, const float* pos, float* out, int64_t M,
                             int ntok, int D, int K, tad_stream_t stream);
int tad_patch_embed_bwd_f16(const uint16_t* dy_f16, const uint16_t* cols, float* dW, float* db, void* ws, size_t ws_bytes, int64_t M,
                            int D, int K, tad_stream_t stream);
int tad_layernorm_fwd_f16(const float* x, const float* gamma, const float* beta, void* y, int y_dtype, float* mean, float* rstd,
                          int64_t rows, int D, float eps, tad_stream_t stream);
int tad_layernorm_bwd_f16(const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean, const float* rstd,
                          const float* dres, float* dx, uint16_t* dx_f16, float* dgamma, float* dbeta, float* colsum_dx,
                          const float* rowscale, int rows_per_scale, int accumulate, void* ws, size_t ws_bytes, int64_t rows, int D,
                          tad_stream_t stream);
int tad_linear_fwd_f16(const uint16_t* x, const uint16_t* w, const float* bias, void* y, int y_dtype, int epilogue, uint16_t* preact,
                       const float* residual, const float* gamma, const float* rowscale, int rows_per_scale, void* ws, size_t ws_bytes,
                       int64_t M, int N, int K, tad_stream_t stream);
int tad_linear_fwd_qkv_f16(const uint16_t* x, const uint16_t* w, const float* q_bias, const float* v_bias, void* y, int y_dtype,
                           float q_prescale, int64_t M, int N, int K, tad_stream_t stream);
int tad_linear_bwd_input_f16(const uint16_t* dy, const uint16_t* wT, void* dx, int dx_dtype, const uint16_t* gelu_preact, void* ws,
                             size_t ws_bytes, int64_t M, int N, int K, tad_stream_t stream);
int tad_linear_bwd_weight_f16(const uint16_t* dy, const uint16_t* x, float* dW, float* db, int accumulate, void* ws, size_t ws_bytes,
                              int64_t M, int N, int K, tad_stream_t stream);
int tad_linear_bwd_weight_qkv_f16(const uint16_t* dy, const uint16_t* x, float* dW, float* dq_bias, float* dv_bias, int accumulate,
                                  void* ws, size_t ws_bytes, int64_t M, int N, int K, tad_stream_t stream);
int tad_linear_bwd_weight_pair_f16(const uint16_t* dy1, const uint16_t* x1, float* dW1, float* db1, float* db1b, int N1,
                                   const uint16_t* dy2, const uint16_t* x2, float* dW2, int N2, int accumulate, void* ws,
                                   size_t ws_bytes, int64_t M, int K, tad_stream_t stream);
int tad_attn_fwd_f16(const uint16_t* qkv, void* out, int out_dtype, uint16_t* out_lo, float* lse, const float* clip_scale, int B, int N,
                     int H, int d, float scale, int q_prescaled, float dropout_p, uint32_t seed, tad_stream_t stream);
int tad_attn_bwd_f16(const uint16_t* qkv, const uint16_t* out, const uint16_t* out_lo, const uint16_t* dout, const float* lse,
                     const float* clip_scale, uint16_t* dqkv, float* delta, int B, int N, int H, int d, float scale, int q_prescaled,
                     float dropout_p, uint32_t seed, tad_stream_t stream);
int tad_meanpool_bwd_f16(const float* dy, float* dx, uint16_t* dx_f16, int B, int N, int D, tad_stream_t stream);
int tad_adamw_step_f16(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint16_t* param_f16,
                       const uint8_t* chunk_group, int64_t n, const float* group_lr, const float* group_wd, int n_groups,
                       const int32_t* group_step, float beta1, float beta2, float eps, const float* grad_scale,
                       float* sumsq_partials, tad_stream_t stream);
int tad_rowscale_transpose_cast_f16(const float* w, const float* gamma, uint16_t* out, int N, int K, tad_stream_t stream);
int tad_branch_dropout_cast_f16(const float* g, uint16_t* y, const float* rowscale, int rows_per_scale, float p, uint32_t seed, int64_t M,
                                int D, tad_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TAD_MI355X_H */
