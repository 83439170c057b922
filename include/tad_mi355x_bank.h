/*
 * tad_mi355x_bank.h -- the STREAM-BANK ABI: the sixth surface of this package, tadb_*, TADB_ABI_VERSION 1, in a shared library of its
 * own, libtad_mi355x_bank.so (csrc/stream_bank.hip).  libtad_mi355x.so is held at its three surfaces (tad_*, tadx_*, tadp_*),
 * libtad_mi355x_serve.so at its one (tads_*) and libtad_mi355x_recon.so at its one (tadr_*), each from a pinned source list, so what
 * feeding many camera streams at once adds is linked apart, the way those two were.  The library is self-contained: it is compiled with
 * hidden visibility, exports these entry points and nothing else, and keeps an error text of its own behind tadb_last_error_string().
 *
 * Every other convention is the core header's: plain C, device pointers and explicit sizes, `stream` a hipStream_t passed as void*,
 * 0 or a negative TAD_E* code, no allocation, no synchronisation, every check made on the host before anything is launched.  Nothing
 * here takes a workspace and nothing uses atomics or talks across workgroups: two calls give the same bits.
 *
 * Pointer alignment (refused with TAD_EINVAL and "<entry point>: <argument> is misaligned: it must be N-byte aligned"):
 *   - src is read as the aligned 4-byte words that hold the pixels asked for, and every frame starts on a multiple of 4 inside it:  4 bytes
 *   - table holds int32 words:                                                                                                      4 bytes
 *   - store may be ANY address: twelve bytes leave as three 4-byte words where their own address allows and as single bytes otherwise;
 *     the bytes written are the same at every address.
 *   - table_host is a host array.
 * tests/test_stream_bank_abi_cpu.py holds this as a table.
 */
#ifndef TAD_MI355X_BANK_H
#define TAD_MI355X_BANK_H

#include "tad_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TADB_ABI_VERSION 1

int tadb_abi_version(void);
/* the text of the last error of a tadb_* call on this thread */
const char* tadb_last_error_string(void);

/* ---- ragged ingest: K decoded uint8 frames of K DIFFERENT sizes, packed in one buffer, each resized (cv2 INTER_CUBIC) to S_h x S_w and
 * written to a slot of its own in a frame store -- ONE launch.  A tick of a camera fleet: every camera's newest frame into that
 * camera's ring slot.
 *   src    uint8, src_bytes bytes: frame k is [h_k, w_k, 3] at byte src_off_k, a multiple of 4.  The ALLOCATION behind src must reach
 *          the next multiple of 4 at or above src_bytes: pixels are loaded as the aligned words that hold them, so up to 3 bytes behind
 *          the last frame's last byte are loaded (and shifted out: no byte outside a frame influences a result).  Only read.
 *   store  uint8 [F, S_h, S_w, 3].  Frame k goes to store[slot_k]; no other byte of store is written.
 *   table  int32, n_words words, on the device:
 *     rows   [K][TADB_ROW_WORDS] = {src_off, h, w, slot, hset, vset, flags, 0}.  flags: TADB_SWAP_RB (bit 0) writes source channel 2 to
 *            stored channel 0 and channel 0 to channel 2, so BGR and RGB cameras fill one store of one channel order.
 *     hsets  [n_hsets] horizontal sets of TAD_FR_SET_HEAD + 5 * S_w words, one per distinct w
 *     vsets  [n_vsets] vertical sets of TAD_FR_SET_HEAD + 5 * S_h words, one per distinct h
 *            each set in tad_frame_resize's own format: {in, out, 0, 0}, first[out], k[out][4].
 * Arithmetic: exactly what tad_mi355x.h states for tad_frame_resize under TAD_FR_NONE, bit for bit -- the host states the 11-bit Keys
 * coefficients (not renormalised), the taps first .. first + 3 are clamped to the source on the device, two int32 passes with nothing
 * rounded in between, byte = clip((sum + (1 << 21)) >> 22, 0, 255).  Equal extents (k = {0, 2048, 0, 0}) give the input bytes back.
 *
 * tadb_ingest_plan_check: host-side check of a HOST copy of the table, no launch.  Refused, each naming the argument or the row:
 *   K outside [1, TADB_MAX_FRAMES]; n_hsets or n_vsets outside [1, TADB_MAX_SETS]; S_h or S_w outside [1, 16384]; F < 1;
 *   src_bytes < 1; n_words != K * TADB_ROW_WORDS + n_hsets * (TAD_FR_SET_HEAD + 5 S_w) + n_vsets * (TAD_FR_SET_HEAD + 5 S_h);
 *   per row: h or w outside [1, TADB_MAX_EXTENT]; src_off negative or no multiple of 4; the frame's h * w * 3 bytes not inside
 *   [0, src_bytes); slot outside [0, F); a slot named by two rows; hset / vset outside their sets; a set whose `in` is not the row's
 *   w / h (or whose `out` is not S_w / S_h); flag bits other than TADB_SWAP_RB; word 7 not 0;
 *   per set: first outside [-2, in - 2]; sum |k| above TAD_FR_MAX_ABS_SUM (the int32 passes would overflow).
 * tadb_ingest_frames: ONE launch, no host synchronisation.  The host checks the scalars, the word count and the pointers; the TABLE is
 *   on the device and is not read by the host, so on the device a malformed table is never an address: a row whose extents are outside
 *   [1, TADB_MAX_EXTENT] or whose frame does not lie inside [0, src_bytes) is ignored (nothing is written for it), a slot is clamped
 *   into [0, F), a set index into its sets, every tap into its row's own source. */
/* Alignment: src, table: 4 bytes; store: any address; table_host: a host array. */
#define TADB_ROW_WORDS 8
#define TADB_MAX_FRAMES 4096
#define TADB_MAX_SETS 64 /* per axis, as TAD_FR_MAX_SETS */
#define TADB_MAX_EXTENT 32768
#define TADB_SWAP_RB 1
int tadb_ingest_plan_check(const int32_t* table_host, int64_t n_words, int K, int n_hsets, int n_vsets, int64_t src_bytes, int64_t F,
                           int S_h, int S_w);
int tadb_ingest_frames(const uint8_t* src, int64_t src_bytes, uint8_t* store, int64_t F, const int32_t* table, int64_t n_words, int K,
                       int n_hsets, int n_vsets, int S_h, int S_w, tad_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TAD_MI355X_BANK_H */
