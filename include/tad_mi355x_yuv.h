/*
 * tad_mi355x_yuv.h -- the YUV-INGEST ABI: the seventh surface of this package, tady_*, TADY_ABI_VERSION 1, in a shared library of its
 * own, libtad_mi355x_yuv.so (csrc/yuv_ingest.hip).  The six older surfaces are held where they are, each from a pinned source list, so
 * what feeding a bank of camera streams with 4:2:0 YUV surfaces adds is linked apart, the way the stream-bank library was.  The library
 * is self-contained: it is compiled with hidden visibility, exports these entry points and nothing else, and keeps an error text of its
 * own behind tady_last_error_string().
 *
 * Every other convention is the core header's: plain C, device pointers and explicit sizes, `stream` a hipStream_t passed as void*,
 * 0 or a negative TAD_E* code, no allocation, no synchronisation, every check made on the host before anything is launched.  Nothing
 * here takes a workspace and nothing uses atomics or talks across workgroups: two calls give the same bits.
 *
 * Pointer alignment (refused with TAD_EINVAL and "<entry point>: <argument> is misaligned: it must be N-byte aligned"):
 *   - src is read as the aligned 4-byte words that hold the samples asked for; planes may start at ANY byte offset inside it:     4 bytes
 *   - table holds int32 words:                                                                                                   4 bytes
 *   - store may be ANY address: twelve bytes leave as three 4-byte words where their own address allows and as single bytes otherwise;
 *     the bytes written are the same at every address.
 *   - table_host is a host array.
 * tests/test_yuv_abi_cpu.py holds this as a table.
 */
#ifndef TAD_MI355X_YUV_H
#define TAD_MI355X_YUV_H

#include "tad_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TADY_ABI_VERSION 1

int tady_abi_version(void);
/* the text of the last error of a tady_* call on this thread */
const char* tady_last_error_string(void);

/* ---- YUV ingest: K pitched 4:2:0 YUV frames (NV12, NV21, I420 -- any mix) of K DIFFERENT sizes, packed in one buffer, each converted to
 * 8-bit RGB, resized (cv2 INTER_CUBIC) to S_h x S_w and written to a slot of its own in a frame store -- ONE launch, no RGB frame in
 * memory in between.
 *   src    uint8, src_bytes bytes, holding every plane of every frame.  The ALLOCATION behind src must reach the next multiple of 4 at or
 *          above src_bytes: samples are loaded as the aligned words that hold them, so no load begins in front of src and none ends
 *          behind src_bytes rounded up to 4.  Only read.
 *   store  uint8 [F, S_h, S_w, 3].  Frame k goes to store[slot_k]; no other byte of store is written.
 *   table  int32, n_words words, on the device:
 *     rows   [K][TADY_ROW_WORDS] = {y_off, y_pitch, u_off, v_off, c_pitch, c_step, h, w, slot, hset, vset, cset, flags, 0, 0, 0}.
 *            Offsets and pitches in bytes.  Luma sample (y, x) is the byte y_off + y * y_pitch + x; the chroma pair of luma sample
 *            (y, x) is chroma sample (y >> 1, x >> 1) (nearest: no chroma interpolation), U the byte u_off + (y >> 1) * c_pitch +
 *            (x >> 1) * c_step and V the byte v_off + the same.  The chroma planes have (h + 1) / 2 rows of (w + 1) / 2 samples: odd
 *            extents are legal.  c_step is 2 for interleaved chroma and 1 for planar:
 *              NV12  u_off = the chroma plane, v_off = u_off + 1, c_step 2        NV21  v_off = the chroma plane, u_off = v_off + 1
 *              I420  u_off and v_off two planes of their own, c_step 1 (YV12: the two exchanged)
 *            Of a plane row only its live bytes are read for a result -- w of a luma row, ((w + 1) / 2) * c_step of a chroma row: no
 *            byte of the pitch padding, of a gap between planes or of a neighbouring frame influences any result.
 *            flags: TADY_BGR (bit 0) writes B to stored channel 0 and R to channel 2, so YUV cameras can fill a BGR store.
 *     hsets  [n_hsets] horizontal sets of TAD_FR_SET_HEAD + 5 * S_w words, one per distinct w
 *     vsets  [n_vsets] vertical sets of TAD_FR_SET_HEAD + 5 * S_h words, one per distinct h
 *            each set in tad_frame_resize's own format: {in, out, 0, 0}, first[out], k[out][4].
 *     csets  [n_csets] colour sets of TADY_CSET_WORDS words {y_off, cy, cvr, cug, cvg, cub, 0, 0}: 20-bit fixed point.
 *
 * Arithmetic, all of it int32 (`>>` is the arithmetic, floor, shift), so the bits do not depend on the compiler:
 *   colour   of luma sample Y and its chroma pair U, V under the row's colour set
 *              yy = max(0, Y - y_off) * cy
 *              R = clip((yy + cvr * (V - 128)                   + (1 << 19)) >> 20, 0, 255)
 *              G = clip((yy + cvg * (V - 128) + cug * (U - 128) + (1 << 19)) >> 20, 0, 255)
 *              B = clip((yy + cub * (U - 128)                   + (1 << 19)) >> 20, 0, 255)
 *            The HOST states the sets, as it states the cubic coefficients: the kernel knows no colour standard.  With {16, 1220542,
 *            1673527, -409993, -852492, 2116026} the formula is the one OpenCV's 8-bit COLOR_YUV2RGB_NV12 documents for BT.601 limited
 *            range; that is a citation, not an oracle: THE CONTRACT IS THE FORMULA ABOVE AS WRITTEN HERE, not the bytes of any OpenCV
 *            build (the core header says the same of the cubic resize).
 *   resize   the converted 8-bit pixel enters exactly what tad_mi355x_bank.h states for tadb_ingest_frames: host-stated taps and 11-bit
 *            coefficients, taps first .. first + 3 clamped to the source on the device, two int32 passes with nothing rounded in
 *            between, byte = clip((sum + (1 << 21)) >> 22, 0, 255).
 *   So the result is, bit for bit, tadb_ingest_frames applied to the frame converted whole by the formula; equal extents
 *   (k = {0, 2048, 0, 0}) give the converted bytes back.
 *
 * tady_ingest_plan_check: host-side check of a HOST copy of the table, no launch.  Refused, each naming the argument or the row:
 *   K outside [1, TADY_MAX_FRAMES]; n_hsets or n_vsets outside [1, TADY_MAX_SETS]; n_csets outside [1, TADY_MAX_CSETS]; S_h or S_w
 *   outside [1, 16384]; F < 1; src_bytes < 1; n_words != K * TADY_ROW_WORDS + n_hsets * (TAD_FR_SET_HEAD + 5 S_w) + n_vsets *
 *   (TAD_FR_SET_HEAD + 5 S_h) + n_csets * TADY_CSET_WORDS;
 *   per row: h or w outside [1, TADY_MAX_EXTENT]; c_step not 1 or 2; y_pitch below w; c_pitch below ((w + 1) / 2) * c_step; the luma
 *   plane, the U plane or the V plane not inside [0, src_bytes); with c_step 2, u_off and v_off not next to each other; slot outside
 *   [0, F); a slot named by two rows; hset / vset / cset outside their sets; a set whose `in` is not the row's w / h (or whose `out` is
 *   not S_w / S_h); flag bits other than TADY_BGR; one of the last three words not 0;
 *   per resize set: first outside [-2, in - 2]; sum |k| above TAD_FR_MAX_ABS_SUM (the int32 passes would overflow);
 *   per colour set: y_off outside [0, 255]; cy negative; 255 * cy + 128 * max(|cvr|, |cub|, |cug| + |cvg|) + (1 << 19) reaching 2^31
 *   (the int32 sums would overflow); one of the last two words not 0.
 * tady_ingest_yuv: ONE launch, no host synchronisation.  The host checks the scalars, the word count and the pointers; the TABLE is on
 *   the device and is not read by the host, so on the device a malformed table is never an address: a row whose extents are outside
 *   [1, TADY_MAX_EXTENT], whose c_step is not 1 or 2, one of whose pitches is below its row's live bytes, or one of whose three planes
 *   does not lie inside [0, src_bytes) is ignored (nothing is written for it); a slot is clamped into [0, F), a set index into its
 *   sets, every tap into its row's own planes. */
/* Alignment: src, table: 4 bytes; store: any address; table_host: a host array. */
#define TADY_ROW_WORDS 16
#define TADY_CSET_WORDS 8
#define TADY_MAX_FRAMES 4096
#define TADY_MAX_SETS 64  /* per axis, as TAD_FR_MAX_SETS */
#define TADY_MAX_CSETS 16
#define TADY_MAX_EXTENT 32768
#define TADY_BGR 1
int tady_ingest_plan_check(const int32_t* table_host, int64_t n_words, int K, int n_hsets, int n_vsets, int n_csets, int64_t src_bytes,
                           int64_t F, int S_h, int S_w);
int tady_ingest_yuv(const uint8_t* src, int64_t src_bytes, uint8_t* store, int64_t F, const int32_t* table, int64_t n_words, int K,
                    int n_hsets, int n_vsets, int n_csets, int S_h, int S_w, tad_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TAD_MI355X_YUV_H */
