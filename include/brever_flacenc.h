/* brever_flacenc.h -- C ABI of libbrever_flacenc.so: a padded device batch of signals encoded as FLAC streams of
 * RFC 9639 on the MI355X (gfx950), one workgroup per frame. brever_amd/flac_enc.py drives it; DESIGN.md 5l has the
 * launch sequence, the search space with its order of ties, and the measurements.
 *
 *   brv_flacenc_frame_capacity  bytes the image of one frame takes in the scratch (a multiple of 256)
 *   brv_flacenc_scratch_elems   int32 elements of scratch that brv_flacenc_encode needs
 *   brv_flacenc_out_capacity    bytes of `out` that hold the streams of any batch of the stated extents
 *   brv_flacenc_encode          DEVICE pointers: a memset of the status words and three launches -- frames (quantise,
 *                               choose, write the bits and both CRCs of every frame into its image), layout (frame
 *                               and row offsets, STREAMINFO), pack (the frames of a row behind its header)
 *
 * The host encoder of include/brever_hip.h (brv_flac_encode16: mono, 16 bits, FIXED predictors) is untouched.
 *
 * Conventions of the library, those of include/brever_flac.h:
 *   - the library allocates nothing persistent and keeps no process-global state;
 *   - the device call takes the HIP stream to launch on and never synchronises;
 *   - return value: >= 0 ok, < 0 refused (-1), > 0 from brv_flacenc_encode a hipError_t;
 *     brv_flacenc_last_error() gives the thread-local message every failing return has set;
 *   - every index a kernel derives from its inputs (the rows' lengths, the frames' lengths it wrote itself) is
 *     checked against the extents the call states before it is used.
 *
 * Input: x is (rows, channels, max_len), float32 (pcm == 0), quantised as
 * clip(rint(x 2^(bps-1)), -2^(bps-1), 2^(bps-1) - 1) with round half to even, or int32 (pcm != 0) already in that
 * range. lengths: rows int64 on the device, 1 ... max_len each; samples behind a row's length are not read.
 *
 * Output: table, 3 rows + 1 int64 on the device =
 *   offsets[rows + 1]  byte offset of each row's stream in `out` (a multiple of 4); the last is the end of all
 *   sizes[rows]        bytes of the row's stream, 0 for a row with a status
 *   status[rows]       0, or the OR of the BRV_FLACENC_ROW_* bits: such a row yields no stream
 * A stream is 'fLaC', STREAMINFO (the nominal block size twice, the frames' least and largest byte size, rate,
 * channels, bits, total samples, an all-zero MD5) and the frames: fixed blocking, the last frame may be shorter.
 */
#ifndef BREVER_FLACENC_H
#define BREVER_FLACENC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

#define BRV_FLACENC_ROW_NONFINITE 1  /* a NaN or an infinity among the row's float samples */
#define BRV_FLACENC_ROW_RANGE 2      /* an int32 sample outside [-2^(bps-1), 2^(bps-1) - 1] */
#define BRV_FLACENC_ROW_LENGTH 4     /* the row's length is not 1 ... max_len */
#define BRV_FLACENC_ROW_INTERNAL 8   /* a frame did not fit its image (the capacity query excludes this) */

#define BRV_FLACENC_MAX_LPC_ORDER 32
#define BRV_FLACENC_MAX_ROWS 65535

int brv_flacenc_version(void);
const char* brv_flacenc_last_error(void);

/* channels 1 or 2, bits_per_sample 16 or 24, 16 <= block_size <= 65535 (as for every call below) */
int64_t brv_flacenc_frame_capacity(int64_t channels, int64_t bits_per_sample, int64_t block_size);

/* 1 <= rows <= 65535, 1 <= max_len <= 2^30, rows ceil(max_len/block_size) <= 2^30 */
int64_t brv_flacenc_scratch_elems(int64_t rows, int64_t channels, int64_t max_len, int64_t bits_per_sample,
                                  int64_t block_size);
int64_t brv_flacenc_out_capacity(int64_t rows, int64_t channels, int64_t max_len, int64_t bits_per_sample,
                                 int64_t block_size);

/* scratch: int32, 256-byte aligned, at least brv_flacenc_scratch_elems(...) elements, contents undefined before and
 * after. out: 4-byte aligned, out_capacity >= brv_flacenc_out_capacity(...) bytes; only the bytes below
 * offsets[rows] are written. 1 <= sample_rate <= 655350, 0 <= lpc_order <= 32 (0: no LPC candidates). */
int brv_flacenc_encode(const void* x, int64_t pcm, const int64_t* lengths, int64_t rows, int64_t channels,
                       int64_t max_len, int64_t sample_rate, int64_t bits_per_sample, int64_t block_size,
                       int64_t lpc_order, int32_t* scratch, int64_t scratch_elems, uint8_t* out,
                       int64_t out_capacity, int64_t* table, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
