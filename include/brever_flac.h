/* brever_flac.h -- C ABI of libbrever_flac.so: FLAC dataset members decoded on the MI355X (gfx950), one frame per
 * lane. brever_amd/flac_gpu.py drives it; DESIGN.md 5j has the launch sequence and the measurements.
 *
 *   brv_flacdec_index          HOST pointers, no GPU: STREAMINFO and the table of frames of one stream, found
 *                              without entropy-decoding (sync, reserved bits, CRC-8, running number, CRC-16)
 *   brv_flacdec_scratch_elems  int32 elements of scratch that brv_flacdec_decode needs
 *   brv_flacdec_decode         DEVICE pointers: two launches, parse (bit-serial, one lane per frame, integer
 *                              subframes into the scratch) and finish (stereo decorrelation, scaling by
 *                              2^-(bps-1), window crop, scatter into the padded batch with whole-line stores)
 *
 * The host decoder and encoder of include/brever_hip.h (brv_flac_decode, brv_flac_encode16) are untouched: they
 * stay the worker-process path and the path for the streams the index declines (BRV_FLACDEC_NOT_TAKEN).
 *
 * Conventions of the library, those of include/brever_resample.h:
 *   - the library allocates nothing persistent and keeps no process-global state;
 *   - the device call takes the HIP stream to launch on and never synchronises;
 *   - return value: >= 0 ok, < 0 refused / malformed (codes below), > 0 from brv_flacdec_decode a hipError_t;
 *     brv_flacdec_last_error() gives the thread-local message every failing return has set;
 *   - whatever a kernel reads from a job is checked against the extents the call states before it is used as
 *     an index: every read is bounded by the frame's byte length, every write by the block size, the job's
 *     window and out_elems, every loop by the bits that remain in the frame.
 *
 * stream_info: BRV_FLACDEC_INFO_WORDS int64 =
 *   (sample rate, channels, bits per sample, total samples, min block size, max block size,
 *    byte offset of the first frame, blocking strategy: 0 fixed / 1 variable)
 *   total samples is the sum of the frames' block sizes when STREAMINFO says 0 (unknown), and is clipped to
 *   STREAMINFO's count otherwise, like brv_flac_decode; min / max block size are those of the frames found.
 * frames: BRV_FLACDEC_FRAME_WORDS int64 per frame =
 *   (byte offset, byte length, first sample, block size, channel assignment 0-10, sample size in bits,
 *    header bytes including the CRC-8, the coded frame or sample number)
 * jobs: BRV_FLACDEC_JOB_WORDS int64 per job, one frame each =
 *   (byte offset of the frame in `bytes`, byte length, block size, channel assignment, sample size, header bytes,
 *    lo, hi: the window [lo, hi) of the frame's samples to keep, 0 <= lo <= hi <= block size,
 *    index in `out` where sample lo of channel 0 lands, channel stride in `out`, 2 words the library ignores)
 */
#ifndef BREVER_FLAC_H
#define BREVER_FLAC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

#define BRV_FLACDEC_INFO_WORDS 8
#define BRV_FLACDEC_FRAME_WORDS 8
#define BRV_FLACDEC_JOB_WORDS 12

/* negative returns of brv_flacdec_index (and -1: refused argument) */
#define BRV_FLACDEC_NOT_TAKEN (-2)   /* well-formed, not taken by the GPU decoder (more than 24 bits per sample) */
#define BRV_FLACDEC_NOT_FLAC (-10)   /* no fLaC marker, metadata cut short, no STREAMINFO */
#define BRV_FLACDEC_BAD_HEADER (-60) /* sync code, reserved bits, a field against STREAMINFO, or the CRC-8 */
#define BRV_FLACDEC_BAD_CRC16 (-61)  /* the frame's CRC-16 does not match */
#define BRV_FLACDEC_BAD_NUMBER (-62) /* the coded frame / sample number does not continue the sequence */
#define BRV_FLACDEC_TRUNCATED (-63)  /* the stream ends inside the last frame */

/* per-job status words of brv_flacdec_decode (0: decoded) */
#define BRV_FLACDEC_JOB_BAD_FIELDS 1 /* the job's own fields are out of the extents the call states */
#define BRV_FLACDEC_JOB_RESERVED 2   /* a reserved or invalid field in a subframe */
#define BRV_FLACDEC_JOB_OVERRUN 3    /* the frame's bits ran out */
#define BRV_FLACDEC_JOB_LENGTH 4     /* the frame does not end where its byte length says */

int brv_flacdec_version(void);
const char* brv_flacdec_last_error(void);

/* The number of frames of the stream; `frames` gets the first min(count, capacity) of them (capacity == 0 with
 * frames == NULL counts only). stream_info may be NULL. */
int64_t brv_flacdec_index(const uint8_t* data, int64_t size, int64_t* stream_info, int64_t* frames,
                          int64_t capacity);

/* ceil(n_jobs/64) 64 channels max_block int32 elements; 1 <= n_jobs <= 4194240 (65535 x 64), as for the decode. */
int64_t brv_flacdec_scratch_elems(int64_t n_jobs, int64_t channels, int64_t max_block);

/* bytes: bytes_size bytes (a multiple of 4, the base 4-byte aligned) holding every job's frame. channels and
 * max_block: upper bounds of the jobs' channel counts and block sizes (a job beyond them gets status 1).
 * scratch: int32, at least brv_flacdec_scratch_elems(n_jobs, channels, max_block) elements, contents undefined
 * before and after. out: float32, out_elems elements, zero-filled by the caller; only the jobs' windows are
 * written. status: n_jobs int32, written for every job. A job with a non-zero status writes nothing to out. */
int brv_flacdec_decode(const uint8_t* bytes, int64_t bytes_size, const int64_t* jobs, int64_t n_jobs,
                       int64_t channels, int64_t max_block, int32_t* scratch, int64_t scratch_elems, float* out,
                       int64_t out_elems, int32_t* status, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
