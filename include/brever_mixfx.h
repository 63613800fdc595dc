/* brever_mixfx.h -- C ABI of libbrever_mixfx.so: the MI355X (gfx950) kernels behind the signal effects of the
 * batched mixture engine (brever_amd/mixture.py): colored_noise, match_ltas / calc_ltas and BRIRDecay of
 * brever/mixture/mixture.py.
 *
 * A library of its own next to libbrever_mix.so, with the same conventions (include/brever_mix.h):
 *   - every pointer is a device pointer borrowed from the caller; the library allocates nothing and keeps
 *     no process-global state;
 *   - every call takes the HIP stream to launch on and never synchronises;
 *   - return value: 0 ok, -1 refused argument, -2 unsupported configuration, > 0 a hipError_t;
 *     brv_mixfx_last_error() gives the thread-local message every non-zero return has set.
 *
 * The transforms around these kernels are brv_dft64_forward / brv_dft64_synthesis / brv_overlap_add of the
 * main library and brv_mix_partition_mac of libbrever_mix.so; spectra are complex64 (rows, bins, frames), frames
 * contiguous. Every descriptor is range-checked in the kernel: an entry out of range is skipped, never
 * followed. Every reduction runs in fp64 in an order fixed by the signal's own length.
 */
#ifndef BREVER_MIXFX_H
#define BREVER_MIXFX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

int brv_mixfx_version(void);
const char* brv_mixfx_last_error(void);

/* The periodic extension a circular convolution of length m is computed from. rows (nrows, row_len): row r =
 * pool[src, src + m) twice, zeros behind. desc (nrows, 2) int64 = (src, m); pool_len bounds src + m. */
int brv_mixfx_pack_periodic(const float* pool, const int64_t* desc, float* rows, int64_t pool_len,
                            int64_t nrows, int64_t row_len, brv_stream_t stream);

/* Masked row copy. desc (ncopies, 5) int64 = (src_row, src_off, n, dst_off, span): dst[dst_off + i] =
 * src[src_row][src_off + i] for i < n and 0 for n <= i < span. src is (src_rows, src_row_len); dst_len bounds
 * dst_off + span. */
int brv_mixfx_copy_rows(const float* src, const int64_t* desc, float* dst, int64_t ncopies, int64_t src_rows,
                        int64_t src_row_len, int64_t dst_len, brv_stream_t stream);

/* Long-term average spectrum of each signal: power (nsig, bins) double = the mean of |X|^2 over the signal's
 * rows and its first `frames_s` frames. desc (nsig, 3) int32 = (first row, rows (1 or 2), frames_s). */
int brv_mixfx_ltas_power(const float* spec, const int32_t* desc, double* power, int64_t nsig, int64_t rows,
                         int64_t bins, int64_t frames, brv_stream_t stream);

/* In place X[row][k][f] *= sqrt(ltas[k] / power[s][k]) for the rows and frames of signal s (desc as above);
 * a bin of zero power is zeroed. ltas (bins) double. */
int brv_mixfx_ltas_equalize(float* spec, const int32_t* desc, const double* power, const double* ltas,
                            int64_t nsig, int64_t rows, int64_t bins, int64_t frames, brv_stream_t stream);

/* BRIRDecay, one workgroup per job. desc (jobs, 8) int64 = (offset in floats of an interleaved (taps, 2) BRIR
 * in brir_pool, taps, offset of the tail noise in noise_pool, noise samples there, offset in floats of the
 * interleaved (n, 2) result in out, n, round(delay fs), claimed tail length or -1). params (jobs, 3) double =
 * (rt60, drr, fs). With i0 = round(delay fs) + the smaller of the ears' first-maximum |h| indices:
 *   out = h padded to n + sqrt(10^(-drr/10) sum(mean over ears of h)^2 / sum tail^2) tail,
 *   tail[i] = exp(-(i - i0)/fs/rt60 3 ln 10) noise[i - i0], i >= i0, the same in both ears.
 * status (jobs) int32 = 0, 1 zero BRIR energy, 2 zero tail energy (the padded BRIR is written), 3 the claimed
 * tail length is not n - i0 or the noise holds fewer samples, 4 a descriptor out of range (3, 4: nothing is
 * written). */
int brv_mixfx_decay_brirs(const float* brir_pool, const float* noise_pool, const int64_t* desc,
                          const double* params, float* out, int32_t* status, int64_t brir_len,
                          int64_t noise_len, int64_t out_len, int64_t jobs, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
