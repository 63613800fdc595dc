/* brever_mix.h -- C ABI of libbrever_mix.so: the MI355X (gfx950) kernels of the batched mixture engine
 * (brever_amd/mixture.py), which replaces brever/mixture/mixture.py (Mixture, split_brir, spatialize,
 * adjust_snr, adjust_rms) for a batch of ragged mixtures.
 *
 * A library of its own next to libbrever_hip.so, with the same conventions (include/brever_hip.h):
 *   - every pointer is a device pointer borrowed from the caller; the library allocates nothing and keeps
 *     no process-global state;
 *   - every call takes the HIP stream to launch on and never synchronises;
 *   - return value: 0 ok, -1 refused argument, -2 unsupported configuration, > 0 a hipError_t;
 *     brv_mix_last_error() gives the thread-local message every non-zero return has set.
 *
 * The long convolutions are uniformly partitioned overlap-save products with block B: the block DFTs (size
 * 2B, bins = B + 1) are brv_dft64_forward / brv_dft64_synthesis of the main library; spectra are complex64
 * (rows, bins, frames), frames contiguous, exactly as those two store and read them. Everything the kernels
 * index with comes from small descriptor arrays on the device, so a batch is drawn without a host round
 * trip; every descriptor is range-checked in the kernel (an entry out of range is skipped, never followed).
 */
#ifndef BREVER_MIX_H
#define BREVER_MIX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

int brv_mix_version(void);
const char* brv_mix_last_error(void);

#define BRV_MIX_ENERGY_CHUNK 2048    /* samples per partial sum of brv_mix_energies */
#define BRV_MIX_MAX_PARTS 512        /* partitions per impulse response the LDS tile of brv_mix_partition_mac holds */

/* rows (nrows, row_len): row r = zeros, with pool[src, src + n) at [dst, dst + n).
 * desc (nrows, 3) int64 = (src, n, dst); pool_len bounds src + n. */
int brv_mix_pack_signals(const float* pool, const int64_t* desc, float* rows, int64_t pool_len,
                         int64_t nrows, int64_t row_len, brv_stream_t stream);

/* split_brir + the ear-planar layout of the partition transform. rows (2 jobs, row_len): rows 2j and 2j + 1
 * are the left and right ear of job j, zeros behind its taps. desc (jobs, 3) int64 = (offset in floats of an
 * interleaved (taps, 2) BRIR in pool, taps, mode); mode 0 copies, 1 keeps the early window of each ear
 * (t < peak + boundary, the weaker ear's peak searched within max_delay of the stronger one's), 2 the rest. */
int brv_mix_pack_brirs(const float* pool, const int64_t* desc, float* rows, int64_t pool_len, int64_t jobs,
                       int64_t row_len, int64_t boundary, int64_t max_delay, brv_stream_t stream);

/* Per-bin partition multiply-accumulate, both ears: for slot s and its jobs j in [begin, end), in that order,
 *   Y[2s + ear][k][f] = sum_j sum_{p < parts_j} X[x_row_j][k][f - p] * H[h_row_j + ear][k][p],  f < frames_s
 * (p ascending, fp32 fused multiply-adds, one accumulator: a slot's result does not depend on the batch around
 * it); frames in [frames_s, yframes) are written as zeros. slots (nslots, 3) int32 = (begin, end, frames);
 * jobs (njobs, 3) int32 = (x_row, h_row, parts). max_parts >= every parts_j sizes the LDS tile (<= 512). */
int brv_mix_partition_mac(const float* xspec, const float* hspec, float* yspec, const int32_t* slots,
                          const int32_t* jobs, int64_t nslots, int64_t njobs, int64_t xrows, int64_t xframes,
                          int64_t hrows, int64_t hparts, int64_t bins, int64_t yframes, int64_t max_parts,
                          brv_stream_t stream);

/* Energy sums of a batch in fp64. y (8 mixtures, row_len): row 8m + 2c + ear, c = early_speech, late_speech,
 * dir_noise, diffuse. mix (mixtures, 4) int32 = (length, speech_end, idx0, idx1): samples >= length do not
 * exist, the two speech components are zero from speech_end on (the reference truncates before it pads again).
 * partials (mixtures, chunks, 40): per chunk of 2048 samples the four 4 x 4 Gram matrices (upper triangle, 10
 * each) of: the channel means over [idx0, idx1), the channel means, the left ear, the right ear. */
int brv_mix_energies(const float* y, const int32_t* mix, double* partials, int64_t mixtures, int64_t row_len,
                     int64_t chunks, brv_stream_t stream);

/* set_ndr, set_snr, set_tmr, set_rms(get_rms() + jitter) and the long-term labels from the sums above.
 * params (mixtures, 4) double = (ndr, snr, tmr, rms_jitter), NaN = step not taken. gains (mixtures, 8) double =
 * the factors of (early, late, dir, diffuse), then the reference's (ndr, snr, tmr, rms) gains; labels
 * (mixtures, 3) = (tmr, tnr, trr); status (mixtures) int32 = 0, 1 "target signal is 0", 2 "noise equals 0". */
int brv_mix_gains(const double* partials, const int32_t* mix, const double* params, double* gains,
                  double* labels, int32_t* status, int64_t mixtures, int64_t chunks, brv_stream_t stream);

/* out (ncomp, mixtures, out_len, 2) = the requested components with the gains applied, zeros behind each
 * mixture's length. comps (ncomp) int32: 0 mixture, 1 foreground, 2 background, 3 speech, 4 noise,
 * 5 early_speech, 6 late_speech, 7 dir_noise, 8 diffuse. */
int brv_mix_compose(const float* y, const double* gains, const int32_t* mix, const int32_t* comps, float* out,
                    int64_t ncomp, int64_t mixtures, int64_t row_len, int64_t out_len, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
