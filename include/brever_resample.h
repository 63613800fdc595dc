/* brever_resample.h -- C ABI of libbrever_resample.so: exact Fourier resampling (brever/io.py resample, which is
 * scipy.signal.resample: a length-N real DFT, the lowest min(N, M)//2 + 1 bins kept, a length-M inverse) on the
 * MI355X (gfx950) for a ragged batch of real signals, in fp64. brever_amd/io.py drives it.
 *
 * N and M are arbitrary, so both transforms are Bluestein chirp transforms: a circular convolution of length
 * L = fft_len, a power of two, computed with hand-written transforms (a four-step decomposition whose short
 * transforms run in LDS). All signals of one L go through the same launches.
 *
 * Conventions, those of include/brever_mixfx.h:
 *   - every pointer is a device pointer borrowed from the caller; the library allocates nothing and keeps
 *     no process-global state;
 *   - every call takes the HIP stream to launch on and never synchronises;
 *   - return value: 0 ok, -1 refused argument, -2 unsupported configuration, > 0 a hipError_t;
 *     brv_rs_last_error() gives the thread-local message every non-zero return has set;
 *   - every descriptor is range-checked in the kernel: a column whose descriptor points outside the operand it
 *     names, or names another fft_len, is skipped, never followed.
 * The result of a column depends on its own (N, M, L) only: no reduction crosses columns, there are no atomics.
 *
 * Shared operands:
 *   tw    (2048, 2) double: exp(-2 pi i j/4096), j < 2048, the butterfly factors of the LDS transforms.
 *   slab  (nslots, fft_len, 2) double: chirp spectra, one slot each (brv_rs_chirp_spectra).
 *   work  (ncols, fft_len, 2) double: scratch, row c belongs to column c of the call.
 *   desc  (ncols, 8) int64 = (x_off, x_stride, N, M, out_off, out_stride, slot, L): sample i of the column is
 *         x[x_off + i x_stride], result sample i goes to out[out_off + i out_stride]; `slot` is the slab slot of
 *         the chirp spectrum the call needs (analysis: kind 0 of N; synthesis: kind 1 of M); L must equal fft_len
 *         and be at least max(N, M) + min(N, M)/2 (brv_rs_fft_length(N, M) is the smallest such).
 */
#ifndef BREVER_RESAMPLE_H
#define BREVER_RESAMPLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

int brv_rs_version(void);
const char* brv_rs_last_error(void);

#define BRV_RS_MAX_COLUMNS 32768     /* the most columns (count, ncols) one call takes */

/* The longest input (and output) in samples: 2^22. */
int64_t brv_rs_max_length(void);

/* The convolution length L of a column of n input and m output samples: the power of two, at least 16, not below
 * max(n, m) + min(n, m)/2. -1 with a message that names the limit when n or m is < 1 or beyond
 * brv_rs_max_length(). */
int64_t brv_rs_fft_length(int64_t n, int64_t m);

/* Chirp spectra into slab slots. desc (count, 3) int64 = (slot, n, kind). Slot `slot` receives the forward
 * transform (in the library's own bin order) of b[j], j < fft_len:
 *   kind 0 (analysis of n input samples):  b[j] = exp(+i pi j^2/n) for j <= fft_len - n, else exp(+i pi (fft_len - j)^2/n)
 *   kind 1 (synthesis of n output samples): b[j] = exp(-i pi j^2/n) for j < n,            else exp(-i pi (fft_len - j)^2/n)
 * with j^2 reduced modulo 2n in 64-bit integers before the sine and cosine are taken. */
int brv_rs_chirp_spectra(double* slab, const int64_t* desc, const double* tw, int64_t nslots, int64_t fft_len,
                         int64_t count, brv_stream_t stream);

/* First half: work[c] = the min(N, M)//2 + 1 lowest bins of the N-point DFT of column c, weighted for the
 * M-point inverse (the Nyquist rule of scipy.signal.resample, 1/N) and multiplied by the synthesis chirp; zeros
 * behind. x is float (x_float32 != 0) or double, x_len elements. */
int brv_rs_analysis(const void* x, const int64_t* desc, const double* slab, const double* tw, double* work,
                    int64_t x_len, int64_t x_float32, int64_t nslots, int64_t fft_len, int64_t ncols,
                    brv_stream_t stream);

/* Second half: the M output samples of column c from work[c], to out (float when out_float32 != 0, else double;
 * out_len elements). work is overwritten. */
int brv_rs_synthesis(double* work, const int64_t* desc, const double* slab, const double* tw, void* out,
                     int64_t out_len, int64_t out_float32, int64_t nslots, int64_t fft_len, int64_t ncols,
                     brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
