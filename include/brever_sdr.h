/* brever_sdr.h -- C ABI of libbrever_sdr.so: the BSS-eval signal-to-distortion ratio (Vincent et al. 2006) with an
 * allowed distortion filter of `filter_length` taps, as a metric and as a differentiable criterion, on the MI355X
 * (gfx950). brever_amd/sdr.py runs it; DESIGN.md 5k states the definition.
 *
 * Per row, with s = the reference y, x = the estimate and T = min(max(lengths[row], 0), stride):
 *   r[k] = sum_t s[t] s[t + k],  b[k] = sum_t s[t] x[t + k]   for k < L (both indices in [0, T); 0 from k = T on)
 *   R = Toeplitz(r) + load_diag r[0] I,  R h = b,  q = b^T h,  E = sum_t x[t]^2
 *   SDR = 10 log10( max(q, eps E) / max(E - q, eps E) ),  eps = 2^-52
 * Inputs are fp32; every sum, the solve, q and E are fp64.
 *
 *   brv_sdr_forward    three launches: the lags of every chunk of brv_sdr_chunk() samples (fp64 vector FMAs on
 *                      8 x 8 register tiles, the chunk and its halo staged in LDS), then per row the sum of the
 *                      chunks in ascending order, the Levinson recursion on r (one workgroup, state in LDS), q, SDR
 *   brv_sdr_backward   gradient of -SDR with respect to x: s through h (FIR, both staged in LDS) fused with
 *                      -(10/ln 10) (2 s_target/q - 2 (x - s_target)/(E - q)), a term whose floor is active dropped
 *
 * Every reduction runs in a fixed order and there are no atomics: results are bitwise repeatable, and a row gives
 * the same bits alone as in a batch of any width.
 *
 * flags (one int32 per row):
 *   1   r[0] is not positive (degenerate)        8   the floor of the numerator is active (q < eps E)
 *   2   E is not positive (degenerate)          16   the floor of the denominator is active (E - q < eps E)
 *   4   a pivot of the recursion is not positive (degenerate)
 * A degenerate row has sdr = NaN, h = 0, q = 0 and a gradient of exact zeros.
 *
 * Conventions of the library, those of include/brever_resample.h:
 *   - every pointer is a device pointer borrowed from the caller; the library allocates nothing and keeps
 *     no process-global state;
 *   - every call takes the HIP stream to launch on and never synchronises;
 *   - return value: 0 ok, -1 refused argument, > 0 a hipError_t; brv_sdr_last_error() gives the thread-local
 *     message every non-zero return has set;
 *   - lengths are clamped to [0, stride] before they are used.
 */
#ifndef BREVER_SDR_H
#define BREVER_SDR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

int brv_sdr_version(void);
const char* brv_sdr_last_error(void);

#define BRV_SDR_MAX_FILTER_LENGTH 512
#define BRV_SDR_CHUNK 2048
/* the bits of a row's flags word (the table above) */
#define BRV_SDR_FLAG_NO_REFERENCE 1
#define BRV_SDR_FLAG_NO_ESTIMATE 2
#define BRV_SDR_FLAG_BAD_PIVOT 4
#define BRV_SDR_FLAG_NUMERATOR_FLOOR 8
#define BRV_SDR_FLAG_DENOMINATOR_FLOOR 16

/* the largest filter_length the kernels take (512) and the chunk length of the correlation kernel (2048) */
int64_t brv_sdr_max_filter_length(void);
int64_t brv_sdr_chunk(void);

/* bytes of `workspace` for brv_sdr_forward (the per-chunk partial lags); -1 for arguments the forward refuses */
int64_t brv_sdr_workspace_bytes(int64_t rows, int64_t stride, int64_t filter_length);

/* x, y (rows, stride) float; lengths (rows) int64. Writes sdr (rows), h (rows, filter_length), q (rows), e (rows)
 * double and flags (rows) int32. load_diag travels as a float (the header parser of the binding takes no double):
 * its fp32 value, widened, is the loading that enters R. */
int brv_sdr_forward(const float* x, const float* y, const int64_t* lengths, int64_t rows, int64_t stride,
                    int64_t filter_length, float load_diag, void* workspace, double* sdr, double* h, double* q,
                    double* e, int32_t* flags, brv_stream_t stream);

/* dx (rows, stride) float: grad_rows[row] times the gradient of MINUS the row's SDR with respect to x for
 * t < lengths[row], 0 at and beyond it; h, q, e, flags as brv_sdr_forward left them for the same x, y, lengths. */
int brv_sdr_backward(const float* x, const float* y, const int64_t* lengths, const double* h, const double* q,
                     const double* e, const int32_t* flags, const double* grad_rows, int64_t rows, int64_t stride,
                     int64_t filter_length, float* dx, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
