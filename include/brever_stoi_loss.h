/* brever_stoi_loss.h -- C ABI of libbrever_stoi_loss.so: the backward pass of the STOI / ESTOI training criteria
 * (brever_amd/criterion.py StoiLoss / EstoiLoss) on the MI355X (gfx950). The forward is the metric's own
 * (include/brever_hip.h: brv_resample_poly, brv_stoi_compact, brv_gemm_f32, brv_stoi_bands, brv_stoi_correlate);
 * brever_amd/stoi.py runs it and keeps `kept`, `geom`, the estimate's spectrum and both band tensors for the
 * launches below, which go back from the per-row upstream gradient to the gradient of the estimate:
 *
 *   brv_sl_segment_backward    gradient of every 30-frame segment with respect to the estimate's band tile
 *   brv_sl_bands_backward      sum of the segment tiles per (band, frame), then through the band magnitude
 *   (frame gradient = spectrum gradient x basis^T: one brv_gemm_f32 with trans_b = 1, by the caller)
 *   brv_sl_fold_frames         adjoint of cutting the compacted signal into 256-sample frames 128 apart
 *   brv_sl_compact_backward    adjoint of the overlap-add of the kept Hann frames
 *   brv_sl_resample_backward   adjoint of brv_resample_poly
 *
 * Only the estimate gets a gradient: frame selection, the target's band magnitudes and its normalised segments
 * are constants. Every stage is a gather: an output element is one lane's sum over its own row's data in a fixed
 * order, so there are no atomics and the result is bitwise repeatable.
 *
 * Conventions of the derivative:
 *   - d sqrt(s)/ds at s = 0 is taken as 0 (band magnitudes; segment norms of STOI; row and column norms of ESTOI);
 *   - STOI's clip min(y scale, x (1 + clip)) passes gradient to y scale where y scale <= x (1 + clip) and none
 *     elsewhere; the scale's dependence on the estimate's norm does pass gradient;
 *   - a row with no segment (geom says fewer than 30 frames are left) gets a gradient of exact zeros.
 *
 * Conventions of the library, those of include/brever_resample.h:
 *   - every pointer is a device pointer borrowed from the caller; the library allocates nothing and keeps
 *     no process-global state;
 *   - every call takes the HIP stream to launch on and never synchronises;
 *   - return value: 0 ok, -1 refused argument, > 0 a hipError_t; brv_sl_last_error() gives the thread-local
 *     message every non-zero return has set;
 *   - what a kernel reads from geom and kept is clamped to the extents the call states before it is used as an
 *     index.
 *
 * Shared operands (rows = items x middle axes, each row on its own):
 *   geom  (rows, 4) int32 = (samples, frames, segments, kept frames) after silent-frame removal, of brv_stoi_compact.
 *   kept  (rows, nf_max) int32: the kept frames of a row in ascending order, of brv_stoi_compact.
 *   tob   (rows, 15, nf_max) float: band magnitudes of brv_stoi_bands.
 *   spec  (rows, nf_max, ncols) float: (re, im) interleaved for the bins [bin0, bin0 + ncols/2).
 */
#ifndef BREVER_STOI_LOSS_H
#define BREVER_STOI_LOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

int brv_sl_version(void);
const char* brv_sl_last_error(void);

/* seg_grad (rows, nseg_max, 15, 30), nseg_max = max(nf_max - 29, 1): tile s of row r = grad_rows[r] times the
 * derivative of MINUS the row's STOI (extended == 0, clip = 10^(15/20)) or ESTOI (extended == 1) through segment
 * s with respect to tob_proc[r][:, s : s + 30]; the mean over segments (and bands) is folded in. Tiles at and
 * beyond the row's segment count are not written and not read by brv_sl_bands_backward. */
int brv_sl_segment_backward(const float* tob_clean, const float* tob_proc, const int32_t* geom,
                            const float* grad_rows, float* seg_grad, int64_t rows, int64_t nf_max, int extended,
                            float clip, brv_stream_t stream);

/* band_grad (rows, 15, nf_max): the sum over the <= 30 segments s that hold frame f, in ascending s, of
 * seg_grad[r][s][band][f - s], divided by tob_proc (0 where tob_proc == 0). spec_grad (rows, nf_max, ncols):
 * (re, im) of a bin times the band_grad of the bands that hold the bin, in ascending band; bins in no band get 0.
 * edges (15, 2) int32: the bins [lo, hi) of a band. */
int brv_sl_bands_backward(const float* seg_grad, const float* tob_proc, const float* spec, const int32_t* edges,
                          const int32_t* geom, float* band_grad, float* spec_grad, int64_t rows, int64_t nf_max,
                          int64_t ncols, int64_t bin0, brv_stream_t stream);

/* comp_grad (rows, comp_stride): position p = the sum of frame_grad[r][f][p - 128 f] over the <= 2 frames
 * f < geom frames that cover p, in ascending f; 0 where none does. frame_grad (rows, nf_max, 256). */
int brv_sl_fold_frames(const float* frame_grad, const int32_t* geom, float* comp_grad, int64_t rows,
                       int64_t nf_max, int64_t comp_stride, brv_stream_t stream);

/* dx (rows, stride): sample n < lengths[r] = the sum over the <= 2 kept frames that cover it, in ascending
 * frame, of the Hann weight times comp_grad at the sample's place in the compacted signal (the frame's rank in
 * `kept`); 0 for a sample in no kept frame and at and beyond lengths[r]. The adjoint of the `proc` side of
 * brv_stoi_compact with `kept` held fixed. */
int brv_sl_compact_backward(const float* comp_grad, const int32_t* kept, const int32_t* geom,
                            const int64_t* lengths, float* dx, int64_t rows, int64_t nf_max,
                            int64_t comp_stride, int64_t stride, brv_stream_t stream);

/* dx (rows, in_stride): dx[r][i] = sum over m < ceil(lengths[r] up/down) of
 * hpad[(m + n_pre_remove) down - i up] dy[r][m] for i < lengths[r], in ascending m; 0 beyond. The adjoint of
 * brv_resample_poly with the same arguments; dy (rows, out_stride). */
int brv_sl_resample_backward(const float* dy, const float* hpad, const int64_t* lengths, float* dx,
                             int64_t rows, int64_t in_stride, int64_t out_stride, int64_t up, int64_t down,
                             int64_t hpad_len, int64_t n_pre_remove, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
