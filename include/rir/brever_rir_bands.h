/* brever_rir_bands.h -- the band entry points of libbrever_rir.so: shoebox room impulse responses with octave-band
 * wall coefficients and, optionally, a spherical-head ear (Brown & Duda 1998), on the MI355X (gfx950). They stand
 * beside the four entry points of brever_rir.h, which they leave as they are; brever_amd/rir.py runs them and
 * DESIGN.md 5n states the model and the kernels.
 *
 * Everything of brever_rir.h stands (lattice n, parity p, x, e0, e1, v = x - r, d, the window W, max_order, the clip
 * to 0 <= t < taps). What changes:
 *
 * Bands. K octave bands, 1 <= K <= BRV_RIR_BANDS_MAX_BANDS, centres fc_k = 125 2^k Hz, fc_{K-1} < fs/2. beta is
 * (K, 6); the wall product of an image is A_k = prod b_k?0^e0 b_k?1^e1 per band (0^0 = 1), and an image is dropped
 * only if A_k = 0 in every band.
 *
 * Receiver modes (one per batch).
 *   BRV_RIR_BANDS_PATTERN  g = a + (1 - a)(v.o)/d, tau = d fs/c; C = K channels of amplitude A_k g / (4 pi d).
 *   BRV_RIR_BANDS_SPHERE   r is the head's centre, o the ear's outward axis, rad the head radius; the direct path is
 *                          longer than rad. theta = acos(clamp((v.o)/d, -1, 1)),
 *                          alpha = (1 + amin/2) + (1 - amin/2) cos(theta 180/150), amin = 0.1,
 *                          delta = -rad cos(theta) for theta < pi/2, else rad (theta - pi/2)   (Woodworth),
 *                          tau = (d + delta) fs/c, spreading 1/(4 pi d) by the centre distance. C = 2K channels:
 *                          channel k is A_k alpha / (4 pi d) ("direct"), channel K + k is A_k (1 - alpha) / (4 pi d)
 *                          ("shadowed": the caller's filter of that channel holds the head's one-pole low-pass).
 *
 * Channel responses. x_c[t], 0 <= t < taps + pad and zero elsewhere, is the sum of brever_rir.h with the channel's
 * amplitude and this tau; fp64.
 *
 * Output. h[t] = sum_c sum_m f_c[m] x_c[t + pad - m] for 0 <= t < taps, with the caller's filters f (C, M_f) fp64, in
 * fp64, stored as fp32. brever_amd/rir.py designs f: raised-cosine octave bands on a log-frequency axis that sum to
 * one, Hann-windowed to N = 2 pad taps, and for the shadowed channels convolved with the head's low-pass.
 *
 * Per job `geom` holds BRV_RIR_BANDS_GEOM_DOUBLES doubles
 *   L[3]  s[3]  r[3]  o[3]  a  beta[BRV_RIR_BANDS_MAX_BANDS][6]      (the first K rows of beta are read)
 * and `shape` BRV_RIR_SHAPE_WORDS int64 (taps, out_offset, out_stride) as in brever_rir.h. `opts` holds
 * BRV_RIR_BANDS_OPT_DOUBLES doubles
 *   fs  c  W  K  mode  rad  pad
 * (K, mode and pad integers held as doubles; rad is read in sphere mode only; 0 <= pad <= BRV_RIR_BANDS_MAX_FILTER/2).
 *
 * Four steps, the first two on the host:
 *   brv_rir_bands_table_rows    checks every job and counts the rows of its tables
 *   brv_rir_bands_build_tables  per job one header row (o, a) and three per-axis candidate tables; a row is 3 + K
 *                               doubles (x_img - r, e0 + e1, (x_img - r)^2, b_k0^e0 b_k1^e1 for every band), an axis
 *                               holds the candidates within reach of tap taps + pad - 1 (in sphere mode the reach is
 *                               wider by rad, the most that delta shortens a path) of which some band's amplitude is
 *                               not 0 and whose count is within max_order, in ascending order of the squared offset.
 *                               `index` gets BRV_RIR_INDEX_WORDS int64 per job: header row, rows of x, y, z, taps,
 *                               out_offset, out_stride, and the job's offset into the scratch in doubles: job j takes
 *                               C (taps_j + pad) doubles after those of the jobs before it.
 *   brv_rir_bands_channels      one launch: one workgroup per (job, tile of BRV_RIR_TILE taps of taps + pad), the
 *                               structure of the kernel of brv_rir_simulate with a list entry that carries the C
 *                               amplitudes: sinc times window once per (image, tap), then C FMAs. A tile's distance
 *                               shell is widened by the range of delta, [-rad, rad pi/2], in sphere mode. Writes the
 *                               fp64 channel rows into scratch (C, taps + pad) per job.
 *   brv_rir_bands_combine       one launch: per job the filters applied to the channel rows, summed over the channels
 *                               in channel order and stored as fp32 to out[out_offset + t out_stride].
 *
 * Every sum has a fixed order that depends on the job alone: no atomics, bitwise repeatable, a job gives the same
 * bits alone as in a batch. Out of scope: air absorption, source directivity, torso effects, other room shapes; a
 * measured ear (HRTFs, pinna cues) is brever_rir_hrir.h.
 *
 * Conventions: those of brever_rir.h. geom, shape, opts, rows and index of the host steps are HOST pointers; tables,
 * index, scratch, filters and out of the two launches are device pointers borrowed from the caller (opts stays a host
 * pointer); the caller's stream, no synchronise, no allocation, no global state; 0 ok, -1 refused argument, > 0 a
 * hipError_t, and brv_rir_last_error() gives the message.
 */
#ifndef BREVER_RIR_BANDS_H
#define BREVER_RIR_BANDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

/* (declared in brever_rir.h as well: the library has one message) */
const char* brv_rir_last_error(void);

#define BRV_RIR_BANDS_MAX_BANDS 8
#define BRV_RIR_BANDS_GEOM_DOUBLES 61
#define BRV_RIR_BANDS_OPT_DOUBLES 7
#define BRV_RIR_BANDS_PATTERN 0
#define BRV_RIR_BANDS_SPHERE 1
/* taps of a filter, at most; a multiple of 16 is required of M_f (pad with zeros) */
#define BRV_RIR_BANDS_MAX_FILTER 2048
/* taps of the output that one workgroup of brv_rir_bands_combine writes */
#define BRV_RIR_BANDS_COMBINE_TILE 1024

/* rows (of 3 + K doubles) that brv_rir_bands_build_tables writes; -1 for a batch it refuses: what brv_rir_table_rows
 * refuses, K outside [1, BRV_RIR_BANDS_MAX_BANDS], fc_{K-1} >= fs/2, a mode that is neither constant, pad outside
 * [0, BRV_RIR_BANDS_MAX_FILTER/2], and in sphere mode a radius not positive, a head that touches a wall or a source
 * inside the sphere. */
int64_t brv_rir_bands_table_rows(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                                 int64_t max_order);

/* rows (n_rows, 3 + K) double and index (n_jobs, BRV_RIR_INDEX_WORDS) int64, host memory; n_rows as counted. */
int brv_rir_bands_build_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                               int64_t max_order, double* rows, int64_t* index, int64_t n_rows);

/* tables and index as built, on the device; scratch (scratch_len) double on the device. A job whose index reaches
 * outside [0, n_rows) or whose channel rows reach outside [0, scratch_len) is skipped, never followed; a scratch_len
 * below C (max_taps + pad) is refused. */
int brv_rir_bands_channels(const double* tables, const int64_t* index, int64_t n_jobs, int64_t n_rows,
                           int64_t max_taps, const double* opts, int64_t max_order, double* scratch,
                           int64_t scratch_len, brv_stream_t stream);

/* filters (C, n_filter) double on the device, n_filter a multiple of 16 up to BRV_RIR_BANDS_MAX_FILTER; out (out_len)
 * float on the device. Jobs are skipped and stores dropped as above. Taps nobody writes keep what out held. */
int brv_rir_bands_combine(const double* scratch, int64_t scratch_len, const int64_t* index, int64_t n_jobs,
                          int64_t max_taps, const double* opts, const double* filters, int64_t n_filter, float* out,
                          int64_t out_len, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
