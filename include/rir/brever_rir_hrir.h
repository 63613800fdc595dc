/* brever_rir_hrir.h -- the measured-ear entry points of libbrever_rir.so: shoebox room impulse responses whose ear is
 * a set of measured head-related impulse responses (HRIRs), on the MI355X (gfx950). They stand beside the entry
 * points of brever_rir.h and brever_rir_bands.h, which they leave as they are; brever_amd/rir.py runs them and
 * DESIGN.md 5o states the model and the kernels.
 *
 * Everything of brever_rir.h and brever_rir_bands.h stands (lattice n, parity p, the wall product A_k per band, the
 * window W, max_order, the clip to 0 <= t < taps, K octave bands with beta (K, 6)). What is new:
 *
 * HRIR set. D unit vectors p_j in the head's frame (x front, y left, z up; azimuth counter-clockwise seen from above,
 * p = (cos el cos az, cos el sin az, sin el)) and H[j][e][m], e = left, right, 0 <= m < T_h, fp64 at the simulation's
 * fs. 1 <= D <= BRV_RIR_HRIR_MAX_DIRS, 1 <= T_h <= BRV_RIR_HRIR_MAX_TAPS.
 *
 * Receiver. r is the head's centre; the head is upright with front f and left l, both unit, horizontal and at right
 * angles, and up u = (0, 0, 1). One job is one (room, source): it yields both ears.
 *
 * Image. v = x_img - r, d = |v| > 0, q = (v.f, v.l, v.u) (not normalised), j* = argmax_j q.p_j with ties to the
 * lowest j, tau = d fs/c, amplitude A_k / (4 pi d) in band k. No pattern, no head radius, no parallax between the
 * ears: the interaural differences are those of the measured pair.
 *
 * Direction rows. x_{k,j}[t], 0 <= t < taps + pad, is the sum of brever_rir.h over the images with j* = j; fp64.
 * Fold. y_{k,e}[t] = sum_j sum_m H[j][e][m] x_{k,j}[t - m], j ascending then m ascending, fp64, 0 <= t < taps + pad.
 * Output. h_e[t] = sum_k sum_m g_k[m] y_{k,e}[t + pad - m], fp32: brv_rir_bands_combine with pattern-mode opts
 * (fs c W K BRV_RIR_BANDS_PATTERN 0 pad) on the fold scratch and the ear index. The HRIR's own onset delay is kept
 * as measured.
 *
 * Per job `geom` holds BRV_RIR_HRIR_GEOM_DOUBLES doubles
 *   L[3]  s[3]  r[3]  f[3]  l[3]  beta[BRV_RIR_BANDS_MAX_BANDS][6]      (the first K rows of beta are read)
 * and `shape` BRV_RIR_HRIR_SHAPE_WORDS int64: taps, out_offset, out_stride, ear_offset -- tap t of the left ear goes to
 * out[out_offset + t out_stride], of the right ear ear_offset elements further. `opts` holds
 * BRV_RIR_HRIR_OPT_DOUBLES doubles
 *   fs  c  W  K  pad  D  T_h
 * (K, pad, D and T_h integers held as doubles). `dirs` is (D, 3) double.
 *
 * Five steps, the first two on the host:
 *   brv_rir_hrir_table_rows    checks every job and the directions and counts the rows of the tables
 *   brv_rir_hrir_build_tables  per job one header row (f, l) and the three per-axis candidate tables of
 *                              brv_rir_bands_build_tables in pattern mode (rows of 3 + K doubles, the same reach).
 *                              `index` gets BRV_RIR_INDEX_WORDS int64 per job: header row, rows of x, y, z, taps, the
 *                              job's offset into the direction scratch, 0, its offset into the fold scratch, both in
 *                              doubles: job j takes K D (taps_j + pad) doubles of the direction scratch (row (k, j')
 *                              at (k D + j')(taps_j + pad)) and 2 K (taps_j + pad) of the fold scratch (row (e, k) at
 *                              (e K + k)(taps_j + pad)) after those of the jobs before it. `ear_index` gets
 *                              BRV_RIR_INDEX_WORDS int64 per (job, ear), job-major: a job of brv_rir_bands_combine
 *                              with C = K whose channel rows are that ear's K rows of the fold scratch and whose
 *                              output is that ear's.
 *   brv_rir_hrir_channels      clears the direction scratch on the caller's stream, then one launch: one workgroup
 *                              per (job, tile of BRV_RIR_TILE taps of taps + pad), the shell and the compaction of
 *                              brv_rir_bands_channels with a list entry that carries its direction index (the argmax
 *                              over D once per entry). A full list is ordered by direction in LDS (stable in list
 *                              order) and walked with K x 2 accumulators per lane that are added to the direction's
 *                              rows at every change of direction. A tile's rows belong to one workgroup.
 *   brv_rir_hrir_fold          one launch: one workgroup per (job, 1 024 taps of taps + pad, band); per direction the
 *                              stretch of its row goes to LDS once and both ears are folded from it, 8 taps per lane,
 *                              filter taps 16 at a time. `hrirs` is (D, 2, n_filter) with n_filter >= T_h a multiple
 *                              of 16, padded with zeros.
 *   brv_rir_bands_combine      (brever_rir_bands.h) on the fold scratch with `ear_index` and 2 n_jobs jobs.
 *
 * Every sum has a fixed order that depends on the job alone: no floating-point atomics, bitwise repeatable, a job
 * gives the same bits alone as in a batch. Out of scope: interpolation between measured directions, distance-dependent
 * and near-field HRTFs, head pitch and roll, SOFA conventions other than SimpleFreeFieldHRIR (brever_amd/rir.py
 * reads that one), air absorption, source directivity, other room shapes.
 *
 * Conventions: those of brever_rir.h. geom, shape, opts, dirs, rows, index and ear_index of the host steps are HOST
 * pointers; tables, index, dirs, hrirs and the scratches of the launches are device pointers borrowed from the caller
 * (opts stays a host pointer); the caller's stream, no synchronise, no allocation, no global state; 0 ok, -1 refused
 * argument, > 0 a hipError_t, and brv_rir_last_error() gives the message.
 */
#ifndef BREVER_RIR_HRIR_H
#define BREVER_RIR_HRIR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

/* (declared in brever_rir.h as well: the library has one message) */
const char* brv_rir_last_error(void);

#define BRV_RIR_HRIR_MAX_DIRS 2048
#define BRV_RIR_HRIR_MAX_TAPS 512
#define BRV_RIR_HRIR_GEOM_DOUBLES 63
#define BRV_RIR_HRIR_SHAPE_WORDS 4
#define BRV_RIR_HRIR_OPT_DOUBLES 7
/* taps of the fold's output that one workgroup of brv_rir_hrir_fold writes */
#define BRV_RIR_HRIR_FOLD_TILE 1024

/* rows (of 3 + K doubles) that brv_rir_hrir_build_tables writes; -1 for a batch it refuses: what
 * brv_rir_bands_table_rows refuses in pattern mode, D or T_h out of range, a direction that is not finite or of zero
 * length (a unit vector is required), f or l not unit, not horizontal or not at right angles, a source at the head's
 * centre, an ear_offset below 1. */
int64_t brv_rir_hrir_table_rows(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                                const double* dirs, int64_t max_order);

/* rows (n_rows, 3 + K) double, index (n_jobs, BRV_RIR_INDEX_WORDS) and ear_index (2 n_jobs, BRV_RIR_INDEX_WORDS)
 * int64, host memory; n_rows as counted. */
int brv_rir_hrir_build_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                              const double* dirs, int64_t max_order, double* rows, int64_t* index,
                              int64_t* ear_index, int64_t n_rows);

/* tables and index as built and dirs (D, 3), on the device; dir_scratch (dir_len) double on the device, all of which
 * is cleared. A job whose index reaches outside [0, n_rows) or whose rows reach outside [0, dir_len) is skipped, never
 * followed; a dir_len below K D (max_taps + pad) is refused. */
int brv_rir_hrir_channels(const double* tables, const int64_t* index, int64_t n_jobs, int64_t n_rows,
                          int64_t max_taps, const double* opts, int64_t max_order, const double* dirs,
                          double* dir_scratch, int64_t dir_len, brv_stream_t stream);

/* hrirs (D, 2, n_filter) double on the device; fold_scratch (fold_len) double on the device. Jobs are skipped as
 * above; every tap of a job's 2 K rows is written. */
int brv_rir_hrir_fold(const double* dir_scratch, int64_t dir_len, const int64_t* index, int64_t n_jobs,
                      int64_t max_taps, const double* opts, const double* hrirs, int64_t n_filter,
                      double* fold_scratch, int64_t fold_len, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
