/* brever_rir.h -- C ABI of libbrever_rir.so: room impulse responses of a shoebox room by the image-source method
 * (Allen & Berkley 1979) with a Hann-windowed sinc per image and a first-order receiver pattern, on the MI355X
 * (gfx950). brever_amd/rir.py runs it; DESIGN.md 5m states the model and the kernel.
 *
 * A batch is n_jobs jobs; a job is one (room, source, receiver) response with its own number of taps and its own
 * place in the output. Per job, `geom` holds BRV_RIR_GEOM_DOUBLES doubles
 *   L[3]  beta[6] = (bx0, bx1, by0, by1, bz0, bz1)  s[3]  r[3]  o[3]  a
 * (room in metres with one corner at the origin, wall reflection coefficients, source, receiver, the receiver's unit
 * orientation and its pattern coefficient: 1 omni, 0.5 cardioid) and `shape` holds BRV_RIR_SHAPE_WORDS int64
 *   taps  out_offset  out_stride
 * (tap t of the job is written to out[out_offset + t out_stride]). `opts` holds BRV_RIR_OPT_DOUBLES doubles
 *   fs  c  W
 * (sample rate, speed of sound, window in samples, any real value >= 2), and max_order >= 0 keeps the images of at
 * most that many reflections, -1 all that reach the taps. For every n in Z^3 and p in {0,1}^3, per axis:
 *   x = (1 - 2p) s + 2 n L,  e0 = |n - p|,  e1 = |n|,  A = prod b?0^e0 b?1^e1 (0^0 = 1),  v = x - r,  d = |v|,
 *   tau = d fs / c,  g = a + (1 - a) (v . o) / d,
 *   h[t] += A g / (4 pi d) sinc(t - tau) (1 + cos(2 pi (t - tau) / W)) / 2    for 0 <= t < taps, |t - tau| < W/2.
 * Geometry, window and accumulation are fp64; the output is fp32.
 *
 * Three steps, the first two on the host:
 *   brv_rir_table_rows     checks every job and counts the rows of its tables
 *   brv_rir_build_tables   writes, per job, one header row (o, a) and three per-axis candidate tables into host
 *                          memory: a row is (x_img - r, b0^e0 b1^e1, e0 + e1, (x_img - r)^2), an axis holds the
 *                          candidates within reach of the last tap whose amplitude is not 0 and whose count is within
 *                          max_order, in ascending order of the squared offset; `index` gets BRV_RIR_INDEX_WORDS int64
 *                          per job: header row, rows of x, y, z, taps, out_offset, out_stride, 0
 *   brv_rir_simulate       one launch over the uploaded tables: one workgroup per (job, tile of BRV_RIR_TILE taps).
 *                          Lanes own (x, y) candidate pairs in table order and solve for the z candidates inside the
 *                          tile's distance shell; the hits are compacted by a prefix count into a list in LDS
 *                          (delay, amplitude, sin(pi frac), the window's cos / sin), then every lane is two taps
 *                          and consumes the list in order: one reciprocal per (image, tap), no transcendental.
 *
 * The order of every sum is a function of the job's own lattice: there are no atomics, results are bitwise
 * repeatable, and a job gives the same bits alone as in a batch.
 *
 * Conventions of the library, those of include/brever_resample.h:
 *   - geom, shape, opts, rows and index of the two host steps are HOST pointers; tables, index and out of
 *     brv_rir_simulate are device pointers borrowed from the caller (opts stays a host pointer); the library
 *     allocates nothing and keeps no process-global state;
 *   - brv_rir_simulate takes the HIP stream to launch on and never synchronises;
 *   - return value: 0 ok, -1 refused argument, > 0 a hipError_t; brv_rir_last_error() gives the thread-local
 *     message every non-zero return has set.
 */
#ifndef BREVER_RIR_H
#define BREVER_RIR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

int brv_rir_version(void);
const char* brv_rir_last_error(void);

#define BRV_RIR_GEOM_DOUBLES 19
#define BRV_RIR_SHAPE_WORDS 3
#define BRV_RIR_OPT_DOUBLES 3
#define BRV_RIR_ROW_DOUBLES 4
#define BRV_RIR_INDEX_WORDS 8
/* taps per workgroup */
#define BRV_RIR_TILE 128
/* the limits: candidates of one axis of one job, taps of one job, jobs of one batch */
#define BRV_RIR_MAX_AXIS_ROWS 1024
#define BRV_RIR_MAX_TAPS 1048576
#define BRV_RIR_MAX_JOBS 1048576

/* rows (of BRV_RIR_ROW_DOUBLES doubles) that brv_rir_build_tables writes for the batch; -1 for a batch it refuses:
 * null pointers, n_jobs outside [1, BRV_RIR_MAX_JOBS], fs or c not positive and finite, W < 2, max_order < -1, a
 * room dimension not positive, beta outside [0, 1], a source or receiver not strictly inside the box, a direct path
 * shorter than 1e-3 m, an orientation that is not a unit vector, a outside [0, 1], taps outside
 * [1, BRV_RIR_MAX_TAPS], a negative out_offset, out_stride < 1, an axis of more than BRV_RIR_MAX_AXIS_ROWS
 * candidates. */
int64_t brv_rir_table_rows(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                           int64_t max_order);

/* rows (n_rows, BRV_RIR_ROW_DOUBLES) double and index (n_jobs, BRV_RIR_INDEX_WORDS) int64, both host memory;
 * n_rows is what brv_rir_table_rows returned for the same arguments, anything else is refused. */
int brv_rir_build_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                         int64_t max_order, double* rows, int64_t* index, int64_t n_rows);

/* tables (n_rows, BRV_RIR_ROW_DOUBLES) double and index (n_jobs, BRV_RIR_INDEX_WORDS) int64 as built, on the device;
 * out (out_len) float on the device; max_taps the largest taps of the batch. A job whose index reaches outside
 * [0, n_rows) or whose taps land outside [0, out_len) is skipped, resp. clipped, never followed. Taps nobody writes
 * keep what out held. */
int brv_rir_simulate(const double* tables, const int64_t* index, int64_t n_jobs, int64_t n_rows, int64_t max_taps,
                     const double* opts, int64_t max_order, float* out, int64_t out_len, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
