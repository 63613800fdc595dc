// Shoebox room impulse responses by the image-source method (include/rir/brever_rir.h): a Hann-windowed
// sinc per image, a first-order receiver pattern, everything in fp64 up to the fp32 store.
//
//   host   build_axis        the candidates of one axis of one job: (offset x_img - r, b0^e0 b1^e1, e0 + e1, offset^2)
//                            for every (n, p) within reach of the last tap, in ascending order of offset^2 (ties in
//                            (n, p) order), so that "inside a distance shell" is a prefix of x, a prefix of y and,
//                            for a given (x, y) pair, one contiguous range of z.
//   device rir_tile_kernel   one workgroup (four waves) per (job, tile of 128 taps), the far (heavy) tiles first.
//                            Produce: lane i of round k owns the (x, y) pair 256 k + i in table order, finds its z
//                            range by two binary searches on the squared offsets (staged in LDS) and appends up to
//                            kPerLane hits per pass at the position a prefix count over the workgroup gives it. An
//                            entry is (tau - t0, amplitude sin(pi frac) / pi with the sign of the integer part,
//                            amplitude if frac == 0, cos and sin of 2 pi (tau - t0) / W, halved).
//                            Consume, whenever the list could not take another pass: wave w takes the entries
//                            w, w + 4, ..., lane j is the taps t0 + j and t0 + j + 64: sinc is sign_j q / u, the window
//                            1/2 + cj cw + sj sw with (cj, sj) of the tap computed once: one reciprocal per (image,
//                            tap), no transcendental.
//                            The four waves' sums are added in wave order and stored as fp32.
//
// Entry positions, the flush points and the slices of the waves are functions of the job's own tables and of the
// tile, nothing else: no atomics, bitwise repeatable, a job alone equals the job in a batch.
//
// rir_bands.cuh, included at the end, adds the band entry points (octave-band walls, a spherical-head ear), and
// rir_hrir.cuh after it the measured-ear entry points (an HRIR set as the ear).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../../include/rir/brever_rir.h"
#include "../status.h"

namespace {

constexpr int kTile = BRV_RIR_TILE;
constexpr int kLaneTaps = kTile/64;             // taps of a lane: lane, lane + 64, ...
constexpr int kThreads = 256, kWaves = kThreads/64;
// Measured at 100 rooms x 19 angles x 8 000 taps: one hit per pass and a list of 512 (33 KB of LDS, four
// workgroups per CU) 162 ms; two hits and 1 024 entries (52 KB, three workgroups) 173 ms; a tile of 256 taps (142 VGPRs,
// two waves per SIMD) 240 ms. The kernel waits on latencies, so residency decides.
constexpr int kPerLane = 1;                    // hits a lane appends per pass
constexpr int kCap = 512;                      // entries of the list; flushed once a pass might not fit
constexpr int kMaxAxis = BRV_RIR_MAX_AXIS_ROWS;
constexpr int kRow = BRV_RIR_ROW_DOUBLES, kIdx = BRV_RIR_INDEX_WORDS, kGeom = BRV_RIR_GEOM_DOUBLES,
              kShape = BRV_RIR_SHAPE_WORDS;
constexpr double kPi = 3.14159265358979323846;
constexpr double kSlack = 1e-6;                // samples by which the shell is widened; the taps test |u| < W/2 exactly
static_assert(kTile%64 == 0 && kTile <= 256, "a lane of a wave is kLaneTaps taps of the tile");
static_assert(kCap >= 2*kThreads*kPerLane, "a flushed list takes one more pass");

// first index of the ascending v[0..n) whose value is >= x (kStrict: > x)
template <bool kStrict> __device__ __forceinline__ int bound(const double* v, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double m = v[mid];
    if (kStrict ? m <= x : m < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// length of the prefix of the ascending column 3 of rows[0..n) that is <= x (uniform; every thread calls it)
__device__ __forceinline__ int prefix_within(const double* rows, int n, double x) {
  int count = 0;
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + (int)threadIdx.x;
    count += __syncthreads_count(i < n && rows[(long long)i*kRow + 3] <= x);
  }
  return count;
}

__global__ __launch_bounds__(kThreads) void rir_tile_kernel(const double* __restrict__ tab,
                                                            const long long* __restrict__ index, long long n_rows,
                                                            double fs, double c, double W, long long max_order,
                                                            float* __restrict__ out, long long out_len) {
  __shared__ double zd2[kMaxAxis];
  __shared__ double e_tau[kCap], e_q[kCap], e_a0[kCap], e_cw[kCap], e_sw[kCap];
  __shared__ int wave_tot[2][kWaves];
  __shared__ double part[kWaves][kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long hdr = ix[0], nxl = ix[1], nyl = ix[2], nzl = ix[3], taps = ix[4], off = ix[5], stride = ix[6];
  // an index that does not describe rows of this table is not followed (uniform)
  if (hdr < 0 || nxl < 0 || nyl < 0 || nzl < 0 || nxl > kMaxAxis || nyl > kMaxAxis || nzl > kMaxAxis ||
      hdr > n_rows - 1 - nxl - nyl - nzl || taps < 1 || taps > BRV_RIR_MAX_TAPS || off < 0 || stride < 1) return;
  const long long ntile = (taps + kTile - 1)/kTile;
  const long long tile = ntile - 1 - (long long)blockIdx.y;
  if (tile < 0) return;
  const long long t0 = tile*kTile;
  const int nx = (int)nxl, ny = (int)nyl, nz = (int)nzl;
  const double* H = tab + hdr*kRow;
  const double* X = H + kRow;
  const double* Y = X + (long long)nx*kRow;
  const double* Z = Y + (long long)ny*kRow;
  const double ox = H[0], oy = H[1], oz = H[2], a = H[3];
  const double halfW = 0.5*W, metres = c/fs;
  const long long t_last = t0 + kTile - 1 < taps - 1 ? t0 + kTile - 1 : taps - 1;
  const double tau_lo = (double)t0 - halfW - kSlack, tau_hi = (double)t_last + halfW + kSlack;
  const double d_lo = tau_lo > 0.0 ? tau_lo*metres : 0.0, d_hi = tau_hi*metres;
  const double lo2 = d_lo*d_lo, hi2 = d_hi*d_hi;

  for (int i = tid; i < nz; i += kThreads) zd2[i] = Z[(long long)i*kRow + 3];
  const int nxe = prefix_within(X, nx, hi2), nye = prefix_within(Y, ny, hi2);   // (barriers: zd2 is visible)
  const long long npairs = nz > 0 ? (long long)nxe*nye : 0;

  // the taps of this lane
  double sj[kLaneTaps], cj[kLaneTaps], acc[kLaneTaps];
#pragma unroll
  for (int k = 0; k < kLaneTaps; ++k) {
    sincospi(2.0*(double)(lane + 64*k)/W, &sj[k], &cj[k]);
    acc[k] = 0.0;
  }
  const double sign_j = (lane & 1) ? -1.0 : 1.0;   // of lane + 64 k as well
  int fill = 0, phase = 0;

  auto consume = [&]() {
    __syncthreads();
#pragma unroll 2
    for (int i = wave; i < fill; i += kWaves) {
      const double tr = e_tau[i], q = sign_j*e_q[i], a0 = e_a0[i], cw = e_cw[i], sw = e_sw[i];
#pragma unroll
      for (int k = 0; k < kLaneTaps; ++k) {
        const double u = (double)(lane + 64*k) - tr;
        const double win = __builtin_fma(sj[k], sw, __builtin_fma(cj[k], cw, 0.5));
        // 1/u as v_rcp_f64 and two Newton steps (five instructions; the IEEE division is about eleven): each step
        // squares the relative error of the one before, far below the fp32 rounding of the output either way. u = 0
        // gives a NaN that the select drops.
        double r = __builtin_amdgcn_rcp(u);
        r = __builtin_fma(__builtin_fma(-u, r, 1.0), r, r);
        r = __builtin_fma(__builtin_fma(-u, r, 1.0), r, r);
        const double v = u == 0.0 ? a0 : q*r*win;
        acc[k] += fabs(u) < halfW ? v : 0.0;
      }
    }
    __syncthreads();
    fill = 0;
  };

  for (long long p0 = 0; p0 < npairs; p0 += kThreads) {
    const long long P = p0 + tid;
    int i0 = 0, i1 = 0, exy = 0;
    double dx = 0.0, dy = 0.0, rxy2 = 0.0, axy = 0.0;
    if (P < npairs) {
      const int ixx = (int)(P/nye), iyy = (int)(P - (long long)ixx*nye);
      const double* xr = X + (long long)ixx*kRow;
      const double* yr = Y + (long long)iyy*kRow;
      dx = xr[0]; dy = yr[0];
      axy = xr[1]*yr[1];
      exy = (int)xr[2] + (int)yr[2];
      rxy2 = xr[3] + yr[3];
      if (rxy2 <= hi2) {
        i0 = bound<false>(zd2, nz, lo2 - rxy2);
        i1 = bound<true>(zd2, nz, hi2 - rxy2);
      }
    }
    for (;;) {
      const int m = i1 - i0 < kPerLane ? i1 - i0 : kPerLane;
      // position of this lane's hits: lanes below it in the wave, then the waves below
      const unsigned long long below = (1ull << lane) - 1ull;
      int pos = 0, tot = 0;
#pragma unroll
      for (int s = 0; s < kPerLane; ++s) {
        const unsigned long long b = __ballot(m > s);
        pos += __popcll(b & below);
        tot += __popcll(b);
      }
      if (lane == 0) wave_tot[phase][wave] = tot;
      __syncthreads();
      int total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int n = wave_tot[phase][w];
        if (w < wave) pos += n;
        total += n;
      }
      phase ^= 1;
      if (total == 0) break;                   // uniform: every lane's range is used up
#pragma unroll
      for (int s = 0; s < kPerLane; ++s) {
        if (s < m) {
          const double* zr = Z + (long long)(i0 + s)*kRow;
          const double dz = zr[0];
          const bool counted = max_order < 0 || exy + (int)zr[2] <= max_order;
          const double d = sqrt(rxy2 + zr[3]);
          const double tau = d*fs/c;
          const double g = a + (1.0 - a)*(dx*ox + dy*oy + dz*oz)/d;
          const double amp = counted ? axy*zr[1]*g/(4.0*kPi*d) : 0.0;
          const double k = floor(tau), f = tau - k;
          const long long kr = (long long)k - t0;
          const double taur = tau - (double)t0;
          double sw, cw;
          sincospi(2.0*taur/W, &sw, &cw);
          const int e = fill + pos + s;        // < kCap: fill <= kCap - kThreads*kPerLane before a pass
          e_tau[e] = taur;
          e_q[e] = f == 0.0 ? 0.0 : amp*sinpi(f)/kPi*((kr & 1) ? 1.0 : -1.0);
          e_a0[e] = f == 0.0 ? amp : 0.0;
          e_cw[e] = 0.5*cw;
          e_sw[e] = 0.5*sw;
        }
      }
      i0 += m;
      fill += total;
      if (fill > kCap - kThreads*kPerLane) consume();
    }
  }
  if (fill > 0) consume();

#pragma unroll
  for (int k = 0; k < kLaneTaps; ++k) part[wave][lane + 64*k] = acc[k];
  __syncthreads();
  if (tid < kTile) {
    const long long t = t0 + tid;
    const double sum = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    if (t < taps) {
      const long long o = off + t*stride;      // taps, stride and off are bounded: no overflow below 2^63
      if (o < out_len) out[o] = (float)sum;
    }
  }
}

struct Row { double d, amp, count, d2; };

// a job's view of the host arrays
struct Job {
  const double *L, *beta, *s, *r, *o;
  double a;
  int64_t taps, off, stride;
};

Job job_at(const double* geom, const int64_t* shape, int64_t j) {
  const double* g = geom + j*kGeom;
  const int64_t* h = shape + j*kShape;
  return Job{g, g + 3, g + 9, g + 12, g + 15, g[18], h[0], h[1], h[2]};
}

bool finite_positive(double v) { return v > 0.0 && v <= 1.79e308; }

// "" or why the batch is refused
std::string check_batch(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                        int64_t max_order) {
  if (!geom || !shape || !opts) return "null pointer: geom, shape and opts are required";
  if (n_jobs < 1 || n_jobs > BRV_RIR_MAX_JOBS) return "requires 1 <= n_jobs <= " + std::to_string(BRV_RIR_MAX_JOBS);
  if (!finite_positive(opts[0]) || !finite_positive(opts[1])) return "requires fs > 0 and c > 0, both finite";
  if (!(opts[2] >= 2.0) || !(opts[2] <= 1e6)) return "requires 2 <= W <= 1e6 (the window in samples)";
  if (max_order < -1) return "requires max_order >= -1";
  for (int64_t j = 0; j < n_jobs; ++j) {
    const Job q = job_at(geom, shape, j);
    const std::string at = "job " + std::to_string(j) + ": ";
    double dist2 = 0.0, norm2 = 0.0;
    for (int k = 0; k < 3; ++k) {
      if (!finite_positive(q.L[k])) return at + "requires room dimensions > 0, finite";
      for (int w = 0; w < 2; ++w)
        if (!(q.beta[2*k + w] >= 0.0) || !(q.beta[2*k + w] <= 1.0)) return at + "requires beta in [0, 1]";
      if (!(q.s[k] > 0.0) || !(q.s[k] < q.L[k])) return at + "the source is outside the box or on a wall";
      if (!(q.r[k] > 0.0) || !(q.r[k] < q.L[k])) return at + "the receiver is outside the box or on a wall";
      dist2 += (q.s[k] - q.r[k])*(q.s[k] - q.r[k]);
      norm2 += q.o[k]*q.o[k];
    }
    if (!(dist2 >= 1e-6)) return at + "requires a direct path of at least 1e-3 m";
    if (!(fabs(norm2 - 1.0) <= 1e-9)) return at + "requires a unit orientation vector";
    if (!(q.a >= 0.0) || !(q.a <= 1.0)) return at + "requires a pattern coefficient in [0, 1]";
    if (q.taps < 1 || q.taps > BRV_RIR_MAX_TAPS) return at + "requires 1 <= taps <= " + std::to_string(BRV_RIR_MAX_TAPS);
    if (q.off < 0 || q.off > (1ll << 40)) return at + "requires 0 <= out_offset <= 2^40";
    if (q.stride < 1 || q.stride > 1024) return at + "requires 1 <= out_stride <= 1024";
  }
  return "";
}

// The candidates of axis k of a job; false if there are more than the limit.
bool build_axis(const Job& q, int k, const double* opts, int64_t max_order, std::vector<Row>* rows) {
  const double fs = opts[0], c = opts[1], W = opts[2];
  const double L = q.L[k], b0 = q.beta[2*k], b1 = q.beta[2*k + 1];
  const double reach = (c/fs)*((double)(q.taps - 1) + 0.5*W + kSlack);
  rows->clear();
  if (reach/L > 4.0*kMaxAxis) return false;
  const long long N = (long long)ceil((reach + L)/(2.0*L)) + 1;
  for (long long n = -N; n <= N; ++n) {
    for (int p = 0; p < 2; ++p) {
      const double x = (1.0 - 2.0*p)*q.s[k] + 2.0*(double)n*L;
      const double d = x - q.r[k];
      if (fabs(d) > reach) continue;
      const long long e0 = n - p < 0 ? p - n : n - p, e1 = n < 0 ? -n : n;
      if (max_order >= 0 && e0 + e1 > max_order) continue;
      const double amp = pow(b0, (double)e0)*pow(b1, (double)e1);      // pow(0, 0) = 1
      if (amp == 0.0) continue;
      rows->push_back(Row{d, amp, (double)(e0 + e1), d*d});
    }
  }
  if ((long long)rows->size() > kMaxAxis) return false;
  std::stable_sort(rows->begin(), rows->end(), [](const Row& u, const Row& v) { return u.d2 < v.d2; });
  return true;
}

const char* kTooMany = "an axis has more than BRV_RIR_MAX_AXIS_ROWS (1024) candidates: fewer taps or a larger room";

}  // namespace

extern "C" {

int64_t brv_rir_table_rows(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                           int64_t max_order) {
  const std::string why = check_batch(geom, shape, n_jobs, opts, max_order);
  if (!why.empty()) return brv::fail(-1, why);
  std::vector<Row> rows;
  int64_t total = 0;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const Job q = job_at(geom, shape, j);
    total += 1;
    for (int k = 0; k < 3; ++k) {
      if (!build_axis(q, k, opts, max_order, &rows)) return brv::fail(-1, "job " + std::to_string(j) + ": " + kTooMany);
      total += (int64_t)rows.size();
    }
  }
  return total;
}

int brv_rir_build_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                         int64_t max_order, double* rows_out, int64_t* index, int64_t n_rows) {
  BRV_REFUSE(!rows_out || !index, "null pointer: rows and index are required");
  const std::string why = check_batch(geom, shape, n_jobs, opts, max_order);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(n_rows < 1, "requires n_rows >= 1: the value of brv_rir_table_rows");
  std::vector<Row> rows;
  int64_t at = 0;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const Job q = job_at(geom, shape, j);
    int64_t* ix = index + j*kIdx;
    BRV_REFUSE(at + 1 > n_rows, "n_rows is not what brv_rir_table_rows gives for this batch");
    ix[0] = at;
    double* h = rows_out + at*kRow;
    h[0] = q.o[0]; h[1] = q.o[1]; h[2] = q.o[2]; h[3] = q.a;
    at += 1;
    for (int k = 0; k < 3; ++k) {
      BRV_REFUSE(!build_axis(q, k, opts, max_order, &rows), "job " + std::to_string(j) + ": " + kTooMany);
      BRV_REFUSE(at + (int64_t)rows.size() > n_rows, "n_rows is not what brv_rir_table_rows gives for this batch");
      ix[1 + k] = (int64_t)rows.size();
      for (const Row& r : rows) {
        double* w = rows_out + at*kRow;
        w[0] = r.d; w[1] = r.amp; w[2] = r.count; w[3] = r.d2;
        at += 1;
      }
    }
    ix[4] = q.taps; ix[5] = q.off; ix[6] = q.stride; ix[7] = 0;
  }
  BRV_REFUSE(at != n_rows, "n_rows is not what brv_rir_table_rows gives for this batch");
  return 0;
}

int brv_rir_simulate(const double* tables, const int64_t* index, int64_t n_jobs, int64_t n_rows, int64_t max_taps,
                     const double* opts, int64_t max_order, float* out, int64_t out_len, brv_stream_t stream) {
  BRV_REFUSE(!tables || !index || !opts || !out, "null pointer: tables, index, opts and out are required");
  BRV_REFUSE(n_jobs < 1 || n_jobs > BRV_RIR_MAX_JOBS, "requires 1 <= n_jobs <= " + std::to_string(BRV_RIR_MAX_JOBS));
  BRV_REFUSE(n_rows < 1, "requires n_rows >= 1");
  BRV_REFUSE(max_taps < 1 || max_taps > BRV_RIR_MAX_TAPS,
             "requires 1 <= max_taps <= " + std::to_string(BRV_RIR_MAX_TAPS));
  BRV_REFUSE(out_len < 1, "requires out_len >= 1");
  BRV_REFUSE(!finite_positive(opts[0]) || !finite_positive(opts[1]), "requires fs > 0 and c > 0, both finite");
  BRV_REFUSE(!(opts[2] >= 2.0) || !(opts[2] <= 1e6), "requires 2 <= W <= 1e6 (the window in samples)");
  BRV_REFUSE(max_order < -1, "requires max_order >= -1");
  const int64_t ntile = (max_taps + kTile - 1)/kTile;          // <= 16384 <= the limit of gridDim.y
  hipLaunchKernelGGL(rir_tile_kernel, dim3((unsigned)n_jobs, (unsigned)ntile), dim3(kThreads), 0,
                     (hipStream_t)stream, tables, (const long long*)index, (long long)n_rows, opts[0], opts[1],
                     opts[2], (long long)max_order, out, (long long)out_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}

// the band entry points (include/rir/brever_rir_bands.h)
#include "rir_bands.cuh"

// the measured-ear entry points (include/rir/brever_rir_hrir.h)
#include "rir_hrir.cuh"

// the library's last-error message and its two status exports (../status.h)
BRV_DEFINE_STATUS(brv_rir_version, brv_rir_last_error)
