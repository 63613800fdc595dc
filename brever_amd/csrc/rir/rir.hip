// Shoebox room impulse responses by the image-source method (include/rir/brever_rir.h): a Hann-windowed
// sinc per image, a first-order receiver pattern, everything in fp64 up to the fp32 store.
//
//   host   rir_host.h        the job checks, build_axis and the table loop of all three families of entry points.
//   device rir_shell.cuh     the walk over the images of a tile's distance shell, the list entry of a delay and the
//                            windowed sinc at a lane's taps, for all three tile kernels.
//          rir_tile_kernel   one workgroup (four waves) per (job, tile of 128 taps). An entry is that of
//                            delay_entry with the amplitude folded in: (tau - t0, amplitude sin(pi frac) / pi with
//                            the sign of the integer part, amplitude if frac == 0, cos and sin of 2 pi (tau - t0) / W,
//                            halved). Consume, whenever the list could not take another pass: wave w takes the entries
//                            w, w + 4, ...; the four waves' sums are added in wave order and stored as fp32.
//
// rir_bands.cuh, included at the end, adds the band entry points (octave-band walls, a spherical-head ear), and
// rir_hrir.cuh after it the measured-ear entry points (an HRIR set as the ear); rir_fir.cuh is the FIR tile of their
// second kernels.
#include <hip/hip_runtime.h>

#include "../../../include/rir/brever_rir.h"
#include "../status.h"
#include "rir_host.h"
#include "rir_shell.cuh"

namespace {

constexpr int kGeom = BRV_RIR_GEOM_DOUBLES;
constexpr int kCap = 512;                      // entries of the list; flushed once a pass might not fit

__global__ __launch_bounds__(kThreads) void rir_tile_kernel(const double* __restrict__ tab,
                                                            const long long* __restrict__ index, long long n_rows,
                                                            double fs, double c, double W, long long max_order,
                                                            float* __restrict__ out, long long out_len) {
  constexpr int RW = kRow;                       // a row is (offset, amplitude, count, offset^2)
  __shared__ double zd2[kMaxAxis];
  __shared__ double e_tau[kCap], e_q[kCap], e_a0[kCap], e_cw[kCap], e_sw[kCap];
  __shared__ int wave_tot[2][kWaves];
  __shared__ double part[kWaves][kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long off = ix[5], stride = ix[6];
  // The index row, the tile and its shell are written out here as this kernel always had them, not taken from
  // shell_rows and shell_tile, whose results are the same: with those two calls the launch of DESIGN.md 5m took 163.0
  // ms where this form takes 161.8 and the kernel before the shared walk 161.6, with the consume loop the same
  // instruction for instruction in all three (profiles/rir_shared_resources.md). The band and measured-ear kernels
  // lose nothing by the calls.
  const long long hdr = ix[0], nxl = ix[1], nyl = ix[2], nzl = ix[3], taps = ix[4];
  // an index that does not describe rows of this table is not followed (uniform)
  if (hdr < 0 || nxl < 0 || nyl < 0 || nzl < 0 || nxl > kMaxAxis || nyl > kMaxAxis || nzl > kMaxAxis ||
      hdr > n_rows - 1 - nxl - nyl - nzl || taps < 1 || taps > BRV_RIR_MAX_TAPS || off < 0 || stride < 1) return;
  const long long ntile = (taps + kTile - 1)/kTile;
  const long long tile = ntile - 1 - (long long)blockIdx.y;
  if (tile < 0) return;
  const long long t0 = tile*kTile;
  const int nx = (int)nxl, ny = (int)nyl, nz = (int)nzl;
  const double* H = tab + hdr*RW;
  const double* X = H + RW;
  const double* Y = X + (long long)nx*RW;
  const double* Z = Y + (long long)ny*RW;
  const double ox = H[0], oy = H[1], oz = H[2], a = H[3];
  const double halfW = 0.5*W, metres = c/fs;
  const long long t_last = t0 + kTile - 1 < taps - 1 ? t0 + kTile - 1 : taps - 1;
  const double tau_lo = (double)t0 - halfW - kSlack, tau_hi = (double)t_last + halfW + kSlack;
  const double d_lo = tau_lo > 0.0 ? tau_lo*metres : 0.0, d_hi = tau_hi*metres;
  const double lo2 = d_lo*d_lo, hi2 = d_hi*d_hi;
  for (int i = tid; i < nz; i += kThreads) zd2[i] = Z[(long long)i*RW + 3];
  const int nxe = prefix_within<RW, 3>(X, nx, hi2), nye = prefix_within<RW, 3>(Y, ny, hi2);
  __syncthreads();                               // zd2 is visible whatever nx and ny are
  const Shell s{H, X, Y, Z, nx, ny, nz, taps, taps, t0, halfW, lo2, hi2, nz > 0 ? (long long)nxe*nye : 0, nye};

  const LaneTaps lt = lane_taps(lane, W);
  double acc[kLaneTaps];
#pragma unroll
  for (int k = 0; k < kLaneTaps; ++k) acc[k] = 0.0;

  auto consume = [&](int fill) {
    __syncthreads();
#pragma unroll 2
    for (int i = wave; i < fill; i += kWaves) {
      double v[kLaneTaps];
      tap_weights(lt, lane, halfW, e_tau[i], e_q[i], e_a0[i], e_cw[i], e_sw[i], v);
#pragma unroll
      for (int k = 0; k < kLaneTaps; ++k) acc[k] += v[k];
    }
    __syncthreads();
  };

  auto append = [&](int e, const Hit& h) {
    const double tau = h.d*fs/c;
    const double g = a + (1.0 - a)*(h.dx*ox + h.dy*oy + h.dz*oz)/h.d;
    const double amp = h.counted ? h.axy*h.zr[1]*g/(4.0*kPi*h.d) : 0.0;
    const Delay dl = delay_entry(tau, t0, W, amp);
    e_tau[e] = dl.taur;
    e_q[e] = dl.s;
    e_a0[e] = dl.whole ? amp : 0.0;
    e_cw[e] = dl.cw;
    e_sw[e] = dl.sw;
  };

  shell_walk<RW, 2, 3, 1, kCap>(s, zd2, wave_tot, max_order, append, consume);

  const double sum = wave_sum(part, acc);
  if (tid < kTile) {
    const long long t = t0 + tid;
    if (t < taps) {
      const long long o = off + t*stride;      // taps, stride and off are bounded: no overflow below 2^63
      if (o < out_len) out[o] = (float)sum;
    }
  }
}

// The batch checked, then its tables counted (rows_out null) or written: "" or why it is refused.
std::string base_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                        int64_t max_order, double* rows_out, int64_t* index, int64_t n_rows, int64_t* total) {
  if (!geom || !shape || !opts) return "null pointer: geom, shape and opts are required";
  std::string why = jobs_why(n_jobs);
  if (why.empty()) why = rate_why(opts);
  if (why.empty() && max_order < -1) why = kNeedsOrder;
  if (!why.empty()) return why;
  const auto job_at = [&](int64_t j) {
    const double* g = geom + j*kGeom;
    const int64_t* h = shape + j*kShape;
    return Job{g, g + 3, g + 9, g + 12, g + 15, nullptr, g[18], h[0], h[1], h[2], 0};
  };
  return tables<1>(n_jobs, job_at, kBase, Opts{opts[0], opts[1], opts[2], 0.0, 1, BRV_RIR_BANDS_PATTERN, 1, 0}, max_order,
                "brv_rir_table_rows", rows_out, index, n_rows, total,
                [](int64_t, const Job& q, double* h, int64_t* ix) {
                  h[0] = q.o[0]; h[1] = q.o[1]; h[2] = q.o[2]; h[3] = q.a;
                  ix[4] = q.taps; ix[5] = q.off; ix[6] = q.stride; ix[7] = 0;
                });
}

}  // namespace

extern "C" {

int64_t brv_rir_table_rows(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                           int64_t max_order) {
  int64_t total = 0;
  const std::string why = base_tables(geom, shape, n_jobs, opts, max_order, nullptr, nullptr, 0, &total);
  return why.empty() ? total : brv::fail(-1, why);
}

int brv_rir_build_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                         int64_t max_order, double* rows_out, int64_t* index, int64_t n_rows) {
  BRV_REFUSE(!rows_out || !index, "null pointer: rows and index are required");
  int64_t total = 0;
  const std::string why = base_tables(geom, shape, n_jobs, opts, max_order, rows_out, index, n_rows, &total);
  BRV_REFUSE(!why.empty(), why);
  return 0;
}

int brv_rir_simulate(const double* tables, const int64_t* index, int64_t n_jobs, int64_t n_rows, int64_t max_taps,
                     const double* opts, int64_t max_order, float* out, int64_t out_len, brv_stream_t stream) {
  BRV_REFUSE(!tables || !index || !opts || !out, "null pointer: tables, index, opts and out are required");
  std::string why = launch_why(n_jobs, n_rows, max_taps);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(out_len < 1, "requires out_len >= 1");
  why = rate_why(opts);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(max_order < -1, kNeedsOrder);
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
