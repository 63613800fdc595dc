// The band entry points of libbrever_rir.so (include/rir/brever_rir_bands.h): octave-band wall
// coefficients and a spherical-head ear. Included by rir.hip after its own kernel; the walk, the list entry and the
// tap weights are those of rir_shell.cuh, the host side that of rir_host.h.
//
//   device rir_bands_tile_kernel   the walk of rir_tile_kernel with C amplitudes per list entry, one instantiation per
//                                  (K, mode): an entry is that of delay_entry and C amplitudes; the consume phase
//                                  computes sinc times window once per (entry, tap) and does C FMAs. The list holds
//                                  512 entries up to C = 4 and 256 above, so that LDS stays at or below 54 KB. In
//                                  sphere mode the delay of an image is (d + delta) fs/c, so the distance shell of a
//                                  tile is wider by the range of delta. Writes fp64 rows (C, taps + pad) per job.
//          rir_bands_combine_kernel one workgroup of 128 threads per (job, 1 024 output taps): the FIR tile of
//                                  rir_fir.cuh, one filter per channel row. Channels in order, filter taps in order.
#include "../../../include/rir/brever_rir_bands.h"
#include "rir_fir.cuh"

namespace {

constexpr int kBGeom = BRV_RIR_BANDS_GEOM_DOUBLES;
constexpr double kAlphaMin = 0.1, kThetaMinDeg = 150.0;
static_assert(BRV_RIR_BANDS_COMBINE_TILE == kFirTile, "the combine kernel's tile is the FIR tile");

template <int K, bool kSphere>
__global__ __launch_bounds__(kThreads) void rir_bands_tile_kernel(const double* __restrict__ tab,
                                                                  const long long* __restrict__ index,
                                                                  long long n_rows, double fs, double c, double W,
                                                                  long long max_order, double rad, long long pad,
                                                                  double* __restrict__ scratch, long long scratch_len) {
  constexpr int C = kSphere ? 2*K : K;
  constexpr int RW = 3 + K;                      // a row is (offset, count, offset^2, K amplitudes)
  constexpr int kCapB = C <= 4 ? 512 : 256;      // entries of the list: a pass adds at most kThreads
  __shared__ double zd2[kMaxAxis];
  __shared__ double e_tau[kCapB], e_s[kCapB], e_cw[kCapB], e_sw[kCapB], e_amp[C][kCapB];
  __shared__ int wave_tot[2][kWaves];
  __shared__ double part[kWaves][kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long soff = ix[7];
  // an index that does not describe rows of this table, or channel rows inside the scratch, is not followed (uniform)
  Shell s;
  if (!shell_rows<RW>(tab, ix, n_rows, pad, &s) || soff < 0) return;
  const long long T = s.T;                       // taps of a channel row
  if ((long long)C*T > scratch_len || soff > scratch_len - (long long)C*T) return;
  const double ox = s.H[0], oy = s.H[1], oz = s.H[2], a = s.H[3];
  // tau = (d + delta) fs/c with -rad <= delta <= rad pi/2: the distances that can land in the tile
  shell_tile<RW, 2>(&s, fs, c, W, kSphere ? 0.5*kPi*rad : 0.0, kSphere ? rad : 0.0, zd2);

  const LaneTaps lt = lane_taps(lane, W);
  double acc[C][kLaneTaps];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
#pragma unroll
    for (int k = 0; k < kLaneTaps; ++k) acc[ch][k] = 0.0;
  }

  auto consume = [&](int fill) {
    __syncthreads();
    for (int i = wave; i < fill; i += kWaves) {
      double base[kLaneTaps];                    // u = 0 is sinc(0) window(0) = 1
      tap_weights(lt, lane, s.halfW, e_tau[i], e_s[i], 1.0, e_cw[i], e_sw[i], base);
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const double amp = e_amp[ch][i];
#pragma unroll
        for (int k = 0; k < kLaneTaps; ++k) acc[ch][k] = __builtin_fma(amp, base[k], acc[ch][k]);
      }
    }
    __syncthreads();
  };

  auto append = [&](int e, const Hit& h) {
    const double d = h.d;
    const double cosang = (h.dx*ox + h.dy*oy + h.dz*oz)/d;
    const double spread = h.counted ? 1.0/(4.0*kPi*d) : 0.0;
    double path = d, g0, g1 = 0.0;               // gain of the channels k, and of K + k in sphere mode
    if (kSphere) {
      const double ct = cosang < -1.0 ? -1.0 : cosang > 1.0 ? 1.0 : cosang;
      const double theta = acos(ct);
      const double alpha = (1.0 + 0.5*kAlphaMin) + (1.0 - 0.5*kAlphaMin)*cos(theta*(180.0/kThetaMinDeg));
      path = d + (theta < 0.5*kPi ? -rad*ct : rad*(theta - 0.5*kPi));
      g0 = alpha*spread;
      g1 = (1.0 - alpha)*spread;
    } else {
      g0 = (a + (1.0 - a)*cosang)*spread;
    }
    const Delay dl = delay_entry(path*fs/c, s.t0, W, 1.0);
    e_tau[e] = dl.taur;
    e_s[e] = dl.s;
    e_cw[e] = dl.cw;
    e_sw[e] = dl.sw;
#pragma unroll
    for (int kb = 0; kb < K; ++kb) {
      const double A = h.xr[3 + kb]*h.yr[3 + kb]*h.zr[3 + kb];
      e_amp[kb][e] = A*g0;
      if (kSphere) e_amp[(kSphere ? K : 0) + kb][e] = A*g1;
    }
  };

  shell_walk<RW, 1, 2, 3, kCapB>(s, zd2, wave_tot, max_order, append, consume);

  double* rows = scratch + soff;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const double sum = wave_sum(part, acc[ch]);
    if (tid < kTile) {
      const long long t = s.t0 + tid;
      if (t < T) rows[(long long)ch*T + t] = sum;   // inside the scratch: soff + C T <= scratch_len
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kFirThreads) void rir_bands_combine_kernel(
    const double* __restrict__ scratch, long long scratch_len, const long long* __restrict__ index, int C,
    long long pad, const double* __restrict__ filters, int nf, float* __restrict__ out, long long out_len) {
  __shared__ double xs[fir_lds(kMaxFilter)];
  const int tid = threadIdx.x;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long taps = ix[4], off = ix[5], stride = ix[6], soff = ix[7];
  if (taps < 1 || taps > BRV_RIR_MAX_TAPS || off < 0 || stride < 1 || soff < 0) return;
  const long long T = taps + pad;
  if ((long long)C*T > scratch_len || soff > scratch_len - (long long)C*T) return;
  const long long t0 = (long long)blockIdx.y*kFirTile;
  if (t0 >= taps) return;
  double acc[1][kFirTaps];
#pragma unroll
  for (int i = 0; i < kFirTaps; ++i) acc[0][i] = 0.0;
  // the tap t0 + i needs the row at t0 + i + pad - m
  for (int ch = 0; ch < C; ++ch) {
    const double* const f[1] = {filters + (long long)ch*nf};
    fir_tile<1>(xs, scratch + soff + (long long)ch*T, T, t0 + pad, nf, f, acc);
  }
#pragma unroll
  for (int i = 0; i < kFirTaps; ++i) {
    const long long t = t0 + (long long)kFirTaps*tid + i;
    if (t < taps) {
      const long long o = off + t*stride;        // taps, stride and off are bounded: no overflow below 2^63
      if (o < out_len) out[o] = (float)acc[0][i];
    }
  }
}

// "" or why the options are refused
std::string read_band_opts(const double* opts, Opts* o) {
  if (!opts) return "null pointer: opts is required";
  const std::string why = rate_why(opts);
  if (!why.empty()) return why;
  if (!(opts[3] >= 1.0) || !(opts[3] <= (double)kMaxBands) || opts[3] != floor(opts[3]))
    return "requires 1 <= K <= " + std::to_string(kMaxBands) + " (the octave bands)";
  if (opts[4] != (double)BRV_RIR_BANDS_PATTERN && opts[4] != (double)BRV_RIR_BANDS_SPHERE)
    return "the ear model is neither BRV_RIR_BANDS_PATTERN (0) nor BRV_RIR_BANDS_SPHERE (1)";
  if (!(opts[6] >= 0.0) || !(opts[6] <= (double)(kMaxFilter/2)) || opts[6] != floor(opts[6]))
    return "requires 0 <= pad <= " + std::to_string(kMaxFilter/2);
  o->fs = opts[0]; o->c = opts[1]; o->W = opts[2];
  o->K = (int)opts[3]; o->mode = (int)opts[4]; o->rad = opts[5]; o->pad = (int64_t)opts[6];
  o->C = o->mode == BRV_RIR_BANDS_SPHERE ? 2*o->K : o->K;
  if (!(125.0*(double)(1 << (o->K - 1)) < 0.5*o->fs))
    return "requires the centre of the last band, 125 * 2^(K-1) Hz, below fs/2";
  if (o->mode == BRV_RIR_BANDS_SPHERE && !(finite_positive(o->rad) && o->rad <= 1.0))
    return "requires a head radius in (0, 1] m in sphere mode";
  return "";
}

// The batch checked, then its tables counted (rows_out null) or written: "" or why it is refused.
std::string band_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                        int64_t max_order, double* rows_out, int64_t* index, int64_t n_rows, int64_t* total) {
  if (!geom || !shape || !opts) return "null pointer: geom, shape and opts are required";
  Opts o;
  std::string why = jobs_why(n_jobs);
  if (why.empty()) why = read_band_opts(opts, &o);
  if (why.empty() && max_order < -1) why = kNeedsOrder;
  if (!why.empty()) return why;
  const auto job_at = [&](int64_t j) {
    const double* g = geom + j*kBGeom;
    const int64_t* h = shape + j*kShape;
    return Job{g, g + 13, g + 3, g + 6, g + 9, nullptr, g[12], h[0], h[1], h[2], 0};
  };
  int64_t soff = 0;
  const auto head = [&](int64_t, const Job& q, double* h, int64_t* ix) {
    h[0] = q.o[0]; h[1] = q.o[1]; h[2] = q.o[2]; h[3] = q.a;
    ix[4] = q.taps; ix[5] = q.off; ix[6] = q.stride; ix[7] = soff;
    soff += (int64_t)o.C*(q.taps + o.pad);
  };
  return with_bands(o.K, [&](auto k) {
    return tables<decltype(k)::value>(n_jobs, job_at, kBands, o, max_order, "brv_rir_bands_table_rows", rows_out, index,
                                      n_rows, total, head);
  });
}

using BandsTileKernel = void (*)(const double*, const long long*, long long, double, double, double, long long, double,
                                 long long, double*, long long);

}  // namespace

extern "C" {

int64_t brv_rir_bands_table_rows(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                                 int64_t max_order) {
  int64_t total = 0;
  const std::string why = band_tables(geom, shape, n_jobs, opts, max_order, nullptr, nullptr, 0, &total);
  return why.empty() ? total : brv::fail(-1, why);
}

int brv_rir_bands_build_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                               int64_t max_order, double* rows_out, int64_t* index, int64_t n_rows) {
  BRV_REFUSE(!rows_out || !index, "null pointer: rows and index are required");
  int64_t total = 0;
  const std::string why = band_tables(geom, shape, n_jobs, opts, max_order, rows_out, index, n_rows, &total);
  BRV_REFUSE(!why.empty(), why);
  return 0;
}

int brv_rir_bands_channels(const double* tables, const int64_t* index, int64_t n_jobs, int64_t n_rows,
                           int64_t max_taps, const double* opts, int64_t max_order, double* scratch,
                           int64_t scratch_len, brv_stream_t stream) {
  BRV_REFUSE(!tables || !index || !opts || !scratch, "null pointer: tables, index, opts and scratch are required");
  Opts o;
  std::string why = launch_why(n_jobs, n_rows, max_taps);
  if (why.empty()) why = read_band_opts(opts, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(max_order < -1, kNeedsOrder);
  BRV_REFUSE(scratch_len < (int64_t)o.C*(max_taps + o.pad),
             "the scratch is too small: a job of max_taps needs C (max_taps + pad) doubles");
  const int64_t ntile = (max_taps + o.pad + kTile - 1)/kTile;  // <= 8200 <= the limit of gridDim.y
  const BandsTileKernel kernel = with_bands(o.K, [&](auto k) -> BandsTileKernel {
    constexpr int K = decltype(k)::value;
    return o.mode == BRV_RIR_BANDS_SPHERE ? rir_bands_tile_kernel<K, true> : rir_bands_tile_kernel<K, false>;
  });
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_jobs, (unsigned)ntile), dim3(kThreads), 0, (hipStream_t)stream, tables,
                     (const long long*)index, (long long)n_rows, o.fs, o.c, o.W, (long long)max_order, o.rad,
                     (long long)o.pad, scratch, (long long)scratch_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_rir_bands_combine(const double* scratch, int64_t scratch_len, const int64_t* index, int64_t n_jobs,
                          int64_t max_taps, const double* opts, const double* filters, int64_t n_filter, float* out,
                          int64_t out_len, brv_stream_t stream) {
  BRV_REFUSE(!scratch || !index || !opts || !filters || !out,
             "null pointer: scratch, index, opts, filters and out are required");
  Opts o;
  std::string why = launch_why(n_jobs, 1, max_taps);
  if (why.empty()) why = read_band_opts(opts, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(n_filter < kFirChunk || n_filter > kMaxFilter || n_filter%kFirChunk != 0,
             "requires n_filter a multiple of 16 in [16, " + std::to_string(kMaxFilter) + "]");
  BRV_REFUSE(out_len < 1, "requires out_len >= 1");
  BRV_REFUSE(scratch_len < (int64_t)o.C*(max_taps + o.pad),
             "the scratch is too small: a job of max_taps needs C (max_taps + pad) doubles");
  const int64_t ntile = (max_taps + kFirTile - 1)/kFirTile;
  hipLaunchKernelGGL(rir_bands_combine_kernel, dim3((unsigned)n_jobs, (unsigned)ntile), dim3(kFirThreads), 0,
                     (hipStream_t)stream, scratch, (long long)scratch_len, (const long long*)index, o.C,
                     (long long)o.pad, filters, (int)n_filter, out, (long long)out_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}
