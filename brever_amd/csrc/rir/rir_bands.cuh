// The band entry points of libbrever_rir.so (include/rir/brever_rir_bands.h): octave-band wall
// coefficients and a spherical-head ear. Included by rir.hip after its own kernel, whose helpers (bound,
// prefix_within, finite_positive) and constants it uses; nothing of that kernel changes.
//
//   host   build_axis_bands        build_axis with K amplitudes per row: (offset, e0 + e1, offset^2, amplitude of every
//                                  band); a candidate leaves only if every band's amplitude is 0.
//   device rir_bands_tile_kernel   rir_tile_kernel with C amplitudes per list entry, one instantiation per (K, mode):
//                                  an entry is (tau - t0, sin(pi frac) / pi with the sign of the integer part, cos and
//                                  sin of 2 pi (tau - t0) / W halved, C amplitudes); the consume phase computes
//                                  sinc times window once per (entry, tap) and does C FMAs. The list holds 512 entries
//                                  up to C = 4 and 256 above, so that LDS stays at or below 54 KB. In sphere mode the
//                                  delay of an image is (d + delta) fs/c, so the distance shell of a tile is wider by
//                                  the range of delta. Writes fp64 rows (C, taps + pad) per job.
//          rir_bands_combine_kernel one workgroup of 128 threads per (job, 1 024 output taps): per channel the needed
//                                  stretch of the row goes to LDS once (swizzled by one double per 16 so that lanes 8
//                                  doubles apart hit different banks), a lane is 8 consecutive taps and takes the
//                                  filter 16 taps at a time from 23 row values in registers: 128 FMAs per 23 LDS reads,
//                                  the coefficients uniform. Channels in order, filter taps in order.
#include "../../../include/rir/brever_rir_bands.h"

namespace {

constexpr int kMaxBands = BRV_RIR_BANDS_MAX_BANDS, kBGeom = BRV_RIR_BANDS_GEOM_DOUBLES;
constexpr int kCombTile = BRV_RIR_BANDS_COMBINE_TILE, kMaxFilter = BRV_RIR_BANDS_MAX_FILTER;
constexpr int kCombThreads = 128, kCombTaps = kCombTile/kCombThreads, kCombChunk = 16;
constexpr double kAlphaMin = 0.1, kThetaMinDeg = 150.0;
static_assert(kCombTaps == 8, "a lane of the combine kernel is 8 taps");

template <int K, bool kSphere>
__global__ __launch_bounds__(kThreads) void rir_bands_tile_kernel(const double* __restrict__ tab,
                                                                  const long long* __restrict__ index,
                                                                  long long n_rows, double fs, double c, double W,
                                                                  long long max_order, double rad, long long pad,
                                                                  double* __restrict__ scratch, long long scratch_len) {
  constexpr int C = kSphere ? 2*K : K;
  constexpr int RW = 3 + K;                      // doubles of a row
  constexpr int kCapB = C <= 4 ? 512 : 256;      // entries of the list: a pass adds at most kThreads
  static_assert(kCapB >= kThreads, "an empty list takes a pass");
  __shared__ double zd2[kMaxAxis];
  __shared__ double e_tau[kCapB], e_s[kCapB], e_cw[kCapB], e_sw[kCapB], e_amp[C][kCapB];
  __shared__ int wave_tot[2][kWaves];
  __shared__ double part[kWaves][kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long hdr = ix[0], nxl = ix[1], nyl = ix[2], nzl = ix[3], taps = ix[4], soff = ix[7];
  // an index that does not describe rows of this table, or channel rows inside the scratch, is not followed (uniform)
  if (hdr < 0 || nxl < 0 || nyl < 0 || nzl < 0 || nxl > kMaxAxis || nyl > kMaxAxis || nzl > kMaxAxis ||
      hdr > n_rows - 1 - nxl - nyl - nzl || taps < 1 || taps > BRV_RIR_MAX_TAPS || soff < 0) return;
  const long long T = taps + pad;                // taps of a channel row
  if ((long long)C*T > scratch_len || soff > scratch_len - (long long)C*T) return;
  const long long ntile = (T + kTile - 1)/kTile;
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
  const long long t_last = t0 + kTile - 1 < T - 1 ? t0 + kTile - 1 : T - 1;
  const double tau_lo = (double)t0 - halfW - kSlack, tau_hi = (double)t_last + halfW + kSlack;
  // tau = (d + delta) fs/c with -rad <= delta <= rad pi/2: the distances that can land in the tile
  const double less = kSphere ? 0.5*kPi*rad : 0.0, more = kSphere ? rad : 0.0;
  const double d_lo = tau_lo*metres - less > 0.0 ? tau_lo*metres - less : 0.0, d_hi = tau_hi*metres + more;
  const double lo2 = d_lo*d_lo, hi2 = d_hi*d_hi;

  for (int i = tid; i < nz; i += kThreads) zd2[i] = Z[(long long)i*RW + 2];
  int nxe = 0, nye = 0;
  for (int base = 0; base < nx; base += kThreads) {
    const int i = base + tid;
    nxe += __syncthreads_count(i < nx && X[(long long)i*RW + 2] <= hi2);
  }
  for (int base = 0; base < ny; base += kThreads) {
    const int i = base + tid;
    nye += __syncthreads_count(i < ny && Y[(long long)i*RW + 2] <= hi2);
  }
  __syncthreads();                               // zd2 is visible whatever nx and ny are
  const long long npairs = nz > 0 ? (long long)nxe*nye : 0;

  double sj[kLaneTaps], cj[kLaneTaps], acc[C][kLaneTaps];
#pragma unroll
  for (int k = 0; k < kLaneTaps; ++k) {
    sincospi(2.0*(double)(lane + 64*k)/W, &sj[k], &cj[k]);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch][k] = 0.0;
  }
  const double sign_j = (lane & 1) ? -1.0 : 1.0;   // of lane + 64 k as well
  int fill = 0, phase = 0;

  auto consume = [&]() {
    __syncthreads();
    for (int i = wave; i < fill; i += kWaves) {
      const double tr = e_tau[i], s = sign_j*e_s[i], cw = e_cw[i], sw = e_sw[i];
      double base[kLaneTaps];
#pragma unroll
      for (int k = 0; k < kLaneTaps; ++k) {
        const double u = (double)(lane + 64*k) - tr;
        const double win = __builtin_fma(sj[k], sw, __builtin_fma(cj[k], cw, 0.5));
        // 1/u as in rir_tile_kernel; u = 0 is sinc(0) window(0) = 1
        double r = __builtin_amdgcn_rcp(u);
        r = __builtin_fma(__builtin_fma(-u, r, 1.0), r, r);
        r = __builtin_fma(__builtin_fma(-u, r, 1.0), r, r);
        const double v = u == 0.0 ? 1.0 : s*r*win;
        base[k] = fabs(u) < halfW ? v : 0.0;
      }
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const double amp = e_amp[ch][i];
#pragma unroll
        for (int k = 0; k < kLaneTaps; ++k) acc[ch][k] = __builtin_fma(amp, base[k], acc[ch][k]);
      }
    }
    __syncthreads();
    fill = 0;
  };

  for (long long p0 = 0; p0 < npairs; p0 += kThreads) {
    const long long P = p0 + tid;
    int i0 = 0, i1 = 0, exy = 0;
    double dx = 0.0, dy = 0.0, rxy2 = 0.0;
    const double *xr = X, *yr = Y;
    if (P < npairs) {
      const int ixx = (int)(P/nye), iyy = (int)(P - (long long)ixx*nye);
      xr = X + (long long)ixx*RW;
      yr = Y + (long long)iyy*RW;
      dx = xr[0]; dy = yr[0];
      exy = (int)xr[1] + (int)yr[1];
      rxy2 = xr[2] + yr[2];
      if (rxy2 <= hi2) {
        i0 = bound<false>(zd2, nz, lo2 - rxy2);
        i1 = bound<true>(zd2, nz, hi2 - rxy2);
      }
    }
    for (;;) {
      const int m = i1 - i0 < 1 ? i1 - i0 : 1;
      // position of this lane's hit: lanes below it in the wave, then the waves below
      const unsigned long long below = (1ull << lane) - 1ull;
      const unsigned long long b = __ballot(m > 0);
      int pos = __popcll(b & below);
      if (lane == 0) wave_tot[phase][wave] = __popcll(b);
      __syncthreads();
      int total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int n = wave_tot[phase][w];
        if (w < wave) pos += n;
        total += n;
      }
      phase ^= 1;
      if (total == 0) break;                     // uniform: every lane's range is used up
      if (m > 0) {
        const double* zr = Z + (long long)i0*RW;
        const double dz = zr[0];
        const bool counted = max_order < 0 || exy + (int)zr[1] <= max_order;
        const double d = sqrt(rxy2 + zr[2]);
        const double cosang = (dx*ox + dy*oy + dz*oz)/d;
        const double spread = counted ? 1.0/(4.0*kPi*d) : 0.0;
        double path = d, g0, g1 = 0.0;           // gain of the channels k, and of K + k in sphere mode
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
        const double tau = path*fs/c;
        const double k = floor(tau), f = tau - k;
        const long long kr = (long long)k - t0;
        const double taur = tau - (double)t0;
        double sw, cw;
        sincospi(2.0*taur/W, &sw, &cw);
        const int e = fill + pos;                // < kCapB: fill <= kCapB - kThreads before a pass
        e_tau[e] = taur;
        e_s[e] = f == 0.0 ? 0.0 : sinpi(f)/kPi*((kr & 1) ? 1.0 : -1.0);
        e_cw[e] = 0.5*cw;
        e_sw[e] = 0.5*sw;
#pragma unroll
        for (int kb = 0; kb < K; ++kb) {
          const double A = xr[3 + kb]*yr[3 + kb]*zr[3 + kb];
          e_amp[kb][e] = A*g0;
          if (kSphere) e_amp[(kSphere ? K : 0) + kb][e] = A*g1;
        }
      }
      i0 += m;
      fill += total;
      if (fill > kCapB - kThreads) consume();
    }
  }
  if (fill > 0) consume();

  double* rows = scratch + soff;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
#pragma unroll
    for (int k = 0; k < kLaneTaps; ++k) part[wave][lane + 64*k] = acc[ch][k];
    __syncthreads();
    if (tid < kTile) {
      const long long t = t0 + tid;
      const double sum = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
      if (t < T) rows[(long long)ch*T + t] = sum;   // inside the scratch: soff + C T <= scratch_len
    }
    __syncthreads();
  }
}

// position in LDS of the local row index l: one double of padding per 16
__device__ __forceinline__ int comb_at(int l) { return l + (l >> 4); }

__global__ __launch_bounds__(kCombThreads) void rir_bands_combine_kernel(
    const double* __restrict__ scratch, long long scratch_len, const long long* __restrict__ index, int C,
    long long pad, const double* __restrict__ filters, int nf, float* __restrict__ out, long long out_len) {
  __shared__ double xs[kCombTile + kMaxFilter + (kCombTile + kMaxFilter)/16 + 1];
  const int tid = threadIdx.x;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long taps = ix[4], off = ix[5], stride = ix[6], soff = ix[7];
  if (taps < 1 || taps > BRV_RIR_MAX_TAPS || off < 0 || stride < 1 || soff < 0) return;
  const long long T = taps + pad;
  if ((long long)C*T > scratch_len || soff > scratch_len - (long long)C*T) return;
  const long long t0 = (long long)blockIdx.y*kCombTile;
  if (t0 >= taps) return;
  // the tap t0 + i needs the row at t0 + i + pad - m: local index l is the row index gbase + l, 0 <= l < n_local
  const long long gbase = t0 + pad - (nf - 1);
  const int n_local = kCombTile + nf - 1;
  double acc[kCombTaps];
#pragma unroll
  for (int i = 0; i < kCombTaps; ++i) acc[i] = 0.0;
  for (int ch = 0; ch < C; ++ch) {
    const double* row = scratch + soff + (long long)ch*T;
    const double* f = filters + (long long)ch*nf;
    __syncthreads();
    for (int l = tid; l < n_local; l += kCombThreads) {
      const long long g = gbase + l;
      xs[comb_at(l)] = g >= 0 && g < T ? row[g] : 0.0;
    }
    __syncthreads();
    for (int m0 = 0; m0 < nf; m0 += kCombChunk) {
      // w[j] is the row at q - (kCombChunk - 1) + j, q the row index of this lane's first tap at filter tap m0
      const int lq = kCombTaps*tid + (nf - 1) - m0;
      double w[kCombChunk - 1 + kCombTaps];
#pragma unroll
      for (int j = 0; j < kCombChunk - 1 + kCombTaps; ++j) w[j] = xs[comb_at(lq - (kCombChunk - 1) + j)];
#pragma unroll
      for (int mm = 0; mm < kCombChunk; ++mm) {
        const double fm = f[m0 + mm];
#pragma unroll
        for (int i = 0; i < kCombTaps; ++i) acc[i] = __builtin_fma(fm, w[kCombChunk - 1 + i - mm], acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kCombTaps; ++i) {
    const long long t = t0 + (long long)kCombTaps*tid + i;
    if (t < taps) {
      const long long o = off + t*stride;        // taps, stride and off are bounded: no overflow below 2^63
      if (o < out_len) out[o] = (float)acc[i];
    }
  }
}

struct BandOpts {
  double fs, c, W, rad;
  int K, mode, C;
  int64_t pad;
};

// "" or why the options are refused
std::string read_band_opts(const double* opts, BandOpts* o) {
  if (!opts) return "null pointer: opts is required";
  if (!finite_positive(opts[0]) || !finite_positive(opts[1])) return "requires fs > 0 and c > 0, both finite";
  if (!(opts[2] >= 2.0) || !(opts[2] <= 1e6)) return "requires 2 <= W <= 1e6 (the window in samples)";
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

struct BandRow { double d, count, d2, amp[kMaxBands]; };

// a job's view of the host arrays
struct BandJob {
  const double *L, *s, *r, *o, *beta;
  double a;
  int64_t taps, off, stride;
};

BandJob band_job_at(const double* geom, const int64_t* shape, int64_t j) {
  const double* g = geom + j*kBGeom;
  const int64_t* h = shape + j*kShape;
  return BandJob{g, g + 3, g + 6, g + 9, g + 13, g[12], h[0], h[1], h[2]};
}

std::string check_band_batch(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                             int64_t max_order, BandOpts* o) {
  if (!geom || !shape || !opts) return "null pointer: geom, shape and opts are required";
  if (n_jobs < 1 || n_jobs > BRV_RIR_MAX_JOBS) return "requires 1 <= n_jobs <= " + std::to_string(BRV_RIR_MAX_JOBS);
  const std::string why = read_band_opts(opts, o);
  if (!why.empty()) return why;
  if (max_order < -1) return "requires max_order >= -1";
  const bool sphere = o->mode == BRV_RIR_BANDS_SPHERE;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const BandJob q = band_job_at(geom, shape, j);
    const std::string at = "job " + std::to_string(j) + ": ";
    double dist2 = 0.0, norm2 = 0.0;
    for (int k = 0; k < 3; ++k) {
      if (!finite_positive(q.L[k])) return at + "requires room dimensions > 0, finite";
      for (int b = 0; b < o->K; ++b)
        for (int w = 0; w < 2; ++w) {
          const double v = q.beta[6*b + 2*k + w];
          if (!(v >= 0.0) || !(v <= 1.0)) return at + "requires beta in [0, 1] in every band";
        }
      if (!(q.s[k] > 0.0) || !(q.s[k] < q.L[k])) return at + "the source is outside the box or on a wall";
      if (!(q.r[k] > 0.0) || !(q.r[k] < q.L[k])) return at + "the receiver is outside the box or on a wall";
      if (sphere && (!(q.r[k] - o->rad > 0.0) || !(q.r[k] + o->rad < q.L[k])))
        return at + "the head reaches a wall: its centre is nearer than the head radius";
      dist2 += (q.s[k] - q.r[k])*(q.s[k] - q.r[k]);
      norm2 += q.o[k]*q.o[k];
    }
    if (sphere && !(dist2 > o->rad*o->rad)) return at + "the source is inside the sphere of the head";
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
bool build_axis_bands(const BandJob& q, int k, const BandOpts& o, int64_t max_order, std::vector<BandRow>* rows) {
  const double L = q.L[k];
  // the last tap of a channel row is taps + pad - 1, and delta >= -rad brings an image of distance reach in
  const double reach = (o.c/o.fs)*((double)(q.taps + o.pad - 1) + 0.5*o.W + kSlack) +
                       (o.mode == BRV_RIR_BANDS_SPHERE ? o.rad : 0.0);
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
      BandRow row{d, (double)(e0 + e1), d*d, {}};
      bool any = false;
      for (int b = 0; b < o.K; ++b) {
        row.amp[b] = pow(q.beta[6*b + 2*k], (double)e0)*pow(q.beta[6*b + 2*k + 1], (double)e1);   // pow(0, 0) = 1
        any = any || row.amp[b] != 0.0;
      }
      if (any) rows->push_back(row);
    }
  }
  if ((long long)rows->size() > kMaxAxis) return false;
  std::stable_sort(rows->begin(), rows->end(), [](const BandRow& u, const BandRow& v) { return u.d2 < v.d2; });
  return true;
}

using BandsTileKernel = void (*)(const double*, const long long*, long long, double, double, double, long long, double,
                                 long long, double*, long long);

template <int K> BandsTileKernel bands_tile_kernel(int mode) {
  return mode == BRV_RIR_BANDS_SPHERE ? rir_bands_tile_kernel<K, true> : rir_bands_tile_kernel<K, false>;
}

BandsTileKernel bands_tile_kernel_of(int K, int mode) {
  switch (K) {
    case 1: return bands_tile_kernel<1>(mode);
    case 2: return bands_tile_kernel<2>(mode);
    case 3: return bands_tile_kernel<3>(mode);
    case 4: return bands_tile_kernel<4>(mode);
    case 5: return bands_tile_kernel<5>(mode);
    case 6: return bands_tile_kernel<6>(mode);
    case 7: return bands_tile_kernel<7>(mode);
    case 8: return bands_tile_kernel<8>(mode);
  }
  return nullptr;
}

}  // namespace

extern "C" {

int64_t brv_rir_bands_table_rows(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                                 int64_t max_order) {
  BandOpts o;
  const std::string why = check_band_batch(geom, shape, n_jobs, opts, max_order, &o);
  if (!why.empty()) return brv::fail(-1, why);
  std::vector<BandRow> rows;
  int64_t total = 0;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const BandJob q = band_job_at(geom, shape, j);
    total += 1;
    for (int k = 0; k < 3; ++k) {
      if (!build_axis_bands(q, k, o, max_order, &rows))
        return brv::fail(-1, "job " + std::to_string(j) + ": " + kTooMany);
      total += (int64_t)rows.size();
    }
  }
  return total;
}

int brv_rir_bands_build_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                               int64_t max_order, double* rows_out, int64_t* index, int64_t n_rows) {
  BRV_REFUSE(!rows_out || !index, "null pointer: rows and index are required");
  BandOpts o;
  const std::string why = check_band_batch(geom, shape, n_jobs, opts, max_order, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(n_rows < 1, "requires n_rows >= 1: the value of brv_rir_bands_table_rows");
  const int RW = 3 + o.K;
  std::vector<BandRow> rows;
  int64_t at = 0, soff = 0;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const BandJob q = band_job_at(geom, shape, j);
    int64_t* ix = index + j*kIdx;
    BRV_REFUSE(at + 1 > n_rows, "n_rows is not what brv_rir_bands_table_rows gives for this batch");
    ix[0] = at;
    double* h = rows_out + at*RW;
    for (int i = 0; i < RW; ++i) h[i] = 0.0;
    h[0] = q.o[0]; h[1] = q.o[1]; h[2] = q.o[2]; h[3] = q.a;
    at += 1;
    for (int k = 0; k < 3; ++k) {
      BRV_REFUSE(!build_axis_bands(q, k, o, max_order, &rows), "job " + std::to_string(j) + ": " + kTooMany);
      BRV_REFUSE(at + (int64_t)rows.size() > n_rows,
                 "n_rows is not what brv_rir_bands_table_rows gives for this batch");
      ix[1 + k] = (int64_t)rows.size();
      for (const BandRow& r : rows) {
        double* w = rows_out + at*RW;
        w[0] = r.d; w[1] = r.count; w[2] = r.d2;
        for (int b = 0; b < o.K; ++b) w[3 + b] = r.amp[b];
        at += 1;
      }
    }
    ix[4] = q.taps; ix[5] = q.off; ix[6] = q.stride; ix[7] = soff;
    soff += (int64_t)o.C*(q.taps + o.pad);
  }
  BRV_REFUSE(at != n_rows, "n_rows is not what brv_rir_bands_table_rows gives for this batch");
  return 0;
}

int brv_rir_bands_channels(const double* tables, const int64_t* index, int64_t n_jobs, int64_t n_rows,
                           int64_t max_taps, const double* opts, int64_t max_order, double* scratch,
                           int64_t scratch_len, brv_stream_t stream) {
  BRV_REFUSE(!tables || !index || !opts || !scratch, "null pointer: tables, index, opts and scratch are required");
  BRV_REFUSE(n_jobs < 1 || n_jobs > BRV_RIR_MAX_JOBS, "requires 1 <= n_jobs <= " + std::to_string(BRV_RIR_MAX_JOBS));
  BRV_REFUSE(n_rows < 1, "requires n_rows >= 1");
  BRV_REFUSE(max_taps < 1 || max_taps > BRV_RIR_MAX_TAPS,
             "requires 1 <= max_taps <= " + std::to_string(BRV_RIR_MAX_TAPS));
  BandOpts o;
  const std::string why = read_band_opts(opts, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(max_order < -1, "requires max_order >= -1");
  BRV_REFUSE(scratch_len < (int64_t)o.C*(max_taps + o.pad),
             "the scratch is too small: a job of max_taps needs C (max_taps + pad) doubles");
  const int64_t ntile = (max_taps + o.pad + kTile - 1)/kTile;  // <= 8200 <= the limit of gridDim.y
  const BandsTileKernel kernel = bands_tile_kernel_of(o.K, o.mode);
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
  BRV_REFUSE(n_jobs < 1 || n_jobs > BRV_RIR_MAX_JOBS, "requires 1 <= n_jobs <= " + std::to_string(BRV_RIR_MAX_JOBS));
  BRV_REFUSE(max_taps < 1 || max_taps > BRV_RIR_MAX_TAPS,
             "requires 1 <= max_taps <= " + std::to_string(BRV_RIR_MAX_TAPS));
  BandOpts o;
  const std::string why = read_band_opts(opts, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(n_filter < kCombChunk || n_filter > kMaxFilter || n_filter%kCombChunk != 0,
             "requires n_filter a multiple of 16 in [16, " + std::to_string(kMaxFilter) + "]");
  BRV_REFUSE(out_len < 1, "requires out_len >= 1");
  BRV_REFUSE(scratch_len < (int64_t)o.C*(max_taps + o.pad),
             "the scratch is too small: a job of max_taps needs C (max_taps + pad) doubles");
  const int64_t ntile = (max_taps + kCombTile - 1)/kCombTile;
  hipLaunchKernelGGL(rir_bands_combine_kernel, dim3((unsigned)n_jobs, (unsigned)ntile), dim3(kCombThreads), 0,
                     (hipStream_t)stream, scratch, (long long)scratch_len, (const long long*)index, o.C,
                     (long long)o.pad, filters, (int)n_filter, out, (long long)out_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}
