// The measured-ear entry points of libbrever_rir.so (include/rir/brever_rir_hrir.h): the ear is a set
// of measured HRIRs, an image goes to the row of the measured direction nearest to its arrival, and the rows are
// folded with that direction's HRIR pair. Included by rir.hip after rir_bands.cuh, whose helpers (read_band_opts,
// build_axis_bands, comb_at) and constants it uses; nothing of the kernels before it changes.
//
//   host   build_axis_bands       as it is, in pattern mode: the reach and the rows of the band tables.
//   device rir_hrir_tile_kernel   the shell and the compaction of rir_bands_tile_kernel (pattern mode, amplitude
//                                 A_k / (4 pi d)); the lane that appends an entry finds its direction, the argmax of
//                                 q.p_j over the D directions read uniformly across the wave (strictly greater wins, so
//                                 ties go to the lowest j), and writes the key (direction, list position). Consume:
//                                 the keys are sorted in LDS (bitonic network; they are distinct, so the order is that
//                                 of the directions and, inside one, of the list), the sorted list is cut into four
//                                 slices at the changes of direction nearest to its quarters, wave w walks slice w with
//                                 K x 2 accumulators per lane and adds them to the direction's rows (load, add, store)
//                                 whenever the direction changes. A direction of a round belongs to one wave and the
//                                 rounds are separated by barriers, so every tap of a row sees its additions in one
//                                 order, that of the job's own tables.
//          rir_hrir_fold_kernel   one workgroup of 128 threads per (job, 1 024 taps, band): per direction the stretch
//                                 of the row goes to LDS as in rir_bands_combine_kernel (the same swizzle), a lane is 8
//                                 consecutive taps and takes the HRIR 16 taps at a time from 23 row values in
//                                 registers, for both ears: 256 FMAs per 23 LDS reads, the coefficients uniform.
//                                 Empty stretches are not passed over: hardly any is empty at 8 000 taps (DESIGN.md
//                                 5o).
#include <limits.h>

#include "../../../include/rir/brever_rir_hrir.h"

namespace {

constexpr int kMaxDirs = BRV_RIR_HRIR_MAX_DIRS, kMaxHrir = BRV_RIR_HRIR_MAX_TAPS, kHGeom = BRV_RIR_HRIR_GEOM_DOUBLES,
              kHShape = BRV_RIR_HRIR_SHAPE_WORDS, kFoldTile = BRV_RIR_HRIR_FOLD_TILE;
constexpr int kFoldThreads = 128, kFoldTaps = kFoldTile/kFoldThreads, kFoldChunk = 16;
static_assert(kFoldTaps == 8, "a lane of the fold kernel is 8 taps");
static_assert(kMaxHrir%kFoldChunk == 0, "the longest HRIR is whole chunks");

template <int K>
__global__ __launch_bounds__(kThreads) void rir_hrir_tile_kernel(const double* __restrict__ tab,
                                                                 const long long* __restrict__ index,
                                                                 long long n_rows, double fs, double c, double W,
                                                                 long long max_order, long long pad,
                                                                 const double* __restrict__ dirs, int D,
                                                                 double* __restrict__ scratch, long long scratch_len) {
  constexpr int RW = 3 + K;                      // doubles of a row
  constexpr int kLog = K <= 6 ? 9 : 8;           // a list of 512 entries up to K = 6 and 256 above: LDS <= 54 KB
  constexpr int kCapH = 1 << kLog;
  static_assert(kCapH >= kThreads, "an empty list takes a pass");
  static_assert(kMaxDirs <= (INT_MAX >> kLog), "a key holds a direction and a list position");
  __shared__ double zd2[kMaxAxis];
  __shared__ double e_tau[kCapH], e_s[kCapH], e_cw[kCapH], e_sw[kCapH], e_amp[K][kCapH];
  __shared__ int ord[kCapH];
  __shared__ int wave_tot[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long hdr = ix[0], nxl = ix[1], nyl = ix[2], nzl = ix[3], taps = ix[4], doff = ix[5];
  // an index that does not describe rows of this table, or direction rows inside the scratch, is not followed (uniform)
  if (hdr < 0 || nxl < 0 || nyl < 0 || nzl < 0 || nxl > kMaxAxis || nyl > kMaxAxis || nzl > kMaxAxis ||
      hdr > n_rows - 1 - nxl - nyl - nzl || taps < 1 || taps > BRV_RIR_MAX_TAPS || doff < 0 || D < 1 || D > kMaxDirs)
    return;
  const long long T = taps + pad;                // taps of a direction row
  const long long need = (long long)K*D*T;       // < 2^3 2^11 2^21
  if (need > scratch_len || doff > scratch_len - need) return;
  const long long ntile = (T + kTile - 1)/kTile;
  const long long tile = ntile - 1 - (long long)blockIdx.y;
  if (tile < 0) return;
  const long long t0 = tile*kTile;
  const int nx = (int)nxl, ny = (int)nyl, nz = (int)nzl;
  const double* H = tab + hdr*RW;
  const double* X = H + RW;
  const double* Y = X + (long long)nx*RW;
  const double* Z = Y + (long long)ny*RW;
  const double fx = H[0], fy = H[1], lx = H[2], ly = H[3];   // front and left, both horizontal
  const double halfW = 0.5*W, metres = c/fs;
  const long long t_last = t0 + kTile - 1 < T - 1 ? t0 + kTile - 1 : T - 1;
  const double tau_lo = (double)t0 - halfW - kSlack, tau_hi = (double)t_last + halfW + kSlack;
  const double d_lo = tau_lo*metres > 0.0 ? tau_lo*metres : 0.0, d_hi = tau_hi*metres;
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

  double sj[kLaneTaps], cj[kLaneTaps], acc[K][kLaneTaps];
#pragma unroll
  for (int k = 0; k < kLaneTaps; ++k) {
    sincospi(2.0*(double)(lane + 64*k)/W, &sj[k], &cj[k]);
#pragma unroll
    for (int ch = 0; ch < K; ++ch) acc[ch][k] = 0.0;
  }
  const double sign_j = (lane & 1) ? -1.0 : 1.0;   // of lane + 64 k as well
  double* rows = scratch + doff;
  int fill = 0, phase = 0;

  // add the accumulators to the rows of direction dj and clear them (dj uniform across the wave)
  // (Loading one direction ahead of the store -- a second set of K x 2 registers -- was measured: 205 VGPRs and two
  // waves per SIMD instead of three at K = 6, 521 ms against 483 ms on the workload of DESIGN.md 5o.)
  auto flush = [&](int dj) {
#pragma unroll
    for (int ch = 0; ch < K; ++ch) {
#pragma unroll
      for (int k = 0; k < kLaneTaps; ++k) {
        const long long t = t0 + lane + 64*k;
        if (t < T) {
          double* at = rows + ((long long)ch*D + dj)*T + t;    // inside the scratch: doff + K D T <= scratch_len
          *at = *at + acc[ch][k];
        }
        acc[ch][k] = 0.0;
      }
    }
  };

  // first position of wave w's slice of the sorted list: the quarter point, moved up to a change of direction
  auto slice = [&](int w) {
    if (w >= kWaves) return fill;
    int p = (int)((long long)w*fill/kWaves);
    while (p > 0 && p < fill && (ord[p] >> kLog) == (ord[p - 1] >> kLog)) ++p;
    return p;
  };

  auto consume = [&]() {
    int P = 1;
    while (P < fill) P <<= 1;                    // <= kCapH, a power of two
    for (int i = fill + tid; i < P; i += kThreads) ord[i] = INT_MAX;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (P >> 1); t += kThreads) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
          const int a = ord[i], b = ord[l];
          if ((a > b) == ((i & k) == 0)) { ord[i] = b; ord[l] = a; }
        }
        __syncthreads();
      }
    }
    const int p0 = slice(wave), p1 = slice(wave + 1);
    int cur = -1;
    for (int p = p0; p < p1; ++p) {
      const int key = __builtin_amdgcn_readfirstlane(ord[p]);
      const int i = key & (kCapH - 1), dj = key >> kLog;
      if (dj != cur) {
        if (cur >= 0) flush(cur);
        cur = dj;
      }
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
      for (int ch = 0; ch < K; ++ch) {
        const double amp = e_amp[ch][i];
#pragma unroll
        for (int k = 0; k < kLaneTaps; ++k) acc[ch][k] = __builtin_fma(amp, base[k], acc[ch][k]);
      }
    }
    if (cur >= 0) flush(cur);
    __syncthreads();                             // the rows are the next round's, the list is free
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
    const double qf = dx*fx + dy*fy, ql = dx*lx + dy*ly;     // v.f and v.l: the same for every z of the pair
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
        const double spread = counted ? 1.0/(4.0*kPi*d) : 0.0;
        // the measured direction nearest to the arrival q = (v.f, v.l, v.u), u = (0, 0, 1); j is uniform
        double best = dirs[0]*qf + dirs[1]*ql + dirs[2]*dz;
        int dj = 0;
        for (int j = 1; j < D; ++j) {
          const double dot = dirs[3*j]*qf + dirs[3*j + 1]*ql + dirs[3*j + 2]*dz;
          if (dot > best) { best = dot; dj = j; }
        }
        const double tau = d*fs/c;
        const double k = floor(tau), f = tau - k;
        const long long kr = (long long)k - t0;
        const double taur = tau - (double)t0;
        double sw, cw;
        sincospi(2.0*taur/W, &sw, &cw);
        const int e = fill + pos;                // < kCapH: fill <= kCapH - kThreads before a pass
        e_tau[e] = taur;
        e_s[e] = f == 0.0 ? 0.0 : sinpi(f)/kPi*((kr & 1) ? 1.0 : -1.0);
        e_cw[e] = 0.5*cw;
        e_sw[e] = 0.5*sw;
        ord[e] = (dj << kLog) | e;
#pragma unroll
        for (int kb = 0; kb < K; ++kb) e_amp[kb][e] = xr[3 + kb]*yr[3 + kb]*zr[3 + kb]*spread;
      }
      i0 += m;
      fill += total;
      if (fill > kCapH - kThreads) consume();
    }
  }
  if (fill > 0) consume();
}

__global__ __launch_bounds__(kFoldThreads) void rir_hrir_fold_kernel(
    const double* __restrict__ dir, long long dir_len, const long long* __restrict__ index, int K, int D,
    long long pad, const double* __restrict__ hrirs, int nf, double* __restrict__ fold, long long fold_len) {
  __shared__ double xs[kFoldTile + kMaxHrir + (kFoldTile + kMaxHrir)/16 + 1];
  const int tid = threadIdx.x, k = blockIdx.z;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long taps = ix[4], doff = ix[5], foff = ix[7];
  if (taps < 1 || taps > BRV_RIR_MAX_TAPS || doff < 0 || foff < 0 || k >= K) return;
  const long long T = taps + pad;
  const long long need = (long long)K*D*T;
  if (need > dir_len || doff > dir_len - need) return;
  if (2ll*K*T > fold_len || foff > fold_len - 2ll*K*T) return;
  const long long t0 = (long long)blockIdx.y*kFoldTile;
  if (t0 >= T) return;
  // the tap t0 + i needs the row at t0 + i - m: local index l is the row index gbase + l, 0 <= l < n_local
  const long long gbase = t0 - (nf - 1);
  const int n_local = kFoldTile + nf - 1;
  double acc[2][kFoldTaps];
#pragma unroll
  for (int i = 0; i < kFoldTaps; ++i) acc[0][i] = acc[1][i] = 0.0;
  for (int j = 0; j < D; ++j) {
    const double* row = dir + doff + ((long long)k*D + j)*T;
    __syncthreads();
    for (int l = tid; l < n_local; l += kFoldThreads) {
      const long long g = gbase + l;
      xs[comb_at(l)] = g >= 0 && g < T ? row[g] : 0.0;
    }
    __syncthreads();
    const double* f0 = hrirs + (long long)j*2*nf;
    const double* f1 = f0 + nf;
    for (int m0 = 0; m0 < nf; m0 += kFoldChunk) {
      // w[i] is the row at q - (kFoldChunk - 1) + i, q the row index of this lane's first tap at filter tap m0
      const int lq = kFoldTaps*tid + (nf - 1) - m0;
      double w[kFoldChunk - 1 + kFoldTaps];
#pragma unroll
      for (int i = 0; i < kFoldChunk - 1 + kFoldTaps; ++i) w[i] = xs[comb_at(lq - (kFoldChunk - 1) + i)];
#pragma unroll
      for (int mm = 0; mm < kFoldChunk; ++mm) {
        const double a = f0[m0 + mm], b = f1[m0 + mm];
#pragma unroll
        for (int i = 0; i < kFoldTaps; ++i) {
          acc[0][i] = __builtin_fma(a, w[kFoldChunk - 1 + i - mm], acc[0][i]);
          acc[1][i] = __builtin_fma(b, w[kFoldChunk - 1 + i - mm], acc[1][i]);
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    double* y = fold + foff + ((long long)e*K + k)*T;          // inside the scratch: foff + 2 K T <= fold_len
#pragma unroll
    for (int i = 0; i < kFoldTaps; ++i) {
      const long long t = t0 + (long long)kFoldTaps*tid + i;
      if (t < T) y[t] = acc[e][i];
    }
  }
}

struct HrirOpts {
  BandOpts band;                                 // pattern mode, C = K
  int D, Th;
};

// "" or why the options are refused
std::string read_hrir_opts(const double* opts, HrirOpts* o) {
  if (!opts) return "null pointer: opts is required";
  const double band[BRV_RIR_BANDS_OPT_DOUBLES] = {opts[0], opts[1], opts[2], opts[3], (double)BRV_RIR_BANDS_PATTERN,
                                                  0.0, opts[4]};
  const std::string why = read_band_opts(band, &o->band);
  if (!why.empty()) return why;
  if (!(opts[5] >= 1.0) || !(opts[5] <= (double)kMaxDirs) || opts[5] != floor(opts[5]))
    return "requires 1 <= D <= " + std::to_string(kMaxDirs) + " (the measured directions)";
  if (!(opts[6] >= 1.0) || !(opts[6] <= (double)kMaxHrir) || opts[6] != floor(opts[6]))
    return "requires 1 <= T_h <= " + std::to_string(kMaxHrir) + " (the taps of an HRIR)";
  o->D = (int)opts[5];
  o->Th = (int)opts[6];
  return "";
}

struct HrirJob {
  BandJob band;                                  // o and a are not read
  const double *f, *l;
  int64_t ear;
};

HrirJob hrir_job_at(const double* geom, const int64_t* shape, int64_t j) {
  const double* g = geom + j*kHGeom;
  const int64_t* h = shape + j*kHShape;
  return HrirJob{BandJob{g, g + 3, g + 6, g + 9, g + 15, 1.0, h[0], h[1], h[2]}, g + 9, g + 12, h[3]};
}

std::string check_hrir_batch(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                             const double* dirs, int64_t max_order, HrirOpts* o) {
  if (!geom || !shape || !opts || !dirs) return "null pointer: geom, shape, opts and dirs are required";
  if (n_jobs < 1 || n_jobs > BRV_RIR_MAX_JOBS) return "requires 1 <= n_jobs <= " + std::to_string(BRV_RIR_MAX_JOBS);
  const std::string why = read_hrir_opts(opts, o);
  if (!why.empty()) return why;
  if (max_order < -1) return "requires max_order >= -1";
  for (int j = 0; j < o->D; ++j) {
    const double* p = dirs + 3*j;
    const double n2 = p[0]*p[0] + p[1]*p[1] + p[2]*p[2];
    if (!(fabs(n2 - 1.0) <= 1e-9))               // (a NaN or an infinity fails it as well)
      return "direction " + std::to_string(j) + " is not a finite unit vector (zero length, or not normalised)";
  }
  for (int64_t j = 0; j < n_jobs; ++j) {
    const HrirJob h = hrir_job_at(geom, shape, j);
    const BandJob& q = h.band;
    const std::string at = "job " + std::to_string(j) + ": ";
    double dist2 = 0.0, f2 = 0.0, l2 = 0.0, fl = 0.0;
    for (int k = 0; k < 3; ++k) {
      if (!finite_positive(q.L[k])) return at + "requires room dimensions > 0, finite";
      for (int b = 0; b < o->band.K; ++b)
        for (int w = 0; w < 2; ++w) {
          const double v = q.beta[6*b + 2*k + w];
          if (!(v >= 0.0) || !(v <= 1.0)) return at + "requires beta in [0, 1] in every band";
        }
      if (!(q.s[k] > 0.0) || !(q.s[k] < q.L[k])) return at + "the source is outside the box or on a wall";
      if (!(q.r[k] > 0.0) || !(q.r[k] < q.L[k])) return at + "the head is outside the box or on a wall";
      dist2 += (q.s[k] - q.r[k])*(q.s[k] - q.r[k]);
      f2 += h.f[k]*h.f[k]; l2 += h.l[k]*h.l[k]; fl += h.f[k]*h.l[k];
    }
    if (!(dist2 >= 1e-6)) return at + "the source is at the head's centre: requires a direct path of at least 1e-3 m";
    if (!(fabs(f2 - 1.0) <= 1e-9) || !(fabs(l2 - 1.0) <= 1e-9) || !(fabs(fl) <= 1e-9))
      return at + "requires unit front and left vectors at right angles";
    if (h.f[2] != 0.0 || h.l[2] != 0.0) return at + "requires an upright head: horizontal front and left vectors";
    if (q.taps < 1 || q.taps > BRV_RIR_MAX_TAPS) return at + "requires 1 <= taps <= " + std::to_string(BRV_RIR_MAX_TAPS);
    if (q.off < 0 || q.off > (1ll << 40)) return at + "requires 0 <= out_offset <= 2^40";
    if (q.stride < 1 || q.stride > 1024) return at + "requires 1 <= out_stride <= 1024";
    if (h.ear < 1 || h.ear > (1ll << 40)) return at + "requires 1 <= ear_offset <= 2^40";
  }
  return "";
}

using HrirTileKernel = void (*)(const double*, const long long*, long long, double, double, double, long long,
                                long long, const double*, int, double*, long long);

HrirTileKernel hrir_tile_kernel_of(int K) {
  switch (K) {
    case 1: return rir_hrir_tile_kernel<1>;
    case 2: return rir_hrir_tile_kernel<2>;
    case 3: return rir_hrir_tile_kernel<3>;
    case 4: return rir_hrir_tile_kernel<4>;
    case 5: return rir_hrir_tile_kernel<5>;
    case 6: return rir_hrir_tile_kernel<6>;
    case 7: return rir_hrir_tile_kernel<7>;
    case 8: return rir_hrir_tile_kernel<8>;
  }
  return nullptr;
}

}  // namespace

extern "C" {

int64_t brv_rir_hrir_table_rows(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                                const double* dirs, int64_t max_order) {
  HrirOpts o;
  const std::string why = check_hrir_batch(geom, shape, n_jobs, opts, dirs, max_order, &o);
  if (!why.empty()) return brv::fail(-1, why);
  std::vector<BandRow> rows;
  int64_t total = 0;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const HrirJob h = hrir_job_at(geom, shape, j);
    total += 1;
    for (int k = 0; k < 3; ++k) {
      if (!build_axis_bands(h.band, k, o.band, max_order, &rows))
        return brv::fail(-1, "job " + std::to_string(j) + ": " + kTooMany);
      total += (int64_t)rows.size();
    }
  }
  return total;
}

int brv_rir_hrir_build_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                              const double* dirs, int64_t max_order, double* rows_out, int64_t* index,
                              int64_t* ear_index, int64_t n_rows) {
  BRV_REFUSE(!rows_out || !index || !ear_index, "null pointer: rows, index and ear_index are required");
  HrirOpts o;
  const std::string why = check_hrir_batch(geom, shape, n_jobs, opts, dirs, max_order, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(n_rows < 1, "requires n_rows >= 1: the value of brv_rir_hrir_table_rows");
  const int K = o.band.K, RW = 3 + K;
  std::vector<BandRow> rows;
  int64_t at = 0, doff = 0, foff = 0;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const HrirJob h = hrir_job_at(geom, shape, j);
    const BandJob& q = h.band;
    int64_t* ix = index + j*kIdx;
    BRV_REFUSE(at + 1 > n_rows, "n_rows is not what brv_rir_hrir_table_rows gives for this batch");
    ix[0] = at;
    double* hd = rows_out + at*RW;
    for (int i = 0; i < RW; ++i) hd[i] = 0.0;
    hd[0] = h.f[0]; hd[1] = h.f[1]; hd[2] = h.l[0]; hd[3] = h.l[1];
    at += 1;
    for (int k = 0; k < 3; ++k) {
      BRV_REFUSE(!build_axis_bands(q, k, o.band, max_order, &rows), "job " + std::to_string(j) + ": " + kTooMany);
      BRV_REFUSE(at + (int64_t)rows.size() > n_rows,
                 "n_rows is not what brv_rir_hrir_table_rows gives for this batch");
      ix[1 + k] = (int64_t)rows.size();
      for (const BandRow& r : rows) {
        double* w = rows_out + at*RW;
        w[0] = r.d; w[1] = r.count; w[2] = r.d2;
        for (int b = 0; b < K; ++b) w[3 + b] = r.amp[b];
        at += 1;
      }
    }
    const int64_t T = q.taps + o.band.pad;
    ix[4] = q.taps; ix[5] = doff; ix[6] = 0; ix[7] = foff;
    for (int e = 0; e < 2; ++e) {
      int64_t* ex = ear_index + (2*j + e)*kIdx;
      ex[0] = ex[1] = ex[2] = ex[3] = 0;
      ex[4] = q.taps; ex[5] = q.off + (e ? h.ear : 0); ex[6] = q.stride; ex[7] = foff + (int64_t)e*K*T;
    }
    doff += (int64_t)K*o.D*T;
    foff += 2*(int64_t)K*T;
  }
  BRV_REFUSE(at != n_rows, "n_rows is not what brv_rir_hrir_table_rows gives for this batch");
  return 0;
}

int brv_rir_hrir_channels(const double* tables, const int64_t* index, int64_t n_jobs, int64_t n_rows,
                          int64_t max_taps, const double* opts, int64_t max_order, const double* dirs,
                          double* dir_scratch, int64_t dir_len, brv_stream_t stream) {
  BRV_REFUSE(!tables || !index || !opts || !dirs || !dir_scratch,
             "null pointer: tables, index, opts, dirs and dir_scratch are required");
  BRV_REFUSE(n_jobs < 1 || n_jobs > BRV_RIR_MAX_JOBS, "requires 1 <= n_jobs <= " + std::to_string(BRV_RIR_MAX_JOBS));
  BRV_REFUSE(n_rows < 1, "requires n_rows >= 1");
  BRV_REFUSE(max_taps < 1 || max_taps > BRV_RIR_MAX_TAPS,
             "requires 1 <= max_taps <= " + std::to_string(BRV_RIR_MAX_TAPS));
  HrirOpts o;
  const std::string why = read_hrir_opts(opts, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(max_order < -1, "requires max_order >= -1");
  BRV_REFUSE(dir_len < (int64_t)o.band.K*o.D*(max_taps + o.band.pad),
             "the direction scratch is too small: a job of max_taps needs K D (max_taps + pad) doubles");
  // rows of directions that no image reaches read as zero, and the kernel adds to what the rows hold
  BRV_HIP_OK(hipMemsetAsync(dir_scratch, 0, (size_t)dir_len*sizeof(double), (hipStream_t)stream));
  const int64_t ntile = (max_taps + o.band.pad + kTile - 1)/kTile;  // <= 8200 <= the limit of gridDim.y
  const HrirTileKernel kernel = hrir_tile_kernel_of(o.band.K);
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_jobs, (unsigned)ntile), dim3(kThreads), 0, (hipStream_t)stream, tables,
                     (const long long*)index, (long long)n_rows, o.band.fs, o.band.c, o.band.W, (long long)max_order,
                     (long long)o.band.pad, dirs, o.D, dir_scratch, (long long)dir_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_rir_hrir_fold(const double* dir_scratch, int64_t dir_len, const int64_t* index, int64_t n_jobs,
                      int64_t max_taps, const double* opts, const double* hrirs, int64_t n_filter,
                      double* fold_scratch, int64_t fold_len, brv_stream_t stream) {
  BRV_REFUSE(!dir_scratch || !index || !opts || !hrirs || !fold_scratch,
             "null pointer: dir_scratch, index, opts, hrirs and fold_scratch are required");
  BRV_REFUSE(n_jobs < 1 || n_jobs > BRV_RIR_MAX_JOBS, "requires 1 <= n_jobs <= " + std::to_string(BRV_RIR_MAX_JOBS));
  BRV_REFUSE(max_taps < 1 || max_taps > BRV_RIR_MAX_TAPS,
             "requires 1 <= max_taps <= " + std::to_string(BRV_RIR_MAX_TAPS));
  HrirOpts o;
  const std::string why = read_hrir_opts(opts, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(n_filter < o.Th || n_filter > kMaxHrir || n_filter%kFoldChunk != 0,
             "requires n_filter a multiple of 16 in [T_h, " + std::to_string(kMaxHrir) + "]");
  BRV_REFUSE(dir_len < (int64_t)o.band.K*o.D*(max_taps + o.band.pad),
             "the direction scratch is too small: a job of max_taps needs K D (max_taps + pad) doubles");
  BRV_REFUSE(fold_len < 2*(int64_t)o.band.K*(max_taps + o.band.pad),
             "the fold scratch is too small: a job of max_taps needs 2 K (max_taps + pad) doubles");
  const int64_t ntile = (max_taps + o.band.pad + kFoldTile - 1)/kFoldTile;
  hipLaunchKernelGGL(rir_hrir_fold_kernel, dim3((unsigned)n_jobs, (unsigned)ntile, (unsigned)o.band.K),
                     dim3(kFoldThreads), 0, (hipStream_t)stream, dir_scratch, (long long)dir_len,
                     (const long long*)index, o.band.K, o.D, (long long)o.band.pad, hrirs, (int)n_filter,
                     fold_scratch, (long long)fold_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}
