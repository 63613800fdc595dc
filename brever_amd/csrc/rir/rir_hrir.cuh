// The measured-ear entry points of libbrever_rir.so (include/rir/brever_rir_hrir.h): the ear is a set
// of measured HRIRs, an image goes to the row of the measured direction nearest to its arrival, and the rows are
// folded with that direction's HRIR pair. Included by rir.hip after rir_bands.cuh, whose options (read_band_opts) it
// reads in pattern mode; the tables are those of the band path (rir_host.h), the walk, the list entry and the tap
// weights those of rir_shell.cuh.
//
//   device rir_hrir_tile_kernel   the walk with the amplitudes A_k / (4 pi d); the lane that appends an entry finds its
//                                 direction, the argmax of q.p_j over the D directions read uniformly across the wave
//                                 (strictly greater wins, so ties go to the lowest j), and writes the key (direction,
//                                 list position). Consume: the keys are sorted in LDS (bitonic network; they are
//                                 distinct, so the order is that of the directions and, inside one, of the list), the
//                                 sorted list is cut into four slices at the changes of direction nearest to its
//                                 quarters, wave w walks slice w with K x 2 accumulators per lane and adds them to the
//                                 direction's rows (load, add, store) whenever the direction changes. A direction of a
//                                 round belongs to one wave and the rounds are separated by barriers, so every tap of
//                                 a row sees its additions in one order, that of the job's own tables.
//          rir_hrir_fold_kernel   one workgroup of 128 threads per (job, 1 024 taps, band): the FIR tile of
//                                 rir_fir.cuh per direction row, two filters per row, the HRIRs of both ears. Empty
//                                 stretches are not passed over: hardly any is empty at 8 000 taps.
#include <limits.h>

#include "../../../include/rir/brever_rir_hrir.h"

namespace {

constexpr int kMaxDirs = BRV_RIR_HRIR_MAX_DIRS, kMaxHrir = BRV_RIR_HRIR_MAX_TAPS, kHGeom = BRV_RIR_HRIR_GEOM_DOUBLES,
              kHShape = BRV_RIR_HRIR_SHAPE_WORDS;
static_assert(BRV_RIR_HRIR_FOLD_TILE == kFirTile, "the fold kernel's tile is the FIR tile");
static_assert(kMaxHrir%kFirChunk == 0, "the longest HRIR is whole chunks");

template <int K>
__global__ __launch_bounds__(kThreads) void rir_hrir_tile_kernel(const double* __restrict__ tab,
                                                                 const long long* __restrict__ index,
                                                                 long long n_rows, double fs, double c, double W,
                                                                 long long max_order, long long pad,
                                                                 const double* __restrict__ dirs, int D,
                                                                 double* __restrict__ scratch, long long scratch_len) {
  constexpr int RW = 3 + K;                      // a row is (offset, count, offset^2, K amplitudes)
  constexpr int kLog = K <= 6 ? 9 : 8;           // a list of 512 entries up to K = 6 and 256 above: LDS <= 54 KB
  constexpr int kCapH = 1 << kLog;
  static_assert(kMaxDirs <= (INT_MAX >> kLog), "a key holds a direction and a list position");
  __shared__ double zd2[kMaxAxis];
  __shared__ double e_tau[kCapH], e_s[kCapH], e_cw[kCapH], e_sw[kCapH], e_amp[K][kCapH];
  __shared__ int ord[kCapH];
  __shared__ int wave_tot[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long doff = ix[5];
  // an index that does not describe rows of this table, or direction rows inside the scratch, is not followed (uniform)
  Shell s;
  if (!shell_rows<RW>(tab, ix, n_rows, pad, &s) || doff < 0 || D < 1 || D > kMaxDirs) return;
  const long long T = s.T;                       // taps of a direction row
  const long long need = (long long)K*D*T;       // < 2^3 2^11 2^21
  if (need > scratch_len || doff > scratch_len - need) return;
  const double fx = s.H[0], fy = s.H[1], lx = s.H[2], ly = s.H[3];   // front and left, both horizontal
  shell_tile<RW, 2>(&s, fs, c, W, 0.0, 0.0, zd2);
  const long long t0 = s.t0;

  const LaneTaps lt = lane_taps(lane, W);
  double acc[K][kLaneTaps];
#pragma unroll
  for (int ch = 0; ch < K; ++ch) {
#pragma unroll
    for (int k = 0; k < kLaneTaps; ++k) acc[ch][k] = 0.0;
  }
  double* rows = scratch + doff;

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
  auto slice = [&](int w, int fill) {
    if (w >= kWaves) return fill;
    int p = (int)((long long)w*fill/kWaves);
    while (p > 0 && p < fill && (ord[p] >> kLog) == (ord[p - 1] >> kLog)) ++p;
    return p;
  };

  auto consume = [&](int fill) {
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
    const int p0 = slice(wave, fill), p1 = slice(wave + 1, fill);
    int cur = -1;
    for (int p = p0; p < p1; ++p) {
      const int key = __builtin_amdgcn_readfirstlane(ord[p]);
      const int i = key & (kCapH - 1), dj = key >> kLog;
      if (dj != cur) {
        if (cur >= 0) flush(cur);
        cur = dj;
      }
      double base[kLaneTaps];                    // u = 0 is sinc(0) window(0) = 1
      tap_weights(lt, lane, s.halfW, e_tau[i], e_s[i], 1.0, e_cw[i], e_sw[i], base);
#pragma unroll
      for (int ch = 0; ch < K; ++ch) {
        const double amp = e_amp[ch][i];
#pragma unroll
        for (int k = 0; k < kLaneTaps; ++k) acc[ch][k] = __builtin_fma(amp, base[k], acc[ch][k]);
      }
    }
    if (cur >= 0) flush(cur);
    __syncthreads();                             // the rows are the next round's, the list is free
  };

  auto append = [&](int e, const Hit& h) {
    const double qf = h.dx*fx + h.dy*fy, ql = h.dx*lx + h.dy*ly;   // v.f and v.l: the same for every z of the pair
    const double spread = h.counted ? 1.0/(4.0*kPi*h.d) : 0.0;
    // the measured direction nearest to the arrival q = (v.f, v.l, v.u), u = (0, 0, 1); j is uniform
    double best = dirs[0]*qf + dirs[1]*ql + dirs[2]*h.dz;
    int dj = 0;
    for (int j = 1; j < D; ++j) {
      const double dot = dirs[3*j]*qf + dirs[3*j + 1]*ql + dirs[3*j + 2]*h.dz;
      if (dot > best) { best = dot; dj = j; }
    }
    const Delay dl = delay_entry(h.d*fs/c, t0, W, 1.0);
    e_tau[e] = dl.taur;
    e_s[e] = dl.s;
    e_cw[e] = dl.cw;
    e_sw[e] = dl.sw;
    ord[e] = (dj << kLog) | e;
#pragma unroll
    for (int kb = 0; kb < K; ++kb) e_amp[kb][e] = h.xr[3 + kb]*h.yr[3 + kb]*h.zr[3 + kb]*spread;
  };

  shell_walk<RW, 1, 2, 3, kCapH>(s, zd2, wave_tot, max_order, append, consume);
}

__global__ __launch_bounds__(kFirThreads) void rir_hrir_fold_kernel(
    const double* __restrict__ dir, long long dir_len, const long long* __restrict__ index, int K, int D,
    long long pad, const double* __restrict__ hrirs, int nf, double* __restrict__ fold, long long fold_len) {
  __shared__ double xs[fir_lds(kMaxHrir)];
  const int tid = threadIdx.x, k = blockIdx.z;
  const long long* ix = index + (long long)blockIdx.x*kIdx;
  const long long taps = ix[4], doff = ix[5], foff = ix[7];
  if (taps < 1 || taps > BRV_RIR_MAX_TAPS || doff < 0 || foff < 0 || k >= K) return;
  const long long T = taps + pad;
  const long long need = (long long)K*D*T;
  if (need > dir_len || doff > dir_len - need) return;
  if (2ll*K*T > fold_len || foff > fold_len - 2ll*K*T) return;
  const long long t0 = (long long)blockIdx.y*kFirTile;
  if (t0 >= T) return;
  double acc[2][kFirTaps];
#pragma unroll
  for (int i = 0; i < kFirTaps; ++i) acc[0][i] = acc[1][i] = 0.0;
  // the tap t0 + i needs the row at t0 + i - m
  for (int j = 0; j < D; ++j) {
    const double* f0 = hrirs + (long long)j*2*nf;
    const double* const f[2] = {f0, f0 + nf};
    fir_tile<2>(xs, dir + doff + ((long long)k*D + j)*T, T, t0, nf, f, acc);
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    double* y = fold + foff + ((long long)e*K + k)*T;          // inside the scratch: foff + 2 K T <= fold_len
#pragma unroll
    for (int i = 0; i < kFirTaps; ++i) {
      const long long t = t0 + (long long)kFirTaps*tid + i;
      if (t < T) y[t] = acc[e][i];
    }
  }
}

struct HrirOpts {
  Opts band;                                     // pattern mode, C = K
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

// The batch checked, then its tables counted (rows_out null) or written with the two ear index rows of every job:
// "" or why it is refused.
std::string hrir_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                        const double* dirs, int64_t max_order, double* rows_out, int64_t* index, int64_t* ear_index,
                        int64_t n_rows, int64_t* total) {
  if (!geom || !shape || !opts || !dirs) return "null pointer: geom, shape, opts and dirs are required";
  HrirOpts o;
  std::string why = jobs_why(n_jobs);
  if (why.empty()) why = read_hrir_opts(opts, &o);
  if (why.empty() && max_order < -1) why = kNeedsOrder;
  if (!why.empty()) return why;
  for (int j = 0; j < o.D; ++j) {
    const double* p = dirs + 3*j;
    const double n2 = p[0]*p[0] + p[1]*p[1] + p[2]*p[2];
    if (!(fabs(n2 - 1.0) <= 1e-9))               // (a NaN or an infinity fails it as well)
      return "direction " + std::to_string(j) + " is not a finite unit vector (zero length, or not normalised)";
  }
  const auto job_at = [&](int64_t j) {
    const double* g = geom + j*kHGeom;
    const int64_t* h = shape + j*kHShape;
    return Job{g, g + 15, g + 3, g + 6, g + 9, g + 12, 1.0, h[0], h[1], h[2], h[3]};
  };
  const int K = o.band.K;
  int64_t doff = 0, foff = 0;
  const auto head = [&](int64_t j, const Job& q, double* h, int64_t* ix) {
    h[0] = q.o[0]; h[1] = q.o[1]; h[2] = q.l[0]; h[3] = q.l[1];
    const int64_t T = q.taps + o.band.pad;
    ix[4] = q.taps; ix[5] = doff; ix[6] = 0; ix[7] = foff;
    for (int e = 0; e < 2; ++e) {
      int64_t* ex = ear_index + (2*j + e)*kIdx;
      ex[0] = ex[1] = ex[2] = ex[3] = 0;
      ex[4] = q.taps; ex[5] = q.off + (e ? q.ear : 0); ex[6] = q.stride; ex[7] = foff + (int64_t)e*K*T;
    }
    doff += (int64_t)K*o.D*T;
    foff += 2*(int64_t)K*T;
  };
  return with_bands(K, [&](auto k) {
    return tables<decltype(k)::value>(n_jobs, job_at, kMeasured, o.band, max_order, "brv_rir_hrir_table_rows", rows_out,
                                      index, n_rows, total, head);
  });
}

using HrirTileKernel = void (*)(const double*, const long long*, long long, double, double, double, long long,
                                long long, const double*, int, double*, long long);

}  // namespace

extern "C" {

int64_t brv_rir_hrir_table_rows(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                                const double* dirs, int64_t max_order) {
  int64_t total = 0;
  const std::string why = hrir_tables(geom, shape, n_jobs, opts, dirs, max_order, nullptr, nullptr, nullptr, 0, &total);
  return why.empty() ? total : brv::fail(-1, why);
}

int brv_rir_hrir_build_tables(const double* geom, const int64_t* shape, int64_t n_jobs, const double* opts,
                              const double* dirs, int64_t max_order, double* rows_out, int64_t* index,
                              int64_t* ear_index, int64_t n_rows) {
  BRV_REFUSE(!rows_out || !index || !ear_index, "null pointer: rows, index and ear_index are required");
  int64_t total = 0;
  const std::string why = hrir_tables(geom, shape, n_jobs, opts, dirs, max_order, rows_out, index, ear_index, n_rows,
                                      &total);
  BRV_REFUSE(!why.empty(), why);
  return 0;
}

int brv_rir_hrir_channels(const double* tables, const int64_t* index, int64_t n_jobs, int64_t n_rows,
                          int64_t max_taps, const double* opts, int64_t max_order, const double* dirs,
                          double* dir_scratch, int64_t dir_len, brv_stream_t stream) {
  BRV_REFUSE(!tables || !index || !opts || !dirs || !dir_scratch,
             "null pointer: tables, index, opts, dirs and dir_scratch are required");
  HrirOpts o;
  std::string why = launch_why(n_jobs, n_rows, max_taps);
  if (why.empty()) why = read_hrir_opts(opts, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(max_order < -1, kNeedsOrder);
  BRV_REFUSE(dir_len < (int64_t)o.band.K*o.D*(max_taps + o.band.pad),
             "the direction scratch is too small: a job of max_taps needs K D (max_taps + pad) doubles");
  // rows of directions that no image reaches read as zero, and the kernel adds to what the rows hold
  BRV_HIP_OK(hipMemsetAsync(dir_scratch, 0, (size_t)dir_len*sizeof(double), (hipStream_t)stream));
  const int64_t ntile = (max_taps + o.band.pad + kTile - 1)/kTile;  // <= 8200 <= the limit of gridDim.y
  const HrirTileKernel kernel = with_bands(o.band.K, [](auto k) -> HrirTileKernel {
    return rir_hrir_tile_kernel<decltype(k)::value>;
  });
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
  HrirOpts o;
  std::string why = launch_why(n_jobs, 1, max_taps);
  if (why.empty()) why = read_hrir_opts(opts, &o);
  BRV_REFUSE(!why.empty(), why);
  BRV_REFUSE(n_filter < o.Th || n_filter > kMaxHrir || n_filter%kFirChunk != 0,
             "requires n_filter a multiple of 16 in [T_h, " + std::to_string(kMaxHrir) + "]");
  BRV_REFUSE(dir_len < (int64_t)o.band.K*o.D*(max_taps + o.band.pad),
             "the direction scratch is too small: a job of max_taps needs K D (max_taps + pad) doubles");
  BRV_REFUSE(fold_len < 2*(int64_t)o.band.K*(max_taps + o.band.pad),
             "the fold scratch is too small: a job of max_taps needs 2 K (max_taps + pad) doubles");
  const int64_t ntile = (max_taps + o.band.pad + kFirTile - 1)/kFirTile;
  hipLaunchKernelGGL(rir_hrir_fold_kernel, dim3((unsigned)n_jobs, (unsigned)ntile, (unsigned)o.band.K),
                     dim3(kFirThreads), 0, (hipStream_t)stream, dir_scratch, (long long)dir_len,
                     (const long long*)index, o.band.K, o.D, (long long)o.band.pad, hrirs, (int)n_filter,
                     fold_scratch, (long long)fold_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}
