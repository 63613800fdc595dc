// Exact Fourier resampling of a ragged batch of real signals in fp64 (include/brever_resample.h; brever_amd/io.py
// drives it): y = irfft(lowest bins of rfft(x, N), M) M/N for arbitrary N and M.
//
// Both transforms are Bluestein chirp transforms, n k = (n^2 + k^2 - (k - n)^2)/2:
//   X[k]  = w[k] sum_n (x[n] w[n]) conj(w)[k - n],        w[n] = exp(-i pi n^2/N),   k < Kb = min(N, M)/2 + 1
//   y[m]  = Re( v[m] sum_k (c[k] v[k]) conj(v)[m - k] )/N, v[k] = exp(+i pi k^2/M),  c = the irfft weights times X
// i.e. two circular convolutions of length L (a power of two >= max(N, M) + Kb - 1) with chirps whose spectra the
// caller caches (brv_rs_chirp_spectra). Chirp phases are reduced in 64-bit integers (n^2 mod 2N) before sincospi;
// no factor is ever accumulated by repeated multiplication.
//
// The length-L transform is a four-step decomposition, in place, L = R1 [R2] S with S = min(L, 4096) and
// R <= 256: column transforms of length R (16 adjacent columns per workgroup, so a wave reads 256 contiguous
// bytes per row), the factors w_L^(k s) from sincospi of the exact product k s, then row transforms of length S.
// The short transforms are radix-2 decimation-in-frequency butterflies in LDS (4096 complex fp64 = 64 KiB) read
// out bit-reversed, so each is natural order in and out. The long transform leaves its bins in the
// decomposition's own order (bin k1 + R k2 at k1 S + k2); the chirp spectra are stored in that order, the
// product is taken there, and the inverse runs the same steps backwards (rows, conjugate factors, columns), so
// no transposition is ever made. The inverse is unscaled; 1/L is folded into the next elementwise kernel.
//
// Every column's descriptor is checked in every kernel that reads it; a bad one is skipped. Nothing here sums
// over columns: the result of a column is a function of its own (x, N, M, L).
#include "../../../include/brever_resample.h"
#include "../status.h"
#include "../gfx950.cuh"

namespace {

typedef double2 cplx;

constexpr long long MAX_LENGTH = 1LL << 22;      // input and output samples
constexpr long long MAX_FFT = 1LL << 23;         // >= MAX_LENGTH + MAX_LENGTH/2
constexpr int ROW_LOG = 12, ROW_MAX = 1 << ROW_LOG;        // the LDS row transform
constexpr int COL_LOG = 8, COL_MAX = 1 << COL_LOG;         // the LDS column transform ...
constexpr int TILE_LOG = 4, TILE = 1 << TILE_LOG;          // ... of 16 adjacent columns
constexpr int TW_LOG = 12;                                 // tw holds exp(-2 pi i j/4096), j < 2048
constexpr int DESC = 8;

__device__ __forceinline__ cplx cmul(cplx a, cplx b) {
  return make_double2(a.x*b.x - a.y*b.y, a.x*b.y + a.y*b.x);
}

// exp(sign i pi j^2/n), 0 <= j < 2^24: j^2 < 2^48 is reduced modulo 2n in integers, the quotient r/n < 2 is
// rounded once.
__device__ __forceinline__ cplx chirp(long long j, long long n, double sign) {
  const unsigned long long r = ((unsigned long long)j*(unsigned long long)j) % (2ull*(unsigned long long)n);
  double s, c;
  sincospi((double)r/(double)n, &s, &c);
  return make_double2(c, sign*s);
}

struct Column {
  long long x_off, x_stride, n, m, out_off, out_stride, slot, kb;
};

// The descriptor of column c, or false: sizes out of range, another L than the call's, L too short.
__device__ __forceinline__ bool column(const long long* desc, long long c, long long L, Column& q) {
  const long long* d = desc + DESC*c;
  q.x_off = d[0]; q.x_stride = d[1]; q.n = d[2]; q.m = d[3];
  q.out_off = d[4]; q.out_stride = d[5]; q.slot = d[6];
  if (q.n < 1 || q.n > MAX_LENGTH || q.m < 1 || q.m > MAX_LENGTH || d[7] != L) return false;
  const long long k = q.n < q.m ? q.n : q.m, big = q.n < q.m ? q.m : q.n;
  q.kb = k/2 + 1;
  return big + q.kb - 1 <= L;
}

__device__ __forceinline__ bool span_ok(long long off, long long stride, long long count, long long len) {
  // off + (count - 1) stride < len without overflow: count <= 2^22 and stride <= 2^31
  return off >= 0 && off < len && stride >= 1 && stride <= (1LL << 31) && (count - 1)*stride < len - off;
}

// ---- the short transform in LDS ------------------------------------------------------------------------------
// 2^logc interleaved transforms of length T = 2^logt: element i of transform c at buf[(i << logc) + c]. Natural
// order in; bin k is left at index bitreverse(k). inv conjugates the factors (an unscaled inverse).
__device__ __forceinline__ void lds_fft(cplx* buf, int logt, int logc, bool inv, const cplx* __restrict__ tw) {
  const int cmask = (1 << logc) - 1;
  const int work = 1 << (logt - 1 + logc);
  for (int lh = logt - 1; lh >= 0; --lh) {                     // half = 2^lh
    __syncthreads();
    for (int e = threadIdx.x; e < work; e += 256) {
      const int c = e & cmask, t = e >> logc;
      const int pos = t & ((1 << lh) - 1), grp = t >> lh;
      const int i = (((grp << (lh + 1)) + pos) << logc) + c, j = i + (1 << (lh + logc));
      cplx w = tw[pos << (TW_LOG - 1 - lh)];                   // exp(-2 pi i pos/2^(lh+1))
      if (inv) w.y = -w.y;
      const cplx u = buf[i], v = buf[j];
      buf[i] = make_double2(u.x + v.x, u.y + v.y);
      buf[j] = cmul(make_double2(u.x - v.x, u.y - v.y), w);
    }
  }
  __syncthreads();
}

__device__ __forceinline__ int bitrev(int k, int logt) { return logt ? (int)(__brev((unsigned)k) >> (32 - logt)) : 0; }

// exp(-+ 2 pi i p/2^logl), 0 <= p < 2^logl: p/2^logl is exact
__device__ __forceinline__ cplx step_factor(long long p, int logl, bool inv) {
  double s, c;
  sincospi(ldexp((double)p, 1 - logl), &s, &c);
  return make_double2(c, inv ? s : -s);
}

// Row of the buffer a workgroup works on: blockIdx.y itself, or the entry sel[blockIdx.y*sel_stride] (checked).
__device__ __forceinline__ long long pick_row(const long long* sel, int sel_stride, long long nrows) {
  const long long r = sel ? sel[(long long)blockIdx.y*sel_stride] : (long long)blockIdx.y;
  return r >= 0 && r < nrows ? r : -1;
}

// Rows of length S = 2^logs, contiguous: blockIdx.x is the row within the signal. With `slab`, the inverse
// multiplies by the chirp spectrum of the column's slot while loading.
__global__ __launch_bounds__(256) void fft_rows_kernel(cplx* __restrict__ buf, long long nrows, long long L, int logs,
                                                       int inv, const cplx* __restrict__ tw,
                                                       const long long* __restrict__ sel, int sel_stride,
                                                       const long long* __restrict__ desc,
                                                       const cplx* __restrict__ slab, long long nslots) {
  __shared__ cplx lds[ROW_MAX];
  const long long row = pick_row(sel, sel_stride, nrows);
  if (row < 0) return;                                         // (uniform)
  const int S = 1 << logs;
  const long long at = (long long)blockIdx.x << logs;
  cplx* p = buf + row*L + at;
  const cplx* b = nullptr;
  if (slab) {
    Column q;
    if (!column(desc, blockIdx.y, L, q) || q.slot < 0 || q.slot >= nslots) return;
    b = slab + q.slot*L + at;
  }
  for (int i = threadIdx.x; i < S; i += 256) lds[i] = b ? cmul(p[i], b[i]) : p[i];
  lds_fft(lds, logs, 0, inv != 0, tw);
  for (int k = threadIdx.x; k < S; k += 256) p[k] = lds[bitrev(k, logs)];
}

// Columns: the signal's L elements seen as (outer, R, Sp) with R = 2^logr and Sp = 2^logsp; a workgroup takes 16
// adjacent columns s of one outer block. Forward: transform over R, then bin k of column s times w_(R Sp)^(k s).
// Inverse: the conjugate factor first, then the inverse transform.
__global__ __launch_bounds__(256) void fft_cols_kernel(cplx* __restrict__ buf, long long nrows, long long L, int logr,
                                                       int logsp, int inv, const cplx* __restrict__ tw,
                                                       const long long* __restrict__ sel, int sel_stride) {
  __shared__ cplx lds[COL_MAX*TILE];
  const long long row = pick_row(sel, sel_stride, nrows);
  if (row < 0) return;                                         // (uniform)
  const int R = 1 << logr;
  const long long tiles = 1LL << (logsp - TILE_LOG);
  const long long outer = blockIdx.x/tiles, s0 = (blockIdx.x - outer*tiles) << TILE_LOG;
  cplx* p = buf + row*L + (outer << (logr + logsp)) + s0;
  const int count = R << TILE_LOG;
  for (int e = threadIdx.x; e < count; e += 256) {
    const int c = e & (TILE - 1), i = e >> TILE_LOG;
    cplx v = p[((long long)i << logsp) + c];
    if (inv) v = cmul(v, step_factor((long long)i*(s0 + c), logr + logsp, true));
    lds[e] = v;
  }
  lds_fft(lds, logr, TILE_LOG, inv != 0, tw);
  for (int e = threadIdx.x; e < count; e += 256) {
    const int c = e & (TILE - 1), k = e >> TILE_LOG;
    cplx v = lds[(bitrev(k, logr) << TILE_LOG) + c];
    if (!inv) v = cmul(v, step_factor((long long)k*(s0 + c), logr + logsp, false));
    p[((long long)k << logsp) + c] = v;
  }
}

// ---- the elementwise stages -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void chirp_fill_kernel(cplx* __restrict__ slab, const long long* __restrict__ desc,
                                                         long long nslots, long long L) {
  const long long* d = desc + 3*(long long)blockIdx.y;
  const long long slot = d[0], n = d[1], kind = d[2];
  if (slot < 0 || slot >= nslots || n < 1 || n > MAX_LENGTH || n > L || (kind != 0 && kind != 1)) return;
  const long long split = kind ? n : L - n + 1;                // b[j] = chirp(j) below, chirp(L - j) from there on
  const double sign = kind ? -1.0 : 1.0;
  cplx* out = slab + slot*L;
  GRID_STRIDE(j, L) out[j] = chirp(j < split ? j : L - j, n, sign);
}

template <typename T>
__global__ __launch_bounds__(256) void load_kernel(const T* __restrict__ x, const long long* __restrict__ desc,
                                                   cplx* __restrict__ work, long long x_len, long long L) {
  Column q;
  if (!column(desc, blockIdx.y, L, q) || !span_ok(q.x_off, q.x_stride, q.n, x_len)) return;
  const T* in = x + q.x_off;
  cplx* out = work + (long long)blockIdx.y*L;
  GRID_STRIDE(i, L) {
    cplx v = make_double2(0.0, 0.0);
    if (i < q.n) {
      const double s = (double)in[i*q.x_stride];
      const cplx w = chirp(i, q.n, -1.0);
      v = make_double2(s*w.x, s*w.y);
    }
    out[i] = v;
  }
}

// work[k] (the convolution, times L) -> g_k X[k] v[k]/N for k < Kb, zero behind. g: the one-sided weights of the
// M-point inverse (1 at k = 0 and at k = M/2 for even M, else 2) times scipy.signal.resample's rule for the
// bin K/2 of an even K = min(N, M): twice when M < N, half when N < M.
__global__ __launch_bounds__(256) void spectrum_kernel(const long long* __restrict__ desc, cplx* __restrict__ work,
                                                       long long L) {
  Column q;
  if (!column(desc, blockIdx.y, L, q)) return;
  cplx* w = work + (long long)blockIdx.y*L;
  const long long K = q.n < q.m ? q.n : q.m;
  const double inv_l = 1.0/(double)L;                          // exact: L is a power of two
  GRID_STRIDE(k, L) {
    cplx v = make_double2(0.0, 0.0);
    if (k < q.kb) {
      double g = (k == 0 || 2*k == q.m) ? 1.0 : 2.0;
      if (2*k == K) g *= q.m < q.n ? 2.0 : q.n < q.m ? 0.5 : 1.0;
      g = g*inv_l/(double)q.n;
      v = cmul(cmul(chirp(k, q.n, -1.0), chirp(k, q.m, 1.0)), w[k]);
      v.x *= g; v.y *= g;
    }
    w[k] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void store_kernel(const cplx* __restrict__ work, const long long* __restrict__ desc,
                                                    T* __restrict__ out, long long out_len, long long L) {
  Column q;
  if (!column(desc, blockIdx.y, L, q) || !span_ok(q.out_off, q.out_stride, q.m, out_len)) return;
  const cplx* w = work + (long long)blockIdx.y*L;
  T* y = out + q.out_off;
  const double inv_l = 1.0/(double)L;
  GRID_STRIDE(i, q.m) {
    const cplx v = chirp(i, q.m, 1.0), c = w[i];
    y[i*q.out_stride] = (T)((v.x*c.x - v.y*c.y)*inv_l);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
int ilog2(long long v) { int l = 0; while ((1LL << l) < v) ++l; return l; }

// In-place transform of `count` rows (those of sel, or the first count) of a (nrows, L) buffer.
int transform(cplx* buf, long long nrows, long long L, long long count, bool inv, const cplx* tw, const long long* sel,
              int sel_stride, const long long* desc, const cplx* slab, long long nslots, hipStream_t st) {
  const int logl = ilog2(L), logs = logl < ROW_LOG ? logl : ROW_LOG;
  int logr[2] = {0, 0};                                        // the column levels, outermost first
  const int rem = logl - logs;
  if (rem > COL_LOG) { logr[0] = rem - COL_LOG; logr[1] = COL_LOG; } else { logr[0] = rem; }
  const dim3 rows_grid((unsigned)(L >> logs), (unsigned)count);
  auto rows = [&]() {
    fft_rows_kernel<<<rows_grid, 256, 0, st>>>(buf, nrows, L, logs, inv ? 1 : 0, tw, sel, sel_stride,
                                               inv ? desc : nullptr, inv ? slab : nullptr, nslots);
  };
  auto cols = [&](int level) {
    if (!logr[level]) return;
    const int logsp = level == 0 ? logl - logr[0] : logs;      // columns of the level: what lies below it
    const dim3 grid((unsigned)(L >> (logr[level] + TILE_LOG)), (unsigned)count);
    fft_cols_kernel<<<grid, 256, 0, st>>>(buf, nrows, L, logr[level], logsp, inv ? 1 : 0, tw, sel, sel_stride);
  };
  if (!inv) { cols(0); cols(1); rows(); } else { rows(); cols(1); cols(0); }
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int check_fft_len(long long L) {
  BRV_REFUSE(L < 16 || (L & (L - 1)) != 0, "requires fft_len a power of two >= 16");
  BRV_UNSUPPORTED(L > MAX_FFT, "fft_len beyond 8388608 (signals of at most 4194304 samples)");
  return 0;
}

}  // namespace

extern "C" {

int64_t brv_rs_max_length(void) { return MAX_LENGTH; }

int64_t brv_rs_fft_length(int64_t n, int64_t m) {
  if (n < 1 || m < 1) return brv::fail(-1, "requires n >= 1 and m >= 1");
  if (n > MAX_LENGTH || m > MAX_LENGTH)
    return brv::fail(-1, "signal of " + std::to_string((long long)n) + " -> " + std::to_string((long long)m) +
                         " samples: at most " + std::to_string(MAX_LENGTH) + " in and out");
  const long long need = (n > m ? n : m) + (n < m ? n : m)/2;
  long long L = 16;
  while (L < need) L <<= 1;
  return L;
}

int brv_rs_chirp_spectra(double* slab, const int64_t* desc, const double* tw, int64_t nslots, int64_t fft_len,
                         int64_t count, brv_stream_t stream) {
  BRV_REFUSE(!slab || !desc || !tw, "null slab, desc or tw");
  BRV_REFUSE(nslots < 1 || count < 1 || count > BRV_RS_MAX_COLUMNS, "requires nslots >= 1 and 1 <= count <= 32768");
  if (int e = check_fft_len(fft_len)) return e;
  hipStream_t st = (hipStream_t)stream;
  const long long* d = (const long long*)desc;
  chirp_fill_kernel<<<dim3(brv::flat_grid(fft_len, 1024).x, (unsigned)count), 256, 0, st>>>((cplx*)slab, d, nslots,
                                                                                          fft_len);
  BRV_HIP_OK(hipGetLastError());
  return transform((cplx*)slab, nslots, fft_len, count, false, (const cplx*)tw, d, 3, nullptr, nullptr, 0, st);
}

int brv_rs_analysis(const void* x, const int64_t* desc, const double* slab, const double* tw, double* work,
                    int64_t x_len, int64_t x_float32, int64_t nslots, int64_t fft_len, int64_t ncols,
                    brv_stream_t stream) {
  BRV_REFUSE(!x || !desc || !slab || !tw || !work, "null x, desc, slab, tw or work");
  BRV_REFUSE(x_len < 1 || x_float32 < 0 || nslots < 1 || ncols < 1 || ncols > BRV_RS_MAX_COLUMNS,
             "requires x_len >= 1, x_float32 >= 0, nslots >= 1 and 1 <= ncols <= 32768");
  if (int e = check_fft_len(fft_len)) return e;
  hipStream_t st = (hipStream_t)stream;
  const long long* d = (const long long*)desc;
  const cplx* t = (const cplx*)tw;
  cplx* w = (cplx*)work;
  const dim3 grid(brv::flat_grid(fft_len, 1024).x, (unsigned)ncols);
  if (x_float32) load_kernel<float><<<grid, 256, 0, st>>>((const float*)x, d, w, x_len, fft_len);
  else load_kernel<double><<<grid, 256, 0, st>>>((const double*)x, d, w, x_len, fft_len);
  BRV_HIP_OK(hipGetLastError());
  if (int e = transform(w, ncols, fft_len, ncols, false, t, nullptr, 0, nullptr, nullptr, 0, st)) return e;
  if (int e = transform(w, ncols, fft_len, ncols, true, t, nullptr, 0, d, (const cplx*)slab, nslots, st)) return e;
  spectrum_kernel<<<grid, 256, 0, st>>>(d, w, fft_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_rs_synthesis(double* work, const int64_t* desc, const double* slab, const double* tw, void* out,
                     int64_t out_len, int64_t out_float32, int64_t nslots, int64_t fft_len, int64_t ncols,
                     brv_stream_t stream) {
  BRV_REFUSE(!work || !desc || !slab || !tw || !out, "null work, desc, slab, tw or out");
  BRV_REFUSE(out_len < 1 || out_float32 < 0 || nslots < 1 || ncols < 1 || ncols > BRV_RS_MAX_COLUMNS,
             "requires out_len >= 1, out_float32 >= 0, nslots >= 1 and 1 <= ncols <= 32768");
  if (int e = check_fft_len(fft_len)) return e;
  hipStream_t st = (hipStream_t)stream;
  const long long* d = (const long long*)desc;
  const cplx* t = (const cplx*)tw;
  cplx* w = (cplx*)work;
  if (int e = transform(w, ncols, fft_len, ncols, false, t, nullptr, 0, nullptr, nullptr, 0, st)) return e;
  if (int e = transform(w, ncols, fft_len, ncols, true, t, nullptr, 0, d, (const cplx*)slab, nslots, st)) return e;
  const dim3 grid(brv::flat_grid(fft_len, 1024).x, (unsigned)ncols);
  if (out_float32) store_kernel<float><<<grid, 256, 0, st>>>(w, d, (float*)out, out_len, fft_len);
  else store_kernel<double><<<grid, 256, 0, st>>>(w, d, (double*)out, out_len, fft_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}

// the library's last-error message and its two status exports (../status.h)
BRV_DEFINE_STATUS(brv_rs_version, brv_rs_last_error)
