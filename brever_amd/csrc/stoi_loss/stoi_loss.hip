// Backward pass of the STOI / ESTOI training criteria (include/brever_stoi_loss.h): from the per-row upstream
// gradient back to the gradient of the estimate, through the stages of ../stoi.hip in reverse. The forward is the
// metric's own and is not restated here; what the kernels below share with it (frame geometry, the Hann window,
// the arithmetic of stoi_segment_kernel up to the point where the derivative starts) is written the same way, so
// that the quantities the derivative is taken at are the forward's.
//
// Every kernel is a gather: one lane owns an output element and sums what reaches it in a fixed order. No atomics.
// All of them are streaming passes over a few MB; none is worth more than a plain grid-stride loop.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../../include/brever_stoi_loss.h"
#include "../status.h"

namespace {

constexpr int kFrame = 256, kHop = 128, kBands = 15, kSeg = 30;
constexpr double kEps = 2.220446049250313e-16;
constexpr long long kMaxRows = 65535;          // rows ride on gridDim.y

// hann(kFrame + 2)[1:-1][m], as ../stoi.hip
__device__ __forceinline__ float hann_inner(int m) {
  return 0.5f - 0.5f*cospif(2.f*(float)(m + 1)/(float)(kFrame + 1));
}
__host__ __device__ inline int frame_count(long long n) {     // len(range(0, n - kFrame, kHop))
  return n > kFrame ? (int)((n - kFrame + kHop - 1)/kHop) : 0;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One workgroup (64 lanes) per (row, segment): the tile's gradient, scaled by -grow[r]/(segments [* bands]).
// xs: clean tile, ys: estimate tile (the names of stoi_segment_kernel).
__global__ __launch_bounds__(64) void segment_backward_kernel(const float* tx, const float* ty, const int* geom,
                                                              const float* grow, float* seg_grad, int nf_max,
                                                              int nseg_max, int extended, float clip) {
  __shared__ float xs[kBands][kSeg + 1], ys[kBands][kSeg + 1], as[kBands][kSeg + 1], gs[kBands][kSeg + 1];
  __shared__ float rnorm[kBands];
  const int r = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const int nseg = clampi(geom[4*r + 2], 0, nf_max - kSeg + 1);
  if (s >= nseg) return;
  const float* bx = tx + (long long)r*kBands*nf_max;
  const float* by = ty + (long long)r*kBands*nf_max;
  for (int i = tid; i < kBands*kSeg; i += 64) {
    const int j = i / kSeg, n = i % kSeg;
    xs[j][n] = bx[(long long)j*nf_max + s + n];
    ys[j][n] = by[(long long)j*nf_max + s + n];
  }
  __syncthreads();
  const float eps = (float)kEps;
  const float scale = -grow[r]/((float)nseg*(extended ? 1.f : (float)kBands));
  if (!extended) {
    // d = c/((|a| + eps)(|b| + eps)), a = yp - mean(yp), b = x - mean(x), yp = min(y sc, x (1 + clip)),
    // sc = |x|/(|y| + eps): back through the correlation, the mean, the clip and the scale, one lane per band
    if (tid < kBands) {
      const int j = tid;
      float nx = 0.f, ny = 0.f;
      for (int n = 0; n < kSeg; ++n) { nx = __builtin_fmaf(xs[j][n], xs[j][n], nx); ny = __builtin_fmaf(ys[j][n], ys[j][n], ny); }
      const float ax = sqrtf(nx), ay = sqrtf(ny);
      const float sc = ax/(ay + eps);
      float my = 0.f, mx = 0.f;
      for (int n = 0; n < kSeg; ++n) {
        const float u = ys[j][n]*sc, v = xs[j][n]*(1.f + clip);
        const float yp = fminf(u, v);
        gs[j][n] = u <= v ? 1.f : 0.f;                      // the clip's pass mask
        as[j][n] = yp; my += yp; mx += xs[j][n];
      }
      my /= kSeg; mx /= kSeg;
      float vy = 0.f, vx = 0.f, c = 0.f;
      for (int n = 0; n < kSeg; ++n) {
        const float a = as[j][n] - my, b = xs[j][n] - mx;
        as[j][n] = a; xs[j][n] = b;
        vy = __builtin_fmaf(a, a, vy); vx = __builtin_fmaf(b, b, vx); c = __builtin_fmaf(a, b, c);
      }
      const float ry = sqrtf(vy), rx = sqrtf(vx);
      const float den = (ry + eps)*(rx + eps);
      const float k_norm = ry > 0.f ? c/(den*(ry + eps)*ry) : 0.f;        // d sqrt at 0 taken as 0
      float mean_ga = 0.f;
      for (int n = 0; n < kSeg; ++n) {
        const float ga = xs[j][n]/den - k_norm*as[j][n];
        as[j][n] = ga; mean_ga += ga;
      }
      mean_ga /= kSeg;
      float dot = 0.f;
      for (int n = 0; n < kSeg; ++n) {
        const float gu = (as[j][n] - mean_ga)*gs[j][n];
        as[j][n] = gu; dot = __builtin_fmaf(gu, ys[j][n], dot);
      }
      const float k_scale = ay > 0.f ? dot*ax/((ay + eps)*(ay + eps)*ay) : 0.f;
      for (int n = 0; n < kSeg; ++n) gs[j][n] = scale*(as[j][n]*sc - k_scale*ys[j][n]);
    }
  } else {
    // rows (bands): remove the mean over frames, unit norm; columns (frames): the same over bands; the clean
    // side as the forward, the estimate's side keeping the centred rows and their norms for the way back
    if (tid < kBands) {
      const int j = tid;
      float m = 0.f;
      for (int n = 0; n < kSeg; ++n) m += xs[j][n];
      m /= kSeg;
      float v = 0.f;
      for (int n = 0; n < kSeg; ++n) { xs[j][n] -= m; v = __builtin_fmaf(xs[j][n], xs[j][n], v); }
      float inv = 1.f/(sqrtf(v) + eps);
      for (int n = 0; n < kSeg; ++n) xs[j][n] *= inv;
      m = 0.f;
      for (int n = 0; n < kSeg; ++n) m += ys[j][n];
      m /= kSeg;
      v = 0.f;
      for (int n = 0; n < kSeg; ++n) { const float a = ys[j][n] - m; as[j][n] = a; v = __builtin_fmaf(a, a, v); }
      const float rn = sqrtf(v);
      rnorm[j] = rn;
      inv = 1.f/(rn + eps);
      for (int n = 0; n < kSeg; ++n) ys[j][n] = as[j][n]*inv;
    }
    __syncthreads();
    if (tid < kSeg) {
      const int n = tid;
      float z[kBands], cc[kBands];
      float m = 0.f;
      for (int j = 0; j < kBands; ++j) m += xs[j][n];
      m /= kBands;
      float v = 0.f;
      for (int j = 0; j < kBands; ++j) { const float d = xs[j][n] - m; z[j] = d; v = __builtin_fmaf(d, d, v); }
      const float invz = 1.f/(sqrtf(v) + eps)/kSeg;                      // contribution = sum(E z)/kSeg
      for (int j = 0; j < kBands; ++j) z[j] *= invz;
      m = 0.f;
      for (int j = 0; j < kBands; ++j) m += ys[j][n];
      m /= kBands;
      float w = 0.f, dot = 0.f;
      for (int j = 0; j < kBands; ++j) {
        const float d = ys[j][n] - m;
        cc[j] = d; w = __builtin_fmaf(d, d, w); dot = __builtin_fmaf(z[j], d, dot);
      }
      const float q = sqrtf(w), iq = 1.f/(q + eps);
      const float k_norm = q > 0.f ? dot*iq*iq/q : 0.f;
      float mean = 0.f;
      for (int j = 0; j < kBands; ++j) { cc[j] = z[j]*iq - k_norm*cc[j]; mean += cc[j]; }
      mean /= kBands;
      for (int j = 0; j < kBands; ++j) gs[j][n] = cc[j] - mean;
    }
    __syncthreads();
    if (tid < kBands) {
      const int j = tid;
      const float rn = rnorm[j], ir = 1.f/(rn + eps);
      float dot = 0.f;
      for (int n = 0; n < kSeg; ++n) dot = __builtin_fmaf(gs[j][n], as[j][n], dot);
      const float k_norm = rn > 0.f ? dot*ir*ir/rn : 0.f;
      float mean = 0.f;
      for (int n = 0; n < kSeg; ++n) { const float ga = gs[j][n]*ir - k_norm*as[j][n]; as[j][n] = ga; mean += ga; }
      mean /= kSeg;
      for (int n = 0; n < kSeg; ++n) gs[j][n] = scale*(as[j][n] - mean);
    }
  }
  __syncthreads();
  float* out = seg_grad + ((long long)r*nseg_max + s)*(kBands*kSeg);
  for (int i = tid; i < kBands*kSeg; i += 64) out[i] = gs[i / kSeg][i % kSeg];
}

// band_grad[r][band][f] = (sum over the segments that hold f, ascending) / tob, 0 where tob == 0
__global__ __launch_bounds__(256) void band_gather_kernel(const float* seg_grad, const float* tob, const int* geom,
                                                          float* band_grad, int rows, int nf_max, int nseg_max) {
  const long long total = (long long)rows*kBands*nf_max;
  for (long long i = (long long)blockIdx.x*256 + threadIdx.x; i < total; i += (long long)gridDim.x*256) {
    const int f = (int)(i % nf_max); const int band = (int)((i / nf_max) % kBands);
    const long long r = i / ((long long)nf_max*kBands);
    const int nseg = clampi(geom[4*r + 2], 0, nf_max - kSeg + 1);
    const int s_lo = f - (kSeg - 1) > 0 ? f - (kSeg - 1) : 0;
    const int s_hi = f < nseg - 1 ? f : nseg - 1;
    float g = 0.f;
    for (int s = s_lo; s <= s_hi; ++s)
      g += seg_grad[((r*nseg_max + s)*kBands + band)*kSeg + (f - s)];
    const float t = tob[i];
    band_grad[i] = t > 0.f ? g/t : 0.f;
  }
}

// spec_grad[r][f][bin] = (re, im) * sum of band_grad over the bands that hold the bin
__global__ __launch_bounds__(256) void spec_grad_kernel(const float* band_grad, const float* spec, const int* edges,
                                                        float* spec_grad, int rows, int nf_max, int nbins,
                                                        int bin0) {
  const long long total = (long long)rows*nf_max*nbins;
  for (long long i = (long long)blockIdx.x*256 + threadIdx.x; i < total; i += (long long)gridDim.x*256) {
    const int k = (int)(i % nbins); const int f = (int)((i / nbins) % nf_max);
    const long long r = i / ((long long)nbins*nf_max);
    const int b = bin0 + k;
    float g = 0.f;
    for (int band = 0; band < kBands; ++band)
      if (b >= edges[2*band] && b < edges[2*band + 1]) g += band_grad[(r*kBands + band)*nf_max + f];
    spec_grad[2*i] = g*spec[2*i];
    spec_grad[2*i + 1] = g*spec[2*i + 1];
  }
}

// comp_grad[r][p] = sum over the <= 2 frames covering p
__global__ __launch_bounds__(256) void fold_frames_kernel(const float* frame_grad, const int* geom, float* comp_grad,
                                                          int nf_max, long long comp_stride) {
  const int r = blockIdx.y;
  const int nf2 = clampi(geom[4*r + 1], 0, nf_max);
  const float* fg = frame_grad + (long long)r*nf_max*kFrame;
  for (long long p = (long long)blockIdx.x*256 + threadIdx.x; p < comp_stride; p += (long long)gridDim.x*256) {
    const long long j = p / kHop;
    float acc = 0.f;
    for (long long f = j - 1; f <= j; ++f) {
      if (f < 0 || f >= nf2) continue;
      const int m = (int)(p - f*kHop);
      if (m >= kFrame) continue;
      acc += fg[f*kFrame + m];
    }
    comp_grad[(long long)r*comp_stride + p] = acc;
  }
}

// dx[r][n] = sum over the <= 2 kept frames covering n of hann * comp_grad[rank of the frame * hop + m]
__global__ __launch_bounds__(256) void compact_backward_kernel(const float* comp_grad, const int* kept,
                                                               const int* geom, const int64_t* lengths, float* dx,
                                                               int nf_max, long long comp_stride, long long stride) {
  const int r = blockIdx.y;
  long long len = lengths[r];
  if (len > stride) len = stride;
  int nf = frame_count(len);
  if (nf > nf_max) nf = nf_max;
  const int k = clampi(geom[4*r + 3], 0, nf_max);
  const int* kp = kept + (long long)r*nf_max;
  const float* cg = comp_grad + (long long)r*comp_stride;
  for (long long n = (long long)blockIdx.x*256 + threadIdx.x; n < stride; n += (long long)gridDim.x*256) {
    float acc = 0.f;
    if (n < len) {
      const long long j = n / kHop;
      for (long long f = j - 1; f <= j; ++f) {
        if (f < 0 || f >= nf) continue;
        const int m = (int)(n - f*kHop);
        if (m >= kFrame) continue;
        int lo = 0, hi = k;                                 // rank of f in the ascending kept list
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (kp[mid] < (int)f) lo = mid + 1; else hi = mid; }
        if (lo >= k || kp[lo] != (int)f) continue;
        const long long p = (long long)lo*kHop + m;
        if (p < comp_stride) acc += hann_inner(m)*cg[p];
      }
    }
    dx[(long long)r*stride + n] = acc;
  }
}

// dx[r][i] = sum_m hpad[(m + n_pre_remove)*down - i*up] dy[r][m], m < ceil(len*up/down), i < len
__global__ __launch_bounds__(256) void resample_backward_kernel(const float* dy, const float* hpad,
                                                                const int64_t* lengths, float* dx,
                                                                long long in_stride, long long out_stride, int up,
                                                                int down, int hlen, int n_pre_remove) {
  const int r = blockIdx.y;
  long long len = lengths[r];
  if (len > in_stride) len = in_stride;
  long long n_out = (len*up + down - 1)/down;
  if (n_out > out_stride) n_out = out_stride;
  const float* g = dy + (long long)r*out_stride;
  for (long long i = (long long)blockIdx.x*256 + threadIdx.x; i < in_stride; i += (long long)gridDim.x*256) {
    float acc = 0.f;
    if (i < len) {
      const long long c = i*up;                             // filter index = (m + n_pre_remove)*down - c in [0, hlen)
      long long m_lo = (c + down - 1)/down - n_pre_remove;
      if (m_lo < 0) m_lo = 0;
      long long m_hi = (c + hlen - 1)/down - n_pre_remove;
      if (m_hi > n_out - 1) m_hi = n_out - 1;
      for (long long m = m_lo; m <= m_hi; ++m)
        acc = __builtin_fmaf(hpad[(m + n_pre_remove)*down - c], g[m], acc);
    }
    dx[(long long)r*in_stride + i] = acc;
  }
}

inline unsigned grid_x(long long n, long long cap) {
  long long g = (n + 255)/256;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

}  // namespace

extern "C" {

int brv_sl_segment_backward(const float* tob_clean, const float* tob_proc, const int32_t* geom,
                            const float* grad_rows, float* seg_grad, int64_t rows, int64_t nf_max, int extended,
                            float clip, brv_stream_t stream) {
  BRV_REFUSE(!tob_clean || !tob_proc || !geom || !grad_rows || !seg_grad,
             "null pointer: tob_clean, tob_proc, geom, grad_rows and seg_grad are required");
  BRV_REFUSE(rows < 1 || rows > kMaxRows || nf_max < 1 || nf_max > (1 << 24) || (extended != 0 && extended != 1) ||
             !(clip >= 0.f),
             "requires 1 <= rows <= 65535, 1 <= nf_max <= 2^24, extended 0 or 1, clip >= 0");
  if (nf_max < kSeg) return 0;                              // no row has a segment: nothing to write
  const int nseg_max = (int)nf_max - kSeg + 1;
  hipLaunchKernelGGL(segment_backward_kernel, dim3((unsigned)nseg_max, (unsigned)rows), dim3(64), 0,
                     (hipStream_t)stream, tob_clean, tob_proc, geom, grad_rows, seg_grad, (int)nf_max, nseg_max,
                     extended, clip);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_sl_bands_backward(const float* seg_grad, const float* tob_proc, const float* spec, const int32_t* edges,
                          const int32_t* geom, float* band_grad, float* spec_grad, int64_t rows, int64_t nf_max,
                          int64_t ncols, int64_t bin0, brv_stream_t stream) {
  BRV_REFUSE(!seg_grad || !tob_proc || !spec || !edges || !geom || !band_grad || !spec_grad,
             "null pointer: seg_grad, tob_proc, spec, edges, geom, band_grad and spec_grad are required");
  BRV_REFUSE(rows < 1 || rows > kMaxRows || nf_max < 1 || nf_max > (1 << 24) || ncols < 2 || (ncols & 1) ||
             ncols > 514 || bin0 < 0,
             "requires 1 <= rows <= 65535, 1 <= nf_max <= 2^24, ncols even in [2, 514], bin0 >= 0");
  hipStream_t st = (hipStream_t)stream;
  const int nseg_max = nf_max >= kSeg ? (int)nf_max - kSeg + 1 : 1;
  hipLaunchKernelGGL(band_gather_kernel, dim3(grid_x(rows*kBands*nf_max, 8192)), dim3(256), 0, st, seg_grad,
                     tob_proc, geom, band_grad, (int)rows, (int)nf_max, nseg_max);
  hipLaunchKernelGGL(spec_grad_kernel, dim3(grid_x(rows*nf_max*(ncols/2), 8192)), dim3(256), 0, st, band_grad,
                     spec, edges, spec_grad, (int)rows, (int)nf_max, (int)(ncols/2), (int)bin0);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_sl_fold_frames(const float* frame_grad, const int32_t* geom, float* comp_grad, int64_t rows,
                       int64_t nf_max, int64_t comp_stride, brv_stream_t stream) {
  BRV_REFUSE(!frame_grad || !geom || !comp_grad, "null pointer: frame_grad, geom and comp_grad are required");
  BRV_REFUSE(rows < 1 || rows > kMaxRows || nf_max < 1 || nf_max > (1 << 24) || comp_stride < 1,
             "requires 1 <= rows <= 65535, 1 <= nf_max <= 2^24, comp_stride >= 1");
  hipLaunchKernelGGL(fold_frames_kernel, dim3(grid_x(comp_stride, 2048), (unsigned)rows), dim3(256), 0,
                     (hipStream_t)stream, frame_grad, geom, comp_grad, (int)nf_max, (long long)comp_stride);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_sl_compact_backward(const float* comp_grad, const int32_t* kept, const int32_t* geom,
                            const int64_t* lengths, float* dx, int64_t rows, int64_t nf_max,
                            int64_t comp_stride, int64_t stride, brv_stream_t stream) {
  BRV_REFUSE(!comp_grad || !kept || !geom || !lengths || !dx,
             "null pointer: comp_grad, kept, geom, lengths and dx are required");
  BRV_REFUSE(rows < 1 || rows > kMaxRows || nf_max < 1 || nf_max > (1 << 24) || comp_stride < 1 || stride < 1,
             "requires 1 <= rows <= 65535, 1 <= nf_max <= 2^24, comp_stride >= 1, stride >= 1");
  hipLaunchKernelGGL(compact_backward_kernel, dim3(grid_x(stride, 2048), (unsigned)rows), dim3(256), 0,
                     (hipStream_t)stream, comp_grad, kept, geom, lengths, dx, (int)nf_max, (long long)comp_stride,
                     (long long)stride);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_sl_resample_backward(const float* dy, const float* hpad, const int64_t* lengths, float* dx,
                             int64_t rows, int64_t in_stride, int64_t out_stride, int64_t up, int64_t down,
                             int64_t hpad_len, int64_t n_pre_remove, brv_stream_t stream) {
  BRV_REFUSE(!dy || !hpad || !lengths || !dx, "null pointer: dy, hpad, lengths and dx are required");
  BRV_REFUSE(rows < 1 || rows > kMaxRows || in_stride < 1 || out_stride < 1 || up < 1 || down < 1 ||
             hpad_len < 1 || n_pre_remove < 0 || up > (1 << 20) || down > (1 << 20) || hpad_len > (1 << 30) ||
             n_pre_remove > (1 << 30),
             "requires 1 <= rows <= 65535, in_stride >= 1, out_stride >= 1, 1 <= up, down <= 2^20, "
             "1 <= hpad_len <= 2^30, 0 <= n_pre_remove <= 2^30");
  hipLaunchKernelGGL(resample_backward_kernel, dim3(grid_x(in_stride, 4096), (unsigned)rows), dim3(256), 0,
                     (hipStream_t)stream, dy, hpad, lengths, dx, (long long)in_stride, (long long)out_stride,
                     (int)up, (int)down, (int)hpad_len, (int)n_pre_remove);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"

// the library's last-error message and its two status exports (../status.h)
BRV_DEFINE_STATUS(brv_sl_version, brv_sl_last_error)
