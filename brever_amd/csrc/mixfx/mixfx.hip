// Kernels behind the signal effects of the batched mixture engine (include/brever_mixfx.h; brever_amd/mixture.py
// drives them): the periodic extension that turns colored_noise's circular convolution into a partitioned
// product, the per-signal long-term average spectrum and its equalisation (match_ltas, calc_ltas), a masked row
// copy, and BRIRDecay.
//
// As in mix/mix.hip every index comes from a descriptor on the device and is checked where it is used: an entry
// that points outside the operand it names is skipped, never followed. Reductions are fp64, in an order fixed
// by the signal's (the job's) own length: nothing depends on the batch.
#include "../../../include/brever_mixfx.h"
#include "../status.h"
#include "../gfx950.cuh"

namespace {

// ---- gather / scatter -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_periodic_kernel(const float* __restrict__ pool,
                                                            const long long* __restrict__ desc,
                                                            float* __restrict__ rows, long long pool_len,
                                                            long long row_len) {
  const long long r = blockIdx.y;
  const long long src = desc[2*r];
  long long m = desc[2*r + 1];
  if (src < 0 || m < 0 || src > pool_len || m > pool_len - src) m = 0;
  float* out = rows + r*row_len;
  GRID_STRIDE(i, row_len) {
    float v = 0.f;
    if (i < m) v = pool[src + i];
    else if (i - m < m) v = pool[src + i - m];
    out[i] = v;
  }
}

__global__ __launch_bounds__(256) void copy_rows_kernel(const float* __restrict__ src,
                                                        const long long* __restrict__ desc,
                                                        float* __restrict__ dst, long long src_rows,
                                                        long long src_row_len, long long dst_len) {
  const long long c = blockIdx.y;
  const long long row = desc[5*c], off = desc[5*c + 1], n = desc[5*c + 2], at = desc[5*c + 3], span = desc[5*c + 4];
  if (row < 0 || row >= src_rows || off < 0 || n < 0 || off > src_row_len || n > src_row_len - off) return;
  if (at < 0 || span < n || at > dst_len || span > dst_len - at) return;
  const float* in = src + row*src_row_len + off;
  float* out = dst + at;
  GRID_STRIDE(i, span) out[i] = i < n ? in[i] : 0.f;
}

// ---- long-term average spectrum ---------------------------------------------------------------------------------
// One wave per (signal, bin): a lane sums its frames in ascending order, row after row, then the lanes fold in
// a fixed tree.
constexpr int LTAS_BINS = 4;

__device__ __forceinline__ bool ltas_signal(const int* desc, int s, int rows, int frames, int& row0, int& nrows,
                                            int& fs) {
  row0 = desc[3*s]; nrows = desc[3*s + 1]; fs = desc[3*s + 2];
  return row0 >= 0 && nrows >= 1 && nrows <= 2 && row0 <= rows - nrows && fs >= 1 && fs <= frames;
}

__global__ __launch_bounds__(256) void ltas_power_kernel(const float2* __restrict__ spec, const int* __restrict__ desc,
                                                         double* __restrict__ power, int rows, int bins, int frames) {
  const int s = blockIdx.y, lane = threadIdx.x & 63, bin = blockIdx.x*LTAS_BINS + (threadIdx.x >> 6);
  if (bin >= bins) return;                                   // (a whole wave)
  int row0, nrows, fs;
  double acc = 0.0;
  const bool ok = ltas_signal(desc, s, rows, frames, row0, nrows, fs);
  if (ok) {
    for (int r = 0; r < nrows; ++r) {
      const float2* x = spec + ((long long)(row0 + r)*bins + bin)*frames;
      for (int f = lane; f < fs; f += 64) {
        const float2 v = x[f];
        acc = fma((double)v.x, (double)v.x, acc);
        acc = fma((double)v.y, (double)v.y, acc);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (lane == 0) power[(long long)s*bins + bin] = ok ? acc/((double)nrows*(double)fs) : 0.0;
}

__global__ __launch_bounds__(256) void ltas_equalize_kernel(float2* __restrict__ spec, const int* __restrict__ desc,
                                                            const double* __restrict__ power,
                                                            const double* __restrict__ ltas, int rows, int bins,
                                                            int frames) {
  const int s = blockIdx.y, bin = blockIdx.x;
  int row0, nrows, fs;
  if (!ltas_signal(desc, s, rows, frames, row0, nrows, fs)) return;
  const double p = power[(long long)s*bins + bin];
  const float g = p > 0.0 ? (float)sqrt(ltas[bin]/p) : 0.f;
  for (int e = threadIdx.x; e < nrows*fs; e += 256) {
    const int r = e/fs, f = e - r*fs;
    float2* x = spec + ((long long)(row0 + r)*bins + bin)*frames + f;
    float2 v = *x;
    v.x *= g; v.y *= g;
    *x = v;
  }
}

// ---- BRIRDecay ------------------------------------------------------------------------------------------------------
// numpy's argmax takes the FIRST maximum: ties go to the lower index (as pack_brirs_kernel of mix/mix.hip).
__device__ __forceinline__ void peak_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__device__ __forceinline__ double decay_env(long long k, double fs, double rt60) {
  return exp(-((double)k/fs)/rt60*3.0*log(10.0));            // the accurate fp64 exponential
}

__global__ __launch_bounds__(256) void decay_brirs_kernel(const float* __restrict__ brir_pool,
                                                          const float* __restrict__ noise_pool,
                                                          const long long* __restrict__ desc,
                                                          const double* __restrict__ params,
                                                          float* __restrict__ out, int* __restrict__ status,
                                                          long long brir_len, long long noise_len,
                                                          long long out_len) {
  __shared__ float sv[2][256];
  __shared__ int si[2][256];
  __shared__ double red[2][256];
  const long long j = blockIdx.x;
  const int tid = threadIdx.x;
  const long long boff = desc[8*j], taps = desc[8*j + 1], noff = desc[8*j + 2], nn = desc[8*j + 3];
  const long long ooff = desc[8*j + 4], n = desc[8*j + 5], d0 = desc[8*j + 6], claimed = desc[8*j + 7];
  const double rt60 = params[3*j], drr = params[3*j + 1], fs = params[3*j + 2];
  const long long big = 1LL << 30;
  bool ok = taps >= 1 && taps < big && boff >= 0 && boff <= brir_len && 2*taps <= brir_len - boff;
  ok = ok && n >= taps && n < big && ooff >= 0 && ooff <= out_len && 2*n <= out_len - ooff;
  ok = ok && noff >= 0 && nn >= 0 && noff <= noise_len && nn <= noise_len - noff && d0 >= 0 && d0 < big;
  ok = ok && rt60 > 0.0 && fs > 0.0;
  if (!ok) {                                                  // (uniform)
    if (tid == 0) status[j] = 4;
    return;
  }
  const float* h = brir_pool + boff;
  const float* noise = noise_pool + noff;
  float v0 = -1.f, v1 = -1.f;
  int i0 = 0, i1 = 0;
  for (long long t = tid; t < taps; t += 256) {                // ascending per thread: the first maximum stays
    const float a0 = fabsf(h[2*t]), a1 = fabsf(h[2*t + 1]);
    if (a0 > v0) { v0 = a0; i0 = (int)t; }
    if (a1 > v1) { v1 = a1; i1 = (int)t; }
  }
  sv[0][tid] = v0; si[0][tid] = i0; sv[1][tid] = v1; si[1][tid] = i1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      peak_merge(sv[0][tid], si[0][tid], sv[0][tid + s], si[0][tid + s]);
      peak_merge(sv[1][tid], si[1][tid], sv[1][tid + s], si[1][tid + s]);
    }
    __syncthreads();
  }
  const long long start = d0 + (si[0][0] < si[1][0] ? si[0][0] : si[1][0]);
  const long long tail = n - start;                            // may be <= 0: no tail, status 2
  if ((claimed >= 0 && claimed != tail) || tail > nn) {        // (uniform)
    if (tid == 0) status[j] = 3;
    return;
  }
  double eh = 0.0, et = 0.0;
  for (long long t = tid; t < taps; t += 256) {
    const double m = 0.5*((double)h[2*t] + (double)h[2*t + 1]);
    eh = fma(m, m, eh);
  }
  for (long long k = tid; k < tail; k += 256) {
    const double v = decay_env(k, fs, rt60)*(double)noise[k];
    et = fma(v, v, et);
  }
  red[0][tid] = eh; red[1][tid] = et;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  eh = red[0][0]; et = red[1][0];
  const int st = eh == 0.0 ? 1 : (et == 0.0 ? 2 : 0);
  const double gain = st == 0 ? sqrt(pow(10.0, -drr/10.0)*eh/et) : 0.0;
  float* o = out + ooff;
  for (long long t = tid; t < n; t += 256) {
    double l = t < taps ? (double)h[2*t] : 0.0, r = t < taps ? (double)h[2*t + 1] : 0.0;
    if (st == 0 && t >= start) {
      const double v = gain*(decay_env(t - start, fs, rt60)*(double)noise[t - start]);
      l += v; r += v;
    }
    o[2*t] = (float)l; o[2*t + 1] = (float)r;
  }
  if (tid == 0) status[j] = st;
}

unsigned grid_x(long long n) {
  long long g = (n + 255)/256;
  return (unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

}  // namespace

extern "C" {

int brv_mixfx_pack_periodic(const float* pool, const int64_t* desc, float* rows, int64_t pool_len, int64_t nrows,
                            int64_t row_len, brv_stream_t stream) {
  BRV_REFUSE(!pool || !desc || !rows, "null pool, desc or rows");
  BRV_REFUSE(pool_len < 1 || nrows < 1 || row_len < 1 || nrows > 65535,
             "requires pool_len >= 1, 1 <= nrows <= 65535, row_len >= 1");
  hipLaunchKernelGGL(pack_periodic_kernel, dim3(grid_x(row_len), (unsigned)nrows), dim3(256), 0,
                     (hipStream_t)stream, pool, (const long long*)desc, rows, (long long)pool_len, (long long)row_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_mixfx_copy_rows(const float* src, const int64_t* desc, float* dst, int64_t ncopies, int64_t src_rows,
                        int64_t src_row_len, int64_t dst_len, brv_stream_t stream) {
  BRV_REFUSE(!src || !desc || !dst, "null src, desc or dst");
  BRV_REFUSE(ncopies < 1 || ncopies > 65535 || src_rows < 1 || src_row_len < 1 || dst_len < 1,
             "requires 1 <= ncopies <= 65535, src_rows >= 1, src_row_len >= 1, dst_len >= 1");
  hipLaunchKernelGGL(copy_rows_kernel, dim3(grid_x(src_row_len), (unsigned)ncopies), dim3(256), 0,
                     (hipStream_t)stream, src, (const long long*)desc, dst, (long long)src_rows, (long long)src_row_len,
                     (long long)dst_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

#define BRV_MIXFX_SPEC_ARGS(spec_null)                                                                          \
  BRV_REFUSE(spec_null, "null spec, desc, power or ltas");                                                      \
  BRV_REFUSE(nsig < 1 || nsig > 65535 || rows < 1 || bins < 1 || frames < 1 || rows >= (1LL << 30) ||           \
             bins >= (1LL << 30) || frames >= (1LL << 30),                                                      \
             "requires 1 <= nsig <= 65535 and 1 <= rows, bins, frames < 2^30")

int brv_mixfx_ltas_power(const float* spec, const int32_t* desc, double* power, int64_t nsig, int64_t rows,
                         int64_t bins, int64_t frames, brv_stream_t stream) {
  BRV_MIXFX_SPEC_ARGS(!spec || !desc || !power);
  hipLaunchKernelGGL(ltas_power_kernel, dim3((unsigned)((bins + LTAS_BINS - 1)/LTAS_BINS), (unsigned)nsig), dim3(256),
                     0, (hipStream_t)stream, (const float2*)spec, desc, power, (int)rows, (int)bins, (int)frames);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_mixfx_ltas_equalize(float* spec, const int32_t* desc, const double* power, const double* ltas,
                            int64_t nsig, int64_t rows, int64_t bins, int64_t frames, brv_stream_t stream) {
  BRV_MIXFX_SPEC_ARGS(!spec || !desc || !power || !ltas);
  hipLaunchKernelGGL(ltas_equalize_kernel, dim3((unsigned)bins, (unsigned)nsig), dim3(256), 0, (hipStream_t)stream,
                     (float2*)spec, desc, power, ltas, (int)rows, (int)bins, (int)frames);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_mixfx_decay_brirs(const float* brir_pool, const float* noise_pool, const int64_t* desc,
                          const double* params, float* out, int32_t* status, int64_t brir_len, int64_t noise_len,
                          int64_t out_len, int64_t jobs, brv_stream_t stream) {
  BRV_REFUSE(!brir_pool || !noise_pool || !desc || !params || !out || !status,
             "null brir_pool, noise_pool, desc, params, out or status");
  BRV_REFUSE(brir_len < 2 || noise_len < 1 || out_len < 2 || jobs < 1 || jobs >= (1LL << 31),
             "requires brir_len >= 2, noise_len >= 1, out_len >= 2, 1 <= jobs < 2^31");
  hipLaunchKernelGGL(decay_brirs_kernel, dim3((unsigned)jobs), dim3(256), 0, (hipStream_t)stream, brir_pool,
                     noise_pool, (const long long*)desc, params, out, status, (long long)brir_len,
                     (long long)noise_len, (long long)out_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}

// the library's last-error message and its two status exports (../status.h)
BRV_DEFINE_STATUS(brv_mixfx_version, brv_mixfx_last_error)
