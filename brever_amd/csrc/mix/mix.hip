// Kernels of the batched mixture engine (include/brever_mix.h; brever_amd/mixture.py drives them).
//
// The long convolutions are uniformly partitioned overlap-save products. The block DFTs run on the fp64 matrix
// pipe of the main library; what is new here is the product between them (partition_mac_kernel) and the small
// kernels around it: gathering signals and BRIRs from pools, split_brir, the energy sums in fp64, the gains
// and labels, and the fused gain-and-sum that writes the requested components.
//
// Everything a kernel indexes with is read from descriptor arrays on the device (the host never learns the
// gains, so a batch has no round trip). A descriptor is therefore checked where it is used: an entry that
// points outside the operand it names is skipped or clamped, never followed.
#include "../../../include/brever_mix.h"
#include "../status.h"
#include "../gfx950.cuh"

namespace {

using brv::lds_barrier;

// ---- gather -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_signals_kernel(const float* __restrict__ pool,
                                                           const long long* __restrict__ desc,
                                                           float* __restrict__ rows, long long pool_len,
                                                           long long row_len) {
  const long long r = blockIdx.y;
  long long src = desc[3*r], n = desc[3*r + 1], dst = desc[3*r + 2];
  if (src < 0 || n < 0 || dst < 0 || src > pool_len || n > pool_len - src) n = 0;
  float* out = rows + r*row_len;
  GRID_STRIDE(i, row_len) {
    const long long k = i - dst;
    out[i] = (k >= 0 && k < n) ? pool[src + k] : 0.f;
  }
}

// split_brir (mixture.py:125-167). numpy's argmax takes the FIRST maximum: ties go to the lower index.
__device__ __forceinline__ void peak_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__global__ __launch_bounds__(256) void pack_brirs_kernel(const float* __restrict__ pool,
                                                         const long long* __restrict__ desc,
                                                         float* __restrict__ rows, long long pool_len,
                                                         long long row_len, int boundary, int max_delay) {
  __shared__ float sv[2][256];
  __shared__ int si[2][256];
  __shared__ int cut[2];
  const long long j = blockIdx.x;
  const long long off = desc[3*j];
  long long taps = desc[3*j + 1];
  const int mode = (int)desc[3*j + 2];
  if (off < 0 || taps < 0 || off > pool_len || 2*taps > pool_len - off) taps = 0;
  // (the peaks are searched in the whole response even where the row holds less of it: what a mixture gets does
  // not depend on the longest response of its batch)
  const float* h = pool + off;
  const int tid = threadIdx.x;
  if (mode != 0) {
    float v0 = -1.f, v1 = -1.f;
    int i0 = 0, i1 = 0;
    for (long long t = tid; t < taps; t += 256) {          // ascending per thread: the first maximum stays
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
    if (tid == 0) {
      int p0 = si[0][0], p1 = si[1][0];
      const int strong = sv[0][0] > sv[1][0] ? 0 : 1;      // peak_val[0] > peak_val[1], else the right ear leads
      const int from = strong == 0 ? p0 : p1;
      float best = -1.f;
      int at = 0;
      for (int d = 0; d < max_delay && from + d < taps; ++d) {
        const float a = fabsf(h[2*(long long)(from + d) + (1 - strong)]);
        if (a > best) { best = a; at = d; }
      }
      if (strong == 0) p1 = p0 + at; else p0 = p1 + at;
      cut[0] = p0 + boundary; cut[1] = p1 + boundary;
    }
    __syncthreads();
  }
  for (int ear = 0; ear < 2; ++ear) {
    float* out = rows + (2*j + ear)*row_len;
    const int c = mode != 0 ? cut[ear] : 0;
    for (long long t = tid; t < row_len; t += 256) {
      float v = t < taps ? h[2*t + ear] : 0.f;            // (t < row_len)
      if ((mode == 1 && t >= c) || (mode == 2 && t < c)) v = 0.f;
      out[t] = v;
    }
  }
}

// ---- the partition multiply-accumulate ------------------------------------------------------------------------
// One workgroup = one output slot x MAC_BINS bins, one wave per bin; a lane owns four consecutive frames.
//   LDS: the H column tile of the job, (hl.re, hl.im, hr.re, hr.im) per (bin, partition): every lane of a wave
//   reads the same address (a broadcast); the X frames [c0 - parts, c0 + 256) of the job's signal, stored by
//   frame phase (frame & 3) so that the four frames a lane needs next are four reads at lane-consecutive
//   addresses. Per four partitions a lane reads 4 X values and 4 H values for 32 complex multiply-adds: the
//   X window slides through registers (a, b, c, d <- the quad below), H never leaves LDS. A slot with one job
//   keeps its H tile across frame chunks.
// The sums run over p ascending, job after job, in fused multiply-adds on one accumulator per output: nothing
// of it depends on the batch (the LDS strides do, the arithmetic does not).
constexpr int MAC_BINS = 4;
constexpr int MAC_CHUNK = 256;
constexpr int MAC_MAX_PARTS = BRV_MIX_MAX_PARTS;

struct MacParams {
  const float2* x; const float2* h; float2* y; const int* slots; const int* jobs;
  int nslots, njobs, xrows, xframes, hrows, hparts, bins, yframes, ppad;
};

__device__ __forceinline__ void cmac2(float2& yl, float2& yr, const float2 x, const float4 h) {
  yl.x = fmaf(x.x, h.x, yl.x); yl.x = fmaf(-x.y, h.y, yl.x);
  yl.y = fmaf(x.x, h.y, yl.y); yl.y = fmaf(x.y, h.x, yl.y);
  yr.x = fmaf(x.x, h.z, yr.x); yr.x = fmaf(-x.y, h.w, yr.x);
  yr.y = fmaf(x.x, h.w, yr.y); yr.y = fmaf(x.y, h.z, yr.y);
}

__global__ __launch_bounds__(256) void partition_mac_kernel(const MacParams p) {
  extern __shared__ float4 smem[];
  const int wq = (p.ppad + MAC_CHUNK)/4;
  float4* Hs = smem;                                               // [MAC_BINS][ppad]
  float2* Xs = reinterpret_cast<float2*>(smem + MAC_BINS*p.ppad);  // [MAC_BINS][4][wq]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.y, bin0 = blockIdx.x*MAC_BINS, bin = bin0 + wave;
  int begin = p.slots[3*s], end = p.slots[3*s + 1], frames = p.slots[3*s + 2];
  if (begin < 0) begin = 0;
  if (end > p.njobs) end = p.njobs;
  if (frames < 0) frames = 0;
  if (frames > p.yframes) frames = p.yframes;
  const bool single = end - begin == 1;
  const float2 zero2 = make_float2(0.f, 0.f);

  for (int c0 = 0; c0 < p.yframes; c0 += MAC_CHUNK) {
    float2 yl[4], yr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { yl[r] = zero2; yr[r] = zero2; }
    if (c0 < frames) {
      for (int j = begin; j < end; ++j) {
        const int xr = p.jobs[3*j], hr = p.jobs[3*j + 1];
        int parts = p.jobs[3*j + 2];
        if (xr < 0 || xr >= p.xrows || hr < 0 || hr + 1 >= p.hrows || parts < 1) continue;   // (uniform)
        if (parts > p.hparts) parts = p.hparts;
        if (parts > p.ppad) parts = p.ppad;
        const int pq = (parts + 3) & ~3;
        lds_barrier();                                   // the readers of the previous tile are done
        if (!(single && c0 > 0)) {
          for (int e = tid; e < MAC_BINS*pq; e += 256) {
            const int b = e/pq, q = e - b*pq;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < parts && bin0 + b < p.bins) {
              const float2 hl = p.h[((long long)hr*p.bins + bin0 + b)*p.hparts + q];
              const float2 hrr = p.h[((long long)(hr + 1)*p.bins + bin0 + b)*p.hparts + q];
              v = make_float4(hl.x, hl.y, hrr.x, hrr.y);
            }
            Hs[b*p.ppad + q] = v;
          }
        }
        const int win = pq + MAC_CHUNK;
        for (int e = tid; e < MAC_BINS*win; e += 256) {
          const int b = e/win, i = e - b*win;
          const int f = c0 - pq + i;
          float2 v = zero2;
          if (f >= 0 && f < p.xframes && bin0 + b < p.bins)
            v = p.x[((long long)xr*p.bins + bin0 + b)*p.xframes + f];
          Xs[(b*4 + (i & 3))*wq + (i >> 2)] = v;
        }
        lds_barrier();
        if (bin < p.bins) {
          const float2* X0 = Xs + (wave*4 + 0)*wq + pq/4 + lane;
          const float2* X1 = X0 + wq;
          const float2* X2 = X1 + wq;
          const float2* X3 = X2 + wq;
          const float4* H = Hs + wave*p.ppad;
          float2 a = X0[0], b = X1[0], c = X2[0], d = X3[0];
          for (int q = 0; q < pq/4; ++q) {
            const float2 n4 = X0[-q - 1], n3 = X1[-q - 1], n2 = X2[-q - 1], n1 = X3[-q - 1];
            const float4 h0 = H[4*q], h1 = H[4*q + 1], h2 = H[4*q + 2], h3 = H[4*q + 3];
            cmac2(yl[0], yr[0], a, h0); cmac2(yl[1], yr[1], b, h0); cmac2(yl[2], yr[2], c, h0); cmac2(yl[3], yr[3], d, h0);
            cmac2(yl[0], yr[0], n1, h1); cmac2(yl[1], yr[1], a, h1); cmac2(yl[2], yr[2], b, h1); cmac2(yl[3], yr[3], c, h1);
            cmac2(yl[0], yr[0], n2, h2); cmac2(yl[1], yr[1], n1, h2); cmac2(yl[2], yr[2], a, h2); cmac2(yl[3], yr[3], b, h2);
            cmac2(yl[0], yr[0], n3, h3); cmac2(yl[1], yr[1], n2, h3); cmac2(yl[2], yr[2], n1, h3); cmac2(yl[3], yr[3], a, h3);
            a = n4; b = n3; c = n2; d = n1;
          }
        }
      }
    }
    if (bin < p.bins) {
      float2* outl = p.y + ((long long)(2*s)*p.bins + bin)*p.yframes;
      float2* outr = p.y + ((long long)(2*s + 1)*p.bins + bin)*p.yframes;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = c0 + 4*lane + r;
        if (f < p.yframes) {
          outl[f] = f < frames ? yl[r] : zero2;
          outr[f] = f < frames ? yr[r] : zero2;
        }
      }
    }
  }
}

// ---- energies ---------------------------------------------------------------------------------------------------
// samples per workgroup: the chunking depends on a mixture's own length only
constexpr int EN_CHUNK = BRV_MIX_ENERGY_CHUNK;
constexpr int EN_SUMS = 40;

__global__ __launch_bounds__(256) void energies_kernel(const float* __restrict__ y, const int* __restrict__ mix,
                                                       double* __restrict__ partials, long long row_len,
                                                       int chunks) {
  __shared__ double red[4][EN_SUMS];
  const int m = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  long long T = mix[4*m], se = mix[4*m + 1], i0 = mix[4*m + 2], i1 = mix[4*m + 3];
  if (T > row_len) T = row_len;
  const float* base = y + (long long)m*8*row_len;
  double acc[EN_SUMS];
#pragma unroll
  for (int k = 0; k < EN_SUMS; ++k) acc[k] = 0.0;
  for (int i = 0; i < EN_CHUNK/256; ++i) {
    const long long t = (long long)chunk*EN_CHUNK + tid + 256*i;
    if (t >= T) break;
    double l[4], r[4], mean[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool live = c >= 2 || t < se;
      l[c] = live ? (double)base[(2*c)*row_len + t] : 0.0;
      r[c] = live ? (double)base[(2*c + 1)*row_len + t] : 0.0;
      mean[c] = 0.5*(l[c] + r[c]);
    }
    const bool in = t >= i0 && t < i1;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = a; b < 4; ++b, ++k) {
        const double mm = mean[a]*mean[b];
        if (in) acc[k] += mm;
        acc[10 + k] += mm;
        acc[20 + k] = fma(l[a], l[b], acc[20 + k]);
        acc[30 + k] = fma(r[a], r[b], acc[30 + k]);
      }
  }
#pragma unroll
  for (int k = 0; k < EN_SUMS; ++k) {
    double v = acc[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < EN_SUMS)
    partials[((long long)m*chunks + chunk)*EN_SUMS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ---- gains and labels ---------------------------------------------------------------------------------------------
// upper-triangle index of (a, b), a <= b, in a 4 x 4 Gram matrix
__device__ __forceinline__ int tri(int a, int b) { return a*4 - a*(a - 1)/2 + (b - a); }
// energy of sum_c g[c] x_c from the Gram matrix of the x_c
__device__ double quad(const double* G, const double* g) {
  double e = 0.0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b) e += (a == b ? 1.0 : 2.0)*g[a]*g[b]*G[tri(a, b)];
  return e;
}

__global__ __launch_bounds__(256) void gains_kernel(const double* __restrict__ partials, const int* __restrict__ mix,
                                                    const double* __restrict__ params, double* __restrict__ gains,
                                                    double* __restrict__ labels, int* __restrict__ status,
                                                    long long mixtures, int chunks) {
  GRID_STRIDE(m, mixtures) {
    const long long T = mix[4*m];
    long long n = (T + EN_CHUNK - 1)/EN_CHUNK;
    if (n > chunks) n = chunks;
    double G[EN_SUMS];
    for (int k = 0; k < EN_SUMS; ++k) G[k] = 0.0;
    for (long long c = 0; c < n; ++c)                            // chunk order: fixed by the mixture's length
      for (int k = 0; k < EN_SUMS; ++k) G[k] += partials[(m*chunks + c)*EN_SUMS + k];
    const double* Gs = G;            // channel means over speech_idx
    const double* Gf = G + 10;       // channel means, whole mixture
    const double ndr = params[4*m], snr = params[4*m + 1], tmr = params[4*m + 2], jitter = params[4*m + 3];
    double g[4] = {1.0, 1.0, 1.0, 1.0};                           // early, late, dir, diffuse
    double g_ndr = 1.0, g_snr = 1.0, g_tmr = 1.0, g_rms = 1.0;
    int st = 0;
    if (ndr == ndr) {                                             // adjust_snr(dir_noise, diffuse, ndr)
      const double es = Gf[tri(2, 2)], en = Gf[tri(3, 3)];
      if (es == 0.0) st = 1; else if (en == 0.0) st = 2;
      else { g_ndr = sqrt(pow(10.0, -ndr/10.0)*es/en); g[3] *= g_ndr; }
    }
    if (st == 0 && snr == snr) {                                  // adjust_snr(foreground, background, snr, speech_idx)
      const double bg[4] = {0.0, g[1], g[2], g[3]};
      const double es = Gs[tri(0, 0)], en = quad(Gs, bg);
      if (es == 0.0) st = 1; else if (en == 0.0) st = 2;
      else { g_snr = sqrt(pow(10.0, -snr/10.0)*es/en); g[2] *= g_snr; g[3] *= g_snr; }
    }
    if (st == 0 && tmr == tmr) {                                  // set_tmr: no check in the reference either
      const double bg[4] = {0.0, g[1], g[2], g[3]};
      g_tmr = sqrt(Gf[tri(0, 0)]*(1.0/tmr - 1.0)/quad(Gf, bg));
      g[1] *= g_tmr; g[2] *= g_tmr; g[3] *= g_tmr;
    }
    if (st == 0) {                                                // set_rms(get_rms() + jitter)
      const double ms0 = quad(G + 20, g)/(double)T, ms1 = quad(G + 30, g)/(double)T;
      const double rms_max = sqrt(ms0 > ms1 ? ms0 : ms1);
      const double rms_db = 20.0*log10(rms_max) + jitter;
      g_rms = pow(10.0, rms_db/20.0)/rms_max;
      for (int c = 0; c < 4; ++c) g[c] *= g_rms;
    }
    const double tgt[4] = {g[0], 0.0, 0.0, 0.0};
    const double m_tmr[4] = {0.0, g[1], g[2], g[3]}, m_tnr[4] = {0.0, 0.0, g[2], g[3]}, m_trr[4] = {0.0, g[1], 0.0, 0.0};
    const double et = quad(Gs, tgt);
    labels[3*m] = et/(et + quad(Gs, m_tmr));
    labels[3*m + 1] = et/(et + quad(Gs, m_tnr));
    labels[3*m + 2] = et/(et + quad(Gs, m_trr));
    for (int c = 0; c < 4; ++c) gains[8*m + c] = g[c];
    gains[8*m + 4] = g_ndr; gains[8*m + 5] = g_snr; gains[8*m + 6] = g_tmr; gains[8*m + 7] = g_rms;
    status[m] = st;
  }
}

// ---- fused gain-and-sum ---------------------------------------------------------------------------------------------
// The sums follow Mixture's properties: speech = early + late, noise = dir + diffuse, mixture = speech + noise,
// background = late + noise.
__global__ __launch_bounds__(256) void compose_kernel(const float* __restrict__ y, const double* __restrict__ gains,
                                                      const int* __restrict__ mix, const int* __restrict__ comps,
                                                      float2* __restrict__ out, int ncomp, long long mixtures,
                                                      long long row_len, long long out_len) {
  const long long m = blockIdx.y;
  long long T = mix[4*m];
  const long long se = mix[4*m + 1];
  if (T > row_len) T = row_len;
  const float* base = y + m*8*row_len;
  float g[4];
  for (int c = 0; c < 4; ++c) g[c] = (float)gains[8*m + c];
  GRID_STRIDE(t, out_len) {
    float2 v[9];
    if (t < T) {
      float2 e[4];
      for (int c = 0; c < 4; ++c) {
        const bool live = c >= 2 || t < se;
        e[c].x = live ? g[c]*base[(2*c)*row_len + t] : 0.f;
        e[c].y = live ? g[c]*base[(2*c + 1)*row_len + t] : 0.f;
      }
      const float2 speech = make_float2(e[0].x + e[1].x, e[0].y + e[1].y);
      const float2 noise = make_float2(e[2].x + e[3].x, e[2].y + e[3].y);
      v[0] = make_float2(speech.x + noise.x, speech.y + noise.y);
      v[1] = e[0];
      v[2] = make_float2(e[1].x + noise.x, e[1].y + noise.y);
      v[3] = speech; v[4] = noise; v[5] = e[0]; v[6] = e[1]; v[7] = e[2]; v[8] = e[3];
    } else {
      for (int c = 0; c < 9; ++c) v[c] = make_float2(0.f, 0.f);
    }
    for (int k = 0; k < ncomp; ++k) {
      const int id = comps[k];
      float2 w = make_float2(0.f, 0.f);
#pragma unroll
      for (int c = 0; c < 9; ++c) if (id == c) w = v[c];
      out[((long long)k*mixtures + m)*out_len + t] = w;
    }
  }
}

unsigned grid_x(long long n) {
  long long g = (n + 255)/256;
  return (unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

}  // namespace

extern "C" {

int brv_mix_pack_signals(const float* pool, const int64_t* desc, float* rows, int64_t pool_len, int64_t nrows,
                         int64_t row_len, brv_stream_t stream) {
  BRV_REFUSE(!pool || !desc || !rows, "null pool, desc or rows");
  BRV_REFUSE(pool_len < 1 || nrows < 1 || row_len < 1 || nrows > 65535,
             "requires pool_len >= 1, 1 <= nrows <= 65535, row_len >= 1");
  hipLaunchKernelGGL(pack_signals_kernel, dim3(grid_x(row_len), (unsigned)nrows), dim3(256), 0, (hipStream_t)stream,
                     pool, (const long long*)desc, rows, (long long)pool_len, (long long)row_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_mix_pack_brirs(const float* pool, const int64_t* desc, float* rows, int64_t pool_len, int64_t jobs,
                       int64_t row_len, int64_t boundary, int64_t max_delay, brv_stream_t stream) {
  BRV_REFUSE(!pool || !desc || !rows, "null pool, desc or rows");
  BRV_REFUSE(pool_len < 2 || pool_len >= (1LL << 31) || jobs < 1 || row_len < 1 || row_len >= (1LL << 30),
             "requires 2 <= pool_len < 2^31, jobs >= 1, 1 <= row_len < 2^30");
  BRV_REFUSE(boundary < 0 || boundary >= (1LL << 30) || max_delay < 1 || max_delay >= (1LL << 30),
             "requires 0 <= boundary < 2^30 and 1 <= max_delay < 2^30");
  hipLaunchKernelGGL(pack_brirs_kernel, dim3((unsigned)jobs), dim3(256), 0, (hipStream_t)stream, pool,
                     (const long long*)desc, rows, (long long)pool_len, (long long)row_len, (int)boundary,
                     (int)max_delay);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_mix_partition_mac(const float* xspec, const float* hspec, float* yspec, const int32_t* slots,
                          const int32_t* jobs, int64_t nslots, int64_t njobs, int64_t xrows, int64_t xframes,
                          int64_t hrows, int64_t hparts, int64_t bins, int64_t yframes, int64_t max_parts,
                          brv_stream_t stream) {
  BRV_REFUSE(!xspec || !hspec || !yspec || !slots || !jobs, "null xspec, hspec, yspec, slots or jobs");
  BRV_REFUSE(nslots < 1 || njobs < 1 || xrows < 1 || xframes < 1 || hrows < 2 || hparts < 1 || bins < 1 ||
             yframes < 1 || max_parts < 1,
             "requires nslots, njobs, xrows, xframes, hparts, bins, yframes, max_parts >= 1 and hrows >= 2");
  const int64_t big = 1LL << 30;
  BRV_REFUSE(nslots > 65535 || njobs >= big || xrows >= big || xframes >= big || hrows >= big || hparts >= big ||
             bins >= big || yframes >= big, "requires nslots <= 65535 and every other count < 2^30");
  BRV_UNSUPPORTED(max_parts > MAC_MAX_PARTS, "more than 512 partitions per impulse response: use a larger block");
  MacParams p;
  p.x = (const float2*)xspec; p.h = (const float2*)hspec; p.y = (float2*)yspec; p.slots = slots; p.jobs = jobs;
  p.nslots = (int)nslots; p.njobs = (int)njobs; p.xrows = (int)xrows; p.xframes = (int)xframes;
  p.hrows = (int)hrows; p.hparts = (int)hparts; p.bins = (int)bins; p.yframes = (int)yframes;
  p.ppad = (int)((max_parts + 3) & ~3LL);
  const size_t lds = (size_t)MAC_BINS*p.ppad*sizeof(float4) + (size_t)MAC_BINS*(p.ppad + MAC_CHUNK)*sizeof(float2);
  const dim3 grid((unsigned)((bins + MAC_BINS - 1)/MAC_BINS), (unsigned)nslots);
  hipLaunchKernelGGL(partition_mac_kernel, grid, dim3(256), lds, (hipStream_t)stream, p);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_mix_energies(const float* y, const int32_t* mix, double* partials, int64_t mixtures, int64_t row_len,
                     int64_t chunks, brv_stream_t stream) {
  BRV_REFUSE(!y || !mix || !partials, "null y, mix or partials");
  BRV_REFUSE(mixtures < 1 || mixtures > 65535 || row_len < 1 || row_len >= (1LL << 31) || chunks < 1,
             "requires 1 <= mixtures <= 65535, 1 <= row_len < 2^31, chunks >= 1");
  BRV_REFUSE(chunks*EN_CHUNK < row_len, "requires chunks*2048 >= row_len");
  hipLaunchKernelGGL(energies_kernel, dim3((unsigned)chunks, (unsigned)mixtures), dim3(256), 0, (hipStream_t)stream,
                     y, mix, partials, (long long)row_len, (int)chunks);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_mix_gains(const double* partials, const int32_t* mix, const double* params, double* gains, double* labels,
                  int32_t* status, int64_t mixtures, int64_t chunks, brv_stream_t stream) {
  BRV_REFUSE(!partials || !mix || !params || !gains || !labels || !status,
             "null partials, mix, params, gains, labels or status");
  BRV_REFUSE(mixtures < 1 || chunks < 1 || chunks >= (1LL << 30), "requires mixtures >= 1, 1 <= chunks < 2^30");
  hipLaunchKernelGGL(gains_kernel, dim3(grid_x(mixtures)), dim3(256), 0, (hipStream_t)stream, partials, mix, params,
                     gains, labels, status, (long long)mixtures, (int)chunks);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_mix_compose(const float* y, const double* gains, const int32_t* mix, const int32_t* comps, float* out,
                    int64_t ncomp, int64_t mixtures, int64_t row_len, int64_t out_len, brv_stream_t stream) {
  BRV_REFUSE(!y || !gains || !mix || !comps || !out, "null y, gains, mix, comps or out");
  BRV_REFUSE(ncomp < 1 || ncomp > 9 || mixtures < 1 || mixtures > 65535 || row_len < 1 || out_len < 1,
             "requires 1 <= ncomp <= 9, 1 <= mixtures <= 65535, row_len >= 1, out_len >= 1");
  hipLaunchKernelGGL(compose_kernel, dim3(grid_x(out_len), (unsigned)mixtures), dim3(256), 0, (hipStream_t)stream,
                     y, gains, mix, comps, (float2*)out, (int)ncomp, (long long)mixtures, (long long)row_len,
                     (long long)out_len);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}

// the library's last-error message and its two status exports (../status.h)
BRV_DEFINE_STATUS(brv_mix_version, brv_mix_last_error)
