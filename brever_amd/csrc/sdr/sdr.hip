// BSS-eval signal-to-distortion ratio with an allowed distortion filter of L <= 512 taps (include/brever_sdr.h;
// DESIGN.md 5k): correlation lags, the Toeplitz solve and the gradient of -SDR, everything in fp64 from fp32 signals.
//
//   sdr_corr_kernel      one workgroup per (chunk of 2048 samples, row): the chunk and its 512-sample halo go to LDS
//                        as fp32 (zeros from the row's length on), then lane g of wave p owns the lags [8g, 8g + 8)
//                        over the quarter p of the chunk: 8 x 8 register tiles of v_fma_f64, 128 FMAs per 40 LDS
//                        floats. The four quarters are summed in order and stored as the chunk's partial lags.
//   sdr_solve_kernel     one workgroup (four waves) per row: chunks summed in ascending order, then the Levinson
//                        recursion on r with the right-hand side b (5 L doubles of LDS state), q = b^T h, the
//                        floors, SDR.
//   sdr_backward_kernel  one workgroup per (1024 outputs, row): s through h with both in LDS, four outputs per
//                        lane from a sliding register window, fused with the elementwise expression.
//
// The vector pipe, not v_mfma_f64_16x16x4_f64: on gfx950 the fp64 matrix peak equals the fp64 vector peak, so the
// matrix pipe has no rate to give, while its operands would be diagonals of a Toeplitz tile that LDS reads have to
// gather; the register tile reaches the same FMA : LDS ratio with plain reads.
//
// Every sum has a fixed order (a lane's FMA chain, a scan within a wave, waves / quarters / chunks ascending)
// and there are no atomics. E is accumulated by the very instruction sequence that accumulates r[0], with x for s:
// an estimate that is a power-of-two multiple of the reference gives E - q = 0 exactly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../../include/brever_sdr.h"
#include "../status.h"

namespace {

constexpr int kMaxL = BRV_SDR_MAX_FILTER_LENGTH;   // filter taps; 64 lanes x 8 lags
constexpr int kChunk = BRV_SDR_CHUNK;          // samples per correlation workgroup
constexpr int kParts = 4;                      // waves of a correlation workgroup: quarters of the chunk
constexpr int kPartLen = kChunk/kParts;
constexpr int kStage = kChunk + kMaxL;         // the chunk and its halo
constexpr int kBwdTile = 1024;                 // outputs per backward workgroup, 4 per lane
constexpr int kBwdHalo = kMaxL + 8;            // samples staged in front of them (the window runs 8 ahead)
constexpr double kEps = 2.220446049250313e-16; // 2^-52
constexpr double kTenOverLn10 = 4.342944819032518;
constexpr long long kMaxRows = 65535;          // rows ride on gridDim.y
constexpr int kNoRef = BRV_SDR_FLAG_NO_REFERENCE, kNoEst = BRV_SDR_FLAG_NO_ESTIMATE, kPivot = BRV_SDR_FLAG_BAD_PIVOT,
              kNumFloor = BRV_SDR_FLAG_NUMERATOR_FLOOR, kDenFloor = BRV_SDR_FLAG_DENOMINATOR_FLOOR;

__device__ __forceinline__ long long row_length(const long long* lengths, int row, long long stride) {
  const long long n = lengths[row];
  return n < 0 ? 0 : (n > stride ? stride : n);
}

// v of the lane kShift below within its row of 16 lanes, 0.0 where the row has none (a DPP row shift of both halves)
template <int kShift> __device__ __forceinline__ double row_shr(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x110 + kShift, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x110 + kShift, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_value(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// sum over the 64 lanes, the same bits in every lane: an inclusive scan within each row of 16 lanes (shifts by 1, 2,
// 4, 8 in registers, no LDS round trip), then the four row totals in ascending order
__device__ __forceinline__ double wave_sum(double v) {
  v += row_shr<1>(v); v += row_shr<2>(v); v += row_shr<4>(v); v += row_shr<8>(v);
  return ((lane_value(v, 15) + lane_value(v, 31)) + lane_value(v, 47)) + lane_value(v, 63);
}

__device__ __forceinline__ void load8(const float* p, double* out) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
  out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
}

// slot of (row, chunk) in the workspace: r[0..L), b[0..L), E
__global__ __launch_bounds__(256) void sdr_corr_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const long long* __restrict__ lengths, long long stride,
                                                       int L, int nchunk, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float ss[kStage];
  __shared__ __attribute__((aligned(16))) float xs[kStage];
  __shared__ double red[kParts][2*kMaxL + 1];
  const int row = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const long long T = row_length(lengths, row, stride);
  const long long c0 = (long long)chunk*kChunk;
  if (c0 >= T) return;                         // the solver reads the chunks below ceil(T / kChunk) only
  const float* sy = y + (long long)row*stride;
  const float* sx = x + (long long)row*stride;
  for (int i = tid; i < kStage; i += 256) {
    const long long t = c0 + i;
    const bool in = t < T;
    ss[i] = in ? sy[t] : 0.f;
    xs[i] = in ? sx[t] : 0.f;
  }
  __syncthreads();
  const int g = tid & 63, p = tid >> 6;
  const int k0 = 8*g;
  const int lim = (int)(T - c0 < kChunk ? T - c0 : kChunk);      // samples of the chunk inside the row
  double ar[8], ab[8], ae = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) { ar[i] = 0.0; ab[i] = 0.0; }
  if (k0 < L) {
    const int t_begin = p*kPartLen;
    const int t_end = t_begin + kPartLen < lim ? t_begin + kPartLen : lim;
    // a block of 8 samples that straddles `lim` reads staged zeros; t0 + k0 + 15 <= 2040 + 504 + 15 < kStage
    for (int t0 = t_begin; t0 < t_end; t0 += 8) {
      double sv[8], wsd[16], wxd[16];
      load8(ss + t0, sv);
      load8(ss + t0 + k0, wsd); load8(ss + t0 + k0 + 8, wsd + 8);
      load8(xs + t0 + k0, wxd); load8(xs + t0 + k0 + 8, wxd + 8);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          ar[i] = __builtin_fma(sv[u], wsd[u + i], ar[i]);
          ab[i] = __builtin_fma(sv[u], wxd[u + i], ab[i]);
        }
      }
      if (g == 0) {                            // k0 == 0: wxd[u] = x[t0 + u]; the chain of ar[0] with x for s
#pragma unroll
        for (int u = 0; u < 8; ++u) ae = __builtin_fma(wxd[u], wxd[u], ae);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) { red[p][k0 + i] = ar[i]; red[p][kMaxL + k0 + i] = ab[i]; }
    if (g == 0) red[p][2*kMaxL] = ae;
  }
  __syncthreads();
  double* slot = ws + ((long long)row*nchunk + chunk)*(2*L + 1);
  for (int k = tid; k < L; k += 256) {
    slot[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    slot[L + k] = ((red[0][kMaxL + k] + red[1][kMaxL + k]) + red[2][kMaxL + k]) + red[3][kMaxL + k];
  }
  if (tid == 0) slot[2*L] = ((red[0][2*kMaxL] + red[1][2*kMaxL]) + red[2][2*kMaxL]) + red[3][2*kMaxL];
}

// Levinson recursion: after step n, a[0..n] (a[0] = 1) is the forward predictor of order n with error `err`, and
// xh[0..n] solves the leading (n + 1) x (n + 1) system. A step is two dot products of length n, one reduction, one
// division and one update, and its cost is the latency of that chain, not its work: four waves, so that a lane holds
// two elements (j and j + 256) whose LDS reads are all in flight at once; the sum over a wave stays in registers
// (wave_sum), the four waves meet through 8 doubles of LDS. Every lane computes the same lam / mu from the same
// words, so the pivot test is uniform.
__global__ __launch_bounds__(256) void sdr_solve_kernel(const double* __restrict__ ws,
                                                        const long long* __restrict__ lengths, long long stride,
                                                        int L, int nchunk, double load_diag,
                                                        double* __restrict__ sdr, double* __restrict__ h,
                                                        double* __restrict__ q_out, double* __restrict__ e_out,
                                                        int* __restrict__ flags) {
  static_assert(kMaxL == 2*256, "a lane of the solver holds the elements j and j + 256");
  __shared__ double r[kMaxL], b[kMaxL], a[2][kMaxL], xh[kMaxL];
  __shared__ double part[4][2];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long T = row_length(lengths, row, stride);
  const int nc = (int)((T + kChunk - 1)/kChunk);                 // <= nchunk since T <= stride
  const int slot = 2*L + 1;
  const double* base = ws + (long long)row*nchunk*slot;
  for (int k = tid; k < L; k += 256) {
    double sr = 0.0, sb = 0.0;
    for (int c = 0; c < nc; ++c) { sr += base[(long long)c*slot + k]; sb += base[(long long)c*slot + L + k]; }
    r[k] = sr; b[k] = sb;
  }
  double E = 0.0;
  for (int c = 0; c < nc; ++c) E += base[(long long)c*slot + 2*L];
  __syncthreads();
  const double r0 = r[0];
  int fl = (r0 > 0.0 ? 0 : kNoRef) | (E > 0.0 ? 0 : kNoEst);
  const double r0l = r0 + load_diag*r0;
  if (!fl) {
    if (tid == 0) { a[0][0] = 1.0; a[1][0] = 1.0; xh[0] = b[0]/r0l; }
    __syncthreads();
    double err = r0l, inv = 1.0/r0l;
    int cur = 0;
    const int j0 = tid, j1 = tid + 256;
    for (int n = 1; n < L; ++n) {
      // dot products over j < n; an index that is out of range reads word 0 and its product is dropped
      const bool d0 = j0 < n, d1 = j1 < n;
      const double ra = r[d0 ? n - j0 : 0], aa = a[cur][d0 ? j0 : 0], xa = xh[d0 ? j0 : 0];
      const double rb = r[d1 ? n - j1 : 0], ab = a[cur][d1 ? j1 : 0], xb = xh[d1 ? j1 : 0];
      double pa = d0 ? aa*ra : 0.0, px = d0 ? xa*ra : 0.0;
      if (d1) { pa = __builtin_fma(ab, rb, pa); px = __builtin_fma(xb, rb, px); }
      pa = wave_sum(pa); px = wave_sum(px);
      if (lane == 0) { part[wave][0] = pa; part[wave][1] = px; }
      __syncthreads();
      const double sa = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
      const double sx = ((part[0][1] + part[1][1]) + part[2][1]) + part[3][1];
      const double lam = -sa*inv;
      err *= 1.0 - lam*lam;
      if (!(err > 0.0)) { fl |= kPivot; break; }
      inv = 1.0/err;
      const double mu = (b[n] - sx)*inv;
      // update over j <= n: a_new[j] = a[j] + lam a[n - j] (the old predictor is 0 at n), xh[j] += mu a_new[n - j],
      // xh[n] = mu. aa / ab already hold a[j] for j < n.
      const bool u0 = j0 <= n, u1 = j1 <= n;
      const double na = a[cur][(u0 && j0 > 0) ? n - j0 : 0], nb = a[cur][u1 ? n - j1 : 0];
      if (u0) {
        const double ao_j = d0 ? aa : 0.0, ao_nj = j0 > 0 ? na : 0.0;
        a[cur ^ 1][j0] = __builtin_fma(lam, ao_nj, ao_j);
        xh[j0] = d0 ? __builtin_fma(mu, __builtin_fma(lam, ao_j, ao_nj), xa) : mu;
      }
      if (u1) {
        const double ao_j = d1 ? ab : 0.0;
        a[cur ^ 1][j1] = __builtin_fma(lam, nb, ao_j);
        xh[j1] = d1 ? __builtin_fma(mu, __builtin_fma(lam, ao_j, nb), xb) : mu;
      }
      cur ^= 1;
      __syncthreads();
    }
  }
  __syncthreads();
  double* hr = h + (long long)row*L;
  if (fl) {
    for (int k = tid; k < L; k += 256) hr[k] = 0.0;
    if (tid == 0) { sdr[row] = __builtin_nan(""); q_out[row] = 0.0; e_out[row] = E; flags[row] = fl; }
    return;
  }
  double pq = 0.0;
  for (int k = tid; k < L; k += 256) { const double hk = xh[k]; hr[k] = hk; pq = __builtin_fma(b[k], hk, pq); }
  pq = wave_sum(pq);
  if (lane == 0) part[wave][0] = pq;
  __syncthreads();
  if (tid == 0) {
    const double q = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
    const double floor_ = kEps*E, d = E - q;
    if (q < floor_) fl |= kNumFloor;
    if (d < floor_) fl |= kDenFloor;
    sdr[row] = 10.0*log10((q < floor_ ? floor_ : q)/(d < floor_ ? floor_ : d));
    q_out[row] = q; e_out[row] = E; flags[row] = fl;
  }
}

__global__ __launch_bounds__(256) void sdr_backward_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const long long* __restrict__ lengths,
                                                           const double* __restrict__ h,
                                                           const double* __restrict__ q_in,
                                                           const double* __restrict__ e_in,
                                                           const int* __restrict__ flags,
                                                           const double* __restrict__ grow, long long stride, int L,
                                                           float* __restrict__ dx) {
  __shared__ __attribute__((aligned(16))) float ss[kBwdHalo + kBwdTile];   // s[c0 - kBwdHalo, c0 + kBwdTile)
  __shared__ double hs[kMaxL];
  const int row = blockIdx.y, tid = threadIdx.x;
  const long long c0 = (long long)blockIdx.x*kBwdTile;
  const long long T = row_length(lengths, row, stride);
  float* out = dx + (long long)row*stride;
  const int fl = flags[row];
  if (c0 >= T || (fl & (kNoRef | kNoEst | kPivot))) {
    for (int i = tid; i < kBwdTile; i += 256) if (c0 + i < stride) out[c0 + i] = 0.f;
    return;
  }
  const float* sy = y + (long long)row*stride;
  const float* sx = x + (long long)row*stride;
  for (int i = tid; i < kBwdHalo + kBwdTile; i += 256) {
    const long long t = c0 - kBwdHalo + i;
    ss[i] = (t >= 0 && t < T) ? sy[t] : 0.f;
  }
  for (int k = tid; k < kMaxL; k += 256) hs[k] = k < L ? h[(long long)row*L + k] : 0.0;
  __syncthreads();
  // lane outputs t = c0 + 4 tid + i, i < 4. In the group of taps [k, k + 4), w[m] = s[t - k - 4 + m]: output i and
  // tap k + kk meet at w[4 + i - kk]. Indices stay in [kBwdHalo - 516, kBwdHalo + 1023].
  const int o = kBwdHalo + 4*tid;
  float4 hi = *reinterpret_cast<const float4*>(ss + o), lo = *reinterpret_cast<const float4*>(ss + o - 4);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const int Lq = (L + 3) & ~3;                                   // hs is 0 from L on
  for (int k = 0; k < Lq; k += 4) {
    const double w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const double hk = hs[k + kk];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __builtin_fma(hk, w[4 + i - kk], acc[i]);
    }
    hi = lo;
    lo = *reinterpret_cast<const float4*>(ss + o - k - 8);
  }
  const double q = q_in[row], d = e_in[row] - q, gr = grow[row];
  const double c1 = (fl & kNumFloor) ? 0.0 : 2.0/q;
  const double c2 = (fl & kDenFloor) ? 0.0 : 2.0/d;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long t = c0 + 4*tid + i;
    if (t >= stride) break;
    float v = 0.f;
    if (t < T) v = (float)(gr*(-kTenOverLn10*(c1*acc[i] - c2*((double)sx[t] - acc[i]))));
    out[t] = v;
  }
}

const char* kShape = "requires 1 <= rows <= 65535, 1 <= stride <= 2^40, 1 <= filter_length <= 512";

bool bad_shape(int64_t rows, int64_t stride, int64_t L) {
  return rows < 1 || rows > kMaxRows || stride < 1 || stride > (1ll << 40) || L < 1 || L > kMaxL;
}

}  // namespace

extern "C" {

int64_t brv_sdr_max_filter_length(void) { return kMaxL; }
int64_t brv_sdr_chunk(void) { return kChunk; }

int64_t brv_sdr_workspace_bytes(int64_t rows, int64_t stride, int64_t filter_length) {
  if (bad_shape(rows, stride, filter_length)) return brv::fail(-1, kShape);
  const int64_t nchunk = (stride + kChunk - 1)/kChunk;
  return rows*nchunk*(2*filter_length + 1)*(int64_t)sizeof(double);
}

int brv_sdr_forward(const float* x, const float* y, const int64_t* lengths, int64_t rows, int64_t stride,
                    int64_t filter_length, float load_diag, void* workspace, double* sdr, double* h, double* q,
                    double* e, int32_t* flags, brv_stream_t stream) {
  BRV_REFUSE(!x || !y || !lengths || !workspace || !sdr || !h || !q || !e || !flags,
             "null pointer: x, y, lengths, workspace, sdr, h, q, e and flags are required");
  BRV_REFUSE(bad_shape(rows, stride, filter_length), kShape);
  BRV_REFUSE(!(load_diag >= 0.f) || !(load_diag <= 1e6f), "requires 0 <= load_diag <= 1e6");
  const int64_t nchunk = (stride + kChunk - 1)/kChunk;
  BRV_REFUSE(nchunk > 0x7fffffff, "requires stride <= 2^31 x 2048");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sdr_corr_kernel, dim3((unsigned)nchunk, (unsigned)rows), dim3(256), 0, st, x, y,
                     (const long long*)lengths, (long long)stride, (int)filter_length, (int)nchunk,
                     (double*)workspace);
  hipLaunchKernelGGL(sdr_solve_kernel, dim3((unsigned)rows), dim3(256), 0, st, (const double*)workspace,
                     (const long long*)lengths, (long long)stride, (int)filter_length, (int)nchunk, (double)load_diag, sdr,
                     h, q, e, (int*)flags);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_sdr_backward(const float* x, const float* y, const int64_t* lengths, const double* h, const double* q,
                     const double* e, const int32_t* flags, const double* grad_rows, int64_t rows, int64_t stride,
                     int64_t filter_length, float* dx, brv_stream_t stream) {
  BRV_REFUSE(!x || !y || !lengths || !h || !q || !e || !flags || !grad_rows || !dx,
             "null pointer: x, y, lengths, h, q, e, flags, grad_rows and dx are required");
  BRV_REFUSE(bad_shape(rows, stride, filter_length), kShape);
  const int64_t ntile = (stride + kBwdTile - 1)/kBwdTile;
  BRV_REFUSE(ntile > 0x7fffffff, "requires stride <= 2^31 x 1024");
  hipLaunchKernelGGL(sdr_backward_kernel, dim3((unsigned)ntile, (unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                     x, y, (const long long*)lengths, h, q, e, (const int*)flags, grad_rows, (long long)stride,
                     (int)filter_length, dx);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}

// SIR and SAR: the joint projection on several references (include/sdr/brever_bsseval.h), on the kernels above
#include "bsseval.cuh"

// the library's last-error message and its two status exports (../status.h)
BRV_DEFINE_STATUS(brv_sdr_version, brv_sdr_last_error)
