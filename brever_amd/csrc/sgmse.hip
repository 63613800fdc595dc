// Building blocks of the SGMSE+ score network (NCSN++ / ADM style U-Net), forward values.
// Reference: brever/models/sgmse/net.py:12-477 (DiffusionUNet, UNetBlock, AttentionBlock,
// NoiseEmbedding, GaussianFourierProjection, GroupNorm) and brever/modules/resampling.py:8-61
// (Resample). Convolutions are brv_conv2d_forward (dccrn.hip), matrix products brv_gemm_f32.
// fp32, NCHW, correctness-first kernels.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/brever_hip.h"
#include "common.cuh"
#include "status.h"

using namespace brv;

namespace {

__device__ __forceinline__ float silu(float v) { return v/(1.f + expf(-v)); }

// GroupNorm in three small steps so that the normalisation itself can be folded into the
// consumer: (1) partial sums of x + add[b][c] over slices of each (item, group), fp64, one
// atomic pair per workgroup on the group's private 128-byte line; (2) fold into a per-(item,
// channel) affine: scale = rstd*gamma*(1 + adm_scale), shift = (beta + (add - mean)*rstd*gamma)
// *(1 + adm_scale) + adm_shift; (3) y = act(scale*x + shift) -- here (affine_act_kernel) or on
// the load path of brv_conv2d_mfma_forward.
constexpr int kGnLine = 16;      // doubles per (item, group) slot

__global__ __launch_bounds__(256) void gn_stats_kernel(const float* x, const float* add,
                                                       double* sums, int C, long long HW,
                                                       int groups, long long slice) {
  __shared__ double scr[8];
  const int bg = blockIdx.x, b = bg / groups, g = bg % groups;
  const int cpg = C/groups;
  const long long n = (long long)cpg*HW;
  const float* xg = x + ((long long)b*C + (long long)g*cpg)*HW;
  const float* ag = add ? add + (long long)b*C + (long long)g*cpg : nullptr;
  const long long lo = (long long)blockIdx.y*slice;
  long long hi = lo + slice;
  if (hi > n) hi = n;
  double s = 0.0, q = 0.0;
  if ((HW & 3) == 0 && ((uintptr_t)x & 15) == 0) {
    // channel by channel (the embedding term is constant along a channel; one division per
    // channel instead of one per element), 16-byte loads, fp32 partial sums over at most 16
    // vectors before they are added to the fp64 accumulators
    long long i = lo;                                     // lo, HW: multiples of 4
    while (i < hi) {
      const long long c = i / HW;
      const long long seg_end = min(hi, (c + 1)*HW);
      const float a = ag ? ag[c] : 0.f;
      for (long long j0 = i + 4*threadIdx.x; j0 < seg_end; j0 += 16*1024) {
        float fs = 0.f, fq = 0.f;
#pragma unroll 4
        for (int u = 0; u < 16; ++u) {
          const long long j = j0 + (long long)u*1024;
          if (j >= seg_end) break;
          float4 v = *reinterpret_cast<const float4*>(xg + j);
          v.x += a; v.y += a; v.z += a; v.w += a;
          fs += (v.x + v.y) + (v.z + v.w);
          fq = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, fq))));
        }
        s += fs; q += fq;
      }
      i = seg_end;
    }
  } else {
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
      const float v = xg[i] + (ag ? ag[i / HW] : 0.f);
      s += v; q += (double)v*v;
    }
  }
  s = block_sum(s, scr); __syncthreads();
  q = block_sum(q, scr);
  if (threadIdx.x == 0 && lo < hi) {
    atomicAdd(&sums[(long long)bg*kGnLine], s);
    atomicAdd(&sums[(long long)bg*kGnLine + 1], q);
  }
}

// one workgroup per (item, group); the group's sums are cleared again once read, so the
// scratch is all zeros whenever a stats kernel starts (it is zeroed once, when allocated)
__global__ __launch_bounds__(64) void gn_fold_kernel(double* sums, const float* add,
                                                     const float* gamma, const float* beta,
                                                     const float* adm_scale, const float* adm_shift,
                                                     float* scale, float* shift, float* mu_out,
                                                     float* rstd_out, int C, long long HW,
                                                     int groups, float eps) {
  const int bg = blockIdx.x, b = bg / groups, g = bg % groups;
  const int cpg = C/groups;
  const double n = (double)cpg*(double)HW;
  const double s1 = sums[(long long)bg*kGnLine], s2 = sums[(long long)bg*kGnLine + 1];
  __syncthreads();
  if (threadIdx.x == 0) { sums[(long long)bg*kGnLine] = 0.0; sums[(long long)bg*kGnLine + 1] = 0.0; }
  const double mean = s1/n;
  double var = s2/n - mean*mean;
  if (var < 0) var = 0;
  const float rstd = (float)(1.0/sqrt(var + (double)eps));
  for (int j = threadIdx.x; j < cpg; j += 64) {
    const int c = g*cpg + j, idx = b*C + c;
    float sc = rstd*gamma[c];
    float sh = beta[c] + ((add ? add[idx] : 0.f) - (float)mean)*sc;
    if (adm_scale) { const float m = 1.f + adm_scale[idx]; sc *= m; sh = sh*m + adm_shift[idx]; }
    scale[idx] = sc; shift[idx] = sh;
    if (mu_out) { mu_out[idx] = (float)mean - (add ? add[idx] : 0.f); rstd_out[idx] = rstd; }
  }
}

// y[b][c][:] = act(scale[b][c]*x + shift[b][c])
__global__ __launch_bounds__(256) void affine_act_kernel(const float* x, const float* scale,
                                                         const float* shift, float* y,
                                                         long long HW, long long total, int act) {
  GRID_STRIDE(i4, total/4) {
    const long long i = i4*4;
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long bc = (i + j)/HW;
      const float t = scale[bc]*r[j] + shift[bc];
      r[j] = act ? silu(t) : t;
    }
    *reinterpret_cast<float4*>(y + i) = make_float4(r[0], r[1], r[2], r[3]);
  }
  if (blockIdx.x == 0 && threadIdx.x < (total & 3)) {
    const long long i = (total & ~3LL) + threadIdx.x;
    const float t = scale[i/HW]*x[i] + shift[i/HW];
    y[i] = act ? silu(t) : t;
  }
}

// ---- backward of y = act(GroupNorm(x + add)) in the folded form ------------------------------
// pre = scale*x + shift, u = dy*act'(pre), xhat = (x - mu)*rstd (mu = group mean - add).
// (1) per (item, channel): s1 = sum u, s2 = sum u*xhat, s3 = sum xhat over the pixels (fp64
// partials per slice); (2) per (item, group): A = sum_c gamma s1, Bg = sum_c gamma s2 and the
// coefficients of dx = k1*u + k2*xhat + k3 with k1 = rstd*gamma, k2 = -rstd*Bg/n, k3 =
// -rstd*A/n, plus d add = k1*s1 + k2*s3 + k3*HW; (3) the elementwise pass.
__device__ __forceinline__ float dsilu(float p) {
  const float sg = 1.f/(1.f + expf(-p));
  return sg*(1.f + p*(1.f - sg));
}
__global__ __launch_bounds__(256) void gn_bwd_sums_kernel(const float* x, const float* dy,
                                                          const float* scale, const float* shift,
                                                          const float* mu, const float* rstd,
                                                          double* part, long long HW, int act) {
  __shared__ double scr[8];
  const long long bc = blockIdx.x;
  const long long per = (HW + gridDim.y - 1)/gridDim.y;
  const long long lo = blockIdx.y*per, hi = lo + per < HW ? lo + per : HW;
  const float sc = scale[bc], sh = shift[bc], m = mu[bc], r = rstd[bc];
  const float* xp = x + bc*HW; const float* dp = dy + bc*HW;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const float xv = xp[i];
    const float u = act ? dp[i]*dsilu(sc*xv + sh) : dp[i];
    const float xh = (xv - m)*r;
    s1 += u; s2 += (double)u*xh; s3 += xh;
  }
  s1 = block_sum(s1, scr); __syncthreads();
  s2 = block_sum(s2, scr); __syncthreads();
  s3 = block_sum(s3, scr);
  if (threadIdx.x == 0) {
    double* o = part + (bc*gridDim.y + blockIdx.y)*3;
    o[0] = s1; o[1] = s2; o[2] = s3;
  }
}
__global__ __launch_bounds__(64) void gn_bwd_coef_kernel(const double* part, int slices,
                                                         const float* gamma, const float* rstd,
                                                         float* k1, float* k2, float* k3,
                                                         float* s1_out, float* s2_out, float* dadd,
                                                         int C, long long HW, int groups) {
  __shared__ double gs1[64], gs2[64];              // gamma-weighted sums of the group's channels
  const int bg = blockIdx.x, b = bg / groups, g = bg % groups;
  const int cpg = C/groups, j = threadIdx.x;       // cpg <= 64 (checked by the caller)
  const long long bc = (long long)b*C + g*cpg + j;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  float gm = 0.f;
  if (j < cpg) {
    for (int i = 0; i < slices; ++i) {
      const double* o = part + (bc*slices + i)*3;
      s1 += o[0]; s2 += o[1]; s3 += o[2];
    }
    gm = gamma[g*cpg + j];
    s1_out[bc] = (float)s1; s2_out[bc] = (float)s2;
  }
  gs1[j] = gm*s1; gs2[j] = gm*s2;
  __syncthreads();
  double A = 0.0, Bg = 0.0;
  for (int t = 0; t < cpg; ++t) { A += gs1[t]; Bg += gs2[t]; }
  if (j < cpg) {
    const double n = (double)cpg*(double)HW;
    const float r = rstd[bc];
    const float c1 = r*gm, c2 = (float)(-r*Bg/n), c3 = (float)(-r*A/n);
    k1[bc] = c1; k2[bc] = c2; k3[bc] = c3;
    if (dadd) dadd[bc] = (float)(c1*s1 + c2*s3 + c3*(double)HW);
  }
}
__global__ __launch_bounds__(256) void affine_bwd_final_kernel(const double* part, int slices,
                                                               float* s1_out, float* s2_out, int n) {
  const int bc = blockIdx.x*256 + threadIdx.x;
  if (bc >= n) return;
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < slices; ++i) { s1 += part[((long long)bc*slices + i)*3]; s2 += part[((long long)bc*slices + i)*3 + 1]; }
  s1_out[bc] = (float)s1; s2_out[bc] = (float)s2;
}
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* x, const float* dy,
                                                           const float* scale, const float* shift,
                                                           const float* mu, const float* rstd,
                                                           const float* k1, const float* k2,
                                                           const float* k3, float* dx, long long HW,
                                                           long long total, int act) {
  GRID_STRIDE(i, total) {
    const long long bc = i/HW;
    const float xv = x[i];
    const float u = act ? dy[i]*dsilu(scale[bc]*xv + shift[bc]) : dy[i];
    dx[i] = k1[bc]*u + k2[bc]*(xv - mu[bc])*rstd[bc] + k3[bc];
  }
}
__global__ __launch_bounds__(256) void silu_bwd_kernel(const float* x, const float* dy, float* dx,
                                                       long long n) {
  GRID_STRIDE(i, n) dx[i] = dy[i]*dsilu(x[i]);
}
// dx = p*(dy - sum_j dy_j p_j) per row
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* p, const float* dy, float* dx,
                                                          int cols) {
  __shared__ float red[8];
  __shared__ float bc;
  const float* pr = p + (long long)blockIdx.x*cols;
  const float* dr = dy + (long long)blockIdx.x*cols;
  float* xr = dx + (long long)blockIdx.x*cols;
  float s = 0.f;
  for (int i = threadIdx.x; i < cols; i += 256) s += pr[i]*dr[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) bc = s;
  __syncthreads();
  const float dot = bc;
  for (int i = threadIdx.x; i < cols; i += 256) xr[i] = pr[i]*(dr[i] - dot);
}

__global__ __launch_bounds__(256) void silu_kernel(const float* x, float* y, long long n) {
  GRID_STRIDE(i, n) y[i] = silu(x[i]);
}

// softmax over the last dimension, one workgroup per row
__global__ __launch_bounds__(256) void softmax_kernel(const float* x, float* y, int cols) {
  __shared__ float red[8];
  __shared__ float bc[2];
  const float* xr = x + (long long)blockIdx.x*cols;
  float* yr = y + (long long)blockIdx.x*cols;
  float m = -INFINITY;
  for (int i = threadIdx.x; i < cols; i += 256) m = fmaxf(m, xr[i]);
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) bc[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  m = bc[0];
  float s = 0.f;
  for (int i = threadIdx.x; i < cols; i += 256) s += expf(xr[i] - m);
  s = block_sum(s, red);
  if (threadIdx.x == 0) bc[1] = s;
  __syncthreads();
  const float inv = 1.f/bc[1];
  for (int i = threadIdx.x; i < cols; i += 256) yr[i] = expf(xr[i] - m)*inv;
}

// Depthwise FIR resampling by 2 (Resample.forward): down = conv2d(stride 2, padding (ph, pw));
// up = conv_transpose2d(stride 2, padding, output_padding) with the kernel times `gain`.
__global__ __launch_bounds__(256) void fir_down_kernel(const float* x, const float* k, float* y,
                                                       long long planes, int H, int W, int Ho,
                                                       int Wo, int K, int ph, int pw) {
  // grid (column blocks, output rows, planes): the index arithmetic is per workgroup
  const int wo = blockIdx.x*256 + threadIdx.x, ho = blockIdx.y;
  const long long pl = blockIdx.z;
  if (wo >= Wo) return;
  const long long idx = (pl*Ho + ho)*(long long)Wo + wo;
  {
    const float* xp = x + pl*H*W;
    float acc = 0.f;
    for (int i = 0; i < K; ++i) {
      const int hi = ho*2 - ph + i;
      if (hi < 0 || hi >= H) continue;
      for (int j = 0; j < K; ++j) {
        const int wi = wo*2 - pw + j;
        if (wi < 0 || wi >= W) continue;
        acc += xp[(long long)hi*W + wi]*k[i*K + j];
      }
    }
    y[idx] = acc;
  }
}
__global__ __launch_bounds__(256) void fir_up_kernel(const float* x, const float* k, float* y,
                                                     long long planes, int H, int W, int Ho, int Wo,
                                                     int K, int ph, int pw, float gain) {
  // grid (column blocks, output rows, planes): the index arithmetic is per workgroup
  const int wo = blockIdx.x*256 + threadIdx.x, ho = blockIdx.y;
  const long long pl = blockIdx.z;
  if (wo >= Wo) return;
  const long long idx = (pl*Ho + ho)*(long long)Wo + wo;
  {
    const float* xp = x + pl*H*W;
    float acc = 0.f;
    for (int i = 0; i < K; ++i) {
      const int hn = ho + ph - i;
      if (hn < 0 || (hn & 1)) continue;
      const int hi = hn >> 1;
      if (hi >= H) continue;
      for (int j = 0; j < K; ++j) {
        const int wn = wo + pw - j;
        if (wn < 0 || (wn & 1)) continue;
        const int wi = wn >> 1;
        if (wi >= W) continue;
        acc += xp[(long long)hi*W + wi]*k[i*K + j];
      }
    }
    y[idx] = gain*acc;
  }
}

// out = alpha*a + beta*b  (b nullable)
__global__ __launch_bounds__(256) void axpby_kernel(const float* a, float alpha, const float* b,
                                                    float beta, float* out, long long n) {
  GRID_STRIDE(i, n) out[i] = alpha*a[i] + (b ? beta*b[i] : 0.f);
}

// out[i] = [sin(2 pi x_i b_j) | cos(2 pi x_i b_j)]   (GaussianFourierProjection)
__global__ __launch_bounds__(256) void fourier_kernel(const float* x, const float* b, float* out,
                                                      int n, int m) {
  GRID_STRIDE(idx, (long long)n*m) {
    const int i = (int)(idx / m), j = (int)(idx % m);
    const float v = 6.283185307179586f*(x[i]*b[j]);      // rounding order of 2*pi*outer(x, b)
    out[(long long)i*2*m + j] = sinf(v);
    out[(long long)i*2*m + m + j] = cosf(v);
  }
}

}  // namespace

extern "C" {

int64_t brv_groupnorm_scratch_bytes(int64_t B, int64_t groups) {
  return B*groups*kGnLine*(int64_t)sizeof(double);
}
int brv_groupnorm_fold(const float* x, const float* add_bc, const float* gamma, const float* beta,
                       const float* adm_scale, const float* adm_shift, void* scratch, float* scale,
                       float* shift, float* mu_bc, float* rstd_bc, int64_t B, int64_t C, int64_t HW,
                       int64_t groups, float eps, brv_stream_t stream) {
  BRV_REFUSE(B < 1 || C < 1 || HW < 1 || groups < 1 || C % groups,
             "requires B >= 1, C >= 1, HW >= 1, groups >= 1, C a multiple of groups");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (C/groups)*HW;
  long long nsplit = (n + 16383)/16384;
  if (nsplit > 64) nsplit = 64;
  const long long slice = ((n + nsplit - 1)/nsplit + 3) & ~3LL;
  hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)(B*groups), (unsigned)nsplit), dim3(256), 0,
                     st, x, add_bc, (double*)scratch, (int)C, (long long)HW, (int)groups, slice);
  hipLaunchKernelGGL(gn_fold_kernel, dim3((unsigned)(B*groups)), dim3(64), 0, st,
                     (double*)scratch, add_bc, gamma, beta, adm_scale, adm_shift, scale, shift,
                     mu_bc, rstd_bc, (int)C, (long long)HW, (int)groups, eps);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
int brv_affine_act(const float* x, const float* scale_bc, const float* shift_bc, float* y,
                   int64_t B, int64_t C, int64_t HW, int act_silu, brv_stream_t stream) {
  BRV_REFUSE(B < 1 || C < 1 || HW < 1, "requires B >= 1, C >= 1, HW >= 1");
  const long long total = B*C*HW;
  hipLaunchKernelGGL(affine_act_kernel, flat_grid(total/4 + 1), dim3(256), 0, (hipStream_t)stream,
                     x, scale_bc, shift_bc, y, (long long)HW, total, act_silu);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
int brv_groupnorm_backward(const float* x, const float* dy, const float* scale_bc,
                           const float* shift_bc, const float* mu_bc, const float* rstd_bc,
                           const float* gamma, float* dx, float* s1_bc, float* s2_bc, float* dadd_bc,
                           float* coef_scratch, int64_t B, int64_t C, int64_t HW, int64_t groups,
                           int act_silu, brv_stream_t stream) {
  BRV_REFUSE(B < 1 || C < 1 || HW < 1 || groups < 1 || C % groups || C/groups > 64,
             "requires B >= 1, C >= 1, HW >= 1, groups >= 1, C a multiple of groups, C/groups <= 64");
  hipStream_t st = (hipStream_t)stream;
  long long slices = (HW + 16383)/16384;
  if (slices > 32) slices = 32;
  double* part = nullptr;
  BRV_HIP_OK(hipMallocAsync((void**)&part, (size_t)B*C*slices*3*sizeof(double), st));
  hipLaunchKernelGGL(gn_bwd_sums_kernel, dim3((unsigned)(B*C), (unsigned)slices), dim3(256), 0, st, x,
                     dy, scale_bc, shift_bc, mu_bc, rstd_bc, part, (long long)HW, act_silu);
  float* k1 = coef_scratch; float* k2 = k1 + B*C; float* k3 = k2 + B*C;
  hipLaunchKernelGGL(gn_bwd_coef_kernel, dim3((unsigned)(B*groups)), dim3(64), 0, st, part,
                     (int)slices, gamma, rstd_bc, k1, k2, k3, s1_bc, s2_bc, dadd_bc, (int)C,
                     (long long)HW, (int)groups);
  BRV_HIP_OK(hipFreeAsync(part, st));
  const long long total = B*C*HW;
  hipLaunchKernelGGL(gn_bwd_apply_kernel, flat_grid(total), dim3(256), 0, st, x, dy, scale_bc,
                     shift_bc, mu_bc, rstd_bc, k1, k2, k3, dx, (long long)HW, total, act_silu);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
// backward of y = act(scale[b][c]*x + shift[b][c]) (brv_affine_act): dx = scale*u, d scale =
// sum_hw u*x, d shift = sum_hw u with u = dy*act'(pre): the group-norm sums kernel with a
// unit "normalisation" (mu = 0, rstd = 1) and its apply kernel with k1 = scale, k2 = k3 = 0
int brv_affine_act_backward(const float* x, const float* dy, const float* scale_bc,
                            const float* shift_bc, const float* zeros_bc, const float* ones_bc,
                            float* dx, float* dscale_bc, float* dshift_bc, int64_t B, int64_t C,
                            int64_t HW, int act_silu, brv_stream_t stream) {
  BRV_REFUSE(B < 1 || C < 1 || HW < 1, "requires B >= 1, C >= 1, HW >= 1");
  hipStream_t st = (hipStream_t)stream;
  long long slices = (HW + 16383)/16384;
  if (slices > 32) slices = 32;
  double* part = nullptr;
  BRV_HIP_OK(hipMallocAsync((void**)&part, (size_t)B*C*slices*3*sizeof(double), st));
  hipLaunchKernelGGL(gn_bwd_sums_kernel, dim3((unsigned)(B*C), (unsigned)slices), dim3(256), 0, st, x,
                     dy, scale_bc, shift_bc, zeros_bc, ones_bc, part, (long long)HW, act_silu);
  hipLaunchKernelGGL(affine_bwd_final_kernel, dim3((unsigned)((B*C + 255)/256)), dim3(256), 0, st,
                     part, (int)slices, dshift_bc, dscale_bc, (int)(B*C));
  BRV_HIP_OK(hipFreeAsync(part, st));
  const long long total = B*C*HW;
  hipLaunchKernelGGL(gn_bwd_apply_kernel, flat_grid(total), dim3(256), 0, st, x, dy, scale_bc,
                     shift_bc, zeros_bc, ones_bc, scale_bc, zeros_bc, zeros_bc, dx, (long long)HW,
                     total, act_silu);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
int brv_silu_backward(const float* x, const float* dy, float* dx, int64_t n, brv_stream_t stream) {
  BRV_REFUSE(n < 1, "requires n >= 1");
  hipLaunchKernelGGL(silu_bwd_kernel, flat_grid(n), dim3(256), 0, (hipStream_t)stream, x, dy, dx,
                     (long long)n);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
int brv_softmax_rows_backward(const float* p, const float* dy, float* dx, int64_t rows, int64_t cols,
                              brv_stream_t stream) {
  BRV_REFUSE(rows < 1 || cols < 1, "requires rows >= 1, cols >= 1");
  hipLaunchKernelGGL(softmax_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p,
                     dy, dx, (int)cols);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
int brv_silu(const float* x, float* y, int64_t n, brv_stream_t stream) {
  BRV_REFUSE(n < 1, "requires n >= 1");
  hipLaunchKernelGGL(silu_kernel, flat_grid(n), dim3(256), 0, (hipStream_t)stream, x, y, (long long)n);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
int brv_softmax_rows(const float* x, float* y, int64_t rows, int64_t cols, brv_stream_t stream) {
  BRV_REFUSE(rows < 1 || cols < 1, "requires rows >= 1, cols >= 1");
  hipLaunchKernelGGL(softmax_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, y,
                     (int)cols);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
int brv_fir_resample2d(const float* x, const float* kernel, float* y, int64_t planes, int64_t H,
                       int64_t W, int64_t Ho, int64_t Wo, int64_t K, int64_t pad_h, int64_t pad_w,
                       int up, float gain, brv_stream_t stream) {
  BRV_REFUSE(planes < 1 || Ho < 1 || Wo < 1 || Ho > 65535, "requires planes >= 1, Ho >= 1, Wo >= 1, Ho <= 65535");
  // grid.z carries the planes: at most 65 535 per launch
  for (int64_t p0 = 0; p0 < planes; p0 += 65535) {
    const int64_t np = planes - p0 < 65535 ? planes - p0 : 65535;
    const dim3 grid((unsigned)((Wo + 255)/256), (unsigned)Ho, (unsigned)np);
    const float* xs = x + p0*H*W;
    float* ys = y + p0*Ho*Wo;
    if (up)
      hipLaunchKernelGGL(fir_up_kernel, grid, dim3(256), 0, (hipStream_t)stream, xs, kernel, ys,
                         (long long)np, (int)H, (int)W, (int)Ho, (int)Wo, (int)K, (int)pad_h,
                         (int)pad_w, gain);
    else
      hipLaunchKernelGGL(fir_down_kernel, grid, dim3(256), 0, (hipStream_t)stream, xs, kernel, ys,
                         (long long)np, (int)H, (int)W, (int)Ho, (int)Wo, (int)K, (int)pad_h,
                         (int)pad_w);
  }
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
int brv_axpby(const float* a, float alpha, const float* b, float beta, float* out, int64_t n,
              brv_stream_t stream) {
  BRV_REFUSE(n < 1, "requires n >= 1");
  hipLaunchKernelGGL(axpby_kernel, flat_grid(n), dim3(256), 0, (hipStream_t)stream, a, alpha, b,
                     beta, out, (long long)n);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}
int brv_fourier_features(const float* x, const float* b, float* out, int64_t n, int64_t m,
                         brv_stream_t stream) {
  BRV_REFUSE(n < 1 || m < 1, "requires n >= 1, m >= 1");
  hipLaunchKernelGGL(fourier_kernel, flat_grid(n*m), dim3(256), 0, (hipStream_t)stream, x, b, out,
                     (int)n, (int)m);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
