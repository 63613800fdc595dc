// Stateful streaming inference of the causal Conv-TasNet (C ABI brv_ctn_stream_*).
//
// One call advances n streams, each held in its own state slot in HBM, by F hops of hop = K/2 input
// samples. Frame t of a stream covers input samples [hop t, hop t + K) (convtasnet.py:115-126: the
// offline encoder pads at the end only), so it exists once hop (t + 2) samples have arrived; output
// samples [hop t, hop (t + 1)) are final once frames t - 1 and t are, and a stream's output lags its
// input by exactly one hop. Per slot the state holds:
//   * the number of hops received (the frame count of every cumulative layer norm follows from it);
//   * (sum x, sum x^2) in fp64 of each of the 1 + 2 layers repeats cumulative layer norms;
//   * the last hop of input samples (the first half of the next frame);
//   * one hop of overlap-add tail per source (the second half of the last decoded frame);
//   * per TCN block, a ring of the last (P - 1) d frames of its cLN_1 output (hidden width,
//     slot = absolute frame mod (P - 1) d): the left context of the dilated depthwise tap.
// A call runs 5 + 3 layers repeats launches: encoder (+ frame sums of the input norm), input norm +
// bottleneck, per block {1x1 product + PReLU_1 frame sums; depthwise tap + PReLU_2 frame sums;
// cLN_2 + [res | skip] product + residual / skip add + ring update}, output product + sigmoid + mask,
// decoder, overlap-add + state commit. Every state read happens before every state write of the same
// quantity (the commit kernel, or a later launch), so no launch synchronises across workgroups.
// Columns are the (stream, frame) pairs of a call; every column's arithmetic is a function of that
// stream's data only (each product element is one MFMA lane's dot product with a fixed k order, each
// frame sum a fixed reduction tree over the rows), so a stream's output is bitwise the same whatever
// other streams share the call.
// Precision: products on v_mfma_f32_16x16x4_f32 (exact fp32 operands, amp = 0) or on
// v_mfma_f32_16x16x32_bf16 with the operands rounded to bf16 (amp = 1); accumulation, activations,
// state and the depthwise tap in fp32, norm statistics in fp64.
#include <hip/hip_runtime.h>
#include <string.h>
#include <string>

#include "../../include/brever_hip.h"
#include "common.cuh"
#include "status.h"
#include "ctn_layout.h"

using namespace brv;

namespace {

__host__ __device__ inline long long upS(long long x, long long a) { return (x + a - 1)/a*a; }

constexpr int kMaxP = 8;           // depthwise taps
constexpr int kMaxKp = 960;        // reduction length of a product (the B tile lives in LDS: < 64 KiB)
constexpr int kTileM = 64;         // rows per workgroup: 4 waves x 16
constexpr int kTileC = 16;         // columns per workgroup of a product
constexpr int kDwCols = 4;         // columns per workgroup of the depthwise kernel
constexpr float kEps = 1e-8f;      // cumulative layer norm (modules/normalization.py)

struct BlkS : CtnBlockOff { long long ring; int dil, R; };

// parameter offsets (ctn_layout.h) + this path's limits and the state layout
struct LayS : CtnLayout<BlkS> {
  int norms, gmax;
  long long st_stats, st_carry, st_tail, st_ring, st_bytes;     // bytes
  static int limits(const brv_ctn_config* c) {
    if (int r = ctn_kernel_size_positive(c)) return r;
    if (!c->causal) return fail(-3, "streaming needs a causal Conv-TasNet (the global layer norm is not streamable)");
    if (c->kernel_size > kMaxP) return fail(-2, "streaming: kernel_size must be <= 8");
    if (c->layers*c->repeats > 64 || c->layers > 24) return fail(-2, "streaming: at most 64 blocks, 24 layers");
    if (c->filter_length % 2) return fail(-2, "streaming: filter_length must be even (hop = filter_length/2)");
    const int widest = c->filters > c->hidden_channels ? c->filters : c->hidden_channels;
    if (upS(widest, 32) > kMaxKp || upS(c->bottleneck_channels, 32) > kMaxKp || upS(c->skip_channels, 32) > kMaxKp ||
        upS(c->filter_length, 32) > kMaxKp)
      return fail(-2, "streaming: channel counts must be <= 960");
    return 0;
  }
  int init(const brv_ctn_config* c) {
    if (int r = CtnLayout::init(c, limits)) return r;
    norms = 1 + 2*nb;
    gmax = ((N > H ? N : H) + kTileM - 1)/kTileM;
    long long ring_frames = 0;
    for (int i = 0; i < nb; ++i) {
      BlkS& b = blk[i];
      b.dil = 1 << (i % layers);
      b.R = (P - 1)*b.dil;
      b.ring = ring_frames;
      ring_frames += b.R;
    }
    // state slot: [int64 hops, int64 reserved][fp64 stats (norms x 2)][carry hop][tail S x hop][rings]
    st_stats = 16;
    st_carry = st_stats + 16LL*norms;
    st_tail = st_carry + upS(4LL*hop, 16);
    st_ring = st_tail + upS(4LL*S*hop, 16);
    st_bytes = upS(st_ring + 4LL*H*ring_frames, 256);
    return 0;
  }
};

// workspace of one call (floats)
struct WsS {
  long long w, x, z1, z2, skip, fsum, y, fr, total;
  void init(const LayS& l, long long C) {
    long long o = 0;
    auto take = [&](long long n) { long long r = o; o += upS(n, 64); return r; };
    w = take(C*l.N); x = take(C*l.Bn); z1 = take(C*l.H); z2 = take(C*l.H); skip = take(C*l.Sc);
    fsum = take((long long)l.norms*C*l.gmax*2);
    y = take(C*l.S*l.N); fr = take(C*l.S*l.K);
    total = o;
  }
};

// everything a kernel of one call needs
struct Call {
  const int32_t* ids; unsigned char* state; long long st_bytes;
  int F, hop; long long C;              // columns = n F
  const float* xin; float* yout;
  float* fsum; int gmax;                // [norm][col][g][2]
  long long st_stats, st_carry, st_tail, st_ring;
};

__device__ __forceinline__ unsigned char* slot_of(const Call& c, long long col) {
  return c.state + (long long)c.ids[col / c.F]*c.st_bytes;
}
// absolute frame index of a column (< 0: the first hop of a stream, no frame yet)
__device__ __forceinline__ long long frame_of(const Call& c, long long col) {
  const long long hops = *(const long long*)slot_of(c, col);
  return hops - 1 + col % c.F;
}

// mean / rstd of cumulative norm `norm` at column `col` over `ch` channels: carried sums + this call's
// frame sums of the stream's columns <= col (fixed order: frame, then row group)
__device__ void col_stats(const Call& c, int norm, int ngroups, long long col, int ch, float& mean, float& rstd) {
  const unsigned char* sl = slot_of(c, col);
  const long long t = *(const long long*)sl - 1 + col % c.F;
  if (t < 0) { mean = 0.f; rstd = 1.f; return; }
  const double* st = (const double*)(sl + c.st_stats) + 2*norm;
  double s1 = st[0], s2 = st[1];
  const long long first = col - col % c.F;
  for (long long q = first; q <= col; ++q) {
    const float* fs = c.fsum + ((long long)norm*c.C + q)*c.gmax*2;
    for (int g = 0; g < ngroups; ++g) { s1 += fs[2*g]; s2 += fs[2*g + 1]; }
  }
  const double n = (double)ch*(double)(t + 1);
  const double m = s1/n, var = s2/n - m*m;
  mean = (float)m; rstd = (float)(1.0/sqrt(var + (double)kEps));
}

// ---- products: D[m][col] = sum_k A[m][k] B[k][col], one 64 x 16 tile per workgroup ----------------
enum Mode { ENC = 0, BOTT = 1, PW1 = 2, RESSKIP = 3, OUTM = 4, DEC = 5 };

struct Gemm {
  Call c;
  int M, K;                       // rows, reduction length
  long long cols;                 // columns of this product (DEC: C S)
  const float* A; long long lda_m, lda_k;       // A[m][k] = A[m lda_m + k lda_k]
  const float* A2; int m_split;   // RESSKIP: rows >= m_split from A2 (row-major, K wide)
  const float* bias; const float* bias2;
  const float* src; int lds;      // B operand source rows
  const float* slope;             // PReLU of the B operand (RESSKIP: prelu2, OUTM: tcn prelu) / of the output (PW1)
  const float* gain; const float* nbias;   // norm applied to the B operand (BOTT, RESSKIP)
  int norm_in, groups_in;         // its index / row groups
  float* dst; int ldd;            // output rows
  float* dst2; int ldd2;          // RESSKIP: skip
  int first;                      // RESSKIP: first block (skip = product instead of skip + product)
  int norm_out, groups_out;       // frame sums of the output (ENC, PW1): index, < 0 = none
  const float* wenc;              // OUTM: encoder output w; DEC: -
  int S, N;                       // OUTM: sources, filters
  // RESSKIP ring update: h1 = cLN_1(prelu_1(z1)) of the last min(F, R) frames -> ring
  const float* z1; const float* slope1; const float* g1; const float* b1; int norm1, groups1, H, R; long long ring;
  int ring_tiles;                 // extra workgroups (grid.y beyond the product tiles)
};

template <int MODE>
__device__ __forceinline__ float load_b(const Gemm& g, long long col, int k, float mean, float rstd) {
  const Call& c = g.c;
  if (MODE == ENC) {
    // sample hop t + k of the stream; t = hops - 1 + f, relative to the call's first new sample
    const long long f = col % c.F;
    const long long r = (long long)c.hop*(f - 1) + k;
    if (frame_of(c, col) < 0) return 0.f;
    if (r < 0) return ((const float*)(slot_of(c, col) + c.st_carry))[c.hop + r];
    return c.xin[(col / c.F)*(long long)c.F*c.hop + r];
  }
  const float v = g.src[col*g.lds + k];
  if (MODE == BOTT) return (v - mean)*rstd*g.gain[k] + g.nbias[k];
  if (MODE == RESSKIP) return (prelu(v, *g.slope) - mean)*rstd*g.gain[k] + g.nbias[k];
  if (MODE == OUTM) return prelu(v, *g.slope);
  return v;     // PW1, DEC
}

__device__ __forceinline__ float load_a(const Gemm& g, int m, int k) {
  if (m >= g.M || k >= g.K) return 0.f;
  if (g.A2 && m >= g.m_split) return g.A2[(long long)(m - g.m_split)*g.K + k];
  return g.A[(long long)m*g.lda_m + (long long)k*g.lda_k];
}

template <int MODE, int AMP>
__global__ __launch_bounds__(256) void stream_gemm_kernel(const Gemm g) {
  extern __shared__ float bt[];                 // [kTileC][ldb]: the B tile, pre-op applied
  __shared__ float st_mean[kTileC], st_rstd[kTileC];
  __shared__ float red[4][kTileC][2];
  const Call& c = g.c;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntiles = (int)((g.cols + kTileC - 1)/kTileC);
  if (MODE == RESSKIP && (int)blockIdx.y >= ntiles) {
    // ring update of this block: columns = (stream, one of its last min(F, R) frames)
    const int keep = c.F < g.R ? c.F : g.R;
    const long long nstreams = c.C / c.F;
    const long long per = ((long long)gridDim.x*g.ring_tiles);
    const long long wgi = (long long)(blockIdx.y - ntiles)*gridDim.x + blockIdx.x;
    for (long long pi = wgi; pi < nstreams*keep; pi += per) {
      const long long col = (pi / keep)*c.F + (c.F - keep) + pi % keep;
      const long long t = frame_of(c, col);
      __syncthreads();
      if (tid == 0) col_stats(c, g.norm1, g.groups1, col, g.H, st_mean[0], st_rstd[0]);
      __syncthreads();
      if (t < 0) continue;
      const float mean = st_mean[0], rstd = st_rstd[0], a = *g.slope1;
      float* ring = (float*)(slot_of(c, col) + c.st_ring) + (g.ring + t % g.R)*g.H;
      for (int ch = tid; ch < g.H; ch += 256)
        ring[ch] = (prelu(g.z1[col*g.H + ch], a) - mean)*rstd*g.g1[ch] + g.b1[ch];
    }
    return;
  }
  const long long c0 = (long long)blockIdx.y*kTileC;
  const int m0 = blockIdx.x*kTileM;
  const int Kp = AMP ? (int)upS(g.K, 32) : (int)upS(g.K, 4);
  const int ldb = Kp + 4;
  if ((MODE == BOTT || MODE == RESSKIP) && tid < kTileC) {
    float m = 0.f, r = 1.f;
    if (c0 + tid < g.cols) col_stats(c, g.norm_in, g.groups_in, c0 + tid, g.K, m, r);
    st_mean[tid] = m; st_rstd[tid] = r;
  }
  __syncthreads();
  for (int i = tid; i < kTileC*Kp; i += 256) {
    const int j = i / Kp, k = i % Kp;
    float v = 0.f;
    if (c0 + j < g.cols && k < g.K) v = load_b<MODE>(g, c0 + j, k, st_mean[j], st_rstd[j]);
    bt[j*ldb + k] = AMP ? rbf(v) : v;
  }
  __syncthreads();
  const int row = m0 + wave*16 + (lane & 15);      // A row of this lane
  const int j = lane & 15, h = lane >> 4;          // B column of this lane, k group
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (m0 + wave*16 < g.M) {
    if (AMP) {
      for (int k0 = 0; k0 < Kp; k0 += 32) {
        float av[8], bv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { av[e] = load_a(g, row, k0 + 8*h + e); bv[e] = bt[j*ldb + k0 + 8*h + e]; }
        bf16x8 a8, b8;
#pragma unroll
        for (int e = 0; e < 8; ++e) { a8[e] = (__bf16)av[e]; b8[e] = (__bf16)bv[e]; }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a8, b8, acc, 0, 0, 0);
      }
    } else {
      // 16 k per round: lane group h holds k0 + 4h + s in the s-th MFMA (a fixed permutation of k)
      for (int k0 = 0; k0 < Kp; k0 += 16) {
        float av[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) av[s] = load_a(g, row, k0 + 4*h + s);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = k0 + 4*h + s;
          const float b = k < Kp ? bt[j*ldb + k] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k < Kp ? av[s] : 0.f, b, acc, 0, 0, 0);
        }
      }
    }
  }
  // epilogue: lane holds D[m0 + 16 wave + 4 h + v][c0 + j]
  const long long col = c0 + j;
  const bool colok = col < g.cols;
  const bool valid = colok && (MODE == DEC || frame_of(c, col) >= 0);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int m = m0 + wave*16 + 4*h + v;
    if (!colok || m >= g.M) continue;
    float val = acc[v];
    if (MODE == ENC) {
      g.dst[col*g.ldd + m] = val;
      s1 += val; s2 = __builtin_fmaf(val, val, s2);
    } else if (MODE == BOTT) {
      g.dst[col*g.ldd + m] = val + g.bias[m];
    } else if (MODE == PW1) {
      val += g.bias[m];
      g.dst[col*g.ldd + m] = val;
      const float p = prelu(val, *g.slope);
      s1 += p; s2 = __builtin_fmaf(p, p, s2);
    } else if (MODE == RESSKIP) {
      if (m < g.m_split) {
        float* d = g.dst + col*g.ldd + m;
        *d = *d + (val + g.bias[m]);
      } else {
        float* d = g.dst2 + col*g.ldd2 + (m - g.m_split);
        const float y = val + g.bias2[m - g.m_split];
        *d = g.first ? y : *d + y;
      }
    } else if (MODE == OUTM) {
      const float pre = val + g.bias[m];
      const float mk = 1.f/(1.f + __expf(-pre));
      const int s = m / g.N, n = m % g.N;
      g.dst[(col*g.S + s)*g.N + n] = mk*g.wenc[col*g.N + n];
    } else {   // DEC
      g.dst[col*g.ldd + m] = val;
    }
  }
  if (MODE == ENC || MODE == PW1) {
    s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
    s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
    if (h == 0) { red[wave][j][0] = s1; red[wave][j][1] = s2; }
    __syncthreads();
    if (tid < kTileC && c0 + tid < g.cols) {
      const long long cc = c0 + tid;
      const bool ok = frame_of(c, cc) >= 0;
      float a = 0.f, b = 0.f;
      for (int w = 0; w < 4; ++w) { a += red[w][tid][0]; b += red[w][tid][1]; }
      float* fs = c.fsum + (((long long)g.norm_out*c.C + cc)*c.gmax + blockIdx.x)*2;
      fs[0] = ok ? a : 0.f; fs[1] = ok ? b : 0.f;
    }
  }
  (void)valid;
}

// ---- depthwise dilated tap: z2 = dconv(h1), h1 = cLN_1(prelu_1(z1)) of this call or of the ring ----
struct Dw {
  Call c;
  const float* z1; float* z2; const float* taps; const float* bias;
  const float* slope1; const float* g1; const float* b1; const float* slope2;
  int H, P, dil, R, norm1, norm2, groups1; long long ring;
};

__global__ __launch_bounds__(256) void stream_dw_kernel(const Dw d) {
  const Call& c = d.c;
  __shared__ float sm[kDwCols][kMaxP], sr[kDwCols][kMaxP];
  __shared__ float red[kDwCols][2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long c0 = (long long)blockIdx.x*kDwCols;
  if (tid < kDwCols*d.P) {
    const int j = tid / d.P, k = tid % d.P;
    const long long col = c0 + j;
    float m = 0.f, r = 1.f;
    if (col < c.C) {
      const long long f = col % c.F - (long long)(d.P - 1 - k)*d.dil;    // chunk column of tap k
      if (f >= 0) col_stats(c, d.norm1, d.groups1, col - (col % c.F) + f, d.H, m, r);
    }
    sm[j][k] = m; sr[j][k] = r;
  }
  __syncthreads();
  const float a1 = *d.slope1, a2 = *d.slope2;
  for (int j = 0; j < kDwCols; ++j) {
    const long long col = c0 + j;
    float s1 = 0.f, s2 = 0.f;
    if (col < c.C) {
      const long long t = frame_of(c, col);
      const long long f = col % c.F;
      const float* ring = (const float*)(slot_of(c, col) + c.st_ring) + d.ring*d.H;
      for (int ch = tid; ch < d.H; ch += 256) {
        float acc = d.bias[ch];
        for (int k = 0; k < d.P; ++k) {
          const long long back = (long long)(d.P - 1 - k)*d.dil;
          const long long ti = t - back;
          if (ti < 0) continue;
          float hv;
          if (f - back >= 0)
            hv = (prelu(d.z1[(col - back)*d.H + ch], a1) - sm[j][k])*sr[j][k]*d.g1[ch] + d.b1[ch];
          else
            hv = ring[(ti % d.R)*d.H + ch];
          acc = __builtin_fmaf(d.taps[ch*d.P + k], hv, acc);
        }
        d.z2[col*d.H + ch] = acc;
        const float p = prelu(acc, a2);
        s1 += p; s2 = __builtin_fmaf(p, p, s2);
      }
      if (t < 0) { s1 = 0.f; s2 = 0.f; }
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    if (lane == 0) { red[j][0][wave] = s1; red[j][1][wave] = s2; }
  }
  __syncthreads();
  if (tid < kDwCols && c0 + tid < c.C) {
    float* fs = c.fsum + ((long long)d.norm2*c.C + c0 + tid)*c.gmax*2;
    fs[0] = red[tid][0][0] + red[tid][0][1] + red[tid][0][2] + red[tid][0][3];
    fs[1] = red[tid][1][0] + red[tid][1][1] + red[tid][1][2] + red[tid][1][3];
  }
}

// ---- overlap-add of the decoded frames, output, state commit: one workgroup per stream ----------
struct Commit {
  Call c; const float* fr; int S, K, norms, g_enc, g_h;   // row groups of the frame sums: input norm, cLN_1 (cLN_2: 1)
};

__global__ __launch_bounds__(256) void stream_commit_kernel(const Commit k) {
  const Call& c = k.c;
  const long long s = blockIdx.x;
  const long long col0 = s*c.F;
  unsigned char* sl = c.state + (long long)c.ids[s]*c.st_bytes;
  const long long hops = *(const long long*)sl;
  float* tail = (float*)(sl + c.st_tail);
  float* carry = (float*)(sl + c.st_carry);
  const int hop = c.hop, F = c.F, S = k.S, K = k.K;
  // y[s][src][f hop + i] = first half of frame t + second half of frame t - 1 (this call or the tail)
  for (long long i = threadIdx.x; i < (long long)S*F*hop; i += 256) {
    const int src = (int)(i / ((long long)F*hop));
    const long long r = i % ((long long)F*hop);
    const int f = (int)(r / hop), q = (int)(r % hop);
    const long long t = hops - 1 + f;
    float v = 0.f;
    if (t >= 0) {
      v = k.fr[((col0 + f)*S + src)*K + q];
      if (f == 0) v += tail[src*hop + q];
      else if (t - 1 >= 0) v += k.fr[((col0 + f - 1)*S + src)*K + hop + q];
    }
    c.yout[(s*S + src)*(long long)F*hop + r] = v;
  }
  __syncthreads();                       // every read of the old tail / hop count is done
  const bool last_ok = hops - 1 + (F - 1) >= 0;
  for (int i = threadIdx.x; i < S*hop; i += 256) {
    const int src = i / hop, q = i % hop;
    if (last_ok) tail[i] = k.fr[((col0 + F - 1)*S + src)*K + hop + q];
  }
  for (int i = threadIdx.x; i < hop; i += 256) carry[i] = c.xin[s*(long long)F*hop + (long long)(F - 1)*hop + i];
  double* st = (double*)(sl + c.st_stats);
  for (int nrm = threadIdx.x; nrm < k.norms; nrm += 256) {
    double s1 = st[2*nrm], s2 = st[2*nrm + 1];
    for (int f = 0; f < F; ++f) {
      const float* fs = c.fsum + ((long long)nrm*c.C + col0 + f)*c.gmax*2;
      const int groups = nrm == 0 ? k.g_enc : (nrm % 2 ? k.g_h : 1);
      for (int g = 0; g < groups; ++g) { s1 += fs[2*g]; s2 += fs[2*g + 1]; }
    }
    st[2*nrm] = s1; st[2*nrm + 1] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) *(long long*)sl = hops + F;
}

// restart the listed slots: hop count, statistics, carry and tail to zero (the rings are only read at
// frames >= 0 that the stream has written since)
__global__ __launch_bounds__(256) void stream_reset_kernel(unsigned char* state, long long st_bytes, const int32_t* ids,
                                                           long long zero_bytes) {
  unsigned int* p = (unsigned int*)(state + (long long)ids[blockIdx.x]*st_bytes);
  for (long long i = threadIdx.x; i < zero_bytes/4; i += 256) p[i] = 0u;
}

// OLA tail of the listed slots -> y (n, S, hop): the output still owed when the input ends on a hop boundary
__global__ __launch_bounds__(256) void stream_tail_kernel(const unsigned char* state, long long st_bytes,
                                                          const int32_t* ids, long long st_tail, int n_tail,
                                                          float* y) {
  const float* tail = (const float*)(state + (long long)ids[blockIdx.x]*st_bytes + st_tail);
  for (int i = threadIdx.x; i < n_tail; i += 256) y[(long long)blockIdx.x*n_tail + i] = tail[i];
}

template <int MODE>
int launch_gemm(const Gemm& g, int amp, hipStream_t st) {
  const int Kp = amp ? (int)upS(g.K, 32) : (int)upS(g.K, 4);
  const size_t lds = (size_t)kTileC*(Kp + 4)*sizeof(float);
  const unsigned ntiles = (unsigned)((g.cols + kTileC - 1)/kTileC);
  dim3 grid((g.M + kTileM - 1)/kTileM, ntiles + (MODE == RESSKIP ? g.ring_tiles : 0));
  if ((long long)ntiles + g.ring_tiles > 65535) return fail(-2, "streaming: too many columns in one call");
  if (amp) hipLaunchKernelGGL((stream_gemm_kernel<MODE, 1>), grid, dim3(256), lds, st, g);
  else hipLaunchKernelGGL((stream_gemm_kernel<MODE, 0>), grid, dim3(256), lds, st, g);
  return 0;
}

}  // namespace

extern "C" {

int64_t brv_ctn_stream_state_bytes(const brv_ctn_config* cfg) {
  LayS l; if (int r = l.init(cfg)) return r;
  return l.st_bytes;
}

int64_t brv_ctn_stream_workspace_bytes(const brv_ctn_config* cfg, int64_t n, int64_t hops, int32_t amp) {
  (void)amp;     // both precisions keep fp32 activations between the launches
  LayS l; if (int r = l.init(cfg)) return r;
  if (n < 1 || hops < 1) return fail(-1, "streaming: n and hops must be >= 1");
  WsS ws; ws.init(l, n*hops);
  return ws.total*4;
}

int brv_ctn_stream_reset(const brv_ctn_config* cfg, void* state, const int32_t* ids, int64_t n,
                         brv_stream_t stream) {
  LayS l; if (int r = l.init(cfg)) return r;
  if (n < 1) return 0;
  hipLaunchKernelGGL(stream_reset_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     (unsigned char*)state, l.st_bytes, ids, l.st_ring);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_ctn_stream_tail(const brv_ctn_config* cfg, const void* state, const int32_t* ids, int64_t n,
                        float* y, brv_stream_t stream) {
  LayS l; if (int r = l.init(cfg)) return r;
  if (n < 1) return 0;
  hipLaunchKernelGGL(stream_tail_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)state, l.st_bytes, ids, l.st_tail, l.S*l.hop, y);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_ctn_stream_step(const brv_ctn_config* cfg, const float* params, void* state, const int32_t* ids,
                        int64_t n, const float* x, int64_t hops, float* y, int32_t amp, void* workspace,
                        int64_t workspace_bytes, const brv_launch_opts* opts, brv_stream_t stream) {
  (void)opts;    // no option of this entry point yet (size / flags reserved)
  LayS l; if (int r = l.init(cfg)) return r;
  if (n < 1 || hops < 1) return fail(-1, "streaming: n and hops must be >= 1");
  const long long C = n*hops;
  WsS ws; ws.init(l, C);
  if (workspace_bytes < ws.total*4) return fail(-1, "streaming: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* W = (float*)workspace;
  // row groups of each norm's frame sums: input norm = encoder rows, cLN_1 = H rows, cLN_2 = 1 (depthwise)
  const int g_enc = (l.N + kTileM - 1)/kTileM, g_h = (l.H + kTileM - 1)/kTileM;
  Call c{ids, (unsigned char*)state, l.st_bytes, (int)hops, l.hop, C, x, y, W + ws.fsum, l.gmax,
         l.st_stats, l.st_carry, l.st_tail, l.st_ring};
  auto base = [&]() { Gemm g; memset(&g, 0, sizeof(g)); g.c = c; g.cols = C; g.lda_k = 1; g.norm_out = -1; return g; };
  // encoder: w = enc_w * frame, frame sums of the input norm
  {
    Gemm g = base();
    g.M = l.N; g.K = l.K; g.A = params + l.enc_w; g.lda_m = l.K;
    g.dst = W + ws.w; g.ldd = l.N; g.norm_out = 0;
    if (int r = launch_gemm<ENC>(g, amp, st)) return r;
  }
  // input norm + bottleneck
  {
    Gemm g = base();
    g.M = l.Bn; g.K = l.N; g.A = params + l.bott_w; g.lda_m = l.N; g.bias = params + l.bott_b;
    g.src = W + ws.w; g.lds = l.N; g.gain = params + l.ln_g; g.nbias = params + l.ln_b;
    g.norm_in = 0; g.groups_in = g_enc;
    g.dst = W + ws.x; g.ldd = l.Bn;
    if (int r = launch_gemm<BOTT>(g, amp, st)) return r;
  }
  for (int i = 0; i < l.nb; ++i) {
    const BlkS& b = l.blk[i];
    const bool has_res = i < l.nb - 1;
    {
      Gemm g = base();
      g.M = l.H; g.K = l.Bn; g.A = params + b.conv_w; g.lda_m = l.Bn; g.bias = params + b.conv_b;
      g.src = W + ws.x; g.lds = l.Bn; g.slope = params + b.prelu1;
      g.dst = W + ws.z1; g.ldd = l.H; g.norm_out = 1 + 2*i;
      if (int r = launch_gemm<PW1>(g, amp, st)) return r;
    }
    {
      Dw d{c, W + ws.z1, W + ws.z2, params + b.dconv_w, params + b.dconv_b, params + b.prelu1, params + b.n1_g,
           params + b.n1_b, params + b.prelu2, l.H, l.P, b.dil, b.R > 0 ? b.R : 1, 1 + 2*i, 2 + 2*i, g_h, b.ring};
      hipLaunchKernelGGL(stream_dw_kernel, dim3((unsigned)((C + kDwCols - 1)/kDwCols)), dim3(256), 0, st, d);
    }
    {
      Gemm g = base();
      const int mres = has_res ? l.Bn : 0;
      g.M = mres + l.Sc; g.K = l.H; g.lda_m = l.H;
      g.A = has_res ? params + b.res_w : params + b.skip_w;
      g.A2 = has_res ? params + b.skip_w : nullptr; g.m_split = mres;
      g.bias = has_res ? params + b.res_b : nullptr; g.bias2 = params + b.skip_b;
      g.src = W + ws.z2; g.lds = l.H; g.slope = params + b.prelu2; g.gain = params + b.n2_g; g.nbias = params + b.n2_b;
      g.norm_in = 2 + 2*i; g.groups_in = 1;
      g.dst = W + ws.x; g.ldd = l.Bn; g.dst2 = W + ws.skip; g.ldd2 = l.Sc; g.first = i == 0;
      g.z1 = W + ws.z1; g.slope1 = params + b.prelu1; g.g1 = params + b.n1_g; g.b1 = params + b.n1_b;
      g.norm1 = 1 + 2*i; g.groups1 = g_h; g.H = l.H; g.R = b.R; g.ring = b.ring;
      if (b.R > 0) {
        const long long pairs = n*(hops < b.R ? hops : b.R);
        const long long gx = (g.M + kTileM - 1)/kTileM;
        long long tiles = (pairs + 4*gx - 1)/(4*gx);              // ~4 frames per workgroup
        g.ring_tiles = (int)(tiles < 1 ? 1 : tiles);
      }
      if (int r = launch_gemm<RESSKIP>(g, amp, st)) return r;
    }
  }
  // PReLU + output product + sigmoid mask x w
  {
    Gemm g = base();
    g.M = l.S*l.N; g.K = l.Sc; g.A = params + l.out_w; g.lda_m = l.Sc; g.bias = params + l.out_b;
    g.src = W + ws.skip; g.lds = l.Sc; g.slope = params + l.tcn_prelu;
    g.dst = W + ws.y; g.wenc = W + ws.w; g.S = l.S; g.N = l.N;
    if (int r = launch_gemm<OUTM>(g, amp, st)) return r;
  }
  // decoder: fr[(col, src)][k] = sum_n y[(col, src)][n] dec_w[n][k]
  {
    Gemm g = base();
    g.cols = C*l.S; g.M = l.K; g.K = l.N; g.A = params + l.dec_w; g.lda_m = 1; g.lda_k = l.K;
    g.src = W + ws.y; g.lds = l.N; g.dst = W + ws.fr; g.ldd = l.K;
    if (int r = launch_gemm<DEC>(g, amp, st)) return r;
  }
  {
    Commit k{c, W + ws.fr, l.S, l.K, l.norms, g_enc, g_h};
    hipLaunchKernelGGL(stream_commit_kernel, dim3((unsigned)n), dim3(256), 0, st, k);
  }
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
