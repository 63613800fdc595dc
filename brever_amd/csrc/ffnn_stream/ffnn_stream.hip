// Stateful streaming inference of the FFNN mask estimator (include/brever_ffnn_stream.h).
// Reference: brever/models/ffnn/ffnn.py:72-203 (_enhance, stack, the normalisers, _FFNN) and
// brever/modules/features.py:142-205 (fbe); the offline kernels these restate are in ../ffnn.hip and
// ../stft.hip (istft_ola_kernel). The two DFTs of a call are the main library's, called by the host.
//
// Columns of a call = (stream, frame) pairs, column s*hops + j. A stream's values depend on its own slot
// and its own rows of the inputs only, and every sum runs in an order fixed by the geometry, so its output
// bits do not depend on which other streams share the call. State is read by every kernel but written by
// commit_kernel alone, the last launch of a step, from the workspace.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../../include/brever_ffnn_stream.h"
#include "../common.cuh"
#include "../status.h"

using namespace brv;

namespace {

constexpr int kMaxFft = 4096, kMaxMel = 256, kMaxChannels = 8, kMaxStacks = 64;

// what the kernels index with; derived from brv_ffs_config on the host (geometry())
struct Geo {
  int n, hop, lag, C, bins, mel, stacks, kinds, NF, R, norm, d;
  int feat_norm[BRV_FFS_MAX_FEATURES], feat_comp[BRV_FFS_MAX_FEATURES];
  float eps_feat, eps_norm;
  long long off_stats, off_carry, off_hist, off_tail, state_bytes;   // bytes into a slot
};

inline long long up256(long long x) { return (x + 255)/256*256; }

// workspace of a call: byte offsets
struct Ws {
  long long stats, feat, act0, act1, tail, total;
  int ld;                                   // floats per column of an activation buffer
};

Geo geometry(const brv_ffs_config& c) {
  Geo g{};
  g.n = c.n_fft; g.hop = c.hop; g.lag = c.n_fft - c.hop; g.C = c.channels; g.bins = c.n_fft/2 + 1;
  g.mel = c.mel; g.stacks = c.stacks; g.kinds = c.features; g.NF = c.features*c.mel;
  g.R = (c.stacks + 1)*g.NF; g.norm = c.norm; g.d = c.n_fft/(2*c.hop) - 1;
  for (int i = 0; i < BRV_FFS_MAX_FEATURES; ++i) { g.feat_norm[i] = c.feat_norm[i]; g.feat_comp[i] = c.feat_comp[i]; }
  g.eps_feat = c.eps_feat; g.eps_norm = c.eps_norm;
  g.off_stats = 16;
  g.off_carry = g.off_stats + (c.norm == 1 ? 16LL*g.R : 0);
  g.off_hist = g.off_carry + 4LL*g.C*g.lag;
  g.off_tail = g.off_hist + 4LL*g.stacks*g.NF;
  g.state_bytes = up256(g.off_tail + 4LL*g.lag);
  return g;
}

Ws ws_layout(const brv_ffs_config& c, const Geo& g, long long n, long long hops) {
  Ws w{};
  int widest = g.R;
  for (int l = 0; l <= c.hidden; ++l) widest = c.widths[l] > widest ? c.widths[l] : widest;
  w.ld = round_up(widest, 32);
  const long long cols = n*hops;
  w.stats = 0;
  w.feat = w.stats + up256(g.norm == 1 ? 16LL*n*g.R : 0);
  w.act0 = w.feat + up256(4LL*cols*g.NF);
  w.act1 = w.act0 + up256(4LL*cols*w.ld);
  w.tail = w.act1 + up256(4LL*cols*w.ld);
  w.total = w.tail + up256(4LL*n*g.lag);
  return w;
}

// -2 with the reason for a model the kernels do not take
int check_config(const brv_ffs_config* c) {
  BRV_UNSUPPORTED(c->n_fft != c->frame_length || !c->center || !c->pad_constant || !c->normalized || !c->onesided ||
                  c->compression != 1.f || c->scale != 1.f,
                  "needs the STFT FFNN builds: n_fft == frame_length, centred, constant padding, normalised, "
                  "one-sided, compression 1, scale 1");
  BRV_UNSUPPORTED(c->hop < 1 || c->n_fft < 2 || c->n_fft % (2*c->hop) != 0,
                  "needs frame_length % (2 hop) == 0 (the centre padding in whole hops)");
  BRV_UNSUPPORTED(c->hidden < 0 || c->hidden > BRV_FFS_MAX_HIDDEN, "takes at most 8 hidden layers");
  BRV_UNSUPPORTED(c->n_fft > kMaxFft || c->mel < 1 || c->mel > kMaxMel || c->channels < 1 || c->channels > kMaxChannels ||
                  c->stacks < 0 || c->stacks > kMaxStacks,
                  "limits: n_fft <= 4096, 1 <= mel <= 256, 1 <= channels <= 8, 0 <= stacks <= 64");
  BRV_UNSUPPORTED(c->features < 1 || c->features > BRV_FFS_MAX_FEATURES, "needs 1 to 6 features of the fbe family");
  for (int i = 0; i < c->features; ++i)
    BRV_UNSUPPORTED(c->feat_norm[i] < 0 || c->feat_norm[i] > 1 || c->feat_comp[i] < 0 || c->feat_comp[i] > 2,
                    "feature kinds: normalise 0 / 1, compression 0 none, 1 log, 2 cubic");
  BRV_UNSUPPORTED(c->norm < 0 || c->norm > 1, "normaliser: 0 static, 1 cumulative");
  for (int l = 0; l <= c->hidden; ++l)
    BRV_UNSUPPORTED(c->widths[l] < 1 || c->widths[l] > (1 << 20), "layer widths must be in [1, 2^20]");
  BRV_UNSUPPORTED(c->widths[c->hidden] != c->mel, "the last layer must have mel outputs");
  return 0;
}

// ---- device helpers -------------------------------------------------------------------------------------------
__device__ __forceinline__ const char* slot_ptr(const void* state, const Geo& g, int id) {
  return static_cast<const char*>(state) + (long long)id*g.state_bytes;
}
// STFT frame of column j of a stream that has received H hops; false where the offline transform has no such
// frame: before frame 0, and in a tail (rest >= 0) behind the last frame of the right-padded signal
__device__ __forceinline__ bool frame_of(const Geo& g, long long H, int j, long long rest, long long* t) {
  *t = H + j - g.d;
  if (*t < 0) return false;
  if (rest >= 0) {
    const long long L = H*g.hop + rest;
    const long long over = L > g.n ? L - g.n : 0;
    const long long last = (over + g.hop - 1)/g.hop + g.n/g.hop;       // = padded length / hop
    if (*t > last) return false;
  }
  return true;
}

// ---- reset ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reset_kernel(void* state, const int* ids, int slots, long long words) {
  const int id = ids[blockIdx.x];
  if (id < 0 || id >= slots) return;
  uint32_t* p = reinterpret_cast<uint32_t*>(static_cast<char*>(state) + (long long)id*words*4);
  for (long long i = threadIdx.x; i < words; i += 256) p[i] = 0u;
}

// ---- front: carry | chunk per (stream, channel) ---------------------------------------------------------------
// xin (n C, lag + hops hop); x (n, C, hops hop), or in a tail (n, C, rest) followed by zeros
__global__ __launch_bounds__(256) void frames_kernel(const Geo g, const void* state, const int* ids, int slots,
                                                     const float* x, int hops, long long rest, float* xin) {
  const int row = blockIdx.x, s = row / g.C, c = row % g.C;
  const int id = ids[s];
  if (id < 0 || id >= slots) return;
  const float* carry = reinterpret_cast<const float*>(slot_ptr(state, g, id) + g.off_carry) + (long long)c*g.lag;
  const long long len = (long long)g.lag + (long long)hops*g.hop;
  const long long have = rest >= 0 ? rest : (long long)hops*g.hop;
  float* out = xin + (long long)row*len;
  for (long long i = (long long)blockIdx.y*256 + threadIdx.x; i < len; i += (long long)gridDim.y*256) {
    float v = 0.f;
    if (i < g.lag) v = carry[i];
    else if (i - g.lag < have) v = x[(long long)row*have + (i - g.lag)];
    out[i] = v;
  }
}

// ---- features of one column: channel-mean power, mel, pdf normalisation, compression ---------------------------
// (fbe_power_kernel, the mel product, col_normalize_kernel and compress_kernel of ../ffnn.hip, per frame)
__global__ __launch_bounds__(256) void feat_kernel(const Geo g, const void* state, const int* ids, int slots,
                                                   int hops, long long rest, const float2* spec,
                                                   const float* mel_fwd, float* feat) {
  __shared__ float P[kMaxFft/2 + 1];
  __shared__ float E[kMaxMel];
  __shared__ float inv_sum;
  const int col = blockIdx.x, s = col / hops, j = col % hops;
  const int id = ids[s];
  if (id < 0 || id >= slots) return;
  const long long H = *reinterpret_cast<const long long*>(slot_ptr(state, g, id));
  long long t;
  if (!frame_of(g, H, j, rest, &t)) return;
  for (int b = threadIdx.x; b < g.bins; b += 256) {
    float p = 0.f;
    for (int c = 0; c < g.C; ++c) {
      const float2 v = spec[(((long long)s*g.C + c)*g.bins + b)*hops + j];
      p += v.x*v.x + v.y*v.y;
    }
    P[b] = p/(float)g.C;
  }
  __syncthreads();
  const int f = threadIdx.x;
  if (f < g.mel) {
    const float* w = mel_fwd + (long long)f*g.bins;
    float e = 0.f;
    for (int b = 0; b < g.bins; ++b) e = fmaf(w[b], P[b], e);
    E[f] = e;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.f;
    for (int m = 0; m < g.mel; ++m) sum += E[m];
    inv_sum = 1.f/(sum + g.eps_feat);
  }
  __syncthreads();
  if (f < g.mel) {
    float* out = feat + (long long)col*g.NF;
    for (int q = 0; q < g.kinds; ++q) {
      float v = E[f];
      if (g.feat_norm[q]) v *= inv_sum;
      if (g.feat_comp[q] == 1) v = logf(v + g.eps_feat);
      else if (g.feat_comp[q] == 2) v = cbrtf(v);
      out[q*g.mel + f] = v;
    }
  }
}

// ---- stacking from the history + the normaliser ---------------------------------------------------------------
// One thread per (stream, stacked row) walks the frames of the call in order (stack_kernel, static_norm_kernel
// and cumulative_norm_kernel of ../ffnn.hip). Feature frame ts of a stream is column ts - (H - d) of this call
// or, from before it, ring entry ts % stacks of the slot; rows older than frame 0 repeat frame 0.
__global__ __launch_bounds__(256) void stack_norm_kernel(const Geo g, const void* state, const int* ids, int slots,
                                                         int n, int hops, long long rest, const float* feat,
                                                         const float* mean, const float* stdv, float* act, int ld,
                                                         double* new_stats) {
  const long long idx = (long long)blockIdx.x*256 + threadIdx.x;
  if (idx >= (long long)n*g.R) return;
  const int s = (int)(idx / g.R), row = (int)(idx % g.R);
  const int id = ids[s];
  if (id < 0 || id >= slots) return;
  const char* slot = slot_ptr(state, g, id);
  const long long H = *reinterpret_cast<const long long*>(slot);
  const float* hist = reinterpret_cast<const float*>(slot + g.off_hist);
  const int kk = row / g.NF, f = row % g.NF;
  double sum = 0.0, sq = 0.0;
  float mu = 0.f, sd = 1.f;
  if (g.norm == 1) {
    const double* st = reinterpret_cast<const double*>(slot + g.off_stats);
    sum = st[row]; sq = st[g.R + row];
  } else {
    mu = mean[row]; sd = stdv[row];
  }
  const long long first = H - g.d;                    // frame of column 0 (may be negative)
  const long long lo = first < 0 ? 0 : first;         // first feature frame this call computes
  for (int j = 0; j < hops; ++j) {
    float* out = act + ((long long)s*hops + j)*ld + row;
    long long t;
    if (!frame_of(g, H, j, rest, &t)) { *out = 0.f; continue; }
    const long long ts = t - kk < 0 ? 0 : t - kk;
    // (ts < lo only where lo > 0, and then lo - stacks <= ts: the ring holds it)
    const float v = ts >= lo ? feat[((long long)s*hops + (ts - first))*g.NF + f] : hist[(ts % g.stacks)*g.NF + f];
    if (g.norm == 1) {
      const double vd = (double)v;
      sum += vd; sq += vd*vd;
      const double cnt = (double)(t + 1);
      const double m = sum/cnt;
      const double var = fmax(sq/cnt - m*m, 0.0);
      *out = (float)((vd - m)/sqrt(var + (double)g.eps_norm));
    } else {
      *out = (v - mu)/sd;
    }
  }
  if (g.norm == 1) {
    new_stats[(long long)s*2*g.R + row] = sum;
    new_stats[(long long)s*2*g.R + g.R + row] = sq;
  }
}

// ---- the MLP: a weight-streaming product for few columns ------------------------------------------------------
// Y (cols, M) = act(W (M, K) X (cols, K)^T + bias) on v_mfma_f32_16x16x4_f32: exact fp32 operands, every output
// element accumulated in ONE lane's register over k in an order fixed by K alone (no split over k, no
// cross-lane sum), so a column's bits do not depend on the other columns. One wave per 16 weight rows: it
// reads its 16 x K strip once, 128 contiguous bytes per row and iteration (lane (r, g) holds k = kb + 8 g ..
// + 7 of row r), and multiplies it into CT column tiles of 16. Lane maps of the instruction: A[i = l & 15]
// [k = l >> 4], B[k = l >> 4][j = l & 15], D register v = row 4 (l >> 4) + v, column l & 15.
__device__ __forceinline__ void load8v(const float* p, float (&v)[8]) {               // 32 aligned bytes
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void load8g(const float* p, int k0, int K, float (&v)[8]) {  // zeros from K on
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = k0 + i;
    const float x = p[k < K ? k : K - 1];
    v[i] = k < K ? x : 0.f;
  }
}

template <int CT>
__global__ __launch_bounds__(64) void mlp_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                                 const float* __restrict__ X, float* __restrict__ Y, int M, int K,
                                                 int cols, int ld, int act, int wvec) {
  const int lane = threadIdx.x, r = lane & 15, grp = lane >> 4;
  const int m0 = blockIdx.x*16, c0 = blockIdx.y*16*CT;
  const int wr = m0 + r < M ? m0 + r : M - 1;          // rows and columns past the edge: a valid copy, not stored
  const float* wrow = W + (long long)wr*K;
  const float* xcol[CT];
  f32x4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int c = c0 + ct*16 + r;
    xcol[ct] = X + (long long)(c < cols ? c : cols - 1)*ld;
    acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // whole blocks of 32 k through 16-byte loads where the weight rows allow them, the rest (and the k edge)
  // element by element: the same values in the same lanes either way
  // (four blocks' loads are issued before their products, so a wave keeps 512 bytes per weight row in flight)
  const int kvec = wvec ? K/32*32 : 0;
  int kb = 0;
  for (; kb + 128 <= kvec; kb += 128) {
    float a[4][8], b[CT][4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) load8v(wrow + kb + 32*u + 8*grp, a[u]);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int u = 0; u < 4; ++u) load8v(xcol[ct] + kb + 32*u + 8*grp, b[ct][u]);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int i = 0; i < 8; ++i)
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i], b[ct][u][i], acc[ct], 0, 0, 0);
  }
  for (; kb < kvec; kb += 32) {
    const int k0 = kb + 8*grp;
    float a[8];
    load8v(wrow + k0, a);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float b[8];
      load8v(xcol[ct] + k0, b);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], acc[ct], 0, 0, 0);
    }
  }
  for (; kb < K; kb += 32) {
    const int k0 = kb + 8*grp;
    float a[8];
    load8g(wrow, k0, K, a);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float b[8];
      load8g(xcol[ct], k0, K, b);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], acc[ct], 0, 0, 0);
    }
  }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int c = c0 + ct*16 + r;
    if (c >= cols) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = m0 + 4*grp + v;
      if (m >= M) continue;
      float y = acc[ct][v] + bias[m];
      y = act == 0 ? (y > 0.f ? y : 0.f) : 1.f/(1.f + expf(-y));
      Y[(long long)c*ld + m] = y;
    }
  }
}

// ---- back: mel-to-bin extrapolation, mask x channel-mean spectrum ----------------------------------------------
// (MelFilterbank.backward and masked_mean_spec_kernel of ../ffnn.hip); a frame that does not exist gets zeros
__global__ __launch_bounds__(256) void mask_kernel(const Geo g, const void* state, const int* ids, int slots,
                                                   int hops, long long rest, const float2* spec, const float* mask,
                                                   int ld, const float* mel_inv, float2* mspec) {
  __shared__ float Mk[kMaxMel];
  const int col = blockIdx.x, s = col / hops, j = col % hops;
  const int id = ids[s];
  if (id < 0 || id >= slots) return;
  const long long H = *reinterpret_cast<const long long*>(slot_ptr(state, g, id));
  long long t;
  const bool live = frame_of(g, H, j, rest, &t);
  if (threadIdx.x < g.mel) Mk[threadIdx.x] = mask[(long long)col*ld + threadIdx.x];
  __syncthreads();
  for (int b = threadIdx.x; b < g.bins; b += 256) {
    float2 o = make_float2(0.f, 0.f);
    if (live) {
      const float* w = mel_inv + (long long)b*g.mel;
      float e = 0.f;
      for (int f = 0; f < g.mel; ++f) e = fmaf(w[f], Mk[f], e);
      float re = 0.f, im = 0.f;
      for (int c = 0; c < g.C; ++c) {
        const float2 v = spec[(((long long)s*g.C + c)*g.bins + b)*hops + j];
        re += v.x; im += v.y;
      }
      const float m = e/(float)g.C;
      o = make_float2(re*m, im*m);
    }
    mspec[((long long)s*g.bins + b)*hops + j] = o;
  }
}

// ---- overlap-add, envelope, output ------------------------------------------------------------------------------
// Position i of a stream's span is sample p = H hop - lag + i: the slot's tail (i < lag) plus this call's frames,
// frames ascending as istft_ola_kernel adds them. A step returns the first hops hop positions and leaves the
// last lag ones as the new tail; a tail returns lag + rest. The envelope counts the frames that exist offline.
__global__ __launch_bounds__(256) void emit_kernel(const Geo g, const void* state, const int* ids, int slots,
                                                   int hops, long long rest, const float* frames, const float* win,
                                                   float* y, float* new_tail) {
  const int s = blockIdx.y;
  const int id = ids[s];
  if (id < 0 || id >= slots) return;
  const char* slot = slot_ptr(state, g, id);
  const long long H = *reinterpret_cast<const long long*>(slot);
  const float* tail = reinterpret_cast<const float*>(slot + g.off_tail);
  const long long span = (long long)g.lag + (long long)hops*g.hop;
  const long long outs = rest >= 0 ? g.lag + rest : (long long)hops*g.hop;
  long long last = 0;                                  // last frame of the offline transform (tail only)
  if (rest >= 0) {
    const long long L = H*g.hop + rest, over = L > g.n ? L - g.n : 0;
    last = (over + g.hop - 1)/g.hop + g.n/g.hop;
  }
  for (long long i = (long long)blockIdx.x*256 + threadIdx.x; i < span; i += (long long)gridDim.x*256) {
    if (rest >= 0 && i >= outs) continue;
    float sum = i < g.lag ? tail[i] : 0.f;
    long long j_hi = i/g.hop; if (j_hi > hops - 1) j_hi = hops - 1;
    long long j_lo = i - g.n + 1 <= 0 ? 0 : (i - g.n + g.hop)/g.hop;
    for (long long j = j_lo; j <= j_hi; ++j) {
      const long long m = i - j*g.hop;
      long long t;
      if (m < 0 || m >= g.n || !frame_of(g, H, (int)j, rest, &t)) continue;
      sum += frames[((long long)s*hops + j)*g.n + m];
    }
    if (i < outs) {
      const long long p = H*g.hop - g.lag + i;
      float v = 0.f;
      if (p >= 0) {
        const long long pos = p + g.n/2;
        long long t_hi = pos/g.hop; if (rest >= 0 && t_hi > last) t_hi = last;
        long long t_lo = (pos - g.n + g.hop)/g.hop; if (pos - g.n + 1 <= 0) t_lo = 0;
        if (t_lo < 0) t_lo = 0;
        float env = 0.f;
        for (long long t = t_lo; t <= t_hi; ++t) {
          const long long m = pos - t*g.hop;
          if (m < 0 || m >= g.n) continue;
          const float w = win[m];
          env += w*w;
        }
        v = sum/env;
      }
      y[(long long)s*outs + i] = v;
    } else {
      new_tail[(long long)s*g.lag + (i - outs)] = sum;
    }
  }
}

// ---- the state commit: the only writes to a slot ----------------------------------------------------------------
__global__ __launch_bounds__(256) void commit_kernel(const Geo g, void* state, const int* ids, int slots, int hops,
                                                     const float* xin, const float* feat, const float* new_tail,
                                                     const double* new_stats) {
  const int s = blockIdx.x;
  const int id = ids[s];
  if (id < 0 || id >= slots) return;
  char* slot = static_cast<char*>(state) + (long long)id*g.state_bytes;
  long long* hdr = reinterpret_cast<long long*>(slot);
  const long long H = hdr[0];
  __syncthreads();                                     // every thread holds H before thread 0 overwrites it
  const long long len = (long long)g.lag + (long long)hops*g.hop;
  float* carry = reinterpret_cast<float*>(slot + g.off_carry);
  for (int i = threadIdx.x; i < g.C*g.lag; i += 256) {
    const int c = i / g.lag, k = i % g.lag;
    carry[i] = xin[((long long)s*g.C + c)*len + (long long)hops*g.hop + k];
  }
  float* tail = reinterpret_cast<float*>(slot + g.off_tail);
  for (int i = threadIdx.x; i < g.lag; i += 256) tail[i] = new_tail[(long long)s*g.lag + i];
  if (g.norm == 1) {
    double* st = reinterpret_cast<double*>(slot + g.off_stats);
    for (int i = threadIdx.x; i < 2*g.R; i += 256) st[i] = new_stats[(long long)s*2*g.R + i];
  }
  const long long first = H - g.d;
  const long long t1 = first + hops < 0 ? 0 : first + hops;          // feature frames after this call
  long long t0 = first < 0 ? 0 : first;
  if (t0 < t1 - g.stacks) t0 = t1 - g.stacks;
  float* hist = reinterpret_cast<float*>(slot + g.off_hist);
  for (long long i = threadIdx.x; i < (t1 - t0)*g.NF; i += 256) {
    const long long t = t0 + i / g.NF;
    const int f = (int)(i % g.NF);
    hist[(t % g.stacks)*g.NF + f] = feat[((long long)s*hops + (t - first))*g.NF + f];
  }
  if (threadIdx.x == 0) { hdr[0] = H + hops; hdr[1] = t1; }
}

int launch_mlp(const float* W, const float* bias, const float* X, float* Y, int M, int K, long long cols, int ld,
               int act, hipStream_t st) {
  const int wvec = (K % 4 == 0) && (reinterpret_cast<uintptr_t>(W) % 16 == 0);
  const int ct = cols <= 16 ? 1 : cols <= 32 ? 2 : 4;
  const dim3 grid((unsigned)((M + 15)/16), (unsigned)((cols + 16*ct - 1)/(16*ct)));
  if (ct == 1) hipLaunchKernelGGL(mlp_kernel<1>, grid, dim3(64), 0, st, W, bias, X, Y, M, K, (int)cols, ld, act, wvec);
  else if (ct == 2) hipLaunchKernelGGL(mlp_kernel<2>, grid, dim3(64), 0, st, W, bias, X, Y, M, K, (int)cols, ld, act, wvec);
  else hipLaunchKernelGGL(mlp_kernel<4>, grid, dim3(64), 0, st, W, bias, X, Y, M, K, (int)cols, ld, act, wvec);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

// the arguments every launch group shares
int check_call(const brv_ffs_config* cfg, int64_t slots, int64_t n, int64_t hops, int64_t rest) {
  BRV_REFUSE(slots < 1 || n < 1 || n > slots || hops < 1, "requires slots >= 1, 1 <= n <= slots, hops >= 1");
  if (int e = check_config(cfg)) return e;
  BRV_REFUSE(rest >= cfg->hop, "requires rest < hop (process the whole hops first)");
  BRV_REFUSE(rest >= 0 && hops != cfg->n_fft/cfg->hop, "a tail requires hops == n_fft / hop");
  BRV_REFUSE(n*hops > 65535*16 || n*(int64_t)cfg->channels > 65535 || hops*(int64_t)cfg->hop > (1LL << 30),
             "requires n hops <= 1048560 columns, n channels <= 65535, hops hop <= 2^30");
  return 0;
}

}  // namespace

extern "C" {

int64_t brv_ffs_state_bytes(const brv_ffs_config* cfg) {
  BRV_REFUSE(!cfg, "null argument: cfg");
  if (int e = check_config(cfg)) return e;
  return geometry(*cfg).state_bytes;
}

int64_t brv_ffs_workspace_bytes(const brv_ffs_config* cfg, int64_t n, int64_t hops) {
  BRV_REFUSE(!cfg, "null argument: cfg");
  BRV_REFUSE(n < 1 || hops < 1, "requires n >= 1, hops >= 1");
  if (int e = check_config(cfg)) return e;
  return ws_layout(*cfg, geometry(*cfg), n, hops).total;
}

int brv_ffs_reset(const brv_ffs_config* cfg, void* state, int64_t slots, const int32_t* ids, int64_t n,
                  brv_stream_t stream) {
  BRV_REFUSE(!cfg || !state || !ids, "null argument: cfg, state and ids are required");
  BRV_REFUSE(slots < 1 || n < 1 || n > slots, "requires slots >= 1, 1 <= n <= slots");
  if (int e = check_config(cfg)) return e;
  const Geo g = geometry(*cfg);
  hipLaunchKernelGGL(reset_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, state, ids, (int)slots,
                     g.state_bytes/4);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_ffs_step_frames(const brv_ffs_config* cfg, const void* state, int64_t slots, const int32_t* ids,
                        int64_t n, const float* x, int64_t hops, int64_t rest, float* xin, brv_stream_t stream) {
  BRV_REFUSE(!cfg || !state || !ids || !xin || (!x && rest != 0),
             "null argument: cfg, state, ids, xin and (unless rest == 0) x are required");
  if (int e = check_call(cfg, slots, n, hops, rest)) return e;
  const Geo g = geometry(*cfg);
  const long long len = (long long)g.lag + hops*g.hop;
  long long gy = (len + 255)/256; if (gy > 64) gy = 64;
  hipLaunchKernelGGL(frames_kernel, dim3((unsigned)(n*g.C), (unsigned)gy), dim3(256), 0, (hipStream_t)stream, g,
                     state, ids, (int)slots, x, (int)hops, (long long)rest, xin);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_ffs_step_net(const brv_ffs_config* cfg, const void* state, int64_t slots, const int32_t* ids, int64_t n,
                     int64_t hops, int64_t rest, const float* spec, float* mspec, void* workspace,
                     int64_t workspace_bytes, brv_stream_t stream) {
  BRV_REFUSE(!cfg || !state || !ids || !spec || !mspec || !workspace,
             "null argument: cfg, state, ids, spec, mspec and workspace are required");
  if (int e = check_call(cfg, slots, n, hops, rest)) return e;
  const Geo g = geometry(*cfg);
  const Ws w = ws_layout(*cfg, g, n, hops);
  BRV_REFUSE(workspace_bytes < w.total, "requires workspace_bytes >= brv_ffs_workspace_bytes(cfg, n, hops)");
  BRV_REFUSE(!cfg->mel_fwd || !cfg->mel_inv || (cfg->norm == 0 && (!cfg->mean || !cfg->std)),
             "null argument: cfg needs mel_fwd, mel_inv and, for the static normaliser, mean and std");
  for (int l = 0; l <= cfg->hidden; ++l)
    BRV_REFUSE(!cfg->weight[l] || !cfg->bias[l], "null argument: cfg needs the weight and bias of every layer");
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  float* feat = reinterpret_cast<float*>(ws + w.feat);
  float* act[2] = {reinterpret_cast<float*>(ws + w.act0), reinterpret_cast<float*>(ws + w.act1)};
  const long long cols = n*hops;
  hipLaunchKernelGGL(feat_kernel, dim3((unsigned)cols), dim3(256), 0, st, g, state, ids, (int)slots, (int)hops,
                     (long long)rest, (const float2*)spec, cfg->mel_fwd, feat);
  hipLaunchKernelGGL(stack_norm_kernel, dim3((unsigned)((n*g.R + 255)/256)), dim3(256), 0, st, g, state, ids,
                     (int)slots, (int)n, (int)hops, (long long)rest, (const float*)feat, cfg->mean, cfg->std, act[0],
                     w.ld, reinterpret_cast<double*>(ws + w.stats));
  BRV_HIP_OK(hipGetLastError());
  int K = g.R, cur = 0;
  for (int l = 0; l <= cfg->hidden; ++l) {
    if (int e = launch_mlp(cfg->weight[l], cfg->bias[l], act[cur], act[cur ^ 1], cfg->widths[l], K, cols, w.ld,
                           l < cfg->hidden ? 0 : 1, st))
      return e;
    K = cfg->widths[l];
    cur ^= 1;
  }
  hipLaunchKernelGGL(mask_kernel, dim3((unsigned)cols), dim3(256), 0, st, g, state, ids, (int)slots, (int)hops,
                     (long long)rest, (const float2*)spec, (const float*)act[cur], w.ld, cfg->mel_inv, (float2*)mspec);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_ffs_step_emit(const brv_ffs_config* cfg, const float* window, void* state, int64_t slots,
                      const int32_t* ids, int64_t n, int64_t hops, int64_t rest, const float* xin,
                      const float* frames, float* y, void* workspace, int64_t workspace_bytes,
                      brv_stream_t stream) {
  BRV_REFUSE(!cfg || !window || !state || !ids || !xin || !frames || !y || !workspace,
             "null argument: cfg, window, state, ids, xin, frames, y and workspace are required");
  if (int e = check_call(cfg, slots, n, hops, rest)) return e;
  const Geo g = geometry(*cfg);
  const Ws w = ws_layout(*cfg, g, n, hops);
  BRV_REFUSE(workspace_bytes < w.total, "requires workspace_bytes >= brv_ffs_workspace_bytes(cfg, n, hops)");
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  float* new_tail = reinterpret_cast<float*>(ws + w.tail);
  const long long span = (long long)g.lag + hops*g.hop;
  long long gx = (span + 255)/256; if (gx > 256) gx = 256;
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, st, g, (const void*)state, ids,
                     (int)slots, (int)hops, (long long)rest, frames, window, y, new_tail);
  if (rest < 0)
    hipLaunchKernelGGL(commit_kernel, dim3((unsigned)n), dim3(256), 0, st, g, state, ids, (int)slots, (int)hops, xin,
                       (const float*)(ws + w.feat), (const float*)new_tail, (const double*)(ws + w.stats));
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"

// the library's last-error message and its two status exports (../status.h)
BRV_DEFINE_STATUS(brv_ffs_version, brv_ffs_last_error)
