// Stateful streaming inference of DCCRN in eval mode (C ABI brv_dccrn_stream_*).
//
// One call advances n streams, each held in its own state slot in HBM, by F hops of `hop` input
// samples. With P = n_fft / (2 hop), G = kt - 1 and D = levels G, input hop r completes STFT frame
// tau = r - P + 1 (frame t covers samples [hop t - n_fft/2, hop t + n_fft/2), left edge zero-padded).
// At that column encoder level e emits its frame tau - e G, the recurrent block its frame tau - D,
// every decoder its frame tau - D, and the mask of frame tau - D is applied to the spectrum of that
// frame; the inverse DFT of that frame completes output hop tau - D - P, so a stream's output lags its
// input by (2P - 1 + D) hops = latency - hop.
//
// Level buffers: 0 = spectrum, e = encoder level e, L + 1 = recurrent block output, L + 1 + k =
// decoder k. A column reads frame v of buffer b from this call's workspace if it was computed in this
// call, else from the slot's ring of buffer b (slot v mod ring). Ring lengths are what the readers
// reach back: the spectrum D frames (mask), encoder e (L + 1 - e) G (next encoder level, and the skip
// input of decoder L + 1 - e, which trails it by (L - e) G frames plus its own G taps), the recurrent
// output and decoders 1 .. L - 1 G frames (the next decoder's taps).
//
// The end of a stream (brv_dccrn_stream_tail) is the same launch sequence with a finite frame count T
// (STFT.pad + centre padding): frame v of a buffer exists iff 0 <= v < T - lim(b), so the STFT frames
// of the zero-padded end are computed, the encoders and the recurrent block stop at their last frame,
// and the decoders' trailing G frames per level see their missing inputs as absent (bias, norm and
// PReLU still applied). No zero frame goes through the encoder.
//
// Launches per call: DFT; one per encoder level; per LSTM layer an input projection of all frames and
// four chains and a recurrence that walks the frames from the (h, c) in the slot; the two Linear maps;
// one per decoder level; mask; inverse DFT; overlap-add + output + state commit. Every state quantity
// is read before the launch that writes it (the commit kernel, or the recurrence for its own (h, c)),
// so no launch synchronises across workgroups. Every output element is one lane's fixed-order sum over
// the data of its own stream: a stream's output is bitwise the same whatever streams share the call.
// Precision: products with fp32 operands (amp = 0) or operands rounded to bf16 (amp = 1), fp32 fused
// multiply-add accumulation; DFT and inverse DFT accumulate in fp64 on the fp64 tables of the offline
// STFT; mask, gate math, norms, state in fp32.
#include <hip/hip_runtime.h>
#include <string.h>
#include <string>

#include "../../include/brever_hip.h"
#include "common.cuh"
#include "status.h"

using namespace brv;

namespace {

constexpr int kMaxL = BRV_DCCRN_STREAM_MAX_LEVELS;
constexpr int kNB = 2*kMaxL + 2;       // level buffers
constexpr int kMaxN = 4096;            // n_fft
constexpr int kMaxH = 512;             // LSTM width
constexpr int kMaxC = 1024;            // channels of a level
constexpr long long kNever = 1LL << 60;
constexpr int kHdr = 16;               // slot header: int64 hops received, int64 reserved

__host__ __device__ inline long long upD(long long x, long long a) { return (x + a - 1)/a*a; }

struct Geo {
  int n, hop, P, L, G, D, lagh, kf, kt, sf, pf, Fq0, bins, cbn, lh, ll, feat, nbuf;
  int C[kMaxL + 1], H[kMaxL + 1];
  int elems[kNB], off[kNB], lim[kNB], ring[kNB];
  long long st_ring[kNB];                 // floats from the end of the slot header
  long long st_hist, st_tail, st_lstm, st_floats, st_bytes;
  int init(const brv_dccrn_stream_config* c) {
    if (!c) return fail(-1, "null config");
    n = c->n_fft; hop = c->hop; L = c->levels; kf = c->kf; kt = c->kt; sf = c->sf; pf = c->pf;
    cbn = c->complex_bn; lh = c->lstm_hidden; ll = c->lstm_layers;
    if (n < 2 || hop < 1 || L < 1 || kf < 1 || kt < 1 || sf < 1 || pf < 0 || c->opf < 0)
      return fail(-1, "invalid DCCRN hyper-parameters");
    if (c->st != 1 || c->pt != 0 || c->opt != 0)
      return fail(-2, "streaming: the time axis needs stride 1, padding 0 and output padding 0");
    if (n % (2*hop)) return fail(-2, "streaming: n_fft must be a multiple of 2 hop");
    if (n > kMaxN) return fail(-2, "streaming: n_fft must be <= 4096");
    if (L > kMaxL) return fail(-2, "streaming: at most 8 encoder levels");
    if (kf*kt > 64) return fail(-2, "streaming: kernel_size[0] * kernel_size[1] must be <= 64");
    if (lh < 1 || lh > kMaxH || ll < 1 || ll > 4) return fail(-2, "streaming: lstm_channels <= 512, lstm_layers <= 4");
    P = n/(2*hop); G = kt - 1; D = L*G; lagh = 2*P - 1 + D; Fq0 = n/2; bins = n/2 + 1;
    C[0] = 1; H[0] = Fq0;
    for (int e = 1; e <= L; ++e) {
      C[e] = c->channels[e - 1];
      if (C[e] < 1 || C[e] > kMaxC) return fail(-2, "streaming: channel counts must be in [1, 1024]");
      H[e] = (H[e - 1] + 2*pf - kf)/sf + 1;
      if (H[e - 1] + 2*pf < kf || H[e] < 1) return fail(-2, "streaming: the encoder runs out of frequency bins");
    }
    for (int e = L; e >= 1; --e)
      if ((H[e] - 1)*sf - 2*pf + kf + c->opf != H[e - 1])
        return fail(-2, "streaming: the decoder's frequency axis does not retrace the encoder's");
    feat = C[L]*H[L];
    nbuf = 2*L + 2;
    elems[0] = 2*Fq0; off[0] = 0; lim[0] = 0; ring[0] = D > G ? D : G;
    for (int e = 1; e <= L; ++e) { elems[e] = 2*C[e]*H[e]; off[e] = e*G; lim[e] = e*G; ring[e] = (L + 1 - e)*G; }
    elems[L + 1] = 2*feat; off[L + 1] = D; lim[L + 1] = D; ring[L + 1] = G;
    for (int k = 1; k <= L; ++k) {
      const int b = L + 1 + k;
      elems[b] = 2*C[L - k]*H[L - k]; off[b] = D; lim[b] = D - k*G; ring[b] = k < L ? G : 0;
    }
    long long o = 0;
    st_hist = o; o += n - hop;
    st_tail = o; o += n - hop;
    st_lstm = o; o += (long long)ll*4*2*lh;
    for (int b = 0; b < nbuf; ++b) { st_ring[b] = o; o += (long long)ring[b]*elems[b]; }
    st_floats = o;
    st_bytes = upD(kHdr + 4*o, 256);
    return 0;
  }
};

// workspace of one call (floats)
struct WsD {
  long long xin, buf[kNB], proj, hout, ms, fr, total;
  void init(const Geo& g, long long C, int F) {
    long long o = 0;
    auto take = [&](long long k) { long long r = o; o += upD(k, 64); return r; };
    xin = take(C*g.hop);
    for (int b = 0; b < g.nbuf; ++b) buf[b] = take(C*g.elems[b]);
    proj = take(C*16LL*g.lh); hout = take((long long)g.ll*C*4*g.lh);
    ms = take(C*2LL*g.bins); fr = take(C*(long long)g.n);
    total = o;
    (void)F;
  }
};

struct Call {
  Geo g;
  const int32_t* ids; unsigned char* state;
  int F; long long C;                 // columns = n F, column = stream-major
  long long end_rest;                 // < 0: ordinary step; r: the tail of a stream ending r samples into hop 0
  const float* x; float* ws; WsD w;
};

__device__ __forceinline__ unsigned char* slot_of(const Call& c, long long col) {
  return c.state + (long long)c.ids[col / c.F]*c.g.st_bytes;
}
__device__ __forceinline__ float* sfl(const Call& c, long long col) { return (float*)(slot_of(c, col) + kHdr); }
__device__ __forceinline__ long long hops_of(const Call& c, long long col) { return *(const long long*)slot_of(c, col); }
// STFT frames of the stream (kNever until its tail)
__device__ __forceinline__ long long frames_of(const Call& c, long long R) {
  if (c.end_rest < 0) return kNever;
  const long long len = R*c.g.hop + c.end_rest;
  const long long over = len > c.g.n ? len - c.g.n : 0;
  return (over + c.g.hop - 1)/c.g.hop + 1 + 2*c.g.P;
}
__device__ __forceinline__ long long tau_of(const Call& c, long long col, long long R) {
  return R + col % c.F - c.g.P + 1;
}
__device__ __forceinline__ bool exists(const Call& c, int b, long long v, long long T) {
  return v >= 0 && v < T - c.g.lim[b];
}
// frame v of buffer b, seen from column col whose own frame of buffer b is vcur
__device__ __forceinline__ const float* frame_ptr(const Call& c, int b, long long col, long long vcur, long long v) {
  const long long back = vcur - v;
  if (col % c.F - back >= 0) return c.ws + c.w.buf[b] + (col - back)*c.g.elems[b];
  return sfl(c, col) + c.g.st_ring[b] + (v % c.g.ring[b])*c.g.elems[b];
}

template <int AMP> __device__ __forceinline__ float op(float v) { return AMP ? rbf(v) : v; }
__device__ __forceinline__ float sigm(float v) { return 1.f/(1.f + expf(-v)); }

// ---- 1. framing + DFT: spectrum bins 1 .. n/2 of frame tau -> buffer 0 (real plane, imaginary plane)
__global__ __launch_bounds__(256) void dft_kernel(const Call c, const double* basis) {
  __shared__ float smp[kMaxN];
  const Geo& g = c.g;
  const long long col = blockIdx.x;
  const long long R = hops_of(c, col), T = frames_of(c, R), tau = tau_of(c, col, R);
  if (!exists(c, 0, tau, T)) return;
  const long long s0 = R*g.hop;                              // first sample of this call
  const long long f = col % c.F;
  const float* xs = c.x + (col - f)*g.hop;                  // this stream's new samples
  const float* hist = sfl(c, col) + g.st_hist;              // samples s0 - (n - hop) .. s0 - 1
  for (int i = threadIdx.x; i < g.n; i += 256) {
    const long long s = g.hop*tau - g.n/2 + i;
    const long long d = s - s0;
    float v = 0.f;
    if (d >= 0) v = xs[d];
    else if (s >= 0) v = hist[g.n - g.hop + d];
    smp[i] = v;
  }
  __syncthreads();
  float* out = c.ws + c.w.buf[0] + col*g.elems[0];
  for (int j = threadIdx.x; j < 2*g.Fq0; j += 256) {
    const int part = j / g.Fq0, bin = j % g.Fq0 + 1;
    const double* row = basis + (2LL*bin + part)*g.n;
    double acc = 0.0;
    for (int i = 0; i < g.n; ++i) acc = fma((double)smp[i], row[i], acc);
    out[j] = (float)acc;
  }
}

// ---- 2. complex (transposed) convolution + bias + eval norm + PReLU, one lane per (column, channel, bin)
struct ConvK {
  Call c;
  int dec, level;                  // encoder level e / decoder k
  const float *wr, *br, *wi, *bi, *nw, *nb, *slope, *rm, *rv;
  float eps;
};

template <int AMP>
__global__ __launch_bounds__(256) void conv_kernel(const ConvK k) {
  const Call& c = k.c;
  const Geo& g = c.g;
  int Cx, Hin, Cout, Hout, bx, bs, bo, nsrc;
  long long vcur_x, vcur_s, vout_off;
  if (!k.dec) {
    const int e = k.level;
    Cx = g.C[e - 1]; Hin = g.H[e - 1]; Cout = g.C[e]; Hout = g.H[e];
    bx = e - 1; bs = -1; bo = e; nsrc = 1;
  } else {
    const int kk = k.level, e = g.L + 1 - kk;
    Cx = g.C[e]; Hin = g.H[e]; Cout = g.C[e - 1]; Hout = g.H[e - 1];
    bx = kk == 1 ? g.L + 1 : g.L + kk; bs = e; bo = g.L + 1 + kk; nsrc = 2;
  }
  const long long per = (long long)Cout*Hout;
  const long long idx = (long long)blockIdx.x*256 + threadIdx.x;
  if (idx >= c.C*per) return;
  const long long col = idx / per;
  const int co = (int)(idx % per / Hout), ho = (int)(idx % Hout);
  const long long R = hops_of(c, col), T = frames_of(c, R), tau = tau_of(c, col, R);
  const long long vout = tau - g.off[bo];
  if (!exists(c, bo, vout, T)) return;
  vcur_x = tau - g.off[bx];
  vcur_s = bs >= 0 ? tau - g.off[bs] : 0;
  (void)vout_off;
  const int Cin = nsrc*Cx;                     // complex input channels of the convolution
  float re = 0.f, im = 0.f;
  for (int b = 0; b < g.kt; ++b) {
    // encoder: input frame vout + b; decoder: input frame vout - b (absent outside the producer's frames)
    const long long v = k.dec ? vout - b : vout + b;
    if (k.dec && !exists(c, bx, v, T)) continue;
    const float* xp = frame_ptr(c, bx, col, vcur_x, v);
    const float* sp = bs >= 0 ? frame_ptr(c, bs, col, vcur_s, v) : xp;
    for (int ci = 0; ci < Cin; ++ci) {
      const float* src = ci < Cx ? xp : sp;
      const int cc = ci < Cx ? ci : ci - Cx;
      for (int a = 0; a < g.kf; ++a) {
        int hi;
        if (!k.dec) {
          hi = ho*g.sf - g.pf + a;
        } else {
          const int hn = ho + g.pf - a;
          if (hn < 0 || hn % g.sf) continue;
          hi = hn / g.sf;
        }
        if (hi < 0 || hi >= Hin) continue;
        const float xr = op<AMP>(src[(long long)cc*Hin + hi]), xi = op<AMP>(src[(long long)(Cx + cc)*Hin + hi]);
        const long long wo = k.dec ? (((long long)ci*Cout + co)*g.kf + a)*g.kt + b
                                   : (((long long)co*Cin + ci)*g.kf + a)*g.kt + b;
        const float wr = op<AMP>(k.wr[wo]), wi = op<AMP>(k.wi[wo]);
        re = __builtin_fmaf(wr, xr, re); re = __builtin_fmaf(-wi, xi, re);
        im = __builtin_fmaf(wr, xi, im); im = __builtin_fmaf(wi, xr, im);
      }
    }
  }
  re += k.br[co] - k.bi[co];
  im += k.br[co] + k.bi[co];
  if (k.nw) {
    if (!g.cbn) {
      re = (re - k.rm[co])*(1.f/sqrtf(k.rv[co] + k.eps))*k.nw[co] + k.nb[co];
      im = (im - k.rm[Cout + co])*(1.f/sqrtf(k.rv[Cout + co] + k.eps))*k.nw[Cout + co] + k.nb[Cout + co];
    } else {
      // ComplexBatchNorm2d in eval mode: whiten with the running 2x2 covariance, then the 2x2 affine map
      const float t0 = re - k.rm[co], t1 = im - k.rm[Cout + co];
      const float vrr = k.rv[co], vri = k.rv[Cout + co], vii = k.rv[3*Cout + co];
      const float s = sqrtf(vrr*vii - vri*vri);
      const float den = sqrtf(vrr + vii + 2.f*s)*s;
      const float p = (vii + s)/den, q = -vri/den, r = -vri/den, s2 = (vrr + s)/den;
      const float z0 = t0*p + t1*r, z1 = t0*q + t1*s2;
      const float w0 = k.nw[co], w1 = k.nw[Cout + co], w2 = k.nw[2*Cout + co];
      re = z0*w0 + z1*w1 + k.nb[co];
      im = z0*w1 + z1*w2 + k.nb[Cout + co];
    }
  }
  if (k.slope) { const float a = *k.slope; re = prelu(re, a); im = prelu(im, a); }
  float* out = c.ws + c.w.buf[bo] + col*g.elems[bo];
  out[(long long)co*Hout + ho] = re;
  out[(long long)(Cout + co)*Hout + ho] = im;
}

// ---- 3a. LSTM input projection of layer l: gates of the 4 chains (module_real / module_imag x real /
// imaginary input), biases included
struct LstmK {
  Call c; int layer;
  const float* wih[2]; const float* whh[2]; const float* bih[2]; const float* bhh[2];
};

__device__ __forceinline__ float lstm_in(const Call& c, int layer, long long col, int imag, int k) {
  const Geo& g = c.g;
  if (layer == 0) return c.ws[c.w.buf[g.L] + col*g.elems[g.L] + (imag ? g.feat : 0) + k];
  const float* h = c.ws + c.w.hout + (((long long)(layer - 1)*c.C + col)*4)*g.lh;
  // complex mix of the previous layer: real = rr - ii, imag = ri + ir
  return imag ? h[2*g.lh + k] + h[3*g.lh + k] : h[k] - h[g.lh + k];
}

template <int AMP>
__global__ __launch_bounds__(256) void lstm_proj_kernel(const LstmK k) {
  const Call& c = k.c;
  const Geo& g = c.g;
  const int G4 = 4*g.lh;
  const long long idx = (long long)blockIdx.x*256 + threadIdx.x;
  if (idx >= c.C*4*G4) return;
  const long long col = idx / (4*G4);
  const int q = (int)(idx % (4*G4) / G4), gi = (int)(idx % G4);
  const long long R = hops_of(c, col), T = frames_of(c, R), tau = tau_of(c, col, R);
  if (!exists(c, g.L + 1, tau - g.D, T)) return;
  const int m = q & 1, imag = q == 1 || q == 2;      // chains: rr, ii, ri, ir
  const int In = k.layer == 0 ? g.feat : g.lh;
  const float* w = k.wih[m] + (long long)gi*In;
  float acc = 0.f;
  for (int i = 0; i < In; ++i) acc = __builtin_fmaf(op<AMP>(w[i]), op<AMP>(lstm_in(c, k.layer, col, imag, i)), acc);
  c.ws[c.w.proj + (col*4 + q)*G4 + gi] = acc + k.bih[m][gi] + k.bhh[m][gi];
}

// ---- 3b. recurrence of layer l: one workgroup per (stream, chain) walks the call's frames in order
template <int AMP>
__global__ __launch_bounds__(256) void lstm_rec_kernel(const LstmK k) {
  __shared__ float hs[kMaxH], cs[kMaxH], gates[4*kMaxH];
  const Call& c = k.c;
  const Geo& g = c.g;
  const int H = g.lh, G4 = 4*H;
  const long long s = blockIdx.x / 4;
  const int q = blockIdx.x % 4, m = q & 1;
  const long long col0 = s*c.F;
  const long long R = hops_of(c, col0), T = frames_of(c, R);
  float* st = sfl(c, col0) + g.st_lstm + ((long long)k.layer*4 + q)*2*H;
  for (int j = threadIdx.x; j < H; j += 256) { hs[j] = st[j]; cs[j] = st[H + j]; }
  __syncthreads();
  const float* whh = k.whh[m];
  for (int f = 0; f < c.F; ++f) {
    const long long col = col0 + f;
    if (!exists(c, g.L + 1, tau_of(c, col, R) - g.D, T)) continue;      // (uniform in the workgroup)
    for (int gi = threadIdx.x; gi < G4; gi += 256) {
      const float* w = whh + (long long)gi*H;
      float acc = 0.f;
      for (int i = 0; i < H; ++i) acc = __builtin_fmaf(op<AMP>(w[i]), op<AMP>(hs[i]), acc);
      gates[gi] = c.ws[c.w.proj + (col*4 + q)*G4 + gi] + acc;
    }
    __syncthreads();
    float* hout = c.ws + c.w.hout + (((long long)k.layer*c.C + col)*4 + q)*H;
    for (int j = threadIdx.x; j < H; j += 256) {
      const float ig = sigm(gates[j]), fg = sigm(gates[H + j]), gg = tanhf(gates[2*H + j]), og = sigm(gates[3*H + j]);
      const float cn = fg*cs[j] + ig*gg;
      const float hn = og*tanhf(cn);
      cs[j] = cn; hs[j] = hn; hout[j] = hn;
    }
    __syncthreads();
  }
  for (int j = threadIdx.x; j < H; j += 256) { st[j] = hs[j]; st[H + j] = cs[j]; }
}

// ---- 3c. linear_r | linear_i on the last layer's complex output -> buffer L + 1
struct LinK { Call c; const float *wr, *br, *wi, *bi; };

template <int AMP>
__global__ __launch_bounds__(256) void linear_kernel(const LinK k) {
  const Call& c = k.c;
  const Geo& g = c.g;
  const long long idx = (long long)blockIdx.x*256 + threadIdx.x;
  if (idx >= c.C*2*g.feat) return;
  const long long col = idx / (2*g.feat);
  const int j = (int)(idx % (2*g.feat));
  const long long R = hops_of(c, col), T = frames_of(c, R), tau = tau_of(c, col, R);
  if (!exists(c, g.L + 1, tau - g.D, T)) return;
  const int imag = j >= g.feat, jj = imag ? j - g.feat : j;
  const float* w = (imag ? k.wi : k.wr) + (long long)jj*g.lh;
  float acc = 0.f;
  for (int i = 0; i < g.lh; ++i) acc = __builtin_fmaf(op<AMP>(w[i]), op<AMP>(lstm_in(c, g.ll, col, imag, i)), acc);
  c.ws[c.w.buf[g.L + 1] + col*g.elems[g.L + 1] + j] = acc + (imag ? k.bi : k.br)[jj];
}

// ---- 4. mask (DCCRN.apply_mask, the formula of the offline kernel) -> masked spectrum, bins 0 .. n/2
__global__ __launch_bounds__(256) void mask_kernel(const Call c) {
  const Geo& g = c.g;
  const long long idx = (long long)blockIdx.x*256 + threadIdx.x;
  if (idx >= c.C*g.Fq0) return;
  const long long col = idx / g.Fq0;
  const int f = (int)(idx % g.Fq0);
  const long long R = hops_of(c, col), T = frames_of(c, R), tau = tau_of(c, col, R);
  const long long m = tau - g.D;
  if (!exists(c, 2*g.L + 1, m, T)) return;
  const float* spec = frame_ptr(c, 0, col, tau, m);
  const float* mk = c.ws + c.w.buf[2*g.L + 1] + col*g.elems[2*g.L + 1];
  const float a = spec[f], b = spec[g.Fq0 + f];
  const float in_mag = sqrtf(a*a + b*b), in_phase = atan2f(b, a);
  float pr = mk[f];
  const float pi = mk[g.Fq0 + f];
  const float mag = tanhf(sqrtf(pr*pr + pi*pi + 1e-7f));
  if (pr == 0.f) pr = 1e-7f;
  const float ph = in_phase + atan2f(pi, pr);
  const float om = in_mag*mag;
  float* out = c.ws + c.w.ms + col*2LL*g.bins;
  out[2*(f + 1)] = om*cosf(ph);
  out[2*(f + 1) + 1] = om*sinf(ph);
  if (f == 0) { out[0] = 0.f; out[1] = 0.f; }        // the DC row the offline path puts back as zeros
}

// ---- 5. inverse DFT of the masked frame (window and normalisation in the synthesis table)
__global__ __launch_bounds__(256) void idft_kernel(const Call c, const double* synth) {
  __shared__ float sp[2*(kMaxN/2 + 1)];
  const Geo& g = c.g;
  const long long col = blockIdx.x;
  const long long R = hops_of(c, col), T = frames_of(c, R), tau = tau_of(c, col, R);
  if (!exists(c, 2*g.L + 1, tau - g.D, T)) return;
  const float* ms = c.ws + c.w.ms + col*2LL*g.bins;
  for (int i = threadIdx.x; i < 2*g.bins; i += 256) sp[i] = ms[i];
  __syncthreads();
  float* fr = c.ws + c.w.fr + col*g.n;
  for (int i = threadIdx.x; i < g.n; i += 256) {
    double acc = 0.0;
    for (int kb = 0; kb < g.bins; ++kb) {
      acc = fma((double)sp[2*kb], synth[(2LL*kb)*g.n + i], acc);
      acc = fma((double)sp[2*kb + 1], synth[(2LL*kb + 1)*g.n + i], acc);
    }
    fr[i] = (float)acc;
  }
}

// ---- 6. overlap-add, window-square envelope, output; state commit. One workgroup per stream.
__global__ __launch_bounds__(256) void commit_kernel(const Call c, const float* win, float* y, long long ylen) {
  __shared__ float tail[kMaxN], tmp[kMaxN];
  const Geo& g = c.g;
  const long long s = blockIdx.x, col0 = s*c.F;
  unsigned char* sl = slot_of(c, col0);
  float* st = sfl(c, col0);
  const long long R = *(const long long*)sl, T = frames_of(c, R);
  const int nt = g.n - g.hop;
  for (int i = threadIdx.x; i < nt; i += 256) tail[i] = st[g.st_tail + i];
  __syncthreads();
  for (int f = 0; f < c.F; ++f) {
    const long long col = col0 + f;
    const long long m = tau_of(c, col, R) - g.D;         // frame whose inverse DFT joins now
    const bool mok = exists(c, 2*g.L + 1, m, T);
    const float* fr = c.ws + c.w.fr + col*g.n;
    const long long j = R + f - g.lagh;                  // output hop completed by frame m
    for (int q = threadIdx.x; q < g.hop; q += 256) {
      float acc = tail[q];
      if (mok) acc += fr[q];
      float out = 0.f;
      if (j >= 0) {
        // torch.istft: divide by the sum of squared window weights of the frames that exist
        long long t0 = j - g.P + 1, t1 = j + g.P;
        if (t0 < 0) t0 = 0;
        if (t1 > T - 1) t1 = T - 1;
        float env = 0.f;
        for (long long t = t0; t <= t1; ++t) {
          const float w = win[(j - t)*g.hop + q + g.n/2];
          env += w*w;
        }
        out = env > 0.f ? acc/env : 0.f;
      }
      const long long p = (long long)f*g.hop + q;
      if (p < ylen) y[s*ylen + p] = out;
    }
    for (int q = threadIdx.x; q < nt; q += 256) {
      float v = q + g.hop < nt ? tail[q + g.hop] : 0.f;
      if (mok) v += fr[g.hop + q];
      tmp[q] = v;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nt; q += 256) tail[q] = tmp[q];
    __syncthreads();
  }
  for (int i = threadIdx.x; i < nt; i += 256) st[g.st_tail + i] = tail[i];
  // input history: the last n - hop samples of [history, this call's samples]
  const long long FH = (long long)c.F*g.hop;
  const float* xs = c.x + col0*g.hop;
  for (int i = threadIdx.x; i < nt; i += 256) {
    const long long p = FH + i;            // index into the concatenation
    tmp[i] = p < nt ? st[g.st_hist + p] : xs[p - nt];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nt; i += 256) st[g.st_hist + i] = tmp[i];
  // rings: the last ring[b] frames of every buffer that exist
  for (int b = 0; b < g.nbuf; ++b) {
    const int rl = g.ring[b];
    if (rl == 0) continue;
    const int E = g.elems[b];
    for (int f = c.F - rl > 0 ? c.F - rl : 0; f < c.F; ++f) {
      const long long col = col0 + f;
      const long long v = tau_of(c, col, R) - g.off[b];
      if (!exists(c, b, v, T)) continue;
      const float* src = c.ws + c.w.buf[b] + col*E;
      float* dst = st + g.st_ring[b] + (v % rl)*E;
      for (int i = threadIdx.x; i < E; i += 256) dst[i] = src[i];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *(long long*)sl = R + c.F;
}

__global__ __launch_bounds__(256) void reset_kernel(unsigned char* state, long long st_bytes, const int32_t* ids) {
  unsigned int* p = (unsigned int*)(state + (long long)ids[blockIdx.x]*st_bytes);
  for (long long i = threadIdx.x; i < st_bytes/4; i += 256) p[i] = 0u;
}

// the tail's input: the last r samples of each stream, then zeros
__global__ __launch_bounds__(256) void tail_input_kernel(const float* rest, long long r, float* x, long long per) {
  const long long idx = (long long)blockIdx.x*256 + threadIdx.x;
  const long long s = blockIdx.y;
  if (idx >= per) return;
  x[s*per + idx] = idx < r ? rest[s*r + idx] : 0.f;
}

unsigned blocks_for(long long n) { return (unsigned)((n + 255)/256); }

template <int AMP>
int run(const brv_dccrn_stream_config* cfg, const Geo& g, const float* params, const float* window,
        const double* basis, const double* synth, void* state, const int32_t* ids, long long n, const float* x,
        int F, long long end_rest, float* y, long long ylen, void* workspace, hipStream_t st) {
  const long long C = n*F;
  Call c;
  memset(&c, 0, sizeof(c));
  c.g = g; c.ids = ids; c.state = (unsigned char*)state; c.F = F; c.C = C; c.end_rest = end_rest;
  c.ws = (float*)workspace; c.w.init(g, C, F);
  c.x = x ? x : c.ws + c.w.xin;
  const auto P = [&](long long off) { return off >= 0 ? params + off : (const float*)nullptr; };
  hipLaunchKernelGGL(dft_kernel, dim3((unsigned)C), dim3(256), 0, st, c, basis);
  auto conv = [&](int dec, int level) {
    const int blk = dec ? g.L + level - 1 : level - 1;
    const int64_t* o = cfg->off_block[blk];
    ConvK k{c, dec, level, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]), P(o[6]),
            o[4] >= 0 ? cfg->run_mean[blk] : nullptr, o[4] >= 0 ? cfg->run_var[blk] : nullptr, cfg->eps[blk]};
    const int e = dec ? g.L + 1 - level : level;
    const long long per = dec ? (long long)g.C[e - 1]*g.H[e - 1] : (long long)g.C[e]*g.H[e];
    hipLaunchKernelGGL((conv_kernel<AMP>), dim3(blocks_for(C*per)), dim3(256), 0, st, k);
  };
  for (int e = 1; e <= g.L; ++e) conv(0, e);
  for (int l = 0; l < g.ll; ++l) {
    LstmK k;
    k.c = c; k.layer = l;
    for (int m = 0; m < 2; ++m) {
      k.wih[m] = P(cfg->off_lstm[l][m][0]); k.whh[m] = P(cfg->off_lstm[l][m][1]);
      k.bih[m] = P(cfg->off_lstm[l][m][2]); k.bhh[m] = P(cfg->off_lstm[l][m][3]);
    }
    hipLaunchKernelGGL((lstm_proj_kernel<AMP>), dim3(blocks_for(C*16LL*g.lh)), dim3(256), 0, st, k);
    hipLaunchKernelGGL((lstm_rec_kernel<AMP>), dim3((unsigned)(4*n)), dim3(256), 0, st, k);
  }
  {
    LinK k{c, P(cfg->off_linear[0]), P(cfg->off_linear[1]), P(cfg->off_linear[2]), P(cfg->off_linear[3])};
    hipLaunchKernelGGL((linear_kernel<AMP>), dim3(blocks_for(C*2LL*g.feat)), dim3(256), 0, st, k);
  }
  for (int kk = 1; kk <= g.L; ++kk) conv(1, kk);
  hipLaunchKernelGGL(mask_kernel, dim3(blocks_for(C*g.Fq0)), dim3(256), 0, st, c);
  hipLaunchKernelGGL(idft_kernel, dim3((unsigned)C), dim3(256), 0, st, c, synth);
  hipLaunchKernelGGL(commit_kernel, dim3((unsigned)n), dim3(256), 0, st, c, window, y, ylen);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int check_cfg_params(const brv_dccrn_stream_config* cfg, const Geo& g) {
  for (int b = 0; b < 2*g.L; ++b) {
    const int64_t* o = cfg->off_block[b];
    for (int i = 0; i < 4; ++i) if (o[i] < 0) return fail(-1, "streaming: missing convolution parameter offset");
    const bool last = b == 2*g.L - 1;
    if (!last && (o[4] < 0 || o[5] < 0 || o[6] < 0 || !cfg->run_mean[b] || !cfg->run_var[b]))
      return fail(-1, "streaming: missing norm / PReLU of a block");
    if (last && (o[4] >= 0 || o[6] >= 0)) return fail(-2, "streaming: the last decoder block has no norm / PReLU");
  }
  return 0;
}

int step_common(const brv_dccrn_stream_config* cfg, const float* params, const float* window, const double* basis,
                const double* synth, void* state, const int32_t* ids, int64_t n, const float* x, int64_t hops,
                int64_t end_rest, float* y, int64_t ylen, int32_t amp, void* workspace, int64_t workspace_bytes,
                hipStream_t st) {
  Geo g; if (int r = g.init(cfg)) return r;
  if (int r = check_cfg_params(cfg, g)) return r;
  if (n < 1 || hops < 1) return fail(-1, "streaming: n and hops must be >= 1");
  long long widest = 16LL*g.lh > 2LL*g.feat ? 16LL*g.lh : 2LL*g.feat;
  for (int e = 0; e <= g.L; ++e) widest = (long long)g.C[e]*g.H[e] > widest ? (long long)g.C[e]*g.H[e] : widest;
  if (hops > (1 << 20) || n*hops > (1LL << 30)/widest*256) return fail(-2, "streaming: too many columns in one call");
  if (!params || !window || !basis || !synth || !state || !ids || !y || !workspace)
    return fail(-1, "streaming: null pointer argument");
  WsD w; w.init(g, n*hops, (int)hops);
  if (workspace_bytes < w.total*4) return fail(-1, "streaming: workspace too small");
  if (amp) return run<1>(cfg, g, params, window, basis, synth, state, ids, n, x, (int)hops, end_rest, y, ylen,
                         workspace, st);
  return run<0>(cfg, g, params, window, basis, synth, state, ids, n, x, (int)hops, end_rest, y, ylen, workspace, st);
}

}  // namespace

extern "C" {

int64_t brv_dccrn_stream_state_bytes(const brv_dccrn_stream_config* cfg) {
  Geo g; if (int r = g.init(cfg)) return r;
  return g.st_bytes;
}

int64_t brv_dccrn_stream_workspace_bytes(const brv_dccrn_stream_config* cfg, int64_t n, int64_t hops, int32_t amp) {
  (void)amp;     // both precisions keep fp32 activations between the launches
  Geo g; if (int r = g.init(cfg)) return r;
  if (n < 1 || hops < 1) return fail(-1, "streaming: n and hops must be >= 1");
  WsD w; w.init(g, n*hops, (int)hops);
  return w.total*4;
}

int brv_dccrn_stream_reset(const brv_dccrn_stream_config* cfg, void* state, const int32_t* ids, int64_t n,
                           brv_stream_t stream) {
  Geo g; if (int r = g.init(cfg)) return r;
  if (n < 1) return 0;
  hipLaunchKernelGGL(reset_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (unsigned char*)state,
                     g.st_bytes, ids);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

int brv_dccrn_stream_step(const brv_dccrn_stream_config* cfg, const float* params, const float* window,
                          const double* basis, const double* synthesis, void* state, const int32_t* ids,
                          int64_t n, const float* x, int64_t hops, float* y, int32_t amp, void* workspace,
                          int64_t workspace_bytes, const brv_launch_opts* opts, brv_stream_t stream) {
  (void)opts;    // no option of this entry point yet (size / flags reserved)
  if (!x) return fail(-1, "streaming: null input");
  Geo g; if (int r = g.init(cfg)) return r;
  return step_common(cfg, params, window, basis, synthesis, state, ids, n, x, hops, -1, y, hops*g.hop, amp,
                     workspace, workspace_bytes, (hipStream_t)stream);
}

int brv_dccrn_stream_tail(const brv_dccrn_stream_config* cfg, const float* params, const float* window,
                          const double* basis, const double* synthesis, void* state, const int32_t* ids,
                          int64_t n, const float* rest, int64_t r, float* y, int32_t amp, void* workspace,
                          int64_t workspace_bytes, const brv_launch_opts* opts, brv_stream_t stream) {
  (void)opts;
  Geo g; if (int e = g.init(cfg)) return e;
  if (r < 0 || r >= g.hop) return fail(-1, "streaming: the rest must be shorter than one hop");
  if (r > 0 && !rest) return fail(-1, "streaming: null rest");
  if (n < 1) return fail(-1, "streaming: n must be >= 1");
  const long long hops = g.lagh + (r > 0 ? 1 : 0);
  WsD w; w.init(g, n*hops, (int)hops);
  if (!workspace || workspace_bytes < w.total*4) return fail(-1, "streaming: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* xin = (float*)workspace + w.xin;
  const long long per = hops*g.hop;
  hipLaunchKernelGGL(tail_input_kernel, dim3(blocks_for(per), (unsigned)n), dim3(256), 0, st, rest, (long long)r,
                     xin, per);
  BRV_HIP_OK(hipGetLastError());
  return step_common(cfg, params, window, basis, synthesis, state, ids, n, nullptr, hops, r, y,
                     (long long)g.lagh*g.hop + r, amp, workspace, workspace_bytes, st);
}

}  // extern "C"
