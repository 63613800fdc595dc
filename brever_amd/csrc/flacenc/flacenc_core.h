// The encode core of libbrever_flacenc.so (include/brever_flacenc.h): one FLAC frame of RFC 9639, written as
// __host__ __device__ code over three small types the caller supplies, so that the kernel (flacenc.hip) and the
// stand-alone host check (tools/flac_enc_check.cpp) run the very same code. `encode_frame` is written for `nt`
// cooperating threads of which the caller is thread `tid`; the host runs it with nt = 1.
//
//   Src    get(code, i): quantised sample i of the frame, coded channel 0 left (or mono), 1 right, 2 mid, 3 side;
//          flags(c, i): the ROW_* bits of input channel c at sample i (non-finite, out of range)
//   Img    the frame's bytes as 32-bit words in memory order: zero(w), orw(w, v), load(w); words() is the capacity
//   Par    sync(): barrier of the nt threads; add64 / or32 / xor32: order-independent updates of a word of `Shared`;
//          publish(): makes the image's words written so far visible to load() of every thread after the next sync
//
// The search space and the order of ties. Per coded channel the candidates are tried in the order
// CONSTANT, VERBATIM, FIXED 0, 1, 2, 3, 4, LPC; a candidate replaces the best so far only when its exact coded bit
// count is strictly smaller. A FIXED / LPC candidate needs order < block size. Its residual is partitioned Rice,
// partition orders 0 ... MAX_PORDER where the block divides and every partition keeps a residual; per partition
// the parameter with the fewest bits, ties to the smaller one, once among 0 ... 14 (4-bit parameters) and once
// among 0 ... 30 (5-bit); then the (partition order, width) pair with the fewest bits, ties to the smaller
// partition order, then to 4 bits. Stereo takes the cheapest of independent, left/side, side/right, mid/side, in
// that order of ties. Every count is exact integer arithmetic, so nothing depends on the number of threads.
//
// LPC: one order, min(lpc_order, block - 1). Samples are reduced to 16 bits (arithmetic shift) and multiplied by an
// integer Welch window of at most 255; |v| < 2^23, so a lag sum over up to 65535 products stays below 2^62 and is
// exact in int64 whatever the order of summation. Levinson-Durbin runs in fp64 on thread 0 (build with
// -ffp-contract=off); the coefficients are quantised to LPC_PRECISION bits with error feedback at the largest shift
// 0 ... 15 that keeps them in range. From there on everything is integer; a candidate one of whose residuals does not
// fit 32 bits is dropped.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define BRV_FE_HD __host__ __device__ __forceinline__
#else
#define BRV_FE_HD inline
#endif

namespace brv_flacenc {

// per-row status bits (include/brever_flacenc.h: BRV_FLACENC_ROW_*)
enum { ROW_NONFINITE = 1, ROW_RANGE = 2, ROW_LENGTH = 4, ROW_INTERNAL = 8 };
enum { KIND_CONSTANT = 0, KIND_VERBATIM = 1, KIND_FIXED = 2, KIND_LPC = 3 };
constexpr int MAX_PORDER = 4, MAX_PARTS = 1 << MAX_PORDER, NODES = 2*MAX_PARTS - 1;
constexpr int NK = 31;                       // Rice parameters 0 ... 30 (31 is the 5-bit escape code)
constexpr int MAX_LPC = 32, LPC_PRECISION = 12;
constexpr int MAX_THREADS = 256;
constexpr int STAGE = 4096;                  // samples of a coded channel kept in `Shared` (a default block)

// ---- quantisation ------------------------------------------------------------------------------------------------
// clip(rint(x 2^(bps-1)), -2^(bps-1), 2^(bps-1) - 1), round half to even; 0 for a non-finite sample (the row is
// refused through flags())
BRV_FE_HD int32_t quantise(float x, int bps) {
  if (!(x - x == 0.0f)) return 0;
  const float hi = (float)((1 << (bps - 1)) - 1), lo = -(float)(1 << (bps - 1));
  const float y = x*(float)(1 << (bps - 1));
  if (y >= hi) return (1 << (bps - 1)) - 1;
  if (y <= lo) return -(1 << (bps - 1));
  return (int32_t)rintf(y);
}
BRV_FE_HD int float_flags(float x) { return x - x == 0.0f ? 0 : ROW_NONFINITE; }
BRV_FE_HD int pcm_flags(int32_t v, int bps) {
  return v < -(1 << (bps - 1)) || v > (1 << (bps - 1)) - 1 ? ROW_RANGE : 0;
}
BRV_FE_HD int32_t coded_channel(int code, int32_t l, int32_t r) {
  return code == 0 ? l : code == 1 ? r : code == 2 ? (l + r) >> 1 : l - r;
}

// ---- residuals and their codes -----------------------------------------------------------------------------------
// residual of the FIXED predictor of `order` at a sample x0 whose predecessors are x1 (newest) ... x4
BRV_FE_HD int32_t fixed_residual(int order, int32_t x0, int32_t x1, int32_t x2, int32_t x3, int32_t x4) {
  switch (order) {                               // 25-bit samples: below 2^28 in magnitude
    case 0: return x0;
    case 1: return x0 - x1;
    case 2: return x0 - 2*x1 + x2;
    case 3: return x0 - 3*x1 + 3*x2 - x3;
    default: return x0 - 4*x1 + 6*x2 - 4*x3 + x4;
  }
}
BRV_FE_HD uint32_t zigzag(int32_t r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }
BRV_FE_HD uint32_t rice_length(uint32_t u, int k) { return (u >> k) + 1u + (uint32_t)k; }

// ---- LPC analysis ------------------------------------------------------------------------------------------------
// integer Welch window of n points, 0 ... 255: 255 * 4 t (1 - t) with t = (i + 1)/(n + 1) in 16 fractional bits.
// step = window_step(n), so that a sample costs no division.
BRV_FE_HD uint32_t window_step(int n) { return (1u << 31)/(uint32_t)(n + 1); }
BRV_FE_HD int32_t window(int i, uint32_t step) {
  const uint64_t t = ((uint32_t)(i + 1)*step) >> 15;        // (i + 1) step < 2^31
  return (int32_t)((1020ull*t*(65536ull - t)) >> 32);
}
BRV_FE_HD int32_t windowed(int32_t x, int width, int i, uint32_t step) {
  return (width > 16 ? x >> (width - 16) : x)*window(i, step);
}

// Levinson-Durbin over the lags r[0 ... order] (as doubles): the predictor a[0 ... order-1],
// x^[i] = sum a[j] x[i-1-j]. false when the recursion breaks down (a zero or negative error).
BRV_FE_HD bool levinson(const double* r, int order, double* a) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  double err = r[0];
  if (!(err > 0.0)) return false;
  for (int i = 0; i < order; ++i) {
    double acc = r[i + 1];
    for (int j = 0; j < i; ++j) acc -= a[j]*r[i - j];
    const double k = acc/err;
    for (int j = 0; j < (i >> 1); ++j) {
      const double lo = a[j], hi = a[i - 1 - j];
      a[j] = lo - k*hi;
      a[i - 1 - j] = hi - k*lo;
    }
    if (i & 1) a[i >> 1] = a[i >> 1] - k*a[i >> 1];
    a[i] = k;
    err = err*(1.0 - k*k);
    if (!(err > 0.0)) return false;
  }
  return true;
}

// LPC_PRECISION-bit coefficients q and their shift (0 ... 15); false when no shift keeps them in range
BRV_FE_HD bool quantise_coefficients(const double* a, int order, int32_t* q, int32_t* shift) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double top = (double)((1 << (LPC_PRECISION - 1)) - 1);
  double cmax = 0.0;
  for (int j = 0; j < order; ++j) {
    const double m = a[j] < 0.0 ? -a[j] : a[j];
    if (!(m - m == 0.0)) return false;
    cmax = m > cmax ? m : cmax;
  }
  if (!(cmax > 0.0)) return false;
  int s = 15;
  while (s >= 0 && cmax*(double)(1 << s) > top) --s;
  if (s < 0) return false;
  double e = 0.0;
  for (int j = 0; j < order; ++j) {
    e = e + a[j]*(double)(1 << s);
    double v = floor(e + 0.5);
    v = v > top ? top : v < -top - 1.0 ? -top - 1.0 : v;
    q[j] = (int32_t)v;
    e = e - v;
  }
  *shift = s;
  return true;
}

// ---- CRCs --------------------------------------------------------------------------------------------------------
BRV_FE_HD uint32_t crc8_byte(uint32_t c, uint32_t byte) {          // x^8 + x^2 + x + 1
  c ^= byte;
  for (int b = 0; b < 8; ++b) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xffu : (c << 1) & 0xffu;
  return c;
}
BRV_FE_HD uint32_t crc16_byte(uint32_t c, uint32_t byte) {         // x^16 + x^15 + x^2 + 1
  c ^= byte << 8;
  for (int b = 0; b < 8; ++b) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xffffu : (c << 1) & 0xffffu;
  return c;
}
// a b mod P, polynomials over GF(2) of degree < 16
BRV_FE_HD uint32_t crc16_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 15; i >= 0; --i) {
    r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xffffu : (r << 1) & 0xffffu;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
// x^(8 bytes) mod P. The CRC has zero initial value, no reflection and no final XOR, so
// crc(A | B) = crc(A) x^(8 |B|) mod P  xor  crc(B).
BRV_FE_HD uint32_t crc16_shift(uint32_t bytes) {
  uint32_t result = 1, base = 0x100u;                       // x^8
  for (; bytes; bytes >>= 1) {
    if (bytes & 1u) result = crc16_mul(result, base);
    base = crc16_mul(base, base);
  }
  return result;
}

// ---- headers -----------------------------------------------------------------------------------------------------
BRV_FE_HD int block_size_code(int bs) {
  if (bs == 192) return 1;
  for (int c = 2; c <= 5; ++c) if (bs == (576 << (c - 2))) return c;
  for (int c = 8; c <= 15; ++c) if (bs == (256 << (c - 8))) return c;
  return bs <= 256 ? 6 : 7;
}
BRV_FE_HD int sample_rate_code(int rate) {
  const int table[11] = {88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  int code = 0;                                             // 0: from STREAMINFO
  for (int c = 0; c < 11; ++c) code = table[c] == rate ? c + 1 : code;
  return code;
}
// The frame header (fixed blocking strategy) with its CRC-8 into h (16 bytes hold it); returns its length.
// number < 2^31: at most 6 bytes in the UTF-8-like coding.
BRV_FE_HD int frame_header(uint8_t* h, int bs, int rate, int assignment, int bps, int64_t number) {
  int n = 0;
  const int bc = block_size_code(bs);
  h[n++] = 0xff; h[n++] = 0xf8;
  h[n++] = (uint8_t)((bc << 4) | sample_rate_code(rate));
  h[n++] = (uint8_t)((assignment << 4) | ((bps == 16 ? 4 : 6) << 1));
  const uint64_t v = (uint64_t)number;
  if (v < 0x80) {
    h[n++] = (uint8_t)v;
  } else {
    int extra = 1;
    while (extra < 6 && v >= (1ull << (5*extra + 6))) ++extra;
    h[n++] = (uint8_t)(((0xff00u >> (extra + 1)) & 0xffu) | (uint32_t)(v >> (6*extra)));
    for (int e = extra - 1; e >= 0; --e) h[n++] = (uint8_t)(0x80u | ((v >> (6*e)) & 0x3fu));
  }
  if (bc == 6) h[n++] = (uint8_t)(bs - 1);
  if (bc == 7) { h[n++] = (uint8_t)((bs - 1) >> 8); h[n++] = (uint8_t)((bs - 1) & 0xff); }
  uint32_t c = 0;
  for (int i = 0; i < n; ++i) c = crc8_byte(c, h[i]);
  h[n++] = (uint8_t)c;
  return n;
}

constexpr int STREAM_HEADER_BYTES = 42;
// 'fLaC', the STREAMINFO block header (last block) and STREAMINFO with an all-zero MD5 ("not computed"). The block
// sizes are the stream's nominal one twice: the RFC's minimum leaves out the last block, and values below 16 are
// not valid there.
BRV_FE_HD void stream_header(uint8_t* h, int block, uint32_t min_frame, uint32_t max_frame, int rate, int channels,
                             int bps, int64_t total) {
  const uint8_t head[8] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34};
  for (int i = 0; i < 8; ++i) h[i] = head[i];
  uint8_t* s = h + 8;
  s[0] = s[2] = (uint8_t)(block >> 8); s[1] = s[3] = (uint8_t)(block & 0xff);
  s[4] = (uint8_t)(min_frame >> 16); s[5] = (uint8_t)(min_frame >> 8); s[6] = (uint8_t)min_frame;
  s[7] = (uint8_t)(max_frame >> 16); s[8] = (uint8_t)(max_frame >> 8); s[9] = (uint8_t)max_frame;
  s[10] = (uint8_t)(rate >> 12); s[11] = (uint8_t)(rate >> 4);
  s[12] = (uint8_t)(((rate & 15) << 4) | ((channels - 1) << 1) | (((bps - 1) >> 4) & 1));
  s[13] = (uint8_t)((((bps - 1) & 15) << 4) | (int)((total >> 32) & 15));
  s[14] = (uint8_t)(total >> 24); s[15] = (uint8_t)(total >> 16); s[16] = (uint8_t)(total >> 8); s[17] = (uint8_t)total;
  for (int i = 18; i < 34; ++i) s[i] = 0;
}

// bytes that hold any frame of the block size: the header, per channel a VERBATIM subframe one bit wider than
// the samples (a side channel), the padding and the CRC-16; a multiple of 256 so that no two frames' images
// share a cache line
BRV_FE_HD int64_t frame_capacity(int64_t channels, int64_t bps, int64_t block) {
  const int64_t bytes = 16 + (channels*(8 + block*(bps + 1)) + 7)/8 + 2;
  return (bytes + 4 + 255)/256*256;
}

// ---- the image ---------------------------------------------------------------------------------------------------
// nbits (1 ... 32) of value at bit `pos` of the frame, MSB first; the bits there are still zero. Touches at most
// two words; a position beyond the capacity writes nothing and returns false.
template <class Img>
BRV_FE_HD bool put_bits(Img& img, uint32_t pos, uint32_t value, int nbits) {
  const uint32_t w = pos >> 5;
  if (nbits < 1 || nbits > 32 || w + 1 >= img.words()) return false;
  const uint64_t v = (uint64_t)(nbits == 32 ? value : value & ((1u << nbits) - 1u)) << (64 - nbits - (int)(pos & 31u));
  const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
  if (hi) img.orw(w, __builtin_bswap32(hi));
  if (lo) img.orw(w + 1, __builtin_bswap32(lo));
  return true;
}
template <class Img>
BRV_FE_HD uint32_t image_byte(Img& img, uint32_t at) { return (img.load(at >> 2) >> (8*(at & 3u))) & 0xffu; }

// ---- the state the threads of a frame share ----------------------------------------------------------------------
struct ChannelChoice {
  uint64_t bits;
  int32_t kind, order, porder, five_bit, shift, value;
  int32_t k[MAX_PARTS];
  int32_t coef[MAX_LPC];
};

struct Shared {
  uint64_t sums[NODES*NK];       // per node of the partition tree (level p at 2^p - 1) and parameter: sum of u >> k
  uint64_t best4[NODES], best5[NODES];
  int64_t lags[MAX_LPC + 1];
  double lpc_r[MAX_LPC + 1], lpc_a[MAX_LPC];
  ChannelChoice choice[4];
  int32_t k4[NODES], k5[NODES];
  int32_t lpc_q[MAX_LPC], lpc_shift, lpc_ok;
  uint32_t scan[2][MAX_THREADS];
  int32_t stage[STAGE];          // the first STAGE samples of the coded channel being worked on
  uint32_t flags, differs, overflow, crc, bad_put;
  uint32_t total_bits, header_bytes, sub_base[2];
  int32_t assignment, sub_code[2];
  uint8_t header[16];
};

struct Frame {
  int bs;                        // samples of this frame, 1 ... 65535
  int channels, bps, rate;       // 1 or 2; 16 or 24
  int lpc_order;                 // 0 ... MAX_LPC
  int64_t number;
};

BRV_FE_HD int coded_width(int code, int bps) { return code == 3 ? bps + 1 : bps; }
BRV_FE_HD int max_porder(int bs, int order) {
  int p = 0;
  while (p < MAX_PORDER && (bs & ((2 << p) - 1)) == 0 && (bs >> (p + 1)) > order) ++p;
  return p;
}
BRV_FE_HD int chunk_of(int n, int nt) { return (n + nt - 1)/nt; }

// A source whose coded channel `code` is read from the staged copy below sample n: a candidate reads every sample
// up to 33 times, and the source quantises and decorrelates at every read.
template <class Src>
struct Staged {
  const Src& src; const int32_t* stage; int code, n;
  BRV_FE_HD int32_t get(int c, int i) const { return c == code && i < n ? stage[i] : src.get(c, i); }
};
template <class Par, class Src>
BRV_FE_HD Staged<Src> stage_channel(Par& par, Shared* sh, const Src& src, int code, int bs, int tid, int nt) {
  const int n = bs < STAGE ? bs : STAGE;
  par.sync();                                               // the readers of the channel staged before are done
  for (int i = tid; i < n; i += nt) sh->stage[i] = src.get(code, i);
  par.sync();
  return Staged<Src>{src, sh->stage, code, n};
}

// the residual of the candidate at sample i >= order (LPC: with the coefficients q and their shift); *fits is
// cleared when an LPC residual leaves 32 bits
template <class Src>
BRV_FE_HD int32_t residual_at(const Src& src, const int32_t* q, int shift, int code, int kind, int order, int i,
                              bool* fits) {
  if (kind == KIND_FIXED) {
    const int32_t x0 = src.get(code, i), x1 = order > 0 ? src.get(code, i - 1) : 0,
                  x2 = order > 1 ? src.get(code, i - 2) : 0, x3 = order > 2 ? src.get(code, i - 3) : 0,
                  x4 = order > 3 ? src.get(code, i - 4) : 0;
    return fixed_residual(order, x0, x1, x2, x3, x4);
  }
  int64_t acc = 0;                                          // 25-bit samples x 12-bit coefficients x 32 taps: 2^41
  for (int j = 0; j < order; ++j) acc += (int64_t)q[j]*(int64_t)src.get(code, i - 1 - j);
  const int64_t r = (int64_t)src.get(code, i) - (acc >> shift);
  if (r < -2147483647ll || r > 2147483647ll) { *fits = false; return 0; }
  return (int32_t)r;
}

// The exact bit count of one FIXED / LPC candidate of coded channel `code`; it replaces the channel's choice when
// strictly smaller.
template <class Par, class Src>
BRV_FE_HD void try_predictor(Par& par, Shared* sh, const Src& src, const Frame& f, int code, int kind, int order,
                             int tid, int nt) {
  const int bs = f.bs, width = coded_width(code, f.bps);
  const int pmax = max_porder(bs, order), fine = bs >> pmax, base = (1 << pmax) - 1;
  for (int e = tid; e < NODES*NK; e += nt) sh->sums[e] = 0;
  if (tid == 0) sh->overflow = 0;
  par.sync();
  {
    const int chunk = chunk_of(bs, nt);
    const int lo = tid*chunk > order ? tid*chunk : order, hi = (tid + 1)*chunk < bs ? (tid + 1)*chunk : bs;
    uint64_t acc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = 0;
    int part = lo < hi ? lo/fine : 0;
    bool fits = true;
    for (int i = lo; i < hi; ++i) {
      const int p = i/fine;
      if (p != part) {
#pragma unroll
        for (int k = 0; k < NK; ++k) { par.add64(&sh->sums[(base + part)*NK + k], acc[k]); acc[k] = 0; }
        part = p;
      }
      const uint32_t u = zigzag(residual_at(src, sh->lpc_q, sh->lpc_shift, code, kind, order, i, &fits));
#pragma unroll
      for (int k = 0; k < NK; ++k) acc[k] += u >> k;
    }
    if (lo < hi) {
#pragma unroll
      for (int k = 0; k < NK; ++k) par.add64(&sh->sums[(base + part)*NK + k], acc[k]);
    }
    if (!fits) par.or32(&sh->overflow, 1u);
  }
  par.sync();
  for (int p = pmax - 1; p >= 0; --p) {                     // the coarser levels: sums of their two halves
    const int at = (1 << p) - 1, below = (2 << p) - 1;
    for (int e = tid; e < (1 << p)*NK; e += nt) {
      const int j = e/NK, k = e - j*NK;
      sh->sums[(at + j)*NK + k] = sh->sums[(below + 2*j)*NK + k] + sh->sums[(below + 2*j + 1)*NK + k];
    }
    par.sync();
  }
  for (int node = tid; node < (2 << pmax) - 1; node += nt) { // per partition: the cheapest parameter of each width
    int p = 0;
    while ((2 << p) - 1 <= node) ++p;
    const int j = node - ((1 << p) - 1);
    const uint64_t count = (uint64_t)((bs >> p) - (j == 0 ? order : 0));
    uint64_t b4 = ~0ull, b5 = ~0ull;
    int k4 = 0, k5 = 0;
    for (int k = 0; k < NK; ++k) {
      const uint64_t c = sh->sums[node*NK + k] + count*(uint64_t)(k + 1);
      if (k <= 14 && c < b4) { b4 = c; k4 = k; }
      if (c < b5) { b5 = c; k5 = k; }
    }
    sh->best4[node] = b4; sh->best5[node] = b5; sh->k4[node] = k4; sh->k5[node] = k5;
  }
  par.sync();
  if (tid == 0 && !sh->overflow) {
    uint64_t best = ~0ull;
    int bp = 0, five = 0;
    for (int p = 0; p <= pmax; ++p) {
      uint64_t t4 = 0, t5 = 0;
      for (int j = 0; j < (1 << p); ++j) {
        t4 += 4 + sh->best4[(1 << p) - 1 + j];
        t5 += 5 + sh->best5[(1 << p) - 1 + j];
      }
      if (t4 < best) { best = t4; bp = p; five = 0; }
      if (t5 < best) { best = t5; bp = p; five = 1; }
    }
    const uint64_t bits = 8 + (uint64_t)(order*width) + (kind == KIND_LPC ? 9 + (uint64_t)(order*LPC_PRECISION) : 0) +
                          6 + best;
    ChannelChoice* c = &sh->choice[code];
    if (bits < c->bits) {
      c->bits = bits; c->kind = kind; c->order = order; c->porder = bp; c->five_bit = five;
      for (int j = 0; j < (1 << bp); ++j) c->k[j] = five ? sh->k5[(1 << bp) - 1 + j] : sh->k4[(1 << bp) - 1 + j];
      if (kind == KIND_LPC) {
        c->shift = sh->lpc_shift;
        for (int j = 0; j < order; ++j) c->coef[j] = sh->lpc_q[j];
      }
    }
  }
  par.sync();
}

// The choice of one coded channel: every candidate in the order of ties.
template <class Par, class Source>
BRV_FE_HD void choose_channel(Par& par, Shared* sh, const Source& source, const Frame& f, int code, int tid, int nt) {
  const int bs = f.bs, width = coded_width(code, f.bps);
  const Staged<Source> src = stage_channel(par, sh, source, code, bs, tid, nt);
  if (tid == 0) sh->differs = 0;
  par.sync();
  {
    const int32_t first = src.get(code, 0);
    bool differs = false;
    for (int i = tid; i < bs; i += nt) differs = differs || src.get(code, i) != first;
    if (differs) par.or32(&sh->differs, 1u);
  }
  par.sync();
  if (tid == 0) {
    ChannelChoice* c = &sh->choice[code];
    c->kind = KIND_VERBATIM; c->order = 0; c->porder = 0; c->five_bit = 0; c->shift = 0;
    c->bits = 8 + (uint64_t)bs*(uint64_t)width;
    c->value = src.get(code, 0);
    if (!sh->differs) { c->kind = KIND_CONSTANT; c->bits = 8 + (uint64_t)width; }
  }
  par.sync();
  for (int order = 0; order <= 4 && order < bs; ++order) try_predictor(par, sh, src, f, code, KIND_FIXED, order, tid, nt);
  int order = f.lpc_order < bs - 1 ? f.lpc_order : bs - 1;
  order = order > MAX_LPC ? MAX_LPC : order;
  if (order < 1) return;
  for (int l = tid; l <= order; l += nt) sh->lags[l] = 0;
  par.sync();
  {
    const int chunk = chunk_of(bs, nt);
    const int lo = tid*chunk, hi = (tid + 1)*chunk < bs ? (tid + 1)*chunk : bs;
    const uint32_t step = window_step(bs);
    for (int l = 0; l <= order; ++l) {
      int64_t acc = 0;
      for (int i = lo > l ? lo : l; i < hi; ++i)
        acc += (int64_t)windowed(src.get(code, i), width, i, step)*(int64_t)windowed(src.get(code, i - l), width, i - l, step);
      if (acc) par.add64((uint64_t*)&sh->lags[l], (uint64_t)acc);
    }
  }
  par.sync();
  if (tid == 0) {
    for (int l = 0; l <= order; ++l) sh->lpc_r[l] = (double)sh->lags[l];
    sh->lpc_ok = levinson(sh->lpc_r, order, sh->lpc_a) &&
                 quantise_coefficients(sh->lpc_a, order, sh->lpc_q, &sh->lpc_shift) ? 1 : 0;
  }
  par.sync();
  if (sh->lpc_ok) try_predictor(par, sh, src, f, code, KIND_LPC, order, tid, nt);
}

// The chosen subframe of coded channel `code` at bit `base` of the image.
template <class Par, class Source, class Img>
BRV_FE_HD void write_subframe(Par& par, Shared* sh, const Source& source, Img& img, const Frame& f, int code,
                              uint32_t base, int tid, int nt) {
  const Staged<Source> src = stage_channel(par, sh, source, code, f.bs, tid, nt);
  const ChannelChoice* c = &sh->choice[code];
  const int bs = f.bs, width = coded_width(code, f.bps), kind = c->kind, order = c->order;
  bool ok = true;
  if (tid == 0) {
    const int type = kind == KIND_CONSTANT ? 0 : kind == KIND_VERBATIM ? 1 : kind == KIND_FIXED ? 8 + order : 31 + order;
    ok = put_bits(img, base, (uint32_t)type << 1, 8) && ok;
    if (kind == KIND_CONSTANT) ok = put_bits(img, base + 8, (uint32_t)c->value, width) && ok;
  }
  if (kind == KIND_VERBATIM)
    for (int i = tid; i < bs; i += nt) ok = put_bits(img, base + 8 + (uint32_t)(i*width), (uint32_t)src.get(code, i), width) && ok;
  if (kind == KIND_FIXED || kind == KIND_LPC) {
    for (int i = tid; i < order; i += nt) ok = put_bits(img, base + 8 + (uint32_t)(i*width), (uint32_t)src.get(code, i), width) && ok;
    uint32_t at = base + 8 + (uint32_t)(order*width);
    if (kind == KIND_LPC) {
      if (tid == 0) {
        ok = put_bits(img, at, LPC_PRECISION - 1, 4) && ok;
        ok = put_bits(img, at + 4, (uint32_t)c->shift, 5) && ok;
      }
      for (int j = tid; j < order; j += nt) ok = put_bits(img, at + 9 + (uint32_t)(j*LPC_PRECISION), (uint32_t)c->coef[j], LPC_PRECISION) && ok;
      at += 9 + (uint32_t)(order*LPC_PRECISION);
    }
    const int pbits = c->five_bit ? 5 : 4, psize = bs >> c->porder;
    if (tid == 0) ok = put_bits(img, at, ((uint32_t)c->five_bit << 4) | (uint32_t)c->porder, 6) && ok;
    at += 6;
    // the codes' places: an exclusive scan of their lengths, a contiguous run of residuals per thread
    const int chunk = chunk_of(bs - order, nt);
    const int lo = order + tid*chunk, hi = lo + chunk < bs ? lo + chunk : bs;
    bool fits = true;
    uint32_t mine = 0;
    for (int i = lo; i < hi; ++i)
      mine += rice_length(zigzag(residual_at(src, c->coef, c->shift, code, kind, order, i, &fits)), c->k[i/psize]);
    sh->scan[0][tid] = mine;
    par.sync();
    int cur = 0;
    for (int d = 1; d < nt; d <<= 1) {
      sh->scan[cur ^ 1][tid] = sh->scan[cur][tid] + (tid >= d ? sh->scan[cur][tid - d] : 0u);
      cur ^= 1;
      par.sync();
    }
    uint32_t prefix = sh->scan[cur][tid] - mine;
    par.sync();                                             // the next subframe's scan writes the same words
    for (int i = lo; i < hi; ++i) {
      const int part = i/psize, k = c->k[part];
      if (i == (part == 0 ? order : part*psize)) ok = put_bits(img, at + (uint32_t)(part*pbits) + prefix, (uint32_t)k, pbits) && ok;
      const uint32_t u = zigzag(residual_at(src, c->coef, c->shift, code, kind, order, i, &fits));
      // the zeros of the unary run are there already: the stop bit and the remainder, k + 1 <= 31 bits
      ok = put_bits(img, at + (uint32_t)((part + 1)*pbits) + prefix + (u >> k), (1u << k) | (u & ((1u << k) - 1u)), k + 1) && ok;
      prefix += rice_length(u, k);
    }
  }
  if (!ok) par.or32(&sh->bad_put, 1u);
}

// One frame into the image. Returns its length in bytes (the same value on every thread), 0 when the image's
// capacity would not hold it (frame_capacity() excludes that). The row's ROW_* bits of the frame's samples go to
// *row_flags (every thread gets them).
template <class Par, class Src, class Img>
BRV_FE_HD uint32_t encode_frame(Par& par, Shared* sh, const Src& src, Img& img, const Frame& f, int tid, int nt,
                                uint32_t* row_flags) {
  const int bs = f.bs;
  if (tid == 0) { sh->flags = 0; sh->bad_put = 0; sh->crc = 0; }
  par.sync();
  {
    uint32_t flags = 0;
    for (int c = 0; c < f.channels; ++c)
      for (int i = tid; i < bs; i += nt) flags |= (uint32_t)src.flags(c, i);
    if (flags) par.or32(&sh->flags, flags);
  }
  const int ncoded = f.channels == 2 ? 4 : 1;
  for (int code = 0; code < ncoded; ++code) choose_channel(par, sh, src, f, code, tid, nt);
  par.sync();
  if (tid == 0) {
    int assignment = 0, a = 0, b = -1;
    if (f.channels == 2) {
      const uint64_t l = sh->choice[0].bits, r = sh->choice[1].bits, m = sh->choice[2].bits, s = sh->choice[3].bits;
      uint64_t best = l + r;
      assignment = 1; a = 0; b = 1;
      if (l + s < best) { best = l + s; assignment = 8; a = 0; b = 3; }
      if (s + r < best) { best = s + r; assignment = 9; a = 3; b = 1; }
      if (m + s < best) { best = m + s; assignment = 10; a = 2; b = 3; }
    }
    sh->assignment = assignment;
    sh->sub_code[0] = a; sh->sub_code[1] = b;
    sh->header_bytes = (uint32_t)frame_header(sh->header, bs, f.rate, assignment, f.bps, f.number);
    sh->sub_base[0] = 8*sh->header_bytes;
    sh->sub_base[1] = sh->sub_base[0] + (uint32_t)sh->choice[a].bits;
    const uint64_t bits = (uint64_t)sh->sub_base[1] + (b >= 0 ? sh->choice[b].bits : 0);
    // the words the frame takes and one more (put_bits looks one word ahead) have to lie inside the image
    sh->total_bits = (bits + 7)/8*8 + 16 + 64 <= 32ull*img.words() ? (uint32_t)((bits + 7)/8*8) : 0u;
  }
  par.sync();
  *row_flags = sh->flags;
  const uint32_t body_bits = sh->total_bits;                // up to the CRC-16, padded to the byte
  if (body_bits == 0) return 0;
  const uint32_t body = body_bits/8, nwords = (body_bits + 16 + 31)/32 + 1;
  for (uint32_t w = (uint32_t)tid; w < nwords; w += (uint32_t)nt) img.zero(w);
  par.publish();
  par.sync();
  if (tid == 0)
    for (uint32_t i = 0; i < sh->header_bytes; ++i) put_bits(img, 8*i, sh->header[i], 8);
  write_subframe(par, sh, src, img, f, sh->sub_code[0], sh->sub_base[0], tid, nt);
  if (sh->sub_code[1] >= 0) write_subframe(par, sh, src, img, f, sh->sub_code[1], sh->sub_base[1], tid, nt);
  par.publish();
  par.sync();
  {                                                         // CRC-16: a run of bytes per thread, shifted to its place
    const uint32_t chunk = (body + (uint32_t)nt - 1)/(uint32_t)nt;
    const uint32_t lo = (uint32_t)tid*chunk, hi = lo + chunk < body ? lo + chunk : body;
    if (lo < hi) {
      uint32_t c = 0;
      for (uint32_t at = lo; at < hi; ++at) c = crc16_byte(c, image_byte(img, at));
      par.xor32(&sh->crc, crc16_mul(c, crc16_shift(body - hi)));
    }
  }
  par.sync();
  if (tid == 0) put_bits(img, body_bits, sh->crc, 16);
  par.publish();
  par.sync();
  return sh->bad_put ? 0u : body + 2;
}

}  // namespace brv_flacenc
