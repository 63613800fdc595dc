// The decode core of libbrever_flac.so (include/brever_flac.h): subframe parser, Rice reader and predictors of
// RFC 9639 as __host__ __device__ code over two small types the caller supplies, so that the kernel
// (flacdec.hip), the host index's diagnosis (flacdec.hip) and the stand-alone host check
// (tools/flac_core_check.cpp) run the very same code.
//
//   Words   load(i): the i-th aligned little-endian dword of the buffer the frame lies in
//   Sink    channel(c): subframe c begins;  put(i, v): sample i of the subframe (wasted bits shifted back in);
//           hset(i, v) / hget(i): a ring of the last 32 samples (LPC history, unshifted);
//           cset(j, c) / cget(j): the up to 32 LPC coefficients
//
// The history and the coefficients live behind the sink because a runtime-indexed register array would go to
// scratch memory on the GPU: the kernel keeps both in LDS. The FIXED predictors use four scalars and no ring.
//
// Nothing here can run off the rails on a damaged frame: a read never loads a dword at or beyond
// (offset + length + 3)/4, `left` counts the frame's bits down and every loop leaves when it turns negative or is
// bounded by the block size, arithmetic on sample values wraps (unsigned), shift counts are range-checked. What
// comes out for a damaged frame is a status, and samples nobody reads.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define BRV_FD_HD __host__ __device__ __forceinline__
#else
#define BRV_FD_HD inline
#endif

namespace brv_flacdec {

// per-job status words (include/brever_flac.h: BRV_FLACDEC_JOB_*)
enum { ST_OK = 0, ST_BAD_FIELDS = 1, ST_RESERVED = 2, ST_OVERRUN = 3, ST_LENGTH = 4 };

// MSB-first reader of one frame: a 64-bit window whose top `have` bits are valid (the rest are zero), refilled
// with aligned dword loads. The loads run two dwords ahead of the window (a0, a1): the bits of a frame are one
// dependent chain, and a load issued only when the window runs dry would put a memory latency into it every 32 bits.
template <class Words>
struct BitReader {
  Words w;
  uint64_t next, limit;      // dword index of the next load; loads at and beyond limit give zeros
  uint64_t window;
  uint32_t a0, a1;           // the dwords at next and next + 1, already loaded
  int have;
  int32_t left;              // bits of the frame not yet consumed; negative: the frame's bits ran out

  // byte_len <= 2^27
  BRV_FD_HD void init(Words words, uint64_t byte_off, int32_t byte_len) {
    w = words;
    next = byte_off >> 2;
    limit = (byte_off + (uint64_t)byte_len + 3) >> 2;
    window = 0; have = 0; left = byte_len*8;
    a0 = fetch(next); a1 = fetch(next + 1);
    const int skip = (int)(byte_off & 3)*8;
    if (skip) { refill(); window <<= skip; have -= skip; }
  }
  BRV_FD_HD uint32_t fetch(uint64_t i) const { return i < limit ? w.load(i) : 0u; }
  BRV_FD_HD void refill() {                               // afterwards have > 32
    while (have <= 32) {
      const uint32_t v = __builtin_bswap32(a0);
      a0 = a1; a1 = fetch(next + 2);
      ++next;
      window |= (uint64_t)v << (32 - have);
      have += 32;
    }
  }
  BRV_FD_HD uint32_t read(int n) {                        // 0 <= n <= 32
    if (n <= 0) return 0;
    refill();
    const uint32_t v = (uint32_t)(window >> (64 - n));
    window <<= n; have -= n; left -= n;
    return v;
  }
  BRV_FD_HD int32_t read_signed(int n) {                  // 0 <= n <= 32
    if (n <= 0) return 0;
    const uint32_t v = read(n), sign = 1u << (n - 1);
    return (int32_t)((v ^ sign) - sign);
  }
  // zeros before the next 1; runs longer than the window take one turn per refill, and the loop leaves when
  // the frame's bits are used up
  BRV_FD_HD uint32_t unary() {
    uint32_t q = 0;
    for (;;) {
      refill();
      if (window == 0) {
        q += (uint32_t)have; left -= have; have = 0;
        if (left < 0) return q;
        continue;
      }
      const int lz = __builtin_clzll(window);             // < have: the bits below `have` are zero
      q += (uint32_t)lz;
      window <<= lz; window <<= 1;
      have -= lz + 1; left -= lz + 1;
      return q;
    }
  }
  BRV_FD_HD void skip_bytes(int n) { for (; n >= 4; n -= 4) read(32); read(8*n); }
  BRV_FD_HD void align() { if (left > 0) read(left & 7); }
};

// Partitioned Rice residual of a subframe: emit(r) is called bs - order times unless a status comes back.
template <class R, class F>
BRV_FD_HD int residual(R& br, int bs, int order, F emit) {
  const int method = (int)br.read(2);
  if (method > 1) return ST_RESERVED;
  const int pbits = 4 + method, esc = (1 << pbits) - 1;
  const int porder = (int)br.read(4);
  if (porder > 0 && ((bs >> porder) << porder) != bs) return ST_RESERVED;
  for (int part = 0; part < (1 << porder); ++part) {
    const int count = (bs >> porder) - (part == 0 ? order : 0);
    if (count < 0) return ST_RESERVED;
    const int k = (int)br.read(pbits);
    if (k == esc) {
      const int nb = (int)br.read(5);
      for (int i = 0; i < count; ++i) {
        emit(br.read_signed(nb));
        if (br.left < 0) return ST_OVERRUN;
      }
    } else {
      for (int i = 0; i < count; ++i) {
        const uint32_t q = br.unary();
        const uint32_t u = (q << k) | br.read(k);
        emit((int32_t)((u >> 1) ^ (0u - (u & 1u))));
        if (br.left < 0) return ST_OVERRUN;
      }
    }
    if (br.left < 0) return ST_OVERRUN;
  }
  return ST_OK;
}

// One subframe of bs samples, bps bits each (4 ... 25), into the sink.
template <class R, class S>
BRV_FD_HD int subframe(R& br, S& s, int bs, int bps) {
  if (br.read(1)) return ST_RESERVED;                     // padding bit
  const int type = (int)br.read(6);
  uint32_t wasted = 0;
  if (br.read(1)) wasted = br.unary() + 1u;
  if (br.left < 0) return ST_OVERRUN;
  if (wasted >= (uint32_t)bps) return ST_RESERVED;
  bps -= (int)wasted;
  if (type == 0) {                                        // CONSTANT
    const uint32_t v = (uint32_t)br.read_signed(bps) << wasted;
    for (int i = 0; i < bs; ++i) s.put(i, (int32_t)v);
  } else if (type == 1) {                                 // VERBATIM
    for (int i = 0; i < bs; ++i) {
      s.put(i, (int32_t)((uint32_t)br.read_signed(bps) << wasted));
      if (br.left < 0) return ST_OVERRUN;
    }
  } else if (type >= 8 && type <= 12) {                   // FIXED, order type - 8
    const int order = type - 8;
    if (order > bs) return ST_RESERVED;
    uint32_t h1 = 0, h2 = 0, h3 = 0, h4 = 0;              // the last four samples, newest first
    for (int i = 0; i < order; ++i) {
      const uint32_t v = (uint32_t)br.read_signed(bps);
      s.put(i, (int32_t)(v << wasted));
      h4 = h3; h3 = h2; h2 = h1; h1 = v;
    }
    if (br.left < 0) return ST_OVERRUN;
    // coefficients of the order as scalars: (1), (2, -1), (3, -3, 1), (4, -6, 4, -1)
    const uint32_t c1 = (uint32_t)order;
    const uint32_t c2 = order == 2 ? 0u - 1u : order == 3 ? 0u - 3u : order == 4 ? 0u - 6u : 0u;
    const uint32_t c3 = order == 3 ? 1u : order == 4 ? 4u : 0u;
    const uint32_t c4 = order == 4 ? 0u - 1u : 0u;
    int i = order;
    const int r = residual(br, bs, order, [&](int32_t res) {
      const uint32_t v = c1*h1 + c2*h2 + c3*h3 + c4*h4 + (uint32_t)res;
      s.put(i, (int32_t)(v << wasted));
      h4 = h3; h3 = h2; h2 = h1; h1 = v;
      ++i;
    });
    if (r) return r;
  } else if (type >= 32) {                                // LPC, order type - 31
    const int order = type - 31;
    if (order > bs) return ST_RESERVED;
    for (int i = 0; i < order; ++i) {
      const int32_t v = br.read_signed(bps);
      s.put(i, (int32_t)((uint32_t)v << wasted));
      s.hset(i, v);
    }
    const int precision = (int)br.read(4) + 1;
    if (precision == 16) return ST_RESERVED;
    const int shift = br.read_signed(5);
    if (shift < 0) return ST_RESERVED;
    for (int j = 0; j < order; ++j) s.cset(j, br.read_signed(precision));
    if (br.left < 0) return ST_OVERRUN;
    int i = order;
    // exact: 25-bit samples times 15-bit coefficients over 32 taps need 45 bits, so the sum is 64 bits wide
    const int r = residual(br, bs, order, [&](int32_t res) {
      uint64_t acc = 0;
      for (int j = 0; j < order; ++j) acc += (uint64_t)((int64_t)s.cget(j)*(int64_t)s.hget(i - 1 - j));
      const uint32_t v = (uint32_t)(uint64_t)((int64_t)acc >> shift) + (uint32_t)res;
      s.put(i, (int32_t)(v << wasted));
      s.hset(i, (int32_t)v);
      ++i;
    });
    if (r) return r;
  } else {
    return ST_RESERVED;                                   // reserved subframe type
  }
  return br.left < 0 ? ST_OVERRUN : ST_OK;
}

BRV_FD_HD int channels_of(int assignment) { return assignment < 8 ? assignment + 1 : 2; }

// The subframes of a frame whose header (header_bytes, CRC-8 included) the index has read. The reader stands at
// the frame's first byte. ST_LENGTH unless the frame ends, after the padding, 16 bits (the CRC-16) before its
// stated length.
template <class R, class S>
BRV_FD_HD int frame(R& br, S& s, int header_bytes, int bs, int assignment, int bps) {
  br.skip_bytes(header_bytes);
  const int nch = channels_of(assignment);
  for (int c = 0; c < nch; ++c) {
    const bool side = (assignment == 8 && c == 1) || (assignment == 9 && c == 0) || (assignment == 10 && c == 1);
    s.channel(c);
    const int r = subframe(br, s, bs, bps + (side ? 1 : 0));
    if (r) return r;
  }
  br.align();
  if (br.left < 0) return ST_OVERRUN;
  return br.left == 16 ? ST_OK : ST_LENGTH;
}

// Sample of channel c from the two subframe values a (subframe 0) and b (subframe 1) of a stereo frame; for
// independent channels the caller passes the channel's own value as a.
BRV_FD_HD int32_t decorrelate(int assignment, int c, int32_t a, int32_t b) {
  const uint32_t ua = (uint32_t)a, ub = (uint32_t)b;
  if (assignment == 8) return c == 0 ? a : (int32_t)(ua - ub);          // left, side
  if (assignment == 9) return c == 0 ? (int32_t)(ua + ub) : b;          // side, right
  if (assignment == 10) {                                               // mid, side: the mid's LSB is the side's
    const uint32_t mid = (ua << 1) | (ub & 1u);
    return (int32_t)(c == 0 ? mid + ub : mid - ub) >> 1;
  }
  return a;
}

// v 2^-(bps - 1): exact in float for the up to 24-bit samples, the value (float)((double)v/2^(bps-1)) of the
// host decoder
BRV_FD_HD float scale_sample(int32_t v, int bps) {
  union { uint32_t u; float f; } s;
  s.u = (uint32_t)(127 - (bps - 1)) << 23;
  return (float)v*s.f;
}

}  // namespace brv_flacdec
