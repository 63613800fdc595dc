// Stand-alone host check of the GPU FLAC encoder's core (brever_amd/csrc/flacenc/flacenc_core.h): the very code
// the kernel runs, here with one thread, over a deterministic corpus built here; every frame is decoded again with the
// decoder's core (brever_amd/csrc/flacdec/flacdec_core.h) and compared. Meant to be built with
// -fsanitize=address,undefined and run directly:
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined tools/flac_enc_check.cpp -o flac_enc_check
//   ./flac_enc_check                                     the corpus: exit 0 and a count, or a message and exit 1
//   ./flac_enc_check encode PCM C BPS BLOCK LPC RATE OUT  PCM holds int32 samples, channel after channel; OUT gets
//                                                        the FLAC stream the core writes for them
//
// The corpus: 16 and 24 bits, mono and stereo, block sizes 16 ... 4500 (one longer than the samples the core
// stages) with short last blocks and blocks shorter than the predictor orders, silence, constants, full-scale noise,
// ramps, resonances, tones, equal and anti-phase channels, frame numbers of one to six coded bytes, LPC on and off.
// The source and the image below check every index, and the image is a heap block of the exact capacity, so the
// sanitizers see what the checks would miss.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../brever_amd/csrc/flacdec/flacdec_core.h"
#include "../brever_amd/csrc/flacenc/flacenc_core.h"

namespace fd = brv_flacdec;
namespace fe = brv_flacenc;

static std::string g_where;                                  // the frame being encoded, for messages from the types below

static void die(const std::string& what) {
  fprintf(stderr, "flac_enc_check: %s%s%s\n", g_where.c_str(), g_where.empty() ? "" : ": ", what.c_str());
  exit(1);
}

// ---- the three types the encode core is written over ---------------------------------------------------------------
struct HostSrc {
  const int32_t* left; const int32_t* right; int bs, bps;
  int32_t get(int code, int i) const {
    if (i < 0 || i >= bs) die("sample load at " + std::to_string(i) + " of " + std::to_string(bs));
    if (code != 0 && !right) die("coded channel " + std::to_string(code) + " of a mono frame");
    return fe::coded_channel(code, left[i], right ? right[i] : 0);
  }
  int flags(int c, int i) const {
    if (i < 0 || i >= bs || c < 0 || c > (right ? 1 : 0)) die("flags index");
    return fe::pcm_flags(c ? right[i] : left[i], bps);
  }
};

struct HostImg {
  uint32_t* p; uint32_t n;
  uint32_t words() const { return n; }
  void at(uint32_t w) const { if (w >= n) die("image word " + std::to_string(w) + " of " + std::to_string(n)); }
  void zero(uint32_t w) { at(w); p[w] = 0; }
  void orw(uint32_t w, uint32_t v) {
    at(w);
    if (p[w] & v) die("a bit of word " + std::to_string(w) + " written twice");
    p[w] |= v;
  }
  uint32_t load(uint32_t w) const { at(w); return p[w]; }
};

struct HostPar {
  void sync() {}
  void publish() {}
  void add64(uint64_t* p, uint64_t v) { *p += v; }
  void or32(uint32_t* p, uint32_t v) { *p |= v; }
  void xor32(uint32_t* p, uint32_t v) { *p ^= v; }
};

// ---- the decoder's two types -----------------------------------------------------------------------------------------
struct Words {
  const uint32_t* p; uint64_t n;
  uint32_t load(uint64_t i) const { if (i >= n) die("decoder load beyond the frame"); return p[i]; }
};
struct Sink {
  int bs, cur;
  std::vector<std::vector<int32_t>> chan;
  int32_t ring[32], coef[32];
  Sink(int blocksize, int channels) : bs(blocksize), cur(0), chan((size_t)channels) {
    for (auto& c : chan) c.assign((size_t)blocksize, 0);
    memset(ring, 0, sizeof ring); memset(coef, 0, sizeof coef);
  }
  void channel(int c) { cur = c; }
  void put(int i, int32_t v) { if (i < 0 || i >= bs) die("decoder store beyond the block"); chan[(size_t)cur][(size_t)i] = v; }
  void hset(int i, int32_t v) { ring[i & 31] = v; }
  int32_t hget(int i) const { return ring[i & 31]; }
  void cset(int j, int32_t c) { coef[j & 31] = c; }
  int32_t cget(int j) const { return coef[j & 31]; }
};

static uint32_t crc(const uint8_t* d, size_t n, uint32_t poly, int width) {
  const uint32_t top = 1u << (width - 1), mask = width == 16 ? 0xffffu : 0xffu;
  uint32_t c = 0;
  for (size_t k = 0; k < n; ++k) {
    c ^= (uint32_t)d[k] << (width - 8);
    for (int i = 0; i < 8; ++i) c = (c & top) ? ((c << 1) ^ poly) & mask : (c << 1) & mask;
  }
  return c;
}

// One frame with the core; its bytes. Checks header, CRCs and the samples that come back.
static std::vector<uint8_t> encode_frame(const int32_t* left, const int32_t* right, int bs, int bps, int rate,
                                         int lpc, int64_t number, const std::string& tag) {
  const int channels = right ? 2 : 1;
  g_where = tag;
  // the capacity of the frame's own size (the kernel's is that of the nominal block size, never smaller)
  const int64_t cap = fe::frame_capacity(channels, bps, bs);
  uint32_t* block = (uint32_t*)malloc((size_t)cap);
  memset(block, 0xa5, (size_t)cap);                          // the core zeroes what it writes into
  fe::Shared* sh = new fe::Shared;
  HostSrc src{left, right, bs, bps};
  HostImg img{block, (uint32_t)(cap/4)};
  HostPar par;
  fe::Frame f{bs, channels, bps, rate, lpc, number};
  uint32_t flags = 0;
  const uint32_t n = fe::encode_frame(par, sh, src, img, f, 0, 1, &flags);
  if (flags) die(tag + ": flags " + std::to_string(flags));
  if (n < 8 || n > (uint32_t)cap) die(tag + ": frame of " + std::to_string(n) + " bytes");
  const uint8_t* bytes = (const uint8_t*)block;
  std::vector<uint8_t> out(bytes, bytes + n);
  const int hdr = (int)sh->header_bytes, assignment = sh->assignment;
  delete sh;
  // both CRCs, by the plain bitwise definition
  if (crc(out.data(), (size_t)hdr - 1, 0x07, 8) != out[(size_t)hdr - 1]) die(tag + ": CRC-8");
  if (crc(out.data(), n - 2, 0x8005, 16) != (((uint32_t)out[n - 2] << 8) | out[n - 1])) die(tag + ": CRC-16");
  if (out[0] != 0xff || out[1] != 0xf8 || (out[3] >> 4) != assignment) die(tag + ": header bytes");
  // the decoder's core reads the frame at dword granularity from the block
  fd::BitReader<Words> br;
  br.init(Words{block, (uint64_t)cap/4}, 0, (int32_t)n);
  Sink sink(bs, channels);
  const int st = fd::frame(br, sink, hdr, bs, assignment, bps);
  if (st != fd::ST_OK) die(tag + ": the decoder's core gives status " + std::to_string(st));
  for (int c = 0; c < channels; ++c)
    for (int i = 0; i < bs; ++i) {
      const int32_t a = sink.chan[assignment >= 8 ? 0 : (size_t)c][(size_t)i];
      const int32_t b = assignment >= 8 ? sink.chan[1][(size_t)i] : 0;
      const int32_t got = fd::decorrelate(assignment, c, a, b), want = c ? right[i] : left[i];
      if (got != want)
        die(tag + ": channel " + std::to_string(c) + " sample " + std::to_string(i) + ": " + std::to_string(got) +
            " != " + std::to_string(want));
    }
  free(block);
  return out;
}

static std::vector<uint8_t> encode_stream(const std::vector<int32_t>& pcm, int channels, int bps, int block, int lpc,
                                          int rate, const std::string& tag, long* frames) {
  const size_t len = pcm.size()/(size_t)channels;
  std::vector<uint8_t> out(fe::STREAM_HEADER_BYTES, 0);
  uint32_t least = ~0u, most = 0;
  int64_t number = 0;
  for (size_t start = 0; start < len; start += (size_t)block, ++number) {
    const int bs = (int)(len - start < (size_t)block ? len - start : (size_t)block);
    const std::vector<uint8_t> fr = encode_frame(pcm.data() + start, channels == 2 ? pcm.data() + len + start : nullptr,
                                                 bs, bps, rate, lpc, number, tag + " frame " + std::to_string(number));
    least = fr.size() < least ? (uint32_t)fr.size() : least;
    most = fr.size() > most ? (uint32_t)fr.size() : most;
    out.insert(out.end(), fr.begin(), fr.end());
    if (frames) ++*frames;
  }
  fe::stream_header(out.data(), block, least, most, rate, channels, bps, (int64_t)len);
  return out;
}

static uint32_t g_seed = 2024;
static uint32_t rnd() { g_seed = g_seed*1664525u + 1013904223u; return g_seed >> 8; }

// kind: 0 silence, 1 constant, 2 full-scale noise, 3 ramp, 4 resonance (AR(2)), 5 two tones, 6 both range ends,
// 7 small noise
static std::vector<int32_t> signal(int kind, size_t n, int bps, int variant) {
  const int64_t top = (1ll << (bps - 1)) - 1, bottom = -(1ll << (bps - 1));
  std::vector<int32_t> x(n);
  double y1 = 0, y2 = 0;
  for (size_t i = 0; i < n; ++i) {
    int64_t v = 0;
    switch (kind) {
      case 0: v = 0; break;
      case 1: v = variant ? bottom : top/3; break;
      case 2: v = bottom + (int64_t)(((uint64_t)rnd() << 8 ^ rnd()) % (uint64_t)(top - bottom + 1)); break;
      case 3: v = (int64_t)i*(variant ? -37 : 5) + 11; break;
      case 4: {
        const double e = ((double)(rnd() % 2001) - 1000.0)*(double)top/40000.0;
        const double y = 1.2*y1 - 0.9*y2 + e;               // a resonance near a tenth of the rate
        y2 = y1; y1 = y; v = (int64_t)y; break;
      }
      case 5: v = (int64_t)((double)top*(0.4*sin(2*M_PI*5000*(double)i/16000) + 0.3*sin(2*M_PI*6500*(double)i/16000 + 1))); break;
      case 6: v = (i + (size_t)variant) & 1 ? top : bottom; break;
      default: v = (int64_t)(rnd() % 7) - 3; break;
    }
    x[i] = (int32_t)(v > top ? top : v < bottom ? bottom : v);
  }
  return x;
}

static int run_corpus() {
  long frames = 0, streams = 0;
  const int blocks[] = {16, 17, 64, 192, 256, 1000, 4096, 4500};   // 4500: beyond the samples the core stages
  for (int bps : {16, 24})
    for (int channels : {1, 2})
      for (int block : blocks)
        for (int kind = 0; kind < 8; ++kind) {
          const size_t lens[] = {1, 3, 15, (size_t)block, (size_t)block*2 + 5};
          for (size_t len : lens) {
            if (block >= 4096 && (kind == 2 || kind == 7) && len > 4096) continue;     // keep the run short
            std::vector<int32_t> pcm = signal(kind, len, bps, 0);
            if (channels == 2) {
              // the right channel: equal, anti-phase, or a signal of its own
              std::vector<int32_t> r = kind % 3 == 0 ? pcm : kind % 3 == 1 ? signal(kind, len, bps, 1) : pcm;
              if (kind % 3 == 2) for (auto& v : r) v = v == -(1 << (bps - 1)) ? (1 << (bps - 1)) - 1 : -v;
              pcm.insert(pcm.end(), r.begin(), r.end());
            }
            for (int lpc : {0, 8, 32}) {
              if (lpc == 32 && block > 256) continue;
              const std::string tag = std::to_string(bps) + " bits, " + std::to_string(channels) + " ch, block " +
                                      std::to_string(block) + ", kind " + std::to_string(kind) + ", " +
                                      std::to_string(len) + " samples, lpc " + std::to_string(lpc);
              encode_stream(pcm, channels, bps, block, lpc, 16000, tag, &frames);
              ++streams;
            }
          }
        }
  // frame numbers of one to four coded bytes, a rate without a code, a block size with a code of its own
  const std::vector<int32_t> one = signal(4, 576, 16, 0);
  for (int64_t number : {0ll, 127ll, 128ll, 2047ll, 2048ll, 65535ll, 65536ll, 2097151ll, 2097152ll, 2147483647ll}) {
    encode_frame(one.data(), nullptr, 576, 16, 12345, 8, number, "frame number " + std::to_string(number));
    ++frames;
  }
  printf("flac_enc_check: %ld frames of %ld streams ok\n", frames, streams);
  return 0;
}

static int run_encode(char** a) {
  FILE* fp = fopen(a[0], "rb");
  if (!fp) die(std::string("cannot open ") + a[0]);
  std::vector<int32_t> pcm;
  int32_t buf[4096];
  size_t n;
  while ((n = fread(buf, 4, 4096, fp)) > 0) pcm.insert(pcm.end(), buf, buf + n);
  fclose(fp);
  const int channels = atoi(a[1]), bps = atoi(a[2]), block = atoi(a[3]), lpc = atoi(a[4]), rate = atoi(a[5]);
  if ((channels != 1 && channels != 2) || (bps != 16 && bps != 24) || block < 16 || block > 65535 || lpc < 0 ||
      lpc > fe::MAX_LPC || rate < 1 || pcm.empty() || pcm.size() % (size_t)channels)
    die("encode: arguments out of range");
  for (int32_t v : pcm) if (fe::pcm_flags(v, bps)) die("encode: a sample out of range");
  const std::vector<uint8_t> out = encode_stream(pcm, channels, bps, block, lpc, rate, a[0], nullptr);
  fp = fopen(a[6], "wb");
  if (!fp) die(std::string("cannot write ") + a[6]);
  fwrite(out.data(), 1, out.size(), fp);
  fclose(fp);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 9 && !strcmp(argv[1], "encode")) return run_encode(argv + 2);
  if (argc != 1) die("usage: flac_enc_check | flac_enc_check encode PCM C BPS BLOCK LPC RATE OUT");
  return run_corpus();
}
