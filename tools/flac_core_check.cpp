// Stand-alone host check of the GPU FLAC decoder's core (brever_amd/csrc/flacdec/flacdec_core.h): the very code the
// kernel runs, on the CPU, over a deterministic corpus built here. Meant to be built with
// -fsanitize=address,undefined and run directly:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/flac_core_check.cpp -o flac_core_check
//   ./flac_core_check                                   the corpus: exit 0 and a count, or a message and exit 1
//   ./flac_core_check decode STREAM FRAMES OUT          decode the frames of a stream with the core: FRAMES is the
//                                                       int64 table of brv_flacdec_index, OUT gets interleaved int32
//
// The corpus: valid frames of every subframe kind (CONSTANT, VERBATIM, FIXED 0-4, LPC 1-32; wasted bits; 4- and
// 5-bit Rice parameters; escape partitions, a 0-bit one among them; all stereo decorrelations; 8 channels; 8-24
// bits; long unary runs), each placed at byte offsets 0-3 of a buffer that ends with the frame, then
//   - decoded: status 0 and the samples that went in;
//   - truncated at every byte: a non-zero status; and the same with the frame table still claiming the original
//     length (zeros where the bytes were): a status, whatever it is;
//   - with every single bit flipped (subframe headers, warm-up, LPC precision / shift / coefficients, Rice method,
//     partition order, parameters and escape widths among them) while the frame table still claims the original
//     length: a status, whatever it is.
// In every case the core must stay inside the buffers it was given: the word source and the sink below check every
// index, and the buffers are heap blocks of the exact size, so the sanitizers see what the checks would miss.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../brever_amd/csrc/flacdec/flacdec_core.h"

namespace fd = brv_flacdec;

static void die(const std::string& what) {
  fprintf(stderr, "flac_core_check: %s\n", what.c_str());
  exit(1);
}

// ---- the two types the core is written over, with every index checked ----------------------------------------------
struct CheckedWords {
  const uint32_t* p; uint64_t n;
  uint32_t load(uint64_t i) const {
    if (i >= n) die("dword load at " + std::to_string(i) + " of " + std::to_string(n));
    return p[i];
  }
};

struct CheckedSink {
  int bs, nch, cur;
  std::vector<std::vector<int32_t>> chan;
  int32_t ring[32], coef[32];
  CheckedSink(int blocksize, int channels) : bs(blocksize), nch(channels), cur(0), chan(channels) {
    for (auto& c : chan) c.assign((size_t)blocksize, 0);
    memset(ring, 0, sizeof ring); memset(coef, 0, sizeof coef);
  }
  void channel(int c) { if (c < 0 || c >= nch) die("channel " + std::to_string(c)); cur = c; }
  void put(int i, int32_t v) {
    if (i < 0 || i >= bs) die("sample store at " + std::to_string(i) + " of " + std::to_string(bs));
    chan[(size_t)cur][(size_t)i] = v;
  }
  void hset(int i, int32_t v) { if (i < 0) die("history index"); ring[i & 31] = v; }
  int32_t hget(int i) const { if (i < 0) die("history index"); return ring[i & 31]; }
  void cset(int j, int32_t c) { if (j < 0 || j > 31) die("coefficient index"); coef[j] = c; }
  int32_t cget(int j) const { if (j < 0 || j > 31) die("coefficient index"); return coef[j]; }
};

struct Frame {                    // what the index records of a frame
  std::vector<uint8_t> bytes;
  int header, bs, assignment, bps;
};

// The frame's first `avail` bytes at byte offset `shift` of an exact heap block, handed to the core as a frame of
// `claimed` bytes; returns the core's status. With claimed > avail (the frame table still claims the original length
// of a cut frame) the block is padded with zeros up to the claimed length, as the uploaded blob would hold other
// bytes there.
static int decode(const Frame& f, size_t avail, int32_t claimed, int shift, CheckedSink& sink) {
  const size_t hold = avail > (size_t)claimed ? avail : (size_t)claimed;
  const size_t total = ((size_t)shift + hold + 3)/4*4;
  // the block ends with the (rounded up) frame: a load beyond it is a heap overflow
  uint32_t* block = (uint32_t*)malloc(total);
  memset(block, 0, total);
  memcpy((uint8_t*)block + shift, f.bytes.data(), avail);
  fd::BitReader<CheckedWords> br;
  // the reader may load up to (shift + claimed + 3)/4 dwords; the checked source refuses what the block does not hold
  br.init(CheckedWords{block, total/4}, (uint64_t)shift, claimed);
  const int st = fd::frame(br, sink, f.header, f.bs, f.assignment, f.bps);
  free(block);
  return st;
}

// ---- a small encoder ---------------------------------------------------------------------------------------------------
struct BitWriter {
  std::vector<uint8_t> out; uint64_t acc = 0; int n = 0;
  void write(uint64_t v, int bits) {
    for (int b = bits - 1; b >= 0; --b) {
      acc = (acc << 1) | ((v >> b) & 1); ++n;
      if (n == 8) { out.push_back((uint8_t)acc); acc = 0; n = 0; }
    }
  }
  void unary(uint32_t q) { for (uint32_t i = 0; i < q; ++i) write(0, 1); write(1, 1); }
  void align() { if (n) write(0, 8 - n); }
};

static uint32_t crc(const std::vector<uint8_t>& d, uint32_t poly, int width) {
  const uint32_t top = 1u << (width - 1), mask = (width == 16 ? 0xffffu : 0xffu);
  uint32_t c = 0;
  for (uint8_t b : d) {
    c ^= (uint32_t)b << (width - 8);
    for (int i = 0; i < 8; ++i) c = (c & top) ? ((c << 1) ^ poly) & mask : (c << 1) & mask;
  }
  return c;
}

struct Spec {
  int kind;                       // 0 CONSTANT, 1 VERBATIM, 2 FIXED, 3 LPC
  int order, bps, assignment, bs, porder;
  bool five_bit, escape;
  int wasted;
  int spikes;                     // > 0: zeros with isolated spikes of this size (long unary runs at parameter 0)
};

static uint32_t g_seed = 12345;
static uint32_t rnd() { g_seed = g_seed*1664525u + 1013904223u; return g_seed >> 8; }

static void write_residual(BitWriter& bw, const std::vector<int64_t>& res, const Spec& s) {
  bw.write(s.five_bit ? 1 : 0, 2);
  bw.write((uint64_t)s.porder, 4);
  const int pbits = s.five_bit ? 5 : 4;
  size_t pos = 0;
  for (int part = 0; part < (1 << s.porder); ++part) {
    const int count = (s.bs >> s.porder) - (part == 0 ? s.order : 0);
    int64_t sum = 0, top = 0;
    for (int i = 0; i < count; ++i) {
      const int64_t a = res[pos + i] < 0 ? -res[pos + i] : res[pos + i];
      sum += a; top = a > top ? a : top;
    }
    if (s.escape && (part % 2 == 1 || (1 << s.porder) == 1)) {
      int nb = 0;                 // a partition of zeros gets the 0-bit escape
      if (top) { nb = 2; while ((1ll << (nb - 1)) <= top) ++nb; }
      bw.write((1u << pbits) - 1, pbits); bw.write((uint64_t)nb, 5);
      for (int i = 0; i < count; ++i) bw.write((uint64_t)res[pos + i], nb);
    } else {
      int k = 0;
      const int64_t mean = count ? sum/count : 0;
      while ((1ll << k) <= mean) ++k;
      if (k > (1 << pbits) - 2) k = (1 << pbits) - 2;
      bw.write((uint64_t)k, pbits);
      for (int i = 0; i < count; ++i) {
        const int64_t v = res[pos + i];
        const uint64_t u = v >= 0 ? (uint64_t)v << 1 : ((uint64_t)(-v) << 1) - 1;
        bw.unary((uint32_t)(u >> k)); bw.write(u & ((1ull << k) - 1), k);
      }
    }
    pos += (size_t)count;
  }
}

static void write_subframe(BitWriter& bw, std::vector<int64_t> x, int bps, const Spec& s) {
  const int n = (int)x.size();
  const int wasted = s.kind == 0 ? 0 : s.wasted;
  for (auto& v : x) v >>= wasted;                      // (the generator made the low bits zero)
  bps -= wasted;
  const int type = s.kind == 0 ? 0 : s.kind == 1 ? 1 : s.kind == 2 ? 8 + s.order : 31 + s.order;
  bw.write(0, 1); bw.write((uint64_t)type, 6); bw.write(wasted ? 1 : 0, 1);
  if (wasted) bw.unary((uint32_t)wasted - 1);
  if (s.kind == 0) { bw.write((uint64_t)x[0], bps); return; }
  if (s.kind == 1) { for (int64_t v : x) bw.write((uint64_t)v, bps); return; }
  for (int i = 0; i < s.order; ++i) bw.write((uint64_t)x[(size_t)i], bps);
  std::vector<int64_t> coef;
  int shift = 0;
  if (s.kind == 2) {
    static const int fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
    for (int j = 0; j < s.order; ++j) coef.push_back(fixed[s.order][j]);
  } else {
    const int precision = 15;                           // the widest: 25-bit samples x 15 bits x 32 taps
    shift = 13;
    bw.write((uint64_t)precision - 1, 4); bw.write((uint64_t)shift, 5);
    for (int j = 0; j < s.order; ++j) {
      // a stable two-tap predictor plus small tails of alternating sign
      int64_t c = j == 0 ? 15500 : j == 1 ? -7400 : ((j & 1) ? 1 : -1)*(int64_t)(rnd() % 90);
      if (s.order == 1) c = 7900;
      coef.push_back(c);
      bw.write((uint64_t)c, precision);
    }
  }
  std::vector<int64_t> res;
  for (int i = s.order; i < n; ++i) {
    int64_t pred = 0;
    for (int j = 0; j < s.order; ++j) pred += coef[(size_t)j]*x[(size_t)(i - 1 - j)];
    res.push_back(x[(size_t)i] - (pred >> shift));
  }
  write_residual(bw, res, s);
}

// channels x bs samples of spec's width and the frame that encodes them
static Frame make_frame(const Spec& s, std::vector<std::vector<int64_t>>& pcm) {
  const int nch = fd::channels_of(s.assignment);
  pcm.assign((size_t)nch, std::vector<int64_t>((size_t)s.bs));
  const int64_t amp = 1ll << (s.bps - 3);
  for (int c = 0; c < nch; ++c) {
    int64_t v = (int64_t)(rnd() % (uint32_t)amp) - amp/2, d = 0;
    for (int i = 0; i < s.bs; ++i) {
      if (s.kind == 0) { pcm[c][i] = v; continue; }
      if (s.spikes < 0) { pcm[c][i] = 0; continue; }
      if (s.spikes) { pcm[c][i] = (rnd() % 97 == 0) ? (int64_t)s.spikes*((rnd() & 1) ? 1 : -1) : 0; continue; }
      if (s.kind == 1) { pcm[c][i] = (((int64_t)(rnd() % (uint32_t)(2*amp)) - amp) >> s.wasted)*(1ll << s.wasted); continue; }
      d += (int64_t)(rnd() % 33) - 16; d -= d/8;        // a smooth walk
      v += d*(amp >> 9 ? amp >> 9 : 1);
      if (v > 3*amp) v = 3*amp;
      if (v < -3*amp) v = -3*amp;
      pcm[c][i] = (v >> s.wasted)*(1ll << s.wasted);
    }
  }
  std::vector<std::vector<int64_t>> sub = pcm;
  std::vector<int> width((size_t)nch, s.bps);
  if (s.assignment >= 8) {
    std::vector<int64_t> side((size_t)s.bs), mid((size_t)s.bs);
    for (int i = 0; i < s.bs; ++i) { side[i] = pcm[0][i] - pcm[1][i]; mid[i] = (pcm[0][i] + pcm[1][i]) >> 1; }
    if (s.assignment == 8) { sub[1] = side; width[1]++; }
    else if (s.assignment == 9) { sub[0] = side; width[0]++; }
    else { sub[0] = mid; sub[1] = side; width[1]++; }
  }
  BitWriter bw;
  bw.write(0xfff8 >> 2, 14); bw.write(0, 2);
  bw.write(7, 4); bw.write(0, 4); bw.write((uint64_t)s.assignment, 4);
  bw.write(s.bps == 8 ? 1 : s.bps == 12 ? 2 : s.bps == 16 ? 4 : s.bps == 20 ? 5 : 6, 3); bw.write(0, 1);
  bw.write(0, 8);                                       // frame number 0
  bw.write((uint64_t)s.bs - 1, 16);
  bw.write(crc(bw.out, 0x07, 8), 8);
  Frame f;
  f.header = (int)bw.out.size(); f.bs = s.bs; f.assignment = s.assignment; f.bps = s.bps;
  for (int c = 0; c < nch; ++c) {
    Spec sc = s;
    // wasted bits survive a side channel, not a mid channel with odd sides
    if (s.assignment == 10 && c == 0) sc.wasted = 0;
    if (s.kind == 0) {
      bool same = true;
      for (int i = 1; i < s.bs; ++i) same = same && sub[c][i] == sub[c][0];
      if (!same) sc.kind = 1;
    }
    write_subframe(bw, sub[c], width[c], sc);
  }
  bw.align();
  bw.write(crc(bw.out, 0x8005, 16), 16);
  f.bytes = bw.out;
  return f;
}

static std::vector<Spec> corpus() {
  std::vector<Spec> v;
  const int B = 64;
  v.push_back({0, 0, 16, 0, B, 0, false, false, 0, 0});                       // CONSTANT
  v.push_back({0, 0, 16, 10, B, 0, false, false, 0, 0});
  v.push_back({1, 0, 16, 1, B, 0, false, false, 0, 0});                       // VERBATIM, two channels
  v.push_back({1, 0, 24, 10, B, 0, false, false, 2, 0});
  v.push_back({1, 0, 8, 7, 16, 0, false, false, 0, 0});                       // eight channels
  for (int o = 0; o <= 4; ++o) {
    v.push_back({2, o, 16, 0, B, 2, false, false, 0, 0});
    v.push_back({2, o, 24, 8 + o % 3, B, o % 3, (o & 1) != 0, (o & 2) != 0, o == 3 ? 3 : 0, 0});
  }
  v.push_back({2, 2, 12, 9, B, 3, true, true, 0, 0});                         // 5-bit parameters with escapes
  v.push_back({2, 1, 20, 0, B, 0, false, true, 0, 0});                        // one partition, escaped
  v.push_back({2, 0, 16, 0, 192, 1, false, true, 0, 300});                    // zeros and spikes: 0-bit escapes
  v.push_back({2, 2, 16, 0, 64, 2, true, true, 0, -1});                       // all zeros: 0-bit escapes for certain
  v.push_back({2, 0, 16, 0, 256, 0, false, false, 0, 400});                   // long unary runs at parameter 0
  v.push_back({2, 1, 16, 10, 256, 2, true, false, 0, 500});
  for (int o : {1, 2, 7, 8, 12, 31, 32}) {
    v.push_back({3, o, 16, 0, 96, 1, false, false, 0, 0});
    v.push_back({3, o, 24, 10, 96, 0, true, (o & 1) != 0, o == 8 ? 1 : 0, 0}); // the 64-bit accumulator case
  }
  v.push_back({3, 4, 8, 9, 40, 3, false, false, 0, 0});
  v.push_back({2, 4, 16, 0, 5, 0, false, false, 0, 0});                       // order next to the block size
  v.push_back({2, 0, 16, 0, 1, 0, false, false, 0, 0});                       // a block of one sample
  return v;
}

static int run_corpus() {
  long cases = 0;
  int which = 0;
  for (const Spec& s : corpus()) {
    std::vector<std::vector<int64_t>> pcm;
    Frame f = make_frame(s, pcm);
    const int nch = fd::channels_of(f.assignment);
    const std::string tag = "case " + std::to_string(which++) + " (kind " + std::to_string(s.kind) + ", order " +
                            std::to_string(s.order) + ", " + std::to_string(s.bps) + " bits, assignment " +
                            std::to_string(s.assignment) + ")";
    for (int shift = 0; shift < 4; ++shift) {           // valid, at every alignment
      CheckedSink sink(f.bs, nch);
      const int st = decode(f, f.bytes.size(), (int32_t)f.bytes.size(), shift, sink);
      if (st != fd::ST_OK) die(tag + ": valid frame gave status " + std::to_string(st));
      for (int c = 0; c < nch; ++c)
        for (int i = 0; i < f.bs; ++i) {
          const int32_t a = sink.chan[f.assignment >= 8 ? 0 : (size_t)c][(size_t)i];
          const int32_t b = f.assignment >= 8 ? sink.chan[1][(size_t)i] : 0;
          const int32_t got = fd::decorrelate(f.assignment, c, a, b);
          if (got != pcm[(size_t)c][(size_t)i])
            die(tag + ": channel " + std::to_string(c) + " sample " + std::to_string(i) + ": " +
                std::to_string(got) + " != " + std::to_string(pcm[(size_t)c][(size_t)i]));
          const float want = (float)((double)got/(double)(1ull << (f.bps - 1)));
          if (fd::scale_sample(got, f.bps) != want) die(tag + ": scaling differs from the host decoder's");
        }
      ++cases;
    }
    for (size_t cut = 1; cut < f.bytes.size(); ++cut) { // truncated at every byte
      CheckedSink sink(f.bs, nch);
      if (decode(f, cut, (int32_t)cut, (int)(cut & 3), sink) == fd::ST_OK)
        die(tag + ": cut at byte " + std::to_string(cut) + " decoded without a status");
      ++cases;
    }
    for (size_t cut = 1; cut < f.bytes.size(); ++cut) { // ... and with the table still claiming the original length
      CheckedSink sink(f.bs, nch);
      const int st = decode(f, cut, (int32_t)f.bytes.size(), (int)(cut & 3), sink);
      if (st < fd::ST_OK || st > fd::ST_LENGTH) die(tag + ": cut at byte " + std::to_string(cut) + " gave " + std::to_string(st));
      ++cases;
    }
    for (size_t bit = 0; bit < 8*f.bytes.size(); ++bit) {                     // every single-bit flip
      Frame g = f;
      g.bytes[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      CheckedSink sink(g.bs, nch);
      const int st = decode(g, g.bytes.size(), (int32_t)g.bytes.size(), (int)(bit & 3), sink);
      if (st < fd::ST_OK || st > fd::ST_LENGTH) die(tag + ": flipped bit " + std::to_string(bit) + " gave " + std::to_string(st));
      ++cases;
    }
  }
  printf("flac_core_check: %ld cases ok\n", cases);
  return 0;
}

static std::vector<uint8_t> slurp(const char* path) {
  FILE* fp = fopen(path, "rb");
  if (!fp) die(std::string("cannot open ") + path);
  std::vector<uint8_t> d;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, fp)) > 0) d.insert(d.end(), buf, buf + n);
  fclose(fp);
  return d;
}

static int run_decode(const char* stream, const char* table, const char* out) {
  const std::vector<uint8_t> d = slurp(stream), t = slurp(table);
  if (t.size() % 64) die("the frame table is not a whole number of 8 x int64 rows");
  FILE* fp = fopen(out, "wb");
  if (!fp) die(std::string("cannot write ") + out);
  for (size_t r = 0; r < t.size()/64; ++r) {
    int64_t w[8];
    memcpy(w, t.data() + 64*r, 64);
    if (w[0] < 0 || w[1] < 1 || (uint64_t)(w[0] + w[1]) > d.size()) die("frame outside the stream");
    Frame f;
    f.bytes.assign(d.begin() + w[0], d.begin() + w[0] + w[1]);
    f.bs = (int)w[3]; f.assignment = (int)w[4]; f.bps = (int)w[5]; f.header = (int)w[6];
    const int nch = fd::channels_of(f.assignment);
    CheckedSink sink(f.bs, nch);
    const int st = decode(f, f.bytes.size(), (int32_t)f.bytes.size(), (int)(w[0] & 3), sink);
    if (st) die("frame " + std::to_string(r) + ": status " + std::to_string(st));
    for (int i = 0; i < f.bs; ++i)
      for (int c = 0; c < nch; ++c) {
        const int32_t a = sink.chan[f.assignment >= 8 ? 0 : (size_t)c][(size_t)i];
        const int32_t b = f.assignment >= 8 ? sink.chan[1][(size_t)i] : 0;
        const int32_t v = fd::decorrelate(f.assignment, c, a, b);
        fwrite(&v, 4, 1, fp);
      }
  }
  fclose(fp);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "decode")) return run_decode(argv[2], argv[3], argv[4]);
  if (argc != 1) die("usage: flac_core_check | flac_core_check decode STREAM FRAMES OUT");
  return run_corpus();
}
