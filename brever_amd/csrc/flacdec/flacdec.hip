// FLAC dataset members decoded on the GPU (include/brever_flac.h; brever_amd/flac_gpu.py drives it).
//
// FLAC frames are independent -- each has its own header, CRC-8 and CRC-16 -- but a frame's bits are serial: a
// subframe starts where the one before it ends and a Rice code where the one before it ends. So the parallel axis
// is frames.
//
//   host    brv_flacdec_index: metadata, then every frame start WITHOUT entropy decoding. A start is accepted when
//           sync code, reserved bits and CRC-8 hold, the coded number continues the sequence, and the CRC-16 over
//           the bytes up to the next accepted start (or the end of the stream) matches: one table-driven CRC pass.
//           Only when no end is found is the frame parsed (flacdec_core.h, on the host) to say what is wrong.
//   parse   flacdec_parse_kernel: one lane per frame, one wave per workgroup. The bit-serial part: subframe
//           headers, Rice decode, prediction (flacdec_core.h). A lane keeps a 64-bit window refilled with aligned
//           dword loads; unary runs are a count-leading-zeros on it. LPC history and coefficients are per-lane
//           columns of LDS ([32][64] int32 each). Integer subframe samples go to the caller's scratch laid out
//           [group][channel][sample][lane], so the lanes of a wave, which walk their frames in step, store
//           sample i side by side: whole lines although every lane owns another frame.
//   finish  flacdec_finish_kernel: fully parallel. A workgroup takes 64 samples x the lanes of a group, reads
//           them as they lie (coalesced), undoes the stereo decorrelation, scales by 2^-(bps-1), transposes
//           through LDS and stores each frame's row of the window as 256 contiguous bytes into the padded batch.
//
// A job whose fields do not fit the extents of the call, or whose frame does not end exactly where the index said,
// gets a non-zero status and nothing of it reaches `out`.
#include <string.h>

#include <string>

#include "../../../include/brever_flac.h"
#include "../status.h"
#include "flacdec_core.h"

namespace fd = brv_flacdec;

namespace {

// ---- host: the frame index ---------------------------------------------------------------------------------------
uint8_t crc8(const uint8_t* d, size_t n) {                 // poly x^8 + x^2 + x + 1
  uint8_t c = 0;
  for (size_t i = 0; i < n; ++i) {
    c ^= d[i];
    for (int b = 0; b < 8; ++b) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : (c << 1));
  }
  return c;
}

struct Crc16Table {                                        // poly x^16 + x^15 + x^2 + 1
  uint16_t t[256];
  Crc16Table() {
    for (int i = 0; i < 256; ++i) {
      uint16_t c = (uint16_t)(i << 8);
      for (int b = 0; b < 8; ++b) c = (uint16_t)((c & 0x8000) ? (c << 1) ^ 0x8005 : (c << 1));
      t[i] = c;
    }
  }
};

struct StreamInfo { int rate, channels, bps; int64_t total; };

// the offset of the first frame, or BRV_FLACDEC_NOT_FLAC
int64_t parse_metadata(const uint8_t* d, size_t n, StreamInfo& si) {
  if (n < 4 + 4 + 34 || memcmp(d, "fLaC", 4) != 0) return BRV_FLACDEC_NOT_FLAC;
  size_t off = 4;
  bool got = false;
  for (;;) {
    if (off + 4 > n) return BRV_FLACDEC_NOT_FLAC;
    const bool last = d[off] & 0x80;
    const int type = d[off] & 0x7f;
    const size_t len = ((size_t)d[off + 1] << 16) | ((size_t)d[off + 2] << 8) | d[off + 3];
    off += 4;
    if (off + len > n) return BRV_FLACDEC_NOT_FLAC;
    if (type == 0) {
      if (len < 34) return BRV_FLACDEC_NOT_FLAC;
      const uint8_t* s = d + off;
      si.rate = (s[10] << 12) | (s[11] << 4) | (s[12] >> 4);
      si.channels = ((s[12] >> 1) & 7) + 1;
      si.bps = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
      si.total = ((int64_t)(s[13] & 0xf) << 32) | ((int64_t)s[14] << 24) | (s[15] << 16) | (s[16] << 8) | s[17];
      got = true;
    }
    off += len;
    if (last) break;
  }
  return got ? (int64_t)off : (int64_t)BRV_FLACDEC_NOT_FLAC;
}

struct Header { int bytes, blocksize, assignment, bps, variable; int64_t number; };

// The frame header at p (avail bytes follow), checked against STREAMINFO: false unless sync code, reserved bits,
// every field and the CRC-8 hold.
bool parse_header(const uint8_t* p, size_t avail, const StreamInfo& si, Header& h) {
  static const int bps_table[8] = {0, 8, 12, -1, 16, 20, 24, 32};
  if (avail < 5 || p[0] != 0xff || (p[1] & 0xfe) != 0xf8) return false;
  h.variable = p[1] & 1;
  const int bs_code = p[2] >> 4, sr_code = p[2] & 15, ch_code = p[3] >> 4, ss_code = (p[3] >> 1) & 7;
  if ((p[3] & 1) || bs_code == 0 || sr_code == 15 || ch_code > 10) return false;
  size_t at = 4;
  const uint32_t first = p[at++];
  int extra = 0;
  if (first & 0x80) {
    uint32_t m = 0x40;
    while (first & m) { ++extra; m >>= 1; }
    if (extra < 1 || extra > 6) return false;
  }
  uint64_t number = extra ? (first & (0x3fu >> extra)) : first;
  for (int i = 0; i < extra; ++i) {
    if (at >= avail || (p[at] & 0xc0) != 0x80) return false;
    number = (number << 6) | (p[at++] & 0x3f);
  }
  h.number = (int64_t)number;
  if (bs_code == 1) h.blocksize = 192;
  else if (bs_code <= 5) h.blocksize = 576 << (bs_code - 2);
  else if (bs_code == 6) { if (at + 1 > avail) return false; h.blocksize = p[at] + 1; at += 1; }
  else if (bs_code == 7) { if (at + 2 > avail) return false; h.blocksize = ((p[at] << 8) | p[at + 1]) + 1; at += 2; }
  else h.blocksize = 256 << (bs_code - 8);
  at += sr_code == 12 ? 1 : (sr_code == 13 || sr_code == 14) ? 2 : 0;
  if (at + 1 > avail) return false;
  if (crc8(p, at) != p[at]) return false;
  h.bytes = (int)at + 1;
  h.bps = ss_code == 0 ? si.bps : bps_table[ss_code];
  h.assignment = ch_code;
  return h.bps == si.bps && fd::channels_of(ch_code) == si.channels && h.blocksize <= 65535;
}

// host side of flacdec_core.h for the diagnosis: bytes at any alignment, nothing kept
struct HostWords {
  const uint8_t* p; size_t n;
  uint32_t load(uint64_t i) const {
    uint32_t v = 0;
    for (int b = 0; b < 4; ++b)
      if (4*i + b < n) v |= (uint32_t)p[4*i + b] << (8*b);
    return v;
  }
};
struct NullSink {
  int32_t ring[32], coef[32];
  void channel(int) {}
  void put(int, int32_t) {}
  void hset(int i, int32_t v) { ring[i & 31] = v; }
  int32_t hget(int i) const { return ring[i & 31]; }
  void cset(int j, int32_t c) { coef[j & 31] = c; }
  int32_t cget(int j) const { return coef[j & 31]; }
};

// The byte length of the frame at p by parsing it; 0 with damaged = false when its bits run out, 0 with
// damaged = true when a subframe field is invalid.
size_t parsed_length(const uint8_t* p, size_t avail, const Header& h, bool& damaged) {
  if (avail > ((size_t)1 << 27)) avail = (size_t)1 << 27;
  // the core wants the frame's length to know where the CRC-16 sits; parse with everything that is left and
  // read the end off the bits it did not use
  fd::BitReader<HostWords> br;
  br.init(HostWords{p, avail}, 0, (int32_t)avail);
  NullSink sink;
  const int st = fd::frame(br, sink, h.bytes, h.blocksize, h.assignment, h.bps);
  damaged = st == fd::ST_RESERVED;
  if ((st != fd::ST_OK && st != fd::ST_LENGTH) || br.left < 16) return 0;
  return avail - (size_t)(br.left/8) + 2;
}

int64_t index_fail(int code, int64_t frame, const std::string& what) {
  return brv::fail(code, "FLAC frame " + std::to_string(frame) + ": " + what);
}

int64_t index_stream(const uint8_t* d, size_t n, int64_t* info, int64_t* frames, int64_t capacity) {
  static const Crc16Table crc;
  StreamInfo si;
  const int64_t first = parse_metadata(d, n, si);
  if (first < 0) return brv::fail((int)first, "not a FLAC stream: no fLaC marker, metadata cut short or no STREAMINFO");
  if (si.bps > 24)
    return brv::fail(BRV_FLACDEC_NOT_TAKEN, "well-formed, but " + std::to_string(si.bps) +
                     " bits per sample are not taken by the GPU decoder (8 - 24); use brv_flac_decode");
  if (si.bps < 4) return brv::fail(BRV_FLACDEC_NOT_FLAC, "not a FLAC stream: STREAMINFO says fewer than 4 bits per sample");
  size_t pos = (size_t)first;
  int64_t count = 0, done = 0, min_block = 0, max_block = 0;
  int variable = 0;
  Header h;
  bool have_header = false;
  while (pos < n && !(si.total > 0 && done >= si.total)) {
    if (!have_header) {                                    // the first frame: later ones were read to accept the end
      if (!parse_header(d + pos, n - pos, si, h))
        return index_fail(BRV_FLACDEC_BAD_HEADER, count, "bad frame header (sync code, reserved bits, a field against STREAMINFO or CRC-8)");
      variable = h.variable;
      if (h.number != 0) return index_fail(BRV_FLACDEC_BAD_NUMBER, count, "the coded number does not start at 0");
    }
    const bool last = si.total > 0 && done + h.blocksize >= si.total;
    const int64_t expect = variable ? done + h.blocksize : count + 1;
    // one CRC pass: the remainder over a whole frame, its CRC-16 included, is zero
    uint16_t c = 0;
    size_t q = pos, end = 0;
    bool zero_before = false;                              // the remainder was zero at an end that was not accepted
    Header nh;
    for (int b = 0; b < h.bytes && q < n; ++b, ++q) c = (uint16_t)((c << 8) ^ crc.t[(c >> 8) ^ d[q]]);
    while (q < n) {
      c = (uint16_t)((c << 8) ^ crc.t[(c >> 8) ^ d[q]]);
      ++q;
      if (c != 0 || q < pos + h.bytes + 3) continue;
      // the remainder stays zero over every further whole frame, so the end of the stream proves nothing once
      // it was zero before: then the frame is parsed below to say where it ends and what follows it
      if (q == n) { if (!zero_before) end = q; break; }
      if (!last && d[q] == 0xff && parse_header(d + q, n - q, si, nh) && nh.variable == variable && nh.number == expect) {
        end = q;
        break;
      }
      zero_before = true;
    }
    bool next_known = end != 0 && end < n;
    if (end == 0) {
      // No end found. If the next frame's header stands further on (valid, the number that continues the
      // sequence), the frame ends there and its CRC-16 does not match: damaged inside.
      if (!last)
        for (size_t q2 = pos + h.bytes + 3; q2 + 5 <= n; ++q2)
          if (d[q2] == 0xff && parse_header(d + q2, n - q2, si, nh) && nh.variable == variable && nh.number == expect)
            return index_fail(BRV_FLACDEC_BAD_CRC16, count, "CRC-16 mismatch");
      // Otherwise parse the frame to say why (or, for a last frame followed by other bytes, to find its end).
      bool damaged = false;
      const size_t len = parsed_length(d + pos, n - pos, h, damaged);
      if (damaged)
        return index_fail(BRV_FLACDEC_BAD_CRC16, count, "CRC-16 cannot match: a subframe field is invalid");
      if (len == 0 || pos + len > n)
        return index_fail(BRV_FLACDEC_TRUNCATED, count, "the stream ends inside the frame");
      uint16_t cc = 0;
      for (size_t i = pos; i < pos + len; ++i) cc = (uint16_t)((cc << 8) ^ crc.t[(cc >> 8) ^ d[i]]);
      if (cc != 0) return index_fail(BRV_FLACDEC_BAD_CRC16, count, "CRC-16 mismatch");
      if (!last && pos + len < n) {
        if (!parse_header(d + pos + len, n - pos - len, si, nh) || nh.variable != variable)
          return index_fail(BRV_FLACDEC_BAD_HEADER, count + 1, "bad frame header (sync code, reserved bits, a field against STREAMINFO or CRC-8)");
        return index_fail(BRV_FLACDEC_BAD_NUMBER, count + 1, "the coded number " + std::to_string(nh.number) +
                          " does not continue the sequence (expected " + std::to_string(expect) + ")");
      }
      end = pos + len;
    }
    if (count < capacity && frames) {
      int64_t* f = frames + BRV_FLACDEC_FRAME_WORDS*count;
      f[0] = (int64_t)pos; f[1] = (int64_t)(end - pos); f[2] = done; f[3] = h.blocksize;
      f[4] = h.assignment; f[5] = h.bps; f[6] = h.bytes; f[7] = h.number;
    }
    min_block = count == 0 || h.blocksize < min_block ? h.blocksize : min_block;
    max_block = h.blocksize > max_block ? h.blocksize : max_block;
    ++count;
    done += h.blocksize;
    pos = end;
    // an end found by the scan below the end of the stream came with the next header; every other end is the
    // stream's last frame, and the loop leaves
    have_header = next_known;
    if (next_known) h = nh;
    else break;
  }
  if (si.total > 0 && done < si.total)
    return index_fail(BRV_FLACDEC_TRUNCATED, count, "the stream ends before the " + std::to_string(si.total) +
                      " samples of STREAMINFO (" + std::to_string(done) + " found)");
  if (info) {
    info[0] = si.rate; info[1] = si.channels; info[2] = si.bps;
    info[3] = si.total > 0 ? si.total : done;
    info[4] = min_block; info[5] = max_block; info[6] = first; info[7] = variable;
  }
  return count;
}

// ---- device ------------------------------------------------------------------------------------------------------
constexpr int LANES = 64;          // lanes of a wave = threads of a parse workgroup
constexpr int TILE = 64;           // samples per finish workgroup
constexpr int J = BRV_FLACDEC_JOB_WORDS;
constexpr long long MAX_JOBS = 65535LL*LANES;   // the finish kernel's grid has a group per y index

struct DevWords {
  const uint32_t* p;
  __device__ __forceinline__ uint32_t load(uint64_t i) const { return p[i]; }
};

// scratch element of (group, channel c, sample i, lane): lanes of a group side by side
__device__ __forceinline__ size_t scratch_at(size_t group, int channels, int max_block, int c, int i, int G, int lane) {
  return (((group*(size_t)channels + (size_t)c)*(size_t)max_block + (size_t)i)*(size_t)G) + (size_t)lane;
}

struct DevSink {
  int32_t* col;                    // scratch of (group, channel 0, sample 0, lane)
  int32_t* ch;                     // the same of the current channel
  size_t chan_step, G;             // max_block G, G
  int32_t* ring;                   // LDS column of the lane: element j at ring[j*LANES]
  int32_t* coef;
  __device__ __forceinline__ void channel(int c) { ch = col + (size_t)c*chan_step; }
  __device__ __forceinline__ void put(int i, int32_t v) { ch[(size_t)i*G] = v; }
  __device__ __forceinline__ void hset(int i, int32_t v) { ring[(i & 31)*LANES] = v; }
  __device__ __forceinline__ int32_t hget(int i) const { return ring[(i & 31)*LANES]; }
  __device__ __forceinline__ void cset(int j, int32_t c) { coef[(j & 31)*LANES] = c; }
  __device__ __forceinline__ int32_t cget(int j) const { return coef[(j & 31)*LANES]; }
};

// the fields of a job against the extents of the call; every index the two kernels form follows from these
__device__ __forceinline__ bool job_ok(const int64_t* j, int64_t bytes_size, int channels, int max_block,
                                       int64_t out_elems) {
  const int64_t off = j[0], len = j[1], bs = j[2], ca = j[3], bps = j[4], hdr = j[5], lo = j[6], hi = j[7];
  const int64_t at = j[8], stride = j[9];
  if (off < 0 || len < 8 || len > (1LL << 27) || off > bytes_size - len) return false;
  if (bs < 1 || bs > max_block || ca < 0 || ca > 10 || bps < 4 || bps > 24) return false;
  if (hdr < 5 || hdr > 16 || hdr + 3 > len) return false;
  const int nch = fd::channels_of((int)ca);
  if (nch > channels || lo < 0 || hi < lo || hi > bs) return false;
  if (at < 0 || stride < 0 || at > out_elems || stride > out_elems) return false;
  // at + (nch - 1) stride + (hi - lo) <= out_elems, every term <= out_elems <= 2^62/8
  return at + (nch - 1)*stride + (hi - lo) <= out_elems;
}

__global__ __launch_bounds__(LANES) void flacdec_parse_kernel(
    const uint32_t* __restrict__ words, int64_t bytes_size, const int64_t* __restrict__ jobs, int64_t n_jobs,
    int channels, int max_block, int G, int32_t* __restrict__ scratch, int64_t out_elems,
    int32_t* __restrict__ status) {
  __shared__ int32_t ring[32*LANES], coef[32*LANES];
  const int lane = threadIdx.x;
  const int64_t job = (int64_t)blockIdx.x*G + lane;
  if (lane >= G || job >= n_jobs) return;
  const int64_t* j = jobs + J*job;
  if (!job_ok(j, bytes_size, channels, max_block, out_elems)) { status[job] = fd::ST_BAD_FIELDS; return; }
  fd::BitReader<DevWords> br;
  br.init(DevWords{words}, (uint64_t)j[0], (int32_t)j[1]);
  DevSink sink;
  sink.col = scratch + scratch_at(blockIdx.x, channels, max_block, 0, 0, G, lane);
  sink.ch = sink.col;
  sink.chan_step = (size_t)max_block*(size_t)G;
  sink.G = (size_t)G;
  sink.ring = ring + lane;
  sink.coef = coef + lane;
  status[job] = fd::frame(br, sink, (int)j[5], (int)j[2], (int)j[3], (int)j[4]);
}

__global__ __launch_bounds__(256) void flacdec_finish_kernel(
    const int64_t* __restrict__ jobs, int64_t n_jobs, int channels, int max_block, int G,
    const int32_t* __restrict__ scratch, float* __restrict__ out, const int32_t* __restrict__ status) {
  __shared__ float tile[LANES*(TILE + 1)];
  __shared__ int64_t sj[LANES][6];                         // block size, window, place, stride of a lane's job
  __shared__ int sa[LANES][2];                             // channel assignment (-1: nothing to write), sample size
  const int tid = threadIdx.x;
  const size_t group = blockIdx.y;
  const int i0 = blockIdx.x*TILE;
  if (tid < G) {
    const int64_t job = (int64_t)group*G + tid;
    int ca = -1;
    if (job < n_jobs && status[job] == 0) {
      const int64_t* j = jobs + J*job;
      // nothing of this job inside [i0, i0 + TILE): skip it
      if (j[6] < j[7] && j[6] < i0 + TILE && j[7] > i0) {
        ca = (int)j[3];
        sj[tid][0] = j[2]; sj[tid][1] = j[6]; sj[tid][2] = j[7]; sj[tid][3] = j[8]; sj[tid][4] = j[9];
        sa[tid][1] = (int)j[4];
      }
    }
    sa[tid][0] = ca;
  }
  __syncthreads();
  for (int c = 0; c < channels; ++c) {
    for (int e = tid; e < TILE*G; e += 256) {              // as the samples lie: lanes side by side
      const int il = e/G, ln = e - il*G, i = i0 + il;
      const int ca = sa[ln][0];
      float v = 0.f;
      if (ca >= 0 && c < fd::channels_of(ca) && i < (int)sj[ln][0]) {
        int32_t a, b = 0;
        if (ca >= 8) {
          a = scratch[scratch_at(group, channels, max_block, 0, i, G, ln)];
          b = scratch[scratch_at(group, channels, max_block, 1, i, G, ln)];
        } else {
          a = scratch[scratch_at(group, channels, max_block, c, i, G, ln)];
        }
        v = fd::scale_sample(fd::decorrelate(ca, c, a, b), sa[ln][1]);
      }
      tile[ln*(TILE + 1) + il] = v;
    }
    __syncthreads();
    for (int e = tid; e < TILE*G; e += 256) {              // as the batch lies: a frame's samples side by side
      const int ln = e/TILE, il = e - ln*TILE, i = i0 + il;
      const int ca = sa[ln][0];
      if (ca >= 0 && c < fd::channels_of(ca) && i >= sj[ln][1] && i < sj[ln][2])
        out[sj[ln][3] + (int64_t)c*sj[ln][4] + (i - sj[ln][1])] = tile[ln*(TILE + 1) + il];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int64_t brv_flacdec_index(const uint8_t* data, int64_t size, int64_t* stream_info, int64_t* frames,
                          int64_t capacity) {
  BRV_REFUSE(!data, "null data");
  BRV_REFUSE(size < 0 || capacity < 0, "requires size >= 0, capacity >= 0");
  BRV_REFUSE(capacity > 0 && !frames, "null frames with capacity > 0");
  return index_stream(data, (size_t)size, stream_info, frames, capacity);
}

int64_t brv_flacdec_scratch_elems(int64_t n_jobs, int64_t channels, int64_t max_block) {
  BRV_REFUSE(n_jobs < 1 || n_jobs > MAX_JOBS, "requires 1 <= n_jobs <= 4194240");
  BRV_REFUSE(channels < 1 || channels > 8, "requires 1 <= channels <= 8");
  BRV_REFUSE(max_block < 1 || max_block > 65535, "requires 1 <= max_block <= 65535");
  return (n_jobs + LANES - 1)/LANES*LANES*channels*max_block;
}

int brv_flacdec_decode(const uint8_t* bytes, int64_t bytes_size, const int64_t* jobs, int64_t n_jobs,
                       int64_t channels, int64_t max_block, int32_t* scratch, int64_t scratch_elems, float* out,
                       int64_t out_elems, int32_t* status, brv_stream_t stream) {
  BRV_REFUSE(!bytes || !jobs || !scratch || !out || !status, "null pointer");
  BRV_REFUSE(bytes_size < 4 || bytes_size % 4 != 0 || ((uintptr_t)bytes & 3) != 0,
             "requires bytes_size >= 4 and a multiple of 4, bytes 4-byte aligned");
  BRV_REFUSE(n_jobs < 1 || n_jobs > MAX_JOBS, "requires 1 <= n_jobs <= 4194240");
  BRV_REFUSE(channels < 1 || channels > 8, "requires 1 <= channels <= 8");
  BRV_REFUSE(max_block < 1 || max_block > 65535, "requires 1 <= max_block <= 65535");
  BRV_REFUSE(out_elems < 1 || out_elems > (1LL << 56), "requires 1 <= out_elems <= 2^56");
  const int64_t need = (n_jobs + LANES - 1)/LANES*LANES*channels*max_block;
  BRV_REFUSE(scratch_elems < need, "requires scratch_elems >= brv_flacdec_scratch_elems(n_jobs, channels, max_block) = " +
             std::to_string(need));
  // a batch of a few hundred frames is latency bound: narrower groups spread it over more compute units
  // (16 and 4096 are heuristics, not measured against other values: DESIGN.md 5j)
  const int G = n_jobs < 4096 ? 16 : LANES;
  const int64_t groups = (n_jobs + G - 1)/G;
  hipStream_t s = (hipStream_t)stream;
  flacdec_parse_kernel<<<dim3((unsigned)groups), dim3(LANES), 0, s>>>(
      (const uint32_t*)bytes, bytes_size, jobs, n_jobs, (int)channels, (int)max_block, G, scratch, out_elems, status);
  BRV_HIP_OK(hipGetLastError());
  const int64_t tiles = (max_block + TILE - 1)/TILE;
  flacdec_finish_kernel<<<dim3((unsigned)tiles, (unsigned)groups), dim3(256), 0, s>>>(
      jobs, n_jobs, (int)channels, (int)max_block, G, scratch, out, status);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"

// the library's last-error message and its two status exports (../status.h)
BRV_DEFINE_STATUS(brv_flacdec_version, brv_flacdec_last_error)
