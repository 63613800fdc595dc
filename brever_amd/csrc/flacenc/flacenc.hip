// A padded device batch encoded as FLAC streams on the GPU (include/brever_flacenc.h; brever_amd/flac_enc.py drives it).
//
// An encoder predicts from the original samples, so the residuals of a frame are independent of each other; only
// the place of a code in the bit stream is a running sum, and that is a prefix scan. So a whole workgroup works on
// one frame.
//
//   frames  flacenc_frame_kernel: one workgroup of 256 threads per (row, frame), running encode_frame of
//           flacenc_core.h: validate, then per coded channel (left, right, mid, side) the exact bit count of every
//           candidate -- per (partition, Rice parameter) sums of u >> k in LDS through 64-bit integer adds, so no
//           count depends on the order of arrival -- the stereo decision, a scan of the chosen codes' lengths, and
//           the deposit of every code's stop bit and remainder with atomicOr into the zero-filled image of the frame
//           (the zeros of a unary run need no writing; OR is order-independent, so the bytes are repeatable). The
//           CRC-16 is a chunk per thread, shifted to its place by x^(8 bytes behind it) mod P and XOR-ed together.
//           Samples are quantised (and mid / side formed) from the input; the coded channel being worked on is kept
//           in LDS up to 4096 samples, what lies beyond is read from the input where it is used. The image lies
//           in global scratch, not LDS, because a frame of the largest block size (65535 x 2 x 25 bits) would not fit
//           there; its words are zeroed, OR-ed and read back with agent-scope atomics (the OR executes in L2, a
//           plain load could hit an older line of the compute unit's L1), and images are 256-byte aligned.
//   layout  flacenc_layout_kernel: one workgroup. Per row the offsets of its frames, the least and largest frame,
//           STREAMINFO; then a scan over the rows' sizes: the offset table.
//   pack    flacenc_pack_kernel: a thread per output dword; the source is at any byte offset of a frame's image
//           (two dword loads and a funnel shift), the stores are whole dwords.
#include <string>

#include "../../../include/brever_flacenc.h"
#include "../status.h"
#include "flacenc_core.h"

namespace fe = brv_flacenc;

namespace {

constexpr int NT = fe::MAX_THREADS;
constexpr int HEADER_WORDS = 12;                     // 42 bytes of 'fLaC' + STREAMINFO per row, padded

struct DevSrc {
  const float* xf; const int32_t* xi;                // the frame's first sample of channel 0, one of the two
  int64_t stride;
  int bps;
  __device__ __forceinline__ int32_t sample(int c, int i) const {
    if (xf) return fe::quantise(xf[(int64_t)c*stride + i], bps);
    const int32_t v = xi[(int64_t)c*stride + i];
    return fe::pcm_flags(v, bps) ? 0 : v;
  }
  __device__ __forceinline__ int32_t get(int code, int i) const {
    const int32_t l = sample(0, i);
    if (code == 0) return l;
    return fe::coded_channel(code, l, sample(1, i));
  }
  __device__ __forceinline__ int flags(int c, int i) const {
    return xf ? fe::float_flags(xf[(int64_t)c*stride + i]) : fe::pcm_flags(xi[(int64_t)c*stride + i], bps);
  }
};

struct DevImg {
  uint32_t* p; uint32_t n;
  __device__ __forceinline__ uint32_t words() const { return n; }
  __device__ __forceinline__ void zero(uint32_t w) { __hip_atomic_store(p + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void orw(uint32_t w, uint32_t v) { atomicOr(p + w, v); }
  __device__ __forceinline__ uint32_t load(uint32_t w) const { return __hip_atomic_load(p + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

struct DevPar {
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ void publish() { __threadfence(); }
  __device__ __forceinline__ void add64(uint64_t* p, uint64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
  __device__ __forceinline__ void or32(uint32_t* p, uint32_t v) { atomicOr(p, v); }
  __device__ __forceinline__ void xor32(uint32_t* p, uint32_t v) { atomicXor(p, v); }
};

// where things lie in the scratch (int32 elements); the status words come first, padded to 16 bytes, and are the
// block the call zeroes
struct Plan {
  int64_t frames_per_row, jobs, cap_words;
  int64_t status, frame_len, frame_off, headers, images, total;
};

Plan plan(int64_t rows, int64_t channels, int64_t max_len, int64_t bps, int64_t block) {
  Plan p;
  p.frames_per_row = (max_len + block - 1)/block;
  p.jobs = rows*p.frames_per_row;
  p.cap_words = fe::frame_capacity(channels, bps, block)/4;
  p.status = 0;
  p.frame_len = (rows + 3)/4*4;
  p.frame_off = p.frame_len + p.jobs;
  p.headers = p.frame_off + p.jobs;
  p.images = (p.headers + rows*HEADER_WORDS + 63)/64*64;
  p.total = p.images + p.jobs*p.cap_words;
  return p;
}

__global__ __launch_bounds__(NT) void flacenc_frame_kernel(
    const void* __restrict__ x, int pcm, const int64_t* __restrict__ lengths, int64_t max_len, int channels, int bps,
    int rate, int block, int lpc_order, int64_t frames_per_row, int64_t cap_words, int32_t* __restrict__ status,
    uint32_t* __restrict__ frame_len, uint32_t* __restrict__ images) {
  __shared__ fe::Shared sh;
  const int tid = threadIdx.x;
  const int64_t job = blockIdx.x, row = job/frames_per_row, fidx = job - row*frames_per_row;
  const int64_t len = lengths[row];
  if (len < 1 || len > max_len) {                    // the row's length against the extent of the call
    if (tid == 0) {
      frame_len[job] = 0;
      if (fidx == 0) atomicOr(&status[row], fe::ROW_LENGTH);
    }
    return;
  }
  const int64_t start = fidx*block;
  if (start >= len) {
    if (tid == 0) frame_len[job] = 0;
    return;
  }
  fe::Frame f;
  f.bs = (int)(len - start < block ? len - start : block);
  f.channels = channels; f.bps = bps; f.rate = rate; f.lpc_order = lpc_order; f.number = fidx;
  const int64_t first = row*channels*max_len + start;  // f.bs samples from here, per channel, lie inside the row
  DevSrc src{pcm ? nullptr : (const float*)x + first, pcm ? (const int32_t*)x + first : nullptr, max_len, bps};
  DevImg img{images + job*cap_words, (uint32_t)cap_words};
  DevPar par;
  uint32_t flags = 0;
  const uint32_t bytes = fe::encode_frame(par, &sh, src, img, f, tid, NT, &flags);
  if (tid == 0) {
    frame_len[job] = bytes;
    if (bytes == 0) flags |= fe::ROW_INTERNAL;
    if (flags) atomicOr(&status[row], (int32_t)flags);
  }
}

__global__ __launch_bounds__(NT) void flacenc_layout_kernel(
    const int64_t* __restrict__ lengths, int64_t rows, int64_t max_len, int channels, int bps, int rate, int block,
    int64_t frames_per_row, int64_t cap_words, const int32_t* __restrict__ status,
    const uint32_t* __restrict__ frame_len, uint32_t* __restrict__ frame_off, uint8_t* __restrict__ headers,
    int64_t* __restrict__ table) {
  __shared__ int64_t scan[2][NT];
  const int tid = threadIdx.x;
  const int64_t chunk = (rows + NT - 1)/NT;
  const int64_t lo = tid*chunk, hi = lo + chunk < rows ? lo + chunk : rows;
  int64_t mine = 0;
  for (int64_t row = lo; row < hi; ++row) {
    const int64_t len = lengths[row];
    int32_t st = status[row];
    int64_t size = 0;
    if (st == 0 && len >= 1 && len <= max_len) {
      const int64_t n = (len + block - 1)/block;
      uint32_t at = fe::STREAM_HEADER_BYTES, least = ~0u, most = 0;
      for (int64_t k = 0; k < n; ++k) {
        uint32_t b = frame_len[row*frames_per_row + k];
        if (b > 4*(uint32_t)cap_words) b = 0;            // a length this call did not write
        frame_off[row*frames_per_row + k] = at;
        at += b;
        least = b < least ? b : least;
        most = b > most ? b : most;
      }
      size = at;
      fe::stream_header(headers + 4*HEADER_WORDS*row, block, least, most, rate, channels, bps, len);
    }
    table[rows + 1 + row] = size;
    table[2*rows + 1 + row] = st;
    table[row] = (size + 3)/4*4;                         // the padded size now, the offset below
    mine += (size + 3)/4*4;
  }
  scan[0][tid] = mine;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < NT; d <<= 1) {
    scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0);
    cur ^= 1;
    __syncthreads();
  }
  int64_t at = scan[cur][tid] - mine;
  for (int64_t row = lo; row < hi; ++row) {
    const int64_t padded = table[row];
    table[row] = at;
    at += padded;
  }
  if (tid == NT - 1) table[rows] = scan[cur][NT - 1];
}

__global__ __launch_bounds__(NT) void flacenc_pack_kernel(
    const int64_t* __restrict__ lengths, int64_t rows, int block, int64_t frames_per_row, int64_t cap_words,
    const uint32_t* __restrict__ frame_len, const uint32_t* __restrict__ frame_off,
    const uint32_t* __restrict__ headers, const uint32_t* __restrict__ images, const int64_t* __restrict__ table,
    uint32_t* __restrict__ out, int64_t out_words) {
  const int64_t row = blockIdx.y;
  const int64_t size = table[rows + 1 + row];
  const int64_t d = (int64_t)blockIdx.x*NT + threadIdx.x;
  if (4*d >= size) return;
  const int64_t n = (lengths[row] + block - 1)/block;  // size > 0: the layout accepted the row's length
  const uint32_t* len = frame_len + row*frames_per_row;
  const uint32_t* off = frame_off + row*frames_per_row;
  const uint32_t* hdr = headers + HEADER_WORDS*row;
  const uint32_t b0 = (uint32_t)(4*d);
  // the frame that holds byte b: the last one that starts at or before it
  auto frame_of = [&](uint32_t b) {
    int64_t l = 0, h = n - 1;
    while (l < h) {
      const int64_t m = (l + h + 1)/2;
      if (off[m] <= b) l = m; else h = m - 1;
    }
    return l;
  };
  auto byte_at = [&](uint32_t b) -> uint32_t {
    if ((int64_t)b >= size) return 0u;
    if (b < fe::STREAM_HEADER_BYTES) return (hdr[b >> 2] >> (8*(b & 3u))) & 0xffu;
    const int64_t k = frame_of(b);
    const uint32_t s = b - off[k];
    if (s >= len[k] || s >= 4*(uint32_t)cap_words) return 0u;
    return (images[(row*frames_per_row + k)*cap_words + (s >> 2)] >> (8*(s & 3u))) & 0xffu;
  };
  uint32_t v;
  const int64_t k = b0 >= fe::STREAM_HEADER_BYTES ? frame_of(b0) : -1;
  if (k >= 0 && b0 - off[k] + 3 < len[k] && len[k] <= 4*(uint32_t)cap_words) {
    const uint32_t s = b0 - off[k], r = 8*(s & 3u);
    const uint32_t* w = images + (row*frames_per_row + k)*cap_words + (s >> 2);
    v = r ? (w[0] >> r) | (w[1] << (32 - r)) : w[0];     // byte s + 3 lies in w[1] and below the frame's length
  } else {
    v = byte_at(b0) | (byte_at(b0 + 1) << 8) | (byte_at(b0 + 2) << 16) | (byte_at(b0 + 3) << 24);
  }
  const int64_t at = table[row]/4 + d;
  if (at >= 0 && at < out_words) out[at] = v;
}

const char* check_extents(int64_t rows, int64_t channels, int64_t max_len, int64_t bps, int64_t block) {
  if (channels != 1 && channels != 2) return "requires channels 1 or 2";
  if (bps != 16 && bps != 24) return "requires bits_per_sample 16 or 24";
  if (block < 16 || block > 65535) return "requires 16 <= block_size <= 65535";
  if (rows < 1 || rows > BRV_FLACENC_MAX_ROWS) return "requires 1 <= rows <= 65535";
  if (max_len < 1 || max_len > (1LL << 30)) return "requires 1 <= max_len <= 2^30";
  if (rows*((max_len + block - 1)/block) > (1LL << 30)) return "requires rows ceil(max_len/block_size) <= 2^30 frames";
  // byte offsets inside a row's stream are 32-bit
  if ((max_len + block - 1)/block*fe::frame_capacity(channels, bps, block) > (1LL << 31) - 64)
    return "requires ceil(max_len/block_size) brv_flacenc_frame_capacity(...) < 2^31 bytes per row";
  return nullptr;
}

}  // namespace

extern "C" {

int64_t brv_flacenc_frame_capacity(int64_t channels, int64_t bits_per_sample, int64_t block_size) {
  const char* why = check_extents(1, channels, 1, bits_per_sample, block_size);
  BRV_REFUSE(why, why);
  return fe::frame_capacity(channels, bits_per_sample, block_size);
}

int64_t brv_flacenc_scratch_elems(int64_t rows, int64_t channels, int64_t max_len, int64_t bits_per_sample,
                                  int64_t block_size) {
  const char* why = check_extents(rows, channels, max_len, bits_per_sample, block_size);
  BRV_REFUSE(why, why);
  return plan(rows, channels, max_len, bits_per_sample, block_size).total;
}

int64_t brv_flacenc_out_capacity(int64_t rows, int64_t channels, int64_t max_len, int64_t bits_per_sample,
                                 int64_t block_size) {
  const char* why = check_extents(rows, channels, max_len, bits_per_sample, block_size);
  BRV_REFUSE(why, why);
  const Plan p = plan(rows, channels, max_len, bits_per_sample, block_size);
  return rows*(4*HEADER_WORDS + p.frames_per_row*p.cap_words*4);
}

int brv_flacenc_encode(const void* x, int64_t pcm, const int64_t* lengths, int64_t rows, int64_t channels,
                       int64_t max_len, int64_t sample_rate, int64_t bits_per_sample, int64_t block_size,
                       int64_t lpc_order, int32_t* scratch, int64_t scratch_elems, uint8_t* out,
                       int64_t out_capacity, int64_t* table, brv_stream_t stream) {
  BRV_REFUSE(!x || !lengths || !scratch || !out || !table, "null pointer");
  const char* why = check_extents(rows, channels, max_len, bits_per_sample, block_size);
  BRV_REFUSE(why, why);
  BRV_REFUSE(sample_rate < 1 || sample_rate > 655350, "requires 1 <= sample_rate <= 655350");
  BRV_REFUSE(lpc_order < 0 || lpc_order > BRV_FLACENC_MAX_LPC_ORDER, "requires 0 <= lpc_order <= 32");
  BRV_REFUSE(((uintptr_t)x & 3) != 0 || ((uintptr_t)scratch & 255) != 0 || ((uintptr_t)out & 3) != 0 ||
             ((uintptr_t)lengths & 7) != 0 || ((uintptr_t)table & 7) != 0,
             "requires x and out 4-byte aligned, lengths and table 8-byte aligned, scratch 256-byte aligned");
  const Plan p = plan(rows, channels, max_len, bits_per_sample, block_size);
  BRV_REFUSE(scratch_elems < p.total, "requires scratch_elems >= brv_flacenc_scratch_elems(...) = " + std::to_string(p.total));
  const int64_t need = rows*(4*HEADER_WORDS + p.frames_per_row*p.cap_words*4);
  BRV_REFUSE(out_capacity < need, "requires out_capacity >= brv_flacenc_out_capacity(...) = " + std::to_string(need));
  hipStream_t s = (hipStream_t)stream;
  int32_t* status = scratch + p.status;
  uint32_t* frame_len = (uint32_t*)scratch + p.frame_len;
  uint32_t* frame_off = (uint32_t*)scratch + p.frame_off;
  uint32_t* headers = (uint32_t*)scratch + p.headers;
  uint32_t* images = (uint32_t*)scratch + p.images;
  BRV_HIP_OK(hipMemsetAsync(status, 0, (size_t)p.frame_len*4, s));
  flacenc_frame_kernel<<<dim3((unsigned)p.jobs), dim3(NT), 0, s>>>(
      x, pcm ? 1 : 0, lengths, max_len, (int)channels, (int)bits_per_sample, (int)sample_rate, (int)block_size,
      (int)lpc_order, p.frames_per_row, p.cap_words, status, frame_len, images);
  BRV_HIP_OK(hipGetLastError());
  flacenc_layout_kernel<<<dim3(1), dim3(NT), 0, s>>>(
      lengths, rows, max_len, (int)channels, (int)bits_per_sample, (int)sample_rate, (int)block_size,
      p.frames_per_row, p.cap_words, status, frame_len, frame_off, (uint8_t*)headers, table);
  BRV_HIP_OK(hipGetLastError());
  const int64_t row_words = HEADER_WORDS + p.frames_per_row*p.cap_words;
  flacenc_pack_kernel<<<dim3((unsigned)((row_words + NT - 1)/NT), (unsigned)rows), dim3(NT), 0, s>>>(
      lengths, rows, (int)block_size, p.frames_per_row, p.cap_words, frame_len, frame_off, headers, images, table,
      (uint32_t*)out, out_capacity/4);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"

// the library's last-error message and its two status exports (../status.h)
BRV_DEFINE_STATUS(brv_flacenc_version, brv_flacenc_last_error)
