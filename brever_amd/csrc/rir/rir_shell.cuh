// What the three tile kernels of libbrever_rir.so share (rir.hip, rir_bands.cuh, rir_hrir.cuh): plain
// inline functions, called with the row layout as compile-time column indices.
//
//   shell_rows, shell_tile   the index row of a job decoded and bounds-checked and the tile of a workgroup, far (heavy)
//                            tiles first; the squared distances [lo2, hi2] an image of that tile can have, the z
//                            column staged in LDS and the prefixes of x and of y that lie inside hi2. (The base
//                            kernel writes these two out, see there.)
//   shell_walk               produce: lane i of round k owns the (x, y) pair 256 k + i in table order, finds its z
//                            range by two binary searches on the staged squared offsets and appends one hit per pass
//                            at the position a prefix count over the workgroup gives it; the kernel's `append` writes
//                            the list entry, its `consume` empties the list whenever another pass might not fit.
//   delay_entry              the fractional delay of an image as a list entry: tau - t0, sin(pi frac) / pi with the
//                            sign of the integer part, cos and sin of 2 pi (tau - t0) / W, halved.
//   lane_taps, tap_weights   consume: lane j is the taps t0 + j and t0 + j + 64: sinc is sign_j q / u, the window
//                            1/2 + cj cw + sj sw with (cj, sj) of the tap computed once: one reciprocal per (image,
//                            tap), no transcendental.
//   wave_sum                 the four waves' sums of a tap, added in wave order.
//
// Entry positions, the flush points and the slices of the waves are functions of the job's own tables and of the
// tile, nothing else: no atomics, bitwise repeatable, a job alone equals the job in a batch.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../../include/rir/brever_rir.h"
#include "rir_host.h"

namespace {

constexpr int kTile = BRV_RIR_TILE;
constexpr int kLaneTaps = kTile/64;             // taps of a lane: lane, lane + 64, ...
constexpr int kThreads = 256, kWaves = kThreads/64;
constexpr double kPi = 3.14159265358979323846;
static_assert(kTile%64 == 0 && kTile <= 256, "a lane of a wave is kLaneTaps taps of the tile");
static_assert(kWaves == 4, "wave_sum adds four waves");

// first index of the ascending v[0..n) whose value is >= x (kStrict: > x)
template <bool kStrict> __device__ __forceinline__ int bound(const double* v, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double m = v[mid];
    if (kStrict ? m <= x : m < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// length of the prefix of the ascending column kCol of the RW-wide rows[0..n) that is <= x (uniform; every thread
// calls it)
template <int RW, int kCol> __device__ __forceinline__ int prefix_within(const double* rows, int n, double x) {
  int count = 0;
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + (int)threadIdx.x;
    count += __syncthreads_count(i < n && rows[(long long)i*RW + kCol] <= x);
  }
  return count;
}

// The job and the tile of a workgroup. Rows are RW doubles: the header H, then the x, y and z candidates.
struct Shell {
  const double *H, *X, *Y, *Z;
  int nx, ny, nz;
  long long taps, T;                            // index word 4; taps of a row of the output, taps + pad
  long long t0;                                 // first tap of the tile
  double halfW, lo2, hi2;                       // squared distances of the images that can land in the tile
  long long npairs;                             // (x, y) pairs inside hi2, x-major
  int nye;
};

// Decodes the index row ix of a table of n_rows rows and takes the tile of this workgroup among those of a row of
// taps + pad taps, the far (heavy) tiles first. False for an index that does not describe rows of this table, and if
// there is no such tile (uniform). Words 5 to 7 are the kernel's own.
template <int RW>
__device__ __forceinline__ bool shell_rows(const double* tab, const long long* ix, long long n_rows, long long pad,
                                           Shell* s) {
  const long long hdr = ix[0], nxl = ix[1], nyl = ix[2], nzl = ix[3], taps = ix[4];
  if (hdr < 0 || nxl < 0 || nyl < 0 || nzl < 0 || nxl > kMaxAxis || nyl > kMaxAxis || nzl > kMaxAxis ||
      hdr > n_rows - 1 - nxl - nyl - nzl || taps < 1 || taps > BRV_RIR_MAX_TAPS) return false;
  const long long T = taps + pad;
  const long long ntile = (T + kTile - 1)/kTile;
  const long long tile = ntile - 1 - (long long)blockIdx.y;
  if (tile < 0) return false;
  s->taps = taps;
  s->T = T;
  s->t0 = tile*kTile;
  s->nx = (int)nxl; s->ny = (int)nyl; s->nz = (int)nzl;
  s->H = tab + hdr*RW;
  s->X = s->H + RW;
  s->Y = s->X + (long long)s->nx*RW;
  s->Z = s->Y + (long long)s->ny*RW;
  return true;
}

// The distance shell of the tile: an image at distance d arrives at (d + delta) fs/c with -less <= delta <= more.
// Stages column kD2 of z in zd2 and counts the pairs; every thread calls it, and it ends with a barrier, so zd2 is
// visible. The kernels read their header row before this call: read after the barriers the four values cost 8 VGPRs,
// which is an occupancy step for rir_bands_tile_kernel<1, sphere> and rir_hrir_tile_kernel<8>.
template <int RW, int kD2>
__device__ __forceinline__ void shell_tile(Shell* s, double fs, double c, double W, double less, double more,
                                           double* zd2) {
  const long long t0 = s->t0, T = s->T;
  const double halfW = 0.5*W, metres = c/fs;
  const long long t_last = t0 + kTile - 1 < T - 1 ? t0 + kTile - 1 : T - 1;
  const double tau_lo = (double)t0 - halfW - kSlack, tau_hi = (double)t_last + halfW + kSlack;
  const double d_lo = tau_lo*metres - less > 0.0 ? tau_lo*metres - less : 0.0, d_hi = tau_hi*metres + more;
  s->halfW = halfW;
  s->lo2 = d_lo*d_lo;
  s->hi2 = d_hi*d_hi;
  for (int i = (int)threadIdx.x; i < s->nz; i += kThreads) zd2[i] = s->Z[(long long)i*RW + kD2];
  const int nxe = prefix_within<RW, kD2>(s->X, s->nx, s->hi2);
  s->nye = prefix_within<RW, kD2>(s->Y, s->ny, s->hi2);
  __syncthreads();                               // zd2 is visible whatever nx and ny are
  s->npairs = s->nz > 0 ? (long long)nxe*s->nye : 0;
}

// An image inside the shell: its rows, the offsets of the receiver to it, its distance, whether max_order counts it,
// and the product of the x and y rows' column kAmp (the first amplitude). axy is the base kernel's per-pair value,
// kept per pair as it was there; the band kernels multiply all K amplitudes per hit and do not read it, so it is dead
// code in them once the walk is inlined. What a kernel derives from dx and dy alone (the measured ear's v.f and v.l)
// is written in its append and hoisted out of the pass loop by the compiler or recomputed per hit: the same values.
struct Hit {
  const double *xr, *yr, *zr;
  double dx, dy, dz, d, axy;
  bool counted;
};

// Walks the images of the shell. append(e, hit) writes entry e of the list, e < kCap, and is called by the lane that
// has the hit; consume(fill) uses up the fill entries of the list and is called by all threads (uniform), whenever the
// list could not take another pass and at the end.
template <int RW, int kCount, int kD2, int kAmp, int kCap, class Append, class Consume>
__device__ __forceinline__ void shell_walk(const Shell& s, const double* zd2, int (*wave_tot)[kWaves],
                                           long long max_order, Append append, Consume consume) {
  static_assert(kCap >= kThreads, "an empty list takes a pass");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int phase = 0, fill = 0;                       // entries in the list
  for (long long p0 = 0; p0 < s.npairs; p0 += kThreads) {
    const long long P = p0 + tid;
    int i0 = 0, i1 = 0, exy = 0;
    double dx = 0.0, dy = 0.0, rxy2 = 0.0, axy = 0.0;
    const double *xr = s.X, *yr = s.Y;
    if (P < s.npairs) {
      const int ixx = (int)(P/s.nye), iyy = (int)(P - (long long)ixx*s.nye);
      xr = s.X + (long long)ixx*RW;
      yr = s.Y + (long long)iyy*RW;
      dx = xr[0]; dy = yr[0];
      axy = xr[kAmp]*yr[kAmp];
      exy = (int)xr[kCount] + (int)yr[kCount];
      rxy2 = xr[kD2] + yr[kD2];
      if (rxy2 <= s.hi2) {
        i0 = bound<false>(zd2, s.nz, s.lo2 - rxy2);
        i1 = bound<true>(zd2, s.nz, s.hi2 - rxy2);
      }
    }
    for (;;) {
      // One hit per lane and pass. Measured at 100 rooms x 19 angles x 8 000 taps: one hit per pass and
      // a list of 512 (33 KB of LDS, four workgroups per CU) 162 ms; two hits and 1 024 entries (52 KB, three
      // workgroups) 173 ms; a tile of 256 taps (142 VGPRs, two waves per SIMD) 240 ms. The kernel waits on latencies,
      // so residency decides.
      const int m = i1 - i0 < 1 ? i1 - i0 : 1;
      // position of this lane's hit: lanes below it in the wave, then the waves below
      const unsigned long long below = (1ull << lane) - 1ull;
      const unsigned long long b = __ballot(m > 0);
      int pos = __popcll(b & below);
      if (lane == 0) wave_tot[phase][wave] = __popcll(b);
      __syncthreads();
      int total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int n = wave_tot[phase][w];
        if (w < wave) pos += n;
        total += n;
      }
      phase ^= 1;
      if (total == 0) break;                     // uniform: every lane's range is used up
      if (m > 0) {
        const double* zr = s.Z + (long long)i0*RW;
        const double dz = zr[0];
        const bool counted = max_order < 0 || exy + (int)zr[kCount] <= max_order;
        const double d = sqrt(rxy2 + zr[kD2]);
        append(fill + pos, Hit{xr, yr, zr, dx, dy, dz, d, axy, counted});   // fill <= kCap - kThreads before a pass
      }
      i0 += m;
      fill += total;
      if (fill > kCap - kThreads) {
        consume(fill);
        fill = 0;
      }
    }
  }
  if (fill > 0) consume(fill);
}

// The list entry of a delay of tau samples in the tile that starts at t0: tau - t0; scale sin(pi frac) / pi with the
// sign of the integer part (0 where frac == 0: the tap at u == 0 then takes its value as it is, see tap_weights); cos
// and sin of 2 pi (tau - t0) / W, halved.
struct Delay {
  double taur, s, cw, sw;
  bool whole;                                   // frac == 0
};

__device__ __forceinline__ Delay delay_entry(double tau, long long t0, double W, double scale) {
  const double k = floor(tau), f = tau - k;
  const long long kr = (long long)k - t0;
  const double taur = tau - (double)t0;
  double sw, cw;
  sincospi(2.0*taur/W, &sw, &cw);
  return Delay{taur, f == 0.0 ? 0.0 : scale*sinpi(f)/kPi*((kr & 1) ? 1.0 : -1.0), 0.5*cw, 0.5*sw, f == 0.0};
}

// the taps of a lane: sin and cos of 2 pi j / W for j = lane + 64 k, and (-1)^j, which is that of lane
struct LaneTaps {
  double sj[kLaneTaps], cj[kLaneTaps], sign;
};

__device__ __forceinline__ LaneTaps lane_taps(int lane, double W) {
  LaneTaps t;
#pragma unroll
  for (int k = 0; k < kLaneTaps; ++k) sincospi(2.0*(double)(lane + 64*k)/W, &t.sj[k], &t.cj[k]);
  t.sign = (lane & 1) ? -1.0 : 1.0;
  return t;
}

// The Hann-windowed sinc of the entry (tr, q, cw, sw) at the taps of a lane; at_zero is its value at u == 0, where
// q is 0.
__device__ __forceinline__ void tap_weights(const LaneTaps& t, int lane, double halfW, double tr, double q,
                                            double at_zero, double cw, double sw, double (&out)[kLaneTaps]) {
  const double s = t.sign*q;
#pragma unroll
  for (int k = 0; k < kLaneTaps; ++k) {
    const double u = (double)(lane + 64*k) - tr;
    const double win = __builtin_fma(t.sj[k], sw, __builtin_fma(t.cj[k], cw, 0.5));
    // 1/u as v_rcp_f64 and two Newton steps (five instructions; the IEEE division is about eleven): each step
    // squares the relative error of the one before, far below the fp32 rounding of the output either way. u = 0
    // gives a NaN that the select drops.
    double r = __builtin_amdgcn_rcp(u);
    r = __builtin_fma(__builtin_fma(-u, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-u, r, 1.0), r, r);
    const double v = u == 0.0 ? at_zero : s*r*win;
    out[k] = fabs(u) < halfW ? v : 0.0;
  }
}

// The sum over the four waves, in wave order, of the tap threadIdx.x of the tile (0 for the threads past the tile).
// One barrier; the caller puts another before part is written again.
__device__ __forceinline__ double wave_sum(double (*part)[kTile], const double (&acc)[kLaneTaps]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < kLaneTaps; ++k) part[wave][lane + 64*k] = acc[k];
  __syncthreads();
  return tid < kTile ? ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid] : 0.0;
}

}  // namespace
