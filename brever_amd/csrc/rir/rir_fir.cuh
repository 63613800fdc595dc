// The FIR tile that rir_bands_combine_kernel and rir_hrir_fold_kernel share: a workgroup of 128 threads is 1 024
// output taps, a lane 8 consecutive ones. The needed stretch of a row goes to LDS once (swizzled by one double per 16
// so that lanes 8 doubles apart hit different banks) and a lane takes the filters 16 taps at a time from 23 row values
// in registers: 128 FMAs per filter and 23 LDS reads, the coefficients uniform. Filter taps in order.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kFirTile = 1024, kFirThreads = 128, kFirTaps = kFirTile/kFirThreads, kFirChunk = 16;
static_assert(kFirTaps == 8, "a lane of a FIR tile is 8 taps");

// position in LDS of the local row index l: one double of padding per 16
__device__ __forceinline__ int comb_at(int l) { return l + (l >> 4); }
// doubles of LDS for filters of up to max_filter taps
constexpr int fir_lds(int max_filter) { return kFirTile + max_filter + (kFirTile + max_filter)/16 + 1; }

// Adds to acc[e][i] the filter f[e] (nf taps, a multiple of 16) applied to the row of T values at the row index
// g0 + 8 tid + i, e < kFilters: the row index g0 - (nf - 1) + l is the local index l, 0 <= l < 1 024 + nf - 1, and
// reads as 0 outside the row. Every thread of the workgroup calls it (barriers); xs holds fir_lds(nf) doubles.
template <int kFilters>
__device__ __forceinline__ void fir_tile(double* xs, const double* row, long long T, long long g0, int nf,
                                         const double* const (&f)[kFilters], double (&acc)[kFilters][kFirTaps]) {
  const int tid = threadIdx.x;
  const long long gbase = g0 - (nf - 1);
  const int n_local = kFirTile + nf - 1;
  __syncthreads();
  for (int l = tid; l < n_local; l += kFirThreads) {
    const long long g = gbase + l;
    xs[comb_at(l)] = g >= 0 && g < T ? row[g] : 0.0;
  }
  __syncthreads();
  for (int m0 = 0; m0 < nf; m0 += kFirChunk) {
    // w[j] is the row at q - (kFirChunk - 1) + j, q the row index of this lane's first tap at filter tap m0
    const int lq = kFirTaps*tid + (nf - 1) - m0;
    double w[kFirChunk - 1 + kFirTaps];
#pragma unroll
    for (int j = 0; j < kFirChunk - 1 + kFirTaps; ++j) w[j] = xs[comb_at(lq - (kFirChunk - 1) + j)];
#pragma unroll
    for (int mm = 0; mm < kFirChunk; ++mm) {
      double fm[kFilters];
#pragma unroll
      for (int e = 0; e < kFilters; ++e) fm[e] = f[e][m0 + mm];
#pragma unroll
      for (int i = 0; i < kFirTaps; ++i) {
#pragma unroll
        for (int e = 0; e < kFilters; ++e) acc[e][i] = __builtin_fma(fm[e], w[kFirChunk - 1 + i - mm], acc[e][i]);
      }
    }
  }
}

}  // namespace
