// BSS-eval SIR and SAR (include/sdr/brever_bsseval.h): the joint projection of S estimates on the span of
// J references, each through L taps. Included by sdr.hip behind its kernels, which it launches: sdr_corr_kernel gives
// every lag, sdr_solve_kernel every single-reference projection (so SDR[e][j] has the bits of brv_sdr_forward).
//
//   bss_pack_kernel    references and estimates of an item side by side as rows of one (items, J + S, stride) array,
//                      so that one stride addresses both operands of sdr_corr_kernel; lengths clamped and repeated
//                      per pair for sdr_solve_kernel
//   bss_block_kernel   one workgroup (four waves) per item, templated on J and S: the chunks of the J^2 reference
//                      pairs summed in ascending order into R(0 .. L-1) in LDS (R(-l) = R(l)^T is not stored), then
//                      the block Levinson recursion. Lane `tid` owns the block indices m = tid and tid + 256: F[m]
//                      and C[m] never leave its registers; B lives in LDS because B'[m] needs B[m - 1]. A step is
//                      2 J^2 + J S sums over the lanes (wave_sum, then the four waves through LDS), three J x J
//                      solves that every lane computes from the same words, and the update: two barriers.
//   bss_final_kernel   one lane per item: the tables, the floors, the permutation, the flags
//
// qJ is accumulated as the recursion goes: d'^T C' - d^T C = eps^T Eb'^-1 eps, a sum of non-negative terms. C[0]
// gets one step of iterative refinement, so that an estimate that is a power-of-two multiple of a reference (or of a
// sum of references) starts the recursion with its exact coefficients, every later eps is 0 and qJ = E exactly.
#pragma once

#include "../../../include/sdr/brever_bsseval.h"

namespace {

constexpr int kMaxJ = BRV_BSS_MAX_REFERENCES;
constexpr double kPivotTol = 0x1p-40;          // a pivot is positive if it exceeds this share of its diagonal entry
static_assert(BRV_BSS_MAX_FILTER_LENGTH == kMaxL, "the block recursion holds two block indices per lane");

// workspace, in doubles from its start (every section a whole number of doubles)
struct BssLayout {
  int64_t pairs, nchunk, slot;       // J S + J^2 pairs, chunks per row, doubles per (row, chunk)
  int64_t lag, sdr1, q1, e1, h1, qj, flags1, blkflags, lengths, sig, total;
};

__host__ BssLayout bss_layout(int64_t B, int64_t S, int64_t J, int64_t T, int64_t L) {
  BssLayout w;
  w.pairs = J*S + J*J;
  w.nchunk = (T + kChunk - 1)/kChunk;
  w.slot = 2*L + 1;
  const int64_t rows1 = J*S*B;
  int64_t o = 0;
  w.lag = o;      o += w.pairs*B*w.nchunk*w.slot;
  w.sdr1 = o;     o += rows1;
  w.q1 = o;       o += rows1;
  w.e1 = o;       o += rows1;
  w.h1 = o;       o += rows1*L;
  w.qj = o;       o += B*S;
  w.flags1 = o;   o += (rows1 + 1)/2;          // int32
  w.blkflags = o; o += (B + 1)/2;              // int32
  w.lengths = o;  o += rows1;                  // int64: the clamped lengths, once per pair (s_j, x_e)
  w.sig = o;      o += (B*(J + S)*T + 1)/2;    // float
  w.total = o;
  return w;
}

__global__ __launch_bounds__(256) void bss_pack_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                       const long long* __restrict__ lengths, long long B, int S,
                                                       int J, long long T, float* __restrict__ sig,
                                                       long long* __restrict__ len_out) {
  const long long n = B*(J + S)*T;
  for (long long i = (long long)blockIdx.x*256 + threadIdx.x; i < n; i += (long long)gridDim.x*256) {
    const long long t = i % T, row = i/T, b = row/(J + S);
    const int a = (int)(row % (J + S));
    sig[i] = a < J ? s[(b*J + a)*T + t] : x[(b*S + (a - J))*T + t];
  }
  for (long long i = (long long)blockIdx.x*256 + threadIdx.x; i < B*J*S; i += (long long)gridDim.x*256)
    len_out[i] = row_length(lengths, (int)(i % B), T);
}

// A = Lf diag(1/dinv) Lf^T from the lower triangle of A (unit Lf, its strict lower part stored); false where a pivot
// is not positive. Reciprocals once, as in sdr_solve_kernel.
template <int J> __device__ __forceinline__ bool ldl_factor(const double (&A)[J][J], double (&Lf)[J][J],
                                                            double (&dinv)[J]) {
  bool ok = true;
  double w[J][J];                                   // w[r][k] = Lf[r][k] d[k]
#pragma unroll
  for (int i = 0; i < J; ++i) {
    double v = A[i][i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = __builtin_fma(-Lf[i][k], w[i][k], v);
    ok = ok && (v > kPivotTol*A[i][i]);
    dinv[i] = 1.0/v;
#pragma unroll
    for (int r = i + 1; r < J; ++r) {
      double u = A[r][i];
#pragma unroll
      for (int k = 0; k < i; ++k) u = __builtin_fma(-Lf[r][k], w[i][k], u);
      w[r][i] = u;
      Lf[r][i] = u*dinv[i];
    }
  }
  return ok;
}

// X = A^-1 Y for N columns, from the factors
template <int J, int N> __device__ __forceinline__ void ldl_solve(const double (&Lf)[J][J], const double (&dinv)[J],
                                                                  const double (&Y)[J][N], double (&X)[J][N]) {
#pragma unroll
  for (int c = 0; c < N; ++c) {
    double y[J];
#pragma unroll
    for (int i = 0; i < J; ++i) {
      double v = Y[i][c];
#pragma unroll
      for (int k = 0; k < i; ++k) v = __builtin_fma(-Lf[i][k], y[k], v);
      y[i] = v;
    }
#pragma unroll
    for (int i = J - 1; i >= 0; --i) {
      double v = y[i]*dinv[i];
#pragma unroll
      for (int k = i + 1; k < J; ++k) v = __builtin_fma(-Lf[k][i], X[k][c], v);
      X[i][c] = v;
    }
  }
}

template <int J, int S>
__global__ __launch_bounds__(256) void bss_block_kernel(const double* __restrict__ lag,
                                                        const long long* __restrict__ lengths, int L, int nchunk,
                                                        int B, double load_diag, double* __restrict__ qj,
                                                        int* __restrict__ blkflags) {
  constexpr int JJ = J*J, kSums = 2*JJ + J*S;
  __shared__ double Rl[kMaxL*JJ];                  // R(l)[i][j] at l JJ + i J + j
  __shared__ double Bl[kMaxL*JJ];                  // the backward predictor, B[m][i][j] likewise
  __shared__ double part[4][kSums];
  const int item = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long T = lengths[item];               // clamped by bss_pack_kernel
  const int nc = (int)((T + kChunk - 1)/kChunk);
  const long long slot = 2*L + 1, rowsz = (long long)nchunk*slot;
  // R: the b part (lags l >= 0 of y = s_i against x = s_j) of pair J S + i J + j, chunks in ascending order
  for (int idx = tid; idx < L*JJ; idx += 256) {
    const int l = idx/JJ, ij = idx - l*JJ;
    const double* base = lag + ((long long)(J*S + ij)*B + item)*rowsz + L + l;
    double v = 0.0;
    for (int c = 0; c < nc; ++c) v += base[(long long)c*slot];
    Rl[idx] = v;
    Bl[idx] = (l == 0 && ij/J == ij % J) ? 1.0 : 0.0;
  }
  // C[u] of the block index m = tid + 256 u holds d[m] until the step that creates C[m]
  double F[2][J][J], C[2][J][S];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int m = tid + 256*u;
#pragma unroll
    for (int i = 0; i < J; ++i) {
#pragma unroll
      for (int j = 0; j < J; ++j) F[u][i][j] = (m == 0 && i == j) ? 1.0 : 0.0;
#pragma unroll
      for (int e = 0; e < S; ++e) {
        double v = 0.0;
        if (m < L) {
          const double* base = lag + ((long long)(e*J + i)*B + item)*rowsz + L + m;
          for (int c = 0; c < nc; ++c) v += base[(long long)c*slot];
        }
        C[u][i][e] = v;
      }
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < J; ++i)
#pragma unroll
      for (int e = 0; e < S; ++e) part[0][i*S + e] = C[0][i][e];
  }
  __syncthreads();
  double Ef[J][J], Eb[J][J], Lff[J][J], Lfb[J][J], dif[J], dib[J], q[S];
  int fl = 0;
#pragma unroll
  for (int i = 0; i < J; ++i) {
#pragma unroll
    for (int j = 0; j < J; ++j) Ef[i][j] = Rl[i*J + j];
    if (!(Ef[i][i] > 0.0)) fl |= BRV_BSS_FLAG_NO_REFERENCE;
    Ef[i][i] += load_diag*Ef[i][i];
  }
#pragma unroll
  for (int i = 0; i < J; ++i)
#pragma unroll
    for (int j = 0; j < J; ++j) { Eb[i][j] = Ef[i][j]; Lff[i][j] = 0.0; Lfb[i][j] = 0.0; }
  if (!fl && !ldl_factor<J>(Eb, Lfb, dib)) fl |= BRV_BSS_FLAG_BAD_PIVOT;
  if (!fl) {
#pragma unroll
    for (int i = 0; i < J; ++i) {
      dif[i] = dib[i];
#pragma unroll
      for (int j = 0; j < J; ++j) Lff[i][j] = Lfb[i][j];
    }
    {
      // C[0] = R(0)^-1 d[0], refined once; q = d[0]^T C[0]
      double d0[J][S], c0[J][S], res[J][S], dc[J][S];
#pragma unroll
      for (int i = 0; i < J; ++i)
#pragma unroll
        for (int e = 0; e < S; ++e) d0[i][e] = part[0][i*S + e];
      ldl_solve<J, S>(Lfb, dib, d0, c0);
#pragma unroll
      for (int i = 0; i < J; ++i)
#pragma unroll
        for (int e = 0; e < S; ++e) {
          double v = d0[i][e];
#pragma unroll
          for (int j = 0; j < J; ++j) v = __builtin_fma(-(i >= j ? Eb[i][j] : Eb[j][i]), c0[j][e], v);
          res[i][e] = v;
        }
      ldl_solve<J, S>(Lfb, dib, res, dc);
#pragma unroll
      for (int e = 0; e < S; ++e) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < J; ++i) { c0[i][e] += dc[i][e]; v = __builtin_fma(d0[i][e], c0[i][e], v); }
        q[e] = v;
      }
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < J; ++i)
#pragma unroll
          for (int e = 0; e < S; ++e) C[0][i][e] = c0[i][e];
      }
    }
    __syncthreads();                               // part[0] is read; the loop writes it
    for (int n = 0; n + 1 < L; ++n) {
      // lane sums: Df over m <= n, Db over 1 <= m <= n + 1 (R(m)^T B[m - 1]), eps = d[n + 1] - sum over m <= n
      double af[J][J], ab[J][J], ae[J][S], Bm[2][J][J];
#pragma unroll
      for (int i = 0; i < J; ++i) {
#pragma unroll
        for (int j = 0; j < J; ++j) { af[i][j] = 0.0; ab[i][j] = 0.0; }
#pragma unroll
        for (int e = 0; e < S; ++e) ae[i][e] = 0.0;
      }
      const bool busy = wave*64 <= n + 1;          // the wave holds a block index that takes part in this step
      if (busy) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int m = tid + 256*u;
          if (m <= n) {
            const double* Rn = Rl + (n + 1 - m)*JJ;
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
              for (int k = 0; k < J; ++k) {
                const double rik = Rn[i*J + k];
#pragma unroll
                for (int j = 0; j < J; ++j) af[i][j] = __builtin_fma(rik, F[u][k][j], af[i][j]);
#pragma unroll
                for (int e = 0; e < S; ++e) ae[i][e] = __builtin_fma(-rik, C[u][k][e], ae[i][e]);
              }
          } else if (m == n + 1) {
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
              for (int e = 0; e < S; ++e) ae[i][e] += C[u][i][e];
          }
          if (m >= 1 && m <= n + 1) {
            const double* Rm = Rl + m*JJ;
            const double* Bp = Bl + (m - 1)*JJ;
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
              for (int j = 0; j < J; ++j) Bm[u][i][j] = Bp[i*J + j];
#pragma unroll
            for (int k = 0; k < J; ++k)
#pragma unroll
              for (int i = 0; i < J; ++i) {
                const double rki = Rm[k*J + i];    // R(m)^T [i][k]
#pragma unroll
                for (int j = 0; j < J; ++j) ab[i][j] = __builtin_fma(rki, Bm[u][k][j], ab[i][j]);
              }
          } else {
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
              for (int j = 0; j < J; ++j) Bm[u][i][j] = 0.0;
          }
        }
#pragma unroll
        for (int i = 0; i < J; ++i) {
#pragma unroll
          for (int j = 0; j < J; ++j) { af[i][j] = wave_sum(af[i][j]); ab[i][j] = wave_sum(ab[i][j]); }
#pragma unroll
          for (int e = 0; e < S; ++e) ae[i][e] = wave_sum(ae[i][e]);
        }
      }
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < J; ++i) {
#pragma unroll
          for (int j = 0; j < J; ++j) { part[wave][i*J + j] = af[i][j]; part[wave][JJ + i*J + j] = ab[i][j]; }
#pragma unroll
          for (int e = 0; e < S; ++e) part[wave][2*JJ + i*S + e] = ae[i][e];
        }
      }
      __syncthreads();
      double Df[J][J], Db[J][J], ep[J][S], Kf[J][J], Kb[J][J], g[J][S];
#pragma unroll
      for (int i = 0; i < J; ++i) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const int a = i*J + j;
          Df[i][j] = ((part[0][a] + part[1][a]) + part[2][a]) + part[3][a];
          Db[i][j] = ((part[0][JJ + a] + part[1][JJ + a]) + part[2][JJ + a]) + part[3][JJ + a];
        }
#pragma unroll
        for (int e = 0; e < S; ++e) {
          const int a = 2*JJ + i*S + e;
          ep[i][e] = ((part[0][a] + part[1][a]) + part[2][a]) + part[3][a];
        }
      }
      ldl_solve<J, J>(Lfb, dib, Df, Kf);           // Kf = Eb^-1 Df
      ldl_solve<J, J>(Lff, dif, Db, Kb);           // Kb = Ef^-1 Db
#pragma unroll
      for (int i = 0; i < J; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {             // the lower triangles, which is all the factorisation reads
          double vf = Ef[i][j], vb = Eb[i][j];
#pragma unroll
          for (int k = 0; k < J; ++k) {
            vf = __builtin_fma(-Db[i][k], Kf[k][j], vf);
            vb = __builtin_fma(-Df[i][k], Kb[k][j], vb);
          }
          Ef[i][j] = vf; Eb[i][j] = vb;
        }
      const bool okf = ldl_factor<J>(Ef, Lff, dif), okb = ldl_factor<J>(Eb, Lfb, dib);
      if (!(okf && okb)) { fl |= BRV_BSS_FLAG_BAD_PIVOT; break; }       // uniform: every lane has the same words
      ldl_solve<J, S>(Lfb, dib, ep, g);            // g = Eb'^-1 eps
#pragma unroll
      for (int e = 0; e < S; ++e) {
        double v = q[e];
#pragma unroll
        for (int i = 0; i < J; ++i) v = __builtin_fma(ep[i][e], g[i][e], v);
        q[e] = v;
      }
      // F'[m] = F[m] - B[m - 1] Kf, B'[m] = B[m - 1] - F[m] Kb, C'[m] = C[m] + B'[m] g for m <= n + 1 (F[n + 1] is
      // still 0, B[-1] is 0, C[n + 1] held d[n + 1] and starts from 0)
      if (busy) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int m = tid + 256*u;
          if (m <= n + 1) {
            double Bn[J][J];
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
              for (int j = 0; j < J; ++j) {
                double vf = F[u][i][j], vb = Bm[u][i][j];
#pragma unroll
                for (int k = 0; k < J; ++k) {
                  vf = __builtin_fma(-Bm[u][i][k], Kf[k][j], vf);
                  vb = __builtin_fma(-F[u][i][k], Kb[k][j], vb);
                }
                Bn[i][j] = vb;
                Bl[m*JJ + i*J + j] = vb;
                af[i][j] = vf;                     // (F[u] is still an operand of the row)
              }
#pragma unroll
            for (int i = 0; i < J; ++i) {
#pragma unroll
              for (int j = 0; j < J; ++j) F[u][i][j] = af[i][j];
#pragma unroll
              for (int e = 0; e < S; ++e) {
                double v = m == n + 1 ? 0.0 : C[u][i][e];
#pragma unroll
                for (int k = 0; k < J; ++k) v = __builtin_fma(Bn[i][k], g[k][e], v);
                C[u][i][e] = v;
              }
            }
          }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int e = 0; e < S; ++e) qj[(long long)item*S + e] = fl ? __builtin_nan("") : q[e];
    blkflags[item] = fl;
  }
}

// rows of the single-reference solves: (e J + j) B + item
__global__ __launch_bounds__(64) void bss_final_kernel(const double* __restrict__ sdr1, const double* __restrict__ q1,
                                                       const double* __restrict__ e1, const int* __restrict__ flags1,
                                                       const double* __restrict__ qj,
                                                       const int* __restrict__ blkflags, int B, int S, int J,
                                                       int permute, double* __restrict__ sdr,
                                                       double* __restrict__ sir, double* __restrict__ sar,
                                                       long long* __restrict__ perm, double* __restrict__ sdr_table,
                                                       double* __restrict__ sir_table, int* __restrict__ item_flags,
                                                       int* __restrict__ est_flags) {
  const int b = blockIdx.x*64 + threadIdx.x;
  if (b >= B) return;
  const double nan = __builtin_nan("");
  const int bf = blkflags[b];
  bool any_nan = false;
  double* st = sdr_table + (long long)b*S*J;
  double* it = sir_table + (long long)b*S*J;
  for (int e = 0; e < S; ++e) {
    const double E = e1[(long long)(e*J)*B + b], Q = qj[(long long)b*S + e], floor_ = kEps*E;
    int ef = E > 0.0 ? 0 : BRV_BSS_FLAG_NO_ESTIMATE;
    const bool dead = bf || ef;
    double a = nan;
    if (!dead) {
      const double d = E - Q;
      if (Q < floor_) ef |= BRV_BSS_FLAG_SAR_NUMERATOR_FLOOR;
      if (d < floor_) ef |= BRV_BSS_FLAG_SAR_DENOMINATOR_FLOOR;
      a = 10.0*log10((Q < floor_ ? floor_ : Q)/(d < floor_ ? floor_ : d));
    }
    sar[(long long)b*S + e] = a;
    est_flags[(long long)b*S + e] = ef;
    for (int j = 0; j < J; ++j) {
      const long long row = (long long)(e*J + j)*B + b;
      st[e*J + j] = sdr1[row];
      double v = nan;
      if (!dead && !(flags1[row] & (kNoRef | kNoEst | kPivot))) {
        const double q = q1[row], d = Q - q;
        v = 10.0*log10((q < floor_ ? floor_ : q)/(d < floor_ ? floor_ : d));
      }
      it[e*J + j] = v;
      any_nan = any_nan || v != v;
    }
  }
  // the permutations of the S estimates onto the first S references in lexicographic order: the S-digit numbers of
  // base S whose digits are all different, ascending; a strictly larger sum replaces the choice
  int best = 0;
  for (int e = 0; e < S; ++e) best = best*S + e;                         // the identity
  if (permute && !any_nan) {
    int count = 1;
    for (int e = 0; e < S; ++e) count *= S;
    double best_sum = -__builtin_inf();
    for (int code = 0; code < count; ++code) {
      int seen = 0, c = code, div = count;
      double sum = 0.0;
      bool valid = true;
      for (int e = 0; e < S; ++e) {
        div /= S;
        const int p = c/div;
        c -= p*div;
        valid = valid && !(seen >> p & 1);
        seen |= 1 << p;
        sum += it[e*J + p];
      }
      if (valid && sum > best_sum) { best_sum = sum; best = code; }
    }
  }
  int div = 1;
  for (int e = 1; e < S; ++e) div *= S;
  for (int e = 0; e < S; ++e) {
    const int p = best/div;
    best -= p*div;
    div = div > 1 ? div/S : 1;
    const long long o = (long long)b*S + e, row = (long long)(e*J + p)*B + b;
    perm[o] = p;
    sdr[o] = st[e*J + p];
    sir[o] = it[e*J + p];
    if (it[e*J + p] == it[e*J + p]) {
      const double E = e1[row], floor_ = kEps*E;
      if (q1[row] < floor_) est_flags[o] |= BRV_BSS_FLAG_SIR_NUMERATOR_FLOOR;
      if (qj[o] - q1[row] < floor_) est_flags[o] |= BRV_BSS_FLAG_SIR_DENOMINATOR_FLOOR;
    }
  }
  item_flags[b] = bf;
}

const char* kBssShape = "requires 1 <= items <= 65535, 2 <= references <= 4, 1 <= estimates <= references, "
                        "1 <= stride <= 2^40, 1 <= filter_length <= 512";

bool bss_bad_shape(int64_t B, int64_t S, int64_t J, int64_t T, int64_t L) {
  return B < 1 || B > kMaxRows || J < BRV_BSS_MIN_REFERENCES || J > kMaxJ || S < 1 || S > J || T < 1 ||
         T > (1ll << 40) || L < 1 || L > kMaxL;
}

template <int J, int S>
void bss_launch_block(const double* lag, const long long* lengths, int L, int nchunk, int B, double ld, double* qj,
                      int* blkflags, hipStream_t st) {
  hipLaunchKernelGGL((bss_block_kernel<J, S>), dim3((unsigned)B), dim3(256), 0, st, lag, lengths, L, nchunk, B, ld, qj,
                     blkflags);
}

}  // namespace

extern "C" {

int64_t brv_bss_max_references(void) { return kMaxJ; }

int64_t brv_bss_workspace_bytes(int64_t items, int64_t estimates, int64_t references, int64_t stride,
                                int64_t filter_length) {
  if (bss_bad_shape(items, estimates, references, stride, filter_length)) return brv::fail(-1, kBssShape);
  return bss_layout(items, estimates, references, stride, filter_length).total*(int64_t)sizeof(double);
}

int brv_bss_eval(const float* x, const float* s, const int64_t* lengths, int64_t items, int64_t estimates,
                 int64_t references, int64_t stride, int64_t filter_length, float load_diag, int32_t permute,
                 void* workspace, double* sdr, double* sir, double* sar, int64_t* perm, double* sdr_table,
                 double* sir_table, int32_t* item_flags, int32_t* estimate_flags, brv_stream_t stream) {
  BRV_REFUSE(!x || !s || !lengths || !workspace || !sdr || !sir || !sar || !perm || !sdr_table || !sir_table ||
                 !item_flags || !estimate_flags,
             "null pointer: x, s, lengths, workspace, sdr, sir, sar, perm, sdr_table, sir_table, item_flags and "
             "estimate_flags are required");
  BRV_REFUSE(bss_bad_shape(items, estimates, references, stride, filter_length), kBssShape);
  BRV_REFUSE(!(load_diag >= 0.f) || !(load_diag <= 1e6f), "requires 0 <= load_diag <= 1e6");
  const int64_t B = items, S = estimates, J = references, T = stride, L = filter_length;
  const BssLayout w = bss_layout(B, S, J, T, L);
  BRV_REFUSE(w.nchunk > 0x7fffffff, "requires stride <= 2^31 x 2048");
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
  float* sig = (float*)(ws + w.sig);
  long long* len = (long long*)(ws + w.lengths);
  int* flags1 = (int*)(ws + w.flags1);
  int* blkflags = (int*)(ws + w.blkflags);
  hipLaunchKernelGGL(bss_pack_kernel, brv::flat_grid(B*(J + S)*T), dim3(256), 0, st, x, s,
                     (const long long*)lengths, (long long)B, (int)S, (int)J, (long long)T, sig, len);
  // pair p < J S is (y = s_j, x = x_e) with p = e J + j; pair J S + i J + j is (y = s_i, x = s_j). Row `item` of a
  // pair starts (J + S) T floats after the row before it.
  const long long item_stride = (J + S)*T;
  for (int64_t p = 0; p < w.pairs; ++p) {
    const int64_t ix = p < J*S ? J + p/J : (p - J*S) % J, iy = p < J*S ? p % J : (p - J*S)/J;
    hipLaunchKernelGGL(sdr_corr_kernel, dim3((unsigned)w.nchunk, (unsigned)B), dim3(256), 0, st, sig + ix*T,
                       sig + iy*T, (const long long*)len, item_stride, (int)L, (int)w.nchunk,
                       ws + w.lag + p*B*w.nchunk*w.slot);
  }
  hipLaunchKernelGGL(sdr_solve_kernel, dim3((unsigned)(J*S*B)), dim3(256), 0, st, (const double*)(ws + w.lag),
                     (const long long*)len, (long long)T, (int)L, (int)w.nchunk, (double)load_diag, ws + w.sdr1,
                     ws + w.h1, ws + w.q1, ws + w.e1, flags1);
  using Launch = void (*)(const double*, const long long*, int, int, int, double, double*, int*, hipStream_t);
  static const Launch table[3][4] = {
      {bss_launch_block<2, 1>, bss_launch_block<2, 2>, nullptr, nullptr},
      {bss_launch_block<3, 1>, bss_launch_block<3, 2>, bss_launch_block<3, 3>, nullptr},
      {bss_launch_block<4, 1>, bss_launch_block<4, 2>, bss_launch_block<4, 3>, bss_launch_block<4, 4>}};
  table[J - 2][S - 1](ws + w.lag, len, (int)L, (int)w.nchunk, (int)B, (double)load_diag, ws + w.qj, blkflags, st);
  hipLaunchKernelGGL(bss_final_kernel, dim3((unsigned)((B + 63)/64)), dim3(64), 0, st, ws + w.sdr1, ws + w.q1,
                     ws + w.e1, flags1, ws + w.qj, blkflags, (int)B, (int)S, (int)J, (int)permute, sdr, sir, sar,
                     (long long*)perm, sdr_table, sir_table, (int*)item_flags, (int*)estimate_flags);
  BRV_HIP_OK(hipGetLastError());
  return 0;
}

}
