/* brever_bsseval.h -- the BSS-eval triple SDR / SIR / SAR (Vincent et al. 2006) of libbrever_sdr.so: the joint
 * projection of every estimate on the span of all references, each through an allowed distortion filter of
 * `filter_length` taps, on the MI355X (gfx950). A second header on the library of include/brever_sdr.h, whose
 * kernels it launches. brever_amd/bsseval.py runs it; DESIGN.md 5p states the definition.
 *
 * Per item: references s_0 .. s_{J-1} (2 <= J <= 4), estimates x_0 .. x_{S-1} (1 <= S <= J; the targets are the first
 * S references, further references are interferers only), T = min(max(lengths[item], 0), stride), L = filter_length,
 * ld = load_diag. Sums run over the t for which both indices are in [0, T).
 *   r_ij[l] = sum_t s_i[t] s_j[t + l]  (|l| < L; r_ij[-l] = r_ji[l]),   b_je[k] = sum_t s_j[t] x_e[t + k]  (k < L),
 *   E_e = sum_t x_e[t]^2
 *   single reference (brever_sdr.h):  (Toeplitz(r_jj) + ld r_jj[0] I) h = b_je,   q1[e][j] = b_je^T h
 *   joint:  sum_m R(k - m) c[m] = d[k]  (k, m < L; blocks c[m] in R^J),  R(l)[i][j] = r_ij[l],  R(-l) = R(l)^T,
 *           R(0) carries ld r_jj[0] on its diagonal,  d[k][j] = b_je[k],   qJ[e] = sum_k d[k]^T c[k]
 *   SDR[e][j] = 10 log10( max(q1, eps E) / max(E - q1, eps E) )      eps = 2^-52, E = E_e
 *   SIR[e][j] = 10 log10( max(q1, eps E) / max(qJ - q1, eps E) )
 *   SAR[e]    = 10 log10( max(qJ, eps E) / max(E - qJ, eps E) )
 * Permutation: among the S! bijections p of the estimates onto the first S references, the one with the largest
 * sum_e SIR[e][p(e)] (the sum in ascending e), the lexicographically smallest among equals; the identity where
 * `permute` is 0 or the SIR table holds a NaN. sdr[e] = SDR[e][p(e)], sir[e] = SIR[e][p(e)], sar[e] = SAR[e].
 *
 * Inputs are fp32; every sum, solve and scalar is fp64. Every reduction runs in a fixed order and there are no
 * atomics: results are bitwise repeatable, and an item gives the same bits alone as in a batch. SDR[e][j] has the bits
 * that brv_sdr_forward gives for the row (x_e, s_j): the lags and the single-reference solves are its kernels.
 *
 * brv_bss_eval launches: one pack (signals side by side, lengths clamped); the lag kernel of brever_sdr.h over the
 * J S pairs (s_j, x_e) and the J^2 ordered pairs (s_i, s_j); its Levinson solve on the J S rows; per item the block
 * Levinson recursion (Whittle-Wiggins-Robinson) of order L with J x J blocks and S right-hand sides, one workgroup,
 * the backward predictor and R in LDS, the forward predictor and the solutions in registers; one kernel for the
 * tables, the permutation and the flags.
 *
 * A pivot d of a J x J factorisation (of R(0) and of the error blocks of the recursion) counts as not positive unless
 * d > 2^-40 a_ii, a_ii being the diagonal entry it is the remainder of: below that, rounding alone decides its sign.
 *
 * item_flags (one int32 per item):
 *   BRV_BSS_FLAG_NO_REFERENCE   r_jj[0] of a reference is not positive      every SIR and SAR of the item is NaN
 *   BRV_BSS_FLAG_BAD_PIVOT      a pivot of the block recursion is not positive      "
 * estimate_flags (one int32 per item and estimate):
 *   BRV_BSS_FLAG_NO_ESTIMATE    E_e is not positive: the estimate's SDR, SIR and SAR are NaN
 *   BRV_BSS_FLAG_SAR_NUMERATOR_FLOOR / _SAR_DENOMINATOR_FLOOR    qJ < eps E / E - qJ < eps E
 *   BRV_BSS_FLAG_SIR_NUMERATOR_FLOOR / _SIR_DENOMINATOR_FLOOR    q1 < eps E / qJ - q1 < eps E at the assigned reference
 * SDR[e][j] keeps the rule of brever_sdr.h (NaN for a degenerate row of its own); SIR[e][j] is NaN with it.
 *
 * Conventions are those of include/brever_sdr.h: borrowed device pointers, the HIP stream to launch on, no
 * synchronisation, 0 ok / -1 refused argument / > 0 a hipError_t, and brv_sdr_last_error() gives the message.
 */
#ifndef BREVER_BSSEVAL_H
#define BREVER_BSSEVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brv_stream_t;          /* hipStream_t */

const char* brv_sdr_last_error(void);

#define BRV_BSS_MIN_REFERENCES 2
#define BRV_BSS_MAX_REFERENCES 4
#define BRV_BSS_MAX_FILTER_LENGTH 512
/* bits of item_flags */
#define BRV_BSS_FLAG_NO_REFERENCE 1
#define BRV_BSS_FLAG_BAD_PIVOT 4
/* bits of estimate_flags */
#define BRV_BSS_FLAG_NO_ESTIMATE 2
#define BRV_BSS_FLAG_SAR_NUMERATOR_FLOOR 8
#define BRV_BSS_FLAG_SAR_DENOMINATOR_FLOOR 16
#define BRV_BSS_FLAG_SIR_NUMERATOR_FLOOR 32
#define BRV_BSS_FLAG_SIR_DENOMINATOR_FLOOR 64

/* the largest number of references the kernels take (4) */
int64_t brv_bss_max_references(void);

/* bytes of `workspace` for brv_bss_eval (the packed signals, the per-chunk partial lags, the single-reference
 * solutions); -1 for arguments brv_bss_eval refuses */
int64_t brv_bss_workspace_bytes(int64_t items, int64_t estimates, int64_t references, int64_t stride,
                                int64_t filter_length);

/* x (items, estimates, stride) and s (items, references, stride) float; lengths (items) int64. Writes sdr, sir, sar
 * (items, estimates) double, perm (items, estimates) int64, sdr_table and sir_table (items, estimates, references)
 * double, item_flags (items) and estimate_flags (items, estimates) int32. load_diag travels as a float, as in
 * brv_sdr_forward. */
int brv_bss_eval(const float* x, const float* s, const int64_t* lengths, int64_t items, int64_t estimates,
                 int64_t references, int64_t stride, int64_t filter_length, float load_diag, int32_t permute,
                 void* workspace, double* sdr, double* sir, double* sar, int64_t* perm, double* sdr_table,
                 double* sir_table, int32_t* item_flags, int32_t* estimate_flags, brv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
