// The host side that the three families of entry points of libbrever_rir.so share (rir.hip, rir_bands.cuh,
// rir_hrir.cuh): the options and the job as every family sees them, the checks of a job and of a launch, the
// candidates of an axis, and the loop that counts or writes the tables of a batch.
//
//   build_axis   the candidates of one axis of one job: (offset x_img - r, e0 + e1, offset^2, b0^e0 b1^e1 of every
//                band) for every (n, p) within reach of the last tap, in ascending order of offset^2 (ties in (n, p)
//                order), so that "inside a distance shell" is a prefix of x, a prefix of y and, for a given (x, y)
//                pair, one contiguous range of z. A candidate leaves only if every band's amplitude is 0. The base
//                path is one band, and writes its own column order.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../../include/rir/brever_rir_bands.h"

namespace {

constexpr int kRow = BRV_RIR_ROW_DOUBLES, kShape = BRV_RIR_SHAPE_WORDS, kIdx = BRV_RIR_INDEX_WORDS;
constexpr int kMaxAxis = BRV_RIR_MAX_AXIS_ROWS;
// samples by which a reach or a shell is widened; the taps test |u| < W/2 exactly
constexpr double kSlack = 1e-6;
constexpr int kMaxBands = BRV_RIR_BANDS_MAX_BANDS, kMaxFilter = BRV_RIR_BANDS_MAX_FILTER;

// the options of a batch; the base path is one band in pattern mode without a pad
struct Opts {
  double fs, c, W, rad;
  int K, mode, C;
  int64_t pad;
};

// a job's view of the host arrays
struct Job {
  const double *L, *beta;                       // beta[6 b + 2 k + w]: band b, axis k, wall w
  const double *s, *r;
  const double *o, *l;                          // the orientation and nothing, or the head's front and left
  double a;                                     // the pattern coefficient (not of a measured ear)
  int64_t taps, off, stride, ear;               // ear: the offset of the second ear (a measured ear only)
};

enum Family { kBase, kBands, kMeasured };

// a candidate of an axis with its K amplitudes (K is a compile-time value so that the sort moves no more than it has to)
template <int K> struct AxisRow { double d, count, d2, amp[K]; };

bool finite_positive(double v) { return v > 0.0 && v <= 1.79e308; }

const char* kTooMany = "an axis has more than BRV_RIR_MAX_AXIS_ROWS (1024) candidates: fewer taps or a larger room";
const char* kNeedsOrder = "requires max_order >= -1";

std::string jobs_why(int64_t n_jobs) {
  if (n_jobs < 1 || n_jobs > BRV_RIR_MAX_JOBS) return "requires 1 <= n_jobs <= " + std::to_string(BRV_RIR_MAX_JOBS);
  return "";
}

// "" or why fs, c and W, the first three options of every family, are refused
std::string rate_why(const double* opts) {
  if (!finite_positive(opts[0]) || !finite_positive(opts[1])) return "requires fs > 0 and c > 0, both finite";
  if (!(opts[2] >= 2.0) || !(opts[2] <= 1e6)) return "requires 2 <= W <= 1e6 (the window in samples)";
  return "";
}

// "" or why a launch over n_jobs index rows of a table of n_rows rows (1 where the launch reads no table) and
// max_taps taps is refused
std::string launch_why(int64_t n_jobs, int64_t n_rows, int64_t max_taps) {
  const std::string why = jobs_why(n_jobs);
  if (!why.empty()) return why;
  if (n_rows < 1) return "requires n_rows >= 1";
  if (max_taps < 1 || max_taps > BRV_RIR_MAX_TAPS) return "requires 1 <= max_taps <= " + std::to_string(BRV_RIR_MAX_TAPS);
  return "";
}

// "" or why the job is refused: K bands; rad is the head radius in sphere mode and 0 otherwise
std::string job_why(const Job& q, Family family, int K, double rad) {
  const bool measured = family == kMeasured;
  double dist2 = 0.0, norm2 = 0.0, l2 = 0.0, fl = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!finite_positive(q.L[k])) return "requires room dimensions > 0, finite";
    for (int b = 0; b < K; ++b)
      for (int w = 0; w < 2; ++w) {
        const double v = q.beta[6*b + 2*k + w];
        if (!(v >= 0.0) || !(v <= 1.0)) return family == kBase ? "requires beta in [0, 1]"
                                                               : "requires beta in [0, 1] in every band";
      }
    if (!(q.s[k] > 0.0) || !(q.s[k] < q.L[k])) return "the source is outside the box or on a wall";
    if (!(q.r[k] > 0.0) || !(q.r[k] < q.L[k])) return measured ? "the head is outside the box or on a wall"
                                                               : "the receiver is outside the box or on a wall";
    if (rad > 0.0 && (!(q.r[k] - rad > 0.0) || !(q.r[k] + rad < q.L[k])))
      return "the head reaches a wall: its centre is nearer than the head radius";
    dist2 += (q.s[k] - q.r[k])*(q.s[k] - q.r[k]);
    norm2 += q.o[k]*q.o[k];
    if (measured) { l2 += q.l[k]*q.l[k]; fl += q.o[k]*q.l[k]; }
  }
  if (rad > 0.0 && !(dist2 > rad*rad)) return "the source is inside the sphere of the head";
  if (!(dist2 >= 1e-6))
    return std::string(measured ? "the source is at the head's centre: " : "") +
           "requires a direct path of at least 1e-3 m";
  if (measured) {
    if (!(fabs(norm2 - 1.0) <= 1e-9) || !(fabs(l2 - 1.0) <= 1e-9) || !(fabs(fl) <= 1e-9))
      return "requires unit front and left vectors at right angles";
    if (q.o[2] != 0.0 || q.l[2] != 0.0) return "requires an upright head: horizontal front and left vectors";
  } else {
    if (!(fabs(norm2 - 1.0) <= 1e-9)) return "requires a unit orientation vector";
    if (!(q.a >= 0.0) || !(q.a <= 1.0)) return "requires a pattern coefficient in [0, 1]";
  }
  if (q.taps < 1 || q.taps > BRV_RIR_MAX_TAPS) return "requires 1 <= taps <= " + std::to_string(BRV_RIR_MAX_TAPS);
  if (q.off < 0 || q.off > (1ll << 40)) return "requires 0 <= out_offset <= 2^40";
  if (q.stride < 1 || q.stride > 1024) return "requires 1 <= out_stride <= 1024";
  if (measured && (q.ear < 1 || q.ear > (1ll << 40))) return "requires 1 <= ear_offset <= 2^40";
  return "";
}

// The candidates of axis k of a job; false if there are more than the limit.
template <int K>
bool build_axis(const Job& q, int k, const Opts& o, int64_t max_order, std::vector<AxisRow<K>>* rows) {
  const double L = q.L[k];
  // the last tap of a channel row is taps + pad - 1, and delta >= -rad brings an image of distance reach in
  const double reach = (o.c/o.fs)*((double)(q.taps + o.pad - 1) + 0.5*o.W + kSlack) +
                       (o.mode == BRV_RIR_BANDS_SPHERE ? o.rad : 0.0);
  rows->clear();
  if (reach/L > 4.0*kMaxAxis) return false;
  const long long N = (long long)ceil((reach + L)/(2.0*L)) + 1;
  for (long long n = -N; n <= N; ++n) {
    for (int p = 0; p < 2; ++p) {
      const double x = (1.0 - 2.0*p)*q.s[k] + 2.0*(double)n*L;
      const double d = x - q.r[k];
      if (fabs(d) > reach) continue;
      const long long e0 = n - p < 0 ? p - n : n - p, e1 = n < 0 ? -n : n;
      if (max_order >= 0 && e0 + e1 > max_order) continue;
      AxisRow<K> row{d, (double)(e0 + e1), d*d, {}};
      bool any = false;
      for (int b = 0; b < K; ++b) {
        row.amp[b] = pow(q.beta[6*b + 2*k], (double)e0)*pow(q.beta[6*b + 2*k + 1], (double)e1);   // pow(0, 0) = 1
        any = any || row.amp[b] != 0.0;
      }
      if (any) rows->push_back(row);
    }
  }
  if ((long long)rows->size() > kMaxAxis) return false;
  std::stable_sort(rows->begin(), rows->end(), [](const AxisRow<K>& u, const AxisRow<K>& v) { return u.d2 < v.d2; });
  return true;
}

// The jobs job_at(0 .. n_jobs - 1) checked, then their tables counted into *total if rows_out is null, else written to
// the n_rows rows of rows_out with index words 0 to 3 of every job; head(j, job, header row, index row) writes the
// header row (cleared before) and the index words 4 to 7, once the job's axes are written. counter names the entry
// point whose value n_rows has to be. K is o.K. Returns "" or the refusal.
template <int K, class JobAt, class Head>
std::string tables(int64_t n_jobs, JobAt job_at, Family family, const Opts& o, int64_t max_order, const char* counter,
                   double* rows_out, int64_t* index, int64_t n_rows, int64_t* total, Head head) {
  for (int64_t j = 0; j < n_jobs; ++j) {
    const std::string why = job_why(job_at(j), family, K, o.mode == BRV_RIR_BANDS_SPHERE ? o.rad : 0.0);
    if (!why.empty()) return "job " + std::to_string(j) + ": " + why;
  }
  const std::string not_rows = std::string("n_rows is not what ") + counter + " gives for this batch";
  if (rows_out && n_rows < 1) return std::string("requires n_rows >= 1: the value of ") + counter;
  const int RW = family == kBase ? kRow : 3 + K;
  std::vector<AxisRow<K>> rows;
  int64_t at = 0;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const Job q = job_at(j);
    if (rows_out) {
      if (at + 1 > n_rows) return not_rows;
      index[j*kIdx] = at;
      for (int i = 0; i < RW; ++i) rows_out[at*RW + i] = 0.0;
    }
    const int64_t header = at++;
    for (int k = 0; k < 3; ++k) {
      if (!build_axis(q, k, o, max_order, &rows)) return "job " + std::to_string(j) + ": " + kTooMany;
      if (rows_out) {
        if (at + (int64_t)rows.size() > n_rows) return not_rows;
        index[j*kIdx + 1 + k] = (int64_t)rows.size();
        double* w = rows_out + at*RW;
        for (const AxisRow<K>& r : rows) {
          if (family == kBase) {
            w[0] = r.d; w[1] = r.amp[0]; w[2] = r.count; w[3] = r.d2;
          } else {
            w[0] = r.d; w[1] = r.count; w[2] = r.d2;
            for (int b = 0; b < K; ++b) w[3 + b] = r.amp[b];
          }
          w += RW;
        }
      }
      at += (int64_t)rows.size();
    }
    if (rows_out) head(j, q, rows_out + header*RW, index + j*kIdx);
  }
  if (rows_out && at != n_rows) return not_rows;
  *total = at;
  return "";
}

// f(std::integral_constant<int, K>) for the K of a batch, 1 to kMaxBands
template <class F> auto with_bands(int K, F f) -> decltype(f(std::integral_constant<int, 1>{})) {
  static_assert(kMaxBands == 8, "one case per number of bands");
  switch (K) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
  }
  return {};
}

}  // namespace
