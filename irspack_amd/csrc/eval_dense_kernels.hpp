// Scores of a DENSE item-weight model (EASE / EDLAE: W is a dense [n_profile_cols, n_items] array) on the
// device: score[u][:] = X[u][:] @ W as scipy computes it for a float64 CSR X and a dense W (csr_matvecs):
// per result row the stored entries (i, x) of the profile in STORAGE order, and for every column j
// `y[j] += x * (double)W[i][j]`, product and sum rounded separately.  Every (user, column) is its own chain
// of __dadd_rn(acc, __dmul_rn(x, w)), so any split over users and columns gives the host block bit for bit;
// the profile is read as it is stored (never sorted, never copied into another order).
//
// One wave takes one user and a strip of DS_STRIP columns; lane l owns the columns l, l + 64, ... of the
// strip, its DS_COLS sums live in registers.  A row segment of W is DS_COLS coalesced loads of one element
// per lane (no alignment needed: a row of I * 4 bytes starts anywhere).  The profile entries are fetched 64
// at a time, one per lane, and broadcast with readlane; the segments of DS_DEPTH consecutive entries are in
// flight while an earlier one is added.  The launch is strip-major with the users of a block longest profile
// first, so the waves running at one time read the same strip of W (I x DS_STRIP x 4 bytes: 27 MB on the
// ML-20M shape) out of the cache.
// (Included by evaluator.hip inside its translation unit, after readlane_f64.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace irs {
namespace eval {

constexpr int DS_COLS = 4;              // columns per lane
constexpr int DS_STRIP = 64 * DS_COLS;  // columns per wave
constexpr int DS_DEPTH = 8;             // row segments of W in flight per wave

template <class TW>  // float or double (float -> double is exact)
__global__ __launch_bounds__(64) void dense_sim_score_kernel(const int64_t *__restrict__ x_ptr,
                                                             const int32_t *__restrict__ x_idx,
                                                             const double *__restrict__ x_val,
                                                             const TW *__restrict__ w, int64_t row0, int64_t m_rows,
                                                             int64_t n_items, double *__restrict__ out,
                                                             const int32_t *__restrict__ order,
                                                             int64_t ld) {  // ld >= n_items: row stride of `out`
  const int lane = threadIdx.x;
  const int64_t unit = blockIdx.x;
  const int64_t strip = unit / m_rows;
  const int64_t r = order[unit % m_rows];
  const int64_t c0 = strip * DS_STRIP;
  const int width = static_cast<int>(min<int64_t>(DS_STRIP, n_items - c0));  // >= 1
  // (a column past the strip's end is read at the strip's last column and never stored: every load is in bounds)
  int col[DS_COLS];
#pragma unroll
  for (int c = 0; c < DS_COLS; c++) col[c] = min(lane + 64 * c, width - 1);
  double acc[DS_COLS];
#pragma unroll
  for (int c = 0; c < DS_COLS; c++) acc[c] = 0.0;
  const int64_t qb = x_ptr[row0 + r], qe = x_ptr[row0 + r + 1];
  for (int64_t q0 = qb; q0 < qe; q0 += 64) {
    const int64_t q = min(q0 + lane, qe - 1);
    const int32_t i_l = x_idx[q];
    const double x_l = x_val[q];
    const int n = static_cast<int>(min<int64_t>(64, qe - q0));
    TW seg[DS_DEPTH][DS_COLS];
    auto fetch = [&](int slot, int k) {
      const int64_t i = static_cast<int64_t>(__builtin_amdgcn_readlane(i_l, k));
      const TW *row = w + i * n_items + c0;
#pragma unroll
      for (int c = 0; c < DS_COLS; c++) seg[slot][c] = row[col[c]];
    };
#pragma unroll
    for (int d = 0; d < DS_DEPTH; d++) fetch(d, min(d, n - 1));
    for (int k0 = 0; k0 < n; k0 += DS_DEPTH) {
#pragma unroll
      for (int d = 0; d < DS_DEPTH; d++) {
        const int k = k0 + d;
        if (k < n) {  // (wave-uniform)
          const double x = readlane_f64(x_l, k);
          double wv[DS_COLS];
#pragma unroll
          for (int c = 0; c < DS_COLS; c++) wv[c] = static_cast<double>(seg[d][c]);
          if (k + DS_DEPTH < n) fetch(d, k + DS_DEPTH);  // (the slot's registers were copied: its next segment starts now)
#pragma unroll
          for (int c = 0; c < DS_COLS; c++) acc[c] = __dadd_rn(acc[c], __dmul_rn(x, wv[c]));
        }
      }
    }
  }
  double *dst = out + r * ld + c0;
#pragma unroll
  for (int c = 0; c < DS_COLS; c++)
    if (lane + 64 * c < width) dst[lane + 64 * c] = acc[c];
}

}  // namespace eval
}  // namespace irs
