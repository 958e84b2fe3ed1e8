// Host logic of the kNN path (no HIP dependency).  Construction: the validated fp64 CSR copy, the counting-sort
// transpose (X_arg^T, knn.hpp:30-41), the weighting tables, the entry scan, the norm finish.  A compute call: chunk
// cuts, the threaded target pass, the launch order, the tile kernel's instance, the arena layout.  Included by knn.hip;
// compiled on its own under ThreadSanitizer / AddressSanitizer (tests/san/host_prep_san.cpp, tests/host/knn_host_prep_main.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>

#include "../../include/irspack_amd.h"
#include "host_util.hpp"

namespace irs {
namespace knn {

// the kernels' TILE, FAST_CAP and TOPK_CAP (knn_kernels.hpp; knn.hip asserts that they are equal)
constexpr int KNN_TILE = 16384, KNN_FAST_CAP = 2048, KNN_TOPK_CAP = 2048;

struct HostCsrD {
  int64_t rows = 0, cols = 0;
  std::vector<int64_t> indptr;
  RawVector<int32_t> indices;  // (sized, then written by several threads: no zero fill)
  RawVector<double> data;
};

// ---------------------------------------------------------------- entry scan
// "safe magnitude / positive" of the values the kernels multiply: |v| in (1e-150, 1e150) - no stored zero, no
// underflow of a product - and v > 0 (the sentinel of the fixed-point sums must not be reached by cancellation)
struct ValueClass {
  bool safe = true, positive = true;
  void add(double v, double abs_v) {
    safe &= abs_v > 1e-150 && abs_v < 1e150;
    positive &= v > 0.0;
  }
  void add(double v) { add(v, std::fabs(v)); }
};
// is every value of [b, e) bit-equal to 1.0?  (a branch-free pass the compiler vectorises)
inline bool all_ones_bits(const double *values, int64_t b, int64_t e) {
  uint64_t diff = 0;
  const uint64_t one_bits = 0x3ff0000000000000ull;
  const uint64_t *vb = reinterpret_cast<const uint64_t *>(values);
  for (int64_t q = b; q < e; q++) diff |= vb[q] ^ one_bits;
  return diff == 0;
}
// what a scan of stored entries or a target pass found: bits, so that threads merge theirs with one fetch_or
enum : unsigned { BAD_INDEX = 1, NOT_ONES = 2, NOT_SAFE = 4, NOT_POSITIVE = 8, ANY_WIDE = 16 };
// One range [b, e) of stored entries: a column index outside [0, cols); `values` (may be null: not looked
// at): one that is not 1.0 by the bit test; `classify`: the ValueClass of the range, looked for only when
// some value is not 1.
inline unsigned scan_entries(const int32_t *indices, const double *values, int64_t b, int64_t e, int64_t cols,
                             bool classify) {
  int32_t lo = 0, hi = 0;
  for (int64_t q = b; q < e; q++) {
    lo = std::min(lo, indices[q]);
    hi = std::max(hi, indices[q]);
  }
  unsigned f = e > b && (lo < 0 || hi >= cols) ? BAD_INDEX : 0u;
  if (values && !all_ones_bits(values, b, e)) {
    ValueClass vc;
    if (classify)
      for (int64_t q = b; q < e; q++) vc.add(values[q]);
    f |= NOT_ONES | (vc.safe ? 0u : NOT_SAFE) | (vc.positive ? 0u : NOT_POSITIVE);
  }
  return f;
}
// f(i) for every row i of a CSR on several host threads (row blocks of about equal entry
// counts); f must only touch its own row
template <class F>
static void for_rows_parallel(const std::vector<int64_t> &indptr, int64_t rows, F &&f) {
  const int64_t nnz = rows > 0 ? indptr[rows] : 0;
  const int n_thr = static_cast<int>(std::max<int64_t>(
      1, std::min<int64_t>({16, static_cast<int64_t>(std::thread::hardware_concurrency()), nnz / 500000 + 1})));
  auto body = [&](int k) {
    const int64_t lo = std::lower_bound(indptr.begin(), indptr.begin() + rows, nnz * k / n_thr) - indptr.begin();
    const int64_t hi = k + 1 == n_thr ? rows
                                      : std::lower_bound(indptr.begin(), indptr.begin() + rows, nnz * (k + 1) / n_thr) - indptr.begin();
    for (int64_t i = (k == 0 ? 0 : lo); i < hi; i++) f(i);
  };
  run_on_threads(n_thr, body);
}

static HostCsrD host_csr(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices, const double *data) {
  check_arg(rows >= 0 && cols >= 0 && indptr, "bad matrix.");
  HostCsrD m;
  m.rows = rows;
  m.cols = cols;
  m.indptr.assign(indptr, indptr + rows + 1);
  const int64_t nnz = indptr[rows];
  check_arg(indptr[0] == 0 && nnz >= 0, "malformed indptr.");
  // the two copies and the index check, on a few host threads (240 MB for 20 M entries)
  m.indices.resize(nnz);
  m.data.resize(nnz);
  const int n_thr = static_cast<int>(std::max<int64_t>(
      1, std::min<int64_t>({8, static_cast<int64_t>(std::thread::hardware_concurrency()), nnz / 1000000 + 1})));
  std::atomic<int> bad(0);
  run_on_threads(n_thr, [&](int k) {
    const int64_t b = nnz * k / n_thr, e = nnz * (k + 1) / n_thr;
    if (e > b) {
      std::memcpy(m.indices.data() + b, indices + b, (e - b) * sizeof(int32_t));
      std::memcpy(m.data.data() + b, data + b, (e - b) * sizeof(double));
    }
    if (scan_entries(indices, nullptr, b, e, cols, false) & BAD_INDEX) bad.store(1);
  });
  check_arg(bad.load() == 0, "column index out of range.");
  return m;
}
// X^T - its pattern only when x_data is null: what a CSC-layout target needs when every stored value is 1 - on
// several host threads: every thread owns a contiguous block of rows (about equal entry counts), counts its
// entries per column, and after a prefix over (column, thread) writes them to its own slots - the entries of
// a column stay in row order whatever the thread count.  `x_indices` must have been range-checked against x_cols.
static HostCsrD transpose_pattern(int64_t x_rows, int64_t x_cols, const int64_t *x_indptr,
                                  const int32_t *x_indices, const double *x_data /* null: pattern only */) {
  HostCsrD t;
  t.rows = x_cols;
  t.cols = x_rows;
  t.indptr.assign(t.rows + 1, 0);
  const int64_t nnz = x_indptr[x_rows];
  t.indices.resize(nnz);
  if (x_data) t.data.resize(nnz);
  // (up to 48 threads: 20 M entries on the pool's 256-thread hosts - 8 threads 25-31 ms, 16: 18-25, 32-48:
  // 13-15, 96+: no better; the pass is bound by the host's memory system)
  const int64_t cap = 48;
  const int n_thr = static_cast<int>(std::max<int64_t>(
      1, std::min<int64_t>({cap, static_cast<int64_t>(std::thread::hardware_concurrency()),
                            nnz / 500000 + 1, (int64_t(1) << 25) / std::max<int64_t>(x_cols, 1)})));
  std::vector<int64_t> row_lo(n_thr + 1, x_rows);
  row_lo[0] = 0;
  for (int k = 1; k < n_thr; k++)
    row_lo[k] = std::lower_bound(x_indptr, x_indptr + x_rows, nnz * k / n_thr) - x_indptr;
  std::vector<std::vector<int32_t>> cnt(n_thr);
  run_on_threads(n_thr, [&](int k) {
    auto &c = cnt[k];
    c.assign(static_cast<size_t>(t.rows), 0);
    for (int64_t q = x_indptr[row_lo[k]]; q < x_indptr[row_lo[k + 1]]; q++) c[x_indices[q]]++;
  });
  // slot of (column c, thread k) = prefix in that order; the threads' counters become write cursors
  // relative to the column's first slot (32 bits: a column holds fewer than 2^31 entries)
  int64_t pos = 0;
  for (int64_t c = 0; c < t.rows; c++) {
    t.indptr[c] = pos;
    int32_t within = 0;
    for (int k = 0; k < n_thr; k++) {
      const int32_t here = cnt[k][c];
      cnt[k][c] = within;
      within += here;
    }
    pos += within;
  }
  t.indptr[t.rows] = pos;
  run_on_threads(n_thr, [&](int k) {
    auto &cur = cnt[k];
    for (int64_t r = row_lo[k]; r < row_lo[k + 1]; r++)
      for (int64_t q = x_indptr[r]; q < x_indptr[r + 1]; q++) {
        const int32_t c = x_indices[q];
        const int64_t d = t.indptr[c] + cur[c]++;
        t.indices[d] = static_cast<int32_t>(r);
        if (x_data) t.data[d] = x_data[q];
      }
  });
  return t;
}

static HostCsrD transpose(const HostCsrD &x) {  // X_arg^T, knn.hpp:30-41
  return transpose_pattern(x.rows, x.cols, x.indptr.data(), x.indices.data(), x.data.data());
}
// Stored entries per column of a CSR (range-checked indices) on several host threads.
static std::vector<int64_t> column_counts(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices) {
  const int64_t nnz = indptr[rows];
  const int n_thr = static_cast<int>(std::max<int64_t>(
      1, std::min<int64_t>({16, static_cast<int64_t>(std::thread::hardware_concurrency()),
                            nnz / 1000000 + 1, (int64_t(1) << 25) / std::max<int64_t>(cols, 1)})));
  std::vector<std::vector<int32_t>> cnt(n_thr);
  run_on_threads(n_thr, [&](int k) {
    cnt[k].assign(static_cast<size_t>(cols), 0);
    auto &c = cnt[k];
    for (int64_t q = nnz * k / n_thr; q < nnz * (k + 1) / n_thr; q++) c[indices[q]]++;
  });
  std::vector<int64_t> out(static_cast<size_t>(cols), 0);
  parallel_ranges(cols, [&](int64_t b, int64_t e) {
    for (int k = 0; k < n_thr; k++)
      for (int64_t c = b; c < e; c++) out[c] += cnt[k][c];
  }, 16, 100000);
  return out;
}
// The two tables of the feature weightings (util.hpp:159-209), from the matrix AS STORED (rows = documents):
//   tf-idf : idf[c] = log(N / (df[c] + smooth))                                  (:196-203)
//   BM25   : idf[c] = log(N / (df[c] + 1) + 1), reg[r] = k1 (1 - b + b dl[r] / avgdl),
//            dl[r] = the row's values summed in entry order, avgdl = (dl summed in row order) / N   (:168-181)
// Every operation is a single IEEE double operation in the order the reference's expression has
// (this file is compiled with -ffp-contract=off); log is libm's.  `ones`: every stored value is 1.
struct WeightTables {
  std::vector<double> idf, reg;  // reg: BM25 only
};
static WeightTables weight_tables(bool bm25, int64_t rows, int64_t cols, const int64_t *indptr,
                                  const int32_t *indices, const double *data, bool ones, double k1, double b,
                                  bool smooth) {
  WeightTables w;
  const std::vector<int64_t> df = column_counts(rows, cols, indptr, indices);
  w.idf.resize(static_cast<size_t>(cols));
  const double N = static_cast<double>(rows);
  if (!bm25) {
    const double sm = smooth ? 1.0 : 0.0;
    parallel_ranges(cols, [&](int64_t lo, int64_t hi) {
      for (int64_t c = lo; c < hi; c++) w.idf[c] = std::log(N / (static_cast<double>(df[c]) + sm));
    }, 16, 20000);
    return w;
  }
  parallel_ranges(cols, [&](int64_t lo, int64_t hi) {
    for (int64_t c = lo; c < hi; c++) w.idf[c] = std::log(N / (static_cast<double>(df[c]) + 1.0) + 1.0);
  }, 16, 20000);
  std::vector<double> dl(static_cast<size_t>(rows), 0.0);
  parallel_ranges(rows, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; r++) {
      double sum = 0.0;
      if (ones) sum = static_cast<double>(indptr[r + 1] - indptr[r]);  // (a sum of 1.0s is exact)
      else
        for (int64_t q = indptr[r]; q < indptr[r + 1]; q++) sum += data[q];
      dl[r] = sum;
    }
  }, 16, 20000);
  double total = 0.0;
  for (double v : dl) total += v;
  const double avgdl = total / N;
  w.reg.resize(static_cast<size_t>(rows));
  parallel_ranges(rows, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; r++) w.reg[r] = k1 * (1 - b + b * dl[r] / avgdl);
  }, 16, 20000);
  return w;
}
// the per-entry pass of the weightings on the host (paths that never reach the device kernel)
static void weight_values_host(bool bm25, const WeightTables &w, int64_t rows, const int64_t *indptr,
                               const int32_t *indices, const double *data, double k1, double *out) {
  const std::vector<int64_t> ip(indptr, indptr + rows + 1);
  for_rows_parallel(ip, rows, [&](int64_t r) {
    for (int64_t q = indptr[r]; q < indptr[r + 1]; q++) {
      const double v = data[q];
      out[q] = bm25 ? w.idf[indices[q]] * (v * (k1 + 1)) / (v + w.reg[r]) : v * w.idf[indices[q]];
    }
  });
}
// ss -> the norm of a row of X_arg (similarities.hpp:20-28, 61-72, 96-107, 143-159): ss is the sum of the
// row's squares, or its entry count where the similarity binarises
inline double finish_norm(int32_t sim_type, double alpha, double ss) {
  switch (sim_type) {
    case IRS_SIM_COSINE: return std::sqrt(ss);
    case IRS_SIM_ASYMMETRIC: return std::pow(ss, 1 - alpha);
    default: return ss;  // (Jaccard / Tversky: the entry count; never weighted)
  }
}
// P3alpha / RP3beta (similarities.hpp:198-222, 265-292): row i pow-ed and normalised to sum 1 (libm's pow)
inline void pow_normalise_row(const int64_t *indptr, int64_t i, const double *in, double alpha, double *out) {
  double sum = 0;
  for (int64_t q = indptr[i]; q < indptr[i + 1]; q++) sum += out[q] = std::pow(in[q], alpha);
  for (int64_t q = indptr[i]; q < indptr[i + 1]; q++) out[q] /= sum;
}

// ---------------------------------------------------------------- the chunks of a compute call
// How many row chunks: IRSPACK_AMD_KNN_CHUNKS (`env`: its value or null) clamped to [1, 64], else three on
// large calls, never more than rows.
inline int chunk_count(const char *env, bool have_work, int64_t entries, int64_t n) {
  int n_chunks = 1;
  if (env) n_chunks = std::min(64, std::max(1, std::atoi(env)));
  else if (have_work && entries >= (int64_t(1) << 22) && n >= 4096) n_chunks = 3;
  return static_cast<int>(std::min<int64_t>(n_chunks, std::max<int64_t>(n, 1)));
}
// chunk k = rows [cb[k], cb[k + 1]) of [row_begin, row_end), cut at about equal entry counts; `ip` is
// monotone over the range
inline std::vector<int64_t> chunk_bounds(const int64_t *ip, int64_t row_begin, int64_t row_end, int n_chunks) {
  const int64_t e_begin = ip[row_begin], e_end = ip[row_end];
  std::vector<int64_t> cb(n_chunks + 1);
  cb[0] = row_begin;
  cb[n_chunks] = row_end;
  for (int k = 1; k < n_chunks; k++) {
    const int64_t e_cut = e_begin + static_cast<int64_t>(static_cast<double>(e_end - e_begin) * k / n_chunks);
    cb[k] = std::max<int64_t>(cb[k - 1], std::lower_bound(ip + row_begin, ip + row_end, e_cut) - ip);
  }
  return cb;
}

// ---------------------------------------------------------------- the target pass
// what the pass reads of the computer: per feature row of X_arg^T its length and the largest / smallest |x|
struct FeatureRows {
  const int64_t *len;
  const double *max, *min;
};
// IRSPACK_AMD_KNN_WIDE (`env`: its value or null): 0 = never two limbs (A/B), 1 = every weighted row
// (tests); else by the range of a row's products
struct WideRule {
  bool ok;
  double ratio;
  explicit WideRule(const char *env) : ok(!(env && env[0] == '0')), ratio((env && env[0] == '1') ? 0.0 : 2.3e5) {}
};
inline int target_pass_threads(int64_t cap, int64_t entries) {
  return static_cast<int>(std::max<int64_t>(
      1, std::min<int64_t>({cap, static_cast<int64_t>(std::thread::hardware_concurrency()), entries / 200000 + 1})));
}
// One chunk - rows [r_lo, r_hi) of the target (ip, ix, dv; `ip` monotone over the chunk) - on n_thr host
// threads: index check, the per-row statistic of the epilogue (tstat), the multiply-add count that orders
// the launch (work), the fixed-point scale (tscale; negative: two limbs), whether the values are all ones /
// safe / positive (the bits above).  The three tables are indexed by row - row_begin.  `binarise`: the values count as 1 and
// are not read (dv may be null).
inline unsigned target_pass(const int64_t *ip, const int32_t *ix, const double *dv, int64_t cols, int64_t r_lo,
                            int64_t r_hi, int64_t row_begin, const FeatureRows &xt, int32_t sim_type,
                            double alpha, bool binarise, const WideRule &wide, int n_thr, double *tstat,
                            double *tscale, int64_t *work) {
  const int64_t ce_begin = ip[r_lo], ce_end = ip[r_hi];
  std::atomic<unsigned> flags(0);
  auto body = [&](int th) {
    // contiguous row chunks of about equal entry counts
    const int64_t lo_e = ce_begin + (ce_end - ce_begin) * th / n_thr;
    const int64_t hi_e = ce_begin + (ce_end - ce_begin) * (th + 1) / n_thr;
    int64_t r0 = std::lower_bound(ip + r_lo, ip + r_hi, lo_e) - ip;
    int64_t r1 = th + 1 == n_thr ? r_hi : std::lower_bound(ip + r_lo, ip + r_hi, hi_e) - ip;
    if (th == 0) r0 = r_lo;
    bool bad = false, ones = true, wide_row = false;
    ValueClass vc;
    // The usual case - every stored value of the chunk is exactly 1 (binary interactions) -
    // is recognised by one tight pass over the values; the row loop then only walks the indices.
    bool chunk_ones = true;
    if (!binarise && r1 > r0) chunk_ones = all_ones_bits(dv, ip[r0], ip[r1]);
    const bool unit = binarise || chunk_ones;
    for (int64_t i = r0; i < r1; i++) {
      if (ip[i + 1] < ip[i]) { bad = true; break; }
      double ss = 0, bound = 0, minprod = std::numeric_limits<double>::infinity();
      int64_t w = 0;
      if (unit) {
        if (cols <= 0 && ip[i + 1] > ip[i]) { bad = true; break; }
        int32_t lo_j = 0, hi_j = 0;  // running min / max: one range test per row
        for (int64_t q = ip[i]; q < ip[i + 1]; q++) {
          const int32_t j = ix[q];
          lo_j = std::min(lo_j, j);
          hi_j = std::max(hi_j, j);
          const int32_t jc = std::min(std::max(j, 0), static_cast<int32_t>(cols - 1));
          w += xt.len[jc];
          bound += xt.max[jc];
          if (xt.min[jc] > 0.0) minprod = std::min(minprod, xt.min[jc]);
        }
        if (lo_j < 0 || hi_j >= cols) { bad = true; break; }
        ss = static_cast<double>(ip[i + 1] - ip[i]);
      } else {
        for (int64_t q = ip[i]; q < ip[i + 1]; q++) {
          const int32_t j = ix[q];
          if (j < 0 || j >= cols) { bad = true; break; }
          const double x = dv[q];  // similarities.hpp:113-118, 165-170
          ss += x * x;
          w += xt.len[j];
          ones &= x == 1.0;
          const double ax = std::fabs(x);
          vc.add(x, ax);
          bound += ax * xt.max[j];  // >= |any sum of this product row|
          if (ax > 0.0 && xt.min[j] > 0.0) minprod = std::min(minprod, ax * xt.min[j]);
        }
      }
      if (bad) break;
      switch (sim_type) {
        case IRS_SIM_COSINE: tstat[i - row_begin] = std::sqrt(ss); break;          // :39
        case IRS_SIM_ASYMMETRIC: tstat[i - row_begin] = std::pow(ss, alpha); break;  // :78-79
        case IRS_SIM_JACCARD:
        case IRS_SIM_TVERSKY:
          tstat[i - row_begin] = static_cast<double>(ip[i + 1] - ip[i]);  // :122, :174
          break;
        default: break;
      }
      work[i - row_begin] = w;
      // fixed-point scale of the row: 2^s with bound * 2^s < 2^61
      if (bound > 0 && std::isfinite(bound)) {
        int ex = 0;
        (void)std::frexp(bound, &ex);  // bound < 2^ex
        tscale[i - row_begin] = std::ldexp(1.0, 61 - ex);
        // One limb rounds every product to a multiple of 2^-s ~ bound 2^-61: 1e-13 of the row's
        // smallest possible product as long as bound / minprod < 2.3e5.  Beyond that (weights
        // over many decades, very long rows) the row is summed in two limbs (negative scale):
        // twice the accumulation time, 2^-40 of the rounding step.
        if (wide.ok && std::isfinite(minprod) && bound > wide.ratio * minprod) {
          tscale[i - row_begin] = -tscale[i - row_begin];
          wide_row = true;
        }
      }
    }
    flags.fetch_or((bad ? BAD_INDEX : 0u) | (ones ? 0u : NOT_ONES) | (vc.safe ? 0u : NOT_SAFE) |
                   (vc.positive ? 0u : NOT_POSITIVE) | (wide_row ? ANY_WIDE : 0u));
  };
  run_on_threads(n_thr, body);
  return flags.load();
}

// ---------------------------------------------------------------- the launch order of a chunk
// Heaviest rows first, for the load balance of the persistent launch only (results do not depend on it):
// a counting sort by 1/64-octave of the work, rows of a bucket in row order - O(n) instead of a 1.2 ms
// comparison sort.  (Not the evaluator's launch_order: that one buckets by length.)
constexpr int WORK_BUCKETS = 64 * 64;
inline int work_bucket(int64_t w) {
  const int b = static_cast<int>(std::log2(static_cast<double>(w) + 1.0) * 64.0);
  return WORK_BUCKETS - 1 - std::min(std::max(b, 0), WORK_BUCKETS - 1);
}
// order[slot] = row of the chunk (relative to its first row) for slot in [0, nc)
inline void heaviest_first(const int64_t *work, int64_t nc, int32_t *order) {
  std::vector<int32_t> start(WORK_BUCKETS + 1, 0);
  std::vector<int32_t> bk(nc);
  for (int64_t i = 0; i < nc; i++) {
    bk[i] = work_bucket(work[i]);
    start[bk[i] + 1]++;
  }
  for (int b = 0; b < WORK_BUCKETS; b++) start[b + 1] += start[b];
  for (int64_t i = 0; i < nc; i++) order[start[bk[i]]++] = static_cast<int32_t>(i);
}
// slot_of[row] = first_slot + slot, the inverse of `order` (slots are work-ordered inside their chunk; the
// compaction reads the inverse map)
inline void slots_of_rows(const int32_t *order, int64_t nc, int32_t first_slot, int32_t *slot_of) {
  for (int64_t sl = 0; sl < nc; sl++) slot_of[order[sl]] = static_cast<int32_t>(first_slot + sl);
}

// ---------------------------------------------------------------- accumulator and kernel variant of a chunk
// the instances of knn_tile_kernel<ONES, SENTINEL, ACC32, FAST> a chunk may be launched with
enum class TileVariant : int32_t {
  FAST_COUNTS,      // <true, true, true, true>, followed by an exact redo launch of COUNTS
  COUNTS,           // <true, true, true>
  ONES_SENTINEL,    // <true, true>
  ONES_BITMAP,      // <true, false>
  VALUES_SENTINEL,  // <false, true>
  VALUES_BITMAP     // <false, false>
};
struct VariantInputs {
  bool xt_all_ones, xt_row_const, xt_nonzero, xt_positive, col_scaled;  // the computer
  int32_t sim_type;
  bool normalize;  // (no variant depends on it)
  double alpha, beta, shrinkage, norm_max;
  bool t_all_ones, t_safe, t_positive;  // the chunk
  double tstat_max;                     // its largest per-row statistic (looked at for Tversky only)
  bool big;                             // the call: top_k above the LDS row merge
  int64_t top_k;
  bool fast_allowed;                    // IRSPACK_AMD_KNN_FAST is not 0
};
struct VariantChoice {
  TileVariant first;
  bool exact_redo;  // a second launch (COUNTS, redo = 1) takes the pairs the approximate selection handed back
  bool sentinel, acc32;  // 32-bit counts when every product is 1, else fixed-point sums with / without the sentinel
};
inline VariantChoice choose_variant(const VariantInputs &v) {
  VariantChoice c;
  // (the sentinel of the fixed-point sums needs positive data: a sum must not return to the
  // "untouched" pattern by cancellation)
  c.sentinel = v.xt_nonzero && v.t_safe && v.xt_positive && v.t_positive;
  c.acc32 = v.xt_all_ones && c.sentinel && v.t_all_ones;
  c.exact_redo = false;
  if (v.xt_all_ones) {
    // counts + a similarity that ends in a division: selection on float32 approximations, exact
    // fp64 values for the candidates only (knn_tile_kernel, FAST).  The error bound of the
    // approximation needs non-negative terms in the denominator.
    // (un-normalised cosine: the similarity IS the count - no division to save, but the 32-bit
    // select and the candidate ranking replace the 64-bit select over every column)
    const bool divides = v.sim_type == IRS_SIM_COSINE || v.sim_type == IRS_SIM_ASYMMETRIC ||
                         v.sim_type == IRS_SIM_JACCARD || v.sim_type == IRS_SIM_TVERSKY;
    // (Tversky: norms(j) - v and target_norm - v are exact in float32 only for counts below
    // 2^24; with larger ones and weights of 16 the approximation was measured at 2.1e-6 from the
    // float64 value - tests/test_knn_approx_bound.py - too close to the candidate margin)
    const bool tv_ok = v.sim_type != IRS_SIM_TVERSKY ||
                       (v.alpha >= 0.0 && v.alpha <= 16.0 && v.beta >= 0.0 && v.beta <= 16.0 &&
                        v.norm_max < 16777216.0 && v.tstat_max < 16777216.0);
    // (asymmetric cosine: norms are s^(1 - alpha) and s^alpha - inside [1, s] only for alpha in
    // [0, 1]; outside, a float32 norm may underflow where the float64 one does not)
    const bool as_ok = v.sim_type != IRS_SIM_ASYMMETRIC || (v.alpha >= 0.0 && v.alpha <= 1.0);
    // (the candidate list holds FAST_CAP columns: a request for more than half of that would send
    // most pairs to the redo list, i.e. accumulate them twice)
    // (a column scale - a separable weighting - may be zero or negative: exact values for every column)
    const bool fast = c.acc32 && !v.col_scaled && !v.big && v.top_k <= KNN_FAST_CAP / 2 && divides && tv_ok && as_ok &&
                      v.shrinkage >= 0.0 && v.shrinkage < 1e30 && v.fast_allowed;
    if (fast) {
      c.first = TileVariant::FAST_COUNTS;
      c.exact_redo = true;
    } else if (c.acc32) c.first = TileVariant::COUNTS;
    else c.first = c.sentinel ? TileVariant::ONES_SENTINEL : TileVariant::ONES_BITMAP;
  } else if (v.xt_row_const) {  // (the all-ones kernels on y' = x_u y: Params::xt_rowval)
    c.first = c.sentinel ? TileVariant::ONES_SENTINEL : TileVariant::ONES_BITMAP;
  } else {
    c.first = c.sentinel ? TileVariant::VALUES_SENTINEL : TileVariant::VALUES_BITMAP;
  }
  return c;
}

// ---------------------------------------------------------------- the scratch arena of a compute call
// ONE device allocation behind the buffers every call needs: this table is its layout, in this order, every
// block rounded up to 256 bytes (an empty one takes 256).
constexpr int ARENA_BLOCKS = 17;
struct ArenaLayout {
  size_t elem_size[ARENA_BLOCKS], count[ARENA_BLOCKS], offset[ARENA_BLOCKS], total;
};
// n target rows with ne stored entries against N columns (tiles of `tile`), out_k winners per row, the
// largest chunk `widest` rows (the candidate lists are one chunk's at a time), n_chunks chunks
inline ArenaLayout arena_layout(int64_t n, size_t ne, int64_t N, int64_t out_k, int64_t widest, int n_chunks) {
  const int64_t tile = KNN_TILE;
  const size_t nn = static_cast<size_t>(n);
  const size_t n_tiles = static_cast<size_t>(ceil_div(std::max<int64_t>(N, 1), tile));
  const size_t tile_k = static_cast<size_t>(std::min<int64_t>(out_k, tile));
  const size_t slots = static_cast<size_t>(widest) * n_tiles, cap = nn * static_cast<size_t>(out_k);
  const size_t table[ARENA_BLOCKS][2] = {
      {8, nn + 1}, {4, std::max<size_t>(ne, 1)}, {8, nn}, {8, nn},   // t_ptr, t_idx, t_stat, t_scale
      {4, nn}, {4, nn}, {8, nn + 1},                                 // order, slot_of, res_ptr
      {4, slots * tile_k}, {8, slots * tile_k}, {4, slots},          // cand_idx, cand_val, cand_cnt
      {4, cap}, {8, cap}, {4, nn}, {4, cap}, {8, cap},               // out_idx, out_val, out_cnt, res_idx, res_val
      {4, 3 * static_cast<size_t>(n_chunks)}, {4, slots}};           // cursor, redo_list
  ArenaLayout L;
  L.total = 0;
  for (int b = 0; b < ARENA_BLOCKS; b++) {
    L.elem_size[b] = table[b][0];
    L.count[b] = table[b][1];
    L.offset[b] = L.total;
    L.total += (std::max<size_t>(table[b][0] * table[b][1], 1) + 255) & ~size_t(255);
  }
  return L;
}

}  // namespace knn
}  // namespace irs
