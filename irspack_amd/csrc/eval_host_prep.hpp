// Host-side preparation shared by the evaluator's model calls and the serving calls (no HIP dependency): checks
// and rebasing of the CSR rows a call is handed (profiles, mask / exclusion rows, candidate lists), the launch
// order inside a score block, the rows per score block, the scan of a sparse W.  Included by evaluator.hip;
// compiled on its own under AddressSanitizer + UBSan (tests/host/eval_host_prep_main.cpp).  What is checked, and
// with which words, is each entry point's own: the flags below select it.
#pragma once
#include <atomic>
#include <cstring>

#include "host_util.hpp"

namespace irs {
namespace eval {

// Rows per block of the Evaluator's host loop (`mb_size`, evaluator.py:363-367: 128 by default).  A call that
// scores a model's users on the device adds their terms as that loop does - per chunk of this many rows the
// sum of reduce_rows_kernel (what a 128-row block call returns), then Metrics::merge chunk after chunk onto the
// running totals (evaluator.cpp:76-85) - so its float64 sums are the default loop's to the last bit.
constexpr int64_t HOST_LOOP_ROWS = 128;

// Sizes that both the kernels and the host rules (eval_emit_plan.hpp) are written against: defined here once, the
// kernel headers take them from this file.
constexpr int SEL_CAP = 2048;    // largest cutoff ranked in LDS (16 KB keys + 8 KB indices)
constexpr int RANK_MAXQ = 32;    // rank_rows_kernel MODE 2: key slots per lane held in registers
constexpr int64_t HIST_DIRECT_MAX = 36864;  // largest catalogue whose item counters fit one CU's LDS
constexpr int FZ_MAX_CUTOFF = 32;  // largest cutoff of the fused paths
constexpr int EM_CAP = 1024;     // candidate slots per user
constexpr int EM_SAMPLE = 2048;  // items of the sample pass (items in catalogue order)
constexpr int EM_SAMPLE_SORTED = 512;  // ... when the items are sorted by norm (bounded variant)
constexpr int EM_SAMPLE2 = 4096;       // second-chance sample of the rows the first left hard
constexpr int EM_HARD_CAP = 2048;      // rows the second chance handles
constexpr int SF_ITEMS = 512, SF_USERS = 16;  // sample_tau_fused_kernel: items of its sample, users per tile

// EvalParams::rec_mode of a call with `n_lists` candidate lists: 0 all items, 1 one list, 2 a list per row
inline int rec_mode_of(int64_t n_lists) { return n_lists == 0 ? 0 : (n_lists == 1 ? 1 : 2); }

// A range of rows of the CSR profile matrix X, in two steps (an entry point checks other arguments in between):
// take_pointers() checks the row pointers and rebases them to the range's first entry, scan_entries() the entries.
struct ProfileRows {
  std::vector<int64_t> ptr;          // rows + 1 pointers, ptr[0] == 0
  int64_t rows = 0, first = 0, nnz = 0;  // first: offset of the range's first entry in the caller's indices / data
  bool all_ones = false;             // (only when scan_entries looked)
  // evaluator calls: rows [begin, end) of a matrix whose indptr[0] must be 0;
  // serve call (`any_first_offset`): rows [0, end) with any non-negative indptr[0], indptr unread when end <= 0
  void take_pointers(const int64_t *indptr, int64_t begin, int64_t end, bool any_first_offset) {
    rows = std::max<int64_t>(end - begin, 0);
    first = any_first_offset && end <= 0 ? 0 : indptr[0];
    check_arg(any_first_offset ? first >= 0 : first == 0, "malformed indptr.");
    for (int64_t r = begin; r < end; r++) check_arg(indptr[r + 1] >= indptr[r], "malformed indptr.");
    if (!any_first_offset) first = indptr[begin];
    nnz = rows > 0 ? indptr[end] - first : 0;
    ptr.resize(static_cast<size_t>(rows) + 1);
    ptr[0] = 0;
    for (int64_t r = 1; r <= rows; r++) ptr[r] = indptr[begin + r] - first;
  }

  // columns inside [0, n_cols); `look_for_ones`: all_ones = no stored value differs from 1.0 in a bit (the sparse
  // score kernel then reads no values; the dense one always does, and its calls skip the look)
  void scan_entries(const int32_t *indices, const double *data, int64_t n_cols, bool look_for_ones) {
    std::atomic<int> bad(0), not_ones(0);
    parallel_ranges(nnz, [&](int64_t lo, int64_t hi) {
      int32_t mn = 0, mx = 0;
      uint64_t diff = 0;
      for (int64_t q = first + lo; q < first + hi; q++) {
        mn = std::min(mn, indices[q]);
        mx = std::max(mx, indices[q]);
        if (look_for_ones) {
          uint64_t bits;
          std::memcpy(&bits, data + q, 8);
          diff |= bits ^ 0x3ff0000000000000ull;
        }
      }
      if (hi > lo && (mn < 0 || mx >= n_cols)) bad.store(1);
      if (diff) not_ones.store(1);
    });
    check_arg(bad.load() == 0, "column index out of range.");
    all_ones = look_for_ones && not_ones.load() == 0;
  }
};

// The mask rows of an evaluator call (rows + 1 pointers, NULL = no mask; `indices` starts at the first entry of
// the call's rows) or the exclusion rows of a serve call, rebased to 0.  What the entry points differ in:
//   check_columns  columns outside [0, n_items) are refused (dense-similarity, factor and serve calls); the masked
//                  and the similarity call hand them to mask_block_kernel, which skips them
//   exclusions     the serve call's wording and stricter pointers: a negative first pointer is refused, and the
//                  pointers are checked even when the rows hold nothing (an evaluator call then has no mask)
struct MaskRows {
  std::vector<int64_t> ptr;
  int64_t nnz = 0;  // > 0: there is something to upload and to mask
  void take(const int64_t *indptr, const int32_t *indices, int64_t rows, int64_t n_items, bool check_columns,
            bool exclusions = false) {
    ptr.clear();
    nnz = 0;
    if (indptr == nullptr || rows <= 0) return;
    const int64_t stored = indptr[rows] - indptr[0];
    if (exclusions) check_arg(indptr[0] >= 0, "excl_indptr must not be negative.");
    else if (stored <= 0) return;
    else check_arg(indices != nullptr, "mask_indices is null.");
    const char *decreasing = exclusions ? "excl_indptr must not decrease." : "mask_indptr must not decrease.";
    ptr.resize(static_cast<size_t>(rows) + 1);
    for (int64_t r = 0; r <= rows; r++) {
      ptr[r] = indptr[r] - indptr[0];
      check_arg(ptr[r] >= (r ? ptr[r - 1] : 0), decreasing);
    }
    nnz = stored;
    if (exclusions) check_arg(nnz == 0 || indices != nullptr, "excl_indices is null.");
    if (!check_columns) return;
    std::atomic<int> bad(0);
    parallel_ranges(nnz, [&](int64_t lo, int64_t hi) {
      int32_t mn = 0, mx = 0;
      for (int64_t q = lo; q < hi; q++) {
        mn = std::min(mn, indices[q]);
        mx = std::max(mx, indices[q]);
      }
      if (hi > lo && (mn < 0 || mx >= n_items)) bad.store(1);
    });
    check_arg(bad.load() == 0, exclusions ? "excluded item index out of range." : "mask column index out of range.");
  }
};

// Launch order inside every block of `per` rows: the block's rows by stored length, longest first (a wave lasts
// as long as its row's profile), rows of equal length in row order (counting sort; lengths above CAP count as
// CAP).  order[b + i] = row, relative to the block's first row b, that the block launches i-th.
inline void launch_order(const std::vector<int64_t> &row_ptr, int64_t rows, int64_t per, std::vector<int32_t> &order) {
  order.resize(static_cast<size_t>(std::max<int64_t>(rows, 0)));
  constexpr int64_t CAP = 1 << 16;
  std::vector<int32_t> start(CAP + 2);
  for (int64_t b = 0; b < rows; b += per) {
    const int64_t m = std::min(per, rows - b);
    std::fill(start.begin(), start.end(), 0);
    auto len = [&](int64_t r) { return std::min<int64_t>(CAP, row_ptr[b + r + 1] - row_ptr[b + r]); };
    for (int64_t r = 0; r < m; r++) start[CAP - len(r) + 1]++;
    for (size_t i = 1; i < start.size(); i++) start[i] += start[i - 1];
    for (int64_t r = 0; r < m; r++) order[b + start[CAP - len(r)]++] = static_cast<int32_t>(r);
  }
}

// Candidate lists (retrieve_recommend_from_score, util.hpp:468-472): order and duplicates kept, out-of-range ids
// dropped.  `checked`: the serve calls also refuse a negative first pointer, pointers that decrease, a null
// `list_items` under a non-empty list and 2^31 candidates or more; irs_retrieve_recommend reads the lists as they come.
struct CandidateLists {
  std::vector<int64_t> ptr;
  std::vector<int32_t> items;  // (never empty when there are lists: one 0 stands in, so that an upload has a pointer)
  int64_t max_cand = 0;        // longest filtered list; n_items without lists
  void take(int64_t n_lists, const int64_t *list_ptr, const int64_t *list_items, int64_t n_items, bool checked) {
    ptr.assign(static_cast<size_t>(n_lists) + 1, 0);
    items.clear();
    max_cand = n_lists == 0 ? n_items : 0;
    if (checked) check_arg(n_lists == 0 || list_ptr[0] >= 0, "list_ptr must not be negative.");
    for (int64_t l = 0; l < n_lists; l++) {
      if (checked) {
        check_arg(list_ptr[l + 1] >= list_ptr[l], "list_ptr must not decrease.");
        check_arg(list_ptr[l + 1] == list_ptr[l] || list_items != nullptr, "null argument.");
      }
      for (int64_t q = list_ptr[l]; q < list_ptr[l + 1]; q++)
        if (list_items[q] >= 0 && list_items[q] < n_items) items.push_back(static_cast<int32_t>(list_items[q]));
      ptr[l + 1] = static_cast<int64_t>(items.size());
      max_cand = std::max(max_cand, ptr[l + 1] - ptr[l]);
    }
    if (checked) check_arg(static_cast<int64_t>(items.size()) < (int64_t(1) << 31), "allowed lists too long.");
    if (n_lists > 0 && items.empty()) items.push_back(0);
  }
};

// Rows per score block.  The five calls, with fit32 = 2^31 / (4 max(ni, 1)), whole(f) = f >= 1024 ? f / 1024 * 1024 : f:
//
//   call                 rule                                                       override (rows)
//   _similarity          max(1, min(rows, 2^32 / max(8 ni, 1)))                     IRSPACK_AMD_EVAL_SIM_BLOCK_ROWS: min(rule, value), at least 1
//   _dense_similarity    the same, cut to whole HOST_LOOP_ROWS chunks when it is    the same, applied after the cut
//                        below `rows` and at least one chunk
//   _factors             min(cap, max(1024, whole(fit32))), cap = 16384             IRSPACK_AMD_EVAL_BLOCK: cap = max(256, value cut to whole HOST_LOOP_ROWS chunks)
//   _ials (two-pass)     the same                                                   IRSPACK_AMD_EVAL_BLOCK: cap = max(256, value), not cut
//   serve calls          min(cap, max(1, whole(fit32))), cap = 16384; then at       IRSPACK_AMD_SERVE_BLOCK: cap = max(256, value), not cut
//                        most the call's rows (at the call site)
//
// (the dense and factor calls merge their sums per HOST_LOOP_ROWS chunk, so their blocks are whole chunks)
inline int64_t rows_per_f64_block(int64_t ni, int64_t rows, bool round_to_host_chunks) {
  int64_t per = std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t(1) << 32) / std::max<int64_t>(8 * ni, 1)));
  if (round_to_host_chunks && per < rows && per >= HOST_LOOP_ROWS) per = per / HOST_LOOP_ROWS * HOST_LOOP_ROWS;
  if (const char *v = std::getenv("IRSPACK_AMD_EVAL_SIM_BLOCK_ROWS"))  // (tests: several blocks on a small call)
    per = std::max<int64_t>(1, std::min<int64_t>(per, std::atoll(v)));
  return per;
}
inline int64_t rows_per_f32_block(int64_t ni, const char *cap_env, bool round_env_to_host_chunks, int64_t floor_rows) {
  const int64_t fit = (int64_t(1) << 31) / (std::max<int64_t>(ni, 1) * 4);
  int64_t block_cap = 16384;
  const int64_t unit = round_env_to_host_chunks ? HOST_LOOP_ROWS : 1;
  if (const char *eb = std::getenv(cap_env)) block_cap = std::max<int64_t>(256, std::atoll(eb) / unit * unit);  // (read per call)
  return std::min<int64_t>(block_cap, std::max<int64_t>(floor_rows, fit >= 1024 ? fit / 1024 * 1024 : fit));
}

// The width of a model call that scores fewer columns than the evaluator ranks (the *_scored entries): the model's
// item operand covers the leading n_scored of the evaluator's n_items columns - W is [profile columns, n_scored],
// an item table [n_scored, k] - and the score kernels write those columns of a block whose row stride stays
// n_items; the columns [n_scored, n_items) hold -inf before the block is masked and ranked (a cold-user evaluator's
// feature-only items, evaluator.py:623-634), and the ranking kernels end a list at the first -inf.
inline int64_t scored_width(int64_t n_scored, int64_t n_items) {
  check_arg(n_scored > 0 && n_scored <= n_items, "n_scored must lie in 1 .. n_items.");
  return n_scored;
}

// The rows of a CSR W [n_rows, n_cols] (pointers already checked): a column outside [0, n_cols), a row whose columns
// do not strictly increase and - `want_duplicates`: such rows are sorted to find out - a column stored twice in a row.
struct WeightRowsScan { bool out_of_range, unsorted, duplicate; };
inline WeightRowsScan scan_weight_rows(const int64_t *indptr, const int32_t *indices, int64_t n_rows, int64_t n_cols,
                                       bool want_duplicates) {
  std::atomic<int> bad(0), dup(0), unsorted(0);
  parallel_ranges(n_rows, [&](int64_t lo, int64_t hi) {
    std::vector<int32_t> tmp;
    for (int64_t r = lo; r < hi; r++) {
      bool inc = true;
      for (int64_t q = indptr[r]; q < indptr[r + 1]; q++) {
        if (indices[q] < 0 || indices[q] >= n_cols) bad.store(1);
        if (q > indptr[r] && indices[q] <= indices[q - 1]) inc = false;
      }
      if (!inc) {
        unsorted.store(1);
        if (want_duplicates) {
          tmp.assign(indices + indptr[r], indices + indptr[r + 1]);
          std::sort(tmp.begin(), tmp.end());
          if (std::adjacent_find(tmp.begin(), tmp.end()) != tmp.end()) dup.store(1);
        }
      }
    }
  }, 16, 4096);
  return WeightRowsScan{bad.load() != 0, unsorted.load() != 0, dup.load() != 0};
}

}  // namespace eval
}  // namespace irs
