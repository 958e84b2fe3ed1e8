// The rule of the row-wise hold-out split (split.hip) and the host decisions round it: how many entries of a row are
// held out, the counter-based keys that say which, the row-length classes of the kernels, the argument checks.  The
// functions the kernels share are IRS_BPR_HD (bpr_host_prep.hpp).  No HIP in it: it compiles with the host compiler
// alone (tests/host/split_host_plan_main.cpp).  DESIGN.md section 17.
//
// The rule (normative; tests/_split_restatement.py restates it in numpy):
//   every stored entry of a canonical row (sorted columns, no duplicates) takes part, explicit zeros included;
//   j is the position of an entry in its row, m the row's length;
//   n_test(m) = floor / ceil (double(m) * ratio) in double, or min(m, n_held_out);
//   row_key = mix64(mix64(seed) ^ mix64(row + 0x53504C4954)),  key(j) = mix64(row_key ^ mix64(j));
//   held out are the n_test smallest pairs (key(j), j) in lexicographic order; both outputs keep the column order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "bpr_host_prep.hpp"
#include "host_util.hpp"

namespace irs {
namespace split {

using bpr::mix64;

constexpr int MODE_RATIO = 0;    // IRS_SPLIT_BY_RATIO
constexpr int MODE_FIXED_N = 1;  // IRS_SPLIT_BY_FIXED_N

constexpr uint64_t kRowSalt = 0x53504C4954ull;  // "SPLIT"

// ---- row-length classes ----------------------------------------------------------------------------------------
// WAVE: one wave per row, the rank of an entry by counting the smaller pairs across the lanes;
// LDS: one workgroup per row, the 64-bit keys in LDS, radix select over them (8 passes of 8 bits);
// STREAM: one workgroup per row, the same select with the keys recomputed in every pass (no key array anywhere).
constexpr int64_t kWaveMax = 64;   // longest row of the WAVE class (one entry per lane)
constexpr int64_t kLdsMax = 4096;  // longest row of the LDS class: 32 KiB of keys, five workgroups per compute unit
constexpr int kSelectThreads = 256;  // workgroup of the LDS / STREAM select and of every scatter: one thread per bin
constexpr int kRadixBits = 8, kRadixBins = 1 << kRadixBits, kRadixPasses = 64 / kRadixBits;
static_assert(kRadixBins == kSelectThreads, "thread t owns bin t of the histogram");
static_assert(kLdsMax * 8 + 4096 <= 64 * 1024, "the key image stays below the default per-block LDS limit");

enum RowClass : int { CLASS_EMPTY = 0, CLASS_WAVE = 1, CLASS_LDS = 2, CLASS_STREAM = 3 };

IRS_BPR_HD int row_class(int64_t m) {
  return m <= 0 ? CLASS_EMPTY : m <= kWaveMax ? CLASS_WAVE : m <= kLdsMax ? CLASS_LDS : CLASS_STREAM;
}

// ---- the held-out count (the reference's cpp_source/util.hpp:127-150) -------------------------------------------
struct Mode {
  int mode;            // MODE_RATIO / MODE_FIXED_N
  double ratio;        // MODE_RATIO
  int ceil;            // MODE_RATIO: ceil, else floor
  int64_t n_held_out;  // MODE_FIXED_N
};

// (the product is rounded to double before floor / ceil, as in the reference: 100 * 0.07 is 7.000000000000001, its
// ceil 8; 100 * 0.57 is 56.99999999999999, its floor 56; 10 * 0.3 rounds to 3.0 itself)
IRS_BPR_HD int64_t n_test_of(int64_t m, const Mode &md) {
  if (md.mode == MODE_FIXED_N) return m < md.n_held_out ? m : md.n_held_out;
  const double x = static_cast<double>(m) * md.ratio;
  const int64_t n = static_cast<int64_t>(md.ceil ? ceil(x) : floor(x));
  return n < 0 ? 0 : n > m ? m : n;  // (0 <= ratio <= 1 keeps it there already; a guard for the kernels' indices)
}

inline void check_mode(const Mode &md) {
  check_arg(md.mode == MODE_RATIO || md.mode == MODE_FIXED_N, "mode must be 0 (ratio) or 1 (fixed n).");
  if (md.mode == MODE_RATIO)
    check_arg(md.ratio <= 1.0 && md.ratio >= 0.0, "test_ratio must be within [0.0, 1.0]");  // (rejects NaN too)
  else
    check_arg(md.n_held_out >= 0, "n_held_out must be >= 0.");
}

inline void check_width(int32_t elem_bytes) {
  check_arg(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8,
            "the element width of data must be 1, 2, 4 or 8 bytes.");
}

// ---- the keys --------------------------------------------------------------------------------------------------
IRS_BPR_HD uint64_t row_key(uint64_t seed, int64_t row) {
  return mix64(mix64(seed) ^ mix64(static_cast<uint64_t>(row) + kRowSalt));
}
// mix64 is a bijection of the 64-bit words (an addition, two xor-shift-multiplies by odd constants, an xor-shift), so
// the keys of one row are pairwise distinct: "key <= threshold key" selects exactly the n_test smallest pairs, which
// is what the LDS / STREAM kernels use.  The tie-break on j keeps the rule total for any key function.
IRS_BPR_HD uint64_t entry_key(uint64_t rkey, int64_t j) { return mix64(rkey ^ mix64(static_cast<uint64_t>(j))); }

// ---- the rule on the host, for any key function (the reference the kernels are held against in the host test) ----
// flags[j] = 1 for the n_test smallest pairs (key(j), j)
template <class KeyFn> inline std::vector<uint8_t> held_out_flags(int64_t m, int64_t n_test, KeyFn &&key) {
  std::vector<uint64_t> k(static_cast<size_t>(m));
  std::vector<int64_t> order(static_cast<size_t>(m));
  for (int64_t j = 0; j < m; j++) k[j] = key(j), order[j] = j;
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return k[a] != k[b] ? k[a] < k[b] : a < b; });
  std::vector<uint8_t> flags(static_cast<size_t>(m), 0);
  for (int64_t q = 0; q < n_test && q < m; q++) flags[order[q]] = 1;
  return flags;
}
inline std::vector<uint8_t> held_out_flags(uint64_t seed, int64_t row, int64_t m, const Mode &md) {
  const uint64_t rk = row_key(seed, row);
  return held_out_flags(m, n_test_of(m, md), [rk](int64_t j) { return entry_key(rk, j); });
}

// ---- the plan of a call: rows per class, and the rows one workgroup each selects --------------------------------
struct Plan {
  int64_t n_class[4] = {0, 0, 0, 0};  // by RowClass
  std::vector<int32_t> long_rows;     // rows of the LDS and STREAM classes, ascending (scatter: a workgroup each)
  std::vector<int32_t> select_lds_rows, select_stream_rows;  // those of them with 0 < n_test < m, by class
  int64_t wave_select_rows = 0;       // rows of the WAVE class with 0 < n_test < m (0: the wave select is skipped)
};

inline Plan make_plan(int64_t rows, const int64_t *indptr, const Mode &md) {
  Plan p;
  for (int64_t r = 0; r < rows; r++) {
    const int64_t m = indptr[r + 1] - indptr[r];
    const int c = row_class(m);
    p.n_class[c]++;
    if (c == CLASS_EMPTY) continue;
    const int64_t n = n_test_of(m, md);
    const bool selects = n > 0 && n < m;
    if (c == CLASS_WAVE) {
      p.wave_select_rows += selects ? 1 : 0;
    } else {
      p.long_rows.push_back(static_cast<int32_t>(r));
      if (selects) (c == CLASS_LDS ? p.select_lds_rows : p.select_stream_rows).push_back(static_cast<int32_t>(r));
    }
  }
  return p;
}

// rows per workgroup of the row-pointer scan: two passes over tiles of this many rows, one block over the tile sums
constexpr int kScanThreads = 256, kScanRowsPerThread = 8, kScanTile = kScanThreads * kScanRowsPerThread;
// (rows + 1 items: the item behind the last row has count 0 and receives the total)
inline int64_t scan_tiles(int64_t rows) { return ceil_div(rows + 1, kScanTile); }

}  // namespace split
}  // namespace irs
