// The host preparation of the evaluator's model calls and the serving calls (irspack_amd/csrc/eval_host_prep.hpp)
// on its own: no HIP, built with -fsanitize=address,undefined by tests/test_host_sanitizers.py.  Every expected
// value is restated here in plain loops or plain expressions.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>

#include "../../irspack_amd/csrc/eval_host_prep.hpp"

using namespace irs;
using namespace irs::eval;

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

template <class F> static std::string error_of(F &&f) {
  try {
    f();
  } catch (const std::invalid_argument &e) {
    return e.what();
  }
  return "";
}

static const double ONE = 1.0;

static void profile_rows() {
  // 5 rows: lengths 2, 0, 3, 1, 2; a matrix of 6 columns
  const std::vector<int64_t> indptr = {0, 2, 2, 5, 6, 8};
  const std::vector<int32_t> indices = {0, 5, 1, 2, 3, 4, 0, 5};
  std::vector<double> ones(8, ONE), mixed(8, ONE);
  mixed[6] = 2.0;
  // evaluator convention: rows [begin, end) of a matrix whose first pointer is 0
  for (int64_t begin = 0; begin <= 5; begin++)
    for (int64_t end = begin; end <= 5; end++) {
      ProfileRows x;
      x.take_pointers(indptr.data(), begin, end, false);
      EXPECT(x.rows == end - begin && x.first == indptr[begin] && x.nnz == indptr[end] - indptr[begin]);
      EXPECT(static_cast<int64_t>(x.ptr.size()) == x.rows + 1);
      for (int64_t r = 0; r <= x.rows; r++) EXPECT(x.ptr[r] == indptr[begin + r] - indptr[begin]);
      x.scan_entries(indices.data(), ones.data(), 6, true);
      EXPECT(x.all_ones);
      x.scan_entries(indices.data(), mixed.data(), 6, true);
      EXPECT(x.all_ones == !(begin <= 4 && end == 5));  // (entry 6 is the first of row 4)
      x.scan_entries(indices.data(), nullptr, 6, false);  // (the dense calls: the values are not looked at)
      EXPECT(!x.all_ones);
      const bool holds_5 = indptr[begin] <= 1 && indptr[end] > 1, holds_last = end == 5 && begin <= 4;
      EXPECT((error_of([&] { x.scan_entries(indices.data(), ones.data(), 5, true); }) == "column index out of range.") ==
             (holds_5 || holds_last));
    }
  {
    ProfileRows x;
    std::vector<int64_t> shifted = {3, 5, 5};
    EXPECT(error_of([&] { x.take_pointers(shifted.data(), 0, 2, false); }) == "malformed indptr.");
    std::vector<int64_t> down = {0, 2, 1, 4};
    EXPECT(error_of([&] { x.take_pointers(down.data(), 0, 3, false); }) == "malformed indptr.");
    x.take_pointers(down.data(), 2, 3, false);  // (only the rows of the range are looked at)
    EXPECT(x.nnz == 3 && x.first == 1);
    std::vector<int32_t> neg = {0, -1};
    x.take_pointers(indptr.data(), 0, 1, false);
    EXPECT(error_of([&] { x.scan_entries(neg.data(), ones.data(), 6, true); }) == "column index out of range.");
  }
  // serve convention: rows [0, rows) from any non-negative first pointer; nothing is read without rows
  {
    ProfileRows x;
    x.take_pointers(indptr.data() + 2, 0, 3, true);  // rows 2 .. 5 of the matrix, pointers as they stand
    EXPECT(x.rows == 3 && x.first == 2 && x.nnz == 6);
    EXPECT((x.ptr == std::vector<int64_t>{0, 3, 4, 6}));
    x.scan_entries(indices.data(), mixed.data(), 6, true);  // (entries first .. first + nnz of the caller's arrays)
    EXPECT(!x.all_ones);
    x.take_pointers(indptr.data() + 1, 0, 2, true);  // an empty row first
    EXPECT(x.first == 2 && x.nnz == 3 && (x.ptr == std::vector<int64_t>{0, 0, 3}));
    x.scan_entries(indices.data(), mixed.data(), 6, true);
    EXPECT(x.all_ones);
    for (int64_t rows : {int64_t(0), int64_t(-3)}) {
      x.take_pointers(nullptr, 0, rows, true);
      EXPECT(x.rows == 0 && x.nnz == 0 && x.first == 0 && x.ptr.size() == 1 && x.ptr[0] == 0);
      x.scan_entries(nullptr, nullptr, 6, true);
      EXPECT(x.all_ones);
    }
    std::vector<int64_t> negative = {-1, 0};
    EXPECT(error_of([&] { x.take_pointers(negative.data(), 0, 1, true); }) == "malformed indptr.");
    std::vector<int64_t> down = {4, 6, 5};
    EXPECT(error_of([&] { x.take_pointers(down.data(), 0, 2, true); }) == "malformed indptr.");
  }
}

static void mask_rows() {
  const std::vector<int64_t> indptr = {4, 6, 6, 9};  // 3 rows from a first pointer of 4
  const std::vector<int32_t> in_range = {0, 9, 3, 4, 5}, stray = {0, 10, 3, -1, 5};
  MaskRows m;
  for (bool check : {false, true})
    for (bool excl : {false, true}) {
      m.take(indptr.data(), in_range.data(), 3, 10, check, excl);
      EXPECT(m.nnz == 5 && (m.ptr == std::vector<int64_t>{0, 2, 2, 5}));
      const std::string err = error_of([&] { m.take(indptr.data(), stray.data(), 3, 10, check, excl); });
      EXPECT(err == (!check ? "" : excl ? "excluded item index out of range." : "mask column index out of range."));
      if (!check) EXPECT(m.nnz == 5);
      m.take(nullptr, nullptr, 3, 10, check, excl);  // no mask
      EXPECT(m.nnz == 0 && m.ptr.empty());
      m.take(indptr.data(), in_range.data(), 0, 10, check, excl);  // no rows
      EXPECT(m.nnz == 0 && m.ptr.empty());
      const std::vector<int64_t> down = {0, 3, 2, 5};
      EXPECT(error_of([&] { m.take(down.data(), in_range.data(), 3, 10, check, excl); }) ==
             (excl ? "excl_indptr must not decrease." : "mask_indptr must not decrease."));
      EXPECT(error_of([&] { m.take(indptr.data(), nullptr, 3, 10, check, excl); }) ==
             (excl ? "excl_indices is null." : "mask_indices is null."));
    }
  // rows that hold nothing: an evaluator call has no mask and looks at nothing, a serve call checks the pointers
  const std::vector<int64_t> nothing = {7, 7, 7}, there_and_back = {2, 5, 2}, negative = {-2, 0, 1};
  m.take(nothing.data(), nullptr, 2, 10, true, false);
  EXPECT(m.nnz == 0 && m.ptr.empty());
  m.take(nothing.data(), nullptr, 2, 10, true, true);
  EXPECT(m.nnz == 0 && (m.ptr == std::vector<int64_t>{0, 0, 0}));
  m.take(there_and_back.data(), nullptr, 2, 10, true, false);
  EXPECT(m.nnz == 0);
  EXPECT(error_of([&] { m.take(there_and_back.data(), nullptr, 2, 10, true, true); }) == "excl_indptr must not decrease.");
  EXPECT(error_of([&] { m.take(negative.data(), in_range.data(), 2, 10, true, true); }) == "excl_indptr must not be negative.");
  m.take(negative.data(), in_range.data(), 2, 10, true, false);  // (a mask is read from its first entry: any base)
  EXPECT(m.nnz == 3);
}

static void orders() {
  constexpr int64_t CAP = 1 << 16;
  // lengths with ties, zeros and two rows above CAP (they tie: row order); blocks of 4 with a ragged last one
  const std::vector<int64_t> lengths = {3, 0, 3, CAP + 5, 1, CAP + 900, 0, 3, CAP, 2, 7};
  std::vector<int64_t> ptr(lengths.size() + 1, 0);
  for (size_t r = 0; r < lengths.size(); r++) ptr[r + 1] = ptr[r] + lengths[r];
  const int64_t rows = static_cast<int64_t>(lengths.size());
  for (int64_t per : {int64_t(4), int64_t(1), rows, rows + 5}) {
    std::vector<int32_t> order(3, 77);
    launch_order(ptr, rows, per, order);
    EXPECT(static_cast<int64_t>(order.size()) == rows);
    for (int64_t b = 0; b < rows; b += per) {
      const int64_t m = std::min(per, rows - b);
      std::vector<int32_t> want(static_cast<size_t>(m));
      std::iota(want.begin(), want.end(), 0);
      std::stable_sort(want.begin(), want.end(), [&](int32_t a, int32_t c) {
        return std::min(CAP, lengths[b + a]) > std::min(CAP, lengths[b + c]);
      });
      for (int64_t i = 0; i < m; i++) EXPECT(order[b + i] == want[i]);
    }
  }
  std::vector<int32_t> order(2, 1);
  launch_order(std::vector<int64_t>{0}, 0, 4, order);
  EXPECT(order.empty());
}

static void candidate_lists() {
  const std::vector<int64_t> list_ptr = {1, 6, 6, 9};  // three lists, the second empty, from a first pointer of 1
  const std::vector<int64_t> items = {99, 4, -1, 4, 10, 0, 12, 3, 9, 99};
  for (bool checked : {false, true}) {
    CandidateLists c;
    c.take(3, list_ptr.data(), items.data(), 10, checked);
    EXPECT((c.ptr == std::vector<int64_t>{0, 3, 3, 5}) && (c.items == std::vector<int32_t>{4, 4, 0, 3, 9}));  // order and duplicates kept
    EXPECT(c.max_cand == 3);
    c.take(0, nullptr, nullptr, 10, checked);
    EXPECT(c.max_cand == 10 && c.items.empty() && c.ptr.size() == 1);
    const std::vector<int64_t> one = {0, 2}, outside = {10, -5};
    c.take(1, one.data(), outside.data(), 10, checked);  // nothing is left of the list: a stand-in entry for the upload
    EXPECT(c.max_cand == 0 && (c.ptr == std::vector<int64_t>{0, 0}) && c.items.size() == 1);
    const std::vector<int64_t> empty = {0, 0};
    c.take(1, empty.data(), nullptr, 10, checked);
    EXPECT(c.max_cand == 0 && c.items.size() == 1);
  }
  CandidateLists c;
  const std::vector<int64_t> down = {2, 1}, negative = {-1, 0}, some = {0, 1};
  EXPECT(error_of([&] { c.take(1, down.data(), items.data(), 10, true); }) == "list_ptr must not decrease.");
  EXPECT(error_of([&] { c.take(1, negative.data(), items.data(), 10, true); }) == "list_ptr must not be negative.");
  EXPECT(error_of([&] { c.take(1, some.data(), nullptr, 10, true); }) == "null argument.");
  c.take(1, down.data(), items.data(), 10, false);  // (irs_retrieve_recommend: an empty walk)
  EXPECT(c.max_cand == 0);
}

// the five formulas as the entry points stated them before they shared the two functions
static int64_t atoll_env(const char *name) { return std::atoll(std::getenv(name)); }
static int64_t sim_rows(int64_t ni, int64_t rows) {
  int64_t per = std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t(1) << 32) / std::max<int64_t>(8 * ni, 1)));
  if (std::getenv("IRSPACK_AMD_EVAL_SIM_BLOCK_ROWS"))
    per = std::max<int64_t>(1, std::min<int64_t>(per, atoll_env("IRSPACK_AMD_EVAL_SIM_BLOCK_ROWS")));
  return per;
}
static int64_t dense_rows(int64_t ni, int64_t rows) {
  int64_t per = std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t(1) << 32) / std::max<int64_t>(8 * ni, 1)));
  if (per < rows && per >= 128) per = per / 128 * 128;
  if (std::getenv("IRSPACK_AMD_EVAL_SIM_BLOCK_ROWS"))
    per = std::max<int64_t>(1, std::min<int64_t>(per, atoll_env("IRSPACK_AMD_EVAL_SIM_BLOCK_ROWS")));
  return per;
}
static int64_t factor_rows(int64_t ni) {
  const int64_t fit = (int64_t(1) << 31) / (std::max<int64_t>(ni, 1) * 4);
  int64_t block_cap = 16384;
  if (std::getenv("IRSPACK_AMD_EVAL_BLOCK")) block_cap = std::max<int64_t>(256, atoll_env("IRSPACK_AMD_EVAL_BLOCK") / 128 * 128);
  return std::min<int64_t>(block_cap, std::max<int64_t>(1024, fit / 1024 * 1024));
}
static int64_t ials_rows(int64_t ni) {
  const int64_t fit = (int64_t(1) << 31) / (std::max<int64_t>(ni, 1) * 4);
  int64_t block_cap = 16384;
  if (std::getenv("IRSPACK_AMD_EVAL_BLOCK")) block_cap = std::max<int64_t>(256, atoll_env("IRSPACK_AMD_EVAL_BLOCK"));
  return std::min<int64_t>(block_cap, std::max<int64_t>(1024, fit / 1024 * 1024));
}
static int64_t serve_rows(int64_t ni) {
  const int64_t fit = (int64_t(1) << 31) / (std::max<int64_t>(ni, 1) * 4);
  int64_t block_cap = 16384;
  if (std::getenv("IRSPACK_AMD_SERVE_BLOCK")) block_cap = std::max<int64_t>(256, atoll_env("IRSPACK_AMD_SERVE_BLOCK"));
  return std::min<int64_t>(block_cap, std::max<int64_t>(1, fit >= 1024 ? fit / 1024 * 1024 : fit));
}

static void block_sizes() {
  const std::vector<int64_t> nis = {0, 1, 2, 63, 300, 2049, 26744, 32768, 40000, 131072, 262143, 262144, 262145,
                                    500000, 524287, 524288, 524289, 600000, 4000000, (int64_t(1) << 29) - 1,
                                    int64_t(1) << 29, (int64_t(1) << 29) + 1, (int64_t(1) << 31) - 1};
  const std::vector<int64_t> rowss = {0, 1, 2, 37, 127, 128, 129, 255, 256, 1000, 1024, 16383, 16384, 16385, 20074,
                                     20075, 138493, 1000000};
  const char *names[3] = {"IRSPACK_AMD_EVAL_SIM_BLOCK_ROWS", "IRSPACK_AMD_EVAL_BLOCK", "IRSPACK_AMD_SERVE_BLOCK"};
  const char *values[] = {nullptr, "0", "1", "17", "37", "127", "128", "129", "255", "256", "300", "1000", "1024", "5000",
                          "16384", "100000", "-5", "junk"};
  for (const char *v : values) {
    for (const char *n : names) {
      if (v) setenv(n, v, 1);
      else unsetenv(n);
    }
    for (int64_t ni : nis) {
      EXPECT(rows_per_f32_block(ni, "IRSPACK_AMD_EVAL_BLOCK", true, 1024) == factor_rows(ni));
      EXPECT(rows_per_f32_block(ni, "IRSPACK_AMD_EVAL_BLOCK", false, 1024) == ials_rows(ni));
      EXPECT(rows_per_f32_block(ni, "IRSPACK_AMD_SERVE_BLOCK", false, 1) == serve_rows(ni));
      for (int64_t rows : rowss) {
        EXPECT(rows_per_f64_block(ni, rows, false) == sim_rows(ni, rows));
        EXPECT(rows_per_f64_block(ni, rows, true) == dense_rows(ni, rows));
      }
    }
  }
  for (const char *n : names) unsetenv(n);
  EXPECT(rec_mode_of(0) == 0 && rec_mode_of(1) == 1 && rec_mode_of(2) == 2 && rec_mode_of(300) == 2);
}

static void weight_rows() {
  // rows: increasing; empty; out of order without a repeat; out of order with one; an equal neighbour
  const std::vector<int64_t> indptr = {0, 3, 3, 6, 10, 12};
  const std::vector<int32_t> indices = {0, 2, 5, 4, 1, 3, 2, 0, 5, 2, 1, 1};
  auto scan = [&](int64_t r0, int64_t r1, int64_t n_cols, bool dups) {
    return scan_weight_rows(indptr.data() + r0, indices.data(), r1 - r0, n_cols, dups);
  };
  WeightRowsScan w = scan(0, 2, 6, true);
  EXPECT(!w.out_of_range && !w.unsorted && !w.duplicate);
  w = scan(0, 3, 6, true);
  EXPECT(!w.out_of_range && w.unsorted && !w.duplicate);
  w = scan(0, 4, 6, true);
  EXPECT(w.unsorted && w.duplicate);
  w = scan(0, 4, 6, false);  // (the evaluator call does not ask)
  EXPECT(w.unsorted && !w.duplicate);
  w = scan(4, 5, 6, true);
  EXPECT(w.unsorted && w.duplicate && !w.out_of_range);
  w = scan(0, 1, 5, true);
  EXPECT(w.out_of_range && !w.unsorted);
  w = scan(0, 0, 6, true);
  EXPECT(!w.out_of_range && !w.unsorted && !w.duplicate);
  // many rows: the scan goes over several threads
  const int64_t n = 40000;
  std::vector<int64_t> ptr(n + 1);
  std::vector<int32_t> idx(2 * n);
  for (int64_t r = 0; r <= n; r++) ptr[r] = 2 * r;
  for (int64_t r = 0; r < n; r++) {
    idx[2 * r] = static_cast<int32_t>(r % 7);
    idx[2 * r + 1] = static_cast<int32_t>(r % 7 + 1);
  }
  w = scan_weight_rows(ptr.data(), idx.data(), n, 8, true);
  EXPECT(!w.out_of_range && !w.unsorted && !w.duplicate);
  idx[2 * 39000 + 1] = idx[2 * 39000];
  w = scan_weight_rows(ptr.data(), idx.data(), n, 8, true);
  EXPECT(!w.out_of_range && w.unsorted && w.duplicate);
  idx[2 * 20000] = -1;
  EXPECT(scan_weight_rows(ptr.data(), idx.data(), n, 8, false).out_of_range);
}

// the entry scans on enough entries for several threads
static void large_scans() {
  const int64_t n = 1200000;
  std::vector<int64_t> indptr = {0, n / 3, n};
  std::vector<int32_t> indices(n);
  std::vector<double> data(n, ONE);
  for (int64_t q = 0; q < n; q++) indices[q] = static_cast<int32_t>(q % 1000);
  ProfileRows x;
  x.take_pointers(indptr.data(), 0, 2, false);
  x.scan_entries(indices.data(), data.data(), 1000, true);
  EXPECT(x.all_ones);
  data[n - 2] = -1.0;
  x.scan_entries(indices.data(), data.data(), 1000, true);
  EXPECT(!x.all_ones);
  MaskRows m;
  m.take(indptr.data(), indices.data(), 2, 1000, true);
  EXPECT(m.nnz == n);
  indices[n - 7] = 1000;
  EXPECT(error_of([&] { x.scan_entries(indices.data(), data.data(), 1000, true); }) == "column index out of range.");
  EXPECT(error_of([&] { m.take(indptr.data(), indices.data(), 2, 1000, true); }) == "mask column index out of range.");
  m.take(indptr.data(), indices.data(), 2, 1000, false);
  EXPECT(m.nnz == n);
}

int main() {
  profile_rows();
  mask_rows();
  orders();
  candidate_lists();
  block_sizes();
  weight_rows();
  large_scans();
  std::printf("eval_host_prep ok\n");
  return 0;
}
