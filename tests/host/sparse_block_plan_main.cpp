// irspack_amd/csrc/sparse_block_plan.hpp and csr_checks.hpp in a program of its own, for the sanitizers
// (tests/test_host_sanitizers.py builds it with -fsanitize=address,undefined, every report fatal, and at -O3):
// the segment plan, the slabs of a Gram pass and the width of a product kernel against the code they replaced,
// written out here as it stood in truncsvd_plan.hpp, truncsvd.hip and nmf.hip; the matrix checks message by
// message and in their order.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../irspack_amd/csrc/csr_checks.hpp"
#include "../../irspack_amd/csrc/sparse_block_plan.hpp"

using namespace irs;
using namespace irs::sblock;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

template <class F> static std::string message_of(F &&f) {
  try {
    f();
  } catch (const std::invalid_argument &e) {
    return e.what();
  }
  return "";
}

// ---- the former code ------------------------------------------------------------------------------------------
constexpr int OLD_SPMM_SEG = 1024, OLD_RIDGE_NB = 64;

// build_segments of truncsvd_plan.hpp up to its copies to the device
static SegmentPlan old_build_segments(const std::vector<int32_t> &ptr) {
  const int64_t rows = static_cast<int64_t>(ptr.size()) - 1;
  std::vector<int32_t> row, beg, end, slot, srow, sfirst, scount;
  int32_t n_slot = 0;
  for (int64_t r = 0; r < rows; r++) {
    const int32_t b = ptr[r], e = ptr[r + 1];
    const int32_t pieces = std::max<int32_t>(1, static_cast<int32_t>(ceil_div(e - b, OLD_SPMM_SEG)));
    if (pieces > 1) {
      srow.push_back(static_cast<int32_t>(r));
      sfirst.push_back(n_slot);
      scount.push_back(pieces);
    }
    for (int32_t k = 0; k < pieces; k++) {
      row.push_back(static_cast<int32_t>(r));
      beg.push_back(b + k * OLD_SPMM_SEG);
      end.push_back(std::min(e, b + (k + 1) * OLD_SPMM_SEG));
      slot.push_back(pieces > 1 ? n_slot++ : -1);
    }
  }
  std::vector<int32_t> order(row.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t a, int32_t b) { return end[a] - beg[a] > end[b] - beg[b]; });
  auto permuted = [&](const std::vector<int32_t> &v) {
    std::vector<int32_t> out(v.size());
    for (size_t i = 0; i < v.size(); i++) out[i] = v[order[i]];
    return out;
  };
  SegmentPlan p;
  p.seg_row = permuted(row), p.seg_begin = permuted(beg), p.seg_end = permuted(end), p.seg_slot = permuted(slot);
  p.split_row = srow, p.split_first = sfirst, p.split_count = scount;
  p.n_seg = static_cast<int64_t>(row.size());
  p.n_split = static_cast<int64_t>(srow.size());
  p.n_slot = n_slot;
  return p;
}

static int64_t old_gram_slabs(int64_t n_tile) { return std::min<int64_t>(256, std::max<int64_t>(1, 2048 / n_tile)); }

// the head of `gram` in truncsvd.hip and nmf.hip: the grid (n_tile, n_slab) and the kernel's rows per slab
static void old_gram_pass(int64_t rows, int64_t l_pad, int64_t *n_tile_out, int64_t *n_slab_out, int64_t *rows_per_slab) {
  const int64_t nb = l_pad / OLD_RIDGE_NB, n_tile = nb * (nb + 1) / 2;
  const int64_t chunks = std::max<int64_t>(1, ceil_div(rows, OLD_RIDGE_NB));
  const int64_t want_slabs = std::min(chunks, old_gram_slabs(n_tile));
  const int64_t chunks_per_slab = ceil_div(chunks, want_slabs), n_slab = ceil_div(chunks, chunks_per_slab);
  *n_tile_out = n_tile, *n_slab_out = n_slab, *rows_per_slab = chunks_per_slab * OLD_RIDGE_NB;
}

// the ladder of `spmm` in truncsvd.hip and nmf.hip and of irs_truncsvd_transform
static void old_spmm_ladder(int lvec, int *lpr, int *nch) {
  if (lvec == 16) *lpr = 16, *nch = 1;
  else if (lvec == 32) *lpr = 32, *nch = 1;
  else if (lvec <= 64) *lpr = 64, *nch = 1;
  else if (lvec <= 128) *lpr = 64, *nch = 2;
  else *lpr = 64, *nch = 3;
}

// ---- the segment plan -----------------------------------------------------------------------------------------
static std::vector<int32_t> pointers_of(const std::vector<int32_t> &lengths) {
  std::vector<int32_t> ptr = {0};
  for (int32_t n : lengths) ptr.push_back(ptr.back() + n);
  return ptr;
}

static void check_plan(const std::vector<int32_t> &lengths) {
  const std::vector<int32_t> ptr = pointers_of(lengths);
  const SegmentPlan got = plan_segments(ptr), want = old_build_segments(ptr);
  CHECK(got.seg_row == want.seg_row && got.seg_begin == want.seg_begin && got.seg_end == want.seg_end);
  CHECK(got.seg_slot == want.seg_slot && got.split_row == want.split_row && got.split_first == want.split_first);
  CHECK(got.split_count == want.split_count);
  CHECK(got.n_seg == want.n_seg && got.n_split == want.n_split && got.n_slot == want.n_slot);
  // and what the kernels rely on, stated on its own
  const size_t n_seg = static_cast<size_t>(got.n_seg);
  CHECK(got.seg_row.size() == n_seg && got.seg_begin.size() == n_seg && got.seg_end.size() == n_seg &&
        got.seg_slot.size() == n_seg);
  int64_t pieces_of_split_rows = 0;
  for (size_t q = 0; q < got.split_row.size(); q++) {
    const int32_t r = got.split_row[q], n = lengths[static_cast<size_t>(r)];
    CHECK(n > SEG_LEN && got.split_count[q] == (n + SEG_LEN - 1) / SEG_LEN);
    CHECK(got.split_first[q] == pieces_of_split_rows);
    pieces_of_split_rows += got.split_count[q];
    // the row's segments, in the order of their begin, hold the consecutive slots first, first + 1, ...
    for (int32_t k = 0; k < got.split_count[q]; k++) {
      bool found = false;
      for (size_t s = 0; s < n_seg; s++)
        if (got.seg_row[s] == r && got.seg_begin[s] == ptr[static_cast<size_t>(r)] + k * SEG_LEN) {
          CHECK(!found && got.seg_slot[s] == got.split_first[q] + k);
          found = true;
        }
      CHECK(found);
    }
  }
  CHECK(got.n_slot == pieces_of_split_rows);
  int64_t covered = 0;
  for (size_t s = 0; s < n_seg; s++) {
    const int32_t r = got.seg_row[s], len = got.seg_end[s] - got.seg_begin[s];
    CHECK(len >= 0 && len <= SEG_LEN && got.seg_begin[s] >= ptr[static_cast<size_t>(r)] &&
          got.seg_end[s] <= ptr[static_cast<size_t>(r) + 1]);
    if (lengths[static_cast<size_t>(r)] <= SEG_LEN) CHECK(got.seg_slot[s] == -1);
    if (s > 0) CHECK(len <= got.seg_end[s - 1] - got.seg_begin[s - 1]);  // longest first
    covered += len;
  }
  CHECK(covered == ptr.back());
}

static void test_plan_segments() {
  check_plan({0, 1, 1023, 1024, 1025, 2048, 2049});
  check_plan({2049, 2048, 1025, 1024, 1023, 1, 0});
  check_plan({1025, 0, 1025, 3, 3, 3, 1024, 3, 1024, 0, 1, 1, 4097, 1});  // equal lengths: the stable order
  check_plan({0, 0, 0, 0, 0});                                            // all empty: one segment per row
  check_plan({});                                                         // zero rows
  check_plan({5});
  // among segments of equal length the order is that of the rows, then of the pieces
  const SegmentPlan p = plan_segments(pointers_of({3, 2048, 3, 1024, 3}));
  CHECK((p.seg_row == std::vector<int32_t>{1, 1, 3, 0, 2, 4}));
  CHECK((p.seg_begin == std::vector<int32_t>{3, 1027, 2054, 0, 2051, 3078}));
  CHECK((p.seg_slot == std::vector<int32_t>{0, 1, -1, -1, -1, -1}));
  CHECK((p.split_row == std::vector<int32_t>{1}) && (p.split_first == std::vector<int32_t>{0}) &&
        (p.split_count == std::vector<int32_t>{2}));
  const SegmentPlan none = plan_segments(std::vector<int32_t>{0});
  CHECK(none.n_seg == 0 && none.n_split == 0 && none.n_slot == 0 && none.seg_row.empty() && none.split_row.empty());
  const SegmentPlan empty = plan_segments(pointers_of({0, 0, 0}));
  CHECK(empty.n_seg == 3 && empty.n_split == 0 && empty.n_slot == 0);
  CHECK((empty.seg_row == std::vector<int32_t>{0, 1, 2}) && (empty.seg_slot == std::vector<int32_t>{-1, -1, -1}));
}

// ---- the Gram pass and the width ------------------------------------------------------------------------------
static void test_plan_gram_pass() {
  CHECK(SEG_LEN == OLD_SPMM_SEG && TILE_EDGE == OLD_RIDGE_NB && MAX_L_PAD == 576);
  for (int64_t l_pad = 64; l_pad <= 576; l_pad += 64) {
    const int64_t nb = l_pad / 64, n_tile = nb * (nb + 1) / 2;
    CHECK(gram_slabs(n_tile) == old_gram_slabs(n_tile));
    for (int64_t rows : {int64_t(0), int64_t(1), int64_t(63), int64_t(64), int64_t(65), int64_t(64 * 256),
                         int64_t(64 * 256 + 1), int64_t(1000000)}) {
      int64_t n_tile_old, n_slab, rows_per_slab;
      old_gram_pass(rows, l_pad, &n_tile_old, &n_slab, &rows_per_slab);
      const GramPass g = plan_gram_pass(rows, l_pad);
      CHECK(g.n_tile == n_tile_old && g.n_tile == n_tile && g.n_slab == n_slab && g.rows_per_slab == rows_per_slab);
      // the slabs cover the rows, none is empty, and the partial buffer (gram_slabs(n_tile) slabs) holds them
      CHECK(g.n_slab >= 1 && g.n_slab <= gram_slabs(n_tile) && g.rows_per_slab % 64 == 0);
      CHECK(g.n_slab * g.rows_per_slab >= rows && (g.n_slab - 1) * g.rows_per_slab < std::max<int64_t>(rows, 1));
    }
  }
}

static void test_spmm_width() {
  for (int l_pad = 64; l_pad <= 576; l_pad += 64) {
    const int lvec = l_pad / 4;  // 16, 32, ..., 144
    int lpr, nch;
    old_spmm_ladder(lvec, &lpr, &nch);
    const SpmmWidth w = spmm_width(lvec);
    CHECK(w.lpr == lpr && w.nch == nch);
    CHECK(w.lpr * w.nch >= lvec);  // the lanes of a row cover its float4 columns
  }
}

// ---- the matrix checks ----------------------------------------------------------------------------------------
struct Matrix {
  int64_t rows, cols;
  std::vector<int64_t> indptr;
  std::vector<int32_t> indices;
  std::vector<float> data;
};

static std::string csr(const Matrix &x) {
  return message_of([&] { validate_csr(x.rows, x.cols, x.indptr.data(), x.indices.data(), x.data.data()); });
}
static std::string finite(const Matrix &x) {
  return message_of([&] { validate_finite_matrix(x.rows, x.cols, x.indptr.data(), x.indices.data(), x.data.data()); });
}

static void test_matrix_checks() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const char *DUP = "duplicate column index in a row (sum duplicates before the call).";
  const char *SORTED = "column indices of a row must be sorted.";
  const char *RANGE = "column index out of range.";
  const char *SHAPE = "the matrix must have at least one row and one column.";
  const char *FINITE = "the matrix holds a non-finite value.";
  // 3 x 5: rows {0, 3}, {}, {1, 2, 4}
  const Matrix m{3, 5, {0, 2, 2, 5}, {0, 3, 1, 2, 4}, {1.f, 2.f, -1.f, 0.f, 3.f}};
  CHECK(csr(m).empty() && finite(m).empty());
  CHECK(validate_csr(m.rows, m.cols, m.indptr.data(), m.indices.data(), m.data.data()) == 5);
  CHECK(validate_finite_matrix(m.rows, m.cols, m.indptr.data(), m.indices.data(), m.data.data()) == 5);
  for (auto check : {csr, finite}) {
    // each message at its first failing condition
    Matrix bad = m;
    bad.rows = -1;
    CHECK(check(bad) == "bad matrix.");
    bad = m, bad.cols = -1;
    CHECK(check(bad) == "bad matrix.");
    bad = m, bad.indptr[0] = 1;
    CHECK(check(bad) == "bad matrix.");
    CHECK(message_of([&] { validate_csr(3, 5, nullptr, m.indices.data(), m.data.data()); }) == "bad matrix.");
    bad = m, bad.cols = (int64_t(1) << 31) - 1;
    CHECK(check(bad) == "rows and cols must be below 2^31.");
    bad = m, bad.indptr[2] = 1;
    CHECK(check(bad) == "malformed indptr.");
    bad = m, bad.rows = 2, bad.indptr = {0, 0, int64_t(1) << 31};  // (nothing past the pointers is read)
    CHECK(check(bad) == "nnz must be below 2^31.");
    bad = m, bad.indices[1] = 5;
    CHECK(check(bad) == RANGE);
    bad = m, bad.indices[2] = -1;  // (equal to the "previous" of a row's first entry: the range speaks first)
    CHECK(check(bad) == RANGE);
    bad = m, bad.indices[1] = -1;  // (and below the entry before it)
    CHECK(check(bad) == RANGE);
    bad = m, bad.indices[1] = 0;
    CHECK(check(bad) == DUP);
    bad = m, bad.indices[3] = 0;
    CHECK(check(bad) == SORTED);
    // precedence: the range before both, a duplicate before an unsorted pair (the first bad entry decides)
    bad = m, bad.indices = {0, 0, 1, 0, 7};
    CHECK(check(bad) == DUP);
    bad = m, bad.indices = {3, 0, 1, 1, 4};
    CHECK(check(bad) == SORTED);
    bad = m, bad.indices = {0, 9, 1, 1, 0};
    CHECK(check(bad) == RANGE);
    bad = m, bad.indices = {0, 3, 2, 2, 9};
    CHECK(check(bad) == DUP);
    // malformed pointers before the indices
    bad = m, bad.indptr[2] = 1, bad.indices[0] = 9;
    CHECK(check(bad) == "malformed indptr.");
  }
  // nnz == 0: the index and value arrays may be null; with entries they may not
  const std::vector<int64_t> zeros = {0, 0, 0};
  CHECK(validate_csr(2, 4, zeros.data(), nullptr, nullptr) == 0);
  CHECK(validate_finite_matrix(2, 4, zeros.data(), nullptr, nullptr) == 0);
  CHECK(message_of([&] { validate_csr(3, 5, m.indptr.data(), nullptr, m.data.data()); }) == "bad matrix.");
  CHECK(message_of([&] { validate_csr(3, 5, m.indptr.data(), m.indices.data(), nullptr); }) == "bad matrix.");
  CHECK(message_of([&] { validate_finite_matrix(3, 5, m.indptr.data(), m.indices.data(), nullptr); }) == "bad matrix.");
  // rows == 0 (and cols == 0): a CSR matrix, not a matrix to fit
  const std::vector<int64_t> one = {0};
  CHECK(validate_csr(0, 4, one.data(), nullptr, nullptr) == 0 && validate_csr(0, 0, one.data(), nullptr, nullptr) == 0);
  CHECK(validate_csr(2, 0, zeros.data(), nullptr, nullptr) == 0);
  CHECK(message_of([&] { validate_finite_matrix(0, 4, one.data(), nullptr, nullptr); }) == SHAPE);
  CHECK(message_of([&] { validate_finite_matrix(2, 0, zeros.data(), nullptr, nullptr); }) == SHAPE);
  // every value finite, checked last: the CSR checks before the shape before the values
  for (float v : {nan, inf, -inf}) {
    Matrix bad = m;
    bad.data[4] = v;
    CHECK(csr(bad).empty() && finite(bad) == FINITE);
    bad.indices[3] = 0;
    CHECK(finite(bad) == SORTED);
    bad = m, bad.data[0] = v, bad.indices[4] = 5;
    CHECK(finite(bad) == RANGE);
  }
  Matrix no_cols{1, 0, {0, 1}, {0}, {nan}};
  CHECK(finite(no_cols) == RANGE);  // (an entry needs a column: the CSR check speaks first)
  Matrix no_rows{0, 3, {0}, {}, {}};
  CHECK(csr(no_rows).empty() && finite(no_rows) == SHAPE);
}

int main() {
  test_plan_segments();
  test_plan_gram_pass();
  test_spmm_width();
  test_matrix_checks();
  std::printf("sparse_block_plan ok\n");
  return 0;
}
