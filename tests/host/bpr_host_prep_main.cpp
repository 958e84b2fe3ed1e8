// irspack_amd/csrc/bpr_host_prep.hpp in a program of its own, for the sanitizers (tests/test_bpr_surface.py builds
// it with -fsanitize=address,undefined, every report fatal): the filter of the positives, the argument checks, the
// permutation, the unseen-rank mapping against a plain scan, whole epochs sampled on the host, the scale bound.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "../../irspack_amd/csrc/bpr_host_prep.hpp"
#include "../../irspack_amd/csrc/csr_checks.hpp"

using namespace irs;
using namespace irs::bpr;

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

struct Matrix {
  int64_t rows, cols;
  std::vector<int64_t> indptr;
  std::vector<int32_t> indices;
  std::vector<float> data;
};

// 6 x 5: an empty row, a full row, a row with all items but one, a row whose only entry is not positive
static Matrix small_matrix() {
  Matrix m{6, 5, {0}, {}, {}};
  const std::vector<std::vector<std::pair<int, float>>> rows = {
      {{0, 1.f}, {3, 2.f}},
      {},
      {{0, 1.f}, {1, 1.f}, {2, 1.f}, {3, 1.f}, {4, 1.f}},
      {{0, 1.f}, {1, 1.f}, {3, 1.f}, {4, 1.f}},
      {{2, 0.f}},
      {{1, -1.f}, {2, 0.5f}, {4, 3.f}}};
  for (const auto &r : rows) {
    for (const auto &e : r) m.indices.push_back(e.first), m.data.push_back(e.second);
    m.indptr.push_back(static_cast<int64_t>(m.indices.size()));
  }
  return m;
}

static void test_filter_and_sampling() {
  const Matrix m = small_matrix();
  CHECK(validate_finite_matrix(m.rows, m.cols, m.indptr.data(), m.indices.data(), m.data.data()) == 15);
  const Positives p = filter_positives(m.rows, m.cols, m.indptr.data(), m.indices.data(), m.data.data());
  CHECK(p.n_positives == 13 && p.n_skipped_rows == 1 && p.n_skipped_positives == 5);
  CHECK((p.indptr == std::vector<int32_t>{0, 2, 2, 7, 11, 11, 13}));
  CHECK((p.pos_user == std::vector<int32_t>{0, 0, 3, 3, 3, 3, 5, 5}));
  CHECK((p.pos_item == std::vector<int32_t>{0, 3, 0, 1, 3, 4, 2, 4}));
  const int64_t n = static_cast<int64_t>(p.pos_user.size());
  std::set<int32_t> negatives_of_0;
  std::vector<uint32_t> first_order;
  for (int64_t epoch = 0; epoch < 50; epoch++) {
    const Perm perm = make_perm(epoch_key(42, epoch, 0), n);
    const uint64_t neg_key = epoch_key(42, epoch, 1);
    std::vector<int> used(static_cast<size_t>(n), 0);
    std::vector<uint32_t> order;
    for (int64_t pos = 0; pos < n; pos++) {
      const uint32_t e = permute(perm, static_cast<uint32_t>(pos));
      CHECK(e < n);
      used[e]++;
      order.push_back(e);
      int32_t u, i, j;
      sample_one(p, m.cols, perm, neg_key, pos, &u, &i, &j);
      CHECK(u == p.pos_user[e] && i == p.pos_item[e] && j >= 0 && j < m.cols);
      for (int32_t q = p.indptr[u]; q < p.indptr[u + 1]; q++) CHECK(p.indices[q] != j);
      if (u == 3) CHECK(j == 2);  // (its one unseen item)
      if (u == 0) negatives_of_0.insert(j);
    }
    for (int c : used) CHECK(c == 1);  // a bijection
    if (epoch == 0) first_order = order;
    if (epoch == 1) CHECK(order != first_order);
  }
  CHECK((negatives_of_0 == std::set<int32_t>{1, 2, 4}));
}

static void test_permutation_sizes() {
  for (int64_t n : {1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1000, 4097, 70001}) {
    const Perm perm = make_perm(epoch_key(7, n, 0), n);
    CHECK((int64_t(1) << (2 * perm.half)) >= n && (n <= 4 || (int64_t(1) << (2 * perm.half)) < 4 * n));
    std::vector<char> seen(static_cast<size_t>(n), 0);
    for (int64_t x = 0; x < n; x++) {
      const uint32_t y = permute(perm, static_cast<uint32_t>(x));
      CHECK(y < n && !seen[y]);
      seen[y] = 1;
    }
  }
  // the largest position space: 2^31 - 1 entries walk inside 32 bits
  const Perm big = make_perm(1, (int64_t(1) << 31) - 1);
  CHECK(big.half == 16);
  for (uint32_t x : {0u, 1u, 2147483646u}) CHECK(permute(big, x) < big.n);
}

static void test_unseen_rank() {
  uint64_t h = 1;
  for (int trial = 0; trial < 2000; trial++) {
    h = mix64(h);
    const int32_t n_items = 1 + static_cast<int32_t>(h % 40);
    std::vector<int32_t> row;
    for (int32_t c = 0; c < n_items; c++)
      if ((mix64(h + c) & 3) == 0) row.push_back(c);
    std::vector<int32_t> unseen;
    for (int32_t c = 0, q = 0; c < n_items; c++) {
      if (q < static_cast<int32_t>(row.size()) && row[q] == c) q++;
      else unseen.push_back(c);
    }
    for (size_t r = 0; r < unseen.size(); r++)
      CHECK(unseen_by_rank(row.data(), static_cast<int32_t>(row.size()), static_cast<int32_t>(r)) == unseen[r]);
    if (!unseen.empty()) {
      const uint32_t r = draw_rank(h, trial, static_cast<uint32_t>(unseen.size()));
      CHECK(r < unseen.size());
    }
  }
  CHECK(draw_rank(0, 0, 1) == 0);
  CHECK(mul_hi(~0ull, 10) == 9 && mul_hi(0, 10) == 0);
}

static void test_checks() {
  const Matrix m = small_matrix();
  auto run = [&](const Matrix &x) {
    return message_of([&] { validate_finite_matrix(x.rows, x.cols, x.indptr.data(), x.indices.data(), x.data.data()); });
  };
  CHECK(run(m).empty());
  Matrix bad = m;
  bad.indptr[2] = 1;
  CHECK(run(bad) == "malformed indptr.");
  bad = m, bad.indices[1] = 7;
  CHECK(run(bad) == "column index out of range.");
  bad = m, bad.indices[1] = 0;
  CHECK(run(bad).find("duplicate column index") == 0);
  bad = m, bad.indices[0] = 4;
  CHECK(run(bad).find("sorted") != std::string::npos);
  bad = m, bad.data[3] = std::numeric_limits<float>::quiet_NaN();
  CHECK(run(bad) == "the matrix holds a non-finite value.");
  auto hyper = [&](int32_t k, float ua, float ia, float lr, int64_t bs) {
    return message_of([&] { validate_hyper(k, ua, ia, lr, bs); });
  };
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  CHECK(hyper(16, 0.f, 0.f, 0.05f, 1).empty() && hyper(512, 1.f, 1.f, 1.f, 1 << 20).empty());
  CHECK(hyper(0, 0.f, 0.f, 0.05f, 1) == "k must be >= 1." && hyper(513, 0.f, 0.f, 0.05f, 1) == "k must be <= 512.");
  CHECK(hyper(16, 0.f, 0.f, 0.05f, 0) == "batch_size must be >= 1.");
  for (float a : {-1e-9f, inf, nan}) {
    CHECK(hyper(16, a, 0.f, 0.05f, 1) == "the alphas must be finite and >= 0.");
    CHECK(hyper(16, 0.f, a, 0.05f, 1) == "the alphas must be finite and >= 0.");
    CHECK(hyper(16, 0.f, 0.f, a, 1) == "learning_rate must be finite and >= 0.");
  }
  CHECK(hyper(16, 0.f, 0.f, 0.f, 1) == "learning_rate must not be 0.");
  std::vector<float> t = {0.f, -1.f, 255.f};
  CHECK(message_of([&] { validate_table(t.data(), 3, "nf", "big"); }).empty());
  t[1] = nan;
  CHECK(message_of([&] { validate_table(t.data(), 3, "nf", "big"); }) == "nf");
  t[1] = -256.f;
  CHECK(message_of([&] { validate_table(t.data(), 3, "nf", "big"); }) == "big");
  std::vector<float> g = {1.f, 1e-30f, 4.f};
  CHECK(message_of([&] { validate_accumulator(g.data(), 3); }).empty());
  for (float v : {0.f, -1.f, inf, nan}) {
    g[2] = v;
    CHECK(!message_of([&] { validate_accumulator(g.data(), 3); }).empty());
  }
  const std::vector<int32_t> u = {0, 5}, i = {4, 0}, j = {1, 2};
  auto triples = [&](std::vector<int32_t> uu, std::vector<int32_t> ii, std::vector<int32_t> jj) {
    return message_of([&] { validate_triples(2, uu.data(), ii.data(), jj.data(), 6, 5); });
  };
  CHECK(triples(u, i, j).empty());
  CHECK(triples({0, 6}, i, j) == "a triple's user is out of range." && triples({-1, 0}, i, j) != "");
  CHECK(triples(u, {5, 0}, j) == "a triple's item is out of range." && triples(u, i, {0, -1}) != "");
  CHECK(message_of([&] { validate_triples(0, nullptr, nullptr, nullptr, 6, 5); }).empty());
}

static void test_scale_and_lanes() {
  // the scaled bound 4 n PARAM_CAP 2^s stays below 2^62, and the step 2^-s below a float32 ulp of a value of
  // 2^-13 (the initial embeddings of K = 512 are below 2^-10) up to batches of 2^16
  for (int64_t n : {int64_t(1), int64_t(63), int64_t(1000), int64_t(4096), int64_t(65536), int64_t(1) << 30}) {
    const int s = scale_log2(n);
    CHECK(s <= MAX_SCALE_LOG2);
    CHECK(std::ldexp(4.0 * static_cast<double>(n) * PARAM_CAP, s) <= std::ldexp(1.0, 62));
    if (n <= 65536) CHECK(s >= 36);
  }
  CHECK(scale_log2(1) == 44 && scale_log2(4096) == 40 && scale_log2(65536) == 36);
  CHECK(std::ldexp(2.0 * PARAM_CAP, MAX_SCALE_LOG2) <= std::ldexp(1.0, 53));
  const int want[][2] = {{1, 1}, {4, 1}, {5, 2}, {8, 2}, {9, 4}, {16, 4}, {17, 8}, {32, 8}, {33, 16}, {64, 16},
                         {65, 32}, {128, 32}, {129, 64}, {130, 64}, {256, 64}, {512, 64}};
  for (const auto &w : want) CHECK(lanes_per_triple(w[0]) == w[1]);
  // the initial values: inside (-0.5, 0.5) / k, not constant, reproducible
  double lo = 1, hi = -1;
  for (uint64_t q = 0; q < 10000; q++) {
    const float v = init_value(42, 1, q, 16);
    CHECK(v > -0.5f / 16 && v < 0.5f / 16 && v == init_value(42, 1, q, 16));
    lo = v < lo ? v : lo, hi = v > hi ? v : hi;
  }
  CHECK(lo < -0.49 / 16 && hi > 0.49 / 16 && init_value(42, 0, 3, 16) != init_value(42, 1, 3, 16));
}

int main() {
  test_filter_and_sampling();
  test_permutation_sizes();
  test_unseen_rank();
  test_checks();
  test_scale_and_lanes();
  std::printf("bpr_host_prep ok\n");
  return 0;
}
