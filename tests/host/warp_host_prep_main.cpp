// What the WARP loss adds to irspack_amd/csrc/bpr_host_prep.hpp, in a program of its own for the sanitizers
// (tests/test_warp_surface.py builds it with -fsanitize=address,undefined, every report fatal): the candidate
// stream on the host against a plain scan, its prefix property, its key, the scale bound, the weight table and the
// argument checks.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "../../irspack_amd/csrc/bpr_host_prep.hpp"

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

// 40 x 23 from the generator: an empty row (2), a full row (5), a row with all items but one (9)
static Matrix some_matrix() {
  Matrix m{40, 23, {0}, {}, {}};
  for (int64_t u = 0; u < m.rows; u++) {
    for (int32_t c = 0; c < m.cols; c++) {
      bool on = (mix64(static_cast<uint64_t>(u * 100 + c)) % 10) < 3;
      if (u == 2) on = false;
      if (u == 5) on = true;
      if (u == 9) on = c != 4;
      if (on) m.indices.push_back(c), m.data.push_back(1.f);
    }
    m.indptr.push_back(static_cast<int64_t>(m.indices.size()));
  }
  return m;
}

static void test_candidate_stream() {
  const Matrix m = some_matrix();
  const Positives p = filter_positives(m.rows, m.cols, m.indptr.data(), m.indices.data(), m.data.data());
  CHECK(p.n_skipped_rows == 1 && p.n_skipped_positives == 23);
  const int64_t n = static_cast<int64_t>(p.pos_user.size());
  std::vector<std::set<int32_t>> drawn(static_cast<size_t>(m.rows));
  for (int64_t epoch = 0; epoch < 20; epoch++) {
    const Perm perm = make_perm(epoch_key(42, epoch, 0), n);
    const uint64_t key = warp_key(42, epoch), neg_key = epoch_key(42, epoch, 1);
    for (int64_t pos = 0; pos < n; pos++) {
      int32_t u, i, u3, i3, ub, ib, jb;
      std::vector<int32_t> c10(10), c3(3);
      warp_candidates_one(p, m.cols, perm, key, pos, 10, &u, &i, c10.data());
      warp_candidates_one(p, m.cols, perm, key, pos, 3, &u3, &i3, c3.data());
      sample_one(p, m.cols, perm, neg_key, pos, &ub, &ib, &jb);
      CHECK(u == ub && i == ib && u == u3 && i == i3);  // the position space and order of the BPR sampler
      // the prefix property: candidate t does not depend on max_sampled
      for (int t = 0; t < 3; t++) CHECK(c3[t] == c10[t]);
      // against a scan: candidate t is the r-th unseen item of the row, r from the draw at counter p * 256 + t
      std::vector<int32_t> unseen;
      for (int32_t c = 0, q = p.indptr[u]; c < m.cols; c++) {
        if (q < p.indptr[u + 1] && p.indices[q] == c) q++;
        else unseen.push_back(c);
      }
      CHECK(!unseen.empty());
      for (int t = 1; t <= 10; t++) {
        const uint32_t r = draw_rank(key, static_cast<uint64_t>(pos) * 256 + t, static_cast<uint32_t>(unseen.size()));
        CHECK(r < unseen.size() && c10[t - 1] == unseen[r]);
        drawn[u].insert(c10[t - 1]);
      }
      if (u == 9) CHECK(std::set<int32_t>(c10.begin(), c10.end()) == std::set<int32_t>{4});
    }
  }
  // every unseen item of a row is drawn sooner or later (row 0: 20 epochs x its positives x 10 candidates)
  std::set<int32_t> unseen0;
  for (int32_t c = 0, q = p.indptr[0]; c < m.cols; c++) {
    if (q < p.indptr[1] && p.indices[q] == c) q++;
    else unseen0.insert(c);
  }
  CHECK(p.indptr[1] > 0 && drawn[0] == unseen0);
  // the last candidate the counter has room for
  int32_t u, i;
  std::vector<int32_t> c256(256);
  const Perm perm = make_perm(epoch_key(7, 0, 0), n);
  warp_candidates_one(p, m.cols, perm, warp_key(7, 0), n - 1, 256, &u, &i, c256.data());
  for (int32_t c : c256) CHECK(c >= 0 && c < m.cols);
}

static void test_key() {
  // a key of its own: not the order or negative key of this epoch or of a neighbour (a third stream of epoch_key
  // would be the order key of the next epoch), and different from epoch to epoch and seed to seed
  CHECK(epoch_key(42, 3, 2) == epoch_key(42, 4, 0));  // (why epoch_key is not reused)
  std::set<uint64_t> keys;
  for (uint64_t seed : {0ull, 1ull, 42ull, ~0ull})
    for (int64_t e = 0; e < 200; e++) {
      keys.insert(warp_key(seed, e));
      for (int64_t other = (e > 2 ? e - 2 : 0); other < e + 3; other++)
        for (uint64_t stream : {0ull, 1ull}) CHECK(warp_key(seed, e) != epoch_key(seed, other, stream));
    }
  CHECK(keys.size() == 800);
}

static void test_scale_and_weights() {
  // the scaled bound 4 n 2^4 PARAM_CAP 2^s stays below 2^62, every scaled contribution (below 2^4 2 PARAM_CAP) is an
  // exact double, and the step 2^-s is at most 2^-32 up to batches of 2^16
  for (int64_t n : {int64_t(1), int64_t(63), int64_t(1000), int64_t(4096), int64_t(65536), int64_t(1) << 30}) {
    const int s = warp_scale_log2(n);
    int lg = 0;
    while ((int64_t(1) << lg) < n) lg++;
    CHECK(s <= WARP_MAX_SCALE_LOG2 && s == std::min(62 - (lg + 2 + 8 + 4), 40));
    CHECK(std::ldexp(4.0 * static_cast<double>(n) * 16.0 * PARAM_CAP, s) <= std::ldexp(1.0, 62));
    if (n <= 65536) CHECK(s >= 32);
  }
  CHECK(warp_scale_log2(1) == 40 && warp_scale_log2(1000) == 38 && warp_scale_log2(4096) == 36 &&
        warp_scale_log2(65536) == 32);
  CHECK(std::ldexp(16.0 * 2.0 * PARAM_CAP, WARP_MAX_SCALE_LOG2) <= std::ldexp(1.0, 53));
  CHECK(WARP_MAX_LOSS < std::ldexp(1.0, WARP_WEIGHT_LOG2));
  // the weights: ln(floor((n_items - 1) / t)), at least ln 1 = 0 and at most 10
  const std::vector<double> w37 = warp_weights(37, 10);
  CHECK(w37.size() == 10);
  const int rank37[10] = {36, 18, 12, 9, 7, 6, 5, 4, 4, 3};
  for (int t = 0; t < 10; t++) CHECK(w37[t] == std::log(static_cast<double>(rank37[t])));
  const std::vector<double> w5 = warp_weights(5, 10);
  CHECK(w5[0] == std::log(4.0) && w5[1] == std::log(2.0));
  for (int t = 2; t < 10; t++) CHECK(w5[t] == 0.0);
  const std::vector<double> big = warp_weights(30000, 3);
  CHECK(std::log(29999.0) > 10.0 && big[0] == 10.0 && big[1] == std::log(14999.0) && big[2] == std::log(9999.0));
  CHECK(warp_weights(22028, 1)[0] == 10.0 && warp_weights(22027, 1)[0] < 10.0);  // (e^10 = 22026.47)
  for (double w : warp_weights(1, 256)) CHECK(w == 0.0);
  for (double w : warp_weights((int64_t(1) << 31) - 2, 256)) CHECK(w >= 0.0 && w <= 10.0);
}

static void test_checks() {
  auto ms = [&](int32_t v) { return message_of([&] { validate_max_sampled(v); }); };
  CHECK(ms(1).empty() && ms(10).empty() && ms(256).empty());
  CHECK(ms(0) == "max_sampled must be >= 1." && ms(-3) == "max_sampled must be >= 1.");
  CHECK(ms(257) == "max_sampled must be <= 256.");
  const std::vector<int32_t> u = {0, 5}, i = {4, 0}, c = {1, 2, 3, 0, 4, 4};
  auto batch = [&](int64_t n, const int32_t *uu, const int32_t *ii, const int32_t *cc) {
    return message_of([&] { validate_warp_batch(n, uu, ii, cc, 3, 6, 5); });
  };
  CHECK(batch(2, u.data(), i.data(), c.data()).empty());
  CHECK(batch(0, nullptr, nullptr, nullptr).empty());
  CHECK(batch(-1, u.data(), i.data(), c.data()) == "n must be >= 0.");
  CHECK(batch((int64_t(1) << 31) / 3 + 1, u.data(), i.data(), c.data()) == "n * max_sampled must be below 2^31.");
  CHECK(batch(2, nullptr, i.data(), c.data()) == "the position and candidate arrays must not be null.");
  CHECK(batch(2, u.data(), i.data(), nullptr) == "the position and candidate arrays must not be null.");
  std::vector<int32_t> bad = u;
  bad[1] = 6;
  CHECK(batch(2, bad.data(), i.data(), c.data()) == "a position's user is out of range.");
  bad = i, bad[0] = -1;
  CHECK(batch(2, u.data(), bad.data(), c.data()) == "a position's item is out of range.");
  bad = c, bad[5] = 5;
  CHECK(batch(2, u.data(), i.data(), bad.data()) == "a candidate is out of range.");
  CHECK(batch(1, u.data(), i.data(), bad.data()).empty());  // (the second position's candidates are not read)
  bad = c, bad[0] = -1;
  CHECK(batch(2, u.data(), i.data(), bad.data()) == "a candidate is out of range.");
}

int main() {
  test_candidate_stream();
  test_key();
  test_scale_and_weights();
  test_checks();
  std::printf("warp_host_prep ok\n");
  return 0;
}
