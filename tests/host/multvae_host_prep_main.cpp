// irspack_amd/csrc/multvae_host_prep.hpp in a program of its own, for the sanitizers (tests/test_multvae_surface.py
// builds it with -fsanitize=address,undefined, every report fatal): the layout of the arena and its packing, the
// argument checks, the schedule, the bias corrections, the order of an epoch, the noise, the initial tables, the
// scale bound and the K-slabs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "../../irspack_amd/csrc/multvae_host_prep.hpp"

using namespace irs;
using namespace irs::mv;

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

static void test_layout_and_packing() {
  for (int64_t H : {1, 4, 5, 33, 574})
    for (int64_t L : {1, 3, 65}) {
      const int64_t I = 70, Hd = 37;
      const Layout y = make_layout(I, H, L, Hd);
      CHECK(y.Hp % 4 == 0 && y.Hp >= H && y.Hp < H + 4 && y.w1_count == (I + 1) * y.Hp);
      const int64_t want[N_TABLES] = {I * H, H, H * 2 * L, 2 * L, L * Hd, Hd, Hd * I, I};
      for (int q = 0; q < N_TABLES; q++) CHECK(y.count(q) == want[q]);
      for (int s = 0; s < 4; s++) CHECK(y.seg[s] % 4 == 0 && y.table[2 * s].offset == y.seg[s]);
      // every element of every table has a place of its own inside the arena, and comes back
      std::vector<std::vector<float>> tables(N_TABLES);
      std::vector<float> arena(static_cast<size_t>(y.total), 0.f);
      float next = 1.f;
      for (int q = 0; q < N_TABLES; q++) {
        tables[q].resize(static_cast<size_t>(y.count(q)));
        for (auto &v : tables[q]) v = next, next += 1.f;
        pack_table(y, q, tables[q].data(), arena.data());
      }
      std::set<float> seen;
      int64_t filled = 0;
      for (float v : arena) {
        if (v == 0.f) continue;
        CHECK(seen.insert(v).second);
        filled++;
      }
      int64_t all = 0;
      for (int q = 0; q < N_TABLES; q++) all += y.count(q);
      CHECK(filled == all);
      for (int q = 0; q < N_TABLES; q++) {
        std::vector<float> back(tables[q].size(), -1.f);
        unpack_table(y, q, arena.data(), back.data());
        CHECK(back == tables[q]);
      }
      // the bias is the row after its weight table
      for (int s = 0; s < 4; s++)
        CHECK(y.table[2 * s + 1].offset == y.table[2 * s].offset + y.table[2 * s].rows * y.table[2 * s].ld);
      CHECK(lanes_per_entry(y.Hp) * chunks_per_lane(y.Hp) >= y.Hp / 4 && chunks_per_lane(y.Hp) <= 3);
      CHECK(256 / lanes_per_entry(y.Hp) * y.Hp <= 1024 * chunks_per_lane(y.Hp));  // (the encoder kernel's LDS rows)
    }
}

static void test_checks() {
  auto hyper = [](int32_t L, int32_t H, int32_t Hd, float p, float l2, double goal, int64_t end, int64_t mb, float lr) {
    return message_of([&] { validate_hyper(L, H, Hd, p, l2, goal, end, mb, lr); });
  };
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  CHECK(hyper(16, 256, 256, 0.5f, 0.f, 0.2, 50, 512, 1e-3f).empty());
  CHECK(hyper(1, 1, 574, 0.f, 7.f, 0.0, 0, 1, 1e-9f).empty());
  CHECK(hyper(0, 8, 8, 0.5f, 0.f, 0.2, 50, 512, 1e-3f) == "dim_z must be >= 1.");
  CHECK(hyper(4, 0, 8, 0.5f, 0.f, 0.2, 50, 512, 1e-3f) == "enc_hidden_dims and dec_hidden_dims must be >= 1.");
  CHECK(hyper(4, 8, 0, 0.5f, 0.f, 0.2, 50, 512, 1e-3f) == "enc_hidden_dims and dec_hidden_dims must be >= 1.");
  CHECK(hyper(4, 575, 8, 0.5f, 0.f, 0.2, 50, 512, 1e-3f) == "enc_hidden_dims and dec_hidden_dims must be <= 574.");
  CHECK(hyper(4, 8, 575, 0.5f, 0.f, 0.2, 50, 512, 1e-3f) == "enc_hidden_dims and dec_hidden_dims must be <= 574.");
  for (float p : {-0.1f, 1.f, nan, inf}) CHECK(hyper(4, 8, 8, p, 0.f, 0.2, 50, 512, 1e-3f) == "dropout_p must be in [0, 1).");
  CHECK(hyper(4, 8, 8, 0.5f, nan, 0.2, 50, 512, 1e-3f) == "l2_regularizer must be finite.");
  CHECK(hyper(4, 8, 8, 0.5f, 0.f, -1.0, 50, 512, 1e-3f) == "kl_anneal_goal must be finite and >= 0.");
  CHECK(hyper(4, 8, 8, 0.5f, 0.f, 0.2, -1, 512, 1e-3f) == "anneal_end_epoch must be >= 0.");
  CHECK(hyper(4, 8, 8, 0.5f, 0.f, 0.2, 50, 0, 1e-3f) == "minibatch_size must be >= 1.");
  for (float lr : {0.f, -1.f, nan, inf}) CHECK(hyper(4, 8, 8, 0.5f, 0.f, 0.2, 50, 512, lr) == "learning_rate must be finite and > 0.");

  const Layout y = make_layout(5, 3, 2, 4);
  std::vector<std::vector<float>> tables(3 * N_TABLES);
  std::vector<const float *> ptrs(3 * N_TABLES);
  for (int q = 0; q < 3 * N_TABLES; q++) {
    tables[q].assign(static_cast<size_t>(y.count(q % N_TABLES)), 0.25f);
    ptrs[q] = tables[q].data();
  }
  auto state = [&](int groups) { return message_of([&] { validate_tables(y, ptrs.data(), groups, "null.", "non-finite."); }); };
  CHECK(state(1).empty() && state(3).empty());
  tables[6][19] = inf;
  CHECK(state(1) == "non-finite.");
  tables[6][19] = 0.f, tables[2 * N_TABLES + 1][2] = -1e-9f;
  CHECK(state(1).empty() && state(3) == "the second moments of the state must be >= 0.");
  tables[2 * N_TABLES + 1][2] = 0.f, ptrs[N_TABLES + 3] = nullptr;
  CHECK(state(1).empty() && state(3) == "null.");
  CHECK(message_of([&] { validate_tables(y, nullptr, 1, "null.", "x"); }) == "null.");

  const int32_t users[3] = {0, 4, 2};
  auto batch = [&](int64_t n, const int32_t *u, int64_t n_users, double klc) {
    return message_of([&] { validate_batch(n, u, n_users, klc); });
  };
  CHECK(batch(3, users, 5, 0.2).empty());
  CHECK(batch(0, users, 5, 0.2) == "a batch must have at least one row.");
  CHECK(batch(3, nullptr, 5, 0.2) == "users must not be null.");
  CHECK(batch(3, users, 4, 0.2) == "a batch row's user is out of range.");
  CHECK(batch(3, users, 5, -0.1) == "klc must be finite and >= 0.");
  CHECK(batch(3, users, 5, std::nan("")) == "klc must be finite and >= 0.");
  const uint8_t keep[4] = {0, 1, 2, 1};
  const float eps[2] = {0.5f, nan};
  CHECK(message_of([&] { validate_noise(2, keep, 1, eps); }).empty());
  CHECK(message_of([&] { validate_noise(3, keep, 1, eps); }) == "keep must hold 0 or 1.");
  CHECK(message_of([&] { validate_noise(2, keep, 2, eps); }) == "eps holds a non-finite value.");
  CHECK(message_of([&] { validate_noise(4, nullptr, 2, nullptr); }).empty());
}

static void test_schedule_and_adam() {
  // multvae.py:161, :244-247 at the ML-20M defaults
  const double total = 50.0 * 138493.0 / 512.0;
  CHECK(kl_coefficient(0.2, 0, 50, 138493, 512) == 0.0);
  CHECK(kl_coefficient(0.2, 1000, 50, 138493, 512) == 0.2 * (1000.0 / total));
  CHECK(kl_coefficient(0.2, static_cast<int64_t>(total) + 1, 50, 138493, 512) == 0.2);
  CHECK(kl_coefficient(0.2, int64_t(1) << 40, 50, 138493, 512) == 0.2);
  CHECK(kl_coefficient(0.4, 0, 0, 100, 10) == 0.4);
  for (int64_t t = 1; t < 200; t++) CHECK(kl_coefficient(0.2, t, 3, 600, 128) >= kl_coefficient(0.2, t - 1, 3, 600, 128));
  CHECK(std::fabs(bias_correction(0.9, 0) - 0.1) < 1e-15 && std::fabs(bias_correction(0.999, 0) - 0.001) < 1e-15);
  CHECK(std::fabs(bias_correction(0.9, 1) - 0.19) < 1e-15 && bias_correction(0.9, 100000) == 1.0);
}

static void test_order_and_noise() {
  for (int64_t n : {1, 2, 3, 7, 64, 600, 1000, 4097}) {
    for (int64_t epoch = 0; epoch < 3; epoch++) {
      const bpr::Perm p = epoch_perm(42, epoch, n);
      std::vector<char> hit(static_cast<size_t>(n), 0);
      for (int64_t q = 0; q < n; q++) {
        const uint32_t u = bpr::permute(p, static_cast<uint32_t>(q));
        CHECK(u < n && !hit[u]);
        hit[u] = 1;
      }
    }
  }
  CHECK(epoch_perm(42, 0, 600).key != epoch_perm(42, 1, 600).key && epoch_perm(42, 0, 600).key != epoch_perm(43, 0, 600).key);
  // (BPR's own order of the same seed and epoch is another one)
  CHECK(epoch_perm(42, 0, 600).key != bpr::make_perm(bpr::epoch_key(42, 0, 0), 600).key);
  CHECK(keep_threshold(0.f) == 0u && keep_threshold(0.5f) == (1u << 23));
  CHECK(noise_key(1, 5, 0) != noise_key(1, 5, 1) && noise_key(1, 5, 0) != noise_key(1, 6, 0) && noise_key(1, 5, 0) != noise_key(2, 5, 0));
  for (float p : {0.f, 0.25f, 0.5f, 0.9f}) {
    const uint32_t thr = keep_threshold(p);
    const uint64_t key = noise_key(7, 3, 0);
    int64_t kept = 0;
    const int64_t N = 200000;
    for (int64_t q = 0; q < N; q++) kept += keep_entry(key, static_cast<uint32_t>(q / 100), static_cast<uint32_t>(q % 100), thr);
    if (p == 0.f) CHECK(kept == N);
    CHECK(std::fabs(static_cast<double>(kept) / N - (1.0 - p)) <= 5.0 * std::sqrt(p * (1.0 - p) / N));
  }
  double sum = 0, sq = 0;
  const int64_t N = 200000;
  const uint64_t key = noise_key(7, 3, 1);
  for (int64_t q = 0; q < N; q++) {
    const double e = gauss(key, static_cast<uint32_t>(q / 64), static_cast<uint32_t>(q % 64));
    CHECK(std::isfinite(e) && std::fabs(e) < 6.0);
    sum += e, sq += e * e;
  }
  const double mean = sum / N, var = sq / N - mean * mean;
  CHECK(std::fabs(mean) <= 5.0 / std::sqrt(static_cast<double>(N)) && std::fabs(var - 1.0) <= 5.0 * std::sqrt(2.0 / N));
  CHECK(gauss(key, 3, 9) == gauss(key, 3, 9) && gauss(key, 3, 9) != gauss(key, 9, 3));
}

static void test_initial_tables() {
  const Layout y = make_layout(300, 40, 8, 24);
  std::vector<float> tables[N_TABLES], again[N_TABLES], other[N_TABLES];
  init_tables(y, 42, tables);
  init_tables(y, 42, again);
  init_tables(y, 43, other);
  for (int q = 0; q < N_TABLES; q++) {
    CHECK(static_cast<int64_t>(tables[q].size()) == y.count(q) && tables[q] == again[q]);
    if (q % 2 == 1) {
      for (float v : tables[q]) CHECK(v == 0.f);
      continue;
    }
    CHECK(tables[q] != other[q]);
    const double sigma = 1.0 / std::sqrt(static_cast<double>(y.table[q].fan_in));
    double sum = 0, sq = 0;
    for (float v : tables[q]) {
      CHECK(std::fabs(v) <= 2.0 * sigma * (1 + 1e-6));
      sum += v, sq += static_cast<double>(v) * v;
    }
    const double n = static_cast<double>(tables[q].size()), mean = sum / n, sd = std::sqrt(sq / n - mean * mean);
    // a normal truncated at +-2 sigma has standard deviation 0.8796 sigma (five standard errors of the estimate)
    CHECK(std::fabs(mean) <= 5.0 * sigma / std::sqrt(n) && std::fabs(sd / sigma - 0.8796) < 0.005 + 5.0 / std::sqrt(2.0 * n));
  }
}

static void test_scale_and_slabs() {
  CHECK(scale_log2(1) == 44 && scale_log2(512) == 44 && scale_log2(1024) == 44 && scale_log2(1025) == 43);
  for (int64_t n : {int64_t(1), int64_t(7), int64_t(512), int64_t(100000), (int64_t(1) << 31) - 1}) {
    // n contributions below 2^8, scaled, stay below 2^62; one scaled contribution is an exact double
    const int s = scale_log2(n);
    CHECK(s >= 1 && s <= MAX_SCALE_LOG2);
    CHECK(std::ldexp(static_cast<long double>(n), CONTRIB_CAP_LOG2 + s) <= std::ldexp(1.0L, 62));
    CHECK(CONTRIB_CAP_LOG2 + s <= 52);
  }
  CHECK(dh2_slab(1) == 512 && dh2_slab(70) == 512 && dh2_slab(512 * 64) == 512 && dh2_slab(512 * 64 + 1) == 1024);
  for (int64_t I : {int64_t(1), int64_t(20108), int64_t(1) << 20, (int64_t(1) << 31) - 2})
    CHECK(ceil_div(I, dh2_slab(I)) <= DH2_MAX_SLABS && dh2_slab(I) % 16 == 0);
  CHECK(lanes_per_entry(4) == 1 && lanes_per_entry(8) == 2 && lanes_per_entry(132) == 64 && lanes_per_entry(576) == 64);
  CHECK(chunks_per_lane(4) == 1 && chunks_per_lane(256) == 1 && chunks_per_lane(260) == 2 && chunks_per_lane(576) == 3);
}

int main() {
  test_layout_and_packing();
  test_checks();
  test_schedule_and_adam();
  test_order_and_noise();
  test_initial_tables();
  test_scale_and_slabs();
  std::printf("multvae_host_prep ok\n");
  return 0;
}
