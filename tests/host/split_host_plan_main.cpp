// irspack_amd/csrc/split_host_plan.hpp in a program of its own, for the sanitizers (tests/test_split_surface.py
// builds it with -fsanitize=address,undefined, every report fatal).  The expectations are written out by hand from
// the rule, not computed by the code under test.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <vector>

#include "../../irspack_amd/csrc/split_host_plan.hpp"

using namespace irs::split;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

template <class F> static bool rejects(F &&f) {
  try {
    f();
  } catch (const std::invalid_argument &) {
    return true;
  }
  return false;
}

static Mode ratio_mode(double r, bool ceil) { return Mode{MODE_RATIO, r, ceil ? 1 : 0, 0}; }
static Mode fixed_mode(int64_t n) { return Mode{MODE_FIXED_N, 0.0, 0, n}; }

int main() {
  // ---- n_test, ratio mode: the product is a double before it is rounded ---------------------------------------------
  CHECK(n_test_of(10, ratio_mode(0.3, false)) == 3);
  // 10 * 0.3: 0.3 is 5404319552844595 / 2^54, ten times that lies 2 / 2^54 below 3 where doubles are 8 / 2^54 apart,
  // so the product rounds to 3.0 itself and ceil gives 3 (what the reference's std::ceil(nnz_row * test_ratio) gives)
  CHECK(n_test_of(10, ratio_mode(0.3, true)) == 3);
  CHECK(n_test_of(20, ratio_mode(0.3, true)) == 6);
  // where the rounded product does leave the integer: 100 * 0.07 = 7.000000000000001, 100 * 0.55 = 55.00000000000001,
  // 100 * 0.57 = 56.99999999999999, 90 * 0.7 = 62.99999999999999
  CHECK(n_test_of(100, ratio_mode(0.07, true)) == 8 && n_test_of(100, ratio_mode(0.07, false)) == 7);
  CHECK(n_test_of(100, ratio_mode(0.55, true)) == 56 && n_test_of(100, ratio_mode(0.55, false)) == 55);
  CHECK(n_test_of(100, ratio_mode(0.57, false)) == 56 && n_test_of(100, ratio_mode(0.57, true)) == 57);
  CHECK(n_test_of(90, ratio_mode(0.7, false)) == 62 && n_test_of(90, ratio_mode(0.7, true)) == 63);
  CHECK(n_test_of(10, ratio_mode(0.5, false)) == 5 && n_test_of(10, ratio_mode(0.5, true)) == 5);
  CHECK(n_test_of(3, ratio_mode(0.5, false)) == 1 && n_test_of(3, ratio_mode(0.5, true)) == 2);
  CHECK(n_test_of(7, ratio_mode(0.0, false)) == 0 && n_test_of(7, ratio_mode(0.0, true)) == 0);
  CHECK(n_test_of(7, ratio_mode(1.0, false)) == 7 && n_test_of(7, ratio_mode(1.0, true)) == 7);
  CHECK(n_test_of(0, ratio_mode(0.7, true)) == 0);
  CHECK(n_test_of(1, ratio_mode(0.1, false)) == 0 && n_test_of(1, ratio_mode(0.1, true)) == 1);
  CHECK(n_test_of(80000, ratio_mode(0.3, false)) == 24000);
  // ---- n_test, fixed mode ------------------------------------------------------------------------------------------
  CHECK(n_test_of(5, fixed_mode(0)) == 0 && n_test_of(5, fixed_mode(1)) == 1 && n_test_of(5, fixed_mode(5)) == 5);
  CHECK(n_test_of(5, fixed_mode(6)) == 5 && n_test_of(0, fixed_mode(3)) == 0);
  CHECK(n_test_of(5, fixed_mode(std::numeric_limits<int64_t>::max())) == 5);

  // ---- argument checks ---------------------------------------------------------------------------------------------
  CHECK(!rejects([] { check_mode(ratio_mode(0.0, false)); }) && !rejects([] { check_mode(ratio_mode(1.0, true)); }));
  CHECK(rejects([] { check_mode(ratio_mode(1.5, false)); }));
  CHECK(rejects([] { check_mode(ratio_mode(-1e-9, false)); }));
  CHECK(rejects([] { check_mode(ratio_mode(std::numeric_limits<double>::quiet_NaN(), false)); }));
  CHECK(!rejects([] { check_mode(fixed_mode(0)); }) && rejects([] { check_mode(fixed_mode(-1)); }));
  CHECK(rejects([] { check_mode(Mode{2, 0.5, 0, 0}); }));
  for (int w : {1, 2, 4, 8}) CHECK(!rejects([w] { check_width(w); }));
  for (int w : {0, 3, 5, 6, 7, 16, -1}) CHECK(rejects([w] { check_width(w); }));

  // ---- class bounds, each boundary -1, 0, +1 -------------------------------------------------------------------------
  CHECK(kWaveMax == 64 && kLdsMax == 4096);
  CHECK(row_class(-1) == CLASS_EMPTY && row_class(0) == CLASS_EMPTY && row_class(1) == CLASS_WAVE);
  CHECK(row_class(63) == CLASS_WAVE && row_class(64) == CLASS_WAVE && row_class(65) == CLASS_LDS);
  CHECK(row_class(4095) == CLASS_LDS && row_class(4096) == CLASS_LDS && row_class(4097) == CLASS_STREAM);
  CHECK(row_class(int64_t(1) << 31) == CLASS_STREAM);

  // ---- the keys: mix64 of splitmix64 (its first outputs from state 0 are mix64(0), mix64(golden), ...) -----------------
  CHECK(mix64(0) == 0xE220A8397B1DCDAFull);
  CHECK(row_key(1, 0) == mix64(mix64(1) ^ mix64(0x53504C4954ull)));
  CHECK(row_key(1, 7) == mix64(mix64(1) ^ mix64(0x53504C495Bull)));
  CHECK(entry_key(row_key(42, 3), 5) == mix64(row_key(42, 3) ^ mix64(5)));
  CHECK(row_key(1, 0) != row_key(2, 0) && row_key(1, 0) != row_key(1, 1));

  // ---- the held-out set: lexicographic in (key, j), with injected keys --------------------------------------------------
  {
    // keys 5 5 1 5 9: the smallest is j = 2, then the three 5s in the order of j
    const uint64_t k[5] = {5, 5, 1, 5, 9};
    auto key = [&](int64_t j) { return k[j]; };
    const std::vector<uint8_t> want[6] = {{0, 0, 0, 0, 0}, {0, 0, 1, 0, 0}, {1, 0, 1, 0, 0},
                                          {1, 1, 1, 0, 0}, {1, 1, 1, 1, 0}, {1, 1, 1, 1, 1}};
    for (int n = 0; n <= 5; n++) CHECK(held_out_flags(5, n, key) == want[n]);
    CHECK(held_out_flags(5, 9, key) == want[5]);  // (never asked for: more than the row)
    // all keys equal: the first n positions
    auto same = [](int64_t) { return uint64_t(77); };
    CHECK((held_out_flags(4, 2, same) == std::vector<uint8_t>{1, 1, 0, 0}));
    // the largest and the smallest word
    const uint64_t e[3] = {~uint64_t(0), 0, ~uint64_t(0)};
    CHECK((held_out_flags(3, 2, [&](int64_t j) { return e[j]; }) == std::vector<uint8_t>{1, 1, 0}));
    CHECK(held_out_flags(0, 0, same).empty());
  }
  // the rule's own keys: the flags are the n smallest keys, and the count is n_test
  for (uint64_t seed : {1ull, 42ull}) {
    for (int64_t m : {1, 2, 10, 64, 65, 300}) {
      const Mode md = ratio_mode(0.3, true);
      const std::vector<uint8_t> f = held_out_flags(seed, 5, m, md);
      int64_t n = 0;
      uint64_t max_in = 0, min_out = ~uint64_t(0);
      for (int64_t j = 0; j < m; j++) {
        const uint64_t key = entry_key(row_key(seed, 5), j);
        if (f[j]) n++, max_in = key > max_in ? key : max_in;
        else min_out = key < min_out ? key : min_out;
      }
      CHECK(n == n_test_of(m, md));
      CHECK(n == 0 || n == m || max_in < min_out);
    }
  }

  // ---- the plan: rows per class, the row lists ----------------------------------------------------------------------------
  {
    //                         lengths: 0  1  64  65  4096  4097  0   2
    const int64_t indptr[9] = {0, 0, 1, 65, 130, 4226, 8323, 8323, 8325};
    Plan p = make_plan(8, indptr, ratio_mode(0.5, false));
    CHECK(p.n_class[CLASS_EMPTY] == 2 && p.n_class[CLASS_WAVE] == 3 && p.n_class[CLASS_LDS] == 2 &&
          p.n_class[CLASS_STREAM] == 1);
    CHECK((p.long_rows == std::vector<int32_t>{3, 4, 5}));
    CHECK((p.select_lds_rows == std::vector<int32_t>{3, 4}) && (p.select_stream_rows == std::vector<int32_t>{5}));
    CHECK(p.wave_select_rows == 2);  // lengths 64 and 2; length 1 has n_test = 0
    p = make_plan(8, indptr, ratio_mode(1.0, false));  // everything held out: nothing to select
    CHECK(p.long_rows.size() == 3 && p.select_lds_rows.empty() && p.select_stream_rows.empty() && p.wave_select_rows == 0);
    p = make_plan(8, indptr, fixed_mode(2));  // the row of 2 is held out whole, the row of 1 as well
    CHECK(p.wave_select_rows == 1 && p.select_lds_rows.size() == 2 && p.select_stream_rows.size() == 1);
    p = make_plan(0, indptr, fixed_mode(2));
    CHECK(p.long_rows.empty() && p.n_class[0] + p.n_class[1] + p.n_class[2] + p.n_class[3] == 0);
  }
  // the scan covers rows + 1 items in tiles of 2,048
  CHECK(kScanTile == 2048);
  CHECK(scan_tiles(0) == 1 && scan_tiles(2047) == 1 && scan_tiles(2048) == 2 && scan_tiles(200000) == 98);

  std::printf("split_host_plan ok\n");
  return 0;
}
