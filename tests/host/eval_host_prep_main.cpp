// The host preparation of the evaluator's model calls and the serving calls (irspack_amd/csrc/eval_host_prep.hpp)
// and the host decisions of the fused call and the ranking dispatch (irspack_amd/csrc/eval_emit_plan.hpp) on their
// own: no HIP, built with -fsanitize=address,undefined by tests/test_host_sanitizers.py.  Every expected value is
// restated here in plain loops or plain expressions; the plans against the chains of conditions that stood between
// the launches of evaluator.hip before, over grids that hold both sides of every boundary.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>

#include "../../irspack_amd/csrc/eval_host_prep.hpp"
#include "../../irspack_amd/csrc/eval_emit_plan.hpp"

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

// ---- eval_emit_plan.hpp against the former condition chains of evaluator.hip ----
static const int64_t P31 = int64_t(1) << 31;
static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static int64_t env64(const char *v) { return v ? std::max<int64_t>(64, std::atoll(v) / 64 * 64) : int64_t(0); }
static EnvInt env_of(const char *v) { return EnvInt{v != nullptr, v ? std::atoll(v) : 0}; }

static void emit_constants() {  // what the kernels were written against
  EXPECT(SEL_CAP == 2048 && RANK_MAXQ == 32 && HIST_DIRECT_MAX == 36864 && FZ_MAX_CUTOFF == 32);
  EXPECT(EM_CAP == 1024 && EM_SAMPLE == 2048 && EM_SAMPLE_SORTED == 512 && EM_SAMPLE2 == 4096 && EM_HARD_CAP == 2048);
  EXPECT(SF_ITEMS == 512 && SF_USERS == 16);
}

static void emit_pass_plan() {
  const char *samples[] = {nullptr, "1", "64", "100", "512", "5000", "4096", "4159", "-3", "junk"};
  const std::vector<int64_t> nis = {1, 8191, 8192, 8250, 26744, 36864, P31 - 1, P31, P31 + 5};
  const std::vector<int64_t> rowss = {0, 1, 15, 16, 17, 63, 64, 65, 330, 2047, 2048, 2049, 32767, 32768, 32769, 524288,
                                     P31 / 1024 - 1, P31 / 1024, P31 / 1024 + 1, P31 - 1, P31};
  const std::vector<int32_t> kps = {16, 32, 48, 64, 96, 128, 160, 192, 224, 256, 288, 320};
  const std::vector<int64_t> cutoffs = {1, 5, 32, 33};
  long checked = 0, in_domain = 0;
  for (const char *sv : samples)
    for (int sw = 0; sw < 8; sw++)
      for (int rec_mode = 0; rec_mode < 3; rec_mode++)
        for (int64_t cutoff : cutoffs)
          for (int64_t ni : nis)
            for (int64_t d_items : {int64_t(0), int64_t(1)})
              for (int64_t rows : rowss)
                for (int32_t KP : kps) {
                  const bool emit_on = sw & 1, bound_on = sw & 2, fused_on = sw & 4;
                  const EmitFacts f{emit_on, bound_on, fused_on, env_of(sv), rec_mode, cutoff, rows, KP, ni, ni + d_items};
                  const EmitPlan p = plan_emit_pass(f);
                  checked++;
                  // emit_block, from its first line to the default arm of its KP switch
                  bool ok = !(!emit_on || rec_mode != 0 || cutoff > 32 || rows <= 0);
                  EXPECT(emit_call_in_domain(f) == ok);
                  if (KP > 256) ok = false;
                  if (ni != ni + d_items || ni < 4 * 2048 || rows > (int64_t(1) << 31) / 1024) ok = false;
                  if (!(KP == 16 || KP == 32 || KP == 64 || KP == 128 || KP == 192 || KP == 256)) ok = false;  // (was: after the sample pass)
                  EXPECT(p.ok == ok);
                  if (!ok) continue;
                  in_domain++;
                  const bool bounded = bound_on && ni < (int64_t(1) << 31) && rows < (int64_t(1) << 31);
                  const int64_t env_sample = env64(sv);
                  const int64_t n_sample = std::min<int64_t>(env_sample ? env_sample : (bounded ? 512 : 2048), 4096);
                  EXPECT(p.bounded == bounded && p.n_sample == n_sample && p.words == cdiv(ni, 64));
                  const bool fused_sample = bounded && n_sample == 512 && (KP == 16 || KP == 32 || KP == 64 || KP == 128) && fused_on;
                  EXPECT(p.fused_sample == fused_sample);
                  if (fused_sample) {
                    const int per_cu = KP == 128 ? 1 : 2;  // the switch over KP: 16, 32, 64 -> 2, default (128) -> 1
                    EXPECT(p.sample_per_cu == per_cu);
                    for (int cus : {1, 80, 256})
                      EXPECT(sample_fused_grid(rows, p.sample_per_cu, cus) == std::min<int64_t>(cdiv(rows, 16), int64_t(per_cu) * cus));
                  }
                  EXPECT(p.sample_block == 32768 && p.hcap == std::min<int64_t>(2048, rows));
                  EXPECT(p.second_chance == (bounded && n_sample < 4096));
                  const int64_t n_ut = cdiv(rows, 64);
                  EXPECT(p.n_ut == n_ut && p.tiles_total == cdiv(rows, 64) * cdiv(ni, 64));
                  const int64_t wg_bound = n_ut * cdiv(cdiv(ni, 64), 4);
                  EXPECT(p.wg_bound == wg_bound && p.wg_len_on_device == (wg_bound <= (int64_t(1) << 24)));
                  if (p.wg_len_on_device) EXPECT(p.wg_grid == static_cast<int32_t>(std::min<int64_t>(wg_bound, 32768)));
                  EXPECT(p.two_level == (rows >= 32768) && p.reduce_chunk == 4096);
                }
  EXPECT(checked > 1000000 && in_domain > 10000);
  // the boundaries by name
  auto plan = [](int64_t rows, int64_t ni, int32_t KP, int64_t cutoff, const char *sample) {
    return plan_emit_pass(EmitFacts{true, true, true, env_of(sample), 0, cutoff, rows, KP, ni, ni});
  };
  EXPECT(!plan(330, 8191, 64, 20, nullptr).ok && plan(330, 8192, 64, 20, nullptr).ok);
  EXPECT(plan(330, 8250, 64, 32, nullptr).ok && !plan(330, 8250, 64, 33, nullptr).ok);
  EXPECT(!plan(330, 8250, 96, 20, nullptr).ok && !plan(330, 8250, 288, 20, nullptr).ok);
  EXPECT(plan(P31 / 1024, 8250, 64, 20, nullptr).ok && !plan(P31 / 1024 + 1, 8250, 64, 20, nullptr).ok);
  EXPECT(plan(330, 8250, 64, 20, "1").n_sample == 64 && plan(330, 8250, 64, 20, "100").n_sample == 64);
  EXPECT(plan(330, 8250, 64, 20, "512").fused_sample && !plan(330, 8250, 64, 20, "64").fused_sample);
  EXPECT(plan(330, 8250, 64, 20, "5000").n_sample == 4096 && !plan(330, 8250, 64, 20, "5000").second_chance);
  EXPECT(!plan(330, 8250, 192, 20, nullptr).fused_sample && plan(330, 8250, 128, 20, nullptr).sample_per_cu == 1);
  EXPECT(!plan(32767, 8250, 64, 20, nullptr).two_level && plan(32768, 8250, 64, 20, nullptr).two_level);
  // the work list at 2^24 entries: 2^15 user tiles (the most a pass holds) x 512 entries (2,048 item tiles), and
  // at 2^24 + 1 = 97 * 257 * 673: 24,929 user tiles x 673 entries (2,692 item tiles)
  const EmitPlan at = plan(int64_t(1) << 21, 131072, 64, 20, nullptr), above = plan(24929 * 64, 2692 * 64, 64, 20, nullptr);
  EXPECT(at.ok && at.wg_bound == (int64_t(1) << 24) && at.wg_len_on_device && at.wg_grid == 32768);
  EXPECT(above.ok && above.wg_bound == (int64_t(1) << 24) + 1 && !above.wg_len_on_device);
  EXPECT(!plan(int64_t(1) << 21, 131073, 64, 20, nullptr).wg_len_on_device);  // one item more: a 513th entry per user tile
  // the grid cap: 1024 user tiles x 32 entries = 32,768, and one user tile more
  EXPECT(plan(65536, 8192, 64, 20, nullptr).wg_grid == 32768 && plan(65536 - 64, 8192, 64, 20, nullptr).wg_grid == 32768 - 32);
  EXPECT(plan(65536 + 1, 8192, 64, 20, nullptr).wg_grid == 32768 && plan(65536 + 1, 8192, 64, 20, nullptr).wg_bound == 32800);
}

static void emit_pass_rows_and_bitmap() {
  const char *envs[] = {nullptr, "1", "64", "100", "256", "1000000", "0", "-7", "junk"};
  // words * 8 * 64 > 2^31 from words = 2^22 + 1 on: the pass would hold fewer than 64 users
  const std::vector<int64_t> nis = {0, 1, 64, 65, 8250, 1000000, 262144, 262145, (int64_t(1) << 28), (int64_t(1) << 28) + 1,
                                    P31 - 1024, P31 - 1};
  for (const char *v : envs)
    for (int64_t ni : nis) {
      const int64_t env_rows = v ? std::max<int64_t>(64, std::atoll(v) / 64 * 64) : int64_t(0);
      const int64_t words = cdiv(std::max<int64_t>(ni, 1), 64);
      int64_t pass = std::min<int64_t>(524288, (int64_t(1) << 31) / (words * 8) / 64 * 64);
      if (env_rows) pass = std::min(pass, env_rows);
      EXPECT(emit_pass_rows(ni, env_of(v)) == (pass < 64 ? 0 : pass));
    }
  EXPECT(emit_pass_rows(int64_t(1) << 28, env_of(nullptr)) == 64 && emit_pass_rows((int64_t(1) << 28) + 1, env_of(nullptr)) == 0);
  EXPECT(emit_pass_rows(8250, env_of("1")) == 64 && emit_pass_rows(8250, env_of("64")) == 64);
  EXPECT(emit_pass_rows(8250, env_of("100")) == 64 && emit_pass_rows(8250, env_of("256")) == 256);
  EXPECT(emit_pass_rows(8250, env_of(nullptr)) == 524288 && emit_pass_rows(1000000, env_of(nullptr)) == 17152);
  // the bitmap: rows * words * 8 bytes, at most 2 GiB
  for (int64_t rows : {int64_t(1), int64_t(64), int64_t(330), int64_t(524288), int64_t(1) << 20, P31 - 1})
    for (int64_t words : {int64_t(1), int64_t(129), int64_t(256), int64_t(512), int64_t(513), int64_t(1) << 22, (int64_t(1) << 25)})
      EXPECT(mask_bitmap_fits(rows, words) == !(static_cast<double>(rows) * words * 8.0 > 2147483648.0));
  EXPECT(mask_bitmap_fits(524288, 512) && !mask_bitmap_fits(524288, 513) && !mask_bitmap_fits(524289, 512));  // exactly 2 GiB
  EXPECT(mask_bitmap_fits(1, int64_t(1) << 28) && !mask_bitmap_fits(1, (int64_t(1) << 28) + 1));
}

static void emit_hard_rows() {
  for (int32_t flags : {0, 1, 4, 5, -1})
    for (int32_t n_hard : {0, 1, 76, 1024, 1025, 2047, 2048, 100000})
      EXPECT(emit_abandon(flags, n_hard) == (flags || n_hard > 1024));
  EXPECT(!emit_abandon(0, 1024) && emit_abandon(0, 1025) && emit_abandon(1, 0));
  for (int64_t n_hard : {int64_t(1), int64_t(76), int64_t(1024)})
    for (int64_t ni : {int64_t(1), int64_t(8192), int64_t(262144), int64_t(262145), int64_t(1) << 28, (int64_t(1) << 28) + 1, P31 - 1})
      EXPECT(hard_row_chunk(n_hard, ni) == std::max<int64_t>(1, std::min<int64_t>(n_hard, (int64_t(1) << 28) / ni)));
  EXPECT(hard_row_chunk(1024, 1) == 1024 && hard_row_chunk(1024, 262144) == 1024 && hard_row_chunk(1024, 262145) == 1023);
  EXPECT(hard_row_chunk(1024, int64_t(1) << 28) == 1 && hard_row_chunk(1024, (int64_t(1) << 28) + 1) == 1);
}

// launch_rank / launch_rank_big as they chose: which template instance, which grid
struct FormerRank { bool big; int64_t cap, per; bool wave; int m; int mode; size_t key_bytes; };
static FormerRank former_rank(int64_t cutoff, int64_t rows, int64_t max_cand, size_t key_size, bool is_float, int rec_mode,
                              int64_t n_items, bool wave_ok, bool todo) {
  FormerRank r{};
  r.key_bytes = static_cast<size_t>(std::max<int64_t>(max_cand, 1)) * key_size;
  if (cutoff > 2048) {
    r.big = true;
    int64_t cap = 1;
    while (cap < cutoff) cap <<= 1;
    r.cap = cap;
    r.per = std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t(1) << 30) / (cap * 13)));
    r.mode = r.key_bytes <= 128 * 1024 ? 1 : 0;
    return r;
  }
  if (wave_ok && rec_mode == 0 && cutoff <= 64 && n_items < (int64_t(1) << 31) - 64 * 16 && todo) {
    r.wave = true;
    r.m = cutoff <= 24 ? 4 : 8;
  }
  if (is_float && max_cand <= 1024 * 32) r.mode = 2;
  else if (r.key_bytes <= 128 * 1024) r.mode = 1;
  else r.mode = 0;
  return r;
}

static void rank_plan() {
  const std::vector<int64_t> cutoffs = {1, 24, 25, 64, 65, 2047, 2048, 2049, 4096, 4097, 100000};
  const std::vector<int64_t> rowss = {1, 330, 20164, 20165, 40329, 40330, 1000000};  // 2^30 / (4096 * 13) = 20164, / (2048 * 13) = 40329
  const std::vector<int64_t> cands = {0, 1, 16384, 16385, 32768, 32769, 1024 * 32, 1024 * 32 + 1, 100000};  // 128 KB: 32,768 float keys, 16,384 double keys
  const std::vector<int64_t> items = {8250, P31 - 1025, P31 - 1024, P31 - 1};
  for (int64_t cutoff : cutoffs)
    for (int64_t rows : rowss)
      for (int64_t max_cand : cands)
        for (bool f32 : {false, true})
          for (int rec_mode = 0; rec_mode < 3; rec_mode++)
            for (int64_t n_items : items)
              for (int sw = 0; sw < 4; sw++) {
                const RankPlan r = plan_rank(cutoff, rows, max_cand, f32, rec_mode, n_items, sw & 1, sw & 2);
                const FormerRank w = former_rank(cutoff, rows, max_cand, f32 ? sizeof(uint32_t) : sizeof(uint64_t), f32, rec_mode,
                                                 n_items, sw & 1, sw & 2);
                EXPECT(r.big == w.big && r.mode == w.mode && r.key_bytes == w.key_bytes && r.wave == w.wave);
                if (w.big) EXPECT(r.big_cap == w.cap && r.big_rows == w.per && r.mode != 2);
                if (w.wave) EXPECT(r.wave_m == w.m);
              }
  EXPECT(plan_rank(24, 9, 8250, true, 0, 8250, true, true).wave_m == 4 && plan_rank(25, 9, 8250, true, 0, 8250, true, true).wave_m == 8);
  EXPECT(plan_rank(64, 9, 8250, true, 0, 8250, true, true).wave && !plan_rank(65, 9, 8250, true, 0, 8250, true, true).wave);
  EXPECT(!plan_rank(20, 9, 8250, true, 0, 8250, true, false).wave);  // the hard rows of the emit path: no scratch, general kernel
  EXPECT(plan_rank(20, 9, 8250, true, 0, P31 - 1025, true, true).wave && !plan_rank(20, 9, 8250, true, 0, P31 - 1024, true, true).wave);
  EXPECT(!plan_rank(SEL_CAP, 9, 8250, true, 0, 8250, true, true).big && plan_rank(SEL_CAP + 1, 9, 8250, true, 0, 8250, true, true).big);
  EXPECT(plan_rank(SEL_CAP + 1, 30000, 8250, true, 0, 8250, true, true).big_cap == 4096);
  EXPECT(plan_rank(SEL_CAP + 1, 30000, 8250, true, 0, 8250, true, true).big_rows == 20164);
  EXPECT(plan_rank(20, 9, 1024 * RANK_MAXQ, true, 0, 8250, true, true).mode == 2);
  EXPECT(plan_rank(20, 9, 1024 * RANK_MAXQ + 1, true, 0, 8250, true, true).mode == 0);  // 4 bytes more than 128 KB of keys
  EXPECT(plan_rank(20, 9, 16384, false, 0, 8250, true, true).mode == 1 && plan_rank(20, 9, 16385, false, 0, 8250, true, true).mode == 0);
  EXPECT(plan_rank(4000, 9, 32768, true, 0, 8250, true, true).mode == 1 && plan_rank(4000, 9, 32769, true, 0, 8250, true, true).mode == 0);
}

static void hist_plan() {
  for (int64_t n : {int64_t(-1), int64_t(0), int64_t(1), int64_t(16384), int64_t(16385), int64_t(65535), int64_t(65536),
                    int64_t(128) * 16384, int64_t(128) * 16384 + 1, int64_t(1024) * 16384 + 1, int64_t(1) << 33})
    for (int64_t n_items : {int64_t(0), int64_t(1), int64_t(8250), HIST_DIRECT_MAX, HIST_DIRECT_MAX + 1}) {
      const HistPlan h = plan_item_hist(n, n_items);
      if (n <= 0) {
        EXPECT(h.grid == 0);
      } else if (n_items > 0 && n_items <= 36864 && n >= 65536) {
        EXPECT(h.direct && h.grid == std::min<int64_t>(128, (n + 16383) / 16384));
      } else {
        EXPECT(!h.direct && h.grid == std::min<int64_t>(1024, (n + 16383) / 16384));
      }
    }
  EXPECT(!plan_item_hist(65535, 8250).direct && plan_item_hist(65536, 8250).direct);
  EXPECT(plan_item_hist(65536, HIST_DIRECT_MAX).direct && !plan_item_hist(65536, HIST_DIRECT_MAX + 1).direct);
}

int main() {
  profile_rows();
  mask_rows();
  orders();
  candidate_lists();
  block_sizes();
  weight_rows();
  large_scans();
  emit_constants();
  emit_pass_plan();
  emit_pass_rows_and_bitmap();
  emit_hard_rows();
  rank_plan();
  hist_plan();
  std::printf("eval_host_prep ok\n");
  return 0;
}
