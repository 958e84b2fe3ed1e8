// The host logic of a kNN construction and compute call (irspack_amd/csrc/knn_host_prep.hpp: entry scan, chunk
// bounds, the threaded target pass, the launch order, the kernel-variant choice, the arena layout) on its own: no
// HIP, built with -fsanitize=address,undefined and with -fsanitize=thread by tests/test_host_sanitizers.py.  Every
// expected value is restated here in plain sequential loops or plain expressions.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../irspack_amd/csrc/host_util.hpp"
#include "../../irspack_amd/csrc/knn_host_prep.hpp"

using namespace irs;
using namespace irs::knn;

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

constexpr int64_t TILE = KNN_TILE, FAST_CAP = KNN_FAST_CAP, TOPK_CAP = KNN_TOPK_CAP;  // (knn.hip asserts: the kernels')

struct Csr {
  int64_t rows = 0, cols = 0;
  std::vector<int64_t> indptr;
  std::vector<int32_t> indices;  // exactly nnz elements: ASan sees a read one past the end
  std::vector<double> ones, weights;
};

// rows x cols with sorted rows: every tenth row empty, row `heavy` holds about a quarter of all entries
static Csr random_csr(int64_t rows, int64_t cols, int per_row, int64_t heavy, uint32_t seed) {
  std::mt19937 gen(seed);
  Csr m;
  m.rows = rows;
  m.cols = cols;
  m.indptr.assign(1, 0);
  const int64_t heavy_len = std::min<int64_t>(cols, rows * per_row / 3);
  for (int64_t r = 0; r < rows; r++) {
    const int64_t len = r == heavy ? heavy_len : (r % 10 == 3 ? 0 : 1 + static_cast<int64_t>(gen() % (2 * per_row)));
    std::vector<char> used(cols, 0);
    for (int64_t k = 0; k < std::min(len, cols); k++) used[gen() % cols] = 1;
    for (int64_t j = 0; j < cols; j++)
      if (used[j] || (r == heavy && j < heavy_len)) m.indices.push_back(static_cast<int32_t>(j));
    m.indptr.push_back(static_cast<int64_t>(m.indices.size()));
  }
  m.ones.assign(m.indices.size(), 1.0);
  std::uniform_real_distribution<double> decades(-3.0, 3.0);
  for (size_t q = 0; q < m.indices.size(); q++) m.weights.push_back(std::pow(10.0, decades(gen)));
  return m;
}

static uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, sizeof(u));
  return u;
}

// ---------------------------------------------------------------- entry scan
static unsigned scan_restated(const Csr &m, const std::vector<double> *vals, int64_t b, int64_t e, int64_t cols,
                              bool classify) {
  unsigned f = 0;
  for (int64_t q = b; q < e; q++) {
    if (m.indices[q] < 0 || m.indices[q] >= cols) f |= BAD_INDEX;
    if (vals && bits((*vals)[q]) != 0x3ff0000000000000ull) f |= NOT_ONES;
  }
  if ((f & NOT_ONES) && classify)
    for (int64_t q = b; q < e; q++) {
      const double v = (*vals)[q], a = v < 0 ? -v : v;
      if (!(a > 1e-150 && a < 1e150)) f |= NOT_SAFE;
      if (!(v > 0.0)) f |= NOT_POSITIVE;
    }
  return f;
}

static void entry_scan(const Csr &base) {
  const int64_t nnz = static_cast<int64_t>(base.indices.size());
  auto check_all = [&](const Csr &m, const std::vector<double> *vals) {
    for (const bool classify : {false, true})
      for (const int64_t cols : {m.cols, m.cols - 1}) {
        const int64_t cuts[] = {0, nnz / 3, nnz / 3, std::max<int64_t>(nnz - 1, 0), nnz};
        for (int k = 0; k + 1 < 5; k++)
          EXPECT((scan_entries(m.indices.data(), vals ? vals->data() : nullptr, cuts[k], cuts[k + 1], cols, classify) ==
                  scan_restated(m, vals, cuts[k], cuts[k + 1], cols, classify)));
        EXPECT((scan_entries(m.indices.data(), vals ? vals->data() : nullptr, 0, nnz, cols, classify) ==
                scan_restated(m, vals, 0, nnz, cols, classify)));
      }
  };
  check_all(base, nullptr);
  check_all(base, &base.ones);
  check_all(base, &base.weights);
  if (nnz == 0) {
    EXPECT(scan_entries(nullptr, nullptr, 0, 0, 0, true) == 0);
    return;
  }
  auto flags_of = [&](const Csr &m, const std::vector<double> &v) {
    const unsigned f = scan_entries(m.indices.data(), v.data(), 0, nnz, m.cols, true);
    EXPECT(f == scan_restated(m, &v, 0, nnz, m.cols, true));
    return f;
  };
  Csr m = base;
  m.indices[nnz / 2] = -1;
  EXPECT(flags_of(m, m.ones) == BAD_INDEX);
  m.indices[nnz / 2] = static_cast<int32_t>(m.cols);
  EXPECT(flags_of(m, m.ones) == BAD_INDEX);
  m = base;
  EXPECT(flags_of(m, m.ones) == 0);
  std::vector<double> v = base.ones;
  v[nnz - 1] = std::nextafter(1.0, 2.0);  // 1.0 + ulp
  EXPECT(flags_of(m, v) == NOT_ONES);
  v = base.ones;
  v[0] = 0.0;
  EXPECT(flags_of(m, v) == (NOT_ONES | NOT_SAFE | NOT_POSITIVE));
  v[0] = 1e-200;
  EXPECT(flags_of(m, v) == (NOT_ONES | NOT_SAFE));
  v[0] = -2.0;
  EXPECT(flags_of(m, v) == (NOT_ONES | NOT_POSITIVE));
}

// ---------------------------------------------------------------- chunk bounds
static void chunks(const Csr &m) {
  EXPECT(chunk_count(nullptr, true, 100, 100) == 1);
  EXPECT(chunk_count(nullptr, true, int64_t(1) << 22, 4096) == 3);
  EXPECT(chunk_count(nullptr, false, int64_t(1) << 22, 4096) == 1);
  EXPECT(chunk_count(nullptr, true, (int64_t(1) << 22) - 1, 4096) == 1 && chunk_count(nullptr, true, int64_t(1) << 22, 4095) == 1);
  EXPECT(chunk_count("0", true, 100, 100) == 1 && chunk_count("7", true, 100, 100) == 7 && chunk_count("900", true, 100, 100) == 64);
  EXPECT(chunk_count("7", true, 100, 3) == 3 && chunk_count("7", false, 0, 0) == 1);
  const std::pair<int64_t, int64_t> ranges[] = {{0, m.rows}, {m.rows / 3, m.rows - std::min<int64_t>(m.rows, 7)}, {0, 0}};
  for (const auto &range : ranges) {
    const int64_t row_begin = range.first, row_end = std::max(range.first, range.second), n = row_end - row_begin;
    for (const int asked : {1, 3, 7, 64, static_cast<int>(m.rows) + 5}) {
      const int n_chunks = chunk_count(std::to_string(asked).c_str(), true, 0, n);
      EXPECT(n_chunks == static_cast<int>(std::min<int64_t>(std::min(asked, 64), std::max<int64_t>(n, 1))));
      const std::vector<int64_t> cb = chunk_bounds(m.indptr.data(), row_begin, row_end, n_chunks);
      EXPECT(static_cast<int>(cb.size()) == n_chunks + 1 && cb.front() == row_begin && cb.back() == row_end);
      const int64_t e_begin = m.indptr[row_begin], e_end = m.indptr[row_end];
      for (int k = 1; k < n_chunks; k++) {
        EXPECT(cb[k] >= cb[k - 1] && cb[k] <= row_end);
        const int64_t e_cut = e_begin + static_cast<int64_t>(static_cast<double>(e_end - e_begin) * k / n_chunks);
        const int64_t cut = std::lower_bound(m.indptr.data() + row_begin, m.indptr.data() + row_end, e_cut) - m.indptr.data();
        EXPECT(cb[k] == std::max(cb[k - 1], cut));
      }
      EXPECT(cb[n_chunks] >= cb[n_chunks - 1]);
    }
  }
}

// ---------------------------------------------------------------- target pass
struct Tables {
  std::vector<double> tstat, tscale;
  std::vector<int64_t> work;
  explicit Tables(int64_t n) : tstat(std::max<int64_t>(n, 1), 0.0), tscale(std::max<int64_t>(n, 1), 1.0), work(std::max<int64_t>(n, 1), 0) {}
};

// one thread, one row after the other; every index is inside [0, cols)
static unsigned pass_restated(const Csr &t, const double *dv, int64_t r_lo, int64_t r_hi, int64_t row_begin,
                                 const FeatureRows &xt, int32_t sim, double alpha, bool binarise, const char *wide_env,
                                 Tables &out) {
  unsigned f = 0;
  const bool wide_ok = !(wide_env && wide_env[0] == '0');
  const double wide_ratio = (wide_env && wide_env[0] == '1') ? 0.0 : 2.3e5;
  for (int64_t i = r_lo; i < r_hi; i++) {
    double ss = 0, bound = 0, minprod = std::numeric_limits<double>::infinity();
    int64_t w = 0;
    for (int64_t q = t.indptr[i]; q < t.indptr[i + 1]; q++) {
      const int32_t j = t.indices[q];
      const double x = binarise ? 1.0 : dv[q], ax = std::fabs(x);
      ss += x * x;
      w += xt.len[j];
      if (x != 1.0) f |= NOT_ONES;
      if (!(x > 0.0)) f |= NOT_POSITIVE;
      if (!(ax > 1e-150 && ax < 1e150)) f |= NOT_SAFE;
      bound += ax * xt.max[j];
      if (ax > 0.0 && xt.min[j] > 0.0) minprod = std::min(minprod, ax * xt.min[j]);
    }
    if (sim == IRS_SIM_COSINE) out.tstat[i - row_begin] = std::sqrt(ss);
    else if (sim == IRS_SIM_ASYMMETRIC) out.tstat[i - row_begin] = std::pow(ss, alpha);
    else if (sim == IRS_SIM_JACCARD || sim == IRS_SIM_TVERSKY) out.tstat[i - row_begin] = static_cast<double>(t.indptr[i + 1] - t.indptr[i]);
    out.work[i - row_begin] = w;
    if (bound > 0 && std::isfinite(bound)) {
      int ex = 0;
      (void)std::frexp(bound, &ex);
      out.tscale[i - row_begin] = std::ldexp(1.0, 61 - ex);
      if (wide_ok && std::isfinite(minprod) && bound > wide_ratio * minprod) {
        out.tscale[i - row_begin] = -out.tscale[i - row_begin];
        f |= ANY_WIDE;
      }
    }
  }
  return f;
}

static bool bit_equal(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

static void target_passes(const Csr &t, uint32_t seed) {
  // the feature rows' tables: lengths, and value ranges with zeros (rows without a positive value)
  std::mt19937 gen(seed);
  std::vector<int64_t> len(t.cols);
  std::vector<double> mx(t.cols), mn(t.cols);
  for (int64_t u = 0; u < t.cols; u++) {
    len[u] = gen() % 400;
    mn[u] = u % 7 == 0 ? 0.0 : std::pow(10.0, -2.0 + static_cast<double>(gen() % 400) / 100.0);
    mx[u] = u % 7 == 0 ? 0.0 : mn[u] * (1.0 + static_cast<double>(gen() % 1000));
  }
  std::vector<double> unit_mx(t.cols, 1.0);
  const int32_t sims[] = {IRS_SIM_COSINE, IRS_SIM_ASYMMETRIC, IRS_SIM_JACCARD, IRS_SIM_TVERSKY, IRS_SIM_P3ALPHA, IRS_SIM_RP3BETA};
  const int64_t row_begin = std::min<int64_t>(2, t.rows), row_end = t.rows, n = row_end - row_begin;
  const int64_t r_lo = row_begin + n / 4, r_hi = row_end;  // (a chunk that is not the call's first)
  std::vector<double> half = t.weights;  // the first rows' values are ones: threads see different classes
  for (int64_t q = 0; q < t.indptr[r_lo + (r_hi - r_lo) / 2]; q++) half[q] = 1.0;
  for (const int32_t sim : sims)
    for (const std::vector<double> *vals : {&t.ones, &t.weights, static_cast<const std::vector<double> *>(&half)})
      for (const bool unit_features : {true, false})
        for (const char *wide_env : {static_cast<const char *>(nullptr), "0", "1"}) {
          const bool binarise = sim == IRS_SIM_JACCARD || sim == IRS_SIM_TVERSKY;
          const FeatureRows xt{len.data(), unit_features ? unit_mx.data() : mx.data(), unit_features ? unit_mx.data() : mn.data()};
          Tables want(n);
          const unsigned fw = pass_restated(t, vals->data(), r_lo, r_hi, row_begin, xt, sim, 0.7, binarise, wide_env, want);
          for (const int n_thr : {1, 2, 5}) {
            Tables got(n);
            const unsigned fg = target_pass(t.indptr.data(), t.indices.data(), binarise ? nullptr : vals->data(), t.cols,
                                               r_lo, r_hi, row_begin, xt, sim, 0.7, binarise, WideRule(wide_env), n_thr,
                                               got.tstat.data(), got.tscale.data(), got.work.data());
            EXPECT(fg == fw);
            EXPECT(bit_equal(got.tstat, want.tstat) && bit_equal(got.tscale, want.tscale) && got.work == want.work);
          }
        }
  if (r_hi - r_lo < 3) return;
  // malformed chunks are reported, and nothing outside the arrays is read on the way (AddressSanitizer's part)
  const FeatureRows xt{len.data(), mx.data(), mn.data()};
  for (const int n_thr : {1, 2, 5})
    for (const std::vector<double> *vals : {&t.ones, &t.weights}) {
      Tables got(n);
      Csr bad = t;  // an index out of range in the last row
      EXPECT(bad.indptr[t.rows] > bad.indptr[t.rows - 1]);
      for (const int32_t j : {static_cast<int32_t>(t.cols), -1, std::numeric_limits<int32_t>::max()}) {
        bad.indices.back() = j;
        EXPECT(target_pass(bad.indptr.data(), bad.indices.data(), vals->data(), t.cols, r_lo, r_hi, row_begin, xt,
                           IRS_SIM_COSINE, 0.7, false, WideRule(nullptr), n_thr, got.tstat.data(), got.tscale.data(),
                           got.work.data()) & BAD_INDEX);
      }
      bad = t;  // a non-monotone row pointer inside the chunk: a row whose end lies before its start
      int64_t mid = r_lo + (r_hi - r_lo) / 2;
      while (bad.indptr[mid] == bad.indptr[mid + 1]) mid--;  // (a row with entries)
      EXPECT(mid > r_lo);
      std::swap(bad.indptr[mid], bad.indptr[mid + 1]);
      EXPECT(target_pass(bad.indptr.data(), bad.indices.data(), vals->data(), t.cols, r_lo, r_hi, row_begin, xt,
                         IRS_SIM_COSINE, 0.7, false, WideRule(nullptr), n_thr, got.tstat.data(), got.tscale.data(),
                         got.work.data()) & BAD_INDEX);
    }
}

// ---------------------------------------------------------------- launch order
static void launch_orders(uint32_t seed) {
  std::mt19937_64 gen(seed);
  for (const int64_t nc : {int64_t(0), int64_t(1), int64_t(2), int64_t(777)}) {
    std::vector<int64_t> work(std::max<int64_t>(nc, 1));
    for (int64_t i = 0; i < nc; i++) work[i] = i % 5 == 0 ? 0 : static_cast<int64_t>(gen() >> (10 + gen() % 50));
    if (nc > 4) work[3] = work[1];
    const int32_t first_slot = 1000;
    std::vector<int32_t> order(std::max<int64_t>(nc, 1), -1), slot_of(std::max<int64_t>(nc, 1), -1);
    heaviest_first(work.data(), nc, order.data());
    slots_of_rows(order.data(), nc, first_slot, slot_of.data());
    std::vector<char> seen(nc, 0);
    for (int64_t sl = 0; sl < nc; sl++) {
      EXPECT(order[sl] >= 0 && order[sl] < nc && !seen[order[sl]]);
      seen[order[sl]] = 1;
      EXPECT(slot_of[order[sl]] == first_slot + sl);
      if (sl == 0) continue;
      const int before = work_bucket(work[order[sl - 1]]), here = work_bucket(work[order[sl]]);
      EXPECT(before <= here);                               // bucket numbers grow as the work shrinks
      if (before == here) EXPECT(order[sl - 1] < order[sl]);  // rows of a bucket in row order
      else EXPECT(work[order[sl - 1]] > work[order[sl]]);
    }
  }
  EXPECT(work_bucket(0) == WORK_BUCKETS - 1 && work_bucket(std::numeric_limits<int64_t>::max()) < 64);
  EXPECT(work_bucket(1000) == WORK_BUCKETS - 1 - static_cast<int>(std::log2(1001.0) * 64.0));
}

// ---------------------------------------------------------------- variant choice
// the chain of conditions at the launch site before it became a function
struct Launches {
  int first;  // index into {<T,T,T,T>, <T,T,T>, <T,T>, <T,F>, <F,T>, <F,F>}
  bool redo, acc32, sentinel;
};
static Launches former_chain(const VariantInputs &v) {
  Launches l{};
  const bool sentinel = v.xt_nonzero && v.t_safe && v.xt_positive && v.t_positive;
  const bool acc32 = v.xt_all_ones && sentinel && v.t_all_ones;
  l.sentinel = sentinel;
  l.acc32 = acc32;
  if (v.xt_all_ones) {
    const bool divides = v.sim_type == IRS_SIM_COSINE || v.sim_type == IRS_SIM_ASYMMETRIC ||
                         v.sim_type == IRS_SIM_JACCARD || v.sim_type == IRS_SIM_TVERSKY;
    const bool tv_ok = v.sim_type != IRS_SIM_TVERSKY ||
                       (v.alpha >= 0.0 && v.alpha <= 16.0 && v.beta >= 0.0 && v.beta <= 16.0 &&
                        v.norm_max < 16777216.0 && v.tstat_max < 16777216.0);
    const bool as_ok = v.sim_type != IRS_SIM_ASYMMETRIC || (v.alpha >= 0.0 && v.alpha <= 1.0);
    const bool fast = acc32 && !v.col_scaled && !v.big && static_cast<int32_t>(v.top_k) <= FAST_CAP / 2 && divides && tv_ok && as_ok && v.shrinkage >= 0.0 &&
                      v.shrinkage < 1e30 &&
                      v.fast_allowed;
    if (fast) {
      l.first = 0;
      l.redo = true;
    } else if (acc32) l.first = 1;
    else if (sentinel) l.first = 2;
    else l.first = 3;
  } else if (v.xt_row_const) {
    if (sentinel) l.first = 2; else l.first = 3;
  } else {
    if (sentinel) l.first = 4; else l.first = 5;
  }
  return l;
}

static void variant_choices() {
  struct Corner { int32_t sim; double alpha, beta, shrinkage, norm_max, tstat_max; };
  const double two24 = 16777216.0;
  const Corner corners[] = {
      {IRS_SIM_COSINE, 0, 0, 0.0, 50, 50},        {IRS_SIM_COSINE, 0, 0, 1e31, 50, 50},     {IRS_SIM_COSINE, 0, 0, 1e29, 50, 50},
      {IRS_SIM_ASYMMETRIC, 0.7, 0, 1.0, 50, 50},  {IRS_SIM_ASYMMETRIC, 1.5, 0, 1.0, 50, 50}, {IRS_SIM_ASYMMETRIC, 1.0, 0, 1.0, 50, 50},
      {IRS_SIM_JACCARD, 0, 0, 1.5, 50, 50},       {IRS_SIM_TVERSKY, 0.7, 2.0, 0, 50, 50},    {IRS_SIM_TVERSKY, 0.7, 17.0, 0, 50, 50},
      {IRS_SIM_TVERSKY, 17.0, 2.0, 0, 50, 50},    {IRS_SIM_TVERSKY, 0.7, 2.0, 0, two24, 50}, {IRS_SIM_TVERSKY, 0.7, 2.0, 0, 50, two24},
      {IRS_SIM_TVERSKY, 16.0, 16.0, 0, two24 - 1, two24 - 1}, {IRS_SIM_P3ALPHA, 0.5, 0, 0, 0, 0}, {IRS_SIM_RP3BETA, 0.7, 0.4, 0, 0, 0}};
  const int64_t top_ks[] = {1, FAST_CAP / 2, FAST_CAP / 2 + 1, TOPK_CAP, TOPK_CAP + 1};
  int64_t cases = 0, fast_cases = 0;
  for (unsigned mask = 0; mask < (1u << 10); mask++)
    for (const Corner &k : corners)
      for (const int64_t top_k : top_ks) {
        VariantInputs v;
        v.xt_all_ones = mask & 1;
        v.xt_row_const = mask & 2;
        v.xt_nonzero = mask & 4;
        v.xt_positive = mask & 8;
        v.col_scaled = mask & 16;
        v.t_all_ones = mask & 32;
        v.t_safe = mask & 64;
        v.t_positive = mask & 128;
        v.normalize = mask & 256;
        v.fast_allowed = mask & 512;
        v.sim_type = k.sim;
        v.alpha = k.alpha;
        v.beta = k.beta;
        v.shrinkage = k.shrinkage;
        v.norm_max = k.norm_max;
        v.tstat_max = k.tstat_max;
        v.top_k = top_k;
        v.big = top_k > TOPK_CAP;
        const Launches want = former_chain(v);
        const VariantChoice got = choose_variant(v);
        const TileVariant by_index[] = {TileVariant::FAST_COUNTS, TileVariant::COUNTS, TileVariant::ONES_SENTINEL,
                                        TileVariant::ONES_BITMAP, TileVariant::VALUES_SENTINEL, TileVariant::VALUES_BITMAP};
        EXPECT(got.first == by_index[want.first] && got.exact_redo == want.redo && got.acc32 == want.acc32 &&
               got.sentinel == want.sentinel);
        cases++;
        fast_cases += got.exact_redo;
      }
  EXPECT(cases == 1024 * 15 * 5 && fast_cases > 0 && fast_cases < cases / 8);
}

// ---------------------------------------------------------------- arena
static void arenas() {
  struct Call { int64_t n, ne, N, top_k, widest; int n_chunks; };
  const Call calls[] = {{0, 0, 200, 20, 0, 1}, {1, 0, 200, 20, 1, 1}, {1, 5, 1, 1, 1, 1}, {300, 4321, 200, 20, 120, 3},
                        {40, 900, 2 * TILE - 100, TILE + 50, 40, 1}, {17000, 85000, 17000, 2500, 17000, 1}};
  for (const Call &k : calls) {
    const int64_t out_k = std::min(k.top_k, k.N);
    const ArenaLayout L = arena_layout(k.n, static_cast<size_t>(k.ne), k.N, out_k, k.widest, k.n_chunks);
    // the former `take` expressions
    const size_t nn = static_cast<size_t>(k.n), ne = static_cast<size_t>(k.ne);
    const size_t n_tiles_a = static_cast<size_t>(ceil_div(std::max<int64_t>(k.N, 1), TILE));
    const size_t tile_k_a = static_cast<size_t>(std::min<int64_t>(out_k, TILE));
    const size_t slots_a = static_cast<size_t>(k.widest) * n_tiles_a, cap_a = nn * static_cast<size_t>(out_k);
    const size_t bytes[] = {(nn + 1) * 8, std::max<size_t>(ne, 1) * 4, nn * 8, nn * 8, nn * 4, nn * 4, (nn + 1) * 8,
                            slots_a * tile_k_a * 4, slots_a * tile_k_a * 8, slots_a * 4, cap_a * 4, cap_a * 8, nn * 4,
                            cap_a * 4, cap_a * 8, 3 * static_cast<size_t>(k.n_chunks) * 4, slots_a * 4};
    static_assert(sizeof(bytes) / sizeof(bytes[0]) == ARENA_BLOCKS, "seventeen blocks");
    size_t off = 0;
    for (int b = 0; b < ARENA_BLOCKS; b++) {
      EXPECT(L.offset[b] == off && L.offset[b] % 256 == 0);
      EXPECT(L.elem_size[b] * L.count[b] == bytes[b]);
      EXPECT(b + 1 == ARENA_BLOCKS || L.offset[b + 1] >= L.offset[b] + std::max<size_t>(bytes[b], 1));  // no overlap
      off += (std::max<size_t>(bytes[b], 1) + 255) & ~size_t(255);
    }
    EXPECT(L.total == off && L.total >= L.offset[ARENA_BLOCKS - 1] + std::max<size_t>(bytes[ARENA_BLOCKS - 1], 1));
  }
}

static void norm_finish() {
  for (const double ss : {0.0, 1.0, 7.0, 1234.5678}) {
    EXPECT(bits(finish_norm(IRS_SIM_COSINE, 0.7, ss)) == bits(std::sqrt(ss)));
    EXPECT(bits(finish_norm(IRS_SIM_ASYMMETRIC, 0.7, ss)) == bits(std::pow(ss, 1 - 0.7)));
    EXPECT(bits(finish_norm(IRS_SIM_JACCARD, 0.7, ss)) == bits(ss) && bits(finish_norm(IRS_SIM_TVERSKY, 0.7, ss)) == bits(ss));
  }
}

int main() {
  const Csr matrices[] = {random_csr(300, 200, 8, 17, 1), random_csr(257, 431, 5, 256, 2), random_csr(65, 300, 3, 0, 3),
                          random_csr(0, 0, 0, -1, 4)};
  uint32_t seed = 10;
  for (const Csr &m : matrices) {
    entry_scan(m);
    chunks(m);
    if (m.rows > 0) target_passes(m, seed++);
  }
  {  // an empty target against a computer with features: the pass of a call without rows
    const Csr &empty = matrices[3];
    std::vector<int64_t> len(1, 0);
    std::vector<double> r(1, 0.0);
    Tables t(0);
    const unsigned f = target_pass(empty.indptr.data(), nullptr, nullptr, 1, 0, 0, 0, FeatureRows{len.data(), r.data(), r.data()},
                                      IRS_SIM_COSINE, 0.5, false, WideRule(nullptr), 1, t.tstat.data(), t.tscale.data(), t.work.data());
    EXPECT(f == 0);
  }
  launch_orders(5);
  variant_choices();
  arenas();
  norm_finish();
  std::printf("knn_host_prep ok\n");
  return 0;
}
