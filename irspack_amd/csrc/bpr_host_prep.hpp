// Host-only part of the BPR trainer (bpr.hip): argument checks, the filter of the positives, the per-entry
// arrays of the sampler, the counter-based generator with its permutation and unseen-rank mapping (shared with
// the kernels through IRS_BPR_HD), the fixed-point scale of the gradient sums, and what the WARP loss adds to these
// (its candidate stream, weight table, scale and checks).  No HIP in it: it compiles with the host compiler alone
// (tests/host/bpr_host_prep_main.cpp, warp_host_prep_main.cpp).  DESIGN.md section 14.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "host_util.hpp"

#if defined(__HIPCC__)
#define IRS_BPR_HD __host__ __device__ __forceinline__
#else
#define IRS_BPR_HD inline
#endif

namespace irs {
namespace bpr {

constexpr int MAX_K = 512;
// |theta| of every parameter stays below 2^PARAM_CAP_LOG2: the apply kernel raises a flag beyond it and the call
// fails (a sigmoid of such a dot product has long saturated - the fit has diverged).  The fixed-point scale
// is derived from this bound, so the bound has to hold, not just to be likely.
constexpr int PARAM_CAP_LOG2 = 8;
constexpr float PARAM_CAP = 256.f;
constexpr int MAX_SCALE_LOG2 = 44;  // 2 PARAM_CAP 2^44 = 2^53: every scaled contribution is an exact double

// ---- the generator: splitmix64's finaliser as a counter-based hash --------------------------------------------
IRS_BPR_HD uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the key of one stream of one epoch (stream 0: the order, 1: the negatives)
IRS_BPR_HD uint64_t epoch_key(uint64_t seed, int64_t epoch, uint64_t stream) {
  return mix64(mix64(seed) ^ mix64(static_cast<uint64_t>(epoch) * 2 + stream + 0x632BE59BD9B4E019ull));
}

// Balanced Feistel network over [0, 2^(2 half)) with cycle walking down to [0, n): a bijection of [0, n) for
// every key.  2^(2 half) < 4 n, so a walk takes fewer than 4 rounds of the network on average; it ends because
// the network is a permutation whose cycle through x returns to x < n.
struct Perm {
  uint64_t key;
  uint32_t n, half, mask;
};
inline Perm make_perm(uint64_t key, int64_t n) {
  int bits = 2;
  while (bits < 32 && (int64_t(1) << bits) < n) bits += 2;
  Perm p;
  p.key = key, p.n = static_cast<uint32_t>(n), p.half = static_cast<uint32_t>(bits / 2);
  p.mask = (1u << p.half) - 1u;
  return p;
}
IRS_BPR_HD uint32_t feistel(const Perm &p, uint32_t x) {
  uint32_t l = x >> p.half, r = x & p.mask;
  for (uint32_t round = 0; round < 6; round++) {
    const uint32_t f = static_cast<uint32_t>(mix64(p.key ^ (static_cast<uint64_t>(round + 1) << 32) ^ r)) & p.mask;
    const uint32_t t = l ^ f;
    l = r, r = t;
  }
  return (l << p.half) | r;
}
IRS_BPR_HD uint32_t permute(const Perm &p, uint32_t x) {
  do x = feistel(p, x);
  while (x >= p.n);
  return x;
}

// high 64 bits of a 64 x 64 product: h uniform over 2^64 -> [0, range) without a rejection loop
IRS_BPR_HD uint64_t mul_hi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}
IRS_BPR_HD uint32_t draw_rank(uint64_t key, uint64_t position, uint32_t range) {
  return static_cast<uint32_t>(mul_hi(mix64(key ^ mix64(position)), range));
}

// the r-th (from 0) column that the sorted row s[0 .. deg) does not hold: r + #{m : s[m] - m <= r}.  s[m] - m
// does not decrease in m, so the count is one binary search; its trip count depends on deg alone.
IRS_BPR_HD int32_t unseen_by_rank(const int32_t *s, int32_t deg, int32_t r) {
  int32_t lo = 0, hi = deg;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (s[mid] - mid <= r) lo = mid + 1;
    else hi = mid;
  }
  return r + lo;
}

// uniform in (-0.5, 0.5) / k from 24 bits of the hash (LightFM's initial embeddings)
inline float init_value(uint64_t seed, uint64_t table, uint64_t index, int32_t k) {
  const uint64_t h = mix64(mix64(seed ^ (table << 62)) ^ mix64(index));
  const float u = (static_cast<float>(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
  return (u - 0.5f) / static_cast<float>(k);
}

// ---- argument checks -------------------------------------------------------------------------------------------
// (the matrix itself: csr_checks.hpp's validate_finite_matrix)
inline void validate_hyper(int32_t k, float user_alpha, float item_alpha, float learning_rate, int64_t batch_size) {
  check_arg(k >= 1, "k must be >= 1.");
  check_arg(k <= MAX_K, "k must be <= 512.");
  check_arg(batch_size >= 1, "batch_size must be >= 1.");
  for (float a : {user_alpha, item_alpha}) check_arg(std::isfinite(a) && a >= 0.f, "the alphas must be finite and >= 0.");
  check_arg(std::isfinite(learning_rate) && learning_rate >= 0.f, "learning_rate must be finite and >= 0.");
  check_arg(learning_rate != 0.f, "learning_rate must not be 0.");
}

// a parameter table: finite and inside the cap the fixed-point sums are scaled for
inline void validate_table(const float *t, int64_t n, const char *non_finite, const char *too_large) {
  for (int64_t q = 0; q < n; q++) {
    check_arg(std::isfinite(t[q]), non_finite);
    check_arg(std::fabs(t[q]) < PARAM_CAP, too_large);
  }
}
inline void validate_accumulator(const float *g, int64_t n) {
  for (int64_t q = 0; q < n; q++)
    check_arg(std::isfinite(g[q]) && g[q] > 0.f, "the Adagrad accumulators must be finite and > 0.");
}

inline void validate_triples(int64_t n, const int32_t *users, const int32_t *pos, const int32_t *neg, int64_t n_users,
                             int64_t n_items) {
  check_arg(n >= 0, "n must be >= 0.");
  check_arg(n < (int64_t(1) << 31), "n must be below 2^31.");
  check_arg(n == 0 || (users && pos && neg), "the triple arrays must not be null.");
  for (int64_t q = 0; q < n; q++) {
    check_arg(users[q] >= 0 && users[q] < n_users, "a triple's user is out of range.");
    check_arg(pos[q] >= 0 && pos[q] < n_items && neg[q] >= 0 && neg[q] < n_items, "a triple's item is out of range.");
  }
}

// ---- the positives ----------------------------------------------------------------------------------------------
// The stored entries > 0 as a CSR pattern (what "seen" means to the sampler), and the entries an epoch draws
// from, by user and item: those of rows that are not full (a full row has no negative).
struct Positives {
  std::vector<int32_t> indptr, indices;      // the filtered rows, every row
  std::vector<int32_t> pos_user, pos_item;   // the entries an epoch uses, in row order
  int64_t n_positives = 0, n_skipped_rows = 0, n_skipped_positives = 0;
};
inline Positives filter_positives(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                                  const float *data) {
  Positives p;
  p.indptr.assign(static_cast<size_t>(n_users) + 1, 0);
  for (int64_t u = 0; u < n_users; u++) {
    for (int64_t q = indptr[u]; q < indptr[u + 1]; q++)
      if (data[q] > 0.f) p.indices.push_back(indices[q]);
    p.indptr[u + 1] = static_cast<int32_t>(p.indices.size());
  }
  p.n_positives = static_cast<int64_t>(p.indices.size());
  for (int64_t u = 0; u < n_users; u++) {
    const int32_t b = p.indptr[u], e = p.indptr[u + 1];
    if (e - b == n_items) {
      p.n_skipped_rows++;
      p.n_skipped_positives += e - b;
      continue;
    }
    for (int32_t q = b; q < e; q++) {
      p.pos_user.push_back(static_cast<int32_t>(u));
      p.pos_item.push_back(p.indices[q]);
    }
  }
  return p;
}

// one triple of an epoch on the host, as the sampler kernel computes it
inline void sample_one(const Positives &p, int64_t n_items, const Perm &perm, uint64_t neg_key, int64_t position,
                       int32_t *u, int32_t *i, int32_t *j) {
  const uint32_t e = permute(perm, static_cast<uint32_t>(position));
  *u = p.pos_user[e], *i = p.pos_item[e];
  const int32_t b = p.indptr[*u], deg = p.indptr[*u + 1] - b;
  const uint32_t r = draw_rank(neg_key, static_cast<uint64_t>(position), static_cast<uint32_t>(n_items - deg));
  *j = unseen_by_rank(p.indices.data() + b, deg, static_cast<int32_t>(r));
}

// ---- the fixed-point scale -------------------------------------------------------------------------------------
// A row's gradient over a batch of n triples is a sum of at most 2 n contributions (a triple adds to its user's
// row once, and to an item's row at most twice: as the positive and as the negative), each of magnitude
// |w| |theta| < 2 PARAM_CAP (w in (0, 1); a difference of two parameters for the user's row) - so the sum stays
// below 4 n PARAM_CAP = 2^(log2ceil(n) + 2 + PARAM_CAP_LOG2).  The scale is the largest power of two that
// keeps the scaled bound below 2^62, capped at 2^MAX_SCALE_LOG2.
inline int scale_log2(int64_t n) {
  int lg = 0;
  while ((int64_t(1) << lg) < n) lg++;
  const int s = 62 - (lg + 2 + PARAM_CAP_LOG2);
  return s < MAX_SCALE_LOG2 ? s : MAX_SCALE_LOG2;
}

// ---- WARP (loss "warp": DESIGN.md section 14, "WARP") ---------------------------------------------------------
constexpr int WARP_MAX_SAMPLED = 256;  // candidate t of position p draws from counter p * 256 + t, 1 <= t <= 256
constexpr double WARP_MAX_LOSS = 10.0;       // LightFM's MAX_LOSS
constexpr int WARP_WEIGHT_LOG2 = 4;          // every weight is <= 10 < 2^4
constexpr int WARP_MAX_SCALE_LOG2 = 40;      // 2^4 2 PARAM_CAP 2^40 = 2^53: every scaled contribution is an exact double

// The key of an epoch's candidate stream.  epoch_key's streams enter as 2 epoch + stream, so a third stream there
// would be the order key of the next epoch; this derivation shares no counter with it.
IRS_BPR_HD uint64_t warp_key(uint64_t seed, int64_t epoch) {
  return mix64(mix64(seed) ^ mix64(mix64(static_cast<uint64_t>(epoch)) + 0xD1B54A32D192ED03ull));
}

// candidate t (from 1) of a position whose user has the sorted row s[0 .. deg): it does not depend on max_sampled
IRS_BPR_HD int32_t warp_candidate(uint64_t key, uint64_t position, int32_t t, const int32_t *s, int32_t deg,
                                  int32_t n_items) {
  const uint32_t r = draw_rank(key, position * WARP_MAX_SAMPLED + static_cast<uint64_t>(t),
                               static_cast<uint32_t>(n_items - deg));
  return unseen_by_rank(s, deg, static_cast<int32_t>(r));
}

// (u, i) of a position and its first `count` candidates on the host, as the kernels compute them
inline void warp_candidates_one(const Positives &p, int64_t n_items, const Perm &perm, uint64_t key, int64_t position,
                                int32_t count, int32_t *u, int32_t *i, int32_t *cand) {
  const uint32_t e = permute(perm, static_cast<uint32_t>(position));
  *u = p.pos_user[e], *i = p.pos_item[e];
  const int32_t b = p.indptr[*u], deg = p.indptr[*u + 1] - b;
  for (int32_t t = 1; t <= count; t++)
    cand[t - 1] = warp_candidate(key, static_cast<uint64_t>(position), t, p.indices.data() + b, deg,
                                 static_cast<int32_t>(n_items));
}

// w_t = min(ln(max(1, floor((n_items - 1) / t))), 10), t = 1 .. max_sampled: LightFM's rank estimate when the first
// violation is found at try t, in double, once per handle (the device needs no log; the restatement uses the same)
inline std::vector<double> warp_weights(int64_t n_items, int32_t max_sampled) {
  std::vector<double> w(static_cast<size_t>(max_sampled));
  for (int32_t t = 1; t <= max_sampled; t++) {
    const int64_t rank = (n_items - 1) / t;
    w[t - 1] = std::min(std::log(static_cast<double>(rank < 1 ? 1 : rank)), WARP_MAX_LOSS);
  }
  return w;
}

// the scale of a WARP batch: a contribution is bounded by 2^4 2 PARAM_CAP instead of 2 PARAM_CAP
inline int warp_scale_log2(int64_t n) {
  int lg = 0;
  while ((int64_t(1) << lg) < n) lg++;
  const int s = 62 - (lg + 2 + PARAM_CAP_LOG2 + WARP_WEIGHT_LOG2);
  return s < WARP_MAX_SCALE_LOG2 ? s : WARP_MAX_SCALE_LOG2;
}

inline void validate_max_sampled(int32_t max_sampled) {
  check_arg(max_sampled >= 1, "max_sampled must be >= 1.");
  check_arg(max_sampled <= WARP_MAX_SAMPLED, "max_sampled must be <= 256.");
}

// positions with the caller's candidates: cand is n x max_sampled, row-major
inline void validate_warp_batch(int64_t n, const int32_t *users, const int32_t *pos, const int32_t *cand,
                                int32_t max_sampled, int64_t n_users, int64_t n_items) {
  check_arg(n >= 0, "n must be >= 0.");
  check_arg(n * max_sampled < (int64_t(1) << 31), "n * max_sampled must be below 2^31.");
  check_arg(n == 0 || (users && pos && cand), "the position and candidate arrays must not be null.");
  for (int64_t q = 0; q < n; q++) {
    check_arg(users[q] >= 0 && users[q] < n_users, "a position's user is out of range.");
    check_arg(pos[q] >= 0 && pos[q] < n_items, "a position's item is out of range.");
    for (int64_t c = q * max_sampled; c < (q + 1) * max_sampled; c++)
      check_arg(cand[c] >= 0 && cand[c] < n_items, "a candidate is out of range.");
  }
}

// lanes that serve one triple (and one row of the apply kernel): one float4 per lane up to a whole wave
inline int lanes_per_triple(int32_t k) {
  const int chunks = (k + 3) / 4;
  int l = 1;
  while (l < chunks && l < 64) l *= 2;
  return l;
}

}  // namespace bpr
}  // namespace irs
