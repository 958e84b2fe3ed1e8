// Host-only part of the Mult-VAE trainer (multvae.hip): argument checks, the layout of the parameter arena, the
// annealing schedule, Adam's bias corrections, the counter-based noise (shared with the kernels through
// IRS_BPR_HD; the order of an epoch is BPR's Feistel permutation, included from bpr_host_prep.hpp and not moved),
// the initial tables, the fixed-point scale of the W1 gradient and the K-slabs of the split reductions.  No HIP
// in it: it compiles with the host compiler alone (tests/host/multvae_host_prep_main.cpp).  DESIGN.md section 15.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "bpr_host_prep.hpp"

namespace irs {
namespace mv {

constexpr int MAX_HIDDEN = 574;      // the scoring factor model has Hd + 2 columns and the evaluator takes 576
constexpr int CONTRIB_CAP_LOG2 = 8;  // a contribution to the W1 gradient sums stays below 2^8 (else: diverged)
constexpr float CONTRIB_CAP = 256.f;
constexpr int MAX_SCALE_LOG2 = 44;   // 2^8 2^44 = 2^52: every scaled contribution is an exact double
constexpr int N_TABLES = 8;          // W1 b1 W2 b2 W3 b3 W4 b4
constexpr int DW4_SLAB = 256;        // batch rows per K-slab of d[W4; b4]
constexpr int DH2_SLAB_UNIT = 512;   // items per K-slab of dh2, times a factor that keeps the slabs <= 64
constexpr int DH2_MAX_SLABS = 64;

// ---- the parameter arena ----------------------------------------------------------------------------------------
// Four segments, each a weight table with its bias as one more row, row-major:
//   [W1; b1] (I + 1) x Hp (Hp = H rounded up to 4, zero padding that every kernel keeps zero)
//   [W2; b2] (H + 1) x 2 L,   [W3; b3] (L + 1) x Hd,   [W4; b4] (Hd + 1) x I
// The activations carry a ones column, so every bias and every bias gradient falls out of the table's product.
struct Table {
  int64_t rows, cols, offset, ld;  // of the host table (a bias: 1 row), and where it sits in the arena
  int64_t fan_in;                  // of a weight table; 0 for a bias
};
struct Layout {
  int64_t I = 0, H = 0, Hp = 0, L = 0, Hd = 0;
  int64_t seg[4] = {0, 0, 0, 0}, total = 0, w1_count = 0;
  Table table[N_TABLES];
  int64_t count(int q) const { return table[q].rows * table[q].cols; }
};
inline Layout make_layout(int64_t I, int64_t H, int64_t L, int64_t Hd) {
  Layout y;
  y.I = I, y.H = H, y.Hp = (H + 3) / 4 * 4, y.L = L, y.Hd = Hd;
  const int64_t rows[4] = {I + 1, H + 1, L + 1, Hd + 1}, ld[4] = {y.Hp, 2 * L, Hd, I}, cols[4] = {H, 2 * L, Hd, I};
  int64_t at = 0;
  for (int s = 0; s < 4; s++) {
    y.seg[s] = at;
    y.table[2 * s] = Table{rows[s] - 1, cols[s], at, ld[s], rows[s] - 1};
    y.table[2 * s + 1] = Table{1, cols[s], at + (rows[s] - 1) * ld[s], ld[s], 0};
    at += (rows[s] * ld[s] + 3) / 4 * 4;
  }
  y.total = at, y.w1_count = (I + 1) * y.Hp;
  return y;
}
// a host table (unpadded) into / out of an arena image (whose padding is zero)
inline void pack_table(const Layout &y, int q, const float *src, float *arena) {
  const Table &t = y.table[q];
  for (int64_t r = 0; r < t.rows; r++) std::memcpy(arena + t.offset + r * t.ld, src + r * t.cols, sizeof(float) * t.cols);
}
inline void unpack_table(const Layout &y, int q, const float *arena, float *dst) {
  const Table &t = y.table[q];
  for (int64_t r = 0; r < t.rows; r++) std::memcpy(dst + r * t.cols, arena + t.offset + r * t.ld, sizeof(float) * t.cols);
}

// ---- argument checks -------------------------------------------------------------------------------------------
inline void validate_hyper(int32_t dim_z, int32_t enc_hidden, int32_t dec_hidden, float dropout_p, float l2,
                           double kl_anneal_goal, int64_t anneal_end_epoch, int64_t minibatch_size, float learning_rate) {
  check_arg(dim_z >= 1, "dim_z must be >= 1.");
  check_arg(dim_z < (1 << 20), "dim_z must be below 2^20.");
  check_arg(enc_hidden >= 1 && dec_hidden >= 1, "enc_hidden_dims and dec_hidden_dims must be >= 1.");
  check_arg(enc_hidden <= MAX_HIDDEN && dec_hidden <= MAX_HIDDEN, "enc_hidden_dims and dec_hidden_dims must be <= 574.");
  check_arg(std::isfinite(dropout_p) && dropout_p >= 0.f && dropout_p < 1.f, "dropout_p must be in [0, 1).");
  check_arg(std::isfinite(l2), "l2_regularizer must be finite.");
  check_arg(std::isfinite(kl_anneal_goal) && kl_anneal_goal >= 0.0, "kl_anneal_goal must be finite and >= 0.");
  check_arg(anneal_end_epoch >= 0, "anneal_end_epoch must be >= 0.");
  check_arg(minibatch_size >= 1, "minibatch_size must be >= 1.");
  check_arg(minibatch_size < (int64_t(1) << 31), "minibatch_size must be below 2^31.");
  check_arg(std::isfinite(learning_rate) && learning_rate > 0.f, "learning_rate must be finite and > 0.");
}

inline void validate_finite(const float *t, int64_t n, const char *msg) {
  for (int64_t q = 0; q < n; q++) check_arg(std::isfinite(t[q]), msg);
}
// the 8 tables, or the 24 of a state (tables, first moments, second moments >= 0)
inline void validate_tables(const Layout &y, const float *const *tables, int n_groups, const char *null_msg,
                            const char *non_finite) {
  check_arg(tables != nullptr, null_msg);
  for (int q = 0; q < N_TABLES * n_groups; q++) check_arg(tables[q] != nullptr, null_msg);
  for (int q = 0; q < N_TABLES * n_groups; q++) validate_finite(tables[q], y.count(q % N_TABLES), non_finite);
  if (n_groups == 3)
    for (int q = 2 * N_TABLES; q < 3 * N_TABLES; q++)
      for (int64_t e = 0; e < y.count(q % N_TABLES); e++)
        check_arg(tables[q][e] >= 0.f, "the second moments of the state must be >= 0.");
}

inline void validate_batch(int64_t n, const int32_t *users, int64_t n_users, double klc) {
  check_arg(n >= 1, "a batch must have at least one row.");
  check_arg(n < (int64_t(1) << 31), "n must be below 2^31.");
  check_arg(users != nullptr, "users must not be null.");
  for (int64_t q = 0; q < n; q++) check_arg(users[q] >= 0 && users[q] < n_users, "a batch row's user is out of range.");
  check_arg(std::isfinite(klc) && klc >= 0.0, "klc must be finite and >= 0.");
}
inline void validate_noise(int64_t n_keep, const uint8_t *keep, int64_t n_eps, const float *eps) {
  if (keep)
    for (int64_t q = 0; q < n_keep; q++) check_arg(keep[q] <= 1, "keep must hold 0 or 1.");
  if (eps) validate_finite(eps, n_eps, "eps holds a non-finite value.");
}

// ---- the schedule and Adam ---------------------------------------------------------------------------------------
// multvae.py:161, :244-247 (anneal_end_epoch = 0, where the reference divides by zero: the goal from the start)
inline double kl_coefficient(double goal, int64_t update, int64_t anneal_end_epoch, int64_t n_users, int64_t minibatch) {
  const double total = static_cast<double>(anneal_end_epoch) * static_cast<double>(n_users) / static_cast<double>(minibatch);
  if (!(total > 0.0)) return goal;
  const double r = static_cast<double>(update) / total;
  return goal * (r < 1.0 ? r : 1.0);
}
// 1 - beta^(t + 1) of optax's bias correction, t = updates done before this one
inline double bias_correction(double beta, int64_t update) { return 1.0 - std::pow(beta, static_cast<double>(update + 1)); }

// ---- the noise -------------------------------------------------------------------------------------------------
// the key of one stream of one update (stream 0: dropout, 1: eps)
IRS_BPR_HD uint64_t noise_key(uint64_t seed, int64_t update, uint64_t stream) {
  return bpr::mix64(bpr::mix64(seed ^ 0x4D565F4E4F495345ull) ^ bpr::mix64(static_cast<uint64_t>(update) * 2 + stream));
}
IRS_BPR_HD uint64_t noise_hash(uint64_t key, uint32_t user, uint32_t index) {
  return bpr::mix64(key ^ bpr::mix64((static_cast<uint64_t>(user) << 32) | index));
}
// dropout: the entry stays when the top 24 bits of its hash reach p 2^24, so P(keep) = 1 - p to 2^-24
inline uint32_t keep_threshold(float p) { return static_cast<uint32_t>(std::llrint(static_cast<double>(p) * 16777216.0)); }
IRS_BPR_HD bool keep_entry(uint64_t key, uint32_t user, uint32_t position, uint32_t threshold) {
  return static_cast<uint32_t>(noise_hash(key, user, position) >> 40) >= threshold;
}
// Box-Muller on two 24-bit uniforms of one hash: u1 in (0, 1], u2 in [0, 1)
IRS_BPR_HD float gauss(uint64_t key, uint32_t user, uint32_t component) {
  const uint64_t h = noise_hash(key, user, component);
  const float u1 = (static_cast<float>(h >> 40) + 1.0f) * (1.0f / 16777216.0f);
  const float u2 = static_cast<float>((h >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// the order of an epoch: BPR's permutation of [0, n_users) under a key of this model's own
inline bpr::Perm epoch_perm(uint64_t seed, int64_t epoch, int64_t n_users) {
  return bpr::make_perm(bpr::epoch_key(seed ^ 0x4D565F4F52444552ull, epoch, 0), n_users);
}

// ---- the initial tables -------------------------------------------------------------------------------------------
// truncated normal at +-2 sigma, sigma = 1 / sqrt(fan_in) (haiku's Linear): Box-Muller in double, redrawn with the
// next attempt number until it lies inside
inline float init_value(uint64_t seed, uint64_t table, uint64_t index, int64_t fan_in) {
  const uint64_t key = bpr::mix64(bpr::mix64(seed ^ 0x4D565F494E4954ull) ^ bpr::mix64(table + 1));
  for (uint64_t attempt = 0;; attempt++) {
    const uint64_t a = bpr::mix64(key ^ bpr::mix64(index * 64 + attempt)), b = bpr::mix64(a ^ 0x9E3779B97F4A7C15ull);
    const double u1 = (static_cast<double>(a >> 11) + 1.0) * (1.0 / 9007199254740992.0);
    const double u2 = static_cast<double>(b >> 11) * (1.0 / 9007199254740992.0);
    const double z = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586476925 * u2);
    if (std::fabs(z) <= 2.0 || attempt == 63) {
      const double c = std::fabs(z) <= 2.0 ? z : 0.0;
      return static_cast<float>(c / std::sqrt(static_cast<double>(fan_in)));
    }
  }
}
inline void init_tables(const Layout &y, uint64_t seed, std::vector<float> *tables) {
  for (int q = 0; q < N_TABLES; q++) {
    tables[q].assign(static_cast<size_t>(y.count(q)), 0.f);
    if (y.table[q].fan_in == 0) continue;
    for (size_t e = 0; e < tables[q].size(); e++) tables[q][e] = init_value(seed, static_cast<uint64_t>(q), e, y.table[q].fan_in);
  }
}

// ---- the fixed-point scale and the K-slabs ---------------------------------------------------------------------
// An element of the W1 gradient (and of b1's, the table's last row) is a sum of at most n contributions, one per
// batch row, each below 2^CONTRIB_CAP_LOG2 (the kernel raises the flag otherwise) - so the sum stays below
// 2^(log2ceil(n) + CONTRIB_CAP_LOG2).  The scale is the largest power of two that keeps the scaled bound below
// 2^62, capped at 2^MAX_SCALE_LOG2.
inline int scale_log2(int64_t n) {
  int lg = 0;
  while ((int64_t(1) << lg) < n) lg++;
  const int s = 62 - (lg + CONTRIB_CAP_LOG2);
  return s < MAX_SCALE_LOG2 ? s : MAX_SCALE_LOG2;
}
// items per K-slab of dh2 = g W4^T: a function of n_items alone, so a batch's bytes do not depend on its length
inline int32_t dh2_slab(int64_t n_items) {
  const int64_t f = ceil_div(n_items, int64_t(DH2_SLAB_UNIT) * DH2_MAX_SLABS);
  return static_cast<int32_t>(DH2_SLAB_UNIT * (f < 1 ? 1 : f));
}

// lanes that serve one stored entry in the two sparse kernels (one float4 of the H axis per lane and pass) and
// the passes a lane makes: a power of two up to a wave, then up to 3 passes (Hp <= 576)
inline int lanes_per_entry(int64_t Hp) {
  const int64_t chunks = Hp / 4;
  int l = 1;
  while (l < chunks && l < 64) l *= 2;
  return l;
}
inline int chunks_per_lane(int64_t Hp) { return static_cast<int>(ceil_div(Hp / 4, lanes_per_entry(Hp))); }

}  // namespace mv
}  // namespace irs
