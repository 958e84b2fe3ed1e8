// Kernels of the BPR trainer (bpr.hip): the sampler, the gradient of one synchronous
// batch and the Adagrad step on the rows the batch touched; for the WARP loss the candidate kernel, the search that
// is also its gradient, and the apply variant that skips a position without a violation.
//
// Tables are row-major float32 with row stride kp = k rounded up to 4 (zero padding that every kernel keeps
// zero), read as float4.  L lanes serve one triple / one row (L = lanes_per_triple(k): a power of two, one float4
// per lane up to K = 256, a whole wave with two float4 per lane above), 256 / L triples per workgroup.
//
// The per-row gradient sums are 64-bit fixed-point integers added with integer atomics - exact, so the sum does
// not depend on the order of arrival and two runs give the same bytes.  An accumulator row holds its kp values
// as [4][kp / 4] (component e of float4 chunk c at e * kp / 4 + c): the lanes of one atomic instruction then
// address consecutive 8-byte words.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bpr_host_prep.hpp"

namespace irs {
namespace bpr {

constexpr int BLOCK = 256;
constexpr int WARP_COUNTER_SLOTS = 1024, WARP_COUNTER_STRIDE = 4;  // (3 counters per slot, a slot 32 bytes)

// positions [first, first + count) of an epoch -> (u, i, j); one thread per position
__global__ void __launch_bounds__(BLOCK)
bpr_sample_kernel(Perm perm, uint64_t neg_key, int64_t first, int32_t count, int32_t n_items,
                  const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                  const int32_t *__restrict__ pos_user, const int32_t *__restrict__ pos_item,
                  int32_t *__restrict__ users, int32_t *__restrict__ pos, int32_t *__restrict__ neg) {
  const int32_t t = static_cast<int32_t>(blockIdx.x) * BLOCK + static_cast<int32_t>(threadIdx.x);
  if (t >= count) return;
  const uint64_t position = static_cast<uint64_t>(first + t);
  const uint32_t e = permute(perm, static_cast<uint32_t>(position));
  const int32_t u = pos_user[e], b = indptr[u], deg = indptr[u + 1] - b;
  const uint32_t r = draw_rank(neg_key, position, static_cast<uint32_t>(n_items - deg));
  users[t] = u;
  pos[t] = pos_item[e];
  neg[t] = unseen_by_rank(indices + b, deg, static_cast<int32_t>(r));
}

__device__ __forceinline__ void add_fixed(unsigned long long *acc, double c, double scale) {
  const long long q = __double2ll_rn(c * scale);
  atomicAdd(acc, static_cast<unsigned long long>(q));
}

// One batch's gradient: every triple reads the parameters as the batch found them and adds its five
// contributions to the fixed-point sums.  The arithmetic between the float32 loads and the integer sums is in
// double (the kernel waits for its gathers and its atomics, not for its arithmetic), so a contribution carries
// the rounding of the fixed-point step alone.  NCH: float4 chunks per lane (2 only with L = 64 and K > 256).
template <int L, int NCH>
__global__ void __launch_bounds__(BLOCK)
bpr_grad_kernel(int32_t n, int32_t kp, const int32_t *__restrict__ users, const int32_t *__restrict__ pos,
                const int32_t *__restrict__ neg, const float *__restrict__ U, const float *__restrict__ V,
                const float *__restrict__ b, unsigned long long *__restrict__ accU,
                unsigned long long *__restrict__ accV, unsigned long long *__restrict__ accb, double scale) {
  const int32_t t = static_cast<int32_t>((static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x) / L);
  const int lane = static_cast<int>(threadIdx.x) % L;
  if (t >= n) return;  // (whole groups leave: the shuffles below stay inside a group)
  const int32_t u = users[t], i = pos[t], j = neg[t];
  const int nchunk = kp / 4;
  const float4 *Ur = reinterpret_cast<const float4 *>(U + static_cast<int64_t>(u) * kp);
  const float4 *Vi = reinterpret_cast<const float4 *>(V + static_cast<int64_t>(i) * kp);
  const float4 *Vj = reinterpret_cast<const float4 *>(V + static_cast<int64_t>(j) * kp);
  float4 pu[NCH];
  double d[NCH][4];
  double x = 0.0;
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    const int c = lane + h * L;
    pu[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    d[h][0] = d[h][1] = d[h][2] = d[h][3] = 0.0;
    if (c < nchunk) {
      pu[h] = Ur[c];
      const float4 vi = Vi[c], vj = Vj[c];
      d[h][0] = static_cast<double>(vi.x) - vj.x, d[h][1] = static_cast<double>(vi.y) - vj.y;
      d[h][2] = static_cast<double>(vi.z) - vj.z, d[h][3] = static_cast<double>(vi.w) - vj.w;
      x += pu[h].x * d[h][0] + pu[h].y * d[h][1] + pu[h].z * d[h][2] + pu[h].w * d[h][3];
    }
  }
#pragma unroll
  for (int m = L / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, L);  // (the same bits in every lane of the group)
  x += static_cast<double>(b[i]) - static_cast<double>(b[j]);
  const double w = 1.0 / (1.0 + exp(x));
  unsigned long long *au = accU + static_cast<int64_t>(u) * kp;
  unsigned long long *ai = accV + static_cast<int64_t>(i) * kp;
  unsigned long long *aj = accV + static_cast<int64_t>(j) * kp;
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    const int c = lane + h * L;
    if (c >= nchunk) continue;
    const float uu[4] = {pu[h].x, pu[h].y, pu[h].z, pu[h].w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int at = e * nchunk + c;
      add_fixed(au + at, -w * d[h][e], scale);
      add_fixed(ai + at, -w * uu[e], scale);
      add_fixed(aj + at, w * uu[e], scale);
    }
  }
  if (lane == 0) {
    add_fixed(accb + i, -w, scale);
    add_fixed(accb + j, w, scale);
  }
}

// theta -= lr g / sqrt(G), then G += g^2, with g = the batch sum + alpha theta; the sum is set back to zero.  In
// double, rounded to float32 once per stored value.
__device__ __forceinline__ void adagrad(float &theta, float &G, unsigned long long &acc, double inv_scale, float alpha,
                                        float lr, bool &bad) {
  const double g = static_cast<double>(static_cast<long long>(acc)) * inv_scale +
                   static_cast<double>(alpha) * static_cast<double>(theta);
  acc = 0ull;
  theta = static_cast<float>(static_cast<double>(theta) - static_cast<double>(lr) * g / sqrt(static_cast<double>(G)));
  G = static_cast<float>(static_cast<double>(G) + g * g);
  bad |= !(fabsf(theta) < PARAM_CAP);
}

template <int L>
__device__ __forceinline__ void apply_row(int lane, int32_t kp, float *__restrict__ T, float *__restrict__ G,
                                          unsigned long long *__restrict__ acc, double inv_scale, float alpha, float lr,
                                          bool &bad) {
  const int nchunk = kp / 4;
  float4 *T4 = reinterpret_cast<float4 *>(T), *G4 = reinterpret_cast<float4 *>(G);
  for (int c = lane; c < nchunk; c += L) {
    float4 th = T4[c], gg = G4[c];
    unsigned long long a0 = acc[c], a1 = acc[nchunk + c], a2 = acc[2 * nchunk + c], a3 = acc[3 * nchunk + c];
    adagrad(th.x, gg.x, a0, inv_scale, alpha, lr, bad);
    adagrad(th.y, gg.y, a1, inv_scale, alpha, lr, bad);
    adagrad(th.z, gg.z, a2, inv_scale, alpha, lr, bad);
    adagrad(th.w, gg.w, a3, inv_scale, alpha, lr, bad);
    T4[c] = th, G4[c] = gg;
    acc[c] = a0, acc[nchunk + c] = a1, acc[2 * nchunk + c] = a2, acc[3 * nchunk + c] = a3;
  }
}

// The rows the batch touched, each exactly once: the group of a triple claims its user row and its two item rows
// by exchanging the batch number into the row's stamp; whoever finds an older stamp there does the row.  Every
// row's new value depends on its own sums alone, so it does not matter which group wins.
template <int L>
__global__ void __launch_bounds__(BLOCK)
bpr_apply_kernel(int32_t n, int32_t kp, const int32_t *__restrict__ users, const int32_t *__restrict__ pos,
                 const int32_t *__restrict__ neg, unsigned long long batch_no, unsigned long long *__restrict__ stampU,
                 unsigned long long *__restrict__ stampV, float *__restrict__ U, float *__restrict__ V,
                 float *__restrict__ b, float *__restrict__ GU, float *__restrict__ GV, float *__restrict__ Gb,
                 unsigned long long *__restrict__ accU, unsigned long long *__restrict__ accV,
                 unsigned long long *__restrict__ accb, double inv_scale, float user_alpha, float item_alpha, float lr,
                 int32_t *__restrict__ diverged) {
  const int32_t t = static_cast<int32_t>((static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x) / L);
  const int lane = static_cast<int>(threadIdx.x) % L;
  if (t >= n) return;
  bool bad = false;
  const int32_t rows[3] = {users[t], pos[t], neg[t]};
#pragma unroll
  for (int which = 0; which < 3; which++) {
    const int64_t r = rows[which];
    int won = 0;
    if (lane == 0) won = atomicExch((which == 0 ? stampU : stampV) + r, batch_no) != batch_no;
    won = __shfl(won, 0, L);
    if (!won) continue;
    if (which == 0) {
      apply_row<L>(lane, kp, U + r * kp, GU + r * kp, accU + r * kp, inv_scale, user_alpha, lr, bad);
    } else {
      apply_row<L>(lane, kp, V + r * kp, GV + r * kp, accV + r * kp, inv_scale, item_alpha, lr, bad);
      if (lane == 0) adagrad(b[r], Gb[r], accb[r], inv_scale, item_alpha, lr, bad);
    }
  }
  if (bad) *diverged = 1;
}

// ---- WARP ------------------------------------------------------------------------------------------------------
// candidates [first, first + count) x [1, max_sampled] of an epoch, and each position's (u, i); one thread per
// candidate (irs_bpr_warp_candidates: the epoch's own search computes them in place, below)
__global__ void __launch_bounds__(BLOCK)
warp_candidates_kernel(Perm perm, uint64_t key, int64_t first, int32_t count, int32_t max_sampled, int32_t n_items,
                       const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                       const int32_t *__restrict__ pos_user, const int32_t *__restrict__ pos_item,
                       int32_t *__restrict__ users, int32_t *__restrict__ pos, int32_t *__restrict__ cand) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (q >= static_cast<int64_t>(count) * max_sampled) return;
  const int32_t p = static_cast<int32_t>(q / max_sampled), t = static_cast<int32_t>(q % max_sampled) + 1;
  const uint64_t position = static_cast<uint64_t>(first + p);
  const uint32_t e = permute(perm, static_cast<uint32_t>(position));
  const int32_t u = pos_user[e], b = indptr[u], deg = indptr[u + 1] - b;
  if (t == 1) users[p] = u, pos[p] = pos_item[e];
  cand[q] = warp_candidate(key, position, t, indices + b, deg, n_items);
}

// unseen_by_rank for F ranks of one row with the F binary searches in step: their loads do not depend on one
// another, so they are in flight together.  Each search is unseen_by_rank's own sequence of comparisons.
template <int F>
__device__ __forceinline__ void unseen_by_ranks(const int32_t *__restrict__ s, int32_t deg, const bool (&valid)[F],
                                                const int32_t (&r)[F], int32_t (&out)[F]) {
  int32_t lo[F], hi[F];
#pragma unroll
  for (int f = 0; f < F; f++) lo[f] = 0, hi[f] = valid[f] ? deg : 0;
  for (;;) {
    bool any = false, active[F];
    int32_t mid[F], at[F];
#pragma unroll
    for (int f = 0; f < F; f++) active[f] = lo[f] < hi[f], any |= active[f], mid[f] = (lo[f] + hi[f]) >> 1;
    if (!any) break;
    // every load is issued before the first is used (a finished search reads s[0]: deg > 0 while any is active)
#pragma unroll
    for (int f = 0; f < F; f++) at[f] = s[active[f] ? mid[f] : 0];
#pragma unroll
    for (int f = 0; f < F; f++) {
      if (active[f]) {
        if (at[f] - mid[f] <= r[f]) lo[f] = mid[f] + 1;
        else hi[f] = mid[f];
      }
    }
  }
#pragma unroll
  for (int f = 0; f < F; f++) out[f] = r[f] + lo[f];
}

// The WARP search of one synchronous batch and, with GRAD, its gradient.  L lanes serve a position (the layouts of
// bpr_grad_kernel): they gather U[u] and V[i] once, then candidate rows F at a time until the first one whose
// score exceeds the positive's minus 1; the contributions are added straight from the registers that hold V[j].
// The triple (u, i, j or -1) goes to the apply kernel, the number of candidates examined to `tries`.
//   GEN  : (u, i) and the candidates are computed here from the epoch's keys (hash and binary search per
//          candidate, no candidate buffer); else (u, i) are read from users / pos and the candidates from cand.
//   GRAD : off is the search alone (irs_bpr_warp_search).
// The search loop is uniform across the wave: it runs while any group of the wave still searches, and a finished
// group (or one past the batch) stays in it with its loads predicated off.  Every shuffle therefore executes with
// all 64 lanes active, whatever the trip counts of the groups; the butterfly leaves the same bits in every lane of
// a group, so `searching` is one value per group and a group's loads, atomics and stores stay together.
// counters: positions, updates, candidates examined - one atomic per wave and counter, into one of
// WARP_COUNTER_SLOTS slots by wave number (the host adds the slots up): every wave of an epoch adding to the same
// three words made the epoch wait for those words alone (20 M positions: 15 - 30 M atomics on one address each).
template <int L, int NCH, int F, bool GEN, bool GRAD>
__global__ void __launch_bounds__(BLOCK)
warp_search_kernel(int32_t n, int32_t kp, int32_t max_sampled, Perm perm, uint64_t key, int64_t first, int32_t n_items,
                   const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                   const int32_t *__restrict__ pos_user, const int32_t *__restrict__ pos_item,
                   const int32_t *__restrict__ cand, const double *__restrict__ weights, int32_t *__restrict__ users,
                   int32_t *__restrict__ pos, int32_t *__restrict__ neg, int32_t *__restrict__ tries,
                   const float *__restrict__ U, const float *__restrict__ V, const float *__restrict__ b,
                   unsigned long long *__restrict__ accU, unsigned long long *__restrict__ accV,
                   unsigned long long *__restrict__ accb, double scale, unsigned long long *__restrict__ counters) {
  const int32_t t = static_cast<int32_t>((static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x) / L);
  const int lane = static_cast<int>(threadIdx.x) % L;
  const bool live = t < n;
  const int nchunk = kp / 4;
  int32_t u = 0, i = 0, deg = 0;
  const int32_t *row = indices;
  uint64_t position = 0;
  if (live) {
    if (GEN) {
      position = static_cast<uint64_t>(first + t);
      const uint32_t e = permute(perm, static_cast<uint32_t>(position));
      u = pos_user[e], i = pos_item[e];
      const int32_t begin = indptr[u];
      deg = indptr[u + 1] - begin, row = indices + begin;
      if (lane == 0) users[t] = u, pos[t] = i;
    } else {
      u = users[t], i = pos[t];
    }
  }
  const float4 *Ur = reinterpret_cast<const float4 *>(U + static_cast<int64_t>(u) * kp);
  const float4 *Vi = reinterpret_cast<const float4 *>(V + static_cast<int64_t>(i) * kp);
  float4 pu[NCH], pv[NCH], pj[NCH];
  double xp = 0.0;
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    const int c = lane + h * L;
    pu[h] = pv[h] = pj[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && c < nchunk) {
      pu[h] = Ur[c], pv[h] = Vi[c];
      xp += static_cast<double>(pu[h].x) * pv[h].x + static_cast<double>(pu[h].y) * pv[h].y +
            static_cast<double>(pu[h].z) * pv[h].z + static_cast<double>(pu[h].w) * pv[h].w;
    }
  }
#pragma unroll
  for (int m = L / 2; m >= 1; m >>= 1) xp += __shfl_xor(xp, m, L);  // (the same bits in every lane of the group)
  xp += live ? static_cast<double>(b[i]) : 0.0;

  bool searching = live;
  int32_t j = -1, examined = 0;
  double w = 0.0;
  for (int32_t base = 0; base < max_sampled; base += F) {
    if (!__any(searching)) break;  // (wave-uniform: no group of this wave searches any more)
    bool valid[F];
    int32_t jf[F];
#pragma unroll
    for (int f = 0; f < F; f++) valid[f] = searching && base + f < max_sampled;
    if (GEN) {
      int32_t r[F];
#pragma unroll
      for (int f = 0; f < F; f++)
        r[f] = static_cast<int32_t>(draw_rank(key, position * WARP_MAX_SAMPLED + static_cast<uint64_t>(base + f + 1),
                                              static_cast<uint32_t>(n_items - deg)));
      unseen_by_ranks<F>(row, deg, valid, r, jf);
    } else {
#pragma unroll
      for (int f = 0; f < F; f++) jf[f] = valid[f] ? cand[static_cast<int64_t>(t) * max_sampled + base + f] : 0;
    }
    float4 vf[F][NCH];
    double xn[F];
#pragma unroll
    for (int f = 0; f < F; f++) {
      const float4 *Vj = reinterpret_cast<const float4 *>(V + static_cast<int64_t>(valid[f] ? jf[f] : 0) * kp);
      xn[f] = valid[f] ? static_cast<double>(b[jf[f]]) : 0.0;
#pragma unroll
      for (int h = 0; h < NCH; h++) {
        const int c = lane + h * L;
        vf[f][h] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid[f] && c < nchunk) vf[f][h] = Vj[c];
      }
    }
#pragma unroll
    for (int f = 0; f < F; f++) {
      double x = 0.0;
#pragma unroll
      for (int h = 0; h < NCH; h++)
        x += static_cast<double>(pu[h].x) * vf[f][h].x + static_cast<double>(pu[h].y) * vf[f][h].y +
             static_cast<double>(pu[h].z) * vf[f][h].z + static_cast<double>(pu[h].w) * vf[f][h].w;
#pragma unroll
      for (int m = L / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, L);
      xn[f] += x;
    }
#pragma unroll
    for (int f = 0; f < F; f++) {  // the lowest t wins: rows loaded past it are dropped
      if (searching && valid[f]) {
        examined = base + f + 1;
        if (xn[f] > xp - 1.0) {
          searching = false;
          j = jf[f];
          w = weights[base + f];
#pragma unroll
          for (int h = 0; h < NCH; h++) pj[h] = vf[f][h];
        }
      }
    }
  }
  if (live && lane == 0) {
    neg[t] = j;
    if (tries != nullptr) tries[t] = examined;
  }
  // counters: the group's first lane carries its position
  const bool head = live && lane == 0;
  const unsigned long long n_pos = __popcll(__ballot(head)), n_upd = __popcll(__ballot(head && j >= 0));
  int32_t sum = head ? examined : 0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
  if (static_cast<int>(threadIdx.x) % 64 == 0 && n_pos != 0) {
    const unsigned wave = blockIdx.x * (BLOCK / 64) + threadIdx.x / 64;
    unsigned long long *c = counters + static_cast<size_t>(wave % WARP_COUNTER_SLOTS) * WARP_COUNTER_STRIDE;
    atomicAdd(c + 0, n_pos);
    atomicAdd(c + 1, n_upd);
    atomicAdd(c + 2, static_cast<unsigned long long>(sum));
  }
  if (!GRAD || j < 0) return;  // (no violation: no row is touched)
  unsigned long long *au = accU + static_cast<int64_t>(u) * kp;
  unsigned long long *ai = accV + static_cast<int64_t>(i) * kp;
  unsigned long long *aj = accV + static_cast<int64_t>(j) * kp;
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    const int c = lane + h * L;
    if (c >= nchunk) continue;
    const float uu[4] = {pu[h].x, pu[h].y, pu[h].z, pu[h].w};
    const double d[4] = {static_cast<double>(pv[h].x) - pj[h].x, static_cast<double>(pv[h].y) - pj[h].y,
                         static_cast<double>(pv[h].z) - pj[h].z, static_cast<double>(pv[h].w) - pj[h].w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int at = e * nchunk + c;
      add_fixed(au + at, -w * d[e], scale);
      add_fixed(ai + at, -w * uu[e], scale);
      add_fixed(aj + at, w * uu[e], scale);
    }
  }
  if (lane == 0) {
    add_fixed(accb + i, -w, scale);
    add_fixed(accb + j, w, scale);
  }
}

// bpr_apply_kernel for WARP triples: a position whose negative is -1 found no violation and claims no row.  The
// skip is a predicate on the claim, not a branch round the shuffle.  (A kernel of its own, so that the code of
// the BPR instantiations does not change.)
template <int L>
__global__ void __launch_bounds__(BLOCK)
warp_apply_kernel(int32_t n, int32_t kp, const int32_t *__restrict__ users, const int32_t *__restrict__ pos,
                  const int32_t *__restrict__ neg, unsigned long long batch_no, unsigned long long *__restrict__ stampU,
                  unsigned long long *__restrict__ stampV, float *__restrict__ U, float *__restrict__ V,
                  float *__restrict__ b, float *__restrict__ GU, float *__restrict__ GV, float *__restrict__ Gb,
                  unsigned long long *__restrict__ accU, unsigned long long *__restrict__ accV,
                  unsigned long long *__restrict__ accb, double inv_scale, float user_alpha, float item_alpha, float lr,
                  int32_t *__restrict__ diverged) {
  const int32_t t = static_cast<int32_t>((static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x) / L);
  const int lane = static_cast<int>(threadIdx.x) % L;
  if (t >= n) return;
  bool bad = false;
  const int32_t rows[3] = {users[t], pos[t], neg[t]};
  const bool updates = rows[2] >= 0;
#pragma unroll
  for (int which = 0; which < 3; which++) {
    const int64_t r = rows[which];
    int won = 0;
    if (lane == 0 && updates) won = atomicExch((which == 0 ? stampU : stampV) + r, batch_no) != batch_no;
    won = __shfl(won, 0, L);
    if (!won) continue;
    if (which == 0) {
      apply_row<L>(lane, kp, U + r * kp, GU + r * kp, accU + r * kp, inv_scale, user_alpha, lr, bad);
    } else {
      apply_row<L>(lane, kp, V + r * kp, GV + r * kp, accV + r * kp, inv_scale, item_alpha, lr, bad);
      if (lane == 0) adagrad(b[r], Gb[r], accb[r], inv_scale, item_alpha, lr, bad);
    }
  }
  if (bad) *diverged = 1;
}

}  // namespace bpr
}  // namespace irs
