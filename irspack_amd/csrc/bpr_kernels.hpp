// Kernels of the BPR trainer (bpr.hip): the sampler, the gradient of one synchronous
// batch and the Adagrad step on the rows the batch touched.
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

}  // namespace bpr
}  // namespace irs
