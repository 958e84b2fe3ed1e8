// Device kernels of the NMF fit (nmf.hip): the row-wise coordinate sweep of sklearn's
// `cd` solver, the reduction of its violation sum, and the truncated SVD's sparse x block product and Gram reduce
// (truncsvd_kernels.hpp) with their sums kept in double, on the same padded row-major blocks: row stride ld, a
// multiple of 64, the columns past k are zero and stay zero.  No float atomics; every sum has a fixed order: two calls give
// identical bytes.
#pragma once
#include "chol_tile_kernels.hpp"
#include "common.hpp"

namespace irs {
namespace nmf {

constexpr int SWEEP_ROWS = 64;  // rows of a workgroup: one wave, one lane per row
constexpr int SWEEP_CB = 16;    // coordinates resolved together
constexpr int SWEEP_CHUNK = 64; // coordinates of a dot product added in one chain (a multiple of SWEEP_CB)

// G[t, t] += l2 for t < k: the tiny prologue of a sweep (the padded diagonal stays zero)
static __global__ __launch_bounds__(64) void nmf_ridge_kernel(float *__restrict__ G, int k, int ld, float l2) {
  const int t = static_cast<int>(blockIdx.x) * 64 + static_cast<int>(threadIdx.x);
  if (t < k) G[static_cast<size_t>(t) * ld + t] += l2;
}

// One half-step's sweep: for every row i of W (n x ld) and t = 0 .. k-1 ascending
//     grad = sum_r G[t, r] W[i, r] - (XH[i, t] - l1);  violation += W[i, t] == 0 ? |min(0, grad)| : |grad|;
//     if G[t, t] != 0: W[i, t] = max(W[i, t] - grad / G[t, t], 0)
// exact Gauss-Seidel.  One lane per row, the coordinates in blocks of SWEEP_CB.  For a block the lane keeps
// g[j] = -(XH[i, t_j] - l1) + sum over the r outside the block of G[t_j, r] W[i, r] in registers: the r loop
// reads the lane's own row of W (a float4 at a time; blocks before this one hold this sweep's values already,
// written by this same lane) against G[r, t_0 .. t_0 + 15] - G is symmetric to the bit, so row r holds the 16
// factors side by side, and the address is the same in every lane: a uniform load of 16 values per 16 fused
// multiply-adds on 64 rows.  The r loop goes in chunks of SWEEP_CHUNK coordinates, each summed from zero and then
// added to g: one chain over all k terms is, at k = 257, four times as far from float64 as a BLAS dot product
// is (which adds in blocks too), the chunked sum no farther.  The block itself is resolved against its 16 x 16 diagonal block of G with the 16
// values of W in registers.  The violation is added per row in coordinate order in double, the rows of the
// workgroup in ascending order by lane 0, to partial[blockIdx.x].
static __global__ __launch_bounds__(SWEEP_ROWS) void nmf_sweep_kernel(float *W, const float *__restrict__ XH,
                                                                      const float *__restrict__ G, int n, int k,
                                                                      int ld, float l1, double *__restrict__ partial) {
  __shared__ double row_violation[SWEEP_ROWS];
  const int lane = static_cast<int>(threadIdx.x);
  const int i = static_cast<int>(blockIdx.x) * SWEEP_ROWS + lane;
  const bool live = i < n;
  // a lane past the last row works on a copy of row n - 1 and writes nothing
  const size_t row = static_cast<size_t>(live ? i : n - 1) * ld;
  float *w_row = W + row;
  const float *xh_row = XH + row;
  const int k4 = (k + 3) & ~3;
  double violation = 0.0;
  for (int t0 = 0; t0 < k; t0 += SWEEP_CB) {
    float g[SWEEP_CB], w[SWEEP_CB];
#pragma unroll
    for (int q = 0; q < SWEEP_CB / 4; q++) {
      const float4 x = *reinterpret_cast<const float4 *>(xh_row + t0 + 4 * q);
      const float4 v = *reinterpret_cast<const float4 *>(w_row + t0 + 4 * q);
      g[4 * q + 0] = -(x.x - l1), g[4 * q + 1] = -(x.y - l1), g[4 * q + 2] = -(x.z - l1), g[4 * q + 3] = -(x.w - l1);
      w[4 * q + 0] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
    for (int c0 = 0; c0 < k4; c0 += SWEEP_CHUNK) {
      const int c1 = min(k4, c0 + SWEEP_CHUNK);
      float h[SWEEP_CB];
#pragma unroll
      for (int j = 0; j < SWEEP_CB; j++) h[j] = 0.f;
      for (int r0 = c0; r0 < c1; r0 += 4) {
        if (r0 >= t0 && r0 < t0 + SWEEP_CB) continue;  // (uniform: the block's own coordinates come below)
        const float4 v = *reinterpret_cast<const float4 *>(w_row + r0);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const float *g_row = G + static_cast<size_t>(r0 + u) * ld + t0;
#pragma unroll
          for (int j = 0; j < SWEEP_CB; j++) h[j] = fmaf(g_row[j], vv[u], h[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < SWEEP_CB; j++) g[j] += h[j];
    }
#pragma unroll
    for (int j = 0; j < SWEEP_CB; j++) {
      const int t = t0 + j;
      if (t < k) {  // (uniform)
        const float *g_row = G + static_cast<size_t>(t) * ld + t0;
        float grad = g[j];
#pragma unroll
        for (int r = 0; r < SWEEP_CB; r++) grad = fmaf(g_row[r], w[r], grad);
        const float pg = w[j] == 0.f ? fminf(grad, 0.f) : grad;
        violation += static_cast<double>(fabsf(pg));
        const float hess = g_row[j];
        if (hess != 0.f) w[j] = fmaxf(w[j] - grad / hess, 0.f);
      }
    }
    if (live) {
#pragma unroll
      for (int q = 0; q < SWEEP_CB / 4; q++)
        *reinterpret_cast<float4 *>(w_row + t0 + 4 * q) = make_float4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
  }
  row_violation[lane] = live ? violation : 0.0;
  __syncthreads();
  if (lane == 0) {
    double v = 0.0;
    for (int r = 0; r < SWEEP_ROWS; r++) v += row_violation[r];
    partial[blockIdx.x] = v;
  }
}

// ---------------------------------------------------------------------------------------------- SpMM, Gram
// tsvd_spmm_kernel with the sums of a row kept in double (a float x float product is exact in double) and
// rounded to float32 once, at the store: same segments, same lane layout, same order.  With a small `alpha` the
// fit amplifies the rounding of XH and G by four orders of magnitude, and a float32 sum over a row
// of 100 entries is ten roundings where the stored value allows one.
// TP: the type of a split row's partial sums.  float (the fit): every segment is rounded, then the segments are added
// in float (tsvd_spmm_reduce_kernel).  double (the truncated SVD's fold-in, irs_truncsvd_transform): the segments'
// sums stay in double and nmf_spmm_reduce_f64_kernel rounds their sum - every row, split or not, is rounded once.
template <int LPR, int NCH, class TP = float>
static __global__ __launch_bounds__(256) void nmf_spmm_kernel(const int32_t *__restrict__ seg_row,
                                                              const int32_t *__restrict__ seg_begin,
                                                              const int32_t *__restrict__ seg_end,
                                                              const int32_t *__restrict__ seg_slot, int n_seg,
                                                              const int32_t *__restrict__ idx,
                                                              const float *__restrict__ val,
                                                              const float *__restrict__ Q, int l_pad,
                                                              float *__restrict__ Y, TP *__restrict__ partial) {
  constexpr int G = 64 / LPR;
  const int s = static_cast<int>(blockIdx.x) * 4 + wave_index_in_block();
  if (s >= n_seg) return;
  const int lane = static_cast<int>(threadIdx.x & 63);
  const int sub = lane / LPR, col = lane % LPR;
  const int lvec = l_pad >> 2;
  const int row = seg_row[s], beg = seg_begin[s], end = seg_end[s], slot = seg_slot[s];
  const float4 *Q4 = reinterpret_cast<const float4 *>(Q);
  bool on[NCH];
  double acc[NCH][4];
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    on[c] = col + 64 * c < lvec;
    acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.0;
  }
  for (int p = beg; p < end; p += 64) {
    const int cnt = min(64, end - p);
    int my_i = 0;
    float my_v = 0.f;
    if (lane < cnt) {
      my_i = idx[p + lane];
      my_v = val[p + lane];
    }
    for (int e = 0; e < cnt; e += 4 * G) {
      float vv[4];
      float4 q[4][NCH];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        // e is a multiple of 4 G below 64, so j <= 63; an entry past the end of the block is (row 0,
        // value 0): a finite row times zero
        const int j = e + u * G + sub;
        const int ii = __shfl(my_i, j);
        vv[u] = __shfl(my_v, j);
        const float4 *src = Q4 + static_cast<size_t>(ii) * lvec + col;
#pragma unroll
        for (int c = 0; c < NCH; c++)
          if (on[c]) q[u][c] = src[64 * c];
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int c = 0; c < NCH; c++)
          if (on[c]) {
            const double v = static_cast<double>(vv[u]);
            acc[c][0] = fma(v, static_cast<double>(q[u][c].x), acc[c][0]);
            acc[c][1] = fma(v, static_cast<double>(q[u][c].y), acc[c][1]);
            acc[c][2] = fma(v, static_cast<double>(q[u][c].z), acc[c][2]);
            acc[c][3] = fma(v, static_cast<double>(q[u][c].w), acc[c][3]);
          }
    }
  }
  if (G > 1) {
#pragma unroll
    for (int off = 32; off >= LPR; off >>= 1)
#pragma unroll
      for (int x = 0; x < 4; x++) acc[0][x] += __shfl_down(acc[0][x], off);
  }
  if constexpr (sizeof(TP) == 8) {
    if (slot >= 0) {  // (wave-uniform) a segment of a split row: its sums as they are
      double *dst = partial + static_cast<size_t>(slot) * l_pad;
      if (sub == 0) {
#pragma unroll
        for (int c = 0; c < NCH; c++)
          if (on[c]) {
#pragma unroll
            for (int x = 0; x < 4; x++) dst[4 * (col + 64 * c) + x] = acc[c][x];
          }
      }
      return;
    }
  }
  float4 *dst = reinterpret_cast<float4 *>(
      slot < 0 ? Y + static_cast<size_t>(row) * l_pad
               : reinterpret_cast<float *>(partial) + static_cast<size_t>(slot) * l_pad);
  if (sub == 0) {
#pragma unroll
    for (int c = 0; c < NCH; c++)
      if (on[c])
        dst[col + 64 * c] = make_float4(static_cast<float>(acc[c][0]), static_cast<float>(acc[c][1]),
                                        static_cast<float>(acc[c][2]), static_cast<float>(acc[c][3]));
  }
}

// Y[row, :] of split row blockIdx.x = its segments' double partial rows added in segment order, rounded to float32
// once (tsvd_spmm_reduce_kernel for nmf_spmm_kernel<.., .., double>)
static __global__ __launch_bounds__(256) void nmf_spmm_reduce_f64_kernel(const int32_t *__restrict__ split_row,
                                                                         const int32_t *__restrict__ split_first,
                                                                         const int32_t *__restrict__ split_count,
                                                                         const double *__restrict__ partial, int l_pad,
                                                                         float *__restrict__ Y) {
  const int r = blockIdx.x;
  const int row = split_row[r], first = split_first[r], count = split_count[r];
  for (int c = threadIdx.x; c < l_pad; c += 256) {
    double v = partial[static_cast<size_t>(first) * l_pad + c];
    for (int k = 1; k < count; k++) v += partial[static_cast<size_t>(first + k) * l_pad + c];
    Y[static_cast<size_t>(row) * l_pad + c] = static_cast<float>(v);
  }
}

// tsvd_gram_reduce_kernel with the slab partials added in double (slab order), rounded to float32 once
static __global__ __launch_bounds__(256) void nmf_gram_reduce_kernel(const float *__restrict__ P, int n_slab,
                                                                     int n_tile, int ld, float *__restrict__ G) {
  int bi, bj;
  ials::ridge_tile_of(blockIdx.x, bi, bj);
  const int e = static_cast<int>(blockIdx.y) * 256 + static_cast<int>(threadIdx.x);
  const int a = e >> 6, b = e & 63;
  if (bi == bj && b > a) return;
  double v = 0.0;
  for (int s = 0; s < n_slab; s++)
    v += static_cast<double>(P[(static_cast<size_t>(s) * n_tile + blockIdx.x) * (ials::RIDGE_NB * ials::RIDGE_NB) + e]);
  const int i = bi * ials::RIDGE_NB + a, j = bj * ials::RIDGE_NB + b;
  G[static_cast<size_t>(i) * ld + j] = static_cast<float>(v);
  G[static_cast<size_t>(j) * ld + i] = static_cast<float>(v);
}

// out[0] = the sum of partial[0 .. count): thread j adds the entries j, j + 256, ... in ascending order, thread 0
// the 256 sums in thread order
static __global__ __launch_bounds__(256) void nmf_violation_kernel(const double *__restrict__ partial, int count,
                                                                   double *__restrict__ out) {
  __shared__ double sums[256];
  double v = 0.0;
  for (int p = threadIdx.x; p < count; p += 256) v += partial[p];
  sums[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int j = 0; j < 256; j++) total += sums[j];
    out[0] = total;
  }
}

}  // namespace nmf
}  // namespace irs
