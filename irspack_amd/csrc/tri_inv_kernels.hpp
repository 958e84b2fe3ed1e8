// The inverse of a lower-triangular factor in 64 x 64 tiles, M = L^-1 (shared by the EASE / EDLAE item-Gram
// inverse, dense_slim.hip, and the block normalisation of the truncated SVD, truncsvd.hip): the diagonal
// tiles inverted in LDS, then block forward substitution of L M = I restricted to the lower triangle - step k:
// M[k][j] = M[k][k] R[k][j] (j < k), R[i][j] -= L[i][k] M[k][j] (i > k >= j), R and M sharing one zeroed
// workspace.  Tiles above the diagonal are never touched.  The kernels are static: two translation units
// of one library include this header.
#pragma once
#include "chol_tile_kernels.hpp"

namespace irs {
namespace dslim {

using ials::f32x4;
using ials::RIDGE_LD;
using ials::RIDGE_NB;
using ials::ridge_acc_pos;
using ials::ridge_mfma_64;
using ials::ridge_tile_of;

// M[k][k] = L[k][k]^-1 for every diagonal tile k = blockIdx.x: thread t solves L_kk x = e_t (one column
// of the inverse; the entries above the diagonal come out as exact zeros), the tile goes out through LDS
static __global__ __launch_bounds__(64) void dslim_diag_inv_kernel(const float *__restrict__ L, int n_pad,
                                                                   float *__restrict__ M) {
  __shared__ float l[RIDGE_NB][RIDGE_LD];
  const int tid = threadIdx.x, o = blockIdx.x * RIDGE_NB;
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 64)
    l[e >> 6][e & 63] = L[static_cast<size_t>(o + (e >> 6)) * n_pad + o + (e & 63)];
  __syncthreads();
  float x[RIDGE_NB];
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) {
    float v = j == tid ? 1.0f : 0.0f;
#pragma unroll
    for (int m = 0; m < j; m++) v = fmaf(-l[j][m], x[m], v);
    x[j] = v / l[j][j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) l[j][tid] = j >= tid ? x[j] : 0.0f;
  __syncthreads();
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 64)
    M[static_cast<size_t>(o + (e >> 6)) * n_pad + o + (e & 63)] = l[e >> 6][e & 63];
}

__device__ inline void zero_acc(f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// 64 x 64 tile at (r0, c0) of a row-major matrix with stride ld into LDS, coalesced
__device__ inline void load_tile(float (&s)[RIDGE_NB][RIDGE_LD], const float *__restrict__ A, int ld, int r0,
                                 int c0) {
  for (int e = threadIdx.x; e < RIDGE_NB * RIDGE_NB; e += 256)
    s[e >> 6][e & 63] = A[static_cast<size_t>(r0 + (e >> 6)) * ld + c0 + (e & 63)];
}

// step k of the substitution, row k: M[k][j] = M[k][k] R[k][j] in place for the tiles j = blockIdx.x < k
static __global__ __launch_bounds__(256) void dslim_inv_row_kernel(float *__restrict__ M, int n_pad, int k) {
  __shared__ float d[RIDGE_NB][RIDGE_LD], r[RIDGE_NB][RIDGE_LD];
  const int o = k * RIDGE_NB, oj = blockIdx.x * RIDGE_NB;
  load_tile(d, M, n_pad, o, o);
  load_tile(r, M, n_pad, o, oj);
  __syncthreads();
  f32x4 acc[2][2];
  zero_acc(acc);
  ridge_mfma_64(acc, &d[0][0], RIDGE_LD, 1, &r[0][0], 1, RIDGE_LD, RIDGE_NB);
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int a, b;
        ridge_acc_pos(i, j, q, a, b);
        M[static_cast<size_t>(o + a) * n_pad + oj + b] = acc[i][j][q];
      }
}

// step k, the rows below: R[i][j] -= L[i][k] M[k][j] for i = k + 1 + blockIdx.x, j = blockIdx.y <= k
static __global__ __launch_bounds__(256) void dslim_inv_update_kernel(const float *__restrict__ L,
                                                                      float *__restrict__ M, int n_pad, int k) {
  __shared__ float l[RIDGE_NB][RIDGE_LD], m[RIDGE_NB][RIDGE_LD];
  const int o = k * RIDGE_NB, oi = (k + 1 + blockIdx.x) * RIDGE_NB, oj = blockIdx.y * RIDGE_NB;
  load_tile(l, L, n_pad, oi, o);
  load_tile(m, M, n_pad, o, oj);
  __syncthreads();
  f32x4 acc[2][2];
  zero_acc(acc);
  ridge_mfma_64(acc, &l[0][0], RIDGE_LD, 1, &m[0][0], 1, RIDGE_LD, RIDGE_NB);
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int a, b;
        ridge_acc_pos(i, j, q, a, b);
        float *p = M + static_cast<size_t>(oi + a) * n_pad + oj + b;
        *p = *p - acc[i][j][q];
      }
}

}  // namespace dslim
}  // namespace irs
