// The generic pieces of the blocked fp32 MFMA Cholesky (shared by the feature-aware iALS ridge system,
// ials_ridge_kernels.hpp, and the EASE / EDLAE item-Gram inverse, dense_slim.hip): a dense row-major
// n_pad x n_pad matrix, n_pad a multiple of RIDGE_NB = 64, 64 x 64 tiles, one 256-thread workgroup per
// tile, each wave a 32 x 32 quarter of 2 x 2 16 x 16 blocks of v_mfma_f32_16x16x4_f32.  MFMA operand
// layout (lane = 16 g + m): A operand A[m][g], B operand B[g][m], accumulator register r = C[4 g + r][m].
// No float atomics; every sum has a fixed order.  The kernels are static: two translation units of one
// library include this header.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace irs {
namespace ials {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RIDGE_NB = 64;
constexpr int RIDGE_LD = RIDGE_NB + 1;  // LDS row stride of a 64 x 64 tile (no bank conflicts)
constexpr int RIDGE_FLAG_CHOL = 16, RIDGE_FLAG_SOLVE = 32;

// (bi, bj), bi >= bj, of lower-triangle tile t (row-major order of the tiles)
__device__ inline void ridge_tile_of(int t, int &bi, int &bj) {
  int i = static_cast<int>((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > t) i--;
  while ((i + 1) * (i + 2) / 2 <= t) i++;
  bi = i;
  bj = t - i * (i + 1) / 2;
}

// acc[i][j] += A_tile(32 w_r rows) * B_tile(32 w_c cols) over 64 inner indices held in LDS:
//   A(a, c) = a_lds[a * lda_a + c * lda_c], B(c, b) = b_lds[b * ldb_b + c * ldb_c]
__device__ inline void ridge_mfma_64(f32x4 (&acc)[2][2], const float *a_lds, int lda_a, int lda_c,
                                     const float *b_lds, int ldb_b, int ldb_c, int inner) {
  const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15, wv = threadIdx.x >> 6;
  const int ar = 32 * (wv >> 1), bc = 32 * (wv & 1);
  for (int s = 0; s < inner; s += 4) {
    const int c = s + g;
    float av[2], bv[2];
#pragma unroll
    for (int i = 0; i < 2; i++) av[i] = a_lds[(ar + 16 * i + m) * lda_a + c * lda_c];
#pragma unroll
    for (int j = 0; j < 2; j++) bv[j] = b_lds[(bc + 16 * j + m) * ldb_b + c * ldb_c];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
  }
}

// element (a, b) of the 64 x 64 tile that register r of acc[i][j] holds in this lane
__device__ inline void ridge_acc_pos(int i, int j, int r, int &a, int &b) {
  const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15, wv = threadIdx.x >> 6;
  a = 32 * (wv >> 1) + 16 * i + 4 * g + r;
  b = 32 * (wv & 1) + 16 * j + m;
}

// ---------------------------------------------------------------- Cholesky G = L L^T (right-looking)
// (1) the diagonal tile k in LDS, unblocked: pivot, column scale, rank-1 update of the rest
static __global__ __launch_bounds__(256) void ridge_chol_diag_kernel(float *__restrict__ G, int FP, int k,
                                                              int32_t *__restrict__ err_flag) {
  __shared__ float s[RIDGE_NB][RIDGE_LD];
  const int tid = threadIdx.x, o = k * RIDGE_NB;
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 256)
    s[e >> 6][e & 63] = G[static_cast<size_t>(o + (e >> 6)) * FP + o + (e & 63)];
  __syncthreads();
  for (int j = 0; j < RIDGE_NB; j++) {
    const float d = s[j][j];
    if (tid == 0 && (!(d > 0.f) || !isfinite(d))) atomicOr(err_flag, RIDGE_FLAG_CHOL);
    const float l = sqrtf(d);
    __syncthreads();
    if (tid > j && tid < RIDGE_NB) s[tid][j] /= l;
    if (tid == j) s[j][j] = l;
    __syncthreads();
    for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 256) {
      const int a = e >> 6, b = e & 63;
      if (b > j && a >= b) s[a][b] = fmaf(-s[a][j], s[b][j], s[a][b]);
    }
    __syncthreads();
  }
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 256) {
    const int a = e >> 6, b = e & 63;
    G[static_cast<size_t>(o + a) * FP + o + b] = b <= a ? s[a][b] : 0.f;
  }
}

// (2) the panel below it: L[r, k-block] = G[r, k-block] L_kk^-T, one thread per row r
static __global__ __launch_bounds__(256) void ridge_chol_trsm_kernel(float *__restrict__ G, int FP, int k) {
  __shared__ float s[RIDGE_NB][RIDGE_LD];
  const int tid = threadIdx.x, o = k * RIDGE_NB;
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 256)
    s[e >> 6][e & 63] = G[static_cast<size_t>(o + (e >> 6)) * FP + o + (e & 63)];
  __syncthreads();
  const int r = o + RIDGE_NB + blockIdx.x * 256 + tid;
  if (r >= FP) return;
  float *row = G + static_cast<size_t>(r) * FP + o;
  float x[RIDGE_NB];
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) x[j] = row[j];
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) {
    float v = x[j];
#pragma unroll
    for (int m = 0; m < j; m++) v = fmaf(-x[m], s[j][m], v);
    x[j] = v / s[j][j];
  }
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) row[j] = x[j];
}

// (3) the trailing lower triangle: G[bi][bj] -= L[bi][k] L[bj][k]^T for k < bj <= bi
static __global__ __launch_bounds__(256) void ridge_chol_update_kernel(float *__restrict__ G, int FP, int k) {
  __shared__ float la[RIDGE_NB][RIDGE_LD], lb[RIDGE_NB][RIDGE_LD];
  const int tid = threadIdx.x, o = k * RIDGE_NB;
  int ti, tj;
  ridge_tile_of(blockIdx.x, ti, tj);
  const int bi = k + 1 + ti, bj = k + 1 + tj;
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 256) {
    la[e >> 6][e & 63] = G[static_cast<size_t>(bi * RIDGE_NB + (e >> 6)) * FP + o + (e & 63)];
    lb[e >> 6][e & 63] = G[static_cast<size_t>(bj * RIDGE_NB + (e >> 6)) * FP + o + (e & 63)];
  }
  __syncthreads();
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  ridge_mfma_64(acc, &la[0][0], RIDGE_LD, 1, &lb[0][0], RIDGE_LD, 1, RIDGE_NB);
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int a, b;
        ridge_acc_pos(i, j, q, a, b);
        float *p = G + static_cast<size_t>(bi * RIDGE_NB + a) * FP + bj * RIDGE_NB + b;
        *p = *p - acc[i][j][q];
      }
}

}  // namespace ials
}  // namespace irs
