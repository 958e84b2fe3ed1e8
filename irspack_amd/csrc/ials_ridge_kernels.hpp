// Feature-aware iALS, the feature-weight ridge system on the device (IALSTrainer.hpp:1082-1171):
//   G = F^T D F + lambda I  (once per side: initialize_feature_weight_cache)   -> ridge_gram_*
//   G = L L^T               (once per side, kept: FeatureWeightCache.llt)      -> ridge_chol_*
//   L L^T W = F^T (D factor) (every epoch: solve_feature_weight)               -> ridge_trsv_*
// D = diag(compute_reg(nnz_r, other_size)), F the feature matrix (CSR; a dense one is a full CSR).
//
// Layout: G and L are dense row-major FP x FP with FP = F rounded up to RIDGE_NB = 64; the padded
// rows / columns of G are those of the identity, so the padded system is block diagonal and its
// leading F x F block is the reference's.  L overwrites the lower triangle of G.  The right-hand
// side / solution S is [FP, KP] (the trainer's padded latent layout, pad rows zero).
//
// Everything is fp32 (the ridge system can be ill-conditioned when lambda is small, so no bf16).
// The O(n^3) / O(n^2 K) parts - Gram tiles, trailing updates of the Cholesky, the off-diagonal
// updates of the substitutions - run on v_mfma_f32_16x16x4_f32: a 64 x 64 output tile per
// 256-thread workgroup, each wave a 32 x 32 quarter of 2 x 2 16 x 16 blocks.  MFMA operand layout
// (lane = 16 g + m): A operand A[m][g], B operand B[g][m], accumulator register r = C[4 g + r][m].
// No float atomics anywhere; every sum has a fixed order, so two runs give bit-identical results.
//
// Error bits of the trainer's flag (sync_and_check): 16 a pivot of G that is not > 0 or not finite
// (Eigen's LLT fails on x <= 0, hpp:1104-1105), 32 a non-finite solution (hpp:1169-1170).
#pragma once
#include "chol_tile_kernels.hpp"
#include "ials_kernels.hpp"

namespace irs {
namespace ials {

// (RIDGE_NB, the tile helpers ridge_tile_of / ridge_mfma_64 / ridge_acc_pos and the Cholesky kernels
// ridge_chol_{diag,trsm,update}_kernel are in chol_tile_kernels.hpp)

// G[a][b] (and G[b][a]) of tile (bi, bj) from its Gram value: + lambda on the diagonal of the
// first F rows, the identity on the padded ones
__device__ inline void ridge_store_gram(float *G, int FP, int F, int bi, int bj, int a, int b, float v,
                                        float lam) {
  const int ga = bi * RIDGE_NB + a, gb = bj * RIDGE_NB + b;
  if (ga == gb) v = ga < F ? v + lam : 1.0f;
  G[static_cast<size_t>(ga) * FP + gb] = v;
  if (bi != bj) G[static_cast<size_t>(gb) * FP + ga] = v;
}

// Gram tile (bi, bj) over the rows of slab `slab`: sum_r w_r f_r[A] f_r[B]^T.  Rows go through LDS
// 16 at a time as dense 16 x 64 slices of the two column blocks (16 threads scan a CSR row); a chunk
// in which no row stores a column of both blocks is skipped.  n_slabs == 1: the tile goes straight
// into G; else into part[slab][tile] for ridge_gram_reduce_kernel.
__global__ __launch_bounds__(256) void ridge_gram_kernel(const int32_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices,
                                                         const float *__restrict__ data,
                                                         const float *__restrict__ w, int64_t n_rows,
                                                         int64_t rows_per_slab, int n_slabs, int F, int FP,
                                                         float lam, float *__restrict__ part,
                                                         float *__restrict__ G) {
  __shared__ float sa[16][RIDGE_LD], sb[16][RIDGE_LD];
  __shared__ int hit[2];
  const int tile = blockIdx.x, slab = blockIdx.y, tid = threadIdx.x;
  int bi, bj;
  ridge_tile_of(tile, bi, bj);
  const int a0 = bi * RIDGE_NB, b0 = bj * RIDGE_NB;
  const int64_t rb = static_cast<int64_t>(slab) * rows_per_slab;
  const int64_t re = min(n_rows, rb + rows_per_slab);
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t r0 = rb; r0 < re; r0 += 16) {
    for (int e = tid; e < 16 * RIDGE_NB; e += 256) {
      sa[e >> 6][e & 63] = 0.f;
      sb[e >> 6][e & 63] = 0.f;
    }
    if (tid < 2) hit[tid] = 0;
    __syncthreads();
    const int lr = tid >> 4, l16 = tid & 15;
    const int64_t r = r0 + lr;
    int ha = 0, hb = 0;
    if (r < re) {
      const float wr = w[r];
      for (int q = indptr[r] + l16; q < indptr[r + 1]; q += 16) {
        const int c = indices[q];
        const float v = data[q];
        if (c >= a0 && c < a0 + RIDGE_NB) {
          sa[lr][c - a0] = wr * v;
          ha = 1;
        }
        if (c >= b0 && c < b0 + RIDGE_NB) {
          sb[lr][c - b0] = v;
          hb = 1;
        }
      }
    }
    if (ha) hit[0] = 1;
    if (hb) hit[1] = 1;
    __syncthreads();
    if (hit[0] && hit[1])  // (uniform over the workgroup)
      ridge_mfma_64(acc, &sa[0][0], 1, RIDGE_LD, &sb[0][0], 1, RIDGE_LD, 16);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int a, b;
        ridge_acc_pos(i, j, q, a, b);
        const float v = acc[i][j][q];
        if (n_slabs == 1) ridge_store_gram(G, FP, F, bi, bj, a, b, v, lam);
        else part[(static_cast<size_t>(slab) * gridDim.x + tile) * (RIDGE_NB * RIDGE_NB) + a * RIDGE_NB + b] = v;
      }
}

// the slabs of every tile added in slab order, then into G like ridge_gram_kernel's direct store
__global__ void ridge_gram_reduce_kernel(const float *__restrict__ part, int n_tiles, int n_slabs, int F,
                                         int FP, float lam, float *__restrict__ G) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t per = static_cast<int64_t>(n_tiles) * RIDGE_NB * RIDGE_NB;
  if (i >= per) return;
  float s = 0.f;
  for (int c = 0; c < n_slabs; c++) s += part[static_cast<size_t>(c) * per + i];
  const int tile = static_cast<int>(i / (RIDGE_NB * RIDGE_NB)), e = static_cast<int>(i % (RIDGE_NB * RIDGE_NB));
  int bi, bj;
  ridge_tile_of(tile, bi, bj);
  ridge_store_gram(G, FP, F, bi, bj, e / RIDGE_NB, e % RIDGE_NB, s, lam);
}


// ---------------------------------------------------------------- L L^T X = S, in place
// Columns are independent: blockIdx.y (or .x) takes 64 of the KP latent columns.
// (1) forward, diagonal tile k: y = L_kk^-1 s; one thread per column
__global__ __launch_bounds__(64) void ridge_trsv_fwd_diag_kernel(const float *__restrict__ L, int FP, int k,
                                                                 float *__restrict__ S, int KP) {
  __shared__ float l[RIDGE_NB][RIDGE_LD];
  const int tid = threadIdx.x, o = k * RIDGE_NB, col = blockIdx.x * RIDGE_NB + tid;
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 64)
    l[e >> 6][e & 63] = L[static_cast<size_t>(o + (e >> 6)) * FP + o + (e & 63)];
  __syncthreads();
  if (col >= KP) return;  // (KP = 16 / 32)
  float x[RIDGE_NB];
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) x[j] = S[static_cast<size_t>(o + j) * KP + col];
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) {
    float v = x[j];
#pragma unroll
    for (int m = 0; m < j; m++) v = fmaf(-l[j][m], x[m], v);
    x[j] = v / l[j][j];
  }
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) S[static_cast<size_t>(o + j) * KP + col] = x[j];
}

// (2) backward, diagonal tile k: x = L_kk^-T y; one thread per column
__global__ __launch_bounds__(64) void ridge_trsv_bwd_diag_kernel(const float *__restrict__ L, int FP, int k,
                                                                 float *__restrict__ S, int KP,
                                                                 int32_t *__restrict__ err_flag) {
  __shared__ float l[RIDGE_NB][RIDGE_LD];
  const int tid = threadIdx.x, o = k * RIDGE_NB, col = blockIdx.x * RIDGE_NB + tid;
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 64)
    l[e >> 6][e & 63] = L[static_cast<size_t>(o + (e >> 6)) * FP + o + (e & 63)];
  __syncthreads();
  if (col >= KP) return;  // (KP = 16 / 32)
  float x[RIDGE_NB];
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) x[j] = S[static_cast<size_t>(o + j) * KP + col];
  bool fin = true;
#pragma unroll
  for (int j = RIDGE_NB - 1; j >= 0; j--) {
    float v = x[j];
#pragma unroll
    for (int m = j + 1; m < RIDGE_NB; m++) v = fmaf(-l[m][j], x[m], v);
    x[j] = v / l[j][j];
    fin = fin && isfinite(x[j]);
  }
#pragma unroll
  for (int j = 0; j < RIDGE_NB; j++) S[static_cast<size_t>(o + j) * KP + col] = x[j];
  if (!fin) atomicOr(err_flag, RIDGE_FLAG_SOLVE);
}

// (3) the other row blocks.  Forward (bwd == 0): S[i] -= L[i][k] S[k] for the blocks i > k
// (blockIdx.x = i - k - 1).  Backward: S[i] -= L[k][i]^T S[k] for the blocks i < k (blockIdx.x = i).
__global__ __launch_bounds__(256) void ridge_trsv_update_kernel(const float *__restrict__ L, int FP, int k,
                                                                int bwd, float *__restrict__ S, int KP) {
  __shared__ float lt[RIDGE_NB][RIDGE_LD], xs[RIDGE_NB][RIDGE_LD];
  const int tid = threadIdx.x, o = k * RIDGE_NB, c0 = blockIdx.y * RIDGE_NB;
  const int bi = bwd ? blockIdx.x : k + 1 + blockIdx.x, oi = bi * RIDGE_NB;
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 256) {
    const int a = e >> 6, b = e & 63;
    // lt[a][c]: the coefficient of S[k-block row c] in the update of S[i-block row a]
    if (bwd) lt[b][a] = L[static_cast<size_t>(o + a) * FP + oi + b];
    else lt[a][b] = L[static_cast<size_t>(oi + a) * FP + o + b];
    xs[a][b] = c0 + b < KP ? S[static_cast<size_t>(o + a) * KP + c0 + b] : 0.f;
  }
  __syncthreads();
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  ridge_mfma_64(acc, &lt[0][0], RIDGE_LD, 1, &xs[0][0], 1, RIDGE_LD, RIDGE_NB);
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int a, b;
        ridge_acc_pos(i, j, q, a, b);
        if (c0 + b < KP) {
          float *p = S + static_cast<size_t>(oi + a) * KP + c0 + b;
          *p = *p - acc[i][j][q];
        }
      }
}

// W[f, :] = S[f, :] for the first F rows - only when nothing this call raised the flag (the
// reference leaves the weights as they were when it throws)
__global__ void ridge_commit_kernel(const float *__restrict__ S, int64_t n, const int32_t *__restrict__ err_flag,
                                    float *__restrict__ W) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n || *err_flag != 0) return;
  W[i] = S[i];
}

}  // namespace ials
}  // namespace irs
