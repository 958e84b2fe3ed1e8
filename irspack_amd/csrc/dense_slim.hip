// EASE (DenseSLIMRecommender, dense_slim.py:39-53) and EDLAE (edlae.py:49-66): W from the inverse of the
// regularised item Gram matrix, fp32 on the device.  DESIGN.md section 10 has the design and the figures.
//
//   G = X^T X                 gram_rows_kernel (gram_setup.hpp) into a zeroed n_pad x n_pad matrix A
//   P = G + diag(lam)         dslim_add_diag_kernel; the padded rows / columns are the identity's, so the
//                             padded matrix is block diagonal and its leading block is the reference's
//   P = L L^T                 ridge_chol_{diag,trsm,update}_kernel (chol_tile_kernels.hpp), L over A's lower
//   M = L^-1                  (tri_inv_kernels.hpp) into the workspace Wk (zeroed): the diagonal tiles
//                             inverted in LDS, then block
//                             forward substitution of L M = I restricted to the lower triangle - step k:
//                             M[k][j] = M[k][k] R[k][j] (j < k), R[i][j] -= L[i][k] M[k][j] (i > k >= j),
//                             R and M sharing Wk.  Tiles above the diagonal are never touched.
//   B = M^T M (lower)         tile (i, j), i >= j: sum over k >= i of M[k][i]^T M[k][j], accumulated in
//                             registers in descending row order (small terms first); B over A (L is no longer needed)
//   W                         W[i][j] = i == j ? 0 : -B[max(i,j)][min(i,j)] / B[j][j], n x n without padding,
//                             into Wk (M is no longer needed), then one copy to the caller's array
//
// 64 x 64 tiles, one 256-thread workgroup per tile, every off-diagonal product on v_mfma_f32_16x16x4_f32
// through ridge_mfma_64.  No float atomics; every sum has a fixed order: two calls give identical bytes.
#include <cmath>

#include "common.hpp"
#include "csr_checks.hpp"
#include "gram_setup.hpp"
#include "phase_spans.hpp"
#include "tile_solver_calls.hpp"

namespace irs {
namespace dslim {

struct NotPositiveDefinite : std::runtime_error {
  using std::runtime_error::runtime_error;
};

static std::string not_pd_message(int64_t col) {
  return "EASE: X^T X + diag(lam) is not positive definite (the pivot of column " + std::to_string(col) +
         " is not > 0 or not finite; an item without interactions needs reg > 0).";
}

// P_jj = G_jj + lam_j, lam_j = diag_scale * G_jj + reg: three float32 roundings, no contraction (numpy
// evaluates `scale * diag + reg`, then `+=`); the padded diagonal is 1
__global__ void dslim_add_diag_kernel(float *__restrict__ A, int n, int n_pad, float reg, float diag_scale) {
  const int j = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= n_pad) return;
  float *p = A + static_cast<size_t>(j) * n_pad + j;
  if (j < n) {
    const float g = *p;
    *p = __fadd_rn(g, __fadd_rn(__fmul_rn(diag_scale, g), reg));
  } else {
    *p = 1.0f;
  }
}

// B[i][j] = sum over k >= i of M[k][i]^T M[k][j] for the lower tile (i, j) = ridge_tile_of(blockIdx.x)
// (row-major tile order: the longest sums start first)
__global__ __launch_bounds__(256) void dslim_mtm_kernel(const float *__restrict__ M, int n_pad,
                                                        float *__restrict__ B) {
  __shared__ float ma[RIDGE_NB][RIDGE_LD], mb[RIDGE_NB][RIDGE_LD];
  int bi, bj;
  ridge_tile_of(blockIdx.x, bi, bj);
  const int nb = n_pad / RIDGE_NB, oi = bi * RIDGE_NB, oj = bj * RIDGE_NB;
  f32x4 acc[2][2];
  zero_acc(acc);
  // descending row index (tiles from the last one, rows of a tile from the last one): a diagonally dominant
  // P puts almost all of B[j][j] into the one term M[j][j]^2, and a chain that starts with it drops every
  // later, smaller term below half an ulp - their sum is 1e-5 of the total at reg = 1e4; small terms first
  for (int k = nb - 1; k >= bi; k--) {
    load_tile(ma, M, n_pad, k * RIDGE_NB, oi);
    load_tile(mb, M, n_pad, k * RIDGE_NB, oj);
    __syncthreads();
    // A(a, c) = M[k][i](63 - c, a), B(c, b) = M[k][j](63 - c, b)
    ridge_mfma_64(acc, &ma[RIDGE_NB - 1][0], 1, -RIDGE_LD, &mb[RIDGE_NB - 1][0], 1, -RIDGE_LD, RIDGE_NB);
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
        B[static_cast<size_t>(oi + a) * n_pad + oj + b] = acc[i][j][q];
      }
}

// W tile (blockIdx.y, blockIdx.x) from the lower triangle of B; rows of 64 floats go out coalesced
__global__ __launch_bounds__(256) void dslim_finalize_kernel(const float *__restrict__ B, int n_pad, int n,
                                                             float *__restrict__ W) {
  __shared__ float s[RIDGE_NB][RIDGE_LD];
  __shared__ float dd[RIDGE_NB];
  const int ti = blockIdx.y, tj = blockIdx.x, tid = threadIdx.x;
  const int oi = ti * RIDGE_NB, oj = tj * RIDGE_NB;
  if (ti >= tj) load_tile(s, B, n_pad, oi, oj);
  else load_tile(s, B, n_pad, oj, oi);
  if (tid < RIDGE_NB) dd[tid] = B[static_cast<size_t>(oj + tid) * n_pad + oj + tid];
  __syncthreads();
  for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 256) {
    const int a = e >> 6, b = e & 63, i = oi + a, j = oj + b;
    if (i >= n || j >= n) continue;
    const float v = ti > tj ? s[a][b] : ti < tj ? s[b][a] : (a >= b ? s[a][b] : s[b][a]);
    W[static_cast<size_t>(i) * n + j] = i == j ? 0.0f : -v / dd[b];
  }
}

static void fit(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices, const float *data,
                float reg, float diag_scale, int device, float *W, irs_dense_slim_stats *stats) {
  const int64_t nnz = indptr[rows];
  const int64_t n_pad = ceil_div(cols, RIDGE_NB) * RIDGE_NB, nb = n_pad / RIDGE_NB;
  if (stats) *stats = irs_dense_slim_stats{0.0, 0.0, 0.0, 0.0, 0.0, n_pad};
  if (cols == 0) return;
  if (nnz == 0) {
    // G = 0, P = reg I: B = I / reg and every off-diagonal entry of W is 0
    if (!(reg > 0.f) || !std::isfinite(reg)) throw NotPositiveDefinite(not_pd_message(0));
    std::fill(W, W + static_cast<size_t>(cols) * static_cast<size_t>(cols), 0.0f);
    return;
  }
  check_arg(nb * (nb + 1) / 2 < (int64_t{1} << 31) && nb < 65536, "too many items for the dense inverse.");
  require_device(device);
  hipStream_t s = nullptr;
  const int n = static_cast<int>(cols), np = static_cast<int>(n_pad);
  const size_t NP2 = static_cast<size_t>(n_pad) * static_cast<size_t>(n_pad);

  // memory: the matrix and the workspace of the inverse (4 n_pad^2 bytes each), X by rows and by columns
  size_t free_b = 0, total_b = 0;
  IRS_HIP(hipMemGetInfo(&free_b, &total_b));
  const double need = 8.0 * double(NP2) + 16.0 * double(nnz) * 2.0 + 64.0 * double(cols) + 8.0 * double(rows) +
                      double(size_t(256) << 20);
  if (need > double(free_b))
    throw std::runtime_error("EASE: the dense item Gram matrix and the workspace of its inverse for " +
                             std::to_string(cols) + " items need " +
                             std::to_string(static_cast<int64_t>(need / 1048576.0)) + " MiB of device memory, " +
                             std::to_string(free_b >> 20) + " MiB are free.");

  Event e0, e1, e2, e3, e4, e5;
  IRS_HIP(hipEventRecord(e0.e, s));
  DeviceBuffer<float> d_A, d_Wk;
  DeviceBuffer<int32_t> d_flag;
  d_A.alloc(NP2);
  d_A.zero(s);
  d_flag.alloc(1);
  d_flag.zero(s);
  slim::GramInput in;
  slim::upload_and_gram(rows, cols, indptr, indices, data, in, d_A.ptr, n_pad, s);
  hipLaunchKernelGGL(dslim_add_diag_kernel, dim3(static_cast<unsigned>(ceil_div(n_pad, 256))), dim3(256), 0, s,
                     d_A.ptr, n, np, reg, diag_scale);
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipEventRecord(e1.e, s));

  // P = L L^T
  float *A = d_A.ptr;
  launch_tile_cholesky(A, np, nb, d_flag.ptr, s);
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipEventRecord(e2.e, s));
  int32_t flag = 0;
  IRS_HIP(hipMemcpyAsync(&flag, d_flag.ptr, sizeof(flag), hipMemcpyDeviceToHost, s));
  IRS_HIP(hipStreamSynchronize(s));
  if (flag != 0) {
    // the first column whose pivot failed: every earlier diagonal entry of L is positive and finite, that
    // one is sqrt of a value that is not (0, NaN or inf)
    std::vector<float> diag(static_cast<size_t>(cols));
    IRS_HIP(hipMemcpy2D(diag.data(), sizeof(float), A, (static_cast<size_t>(n_pad) + 1) * sizeof(float), sizeof(float),
                        static_cast<size_t>(cols), hipMemcpyDeviceToHost));
    int64_t bad = 0;
    while (bad < cols - 1 && diag[bad] > 0.f && std::isfinite(diag[bad])) bad++;
    throw NotPositiveDefinite(not_pd_message(bad));
  }

  // M = L^-1 into the workspace, B = M^T M back over A
  d_Wk.alloc(NP2);
  d_Wk.zero(s);
  float *M = d_Wk.ptr;
  launch_tile_tri_inverse(A, M, np, nb, s);
  hipLaunchKernelGGL(dslim_mtm_kernel, dim3(static_cast<unsigned>(nb * (nb + 1) / 2)), dim3(256), 0, s,
                     static_cast<const float *>(M), np, A);
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipEventRecord(e3.e, s));

  // W over the workspace, then home
  hipLaunchKernelGGL(dslim_finalize_kernel, dim3(static_cast<unsigned>(nb), static_cast<unsigned>(nb)), dim3(256), 0,
                     s, static_cast<const float *>(A), np, n, M);
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipEventRecord(e4.e, s));
  IRS_HIP(hipMemcpyAsync(W, M, static_cast<size_t>(cols) * static_cast<size_t>(cols) * sizeof(float),
                         hipMemcpyDeviceToHost, s));
  IRS_HIP(hipEventRecord(e5.e, s));
  IRS_HIP(hipStreamSynchronize(s));
  if (stats) {
    stats->gram_ms = elapsed_ms(e0, e1);
    stats->factor_ms = elapsed_ms(e1, e2);
    stats->invert_ms = elapsed_ms(e2, e3);
    stats->finalize_ms = elapsed_ms(e3, e4);
    stats->d2h_ms = elapsed_ms(e4, e5);
  }
}

}  // namespace dslim
}  // namespace irs

using namespace irs;

extern "C" {

irs_status irs_dense_slim_fit(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices,
                              const float *data, float reg, float diag_scale, int32_t device, float *W,
                              irs_dense_slim_stats *stats) {
  return guard([&] {
    validate_csr(rows, cols, indptr, indices, data);
    check_arg(cols == 0 || W != nullptr, "W must not be null.");
    dslim::fit(rows, cols, indptr, indices, data, reg, diag_scale, device, W, stats);
  });
}

}  // extern "C"
