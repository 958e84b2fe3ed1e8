// The launch sequences of the tiled Cholesky factorisation (chol_tile_kernels.hpp) and of the tiled inverse of
// its factor (tri_inv_kernels.hpp), shared by the truncated SVD, EASE / EDLAE and the iALS feature ridge.
// static, like the kernels they launch: every translation unit launches its own copy of the kernels.  The caller
// brackets the sequence with its span or profiler range and checks hipGetLastError after it.
#pragma once
#include "chol_tile_kernels.hpp"
#include "host_util.hpp"
#include "tri_inv_kernels.hpp"

namespace irs {

// G (nb x nb tiles of 64 x 64, row stride ld) = L L^T in place, L over the lower triangle, one block column
// after the other; a pivot that is not > 0 or not finite raises `flag`
static void launch_tile_cholesky(float *G, int ld, int64_t nb, int32_t *flag, hipStream_t s) {
  for (int64_t k = 0; k < nb; k++) {
    hipLaunchKernelGGL(ials::ridge_chol_diag_kernel, dim3(1), dim3(256), 0, s, G, ld, static_cast<int>(k), flag);
    const int64_t t = nb - k - 1;  // block rows below the diagonal tile
    if (t == 0) continue;
    hipLaunchKernelGGL(ials::ridge_chol_trsm_kernel, dim3(static_cast<unsigned>(ceil_div(t * ials::RIDGE_NB, 256))),
                       dim3(256), 0, s, G, ld, static_cast<int>(k));
    hipLaunchKernelGGL(ials::ridge_chol_update_kernel, dim3(static_cast<unsigned>(t * (t + 1) / 2)), dim3(256), 0, s,
                       G, ld, static_cast<int>(k));
  }
}

// W = L^-1 for the factor L of launch_tile_cholesky: the diagonal tiles inverted, then block forward
// substitution restricted to the lower triangle.  W is zeroed by the caller.
static void launch_tile_tri_inverse(const float *L, float *W, int ld, int64_t nb, hipStream_t s) {
  hipLaunchKernelGGL(dslim::dslim_diag_inv_kernel, dim3(static_cast<unsigned>(nb)), dim3(64), 0, s, L, ld, W);
  for (int64_t k = 0; k < nb; k++) {
    if (k > 0)
      hipLaunchKernelGGL(dslim::dslim_inv_row_kernel, dim3(static_cast<unsigned>(k)), dim3(256), 0, s, W, ld,
                         static_cast<int>(k));
    if (k + 1 < nb)
      hipLaunchKernelGGL(dslim::dslim_inv_update_kernel,
                         dim3(static_cast<unsigned>(nb - k - 1), static_cast<unsigned>(k + 1)), dim3(256), 0, s, L, W,
                         ld, static_cast<int>(k));
  }
}

}  // namespace irs
