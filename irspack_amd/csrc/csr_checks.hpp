// Invalid-argument checks of a CSR matrix handed to the C ABI, before any device work.  No HIP in it: it compiles
// with the host compiler alone (tests/host/sparse_block_plan_main.cpp, bpr_host_prep_main.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#include "host_util.hpp"

namespace irs {

// Monotone indptr, sizes below 2^31, indices in range and strictly ascending within a row (the Gram kernel's
// lanes must hit distinct elements).  Returns nnz.
inline int64_t validate_csr(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices,
                            const float *data) {
  check_arg(rows >= 0 && cols >= 0 && indptr && indptr[0] == 0, "bad matrix.");
  check_arg(rows < (int64_t(1) << 31) - 1 && cols < (int64_t(1) << 31) - 1, "rows and cols must be below 2^31.");
  for (int64_t i = 0; i < rows; i++) check_arg(indptr[i + 1] >= indptr[i], "malformed indptr.");
  const int64_t nnz = indptr[rows];
  check_arg(nnz < (int64_t(1) << 31), "nnz must be below 2^31.");
  check_arg(nnz == 0 || (indices && data), "bad matrix.");
  for (int64_t i = 0; i < rows; i++) {
    int64_t prev = -1;
    for (int64_t q = indptr[i]; q < indptr[i + 1]; q++) {
      const int64_t c = indices[q];
      check_arg(c >= 0 && c < cols, "column index out of range.");
      check_arg(c != prev, "duplicate column index in a row (sum duplicates before the call).");
      check_arg(c > prev, "column indices of a row must be sorted.");
      prev = c;
    }
  }
  return nnz;
}

// validate_csr, then at least one row and one column, then every value finite (the truncated SVD, NMF, BPR / WARP
// and Mult-VAE).  Returns nnz.
inline int64_t validate_finite_matrix(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices,
                                      const float *data) {
  const int64_t nnz = validate_csr(rows, cols, indptr, indices, data);
  check_arg(rows >= 1 && cols >= 1, "the matrix must have at least one row and one column.");
  for (int64_t q = 0; q < nnz; q++) check_arg(std::isfinite(data[q]), "the matrix holds a non-finite value.");
  return nnz;
}

}  // namespace irs
