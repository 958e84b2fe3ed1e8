// The dense item Gram matrix G = X^T X on the device, shared by SLIM (slim.hip) and EASE / EDLAE
// (dense_slim.hip): the upload of X by rows and by columns, the longest-first order and gram_rows_kernel
// itself.
#pragma once
#include <algorithm>
#include <numeric>

#include "common.hpp"

namespace irs {
namespace slim {

// ---------------------------------------------------------------------------------------------- Gram
// Row f of G = sum over the users u of column f of x_uf * X[u, :].  ONE wave owns the row and walks the
// users in their stored (ascending) order; the 64 lanes take 64 entries of X[u, :] - distinct columns,
// the host rejects duplicates - so every element of G is a sum in a fixed order: bit-identical from run
// to run for any values (and exact for counts below 2^24).  A wave's loads and stores to one address
// complete in program order, so the row is accumulated in place in global memory (it stays in L2).
// `order` hands the longest columns out first.  `ld` >= n_items is the row stride of G (EASE pads it).
// (static: the header is included by two translation units of one library)
static __global__ __launch_bounds__(256) void gram_rows_kernel(const int32_t *__restrict__ rptr,
                                                               const int32_t *__restrict__ ridx,
                                                               const float *__restrict__ rval,
                                                               const int32_t *__restrict__ cptr,
                                                               const int32_t *__restrict__ cidx,
                                                               const float *__restrict__ cval,
                                                               const int32_t *__restrict__ order, int32_t n_items,
                                                               int64_t ld, float *G) {
  const int slot = static_cast<int>(blockIdx.x) * 4 + wave_index_in_block();
  if (slot >= n_items) return;
  const int lane = static_cast<int>(threadIdx.x & 63);
  const int f = order[slot];
  float *row = G + static_cast<int64_t>(f) * ld;
  const int p_end = cptr[f + 1];
  for (int p = cptr[f]; p < p_end; p++) {
    const int u = cidx[p];
    const float xv = cval[p];
    const int q_end = rptr[u + 1];
    for (int q = rptr[u] + lane; q < q_end; q += 64) {
      const int g = ridx[q];
      row[g] += xv * rval[q];
    }
  }
}

// X by rows and by columns on the device and the order in which the rows of G are handed out
struct GramInput {
  DeviceBuffer<int32_t> rptr, ridx, cptr, cidx, order;
  DeviceBuffer<float> rval, cval;
  DeviceBuffer<char> tmp;
  std::vector<int32_t> h_rptr, h_cptr, h_order;  // sources of asynchronous uploads: they live as long as this
};

// Uploads X (validated, nnz > 0), transposes it on the device (synchronises `s` once: the column counts
// come back to the host) and fills G, a zeroed dense matrix with row stride `ld` >= cols: rows and
// columns [0, cols) receive X^T X, the rest is left as it is.
inline void upload_and_gram(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices,
                            const float *data, GramInput &in, float *G, int64_t ld, hipStream_t s) {
  const int64_t nnz = indptr[rows];
  const size_t I = static_cast<size_t>(cols);
  std::vector<int32_t> &ip32 = in.h_rptr, &cp32 = in.h_cptr, &order = in.h_order;
  ip32.resize(static_cast<size_t>(rows) + 1);
  for (int64_t i = 0; i <= rows; i++) ip32[i] = static_cast<int32_t>(indptr[i]);
  in.rptr.upload(ip32, s);
  in.ridx.upload(indices, static_cast<size_t>(nnz), s);
  in.rval.upload(data, static_cast<size_t>(nnz), s);
  in.cidx.alloc(static_cast<size_t>(nnz));
  in.cval.alloc(static_cast<size_t>(nnz));
  std::vector<int32_t> col_count;
  transpose_csr_device(in.rptr.ptr, in.ridx.ptr, in.rval.ptr, rows, cols, nnz, in.cidx.ptr, in.cval.ptr, col_count,
                       in.tmp, s);
  cp32.assign(I + 1, 0);
  order.resize(I);
  for (size_t f = 0; f < I; f++) cp32[f + 1] = cp32[f] + col_count[f];
  // most popular columns first (Gram rows: the longest walk; descent: the most coordinate changes)
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return col_count[a] > col_count[b]; });
  in.cptr.upload(cp32, s);
  in.order.upload(order, s);
  hipLaunchKernelGGL(gram_rows_kernel, dim3(static_cast<unsigned>(ceil_div(cols, 4))), dim3(256), 0, s,
                     static_cast<const int32_t *>(in.rptr.ptr), static_cast<const int32_t *>(in.ridx.ptr),
                     static_cast<const float *>(in.rval.ptr), static_cast<const int32_t *>(in.cptr.ptr),
                     static_cast<const int32_t *>(in.cidx.ptr), static_cast<const float *>(in.cval.ptr),
                     static_cast<const int32_t *>(in.order.ptr), static_cast<int32_t>(cols), ld, G);
  IRS_HIP(hipGetLastError());
}

}  // namespace slim
}  // namespace irs
