// Device side of sparse_block_plan.hpp, shared by the truncated SVD (truncsvd.hip) and the NMF fit (nmf.hip): a
// CSR matrix on the device with its segment plan, the upload of a matrix with its transpose, and the launches
// of a product kernel at the planned width, of its split-row reduce and of the partial sums of a Gram pass.
#pragma once
#include <type_traits>

#include "sparse_block_plan.hpp"
#include "truncsvd_kernels.hpp"

namespace irs {
namespace sblock {

// a CSR matrix on the device with its segment list (tsvd_spmm_kernel)
struct Csr {
  int64_t rows = 0, cols = 0;
  DeviceBuffer<int32_t> idx, seg_row, seg_begin, seg_end, seg_slot, split_row, split_first, split_count;
  DeviceBuffer<float> val;
  int64_t n_seg = 0, n_split = 0, n_slot = 0;
};

// the segment plan of the row pointers `ptr` onto the device (blocking copies out of temporaries: set-up, once
// per matrix)
static void upload_segments(const std::vector<int32_t> &ptr, Csr &m) {
  const SegmentPlan p = plan_segments(ptr);
  auto put = [&](DeviceBuffer<int32_t> &d, const std::vector<int32_t> &v) {
    d.alloc(v.size());
    if (!v.empty()) IRS_HIP(hipMemcpy(d.ptr, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  };
  put(m.seg_row, p.seg_row);
  put(m.seg_begin, p.seg_begin);
  put(m.seg_end, p.seg_end);
  put(m.seg_slot, p.seg_slot);
  put(m.split_row, p.split_row);
  put(m.split_first, p.split_first);
  put(m.split_count, p.split_count);
  m.n_seg = p.n_seg, m.n_split = p.n_split, m.n_slot = p.n_slot;
}

// X (rows x cols, validated) and X^T on the device with their segment lists; `partial` gets a slot of
// `partial_width` floats for every segment of a split row of the matrix that has more of them.  h_ptr, the row
// pointers in 32 bits, is the source of an asynchronous copy: it must live until `s` is next synchronised
// (the transpose does that when nnz > 0).
static void upload_with_transpose(const std::vector<int32_t> &h_ptr, const int32_t *indices, const float *data,
                                  int64_t rows, int64_t cols, int64_t nnz, Csr &X, Csr &Xt,
                                  DeviceBuffer<float> &partial, int64_t partial_width, hipStream_t s) {
  X.rows = rows, X.cols = cols, Xt.rows = cols, Xt.cols = rows;
  DeviceBuffer<int32_t> d_ptr;
  d_ptr.upload(h_ptr, s);
  X.idx.upload(indices, static_cast<size_t>(nnz), s);
  X.val.upload(data, static_cast<size_t>(nnz), s);
  Xt.idx.alloc(static_cast<size_t>(nnz));
  Xt.val.alloc(static_cast<size_t>(nnz));
  std::vector<int32_t> col_count(static_cast<size_t>(cols), 0);
  DeviceBuffer<char> tmp;
  if (nnz > 0)
    transpose_csr_device(d_ptr.ptr, X.idx.ptr, X.val.ptr, rows, cols, nnz, Xt.idx.ptr, Xt.val.ptr, col_count, tmp, s);
  std::vector<int32_t> t_ptr(static_cast<size_t>(cols) + 1, 0);
  for (int64_t c = 0; c < cols; c++) t_ptr[c + 1] = t_ptr[c] + col_count[c];
  upload_segments(h_ptr, X);
  upload_segments(t_ptr, Xt);
  partial.alloc(static_cast<size_t>(std::max<int64_t>(1, std::max(X.n_slot, Xt.n_slot)) * partial_width));
}

// f(LPR, NCH) with spmm_width(lvec) as std::integral_constants: the caller names its kernel<LPR, NCH>
template <int V> using Int = std::integral_constant<int, V>;
template <class F> static void for_spmm_width(int lvec, F &&f) {
  const SpmmWidth w = spmm_width(lvec);
  if (w.lpr == 16) f(Int<16>{}, Int<1>{});
  else if (w.lpr == 32) f(Int<32>{}, Int<1>{});
  else if (w.nch == 1) f(Int<64>{}, Int<1>{});
  else if (w.nch == 2) f(Int<64>{}, Int<2>{});
  else f(Int<64>{}, Int<3>{});
}

// out (M.rows x l_pad) = M in (M.cols x l_pad) by an instance of tsvd_spmm_kernel or nmf_spmm_kernel; the
// segments of split rows go to `partial`
template <class K, class P>
static void launch_spmm(K kernel, const Csr &M, const float *in, int l_pad, float *out, P *partial, hipStream_t s) {
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(ceil_div(M.n_seg, 4))), dim3(256), 0, s,
                     static_cast<const int32_t *>(M.seg_row.ptr), static_cast<const int32_t *>(M.seg_begin.ptr),
                     static_cast<const int32_t *>(M.seg_end.ptr), static_cast<const int32_t *>(M.seg_slot.ptr),
                     static_cast<int>(M.n_seg), static_cast<const int32_t *>(M.idx.ptr),
                     static_cast<const float *>(M.val.ptr), in, l_pad, out, partial);
}

// the split rows of M summed out of `partial` in segment order (tsvd_spmm_reduce_kernel, or
// nmf_spmm_reduce_f64_kernel for sums kept in double)
template <class K, class P>
static void launch_split_reduce(K kernel, const Csr &M, const P *partial, int l_pad, float *out, hipStream_t s) {
  if (M.n_split > 0)
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(M.n_split)), dim3(256), 0, s,
                       static_cast<const int32_t *>(M.split_row.ptr), static_cast<const int32_t *>(M.split_first.ptr),
                       static_cast<const int32_t *>(M.split_count.ptr), partial, l_pad, out);
}

// the per-slab partial sums of B^T B for the block B of `rows` rows and l_pad columns; the caller reduces them
// over pass.n_slab with its own kernel
static GramPass launch_gram_partials(const float *B, int64_t rows, int64_t l_pad, float *gram_partial,
                                     hipStream_t s) {
  const GramPass pass = plan_gram_pass(rows, l_pad);
  hipLaunchKernelGGL(tsvd::tsvd_gram_kernel,
                     dim3(static_cast<unsigned>(pass.n_tile), static_cast<unsigned>(pass.n_slab)), dim3(256), 0, s, B,
                     static_cast<int>(rows), static_cast<int>(l_pad), static_cast<int>(pass.rows_per_slab),
                     gram_partial);
  return pass;
}

}  // namespace sblock
}  // namespace irs
