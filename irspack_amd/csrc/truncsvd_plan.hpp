// The host planning that the truncated SVD (truncsvd.hip) and the NMF fit (nmf.hip) share: a CSR matrix on the
// device with the segment list of tsvd_spmm_kernel, the launch of that kernel and the slab count of a Gram pass.
#pragma once
#include <algorithm>
#include <numeric>

#include "truncsvd_kernels.hpp"

namespace irs {
namespace tsvd {

constexpr int64_t MAX_L_PAD = 576;

// a CSR matrix on the device with its segment list (tsvd_spmm_kernel)
struct Csr {
  int64_t rows = 0, cols = 0;
  DeviceBuffer<int32_t> idx, seg_row, seg_begin, seg_end, seg_slot, split_row, split_first, split_count;
  DeviceBuffer<float> val;
  int64_t n_seg = 0, n_split = 0, n_slot = 0;
};

// rows cut into segments of at most SPMM_SEG entries, longest segments first (stable); a row of several
// segments gets consecutive slots of the partial buffer
static void build_segments(const std::vector<int32_t> &ptr, Csr &m) {
  const int64_t rows = static_cast<int64_t>(ptr.size()) - 1;
  std::vector<int32_t> row, beg, end, slot, srow, sfirst, scount;
  int32_t n_slot = 0;
  for (int64_t r = 0; r < rows; r++) {
    const int32_t b = ptr[r], e = ptr[r + 1];
    const int32_t pieces = std::max<int32_t>(1, static_cast<int32_t>(ceil_div(e - b, SPMM_SEG)));
    if (pieces > 1) {
      srow.push_back(static_cast<int32_t>(r));
      sfirst.push_back(n_slot);
      scount.push_back(pieces);
    }
    for (int32_t k = 0; k < pieces; k++) {
      row.push_back(static_cast<int32_t>(r));
      beg.push_back(b + k * SPMM_SEG);
      end.push_back(std::min(e, b + (k + 1) * SPMM_SEG));
      slot.push_back(pieces > 1 ? n_slot++ : -1);
    }
  }
  std::vector<int32_t> order(row.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t a, int32_t b) { return end[a] - beg[a] > end[b] - beg[b]; });
  auto permuted = [&](const std::vector<int32_t> &v) {
    std::vector<int32_t> out(v.size());
    for (size_t i = 0; i < v.size(); i++) out[i] = v[order[i]];
    return out;
  };
  // (blocking copies out of temporaries: set-up, once per handle)
  auto put = [&](DeviceBuffer<int32_t> &d, const std::vector<int32_t> &v) {
    d.alloc(v.size());
    if (!v.empty()) IRS_HIP(hipMemcpy(d.ptr, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  };
  put(m.seg_row, permuted(row));
  put(m.seg_begin, permuted(beg));
  put(m.seg_end, permuted(end));
  put(m.seg_slot, permuted(slot));
  put(m.split_row, srow);
  put(m.split_first, sfirst);
  put(m.split_count, scount);
  m.n_seg = static_cast<int64_t>(row.size());
  m.n_split = static_cast<int64_t>(srow.size());
  m.n_slot = n_slot;
}

template <int LPR, int NCH>
static void launch_spmm(const Csr &M, const float *Q, int l_pad, float *Y, float *partial, hipStream_t s) {
  hipLaunchKernelGGL((tsvd_spmm_kernel<LPR, NCH>), dim3(static_cast<unsigned>(ceil_div(M.n_seg, 4))), dim3(256), 0,
                     s, static_cast<const int32_t *>(M.seg_row.ptr), static_cast<const int32_t *>(M.seg_begin.ptr),
                     static_cast<const int32_t *>(M.seg_end.ptr), static_cast<const int32_t *>(M.seg_slot.ptr),
                     static_cast<int>(M.n_seg), static_cast<const int32_t *>(M.idx.ptr),
                     static_cast<const float *>(M.val.ptr), Q, l_pad, Y, partial);
}

// row slabs of a Gram pass: about 2,048 workgroups, at most 256 partial sums per element for the reduce
static int64_t gram_slabs(int64_t n_tile) { return std::min<int64_t>(256, std::max<int64_t>(1, 2048 / n_tile)); }

}  // namespace tsvd
}  // namespace irs
