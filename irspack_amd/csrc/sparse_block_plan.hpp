// Host planning of the sparse x tall-block products and the tiled Gram passes that the truncated SVD
// (truncsvd.hip) and the NMF fit (nmf.hip) share: the segment list of a CSR matrix, the slabs of a Gram pass and
// the kernel width of a product.  No HIP in it: it compiles with the host compiler alone
// (tests/host/sparse_block_plan_main.cpp); sparse_block.hpp puts the plans on the device and launches.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "host_util.hpp"

namespace irs {
namespace sblock {

// restated from the kernel headers (SPMM_SEG of truncsvd_kernels.hpp, RIDGE_NB of chol_tile_kernels.hpp);
// truncsvd.hip sees both sides and asserts that they agree
constexpr int SEG_LEN = 1024;
constexpr int TILE_EDGE = 64;
constexpr int64_t MAX_L_PAD = 576;  // the widest block: 9 tiles, the last rung of spmm_width

// the segment list of tsvd_spmm_kernel and the split rows of its reduce
struct SegmentPlan {
  std::vector<int32_t> seg_row, seg_begin, seg_end, seg_slot, split_row, split_first, split_count;
  int64_t n_seg = 0, n_split = 0, n_slot = 0;
};

// rows cut into segments of at most SEG_LEN entries, longest segments first (stable); a row of several
// segments gets consecutive slots of the partial buffer
inline SegmentPlan plan_segments(const std::vector<int32_t> &ptr) {
  const int64_t rows = static_cast<int64_t>(ptr.size()) - 1;
  std::vector<int32_t> row, beg, end, slot;
  SegmentPlan p;
  int32_t n_slot = 0;
  for (int64_t r = 0; r < rows; r++) {
    const int32_t b = ptr[r], e = ptr[r + 1];
    const int32_t pieces = std::max<int32_t>(1, static_cast<int32_t>(ceil_div(e - b, SEG_LEN)));
    if (pieces > 1) {
      p.split_row.push_back(static_cast<int32_t>(r));
      p.split_first.push_back(n_slot);
      p.split_count.push_back(pieces);
    }
    for (int32_t k = 0; k < pieces; k++) {
      row.push_back(static_cast<int32_t>(r));
      beg.push_back(b + k * SEG_LEN);
      end.push_back(std::min(e, b + (k + 1) * SEG_LEN));
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
  p.seg_row = permuted(row), p.seg_begin = permuted(beg), p.seg_end = permuted(end), p.seg_slot = permuted(slot);
  p.n_seg = static_cast<int64_t>(row.size());
  p.n_split = static_cast<int64_t>(p.split_row.size());
  p.n_slot = n_slot;
  return p;
}

// row slabs of a Gram pass: about 2,048 workgroups, at most 256 partial sums per element for the reduce
inline int64_t gram_slabs(int64_t n_tile) { return std::min<int64_t>(256, std::max<int64_t>(1, 2048 / n_tile)); }

// the grid of a Gram pass over a block of `rows` rows and l_pad columns: the lower tiles by the slabs, a slab
// a whole number of 64-row chunks
struct GramPass {
  int64_t n_tile, n_slab, rows_per_slab;
};
inline GramPass plan_gram_pass(int64_t rows, int64_t l_pad) {
  const int64_t nb = l_pad / TILE_EDGE, n_tile = nb * (nb + 1) / 2;
  const int64_t chunks = std::max<int64_t>(1, ceil_div(rows, TILE_EDGE));
  const int64_t want_slabs = std::min(chunks, gram_slabs(n_tile));
  const int64_t chunks_per_slab = ceil_div(chunks, want_slabs), n_slab = ceil_div(chunks, chunks_per_slab);
  return {n_tile, n_slab, chunks_per_slab * TILE_EDGE};
}

// the instance <LPR, NCH> of a product kernel for a block of lvec = l_pad / 4 float4 columns: LPR lanes per row,
// each with NCH float4 columns
struct SpmmWidth {
  int lpr, nch;
};
inline SpmmWidth spmm_width(int lvec) {
  if (lvec == 16) return {16, 1};
  if (lvec == 32) return {32, 1};
  if (lvec <= 64) return {64, 1};
  if (lvec <= 128) return {64, 2};
  return {64, 3};
}

}  // namespace sblock
}  // namespace irs
