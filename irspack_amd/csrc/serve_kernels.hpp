// Serving (irs_serve_*): what a resident model keeps on the device and the output stage of a recommend call.
// A call scores its rows chunk by chunk with the evaluator's own kernels (sim_score_kernel,
// dense_sim_score_kernel, the fp32 MFMA factor tiles), masks the chunk (mask_block_kernel), ranks it
// (rank_rows_kernel / rank_wave_kernel with EvalParams::retrieve = 1) and then emits (index, score) pairs:
// the score block never leaves the device.
// (Included by evaluator.hip inside its translation unit, after the kernels above.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

namespace irs {
namespace eval {

// One wave per row: reads the row's ranked items (`rec`: [rows, width], best first, -1 padded - what the rank
// kernels leave with retrieve = 1), gathers each winner's score from the masked block, narrows it to float32
// (round to nearest: the reference returns pair<int64_t, float>, util.hpp:426-504) and writes the row's part of
// the three output arrays.  Any width: 64 slots per step (cutoffs above SEL_CAP included).
template <class T>
__global__ __launch_bounds__(256) void serve_emit_kernel(const int32_t *__restrict__ rec, const T *__restrict__ scores,
                                                         int64_t rows, int64_t n_items, int32_t width,
                                                         int32_t *__restrict__ out_idx, float *__restrict__ out_score,
                                                         int32_t *__restrict__ out_len) {
  const int ln = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + wave_index_in_block();
  if (row >= rows) return;
  const int32_t *rec_row = rec + row * width;
  const T *srow = scores + row * n_items;
  int32_t *idx_row = out_idx + row * width;
  float *score_row = out_score + row * width;
  int32_t n = 0;
  for (int32_t b = 0; b < width; b += 64) {
    const int32_t i = b + ln;
    const int32_t it = i < width ? rec_row[i] : -1;
    const bool live = it >= 0 && it < n_items;
    float sc = 0.0f;
    if (live) {
      if constexpr (sizeof(T) == 8)
        sc = __double2float_rn(srow[it]);
      else
        sc = srow[it];
    }
    if (i < width) {
      idx_row[i] = live ? it : -1;
      score_row[i] = sc;
    }
    n += __popcll(__ballot(live));
  }
  if (ln == 0) out_len[row] = n;
}

}  // namespace eval
}  // namespace irs

// The resident model (one of three kinds) and the scratch a call reuses (grow-only: a second call of the same
// size allocates nothing).  The scratch is ONE set per handle, so `call_mutex` lets one recommend call at a time
// use it: calls from several threads on one handle are safe and run one after the other.
struct irs_server {
  enum Kind { SPARSE = 0, DENSE = 1, FACTORS = 2 };
  int kind = SPARSE;
  int device = 0;
  int64_t n_profile_cols = 0, n_items = 0;
  // SPARSE: W by rows, and per (row, tile) the first entry inside the tile when the rows are sorted
  irs::DeviceBuffer<int64_t> w_ptr;
  irs::DeviceBuffer<int32_t> w_idx, w_tptr;
  irs::DeviceBuffer<double> w_val;
  int64_t w_nnz = 0;
  int32_t n_tiles = 1;
  bool w_tiled = false;
  // DENSE: W [n_profile_cols, n_items] row-major, float32 or float64
  irs::DeviceBuffer<char> w_dense;
  int w_is_f64 = 0;
  // FACTORS: the item table, rows zero-padded to KP
  irs::DeviceBuffer<float> item;
  int32_t k = 0, KP = 0;
  // per call
  irs::DeviceBuffer<int64_t> x_ptr, excl_ptr, list_ptr;
  irs::DeviceBuffer<int32_t> x_idx, excl_idx, list_items, order, rec, todo, out_idx, out_len;
  irs::DeviceBuffer<double> x_val;
  irs::DeviceBuffer<float> user, out_score;
  irs::DeviceBuffer<irs::eval::RowOut> row_out;
  irs::DeviceBuffer<char> scores;
  double phase_ms[4] = {0.0, 0.0, 0.0, 0.0};
  std::mutex call_mutex;  // held from the first use of the scratch to the end of a recommend call
};
