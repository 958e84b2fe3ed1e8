// Serving (irs_serve_*): what a resident model keeps on the device and the output stage of a recommend call.
// A call scores its rows chunk by chunk with the evaluator's own kernels (sim_score_kernel,
// dense_sim_score_kernel, the fp32 MFMA factor tiles), masks the chunk (mask_block_kernel), ranks it
// (rank_rows_kernel / rank_wave_kernel with EvalParams::retrieve = 1) and then emits (index, score) pairs:
// the score block never leaves the device.  A neighbour call (irs_serve_neighbors) builds its score block from the
// resident operand itself (the nb_* kernels) and goes through the same mask, rank and emit.
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

// ---- neighbours (irs_serve_neighbors): the score block of "entities like ids[r]" out of the resident operand ----
// Bandwidth-bound passes, one workgroup of 256 per row of the chunk (any chunk size: the row is blockIdx.x), no
// atomics; every loop runs the same number of times in every lane (the bounds test is inside the body).

constexpr int NB_THREADS = 256;

// row[0 .. n) = -inf: 16-byte stores from the first 16-byte boundary on (a row of an odd-width block starts 8 off)
__device__ inline void nb_fill_row(double *row, int64_t n) {
  const double ninf = -std::numeric_limits<double>::infinity();
  const int64_t head = n > 0 ? static_cast<int64_t>((reinterpret_cast<uintptr_t>(row) >> 3) & 1) : 0;
  double2 *body = reinterpret_cast<double2 *>(row + head);
  const int64_t n_pairs = (n - head) / 2;
  for (int64_t base = 0; base < n_pairs; base += NB_THREADS) {
    const int64_t i = base + threadIdx.x;
    if (i < n_pairs) body[i] = make_double2(ninf, ninf);
  }
  if (threadIdx.x == 0) {
    if (head) row[0] = ninf;
    if (head + 2 * n_pairs < n) row[n - 1] = ninf;
  }
}

// Sparse W: row r of the block is -inf, then the stored entries of row ids[r] of W (stored zeros too; no column
// is stored twice, the constructor saw to that; any order), the entity itself left at -inf.  The fill and the
// scatter are two phases of one workgroup with a barrier between them.
__global__ __launch_bounds__(NB_THREADS) void nb_sparse_rows_kernel(double *__restrict__ block, int64_t rows,
                                                                    int64_t n_items, const int64_t *__restrict__ ids,
                                                                    const int64_t *__restrict__ w_ptr,
                                                                    const int32_t *__restrict__ w_idx,
                                                                    const double *__restrict__ w_val) {
  const int64_t r = blockIdx.x;
  if (r >= rows) return;
  double *row = block + r * n_items;
  nb_fill_row(row, n_items);
  __syncthreads();
  const int64_t self = ids[r];
  const int64_t first = w_ptr[self], count = w_ptr[self + 1] - first;
  for (int64_t base = 0; base < count; base += NB_THREADS) {
    const int64_t q = base + threadIdx.x;
    if (q < count) {
      const int32_t j = w_idx[first + q];
      if (j != self && j >= 0 && j < n_items) row[j] = w_val[first + q];
    }
  }
}

// Dense W (float32 widened exactly, or float64): row r of the block is row ids[r] of W with the entity itself at
// -inf.  Four columns per lane and step: one float4 (two double2) load and two double2 stores when the width is a
// multiple of 4 (every row of W and of the block then starts on a 32-byte boundary), single elements otherwise.
template <class TW>
__global__ __launch_bounds__(NB_THREADS) void nb_dense_rows_kernel(double *__restrict__ block, int64_t rows,
                                                                   int64_t n_items, const int64_t *__restrict__ ids,
                                                                   const TW *__restrict__ W) {
  const int64_t r = blockIdx.x;
  if (r >= rows) return;
  const double ninf = -std::numeric_limits<double>::infinity();
  const int64_t self = ids[r];
  const TW *src = W + self * n_items;
  double *row = block + r * n_items;
  if ((n_items & 3) == 0) {
    const int64_t n_quads = n_items / 4;
    for (int64_t base = 0; base < n_quads; base += NB_THREADS) {
      const int64_t i = base + threadIdx.x;
      if (i < n_quads) {
        double v[4];
        if constexpr (sizeof(TW) == 4) {
          const float4 f = reinterpret_cast<const float4 *>(src)[i];
          v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
          const double2 a = reinterpret_cast<const double2 *>(src)[2 * i];
          const double2 b = reinterpret_cast<const double2 *>(src)[2 * i + 1];
          v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
        }
        const int64_t e = self - 4 * i;  // (0 .. 3 in the one lane that holds the entity itself)
        reinterpret_cast<double2 *>(row)[2 * i] = make_double2(e == 0 ? ninf : v[0], e == 1 ? ninf : v[1]);
        reinterpret_cast<double2 *>(row)[2 * i + 1] = make_double2(e == 2 ? ninf : v[2], e == 3 ? ninf : v[3]);
      }
    }
  } else {
    for (int64_t base = 0; base < n_items; base += NB_THREADS) {
      const int64_t j = base + threadIdx.x;
      if (j < n_items) row[j] = j == self ? ninf : static_cast<double>(src[j]);
    }
  }
}

// Factor tables [n, KP] (KP a multiple of 32, so a row is a whole number of 128-byte pieces): eight lanes share a
// row, a float4 each per step of 32 columns; 32 rows per workgroup.
constexpr int NB_ROW_LANES = 8, NB_ROWS_PER_BLOCK = NB_THREADS / NB_ROW_LANES;

// inv[i] = 1 / ||table[i, 0:k_used]||_2, or 0 for a row of zeros: the squares are summed and the root is taken in
// double (a row scaled by 1e19 overflows a float32 sum of squares, one scaled by 1e-20 vanishes in it), one
// rounding to float32 at the end.  The eight partial sums are folded by a fixed shuffle tree: the same bits at
// every call.
__global__ __launch_bounds__(NB_THREADS) void nb_inv_norm_kernel(const float *__restrict__ table, int64_t n,
                                                                 int32_t KP, int32_t k_used, float *__restrict__ inv) {
  const int sub = threadIdx.x & (NB_ROW_LANES - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * NB_ROWS_PER_BLOCK + threadIdx.x / NB_ROW_LANES;
  const bool live = i < n;
  const float *row = table + (live ? i : 0) * KP;
  double sum = 0.0;
  for (int32_t c = 0; c < k_used; c += 4 * NB_ROW_LANES) {  // (c + 4 * sub + 3 < KP: KP is a multiple of 32)
    const int32_t col = c + 4 * sub;
    const float4 f = *reinterpret_cast<const float4 *>(row + col);
    const double x[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (col + e < k_used) sum += x[e] * x[e];
  }
#pragma unroll
  for (int d = NB_ROW_LANES / 2; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, NB_ROW_LANES);
  if (live && sub == 0) inv[i] = sum > 0.0 ? static_cast<float>(1.0 / sqrt(sum)) : 0.0f;
}

// The query block of a call: out[r, :] = table[ids[r], 0:k_used] * (inv ? inv[ids[r]] : 1), zero from k_used to KP
// (what the MFMA tiles read).  Nothing comes from the host.
__global__ __launch_bounds__(NB_THREADS) void nb_gather_kernel(const float *__restrict__ table,
                                                               const int64_t *__restrict__ ids, int64_t rows,
                                                               int32_t KP, int32_t k_used,
                                                               const float *__restrict__ inv, float *__restrict__ out) {
  const int sub = threadIdx.x & (NB_ROW_LANES - 1);
  const int64_t r = static_cast<int64_t>(blockIdx.x) * NB_ROWS_PER_BLOCK + threadIdx.x / NB_ROW_LANES;
  const bool live = r < rows;
  const int64_t self = live ? ids[r] : 0;
  const float scale = inv ? inv[self] : 1.0f;
  const float *src = table + self * KP;
  for (int32_t c = 0; c < KP; c += 4 * NB_ROW_LANES) {
    const int32_t col = c + 4 * sub;
    float4 f = *reinterpret_cast<const float4 *>(src + col);
    f.x = col + 0 < k_used ? f.x * scale : 0.0f;
    f.y = col + 1 < k_used ? f.y * scale : 0.0f;
    f.z = col + 2 < k_used ? f.z * scale : 0.0f;
    f.w = col + 3 < k_used ? f.w * scale : 0.0f;
    if (live) *reinterpret_cast<float4 *>(out + r * KP + col) = f;
  }
}

// After the tiles: cosine multiplies score[r, j] by inv[j]; a candidate of norm zero, and the whole row of a query
// of norm zero, become -inf; the entity itself becomes -inf.  `inv` null (dot): only the last.  float4 when the
// width is a multiple of 4.
__device__ inline float nb_finish_one(float s, int64_t j, int64_t self, float inv_q, const float *__restrict__ inv) {
  const float inv_j = inv[j];
  return (j == self || inv_j == 0.0f || inv_q == 0.0f) ? -std::numeric_limits<float>::infinity() : s * inv_j;
}

__global__ __launch_bounds__(NB_THREADS) void nb_finish_kernel(float *__restrict__ block, int64_t rows,
                                                               int64_t n_items, const int64_t *__restrict__ ids,
                                                               const float *__restrict__ inv) {
  const int64_t r = blockIdx.x;
  if (r >= rows) return;
  const int64_t self = ids[r];
  float *row = block + r * n_items;
  if (inv == nullptr) {
    if (threadIdx.x == 0) row[self] = -std::numeric_limits<float>::infinity();
    return;
  }
  const float inv_q = inv[self];
  if ((n_items & 3) == 0) {
    const int64_t n_quads = n_items / 4;
    for (int64_t base = 0; base < n_quads; base += NB_THREADS) {
      const int64_t i = base + threadIdx.x;
      if (i < n_quads) {
        float4 f = reinterpret_cast<float4 *>(row)[i];
        const float4 w = reinterpret_cast<const float4 *>(inv)[i];
        const float ninf = -std::numeric_limits<float>::infinity();
        const bool dead = inv_q == 0.0f;
        const int64_t e = self - 4 * i;  // (0 .. 3 in the one lane that holds the entity itself)
        f.x = (dead || w.x == 0.0f || e == 0) ? ninf : f.x * w.x;
        f.y = (dead || w.y == 0.0f || e == 1) ? ninf : f.y * w.y;
        f.z = (dead || w.z == 0.0f || e == 2) ? ninf : f.z * w.z;
        f.w = (dead || w.w == 0.0f || e == 3) ? ninf : f.w * w.w;
        reinterpret_cast<float4 *>(row)[i] = f;
      }
    }
  } else {
    for (int64_t base = 0; base < n_items; base += NB_THREADS) {
      const int64_t j = base + threadIdx.x;
      if (j < n_items) row[j] = nb_finish_one(row[j], j, self, inv_q, inv);
    }
  }
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
  // FACTORS, neighbour calls: one inverse L2 norm per table row over the leading `inv_norm_k` columns (0: not made
  // yet); made at the first cosine call and again when k_used changes
  irs::DeviceBuffer<float> inv_norm;
  int32_t inv_norm_k = 0;
  // per call
  irs::DeviceBuffer<int64_t> nb_ids;  // the query entities of a neighbour call
  irs::DeviceBuffer<int64_t> x_ptr, excl_ptr, list_ptr;
  irs::DeviceBuffer<int32_t> x_idx, excl_idx, list_items, order, rec, todo, out_idx, out_len;
  irs::DeviceBuffer<double> x_val;
  irs::DeviceBuffer<float> user, out_score;
  irs::DeviceBuffer<irs::eval::RowOut> row_out;
  irs::DeviceBuffer<char> scores;
  double phase_ms[4] = {0.0, 0.0, 0.0, 0.0};
  std::mutex call_mutex;  // held from the first use of the scratch to the end of a recommend call
};
