// What follows the ranking of a block: the fixed-order sums of the per-user terms (one or two levels), the item
// histogram of the recommended lists (hashed or direct LDS table; which one: plan_item_hist, eval_emit_plan.hpp),
// and the kernels that write -inf over masked scores.
// (Included by evaluator.hip after eval_rank_kernels.hpp: RowOut.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "eval_host_prep.hpp"

namespace irs {
namespace eval {

// First level of the sum for large calls: workgroup b folds the rows [b * chunk, (b + 1) * chunk)
// into one RowOut-like partial with the SAME code as reduce_rows_kernel, so that the second
// level (reduce over the partials) keeps a fixed order.  See reduce_rows_kernel.
struct RowPartial {
  long long valid;
  double hit, recall, ndcg, precision, map;
};

// Sum of the per-user terms of one call (one 1024-thread workgroup) in a fixed order, so the
// fp64 result is reproducible run to run; it is not the strict user order of a
// single-threaded reference run (the reference's own order depends on n_threads,
// evaluator.cpp:280-312).
__global__ __launch_bounds__(1024) void reduce_rows_kernel(const RowOut *rows, int64_t n,
                                                           irs_metrics *out,
                                                           RowPartial *partials = nullptr,
                                                           int64_t chunk = 0) {
  // thread t adds rows t, t + 1024, ... in that order; the 64 lanes of a wave fold by a fixed
  // butterfly and wave 0 adds the 16 wave sums in wave order.  With `partials` workgroup b does
  // that for its chunk of rows only and leaves the sums there (reduce_partials_kernel adds the
  // chunks in order): one workgroup walking 138 k rows alone took 0.11 ms.
  __shared__ double part[16][5];
  __shared__ long long part_valid[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  long long valid = 0;
  double hit = 0, recall = 0, ndcg = 0, precision = 0, map = 0;
  if (partials) {
    rows += static_cast<int64_t>(blockIdx.x) * chunk;
    n = min(chunk, n - static_cast<int64_t>(blockIdx.x) * chunk);
  }
  for (int64_t i = tid; i < n; i += 1024) {
    const RowOut r = rows[i];
    if (r.valid) {
      valid += 1;
      hit += r.hit;
      recall += r.recall;
      ndcg += r.ndcg;
      precision += r.precision;
      map += r.map;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    valid += __shfl_xor(valid, o, 64);
    hit += __shfl_xor(hit, o, 64);
    recall += __shfl_xor(recall, o, 64);
    ndcg += __shfl_xor(ndcg, o, 64);
    precision += __shfl_xor(precision, o, 64);
    map += __shfl_xor(map, o, 64);
  }
  if (lane == 0) {
    part_valid[wv] = valid;
    part[wv][0] = hit;
    part[wv][1] = recall;
    part[wv][2] = ndcg;
    part[wv][3] = precision;
    part[wv][4] = map;
  }
  __syncthreads();
  if (tid == 0) {
    long long v = 0;
    double acc[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < 16; w++) {
      v += part_valid[w];
      for (int c = 0; c < 5; c++) acc[c] += part[w][c];
    }
    if (partials) {
      partials[blockIdx.x] = RowPartial{v, acc[0], acc[1], acc[2], acc[3], acc[4]};
      return;
    }
    out->valid_user += v;
    out->total_user += n;
    out->hit += acc[0];
    out->recall += acc[1];
    out->ndcg += acc[2];
    out->precision += acc[3];
    out->map += acc[4];
  }
}

__global__ void reduce_partials_kernel(const RowPartial *partials, int nb, int64_t n, irs_metrics *out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long v = 0;
  double acc[5] = {0, 0, 0, 0, 0};
  for (int b = 0; b < nb; b++) {  // chunk order
    v += partials[b].valid;
    acc[0] += partials[b].hit;
    acc[1] += partials[b].recall;
    acc[2] += partials[b].ndcg;
    acc[3] += partials[b].precision;
    acc[4] += partials[b].map;
  }
  out->valid_user += v;
  out->total_user += n;
  out->hit += acc[0];
  out->recall += acc[1];
  out->ndcg += acc[2];
  out->precision += acc[3];
  out->map += acc[4];
}

__global__ void merge_partials_kernel(const RowPartial *partials, int nb, int64_t n, irs_metrics *out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long v = out->valid_user;
  double acc[5] = {out->hit, out->recall, out->ndcg, out->precision, out->map};
  for (int b = 0; b < nb; b++) {  // chunk order, every chunk onto the running sum
    v += partials[b].valid;
    acc[0] += partials[b].hit;
    acc[1] += partials[b].recall;
    acc[2] += partials[b].ndcg;
    acc[3] += partials[b].precision;
    acc[4] += partials[b].map;
  }
  out->valid_user = v;
  out->total_user += n;
  out->hit = acc[0];
  out->recall = acc[1];
  out->ndcg = acc[2];
  out->precision = acc[3];
  out->map = acc[4];
}

// item_cnt[i] += how often item i stands in the recommended lists of a call (Metrics::update,
// evaluator.cpp:146).  `rec` = the lists the ranking kernels wrote ([rows, cutoff], -1 where
// there is no entry).  Everybody's list is full of the same popular items, so one global atomic
// per entry queues up on a few addresses (1 ms for 2.7 M entries); each workgroup counts its
// slice in an LDS table first (direct-mapped, a colliding item goes to memory at once) and adds
// one total per item it met.
constexpr int HIST_SLOTS = 8192;
__global__ __launch_bounds__(1024) void item_hist_kernel(const int32_t *__restrict__ rec, int64_t n,
                                                         unsigned long long *__restrict__ item_cnt) {
  __shared__ int32_t ids[HIST_SLOTS];
  __shared__ uint32_t cnt[HIST_SLOTS];
  for (int i = threadIdx.x; i < HIST_SLOTS; i += 1024) {
    ids[i] = -1;
    cnt[i] = 0;
  }
  __syncthreads();
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t b = per * blockIdx.x, e = min(b + per, n);
  for (int64_t i = b + threadIdx.x; i < e; i += 1024) {
    const int32_t it = rec[i];
    if (it < 0) continue;
    const uint32_t slot = (static_cast<uint32_t>(it) * 2654435761u) >> 19;  // 13 bits
    const int32_t prev = atomicCAS(&ids[slot], -1, it);
    if (prev == -1 || prev == it) atomicAdd(&cnt[slot], 1u);
    else atomicAdd(&item_cnt[it], 1ull);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < HIST_SLOTS; i += 1024)
    if (ids[i] >= 0 && cnt[i] > 0) atomicAdd(&item_cnt[ids[i]], static_cast<unsigned long long>(cnt[i]));
}

// Catalogues whose counters fit one CU's LDS (n_items <= 36,864; ML-20M: 26,744): a direct table per
// workgroup - one LDS atomic per entry, no tags, no collisions (the hashed table above sends every
// collision to a hot global address: 109 us for the 2.8 M entries of an ML-20M call, this form 12).
__global__ __launch_bounds__(1024) void item_hist_direct_kernel(const int32_t *__restrict__ rec, int64_t n,
                                                                int32_t n_items,
                                                                unsigned long long *__restrict__ item_cnt) {
  extern __shared__ uint32_t hist_cnt[];
  for (int i = threadIdx.x; i < n_items; i += 1024) hist_cnt[i] = 0u;
  __syncthreads();
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t b = per * blockIdx.x, e = min(b + per, n);
  for (int64_t i = b + threadIdx.x; i < e; i += 1024) {
    const int32_t it = rec[i];
    if (it >= 0 && it < n_items) atomicAdd(&hist_cnt[it], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_items; i += 1024) {
    const uint32_t c = hist_cnt[i];
    if (c) atomicAdd(&item_cnt[i], static_cast<unsigned long long>(c));
  }
}

// scores[row, col] = -inf for the stored entries of the mask rows (evaluator.py:426-432)
// (`n_items` = row stride = number of leading items the block holds: entries beyond are skipped)
// (`row_list`, when given: score row r is masked with the mask row row_list[r])
__global__ void mask_rows_kernel(float *scores, int64_t rows, int64_t n_items,
                                 const int64_t *mask_ptr, const int32_t *mask_idx,
                                 const int32_t *row_list = nullptr) {
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  const int64_t mrow = row_list ? row_list[row] : row;
  for (int64_t q = mask_ptr[mrow] + threadIdx.x; q < mask_ptr[mrow + 1]; q += blockDim.x) {
    const int32_t j = mask_idx[q];
    if (j < n_items) scores[row * n_items + j] = -std::numeric_limits<float>::infinity();
  }
}

// the same for a block of either score type whose mask rows arrive with the call
// (irs_eval_get_metrics_masked): mask_ptr is relative to the first row of the block
template <class T>
__global__ void mask_block_kernel(T *scores, int64_t rows, int64_t n_items,
                                  const int64_t *mask_ptr, const int32_t *mask_idx) {
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  for (int64_t q = mask_ptr[row] + threadIdx.x; q < mask_ptr[row + 1]; q += blockDim.x) {
    const int32_t j = mask_idx[q];
    if (j >= 0 && j < n_items) scores[row * n_items + j] = -std::numeric_limits<T>::infinity();
  }
}

// scores[row, n_scored .. n_items) = -inf: the trailing columns of a block that the model does not score (the
// feature-only items of a cold-user evaluation, evaluator.py:623-634); the score kernels wrote the columns below
// n_scored of the same rows.  One workgroup per row.
template <class T>
__global__ void fill_unscored_kernel(T *scores, int64_t rows, int64_t n_items, int64_t n_scored) {
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  for (int64_t j = n_scored + threadIdx.x; j < n_items; j += blockDim.x)
    scores[row * n_items + j] = -std::numeric_limits<T>::infinity();
}

}  // namespace eval
}  // namespace irs
