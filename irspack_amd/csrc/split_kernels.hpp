// Kernels of the row-wise hold-out split (split.hip; the rule and the row classes: split_host_plan.hpp).
//
//   select   per row with 0 < n_test < m: the threshold key T, the n_test-th smallest key of the row -> thr[row]
//            WAVE class: a wave per row, every lane ranks its entry by counting the smaller pairs of the other lanes;
//            LDS / STREAM class: a workgroup per row, radix select over the 64-bit keys, 8 bits a pass, the histogram
//            of a pass in LDS (integer counts: their sum does not depend on the order of the additions);
//   scan     test_ptr = exclusive scan of n_test(m) over the rows (tile sums, one block over the tiles, tile rescan);
//            train_ptr = indptr - test_ptr;
//   scatter  per entry: held out = key <= T (or all / none of the row); the position inside the output row is the
//            count of entries of the same kind before it in the row (ballot + popcount, wave totals through LDS), so
//            both outputs keep the column order and no atomic decides a position.
// Keys are recomputed from (seed, row, j) wherever they are needed: there is no key array in device memory.
#pragma once
#include "common.hpp"
#include "split_host_plan.hpp"

namespace irs {
namespace split {

constexpr int kWavesPerBlock = kSelectThreads / 64;

__device__ __forceinline__ int lane_id() { return static_cast<int>(threadIdx.x & 63); }

// ---- select, WAVE class: rows of 1 .. 64 entries, one wave each (rows of another class return at once) ------------
__global__ __launch_bounds__(kSelectThreads) void split_select_wave_kernel(const int64_t *__restrict__ indptr,
                                                                           int64_t rows, uint64_t seed, Mode md,
                                                                           uint64_t *__restrict__ thr) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_index_in_block();
  if (row >= rows) return;  // (wave-uniform, like every exit below: all 64 lanes reach the shuffles)
  const int64_t m = indptr[row + 1] - indptr[row];
  if (m <= 0 || m > kWaveMax) return;
  const int64_t n = n_test_of(m, md);
  if (n <= 0 || n >= m) return;
  const int lane = lane_id();
  const uint64_t key = entry_key(row_key(seed, row), lane);  // lanes >= m hold a key nobody counts
  int rank = 0;
  for (int i = 0; i < static_cast<int>(m); i++) {
    const uint64_t other = __shfl(key, i, 64);
    rank += (other < key || (other == key && i < lane)) ? 1 : 0;
  }
  if (lane < m && rank == n - 1) thr[row] = key;
}

// ---- select, LDS and STREAM classes: one workgroup per listed row ------------------------------------------------
template <bool LDS_KEYS>
__global__ __launch_bounds__(kSelectThreads) void split_select_block_kernel(const int64_t *__restrict__ indptr,
                                                                            const int32_t *__restrict__ select_rows,
                                                                            uint64_t seed, Mode md,
                                                                            uint64_t *__restrict__ thr) {
  __shared__ uint64_t keys[LDS_KEYS ? kLdsMax : 1];
  __shared__ uint32_t hist[kRadixBins];
  __shared__ uint32_t wave_sum[kWavesPerBlock];
  __shared__ uint64_t s_prefix;
  __shared__ uint32_t s_k;
  const int64_t row = select_rows[blockIdx.x];
  const int64_t m = indptr[row + 1] - indptr[row];
  const int tid = static_cast<int>(threadIdx.x), lane = lane_id(), wave = wave_index_in_block();
  const uint64_t rk = row_key(seed, row);
  if (LDS_KEYS) {
    if (m > kLdsMax) return;  // (the plan never lists such a row here; the key image must not be overrun)
    for (int64_t j = tid; j < m; j += kSelectThreads) keys[j] = entry_key(rk, j);
  }
  uint32_t k = static_cast<uint32_t>(n_test_of(m, md) - 1);  // rank sought among the entries that share the prefix
  uint64_t prefix = 0;                                        // the bits of T decided so far
  for (int pass = 0; pass < kRadixPasses; pass++) {
    const int shift = 64 - kRadixBits * (pass + 1);
    hist[tid] = 0;
    __syncthreads();  // (pass 0: the key image is complete as well)
    for (int64_t j = tid; j < m; j += kSelectThreads) {
      const uint64_t key = LDS_KEYS ? keys[j] : entry_key(rk, j);
      if (pass == 0 || (key >> (shift + kRadixBits)) == prefix)
        atomicAdd(&hist[static_cast<uint32_t>(key >> shift) & (kRadixBins - 1)], 1u);
    }
    __syncthreads();
    // exclusive scan of the 256 bins, thread t on bin t; the bin that holds rank k extends the prefix
    const uint32_t c = hist[tid];
    uint32_t incl = c;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t excl = incl - c;
    for (int w = 0; w < wave; w++) excl += wave_sum[w];
    if (c > 0 && k >= excl && k - excl < c) {  // exactly one bin
      s_prefix = (prefix << kRadixBits) | static_cast<uint64_t>(tid);
      s_k = k - excl;
    }
    __syncthreads();
    prefix = s_prefix;
    k = s_k;
  }
  if (tid == 0) thr[row] = prefix;
}

// ---- scan --------------------------------------------------------------------------------------------------------
// Item r of the scan is row r for r < rows and an item of count 0 for r == rows, so that ptr[rows] is the total.
__device__ __forceinline__ int64_t scan_count(const int64_t *__restrict__ indptr, int64_t rows, int64_t r,
                                              const Mode &md) {
  return r < rows ? n_test_of(indptr[r + 1] - indptr[r], md) : 0;
}

// exclusive scan of one int64 per thread over the workgroup (kScanThreads threads); *total: the workgroup's sum
__device__ __forceinline__ int64_t block_exclusive_scan(int64_t v, int64_t *wave_tot /* LDS, kWavesPerBlock */,
                                                        int64_t *total) {
  const int lane = lane_id(), wave = wave_index_in_block();
  int64_t incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  __syncthreads();  // (the previous use of wave_tot has been read)
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  int64_t excl = incl - v, all = 0;
  for (int w = 0; w < kWavesPerBlock; w++) {
    if (w < wave) excl += wave_tot[w];
    all += wave_tot[w];
  }
  *total = all;
  return excl;
}
static_assert(kScanThreads == kSelectThreads, "block_exclusive_scan assumes kWavesPerBlock waves");

__global__ __launch_bounds__(kScanThreads) void split_tile_sums_kernel(const int64_t *__restrict__ indptr, int64_t rows,
                                                                       Mode md, int64_t *__restrict__ tile_sum) {
  __shared__ int64_t wave_tot[kWavesPerBlock];
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kScanTile + static_cast<int64_t>(threadIdx.x) * kScanRowsPerThread;
  int64_t mine = 0;
  for (int q = 0; q < kScanRowsPerThread; q++)
    if (first + q <= rows) mine += scan_count(indptr, rows, first + q, md);
  int64_t total;
  (void)block_exclusive_scan(mine, wave_tot, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: tile_sum becomes its own exclusive scan
__global__ __launch_bounds__(kScanThreads) void split_scan_tiles_kernel(int64_t *__restrict__ tile_sum, int64_t n_tiles) {
  __shared__ int64_t wave_tot[kWavesPerBlock];
  int64_t carry = 0;
  for (int64_t base = 0; base < n_tiles; base += kScanThreads) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = i < n_tiles ? tile_sum[i] : 0;
    int64_t total;
    const int64_t excl = block_exclusive_scan(v, wave_tot, &total);
    if (i < n_tiles) tile_sum[i] = carry + excl;
    carry += total;
  }
}

__global__ __launch_bounds__(kScanThreads) void split_row_ptr_kernel(const int64_t *__restrict__ indptr, int64_t rows,
                                                                     Mode md, const int64_t *__restrict__ tile_off,
                                                                     int64_t *__restrict__ train_ptr,
                                                                     int64_t *__restrict__ test_ptr) {
  __shared__ int64_t wave_tot[kWavesPerBlock];
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kScanTile + static_cast<int64_t>(threadIdx.x) * kScanRowsPerThread;
  int64_t cnt[kScanRowsPerThread], mine = 0;
#pragma unroll
  for (int q = 0; q < kScanRowsPerThread; q++) {
    cnt[q] = first + q <= rows ? scan_count(indptr, rows, first + q, md) : 0;
    mine += cnt[q];
  }
  int64_t total;
  int64_t at = tile_off[blockIdx.x] + block_exclusive_scan(mine, wave_tot, &total);
#pragma unroll
  for (int q = 0; q < kScanRowsPerThread; q++) {
    const int64_t r = first + q;
    if (r <= rows) {
      test_ptr[r] = at;
      train_ptr[r] = indptr[r] - at;
    }
    at += cnt[q];
  }
}

// ---- scatter -----------------------------------------------------------------------------------------------------
// out_indices / out_data hold the train matrix's entries first, the test matrix's behind them (at nnz_train).
__device__ __forceinline__ bool is_held_out(int64_t j, int64_t m, int64_t n, uint64_t rk, uint64_t T) {
  if (n >= m) return true;
  if (n <= 0) return false;
  return entry_key(rk, j) <= T;
}

template <class E>
__global__ __launch_bounds__(kSelectThreads) void split_scatter_wave_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const E *__restrict__ data, int64_t rows,
    uint64_t seed, Mode md, const uint64_t *__restrict__ thr, const int64_t *__restrict__ test_ptr,
    int32_t *__restrict__ out_indices, E *__restrict__ out_data) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_index_in_block();
  if (row >= rows) return;
  const int64_t begin = indptr[row], m = indptr[row + 1] - begin;
  if (m <= 0 || m > kWaveMax) return;
  const int64_t n = n_test_of(m, md);
  const int64_t nnz_train = indptr[rows] - test_ptr[rows];
  const int64_t test_at = test_ptr[row], train_at = begin - test_at;
  const uint64_t T = (n > 0 && n < m) ? thr[row] : 0;
  const int lane = lane_id();
  const bool in = lane < m;
  const bool held = in && is_held_out(lane, m, n, row_key(seed, row), T);
  const unsigned long long mask = __ballot(held);
  const int before = __popcll(mask & ((1ull << lane) - 1ull));
  if (in) {
    const int64_t dst = held ? nnz_train + test_at + before : train_at + lane - before;
    if (dst >= 0 && dst < indptr[rows]) {  // (always, while thr[row] is the row's n-th key; never a store outside)
      out_indices[dst] = indices[begin + lane];
      out_data[dst] = data[begin + lane];
    }
  }
}

template <class E>
__global__ __launch_bounds__(kSelectThreads) void split_scatter_block_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const E *__restrict__ data, int64_t rows,
    const int32_t *__restrict__ long_rows, uint64_t seed, Mode md, const uint64_t *__restrict__ thr,
    const int64_t *__restrict__ test_ptr, int32_t *__restrict__ out_indices, E *__restrict__ out_data) {
  __shared__ int wave_cnt[2][kWavesPerBlock];
  const int64_t row = long_rows[blockIdx.x];
  const int64_t begin = indptr[row], m = indptr[row + 1] - begin;
  const int64_t n = n_test_of(m, md);
  const int64_t nnz_train = indptr[rows] - test_ptr[rows];
  const int64_t test_at = test_ptr[row], train_at = begin - test_at;
  const uint64_t T = (n > 0 && n < m) ? thr[row] : 0;
  const uint64_t rk = row_key(seed, row);
  const int tid = static_cast<int>(threadIdx.x), lane = lane_id(), wave = wave_index_in_block();
  int64_t run = 0;  // held-out entries of the row in front of this chunk
  int buf = 0;
  for (int64_t base = 0; base < m; base += kSelectThreads, buf ^= 1) {
    const int64_t j = base + tid;
    const bool in = j < m;
    const bool held = in && is_held_out(j, m, n, rk, T);
    const unsigned long long mask = __ballot(held);
    int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[buf][wave] = __popcll(mask);
    __syncthreads();  // (the other buffer is written next: its readers of the chunk before have passed this barrier)
    int chunk = 0;
    for (int w = 0; w < kWavesPerBlock; w++) {
      const int c = wave_cnt[buf][w];
      if (w < wave) before += c;
      chunk += c;
    }
    if (in) {
      const int64_t dst = held ? nnz_train + test_at + run + before : train_at + j - (run + before);
      if (dst >= 0 && dst < indptr[rows]) {  // (always, while thr[row] is the row's n-th key; never a store outside)
        out_indices[dst] = indices[begin + j];
        out_data[dst] = data[begin + j];
      }
    }
    run += chunk;
  }
}

}  // namespace split
}  // namespace irs
