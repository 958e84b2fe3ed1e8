// Scores of a SIMILARITY model on the device (round 6): score[u][:] = X[u][:] @ W
// (BaseSimilarityRecommender.get_score_block, base.py:406-429: `X_train_all[begin:end].dot(W)` through
// scipy's row-by-row sparse product).  One wave per (user, tile of SIM_TILE columns): the tile's float64
// sums live in the wave's own LDS slab; the wave walks the user's stored (i, x) in order and, for each,
// the stored entries (j, w) of row i of W, adding x * w to column j when it lies in the tile - product and
// sum rounded separately (__dmul_rn / __dadd_rn), entries of the profile in storage order.  That IS the
// order in which scipy's csr_matmat accumulates `sums[j] += x * w` for a result row, so the block is the
// host product bit for bit (a column gets at most one update per profile entry - W's rows hold distinct
// columns - and LDS operations of one wave execute in order: no atomics, no barriers, no dependence on
// arrival order).  When W's rows hold strictly increasing columns (every recommender of this package) a
// table made per call (sim_tile_ptr_kernel) gives each (row of W, tile) its range of entries, so a tile
// reads a row's entries INSIDE it - one strip, sixteen rows in flight; otherwise every tile re-scans the
// whole rows (two strips, eight rows in flight).
// (Included by evaluator.hip inside its translation unit, before eval_dense_kernels.hpp, which uses readlane_f64.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace irs {
namespace eval {

constexpr int SIM_TILE = 2048;  // columns per wave: 16 KB of LDS, ten waves per CU (4096: 65 ms for the ML-20M model, 2048: 59, 1024: 66)

__device__ __forceinline__ int64_t readlane_i64(int64_t v, int src) {
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(v), src);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32), src);
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}
__device__ __forceinline__ double readlane_f64(double v, int src) {
  return __longlong_as_double(readlane_i64(__double_as_longlong(v), src));
}

// tptr[i * (n_tiles + 1) + t] = first entry of row i of W (columns increasing) whose column is >= t * SIM_TILE
__global__ __launch_bounds__(256) void sim_tile_ptr_kernel(const int64_t *__restrict__ w_ptr,
                                                           const int32_t *__restrict__ w_idx, int64_t n_rows,
                                                           int32_t n_tiles, int32_t *__restrict__ tptr) {
  const int64_t id = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= n_rows * (n_tiles + 1)) return;
  const int64_t i = id / (n_tiles + 1);
  const int32_t t = static_cast<int32_t>(id % (n_tiles + 1));
  int64_t lo = w_ptr[i], hi = w_ptr[i + 1];
  const int64_t bound = static_cast<int64_t>(t) * SIM_TILE;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (w_idx[mid] < bound) lo = mid + 1;
    else hi = mid;
  }
  tptr[id] = static_cast<int32_t>(lo);
}

template <bool TILED>  // TILED: w_tptr given - a row's entries inside the tile are one strip (a second one is not fetched)
__global__ __launch_bounds__(64) void sim_score_kernel(const int64_t *__restrict__ x_ptr, const int32_t *__restrict__ x_idx,
                                                       const double *__restrict__ x_val,  // null: all ones
                                                       const int64_t *__restrict__ w_ptr, const int32_t *__restrict__ w_idx,
                                                       const double *__restrict__ w_val, int64_t w_last, int64_t row0,
                                                       int64_t n_items, int32_t n_tiles, double *__restrict__ out,
                                                       const int32_t *__restrict__ w_tptr,
                                                       const int32_t *__restrict__ order,
                                                       int64_t ld) {  // ld >= n_items: row stride of `out`
  __shared__ double acc[SIM_TILE];
  const int lane = threadIdx.x;
  const int64_t unit = blockIdx.x;
  // row of the block: the rows are LAUNCHED longest profile first (`order`; a wave lasts as long as its
  // user's profile, and a 9,000-item profile at the end of a block was a tail of its own)
  const int64_t r = order[unit / n_tiles];
  const int32_t tile = static_cast<int32_t>(unit % n_tiles);
  const int32_t c0 = tile * SIM_TILE, width = static_cast<int32_t>(min<int64_t>(SIM_TILE, n_items - c0));
  for (int k = lane; k < width; k += 64) acc[k] = 0.0;
  const int64_t qb = x_ptr[row0 + r], qe = x_ptr[row0 + r + 1];
  auto add = [&](int32_t jg, double x, double w) {  // (in program order per wave: LDS operations do not overtake)
    const int32_t j = jg - c0;
    if (static_cast<uint32_t>(j) < static_cast<uint32_t>(width)) acc[j] = __dadd_rn(acc[j], __dmul_rn(x, w));
  };
  // The walk is a chain of dependent loads (profile entry -> row bounds of W -> the row's columns and values):
  // 64 profile entries are fetched at once (one per lane, with their row bounds), and the first 128 entries of
  // the rows of D consecutive profile entries are in flight while an earlier row is added - one exposed round
  // trip per 64 profile entries instead of three per entry (195 -> ~40 ms for the ML-20M model).
  constexpr int D = TILED ? 16 : 8;  // rows in flight (TILED: one strip per row, twice the rows)
  for (int64_t q0 = qb; q0 < qe; q0 += 64) {
    const int64_t q = min(q0 + lane, qe - 1);
    const int32_t i_l = x_idx[q];
    const double x_l = x_val ? x_val[q] : 1.0;
    // (rows of W with increasing columns: only the row's entries INSIDE this tile, from the table
    // sim_tile_ptr_kernel made - a seventh of a row on the ML-20M shape, one strip instead of two)
    int64_t eb_l, ee_l;
    if constexpr (TILED) {
      const int32_t *tp = w_tptr + static_cast<int64_t>(i_l) * (n_tiles + 1) + tile;
      eb_l = tp[0];
      ee_l = tp[1];
    } else {
      eb_l = w_ptr[i_l];
      ee_l = w_ptr[i_l + 1];
    }
    const int n = static_cast<int>(min<int64_t>(64, qe - q0));
    int32_t ja[D], jb[D];
    double wa[D], wb[D];
    auto fetch = [&](int slot, int k) {  // the first two strips of row k (clamped loads, masked when used)
      const int64_t eb = readlane_i64(eb_l, k), ee = readlane_i64(ee_l, k);
      // (unconditional: a load under a branch would drain the queue; w_last = the last valid entry, >= 0)
      const int64_t e0 = min(eb + lane, w_last), e1 = min(eb + 64 + lane, w_last);
      ja[slot] = w_idx[e0];
      wa[slot] = w_val[e0];
      if constexpr (!TILED) {
        jb[slot] = w_idx[e1];
        wb[slot] = w_val[e1];
      }
      (void)ee;
      (void)e1;
    };
#pragma unroll
    for (int d = 0; d < D; d++) fetch(d, min(d, n - 1));
    for (int k0 = 0; k0 < n; k0 += D) {
#pragma unroll
      for (int d = 0; d < D; d++) {
        const int k = k0 + d;
        if (k < n) {  // (wave-uniform)
          const int64_t eb = readlane_i64(eb_l, k), ee = readlane_i64(ee_l, k);
          const double x = readlane_f64(x_l, k);
          const int32_t j0 = ja[d], j1 = TILED ? 0 : jb[d];
          const double w0 = wa[d], w1 = TILED ? 0.0 : wb[d];
          if (k + D < n) fetch(d, k + D);  // (the slot's registers were copied: its next row starts now)
          if (eb + lane < ee) add(j0, x, w0);
          if constexpr (!TILED) {
            if (eb + 64 + lane < ee) add(j1, x, w1);
          }
          // (rows above 128 entries; TILED: more than 64 of a row's entries inside one tile)
          for (int64_t e = eb + (TILED ? 64 : 128) + lane; e < ee; e += 64) add(w_idx[e], x, w_val[e]);
        }
      }
    }
  }
  double *dst = out + r * ld + c0;
  for (int k = lane; k < width; k += 64) dst[k] = acc[k];
}

}  // namespace eval
}  // namespace irs
