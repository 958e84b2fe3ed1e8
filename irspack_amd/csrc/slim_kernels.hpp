// SLIM (elastic-net coordinate descent, cpp_source/util.hpp:228-424) on the item Gram matrix: the
// device kernels of slim.hip.  DESIGN.md section 9 has the design and the measurements.
//
//   gram_rows_kernel      G = X^T X, dense I x I fp32, one wave per row of G (gram_setup.hpp: EASE shares it)
//   slim_descent_kernel   one persistent workgroup per target column; exact Gauss-Seidel in ascending
//                         coordinate order, a chunk of blockDim.x coordinates evaluated at once
//   count / scan / emit   the dense coefficient rows -> CSC arrays (top_k selection by value)
#pragma once
#include "common.hpp"
#include "slim_host_plan.hpp"  // kMaxWaves, kSlotBytes: the LDS layout the launch decision counts with

namespace irs {
namespace slim {

__global__ void gram_diag_kernel(const float *__restrict__ G, int32_t n_items, float *__restrict__ diag) {
  const int f = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (f < n_items) diag[f] = G[static_cast<int64_t>(f) * n_items + f];
}

// --------------------------------------------------------------------------------------------- descent
// One update of a coordinate (util.hpp:300-345 on the Gram matrix): `lin` = q_f - G_fj - G_ff w_f.
template <bool POSITIVE> __device__ __forceinline__ float cd_candidate(float lin, float quad, float l1) {
  const float plus = (-lin - l1) / quad;
  if (plus > 0.f) return plus;
  if (!POSITIVE) {
    const float minus = (-lin + l1) / quad;
    if (minus < 0.f) return minus;
  }
  return 0.f;  // also G_ff + l2 == 0: NaN and -inf fail both tests
}

// Workgroups take target columns off `cursor` (in `order`: most popular first).  State of a column:
// r = G w - G[:, j] (I floats: LDS, or a row of `scratch` when LDS_R is false) and w (row j of the dense
// W, global).  Thread t owns the coordinates t, t + blockDim.x, ...: it alone reads and writes their r
// and w, so no barrier orders those.  A chunk of blockDim.x consecutive coordinates is evaluated at once
// from the current r; every coordinate before the first one whose value changes is final (its update is
// the identity), the first change is applied (r += G[f, :] * delta, the whole workgroup, G symmetric so
// the column is read as a row) and the coordinates behind it are evaluated again.  That is the
// one-at-a-time loop's arithmetic in its order.  One barrier per evaluation: each wave leaves its ballot
// and its first changed lane's delta in an LDS slot (two slot buffers alternate, a wave is never more
// than one evaluation ahead of another).
template <bool POSITIVE, bool LDS_R>
__global__ __launch_bounds__(1024) void slim_descent_kernel(const float *__restrict__ G,
                                                            const float *__restrict__ diag,
                                                            const int32_t *__restrict__ order, int32_t n_items,
                                                            int64_t n_iter, float l2, float l1, float tol,
                                                            float *W, float *scratch, int32_t *cursor,
                                                            unsigned long long *stats) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long *s_ballot = reinterpret_cast<unsigned long long *>(smem);      // [2][kMaxWaves]
  float *s_delta = reinterpret_cast<float *>(smem + 2 * kMaxWaves * 8);               // [2][kMaxWaves]
  int32_t *s_col = reinterpret_cast<int32_t *>(smem + 2 * kMaxWaves * 8 + 2 * kMaxWaves * 4);
  float *r_lds = reinterpret_cast<float *>(smem + kSlotBytes);
  float *r_glb = scratch + static_cast<int64_t>(blockIdx.x) * n_items;
  const int tid = static_cast<int>(threadIdx.x), nthr = static_cast<int>(blockDim.x);
  const int lane = tid & 63, wave = wave_index_in_block(), n_waves = nthr >> 6;
  int par = 0;

  for (;;) {
    if (tid == 0) *s_col = atomicAdd(cursor, 1);
    __syncthreads();
    const int slot = *s_col;
    __syncthreads();
    if (slot >= n_items) return;
    const int j = order[slot];
    const float *Gj = G + static_cast<int64_t>(j) * n_items;
    float *w = W + static_cast<int64_t>(j) * n_items;  // zeroed by the host
    for (int g = tid; g < n_items; g += nthr) {
      if (LDS_R) r_lds[g] = -Gj[g];
      else r_glb[g] = -Gj[g];
    }
    unsigned long long sweeps = 0, updates = 0;
    for (int64_t it = 0; it < n_iter; it++) {
      float sweep_max = 0.f;
      // this thread's coordinate of the chunk at hand and of the next one (loaded a chunk ahead: a
      // chunk's updates touch that chunk's w only)
      float wf = 0.f, df = 0.f, wf_next = 0.f, df_next = 0.f;
      if (tid < n_items) {
        wf_next = w[tid];
        df_next = diag[tid];
      }
      for (int base = 0; base < n_items; base += nthr) {
        const int f = base + tid;
        wf = wf_next;
        df = df_next;
        if (f + nthr < n_items) {
          wf_next = w[f + nthr];
          df_next = diag[f + nthr];
        }
        const bool mine = f < n_items && f != j;
        const float quad = df + l2;
        int lo = 0;  // the chunk's coordinates below lo are final
        for (;;) {
          float wn = wf;
          if (mine && tid >= lo) {
            const float rf = LDS_R ? r_lds[f] : r_glb[f];
            wn = cd_candidate<POSITIVE>(rf - df * wf, quad, l1);
          }
          const bool changed = wn != wf;
          const unsigned long long ballot = __ballot(changed);
          if (lane == 0) s_ballot[par * kMaxWaves + wave] = ballot;
          if (changed && lane == __ffsll(static_cast<long long>(ballot)) - 1)
            s_delta[par * kMaxWaves + wave] = wn - wf;
          __syncthreads();
          int first = -1;
          float delta = 0.f;
          for (int v = 0; v < n_waves; v++) {
            const unsigned long long b = s_ballot[par * kMaxWaves + v];
            if (b != 0) {
              first = v * 64 + __ffsll(static_cast<long long>(b)) - 1;
              delta = s_delta[par * kMaxWaves + v];
              break;
            }
          }
          par ^= 1;
          if (first < 0) break;
          if (tid == first) {
            wf = wn;
            w[f] = wn;
          }
          const float *Gf = G + static_cast<int64_t>(base + first) * n_items;
          if (LDS_R) {
#pragma unroll 8
            for (int g = tid; g < n_items; g += nthr) r_lds[g] += Gf[g] * delta;
          } else {
#pragma unroll 8
            for (int g = tid; g < n_items; g += nthr) r_glb[g] += Gf[g] * delta;
          }
          sweep_max = fmaxf(sweep_max, fabsf(delta));
          updates++;
          lo = first + 1;
        }
      }
      sweeps++;
      if (sweep_max < tol) break;
    }
    if (tid == 0) {
      atomicAdd(&stats[0], sweeps);
      atomicAdd(&stats[1], updates);
    }
  }
}

// ------------------------------------------------------------------------------------------------ emit
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum over the 256 threads of the workgroup (every thread receives it); s_w: 4 ints of LDS
__device__ __forceinline__ int block_sum(int v, int *s_w) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  const int t = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  __syncthreads();
  return t;
}

// exclusive prefix count of `flag` over the 256 threads in thread order, and the total
__device__ __forceinline__ int block_rank(bool flag, int &total, int *s_w) {
  const unsigned long long b = __ballot(flag);
  const int lane = static_cast<int>(threadIdx.x & 63), wave = static_cast<int>(threadIdx.x >> 6);
  const int below = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) s_w[wave] = __popcll(b);
  __syncthreads();
  int off = 0, tot = 0;
  for (int v = 0; v < 4; v++) {
    const int c = s_w[v];
    if (v < wave) off += c;
    tot += c;
  }
  __syncthreads();
  total = tot;
  return off + below;
}

// order-preserving key of a float: a > b  <=>  key(a) > key(b)
__device__ __forceinline__ uint32_t value_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// stored entries of every column: its non-zeros, at most top_k of them when top_k >= 0
__global__ __launch_bounds__(256) void slim_count_kernel(const float *__restrict__ W, int32_t n_items,
                                                         int64_t top_k, int32_t *__restrict__ raw_count,
                                                         int32_t *__restrict__ count) {
  __shared__ int s_w[4];
  const int j = static_cast<int>(blockIdx.x);
  const float *w = W + static_cast<int64_t>(j) * n_items;
  int c = 0;
  for (int g = static_cast<int>(threadIdx.x); g < n_items; g += 256) c += w[g] != 0.f ? 1 : 0;
  c = block_sum(c, s_w);
  if (threadIdx.x == 0) {
    raw_count[j] = c;
    count[j] = (top_k >= 0 && c > top_k) ? static_cast<int32_t>(top_k) : c;
  }
}

// col_ptr[0 .. n] = exclusive prefix sum of count[0 .. n) (one workgroup of 1024 threads)
__global__ __launch_bounds__(1024) void slim_scan_kernel(const int32_t *__restrict__ count, int32_t n,
                                                         int64_t *__restrict__ col_ptr) {
  __shared__ long long s_part[1024];
  const int tid = static_cast<int>(threadIdx.x);
  const int per = (n + 1023) / 1024;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  long long sum = 0;
  for (int i = lo; i < hi; i++) sum += count[i];
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int i = 0; i < 1024; i++) {
      const long long v = s_part[i];
      s_part[i] = run;
      run += v;
    }
    col_ptr[n] = run;
  }
  __syncthreads();
  long long run = s_part[tid];
  for (int i = lo; i < hi; i++) {
    col_ptr[i] = run;
    run += count[i];
  }
}

// Column j of the CSC result from row j of the dense W: the non-zeros in ascending row order.  A column
// with more non-zeros than top_k keeps the top_k largest VALUES (util.hpp:383-392; ties: the lower row
// index): T = the top_k-th largest key by a bit-by-bit search, then everything above T and the first
// entries equal to T.
__global__ __launch_bounds__(256) void slim_emit_kernel(const float *__restrict__ W, int32_t n_items,
                                                        const int32_t *__restrict__ raw_count,
                                                        const int32_t *__restrict__ count,
                                                        const int64_t *__restrict__ col_ptr,
                                                        int32_t *__restrict__ out_idx,
                                                        float *__restrict__ out_val) {
  __shared__ int s_w[4];
  const int j = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const float *w = W + static_cast<int64_t>(j) * n_items;
  const int keep = count[j];
  if (keep == 0) return;
  const bool select = raw_count[j] > keep;
  uint32_t T = 0;
  int eq_quota = 0;
  if (select) {
    for (int bit = 31; bit >= 0; bit--) {
      const uint32_t cand = T | (1u << bit);
      int c = 0;
      for (int g = tid; g < n_items; g += 256) {
        const float v = w[g];
        c += (v != 0.f && value_key(v) >= cand) ? 1 : 0;
      }
      if (block_sum(c, s_w) >= keep) T = cand;
    }
    int c = 0;
    for (int g = tid; g < n_items; g += 256) {
      const float v = w[g];
      c += (v != 0.f && value_key(v) > T) ? 1 : 0;
    }
    eq_quota = keep - block_sum(c, s_w);
  }
  int64_t out = col_ptr[j];
  int eq_seen = 0;
  for (int base = 0; base < n_items; base += 256) {
    const int g = base + tid;
    const float v = g < n_items ? w[g] : 0.f;
    bool take = v != 0.f;
    if (select) {
      const uint32_t key = value_key(v);
      const bool eq = take && key == T;
      int eq_total = 0;
      const int eq_rank = block_rank(eq, eq_total, s_w);
      take = take && (key > T || (eq && eq_seen + eq_rank < eq_quota));
      eq_seen += eq_total;
    }
    int total = 0;
    const int rank = block_rank(take, total, s_w);
    if (take) {
      out_idx[out + rank] = g;
      out_val[out + rank] = v;
    }
    out += total;
  }
}

}  // namespace slim
}  // namespace irs
