// Device kernels of the randomized truncated SVD (truncsvd.hip): the sparse x
// dense-block product over CSR rows, the Gram matrix of a tall block and the product of a tall block with a
// small square matrix.  Blocks are row-major with row stride ld = l_pad floats, l_pad a multiple of 64; the
// columns past the sketch width are zero and stay zero.  No float atomics; every sum has a fixed order: two
// calls give identical bytes.
#pragma once
#include "chol_tile_kernels.hpp"
#include "common.hpp"

namespace irs {
namespace tsvd {

using ials::f32x4;
using ials::RIDGE_LD;
using ials::RIDGE_NB;
using ials::ridge_acc_pos;
using ials::ridge_mfma_64;
using ials::ridge_tile_of;

// ---------------------------------------------------------------------------------------------- SpMM
// Y[r, :] = sum over the stored entries (j, x) of row r of x * Q[j, :].  One wave per segment of a row (the
// host cuts a row into segments of at most SPMM_SEG entries and hands the longest out first).  A gathered row
// of Q is l_pad * 4 bytes contiguous: LPR lanes take one float4 each (NCH float4 each when the row is wider
// than a wave), so a 256-byte row leaves room for 64 / LPR entries side by side - sub-group s of the wave
// takes the entries s, s + G, s + 2 G, ... of the segment in stored order, four of them in flight per lane,
// and the G partial sums are added by a fixed shuffle tree at the end (G = 2: s0 + s1; G = 4:
// (s0 + s2) + (s1 + s3)).  The index / value block is loaded once per 64 entries, coalesced, and handed
// round with bpermute.  A segment of a split row goes to its slot of `partial`, summed in segment order by
// tsvd_spmm_reduce_kernel; every other row is written straight to Y (a row without entries writes zeros).
constexpr int SPMM_SEG = 1024;

template <int LPR, int NCH>
static __global__ __launch_bounds__(256) void tsvd_spmm_kernel(const int32_t *__restrict__ seg_row,
                                                               const int32_t *__restrict__ seg_begin,
                                                               const int32_t *__restrict__ seg_end,
                                                               const int32_t *__restrict__ seg_slot, int n_seg,
                                                               const int32_t *__restrict__ idx,
                                                               const float *__restrict__ val,
                                                               const float *__restrict__ Q, int l_pad,
                                                               float *__restrict__ Y, float *__restrict__ partial) {
  constexpr int G = 64 / LPR;
  const int s = static_cast<int>(blockIdx.x) * 4 + wave_index_in_block();
  if (s >= n_seg) return;
  const int lane = static_cast<int>(threadIdx.x & 63);
  const int sub = lane / LPR, col = lane % LPR;
  const int lvec = l_pad >> 2;
  const int row = seg_row[s], beg = seg_begin[s], end = seg_end[s], slot = seg_slot[s];
  const float4 *Q4 = reinterpret_cast<const float4 *>(Q);
  bool on[NCH];
  float4 acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    on[c] = col + 64 * c < lvec;
    acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int p = beg; p < end; p += 64) {
    const int cnt = min(64, end - p);
    int my_i = 0;
    float my_v = 0.f;
    if (lane < cnt) {
      my_i = idx[p + lane];
      my_v = val[p + lane];
    }
    for (int e = 0; e < cnt; e += 4 * G) {
      float vv[4];
      float4 q[4][NCH];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        // e is a multiple of 4 G below 64, so j <= 63; an entry past the end of the block is (row 0,
        // value 0): a finite row times zero
        const int j = e + u * G + sub;
        const int ii = __shfl(my_i, j);
        vv[u] = __shfl(my_v, j);
        const float4 *src = Q4 + static_cast<size_t>(ii) * lvec + col;
#pragma unroll
        for (int c = 0; c < NCH; c++)
          if (on[c]) q[u][c] = src[64 * c];
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int c = 0; c < NCH; c++)
          if (on[c]) {
            acc[c].x = fmaf(vv[u], q[u][c].x, acc[c].x);
            acc[c].y = fmaf(vv[u], q[u][c].y, acc[c].y);
            acc[c].z = fmaf(vv[u], q[u][c].z, acc[c].z);
            acc[c].w = fmaf(vv[u], q[u][c].w, acc[c].w);
          }
    }
  }
  if (G > 1) {
#pragma unroll
    for (int off = 32; off >= LPR; off >>= 1) {
      acc[0].x += __shfl_down(acc[0].x, off);
      acc[0].y += __shfl_down(acc[0].y, off);
      acc[0].z += __shfl_down(acc[0].z, off);
      acc[0].w += __shfl_down(acc[0].w, off);
    }
  }
  float4 *dst = reinterpret_cast<float4 *>(slot < 0 ? Y + static_cast<size_t>(row) * l_pad
                                                    : partial + static_cast<size_t>(slot) * l_pad);
  if (sub == 0) {
#pragma unroll
    for (int c = 0; c < NCH; c++)
      if (on[c]) dst[col + 64 * c] = acc[c];
  }
}

// Y[row, :] of split row blockIdx.x = its segments' partial rows added in segment order
static __global__ __launch_bounds__(256) void tsvd_spmm_reduce_kernel(const int32_t *__restrict__ split_row,
                                                                      const int32_t *__restrict__ split_first,
                                                                      const int32_t *__restrict__ split_count,
                                                                      const float *__restrict__ partial, int l_pad,
                                                                      float *__restrict__ Y) {
  const int r = blockIdx.x;
  const int row = split_row[r], first = split_first[r], count = split_count[r];
  for (int c = threadIdx.x; c < l_pad; c += 256) {
    float v = partial[static_cast<size_t>(first) * l_pad + c];
    for (int k = 1; k < count; k++) v += partial[static_cast<size_t>(first + k) * l_pad + c];
    Y[static_cast<size_t>(row) * l_pad + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------- Gram
// The partial sums of G = Y^T Y: lower 64 x 64 tile blockIdx.x over the row slab blockIdx.y (rows_per_slab a
// multiple of 64), on v_mfma_f32_16x16x4_f32, to P[slab][tile][64 x 64].  Rows past n count as zeros.
static __global__ __launch_bounds__(256) void tsvd_gram_kernel(const float *__restrict__ Y, int n, int ld,
                                                               int rows_per_slab, float *__restrict__ P) {
  __shared__ float ya[RIDGE_NB][RIDGE_LD], yb[RIDGE_NB][RIDGE_LD];
  int bi, bj;
  ridge_tile_of(blockIdx.x, bi, bj);
  const int tid = threadIdx.x;
  const int r_begin = blockIdx.y * rows_per_slab, r_end = min(n, r_begin + rows_per_slab);
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = r_begin; r0 < r_end; r0 += RIDGE_NB) {
    for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 256) {
      const int a = e >> 6, b = e & 63, r = r0 + a;
      const float *row = Y + static_cast<size_t>(r) * ld;
      ya[a][b] = r < n ? row[bi * RIDGE_NB + b] : 0.f;
      yb[a][b] = r < n ? row[bj * RIDGE_NB + b] : 0.f;
    }
    __syncthreads();
    // A(a, c) = Y[r0 + c][64 bi + a], B(c, b) = Y[r0 + c][64 bj + b]
    ridge_mfma_64(acc, &ya[0][0], 1, RIDGE_LD, &yb[0][0], 1, RIDGE_LD, RIDGE_NB);
    __syncthreads();
  }
  float *out = P + (static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * (RIDGE_NB * RIDGE_NB);
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int a, b;
        ridge_acc_pos(i, j, q, a, b);
        out[a * RIDGE_NB + b] = acc[i][j][q];
      }
}

// G (ld x ld, both triangles) from the slab partials, added in slab order; a diagonal tile is mirrored from
// its lower half, so G is symmetric to the bit.  Tile blockIdx.x, its rows 4 blockIdx.y .. 4 blockIdx.y + 3:
// one element per thread
static __global__ __launch_bounds__(256) void tsvd_gram_reduce_kernel(const float *__restrict__ P, int n_slab,
                                                                      int n_tile, int ld, float *__restrict__ G) {
  int bi, bj;
  ridge_tile_of(blockIdx.x, bi, bj);
  const int e = static_cast<int>(blockIdx.y) * 256 + static_cast<int>(threadIdx.x);
  const int a = e >> 6, b = e & 63;
  if (bi == bj && b > a) return;
  float v = 0.f;
  for (int s = 0; s < n_slab; s++) v += P[(static_cast<size_t>(s) * n_tile + blockIdx.x) * (RIDGE_NB * RIDGE_NB) + e];
  const int i = bi * RIDGE_NB + a, j = bj * RIDGE_NB + b;
  G[static_cast<size_t>(i) * ld + j] = v;
  G[static_cast<size_t>(j) * ld + i] = v;
}

// G += d I over all ld diagonal entries, d = 1e-5 * trace(G) / l (the trace over the leading l entries, added
// in ascending order): the shifted matrix always has a Cholesky factor, also for a rank-deficient block,
// and the padded diagonal becomes d
static __global__ __launch_bounds__(64) void tsvd_shift_kernel(float *__restrict__ G, int l, int ld) {
  __shared__ float d;
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int j = 0; j < l; j++) t += G[static_cast<size_t>(j) * ld + j];
    d = 1e-5f * t / static_cast<float>(l);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < ld; j += 64) G[static_cast<size_t>(j) * ld + j] += d;
}

// ---------------------------------------------------------------------------------------------- apply
// out = Y M for the 64 rows blockIdx.x and the 64 columns blockIdx.y; M is ld x ld row-major.  TRANS: M = W^T
// of the lower-triangular W handed in (W = L^-1: the tiles above the diagonal are never read, so the inner
// tiles stop at the diagonal).  Both operands go through LDS with the inner index leading.
template <bool TRANS>
static __global__ __launch_bounds__(256) void tsvd_apply_kernel(const float *__restrict__ Y, int n, int ld,
                                                                const float *__restrict__ W,
                                                                float *__restrict__ out) {
  __shared__ float yt[RIDGE_NB][RIDGE_LD], ms[RIDGE_NB][RIDGE_LD];
  const int tid = threadIdx.x, r0 = blockIdx.x * RIDGE_NB, tj = blockIdx.y, nb = ld / RIDGE_NB;
  const int kt_end = TRANS ? tj + 1 : nb;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < kt_end; kt++) {
    for (int e = tid; e < RIDGE_NB * RIDGE_NB; e += 256) {
      const int a = e >> 6, c = e & 63, r = r0 + a;
      yt[c][a] = r < n ? Y[static_cast<size_t>(r) * ld + kt * RIDGE_NB + c] : 0.f;
      if (TRANS)  // M[64 kt + c][64 tj + a] = W[64 tj + a][64 kt + c]
        ms[c][a] = W[static_cast<size_t>(tj * RIDGE_NB + a) * ld + kt * RIDGE_NB + c];
      else  // (here a is the inner index and c the column)
        ms[a][c] = W[static_cast<size_t>(kt * RIDGE_NB + a) * ld + tj * RIDGE_NB + c];
    }
    __syncthreads();
    // A(a, c) = yt[c][a], B(c, b) = ms[c][b]
    ridge_mfma_64(acc, &yt[0][0], 1, RIDGE_LD, &ms[0][0], 1, RIDGE_LD, RIDGE_NB);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int a, b;
        ridge_acc_pos(i, j, q, a, b);
        if (r0 + a < n) out[static_cast<size_t>(r0 + a) * ld + tj * RIDGE_NB + b] = acc[i][j][q];
      }
}

}  // namespace tsvd
}  // namespace irs
