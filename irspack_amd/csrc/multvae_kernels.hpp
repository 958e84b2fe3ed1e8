// Kernels of the Mult-VAE trainer (multvae.hip).
//
// The parameters live in one float32 arena of four segments, each a weight table with its bias as one more row
// (multvae_host_prep.hpp); the activations h1, z, h2 carry a ones column.  The dense products of a step are one
// template (mv_gemm_kernel: fp32-input MFMA, LDS tiles, zero-padded edges) - but for the two small products
// that make activations, which sum in double (mv_forward_dense_kernel); the two products whose K is long
// against their output (d[W4; b4] over the batch, dh2 over the items) are split into K-slabs whose partials
// mv_reduce_slabs_kernel adds in slab order.  The two sparse products are one workgroup per batch row; the
// gradient of W1 is summed in 64-bit fixed point with integer atomics (BPR's idiom), so no sum of a step depends
// on the order of arrival.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "multvae_host_prep.hpp"

namespace irs {
namespace mv {

constexpr int BLOCK = 256;

// the sum of v over the workgroup's BLOCK threads as a fixed tree through `red` (BLOCK values); every thread
// gets it
template <class T> __device__ __forceinline__ T block_sum(T v, T *red) {
  const int tid = static_cast<int>(threadIdx.x);
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const T out = red[0];
  __syncthreads();
  return out;
}
__device__ __forceinline__ float block_max(float v, float *red) {
  const int tid = static_cast<int>(threadIdx.x);
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  const float out = red[0];
  __syncthreads();
  return out;
}

// positions [first, first + count) of an epoch -> users
__global__ void __launch_bounds__(BLOCK)
mv_order_kernel(bpr::Perm perm, int64_t first, int32_t count, int32_t *__restrict__ users) {
  const int32_t t = static_cast<int32_t>(blockIdx.x) * BLOCK + static_cast<int32_t>(threadIdx.x);
  if (t >= count) return;
  users[t] = static_cast<int32_t>(bpr::permute(perm, static_cast<uint32_t>(first + t)));
}

// the noise of one update written out (irs_multvae_noise): one workgroup per row
__global__ void __launch_bounds__(BLOCK)
mv_noise_kernel(uint64_t keep_key, uint64_t eps_key, uint32_t threshold, int32_t L, const int32_t *__restrict__ users,
                const int32_t *__restrict__ indptr, const int32_t *__restrict__ keep_ptr, uint8_t *__restrict__ keep,
                float *__restrict__ eps) {
  const int r = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const uint32_t u = static_cast<uint32_t>(users[r]);
  const int32_t deg = indptr[u + 1] - indptr[u];
  if (keep != nullptr)
    for (int32_t q = tid; q < deg; q += BLOCK)
      keep[keep_ptr[r] + q] = keep_entry(keep_key, u, static_cast<uint32_t>(q), threshold) ? 1 : 0;
  if (eps != nullptr)
    for (int32_t l = tid; l < L; l += BLOCK) eps[static_cast<int64_t>(r) * L + l] = gauss(eps_key, u, static_cast<uint32_t>(l));
}

// what the two sparse kernels know about the rows of a batch and their dropout
struct SparseRows {
  const int32_t *rows;     // user of batch row r (nullptr: r itself)
  const int32_t *indptr;   // CSR of the matrix the rows are taken from
  const int32_t *indices;
  const float *data;
  const uint8_t *keep;     // the caller's dropout, one byte per stored entry of the batch (nullptr: hashed)
  const int32_t *keep_ptr; // where row r's bytes begin
  uint64_t keep_key;
  uint32_t threshold;      // 0: every entry stays
};
__device__ __forceinline__ bool row_keeps(const SparseRows &x, int r, uint32_t u, int32_t position) {
  if (x.keep != nullptr) return x.keep[x.keep_ptr[r] + position] != 0;
  return x.threshold == 0u || keep_entry(x.keep_key, u, static_cast<uint32_t>(position), x.threshold);
}

// h1 = tanh(xd W1 + b1) of one batch row per workgroup, xd = x keep / (sqrt(sum x^2 + 1e-8) (1 - p)).  G lanes
// serve one stored entry (a float4 of W1's row per lane and pass, NCH passes), the 256 / G groups take interleaved
// entries, and their partial rows are added through LDS in group order.  The sums and the tanh are in double (the
// kernel waits for its gathers): h1 carries one rounding, which matters where a pre-activation nearly cancels.  The
// row's scale goes to `rowscale` for the backward kernel.
template <int NCH>
__global__ void __launch_bounds__(BLOCK)
mv_encode_input_kernel(SparseRows x, int32_t H, int32_t Hp, int32_t G, int64_t n_items, const float *__restrict__ W1b,
                       float inv_keep_p, float *__restrict__ h1a, float *__restrict__ rowscale) {
  __shared__ double part[1024 * NCH];
  __shared__ double red[BLOCK];
  const int r = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const uint32_t u = static_cast<uint32_t>(x.rows ? x.rows[r] : r);
  const int32_t b = x.indptr[u], e = x.indptr[u + 1];
  double ss = 0.0;
  for (int32_t q = b + tid; q < e; q += BLOCK) ss += static_cast<double>(x.data[q]) * static_cast<double>(x.data[q]);
  ss = block_sum(ss, red);
  const float s = static_cast<float>(1.0 / sqrt(ss + 1e-8)) * inv_keep_p;
  const int g = tid / G, lane = tid % G, NG = BLOCK / G, nchunk = Hp / 4;
  double acc[NCH][4];
#pragma unroll
  for (int h = 0; h < NCH; h++) acc[h][0] = acc[h][1] = acc[h][2] = acc[h][3] = 0.0;
  for (int32_t q = b + g; q < e; q += NG) {
    if (!row_keeps(x, r, u, q - b)) continue;
    const double v = static_cast<double>(x.data[q] * s);  // (xd as the backward kernel forms it)
    const float4 *w = reinterpret_cast<const float4 *>(W1b + static_cast<int64_t>(x.indices[q]) * Hp);
#pragma unroll
    for (int h = 0; h < NCH; h++) {
      const int c = lane + h * G;
      if (c < nchunk) {
        const float4 wv = w[c];
        acc[h][0] += v * wv.x, acc[h][1] += v * wv.y, acc[h][2] += v * wv.z, acc[h][3] += v * wv.w;
      }
    }
  }
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    const int c = lane + h * G;
    if (c < nchunk) {
      double *to = part + g * Hp + 4 * c;
      to[0] = acc[h][0], to[1] = acc[h][1], to[2] = acc[h][2], to[3] = acc[h][3];
    }
  }
  __syncthreads();
  const float *b1 = W1b + n_items * Hp;
  for (int h = tid; h < H; h += BLOCK) {
    double a = static_cast<double>(b1[h]);
    for (int k = 0; k < NG; k++) a += part[k * Hp + h];
    h1a[static_cast<int64_t>(r) * (H + 1) + h] = static_cast<float>(tanh(a));
  }
  if (tid == 0) {
    h1a[static_cast<int64_t>(r) * (H + 1) + H] = 1.f;
    rowscale[r] = s;
  }
}

__device__ __forceinline__ void add_fixed(unsigned long long *acc, double c, double scale, bool &bad) {
  bad |= !(fabs(c) < static_cast<double>(CONTRIB_CAP));
  const long long q = __double2ll_rn(c * scale);
  atomicAdd(acc, static_cast<unsigned long long>(q));
}

// d[W1; b1] += xd^T da1 of one batch row per workgroup, into the fixed-point sums: a row of the accumulator holds
// its Hp values as [4][Hp / 4] (component e of float4 chunk c at e Hp / 4 + c), so the lanes of one atomic
// instruction address consecutive 8-byte words.  The entry after the row's last is the bias row with xd = 1.
template <int NCH>
__global__ void __launch_bounds__(BLOCK)
mv_dw1_kernel(SparseRows x, int32_t Hp, int32_t G, int64_t n_items, const float *__restrict__ da1,
              const float *__restrict__ rowscale, unsigned long long *__restrict__ acc, double scale,
              int32_t *__restrict__ diverged) {
  const int r = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const uint32_t u = static_cast<uint32_t>(x.rows ? x.rows[r] : r);
  const int32_t b = x.indptr[u], e = x.indptr[u + 1];
  const float s = rowscale[r];
  const int g = tid / G, lane = tid % G, NG = BLOCK / G, nchunk = Hp / 4;
  float4 d[NCH];
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    const int c = lane + h * G;
    d[h] = c < nchunk ? reinterpret_cast<const float4 *>(da1 + static_cast<int64_t>(r) * Hp)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  bool bad = false;
  for (int32_t q = b + g; q <= e; q += NG) {
    double v = 1.0;
    int64_t i = n_items;
    if (q < e) {
      if (!row_keeps(x, r, u, q - b)) continue;
      v = static_cast<double>(x.data[q] * s);
      i = x.indices[q];
    }
    unsigned long long *a = acc + i * Hp;
#pragma unroll
    for (int h = 0; h < NCH; h++) {
      const int c = lane + h * G;
      if (c >= nchunk) continue;
      add_fixed(a + c, v * d[h].x, scale, bad);
      add_fixed(a + nchunk + c, v * d[h].y, scale, bad);
      add_fixed(a + 2 * nchunk + c, v * d[h].z, scale, bad);
      add_fixed(a + 3 * nchunk + c, v * d[h].w, scale, bad);
    }
  }
  if (bad) *diverged = 1;
}

// ---- the dense products ---------------------------------------------------------------------------------------
enum Epilogue { EPI_NONE = 0, EPI_TANH = 1, EPI_DTANH = 2 };
constexpr int BM = 128, BN = 128, BK = 16, LDT = BM + 4;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// C[M, N] = op(A)[M, K] op(B)[K, N] over k in [z slab, min(K, (z + 1) slab)), z = blockIdx.z, written at
// C + z c_slab_stride.  TA: A is stored [K, M] (M contiguous), else [M, K]; TB: B is stored [N, K], else [K, N].
// A 128 x 128 tile per workgroup, 64 x 64 (2 x 2 MFMA tiles of 32 x 32, mfma_f32_32x32x2f32) per wave, K in steps
// of 16 through LDS held k-major, the next step's global loads in flight under this step's MFMAs.  Rows, columns
// and k beyond the edges are read as zero and not written.  An f32 MFMA is a k-ordered fma chain, so the bytes
// of C depend on the tiling alone.  EPI_DTANH: the sum times 1 - aux^2.
template <bool TA, bool TB, int EPI>
__global__ void __launch_bounds__(BLOCK)
mv_gemm_kernel(int32_t M, int32_t N, int32_t K, const float *__restrict__ A, int64_t lda, const float *__restrict__ B,
               int64_t ldb, float *__restrict__ C, int64_t ldc, const float *__restrict__ aux, int64_t ldaux,
               int32_t slab, int64_t c_slab_stride) {
  __shared__ float As[BK * LDT];
  __shared__ float Bs[BK * LDT];
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = wave_index_in_block();
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = static_cast<int64_t>(blockIdx.y) * BM, n0 = static_cast<int64_t>(blockIdx.x) * BN;
  const int32_t k_begin = static_cast<int32_t>(blockIdx.z) * slab;
  const int32_t k_end = K - k_begin < slab ? K : k_begin + slab;
  float ra[8], rb[8];
  auto load = [&](int32_t k0) {
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int idx = tid + e * BLOCK;
      {
        const int kk = TA ? idx / BM : idx % BK, mm = TA ? idx % BM : idx / BK;
        const int64_t m = m0 + mm, k = k0 + kk;
        ra[e] = (m < M && k < k_end) ? (TA ? A[k * lda + m] : A[m * lda + k]) : 0.f;
      }
      {
        const int kk = TB ? idx % BK : idx / BN, nn = TB ? idx / BK : idx % BN;
        const int64_t n = n0 + nn, k = k0 + kk;
        rb[e] = (n < N && k < k_end) ? (TB ? B[n * ldb + k] : B[k * ldb + n]) : 0.f;
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int idx = tid + e * BLOCK;
      As[(TA ? idx / BM : idx % BK) * LDT + (TA ? idx % BM : idx / BK)] = ra[e];
      Bs[(TB ? idx % BK : idx / BN) * LDT + (TB ? idx / BK : idx % BN)] = rb[e];
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int q = 0; q < 16; q++) acc[a][b][q] = 0.f;
  load(k_begin);
  for (int32_t k0 = k_begin; k0 < k_end; k0 += BK) {
    stage();
    __syncthreads();
    if (k0 + BK < k_end) load(k0 + BK);
    const float *ap = As + (lane >> 5) * LDT + wm * 64 + (lane & 31);
    const float *bp = Bs + (lane >> 5) * LDT + wn * 64 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const float a0 = ap[kk * LDT], a1 = ap[kk * LDT + 32], b0 = bp[kk * LDT], b1 = bp[kk * LDT + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  float *Cz = C + static_cast<int64_t>(blockIdx.z) * c_slab_stride;
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const int64_t col = n0 + wn * 64 + b * 32 + (lane & 31);
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const int64_t row = m0 + wm * 64 + a * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (row < M && col < N) {
          float v = acc[a][b][q];
          if (EPI == EPI_DTANH) {
            const float h = aux[row * ldaux + col];
            v *= 1.f - h * h;
          }
          Cz[row * ldc + col] = v;
        }
      }
    }
}

// The two small products of the forward pass, [mu | lv] = [h1 | 1] [W2; b2] and h2 = tanh([z | 1] [W3; b3])
// (0.1 % of a step's flops): C[M, N] = A[M, K] B[K, N], both row-major, one output per thread, 16 x 16 outputs per
// workgroup, K in steps of 16 through LDS, the sum (in k order) and the tanh in double.  Their outputs are the
// activations that multiply whole rows of the weight gradients, so they carry one rounding each.
template <int EPI>
__global__ void __launch_bounds__(BLOCK)
mv_forward_dense_kernel(int32_t M, int32_t N, int32_t K, const float *__restrict__ A, int64_t lda,
                        const float *__restrict__ B, int64_t ldb, float *__restrict__ C, int64_t ldc) {
  __shared__ float As[16][17];
  __shared__ float Bs[16][17];
  const int tx = static_cast<int>(threadIdx.x) & 15, ty = static_cast<int>(threadIdx.x) >> 4;
  const int64_t row = static_cast<int64_t>(blockIdx.y) * 16 + ty, col = static_cast<int64_t>(blockIdx.x) * 16 + tx;
  double acc = 0.0;
  for (int32_t k0 = 0; k0 < K; k0 += 16) {
    As[ty][tx] = (row < M && k0 + tx < K) ? A[row * lda + k0 + tx] : 0.f;
    Bs[ty][tx] = (k0 + ty < K && col < N) ? B[(k0 + ty) * ldb + col] : 0.f;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) acc += static_cast<double>(As[ty][k]) * static_cast<double>(Bs[k][tx]);
    __syncthreads();
  }
  if (row < M && col < N) C[row * ldc + col] = static_cast<float>(EPI == EPI_TANH ? tanh(acc) : acc);
}

// C[M, N] = the n_slabs partial products at part + z stride, added in slab order, then the epilogue
template <int EPI>
__global__ void __launch_bounds__(BLOCK)
mv_reduce_slabs_kernel(int64_t count, int32_t N, int32_t n_slabs, const float *__restrict__ part, int64_t stride,
                       float *__restrict__ C, int64_t ldc, const float *__restrict__ aux, int64_t ldaux) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (idx >= count) return;
  const int64_t row = idx / N, col = idx % N;
  float v = part[idx];
  for (int z = 1; z < n_slabs; z++) v += part[z * stride + idx];
  if (EPI == EPI_DTANH) {
    const float h = aux[row * ldaux + col];
    v *= 1.f - h * h;
  }
  C[row * ldc + col] = v;
}

// ---- softmax, latent, loss, Adam ---------------------------------------------------------------------------------
enum SoftmaxMode { SM_GRADIENT = 0, SM_LOG_SOFTMAX = 1, SM_LSE_ONLY = 2 };

// One row of the [n, I] block per workgroup: the row's max, its log-sum-exp (the sum in double, a fixed tree) and
// NLL = lse sum(x) - sum(x logit) over the row's stored raw values; then, by mode, g = (softmax sum(x) - x) / n
// in place of the logits (the stored entries are subtracted after the pass over the row), the log-softmax in
// place, or nothing.
__global__ void __launch_bounds__(BLOCK)
mv_softmax_kernel(SparseRows x, int64_t n_items, float *__restrict__ block, float inv_n, int mode,
                  double *__restrict__ row_nll, float *__restrict__ row_lse) {
  __shared__ double red[BLOCK];
  __shared__ float redf[BLOCK];
  const int r = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const uint32_t u = static_cast<uint32_t>(x.rows ? x.rows[r] : r);
  const int32_t b = x.indptr[u], e = x.indptr[u + 1];
  float *row = block + static_cast<int64_t>(r) * n_items;
  float mx = -INFINITY;
  for (int64_t i = tid; i < n_items; i += BLOCK) mx = fmaxf(mx, row[i]);
  mx = block_max(mx, redf);
  double se = 0.0;
  for (int64_t i = tid; i < n_items; i += BLOCK) se += static_cast<double>(expf(row[i] - mx));
  se = block_sum(se, red);
  const double lse = static_cast<double>(mx) + log(se);
  const float lse_f = static_cast<float>(lse);
  double sx = 0.0, sxl = 0.0;
  for (int32_t q = b + tid; q < e; q += BLOCK) {
    sx += static_cast<double>(x.data[q]);
    sxl += static_cast<double>(x.data[q]) * static_cast<double>(row[x.indices[q]]);
  }
  sx = block_sum(sx, red);
  sxl = block_sum(sxl, red);
  if (tid == 0) {
    if (row_nll) row_nll[r] = lse * sx - sxl;
    if (row_lse) row_lse[r] = lse_f;
  }
  if (mode == SM_LSE_ONLY) return;
  if (mode == SM_LOG_SOFTMAX) {
    for (int64_t i = tid; i < n_items; i += BLOCK) row[i] -= lse_f;
    return;
  }
  const float sx_f = static_cast<float>(sx);
  for (int64_t i = tid; i < n_items; i += BLOCK) row[i] = expf(row[i] - lse_f) * sx_f * inv_n;
  __syncthreads();
  for (int32_t q = b + tid; q < e; q += BLOCK) row[x.indices[q]] -= x.data[q] * inv_n;
}

// std = exp(lv / 2), z = mu + eps std (evaluation: z = mu), the row's KL sum, and the ones columns of z and h2
__global__ void __launch_bounds__(BLOCK)
mv_latent_forward_kernel(int32_t L, int32_t Hd, const int32_t *__restrict__ rows, const float *__restrict__ ml,
                         uint64_t eps_key, const float *__restrict__ eps_in, int evaluate, float *__restrict__ za,
                         float *__restrict__ h2a, float *__restrict__ stdv, float *__restrict__ epsv,
                         double *__restrict__ row_kl) {
  __shared__ double red[BLOCK];
  const int r = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const uint32_t u = static_cast<uint32_t>(rows ? rows[r] : r);
  const float *m = ml + static_cast<int64_t>(r) * 2 * L;
  double kl = 0.0;
  for (int32_t l = tid; l < L; l += BLOCK) {
    const float mu = m[l], lv = m[L + l], sd = static_cast<float>(exp(0.5 * static_cast<double>(lv)));
    float ep = 0.f;
    if (!evaluate) ep = eps_in ? eps_in[static_cast<int64_t>(r) * L + l] : gauss(eps_key, u, static_cast<uint32_t>(l));
    za[static_cast<int64_t>(r) * (L + 1) + l] = static_cast<float>(static_cast<double>(mu) + static_cast<double>(ep) * sd);
    stdv[static_cast<int64_t>(r) * L + l] = sd, epsv[static_cast<int64_t>(r) * L + l] = ep;
    kl += 0.5 * (-static_cast<double>(lv) + static_cast<double>(sd) * sd + static_cast<double>(mu) * mu - 1.0);
  }
  kl = block_sum(kl, red);
  if (tid == 0) {
    row_kl[r] = kl;
    za[static_cast<int64_t>(r) * (L + 1) + L] = 1.f;
    h2a[static_cast<int64_t>(r) * (Hd + 1) + Hd] = 1.f;
  }
}

// dmu = dz + klc mu / n, dlv = dz eps std / 2 + klc (std^2 - 1) / (2 n); one thread per (row, component)
__global__ void __launch_bounds__(BLOCK)
mv_latent_backward_kernel(int64_t count, int32_t L, const float *__restrict__ dz, const float *__restrict__ ml,
                          const float *__restrict__ stdv, const float *__restrict__ epsv, float klc_over_n,
                          float *__restrict__ dml) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (idx >= count) return;
  const int64_t r = idx / L, l = idx % L;
  const float d = dz[idx], sd = stdv[idx], mu = ml[r * 2 * L + l];
  dml[r * 2 * L + l] = fmaf(klc_over_n, mu, d);
  dml[r * 2 * L + L + l] = fmaf(0.5f * klc_over_n, sd * sd - 1.f, 0.5f * d * epsv[idx] * sd);
}

// the two means of the loss over the batch rows, in double, a fixed tree (one workgroup)
__global__ void __launch_bounds__(BLOCK)
mv_loss_kernel(int32_t n, const double *__restrict__ row_nll, const double *__restrict__ row_kl, double *__restrict__ out) {
  __shared__ double red[BLOCK];
  const int tid = static_cast<int>(threadIdx.x);
  double a = 0.0, b = 0.0;
  for (int32_t r = tid; r < n; r += BLOCK) a += row_nll[r], b += row_kl[r];
  a = block_sum(a, red);
  b = block_sum(b, red);
  if (tid == 0) out[0] = a / n, out[1] = b / n;
}

// optax's adam on every element of the arena.  The elements of [W1; b1] take their gradient from the fixed-point
// sums (which are set back to zero) and leave it in G; the others find it in G.
__global__ void __launch_bounds__(BLOCK)
mv_adam_kernel(int64_t total, int64_t w1_count, int32_t Hp, float *__restrict__ theta, float *__restrict__ m,
               float *__restrict__ v, float *__restrict__ G, unsigned long long *__restrict__ acc, double inv_scale,
               float lr, float correction1, float correction2) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (p >= total) return;
  float g;
  if (p < w1_count) {
    const int64_t row = p / Hp;
    const int h = static_cast<int>(p % Hp);
    const int64_t at = row * Hp + (h & 3) * (Hp / 4) + (h >> 2);
    g = static_cast<float>(static_cast<double>(static_cast<long long>(acc[at])) * inv_scale);
    acc[at] = 0ull;
    G[p] = g;
  } else {
    g = G[p];
  }
  const float m1 = 0.9f * m[p] + 0.1f * g, v1 = 0.999f * v[p] + 0.001f * (g * g);
  m[p] = m1, v[p] = v1;
  theta[p] -= lr * (m1 / correction1) / (sqrtf(v1 / correction2) + 1e-8f);
}

}  // namespace mv
}  // namespace irs
