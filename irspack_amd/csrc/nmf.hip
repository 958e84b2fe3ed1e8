// NMFRecommender (nmf.py of the reference: sklearn's NMF, solver "cd", Frobenius loss): the device side of
// utils.nmf_fit and utils.nmf_transform.  DESIGN.md section 12 has the algorithm and the figures.
//
// W (n_users x k) and H^T (n_items x k) live on the device as row-major blocks of row stride k_pad = k rounded
// up to 64 with zero padding, X and X^T as CSR with the segment lists of the truncated SVD's product kernel
// (sparse_block.hpp); the product and the Gram reduce are that kernel family's with their sums in double
// (nmf_kernels.hpp).  One iteration is two half-steps
//     XH = A Ht (SpMM);  G = Ht^T Ht (Gram), G[t, t] += l2;  sweep the rows of W against G and XH - l1
// with (A, W, Ht) = (X, W, H^T) and then (X^T, H^T, W); the violation sums of both sweeps are reduced on the
// device and the host reads one double per iteration for sklearn's stopping test.  With update_H = 0 (transform)
// only the first half-step runs, and its product and Gram matrix, which no iteration changes, are computed once.
// One stream.  Every argument check comes before any device work.
#include <algorithm>
#include <cmath>

#include "csr_checks.hpp"
#include "nmf_kernels.hpp"
#include "phase_spans.hpp"
#include "sparse_block.hpp"
#include "truncsvd_kernels.hpp"

namespace irs {
namespace nmf {

using sblock::Csr;
using tsvd::RIDGE_NB;

enum Phase { PH_SETUP = 0, PH_SPMM, PH_GRAM, PH_SWEEP, PH_D2H, PH_COUNT };

struct Fit {
  int64_t n_users = 0, n_items = 0, nnz = 0, k = 0, k_pad = 0;
  Csr X, Xt;
  DeviceBuffer<float> W, Ht, XH, G, gram_partial, spmm_partial;
  DeviceBuffer<double> partial, violation;
  PhaseSpans<PH_COUNT> spans;  // recording only when the caller asked for the times
};

// X and X^T on the device with their segment lists (synchronises: the transpose's column counts)
static void upload_matrix(Fit &f, const int64_t *indptr, const int32_t *indices, const float *data, hipStream_t s) {
  std::vector<int32_t> h_ptr(static_cast<size_t>(f.n_users) + 1);
  for (int64_t i = 0; i <= f.n_users; i++) h_ptr[i] = static_cast<int32_t>(indptr[i]);
  sblock::upload_with_transpose(h_ptr, indices, data, f.n_users, f.n_items, f.nnz, f.X, f.Xt, f.spmm_partial, f.k_pad,
                                s);
  IRS_HIP(hipStreamSynchronize(s));  // (h_ptr is the source of an asynchronous copy)
}

// out (M.rows x k_pad) = M in (M.cols x k_pad)
static void spmm(Fit &f, const Csr &M, const float *in, float *out, hipStream_t s) {
  auto sp = f.spans.span(PH_SPMM, s);
  const int lp = static_cast<int>(f.k_pad);
  float *partial = f.spmm_partial.ptr;
  sblock::for_spmm_width(lp / 4, [&](auto lpr, auto nch) {
    sblock::launch_spmm(nmf_spmm_kernel<decltype(lpr)::value, decltype(nch)::value>, M, in, lp, out, partial, s);
  });
  sblock::launch_split_reduce(tsvd::tsvd_spmm_reduce_kernel, M, partial, lp, out, s);
  IRS_HIP(hipGetLastError());
  sp.stop();
}

// G (k_pad x k_pad, symmetric) = B^T B for the block B of `rows` rows, then G[t, t] += l2 for t < k
static void gram(Fit &f, const float *B, int64_t rows, float l2, hipStream_t s) {
  auto sp = f.spans.span(PH_GRAM, s);
  const sblock::GramPass pass = sblock::launch_gram_partials(B, rows, f.k_pad, f.gram_partial.ptr, s);
  hipLaunchKernelGGL(nmf_gram_reduce_kernel, dim3(static_cast<unsigned>(pass.n_tile), RIDGE_NB * RIDGE_NB / 256),
                     dim3(256), 0, s, static_cast<const float *>(f.gram_partial.ptr), static_cast<int>(pass.n_slab),
                     static_cast<int>(pass.n_tile), static_cast<int>(f.k_pad), f.G.ptr);
  if (l2 != 0.f)
    hipLaunchKernelGGL(nmf_ridge_kernel, dim3(static_cast<unsigned>(ceil_div(f.k, 64))), dim3(64), 0, s, f.G.ptr,
                       static_cast<int>(f.k), static_cast<int>(f.k_pad), l2);
  IRS_HIP(hipGetLastError());
  sp.stop();
}

static int64_t sweep_groups(int64_t rows) { return ceil_div(rows, SWEEP_ROWS); }

// the rows of Wd swept against G and XH - l1; the workgroups' violation sums go to partial[first ...)
static void sweep(Fit &f, float *Wd, int64_t rows, float l1, int64_t first, hipStream_t s) {
  auto sp = f.spans.span(PH_SWEEP, s);
  hipLaunchKernelGGL(nmf_sweep_kernel, dim3(static_cast<unsigned>(sweep_groups(rows))), dim3(SWEEP_ROWS), 0, s, Wd,
                     static_cast<const float *>(f.XH.ptr), static_cast<const float *>(f.G.ptr), static_cast<int>(rows),
                     static_cast<int>(f.k), static_cast<int>(f.k_pad), l1, f.partial.ptr + first);
  IRS_HIP(hipGetLastError());
  sp.stop();
}

static void fit(Fit &f, const int64_t *indptr, const int32_t *indices, const float *data, float *W, float *H,
                float l1_W, float l2_W, float l1_H, float l2_H, double tol, int64_t max_iter, bool update_H,
                int64_t *n_iter_out, double *violations) {
  hipStream_t s = nullptr;
  const size_t U = static_cast<size_t>(f.n_users), I = static_cast<size_t>(f.n_items), K = static_cast<size_t>(f.k),
               KP = static_cast<size_t>(f.k_pad);
  std::vector<float> h_t(I * KP, 0.f);  // H^T, padded
  {
    auto sp = f.spans.span(PH_SETUP, s);
    upload_matrix(f, indptr, indices, data, s);
    for (size_t t = 0; t < K; t++)
      for (size_t i = 0; i < I; i++) h_t[i * KP + t] = H[t * I + i];
    f.Ht.upload(h_t, s);
    f.W.alloc(U * KP);
    f.W.zero(s);
    IRS_HIP(hipMemcpy2DAsync(f.W.ptr, KP * sizeof(float), W, K * sizeof(float), K * sizeof(float), U,
                             hipMemcpyHostToDevice, s));
    f.XH.alloc(std::max(U, I) * KP);
    f.G.alloc(KP * KP);
    const int64_t nb = f.k_pad / RIDGE_NB, n_tile = nb * (nb + 1) / 2;
    f.gram_partial.alloc(static_cast<size_t>(sblock::gram_slabs(n_tile) * n_tile * RIDGE_NB * RIDGE_NB));
    f.partial.alloc(static_cast<size_t>(sweep_groups(f.n_users) + sweep_groups(f.n_items)));
    f.violation.alloc(1);
    sp.stop();
  }
  const int64_t groups_W = sweep_groups(f.n_users), groups_H = update_H ? sweep_groups(f.n_items) : 0;
  if (!update_H) {
    spmm(f, f.X, f.Ht.ptr, f.XH.ptr, s);
    gram(f, f.Ht.ptr, f.n_items, l2_W, s);
  }
  double violation_init = 0.0;
  int64_t n_iter = 0;
  for (int64_t it = 1; it <= max_iter; it++) {
    if (update_H) {
      spmm(f, f.X, f.Ht.ptr, f.XH.ptr, s);
      gram(f, f.Ht.ptr, f.n_items, l2_W, s);
    }
    sweep(f, f.W.ptr, f.n_users, l1_W, 0, s);
    if (update_H) {
      spmm(f, f.Xt, f.W.ptr, f.XH.ptr, s);
      gram(f, f.W.ptr, f.n_users, l2_H, s);
      sweep(f, f.Ht.ptr, f.n_items, l1_H, groups_W, s);
    }
    double violation = 0.0;
    {
      auto sp = f.spans.span(PH_D2H, s);
      hipLaunchKernelGGL(nmf_violation_kernel, dim3(1), dim3(256), 0, s, static_cast<const double *>(f.partial.ptr),
                         static_cast<int>(groups_W + groups_H), f.violation.ptr);
      IRS_HIP(hipGetLastError());
      IRS_HIP(hipMemcpyAsync(&violation, f.violation.ptr, sizeof(double), hipMemcpyDeviceToHost, s));
      sp.stop();
    }
    IRS_HIP(hipStreamSynchronize(s));
    f.spans.fold();
    n_iter = it;
    if (violations != nullptr) violations[it - 1] = violation;
    // sklearn's test, _fit_coordinate_descent
    if (it == 1) violation_init = violation;
    if (violation_init == 0) break;
    if (violation / violation_init <= tol) break;
  }
  {
    auto sp = f.spans.span(PH_D2H, s);
    IRS_HIP(hipMemcpy2DAsync(W, K * sizeof(float), f.W.ptr, KP * sizeof(float), K * sizeof(float), U,
                             hipMemcpyDeviceToHost, s));
    if (update_H) IRS_HIP(hipMemcpyAsync(h_t.data(), f.Ht.ptr, I * KP * sizeof(float), hipMemcpyDeviceToHost, s));
    sp.stop();
  }
  IRS_HIP(hipStreamSynchronize(s));
  f.spans.fold();
  if (update_H)
    for (size_t t = 0; t < K; t++)
      for (size_t i = 0; i < I; i++) H[t * I + i] = h_t[i * KP + t];
  *n_iter_out = n_iter;
}

}  // namespace nmf
}  // namespace irs

using namespace irs;

extern "C" {

irs_status irs_nmf_fit(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                       const float *data, int64_t k, float *W, float *H, float l1_W, float l2_W, float l1_H,
                       float l2_H, double tol, int64_t max_iter, int32_t update_H, int32_t device, int64_t *n_iter,
                       double *violations, irs_nmf_stats_t *stats) {
  return guard([&] {
    const int64_t nnz = validate_finite_matrix(n_users, n_items, indptr, indices, data);
    for (int64_t q = 0; q < nnz; q++) check_arg(data[q] >= 0.f, "the matrix holds a negative value.");
    check_arg(k >= 1, "k must be >= 1.");
    check_arg(k <= sblock::MAX_L_PAD, "k must be <= 576.");
    check_arg(max_iter >= 1, "max_iter must be >= 1.");
    check_arg(tol >= 0.0, "tol must be >= 0.");
    for (float r : {l1_W, l2_W, l1_H, l2_H})
      check_arg(std::isfinite(r) && r >= 0.f, "the regularisers must be finite and >= 0.");
    check_arg(W != nullptr && H != nullptr && n_iter != nullptr, "W, H and n_iter must not be null.");
    for (int64_t q = 0; q < n_users * k; q++)
      check_arg(std::isfinite(W[q]) && W[q] >= 0.f, "the initial W must be finite and non-negative.");
    for (int64_t q = 0; q < k * n_items; q++)
      check_arg(std::isfinite(H[q]) && H[q] >= 0.f, "the initial H must be finite and non-negative.");
    check_arg(device >= 0, "irspack_amd: device index out of range.");
    require_device(device);
    nmf::Fit f;
    f.n_users = n_users, f.n_items = n_items, f.nnz = nnz, f.k = k;
    f.k_pad = ceil_div(k, tsvd::RIDGE_NB) * tsvd::RIDGE_NB;
    f.spans.enabled = stats != nullptr;
    nmf::fit(f, indptr, indices, data, W, H, l1_W, l2_W, l1_H, l2_H, tol, max_iter, update_H != 0, n_iter,
             violations);
    if (stats != nullptr) {
      stats->setup_ms = f.spans.ms[nmf::PH_SETUP];
      stats->spmm_ms = f.spans.ms[nmf::PH_SPMM];
      stats->gram_ms = f.spans.ms[nmf::PH_GRAM];
      stats->sweep_ms = f.spans.ms[nmf::PH_SWEEP];
      stats->d2h_ms = f.spans.ms[nmf::PH_D2H];
    }
  });
}

}  // extern "C"
