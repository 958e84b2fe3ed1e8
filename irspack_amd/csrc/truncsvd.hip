// TruncatedSVDRecommender (truncsvd.py of the reference: sklearn's randomized TruncatedSVD): the device side
// of utils.truncated_svd.  DESIGN.md section 11 has the algorithm and the figures.
//
// A = X when n_users >= n_items, else X^T (sklearn's transpose="auto"): m x n, m >= n.  The handle keeps A and
// A^T as CSR and three m x l_pad float32 blocks on the device (Y, Q and the target of the out-of-place
// products), l_pad = the sketch width rounded up to 64.
//
//   range    Q = omega; n_iter times { Y = A Q, normalise Y; Q = A^T Y, normalise Q }; Y = A Q; G = Y^T Y
//            normalise: G = Y^T Y, G + d I = L L^T (chol_tile_kernels.hpp), W = L^-1 (tri_inv_kernels.hpp),
//            Y <- Y W^T - keeps the block well conditioned, spans the same subspace
//   apply    Y <- Y M for a host matrix M (the eigen-decomposition of G happens between the calls); G = Y^T Y
//   project  Q = A^T Y (= B^T for B = Y^T A); G = Q^T Q = B B^T
//   finish   V = Q M or Y M (the n_items x k side), z = X V by one more SpMM, signs, copies home
//
// One stream; one synchronisation per call, except that the first `range` also sets the matrix up on the
// device (blocking copies of the segment lists, the device transpose's synchronisation).  Every argument
// check of every call comes before any device work.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>

#include "csr_checks.hpp"
#include "nmf_kernels.hpp"
#include "phase_spans.hpp"
#include "sparse_block.hpp"
#include "tile_solver_calls.hpp"
#include "truncsvd_kernels.hpp"

namespace irs {
namespace tsvd {

using sblock::Csr;
using sblock::MAX_L_PAD;
static_assert(sblock::SEG_LEN == SPMM_SEG && sblock::TILE_EDGE == RIDGE_NB, "sparse_block_plan.hpp's constants");

enum Phase { PH_SPMM = 0, PH_GRAM, PH_CHOL, PH_APPLY, PH_D2H, PH_SETUP, PH_COUNT };

struct Handle {
  int device = 0;
  int64_t n_users = 0, n_items = 0, nnz = 0;
  bool transposed = false;  // A = X^T
  int64_t m = 0, n = 0;     // A is m x n
  // the caller's matrix until the first range call uploads it
  std::vector<int32_t> h_ptr, h_idx;
  std::vector<float> h_val;
  bool on_device = false;
  Csr X, Xt;
  const Csr *A = nullptr, *At = nullptr;
  int64_t l = 0, l_pad = 0;  // current width (range: the sketch; apply: M's columns), padded width (fixed by range)
  bool projected = false;
  DeviceBuffer<float> buf[3], G, W, Ms, gram_partial, spmm_partial;
  DeviceBuffer<int32_t> flag;
  float *Y = nullptr, *Q = nullptr, *S = nullptr;
  PhaseSpans<PH_COUNT> spans;  // always recording: the running call's pairs, folded after its synchronisation
  double host_ms = 0.0;  // finish: signs and transpose on the host
  int64_t n_spmm = 0;
};

static void ensure_on_device(Handle &h, hipStream_t s) {
  require_device(h.device);
  if (h.on_device) return;
  auto sp = h.spans.span(PH_SETUP, s);
  sblock::upload_with_transpose(h.h_ptr, h.h_idx.data(), h.h_val.data(), h.n_users, h.n_items, h.nnz, h.X, h.Xt,
                                h.spmm_partial, MAX_L_PAD, s);
  h.flag.alloc(1);
  h.A = h.transposed ? &h.Xt : &h.X;
  h.At = h.transposed ? &h.X : &h.Xt;
  sp.stop();
  h.on_device = true;
  h.h_idx = std::vector<int32_t>();
  h.h_val = std::vector<float>();
}

// out (M.rows x l_pad) = M in (M.cols x l_pad)
static void spmm(Handle &h, const Csr &M, const float *in, float *out, hipStream_t s) {
  if (M.rows == 0) return;
  auto sp = h.spans.span(PH_SPMM, s);
  const int lp = static_cast<int>(h.l_pad);
  float *partial = h.spmm_partial.ptr;
  sblock::for_spmm_width(lp / 4, [&](auto lpr, auto nch) {
    sblock::launch_spmm(tsvd_spmm_kernel<decltype(lpr)::value, decltype(nch)::value>, M, in, lp, out, partial, s);
  });
  sblock::launch_split_reduce(tsvd_spmm_reduce_kernel, M, partial, lp, out, s);
  IRS_HIP(hipGetLastError());
  sp.stop();
  h.n_spmm++;
}

// G (l_pad x l_pad, symmetric) = B^T B for the block B of `rows` rows
static void gram(Handle &h, const float *B, int64_t rows, hipStream_t s) {
  auto sp = h.spans.span(PH_GRAM, s);
  const sblock::GramPass pass = sblock::launch_gram_partials(B, rows, h.l_pad, h.gram_partial.ptr, s);
  hipLaunchKernelGGL(tsvd_gram_reduce_kernel, dim3(static_cast<unsigned>(pass.n_tile), RIDGE_NB * RIDGE_NB / 256),
                     dim3(256), 0, s, static_cast<const float *>(h.gram_partial.ptr), static_cast<int>(pass.n_slab),
                     static_cast<int>(pass.n_tile), static_cast<int>(h.l_pad), h.G.ptr);
  IRS_HIP(hipGetLastError());
  sp.stop();
}

// out = B M (TRANS: M = W^T, W lower triangular) for the block B of `rows` rows
template <bool TRANS>
static void apply(Handle &h, const float *B, int64_t rows, const float *M, float *out, hipStream_t s) {
  if (rows == 0) return;
  auto sp = h.spans.span(PH_APPLY, s);
  hipLaunchKernelGGL((tsvd_apply_kernel<TRANS>),
                     dim3(static_cast<unsigned>(ceil_div(rows, RIDGE_NB)), static_cast<unsigned>(h.l_pad / RIDGE_NB)),
                     dim3(256), 0, s, B, static_cast<int>(rows), static_cast<int>(h.l_pad), M, out);
  IRS_HIP(hipGetLastError());
  sp.stop();
}

// B <- B L^-T with L L^T = B^T B + d I; the result lands in h.S, the caller swaps
static void normalise(Handle &h, const float *B, int64_t rows, hipStream_t s) {
  gram(h, B, rows, s);
  {
    auto sp = h.spans.span(PH_CHOL, s);
    const int lp = static_cast<int>(h.l_pad);
    const int64_t nb = h.l_pad / RIDGE_NB;
    float *G = h.G.ptr, *W = h.W.ptr;
    hipLaunchKernelGGL(tsvd_shift_kernel, dim3(1), dim3(64), 0, s, G, static_cast<int>(h.l), lp);
    launch_tile_cholesky(G, lp, nb, h.flag.ptr, s);
    h.W.zero(s);
    launch_tile_tri_inverse(G, W, lp, nb, s);
    IRS_HIP(hipGetLastError());
    sp.stop();
  }
  apply<true>(h, B, rows, h.W.ptr, h.S, s);
}

// the leading l x l block of G into the caller's array, then the call's one synchronisation
static void gram_home_and_sync(Handle &h, float *gram_out, hipStream_t s) {
  {
    auto sp = h.spans.span(PH_D2H, s);
    IRS_HIP(hipMemcpy2DAsync(gram_out, static_cast<size_t>(h.l) * sizeof(float), h.G.ptr,
                             static_cast<size_t>(h.l_pad) * sizeof(float), static_cast<size_t>(h.l) * sizeof(float),
                             static_cast<size_t>(h.l), hipMemcpyDeviceToHost, s));
    sp.stop();
  }
  IRS_HIP(hipStreamSynchronize(s));
  h.spans.fold();
}

static void range(Handle &h, const float *omega, int64_t rows, int64_t l, int64_t n_iter, float *gram_out) {
  check_arg(l >= 1, "the sketch width l must be >= 1.");
  check_arg(rows == h.n, "omega must have min(n_users, n_items) rows: n_items when n_users >= n_items, else n_users.");
  check_arg(l <= std::min(h.n_users, h.n_items), "the sketch width l must be <= min(n_users, n_items).");
  check_arg(l <= MAX_L_PAD, "the sketch width l must be <= 576.");
  check_arg(n_iter >= 0, "n_iter must be >= 0.");
  check_arg(omega != nullptr && gram_out != nullptr, "omega and gram_out must not be null.");
  for (int64_t i = 0; i < rows * l; i++) check_arg(std::isfinite(omega[i]), "omega must be finite.");
  hipStream_t s = nullptr;
  h.spans.clear();
  ensure_on_device(h, s);
  h.l = l;
  h.l_pad = ceil_div(l, RIDGE_NB) * RIDGE_NB;
  h.projected = false;
  const size_t block = static_cast<size_t>(h.m) * static_cast<size_t>(h.l_pad);
  const size_t LP2 = static_cast<size_t>(h.l_pad * h.l_pad);
  size_t free_b = 0, total_b = 0;
  IRS_HIP(hipMemGetInfo(&free_b, &total_b));
  size_t have = 0;
  for (auto &b : h.buf) have += b.count >= block ? block : 0;
  const int64_t nb = h.l_pad / RIDGE_NB, n_tile = nb * (nb + 1) / 2;
  const size_t partials = static_cast<size_t>(sblock::gram_slabs(n_tile) * n_tile * RIDGE_NB * RIDGE_NB);
  const double need = 4.0 * double(3 * block - have) + 12.0 * double(LP2) + 4.0 * double(partials) +
                      double(size_t(64) << 20);
  if (need > double(free_b))
    throw std::runtime_error("truncated SVD: three " + std::to_string(h.m) + " x " + std::to_string(h.l_pad) +
                             " float32 blocks need " + std::to_string(static_cast<int64_t>(need / 1048576.0)) +
                             " MiB of device memory, " + std::to_string(free_b >> 20) + " MiB are free.");
  for (auto &b : h.buf) b.alloc(block);
  h.G.alloc(LP2);
  h.W.alloc(LP2);
  h.Ms.alloc(LP2);
  h.gram_partial.alloc(partials);
  h.Y = h.buf[0].ptr, h.Q = h.buf[1].ptr, h.S = h.buf[2].ptr;
  h.flag.zero(s);
  // Q = omega in the leading columns, zeros in the padding
  IRS_HIP(hipMemsetAsync(h.Q, 0, static_cast<size_t>(h.n) * h.l_pad * sizeof(float), s));
  IRS_HIP(hipMemcpy2DAsync(h.Q, static_cast<size_t>(h.l_pad) * sizeof(float), omega,
                           static_cast<size_t>(l) * sizeof(float), static_cast<size_t>(l) * sizeof(float),
                           static_cast<size_t>(rows), hipMemcpyHostToDevice, s));
  for (int64_t it = 0; it < n_iter; it++) {
    spmm(h, *h.A, h.Q, h.Y, s);
    normalise(h, h.Y, h.m, s);
    std::swap(h.Y, h.S);
    spmm(h, *h.At, h.Y, h.Q, s);
    normalise(h, h.Q, h.n, s);
    std::swap(h.Q, h.S);
  }
  spmm(h, *h.A, h.Q, h.Y, s);
  gram(h, h.Y, h.m, s);
  int32_t flag = 0;
  IRS_HIP(hipMemcpyAsync(&flag, h.flag.ptr, sizeof(flag), hipMemcpyDeviceToHost, s));
  gram_home_and_sync(h, gram_out, s);
  if (flag != 0)
    throw std::runtime_error("truncated SVD: the Gram matrix of a block has no Cholesky factor (a pivot is not > 0 "
                             "or not finite: the matrix is zero or its products overflow float32).");
}

// a host matrix [rows, cols] into the zeroed l_pad x l_pad device matrix Ms
static void upload_small(Handle &h, const float *M, int64_t rows, int64_t cols, hipStream_t s) {
  h.Ms.zero(s);
  IRS_HIP(hipMemcpy2DAsync(h.Ms.ptr, static_cast<size_t>(h.l_pad) * sizeof(float), M,
                           static_cast<size_t>(cols) * sizeof(float), static_cast<size_t>(cols) * sizeof(float),
                           static_cast<size_t>(rows), hipMemcpyHostToDevice, s));
}

static void apply_host(Handle &h, const float *M, int64_t l2, float *gram_out) {
  check_arg(h.l >= 1 && h.Y != nullptr, "irs_truncsvd_range has not run.");
  check_arg(l2 >= 1 && l2 <= h.l, "l2 must be in [1, l].");
  check_arg(M != nullptr && gram_out != nullptr, "m and gram_out must not be null.");
  for (int64_t i = 0; i < h.l * l2; i++) check_arg(std::isfinite(M[i]), "m must be finite.");
  hipStream_t s = nullptr;
  h.spans.clear();
  require_device(h.device);
  upload_small(h, M, h.l, l2, s);
  apply<false>(h, h.Y, h.m, h.Ms.ptr, h.S, s);
  std::swap(h.Y, h.S);
  h.l = l2;
  h.projected = false;
  gram(h, h.Y, h.m, s);
  gram_home_and_sync(h, gram_out, s);
}

static void project(Handle &h, float *gram_out) {
  check_arg(h.l >= 1 && h.Y != nullptr, "irs_truncsvd_range has not run.");
  check_arg(gram_out != nullptr, "gram_out must not be null.");
  hipStream_t s = nullptr;
  h.spans.clear();
  require_device(h.device);
  spmm(h, *h.At, h.Y, h.Q, s);
  gram(h, h.Q, h.n, s);
  h.projected = true;
  gram_home_and_sync(h, gram_out, s);
}

static void finish(Handle &h, const float *rot, int64_t k, float *z_out, float *components_out) {
  check_arg(k >= 1, "k must be >= 1.");
  check_arg(k <= h.l, "k > l2: more components than the basis has columns.");
  check_arg(h.projected, "irs_truncsvd_project has not run.");
  check_arg(rot != nullptr && z_out != nullptr && components_out != nullptr, "null argument.");
  for (int64_t i = 0; i < h.l * k; i++) check_arg(std::isfinite(rot[i]), "rot must be finite.");
  hipStream_t s = nullptr;
  h.spans.clear();
  require_device(h.device);
  upload_small(h, rot, h.l, k, s);
  // V, n_items x k: rows of Q when A = X (B^T R / sigma), rows of Y when A = X^T (Y R); z = X V
  float *z_dev;
  if (!h.transposed) {
    apply<false>(h, h.Q, h.n, h.Ms.ptr, h.S, s);
    spmm(h, *h.A, h.S, h.Y, s);
    z_dev = h.Y;
  } else {
    apply<false>(h, h.Y, h.m, h.Ms.ptr, h.S, s);
    spmm(h, *h.At, h.S, h.Q, s);
    z_dev = h.Q;
  }
  h.projected = false;  // (Y or Q now holds z)
  const size_t I = static_cast<size_t>(h.n_items), U = static_cast<size_t>(h.n_users), K = static_cast<size_t>(k);
  std::vector<float> V(I * K);
  {
    auto sp = h.spans.span(PH_D2H, s);
    IRS_HIP(hipMemcpy2DAsync(V.data(), K * sizeof(float), h.S, static_cast<size_t>(h.l_pad) * sizeof(float),
                             K * sizeof(float), I, hipMemcpyDeviceToHost, s));
    IRS_HIP(hipMemcpy2DAsync(z_out, K * sizeof(float), z_dev, static_cast<size_t>(h.l_pad) * sizeof(float),
                             K * sizeof(float), U, hipMemcpyDeviceToHost, s));
    sp.stop();
  }
  IRS_HIP(hipStreamSynchronize(s));
  h.spans.fold();
  // svd_flip(u_based_decision=False): the entry of largest magnitude of every component (the first of equals)
  // is positive; the components go out transposed
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<float> sign(K, 1.0f);
  for (size_t j = 0; j < K; j++) {
    float best = -1.0f, at = 0.0f;
    for (size_t i = 0; i < I; i++) {
      const float v = V[i * K + j];
      if (std::fabs(v) > best) best = std::fabs(v), at = v;
    }
    sign[j] = at < 0.0f ? -1.0f : 1.0f;
    for (size_t i = 0; i < I; i++) components_out[j * I + i] = sign[j] * V[i * K + j];
  }
  for (size_t u = 0; u < U; u++)
    for (size_t j = 0; j < K; j++) z_out[u * K + j] *= sign[j];
  h.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace tsvd
}  // namespace irs

using namespace irs;

struct irs_truncsvd {
  tsvd::Handle h;
};

extern "C" {

irs_status irs_truncsvd_create(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                               const float *data, int32_t device, irs_truncsvd **out) {
  return guard([&] {
    check_arg(out != nullptr, "out must not be null.");
    *out = nullptr;
    const int64_t nnz = validate_finite_matrix(n_users, n_items, indptr, indices, data);
    check_arg(device >= 0, "irspack_amd: device index out of range.");
    std::unique_ptr<irs_truncsvd> p(new irs_truncsvd());
    tsvd::Handle &h = p->h;
    h.device = device;
    h.n_users = n_users, h.n_items = n_items, h.nnz = nnz;
    h.transposed = n_users < n_items;
    h.m = std::max(n_users, n_items), h.n = std::min(n_users, n_items);
    h.h_ptr.resize(static_cast<size_t>(n_users) + 1);
    for (int64_t i = 0; i <= n_users; i++) h.h_ptr[i] = static_cast<int32_t>(indptr[i]);
    h.h_idx.assign(indices, indices + nnz);
    h.h_val.assign(data, data + nnz);
    *out = p.release();
  });
}

irs_status irs_truncsvd_range(irs_truncsvd *t, const float *omega, int64_t rows, int64_t l, int64_t n_iter,
                              float *gram_out) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    tsvd::range(t->h, omega, rows, l, n_iter, gram_out);
  });
}

irs_status irs_truncsvd_apply(irs_truncsvd *t, const float *m, int64_t l2, float *gram_out) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    tsvd::apply_host(t->h, m, l2, gram_out);
  });
}

irs_status irs_truncsvd_project(irs_truncsvd *t, float *gram_out) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    tsvd::project(t->h, gram_out);
  });
}

irs_status irs_truncsvd_finish(irs_truncsvd *t, const float *rot, int64_t k, float *z_out, float *components_out) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    tsvd::finish(t->h, rot, k, z_out, components_out);
  });
}

irs_status irs_truncsvd_stats(irs_truncsvd *t, irs_truncsvd_stats_t *out) {
  return guard([&] {
    check_arg(t != nullptr && out != nullptr, "null argument.");
    const tsvd::Handle &h = t->h;
    out->setup_ms = h.spans.ms[tsvd::PH_SETUP];
    out->spmm_ms = h.spans.ms[tsvd::PH_SPMM];
    out->gram_ms = h.spans.ms[tsvd::PH_GRAM];
    out->chol_ms = h.spans.ms[tsvd::PH_CHOL];
    out->apply_ms = h.spans.ms[tsvd::PH_APPLY];
    out->d2h_ms = h.spans.ms[tsvd::PH_D2H];
    out->host_ms = h.host_ms;
    out->n_spmm = h.n_spmm;
    out->l_pad = h.l_pad;
  });
}

irs_status irs_truncsvd_destroy(irs_truncsvd *t) {
  return guard([&] { delete t; });
}

// The fold-in of new rows, z = X V for the item table V [n_items, k] (components_^T): stateless, one sparse x
// tall-block product with the row sums in double (nmf_spmm_kernel), every element rounded to float32 once - a split
// row's segments are added in double too.  The sums have a fixed order: the result is a function of the arguments.
irs_status irs_truncsvd_transform(int64_t rows, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                                  const float *data, int64_t k, const float *item_factors, int32_t device,
                                  float *out) {
  return guard([&] {
    const int64_t nnz = validate_csr(rows, n_items, indptr, indices, data);
    check_arg(n_items >= 1, "the matrix must have at least one column.");
    for (int64_t q = 0; q < nnz; q++) check_arg(std::isfinite(data[q]), "the matrix holds a non-finite value.");
    check_arg(k >= 1 && k <= tsvd::MAX_L_PAD, "k must lie in 1 .. 576.");
    check_arg(item_factors != nullptr && (rows == 0 || out != nullptr), "null argument.");
    check_arg(device >= 0, "irspack_amd: device index out of range.");
    if (rows == 0) return;
    require_device(device);
    hipStream_t s = nullptr;
    const int64_t k_pad = ceil_div(k, tsvd::RIDGE_NB) * tsvd::RIDGE_NB;
    const size_t K = static_cast<size_t>(k), KP = static_cast<size_t>(k_pad);
    tsvd::Csr X;
    X.rows = rows, X.cols = n_items;
    std::vector<int32_t> h_ptr(static_cast<size_t>(rows) + 1);
    for (int64_t i = 0; i <= rows; i++) h_ptr[i] = static_cast<int32_t>(indptr[i]);
    X.idx.upload(indices, static_cast<size_t>(nnz), s);
    X.val.upload(data, static_cast<size_t>(nnz), s);
    sblock::upload_segments(h_ptr, X);
    DeviceBuffer<float> V, Z;
    DeviceBuffer<double> partial;
    V.alloc(static_cast<size_t>(n_items) * KP);
    if (KP != K) V.zero(s);
    IRS_HIP(hipMemcpy2DAsync(V.ptr, KP * sizeof(float), item_factors, K * sizeof(float), K * sizeof(float),
                             static_cast<size_t>(n_items), hipMemcpyHostToDevice, s));
    Z.alloc(static_cast<size_t>(rows) * KP);
    partial.alloc(static_cast<size_t>(std::max<int64_t>(1, X.n_slot)) * KP);
    const int lp = static_cast<int>(k_pad);
    sblock::for_spmm_width(lp / 4, [&](auto lpr, auto nch) {
      sblock::launch_spmm(nmf::nmf_spmm_kernel<decltype(lpr)::value, decltype(nch)::value, double>, X, V.ptr, lp,
                          Z.ptr, partial.ptr, s);
    });
    sblock::launch_split_reduce(nmf::nmf_spmm_reduce_f64_kernel, X, partial.ptr, lp, Z.ptr, s);
    IRS_HIP(hipGetLastError());
    IRS_HIP(hipMemcpy2DAsync(out, K * sizeof(float), Z.ptr, KP * sizeof(float), K * sizeof(float),
                             static_cast<size_t>(rows), hipMemcpyDeviceToHost, s));
    IRS_HIP(hipStreamSynchronize(s));
  });
}

}  // extern "C"
