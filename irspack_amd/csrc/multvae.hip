// MultVAERecommender (multvae.py of the reference trains with jax / haiku / optax; the arithmetic here is this
// project's own statement of the same model - DESIGN.md section 15): the device side of
// irspack_amd.recommenders.multvae.MultVAETrainer.
//
// The parameter arena, its Adam moments, the gradient arena, the matrix and the work buffers of one batch live on
// the device for the life of the handle.  A batch is a fixed sequence of launches on one stream
// (multvae_kernels.hpp), an epoch a host loop over its batches with no copy and no synchronisation in it; the call
// synchronises once at its end and reads the divergence flag.  The handle is made without a device: every
// argument check comes before any device work.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "csr_checks.hpp"
#include "multvae_kernels.hpp"
#include "phase_spans.hpp"

namespace irs {
namespace mv {

enum Phase { PH_ENCODE = 0, PH_DENSE, PH_LOGIT, PH_SOFTMAX, PH_DW4, PH_DH2, PH_DW1, PH_ADAM, PH_COUNT };

}  // namespace mv
}  // namespace irs

struct irs_multvae {
  int64_t n_users = 0, n_items = 0, minibatch = 0, anneal_end_epoch = 0, n_updates = 0, epoch = 0;
  int32_t device = 0, G = 1, nch = 1;
  float dropout_p = 0.f, l2 = 0.f, lr = 0.f;
  double kl_goal = 0.0;
  uint64_t seed = 0;
  irs::mv::Layout y;
  bool on_device = false;
  std::vector<int32_t> h_indptr;                        // (kept: the offsets of a batch's dropout bytes)
  std::vector<int32_t> h_indices;                       // until the first device call
  std::vector<float> h_data;
  std::vector<float> h_state[3 * irs::mv::N_TABLES];    // tables, m, v (unpadded) until the first device call
  irs::DeviceBuffer<float> theta, m, v, G_arena, data;
  irs::DeviceBuffer<unsigned long long> acc;
  irs::DeviceBuffer<int32_t> indptr, indices, users, keep_ptr, diverged;
  irs::DeviceBuffer<uint8_t> keep;
  irs::DeviceBuffer<float> eps, h1a, ml, za, stdv, epsv, h2a, block, da3, dz, dml, da1, rowscale, row_lse, part;
  irs::DeviceBuffer<double> row_nll, row_kl, loss;
  // a caller's rows (encode, score)
  irs::DeviceBuffer<int32_t> c_indptr, c_indices;
  irs::DeviceBuffer<float> c_data;
  int64_t cap = 0;  // batch rows the work buffers hold
  double klc_last = 0, nll_last = 0, kl_last = 0;
  irs::PhaseSpans<irs::mv::PH_COUNT> spans;  // on with IRSPACK_AMD_MULTVAE_PHASES
  double epoch_ms = 0;
};

namespace irs {
namespace mv {

// the host tables of one group (0: parameters, 1: m, 2: v) <-> an arena on the device
static void upload_arena(irs_multvae &t, int group, DeviceBuffer<float> &d, hipStream_t s) {
  std::vector<float> image(static_cast<size_t>(t.y.total), 0.f);
  for (int q = 0; q < N_TABLES; q++) pack_table(t.y, q, t.h_state[group * N_TABLES + q].data(), image.data());
  d.upload(image, s);
  IRS_HIP(hipStreamSynchronize(s));  // (image is the source of an asynchronous copy)
}
static void download_arena(irs_multvae &t, const DeviceBuffer<float> &d, float *const *dst) {
  bool any = false;
  for (int q = 0; q < N_TABLES; q++) any |= dst[q] != nullptr;
  if (!any) return;
  std::vector<float> image(static_cast<size_t>(t.y.total));
  IRS_HIP(hipMemcpy(image.data(), d.ptr, image.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int q = 0; q < N_TABLES; q++)
    if (dst[q]) unpack_table(t.y, q, image.data(), dst[q]);
}

template <class T> static void alloc_or_explain(DeviceBuffer<T> &d, size_t n, const char *what) {
  try {
    d.alloc(n);
  } catch (const std::exception &) {
    (void)hipGetLastError();
    throw std::runtime_error(std::string("Mult-VAE: not enough device memory for ") + what + " (" +
                             std::to_string(n * sizeof(T) >> 20) + " MiB): lower minibatch_size.");
  }
}

// work buffers for batches of up to `rows` rows
static void reserve(irs_multvae &t, int64_t rows, hipStream_t s) {
  if (rows <= t.cap) return;
  const Layout &y = t.y;
  const size_t n = static_cast<size_t>(rows), I = static_cast<size_t>(y.I), H = static_cast<size_t>(y.H),
               L = static_cast<size_t>(y.L), Hd = static_cast<size_t>(y.Hd), Hp = static_cast<size_t>(y.Hp);
  alloc_or_explain(t.block, n * I, "the [batch, n_items] block");
  const size_t dw4_slabs = static_cast<size_t>(ceil_div(rows, DW4_SLAB)), dh2_slabs = static_cast<size_t>(ceil_div(y.I, dh2_slab(y.I)));
  alloc_or_explain(t.part, std::max(dw4_slabs * (Hd + 1) * I, dh2_slabs * n * Hd), "the K-slab partial products");
  t.users.alloc(n), t.keep_ptr.alloc(n + 1);
  t.h1a.alloc(n * (H + 1)), t.ml.alloc(n * 2 * L), t.za.alloc(n * (L + 1)), t.stdv.alloc(n * L), t.epsv.alloc(n * L);
  t.eps.alloc(n * L), t.h2a.alloc(n * (Hd + 1)), t.da3.alloc(n * Hd), t.dz.alloc(n * L), t.dml.alloc(n * 2 * L);
  t.da1.alloc(n * Hp), t.rowscale.alloc(n), t.row_lse.alloc(n), t.row_nll.alloc(n), t.row_kl.alloc(n);
  t.da1.zero(s);  // (the padding columns are never written)
  t.cap = rows;
}

// first device use of the handle: the device, the matrix, the arenas, zeroed sums
static void to_device(irs_multvae &t) {
  require_device(t.device);
  if (t.on_device) return;
  hipStream_t s = nullptr;
  t.indptr.upload(t.h_indptr, s);
  t.indices.upload(t.h_indices, s);
  t.data.upload(t.h_data, s);
  IRS_HIP(hipStreamSynchronize(s));
  upload_arena(t, 0, t.theta, s);
  upload_arena(t, 1, t.m, s);
  upload_arena(t, 2, t.v, s);
  t.G_arena.alloc(static_cast<size_t>(t.y.total));
  t.G_arena.zero(s);
  t.acc.alloc(static_cast<size_t>(t.y.w1_count));
  t.acc.zero(s);
  t.diverged.alloc(1);
  t.diverged.zero(s);
  t.loss.alloc(2);
  t.loss.zero(s);
  reserve(t, std::max<int64_t>(1, std::min(t.minibatch, t.n_users)), s);
  IRS_HIP(hipStreamSynchronize(s));
  for (auto &h : t.h_state) std::vector<float>().swap(h);
  std::vector<int32_t>().swap(t.h_indices);
  std::vector<float>().swap(t.h_data);
  t.on_device = true;
}

template <bool TA, bool TB, int EPI>
static void gemm(int64_t M, int64_t N, int64_t K, const float *A, int64_t lda, const float *B, int64_t ldb, float *C,
                 int64_t ldc, const float *aux, int64_t ldaux, int64_t slab, int64_t c_slab_stride, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(ceil_div(N, BN)), static_cast<unsigned>(ceil_div(M, BM)),
                  static_cast<unsigned>(ceil_div(K, slab)));
  hipLaunchKernelGGL((mv_gemm_kernel<TA, TB, EPI>), grid, dim3(BLOCK), 0, s, static_cast<int32_t>(M),
                     static_cast<int32_t>(N), static_cast<int32_t>(K), A, lda, B, ldb, C, ldc, aux, ldaux,
                     static_cast<int32_t>(slab), c_slab_stride);
  IRS_HIP(hipGetLastError());
}
template <bool TA, bool TB, int EPI>
static void gemm(int64_t M, int64_t N, int64_t K, const float *A, int64_t lda, const float *B, int64_t ldb, float *C,
                 int64_t ldc, const float *aux, int64_t ldaux, hipStream_t s) {
  gemm<TA, TB, EPI>(M, N, K, A, lda, B, ldb, C, ldc, aux, ldaux, K, 0, s);
}
template <int EPI>
static void forward_dense(int64_t M, int64_t N, int64_t K, const float *A, int64_t lda, const float *B, int64_t ldb,
                          float *C, int64_t ldc, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(ceil_div(N, 16)), static_cast<unsigned>(ceil_div(M, 16)));
  hipLaunchKernelGGL((mv_forward_dense_kernel<EPI>), grid, dim3(BLOCK), 0, s, static_cast<int32_t>(M),
                     static_cast<int32_t>(N), static_cast<int32_t>(K), A, lda, B, ldb, C, ldc);
  IRS_HIP(hipGetLastError());
}
// a product split into K-slabs: the partials, then their sum in slab order with the epilogue
template <bool TA, bool TB, int EPI>
static void gemm_slabs(irs_multvae &t, int64_t M, int64_t N, int64_t K, int64_t slab, const float *A, int64_t lda,
                       const float *B, int64_t ldb, float *C, int64_t ldc, const float *aux, int64_t ldaux, hipStream_t s) {
  const int64_t n_slabs = ceil_div(K, slab);
  gemm<TA, TB, EPI_NONE>(M, N, K, A, lda, B, ldb, t.part.ptr, N, nullptr, 0, slab, M * N, s);
  hipLaunchKernelGGL((mv_reduce_slabs_kernel<EPI>), dim3(static_cast<unsigned>(ceil_div(M * N, BLOCK))), dim3(BLOCK), 0, s,
                     M * N, static_cast<int32_t>(N), static_cast<int32_t>(n_slabs),
                     static_cast<const float *>(t.part.ptr), M * N, C, ldc, aux, ldaux);
  IRS_HIP(hipGetLastError());
}

static void launch_encode_input(irs_multvae &t, const SparseRows &x, int64_t n, float inv_keep_p, hipStream_t s) {
  const Layout &y = t.y;
  const dim3 grid(static_cast<unsigned>(n)), block(BLOCK);
  const int32_t H = static_cast<int32_t>(y.H), Hp = static_cast<int32_t>(y.Hp);
  const float *W1b = t.theta.ptr + y.seg[0];
  switch (t.nch) {
    case 1: hipLaunchKernelGGL((mv_encode_input_kernel<1>), grid, block, 0, s, x, H, Hp, t.G, y.I, W1b, inv_keep_p, t.h1a.ptr, t.rowscale.ptr); break;
    case 2: hipLaunchKernelGGL((mv_encode_input_kernel<2>), grid, block, 0, s, x, H, Hp, t.G, y.I, W1b, inv_keep_p, t.h1a.ptr, t.rowscale.ptr); break;
    default: hipLaunchKernelGGL((mv_encode_input_kernel<3>), grid, block, 0, s, x, H, Hp, t.G, y.I, W1b, inv_keep_p, t.h1a.ptr, t.rowscale.ptr);
  }
  IRS_HIP(hipGetLastError());
}
static void launch_dw1(irs_multvae &t, const SparseRows &x, int64_t n, double scale, hipStream_t s) {
  const Layout &y = t.y;
  const dim3 grid(static_cast<unsigned>(n)), block(BLOCK);
  const int32_t Hp = static_cast<int32_t>(y.Hp);
  const float *da1 = t.da1.ptr, *rs = t.rowscale.ptr;
  switch (t.nch) {
    case 1: hipLaunchKernelGGL((mv_dw1_kernel<1>), grid, block, 0, s, x, Hp, t.G, y.I, da1, rs, t.acc.ptr, scale, t.diverged.ptr); break;
    case 2: hipLaunchKernelGGL((mv_dw1_kernel<2>), grid, block, 0, s, x, Hp, t.G, y.I, da1, rs, t.acc.ptr, scale, t.diverged.ptr); break;
    default: hipLaunchKernelGGL((mv_dw1_kernel<3>), grid, block, 0, s, x, Hp, t.G, y.I, da1, rs, t.acc.ptr, scale, t.diverged.ptr);
  }
  IRS_HIP(hipGetLastError());
}

// the forward pass of n rows up to the logits in t.block; evaluate: no dropout, z = mu
static void forward(irs_multvae &t, const SparseRows &x, int64_t n, bool evaluate, uint64_t eps_key, const float *eps_in,
                    hipStream_t s) {
  const Layout &y = t.y;
  const float *th = t.theta.ptr;
  {
    auto sp = t.spans.span(PH_ENCODE, s);
    launch_encode_input(t, x, n, evaluate ? 1.f : 1.f / (1.f - t.dropout_p), s);
    sp.stop();
  }
  {
    auto sp = t.spans.span(PH_DENSE, s);
    forward_dense<EPI_NONE>(n, 2 * y.L, y.H + 1, t.h1a.ptr, y.H + 1, th + y.seg[1], 2 * y.L, t.ml.ptr, 2 * y.L, s);
    hipLaunchKernelGGL(mv_latent_forward_kernel, dim3(static_cast<unsigned>(n)), dim3(BLOCK), 0, s,
                       static_cast<int32_t>(y.L), static_cast<int32_t>(y.Hd), x.rows, static_cast<const float *>(t.ml.ptr),
                       eps_key, eps_in, evaluate ? 1 : 0, t.za.ptr, t.h2a.ptr, t.stdv.ptr, t.epsv.ptr, t.row_kl.ptr);
    IRS_HIP(hipGetLastError());
    forward_dense<EPI_TANH>(n, y.Hd, y.L + 1, t.za.ptr, y.L + 1, th + y.seg[2], y.Hd, t.h2a.ptr, y.Hd + 1, s);
    sp.stop();
  }
  auto sp = t.spans.span(PH_LOGIT, s);
  gemm<false, false, EPI_NONE>(n, y.I, y.Hd + 1, t.h2a.ptr, y.Hd + 1, th + y.seg[3], y.I, t.block.ptr, y.I, nullptr, 0, s);
  sp.stop();
}

static void launch_softmax(irs_multvae &t, const SparseRows &x, int64_t n, int mode, hipStream_t s) {
  hipLaunchKernelGGL(mv_softmax_kernel, dim3(static_cast<unsigned>(n)), dim3(BLOCK), 0, s, x, t.y.I, t.block.ptr,
                     1.f / static_cast<float>(n), mode, t.row_nll.ptr, t.row_lse.ptr);
  IRS_HIP(hipGetLastError());
}

// one update on the n rows whose users are in t.users; keep / eps: the caller's noise, already on the device
static void step(irs_multvae &t, int64_t n, double klc, bool own_keep, bool own_eps, bool want_loss, hipStream_t s) {
  const Layout &y = t.y;
  SparseRows x;
  x.rows = t.users.ptr, x.indptr = t.indptr.ptr, x.indices = t.indices.ptr, x.data = t.data.ptr;
  x.keep = own_keep ? t.keep.ptr : nullptr, x.keep_ptr = t.keep_ptr.ptr;
  x.keep_key = noise_key(t.seed, t.n_updates, 0), x.threshold = keep_threshold(t.dropout_p);
  float *th = t.theta.ptr, *G = t.G_arena.ptr;
  forward(t, x, n, false, noise_key(t.seed, t.n_updates, 1), own_eps ? t.eps.ptr : nullptr, s);
  {
    auto sp = t.spans.span(PH_SOFTMAX, s);
    launch_softmax(t, x, n, SM_GRADIENT, s);
    sp.stop();
  }
  {
    auto sp = t.spans.span(PH_DW4, s);
    gemm_slabs<true, false, EPI_NONE>(t, y.Hd + 1, y.I, n, DW4_SLAB, t.h2a.ptr, y.Hd + 1, t.block.ptr, y.I, G + y.seg[3], y.I, nullptr, 0, s);
    sp.stop();
  }
  {
    auto sp = t.spans.span(PH_DH2, s);
    gemm_slabs<false, true, EPI_DTANH>(t, n, y.Hd, y.I, dh2_slab(y.I), t.block.ptr, y.I, th + y.seg[3], y.I, t.da3.ptr, y.Hd, t.h2a.ptr, y.Hd + 1, s);
    sp.stop();
  }
  {
    auto sp = t.spans.span(PH_DENSE, s);
    gemm<true, false, EPI_NONE>(y.L + 1, y.Hd, n, t.za.ptr, y.L + 1, t.da3.ptr, y.Hd, G + y.seg[2], y.Hd, nullptr, 0, s);
    gemm<false, true, EPI_NONE>(n, y.L, y.Hd, t.da3.ptr, y.Hd, th + y.seg[2], y.Hd, t.dz.ptr, y.L, nullptr, 0, s);
    hipLaunchKernelGGL(mv_latent_backward_kernel, dim3(static_cast<unsigned>(ceil_div(n * y.L, BLOCK))), dim3(BLOCK), 0, s,
                       n * y.L, static_cast<int32_t>(y.L), static_cast<const float *>(t.dz.ptr),
                       static_cast<const float *>(t.ml.ptr), static_cast<const float *>(t.stdv.ptr),
                       static_cast<const float *>(t.epsv.ptr), static_cast<float>(klc / static_cast<double>(n)), t.dml.ptr);
    IRS_HIP(hipGetLastError());
    gemm<true, false, EPI_NONE>(y.H + 1, 2 * y.L, n, t.h1a.ptr, y.H + 1, t.dml.ptr, 2 * y.L, G + y.seg[1], 2 * y.L, nullptr, 0, s);
    gemm<false, true, EPI_DTANH>(n, y.H, 2 * y.L, t.dml.ptr, 2 * y.L, th + y.seg[1], 2 * y.L, t.da1.ptr, y.Hp, t.h1a.ptr, y.H + 1, s);
    sp.stop();
  }
  const double scale = std::ldexp(1.0, scale_log2(n));
  {
    auto sp = t.spans.span(PH_DW1, s);
    launch_dw1(t, x, n, scale, s);
    sp.stop();
  }
  {
    auto sp = t.spans.span(PH_ADAM, s);
    hipLaunchKernelGGL(mv_adam_kernel, dim3(static_cast<unsigned>(ceil_div(y.total, BLOCK))), dim3(BLOCK), 0, s, y.total,
                       y.w1_count, static_cast<int32_t>(y.Hp), th, t.m.ptr, t.v.ptr, G, t.acc.ptr, 1.0 / scale, t.lr,
                       static_cast<float>(bias_correction(0.9, t.n_updates)),
                       static_cast<float>(bias_correction(0.999, t.n_updates)));
    IRS_HIP(hipGetLastError());
    sp.stop();
  }
  if (want_loss) {
    hipLaunchKernelGGL(mv_loss_kernel, dim3(1), dim3(BLOCK), 0, s, static_cast<int32_t>(n),
                       static_cast<const double *>(t.row_nll.ptr), static_cast<const double *>(t.row_kl.ptr), t.loss.ptr);
    IRS_HIP(hipGetLastError());
  }
  t.klc_last = klc;
  t.n_updates++;
}

// (after a synchronisation)
static void finish_update(irs_multvae &t) {
  int32_t flag = 0;
  IRS_HIP(hipMemcpy(&flag, t.diverged.ptr, sizeof(flag), hipMemcpyDeviceToHost));
  if (flag != 0)
    throw std::runtime_error("Mult-VAE: a contribution to the gradient of W1 is not finite or reached 2^8 in magnitude: "
                             "the fit has diverged (lower learning_rate); the state is no longer usable.");
  double loss[2] = {0, 0};
  IRS_HIP(hipMemcpy(loss, t.loss.ptr, sizeof(loss), hipMemcpyDeviceToHost));
  t.nll_last = loss[0], t.kl_last = loss[1];
}

// the evaluation forward of a caller's rows, `cap` rows at a time: fn(first, n) is called with the logits of rows
// [first, first + n) in t.block, h2 in t.h2a and the softmax not yet run: fn(rows, first, n, stream)
template <class F>
static void for_caller_rows(irs_multvae &t, int64_t rows, const int64_t *indptr, const int32_t *indices, const float *data,
                            F &&fn) {
  hipStream_t s = nullptr;
  const bool timed = t.spans.enabled;
  t.spans.enabled = false;
  for (int64_t first = 0; first < rows; first += t.cap) {
    const int64_t n = std::min(t.cap, rows - first);
    const int64_t b = indptr[first], e = indptr[first + n];
    std::vector<int32_t> local(static_cast<size_t>(n) + 1);
    for (int64_t r = 0; r <= n; r++) local[static_cast<size_t>(r)] = static_cast<int32_t>(indptr[first + r] - b);
    t.c_indptr.upload(local, s);
    t.c_indices.upload(indices + b, static_cast<size_t>(e - b), s);
    t.c_data.upload(data + b, static_cast<size_t>(e - b), s);
    SparseRows x;
    x.rows = nullptr, x.indptr = t.c_indptr.ptr, x.indices = t.c_indices.ptr, x.data = t.c_data.ptr;
    x.keep = nullptr, x.keep_ptr = nullptr, x.keep_key = 0, x.threshold = 0;
    forward(t, x, n, true, 0, nullptr, s);
    fn(x, first, n, s);
    IRS_HIP(hipStreamSynchronize(s));  // (local is the source of an asynchronous copy; the buffers are reused)
  }
  t.spans.enabled = timed;
}

static void validate_caller_rows(const irs_multvae &t, int64_t rows, const int64_t *indptr, const int32_t *indices,
                                 const float *data) {
  check_arg(rows >= 0, "rows must be >= 0.");
  if (rows == 0) return;
  validate_finite_matrix(rows, t.n_items, indptr, indices, data);
}

}  // namespace mv
}  // namespace irs

using namespace irs;

extern "C" {

irs_status irs_multvae_create(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                              const float *data, int32_t dim_z, int32_t enc_hidden, int32_t dec_hidden,
                              float dropout_p, float l2_regularizer, double kl_anneal_goal, int64_t anneal_end_epoch,
                              int64_t minibatch_size, float learning_rate, uint64_t seed, const float *const *init,
                              int32_t device, irs_multvae **out) {
  return guard([&] {
    check_arg(out != nullptr, "out must not be null.");
    const int64_t nnz = validate_finite_matrix(n_users, n_items, indptr, indices, data);
    mv::validate_hyper(dim_z, enc_hidden, dec_hidden, dropout_p, l2_regularizer, kl_anneal_goal, anneal_end_epoch,
                       minibatch_size, learning_rate);
    const mv::Layout y = mv::make_layout(n_items, enc_hidden, dim_z, dec_hidden);
    if (init)
      mv::validate_tables(y, init, 1, "the initial tables must not be null.", "an initial table holds a non-finite value.");
    check_arg(device >= 0, "irspack_amd: device index out of range.");
    std::unique_ptr<irs_multvae> t(new irs_multvae());
    t->n_users = n_users, t->n_items = n_items, t->minibatch = minibatch_size, t->anneal_end_epoch = anneal_end_epoch;
    t->device = device, t->y = y, t->G = mv::lanes_per_entry(y.Hp), t->nch = mv::chunks_per_lane(y.Hp);
    t->dropout_p = dropout_p, t->l2 = l2_regularizer, t->kl_goal = kl_anneal_goal, t->lr = learning_rate, t->seed = seed;
    t->spans.enabled = env_flag("IRSPACK_AMD_MULTVAE_PHASES", false);
    t->h_indptr.resize(static_cast<size_t>(n_users) + 1);
    for (int64_t u = 0; u <= n_users; u++) t->h_indptr[static_cast<size_t>(u)] = static_cast<int32_t>(indptr[u]);
    t->h_indices.assign(indices, indices + nnz);
    t->h_data.assign(data, data + nnz);
    if (init) {
      for (int q = 0; q < mv::N_TABLES; q++) t->h_state[q].assign(init[q], init[q] + y.count(q));
    } else {
      mv::init_tables(y, seed, t->h_state);
    }
    for (int q = mv::N_TABLES; q < 3 * mv::N_TABLES; q++) t->h_state[q].assign(static_cast<size_t>(y.count(q % mv::N_TABLES)), 0.f);
    *out = t.release();  // (the device is first used by the first call that computes or copies)
  });
}

irs_status irs_multvae_run_epochs(irs_multvae *t, int64_t n_epochs) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    check_arg(n_epochs >= 0, "n_epochs must be >= 0.");
    mv::to_device(*t);
    hipStream_t s = nullptr;
    for (int64_t e = 0; e < n_epochs; e++) {
      const bool last = e + 1 == n_epochs;
      Event e0, e1;
      if (last) {
        std::fill(t->spans.ms, t->spans.ms + mv::PH_COUNT, 0.0);
        IRS_HIP(hipEventRecord(e0.e, s));
      }
      const bool timed = t->spans.enabled;
      t->spans.enabled = timed && last;
      const bpr::Perm perm = mv::epoch_perm(t->seed, t->epoch, t->n_users);
      for (int64_t first = 0; first < t->n_users; first += t->minibatch) {
        const int64_t n = std::min(t->minibatch, t->n_users - first);
        hipLaunchKernelGGL(mv::mv_order_kernel, dim3(static_cast<unsigned>(ceil_div(n, mv::BLOCK))), dim3(mv::BLOCK), 0, s,
                           perm, first, static_cast<int32_t>(n), t->users.ptr);
        IRS_HIP(hipGetLastError());
        const double klc = mv::kl_coefficient(t->kl_goal, t->n_updates, t->anneal_end_epoch, t->n_users, t->minibatch);
        mv::step(*t, n, klc, false, false, last && first + t->minibatch >= t->n_users, s);
      }
      t->spans.enabled = timed;
      t->epoch++;
      if (last) {
        IRS_HIP(hipEventRecord(e1.e, s));
        IRS_HIP(hipStreamSynchronize(s));
        t->epoch_ms = elapsed_ms(e0, e1);
        t->spans.fold();
      }
    }
    IRS_HIP(hipStreamSynchronize(s));
    mv::finish_update(*t);
  });
}

irs_status irs_multvae_order(irs_multvae *t, int64_t epoch, int64_t first, int64_t count, int32_t *users) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    check_arg(epoch >= 0, "epoch must be >= 0.");
    check_arg(first >= 0 && count >= 0 && first <= t->n_users && count <= t->n_users - first,
              "first and count must describe positions of the epoch.");
    check_arg(count == 0 || users != nullptr, "users must not be null.");
    const bpr::Perm perm = mv::epoch_perm(t->seed, epoch, t->n_users);
    for (int64_t q = 0; q < count; q++)
      users[q] = static_cast<int32_t>(bpr::permute(perm, static_cast<uint32_t>(first + q)));
  });
}

irs_status irs_multvae_noise(irs_multvae *t, int64_t update, int64_t n, const int32_t *users, uint8_t *keep, float *eps) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    check_arg(update >= 0, "update must be >= 0.");
    if (n == 0) return;
    mv::validate_batch(n, users, t->n_users, 0.0);
    mv::to_device(*t);
    hipStream_t s = nullptr;
    mv::reserve(*t, n, s);
    std::vector<int32_t> kp(static_cast<size_t>(n) + 1, 0);
    for (int64_t r = 0; r < n; r++) kp[r + 1] = kp[r] + (t->h_indptr[users[r] + 1] - t->h_indptr[users[r]]);
    const size_t n_keep = static_cast<size_t>(kp[n]), n_eps = static_cast<size_t>(n * t->y.L);
    t->keep_ptr.upload(kp, s);
    t->users.upload(users, static_cast<size_t>(n), s);
    t->keep.alloc(n_keep);
    hipLaunchKernelGGL(mv::mv_noise_kernel, dim3(static_cast<unsigned>(n)), dim3(mv::BLOCK), 0, s,
                       mv::noise_key(t->seed, update, 0), mv::noise_key(t->seed, update, 1),
                       mv::keep_threshold(t->dropout_p), static_cast<int32_t>(t->y.L),
                       static_cast<const int32_t *>(t->users.ptr), static_cast<const int32_t *>(t->indptr.ptr),
                       static_cast<const int32_t *>(t->keep_ptr.ptr), keep ? t->keep.ptr : nullptr,
                       eps ? t->eps.ptr : nullptr);
    IRS_HIP(hipGetLastError());
    if (keep && n_keep) IRS_HIP(hipMemcpyAsync(keep, t->keep.ptr, n_keep, hipMemcpyDeviceToHost, s));
    if (eps) IRS_HIP(hipMemcpyAsync(eps, t->eps.ptr, n_eps * sizeof(float), hipMemcpyDeviceToHost, s));
    IRS_HIP(hipStreamSynchronize(s));
  });
}

irs_status irs_multvae_step_batch(irs_multvae *t, int64_t n, const int32_t *users, const uint8_t *keep, const float *eps,
                                  double klc, double *nll, double *kl) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    mv::validate_batch(n, users, t->n_users, klc);
    std::vector<int32_t> kp(static_cast<size_t>(n) + 1, 0);
    for (int64_t r = 0; r < n; r++) kp[r + 1] = kp[r] + (t->h_indptr[users[r] + 1] - t->h_indptr[users[r]]);
    mv::validate_noise(kp[n], keep, n * t->y.L, eps);
    mv::to_device(*t);
    hipStream_t s = nullptr;
    mv::reserve(*t, n, s);
    t->users.upload(users, static_cast<size_t>(n), s);
    t->keep_ptr.upload(kp, s);
    if (keep) t->keep.upload(keep, static_cast<size_t>(kp[n]), s);
    if (eps) t->eps.upload(eps, static_cast<size_t>(n * t->y.L), s);
    const bool timed = t->spans.enabled;
    t->spans.enabled = false;
    mv::step(*t, n, klc, keep != nullptr, eps != nullptr, true, s);
    t->spans.enabled = timed;
    IRS_HIP(hipStreamSynchronize(s));
    mv::finish_update(*t);
    if (nll) *nll = t->nll_last;
    if (kl) *kl = t->kl_last;
  });
}

irs_status irs_multvae_gradients(irs_multvae *t, float *const *grads) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    check_arg(grads != nullptr, "grads must not be null.");
    check_arg(t->n_updates > 0 && t->on_device, "no update has been made with this handle yet.");
    mv::to_device(*t);
    IRS_HIP(hipDeviceSynchronize());
    mv::download_arena(*t, t->G_arena, grads);
  });
}

irs_status irs_multvae_get_state(irs_multvae *t, float *const *tables, int64_t *n_updates, int64_t *epoch) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    if (n_updates) *n_updates = t->n_updates;
    if (epoch) *epoch = t->epoch;
    if (tables == nullptr) return;
    if (!t->on_device) {  // (not yet uploaded: the host copies are the state)
      for (int q = 0; q < 3 * mv::N_TABLES; q++)
        if (tables[q]) std::copy(t->h_state[q].begin(), t->h_state[q].end(), tables[q]);
      return;
    }
    mv::to_device(*t);
    IRS_HIP(hipDeviceSynchronize());
    mv::download_arena(*t, t->theta, tables);
    mv::download_arena(*t, t->m, tables + mv::N_TABLES);
    mv::download_arena(*t, t->v, tables + 2 * mv::N_TABLES);
  });
}

irs_status irs_multvae_set_state(irs_multvae *t, const float *const *tables, int64_t n_updates, int64_t epoch) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    mv::validate_tables(t->y, tables, 3, "the state arrays must not be null.", "the state holds a non-finite value.");
    check_arg(n_updates >= 0, "n_updates must be >= 0.");
    check_arg(epoch >= 0, "epoch must be >= 0.");
    for (int q = 0; q < 3 * mv::N_TABLES; q++) t->h_state[q].assign(tables[q], tables[q] + t->y.count(q % mv::N_TABLES));
    if (t->on_device) {
      mv::to_device(*t);
      hipStream_t s = nullptr;
      mv::upload_arena(*t, 0, t->theta, s);
      mv::upload_arena(*t, 1, t->m, s);
      mv::upload_arena(*t, 2, t->v, s);
      t->diverged.zero(s);
      t->acc.zero(s);
      IRS_HIP(hipStreamSynchronize(s));
      for (auto &h : t->h_state) std::vector<float>().swap(h);
    }
    t->n_updates = n_updates, t->epoch = epoch;
  });
}

irs_status irs_multvae_encode(irs_multvae *t, int64_t rows, const int64_t *indptr, const int32_t *indices,
                              const float *data, float *h2, float *lse) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    mv::validate_caller_rows(*t, rows, indptr, indices, data);
    if (rows == 0) return;
    mv::to_device(*t);
    const int64_t Hd = t->y.Hd;
    mv::for_caller_rows(*t, rows, indptr, indices, data, [&](const mv::SparseRows &x, int64_t first, int64_t n, hipStream_t s) {
      mv::launch_softmax(*t, x, n, mv::SM_LSE_ONLY, s);
      if (h2)
        IRS_HIP(hipMemcpy2DAsync(h2 + first * Hd, sizeof(float) * Hd, t->h2a.ptr, sizeof(float) * (Hd + 1),
                                 sizeof(float) * Hd, static_cast<size_t>(n), hipMemcpyDeviceToHost, s));
      if (lse) IRS_HIP(hipMemcpyAsync(lse + first, t->row_lse.ptr, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    });
  });
}

irs_status irs_multvae_score(irs_multvae *t, int64_t rows, const int64_t *indptr, const int32_t *indices,
                             const float *data, float *scores) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    mv::validate_caller_rows(*t, rows, indptr, indices, data);
    if (rows == 0) return;
    check_arg(scores != nullptr, "scores must not be null.");
    mv::to_device(*t);
    const int64_t I = t->y.I;
    mv::for_caller_rows(*t, rows, indptr, indices, data, [&](const mv::SparseRows &x, int64_t first, int64_t n, hipStream_t s) {
      mv::launch_softmax(*t, x, n, mv::SM_LOG_SOFTMAX, s);
      IRS_HIP(hipMemcpyAsync(scores + first * I, t->block.ptr, sizeof(float) * n * I, hipMemcpyDeviceToHost, s));
    });
  });
}

irs_status irs_multvae_stats(irs_multvae *t, irs_multvae_stats_t *out) {
  return guard([&] {
    check_arg(t != nullptr && out != nullptr, "null argument.");
    out->n_updates = t->n_updates;
    out->epoch = t->epoch;
    out->batches_per_epoch = ceil_div(t->n_users, t->minibatch);
    out->dh2_slab = mv::dh2_slab(t->n_items);
    out->dw4_slab = mv::DW4_SLAB;
    out->scale_log2 = mv::scale_log2(std::max<int64_t>(1, std::min(t->minibatch, t->n_users)));
    out->reserved = 0;
    out->klc_next = mv::kl_coefficient(t->kl_goal, t->n_updates, t->anneal_end_epoch, t->n_users, t->minibatch);
    out->klc_last = t->klc_last, out->nll_last = t->nll_last, out->kl_last = t->kl_last;
    out->epoch_ms = t->epoch_ms;
    out->encode_ms = t->spans.ms[mv::PH_ENCODE], out->dense_ms = t->spans.ms[mv::PH_DENSE], out->logit_ms = t->spans.ms[mv::PH_LOGIT];
    out->softmax_ms = t->spans.ms[mv::PH_SOFTMAX], out->dw4_ms = t->spans.ms[mv::PH_DW4], out->dh2_ms = t->spans.ms[mv::PH_DH2];
    out->dw1_ms = t->spans.ms[mv::PH_DW1], out->adam_ms = t->spans.ms[mv::PH_ADAM];
  });
}

irs_status irs_multvae_destroy(irs_multvae *t) {
  return guard([&] { delete t; });
}

}  // extern "C"
