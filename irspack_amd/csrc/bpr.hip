// BPRFMRecommender (bpr.py of the reference wraps LightFM; the arithmetic here is this project's own synchronous
// mini-batch form of it: BPR loss, Adagrad, item biases - DESIGN.md section 14): the device side of
// irspack_amd.recommenders.bpr.BPRFMTrainer.
//
// The six tables, the filtered matrix, the fixed-point gradient sums and the row stamps live on the device for
// the life of the handle.  A batch is three ordinary launches on one stream - sampler, gradient, apply
// (bpr_kernels.hpp) -, an epoch a host loop over its batches with no copy and no synchronisation in it; the call
// synchronises once at its end and reads the divergence flag.  Every argument check comes before any device work.
// A handle made by irs_bpr_create_warp trains with the WARP loss instead: a batch is two launches, the search that
// samples, searches and adds the gradient, and the apply that skips a position without a violation.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "bpr_kernels.hpp"
#include "common.hpp"
#include "csr_checks.hpp"
#include "phase_spans.hpp"

namespace irs {
namespace bpr {

enum Phase { PH_SAMPLE = 0, PH_GRAD, PH_APPLY, PH_COUNT };
// candidate rows the WARP search keeps in flight (IRSPACK_AMD_WARP_IN_FLIGHT = 1, 2 or 4 when the handle is made)
constexpr int WARP_IN_FLIGHT = 4;

}  // namespace bpr
}  // namespace irs

struct irs_bpr {
  int64_t n_users = 0, n_items = 0, n_used = 0, batch_size = 0, epoch = 0;
  int32_t k = 0, kp = 0, device = 0, lanes = 1;
  float user_alpha = 0.f, item_alpha = 0.f, lr = 0.f;
  uint64_t seed = 0;
  unsigned long long batch_no = 0;  // of this handle, never reused: the stamps compare against it
  irs::bpr::Positives positives;
  bool on_device = false;
  std::vector<float> h_tables[6];  // U, V, b, GU, GV, Gb (unpadded) until the first device call
  irs::DeviceBuffer<float> U, V, b, GU, GV, Gb;
  irs::DeviceBuffer<unsigned long long> accU, accV, accb, stampU, stampV;
  irs::DeviceBuffer<int32_t> indptr, indices, pos_user, pos_item, t_user, t_pos, t_neg, diverged;
  irs::PhaseSpans<irs::bpr::PH_COUNT> spans;  // on with IRSPACK_AMD_BPR_PHASES
  double epoch_ms = 0;
  // loss "warp" (max_sampled >= 1; 0 is a BPR handle): the weight table, the caller's candidates, the tries of the
  // search probe and the counters of the search kernel
  int32_t max_sampled = 0, in_flight = 0;
  std::vector<double> weights;
  irs::DeviceBuffer<double> d_weights;
  irs::DeviceBuffer<int32_t> t_cand, t_tries;
  irs::DeviceBuffer<unsigned long long> counters;
  int64_t epoch_counts[3] = {0, 0, 0}, call_counts[3] = {0, 0, 0};  // positions, updates, candidates examined
};

namespace irs {
namespace bpr {

// a (rows x k) host table <-> its (rows x kp) device image; the padding holds `pad`
static void upload_table(DeviceBuffer<float> &d, const float *h, int64_t rows, int32_t k, int32_t kp, float pad,
                         hipStream_t s) {
  std::vector<float> staged(static_cast<size_t>(rows) * kp, pad);
  for (int64_t r = 0; r < rows; r++) std::memcpy(staged.data() + r * kp, h + r * k, sizeof(float) * k);
  d.upload(staged, s);
  IRS_HIP(hipStreamSynchronize(s));  // (staged is the source of an asynchronous copy)
}
static void download_table(const DeviceBuffer<float> &d, float *h, int64_t rows, int32_t k, int32_t kp, hipStream_t s) {
  if (h == nullptr) return;
  IRS_HIP(hipMemcpy2DAsync(h, sizeof(float) * k, d.ptr, sizeof(float) * kp, sizeof(float) * k,
                           static_cast<size_t>(rows), hipMemcpyDeviceToHost, s));
}

static void upload_state(irs_bpr &t, hipStream_t s) {
  const int64_t U = t.n_users, I = t.n_items;
  upload_table(t.U, t.h_tables[0].data(), U, t.k, t.kp, 0.f, s);
  upload_table(t.V, t.h_tables[1].data(), I, t.k, t.kp, 0.f, s);
  upload_table(t.b, t.h_tables[2].data(), I, 1, 1, 0.f, s);
  upload_table(t.GU, t.h_tables[3].data(), U, t.k, t.kp, 1.f, s);
  upload_table(t.GV, t.h_tables[4].data(), I, t.k, t.kp, 1.f, s);
  upload_table(t.Gb, t.h_tables[5].data(), I, 1, 1, 1.f, s);
}

// first device use of the handle: the device, the matrix, the tables, zeroed sums and stamps
static void to_device(irs_bpr &t) {
  require_device(t.device);
  if (t.on_device) return;
  hipStream_t s = nullptr;
  const size_t U = static_cast<size_t>(t.n_users), I = static_cast<size_t>(t.n_items), KP = static_cast<size_t>(t.kp);
  t.indptr.upload(t.positives.indptr, s);
  t.indices.upload(t.positives.indices, s);
  t.pos_user.upload(t.positives.pos_user, s);
  t.pos_item.upload(t.positives.pos_item, s);
  upload_state(t, s);
  t.accU.alloc(U * KP), t.accV.alloc(I * KP), t.accb.alloc(I), t.stampU.alloc(U), t.stampV.alloc(I);
  for (auto *d : {&t.accU, &t.accV, &t.accb, &t.stampU, &t.stampV}) d->zero(s);
  t.diverged.alloc(1);
  t.diverged.zero(s);
  const size_t cap = static_cast<size_t>(std::max<int64_t>(1, std::min(t.batch_size, t.n_used)));
  t.t_user.alloc(cap), t.t_pos.alloc(cap), t.t_neg.alloc(cap);
  if (t.max_sampled > 0) {
    t.d_weights.upload(t.weights, s);
    t.counters.alloc(static_cast<size_t>(WARP_COUNTER_SLOTS) * WARP_COUNTER_STRIDE);
    t.counters.zero(s);
  }
  IRS_HIP(hipStreamSynchronize(s));
  for (auto &h : t.h_tables) std::vector<float>().swap(h);
  t.on_device = true;
}

static void launch_sample(irs_bpr &t, int64_t epoch, int64_t first, int64_t count, hipStream_t s) {
  const Perm perm = make_perm(epoch_key(t.seed, epoch, 0), t.n_used);
  hipLaunchKernelGGL(bpr_sample_kernel, dim3(static_cast<unsigned>(ceil_div(count, BLOCK))), dim3(BLOCK), 0, s, perm,
                     epoch_key(t.seed, epoch, 1), first, static_cast<int32_t>(count), static_cast<int32_t>(t.n_items),
                     static_cast<const int32_t *>(t.indptr.ptr), static_cast<const int32_t *>(t.indices.ptr),
                     static_cast<const int32_t *>(t.pos_user.ptr), static_cast<const int32_t *>(t.pos_item.ptr),
                     t.t_user.ptr, t.t_pos.ptr, t.t_neg.ptr);
  IRS_HIP(hipGetLastError());
}

template <int L, int NCH> static void launch_grad(irs_bpr &t, int64_t n, double scale, hipStream_t s) {
  hipLaunchKernelGGL((bpr_grad_kernel<L, NCH>), dim3(static_cast<unsigned>(ceil_div(n * L, BLOCK))), dim3(BLOCK), 0, s,
                     static_cast<int32_t>(n), t.kp, static_cast<const int32_t *>(t.t_user.ptr),
                     static_cast<const int32_t *>(t.t_pos.ptr), static_cast<const int32_t *>(t.t_neg.ptr),
                     static_cast<const float *>(t.U.ptr), static_cast<const float *>(t.V.ptr),
                     static_cast<const float *>(t.b.ptr), t.accU.ptr, t.accV.ptr, t.accb.ptr, scale);
}

template <int L> static void launch_apply(irs_bpr &t, int64_t n, double scale, hipStream_t s) {
  hipLaunchKernelGGL((bpr_apply_kernel<L>), dim3(static_cast<unsigned>(ceil_div(n * L, BLOCK))), dim3(BLOCK), 0, s,
                     static_cast<int32_t>(n), t.kp, static_cast<const int32_t *>(t.t_user.ptr),
                     static_cast<const int32_t *>(t.t_pos.ptr), static_cast<const int32_t *>(t.t_neg.ptr), t.batch_no,
                     t.stampU.ptr, t.stampV.ptr, t.U.ptr, t.V.ptr, t.b.ptr, t.GU.ptr, t.GV.ptr, t.Gb.ptr, t.accU.ptr,
                     t.accV.ptr, t.accb.ptr, 1.0 / scale, t.user_alpha, t.item_alpha, t.lr, t.diverged.ptr);
}

// one synchronous batch on the n triples in t_user / t_pos / t_neg
static void step(irs_bpr &t, int64_t n, hipStream_t s) {
  const double scale = std::ldexp(1.0, scale_log2(n));
  t.batch_no++;
  {
    auto sp = t.spans.span(PH_GRAD, s);
    switch (t.lanes) {
      case 1: launch_grad<1, 1>(t, n, scale, s); break;
      case 2: launch_grad<2, 1>(t, n, scale, s); break;
      case 4: launch_grad<4, 1>(t, n, scale, s); break;
      case 8: launch_grad<8, 1>(t, n, scale, s); break;
      case 16: launch_grad<16, 1>(t, n, scale, s); break;
      case 32: launch_grad<32, 1>(t, n, scale, s); break;
      default:
        if (t.kp <= 256) launch_grad<64, 1>(t, n, scale, s);
        else launch_grad<64, 2>(t, n, scale, s);
    }
    IRS_HIP(hipGetLastError());
    sp.stop();
  }
  auto sp = t.spans.span(PH_APPLY, s);
  switch (t.lanes) {
    case 1: launch_apply<1>(t, n, scale, s); break;
    case 2: launch_apply<2>(t, n, scale, s); break;
    case 4: launch_apply<4>(t, n, scale, s); break;
    case 8: launch_apply<8>(t, n, scale, s); break;
    case 16: launch_apply<16>(t, n, scale, s); break;
    case 32: launch_apply<32>(t, n, scale, s); break;
    default: launch_apply<64>(t, n, scale, s);
  }
  IRS_HIP(hipGetLastError());
  sp.stop();
}

// ---- WARP: the search (with GEN: on the epoch's own candidates; with GRAD: and its gradient), then the apply ----
template <int L, int NCH, int F, bool GEN, bool GRAD>
static void launch_search(irs_bpr &t, int64_t n, int64_t epoch, int64_t first, double scale, hipStream_t s) {
  const Perm perm = make_perm(epoch_key(t.seed, epoch, 0), std::max<int64_t>(1, t.n_used));
  hipLaunchKernelGGL((warp_search_kernel<L, NCH, F, GEN, GRAD>), dim3(static_cast<unsigned>(ceil_div(n * L, BLOCK))),
                     dim3(BLOCK), 0, s, static_cast<int32_t>(n), t.kp, t.max_sampled, perm, warp_key(t.seed, epoch),
                     first, static_cast<int32_t>(t.n_items), static_cast<const int32_t *>(t.indptr.ptr),
                     static_cast<const int32_t *>(t.indices.ptr), static_cast<const int32_t *>(t.pos_user.ptr),
                     static_cast<const int32_t *>(t.pos_item.ptr), static_cast<const int32_t *>(t.t_cand.ptr),
                     static_cast<const double *>(t.d_weights.ptr), t.t_user.ptr, t.t_pos.ptr, t.t_neg.ptr,
                     GRAD ? nullptr : t.t_tries.ptr, static_cast<const float *>(t.U.ptr),
                     static_cast<const float *>(t.V.ptr), static_cast<const float *>(t.b.ptr), t.accU.ptr, t.accV.ptr,
                     t.accb.ptr, scale, t.counters.ptr);
}

template <int L, int NCH, bool GEN, bool GRAD>
static void launch_search_in_flight(irs_bpr &t, int64_t n, int64_t epoch, int64_t first, double scale, hipStream_t s) {
  switch (t.in_flight) {
    case 1: launch_search<L, NCH, 1, GEN, GRAD>(t, n, epoch, first, scale, s); break;
    case 2: launch_search<L, NCH, 2, GEN, GRAD>(t, n, epoch, first, scale, s); break;
    default: launch_search<L, NCH, 4, GEN, GRAD>(t, n, epoch, first, scale, s);
  }
}

template <bool GEN, bool GRAD>
static void launch_search_lanes(irs_bpr &t, int64_t n, int64_t epoch, int64_t first, double scale, hipStream_t s) {
  switch (t.lanes) {
    case 1: launch_search_in_flight<1, 1, GEN, GRAD>(t, n, epoch, first, scale, s); break;
    case 2: launch_search_in_flight<2, 1, GEN, GRAD>(t, n, epoch, first, scale, s); break;
    case 4: launch_search_in_flight<4, 1, GEN, GRAD>(t, n, epoch, first, scale, s); break;
    case 8: launch_search_in_flight<8, 1, GEN, GRAD>(t, n, epoch, first, scale, s); break;
    case 16: launch_search_in_flight<16, 1, GEN, GRAD>(t, n, epoch, first, scale, s); break;
    case 32: launch_search_in_flight<32, 1, GEN, GRAD>(t, n, epoch, first, scale, s); break;
    default:
      if (t.kp <= 256) launch_search_in_flight<64, 1, GEN, GRAD>(t, n, epoch, first, scale, s);
      else launch_search_in_flight<64, 2, GEN, GRAD>(t, n, epoch, first, scale, s);
  }
  IRS_HIP(hipGetLastError());
}

template <int L> static void launch_warp_apply(irs_bpr &t, int64_t n, double scale, hipStream_t s) {
  hipLaunchKernelGGL((warp_apply_kernel<L>), dim3(static_cast<unsigned>(ceil_div(n * L, BLOCK))), dim3(BLOCK), 0, s,
                     static_cast<int32_t>(n), t.kp, static_cast<const int32_t *>(t.t_user.ptr),
                     static_cast<const int32_t *>(t.t_pos.ptr), static_cast<const int32_t *>(t.t_neg.ptr), t.batch_no,
                     t.stampU.ptr, t.stampV.ptr, t.U.ptr, t.V.ptr, t.b.ptr, t.GU.ptr, t.GV.ptr, t.Gb.ptr, t.accU.ptr,
                     t.accV.ptr, t.accb.ptr, 1.0 / scale, t.user_alpha, t.item_alpha, t.lr, t.diverged.ptr);
}

// one synchronous WARP batch of n positions: the epoch's [first, first + n) with GEN, else those in t_user / t_pos
// with their candidates in t_cand
template <bool GEN> static void warp_step(irs_bpr &t, int64_t n, int64_t epoch, int64_t first, hipStream_t s) {
  const double scale = std::ldexp(1.0, warp_scale_log2(n));
  t.batch_no++;
  {
    auto sp = t.spans.span(PH_GRAD, s);
    launch_search_lanes<GEN, true>(t, n, epoch, first, scale, s);
    sp.stop();
  }
  auto sp = t.spans.span(PH_APPLY, s);
  switch (t.lanes) {
    case 1: launch_warp_apply<1>(t, n, scale, s); break;
    case 2: launch_warp_apply<2>(t, n, scale, s); break;
    case 4: launch_warp_apply<4>(t, n, scale, s); break;
    case 8: launch_warp_apply<8>(t, n, scale, s); break;
    case 16: launch_warp_apply<16>(t, n, scale, s); break;
    case 32: launch_warp_apply<32>(t, n, scale, s); break;
    default: launch_warp_apply<64>(t, n, scale, s);
  }
  IRS_HIP(hipGetLastError());
  sp.stop();
}

static void launch_candidates(irs_bpr &t, int64_t epoch, int64_t first, int64_t count, hipStream_t s) {
  const Perm perm = make_perm(epoch_key(t.seed, epoch, 0), t.n_used);
  hipLaunchKernelGGL(warp_candidates_kernel, dim3(static_cast<unsigned>(ceil_div(count * t.max_sampled, BLOCK))),
                     dim3(BLOCK), 0, s, perm, warp_key(t.seed, epoch), first, static_cast<int32_t>(count),
                     t.max_sampled, static_cast<int32_t>(t.n_items), static_cast<const int32_t *>(t.indptr.ptr),
                     static_cast<const int32_t *>(t.indices.ptr), static_cast<const int32_t *>(t.pos_user.ptr),
                     static_cast<const int32_t *>(t.pos_item.ptr), t.t_user.ptr, t.t_pos.ptr, t.t_cand.ptr);
  IRS_HIP(hipGetLastError());
}

// (after a synchronisation) the counters of the search launches since they were last set to zero
static void read_counters(irs_bpr &t, int64_t *out) {
  std::vector<unsigned long long> c(t.counters.count);
  IRS_HIP(hipMemcpy(c.data(), t.counters.ptr, c.size() * sizeof(c[0]), hipMemcpyDeviceToHost));
  for (int q = 0; q < 3; q++) out[q] = 0;
  for (int slot = 0; slot < WARP_COUNTER_SLOTS; slot++)
    for (int q = 0; q < 3; q++) out[q] += static_cast<int64_t>(c[static_cast<size_t>(slot) * WARP_COUNTER_STRIDE + q]);
}

// the caller's positions and candidates into t_user / t_pos / t_cand
static void upload_warp_batch(irs_bpr &t, int64_t n, const int32_t *users, const int32_t *pos, const int32_t *cand,
                              hipStream_t s) {
  const size_t cnt = static_cast<size_t>(n);
  if (cnt > t.t_user.count) t.t_user.alloc(cnt), t.t_pos.alloc(cnt), t.t_neg.alloc(cnt);
  t.t_cand.alloc(cnt * t.max_sampled);
  t.t_tries.alloc(cnt);
  IRS_HIP(hipMemcpyAsync(t.t_user.ptr, users, cnt * sizeof(int32_t), hipMemcpyHostToDevice, s));
  IRS_HIP(hipMemcpyAsync(t.t_pos.ptr, pos, cnt * sizeof(int32_t), hipMemcpyHostToDevice, s));
  IRS_HIP(hipMemcpyAsync(t.t_cand.ptr, cand, cnt * t.max_sampled * sizeof(int32_t), hipMemcpyHostToDevice, s));
  t.counters.zero(s);
}

static void require_warp(const irs_bpr *t) {
  check_arg(t != nullptr, "null handle.");
  check_arg(t->max_sampled > 0, "this call needs a handle made by irs_bpr_create_warp.");
}

// (after a synchronisation) a parameter left the range the fixed-point sums are scaled for
static void check_diverged(irs_bpr &t) {
  int32_t flag = 0;
  IRS_HIP(hipMemcpy(&flag, t.diverged.ptr, sizeof(flag), hipMemcpyDeviceToHost));
  if (flag != 0)
    throw std::runtime_error("BPR: a parameter is not finite or reached 2^8 in magnitude: the fit has diverged "
                             "(lower learning_rate); the state is no longer usable.");
}

static void fill_state(irs_bpr &t, const float *U, const float *V, const float *b, const float *GU, const float *GV,
                       const float *Gb) {
  const size_t nu = static_cast<size_t>(t.n_users) * t.k, ni = static_cast<size_t>(t.n_items) * t.k,
               nb = static_cast<size_t>(t.n_items);
  const float *src[6] = {U, V, b, GU, GV, Gb};
  const size_t len[6] = {nu, ni, nb, nu, ni, nb};
  for (int q = 0; q < 6; q++) t.h_tables[q].assign(src[q], src[q] + len[q]);
}

// max_sampled: 0 for the BPR loss, else WARP's (checked by the caller)
static void create(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices, const float *data,
                   int32_t k, float user_alpha, float item_alpha, float learning_rate, int64_t batch_size,
                   uint64_t seed, const float *user_init, const float *item_init, int32_t device, int32_t max_sampled,
                   irs_bpr **out) {
  check_arg(out != nullptr, "out must not be null.");
  validate_finite_matrix(n_users, n_items, indptr, indices, data);
  bpr::validate_hyper(k, user_alpha, item_alpha, learning_rate, batch_size);
  if (user_init)
    bpr::validate_table(user_init, n_users * k, "the initial user table holds a non-finite value.",
                        "the initial user table holds a value of magnitude >= 2^8.");
  if (item_init)
    bpr::validate_table(item_init, n_items * k, "the initial item table holds a non-finite value.",
                        "the initial item table holds a value of magnitude >= 2^8.");
  check_arg(device >= 0, "irspack_amd: device index out of range.");
  std::unique_ptr<irs_bpr> t(new irs_bpr());
  t->n_users = n_users, t->n_items = n_items, t->k = k, t->kp = (k + 3) / 4 * 4, t->device = device;
  t->lanes = bpr::lanes_per_triple(k);
  t->user_alpha = user_alpha, t->item_alpha = item_alpha, t->lr = learning_rate, t->batch_size = batch_size;
  t->seed = seed;
  t->spans.enabled = env_flag("IRSPACK_AMD_BPR_PHASES", false);
  t->positives = bpr::filter_positives(n_users, n_items, indptr, indices, data);
  t->n_used = static_cast<int64_t>(t->positives.pos_user.size());
  const size_t nu = static_cast<size_t>(n_users) * k, ni = static_cast<size_t>(n_items) * k;
  std::vector<float> U(nu), V(ni), b(static_cast<size_t>(n_items), 0.f), GU(nu, 1.f), GV(ni, 1.f), Gb(b.size(), 1.f);
  for (size_t q = 0; q < nu; q++) U[q] = user_init ? user_init[q] : bpr::init_value(seed, 0, q, k);
  for (size_t q = 0; q < ni; q++) V[q] = item_init ? item_init[q] : bpr::init_value(seed, 1, q, k);
  bpr::fill_state(*t, U.data(), V.data(), b.data(), GU.data(), GV.data(), Gb.data());
  if (max_sampled > 0) {
    t->max_sampled = max_sampled;
    t->weights = bpr::warp_weights(n_items, max_sampled);
    const char *in_flight = std::getenv("IRSPACK_AMD_WARP_IN_FLIGHT");
    t->in_flight = in_flight ? std::atoi(in_flight) : WARP_IN_FLIGHT;
    check_arg(t->in_flight == 1 || t->in_flight == 2 || t->in_flight == 4,
              "IRSPACK_AMD_WARP_IN_FLIGHT must be 1, 2 or 4.");
  }
  *out = t.release();  // (the device is first used by the first call that computes or copies)
}

}  // namespace bpr
}  // namespace irs

using namespace irs;

extern "C" {

irs_status irs_bpr_create(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                          const float *data, int32_t k, float user_alpha, float item_alpha, float learning_rate,
                          int64_t batch_size, uint64_t seed, const float *user_init, const float *item_init,
                          int32_t device, irs_bpr **out) {
  return guard([&] {
    bpr::create(n_users, n_items, indptr, indices, data, k, user_alpha, item_alpha, learning_rate, batch_size, seed,
                user_init, item_init, device, 0, out);
  });
}

irs_status irs_bpr_create_warp(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                               const float *data, int32_t k, float user_alpha, float item_alpha, float learning_rate,
                               int64_t batch_size, uint64_t seed, const float *user_init, const float *item_init,
                               int32_t device, int32_t max_sampled, irs_bpr **out) {
  return guard([&] {
    check_arg(out != nullptr, "out must not be null.");
    bpr::validate_max_sampled(max_sampled);
    bpr::create(n_users, n_items, indptr, indices, data, k, user_alpha, item_alpha, learning_rate, batch_size, seed,
                user_init, item_init, device, max_sampled, out);
  });
}

irs_status irs_bpr_run_epochs(irs_bpr *t, int64_t n_epochs) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    check_arg(n_epochs >= 0, "n_epochs must be >= 0.");
    bpr::to_device(*t);
    hipStream_t s = nullptr;
    for (int64_t e = 0; e < n_epochs; e++) {
      const bool last = e + 1 == n_epochs;
      Event e0, e1;
      if (last) {
        std::fill(t->spans.ms, t->spans.ms + bpr::PH_COUNT, 0.0);
        IRS_HIP(hipEventRecord(e0.e, s));
      }
      const bool timed = t->spans.enabled;
      t->spans.enabled = timed && last;
      const bool warp = t->max_sampled > 0;
      if (warp && last) t->counters.zero(s);
      for (int64_t first = 0; first < t->n_used; first += t->batch_size) {
        const int64_t n = std::min(t->batch_size, t->n_used - first);
        if (warp) {  // (no sampler launch: the search computes its positions and candidates)
          bpr::warp_step<true>(*t, n, t->epoch, first, s);
          continue;
        }
        auto sp = t->spans.span(bpr::PH_SAMPLE, s);
        bpr::launch_sample(*t, t->epoch, first, n, s);
        sp.stop();
        bpr::step(*t, n, s);
      }
      t->spans.enabled = timed;
      t->epoch++;
      if (last) {
        IRS_HIP(hipEventRecord(e1.e, s));
        IRS_HIP(hipStreamSynchronize(s));
        t->epoch_ms = elapsed_ms(e0, e1);
        t->spans.fold();
        if (warp) {
          bpr::read_counters(*t, t->epoch_counts);
          std::copy(t->epoch_counts, t->epoch_counts + 3, t->call_counts);
        }
      }
    }
    IRS_HIP(hipStreamSynchronize(s));
    bpr::check_diverged(*t);
  });
}

irs_status irs_bpr_sample(irs_bpr *t, int64_t epoch, int64_t first, int64_t count, int32_t *users, int32_t *pos,
                          int32_t *neg) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    check_arg(t->max_sampled == 0, "a WARP handle has no single negative per position: use irs_bpr_warp_candidates.");
    check_arg(epoch >= 0, "epoch must be >= 0.");
    check_arg(first >= 0 && count >= 0 && first <= t->n_used && count <= t->n_used - first,
              "first and count must describe positions of the epoch.");
    check_arg(count == 0 || (users && pos && neg), "the triple arrays must not be null.");
    bpr::to_device(*t);
    hipStream_t s = nullptr;
    const bool timed = t->spans.enabled;
    t->spans.enabled = false;
    const int64_t cap = static_cast<int64_t>(t->t_user.count);
    for (int64_t done = 0; done < count; done += cap) {
      const int64_t n = std::min(cap, count - done);
      bpr::launch_sample(*t, epoch, first + done, n, s);
      const size_t bytes = static_cast<size_t>(n) * sizeof(int32_t);
      IRS_HIP(hipMemcpyAsync(users + done, t->t_user.ptr, bytes, hipMemcpyDeviceToHost, s));
      IRS_HIP(hipMemcpyAsync(pos + done, t->t_pos.ptr, bytes, hipMemcpyDeviceToHost, s));
      IRS_HIP(hipMemcpyAsync(neg + done, t->t_neg.ptr, bytes, hipMemcpyDeviceToHost, s));
    }
    IRS_HIP(hipStreamSynchronize(s));
    t->spans.enabled = timed;
  });
}

irs_status irs_bpr_step_triples(irs_bpr *t, int64_t n, const int32_t *users, const int32_t *pos, const int32_t *neg) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    check_arg(t->max_sampled == 0, "a WARP handle steps on candidates, not on triples: use irs_bpr_warp_step.");
    bpr::validate_triples(n, users, pos, neg, t->n_users, t->n_items);
    if (n == 0) return;
    bpr::to_device(*t);
    hipStream_t s = nullptr;
    const size_t cnt = static_cast<size_t>(n);
    if (cnt > t->t_user.count) t->t_user.alloc(cnt), t->t_pos.alloc(cnt), t->t_neg.alloc(cnt);
    IRS_HIP(hipMemcpyAsync(t->t_user.ptr, users, cnt * sizeof(int32_t), hipMemcpyHostToDevice, s));
    IRS_HIP(hipMemcpyAsync(t->t_pos.ptr, pos, cnt * sizeof(int32_t), hipMemcpyHostToDevice, s));
    IRS_HIP(hipMemcpyAsync(t->t_neg.ptr, neg, cnt * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const bool timed = t->spans.enabled;
    t->spans.enabled = false;
    bpr::step(*t, n, s);
    t->spans.enabled = timed;
    IRS_HIP(hipStreamSynchronize(s));
    bpr::check_diverged(*t);
  });
}

irs_status irs_bpr_get_state(irs_bpr *t, float *U, float *V, float *b, float *GU, float *GV, float *Gb,
                             int64_t *epoch) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    if (epoch) *epoch = t->epoch;
    if (!t->on_device) {  // (not yet uploaded: the host copies are the state)
      float *dst[6] = {U, V, b, GU, GV, Gb};
      for (int q = 0; q < 6; q++)
        if (dst[q]) std::copy(t->h_tables[q].begin(), t->h_tables[q].end(), dst[q]);
      return;
    }
    bpr::to_device(*t);
    hipStream_t s = nullptr;
    bpr::download_table(t->U, U, t->n_users, t->k, t->kp, s);
    bpr::download_table(t->V, V, t->n_items, t->k, t->kp, s);
    bpr::download_table(t->b, b, t->n_items, 1, 1, s);
    bpr::download_table(t->GU, GU, t->n_users, t->k, t->kp, s);
    bpr::download_table(t->GV, GV, t->n_items, t->k, t->kp, s);
    bpr::download_table(t->Gb, Gb, t->n_items, 1, 1, s);
    IRS_HIP(hipStreamSynchronize(s));
  });
}

irs_status irs_bpr_set_state(irs_bpr *t, const float *U, const float *V, const float *b, const float *GU,
                             const float *GV, const float *Gb, int64_t epoch) {
  return guard([&] {
    check_arg(t != nullptr, "null handle.");
    check_arg(U && V && b && GU && GV && Gb, "the state arrays must not be null.");
    check_arg(epoch >= 0, "epoch must be >= 0.");
    const int64_t nu = t->n_users * t->k, ni = t->n_items * t->k;
    const char *nf = "the state holds a non-finite value.", *big = "the state holds a value of magnitude >= 2^8.";
    bpr::validate_table(U, nu, nf, big);
    bpr::validate_table(V, ni, nf, big);
    bpr::validate_table(b, t->n_items, nf, big);
    bpr::validate_accumulator(GU, nu);
    bpr::validate_accumulator(GV, ni);
    bpr::validate_accumulator(Gb, t->n_items);
    bpr::fill_state(*t, U, V, b, GU, GV, Gb);
    if (t->on_device) {
      bpr::upload_state(*t, nullptr);
      t->diverged.zero(nullptr);
      for (auto &h : t->h_tables) std::vector<float>().swap(h);
    }
    t->epoch = epoch;
  });
}

irs_status irs_bpr_stats(irs_bpr *t, irs_bpr_stats_t *out) {
  return guard([&] {
    check_arg(t != nullptr && out != nullptr, "null argument.");
    out->n_positives = t->positives.n_positives;
    out->n_skipped_full_rows = t->positives.n_skipped_rows;
    out->n_skipped_positives = t->positives.n_skipped_positives;
    out->batches_per_epoch = ceil_div(t->n_used, t->batch_size);
    out->lanes_per_triple = t->lanes;
    out->scale_log2 = bpr::scale_log2(std::max<int64_t>(1, std::min(t->batch_size, t->n_used)));
    out->epoch_ms = t->epoch_ms;
    out->sample_ms = t->spans.ms[bpr::PH_SAMPLE];
    out->grad_ms = t->spans.ms[bpr::PH_GRAD];
    out->apply_ms = t->spans.ms[bpr::PH_APPLY];
  });
}

irs_status irs_bpr_warp_candidates(irs_bpr *t, int64_t epoch, int64_t first, int64_t count, int32_t *users,
                                   int32_t *pos, int32_t *cand) {
  return guard([&] {
    bpr::require_warp(t);
    check_arg(epoch >= 0, "epoch must be >= 0.");
    check_arg(first >= 0 && count >= 0 && first <= t->n_used && count <= t->n_used - first,
              "first and count must describe positions of the epoch.");
    check_arg(count == 0 || (users && pos && cand), "the position and candidate arrays must not be null.");
    if (count == 0) return;
    bpr::to_device(*t);
    hipStream_t s = nullptr;
    const int64_t cap = static_cast<int64_t>(t->t_user.count), ms = t->max_sampled;
    t->t_cand.alloc(static_cast<size_t>(std::min(cap, count) * ms));
    for (int64_t done = 0; done < count; done += cap) {
      const int64_t n = std::min(cap, count - done);
      bpr::launch_candidates(*t, epoch, first + done, n, s);
      const size_t bytes = static_cast<size_t>(n) * sizeof(int32_t);
      IRS_HIP(hipMemcpyAsync(users + done, t->t_user.ptr, bytes, hipMemcpyDeviceToHost, s));
      IRS_HIP(hipMemcpyAsync(pos + done, t->t_pos.ptr, bytes, hipMemcpyDeviceToHost, s));
      IRS_HIP(hipMemcpyAsync(cand + done * ms, t->t_cand.ptr, bytes * ms, hipMemcpyDeviceToHost, s));
    }
    IRS_HIP(hipStreamSynchronize(s));
  });
}

irs_status irs_bpr_warp_search(irs_bpr *t, int64_t n, const int32_t *users, const int32_t *pos, const int32_t *cand,
                               int32_t *neg_out, int32_t *tries_out) {
  return guard([&] {
    bpr::require_warp(t);
    bpr::validate_warp_batch(n, users, pos, cand, t->max_sampled, t->n_users, t->n_items);
    check_arg(n == 0 || (neg_out && tries_out), "the output arrays must not be null.");
    std::fill(t->call_counts, t->call_counts + 3, int64_t(0));
    if (n == 0) return;
    bpr::to_device(*t);
    hipStream_t s = nullptr;
    bpr::upload_warp_batch(*t, n, users, pos, cand, s);
    bpr::launch_search_lanes<false, false>(*t, n, 0, 0, 1.0, s);
    const size_t bytes = static_cast<size_t>(n) * sizeof(int32_t);
    IRS_HIP(hipMemcpyAsync(neg_out, t->t_neg.ptr, bytes, hipMemcpyDeviceToHost, s));
    IRS_HIP(hipMemcpyAsync(tries_out, t->t_tries.ptr, bytes, hipMemcpyDeviceToHost, s));
    IRS_HIP(hipStreamSynchronize(s));
    bpr::read_counters(*t, t->call_counts);
  });
}

irs_status irs_bpr_warp_step(irs_bpr *t, int64_t n, const int32_t *users, const int32_t *pos, const int32_t *cand) {
  return guard([&] {
    bpr::require_warp(t);
    bpr::validate_warp_batch(n, users, pos, cand, t->max_sampled, t->n_users, t->n_items);
    std::fill(t->call_counts, t->call_counts + 3, int64_t(0));
    if (n == 0) return;
    bpr::to_device(*t);
    hipStream_t s = nullptr;
    bpr::upload_warp_batch(*t, n, users, pos, cand, s);
    const bool timed = t->spans.enabled;
    t->spans.enabled = false;
    bpr::warp_step<false>(*t, n, 0, 0, s);
    t->spans.enabled = timed;
    IRS_HIP(hipStreamSynchronize(s));
    bpr::read_counters(*t, t->call_counts);
    bpr::check_diverged(*t);
  });
}

irs_status irs_bpr_warp_stats(irs_bpr *t, irs_bpr_warp_stats_t *out) {
  return guard([&] {
    bpr::require_warp(t);
    check_arg(out != nullptr, "null argument.");
    out->max_sampled = t->max_sampled;
    out->scale_log2 = bpr::warp_scale_log2(std::max<int64_t>(1, std::min(t->batch_size, t->n_used)));
    out->in_flight = t->in_flight;
    out->reserved = 0;
    out->epoch_positions = t->epoch_counts[0], out->epoch_updates = t->epoch_counts[1];
    out->epoch_tries = t->epoch_counts[2];
    out->call_positions = t->call_counts[0], out->call_updates = t->call_counts[1];
    out->call_tries = t->call_counts[2];
    out->epoch_ms = t->epoch_ms;
    out->search_ms = t->spans.ms[bpr::PH_GRAD];
    out->apply_ms = t->spans.ms[bpr::PH_APPLY];
  });
}

irs_status irs_bpr_destroy(irs_bpr *t) {
  return guard([&] { delete t; });
}

}  // extern "C"
