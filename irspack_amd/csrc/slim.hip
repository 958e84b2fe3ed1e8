// SLIM: elastic-net coordinate descent per target item on the device (the reference's
// cpp_source/util.hpp:228-424, bound as slim_weight_positive_only / slim_weight_allow_negative in
// cpp_source/util.cpp:31-40).  Host side of the C ABI; the kernels are in slim_kernels.hpp.
#include <algorithm>
#include <chrono>
#include <mutex>

#include "common.hpp"
#include "csr_checks.hpp"
#include "gram_setup.hpp"
#include "phase_spans.hpp"
#include "slim_kernels.hpp"

struct irs_slim_result {
  int64_t cols = 0;
  std::vector<int64_t> col_ptr;
  std::vector<int32_t> indices;
  std::vector<float> data;
  double gram_ms = 0.0, descent_ms = 0.0, emit_ms = 0.0;
  int64_t sweeps_total = 0, updates_total = 0;
  irs::slim::LaunchPlan plan;  // of the descent launch (all zero when the call did no device work)
  int64_t lds_per_block = 0;   // sharedMemPerBlock as the device reported it
};

namespace irs {
namespace slim {

// the large dynamic-LDS limit of a descent kernel is raised once per kernel and device, not per launch
template <class K> static void allow_dynamic_lds(K kernel, int which, int device, int bytes) {
  static std::mutex mu;
  static std::vector<uint32_t> done;  // per device: bit `which`
  std::lock_guard<std::mutex> lock(mu);
  if (done.size() <= static_cast<size_t>(device)) done.resize(static_cast<size_t>(device) + 1, 0u);
  if (done[device] & (1u << which)) return;
  IRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              bytes));
  done[device] |= 1u << which;
}

static void fit(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices, const float *data,
                bool positive_only, int64_t n_iter, float l2, float l1, float tol, int64_t top_k, int device,
                irs_slim_result &res) {
  res.cols = cols;
  res.col_ptr.assign(static_cast<size_t>(cols) + 1, 0);
  const int64_t nnz = indptr[rows];
  // an empty matrix has G = 0: every candidate is -l1 / l2 <= 0 (or 0 / 0), every coefficient stays 0
  if (cols == 0 || nnz == 0) return;
  require_device(device);
  hipStream_t s = nullptr;
  hipDeviceProp_t prop;
  IRS_HIP(hipGetDeviceProperties(&prop, device));
  const int n_items = static_cast<int>(cols);
  const size_t I = static_cast<size_t>(cols);

  // where the running vector lives, and the launch shape that follows from it
  const LaunchPlan plan = plan_launch(cols, prop.sharedMemPerBlock, prop.maxSharedMemoryPerMultiProcessor,
                                      prop.multiProcessorCount, env_flag("IRSPACK_AMD_SLIM_LDS", true));
  const bool lds_r = plan.lds_r;
  const int lds_bytes = plan.lds_bytes, threads = plan.threads, n_wg = plan.n_wg;
  res.plan = plan;
  res.lds_per_block = static_cast<int64_t>(prop.sharedMemPerBlock);

  // memory: G and the dense W (4 I^2 bytes each), the matrix twice, the q rows of the global path
  size_t free_b = 0, total_b = 0;
  IRS_HIP(hipMemGetInfo(&free_b, &total_b));
  const double need = 8.0 * double(I) * double(I) + 16.0 * double(nnz) * 2.0 + 64.0 * double(I) +
                      (lds_r ? 0.0 : 4.0 * double(I) * n_wg) + double(size_t(256) << 20);
  if (need > double(free_b))
    throw std::runtime_error("SLIM: the dense item Gram matrix and coefficient matrix of " + std::to_string(cols) +
                             " items need " + std::to_string(static_cast<int64_t>(need / 1048576.0)) +
                             " MiB of device memory, " + std::to_string(free_b >> 20) +
                             " MiB are free (a sparse Gram path is not implemented).");

  Event e0, e1, e2, e3;
  IRS_HIP(hipEventRecord(e0.e, s));
  // X by rows and by columns on the device, G = X^T X
  GramInput in;
  DeviceBuffer<int32_t> &d_order = in.order;
  DeviceBuffer<float> d_G, d_W, d_diag, d_scratch;
  d_G.alloc(I * I);
  d_G.zero(s);
  d_diag.alloc(I);
  upload_and_gram(rows, cols, indptr, indices, data, in, d_G.ptr, cols, s);
  hipLaunchKernelGGL(gram_diag_kernel, dim3(static_cast<unsigned>(ceil_div(cols, 256))), dim3(256), 0, s,
                     static_cast<const float *>(d_G.ptr), n_items, d_diag.ptr);
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipEventRecord(e1.e, s));

  // descent
  d_W.alloc(I * I);
  d_W.zero(s);
  if (!lds_r) d_scratch.alloc(I * static_cast<size_t>(n_wg));
  DeviceBuffer<int32_t> d_cursor;
  DeviceBuffer<unsigned long long> d_stats;
  d_cursor.alloc(1);
  d_cursor.zero(s);
  d_stats.alloc(2);
  d_stats.zero(s);
  auto launch = [&](auto kernel, int which) {
    if (plan.raise_dynamic_lds) allow_dynamic_lds(kernel, which, device, static_cast<int>(prop.sharedMemPerBlock));
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(n_wg)), dim3(static_cast<unsigned>(threads)),
                       static_cast<size_t>(lds_bytes), s, static_cast<const float *>(d_G.ptr),
                       static_cast<const float *>(d_diag.ptr), static_cast<const int32_t *>(d_order.ptr), n_items,
                       n_iter, l2, l1, tol, d_W.ptr, d_scratch.ptr, d_cursor.ptr, d_stats.ptr);
  };
  if (positive_only) {
    if (lds_r) launch(slim_descent_kernel<true, true>, 0);
    else launch(slim_descent_kernel<true, false>, 1);
  } else {
    if (lds_r) launch(slim_descent_kernel<false, true>, 2);
    else launch(slim_descent_kernel<false, false>, 3);
  }
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipEventRecord(e2.e, s));

  // emit: counts, prefix sum, compaction; then one read-back of the arrays
  DeviceBuffer<int32_t> d_raw, d_cnt, d_oidx;
  DeviceBuffer<int64_t> d_colptr;
  DeviceBuffer<float> d_oval;
  d_raw.alloc(I);
  d_cnt.alloc(I);
  d_colptr.alloc(I + 1);
  hipLaunchKernelGGL(slim_count_kernel, dim3(static_cast<unsigned>(cols)), dim3(256), 0, s,
                     static_cast<const float *>(d_W.ptr), n_items, top_k, d_raw.ptr, d_cnt.ptr);
  hipLaunchKernelGGL(slim_scan_kernel, dim3(1), dim3(1024), 0, s, static_cast<const int32_t *>(d_cnt.ptr), n_items,
                     d_colptr.ptr);
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipMemcpyAsync(res.col_ptr.data(), d_colptr.ptr, (I + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  IRS_HIP(hipStreamSynchronize(s));
  const int64_t out_nnz = res.col_ptr[I];
  if (out_nnz < 0 || static_cast<double>(out_nnz) > double(I) * double(I))
    throw std::runtime_error("SLIM: inconsistent result size.");
  res.indices.resize(static_cast<size_t>(out_nnz));
  res.data.resize(static_cast<size_t>(out_nnz));
  if (out_nnz > 0) {
    d_oidx.alloc(static_cast<size_t>(out_nnz));
    d_oval.alloc(static_cast<size_t>(out_nnz));
    hipLaunchKernelGGL(slim_emit_kernel, dim3(static_cast<unsigned>(cols)), dim3(256), 0, s,
                       static_cast<const float *>(d_W.ptr), n_items, static_cast<const int32_t *>(d_raw.ptr),
                       static_cast<const int32_t *>(d_cnt.ptr), static_cast<const int64_t *>(d_colptr.ptr),
                       d_oidx.ptr, d_oval.ptr);
    IRS_HIP(hipGetLastError());
  }
  IRS_HIP(hipEventRecord(e3.e, s));
  if (out_nnz > 0) {
    IRS_HIP(hipMemcpyAsync(res.indices.data(), d_oidx.ptr, res.indices.size() * sizeof(int32_t),
                           hipMemcpyDeviceToHost, s));
    IRS_HIP(hipMemcpyAsync(res.data.data(), d_oval.ptr, res.data.size() * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  unsigned long long stats[2] = {0, 0};
  IRS_HIP(hipMemcpyAsync(stats, d_stats.ptr, sizeof(stats), hipMemcpyDeviceToHost, s));
  IRS_HIP(hipStreamSynchronize(s));
  res.gram_ms = elapsed_ms(e0, e1);
  res.descent_ms = elapsed_ms(e1, e2);
  res.emit_ms = elapsed_ms(e2, e3);
  res.sweeps_total = static_cast<int64_t>(stats[0]);
  res.updates_total = static_cast<int64_t>(stats[1]);
}

}  // namespace slim
}  // namespace irs

using namespace irs;

extern "C" {

irs_status irs_slim_fit(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices,
                        const float *data, int32_t positive_only, int64_t n_iter, float l2_coeff, float l1_coeff,
                        float tol, int64_t top_k, int32_t device, irs_slim_result **out) {
  return guard([&] {
    check_arg(out != nullptr, "out must not be null.");
    *out = nullptr;
    // util.hpp:233-236 (the reference's wording)
    check_arg(n_iter > 0, "n_iter must be > 0.");
    check_arg(l2_coeff >= 0, "l2_coeff must be > 0.");
    check_arg(l1_coeff >= 0, "l1_coeff must be > 0.");
    validate_csr(rows, cols, indptr, indices, data);
    auto res = std::make_unique<irs_slim_result>();
    slim::fit(rows, cols, indptr, indices, data, positive_only != 0, n_iter, l2_coeff, l1_coeff, tol, top_k, device,
              *res);
    *out = res.release();
  });
}

irs_status irs_slim_nnz(irs_slim_result *r, int64_t *nnz) {
  return guard([&] {
    check_arg(r && nnz, "null argument.");
    *nnz = static_cast<int64_t>(r->indices.size());
  });
}

irs_status irs_slim_fetch(irs_slim_result *r, int64_t *col_ptr, int32_t *indices, float *data) {
  return guard([&] {
    check_arg(r && col_ptr, "null argument.");
    std::copy(r->col_ptr.begin(), r->col_ptr.end(), col_ptr);
    if (!r->indices.empty()) {
      check_arg(indices && data, "null argument.");
      std::copy(r->indices.begin(), r->indices.end(), indices);
      std::copy(r->data.begin(), r->data.end(), data);
    }
  });
}

irs_status irs_slim_last_stats(irs_slim_result *r, double *gram_ms, double *descent_ms, double *emit_ms,
                               int64_t *sweeps_total, int64_t *updates_total) {
  return guard([&] {
    check_arg(r != nullptr, "null argument.");
    if (gram_ms) *gram_ms = r->gram_ms;
    if (descent_ms) *descent_ms = r->descent_ms;
    if (emit_ms) *emit_ms = r->emit_ms;
    if (sweeps_total) *sweeps_total = r->sweeps_total;
    if (updates_total) *updates_total = r->updates_total;
  });
}

irs_status irs_slim_last_launch(irs_slim_result *r, int32_t *lds_r, int32_t *lds_bytes, int32_t *threads,
                                int32_t *n_wg, int32_t *raise_dynamic_lds, int64_t *lds_per_block) {
  return guard([&] {
    check_arg(r != nullptr, "null argument.");
    if (lds_r) *lds_r = r->plan.lds_r ? 1 : 0;
    if (lds_bytes) *lds_bytes = r->plan.lds_bytes;
    if (threads) *threads = r->plan.threads;
    if (n_wg) *n_wg = r->plan.n_wg;
    if (raise_dynamic_lds) *raise_dynamic_lds = r->plan.raise_dynamic_lds ? 1 : 0;
    if (lds_per_block) *lds_per_block = r->lds_per_block;
  });
}

irs_status irs_slim_destroy(irs_slim_result *r) {
  return guard([&] { delete r; });
}

}  // extern "C"
