// The row-wise hold-out split on the device (the reference's SplitFunction, cpp_source/util.hpp:72-156, bound as
// rowwise_train_test_split_by_ratio / _by_fixed_n).  Host side of the C ABI; the rule, the row classes and the
// argument checks are in split_host_plan.hpp, the kernels in split_kernels.hpp.
#include <cstring>

#include "common.hpp"
#include "csr_checks.hpp"
#include "phase_spans.hpp"
#include "split_kernels.hpp"

struct irs_split_result {
  int64_t rows = 0, nnz_train = 0, nnz_test = 0;
  int32_t elem_bytes = 0;
  irs::RawVector<int64_t> train_ptr, test_ptr;
  irs::RawVector<int32_t> indices;  // the train matrix's entries, the test matrix's behind them
  irs::RawVector<char> data;        // likewise, elem_bytes each
  irs_split_stats stats = {};
};

namespace irs {
namespace split {

template <class E>
static void launch_scatter(const Plan &plan, int64_t rows, const int64_t *d_indptr, const int32_t *d_indices,
                           const char *d_data, const int32_t *d_long, uint64_t seed, const Mode &md,
                           const uint64_t *d_thr, const int64_t *d_test_ptr, int32_t *d_oidx, char *d_odata,
                           hipStream_t s) {
  const E *in = reinterpret_cast<const E *>(d_data);
  E *out = reinterpret_cast<E *>(d_odata);
  if (plan.n_class[CLASS_WAVE] > 0)
    hipLaunchKernelGGL(split_scatter_wave_kernel<E>, dim3(static_cast<unsigned>(ceil_div(rows, kWavesPerBlock))),
                       dim3(kSelectThreads), 0, s, d_indptr, d_indices, in, rows, seed, md, d_thr, d_test_ptr, d_oidx,
                       out);
  if (!plan.long_rows.empty())
    hipLaunchKernelGGL(split_scatter_block_kernel<E>, dim3(static_cast<unsigned>(plan.long_rows.size())),
                       dim3(kSelectThreads), 0, s, d_indptr, d_indices, in, rows, d_long, seed, md, d_thr, d_test_ptr,
                       d_oidx, out);
}

static void run(int64_t rows, const int64_t *indptr, const int32_t *indices, const void *data, int32_t w,
                uint64_t seed, const Mode &md, int device, irs_split_result &res) {
  const int64_t nnz = indptr[rows];
  const Plan plan = make_plan(rows, indptr, md);
  res.rows = rows;
  res.elem_bytes = w;
  res.stats.rows_empty = plan.n_class[CLASS_EMPTY];
  res.stats.rows_wave = plan.n_class[CLASS_WAVE];
  res.stats.rows_lds = plan.n_class[CLASS_LDS];
  res.stats.rows_stream = plan.n_class[CLASS_STREAM];
  res.train_ptr.resize(static_cast<size_t>(rows) + 1);
  res.test_ptr.resize(static_cast<size_t>(rows) + 1);
  if (nnz == 0) {  // nothing to move: both row pointers are zero, no device is asked for
    std::fill(res.train_ptr.begin(), res.train_ptr.end(), int64_t(0));
    std::fill(res.test_ptr.begin(), res.test_ptr.end(), int64_t(0));
    return;
  }
  require_device(device);
  hipStream_t s = nullptr;
  const size_t R = static_cast<size_t>(rows), N = static_cast<size_t>(nnz), W = static_cast<size_t>(w);

  Event e0, e1, e2, e3, e4, e5;
  IRS_HIP(hipEventRecord(e0.e, s));
  DeviceBuffer<int64_t> d_indptr, d_train_ptr, d_test_ptr, d_tiles;
  DeviceBuffer<int32_t> d_indices, d_oidx, d_long, d_sel_lds, d_sel_stream;
  DeviceBuffer<char> d_data, d_odata;
  DeviceBuffer<uint64_t> d_thr;
  d_indptr.upload(indptr, R + 1, s);
  d_indices.upload(indices, N, s);
  d_data.upload(static_cast<const char *>(data), N * W, s);
  d_long.upload(plan.long_rows, s);
  d_sel_lds.upload(plan.select_lds_rows, s);
  d_sel_stream.upload(plan.select_stream_rows, s);
  IRS_HIP(hipEventRecord(e1.e, s));

  // select: thr[row] for every row with 0 < n_test < m (the others never read it)
  d_thr.alloc(R);
  d_thr.zero(s);
  if (plan.wave_select_rows > 0)
    hipLaunchKernelGGL(split_select_wave_kernel, dim3(static_cast<unsigned>(ceil_div(rows, kWavesPerBlock))),
                       dim3(kSelectThreads), 0, s, static_cast<const int64_t *>(d_indptr.ptr), rows, seed, md,
                       d_thr.ptr);
  if (!plan.select_lds_rows.empty())
    hipLaunchKernelGGL(split_select_block_kernel<true>, dim3(static_cast<unsigned>(plan.select_lds_rows.size())),
                       dim3(kSelectThreads), 0, s, static_cast<const int64_t *>(d_indptr.ptr),
                       static_cast<const int32_t *>(d_sel_lds.ptr), seed, md, d_thr.ptr);
  if (!plan.select_stream_rows.empty())
    hipLaunchKernelGGL(split_select_block_kernel<false>, dim3(static_cast<unsigned>(plan.select_stream_rows.size())),
                       dim3(kSelectThreads), 0, s, static_cast<const int64_t *>(d_indptr.ptr),
                       static_cast<const int32_t *>(d_sel_stream.ptr), seed, md, d_thr.ptr);
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipEventRecord(e2.e, s));

  // scan: the row pointers of both outputs
  const int64_t n_tiles = scan_tiles(rows);
  d_tiles.alloc(static_cast<size_t>(n_tiles));
  d_train_ptr.alloc(R + 1);
  d_test_ptr.alloc(R + 1);
  hipLaunchKernelGGL(split_tile_sums_kernel, dim3(static_cast<unsigned>(n_tiles)), dim3(kScanThreads), 0, s,
                     static_cast<const int64_t *>(d_indptr.ptr), rows, md, d_tiles.ptr);
  hipLaunchKernelGGL(split_scan_tiles_kernel, dim3(1), dim3(kScanThreads), 0, s, d_tiles.ptr, n_tiles);
  hipLaunchKernelGGL(split_row_ptr_kernel, dim3(static_cast<unsigned>(n_tiles)), dim3(kScanThreads), 0, s,
                     static_cast<const int64_t *>(d_indptr.ptr), rows, md, static_cast<const int64_t *>(d_tiles.ptr),
                     d_train_ptr.ptr, d_test_ptr.ptr);
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipEventRecord(e3.e, s));

  // scatter
  d_oidx.alloc(N);
  d_odata.alloc(N * W);
  auto scatter = [&](auto elem) {
    launch_scatter<decltype(elem)>(plan, rows, d_indptr.ptr, d_indices.ptr, d_data.ptr, d_long.ptr, seed, md, d_thr.ptr,
                                   d_test_ptr.ptr, d_oidx.ptr, d_odata.ptr, s);
  };
  if (w == 1) scatter(uint8_t{});
  else if (w == 2) scatter(uint16_t{});
  else if (w == 4) scatter(uint32_t{});
  else scatter(uint64_t{});
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipEventRecord(e4.e, s));

  // copy back
  res.indices.resize(N);
  res.data.resize(N * W);
  IRS_HIP(hipMemcpyAsync(res.train_ptr.data(), d_train_ptr.ptr, (R + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  IRS_HIP(hipMemcpyAsync(res.test_ptr.data(), d_test_ptr.ptr, (R + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  IRS_HIP(hipMemcpyAsync(res.indices.data(), d_oidx.ptr, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  IRS_HIP(hipMemcpyAsync(res.data.data(), d_odata.ptr, N * W, hipMemcpyDeviceToHost, s));
  IRS_HIP(hipEventRecord(e5.e, s));
  IRS_HIP(hipStreamSynchronize(s));
  res.nnz_test = res.test_ptr[R];
  res.nnz_train = res.train_ptr[R];
  if (res.nnz_test < 0 || res.nnz_train < 0 || res.nnz_train + res.nnz_test != nnz)
    throw std::runtime_error("split: inconsistent result size.");
  res.stats.upload_ms = elapsed_ms(e0, e1);
  res.stats.select_ms = elapsed_ms(e1, e2);
  res.stats.scan_ms = elapsed_ms(e2, e3);
  res.stats.scatter_ms = elapsed_ms(e3, e4);
  res.stats.d2h_ms = elapsed_ms(e4, e5);
}

}  // namespace split
}  // namespace irs

using namespace irs;

extern "C" {

irs_status irs_split_rowwise(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices,
                             const void *data, int32_t elem_bytes, int64_t random_seed, int32_t mode,
                             double heldout_ratio, int32_t n_test_ceil, int64_t n_held_out, int32_t device,
                             irs_split_result **out) {
  return guard([&] {
    check_arg(out != nullptr, "out must not be null.");
    *out = nullptr;
    const split::Mode md{mode, heldout_ratio, n_test_ceil != 0 ? 1 : 0, n_held_out};
    split::check_mode(md);
    split::check_width(elem_bytes);
    // (the matrix checks read indptr and indices only; data is looked at for being there)
    validate_csr(rows, cols, indptr, indices, static_cast<const float *>(data));
    auto res = std::make_unique<irs_split_result>();
    split::run(rows, indptr, indices, data, elem_bytes, static_cast<uint64_t>(random_seed), md, device, *res);
    *out = res.release();
  });
}

irs_status irs_split_nnz(irs_split_result *r, int64_t *nnz_train, int64_t *nnz_test) {
  return guard([&] {
    check_arg(r && nnz_train && nnz_test, "null argument.");
    *nnz_train = r->nnz_train;
    *nnz_test = r->nnz_test;
  });
}

irs_status irs_split_fetch(irs_split_result *r, int64_t *train_indptr, int32_t *train_indices, void *train_data,
                           int64_t *test_indptr, int32_t *test_indices, void *test_data) {
  return guard([&] {
    check_arg(r && train_indptr && test_indptr, "null argument.");
    std::copy(r->train_ptr.begin(), r->train_ptr.end(), train_indptr);
    std::copy(r->test_ptr.begin(), r->test_ptr.end(), test_indptr);
    const size_t w = static_cast<size_t>(r->elem_bytes);
    const size_t n_train = static_cast<size_t>(r->nnz_train), n_test = static_cast<size_t>(r->nnz_test);
    if (n_train) {
      check_arg(train_indices && train_data, "null argument.");
      std::memcpy(train_indices, r->indices.data(), n_train * sizeof(int32_t));
      std::memcpy(train_data, r->data.data(), n_train * w);
    }
    if (n_test) {
      check_arg(test_indices && test_data, "null argument.");
      std::memcpy(test_indices, r->indices.data() + n_train, n_test * sizeof(int32_t));
      std::memcpy(test_data, r->data.data() + n_train * w, n_test * w);
    }
  });
}

irs_status irs_split_last_stats(irs_split_result *r, irs_split_stats *stats) {
  return guard([&] {
    check_arg(r && stats, "null argument.");
    *stats = r->stats;
  });
}

irs_status irs_split_destroy(irs_split_result *r) {
  return guard([&] { delete r; });
}

}  // extern "C"
