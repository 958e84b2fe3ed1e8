// Item-kNN similarity on gfx950: the computer, its buffers and the C ABI of include/irspack_amd.h.  The kernels are in
// knn_kernels.hpp, the host logic that needs no device (scans, chunks, target pass, variant, arena) in knn_host_prep.hpp.
#include <algorithm>
#include <array>
#include <atomic>
#include <thread>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>

#include "common.hpp"
#include "knn_host_prep.hpp"
#include "knn_kernels.hpp"

namespace irs {
namespace knn {

// (the HIP-free host logic and its test take the kernels' constants from knn_host_prep.hpp)
static_assert(TILE == KNN_TILE && FAST_CAP == KNN_FAST_CAP && TOPK_CAP == KNN_TOPK_CAP, "knn_host_prep.hpp's constants");
static void check_lower(double x, double low, const char *name) {  // argcheck.hpp:13-20
  if (x < low) {
    std::string msg = std::string(name) + " must be greater than or equal to  " + std::to_string(low);
    throw std::invalid_argument(msg);
  }
}

}  // namespace knn
}  // namespace irs

using namespace irs;
using namespace irs::knn;

struct irs_knn_computer {
  int device = 0;
  int32_t sim_type = 0;
  int64_t N = 0, n_features = 0;
  double shrinkage = 0, alpha = 0, beta = 0;
  bool normalize = false;
  std::vector<int64_t> xt_row_len;  // host: stored entries per feature row (work model)
  DeviceBuffer<uint32_t> xt_tptr;  // [n_features, n_tiles + 1], see Params
  DeviceBuffer<uint32_t> xt_idx16;
  DeviceBuffer<double> xt_val, norms;
  DeviceBuffer<double> xt_rowval;  // see Params (allocated only when every feature row is constant)
  bool xt_row_const = false;
  bool xt_all_ones = false;
  DeviceBuffer<double> col_scale;  // see Params (allocated only for a separable fused weighting)
  bool col_scaled = false;
  double norm_max = 0.0;  // largest column norm (the approximate selection needs counts below 2^24 for Tversky)
  bool xt_nonzero = false;  // |x| in (1e-150, 1e150) for every stored x
  bool xt_positive = false; // every stored x > 0
  std::vector<double> xt_rowmax;  // host: max |x| per feature row (bound of a target row's sums)
  std::vector<double> xt_rowmin;  // host: min |x| per feature row (smallest product of a target row)
  // last result (host)
  std::vector<int64_t> res_ptr;
  DeviceBuffer<int32_t> res_idx;  // the last result stays on the device until irs_knn_fetch
  DeviceBuffer<double> res_val;
  int64_t res_nnz = 0;
  double last_ms = 0;
  int64_t last_macs = 0, last_walked = 0;
  // scratch of a compute call, kept between calls (hipMalloc / hipFree of ~200 MB per call
  // cost more than a millisecond, and hipFree synchronises the device)
  struct Scratch {
    DeviceBuffer<int64_t> t_ptr, res_ptr;
    DeviceBuffer<int32_t> t_idx, order, cand_idx, cand_cnt, out_idx, out_cnt, cursor, slot_of, redo_list;
    DeviceBuffer<double> t_val, t_stat, t_scale, cand_val, out_val;
    DeviceBuffer<uint64_t> hi_stash;
    // ONE allocation behind the buffers every call needs (carved per call; t_val / hi_stash, which
    // only some calls need, are allocations of their own): seventeen hipMalloc calls were 11 ms of the
    // first call of a computer - and `learn()` of a kNN recommender makes exactly one call
    DeviceBuffer<char> arena;
  } scratch;
  // a compute call: set-up, the counts of the finished chunks and the end of the call; the kernels of its
  // row chunks, one chunk after the other; the chunks' small inputs; the column indices (uploader
  // thread); compaction + device-to-host copy of the chunks that are done.
  // (Measured and dropped, round 5: the chunks' tile kernels on two or three streams in turn with the
  // merges on a stream of their own, so that a chunk's last heavy pairs overlap the next chunk.  The
  // ML-20M call went from 9.5 ms (four chunks, one stream) to 11.8 ms of device time: the 130 KB
  // workgroups of two persistent kernels and the small merge blocks take each other's compute units.)
  hipStream_t stream = nullptr, stream_k = nullptr, stream_in = nullptr, stream_up = nullptr, stream_out = nullptr;
  hipEvent_t ev_in = nullptr, ev_setup = nullptr;
  // the last result once more in page-locked host memory (kept between calls): the device-to-host copy
  // runs at the link's rate at the end of the compute call, irs_knn_fetch is then a multi-threaded
  // host copy into the caller's (pageable, usually untouched) arrays
  char *stage = nullptr;
  size_t stage_bytes = 0, stage_idx_offset = 0;  // values at 0, column indices at stage_idx_offset
  bool staged = false;
  int64_t n_calls = 0;  // compute calls so far
  std::array<hipStream_t *, 5> all_streams() { return {&stream, &stream_k, &stream_in, &stream_up, &stream_out}; }
  ~irs_knn_computer() {
    if (stage) (void)hipHostFree(stage);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_setup) (void)hipEventDestroy(ev_setup);
    for (hipStream_t st : {stream, stream_k, stream_in, stream_up, stream_out})
      if (st) (void)hipStreamDestroy(st);
  }
};

// The arena and the page-locked staging buffer of the last computer that was destroyed, per device: a
// tuning loop constructs, uses once and drops one computer after the other, and mapping ~250 MB of
// device memory (14 ms) + page-locking 32 MB (6 ms) cost more than the ML-20M call itself (11 ms).
namespace {
struct KnnBufferCache {
  std::mutex mu;
  struct Slot {
    int device = -1;
    char *arena = nullptr;
    size_t arena_bytes = 0;
    char *stage = nullptr;
    size_t stage_bytes = 0;
    // (five stream creations are another 5 - 10 ms of a computer's first call)
    hipStream_t streams[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_in = nullptr, ev_setup = nullptr;
  } slot;
  ~KnnBufferCache() {}  // (process exit: the runtime may be gone already - nothing to free safely)
  static void move(char *&to, size_t &to_bytes, char *&from, size_t &from_bytes) {
    to = from;
    to_bytes = from_bytes;
    from = nullptr;
    from_bytes = 0;
  }
  // A computer that is being destroyed (its streams are idle) leaves to the next one on its device: the arena when it
  // is larger than the slot's or the slot belongs to another device, streams and events when the slot has none, the larger stage.
  void keep(irs_knn_computer *c) {
    std::lock_guard<std::mutex> lock(mu);
    irs_knn_computer::Scratch &sc = c->scratch;
    if (sc.arena.ptr && sc.arena.owned && (slot.device != c->device || sc.arena.count > slot.arena_bytes)) {
      if (slot.arena) (void)hipFree(slot.arena);
      move(slot.arena, slot.arena_bytes, sc.arena.ptr, sc.arena.count);  // (the views into it die with the computer)
      if (slot.device != c->device) {  // (what the slot holds belongs to another device)
        if (slot.stage) (void)hipHostFree(slot.stage);
        slot.stage = nullptr;
        slot.stage_bytes = 0;
        for (auto &st : slot.streams) {
          if (st) (void)hipStreamDestroy(st);
          st = nullptr;
        }
        if (slot.ev_in) (void)hipEventDestroy(slot.ev_in);
        if (slot.ev_setup) (void)hipEventDestroy(slot.ev_setup);
        slot.ev_in = slot.ev_setup = nullptr;
      }
      slot.device = c->device;
    }
    if (c->stream && slot.device == c->device && !slot.streams[0]) swap_streams(c);
    if (c->stage && slot.device == c->device && c->stage_bytes > slot.stage_bytes) {
      if (slot.stage) (void)hipHostFree(slot.stage);
      move(slot.stage, slot.stage_bytes, c->stage, c->stage_bytes);
    }
  }
  // a dropped computer's streams and events, for a computer of the same device that has none yet
  void hand_streams(irs_knn_computer *c) {
    std::lock_guard<std::mutex> lock(mu);
    if (slot.device == c->device && slot.streams[0]) swap_streams(c);
  }
  void swap_streams(irs_knn_computer *c) {  // (one side holds streams and events, the other nulls)
    const auto mine = c->all_streams();
    for (int k = 0; k < 5; k++) std::swap(*mine[k], slot.streams[k]);
    std::swap(c->ev_in, slot.ev_in);
    std::swap(c->ev_setup, slot.ev_setup);
  }
  // a dropped computer's arena when it holds `need` bytes (the computer's own does not), and its stage when larger
  void hand_buffers(irs_knn_computer *c, size_t need) {
    std::lock_guard<std::mutex> lock(mu);
    irs_knn_computer::Scratch &sc = c->scratch;
    if (slot.device == c->device && slot.arena && slot.arena_bytes >= need) {
      sc.arena.release();
      move(sc.arena.ptr, sc.arena.count, slot.arena, slot.arena_bytes);  // (released: `owned` again)
    }
    if (slot.device == c->device && slot.stage && slot.stage_bytes > c->stage_bytes) {
      if (c->stage) (void)hipHostFree(c->stage);
      move(c->stage, c->stage_bytes, slot.stage, slot.stage_bytes);
    }
  }
} knn_buffer_cache;
// host threads of the target pass (IRSPACK_AMD_KNN_THREADS overrides)
int64_t host_thread_cap() {
  const char *e = std::getenv("IRSPACK_AMD_KNN_THREADS");  // (read per call: tests toggle it)
  return e ? std::max<int64_t>(1, std::atoll(e)) : int64_t(32);
}
// IRSPACK_AMD_KNN_TIMING=1 prints the host phases of a compute call to stderr
struct PhaseTimer {
  bool on = std::getenv("IRSPACK_AMD_KNN_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void mark(const char *what) {
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "knn host phase %-18s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};
// The CSR arrays of a matrix on their way to the device from pageable memory (the copies occupy a host thread) while the
// caller validates and classifies them: row pointers and column indices at once, the values only if they are not all ones.
struct CsrUploader {
  DeviceBuffer<int32_t> indptr, indices;
  DeviceBuffer<double> values, extra;  // extra: `extra_count` doubles allocated on the way (irs_knn_weight's result)
  CsrUploader(int device, int64_t rows, int64_t nnz, const int64_t *h_indptr, const int32_t *h_indices, size_t extra_count) {
    thread = std::thread([this, device, rows, nnz, h_indptr, h_indices, extra_count] {
      try {
        IRS_HIP(hipSetDevice(device));
        std::vector<int32_t> ip32(rows + 1);
        for (int64_t i = 0; i <= rows; i++) ip32[i] = static_cast<int32_t>(h_indptr[i]);
        indptr.alloc(static_cast<size_t>(rows) + 1);
        indices.alloc(static_cast<size_t>(nnz));
        if (extra_count) extra.alloc(extra_count);
        IRS_HIP(hipMemcpy(indptr.ptr, ip32.data(), ip32.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        IRS_HIP(hipMemcpy(indices.ptr, h_indices, static_cast<size_t>(nnz) * sizeof(int32_t), hipMemcpyHostToDevice));
        int k = 0;
        while ((k = kind.load(std::memory_order_acquire)) == 0) std::this_thread::yield();
        if (k == 2) {
          values.alloc(static_cast<size_t>(nnz));
          IRS_HIP(hipMemcpy(values.ptr, h_values, static_cast<size_t>(nnz) * sizeof(double), hipMemcpyHostToDevice));
        }
      } catch (const std::exception &e) {
        error = e.what();
      }
    });
  }
  // the caller has looked at every value: all ones (nothing more travels), or `vals` follow
  void classified(bool ones, const double *vals) {
    h_values = vals;
    kind.store(ones ? 1 : 2, std::memory_order_release);
  }
  void finish() {
    thread.join();
    if (!error.empty()) throw std::runtime_error(error);
  }
  ~CsrUploader() {
    int zero = 0;
    kind.compare_exchange_strong(zero, 3);  // (an exception before the classification: the uploader must not wait)
    if (thread.joinable()) thread.join();
  }

 private:
  std::string error;
  std::atomic<int> kind{0};  // 0: not classified yet, 1: all ones, 2: the values travel too, 3: give up
  const double *h_values = nullptr;
  std::thread thread;
};
// the per-entry pass of a feature weighting (util.hpp:183-184, :206) over a device-resident CSR; in_vals null:
// every stored value is 1; flags (may be null): what the weighted values are like, see knn_weight_kernel
void launch_weight(bool bm25, const DeviceBuffer<int32_t> &indptr, const DeviceBuffer<int32_t> &indices,
                   const double *in_vals, const DeviceBuffer<double> &idf, const DeviceBuffer<double> &reg, double k1,
                   int64_t rows, double *out, int32_t *flags, hipStream_t s) {
  auto go = [&](auto kernel, const double *reg_p, double k) {
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(ceil_div(rows, 4))), dim3(256), 0, s,
                       static_cast<const int32_t *>(indptr.ptr), static_cast<const int32_t *>(indices.ptr), in_vals,
                       static_cast<const double *>(idf.ptr), reg_p, k, rows, out, flags);
  };
  if (bm25) go(knn_weight_kernel<true>, reg.ptr, k1 + 1); else go(knn_weight_kernel<false>, nullptr, 0.0);
  IRS_HIP(hipGetLastError());
}
// nnz device-resident values - and indices, if dst_idx is not null - into the caller's (pageable, usually
// untouched) arrays: a few device-to-host copies side by side, one per `per_copy` entries and four at the
// most (one pageable copy is staged through a single pinned bounce buffer by the runtime).  False: a copy failed.
bool copy_to_host_threaded(int device, int64_t nnz, int64_t per_copy, double *dst_val, const double *src_val,
                           int32_t *dst_idx, const int32_t *src_idx) {
  const int n_copy = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(4, nnz / per_copy)));
  std::atomic<int> failed(0);
  run_on_threads(n_copy, [&](int k) {
    const int64_t q0 = nnz * k / n_copy, q1 = nnz * (k + 1) / n_copy;
    if (q1 <= q0) return;
    const size_t cnt = static_cast<size_t>(q1 - q0);
    if (hipSetDevice(device) != hipSuccess ||
        hipMemcpy(dst_val + q0, src_val + q0, cnt * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        (dst_idx && hipMemcpy(dst_idx + q0, src_idx + q0, cnt * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess))
      failed.store(1);
  });
  return failed.load() == 0;
}
// a result in page-locked memory -> the caller's arrays, on several host threads
void copy_from_stage(const char *stage_val, const char *stage_idx, int64_t nnz, double *data, int32_t *indices) {
  const double *sv = reinterpret_cast<const double *>(stage_val);
  const int32_t *si = reinterpret_cast<const int32_t *>(stage_idx);
  parallel_ranges(nnz, [&](int64_t lo, int64_t hi) {
    std::memcpy(data + lo, sv + lo, static_cast<size_t>(hi - lo) * sizeof(double));
    std::memcpy(indices + lo, si + lo, static_cast<size_t>(hi - lo) * sizeof(int32_t));
  }, 8, 200000);
}

// ---------------------------------------------------------------- construction
// the arguments of irs_knn_create once they are checked, and what the checks derive from them
struct CreateInput {
  int32_t sim_type;
  int64_t rows, cols;  // of X_arg
  const int64_t *indptr;
  const int32_t *indices;
  const double *data;
  const irs_knn_input *spec;
  double shrinkage, alpha, beta;
  int32_t normalize, device;
  int32_t layout, weighting;
  int64_t m_rows, m_cols, nnz;  // M: the matrix as the arrays store it - X_arg itself, or X_arg^T for the CSC layout
  bool device_candidate;
  HostCsrD conv;  // host_regroup()'s private arrays
  RawVector<double> conv_w;
  // (every stored value becomes 1: similarities.hpp:96-107, 143-159)
  bool binarises() const { return sim_type == IRS_SIM_JACCARD || sim_type == IRS_SIM_TVERSKY; }
  // (P3alpha / RP3beta: the rows are pow-ed and normalised on the host first)
  bool transforms() const { return sim_type == IRS_SIM_P3ALPHA || sim_type == IRS_SIM_RP3BETA; }
};
// the checks of irs_knn_create, in the order the reference makes them
CreateInput check_create_args(int32_t sim_type, int64_t rows, int64_t cols, const int64_t *indptr,
                              const int32_t *indices, const double *data, const irs_knn_input *input,
                              double shrinkage, double alpha, double beta, int32_t normalize, int64_t n_threads,
                              int64_t max_chunk_size, int32_t device, irs_knn_computer **out) {
  check_arg(out != nullptr, "null argument.");
  // KNNComputer ctor, knn.hpp:35-38
  check_lower(shrinkage, 0, "shrinkage");
  check_arg(n_threads >= 1, "n_threads must be greater than or equal to  1");
  check_arg(max_chunk_size >= 1, "max_chunk_size must be greater than or equal to  1");
  // (the parameter checks of the similarities' constructors first: similarities.hpp:61-72, 143-159, 198-222, 265-292)
  if (sim_type < IRS_SIM_COSINE || sim_type > IRS_SIM_RP3BETA) throw std::invalid_argument("unknown similarity type.");
  if (sim_type != IRS_SIM_COSINE && sim_type != IRS_SIM_JACCARD) check_lower(alpha, 0, "alpha");
  if (sim_type == IRS_SIM_ASYMMETRIC && alpha > 1)
    throw std::invalid_argument("alpha must be less than or equal to  " + std::to_string(1.0));
  if (sim_type == IRS_SIM_TVERSKY || sim_type == IRS_SIM_RP3BETA) check_lower(beta, 0, "beta");
  CreateInput in{sim_type, rows, cols, indptr, indices, data, input, shrinkage, alpha, beta, normalize, device};
  in.layout = input ? input->layout : IRS_LAYOUT_CSR;
  in.weighting = input ? input->weighting : IRS_WEIGHT_NONE;
  check_arg(in.layout == IRS_LAYOUT_CSR || in.layout == IRS_LAYOUT_CSC, "unknown matrix layout.");
  check_arg(in.weighting == IRS_WEIGHT_NONE || in.weighting == IRS_WEIGHT_TF_IDF || in.weighting == IRS_WEIGHT_BM25,
            "unknown feature weighting.");
  check_arg(rows >= 0 && cols >= 0 && indptr, "bad matrix.");
  check_arg(rows < (int64_t(1) << 31) && cols < (int64_t(1) << 31), "too many rows.");
  in.m_rows = in.layout == IRS_LAYOUT_CSC ? cols : rows;
  in.m_cols = in.layout == IRS_LAYOUT_CSC ? rows : cols;
  check_arg(indptr[0] == 0 && indptr[in.m_rows] >= 0, "malformed indptr.");
  for (int64_t i = 0; i < in.m_rows; i++) check_arg(indptr[i + 1] >= indptr[i], "malformed indptr.");
  in.nnz = indptr[in.m_rows];
  check_arg(in.nnz == 0 || (indices && data), "bad matrix.");
  // IRSPACK_AMD_KNN_DEVICE_CREATE=0: host path for everything (A/B)
  in.device_candidate = in.nnz > 0 && cols > 0 && in.nnz < (int64_t(1) << 31) - 1024 &&
                        env_flag("IRSPACK_AMD_KNN_DEVICE_CREATE", true);
  check_arg(!(in.transforms() && in.weighting != IRS_WEIGHT_NONE), "P3alpha / RP3beta take no feature weighting.");
  if (in.binarises()) in.weighting = IRS_WEIGHT_NONE;
  return in;
}
// The paths that read X_arg's rows on the host (P3alpha / RP3beta's row normalisation; the host
// construction; empty matrices) get them: weighting and regrouping on host threads, into the private arrays
// of `in`, which then describes an unweighted CSR matrix.
void host_regroup(CreateInput &in, PhaseTimer &pt) {
  if (!((!in.device_candidate || in.transforms()) && (in.layout == IRS_LAYOUT_CSC || in.weighting != IRS_WEIGHT_NONE)))
    return;
  std::atomic<int> bad_idx(0);
  parallel_ranges(in.nnz, [&](int64_t b, int64_t e) {
    if (scan_entries(in.indices, nullptr, b, e, in.m_cols, false) & BAD_INDEX) bad_idx.store(1);
  });
  check_arg(bad_idx.load() == 0, "column index out of range.");
  if (in.weighting != IRS_WEIGHT_NONE) {
    const bool bm = in.weighting == IRS_WEIGHT_BM25;
    const WeightTables wt = weight_tables(bm, in.m_rows, in.m_cols, in.indptr, in.indices, in.data, false, in.spec->k1,
                                          in.spec->b, in.spec->smooth != 0);
    in.conv_w.resize(static_cast<size_t>(in.nnz));
    weight_values_host(bm, wt, in.m_rows, in.indptr, in.indices, in.data, in.spec->k1, in.conv_w.data());
    in.data = in.conv_w.data();
    in.weighting = IRS_WEIGHT_NONE;
  }
  if (in.layout == IRS_LAYOUT_CSC) {
    in.conv = transpose_pattern(in.m_rows, in.m_cols, in.indptr, in.indices, in.data);
    in.indptr = in.conv.indptr.data();
    in.indices = in.conv.indices.data();
    in.data = in.conv.data.data();
    in.layout = IRS_LAYOUT_CSR;
    in.m_rows = in.rows;
    in.m_cols = in.cols;
  }
  pt.mark("create: host regroup");
}

std::unique_ptr<irs_knn_computer> new_computer(const CreateInput &in) {
  auto c = std::make_unique<irs_knn_computer>();
  c->device = in.device;
  c->sim_type = in.sim_type;
  c->N = in.rows;
  c->n_features = in.cols;
  c->shrinkage = in.shrinkage;
  c->alpha = in.alpha;
  c->beta = in.beta;
  c->normalize = in.normalize != 0;
  return c;
}
// Cosine / asymmetric cosine / Jaccard / Tversky, round 5: the caller's arrays are validated and
// classified in place (no private copy), the column indices - and the values, if they are not all
// ones - travel to the device beside that pass, and X_arg^T, its slice pointers, its packed offsets
// and its per-row value ranges are built THERE (stable radix sort of the entry numbers by column +
// one gather, three small kernels): 68 -> 5 ms for binary interactions on the ML-20M shape, where the
// host spent 17 ms on the copy, 29 ms on the transpose and 15 ms on slices + packing.  Same
// similarities bit for bit (test_device_create_is_the_host_create).  P3alpha / RP3beta: the rows are
// pow-ed and normalised on the host first (libm's pow), into the one private array of this path.
struct DeviceCreate {
  const CreateInput &in;
  PhaseTimer &pt;
  const bool csc, bm25;  // csc: the arrays ARE X_arg^T
  RawVector<double> tvals;  // P3alpha / RP3beta: the rows pow-ed and normalised (pow_normalise_row), this path's one private array
  const double *vals;
  const std::vector<int64_t> ipv;
  CsrUploader up;  // (after every host array it reads: it is joined before they go)
  std::atomic<unsigned> flags{0};  // BAD_INDEX .. NOT_POSITIVE of the values the kernels multiply
  bool input_ones = false, norms_on_device = false;
  bool weighted = false;     // does the value stream of the kernels carry anything but ones?
  bool separable = false;    // see separable_factors()
  bool stream_vals = false;  // do the kernels read a float64 value per entry?
  WeightTables wt;
  std::unique_ptr<irs_knn_computer> c;
  std::vector<double> norms, sep_rowval, sep_colscale;  // (sep_*: empty = that factor is 1)
  hipStream_t s = nullptr;
  size_t padded = 0;
  std::vector<int32_t> t_count;  // stored entries per row of X_arg^T
  DeviceBuffer<char> tmp;
  DeviceBuffer<double> d_ss;
  DeviceBuffer<int32_t> d_tidx;
  const int32_t *xt_idx_src = nullptr;  // column indices of X_arg^T's entries (device)
  DeviceCreate(const CreateInput &in_, PhaseTimer &pt_)
      : in(in_), pt(pt_), csc(in_.layout == IRS_LAYOUT_CSC), bm25(in_.weighting == IRS_WEIGHT_BM25), vals(in_.data),
        ipv(in_.indptr, in_.indptr + in_.m_rows + 1), up(in_.device, in_.m_rows, in_.nnz, in_.indptr, in_.indices, 0) {}
  irs_knn_computer *run() {
    classify();
    // The feature weighting (util.hpp:159-209), fused: the two small tables on host threads while the
    // uploads run, the per-entry pass on the device - the weighted matrix is never materialised on the host.
    if (in.weighting != IRS_WEIGHT_NONE) {
      wt = weight_tables(bm25, in.m_rows, in.m_cols, in.indptr, in.indices, in.data, input_ones, in.spec->k1, in.spec->b,
                         in.spec->smooth != 0);
      pt.mark("create: weight tables");
    }
    c = new_computer(in);
    host_norms();
    up.finish();
    pt.mark("create: norms + upload");
    weighted = !input_ones;
    if (in.weighting != IRS_WEIGHT_NONE) weight_on_device();
    separable_factors();
    stream_vals = weighted && !separable;
    padded = (static_cast<size_t>(in.nnz) + 256 + 1) & ~size_t(1);
    if (csc) streams_of_csc(); else streams_by_transpose();
    if (norms_on_device) device_norms();
    slices_and_pack();
    if (!tvals.empty()) {
      auto *junk = new RawVector<double>();
      junk->swap(tvals);
      std::thread([junk] { delete junk; }).detach();  // (returning 160 MB to the system takes 10+ ms: nothing waits)
    }
    return c.release();
  }
  void classify() {
    if (in.transforms()) {
      tvals.resize(static_cast<size_t>(in.nnz));
      for_rows_parallel(ipv, in.m_rows, [&](int64_t i) { pow_normalise_row(in.indptr, i, in.data, in.alpha, tvals.data()); });
      vals = tvals.data();
      pt.mark("create: transform");
    }
    const int n_thr = static_cast<int>(std::max<int64_t>(
        1, std::min<int64_t>({16, static_cast<int64_t>(std::thread::hardware_concurrency()), in.nnz / 500000 + 1})));
    const double *scan_vals = in.binarises() ? nullptr : vals;  // (binarising similarities: never looked at)
    run_on_threads(n_thr, [&](int k) {
      flags.fetch_or(scan_entries(in.indices, scan_vals, in.nnz * k / n_thr, in.nnz * (k + 1) / n_thr, in.m_cols, true));
    });
    check_arg(!(flags & BAD_INDEX), "column index out of range.");
    input_ones = !(flags & NOT_ONES);  // (binarising similarities: always)
    up.classified(input_ones, vals);
    pt.mark("create: validate");
  }
  // the norms (similarities.hpp:20-28, 61-72, 96-107, 143-159); rows of ones: sqrt / pow of the entry
  // count, which is what their sums of 1.0 * 1.0 are.  From the caller's arrays on host threads when
  // they hold X_arg's rows and nothing weights them; else from the device (device_norms()).
  void host_norms() {
    norms.assign(in.rows, 0.0);
    norms_on_device = !in.transforms() && (in.weighting != IRS_WEIGHT_NONE || (csc && !input_ones));
    if (in.transforms() || norms_on_device) return;  // (P3alpha / RP3beta have none)
    if (csc) {  // all ones: the entry count of every column of M
      const std::vector<int64_t> cnt = column_counts(in.m_rows, in.m_cols, in.indptr, in.indices);
      parallel_ranges(in.rows, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) norms[i] = finish_norm(in.sim_type, in.alpha, static_cast<double>(cnt[i]));
      }, 16, 20000);
    } else {
      for_rows_parallel(ipv, in.rows, [&](int64_t i) {
        double ss = static_cast<double>(in.indptr[i + 1] - in.indptr[i]);
        if (!input_ones) {
          ss = 0;
          for (int64_t q = in.indptr[i]; q < in.indptr[i + 1]; q++) ss += in.data[q] * in.data[q];
        }
        norms[i] = finish_norm(in.sim_type, in.alpha, ss);
      });
    }
  }
  // the weighted values take the place of the caller's on the device; the kernel reports what they are like
  void weight_on_device() {
    int32_t w_flags = 0;
    DeviceBuffer<double> d_idf, d_reg, d_w;
    DeviceBuffer<int32_t> d_flags;
    d_idf.upload(wt.idf, s);
    if (bm25) d_reg.upload(wt.reg, s);
    d_w.alloc(static_cast<size_t>(in.nnz));
    d_flags.alloc(1);
    IRS_HIP(hipMemsetAsync(d_flags.ptr, 0, sizeof(int32_t), s));
    launch_weight(bm25, up.indptr, up.indices, input_ones ? nullptr : up.values.ptr, d_idf, d_reg, in.spec->k1, in.m_rows,
                  d_w.ptr, d_flags.ptr, s);
    IRS_HIP(hipMemcpyAsync(&w_flags, d_flags.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    IRS_HIP(hipStreamSynchronize(s));
    std::swap(up.values.ptr, d_w.ptr);  // (the weighted values take the place of the caller's, which go with d_w)
    std::swap(up.values.count, d_w.count);
    weighted = (w_flags & 1) != 0;
    flags = ((w_flags & 2) ? NOT_SAFE : 0u) | ((w_flags & 4) ? NOT_POSITIVE : 0u);
    pt.mark("create: weight");
  }
  // SEPARABLE weightings.  On binary interactions both weightings factor over the stored matrix M
  // (rows r = documents, columns t = terms): tf-idf w[r][t] = idf[t] (util.hpp:206 with x = 1), BM25
  // w[r][t] = (idf[t] (k1 + 1)) / (1 + reg[r]) (:183-184).  The kernels then never read a value stream:
  // the factor that belongs to X_arg^T's ROWS (the features) becomes `xt_rowval` - the all-ones kernels
  // on y' = x_u y, round 5 - and the factor that belongs to its COLUMNS (the computer's items / users)
  // becomes `col_scale`, applied to the finished sum with one rounding.  Pure tf-idf of an item-kNN
  // (CSC layout: idf belongs to the columns) therefore runs the exact COUNT kernel.  The sums differ
  // from the sums of the individually rounded weights by rounding only (<= 2 ulp per term, far inside
  // the 1e-12 of the parity bar; columns whose weights and counts are equal tie EXACTLY and are ordered
  // by column - DESIGN 3.4, `test_separable_weighting`).  The norms still come from the individually
  // rounded weights (up.values), like the reference's.  IRSPACK_AMD_KNN_SEPARABLE=0: the general form (A/B).
  void separable_factors() {
    separable = in.weighting != IRS_WEIGHT_NONE && input_ones && env_flag("IRSPACK_AMD_KNN_SEPARABLE", true);
    if (!separable) return;
    const double k1p1 = bm25 ? in.spec->k1 + 1 : 1.0;
    std::vector<double> &term_f = csc ? sep_colscale : sep_rowval;  // per column of M
    std::vector<double> &doc_f = csc ? sep_rowval : sep_colscale;   // per row of M
    term_f.resize(static_cast<size_t>(in.m_cols));
    for (int64_t t = 0; t < in.m_cols; t++) term_f[t] = bm25 ? wt.idf[t] * k1p1 : wt.idf[t];
    if (bm25) {
      doc_f.resize(static_cast<size_t>(in.m_rows));
      for (int64_t r = 0; r < in.m_rows; r++) doc_f[r] = 1.0 / (1.0 + wt.reg[r]);
    }
  }
  // CSR layout: X_arg^T by a transpose on the device (the sums of squares of X_arg's rows as stored first:
  // the transpose reorders the values)
  void streams_by_transpose() {
    if (norms_on_device) {
      d_ss.alloc(static_cast<size_t>(std::max<int64_t>(in.rows, 1)));
      hipLaunchKernelGGL(knn_row_sumsq_kernel, dim3(static_cast<unsigned>(ceil_div(in.rows, 4))), dim3(256), 0, s,
                         reinterpret_cast<const uint32_t *>(up.indptr.ptr), static_cast<const double *>(up.values.ptr),
                         in.rows, d_ss.ptr);
    }
    d_tidx.alloc(static_cast<size_t>(in.nnz));
    if (stream_vals) {  // the transposed values straight into the padded value stream of the kernels
      c->xt_val.alloc(padded);
      IRS_HIP(hipMemsetAsync(c->xt_val.ptr + in.nnz, 0, (padded - static_cast<size_t>(in.nnz)) * sizeof(double), s));
      transpose_csr_device(up.indptr.ptr, up.indices.ptr, static_cast<const double *>(up.values.ptr), in.rows, in.cols, in.nnz,
                           d_tidx.ptr, c->xt_val.ptr, t_count, tmp, s);
    } else {
      c->xt_val.alloc(2);  // (the ONES kernels never read the value stream)
      transpose_csr_device(up.indptr.ptr, up.indices.ptr, static_cast<const double *>(nullptr), in.rows, in.cols, in.nnz,
                           d_tidx.ptr, static_cast<double *>(nullptr), t_count, tmp, s);
    }
    xt_idx_src = d_tidx.ptr;
    pt.mark("create: transpose");
  }
  // CSC layout: the arrays ARE X_arg^T - nothing to transpose for the kernels' streams; only the
  // norms of a weighted matrix need X_arg's rows together (their squares are added in row order)
  void streams_of_csc() {
    t_count.resize(static_cast<size_t>(in.cols));
    for (int64_t u = 0; u < in.cols; u++) t_count[u] = static_cast<int32_t>(in.indptr[u + 1] - in.indptr[u]);
    if (stream_vals) {
      c->xt_val.alloc(padded);
      hipLaunchKernelGGL(knn_pad_copy_kernel, dim3(static_cast<unsigned>(ceil_div(static_cast<int64_t>(padded), 256))),
                         dim3(256), 0, s, static_cast<const double *>(up.values.ptr), in.nnz,
                         static_cast<int64_t>(padded), c->xt_val.ptr);
    } else {
      c->xt_val.alloc(2);
    }
    if (norms_on_device) {
      DeviceBuffer<double> d_tval;
      DeviceBuffer<uint32_t> d_rptr;
      std::vector<int32_t> r_count;
      d_tval.alloc(static_cast<size_t>(in.nnz));
      d_tidx.alloc(static_cast<size_t>(in.nnz));
      transpose_csr_device(up.indptr.ptr, up.indices.ptr, static_cast<const double *>(up.values.ptr), in.m_rows, in.m_cols,
                           in.nnz, d_tidx.ptr, d_tval.ptr, r_count, tmp, s);
      std::vector<uint32_t> rptr(static_cast<size_t>(in.rows) + 1, 0u);
      for (int64_t i = 0; i < in.rows; i++) rptr[i + 1] = rptr[i] + static_cast<uint32_t>(r_count[i]);
      d_rptr.upload(rptr, s);
      d_ss.alloc(static_cast<size_t>(std::max<int64_t>(in.rows, 1)));
      hipLaunchKernelGGL(knn_row_sumsq_kernel, dim3(static_cast<unsigned>(ceil_div(in.rows, 4))), dim3(256), 0, s,
                         static_cast<const uint32_t *>(d_rptr.ptr), static_cast<const double *>(d_tval.ptr), in.rows,
                         d_ss.ptr);
      IRS_HIP(hipGetLastError());
      IRS_HIP(hipStreamSynchronize(s));  // (rptr and the scratch go out of scope)
    }
    xt_idx_src = up.indices.ptr;
    pt.mark("create: csc streams");
  }
  void device_norms() {
    std::vector<double> ss(static_cast<size_t>(in.rows), 0.0);
    IRS_HIP(hipGetLastError());
    if (in.rows > 0) IRS_HIP(hipMemcpyAsync(ss.data(), d_ss.ptr, static_cast<size_t>(in.rows) * sizeof(double),
                                        hipMemcpyDeviceToHost, s));
    IRS_HIP(hipStreamSynchronize(s));
    parallel_ranges(in.rows, [&](int64_t lo, int64_t hi) {
      for (int64_t i = lo; i < hi; i++) norms[i] = finish_norm(in.sim_type, in.alpha, ss[i]);
    }, 16, 20000);
    pt.mark("create: device norms");
  }
  // the slice pointers, the packed 16-bit offsets and the per-row value ranges of X_arg^T, the flags, the norms
  void slices_and_pack() {
    const int64_t n_tiles = std::max<int64_t>(1, ceil_div(in.rows, TILE));
    std::vector<uint32_t> xt_ptr(static_cast<size_t>(in.cols) + 1, 0u);
    c->xt_row_len.resize(in.cols);
    c->xt_rowmax.assign(in.cols, 0.0);
    c->xt_rowmin.assign(in.cols, 0.0);
    for (int64_t u = 0; u < in.cols; u++) {
      xt_ptr[u + 1] = xt_ptr[u] + static_cast<uint32_t>(t_count[u]);
      c->xt_row_len[u] = t_count[u];
      if (!stream_vals && t_count[u] > 0)
        c->xt_rowmax[u] = c->xt_rowmin[u] = sep_rowval.empty() ? 1.0 : std::fabs(sep_rowval[u]);
    }
    DeviceBuffer<uint32_t> d_xt_ptr;
    DeviceBuffer<double> d_range;
    d_xt_ptr.upload(xt_ptr, s);
    c->xt_tptr.alloc(static_cast<size_t>(in.cols) * (n_tiles + 1));
    const int64_t n_pairs = in.cols * (n_tiles + 1);
    hipLaunchKernelGGL(xt_slices_kernel, dim3(static_cast<unsigned>(ceil_div(n_pairs, 256))), dim3(256), 0, s,
                       static_cast<const uint32_t *>(d_xt_ptr.ptr), xt_idx_src, in.cols,
                       static_cast<int32_t>(n_tiles), c->xt_tptr.ptr);
    c->xt_idx16.alloc(padded / 2);
    hipLaunchKernelGGL(xt_pack16_kernel, dim3(static_cast<unsigned>(ceil_div(static_cast<int64_t>(padded / 2), 256))),
                       dim3(256), 0, s, xt_idx_src, in.nnz,
                       static_cast<int64_t>(padded / 2), c->xt_idx16.ptr);
    DeviceBuffer<int32_t> d_not_const;
    int32_t not_const = 1;
    if (stream_vals) {
      d_range.alloc(2 * static_cast<size_t>(in.cols));
      c->xt_rowval.alloc(static_cast<size_t>(in.cols));
      d_not_const.alloc(1);
      IRS_HIP(hipMemsetAsync(d_not_const.ptr, 0, sizeof(int32_t), s));
      hipLaunchKernelGGL(xt_row_range_kernel, dim3(static_cast<unsigned>(ceil_div(in.cols, 256))), dim3(256), 0, s,
                         static_cast<const uint32_t *>(d_xt_ptr.ptr), static_cast<const double *>(c->xt_val.ptr), in.cols,
                         d_range.ptr, d_range.ptr + in.cols, c->xt_rowval.ptr, d_not_const.ptr);
      IRS_HIP(hipMemcpyAsync(&not_const, d_not_const.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      IRS_HIP(hipMemcpyAsync(c->xt_rowmax.data(), d_range.ptr, static_cast<size_t>(in.cols) * sizeof(double),
                             hipMemcpyDeviceToHost, s));
      IRS_HIP(hipMemcpyAsync(c->xt_rowmin.data(), d_range.ptr + in.cols, static_cast<size_t>(in.cols) * sizeof(double),
                             hipMemcpyDeviceToHost, s));
    }
    IRS_HIP(hipGetLastError());
    c->xt_all_ones = !stream_vals && sep_rowval.empty();
    c->xt_nonzero = !(flags & NOT_SAFE);
    c->xt_positive = !(flags & NOT_POSITIVE);
    if (separable) {  // (the flags describe what the kernels multiply: the row factors)
      ValueClass vc;
      for (const double v : sep_rowval) vc.add(v);
      c->xt_nonzero = vc.safe;
      c->xt_positive = vc.positive;
      if (!sep_rowval.empty()) {
        c->xt_row_const = true;
        c->xt_rowval.upload(sep_rowval, s);
      }
      if (!sep_colscale.empty()) {
        c->col_scaled = true;
        c->col_scale.upload(sep_colscale, s);
      }
    }
    c->norm_max = norms.empty() ? 0.0 : *std::max_element(norms.begin(), norms.end());
    c->norms.upload(norms, s);
    IRS_HIP(hipStreamSynchronize(s));  // the host vectors and the device scratch go out of scope
    if (stream_vals && not_const == 0) {  // one value per feature row: the value stream is not needed
      c->xt_row_const = true;
      c->xt_val.release();
      c->xt_val.alloc(2);
    } else if (!c->xt_row_const) {
      c->xt_rowval.release();
    }
    pt.mark("create: slices + pack");
  }
};
// The construction on host threads: IRSPACK_AMD_KNN_DEVICE_CREATE=0 and empty matrices; the device
// construction is compared with it (test_device_create_is_the_host_create).
irs_knn_computer *create_on_host(const CreateInput &in, PhaseTimer &pt) {
  const int64_t rows = in.rows;
  const int32_t sim_type = in.sim_type;
  const double alpha = in.alpha;
  HostCsrD X = host_csr(rows, in.cols, in.indptr, in.indices, in.data);
  pt.mark("create: copy");
  std::vector<double> norms(rows, 0.0);
  // (similarities.hpp:20-28, 61-72; 96-107, 143-159: stored entries become 1; 198-222, 265-292: no norms)
  for_rows_parallel(X.indptr, rows, [&](int64_t i) {
    if (in.transforms()) return pow_normalise_row(X.indptr.data(), i, X.data.data(), alpha, X.data.data());
    double ss = 0;
    for (int64_t q = X.indptr[i]; q < X.indptr[i + 1]; q++) {
      if (in.binarises()) X.data[q] = 1;
      ss += X.data[q] * X.data[q];
    }
    norms[i] = finish_norm(sim_type, alpha, ss);
  });
  pt.mark("create: norms");
  require_device(in.device);
  pt.mark("create: device");
  auto c = new_computer(in);
  HostCsrD Xt = transpose(X);
  pt.mark("create: transpose");
  const int64_t xt_nnz = Xt.indptr[Xt.rows];
  c->xt_row_len.resize(Xt.rows);
  c->xt_rowmax.assign(Xt.rows, 0.0);
  c->xt_rowmin.assign(Xt.rows, 0.0);
  hipStream_t s = nullptr;
  const int64_t n_tiles = std::max<int64_t>(1, ceil_div(rows, TILE));
  check_arg(xt_nnz < (int64_t(1) << 31) - 1024, "nnz must be below 2^31.");
  std::vector<uint32_t> tptr(static_cast<size_t>(Xt.rows) * (n_tiles + 1));
  // columns relative to their tile as 16-bit LDS byte offsets (column * 4), two per dword;
  // 256 padding entries: the accumulate loop reads whole 128-entry strips from the (even)
  // start of a slice
  static_assert(TILE * 4 <= 65536, "tile-relative column offsets are stored in 16 bits");
  const size_t nnz = Xt.indices.size(), padded = (nnz + 256 + 1) & ~size_t(1);
  std::vector<uint32_t> idx_p(padded / 2, 0u);
  uint16_t *idx16 = reinterpret_cast<uint16_t *>(idx_p.data());  // little endian: entry e = half e
  std::atomic<unsigned> found(0);
  for_rows_parallel(Xt.indptr, Xt.rows, [&](int64_t u) {  // (row blocks of about equal entry counts)
    bool ones = true;
    ValueClass vc;
    c->xt_row_len[u] = Xt.indptr[u + 1] - Xt.indptr[u];
    double mx = 0.0, mn = std::numeric_limits<double>::infinity();
    for (int64_t q = Xt.indptr[u]; q < Xt.indptr[u + 1]; q++) {
      const double v = Xt.data[q], a = std::fabs(v);
      mx = std::max(mx, a);
      if (a > 0.0) mn = std::min(mn, a);
      ones &= v == 1.0;
      vc.add(v, a);
      idx16[q] = static_cast<uint16_t>((Xt.indices[q] % TILE) * 4);
    }
    c->xt_rowmax[u] = mx;
    c->xt_rowmin[u] = std::isfinite(mn) ? mn : 0.0;
    const int32_t *b = Xt.indices.data() + Xt.indptr[u], *e = Xt.indices.data() + Xt.indptr[u + 1];
    uint32_t *dst = tptr.data() + u * (n_tiles + 1);
    for (int64_t t = 0; t < n_tiles; t++)
      dst[t] = static_cast<uint32_t>(Xt.indptr[u] +
                                     (std::lower_bound(b, e, static_cast<int32_t>(t * TILE)) - b));
    dst[n_tiles] = static_cast<uint32_t>(Xt.indptr[u + 1]);
    const unsigned f = (ones ? 0u : NOT_ONES) | (vc.safe ? 0u : NOT_SAFE) | (vc.positive ? 0u : NOT_POSITIVE);
    if (f) found.fetch_or(f);
  });
  c->xt_tptr.upload(tptr, s);
  pt.mark("create: slices");
  c->xt_idx16.upload(idx_p, s);
  c->xt_all_ones = !(found & NOT_ONES);
  c->xt_nonzero = !(found & NOT_SAFE);
  c->xt_positive = !(found & NOT_POSITIVE);
  if (c->xt_all_ones) {  // the ONES kernels never read the value stream
    c->xt_val.alloc(2);
  } else {
    std::vector<double> val_p(Xt.data.begin(), Xt.data.end());
    val_p.resize(padded, 0.0);
    c->xt_val.upload(val_p, s);
  }
  IRS_HIP(hipStreamSynchronize(s));  // the host vectors go out of scope
  c->norm_max = norms.empty() ? 0.0 : *std::max_element(norms.begin(), norms.end());
  c->norms.upload(norms, s);
  IRS_HIP(hipStreamSynchronize(s));
  pt.mark("create: pack+upload");
  // (the host staging - half a gigabyte for 20 M entries - is released here rather than at
  // scope exit so that the phase shows up in the timing)
  auto *junk = new std::pair<HostCsrD, HostCsrD>();
  junk->first.indices.swap(X.indices);
  junk->first.data.swap(X.data);
  junk->second.indices.swap(Xt.indices);
  junk->second.data.swap(Xt.data);
  std::thread([junk] { delete junk; }).detach();  // (munmap of 480 MB takes 56 ms: nothing waits for it)
  pt.mark("create: release host");
  return c.release();
}

// ---------------------------------------------------------------- a compute call
// The rows of the call are taken in CHUNKS (contiguous row ranges of about equal entry counts): per
// chunk one host pass on several threads - index check, the per-row statistic of the epilogue, the
// multiply-add count that orders the launch, whether the values are all ones / free of zeros (which
// accumulator the kernel may use) - then the chunk's launches.  The pass over chunk k + 1 and the
// upload of its column indices (a second host thread) run while the device works on chunk k: of
// the 2.3 ms the pass takes on the ML-20M shape only the first chunk's share comes before the first
// kernel, and a finished chunk's rows are compacted and copied to the host beside the later chunks'
// kernels.  Every chunk chooses its kernel variant from its own rows (each variant gives the
// reference's values; section 3.4 of DESIGN.md).  Three chunks on large calls: a chunk lasts at least
// as long as its heaviest (row, tile) pair - 2.1 of the ML-20M call's 8.4 ms - so more, shorter
// chunks lengthen the device time (4: +0.5 ms, 8: +6 ms) by more than they take off the start.
// IRSPACK_AMD_KNN_CHUNKS overrides the count (1: the whole call at once; tests force small ones).
struct ComputeCall {
  irs_knn_computer *const c;
  irs_knn_computer::Scratch &sc;
  PhaseTimer pt;
  // the target: rows [row_begin, row_end) of (ip, ix, dv) - the caller's arrays or one of the private copies
  const int64_t rows, cols;
  const int64_t *ip;
  const int32_t *ix;
  const double *dv;
  const int64_t row_begin, row_end, n, top_k;
  const bool as_w;
  HostCsrD regrouped, T;  // a CSC-layout target by rows; as_w only: the transformed values
  bool target_unit = false, binarise = false;
  int64_t e_begin = 0, e_end = 0, out_k = 0, tile_k = 0;  // the plan
  size_t ne = 0;
  bool have_work = false, big = false, use_stage = false;
  int n_chunks = 1, n_tiles = 1, n_cu = 0;
  std::vector<int64_t> cb;  // chunk k = rows [cb[k], cb[k + 1])
  WideRule wide{std::getenv("IRSPACK_AMD_KNN_WIDE")};
  std::vector<double> tstat, tscale;  // per row of the call (the chunks fill their parts)
  std::vector<int64_t> work;
  std::vector<int32_t> order, slot_of, h_cnt;  // order: per chunk its rows (chunk-relative ids), heaviest first
  std::vector<double> ones_host;  // (binarise on a path that reads values: sized once for the largest chunk
  size_t ones_entries = 0;        //  - copies of it may be in flight, it must never move)
  // The row pointers and column indices of the call's rows travel to the device on a second
  // host thread, chunk by chunk, while this one walks them (the values follow later, and only if
  // the kernel reads them).  An index out of range is found by the walk before its chunk's kernel runs.
  std::string upload_error;
  std::thread uploader;
  std::atomic<int> uploaded{0};  // chunks whose indices are on the device
  // per chunk: "its merged rows are in out_idx / out_val"; the call's device span lies between ev_first
  // (before the first launch) and ev_last (after every chunk)
  std::vector<hipEvent_t> ev_done;
  hipEvent_t ev_first = nullptr, ev_last = nullptr;
  bool ev_first_recorded = false;
  int retired = 0;  // chunks whose results are on their way to the host
  // (before any member goes - on an exception too: the uploader is joined and the streams are drained
  // before the host arrays the device work reads are freed, then the events are destroyed)
  ~ComputeCall() {
    if (uploader.joinable()) uploader.join();
    if (have_work)
      for (hipStream_t st : {c->stream_in, c->stream_k, c->stream_out, c->stream})
        if (st) (void)hipStreamSynchronize(st);
    for (auto e : ev_done) if (e) (void)hipEventDestroy(e);
    if (ev_first) (void)hipEventDestroy(ev_first);
    if (ev_last) (void)hipEventDestroy(ev_last);
  }
  // A CSC-layout target (knn.py:79 passes `X_train_all.T`): the arrays are the rows of target^T
  // [cols, rows]; the call walks the target's ROWS, so its columns are regrouped here on host threads
  // (a counting sort that keeps a row's entries in ascending column order), into private arrays - the
  // indices only when every stored value is 1 or the similarity binarises them (the host pass and the
  // kernels then never read a value).
  void regroup_csc_target() {
    check_arg(rows < (int64_t(1) << 31) && cols < (int64_t(1) << 31), "too many rows.");
    for (int64_t u = 0; u < cols; u++) check_arg(ip[u + 1] >= ip[u], "malformed indptr.");
    const int64_t t_nnz = ip[cols];
    check_arg(t_nnz < (int64_t(1) << 31), "nnz must be below 2^31.");
    check_arg(t_nnz == 0 || (ix && dv), "bad matrix.");
    std::atomic<unsigned> flags(0);
    parallel_ranges(t_nnz, [&](int64_t b, int64_t e) { flags.fetch_or(scan_entries(ix, dv, b, e, rows, false)); });
    check_arg(!(flags & BAD_INDEX), "malformed matrix: column index out of range or indptr not monotone.");
    const bool sim_binarises = c->sim_type == IRS_SIM_JACCARD || c->sim_type == IRS_SIM_TVERSKY;
    target_unit = !as_w && (sim_binarises || !(flags & NOT_ONES));
    regrouped = transpose_pattern(cols, rows, ip, ix, target_unit ? nullptr : dv);
    ip = regrouped.indptr.data();
    ix = regrouped.indices.data();
    dv = target_unit ? nullptr : regrouped.data.data();
    pt.mark("regroup columns");
  }
  // Target preparation of compute_W (similarities.hpp:224-240, 294-324; mirrors its prologue): it alone
  // transforms the values, in a private copy; otherwise the caller's arrays are read in place, and only the
  // rows of this call are looked at.
  void compute_w_prologue() {
    T = host_csr(rows, cols, ip, ix, dv);
    std::vector<double> norm_temp(cols, 0.0), pop(rows, 0.0);
    // (the pow calls and the divisions run on several host threads; the column sums are
    // added in entry order on one, like the reference's loop, so they are the same numbers)
    if (c->sim_type == IRS_SIM_RP3BETA) {
      for_rows_parallel(T.indptr, rows, [&](int64_t i) {
        double sum = 0;
        for (int64_t q = T.indptr[i]; q < T.indptr[i + 1]; q++) sum += T.data[q];
        pop[i] = std::pow(sum, c->beta);
      });
    }
    for_rows_parallel(T.indptr, rows, [&](int64_t i) {
      for (int64_t q = T.indptr[i]; q < T.indptr[i + 1]; q++) T.data[q] = std::pow(T.data[q], c->alpha);
    });
    for (int64_t q = 0; q < T.indptr[rows]; q++) norm_temp[T.indices[q]] += T.data[q];
    for_rows_parallel(T.indptr, rows, [&](int64_t i) {
      for (int64_t q = T.indptr[i]; q < T.indptr[i + 1]; q++) {
        if (c->sim_type == IRS_SIM_RP3BETA)
          T.data[q] /= (norm_temp[T.indices[q]] * pop[i]);
        else
          T.data[q] /= norm_temp[T.indices[q]];
      }
    });
    ip = T.indptr.data();
    ix = T.indices.data();
    dv = T.data.data();
  }
  // the entry range of the call, its chunks, the sizes that follow from top_k
  void plan() {
    // (binarise: the target's values count as 1 - the similarity says so, or a CSC-layout target was all ones)
    binarise = c->sim_type == IRS_SIM_JACCARD || c->sim_type == IRS_SIM_TVERSKY || target_unit;
    tstat.assign(std::max<int64_t>(n, 1), 0.0);
    tscale.assign(std::max<int64_t>(n, 1), 1.0);
    work.assign(std::max<int64_t>(n, 1), 0);
    e_begin = ip[row_begin];
    e_end = ip[row_end];
    check_arg(e_begin >= 0 && e_end >= e_begin, "malformed indptr.");
    check_arg(e_end < (int64_t(1) << 31), "nnz must be below 2^31.");
    // the row pointers of the call must be monotone BEFORE anything walks or uploads them: the
    // threads of the pass cut [e_begin, e_end) by lower_bound, which on a non-monotone array yields
    // rows whose entries lie outside that range (an out-of-bounds host read instead of this error)
    for (int64_t i = row_begin; i < row_end; i++) check_arg(ip[i + 1] >= ip[i], "malformed indptr.");
    out_k = std::min<int64_t>(top_k, c->N);
    have_work = n > 0 && out_k > 0 && c->N > 0;
    ne = static_cast<size_t>(e_end - e_begin);
    n_chunks = chunk_count(std::getenv("IRSPACK_AMD_KNN_CHUNKS"), have_work, e_end - e_begin, n);  // (read per call)
    cb = chunk_bounds(ip, row_begin, row_end, n_chunks);
    n_tiles = static_cast<int>(ceil_div(std::max<int64_t>(c->N, 1), TILE));
    big = out_k > TOPK_CAP;  // row merge by threshold select (knn_merge_big_kernel)
    tile_k = std::min<int64_t>(out_k, TILE);
  }
  // streams and events (a dropped computer's first), the call's buffers carved out of the arena, the uploader
  void scratch_and_uploader() {
    IRS_HIP(hipSetDevice(c->device));
    if (!c->stream) knn_buffer_cache.hand_streams(c);
    // (each on its own: a creation that failed half way must not leave a later call with null streams)
    for (hipStream_t *st : c->all_streams())
      if (!*st) IRS_HIP(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    for (hipEvent_t *ev : {&c->ev_in, &c->ev_setup})
      if (!*ev) IRS_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    // carve the call's buffers out of the arena (the last result, which lives there too, is gone now)
    int64_t widest = 0;  // rows of the largest chunk: the candidate lists are one chunk's at a time
    for (int k = 0; k < n_chunks; k++) widest = std::max(widest, cb[k + 1] - cb[k]);
    const ArenaLayout L = arena_layout(n, ne, c->N, out_k, widest, n_chunks);
    if (sc.arena.count < L.total) knn_buffer_cache.hand_buffers(c, L.total);  // (a dropped computer's buffers first)
    sc.arena.alloc(L.total);
    int b = 0;  // (the blocks in the table's order)
    auto view = [&](auto &...buf) {
      ((check_arg(sizeof(*buf.ptr) == L.elem_size[b], "arena table."), buf.view(sc.arena.ptr + L.offset[b], L.count[b]), b++), ...);
    };
    view(sc.t_ptr, sc.t_idx, sc.t_stat, sc.t_scale, sc.order, sc.slot_of, sc.res_ptr, sc.cand_idx, sc.cand_val, sc.cand_cnt,
         sc.out_idx, sc.out_val, sc.out_cnt, c->res_idx, c->res_val, sc.cursor, sc.redo_list);
    uploader = std::thread([this] {
      try {
        IRS_HIP(hipSetDevice(c->device));
        std::vector<int64_t> rel(n + 1);
        for (int64_t i = 0; i <= n; i++) rel[i] = ip[row_begin + i] - e_begin;
        IRS_HIP(hipMemcpyAsync(sc.t_ptr.ptr, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream_up));
        for (int k = 0; k < n_chunks; k++) {
          const int64_t q0 = ip[cb[k]], q1 = ip[cb[k + 1]];
          if (q1 > q0)
            IRS_HIP(hipMemcpyAsync(sc.t_idx.ptr + (q0 - e_begin), ix + q0,
                                   static_cast<size_t>(q1 - q0) * sizeof(int32_t), hipMemcpyHostToDevice,
                                   c->stream_up));
          IRS_HIP(hipStreamSynchronize(c->stream_up));
          uploaded.store(k + 1, std::memory_order_release);
        }
      } catch (const std::exception &e) {
        upload_error = e.what();
        (void)hipStreamSynchronize(c->stream_up);  // `rel` goes out of scope
        uploaded.store(n_chunks, std::memory_order_release);
      }
    });
  }
  // the computer's last result is gone; the host tables of this one
  void reset_result(int64_t *nnz_out) {
    c->res_ptr.assign(n + 1, 0);
    c->res_nnz = 0;
    c->staged = false;
    c->last_ms = 0;
    c->last_macs = 0;
    c->last_walked = 0;
    *nnz_out = 0;
    order.resize(std::max<int64_t>(n, 1));
    ev_done.assign(n_chunks, nullptr);
    slot_of.resize(std::max<int64_t>(n, 1));
    h_cnt.resize(std::max<int64_t>(n, 1));
  }
  // the page-locked stage of the result, the cursors, the events of the call's device span
  void begin_device_work() {
    int64_t max_entries = 0;
    for (int k = 0; k < n_chunks; k++) max_entries = std::max(max_entries, ip[cb[k + 1]] - ip[cb[k]]);
    ones_entries = static_cast<size_t>(max_entries);
    const size_t cap = static_cast<size_t>(n) * out_k;  // entries the result can have
    // (c->res_idx / res_val hold `cap` entries: the chunks are compacted as they finish, before the total is known)
    // results of up to 1 GB also travel to a page-locked staging buffer, chunk by chunk as the chunks finish
    // (IRSPACK_AMD_KNN_STAGE=0: irs_knn_fetch copies from the device into the caller's arrays, as before round 5)
    const size_t bytes = cap * (sizeof(double) + sizeof(int32_t));
    // (not on a computer's FIRST call: page-locking 32 MB costs several milliseconds, more than the
    // staged copy saves once - `learn()` of a kNN recommender makes exactly one call)
    if (bytes <= (size_t(1) << 30) && (c->n_calls > 0 || c->stage_bytes >= bytes) &&
        env_flag("IRSPACK_AMD_KNN_STAGE", true)) {
      if (c->stage_bytes < bytes) {
        if (c->stage) (void)hipHostFree(c->stage);
        c->stage = nullptr;
        c->stage_bytes = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&c->stage), bytes, hipHostMallocDefault) == hipSuccess)
          c->stage_bytes = bytes;
        else
          (void)hipGetLastError();  // (no page-locked memory to be had: fetch from the device)
      }
      use_stage = c->stage_bytes >= bytes;
      c->stage_idx_offset = cap * sizeof(double);
    }
    IRS_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
    // [3 k + 0] pairs, [3 k + 1] pairs of the redo list, [3 k + 2] length of the redo list of chunk k
    IRS_HIP(hipMemsetAsync(sc.cursor.ptr, 0, 3 * static_cast<size_t>(n_chunks) * sizeof(int32_t), c->stream));
    IRS_HIP(hipEventRecord(c->ev_setup, c->stream));
    IRS_HIP(hipStreamWaitEvent(c->stream_k, c->ev_setup, 0));
    IRS_HIP(hipEventCreate(&ev_first));
    IRS_HIP(hipEventCreate(&ev_last));
  }
  // A chunk whose kernels are done: its counts come back, its rows of the CSR get their places (the
  // chunks are contiguous row ranges: the offsets continue from the chunk before), its winners are
  // compacted on the device and copied to the staging buffer - all on a stream of its own beside the
  // kernels of the later chunks.
  void retire(int j) {
    hipStream_t s = c->stream, s_out = c->stream_out;
    const int64_t rel0 = cb[j] - row_begin, nc = cb[j + 1] - cb[j];
    if (nc <= 0 || !ev_done[j]) return;
    // (the counts on the call's own stream, idle until the end: behind the earlier chunks' result copies
    // on s_out - copy kernels that crawl while the tile kernels hold the compute units - this thread
    // would wait milliseconds and launch the next chunk late)
    IRS_HIP(hipStreamWaitEvent(s, ev_done[j], 0));
    IRS_HIP(hipMemcpyAsync(h_cnt.data() + rel0, sc.out_cnt.ptr + rel0, nc * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    IRS_HIP(hipStreamSynchronize(s));
    IRS_HIP(hipStreamWaitEvent(s_out, ev_done[j], 0));
    for (int64_t i = rel0; i < rel0 + nc; i++) c->res_ptr[i + 1] = c->res_ptr[i] + h_cnt[slot_of[i]];
    const int64_t q0 = c->res_ptr[rel0], q1 = c->res_ptr[rel0 + nc];
    if (q1 == q0) return;
    IRS_HIP(hipMemcpyAsync(sc.res_ptr.ptr + rel0, c->res_ptr.data() + rel0, (nc + 1) * sizeof(int64_t),
                           hipMemcpyHostToDevice, s_out));
    hipLaunchKernelGGL(knn_compact_kernel, dim3(static_cast<unsigned>(ceil_div(nc, 4))), dim3(256), 0, s_out,
                       sc.out_idx.ptr, sc.out_val.ptr, sc.slot_of.ptr + rel0, sc.res_ptr.ptr + rel0, nc,
                       static_cast<int32_t>(out_k), c->res_idx.ptr, c->res_val.ptr);
    IRS_HIP(hipGetLastError());
    if (use_stage) {
      IRS_HIP(hipMemcpyAsync(c->stage + static_cast<size_t>(q0) * sizeof(double), c->res_val.ptr + q0,
                             static_cast<size_t>(q1 - q0) * sizeof(double), hipMemcpyDeviceToHost, s_out));
      IRS_HIP(hipMemcpyAsync(c->stage + c->stage_idx_offset + static_cast<size_t>(q0) * sizeof(int32_t),
                             c->res_idx.ptr + q0, static_cast<size_t>(q1 - q0) * sizeof(int32_t),
                             hipMemcpyDeviceToHost, s_out));
    }
  }
  // one chunk: the host pass over its rows, their order, its inputs, its launches; then whatever has finished
  void chunk(int ck) {
    const int64_t r_lo = cb[ck], r_hi = cb[ck + 1], nc = r_hi - r_lo, rel0 = r_lo - row_begin;
    if (nc <= 0 && n > 0) return;
    const FeatureRows xt{c->xt_row_len.data(), c->xt_rowmax.data(), c->xt_rowmin.data()};
    const unsigned tf =
        target_pass(ip, ix, dv, cols, r_lo, r_hi, row_begin, xt, c->sim_type, c->alpha, binarise, wide,
                    target_pass_threads(host_thread_cap(), ip[r_hi] - ip[r_lo]), tstat.data(), tscale.data(), work.data());
    check_arg(!(tf & BAD_INDEX), "malformed matrix: column index out of range or indptr not monotone.");
    pt.mark("target pass");
    if (!have_work) return;
    int64_t chunk_macs = 0;
    for (int64_t i = 0; i < nc; i++) chunk_macs += work[rel0 + i];
    c->last_macs += chunk_macs;
    // rows of the chunk, heaviest product row first (ids relative to the chunk's first row)
    heaviest_first(work.data() + rel0, nc, order.data() + rel0);
    pt.mark("work + order");
    const char *fast_env = std::getenv("IRSPACK_AMD_KNN_FAST");  // (0: no approximate selection, A/B; read per call)
    const double tstat_max =  // (looked at for Tversky only)
        c->sim_type == IRS_SIM_TVERSKY ? *std::max_element(tstat.begin() + rel0, tstat.begin() + rel0 + nc) : 0.0;
    const VariantInputs vi{c->xt_all_ones, c->xt_row_const, c->xt_nonzero, c->xt_positive, c->col_scaled,  // the computer
                           c->sim_type, c->normalize, c->alpha, c->beta, c->shrinkage, c->norm_max,
                           !(tf & NOT_ONES), !(tf & NOT_SAFE), !(tf & NOT_POSITIVE), tstat_max,  // the chunk
                           big, out_k, !(fast_env && fast_env[0] == '0')};  // the call
    const VariantChoice v = choose_variant(vi);
    upload_inputs(ck, v.acc32);
    c->last_walked += chunk_macs;  // (every multiply-add is added one by one)
    Params p = make_params(ck);
    if (!v.acc32 && (tf & ANY_WIDE)) {  // first limbs of the wide-range pairs, one tile per resident workgroup
      sc.hi_stash.alloc(static_cast<size_t>(std::max(n_cu, 1)) * TILE);
      p.hi_stash = sc.hi_stash.ptr;
    }
    // the chunk's column indices must have arrived (the uploader works ahead of the walk)
    while (uploaded.load(std::memory_order_acquire) <= ck) std::this_thread::yield();
    if (!upload_error.empty()) throw std::runtime_error(upload_error);
    pt.mark("uploads + flags");
    launch(ck, p, v);
    pt.mark("launches");
    // chunks that have finished meanwhile
    while (retired < ck && (!ev_done[retired] || hipEventQuery(ev_done[retired]) == hipSuccess)) retire(retired++);
    (void)hipGetLastError();  // (hipErrorNotReady of the query)
  }
  // the chunk's inputs, on their own stream (the kernels of the chunk before are still running on stream_k)
  void upload_inputs(int ck, bool acc32) {
    hipStream_t s_in = c->stream_in;
    const int64_t nc = cb[ck + 1] - cb[ck], rel0 = cb[ck] - row_begin, ce_begin = ip[cb[ck]];
    const size_t cne = static_cast<size_t>(ip[cb[ck + 1]] - ce_begin);
    if (acc32) {
      sc.t_val.alloc(1);
    } else {
      sc.t_val.alloc(std::max<size_t>(ne, 1));  // (whole call: the row pointers are relative to its first entry)
      if (binarise) {
        if (ones_host.empty()) ones_host.assign(std::max<size_t>(ones_entries, 1), 1.0);
        if (cne) IRS_HIP(hipMemcpyAsync(sc.t_val.ptr + (ce_begin - e_begin), ones_host.data(), cne * sizeof(double),
                                        hipMemcpyHostToDevice, s_in));
      } else if (cne) {
        IRS_HIP(hipMemcpyAsync(sc.t_val.ptr + (ce_begin - e_begin), dv + ce_begin, cne * sizeof(double),
                               hipMemcpyHostToDevice, s_in));
      }
    }
    IRS_HIP(hipMemcpyAsync(sc.t_stat.ptr + rel0, tstat.data() + rel0, nc * sizeof(double), hipMemcpyHostToDevice, s_in));
    IRS_HIP(hipMemcpyAsync(sc.t_scale.ptr + rel0, tscale.data() + rel0, nc * sizeof(double), hipMemcpyHostToDevice, s_in));
    IRS_HIP(hipMemcpyAsync(sc.order.ptr + rel0, order.data() + rel0, nc * sizeof(int32_t), hipMemcpyHostToDevice, s_in));
    slots_of_rows(order.data() + rel0, nc, static_cast<int32_t>(rel0), slot_of.data() + rel0);
    IRS_HIP(hipMemcpyAsync(sc.slot_of.ptr + rel0, slot_of.data() + rel0, nc * sizeof(int32_t), hipMemcpyHostToDevice, s_in));
    IRS_HIP(hipEventRecord(c->ev_in, s_in));
    IRS_HIP(hipStreamWaitEvent(c->stream_k, c->ev_in, 0));
  }
  // the kernels' arguments of chunk ck (hi_stash, redo_list and redo are set at the launch)
  Params make_params(int ck) const {
    const int64_t nc = cb[ck + 1] - cb[ck], rel0 = cb[ck] - row_begin;
    Params p;
    p.xt_tptr = c->xt_tptr.ptr;
    p.xt_idx16 = c->xt_idx16.ptr;
    p.xt_val = c->xt_val.ptr;
    p.xt_rowval = c->xt_row_const ? c->xt_rowval.ptr : nullptr;
    p.norms = c->norms.ptr;
    p.col_scale = c->col_scaled ? c->col_scale.ptr : nullptr;
    p.t_ptr = sc.t_ptr.ptr + rel0;  // (values relative to the CALL's first entry, like t_idx / t_val)
    p.t_idx = sc.t_idx.ptr;
    p.t_val = sc.t_val.ptr;
    p.t_stat = sc.t_stat.ptr + rel0;
    p.t_scale = sc.t_scale.ptr + rel0;
    p.hi_stash = nullptr;
    p.row_order = sc.order.ptr + rel0;
    p.n_rows = static_cast<int32_t>(nc);
    p.n_tiles = n_tiles;
    p.N = static_cast<int32_t>(c->N);
    p.sim_type = c->sim_type;
    p.normalize = c->normalize ? 1 : 0;
    p.shrinkage = c->shrinkage;
    p.alpha = c->alpha;
    p.beta = c->beta;
    p.shrink_f = static_cast<float>(c->shrinkage);
    p.alpha_f = static_cast<float>(c->alpha);
    p.beta_f = static_cast<float>(c->beta);
    p.top_k = static_cast<int32_t>(out_k);
    p.tile_k = static_cast<int32_t>(tile_k);
    p.cand_idx = sc.cand_idx.ptr;  // (scratch of one chunk at a time: the chunks follow one another on the stream)
    p.cand_val = sc.cand_val.ptr;
    p.cand_cnt = sc.cand_cnt.ptr;
    p.out_idx = sc.out_idx.ptr + static_cast<size_t>(rel0) * out_k;
    p.out_val = sc.out_val.ptr + static_cast<size_t>(rel0) * out_k;
    p.out_cnt = sc.out_cnt.ptr + rel0;
    p.cursor = sc.cursor.ptr + 3 * ck;
    p.redo_count = p.cursor + 2;
    p.redo_list = nullptr;
    p.redo = 0;
    {  // merge buffer: all tiles' candidates at once when they fit, else rounds of MERGE_CAP
      int64_t want = std::max<int64_t>(2 * out_k, std::min<int64_t>(int64_t(n_tiles) * out_k, MERGE_CAP));
      int cap = 64;
      while (cap < want) cap <<= 1;
      p.merge_cap = std::min(cap, MERGE_CAP);
    }
    p.n_slots = static_cast<int32_t>(static_cast<size_t>(nc) * n_tiles);
    return p;
  }
  // the tile kernel of the chunk's variant (persistent: one resident workgroup per CU - its LDS footprint
  // allows no second), the exact redo launch of the approximate selection, the row merge
  void launch(int ck, Params &p, const VariantChoice &v) {
    hipStream_t ks = c->stream_k;
    const size_t lds = TILE * sizeof(double) + (TILE / 32) * sizeof(uint32_t) +
                       256 * sizeof(uint32_t) + 16 * sizeof(int32_t) + 64 * sizeof(double);
    const unsigned grid = static_cast<unsigned>(
        std::min<size_t>(static_cast<size_t>(p.n_slots), static_cast<size_t>(std::max(n_cu, 1))));
    auto tile = [&](auto kernel) {
      IRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(lds)));
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), lds, ks, p);
    };
    if (!ev_first_recorded) {
      IRS_HIP(hipEventRecord(ev_first, ks));
      ev_first_recorded = true;
    }
    switch (v.first) {
      case TileVariant::FAST_COUNTS:
        p.redo_list = sc.redo_list.ptr;
        tile(knn_tile_kernel<true, true, true, true>);
        break;
      case TileVariant::COUNTS: tile(knn_tile_kernel<true, true, true>); break;
      case TileVariant::ONES_SENTINEL: tile(knn_tile_kernel<true, true>); break;
      case TileVariant::ONES_BITMAP: tile(knn_tile_kernel<true, false>); break;
      case TileVariant::VALUES_SENTINEL: tile(knn_tile_kernel<false, true>); break;
      case TileVariant::VALUES_BITMAP: tile(knn_tile_kernel<false, false>); break;
    }
    if (v.exact_redo) {
      p.redo = 1;  // the pairs the approximate selection handed back (usually none), exactly
      tile(knn_tile_kernel<true, true, true>);
      p.redo = 0;
    }
    if (big) {
      hipLaunchKernelGGL(knn_merge_big_kernel, dim3(static_cast<unsigned>(p.n_rows)), dim3(256), 0, ks, p);
    } else {
      IRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(knn_merge_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, MERGE_CAP * 20));
      hipLaunchKernelGGL(knn_merge_kernel, dim3(static_cast<unsigned>(p.n_rows)), dim3(256),
                         static_cast<size_t>(p.merge_cap) * 20, ks, p);
    }
    IRS_HIP(hipEventCreateWithFlags(&ev_done[ck], hipEventDisableTiming));
    IRS_HIP(hipEventRecord(ev_done[ck], ks));
    IRS_HIP(hipGetLastError());
  }
  // every chunk retired, the device span measured, the result's size
  void finish(int64_t *nnz_out) {
    hipStream_t s = c->stream;
    for (; retired < n_chunks; retired++) retire(retired);  // (waits for each in turn)
    for (int ck = 0; ck < n_chunks; ck++)
      if (ev_done[ck]) IRS_HIP(hipStreamWaitEvent(s, ev_done[ck], 0));
    IRS_HIP(hipEventRecord(ev_last, s));
    IRS_HIP(hipStreamSynchronize(c->stream_out));
    IRS_HIP(hipStreamSynchronize(s));
    if (ev_first_recorded) {  // first launch .. last merge, the waits for the host in between included
      float ms = 0;
      IRS_HIP(hipEventElapsedTime(&ms, ev_first, ev_last));
      c->last_ms = ms;
    }
    c->res_nnz = c->res_ptr[n];
    c->staged = use_stage && c->res_nnz > 0;
    c->n_calls++;
    pt.mark("kernels + retire");
#ifdef IRS_KNN_PHASES
    {
      unsigned long long h[8] = {0}, z[8] = {0};
      IRS_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(knn_phase_clk), sizeof(h)));
      IRS_HIP(hipMemcpyToSymbol(HIP_SYMBOL(knn_phase_clk), z, sizeof(z)));
      fprintf(stderr, "knn phases (10 ns ticks, sum over the WGs): init %llu acc %llu bitmap %llu epi %llu select %llu write %llu\n",
              h[0], h[1], h[2], h[3], h[4], h[5]);
      IRS_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(knn_fast_stat), sizeof(h)));
      IRS_HIP(hipMemcpyToSymbol(HIP_SYMBOL(knn_fast_stat), z, sizeof(z)));
      fprintf(stderr, "knn fast path: pairs %llu exact-path %llu candidates %llu; pairs with <= 128 / 256 / 512 / 1024 candidates: %llu %llu %llu %llu\n",
              h[0], h[1], h[2], h[3], h[4], h[5], h[6]);
    }
#endif
    *nnz_out = c->res_ptr[n];
    pt.mark("assemble");
  }
};

}  // namespace

extern "C" {

irs_status irs_knn_create(int32_t sim_type, int64_t rows, int64_t cols, const int64_t *indptr,
                          const int32_t *indices, const double *data, const irs_knn_input *input,
                          double shrinkage, double alpha, double beta, int32_t normalize, int64_t n_threads,
                          int64_t max_chunk_size, int32_t device, irs_knn_computer **out) {
  return guard([&] {
    PhaseTimer pt;
    CreateInput in = check_create_args(sim_type, rows, cols, indptr, indices, data, input, shrinkage, alpha, beta,
                                       normalize, n_threads, max_chunk_size, device, out);
    host_regroup(in, pt);
    if (in.device_candidate) {
      require_device(device);
      IRS_HIP(hipSetDevice(device));
      *out = DeviceCreate(in, pt).run();
    } else {
      *out = create_on_host(in, pt);
    }
  });
}

irs_status irs_knn_weight(int32_t weighting, int64_t rows, int64_t cols, const int64_t *indptr,
                          const int32_t *indices, const double *data, double k1, double b, int32_t smooth,
                          int32_t device, double *out) {
  return guard([&] {
    check_arg(weighting == IRS_WEIGHT_TF_IDF || weighting == IRS_WEIGHT_BM25, "unknown feature weighting.");
    check_arg(rows >= 0 && cols >= 0 && indptr && indptr[0] == 0, "bad matrix.");
    for (int64_t i = 0; i < rows; i++) check_arg(indptr[i + 1] >= indptr[i], "malformed indptr.");
    const int64_t nnz = indptr[rows];
    if (nnz == 0) return;
    check_arg(indices && data && out, "bad matrix.");
    check_arg(nnz < (int64_t(1) << 31), "nnz must be below 2^31.");
    PhaseTimer pt;
    require_device(device);
    IRS_HIP(hipSetDevice(device));
    const bool bm25 = weighting == IRS_WEIGHT_BM25;
    // the uploads beside the validation and the tables; the result's buffer is allocated on the way
    CsrUploader up(device, rows, nnz, indptr, indices, static_cast<size_t>(nnz));
    std::atomic<unsigned> flags(0);
    parallel_ranges(nnz, [&](int64_t lo, int64_t hi) { flags.fetch_or(scan_entries(indices, data, lo, hi, cols, false)); });
    check_arg(!(flags & BAD_INDEX), "column index out of range.");
    const bool ones = !(flags & NOT_ONES);
    up.classified(ones, data);
    pt.mark("weight: validate");
    const WeightTables wt = weight_tables(bm25, rows, cols, indptr, indices, data, ones, k1, b, smooth != 0);
    pt.mark("weight: tables");
    up.finish();
    hipStream_t s = nullptr;
    DeviceBuffer<double> d_idf, d_reg;
    d_idf.upload(wt.idf, s);
    if (bm25) d_reg.upload(wt.reg, s);
    launch_weight(bm25, up.indptr, up.indices, ones ? nullptr : up.values.ptr, d_idf, d_reg, k1, rows, up.extra.ptr,
                  nullptr, s);
    pt.mark("weight: upload + launch");
    IRS_HIP(hipStreamSynchronize(s));
    if (!copy_to_host_threaded(device, nnz, int64_t(1) << 21, out, up.extra.ptr, nullptr, nullptr))
      throw std::runtime_error("copying the weighted values to the host failed.");
    pt.mark("weight: result copy");
  });
}

irs_status irs_knn_destroy(irs_knn_computer *c) {
  return guard([&] {
    if (c) {
      (void)hipSetDevice(c->device);
      for (hipStream_t *st : c->all_streams())
        if (*st) (void)hipStreamSynchronize(*st);
      knn_buffer_cache.keep(c);  // leave the larger buffers to the next computer on this device
      delete c;
    }
  });
}

irs_status irs_knn_compute(irs_knn_computer *c, int64_t rows, int64_t cols,
                           const int64_t *indptr, const int32_t *indices, const double *data,
                           int32_t layout, int64_t top_k, int32_t as_w, int64_t row_begin, int64_t row_end,
                           int64_t *nnz_out) {
  return guard([&] {
    check_arg(c && nnz_out, "null argument.");
    if (cols != c->n_features) throw std::invalid_argument("illegal # of feature.");  // knn.hpp:44-45
    check_arg(top_k >= 0, "top_k must be non-negative.");
    PhaseTimer pt;
    check_arg(rows >= 0 && cols >= 0 && indptr && indptr[0] == 0, "bad matrix.");
    check_arg(0 <= row_begin && row_begin <= row_end && row_end <= rows, "row range out of bounds.");
    check_arg(layout == IRS_LAYOUT_CSR || layout == IRS_LAYOUT_CSC, "unknown matrix layout.");
    ComputeCall call{c, c->scratch, pt, rows, cols, indptr, indices, data, row_begin, row_end, row_end - row_begin, top_k, as_w != 0};
    if (layout == IRS_LAYOUT_CSC) call.regroup_csc_target();
    if (as_w) call.compute_w_prologue();
    call.pt.mark("compute_W prologue");
    call.plan();
    if (call.have_work) call.scratch_and_uploader();
    call.reset_result(nnz_out);
    if (call.have_work) call.begin_device_work();
    call.pt.mark("set-up");
    for (int ck = 0; ck < call.n_chunks; ck++) call.chunk(ck);
    if (call.have_work) call.finish(nnz_out);
  });
}

irs_status irs_knn_fetch(irs_knn_computer *c, int64_t *indptr, int32_t *indices, double *data) {
  return guard([&] {
    check_arg(c && indptr, "null argument.");
    std::copy(c->res_ptr.begin(), c->res_ptr.end(), indptr);
    if (c->res_nnz > 0) check_arg(indices && data, "null argument.");
    if (c->res_nnz > 0 && c->staged) {  // page-locked copy of the result -> the caller's arrays
      copy_from_stage(c->stage, c->stage + c->stage_idx_offset, c->res_nnz, data, indices);
    } else if (c->res_nnz > 0) {  // device -> the caller's arrays, one copy each
      IRS_HIP(hipSetDevice(c->device));
      IRS_HIP(hipMemcpy(indices, c->res_idx.ptr, static_cast<size_t>(c->res_nnz) * sizeof(int32_t), hipMemcpyDeviceToHost));
      IRS_HIP(hipMemcpy(data, c->res_val.ptr, static_cast<size_t>(c->res_nnz) * sizeof(double), hipMemcpyDeviceToHost));
    }
  });
}

irs_status irs_knn_fetch_csc(irs_knn_computer *c, int64_t zero_diagonal_row0, int64_t *col_ptr, int32_t *row_idx,
                             double *data) {
  return guard([&] {
    check_arg(c && col_ptr, "null argument.");
    const int64_t n = static_cast<int64_t>(c->res_ptr.size()) - 1, N = c->N, nnz = c->res_nnz;
    std::fill(col_ptr, col_ptr + N + 1, int64_t(0));
    if (nnz <= 0) return;
    check_arg(row_idx && data, "null argument.");
    check_arg(nnz < (int64_t(1) << 31), "nnz must be below 2^31.");
    IRS_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;  // (idle: the compute call that made the result has returned)
    // Scratch out of the compute call's arena: its merged-row buffers (out_idx / out_val, sized like the result)
    // and the target's column indices (t_idx: tens of MB) are dead once the call has returned - five hipMalloc /
    // hipFree pairs per learn() were 4 of this call's 13 ms.
    irs_knn_computer::Scratch &sc = c->scratch;
    const bool arena = sc.out_idx.ptr && sc.out_idx.count >= static_cast<size_t>(nnz) &&
                       sc.out_val.count >= static_cast<size_t>(nnz) && sc.t_idx.ptr;
    DeviceBuffer<int32_t> own_tidx, d_rp, d_cp;
    DeviceBuffer<double> own_tval;
    DeviceBuffer<char> tmp;
    int32_t *t_idx = nullptr;
    double *t_val = nullptr;
    if (arena) {
      t_idx = sc.out_idx.ptr;
      t_val = sc.out_val.ptr;
      tmp.view(sc.t_idx.ptr, sc.t_idx.count * sizeof(int32_t));
    } else {
      own_tidx.alloc(static_cast<size_t>(nnz));
      own_tval.alloc(static_cast<size_t>(nnz));
      t_idx = own_tidx.ptr;
      t_val = own_tval.ptr;
    }
    std::vector<int32_t> rp(static_cast<size_t>(n) + 1);
    for (int64_t i = 0; i <= n; i++) rp[i] = static_cast<int32_t>(c->res_ptr[i]);
    d_rp.upload(rp, s);
    std::vector<int32_t> t_count;
    transpose_csr_device(d_rp.ptr, c->res_idx.ptr, static_cast<const double *>(c->res_val.ptr), n, N, nnz, t_idx, t_val,
                         t_count, tmp, s);
    for (int64_t j = 0; j < N; j++) col_ptr[j + 1] = col_ptr[j] + t_count[j];
    if (zero_diagonal_row0 >= 0) {
      std::vector<int32_t> cp(static_cast<size_t>(N) + 1);
      for (int64_t j = 0; j <= N; j++) cp[j] = static_cast<int32_t>(col_ptr[j]);
      d_cp.upload(cp, s);
      hipLaunchKernelGGL(knn_zero_diagonal_csc_kernel, dim3(static_cast<unsigned>(ceil_div(N, 256))), dim3(256), 0, s,
                         static_cast<const int32_t *>(d_cp.ptr), static_cast<const int32_t *>(t_idx), N,
                         zero_diagonal_row0, t_val);
      IRS_HIP(hipGetLastError());
      IRS_HIP(hipStreamSynchronize(s));  // (cp goes out of scope)
    }
    // To the caller's (pageable, usually untouched) arrays: through the computer's page-locked staging buffer
    // when it has one of the size (one copy at the link's rate + a threaded host copy; the staged CSR copy of the
    // result is gone afterwards), else a few device-to-host copies side by side (see irs_knn_weight).
    const size_t need = static_cast<size_t>(nnz) * (sizeof(double) + sizeof(int32_t));
    if (c->stage && c->stage_bytes >= need) {
      c->staged = false;
      char *sv = c->stage, *si = c->stage + static_cast<size_t>(nnz) * sizeof(double);
      IRS_HIP(hipMemcpyAsync(sv, t_val, static_cast<size_t>(nnz) * sizeof(double), hipMemcpyDeviceToHost, s));
      IRS_HIP(hipMemcpyAsync(si, t_idx, static_cast<size_t>(nnz) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      IRS_HIP(hipStreamSynchronize(s));
      copy_from_stage(sv, si, nnz, data, row_idx);
      return;
    }
    if (!copy_to_host_threaded(c->device, nnz, int64_t(1) << 20, data, t_val, row_idx, t_idx))
      throw std::runtime_error("copying the result to the host failed.");
  });
}

irs_status irs_knn_last_walked(irs_knn_computer *c, int64_t *walked_macs, int32_t *dense_rows) {
  return guard([&] {
    check_arg(c && walked_macs && dense_rows, "null argument.");
    *walked_macs = c->last_walked;
    *dense_rows = 0;  // (the dense block of the popular items was removed in round 5)
  });
}

irs_status irs_knn_last_stats(irs_knn_computer *c, double *kernel_ms, int64_t *macs) {
  return guard([&] {
    check_arg(c && kernel_ms && macs, "null argument.");
    *kernel_ms = c->last_ms;
    *macs = c->last_macs;
  });
}

// remove_diagonal, util.hpp:211-226: stored diagonal entries become explicit zeros
irs_status irs_remove_diagonal(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices, double *data) {
  return guard([&] {
    check_arg(rows == cols, "X must be square");
    check_arg(indptr && (indptr[rows] == 0 || (indices && data)), "null argument.");
    for (int64_t i = 0; i < rows; i++)
      for (int64_t q = indptr[i]; q < indptr[i + 1]; q++)
        if (indices[q] == i) data[q] = 0.0;
  });
}

}  // extern "C"
