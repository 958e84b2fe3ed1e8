// Ranking-metric evaluator on gfx950.  Replaces EvaluatorCore::get_metrics /
// get_metrics_local / Metrics::update of /root/reference/cpp_source/evaluator.cpp
// (:256-284, :292-367, :127-166) behind include/irspack_amd.h.
//
// One workgroup ranks one user row (1024 threads with the row's keys held in registers or
// LDS after one pass over the scores, else 256 threads re-reading the scores per pass):
//   1. candidates = all items | global list | per-user list, score != -inf (:324-348)
//   2. top-`cutoff` by the total order (score desc, index asc) — the order
//      std::partial_sort gives on (-score, index) pairs (:329, :353-355):
//      MSB-first 8-bit radix select of the cutoff-th key (wave-aggregated histogram, early
//      exit), then an index-ordered pick of the ties at the threshold, then a bitonic sort
//      of the winners (a shuffle network in one wave for cutoff <= 64, else in LDS)
//   3. hits against the (recommendable-filtered) ground-truth row, then the sequential
//      dcg / AP recurrences of Metrics::update
// Per-user terms are folded by a fixed-order wave reduction (double), item counts with
// int64 atomics.  The same kernel serves retrieve_recommend_from_score (no ground truth).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <limits>
#include <memory>

#include <thread>
#include <cstring>

#include "common.hpp"
#include "eval_host_prep.hpp"
#include "eval_emit_plan.hpp"

// the kernels, in this order (each header names what it needs from the ones before it)
#include "eval_rank_kernels.hpp"
#include "eval_fused_kernels.hpp"
#include "eval_cand_kernels.hpp"
#include "eval_reduce_kernels.hpp"
#include "eval_sim_kernels.hpp"
#include "eval_dense_kernels.hpp"
#include "serve_kernels.hpp"
#include "eval_fold_kernels.hpp"

using namespace irs;
using namespace irs::eval;

// exported by ials.hip: user[0:m] @ item^T of factor tables the CALLER holds on the device ([rows, KP]
// row-major, KP a multiple of 32, padded columns zero) through the fp32 MFMA tiles of the iALS scores
extern "C" irs_status irs_gk_scores_device_(const float *user, const float *item, int32_t KP, int64_t m,
                                            int64_t n_items, float *device_out, int64_t ld, void *stream);
// exported by ials.hip for the fused path
extern "C" irs_status irs_ials_scores_device_(irs_ials_trainer *t, int64_t begin, int64_t end,
                                              float *device_out, void **stream_out,
                                              int32_t *device_index);
extern "C" irs_status irs_ials_scores_prefix_device_(irs_ials_trainer *t, int64_t begin, int64_t end,
                                                     int64_t n_prefix, const float *item_rows,
                                                     const float *user_rows, float *device_out);
extern "C" irs_status irs_ials_factors_device_(irs_ials_trainer *t, const float **user,
                                               const float **item, int32_t *KP, int64_t *n_users,
                                               int64_t *n_items, void **stream_out,
                                               int32_t *device_index);

struct irs_evaluator {
  int device = 0;
  int64_t n_users = 0, n_items = 0;
  int rec_mode = 0;
  DeviceBuffer<int32_t> gt_ptr, gt_idx, rec_items;
  DeviceBuffer<int64_t> rec_ptr;
  DeviceBuffer<double> disc, idcg_prefix;
  DeviceBuffer<RowOut> row_out;
  DeviceBuffer<int32_t> rec_out, todo;
  DeviceBuffer<unsigned long long> item_cnt;
  DeviceBuffer<irs_metrics> metrics;
  DeviceBuffer<char> score_buf;
  // mask of the fused path kept on the device between calls (irs_eval_cache_mask)
  DeviceBuffer<int64_t> mask_ptr;
  DeviceBuffer<int32_t> mask_idx;
  int64_t mask_rows = -1;
  DeviceBuffer<float> fused_scores;  // score block of the two-pass path, kept between calls
  // fused call (eval_fused_kernels.hpp): the cached mask as a bitmap + scratch of the emit path
  DeviceBuffer<uint64_t> mask_bits;
  DeviceBuffer<int32_t> mask_count;
  int64_t mask_bits_rows = -1;  // rows the bitmap was built for (-1: none)
  DeviceBuffer<float> cand_score, tau;
  DeviceBuffer<int32_t> cand_item, cand_cnt, bad_flag;
  // bounded variant of the emit path: norms, the two sort permutations, per-tile limits
  DeviceBuffer<float> inorm, inorm_sorted, unorm, radius, radius_sorted, sample_item, hard_user;
  DeviceBuffer<int32_t> iota, iperm, iinv, uperm, limit_tiles, hard, hard_list, wg_prefix;
  DeviceBuffer<int4> wg_desc;
  DeviceBuffer<char> sort_tmp;
  int32_t *flags_host = nullptr;  // page-locked: the emit path's flags / hard-row count / scored tiles, one copy per pass
  DeviceBuffer<RowPartial> row_partials;  // chunk sums of the two-level reduction
  DeviceBuffer<int32_t> mask_row;         // row of every mask entry (built with the bitmap)
  std::vector<int64_t> mask_ptr_host;     // host copy of the mask's row pointers
  irs_eval_stats stats{};  // of the last irs_eval_get_metrics_ials call
  hipEvent_t ev_first = nullptr, ev_last = nullptr;  // span of that call's device work
  bool span_open = false;
  double phase_ms[4] = {0.0, 0.0, 0.0, 0.0};  // of the last dense-similarity / factor-model call (irs_eval_last_phases)
};

namespace {

void validate_call(irs_evaluator *e, int64_t rows, int64_t cutoff, int64_t offset,
                   int64_t n_threads) {
  // evaluator.cpp:209, 263-268
  check_arg(n_threads > 0, "n_threads must be strictly positive.");
  check_arg(offset >= 0 && e->n_users > offset, "got offset >= n_users");
  check_arg(offset + rows <= e->n_users, "offset + scores.shape[0] exceeds n_users");
  check_arg(cutoff > 0, "cutoff must be strictly greather than 0.");
  check_arg(cutoff <= e->n_items, "cutoff must not exeeed the number of items.");
}

// IRSPACK_AMD_EVAL_WAVE=0: general kernel only (read per call: tests toggle it)
bool wave_enabled() {
  const char *e = std::getenv("IRSPACK_AMD_EVAL_WAVE");
  return !(e && e[0] == '0');
}

// cutoff > SEL_CAP: the lists of a launch's workgroups in global scratch (13 bytes per entry,
// big_cap entries per row), at most ~1 GiB of it: the rows go through in launches of
// `big_rows` rows.  Rare (the reference's callers use cutoffs of 5..100), so the goal is only to be
// correct for every cutoff the reference accepts and not slower than its partial_sort.
template <class T, bool POS = false> void launch_rank_big(EvalParams p, const RankPlan &r, hipStream_t s) {
  DeviceBuffer<uint64_t> bk;
  DeviceBuffer<int32_t> bi;
  DeviceBuffer<uint8_t> bh;
  bk.alloc(static_cast<size_t>(r.big_rows) * r.big_cap);
  bi.alloc(static_cast<size_t>(r.big_rows) * r.big_cap);
  bh.alloc(static_cast<size_t>(r.big_rows) * r.big_cap);
  p.big_key = bk.ptr;
  p.big_idx = bi.ptr;
  p.big_hit = bh.ptr;
  p.big_cap = static_cast<int32_t>(r.big_cap);
  p.todo = nullptr;
  for (int64_t b = 0; b < p.rows; b += r.big_rows) {
    const unsigned m = static_cast<unsigned>(std::min<int64_t>(r.big_rows, p.rows - b));
    p.row_base = b;
    if (r.mode == 1) {
      auto kernel = rank_rows_kernel<T, 1024, 1, RANK_MAXQ, true, POS>;
      IRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(r.key_bytes)));
      hipLaunchKernelGGL(kernel, dim3(m), dim3(1024), r.key_bytes, s, p);
    } else {
      hipLaunchKernelGGL((rank_rows_kernel<T, 256, 0, RANK_MAXQ, true, POS>), dim3(m), dim3(256), 0, s, p);
    }
  }
  IRS_HIP(hipGetLastError());
  IRS_HIP(hipStreamSynchronize(s));  // the scratch is released on return
}

// Ranks the rows of `p` with the kernels plan_rank names (`todo`: scratch of one flag per row, or null = the
// general kernel for every row).
template <class T, bool POS = false> void launch_rank(EvalParams p, int64_t max_cand, hipStream_t s, int32_t *todo) {
  const RankPlan r = plan_rank(p.cutoff, p.rows, max_cand, std::is_same<T, float>::value, p.rec_mode, p.n_items,
                               wave_enabled(), todo != nullptr);
  if (r.big) {
    launch_rank_big<T, POS>(p, r, s);
    return;
  }
  p.todo = nullptr;
  if (r.wave) {
    p.todo = todo;
    const dim3 grid(static_cast<unsigned>((p.rows + 3) / 4));
    if (r.wave_m == 4)
      hipLaunchKernelGGL((rank_wave_kernel<T, 4>), grid, dim3(256), 0, s, p);
    else
      hipLaunchKernelGGL((rank_wave_kernel<T, 8>), grid, dim3(256), 0, s, p);
  }
  if (r.mode == 2) {
    hipLaunchKernelGGL((rank_rows_kernel<T, 1024, 2, RANK_MAXQ, false, POS>), dim3(p.rows), dim3(1024), 0, s, p);
  } else if (r.mode == 1) {
    auto kernel = rank_rows_kernel<T, 1024, 1, RANK_MAXQ, false, POS>;
    IRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(r.key_bytes)));
    hipLaunchKernelGGL(kernel, dim3(p.rows), dim3(1024), r.key_bytes, s, p);
  } else {
    hipLaunchKernelGGL((rank_rows_kernel<T, 256, 0, RANK_MAXQ, false, POS>), dim3(p.rows), dim3(256), 0, s, p);
  }
}

// item_cnt += the histogram of the `n` list entries at `rec`
void launch_item_hist(const int32_t *rec, int64_t n, unsigned long long *item_cnt, hipStream_t s, int64_t n_items) {
  const HistPlan h = plan_item_hist(n, n_items);
  if (h.grid <= 0) return;
  if (h.direct) {
    IRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(item_hist_direct_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(HIST_DIRECT_MAX * sizeof(uint32_t))));
    hipLaunchKernelGGL(item_hist_direct_kernel, dim3(static_cast<unsigned>(h.grid)), dim3(1024),
                       static_cast<size_t>(n_items) * sizeof(uint32_t), s, rec, n, static_cast<int32_t>(n_items), item_cnt);
  } else {
    hipLaunchKernelGGL(item_hist_kernel, dim3(static_cast<unsigned>(h.grid)), dim3(1024), 0, s, rec, n, item_cnt);
  }
}

// EvalParams of a ranking against the evaluator's ground truth (retrieve = 0): rows [offset, offset + rows) of the
// evaluator, lists into e->rec_out, per-user terms into e->row_out (both sized here)
EvalParams metric_params(irs_evaluator *e, const void *scores, int64_t rows, int64_t cutoff, int64_t offset, bool rwc) {
  e->row_out.alloc(rows);
  e->rec_out.alloc(rows * cutoff);
  e->todo.alloc(rows);
  EvalParams p{};
  p.scores = scores;
  p.rows = rows;
  p.n_items = e->n_items;
  p.offset = offset;
  p.gt_ptr = e->gt_ptr.ptr;
  p.gt_idx = e->gt_idx.ptr;
  p.rec_mode = e->rec_mode;
  p.rec_ptr = e->rec_ptr.ptr;
  p.rec_items = e->rec_items.ptr;
  p.cutoff = static_cast<int32_t>(cutoff);
  p.retrieve = 0;
  p.recall_with_cutoff = rwc ? 1 : 0;
  p.disc = e->disc.ptr;
  p.idcg_prefix = e->idcg_prefix.ptr;
  p.out = e->row_out.ptr;
  p.rec_out = e->rec_out.ptr;
  p.item_cnt = e->item_cnt.ptr;
  return p;
}

// ranks `rows` rows already resident at `d_scores` and accumulates into out / item_cnt
// (`running`, when given: the per-user terms are added to `running` in HOST_LOOP_ROWS-row chunks, chunk after
// chunk, instead of to e->metrics - see CutoffTotals)
template <class T>
void rank_block(irs_evaluator *e, const void *d_scores, int64_t rows, int64_t cutoff,
                int64_t offset, bool rwc, hipStream_t s, irs_metrics *running = nullptr) {
  const EvalParams p = metric_params(e, d_scores, rows, cutoff, offset, rwc);
  launch_rank<T>(p, e->n_items, s, e->todo.ptr);
  launch_item_hist(e->rec_out.ptr, rows * cutoff, e->item_cnt.ptr, s, e->n_items);
  if (running) {
    const int nb = static_cast<int>(ceil_div(rows, HOST_LOOP_ROWS));
    e->row_partials.alloc(nb);
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(nb), dim3(1024), 0, s, e->row_out.ptr, rows, running,
                       e->row_partials.ptr, HOST_LOOP_ROWS);
    hipLaunchKernelGGL(merge_partials_kernel, dim3(1), dim3(64), 0, s,
                       static_cast<const RowPartial *>(e->row_partials.ptr), nb, rows, running);
  } else {
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(1024), 0, s, e->row_out.ptr, rows,
                       e->metrics.ptr);
  }
  IRS_HIP(hipGetLastError());
}


void begin_accumulate(irs_evaluator *e, hipStream_t s) {
  e->metrics.alloc(1);
  e->metrics.zero(s);
  e->item_cnt.zero(s);
}

void finish_accumulate(irs_evaluator *e, irs_metrics *out, int64_t *item_cnt, hipStream_t s) {
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "");
  if (e->span_open) IRS_HIP(hipEventRecord(e->ev_last, s));
  IRS_HIP(hipMemcpyAsync(out, e->metrics.ptr, sizeof(irs_metrics), hipMemcpyDeviceToHost, s));
  IRS_HIP(hipMemcpyAsync(item_cnt, e->item_cnt.ptr, e->n_items * sizeof(int64_t),
                         hipMemcpyDeviceToHost, s));
  IRS_HIP(hipStreamSynchronize(s));
}

// ---- shared by the dense-similarity and factor-model calls (irs_eval_get_metrics_dense_similarity / _factors) ----

// Mask or exclusion rows checked on the host go up (nothing when nothing is stored): masked, model and serve calls
void upload_mask_rows(const MaskRows &rows, const int32_t *indices, DeviceBuffer<int64_t> &ptr, DeviceBuffer<int32_t> &idx,
                      hipStream_t s) {
  if (rows.nnz <= 0) return;
  ptr.upload(rows.ptr, s);
  idx.upload(indices, static_cast<size_t>(rows.nnz), s);
}

// The mask rows that arrive with an evaluator call.  `ptr.ptr` stays null when nothing is masked.
struct CallMask {
  DeviceBuffer<int64_t> ptr;
  DeviceBuffer<int32_t> idx;
  MaskRows host;
  void upload(const int64_t *mask_indptr, const int32_t *mask_indices, int64_t rows, int64_t n_items, bool check_columns,
              hipStream_t s) {
    host.take(mask_indptr, mask_indices, rows, n_items, check_columns);
    upload_mask_rows(host, mask_indices, ptr, idx, s);
  }
  // The similarity call: its usual caller masks with the rows it scores from (`X_train[u] @ W`, seen items removed)
  // and hands the same arrays over twice: the mask then aliases the profile rows `x` already on the device (80 MB
  // less over PCIe on the ML-20M shape).
  void upload_or_alias(const int64_t *mask_indptr, const int32_t *mask_indices, int64_t rows, int64_t n_items,
                       const ProfileRows &x, const int32_t *x_indices, const DeviceBuffer<int64_t> &d_xp,
                       const DeviceBuffer<int32_t> &d_xi, hipStream_t s) {
    host.take(mask_indptr, mask_indices, rows, n_items, false);
    if (host.nnz > 0 && mask_indices == x_indices + x.first && host.nnz == x.nnz && host.ptr == x.ptr) {
      ptr.borrow(d_xp);
      idx.borrow(d_xi);
    } else {
      upload_mask_rows(host, mask_indices, ptr, idx, s);
    }
  }
};

// Where the stream time of such a call went (irs_eval_last_phases): an event after every phase of every
// block, read after the call's last synchronisation.
enum Phase { PH_UPLOAD = 0, PH_SCORE = 1, PH_MASK = 2, PH_RANK = 3, PH_COUNT = 4 };
struct PhaseClock {
  std::vector<std::pair<hipEvent_t, int>> marks;  // (event, phase that ended there; -1: the start)
  hipStream_t s;
  explicit PhaseClock(hipStream_t stream) : s(stream) { mark(-1); }
  ~PhaseClock() {
    for (auto &m : marks) (void)hipEventDestroy(m.first);
  }
  void mark(int phase) {
    hipEvent_t ev = nullptr;
    IRS_HIP(hipEventCreate(&ev));
    marks.emplace_back(ev, phase);
    IRS_HIP(hipEventRecord(ev, s));
  }
  void read(double *ms) const {  // (after the stream was synchronised)
    std::fill(ms, ms + PH_COUNT, 0.0);
    for (size_t i = 1; i < marks.size(); i++) {
      float t = 0.0f;
      IRS_HIP(hipEventElapsedTime(&t, marks[i - 1].first, marks[i].first));
      ms[marks[i].second] += t;
    }
  }
};

// Per cutoff the running totals of a call's blocks, on the device: every block is ranked once per cutoff and its
// item counts added; one read-back after the last block.  The per-user terms reach the totals in one of two orders,
// each call keeping its own (the float64 sums differ in the last bits):
//   CHUNKS  dense-similarity and factor calls: the Evaluator's default host loop (HOST_LOOP_ROWS-row chunks in
//           sequence; the blocks of such a call are multiples of that, so the chunk boundaries are the loop's)
//   BLOCKS  similarity call: the block as one block call sums it, then Metrics::merge (evaluator.cpp:76-85) per block
struct CutoffTotals {
  enum Order { CHUNKS, BLOCKS } order;
  DeviceBuffer<irs_metrics> m;
  DeviceBuffer<unsigned long long> cnt;
  // `running` (CHUNKS only; one irs_metrics per cutoff, or null): the sums of the users before this call's - the
  // call's chunks are merged onto them, so a caller that hands its users over in several calls of whole chunks gets
  // the sums of one call (the item counts are integers and start from zero either way: the caller adds them)
  CutoffTotals(Order order_, int32_t n_cutoffs, int64_t ni, int64_t *item_cnt, hipStream_t s,
               const irs_metrics *running = nullptr)
      : order(order_) {
    std::fill(item_cnt, item_cnt + static_cast<int64_t>(std::max(n_cutoffs, 0)) * ni, int64_t(0));
    const size_t nc = static_cast<size_t>(std::max(n_cutoffs, 1));
    m.alloc(nc);
    cnt.alloc(nc * static_cast<size_t>(std::max<int64_t>(ni, 1)));
    m.zero(s);
    cnt.zero(s);
    if (running != nullptr && n_cutoffs > 0)
      IRS_HIP(hipMemcpyAsync(m.ptr, running, sizeof(irs_metrics) * static_cast<size_t>(n_cutoffs), hipMemcpyHostToDevice, s));
  }
  template <class T>
  void add_block(irs_evaluator *e, const T *scores, int64_t rows, int32_t n_cutoffs, const int64_t *cutoffs,
                 int64_t offset, bool rwc, hipStream_t s) {
    const int64_t ni = e->n_items;
    for (int32_t c = 0; c < n_cutoffs; c++) {
      begin_accumulate(e, s);
      if (order == CHUNKS) {
        rank_block<T>(e, scores, rows, cutoffs[c], offset, rwc, s, m.ptr + c);
      } else {
        rank_block<T>(e, scores, rows, cutoffs[c], offset, rwc, s);
        hipLaunchKernelGGL(metrics_fold_kernel, dim3(1), dim3(64), 0, s, static_cast<const irs_metrics *>(e->metrics.ptr),
                           m.ptr + c);
      }
      if (ni > 0)
        hipLaunchKernelGGL(counts_fold_kernel, dim3(static_cast<unsigned>(ceil_div(ni, 256))), dim3(256), 0, s,
                           static_cast<const unsigned long long *>(e->item_cnt.ptr), ni, cnt.ptr + static_cast<size_t>(c) * ni);
    }
    IRS_HIP(hipGetLastError());
  }
  void finish(irs_evaluator *e, int32_t n_cutoffs, irs_metrics *out, int64_t *item_cnt, hipStream_t s) {
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "");
    const int64_t ni = e->n_items;
    if (e->span_open) IRS_HIP(hipEventRecord(e->ev_last, s));
    if (n_cutoffs > 0) {
      IRS_HIP(hipMemcpyAsync(out, m.ptr, sizeof(irs_metrics) * static_cast<size_t>(n_cutoffs), hipMemcpyDeviceToHost, s));
      if (ni > 0)
        IRS_HIP(hipMemcpyAsync(item_cnt, cnt.ptr, sizeof(int64_t) * static_cast<size_t>(n_cutoffs) * ni,
                               hipMemcpyDeviceToHost, s));
    }
    IRS_HIP(hipStreamSynchronize(s));
  }
};

// a factor table [n, k] goes up, rows zero-padded to KP (what the MFMA tiles read); no memset when KP == k
void upload_padded(DeviceBuffer<float> &d, const float *host, int64_t n, int32_t k, int32_t KP, hipStream_t s) {
  const size_t count = static_cast<size_t>(std::max<int64_t>(n, 1)) * KP;
  d.alloc(count);
  if (KP != k || n <= 0) IRS_HIP(hipMemsetAsync(d.ptr, 0, count * sizeof(float), s));
  if (n > 0)
    IRS_HIP(hipMemcpy2DAsync(d.ptr, sizeof(float) * KP, host, sizeof(float) * k, sizeof(float) * k, static_cast<size_t>(n),
                             hipMemcpyHostToDevice, s));
}

// EvalParams of a ranking without ground truth (retrieve = 1): the `cutoff` best candidates of each row into rec_out
EvalParams retrieve_params(const void *scores, int64_t rows, int64_t n_items, int64_t offset, int64_t n_lists,
                           const int64_t *list_ptr, const int32_t *list_items, int64_t cutoff, RowOut *row_out,
                           int32_t *rec_out) {
  EvalParams p{};
  p.scores = scores;
  p.rows = rows;
  p.n_items = n_items;
  p.offset = offset;  // (per-row lists are numbered from the call's first row)
  p.rec_mode = rec_mode_of(n_lists);
  p.rec_ptr = list_ptr;
  p.rec_items = list_items;
  p.cutoff = static_cast<int32_t>(cutoff);
  p.retrieve = 1;
  p.out = row_out;
  p.rec_out = rec_out;
  return p;
}

// The switches of the fused call, on unless set to 0 (read per call: tests toggle them):
//   IRSPACK_AMD_EVAL_EMIT          the threshold-filtered path (off: A/B against the two-pass one)
//   IRSPACK_AMD_EVAL_BOUND         its norm-bound pruning (off: the emit path scores every tile)
//   IRSPACK_AMD_EVAL_SAMPLE_FUSED  its sample pass in one launch (off: three launches per 32,768 users, round 5)
bool env_on(const char *name) {
  const char *e = std::getenv(name);
  return e ? std::atoi(e) != 0 : true;
}
EnvInt env_int(const char *name) {
  const char *v = std::getenv(name);
  return EnvInt{v != nullptr, v ? std::atoll(v) : 0};
}

int device_cu_count(int device) {
  static std::atomic<int> cached[64] = {};
  const int slot = device >= 0 && device < 64 ? device : 0;
  int n = cached[slot].load(std::memory_order_relaxed);
  if (n <= 0) {
    IRS_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device));
    n = std::max(n, 1);
    cached[slot].store(n, std::memory_order_relaxed);
  }
  return n;
}

// Builds (or reuses) the bitmap + per-row count of the mask CSR; false when it would not fit.
bool ensure_mask_bitmap(irs_evaluator *e, int64_t rows, int64_t words, const int64_t *d_mptr,
                        const int32_t *d_midx, hipStream_t s, bool cacheable) {
  if (!mask_bitmap_fits(rows, words)) return false;
  const bool cached = cacheable && d_mptr == e->mask_ptr.ptr && e->mask_bits_rows == rows;
  if (!cached) {
    e->mask_bits.alloc(static_cast<size_t>(rows) * words);
    e->mask_count.alloc(rows);
    IRS_HIP(hipMemsetAsync(e->mask_bits.ptr, 0, static_cast<size_t>(rows) * words * 8, s));
    hipLaunchKernelGGL(mask_bitmap_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, s, d_mptr, d_midx,
                       rows, words, e->mask_bits.ptr);
    hipLaunchKernelGGL(mask_count_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, s, e->mask_bits.ptr,
                       rows, words, e->mask_count.ptr);
    // row ids per entry + the row pointers on the host (entry ranges of the sample blocks)
    e->mask_ptr_host.resize(rows + 1);
    IRS_HIP(hipMemcpyAsync(e->mask_ptr_host.data(), d_mptr, (rows + 1) * sizeof(int64_t),
                           hipMemcpyDeviceToHost, s));
    IRS_HIP(hipStreamSynchronize(s));
    e->mask_row.alloc(static_cast<size_t>(std::max<int64_t>(e->mask_ptr_host[rows], 1)));
    hipLaunchKernelGGL(mask_row_ids_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, s, d_mptr, rows,
                       e->mask_row.ptr);
    // only the resident mask, covered by ONE pass, is cached
    e->mask_bits_rows = (cacheable && d_mptr == e->mask_ptr.ptr) ? rows : -1;
  }
  return true;
}

// ---- The threshold-filtered path of irs_eval_get_metrics_ials (eval_fused_kernels.hpp, second half). ----
// One pass of it over the users [begin, begin + rows): what the stages below share.  `plan` (eval_emit_plan.hpp)
// holds every decision; the stages launch, in this order, on the one stream.
struct EmitPass {
  irs_evaluator *e;
  irs_ials_trainer *t;
  hipStream_t s;
  EmitPlan plan;
  const float *user, *item;  // the trainer's factor tables, [*, KP]
  int32_t KP, dev;
  int64_t ni;
  int64_t begin, rows, cutoff, offset;
  bool rwc, first;           // first: the first pass of a call prepares the item side
  const int64_t *d_mptr;     // mask CSR of the pass's rows, or null
  const int32_t *d_midx;
  float norm_c;              // rounding allowance of the norms
};
// e->bad_flag: [0] flags, [1] hard rows at the end, [2] hard rows after the sample pass, [3] workgroups
// ([4..5]: the scored-tile count, 64 bits - one block, so that the call's single read-back is ONE copy, into
// page-locked memory: two pageable copies and their staging cost ~50 us of a 1.2 ms call)
enum { FLAG_BAD = 0, FLAG_HARD = 1, FLAG_HARD_SAMPLE = 2, FLAG_WG = 3, FLAG_TILES = 4, FLAG_WORDS = 8 };

void scores_prefix(const EmitPass &c, int64_t r0, int64_t r1, int64_t n_prefix, const float *item_rows,
                   const float *user_rows, float *out) {
  if (irs_ials_scores_prefix_device_(c.t, r0, r1, n_prefix, item_rows, user_rows, out) != IRS_OK)
    throw std::runtime_error(irs_last_error());
}

// 1. item side (bounded variant): items in order of decreasing norm - the sample is then the items of largest
//    norm, which hold most of every user's final list.  iota covers the items' sort and this pass's users'.
void emit_item_side(const EmitPass &c) {
  irs_evaluator *e = c.e;
  const int64_t ni = c.ni, n_iota = std::max(ni, c.rows);
  e->iota.alloc(n_iota);
  hipLaunchKernelGGL(iota_kernel, dim3(ceil_div(n_iota, 256)), dim3(256), 0, c.s, e->iota.ptr, n_iota);
  if (!c.first) return;  // (the item side is ready)
  e->inorm.alloc(ni);
  e->inorm_sorted.alloc(ni);
  e->iperm.alloc(ni);
  e->iinv.alloc(ni);
  hipLaunchKernelGGL(row_norm_up_kernel, dim3(ceil_div(ni, 16)), dim3(256), 0, c.s, c.item, int64_t(0),
                     ni, c.KP, c.norm_c, e->inorm.ptr, e->bad_flag.ptr);
  sort_pairs_f32(true, e->inorm.ptr, e->inorm_sorted.ptr, e->iota.ptr, e->iperm.ptr, ni, e->sort_tmp, c.s);
  hipLaunchKernelGGL(inverse_perm_kernel, dim3(ceil_div(ni, 256)), dim3(256), 0, c.s, e->iperm.ptr, ni,
                     e->iinv.ptr);
  e->sample_item.alloc(static_cast<size_t>(EM_SAMPLE2) * c.KP);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(ceil_div(int64_t(EM_SAMPLE2) * (c.KP / 4), 256)), dim3(256),
                     0, c.s, c.item, e->iperm.ptr, static_cast<int64_t>(EM_SAMPLE2), c.KP,
                     e->sample_item.ptr, static_cast<const int32_t *>(nullptr));
}

// 2. sample pass: thresholds from the first n_sample items - in one launch, or in blocks of users
void emit_sample_tau(const EmitPass &c) {
  irs_evaluator *e = c.e;
  const EmitPlan &pl = c.plan;
  const int64_t rows = c.rows, n_sample = pl.n_sample;
  e->tau.alloc(rows);
  e->fused_scores.alloc(std::max(static_cast<size_t>(std::min(pl.sample_block, rows)) * n_sample,
                                 static_cast<size_t>(pl.hcap) * EM_SAMPLE2));
  if (pl.fused_sample) {
    SampleParams sp{};
    sp.user = c.user;
    sp.sample = e->sample_item.ptr;
    sp.begin = c.begin;
    sp.rows = rows;
    sp.mask_ptr = c.d_mptr;
    sp.mask_idx = c.d_midx;
    sp.iinv = e->iinv.ptr;
    sp.cutoff = static_cast<int32_t>(c.cutoff);
    sp.tau = e->tau.ptr;
    sp.hard = e->hard.ptr;
    sp.bad_flag = e->bad_flag.ptr;
    auto launch = [&](auto kernel) {
      IRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(SF_LDS_BYTES)));
      const int64_t grid = sample_fused_grid(rows, pl.sample_per_cu, device_cu_count(c.dev));
      hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(grid)), dim3(512), SF_LDS_BYTES, c.s, sp);
    };
    switch (c.KP) {
      case 16: launch(sample_tau_fused_kernel<16>); break;
      case 32: launch(sample_tau_fused_kernel<32>); break;
      case 64: launch(sample_tau_fused_kernel<64>); break;
      default: launch(sample_tau_fused_kernel<128>); break;
    }
    return;
  }
  const int32_t *no_list = nullptr;
  for (int64_t b = 0; b < rows; b += pl.sample_block) {
    const int64_t m = std::min(pl.sample_block, rows - b);
    scores_prefix(c, c.begin + b, c.begin + b + m, n_sample, pl.bounded ? e->sample_item.ptr : nullptr, nullptr,
                  e->fused_scores.ptr);
    if (c.d_mptr && pl.bounded) {
      const int64_t q0 = e->mask_ptr_host[b], q1 = e->mask_ptr_host[b + m];
      if (q1 > q0)
        hipLaunchKernelGGL(mask_entries_perm_kernel, dim3(ceil_div(q1 - q0, 256)), dim3(256), 0, c.s,
                           e->fused_scores.ptr, n_sample, b, q0, q1, e->mask_row.ptr, c.d_midx,
                           e->iinv.ptr);
    } else if (c.d_mptr)
      hipLaunchKernelGGL(mask_rows_kernel, dim3(m), dim3(64), 0, c.s, e->fused_scores.ptr, m,
                         n_sample, c.d_mptr + b, c.d_midx);
    hipLaunchKernelGGL((sample_tau_kernel<8>), dim3(static_cast<unsigned>(ceil_div(m, 4))), dim3(256),
                       0, c.s, e->fused_scores.ptr, m, n_sample,
                       static_cast<int32_t>(c.cutoff), e->tau.ptr + b, e->bad_flag.ptr,
                       e->hard.ptr + b, no_list, no_list);
  }
}

// 3. second chance: up to hcap hard rows against the EM_SAMPLE2 items of largest norm (no host round trip: the
//    kernels run on hcap rows and stop at the device-side count)
void emit_second_chance(const EmitPass &c) {
  irs_evaluator *e = c.e;
  const int64_t HCAP = c.plan.hcap;
  const int32_t *n_hard1 = e->bad_flag.ptr + FLAG_HARD_SAMPLE;
  hipLaunchKernelGGL(collect_hard_kernel, dim3(ceil_div(c.rows, 256)), dim3(256), 0, c.s, e->hard.ptr,
                     e->gt_ptr.ptr, c.offset, c.rows, e->hard_list.ptr, e->bad_flag.ptr + FLAG_HARD_SAMPLE,
                     static_cast<int32_t>(HCAP));
  e->hard_user.alloc(static_cast<size_t>(HCAP) * c.KP);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(ceil_div(HCAP * (c.KP / 4), 256)), dim3(256), 0, c.s,
                     c.user + c.begin * c.KP, e->hard_list.ptr, HCAP, c.KP, e->hard_user.ptr, n_hard1);
  scores_prefix(c, 0, HCAP, EM_SAMPLE2, e->sample_item.ptr, e->hard_user.ptr, e->fused_scores.ptr);
  const int32_t *list = e->hard_list.ptr;
  if (c.d_mptr)
    hipLaunchKernelGGL(mask_rows_perm_kernel, dim3(HCAP), dim3(64), 0, c.s, e->fused_scores.ptr, HCAP,
                       static_cast<int64_t>(EM_SAMPLE2), c.d_mptr, c.d_midx, e->iinv.ptr, list, n_hard1);
  hipLaunchKernelGGL((sample_tau_kernel<8>), dim3(static_cast<unsigned>(ceil_div(HCAP, 4))), dim3(256),
                     0, c.s, e->fused_scores.ptr, HCAP, static_cast<int64_t>(EM_SAMPLE2),
                     static_cast<int32_t>(c.cutoff), e->tau.ptr, e->bad_flag.ptr, e->hard.ptr, list, n_hard1);
}

// 4. (bounded variant) users in order of increasing pruning radius, what each 64-user tile still needs, and the
//    work list: only workgroups with a live tile are launched (the others would still queue for a workgroup slot
//    and its LDS just to leave).  Returns the grid of score_emit_kernel.
int32_t emit_work_list(const EmitPass &c, EmitParams &f) {
  irs_evaluator *e = c.e;
  const EmitPlan &pl = c.plan;
  const int64_t rows = c.rows, n_ut = pl.n_ut;
  unsigned long long *const tiles_scored_dev = reinterpret_cast<unsigned long long *>(e->bad_flag.ptr + FLAG_TILES);
  e->unorm.alloc(rows);
  e->radius.alloc(rows);
  e->radius_sorted.alloc(rows);
  e->uperm.alloc(rows);
  e->limit_tiles.alloc(n_ut);
  hipLaunchKernelGGL(row_norm_up_kernel, dim3(ceil_div(rows, 16)), dim3(256), 0, c.s, c.user, c.begin, rows,
                     c.KP, c.norm_c, e->unorm.ptr, e->bad_flag.ptr);
  hipLaunchKernelGGL(prune_radius_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, c.s, e->tau.ptr,
                     e->unorm.ptr, e->gt_ptr.ptr, c.offset, rows, e->hard.ptr, e->radius.ptr);
  sort_pairs_f32(false, e->radius.ptr, e->radius_sorted.ptr, e->iota.ptr, e->uperm.ptr, rows, e->sort_tmp, c.s);
  hipLaunchKernelGGL(tile_limit_kernel, dim3(ceil_div(n_ut, 256)), dim3(256), 0, c.s,
                     e->radius_sorted.ptr, rows, e->inorm_sorted.ptr, c.ni, e->limit_tiles.ptr,
                     tiles_scored_dev);
  f.iperm = e->iperm.ptr;
  f.uperm = e->uperm.ptr;
  f.limit_tiles = e->limit_tiles.ptr;
  e->wg_prefix.alloc(n_ut + 1);
  hipLaunchKernelGGL(wg_scan_kernel, dim3(1), dim3(1024), 0, c.s, e->limit_tiles.ptr, n_ut,
                     e->wg_prefix.ptr, e->bad_flag.ptr + FLAG_WG);
  int32_t n_wg = 0;
  if (pl.wg_len_on_device) {
    n_wg = pl.wg_grid;
    e->wg_desc.alloc(std::max<int64_t>(pl.wg_bound, 1));
    f.n_wg = e->bad_flag.ptr + FLAG_WG;
  } else {  // the length comes back first
    IRS_HIP(hipMemcpyAsync(&n_wg, e->bad_flag.ptr + FLAG_WG, sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    IRS_HIP(hipStreamSynchronize(c.s));
    e->wg_desc.alloc(std::max<int64_t>(n_wg, 1));
  }
  hipLaunchKernelGGL(wg_fill_kernel, dim3(ceil_div(n_ut, 4)), dim3(256), 0, c.s, e->wg_prefix.ptr,
                     e->limit_tiles.ptr, n_ut, e->wg_desc.ptr);
  f.wg_desc = e->wg_desc.ptr;
  return n_wg;
}

// 5. the whole score matrix, candidates only: `tiles` 64 x 64 tiles, four per workgroup
void emit_scores(const EmitPass &c, const EmitParams &f, int64_t tiles) {
  const size_t lds = 4 * 64 * FZ_SROW * sizeof(float) + 4 * 64 * sizeof(int32_t);
  auto launch = [&](auto kernel) {
    IRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(ceil_div(tiles, 4))), dim3(256), lds, c.s, f);
  };
#define IRS_EMIT_CASE(KK)                                        \
  case KK:                                                       \
    if (c.plan.bounded) launch(score_emit_kernel<KK, true>);     \
    else launch(score_emit_kernel<KK, false>);                   \
    break;
  switch (c.KP) {  // (emit_width_ok: one of these)
    IRS_EMIT_CASE(16)
    IRS_EMIT_CASE(32)
    IRS_EMIT_CASE(64)
    IRS_EMIT_CASE(128)
    IRS_EMIT_CASE(192)
    IRS_EMIT_CASE(256)
    default: break;
  }
#undef IRS_EMIT_CASE
}

// 6. rank the candidates, metrics; the rows left hard are listed and counted
EvalParams emit_rank_candidates(const EmitPass &c, const EmitParams &f, const int32_t *n_masked) {
  irs_evaluator *e = c.e;
  EvalParams p = metric_params(e, nullptr, c.rows, c.cutoff, c.offset, c.rwc);
  p.todo = e->todo.ptr;
  const dim3 grid(static_cast<unsigned>(ceil_div(c.rows, 4)));
  hipLaunchKernelGGL((rank_cand_kernel<8>), grid, dim3(256), 0, c.s, p, f, n_masked);
  hipLaunchKernelGGL(rank_cand_slow_kernel, grid, dim3(256), 0, c.s, p, f, n_masked);
  hipLaunchKernelGGL(collect_hard_kernel, dim3(ceil_div(c.rows, 256)), dim3(256), 0, c.s, e->hard.ptr,
                     e->gt_ptr.ptr, c.offset, c.rows, e->hard_list.ptr, e->bad_flag.ptr + FLAG_HARD,
                     static_cast<int32_t>(c.rows));
  IRS_HIP(hipGetLastError());
  return p;
}

// 7. the hard rows from their full score rows, in chunks: gather the user factors -> scores -> mask -> the general
//    ranking (no `todo` scratch; why: emit_abandon), all through the row list
void emit_hard_rows(const EmitPass &c, const EvalParams &p, int64_t n_hard) {
  irs_evaluator *e = c.e;
  const int64_t ni = c.ni, chunk = hard_row_chunk(n_hard, ni);
  e->hard_user.alloc(static_cast<size_t>(chunk) * c.KP);
  e->fused_scores.alloc(static_cast<size_t>(chunk) * ni);
  for (int64_t b = 0; b < n_hard; b += chunk) {
    const int64_t m = std::min(chunk, n_hard - b);
    const int32_t *list = e->hard_list.ptr + b;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(ceil_div(m * (c.KP / 4), 256)), dim3(256), 0, c.s,
                       c.user + c.begin * c.KP, list, m, c.KP, e->hard_user.ptr,
                       static_cast<const int32_t *>(nullptr));
    scores_prefix(c, 0, m, ni, nullptr, e->hard_user.ptr, e->fused_scores.ptr);
    if (c.d_mptr)
      hipLaunchKernelGGL(mask_rows_kernel, dim3(m), dim3(256), 0, c.s, e->fused_scores.ptr, m, ni, c.d_mptr,
                         c.d_midx, list);
    EvalParams q = p;
    q.scores = e->fused_scores.ptr;
    q.rows = m;
    q.row_map = list;
    launch_rank<float>(q, ni, c.s, nullptr);
  }
  IRS_HIP(hipGetLastError());
}

// 8. item histogram of the lists, sum of the per-user terms (one level, or chunks and then the chunks in order)
void emit_hist_reduce(const EmitPass &c) {
  irs_evaluator *e = c.e;
  const int64_t rows = c.rows;
  launch_item_hist(e->rec_out.ptr, rows * c.cutoff, e->item_cnt.ptr, c.s, e->n_items);
  if (c.plan.two_level) {
    const int64_t chunk = c.plan.reduce_chunk;
    const int nb = static_cast<int>(ceil_div(rows, chunk));
    e->row_partials.alloc(nb);
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(nb), dim3(1024), 0, c.s, e->row_out.ptr, rows,
                       e->metrics.ptr, e->row_partials.ptr, chunk);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(64), 0, c.s, e->row_partials.ptr, nb, rows,
                       e->metrics.ptr);
  } else {
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(1024), 0, c.s, e->row_out.ptr, rows,
                       e->metrics.ptr, static_cast<RowPartial *>(nullptr), int64_t(0));
  }
  IRS_HIP(hipGetLastError());
}

// One pass.  Returns false when the call is outside the path's domain or had to be abandoned; the caller then
// runs the two-pass path.  `single` = the only pass of the call (the mask bitmap of a resident mask may then be
// kept for the next call).
bool emit_block(irs_evaluator *e, irs_ials_trainer *t, int64_t begin, int64_t rows,
                const int64_t *d_mptr, const int32_t *d_midx, int64_t cutoff, int64_t offset,
                bool rwc, hipStream_t s, bool first, bool single) {
  EmitFacts facts{env_on("IRSPACK_AMD_EVAL_EMIT"), env_on("IRSPACK_AMD_EVAL_BOUND"),
                  env_on("IRSPACK_AMD_EVAL_SAMPLE_FUSED"), env_int("IRSPACK_AMD_EVAL_SAMPLE"),
                  e->rec_mode, cutoff, rows, 0, 0, e->n_items};
  if (!emit_call_in_domain(facts)) return false;
  EmitPass c{e, t, s, EmitPlan{}, nullptr, nullptr, 0, 0, 0, begin, rows, cutoff, offset, rwc, first, d_mptr, d_midx, 0.0f};
  int64_t nu = 0;
  void *sv = nullptr;
  if (irs_ials_factors_device_(t, &c.user, &c.item, &c.KP, &nu, &c.ni, &sv, &c.dev) != IRS_OK)
    throw std::runtime_error(irs_last_error());
  facts.KP = c.KP;
  facts.ni = c.ni;
  const EmitPlan &pl = c.plan = plan_emit_pass(facts);
  if (!pl.ok) return false;
  c.norm_c = 1.0f + (c.KP + 16) * 2.5e-7f;
  const uint64_t *bits = nullptr;
  const int32_t *n_masked = nullptr;
  if (d_mptr) {
    if (!ensure_mask_bitmap(e, rows, pl.words, d_mptr, d_midx, s, single)) return false;
    bits = e->mask_bits.ptr;
    n_masked = e->mask_count.ptr;
  }
  e->bad_flag.alloc(FLAG_WORDS);
  IRS_HIP(hipMemsetAsync(e->bad_flag.ptr, 0, FLAG_WORDS * sizeof(int32_t), s));
  if (!e->flags_host)
    IRS_HIP(hipHostMalloc(reinterpret_cast<void **>(&e->flags_host), FLAG_WORDS * sizeof(int32_t), hipHostMallocDefault));
  e->hard.alloc(rows);
  e->hard_list.alloc(rows);
  IRS_HIP(hipMemsetAsync(e->hard.ptr, 0, rows * sizeof(int32_t), s));
  if (pl.bounded) emit_item_side(c);
  emit_sample_tau(c);
  if (pl.second_chance) emit_second_chance(c);
  e->cand_score.alloc(static_cast<size_t>(rows) * EM_CAP);
  e->cand_item.alloc(static_cast<size_t>(rows) * EM_CAP);
  e->cand_cnt.alloc(rows);
  IRS_HIP(hipMemsetAsync(e->cand_cnt.ptr, 0, rows * sizeof(int32_t), s));
  EmitParams f{};
  f.user = c.user;
  f.item = c.item;
  f.begin = begin;
  f.rows = rows;
  f.n_items = c.ni;
  f.mask_bits = bits;
  f.words = pl.words;
  f.tau = e->tau.ptr;
  f.cand_score = e->cand_score.ptr;
  f.cand_item = e->cand_item.ptr;
  f.cand_cnt = e->cand_cnt.ptr;
  f.bad_flag = e->bad_flag.ptr;
  f.hard = e->hard.ptr;
  const int64_t tiles = pl.bounded ? int64_t(emit_work_list(c, f)) * 4 : pl.tiles_total;
  if (tiles > 0) emit_scores(c, f, tiles);
  const EvalParams p = emit_rank_candidates(c, f, n_masked);
  IRS_HIP(hipMemcpyAsync(e->flags_host, e->bad_flag.ptr, FLAG_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  IRS_HIP(hipStreamSynchronize(s));
  const int32_t flags = e->flags_host[FLAG_BAD], n_hard = e->flags_host[FLAG_HARD];
  unsigned long long tiles_scored = 0;
  std::memcpy(&tiles_scored, e->flags_host + FLAG_TILES, sizeof(tiles_scored));
  if (first) e->stats = irs_eval_stats{pl.bounded ? 2 : 1, 0, 0, 0, pl.n_sample};
  e->stats.hard_rows += n_hard;
  e->stats.tiles_total += pl.tiles_total;
  e->stats.tiles_scored += pl.bounded ? static_cast<int64_t>(tiles_scored) : pl.tiles_total;
  if (emit_abandon(flags, n_hard)) return false;
  if (n_hard > 0) emit_hard_rows(c, p, n_hard);
  emit_hist_reduce(c);
  return true;
}

// The threshold-filtered path over all users of a call, in passes that keep the scratch bounded
// (emit_pass_rows; IRSPACK_AMD_EVAL_PASS_ROWS overrides the pass size).  False: outside the
// path's domain or abandoned - the caller resets the sums and runs the two-pass path.
bool emit_path(irs_evaluator *e, irs_ials_trainer *t, int64_t begin, int64_t rows,
               const int64_t *d_mptr, const int32_t *d_midx, int64_t cutoff, int64_t offset,
               bool rwc, hipStream_t s) {
  if (rows <= 0) return false;
  const int64_t pass = emit_pass_rows(e->n_items, env_int("IRSPACK_AMD_EVAL_PASS_ROWS"));
  if (pass == 0) return false;
  if (rows <= pass) return emit_block(e, t, begin, rows, d_mptr, d_midx, cutoff, offset, rwc, s, true, true);
  for (int64_t b = 0; b < rows; b += pass) {
    const int64_t m = std::min(pass, rows - b);
    if (!emit_block(e, t, begin + b, m, d_mptr ? d_mptr + b : nullptr, d_midx, cutoff, offset + b, rwc,
                    s, b == 0, false))
      return false;
  }
  return true;
}

}  // namespace

extern "C" {

irs_status irs_eval_create(int64_t n_users, int64_t n_items, const int64_t *indptr,
                           const int32_t *indices, int64_t n_lists, const int64_t *rec_ptr,
                           const int64_t *rec_items, int32_t device, irs_evaluator **out) {
  return guard([&] {
    check_arg(out && indptr, "null argument.");
    check_arg(n_users >= 0 && n_items >= 0, "negative shape.");
    // evaluator.cpp:187-190
    check_arg(n_lists == 0 || n_lists == 1 || n_lists == n_users,
              "recommendable.size.() must be in {0, 1, ground_truth.size()}");
    const int64_t nnz = indptr[n_users];
    check_arg(nnz < (int64_t(1) << 31), "nnz must be below 2^31.");
    // sort + validate the recommendable lists (:193-205)
    std::vector<std::vector<int32_t>> lists(n_lists);
    for (int64_t l = 0; l < n_lists; l++) {
      auto &v = lists[l];
      for (int64_t q = rec_ptr[l]; q < rec_ptr[l + 1]; q++) {
        check_arg(rec_items[q] >= 0 && rec_items[q] < n_items,
                  "recommendable items contain a index >= n_items.");
        v.push_back(static_cast<int32_t>(rec_items[q]));
      }
      std::sort(v.begin(), v.end());
      for (size_t i = 1; i < v.size(); i++)
        check_arg(v[i] > v[i - 1], "duplicate recommendable items.");
    }
    // ground truth restricted to the recommendable set (cache_X_map, :208-254)
    std::vector<int32_t> gptr(n_users + 1, 0), gidx;
    gidx.reserve(nnz);
    for (int64_t u = 0; u < n_users; u++) {
      std::vector<int32_t> row(indices + indptr[u], indices + indptr[u + 1]);
      std::sort(row.begin(), row.end());
      row.erase(std::unique(row.begin(), row.end()), row.end());
      for (auto c : row) check_arg(c >= 0 && c < n_items, "column index out of range.");
      if (n_lists == 0) {
        gidx.insert(gidx.end(), row.begin(), row.end());
      } else {
        const auto &rec = n_lists == 1 ? lists[0] : lists[u];
        std::set_intersection(row.begin(), row.end(), rec.begin(), rec.end(),
                              std::back_inserter(gidx));
      }
      gptr[u + 1] = static_cast<int32_t>(gidx.size());
    }
    require_device(device);
    auto e = std::make_unique<irs_evaluator>();
    e->device = device;
    e->n_users = n_users;
    e->n_items = n_items;
    e->rec_mode = rec_mode_of(n_lists);
    hipStream_t s = nullptr;
    e->gt_ptr.upload(gptr, s);
    e->gt_idx.upload(gidx, s);
    std::vector<int64_t> rp(n_lists + 1, 0);
    std::vector<int32_t> ri;
    for (int64_t l = 0; l < n_lists; l++) {
      ri.insert(ri.end(), lists[l].begin(), lists[l].end());
      rp[l + 1] = static_cast<int64_t>(ri.size());
    }
    e->rec_ptr.upload(rp, s);
    e->rec_items.upload(ri, s);
    // prepare_dcg_discount (:42-48) and its sequential prefix sums (std::accumulate, :137-139)
    const int64_t nd = std::max<int64_t>(n_items, 1);  // any cutoff up to n_items (:263-268)
    std::vector<double> disc(nd), pre(nd + 1, 0.0);
    for (int64_t i = 0; i < nd; i++) disc[i] = 1 / std::log2(2 + i);
    for (int64_t i = 0; i < nd; i++) pre[i + 1] = pre[i] + disc[i];
    e->disc.upload(disc, s);
    e->idcg_prefix.upload(pre, s);
    e->item_cnt.alloc(std::max<int64_t>(n_items, 1));
    e->metrics.alloc(1);
    IRS_HIP(hipStreamSynchronize(s));
    *out = e.release();
  });
}

irs_status irs_eval_last_stats(irs_evaluator *e, irs_eval_stats *out) {
  return guard([&] {
    check_arg(e && out, "null argument.");
    *out = e->stats;
  });
}

irs_status irs_eval_destroy(irs_evaluator *e) {
  return guard([&] {
    if (e) {
      (void)hipSetDevice(e->device);
      if (e->ev_first) (void)hipEventDestroy(e->ev_first);
      if (e->ev_last) (void)hipEventDestroy(e->ev_last);
      if (e->flags_host) (void)hipHostFree(e->flags_host);
      delete e;
    }
  });
}

irs_status irs_eval_get_metrics(irs_evaluator *e, int32_t is_f64, const void *scores,
                                int64_t rows, int64_t cutoff, int64_t offset,
                                int64_t n_threads, int32_t recall_with_cutoff,
                                irs_metrics *out, int64_t *item_cnt) {
  return guard([&] {
    check_arg(e && out && item_cnt, "null argument.");
    check_arg(rows >= 0, "negative row count.");
    validate_call(e, rows, cutoff, offset, n_threads);
    IRS_HIP(hipSetDevice(e->device));
    hipStream_t s = nullptr;
    begin_accumulate(e, s);
    if (rows > 0) {
      const size_t bytes = static_cast<size_t>(rows) * e->n_items * (is_f64 ? 8 : 4);
      e->score_buf.alloc(bytes);
      IRS_HIP(hipMemcpyAsync(e->score_buf.ptr, scores, bytes, hipMemcpyHostToDevice, s));
      if (is_f64)
        rank_block<double>(e, e->score_buf.ptr, rows, cutoff, offset, recall_with_cutoff != 0, s);
      else
        rank_block<float>(e, e->score_buf.ptr, rows, cutoff, offset, recall_with_cutoff != 0, s);
    }
    finish_accumulate(e, out, item_cnt, s);
  });
}

irs_status irs_eval_get_metrics_masked(irs_evaluator *e, int32_t is_f64, const void *scores,
                                       int64_t rows, const int64_t *mask_indptr,
                                       const int32_t *mask_indices, int32_t n_cutoffs,
                                       const int64_t *cutoffs, int64_t offset,
                                       int64_t n_threads, int32_t recall_with_cutoff,
                                       irs_metrics *out, int64_t *item_cnt) {
  return guard([&] {
    check_arg(e && out && item_cnt && cutoffs, "null argument.");
    check_arg(rows >= 0 && n_cutoffs >= 0, "negative count.");
    check_arg(rows == 0 || scores != nullptr, "null score block.");
    for (int32_t c = 0; c < n_cutoffs; c++) validate_call(e, rows, cutoffs[c], offset, n_threads);
    IRS_HIP(hipSetDevice(e->device));
    hipStream_t s = nullptr;
    CallMask mask;
    if (rows > 0) {
      const size_t bytes = static_cast<size_t>(rows) * e->n_items * (is_f64 ? 8 : 4);
      e->score_buf.alloc(bytes);
      IRS_HIP(hipMemcpyAsync(e->score_buf.ptr, scores, bytes, hipMemcpyHostToDevice, s));
      mask.upload(mask_indptr, mask_indices, rows, e->n_items, false, s);  // (stray columns: the kernel skips them)
      if (mask.ptr.ptr) {
        if (is_f64)
          hipLaunchKernelGGL(mask_block_kernel<double>, dim3(static_cast<unsigned>(rows)), dim3(64), 0, s,
                             reinterpret_cast<double *>(e->score_buf.ptr), rows, e->n_items, mask.ptr.ptr,
                             mask.idx.ptr);
        else
          hipLaunchKernelGGL(mask_block_kernel<float>, dim3(static_cast<unsigned>(rows)), dim3(64), 0, s,
                             reinterpret_cast<float *>(e->score_buf.ptr), rows, e->n_items, mask.ptr.ptr,
                             mask.idx.ptr);
        IRS_HIP(hipGetLastError());
      }
    }
    for (int32_t c = 0; c < n_cutoffs; c++) {
      begin_accumulate(e, s);
      if (rows > 0) {
        if (is_f64)
          rank_block<double>(e, e->score_buf.ptr, rows, cutoffs[c], offset, recall_with_cutoff != 0, s);
        else
          rank_block<float>(e, e->score_buf.ptr, rows, cutoffs[c], offset, recall_with_cutoff != 0, s);
      }
      finish_accumulate(e, out + c, item_cnt + static_cast<int64_t>(c) * e->n_items, s);
    }
  });
}

}  // extern "C"
namespace {
// ---- the score launches the similarity calls and the serve calls share (they stand between the entry points so
// that the score kernels' instances keep the place in the code object that their first use, below, gives them) ----

// profile rows on the device: rebased pointers, columns, values (null: all 1.0; the dense kernel always reads them)
struct ProfileView { const int64_t *ptr; const int32_t *idx; const double *val; };
// a sparse W by rows on the device; `tptr` (null: the rows are not in column order): per (row, tile of SIM_TILE
// columns) the first entry inside the tile, from build_tile_table
struct SparseWeightsView {
  const int64_t *ptr; const int32_t *idx; const double *val;
  int64_t nnz; int32_t n_tiles; const int32_t *tptr;
};

inline int32_t sim_tiles(int64_t ni) { return static_cast<int32_t>(ceil_div(std::max<int64_t>(ni, 1), SIM_TILE)); }

void build_tile_table(DeviceBuffer<int32_t> &tptr, const DeviceBuffer<int64_t> &w_ptr, const DeviceBuffer<int32_t> &w_idx,
                      int64_t n_rows, int32_t n_tiles, hipStream_t s) {
  const int64_t n_tp = n_rows * (n_tiles + 1);
  tptr.alloc(static_cast<size_t>(n_tp));
  hipLaunchKernelGGL(sim_tile_ptr_kernel, dim3(static_cast<unsigned>(ceil_div(n_tp, 256))), dim3(256), 0, s,
                     static_cast<const int64_t *>(w_ptr.ptr), static_cast<const int32_t *>(w_idx.ptr), n_rows, n_tiles,
                     tptr.ptr);
  IRS_HIP(hipGetLastError());
}

// scores of the rows row0 .. row0 + m of `x` (launched in `order`, relative to row0) into out [m, ni]
// (`ni`: the columns scored = W's width; `ld` >= ni: the row stride of `out`, 0 = ni)
void launch_sim_scores(const ProfileView &x, const SparseWeightsView &w, int64_t row0, int64_t m, int64_t ni, double *out,
                       const int32_t *order, hipStream_t s, int64_t ld = 0) {
  hipLaunchKernelGGL(w.tptr ? sim_score_kernel<true> : sim_score_kernel<false>, dim3(static_cast<unsigned>(m * w.n_tiles)),
                     dim3(64), 0, s, x.ptr, x.idx, x.val, w.ptr, w.idx, w.val, std::max<int64_t>(w.nnz - 1, 0), row0, ni,
                     w.n_tiles, out, w.tptr, order, ld > 0 ? ld : ni);
}
void launch_dense_scores(const ProfileView &x, const void *w, bool w_is_f64, int64_t row0, int64_t m, int64_t ni,
                         double *out, const int32_t *order, hipStream_t s, int64_t ld = 0) {
  if (ld <= 0) ld = ni;
  const dim3 grid(static_cast<unsigned>(m * ceil_div(std::max<int64_t>(ni, 1), DS_STRIP)));
  if (w_is_f64)
    hipLaunchKernelGGL(dense_sim_score_kernel<double>, grid, dim3(64), 0, s, x.ptr, x.idx, x.val,
                       static_cast<const double *>(w), row0, m, ni, out, order, ld);
  else
    hipLaunchKernelGGL(dense_sim_score_kernel<float>, grid, dim3(64), 0, s, x.ptr, x.idx, x.val,
                       static_cast<const float *>(w), row0, m, ni, out, order, ld);
}

// the columns [ns, ni) of a block that a model call does not score (the *_scored entries with n_scored < n_items)
template <class T> void fill_unscored(T *scores, int64_t m, int64_t ni, int64_t ns, hipStream_t s) {
  if (ns >= ni || m <= 0) return;
  hipLaunchKernelGGL(fill_unscored_kernel<T>, dim3(static_cast<unsigned>(m)), dim3(64), 0, s, scores, m, ni, ns);
}

// The width argument of the three model calls below: WHOLE_WIDTH = the evaluator's n_items (the entries without
// `n_scored`, which also take an evaluator without items); anything else goes through scored_width().
constexpr int64_t WHOLE_WIDTH = -1;
inline int64_t width_of(int64_t n_scored, int64_t ni) { return n_scored == WHOLE_WIDTH ? ni : scored_width(n_scored, ni); }
// what a *_scored entry checks before it hands over to the call it shares with the entry without `n_scored`
irs_status check_scored_entry(const irs_evaluator *e, int64_t n_scored) {
  return guard([&] {
    check_arg(e != nullptr, "null argument.");
    scored_width(n_scored, e->n_items);
  });
}

}  // namespace
extern "C" {

static irs_status similarity_call(irs_evaluator *e, int64_t begin, int64_t end, int64_t n_model_users,
                                  int64_t n_profile_cols, const int64_t *x_indptr,
                                  const int32_t *x_indices, const double *x_data,
                                  const int64_t *w_indptr, const int32_t *w_indices,
                                  const double *w_data, int64_t n_scored, const int64_t *mask_indptr,
                                  const int32_t *mask_indices, int32_t n_cutoffs,
                                  const int64_t *cutoffs, int64_t offset, int32_t recall_with_cutoff,
                                  irs_metrics *out, int64_t *item_cnt) {
  return guard([&] {
    check_arg(e && out && item_cnt && cutoffs && x_indptr && w_indptr, "null argument.");
    check_arg(0 <= begin && begin <= end && end <= n_model_users, "user range out of bounds.");
    check_arg(n_cutoffs >= 0, "negative count.");
    const int64_t rows = end - begin, ni = e->n_items;
    const int64_t ns = width_of(n_scored, ni);  // W is [n_profile_cols, ns]; the block's row stride stays ni
    for (int32_t c = 0; c < n_cutoffs; c++) validate_call(e, rows, cutoffs[c], offset, 1);
    // the two CSR matrices: the profiles X [n_model_users, n_profile_cols] (rows begin .. end are read) and
    // W [n_profile_cols, n_items]: item-kNN / P3alpha / RP3beta: X = the training matrix, W item x item;
    // user-kNN (base.py:432-453: U[u] @ X): X = the user-user weights, W = the training matrix
    const int64_t np_ = n_profile_cols;
    check_arg(np_ >= 0 && np_ < (int64_t(1) << 31), "bad profile width.");
    ProfileRows x;
    x.take_pointers(x_indptr, begin, end, false);
    check_arg(w_indptr[0] == 0, "malformed indptr.");
    for (int64_t i = 0; i < np_; i++) check_arg(w_indptr[i + 1] >= w_indptr[i], "malformed indptr.");
    const int64_t w_nnz = w_indptr[np_];
    check_arg((x.nnz == 0 || (x_indices && x_data)) && (w_nnz == 0 || (w_indices && w_data)), "null argument.");
    x.scan_entries(x_indices, x_data, np_, true);
    // rows of W with strictly increasing columns (what every recommender of this package stores) are cut
    // into per-tile ranges on the device; any other W takes the whole-row walk.  (A column stored twice in a
    // row is not looked for here.)
    const WeightRowsScan w_rows = scan_weight_rows(w_indptr, w_indices, np_, ns, false);
    check_arg(!w_rows.out_of_range, "column index out of range.");
    const bool w_tiled = !w_rows.unsorted && w_nnz < (int64_t(1) << 31);
    IRS_HIP(hipSetDevice(e->device));
    hipStream_t s = nullptr;
    // uploads: the profile rows (values only when they are not all ones), W by rows, the mask rows
    DeviceBuffer<int64_t> d_xp, d_wp;
    DeviceBuffer<int32_t> d_xi, d_wi;
    DeviceBuffer<double> d_xv, d_wv;
    d_xp.upload(x.ptr, s);
    d_xi.upload(x_indices + x.first, static_cast<size_t>(x.nnz), s);
    if (!x.all_ones) d_xv.upload(x_data + x.first, static_cast<size_t>(x.nnz), s);
    d_wp.upload(w_indptr, static_cast<size_t>(np_) + 1, s);
    d_wi.upload(w_indices, static_cast<size_t>(w_nnz), s);
    d_wv.upload(w_data, static_cast<size_t>(w_nnz), s);
    CallMask mask;  // (stray columns: the kernel skips them)
    mask.upload_or_alias(mask_indptr, mask_indices, rows, ni, x, x_indices, d_xp, d_xi, s);
    // blocks of users whose dense float64 scores fit 4 GB; every cutoff ranks the same block.  (All 138,493 users
    // of the ML-20M shape, 29.6 GB of scores: 1 GB blocks 59.8 ms, 2 GB 50.1, 4 GB 44.5, 8 GB 42.6, one block
    // 40.5 - against 90 / 190 / 310 ms for the first call's allocation at 1 / 4 / 8 GB.)
    const int64_t per = rows_per_f64_block(ni, rows, false);
    const int32_t n_tiles = sim_tiles(ns);
    CutoffTotals totals(CutoffTotals::BLOCKS, n_cutoffs, ni, item_cnt, s);
    if (rows > 0) e->score_buf.alloc(static_cast<size_t>(per) * ni * 8);
    DeviceBuffer<int32_t> d_wt;
    if (w_tiled && rows > 0 && np_ > 0) build_tile_table(d_wt, d_wp, d_wi, np_, n_tiles, s);
    DeviceBuffer<int32_t> d_order;
    if (rows > 0) {
      std::vector<int32_t> order;
      launch_order(x.ptr, rows, per, order);
      d_order.upload(order, s);
    }
    const ProfileView xv{d_xp.ptr, d_xi.ptr, x.all_ones ? nullptr : d_xv.ptr};
    const SparseWeightsView wv{d_wp.ptr, d_wi.ptr, d_wv.ptr, w_nnz, n_tiles, d_wt.ptr};
    for (int64_t b = 0; b < rows; b += per) {
      const int64_t m = std::min(per, rows - b);
      double *scores = reinterpret_cast<double *>(e->score_buf.ptr);
      launch_sim_scores(xv, wv, b, m, ns, scores, d_order.ptr + b, s, ni);
      fill_unscored(scores, m, ni, ns, s);
      if (mask.ptr.ptr)
        hipLaunchKernelGGL(mask_block_kernel<double>, dim3(static_cast<unsigned>(m)), dim3(64), 0, s, scores, m, ni,
                           mask.ptr.ptr + b, mask.idx.ptr);
      IRS_HIP(hipGetLastError());
      totals.add_block<double>(e, scores, m, n_cutoffs, cutoffs, offset + b, recall_with_cutoff != 0, s);
    }
    totals.finish(e, n_cutoffs, out, item_cnt, s);
  });
}

irs_status irs_eval_get_metrics_similarity(irs_evaluator *e, int64_t begin, int64_t end, int64_t n_model_users,
                                           int64_t n_profile_cols,
                                           const int64_t *x_indptr, const int32_t *x_indices, const double *x_data,
                                           const int64_t *w_indptr, const int32_t *w_indices, const double *w_data,
                                           const int64_t *mask_indptr, const int32_t *mask_indices,
                                           int32_t n_cutoffs, const int64_t *cutoffs, int64_t offset,
                                           int32_t recall_with_cutoff, irs_metrics *out, int64_t *item_cnt) {
  return similarity_call(e, begin, end, n_model_users, n_profile_cols, x_indptr, x_indices,
                         x_data, w_indptr, w_indices, w_data, WHOLE_WIDTH, mask_indptr,
                         mask_indices, n_cutoffs, cutoffs, offset, recall_with_cutoff, out,
                         item_cnt);
}

irs_status irs_eval_get_metrics_similarity_scored(irs_evaluator *e, int64_t begin, int64_t end, int64_t n_model_users,
                                                  int64_t n_profile_cols, const int64_t *x_indptr,
                                                  const int32_t *x_indices, const double *x_data,
                                                  const int64_t *w_indptr, const int32_t *w_indices,
                                                  const double *w_data, int64_t n_scored, const int64_t *mask_indptr,
                                                  const int32_t *mask_indices, int32_t n_cutoffs,
                                                  const int64_t *cutoffs, int64_t offset, int32_t recall_with_cutoff,
                                                  irs_metrics *out, int64_t *item_cnt) {
  const irs_status st = check_scored_entry(e, n_scored);
  if (st != IRS_OK) return st;
  return similarity_call(e, begin, end, n_model_users, n_profile_cols, x_indptr, x_indices, x_data, w_indptr, w_indices,
                         w_data, n_scored, mask_indptr, mask_indices, n_cutoffs, cutoffs, offset, recall_with_cutoff,
                         out, item_cnt);
}

static irs_status dense_similarity_call(irs_evaluator *e, int64_t begin, int64_t end,
                                        int64_t n_model_users, int64_t n_profile_cols,
                                        const int64_t *x_indptr, const int32_t *x_indices,
                                        const double *x_data, int32_t w_is_f64, const void *w,
                                        int64_t n_scored, const int64_t *mask_indptr,
                                        const int32_t *mask_indices, int32_t n_cutoffs,
                                        const int64_t *cutoffs, int64_t offset,
                                        int32_t recall_with_cutoff, irs_metrics *out,
                                        int64_t *item_cnt) {
  return guard([&] {
    check_arg(e && out && item_cnt && cutoffs && x_indptr, "null argument.");
    check_arg(0 <= begin && begin <= end && end <= n_model_users, "user range out of bounds.");
    check_arg(n_cutoffs >= 0, "negative count.");
    const int64_t rows = end - begin, ni = e->n_items, np_ = n_profile_cols;
    const int64_t ns = width_of(n_scored, ni);  // W is [n_profile_cols, ns]; the block's row stride stays ni
    for (int32_t c = 0; c < n_cutoffs; c++) validate_call(e, rows, cutoffs[c], offset, 1);
    check_arg(np_ >= 0 && np_ < (int64_t(1) << 31), "bad profile width.");
    ProfileRows x;
    x.take_pointers(x_indptr, begin, end, false);
    const int64_t x_nnz = x.nnz;
    check_arg((x_nnz == 0 || (x_indices && x_data)) && (np_ == 0 || ni == 0 || w != nullptr), "null argument.");
    x.scan_entries(x_indices, x_data, np_, false);
    IRS_HIP(hipSetDevice(e->device));
    hipStream_t s = nullptr;
    PhaseClock clock(s);
    // uploads: the profile rows as they are stored, W (once per call, never kept: a tuning loop evaluates every
    // fitted W once), the mask rows
    DeviceBuffer<int64_t> d_xp;
    DeviceBuffer<int32_t> d_xi;
    DeviceBuffer<double> d_xv;
    DeviceBuffer<char> d_w;
    d_xp.upload(x.ptr, s);
    d_xi.upload(x_indices + x.first, static_cast<size_t>(x_nnz), s);
    d_xv.upload(x_data + x.first, static_cast<size_t>(x_nnz), s);
    if (rows > 0 && x_nnz > 0)
      d_w.upload(static_cast<const char *>(w), static_cast<size_t>(np_) * ns * (w_is_f64 ? 8 : 4), s);
    CallMask mask;
    mask.upload(mask_indptr, mask_indices, rows, ni, true, s);
    const int64_t per = rows_per_f64_block(ni, rows, true);  // (whole chunks of the host loop)
    const int64_t n_strips = ceil_div(std::max<int64_t>(ns, 1), DS_STRIP);
    check_arg(per * n_strips < (int64_t(1) << 31), "score block too large for one launch.");
    CutoffTotals totals(CutoffTotals::CHUNKS, n_cutoffs, ni, item_cnt, s);
    DeviceBuffer<int32_t> d_order;
    if (rows > 0 && ni > 0) {
      e->score_buf.alloc(static_cast<size_t>(per) * ni * 8);
      std::vector<int32_t> order;
      launch_order(x.ptr, rows, per, order);
      d_order.upload(order, s);
    }
    clock.mark(PH_UPLOAD);
    const ProfileView xv{d_xp.ptr, d_xi.ptr, d_xv.ptr};
    for (int64_t b = 0; b < rows && ni > 0; b += per) {
      const int64_t m = std::min(per, rows - b);
      double *scores = reinterpret_cast<double *>(e->score_buf.ptr);
      if (x_nnz == 0)  // (no profile entry in the whole call: W was not uploaded, every score is 0)
        IRS_HIP(hipMemsetAsync(scores, 0, static_cast<size_t>(m) * ni * 8, s));
      else
        launch_dense_scores(xv, d_w.ptr, w_is_f64 != 0, b, m, ns, scores, d_order.ptr + b, s, ni);
      fill_unscored(scores, m, ni, ns, s);
      IRS_HIP(hipGetLastError());
      clock.mark(PH_SCORE);
      if (mask.ptr.ptr)
        hipLaunchKernelGGL(mask_block_kernel<double>, dim3(static_cast<unsigned>(m)), dim3(64), 0, s, scores, m, ni,
                           static_cast<const int64_t *>(mask.ptr.ptr) + b, static_cast<const int32_t *>(mask.idx.ptr));
      IRS_HIP(hipGetLastError());
      clock.mark(PH_MASK);
      totals.add_block<double>(e, scores, m, n_cutoffs, cutoffs, offset + b, recall_with_cutoff != 0, s);
      clock.mark(PH_RANK);
    }
    totals.finish(e, n_cutoffs, out, item_cnt, s);
    clock.read(e->phase_ms);
  });
}

irs_status irs_eval_get_metrics_dense_similarity(irs_evaluator *e, int64_t begin, int64_t end, int64_t n_model_users,
                                                 int64_t n_profile_cols, const int64_t *x_indptr,
                                                 const int32_t *x_indices, const double *x_data, int32_t w_is_f64,
                                                 const void *w, const int64_t *mask_indptr,
                                                 const int32_t *mask_indices, int32_t n_cutoffs, const int64_t *cutoffs,
                                                 int64_t offset, int32_t recall_with_cutoff, irs_metrics *out,
                                                 int64_t *item_cnt) {
  return dense_similarity_call(e, begin, end, n_model_users, n_profile_cols, x_indptr, x_indices,
                               x_data, w_is_f64, w, WHOLE_WIDTH, mask_indptr, mask_indices,
                               n_cutoffs, cutoffs, offset, recall_with_cutoff, out, item_cnt);
}

irs_status irs_eval_get_metrics_dense_similarity_scored(irs_evaluator *e, int64_t begin, int64_t end,
                                                        int64_t n_model_users, int64_t n_profile_cols,
                                                        const int64_t *x_indptr, const int32_t *x_indices,
                                                        const double *x_data, int32_t w_is_f64, const void *w,
                                                        int64_t n_scored, const int64_t *mask_indptr,
                                                        const int32_t *mask_indices, int32_t n_cutoffs,
                                                        const int64_t *cutoffs, int64_t offset,
                                                        int32_t recall_with_cutoff, irs_metrics *out,
                                                        int64_t *item_cnt) {
  const irs_status st = check_scored_entry(e, n_scored);
  if (st != IRS_OK) return st;
  return dense_similarity_call(e, begin, end, n_model_users, n_profile_cols, x_indptr, x_indices, x_data, w_is_f64, w,
                               n_scored, mask_indptr, mask_indices, n_cutoffs, cutoffs, offset, recall_with_cutoff,
                               out, item_cnt);
}

static irs_status factors_call(irs_evaluator *e, int64_t begin, int64_t end, int64_t n_model_users,
                               int32_t k, const float *user_factors, const float *item_factors,
                               int64_t n_scored, const irs_metrics *running,
                               const int64_t *mask_indptr, const int32_t *mask_indices,
                               int32_t n_cutoffs, const int64_t *cutoffs, int64_t offset,
                               int32_t recall_with_cutoff, irs_metrics *out, int64_t *item_cnt) {
  return guard([&] {
    check_arg(e && out && item_cnt && cutoffs, "null argument.");
    check_arg(0 <= begin && begin <= end && end <= n_model_users, "user range out of bounds.");
    check_arg(n_cutoffs >= 0, "negative count.");
    check_arg(k >= 1 && k <= 576, "the number of factors must lie in 1 .. 576.");
    const int64_t rows = end - begin, ni = e->n_items;
    const int64_t ns = width_of(n_scored, ni);  // the item table is [ns, k]; the block's row stride stays ni
    for (int32_t c = 0; c < n_cutoffs; c++) validate_call(e, rows, cutoffs[c], offset, 1);
    check_arg((rows == 0 || user_factors) && (ni == 0 || item_factors), "null argument.");
    IRS_HIP(hipSetDevice(e->device));
    hipStream_t s = nullptr;
    PhaseClock clock(s);
    // the factor tables, rows zero-padded to KP (a multiple of 32) on the way up
    const int32_t KP = (k + 31) / 32 * 32;
    DeviceBuffer<float> d_user, d_item;
    upload_padded(d_user, rows > 0 ? user_factors + begin * static_cast<int64_t>(k) : nullptr, rows, k, KP, s);
    upload_padded(d_item, item_factors, ns, k, KP, s);
    CallMask mask;
    mask.upload(mask_indptr, mask_indices, rows, ni, true, s);
    // users scored and ranked per pass: as in irs_eval_get_metrics_ials, in whole chunks of the host loop
    const int64_t BLOCK = rows_per_f32_block(ni, "IRSPACK_AMD_EVAL_BLOCK", true, 1024);
    CutoffTotals totals(CutoffTotals::CHUNKS, n_cutoffs, ni, item_cnt, s, running);
    DeviceBuffer<float> &scores = e->fused_scores;
    if (rows > 0 && ni > 0) scores.alloc(static_cast<size_t>(std::min(BLOCK, rows)) * ni);
    clock.mark(PH_UPLOAD);
    for (int64_t b = 0; b < rows && ni > 0; b += BLOCK) {
      const int64_t m = std::min(BLOCK, rows - b);
      if (irs_gk_scores_device_(d_user.ptr + b * KP, d_item.ptr, KP, m, ns, scores.ptr, ni, s) != IRS_OK)
        throw std::runtime_error(irs_last_error());
      fill_unscored(scores.ptr, m, ni, ns, s);
      clock.mark(PH_SCORE);
      if (mask.ptr.ptr)
        hipLaunchKernelGGL(mask_rows_kernel, dim3(static_cast<unsigned>(m)), dim3(64), 0, s, scores.ptr, m, ni,
                           static_cast<const int64_t *>(mask.ptr.ptr) + b, static_cast<const int32_t *>(mask.idx.ptr),
                           static_cast<const int32_t *>(nullptr));
      IRS_HIP(hipGetLastError());
      clock.mark(PH_MASK);
      totals.add_block<float>(e, scores.ptr, m, n_cutoffs, cutoffs, offset + b, recall_with_cutoff != 0, s);
      clock.mark(PH_RANK);
    }
    totals.finish(e, n_cutoffs, out, item_cnt, s);
    clock.read(e->phase_ms);
  });
}

irs_status irs_eval_get_metrics_factors(irs_evaluator *e, int64_t begin, int64_t end, int64_t n_model_users, int32_t k,
                                        const float *user_factors, const float *item_factors,
                                        const int64_t *mask_indptr, const int32_t *mask_indices, int32_t n_cutoffs,
                                        const int64_t *cutoffs, int64_t offset, int32_t recall_with_cutoff,
                                        irs_metrics *out, int64_t *item_cnt) {
  return factors_call(e, begin, end, n_model_users, k, user_factors, item_factors, WHOLE_WIDTH,
                      nullptr, mask_indptr, mask_indices, n_cutoffs, cutoffs, offset,
                      recall_with_cutoff, out, item_cnt);
}

irs_status irs_eval_get_metrics_factors_scored(irs_evaluator *e, int64_t begin, int64_t end, int64_t n_model_users,
                                               int32_t k, const float *user_factors, const float *item_factors,
                                               int64_t n_scored, const irs_metrics *running,
                                               const int64_t *mask_indptr, const int32_t *mask_indices,
                                               int32_t n_cutoffs, const int64_t *cutoffs, int64_t offset,
                                               int32_t recall_with_cutoff, irs_metrics *out, int64_t *item_cnt) {
  const irs_status st = check_scored_entry(e, n_scored);
  if (st != IRS_OK) return st;
  return factors_call(e, begin, end, n_model_users, k, user_factors, item_factors, n_scored, running, mask_indptr,
                      mask_indices, n_cutoffs, cutoffs, offset, recall_with_cutoff, out, item_cnt);
}

irs_status irs_eval_last_phases(irs_evaluator *e, double *ms) {
  return guard([&] {
    check_arg(e && ms, "null argument.");
    std::copy(e->phase_ms, e->phase_ms + 4, ms);
  });
}

irs_status irs_eval_get_metrics_ials(irs_evaluator *e, irs_ials_trainer *t, int64_t begin,
                                     int64_t end, const int64_t *mask_indptr,
                                     const int32_t *mask_indices, int64_t cutoff,
                                     int64_t offset, int32_t recall_with_cutoff,
                                     irs_metrics *out, int64_t *item_cnt) {
  return guard([&] {
    check_arg(e && t && out && item_cnt, "null argument.");
    check_arg(end >= begin && begin >= 0, "bad user block.");
    const int64_t rows = end - begin;
    validate_call(e, rows, cutoff, offset, 1);
    IRS_HIP(hipSetDevice(e->device));
    // users scored and ranked per pass: enough rows to fill the device with one wave per row
    // (32 waves x 256 CUs), within a 2 GiB score block
    const int64_t BLOCK = rows_per_f32_block(e->n_items, "IRSPACK_AMD_EVAL_BLOCK", false, 1024);
    DeviceBuffer<int64_t> mptr;
    DeviceBuffer<int32_t> midx;
    void *sv = nullptr;
    int32_t dev = 0;
    // a zero-row call only fetches the trainer's stream / device
    if (irs_ials_scores_device_(t, begin, begin, nullptr, &sv, &dev) != IRS_OK)
      throw std::runtime_error(irs_last_error());
    check_arg(dev == e->device, "evaluator and trainer live on different devices.");
    hipStream_t s = static_cast<hipStream_t>(sv);
    const auto host_t0 = std::chrono::steady_clock::now();
    if (!e->ev_first) {
      IRS_HIP(hipEventCreate(&e->ev_first));
      IRS_HIP(hipEventCreate(&e->ev_last));
    }
    IRS_HIP(hipEventRecord(e->ev_first, s));
    e->span_open = true;
    struct CloseSpan {  // the call's times, whichever path returns (irs_eval_stats: call_ms, device_span_ms)
      irs_evaluator *e;
      std::chrono::steady_clock::time_point t0;
      ~CloseSpan() {
        float ms = 0.0f;
        if (e->span_open && hipEventElapsedTime(&ms, e->ev_first, e->ev_last) != hipSuccess) {
          (void)hipGetLastError();
          ms = 0.0f;
        }
        e->span_open = false;
        e->stats.device_span_ms = ms;
        e->stats.call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      }
    } close_span{e, host_t0};
    begin_accumulate(e, s);
    const int64_t *d_mptr = nullptr;
    const int32_t *d_midx = nullptr;
    if (mask_indptr) {
      std::vector<int64_t> mp(mask_indptr, mask_indptr + rows + 1);
      mptr.upload(mp, s);
      midx.upload(mask_indices, static_cast<size_t>(mask_indptr[rows]), s);
      IRS_HIP(hipStreamSynchronize(s));
      d_mptr = mptr.ptr;
      d_midx = midx.ptr;
    } else if (e->mask_rows == rows) {  // the cached mask (irs_eval_cache_mask)
      d_mptr = e->mask_ptr.ptr;
      d_midx = e->mask_idx.ptr;
    }
    if (emit_path(e, t, begin, rows, d_mptr, d_midx, cutoff, offset, recall_with_cutoff != 0, s)) {
      finish_accumulate(e, out, item_cnt, s);
      return;
    }
    begin_accumulate(e, s);  // (an abandoned attempt may have touched the sums)
    e->stats = irs_eval_stats{0, 0, ceil_div(rows, 64) * ceil_div(e->n_items, 64),
                              ceil_div(rows, 64) * ceil_div(e->n_items, 64), 0};
    DeviceBuffer<float> &scores = e->fused_scores;
    scores.alloc(static_cast<size_t>(std::min(BLOCK, std::max<int64_t>(rows, 1))) * e->n_items);
    for (int64_t b = 0; b < rows; b += BLOCK) {
      const int64_t m = std::min(BLOCK, rows - b);
      if (irs_ials_scores_device_(t, begin + b, begin + b + m, scores.ptr, &sv, &dev) != IRS_OK)
        throw std::runtime_error(irs_last_error());
      if (d_mptr)
        hipLaunchKernelGGL(mask_rows_kernel, dim3(m), dim3(64), 0, s, scores.ptr, m, e->n_items,
                           d_mptr + b, d_midx);
      rank_block<float>(e, scores.ptr, m, cutoff, offset + b, recall_with_cutoff != 0, s);
    }
    finish_accumulate(e, out, item_cnt, s);
  });
}

irs_status irs_eval_cache_mask(irs_evaluator *e, int64_t rows, const int64_t *mask_indptr,
                               const int32_t *mask_indices) {
  return guard([&] {
    check_arg(e != nullptr, "null argument.");
    e->mask_bits_rows = -1;  // the bitmap follows the cached mask
    if (mask_indptr == nullptr || rows <= 0) {  // drop the cached mask
      e->mask_rows = -1;
      return;
    }
    check_arg(mask_indices != nullptr && mask_indptr[0] == 0, "malformed mask.");
    IRS_HIP(hipSetDevice(e->device));
    hipStream_t s = nullptr;
    std::vector<int64_t> mp(mask_indptr, mask_indptr + rows + 1);
    e->mask_ptr.upload(mp, s);
    e->mask_idx.upload(mask_indices, static_cast<size_t>(std::max<int64_t>(mask_indptr[rows], 1)), s);
    IRS_HIP(hipStreamSynchronize(s));
    e->mask_rows = rows;
  });
}

// 64-bit content fingerprint of a host buffer on several threads (the strict check of the
// evaluator's device-resident mask: every byte of ~140 MB per call, 4.5 ms with one thread of
// xxh3).  Not cryptographic: per 1 MiB piece a multiply-rotate mix of its 8-byte words (any changed
// word changes the piece's value), the pieces combined with their position.
irs_status irs_fingerprint(const void *data, int64_t n_bytes, uint64_t seed, uint64_t *out) {
  return guard([&] {
    check_arg(out != nullptr && n_bytes >= 0 && (data != nullptr || n_bytes == 0), "bad argument.");
    const unsigned char *p = static_cast<const unsigned char *>(data);
    constexpr int64_t PIECE = int64_t(1) << 20;
    const int64_t n_pieces = ceil_div(n_bytes, PIECE);
    int n_thr = static_cast<int>(std::max<int64_t>(
        1, std::min<int64_t>({16, static_cast<int64_t>(std::thread::hardware_concurrency()), n_pieces / 4 + 1})));
    // (IRSPACK_AMD_FINGERPRINT_THREADS: tests force the thread count - the value must not depend on it)
    if (const char *te = std::getenv("IRSPACK_AMD_FINGERPRINT_THREADS"))
      n_thr = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(64, std::atoll(te))));
    auto mix = [](uint64_t h, uint64_t w) {
      h ^= w * 0x9E3779B97F4A7C15ull;
      h = (h << 29) | (h >> 35);
      return h * 0xD6E8FEB86659FD93ull;
    };
    auto piece_hash = [&](int64_t k) {
      const int64_t b = k * PIECE, e = std::min(n_bytes, b + PIECE);
      uint64_t h[4] = {seed ^ 0x243F6A8885A308D3ull, seed ^ 0x13198A2E03707344ull, seed ^ 0xA4093822299F31D0ull,
                       seed ^ 0x082EFA98EC4E6C89ull};  // four independent lanes: the loop pipelines
      int64_t i = b;
      for (; i + 32 <= e; i += 32) {
        uint64_t w[4];
        std::memcpy(w, p + i, 32);
        h[0] = mix(h[0], w[0]);
        h[1] = mix(h[1], w[1]);
        h[2] = mix(h[2], w[2]);
        h[3] = mix(h[3], w[3]);
      }
      uint64_t tail[4] = {0, 0, 0, 0};
      std::memcpy(tail, p + i, static_cast<size_t>(e - i));
      for (int q = 0; q < 4; q++) h[q] = mix(h[q], tail[q] + static_cast<uint64_t>(e - i));
      return mix(mix(h[0], h[1]), mix(h[2], h[3]) + static_cast<uint64_t>(k));
    };
    std::vector<uint64_t> part(static_cast<size_t>(n_thr), 0);
    auto work = [&](int t) {
      uint64_t acc = 0;
      for (int64_t k = t; k < n_pieces; k += n_thr) acc += mix(piece_hash(k), static_cast<uint64_t>(k) + 1);
      part[t] = acc;
    };
    {
      std::vector<std::thread> th;
      struct Join {
        std::vector<std::thread> &v;
        ~Join() { for (auto &t : v) if (t.joinable()) t.join(); }
      } join{th};
      for (int t = 1; t < n_thr; t++) th.emplace_back(work, t);
      work(0);
    }
    uint64_t h = mix(seed, static_cast<uint64_t>(n_bytes));
    for (int t = 0; t < n_thr; t++) h += part[t];  // (a sum: independent of the thread count's dealing)
    *out = h;
  });
}

irs_status irs_retrieve_recommend(int32_t is_f64, const void *scores, int64_t rows,
                                  int64_t n_items, int64_t n_lists, const int64_t *list_ptr,
                                  const int64_t *list_items, int64_t cutoff, int64_t n_threads,
                                  int32_t device, int32_t *out_idx) {
  return guard([&] {
    // util.hpp:426-439
    check_arg(n_threads > 0, "n_threads must not be 0.");
    check_arg(rows >= 0 && n_items >= 0, "negative shape.");
    check_arg(n_lists == 0 || n_lists == 1 || n_lists == rows,
              "allowed_indices, if not empty, must have a size equal to X.rows()");
    check_arg(out_idx != nullptr && (rows == 0 || scores != nullptr), "null argument.");
    if (rows == 0 || cutoff <= 0) return;
    require_device(device);
    hipStream_t s = nullptr;
    CandidateLists lists;
    lists.take(n_lists, list_ptr, list_items, n_items, false);
    DeviceBuffer<int64_t> d_lptr;
    DeviceBuffer<int32_t> d_litems, d_rec;
    DeviceBuffer<RowOut> d_rows;
    DeviceBuffer<char> d_scores;
    if (n_lists > 0) {
      d_lptr.upload(lists.ptr, s);
      d_litems.upload(lists.items, s);
    }
    const size_t bytes = static_cast<size_t>(rows) * n_items * (is_f64 ? 8 : 4);
    d_scores.alloc(std::max<size_t>(bytes, 8));
    IRS_HIP(hipMemcpyAsync(d_scores.ptr, scores, bytes, hipMemcpyHostToDevice, s));
    d_rec.alloc(static_cast<size_t>(rows) * cutoff);
    d_rows.alloc(rows);
    DeviceBuffer<int32_t> d_todo;
    d_todo.alloc(rows);
    const EvalParams p = retrieve_params(d_scores.ptr, rows, n_items, 0, n_lists, d_lptr.ptr, d_litems.ptr, cutoff,
                                         d_rows.ptr, d_rec.ptr);
    if (is_f64)
      launch_rank<double>(p, lists.max_cand, s, d_todo.ptr);
    else
      launch_rank<float>(p, lists.max_cand, s, d_todo.ptr);
    IRS_HIP(hipGetLastError());
    IRS_HIP(hipMemcpyAsync(out_idx, d_rec.ptr, static_cast<size_t>(rows) * cutoff * sizeof(int32_t),
                           hipMemcpyDeviceToHost, s));
    IRS_HIP(hipStreamSynchronize(s));
  });
}

}  // extern "C"

#include "serve_calls.hpp"
