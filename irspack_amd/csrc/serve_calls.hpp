// Serving: irs_serve_* (include/irspack_amd.h).  The item-side operand lives in an irs_server; a recommend call
// uploads its rows, then per chunk: score, mask, rank (retrieve = 1), emit (serve_kernels.hpp).  A neighbour call
// (irs_serve_neighbors) uploads only ids and scores them against the resident operand itself; the rest is the same.
// (Included by evaluator.hip at the end of its translation unit: the calls use its host helpers and kernels.)
#pragma once

namespace {

// what the two recommend calls and the neighbour call share
struct ServeCall {
  int64_t rows;
  const int64_t *excl_indptr;
  const int32_t *excl_indices;
  int64_t n_lists;
  const int64_t *list_ptr;
  const int64_t *list_items;
  int64_t cutoff;
  int32_t *out_idx;
  float *out_score;
  int32_t *out_len;
  // filled by serve_check
  int32_t width = 0;
  MaskRows excl;
  CandidateLists lists;
};

// rows per chunk: a 2 GiB float block (the same rows of float64 scores: 4 GB), at most 16384 rows (eval_host_prep.hpp)
int64_t serve_block_rows(int64_t ni) { return rows_per_f32_block(ni, "IRSPACK_AMD_SERVE_BLOCK", false, 1); }

// every argument check of what the two calls share (host only); false: nothing to compute (the outputs are set)
bool serve_check(irs_server *sv, ServeCall &c) {
  check_arg(c.rows >= 0, "negative row count.");
  check_arg(c.cutoff >= 0, "cutoff must not be negative.");
  check_arg(c.n_lists == 0 || c.n_lists == 1 || c.n_lists == c.rows,
            "allowed_indices, if not empty, must have a size equal to X.rows()");
  check_arg(c.n_lists == 0 || c.list_ptr != nullptr, "null argument.");
  const int64_t ni = sv->n_items;
  c.width = static_cast<int32_t>(std::min<int64_t>(c.cutoff, ni));
  check_arg(c.rows == 0 || c.out_len != nullptr, "null argument.");
  check_arg(c.rows == 0 || c.width == 0 || (c.out_idx && c.out_score), "null argument.");
  check_arg(c.rows * static_cast<int64_t>(std::max(c.width, 1)) < (int64_t(1) << 40), "output too large.");
  // exclusion rows: pointers that do not decrease, columns inside [0, n_items); rebased to 0
  c.excl.take(c.excl_indptr, c.excl_indices, c.rows, ni, true, true);
  c.lists.take(c.n_lists, c.list_ptr, c.list_items, ni, true);
  if (c.rows == 0) return false;
  if (c.width == 0) {
    std::fill(c.out_len, c.out_len + c.rows, 0);
    return false;
  }
  return true;
}

// The chunks of a call: `score(b, m, block)` leaves the scores of the rows b .. b + m in `block`; then the
// exclusions, the ranking and the output stage; three copies home after the last chunk.
template <class T, class ScoreFn>
void serve_run(irs_server *sv, ServeCall &c, hipStream_t s, PhaseClock &clock, ScoreFn &&score) {
  const int64_t ni = sv->n_items, rows = c.rows, width = c.width;
  upload_mask_rows(c.excl, c.excl_indices, sv->excl_ptr, sv->excl_idx, s);
  if (c.n_lists > 0) {
    sv->list_ptr.upload(c.lists.ptr, s);
    sv->list_items.upload(c.lists.items, s);
  }
  const int64_t BLOCK = std::min(serve_block_rows(ni), rows);
  sv->scores.alloc(static_cast<size_t>(BLOCK) * ni * sizeof(T));
  sv->rec.alloc(static_cast<size_t>(BLOCK) * width);
  sv->todo.alloc(static_cast<size_t>(BLOCK));
  sv->row_out.alloc(static_cast<size_t>(BLOCK));
  sv->out_idx.alloc(static_cast<size_t>(rows) * width);
  sv->out_score.alloc(static_cast<size_t>(rows) * width);
  sv->out_len.alloc(static_cast<size_t>(rows));
  clock.mark(PH_UPLOAD);
  T *block = reinterpret_cast<T *>(sv->scores.ptr);
  for (int64_t b = 0; b < rows; b += BLOCK) {
    const int64_t m = std::min(BLOCK, rows - b);
    score(b, m, block);
    IRS_HIP(hipGetLastError());
    clock.mark(PH_SCORE);
    if (c.excl.nnz > 0)
      hipLaunchKernelGGL(mask_block_kernel<T>, dim3(static_cast<unsigned>(m)), dim3(64), 0, s, block, m, ni,
                         static_cast<const int64_t *>(sv->excl_ptr.ptr) + b, static_cast<const int32_t *>(sv->excl_idx.ptr));
    IRS_HIP(hipGetLastError());
    clock.mark(PH_MASK);
    const EvalParams p = retrieve_params(block, m, ni, b, c.n_lists, sv->list_ptr.ptr, sv->list_items.ptr, width,
                                         sv->row_out.ptr, sv->rec.ptr);
    if (c.n_lists > 0)  // (equal scores in candidate order, whatever the order of the list)
      launch_rank<T, true>(p, c.lists.max_cand, s, sv->todo.ptr);
    else
      launch_rank<T>(p, c.lists.max_cand, s, sv->todo.ptr);
    hipLaunchKernelGGL(serve_emit_kernel<T>, dim3(static_cast<unsigned>(ceil_div(m, 4))), dim3(256), 0, s,
                       sv->rec.ptr, block, m, ni, static_cast<int32_t>(width), sv->out_idx.ptr + b * width,
                       sv->out_score.ptr + b * width, sv->out_len.ptr + b);
    IRS_HIP(hipGetLastError());
    clock.mark(PH_RANK);
  }
  IRS_HIP(hipMemcpyAsync(c.out_idx, sv->out_idx.ptr, static_cast<size_t>(rows) * width * sizeof(int32_t),
                         hipMemcpyDeviceToHost, s));
  IRS_HIP(hipMemcpyAsync(c.out_score, sv->out_score.ptr, static_cast<size_t>(rows) * width * sizeof(float),
                         hipMemcpyDeviceToHost, s));
  IRS_HIP(hipMemcpyAsync(c.out_len, sv->out_len.ptr, static_cast<size_t>(rows) * sizeof(int32_t),
                         hipMemcpyDeviceToHost, s));
  clock.mark(PH_RANK);
  IRS_HIP(hipStreamSynchronize(s));
  clock.read(sv->phase_ms);
}

}  // namespace

extern "C" {

irs_status irs_serve_create_similarity(int64_t n_profile_cols, int64_t n_items, const int64_t *w_indptr,
                                       const int32_t *w_indices, const double *w_data, int32_t device,
                                       irs_server **out) {
  return guard([&] {
    check_arg(out && w_indptr, "null argument.");
    const int64_t np_ = n_profile_cols, ni = n_items;
    check_arg(np_ >= 0 && np_ < (int64_t(1) << 31) && ni >= 0 && ni < (int64_t(1) << 31), "bad shape.");
    check_arg(w_indptr[0] == 0, "malformed indptr.");
    for (int64_t i = 0; i < np_; i++) check_arg(w_indptr[i + 1] >= w_indptr[i], "malformed indptr.");
    const int64_t w_nnz = w_indptr[np_];
    check_arg(w_nnz == 0 || (w_indices && w_data), "null argument.");
    // columns in range; a column stored twice in a row is refused (two lanes of sim_score_kernel would add to
    // one sum at the same time); rows with increasing columns are cut into per-tile ranges
    const WeightRowsScan w_rows = scan_weight_rows(w_indptr, w_indices, np_, ni, true);
    check_arg(!w_rows.out_of_range, "column index out of range.");
    check_arg(!w_rows.duplicate, "duplicate column in a row of W");
    require_device(device);
    auto sv = std::make_unique<irs_server>();
    sv->kind = irs_server::SPARSE;
    sv->device = device;
    sv->n_profile_cols = np_;
    sv->n_items = ni;
    sv->w_nnz = w_nnz;
    sv->n_tiles = sim_tiles(ni);
    sv->w_tiled = !w_rows.unsorted && w_nnz < (int64_t(1) << 31) && np_ > 0;
    hipStream_t s = nullptr;
    sv->w_ptr.upload(w_indptr, static_cast<size_t>(np_) + 1, s);
    sv->w_idx.upload(w_indices, static_cast<size_t>(w_nnz), s);
    sv->w_val.upload(w_data, static_cast<size_t>(w_nnz), s);
    if (sv->w_tiled) build_tile_table(sv->w_tptr, sv->w_ptr, sv->w_idx, np_, sv->n_tiles, s);
    IRS_HIP(hipStreamSynchronize(s));
    *out = sv.release();
  });
}

irs_status irs_serve_create_dense_similarity(int64_t n_profile_cols, int64_t n_items, int32_t w_is_f64, const void *w,
                                             int32_t device, irs_server **out) {
  return guard([&] {
    check_arg(out != nullptr, "null argument.");
    const int64_t np_ = n_profile_cols, ni = n_items;
    check_arg(np_ >= 0 && np_ < (int64_t(1) << 31) && ni >= 0 && ni < (int64_t(1) << 31), "bad shape.");
    check_arg(np_ == 0 || ni == 0 || w != nullptr, "null argument.");
    require_device(device);
    auto sv = std::make_unique<irs_server>();
    sv->kind = irs_server::DENSE;
    sv->device = device;
    sv->n_profile_cols = np_;
    sv->n_items = ni;
    sv->w_is_f64 = w_is_f64 ? 1 : 0;
    hipStream_t s = nullptr;
    if (np_ > 0 && ni > 0)
      sv->w_dense.upload(static_cast<const char *>(w), static_cast<size_t>(np_) * ni * (w_is_f64 ? 8 : 4), s);
    IRS_HIP(hipStreamSynchronize(s));
    *out = sv.release();
  });
}

irs_status irs_serve_create_factors(int64_t n_items, int32_t k, const float *item_factors, int32_t device,
                                    irs_server **out) {
  return guard([&] {
    check_arg(out != nullptr, "null argument.");
    check_arg(k >= 1 && k <= 576, "the number of factors must lie in 1 .. 576.");
    check_arg(n_items >= 0 && n_items < (int64_t(1) << 31), "bad shape.");
    check_arg(n_items == 0 || item_factors != nullptr, "null argument.");
    require_device(device);
    auto sv = std::make_unique<irs_server>();
    sv->kind = irs_server::FACTORS;
    sv->device = device;
    sv->n_items = n_items;
    sv->k = k;
    sv->KP = (k + 31) / 32 * 32;
    hipStream_t s = nullptr;
    upload_padded(sv->item, item_factors, n_items, k, sv->KP, s);
    IRS_HIP(hipStreamSynchronize(s));
    *out = sv.release();
  });
}

irs_status irs_serve_destroy(irs_server *sv) {
  return guard([&] {
    if (sv) {
      (void)hipSetDevice(sv->device);
      delete sv;
    }
  });
}

irs_status irs_serve_last_phases(irs_server *sv, double *ms) {
  return guard([&] {
    check_arg(sv && ms, "null argument.");
    std::lock_guard<std::mutex> one_call(sv->call_mutex);
    std::copy(sv->phase_ms, sv->phase_ms + 4, ms);
  });
}

irs_status irs_serve_recommend_profiles(irs_server *sv, int64_t rows, const int64_t *x_indptr, const int32_t *x_indices,
                                        const double *x_data, const int64_t *excl_indptr, const int32_t *excl_indices,
                                        int64_t n_lists, const int64_t *list_ptr, const int64_t *list_items,
                                        int64_t cutoff, int32_t *out_idx, float *out_score, int32_t *out_len) {
  return guard([&] {
    check_arg(sv != nullptr, "null argument.");
    check_arg(sv->kind == irs_server::SPARSE || sv->kind == irs_server::DENSE,
              "this server holds factors: call irs_serve_recommend_factors.");
    ServeCall c{rows, excl_indptr, excl_indices, n_lists, list_ptr, list_items, cutoff, out_idx, out_score, out_len};
    check_arg(rows <= 0 || x_indptr != nullptr, "null argument.");
    const int64_t np_ = sv->n_profile_cols, ni = sv->n_items;
    ProfileRows x;
    x.take_pointers(x_indptr, 0, rows, true);
    const int64_t x_nnz = x.nnz;
    check_arg(x_nnz == 0 || (x_indices && x_data), "null argument.");
    check_arg(x_nnz < (int64_t(1) << 40), "profile too large.");
    x.scan_entries(x_indices, x_data, np_, true);
    if (!serve_check(sv, c)) return;
    std::lock_guard<std::mutex> one_call(sv->call_mutex);  // (the call scratch is the handle's)
    const int64_t BLOCK = std::min(serve_block_rows(ni), rows);
    const int64_t n_strips = ceil_div(std::max<int64_t>(ni, 1), DS_STRIP);
    check_arg(BLOCK * std::max<int64_t>(n_strips, sv->n_tiles) < (int64_t(1) << 31), "score block too large for one launch.");
    IRS_HIP(hipSetDevice(sv->device));
    hipStream_t s = nullptr;
    PhaseClock clock(s);
    sv->x_ptr.upload(x.ptr, s);
    sv->x_idx.upload(x_indices + x.first, static_cast<size_t>(x_nnz), s);
    // (the sparse kernel reads no values when they are all ones; the dense one always does)
    const bool with_values = sv->kind == irs_server::DENSE || !x.all_ones;
    if (with_values) sv->x_val.upload(x_data + x.first, static_cast<size_t>(x_nnz), s);
    {
      std::vector<int32_t> order;
      launch_order(x.ptr, rows, BLOCK, order);
      sv->order.upload(order, s);
    }
    const ProfileView xv{sv->x_ptr.ptr, sv->x_idx.ptr, with_values ? sv->x_val.ptr : nullptr};
    const SparseWeightsView wv{sv->w_ptr.ptr, sv->w_idx.ptr, sv->w_val.ptr, sv->w_nnz, sv->n_tiles,
                               sv->w_tiled ? sv->w_tptr.ptr : nullptr};
    serve_run<double>(sv, c, s, clock, [&](int64_t b, int64_t m, double *block) {
      const int32_t *order = static_cast<const int32_t *>(sv->order.ptr) + b;
      if (x_nnz == 0) {  // (no profile entry in the whole call: every score is 0)
        IRS_HIP(hipMemsetAsync(block, 0, static_cast<size_t>(m) * ni * 8, s));
      } else if (sv->kind == irs_server::SPARSE) {
        launch_sim_scores(xv, wv, b, m, ni, block, order, s);
      } else {
        launch_dense_scores(xv, sv->w_dense.ptr, sv->w_is_f64 != 0, b, m, ni, block, order, s);
      }
    });
  });
}

irs_status irs_serve_recommend_factors(irs_server *sv, int64_t rows, const float *user_factors,
                                       const int64_t *excl_indptr, const int32_t *excl_indices, int64_t n_lists,
                                       const int64_t *list_ptr, const int64_t *list_items, int64_t cutoff,
                                       int32_t *out_idx, float *out_score, int32_t *out_len) {
  return guard([&] {
    check_arg(sv != nullptr, "null argument.");
    check_arg(sv->kind == irs_server::FACTORS, "this server holds similarity weights: call irs_serve_recommend_profiles.");
    ServeCall c{rows, excl_indptr, excl_indices, n_lists, list_ptr, list_items, cutoff, out_idx, out_score, out_len};
    check_arg(rows <= 0 || user_factors != nullptr, "null argument.");
    if (!serve_check(sv, c)) return;
    std::lock_guard<std::mutex> one_call(sv->call_mutex);  // (the call scratch is the handle's)
    const int64_t ni = sv->n_items;
    const int32_t k = sv->k, KP = sv->KP;
    IRS_HIP(hipSetDevice(sv->device));
    hipStream_t s = nullptr;
    PhaseClock clock(s);
    upload_padded(sv->user, user_factors, rows, k, KP, s);  // (the user rows)
    serve_run<float>(sv, c, s, clock, [&](int64_t b, int64_t m, float *block) {
      if (irs_gk_scores_device_(sv->user.ptr + b * KP, sv->item.ptr, KP, m, ni, block, ni, s) != IRS_OK)
        throw std::runtime_error(irs_last_error());
    });
  });
}

irs_status irs_serve_neighbors(irs_server *sv, int64_t rows, const int64_t *ids, int32_t metric, int32_t k_used,
                               const int64_t *excl_indptr, const int32_t *excl_indices, int64_t n_lists,
                               const int64_t *list_ptr, const int64_t *list_items, int64_t cutoff, int32_t *out_idx,
                               float *out_score, int32_t *out_len) {
  return guard([&] {
    check_arg(sv != nullptr, "null argument.");
    const int64_t ni = sv->n_items;
    const bool factors = sv->kind == irs_server::FACTORS;
    if (factors) {
      check_arg(metric == IRS_NEIGHBOR_COSINE || metric == IRS_NEIGHBOR_DOT,
                "this server holds factors: the metric is IRS_NEIGHBOR_COSINE or IRS_NEIGHBOR_DOT.");
      check_arg(k_used >= 1 && k_used <= sv->k, "k_used must lie in 1 .. k.");
    } else {
      check_arg(metric == IRS_NEIGHBOR_WEIGHT, "this server holds similarity weights: the metric is IRS_NEIGHBOR_WEIGHT.");
      check_arg(k_used == 0, "k_used must be 0 on a similarity server.");
      check_arg(sv->n_profile_cols == ni, "neighbours need a square W.");
    }
    ServeCall c{rows, excl_indptr, excl_indices, n_lists, list_ptr, list_items, cutoff, out_idx, out_score, out_len};
    check_arg(rows <= 0 || ids != nullptr, "null argument.");
    for (int64_t r = 0; r < rows; r++) check_arg(ids[r] >= 0 && ids[r] < ni, "neighbour id out of range.");
    if (!serve_check(sv, c)) return;
    std::lock_guard<std::mutex> one_call(sv->call_mutex);  // (the call scratch is the handle's)
    IRS_HIP(hipSetDevice(sv->device));
    hipStream_t s = nullptr;
    PhaseClock clock(s);
    sv->nb_ids.upload(ids, static_cast<size_t>(rows), s);
    const int64_t *d_ids = sv->nb_ids.ptr;
    if (!factors) {
      serve_run<double>(sv, c, s, clock, [&](int64_t b, int64_t m, double *block) {
        const dim3 grid(static_cast<unsigned>(m)), wg(NB_THREADS);
        if (sv->kind == irs_server::SPARSE)
          hipLaunchKernelGGL(nb_sparse_rows_kernel, grid, wg, 0, s, block, m, ni, d_ids + b,
                             static_cast<const int64_t *>(sv->w_ptr.ptr), static_cast<const int32_t *>(sv->w_idx.ptr),
                             static_cast<const double *>(sv->w_val.ptr));
        else if (sv->w_is_f64)
          hipLaunchKernelGGL(nb_dense_rows_kernel<double>, grid, wg, 0, s, block, m, ni, d_ids + b,
                             reinterpret_cast<const double *>(sv->w_dense.ptr));
        else
          hipLaunchKernelGGL(nb_dense_rows_kernel<float>, grid, wg, 0, s, block, m, ni, d_ids + b,
                             reinterpret_cast<const float *>(sv->w_dense.ptr));
      });
      return;
    }
    const int32_t KP = sv->KP;
    const float *inv = nullptr;
    if (metric == IRS_NEIGHBOR_COSINE) {
      if (sv->inv_norm_k != k_used) {
        sv->inv_norm_k = 0;
        sv->inv_norm.alloc(static_cast<size_t>(ni));
        hipLaunchKernelGGL(nb_inv_norm_kernel, dim3(static_cast<unsigned>(ceil_div(ni, NB_ROWS_PER_BLOCK))),
                           dim3(NB_THREADS), 0, s, static_cast<const float *>(sv->item.ptr), ni, KP, k_used,
                           sv->inv_norm.ptr);
        IRS_HIP(hipGetLastError());
        sv->inv_norm_k = k_used;
      }
      inv = sv->inv_norm.ptr;
    }
    // the query block [rows, KP] out of the resident table (scaled for cosine, zero from k_used on)
    sv->user.alloc(static_cast<size_t>(rows) * KP);
    hipLaunchKernelGGL(nb_gather_kernel, dim3(static_cast<unsigned>(ceil_div(rows, NB_ROWS_PER_BLOCK))),
                       dim3(NB_THREADS), 0, s, static_cast<const float *>(sv->item.ptr), d_ids, rows, KP, k_used, inv,
                       sv->user.ptr);
    IRS_HIP(hipGetLastError());
    serve_run<float>(sv, c, s, clock, [&](int64_t b, int64_t m, float *block) {
      if (irs_gk_scores_device_(sv->user.ptr + b * KP, sv->item.ptr, KP, m, ni, block, ni, s) != IRS_OK)
        throw std::runtime_error(irs_last_error());
      hipLaunchKernelGGL(nb_finish_kernel, dim3(static_cast<unsigned>(m)), dim3(NB_THREADS), 0, s, block, m, ni,
                         d_ids + b, inv);
    });
  });
}

}  // extern "C"
