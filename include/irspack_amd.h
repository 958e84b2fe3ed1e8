/*
 * irspack_amd.h — C ABI of libirspack_amd.so, the MI355X (gfx950) native
 * implementation of irspack's compiled hot path.
 *
 * Every entry point below is what the reference's FFI for this path binds
 * (nanobind modules `irspack.recommenders._ials_core`, `._knn`,
 * `irspack.evaluation._core_evaluator`, and `remove_diagonal` and the SLIM
 * coordinate descent of `irspack.utils._util_cpp`); the reference interface each one replaces is
 * cited as file:line relative to /root/reference.
 *
 * Conventions
 *  - plain C: opaque handles, caller-owned host pointers + sizes, no torch or
 *    HIP types in any signature (`void *stream` is a hipStream_t passed through
 *    as an integer-sized pointer).
 *  - every function returns an irs_status: 0 ok, 1 invalid argument (the
 *    reference throws std::invalid_argument -> Python ValueError), 2 runtime
 *    error (std::runtime_error -> RuntimeError).  irs_last_error() returns the
 *    message of the last failing call on the calling thread.
 *  - calls are synchronous: on return device work is complete and outputs are
 *    host-visible, unless the function name ends in `_async`.
 *  - inputs are copied before return; the library never keeps a caller pointer.
 *  - CSR inputs: indptr int64[rows+1], indices int32[nnz] (sorted within a
 *    row), data float32 (iALS) or float64 (kNN / evaluator).
 *  - handles are not thread-safe (neither are the reference's objects).
 */
#ifndef IRSPACK_AMD_H
#define IRSPACK_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t irs_status;
#define IRS_OK 0
#define IRS_INVALID_ARGUMENT 1
#define IRS_RUNTIME_ERROR 2

/* Layout version of the structs below: 2 since irs_ceilings grew the gather rates, 3 since
 * irs_eval_stats carries the call's times.  A binding compares irs_abi_version() with the header it
 * was written against before passing structs. */
#define IRS_ABI_VERSION 4

const char *irs_last_error(void);
/* Library / device probe.  irs_device_count() returns 0 when no GPU is visible. */
int32_t irs_abi_version(void);
int32_t irs_device_count(void);

/* ------------------------------------------------------------------ iALS
 * enums: cpp_source/als/IALSLearningConfig.hpp:11-12, als/wrapper.cpp:25-40 */
#define IRS_LOSS_ORIGINAL 0
#define IRS_LOSS_IALSPP 1
#define IRS_SOLVER_CHOLESKY 0
#define IRS_SOLVER_CG 1
#define IRS_SOLVER_IALSPP 2

/* IALSModelConfig, IALSLearningConfig.hpp:15-31 (als/wrapper.cpp:42-71) */
typedef struct irs_ials_model_config {
  uint64_t K;
  float alpha0;
  float reg;
  float nu;
  float init_stdev;
  int32_t random_seed;
  int32_t loss_type;
  float lambda_user_feature;  /* feature-aware iALS: the ridge terms of the feature-weight  */
  float lambda_item_feature;  /* updates and the plain epochs before the first feature one */
  uint64_t feature_warmup_epochs; /* (irs_ials_feature_step).                              */
} irs_ials_model_config;

/* SolverConfig, IALSLearningConfig.hpp:97-112 (als/wrapper.cpp:92-115) */
typedef struct irs_ials_solver_config {
  uint64_t n_threads;   /* validated (> 0) like the reference; no effect on the GPU */
  int32_t solver_type;
  uint64_t max_cg_steps;
  uint64_t ialspp_subspace_dimension;
  uint64_t ialspp_iteration;
} irs_ials_solver_config;

typedef struct irs_ials_trainer irs_ials_trainer;

/* Row shard of a multi-GPU run: this handle solves users [user_begin,user_end)
 * and items [item_begin,item_end) and keeps full replicas of both factor
 * matrices.  {0,n_users,0,n_items} is the single-GPU case. */
typedef struct irs_ials_shard {
  int64_t user_begin, user_end, item_begin, item_end;
} irs_ials_shard;

/* IALSTrainer(config, X): IALSTrainer.hpp:710-720, als/wrapper.cpp:131-132.
 * Copies X (CSR f32), builds X^T, initialises both factor matrices from the same
 * seed (hpp:64-76, 718-719).  `shard` may be NULL. */
irs_status irs_ials_create(const irs_ials_model_config *config, int64_t n_users,
                           int64_t n_items, const int64_t *indptr,
                           const int32_t *indices, const float *data,
                           int32_t device, const irs_ials_shard *shard,
                           irs_ials_trainer **out);
/* Deserialising constructor IALSTrainer(config, user, item): hpp:746-756,
 * als/wrapper.cpp:167-181.  No interaction matrix is kept. */
irs_status irs_ials_create_from_factors(const irs_ials_model_config *config,
                                        int64_t n_users, int64_t n_items,
                                        const float *user, const float *item,
                                        int32_t device, irs_ials_trainer **out);
irs_status irs_ials_destroy(irs_ials_trainer *t);

/* IALSTrainer::step, hpp:784-788: P_u, user solve, P_i, item solve - the plain epoch, also on a
 * trainer with features (irs_ials_feature_step runs the feature-aware one).  Advances the epoch
 * counter that irs_ials_feature_step's warm-up reads. */
irs_status irs_ials_step(irs_ials_trainer *t, const irs_ials_solver_config *sc);
/* `.user` / `.item` read-write attributes, als/wrapper.cpp:158-159.
 * which: 0 = user, 1 = item.  out/in are C-contiguous float32 [rows, K]. */
irs_status irs_ials_get_factor(irs_ials_trainer *t, int32_t which, float *out);
irs_status irs_ials_set_factor(irs_ials_trainer *t, int32_t which,
                               const float *in, int64_t rows, int64_t cols);
/* IALSTrainer::user_scores, hpp:942-984.  out is float32 [end-begin, n_items]. */
irs_status irs_ials_user_scores(irs_ials_trainer *t, int64_t begin, int64_t end,
                                const irs_ials_solver_config *sc, float *out);
/* IALSTrainer::transform_user / transform_item, hpp:791-802 (+ X_to_vector
 * hpp:122-141).  side 0: X is [rows, n_items] -> out [rows, K];
 * side 1: X is [n_users, cols] -> out [cols, K]. */
irs_status irs_ials_transform(irs_ials_trainer *t, int32_t side, int64_t rows,
                              int64_t cols, const int64_t *indptr,
                              const int32_t *indices, const float *data,
                              const irs_ials_solver_config *sc, float *out);
/* transform_user_with_feature / transform_item_with_feature (hpp:803-824,
 * X_to_vector_with_prior hpp:143-168): as irs_ials_transform with a feature prior
 * (host float32 [out rows, K]): the rows start from the prior and the solve adds
 * reg_r * prior_r to the right-hand side (step_cholesky_with_prior hpp:333-385, step_cg
 * hpp:212-215).  IALSPP is rejected like in the reference (hpp:659-661). */
irs_status irs_ials_transform_with_prior(irs_ials_trainer *t, int32_t side, int64_t rows,
                                         int64_t cols, const int64_t *indptr,
                                         const int32_t *indices, const float *data,
                                         const float *prior,
                                         const irs_ials_solver_config *sc, float *out);
/* Feature-aware training, piece by piece: the prior of side `which` (host float32 [rows, K] =
 * features @ feature_weight) used by the following irs_ials_half_step_async calls of that side;
 * NULL clears it.  irs_ials_feature_step runs the whole feature-aware epoch, ridge update of the
 * feature weights (hpp:1052-1209) included, on the device; these calls remain for callers that
 * drive the half steps themselves. */
irs_status irs_ials_set_prior(irs_ials_trainer *t, int32_t which, const float *prior);
/* The two feature products of feature-aware training on the device, so that the factor
 * matrices never leave HBM during an epoch.  irs_ials_set_features stores the feature
 * matrix of side `which` (CSR float32 [rows, n_feat]; a dense matrix is passed as a full
 * CSR; FeatureMatrix, hpp:693-700).  irs_ials_apply_feature_prior computes
 * prior = features @ weight (host float32 [n_feat, K]; feature_times_weight hpp:702-708)
 * and installs it like irs_ials_set_prior.  irs_ials_feature_rhs returns
 * features^T (reg_r * factor_r) as host float32 [n_feat, K], the right-hand side of the
 * feature-weight ridge system (solve_feature_weight hpp:1134-1171). */
irs_status irs_ials_set_features(irs_ials_trainer *t, int32_t which, int64_t rows,
                                 int64_t n_feat, const int64_t *indptr,
                                 const int32_t *indices, const float *data);
irs_status irs_ials_apply_feature_prior(irs_ials_trainer *t, int32_t which,
                                        const float *weight);
irs_status irs_ials_feature_rhs(irs_ials_trainer *t, int32_t which, float *out);
/* IALSTrainer::step for a feature-aware trainer, hpp:758-789, in one call.  The epoch counter,
 * warm-up (feature_warmup_epochs plain epochs first), IALSPP rejection, empty-row check
 * (hpp:639-653), per-side prior -> solve -> ridge update of the feature weights, and the ridge
 * LLT cache all live in the library.  A side without features (or with n_feat == 0) runs its
 * plain half step.  The feature weights start at zero; the ridge system F^T D F + lambda I is
 * formed and factorised on the device once per side and kept until irs_ials_set_features
 * replaces that side's features.  One synchronisation, at the end.  Errors: IALSPP and an
 * undefined empty-row prior are invalid arguments; "Feature ridge Cholesky decomposition
 * failed." / "Feature ridge solve failed." are runtime errors (hpp:1104-1105, 1169-1170), after
 * which the weights keep their previous values.  Not available on a sharded trainer. */
irs_status irs_ials_feature_step(irs_ials_trainer *t, const irs_ials_solver_config *sc);
/* The `.user_feature_weight` / `.item_feature_weight` attributes (als/wrapper.cpp:160-161):
 * float32 [n_feat, K], C-contiguous, resident on the device.  get writes nothing when the side
 * has no weights.  set replaces W only (the cached ridge LLT stays); with features set, rows must
 * be that side's n_feat; cols must be K. */
irs_status irs_ials_get_feature_weight(irs_ials_trainer *t, int32_t which, float *out);
irs_status irs_ials_set_feature_weight(irs_ials_trainer *t, int32_t which,
                                       const float *in, int64_t rows, int64_t cols);
/* IALSTrainer::compute_loss, hpp:836-940. */
irs_status irs_ials_compute_loss(irs_ials_trainer *t,
                                 const irs_ials_solver_config *sc, float *out);

/* -- device-level pieces of IALSTrainer::step, for the multi-GPU host loop and
 *    the benchmark (one process per GPU; collectives run outside this library
 *    on the buffers these calls expose). -- */
irs_status irs_ials_set_stream(irs_ials_trainer *t, void *hip_stream);
/* which: 0 user factors, 1 item factors (float32 [rows, ld]; `rows` is the allocated row
 * count = the matrix's rows rounded up to a multiple of 8, zero padded, so that 1 / 2 / 4 / 8
 * equal row shards tile the buffer and one in-place all-gather can exchange them);
 * 2 / 3: Gramian used by the user / item solve (float32 [ld, ld], unscaled
 * sum over this rank's shard until irs_ials_finish_gramian is called). */
irs_status irs_ials_device_buffer(irs_ials_trainer *t, int32_t which,
                                  void **device_ptr, int64_t *rows, int64_t *ld);
/* Device-to-device copy of rows [row_begin,row_end) of buffer `which` (same
 * numbering as irs_ials_device_buffer) to (to_ext != 0) or from an external
 * device pointer holding (row_end-row_begin) x ld floats, on the trainer's
 * stream.  This is how the host loop stages the Gramian all-reduce and the
 * factor all-gather through torch.distributed tensors. */
irs_status irs_ials_copy_rows_async(irs_ials_trainer *t, int32_t which,
                                    int64_t row_begin, int64_t row_end,
                                    void *ext_device_ptr, int32_t to_ext);
/* Solver::prepare_p (hpp:78-115) split in two so that an all-reduce can sit in
 * between: partial = sum over this shard's rows of the *other* side's factors
 * (side 0: Gramian for the user solve = item rows of this shard). */
irs_status irs_ials_partial_gramian_async(irs_ials_trainer *t, int32_t side);
irs_status irs_ials_finish_gramian_async(irs_ials_trainer *t, int32_t side);
/* The two in one call for a trainer that holds every row (nothing to all-reduce in between): the
 * reduction writes the scaled Gramian in all its layouts itself, one launch less per half-epoch. */
irs_status irs_ials_gramian_async(irs_ials_trainer *t, int32_t side);
/* Solver::step (hpp:664-679) over this shard's rows of `side`. */
irs_status irs_ials_half_step_async(irs_ials_trainer *t, int32_t side,
                                    const irs_ials_solver_config *sc);
/* Waits for the stream and raises what the reference would have thrown from
 * inside the solve (hpp:317-323, 250-254). */
irs_status irs_ials_synchronize(irs_ials_trainer *t);
/* ---- row-sharded epoch (one process per GPU; no reference counterpart: the reference has no
 * distributed layer; the sharded unit is IALSTrainer::step, hpp:758-789).
 * irs_comm is this rank's transport of the two exchanges a sharded epoch needs: the K x K
 * all-reduce of the Gramian and the exchange of the freshly solved rows.
 *   irs_comm_create: two RCCL communicators (solved rows; Gramians).  id256: 256 bytes made by
 *     irs_comm_unique_id on ONE rank and handed to every rank by the caller (torch.distributed /
 *     MPI / a file).
 *   irs_comm_create_local: no RCCL at all - both exchanges are stores into the peers' mapped
 *     memory (below); needs irs_comm_export + irs_comm_attach before the first step.
 * How the solved rows reach the other replicas: */
#define IRS_EXCHANGE_AUTO 0      /* ncclAllGather in place (equal row blocks) or grouped broadcasts */
#define IRS_EXCHANGE_BROADCAST 1 /* one group of in-place ncclBroadcast, one per rank */
#define IRS_EXCHANGE_MESH 2      /* one group of ncclSend / ncclRecv: own block to every peer, every
                                  * peer's block into place - all links of the xGMI mesh at once */
#define IRS_EXCHANGE_PEER 3      /* a copy kernel stores the own block into every peer's mapped factor
                                  * buffer; arrival = sequence numbers in mapped flag words */
typedef struct irs_comm irs_comm;
irs_status irs_comm_unique_id(void *id256);
irs_status irs_comm_create(const void *id256, int32_t rank, int32_t world, int32_t device,
                           irs_comm **out);
irs_status irs_comm_create_local(int32_t rank, int32_t world, int32_t device, irs_comm **out);
irs_status irs_comm_destroy(irs_comm *c);
/* Peer stores: irs_comm_export fills handle256 (256 bytes: hipIpc handles of the trainer's two
 * factor buffers and of the communicator's flag + mailbox block); the caller gathers the blobs of
 * all ranks in rank order (world x 256 bytes) and gives them to irs_comm_attach on every rank,
 * which maps the peers' memory.  The trainer must outlive the communicator's use. */
irs_status irs_comm_export(irs_comm *c, irs_ials_trainer *t, void *handle256);
irs_status irs_comm_attach(irs_comm *c, irs_ials_trainer *t, const void *handles);
/* Selects IRS_EXCHANGE_* for the steps that follow (the same value on every rank). */
irs_status irs_comm_set_exchange(irs_comm *c, int32_t mode);
int32_t irs_comm_get_exchange(irs_comm *c);
/* IALSTrainer::step (hpp:758-789) over the ranks of `c`: the trainer holds the shard
 * [bounds[rank], bounds[rank + 1]) of each side (irs_ials_create with a shard); per half-epoch the
 * partial Gramian of the own rows is all-reduced, the own rows are solved and exchanged into
 * every replica (in place), the next half-epoch's Gramian overlapping the row exchange.  What the
 * reference would throw from inside a solve (hpp:317-323, 250-254) is raised on EVERY rank.
 * user_bounds / item_bounds: world + 1 row offsets, identical on every rank. */
irs_status irs_ials_sharded_step(irs_ials_trainer *t, const irs_ials_solver_config *sc, irs_comm *c,
                                 const int64_t *user_bounds, const int64_t *item_bounds);
/* Which rows of the last half-step were solved in the eigenbasis of the Gramian (measurement /
 * tests only, no reference counterpart): bit 0 = the rows of <= 32 stored entries. */
int32_t irs_ials_last_eigenbasis(irs_ials_trainer *t);
/* Test hook for the eigen-decomposition kernel of the short-row path (csrc/ials_eig_kernels.hpp):
 * P [K, K] row-major symmetric, K <= 128 -> Qrows [K, K] (row k = eigenvector k), lam [K],
 * stats [3] = largest, smallest eigenvalue, sweeps; P_prev (or NULL): a nearby matrix whose
 * eigenvectors warm-start the sweeps, as the previous epoch's Gramian does in a fit. */
irs_status irs_ials_eigen_debug(const float *P, int64_t K, int32_t device, float *Qrows, float *lam,
                                float *stats, const float *P_prev);
/* Per-kernel device times of the launches that follow (HIP events riding on the dispatches).
 * enable: 0 off, 1 every launch, 2 the dominant kernel only (the "ials_solve_*" launch of the side
 * with more rows: event pairs on all ten launches of an epoch cost 0.05 ms of 2.1, which a timed run
 * should not pay for durations it does not need). */
irs_status irs_ials_profile(irs_ials_trainer *t, int32_t enable);
irs_status irs_ials_profile_read(irs_ials_trainer *t, int32_t cap,
                                 char (*names)[48], double *ms,
                                 int64_t *launches, int32_t *count);

/* ------------------------------------------------------------------ kNN
 * cpp_source/knn/wrapper.cpp:11-66; KNNComputer knn.hpp:30-83 */
#define IRS_SIM_COSINE 0
#define IRS_SIM_ASYMMETRIC 1
#define IRS_SIM_JACCARD 2
#define IRS_SIM_TVERSKY 3
#define IRS_SIM_P3ALPHA 4
#define IRS_SIM_RP3BETA 5

typedef struct irs_knn_computer irs_knn_computer;

/* How (indptr, indices, data) store a [rows, cols] sparse matrix.  The reference's binding takes
 * either scipy layout (nanobind's Eigen caster converts: cpp_source/knn/wrapper.cpp:11-19 declares
 * `const CSRMatrix &`, and irspack/recommenders/knn.py:77-79 passes `X_weighted.T` / `X_train_all.T`,
 * which are CSC).  IRS_LAYOUT_CSC: the arrays are the compressed COLUMNS of the matrix, i.e. the CSR
 * arrays of its transpose [cols, rows] - indptr has cols + 1 entries, indices are row numbers.  No
 * host conversion: the library reads them as they are. */
#define IRS_LAYOUT_CSR 0
#define IRS_LAYOUT_CSC 1
/* Feature weighting of the interaction matrix before a similarity computer is built on it
 * (cpp_source/util.hpp:159-188 okapi_BM_25_weight, :190-209 tf_idf_weight; callers
 * irspack/recommenders/knn.py:67-75, user_knn.py:62-72). */
#define IRS_WEIGHT_NONE 0
#define IRS_WEIGHT_TF_IDF 1
#define IRS_WEIGHT_BM25 2
/* Optional description of the arrays handed to irs_knn_create (null = CSR, no weighting).
 * `weighting` is applied ON THE DEVICE, on the way in, to the matrix AS STORED - its compressed rows
 * are the documents, `indices` the terms, exactly what tf_idf_weight / okapi_BM_25_weight do with a
 * CSR matrix: `CosineSimilarityComputer(tf_idf_weight(X).T, ...)` of the reference is
 * irs_knn_create(rows = X.cols, cols = X.rows, X's CSR arrays, {IRS_LAYOUT_CSC, IRS_WEIGHT_TF_IDF}),
 * and the user-kNN `CosineSimilarityComputer(tf_idf_weight(X), ...)` is {IRS_LAYOUT_CSR,
 * IRS_WEIGHT_TF_IDF} - the weighted matrix never exists on the host.  Jaccard / Tversky binarise their
 * input (similarities.hpp:96-107, 143-159), which makes any weighting a no-op; P3alpha / RP3beta
 * take no weighting (invalid argument). */
typedef struct irs_knn_input {
  int32_t layout;    /* IRS_LAYOUT_* */
  int32_t weighting; /* IRS_WEIGHT_* */
  int32_t smooth;    /* tf-idf: idf = log(N / (df + smooth)) (util.hpp:203; the Python default is 1) */
  int32_t reserved;  /* 0 */
  double k1, b;      /* BM25 (util.hpp:159; Python defaults 1.2, 0.75) */
} irs_knn_input;

/* *SimilarityComputer(X, shrinkage, [alpha, beta, normalize], n_threads,
 * max_chunk_size): similarities.hpp:20-28, 61-72, 96-107, 143-159, 198-222,
 * 265-292.  X is float64 [rows = N, cols = n_features], stored as `input` says. */
irs_status irs_knn_create(int32_t sim_type, int64_t rows, int64_t cols,
                          const int64_t *indptr, const int32_t *indices,
                          const double *data, const irs_knn_input *input,
                          double shrinkage, double alpha,
                          double beta, int32_t normalize, int64_t n_threads,
                          int64_t max_chunk_size, int32_t device,
                          irs_knn_computer **out);
/* tf_idf_weight(X, smooth) / okapi_BM_25_weight(X, k1, b) on their own (util.hpp:159-209, bound at
 * util.cpp:29-32): X is CSR float64 [rows, cols]; `out` (caller-allocated, nnz doubles) receives the
 * weighted values in X's entry order (X's pattern is unchanged).  Column counts, row sums and the
 * idf table (libm's log) are made on host threads, the per-entry pass runs on the device
 * (knn_weight_kernel: one IEEE multiply for tf-idf; multiply, multiply, add, divide for BM25, each
 * rounded once - the host loop's values bit for bit). */
irs_status irs_knn_weight(int32_t weighting, int64_t rows, int64_t cols,
                          const int64_t *indptr, const int32_t *indices,
                          const double *data, double k1, double b, int32_t smooth,
                          int32_t device, double *out);
irs_status irs_knn_destroy(irs_knn_computer *c);
/* compute_similarity(X, top_k) (knn.hpp:43-139) / compute_W (similarities.hpp:
 * 224-240, 294-324; as_w != 0, result still row-major [rows, N]).  Two calls:
 * compute runs the device work and reports nnz; fetch copies the CSR out (from a
 * page-locked copy the compute call made while its later row chunks were still
 * running, or from the device).  The caller's arrays are read in place, never
 * written.  `layout` (IRS_LAYOUT_*): how the arrays store the [rows, cols] target - knn.py:79 passes
 * `X_train_all.T`, a CSC matrix; its columns are regrouped into rows on host threads inside the call (indices
 * only when every value is 1).  row_begin/row_end select a shard of target rows (multi-GPU: rows are
 * independent, no collective). */
irs_status irs_knn_compute(irs_knn_computer *c, int64_t rows, int64_t cols,
                           const int64_t *indptr, const int32_t *indices,
                           const double *data, int32_t layout, int64_t top_k, int32_t as_w,
                           int64_t row_begin, int64_t row_end, int64_t *nnz_out);
irs_status irs_knn_fetch(irs_knn_computer *c, int64_t *indptr, int32_t *indices,
                         double *data);
/* The last result once more, as the compressed COLUMNS of the [rows of the call, N] matrix (col_ptr
 * int64[N + 1], row numbers relative to the call's first row, ascending in every column) - what
 * `remove_diagonal(result).tocsc()` of irspack/recommenders/knn.py:78-80 builds on the host (util.hpp:211-226
 * + scipy's conversion, ~50 ms for the ML-20M result), regrouped on the device instead.
 * zero_diagonal_row0 >= 0: the stored entries whose column equals zero_diagonal_row0 + their row are set to
 * 0.0 and KEPT (remove_diagonal; pass the call's row_begin, 0 for a whole matrix); < 0: values unchanged. */
irs_status irs_knn_fetch_csc(irs_knn_computer *c, int64_t zero_diagonal_row0, int64_t *col_ptr,
                             int32_t *row_idx, double *data);
/* Measurement only: multiply-adds of the last call that were added one by one, and the rows of the
 * dense block of the popular items - an opt-in of rounds 4 - 5 that was removed: every multiply-add is
 * added one by one and dense_rows is 0 (kept for ABI 3). */
irs_status irs_knn_last_walked(irs_knn_computer *c, int64_t *walked_macs, int32_t *dense_rows);
/* Milliseconds of device time of the last irs_knn_compute (HIP events: first launch to last row merge of
 * the call's row chunks) and the number of multiply-adds it performed. */
irs_status irs_knn_last_stats(irs_knn_computer *c, double *kernel_ms,
                              int64_t *macs);
/* remove_diagonal, cpp_source/util.hpp:211-226 (in place on `data`). */
irs_status irs_remove_diagonal(int64_t rows, int64_t cols, const int64_t *indptr,
                               const int32_t *indices, double *data);
/* retrieve_recommend_from_score_{f32,f64}, cpp_source/util.hpp:426-504 (bound at
 * util.cpp; caller utils/id_mapping.py:29-44, 312-317): top-`cutoff` candidates of every
 * score row, best first, stopping at -inf.  scores: host row-major [rows, n_items], float32
 * (is_f64 == 0) or float64.  Allowed lists are ragged (list_ptr int64[n_lists + 1],
 * list_items int64; n_lists in {0, 1, rows}); ids outside [0, n_items) are dropped, order
 * and duplicates are kept.  out_idx: int32 [rows, cutoff], -1 padded; the caller reads the
 * scores of the winners from its own array.  Equal scores come out in candidate order (the
 * reference's comparator leaves their order unspecified, util.hpp:483-485). */
irs_status irs_retrieve_recommend(int32_t is_f64, const void *scores, int64_t rows,
                                  int64_t n_items, int64_t n_lists, const int64_t *list_ptr,
                                  const int64_t *list_items, int64_t cutoff,
                                  int64_t n_threads, int32_t device, int32_t *out_idx);

/* ------------------------------------------------------------------ evaluator
 * cpp_source/evaluator.cpp:441-484 */
typedef struct irs_evaluator irs_evaluator;

/* Metrics accumulator state (evaluator.cpp:168-178): the caller owns
 * item_cnt[n_items]. */
typedef struct irs_metrics {
  uint64_t valid_user;
  uint64_t total_user;
  double hit, recall, ndcg, precision, map;
} irs_metrics;

/* EvaluatorCore(ground_truth, recommendable): evaluator.cpp:183-206.
 * Recommendable lists are ragged: rec_ptr int64[n_lists+1], rec_items int64. */
irs_status irs_eval_create(int64_t n_users, int64_t n_items,
                           const int64_t *indptr, const int32_t *indices,
                           int64_t n_lists, const int64_t *rec_ptr,
                           const int64_t *rec_items, int32_t device,
                           irs_evaluator **out);
irs_status irs_eval_destroy(irs_evaluator *e);
/* get_metrics_f32 / get_metrics_f64: evaluator.cpp:256-284 (+ :292-367,
 * Metrics::update :127-166).  scores is a host row-major [rows, n_items] block
 * of float32 (is_f64 == 0) or float64. */
irs_status irs_eval_get_metrics(irs_evaluator *e, int32_t is_f64,
                                const void *scores, int64_t rows, int64_t cutoff,
                                int64_t offset, int64_t n_threads,
                                int32_t recall_with_cutoff, irs_metrics *out,
                                int64_t *item_cnt);
/* The caller loop of evaluation/evaluator.py:371-393 (score chunks) and :417-438 (model blocks)
 * for one block, on the device: the host block is uploaded ONCE (the upload is the copy the
 * reference makes at :387, so the caller's array is never written), the stored entries of the
 * mask rows are set to -inf there (:389 / :432; the caller passes the NONZERO entries only:
 * mask_indptr has rows + 1 entries, mask_indices[mask_indptr[r] - mask_indptr[0] ..) are the
 * columns of row r; NULL = no mask) and the block is ranked once per cutoff (:390-391 /
 * :433-439).  out[c] / item_cnt[c * n_items ..] receive the metrics of cutoffs[c]. */
irs_status irs_eval_get_metrics_masked(irs_evaluator *e, int32_t is_f64, const void *scores,
                                       int64_t rows, const int64_t *mask_indptr,
                                       const int32_t *mask_indices, int32_t n_cutoffs,
                                       const int64_t *cutoffs, int64_t offset,
                                       int64_t n_threads, int32_t recall_with_cutoff,
                                       irs_metrics *out, int64_t *item_cnt);
/* Evaluator.get_score(model) for a SIMILARITY model (evaluation/evaluator.py:400-441 with
 * BaseSimilarityRecommender.get_score_block, recommenders/base.py:406-429: score = X_train[u] @ W), without
 * the host in the loop: users begin .. end of the model are scored on the device - x_* are the profiles
 * X [n_model_users, n_profile_cols] as CSR float64, w_* is W [n_profile_cols, n_items] BY ROWS (CSR): the
 * training matrix and the learnt item-item weights for item-kNN / P3alpha / RP3beta, the learnt user-user
 * weights and the training matrix for user-kNN (base.py:432-453) - with the per-entry order and rounding of
 * scipy's row-by-row sparse product (the block is the host product bit for bit), masked (mask_* as in irs_eval_get_metrics_masked: the rows begin .. end only, NULL = no mask) and
 * ranked once per cutoff; out[c] / item_cnt[c * n_items ..] receive the metrics of cutoffs[c].  `offset`:
 * ground-truth row of user `begin`. */
irs_status irs_eval_get_metrics_similarity(irs_evaluator *e, int64_t begin, int64_t end,
                                           int64_t n_model_users, int64_t n_profile_cols,
                                           const int64_t *x_indptr,
                                           const int32_t *x_indices, const double *x_data,
                                           const int64_t *w_indptr, const int32_t *w_indices,
                                           const double *w_data, const int64_t *mask_indptr,
                                           const int32_t *mask_indices, int32_t n_cutoffs,
                                           const int64_t *cutoffs, int64_t offset,
                                           int32_t recall_with_cutoff, irs_metrics *out,
                                           int64_t *item_cnt);
/* The same for a similarity model whose weights are a DENSE array (DenseSLIM / EASE, EDLAE): x_* are the
 * profiles X [n_model_users, n_profile_cols] as CSR float64, read in their STORAGE order (the rows need not be
 * sorted and are not copied into another order), w is W [n_profile_cols, n_items] row-major, float32
 * (w_is_f64 == 0) or float64, uploaded once per call and not kept.  Per (user, column) the score is the chain
 * acc = acc + x * (double)w over the user's stored entries, product and sum rounded separately: scipy's
 * `X[b:e].dot(W)` (csr_matvecs) bit for bit.  Mask, cutoffs, offset and outputs as in
 * irs_eval_get_metrics_similarity. */
irs_status irs_eval_get_metrics_dense_similarity(irs_evaluator *e, int64_t begin, int64_t end,
                                                 int64_t n_model_users, int64_t n_profile_cols,
                                                 const int64_t *x_indptr, const int32_t *x_indices,
                                                 const double *x_data, int32_t w_is_f64, const void *w,
                                                 const int64_t *mask_indptr, const int32_t *mask_indices,
                                                 int32_t n_cutoffs, const int64_t *cutoffs, int64_t offset,
                                                 int32_t recall_with_cutoff, irs_metrics *out,
                                                 int64_t *item_cnt);
/* The same for a FACTOR model (truncated SVD, NMF): score = user_factors[u] @ item_factors^T in float32
 * through the fp32 MFMA tiles of the iALS scores (operands zero-padded to a multiple of 32 on upload), for the
 * users begin .. end of user_factors [n_model_users, k] against item_factors [n_items, k], both host
 * row-major, 1 <= k <= 576; masked and ranked once per cutoff as above. */
irs_status irs_eval_get_metrics_factors(irs_evaluator *e, int64_t begin, int64_t end,
                                        int64_t n_model_users, int32_t k, const float *user_factors,
                                        const float *item_factors, const int64_t *mask_indptr,
                                        const int32_t *mask_indices, int32_t n_cutoffs,
                                        const int64_t *cutoffs, int64_t offset,
                                        int32_t recall_with_cutoff, irs_metrics *out, int64_t *item_cnt);
/* The three model calls for a model that scores fewer columns than the evaluator ranks (EvaluatorWithColdUser with
 * feature-only items behind the training items, evaluator.py:623-634): the item operand covers the leading
 * n_scored columns, 1 <= n_scored <= n_items - w_* / w is W [n_profile_cols, n_scored], item_factors is
 * [n_scored, k] - the scores go to those columns of a block whose rows stay n_items wide, and the columns
 * n_scored .. n_items hold -inf before the block is masked and ranked, so they are never recommended.  With
 * n_scored == n_items these are the calls above.  `running` of the factor call (NULL, or one irs_metrics per
 * cutoff): the sums of the users that earlier calls covered; the call merges its 128-user chunks onto them and
 * returns the continued sums in out[c], so users handed over in several calls of whole chunks (a fold-in per
 * call) are summed as one call sums them.  item_cnt is this call's alone. */
irs_status irs_eval_get_metrics_similarity_scored(irs_evaluator *e, int64_t begin, int64_t end,
                                                  int64_t n_model_users, int64_t n_profile_cols,
                                                  const int64_t *x_indptr, const int32_t *x_indices,
                                                  const double *x_data, const int64_t *w_indptr,
                                                  const int32_t *w_indices, const double *w_data,
                                                  int64_t n_scored, const int64_t *mask_indptr,
                                                  const int32_t *mask_indices, int32_t n_cutoffs,
                                                  const int64_t *cutoffs, int64_t offset,
                                                  int32_t recall_with_cutoff, irs_metrics *out,
                                                  int64_t *item_cnt);
irs_status irs_eval_get_metrics_dense_similarity_scored(irs_evaluator *e, int64_t begin, int64_t end,
                                                        int64_t n_model_users, int64_t n_profile_cols,
                                                        const int64_t *x_indptr, const int32_t *x_indices,
                                                        const double *x_data, int32_t w_is_f64, const void *w,
                                                        int64_t n_scored, const int64_t *mask_indptr,
                                                        const int32_t *mask_indices, int32_t n_cutoffs,
                                                        const int64_t *cutoffs, int64_t offset,
                                                        int32_t recall_with_cutoff, irs_metrics *out,
                                                        int64_t *item_cnt);
irs_status irs_eval_get_metrics_factors_scored(irs_evaluator *e, int64_t begin, int64_t end,
                                               int64_t n_model_users, int32_t k, const float *user_factors,
                                               const float *item_factors, int64_t n_scored,
                                               const irs_metrics *running, const int64_t *mask_indptr,
                                               const int32_t *mask_indices, int32_t n_cutoffs,
                                               const int64_t *cutoffs, int64_t offset,
                                               int32_t recall_with_cutoff, irs_metrics *out, int64_t *item_cnt);
/* Stream time of the last irs_eval_get_metrics_dense_similarity / _factors call by phase, in milliseconds
 * (measurement only): ms[0] uploads, ms[1] scoring, ms[2] masking, ms[3] ranking and folding. */
irs_status irs_eval_last_phases(irs_evaluator *e, double *ms);
/* Fused device path used by the Evaluator counterpart when the model is an
 * iALS trainer of this library: scores = user[begin:end] @ item^T (hpp:942-984)
 * are produced, masked (evaluator.py:417-432, mask = CSR rows given here, set
 * to -inf) and ranked on the device without leaving HBM.  mask_indptr may be
 * NULL (no mask, or the mask cached by irs_eval_cache_mask); it has rows+1 entries
 * relative to `begin`. */
irs_status irs_eval_get_metrics_ials(irs_evaluator *e, irs_ials_trainer *t,
                                     int64_t begin, int64_t end,
                                     const int64_t *mask_indptr,
                                     const int32_t *mask_indices, int64_t cutoff,
                                     int64_t offset, int32_t recall_with_cutoff,
                                     irs_metrics *out, int64_t *item_cnt);
/* Keeps the mask of the fused path on the device between calls: the same CSR rows
 * irs_eval_get_metrics_ials takes (rows + 1 entries of indptr relative to its `begin`).
 * While a mask of `rows` rows is cached, a call of irs_eval_get_metrics_ials over that many
 * users with mask_indptr == NULL applies it; rows <= 0 or mask_indptr == NULL drops it. */
irs_status irs_eval_cache_mask(irs_evaluator *e, int64_t rows, const int64_t *mask_indptr,
                               const int32_t *mask_indices);

/* 64-bit content fingerprint of a host buffer, computed on several host threads: the check that the
 * device-resident mask of irs_eval_cache_mask is still the caller's matrix (every byte, every call;
 * no reference counterpart).  Not cryptographic. */
irs_status irs_fingerprint(const void *data, int64_t n_bytes, uint64_t seed, uint64_t *out);

/* What the last irs_eval_get_metrics_ials call did (measurement only, no reference
 * counterpart).  path: 0 = score block + ranking (two passes), 1 = threshold-filtered
 * candidates, 2 = threshold-filtered with norm-bound pruning (3, a single-pass variant, was removed in ABI 3's round). */
typedef struct irs_eval_stats {
  int32_t path;
  int32_t hard_rows;    /* rows ranked from their full score row after the filtered pass */
  int64_t tiles_total;  /* 64 x 64 score tiles of the user block */
  int64_t tiles_scored; /* tiles the scoring kernel computed (= tiles_total unless pruned) */
  int64_t sample_items; /* items of the threshold sample pass (0: none) */
  double call_ms;        /* host clock around the whole C call (mask upload, launches, read-back) */
  double device_span_ms; /* HIP events on the launch stream: first kernel of the call -> last one done
                          * (includes the gaps in which the host reads the hard-row list back) */
} irs_eval_stats;
irs_status irs_eval_last_stats(irs_evaluator *e, irs_eval_stats *out);

/* ------------------------------------------------------------------ SLIM
 * slim_weight_positive_only / slim_weight_allow_negative of irspack.utils._util_cpp
 * (cpp_source/util.cpp:31-40, the coordinate descent of cpp_source/util.hpp:228-424; the caller is
 * src/irspack/recommenders/slim.py).  For every target item j, by cyclic coordinate descent from w = 0
 * on the item Gram matrix G = X^T X (dense fp32 on the device):
 *     min_w  1/2 |x_j - X w|^2 + l2/2 |w|^2 + l1 |w|_1,   w_j = 0   [w >= 0 when positive_only]
 * with the update of util.hpp:300-345, at most n_iter sweeps, a column stopping after the first sweep
 * whose largest coefficient change is < tol (util.hpp:346-351, here per column, the reference per SIMD
 * block of columns).  Where the reference is not a function of its arguments this library is: the
 * coordinate order of every sweep is the ascending one (the reference shuffles with a per-thread
 * generator shared by the blocks a thread happens to fetch, util.hpp:251,293), so the result is
 * bit-identical from call to call; a coordinate with G_ff + l2 == 0 keeps the coefficient 0.
 * top_k >= 0: a column with more non-zeros keeps its top_k largest VALUES (not magnitudes,
 * util.hpp:383-392; ties: the lower row index); top_k < 0: no limit.
 * X is CSR float32 [rows, cols], validated on the host: monotone indptr, column indices in range and
 * strictly ascending within a row - a duplicate column index is IRS_INVALID_ARGUMENT, not summed.
 * Argument checks and messages: util.hpp:233-236 (n_iter > 0, l2_coeff >= 0, l1_coeff >= 0); they come
 * before any device work.  IRS_RUNTIME_ERROR when 8 cols^2 bytes (G and the dense coefficients) plus
 * working space exceed the free device memory.
 * The result [cols, cols] is held by the handle as CSC: col_ptr int64[cols + 1], indices (rows, ascending)
 * int32[nnz], data float32[nnz]; no stored zeros, empty diagonal.  The fetch arrays are caller-owned
 * (sizes from the nnz call). */
typedef struct irs_slim_result irs_slim_result;
irs_status irs_slim_fit(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices,
                        const float *data, int32_t positive_only, int64_t n_iter, float l2_coeff,
                        float l1_coeff, float tol, int64_t top_k, int32_t device,
                        irs_slim_result **out);
irs_status irs_slim_nnz(irs_slim_result *r, int64_t *nnz);
irs_status irs_slim_fetch(irs_slim_result *r, int64_t *col_ptr, int32_t *indices, float *data);
/* Measurement only: device milliseconds (HIP events) of the three phases - Gram matrix (with the upload
 * and the transpose), descent, emit - the sweeps run summed over the columns, and the coordinate
 * changes applied (one axpy over a column of G each).  Any pointer may be NULL. */
irs_status irs_slim_last_stats(irs_slim_result *r, double *gram_ms, double *descent_ms,
                               double *emit_ms, int64_t *sweeps_total, int64_t *updates_total);
/* Measurement only: the launch of the descent kernel in the call that produced the result.  lds_r: 1 when
 * the running vector of a column lived in LDS, 0 when in a global scratch row per workgroup; lds_bytes: the
 * dynamic LDS of the launch (400 + 4 cols, or the 400 bytes of slots alone); threads: the workgroup size,
 * which is the width of a chunk (256 up to 40 KiB of LDS, 512 up to 80 KiB, 1024 above); n_wg: the
 * persistent workgroups; raise_dynamic_lds: 1 when the launch needed the kernel's dynamic-LDS limit raised
 * (above 64 KiB); lds_per_block: the per-block LDS limit the device reported (the vector is in LDS while
 * 400 + 4 cols is at most that and IRSPACK_AMD_SLIM_LDS is not 0).  All 0 after a call that did no device
 * work (no columns or no entries).  Any pointer may be NULL. */
irs_status irs_slim_last_launch(irs_slim_result *r, int32_t *lds_r, int32_t *lds_bytes, int32_t *threads,
                                int32_t *n_wg, int32_t *raise_dynamic_lds, int64_t *lds_per_block);
irs_status irs_slim_destroy(irs_slim_result *r);

/* ------------------------------------------------------------------ row-wise hold-out split
 * rowwise_train_test_split_by_ratio / _by_fixed_n of irspack.utils._util_cpp (SplitFunction,
 * cpp_source/util.hpp:72-156): every row of X is split into a train and a test (held-out) part, on the device.
 * The reference's result depends on libstdc++'s std::shuffle; this library has a rule of its own (normative text:
 * irspack_amd/csrc/split_host_plan.hpp), a function of the arguments alone:
 *   every stored entry takes part (explicit zeros too); j = position of an entry in its row, m = the row's length;
 *   n_test(m) = floor or ceil of double(m) * heldout_ratio, computed in double (mode IRS_SPLIT_BY_RATIO), or
 *               min(m, n_held_out) (mode IRS_SPLIT_BY_FIXED_N) - util.hpp:127-150;
 *   row_key = mix64(mix64(seed) ^ mix64(row + 0x53504C4954)), key(j) = mix64(row_key ^ mix64(j)), mix64 being the
 *   finaliser of splitmix64; held out are the n_test smallest pairs (key(j), j) of the row.
 * X is CSR [rows, cols]: indptr int64, indices int32, data opaque elements of elem_bytes = 1, 2, 4 or 8 bytes, which
 * are moved and never converted.  Validated on the host before any device work (IRS_INVALID_ARGUMENT): monotone
 * indptr, column indices in range and strictly ascending within a row (duplicates are not summed), the element
 * width, 0 <= heldout_ratio <= 1 (the reference's message), n_held_out >= 0, the mode.  Zero rows or zero stored
 * entries succeed with empty outputs and without a device.
 * Both results have X's shape and keep the column order inside a row; the handle holds them on the host.  The fetch
 * arrays are caller-owned: indptr int64[rows + 1], indices int32[nnz], data elem_bytes * nnz bytes each (sizes from
 * the nnz call; the pointers of a matrix without entries may be NULL). */
#define IRS_SPLIT_BY_RATIO 0
#define IRS_SPLIT_BY_FIXED_N 1
typedef struct irs_split_result irs_split_result;
typedef struct {
  double upload_ms;    /* HIP events: the matrix and the row lists to the device */
  double select_ms;    /* the threshold key of every row with 0 < n_test < m */
  double scan_ms;      /* the two row-pointer arrays */
  double scatter_ms;   /* flags and the ordered compaction into both outputs */
  double d2h_ms;       /* the copy back into the handle */
  int64_t rows_empty;  /* rows per class: no entries, */
  int64_t rows_wave;   /* 1 .. 64 entries (a wave per row), */
  int64_t rows_lds;    /* 65 .. 4096 (a workgroup per row, keys in LDS), */
  int64_t rows_stream; /* longer (a workgroup per row, keys recomputed per pass) */
} irs_split_stats;
irs_status irs_split_rowwise(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices,
                             const void *data, int32_t elem_bytes, int64_t random_seed, int32_t mode,
                             double heldout_ratio, int32_t n_test_ceil, int64_t n_held_out, int32_t device,
                             irs_split_result **out);
irs_status irs_split_nnz(irs_split_result *r, int64_t *nnz_train, int64_t *nnz_test);
irs_status irs_split_fetch(irs_split_result *r, int64_t *train_indptr, int32_t *train_indices, void *train_data,
                           int64_t *test_indptr, int32_t *test_indices, void *test_data);
/* Measurement only: the phase times and the rows per class of the call that produced the result. */
irs_status irs_split_last_stats(irs_split_result *r, irs_split_stats *stats);
irs_status irs_split_destroy(irs_split_result *r);

/* ------------------------------------------------------------------ EASE / EDLAE
 * DenseSLIMRecommender (src/irspack/recommenders/dense_slim.py:39-53) and EDLAERecommender
 * (edlae.py:49-66): the closed-form item-item weights, float32 throughout, on the device:
 *     G = X^T X,   P = G + diag(lam),  lam_j = diag_scale * G_jj + reg   (each operation rounded to
 *     float32, no fused multiply-add: numpy's evaluation order),   B = P^-1,
 *     W_ij = -B_ij / B_jj (i != j),  W_jj = 0.
 * EASE passes diag_scale = 0, EDLAE float32(dropout_p / (1 - dropout_p)).  P is padded to a multiple of
 * 64 with identity rows, factored P = L L^T (blocked fp32 MFMA Cholesky), inverted from the factor
 * (L^-1, then B = L^-T L^-1 for the lower triangle) and finalized into W [cols, cols] row-major, which
 * is caller-owned and written by one device-to-host copy.  Two calls give identical bytes.
 * The matrix checks are irs_slim_fit's (IRS_INVALID_ARGUMENT, before any device work).  An empty matrix
 * with reg > 0 gives W = 0 without device work.  IRS_RUNTIME_ERROR: 8 n_pad^2 bytes plus the matrix twice
 * exceed the free device memory; or P is not positive definite (a pivot that is not > 0 or not finite;
 * the message holds "not positive definite" and the first failing column) - W is then not written.
 * Unlike the reference's LU inverse, an indefinite but non-singular P is an error. */
typedef struct {
  double gram_ms;     /* HIP events: upload, transpose, X^T X, diagonal */
  double factor_ms;   /* P = L L^T */
  double invert_ms;   /* L^-1 and B = L^-T L^-1 */
  double finalize_ms; /* W from B */
  double d2h_ms;      /* the copy into the caller's array */
  int64_t n_pad;      /* padded order: cols rounded up to 64 */
} irs_dense_slim_stats;
irs_status irs_dense_slim_fit(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices,
                              const float *data, float reg, float diag_scale, int32_t device, float *W,
                              irs_dense_slim_stats *stats /* may be NULL */);

/* ------------------------------------------------------------------ truncated SVD
 * TruncatedSVDRecommender (src/irspack/recommenders/truncsvd.py: sklearn's randomized TruncatedSVD) - the
 * device side of irspack_amd.utils.truncated_svd, float32.  A = X when n_users >= n_items, else X^T
 * (sklearn's transpose="auto"): m x n with m >= n.  The handle keeps A, A^T and three m x l_pad blocks on the
 * device (l_pad: the sketch width rounded up to 64, at most 576); the l x l symmetric eigenproblems between
 * the calls are the caller's (float64 on the host).  One stream; one synchronisation per call, except that
 * the first range call also sets the matrix up (blocking copies, the device transpose's synchronisation).  No
 * float atomics, every sum has a fixed order: two runs give identical bytes.
 *   create   validates X (CSR float32; the checks of irs_slim_fit, and every value finite) and keeps a copy;
 *            the matrix reaches the device with the first range call, so every argument check of every call
 *            comes before any device work (IRS_INVALID_ARGUMENT).
 *   range    omega [rows, l] row-major is the Gaussian test matrix, rows == n (n_items when
 *            n_users >= n_items, else n_users), 1 <= l <= min(n_users, n_items, 576).  Q = omega; n_iter times
 *            { Y = A Q, normalise; Q = A^T Y, normalise }; Y = A Q.  Normalise: G = Y^T Y, Cholesky of
 *            G + d I with d = 1e-5 trace(G) / l, Y <- Y L^-T.  gram_out [l, l] receives Y^T Y.
 *   apply    Y <- Y m for m [l, l2] row-major, 1 <= l2 <= l; l becomes l2; gram_out [l2, l2] = Y^T Y.
 *   project  Q = A^T Y (B^T for B = Y^T A); gram_out [l, l] = B B^T.
 *   finish   rot [l, k] row-major, 1 <= k <= l: V = Q rot (A = X) or Y rot (A = X^T), the n_items x k side;
 *            z = X V by one more product; every component's entry of largest magnitude is made positive
 *            (sklearn's svd_flip on the rows of components_).  z_out [n_users, k], components_out [k, n_items].
 * IRS_RUNTIME_ERROR: no device, not enough device memory, or a block whose Gram matrix has no Cholesky
 * factor (a zero matrix; overflow). */
typedef struct irs_truncsvd irs_truncsvd;
typedef struct {
  double setup_ms; /* HIP events, summed over the calls so far: upload, transpose, segment lists */
  double spmm_ms;  /* the sparse x block products */
  double gram_ms;  /* the Gram matrices of the blocks */
  double chol_ms;  /* shift, Cholesky and triangular inverse of the l_pad x l_pad matrices */
  double apply_ms; /* block x small-matrix products */
  double d2h_ms;   /* copies into the caller's arrays */
  double host_ms;  /* finish: signs and the transpose of the components on the host (host clock) */
  int64_t n_spmm;  /* sparse x block products so far */
  int64_t l_pad;
} irs_truncsvd_stats_t;
irs_status irs_truncsvd_create(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                               const float *data, int32_t device, irs_truncsvd **out);
irs_status irs_truncsvd_range(irs_truncsvd *t, const float *omega, int64_t rows, int64_t l, int64_t n_iter,
                              float *gram_out);
irs_status irs_truncsvd_apply(irs_truncsvd *t, const float *m, int64_t l2, float *gram_out);
irs_status irs_truncsvd_project(irs_truncsvd *t, float *gram_out);
irs_status irs_truncsvd_finish(irs_truncsvd *t, const float *rot, int64_t k, float *z_out, float *components_out);
irs_status irs_truncsvd_stats(irs_truncsvd *t, irs_truncsvd_stats_t *out);
irs_status irs_truncsvd_destroy(irs_truncsvd *t);
/* The fold-in of rows the fit has not seen (TruncatedSVD.transform: z = X @ components_^T), stateless: X is CSR
 * [rows, n_items] (float32, sorted, no duplicates, finite), item_factors the table components_^T [n_items, k]
 * row-major, 1 <= k <= 576, out [rows, k].  One sparse x block product with the row sums in double; every element
 * is rounded to float32 once, also in a row long enough to be split.  The sums have a fixed order: the result is
 * a function of the arguments, identical from call to call. */
irs_status irs_truncsvd_transform(int64_t rows, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                                  const float *data, int64_t k, const float *item_factors, int32_t device,
                                  float *out);

/* ------------------------------------------------------------------ NMF
 * NMFRecommender (src/irspack/recommenders/nmf.py: sklearn.decomposition.NMF, solver "cd", Frobenius loss,
 * shuffle off) - the device side of irspack_amd.utils.nmf_fit / nmf_transform, float32.  X is CSR (float32,
 * sorted, no duplicates, non-negative); W [n_users, k] and H [k, n_items] row-major hold the initial factors and
 * receive the result (update_H = 0: H is read only, only W is fitted - sklearn's transform).  One iteration:
 *     half(X, W, H^T, l1_W, l2_W), then, when update_H, half(X^T, H^T, W, l1_H, l2_H);
 *     half(A, W, Ht, l1, l2):  G = Ht^T Ht, G[t, t] += l2;  XH = A Ht - l1;  for t = 0 .. k-1, every row i:
 *         grad = sum_r G[t, r] W[i, r] - XH[i, t];  violation += W[i, t] == 0 ? |min(0, grad)| : |grad|;
 *         if G[t, t] != 0: W[i, t] = max(W[i, t] - grad / G[t, t], 0)
 * XH and G are summed in double and stored as float32; the violation is summed in double in a fixed order.  The loop stops when the first iteration's violation is 0,
 * after the iteration whose violation / the first one's <= tol, or after max_iter iterations; n_iter receives
 * the count, violations (NULL or double[max_iter]) the per-iteration sums.  No float atomics: two calls give
 * identical bytes.  IRS_INVALID_ARGUMENT before any device work: the matrix checks of irs_truncsvd_create, a
 * negative value, k < 1 or k > 576, max_iter < 1, tol < 0, a negative or non-finite regulariser, a non-finite or
 * negative entry of the initial W or H.  IRS_RUNTIME_ERROR: no device, not enough device memory. */
typedef struct {
  double setup_ms; /* HIP events: upload, transpose, segment lists, the initial factors */
  double spmm_ms;  /* the sparse x block products */
  double gram_ms;  /* the k x k Gram matrices */
  double sweep_ms; /* the coordinate sweeps */
  double d2h_ms;   /* the violation reduce and its copy per iteration, the factors at the end */
} irs_nmf_stats_t;
irs_status irs_nmf_fit(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                       const float *data, int64_t k, float *W, float *H, float l1_W, float l2_W, float l1_H,
                       float l2_H, double tol, int64_t max_iter, int32_t update_H, int32_t device, int64_t *n_iter,
                       double *violations /* may be NULL */, irs_nmf_stats_t *stats /* may be NULL */);

/* ------------------------------------------------------------------ BPR
 * BPRFMRecommender (src/irspack/recommenders/bpr.py wraps LightFM; the arithmetic here is this library's own
 * synchronous mini-batch form of LightFM's per-sample step - BPR loss, Adagrad, item biases, no user bias -
 * DESIGN.md section 14).  State, all float32: U [n_users, k], V [n_items, k], item bias b [n_items], the Adagrad
 * accumulators GU, GV, Gb of the same shapes (1 at the start) and an epoch counter.  Without initial tables U and V
 * are uniform in (-0.5, 0.5) / k from `seed` through the library's counter-based generator, b = 0.
 * Positives: the stored entries of X (CSR float32) with value > 0; the values are not used otherwise.
 *   epoch    every positive of a user with an unseen item once, in an order that depends on (seed, epoch) alone
 *            (a keyed Feistel permutation of the positions); the negative of a position is uniform over the items
 *            its user has no positive on - the r-th unseen item by a binary search in the user's row, r from the
 *            generator at (seed, epoch, position), no rejection loop.  A user with a positive on every item has no
 *            negative: its positives are skipped and counted.
 *   batch    batch_size consecutive triples (u, i, j) of that order (the last batch of an epoch may be shorter),
 *            synchronous - every triple reads the parameters as the batch found them:
 *              x = U[u].(V[i] - V[j]) + b[i] - b[j],  w = 1 / (1 + exp(x))
 *              gU[u] -= w (V[i] - V[j]);  gV[i] -= w U[u];  gV[j] += w U[u];  gb[i] -= w;  gb[j] += w
 *            summed over the batch per row; every row the batch touched then gets gU[r] += user_alpha U[r]
 *            (gV, gb: item_alpha) once, and theta -= learning_rate g / sqrt(G), G += g^2 element by element (G is
 *            read before it is updated).  Untouched rows keep their bytes.
 * The per-row sums are 64-bit fixed-point integers (scale 2^s, s from the batch length: irs_bpr_stats) added with
 * integer atomics, so they do not depend on the order of arrival: two runs give identical bytes.  The scale assumes
 * |theta| < 2^8 for every parameter; a call after which one is not (or is not finite) returns IRS_RUNTIME_ERROR and
 * the state is lost.
 *   create        validates and keeps the arguments; the device is first used by the first other call that needs
 *                 it, so every argument check of every call comes before any device work.
 *   run_epochs    n_epochs epochs from the current state and epoch counter: per batch three launches on one
 *                 stream, no copy and no synchronisation inside an epoch.
 *   sample        the triples run_epochs uses at positions [first, first + count) of `epoch` (the same kernel), into
 *                 users / pos / neg; 0 <= first, first + count <= n_positives - n_skipped_positives.
 *   step_triples  ONE synchronous batch on the caller's n triples through the kernels of an epoch (the epoch
 *                 counter stays); a triple's rows need not be related by X.
 *   get_state     any of the six arrays and epoch may be NULL.  set_state replaces all of them.
 * IRS_INVALID_ARGUMENT before any device work: the matrix checks of irs_truncsvd_create (unsorted or duplicate
 * indices within a row among them), k < 1 or k > 512, batch_size < 1, a negative or non-finite alpha or
 * learning_rate, learning_rate == 0, a non-finite entry (or one of magnitude >= 2^8) in the initial tables or in a
 * state being set, an accumulator <= 0 in a state being set, a triple out of range in step_triples.
 * IRS_RUNTIME_ERROR: no device, not enough device memory, a diverged fit.  One handle is used by one thread at a
 * time. */
typedef struct irs_bpr irs_bpr;
typedef struct {
  int64_t n_positives;         /* stored entries > 0 */
  int64_t n_skipped_full_rows; /* users with a positive on every item ... */
  int64_t n_skipped_positives; /* ... and their positives, which no epoch uses */
  int64_t batches_per_epoch;
  int32_t lanes_per_triple;    /* of the gradient and apply kernels at this k */
  int32_t scale_log2;          /* s of a full batch */
  double epoch_ms;             /* HIP events round the last epoch run_epochs ran */
  double sample_ms;            /* that epoch by phase, collected only with IRSPACK_AMD_BPR_PHASES=1 in the */
  double grad_ms;              /* environment when the handle is made (two more events per launch), else 0 */
  double apply_ms;
} irs_bpr_stats_t;
irs_status irs_bpr_create(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                          const float *data, int32_t k, float user_alpha, float item_alpha, float learning_rate,
                          int64_t batch_size, uint64_t seed, const float *user_init /* may be NULL */,
                          const float *item_init /* may be NULL */, int32_t device, irs_bpr **out);
irs_status irs_bpr_run_epochs(irs_bpr *t, int64_t n_epochs);
irs_status irs_bpr_sample(irs_bpr *t, int64_t epoch, int64_t first, int64_t count, int32_t *users, int32_t *pos,
                          int32_t *neg);
irs_status irs_bpr_step_triples(irs_bpr *t, int64_t n, const int32_t *users, const int32_t *pos, const int32_t *neg);
irs_status irs_bpr_get_state(irs_bpr *t, float *U, float *V, float *b, float *GU, float *GV, float *Gb,
                             int64_t *epoch);
irs_status irs_bpr_set_state(irs_bpr *t, const float *U, const float *V, const float *b, const float *GU,
                             const float *GV, const float *Gb, int64_t epoch);
irs_status irs_bpr_stats(irs_bpr *t, irs_bpr_stats_t *out);
irs_status irs_bpr_destroy(irs_bpr *t);

/* The WARP loss on the same handle type ("WARP"; the project's own synchronous form, not
 * LightFM bit parity).  State, start, positives, position space and the order of an epoch are those of the BPR
 * handle: position p of epoch e is the (u, i) that a handle of irs_bpr_create with the same seed gives.
 *   candidates  candidate t (1 <= t <= max_sampled <= 256) of position p is the r-th item its user has no positive
 *               on, r from one hash of (seed, epoch, p * 256 + t) under a key of the epoch of its own; it does not
 *               depend on max_sampled.
 *   search      every position reads the parameters as the batch found them: x+ = U[u].V[i] + b[i]; for t = 1, 2,
 *               ...: x- = U[u].V[j_t] + b[j_t]; the first t with x- > x+ - 1 ends the search with j = j_t.  A
 *               position without such a t contributes nothing and touches no row.
 *   weight      w_t = min(ln(max(1, floor((n_items - 1) / t))), 10), computed once on the host in double.
 *   update      that of irs_bpr_run_epochs with w_t in place of the sigmoid; L2 term and Adagrad are unchanged.
 *               The fixed-point scale is 2^s, s = 62 - (ceil(log2 n) + 14), at most 40.
 *   create_warp       the arguments of irs_bpr_create and max_sampled.  run_epochs, get_state, set_state, stats and
 *                     destroy work on its handle; irs_bpr_sample and irs_bpr_step_triples return
 *                     IRS_INVALID_ARGUMENT.  The calls below return IRS_INVALID_ARGUMENT on a handle of
 *                     irs_bpr_create.
 *   warp_candidates   positions [first, first + count) of `epoch`: users, pos [count], cand [count, max_sampled].
 *   warp_search       the search on the current state with the caller's candidates (cand [n, max_sampled]);
 *                     nothing is updated.  neg_out [n]: j, or -1 without a violation; tries_out [n]: the
 *                     candidates examined (max_sampled without a violation).
 *   warp_step         one synchronous batch on the caller's positions and candidates.
 *   warp_stats        see the struct.
 * IRS_INVALID_ARGUMENT, before any device work: max_sampled outside [1, 256], a null array, a user, an item or a
 * candidate out of range, n * max_sampled >= 2^31, a window outside the epoch. */
typedef struct {
  int32_t max_sampled;
  int32_t scale_log2;       /* s of a full batch */
  int32_t in_flight;        /* candidate rows the search gathers at a time (IRSPACK_AMD_WARP_IN_FLIGHT) */
  int32_t reserved;
  int64_t epoch_positions;  /* the last epoch run_epochs ran: its positions, ... */
  int64_t epoch_updates;    /* ... those that found a violation, ... */
  int64_t epoch_tries;      /* ... and the candidates examined, summed */
  int64_t call_positions;   /* the same of the last run_epochs (its last epoch), warp_search or warp_step call */
  int64_t call_updates;
  int64_t call_tries;
  double epoch_ms;          /* as in irs_bpr_stats_t */
  double search_ms;         /* the search-and-gradient launches (IRSPACK_AMD_BPR_PHASES=1), else 0 */
  double apply_ms;
} irs_bpr_warp_stats_t;
irs_status irs_bpr_create_warp(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                               const float *data, int32_t k, float user_alpha, float item_alpha, float learning_rate,
                               int64_t batch_size, uint64_t seed, const float *user_init /* may be NULL */,
                               const float *item_init /* may be NULL */, int32_t device, int32_t max_sampled,
                               irs_bpr **out);
irs_status irs_bpr_warp_candidates(irs_bpr *t, int64_t epoch, int64_t first, int64_t count, int32_t *users,
                                   int32_t *pos, int32_t *cand);
irs_status irs_bpr_warp_search(irs_bpr *t, int64_t n, const int32_t *users, const int32_t *pos, const int32_t *cand,
                               int32_t *neg_out, int32_t *tries_out);
irs_status irs_bpr_warp_step(irs_bpr *t, int64_t n, const int32_t *users, const int32_t *pos, const int32_t *cand);
irs_status irs_bpr_warp_stats(irs_bpr *t, irs_bpr_warp_stats_t *out);

/* ------------------------------------------------------------------ Mult-VAE
 * MultVAERecommender (src/irspack/recommenders/multvae.py; the reference trains with jax / haiku / optax and jax's
 * generator - the trainer here is this library's own statement of the same model).
 * With I = n_items, H = enc_hidden, Hd = dec_hidden, L = dim_z the eight float32 tables are, in this order,
 *   W1 [I, H], b1 [H], W2 [H, 2 L], b2 [2 L], W3 [L, Hd], b3 [Hd], W4 [Hd, I], b4 [I],
 * each with Adam moments m and v of its shape.  Wherever 8 tables are passed they are an array of 8 pointers in
 * that order; a state is an array of 24: the tables, their m, their v.  Initial tables (init == NULL): biases 0,
 * weights truncated normal at +-2 sigma, sigma = 1 / sqrt(fan_in), from the counter-based generator keyed by
 * (seed, table, index).
 *
 * One update on n user rows with raw stored values x (t = updates done before it):
 *   klc = kl_anneal_goal min(1, t / (anneal_end_epoch n_users / minibatch_size))     (run_epochs; step_batch takes it)
 *   xn = x / sqrt(sum x^2 + 1e-8) per row; xd = xn keep / (1 - dropout_p), keep in {0, 1} per stored entry
 *   h1 = tanh(xd W1 + b1); [mu | lv] = h1 W2 + b2; std = exp(lv / 2); z = mu + eps std
 *   h2 = tanh(z W3 + b3); logit = h2 W4 + b4; lsm = logit - logsumexp(logit) per row
 *   loss = mean_rows(-sum_i lsm x) + klc mean_rows(sum 0.5 (-lv + std^2 + mu^2 - 1))
 * then Adam (b1 0.9, b2 0.999, eps 1e-8, bias-corrected, optax's form) with the gradient of loss on every element
 * of every table.  A user without entries takes part (its KL term, and it counts in n); the last batch of an epoch
 * is short.  l2_regularizer is stored and has no effect, as in the reference.  The order of an epoch is a seeded
 * bijection of the users keyed by (seed, epoch); keep is a hash of (seed, update, user, stored position) against
 * dropout_p, eps a Gaussian keyed by (seed, update, user, component).  Evaluation (encode, score): no dropout,
 * z = mu.
 *
 * The gradient of W1 is summed in 64-bit fixed point (scale 2^s, s from the batch length: stats), so the bytes
 * do not depend on the order of arrival; a contribution that is not finite or reaches 2^8 in magnitude makes the
 * call return IRS_RUNTIME_ERROR ("the fit has diverged") and the state is lost.  Every other sum has a fixed
 * order: two runs give identical bytes.
 *
 * create      checks everything and keeps host copies; the device is first used by the first call that computes.
 *             1 <= enc_hidden, dec_hidden <= 574, dim_z >= 1, 0 <= dropout_p < 1, minibatch_size >= 1,
 *             learning_rate > 0, kl_anneal_goal >= 0, anneal_end_epoch >= 0.
 * run_epochs  whole epochs, one synchronisation at the end.
 * order       users [count] of positions [first, first + count) of an epoch (host only).
 * noise       for n users at one update: keep (one byte per stored entry, the rows in the order of `users`) and
 *             eps [n, L], as run_epochs draws them.
 * step_batch  one update on the caller's rows with the caller's keep / eps (NULL: drawn as
 *             run_epochs would at the current update count) and klc; nll and kl (may be NULL) receive the two
 *             means of the loss.  Counts as an update, not as an epoch.
 * gradients   the 8 gradient tables of the last update.
 * get_state / set_state   24 tables (entries of get_state may be NULL), the update and the epoch counter.
 * encode      rows of a CSR matrix of n_items columns -> h2 [rows, Hd] and lse [rows] (either may be NULL), so
 *             that the log-softmax scores are [h2 | 1] [W4; b4] - lse.
 * score       the same rows -> log-softmax [rows, I] float32.
 * IRS_INVALID_ARGUMENT for every argument check (all come before any device work); IRS_RUNTIME_ERROR: no device,
 * not enough device memory for the [batch, I] block, a diverged fit.  One handle is used by one thread at a time. */
typedef struct irs_multvae irs_multvae;
typedef struct {
  int64_t n_updates;         /* updates done */
  int64_t epoch;             /* epochs done */
  int64_t batches_per_epoch; /* ceil(n_users / minibatch_size) */
  int32_t dh2_slab;          /* items per K-slab of dh2 = g W4^T (partials added in slab order) */
  int32_t dw4_slab;          /* batch rows per K-slab of d[W4; b4] = [h2 | 1]^T g */
  int32_t scale_log2;        /* s of the fixed-point scale of a full batch */
  int32_t reserved;
  double klc_next;           /* klc of the next update of run_epochs */
  double klc_last;           /* klc, nll and kl of the last update */
  double nll_last;
  double kl_last;
  double epoch_ms;           /* device time of the last epoch run */
  double encode_ms;          /* that epoch by phase, collected only with IRSPACK_AMD_MULTVAE_PHASES=1 in the */
  double dense_ms;           /* environment when the handle is made, else 0: encoder input product; the small */
  double logit_ms;           /* dense products and the latent kernels; logits; softmax and its gradient; */
  double softmax_ms;         /* d[W4; b4]; dh2; the fixed-point dW1; Adam */
  double dw4_ms;
  double dh2_ms;
  double dw1_ms;
  double adam_ms;
} irs_multvae_stats_t;
irs_status irs_multvae_create(int64_t n_users, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                              const float *data, int32_t dim_z, int32_t enc_hidden, int32_t dec_hidden,
                              float dropout_p, float l2_regularizer, double kl_anneal_goal, int64_t anneal_end_epoch,
                              int64_t minibatch_size, float learning_rate, uint64_t seed,
                              const float *const *init /* 8 tables, may be NULL */, int32_t device,
                              irs_multvae **out);
irs_status irs_multvae_run_epochs(irs_multvae *t, int64_t n_epochs);
irs_status irs_multvae_order(irs_multvae *t, int64_t epoch, int64_t first, int64_t count, int32_t *users);
irs_status irs_multvae_noise(irs_multvae *t, int64_t update, int64_t n, const int32_t *users, uint8_t *keep,
                             float *eps);
irs_status irs_multvae_step_batch(irs_multvae *t, int64_t n, const int32_t *users, const uint8_t *keep,
                                  const float *eps, double klc, double *nll, double *kl);
irs_status irs_multvae_gradients(irs_multvae *t, float *const *grads /* 8 tables */);
irs_status irs_multvae_get_state(irs_multvae *t, float *const *tables /* 24 */, int64_t *n_updates, int64_t *epoch);
irs_status irs_multvae_set_state(irs_multvae *t, const float *const *tables /* 24 */, int64_t n_updates,
                                 int64_t epoch);
irs_status irs_multvae_encode(irs_multvae *t, int64_t rows, const int64_t *indptr, const int32_t *indices,
                              const float *data, float *h2, float *lse);
irs_status irs_multvae_score(irs_multvae *t, int64_t rows, const int64_t *indptr, const int32_t *indices,
                             const float *data, float *scores);
irs_status irs_multvae_stats(irs_multvae *t, irs_multvae_stats_t *out);
irs_status irs_multvae_destroy(irs_multvae *t);

/* ------------------------------------------------------------------ serving
 * Batch top-k recommendations from a model that stays on the device (the reference's path:
 * utils/id_mapping.py:172-223, 399-453 - get_score_remove_seen on the host, then
 * retrieve_recommend_from_score, util.hpp:426-504).  A server holds the item-side operand of one model,
 * validated and uploaded once by one of three constructors:
 *   similarity        W [n_profile_cols, n_items] as CSR by rows, float64 (item-kNN, P3alpha, RP3beta, SLIM;
 *                     user-kNN with W = the training matrix).  A row that stores a column twice is
 *                     IRS_INVALID_ARGUMENT ("duplicate column in a row of W": two lanes of the score kernel
 *                     would add to one sum at once).  Rows with increasing columns get their per-tile ranges
 *                     here, once; other rows are walked whole.
 *   dense similarity  W [n_profile_cols, n_items] row-major, float32 or float64 (EASE, EDLAE).
 *   factors           item_factors [n_items, k] row-major float32, 1 <= k <= 576, rows zero-padded to a
 *                     multiple of 32 on upload (iALS embeddings, truncated SVD, NMF).
 * A recommend call scores `rows` rows - profiles (CSR float64 [rows, n_profile_cols]: score = profile @ W, the
 * host product bit for bit) or user factors (float32 [rows, k]: fp32 MFMA tiles) -, sets the excluded items of
 * every row to -inf (excl_indptr int64[rows + 1], excl_indices; NULL = none; seen and forbidden items merged by
 * the caller), ranks the candidates and writes, with width = min(cutoff, n_items):
 *   out_idx int32 [rows, width] (-1 padded), out_score float [rows, width] (the winners' scores narrowed to
 *   float32, 0 in the padding), out_len int32 [rows].
 * Allowed lists as in irs_retrieve_recommend: ragged, n_lists in {0, 1, rows}, order and duplicates kept, ids
 * outside [0, n_items) dropped.  Best first, stop at -inf, equal scores in candidate order.  cutoff == 0 or
 * rows == 0 gives empty results without device work; every argument error (IRS_INVALID_ARGUMENT) comes before
 * any device work.  The rows go through in chunks of at most 16384 (IRSPACK_AMD_SERVE_BLOCK overrides the
 * cap, at least 256) whose scores fit 2 GiB (float) / 4 GiB (double); the score block stays on the device,
 * the three output arrays come home once per call.  Two calls give identical bytes.
 * Threads: a server keeps ONE set of call scratch, so it runs one recommend call at a time - calls from several
 * threads on the same server are safe and are serialised by a mutex inside it (use one server per thread to
 * overlap them).  irs_serve_destroy must not run while another thread still uses the server.  The row, offset
 * and list arrays are read by absolute offset: x_indptr[0], excl_indptr[0] and list_ptr[0] must not be negative. */
typedef struct irs_server irs_server;
irs_status irs_serve_create_similarity(int64_t n_profile_cols, int64_t n_items, const int64_t *w_indptr,
                                       const int32_t *w_indices, const double *w_data, int32_t device,
                                       irs_server **out);
irs_status irs_serve_create_dense_similarity(int64_t n_profile_cols, int64_t n_items, int32_t w_is_f64,
                                             const void *w, int32_t device, irs_server **out);
irs_status irs_serve_create_factors(int64_t n_items, int32_t k, const float *item_factors, int32_t device,
                                    irs_server **out);
irs_status irs_serve_destroy(irs_server *s);
irs_status irs_serve_recommend_profiles(irs_server *s, int64_t rows, const int64_t *x_indptr,
                                        const int32_t *x_indices, const double *x_data,
                                        const int64_t *excl_indptr, const int32_t *excl_indices, int64_t n_lists,
                                        const int64_t *list_ptr, const int64_t *list_items, int64_t cutoff,
                                        int32_t *out_idx, float *out_score, int32_t *out_len);
irs_status irs_serve_recommend_factors(irs_server *s, int64_t rows, const float *user_factors,
                                       const int64_t *excl_indptr, const int32_t *excl_indices, int64_t n_lists,
                                       const int64_t *list_ptr, const int64_t *list_items, int64_t cutoff,
                                       int32_t *out_idx, float *out_score, int32_t *out_len);
/* Neighbours: "entities like ids[r]", ranked inside the resident operand (no reference counterpart).  Row r of
 * the call scores every entity j of the server against ids[r] (int64 [rows], each in [0, n_items), repeats
 * allowed); the entity itself is always excluded (score -inf), also when an allowed list names it.  Outputs,
 * allowed lists, exclusions, chunking, ties, threads and "two calls give identical bytes" are those of the
 * recommend calls above, word for word; every argument error (IRS_INVALID_ARGUMENT: an id out of range, a metric
 * that does not fit the server, k_used outside 1 .. k on a factor server or != 0 on a similarity server, a
 * similarity server whose W is not square) comes before any device work.  Nothing but the ids, the exclusions
 * and the lists is uploaded.
 *   similarity servers, IRS_NEIGHBOR_WEIGHT (float64 scores): score[r, j] = W[ids[r], j].  Sparse W: only the
 *     STORED entries of the row are candidates (stored zeros included, any order) - an item without a stored
 *     weight is never listed, which is where the call differs from recommending for a one-hot profile.  Dense
 *     W: the whole row (float32 widened exactly).
 *   factor servers (float32 scores through the MFMA tiles), over the leading k_used columns of the table only
 *     (a bias column or a constant column of the model's table is left out this way):
 *     IRS_NEIGHBOR_DOT     v_q . v_j
 *     IRS_NEIGHBOR_COSINE  (v_q / |v_q|) . v_j / |v_j|: one inverse norm per table row - sum of squares and
 *                          1/sqrt in double, rounded once to float32 - made at the first cosine call, kept on
 *                          the server and remade when k_used changes.  A candidate of norm zero is never listed;
 *                          a query of norm zero gets an empty list.
 *   Tables are finite, as for the recommend calls. */
#define IRS_NEIGHBOR_WEIGHT 0 /* similarity servers */
#define IRS_NEIGHBOR_COSINE 1 /* factor servers */
#define IRS_NEIGHBOR_DOT 2    /* factor servers */
irs_status irs_serve_neighbors(irs_server *s, int64_t rows, const int64_t *ids, int32_t metric, int32_t k_used,
                               const int64_t *excl_indptr, const int32_t *excl_indices, int64_t n_lists,
                               const int64_t *list_ptr, const int64_t *list_items, int64_t cutoff,
                               int32_t *out_idx, float *out_score, int32_t *out_len);
/* Stream time of the last recommend call by phase, in milliseconds (measurement only): ms[0] uploads,
 * ms[1] scoring, ms[2] exclusions, ms[3] ranking, the output stage and the copies home. */
irs_status irs_serve_last_phases(irs_server *s, double *ms);

/* ------------------------------------------------------------ measurement
 * No reference counterpart: SURVEY.md 8(d) asks for ceilings MEASURED on the box next to the
 * spec peaks.  Runs a 1 GiB device copy and STREAM triad (HBM bytes moved / time), a loop of
 * nothing but v_mfma_f32_16x16x4_f32 on every SIMD, and a loop of random-bank ds_add_u32 on
 * every CU (the kNN count accumulation's instruction), and a random whole-row gather out of a
 * 1 GiB table (the iALS access pattern); all HIP-event timed, best of 3-5. */
typedef struct irs_ceilings {
  double copy_gbs;            /* read + write bytes per second of dst = src, GB/s */
  double triad_gbs;           /* a = b + s c: 3 x bytes, GB/s */
  double mfma_f32_tflops;     /* dense fp32 MFMA rate, TFLOP/s */
  double lds_atomic_u32_gops; /* lane-level LDS atomic adds per second (whole device), G/s */
  double clock_mhz;           /* hipDeviceAttributeClockRate */
  int32_t n_cu;
  double gather256_gbs;       /* uniformly random 256-byte rows of a 1 GiB table (16 lanes per row), GB/s */
  double gather512_gbs;       /* the same with 512-byte rows (K = 128 factor rows) */
} irs_ceilings;
irs_status irs_measure_ceilings(int32_t device, irs_ceilings *out);

#ifdef __cplusplus
}
#endif
#endif /* IRSPACK_AMD_H */
