// Host decisions of the iALS path (no HIP dependency): the task plan of a side - which rows are cut into chunks,
// the order of the tasks, the row classes of the other kernels - and the route of a half-step - which kernel family
// and which of its instances a solve launches.  Included by ials.hip, which owns the buffers, streams and launches;
// compiled on its own under AddressSanitizer / ThreadSanitizer (tests/host/ials_host_plan_main.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/irspack_amd.h"
#include "host_util.hpp"
#include "ials_types.hpp"

namespace irs {
namespace ials {

// factors are stored [rows, KP]
inline int padded_k(int64_t K) {
  return K <= 16 ? 16 : K <= 32 ? 32 : K <= 64 ? 64 : static_cast<int>(ceil_div(K, 64) * 64);
}
// the step count of a CG solve: 0 = K steps (hpp:232-234); a caller's own count below 2^20
inline int32_t cg_step_count(uint64_t max_cg_steps, int64_t K) {
  return static_cast<int32_t>(max_cg_steps == 0 ? static_cast<uint64_t>(K) : std::min<uint64_t>(max_cg_steps, 1u << 20));
}

// ---------------------------------------------------------------- the task plan of a side
constexpr int MAX_CHUNKS = 256;  // of one row

// the scalars of a plan: what a Side (ials.hip) keeps on the host beside the device copies of the lists
struct PlanCounts {
  int32_t n_tasks = 0, n_split = 0, n_slots = 0, n_fold = 0;
  // tasks at the end of the list that are whole rows of <= SHORT_MAX / <= 16 / <= 8 entries
  int32_t n_short = 0, n_short16 = 0, n_short8 = 0;
  int64_t long_entries = 0;  // stored entries of the tasks [0, n_tasks - n_short)
  int32_t n_long = 0;        // rows of more than 2048 entries (ialspp_long_kernel)
  // matrix-free CG, 128 < K <= 256 only (ials_mf_kernels.hpp): rows_by_len is cut into the level-synchronous
  // rows (class 0: more than MF_NCAP entries, chunked) and the resident classes of MF_CAPS (class c: MF_CAPS[c + 1]
  // < length <= MF_CAPS[c]); mf_class[c] = first index of class c in rows_by_len, [MF_CLASSES] = end
  int32_t mf_n_lrows = 0, mf_n_chunks = 0, mf_class[MF_CLASSES + 1] = {};
  float reg_min = 0.f;     // smallest per-row regulariser of the rows [row_begin, row_end)
  bool has_empty = false;  // some row of the whole matrix stores no entry (feature-aware step, hpp:639-653)
};
struct TaskPlan : PlanCounts {
  std::vector<Task> tasks;           // longest first, ties in row (and chunk) order
  std::vector<SplitRow> split;       // most slots first, ties in row order
  std::vector<FoldGroup> fold;       // in row order
  std::vector<int32_t> rows_by_len;  // rows [row_begin, row_end) longest first, ties in row order
  std::vector<MfLongRow> mf_lrows;
  std::vector<MfChunk> mf_chunks;
  std::vector<float> reg;            // per row of the WHOLE matrix
};

// emit(place, i) for every item i of [0, n): longest first, ties in item order (a stable counting sort by
// length, O(n + max length))
template <class Len, class Emit> inline void longest_first(int64_t n, Len len, Emit emit) {
  int32_t max_len = 0;
  for (int64_t i = 0; i < n; i++) max_len = std::max(max_len, len(i));
  std::vector<int32_t> start(static_cast<size_t>(max_len) + 2, 0);
  for (int64_t i = 0; i < n; i++) start[max_len - len(i) + 1]++;
  for (size_t i = 1; i < start.size(); i++) start[i] += start[i - 1];
  for (int64_t i = 0; i < n; i++) emit(start[max_len - len(i)]++, i);
}

// `ip`: the row pointer of a matrix of n_rows x n_cols (n_rows + 1 values); the tasks cover the rows
// [rb, re).  `chunk`: a row of more entries is cut (a multiple of 4, IRSPACK_AMD_IALS_CHUNK);
// `chunk_long` >= chunk: the chunk length above 32 chunks (IRSPACK_AMD_IALS_CHUNK_LONG).
inline TaskPlan plan_tasks(const int32_t *ip, int64_t n_rows, int64_t n_cols, int64_t rb, int64_t re,
                           const irs_ials_model_config &cfg, int chunk, int32_t chunk_long) {
  TaskPlan pl;
  pl.reg.resize(n_rows);
  parallel_ranges(n_rows, [&](int64_t r0, int64_t r1) {  // (10 M powf at the 10 M x 1 M shape)
    for (int64_t r = r0; r < r1; r++) {
      // Solver::compute_reg, hpp:117-120, evaluated in float like the reference
      const int64_t nz = ip[r + 1] - ip[r];
      pl.reg[r] = cfg.reg * std::pow(cfg.alpha0 * n_cols + nz, cfg.nu);
    }
  });
  for (int64_t r = rb; r < re; r++) pl.reg_min = r == rb ? pl.reg[r] : std::min(pl.reg_min, pl.reg[r]);
  for (int64_t r = 0; r < n_rows && !pl.has_empty; r++) pl.has_empty = ip[r + 1] == ip[r];
  std::vector<Task> &tk = pl.tasks;
  tk.reserve(re - rb);
  int32_t slots = 0;
  for (int64_t r = rb; r < re; r++) {
    const int32_t b = ip[r], e = ip[r + 1], nz = e - b;
    if (nz > chunk) {
      // a bounded number of chunks per row: the second kernel adds a row's partials one after the other, and a
      // chunk is one wave's serial work (the longest chunk is the floor of the half-step: 4.4 M entries in 32
      // chunks were 16 ms of one wave at K = 128).  Up to 32 chunks of any length, more only to keep a chunk below
      // 16 K entries: the ML-20M shape's longest row - 116 k entries - stays at 32 chunks and needs no fold pass.
      const int32_t nch = std::min<int32_t>(
          (nz + chunk - 1) / chunk, std::max<int32_t>(32, std::min<int32_t>(MAX_CHUNKS, (nz + chunk_long - 1) / chunk_long)));
      const int32_t per = (((nz + nch - 1) / nch) + 3) & ~3;
      SplitRow sr{static_cast<int32_t>(r), slots, 0, nz, 1};
      for (int32_t c = b; c < e; c += per) {
        tk.push_back(Task{static_cast<int32_t>(r), c, std::min(c + per, e), slots++});
        sr.n_slots++;
      }
      if (sr.n_slots > FOLD_MIN) {
        for (int32_t g = 0; g < sr.n_slots; g += FOLD_GROUP)
          pl.fold.push_back(FoldGroup{sr.first_slot + g, std::min(FOLD_GROUP, sr.n_slots - g)});
        sr.n_slots = (sr.n_slots + FOLD_GROUP - 1) / FOLD_GROUP;
        sr.slot_stride = FOLD_GROUP;
      }
      pl.split.push_back(sr);
    } else {
      tk.push_back(Task{static_cast<int32_t>(r), b, e, -1});
    }
  }
  {
    std::vector<Task> sorted(tk.size());
    longest_first(static_cast<int64_t>(tk.size()), [&](int64_t i) { return tk[i].end - tk[i].begin; },
                  [&](int32_t place, int64_t i) { sorted[place] = tk[i]; });
    tk.swap(sorted);
  }
  // (dealing length strata round-robin so that neighbouring waves sit in different phases
  // was tried: 3-5 % slower, and 2x slower when the stratum count shares a factor with the
  // 8 XCDs the dispatcher deals workgroups to - longest-first keeps the XCDs balanced)
  std::stable_sort(pl.split.begin(), pl.split.end(),
                   [](const SplitRow &a, const SplitRow &b) { return a.n_slots > b.n_slots; });
  pl.n_tasks = static_cast<int32_t>(tk.size());
  pl.n_split = static_cast<int32_t>(pl.split.size());
  pl.n_fold = static_cast<int32_t>(pl.fold.size());
  pl.n_slots = slots;
  // the short rows: the scan stops at the first task that is longer or owns a slot (a split row's chunk is no ROW)
  for (int32_t i = pl.n_tasks - 1; i >= 0 && tk[i].slot < 0 && tk[i].end - tk[i].begin <= SHORT_MAX; i--) {
    if (tk[i].end - tk[i].begin <= 16) pl.n_short16++;
    if (tk[i].end - tk[i].begin <= 8) pl.n_short8++;
    pl.n_short++;
  }
  // entries of the tasks in front of the short ones (the rank-update kernels' work)
  for (int32_t i = 0; i < pl.n_tasks - pl.n_short; i++) pl.long_entries += tk[i].end - tk[i].begin;
  std::vector<int32_t> &order = pl.rows_by_len;
  order.resize(re - rb);
  longest_first(re - rb, [&](int64_t i) { return ip[rb + i + 1] - ip[rb + i]; },
                [&](int32_t place, int64_t i) { order[place] = static_cast<int32_t>(rb + i); });
  if (cfg.K > 128 && cfg.K <= 256) {  // the classes of the matrix-free CG kernels
    size_t i = 0;
    for (int c = 0; c < MF_CLASSES; c++) {
      pl.mf_class[c] = static_cast<int32_t>(i);
      const int32_t lower = c + 1 < MF_CLASSES ? MF_CAPS[c + 1] : -1;  // class c: lower < length <= MF_CAPS[c]
      while (i < order.size() && ip[order[i] + 1] - ip[order[i]] > lower) i++;
    }
    pl.mf_class[MF_CLASSES] = static_cast<int32_t>(order.size());
    for (int32_t k = 0; k < pl.mf_class[1]; k++) {
      const int32_t r = order[k], b = ip[r], e = ip[r + 1], nz = e - b;
      const int32_t nch = (nz + MF_CHUNK - 1) / MF_CHUNK;
      const int32_t per = (((nz + nch - 1) / nch) + 15) & ~15;  // whole 16-entry groups
      MfLongRow L{r, static_cast<int32_t>(pl.mf_chunks.size()), 0, 0};
      for (int32_t c = b; c < e; c += per) {
        pl.mf_chunks.push_back(MfChunk{k, c, std::min(c + per, e), 0});
        L.n_chunks++;
      }
      pl.mf_lrows.push_back(L);
    }
    pl.mf_n_lrows = static_cast<int32_t>(pl.mf_lrows.size());
    pl.mf_n_chunks = static_cast<int32_t>(pl.mf_chunks.size());
  }
  while (pl.n_long < static_cast<int32_t>(order.size()) && ip[order[pl.n_long] + 1] - ip[order[pl.n_long]] > 2048)
    pl.n_long++;
  return pl;
}

// ---------------------------------------------------------------- the route of a half-step
// the development switches of a trainer (ials.hip: read_switches names their variables)
struct Switches {
  bool opt_wave128 = true, opt_unit = true, opt_short = true, opt_wg16 = true;
  bool opt_short2 = true;     // two short rows per wave (IRSPACK_AMD_IALS_SHORT2)
  bool opt_pp_direct = true;  // iALS++ with one block = the direct solve (IRSPACK_AMD_IALSPP_DIRECT)
  bool opt_pp_chain = true;   // iALS++ prediction passes merged into the rank updates (IRSPACK_AMD_IALSPP_CHAIN)
  bool opt_pp_fork = true;    // iALS++ short-row launch on a second stream (IRSPACK_AMD_IALSPP_FORK)
  bool opt_bf16x3 = false;
  bool opt_gather_lds = false;  // the bf16x3 gather staged in LDS (IRSPACK_AMD_IALS_GATHER_LDS)
  bool opt_eig = true, opt_mf = true;  // IRSPACK_AMD_IALS_EIG, IRSPACK_AMD_IALS_MF
};
// what launch_solve knows before it launches anything
struct SolveFacts : Switches {
  int T = 0, KP = 0;  // KP = padded_k(K), T = KP / 16
  int64_t K = 0;
  int32_t solver_type = IRS_SOLVER_CHOLESKY;
  uint64_t subspace_dimension = 0, sweeps = 0;  // iALS++
  bool has_prior = false;   // feature-aware half-step
  bool other_own = false;   // the gathered table is the trainer's factor buffer of the other side
  bool target_own = false;  // the solved rows are the trainer's factor buffer of this side
  // the side
  bool unit = false, positive = false;
  int32_t n_tasks = 0, n_short = 0, n_short16 = 0;
  int64_t n_other = 0, long_entries = 0;
  int64_t zero_row = 0;  // the all-zero row the UNIT kernels gather past a row's end: n_other rounded up to 8
};

// the form of an iALS++ sweep (Solver::step_ialspp, hpp:516-630)
struct PpVariant {
  bool general;  // blocks wider than 64 dims, or KP > 2048: the run-time-size kernels (ials_gk_kernels.hpp)
  int32_t sub;   // dims per block (0 and 1 are the iCD branch, hpp:673-677); general: at most K
  int TS;        // 16-dim tiles of a block: ialspp_kernel<TS, aligned, form>
  bool aligned;  // every block starts at a multiple of TS
  bool single;   // one block covers every dim (form 1)
  bool chained;  // 64-dim blocks at K > 64, prediction passes merged into the rank updates (form 2; P packed)
};
inline PpVariant pp_variant(uint64_t subspace_dimension, int64_t K, int KP, bool opt_pp_chain) {
  PpVariant v{};
  v.general = subspace_dimension > 64 || KP > 2048;
  if (v.general) {
    v.sub = static_cast<int32_t>(std::min<uint64_t>(std::max<uint64_t>(1, subspace_dimension), K));
    return v;
  }
  v.sub = static_cast<int32_t>(std::max<uint64_t>(1, subspace_dimension));
  const int D = static_cast<int>(std::min<int64_t>(v.sub, K));
  v.TS = D <= 16 ? 1 : D <= 32 ? 2 : 4;
  v.aligned = v.sub % v.TS == 0;
  v.single = v.sub >= K;
  v.chained = opt_pp_chain && v.sub == 64 && K > 64;  // (then TS = 4, aligned, not single)
  return v;
}

// The LDS-staged gather keeps ONE 8-KB group per wave in flight (16 waves per CU) where the register-staged one
// keeps two (12 waves): faster while the gathered table is served by L2, slower beyond.  ML-20M shape, K = 64, one
// MI355X: the 6.8 MB item table 1.067 -> 1.045 ms (user half), the 35 MB user table 0.617 -> 0.625 ms (item half);
// nothing was measured in between, the limit is set between the two at four times an XCD's L2.
constexpr uint64_t GATHER_LDS_MAX_TABLE_BYTES = uint64_t(16) << 20;

enum class SolvePath : int32_t {
  PP_BLOCKS,   // iALS++ sweeps over blocks of up to 64 dims (ials_pp_kernels.hpp)
  PP_GENERAL,  // iALS++ with wider blocks or KP > 2048 (ials_gk_kernels.hpp)
  GK,          // K > 256: every size is a run-time value (ials_gk_kernels.hpp)
  MF_CG,       // CG at 128 < K <= 256, matrix free (ials_mf_kernels.hpp)
  DENSE        // the K x K system of every task in registers / LDS
};
enum class DenseFamily : int32_t {
  WAVE,   // T <= 4: ials_solve_kernel<T, ...>, one wave per task
  WAVE8,  // T = 8: ials_solve_kernel<8, ...>
  WG16,   // Cholesky, T >= 12 (or T = 8 without WAVE128): ials_wg16_cholesky_kernel
  WG      // ials_wg_solve_kernel
};
struct SolveRoute {
  SolvePath path;
  bool pp_direct;  // iALS++ with one block that covers every dimension: the direct solve in gradient form (RESID)
  bool cg;  // (from here on: path == DENSE only)
  bool unit;  // binary interactions on the UNIT kernels (they address the gathered table with 32-bit byte offsets)
  DenseFamily family;
  // the bf16x3 rank update of: the launch over the regular tasks; the launch that finishes the split rows (CG only:
  // lower-form partials); a dense launch over the short rows after the eigenbasis path declined
  bool x3, x3_split, x3_declined;
  // the bf16x3 launches over tasks stage their gathered rows in LDS instead of registers (Cholesky at T = 4: the
  // CG kernel keeps its matrix rows in 64 registers and gains no wave from the 48 the staging frees), where the
  // gathered table is at most GATHER_LDS_MAX_TABLE_BYTES
  bool x3_lds;
  bool short_cg_ok, short_fork;  // the short rows take the matrix-free short-row CG kernels; on the second stream
  bool eig_candidate;  // the eigenbasis path for the short rows is worth trying (then P's conditioning decides)
  int32_t n_regular;   // tasks of the dense launch: all, or all but the short rows
};
inline SolveRoute solve_route(const SolveFacts &f) {
  SolveRoute r{};
  r.n_regular = f.n_tasks;
  if (f.solver_type == IRS_SOLVER_IALSPP) {
    r.pp_direct = f.opt_pp_direct && f.subspace_dimension > 1 && f.subspace_dimension >= static_cast<uint64_t>(f.K) &&
                  f.sweeps >= 1 && f.T <= 4 && f.target_own;
    if (!r.pp_direct) {
      r.path = pp_variant(f.subspace_dimension, f.K, f.KP, f.opt_pp_chain).general ? SolvePath::PP_GENERAL
                                                                                  : SolvePath::PP_BLOCKS;
      return r;
    }
  }
  r.cg = f.solver_type == IRS_SOLVER_CG;
  if (f.KP > 256) {
    r.path = SolvePath::GK;
    return r;
  }
  if (r.cg && f.T > 8 && !f.has_prior && f.opt_mf) {
    r.path = SolvePath::MF_CG;
    return r;
  }
  r.path = SolvePath::DENSE;
  const bool unit_any = f.unit && f.opt_unit && f.other_own;
  r.unit = unit_any && static_cast<uint64_t>(f.zero_row + 8) * f.KP * sizeof(float) < (uint64_t(1) << 32);
  // short rows (<= 32 entries) in the eigenbasis of P (ials_eig_kernels.hpp): worth one eigen-decomposition (ms of
  // ONE compute unit) and the product that takes every gathered row into the eigenbasis (n_other x KP x KP)?
  // configs[3]: the user side (9.7 M short rows, 10^6 gathered rows) yes, the item side (0.8 M, 10^7) no.  Cholesky
  // saves a dense KP^3 / 3 factorisation per short row, CG only its products with P (hence the two ratios).
  r.eig_candidate = !f.has_prior && !r.pp_direct && f.other_own && f.opt_eig && (f.KP == 64 || f.KP == 128) &&
                    f.positive && f.n_short > 0 &&
                    !(static_cast<double>(f.n_short) * f.KP * f.KP * f.KP < 3e11) &&
                    !(static_cast<double>(f.n_short) * f.KP < (r.cg ? 64.0 : 8.0) * static_cast<double>(f.n_other));
  // CG: the matrix-free short-row kernels take the tail of the task list, beside the long rows when it is long
  r.short_cg_ok = r.cg && !f.has_prior && f.n_short > 0 && (f.T <= 4 || f.T == 8) && f.opt_short;
  r.short_fork = !r.eig_candidate && r.short_cg_ok && f.n_short >= 65536;
  if (r.eig_candidate || r.short_cg_ok) r.n_regular = f.n_tasks - f.n_short;
  if (!r.cg && (f.T >= 12 || (f.T == 8 && !f.opt_wave128)) && f.opt_wg16) r.family = DenseFamily::WG16;
  else if (f.T == 8 && f.opt_wave128) r.family = DenseFamily::WAVE8;
  else if (f.T <= 4) r.family = DenseFamily::WAVE;
  else r.family = DenseFamily::WG;
  if (r.family == DenseFamily::WAVE) {
    r.x3 = r.x3_declined = r.unit && f.opt_bf16x3 && f.T == 4;
    r.x3_split = r.x3 && r.cg;
    r.x3_lds = r.x3 && !r.cg && !r.pp_direct && f.opt_gather_lds &&
               static_cast<uint64_t>(f.n_other) * f.KP * sizeof(float) <= GATHER_LDS_MAX_TABLE_BYTES;
  } else if (r.family == DenseFamily::WAVE8) {
    // The bf16x3 kernels hold ~410-440 registers (one wave per SIMD), the fp32-input Cholesky kernel 236 (two).
    // Under Cholesky the second wave is worth more than the faster rank update when rows are short - ML-20M user
    // half, 144 entries per task: 4.8 ms fp32-input, 5.3 ms bf16x3; item half, 544 per task: 3.1 -> 2.5 ms - so the
    // choice goes by the mean task length.  (No 4 GB limit: the T = 8 bf16x3 gather uses 64-bit row addresses.)
    const bool x3_any = unit_any && f.opt_bf16x3;
    auto long_enough = [&](int32_t count) { return f.long_entries >= int64_t(320) * std::max(count, 1); };
    r.x3 = x3_any && (r.cg || long_enough(r.n_regular));
    r.x3_declined = x3_any && (r.cg || long_enough(f.n_short));
    r.x3_split = x3_any && r.cg;
  }
  return r;
}

// ---------------------------------------------------------------- the eigenbasis short-row path
// M = P + reg_r I must be well conditioned for EVERY row (float32 carries Q and 1 / (lambda + reg)); lam_max,
// lam_min: the extreme eigenvalues of P the decomposition kernel reports
inline bool eig_well_conditioned(float lam_max, float lam_min, float reg_min) {
  const double lo = std::max(0.0, static_cast<double>(lam_min)) + reg_min;
  const double hi = static_cast<double>(lam_max) + reg_min;
  return lo > 0.0 && hi <= 1e4 * lo && std::isfinite(hi);
}
// A pass over the short rows [b0, b0 + m) of the longest-first list [17..32 entries | 9..16 | <= 8]:
// [0, m2) have 17..32 entries (one row per wave), [m2, m3) 9..16, [m3, m) <= 8 (four rows per wave)
struct EigCuts {
  int32_t m2, m3;
};
inline EigCuts eig_pass_cuts(int32_t b0, int32_t m, int32_t n_short, int32_t n_short16, int32_t n_short8) {
  const int32_t n32 = n_short - n_short16, n16 = n_short - n_short8;
  EigCuts c;
  c.m2 = std::max(0, std::min(b0 + m, n32) - b0);
  c.m3 = std::max(c.m2, std::min(b0 + m, n16) - b0);
  return c;
}

}  // namespace ials
}  // namespace irs
