// What the evaluator decides on the host before and between its launches (no HIP dependency): the domain and the
// shape of a pass of the threshold-filtered ("emit") path of irs_eval_get_metrics_ials, which ranking kernel a
// block takes, which item-histogram table.  Plain functions from facts to small plans; evaluator.hip reads the
// environment switches (per call) and hands them in, launches what the plan says, and decides nothing itself.
// Compiled on its own under AddressSanitizer + UBSan against restatements of the former condition chains
// (tests/host/eval_host_prep_main.cpp).
#pragma once
#include "eval_host_prep.hpp"

namespace irs {
namespace eval {

// an integer switch as the caller found it: unset, or std::atoll of its text
struct EnvInt { bool set; int64_t value; };
// IRSPACK_AMD_EVAL_SAMPLE / _PASS_ROWS count in multiples of 64, at least 64; 0: not set
inline int64_t whole_64(EnvInt v) { return v.set ? std::max<int64_t>(64, v.value / 64 * 64) : int64_t(0); }

// Users per pass of the emit path: the candidate lists take 8 KB per user and the mask bitmap n_items / 8 bytes
// per user, at most 2 GiB per pass.  0: a catalogue so wide that a pass would hold fewer than 64 users - not this path.
inline int64_t emit_pass_rows(int64_t n_items, EnvInt env_pass_rows) {
  const int64_t words = ceil_div(std::max<int64_t>(n_items, 1), 64);
  int64_t pass = std::min<int64_t>(524288, (int64_t(1) << 31) / (words * 8) / 64 * 64);
  if (const int64_t env_rows = whole_64(env_pass_rows)) pass = std::min(pass, env_rows);
  return pass < 64 ? 0 : pass;
}

// the mask of a pass as a bitmap: at most 2 GiB
inline bool mask_bitmap_fits(int64_t rows, int64_t words) { return !(static_cast<double>(rows) * words * 8.0 > 2147483648.0); }

struct EmitFacts {
  bool emit_on, bound_on, sample_fused_on;  // IRSPACK_AMD_EVAL_EMIT / _BOUND / _SAMPLE_FUSED
  EnvInt sample;                            // IRSPACK_AMD_EVAL_SAMPLE
  int rec_mode;
  int64_t cutoff, rows;                     // rows of this pass
  int32_t KP;                               // padded width of the factor tables
  int64_t ni, n_items;                      // items of the model, of the evaluator
};

struct EmitPlan {
  bool ok;              // inside the path's domain
  bool bounded;         // items by decreasing norm, tiles pruned by the norm bound
  int64_t n_sample;     // items of the sample pass
  int64_t words;        // bitmap words per row
  bool fused_sample;    // the sample pass is one launch of sample_tau_fused_kernel<KP> ...
  int sample_per_cu;    // ... of at most this many workgroups per CU
  int64_t sample_block; // else: users per block of the three-launch form (<= 256 MB of scores)
  int64_t hcap;         // rows the second chance handles
  bool second_chance;
  int64_t tiles_total;  // 64 x 64 tiles of the pass (all of them are scored when not bounded)
  int64_t n_ut;         // user tiles
  int64_t wg_bound;     // work list: at most ceil(item tiles / 4) entries per user tile
  bool wg_len_on_device;  // the list is sized for wg_bound and its length never comes back; else it is read first
  int32_t wg_grid;      // grid of score_emit_kernel over a list whose length stays on the device
  bool two_level;       // the sum of the per-user terms: chunks of reduce_chunk rows, then the chunks in order
  int64_t reduce_chunk;
};

// what can be said before the model is looked at
inline bool emit_call_in_domain(const EmitFacts &f) {
  return f.emit_on && f.rec_mode == 0 && f.cutoff <= FZ_MAX_CUTOFF && f.rows > 0;
}
// widths score_emit_kernel is instantiated for (a wider model takes the two-pass path's run-time-sized kernel)
inline bool emit_width_ok(int32_t KP) { return KP == 16 || KP == 32 || KP == 64 || KP == 128 || KP == 192 || KP == 256; }

inline EmitPlan plan_emit_pass(const EmitFacts &f) {
  EmitPlan p{};
  // worth it only when the sample is a small part of the catalogue
  p.ok = emit_call_in_domain(f) && emit_width_ok(f.KP) && f.ni == f.n_items && f.ni >= 4 * EM_SAMPLE &&
         f.rows <= (int64_t(1) << 31) / EM_CAP;
  if (!p.ok) return p;
  p.bounded = f.bound_on && f.ni < (int64_t(1) << 31) && f.rows < (int64_t(1) << 31);
  // Sorted by norm (bounded variant) a few hundred items already hold nearly every user's threshold.  The users the
  // sample leaves without one (they have seen almost all of it) get a second chance on EM_SAMPLE2 items.
  const int64_t env_sample = whole_64(f.sample);
  p.n_sample = std::min<int64_t>(env_sample ? env_sample : (p.bounded ? EM_SAMPLE_SORTED : EM_SAMPLE), EM_SAMPLE2);
  p.words = ceil_div(f.ni, 64);
  p.fused_sample = p.bounded && p.n_sample == SF_ITEMS && (f.KP == 16 || f.KP == 32 || f.KP == 64 || f.KP == 128) &&
                   f.sample_fused_on;
  p.sample_per_cu = f.KP == 128 ? 1 : 2;
  p.sample_block = 32768;
  p.hcap = std::min<int64_t>(EM_HARD_CAP, f.rows);
  p.second_chance = p.bounded && p.n_sample < EM_SAMPLE2;
  p.n_ut = ceil_div(f.rows, 64);
  p.tiles_total = p.n_ut * ceil_div(f.ni, 64);
  // up to 2^24 entries (64 MB) the work list is sized for its bound and score_emit_kernel walks it with a grid stride
  p.wg_bound = p.n_ut * ceil_div(ceil_div(f.ni, 64), 4);
  p.wg_len_on_device = p.wg_bound <= (int64_t(1) << 24);
  p.wg_grid = static_cast<int32_t>(std::min<int64_t>(p.wg_bound, 32768));
  p.two_level = f.rows >= 32768;
  p.reduce_chunk = 4096;
  return p;
}

inline int64_t sample_fused_grid(int64_t rows, int per_cu, int cu_count) {
  return std::min<int64_t>(ceil_div(rows, SF_USERS), int64_t(per_cu) * cu_count);
}

// After the candidates are ranked: non-finite scores (the two-pass path defines the order of NaN), or so many hard
// rows that one by one is the slower way - the caller runs the two-pass path.  So at most 1,024 hard rows are ever
// ranked from their full score rows, and they always take the general kernel: a few dozen rows leave the
// one-wave-per-row kernel latency bound (51 us for 76 rows of an ML-20M call, the 1024-thread form takes 12).
inline bool emit_abandon(int32_t flags, int32_t n_hard) { return flags != 0 || n_hard > 1024; }
// hard rows per chunk: <= 1 GB of scores
inline int64_t hard_row_chunk(int64_t n_hard, int64_t ni) {
  return std::max<int64_t>(1, std::min<int64_t>(n_hard, (int64_t(1) << 28) / ni));
}

// Which ranking kernels a block of score rows takes (launch_rank).
struct RankPlan {
  bool big;          // cutoff > SEL_CAP: the selected lists in global scratch, ...
  int64_t big_cap;   // ... this many entries per row (a power of two >= cutoff, 13 bytes each), ...
  int64_t big_rows;  // ... this many rows per launch (<= 1 GiB of scratch)
  bool wave;         // rank_wave_kernel<T, wave_m> first; rank_rows_kernel then ranks the rows it flags
  int wave_m;
  int mode;          // rank_rows_kernel: 2 keys in registers, 1 keys in key_bytes of LDS, 0 scores re-read
  size_t key_bytes;
};
inline RankPlan plan_rank(int64_t cutoff, int64_t rows, int64_t max_cand, bool f32_scores, int rec_mode,
                          int64_t n_items, bool wave_on, bool has_todo) {
  RankPlan r{};
  r.key_bytes = static_cast<size_t>(std::max<int64_t>(max_cand, 1)) * (f32_scores ? 4 : 8);
  const bool keys_fit_lds = r.key_bytes <= 128 * 1024;  // next to the 28 KB of static LDS
  r.big = cutoff > SEL_CAP;
  if (r.big) {
    r.big_cap = 1;
    while (r.big_cap < cutoff) r.big_cap <<= 1;
    r.big_rows = std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t(1) << 30) / (r.big_cap * 13)));
    r.mode = keys_fit_lds ? 1 : 0;
    return r;
  }
  // the usual case (all items are candidates, cutoff <= 64): one wave per row
  r.wave = wave_on && rec_mode == 0 && cutoff <= 64 && n_items < (int64_t(1) << 31) - 64 * 16 && has_todo;
  r.wave_m = cutoff <= 24 ? 4 : 8;
  r.mode = f32_scores && max_cand <= 1024 * RANK_MAXQ ? 2 : (keys_fit_lds ? 1 : 0);
  return r;
}

// Item histogram of `n` list entries: the direct table when the catalogue's counters fit one CU's LDS and there
// is enough to count, else the hashed one; grid 0: nothing to launch.
struct HistPlan { bool direct; int64_t grid; };
inline HistPlan plan_item_hist(int64_t n, int64_t n_items) {
  if (n <= 0) return HistPlan{false, 0};
  const bool direct = n_items > 0 && n_items <= HIST_DIRECT_MAX && n >= 65536;
  return HistPlan{direct, std::min<int64_t>(direct ? 128 : 1024, (n + 16383) / 16384)};
}

}  // namespace eval
}  // namespace irs
