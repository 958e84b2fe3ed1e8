// Ranking kernel of the evaluator and the serving calls: what a ranking launch is handed (EvalParams), what it
// leaves per row (RowOut), the order-preserving keys, and rank_rows_kernel - one workgroup per user row, any
// cutoff, any candidate list (evaluator.cpp:292-367, :127-166; the header of evaluator.hip describes the steps).
// Which instance a call launches is decided on the host: plan_rank, eval_emit_plan.hpp.
// (Included by evaluator.hip inside its translation unit, first of the kernel headers: the others use its types.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "eval_host_prep.hpp"

namespace irs {
namespace eval {

struct RowOut {
  double hit, recall, ndcg, precision, map;
  int32_t valid;   // 1 when the user has ground truth
  int32_t n_rec;
};

// order-preserving integer keys; larger key = better score.  NaN ranks last,
// -0.0 == +0.0 (the reference compares floats, where they tie).
__device__ __forceinline__ uint64_t order_key(float s) {
  if (s != s) return 0ull;
  if (s == 0.f) s = 0.f;
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return static_cast<uint64_t>(u);
}
__device__ __forceinline__ uint64_t order_key(double s) {
  if (s != s) return 0ull;
  if (s == 0.0) s = 0.0;
  uint64_t u = static_cast<uint64_t>(__double_as_longlong(s));
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
template <class T> struct KeyBits;
template <> struct KeyBits<float> { static constexpr int value = 32; };
template <> struct KeyBits<double> { static constexpr int value = 64; };
template <class T> __device__ __forceinline__ bool is_neg_inf(T s) {
  return s == -std::numeric_limits<T>::infinity();
}

struct EvalParams {
  const void *scores;        // [rows, n_items] row-major
  int64_t rows, n_items;
  int64_t offset;            // ground-truth row of scores row 0
  const int32_t *gt_ptr;     // filtered ground truth CSR (relevant ∩ recommendable)
  const int32_t *gt_idx;
  int32_t rec_mode;          // 0 all items, 1 global list, 2 per-user lists
  const int64_t *rec_ptr;
  const int32_t *rec_items;
  int32_t cutoff;
  int32_t retrieve;          // 1: only the ranked lists are wanted (no ground truth, no metrics)
  int32_t recall_with_cutoff;
  const double *disc;        // 1 / log2(2 + i)
  const double *idcg_prefix; // sequential prefix sums of disc
  RowOut *out;
  int32_t *rec_out;          // [rows, cutoff] recommended items (-1 padded)
  unsigned long long *item_cnt;
  int32_t *todo;             // per row: 1 = left to rank_rows_kernel by rank_wave_kernel (or null)
  // score row r stands for row row_map[r] of the call (ground truth, outputs); null: r itself
  const int32_t *row_map = nullptr;
  // cutoff > SEL_CAP (rank_rows_kernel<..., BIG>): the selected (key, index, hit) lists live in
  // global scratch, `big_cap` (a power of two >= cutoff) entries per workgroup of the launch;
  // the launch covers the rows row_base + blockIdx.x
  int64_t row_base = 0;
  uint64_t *big_key = nullptr;
  int32_t *big_idx = nullptr;
  uint8_t *big_hit = nullptr;
  int32_t big_cap = 0;
};

// key value no score maps to (it is the image of a negative NaN pattern, and NaNs are
// canonicalised to 0): marks "not rankable" (-inf) in the cached keys
constexpr uint64_t KEY_SKIP = 1ull;
template <class T> struct KeyStore;
template <> struct KeyStore<float> { using type = uint32_t; };
template <> struct KeyStore<double> { using type = uint64_t; };

// NT threads per user row.  Wave w owns the contiguous candidates [w * span, (w + 1) * span) in
// 64-wide steps: slot q of lane l is candidate w * span + 64 q + l, so (wave, slot, lane)
// order is index order.  Where the keys live between the passes:
//   MODE 2 (NT = 1024, float scores, <= 32 slots per lane): in registers - one pass over the
//          scores in HBM, no LDS traffic for keys (same speed as MODE 1 today: the kernel is
//          bound by its barrier / latency chain, and the 64-VGPR budget that a second
//          workgroup per CU would need spills);
//   MODE 1 (NT = 1024): in dynamic LDS - one pass over the scores, one workgroup per CU;
//   MODE 0 (NT = 256): nowhere, every pass re-reads the scores.

// BIG (cutoff > SEL_CAP, any cutoff up to n_items like the reference, evaluator.cpp:263-268):
// the selected lists are kept in global scratch instead of LDS (a workgroup's own global stores
// are visible to its other waves after __syncthreads: they share the CU's L1), everything else
// is the same code.
// POS (the serving calls, retrieve = 1 with candidate lists): the selected entries carry the candidate's POSITION in
// its list instead of its item, so equal scores come out in candidate order whatever the order of the list
// (util.hpp:426-504 through a stable sort); the item is looked up when the list is written.  The evaluator's lists
// are sorted and without duplicates, where the two orders are the same.
template <class T, int NT, int MODE, int MAXQ = RANK_MAXQ, bool BIG = false, bool POS = false>
__global__ __launch_bounds__(NT, MODE == 2 ? 4 : 1) void rank_rows_kernel(EvalParams p) {
  using KeyT = typename KeyStore<T>::type;
  constexpr int NWV = NT / 64;
  constexpr bool CACHED = MODE == 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char rank_dyn[];
  KeyT *keys = reinterpret_cast<KeyT *>(rank_dyn);
  __shared__ uint32_t hist[256];
  __shared__ uint64_t sel_key_lds[BIG ? 1 : SEL_CAP];
  __shared__ int32_t sel_idx_lds[BIG ? 1 : SEL_CAP];
  __shared__ uint8_t sel_hit_lds[BIG ? 1 : SEL_CAP];
  __shared__ int32_t scan_buf[NWV > 4 ? NWV : 4];
  __shared__ uint64_t sh_prefix;
  __shared__ int32_t sh_need, sh_count;
  const int sel_cap = BIG ? p.big_cap : SEL_CAP;
  uint64_t *sel_key = BIG ? p.big_key + static_cast<size_t>(blockIdx.x) * p.big_cap : sel_key_lds;
  int32_t *sel_idx = BIG ? p.big_idx + static_cast<size_t>(blockIdx.x) * p.big_cap : sel_idx_lds;
  uint8_t *sel_hit = BIG ? p.big_hit + static_cast<size_t>(blockIdx.x) * p.big_cap : sel_hit_lds;

  const int tid = threadIdx.x;
  const int wv = tid >> 6, ln = tid & 63;
  const int64_t row = p.row_base + blockIdx.x;
  if (p.todo != nullptr && p.todo[row] == 0) return;  // ranked by rank_wave_kernel
  const int64_t orow = p.row_map ? p.row_map[row] : row;
  const int64_t u = orow + p.offset;
  const T *srow = static_cast<const T *>(p.scores) + row * p.n_items;
  RowOut res{0, 0, 0, 0, 0, 0, 0};
  const int gb = p.retrieve ? 0 : p.gt_ptr[u], ge = p.retrieve ? 0 : p.gt_ptr[u + 1];
  const int n_gt = ge - gb;
  int32_t *rec_row = p.rec_out + orow * p.cutoff;
  for (int i = tid; i < p.cutoff; i += NT) rec_row[i] = -1;
  if (n_gt == 0 && !p.retrieve) {  // counted in total_user only (:316-321)
    if (tid == 0) p.out[orow] = res;
    return;
  }
  // what the last phase needs from HBM is requested now, so that its latency hides behind
  // the ranking: a short ground-truth row, the discounts, the ideal dcg
  int32_t gt_pref = -1;
  double disc_pref = 0.0, idcg_pref = 0.0;
  if (!p.retrieve) {
    if (n_gt <= 64 && ln < n_gt) gt_pref = p.gt_idx[gb + ln];
    if (ln < min(p.cutoff, 64)) disc_pref = p.disc[ln];
    idcg_pref = p.idcg_prefix[min(n_gt, p.cutoff)];
  }
  // candidate list
  int64_t cb = 0, n_cand = p.n_items;
  const int32_t *list = nullptr;
  if (p.rec_mode == 1) {
    cb = p.rec_ptr[0];
    n_cand = p.rec_ptr[1] - cb;
    list = p.rec_items + cb;
  } else if (p.rec_mode == 2) {
    cb = p.rec_ptr[u];
    n_cand = p.rec_ptr[u + 1] - cb;
    list = p.rec_items + cb;
  }
  auto item_of = [&](int64_t j) -> int32_t { return list ? list[j] : static_cast<int32_t>(j); };
  auto sel_of = [&](int64_t j) -> int32_t {  // what a selected entry carries (and ties are ordered by)
    if constexpr (POS) return static_cast<int32_t>(j);
    else return item_of(j);
  };
  auto key_from_scores = [&](int64_t j) -> uint64_t {
    const T s = srow[item_of(j)];
    return is_neg_inf(s) ? KEY_SKIP : order_key(s);
  };
  auto key_at = [&](int64_t j) -> uint64_t {
    return CACHED ? static_cast<uint64_t>(keys[j]) : key_from_scores(j);
  };

  // --- count rankable candidates (and fill the key cache).  Eight independent loads per
  //     thread are issued before the first use (clamped index, result masked) so the one
  //     pass over the scores in HBM is not a chain of exposed latencies.
  const int64_t span = ((n_cand + NT - 1) / NT) * 64;
  const int64_t wbeg = wv * span, wend = min<int64_t>(wbeg + span, n_cand);
  KeyT kreg[MODE == 2 ? MAXQ : 1];
  int local = 0;
  uint64_t tmax = 0;  // best rankable key of this thread (0: none)
  if constexpr (MODE == 2) {
#pragma unroll
    for (int qb = 0; qb < MAXQ; qb += 8) {  // eight loads in flight, small register peak
      T sv[8];
#pragma unroll
      for (int q = 0; q < 8; q++)
        sv[q] = srow[item_of(max<int64_t>(min<int64_t>(wbeg + 64 * (qb + q) + ln, n_cand - 1), 0))];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const bool live = wbeg + 64 * (qb + q) + ln < wend;
        const uint64_t k = (!live || is_neg_inf(sv[q])) ? KEY_SKIP : order_key(sv[q]);
        kreg[qb + q] = static_cast<KeyT>(k);
        local += k != KEY_SKIP;
        tmax = (k != KEY_SKIP && k > tmax) ? k : tmax;
      }
    }
  } else {
    for (int64_t base = 0; base < n_cand; base += NT * 8) {
      T sv[8];
#pragma unroll
      for (int q = 0; q < 8; q++)
        sv[q] = srow[item_of(min<int64_t>(base + q * NT + tid, n_cand - 1))];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const int64_t j = base + q * NT + tid;
        if (j < n_cand) {
          const uint64_t k = is_neg_inf(sv[q]) ? KEY_SKIP : order_key(sv[q]);
          if (CACHED) keys[j] = static_cast<KeyT>(k);
          local += k != KEY_SKIP;
          tmax = (k != KEY_SKIP && k > tmax) ? k : tmax;
        }
      }
    }
  }
  // visit every slot of this wave, all lanes together (f may use wave-wide ballots); f
  // returns false to stop early (a wave-uniform decision)
  auto for_each_slot = [&](auto &&f) {
    if constexpr (MODE == 2) {
      bool go = true;
#pragma unroll
      for (int q = 0; q < MAXQ; q++)
        if (go && wbeg + 64 * q < wend) go = f(wbeg + 64 * q + ln, static_cast<uint64_t>(kreg[q]));
    } else {
      for (int64_t base = wbeg; base < wend; base += 64) {
        const int64_t j = base + ln;
        if (!f(j, j < wend ? key_at(j) : KEY_SKIP)) break;
      }
    }
  };
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) local += __shfl_xor(local, o, 64);
  if (ln == 0) scan_buf[wv] = local;
  if (tid < 256) hist[tid] = 0;
  __syncthreads();
  int n_rankable = 0;
  for (int w = 0; w < NWV; w++) n_rankable += scan_buf[w];
  __syncthreads();
  const int n_rec = min(p.cutoff, n_rankable);
  res.valid = 1;
  res.n_rec = n_rec;
  if (n_rec == 0) {  // :132-135
    if (tid == 0) p.out[orow] = res;
    return;
  }

  // --- short lists (the usual cutoffs): the n_rec-th largest of the per-thread maxima is a
  //     lower bound L of the n_rec-th largest key (those maxima are n_rec different keys
  //     >= L).  L costs a radix select over ONE key per thread, and the keys >= L - the
  //     n_rec winners, all their ties and a few more - are gathered in one sweep and
  //     sorted exactly by (key desc, index asc) below.  Rows where that list does not fit
  //     (e.g. thousands of equal scores) take the general selection.
  constexpr int BITS = KeyBits<T>::value;
  int n_sel = n_rec;  // entries in sel_key / sel_idx; the best n_rec of them are the result
  bool fast = n_rec <= NT;
  if (fast) {
    uint64_t lpre = 0;
    int lneed = n_rec;
    for (int shift = BITS - 8; shift >= 0; shift -= 8) {
      const uint64_t hi_mask = (shift + 8 >= 64) ? 0ull : (~0ull << (shift + 8));
      const bool in = (tmax & hi_mask) == (lpre & hi_mask);
      const uint32_t digit = static_cast<uint32_t>(tmax >> shift) & 0xffu;
      const unsigned long long todo = __ballot(in);
      if (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const uint32_t d = __builtin_amdgcn_readlane(digit, leader);
        const unsigned long long same = __ballot(in && digit == d);
        if (same == todo) {
          if (ln == leader) atomicAdd(&hist[d], static_cast<uint32_t>(__popcll(same)));
        } else if (in) {
          atomicAdd(&hist[digit], 1u);
        }
      }
      __syncthreads();
      int bin = 0, incl = 0;
      if (tid < 256) {
        bin = static_cast<int>(hist[255 - tid]);
        incl = bin;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(incl, o, 64);
          if (ln >= o) incl += t;
        }
        if (ln == 63) scan_buf[wv] = incl;
      }
      __syncthreads();
      if (tid < 256) {
        for (int w = 0; w < wv && w < 4; w++) incl += scan_buf[w];
        if (incl - bin < lneed && incl >= lneed) {
          sh_prefix = lpre | (static_cast<uint64_t>(255 - tid) << shift);
          sh_need = (incl == lneed) ? -1 : lneed - (incl - bin);
        }
        hist[tid] = 0;
      }
      __syncthreads();
      lpre = sh_prefix;
      lneed = sh_need;
      if (lneed < 0) break;  // the whole bin is wanted: its lowest possible key bounds L
    }
    const uint64_t L = lpre;
    if (tid == 0) sh_count = 0;
    __syncthreads();
    for_each_slot([&](int64_t j, uint64_t k) {
      if (k != KEY_SKIP && k >= L) {
        const int pos = atomicAdd(&sh_count, 1);
        if (pos < sel_cap) {
          sel_key[pos] = k;
          sel_idx[pos] = sel_of(j);
        }
      }
      return true;
    });
    __syncthreads();
    n_sel = sh_count;
    fast = n_sel <= sel_cap;
    __syncthreads();  // sh_count is reset by the general selection
  }
  if (!fast) {
  n_sel = n_rec;
  // --- radix select: key of the n_rec-th best candidate
  uint64_t prefix = 0;
  int need = n_rec;  // how many still to take among keys matching `prefix` so far
  bool inclusive = false;  // true: every key >= prefix is taken and there is no tie pick
  // hist is zero here (cleared before the count barrier) and is cleared again by the bin scan
  // of every pass: three barriers per digit
  for (int shift = BITS - 8; shift >= 0; shift -= 8) {
    const uint64_t hi_mask = (shift + 8 >= 64) ? 0ull : (~0ull << (shift + 8));
    for_each_slot([&](int64_t, uint64_t k) {
      const bool in = k != KEY_SKIP && (k & hi_mask) == (prefix & hi_mask);
      const uint32_t digit = static_cast<uint32_t>(k >> shift) & 0xffu;
      // scores share their leading byte(s): when all candidate lanes of a wave fall into
      // one bin a single lane adds the count (no same-address atomic storm); otherwise
      // the digits are spread and per-lane atomics are cheap
      const unsigned long long todo = __ballot(in);
      if (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const uint32_t d = __builtin_amdgcn_readlane(digit, leader);
        const unsigned long long same = __ballot(in && digit == d);
        if (same == todo) {
          if (ln == leader) atomicAdd(&hist[d], static_cast<uint32_t>(__popcll(same)));
        } else if (in) {
          atomicAdd(&hist[digit], 1u);
        }
      }
      return true;
    });
    __syncthreads();
    // the digit d with  #(digits > d) < need <= #(digits >= d): bins scanned in descending
    // order by the first four waves
    int bin = 0, incl = 0;
    if (tid < 256) {
      bin = static_cast<int>(hist[255 - tid]);
      incl = bin;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (ln >= o) incl += t;
      }
      if (ln == 63) scan_buf[wv] = incl;
    }
    __syncthreads();
    if (tid < 256) {
      for (int w = 0; w < wv; w++) incl += scan_buf[w];
      if (incl - bin < need && incl >= need) {
        sh_prefix = prefix | (static_cast<uint64_t>(255 - tid) << shift);
        // the whole bin is wanted: no lower digit has to be resolved (-1 stops the loop)
        sh_need = (incl == need) ? -1 : need - (incl - bin);
      }
      hist[tid] = 0;  // every bin was read before the barrier above
    }
    __syncthreads();
    // (the next write to sh_prefix / sh_need sits two barriers ahead: no barrier after the read)
    prefix = sh_prefix;
    need = sh_need;
    if (need < 0) {
      inclusive = true;
      need = 0;
      break;
    }
  }
  const uint64_t thr = prefix;  // threshold key; `need` ties at thr are taken, lowest index first

  // --- gather winners ((wave, slot, lane) order is index order): sweep 1 appends the keys
  //     above the threshold and counts the wave's ties, sweep 2 gives the `need` lowest-index
  //     ties their slots (evaluator.cpp:329, 353-355)
  if (tid == 0) sh_count = 0;
  __syncthreads();
  int my_ties = 0;
  for_each_slot([&](int64_t j, uint64_t k) {
    bool tie = false;
    if (k != KEY_SKIP) {
      if (inclusive ? k >= thr : k > thr) {
        const int pos = atomicAdd(&sh_count, 1);
        sel_key[pos] = k;
        sel_idx[pos] = sel_of(j);
      } else if (k == thr) {
        tie = true;
      }
    }
    my_ties += __popcll(__ballot(tie));
    return true;
  });
  if (ln == 0) scan_buf[wv] = my_ties;
  __syncthreads();
  int seen = 0;
  for (int w = 0; w < wv; w++) seen += scan_buf[w];
  for_each_slot([&](int64_t j, uint64_t k) {
    if (seen >= need) return false;
    const bool tie = k != KEY_SKIP && k == thr;
    const unsigned long long bal = __ballot(tie);
    const int rank = seen + __popcll(bal & ((1ull << ln) - 1ull));
    if (tie && rank < need) {
      const int pos = atomicAdd(&sh_count, 1);
      sel_key[pos] = k;
      sel_idx[pos] = sel_of(j);
    }
    seen += __popcll(bal);
    return true;
  });
  __syncthreads();
  }  // general selection
  if (n_sel <= 64) {
    // --- common cutoffs: one wave finishes the row without further barriers.  Lane i holds
    //     candidate i (the best n_rec of the n_sel gathered ones are the list); bitonic network
    //     over the lanes (key desc, index asc), hits by binary search, then the sequential
    //     dcg / AP recurrences of Metrics::update (:136-165).
    if (wv != 0) return;
    uint64_t mk = ln < n_sel ? sel_key[ln] : 0ull;
    int32_t mi = ln < n_sel ? sel_idx[ln] : 0x7fffffff;
#pragma unroll
    for (int k2 = 2; k2 <= 64; k2 <<= 1) {
#pragma unroll
      for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
        const uint64_t ok = __shfl_xor(static_cast<unsigned long long>(mk), j2, 64);
        const int32_t oi = __shfl_xor(mi, j2, 64);
        const bool mine_first = (mk != ok) ? mk > ok : mi < oi;
        const bool lower = (ln & j2) == 0, up = (ln & k2) == 0;
        const bool keep = (lower == up) ? mine_first : !mine_first;
        mk = keep ? mk : ok;
        mi = keep ? mi : oi;
      }
    }
    if (p.retrieve) {
      if (ln < n_rec) rec_row[ln] = POS ? item_of(mi) : mi;
      return;
    }
    bool hit = false;
    if (ln < n_rec) rec_row[ln] = mi;  // (counted by item_hist_kernel, :146)
    if (n_gt <= 64) {
      // short ground-truth row (prefetched at kernel start): compare against every entry
      // instead of a chain of dependent loads
      for (int c = 0; c < n_gt; c++) hit |= __builtin_amdgcn_readlane(gt_pref, c) == mi;
      hit = hit && ln < n_rec;
    } else if (ln < n_rec) {
      int lo = gb, hi = ge;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p.gt_idx[mid] < mi) lo = mid + 1; else hi = mid;
      }
      hit = lo < ge && p.gt_idx[lo] == mi;
    }
    const double disc_l = ln < n_rec ? disc_pref : 0.0;
    unsigned long long hits = __ballot(hit);
    double dcg = 0, ap = 0;
    int cum_hit = 0;
    while (hits) {  // ascending rank order, like the reference's loop over the list
      const int i = __ffsll(static_cast<long long>(hits)) - 1;
      hits &= hits - 1;
      dcg += __shfl(disc_l, i, 64);
      cum_hit++;
      ap += static_cast<double>(cum_hit) / (i + 1);
    }
    const double idcg = min(n_gt, n_rec) == min(n_gt, p.cutoff)
                            ? idcg_pref
                            : p.idcg_prefix[min(n_gt, n_rec)];
    res.hit = cum_hit > 0 ? 1.0 : 0.0;
    res.precision = cum_hit / static_cast<double>(n_rec);
    res.recall = cum_hit / static_cast<double>(
                               p.recall_with_cutoff ? (n_gt > n_rec ? n_rec : n_gt) : n_gt);
    res.ndcg = dcg / idcg;
    res.map = ap / n_gt;
    if (ln == 0) p.out[orow] = res;
    return;
  }
  // --- bitonic sort of the n_sel gathered candidates: key desc, index asc
  int n_pow = 1;
  while (n_pow < n_sel) n_pow <<= 1;
  for (int i = n_sel + tid; i < n_pow; i += NT) {
    sel_key[i] = 0ull;
    sel_idx[i] = 0x7fffffff;
  }
  __syncthreads();
  auto before = [&](int a, int b) {  // element a ranks before element b
    if (sel_key[a] != sel_key[b]) return sel_key[a] > sel_key[b];
    return sel_idx[a] < sel_idx[b];
  };
  for (int k2 = 2; k2 <= n_pow; k2 <<= 1) {
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (int i = tid; i < n_pow; i += NT) {
        const int l = i ^ j2;
        if (l > i) {
          const bool up = (i & k2) == 0;
          const bool swap = up ? before(l, i) : before(i, l);
          if (swap) {
            const uint64_t tk = sel_key[i];
            sel_key[i] = sel_key[l];
            sel_key[l] = tk;
            const int32_t ti = sel_idx[i];
            sel_idx[i] = sel_idx[l];
            sel_idx[l] = ti;
          }
        }
      }
      __syncthreads();
    }
  }
  if (p.retrieve) {
    for (int i = tid; i < n_rec; i += NT) rec_row[i] = POS ? item_of(sel_idx[i]) : sel_idx[i];
    return;
  }
  // --- hits, histogram, output list
  for (int i = tid; i < n_rec; i += NT) {
    const int32_t it = sel_idx[i];
    rec_row[i] = it;  // (counted by item_hist_kernel, :146)
    int lo = gb, hi = ge;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p.gt_idx[mid] < it) lo = mid + 1; else hi = mid;
    }
    sel_hit[i] = (lo < ge && p.gt_idx[lo] == it) ? 1 : 0;
  }
  __syncthreads();
  if (wv == 0) {
    // Metrics::update :136-165 in the same sequential order: the wave reads 64 hit flags at a
    // time and walks the set bits in ascending rank (every lane carries the same sums)
    double dcg = 0, ap = 0;
    int cum_hit = 0;
    for (int base = 0; base < n_rec; base += 64) {
      unsigned long long hits = __ballot(base + ln < n_rec && sel_hit[base + ln] != 0);
      while (hits) {
        const int i = base + __ffsll(static_cast<long long>(hits)) - 1;
        hits &= hits - 1;
        dcg += p.disc[i];
        cum_hit++;
        ap += static_cast<double>(cum_hit) / (i + 1);
      }
    }
    const double idcg = p.idcg_prefix[min(n_gt, n_rec)];
    res.hit = cum_hit > 0 ? 1.0 : 0.0;
    res.precision = cum_hit / static_cast<double>(n_rec);
    res.recall = cum_hit / static_cast<double>(
                               p.recall_with_cutoff ? (n_gt > n_rec ? n_rec : n_gt) : n_gt);
    res.ndcg = dcg / idcg;
    res.map = ap / n_gt;
    if (ln == 0) p.out[orow] = res;
  }
}

}  // namespace eval
}  // namespace irs
