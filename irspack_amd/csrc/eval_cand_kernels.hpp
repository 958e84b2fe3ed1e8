// Kernels that rank one user row per WAVE: rank_wave_kernel (a row of scores, cutoff <= 64) and, for the emit path
// of irs_eval_get_metrics_ials, rank_cand_kernel / rank_cand_slow_kernel (a candidate list written by
// score_emit_kernel), with the metrics tail they share.
// (Included by evaluator.hip after eval_rank_kernels.hpp and eval_fused_kernels.hpp: EvalParams, EmitParams.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace irs {
namespace eval {

// ---------------------------------------------------------------------------
// One WAVE per user row, one pass over the scores, no barrier and no LDS: the usual case
// (every item is a candidate, cutoff <= 64).  Lane l streams the scores l, l + 64, ... with
// U loads in flight and keeps its own M best (key, index) pairs sorted in registers.  The
// list is then drawn from the 64 heads: a wave-wide arg-max of (key desc, index asc) per
// rank, the winning lane popping its head; lane i ends up with rank i, exactly the state the
// single-wave finish of rank_rows_kernel starts from.  A lane that runs dry although it saw
// more than M rankable scores may hide a better candidate: the row is then flagged in p.todo
// and ranked by rank_rows_kernel (for cutoff 20 and M = 4 about one row in a thousand).
// 8 waves per SIMD are resident, so the loads of some rows overlap the drawing of others.
// Last phase of a wave-ranked row: lane i holds the item of rank i (mi, i < n_rec).  Hits,
// then the SEQUENTIAL dcg / AP recurrences of Metrics::update (evaluator.cpp:136-165) so that
// the fp64 terms are those of the reference.
__device__ __forceinline__ void wave_metrics_tail(const EvalParams &p, int64_t row, int ln,
                                                  int32_t mi, int n_rec, int gb, int ge, int n_gt,
                                                  int32_t gt_pref, double disc_pref,
                                                  double idcg_pref, RowOut res, int32_t *rec_row) {
  if (p.retrieve) {
    if (ln < n_rec) rec_row[ln] = mi;
    return;
  }
  bool hit = false;
  if (ln < n_rec) rec_row[ln] = mi;  // (counted by item_hist_kernel, :146)
  if (n_gt <= 64) {
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
  while (hits) {  // ascending rank order, like the reference's loop over the list (:136-165)
    const int i = __ffsll(static_cast<long long>(hits)) - 1;
    hits &= hits - 1;
    dcg += __shfl(disc_l, i, 64);
    cum_hit++;
    ap += static_cast<double>(cum_hit) / (i + 1);
  }
  const double idcg = min(n_gt, n_rec) == min(n_gt, p.cutoff) ? idcg_pref
                                                              : p.idcg_prefix[min(n_gt, n_rec)];
  res.hit = cum_hit > 0 ? 1.0 : 0.0;
  res.precision = cum_hit / static_cast<double>(n_rec);
  res.recall = cum_hit / static_cast<double>(
                             p.recall_with_cutoff ? (n_gt > n_rec ? n_rec : n_gt) : n_gt);
  res.ndcg = dcg / idcg;
  res.map = ap / n_gt;
  if (ln == 0) p.out[row] = res;
}

// Emit path, last kernel: one wave per user ranks its candidate list (score_emit_kernel:
// every unmasked item with score >= tau_u, in arbitrary order) by (score desc, index asc).
// Lane l keeps the M best of the entries l, l + 64, ... sorted in registers, the list is drawn
// from the 64 heads; a lane that runs dry with entries left over may hide a better one: the row
// is then ranked by rank_cand_slow_kernel.
template <int M>
__global__ __launch_bounds__(256) void rank_cand_kernel(EvalParams p, EmitParams f,
                                                        const int32_t *__restrict__ n_masked) {
  const int ln = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + wave_index_in_block();
  if (row >= p.rows) return;
  const int64_t u = row + p.offset;
  RowOut res{0, 0, 0, 0, 0, 0, 0};
  const int gb = p.gt_ptr[u], ge = p.gt_ptr[u + 1];
  const int n_gt = ge - gb;
  int32_t *rec_row = p.rec_out + row * p.cutoff;
  if (ln < p.cutoff) rec_row[ln] = -1;  // cutoff <= 32
  if (ln == 0) p.todo[row] = 0;
  if (n_gt == 0) {  // counted in total_user only (:316-321)
    if (ln == 0) p.out[row] = res;
    return;
  }
  int32_t gt_pref = -1;
  double disc_pref = 0.0;
  if (n_gt <= 64 && ln < n_gt) gt_pref = p.gt_idx[gb + ln];
  if (ln < p.cutoff) disc_pref = p.disc[ln];
  const double idcg_pref = p.idcg_prefix[min(n_gt, p.cutoff)];
  if (f.hard[row]) return;  // ranked from its full score row afterwards
  const int n = min(f.cand_cnt[row], EM_CAP);
  const int64_t n_rankable = f.n_items - (n_masked ? n_masked[row] : 0);
  const int n_rec = static_cast<int>(min<int64_t>(p.cutoff, n_rankable));
  res.valid = 1;
  res.n_rec = n_rec;
  if (n_rec == 0) {  // :132-135
    if (ln == 0) p.out[row] = res;
    return;
  }
  if (n < n_rec) {  // cannot happen with a valid threshold: have the host repeat the call
    if (ln == 0) atomicOr(f.bad_flag, 2);
    if (ln == 0) p.out[row] = res;
    return;
  }
  const float NEG_INF = -std::numeric_limits<float>::infinity();
  const float *cs = f.cand_score + static_cast<size_t>(row) * EM_CAP;
  const int32_t *ci = f.cand_item + static_cast<size_t>(row) * EM_CAP;
  if (n <= 64) {
    // The usual case after pruning (a few dozen candidates): one candidate per lane, its rank
    // = the number of candidates that go before it (score desc, index asc: a strict order, so
    // the ranks are a permutation), counted against every candidate by v_readlane; the item
    // of rank r is then pushed to lane r.
    const float s = ln < n ? cs[ln] : NEG_INF;
    const int32_t i = ln < n ? ci[ln] : 0x7fffffff;
    int rank = 0;
    for (int k = 0; k < n; k++) {  // n is wave-uniform
      const float sk = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), k));
      const int32_t ik = __builtin_amdgcn_readlane(i, k);
      rank += (sk > s || (sk == s && ik < i)) ? 1 : 0;
    }
    if (ln >= n) rank = ln;  // lanes without a candidate keep to themselves
    const int32_t mi = __builtin_amdgcn_ds_permute(rank << 2, i);
    wave_metrics_tail(p, row, ln, mi, n_rec, gb, ge, n_gt, gt_pref, disc_pref, idcg_pref, res, rec_row);
    return;
  }
  float bs[M];
  int32_t bi[M];
#pragma unroll
  for (int t = 0; t < M; t++) {
    bs[t] = NEG_INF;
    bi[t] = 0x7fffffff;
  }
  for (int e0 = 0; e0 < n; e0 += 64) {
    const int e = e0 + ln;
    float s = e < n ? cs[e] : NEG_INF;
    int32_t i = e < n ? ci[e] : 0x7fffffff;
#pragma unroll
    for (int t = 0; t < M; t++) {
      const bool better = s > bs[t] || (s == bs[t] && i < bi[t]);
      const float ts = bs[t];
      const int32_t ti = bi[t];
      bs[t] = better ? s : ts;
      bi[t] = better ? i : ti;
      s = better ? ts : s;
      i = better ? ti : i;
    }
  }
  const int mine_total = (n - ln + 63) / 64;  // entries this lane has seen
  int32_t mi = 0x7fffffff;
  int popped = 0;
  for (int it = 0; it < n_rec; it++) {
    float ws = bs[0];
    int32_t wi = bi[0];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float os = __shfl_xor(ws, o, 64);
      const int32_t oi = __shfl_xor(wi, o, 64);
      const bool better = os > ws || (os == ws && oi < wi);
      ws = better ? os : ws;
      wi = better ? oi : wi;
    }
    if (ln == it) mi = wi;
    if (bi[0] == wi && bs[0] == ws) {  // item ids are unique: one lane
#pragma unroll
      for (int t = 0; t + 1 < M; t++) {
        bs[t] = bs[t + 1];
        bi[t] = bi[t + 1];
      }
      bs[M - 1] = NEG_INF;
      bi[M - 1] = 0x7fffffff;
      popped++;
    }
    if (it + 1 < n_rec && __any(popped == M && mine_total > M)) {
      if (ln == 0) p.todo[row] = 1;
      return;
    }
  }
  wave_metrics_tail(p, row, ln, mi, n_rec, gb, ge, n_gt, gt_pref, disc_pref, idcg_pref, res, rec_row);
}

// The rows rank_cand_kernel flagged: exact rank of every candidate by counting (LDS copy).
__global__ __launch_bounds__(256) void rank_cand_slow_kernel(EvalParams p, EmitParams f,
                                                             const int32_t *__restrict__ n_masked) {
  __shared__ float cs[4][EM_CAP];
  __shared__ int32_t ci[4][EM_CAP];
  __shared__ int32_t sel[4][64];
  const int ln = threadIdx.x & 63, wv = wave_index_in_block();
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + wv;
  if (row >= p.rows || p.todo[row] == 0) return;
  const int64_t u = row + p.offset;
  RowOut res{0, 0, 0, 0, 0, 0, 0};
  const int gb = p.gt_ptr[u], ge = p.gt_ptr[u + 1];
  const int n_gt = ge - gb;
  int32_t *rec_row = p.rec_out + row * p.cutoff;
  int32_t gt_pref = -1;
  double disc_pref = 0.0;
  if (n_gt <= 64 && ln < n_gt) gt_pref = p.gt_idx[gb + ln];
  if (ln < p.cutoff) disc_pref = p.disc[ln];
  const double idcg_pref = p.idcg_prefix[min(n_gt, p.cutoff)];
  const int n = min(f.cand_cnt[row], EM_CAP);
  const int64_t n_rankable = f.n_items - (n_masked ? n_masked[row] : 0);
  const int n_rec = static_cast<int>(min<int64_t>(p.cutoff, n_rankable));
  res.valid = 1;
  res.n_rec = n_rec;
  for (int e = ln; e < n; e += 64) {
    cs[wv][e] = f.cand_score[static_cast<size_t>(row) * EM_CAP + e];
    ci[wv][e] = f.cand_item[static_cast<size_t>(row) * EM_CAP + e];
  }
  __threadfence_block();
  for (int e = ln; e < n; e += 64) {
    const float s = cs[wv][e];
    const int32_t i = ci[wv][e];
    int rank = 0;
    for (int k = 0; k < n; k++) {
      const float sk = cs[wv][k];
      const int32_t ik = ci[wv][k];
      rank += (sk > s || (sk == s && ik < i)) ? 1 : 0;
    }
    if (rank < n_rec) sel[wv][rank] = i;
  }
  __threadfence_block();
  const int32_t mi = ln < n_rec ? sel[wv][ln] : 0x7fffffff;
  wave_metrics_tail(p, row, ln, mi, n_rec, gb, ge, n_gt, gt_pref, disc_pref, idcg_pref, res, rec_row);
}

template <class T, int M>
__global__ __launch_bounds__(256) void rank_wave_kernel(EvalParams p) {
  constexpr int U = 16;
  const int ln = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + wave_index_in_block();
  if (row >= p.rows) return;
  const int64_t orow = p.row_map ? p.row_map[row] : row;
  const int64_t u = orow + p.offset;
  const T *srow = static_cast<const T *>(p.scores) + row * p.n_items;
  RowOut res{0, 0, 0, 0, 0, 0, 0};
  const int gb = p.retrieve ? 0 : p.gt_ptr[u], ge = p.retrieve ? 0 : p.gt_ptr[u + 1];
  const int n_gt = ge - gb;
  int32_t *rec_row = p.rec_out + orow * p.cutoff;
  if (ln < p.cutoff) rec_row[ln] = -1;  // cutoff <= 64
  if (ln == 0) p.todo[row] = 0;
  if (n_gt == 0 && !p.retrieve) {  // counted in total_user only (:316-321)
    if (ln == 0) p.out[orow] = res;
    return;
  }
  int32_t gt_pref = -1;
  double disc_pref = 0.0, idcg_pref = 0.0;
  if (!p.retrieve) {
    if (n_gt <= 64 && ln < n_gt) gt_pref = p.gt_idx[gb + ln];
    if (ln < p.cutoff) disc_pref = p.disc[ln];
    idcg_pref = p.idcg_prefix[min(n_gt, p.cutoff)];
  }
  // The lists hold the raw scores: float comparison is the reference's order (-0.0 == +0.0
  // ties; equal scores keep index order because insertion is strict), -inf marks an empty
  // slot and is never inserted - exactly the scores that are not rankable.  A NaN (ranks last
  // among the rankable, evaluator.hip header) would never be inserted either, so a row that
  // contains one goes to the general kernel.
  const T NEG_INF = -std::numeric_limits<T>::infinity();
  T bs[M];
  int32_t bi[M];
#pragma unroll
  for (int t = 0; t < M; t++) {
    bs[t] = NEG_INF;
    bi[t] = 0x7fffffff;
  }
  int n_rankable = 0;             // wave-uniform
  unsigned long long nan_any = 0;  // lanes that met a NaN
  const int32_t n = static_cast<int32_t>(p.n_items);
  auto insert = [&](T cs, int32_t ci) {
    if (__any(cs > bs[M - 1])) {
      // from the first entry the new score beats, the tail SHIFTS down one place (sticky
      // `gt`): an entry pushed down by one place still goes before its equals, whose
      // indices are higher
      bool gt = false;
#pragma unroll
      for (int t = 0; t < M; t++) {
        gt = gt || cs > bs[t];
        const T ts = bs[t];
        const int32_t ti = bi[t];
        bs[t] = gt ? cs : ts;
        bi[t] = gt ? ci : ti;
        cs = gt ? ts : cs;
        ci = gt ? ti : ci;
      }
    }
  };
  int32_t base = 0;
  for (; base + 64 * U <= n; base += 64 * U) {  // full groups: no bounds to check
    const T *sp = srow + base + ln;
    T sv[U];
#pragma unroll
    for (int q = 0; q < U; q++) sv[q] = sp[64 * q];
#pragma unroll
    for (int q = 0; q < U; q++) {
      nan_any |= __ballot(sv[q] != sv[q]);
      n_rankable += __popcll(__ballot(sv[q] != NEG_INF));
      insert(sv[q], base + 64 * q + ln);
    }
  }
  if (base < n) {  // the last, partial group
    T sv[U];
#pragma unroll
    for (int q = 0; q < U; q++) sv[q] = srow[min(base + 64 * q + ln, n - 1)];
#pragma unroll
    for (int q = 0; q < U; q++) {
      const int32_t j = base + 64 * q + ln;
      const T s1 = j < n ? sv[q] : NEG_INF;
      nan_any |= __ballot(s1 != s1);
      n_rankable += __popcll(__ballot(s1 != NEG_INF));
      insert(s1, j);
    }
  }
  if (nan_any) {
    if (ln == 0) p.todo[row] = 1;
    return;
  }
  const int n_rec = min(p.cutoff, n_rankable);
  res.valid = 1;
  res.n_rec = n_rec;
  if (n_rec == 0) {  // :132-135
    if (ln == 0) p.out[orow] = res;
    return;
  }
  // --- draw the list: rank `it` is the best head
  int32_t mi = 0x7fffffff;
  int popped = 0;
  for (int it = 0; it < n_rec; it++) {
    T ws = bs[0];
    int32_t wi = bi[0];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const T os = __shfl_xor(ws, o, 64);
      const int32_t oi = __shfl_xor(wi, o, 64);
      const bool better = os > ws || (os == ws && oi < wi);
      ws = better ? os : ws;
      wi = better ? oi : wi;
    }
    if (ln == it) mi = wi;
    const bool mine = bi[0] == wi && bs[0] == ws;  // indices are unique: one lane
    if (mine) {
#pragma unroll
      for (int t = 0; t + 1 < M; t++) {
        bs[t] = bs[t + 1];
        bi[t] = bi[t + 1];
      }
      bs[M - 1] = NEG_INF;
      bi[M - 1] = 0x7fffffff;
      popped++;
    }
    // a lane that ran dry may hide the next best candidate (it kept only its M best)
    if (it + 1 < n_rec && __any(popped == M)) {
      if (ln == 0) p.todo[row] = 1;
      return;
    }
  }
  wave_metrics_tail(p, orow, ln, mi, n_rec, gb, ge, n_gt, gt_pref, disc_pref, idcg_pref, res, rec_row);
}

}  // namespace eval
}  // namespace irs
