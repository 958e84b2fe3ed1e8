// Item-kNN similarity on gfx950: the kernels.  They replace KNN::KNNComputer::compute_similarity /
// compute_similarity_triple (the reference's cpp_source/knn/knn.hpp:43-139) and the
// compute_similarity_imple bodies of knn/similarities.hpp (:29-46, 73-87, 109-130,
// 161-184, 242-250, 326-334) behind include/irspack_amd.h.  Arithmetic is fp64
// like the reference (knn/wrapper.cpp:9).  Host side: knn.hip (the C ABI), knn_host_prep.hpp.
//
// R = target * X_t is a sparse x sparse product whose rows are dense-ish (up to
// N stored entries), so each workgroup owns one (target row, column tile) pair
// and keeps the tile's accumulators plus a "stored entry" bitmap in LDS:
//   1. for every stored (u, y) of the target row (one wave per u), walk the part
//      of X_arg^T's row u that falls in the tile: acc[j] += x * y (LDS integer atomics:
//      32-bit counts when every product is 1, else 64-bit fixed point scaled per target
//      row), touched[j] = 1  - every touched j is a stored entry of the product, exact
//      zeros included (knn.hpp:111-118 ranks stored entries)
//   2. similarity epilogue per touched j (similarities.hpp, the `+ 1e-6` forms),
//      written with explicit non-contracted fp64 ops
//   3. top-k of the tile by (value desc, column asc) (knn.hpp:119-129): radix
//      select on order-preserving 64-bit keys + index-ordered tie pick
// A second kernel merges the tiles of a row, keeps top_k and sorts them by
// column (knn.hpp:130).  Integer adds commute, so no sum - weighted ones included -
// depends on the order in which the atomics land: results are bit-reproducible run to
// run; counts of binary interactions are exact, fixed-point sums are within (product
// count) * 2^-(s+1) of the real sum (see `add` in knn_tile_kernel).
#pragma once
#include "common.hpp"

namespace irs {
namespace knn {
constexpr int TILE = 16384;     // columns per workgroup (128 KB of fp64 accumulators)
constexpr int TOPK_CAP = 2048;  // largest top_k of the LDS row merge (two candidate sets must fit one
                                // round); above it the rows are merged by knn_merge_big_kernel
constexpr int MERGE_CAP = 4096; // candidates a row merge can hold
constexpr int THREADS = 1024;

struct Params {
  // X_arg^T by rows u: (column j, value x) sorted by j; xt_tptr[u * (n_tiles + 1) + t]
  // is the position of the first entry of row u with column >= t * TILE (the last one is
  // the row end), so a (row, tile) workgroup walks exactly its own slice of every row
  const uint32_t *xt_tptr;
  const uint32_t *xt_idx16;  // tile-relative columns, 16 bits each, two per dword
  const double *xt_val;
  // Not null: every feature row u of X_arg^T holds ONE value xt_rowval[u] in all its stored entries
  // (TF-IDF of binary interactions: the weight is the row's idf).  The kernels then run their all-ones
  // form on y' = x_u y - the same products x y, bit for bit - and never read the 8-byte value stream
  // (four fifths of the bytes of a weighted walk).
  const double *xt_rowval;
  const double *norms;  // per column j
  // Not null: the sums of column j are multiplied by col_scale[j] (one rounding) before the similarity's
  // epilogue - the column factor of a SEPARABLE weighting w[u][j] = rowval[u] * col_scale[j] (tf-idf / BM25 of
  // binary interactions, fused at construction: DESIGN 3.4).  Exact kernels only (never FAST).
  const double *col_scale;
  // target rows
  const int64_t *t_ptr;
  const int32_t *t_idx;
  const double *t_val;
  const double *t_stat;       // per target row (norm / pow / count), see epilogue
  const double *t_scale;      // per target row: power of two that maps its products to the
                              // 64-bit fixed-point accumulators (weighted paths); NEGATIVE: the
                              // row's products span a wide range - two limbs, see `hi_stash`
  uint64_t *hi_stash;         // [workgroups x TILE]: the first limbs of a wide-range pair while the
                              // second ones are accumulated
  const int32_t *row_order;   // work-sorted list of target rows of this call
  int32_t n_rows;             // rows in this call
  int32_t n_tiles;
  int32_t N;
  int32_t sim_type;
  int32_t normalize;
  double shrinkage, alpha, beta;
  float shrink_f, alpha_f, beta_f;  // the same rounded to float32 (FAST path: scalar operands, no conversions)
  int32_t top_k;
  int32_t tile_k;      // winners one (row, tile) pair can hold: min(top_k, TILE)
  // per (row slot, tile) winners, in ascending column order
  int32_t *cand_idx;   // [n_rows * n_tiles * tile_k]
  double *cand_val;
  int32_t *cand_cnt;   // [n_rows * n_tiles]
  // final rows
  int32_t *out_idx;    // [n_rows * top_k]
  double *out_val;
  int32_t *out_cnt;    // [n_rows]
  // persistent launch: workgroups draw (row slot, tile) pairs from this counter
  int32_t *cursor;
  int32_t n_slots;     // n_rows * n_tiles
  // FAST: pairs whose candidates did not fit are listed here and taken by a second launch of the
  // exact kernel (redo != 0: the pairs are redo_list[0 .. *redo_count), drawn through cursor[1])
  int32_t *redo_list;
  int32_t *redo_count;
  int32_t redo;
  int32_t merge_cap;   // entries of the merge buffer: power of two, >= 2 * top_k
};

__device__ __forceinline__ int64_t readlane_i64(int64_t v, int src) {
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(v), src);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32), src);
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}
__device__ __forceinline__ double readlane_f64(double v, int src) {
  return __longlong_as_double(readlane_i64(__double_as_longlong(v), src));
}

__device__ __forceinline__ uint64_t order_key(double s) {
  if (s != s) return 0ull;
  if (s == 0.0) s = 0.0;
  uint64_t u = static_cast<uint64_t>(__double_as_longlong(s));
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double key_to_double(uint64_t k) {  // inverse of order_key (non-NaN)
  const uint64_t u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double(static_cast<long long>(u));
}

// similarities.hpp epilogues; operations are kept un-fused so that the value is
// the one a default x86-64 build of the reference computes.
__device__ __forceinline__ double epilogue(const Params &p, double v, double norm_j,
                                           double tstat) {
  const double eps = 1e-6;
  switch (p.sim_type) {
    case IRS_SIM_COSINE:
      if (!p.normalize) return v;
      return __ddiv_rn(v, __dadd_rn(__dadd_rn(__dmul_rn(norm_j, tstat), p.shrinkage), eps));
    case IRS_SIM_ASYMMETRIC:
      return __ddiv_rn(v, __dadd_rn(__dadd_rn(__dmul_rn(norm_j, tstat), p.shrinkage), eps));
    case IRS_SIM_JACCARD:
      // norms(j) + target_norm - v + shrinkage + 1e-6   (left to right)
      return __ddiv_rn(
          v, __dadd_rn(__dadd_rn(__dsub_rn(__dadd_rn(norm_j, tstat), v), p.shrinkage), eps));
    case IRS_SIM_TVERSKY: {
      // itv + beta * (norms(j) - itv) + alpha * (target_norm - itv) + shrinkage + 1e-6
      const double a = __dadd_rn(v, __dmul_rn(p.beta, __dsub_rn(norm_j, v)));
      const double b = __dadd_rn(a, __dmul_rn(p.alpha, __dsub_rn(tstat, v)));
      return __ddiv_rn(v, __dadd_rn(__dadd_rn(b, p.shrinkage), eps));
    }
    default:
      return v;
  }
}

// float32 approximation of `epilogue` for a COUNT v >= 1 (FAST path).  Every term of the
// denominator is non-negative (the host checks shrinkage, alpha, beta >= 0) and the only
// subtractions are of integers below 2^24 (exact in float32) or leave a result no smaller than
// half of their operands' sum, so the relative error stays below ~12 roundings of 2^-24 < 2^-20.
__device__ __forceinline__ float approx_epilogue(const Params &p, float v, float norm_j, float tstat,
                                                 float shrink, float alpha, float beta) {
  if (p.sim_type == IRS_SIM_COSINE && !p.normalize) return v;  // the count itself (exact below 2^24)
  float d;
  switch (p.sim_type) {
    case IRS_SIM_JACCARD: d = (norm_j + tstat) - v; break;
    case IRS_SIM_TVERSKY: d = v + beta * (norm_j - v) + alpha * (tstat - v); break;
    default: d = norm_j * tstat; break;  // cosine (normalised), asymmetric cosine
  }
  d = d + shrink + 1e-6f;
  return v * __builtin_amdgcn_rcpf(d);
}
constexpr int FAST_CAP = 2048;   // candidates the exact ranking of the FAST path holds (32 KB of LDS)
#ifndef IRS_KNN_FAST_SLACK
#define IRS_KNN_FAST_SLACK 96
#endif
constexpr int FAST_SLACK = IRS_KNN_FAST_SLACK;  // the approximate select stops once at most top_k + this many keys remain

// touched-ness of a column without a bitmap atomic: accumulators start at -0.0, and
// -0.0 + x is x for every x that is not itself -0.0, so a column stays at the bit
// pattern of -0.0 exactly when nothing (or only -0.0 products) was added.  The host
// selects this only when no product can be a zero (no stored zeros, no underflow);
// otherwise the bitmap is maintained with atomics next to the sums.
constexpr uint64_t NEG_ZERO_BITS = 0x8000000000000000ull;

#ifdef IRS_KNN_PHASES
__device__ unsigned long long knn_fast_stat[8];  // pairs, exact-path pairs, sum of candidates, pairs with <= 128 / 256 / 512 / 1024 candidates
__device__ unsigned long long knn_phase_clk[8];
#define PHASE_MARK(i) do { if (threadIdx.x == 0) { const unsigned long long t_ = wall_clock64(); atomicAdd(&knn_phase_clk[i], t_ - ph_t); ph_t = t_; } } while (0)
#else
#define PHASE_MARK(i)
#endif

// ACC32 (every stored value of both operands is exactly 1, so every product is 1): the sums
// are counts, accumulated with 32-bit LDS atomics (one bank per lane instead of two: 1.5x the
// fp64 atomic rate) in the upper half of the accumulator block and widened to fp64 in place
// afterwards - the same values as the fp64 sums, which are exact for integers.
// (A COMPACT form of the count path - 512 threads and 66 KB of LDS per workgroup, two workgroups per CU so
// that one pair's epilogue / selection overlaps the other's accumulation - was built in round 3, measured
// at 10.69 against 10.54 ms and kept as an opt-in; removed in round 5.  DESIGN.md 3.4 has the numbers.)
// FAST (round 3; counts only, the four similarities that end in a division): the selection runs
// on float32 APPROXIMATIONS of the similarities (8 vector instructions per column instead of the
// ~45 of the un-fused fp64 epilogue, 32-bit keys), and only the columns that can still be among
// the top_k - approximation within 2^-17 of the top_k-th best approximation - get the exact
// fp64 value and are ranked exactly (value desc, column asc).  With |approx - exact| <=
// eps * exact for every stored column (eps < 2^-20, see approx_epilogue and
// tests/test_knn_approx_bound.py) a column of the exact
// top_k has approx >= t (1 - eps) / (1 + eps), t = the top_k-th largest approximation, so the
// candidate set is a superset of the exact winners whatever the ties; when it does not fit
// FAST_CAP entries (thousands of near-ties) the pair takes the exact path below.
template <bool ONES, bool SENTINEL, bool ACC32 = false, bool FAST = false>
__global__ __launch_bounds__(THREADS, 1) void knn_tile_kernel(Params p) {
  static_assert(!ACC32 || (ONES && SENTINEL), "counts need all-ones operands");
  static_assert(!FAST || ACC32, "the approximate selection is built for the count path");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *acc = reinterpret_cast<double *>(smem);                        // TILE
  uint32_t *bits = reinterpret_cast<uint32_t *>(acc + TILE);             // TILE / 32
  uint32_t *hist = bits + TILE / 32;                                     // 256
  int32_t *wave_cnt = reinterpret_cast<int32_t *>(hist + 256);           // 16
  // one sink per lane for the lanes of a strip that lie outside their slice: the atomic is
  // issued without a branch (ACC32 uses the idle upper half of the accumulator block)
  constexpr uint32_t SINK_BYTES = TILE * 8 + (TILE / 32) * 4 + 256 * 4 + 16 * 4;
  __shared__ uint64_t sh_prefix;
  __shared__ int32_t sh_need, sh_count, sh_total;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int NW = THREADS / 64;
  __shared__ int32_t sh_slot;
  // One workgroup per CU stays resident and draws (row slot, tile) pairs, heaviest rows
  // first, from a global counter: a 1024-thread / 130 KB workgroup costs ~20 us to launch
  // and retire, as much as the whole accumulation of a light row.  The draw for the next
  // pair is issued before the current one is processed, so its latency is hidden.
  int32_t next_slot = 0;
  int32_t *const cursor = p.redo ? p.cursor + 1 : p.cursor;
  const int n_draw = p.redo ? *p.redo_count : p.n_slots;
  if (tid == 0) next_slot = atomicAdd(cursor, 1);
  for (;;) {
  __syncthreads();  // the previous pair is finished by every wave (LDS and sh_* reuse)
  if (tid == 0) {
    sh_slot = next_slot;
    next_slot = atomicAdd(cursor, 1);
  }
  __syncthreads();
  if (sh_slot >= n_draw) break;
  const int bid = p.redo ? p.redo_list[sh_slot] : sh_slot;
  const int slot = bid / p.n_tiles, tile = bid % p.n_tiles;
  const int r = p.row_order[slot];
  const int c0 = tile * TILE, c1 = min(c0 + TILE, p.N);
  const int width = c1 - c0;
#ifdef IRS_KNN_PHASES
  unsigned long long ph_t = wall_clock64();
#endif

  uint32_t *cnt = reinterpret_cast<uint32_t *>(acc);  // ACC32: TILE counters
  const uint32_t *const xt_tptr_l = p.xt_tptr;
  const uint32_t *const xt_idx16_l = p.xt_idx16;
  if (ACC32) {
    for (int i = tid; i < width; i += THREADS) cnt[i] = 0u;
  } else {
    for (int i = tid; i < width; i += THREADS) acc[i] = SENTINEL ? -0.0 : 0.0;
  }
  for (int i = tid; i < TILE / 32; i += THREADS) bits[i] = 0u;
  __syncthreads();
  PHASE_MARK(0);

  // ---- 1. accumulate.  A wave takes 16 stored (u, y) of the target row at a time: lanes
  //      0..15 own one each.  The walk is a chain of dependent loads (t_idx -> slice bounds
  //      -> columns -> LDS atomic), software pipelined three blocks deep; per slice the wave
  //      spends ~16 instructions: positions are 32-bit (nnz < 2^31), bounds travel by
  //      v_readlane, the column fields are stored as LDS byte offsets (column * 4) and the
  //      atomic is issued by every lane (lanes outside the slice add to their sink).
  // Wide-range rows (weights spanning many decades: tf-idf / BM25 / RP3beta powers on large
  // matrices): one scale per row leaves a column whose sum is tiny next to the row's bound with
  // few significant bits.  Their sums are kept in TWO 64-bit limbs - q_hi = round(v 2^s) as always,
  // q_lo = round((v 2^s - q_hi) 2^40) - accumulated in two passes over the same slices into the
  // same LDS block (the first limbs wait in global scratch meanwhile): integer adds, so still
  // independent of the order of arrival, and 2^-40 of the one-limb rounding step.
  const double ts_ = ACC32 ? 1.0 : p.t_scale[r];
  const bool wide = !ACC32 && ts_ < 0.0;
  const double fx_scale = ACC32 ? 1.0 : fabs(ts_);
  int pass = 0;
  auto add = [&](uint32_t off4, bool ok, double v) {
    if (ACC32) {
      // (lanes outside their slice are masked off - v_cmp + exec save / restore on the scalar unit,
      // no branch: one vector instruction fewer per atomic than selecting a per-lane sink
      // address, 8.77 -> 8.35 ms per ML-20M call)
      if (ok) atomicAdd(reinterpret_cast<uint32_t *>(smem + off4), 1u);
    } else {
      // Weighted products are summed in 64-bit FIXED POINT (v * 2^s rounded to an integer, s
      // per target row such that the row's largest possible sum stays below 2^61): integer
      // adds commute, so the sums - and with them the top-k - do not depend on the order in
      // which the LDS atomics land, run to run.  |error| of a column <= (its product count)
      // * 2^-(s+1).  With the sentinel (positive data) a product never rounds to 0: the
      // column must leave the "untouched" pattern.
      const uint32_t a = ok ? 2 * off4 : SINK_BYTES + 8 * lane;
      const double scaled = v * fx_scale;  // (a power of two: exact)
      long long q = __double2ll_rn(scaled);
      if (SENTINEL) q = q == 0 ? 1 : q;
      // second limb: what the first one left out (|scaled - q| <= 1; above 2^53 both are the same integer)
      if (pass == 1) q = __double2ll_rn((scaled - static_cast<double>(q)) * 0x1p40);
      atomicAdd(reinterpret_cast<unsigned long long *>(smem + a), static_cast<unsigned long long>(q));
      if (!SENTINEL && ok && pass == 0) {
        const uint32_t j = off4 >> 2, bit = 1u << (j & 31);
        if (!(bits[j >> 5] & bit)) atomicOr(&bits[j >> 5], bit);
      }
    }
  };
  const int64_t tb = p.t_ptr[r], te = p.t_ptr[r + 1];
  const int tp_stride = p.n_tiles + 1;
  const int64_t stride = 16 * NW;
  // every load below is unconditional (clamped address, result masked afterwards): a load
  // under a branch makes hipcc drain the whole vector-memory queue (s_waitcnt vmcnt(0))
  // right behind it, which would serialise the pipeline
  auto load_uy = [&](int64_t q0, int64_t &u, double &y, bool &v) {
    const int64_t q = q0 + lane;
    v = lane < 16 && q < te;
    const int64_t qc = min(q, te - 1);  // te > tb here
    u = p.t_idx[qc];
    y = ACC32 ? 1.0 : p.t_val[qc];  // ACC32: the value stream is not uploaded
    if (!ACC32 && ONES && p.xt_rowval != nullptr) y = __dmul_rn(p.xt_rowval[u], y);
  };
  auto load_bounds = [&](int64_t u, bool v, uint32_t &lo, int &len) {
    const uint32_t *tp = xt_tptr_l + u * tp_stride + tile;
    lo = tp[0];
    uint32_t hi = tp[1];
    asm volatile("" : "+v"(hi));  // keep the load out of the select below (see above)
    len = v ? static_cast<int>(hi - lo) : 0;
  };
  // Columns are stored tile-relative in 16 bits, two per dword: lane l of a strip takes the
  // entries a + 2l and a + 2l + 1 (a = slice start rounded down to even), so one 256-byte
  // wave load covers 128 entries of a slice.  The 16 slices of a block are cut into such
  // strips and the strips are processed in batches of 16 (16 loads in flight, then 32
  // atomics), whatever slice they belong to: lanes 0..15 each describe one strip of the
  // batch (first dword, offset of its first entry in the slice, slice length, y) by a
  // binary search in the running strip count of the block.
  struct Block {   // per-lane (0..15) state of one block of 16 stored (u, y)
    uint32_t lo;   // slice start in xt_idx16 / xt_val (entries)
    int len;       // slice length, 0 past the end of the row
    double y;
    int pin;       // inclusive prefix of the strip counts over lanes 0..15
    int total, nb; // strips, batches (wave-uniform)
  };
  auto count_strips = [&](Block &bk) {
    const int ns = bk.len > 0 ? (bk.len + static_cast<int>(bk.lo & 1u) + 127) >> 7 : 0;
    int pin = lane < 16 ? ns : 0;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const int t = __shfl_up(pin, o, 64);
      if (lane >= o) pin += t;
    }
    bk.pin = pin;
    bk.total = __builtin_amdgcn_readlane(pin, 15);
    bk.nb = max(1, (bk.total + 15) >> 4);
  };
  struct Batch {  // per-lane (0..15): one strip
    uint32_t dw;  // first dword of the strip in xt_idx16
    uint32_t ol;  // (slice length << 16) | (slice offset of the strip's first entry + 1): both are at
                  // most TILE, the offset is -1 when the slice starts odd, the length 0 without a strip
                  // - one word, one v_readlane per strip instead of two
    double y;
  };
  auto make_batch = [&](uint32_t lo, int len, double y, int pin, int total, int j) {
    const int m = 16 * j + (lane & 15);
    int u = 0;  // smallest slice with pin[u] > m
#pragma unroll
    for (int step = 8; step >= 1; step >>= 1) {
      const int t = __shfl(pin, u + step - 1, 64);
      if (t <= m) u += step;
    }
    u = min(u, 15);
    const int before = __shfl(pin, max(u - 1, 0), 64);
    const int sidx = m - (u > 0 ? before : 0);
    const uint32_t lo_u = __shfl(lo, u, 64);
    Batch bt;
    // (strip loads that start on 128-byte lines were timed - wrong sums, same 8.45 ms: the line
    // traffic of the unaligned strips is not what bounds the accumulation)
    bt.dw = (lo_u >> 1) + 64u * static_cast<uint32_t>(sidx);
    const uint32_t o0p1 = static_cast<uint32_t>(128 * sidx + 1) - (lo_u & 1u);
    // (shuffles stay outside conditionals: ds_bpermute returns 0 from an inactive source lane)
    const int len_u = __shfl(len, u, 64);
    bt.ol = m < total ? ((static_cast<uint32_t>(len_u) << 16) | o0p1) : 0u;
    bt.y = ACC32 ? 1.0 : __shfl(y, u, 64);
    if (!(m < total)) bt.dw = lo_u >> 1;  // a valid address for the (ignored) load
    return bt;
  };
  auto issue_idx = [&](const Batch &bt, uint32_t (&w)[16]) {
#pragma unroll
    for (int t = 0; t < 16; t++) {
      // (uniform strip pointer + lane: one 64-bit shift-add on a precomputed per-lane base; the
      // 32-bit index `dw + lane` cost an add and a 64-bit scale per strip)
      const uint32_t dw = __builtin_amdgcn_readlane(bt.dw, t);
      const uint32_t *strip = xt_idx16_l + dw;
      w[t] = strip[lane];  // padded arrays
    }
  };
  auto accumulate = [&](const Batch &bt, const uint32_t (&w)[16]) {
    constexpr int SUB = ONES ? 16 : 8;  // the value stream costs 4 registers per strip
#pragma unroll
    for (int h = 0; h < 16; h += SUB) {
      double xa[ONES ? 1 : SUB], xb[ONES ? 1 : SUB];
      if (!ONES) {
#pragma unroll
        for (int t = 0; t < SUB; t++) {
          const uint32_t dw = __builtin_amdgcn_readlane(bt.dw, h + t);
          const double2 xv = *reinterpret_cast<const double2 *>(
              p.xt_val + 2u * (dw + static_cast<uint32_t>(lane)));
          xa[t] = xv.x;
          xb[t] = xv.y;
        }
      }
#pragma unroll
      for (int t = 0; t < SUB; t++) {
        // (a scalar fast path for strips that lie wholly inside their slice - no lane masks - was
        // tried in round 3: 10.58 -> 11.48 ms; the branch per strip costs the counted vmcnt waits)
        const uint32_t ol = __builtin_amdgcn_readlane(bt.ol, h + t);
        const int o = (2 * lane - 1) + static_cast<int>(ol & 0xffffu);
        const int ln = static_cast<int>(ol >> 16);
        const uint32_t wd = w[h + t];
        const bool oka = static_cast<uint32_t>(o) < static_cast<uint32_t>(ln);
        const bool okb = o < ln - 1;
        // ONES: x == 1 exactly, x * y == y and the value stream is never read
        const double y_t = ACC32 ? 1.0 : readlane_f64(bt.y, h + t);
        add(wd & 0xffffu, oka, ONES ? y_t : __dmul_rn(xa[ONES ? 0 : t], y_t));
        add(wd >> 16, okb, ONES ? y_t : __dmul_rn(xb[ONES ? 0 : t], y_t));
      }
    }
  };
  // Pipeline: while batch b is added, the column words of batch b + 1 are in flight, and so
  // are the slice bounds of block k + 2 and the (u, y) of block k + 3.  The block-level
  // loads are issued with every batch (their results are used when the block advances): a
  // load under a branch would make hipcc drain the queue.
  const int64_t q00 = tb + 16 * wv;
  uint64_t *const stash = ACC32 ? nullptr : p.hi_stash + static_cast<size_t>(blockIdx.x) * TILE;
  for (pass = 0; pass < (wide ? 2 : 1); pass++) {
  if (!ACC32 && pass == 1) {  // first limbs out, accumulators back to zero
    __syncthreads();
    for (int i = tid; i < width; i += THREADS) {
      stash[i] = static_cast<uint64_t>(__double_as_longlong(acc[i]));
      acc[i] = 0.0;
    }
    __syncthreads();
  }
  if (q00 < te) {
    Block A, B;
    int64_t uA, uB, uC;
    double yC;
    bool vA, vB, vC;
    load_uy(q00, uA, A.y, vA);
    load_uy(q00 + stride, uB, B.y, vB);
    load_uy(q00 + 2 * stride, uC, yC, vC);
    load_bounds(uA, vA, A.lo, A.len);
    load_bounds(uB, vB, B.lo, B.len);
    count_strips(A);
    count_strips(B);
    Batch cur = make_batch(A.lo, A.len, A.y, A.pin, A.total, 0);
    uint32_t w0[16], w1[16];
    issue_idx(cur, w0);
    int j = 0;
    int64_t q0 = q00;
    // one batch: issue the next batch's words into `wn`, add the current one from `wc`; the two
    // buffers swap roles by calling it twice per trip (no 16-register copy per batch).  Returns
    // true when the row is finished.
    auto one_batch = [&](uint32_t (&wc)[16], uint32_t (&wn)[16]) -> bool {
      const bool adv = j + 1 >= A.nb;  // wave-uniform
      // The block-level loads (slice bounds of block k + 2, (u, y) of block k + 3) are issued HERE,
      // every iteration, and consumed in `if (adv)` after the batch has been added.  (Earlier
      // versions pinned them with an `asm("" : "+v")` use, which made the wave wait for them
      // on the spot - s_waitcnt vmcnt(0) at the top of the loop.  Without it the compiler keeps
      // them here and waits at the use; the measured time is the same, 8.45 ms: the loop is not
      // bound by that round trip either.)
      const uint32_t *tpN = xt_tptr_l + uC * tp_stride + tile;
      const uint32_t loN = tpN[0], hiN = tpN[1];
      const int64_t qD = q0 + 3 * stride + lane;
      const bool vD = lane < 16 && qD < te;
      const int64_t qDc = min(qD, te - 1);
      const int64_t uD = p.t_idx[qDc];
      double yD = 1.0;
      if (!ACC32) {
        yD = p.t_val[qDc];
        if (ONES && p.xt_rowval != nullptr) yD = __dmul_rn(p.xt_rowval[uD], yD);  // (as in load_uy)
      }
      const int jn = adv ? 0 : j + 1;
      const Batch nxt = make_batch(adv ? B.lo : A.lo, adv ? B.len : A.len, adv ? B.y : A.y,
                                   adv ? B.pin : A.pin, adv ? B.total : A.total, jn);
      issue_idx(nxt, wn);
      accumulate(cur, wc);
      if (adv) {
        A = B;
        B.lo = loN;
        B.len = vC ? static_cast<int>(hiN - loN) : 0;
        B.y = yC;
        count_strips(B);
        uC = uD;
        yC = yD;
        vC = vD;
        q0 += stride;
        if (q0 >= te) return true;
      }
      j = jn;
      cur = nxt;
      return false;
    };
    for (;;) {
      if (one_batch(w0, w1)) break;
      if (one_batch(w1, w0)) break;
    }
  }
  }  // pass
  // (the column norms of this thread's first eight columns are fetched while the slower
  // waves finish accumulating)
  constexpr int PER = TILE / THREADS;  // 16
  // (opaque to the optimiser: everything derived from it - 16 column offsets, their clamped
  // forms, LDS addresses - would otherwise be hoisted out of the persistent loop and held in
  // registers across the accumulation, which has none to spare)
  int cbase_ = wv * (PER * 64) + lane;
  asm volatile("" : "+v"(cbase_));
  const int cbase = cbase_;
  // (FAST: all sixteen - the accumulation's registers are dead by now - and the exact path of a
  // FAST kernel reloads its own)
  double nrm0[FAST ? PER : 8];
#pragma unroll
  for (int k = 0; k < (FAST ? PER : 8); k++) nrm0[k] = p.norms[c0 + min(cbase + 64 * k, width - 1)];
  __syncthreads();
  PHASE_MARK(1);

  // ---- 2. epilogue.  Thread (wave w, lane l) owns the columns w * 1024 + 64 k + l,
  //      k = 0..15, so (wave, k, lane) order is column order.  The similarity of every stored
  //      entry is written back (the winners' values are read from there) and its
  //      order-preserving key stays in registers: the selection below never reads LDS keys.
  static_assert(PER * THREADS == TILE && PER <= 32 && PER % 8 == 0, "column ownership (the `have` mask is 32 bits)");
  const double tstat = p.t_stat[r];
  const double fx_inv = 1.0 / fx_scale;  // a power of two: exact
  uint32_t have = 0;  // bit k: column k of this thread is a stored entry of the product row
  int32_t *cidx = p.cand_idx + static_cast<size_t>(bid) * p.tile_k;
  double *cval = p.cand_val + static_cast<size_t>(bid) * p.tile_k;
  bool fast_done = false;
  if constexpr (FAST) {
    // ---- 2F. approximate similarities (float32) of the stored columns: positive, so their bit
    //      patterns order like the values
    //      (the counters stay where they are, in the lower half of the accumulator block: the
    //      candidate list below lives in the upper half, and the exact path re-reads them)
    uint32_t k32[PER];
    int local_bad = 0;
    {
      const float tstat_f = static_cast<float>(tstat), shrink_f = p.shrink_f;
      const float alpha_f = p.alpha_f, beta_f = p.beta_f;
#pragma unroll
      for (int k = 0; k < PER; k++) {
        const int i = cbase + 64 * k;
        const uint32_t c32 = cnt[min(i, TILE - 1)];
        const bool st = i < width && c32 != 0u;
        if (st) have |= 1u << k;
        const float a = approx_epilogue(p, static_cast<float>(c32), static_cast<float>(nrm0[FAST ? k : 0]), tstat_f,
                                        shrink_f, alpha_f, beta_f);
        k32[k] = st ? __float_as_uint(a) : 0u;
        // (safety net behind the host's checks: a stored column whose approximation is not a
        // positive normal number - the error bound does not cover it - sends the pair to the
        // exact kernel)
        if (st && !(a >= 1.17549435e-38f && a <= 3.0e38f)) local_bad = 1;
      }
    }
    // (barriers are most of what is left of a pair's fixed cost: the statistics have their own
    // LDS words, the histogram is returned to zero by the wave that scans it, and the candidates
    // are counted by the compaction itself - two barriers per digit pass, five around them)
    __shared__ uint32_t f_and[16], f_or[16];
    __shared__ int32_t f_cnt[16];
    uint32_t a_and = ~0u, a_or = 0u;
#pragma unroll
    for (int k = 0; k < PER; k++) {
      if ((have >> k) & 1u) {
        a_and &= k32[k];
        a_or |= k32[k];
      }
    }
    int local = __popc(have);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      local += __shfl_xor(local, o, 64);
      a_and &= __shfl_xor(a_and, o, 64);
      a_or |= __shfl_xor(a_or, o, 64);
    }
    local_bad = __any(local_bad) ? 1 : 0;
    if (lane == 0) {
      f_and[wv] = a_and;
      f_or[wv] = a_or;
      f_cnt[wv] = local | (local_bad << 30);
    }
    if (tid < 256) hist[tid] = 0;
    if (tid == 0) sh_count = 0;
    __syncthreads();
    int n_stored = 0;
    a_and = ~0u;
    a_or = 0u;
    int any_bad = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      n_stored += f_cnt[w] & 0x3fffffff;
      any_bad |= f_cnt[w] >> 30;
      a_and &= f_and[w];
      a_or |= f_or[w];
    }
    if (any_bad) {  // (block-uniform)
      if (tid == 0) p.redo_list[atomicAdd(p.redo_count, 1)] = bid;
      continue;
    }
    const int n_sel = min(p.top_k, n_stored);
    if (n_sel == 0) {  // (block-uniform; the next pair starts with a barrier)
      if (tid == 0) p.cand_cnt[bid] = 0;
      continue;
    }
    PHASE_MARK(3);
    // ---- 3F. a lower bound `prefix` of the n_sel-th largest approximation: the radix select of
    //      the exact path on 32-bit keys (it stops as soon as the bin of that key is known)
    uint32_t prefix = 0;
    const bool take_all = n_sel >= n_stored;
    if (!take_all) {
      int need = n_sel;
      const uint32_t diff = a_and ^ a_or;
      if (diff == 0) {
        prefix = a_and;
      } else {
        // digits of up to 8 bits from the highest differing bit downwards (NOT byte aligned: the
        // top byte of a positive float is 7 exponent bits - a handful of values, i.e. a
        // same-address atomic storm in the histogram; starting at the first bit that differs
        // spreads the first digit over exponent AND mantissa bits)
        int top = 32 - __clz(static_cast<int>(diff));           // bits [top - 1 .. 0] may differ
        const int low_bit = __ffs(static_cast<int>(a_or)) - 1;  // below it every key is zero
        prefix = top >= 32 ? 0u : a_and & (~0u << top);
        while (top > 0) {
          const int lo = max(top - 8, 0);
          const uint32_t dmask = (1u << (top - lo)) - 1u;
          const uint32_t hi_mask = top >= 32 ? 0u : (~0u << top);
#pragma unroll
          for (int k = 0; k < PER; k++) {
            const bool in = ((have >> k) & 1u) && (k32[k] & hi_mask) == prefix;
            const uint32_t digit = (k32[k] >> lo) & dmask;
            const unsigned long long todo = __ballot(in);
            if (todo) {
              const int leader = __ffsll(static_cast<long long>(todo)) - 1;
              const uint32_t d = __builtin_amdgcn_readlane(digit, leader);
              const unsigned long long same = __ballot(in && digit == d);
              if (same == todo) {
                if (lane == leader) atomicAdd(&hist[d], static_cast<uint32_t>(__popcll(same)));
              } else if (in) {
                atomicAdd(&hist[digit], 1u);
              }
            }
          }
          __syncthreads();
          if (wv == 0) {
            // lane l scans the bins 255 - 4 l .. 252 - 4 l (descending digits) and clears them
            int bn[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
              bn[j] = static_cast<int>(hist[255 - 4 * lane - j]);
              hist[255 - 4 * lane - j] = 0u;
              sum += bn[j];
            }
            int incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
              const int t = __shfl_up(incl, o, 64);
              if (lane >= o) incl += t;
            }
            int run = incl - sum;  // keys in higher bins
#pragma unroll
            for (int j = 0; j < 4; j++) {
              if (run < need && run + bn[j] >= need) {
                sh_prefix = prefix | (static_cast<uint32_t>(255 - 4 * lane - j) << lo);
                sh_need = (run + bn[j] == need) ? -1 : need - run;
                sh_total = n_sel - need + run + bn[j];  // keys >= the lower bound of this bin
              }
              run += bn[j];
            }
          }
          __syncthreads();
          prefix = static_cast<uint32_t>(sh_prefix);
          need = sh_need;
          const int above = sh_total;
          top = lo;
          // every key of the chosen bin is >= prefix, which is all a lower bound needs: stop when
          // the bin is wanted as a whole, no lower digit differs, or few enough keys lie at or
          // above it (they all become candidates)
          if (need < 0 || top <= low_bit || above <= n_sel + FAST_SLACK) break;
        }
      }
    }
    // candidates: approximation >= prefix (1 - 2^-17), one more unit in the last place for the
    // rounding of this very product
    uint32_t thr = 0u;
    if (!take_all) {
      const float lf = __uint_as_float(prefix) * (1.0f - 0x1p-17f);
      thr = __float_as_uint(lf);
      thr = thr > 0u ? thr - 1u : 0u;
    }
    uint32_t candmask = 0;
#pragma unroll
    for (int k = 0; k < PER; k++)
      if (((have >> k) & 1u) && k32[k] >= thr) candmask |= 1u << k;
    PHASE_MARK(4);
    {
      // (upper half of the accumulator block, behind the 256 bytes of sinks: idle on the count path)
      uint64_t *candK = reinterpret_cast<uint64_t *>(smem + TILE * 4 + 1024);
      uint32_t *candC = reinterpret_cast<uint32_t *>(candK + FAST_CAP);
      uint32_t *candV = candC + FAST_CAP;  // the count
      // owners hand (column, count) to the list; thread t then takes candidate t: ONE gathered
      // norm load and one fp64 epilogue per candidate, all of them side by side (under the
      // owners' branches every load would expose its own latency)
      {
        // one returning atomic per wave: the wave's candidates take consecutive slots
        int mine = __popc(candmask), total = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(total, o, 64);
          if (lane >= o) total += t;
        }
        int base = 0;
        if (lane == 63) base = total > 0 ? atomicAdd(&sh_count, total) : 0;
        base = __shfl(base, 63, 64) + total - mine;
#pragma unroll
        for (int k = 0; k < PER; k++) {
          if ((candmask >> k) & 1u) {
            if (base < FAST_CAP) {
              candC[base] = static_cast<uint32_t>(cbase + 64 * k);
              candV[base] = cnt[cbase + 64 * k];
            }
            base++;
          }
        }
      }
      __syncthreads();
      const int n_cand = sh_count;  // (the compaction counted them)
#ifdef IRS_KNN_PHASES
      if (tid == 0) {
        atomicAdd(&knn_fast_stat[0], 1ull);
        if (n_cand > FAST_CAP) atomicAdd(&knn_fast_stat[1], 1ull);
        atomicAdd(&knn_fast_stat[2], static_cast<unsigned long long>(n_cand));
        if (n_cand <= 128) atomicAdd(&knn_fast_stat[3], 1ull);
        if (n_cand <= 256) atomicAdd(&knn_fast_stat[4], 1ull);
        if (n_cand <= 512) atomicAdd(&knn_fast_stat[5], 1ull);
        if (n_cand <= 1024) atomicAdd(&knn_fast_stat[6], 1ull);
      }
#endif
      if (n_cand <= FAST_CAP) {  // (block-uniform)
      for (int t = tid; t < n_cand; t += THREADS) {
        const double sv = epilogue(p, static_cast<double>(candV[t]), p.norms[c0 + candC[t]], tstat);
        candK[t] = order_key(sv);
      }
      __syncthreads();
      // rank = candidates that go before (value desc, column asc): eight threads per candidate,
      // each against every eighth entry of the list.  The winners leave in RANK order (the row
      // merge sorts the tiles' lists anyway; calls whose merge relies on column-sorted lists,
      // top_k > TOPK_CAP, do not take this path).
      constexpr int TPC = 8, CPR = THREADS / TPC;  // candidates per round
      int tid_ = tid;
      asm volatile("" : "+v"(tid_));  // (nothing derived from it is worth a register across the accumulation)
      const int sub = tid_ & (TPC - 1);
      for (int t0 = 0; t0 < n_cand; t0 += CPR) {
        const int t = t0 + tid_ / TPC;
        const bool live = t < n_cand;
        const uint64_t mk = candK[live ? t : 0];
        const uint32_t mc = candC[live ? t : 0];
        int before = 0;
        for (int q = sub; q < n_cand; q += TPC) {
          const uint64_t ok = candK[q];
          const uint32_t oc = candC[q];
          before += (ok > mk || (ok == mk && oc < mc)) ? 1 : 0;
        }
        before += __shfl_xor(before, 1, 64);
        before += __shfl_xor(before, 2, 64);
        before += __shfl_xor(before, 4, 64);
        if (live && sub == 0 && before < n_sel) {
          cidx[before] = c0 + static_cast<int>(mc);
          cval[before] = key_to_double(mk);  // (order_key is invertible on the finite values)
        }
      }
      if (tid == 0) p.cand_cnt[bid] = n_sel;
      fast_done = true;
      }
      PHASE_MARK(5);
    }
  }
  if constexpr (FAST) {
    // (rare: thousands of near-ties at the threshold) the pair goes to the exact kernel's list
    if (!fast_done && tid == 0) p.redo_list[atomicAdd(p.redo_count, 1)] = bid;
  } else {
  uint64_t key[PER];
  have = 0;
  uint32_t cv[ACC32 ? PER : 1];
  if (ACC32) {
    // count i sits in the bytes of acc[i / 2]: every count is read before any sum is written
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int i = cbase + 64 * k;
      cv[k] = cnt[min(i, TILE - 1)];
      if (i < width && cv[k] != 0u) have |= 1u << k;
    }
    __syncthreads();
  }
#pragma unroll
  for (int h = 0; h < PER; h += 8) {  // eight columns at a time (register budget)
    double nrm[8], raw[8];
#pragma unroll
    for (int k = 0; k < 8; k++)
      nrm[k] = h == 0 ? nrm0[k] : p.norms[c0 + min(cbase + 64 * (h + k), width - 1)];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int i = cbase + 64 * (h + k);
      if (ACC32) {
        raw[k] = static_cast<double>(cv[ACC32 ? h + k : 0]);
      } else {
        // fixed-point sum -> double (one rounding).  Sentinel: the accumulator started at the
        // bit pattern of -0.0 = INT64_MIN, the sum is the difference.
        uint64_t fx = static_cast<uint64_t>(__double_as_longlong(acc[min(i, TILE - 1)]));
        double low = 0.0;
        if (wide) {  // (block-uniform) the accumulator holds the second limb, the stash the first
          low = static_cast<double>(static_cast<long long>(fx)) * 0x1p-40;
          fx = stash[min(i, TILE - 1)];
        }
        raw[k] = (static_cast<double>(static_cast<long long>(fx ^ (SENTINEL ? NEG_ZERO_BITS : 0ull))) + low) *
                 fx_inv;
        const bool st = SENTINEL ? fx != NEG_ZERO_BITS
                                 : ((bits[min(i, TILE - 1) >> 5] >> (i & 31)) & 1u) != 0u;
        if (i < width && st) have |= 1u << (h + k);
      }
    }
    if (!FAST && p.col_scale != nullptr) {  // (block-uniform)
#pragma unroll
      for (int k = 0; k < 8; k++)
        raw[k] = __dmul_rn(raw[k], p.col_scale[c0 + min(cbase + 64 * (h + k), width - 1)]);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const double sv = epilogue(p, raw[k], nrm[k], tstat);
      key[h + k] = order_key(sv);
      if ((have >> (h + k)) & 1u) acc[cbase + 64 * (h + k)] = sv;
    }
  }
  // stored entries of the tile, and the bits in which their keys differ (the radix select
  // starts at the first digit that is not common to all of them)
  uint64_t k_and = ~0ull, k_or = 0ull;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    if ((have >> k) & 1u) {
      k_and &= key[k];
      k_or |= key[k];
    }
  }
  int local = __popc(have);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    local += __shfl_xor(local, o, 64);
    k_and &= __shfl_xor(k_and, o, 64);
    k_or |= __shfl_xor(k_or, o, 64);
  }
  uint64_t *red = reinterpret_cast<uint64_t *>(hist);  // 16 x (and, or) + counts behind
  if (lane == 0) {
    red[2 * wv] = k_and;
    red[2 * wv + 1] = k_or;
    wave_cnt[wv] = local;
  }
  __syncthreads();
  int n_stored = 0;
  k_and = ~0ull;
  k_or = 0ull;
#pragma unroll
  for (int w = 0; w < NW; w++) {
    n_stored += wave_cnt[w];
    k_and &= red[2 * w];
    k_or |= red[2 * w + 1];
  }
  __syncthreads();  // red / wave_cnt are reused below
  const int n_sel = min(p.top_k, n_stored);
  if (tid == 0) p.cand_cnt[bid] = n_sel;
  if (n_sel == 0) continue;
  PHASE_MARK(3);

  // ---- 3. radix select of the n_sel-th largest key (value desc, column asc on ties):
  //      `prefix` becomes that key and `need` the number of its ties that are taken.
  uint64_t prefix = 0;
  int need = n_sel;
  const bool take_all = n_sel >= n_stored;
  if (!take_all) {
    const uint64_t diff = k_and ^ k_or;
    if (diff == 0) {
      prefix = k_and;  // all stored keys are equal: everything ties
    } else {
      int shift = ((63 - __clzll(static_cast<long long>(diff))) >> 3) << 3;
      const int low_shift = ((__ffsll(static_cast<long long>(k_or)) - 1) >> 3) << 3;
      prefix = shift + 8 >= 64 ? 0ull : k_and & (~0ull << (shift + 8));
      for (; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const uint64_t hi_mask = (shift + 8 >= 64) ? 0ull : (~0ull << (shift + 8));
#pragma unroll
        for (int k = 0; k < PER; k++) {
          const bool in = ((have >> k) & 1u) && (key[k] & hi_mask) == prefix;
          const uint32_t digit = static_cast<uint32_t>(key[k] >> shift) & 0xffu;
          // similarities share their leading bytes: when every candidate lane of the wave
          // has the same digit, one lane adds the count (no same-address atomic storm);
          // otherwise the digits are spread and per-lane atomics are cheap
          const unsigned long long todo = __ballot(in);
          if (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const uint32_t d = __builtin_amdgcn_readlane(digit, leader);
            const unsigned long long same = __ballot(in && digit == d);
            if (same == todo) {
              if (lane == leader) atomicAdd(&hist[d], static_cast<uint32_t>(__popcll(same)));
            } else if (in) {
              atomicAdd(&hist[digit], 1u);
            }
          }
        }
        __syncthreads();
        // the digit d with  #(digits > d) < need <= #(digits >= d): scan the bins in
        // descending digit order with the first four waves
        int bin = 0, incl = 0;
        if (tid < 256) {
          bin = static_cast<int>(hist[255 - tid]);
          incl = bin;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
          }
          if (lane == 63) wave_cnt[wv] = incl;
        }
        __syncthreads();
        if (tid < 256) {
          for (int w = 0; w < wv; w++) incl += wave_cnt[w];
          const int excl = incl - bin;
          if (excl < need && incl >= need) {
            sh_prefix = prefix | (static_cast<uint64_t>(255 - tid) << shift);
            // the whole bin is wanted: every key >= the bin's lowest possible key is taken
            // and no further digit has to be resolved (-1 tells the loop to stop)
            sh_need = (incl == need) ? -1 : need - excl;
            sh_total = bin;
          }
        }
        __syncthreads();
        prefix = sh_prefix;
        need = sh_need;
        const int in_bin = sh_total;
        __syncthreads();
        // below the lowest set bit of any key every digit is zero: the prefix is the key
        if (need < 0 || shift == 0 || shift <= low_shift) break;
        if (in_bin <= 64) {
          // few candidates left: one wave ranks them instead of more digit passes
          const uint64_t lo_mask = ~0ull << shift;
          if (tid == 0) sh_count = 0;
          __syncthreads();
#pragma unroll
          for (int k = 0; k < PER; k++)
            if (((have >> k) & 1u) && (key[k] & lo_mask) == prefix)
              red[atomicAdd(&sh_count, 1)] = key[k];
          __syncthreads();
          if (wv == 0) {
            const uint64_t mine = lane < in_bin ? red[lane] : 0ull;
            int gt = 0, ge = 0;
            for (int q = 0; q < in_bin; q++) {
              const uint64_t other = red[q];
              gt += other > mine;
              ge += other >= mine;
            }
            if (lane < in_bin && gt < need && need <= ge) {  // equal keys write equal values
              sh_prefix = mine;
              sh_need = need - gt;
            }
          }
          __syncthreads();
          prefix = sh_prefix;
          need = sh_need;
          __syncthreads();
          break;
        }
      }
      if (need < 0) {
        if (prefix == 0) {  // lowest possible key: nothing is excluded, everything else ties
          need = n_sel;
        } else {
          prefix -= 1;  // k > prefix - 1  <=>  k >= prefix
          need = 0;
        }
      }
    }
  } else {
    need = 0;  // everything is taken
  }
  PHASE_MARK(4);
  // Ordered compaction: (wave, slot k, lane) order is column order, so the winners are
  // written in ascending column order without atomics and the tile's list is column-sorted
  // (the row merge for top_k > TOPK_CAP relies on it).  Pass A counts this wave's ties with
  // the threshold key; pass B ranks the ties in column order (the `need` lowest columns win,
  // knn.hpp:119-136) and counts this wave's winners; pass C writes them.
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  int my_ties = 0;
  if (!take_all && need > 0) {
#pragma unroll
    for (int k = 0; k < PER; k++)
      my_ties += __popcll(__ballot(((have >> k) & 1u) && key[k] == prefix));
  }
  __syncthreads();  // wave_cnt (stored entries per wave) has been read by everyone
  if (lane == 0) wave_cnt[wv] = my_ties;
  __syncthreads();
  int ties_before = 0;
  for (int w = 0; w < wv; w++) ties_before += wave_cnt[w];
  uint32_t winmask = 0;
  int my_wins = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const bool st = (have >> k) & 1u;
    const bool tie = st && !take_all && key[k] == prefix;
    const unsigned long long bal = __ballot(tie);
    const int rank = ties_before + __popcll(bal & lt_mask);
    const bool win = st && (take_all || key[k] > prefix || (tie && rank < need));
    ties_before += __popcll(bal);
    if (win) winmask |= 1u << k;
    my_wins += __popcll(__ballot(win));
  }
  __syncthreads();  // the tie counts have been read
  if (lane == 0) wave_cnt[wv] = my_wins;
  __syncthreads();
  int pos0 = 0;
  for (int w = 0; w < wv; w++) pos0 += wave_cnt[w];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const bool win = (winmask >> k) & 1u;
    const unsigned long long bal = __ballot(win);
    if (win) {
      const int pos = pos0 + __popcll(bal & lt_mask);
      cidx[pos] = c0 + cbase + 64 * k;
      cval[pos] = acc[cbase + 64 * k];
    }
    pos0 += __popcll(bal);
  }
  PHASE_MARK(5);
  }  // exact path
  }  // persistent loop
}

// One 256-thread workgroup per target row: union of the tile winners, keep the
// top_k by (value desc, column asc), emit them sorted by column (knn.hpp:119-136).
// The tiles are merged in rounds: as many tiles as fit next to the best-so-far are appended,
// the buffer is sorted and cut back to top_k (any number of tiles, top_k <= MERGE_CAP / 2).
__global__ __launch_bounds__(256) void knn_merge_kernel(Params p) {
  // merge_cap entries (a power of two sized to the request, at most MERGE_CAP): 20 B each
  extern __shared__ __attribute__((aligned(16))) unsigned char merge_smem[];
  uint64_t *key = reinterpret_cast<uint64_t *>(merge_smem);
  double *val = reinterpret_cast<double *>(key + p.merge_cap);
  int32_t *idx = reinterpret_cast<int32_t *>(val + p.merge_cap);
  const int tid = threadIdx.x;
  const int slot = blockIdx.x;
  auto swap_el = [&](int a, int b) {
    const uint64_t tk = key[a]; key[a] = key[b]; key[b] = tk;
    const double tv = val[a]; val[a] = val[b]; val[b] = tv;
    const int32_t ti = idx[a]; idx[a] = idx[b]; idx[b] = ti;
  };
  int n = 0;  // entries currently in the buffer (the best so far after a round)
  int t = 0;
  do {
    // append tiles while they fit (cand_cnt <= top_k <= MERGE_CAP / 2: at least one fits)
    while (t < p.n_tiles) {
      const int b = slot * p.n_tiles + t;
      const int c = p.cand_cnt[b];
      if (n + c > p.merge_cap) break;
      for (int i = tid; i < c; i += 256) {
        const double v = p.cand_val[static_cast<size_t>(b) * p.tile_k + i];
        val[n + i] = v;
        key[n + i] = order_key(v);
        idx[n + i] = p.cand_idx[static_cast<size_t>(b) * p.tile_k + i];
      }
      n += c;
      t++;
    }
    int n_pow = 1;
    while (n_pow < n) n_pow <<= 1;
    for (int i = n + tid; i < n_pow; i += 256) {
      key[i] = 0ull;
      val[i] = 0.0;
      idx[i] = 0x7fffffff;
    }
    __syncthreads();
    // (value desc, column asc); padding (column = INT_MAX) sorts last among equal keys
    for (int k2 = 2; k2 <= n_pow; k2 <<= 1)
      for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
        for (int i = tid; i < n_pow; i += 256) {
          const int l = i ^ j2;
          if (l > i) {
            const bool up = (i & k2) == 0;
            const bool l_first = (key[l] != key[i]) ? key[l] > key[i] : idx[l] < idx[i];
            const bool i_first = (key[l] != key[i]) ? key[i] > key[l] : idx[i] < idx[l];
            if (up ? l_first : i_first) swap_el(i, l);
          }
        }
        __syncthreads();
      }
    n = min(n, p.top_k);  // real entries with key 0 (NaN) outrank padding by column
  } while (t < p.n_tiles);
  const int keep = n;
  int k_pow = 1;
  while (k_pow < keep) k_pow <<= 1;
  for (int i = keep + tid; i < k_pow; i += 256) idx[i] = 0x7fffffff;
  __syncthreads();
  // the kept entries by column
  for (int k2 = 2; k2 <= k_pow; k2 <<= 1)
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (int i = tid; i < k_pow; i += 256) {
        const int l = i ^ j2;
        if (l > i) {
          const bool up = (i & k2) == 0;
          if (up ? idx[l] < idx[i] : idx[i] < idx[l]) swap_el(i, l);
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < keep; i += 256) {
    p.out_idx[static_cast<size_t>(slot) * p.top_k + i] = idx[i];
    p.out_val[static_cast<size_t>(slot) * p.top_k + i] = val[i];
  }
  if (tid == 0) p.out_cnt[slot] = keep;
}

// Row merge for top_k > TOPK_CAP (e.g. P3alpha / RP3beta with their default top_k = None, or a
// user-kNN over every user): the tiles' winner lists are column-sorted and the tiles are in
// column order, so the row only needs the top_k-th best key as a threshold - an MSB-first
// 8-bit radix select over the keys in global memory - and one ordered compaction: everything
// above the threshold plus the `need` lowest-column ties (knn.hpp:119-136).  The output comes
// out sorted by column.  One 256-thread workgroup per target row.
__global__ __launch_bounds__(256) void knn_merge_big_kernel(Params p) {
  __shared__ int32_t hist[256];
  __shared__ int32_t wsum[4];
  __shared__ uint64_t sh_prefix;
  __shared__ int32_t sh_need;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int slot = blockIdx.x;
  const int32_t *cnt = p.cand_cnt + static_cast<size_t>(slot) * p.n_tiles;
  int n_total = 0;
  for (int t = 0; t < p.n_tiles; t++) n_total += cnt[t];
  int32_t *oidx = p.out_idx + static_cast<size_t>(slot) * p.top_k;
  double *oval = p.out_val + static_cast<size_t>(slot) * p.top_k;
  const size_t cbase = static_cast<size_t>(slot) * p.n_tiles * p.tile_k;
  uint64_t thr = 0;
  int need = 0;
  const bool all = n_total <= p.top_k;
  if (!all) {
    uint64_t prefix = 0;
    int remaining = p.top_k;  // rank of the wanted key among those matching the prefix so far
    for (int shift = 56; shift >= 0; shift -= 8) {
      hist[tid] = 0;
      __syncthreads();
      const uint64_t hi_mask = shift == 56 ? 0ull : (~0ull << (shift + 8));
      for (int t = 0; t < p.n_tiles; t++) {
        const double *v = p.cand_val + cbase + static_cast<size_t>(t) * p.tile_k;
        for (int i = tid; i < cnt[t]; i += 256) {
          const uint64_t k = order_key(v[i]);
          if ((k & hi_mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
        }
      }
      __syncthreads();
      if (tid == 0) {
        int d = 255, above = 0;
        while (above + hist[d] < remaining) { above += hist[d]; d--; }
        sh_prefix = prefix | (static_cast<uint64_t>(d) << shift);
        sh_need = remaining - above;
      }
      __syncthreads();
      prefix = sh_prefix;
      remaining = sh_need;
      __syncthreads();
    }
    thr = prefix;
    need = remaining;  // ties with the threshold key that are taken (lowest columns)
  }
  // ordered compaction, 256 entries per round in list order
  int out_n = 0, ties_seen = 0;
  for (int t = 0; t < p.n_tiles; t++) {
    const double *v = p.cand_val + cbase + static_cast<size_t>(t) * p.tile_k;
    const int32_t *ix = p.cand_idx + cbase + static_cast<size_t>(t) * p.tile_k;
    for (int i0 = 0; i0 < cnt[t]; i0 += 256) {
      const int i = i0 + tid;
      const bool in = i < cnt[t];
      const double val = in ? v[i] : 0.0;
      const int32_t col = in ? ix[i] : 0;
      const uint64_t k = order_key(val);
      const bool tie = in && !all && k == thr;
      // rank of this tie among the row's ties, in column order
      const unsigned long long tb = __ballot(tie);
      if (lane == 0) wsum[wv] = __popcll(tb);
      __syncthreads();
      int tbefore = ties_seen;
      for (int w = 0; w < wv; w++) tbefore += wsum[w];
      const int tie_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
      __syncthreads();
      const int trank = tbefore + __popcll(tb & ((1ull << lane) - 1ull));
      const bool win = in && (all || k > thr || (tie && trank < need));
      const unsigned long long wb = __ballot(win);
      if (lane == 0) wsum[wv] = __popcll(wb);
      __syncthreads();
      int wbefore = out_n;
      for (int w = 0; w < wv; w++) wbefore += wsum[w];
      const int win_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
      __syncthreads();
      if (win) {
        const int pos = wbefore + __popcll(wb & ((1ull << lane) - 1ull));
        oidx[pos] = col;
        oval[pos] = val;
      }
      out_n += win_total;
      ties_seen += tie_total;
    }
  }
  if (tid == 0) p.out_cnt[slot] = out_n;
}

// The merged rows (work-ordered slots, top_k entries apart) -> one contiguous CSR in target-row
// order on the device, so that the result crosses PCIe once, straight into the caller's arrays.
__global__ __launch_bounds__(256) void knn_compact_kernel(const int32_t *__restrict__ out_idx,
                                                          const double *__restrict__ out_val,
                                                          const int32_t *__restrict__ slot_of,
                                                          const int64_t *__restrict__ res_ptr,
                                                          int64_t n_rows, int32_t top_k,
                                                          int32_t *__restrict__ dst_idx,
                                                          double *__restrict__ dst_val) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + wave_index_in_block();
  if (row >= n_rows) return;
  const int lane = threadIdx.x & 63;
  const int64_t b = res_ptr[row], e = res_ptr[row + 1];
  const size_t src = static_cast<size_t>(slot_of[row]) * top_k;
  for (int64_t i = lane; i < e - b; i += 64) {
    dst_idx[b + i] = out_idx[src + i];
    dst_val[b + i] = out_val[src + i];
  }
}

// irs_knn_create on the device (all-ones matrices): the slice pointers and the packed 16-bit offsets
// of X_arg^T from its device-resident transpose (transpose_csr_device, device_sort.hip).
// xt_ptr[u] = first entry of feature row u; tptr[u][t] = first entry of the row with column >= t TILE.
__global__ __launch_bounds__(256) void xt_slices_kernel(const uint32_t *__restrict__ xt_ptr,
                                                        const int32_t *__restrict__ t_idx, int64_t n_rows,
                                                        int32_t n_tiles, uint32_t *__restrict__ tptr) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n_rows * (n_tiles + 1)) return;
  const int64_t u = i / (n_tiles + 1);
  const int32_t t = static_cast<int32_t>(i % (n_tiles + 1));
  const uint32_t b = xt_ptr[u], e = xt_ptr[u + 1];
  if (t == n_tiles) {
    tptr[i] = e;
    return;
  }
  const int32_t key = t * TILE;
  uint32_t lo = b, hi = e;  // the first position whose column is >= key
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (t_idx[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  tptr[i] = lo;
}

// per feature row of X_arg^T: largest and smallest non-zero |x| (0 when the row has none): the bounds
// the target pass builds the fixed-point scales from
// ... and the row's first value + whether any row holds two different ones (bit patterns compared)
__global__ __launch_bounds__(256) void xt_row_range_kernel(const uint32_t *__restrict__ xt_ptr,
                                                           const double *__restrict__ xt_val, int64_t n_rows,
                                                           double *__restrict__ row_max, double *__restrict__ row_min,
                                                           double *__restrict__ row_val, int32_t *__restrict__ not_const) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (u >= n_rows) return;
  double mx = 0.0, mn = __longlong_as_double(0x7ff0000000000000ll);
  const uint32_t b = xt_ptr[u], e = xt_ptr[u + 1];
  const double first = b < e ? xt_val[b] : 0.0;
  bool same = true;
  for (uint32_t q = b; q < e; q++) {
    const double v = xt_val[q], a = fabs(v);
    mx = fmax(mx, a);
    if (a > 0.0) mn = fmin(mn, a);
    same &= __double_as_longlong(v) == __double_as_longlong(first);
  }
  row_max[u] = mx;
  row_min[u] = isfinite(mn) ? mn : 0.0;
  row_val[u] = first;
  if (!same) atomicOr(not_const, 1);
}

// two tile-relative LDS byte offsets (column x 4, 16 bits each) per dword; zeros behind the last entry
__global__ __launch_bounds__(256) void xt_pack16_kernel(const int32_t *__restrict__ t_idx, int64_t nnz,
                                                        int64_t n_words, uint32_t *__restrict__ idx_p) {
  const int64_t w = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (w >= n_words) return;
  const int64_t q = 2 * w;
  const uint32_t lo = q < nnz ? static_cast<uint32_t>((t_idx[q] % TILE) * 4) : 0u;
  const uint32_t hi = q + 1 < nnz ? static_cast<uint32_t>((t_idx[q + 1] % TILE) * 4) : 0u;
  idx_p[w] = lo | (hi << 16);
}


// ---------------------------------------------------------------------------------------------------------
// Feature weighting on the device (util.hpp:159-209; host tables: knn_host_prep.hpp weight_tables).
// One wave per stored row of the matrix (its documents): w[q] = v * idf[col] (tf-idf, :206) or
// idf[col] * (v * (k1 + 1)) / (v + reg[row]) (BM25, :183-184) - each operation rounded once, in the
// reference's order (__dmul_rn / __dadd_rn / __ddiv_rn: no contraction), so the values are the host
// loop's bit for bit.  `vals` null: every stored value is 1.  flags (or-ed): 1 some weight != 1,
// 2 some |weight| outside (1e-150, 1e150) (or zero), 4 some weight <= 0 - what the host pass of
// irs_knn_create derives from the caller's values when it does not weight.
template <bool BM25>
__global__ __launch_bounds__(256) void knn_weight_kernel(const int32_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices,
                                                         const double *__restrict__ vals,
                                                         const double *__restrict__ idf,
                                                         const double *__restrict__ reg, double k1p1,
                                                         int64_t n_rows, double *__restrict__ out,
                                                         int32_t *__restrict__ flags) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 4 + wave_index_in_block();
  if (r >= n_rows) return;
  const int lane = threadIdx.x & 63;
  const int32_t b = indptr[r], e = indptr[r + 1];
  const double rg = BM25 ? reg[r] : 0.0;
  int32_t f = 0;
  for (int32_t q = b + lane; q < e; q += 64) {
    const double v = vals ? vals[q] : 1.0;
    const double w = idf[indices[q]];
    double o;
    if (BM25) o = __ddiv_rn(__dmul_rn(w, __dmul_rn(v, k1p1)), __dadd_rn(v, rg));
    else o = __dmul_rn(v, w);
    out[q] = o;
    const double a = fabs(o);
    f |= (o != 1.0 ? 1 : 0) | (!(a > 1e-150 && a < 1e150) ? 2 : 0) | (!(o > 0.0) ? 4 : 0);
  }
  if (flags) {
    f = (__ballot(f & 1) ? 1 : 0) | (__ballot(f & 2) ? 2 : 0) | (__ballot(f & 4) ? 4 : 0);  // wave-wide or
    if (lane == 0 && f && (__hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & f) != f)
      atomicOr(flags, f);
  }
}

// ss[r] = the squares of row r's values added one by one in storage order, product and sum rounded
// separately (the `ss += x * x` loop of the norms, similarities.hpp:20-28 / :61-72, compiled without
// contraction).  One wave per row: the lanes load and square a strip of 64 values, then every lane runs
// the same 64-step chain over the strip's squares (lane broadcasts) - the order of the sum is the
// sequential one, only the loads are parallel.  Entries past the row's end add +0.0, which changes no
// partial sum (they are >= +0.0).
__global__ __launch_bounds__(256) void knn_row_sumsq_kernel(const uint32_t *__restrict__ ptr,
                                                            const double *__restrict__ vals, int64_t n_rows,
                                                            double *__restrict__ ss) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 4 + wave_index_in_block();
  if (r >= n_rows) return;
  const int lane = threadIdx.x & 63;
  const uint32_t b = ptr[r], e = ptr[r + 1];
  double sum = 0.0;
  for (uint32_t q0 = b; q0 < e; q0 += 64) {
    const uint32_t q = q0 + lane;
    const double v = q < e ? vals[q] : 0.0;
    const double sq = __dmul_rn(v, v);
    const uint32_t n = min(64u, e - q0);
    if (n == 64) {
#pragma unroll
      for (int j = 0; j < 64; j++) sum = __dadd_rn(sum, __shfl(sq, j));
    } else {
      for (uint32_t j = 0; j < n; j++) sum = __dadd_rn(sum, __shfl(sq, static_cast<int>(j)));
    }
  }
  if (lane == 0) ss[r] = sum;
}

// the padded value stream of X_arg^T from values that are already on the device (zeros behind the last entry)
__global__ __launch_bounds__(256) void knn_pad_copy_kernel(const double *__restrict__ src, int64_t nnz,
                                                           int64_t padded, double *__restrict__ dst) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (q < padded) dst[q] = q < nnz ? src[q] : 0.0;
}


// remove_diagonal (util.hpp:211-226) on the TRANSPOSED result: column c's entries hold ascending row numbers;
// the one whose row is c - row0 (if stored) is set to 0.0 and kept.  One thread per column.
__global__ __launch_bounds__(256) void knn_zero_diagonal_csc_kernel(const int32_t *__restrict__ col_ptr,
                                                                    const int32_t *__restrict__ row_idx,
                                                                    int64_t n_cols, int64_t row0,
                                                                    double *__restrict__ val) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (c >= n_cols) return;
  const int64_t want = c - row0;
  int32_t lo = col_ptr[c], hi = col_ptr[c + 1];
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (row_idx[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  if (lo < col_ptr[c + 1] && row_idx[lo] == want) val[lo] = 0.0;
}

}  // namespace knn
}  // namespace irs
