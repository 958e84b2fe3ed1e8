// The host decisions of the iALS path (irspack_amd/csrc/ials_host_plan.hpp: the task plan of a side, the route of
// a half-step, the iALS++ variant, the eigenbasis cuts) on their own: no HIP, built with
// -fsanitize=address,undefined and with -fsanitize=thread by tests/test_host_sanitizers.py.  Expected values are
// written out by hand, restated in plain loops, or - the route - the chains of conditions launch_solve,
// launch_ialspp and eig_begin consisted of before the route was computed in one place, written out literally.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "../../irspack_amd/csrc/host_util.hpp"
#include "../../irspack_amd/csrc/ials_host_plan.hpp"

using namespace irs;
using namespace irs::ials;

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

#if defined(__SANITIZE_THREAD__)
constexpr bool kThreadSanitizer = true;
#elif defined(__has_feature)
#if __has_feature(thread_sanitizer)
constexpr bool kThreadSanitizer = true;
#else
constexpr bool kThreadSanitizer = false;
#endif
#else
constexpr bool kThreadSanitizer = false;
#endif

static irs_ials_model_config config(uint64_t K) {
  irs_ials_model_config c{};
  c.K = K;
  c.alpha0 = 0.1f;
  c.reg = 0.05f;
  c.nu = 0.5f;
  return c;
}
static std::vector<int32_t> row_pointer(const std::vector<int32_t> &lengths) {
  std::vector<int32_t> ip(lengths.size() + 1, 0);  // exactly rows + 1 values: ASan sees a read past the end
  for (size_t r = 0; r < lengths.size(); r++) ip[r + 1] = ip[r] + lengths[r];
  return ip;
}
static bool same(const Task &a, const Task &b) { return a.row == b.row && a.begin == b.begin && a.end == b.end && a.slot == b.slot; }
static bool same(const SplitRow &a, const SplitRow &b) {
  return a.row == b.row && a.first_slot == b.first_slot && a.n_slots == b.n_slots && a.nnz == b.nnz && a.slot_stride == b.slot_stride;
}
static bool same(const FoldGroup &a, const FoldGroup &b) { return a.first_slot == b.first_slot && a.count == b.count; }
template <class T> static bool same_list(const std::vector<T> &got, const std::vector<T> &want) {
  if (got.size() != want.size()) return false;
  for (size_t i = 0; i < got.size(); i++)
    if (!same(got[i], want[i])) return false;
  return true;
}

// ---------------------------------------------------------------- the task plan: properties of every case
static TaskPlan checked_plan(const std::vector<int32_t> &lengths, int64_t rb, int64_t re, uint64_t K, int chunk,
                             int32_t chunk_long, int64_t n_cols = 1000) {
  const std::vector<int32_t> ip = row_pointer(lengths);
  const int64_t n_rows = static_cast<int64_t>(lengths.size());
  const irs_ials_model_config cfg = config(K);
  const TaskPlan pl = plan_tasks(ip.data(), n_rows, n_cols, rb, re, cfg, chunk, chunk_long);
  auto len = [](const Task &a) { return a.end - a.begin; };
  EXPECT(pl.n_tasks == static_cast<int32_t>(pl.tasks.size()) && pl.n_split == static_cast<int32_t>(pl.split.size()) &&
         pl.n_fold == static_cast<int32_t>(pl.fold.size()));
  // longest first, and stable: equal lengths in (row, chunk) order
  for (size_t i = 1; i < pl.tasks.size(); i++) {
    const Task &a = pl.tasks[i - 1], &b = pl.tasks[i];
    EXPECT(len(a) >= len(b));
    if (len(a) == len(b)) EXPECT(a.row < b.row || (a.row == b.row && a.begin < b.begin));
  }
  // per row: its tasks tile [ip[r], ip[r + 1]) exactly, cuts at multiples of 4 from the row's start, a row up to
  // `chunk` entries is one task without a slot, the slots of a longer row are consecutive in chunk order
  std::vector<int> seen_slot(static_cast<size_t>(pl.n_slots), 0);
  size_t n_split_rows = 0;
  for (int64_t r = rb; r < re; r++) {
    std::vector<Task> mine;
    for (const Task &a : pl.tasks)
      if (a.row == r) mine.push_back(a);
    std::sort(mine.begin(), mine.end(), [](const Task &a, const Task &b) { return a.begin < b.begin; });
    EXPECT(!mine.empty() && mine.front().begin == ip[r] && mine.back().end == ip[r + 1]);
    const bool is_split = lengths[r] > chunk;
    n_split_rows += is_split;
    EXPECT(is_split || (mine.size() == 1 && mine[0].slot == -1));
    EXPECT(static_cast<int>(mine.size()) <= MAX_CHUNKS);
    for (size_t i = 0; i < mine.size(); i++) {
      if (i) EXPECT(mine[i].begin == mine[i - 1].end && (mine[i].begin - ip[r]) % 4 == 0 && len(mine[i - 1]) >= len(mine[i]));
      EXPECT(len(mine[i]) > 0 || lengths[r] == 0);
      if (is_split) {
        EXPECT(mine[i].slot == mine[0].slot + static_cast<int32_t>(i) && mine[i].slot >= 0 && mine[i].slot < pl.n_slots);
        seen_slot[mine[i].slot]++;
      }
    }
    if (!is_split) continue;
    // its SplitRow, and the fold groups that tile its slots when there are more than FOLD_MIN
    const SplitRow *sr = nullptr;
    for (const SplitRow &s : pl.split)
      if (s.row == r) {
        EXPECT(sr == nullptr);
        sr = &s;
      }
    EXPECT(sr && sr->first_slot == mine[0].slot && sr->nnz == lengths[r]);
    const int32_t raw = static_cast<int32_t>(mine.size());
    std::vector<FoldGroup> groups;
    for (const FoldGroup &g : pl.fold)
      if (g.first_slot >= sr->first_slot && g.first_slot < sr->first_slot + raw) groups.push_back(g);
    if (raw > FOLD_MIN) {
      EXPECT(sr->slot_stride == FOLD_GROUP && sr->n_slots == (raw + FOLD_GROUP - 1) / FOLD_GROUP &&
             static_cast<int32_t>(groups.size()) == sr->n_slots && sr->n_slots <= FOLD_MIN);
      int32_t next = sr->first_slot;
      for (size_t g = 0; g < groups.size(); g++) {
        EXPECT(groups[g].first_slot == next && groups[g].first_slot == sr->first_slot + static_cast<int32_t>(g) * sr->slot_stride);
        EXPECT(groups[g].count >= 1 && groups[g].count <= FOLD_GROUP);
        next += groups[g].count;
      }
      EXPECT(next == sr->first_slot + raw);
    } else {
      EXPECT(sr->slot_stride == 1 && sr->n_slots == raw && groups.empty());
    }
  }
  EXPECT(pl.split.size() == n_split_rows);
  for (int used : seen_slot) EXPECT(used == 1);  // dense: every slot exactly once
  size_t fold_total = 0;
  for (const FoldGroup &g : pl.fold) fold_total += g.count;
  for (size_t i = 1; i < pl.split.size(); i++)  // most slots first, ties in row order
    EXPECT(pl.split[i - 1].n_slots > pl.split[i].n_slots ||
           (pl.split[i - 1].n_slots == pl.split[i].n_slots && pl.split[i - 1].row < pl.split[i].row));
  // the short tail, restated: whole rows only, it stops at the first task that is longer or owns a slot
  int32_t n_short = 0, n16 = 0, n8 = 0;
  for (int32_t i = pl.n_tasks - 1; i >= 0; i--) {
    const Task &a = pl.tasks[i];
    if (a.slot >= 0 || len(a) > SHORT_MAX) break;
    n_short++;
    n16 += len(a) <= 16;
    n8 += len(a) <= 8;
  }
  EXPECT(pl.n_short == n_short && pl.n_short16 == n16 && pl.n_short8 == n8);
  int64_t long_entries = 0;
  for (int32_t i = 0; i < pl.n_tasks - n_short; i++) long_entries += len(pl.tasks[i]);
  EXPECT(pl.long_entries == long_entries);
  // rows_by_len: every row of the range exactly once, longest first, ties in row order
  EXPECT(static_cast<int64_t>(pl.rows_by_len.size()) == re - rb);
  std::vector<int> seen_row(lengths.size(), 0);
  int32_t n_long = 0;
  for (size_t i = 0; i < pl.rows_by_len.size(); i++) {
    const int32_t r = pl.rows_by_len[i];
    EXPECT(r >= rb && r < re && seen_row[r]++ == 0);
    n_long += lengths[r] > 2048;
    if (i) {
      const int32_t q = pl.rows_by_len[i - 1];
      EXPECT(lengths[q] > lengths[r] || (lengths[q] == lengths[r] && q < r));
    }
  }
  EXPECT(pl.n_long == n_long);
  // the matrix-free classes: 128 < K <= 256 only
  if (K > 128 && K <= 256) {
    EXPECT(pl.mf_class[0] == 0 && pl.mf_class[MF_CLASSES] == re - rb);
    for (int c = 0; c < MF_CLASSES; c++) {
      EXPECT(pl.mf_class[c] <= pl.mf_class[c + 1]);
      for (int32_t i = pl.mf_class[c]; i < pl.mf_class[c + 1]; i++) {
        const int32_t n = lengths[pl.rows_by_len[i]];
        EXPECT(n <= MF_CAPS[c] && (c + 1 == MF_CLASSES || n > MF_CAPS[c + 1]));
      }
    }
    EXPECT(static_cast<int32_t>(pl.mf_lrows.size()) == pl.mf_class[1]);
    int32_t next_chunk = 0;
    for (size_t k = 0; k < pl.mf_lrows.size(); k++) {
      const MfLongRow &L = pl.mf_lrows[k];
      EXPECT(L.row == pl.rows_by_len[k] && L.first_chunk == next_chunk && L.n_chunks >= 1 && L.pad == 0);
      for (int32_t c = 0; c < L.n_chunks; c++) {
        const MfChunk &ch = pl.mf_chunks[L.first_chunk + c];
        EXPECT(ch.lrow == static_cast<int32_t>(k) && ch.pad == 0 && ch.end > ch.begin && ch.end - ch.begin <= MF_CHUNK + 15);
        EXPECT(ch.begin == (c ? pl.mf_chunks[L.first_chunk + c - 1].end : ip[L.row]) && (ch.begin - ip[L.row]) % 16 == 0);
      }
      EXPECT(pl.mf_chunks[L.first_chunk + L.n_chunks - 1].end == ip[L.row + 1]);
      next_chunk += L.n_chunks;
    }
    EXPECT(next_chunk == static_cast<int32_t>(pl.mf_chunks.size()));
  } else {
    EXPECT(pl.mf_lrows.empty() && pl.mf_chunks.empty());
    for (int c = 0; c <= MF_CLASSES; c++) EXPECT(pl.mf_class[c] == 0);
  }
  // the regulariser (float, like the reference), its minimum over the range, empty rows over the whole matrix
  EXPECT(static_cast<int64_t>(pl.reg.size()) == n_rows);
  bool has_empty = false;
  float reg_min = 0.f;
  for (int64_t r = 0; r < n_rows; r++) {
    const int64_t nz = lengths[r];
    const float want = cfg.reg * std::pow(cfg.alpha0 * n_cols + nz, cfg.nu);
    EXPECT(std::memcmp(&want, &pl.reg[r], sizeof(float)) == 0);
    has_empty |= nz == 0;
    if (r >= rb && r < re) reg_min = r == rb ? want : std::min(reg_min, want);
  }
  EXPECT(pl.has_empty == has_empty && pl.reg_min == reg_min);
  return pl;
}

static void task_plan_cases() {
  const int CH = 64;
  {  // chunk and chunk + 1 entries, an empty row, a short row; the second chunk of the split row has 29 entries
     // and a slot: it is NOT a short row, and the scan of the short tail stops there
    const TaskPlan pl = checked_plan({64, 65, 0, 8}, 0, 4, 64, CH, 64);
    EXPECT(same_list(pl.tasks, {Task{0, 0, 64, -1}, Task{1, 64, 100, 0}, Task{1, 100, 129, 1}, Task{3, 129, 137, -1},
                                Task{2, 129, 129, -1}}));
    EXPECT(same_list(pl.split, {SplitRow{1, 0, 2, 65, 1}}));
    EXPECT(pl.fold.empty() && pl.n_slots == 2);
    EXPECT(pl.n_short == 2 && pl.n_short16 == 2 && pl.n_short8 == 2 && pl.long_entries == 129);
    EXPECT((pl.rows_by_len == std::vector<int32_t>{1, 0, 3, 2}) && pl.n_long == 0 && pl.has_empty);
  }
  {  // the row classes 0, 8, 9, 16, 17, 32, 33 in a sub-range in the middle of the matrix
    const std::vector<int32_t> lengths = {5, 33, 32, 17, 16, 9, 8, 0, 40};
    const TaskPlan pl = checked_plan(lengths, 1, 8, 64, CH, 64);
    EXPECT(same_list(pl.tasks, {Task{1, 5, 38, -1}, Task{2, 38, 70, -1}, Task{3, 70, 87, -1}, Task{4, 87, 103, -1},
                                Task{5, 103, 112, -1}, Task{6, 112, 120, -1}, Task{7, 120, 120, -1}}));
    EXPECT(pl.split.empty() && pl.fold.empty() && pl.n_slots == 0);
    EXPECT(pl.n_short == 6 && pl.n_short16 == 4 && pl.n_short8 == 2 && pl.long_entries == 33);
    EXPECT((pl.rows_by_len == std::vector<int32_t>{1, 2, 3, 4, 5, 6, 7}) && pl.has_empty);
    // the empty row outside the range: has_empty looks at all rows, reg_min at the range only
    const TaskPlan in = checked_plan(lengths, 0, 7, 64, CH, 64);
    EXPECT(in.has_empty && in.n_short == 6 && in.n_short16 == 4 && in.n_short8 == 2);
    EXPECT(in.reg_min == in.reg[0] && pl.reg_min == pl.reg[7] && pl.reg[7] < in.reg[0]);
    // row_begin == row_end
    const TaskPlan none = checked_plan(lengths, 3, 3, 64, CH, 64);
    EXPECT(none.tasks.empty() && none.rows_by_len.empty() && none.n_short == 0 && none.reg_min == 0.f && none.has_empty);
    EXPECT(!checked_plan({5, 33, 32}, 1, 3, 64, CH, 64).has_empty);
  }
  {  // exactly 32 chunks: no fold group; exactly 33: three groups (16 + 16 + 1) behind three slots of stride 16
    const TaskPlan a = checked_plan({3, 2048}, 0, 2, 64, CH, 64);
    EXPECT(a.n_slots == 32 && a.fold.empty() && same_list(a.split, {SplitRow{1, 0, 32, 2048, 1}}));
    const TaskPlan b = checked_plan({3, 2112, 2048}, 0, 3, 64, CH, 64);
    EXPECT(b.n_slots == 65 && b.n_tasks == 66);
    EXPECT(same_list(b.fold, {FoldGroup{0, 16}, FoldGroup{16, 16}, FoldGroup{32, 1}}));
    EXPECT(same_list(b.split, {SplitRow{2, 33, 32, 2048, 1}, SplitRow{1, 0, 3, 2112, FOLD_GROUP}}));
    for (int32_t i = 0; i < 33; i++) EXPECT(same(b.tasks[i], Task{1, 3 + 64 * i, 3 + 64 * i + 64, i}));
    for (int32_t i = 0; i < 32; i++) EXPECT(same(b.tasks[33 + i], Task{2, 2115 + 64 * i, 2115 + 64 * i + 64, 33 + i}));
    EXPECT(same(b.tasks[65], Task{0, 0, 3, -1}) && b.n_short == 1 && b.long_entries == 2112 + 2048);
    const TaskPlan c = checked_plan({2049}, 0, 1, 64, CH, 64);  // 33 chunks of 64 (the last holds one entry)
    EXPECT(c.n_tasks == 33 && c.n_short == 0 && c.split[0].n_slots == 3 && c.tasks[32].end - c.tasks[32].begin == 1);
    EXPECT(c.n_long == 1 && a.n_long == 0);  // n_long: more than 2048 entries
  }
  {  // the cap of 256 chunks per row: 19200 entries would be 300 chunks of 64; chunks of 76 instead
    const TaskPlan pl = checked_plan({19200, 7}, 0, 2, 64, CH, 64);
    EXPECT(pl.n_slots == 253 && pl.tasks[0].end - pl.tasks[0].begin == 76 && pl.split[0].n_slots == 16 && pl.n_fold == 16);
    // chunk_long larger than the row: 32 chunks however long they get
    const TaskPlan lo = checked_plan({19200, 7}, 0, 2, 64, CH, 100000);
    EXPECT(lo.n_slots == 32 && lo.tasks[0].end - lo.tasks[0].begin == 600 && lo.fold.empty());
    // ... and in between: chunk_long = 128 asks for 150 chunks
    EXPECT(checked_plan({19200, 7}, 0, 2, 64, CH, 128).n_slots == 150);
  }
  {  // the matrix-free classes at every MF_CAPS boundary; present at K = 129 and 256, absent at 128
    static_assert(MF_NCAP == 320 && MF_CAPS[2] == 160 && MF_CAPS[3] == 80 && MF_CAPS[4] == 40 && MF_CHUNK == 1024, "");
    const std::vector<int32_t> lengths = {40, 321, 0, 80, 2049, 161, 41, 320, 160, 81};
    checked_plan(lengths, 0, 10, 128, 1024, 16384);
    for (const uint64_t K : {129, 256}) {
      const TaskPlan pl = checked_plan(lengths, 0, 10, K, 1024, 16384);
      EXPECT((pl.rows_by_len == std::vector<int32_t>{4, 1, 7, 5, 8, 9, 3, 6, 0, 2}));
      const int32_t want_class[MF_CLASSES + 1] = {0, 2, 4, 6, 8, 10};
      EXPECT(std::equal(want_class, want_class + MF_CLASSES + 1, pl.mf_class));
      // 2049 entries (row 4 starts at 441): three chunks of 688 = ceil(2049 / 3) rounded up to 16; 321: one chunk
      EXPECT(pl.mf_lrows.size() == 2 && pl.mf_lrows[0].row == 4 && pl.mf_lrows[0].n_chunks == 3 &&
             pl.mf_lrows[1].row == 1 && pl.mf_lrows[1].first_chunk == 3 && pl.mf_lrows[1].n_chunks == 1);
      EXPECT(pl.mf_chunks.size() == 4 && pl.mf_chunks[0].begin == 441 && pl.mf_chunks[0].end == 441 + 688 &&
             pl.mf_chunks[1].end == 441 + 1376 && pl.mf_chunks[2].end == 441 + 2049 && pl.mf_chunks[2].lrow == 0 &&
             pl.mf_chunks[3].begin == 40 && pl.mf_chunks[3].end == 361 && pl.mf_chunks[3].lrow == 1);
      EXPECT(pl.n_long == 1 && pl.n_split == 1);  // (2049 > the chunk of 1024: two tasks)
    }
    checked_plan(lengths, 2, 9, 192, 64, 64);
    checked_plan({2048, 2049, 2048}, 0, 3, 256, 64, 64);
  }
  {  // mixed lengths, every range
    std::vector<int32_t> lengths;
    uint32_t x = 12345;
    for (int r = 0; r < 60; r++) {
      x = x * 1664525u + 1013904223u;
      lengths.push_back(r % 11 == 0 ? 0 : r % 13 == 0 ? 64 * 33 + static_cast<int32_t>(x >> 28) : static_cast<int32_t>((x >> 16) % 200));
    }
    for (const uint64_t K : {64, 200})
      for (int64_t rb = 0; rb <= 60; rb += 12)
        for (int64_t re = rb; re <= 60; re += 15) checked_plan(lengths, rb, re, K, CH, 64);
  }
}

// the regulariser of a many-row matrix (several threads: parallel_ranges) against a sequential loop
static void reg_threaded() {
  const int64_t n_rows = 1100000, n_cols = 77777;
  std::vector<int32_t> ip(n_rows + 1, 0);
  for (int64_t r = 0; r < n_rows; r++) ip[r + 1] = ip[r] + static_cast<int32_t>((r * 2654435761u >> 7) % 23 % 9);
  const irs_ials_model_config cfg = config(64);
  const TaskPlan pl = plan_tasks(ip.data(), n_rows, n_cols, 1000, 2000, cfg, 64, 64);
  float reg_min = 0.f;
  for (int64_t r = 0; r < n_rows; r++) {
    const int64_t nz = ip[r + 1] - ip[r];
    const float want = cfg.reg * std::pow(cfg.alpha0 * n_cols + nz, cfg.nu);
    EXPECT(std::memcmp(&want, &pl.reg[r], sizeof(float)) == 0);
    if (r >= 1000 && r < 2000) reg_min = r == 1000 ? want : std::min(reg_min, want);
  }
  EXPECT(pl.reg_min == reg_min && pl.n_tasks == 1000 && pl.has_empty);
}

// ---------------------------------------------------------------- the route, against the former conditions
// what launch_solve decided, in the words it used (`t->` and `sd.` dropped; `other == t->factor[1 - pidx].ptr` is
// other_own, `target == t->factor[pidx].ptr` is target_own, `prior` a flag)
struct Literal {
  int path;  // 0 launch_ialspp (1: its general branch), 2 launch_gk_solve, 3 launch_mf_cg, 4 the dense kernels
  bool pp_direct, cg, unit, short_cg_ok, short_forked, eig_cand;
  int family;  // 0 T <= 4, 1 T == 8, 2 wg16, 3 wg
  bool x3, x3_split, x3_declined;
  int32_t n_regular;
};
static bool literal_eig_begin(const SolveFacts &f, bool cg) {
  const int KP = f.KP;
  if (!f.opt_eig || (KP != 64 && KP != 128) || !f.positive || f.n_short <= 0) return false;
  if (static_cast<double>(f.n_short) * KP * KP * KP < 3e11) return false;
  const double ratio = cg ? 64.0 : 8.0;
  if (static_cast<double>(f.n_short) * KP < ratio * static_cast<double>(f.n_other)) return false;
  return true;
}
static Literal literal_route(const SolveFacts &f) {
  Literal L{};
  const int T = f.T;
  const bool prior = f.has_prior;
  bool pp_direct = false;
  if (f.solver_type == IRS_SOLVER_IALSPP) {
    pp_direct = f.opt_pp_direct && f.subspace_dimension > 1 &&
                static_cast<uint64_t>(f.subspace_dimension) >= static_cast<uint64_t>(f.K) && f.sweeps >= 1 && T <= 4 &&
                f.target_own;
    if (!pp_direct) {
      L.path = (f.subspace_dimension > 64 || f.KP > 2048) ? 1 : 0;
      return L;
    }
  }
  L.pp_direct = pp_direct;
  if (f.KP > 256) {
    L.path = 2;
    return L;
  }
  if (f.solver_type == IRS_SOLVER_CG && T > 8 && !prior && f.opt_mf) {
    L.path = 3;
    return L;
  }
  L.path = 4;
  const int32_t zero_row = static_cast<int32_t>(ceil_div(f.n_other, 8) * 8);
  (void)zero_row;  // (the enumeration sets zero_row itself, on each side of the limit)
  const bool unit = f.unit && f.opt_unit && f.other_own &&
                    static_cast<uint64_t>(f.zero_row + 8) * f.KP * sizeof(float) < (uint64_t(1) << 32);
  const bool cg = f.solver_type == IRS_SOLVER_CG;
  int n_regular = f.n_tasks;
  const bool short_cg_ok = cg && !prior && f.n_short > 0 && (T <= 4 || T == 8) && f.opt_short;
  const bool eig_cand = !prior && !pp_direct && f.other_own && literal_eig_begin(f, cg);
  bool short_forked = false;
  if (eig_cand) {
    n_regular = f.n_tasks - f.n_short;
  } else if (short_cg_ok) {
    if (f.n_short >= 65536) short_forked = true;
    n_regular = f.n_tasks - f.n_short;
  }
  L.cg = cg;
  L.unit = unit;
  L.short_cg_ok = short_cg_ok;
  L.short_forked = short_forked;
  L.eig_cand = eig_cand;
  L.n_regular = n_regular;
  // launch_dense(tasks, count, with_split): (n_regular, true), and (n_short, false) after the eigenbasis declined
  auto dense = [&](int count, bool &x3_out, bool &x3_split_out) {
    const int n_regular = count;
    x3_out = x3_split_out = false;
    if (!cg && (T >= 12 || (T == 8 && !f.opt_wave128)) && f.opt_wg16) {
      L.family = 2;
    } else if (T == 8 && f.opt_wave128) {
      L.family = 1;
      const bool x3_any = f.unit && f.opt_unit && f.other_own && f.opt_bf16x3;
      const bool x3 = x3_any && (cg || f.long_entries >= int64_t(320) * std::max(n_regular, 1));
      x3_out = x3;  // (cg && x3) / x3 pick the <8, ., 0, true, true> kernels
      x3_split_out = cg && f.unit && f.opt_unit && f.other_own && f.opt_bf16x3;
    } else if (T <= 4) {
      L.family = 0;
      // regular: pp_direct && unit && opt_bf16x3 && TT == 4 / cg && unit && opt_bf16x3 && TT == 4 /
      // unit && opt_bf16x3 && TT == 4, in this order
      x3_out = (pp_direct && unit && f.opt_bf16x3 && T == 4) || (!pp_direct && cg && unit && f.opt_bf16x3 && T == 4) ||
               (!pp_direct && !cg && unit && f.opt_bf16x3 && T == 4);
      x3_split_out = !pp_direct && cg && unit && f.opt_bf16x3 && T == 4;
    } else {
      L.family = 3;
    }
  };
  bool unused = false;
  dense(f.n_short, L.x3_declined, unused);
  dense(n_regular, L.x3, L.x3_split);
  return L;
}

static void compare_route(const SolveFacts &f) {
  const SolveRoute r = solve_route(f);
  const Literal L = literal_route(f);
  const int path = r.path == SolvePath::PP_BLOCKS ? 0 : r.path == SolvePath::PP_GENERAL ? 1 : r.path == SolvePath::GK ? 2
                   : r.path == SolvePath::MF_CG ? 3 : 4;
  EXPECT(path == L.path && r.pp_direct == L.pp_direct);
  if (path != 4) return;
  const int family = r.family == DenseFamily::WAVE ? 0 : r.family == DenseFamily::WAVE8 ? 1 : r.family == DenseFamily::WG16 ? 2 : 3;
  EXPECT(r.cg == L.cg && r.unit == L.unit && family == L.family);
  EXPECT(r.x3 == L.x3 && r.x3_split == L.x3_split && r.x3_declined == L.x3_declined);
  EXPECT(r.short_cg_ok == L.short_cg_ok && r.short_fork == L.short_forked && r.eig_candidate == L.eig_cand);
  EXPECT(r.n_regular == L.n_regular);
}

// launch_ialspp's own choices, in its former words
static void compare_pp(uint64_t subspace_dimension, int64_t K, int KP, bool opt_pp_chain) {
  const PpVariant v = pp_variant(subspace_dimension, K, KP, opt_pp_chain);
  const bool general = subspace_dimension > 64 || KP > 2048;
  EXPECT(v.general == general);
  if (general) {
    EXPECT(v.sub == static_cast<int32_t>(std::min<uint64_t>(std::max<uint64_t>(1, subspace_dimension), K)));
    return;
  }
  const int32_t p_sub = static_cast<int32_t>(std::max<uint64_t>(1, subspace_dimension));
  const int32_t p_K = static_cast<int32_t>(K);
  const int p_chain = opt_pp_chain ? 1 : 0;
  const bool pack = p_chain && p_sub == 64 && p_K > 64;
  const int D = std::min<int>(p_sub, p_K);
  const int TS = D <= 16 ? 1 : D <= 32 ? 2 : 4;
  const bool aligned = p_sub % TS == 0;
  const bool single = p_sub >= p_K;
  const bool chained = !single && TS == 4 && aligned && p_chain && p_sub == 64 && p_K > 64;
  EXPECT(v.sub == p_sub && v.TS == TS && v.aligned == aligned && v.single == single && v.chained == chained);
  EXPECT(chained == pack);  // (the packed P is made exactly for the chained sweeps)
}

static void route_enumeration() {
  const int Ts[] = {1, 2, 3, 4, 8, 12, 16, 20};
  const int32_t solvers[] = {IRS_SOLVER_CHOLESKY, IRS_SOLVER_CG, IRS_SOLVER_IALSPP};
  // under ThreadSanitizer (every access instrumented) the 2^11 switch settings are strided; the other builds
  // take all of them
  const unsigned mask_step = kThreadSanitizer ? 29 : 1;
  std::atomic<long long> n_checked(0);
  std::atomic<int> next_item(0);  // work items: (T, solver)
  run_on_threads(8, [&](int) {
    long long mine = 0;
    for (int item = next_item++; item < 8 * 3; item = next_item++) {
      SolveFacts f;
      f.T = Ts[item / 3];
      f.KP = 16 * f.T;
      f.solver_type = solvers[item % 3];
      const int64_t K = f.KP - 3;  // (so that a subspace dimension of K, K + 1 and KP are three different things)
      f.K = K;
      const uint64_t subs[] = {0, 1, 16, 48, 64, 65, static_cast<uint64_t>(K), static_cast<uint64_t>(K + 1)};
      for (const uint64_t sub : subs)
        for (const bool chain : {false, true}) compare_pp(sub, K, f.KP, chain);
      f.n_tasks = 1 << 22;
      f.n_other = 1 << 20;
      // n_short on each side of: the fork (65536), n_short KP^3 >= 3e11, n_short KP >= ratio n_other (64 under
      // CG, 8 otherwise)
      const double kp3 = static_cast<double>(f.KP) * f.KP * f.KP;
      const int32_t at_3e11 = static_cast<int32_t>(std::min(3e11 / kp3, 4e6));
      const int32_t at_ratio = static_cast<int32_t>((f.solver_type == IRS_SOLVER_CG ? 64 : 8) * f.n_other / f.KP);
      const int32_t shorts[] = {0, 1, 65535, 65536, at_3e11 - 1, at_3e11 + 2, at_ratio - 1, at_ratio};
      const int64_t limit_rows = ceil_div(int64_t(1) << 32, f.KP * 4);  // (zero_row + 8) KP 4 < 2^32 below it
      for (const uint64_t sub : subs)
        for (const uint64_t sweeps : {0, 1, 2})
          for (unsigned mask = 0; mask < 2048; mask += mask_step)
            for (unsigned flags = 0; flags < 32; flags++)
              for (const int32_t n_short : shorts) {
                f.subspace_dimension = sub;
                f.sweeps = sweeps;
                f.opt_wave128 = mask & 1, f.opt_unit = mask & 2, f.opt_short = mask & 4, f.opt_short2 = mask & 8;
                f.opt_wg16 = mask & 16, f.opt_bf16x3 = mask & 32, f.opt_pp_direct = mask & 64, f.opt_pp_chain = mask & 128;
                f.opt_pp_fork = mask & 256, f.opt_eig = mask & 512, f.opt_mf = mask & 1024;
                f.has_prior = flags & 1, f.other_own = flags & 2, f.target_own = flags & 4;
                f.unit = flags & 8, f.positive = flags & 16;
                f.n_short = n_short;
                f.n_short16 = n_short / 2;
                for (const int side : {0, 1}) {
                  // long_entries on each side of 320 x the tasks of the launch: all tasks, all but the short
                  // ones, or - the dense launch after the eigenbasis declined - the short ones.  Only T = 8
                  // reads it; the other sizes take the first.
                  f.zero_row = limit_rows - 8 - 1 + side;
                  f.long_entries = int64_t(320) * f.n_tasks - 1 + side;
                  compare_route(f);
                  mine++;
                  if (f.T != 8) continue;
                  f.long_entries = int64_t(320) * (f.n_tasks - n_short) - 1 + side;
                  compare_route(f);
                  f.long_entries = int64_t(320) * std::max(n_short, 1) - 1 + side;
                  f.zero_row = limit_rows - 8 - side;
                  compare_route(f);
                  mine += 2;
                }
              }
    }
    n_checked += mine;
  });
  std::printf("route: %lld settings compared\n", n_checked.load());
}

static void small_functions() {
  EXPECT(padded_k(1) == 16 && padded_k(16) == 16 && padded_k(17) == 32 && padded_k(32) == 32 && padded_k(33) == 64 &&
         padded_k(64) == 64 && padded_k(65) == 128 && padded_k(128) == 128 && padded_k(129) == 192 &&
         padded_k(256) == 256 && padded_k(257) == 320 && padded_k(32768) == 32768);
  EXPECT(cg_step_count(0, 77) == 77 && cg_step_count(3, 77) == 3 && cg_step_count(1u << 20, 77) == (1 << 20) &&
         cg_step_count((1u << 20) + 1, 77) == (1 << 20) && cg_step_count(~uint64_t(0), 77) == (1 << 20));
  // conditioning: lo = max(0, lam_min) + reg_min > 0, hi = lam_max + reg_min <= 1e4 lo, hi finite
  EXPECT(eig_well_conditioned(100.f, 1.f, 0.f) && eig_well_conditioned(1e4f, 1.f, 0.f) && !eig_well_conditioned(10001.f, 1.f, 0.f));
  EXPECT(!eig_well_conditioned(1.f, 0.f, 0.f) && !eig_well_conditioned(1.f, -1.f, 0.f) && eig_well_conditioned(1.f, -1.f, 0.5f));
  EXPECT(!eig_well_conditioned(INFINITY, 1.f, 1.f) && !eig_well_conditioned(NAN, 1.f, 1.f));
  // the cuts of a pass, against the former expressions, for every pass of several lists
  for (const int32_t n_short : {0, 1, 7, 64, 100})
    for (int32_t n16 = 0; n16 <= n_short; n16 += 3)
      for (int32_t n8 = 0; n8 <= n16; n8 += 2)
        for (const int32_t B : {1, 5, 64, 1000})
          for (int32_t b0 = 0; b0 < n_short; b0 += B) {
            const int32_t m = std::min(B, n_short - b0);
            const int32_t n32 = n_short - n16;
            const int32_t n16rows = n_short - n8;
            const int32_t m2 = std::max(0, std::min(b0 + m, n32) - b0);
            const int32_t m3 = std::max(m2, std::min(b0 + m, n16rows) - b0);
            const EigCuts c = eig_pass_cuts(b0, m, n_short, n16, n8);
            EXPECT(c.m2 == m2 && c.m3 == m3 && 0 <= c.m2 && c.m2 <= c.m3 && c.m3 <= m);
          }
}

int main() {
  task_plan_cases();
  reg_threaded();
  small_functions();
  route_enumeration();
  std::printf("ials_host_plan ok\n");
  return 0;
}
