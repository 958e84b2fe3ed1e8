// Plain structs and constants of the iALS path that the host writes and the kernels read (no HIP
// dependency): the task list of a side (ials_kernels.hpp), the short-row limit (ials_short_kernels.hpp)
// and the row classes of the matrix-free CG (ials_mf_kernels.hpp).  Included by those kernel headers and by
// ials_host_plan.hpp, which fills them.
#pragma once
#include <cstdint>

namespace irs {
namespace ials {

struct Task {
  int32_t row;    // row of the solved side
  int32_t begin;  // [begin, end) into indices / data
  int32_t end;
  int32_t slot;   // < 0: whole row, solve inline; >= 0: partial Gramian slot
};

struct SplitRow {
  int32_t row;
  int32_t first_slot;
  int32_t n_slots;      // slots the second kernel adds: first_slot + i * slot_stride
  int32_t nnz;
  int32_t slot_stride;  // 1, or FOLD_GROUP once fold_partials_kernel has summed each group into its first slot
};

// A row cut into more than FOLD_MIN chunks has its partial Gramians summed in groups of
// FOLD_GROUP first (one thread per float4 of the partial, every group in parallel), so that the
// one wave (or workgroup) that finishes the row adds at most FOLD_MIN partials one after another.
constexpr int FOLD_GROUP = 16;
constexpr int FOLD_MIN = 32;
struct FoldGroup {
  int32_t first_slot;
  int32_t count;
};

constexpr int SHORT_MAX = 32;    // rows up to this many stored entries take a short kernel

#ifndef IRS_MF_J
#define IRS_MF_J 10
#endif
constexpr int MF_J = IRS_MF_J;           // groups of four gathered rows a wave keeps in registers
constexpr int MF_NCAP = 32 * MF_J;       // longest resident row: 8 waves x MF_J groups of 4 entries
// row classes by stored entries, longest first: class 0 = level-synchronous, then the resident
// classes of mf_cg_rows_kernel<KP, R, W, 10> (capacity 40 W): <1, 8>, <1, 4>, <2, 2>, <4, 1>
constexpr int MF_CHUNK = 1024;  // entries per chunk of a level-synchronous row
constexpr int MF_CLASSES = 5;
constexpr int32_t MF_CAPS[MF_CLASSES] = {INT32_MAX, MF_NCAP, 16 * MF_J, 8 * MF_J, 4 * MF_J};

struct MfLongRow {
  int32_t row;          // row of the solved side
  int32_t first_chunk;  // chunks [first_chunk, first_chunk + n_chunks) in row order
  int32_t n_chunks;
  int32_t pad;
};
struct MfChunk {
  int32_t lrow;   // index into the long-row list
  int32_t begin;  // [begin, end) into indices / data
  int32_t end;
  int32_t pad;
};

}  // namespace ials
}  // namespace irs
