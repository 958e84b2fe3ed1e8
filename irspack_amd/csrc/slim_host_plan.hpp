// Host decision of the SLIM descent (slim.hip): where the running vector of a column lives and the launch
// shape of slim_descent_kernel that follows from it.  No HIP in it: it compiles with the host compiler alone
// (tests/host/slim_host_plan_main.cpp); slim_kernels.hpp takes the LDS layout constants from here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace irs {
namespace slim {

constexpr int kMaxWaves = 16;  // waves of a descent workgroup (1024 threads)
// fixed head of the descent kernel's dynamic LDS (bytes): two buffers of per-wave (ballot, delta) slots
// and the column handed out by the cursor; the running vector follows it (16-byte aligned, Guideline 17)
constexpr int kSlotBytes = 2 * kMaxWaves * 8 + 2 * kMaxWaves * 4 + 16;
static_assert(kSlotBytes % 16 == 0, "the running vector starts 16-byte aligned");

struct LaunchPlan {
  bool lds_r = false;              // the running vector in LDS (else: a global scratch row per workgroup)
  int lds_bytes = 0;               // dynamic LDS of the launch
  int threads = 0;                 // workgroup size = chunk width
  int n_wg = 0;                    // persistent workgroups
  bool raise_dynamic_lds = false;  // the kernel's dynamic-LDS limit has to be raised before the launch
};

// cols: items of the catalogue; lds_per_block / lds_per_cu / n_cu: sharedMemPerBlock,
// maxSharedMemoryPerMultiProcessor and multiProcessorCount of the device; lds_flag: IRSPACK_AMD_SLIM_LDS
inline LaunchPlan plan_launch(int64_t cols, size_t lds_per_block, size_t lds_per_cu, int n_cu, bool lds_flag) {
  const size_t I = static_cast<size_t>(cols);
  LaunchPlan p;
  const int lds_need = kSlotBytes + static_cast<int>(std::min<size_t>(I * 4, size_t(1) << 30));
  p.lds_r = lds_flag && I * 4 + kSlotBytes <= lds_per_block;
  p.lds_bytes = p.lds_r ? lds_need : kSlotBytes;
  // few workgroups fit beside a large LDS image: make each one wide (every wave streams the axpy)
  p.threads = p.lds_bytes > 80 * 1024 ? 1024 : p.lds_bytes > 40 * 1024 ? 512 : 256;
  const int per_cu =
      std::max(1, std::min<int>(2048 / p.threads, static_cast<int>(lds_per_cu / std::max(p.lds_bytes, 1))));
  p.n_wg = static_cast<int>(std::min<int64_t>(cols, int64_t(n_cu) * std::min(per_cu, 4)));
  p.raise_dynamic_lds = p.lds_bytes > 64 * 1024;
  return p;
}

}  // namespace slim
}  // namespace irs
