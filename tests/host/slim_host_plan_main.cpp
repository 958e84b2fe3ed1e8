// irspack_amd/csrc/slim_host_plan.hpp in a program of its own, for the sanitizers (tests/test_host_sanitizers.py
// builds it with -fsanitize=address,undefined, every report fatal, and at -O3).  The expectations are written out by
// hand from the rule, not computed by the code under test:
//   LDS need = 400 + 4 I bytes (the I * 4 term clamped to 2^30); in LDS when the switch is on and the need is at
//   most the per-block limit, else 400 bytes of slots only; 256 threads up to 40 KiB, 512 up to 80 KiB, 1024 above;
//   workgroups per CU = min(2048 / threads, per-CU LDS / LDS bytes), at least 1, at most 4; workgroups =
//   min(items, CUs x that); the dynamic-LDS limit is raised above 64 KiB.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../irspack_amd/csrc/slim_host_plan.hpp"

using namespace irs::slim;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static int n_cases = 0;

static void expect(int64_t cols, size_t per_block, size_t per_cu, int n_cu, bool flag, bool lds_r, int lds_bytes,
                   int threads, int n_wg, bool raise, int line) {
  const LaunchPlan p = plan_launch(cols, per_block, per_cu, n_cu, flag);
  if (p.lds_r != lds_r || p.lds_bytes != lds_bytes || p.threads != threads || p.n_wg != n_wg ||
      p.raise_dynamic_lds != raise) {
    std::fprintf(stderr,
                 "%s:%d: items %lld: got {lds_r %d, lds_bytes %d, threads %d, n_wg %d, raise %d}, expected "
                 "{%d, %d, %d, %d, %d}\n",
                 __FILE__, line, static_cast<long long>(cols), int(p.lds_r), p.lds_bytes, p.threads, p.n_wg,
                 int(p.raise_dynamic_lds), int(lds_r), lds_bytes, threads, n_wg, int(raise));
    std::exit(1);
  }
  n_cases++;
}
#define EXPECT(...) expect(__VA_ARGS__, __LINE__)

int main() {
  CHECK(kMaxWaves == 16);
  CHECK(kSlotBytes == 400);  // 2 x 16 ballots of 8 bytes, 2 x 16 deltas of 4, 16 for the column

  constexpr size_t K64 = 65536, K160 = 163840;
  constexpr int CU = 256;  // 256 CUs with 160 KiB each: 4 workgroups per CU at most = 1,024 device-wide

  // ---- the three widths, per-block limit 160 KiB -----------------------------------------------------------------
  //     items  block  per CU  CUs  flag   lds_r  bytes   threads  n_wg  raise
  EXPECT(1, K160, K160, CU, true, true, 404, 256, 1, false);
  EXPECT(2, K160, K160, CU, true, true, 408, 256, 2, false);
  // 400 + 4 x 10,140 = 40,960 = 40 KiB: the last 256-thread size; min(8, 163,840 / 40,960 = 4) -> 4 per CU
  EXPECT(10140, K160, K160, CU, true, true, 40960, 256, 1024, false);
  // 40,964 bytes: 512 threads; min(4, 163,840 / 40,964 = 3) -> 3 per CU
  EXPECT(10141, K160, K160, CU, true, true, 40964, 512, 768, false);
  // 400 + 4 x 16,284 = 65,536 = 64 KiB: the last size below the raised limit; min(4, 2) -> 2 per CU
  EXPECT(16284, K160, K160, CU, true, true, 65536, 512, 512, false);
  EXPECT(16285, K160, K160, CU, true, true, 65540, 512, 512, true);
  // 400 + 4 x 20,380 = 81,920 = 80 KiB: the last 512-thread size
  EXPECT(20380, K160, K160, CU, true, true, 81920, 512, 512, true);
  // 81,924 bytes: 1024 threads; min(2, 163,840 / 81,924 = 1) -> 1 per CU
  EXPECT(20381, K160, K160, CU, true, true, 81924, 1024, 256, true);
  EXPECT(20480, K160, K160, CU, true, true, 82320, 1024, 256, true);
  EXPECT(26744, K160, K160, CU, true, true, 107376, 1024, 256, true);  // the ML-20M catalogue
  // the per-block edge at 160 KiB: 400 + 4 x 40,860 = 163,840 fits, 40,861 does not (then 256 threads, 4 per CU)
  EXPECT(40860, K160, K160, CU, true, true, 163840, 1024, 256, true);
  EXPECT(40861, K160, K160, CU, true, false, 400, 256, 1024, false);
  EXPECT(70000, K160, K160, CU, true, false, 400, 256, 1024, false);

  // ---- per-block limit 64 KiB ------------------------------------------------------------------------------------
  EXPECT(10140, K64, K160, CU, true, true, 40960, 256, 1024, false);
  EXPECT(10141, K64, K160, CU, true, true, 40964, 512, 768, false);
  EXPECT(16284, K64, K160, CU, true, true, 65536, 512, 512, false);  // the last that fits: never a raised limit
  EXPECT(16285, K64, K160, CU, true, false, 400, 256, 1024, false);
  EXPECT(20380, K64, K160, CU, true, false, 400, 256, 1024, false);
  EXPECT(20381, K64, K160, CU, true, false, 400, 256, 1024, false);
  // 64 KiB per CU as well: min(4, 65,536 / 40,964 = 1) -> 1 per CU; min(8, 65,536 / 40,960 = 1) -> 1 per CU
  EXPECT(10141, K64, K64, CU, true, true, 40964, 512, 256, false);
  EXPECT(10140, K64, K64, CU, true, true, 40960, 256, 256, false);
  EXPECT(16284, K64, K64, CU, true, true, 65536, 512, 256, false);

  // ---- the switch off at sizes that would fit ---------------------------------------------------------------------
  EXPECT(5000, K160, K160, CU, false, false, 400, 256, 1024, false);
  EXPECT(1, K160, K160, CU, false, false, 400, 256, 1, false);
  EXPECT(20381, K160, K160, CU, false, false, 400, 256, 1024, false);
  EXPECT(16284, K64, K160, CU, false, false, 400, 256, 1024, false);

  // ---- workgroups: items below and above the device-wide count, at most 4 per CU ---------------------------------
  // 256 threads, 404 + ... bytes: min(8, many) = 8 per CU by threads and LDS, capped at 4
  EXPECT(39, K160, K160, 10, true, true, 556, 256, 39, false);
  EXPECT(40, K160, K160, 10, true, true, 560, 256, 40, false);
  EXPECT(41, K160, K160, 10, true, true, 564, 256, 40, false);
  EXPECT(2000, K160, K160, 10, true, true, 8400, 256, 40, false);
  EXPECT(1023, K160, K160, CU, true, true, 4492, 256, 1023, false);
  EXPECT(1025, K160, K160, CU, true, true, 4500, 256, 1024, false);
  // 8,000 items: 32,400 bytes, min(8, 163,840 / 32,400 = 5) = 5, capped at 4
  EXPECT(8000, K160, K160, 8, true, true, 32400, 256, 32, false);
  // 9,000 items: 36,400 bytes, min(8, 4) = 4; with 100,000 bytes per CU min(8, 2) = 2
  EXPECT(9000, K160, K160, 8, true, true, 36400, 256, 32, false);
  EXPECT(9000, K160, 100000, 8, true, true, 36400, 256, 16, false);
  // the LDS of a CU smaller than one image: still one workgroup per CU
  EXPECT(20381, K160, K64, 8, true, true, 81924, 1024, 8, true);
  EXPECT(5, K160, K64, 8, true, true, 420, 256, 5, false);
  // the global path's 400 bytes: 4 per CU whatever the catalogue
  EXPECT(100000, K160, K160, 8, true, false, 400, 256, 32, false);

  // ---- I = 2^31 - 1: I * 4 is clamped to 2^30, so the need (400 + 2^30 = 1,073,742,224) stays inside an int ------
  constexpr int64_t IMAX = 2147483647;
  EXPECT(IMAX, K160, K160, CU, true, false, 400, 256, 1024, false);
  EXPECT(IMAX, K64, K160, CU, false, false, 400, 256, 1024, false);
  // (a limit no device has, to see the clamped figure itself; the true need, 8,589,934,988, is below it;
  // min(2048 / 1024, 2^40 / 1,073,742,224 = 1,023) = 2 per CU)
  EXPECT(IMAX, size_t(1) << 40, size_t(1) << 40, CU, true, true, 1073742224, 1024, 512, true);
  // above the clamp but under 2^31 bytes: 300,000,000 items need 1,200,000,400 bytes, reported as 400 + 2^30
  EXPECT(300000000, size_t(1) << 40, size_t(1) << 40, CU, true, true, 1073742224, 1024, 512, true);
  // the last catalogue below the clamp: 4 x 268,435,456 = 2^30
  EXPECT(268435456, size_t(1) << 40, size_t(1) << 40, CU, true, true, 1073742224, 1024, 512, true);
  EXPECT(268435455, size_t(1) << 40, size_t(1) << 40, CU, true, true, 1073742220, 1024, 512, true);

  CHECK(n_cases == 44);
  std::printf("slim_host_plan ok\n");
  return 0;
}
