// SolveRoute::x3_lds (irspack_amd/csrc/ials_host_plan.hpp): which half-steps stage the bf16x3 gather in LDS.  No HIP;
// built and run by tests/test_ials_gather_lds_route.py.  The expectation is the sentence of DESIGN 3.1 written as
// one condition: binary interactions on the UNIT kernels, the bf16x3 rank update, K padded to 64, Cholesky (not CG,
// not the gradient form of iALS++), a gathered table of at most 16 MiB (both sides of the limit), and the switch.
// Every other field of the route must not move with the switch.
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

static bool same_but_lds(SolveRoute a, SolveRoute b) {
  a.x3_lds = b.x3_lds = false;
  return a.path == b.path && a.pp_direct == b.pp_direct && a.cg == b.cg && a.unit == b.unit && a.family == b.family &&
         a.x3 == b.x3 && a.x3_split == b.x3_split && a.x3_declined == b.x3_declined && a.short_cg_ok == b.short_cg_ok &&
         a.short_fork == b.short_fork && a.eig_candidate == b.eig_candidate && a.n_regular == b.n_regular;
}

int main() {
  EXPECT(!Switches{}.opt_gather_lds);  // (a trainer sets it from IRSPACK_AMD_IALS_GATHER_LDS, default on)
  const int Ts[] = {1, 2, 3, 4, 8, 12, 16, 20};
  const int32_t solvers[] = {IRS_SOLVER_CHOLESKY, IRS_SOLVER_CG, IRS_SOLVER_IALSPP};
  long long n = 0, n_lds = 0;
  for (const int T : Ts)
    for (const int32_t solver : solvers)
      for (const uint64_t sub : {uint64_t(0), uint64_t(16), uint64_t(64), uint64_t(16 * T)})
        for (unsigned mask = 0; mask < 32; mask++)
          for (unsigned flags = 0; flags < 32; flags++)
            for (const int side : {0, 1, 2, 3}) {
              SolveFacts f;
              f.T = T;
              f.KP = 16 * T;
              f.K = f.KP - 3;
              f.solver_type = solver;
              f.subspace_dimension = sub;
              f.sweeps = 1;
              f.n_tasks = 1 << 20;
              f.n_other = (int64_t(16) << 20) / (f.KP * 4) + (side >> 1);  // 16 MiB of rows, and one row more
              f.n_short = 1000;
              f.n_short16 = 500;
              f.long_entries = int64_t(1) << 28;
              f.opt_unit = mask & 1, f.opt_bf16x3 = mask & 2, f.opt_pp_direct = mask & 4, f.opt_eig = mask & 8;
              f.opt_wave128 = mask & 16;
              f.has_prior = flags & 1, f.other_own = flags & 2, f.target_own = flags & 4;
              f.unit = flags & 8, f.positive = flags & 16;
              // the gathered table on each side of the 4 GB limit of 32-bit byte offsets
              const int64_t limit_rows = ceil_div(int64_t(1) << 32, f.KP * 4);
              f.zero_row = limit_rows - 8 - 1 + (side & 1);
              f.opt_gather_lds = false;
              const SolveRoute off = solve_route(f);
              f.opt_gather_lds = true;
              const SolveRoute on = solve_route(f);
              EXPECT(!off.x3_lds);
              EXPECT(same_but_lds(on, off));
              const bool dense_wave = on.path == SolvePath::DENSE && on.family == DenseFamily::WAVE;
              const bool want = dense_wave && T == 4 && solver == IRS_SOLVER_CHOLESKY && f.unit && f.opt_unit &&
                                f.other_own && f.opt_bf16x3 && (side >> 1) == 0 &&
                                static_cast<uint64_t>(f.zero_row + 8) * f.KP * sizeof(float) < (uint64_t(1) << 32);
              EXPECT(on.x3_lds == want);
              if (on.x3_lds) EXPECT(on.x3 && on.x3_declined && !on.x3_split && !on.cg && !on.pp_direct && on.unit);
              n++;
              n_lds += on.x3_lds;
            }
  EXPECT(n_lds > 0 && n_lds < n);
  std::printf("x3_lds: %lld settings, %lld staged in LDS\nials_gather_lds_route ok\n", n, n_lds);
  return 0;
}
