// The host rule of the evaluator's *_scored model calls (irspack_amd/csrc/eval_host_prep.hpp: scored_width) on its
// own: no HIP, built with -fsanitize=address,undefined by tests/test_eval_scored_width_host.py.  The rule stands in
// front of every launch of such a call: the item operand is n_scored columns wide, the block n_items, and the fill
// kernel writes the columns in between - a width outside 1 .. n_items would make the score kernels or the fill
// write outside the block.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "../../irspack_amd/csrc/eval_host_prep.hpp"

using namespace irs;
using namespace irs::eval;

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

template <class F> static std::string error_of(F &&f) {
  try {
    f();
  } catch (const std::invalid_argument &e) {
    return e.what();
  }
  return "";
}

static const char *REFUSED = "n_scored must lie in 1 .. n_items.";

int main() {
  // every width of small catalogues, both sides of both ends
  for (int64_t ni = 0; ni <= 70; ni++)
    for (int64_t ns = -2; ns <= ni + 2; ns++) {
      const std::string err = error_of([&] { EXPECT(scored_width(ns, ni) == ns); });
      EXPECT((err == "") == (ns >= 1 && ns <= ni));
      EXPECT(err == "" || err == REFUSED);
    }
  // the sizes at which the score kernels change tiles: a 64-column MFMA tile, a 256-column strip, a 2,048-column tile
  for (int64_t edge : {64, 256, 2048})
    for (int64_t ns = edge - 1; ns <= edge + 1; ns++)
      for (int64_t ni = edge - 1; ni <= edge + 1; ni++)
        EXPECT((error_of([&] { scored_width(ns, ni); }) == "") == (ns <= ni));
  // the ends of the range of the arguments: no overflow on the way to the answer
  const int64_t big = std::numeric_limits<int64_t>::max(), low = std::numeric_limits<int64_t>::min();
  EXPECT(scored_width(big, big) == big && scored_width(1, big) == 1);
  EXPECT(error_of([&] { scored_width(big, big - 1); }) == REFUSED);
  EXPECT(error_of([&] { scored_width(low, big); }) == REFUSED);
  EXPECT(error_of([&] { scored_width(1, low); }) == REFUSED);
  EXPECT(error_of([&] { scored_width(0, 0); }) == REFUSED);  // (an evaluator without items has nothing to score)
  std::printf("eval_scored_width ok\n");
  return 0;
}
