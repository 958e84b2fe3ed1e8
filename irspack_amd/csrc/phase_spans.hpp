// Phase timing with HIP events: an event pair round a phase of a call, folded into ms[] after the call's
// synchronisation (NMF, the truncated SVD, BPR / WARP, Mult-VAE), and the bare Event for a caller's own pairs.
#pragma once
#include <memory>
#include <vector>

#include "common.hpp"

namespace irs {

struct Event {
  hipEvent_t e = nullptr;
  Event() { IRS_HIP(hipEventCreate(&e)); }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
};

inline double elapsed_ms(const Event &a, const Event &b) {
  float ms = 0.f;
  IRS_HIP(hipEventElapsedTime(&ms, a.e, b.e));
  return static_cast<double>(ms);
}

// N phases.  While `enabled` is false a span records nothing, so the untimed path creates no event.
template <int N> struct PhaseSpans {
  bool enabled = true;
  double ms[N] = {};
  std::vector<std::unique_ptr<Event>> ev;  // start, stop, start, stop, ...
  std::vector<int> ev_phase;               // the phase at a start, -1 at a stop

  struct Span {
    PhaseSpans &p;
    hipStream_t s;
    void stop() { p.mark(-1, s); }
  };
  // records the start; the caller records the end with stop()
  Span span(int phase, hipStream_t s) {
    mark(phase, s);
    return Span{*this, s};
  }
  void mark(int phase, hipStream_t s) {
    if (!enabled) return;
    ev.emplace_back(new Event());
    ev_phase.push_back(phase);
    IRS_HIP(hipEventRecord(ev.back()->e, s));
  }
  // (after a synchronisation)
  void fold() {
    for (size_t i = 0; i + 1 < ev.size(); i += 2) ms[ev_phase[i]] += elapsed_ms(*ev[i], *ev[i + 1]);
    clear();
  }
  void clear() {
    ev.clear();
    ev_phase.clear();
  }
};

}  // namespace irs
