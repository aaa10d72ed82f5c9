// What refine.hip's host side does before it copies anything, as plain C++ without HIP: the walk over one item's starts and levels
// that checks them, and the result of a call that needs no device.  Host-only and free of the library's state, so that
// tests/native/refine_pack_check.cpp can run it under a sanitizer.  The caller has checked the offsets of the items.
#pragma once
#include <stdint.h>

namespace chiron {

constexpr int32_t REFINE_LEVEL_MAX = 32767;   // |level|: with int16 samples |x - e| <= 65535, 64 of them sum below 2^23

enum RefineFault { REFINE_FINE = 0, REFINE_START_RANGE = 1, REFINE_START_ORDER = 2, REFINE_LEVEL_RANGE = 3 };

// What refine_check_item found wrong: `at` is the index into the item's start entries (START_*) or bases (LEVEL_RANGE), value what
// it holds there.
struct RefineFinding {
  RefineFault fault;
  int64_t at;
  int64_t value;
};

// One item of `bases` bases and `samples` samples.  start: its bases + 1 entries, relative to its first sample; level: its `bases`
// entries (not read when bases == 0).  Checks every start entry (inside 0 .. samples, never below its predecessor) and every level
// (-32767 .. 32767), in the order of the bases, and stops at the first fault.  Reads nothing past start[bases] and level[bases - 1].
inline RefineFinding refine_check_item(const int32_t* start, const int32_t* level, int64_t bases, int64_t samples) {
  int64_t prev = start[0];
  if (prev < 0 || prev > samples) return {REFINE_START_RANGE, 0, prev};
  for (int64_t n = 0; n < bases; ++n) {
    const int64_t next = start[n + 1];
    if (next < 0 || next > samples) return {REFINE_START_RANGE, n + 1, next};
    if (next < prev) return {REFINE_START_ORDER, n + 1, next};
    const int64_t e = level[n];
    if (e < -REFINE_LEVEL_MAX || e > REFINE_LEVEL_MAX) return {REFINE_LEVEL_RANGE, n, e};
    prev = next;
  }
  return {REFINE_FINE, 0, 0};
}

// A call whose items have no base at all: every item keeps its one start entry and costs nothing.  start_in and start_out hold
// `items` entries, cost_out `items`.
inline void refine_without_bases(const int32_t* start_in, int64_t items, int32_t* start_out, int64_t* cost_out) {
  for (int64_t i = 0; i < items; ++i) {
    start_out[i] = start_in[i];
    cost_out[i] = 0;
  }
}

}  // namespace chiron
