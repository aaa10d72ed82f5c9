// What `locate --events` does on the host, as plain C++ without HIP: the event detector of chiron_signal_events (the definition is in
// include/chiron_amd.h and is restated in plain Python by tests/event_ref.py), and the caps chiron_event_locate holds its queries to.
// The offsets and the levels of the reference are walked by locate_pack.h.  Host-only and free of the library's state, so that
// tests/native/event_pack_check.cpp can run it under a sanitizer.
#pragma once
#include <stdint.h>

#include <vector>

#include "locate_pack.h"

namespace chiron {

constexpr int64_t EVENT_MAX_SAMPLES = 1 << 17;       // CHIRON_EVENT_MAX_SAMPLES: samples of one item of the detector
constexpr int32_t EVENT_MAX_WINDOW = 16;             // CHIRON_EVENT_MAX_WINDOW
constexpr int32_t EVENT_MAX_RADIUS = 16;             // CHIRON_EVENT_MAX_RADIUS
constexpr int64_t EVENT_MAX_THRESHOLD = 1ll << 52;   // CHIRON_EVENT_MAX_THRESHOLD
constexpr int64_t EVENT_MAX_QUERY = 8192;            // CHIRON_EVENT_MAX_QUERY: events of one query of the DP
constexpr int32_t EVENT_MAX_PENALTY = 65534;         // CHIRON_EVENT_MAX_PENALTY
constexpr int64_t EVENT_CHUNK = 64;                  // CHIRON_EVENT_CHUNK: rows a launch
static_assert(EVENT_MAX_QUERY * (65535 + EVENT_MAX_PENALTY) < (1ll << 30), "every real cost is below 2^30: the DP is 32-bit");
static_assert((int64_t)EVENT_MAX_WINDOW * (EVENT_MAX_WINDOW * 65535ll) * (EVENT_MAX_WINDOW * 65535ll) * 256 < (1ll << 52), "T's numerator is below 2^52");

static_assert(EVENT_CHUNK == LOCATE_CHUNK, "locate_launches plans both calls");

// floor((2 s + c) / (2 c)), c > 0: the mean with halves up, as chiron_signal_levels rounds
inline int64_t event_level(int64_t s, int64_t c) {
  const int64_t a = 2 * s + c, b = 2 * c;
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}

// T[0 .. n] of one item: resizes t to n + 1.  x has exactly n samples, 2 <= w.
inline void event_statistic(const int16_t* x, int64_t n, int32_t w, std::vector<int64_t>& t) {
  t.assign((size_t)n + 1, 0);
  if (n < 2 * (int64_t)w) return;
  int64_t s1 = 0, q1 = 0, s2 = 0, q2 = 0;             // the windows x[i-w .. i) and x[i .. i+w), from i = w on
  for (int32_t k = 0; k < w; ++k) {
    const int64_t a = x[k], b = x[w + k];
    s1 += a, q1 += a * a, s2 += b, q2 += b * b;
  }
  for (int64_t i = w;; ++i) {
    const int64_t d = s1 - s2;
    const int64_t v = (w * q1 - s1 * s1) + (w * q2 - s2 * s2);
    t[(size_t)i] = (w * d * d * 256) / (v > 1 ? v : 1);
    if (i == n - w) break;
    const int64_t out = x[i - w], mid = x[i], in = x[i + w];   // i + w <= n - 1 here
    s1 += mid - out, q1 += mid * mid - out * out;
    s2 += in - mid, q2 += in * in - mid * mid;
  }
}

// One item: its borders (count + 1 of them, border[0] = 0) and levels (count) into arrays that hold n + 1 and n entries; at most
// max_events events, the first ones.  -> the count; *truncated says whether an event was dropped.  t is scratch.
inline int32_t event_segment(const int16_t* x, int64_t n, int32_t w, int32_t r, int64_t thr, int32_t max_events, int32_t* border, int16_t* level,
                             bool* truncated, std::vector<int64_t>& t) {
  event_statistic(x, n, w, t);
  int32_t count = 0;
  int64_t from = 0;
  *truncated = false;
  border[0] = 0;
  for (int64_t i = 1; i <= n; ++i) {
    bool is_border = i == n;
    if (!is_border && t[(size_t)i] >= thr) {
      is_border = true;
      const int64_t lo = i - r > 0 ? i - r : 0, hi = i + r < n ? i + r : n;
      for (int64_t j = lo; j <= hi && is_border; ++j)
        if (j < i ? t[(size_t)j] >= t[(size_t)i] : t[(size_t)j] > t[(size_t)i]) is_border = false;   // the first index of the maximum
    }
    if (!is_border) continue;
    if (count == max_events) {
      *truncated = true;
      break;
    }
    int64_t s = 0;
    for (int64_t j = from; j < i; ++j) s += x[j];
    level[count] = (int16_t)event_level(s, i - from);   // a mean of int16 values with halves up: inside int16
    border[++count] = (int32_t)i;
    from = i;
  }
  return count;
}

}  // namespace chiron
