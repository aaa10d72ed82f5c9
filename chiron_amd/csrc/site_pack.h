// What site_score.hip's host side does before it copies anything, as plain C++ without HIP: the walk over the segments' offsets and
// the walk over the candidates -- their offsets, their segment indices and their levels -- that check them.  Host-only and free of
// the library's state, so that tests/native/site_pack_check.cpp can run it under a sanitizer.
#pragma once
#include <stdint.h>

namespace chiron {

constexpr int32_t SITE_LEVEL_MAX = 32767;            // |level|: with int16 samples |x - e| <= 65535
constexpr int64_t SITE_MAX_SAMPLES = 4096;           // CHIRON_SITE_MAX_SAMPLES
constexpr int64_t SITE_MAX_COLUMNS = 16;             // CHIRON_SITE_MAX_COLUMNS
constexpr int32_t SITE_INFEASIBLE = INT32_MAX;       // CHIRON_SITE_INFEASIBLE
static_assert(SITE_MAX_SAMPLES * 65535 < (1ll << 30), "every real cost is below 2^30: the DP is 32-bit and 2^30 stands for no path");

enum SiteFault {
  SITE_FINE = 0,
  SITE_OFF_NEGATIVE = 1,     // sample_off[0] or level_off[0] below 0
  SITE_OFF_ORDER = 2,        // an offset below its predecessor
  SITE_SEGMENT_LONG = 3,     // a segment above SITE_MAX_SAMPLES
  SITE_COLUMNS = 4,          // a candidate with 0 or more than SITE_MAX_COLUMNS levels
  SITE_SEGMENT_INDEX = 5,    // seg[c] outside 0 .. segments - 1
  SITE_LEVEL_RANGE = 6       // a level outside -32767 .. 32767
};

// What a walk found wrong: `at` is the index into the offsets (OFF_*), the segment (SEGMENT_LONG) or the candidate (COLUMNS,
// SEGMENT_INDEX, LEVEL_RANGE), `column` the level's index inside its candidate (LEVEL_RANGE), value what is held there (the length
// for SEGMENT_LONG and COLUMNS).
struct SiteFinding {
  SiteFault fault;
  int64_t at;
  int64_t column;
  int64_t value;
};

// sample_off[0 .. segments]: starts at or above 0, never decreases, no segment above SITE_MAX_SAMPLES; an empty segment is legal.
// Stops at the first fault.  Reads nothing past sample_off[segments].
inline SiteFinding site_check_segments(const int64_t* sample_off, int64_t segments) {
  if (sample_off[0] < 0) return {SITE_OFF_NEGATIVE, 0, 0, sample_off[0]};
  for (int64_t g = 0; g < segments; ++g) {
    // the difference of two int64 can leave int64 only when they differ in sign, and both are at or above 0 here
    if (sample_off[g + 1] < sample_off[g]) return {SITE_OFF_ORDER, g + 1, 0, sample_off[g + 1]};
    const int64_t s = sample_off[g + 1] - sample_off[g];
    if (s > SITE_MAX_SAMPLES) return {SITE_SEGMENT_LONG, g, 0, s};
  }
  return {SITE_FINE, 0, 0, 0};
}

// The candidates in their order: level_off[0 .. candidates] starts at or above 0 and never decreases, candidate c has 1 ..
// SITE_MAX_COLUMNS levels, seg[c] lies inside 0 .. segments - 1 and every one of its levels level[level_off[c] ..) inside -32767 ..
// 32767.  Stops at the first fault.  Reads nothing past level_off[candidates], seg[candidates - 1] and level[level_off[candidates] - 1].
inline SiteFinding site_check_candidates(const int64_t* level_off, const int32_t* seg, const int32_t* level, int64_t candidates, int64_t segments) {
  if (level_off[0] < 0) return {SITE_OFF_NEGATIVE, 0, 0, level_off[0]};
  for (int64_t c = 0; c < candidates; ++c) {
    if (level_off[c + 1] < level_off[c]) return {SITE_OFF_ORDER, c + 1, 0, level_off[c + 1]};
    const int64_t n = level_off[c + 1] - level_off[c];
    if (n < 1 || n > SITE_MAX_COLUMNS) return {SITE_COLUMNS, c, 0, n};
    if (seg[c] < 0 || seg[c] >= segments) return {SITE_SEGMENT_INDEX, c, 0, seg[c]};
    for (int64_t k = 0; k < n; ++k) {
      const int32_t e = level[level_off[c] + k];
      if (e < -SITE_LEVEL_MAX || e > SITE_LEVEL_MAX) return {SITE_LEVEL_RANGE, c, k, e};
    }
  }
  return {SITE_FINE, 0, 0, 0};
}

// launches' units: batches of 64 candidates, a lane each
constexpr int64_t site_batches(int64_t candidates) { return (candidates + 63) / 64; }

}  // namespace chiron
