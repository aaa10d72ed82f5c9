// What locate.hip's host side does before it copies anything, as plain C++ without HIP: the walk over the queries' offsets and over
// the reference's levels that checks them, and the counts the launches are planned with.  Host-only and free of the library's
// state, so that tests/native/locate_pack_check.cpp can run it under a sanitizer.
#pragma once
#include <stdint.h>

namespace chiron {

constexpr int32_t LOCATE_LEVEL_MAX = 32767;          // |level| and |sample|: a row adds at most 65534
constexpr int32_t LOCATE_BREAK = INT32_MIN;          // CHIRON_LOCATE_BREAK: a column no path may use
constexpr int32_t LOCATE_NONE = INT32_MAX;           // CHIRON_LOCATE_NONE: a block without a path
constexpr int64_t LOCATE_MAX_QUERY = 16384;          // CHIRON_LOCATE_MAX_QUERY
constexpr int64_t LOCATE_BLOCK = 1024;               // CHIRON_LOCATE_BLOCK
constexpr int64_t LOCATE_CHUNK = 64;                 // CHIRON_LOCATE_CHUNK: rows a launch
static_assert(LOCATE_MAX_QUERY * 2 * LOCATE_LEVEL_MAX < (1ll << 30), "every real cost is below 2^30: the DP is 32-bit");

enum LocateFault { LOCATE_FINE = 0, LOCATE_OFF_NEGATIVE = 1, LOCATE_OFF_ORDER = 2, LOCATE_QUERY_EMPTY = 3, LOCATE_QUERY_LONG = 4, LOCATE_LEVEL_RANGE = 5 };

// What a walk found wrong: `at` is the index into the offsets (OFF_*), the item (QUERY_*) or the column (LEVEL_RANGE), value what
// it holds there (the query's length for QUERY_*).
struct LocateFinding {
  LocateFault fault;
  int64_t at;
  int64_t value;
};

// off[0 .. items]: starts at or above 0, never decreases, every item has 1 .. limit entries (LOCATE_MAX_QUERY samples; for
// event_pack.h's callers EVENT_MAX_QUERY events or EVENT_MAX_SAMPLES samples).  Stops at the first fault; *longest receives the
// longest item when there is none.  Reads nothing past off[items].
inline LocateFinding locate_check_offsets(const int64_t* off, int64_t items, int64_t limit, int64_t* longest) {
  if (off[0] < 0) return {LOCATE_OFF_NEGATIVE, 0, off[0]};
  int64_t most = 0;
  for (int64_t i = 0; i < items; ++i) {
    // the difference of two int64 can leave int64 only when they differ in sign, and both are at or above 0 here
    if (off[i + 1] < off[i]) return {LOCATE_OFF_ORDER, i + 1, off[i + 1]};
    const int64_t q = off[i + 1] - off[i];
    if (q == 0) return {LOCATE_QUERY_EMPTY, i, 0};
    if (q > limit) return {LOCATE_QUERY_LONG, i, q};
    if (q > most) most = q;
  }
  *longest = most;
  return {LOCATE_FINE, 0, 0};
}

// level[0 .. ref_len): inside -32767 .. 32767 or LOCATE_BREAK.  Stops at the first fault.
inline LocateFinding locate_check_levels(const int32_t* level, int64_t ref_len) {
  for (int64_t j = 0; j < ref_len; ++j) {
    const int32_t e = level[j];
    if (e != LOCATE_BREAK && (e < -LOCATE_LEVEL_MAX || e > LOCATE_LEVEL_MAX)) return {LOCATE_LEVEL_RANGE, j, e};
  }
  return {LOCATE_FINE, 0, 0};
}

// blocks of LOCATE_BLOCK columns that hold ref_len columns: the triples an item has in block_out
inline int64_t locate_blocks(int64_t ref_len) { return (ref_len + LOCATE_BLOCK - 1) / LOCATE_BLOCK; }

// launches a call needs: chunks of LOCATE_CHUNK rows of its longest query
inline int64_t locate_launches(int64_t longest) { return (longest + LOCATE_CHUNK - 1) / LOCATE_CHUNK; }

}  // namespace chiron
