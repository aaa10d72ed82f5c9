// Stand-alone check of csrc/locate_pack.h, the host walk of chiron_signal_locate, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_locate_cpu.py).  Every buffer is allocated at exactly the size the walk
// is told, so a read past it is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../chiron_amd/csrc/locate_pack.h"

using namespace chiron;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33);
}

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("locate_pack_check: line %d: %s\n", __LINE__, #cond);    \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  // offsets of 0, 1, 2, 63, 64, 65, 257 and random numbers of queries of 1 .. 16384 samples, from a first offset above 0
  const int64_t fixed[] = {0, 1, 2, 63, 64, 65, 257};
  std::vector<int64_t> counts(fixed, fixed + sizeof(fixed) / sizeof(fixed[0]));
  for (int k = 0; k < 60; ++k) counts.push_back((int64_t)(next_u32() % 41));
  for (size_t r = 0; r < counts.size(); ++r) {
    const int64_t items = counts[r];
    int64_t* off = (int64_t*)malloc((size_t)(items + 1) * sizeof(int64_t));   // exactly: no slack for an overrun to hide in
    CHECK(off);
    off[0] = (int64_t)(next_u32() % 5);
    int64_t want_longest = 0;
    for (int64_t i = 0; i < items; ++i) {
      int64_t q = 1 + (int64_t)(next_u32() % 3000);
      if (i == items - 1 && r % 2) q = LOCATE_MAX_QUERY;   // the cap itself is legal
      if (i == 0 && r % 3 == 0) q = 1;
      off[i + 1] = off[i] + q;
      if (q > want_longest) want_longest = q;
    }
    int64_t longest = -1;
    LocateFinding f = locate_check_offsets(off, items, LOCATE_MAX_QUERY, &longest);
    CHECK(f.fault == LOCATE_FINE && longest == want_longest);
    CHECK(locate_launches(longest) == (longest + 63) / 64);
    if (items > 0) {   // one fault of each kind at the last query: found there, and nothing past the array is touched
      const int64_t keep = off[items];
      off[items] = off[items - 1];
      f = locate_check_offsets(off, items, LOCATE_MAX_QUERY, &longest);
      CHECK(f.fault == LOCATE_QUERY_EMPTY && f.at == items - 1);
      off[items] = off[items - 1] - 1;
      f = locate_check_offsets(off, items, LOCATE_MAX_QUERY, &longest);
      CHECK(f.fault == LOCATE_OFF_ORDER && f.at == items && f.value == off[items - 1] - 1);
      off[items] = off[items - 1] + LOCATE_MAX_QUERY + 1;
      f = locate_check_offsets(off, items, LOCATE_MAX_QUERY, &longest);
      CHECK(f.fault == LOCATE_QUERY_LONG && f.at == items - 1 && f.value == LOCATE_MAX_QUERY + 1);
      off[items] = INT64_MAX;   // the difference stays inside int64: both offsets are at or above 0
      f = locate_check_offsets(off, items, LOCATE_MAX_QUERY, &longest);
      CHECK(f.fault == LOCATE_QUERY_LONG && f.at == items - 1);
      off[items] = keep;
      CHECK(locate_check_offsets(off, items, LOCATE_MAX_QUERY, &longest).fault == LOCATE_FINE);
    }
    const int64_t keep0 = off[0];
    off[0] = -1;
    f = locate_check_offsets(off, items, LOCATE_MAX_QUERY, &longest);
    CHECK(f.fault == LOCATE_OFF_NEGATIVE && f.at == 0 && f.value == -1);   // reported before anything behind it is looked at
    off[0] = INT64_MIN;
    CHECK(locate_check_offsets(off, items, LOCATE_MAX_QUERY, &longest).fault == LOCATE_OFF_NEGATIVE);
    off[0] = keep0;
    free(off);
  }
  // references of 0, 1, 1023, 1024, 1025, 2049 and random numbers of columns, breaks among them
  const int64_t lens[] = {0, 1, 1023, 1024, 1025, 2049, 7, 300};
  for (size_t r = 0; r < sizeof(lens) / sizeof(lens[0]); ++r) {
    const int64_t R = lens[r];
    int32_t* level = R > 0 ? (int32_t*)malloc((size_t)R * sizeof(int32_t)) : nullptr;
    CHECK(level || R == 0);
    for (int64_t j = 0; j < R; ++j)
      level[j] = j % 7 == 0 ? (j % 2 ? 32767 : -32767) : (j % 11 == 0 ? LOCATE_BREAK : (int32_t)(next_u32() % 65535) - 32767);   // the ends are legal
    CHECK(locate_check_levels(level, R).fault == LOCATE_FINE);
    CHECK(locate_blocks(R) == (R + 1023) / 1024);
    if (R > 0) {
      const int32_t keep = level[R - 1];
      const int32_t bad[] = {32768, -32768, INT32_MIN + 1, INT32_MAX};
      for (int k = 0; k < 4; ++k) {
        level[R - 1] = bad[k];
        LocateFinding f = locate_check_levels(level, R);
        CHECK(f.fault == LOCATE_LEVEL_RANGE && f.at == R - 1 && f.value == bad[k]);
      }
      level[R - 1] = LOCATE_BREAK;
      CHECK(locate_check_levels(level, R).fault == LOCATE_FINE);
      level[R - 1] = keep;
      level[0] = 40000;   // a fault at the first column is reported before anything behind it is looked at
      LocateFinding f = locate_check_levels(level, R);
      CHECK(f.fault == LOCATE_LEVEL_RANGE && f.at == 0 && f.value == 40000);
    }
    free(level);
  }
  CHECK(locate_blocks(0) == 0 && locate_blocks(1) == 1 && locate_blocks(1 << 28) == 1 << 18 && locate_launches(1) == 1 && locate_launches(16384) == 256);
  printf("locate pack OK\n");
  return 0;
}
