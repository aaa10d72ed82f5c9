// Stand-alone check of csrc/site_pack.h, the host walk of chiron_signal_score, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_modcall_cpu.py).  Every buffer is allocated at exactly the size the walk
// is told, so a read past it is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../chiron_amd/csrc/site_pack.h"

using namespace chiron;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33);
}

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      printf("site_pack_check: line %d: %s\n", __LINE__, #cond);    \
      return 1;                                                     \
    }                                                               \
  } while (0)

int main() {
  const int64_t fixed[] = {0, 1, 2, 63, 64, 65, 257};
  std::vector<int64_t> counts(fixed, fixed + sizeof(fixed) / sizeof(fixed[0]));
  for (int k = 0; k < 60; ++k) counts.push_back((int64_t)(next_u32() % 41));

  // segments: 0, 1, 2, 63, 64, 65, 257 and random numbers of them, of 0 .. 4096 samples, from a first offset above 0
  for (size_t r = 0; r < counts.size(); ++r) {
    const int64_t segments = counts[r];
    int64_t* off = (int64_t*)malloc((size_t)(segments + 1) * sizeof(int64_t));   // exactly: no slack for an overrun to hide in
    CHECK(off);
    off[0] = (int64_t)(next_u32() % 5);
    for (int64_t g = 0; g < segments; ++g) {
      int64_t s = (int64_t)(next_u32() % 300);
      if (g == segments - 1 && r % 2) s = SITE_MAX_SAMPLES;   // the cap itself is legal
      if (g == 0 && r % 3 == 0) s = 0;                        // and so is an empty segment
      off[g + 1] = off[g] + s;
    }
    CHECK(site_check_segments(off, segments).fault == SITE_FINE);
    if (segments > 0) {   // one fault of each kind at the last segment: found there, and nothing past the array is touched
      const int64_t keep = off[segments];
      off[segments] = off[segments - 1] - 1;
      SiteFinding f = site_check_segments(off, segments);
      CHECK(f.fault == SITE_OFF_ORDER && f.at == segments && f.value == off[segments - 1] - 1);
      off[segments] = off[segments - 1] + SITE_MAX_SAMPLES + 1;
      f = site_check_segments(off, segments);
      CHECK(f.fault == SITE_SEGMENT_LONG && f.at == segments - 1 && f.value == SITE_MAX_SAMPLES + 1);
      off[segments] = INT64_MAX;   // the difference stays inside int64: both offsets are at or above 0
      f = site_check_segments(off, segments);
      CHECK(f.fault == SITE_SEGMENT_LONG && f.at == segments - 1);
      off[segments] = keep;
      CHECK(site_check_segments(off, segments).fault == SITE_FINE);
    }
    const int64_t keep0 = off[0];
    off[0] = -1;
    SiteFinding f = site_check_segments(off, segments);
    CHECK(f.fault == SITE_OFF_NEGATIVE && f.at == 0 && f.value == -1);   // reported before anything behind it is looked at
    off[0] = INT64_MIN;
    CHECK(site_check_segments(off, segments).fault == SITE_OFF_NEGATIVE);
    off[0] = keep0;
    free(off);
  }

  // candidates: the same numbers of them, of 1 .. 16 levels, on `segments` segments, the levels from a first offset above 0
  for (size_t r = 0; r < counts.size(); ++r) {
    const int64_t candidates = counts[r], segments = 1 + (int64_t)(next_u32() % 9);
    int64_t* off = (int64_t*)malloc((size_t)(candidates + 1) * sizeof(int64_t));
    int32_t* seg = candidates > 0 ? (int32_t*)malloc((size_t)candidates * sizeof(int32_t)) : nullptr;
    CHECK(off && (seg || candidates == 0));
    off[0] = (int64_t)(next_u32() % 5);
    for (int64_t c = 0; c < candidates; ++c) {
      int64_t n = 1 + (int64_t)(next_u32() % SITE_MAX_COLUMNS);
      if (c == candidates - 1) n = r % 2 ? SITE_MAX_COLUMNS : 1;   // both ends of the range are legal
      off[c + 1] = off[c] + n;
      seg[c] = (int32_t)(next_u32() % segments);
      if (c == candidates - 1) seg[c] = r % 2 ? (int32_t)(segments - 1) : 0;
    }
    const int64_t total = off[candidates];   // level is indexed from 0: the entries below off[0] belong to nobody and are never read
    int32_t* level = total > 0 ? (int32_t*)malloc((size_t)total * sizeof(int32_t)) : nullptr;
    CHECK(level || total == 0);
    for (int64_t j = 0; j < total; ++j) level[j] = j < off[0] ? INT32_MIN : (j % 7 == 0 ? (j % 2 ? 32767 : -32767) : (int32_t)(next_u32() % 65535) - 32767);
    CHECK(site_check_candidates(off, seg, level, candidates, segments).fault == SITE_FINE);
    if (candidates > 0) {   // one fault of each kind at the last candidate, the level faults at its last level
      const int64_t last = candidates - 1, keep = off[candidates];
      SiteFinding f;
      off[candidates] = off[last] - 1;
      f = site_check_candidates(off, seg, level, candidates, segments);
      CHECK(f.fault == SITE_OFF_ORDER && f.at == candidates && f.value == off[last] - 1);
      off[candidates] = off[last];
      f = site_check_candidates(off, seg, level, candidates, segments);
      CHECK(f.fault == SITE_COLUMNS && f.at == last && f.value == 0);
      off[candidates] = off[last] + SITE_MAX_COLUMNS + 1;   // refused before any of its levels is read: they would lie past the array
      f = site_check_candidates(off, seg, level, candidates, segments);
      CHECK(f.fault == SITE_COLUMNS && f.at == last && f.value == SITE_MAX_COLUMNS + 1);
      off[candidates] = INT64_MAX;
      CHECK(site_check_candidates(off, seg, level, candidates, segments).fault == SITE_COLUMNS);
      off[candidates] = keep;
      const int32_t keep_seg = seg[last];
      const int32_t bad_seg[] = {-1, (int32_t)segments, INT32_MIN, INT32_MAX};
      for (int k = 0; k < 4; ++k) {
        seg[last] = bad_seg[k];
        f = site_check_candidates(off, seg, level, candidates, segments);
        CHECK(f.fault == SITE_SEGMENT_INDEX && f.at == last && f.value == bad_seg[k]);
      }
      seg[last] = keep_seg;
      f = site_check_candidates(off, seg, level, candidates, 0);   // a call without any segment: the first candidate names none
      CHECK(f.fault == SITE_SEGMENT_INDEX && f.at == 0);
      const int32_t keep_level = level[total - 1];
      const int32_t bad[] = {32768, -32768, INT32_MIN, INT32_MAX};
      for (int k = 0; k < 4; ++k) {
        level[total - 1] = bad[k];
        f = site_check_candidates(off, seg, level, candidates, segments);
        CHECK(f.fault == SITE_LEVEL_RANGE && f.at == last && f.column == total - off[last] - 1 && f.value == bad[k]);
      }
      level[total - 1] = keep_level;
      CHECK(site_check_candidates(off, seg, level, candidates, segments).fault == SITE_FINE);
    }
    const int64_t keep0 = off[0];
    off[0] = -3;
    SiteFinding f = site_check_candidates(off, seg, level, candidates, segments);
    CHECK(f.fault == SITE_OFF_NEGATIVE && f.at == 0 && f.value == -3);   // reported before anything behind it is looked at
    off[0] = keep0;
    free(level);
    free(seg);
    free(off);
  }
  CHECK(site_batches(0) == 0 && site_batches(1) == 1 && site_batches(64) == 1 && site_batches(65) == 2 && site_batches(0x7FFFFFFF) == 1 << 25);
  printf("site pack OK\n");
  return 0;
}
