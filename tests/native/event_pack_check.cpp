// Stand-alone check of csrc/event_pack.h, the host side of chiron_signal_events and chiron_event_locate, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_event_cpu.py).  Every buffer is allocated at exactly the size the code
// is told, so a read or write past it is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../chiron_amd/csrc/event_pack.h"

using namespace chiron;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33);
}

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("event_pack_check: line %d: %s\n", __LINE__, #cond);    \
      return 1;                                                      \
    }                                                                \
  } while (0)

// T[i] with the windows' sums taken anew
static int64_t statistic_at(const int16_t* x, int64_t n, int32_t w, int64_t i) {
  if (i < w || i > n - w) return 0;
  int64_t s1 = 0, q1 = 0, s2 = 0, q2 = 0;
  for (int32_t k = 0; k < w; ++k) {
    const int64_t a = x[i - w + k], b = x[i + k];
    s1 += a, q1 += a * a, s2 += b, q2 += b * b;
  }
  const int64_t d = s1 - s2, v = (w * q1 - s1 * s1) + (w * q2 - s2 * s2);
  return (w * d * d * 256) / (v > 1 ? v : 1);
}

int main() {
  // the offsets: random numbers of items of 1 .. limit entries, from a first offset above 0; one fault of each kind at the last item
  const int64_t limits[] = {EVENT_MAX_QUERY, EVENT_MAX_SAMPLES};
  for (int r = 0; r < 60; ++r) {
    const int64_t limit = limits[r % 2];
    const int64_t items = r < 4 ? r : (int64_t)(next_u32() % 41);
    int64_t* off = (int64_t*)malloc((size_t)(items + 1) * sizeof(int64_t));   // exactly: no slack for an overrun to hide in
    CHECK(off);
    off[0] = (int64_t)(next_u32() % 5);
    int64_t want_longest = 0;
    for (int64_t i = 0; i < items; ++i) {
      int64_t q = 1 + (int64_t)(next_u32() % 3000);
      if (i == items - 1 && r % 3 == 1) q = limit;   // the cap itself is legal
      off[i + 1] = off[i] + q;
      if (q > want_longest) want_longest = q;
    }
    int64_t longest = -1;
    LocateFinding f = locate_check_offsets(off, items, limit, &longest);
    CHECK(f.fault == LOCATE_FINE && longest == want_longest);
    CHECK(locate_launches(longest) == (longest + 63) / 64);
    if (items > 0) {
      const int64_t keep = off[items];
      off[items] = off[items - 1];
      f = locate_check_offsets(off, items, limit, &longest);
      CHECK(f.fault == LOCATE_QUERY_EMPTY && f.at == items - 1);
      off[items] = off[items - 1] - 1;
      f = locate_check_offsets(off, items, limit, &longest);
      CHECK(f.fault == LOCATE_OFF_ORDER && f.at == items && f.value == off[items - 1] - 1);
      off[items] = off[items - 1] + limit + 1;
      f = locate_check_offsets(off, items, limit, &longest);
      CHECK(f.fault == LOCATE_QUERY_LONG && f.at == items - 1 && f.value == limit + 1);
      off[items] = INT64_MAX;   // the difference stays inside int64: both offsets are at or above 0
      f = locate_check_offsets(off, items, limit, &longest);
      CHECK(f.fault == LOCATE_QUERY_LONG && f.at == items - 1);
      off[items] = keep;
      CHECK(locate_check_offsets(off, items, limit, &longest).fault == LOCATE_FINE);
    }
    const int64_t keep0 = off[0];
    off[0] = -1;
    f = locate_check_offsets(off, items, limit, &longest);
    CHECK(f.fault == LOCATE_OFF_NEGATIVE && f.at == 0 && f.value == -1);
    off[0] = INT64_MIN;
    CHECK(locate_check_offsets(off, items, limit, &longest).fault == LOCATE_OFF_NEGATIVE);
    off[0] = keep0;
    free(off);
  }
  CHECK(locate_launches(1) == 1 && locate_launches(64) == 1 && locate_launches(65) == 2 && locate_launches(EVENT_MAX_QUERY) == 128);
  CHECK(event_level(7, 2) == 4 && event_level(-7, 2) == -3 && event_level(-8, 2) == -4 && event_level(-1, 2) == 0 && event_level(-3, 2) == -1 &&
        event_level(0, 5) == 0 && event_level(32767 * 9ll, 9) == 32767 && event_level(-32768 * 9ll, 9) == -32768);

  // the detector: step signals with noise, constant signals, the extreme values, items shorter than two windows; every array at
  // exactly n, n + 1 and n entries
  std::vector<int64_t> t;
  const int64_t lens[] = {1, 2, 3, 4, 5, 6, 7, 31, 32, 33, 64, 200, 1000, 4097};
  for (size_t li = 0; li < sizeof(lens) / sizeof(lens[0]); ++li) {
    for (int kind = 0; kind < 4; ++kind) {
      const int64_t n = lens[li];
      const int32_t w = 2 + (int32_t)(next_u32() % 15), r = 1 + (int32_t)(next_u32() % 16);
      const int64_t thr = kind == 3 ? EVENT_MAX_THRESHOLD : 1 + (int64_t)(next_u32() % 2000);
      int16_t* x = (int16_t*)malloc((size_t)n * sizeof(int16_t));
      int32_t* border = (int32_t*)malloc((size_t)(n + 1) * sizeof(int32_t));
      int16_t* level = (int16_t*)malloc((size_t)n * sizeof(int16_t));
      CHECK(x && border && level);
      int32_t base = 0, left = 0;
      for (int64_t i = 0; i < n; ++i) {
        if (left == 0) {
          base = (int32_t)(next_u32() % 2001) - 1000;
          left = 1 + (int32_t)(next_u32() % 14);
        }
        --left;
        x[i] = kind == 0   ? (int16_t)(base + (int32_t)(next_u32() % 61) - 30)
               : kind == 1 ? (int16_t)7                                              // V = 0 throughout
               : kind == 2 ? (int16_t)((i / w) % 2 ? 32767 : -32768)                 // the largest d and the largest squares
                           : (int16_t)base;
      }
      const int32_t max_events = kind == 0 && li % 2 ? 3 : (int32_t)EVENT_MAX_SAMPLES;
      bool truncated = true;
      const int32_t count = event_segment(x, n, w, r, thr, max_events, border, level, &truncated, t);
      CHECK((int64_t)t.size() == n + 1);
      for (int64_t i = 0; i <= n; ++i) CHECK(t[(size_t)i] == statistic_at(x, n, w, i) && t[(size_t)i] >= 0 && t[(size_t)i] < (1ll << 52));
      CHECK(count >= 1 && count <= max_events && count <= n && border[0] == 0);
      CHECK(truncated || border[count] == n);
      if (kind == 1 || n < 2 * w) CHECK(count == 1 && border[1] == n && !truncated);
      for (int32_t k = 0; k < count; ++k) {
        CHECK(border[k] < border[k + 1] && border[k + 1] <= n);
        int64_t s = 0;
        for (int32_t i = border[k]; i < border[k + 1]; ++i) s += x[i];
        CHECK(level[k] == event_level(s, border[k + 1] - border[k]));
        if (k > 0) {   // an inner border: at or above the threshold, above what lies within r to its left, at or above what lies right
          const int64_t b = border[k];
          CHECK(t[(size_t)b] >= thr);
          for (int64_t j = b - r > 0 ? b - r : 0; j <= (b + r < n ? b + r : n); ++j) CHECK(j < b ? t[(size_t)j] < t[(size_t)b] : t[(size_t)j] <= t[(size_t)b]);
        }
      }
      free(x);
      free(border);
      free(level);
    }
  }
  printf("event pack OK\n");
  return 0;
}
