// Stand-alone check of csrc/refine_pack.h, the host walk of chiron_signal_refine, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_refine_cpu.py).  Every buffer is allocated at exactly the size the walk
// is told, so a read or write past it is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../chiron_amd/csrc/refine_pack.h"

using namespace chiron;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33);
}

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("refine_pack_check: line %d: %s\n", __LINE__, #cond);    \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  // items of 0, 1, 63, 64, 65, 257 and random numbers of bases, spans of 0 .. 11 samples and one of 5000, behind a head nobody owns
  const int64_t fixed[] = {0, 1, 63, 64, 65, 257, 0};
  std::vector<int64_t> lens(fixed, fixed + sizeof(fixed) / sizeof(fixed[0]));
  for (int k = 0; k < 100; ++k) lens.push_back((int64_t)(next_u32() % 41));
  for (size_t r = 0; r < lens.size(); ++r) {
    const int64_t L = lens[r];
    int32_t* start = (int32_t*)malloc((size_t)(L + 1) * sizeof(int32_t));   // exactly: no slack for an overrun to hide in
    int32_t* level = L > 0 ? (int32_t*)malloc((size_t)L * sizeof(int32_t)) : nullptr;
    CHECK(start && (level || L == 0));
    start[0] = (int32_t)(next_u32() % 5);
    for (int64_t n = 0; n < L; ++n) {
      const int32_t span = (r == 5 && n == 100) ? 5000 : (int32_t)(next_u32() % 12);
      start[n + 1] = start[n] + span;
      level[n] = n % 7 == 0 ? (n % 2 ? 32767 : -32767) : (int32_t)(next_u32() % 65535) - 32767;   // the two ends are legal
    }
    const int64_t S = start[L] + (int64_t)(next_u32() % 3);
    RefineFinding f = refine_check_item(start, level, L, S);
    CHECK(f.fault == REFINE_FINE);
    if (L > 0) {   // one fault of each kind, at the last place it can sit: found there, and nothing past the arrays is touched
      const int64_t at = L - 1;
      const int32_t keep_level = level[at], keep_start = start[L];
      level[at] = 32768;
      f = refine_check_item(start, level, L, S);
      CHECK(f.fault == REFINE_LEVEL_RANGE && f.at == at && f.value == 32768);
      level[at] = -32768;
      f = refine_check_item(start, level, L, S);
      CHECK(f.fault == REFINE_LEVEL_RANGE && f.at == at && f.value == -32768);
      level[at] = INT32_MIN;
      CHECK(refine_check_item(start, level, L, S).fault == REFINE_LEVEL_RANGE);
      level[at] = keep_level;
      start[L] = (int32_t)S + 1;
      f = refine_check_item(start, level, L, S);
      CHECK(f.fault == REFINE_START_RANGE && f.at == L && f.value == S + 1);
      if (start[L - 1] > 0) {
        start[L] = start[L - 1] - 1;
        f = refine_check_item(start, level, L, S);
        CHECK(f.fault == REFINE_START_ORDER && f.at == L && f.value == start[L - 1] - 1);
      }
      start[L] = keep_start;
      CHECK(refine_check_item(start, level, L, S).fault == REFINE_FINE);
      // a fault at the first base is reported before anything behind it is looked at
      level[0] = 40000;
      start[L] = -7;
      f = refine_check_item(start, level, L, S);
      CHECK(L == 1 ? (f.fault == REFINE_START_RANGE && f.at == 1) : (f.fault == REFINE_LEVEL_RANGE && f.at == 0 && f.value == 40000));
    }
    start[0] = -1;
    f = refine_check_item(start, level, L, S);
    CHECK(f.fault == REFINE_START_RANGE && f.at == 0 && f.value == -1);
    start[0] = (int32_t)S + 1;
    CHECK(refine_check_item(start, level, L, S).fault == REFINE_START_RANGE);
    free(start);
    free(level);
  }
  // a call without any base: every item keeps its one entry
  for (int64_t items = 0; items < 70; items += 23) {
    int32_t* in = (int32_t*)malloc((size_t)(items > 0 ? items : 1) * sizeof(int32_t));
    int32_t* out = (int32_t*)malloc((size_t)(items > 0 ? items : 1) * sizeof(int32_t));
    int64_t* cost = (int64_t*)malloc((size_t)(items > 0 ? items : 1) * sizeof(int64_t));
    CHECK(in && out && cost);
    for (int64_t i = 0; i < items; ++i) {
      in[i] = (int32_t)(next_u32() % 1000);
      out[i] = -1;
      cost[i] = -1;
    }
    refine_without_bases(in, items, out, cost);
    for (int64_t i = 0; i < items; ++i) CHECK(out[i] == in[i] && cost[i] == 0);
    free(in);
    free(out);
    free(cost);
  }
  printf("refine pack OK\n");
  return 0;
}
