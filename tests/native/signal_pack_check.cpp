// Stand-alone check of csrc/signal_pack.h, the host walk of chiron_signal_levels, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_signal_pack_cpu.py).  Every buffer is allocated at exactly the size the
// packer is told, so a write or read past it is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../chiron_amd/csrc/signal_pack.h"

using namespace chiron;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33);
}

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("signal_pack_check: line %d: %s\n", __LINE__, #cond);    \
      return 1;                                                       \
    }                                                                 \
  } while (0)

// floor((2 s + c) / (2 c)) without a division: the largest q with 2 c q <= 2 s + c
static int32_t level_by_search(int64_t s, int32_t c) {
  int64_t lo = -40000, hi = 40000;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (2 * (int64_t)c * mid <= 2 * s + c) lo = mid; else hi = mid - 1;
  }
  return (int32_t)lo;
}

int main() {
  // the rounding rule: halves up, floor division at negative sums, one sample, the lowest value, the largest count
  CHECK(signal_level(-3, 2) == -1 && signal_level(3, 2) == 2 && signal_level(-1, 1) == -1 && signal_level(-7, 2) == -3);
  CHECK(signal_level(-32768, 1) == -32768 && signal_level(3 * -32768ll, 3) == -32768 && signal_level(-65535, 2) == -32767);
  CHECK(signal_level(-1, 2) == 0 && signal_level(1, 2) == 1 && signal_level(-16, 3) == -5 && signal_level(-17, 3) == -6 && signal_level(4, 3) == 1);
  CHECK(signal_level((int64_t)0x7FFFFFFF * 32767, 0x7FFFFFFF) == 32767 && signal_level((int64_t)0x7FFFFFFF * -32768, 0x7FFFFFFF) == -32768);
  for (int k = 0; k < 20000; ++k) {
    const int32_t c = 1 + (int32_t)(next_u32() % (k % 2 ? 12 : 6000));
    int64_t s = 0;
    for (int32_t i = 0; i < c; ++i) s += (int64_t)(next_u32() % 65536) - 32768;
    CHECK(signal_level(s, c) == level_by_search(s, c));
  }
  // reads of 0, 1, 63, 64, 65 and random numbers of bases, spans of 0 .. 11 samples and one of 5000, behind a head nobody owns
  const int64_t fixed[] = {0, 1, 63, 64, 65, 257, 0};
  std::vector<int64_t> lens(fixed, fixed + sizeof(fixed) / sizeof(fixed[0]));
  for (int k = 0; k < 100; ++k) lens.push_back((int64_t)(next_u32() % 41));
  const int64_t bins = 7;
  int64_t sample_first = 11;
  for (size_t r = 0; r < lens.size(); ++r) {
    const int64_t L = lens[r];
    int32_t* start = (int32_t*)malloc((size_t)(L + 1) * sizeof(int32_t));   // exactly: no slack for an overrun to hide in
    int32_t* bin = (int32_t*)malloc((size_t)(L > 0 ? L : 1) * sizeof(int32_t));
    SignalBase* recs = (SignalBase*)malloc((size_t)(L > 0 ? L : 1) * sizeof(SignalBase));
    CHECK(start && bin && recs);
    start[0] = (int32_t)(next_u32() % 5);
    for (int64_t n = 0; n < L; ++n) {
      const int32_t span = (r == 5 && n == 100) ? 5000 : (int32_t)(next_u32() % 12);
      start[n + 1] = start[n] + span;
      bin[n] = (int32_t)(next_u32() % (bins + 1)) - 1;
    }
    const int64_t S = start[L] + (int64_t)(next_u32() % 3);
    SignalFinding f = signal_pack_read(start, L > 0 ? bin : nullptr, L, S, sample_first, bins, L > 0 ? recs : nullptr);
    CHECK(f.fault == SIGNAL_FINE);
    for (int64_t n = 0; n < L; ++n)
      CHECK(recs[n].first == sample_first + start[n] && recs[n].count == start[n + 1] - start[n] && recs[n].bin == bin[n]);
    if (L > 0) {   // one fault of each kind, at the last place it can sit: found there, and nothing past the arrays is touched
      const int64_t at = L - 1;
      const int32_t keep_bin = bin[at], keep_start = start[L];
      bin[at] = (int32_t)bins;
      f = signal_pack_read(start, bin, L, S, sample_first, bins, recs);
      CHECK(f.fault == SIGNAL_BIN_RANGE && f.at == at && f.value == bins);
      bin[at] = -2;
      f = signal_pack_read(start, bin, L, S, sample_first, bins, recs);
      CHECK(f.fault == SIGNAL_BIN_RANGE && f.at == at && f.value == -2);
      bin[at] = keep_bin;
      start[L] = (int32_t)S + 1;
      f = signal_pack_read(start, bin, L, S, sample_first, bins, recs);
      CHECK(f.fault == SIGNAL_START_RANGE && f.at == L && f.value == S + 1);
      if (start[L - 1] > 0) {
        start[L] = start[L - 1] - 1;
        f = signal_pack_read(start, bin, L, S, sample_first, bins, recs);
        CHECK(f.fault == SIGNAL_START_ORDER && f.at == L && f.value == start[L - 1] - 1);
      }
      start[L] = keep_start;
      CHECK(signal_pack_read(start, bin, L, S, sample_first, bins, recs).fault == SIGNAL_FINE);
    }
    start[0] = -1;
    f = signal_pack_read(start, bin, L, S, sample_first, bins, recs);
    CHECK(f.fault == SIGNAL_START_RANGE && f.at == 0 && f.value == -1);
    sample_first += S;
    free(start);
    free(bin);
    free(recs);
  }
  printf("signal pack OK\n");
  return 0;
}
