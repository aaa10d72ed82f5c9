// What signal.hip's host side lays out before it copies anything, as plain C++ without HIP: the walk over one read's base starts and
// bins that checks them and writes the flat per-base record the kernel reads.  Host-only and free of the library's state, so that
// tests/native/signal_pack_check.cpp can run it under a sanitizer.  The caller has checked the offsets of the reads.
#pragma once
#include <stdint.h>

namespace chiron {

// One base as the kernel reads it: its samples are first .. first + count) of the call's sample array (the samples of read 0 start
// at 0), count may be 0; bin is -1 or a plane index.
struct SignalBase {
  int64_t first;
  int32_t count;
  int32_t bin;
};
static_assert(sizeof(SignalBase) == 16, "the header states 16 bytes a base");

enum SignalFault { SIGNAL_FINE = 0, SIGNAL_START_RANGE = 1, SIGNAL_START_ORDER = 2, SIGNAL_BIN_RANGE = 3 };

// What signal_pack_read found wrong: `at` is the index into the read's start entries (START_*) or bases (BIN_RANGE), value what it
// holds there.
struct SignalFinding {
  SignalFault fault;
  int64_t at;
  int64_t value;
};

// One read of `bases` bases and `samples` samples whose first sample is sample `sample_first` of the call.  start: its bases + 1
// entries, relative to its first sample; bin: its `bases` entries.  Checks every start entry (inside 0 .. samples, never below its
// predecessor) and every bin (-1 .. bins - 1) and fills recs[0 .. bases).  Stops at the first fault: the records before it are
// written, nothing past recs[bases - 1] ever is.
inline SignalFinding signal_pack_read(const int32_t* start, const int32_t* bin, int64_t bases, int64_t samples, int64_t sample_first,
                                      int64_t bins, SignalBase* recs) {
  int64_t prev = start[0];
  if (prev < 0 || prev > samples) return {SIGNAL_START_RANGE, 0, prev};
  for (int64_t n = 0; n < bases; ++n) {
    const int64_t next = start[n + 1];
    if (next < 0 || next > samples) return {SIGNAL_START_RANGE, n + 1, next};
    if (next < prev) return {SIGNAL_START_ORDER, n + 1, next};
    const int64_t b = bin[n];
    if (b < -1 || b >= bins) return {SIGNAL_BIN_RANGE, n, b};
    recs[n].first = sample_first + prev;
    recs[n].count = (int32_t)(next - prev);
    recs[n].bin = (int32_t)b;
    prev = next;
  }
  return {SIGNAL_FINE, 0, 0};
}

// floor((2 s + c) / (2 c)), c > 0: the mean of c samples of sum s rounded to nearest, halves up.  Floor division, not C's
// truncation: s = -3, c = 2 gives -1.  Shared by the kernel and the stand-alone check.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int32_t signal_level(int64_t s, int32_t c) {
  const int64_t num = 2 * s + c, den = 2 * (int64_t)c;
  int64_t q = num / den;
  if (num % den < 0) --q;
  return (int32_t)q;
}

}  // namespace chiron
