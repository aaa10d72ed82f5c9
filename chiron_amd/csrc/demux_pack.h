// What demux.hip's host side lays out before it copies anything, as plain C++ without HIP: the per-pattern record of the bit-vector
// automaton and the windows' codes on 8-byte boundaries.  Host-only and free of the library's state, so that
// tests/native/demux_pack_check.cpp can run it under a sanitizer.  The callers have checked every offset and code.
#pragma once
#include <stdint.h>
#include <string.h>

namespace chiron {

// One pattern as the kernel reads it.  Bit i of mask[c] is set when base i of the pattern is c, c = 0..3; a code 4 sets no bit, so
// it matches nothing.  Bits at and above len are 0.
struct DemuxPattern {
  uint64_t mask[4];
  int32_t len;
  int32_t group;
};
static_assert(sizeof(DemuxPattern) == 40, "the header states 40 bytes a pattern");

// One window: its codes are win[start .. start + m) of the packed array, start a multiple of 8.
struct DemuxWindow {
  int64_t start;
  int32_t m;
  int32_t reserved;
};
static_assert(sizeof(DemuxWindow) == 16, "the header states 16 bytes of record a window");

constexpr uint8_t DEMUX_PAD = 0xFF;   // what fills a window up to its 8-byte boundary: a code that matches nothing

inline DemuxPattern demux_pack_pattern(const uint8_t* codes, int32_t len, int32_t group) {
  DemuxPattern p;
  memset(&p, 0, sizeof(p));
  p.len = len;
  p.group = group;
  for (int32_t i = 0; i < len; ++i)
    if (codes[i] < 4) p.mask[codes[i]] |= (uint64_t)1 << i;
  return p;
}

inline int64_t demux_padded(int64_t m) { return (m + 7) & ~(int64_t)7; }

// The bytes demux_pack_windows writes for these offsets.
inline int64_t demux_packed_bytes(const int64_t* win_off, int64_t windows) {
  int64_t at = 0;
  for (int64_t w = 0; w < windows; ++w) at += demux_padded(win_off[w + 1] - win_off[w]);
  return at;
}

// Fills recs[0 .. windows) and packed[0 .. demux_packed_bytes).
inline void demux_pack_windows(const uint8_t* codes, const int64_t* win_off, int64_t windows, DemuxWindow* recs, uint8_t* packed) {
  int64_t at = 0;
  for (int64_t w = 0; w < windows; ++w) {
    const int64_t m = win_off[w + 1] - win_off[w], room = demux_padded(m);
    recs[w].start = at;
    recs[w].m = (int32_t)m;
    recs[w].reserved = 0;
    if (m > 0) memcpy(packed + at, codes + win_off[w], (size_t)m);
    if (room > m) memset(packed + at + m, DEMUX_PAD, (size_t)(room - m));
    at += room;
  }
}

}  // namespace chiron
