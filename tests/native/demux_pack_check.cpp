// Stand-alone check of csrc/demux_pack.h, the host packer of chiron_demux_windows, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_demux_pack_cpu.py).  Every buffer is allocated at exactly the size the
// packer is told, so a write or read past it is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../chiron_amd/csrc/demux_pack.h"

using namespace chiron;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33);
}

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("demux_pack_check: line %d: %s\n", __LINE__, #cond);    \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main() {
  // patterns of every length 1..64, codes 0..4: the masks are disjoint, hold exactly the bases 0..3 and nothing at or above len
  for (int len = 1; len <= 64; ++len) {
    for (int rep = 0; rep < 8; ++rep) {
      std::vector<uint8_t> codes((size_t)len);
      for (auto& c : codes) c = (uint8_t)(next_u32() % 5);
      const DemuxPattern p = demux_pack_pattern(codes.data(), len, rep);
      CHECK(p.len == len && p.group == rep);
      uint64_t all = 0;
      for (int c = 0; c < 4; ++c) {
        CHECK((all & p.mask[c]) == 0);
        all |= p.mask[c];
      }
      for (int i = 0; i < 64; ++i) {
        const bool set = (all >> i) & 1;
        CHECK(set == (i < len && codes[(size_t)i] < 4));
        if (set) CHECK((p.mask[codes[(size_t)i]] >> i) & 1);
      }
    }
  }
  // the top bit of a 64-base pattern
  {
    std::vector<uint8_t> codes(64, 2);
    const DemuxPattern p = demux_pack_pattern(codes.data(), 64, 0);
    CHECK(p.mask[2] == ~(uint64_t)0 && p.mask[0] == 0 && p.mask[1] == 0 && p.mask[3] == 0);
  }
  // windows of 0, 1, 7, 8, 9, 150, 4096 and random lengths, read from an offset array that does not start at 0
  const int64_t fixed[] = {0, 1, 7, 8, 9, 0, 150, 4096, 0};
  std::vector<int64_t> lens(fixed, fixed + sizeof(fixed) / sizeof(fixed[0]));
  for (int k = 0; k < 200; ++k) lens.push_back((int64_t)(next_u32() % 41));
  const int64_t windows = (int64_t)lens.size();
  std::vector<int64_t> off((size_t)windows + 1);
  off[0] = 5;
  for (int64_t w = 0; w < windows; ++w) off[(size_t)w + 1] = off[(size_t)w] + lens[(size_t)w];
  std::vector<uint8_t> codes((size_t)off[(size_t)windows]);
  for (auto& c : codes) c = (uint8_t)(next_u32() % 5);
  const int64_t bytes = demux_packed_bytes(off.data(), windows);
  CHECK(bytes % 8 == 0 && bytes <= (off[(size_t)windows] - off[0]) + 7 * windows);
  std::vector<DemuxWindow> recs((size_t)windows);
  uint8_t* packed = (uint8_t*)malloc((size_t)bytes);   // exactly: no slack for an overrun to hide in
  CHECK(packed != nullptr);
  demux_pack_windows(codes.data(), off.data(), windows, recs.data(), packed);
  int64_t at = 0;
  for (int64_t w = 0; w < windows; ++w) {
    const DemuxWindow& r = recs[(size_t)w];
    CHECK(r.start == at && r.start % 8 == 0 && r.m == lens[(size_t)w] && r.reserved == 0);
    for (int64_t i = 0; i < r.m; ++i) CHECK(packed[r.start + i] == codes[(size_t)(off[(size_t)w] + i)]);
    for (int64_t i = r.m; i < demux_padded(r.m); ++i) CHECK(packed[r.start + i] == DEMUX_PAD);
    at += demux_padded(r.m);
  }
  CHECK(at == bytes);
  free(packed);
  // no windows: nothing is touched
  demux_pack_windows(nullptr, off.data(), 0, nullptr, nullptr);
  CHECK(demux_packed_bytes(off.data(), 0) == 0);
  printf("demux pack OK\n");
  return 0;
}
