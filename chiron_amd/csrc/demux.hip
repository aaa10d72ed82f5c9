// Barcode and adapter search for `demux` on gfx950: very many short windows (read ends, about 150 bases), each against the same few
// patterns of at most 64 bases.  The definition is in include/chiron_amd.h and is restated in numpy by tests/demux_ref.py.
//
//   demux_kernel  The bit-parallel edit-distance automaton (Myers 1999 in Hyyro's form): a pattern's DP column is the two 64-bit
//                 words Pv / Mv of its vertical +1 / -1 differences, one window base advances the whole column in about fifteen
//                 64-bit integer operations (advance_block of bitvector.h, the step the edit distance of ctc_loss.hip chains over
//                 blocks), and the score of the column's last cell follows from the pattern's top bit.  The first row is free (a
//                 match may start anywhere in the window), so the horizontal input of every step is 0.  Exact at any distance: no
//                 band, no LDS row, no barrier (infix_kernel of map.hip has all three and one workgroup a pair).
//                 One pattern a lane.  With P2 the smallest power of two >= min(patterns, 64) a wavefront holds 64 / P2 window
//                 slots: lane l serves slot l / P2 and the patterns l % P2, l % P2 + P2, ...; 12 barcodes put four windows into a
//                 wave, 96 barcodes one window whose lanes run two patterns each, one after the other.  A wave runs to the longest
//                 window of its slots; shorter slots and lanes without a pattern step along and are masked where a result is kept.
//                 A slot's bases are one address for all its lanes, read eight at a time as one 64-bit word (the host puts every
//                 window on an 8-byte boundary); with one slot a wave (ONE_SLOT) the address is formed from readfirstlane values, so
//                 the compiler knows it to be wave-uniform.  A lane picks its match mask by four compares, not by an indexed array
//                 of registers, which the compiler would put into scratch (ctc_score.hip says the same of its classes).
//                 The per-window result is reduced over the slot's P2 lanes by __shfl_xor: the smallest (E, pattern) key and the
//                 smallest E of another group travel together.
//
// No atomics and nothing shared between windows: a window's outputs depend on that window and the patterns alone.  Every offset is
// 64-bit.  A pattern of exactly 64 bases relies on the wrap of the 64-bit add; every word of the automaton is uint64_t.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "bitvector.h"
#include "demux_pack.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_DEMUX_THREADS;
constexpr int WAVES = NT / 64;
constexpr int NO_KEY = 0x7FFFFFFF;   // the key of a lane without a pattern or a window: loses against every (E, q)
static_assert(CHIRON_DEMUX_MAX_PATTERN == 64, "a pattern column is one 64-bit word");
static_assert(CHIRON_DEMUX_MAX_PATTERNS <= (1 << 16) && CHIRON_DEMUX_MAX_PATTERN < (1 << 14), "key = E * 2^16 + q in 31 bits");

struct DemuxResult {
  int32_t best, dist, end, second;
};

struct DemuxParams {
  const DemuxPattern* pat;   // [patterns]
  const DemuxWindow* win;    // [windows]
  const uint8_t* codes;      // the windows, each on an 8-byte boundary
  DemuxResult* result;       // [windows]
  int16_t* pair_dist;        // [windows][patterns] or null
  int16_t* pair_end;
  int64_t windows;
  int32_t patterns;
  int32_t p2_shift;          // P2 = 1 << p2_shift lanes a window slot
};

struct DemuxLayout {
  size_t pat, win, codes, result, pair_dist, pair_end, bytes;
};

// What a lane, and then a slot, knows: the winner (key = E * 2^16 + q, its end, its group) and the smallest E of another group.
struct Summary {
  int key, end, group, other;
};

// Commutative: the smaller key wins, and keys of two patterns never tie.  The loser's side contributes its winner's E when that is
// of another group than the new winner (it is the smallest E of its side), else its own `other`.
__device__ __forceinline__ Summary merge(Summary a, Summary b) {
  const bool swap = b.key < a.key;
  const Summary w = swap ? b : a, l = swap ? a : b;
  const int from_loser = (l.key != NO_KEY && l.group != w.group) ? (l.key >> 16) : l.other;
  return {w.key, w.end, w.group, from_loser < w.other ? from_loser : w.other};
}

template <bool ONE_SLOT>
__global__ __launch_bounds__(CHIRON_DEMUX_THREADS) void demux_kernel(DemuxParams p) {
  const int lane = threadIdx.x & 63;
  const int shift = ONE_SLOT ? 6 : p.p2_shift;
  const int P2 = 1 << shift;
  const int slots = 64 >> shift;
  const int slot = lane >> shift, sub = lane & (P2 - 1);
  const int64_t wave = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  const int64_t slot_groups = (p.windows + slots - 1) >> (6 - shift);
  const int rounds = (p.patterns + P2 - 1) >> shift;
  for (int64_t g = wave; g < slot_groups; g += nwaves) {
    const int64_t w = g * slots + slot;
    const bool have = w < p.windows;
    int64_t start = 0;
    int m = 0;
    if (have) {
      const DemuxWindow rec = p.win[w];
      start = rec.start;
      m = rec.m;
    }
    int longest = m;
    if (ONE_SLOT) {   // w, and with it the record, is the same in every lane: say so
      m = longest = __builtin_amdgcn_readfirstlane(m);
      start = ((int64_t)__builtin_amdgcn_readfirstlane((int)(start >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
    } else {
      for (int o = 32; o >= 1; o >>= 1) {
        const int other = __shfl_xor(longest, o, 64);
        longest = other > longest ? other : longest;
      }
      longest = __builtin_amdgcn_readfirstlane(longest);
    }
    const uint8_t* text = p.codes + start;
    Summary mine = {NO_KEY, 0, -1, CHIRON_DEMUX_NONE};
    for (int r = 0; r < rounds; ++r) {
      const int q = sub + (r << shift);
      const bool live = have && q < p.patterns;
      uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
      int n = 0, group = -1;
      if (live) {
        const DemuxPattern pt = p.pat[q];
        m0 = pt.mask[0];
        m1 = pt.mask[1];
        m2 = pt.mask[2];
        m3 = pt.mask[3];
        n = pt.len;
        group = pt.group;
      }
      const uint64_t top = n > 0 ? (uint64_t)1 << (n - 1) : 0;
      uint64_t Pv = ~(uint64_t)0, Mv = 0;
      int score = n, best = n, end = 0;
      for (int j0 = 0; j0 < longest; j0 += 8) {
        // eight bases; a slot that has ended reads nothing (its window's padding ends at its own 8-byte boundary)
        const uint64_t word = j0 < m ? *(const uint64_t*)(text + j0) : ~(uint64_t)0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = (int)(word >> (8 * k)) & 0xFF;
          const uint64_t Eq = c == 0 ? m0 : c == 1 ? m1 : c == 2 ? m2 : c == 3 ? m3 : 0;
          score += advance_block(Pv, Mv, Eq, 0, top);   // hin = 0: the first row is free, nothing is shifted in
          // the first minimum, and only while the slot's window lasts; what a lane computes past it is never kept
          const bool better = (j0 + k < m) && score < best;
          best = better ? score : best;
          end = better ? j0 + k + 1 : end;
        }
      }
      if (live) {
        if (p.pair_dist) {
          const int64_t at = w * p.patterns + q;
          p.pair_dist[at] = (int16_t)best;
          p.pair_end[at] = (int16_t)end;
        }
        mine = merge(mine, Summary{(best << 16) | q, end, group, CHIRON_DEMUX_NONE});
      }
    }
    for (int o = P2 >> 1; o >= 1; o >>= 1) {
      Summary theirs;
      theirs.key = __shfl_xor(mine.key, o, 64);
      theirs.end = __shfl_xor(mine.end, o, 64);
      theirs.group = __shfl_xor(mine.group, o, 64);
      theirs.other = __shfl_xor(mine.other, o, 64);
      mine = merge(mine, theirs);
    }
    if (have && sub == 0) p.result[w] = DemuxResult{mine.key & 0xFFFF, mine.key >> 16, mine.end, mine.other};
  }
}

chiron_status demux_sizes(const char* who, int64_t windows, int64_t window_bytes, int64_t patterns, bool matrix, DemuxLayout* l) {
  memset(l, 0, sizeof(*l));
  if (windows < 0 || window_bytes < 0 || patterns < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative size (windows %lld, window bytes %lld, patterns %lld)", who, (long long)windows,
                     (long long)window_bytes, (long long)patterns);
  if (patterns == 0) return set_error(CHIRON_ERR_INVALID, "%s: no patterns", who);
  if (windows > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld windows in one call, at most 2^24", who, (long long)windows);
  if (patterns > CHIRON_DEMUX_MAX_PATTERNS)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld patterns in one call, at most %d", who, (long long)patterns, CHIRON_DEMUX_MAX_PATTERNS);
  if (window_bytes > windows * CHIRON_DEMUX_MAX_WINDOW)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld window bytes for %lld windows of at most %d bases", who, (long long)window_bytes,
                     (long long)windows, CHIRON_DEMUX_MAX_WINDOW);
  const size_t pairs = matrix ? (size_t)windows * (size_t)patterns * sizeof(int16_t) : 0;
  l->pat = 0;
  l->win = l->pat + up256((size_t)patterns * sizeof(DemuxPattern));
  l->codes = l->win + up256((size_t)windows * sizeof(DemuxWindow));
  l->result = l->codes + up256((size_t)window_bytes + 8 * (size_t)windows);
  l->pair_dist = l->result + up256((size_t)windows * sizeof(DemuxResult));
  l->pair_end = l->pair_dist + up256(pairs);
  l->bytes = l->pair_end + up256(pairs);
  return CHIRON_OK;
}

// the codes of `count` items of one array: none above 4
chiron_status check_codes(const char* who, const char* item, const uint8_t* codes, const int64_t* off, int64_t count) {
  for (int64_t q = 0; q < count; ++q)
    for (int64_t i = off[q]; i < off[q + 1]; ++i)
      if (codes[i] > 4)
        return set_error(CHIRON_ERR_INVALID, "%s: code %d at %lld of %s %lld outside 0..4", who, (int)codes[i], (long long)(i - off[q]), item, (long long)q);
  return CHIRON_OK;
}

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_demux_workspace_size(int64_t windows, int64_t window_bytes, int64_t patterns, int32_t want_matrix, size_t* bytes) {
  const char* who = "chiron_demux_workspace_size";
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  DemuxLayout l;
  if (chiron_status st = demux_sizes(who, windows, window_bytes, patterns, want_matrix != 0, &l)) return st;
  *bytes = windows == 0 ? 0 : l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_demux_windows(int32_t device_id, const uint8_t* win_codes, const int64_t* win_off, int64_t windows,
                                              const uint8_t* pat_codes, const int64_t* pat_off, const int32_t* pat_group, int64_t patterns,
                                              uint32_t flags, int32_t* best_out, int32_t* dist_out, int32_t* end_out, int32_t* second_out,
                                              int16_t* pair_dist_out, int16_t* pair_end_out, void* workspace, void* stream_) {
  const char* who = "chiron_demux_windows";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  const bool matrix = pair_dist_out != nullptr;
  DemuxLayout l;
  if (chiron_status st = demux_sizes(who, windows, 0, patterns, false, &l)) return st;
  if (windows == 0) return CHIRON_OK;
  if (!win_off || !pat_off) return set_error(CHIRON_ERR_INVALID, "%s: null offsets", who);
  if (!pat_codes || !pat_group) return set_error(CHIRON_ERR_INVALID, "%s: null patterns", who);
  if (!best_out || !dist_out || !end_out || !second_out) return set_error(CHIRON_ERR_INVALID, "%s: null output", who);
  if ((pair_dist_out != nullptr) != (pair_end_out != nullptr))
    return set_error(CHIRON_ERR_INVALID, "%s: pair_dist_out and pair_end_out go together, both or neither", who);
  int64_t longest = 0, window_bytes = 0, pattern_bytes = 0;
  if (chiron_status st = check_offsets(who, "pat", "pattern", "bases", pat_off, patterns, CHIRON_DEMUX_MAX_PATTERN, &longest, &pattern_bytes)) return st;
  for (int64_t q = 0; q < patterns; ++q) {
    if (pat_off[q + 1] == pat_off[q]) return set_error(CHIRON_ERR_INVALID, "%s: pattern %lld has no bases", who, (long long)q);
    if (pat_group[q] < 0) return set_error(CHIRON_ERR_INVALID, "%s: pat_group[%lld] = %d is negative", who, (long long)q, (int)pat_group[q]);
  }
  if (chiron_status st = check_offsets(who, "win", "window", "bases", win_off, windows, CHIRON_DEMUX_MAX_WINDOW, &longest, &window_bytes)) return st;
  if (window_bytes > 0 && !win_codes) return set_error(CHIRON_ERR_INVALID, "%s: null windows", who);
  if (chiron_status st = check_codes(who, "pattern", pat_codes, pat_off, patterns)) return st;
  if (chiron_status st = check_codes(who, "window", win_codes, win_off, windows)) return st;
  if (chiron_status st = demux_sizes(who, windows, window_bytes, patterns, matrix, &l)) return st;
  // every refusal but the device's has passed: only now the records and the padded copy of the windows
  std::vector<DemuxPattern> pats((size_t)patterns);
  for (int64_t q = 0; q < patterns; ++q) pats[(size_t)q] = demux_pack_pattern(pat_codes + pat_off[q], (int32_t)(pat_off[q + 1] - pat_off[q]), pat_group[q]);
  std::vector<DemuxWindow> recs((size_t)windows);
  const int64_t packed_bytes = demux_packed_bytes(win_off, windows);   // <= window_bytes + 7 windows
  std::vector<uint8_t> packed((size_t)packed_bytes + 8);
  demux_pack_windows(win_codes, win_off, windows, recs.data(), packed.data());
  if (chiron_status st = use_device_workspace(who, device_id, workspace)) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.pat, pats.data(), pats.size() * sizeof(DemuxPattern), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.win, recs.data(), recs.size() * sizeof(DemuxWindow), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (packed_bytes > 0 && hipMemcpyAsync(ws + l.codes, packed.data(), (size_t)packed_bytes, hipMemcpyHostToDevice, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the windows to the device failed", who);
  int shift = 0;
  while (shift < 6 && ((int64_t)1 << shift) < patterns) ++shift;
  DemuxParams p;
  p.pat = (const DemuxPattern*)(ws + l.pat);
  p.win = (const DemuxWindow*)(ws + l.win);
  p.codes = (const uint8_t*)(ws + l.codes);
  p.result = (DemuxResult*)(ws + l.result);
  p.pair_dist = matrix ? (int16_t*)(ws + l.pair_dist) : nullptr;
  p.pair_end = matrix ? (int16_t*)(ws + l.pair_end) : nullptr;
  p.windows = windows;
  p.patterns = (int32_t)patterns;
  p.p2_shift = shift;
  const int64_t slots = 64 >> shift;
  const int64_t want = ((windows + slots - 1) / slots + WAVES - 1) / WAVES;
  const dim3 grid((unsigned)(want < CHIRON_DEMUX_MAX_GROUPS ? want : CHIRON_DEMUX_MAX_GROUPS));
  if (shift == 6)
    hipLaunchKernelGGL(demux_kernel<true>, grid, dim3(NT), 0, stream, p);
  else
    hipLaunchKernelGGL(demux_kernel<false>, grid, dim3(NT), 0, stream, p);
  if (chiron_status st = launched(who)) return st;
  std::vector<DemuxResult> res((size_t)windows);
  const size_t pair_bytes = (size_t)windows * (size_t)patterns * sizeof(int16_t);
  if (hipMemcpyAsync(res.data(), ws + l.result, res.size() * sizeof(DemuxResult), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      (matrix && hipMemcpyAsync(pair_dist_out, ws + l.pair_dist, pair_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      (matrix && hipMemcpyAsync(pair_end_out, ws + l.pair_end, pair_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the search kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  for (int64_t w = 0; w < windows; ++w) {
    best_out[w] = res[(size_t)w].best;
    dist_out[w] = res[(size_t)w].dist;
    end_out[w] = res[(size_t)w].end;
    second_out[w] = res[(size_t)w].second;
  }
  return CHIRON_OK;
}
