// Event location for `locate --events` on gfx950: where on a reference of expected levels a query of event levels comes from, by an
// exact subsequence DTW whose path may skip a column at a price, and the host-only event detector that makes such queries.  The
// definitions are in include/chiron_amd.h and are restated in plain Python by tests/event_ref.py.
//
//   event_locate_kernel  locate_kernel's form (csrc/locate.hip) with one more predecessor.  One launch runs EVENT_CHUNK = 64 rows
//                  (events) of every item; an item's DP row, (cost, start) a column as one 64-bit word with the cost above the
//                  start, lives in the workspace between launches in two buffers that the launches swap.  A wave takes one (item,
//                  tile of 1024 columns); the units are dealt to the launch's waves in a loop.  Lane l keeps the tile's columns
//                  16 l .. 16 l + 15 in registers with their levels and their skip prices -- the penalty, or INF where the column to
//                  the left is a break -- and two columns of the halo: the 128 columns left of the tile, columns 2 l and 2 l + 1 of
//                  them.  A row updates a lane's columns from the highest down, so column k still sees the old columns k - 1 and
//                  k - 2; columns 0 and 1 take the old columns 14 and 15 of lane l - 1 by two DPP wave shifts, lane 0 the old last
//                  two halo columns by lane reads.  The halo runs the same step with nothing coming in at its left end.  A path
//                  moves at most two columns a row, so after r rows the halo's columns at least 2 r from that end are right; an
//                  owned column reads the halo's last two columns, 126 and 127, of row r - 1, which are right while 2 (r - 1) <=
//                  126: through all 64 rows of the launch.  Only owned columns are stored.  An item whose last row lies in the
//                  launch reduces its owned columns to the block triple instead, as locate_kernel does.
//
// Costs are uint32 with INF = 2^30 for a column without a path; a break column's biased level lies 2^30 above every sample, so its
// sum passes INF and is cut back to it; a skip price of INF does the same for a skip across a break.  Every offset is 64-bit.  No
// LDS, no scratch, no indexed register array, no workgroup barrier, no wave that waits for another.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "event_pack.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_LOCATE_THREADS;
constexpr int WAVES = NT / 64;
constexpr int COLS = 16;                              // columns a lane
constexpr int TILE = 64 * COLS;                       // columns a wave owns
constexpr int CHUNK = CHIRON_EVENT_CHUNK;             // rows a launch
constexpr int HALO = CHIRON_EVENT_HALO;               // columns left of the tile a launch recomputes: two a lane
constexpr unsigned INF = 1u << 30;                    // a column without a path; every real cost is below it
constexpr unsigned BIAS = 32768;                      // events and levels as unsigned: 0 .. 65535
constexpr unsigned BRK = INF + 2 * 65536;             // a break column's biased level: |x - BRK| > INF for every event
static_assert(TILE == CHIRON_LOCATE_BLOCK, "a wave's owned columns are one block of the output");
static_assert(CHUNK == 64, "row r's event sits on lane r");
static_assert(HALO == 2 * CHUNK && HALO == 2 * 64, "two columns a row, two halo columns a lane");
static_assert(CHUNK == EVENT_CHUNK && CHIRON_EVENT_MAX_QUERY == EVENT_MAX_QUERY && CHIRON_EVENT_MAX_PENALTY == EVENT_MAX_PENALTY, "header and pack agree");
static_assert(CHIRON_EVENT_MAX_SAMPLES == EVENT_MAX_SAMPLES && CHIRON_EVENT_MAX_WINDOW == EVENT_MAX_WINDOW && CHIRON_EVENT_MAX_RADIUS == EVENT_MAX_RADIUS &&
                  CHIRON_EVENT_MAX_THRESHOLD == EVENT_MAX_THRESHOLD,
              "header and pack agree");
static_assert(NT % 64 == 0, "whole waves");

struct EventParams {
  const int16_t* events;             // the call's events
  const int64_t* event_off;          // [items + 1], as the caller gave them: the kernel subtracts event_off[0]
  const int32_t* level;              // [ref_len]
  const unsigned long long* prev;    // [items][stride]: the row before this launch's first (not read by launch 0)
  unsigned long long* next;          // [items][stride]: this launch's last row
  int32_t* block;                    // [items][tiles][3]
  int64_t items;
  int64_t stride;                    // columns of an item's row in the workspace: tiles * TILE
  int32_t ref_len;
  int32_t tiles;
  int32_t chunk;                     // this launch's rows: chunk * CHUNK ..
  uint32_t penalty;                  // what a skipped column costs
};

struct EventLayout {
  size_t event_off, events, level, block, row[2], bytes;   // row: the two buffers
  int64_t tiles, stride;
};

// lane l takes v of lane l - 1, lane 0 takes `first` (DPP wave_shr:1; without bound_ctrl a lane with no source keeps `old`)
__device__ __forceinline__ int shift_in(int first, int v) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

// A column's pair as one word, the cost above the start: the lexmin of two pairs is the smaller word.
typedef unsigned long long pair_t;
__device__ __forceinline__ pair_t pair_of(unsigned cost, int start) { return ((pair_t)cost << 32) | (unsigned)start; }

__device__ __forceinline__ pair_t shift_in(pair_t first, pair_t v) {
  return pair_of((unsigned)shift_in((int)(first >> 32), (int)(v >> 32)), shift_in((int)first, (int)v));
}

// lane `from`'s pair on every lane
__device__ __forceinline__ pair_t lane_pair(pair_t v, int from) {
  return pair_of((unsigned)__builtin_amdgcn_readlane((int)(v >> 32), from), __builtin_amdgcn_readlane((int)v, from));
}

// |x - e| on top of a cost, cut back to INF: the cost is at most INF and the difference below 2^31, so nothing wraps
__device__ __forceinline__ unsigned add_to(unsigned cost, unsigned x, unsigned e) {
  const unsigned v = cost + (x > e ? x - e : e - x);
  return v < INF ? v : INF;
}

// One cell: the lexmin of k, the column's own pair of the row before, k1, its left neighbour's, and k2, the pair two to the left
// with the skip's price on its cost, plus |x - e|.  k2's cost and the price are at most INF each, so the sum stays inside 32 bits;
// k is at most INF, so the minimum is.
__device__ __forceinline__ void cell(pair_t& k, pair_t k1, pair_t k2, unsigned price, unsigned x, unsigned e) {
  const pair_t s = pair_of((unsigned)(k2 >> 32) + price, (int)k2);
  pair_t m = k1 < k ? k1 : k;
  m = s < m ? s : m;
  k = pair_of(add_to((unsigned)(m >> 32), x, e), (int)m);
}

__device__ __forceinline__ unsigned biased(int32_t e) { return e == CHIRON_LOCATE_BREAK ? BRK : (unsigned)(e + (int)BIAS); }

// what the skip over a column of biased level `over` costs
__device__ __forceinline__ unsigned price_of(unsigned over, unsigned penalty) { return over == BRK ? INF : penalty; }

__global__ __launch_bounds__(CHIRON_LOCATE_THREADS) void event_locate_kernel(EventParams p) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t units = p.items * p.tiles;
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  const int row0 = p.chunk * CHUNK;
  for (int64_t u = (int64_t)blockIdx.x * WAVES + wv; u < units; u += nwaves) {
    const int64_t it = u / p.tiles;
    const int tile = (int)(u - it * p.tiles);
    const int64_t q64 = p.event_off[it + 1] - p.event_off[it];
    const int Q = (int)q64;
    if (row0 >= Q) continue;                                      // the item ended in an earlier launch
    const int rows = Q - row0 < CHUNK ? Q - row0 : CHUNK;
    const int16_t* __restrict__ x = p.events + (p.event_off[it] - p.event_off[0]) + row0;
    const unsigned xv = lane < rows ? (unsigned)((int)x[lane] + (int)BIAS) : 0u;   // row r's event on lane r
    const int col0 = tile * TILE + lane * COLS;                   // below 2^28 + 1024
    const int hcol = tile * TILE - HALO + 2 * lane;               // this lane's first halo column; below 0 left of the reference
    const int64_t at = it * p.stride + col0;
    const int64_t hat = it * p.stride + hcol;

    unsigned e[COLS], price[COLS];
    pair_t c[COLS];
#pragma unroll
    for (int k = 0; k < COLS; ++k) e[k] = col0 + k < p.ref_len ? biased(p.level[col0 + k]) : BRK;
    // the column left of a lane's first: col0 - 1 < ref_len wherever col0 is a column, and the price of a column past the end is idle
    price[0] = price_of(col0 >= 1 && col0 <= p.ref_len ? biased(p.level[col0 - 1]) : BRK, p.penalty);
#pragma unroll
    for (int k = 1; k < COLS; ++k) price[k] = price_of(e[k - 1], p.penalty);
    unsigned he[2], hprice[2];                                    // hcol + 1 < tile * TILE < ref_len
    he[0] = hcol >= 0 ? biased(p.level[hcol]) : BRK;
    he[1] = hcol >= 0 ? biased(p.level[hcol + 1]) : BRK;
    hprice[0] = price_of(hcol >= 1 ? biased(p.level[hcol - 1]) : BRK, p.penalty);
    hprice[1] = price_of(he[0], p.penalty);
    pair_t hc[2];
    int first;                                                    // the first row this launch steps through
    if (p.chunk == 0) {                                           // row 0: every column starts its own path
      const unsigned x0 = (unsigned)__builtin_amdgcn_readlane((int)xv, 0);
#pragma unroll
      for (int k = 0; k < COLS; ++k) c[k] = pair_of(add_to(0, x0, e[k]), col0 + k);
      hc[0] = pair_of(add_to(0, x0, he[0]), hcol);
      hc[1] = pair_of(add_to(0, x0, he[1]), hcol + 1);
      first = 1;
    } else {
#pragma unroll
      for (int k = 0; k < COLS; ++k) c[k] = p.prev[at + k];
      hc[0] = hcol >= 0 ? p.prev[hat] : pair_of(INF, 0);
      hc[1] = hcol >= 0 ? p.prev[hat + 1] : pair_of(INF, 0);
      first = 0;
    }

    for (int r = first; r < rows; ++r) {
      const unsigned xr = (unsigned)__builtin_amdgcn_readlane((int)xv, r);
      const pair_t none = pair_of(INF, 0);                        // nothing comes into the halo's left end
      const pair_t hin1 = shift_in(none, hc[1]);
      const pair_t hin2 = shift_in(none, hc[0]);
      const pair_t in1 = shift_in(lane_pair(hc[1], 63), c[COLS - 1]);   // lane 0 takes the halo's last two columns
      const pair_t in2 = shift_in(lane_pair(hc[0], 63), c[COLS - 2]);
#pragma unroll
      for (int k = COLS - 1; k >= 2; --k) cell(c[k], c[k - 1], c[k - 2], price[k], xr, e[k]);
      cell(c[1], c[0], in1, price[1], xr, e[1]);
      cell(c[0], in1, in2, price[0], xr, e[0]);
      cell(hc[1], hc[0], hin1, hprice[1], xr, he[1]);
      cell(hc[0], hin1, hin2, hprice[0], xr, he[0]);
    }

    if (row0 + rows < Q) {                                        // more rows to come: the owned columns of this launch's last row
#pragma unroll
      for (int k = 0; k < COLS; ++k) p.next[at + k] = c[k];
      continue;
    }
    // the item's last row: the block's least cost, the smallest column that attains it, and that column's start
    pair_t best = pair_of((unsigned)(c[0] >> 32), col0);
    int bs = (int)c[0];
#pragma unroll
    for (int k = 1; k < COLS; ++k) {
      const pair_t key = pair_of((unsigned)(c[k] >> 32), col0 + k);
      if (key < best) {
        best = key;
        bs = (int)c[k];
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const pair_t other = (pair_t)__shfl_xor((long long)best, o, 64);
      const int os = __shfl_xor(bs, o, 64);
      if (other < best) {
        best = other;
        bs = os;
      }
    }
    if (lane == 0) {
      int32_t* __restrict__ out = p.block + (it * p.tiles + tile) * 3;
      const unsigned cost = (unsigned)(best >> 32);
      const bool none = cost >= INF;
      out[0] = none ? CHIRON_LOCATE_NONE : (int32_t)cost;
      out[1] = none ? CHIRON_LOCATE_NONE : (int32_t)(unsigned)best;
      out[2] = none ? CHIRON_LOCATE_NONE : bs;
    }
  }
}

chiron_status event_sizes(const char* who, int64_t items, int64_t events, int64_t ref_len, EventLayout* l) {
  if (items < 0 || events < 0 || ref_len < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative size (items %lld, events %lld, ref_len %lld)", who, (long long)items, (long long)events,
                     (long long)ref_len);
  if (items > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items in one call, at most 2^31 - 1", who, (long long)items);
  if (events > CHIRON_SIGNAL_MAX_SAMPLES)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld events in one call, at most %d", who, (long long)events, CHIRON_SIGNAL_MAX_SAMPLES);
  if (ref_len > CHIRON_LOCATE_MAX_REF)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: ref_len %lld, at most %d", who, (long long)ref_len, CHIRON_LOCATE_MAX_REF);
  l->tiles = locate_blocks(ref_len);
  l->stride = l->tiles * TILE;
  const int64_t cells = items * l->stride;                        // below 2^31 * (2^28 + 2^10): inside int64
  if (cells > CHIRON_LOCATE_MAX_CELLS)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items on %lld columns are %lld row cells, at most 2^40", who, (long long)items, (long long)ref_len,
                     (long long)cells);
  l->event_off = 0;
  l->events = l->event_off + up256(items > 0 ? (size_t)(items + 1) * sizeof(int64_t) : 0);
  l->level = l->events + up256((size_t)events * sizeof(int16_t));
  l->block = l->level + up256((size_t)ref_len * sizeof(int32_t));
  l->row[0] = l->block + up256((size_t)(items * l->tiles) * 3 * sizeof(int32_t));
  l->row[1] = l->row[0] + up256((size_t)cells * sizeof(pair_t));
  l->bytes = l->row[1] + up256((size_t)cells * sizeof(pair_t));
  return CHIRON_OK;
}

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_signal_events(const int16_t* samples, const int64_t* sample_off, int64_t items, int32_t window, int32_t radius,
                                              int64_t threshold, int32_t max_events, uint32_t flags, int32_t* count_out, int32_t* border_out,
                                              int16_t* level_out, uint8_t* truncated_out) {
  const char* who = "chiron_signal_events";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  if (items < 0) return set_error(CHIRON_ERR_INVALID, "%s: negative size (items %lld)", who, (long long)items);
  if (items > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items in one call, at most 2^31 - 1", who, (long long)items);
  if (window < 2 || window > CHIRON_EVENT_MAX_WINDOW)
    return set_error(CHIRON_ERR_INVALID, "%s: window %d outside 2..%d", who, window, CHIRON_EVENT_MAX_WINDOW);
  if (radius < 1 || radius > CHIRON_EVENT_MAX_RADIUS)
    return set_error(CHIRON_ERR_INVALID, "%s: radius %d outside 1..%d", who, radius, CHIRON_EVENT_MAX_RADIUS);
  if (threshold < 1 || threshold > CHIRON_EVENT_MAX_THRESHOLD)
    return set_error(CHIRON_ERR_INVALID, "%s: threshold %lld outside 1..2^52", who, (long long)threshold);
  if (max_events < 1 || max_events > CHIRON_EVENT_MAX_SAMPLES)
    return set_error(CHIRON_ERR_INVALID, "%s: max_events %d outside 1..%d", who, max_events, CHIRON_EVENT_MAX_SAMPLES);
  if (items == 0) return CHIRON_OK;   // nothing to cut and nothing to write
  if (!sample_off || !samples) return set_error(CHIRON_ERR_INVALID, "%s: null samples / sample_off", who);
  if (!count_out || !border_out || !level_out || !truncated_out)
    return set_error(CHIRON_ERR_INVALID, "%s: null count_out / border_out / level_out / truncated_out", who);
  int64_t longest = 0;
  const LocateFinding f = event_check_offsets(sample_off, items, EVENT_MAX_SAMPLES, &longest);
  if (f.fault == LOCATE_OFF_NEGATIVE) return set_error(CHIRON_ERR_INVALID, "%s: sample_off[0] = %lld is negative", who, (long long)f.value);
  if (f.fault == LOCATE_OFF_ORDER)
    return set_error(CHIRON_ERR_INVALID, "%s: sample_off[%lld] = %lld below its predecessor %lld", who, (long long)f.at, (long long)f.value,
                     (long long)sample_off[f.at - 1]);
  if (f.fault == LOCATE_QUERY_EMPTY) return set_error(CHIRON_ERR_INVALID, "%s: item %lld is empty", who, (long long)f.at);
  if (f.fault == LOCATE_QUERY_LONG)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: item %lld has %lld samples, at most %d", who, (long long)f.at, (long long)f.value, CHIRON_EVENT_MAX_SAMPLES);
  std::vector<int64_t> t;   // the statistic of one item: 8 bytes a sample, 1 MiB at most
  for (int64_t i = 0; i < items; ++i) {
    const int64_t at = sample_off[i] - sample_off[0];
    bool truncated = false;
    count_out[i] = event_segment(samples + sample_off[i], sample_off[i + 1] - sample_off[i], window, radius, threshold, max_events, border_out + at + i,
                                 level_out + at, &truncated, t);
    truncated_out[i] = truncated ? 1 : 0;
  }
  return CHIRON_OK;
}

extern "C" chiron_status chiron_event_locate_workspace_size(int64_t items, int64_t events, int64_t ref_len, size_t* bytes) {
  const char* who = "chiron_event_locate_workspace_size";
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  EventLayout l;
  if (chiron_status st = event_sizes(who, items, events, ref_len, &l)) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_event_locate(int32_t device_id, const int16_t* events, const int64_t* event_off, int64_t items,
                                             const int32_t* ref_level, int64_t ref_len, int32_t penalty, int32_t* block_out, void* workspace,
                                             size_t workspace_bytes, uint32_t flags, void* stream_) {
  const char* who = "chiron_event_locate";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  if (penalty < 0 || penalty > CHIRON_EVENT_MAX_PENALTY)
    return set_error(CHIRON_ERR_INVALID, "%s: penalty %d outside 0..%d", who, penalty, CHIRON_EVENT_MAX_PENALTY);
  EventLayout l;
  if (chiron_status st = event_sizes(who, items, 0, ref_len, &l)) return st;
  if (items == 0) return CHIRON_OK;   // nothing to compute and nothing to write: no device is touched
  if (!event_off || !events) return set_error(CHIRON_ERR_INVALID, "%s: null events / event_off", who);
  if (ref_len > 0 && !ref_level) return set_error(CHIRON_ERR_INVALID, "%s: null ref_level", who);
  if (ref_len > 0 && !block_out) return set_error(CHIRON_ERR_INVALID, "%s: null block_out", who);
  int64_t longest = 0;
  LocateFinding f = event_check_offsets(event_off, items, EVENT_MAX_QUERY, &longest);
  if (f.fault == LOCATE_OFF_NEGATIVE) return set_error(CHIRON_ERR_INVALID, "%s: event_off[0] = %lld is negative", who, (long long)f.value);
  if (f.fault == LOCATE_OFF_ORDER)
    return set_error(CHIRON_ERR_INVALID, "%s: event_off[%lld] = %lld below its predecessor %lld", who, (long long)f.at, (long long)f.value,
                     (long long)event_off[f.at - 1]);
  if (f.fault == LOCATE_QUERY_EMPTY) return set_error(CHIRON_ERR_INVALID, "%s: query %lld is empty", who, (long long)f.at);
  if (f.fault == LOCATE_QUERY_LONG)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: query %lld has %lld events, at most %d", who, (long long)f.at, (long long)f.value, CHIRON_EVENT_MAX_QUERY);
  const int64_t n_events = event_off[items] - event_off[0];
  if (chiron_status st = event_sizes(who, items, n_events, ref_len, &l)) return st;
  f = locate_check_levels(ref_level, ref_len);
  if (f.fault == LOCATE_LEVEL_RANGE)
    return set_error(CHIRON_ERR_INVALID, "%s: level %lld of column %lld outside -%d..%d and not the break value", who, (long long)f.value, (long long)f.at,
                     LOCATE_LEVEL_MAX, LOCATE_LEVEL_MAX);
  if (ref_len == 0) return CHIRON_OK;   // no column and no block: nothing to fill, no device is touched
  if (chiron_status st = use_device_workspace(who, device_id, workspace)) return st;
  if (workspace_bytes < l.bytes)
    return set_error(CHIRON_ERR_INVALID, "%s: a workspace of %llu bytes, %llu are needed", who, (unsigned long long)workspace_bytes, (unsigned long long)l.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.event_off, event_off, (size_t)(items + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.events, events + event_off[0], (size_t)n_events * sizeof(int16_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.level, ref_level, (size_t)ref_len * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the queries and the reference to the device failed", who);
  EventParams p;
  p.events = (const int16_t*)(ws + l.events);
  p.event_off = (const int64_t*)(ws + l.event_off);
  p.level = (const int32_t*)(ws + l.level);
  p.block = (int32_t*)(ws + l.block);
  p.items = items;
  p.stride = l.stride;
  p.ref_len = (int32_t)ref_len;
  p.tiles = (int32_t)l.tiles;
  p.penalty = (uint32_t)penalty;
  const int64_t want = (items * l.tiles + WAVES - 1) / WAVES;
  const dim3 grid((unsigned)(want < CHIRON_LOCATE_MAX_GROUPS ? want : CHIRON_LOCATE_MAX_GROUPS));
  const int64_t launches = event_launches(longest);
  for (int64_t k = 0; k < launches; ++k) {   // launch k writes buffer k & 1 and reads the other
    p.next = (pair_t*)(ws + l.row[k & 1]);
    p.prev = (const pair_t*)(ws + l.row[1 - (k & 1)]);
    p.chunk = (int32_t)k;
    hipLaunchKernelGGL(event_locate_kernel, grid, dim3(NT), 0, stream, p);
    if (chiron_status st = launched(who)) return st;
  }
  if (hipMemcpyAsync(block_out, ws + l.block, (size_t)(items * l.tiles) * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the event locate kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  return CHIRON_OK;
}
