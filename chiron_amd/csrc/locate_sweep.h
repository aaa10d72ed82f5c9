// What locate.hip and event_locate.hip share: the subsequence-DTW sweep of locate_kernel and event_locate_kernel (device), and the
// workspace layout, the argument checks and the launches of chiron_signal_locate and chiron_event_locate (host).  The host part
// takes the entry point's name and nouns: the text of chiron_last_error() is part of what the tests pin.
//
//   locate_sweep<REACH>  REACH is the most columns a path moves a row: 1 for samples (stay or step), 2 for events (stay, step, or
//                  skip a column at a price).  One launch runs CHUNK = 64 rows of every item; an item's DP row, (cost, start) a
//                  column as one 64-bit word with the cost above the start, lives in the workspace between launches in two buffers
//                  that the launches swap.  A wave takes one (item, tile of 1024 columns); the units are dealt to the launch's
//                  waves in a loop.  Row r's query value sits on lane r and every row reads its own with v_readlane.  Lane l keeps
//                  the tile's columns 16 l .. 16 l + 15 in registers, their levels with them (and for REACH 2 their skip prices:
//                  the penalty, or INF where the column to the left is a break), and REACH columns of the halo: the HALO = REACH x
//                  64 columns left of the tile, columns REACH l .. REACH l + REACH - 1 of them.  A row updates a lane's columns
//                  from the highest down, so column k still sees the old columns k - 1 .. k - REACH; the first REACH columns take
//                  the old last REACH columns of lane l - 1 by DPP wave shifts, lane 0 the old last REACH halo columns by lane
//                  reads.  The halo runs the same step with nothing coming in at its left end: after r rows the halo is right from
//                  column REACH r on; an owned column reads its last REACH columns of row r - 1, right while REACH (r - 1) <= HALO -
//                  REACH: through all 64 rows of the launch.  Only owned columns are stored.  An item whose last row lies in the
//                  launch reduces its owned columns to the block triple instead: a lexmin over (cost, column) in the lane and then
//                  across the wave, and one lane stores it.  Items with fewer rows are idle in later launches.
//
// Costs are uint32 with INF = 2^30 for a column without a path; a break column's biased level lies 2^30 above every query value, so
// its sum passes INF and is cut back to it; a skip price of INF does the same for a skip across a break.  Every offset is 64-bit.
// No LDS, no scratch, no indexed register array (the columns are unrolled), no workgroup barrier, no wave that waits for another.
// Stores are plain vector stores.  REACH is the only compile-time parameter and the row loop has no run-time switch.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "locate_pack.h"

namespace chiron {

// ---------------------------------------------------------------------------------------------
// device: the sweep
// ---------------------------------------------------------------------------------------------
constexpr int NT = CHIRON_LOCATE_THREADS;
constexpr int WAVES = NT / 64;
constexpr int COLS = 16;                              // columns a lane
constexpr int TILE = 64 * COLS;                       // columns a wave owns
constexpr int CHUNK = CHIRON_LOCATE_CHUNK;            // rows a launch
constexpr unsigned INF = 1u << 30;                    // a column without a path; every real cost is below it
constexpr unsigned BIAS = 32768;                      // query values and levels as unsigned: 0 .. 65535
constexpr unsigned BRK = INF + 2 * 65536;             // a break column's biased level: |x - BRK| > INF for every query value
static_assert(TILE == CHIRON_LOCATE_BLOCK, "a wave's owned columns are one block of the output");
static_assert(CHUNK == 64, "row r's query value sits on lane r");
static_assert(CHIRON_EVENT_CHUNK == CHUNK && CHIRON_EVENT_HALO == 2 * CHUNK, "one chunk for both kernels; the halo is REACH columns a lane");
static_assert(CHUNK == LOCATE_CHUNK && CHIRON_LOCATE_BLOCK == LOCATE_BLOCK, "header and pack agree");
static_assert(CHIRON_LOCATE_BREAK == LOCATE_BREAK && CHIRON_LOCATE_NONE == LOCATE_NONE, "header and pack agree");
static_assert(NT % 64 == 0, "whole waves");

// A column's pair as one word, the cost above the start: the lexmin of two pairs is the smaller word.
typedef unsigned long long pair_t;

struct SweepParams {
  const int16_t* query;              // the call's samples or events
  const int64_t* query_off;          // [items + 1], as the caller gave them: the kernel subtracts query_off[0]
  const int32_t* level;              // [ref_len]
  const pair_t* prev;                // [items][stride]: the row before this launch's first (not read by launch 0)
  pair_t* next;                      // [items][stride]: this launch's last row
  int32_t* block;                    // [items][tiles][3]
  int64_t items;
  int64_t stride;                    // columns of an item's row in the workspace: tiles * TILE
  int32_t ref_len;
  int32_t tiles;
  int32_t chunk;                     // this launch's rows: chunk * CHUNK ..
  uint32_t penalty;                  // what a skipped column costs; unused at REACH 1
};

// lane l takes v of lane l - 1, lane 0 takes `first` (DPP wave_shr:1; without bound_ctrl a lane with no source keeps `old`)
__device__ __forceinline__ int shift_in(int first, int v) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

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

__device__ __forceinline__ unsigned biased(int32_t e) { return e == CHIRON_LOCATE_BREAK ? BRK : (unsigned)(e + (int)BIAS); }

// what the skip over a column of biased level `over` costs
__device__ __forceinline__ unsigned price_of(unsigned over, unsigned penalty) { return over == BRK ? INF : penalty; }

// One cell: the lexmin of k, the column's own pair of the row before, k1, its left neighbour's, and at REACH 2 k2, the pair two to
// the left with the skip's price on its cost, plus |x - e|.  k2's cost and the price are at most INF each, so the sum stays inside
// 32 bits; k is at most INF, so the minimum is.  At REACH 1 k2 and the price are not looked at.
template <int REACH>
__device__ __forceinline__ void cell(pair_t& k, pair_t k1, pair_t k2, unsigned price, unsigned x, unsigned e) {
  pair_t m = k1 < k ? k1 : k;
  if constexpr (REACH == 2) {
    const pair_t s = pair_of((unsigned)(k2 >> 32) + price, (int)k2);
    m = s < m ? s : m;
  }
  k = pair_of(add_to((unsigned)(m >> 32), x, e), (int)m);
}

template <int REACH>
__device__ __forceinline__ void locate_sweep(const SweepParams& p) {
  static_assert(REACH == 1 || REACH == 2, "stay and step, or stay, step and skip");
  constexpr int HALO = REACH * CHUNK;                             // columns left of the tile a launch recomputes: REACH a lane
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t units = p.items * p.tiles;
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  const int row0 = p.chunk * CHUNK;
  for (int64_t u = (int64_t)blockIdx.x * WAVES + wv; u < units; u += nwaves) {
    const int64_t it = u / p.tiles;
    const int tile = (int)(u - it * p.tiles);
    const int64_t q64 = p.query_off[it + 1] - p.query_off[it];
    const int Q = (int)q64;
    if (row0 >= Q) continue;                                      // the item ended in an earlier launch
    const int rows = Q - row0 < CHUNK ? Q - row0 : CHUNK;
    const int16_t* __restrict__ x = p.query + (p.query_off[it] - p.query_off[0]) + row0;
    const unsigned xv = lane < rows ? (unsigned)((int)x[lane] + (int)BIAS) : 0u;   // row r's query value on lane r
    const int col0 = tile * TILE + lane * COLS;                   // below 2^28 + 1024
    const int hcol = tile * TILE - HALO + REACH * lane;           // this lane's first halo column; below 0 left of the reference
    const int64_t at = it * p.stride + col0;
    const int64_t hat = it * p.stride + hcol;

    unsigned e[COLS], he[REACH], price[COLS] = {}, hprice[REACH] = {};   // the prices are idle at REACH 1
    pair_t c[COLS], hc[REACH];
#pragma unroll
    for (int k = 0; k < COLS; ++k) e[k] = col0 + k < p.ref_len ? biased(p.level[col0 + k]) : BRK;
    if constexpr (REACH == 2) {
      // the column left of a lane's first: col0 - 1 < ref_len wherever col0 is a column, and the price of a column past the end is idle
      price[0] = price_of(col0 >= 1 && col0 <= p.ref_len ? biased(p.level[col0 - 1]) : BRK, p.penalty);
#pragma unroll
      for (int k = 1; k < COLS; ++k) price[k] = price_of(e[k - 1], p.penalty);
    }
#pragma unroll
    for (int k = 0; k < REACH; ++k) he[k] = hcol >= 0 ? biased(p.level[hcol + k]) : BRK;   // hcol + k < tile * TILE < ref_len
    if constexpr (REACH == 2) {
      hprice[0] = price_of(hcol >= 1 ? biased(p.level[hcol - 1]) : BRK, p.penalty);
      hprice[1] = price_of(he[0], p.penalty);
    }
    int first;                                                    // the first row this launch steps through
    if (p.chunk == 0) {                                           // row 0: every column starts its own path
      const unsigned x0 = (unsigned)__builtin_amdgcn_readlane((int)xv, 0);
#pragma unroll
      for (int k = 0; k < COLS; ++k) c[k] = pair_of(add_to(0, x0, e[k]), col0 + k);
#pragma unroll
      for (int k = 0; k < REACH; ++k) hc[k] = pair_of(add_to(0, x0, he[k]), hcol + k);
      first = 1;
    } else {
#pragma unroll
      for (int k = 0; k < COLS; ++k) c[k] = p.prev[at + k];
#pragma unroll
      for (int k = 0; k < REACH; ++k) hc[k] = hcol >= 0 ? p.prev[hat + k] : pair_of(INF, 0);
      first = 0;
    }

    for (int r = first; r < rows; ++r) {
      const unsigned xr = (unsigned)__builtin_amdgcn_readlane((int)xv, r);
      // The old last REACH columns of lane l - 1, the nearest first: nothing comes into the halo's left end, and lane 0 takes the
      // halo's last columns.  They are not filled in a loop over REACH, and the first REACH columns and the halo are written out,
      // not folded into the loop below with conditions on k: either spelling gave the REACH 2 kernel another schedule, 0.5 % slower
      // on the MI355X (Resources).
      const pair_t none = pair_of(INF, 0);
      pair_t in[REACH], hin[REACH];
      hin[0] = shift_in(none, hc[REACH - 1]);
      if constexpr (REACH == 2) hin[1] = shift_in(none, hc[0]);
      in[0] = shift_in(lane_pair(hc[REACH - 1], 63), c[COLS - 1]);
      if constexpr (REACH == 2) in[1] = shift_in(lane_pair(hc[0], 63), c[COLS - 2]);
#pragma unroll
      for (int k = COLS - 1; k >= REACH; --k) cell<REACH>(c[k], c[k - 1], c[k - REACH], price[k], xr, e[k]);
      if constexpr (REACH == 2) cell<REACH>(c[1], c[0], in[0], price[1], xr, e[1]);
      cell<REACH>(c[0], in[0], in[REACH - 1], price[0], xr, e[0]);
      if constexpr (REACH == 2) cell<REACH>(hc[1], hc[0], hin[0], hprice[1], xr, he[1]);
      cell<REACH>(hc[0], hin[0], hin[REACH - 1], hprice[0], xr, he[0]);
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

// ---------------------------------------------------------------------------------------------
// host: the workspace and the call
// ---------------------------------------------------------------------------------------------
struct SweepLayout {
  size_t query_off, query, level, block, row[2], bytes;   // row: the two buffers
  int64_t tiles, stride;
};

// What an entry point is and calls its arguments.
struct SweepCall {
  const char* who;
  const char* unit;                  // what a query counts: "samples", "events"
  const char* off_name;              // "sample_off", "event_off"
  int64_t max_query;                 // CHIRON_LOCATE_MAX_QUERY, CHIRON_EVENT_MAX_QUERY
  void (*kernel)(SweepParams);
  uint32_t penalty;                  // checked by the caller
  const char* kernel_noun;           // "locate", "event locate"
};

// The refusals that need the counts only, and where everything lies in the workspace.
inline chiron_status sweep_sizes(const char* who, const char* unit, int64_t items, int64_t count, int64_t ref_len, SweepLayout* l) {
  if (items < 0 || count < 0 || ref_len < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative size (items %lld, %s %lld, ref_len %lld)", who, (long long)items, unit, (long long)count,
                     (long long)ref_len);
  if (items > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items in one call, at most 2^31 - 1", who, (long long)items);
  if (count > CHIRON_SIGNAL_MAX_SAMPLES)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld %s in one call, at most %d", who, (long long)count, unit, CHIRON_SIGNAL_MAX_SAMPLES);
  if (ref_len > CHIRON_LOCATE_MAX_REF)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: ref_len %lld, at most %d", who, (long long)ref_len, CHIRON_LOCATE_MAX_REF);
  l->tiles = locate_blocks(ref_len);
  l->stride = l->tiles * TILE;
  const int64_t cells = items * l->stride;                        // below 2^31 * (2^28 + 2^10): inside int64
  if (cells > CHIRON_LOCATE_MAX_CELLS)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items on %lld columns are %lld row cells, at most 2^40", who, (long long)items, (long long)ref_len,
                     (long long)cells);
  l->query_off = 0;
  l->query = l->query_off + up256(items > 0 ? (size_t)(items + 1) * sizeof(int64_t) : 0);
  l->level = l->query + up256((size_t)count * sizeof(int16_t));
  l->block = l->level + up256((size_t)ref_len * sizeof(int32_t));
  l->row[0] = l->block + up256((size_t)(items * l->tiles) * 3 * sizeof(int32_t));
  l->row[1] = l->row[0] + up256((size_t)cells * sizeof(pair_t));
  l->bytes = l->row[1] + up256((size_t)cells * sizeof(pair_t));
  return CHIRON_OK;
}

inline chiron_status sweep_workspace_size(const char* who, const char* unit, int64_t items, int64_t count, int64_t ref_len, size_t* bytes) {
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  SweepLayout l;
  if (chiron_status st = sweep_sizes(who, unit, items, count, ref_len, &l)) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

// Everything of a call behind its flags (and its penalty): the refusals, the copies in, the launches, the triples out.
inline chiron_status sweep_call(const SweepCall& call, int32_t device_id, const int16_t* query, const int64_t* off, int64_t items, const int32_t* ref_level,
                                int64_t ref_len, int32_t* block_out, void* workspace, size_t workspace_bytes, void* stream_) {
  const char* who = call.who;
  SweepLayout l;
  if (chiron_status st = sweep_sizes(who, call.unit, items, 0, ref_len, &l)) return st;
  if (items == 0) return CHIRON_OK;   // nothing to compute and nothing to write: no device is touched
  if (!off || !query) return set_error(CHIRON_ERR_INVALID, "%s: null %s / %s", who, call.unit, call.off_name);
  if (ref_len > 0 && !ref_level) return set_error(CHIRON_ERR_INVALID, "%s: null ref_level", who);
  if (ref_len > 0 && !block_out) return set_error(CHIRON_ERR_INVALID, "%s: null block_out", who);
  int64_t longest = 0;
  LocateFinding f = locate_check_offsets(off, items, call.max_query, &longest);
  if (f.fault == LOCATE_OFF_NEGATIVE) return set_error(CHIRON_ERR_INVALID, "%s: %s[0] = %lld is negative", who, call.off_name, (long long)f.value);
  if (f.fault == LOCATE_OFF_ORDER)
    return set_error(CHIRON_ERR_INVALID, "%s: %s[%lld] = %lld below its predecessor %lld", who, call.off_name, (long long)f.at, (long long)f.value,
                     (long long)off[f.at - 1]);
  if (f.fault == LOCATE_QUERY_EMPTY) return set_error(CHIRON_ERR_INVALID, "%s: query %lld is empty", who, (long long)f.at);
  if (f.fault == LOCATE_QUERY_LONG)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: query %lld has %lld %s, at most %lld", who, (long long)f.at, (long long)f.value, call.unit,
                     (long long)call.max_query);
  const int64_t count = off[items] - off[0];
  if (chiron_status st = sweep_sizes(who, call.unit, items, count, ref_len, &l)) return st;
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
  if (hipMemcpyAsync(ws + l.query_off, off, (size_t)(items + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.query, query + off[0], (size_t)count * sizeof(int16_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.level, ref_level, (size_t)ref_len * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the queries and the reference to the device failed", who);
  SweepParams p;
  p.query = (const int16_t*)(ws + l.query);
  p.query_off = (const int64_t*)(ws + l.query_off);
  p.level = (const int32_t*)(ws + l.level);
  p.block = (int32_t*)(ws + l.block);
  p.items = items;
  p.stride = l.stride;
  p.ref_len = (int32_t)ref_len;
  p.tiles = (int32_t)l.tiles;
  p.penalty = call.penalty;
  const int64_t want = (items * l.tiles + WAVES - 1) / WAVES;
  const dim3 grid((unsigned)(want < CHIRON_LOCATE_MAX_GROUPS ? want : CHIRON_LOCATE_MAX_GROUPS));
  const int64_t launches = locate_launches(longest);
  for (int64_t k = 0; k < launches; ++k) {   // launch k writes buffer k & 1 and reads the other
    p.next = (pair_t*)(ws + l.row[k & 1]);
    p.prev = (const pair_t*)(ws + l.row[1 - (k & 1)]);
    p.chunk = (int32_t)k;
    hipLaunchKernelGGL(call.kernel, grid, dim3(NT), 0, stream, p);
    if (chiron_status st = launched(who)) return st;
  }
  if (hipMemcpyAsync(block_out, ws + l.block, (size_t)(items * l.tiles) * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the %s kernel failed (%s)", who, call.kernel_noun, hipGetErrorString(hipGetLastError()));
  return CHIRON_OK;
}

}  // namespace chiron
