// Signal location for `locate` on gfx950: where on a reference of expected levels a stretch of raw samples comes from, by an exact
// subsequence DTW of the samples against every column of the reference.  The definition is in include/chiron_amd.h and is restated
// in plain Python by tests/locate_ref.py.
//
//   locate_kernel  One launch runs LOCATE_CHUNK = 64 rows (samples) of every item; the DP row of an item, (cost, start) a column,
//                  lives in the workspace between launches, one 64-bit word a column with the cost above the start, in two
//                  buffers that the launches swap.  A wave takes one (item, tile of 1024 columns); the units are dealt to the
//                  launch's waves in a loop.  Lane l keeps the tile's columns
//                  16 l .. 16 l + 15 in registers, their levels with them, and one column of the halo: the 64 columns left of
//                  the tile, column l of them.  A row updates a lane's columns from the highest down; column 0 takes the old
//                  column 15 of lane l - 1 by a DPP wave shift, lane 0 the old last halo column by a lane read.  The halo runs
//                  the same step with no value coming in at its left end: after r rows its columns at least r from that end are
//                  right, so through all 64 rows of the launch every owned column is.  Only owned columns are stored.
//                  An item whose last row lies in the launch reduces its owned columns to the block triple instead: a lexmin
//                  over (cost, column) in the lane and then across the wave, and one lane stores it.  Items with fewer rows are
//                  idle in later launches.
//
// Costs are uint32 with INF = 2^30 for a column without a path; a break column's biased level lies 2^30 above every sample, so its
// sum passes INF and is cut back to it.  Every offset is 64-bit.  No LDS, no scratch, no indexed register array (the 16 columns
// are unrolled), no workgroup barrier, no wave that waits for another.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "locate_pack.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_LOCATE_THREADS;
constexpr int WAVES = NT / 64;
constexpr int COLS = 16;                              // columns a lane
constexpr int TILE = 64 * COLS;                       // columns a wave owns
constexpr int CHUNK = CHIRON_LOCATE_CHUNK;            // rows a launch, and the halo's columns
constexpr unsigned INF = 1u << 30;                    // a column without a path; every real cost is below it
constexpr unsigned BIAS = 32768;                      // samples and levels as unsigned: 1 .. 65535
constexpr unsigned BRK = INF + 2 * 65536;             // a break column's biased level: |x - BRK| > INF for every sample
static_assert(TILE == CHIRON_LOCATE_BLOCK, "a wave's owned columns are one block of the output");
static_assert(CHUNK == 64, "the halo is one column a lane");
static_assert(CHUNK == LOCATE_CHUNK && CHIRON_LOCATE_BLOCK == LOCATE_BLOCK && CHIRON_LOCATE_MAX_QUERY == LOCATE_MAX_QUERY, "header and pack agree");
static_assert(CHIRON_LOCATE_BREAK == LOCATE_BREAK && CHIRON_LOCATE_NONE == LOCATE_NONE, "header and pack agree");
static_assert(NT % 64 == 0, "whole waves");

struct LocateParams {
  const int16_t* samples;            // the call's samples
  const int64_t* sample_off;         // [items + 1], as the caller gave them: the kernel subtracts sample_off[0]
  const int32_t* level;              // [ref_len]
  const unsigned long long* prev;    // [items][stride]: the row before this launch's first (not read by launch 0)
  unsigned long long* next;          // [items][stride]: this launch's last row
  int32_t* block;                    // [items][tiles][3]
  int64_t items;
  int64_t stride;                    // columns of an item's row in the workspace: tiles * TILE
  int32_t ref_len;
  int32_t tiles;
  int32_t chunk;                     // this launch's rows: chunk * CHUNK ..
};

struct LocateLayout {
  size_t sample_off, samples, level, block, row[2], bytes;   // row: the two buffers
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

// |x - e| on top of a cost, cut back to INF: the cost is at most INF and the difference below 2^31, so nothing wraps
__device__ __forceinline__ unsigned add_to(unsigned cost, unsigned x, unsigned e) {
  const unsigned v = cost + (x > e ? x - e : e - x);
  return v < INF ? v : INF;
}

// One cell: the lexmin of k, the column's own pair of the row before, and kl, its left neighbour's, plus |x - e|.
__device__ __forceinline__ void cell(pair_t& k, pair_t kl, unsigned x, unsigned e) {
  const pair_t m = kl < k ? kl : k;
  k = pair_of(add_to((unsigned)(m >> 32), x, e), (int)m);
}

__device__ __forceinline__ unsigned biased(int32_t e) { return e == CHIRON_LOCATE_BREAK ? BRK : (unsigned)(e + (int)BIAS); }

__global__ __launch_bounds__(CHIRON_LOCATE_THREADS) void locate_kernel(LocateParams p) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t units = p.items * p.tiles;
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  const int row0 = p.chunk * CHUNK;
  for (int64_t u = (int64_t)blockIdx.x * WAVES + wv; u < units; u += nwaves) {
    const int64_t it = u / p.tiles;
    const int tile = (int)(u - it * p.tiles);
    const int64_t q64 = p.sample_off[it + 1] - p.sample_off[it];
    const int Q = (int)q64;
    if (row0 >= Q) continue;                                      // the item ended in an earlier launch
    const int rows = Q - row0 < CHUNK ? Q - row0 : CHUNK;
    const int16_t* __restrict__ x = p.samples + (p.sample_off[it] - p.sample_off[0]) + row0;
    const unsigned xv = lane < rows ? (unsigned)((int)x[lane] + (int)BIAS) : 0u;   // row r's sample on lane r
    const int col0 = tile * TILE + lane * COLS;                   // below 2^28 + 1024
    const int hcol = tile * TILE - CHUNK + lane;                  // this lane's halo column; below 0 left of the reference
    const int64_t at = it * p.stride + col0;
    const int64_t hat = it * p.stride + hcol;

    unsigned e[COLS];
    pair_t c[COLS];
#pragma unroll
    for (int k = 0; k < COLS; ++k) e[k] = col0 + k < p.ref_len ? biased(p.level[col0 + k]) : BRK;
    const unsigned he = hcol >= 0 ? biased(p.level[hcol]) : BRK;  // hcol < tile * TILE < ref_len
    pair_t hc;
    int first;                                                    // the first row this launch steps through
    if (p.chunk == 0) {                                           // row 0: every column starts its own path
      const unsigned x0 = (unsigned)__builtin_amdgcn_readlane((int)xv, 0);
#pragma unroll
      for (int k = 0; k < COLS; ++k) c[k] = pair_of(add_to(0, x0, e[k]), col0 + k);
      hc = pair_of(add_to(0, x0, he), hcol);
      first = 1;
    } else {
#pragma unroll
      for (int k = 0; k < COLS; ++k) c[k] = p.prev[at + k];
      hc = hcol >= 0 ? p.prev[hat] : pair_of(INF, 0);
      first = 0;
    }

    for (int r = first; r < rows; ++r) {
      const unsigned xr = (unsigned)__builtin_amdgcn_readlane((int)xv, r);
      const pair_t hin = shift_in(pair_of(INF, 0), hc);           // nothing comes into the halo's left end
      const pair_t hlast = pair_of((unsigned)__builtin_amdgcn_readlane((int)(hc >> 32), 63), __builtin_amdgcn_readlane((int)hc, 63));
      const pair_t in = shift_in(hlast, c[COLS - 1]);             // lane 0 takes the halo's last column
#pragma unroll
      for (int k = COLS - 1; k >= 1; --k) cell(c[k], c[k - 1], xr, e[k]);
      cell(c[0], in, xr, e[0]);
      cell(hc, hin, xr, he);
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

chiron_status locate_sizes(const char* who, int64_t items, int64_t samples, int64_t ref_len, LocateLayout* l) {
  if (items < 0 || samples < 0 || ref_len < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative size (items %lld, samples %lld, ref_len %lld)", who, (long long)items, (long long)samples,
                     (long long)ref_len);
  if (items > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items in one call, at most 2^31 - 1", who, (long long)items);
  if (samples > CHIRON_SIGNAL_MAX_SAMPLES)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld samples in one call, at most %d", who, (long long)samples, CHIRON_SIGNAL_MAX_SAMPLES);
  if (ref_len > CHIRON_LOCATE_MAX_REF)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: ref_len %lld, at most %d", who, (long long)ref_len, CHIRON_LOCATE_MAX_REF);
  l->tiles = locate_blocks(ref_len);
  l->stride = l->tiles * TILE;
  const int64_t cells = items * l->stride;                        // below 2^31 * (2^28 + 2^10): inside int64
  if (cells > CHIRON_LOCATE_MAX_CELLS)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items on %lld columns are %lld row cells, at most 2^40", who, (long long)items, (long long)ref_len,
                     (long long)cells);
  l->sample_off = 0;
  l->samples = l->sample_off + up256(items > 0 ? (size_t)(items + 1) * sizeof(int64_t) : 0);
  l->level = l->samples + up256((size_t)samples * sizeof(int16_t));
  l->block = l->level + up256((size_t)ref_len * sizeof(int32_t));
  l->row[0] = l->block + up256((size_t)(items * l->tiles) * 3 * sizeof(int32_t));
  l->row[1] = l->row[0] + up256((size_t)cells * sizeof(pair_t));
  l->bytes = l->row[1] + up256((size_t)cells * sizeof(pair_t));
  return CHIRON_OK;
}

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_signal_locate_workspace_size(int64_t items, int64_t samples, int64_t ref_len, size_t* bytes) {
  const char* who = "chiron_signal_locate_workspace_size";
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  LocateLayout l;
  if (chiron_status st = locate_sizes(who, items, samples, ref_len, &l)) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_signal_locate(int32_t device_id, const int16_t* samples, const int64_t* sample_off, int64_t items,
                                              const int32_t* ref_level, int64_t ref_len, int32_t* block_out, void* workspace,
                                              size_t workspace_bytes, uint32_t flags, void* stream_) {
  const char* who = "chiron_signal_locate";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  LocateLayout l;
  if (chiron_status st = locate_sizes(who, items, 0, ref_len, &l)) return st;
  if (items == 0) return CHIRON_OK;   // nothing to compute and nothing to write: no device is touched
  if (!sample_off || !samples) return set_error(CHIRON_ERR_INVALID, "%s: null samples / sample_off", who);
  if (ref_len > 0 && !ref_level) return set_error(CHIRON_ERR_INVALID, "%s: null ref_level", who);
  if (ref_len > 0 && !block_out) return set_error(CHIRON_ERR_INVALID, "%s: null block_out", who);
  int64_t longest = 0;
  LocateFinding f = locate_check_offsets(sample_off, items, &longest);
  if (f.fault == LOCATE_OFF_NEGATIVE) return set_error(CHIRON_ERR_INVALID, "%s: sample_off[0] = %lld is negative", who, (long long)f.value);
  if (f.fault == LOCATE_OFF_ORDER)
    return set_error(CHIRON_ERR_INVALID, "%s: sample_off[%lld] = %lld below its predecessor %lld", who, (long long)f.at, (long long)f.value,
                     (long long)sample_off[f.at - 1]);
  if (f.fault == LOCATE_QUERY_EMPTY) return set_error(CHIRON_ERR_INVALID, "%s: query %lld is empty", who, (long long)f.at);
  if (f.fault == LOCATE_QUERY_LONG)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: query %lld has %lld samples, at most %d", who, (long long)f.at, (long long)f.value, CHIRON_LOCATE_MAX_QUERY);
  const int64_t n_samples = sample_off[items] - sample_off[0];
  if (chiron_status st = locate_sizes(who, items, n_samples, ref_len, &l)) return st;
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
  if (hipMemcpyAsync(ws + l.sample_off, sample_off, (size_t)(items + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.samples, samples + sample_off[0], (size_t)n_samples * sizeof(int16_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.level, ref_level, (size_t)ref_len * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the queries and the reference to the device failed", who);
  LocateParams p;
  p.samples = (const int16_t*)(ws + l.samples);
  p.sample_off = (const int64_t*)(ws + l.sample_off);
  p.level = (const int32_t*)(ws + l.level);
  p.block = (int32_t*)(ws + l.block);
  p.items = items;
  p.stride = l.stride;
  p.ref_len = (int32_t)ref_len;
  p.tiles = (int32_t)l.tiles;
  const int64_t want = (items * l.tiles + WAVES - 1) / WAVES;
  const dim3 grid((unsigned)(want < CHIRON_LOCATE_MAX_GROUPS ? want : CHIRON_LOCATE_MAX_GROUPS));
  const int64_t launches = locate_launches(longest);
  for (int64_t k = 0; k < launches; ++k) {   // launch k writes buffer k & 1 and reads the other
    p.next = (pair_t*)(ws + l.row[k & 1]);
    p.prev = (const pair_t*)(ws + l.row[1 - (k & 1)]);
    p.chunk = (int32_t)k;
    hipLaunchKernelGGL(locate_kernel, grid, dim3(NT), 0, stream, p);
    if (chiron_status st = launched(who)) return st;
  }
  if (hipMemcpyAsync(block_out, ws + l.block, (size_t)(items * l.tiles) * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the locate kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  return CHIRON_OK;
}
