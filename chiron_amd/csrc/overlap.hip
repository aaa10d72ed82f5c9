// Read-to-read overlaps on gfx950: dovetail alignment of two reads inside a band of diagonals the caller gives, cost 2 E - M,
// exact (cost, M, s, e) per pair.
//
//   over every path through the (n+1) x (m+1) table that starts on row 0 or on column 0, ends on row n or on column m and stays
//   on the diagonals d = j - i of [dlo, dhi]: smallest cost 2 E - M, then most matching columns M, then smallest start s, then
//   smallest end e, s and e being the boundary cell's diagonal plus n                                      (include/chiron_amd.h)
//
// Under unit cost the empty overlap (cost 0 at a corner) would always win; with a match at -1 and every other move at +2 the
// score M - 2 E rises along any stretch of identity above 2/3.  The band is part of the definition: an overlap on a diagonal
// outside it is another path, which nothing computed inside the band can exclude, so there is no certificate and no widening
// here.  The caller chooses the band and owns the rule that widens it (chiron_amd/overlap.py).
//
// A cell is the lexicographic minimum of (cost, -M, s) over the paths that reach it, in one signed 64-bit key:
//   key = cost * 2^40 - M * 2^20 + (d0 + 2^17),   d0 the diagonal of the path's start cell, s = d0 + n
// A read has at most 2^17 bases (checked on the host, CHIRON_ERR_OVERFLOW), so 0 <= d0 + 2^17 <= 2^18 < 2^20 and M <= 2^17 < 2^20:
// the start never borrows from M's field and -M * 2^20 + start, within (-2^38, 2^19), never from the cost's; a path has at most
// n + m <= 2^18 moves, so -2^17 <= cost <= 2^19 and every key of a reached cell lies within (-2^58, 2^60), far below the 2^62 of a
// cell no path reaches.  The bias 2^17 stands for n, which differs from pair to pair, so that the cell policy needs no argument:
// it orders the starts as s does.  A match adds -2^40 - 2^20, any other move 2^41; both leave the start alone, so the step added
// to two prefixes keeps their order and the three-way min of the keys is exact (map.hip's scheme with a signed cost).
//
// Sweep: align_common.h's band_sweep under OverlapCell, unchanged.  border() gives the cells of row 0 AND of column 0 the key of
// a start (cost 0, M 0, their own diagonal).  FREE_ROW0 stays off: the sweep then also tries the move along the border into
// such a cell, which comes from another start at cost 0 and adds 2, so the border's own key always wins -- no switch is needed.
// Every value a cell reads was written by this pair: (i-1, j-1), (i-1, j) and (i, j-1) are read only when they lie in the table
// and, by the d < dhi and d > dlo guards, in the band, so what an earlier pair of the workgroup left in the row is never seen.
//
// End: the last cell of diagonal d is (n, n + d) for d <= m - n and (m - d, m) above, a boundary end cell either way, and e = n + d
// for both.  After the sweep EVERY slot of the row is such an end, and the result is the smallest (key, e) over the whole band:
// a scan per thread, then an LDS tree.
//
// Work mapping: one workgroup of 256 threads a pair, pair p on workgroup p mod the group count (at most 2048), one barrier per
// anti-diagonal, n + m + 1 of them; the row lives in LDS while the band has at most CHIRON_ALIGN_LDS_SLOTS diagonals and in the
// workgroup's workspace row beyond.  64-bit offsets, no atomics; a pair's result depends on that pair alone.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "kernels.h"

namespace chiron {

namespace {

constexpr int64_t OVL_COST = (int64_t)1 << 40;      // one unit of cost
constexpr int64_t OVL_MATCH = (int64_t)1 << 20;     // one match, subtracted
constexpr int64_t OVL_INF = (int64_t)1 << 62;
constexpr int OVL_BIAS = CHIRON_OVERLAP_MAX_READ;   // added to a start's diagonal: the key's lowest field is never negative
constexpr int NT = CHIRON_ALIGN_THREADS;
static_assert(CHIRON_OVERLAP_MAX_READ == (1 << 17) && 2 * CHIRON_OVERLAP_MAX_READ < OVL_MATCH, "the key's fields: start and M below 2^20");

struct OverlapCell {
  static constexpr int64_t EDIT = 2 * OVL_COST, MATCH = -OVL_COST - OVL_MATCH;
  static constexpr bool FREE_ROW0 = false;
  // row 0 and column 0: a start at cost 0 on its own diagonal j - i
  __device__ static int64_t border(int, int i, int j) { return (i == 0 || j == 0) ? (int64_t)(j - i + OVL_BIAS) : OVL_INF; }
};

// one pass over the band [dlo, dhi] (inside -n .. m); leaves the smallest (key, e) of the band's end cells in red_key[0], red_end[0]
__device__ __forceinline__ void overlap_pass(int64_t* row, int64_t* red_key, int* red_end, const uint8_t* __restrict__ a,
                                             const uint8_t* __restrict__ b, int n, int m, int dlo, int dhi) {
  const int tid = threadIdx.x;
  band_sweep<OverlapCell>(row, a, b, n, m, dlo, dhi);
  int64_t bk = OVL_INF;
  int be = 0;
  for (int d = dlo + tid; d <= dhi; d += NT) {       // each thread meets its e in rising order
    const int64_t key = row[d - dlo];
    if (key < bk) {
      bk = key;
      be = n + d;
    }
  }
  red_key[tid] = bk;
  red_end[tid] = be;
  __syncthreads();
  for (int step = NT / 2; step > 0; step >>= 1) {
    if (tid < step) {
      const int64_t ok = red_key[tid + step];
      const int oe = red_end[tid + step];
      if (ok < red_key[tid] || (ok == red_key[tid] && oe < red_end[tid])) {
        red_key[tid] = ok;
        red_end[tid] = oe;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(CHIRON_ALIGN_THREADS) void overlap_kernel(OverlapParams p) {
  __shared__ int64_t lds_row[CHIRON_ALIGN_LDS_SLOTS];
  __shared__ int64_t red_key[CHIRON_ALIGN_THREADS];
  __shared__ int red_end[CHIRON_ALIGN_THREADS];
  int64_t* const ws_row = p.rows ? p.rows + (int64_t)blockIdx.x * p.row_slots : nullptr;
  for (int64_t q = blockIdx.x; q < p.pairs; q += gridDim.x) {
    const OverlapPair pr = p.pair[q];
    const int n = pr.n, m = pr.m;
    const bool fits = with_row(lds_row, ws_row, pr.dhi - pr.dlo + 1, p.row_slots, [&](int64_t* row) {
      overlap_pass(row, red_key, red_end, p.codes + pr.a, p.codes + pr.b, n, m, pr.dlo, pr.dhi);
    });
    if (threadIdx.x == 0) {
      int cost = 0, M = 0, S = 0, End = 0;
      if (fits) {
        const int64_t key = red_key[0];
        cost = (int)((key + (OVL_COST >> 1)) >> 40);             // arithmetic shift: the floor, for a negative cost too
        const int64_t rem = (int64_t)cost * OVL_COST - key;      // M * 2^20 - start, 0 <= start < 2^20
        M = (int)((rem + OVL_MATCH - 1) >> 20);
        S = (int)((int64_t)M * OVL_MATCH - rem) - OVL_BIAS + n;
        End = red_end[0];
      }
      p.out[q * 5 + 0] = cost;
      p.out[q * 5 + 1] = M;
      p.out[q * 5 + 2] = S;
      p.out[q * 5 + 3] = End;
      p.out[q * 5 + 4] = fits ? 0 : 1;
    }
    __syncthreads();   // thread 0 has read the result before the next pair writes the arrays
  }
}

// byte offsets of the workspace's parts and its size
struct OverlapLayout {
  size_t pair, out, codes, rows, bytes;
  int64_t row_slots;
  int groups;
};

chiron_status overlap_layout(const char* who, int64_t reads, int64_t total_bases, int64_t pairs, int64_t max_band, OverlapLayout* l) {
  if (reads < 0 || total_bases < 0 || pairs < 0 || max_band < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative reads / total_bases / pairs / max_band", who);
  if (pairs > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld pairs in one call, at most 2^24", who, (long long)pairs);
  if (reads > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld reads in one call, at most 2^24", who, (long long)reads);
  if (total_bases > reads * (int64_t)CHIRON_OVERLAP_MAX_READ)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld bases in %lld reads, a read has at most %d", who, (long long)total_bases, (long long)reads,
                     CHIRON_OVERLAP_MAX_READ);
  if (max_band > 2 * (int64_t)CHIRON_OVERLAP_MAX_READ + 1)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: a band of %lld diagonals, the largest table has %d", who, (long long)max_band,
                     2 * CHIRON_OVERLAP_MAX_READ + 1);
  // pairs, reads <= 2^24, total_bases <= 2^41, max_band < 2^19: every product below stays under 2^48
  l->groups = (int)(pairs < CHIRON_ALIGN_MAX_GROUPS ? pairs : CHIRON_ALIGN_MAX_GROUPS);
  l->row_slots = max_band > CHIRON_ALIGN_LDS_SLOTS ? max_band : 0;
  l->pair = 0;
  l->out = l->pair + up256((size_t)pairs * sizeof(OverlapPair));
  l->codes = l->out + up256((size_t)pairs * 5 * sizeof(int32_t));
  l->rows = l->codes + up256((size_t)total_bases);
  l->bytes = l->rows + up256((size_t)l->groups * (size_t)l->row_slots * sizeof(int64_t));
  return CHIRON_OK;
}

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_align_overlap_workspace_size(int64_t reads, int64_t total_bases, int64_t pairs, int64_t max_band, size_t* bytes) {
  const char* const who = "chiron_align_overlap_workspace_size";
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  OverlapLayout l;
  if (chiron_status st = overlap_layout(who, reads, total_bases, pairs, max_band, &l)) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_align_overlap(int32_t device_id, const uint8_t* codes, const int64_t* read_off, int64_t reads,
                                              const int32_t* pair_a, const int32_t* pair_b, const int32_t* dlo, const int32_t* dhi, int64_t pairs,
                                              int32_t* out, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream_) {
  const char* const who = "chiron_align_overlap";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  if (reads < 0 || pairs < 0) return set_error(CHIRON_ERR_INVALID, "%s: negative count (reads %lld, pairs %lld)", who, (long long)reads, (long long)pairs);
  if (pairs == 0) return CHIRON_OK;
  if (pairs > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld pairs in one call, at most 2^24", who, (long long)pairs);
  if (reads > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld reads in one call, at most 2^24", who, (long long)reads);
  if (!read_off) return set_error(CHIRON_ERR_INVALID, "%s: null read_off", who);
  if (!pair_a || !pair_b || !dlo || !dhi) return set_error(CHIRON_ERR_INVALID, "%s: null pair_a / pair_b / dlo / dhi", who);
  if (!out) return set_error(CHIRON_ERR_INVALID, "%s: null out", who);
  // offsets first (they bound what may be read of `codes`), then the codes, then the pairs against the reads' lengths
  int64_t max_read = 0, total = 0;
  if (chiron_status st = check_offsets(who, "read", "read", "bases", read_off, reads, CHIRON_OVERLAP_MAX_READ, &max_read, &total)) return st;
  if (total > 0 && !codes) return set_error(CHIRON_ERR_INVALID, "%s: null codes", who);
  const int64_t base0 = read_off[0];
  int64_t r = 0;
  for (int64_t i = 0; i < total; ++i) {
    const uint8_t c = codes[base0 + i];
    if (c > 4) {
      while (read_off[r + 1] - base0 <= i) ++r;
      return set_error(CHIRON_ERR_INVALID, "%s: code %d at %lld of read %lld outside 0..4", who, (int)c, (long long)(base0 + i - read_off[r]), (long long)r);
    }
  }
  std::vector<OverlapPair> recs((size_t)pairs);
  int64_t max_band = 0;
  for (int64_t q = 0; q < pairs; ++q) {
    const int64_t ia = pair_a[q], ib = pair_b[q];
    if (ia < 0 || ia >= reads || ib < 0 || ib >= reads)
      return set_error(CHIRON_ERR_INVALID, "%s: pair %lld names reads %lld and %lld, the call has %lld", who, (long long)q, (long long)ia, (long long)ib,
                       (long long)reads);
    OverlapPair& pr = recs[(size_t)q];
    pr.a = read_off[ia] - base0;
    pr.b = read_off[ib] - base0;
    pr.n = (int32_t)(read_off[ia + 1] - read_off[ia]);
    pr.m = (int32_t)(read_off[ib + 1] - read_off[ib]);
    pr.dlo = imax(dlo[q], -pr.n);
    pr.dhi = imin(dhi[q], pr.m);
    if (pr.dlo > pr.dhi)
      return set_error(CHIRON_ERR_INVALID, "%s: pair %lld: the band %d .. %d holds no diagonal of the table's %d .. %d", who, (long long)q, dlo[q], dhi[q],
                       -pr.n, pr.m);
    const int64_t band = (int64_t)pr.dhi - pr.dlo + 1;
    if (band > max_band) max_band = band;
  }
  OverlapLayout l;
  if (chiron_status st = overlap_layout(who, reads, total, pairs, max_band, &l)) return st;
  if (workspace_bytes < l.bytes)
    return set_error(CHIRON_ERR_INVALID, "%s: a workspace of %zu bytes, %zu are needed", who, workspace_bytes, l.bytes);
  if (chiron_status st = use_device_workspace(who, device_id, workspace)) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.pair, recs.data(), recs.size() * sizeof(OverlapPair), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (total > 0 && hipMemcpyAsync(ws + l.codes, codes + base0, (size_t)total, hipMemcpyHostToDevice, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the pairs to the device failed", who);
  OverlapParams p;
  p.codes = (const uint8_t*)(ws + l.codes);
  p.pair = (const OverlapPair*)(ws + l.pair);
  p.pairs = pairs;
  p.rows = l.row_slots ? (int64_t*)(ws + l.rows) : nullptr;
  p.row_slots = l.row_slots;
  p.out = (int32_t*)(ws + l.out);
  hipLaunchKernelGGL(overlap_kernel, dim3(l.groups), dim3(CHIRON_ALIGN_THREADS), 0, stream, p);
  if (chiron_status st = launched(who)) return st;
  std::vector<int32_t> got((size_t)pairs * 5);
  if (hipMemcpyAsync(got.data(), ws + l.out, got.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the overlap kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  for (int64_t q = 0; q < pairs; ++q)
    if (got[(size_t)q * 5 + 4] != 0) return set_error(CHIRON_ERR_STATE, "%s: pair %lld outgrew its workspace row", who, (long long)q);
  for (size_t i = 0; i < got.size(); ++i) out[i] = got[i];
  return CHIRON_OK;
}
