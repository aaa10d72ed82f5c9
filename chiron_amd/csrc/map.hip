// Read mapping on gfx950: infix (semi-global) alignment of a read against the best substring of a genome window, unit costs,
// exact (E, M, s, e) per pair.
//
//   over every substring b[s:e) of the window and every global alignment of the read a against it: smallest edit cost E, then
//   most matching columns M, then smallest s, then smallest e                                               (include/chiron_amd.h)
//
// A cell is the lexicographic minimum of (E, -M, s) over the paths that reach it, in one 64-bit key:
//   key = E * 2^40 - M * 2^20 + s,   M < 2^20 and s < 2^20  (read <= 2^17 bases, window <= 2^20 - 1 bases, checked on the host)
// so -M * 2^20 + s never borrows from E's field, s never from M's, and E <= n + m < 2^21 keeps every key under 2^61.  Row 0 is
// free: cell (0, j) = (0, 0, s = j).  Column 0 is cell (i, 0) = (i, 0, 0).  A match adds -2^20, a mismatch or a gap 2^40; both
// leave s alone, so the step added to two prefixes keeps their order and the three-way min of the keys is exact.
//
// Work mapping: as assess.hip, the same sweep (align_common.h, band_sweep) under another cell policy: one workgroup per pair, an
// anti-diagonal wavefront over a band of diagonals d = j - i in [min(0, m-n) - w, max(0, m-n) + w], one array indexed by d, one
// barrier per step; the array lives in LDS while the band has at most CHIRON_INFIX_LDS_SLOTS diagonals and in the workgroup's
// workspace row beyond that.
//
// End: the last cell of a diagonal d <= m - n is (n, n + d), and nothing overwrites its slot afterwards, so after the sweep the
// array holds row n for e = n + d.  The result is the smallest (key, e) over those slots.  Diagonals above m - n end on column m,
// not on row n, and take no part.
//
// Exactness: a path starts on row 0, on a diagonal s >= 0, and ends on row n, on a diagonal e - n <= m - n; only a gap changes
// the diagonal, by one, at cost one.  A path that touches diagonal max(0, m-n) + w + 1 has to come down to m - n or below: at
// least w + 1 gaps.  A path that touches diagonal min(0, m-n) - w - 1 started at 0 or above: at least w + 1 gaps.  That includes
// the paths that START above the band (row-0 cells beyond its upper edge).  So every alignment of cost <= w lies inside the
// band, and when the banded result has E <= w it is the true E, every alignment of that cost was seen, and M, s, e are exact for
// the whole window.  Otherwise w doubles and the pair is redone, up to the full table, which is always accepted; all inside the
// kernel, so a batch is one launch.  (The certificate is E <= w, not assess.hip's 2w + 1 + |m-n|: a global path must leave AND
// come back between fixed ends, an infix path's ends are free within [0, m-n].)
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "kernels.h"

namespace chiron {

namespace {

constexpr int64_t INFIX_EDIT = (int64_t)1 << 40;    // one mismatch or gap
constexpr int64_t INFIX_MATCH = (int64_t)1 << 20;   // one match, subtracted
constexpr int64_t INFIX_INF = (int64_t)1 << 62;
constexpr int NT = CHIRON_INFIX_THREADS;
static_assert(CHIRON_INFIX_MAX_GROUPS == CHIRON_ALIGN_MAX_GROUPS, "pair_layout sizes the rows of both kernels");

struct InfixCell {
  static constexpr int64_t EDIT = INFIX_EDIT, MATCH = -INFIX_MATCH;
  static constexpr bool FREE_ROW0 = true;
  __device__ static int64_t border(int, int i, int j) { return i == 0 ? (int64_t)j : INFIX_INF; }   // row 0: a free start at s = j, cost 0
};

// one pass over the band [dlo, dhi] (already clipped to the table's diagonals -n .. m); returns the smallest (key, e) of row n
__device__ __forceinline__ void band_pass(int64_t* row, int64_t* red_key, int* red_end, const uint8_t* __restrict__ a,
                                          const uint8_t* __restrict__ b, int n, int m, int dlo, int dhi, int64_t* key_out, int* end_out) {
  const int tid = threadIdx.x;
  band_sweep<InfixCell>(row, a, b, n, m, dlo, dhi);
  // row n: slots of the diagonals dlo .. m - n, e = n + d; smallest key, then smallest e (each thread meets its e in rising order)
  int64_t bk = INFIX_INF;
  int be = 0;
  for (int d = dlo + tid; d <= m - n; d += NT) {
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
  *key_out = red_key[0];
  *end_out = red_end[0];
  __syncthreads();   // every thread has read the result before the next pass writes the arrays
}

__global__ __launch_bounds__(CHIRON_INFIX_THREADS) void infix_kernel(AlignParams p) {
  __shared__ int64_t lds_row[CHIRON_INFIX_LDS_SLOTS];
  __shared__ int64_t red_key[CHIRON_INFIX_THREADS];
  __shared__ int red_end[CHIRON_INFIX_THREADS];
  int64_t* const ws_row = p.rows ? p.rows + (int64_t)blockIdx.x * p.row_slots : nullptr;
  for (int64_t q = blockIdx.x; q < p.pairs; q += gridDim.x) {
    const AlignPair pr = p.pair[q];
    const int n = pr.n, m = pr.m;
    const uint8_t* a = p.codes + pr.start;
    const uint8_t* b = a + n;
    int w = p.band0;
    int E, M, S, End;
    for (;;) {
      const Diagonals bd = p.band0 == 0 ? Diagonals{-n, m} : band_clip(n, m, w);
      const bool full = bd.dlo == -n && bd.dhi == m;
      int64_t key;
      const bool fits = with_row(lds_row, ws_row, bd.dhi - bd.dlo + 1, p.row_slots,
                                 [&](int64_t* row) { band_pass(row, red_key, red_end, a, b, n, m, bd.dlo, bd.dhi, &key, &End); });
      if (!fits) {
        E = -1;
        M = S = End = 0;
        break;
      }
      E = (int)((key + (INFIX_EDIT >> 1)) >> 40);
      const int64_t rem = (int64_t)E * INFIX_EDIT - key;       // M * 2^20 - s, 0 <= s < 2^20
      M = (int)((rem + INFIX_MATCH - 1) >> 20);
      S = (int)((int64_t)M * INFIX_MATCH - rem);
      if (full || E <= w) break;
      w *= 2;
    }
    if (threadIdx.x == 0) {
      p.out[q * 5 + 0] = E;
      p.out[q * 5 + 1] = M;
      p.out[q * 5 + 2] = S;
      p.out[q * 5 + 3] = End;
      p.out[q * 5 + 4] = w;
    }
  }
}

}  // namespace

chiron_status infix_layout(int64_t pairs, int64_t max_read, int64_t max_window, AlignLayout* l) {
  if (pairs < 0 || max_read < 0 || max_window < 0) return set_error(CHIRON_ERR_INVALID, "align_infix: negative pairs / max_read / max_window");
  if (max_read > CHIRON_INFIX_MAX_READ)
    return set_error(CHIRON_ERR_OVERFLOW, "align_infix: a read of %lld bases, the kernel takes at most %d", (long long)max_read, CHIRON_INFIX_MAX_READ);
  if (max_window > CHIRON_INFIX_MAX_WINDOW)
    return set_error(CHIRON_ERR_OVERFLOW, "align_infix: a window of %lld bases, the kernel takes at most %d", (long long)max_window,
                     CHIRON_INFIX_MAX_WINDOW);
  if (pairs > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "align_infix: %lld pairs in one call, at most 2^24", (long long)pairs);
  pair_layout(pairs, max_read + max_window, 5, max_read + max_window + 1, l);
  return CHIRON_OK;
}

int launch_infix(const AlignParams& p, int groups, hipStream_t stream) {
  if (p.pairs <= 0) return 0;
  hipLaunchKernelGGL(infix_kernel, dim3(groups), dim3(CHIRON_INFIX_THREADS), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_align_infix_workspace_size(int64_t pairs, int64_t max_read, int64_t max_window, size_t* bytes) {
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "chiron_align_infix_workspace_size: null bytes");
  AlignLayout l;
  chiron_status st = infix_layout(pairs, max_read, max_window, &l);
  if (st) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_align_infix(int32_t device_id, const uint8_t* codes, const int64_t* read_off, const int64_t* win_off,
                                            int64_t pairs, int32_t band0, uint32_t flags, int32_t* edit_out, int32_t* match_out,
                                            int32_t* start_out, int32_t* end_out, int32_t* band_out, void* workspace, void* stream_) {
  const char* const who = "chiron_align_infix";
  if (pairs < 0) return set_error(CHIRON_ERR_INVALID, "%s: pairs %lld", who, (long long)pairs);
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  if (band0 < 0) return set_error(CHIRON_ERR_INVALID, "%s: band0 %d is negative", who, band0);
  if (band0 > CHIRON_INFIX_MAX_WINDOW)
    return set_error(CHIRON_ERR_INVALID, "%s: band0 %d above the longest window, %d (0 asks for the full table)", who, band0, CHIRON_INFIX_MAX_WINDOW);
  if (pairs == 0) return CHIRON_OK;
  if (pairs > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld pairs in one call, at most 2^24", who, (long long)pairs);
  if (!read_off || !win_off || !edit_out || !match_out || !start_out || !end_out || !band_out)
    return set_error(CHIRON_ERR_INVALID, "%s: null operand", who);
  // offsets first (they bound what may be read of `codes`), then the codes while they are packed pair by pair
  int64_t max_read = 0, max_window = 0, total = 0;
  chiron_status st = check_offsets(who, "read", "read", "bases", read_off, pairs, CHIRON_INFIX_MAX_READ, &max_read, &total);
  if (!st) st = check_offsets(who, "win", "window", "bases", win_off, pairs, CHIRON_INFIX_MAX_WINDOW, &max_window, &total);
  if (st) return st;
  if (total > 0 && !codes) return set_error(CHIRON_ERR_INVALID, "%s: null codes", who);
  std::vector<uint8_t> packed((size_t)total);
  std::vector<AlignPair> recs((size_t)pairs);
  AlignLayout l;
  if ((st = pack_codes(who, "read", "window", codes, read_off, win_off, pairs, recs.data(), packed.data()))) return st;
  if ((st = infix_layout(pairs, max_read, max_window, &l))) return st;
  if ((st = use_device_workspace(who, device_id, workspace))) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.pair, recs.data(), recs.size() * sizeof(AlignPair), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (total > 0 && hipMemcpyAsync(ws + l.codes, packed.data(), packed.size(), hipMemcpyHostToDevice, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the pairs to the device failed", who);
  if (launch_infix(align_params(workspace, l, pairs, band0), l.groups, stream) != 0) return set_error(CHIRON_ERR_DEVICE, "%s: launch failed", who);
  std::vector<int32_t> out((size_t)pairs * 5);
  if (hipMemcpyAsync(out.data(), ws + l.out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the alignment kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  for (int64_t q = 0; q < pairs; ++q) {
    if (out[q * 5] < 0) return set_error(CHIRON_ERR_STATE, "%s: pair %lld outgrew its workspace row", who, (long long)q);
    edit_out[q] = out[q * 5];
    match_out[q] = out[q * 5 + 1];
    start_out[q] = out[q * 5 + 2];
    end_out[q] = out[q * 5 + 3];
    band_out[q] = out[q * 5 + 4];
  }
  return CHIRON_OK;
}
