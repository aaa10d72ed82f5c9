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
// Work mapping: as assess.hip.  One workgroup per pair, an anti-diagonal wavefront over a band of diagonals d = j - i in
// [min(0, m-n) - w, max(0, m-n) + w], the last three anti-diagonals in ONE array indexed by d (step k rewrites the slots of k's
// parity in place and reads the other parity's), one barrier per step; the array lives in LDS while the band has at most
// CHIRON_INFIX_LDS_SLOTS diagonals and in the workgroup's workspace row beyond that.
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

#include <cstring>
#include <vector>

#include "../../include/chiron_amd.h"
#include "kernels.h"

namespace chiron {

chiron_status set_error(chiron_status st, const char* fmt, ...);   // engine.hip

namespace {

constexpr int64_t INFIX_EDIT = (int64_t)1 << 40;    // one mismatch or gap
constexpr int64_t INFIX_MATCH = (int64_t)1 << 20;   // one match, subtracted
constexpr int64_t INFIX_INF = (int64_t)1 << 62;
constexpr int NT = CHIRON_INFIX_THREADS;

__device__ inline int imax(int a, int b) { return a > b ? a : b; }
__device__ inline int imin(int a, int b) { return a < b ? a : b; }

// one pass over the band [dlo, dhi] (already clipped to the table's diagonals -n .. m); returns the smallest (key, e) of row n
__device__ __forceinline__ void band_pass(int64_t* row, int64_t* red_key, int* red_end, const uint8_t* __restrict__ a,
                                          const uint8_t* __restrict__ b, int n, int m, int dlo, int dhi, int64_t* key_out, int* end_out) {
  const int tid = threadIdx.x;
  for (int k = 0; k <= n + m; ++k) {
    // the anti-diagonal's cells inside the table and the band: 0 <= i = (k-d)/2 <= n, 0 <= j = (k+d)/2 <= m
    const int lo = imax(imax(dlo, -k), k - 2 * n);
    const int hi = imin(imin(dhi, k), 2 * m - k);
    const int first = lo + ((lo + k) & 1);
    for (int d = first + 2 * tid; d <= hi; d += 2 * NT) {
      const int i = (k - d) >> 1, j = (k + d) >> 1;
      const int s = d - dlo;
      int64_t best = i == 0 ? (int64_t)j : INFIX_INF;      // row 0: a free start at s = j, cost 0
      if (i > 0) {
        if (j > 0) {
          const uint8_t ca = a[i - 1], cb = b[j - 1];
          best = row[s] + ((ca == cb && ca < 4) ? -INFIX_MATCH : INFIX_EDIT);
        }
        if (d < dhi) {
          const int64_t up = row[s + 1] + INFIX_EDIT;
          best = up < best ? up : best;
        }
        if (j > 0 && d > dlo) {
          const int64_t left = row[s - 1] + INFIX_EDIT;
          best = left < best ? left : best;
        }
      }
      row[s] = best;
    }
    __syncthreads();
  }
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

__global__ __launch_bounds__(CHIRON_INFIX_THREADS) void infix_kernel(InfixParams p) {
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
      const int dlo = p.band0 == 0 ? -n : imax((m < n ? m - n : 0) - w, -n);
      const int dhi = p.band0 == 0 ? m : imin((m > n ? m - n : 0) + w, m);
      const bool full = dlo == -n && dhi == m;
      const int slots = dhi - dlo + 1;
      // the host sized the row for the full table of the call's longest read and window; a pair that would not fit cannot
      // occur, and is answered with E = -1 rather than with a write past the row
      int64_t key;
      if (slots <= CHIRON_INFIX_LDS_SLOTS) {
        band_pass(lds_row, red_key, red_end, a, b, n, m, dlo, dhi, &key, &End);
      } else if (ws_row && slots <= p.row_slots) {
        band_pass(ws_row, red_key, red_end, a, b, n, m, dlo, dhi, &key, &End);
      } else {
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

chiron_status infix_layout(int64_t pairs, int64_t max_read, int64_t max_window, InfixLayout* l) {
  if (pairs < 0 || max_read < 0 || max_window < 0) return set_error(CHIRON_ERR_INVALID, "align_infix: negative pairs / max_read / max_window");
  if (max_read > CHIRON_INFIX_MAX_READ)
    return set_error(CHIRON_ERR_OVERFLOW, "align_infix: a read of %lld bases, the kernel takes at most %d", (long long)max_read, CHIRON_INFIX_MAX_READ);
  if (max_window > CHIRON_INFIX_MAX_WINDOW)
    return set_error(CHIRON_ERR_OVERFLOW, "align_infix: a window of %lld bases, the kernel takes at most %d", (long long)max_window,
                     CHIRON_INFIX_MAX_WINDOW);
  if (pairs > ((int64_t)1 << 24)) return set_error(CHIRON_ERR_OVERFLOW, "align_infix: %lld pairs in one call, at most 2^24", (long long)pairs);
  // pairs <= 2^24, max_read + max_window < 2^21: every product below stays under 2^48
  const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const int64_t table = max_read + max_window + 1;             // diagonals of the full table
  l->groups = (int)(pairs < CHIRON_INFIX_MAX_GROUPS ? pairs : CHIRON_INFIX_MAX_GROUPS);
  l->row_slots = table > CHIRON_INFIX_LDS_SLOTS ? table + 1 : 0;
  l->pair = 0;
  l->out = l->pair + up((size_t)pairs * sizeof(AlignPair));
  l->codes = l->out + up((size_t)pairs * 5 * sizeof(int32_t));
  l->rows = l->codes + up((size_t)pairs * (size_t)(max_read + max_window));
  l->bytes = l->rows + up((size_t)l->groups * (size_t)l->row_slots * sizeof(int64_t));
  return CHIRON_OK;
}

int launch_infix(const InfixParams& p, int groups, hipStream_t stream) {
  if (p.pairs <= 0) return 0;
  hipLaunchKernelGGL(infix_kernel, dim3(groups), dim3(CHIRON_INFIX_THREADS), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_align_infix_workspace_size(int64_t pairs, int64_t max_read, int64_t max_window, size_t* bytes) {
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "chiron_align_infix_workspace_size: null bytes");
  InfixLayout l;
  chiron_status st = infix_layout(pairs, max_read, max_window, &l);
  if (st) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_align_infix(int32_t device_id, const uint8_t* codes, const int64_t* read_off, const int64_t* win_off,
                                            int64_t pairs, int32_t band0, uint32_t flags, int32_t* edit_out, int32_t* match_out,
                                            int32_t* start_out, int32_t* end_out, int32_t* band_out, void* workspace, void* stream_) {
  if (pairs < 0) return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: pairs %lld", (long long)pairs);
  if (flags) return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: unknown flags 0x%x", flags);
  if (band0 < 0) return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: band0 %d is negative", band0);
  if (band0 > CHIRON_INFIX_MAX_WINDOW)
    return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: band0 %d above the longest window, %d (0 asks for the full table)", band0,
                     CHIRON_INFIX_MAX_WINDOW);
  if (pairs == 0) return CHIRON_OK;
  if (pairs > ((int64_t)1 << 24)) return set_error(CHIRON_ERR_OVERFLOW, "chiron_align_infix: %lld pairs in one call, at most 2^24", (long long)pairs);
  if (!read_off || !win_off || !edit_out || !match_out || !start_out || !end_out || !band_out)
    return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: null operand");
  // offsets first (they bound what may be read of `codes`), then the codes while they are packed pair by pair
  int64_t max_len[2] = {0, 0}, total = 0;
  for (int which = 0; which < 2; ++which) {
    const int64_t* off = which ? win_off : read_off;
    const int64_t limit = which ? CHIRON_INFIX_MAX_WINDOW : CHIRON_INFIX_MAX_READ;
    if (off[0] < 0) return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: %s_off[0] = %lld is negative", which ? "win" : "read", (long long)off[0]);
    for (int64_t q = 0; q < pairs; ++q) {
      if (off[q + 1] < off[q])
        return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: %s_off[%lld] = %lld below its predecessor %lld", which ? "win" : "read",
                         (long long)(q + 1), (long long)off[q + 1], (long long)off[q]);
      const int64_t len = off[q + 1] - off[q];
      if (len > limit)
        return set_error(CHIRON_ERR_OVERFLOW, "chiron_align_infix: %s %lld has %lld bases, at most %lld", which ? "window" : "read",
                         (long long)q, (long long)len, (long long)limit);
      if (len > max_len[which]) max_len[which] = len;
      total += len;
    }
  }
  if (total > 0 && !codes) return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: null codes");
  std::vector<uint8_t> packed((size_t)total);
  std::vector<AlignPair> recs((size_t)pairs);
  int64_t at = 0;
  for (int64_t q = 0; q < pairs; ++q) {
    recs[q].start = at;
    recs[q].n = (int32_t)(read_off[q + 1] - read_off[q]);
    recs[q].m = (int32_t)(win_off[q + 1] - win_off[q]);
    for (int which = 0; which < 2; ++which) {
      const int64_t lo = which ? win_off[q] : read_off[q], len = which ? recs[q].m : recs[q].n;
      for (int64_t i = 0; i < len; ++i) {
        const uint8_t c = codes[lo + i];
        if (c > 4)
          return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: code %d at %lld of %s %lld outside 0..4", (int)c, (long long)i,
                           which ? "window" : "read", (long long)q);
        packed[(size_t)(at + i)] = c;
      }
      at += len;
    }
  }
  InfixLayout l;
  chiron_status st = infix_layout(pairs, max_len[0], max_len[1], &l);
  if (st) return st;
  if (!workspace) return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: null workspace");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) {
    (void)hipGetLastError();
    return set_error(CHIRON_ERR_DEVICE, "no HIP device %d: libchiron_amd has no CPU fallback", device_id);
  }
  if (hipSetDevice(device_id) != hipSuccess) return set_error(CHIRON_ERR_DEVICE, "hipSetDevice(%d) failed", device_id);
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, workspace) != hipSuccess || attr.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return set_error(CHIRON_ERR_INVALID, "chiron_align_infix: workspace must be device memory on device %d", device_id);
  }
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.pair, recs.data(), recs.size() * sizeof(AlignPair), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (total > 0 && hipMemcpyAsync(ws + l.codes, packed.data(), packed.size(), hipMemcpyHostToDevice, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "chiron_align_infix: copying the pairs to the device failed");
  InfixParams p;
  p.codes = (const uint8_t*)(ws + l.codes);
  p.pair = (const AlignPair*)(ws + l.pair);
  p.pairs = pairs;
  p.rows = l.row_slots ? (int64_t*)(ws + l.rows) : nullptr;
  p.row_slots = l.row_slots;
  p.out = (int32_t*)(ws + l.out);
  p.band0 = band0;
  if (launch_infix(p, l.groups, stream) != 0) return set_error(CHIRON_ERR_DEVICE, "chiron_align_infix: launch failed");
  std::vector<int32_t> out((size_t)pairs * 5);
  if (hipMemcpyAsync(out.data(), ws + l.out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "chiron_align_infix: the alignment kernel failed (%s)", hipGetErrorString(hipGetLastError()));
  for (int64_t q = 0; q < pairs; ++q) {
    if (out[q * 5] < 0) return set_error(CHIRON_ERR_STATE, "chiron_align_infix: pair %lld outgrew its workspace row", (long long)q);
    edit_out[q] = out[q * 5];
    match_out[q] = out[q * 5 + 1];
    start_out[q] = out[q * 5 + 2];
    end_out[q] = out[q * 5 + 3];
    band_out[q] = out[q * 5 + 4];
  }
  return CHIRON_OK;
}
