// What the alignment stages share: the banded anti-diagonal sweep of assess.hip and map.hip and the band arithmetic trace.hip
// uses as well (device), and the argument checks, packing and device set-up of the entry points of assess.hip, map.hip,
// trace.hip, pileup.hip and ctc_align.hip (host).  Every host helper takes the entry point's name and nouns: the text of
// chiron_last_error() is part of what the tests pin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/chiron_amd.h"
#include "host_entry.h"

namespace chiron {

// ---------------------------------------------------------------------------------------------
// device: the band and its sweep
// ---------------------------------------------------------------------------------------------
static_assert(CHIRON_INFIX_THREADS == CHIRON_ALIGN_THREADS && CHIRON_INFIX_LDS_SLOTS == CHIRON_ALIGN_LDS_SLOTS,
              "assess.hip and map.hip run one sweep: one workgroup size, one LDS row");
constexpr int BAND_THREADS = CHIRON_ALIGN_THREADS;
constexpr int BAND_LDS_SLOTS = CHIRON_ALIGN_LDS_SLOTS;

__host__ __device__ inline int imax(int a, int b) { return a > b ? a : b; }
__host__ __device__ inline int imin(int a, int b) { return a < b ? a : b; }

// the diagonals d = j - i of the band of half-width w around [min(0, m-n), max(0, m-n)], clipped to the table's -n .. m
struct Diagonals {
  int dlo, dhi;
};
__host__ __device__ inline Diagonals band_clip(int n, int m, int w) { return {imax((m < n ? m - n : 0) - w, -n), imin((m > n ? m - n : 0) + w, m)}; }

// the cells of anti-diagonal k = i + j inside the table and the band: 0 <= i = (k-d)/2 <= n, 0 <= j = (k+d)/2 <= m; they are the
// diagonals first, first + 2, ... <= hi
struct DiagRange {
  int first, hi;
};
__device__ inline DiagRange diag_range(int k, int n, int m, int dlo, int dhi) {
  const int lo = imax(imax(dlo, -k), k - 2 * n);
  return {lo + ((lo + k) & 1), imin(imin(dhi, k), 2 * m - k)};
}

// Runs pass(row) on the array a band of `slots` diagonals lives in: the LDS row while it fits, the workgroup's workspace row
// while slots <= ws_fit, else nothing (false).  The host sized the workspace row for the widest band of the call, so a band that
// fits neither cannot occur; the caller answers it with a status rather than with a write past the row.  ws_fit is row_slots
// for assess.hip and map.hip and row_slots - 1 for trace.hip, whose two halves take slots + 1 entries when slots is odd.
// Inlined, so that each pass is compiled for its own address space.
template <class Pass>
__device__ __forceinline__ bool with_row(int64_t* lds_row, int64_t* ws_row, int slots, int64_t ws_fit, Pass&& pass) {
  if (slots <= BAND_LDS_SLOTS) {
    pass(lds_row);
  } else if (ws_row && slots <= ws_fit) {
    pass(ws_row);
  } else {
    return false;
  }
  return true;
}

// One pass over the band [dlo, dhi] (already clipped).  Cell (i, j) sits on anti-diagonal k = i + j and reads (i-1, j-1) =
// (k-2, d), (i-1, j) = (k-1, d+1) and (i, j-1) = (k-1, d-1).  Cells of one anti-diagonal share k's parity, so the last three
// anti-diagonals fit ONE array indexed by d: step k overwrites the slots of k's parity in place (each slot's old value, from
// k-2, is read by its own thread only) and reads the other parity's slots, which step k-1 wrote.  One barrier per step; after
// the last one row[d - dlo] holds the last cell of diagonal d.
//
// Cell is the recurrence's policy: EDIT is added for a mismatch or a gap and MATCH for a match, border(k, i, j) is the value of
// a cell before any move into it (k = i + j is passed because it is uniform over the workgroup), and with FREE_ROW0 the cells of
// row 0 are starts of their own: no move is taken into them.
template <class Cell>
__device__ __forceinline__ void band_sweep(int64_t* row, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int n, int m, int dlo,
                                           int dhi) {
  const int tid = threadIdx.x;
  for (int k = 0; k <= n + m; ++k) {
    const DiagRange r = diag_range(k, n, m, dlo, dhi);
    for (int d = r.first + 2 * tid; d <= r.hi; d += 2 * BAND_THREADS) {
      const int i = (k - d) >> 1, j = (k + d) >> 1;
      const int s = d - dlo;
      int64_t best = Cell::border(k, i, j);
      if (!Cell::FREE_ROW0 || i > 0) {
        if (i > 0 && j > 0) {
          const uint8_t ca = a[i - 1], cb = b[j - 1];
          best = row[s] + ((ca == cb && ca < 4) ? Cell::MATCH : Cell::EDIT);
        }
        if (i > 0 && d < dhi) {
          const int64_t up = row[s + 1] + Cell::EDIT;
          best = up < best ? up : best;
        }
        if (j > 0 && d > dlo) {
          const int64_t left = row[s - 1] + Cell::EDIT;
          best = left < best ? left : best;
        }
      }
      row[s] = best;
    }
    __syncthreads();
  }
}

// key = E * 2^32 - M of assess.hip and trace.hip, M < 2^31: the smallest key is the smallest E and, among those, the largest M
constexpr int64_t KEY32_EDIT = (int64_t)1 << 32;
__device__ inline void key32_decode(int64_t key, int* E, int* M) {
  *E = (int)((key + (KEY32_EDIT >> 1)) >> 32);
  *M = (int)((int64_t)*E * KEY32_EDIT - key);
}

// ---------------------------------------------------------------------------------------------
// host: what the entry points check and set up before they launch
// ---------------------------------------------------------------------------------------------
constexpr int64_t MAX_BATCH_ITEMS = (int64_t)1 << 24;   // pairs, reads or alignments of one call
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// off[0 .. count] of the array `short_name`_off: starts at or above 0, never decreases, no item longer than limit.  Raises
// *max_len to the longest item and adds the items' lengths to *total.
inline chiron_status check_offsets(const char* who, const char* short_name, const char* item, const char* unit, const int64_t* off, int64_t count,
                                   int64_t limit, int64_t* max_len, int64_t* total) {
  if (off[0] < 0) return set_error(CHIRON_ERR_INVALID, "%s: %s_off[0] = %lld is negative", who, short_name, (long long)off[0]);
  for (int64_t q = 0; q < count; ++q) {
    if (off[q + 1] < off[q])
      return set_error(CHIRON_ERR_INVALID, "%s: %s_off[%lld] = %lld below its predecessor %lld", who, short_name, (long long)(q + 1),
                       (long long)off[q + 1], (long long)off[q]);
    const int64_t len = off[q + 1] - off[q];
    if (len > limit)
      return set_error(CHIRON_ERR_OVERFLOW, "%s: %s %lld has %lld %s, at most %lld", who, item, (long long)q, (long long)len, unit, (long long)limit);
    if (len > *max_len) *max_len = len;
    *total += len;
  }
  return CHIRON_OK;
}

// Packs pair q as a[q] then b[q], pair after pair, while checking every code, and fills recs[q].start / n / m (AlignPair,
// TracePair).  The offsets have passed check_offsets.
template <class Rec>
inline chiron_status pack_codes(const char* who, const char* item_a, const char* item_b, const uint8_t* codes, const int64_t* off_a,
                                const int64_t* off_b, int64_t pairs, Rec* recs, uint8_t* packed) {
  int64_t at = 0;
  for (int64_t q = 0; q < pairs; ++q) {
    recs[q].start = at;
    recs[q].n = (int32_t)(off_a[q + 1] - off_a[q]);
    recs[q].m = (int32_t)(off_b[q + 1] - off_b[q]);
    for (int which = 0; which < 2; ++which) {
      const int64_t lo = which ? off_b[q] : off_a[q], len = which ? recs[q].m : recs[q].n;
      for (int64_t i = 0; i < len; ++i) {
        const uint8_t c = codes[lo + i];
        if (c > 4)
          return set_error(CHIRON_ERR_INVALID, "%s: code %d at %lld of %s %lld outside 0..4", who, (int)c, (long long)i, which ? item_b : item_a,
                           (long long)q);
        packed[at + i] = c;
      }
      at += len;
    }
  }
  return CHIRON_OK;
}

// The last refusals before the first copy: a workspace, a device to run on, and the workspace in that device's memory.
inline chiron_status use_device_workspace(const char* who, int32_t device_id, const void* workspace) {
  if (!workspace) return set_error(CHIRON_ERR_INVALID, "%s: null workspace", who);
  if (chiron_status st = enter_device(nullptr, device_id)) return st;
  if (!on_device(workspace)) return set_error(CHIRON_ERR_INVALID, "%s: workspace must be device memory on device %d", who, device_id);
  return CHIRON_OK;
}

}  // namespace chiron
