// Read-level assessment on gfx950: global alignment of a read against its reference, unit costs, exact (E, M) per pair.
//
//   E = Levenshtein distance, M = most matching columns over the alignments of cost E          (include/chiron_amd.h)
//
// One 64-bit key per DP cell carries both: key = E * 2^32 - M.  A match adds -1, a mismatch or a gap adds 2^32, and the
// recurrence is a three-way min: the smallest key is the smallest E and, among those, the largest M (M < 2^31 never borrows
// from E's half).
//
// Work mapping: one workgroup per pair, an anti-diagonal wavefront over a band of diagonals d = j - i in
// [min(0, m-n) - w, max(0, m-n) + w].  Cell (i, j) sits on anti-diagonal k = i + j and reads (i-1, j-1) = (k-2, d),
// (i-1, j) = (k-1, d+1) and (i, j-1) = (k-1, d-1).  Cells of one anti-diagonal share k's parity, so the last three
// anti-diagonals fit ONE array indexed by d: step k overwrites the slots of k's parity in place (each slot's old value, from
// k-2, is read by its own thread only) and reads the other parity's slots, which step k-1 wrote.  One barrier per step.
// The array lives in LDS while the band has at most CHIRON_ALIGN_LDS_SLOTS diagonals and in the workgroup's workspace row
// beyond that.
//
// Exactness: the path starts on diagonal 0 and ends on diagonal m-n, and only a gap changes the diagonal, by one.  To touch a
// diagonal outside the band a path needs at least w + 1 gaps to get there from the nearer end of [0, m-n], w + 1 to come back,
// and |m-n| more to cover the distance between the ends: 2(w+1) + |m-n| in all.  So when the banded minimum satisfies
// E <= 2w + 1 + |m-n|, every path of cost <= E lies inside the band: E is the true distance and every optimal alignment was
// seen, so M is exact as well.  Otherwise w doubles and the pair is redone, up to the full table; all inside the kernel, so a
// batch is one launch.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/chiron_amd.h"
#include "kernels.h"

namespace chiron {

chiron_status set_error(chiron_status st, const char* fmt, ...);   // engine.hip

namespace {

constexpr int64_t ALIGN_GAP = (int64_t)1 << 32;
constexpr int NT = CHIRON_ALIGN_THREADS;

__device__ inline int imax(int a, int b) { return a > b ? a : b; }
__device__ inline int imin(int a, int b) { return a < b ? a : b; }

// one pass over the band [dlo, dhi] (already clipped to the table's diagonals -n .. m); returns the key of cell (n, m)
__device__ __forceinline__ int64_t band_pass(int64_t* row, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int n, int m, int dlo, int dhi) {
  const int tid = threadIdx.x;
  for (int k = 0; k <= n + m; ++k) {
    // the anti-diagonal's cells inside the table and the band: 0 <= i = (k-d)/2 <= n, 0 <= j = (k+d)/2 <= m
    const int lo = imax(imax(dlo, -k), k - 2 * n);
    const int hi = imin(imin(dhi, k), 2 * m - k);
    const int first = lo + ((lo + k) & 1);
    for (int d = first + 2 * tid; d <= hi; d += 2 * NT) {
      const int i = (k - d) >> 1, j = (k + d) >> 1;
      const int s = d - dlo;
      int64_t best = k == 0 ? 0 : (int64_t)1 << 60;
      if (i > 0 && j > 0) {
        const uint8_t ca = a[i - 1], cb = b[j - 1];
        best = row[s] + ((ca == cb && ca < 4) ? (int64_t)-1 : ALIGN_GAP);
      }
      if (i > 0 && d < dhi) {
        const int64_t up = row[s + 1] + ALIGN_GAP;
        best = up < best ? up : best;
      }
      if (j > 0 && d > dlo) {
        const int64_t left = row[s - 1] + ALIGN_GAP;
        best = left < best ? left : best;
      }
      row[s] = best;
    }
    __syncthreads();
  }
  const int64_t key = row[(m - n) - dlo];
  __syncthreads();   // every thread has read the result before the next pass writes the array
  return key;
}

__global__ __launch_bounds__(CHIRON_ALIGN_THREADS) void align_kernel(AlignParams p) {
  __shared__ int64_t lds_row[CHIRON_ALIGN_LDS_SLOTS];
  int64_t* const ws_row = p.rows ? p.rows + (int64_t)blockIdx.x * p.row_slots : nullptr;
  for (int64_t q = blockIdx.x; q < p.pairs; q += gridDim.x) {
    const AlignPair pr = p.pair[q];
    const int n = pr.n, m = pr.m;
    const uint8_t* a = p.codes + pr.start;
    const uint8_t* b = a + n;
    const int gap = m > n ? m - n : n - m;
    int w = CHIRON_ALIGN_BAND0;
    int E, M;
    for (;;) {
      const int dlo = imax((m < n ? m - n : 0) - w, -n);
      const int dhi = imin((m > n ? m - n : 0) + w, m);
      const bool full = dlo == -n && dhi == m;
      const int slots = dhi - dlo + 1;
      // the host sized the row for the full table of the call's longest pair; a pair that would not fit cannot occur, and is
      // answered with E = -1 rather than with a write past the row
      int64_t key;
      if (slots <= CHIRON_ALIGN_LDS_SLOTS) {
        key = band_pass(lds_row, a, b, n, m, dlo, dhi);
      } else if (ws_row && slots <= p.row_slots) {
        key = band_pass(ws_row, a, b, n, m, dlo, dhi);
      } else {
        E = -1;
        M = 0;
        break;
      }
      E = (int)((key + (ALIGN_GAP >> 1)) >> 32);
      M = (int)((int64_t)E * ALIGN_GAP - key);
      if (full || E <= 2 * w + 1 + gap) break;
      w *= 2;
    }
    if (threadIdx.x == 0) {
      p.out[q * 3 + 0] = E;
      p.out[q * 3 + 1] = M;
      p.out[q * 3 + 2] = w;
    }
  }
}

}  // namespace

chiron_status align_layout(int64_t pairs, int64_t max_len, AlignLayout* l) {
  if (pairs < 0 || max_len < 0) return set_error(CHIRON_ERR_INVALID, "align: negative pairs / max_len");
  if (max_len > CHIRON_ALIGN_MAX_LEN)
    return set_error(CHIRON_ERR_OVERFLOW, "align: a sequence of %lld bases, the kernel takes at most %d", (long long)max_len, CHIRON_ALIGN_MAX_LEN);
  if (pairs > ((int64_t)1 << 24)) return set_error(CHIRON_ERR_OVERFLOW, "align: %lld pairs in one call, at most 2^24", (long long)pairs);
  // pairs <= 2^24 and max_len <= 2^17: every product below stays under 2^46
  const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  l->groups = (int)(pairs < CHIRON_ALIGN_MAX_GROUPS ? pairs : CHIRON_ALIGN_MAX_GROUPS);
  l->row_slots = 2 * max_len + 1 > CHIRON_ALIGN_LDS_SLOTS ? 2 * max_len + 2 : 0;
  l->pair = 0;
  l->out = l->pair + up((size_t)pairs * sizeof(AlignPair));
  l->codes = l->out + up((size_t)pairs * 3 * sizeof(int32_t));
  l->rows = l->codes + up((size_t)pairs * 2 * (size_t)max_len);
  l->bytes = l->rows + up((size_t)l->groups * (size_t)l->row_slots * sizeof(int64_t));
  return CHIRON_OK;
}

int launch_align(const AlignParams& p, int groups, hipStream_t stream) {
  if (p.pairs <= 0) return 0;
  hipLaunchKernelGGL(align_kernel, dim3(groups), dim3(CHIRON_ALIGN_THREADS), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_align_workspace_size(int64_t pairs, int64_t max_len, size_t* bytes) {
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "chiron_align_workspace_size: null bytes");
  AlignLayout l;
  chiron_status st = align_layout(pairs, max_len, &l);
  if (st) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_align_pairs(int32_t device_id, const uint8_t* codes, const int64_t* read_off, const int64_t* ref_off,
                                            int64_t pairs, uint32_t flags, int32_t* edit_out, int32_t* match_out, int32_t* band_out,
                                            void* workspace, void* stream_) {
  if (pairs < 0) return set_error(CHIRON_ERR_INVALID, "chiron_align_pairs: pairs %lld", (long long)pairs);
  if (flags) return set_error(CHIRON_ERR_INVALID, "chiron_align_pairs: unknown flags 0x%x", flags);
  if (pairs == 0) return CHIRON_OK;
  if (pairs > ((int64_t)1 << 24)) return set_error(CHIRON_ERR_OVERFLOW, "chiron_align_pairs: %lld pairs in one call, at most 2^24", (long long)pairs);
  if (!read_off || !ref_off || !edit_out || !match_out || !band_out) return set_error(CHIRON_ERR_INVALID, "chiron_align_pairs: null operand");
  // offsets first (they bound what may be read of `codes`), then the codes while they are packed pair by pair
  int64_t max_len = 0, total = 0;
  for (int which = 0; which < 2; ++which) {
    const int64_t* off = which ? ref_off : read_off;
    if (off[0] < 0) return set_error(CHIRON_ERR_INVALID, "chiron_align_pairs: %s_off[0] = %lld is negative", which ? "ref" : "read", (long long)off[0]);
    for (int64_t q = 0; q < pairs; ++q) {
      if (off[q + 1] < off[q])
        return set_error(CHIRON_ERR_INVALID, "chiron_align_pairs: %s_off[%lld] = %lld below its predecessor %lld", which ? "ref" : "read",
                         (long long)(q + 1), (long long)off[q + 1], (long long)off[q]);
      const int64_t len = off[q + 1] - off[q];
      if (len > CHIRON_ALIGN_MAX_LEN)
        return set_error(CHIRON_ERR_OVERFLOW, "chiron_align_pairs: %s %lld has %lld bases, at most %d", which ? "reference" : "read",
                         (long long)q, (long long)len, CHIRON_ALIGN_MAX_LEN);
      if (len > max_len) max_len = len;
      total += len;
    }
  }
  if (total > 0 && !codes) return set_error(CHIRON_ERR_INVALID, "chiron_align_pairs: null codes");
  std::vector<uint8_t> packed((size_t)total);
  std::vector<AlignPair> recs((size_t)pairs);
  int64_t at = 0;
  for (int64_t q = 0; q < pairs; ++q) {
    recs[q].start = at;
    recs[q].n = (int32_t)(read_off[q + 1] - read_off[q]);
    recs[q].m = (int32_t)(ref_off[q + 1] - ref_off[q]);
    for (int which = 0; which < 2; ++which) {
      const int64_t lo = which ? ref_off[q] : read_off[q], len = which ? recs[q].m : recs[q].n;
      for (int64_t i = 0; i < len; ++i) {
        const uint8_t c = codes[lo + i];
        if (c > 4)
          return set_error(CHIRON_ERR_INVALID, "chiron_align_pairs: code %d at %lld of %s %lld outside 0..4", (int)c, (long long)i,
                           which ? "reference" : "read", (long long)q);
        packed[(size_t)(at + i)] = c;
      }
      at += len;
    }
  }
  AlignLayout l;
  chiron_status st = align_layout(pairs, max_len, &l);
  if (st) return st;
  if (!workspace) return set_error(CHIRON_ERR_INVALID, "chiron_align_pairs: null workspace");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) {
    (void)hipGetLastError();
    return set_error(CHIRON_ERR_DEVICE, "no HIP device %d: libchiron_amd has no CPU fallback", device_id);
  }
  if (hipSetDevice(device_id) != hipSuccess) return set_error(CHIRON_ERR_DEVICE, "hipSetDevice(%d) failed", device_id);
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, workspace) != hipSuccess || attr.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return set_error(CHIRON_ERR_INVALID, "chiron_align_pairs: workspace must be device memory on device %d", device_id);
  }
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.pair, recs.data(), recs.size() * sizeof(AlignPair), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (total > 0 && hipMemcpyAsync(ws + l.codes, packed.data(), packed.size(), hipMemcpyHostToDevice, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "chiron_align_pairs: copying the pairs to the device failed");
  AlignParams p;
  p.codes = (const uint8_t*)(ws + l.codes);
  p.pair = (const AlignPair*)(ws + l.pair);
  p.pairs = pairs;
  p.rows = l.row_slots ? (int64_t*)(ws + l.rows) : nullptr;
  p.row_slots = l.row_slots;
  p.out = (int32_t*)(ws + l.out);
  if (launch_align(p, l.groups, stream) != 0) return set_error(CHIRON_ERR_DEVICE, "chiron_align_pairs: launch failed");
  std::vector<int32_t> out((size_t)pairs * 3);
  if (hipMemcpyAsync(out.data(), ws + l.out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "chiron_align_pairs: the alignment kernel failed (%s)", hipGetErrorString(hipGetLastError()));
  for (int64_t q = 0; q < pairs; ++q) {
    if (out[q * 3] < 0) return set_error(CHIRON_ERR_STATE, "chiron_align_pairs: pair %lld outgrew its workspace row", (long long)q);
    edit_out[q] = out[q * 3];
    match_out[q] = out[q * 3 + 1];
    band_out[q] = out[q * 3 + 2];
  }
  return CHIRON_OK;
}
