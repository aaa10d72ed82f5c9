// Alignment traceback on gfx950: the canonical optimal global alignment of a read against its reference, as a column string.
//
// The pair's (E, M) is known (chiron_align_pairs, chiron_align_infix).  Among the alignments with that (E, M) the canonical one
// is the one whose column string, read from the last column to the first, is smallest under diagonal < I < D: walking back from
// (n, m), every cell takes its first admissible predecessor in the order diagonal, up, left.  That order is fixed, so one 2-bit
// pointer per cell, written during the forward sweep, is the whole record.              (include/chiron_amd.h)
//
// Work mapping: one workgroup per pair, assess.hip's recurrence over one array of keys E * 2^32 - M indexed by diagonal (the band
// clip, the anti-diagonal's range, the row choice and the key are align_common.h's; the sweep is this file's own, below),
// run ONCE at the half-width the known cost allows: a path that touches diagonal max(0, m-n) + x costs at least 2x + |m-n|, so
// every alignment of cost E lies inside w* = (E - |m-n|) / 2 and no doubling is needed.  The cells of one anti-diagonal share
// its parity, so the array is kept as two halves, even slots and odd slots: cell c of anti-diagonal k (slot 2c + parity) is entry
// c of its half and its two gap neighbours are entries c - 1 + parity and c + parity of the other half.  A thread owns four
// consecutive cells: 32 contiguous bytes of keys, and their four pointers make one byte, so the bytes a wave stores per step are
// consecutive.  Keys live in LDS while the band has at most CHIRON_ALIGN_LDS_SLOTS diagonals, in the workgroup's workspace row
// beyond that.  One barrier per anti-diagonal.  The traceback is sequential: one lane walks the pointers from (n, m) and fills the
// pair's columns from the last one down.  No atomics: a pair's result does not depend on what else is in the batch.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "kernels.h"

namespace chiron {

namespace {

constexpr int64_t ALIGN_GAP = KEY32_EDIT;
constexpr int NT = CHIRON_ALIGN_THREADS;
constexpr int STATUS_MISMATCH = 1;           // the end cell's (E, M) is not what the caller passed in
constexpr int STATUS_INTERNAL = 2;           // a guard of the kernel fired: reported as CHIRON_ERR_STATE, never returned to the caller

// the sweep over the band [dlo, dhi] (clipped to the table's diagonals -n .. m); writes every cell's pointer, returns the key of (n, m)
__device__ __forceinline__ int64_t traced_pass(int64_t* row, uint8_t* __restrict__ bp, const uint8_t* __restrict__ a,
                                               const uint8_t* __restrict__ b, int n, int m, int dlo, int dhi, int rowbytes) {
  const int tid = threadIdx.x;
  const int half = (dhi - dlo + 2) >> 1;      // entries of the even half; the odd half follows it
  for (int k = 0; k <= n + m; ++k) {
    const DiagRange r = diag_range(k, n, m, dlo, dhi);
    const int first = r.first, hi = r.hi;
    if (first <= hi) {
      const int par = (k - dlo) & 1;          // the parity of this anti-diagonal's slots d - dlo
      int64_t* own = row + par * half;        // step k rewrites its own half in place (each entry's old value, from k-2, is read by its own thread only)
      const int64_t* oth = row + (par ^ 1) * half;   // and reads the other one, which step k-1 wrote
      const int cmin = (first - dlo) >> 1, cmax = (hi - dlo) >> 1;
      uint8_t* bprow = bp + (int64_t)k * rowbytes;
      for (int g = (cmin >> 2) + tid; g <= (cmax >> 2); g += NT) {
        unsigned byte = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int c = 4 * g + t;
          if (c >= cmin && c <= cmax) {
            const int d = dlo + par + 2 * c;
            const int i = (k - d) >> 1, j = (k + d) >> 1;
            int64_t best = k == 0 ? 0 : (int64_t)1 << 60;
            unsigned ptr = 0;
            if (i > 0 && j > 0) {
              const uint8_t ca = a[i - 1], cb = b[j - 1];
              best = own[c] + ((ca == cb && ca < 4) ? (int64_t)-1 : ALIGN_GAP);
            }
            if (i > 0 && d < dhi) {
              const int64_t up = oth[c + par] + ALIGN_GAP;
              if (up < best) {
                best = up;
                ptr = 1;
              }
            }
            if (j > 0 && d > dlo) {
              const int64_t left = oth[c + par - 1] + ALIGN_GAP;
              if (left < best) {
                best = left;
                ptr = 2;
              }
            }
            own[c] = best;
            byte |= ptr << (2 * t);
          }
        }
        bprow[g] = (uint8_t)byte;
      }
    }
    __syncthreads();
  }
  const int s = (m - n) - dlo;
  const int64_t key = row[(s & 1) * half + (s >> 1)];
  __syncthreads();   // every thread has read the result before the next pair writes the array
  return key;
}

// One lane: rederive (E, M) from the end cell's key, then walk the pointers from (n, m) and fill the columns from the last one down.
__device__ int walk(const TracePair& pr, int64_t key, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                    const uint8_t* bp, uint8_t* __restrict__ ops) {
  int E, M;
  key32_decode(key, &E, &M);
  if (E != pr.E || M != pr.M) return STATUS_MISMATCH;
  const int dlo = pr.dlo, slots = pr.dhi - pr.dlo + 1;
  int i = pr.n, j = pr.m, pos = E + M;
  while (i > 0 || j > 0) {
    const int s = (j - i) - dlo;
    if (s < 0 || s >= slots || pos <= 0) return STATUS_INTERNAL;   // a path never leaves the band, and it has exactly E + M columns
    const int c = s >> 1;
    const unsigned ptr = (bp[(int64_t)(i + j) * pr.rowbytes + (c >> 2)] >> (2 * (c & 3))) & 3;
    if (ptr == 3 || (ptr != 2 && i == 0) || (ptr != 1 && j == 0)) return STATUS_INTERNAL;
    uint8_t op;
    if (ptr == 0) {
      const uint8_t ca = a[i - 1], cb = b[j - 1];
      op = (ca == cb && ca < 4) ? 0 : 1;
      --i;
      --j;
    } else if (ptr == 1) {
      op = 2;
      --i;
    } else {
      op = 3;
      --j;
    }
    ops[--pos] = op;
  }
  return pos == 0 ? 0 : STATUS_INTERNAL;
}

__global__ __launch_bounds__(CHIRON_ALIGN_THREADS) void trace_kernel(TraceParams p) {
  __shared__ int64_t lds_row[CHIRON_ALIGN_LDS_SLOTS];
  int64_t* const ws_row = p.rows ? p.rows + (int64_t)blockIdx.x * p.row_slots : nullptr;
  for (int64_t q = blockIdx.x; q < p.pairs; q += gridDim.x) {
    const TracePair pr = p.pair[q];
    const int n = pr.n, m = pr.m, dlo = pr.dlo, dhi = pr.dhi;
    const uint8_t* a = p.codes + pr.start;
    const uint8_t* b = a + n;
    uint8_t* bp = p.bp + pr.bp;
    // the two halves take slots + 1 entries when slots is odd (LDS_SLOTS is even): a workspace row has to be longer than slots
    int64_t key;
    if (!with_row(lds_row, ws_row, dhi - dlo + 1, p.row_slots - 1,
                  [&](int64_t* row) { key = traced_pass(row, bp, a, b, n, m, dlo, dhi, pr.rowbytes); })) {
      if (threadIdx.x == 0) p.status[q] = STATUS_INTERNAL;
      continue;
    }
    if (threadIdx.x == 0) p.status[q] = walk(pr, key, a, b, bp, p.ops + pr.ops);   // the others wait at the next pair's first barrier
  }
}

}  // namespace

TraceBand trace_band(int64_t n, int64_t m, int64_t E) {
  const int64_t gap = m > n ? m - n : n - m;
  const Diagonals bd = band_clip((int)n, (int)m, (int)((E - gap) / 2));   // check_pair has bounded n, m and E by CHIRON_ALIGN_MAX_LEN
  TraceBand t;
  t.dlo = bd.dlo;
  t.dhi = bd.dhi;
  t.width = (int64_t)bd.dhi - bd.dlo + 1;
  const int64_t cells = (t.width + 1) >> 1;   // of one anti-diagonal
  t.rowbytes = (int32_t)((cells + 3) >> 2);
  t.bytes = (n + m + 1) * (int64_t)t.rowbytes;
  return t;
}

static chiron_status check_pair(const char* who, int64_t q, int64_t n, int64_t m, int64_t E) {
  if (n < 0 || m < 0) return set_error(CHIRON_ERR_INVALID, "%s: pair %lld has a negative length", who, (long long)q);
  if (n > CHIRON_ALIGN_MAX_LEN || m > CHIRON_ALIGN_MAX_LEN)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: pair %lld has %lld / %lld bases, at most %d", who, (long long)q, (long long)n, (long long)m,
                     CHIRON_ALIGN_MAX_LEN);
  const int64_t gap = m > n ? m - n : n - m, longest = m > n ? m : n;
  if (E < gap || E > longest)
    return set_error(CHIRON_ERR_INVALID, "%s: pair %lld (%lld against %lld bases) cannot have edit distance %lld", who, (long long)q, (long long)n,
                     (long long)m, (long long)E);
  return CHIRON_OK;
}

chiron_status trace_layout(int64_t pairs, int64_t backpointer_bytes, int64_t max_len, int64_t max_band, TraceLayout* l) {
  if (pairs < 0 || backpointer_bytes < 0 || max_len < 0 || max_band < 0)
    return set_error(CHIRON_ERR_INVALID, "align_trace: negative pairs / backpointer_bytes / max_len / max_band");
  if (max_len > CHIRON_ALIGN_MAX_LEN)
    return set_error(CHIRON_ERR_OVERFLOW, "align_trace: a sequence of %lld bases, the kernel takes at most %d", (long long)max_len, CHIRON_ALIGN_MAX_LEN);
  if (pairs > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "align_trace: %lld pairs in one call, at most 2^24", (long long)pairs);
  if (backpointer_bytes > ((int64_t)1 << 46))
    return set_error(CHIRON_ERR_OVERFLOW, "align_trace: the back-pointers of the call pass 2^46 bytes: split the batch");
  if (max_band > 2 * max_len + 1) max_band = 2 * max_len + 1;   // no band is wider than the table
  // pairs <= 2^24 and max_len <= 2^17: every product below stays under 2^46
  l->groups = (int)(pairs < CHIRON_ALIGN_MAX_GROUPS ? pairs : CHIRON_ALIGN_MAX_GROUPS);
  l->row_slots = max_band > CHIRON_ALIGN_LDS_SLOTS ? ((max_band + 2) & ~(int64_t)1) : 0;
  l->pair = 0;
  l->status = l->pair + up256((size_t)pairs * sizeof(TracePair));
  l->codes = l->status + up256((size_t)pairs * sizeof(int32_t));
  l->ops = l->codes + up256((size_t)pairs * 2 * (size_t)max_len);
  l->rows = l->ops + up256((size_t)pairs * 2 * (size_t)max_len);
  l->bp = l->rows + up256((size_t)l->groups * (size_t)l->row_slots * sizeof(int64_t));
  l->bytes = l->bp + up256((size_t)backpointer_bytes);
  return CHIRON_OK;
}

int launch_trace(const TraceParams& p, int groups, hipStream_t stream) {
  if (p.pairs <= 0) return 0;
  hipLaunchKernelGGL(trace_kernel, dim3(groups), dim3(CHIRON_ALIGN_THREADS), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_align_trace_pair_size(int64_t n, int64_t m, int64_t edit, int64_t* backpointer_bytes, int64_t* band) {
  if (!backpointer_bytes || !band) return set_error(CHIRON_ERR_INVALID, "chiron_align_trace_pair_size: null output");
  chiron_status st = check_pair("chiron_align_trace_pair_size", 0, n, m, edit);
  if (st) return st;
  const TraceBand t = trace_band(n, m, edit);
  *backpointer_bytes = t.bytes;
  *band = t.width;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_align_trace_workspace_size(int64_t pairs, int64_t backpointer_bytes, int64_t max_len, int64_t max_band,
                                                           size_t* bytes) {
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "chiron_align_trace_workspace_size: null bytes");
  TraceLayout l;
  chiron_status st = trace_layout(pairs, backpointer_bytes, max_len, max_band, &l);
  if (st) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_align_trace(int32_t device_id, const uint8_t* codes, const int64_t* read_off, const int64_t* ref_off,
                                            int64_t pairs, const int32_t* edit_in, const int32_t* match_in, const int64_t* ops_off,
                                            uint32_t flags, uint8_t* ops_out, int32_t* status_out, void* workspace, void* stream_) {
  const char* const who = "chiron_align_trace";
  if (pairs < 0) return set_error(CHIRON_ERR_INVALID, "%s: pairs %lld", who, (long long)pairs);
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  if (pairs == 0) return CHIRON_OK;
  if (pairs > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld pairs in one call, at most 2^24", who, (long long)pairs);
  if (!read_off || !ref_off || !edit_in || !match_in || !ops_off || !status_out) return set_error(CHIRON_ERR_INVALID, "%s: null operand", who);
  // offsets first (they bound what may be read of `codes`), then (E, M) against the lengths and the columns, then the codes
  int64_t max_len = 0, total = 0;
  chiron_status st = check_offsets(who, "read", "read", "bases", read_off, pairs, CHIRON_ALIGN_MAX_LEN, &max_len, &total);
  if (!st) st = check_offsets(who, "ref", "reference", "bases", ref_off, pairs, CHIRON_ALIGN_MAX_LEN, &max_len, &total);
  if (st) return st;
  if (ops_off[0] < 0) return set_error(CHIRON_ERR_INVALID, "%s: ops_off[0] = %lld is negative", who, (long long)ops_off[0]);
  std::vector<TracePair> recs((size_t)pairs);
  int64_t bp = 0, max_band = 0;
  for (int64_t q = 0; q < pairs; ++q) {
    const int64_t n = read_off[q + 1] - read_off[q], m = ref_off[q + 1] - ref_off[q], E = edit_in[q], M = match_in[q];
    if ((st = check_pair(who, q, n, m, E))) return st;
    // X = n + m - 2M - E mismatches, and the alignment has n + m - M - X = E + M columns
    if (M < 0 || n + m - 2 * M - E < 0)
      return set_error(CHIRON_ERR_INVALID, "%s: pair %lld (%lld against %lld bases, edit %lld) cannot have %lld matches", who, (long long)q,
                       (long long)n, (long long)m, (long long)E, (long long)M);
    if (ops_off[q + 1] - ops_off[q] != E + M)
      return set_error(CHIRON_ERR_INVALID, "%s: ops_off gives pair %lld %lld columns, its alignment has %lld", who, (long long)q,
                       (long long)(ops_off[q + 1] - ops_off[q]), (long long)(E + M));
    const TraceBand t = trace_band(n, m, E);
    TracePair& r = recs[(size_t)q];   // start, n and m: pack_codes below
    r.bp = bp;
    r.ops = ops_off[q] - ops_off[0];
    r.E = (int32_t)E;
    r.M = (int32_t)M;
    r.dlo = t.dlo;
    r.dhi = t.dhi;
    r.rowbytes = t.rowbytes;
    r.pad_ = 0;
    bp += t.bytes;
    if (bp > ((int64_t)1 << 46)) return set_error(CHIRON_ERR_OVERFLOW, "%s: the back-pointers of the call pass 2^46 bytes: split the batch", who);
    if (t.width > max_band) max_band = t.width;
  }
  if (total > 0 && !codes) return set_error(CHIRON_ERR_INVALID, "%s: null codes", who);
  const int64_t columns = ops_off[pairs] - ops_off[0];
  if (columns > 0 && !ops_out) return set_error(CHIRON_ERR_INVALID, "%s: null ops_out", who);
  std::vector<uint8_t> packed((size_t)total);
  TraceLayout l;
  if ((st = pack_codes(who, "read", "reference", codes, read_off, ref_off, pairs, recs.data(), packed.data()))) return st;
  if ((st = trace_layout(pairs, bp, max_len, max_band, &l))) return st;
  if ((st = use_device_workspace(who, device_id, workspace))) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.pair, recs.data(), recs.size() * sizeof(TracePair), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (total > 0 && hipMemcpyAsync(ws + l.codes, packed.data(), packed.size(), hipMemcpyHostToDevice, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the pairs to the device failed", who);
  TraceParams p;
  p.codes = (const uint8_t*)(ws + l.codes);
  p.pair = (const TracePair*)(ws + l.pair);
  p.pairs = pairs;
  p.rows = l.row_slots ? (int64_t*)(ws + l.rows) : nullptr;
  p.row_slots = l.row_slots;
  p.bp = (uint8_t*)(ws + l.bp);
  p.ops = (uint8_t*)(ws + l.ops);
  p.status = (int32_t*)(ws + l.status);
  if (launch_trace(p, l.groups, stream) != 0) return set_error(CHIRON_ERR_DEVICE, "%s: launch failed", who);
  std::vector<uint8_t> cols((size_t)columns);
  if (hipMemcpyAsync(status_out, ws + l.status, (size_t)pairs * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      (columns > 0 && hipMemcpyAsync(cols.data(), ws + l.ops, cols.size(), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the traceback kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  for (int64_t q = 0; q < pairs; ++q)
    if (status_out[q] == STATUS_INTERNAL) return set_error(CHIRON_ERR_STATE, "%s: pair %lld outgrew its workspace", who, (long long)q);
  // a pair whose (E, M) the kernel did not confirm keeps whatever its slice of ops_out held
  for (int64_t q = 0; q < pairs; ++q) {
    const int64_t len = ops_off[q + 1] - ops_off[q];
    if (status_out[q] == 0 && len > 0) memcpy(ops_out + ops_off[q], cols.data() + (ops_off[q] - ops_off[0]), (size_t)len);
  }
  return CHIRON_OK;
}
