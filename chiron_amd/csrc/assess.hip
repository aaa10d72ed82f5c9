// Read-level assessment on gfx950: global alignment of a read against its reference, unit costs, exact (E, M) per pair.
//
//   E = Levenshtein distance, M = most matching columns over the alignments of cost E          (include/chiron_amd.h)
//
// One 64-bit key per DP cell carries both: key = E * 2^32 - M.  A match adds -1, a mismatch or a gap adds 2^32, and the
// recurrence is a three-way min: the smallest key is the smallest E and, among those, the largest M (M < 2^31 never borrows
// from E's half).
//
// Work mapping: one workgroup per pair, the anti-diagonal wavefront of align_common.h (band_sweep) over a band of diagonals
// d = j - i in [min(0, m-n) - w, max(0, m-n) + w]: one array indexed by d, one barrier per step, the array in LDS while the band
// has at most CHIRON_ALIGN_LDS_SLOTS diagonals and in the workgroup's workspace row beyond that.  Only the origin is a border
// cell, and the result is cell (n, m).
//
// Exactness: the path starts on diagonal 0 and ends on diagonal m-n, and only a gap changes the diagonal, by one.  To touch a
// diagonal outside the band a path needs at least w + 1 gaps to get there from the nearer end of [0, m-n], w + 1 to come back,
// and |m-n| more to cover the distance between the ends: 2(w+1) + |m-n| in all.  So when the banded minimum satisfies
// E <= 2w + 1 + |m-n|, every path of cost <= E lies inside the band: E is the true distance and every optimal alignment was
// seen, so M is exact as well.  Otherwise w doubles and the pair is redone, up to the full table; all inside the kernel, so a
// batch is one launch.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "kernels.h"

namespace chiron {

namespace {

struct GlobalCell {
  static constexpr int64_t EDIT = KEY32_EDIT, MATCH = -1;
  static constexpr bool FREE_ROW0 = false;
  __device__ static int64_t border(int k, int, int) { return k == 0 ? 0 : (int64_t)1 << 60; }
};

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
      const Diagonals bd = band_clip(n, m, w);
      const bool full = bd.dlo == -n && bd.dhi == m;
      int64_t key;
      const bool fits = with_row(lds_row, ws_row, bd.dhi - bd.dlo + 1, p.row_slots, [&](int64_t* row) {
        band_sweep<GlobalCell>(row, a, b, n, m, bd.dlo, bd.dhi);
        key = row[(m - n) - bd.dlo];
        __syncthreads();   // every thread has read the result before the next pass writes the array
      });
      if (!fits) {
        E = -1;
        M = 0;
        break;
      }
      key32_decode(key, &E, &M);
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

void pair_layout(int64_t pairs, int64_t code_bytes, int out_words, int64_t table, AlignLayout* l) {
  // the callers keep pairs <= 2^24 and code_bytes, table < 2^21: every product below stays under 2^48
  l->groups = (int)(pairs < CHIRON_ALIGN_MAX_GROUPS ? pairs : CHIRON_ALIGN_MAX_GROUPS);
  l->row_slots = table > CHIRON_ALIGN_LDS_SLOTS ? table + 1 : 0;
  l->pair = 0;
  l->out = l->pair + up256((size_t)pairs * sizeof(AlignPair));
  l->codes = l->out + up256((size_t)pairs * (size_t)out_words * sizeof(int32_t));
  l->rows = l->codes + up256((size_t)pairs * (size_t)code_bytes);
  l->bytes = l->rows + up256((size_t)l->groups * (size_t)l->row_slots * sizeof(int64_t));
}

AlignParams align_params(void* workspace, const AlignLayout& l, int64_t pairs, int32_t band0) {
  char* ws = (char*)workspace;
  AlignParams p;
  p.codes = (const uint8_t*)(ws + l.codes);
  p.pair = (const AlignPair*)(ws + l.pair);
  p.pairs = pairs;
  p.rows = l.row_slots ? (int64_t*)(ws + l.rows) : nullptr;
  p.row_slots = l.row_slots;
  p.out = (int32_t*)(ws + l.out);
  p.band0 = band0;
  return p;
}

chiron_status align_layout(int64_t pairs, int64_t max_len, AlignLayout* l) {
  if (pairs < 0 || max_len < 0) return set_error(CHIRON_ERR_INVALID, "align: negative pairs / max_len");
  if (max_len > CHIRON_ALIGN_MAX_LEN)
    return set_error(CHIRON_ERR_OVERFLOW, "align: a sequence of %lld bases, the kernel takes at most %d", (long long)max_len, CHIRON_ALIGN_MAX_LEN);
  if (pairs > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "align: %lld pairs in one call, at most 2^24", (long long)pairs);
  pair_layout(pairs, 2 * max_len, 3, 2 * max_len + 1, l);
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
  const char* const who = "chiron_align_pairs";
  if (pairs < 0) return set_error(CHIRON_ERR_INVALID, "%s: pairs %lld", who, (long long)pairs);
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  if (pairs == 0) return CHIRON_OK;
  if (pairs > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld pairs in one call, at most 2^24", who, (long long)pairs);
  if (!read_off || !ref_off || !edit_out || !match_out || !band_out) return set_error(CHIRON_ERR_INVALID, "%s: null operand", who);
  // offsets first (they bound what may be read of `codes`), then the codes while they are packed pair by pair
  int64_t max_len = 0, total = 0;
  chiron_status st = check_offsets(who, "read", "read", "bases", read_off, pairs, CHIRON_ALIGN_MAX_LEN, &max_len, &total);
  if (!st) st = check_offsets(who, "ref", "reference", "bases", ref_off, pairs, CHIRON_ALIGN_MAX_LEN, &max_len, &total);
  if (st) return st;
  if (total > 0 && !codes) return set_error(CHIRON_ERR_INVALID, "%s: null codes", who);
  std::vector<uint8_t> packed((size_t)total);
  std::vector<AlignPair> recs((size_t)pairs);
  AlignLayout l;
  if ((st = pack_codes(who, "read", "reference", codes, read_off, ref_off, pairs, recs.data(), packed.data()))) return st;
  if ((st = align_layout(pairs, max_len, &l))) return st;
  if ((st = use_device_workspace(who, device_id, workspace))) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.pair, recs.data(), recs.size() * sizeof(AlignPair), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (total > 0 && hipMemcpyAsync(ws + l.codes, packed.data(), packed.size(), hipMemcpyHostToDevice, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the pairs to the device failed", who);
  if (launch_align(align_params(workspace, l, pairs, 0), l.groups, stream) != 0) return set_error(CHIRON_ERR_DEVICE, "%s: launch failed", who);
  std::vector<int32_t> out((size_t)pairs * 3);
  if (hipMemcpyAsync(out.data(), ws + l.out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the alignment kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  for (int64_t q = 0; q < pairs; ++q) {
    if (out[q * 3] < 0) return set_error(CHIRON_ERR_STATE, "%s: pair %lld outgrew its workspace row", who, (long long)q);
    edit_out[q] = out[q * 3];
    match_out[q] = out[q * 3 + 1];
    band_out[q] = out[q * 3 + 2];
  }
  return CHIRON_OK;
}
