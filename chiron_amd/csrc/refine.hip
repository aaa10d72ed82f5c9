// Signal refinement for `squiggle --refine` on gfx950: the borders between a read's bases moved to where the samples change level,
// by an exact banded DTW of the samples against the bases' expected levels.  The definition is in include/chiron_amd.h and is
// restated in plain Python by tests/refine_ref.py.
//
//   refine_kernel  A wave an item; the items are dealt to the launch's waves in a loop.  The borders 1 .. L are rows that run in
//                  sequence, the 64 lanes are the candidates a[n] - 32 + lane of border n.  Borders 0 and L have one candidate,
//                  lane 32, so every row has the same shape.  Row n, from row n-1, with e the level of base n-1, w = a[n-1] - 32
//                  and d = a[n] - a[n-1]:
//                    - the samples w .. w + d + 64) that the two windows span are loaded in pieces of 64, a sample a lane, and only
//                      where they lie inside a[0] .. a[L]) (elsewhere 0: no candidate out there is valid);
//                    - piece 0 gives P at the old candidates by an int32 wave scan of |x - e| (a piece sums below 2^23); the pieces
//                      between add up lane by lane in int64 and are reduced once; the last one or two pieces, scanned, give P at
//                      the new candidates with that int64 carry; the scans are DPP steps (row_shr 1, 2, 4, 8, row_bcast 15, 31);
//                    - G = F - P, an int64 wave prefix-min M of it, and new lane j takes M at old lane min(j + d - 1, 63): the
//                      old candidates below its own.  F = M + P, or no value where there is none.
//                    - the lanes whose G is below every G before them are one ballot: the row's mask, 8 bytes in the workspace.
//                  The predecessor of candidate j of row n is the highest set bit of the mask at or below min(j + d - 1, 63):
//                  the first lane that reaches the prefix minimum, which is the smallest s' that attains it.  After its forward
//                  pass the same wave walks back from lane 32 of row L: it loads 64 masks and shifts with one load each and steps
//                  through them with cross-lane reads; lane r of the chunk keeps the start of its row and stores it.
//
// Every offset is 64-bit.  No LDS, no scratch, no indexed register array, no workgroup barrier.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "refine_pack.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_REFINE_THREADS;
constexpr int WAVES = NT / 64;
constexpr int HALF = CHIRON_REFINE_HALF;
constexpr long long NONE = CHIRON_REFINE_INFEASIBLE;   // a candidate without a value; every real cost is below 2^47
static_assert(2 * HALF == 64, "a border's candidates are the lanes of one wave");
static_assert(NT % 64 == 0, "whole waves");
static_assert(64ll * (32767 + REFINE_LEVEL_MAX + 1) < (1ll << 23), "a piece of |x - e| sums below 2^23: int32 scans");

struct RefineParams {
  const int16_t* samples;            // the call's samples
  const int64_t* sample_off;         // [items + 1], as the caller gave them: the kernel subtracts sample_off[0]
  const int64_t* base_off;           // [items + 1], likewise
  const int32_t* level;              // [bases]
  const int32_t* start_in;           // [bases + items]
  int32_t* start_out;                // [bases + items]
  unsigned long long* mask;          // [bases]: row n of an item at its base n - 1
  long long* cost;                   // [items]
  int64_t items;
};

struct RefineLayout {
  size_t sample_off, base_off, samples, level, start_in, start_out, mask, cost, bytes;
};

// One DPP step: lane i takes v of the lane the control names, or `old` where that lane lies outside the row or the row is masked
// out.  0x111 / 0x112 / 0x114 / 0x118: row_shr 1 / 2 / 4 / 8 within rows of 16 lanes; 0x142: row_bcast15, lane 15 of a row to the
// whole next row (row mask 0xa: rows 1 and 3); 0x143: row_bcast31, lane 31 to rows 2 and 3 (row mask 0xc).
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWS, 0xf, false);
}

// inclusive wave scan of a sum: four steps inside the rows, two across them; the last lane holds the piece's total
__device__ __forceinline__ int scan_add(int v) {
  v += dpp<0x111, 0xf>(0, v);
  v += dpp<0x112, 0xf>(0, v);
  v += dpp<0x114, 0xf>(0, v);
  v += dpp<0x118, 0xf>(0, v);
  v += dpp<0x142, 0xa>(0, v);
  v += dpp<0x143, 0xc>(0, v);
  return v;
}

template <int CTRL, int ROWS>
__device__ __forceinline__ long long min_step(long long v) {
  const int lo = dpp<CTRL, ROWS>((int)0xFFFFFFFF, (int)v), hi = dpp<CTRL, ROWS>(0x7FFFFFFF, (int)(v >> 32));   // NONE where no lane
  const long long u = ((long long)hi << 32) | (unsigned)lo;
  return u < v ? u : v;
}

// inclusive wave scan of a minimum
__device__ __forceinline__ long long scan_min(long long v) {
  v = min_step<0x111, 0xf>(v);
  v = min_step<0x112, 0xf>(v);
  v = min_step<0x114, 0xf>(v);
  v = min_step<0x118, 0xf>(v);
  v = min_step<0x142, 0xa>(v);
  v = min_step<0x143, 0xc>(v);
  return v;
}

// lane l of v for the whole wave, l uniform
__device__ __forceinline__ long long lane_of(long long v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)v, l), hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
  return ((long long)hi << 32) | (unsigned)lo;
}

__global__ __launch_bounds__(CHIRON_REFINE_THREADS) void refine_kernel(RefineParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  for (int64_t it = wave; it < p.items; it += nwaves) {
    const int64_t b0 = p.base_off[it] - p.base_off[0];
    const int64_t L = p.base_off[it + 1] - p.base_off[it];
    const int16_t* __restrict__ x = p.samples + (p.sample_off[it] - p.sample_off[0]);
    const int32_t* __restrict__ e = p.level + b0;
    const int32_t* __restrict__ a = p.start_in + b0 + it;
    int32_t* __restrict__ out = p.start_out + b0 + it;
    unsigned long long* __restrict__ mask = p.mask + b0;
    const int64_t a0 = a[0], aL = a[L];

    // ---- forward: rows 1 .. L -------------------------------------------------------------------------------------------
    long long F = lane == HALF ? 0 : NONE;
    int64_t a_prev = a0;
    int ev = 0, av = 0;
    for (int64_t n = 1; n <= L; ++n) {
      const int r = (int)((n - 1) & 63);
      if (r == 0) {   // the levels and starts of the next 64 rows, a row a lane
        const int64_t at = n - 1 + lane;
        ev = at < L ? e[at] : 0;
        av = at < L ? a[at + 1] : 0;
      }
      const int lv = __builtin_amdgcn_readlane(ev, r);
      const int64_t a_cur = __builtin_amdgcn_readlane(av, r);
      const int64_t w = a_prev - HALF, d = a_cur - a_prev;
      const int64_t kd = d >> 6;
      const int rem = (int)(d & 63);
      auto piece = [&](int64_t k) -> int {   // |x - e| at sample w + 64 k + lane, 0 outside the item's span
        const int64_t pos = w + k * 64 + lane;
        int v = 0;
        if (pos >= a0 && pos < aL) {
          v = (int)x[pos] - lv;
          v = v < 0 ? -v : v;
        }
        return v;
      };
      const int v0 = piece(0);
      const int i0 = scan_add(v0);
      const int P_old = i0 - v0;                                  // P at old candidate `lane`, from w
      long long carry = 0;                                        // P at the first sample of piece kd
      int vA = v0, iA = i0;
      if (kd > 0) {
        long long between = 0;
        for (int64_t k = 1; k < kd; ++k) between += piece(k);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) between += __shfl_xor(between, o, 64);
        carry = (long long)__builtin_amdgcn_readlane(i0, 63) + between;
        vA = piece(kd);
        iA = scan_add(vA);
      }
      int eB = 0;                                                 // the piece behind it, which new candidates reach when rem > 0
      if (rem > 0) {
        const int vB = piece(kd + 1);
        eB = scan_add(vB) - vB;
      }
      const int eA = iA - vA, tA = __builtin_amdgcn_readlane(iA, 63);
      const int to = rem + lane;                                  // new candidate `lane` is sample to of piece kd
      const int pa = __shfl(eA, to & 63, 64), pb = __shfl(eB, to & 63, 64);
      const long long P_new = carry + (to < 64 ? pa : tA + pb);

      const long long G = F == NONE ? NONE : F - P_old;
      const long long M = scan_min(G);
      long long before = __shfl_up(M, 1, 64);
      if (lane == 0) before = NONE;
      const unsigned long long flags = __ballot(G < before);
      if (lane == 0) mask[n - 1] = flags;
      const int reach = lane + (int)(d < 64 ? d : 64) - 1;        // the highest old lane below this candidate
      const long long m = __shfl(M, reach < 0 ? 0 : (reach > 63 ? 63 : reach), 64);
      const int64_t s = a_cur - HALF + lane;
      const bool live = (n < L || lane == HALF) && s >= a0 && s <= aL && reach >= 0 && m != NONE;
      F = live ? m + P_new : NONE;
      a_prev = a_cur;
    }

    // ---- back: from lane 32 of row L ------------------------------------------------------------------------------------
    const long long cost = lane_of(F, HALF);
    if (cost == NONE) {
      for (int64_t i = lane; i <= L; i += 64) out[i] = a[i];
      if (lane == 0) p.cost[it] = NONE;
      continue;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");        // lane 0 wrote the masks, every lane reads them
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    int j = HALF;
    for (int64_t hi = L; hi >= 1; hi -= 64) {
      const int64_t lo = hi > 63 ? hi - 63 : 1;                   // rows lo .. hi, row lo + lane on lane `lane`
      const int64_t n = lo + lane;
      unsigned long long mk = 0;
      int shift = 0, ap = 0;
      if (n <= hi) {
        mk = mask[n - 1];
        ap = a[n - 1];
        const int64_t d = (int64_t)a[n] - ap;
        shift = (int)(d < 64 ? d : 64);
      }
      int mine = 0;
      for (int r = (int)(hi - lo); r >= 0; --r) {
        const unsigned long long row = (unsigned long long)lane_of((long long)mk, r);
        int reach = j + __builtin_amdgcn_readlane(shift, r) - 1;
        reach = reach > 63 ? 63 : reach;
        const unsigned long long bits = reach < 0 ? 0ull : row & (~0ull >> (63 - reach));
        j = bits ? 63 - __clzll((long long)bits) : 0;             // a finite cost has a predecessor on every row
        if (lane == r) mine = j;
      }
      if (n <= hi) out[n - 1] = ap - HALF + mine;
    }
    if (lane == 0) {
      out[L] = (int32_t)aL;
      p.cost[it] = cost;
    }
  }
}

chiron_status refine_sizes(const char* who, int64_t items, int64_t samples, int64_t bases, RefineLayout* l) {
  if (items < 0 || samples < 0 || bases < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative size (items %lld, samples %lld, bases %lld)", who, (long long)items, (long long)samples,
                     (long long)bases);
  if (items > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items in one call, at most 2^31 - 1", who, (long long)items);
  if (samples > CHIRON_SIGNAL_MAX_SAMPLES)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld samples in one call, at most %d", who, (long long)samples, CHIRON_SIGNAL_MAX_SAMPLES);
  if (bases > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld bases in one call, at most 2^31 - 1", who, (long long)bases);
  const size_t offs = items > 0 ? (size_t)(items + 1) * sizeof(int64_t) : 0;
  const size_t starts = items > 0 ? (size_t)(bases + items) * sizeof(int32_t) : 0;
  l->sample_off = 0;
  l->base_off = l->sample_off + up256(offs);
  l->samples = l->base_off + up256(offs);
  l->level = l->samples + up256((size_t)samples * sizeof(int16_t));
  l->start_in = l->level + up256((size_t)bases * sizeof(int32_t));
  l->start_out = l->start_in + up256(starts);
  l->mask = l->start_out + up256(starts);
  l->cost = l->mask + up256((size_t)bases * sizeof(int64_t));
  l->bytes = l->cost + up256((size_t)items * sizeof(int64_t));
  return CHIRON_OK;
}

// off[0 .. items] of sample_off or base_off: starts at or above 0 and never decreases
chiron_status check_item_offsets(const char* who, const char* name, const int64_t* off, int64_t items) {
  if (off[0] < 0) return set_error(CHIRON_ERR_INVALID, "%s: %s[0] = %lld is negative", who, name, (long long)off[0]);
  for (int64_t i = 0; i < items; ++i)
    if (off[i + 1] < off[i])
      return set_error(CHIRON_ERR_INVALID, "%s: %s[%lld] = %lld below its predecessor %lld", who, name, (long long)(i + 1), (long long)off[i + 1],
                       (long long)off[i]);
  return CHIRON_OK;
}

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_signal_refine_workspace_size(int64_t items, int64_t samples, int64_t bases, size_t* bytes) {
  const char* who = "chiron_signal_refine_workspace_size";
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  RefineLayout l;
  if (chiron_status st = refine_sizes(who, items, samples, bases, &l)) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_signal_refine(int32_t device_id, const int16_t* samples, const int64_t* sample_off, const int32_t* level,
                                              const int32_t* start_in, const int64_t* base_off, int64_t items, uint32_t flags,
                                              int32_t* start_out, int64_t* cost_out, void* workspace, void* stream_) {
  const char* who = "chiron_signal_refine";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  RefineLayout l;
  if (chiron_status st = refine_sizes(who, items, 0, 0, &l)) return st;
  if (items == 0) return CHIRON_OK;   // nothing to compute and nothing to write: no device is touched
  if (!sample_off || !base_off || !start_in) return set_error(CHIRON_ERR_INVALID, "%s: null sample_off / base_off / start_in", who);
  if (!start_out || !cost_out) return set_error(CHIRON_ERR_INVALID, "%s: null start_out / cost_out", who);
  if (chiron_status st = check_item_offsets(who, "sample_off", sample_off, items)) return st;
  if (chiron_status st = check_item_offsets(who, "base_off", base_off, items)) return st;
  const int64_t n_samples = sample_off[items] - sample_off[0], n_bases = base_off[items] - base_off[0];
  if (chiron_status st = refine_sizes(who, items, n_samples, n_bases, &l)) return st;
  if (n_bases > 0 && !level) return set_error(CHIRON_ERR_INVALID, "%s: null level", who);
  if (n_samples > 0 && !samples) return set_error(CHIRON_ERR_INVALID, "%s: null samples", who);
  for (int64_t i = 0; i < items; ++i) {
    const int64_t L = base_off[i + 1] - base_off[i], S = sample_off[i + 1] - sample_off[i];
    const RefineFinding f = refine_check_item(start_in + base_off[i] + i, level ? level + base_off[i] : nullptr, L, S);
    if (f.fault == REFINE_START_RANGE)
      return set_error(CHIRON_ERR_INVALID, "%s: start entry %lld of item %lld = %lld outside 0..%lld, its samples", who, (long long)f.at, (long long)i,
                       (long long)f.value, (long long)S);
    if (f.fault == REFINE_START_ORDER)
      return set_error(CHIRON_ERR_INVALID, "%s: start entry %lld of item %lld = %lld below its predecessor", who, (long long)f.at, (long long)i,
                       (long long)f.value);
    if (f.fault == REFINE_LEVEL_RANGE)
      return set_error(CHIRON_ERR_INVALID, "%s: level %lld of base %lld of item %lld outside -%d..%d", who, (long long)f.value, (long long)f.at,
                       (long long)i, REFINE_LEVEL_MAX, REFINE_LEVEL_MAX);
  }
  const int32_t* first_start = start_in + base_off[0];
  if (n_bases == 0) {   // no border to move: no device is touched
    refine_without_bases(first_start, items, start_out, cost_out);
    return CHIRON_OK;
  }
  if (chiron_status st = use_device_workspace(who, device_id, workspace)) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  const size_t off_bytes = (size_t)(items + 1) * sizeof(int64_t), start_bytes = (size_t)(n_bases + items) * sizeof(int32_t);
  if (hipMemcpyAsync(ws + l.sample_off, sample_off, off_bytes, hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.base_off, base_off, off_bytes, hipMemcpyHostToDevice, stream) != hipSuccess ||
      (n_samples > 0 &&
       hipMemcpyAsync(ws + l.samples, samples + sample_off[0], (size_t)n_samples * sizeof(int16_t), hipMemcpyHostToDevice, stream) != hipSuccess) ||
      hipMemcpyAsync(ws + l.level, level + base_off[0], (size_t)n_bases * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.start_in, first_start, start_bytes, hipMemcpyHostToDevice, stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the items to the device failed", who);
  RefineParams p;
  p.samples = (const int16_t*)(ws + l.samples);
  p.sample_off = (const int64_t*)(ws + l.sample_off);
  p.base_off = (const int64_t*)(ws + l.base_off);
  p.level = (const int32_t*)(ws + l.level);
  p.start_in = (const int32_t*)(ws + l.start_in);
  p.start_out = (int32_t*)(ws + l.start_out);
  p.mask = (unsigned long long*)(ws + l.mask);
  p.cost = (long long*)(ws + l.cost);
  p.items = items;
  const int64_t want = (items + WAVES - 1) / WAVES;
  const dim3 grid((unsigned)(want < CHIRON_REFINE_MAX_GROUPS ? want : CHIRON_REFINE_MAX_GROUPS));
  hipLaunchKernelGGL(refine_kernel, grid, dim3(NT), 0, stream, p);
  if (chiron_status st = launched(who)) return st;
  if (hipMemcpyAsync(start_out, ws + l.start_out, start_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(cost_out, ws + l.cost, (size_t)items * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the refine kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  return CHIRON_OK;
}
