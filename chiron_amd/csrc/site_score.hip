// Site scoring for `modcall` on gfx950: how well a short stretch of samples fits each of several short rows of expected levels,
// both ends fixed, by an exact DTW.  The definition is in include/chiron_amd.h and is restated in plain Python by tests/site_ref.py.
//
//   site_kernel  A lane a candidate; the candidates are dealt 64 at a time (a batch) to the launch's waves in a loop.  A lane keeps
//                its 16 columns and its 16 levels in registers, unrolled, and steps through its segment's samples; a row updates the
//                columns from the highest down, so that column n still sees the old column n - 1.  Column 0's left neighbour is a
//                value that is 0 before the first sample and INF after it: the path starts in column 0.  Lanes differ in L: the
//                columns at and above L have level 0, are computed and ignored, and column L - 1 is picked by a chain of selects
//                after the last sample.  Lanes differ in S: the wave runs to its longest segment and a lane past its own S keeps its
//                row.
//                The samples go through LDS in pieces of 64 samples a segment.  The lanes that are the lowest of their segment
//                are one ballot, and a segment's row in the slice is the number of such lanes below its own: every distinct
//                segment of the batch is loaded once a piece, a sample a lane (128 consecutive bytes), biased to unsigned 16 bits.
//                A row is 33 words, so rows r and r' share a bank only when r - r' is a multiple of 32, which among the rows of
//                lanes 0 .. 31 never happens; lanes of one segment read one address.  A lane reads its row two samples a word.
//                The slice is the wave's own: no workgroup barrier, and LDS operations of one wave execute in order.
//
// Costs are uint32 with INF = 2^30 for a column without a path: INF + 4096 * 65535 < 2^31, so nothing is clamped and nothing wraps,
// and a result at or above INF is "infeasible".  Every offset is 64-bit.  No scratch, no indexed register array, no workgroup
// barrier.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "site_pack.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_SITE_THREADS;
constexpr int WAVES = NT / 64;
constexpr int COLS = CHIRON_SITE_MAX_COLUMNS;         // columns a lane
constexpr int PIECE = 64;                             // samples of a segment that are staged at a time
constexpr int ROW_WORDS = PIECE / 2 + 1;              // a row of the slice: odd, so that consecutive rows fall on consecutive banks
constexpr unsigned INF = 1u << 30;                    // a column without a path; every real cost is below it
constexpr int BIAS = 32768;                           // samples and levels as unsigned: 0 .. 65535
static_assert(COLS == 16 && COLS == SITE_MAX_COLUMNS && CHIRON_SITE_MAX_SAMPLES == SITE_MAX_SAMPLES, "header and pack agree");
static_assert(CHIRON_SITE_INFEASIBLE == SITE_INFEASIBLE, "header and pack agree");
static_assert((unsigned long long)INF + (unsigned long long)CHIRON_SITE_MAX_SAMPLES * 65535 < (1ull << 31), "no clamp: INF plus every row stays below 2^31");
static_assert(NT % 64 == 0 && ROW_WORDS % 2 == 1, "whole waves; rows an odd number of words apart");

struct SiteParams {
  const int16_t* samples;            // the call's samples
  const int64_t* sample_off;         // [segments + 1], as the caller gave them: the kernel subtracts sample_off[0]
  const int32_t* level;              // the call's levels
  const int64_t* level_off;          // [candidates + 1], likewise
  const int32_t* seg;                // [candidates]
  int32_t* cost;                     // [candidates]
  int64_t candidates;
};

struct SiteLayout {
  size_t sample_off, samples, level_off, level, seg, cost, bytes;
};

typedef uint32_t __attribute__((may_alias)) word_t;    // the slice is written a sample and read a word

// One cell: the smaller of the column's own cost of the row before and its left neighbour's, plus |x - e|.
__device__ __forceinline__ unsigned cell(unsigned own, unsigned left, unsigned x, unsigned e) {
  return (left < own ? left : own) + (x > e ? x - e : e - x);
}

__global__ __launch_bounds__(CHIRON_SITE_THREADS) void site_kernel(SiteParams p) {
  __shared__ __attribute__((aligned(16))) uint16_t stage[WAVES][64 * ROW_WORDS * 2];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint16_t* mine = stage[wv];
  const int64_t batches = site_batches(p.candidates);
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  for (int64_t b = (int64_t)blockIdx.x * WAVES + wv; b < batches; b += nwaves) {
    const int64_t c = b * 64 + lane;
    const bool have = c < p.candidates;
    int sg = -1, S = 0, L = 1;
    int64_t x0 = 0, l0 = 0;
    if (have) {
      sg = p.seg[c];
      x0 = p.sample_off[sg] - p.sample_off[0];
      S = (int)(p.sample_off[sg + 1] - p.sample_off[sg]);
      l0 = p.level_off[c] - p.level_off[0];
      L = (int)(p.level_off[c + 1] - p.level_off[c]);
    }
    unsigned e[COLS], d[COLS];
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      e[k] = k < L && have ? (unsigned)(p.level[l0 + k] + BIAS) : 0u;
      d[k] = INF;
    }
    unsigned left = 0;                                            // what column 0 sees to its left: 0 before the first sample

    // the lowest lane of every lane's segment, and the segment's row in the slice
    int head = lane;
#pragma unroll 8
    for (int i = 63; i >= 0; --i)
      if (__builtin_amdgcn_readlane(sg, i) == sg) head = i;
    const unsigned long long heads = __builtin_amdgcn_ballot_w64(have && head == lane);
    const int row = __popcll(heads & ((1ull << head) - 1));       // head <= 63
    int longest = S;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const int other = __shfl_xor(longest, o, 64);
      longest = other > longest ? other : longest;
    }
    longest = __builtin_amdgcn_readfirstlane(longest);
    const word_t* my = reinterpret_cast<const word_t*>(mine) + row * ROW_WORDS;

    for (int t0 = 0; t0 < longest; t0 += PIECE) {
      int r = 0;
      for (unsigned long long m = heads; m; m &= m - 1, ++r) {   // every distinct segment once: row r, a sample a lane
        const int l = __builtin_ctzll(m);
        const int Sl = __builtin_amdgcn_readlane(S, l);
        if (t0 >= Sl) continue;                                   // the segment ended in an earlier piece: its lanes keep their rows
        const int64_t at = (((int64_t)__builtin_amdgcn_readlane((int)(x0 >> 32), l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)x0, l)) + t0 + lane;
        if (t0 + lane < Sl) mine[r * (ROW_WORDS * 2) + lane] = (uint16_t)((int)p.samples[at] + BIAS);
      }
      __builtin_amdgcn_wave_barrier();                            // wave-private slice: LDS operations of a wave execute in order
      const int steps = longest - t0 < PIECE ? longest - t0 : PIECE;
      for (int t = 0; t < steps; t += 8) {
        // four words, eight samples: the reads stay inside the row (t <= 56), and what lies past a lane's S is never used
        const unsigned w0 = my[(t >> 1) + 0], w1 = my[(t >> 1) + 1], w2 = my[(t >> 1) + 2], w3 = my[(t >> 1) + 3];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const unsigned w = u < 2 ? w0 : (u < 4 ? w1 : (u < 6 ? w2 : w3));
          const unsigned x = (u & 1) ? w >> 16 : w & 0xFFFFu;
          if (t0 + t + u < S) {
#pragma unroll
            for (int k = COLS - 1; k >= 1; --k) d[k] = cell(d[k], d[k - 1], x, e[k]);
            d[0] = cell(d[0], left, x, e[0]);
            left = INF;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();                            // the next piece overwrites the slice only after these reads
    }

    unsigned best = d[0];
#pragma unroll
    for (int k = 1; k < COLS; ++k) best = L - 1 == k ? d[k] : best;
    if (have) p.cost[c] = best >= INF ? CHIRON_SITE_INFEASIBLE : (int32_t)best;
  }
}

chiron_status site_sizes(const char* who, int64_t segments, int64_t samples, int64_t candidates, int64_t levels, SiteLayout* l) {
  if (segments < 0 || samples < 0 || candidates < 0 || levels < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative size (segments %lld, samples %lld, candidates %lld, levels %lld)", who, (long long)segments,
                     (long long)samples, (long long)candidates, (long long)levels);
  if (segments > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld segments in one call, at most 2^31 - 1", who, (long long)segments);
  if (samples > CHIRON_SIGNAL_MAX_SAMPLES)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld samples in one call, at most %d", who, (long long)samples, CHIRON_SIGNAL_MAX_SAMPLES);
  if (candidates > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld candidates in one call, at most 2^31 - 1", who, (long long)candidates);
  if (levels > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld levels in one call, at most 2^31 - 1", who, (long long)levels);
  l->sample_off = 0;
  l->samples = l->sample_off + up256((size_t)(segments + 1) * sizeof(int64_t));
  l->level_off = l->samples + up256((size_t)samples * sizeof(int16_t) + 16);
  l->level = l->level_off + up256((size_t)(candidates + 1) * sizeof(int64_t));
  l->seg = l->level + up256((size_t)levels * sizeof(int32_t));
  l->cost = l->seg + up256((size_t)candidates * sizeof(int32_t));
  l->bytes = l->cost + up256((size_t)candidates * sizeof(int32_t));
  return CHIRON_OK;
}

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_signal_score_workspace_size(int64_t segments, int64_t samples, int64_t candidates, int64_t levels, size_t* bytes) {
  const char* who = "chiron_signal_score_workspace_size";
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  SiteLayout l;
  if (chiron_status st = site_sizes(who, segments, samples, candidates, levels, &l)) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_signal_score(int32_t device_id, const int16_t* samples, const int64_t* sample_off, int64_t segments,
                                             const int32_t* level, const int64_t* level_off, const int32_t* seg, int64_t candidates,
                                             int32_t* cost_out, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream_) {
  const char* who = "chiron_signal_score";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  SiteLayout l;
  if (chiron_status st = site_sizes(who, segments, 0, candidates, 0, &l)) return st;
  if (candidates == 0) return CHIRON_OK;   // nothing to compute and nothing to write: no device is touched
  if (!level || !level_off || !seg) return set_error(CHIRON_ERR_INVALID, "%s: null level / level_off / seg", who);
  if (!cost_out) return set_error(CHIRON_ERR_INVALID, "%s: null cost_out", who);
  if (segments > 0 && !sample_off) return set_error(CHIRON_ERR_INVALID, "%s: null sample_off", who);
  int64_t n_samples = 0;
  if (segments > 0) {
    const SiteFinding f = site_check_segments(sample_off, segments);
    if (f.fault == SITE_OFF_NEGATIVE) return set_error(CHIRON_ERR_INVALID, "%s: sample_off[0] = %lld is negative", who, (long long)f.value);
    if (f.fault == SITE_OFF_ORDER)
      return set_error(CHIRON_ERR_INVALID, "%s: sample_off[%lld] = %lld below its predecessor %lld", who, (long long)f.at, (long long)f.value,
                       (long long)sample_off[f.at - 1]);
    if (f.fault == SITE_SEGMENT_LONG)
      return set_error(CHIRON_ERR_INVALID, "%s: segment %lld has %lld samples, at most %d", who, (long long)f.at, (long long)f.value, CHIRON_SITE_MAX_SAMPLES);
    n_samples = sample_off[segments] - sample_off[0];
  }
  if (n_samples > 0 && !samples) return set_error(CHIRON_ERR_INVALID, "%s: null samples", who);
  const SiteFinding f = site_check_candidates(level_off, seg, level, candidates, segments);
  if (f.fault == SITE_OFF_NEGATIVE) return set_error(CHIRON_ERR_INVALID, "%s: level_off[0] = %lld is negative", who, (long long)f.value);
  if (f.fault == SITE_OFF_ORDER)
    return set_error(CHIRON_ERR_INVALID, "%s: level_off[%lld] = %lld below its predecessor %lld", who, (long long)f.at, (long long)f.value,
                     (long long)level_off[f.at - 1]);
  if (f.fault == SITE_COLUMNS)
    return set_error(CHIRON_ERR_INVALID, "%s: candidate %lld has %lld levels, 1..%d are allowed", who, (long long)f.at, (long long)f.value, CHIRON_SITE_MAX_COLUMNS);
  if (f.fault == SITE_SEGMENT_INDEX)
    return set_error(CHIRON_ERR_INVALID, "%s: seg[%lld] = %lld outside 0..%lld, the call's segments", who, (long long)f.at, (long long)f.value,
                     (long long)segments - 1);
  if (f.fault == SITE_LEVEL_RANGE)
    return set_error(CHIRON_ERR_INVALID, "%s: level %lld of column %lld of candidate %lld outside -%d..%d", who, (long long)f.value, (long long)f.column,
                     (long long)f.at, SITE_LEVEL_MAX, SITE_LEVEL_MAX);
  const int64_t n_levels = level_off[candidates] - level_off[0];   // at most 16 a candidate: inside int64
  if (chiron_status st = site_sizes(who, segments, n_samples, candidates, n_levels, &l)) return st;
  if (!workspace) return set_error(CHIRON_ERR_INVALID, "%s: null workspace", who);
  if (workspace_bytes < l.bytes)
    return set_error(CHIRON_ERR_INVALID, "%s: a workspace of %llu bytes, %llu are needed", who, (unsigned long long)workspace_bytes, (unsigned long long)l.bytes);
  if (chiron_status st = use_device_workspace(who, device_id, workspace)) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.sample_off, sample_off, (size_t)(segments + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (n_samples > 0 &&
       hipMemcpyAsync(ws + l.samples, samples + sample_off[0], (size_t)n_samples * sizeof(int16_t), hipMemcpyHostToDevice, stream) != hipSuccess) ||
      hipMemcpyAsync(ws + l.level_off, level_off, (size_t)(candidates + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.level, level + level_off[0], (size_t)n_levels * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(ws + l.seg, seg, (size_t)candidates * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the segments and the candidates to the device failed", who);
  SiteParams p;
  p.samples = (const int16_t*)(ws + l.samples);
  p.sample_off = (const int64_t*)(ws + l.sample_off);
  p.level = (const int32_t*)(ws + l.level);
  p.level_off = (const int64_t*)(ws + l.level_off);
  p.seg = (const int32_t*)(ws + l.seg);
  p.cost = (int32_t*)(ws + l.cost);
  p.candidates = candidates;
  const int64_t want = (site_batches(candidates) + WAVES - 1) / WAVES;
  const dim3 grid((unsigned)(want < CHIRON_SITE_MAX_GROUPS ? want : CHIRON_SITE_MAX_GROUPS));
  hipLaunchKernelGGL(site_kernel, grid, dim3(NT), 0, stream, p);
  if (chiron_status st = launched(who)) return st;
  if (hipMemcpyAsync(cost_out, ws + l.cost, (size_t)candidates * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the site kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  return CHIRON_OK;
}
