// Signal levels for `squiggle` on gfx950: the mean current of every base's samples, and per bin (a genome position and strand, or a
// k-mer) the number of bases, their samples and the sum and squared sum of their levels.  The definition is in
// include/chiron_amd.h and is restated in plain Python by tests/squiggle_ref.py.
//
//   signal_kernel  Flat over bases, a base a lane: given the host's per-base record (first sample, count, bin: signal_pack.h) bases
//                  are independent, so there is no scan and no workgroup a read (pileup.hip has one, and idles on few long reads).
//                  Chunks of 64 consecutive bases are dealt to the launch's waves round-robin.  The records of a call are in sample
//                  order, so a chunk owns ONE run of samples, lo .. hi): within a read it is contiguous, across reads it also holds
//                  the samples nobody owns (a read's unlabelled head, a read without bases), which are loaded and not used; a whole
//                  piece of them is skipped.  The wave stages the run through its own LDS slice PIECE samples at a time, 16 bytes
//                  a lane and load, each sample loaded once; a lane then sums the intersection of its span with the piece out of LDS, in 32 bits (PIECE * 2^15
//                  < 2^31) and adds that to its 64-bit sum.  A 5000-sample stall costs its wave five pieces; no lane walks global
//                  memory an element at a time.  The slice is the wave's own, so no barrier: LDS operations of a wave execute in
//                  order.
//                  The level goes out with a plain store; the planes get four relaxed agent-scope 64-bit atomic adds whose result is
//                  unused (global_atomic_add_x2).  Integer sums: the result does not depend on their order.
//
// Every offset is 64-bit.  No scratch, no indexed register array.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "signal_pack.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_SIGNAL_THREADS;
constexpr int WAVES = NT / 64;
constexpr int PIECE = 1024;                  // samples a wave stages at once: 2 KiB of LDS a wave
constexpr int LOADS = PIECE / (64 * 8);      // 16-byte loads a lane and piece
static_assert(PIECE % (64 * 8) == 0, "a piece is whole 16-byte loads of a whole wave");
static_assert((int64_t)PIECE * 32768 < ((int64_t)1 << 31), "a lane's sum over one piece fits 32 bits");
static_assert(CHIRON_SIGNAL_PLANES == 4, "events, dwell, sum, squared sum");

struct SignalParams {
  const SignalBase* rec;     // [bases], in sample order
  const int16_t* samples;    // the call's samples, the part padded to a multiple of 256 bytes
  int32_t* level;            // [bases] or null
  long long* planes;         // [4][bins] or null (bins == 0)
  int64_t bases;
  int64_t bins;
};

struct SignalLayout {
  size_t rec, samples, level, planes, bytes;
};

__device__ __forceinline__ void add_to(long long* p, long long v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CHIRON_SIGNAL_THREADS) void signal_kernel(SignalParams p) {
  __shared__ __attribute__((aligned(16))) int16_t stage[WAVES][PIECE];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int16_t* mine = stage[wv];
  const int64_t wave = (int64_t)blockIdx.x * WAVES + wv;
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  const int64_t chunks = (p.bases + 63) >> 6;
  for (int64_t c = wave; c < chunks; c += nwaves) {
    const int64_t b = c * 64 + lane;
    const bool have = b < p.bases;
    int64_t first = 0;
    int count = 0, bin = -1;
    if (have) {
      const SignalBase r = p.rec[b];
      first = r.first;
      count = r.count;
      bin = r.bin;
    }
    const int64_t end = first + count;
    // the chunk's run of samples: the records are in sample order, so it is first of the first span .. end of the last one
    long long lo = count > 0 ? first : 0x7FFFFFFFFFFFFFFFll, hi = count > 0 ? end : 0;
    for (int o = 32; o >= 1; o >>= 1) {
      const long long lo2 = __shfl_xor(lo, o, 64), hi2 = __shfl_xor(hi, o, 64);
      lo = lo2 < lo ? lo2 : lo;
      hi = hi2 > hi ? hi2 : hi;
    }
    int64_t sum = 0;
    // pieces start on a 16-byte boundary of the sample array; a chunk without a sample has lo > hi and stages nothing
    for (int64_t pos = lo & ~(int64_t)7; pos < hi; pos += PIECE) {
      const int64_t a = first > pos ? first : pos, z = end < pos + PIECE ? end : pos + PIECE;
      const int ia = a < z ? (int)(a - pos) : 0, iz = a < z ? (int)(z - pos) : 0;
      if (__builtin_amdgcn_ballot_w64(a < z) == 0) continue;   // a piece nobody owns a sample of (a long unlabelled head): not loaded
#pragma unroll
      for (int k = 0; k < LOADS; ++k) {
        const int at = (k * 64 + lane) * 8;
        // a load that starts below hi ends inside the padded sample array; what it reads past hi is never summed
        if (pos + at < hi) *reinterpret_cast<int4*>(mine + at) = *reinterpret_cast<const int4*>(p.samples + pos + at);
      }
      __builtin_amdgcn_wave_barrier();   // wave-private slice: LDS operations of a wave execute in order
      int part = 0;
      for (int i = ia; i < iz; ++i) part += mine[i];
      sum += part;
      __builtin_amdgcn_wave_barrier();   // the next piece overwrites the slice only after these reads
    }
    if (have) {
      int level = CHIRON_SIGNAL_EMPTY;
      if (count > 0) {
        level = signal_level(sum, count);
        if (bin >= 0) {
          long long* at = p.planes + bin;
          add_to(at, 1);
          add_to(at + p.bins, count);
          add_to(at + 2 * p.bins, level);
          add_to(at + 3 * p.bins, (long long)level * level);
        }
      }
      if (p.level) p.level[b] = level;
    }
  }
}

chiron_status signal_sizes(const char* who, int64_t reads, int64_t samples, int64_t bases, int64_t bins, bool levels, SignalLayout* l) {
  if (reads < 0 || samples < 0 || bases < 0 || bins < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative size (reads %lld, samples %lld, bases %lld, bins %lld)", who, (long long)reads,
                     (long long)samples, (long long)bases, (long long)bins);
  if (samples > CHIRON_SIGNAL_MAX_SAMPLES)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld samples in one call, at most %d", who, (long long)samples, CHIRON_SIGNAL_MAX_SAMPLES);
  if (bases > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld bases in one call, at most 2^31 - 1", who, (long long)bases);
  if (bins > CHIRON_SIGNAL_MAX_BINS)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld bins in one call, at most %d", who, (long long)bins, CHIRON_SIGNAL_MAX_BINS);
  l->rec = 0;
  l->samples = l->rec + up256((size_t)bases * sizeof(SignalBase));
  l->level = l->samples + up256((size_t)samples * sizeof(int16_t));
  l->planes = l->level + up256(levels ? (size_t)bases * sizeof(int32_t) : 0);
  l->bytes = l->planes + up256((size_t)CHIRON_SIGNAL_PLANES * (size_t)bins * sizeof(int64_t));
  return CHIRON_OK;
}

// off[0 .. reads] of sample_off or base_off: starts at or above 0 and never decreases
chiron_status check_read_offsets(const char* who, const char* name, const int64_t* off, int64_t reads) {
  if (off[0] < 0) return set_error(CHIRON_ERR_INVALID, "%s: %s[0] = %lld is negative", who, name, (long long)off[0]);
  for (int64_t r = 0; r < reads; ++r)
    if (off[r + 1] < off[r])
      return set_error(CHIRON_ERR_INVALID, "%s: %s[%lld] = %lld below its predecessor %lld", who, name, (long long)(r + 1), (long long)off[r + 1],
                       (long long)off[r]);
  return CHIRON_OK;
}

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_signal_workspace_size(int64_t reads, int64_t samples, int64_t bases, int64_t bins, int32_t want_levels, size_t* bytes) {
  const char* who = "chiron_signal_workspace_size";
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  SignalLayout l;
  if (chiron_status st = signal_sizes(who, reads, samples, bases, bins, want_levels != 0, &l)) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_signal_levels(int32_t device_id, const int16_t* samples, const int64_t* sample_off, const int32_t* start,
                                              const int64_t* base_off, const int32_t* bin, int64_t reads, int64_t bins, uint32_t flags,
                                              int64_t* planes_out, int32_t* level_out, void* workspace, void* stream_) {
  const char* who = "chiron_signal_levels";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  SignalLayout l;
  if (chiron_status st = signal_sizes(who, reads, 0, 0, bins, false, &l)) return st;
  if (bins > 0 && !planes_out) return set_error(CHIRON_ERR_INVALID, "%s: null planes_out with %lld bins", who, (long long)bins);
  if (reads > 0 && (!sample_off || !base_off || !start)) return set_error(CHIRON_ERR_INVALID, "%s: null sample_off / base_off / start", who);
  int64_t n_samples = 0, n_bases = 0;
  if (reads > 0) {
    if (chiron_status st = check_read_offsets(who, "sample_off", sample_off, reads)) return st;
    if (chiron_status st = check_read_offsets(who, "base_off", base_off, reads)) return st;
    n_samples = sample_off[reads] - sample_off[0];
    n_bases = base_off[reads] - base_off[0];
  }
  const bool levels = level_out != nullptr && n_bases > 0;
  if (chiron_status st = signal_sizes(who, reads, n_samples, n_bases, bins, levels, &l)) return st;
  if (n_bases > 0 && !bin) return set_error(CHIRON_ERR_INVALID, "%s: null bin", who);
  if (n_samples > 0 && !samples) return set_error(CHIRON_ERR_INVALID, "%s: null samples", who);
  // the walk over every base: its checks and, on the way, the record the kernel reads
  std::unique_ptr<SignalBase[]> recs(n_bases > 0 ? new (std::nothrow) SignalBase[(size_t)n_bases] : nullptr);
  if (n_bases > 0 && !recs) return set_error(CHIRON_ERR_STATE, "%s: no host memory for the records of %lld bases", who, (long long)n_bases);
  for (int64_t r = 0; r < reads; ++r) {
    const int64_t L = base_off[r + 1] - base_off[r], S = sample_off[r + 1] - sample_off[r];
    const SignalFinding f = signal_pack_read(start + base_off[r] + r, bin ? bin + base_off[r] : nullptr, L, S, sample_off[r] - sample_off[0], bins,
                                             recs.get() + (base_off[r] - base_off[0]));
    if (f.fault == SIGNAL_START_RANGE)
      return set_error(CHIRON_ERR_INVALID, "%s: start entry %lld of read %lld = %lld outside 0..%lld, its samples", who, (long long)f.at, (long long)r,
                       (long long)f.value, (long long)S);
    if (f.fault == SIGNAL_START_ORDER)
      return set_error(CHIRON_ERR_INVALID, "%s: start entry %lld of read %lld = %lld below its predecessor", who, (long long)f.at, (long long)r,
                       (long long)f.value);
    if (f.fault == SIGNAL_BIN_RANGE)
      return set_error(CHIRON_ERR_INVALID, "%s: bin %lld of base %lld of read %lld outside -1..%lld", who, (long long)f.value, (long long)f.at,
                       (long long)r, (long long)bins - 1);
  }
  if (n_bases == 0 && bins == 0) return CHIRON_OK;   // nothing to compute and nothing to clear: no device is touched
  if (chiron_status st = use_device_workspace(who, device_id, workspace)) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  const size_t plane_bytes = (size_t)CHIRON_SIGNAL_PLANES * (size_t)bins * sizeof(int64_t);
  if ((n_bases > 0 && hipMemcpyAsync(ws + l.rec, recs.get(), (size_t)n_bases * sizeof(SignalBase), hipMemcpyHostToDevice, stream) != hipSuccess) ||
      (n_bases > 0 && n_samples > 0 &&
       hipMemcpyAsync(ws + l.samples, samples + sample_off[0], (size_t)n_samples * sizeof(int16_t), hipMemcpyHostToDevice, stream) != hipSuccess) ||
      (bins > 0 && hipMemsetAsync(ws + l.planes, 0, plane_bytes, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the reads to the device failed", who);
  if (n_bases > 0) {
    SignalParams p;
    p.rec = (const SignalBase*)(ws + l.rec);
    p.samples = (const int16_t*)(ws + l.samples);
    p.level = levels ? (int32_t*)(ws + l.level) : nullptr;
    p.planes = bins > 0 ? (long long*)(ws + l.planes) : nullptr;
    p.bases = n_bases;
    p.bins = bins;
    const int64_t want = ((n_bases + 63) / 64 + WAVES - 1) / WAVES;
    const dim3 grid((unsigned)(want < CHIRON_SIGNAL_MAX_GROUPS ? want : CHIRON_SIGNAL_MAX_GROUPS));
    hipLaunchKernelGGL(signal_kernel, grid, dim3(NT), 0, stream, p);
    if (chiron_status st = launched(who)) return st;
  }
  if ((levels && hipMemcpyAsync(level_out, ws + l.level, (size_t)n_bases * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      (bins > 0 && hipMemcpyAsync(planes_out, ws + l.planes, plane_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the level kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
  return CHIRON_OK;
}
