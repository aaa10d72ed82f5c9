// Signal location for `locate` on gfx950: where on a reference of expected levels a stretch of raw samples comes from, by an exact
// subsequence DTW of the samples against every column of the reference.  The definition is in include/chiron_amd.h and is restated
// in plain Python by tests/locate_ref.py.
//
//   locate_kernel  locate_sweep<1> of csrc/locate_sweep.h, where the form is stated: a row is a sample, a path stays on a column or
//                  steps to the next, and the halo is the 64 columns left of the tile, one a lane.
#include "locate_sweep.h"

namespace chiron {

namespace {

static_assert(CHIRON_LOCATE_MAX_QUERY == LOCATE_MAX_QUERY, "header and pack agree");

__global__ __launch_bounds__(CHIRON_LOCATE_THREADS) void locate_kernel(SweepParams p) { locate_sweep<1>(p); }

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_signal_locate_workspace_size(int64_t items, int64_t samples, int64_t ref_len, size_t* bytes) {
  return sweep_workspace_size("chiron_signal_locate_workspace_size", "samples", items, samples, ref_len, bytes);
}

extern "C" chiron_status chiron_signal_locate(int32_t device_id, const int16_t* samples, const int64_t* sample_off, int64_t items,
                                              const int32_t* ref_level, int64_t ref_len, int32_t* block_out, void* workspace,
                                              size_t workspace_bytes, uint32_t flags, void* stream) {
  const SweepCall call = {"chiron_signal_locate", "samples", "sample_off", CHIRON_LOCATE_MAX_QUERY, locate_kernel, 0, "locate"};
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", call.who, flags);
  return sweep_call(call, device_id, samples, sample_off, items, ref_level, ref_len, block_out, workspace, workspace_bytes, stream);
}
