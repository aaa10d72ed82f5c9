// Event location for `locate --events` on gfx950: where on a reference of expected levels a query of event levels comes from, by an
// exact subsequence DTW whose path may skip a column at a price, and the host-only event detector that makes such queries.  The
// definitions are in include/chiron_amd.h and are restated in plain Python by tests/event_ref.py.
//
//   event_locate_kernel  locate_sweep<2> of csrc/locate_sweep.h, where the form is stated: a row is an event, a path stays, steps or
//                  skips one column at the penalty -- never across a break -- so a cell has a third candidate and a price register,
//                  and the halo is the 128 columns left of the tile, two a lane: columns 126 and 127 of row r - 1 are right while
//                  2 (r - 1) <= 126, through all 64 rows of the launch.
#include "event_pack.h"
#include "locate_sweep.h"

namespace chiron {

namespace {

static_assert(CHIRON_EVENT_MAX_QUERY == EVENT_MAX_QUERY && CHIRON_EVENT_MAX_PENALTY == EVENT_MAX_PENALTY, "header and pack agree");
static_assert(CHIRON_EVENT_MAX_SAMPLES == EVENT_MAX_SAMPLES && CHIRON_EVENT_MAX_WINDOW == EVENT_MAX_WINDOW && CHIRON_EVENT_MAX_RADIUS == EVENT_MAX_RADIUS &&
                  CHIRON_EVENT_MAX_THRESHOLD == EVENT_MAX_THRESHOLD,
              "header and pack agree");

__global__ __launch_bounds__(CHIRON_LOCATE_THREADS) void event_locate_kernel(SweepParams p) { locate_sweep<2>(p); }

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_signal_events(const int16_t* samples, const int64_t* sample_off, int64_t items, int32_t window, int32_t radius,
                                              int64_t threshold, int32_t max_events, uint32_t flags, int32_t* count_out, int32_t* border_out,
                                              int16_t* level_out, uint8_t* truncated_out) {
  const char* who = "chiron_signal_events";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  if (items < 0) return set_error(CHIRON_ERR_INVALID, "%s: negative size (items %lld)", who, (long long)items);
  if (items > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items in one call, at most 2^31 - 1", who, (long long)items);
  if (window < 2 || window > CHIRON_EVENT_MAX_WINDOW)
    return set_error(CHIRON_ERR_INVALID, "%s: window %d outside 2..%d", who, window, CHIRON_EVENT_MAX_WINDOW);
  if (radius < 1 || radius > CHIRON_EVENT_MAX_RADIUS)
    return set_error(CHIRON_ERR_INVALID, "%s: radius %d outside 1..%d", who, radius, CHIRON_EVENT_MAX_RADIUS);
  if (threshold < 1 || threshold > CHIRON_EVENT_MAX_THRESHOLD)
    return set_error(CHIRON_ERR_INVALID, "%s: threshold %lld outside 1..2^52", who, (long long)threshold);
  if (max_events < 1 || max_events > CHIRON_EVENT_MAX_SAMPLES)
    return set_error(CHIRON_ERR_INVALID, "%s: max_events %d outside 1..%d", who, max_events, CHIRON_EVENT_MAX_SAMPLES);
  if (items == 0) return CHIRON_OK;   // nothing to cut and nothing to write
  if (!sample_off || !samples) return set_error(CHIRON_ERR_INVALID, "%s: null samples / sample_off", who);
  if (!count_out || !border_out || !level_out || !truncated_out)
    return set_error(CHIRON_ERR_INVALID, "%s: null count_out / border_out / level_out / truncated_out", who);
  int64_t longest = 0;
  const LocateFinding f = locate_check_offsets(sample_off, items, EVENT_MAX_SAMPLES, &longest);
  if (f.fault == LOCATE_OFF_NEGATIVE) return set_error(CHIRON_ERR_INVALID, "%s: sample_off[0] = %lld is negative", who, (long long)f.value);
  if (f.fault == LOCATE_OFF_ORDER)
    return set_error(CHIRON_ERR_INVALID, "%s: sample_off[%lld] = %lld below its predecessor %lld", who, (long long)f.at, (long long)f.value,
                     (long long)sample_off[f.at - 1]);
  if (f.fault == LOCATE_QUERY_EMPTY) return set_error(CHIRON_ERR_INVALID, "%s: item %lld is empty", who, (long long)f.at);
  if (f.fault == LOCATE_QUERY_LONG)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: item %lld has %lld samples, at most %d", who, (long long)f.at, (long long)f.value, CHIRON_EVENT_MAX_SAMPLES);
  std::vector<int64_t> t;   // the statistic of one item: 8 bytes a sample, 1 MiB at most
  for (int64_t i = 0; i < items; ++i) {
    const int64_t at = sample_off[i] - sample_off[0];
    bool truncated = false;
    count_out[i] = event_segment(samples + sample_off[i], sample_off[i + 1] - sample_off[i], window, radius, threshold, max_events, border_out + at + i,
                                 level_out + at, &truncated, t);
    truncated_out[i] = truncated ? 1 : 0;
  }
  return CHIRON_OK;
}

extern "C" chiron_status chiron_event_locate_workspace_size(int64_t items, int64_t events, int64_t ref_len, size_t* bytes) {
  return sweep_workspace_size("chiron_event_locate_workspace_size", "events", items, events, ref_len, bytes);
}

extern "C" chiron_status chiron_event_locate(int32_t device_id, const int16_t* events, const int64_t* event_off, int64_t items,
                                             const int32_t* ref_level, int64_t ref_len, int32_t penalty, int32_t* block_out, void* workspace,
                                             size_t workspace_bytes, uint32_t flags, void* stream) {
  const SweepCall call = {"chiron_event_locate", "events", "event_off", CHIRON_EVENT_MAX_QUERY, event_locate_kernel, (uint32_t)penalty, "event locate"};
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", call.who, flags);
  if (penalty < 0 || penalty > CHIRON_EVENT_MAX_PENALTY)
    return set_error(CHIRON_ERR_INVALID, "%s: penalty %d outside 0..%d", call.who, penalty, CHIRON_EVENT_MAX_PENALTY);
  return sweep_call(call, device_id, events, event_off, items, ref_level, ref_len, block_out, workspace, workspace_bytes, stream);
}
