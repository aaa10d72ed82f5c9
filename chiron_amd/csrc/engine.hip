// libchiron_amd.so -- engine: C ABI (include/chiron_amd.h), weight preparation, workspace, and the
// launch sequence that replaces chiron_model.inference (chiron_model.py:134-172) + the decode
// sub-graph (chiron_eval.py:465-492) of the reference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/chiron_amd.h"
#include "kernels.h"
#include "model_layout.h"
#include "weight_pack.h"
#include <dlfcn.h>

// profiling buckets (chiron_engine_profile_read) = names of the roctx ranges (CHIRON_ROCTX); order = the PN_* enum below
static const char* const kProfNames[] = {"conv_dma", "lstm_proj_dma", "lstm_recurrence", "fc_head", "ctc_greedy", "ctc_beam", "sparse_build",
                                         "path_prob", "conv_lift", "conv_res", "conv1_pwl", "conv_wino", "lstm_proj0_dma", "conv2a"};

using namespace chiron;

// ----------------------------------------------------------------------------------------------
// error plumbing: never throw across the ABI
// ----------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
namespace chiron {
chiron_status set_error(chiron_status st, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return st;
}
}  // namespace chiron
static constexpr auto& fail = chiron::set_error;   // this file's name for it
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(CHIRON_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                  __LINE__);                                                                       \
  } while (0)

extern "C" const char* chiron_last_error(void) { return g_err; }
extern "C" int32_t chiron_abi_version(void) { return CHIRON_ABI_VERSION; }

// Objects built with CHIRON_TIMING_BUILD (timing_variants.h: parts of a kernel switched off, garbage results) register here from
// a static constructor; the flag is constant-initialised, so the order of static initialisation does not matter.
static int g_timing_build = 0;
static char g_timing_source[96] = "";
namespace chiron {
void mark_timing_build(const char* source) {
  g_timing_build = 1;
  snprintf(g_timing_source, sizeof(g_timing_source), "%s", source ? source : "?");
}
}  // namespace chiron
extern "C" uint32_t chiron_build_flags(void) { return g_timing_build ? CHIRON_BUILD_TIMING : 0u; }

extern "C" chiron_status chiron_device_pci_bus_id(int32_t device_id, char* out, size_t cap) {
  if (!out || cap < 16) return chiron::set_error(CHIRON_ERR_INVALID, "chiron_device_pci_bus_id: buffer of at least 16 bytes needed");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return chiron::set_error(CHIRON_ERR_DEVICE, "no HIP device");
  if (device_id < 0 || device_id >= n) return chiron::set_error(CHIRON_ERR_INVALID, "device %d of %d", device_id, n);
  hipError_t err = hipDeviceGetPCIBusId(out, (int)cap, device_id);
  if (err != hipSuccess) return chiron::set_error(CHIRON_ERR_DEVICE, "hipDeviceGetPCIBusId: %s", hipGetErrorString(err));
  for (char* c = out; *c; ++c)
    if (*c >= 'A' && *c <= 'F') *c += 'a' - 'A';   // sysfs spells PCI addresses in lower case
  return CHIRON_OK;
}

extern "C" chiron_status chiron_weights_size(const chiron_model_desc* d, size_t* n_floats) {
  BlobMap map;
  chiron_status st = blob_map(d, &map);
  if (st) return st;
  if (!n_floats) return fail(CHIRON_ERR_INVALID, "null n_floats");
  *n_floats = map.total;
  return CHIRON_OK;
}

// ----------------------------------------------------------------------------------------------
// engine state
// ----------------------------------------------------------------------------------------------
// Default form of the fp32 recurrence (DESIGN 3.2 has the same-box A/B figures behind the choice)
#define CHIRON_LSTM_WIDE_DEFAULT 2

struct CalibRecord {           // one measured input: columns [k0, k0 + cin) of the plan behind `shift`, or rows of an LSTM kernel
  const float* shift;         // device shift array of the plan (key into plan_host), or the projection's for an LSTM layer
  int k0, cin;
  int lstm_layer, lstm_dir, lstm_part;   // lstm_layer >= 0: part 0 = x rows [k0, k0 + cin) of the TF kernel, part 1 = its h rows; dir -1 = both
  double rows;                 // rows summed
  size_t slot;                 // index of the record's [256] doubles in the device sum buffer
};
struct CalibCtx {
  double* dev_sums = nullptr;  // [max_records][256]
  size_t max_records = 0;
  std::vector<CalibRecord> rec;
  int skipped = 0;             // inputs that could not be measured (more than 256 channels, or more records than max_records)
};

struct ProfEvent {
  int name_id;
  hipEvent_t a, b;
  double flops, bytes;
};

struct Slot {
  hipStream_t stream = nullptr;
  unsigned long long* tile_ctr = nullptr;   // device [16]: [0..7] per-XCD tile counters of the DMA GEMM / Winograd kernels (GemmParams::tile_ctr),
                                            // [8] the streaming 1 x 1 kernel's; never reset
  unsigned long long tile_base = 0;         // host: the number the stream's next GEMM / Winograd launch starts at
  unsigned long long tile_base32 = 0;       // host: the same for counter [8]
  float* sig = nullptr;
  int32_t* seq = nullptr;
  float* act[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // 3 in population mode, 5 in batch-BN mode
  double* bn_sums = nullptr;  // batch-BN mode: two sets of [2][C] sums
  float* z = nullptr;
  float* lasth[2] = {nullptr, nullptr};
  float* lasth_f32 = nullptr;  // dtype fp32-split: the recurrence writes plain fp32 here, a pass converts it for the next GEMM
  float* logits = nullptr;
  uint8_t* labels = nullptr;
  int32_t* count = nullptr;
  float* log_prob = nullptr;
  float* prob = nullptr;
  int64_t* offsets = nullptr;
  int64_t* indices = nullptr;
  int64_t* values = nullptr;
  int64_t* meta = nullptr;
  void* beam_ws = nullptr;
  size_t beam_ws_bytes = 0;
  // pinned host
  float* h_sig = nullptr;
  int32_t* h_seq = nullptr;
  int64_t* h_indices = nullptr;
  int64_t* h_values = nullptr;
  int64_t* h_meta = nullptr;
  float* h_log_prob = nullptr;
  float* h_prob = nullptr;
  float* h_logits = nullptr;
  uint8_t* h_labels = nullptr;   // CHIRON_COMPACT_DECODE: the device's per-row label strings [B][T] ...
  int32_t* h_count = nullptr;    // ... and their lengths [B], copied in-stream behind the decode
  uint8_t* h_flat = nullptr;     // the rows' labels back to back, built by collect (plain host memory)
  // state of the in-flight batch
  // 0 = idle, 1 = a batch is in flight (between a successful submit / decode and its collect).  Atomic: submit and
  // collect of one slot may come from different threads (one producer, one consumer per engine; include/chiron_amd.h).
  struct State {
    std::atomic<int> v{0};
    State() {}
    State(const State& o) : v(o.v.load()) {}
    State& operator=(const State& o) {
      v.store(o.v.load());
      return *this;
    }
  } state;
  int batch = 0;
  uint32_t flags = 0;
  const float* sig_used = nullptr;
  // what chiron_engine_features / chiron_engine_rnn_output may hand out: the batch size of the last NETWORK batch of this slot
  // (0 after a decode-only batch or a failed submit: `batch` alone also counts chiron_engine_decode, which runs no network)
  int net_batch = 0;
  const float* rnn_out = nullptr;   // the last layer's lasth (time-major [T][BP][lasth_ld]; rnn_out_f32 = false: halves)
  bool rnn_out_f32 = true;
  std::vector<ProfEvent> events;
  // chiron_engine_score: labels, outputs and the edit-distance workspace of the scored batch; grown on demand, freed on destroy
  struct ScoreBufs {
    int32_t* labels = nullptr;     // [cap_labels]
    int32_t* label_len = nullptr;  // [cap_rows]
    float* loss = nullptr;         // [cap_rows]
    float* edit = nullptr;         // [cap_rows]
    int32_t* status = nullptr;     // [cap_rows]
    uint64_t* ws = nullptr;        // [cap_ws] edit-distance bit vectors
    size_t cap_labels = 0, cap_rows = 0, cap_ws = 0;
  } score;
};

struct chiron_engine : NetPlans {   // T, C, the stem, blocks, lstm and the FC head: filled by build_plans
  chiron_model_desc desc;
  BlobMap map;                    // where desc puts every tensor of the weight blob
  chiron_engine_opts opts;
  int L = 0, H = 0, K = 0;
  int maxB = 0, BP = 0;
  bool stream32 = true;           // fp32: 1 x 1 convolutions on the weight-stationary streaming kernel (CHIRON_NO_STREAM32=1: gemm.hip, A/B switch)
  bool stream16 = true;           // f16: 1 x 1 convolutions on the streaming kernel (CHIRON_NO_STREAM16=1: gemm.hip, A/B switch)
  bool proj_bf16 = true;          // fp32: the K = 256 / K = 200 LSTM x-projections as six-term bf16 products (CHIRON_PROJ_FP32=1: the fp32 MFMA kernels)
  bool dyn_tiles = true;          // DMA GEMM: tiles handed out by per-XCD counters instead of fixed shares (CHIRON_STATIC_TILES=1: off)
  int lstm16_pair = -1;           // f16 fused recurrence, two 16-row groups per workgroup: 1 always, 0 never (CHIRON_LSTM16_PAIR), -1 when single groups would not fit one round
  bool lstm16_fused = false;      // f16: x-projection inside the recurrence (whole 16-row groups that fill the CUs)
  bool lstm16_narrow = false;     // A/B switch: f16 recurrence on 4-row workgroups only
  bool lstm_fixed_roles = false;  // A/B switch: light role always on wave 6
  int lstm_form = 0;              // fp32 recurrence: 0 = 4-row kernels (lstm_kernel), 1 = lstm32w_kernel, 2 = lstm32w2_kernel
  bool lstm_paired = false;  // fp32 recurrence: 14-wave workgroups for the part of a batch that fits one resident round
  bool bn_batch = false;  // desc.bn_mode == CHIRON_BN_BATCH
  bool f16 = false;    // opts.dtype == CHIRON_F16: halves for activations / weights, fp32 accumulate, z, gates, logits
  bool w2 = false;     // opts.dtype == CHIRON_F16_W2: an f16 engine (f16 is set too) whose weights are exact hi + lo half pairs -- every GEMM
                       // runs its K-segments twice ([x, x] . [W_hi; W_lo], tiled DMA GEMMs only), z stays fp32, the recurrence is lstm16w2_kernel
  bool lasth32 = true;    // f16 engines: the LAST recurrent layer writes its output (what the FC head reads) as fp32 (LstmParams::out_f32);
                          // CHIRON_F16_LASTH16=1: halves as rounds 2 .. 5 (A/B)
  bool w2_zf16 = false;   // f16-w2, A/B switch CHIRON_W2_ZF16=1: z as halves between projection and recurrence
  bool split = false;  // opts.dtype == CHIRON_F32_SPLIT: fp32 values as hi/lo half pairs on the f16 matrix cores (GEMMs only)
  int lasth_ld = 0;    // elements per lasth row (2H; split: rounded up to whole 32-element blocks)
  int kq = GEMM_BK;    // K padding quantum in elements: one LDS chunk = 128 bytes per row (32 floats / 64 halves)
  std::vector<Slot> slots;
  std::map<const float*, PlanHost> plan_host;   // f16 engine: keyed by the plan's device shift pointer
  std::vector<float> host_weights;              // f16 engine: the caller's blob (LSTM kernels are read back from it in calibration)
  CalibCtx* calib = nullptr;                    // non-null while chiron_engine_calibrate runs the network
  int calibrated = 0;                           // iterations applied so far
  std::vector<void*> owned;  // device allocations freed on destroy
  bool profiling = false;
  std::vector<std::string> prof_names;
  std::mutex mu;
};

static chiron_status dev_alloc(chiron_engine* e, void** p, size_t bytes, bool zero) {
  HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
  e->owned.push_back(*p);
  if (zero) HIP_TRY(hipMemset(*p, 0, bytes ? bytes : 16));
  return CHIRON_OK;
}
// What the packer (weight_pack.h) prepared, onto the device: allocate, copy, store the plan's pointer; an f16 GEMM's host record goes
// under its device shift pointer
static chiron_status upload_plans(chiron_engine* e, std::vector<Upload>& ups) {
  for (Upload& u : ups) {
    chiron_status st = dev_alloc(e, u.dst, u.bytes, false);
    if (st) return st;
    HIP_TRY(hipMemcpy(*u.dst, u.data, u.bytes, hipMemcpyHostToDevice));
    u.owner.reset();
    if (u.host.Npad > 0) e->plan_host[(const float*)*u.dst] = std::move(u.host);
  }
  return CHIRON_OK;
}

static bool split_row_scale() {   // read once per process, by the first fp32-split engine
  static const bool on = getenv("CHIRON_SPLIT_NO_ROW_SCALE") == nullptr;
  return on;
}

static chiron_status build_plans(chiron_engine* e, const float* w) {
  e->bn_batch = e->desc.bn_mode == CHIRON_BN_BATCH;
  PackSwitches sw;
  sw.no_winograd = getenv("CHIRON_NO_WINOGRAD") != nullptr;
  sw.wino_f2 = getenv("CHIRON_WINOGRAD_F2") != nullptr;
  sw.wino_f4 = getenv("CHIRON_WINOGRAD_F4") != nullptr;
  sw.no_pwl = getenv("CHIRON_NO_PWL") != nullptr;
  sw.split_rec32 = getenv("CHIRON_SPLIT_REC32") != nullptr;
  if (e->split) sw.split_row_scale = split_row_scale();
  std::vector<Upload> ups;
  chiron_status st = pack_weights(e->desc, e->map, w, e->L, e->opts.dtype, sw, e, &ups);
  if (st) return st;
  // fp32 engines: the projections gemm_proj_bf16x3_kernel covers get their weights a second time, as three bf16 planes cut from the packed
  // fp32 rows while the packer's host copy is still there
  if (e->proj_bf16 && e->opts.dtype == CHIRON_F32 && !e->bn_batch) {
    for (LstmPlan& lp : e->lstm) {
      ConvGemmPlan& g = lp.proj[0];
      if (lp.nproj != 1 || (lp.in_w != 256 && lp.in_w != 200) || g.N % BF3_BN != 0) continue;
      for (const Upload& u : ups) {
        if (u.dst != reinterpret_cast<void**>(&g.Wt)) continue;
        const std::vector<uint16_t> planes = bf16x3_planes(static_cast<const float*>(u.data), g.N, g.K, lp.in_w);
        if ((st = dev_alloc(e, &g.w_bf3, planes.size() * sizeof(uint16_t), false))) return st;
        HIP_TRY(hipMemcpy(g.w_bf3, planes.data(), planes.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      }
    }
  }
  return upload_plans(e, ups);
}

// ---- sizes of an engine, computable without a GPU: the frame count, the largest tensor a kernel addresses with a
// 32-bit byte offset, the device memory of a slot.  chiron_engine_create refuses what this refuses.
// Limits (kernels.h / gemm.hip): the DMA GEMMs read their A operand through a raw-buffer descriptor with
// num_records = 0xFFFE0000 and 32-bit per-lane byte offsets, and the recurrence writes lasth through 32-bit byte
// offsets, so every activation tensor and every lasth tensor must stay below 0xFFFE0000 bytes; row counts are ints.
static const uint64_t TENSOR_LIMIT = 0xFFFE0000ull;

static chiron_status plan_sizes(const chiron_model_desc* d, const chiron_engine_opts* o, chiron_engine_sizes* out) {
  BlobMap map;
  chiron_status st = blob_map(d, &map);
  if (st) return st;
  if (!o) return fail(CHIRON_ERR_INVALID, "null opts");
  if (o->max_batch < 1 || o->segment_len < 1) return fail(CHIRON_ERR_INVALID, "max_batch/segment_len must be positive");
  if (o->dtype != CHIRON_F32 && o->dtype != CHIRON_F16 && o->dtype != CHIRON_F32_SPLIT && o->dtype != CHIRON_F16_W2)
    return fail(CHIRON_ERR_INVALID, "dtype %d unknown (0 = f32, 1 = f16, 2 = f32 as hi/lo half pairs, 3 = f16 activations against hi/lo weights)", o->dtype);
  if (o->max_beam < 0) return fail(CHIRON_ERR_INVALID, "max_beam %d", o->max_beam);
  if (o->max_beam > 0 && d->classes != CHIRON_CLASSES)
    return fail(CHIRON_ERR_INVALID, "max_beam %d with classes %d: the beam search kernels are built for %d classes (greedy decoding takes 2..%d)",
                o->max_beam, d->classes, CHIRON_CLASSES, CHIRON_KMAX);
  if (d->bn_mode == CHIRON_BN_BATCH)
    for (int i = 0; i < map.n_sites; ++i)
      if (map.site[i].co > BN_BATCH_MAX_C)
        return fail(CHIRON_ERR_INVALID, "bn_mode=batch: a convolution with %d output channels; the batch-statistics kernels cover at most %d",
                    map.site[i].co, BN_BATCH_MAX_C);
  const bool f16 = o->dtype == CHIRON_F16 || o->dtype == CHIRON_F16_W2, split = o->dtype == CHIRON_F32_SPLIT, bn_batch = d->bn_mode == CHIRON_BN_BATCH;
  const uint64_t B = (uint64_t)o->max_batch, BP = (uint64_t)roundup(o->max_batch, 16), L = (uint64_t)o->segment_len, H = d->hidden, K = d->classes;
  SiteFrames fr[MAX_SITES];
  const uint64_t T = (uint64_t)frames(map, o->segment_len, fr);
  uint64_t tmax = 0, cmax = 0;
  for (int i = map.has_stem; i < map.n_sites; ++i) {   // a block's input and output lengths are among its sites'
    tmax = std::max<uint64_t>(tmax, (uint64_t)std::max(fr[i].tin, fr[i].tout));
    cmax = std::max<uint64_t>(cmax, (uint64_t)map.site[i].co);
  }
  if (map.has_stem) cmax = std::max<uint64_t>(cmax, (uint64_t)map.site[0].co);   // the stem's output lies in an activation buffer too
  const uint64_t lasth_ld = !split ? 2 * H : d->rnn_kind == CHIRON_RNN_MULTI ? 2 * (uint64_t)roundup(d->hidden, 32) : (uint64_t)roundup(2 * d->hidden, 32);
  const uint64_t act = B * tmax * cmax * (f16 ? 2 : 4), lasth = T * BP * lasth_ld * 4, z = T * BP * 2 * 4 * H * 4;
  if (B * tmax >= (1ull << 31) || T * BP >= (1ull << 31))
    return fail(CHIRON_ERR_OVERFLOW, "max_batch %d x %llu frames does not fit the kernels' int row index", o->max_batch, (unsigned long long)tmax);
  if (act > TENSOR_LIMIT)
    return fail(CHIRON_ERR_OVERFLOW, "max_batch %d: an activation tensor [%d x %llu x %llu] needs %llu bytes, the kernels address at most %llu "
                "per tensor (about %llu windows at this segment length and dtype): use a smaller max_batch",
                o->max_batch, o->max_batch, (unsigned long long)tmax, (unsigned long long)cmax, (unsigned long long)act,
                (unsigned long long)TENSOR_LIMIT, (unsigned long long)(TENSOR_LIMIT / (tmax * cmax * (f16 ? 2 : 4))));
  if (T * BP * lasth_ld * (f16 ? 2 : 4) > TENSOR_LIMIT)   // the f16 engine keeps lasth as halves (the allocation stays 4 bytes per element)
    return fail(CHIRON_ERR_OVERFLOW, "max_batch %d: the recurrent output [%llu x %llu x %llu] needs %llu bytes, the kernels address at most %llu per tensor",
                o->max_batch, (unsigned long long)T, (unsigned long long)BP, (unsigned long long)lasth_ld, (unsigned long long)lasth,
                (unsigned long long)TENSOR_LIMIT);
  uint64_t slot = B * L * 4 + BP * 4 + (bn_batch ? 5 : 3) * act + (bn_batch ? 2 * 2 * cmax * 8 : 0) + z + 2 * lasth + (split ? T * BP * 2 * H * 4 : 0);
  slot += B * T * K * 4 + B * T + 3 * B * 4 + (B + 1) * 8 + B * T * 16 + B * T * 8 + 3 * 8;
  if (o->max_beam > 0) slot += beam_workspace_bytes((int)B, (int)T, o->max_beam);
  if (out) {
    out->T = (int32_t)T;
    out->ratio = (double)o->segment_len / (double)T;
    out->largest_tensor_bytes = std::max(act, T * BP * lasth_ld * (f16 ? 2 : 4));
    out->tensor_limit_bytes = TENSOR_LIMIT;
    out->slot_bytes = slot;
    out->total_bytes = slot * (uint64_t)std::max(1, o->n_slots);
  }
  return CHIRON_OK;
}

extern "C" chiron_status chiron_engine_plan(const chiron_model_desc* desc, const chiron_engine_opts* opts, chiron_engine_sizes* out) {
  if (!out) return fail(CHIRON_ERR_INVALID, "null out");
  memset(out, 0, sizeof(*out));
  return plan_sizes(desc, opts, out);
}

static chiron_status alloc_slot(chiron_engine* e, Slot* s) {
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  const size_t B = e->maxB, BP = e->BP, L = e->L, T = e->T, H = e->H, K = e->K;
  size_t tmax = 0, cmax = 0;
  for (const BlockPlan& b : e->blocks) {
    tmax = std::max<size_t>(tmax, b.t_in);  // the lifted conv2a is materialised at input resolution
    tmax = std::max<size_t>(tmax, b.t_out);
    cmax = std::max<size_t>(cmax, b.c);
  }
  if (e->stem_k > 0) cmax = std::max<size_t>(cmax, e->stem_c);   // wider than every block where the blocks narrow (plan_sizes counts it too)
  chiron_status st;
  if ((st = dev_alloc(e, (void**)&s->tile_ctr, 16 * sizeof(unsigned long long), true))) return st;
  if ((st = dev_alloc(e, (void**)&s->sig, B * L * 4, true))) return st;
  if ((st = dev_alloc(e, (void**)&s->seq, BP * 4, true))) return st;
  for (int i = 0; i < (e->bn_batch ? 5 : 3); ++i)
    if ((st = dev_alloc(e, (void**)&s->act[i], B * tmax * cmax * (e->f16 ? 2 : 4), false))) return st;
  if (e->bn_batch && (st = dev_alloc(e, (void**)&s->bn_sums, 2 * 2 * cmax * sizeof(double), true))) return st;
  if ((st = dev_alloc(e, (void**)&s->z, (size_t)T * BP * 2 * 4 * H * 4, true))) return st;
  for (int i = 0; i < 2; ++i)
    if ((st = dev_alloc(e, (void**)&s->lasth[i], T * BP * (size_t)e->lasth_ld * 4, true))) return st;
  if (e->split && (st = dev_alloc(e, (void**)&s->lasth_f32, T * BP * 2 * H * 4, true))) return st;
  if ((st = dev_alloc(e, (void**)&s->logits, B * T * K * 4, false))) return st;
  if ((st = dev_alloc(e, (void**)&s->labels, B * T, false))) return st;
  if ((st = dev_alloc(e, (void**)&s->count, B * 4, true))) return st;
  if ((st = dev_alloc(e, (void**)&s->log_prob, B * 4, true))) return st;
  if ((st = dev_alloc(e, (void**)&s->prob, B * 4, true))) return st;
  if ((st = dev_alloc(e, (void**)&s->offsets, (B + 1) * 8, true))) return st;
  if ((st = dev_alloc(e, (void**)&s->indices, B * T * 16, false))) return st;
  if ((st = dev_alloc(e, (void**)&s->values, B * T * 8, false))) return st;
  if ((st = dev_alloc(e, (void**)&s->meta, 3 * 8, true))) return st;
  if (e->opts.max_beam > 0) {
    s->beam_ws_bytes = beam_workspace_bytes((int)B, (int)T, e->opts.max_beam);
    if ((st = dev_alloc(e, &s->beam_ws, s->beam_ws_bytes, false))) return st;
  }
  HIP_TRY(hipHostMalloc((void**)&s->h_sig, B * L * 4, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&s->h_seq, BP * 4, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&s->h_indices, B * T * 16, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&s->h_values, B * T * 8, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&s->h_meta, 3 * 8, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&s->h_log_prob, B * 4, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&s->h_prob, B * 4, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&s->h_logits, B * T * K * 4, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&s->h_labels, B * T, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&s->h_count, B * 4, hipHostMallocDefault));
  s->h_flat = (uint8_t*)malloc(B * T ? B * T : 1);
  if (!s->h_flat) return fail(CHIRON_ERR_DEVICE, "out of host memory");
  memset(s->h_prob, 0, B * 4);
  return CHIRON_OK;
}

extern "C" chiron_status chiron_engine_create(const chiron_model_desc* desc, const float* weights, size_t n_floats,
                                              const chiron_engine_opts* opts, chiron_engine** out) {
  if (!out) return fail(CHIRON_ERR_INVALID, "null out");
  *out = nullptr;
  BlobMap map;
  chiron_status st = blob_map(desc, &map);
  if (st) return st;
  if (!weights || !opts) return fail(CHIRON_ERR_INVALID, "null weights/opts");
  if (map.total != n_floats) return fail(CHIRON_ERR_INVALID, "weight blob has %zu floats, descriptor needs %zu", n_floats, map.total);
  {
    chiron_engine_sizes sz;
    if ((st = plan_sizes(desc, opts, &sz))) return st;   // argument checks and the 32-bit addressing limits, before any GPU call
  }
  if (desc->hidden != 100) return fail(CHIRON_ERR_INVALID, "hidden=%d: the recurrence kernel is built for hidden=100 (both shipped models)", desc->hidden);
  // CHIRON_TRACE_CREATE=1: one line on stderr with where the time of this call went (tools/cold_start.py: the start-up budget of a
  // rank of `chiron call`; at 1250 reads per GPU the compute is ~3 s, so start-up decides the end-to-end figure of configs[3])
  const bool trace = getenv("CHIRON_TRACE_CREATE") != nullptr;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_enter = now();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(CHIRON_ERR_DEVICE, "no HIP device visible: libchiron_amd has no CPU fallback");
  if (opts->device_id < 0 || opts->device_id >= ndev) return fail(CHIRON_ERR_INVALID, "device_id %d out of range (%d devices)", opts->device_id, ndev);
  HIP_TRY(hipSetDevice(opts->device_id));
  if (trace) HIP_TRY(hipFree(nullptr));     // forces the context (and the code objects of this library) onto the device now, so that the stage below is not charged for it
  const double t_runtime = now();

  chiron_engine* e = new chiron_engine();
  e->desc = *desc;
  e->map = map;
  e->opts = *opts;
  if (e->opts.n_slots < 1) e->opts.n_slots = 1;
  e->L = opts->segment_len;
  e->H = desc->hidden;
  e->K = desc->classes;
  e->maxB = opts->max_batch;
  e->BP = roundup(opts->max_batch, 16);
  e->w2 = opts->dtype == CHIRON_F16_W2;
  e->w2_zf16 = e->w2 && getenv("CHIRON_W2_ZF16") != nullptr;
  e->lasth32 = getenv("CHIRON_F16_LASTH16") == nullptr;
  e->f16 = opts->dtype == CHIRON_F16 || e->w2;
  e->split = opts->dtype == CHIRON_F32_SPLIT;
  e->kq = e->f16 ? 2 * GEMM_BK : GEMM_BK;
  // split: rows hold whole 32-element blocks; MultiRNN reads each direction as its own K-segment, so the backward half
  // starts on a block boundary (fw at 0, bw at roundup(H, 32))
  e->lasth_ld = !e->split ? 2 * desc->hidden
                : desc->rnn_kind == CHIRON_RNN_MULTI ? 2 * roundup(desc->hidden, 32) : roundup(2 * desc->hidden, 32);
  // Tuning knob, off by default; results do not depend on it (same arithmetic per row).  Paired workgroups are 14 %
  // faster per resident round, but they fill their CU: with several batches in flight the 7-wave form, which shares a CU
  // with another slot's GEMM workgroups, gives the higher throughput (3905 vs 4004 kbases/s on one box).
  e->lstm_paired = getenv("CHIRON_LSTM_PAIR") != nullptr;
  e->lstm_fixed_roles = getenv("CHIRON_LSTM_FIXED_ROLES") != nullptr;
  // fp32 recurrence form: CHIRON_LSTM_WIDE=1 -> lstm32w_kernel (16 rows per workgroup), =0 -> lstm_kernel (4 rows); read once here
  {
    const char* wv = getenv("CHIRON_LSTM_WIDE");
    // (fp32-split: the GEMMs take a third of their fp32 time, the recurrence dominates and nothing fills the CUs a wide
    // launch leaves alone -- the 4-row form, 1.10 against 1.29 ms per launch, is the faster one there)
    e->lstm_form = wv ? atoi(wv) : (e->split ? 0 : CHIRON_LSTM_WIDE_DEFAULT);
    if (e->lstm_form < 0 || e->lstm_form > 2) e->lstm_form = CHIRON_LSTM_WIDE_DEFAULT;
  }
  e->lstm16_narrow = getenv("CHIRON_LSTM16_NARROW") != nullptr;
  e->lstm16_pair = getenv("CHIRON_LSTM16_PAIR") ? atoi(getenv("CHIRON_LSTM16_PAIR")) : -1;
  e->stream16 = getenv("CHIRON_NO_STREAM16") == nullptr && opts->dtype != CHIRON_F16_W2;   // (the streaming kernels hold ONE half per weight in registers)
  e->stream32 = getenv("CHIRON_NO_STREAM32") == nullptr;
  e->proj_bf16 = getenv("CHIRON_PROJ_FP32") == nullptr;   // A/B switch, per engine: the fp32 MFMA projections
  e->dyn_tiles = getenv("CHIRON_STATIC_TILES") == nullptr;   // A/B switch: fixed tile shares per workgroup
  {
    // f16 engines run the x-projection inside the recurrence (lstm16f_kernel) from 64 sixteen-row workgroups up (B >= 512:
    // a workgroup alone on its CU takes 0.69 ms for T = 400 whatever the batch, the projection GEMMs + the 4-row recurrence
    // take 0.66 ms at B = 512, 1.18 at 1100, 1.9 at 2048; measured per batch 2.04 vs 2.18 / 3.36 vs 4.12 / 5.33 vs 6.84 ms).
    // CHIRON_LSTM16_UNFUSED=1 keeps the projection GEMM + z (A/B switch), CHIRON_LSTM16_FUSED_MIN=<workgroups> moves the threshold.
    const int min_groups = getenv("CHIRON_LSTM16_FUSED_MIN") ? atoi(getenv("CHIRON_LSTM16_FUSED_MIN")) : 64;
    e->lstm16_fused = e->f16 && !e->w2 && !e->lstm16_narrow && desc->hidden == 100 && (e->BP / 16) * 2 >= min_groups && getenv("CHIRON_LSTM16_UNFUSED") == nullptr;
  }
  if (e->f16 && !e->w2) e->host_weights.assign(weights, weights + n_floats);
  st = build_plans(e, weights);
  const double t_plans = now();
  if (st == CHIRON_OK) {
    e->slots.resize(e->opts.n_slots);
    for (Slot& s : e->slots)
      if ((st = alloc_slot(e, &s))) break;
  }
  const double t_slots = now();
  if (st == CHIRON_OK && hipDeviceSynchronize() != hipSuccess) st = fail(CHIRON_ERR_DEVICE, "device sync after setup failed");
  if (trace)
    fprintf(stderr, "chiron_engine_create: {\"hip_runtime_and_context_ms\": %.1f, \"weights_prepared_and_uploaded_ms\": %.1f, \"slot_buffers_ms\": %.1f, "
                    "\"final_sync_ms\": %.1f, \"slots\": %d}\n", t_runtime - t_enter, t_plans - t_runtime, t_slots - t_plans, now() - t_slots, e->opts.n_slots);
  if (st) {
    chiron_engine_destroy(e);
    return st;
  }
  e->prof_names.assign(std::begin(kProfNames), std::end(kProfNames));
  *out = e;
  return CHIRON_OK;
}

extern "C" void chiron_engine_destroy(chiron_engine* e) {
  if (!e) return;
  hipSetDevice(e->opts.device_id);
  hipDeviceSynchronize();
  for (Slot& s : e->slots) {
    for (ProfEvent& ev : s.events) {
      hipEventDestroy(ev.a);
      hipEventDestroy(ev.b);
    }
    if (s.stream) hipStreamDestroy(s.stream);
    void* sp[] = {s.score.labels, s.score.label_len, s.score.loss, s.score.edit, s.score.status, s.score.ws};
    for (void* q : sp)
      if (q) hipFree(q);
    void* hp[] = {s.h_sig, s.h_seq, s.h_indices, s.h_values, s.h_meta, s.h_log_prob, s.h_prob, s.h_logits, s.h_labels, s.h_count};
    free(s.h_flat);
    for (void* q : hp)
      if (q) hipHostFree(q);
  }
  for (void* q : e->owned) hipFree(q);
  delete e;
}

extern "C" chiron_status chiron_engine_dims(const chiron_engine* e, int32_t* out_T, double* out_ratio) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  if (out_T) *out_T = e->T;
  if (out_ratio) *out_ratio = (double)e->L / (double)e->T;  // chiron_model.py:151-152 (true division)
  return CHIRON_OK;
}

// ----------------------------------------------------------------------------------------------
// launch sequence
// ----------------------------------------------------------------------------------------------
enum { PN_CONV = 0, PN_PROJ, PN_REC, PN_FC, PN_GREEDY, PN_BEAM, PN_SPARSE, PN_PATHPROB, PN_LIFT, PN_RES, PN_PWL, PN_WINO, PN_PROJ0, PN_CONV2A };

// roctx ranges around every stage's launches (CHIRON_ROCTX=1): a `rocprofv3 --kernel-trace --marker-trace` run then names the stages
// by themselves -- "conv_wino", "lstm_recurrence", ... -- instead of through bench.py's bucket -> kernel symbol table.  The marker
// library is looked up at run time (librocprofiler-sdk-roctx.so, else libroctx64.so): the engine links only the HIP runtime, and
// without the switch, or without the library, nothing is called.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* v = getenv("CHIRON_ROCTX");
    if (!v || !*v || *v == '0') return;
    for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (!h) continue;
      push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
      pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
      if (push && pop) return;
      push = nullptr, pop = nullptr;
    }
    fprintf(stderr, "chiron_amd: CHIRON_ROCTX is set but no roctx library could be loaded: no ranges\n");
  }
};
static const Roctx& roctx() {
  static const Roctx r;
  return r;
}

struct Prof {
  chiron_engine* e;
  Slot* s;
  ProfEvent ev;
  bool on;
  bool range;
  Prof(chiron_engine* e_, Slot* s_, int name_id, double flops, double bytes) : e(e_), s(s_), on(e_->profiling), range(roctx().push != nullptr) {
    if (range) roctx().push(kProfNames[name_id]);
    if (!on) return;
    ev.name_id = name_id;
    ev.flops = flops;
    ev.bytes = bytes;
    hipEventCreate(&ev.a);
    hipEventCreate(&ev.b);
    hipEventRecord(ev.a, s->stream);
  }
  ~Prof() {
    if (on) {
      hipEventRecord(ev.b, s->stream);
      s->events.push_back(ev);
    }
    if (range) roctx().pop();
  }
};

// The K-segments of one GEMM, in ELEMENTS; the f16 kernels address in 4-byte units (see GemmParams::f16)
struct Segs {
  GemmSeg s[GEMM_MAX_SEG];
  int n = 0;
  Segs(std::initializer_list<GemmSeg> l) {
    for (const GemmSeg& g : l) s[n++] = g;
  }
  // the k taps of a 1 x k convolution over src [.][C], each tap a segment `cop` columns wide
  Segs(const float* src, int C, int cop, int t_in, int stride, int k, int left) {
    for (int j = 0; j < k; ++j) s[n++] = GemmSeg{src, C, 0, C, cop, t_in, stride, j - left, 0};
  }
};

// The launch descriptor of plan w over M output rows of T_out frames per window, written to out [M][ldo]; everything else zero
static GemmParams gemm_desc(const chiron_engine* e, const ConvGemmPlan& w, int B, long M, int T_out, const Segs& segs, int relu, float* out, int ldo) {
  GemmParams g;
  memset(&g, 0, sizeof(g));
  g.B = B;
  g.BP = e->BP;
  g.N = w.N;
  g.K = w.K;
  g.Wt = w.Wt;
  g.shift = w.shift;
  g.descale = w.descale;
  g.z_dirs_total = 2;
  g.M = (int)M;
  g.T_out = T_out;
  g.nseg = segs.n;
  for (int i = 0; i < segs.n; ++i) g.seg[i] = segs.s[i];
  g.relu = relu;
  g.out = out;
  g.ldo = ldo;
  return g;
}

// Calibration pass of the f16 engine: before a convolution GEMM runs, the column sums of every K-segment's source.
static void calib_measure(chiron_engine* e, const float* shift, int k0, const void* src, long rows, int ld, int col0, int cin, int BP, int B,
                          int lstm_layer, int lstm_dir, int lstm_part, hipStream_t stream) {
  CalibCtx* c = e->calib;
  if (!c) return;
  if (c->rec.size() >= c->max_records || cin > 256) {   // a partially applied correction must not pass silently (advisor, round 4)
    ++c->skipped;
    return;
  }
  CalibRecord r{shift, k0, cin, lstm_layer, lstm_dir, lstm_part, BP > 0 ? (double)(rows / BP) * B : (double)rows, c->rec.size()};
  launch_colsum_f16(src, rows, ld, col0, cin, BP, B, c->dev_sums + r.slot * 256, stream);
  c->rec.push_back(r);
}

static bool launch(chiron_engine* e, GemmParams& g, hipStream_t stream) {
  if (e->calib && e->f16 && g.out_mode == 0) {       // (the LSTM projections are measured in run_rnn, fused or not)
    int k0 = 0;
    for (int i = 0; i < g.nseg; ++i) {
      const GemmSeg& sg = g.seg[i];
      if (sg.src) calib_measure(e, g.shift, k0, sg.src, (long)g.B * sg.w_in, sg.lda, sg.col0, sg.cin, 0, g.B, -1, 0, 0, stream);
      k0 += sg.kpad;
    }
  }
  Slot* own = nullptr;   // the slot this stream belongs to: its tile counters (dynamic tile scheduling)
  if (e->dyn_tiles)
    for (Slot& sl : e->slots)
      if (sl.stream == stream) own = &sl;
  if (!e->f16 && !e->split && e->stream32) {   // fp32 256 -> 256 channel 1 x 1 convolutions
    if (own) g.tile_ctr = own->tile_ctr + 8, g.tile_base_host = &own->tile_base32;
    if (launch_stream32(g, stream)) return true;
  }
  g.tile_ctr = own ? own->tile_ctr : nullptr;
  g.tile_base_host = own ? &own->tile_base : nullptr;
  if (e->split) g.f16 = 2;  // same 4-byte element units as fp32; only the content of the 128-byte blocks differs
  if (e->f16) {
    if (e->stream16 && launch_stream16(g, stream)) return true;   // 256 -> 256 channel 1 x 1 convolutions: streaming kernel
    g.f16 = 1;
    for (int i = 0; i < g.nseg; ++i) {
      g.seg[i].lda /= 2;
      g.seg[i].col0 /= 2;
      g.seg[i].cin /= 2;
      g.seg[i].kpad /= 2;
    }
    g.K /= 2;
    if (g.out_mode == 0) g.ldo /= 2;
    if (e->w2) {   // [x, x] . [W_hi; W_lo]: the same A segments again, against the lo columns of the weight rows (upload_gemm)
      if (2 * g.nseg > GEMM_MAX_SEG) return false;
      for (int i = 0; i < g.nseg; ++i) g.seg[g.nseg + i] = g.seg[i];
      g.nseg *= 2;
      g.K *= 2;
    }
  }
  return launch_gemm(g, stream);
}

// bn_mode = batch: every BN site is raw conv -> batch moments -> normalise (cnn.py:166-188), nothing folds.
static bool run_cnn_batch_bn(chiron_engine* e, Slot* s, int B, const float* sig) {
  bool ok = true;
  int xi = -1;
  const float* x = nullptr;
  if (e->stem_k > 0) {
    const long M0 = (long)B * e->stem_t;
    launch_stem_conv(sig, e->stem_w, e->stem_shift, s->act[4], B, e->L, e->stem_t, e->stem_k, e->stem_stride, e->stem_left, e->stem_c, 0, 0,
                     s->stream);
    launch_bn_stats(s->act[4], M0, e->stem_c, s->bn_sums, s->stream);
    launch_bn_apply(s->act[4], s->bn_sums, e->stem_scale, e->stem_offset, M0, e->stem_c, 1, nullptr, nullptr, nullptr, nullptr, s->stream);
    x = s->act[4];
    xi = 4;
  }
  for (const BlockPlan& b : e->blocks) {
    float* buf[4];
    for (int i = 0, j = 0; i < 5 && j < 4; ++i)
      if (i != xi) buf[j++] = s->act[i];
    float *A = buf[0], *Bf = buf[1], *Cf = buf[2], *D = buf[3];
    const int cop = roundup(b.c, e->kq), C = b.c;
    const long Min = (long)B * b.t_in, Mout = (long)B * b.t_out;
    double* s0 = s->bn_sums;
    double* s1 = s->bn_sums + 2 * C;
    const Segs in_taps(A, C, cop, b.t_in, b.stride, b.k, b.left);
    Prof pr(e, s, PN_CONV, 2.0 * ((double)Min * b.c_in * C + (double)Mout * (b.k * C + C + b.c_in) * C), 4.0 * (Min + 3.0 * Mout) * C * 3);
    // conv2a + BN + ReLU
    if (b.lift) {
      launch_rank1_conv(sig, b.lift_a, A, Min, b.t_in, e->L, 1, C, true, s->stream);   // BN follows: centered (bn_batch.hip)
    } else {
      GemmParams g = gemm_desc(e, b.ga, B, Min, b.t_in, {GemmSeg{x, b.c_in, 0, b.c_in, roundup(b.c_in, e->kq), b.t_in, 1, 0, 0}}, 0, A, C);
      ok &= launch(e, g, s->stream);
    }
    launch_bn_stats(A, Min, C, s0, s->stream);
    launch_bn_apply(A, s0, b.bn_scale[1], b.bn_offset[1], Min, C, 1, nullptr, nullptr, nullptr, nullptr, s->stream);
    // conv2b + BN + ReLU
    GemmParams g = gemm_desc(e, b.gb, B, Mout, b.t_out, in_taps, 0, Bf, C);
    ok &= launch(e, g, s->stream);
    launch_bn_stats(Bf, Mout, C, s0, s->stream);
    launch_bn_apply(Bf, s0, b.bn_scale[2], b.bn_offset[2], Mout, C, 1, nullptr, nullptr, nullptr, nullptr, s->stream);
    // conv2c (+ BN), branch1 conv1 (+ BN iff i_bn), add, ReLU
    g = gemm_desc(e, b.gc, B, Mout, b.t_out, {GemmSeg{Bf, C, 0, C, cop, b.t_out, 1, 0, 0}}, 0, Cf, C);
    ok &= launch(e, g, s->stream);
    launch_bn_stats(Cf, Mout, C, s0, s->stream);
    if (b.lift) {
      launch_rank1_conv(sig, b.res_a, D, Mout, b.t_out, e->L, b.stride, C, b.i_bn, s->stream);
    } else {
      g = gemm_desc(e, b.g1, B, Mout, b.t_out, {GemmSeg{x, b.c_in, 0, b.c_in, roundup(b.c_in, e->kq), b.t_in, b.stride, 0, 0}}, 0, D, C);
      ok &= launch(e, g, s->stream);
    }
    if (b.i_bn) launch_bn_stats(D, Mout, C, s1, s->stream);
    launch_bn_apply(Cf, s0, b.bn_scale[3], b.bn_offset[3], Mout, C, 1, D, b.i_bn ? s1 : nullptr, b.bn_scale[0], b.bn_offset[0], s->stream);
    x = Cf;
    for (int i = 0; i < 5; ++i)
      if (s->act[i] == Cf) xi = i;
  }
  s->sig_used = x;
  return ok;
}

static bool run_cnn(chiron_engine* e, Slot* s, int B, const float* sig) {
  if (e->bn_batch) return run_cnn_batch_bn(e, s, B, sig);
  bool ok = true;
  float* x = nullptr;  // block input (channels-last [B*T][C])
  int xi = -1;         // which act buffer holds x
  if (e->stem_k > 0) {
    Prof pr(e, s, PN_LIFT, 2.0 * B * e->stem_t * (double)e->stem_k * e->stem_c, 4.0 * B * e->L + 4.0 * B * e->stem_t * e->stem_c);
    launch_stem_conv(sig, e->stem_w, e->stem_shift, s->act[2], B, e->L, e->stem_t, e->stem_k, e->stem_stride, e->stem_left, e->stem_c,
                     e->f16 ? 1 : e->split ? 2 : 0, 1, s->stream);
    x = s->act[2];
    xi = 2;
  }
  for (const BlockPlan& b : e->blocks) {
    const int cop = roundup(b.c, e->kq);
    // pick two scratch buffers different from x
    int ia = (xi + 1) % 3, ib = (xi + 2) % 3;
    if (xi < 0) {
      ia = 0;
      ib = 1;
    }
    float* bufA = s->act[ia];
    float* bufB = s->act[ib];
    const long Mout = (long)B * b.t_out;
    const Segs in_taps(bufA, b.c, cop, b.t_in, b.stride, b.k, b.left);   // conv2b reads conv2a's output from bufA
    if (b.lift) {
      bool done_pwl = false;
      if (b.pwl_tab != nullptr) {
        // conv2a + conv2b in one memory-bound pass over a piecewise-linear table of the signal value (pwl.hip)
        PwlConvParams q;
        q.sig = sig, q.bp = b.pwl_bp, q.ref = b.pwl_ref, q.tab = reinterpret_cast<const float2*>(b.pwl_tab), q.shift = b.pwl_shift, q.out = bufB;
        q.B = B, q.L = e->L, q.T_out = b.t_out, q.k = b.k, q.stride = b.stride, q.left = b.left, q.C = b.c, q.nbp = b.pwl_nbp;
        q.fmt = e->f16 ? 1 : e->split ? 2 : 0;
        Prof pr(e, s, PN_PWL, 2.0 * B * b.t_out * (double)b.k * b.c, 4.0 * B * e->L + (e->f16 ? 2.0 : 4.0) * B * b.t_out * b.c);
        done_pwl = launch_pwl_conv(q, s->stream);
      }
      if (!done_pwl) {
        // conv2a of the signal is materialised (one HBM-bound pass), conv2b is then an ordinary DMA launch
        {
          Prof pr(e, s, PN_LIFT, 2.0 * B * b.t_in * b.c, 4.0 * B * b.t_in + (e->f16 ? 2.0 : 4.0) * B * b.t_in * b.c);
          launch_lift(sig, b.lift_a, b.lift_b, bufA, (long)B * b.t_in, b.c, e->f16 ? 1 : e->split ? 2 : 0, s->stream);
        }
        // conv2b over the lifted signal: A(m, tap*C + c) = relu(sig*a[c] + b[c])
        GemmParams g = gemm_desc(e, b.gb, B, Mout, b.t_out, in_taps, 1, bufB, b.c);
        Prof pr(e, s, PN_CONV, 2.0 * B * b.t_out * (double)b.k * b.c * b.c, (e->f16 ? 2.0 : 4.0) * B * (b.t_in + b.t_out) * b.c);
        ok &= launch(e, g, s->stream);
      }
      // conv2c + lifted branch1 + ReLU
      GemmParams g = gemm_desc(e, b.gc, B, Mout, b.t_out, {GemmSeg{bufB, b.c, 0, b.c, cop, b.t_out, 1, 0, 0}}, 1, bufA, b.c);
      g.sig = sig;
      g.L = e->L;
      g.res_a = b.res_a;
      g.res_b = b.res_b;
      g.res_stride = b.stride;
      {
        Prof pr(e, s, PN_RES, 2.0 * B * b.t_out * (double)b.c * b.c, 8.0 * B * b.t_out * b.c);
        ok &= launch(e, g, s->stream);
      }
      x = bufA;
      xi = ia;
    } else {
      const int cip = roundup(b.c_in, e->kq);
      // conv2a
      GemmParams g = gemm_desc(e, b.ga, B, (long)B * b.t_in, b.t_in, {GemmSeg{x, b.c_in, 0, b.c_in, cip, b.t_in, 1, 0, 0}}, 1, bufA, b.c);
      {
        // conv2a (K = c_in) has its own bucket: on the fp32 engine it runs on the streaming kernel (stream32.hip)
        Prof pr(e, s, PN_CONV2A, 2.0 * B * b.t_in * (double)b.c_in * b.c, 4.0 * B * b.t_in * (b.c_in + b.c));
        ok &= launch(e, g, s->stream);
      }
      // conv2b
      g = gemm_desc(e, b.gb, B, Mout, b.t_out, in_taps, 1, bufB, b.c);
      {
        bool done = false;
        if (b.wino_u != nullptr) {
          WinoParams wq;
          wq.src = bufA, wq.U = b.wino_u, wq.shift = b.gb.shift, wq.out = bufB;
          wq.B = B, wq.T = b.t_in, wq.C = b.c, wq.N = b.c, wq.lda = b.c, wq.ldo = b.c, wq.relu = 1, wq.f4 = b.wino_f4;
          wq.tile_ctr = e->dyn_tiles ? s->tile_ctr : nullptr, wq.tile_base = 0, wq.tile_base_host = &s->tile_base;
          // FLOPs of the convolution as the reference defines it (2 * 3 taps * C * C per position); 2/3 of them are executed
          Prof pr(e, s, PN_WINO, 2.0 * B * b.t_out * (double)b.k * b.c * b.c, 4.0 * B * (b.t_in + b.t_out) * b.c);
          done = launch_wino_conv3(wq, s->stream);
        }
        if (!done) {
          Prof pr(e, s, PN_CONV, 2.0 * B * b.t_out * (double)b.k * b.c * b.c, 4.0 * B * (b.t_in + b.t_out) * b.c);
          ok &= launch(e, g, s->stream);
        }
      }
      // conv2c + branch1/conv1 fused along K, + ReLU
      g = gemm_desc(e, b.gc, B, Mout, b.t_out,
                    {GemmSeg{bufB, b.c, 0, b.c, cop, b.t_out, 1, 0, 0}, GemmSeg{x, b.c_in, 0, b.c_in, cip, b.t_in, b.stride, 0, 0}}, 1, bufA, b.c);
      {
        Prof pr(e, s, PN_CONV, 2.0 * B * b.t_out * (double)(b.c + b.c_in) * b.c, 4.0 * B * b.t_out * (2.0 * b.c + b.c_in));
        ok &= launch(e, g, s->stream);
      }
      x = bufA;
      xi = ia;
    }
  }
  s->sig_used = x;  // CNN feature [B*T][C]
  return ok;
}

static bool run_rnn(chiron_engine* e, Slot* s, int B) {
  bool ok = true;
  bool last_out_f32 = false;
  const float* fea = s->sig_used;
  const int T = e->T, H = e->H, BP = e->BP;
  const int zc = 4 * H;
  const float* prev = nullptr;
  for (size_t l = 0; l < e->lstm.size(); ++l) {
    const LstmPlan& lp = e->lstm[l];
    float* outbuf = s->lasth[l & 1];
    // f16, whole 16-row groups filling the CUs: the projection runs inside the recurrence (lstm16f_kernel), no z
    const bool fused = e->lstm16_fused && lp.wxwide != nullptr;
    for (int pj = 0; pj < (fused ? 0 : lp.nproj); ++pj) {
      const int Kp = roundup(lp.in_w, e->kq);
      const GemmSeg src = l == 0           ? GemmSeg{fea, e->C, 0, e->C, Kp, T, 1, 0, 0}
                          : lp.nproj == 1 ? GemmSeg{prev, e->lasth_ld, 0, 2 * H, Kp, T, 1, 0, 1}
                                          : GemmSeg{prev, e->lasth_ld, e->split ? pj * roundup(H, 32) : pj * H, H, Kp, T, 1, 0, 1};
      GemmParams g = gemm_desc(e, lp.proj[pj], B, (long)T * BP, T, {src}, 0, s->z, 0);
      g.m_time_major = 1;
      g.out_mode = 1;
      g.z_cols = zc;
      g.z_ndir = lp.nproj == 1 ? 2 : 1;
      g.z_dir0 = lp.nproj == 1 ? 0 : pj;
      g.z_seq_len = s->seq;
      g.w_bf3 = lp.proj[pj].w_bf3;   // non-null: gemm_proj_bf16x3_kernel (build_plans)
      g.z_f16 = (e->f16 && (!e->w2 || e->w2_zf16)) ? 1 : 0;
      const double ndir = lp.nproj == 1 ? 2.0 : 1.0;
      // layer 0 reads the CNN features (K = 256: its own kernel instantiation), the other layers the recurrent output
      Prof pr(e, s, l == 0 ? PN_PROJ0 : PN_PROJ, 2.0 * B * T * (double)lp.in_w * 4 * H * ndir, 4.0 * B * T * (lp.in_w + ndir * zc));
      ok &= launch(e, g, s->stream);
    }
    LstmParams r;
    r.z = s->z;
    r.wfrag = lp.wfrag;
    r.wlight = lp.wlight;
    r.wwide = lp.wwide;
    r.wwide32 = lp.wwide32;
    r.wsplit = lp.wsplit;
    r.form32 = e->lstm_form;
    r.narrow16 = e->lstm16_narrow ? 1 : 0;
    r.xsrc = nullptr;
    r.wxwide = nullptr;
    r.whfused = nullptr;
    r.fused_pair = 0;
    r.xbias = nullptr;
    r.xK = r.xld = r.x_time_major = 0;
    if (fused) {
      r.xsrc = l == 0 ? (const void*)fea : (const void*)prev;
      r.wxwide = lp.wxwide;
      r.whfused = lp.whfused;
      // one 8-wave workgroup per CU either way (registers): 16-row workgroups that need a second round (B = 4096: 512) take 2 x 0.66 ms,
      // 256 32-row workgroups 1.24 ms in one; below one round the 16-row form finishes in 0.66 (B = 2048)
      r.fused_pair = e->lstm16_pair >= 0 ? (e->lstm16_pair ? 1 : 0) : ((BP / 16) * 2 > current_device_cus() ? 1 : 0);
      r.xbias = lp.proj[0].shift;
      r.xK = lp.in_w;
      r.xld = l == 0 ? e->C : e->lasth_ld;
      r.x_time_major = l == 0 ? 0 : 1;
    }
    r.seq_len = s->seq;
    r.out = e->split ? s->lasth_f32 : outbuf;
    // f16 engines: the last layer's output goes to the FC head as fp32 (not while the calibration pass measures the layers' outputs as halves)
    r.out_f32 = (e->f16 && e->lasth32 && e->calib == nullptr && l + 1 == e->lstm.size()) ? 1 : 0;
    last_out_f32 = r.out_f32 != 0;
    // fp32-split with its own recurrence (lstm32s_kernel): a layer that feeds another projection writes the hi / lo format that
    // projection reads straight into the layer's lasth buffer -- no fp32 copy, no conversion pass; the last layer writes fp32 for the FC head
    const bool direct_split = e->split && lp.wsplit != nullptr && l + 1 < e->lstm.size();
    r.out_split = direct_split ? (void*)outbuf : nullptr;
    r.split_ld = e->lasth_ld;
    r.split_bw0 = e->desc.rnn_kind == CHIRON_RNN_MULTI ? roundup(H, 32) : H;
    r.T = T;
    r.B = B;
    r.BP = BP;
    r.H = H;
    r.ndir = 2;
    r.paired = e->lstm_paired ? 1 : 0;
    r.fixed_roles = e->lstm_fixed_roles ? 1 : 0;
    r.group0 = 0;
    r.f16 = e->f16 ? 1 : 0;
    r.w2 = e->w2 ? (e->w2_zf16 ? 2 : 1) : 0;
    if (e->calib && e->f16) {
      // x rows of the layer's kernels: the means of the layer's input (features: batch-major rows; lasth: time-major)
      for (int pj = 0; pj < lp.nproj; ++pj) {
        const int dir = lp.nproj == 1 ? -1 : pj;
        if (l == 0)
          calib_measure(e, lp.proj[pj].shift, 0, fea, (long)B * T, e->C, 0, e->C, 0, B, (int)l, dir, 0, s->stream);
        else
          calib_measure(e, lp.proj[pj].shift, 0, prev, (long)T * BP, e->lasth_ld, lp.nproj == 1 ? 0 : pj * H, lp.in_w, BP, B, (int)l, dir, 0, s->stream);
      }
    }
    {
      Prof pr(e, s, PN_REC, 2.0 * 2.0 * B * T * (double)H * 4 * H + (fused ? 2.0 * B * T * (double)lp.in_w * 4 * H * 2.0 : 0.0),
              fused ? (e->f16 ? 2.0 : 4.0) * B * T * (2.0 * lp.in_w + 2.0 * H) : 4.0 * B * T * 2.0 * (zc + H));
      launch_lstm(r, s->stream);
    }
    if (e->calib && e->f16)      // h rows: the means of the layer's own output, per direction
      for (int dir = 0; dir < 2; ++dir)
        calib_measure(e, lp.proj[lp.nproj == 1 ? 0 : dir].shift, 0, outbuf, (long)T * BP, e->lasth_ld, dir * H, H, BP, B, (int)l, dir, 1, s->stream);
    prev = outbuf;
    if (e->split) {
      if (direct_split) {
        // nothing to convert
      } else if (l + 1 < e->lstm.size()) {
        Prof pr(e, s, PN_REC, 0.0, (4.0 + 4.0) * T * BP * 2.0 * H);
        const bool multi = e->desc.rnn_kind == CHIRON_RNN_MULTI;
        launch_split_convert(s->lasth_f32, outbuf, (long)T * BP, 2 * H, e->lasth_ld, multi ? H : 0, multi ? roundup(H, 32) : 0, s->stream);
      } else {
        prev = s->lasth_f32;   // the FC head reads the last layer's fp32 output directly
      }
    }
  }
  s->rnn_out = prev;
  FcParams f;
  f.lasth = prev;
  f.w = e->fc_w;
  f.bias = e->fc_b;
  f.wc = e->fc_wc;
  f.bc = e->fc_bc;
  f.logits = s->logits;
  f.T = T;
  f.B = B;
  f.BP = BP;
  f.H = H;
  f.K = e->K;
  f.f16 = (e->f16 && !last_out_f32) ? 1 : 0;
  f.split = 0;
  f.ld = e->lasth_ld;
  s->rnn_out_f32 = !e->f16 || last_out_f32;
  {
    Prof pr(e, s, PN_FC, 2.0 * B * T * (2.0 * H + (double)H * e->K), 4.0 * B * T * (2.0 * H + e->K));
    launch_fc(f, s->stream);
  }
  return ok;
}

static chiron_status enqueue_decode(chiron_engine* e, Slot* s, int B, int beam_width, uint32_t flags) {
  const int T = e->T, K = e->K;
  if (beam_width == 0) {
    GreedyParams g;
    g.logits = s->logits;
    g.seq_len = s->seq;
    g.labels = s->labels;
    g.count = s->count;
    g.log_prob = s->log_prob;
    g.prob_logits = (flags & CHIRON_WANT_PROB) ? s->prob : nullptr;
    g.B = B;
    g.T = T;
    g.K = K;
    Prof pr(e, s, PN_GREEDY, 0, 4.0 * B * T * K);
    launch_greedy(g, s->stream);
  } else {
    if (flags & CHIRON_WANT_PROB) {
      PathProbParams pp{s->logits, s->prob, B, T, K};
      Prof pr(e, s, PN_PATHPROB, 0, 4.0 * B * T * K);
      launch_path_prob(pp, s->stream);
    }
    BeamParams bp;
    bp.logits = s->logits;
    bp.seq_len = s->seq;
    bp.labels = s->labels;
    bp.count = s->count;
    bp.log_prob = s->log_prob;
    bp.workspace = s->beam_ws;
    bp.workspace_bytes = s->beam_ws_bytes;
    bp.B = B;
    bp.T = T;
    bp.K = K;
    bp.beam = beam_width;
    Prof pr(e, s, PN_BEAM, 0, 4.0 * B * T * K);
    if (launch_beam(bp, s->stream) != 0) return fail(CHIRON_ERR_INVALID, "beam search launch rejected (beam_width %d)", beam_width);
  }
  {
    SparseParams sp{s->labels, s->count, s->offsets, s->indices, s->values, s->meta, B, T};
    Prof pr(e, s, PN_SPARSE, 0, 0);
    launch_sparse(sp, s->stream);
  }
  HIP_TRY(hipMemcpyAsync(s->h_meta, s->meta, 3 * 8, hipMemcpyDeviceToHost, s->stream));
  if (flags & CHIRON_COMPACT_DECODE) {
    // fixed-size copies, known at submit time: no second round trip in collect (the SparseTensor's size is only known once the
    // decode has run, so its copy is issued BY collect: sync, read nnz, copy nnz * 24 bytes, sync again)
    HIP_TRY(hipMemcpyAsync(s->h_labels, s->labels, (size_t)B * T, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_count, s->count, (size_t)B * 4, hipMemcpyDeviceToHost, s->stream));
  }
  HIP_TRY(hipMemcpyAsync(s->h_log_prob, s->log_prob, (size_t)B * 4, hipMemcpyDeviceToHost, s->stream));
  if (flags & CHIRON_WANT_PROB) HIP_TRY(hipMemcpyAsync(s->h_prob, s->prob, (size_t)B * 4, hipMemcpyDeviceToHost, s->stream));
  if (flags & CHIRON_WANT_LOGITS)
    HIP_TRY(hipMemcpyAsync(s->h_logits, s->logits, (size_t)B * T * K * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipGetLastError());
  return CHIRON_OK;
}

// After a failed submit / collect the slot's stream is drained; a launch that never ran has not taken its numbers from the
// tile counters while the host side already counted them (GemmParams::tile_base), and every later workgroup would read
// "no tile left".  Both sides restart from zero.
static void resync_tile_counters(Slot* s) {
  hipStreamSynchronize(s->stream);
  if (s->tile_ctr && hipMemsetAsync(s->tile_ctr, 0, 16 * sizeof(unsigned long long), s->stream) == hipSuccess) hipStreamSynchronize(s->stream);
  s->tile_base = s->tile_base32 = 0;
  (void)hipGetLastError();
}

static chiron_status submit_impl(chiron_engine* e, int32_t slot, const float* x, const float* const* pieces, const int32_t* piece_rows,
                                 const int64_t* piece_row_stride, int32_t n_pieces, const int32_t* seq_len, int32_t batch, int32_t beam_width,
                                 uint32_t flags);

// A host batch onto the slot's stream through its pinned staging buffers: B windows x (null: h_sig already holds them) and their
// lengths; the padded rows of seq read 0
static chiron_status stage_input(chiron_engine* e, Slot* s, const float* x, const int32_t* seq_len, int B) {
  HIP_TRY(hipMemsetAsync(s->seq, 0, e->BP * 4, s->stream));
  if (x) memcpy(s->h_sig, x, (size_t)B * e->L * 4);
  memcpy(s->h_seq, seq_len, (size_t)B * 4);
  HIP_TRY(hipMemcpyAsync(s->sig, s->h_sig, (size_t)B * e->L * 4, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->seq, s->h_seq, (size_t)B * 4, hipMemcpyHostToDevice, s->stream));
  return CHIRON_OK;
}

extern "C" chiron_status chiron_engine_submit(chiron_engine* e, int32_t slot, const float* x, const int32_t* seq_len,
                                              int32_t batch, int32_t beam_width, uint32_t flags) {
  if (!x) return fail(CHIRON_ERR_INVALID, "null x/seq_len");
  return submit_impl(e, slot, x, nullptr, nullptr, nullptr, 0, seq_len, batch, beam_width, flags);
}

extern "C" chiron_status chiron_engine_submit_pieces(chiron_engine* e, int32_t slot, const float* const* pieces, const int32_t* piece_rows,
                                                     const int64_t* piece_row_stride, int32_t n_pieces, const int32_t* seq_len, int32_t batch,
                                                     int32_t beam_width, uint32_t flags) {
  if (!pieces || !piece_rows || n_pieces < 1) return fail(CHIRON_ERR_INVALID, "null / empty piece list");
  if (flags & CHIRON_X_ON_DEVICE) return fail(CHIRON_ERR_INVALID, "chiron_engine_submit_pieces takes host pieces");
  long rows = 0;
  for (int i = 0; i < n_pieces; ++i) {
    if (!pieces[i] || piece_rows[i] < 0) return fail(CHIRON_ERR_INVALID, "piece %d: null pointer or negative row count", i);
    if (piece_row_stride && piece_row_stride[i] < 1) return fail(CHIRON_ERR_INVALID, "piece %d: row stride %lld", i, (long long)piece_row_stride[i]);
    rows += piece_rows[i];
  }
  if (rows != batch) return fail(CHIRON_ERR_INVALID, "the pieces hold %ld rows, batch is %d", rows, batch);
  return submit_impl(e, slot, nullptr, pieces, piece_rows, piece_row_stride, n_pieces, seq_len, batch, beam_width, flags);
}

static chiron_status submit_impl(chiron_engine* e, int32_t slot, const float* x, const float* const* pieces, const int32_t* piece_rows,
                                 const int64_t* piece_row_stride, int32_t n_pieces, const int32_t* seq_len, int32_t batch, int32_t beam_width,
                                 uint32_t flags) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  if (slot < 0 || slot >= (int)e->slots.size()) return fail(CHIRON_ERR_STATE, "slot %d out of range (%zu slots)", slot, e->slots.size());
  if (!seq_len) return fail(CHIRON_ERR_INVALID, "null x/seq_len");
  if (batch < 1 || batch > e->maxB) return fail(CHIRON_ERR_OVERFLOW, "batch %d exceeds max_batch %d", batch, e->maxB);
  if (beam_width < 0) return fail(CHIRON_ERR_INVALID, "beam_width %d", beam_width);
  if (beam_width > e->opts.max_beam) return fail(CHIRON_ERR_OVERFLOW, "beam_width %d exceeds max_beam %d given at create", beam_width, e->opts.max_beam);
  Slot* s = &e->slots[slot];
  if (s->state.v.load(std::memory_order_acquire) != 0)
    return fail(CHIRON_ERR_STATE, "slot %d still holds an uncollected batch: collect it before the next submit", slot);
  HIP_TRY(hipSetDevice(e->opts.device_id));
  const int B = batch;
  // Everything from here on puts work on the slot's stream that reads the slot's pinned staging buffers.  If any
  // step fails the stream is drained before returning, so a later submit can never overwrite h_sig / h_seq under a
  // copy that is still running; the slot stays idle.
  auto enqueue = [&]() -> chiron_status {
    const float* sig;
    if (flags & CHIRON_X_ON_DEVICE) {
      sig = x;
      HIP_TRY(hipMemsetAsync(s->seq, 0, e->BP * 4, s->stream));
      HIP_TRY(hipMemcpyAsync(s->seq, seq_len, (size_t)B * 4, hipMemcpyDeviceToDevice, s->stream));
    } else {
      if (!x) {   // cross-read packing (chiron_eval.py:321-334) straight into the staging buffer: the batch is never assembled anywhere else
        size_t row = 0;
        for (int i = 0; i < n_pieces; ++i) {
          const int64_t stride = piece_row_stride ? piece_row_stride[i] : e->L;
          if (stride == e->L) {
            memcpy(s->h_sig + row * e->L, pieces[i], (size_t)piece_rows[i] * e->L * 4);
          } else {   // windows of one signal buffer: row r starts r * jump samples in and overlaps its neighbour (chiron_input.py:276-286)
            for (int r = 0; r < piece_rows[i]; ++r) memcpy(s->h_sig + (row + r) * e->L, pieces[i] + (size_t)r * stride, (size_t)e->L * 4);
          }
          row += piece_rows[i];
        }
      }
      const chiron_status st = stage_input(e, s, x, seq_len, B);
      if (st) return st;
      sig = s->sig;
    }
    if (!run_cnn(e, s, B, sig) || !run_rnn(e, s, B))
      return fail(CHIRON_ERR_INVALID, "a GEMM of this topology has no kernel for the engine's dtype");
    chiron_status st = enqueue_decode(e, s, B, beam_width, flags);
    if (st) return st;
    HIP_TRY(hipGetLastError());
    return CHIRON_OK;
  };
  const chiron_status st = enqueue();
  if (st) {
    s->net_batch = 0;
    resync_tile_counters(s);
    return st;
  }
  s->batch = B;
  s->net_batch = B;
  s->flags = flags;
  s->state.v.store(1, std::memory_order_release);
  return CHIRON_OK;
}

// Decode-only entry: run the decode sub-graph (chiron_eval.py:465-492) on caller-supplied logits.
extern "C" chiron_status chiron_engine_decode(chiron_engine* e, int32_t slot, const float* logits, const int32_t* seq_len,
                                              int32_t batch, int32_t beam_width, uint32_t flags) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  if (slot < 0 || slot >= (int)e->slots.size()) return fail(CHIRON_ERR_STATE, "slot %d out of range (%zu slots)", slot, e->slots.size());
  if (!logits || !seq_len) return fail(CHIRON_ERR_INVALID, "null logits/seq_len");
  if (batch < 1 || batch > e->maxB) return fail(CHIRON_ERR_OVERFLOW, "batch %d exceeds max_batch %d", batch, e->maxB);
  if (beam_width < 0) return fail(CHIRON_ERR_INVALID, "beam_width %d", beam_width);
  if (beam_width > e->opts.max_beam) return fail(CHIRON_ERR_OVERFLOW, "beam_width %d exceeds max_beam %d given at create", beam_width, e->opts.max_beam);
  Slot* s = &e->slots[slot];
  if (s->state.v.load(std::memory_order_acquire) != 0)
    return fail(CHIRON_ERR_STATE, "slot %d still holds an uncollected batch: collect it before the next decode", slot);
  HIP_TRY(hipSetDevice(e->opts.device_id));
  const size_t nlog = (size_t)batch * e->T * e->K * 4;
  auto enqueue = [&]() -> chiron_status {
    HIP_TRY(hipMemsetAsync(s->seq, 0, e->BP * 4, s->stream));
    const hipMemcpyKind kind = (flags & CHIRON_X_ON_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const float* src = logits;
    const int32_t* sl = seq_len;
    if (!(flags & CHIRON_X_ON_DEVICE)) {
      memcpy(s->h_logits, logits, nlog);
      memcpy(s->h_seq, seq_len, (size_t)batch * 4);
      src = s->h_logits;
      sl = s->h_seq;
    }
    HIP_TRY(hipMemcpyAsync(s->logits, src, nlog, kind, s->stream));
    HIP_TRY(hipMemcpyAsync(s->seq, sl, (size_t)batch * 4, kind, s->stream));
    return enqueue_decode(e, s, batch, beam_width, flags & ~CHIRON_WANT_LOGITS);
  };
  const chiron_status st = enqueue();
  s->net_batch = 0;     // the slot's activations no longer belong to the batch it reports
  if (st) {
    hipStreamSynchronize(s->stream);
    return st;
  }
  s->batch = batch;
  s->flags = flags & ~CHIRON_WANT_LOGITS;
  s->state.v.store(1, std::memory_order_release);
  return CHIRON_OK;
}

extern "C" chiron_status chiron_engine_collect(chiron_engine* e, int32_t slot, chiron_decoded* out) {
  if (!e || !out) return fail(CHIRON_ERR_INVALID, "null engine/out");
  if (slot < 0 || slot >= (int)e->slots.size()) return fail(CHIRON_ERR_STATE, "slot %d out of range", slot);
  Slot* s = &e->slots[slot];
  if (s->state.v.load(std::memory_order_acquire) != 1) return fail(CHIRON_ERR_STATE, "collect on slot %d without a submitted batch", slot);
  HIP_TRY(hipSetDevice(e->opts.device_id));
  // A HIP error below loses the batch, not the slot: the stream is drained and the slot returns to idle, as a failed
  // submit leaves it (otherwise every later submit would be refused with "still holds an uncollected batch").
  auto drain = [&]() -> chiron_status {
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int64_t n = s->h_meta[0];
    if (!(s->flags & (CHIRON_NO_DECODE_COPY | CHIRON_COMPACT_DECODE)) && n > 0) {
      HIP_TRY(hipMemcpyAsync(s->h_indices, s->indices, (size_t)n * 16, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(s->h_values, s->values, (size_t)n * 8, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return CHIRON_OK;
  };
  const chiron_status dst = drain();
  if (dst) {
    resync_tile_counters(s);
    s->state.v.store(0, std::memory_order_release);
    return dst;
  }
  const int64_t nnz = s->h_meta[0];
  if (!(s->flags & CHIRON_WANT_PROB)) memset(s->h_prob, 0, (size_t)s->batch * 4);
  out->nnz = nnz;
  const bool compact = (s->flags & CHIRON_COMPACT_DECODE) != 0;
  out->indices = compact ? nullptr : s->h_indices;
  out->values = compact ? nullptr : s->h_values;
  out->flat_labels = nullptr;
  out->row_counts = nullptr;
  if (compact) {
    // the per-read regroup of chiron_eval.py:403-446 needs, per run of rows, the rows' label strings back to back and their lengths:
    // exactly this, in row order, built here in one pass over what the decoder wrote (labels[b][0 .. count[b]))
    const int T = e->T;
    int64_t off = 0;
    for (int b = 0; b < s->batch; ++b) {
      const int c = s->h_count[b];
      if (c < 0 || c > T || off + c > nnz) {
        s->state.v.store(0, std::memory_order_release);
        return fail(CHIRON_ERR_DEVICE, "decoder wrote an impossible row length %d (row %d)", c, b);
      }
      memcpy(s->h_flat + off, s->h_labels + (size_t)b * T, (size_t)c);
      off += c;
    }
    if (off != nnz) {
      s->state.v.store(0, std::memory_order_release);
      return fail(CHIRON_ERR_DEVICE, "row lengths sum to %lld, the SparseTensor holds %lld", (long long)off, (long long)nnz);
    }
    out->flat_labels = s->h_flat;
    out->row_counts = s->h_count;
  }
  out->dense_shape[0] = s->h_meta[1];
  out->dense_shape[1] = s->h_meta[2];
  out->log_prob = s->h_log_prob;
  out->prob_logits = s->h_prob;
  out->logits = (s->flags & CHIRON_WANT_LOGITS) ? s->h_logits : nullptr;
  out->batch = s->batch;
  out->T = e->T;
  s->state.v.store(0, std::memory_order_release);
  return CHIRON_OK;
}

extern "C" chiron_status chiron_engine_sync(chiron_engine* e) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->opts.device_id));
  for (Slot& s : e->slots) HIP_TRY(hipStreamSynchronize(s.stream));
  return CHIRON_OK;
}

extern "C" chiron_status chiron_engine_device_results(chiron_engine* e, int32_t slot, const float** logits,
                                                      const int64_t** indices, const int64_t** values,
                                                      const int64_t** nnz_and_shape) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  if (slot < 0 || slot >= (int)e->slots.size()) return fail(CHIRON_ERR_STATE, "slot %d out of range", slot);
  Slot* s = &e->slots[slot];
  if (logits) *logits = s->logits;
  if (indices) *indices = s->indices;
  if (values) *values = s->values;
  if (nnz_and_shape) *nnz_and_shape = s->meta;
  return CHIRON_OK;
}

// chiron_model.loss (chiron_model.py:50-75) + prediction's edit distance (:101-132) on the slot's last collected batch: device logits,
// device seq_len and the device SparseTensor the decode left behind (enqueue_decode runs launch_sparse on every path)
template <class Tp>
static chiron_status grow(Tp** p, size_t* cap, size_t need) {
  if (need <= *cap && *p) return CHIRON_OK;
  if (*p) HIP_TRY(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  HIP_TRY(hipMalloc((void**)p, (need ? need : 1) * sizeof(Tp)));
  *cap = need;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_engine_score(chiron_engine* e, int32_t slot, const int32_t* labels, const int32_t* label_len, int32_t batch,
                                             int32_t max_label_len, uint32_t flags, float* loss_out, float* edit_out, int32_t* status_out) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  if (slot < 0 || slot >= (int)e->slots.size()) return fail(CHIRON_ERR_STATE, "slot %d out of range", slot);
  if (flags != 0) return fail(CHIRON_ERR_INVALID, "chiron_engine_score: flags must be 0");
  if (!label_len || (!labels && max_label_len > 0) || !loss_out || !edit_out || !status_out || max_label_len < 0)
    return fail(CHIRON_ERR_INVALID, "chiron_engine_score: null operand or negative max_label_len");
  Slot* s = &e->slots[slot];
  if (s->state.v.load(std::memory_order_acquire) != 0) return fail(CHIRON_ERR_STATE, "slot %d holds an uncollected batch", slot);
  if (s->batch <= 0) return fail(CHIRON_ERR_STATE, "no batch has been collected on slot %d", slot);
  if (batch != s->batch) return fail(CHIRON_ERR_STATE, "chiron_engine_score: batch %d, the slot's collected batch has %d rows", batch, s->batch);
  if (e->K != CHIRON_CLASSES) return fail(CHIRON_ERR_INVALID, "chiron_engine_score: CTC over %d classes (A,C,G,T,blank expected)", e->K);
  chiron_status st = ctc_check_rows(nullptr, labels, label_len, batch, e->T, max_label_len);
  if (st) return st;
  int S_ws = 0;
  size_t ws_bytes = 0;
  if ((st = ctc_sizes(batch, e->T, max_label_len, 0, &S_ws, &ws_bytes))) return st;
  if (ctc_lds_bytes(S_ws) > 160 * 1024) return fail(CHIRON_ERR_OVERFLOW, "chiron_engine_score: %d CTC states per frame", S_ws);
  HIP_TRY(hipSetDevice(e->opts.device_id));
  Slot::ScoreBufs& sb = s->score;
  const int words = (max_label_len + 63) / 64;
  const size_t n_lab = (size_t)batch * max_label_len;
  if ((st = grow(&sb.labels, &sb.cap_labels, n_lab))) return st;
  if ((st = grow(&sb.ws, &sb.cap_ws, (size_t)batch * 6 * (words ? words : 1)))) return st;
  if ((size_t)batch > sb.cap_rows || !sb.status) {   // the four per-row buffers grow together
    size_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    sb.cap_rows = 0;
    if ((st = grow(&sb.label_len, &c0, (size_t)batch)) || (st = grow(&sb.loss, &c1, (size_t)batch)) ||
        (st = grow(&sb.edit, &c2, (size_t)batch)) || (st = grow(&sb.status, &c3, (size_t)batch)))
      return st;
    sb.cap_rows = batch;
  }
  auto run = [&]() -> chiron_status {
    if (n_lab) HIP_TRY(hipMemcpyAsync(sb.labels, labels, n_lab * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(sb.label_len, label_len, (size_t)batch * 4, hipMemcpyHostToDevice, s->stream));
    CtcParams p;
    p.logits = s->logits;
    p.seq_len = s->seq;
    p.labels = sb.labels;
    p.label_len = sb.label_len;
    p.B = batch;
    p.T = e->T;
    p.Lmax = max_label_len;
    p.S_ws = S_ws;
    p.S_lds = S_ws;
    p.loss = sb.loss;
    p.grad = nullptr;
    p.alpha = nullptr;
    p.status = sb.status;
    if (launch_ctc(p, false, s->stream) != 0) return fail(CHIRON_ERR_DEVICE, "chiron_engine_score: CTC launch failed");
    EditParams ep{s->indices, s->values, s->meta, sb.labels, sb.label_len, batch, max_label_len, words ? words : 1, sb.ws, sb.edit};
    launch_edit(ep, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(loss_out, sb.loss, (size_t)batch * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(edit_out, sb.edit, (size_t)batch * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(status_out, sb.status, (size_t)batch * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return CHIRON_OK;
  };
  st = run();
  if (st) hipStreamSynchronize(s->stream);
  return st;
}

// getcnnfeature (cnn.py:334-371): the [batch, T, C] feature tensor the CNN handed to the recurrent layers for the batch
// most recently run on an idle slot.
extern "C" chiron_status chiron_engine_features(chiron_engine* e, int32_t slot, float* out, size_t cap_floats, int32_t* out_batch,
                                                int32_t* out_channels) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  if (slot < 0 || slot >= (int)e->slots.size()) return fail(CHIRON_ERR_STATE, "slot %d out of range", slot);
  Slot* s = &e->slots[slot];
  if (s->state.v.load(std::memory_order_acquire) != 0) return fail(CHIRON_ERR_STATE, "slot %d holds an uncollected batch", slot);
  if (s->net_batch < 1 || s->sig_used == nullptr)
    return fail(CHIRON_ERR_STATE, "slot %d holds no network batch (nothing submitted yet, or its last batch was decode-only)", slot);
  const size_t n = (size_t)s->net_batch * e->T * e->C;
  if (out_batch) *out_batch = s->net_batch;
  if (out_channels) *out_channels = e->C;
  if (!out || cap_floats < n) return fail(CHIRON_ERR_OVERFLOW, "features need %zu floats, capacity %zu", n, cap_floats);
  HIP_TRY(hipSetDevice(e->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (e->f16) {
    std::vector<_Float16> h(n);
    HIP_TRY(hipMemcpy(h.data(), s->sig_used, n * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = (float)h[i];
  } else if (e->split) {
    // hi + lo half pairs, per 32-element block of a row 32 hi halves then 32 lo halves (gemm.hip's split epilogue; C is a multiple of 128)
    std::vector<_Float16> h(2 * n);
    HIP_TRY(hipMemcpy(h.data(), s->sig_used, n * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
      const size_t at = (i / 32) * 64 + i % 32;
      out[i] = (float)h[at] + (float)h[at + 32];
    }
  } else {
    HIP_TRY(hipMemcpy(out, s->sig_used, n * 4, hipMemcpyDeviceToHost));
  }
  return CHIRON_OK;
}

// The device pointer behind chiron_engine_features: the frozen CNN's output reaches a trainer (chiron_rnn_train_forward) without a
// host round trip.  Same slot-state rules; fp32 engines only (the other dtypes keep features as halves or hi/lo pairs).
extern "C" chiron_status chiron_engine_device_features(chiron_engine* e, int32_t slot, const float** out_ptr, int32_t* out_batch,
                                                       int32_t* out_channels) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  if (slot < 0 || slot >= (int)e->slots.size()) return fail(CHIRON_ERR_STATE, "slot %d out of range", slot);
  Slot* s = &e->slots[slot];
  if (s->state.v.load(std::memory_order_acquire) != 0) return fail(CHIRON_ERR_STATE, "slot %d holds an uncollected batch", slot);
  if (s->net_batch < 1 || s->sig_used == nullptr)
    return fail(CHIRON_ERR_STATE, "slot %d holds no network batch (nothing submitted yet, or its last batch was decode-only)", slot);
  if (e->split || e->f16) return fail(CHIRON_ERR_INVALID, "chiron_engine_device_features: fp32 engines only");
  if (!out_ptr) return fail(CHIRON_ERR_INVALID, "chiron_engine_device_features: null out_ptr");
  *out_ptr = (const float*)s->sig_used;
  if (out_batch) *out_batch = s->net_batch;
  if (out_channels) *out_channels = e->C;
  return CHIRON_OK;
}

// Bias correction of the f16 engine (post-training-quantisation style, data dependent only through per-channel MEANS of a
// calibration batch): run the network, measure the mean of every input channel of every f16 weight matrix, move
// sum_k E[x_k] (f16(W) - W)[n][k] out of the shift / LSTM bias of output n.  Upstream corrections move downstream means a little,
// hence `iterations` (2 is enough).  tools/f16_study.py: on trained-checkpoint-like weights the mean term is most of what rounding
// the weights to halves costs.
extern "C" chiron_status chiron_engine_calibrate(chiron_engine* e, const float* x, const int32_t* seq_len, int32_t batch, int32_t iterations) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  if (iterations < 0 || iterations > 16) return fail(CHIRON_ERR_INVALID, "iterations %d", iterations);
  if (iterations > 0) {     // iterations = 0 only restores the uncorrected shifts: it reads no calibration data
    if (!x || !seq_len) return fail(CHIRON_ERR_INVALID, "null x/seq_len");
    if (batch < 1 || batch > e->maxB) return fail(CHIRON_ERR_OVERFLOW, "batch %d exceeds max_batch %d", batch, e->maxB);
  }
  if (!e->f16 || e->w2) return CHIRON_OK;      // fp32 / fp32-split / hi + lo weights are not rounded: nothing to correct
  Slot* s = &e->slots[0];
  for (Slot& sl : e->slots)
    if (sl.state.v.load(std::memory_order_acquire) != 0) return fail(CHIRON_ERR_STATE, "chiron_engine_calibrate needs every slot idle");
  HIP_TRY(hipSetDevice(e->opts.device_id));
  const int B = batch, H = e->H;
  CalibCtx ctx;
  ctx.max_records = 256;
  HIP_TRY(hipMalloc((void**)&ctx.dev_sums, ctx.max_records * 256 * sizeof(double)));
  struct FreeSums {            // every exit path below, early ones included
    double* p;
    ~FreeSums() { (void)hipFree(p); }
  } free_sums{ctx.dev_sums};
  chiron_status st = CHIRON_OK;
  std::vector<double> sums(ctx.max_records * 256);
  for (int it = 0; it < iterations && st == CHIRON_OK; ++it) {
    ctx.rec.clear();
    ctx.skipped = 0;
    auto run = [&]() -> chiron_status {
      HIP_TRY(hipMemsetAsync(ctx.dev_sums, 0, ctx.max_records * 256 * sizeof(double), s->stream));
      const chiron_status staged = stage_input(e, s, x, seq_len, B);
      if (staged) return staged;
      e->calib = &ctx;
      const bool ok = run_cnn(e, s, B, s->sig) && run_rnn(e, s, B);
      e->calib = nullptr;
      if (!ok) return fail(CHIRON_ERR_INVALID, "a GEMM of this topology has no kernel for the engine's dtype");
      HIP_TRY(hipStreamSynchronize(s->stream));
      HIP_TRY(hipMemcpy(sums.data(), ctx.dev_sums, ctx.rec.size() * 256 * sizeof(double), hipMemcpyDeviceToHost));
      return CHIRON_OK;
    };
    st = run();
    s->net_batch = 0;
    if (st == CHIRON_OK && ctx.skipped)
      st = fail(CHIRON_ERR_OVERFLOW, "calibration could not measure %d of the network's inputs (more than 256 channels, or more than %zu "
                "measured inputs): no correction applied.  Run this model uncorrected (`chiron call --no-calibration`, "
                "Engine(calibrate=False), `serve.py --no-calibration`) or with dtype fp16-w2, whose weights are exact", ctx.skipped, ctx.max_records);
    if (st) {
      resync_tile_counters(s);
      break;
    }
    // corrections, always from the ORIGINAL shifts: correction[n] = - sum over the records of the plan of sum_c mean[c] * dW[n][k0 + c]
    std::map<const float*, std::vector<double>> corr;
    const int parts = getenv("CHIRON_CALIB_PARTS") ? atoi(getenv("CHIRON_CALIB_PARTS")) : 7;   // diagnostics: 1 convolutions, 2 LSTM x rows, 4 LSTM h rows
    for (const CalibRecord& r : ctx.rec) {
      auto ph = e->plan_host.find(r.shift);
      if (ph == e->plan_host.end() || r.rows <= 0) continue;
      if (!(parts & (r.lstm_layer < 0 ? 1 : r.lstm_part == 0 ? 2 : 4))) continue;
      std::vector<double>& c = corr[r.shift];
      c.resize(ph->second.Npad, 0.0);
      const double* sm = &sums[r.slot * 256];
      if (r.lstm_layer < 0) {
        const PlanHost& P = ph->second;
        for (int n = 0; n < P.N; ++n) {
          double a = 0;
          for (int k = 0; k < r.cin; ++k) a += sm[k] * (double)P.dW[(size_t)n * P.K + r.k0 + k];
          c[n] -= a / r.rows;
        }
      } else {
        // rows of the TF kernel [(in_w + H)][4H] of layer l, direction d: x rows (part 0) or h rows (part 1); output column n of the
        // plan = dir * 4H + gate * H + unit (one direction per plan in the MultiRNN layers above 0)
        const LstmPlan& lp = e->lstm[r.lstm_layer];
        const int zc = 4 * H;
        for (int dir = 0; dir < 2; ++dir) {
          if (r.lstm_dir >= 0 && dir != r.lstm_dir) continue;
          const float* kern = e->host_weights.data() + e->map.lstm_kernel[r.lstm_layer][dir];
          const int row0 = r.lstm_part == 0 ? 0 : lp.in_w;
          const int nbase = lp.nproj == 1 ? dir * zc : 0;
          for (int col = 0; col < zc; ++col) {
            double a = 0;
            for (int k = 0; k < r.cin; ++k) {
              const float wv = kern[(size_t)(row0 + k) * zc + col];
              a += sm[k] * ((double)(float)(_Float16)wv - (double)wv);
            }
            c[nbase + col] -= a / r.rows;
          }
        }
      }
    }
    for (auto& kv : corr) {
      const PlanHost& P = e->plan_host[kv.first];
      std::vector<float> sh(P.shift0);
      for (int n = 0; n < P.Npad; ++n) sh[n] = (float)((double)P.shift0[n] + kv.second[n]);
      if (hipMemcpy(const_cast<float*>(kv.first), sh.data(), sh.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        st = fail(CHIRON_ERR_DEVICE, "uploading a corrected shift failed");
        break;
      }
    }
    if (st == CHIRON_OK) e->calibrated = it + 1;
  }
  if (iterations == 0) {   // back to the uncorrected engine
    for (auto& kv : e->plan_host)
      if (hipMemcpy(const_cast<float*>(kv.first), kv.second.shift0.data(), kv.second.shift0.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        st = fail(CHIRON_ERR_DEVICE, "restoring a shift failed");
    e->calibrated = 0;
  }
  return st;
}

// The recurrent stack's output (rnn.py:63-65 / :140-145, the tensor the FC head of rnn.py:72-96 reads), re-ordered from the
// engine's time-major [T][BP][2H] to the reference's [batch, T, 2H].
extern "C" chiron_status chiron_engine_rnn_output(chiron_engine* e, int32_t slot, float* out, size_t cap_floats, int32_t* out_batch,
                                                  int32_t* out_width) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  if (slot < 0 || slot >= (int)e->slots.size()) return fail(CHIRON_ERR_STATE, "slot %d out of range", slot);
  Slot* s = &e->slots[slot];
  if (s->state.v.load(std::memory_order_acquire) != 0) return fail(CHIRON_ERR_STATE, "slot %d holds an uncollected batch", slot);
  if (s->net_batch < 1 || s->rnn_out == nullptr)
    return fail(CHIRON_ERR_STATE, "slot %d holds no network batch (nothing submitted yet, or its last batch was decode-only)", slot);
  if (e->split) return fail(CHIRON_ERR_INVALID, "chiron_engine_rnn_output: not exported for dtype fp32-split");
  const int B = s->net_batch, T = e->T, W = 2 * e->H, BP = e->BP, ld = e->lasth_ld;
  const size_t n = (size_t)B * T * W;
  if (out_batch) *out_batch = B;
  if (out_width) *out_width = W;
  if (!out || cap_floats < n) return fail(CHIRON_ERR_OVERFLOW, "the recurrent output needs %zu floats, capacity %zu", n, cap_floats);
  HIP_TRY(hipSetDevice(e->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  const size_t all = (size_t)T * BP * ld;
  if (!s->rnn_out_f32) {
    std::vector<_Float16> h(all);
    HIP_TRY(hipMemcpy(h.data(), s->rnn_out, all * 2, hipMemcpyDeviceToHost));
    for (int t = 0; t < T; ++t)
      for (int b = 0; b < B; ++b)
        for (int k = 0; k < W; ++k) out[((size_t)b * T + t) * W + k] = (float)h[((size_t)t * BP + b) * ld + k];
  } else {
    std::vector<float> h(all);
    HIP_TRY(hipMemcpy(h.data(), s->rnn_out, all * 4, hipMemcpyDeviceToHost));
    for (int t = 0; t < T; ++t)
      for (int b = 0; b < B; ++b) memcpy(out + ((size_t)b * T + t) * W, h.data() + ((size_t)t * BP + b) * ld, (size_t)W * 4);
  }
  return CHIRON_OK;
}

extern "C" chiron_status chiron_engine_profile(chiron_engine* e, int32_t enable) {
  if (!e) return fail(CHIRON_ERR_INVALID, "null engine");
  chiron_status st = chiron_engine_sync(e);
  if (st) return st;
  for (Slot& s : e->slots) {
    for (ProfEvent& ev : s.events) {
      hipEventDestroy(ev.a);
      hipEventDestroy(ev.b);
    }
    s.events.clear();
  }
  e->profiling = enable != 0;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_engine_profile_read(chiron_engine* e, chiron_kernel_stat* stats, int32_t max_stats,
                                                    int32_t* n_stats) {
  if (!e || !stats || !n_stats) return fail(CHIRON_ERR_INVALID, "null argument");
  chiron_status st = chiron_engine_sync(e);
  if (st) return st;
  std::vector<chiron_kernel_stat> acc(e->prof_names.size());
  for (size_t i = 0; i < acc.size(); ++i) {
    memset(&acc[i], 0, sizeof(acc[i]));
    snprintf(acc[i].name, sizeof(acc[i].name), "%s", e->prof_names[i].c_str());
  }
  for (Slot& s : e->slots)
    for (ProfEvent& ev : s.events) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev.a, ev.b) != hipSuccess) continue;
      chiron_kernel_stat& k = acc[ev.name_id];
      k.total_ms += ms;
      k.launches += 1;
      k.flops += ev.flops;
      k.bytes += ev.bytes;
    }
  int n = 0;
  for (size_t i = 0; i < acc.size() && n < max_stats; ++i)
    if (acc[i].launches > 0) stats[n++] = acc[i];
  *n_stats = n;
  return CHIRON_OK;
}
