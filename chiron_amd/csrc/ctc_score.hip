// CTC log-likelihoods of very many short, ragged (frame segment, candidate label) problems on gfx950: what `polish` asks when it
// rescores a pileup variant with the reads' own frame posteriors.  The definition is in include/chiron_amd.h and is restated in
// numpy float64 by tests/polish_ref.py.
//
//   score_softmax_kernel  one thread per frame: the double log-softmax of every frame of the call, [frames][5], written once
//                         into the workspace.  Both alleles of a variant, neighbouring variants and every candidate of an item
//                         read the same frames.
//   ctc_score_kernel      one wavefront per candidate, four to a workgroup; candidate c runs on wave c mod the launch's waves.
//                         Lane j keeps the states 4j .. 4j+3 of the S = 2L+1 <= 255 in registers, in double.  State 4j is a
//                         blank, so it has no s-2 predecessor, and of everything a lane reads only alpha(4j-1) lives in another
//                         lane: one __shfl_up of a double per frame.  No LDS row and no barrier (ctc_alpha_kernel of ctc_loss.hip
//                         has both).  A frame's five log-probabilities are loaded before its four lse chains, which do not
//                         depend on them, and added after.
//                         A lane's classes, its "s-2 allowed" bits and its "s < S" bits are packed once per candidate, one byte a
//                         state as in ctc_loss.hip; a state's log-probability is picked by compares, never by an indexed table,
//                         which the compiler would put into scratch.
//
// No atomics and no sum across candidates: a value depends on its candidate alone, whatever else the call holds and in whatever
// order.  Every offset is 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/chiron_amd.h"
#include "align_common.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_SCORE_THREADS;
constexpr int WAVES = NT / 64;
constexpr int BLANK = 4;
constexpr int64_t MAX_FRAMES_TOTAL = (int64_t)1 << 40;   // frames of one call: keeps every byte count far below 2^63

struct ScoreCand {
  int64_t frame0;   // first frame of the candidate's item
  int64_t label0;   // first base in `labels`
  int32_t T, L;
};

struct ScoreParams {
  const float* scores;      // [frames][5]
  double* lp;               // [frames][5]
  const uint8_t* labels;
  const ScoreCand* cand;    // [candidates]
  int64_t frames, candidates;
  double* loglik;           // [candidates]
  int32_t* status;          // [candidates]
};

struct ScoreLayout {
  size_t cand, scores, lp, labels, loglik, status, bytes;
};

__device__ __forceinline__ double ninf() { return -INFINITY; }

// m + log(sum exp(. - m)) in the order given; -inf when every operand is (m is then replaced by 0: log(0) gives the -inf).
// lse2 is lse3 with a third operand of -inf, whose term is an exact 0: a blank state never has an s-2 predecessor, so its third
// exp is not computed.  (Leaving out the largest operand's exp(0) as well and taking log1p of the rest was tried: log1p costs
// more than the saved exp gives, 7.35 against 7.11 ms on the workload of tools/bench_polish.py, and the value no longer is
// the header's sum term for term.)
__device__ __forceinline__ double lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  const double mm = m == ninf() ? 0.0 : m;
  return mm + log(exp(a - mm) + exp(b - mm) + exp(c - mm));
}
__device__ __forceinline__ double lse2(double a, double b) {
  const double m = fmax(a, b);
  const double mm = m == ninf() ? 0.0 : m;
  return mm + log(exp(a - mm) + exp(b - mm));
}

// the log-probability of the class in bits 0..2 of e
__device__ __forceinline__ double pick(int e, double l0, double l1, double l2, double l3, double l4) {
  const int c = e & 7;
  return c == 0 ? l0 : c == 1 ? l1 : c == 2 ? l2 : c == 3 ? l3 : l4;
}

__global__ __launch_bounds__(CHIRON_SCORE_THREADS) void score_softmax_kernel(ScoreParams p) {
  for (int64_t f = (int64_t)blockIdx.x * NT + threadIdx.x; f < p.frames; f += (int64_t)gridDim.x * NT) {
    const float* x = p.scores + f * 5;
    const double x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4];
    const double m = fmax(fmax(fmax(x0, x1), fmax(x2, x3)), x4);
    const double d0 = x0 - m, d1 = x1 - m, d2 = x2 - m, d3 = x3 - m, d4 = x4 - m;
    const double l = log((((exp(d0) + exp(d1)) + exp(d2)) + exp(d3)) + exp(d4));
    double* o = p.lp + f * 5;
    o[0] = d0 - l;
    o[1] = d1 - l;
    o[2] = d2 - l;
    o[3] = d3 - l;
    o[4] = d4 - l;
  }
}

constexpr int E_ALLOW = 8, E_VALID = 16;

__global__ __launch_bounds__(CHIRON_SCORE_THREADS) void ctc_score_kernel(ScoreParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  for (int64_t c = wave; c < p.candidates; c += nwaves) {
    const ScoreCand cd = p.cand[c];
    const int T = cd.T, L = cd.L, S = 2 * L + 1;
    const uint8_t* lab = p.labels + cd.label0;
    // lane j: base 2j under state 4j+1, base 2j+1 under state 4j+3, and base 2j-1 for the repeat rule
    const int j0 = 2 * lane;
    const int bm = (j0 >= 1 && j0 - 1 < L) ? lab[j0 - 1] : BLANK;
    const int b0 = j0 < L ? lab[j0] : BLANK;
    const int b1 = j0 + 1 < L ? lab[j0 + 1] : BLANK;
    int rep = (j0 >= 1 && j0 < L && b0 == bm) + (j0 + 1 < L && b1 == b0);
    for (int o = 32; o >= 1; o >>= 1) rep += __shfl_xor(rep, o, 64);
    if (T < L + rep) {
      if (lane == 0) {
        p.loglik[c] = ninf();
        p.status[c] = 1;
      }
      continue;
    }
    if (T == 0) {   // L == 0 here: the empty path
      if (lane == 0) {
        p.loglik[c] = 0.0;
        p.status[c] = 0;
      }
      continue;
    }
    // one byte a state: bits 0..2 the class, bit 3 "s-2 allowed", bit 4 "s < S"
    const int s0 = 4 * lane;
    const int e0 = BLANK | (s0 < S ? E_VALID : 0);
    const int e1 = b0 | ((j0 >= 1 && j0 < L && bm != b0) ? E_ALLOW : 0) | (s0 + 1 < S ? E_VALID : 0);
    const int e2 = BLANK | (s0 + 2 < S ? E_VALID : 0);
    const int e3 = b1 | ((j0 + 1 < L && b0 != b1) ? E_ALLOW : 0) | (s0 + 3 < S ? E_VALID : 0);
    const double* lp = p.lp + cd.frame0 * 5;
    double l0 = lp[0], l1 = lp[1], l2 = lp[2], l3 = lp[3], l4 = lp[4];
    double a0 = lane == 0 ? l4 : ninf();
    double a1 = (lane == 0 && L >= 1) ? pick(e1, l0, l1, l2, l3, l4) : ninf();
    double a2 = ninf(), a3 = ninf();
    for (int t = 1; t < T; ++t) {
      const double* nx = lp + (int64_t)t * 5;
      l0 = nx[0];
      l1 = nx[1];
      l2 = nx[2];
      l3 = nx[3];
      l4 = nx[4];
      double pm = __shfl_up(a3, 1, 64);   // alpha(4j-1)
      if (lane == 0) pm = ninf();
      const double n0 = lse2(a0, pm) + l4;
      const double n1 = lse3(a1, a0, (e1 & E_ALLOW) ? pm : ninf()) + pick(e1, l0, l1, l2, l3, l4);
      const double n2 = lse2(a2, a1) + l4;
      const double n3 = lse3(a3, a2, (e3 & E_ALLOW) ? a1 : ninf()) + pick(e3, l0, l1, l2, l3, l4);
      a0 = (e0 & E_VALID) ? n0 : ninf();
      a1 = (e1 & E_VALID) ? n1 : ninf();
      a2 = (e2 & E_VALID) ? n2 : ninf();
      a3 = (e3 & E_VALID) ? n3 : ninf();
    }
    // alpha(S-1) and alpha(S-2): picked in their lanes by a wave-uniform index, then read from there
    const int k1 = (S - 1) & 3, k2 = (S - 2) & 3;
    const double m1 = k1 == 0 ? a0 : k1 == 1 ? a1 : k1 == 2 ? a2 : a3;
    const double m2 = k2 == 0 ? a0 : k2 == 1 ? a1 : k2 == 2 ? a2 : a3;
    const double vlast = __shfl(m1, (S - 1) >> 2, 64);
    const double vprev = S >= 2 ? __shfl(m2, (S - 2) >> 2, 64) : ninf();
    if (lane == 0) {
      p.loglik[c] = lse2(vlast, vprev);
      p.status[c] = 0;
    }
  }
}

chiron_status score_sizes(const char* who, int64_t frames, int64_t items, int64_t candidates, int64_t label_bytes, ScoreLayout* l) {
  memset(l, 0, sizeof(*l));
  if (frames < 0 || items < 0 || candidates < 0 || label_bytes < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative size (frames %lld, items %lld, candidates %lld, label bytes %lld)", who, (long long)frames,
                     (long long)items, (long long)candidates, (long long)label_bytes);
  if (items > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld items in one call, at most 2^24", who, (long long)items);
  if (candidates > MAX_BATCH_ITEMS)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld candidates in one call, at most 2^24", who, (long long)candidates);
  if (frames > MAX_FRAMES_TOTAL) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld frames in one call, at most 2^40", who, (long long)frames);
  if (label_bytes > candidates * CHIRON_SCORE_MAX_LABEL)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld label bytes for %lld candidates of at most %d bases", who, (long long)label_bytes,
                     (long long)candidates, CHIRON_SCORE_MAX_LABEL);
  l->cand = 0;
  l->scores = l->cand + up256((size_t)candidates * sizeof(ScoreCand));
  l->lp = l->scores + up256((size_t)frames * 5 * sizeof(float));
  l->labels = l->lp + up256((size_t)frames * 5 * sizeof(double));
  l->loglik = l->labels + up256((size_t)label_bytes);
  l->status = l->loglik + up256((size_t)candidates * sizeof(double));
  l->bytes = l->status + up256((size_t)candidates * sizeof(int32_t));
  return CHIRON_OK;
}

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_ctc_score_workspace_size(int64_t frames, int64_t items, int64_t candidates, int64_t label_bytes, size_t* bytes) {
  const char* who = "chiron_ctc_score_workspace_size";
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  ScoreLayout l;
  if (chiron_status st = score_sizes(who, frames, items, candidates, label_bytes, &l)) return st;
  *bytes = (items == 0 || candidates == 0) ? 0 : l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_ctc_score(int32_t device_id, const float* scores, int64_t frames, const int64_t* item_begin,
                                          const int64_t* item_end, const int64_t* cand_off, int64_t items, const uint8_t* labels,
                                          const int64_t* label_off, int64_t candidates, uint32_t flags, double* loglik_out, int32_t* status_out,
                                          void* workspace, void* stream_) {
  const char* who = "chiron_ctc_score";
  if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  ScoreLayout l;
  if (chiron_status st = score_sizes(who, frames, items, candidates, 0, &l)) return st;
  if (items == 0 || candidates == 0) return CHIRON_OK;
  if (!item_begin || !item_end || !cand_off || !label_off) return set_error(CHIRON_ERR_INVALID, "%s: null offsets", who);
  if (!loglik_out || !status_out) return set_error(CHIRON_ERR_INVALID, "%s: null output", who);
  if (frames > 0 && !scores) return set_error(CHIRON_ERR_INVALID, "%s: null scores", who);
  if (cand_off[0] != 0) return set_error(CHIRON_ERR_INVALID, "%s: cand_off[0] = %lld, the first item's candidates start at 0", who, (long long)cand_off[0]);
  for (int64_t i = 0; i < items; ++i) {
    if (cand_off[i + 1] < cand_off[i])
      return set_error(CHIRON_ERR_INVALID, "%s: cand_off[%lld] = %lld below its predecessor %lld", who, (long long)(i + 1), (long long)cand_off[i + 1],
                       (long long)cand_off[i]);
    if (cand_off[i + 1] > candidates)
      return set_error(CHIRON_ERR_INVALID, "%s: cand_off[%lld] = %lld past the %lld candidates", who, (long long)(i + 1), (long long)cand_off[i + 1],
                       (long long)candidates);
    if (item_begin[i] < 0 || item_end[i] < item_begin[i] || item_end[i] > frames)
      return set_error(CHIRON_ERR_INVALID, "%s: item %lld covers frames %lld .. %lld, outside 0 .. %lld", who, (long long)i, (long long)item_begin[i],
                       (long long)item_end[i], (long long)frames);
    if (item_end[i] - item_begin[i] > CHIRON_SCORE_MAX_FRAMES)
      return set_error(CHIRON_ERR_OVERFLOW, "%s: item %lld has %lld frames, at most %d", who, (long long)i, (long long)(item_end[i] - item_begin[i]),
                       CHIRON_SCORE_MAX_FRAMES);
  }
  if (cand_off[items] != candidates)
    return set_error(CHIRON_ERR_INVALID, "%s: cand_off[%lld] = %lld, the items own %lld candidates", who, (long long)items, (long long)cand_off[items],
                     (long long)candidates);
  int64_t longest = 0, label_total = 0;
  if (chiron_status st = check_offsets(who, "label", "candidate", "bases", label_off, candidates, CHIRON_SCORE_MAX_LABEL, &longest, &label_total)) return st;
  // every offset has passed: only now the records, 24 bytes a candidate
  std::vector<ScoreCand> recs((size_t)candidates);
  for (int64_t i = 0; i < items; ++i)
    for (int64_t c = cand_off[i]; c < cand_off[i + 1]; ++c)
      recs[(size_t)c] = ScoreCand{item_begin[i], label_off[c] - label_off[0], (int32_t)(item_end[i] - item_begin[i]), (int32_t)(label_off[c + 1] - label_off[c])};
  const int64_t label_bytes = label_off[candidates] - label_off[0];
  if (label_bytes > 0 && !labels) return set_error(CHIRON_ERR_INVALID, "%s: null labels", who);
  const uint8_t* lab = labels ? labels + label_off[0] : nullptr;
  for (int64_t i = 0; i < label_bytes; ++i)
    if (lab[i] > 3) return set_error(CHIRON_ERR_INVALID, "%s: code %d at base %lld outside 0..3", who, (int)lab[i], (long long)(label_off[0] + i));
  for (int64_t i = 0; i < frames * 5; ++i)
    if (!std::isfinite(scores[i]))
      return set_error(CHIRON_ERR_INVALID, "%s: score %lld of frame %lld is not finite", who, (long long)(i % 5), (long long)(i / 5));
  if (chiron_status st = score_sizes(who, frames, items, candidates, label_bytes, &l)) return st;
  if (chiron_status st = use_device_workspace(who, device_id, workspace)) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.cand, recs.data(), recs.size() * sizeof(ScoreCand), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (frames > 0 && hipMemcpyAsync(ws + l.scores, scores, (size_t)frames * 5 * sizeof(float), hipMemcpyHostToDevice, stream) != hipSuccess) ||
      (label_bytes > 0 && hipMemcpyAsync(ws + l.labels, lab, (size_t)label_bytes, hipMemcpyHostToDevice, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "%s: copying the candidates to the device failed", who);
  ScoreParams p;
  p.scores = (const float*)(ws + l.scores);
  p.lp = (double*)(ws + l.lp);
  p.labels = (const uint8_t*)(ws + l.labels);
  p.cand = (const ScoreCand*)(ws + l.cand);
  p.frames = frames;
  p.candidates = candidates;
  p.loglik = (double*)(ws + l.loglik);
  p.status = (int32_t*)(ws + l.status);
  if (frames > 0) {
    const int64_t want = (frames + NT - 1) / NT;
    hipLaunchKernelGGL(score_softmax_kernel, dim3((unsigned)(want < CHIRON_SCORE_MAX_GROUPS ? want : CHIRON_SCORE_MAX_GROUPS)), dim3(NT), 0, stream, p);
    if (chiron_status st = launched(who)) return st;
  }
  const int64_t groups = (candidates + WAVES - 1) / WAVES;
  hipLaunchKernelGGL(ctc_score_kernel, dim3((unsigned)(groups < CHIRON_SCORE_MAX_GROUPS ? groups : CHIRON_SCORE_MAX_GROUPS)), dim3(NT), 0, stream, p);
  if (chiron_status st = launched(who)) return st;
  if (hipMemcpyAsync(loglik_out, ws + l.loglik, (size_t)candidates * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(status_out, ws + l.status, (size_t)candidates * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "%s: the scoring kernels failed (%s)", who, hipGetErrorString(hipGetLastError()));
  return CHIRON_OK;
}
