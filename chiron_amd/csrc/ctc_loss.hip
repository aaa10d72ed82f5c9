// CTC loss, its gradient with respect to the logits, and the normalized edit distance for gfx950: what the reference's
// training loop evaluates on labelled windows, chiron_model.loss() (chiron/chiron_model.py:50-75: tf.nn.ctc_loss with
// ctc_merge_repeated=True, ignore_longer_outputs_than_inputs=True) and chiron_model.prediction() (:101-132:
// tf.edit_distance(decoded, label, normalize=True)).
//
//   ctc_alpha_kernel  one wavefront per window: the log-space forward recursion over the extended label l' (S = 2L+1 states,
//                     blank = class 4 between and around the labels), in double.  The alpha row is one LDS row of S doubles,
//                     updated in place; lane j owns the states j, j+64, j+128, ...  One barrier per frame.  The loss is
//                     -logsumexp(alpha_{T-1}(S-1), alpha_{T-1}(S-2)).  With a workspace, every frame's alpha row also goes to
//                     it, in double ([B][T][S_max], 64-bit offsets), for the backward pass.
//   ctc_beta_kernel   one wavefront per window: the backward recursion in the same layout, and per frame the class posteriors
//                     sum_{s: l'(s)=k} exp(alpha_t(s) + beta_t(s) - lp_t(s) - log p) reduced over the wave in a fixed order and
//                     normalised to sum 1 per frame; grad(t,k) = softmax(t,k) - posterior(t,k) (TF's gradient with respect to
//                     the pre-softmax logits).
//   edit_kernel       one thread per row: Levenshtein distance of the row's decoded labels (read from the SparseTensor
//                     (indices, values) the decoder left on the device) against its truth, by Myers' bit-vector algorithm in
//                     blocks of 64 truth positions (Myers 1999, "advance_block"; alphabet 4), divided by the truth length.
//
// Deterministic: no atomics; every sum has a fixed order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/chiron_amd.h"
#include "bitvector.h"
#include "host_entry.h"
#include "kernels.h"

namespace chiron {

namespace {

constexpr int CTC_BLANK = 4;
constexpr int CTC_K = 5;

__device__ __forceinline__ double lse2(double a, double b) {
  const double m = fmax(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m));
}

__device__ __forceinline__ double lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

struct Frame {   // one frame's log-softmax over the 5 classes, in double
  double lp0, lp1, lp2, lp3, lp4;
};

// The states read the frame's log-softmax by class from LDS: a lookup in registers is compiled into a table in scratch memory,
// which would sit in the dependent chain of every frame.  Lanes 0..4 write it; every lane computes the same Frame.
__device__ __forceinline__ void put_frame(const Frame& f, volatile double* lpb) {
  const int lane = threadIdx.x;
  if (lane < CTC_K) lpb[lane] = lane == 0 ? f.lp0 : lane == 1 ? f.lp1 : lane == 2 ? f.lp2 : lane == 3 ? f.lp3 : f.lp4;
}

__device__ __forceinline__ void load_frame(const float* x, float* v) {
#pragma unroll
  for (int k = 0; k < CTC_K; ++k) v[k] = x[k];
}

// log-softmax over the 5 classes of one frame, in double from the float32 logits
__device__ __forceinline__ Frame log_softmax5(const float* x) {
  const double x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4];
  const double m = fmax(fmax(fmax(x0, x1), fmax(x2, x3)), x4);
  const double lse = m + log(exp(x0 - m) + exp(x1 - m) + exp(x2 - m) + exp(x3 - m) + exp(x4 - m));
  return Frame{x0 - lse, x1 - lse, x2 - lse, x3 - lse, x4 - lse};
}

// fixed-order butterfly; every lane ends with the same value
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct RowInfo {
  int Tb, L, status;   // status: 0 scored, 1 skipped (L > Tb), 2 infeasible (L + repeats > Tb)
};

__device__ RowInfo row_info(const CtcParams& p, int b) {
  RowInfo r;
  int tb = p.seq_len[b];
  tb = tb < 0 ? 0 : (tb > p.T ? p.T : tb);
  int L = p.label_len[b];
  L = L < 0 ? 0 : (L > p.Lmax ? p.Lmax : L);   // checked on the host unless CHIRON_CTC_TRUSTED; clamped here either way
  r.Tb = tb;
  r.L = L;
  r.status = 0;
  if (r.L > r.Tb) {
    r.status = 1;
    return r;
  }
  const int32_t* lab = p.labels + (size_t)b * p.Lmax;
  int rep = 0;
  for (int i = (int)threadIdx.x + 1; i < r.L; i += 64) rep += lab[i] == lab[i - 1];
  rep = wave_sum_i(rep);
  if (r.L + rep > r.Tb) r.status = 2;
  return r;
}

// extended label: bits 0..2 the class of state s, bit 3 "the transition s-2 -> s is allowed"
__device__ void fill_ext(const CtcParams& p, int b, int L, uint8_t* ext) {
  const int32_t* lab = p.labels + (size_t)b * p.Lmax;
  const int S = 2 * L + 1;
  for (int s = threadIdx.x; s < S; s += 64) {
    int v = CTC_BLANK;
    if (s & 1) {
      const int i = s >> 1;
      v = lab[i] & 3;
      if (i >= 1 && (lab[i - 1] & 3) != v) v |= 8;
    }
    ext[s] = (uint8_t)v;
  }
}

// The recursions keep ONE row of S doubles in LDS and update it in place: alpha_t(s) reads alpha_{t-1}(s, s-1, s-2), so the
// forward pass walks the 64-state chunks from the last to the first (a chunk reads itself and the chunk before, neither written
// yet this frame; within a chunk every lane's loads are issued before its store, one wavefront), the backward pass from the first
// to the last.  volatile keeps the compiler from caching or reordering these cross-lane LDS accesses.  Doubles: an fp32 recursion
// rounds every state at every frame, and at T = 400 that alone moves the gradient by 1e-5.
__global__ __launch_bounds__(64) void ctc_alpha_kernel(const CtcParams p) {
  extern __shared__ double smem[];
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  volatile double* buf = smem;
  volatile double* lpb = smem + p.S_lds;
  uint8_t* ext = reinterpret_cast<uint8_t*>(smem + p.S_lds + 8);
  const RowInfo r = row_info(p, b);
  if (r.status != 0 || r.Tb == 0) {   // Tb == 0 with status 0 means L == 0: p(empty | empty) = 1
    if (lane == 0) {
      p.loss[b] = r.status == 2 ? INFINITY : 0.f;
      if (p.status) p.status[b] = r.status;
    }
    return;
  }
  const int S = 2 * r.L + 1;
  const int nch = (S + 63) >> 6;
  fill_ext(p, b, r.L, ext);
  const float* x = p.logits + (size_t)b * p.T * CTC_K;
  double* alpha = p.alpha ? p.alpha + (size_t)b * p.T * p.S_ws : nullptr;
  float nxt[CTC_K];
  put_frame(log_softmax5(x), lpb);
  if (r.Tb > 1) load_frame(x + CTC_K, nxt);
  __syncthreads();
  for (int s = lane; s < S; s += 64) {
    const double a = s < 2 ? lpb[ext[s] & 7] : -INFINITY;
    buf[s] = a;
    if (alpha) alpha[s] = a;
  }
  for (int t = 1; t < r.Tb; ++t) {
    const Frame f = log_softmax5(nxt);
    if (t + 1 < r.Tb) load_frame(x + (size_t)(t + 1) * CTC_K, nxt);
    __syncthreads();
    put_frame(f, lpb);
    double* arow = alpha ? alpha + (size_t)t * p.S_ws : nullptr;
    for (int j = nch - 1; j >= 0; --j) {
      const int s = lane + 64 * j;
      if (s < S) {
        const int e = ext[s];
        const double a0 = buf[s];
        const double a1 = s >= 1 ? buf[s - 1] : -INFINITY;
        const double a2 = (e & 8) ? buf[s - 2] : -INFINITY;
        const double a = lse3(a0, a1, a2) + lpb[e & 7];
        buf[s] = a;
        if (arow) arow[s] = a;
      }
    }
  }
  __syncthreads();
  if (lane == 0) {
    const double ll = S >= 2 ? lse2(buf[S - 1], buf[S - 2]) : buf[S - 1];
    p.loss[b] = (float)-ll;
    if (p.status) p.status[b] = 0;
  }
}

__global__ __launch_bounds__(64) void ctc_beta_kernel(const CtcParams p) {
  extern __shared__ double smem[];
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  volatile double* buf = smem;
  volatile double* lpb = smem + p.S_lds;
  uint8_t* ext = reinterpret_cast<uint8_t*>(smem + p.S_lds + 8);
  float* g = p.grad + (size_t)b * p.T * CTC_K;
  const RowInfo r = row_info(p, b);
  const int t0 = (r.status != 0) ? 0 : r.Tb;   // frames from t0 on get a zero gradient
  for (size_t i = (size_t)t0 * CTC_K + lane; i < (size_t)p.T * CTC_K; i += 64) g[i] = 0.f;
  if (r.status != 0 || r.Tb == 0) return;
  const int S = 2 * r.L + 1;
  const int nch = (S + 63) >> 6;
  fill_ext(p, b, r.L, ext);
  const float* x = p.logits + (size_t)b * p.T * CTC_K;
  const double* alpha = p.alpha + (size_t)b * p.T * p.S_ws;
  // log p from the final alpha row, in double (the float loss would put its own rounding into every posterior)
  const double* last = alpha + (size_t)(r.Tb - 1) * p.S_ws;
  const double logp = S >= 2 ? lse2(last[S - 1], last[S - 2]) : last[S - 1];
  float nxt[CTC_K];
  load_frame(x + (size_t)(r.Tb - 1) * CTC_K, nxt);
  for (int t = r.Tb - 1; t >= 0; --t) {
    const Frame f = log_softmax5(nxt);
    const float y0 = (float)exp(f.lp0), y1 = (float)exp(f.lp1), y2 = (float)exp(f.lp2), y3 = (float)exp(f.lp3), y4 = (float)exp(f.lp4);
    if (t >= 1) load_frame(x + (size_t)(t - 1) * CTC_K, nxt);
    const double* arow = alpha + (size_t)t * p.S_ws;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f, c4 = 0.f;
    __syncthreads();
    put_frame(f, lpb);
    for (int j = 0; j < nch; ++j) {
      const int s = lane + 64 * j;
      if (s < S) {
        const int cls = ext[s] & 7;
        const double l = lpb[cls];
        double v;
        if (t == r.Tb - 1) {
          v = s >= S - 2 ? l : -INFINITY;
        } else {
          const double b0 = buf[s];
          const double b1 = s + 1 < S ? buf[s + 1] : -INFINITY;
          const double b2 = (s + 2 < S && (ext[s + 2] & 8)) ? buf[s + 2] : -INFINITY;
          v = lse3(b0, b1, b2) + l;
        }
        buf[s] = v;
        const float post = (float)exp(arow[s] + v - l - logp);
        c0 += cls == 0 ? post : 0.f;
        c1 += cls == 1 ? post : 0.f;
        c2 += cls == 2 ? post : 0.f;
        c3 += cls == 3 ? post : 0.f;
        c4 += cls == 4 ? post : 0.f;
      }
    }
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    c2 = wave_sum(c2);
    c3 = wave_sum(c3);
    c4 = wave_sum(c4);
    // the posteriors of a frame sum to 1: dividing by their computed sum removes what is left of a common shift
    const float tot = c0 + c1 + c2 + c3 + c4;
    const float inv = tot > 0.f ? 1.f / tot : 0.f;
    if (lane < CTC_K) {
      const float y = lane == 0 ? y0 : lane == 1 ? y1 : lane == 2 ? y2 : lane == 3 ? y3 : y4;
      const float c = lane == 0 ? c0 : lane == 1 ? c1 : lane == 2 ? c2 : lane == 3 ? c3 : c4;
      g[(size_t)t * CTC_K + lane] = y - c * inv;
    }
  }
}

__device__ int64_t lower_bound_row(const int64_t* indices, int64_t nnz, int64_t row) {
  int64_t lo = 0, hi = nnz;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (indices[2 * mid] < row) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(64) void edit_kernel(const EditParams p) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= p.B) return;
  const int64_t nnz = p.meta[0];
  const int64_t lo = lower_bound_row(p.indices, nnz, b);
  const int64_t hi = lower_bound_row(p.indices, nnz, (int64_t)b + 1);
  const int64_t n = hi - lo;
  const int m = p.label_len[b];
  if (m <= 0) {
    p.edit[b] = n == 0 ? 0.f : INFINITY;
    return;
  }
  const int W = (m + 63) >> 6;
  uint64_t* ws = p.ws + (size_t)b * 6 * p.words;
  uint64_t* Pv = ws;
  uint64_t* Mv = ws + p.words;
  uint64_t* Peq = ws + 2 * p.words;   // [4][words]
  for (int w = 0; w < W; ++w) {
    Pv[w] = ~0ull;
    Mv[w] = 0ull;
    for (int c = 0; c < 4; ++c) Peq[c * p.words + w] = 0ull;
  }
  const int32_t* lab = p.labels + (size_t)b * p.Lmax;
  for (int i = 0; i < m; ++i) {
    const int c = lab[i];
    if (c >= 0 && c < 4) Peq[c * p.words + (i >> 6)] |= 1ull << (i & 63);
  }
  const uint64_t last_high = 1ull << ((m - 1) & 63);
  int64_t score = m;
  for (int64_t j = lo; j < hi; ++j) {
    const int64_t c = p.values[j];
    int h = 1;   // top row D[0][j] = j: every column enters with +1
    for (int w = 0; w < W; ++w) {
      const uint64_t eq = (c >= 0 && c < 4) ? Peq[c * p.words + w] : 0ull;
      uint64_t pv = Pv[w], mv = Mv[w];
      h = advance_block(pv, mv, eq, h, w == W - 1 ? last_high : (1ull << 63));
      Pv[w] = pv;
      Mv[w] = mv;
    }
    score += h;
  }
  p.edit[b] = (float)score / (float)m;
}

}  // namespace

// LDS of the recursions: the state row (S doubles), the frame's log-softmax (8 doubles), the extended label (S bytes)
size_t ctc_lds_bytes(int S_lds) { return ((size_t)S_lds + 8) * sizeof(double) + (((size_t)S_lds + 7) & ~(size_t)7); }

int launch_ctc(const CtcParams& p, bool want_grad, hipStream_t stream) {
  if (p.B <= 0) return 0;
  const size_t lds = ctc_lds_bytes(p.S_lds);
  if (lds > 160 * 1024) return 1;
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_alpha_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_beta_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return 1;
  }
  hipLaunchKernelGGL(ctc_alpha_kernel, dim3(p.B), dim3(64), lds, stream, p);
  if (want_grad) hipLaunchKernelGGL(ctc_beta_kernel, dim3(p.B), dim3(64), lds, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

void launch_edit(const EditParams& p, hipStream_t stream) {
  if (p.B <= 0) return;
  hipLaunchKernelGGL(edit_kernel, dim3((p.B + 63) / 64), dim3(64), 0, stream, p);
}

// host-side checks shared by chiron_ctc_loss and chiron_engine_score: label values, lengths, seq_len
chiron_status ctc_check_rows(const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int batch, int T, int Lmax) {
  for (int b = 0; b < batch; ++b) {
    if (seq_len && (seq_len[b] < 0 || seq_len[b] > T))
      return set_error(CHIRON_ERR_INVALID, "ctc: seq_len[%d] = %d outside 0..T = %d", b, seq_len[b], T);
    const int L = label_len[b];
    if (L < 0 || L > Lmax) return set_error(CHIRON_ERR_INVALID, "ctc: label_len[%d] = %d outside 0..max_label_len = %d", b, L, Lmax);
    for (int i = 0; i < L; ++i) {
      const int c = labels[(size_t)b * Lmax + i];
      if (c < 0 || c > 3) return set_error(CHIRON_ERR_INVALID, "ctc: label[%d][%d] = %d outside 0..3 (A,C,G,T)", b, i, c);
    }
  }
  return CHIRON_OK;
}

// sizes of the CTC workspace; CHIRON_ERR_OVERFLOW past what the kernels address
chiron_status ctc_sizes(int64_t batch, int64_t T, int64_t Lmax, uint32_t flags, int* S_ws, size_t* bytes) {
  if (batch < 0 || T < 0 || Lmax < 0) return set_error(CHIRON_ERR_INVALID, "ctc: negative batch / T / max_label_len");
  if (T > CHIRON_CTC_MAX_T) return set_error(CHIRON_ERR_OVERFLOW, "ctc: T = %lld frames, the kernels take at most %d", (long long)T, CHIRON_CTC_MAX_T);
  if (Lmax > CHIRON_CTC_MAX_LABEL) return set_error(CHIRON_ERR_OVERFLOW, "ctc: max_label_len %lld past %d", (long long)Lmax, CHIRON_CTC_MAX_LABEL);
  const int64_t S = 2 * (Lmax < T ? Lmax : T) + 1;
  *S_ws = (int)S;
  if (!(flags & CHIRON_CTC_WANT_GRAD)) {
    *bytes = 0;
    return CHIRON_OK;
  }
  // batch * T * S * 8 within int64 (every offset the kernels form is 64-bit)
  const unsigned __int128 n = (unsigned __int128)batch * (unsigned __int128)T * (unsigned __int128)S * 8u;
  if (n > (unsigned __int128)INT64_MAX)
    return set_error(CHIRON_ERR_OVERFLOW, "ctc: workspace of %lld x %lld x %lld floats past 64-bit addressing", (long long)batch, (long long)T, (long long)S);
  *bytes = (size_t)n;
  return CHIRON_OK;
}

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_ctc_workspace_size(int32_t batch, int32_t T, int32_t max_label_len, uint32_t flags, size_t* bytes) {
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_workspace_size: null bytes");
  int S = 0;
  return ctc_sizes(batch, T, max_label_len, flags, &S, bytes);
}

// the int32 operands of chiron_ctc_loss, read back for the checks (device memory), or read in place (host memory)
static chiron_status read_ints(const int32_t* p, size_t n, hipStream_t stream, std::vector<int32_t>& out, bool* on_device) {
  out.resize(n);
  *on_device = false;
  if (n == 0) return CHIRON_OK;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeDevice) {
    *on_device = true;
    if (hipMemcpyAsync(out.data(), p, n * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
      return set_error(CHIRON_ERR_DEVICE, "chiron_ctc_loss: reading the int32 operands back failed");
    return CHIRON_OK;
  }
  (void)hipGetLastError();
  memcpy(out.data(), p, n * 4);
  return CHIRON_OK;
}

extern "C" chiron_status chiron_ctc_loss(int32_t device_id, const float* logits, const int32_t* seq_len, const int32_t* labels,
                                         const int32_t* label_len, int32_t batch, int32_t T, int32_t max_label_len, uint32_t flags,
                                         float* loss_out, float* grad_out, void* workspace, void* stream_) {
  if (batch < 0) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_loss: batch %d", batch);
  if (T < 1 || max_label_len < 0) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_loss: T %d, max_label_len %d", T, max_label_len);
  if (flags & ~(CHIRON_CTC_WANT_GRAD | CHIRON_CTC_TRUSTED)) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_loss: unknown flags 0x%x", flags);
  const bool grad = (flags & CHIRON_CTC_WANT_GRAD) != 0;
  int S_ws = 0;
  size_t ws_bytes = 0;
  chiron_status st = ctc_sizes(batch, T, max_label_len, flags, &S_ws, &ws_bytes);
  if (st) return st;
  if (batch == 0) return CHIRON_OK;
  if (!logits || !seq_len || !labels || !label_len || !loss_out) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_loss: null operand");
  if (grad && (!grad_out || !workspace)) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_loss: CHIRON_CTC_WANT_GRAD needs grad_out and workspace");
  hipStream_t stream = (hipStream_t)stream_;
  int ndev = 0;
  const bool have_gpu = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && device_id >= 0 && device_id < ndev;
  if (have_gpu && hipSetDevice(device_id) != hipSuccess) return set_error(CHIRON_ERR_DEVICE, "hipSetDevice(%d) failed", device_id);
  (void)hipGetLastError();
  bool d_seq = false, d_len = false, d_lab = false;
  if (flags & CHIRON_CTC_TRUSTED) {   // no read-back, no synchronisation: the kernels clamp what they index with
    d_seq = on_device(seq_len);
    d_len = on_device(label_len);
    d_lab = max_label_len == 0 || on_device(labels);
  } else {
    std::vector<int32_t> h_seq, h_len, h_lab;
    if ((st = read_ints(seq_len, (size_t)batch, stream, h_seq, &d_seq))) return st;
    if ((st = read_ints(label_len, (size_t)batch, stream, h_len, &d_len))) return st;
    if ((st = read_ints(labels, (size_t)batch * max_label_len, stream, h_lab, &d_lab))) return st;
    if ((st = ctc_check_rows(h_seq.data(), h_lab.data(), h_len.data(), batch, T, max_label_len))) return st;
  }
  if (!have_gpu) return set_error(CHIRON_ERR_DEVICE, "no HIP device %d: libchiron_amd has no CPU fallback", device_id);
  if (!(d_seq && d_len && (d_lab || max_label_len == 0) && on_device(logits) && on_device(loss_out) &&
        (!grad || (on_device(grad_out) && on_device(workspace)))))
    return set_error(CHIRON_ERR_INVALID, "chiron_ctc_loss: every operand must be device memory on device %d", device_id);
  CtcParams p;
  p.logits = logits;
  p.seq_len = seq_len;
  p.labels = labels;
  p.label_len = label_len;
  p.B = batch;
  p.T = T;
  p.Lmax = max_label_len;
  p.S_ws = S_ws;
  p.S_lds = S_ws;
  p.loss = loss_out;
  p.grad = grad ? grad_out : nullptr;
  p.alpha = grad ? (double*)workspace : nullptr;
  p.status = nullptr;
  if (launch_ctc(p, grad, stream) != 0) return set_error(CHIRON_ERR_DEVICE, "chiron_ctc_loss: launch failed");
  return CHIRON_OK;
}
