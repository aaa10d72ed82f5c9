// CTC forced alignment on gfx950: the best monotone assignment of a read's frames to the bases it is known to have.
//
//   v_t(s) = best(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2)) + x_t[class(s)]   over the S = 2L+1 states of the extended label,
//
// max-plus, in doubles, with a traceback: the semantics, the tie order and the band rule are stated in include/chiron_amd.h and
// restated in numpy by tests/ctc_align_ref.py, which the kernel equals bit for bit.
//
// Work mapping: one workgroup per read.  A pass of half-width w keeps two recursion rows of doubles, used ping-pong and indexed by
// s - lo(t), lo(t) = max(0, c(t) - w): in LDS while the band has at most the launch's lds_slots states, in the workgroup's
// workspace rows beyond that.  One barrier per frame.  A thread owns four consecutive states: it loads the six predecessors they
// share once, and the four 2-bit back-pointers make one byte, so the stores of a wave coalesce.  The frame's five scores and the
// band's bases are staged in LDS a chunk of CHUNK frames ahead (loaded into registers at the start of a chunk, stored before its
// last barrier), which keeps global loads off the frame-to-frame chain.  The traceback is sequential: one lane walks the
// back-pointers from the last frame, checks the edge rule and writes start_out.  A rejected pass doubles w and the read is redone
// inside the kernel, so a batch is one launch.  No atomics: a read's result does not depend on what else is in the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/chiron_amd.h"
#include "align_common.h"
#include "kernels.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_LABEL_THREADS;
constexpr int CHUNK = 32;                    // frames whose scores and bases are staged in LDS at a time
constexpr int BLANK = 4;
constexpr int LAB_REGS = (CHIRON_LABEL_LDS_SLOTS / 2 + 2 * CHUNK + 8 + NT - 1) / NT;   // bases a thread carries to the next chunk's window
constexpr int STATUS_INTERNAL = 3;           // a guard of the kernel fired: reported as CHIRON_ERR_STATE, never returned to the caller

// bases a chunk can need: the band's own (lds_slots / 2) plus what c(t) moves in CHUNK frames.  A feasible read has F >= L, so
// c(t) advances by at most 4 states per frame (L >= 2: 2L / (L-1) <= 4) and a chunk moves it by at most 4 (CHUNK - 1) + 1: the
// window is (lds_slots + 4 CHUNK) / 2 + 4 bases at most.
__host__ __device__ inline int lab_cap(int lds_slots) { return lds_slots / 2 + 2 * CHUNK + 8; }

struct Band {
  int64_t num, den;   // c(t) = floor(t * num / den), num = S - 1, den = max(F - 1, 1)
  int S, w;
  bool full;
  __device__ int c(int t) const { return (int)((int64_t)t * num / den); }
  __device__ int lo(int c) const { return full ? 0 : (c - w > 0 ? c - w : 0); }
  __device__ int hi(int c) const { return full ? S - 1 : (c + w < S - 1 ? c + w : S - 1); }
};

__device__ inline double ninf() { return -INFINITY; }
__device__ inline int imax_(int a, int b) { return a > b ? a : b; }
__device__ inline int imin_(int a, int b) { return a < b ? a : b; }

// One band pass.  Returns through *res (LDS): res[0] = 1 accepted / 0 rejected / -1 guard fired; the score goes to *score_out.
// LDSLAB: the bases come from the staged LDS window (bands that fit LDS); otherwise straight from global memory.
template <bool LDSLAB>
__device__ void band_pass(const LabelParams& p, const LabelRead& rd, const Band& B, double* row0, double* row1, float* sbuf, uint8_t* lbuf,
                          int lcap, uint8_t* bp, int rowbytes, int* res, double* score_out) {
  const int tid = threadIdx.x;
  const int F = rd.F, L = rd.L, S = B.S;
  const float* x = p.scores + rd.frame0 * 5;
  const uint8_t* lab = p.labels + rd.label0;
  const int64_t qn = B.num / B.den, rn = B.num % B.den;

  // stage chunk 0
  int jbase = 0;
  {
    const int t1 = F < CHUNK ? F : CHUNK;
    if (tid < t1 * 5) sbuf[tid] = x[tid];
    if (LDSLAB) {
      const int jend = imin_(L - 1, (B.hi(B.c(t1 - 1)) >> 1) + 1);   // + 1: the base after the band's last state is loaded too
      if (jend + 1 > lcap) {
        if (tid == 0) res[0] = -1;
        __syncthreads();
        return;
      }
      for (int j = tid; j <= jend; j += NT) lbuf[j] = lab[j];
    }
  }
  __syncthreads();
  // frame 0: v_0(0) = x_0[blank], v_0(1) = x_0[l_0]; every other state of the band is -inf
  {
    const int h0 = B.hi(0);
    for (int s = tid; s <= h0; s += NT) row0[s] = s == 0 ? (double)sbuf[BLANK] : s == 1 ? (double)sbuf[LDSLAB ? lbuf[0] : lab[0]] : ninf();
  }
  __syncthreads();

  double* prow = row0;
  double* crow = row1;
  int64_t cq = 0, cr = 0;          // c(t-1) and its remainder, advanced one frame at a time
  int plo = 0, phi = B.hi(0);
  for (int t0 = 0; t0 < F; t0 += CHUNK) {
    const int t1 = imin_(t0 + CHUNK, F);
    const int cb = (t0 / CHUNK) & 1;
    const float* sc = sbuf + cb * CHUNK * 5;
    const uint8_t* lc = lbuf + cb * lcap;
    // the next chunk's scores and bases: loaded now, stored before this chunk's last barrier
    float nsc = 0.f;
    uint8_t nlab[LAB_REGS];
    int njbase = 0, njcnt = 0;
    const int t2 = imin_(t1 + CHUNK, F);
    if (t1 < F) {
      if (tid < (t2 - t1) * 5) nsc = x[(int64_t)t1 * 5 + tid];
      if (LDSLAB) {
        njbase = imax_(0, (B.lo(B.c(t1)) >> 1) - 1);
        njcnt = imin_(L - 1, (B.hi(B.c(t2 - 1)) >> 1) + 1) - njbase + 1;
        if (njcnt > lcap || njcnt > LAB_REGS * NT) {   // cannot happen for a feasible read (lab_cap); never write past the window
          if (tid == 0) res[0] = -1;
          __syncthreads();
          return;
        }
#pragma unroll
        for (int k = 0; k < LAB_REGS; ++k) {
          const int j = tid + k * NT;
          nlab[k] = j < njcnt ? lab[njbase + j] : 0;
        }
      }
    }
    for (int t = t0 > 0 ? t0 : 1; t < t1; ++t) {
      cq += qn;
      cr += rn;
      if (cr >= B.den) {
        cr -= B.den;
        ++cq;
      }
      const int ct = (int)cq;
      const int lo = B.lo(ct), hi = B.hi(ct);
      const float* xt = sc + (t - t0) * 5;
      const float xb = xt[BLANK];
      uint8_t* bprow = bp + (int64_t)t * rowbytes;
      for (int g = tid; 4 * g <= hi - lo; g += NT) {
        const int s0 = lo + 4 * g;
        double pv[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const int sp = s0 - 2 + k;
          pv[k] = (sp >= plo && sp <= phi) ? prow[sp - plo] : ninf();
        }
        // the bases under these four states: j0 - 1 (for the repeat rule), j0, j0 + 1
        const int j0 = s0 >> 1;
        int lm = 4, l0 = 4, l1 = 4;
        if (LDSLAB) {
          if (j0 >= 1 && j0 - 1 < L) lm = lc[j0 - 1 - jbase];
          if (j0 < L) l0 = lc[j0 - jbase];
          if (j0 + 1 < L) l1 = lc[j0 + 1 - jbase];
        } else {
          if (j0 >= 1 && j0 - 1 < L) lm = lab[j0 - 1];
          if (j0 < L) l0 = lab[j0];
          if (j0 + 1 < L) l1 = lab[j0 + 1];
        }
        unsigned byte = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int s = s0 + i;
          if (s <= hi) {
            double best = pv[i + 2];
            unsigned m = 0;
            if (pv[i + 1] > best) {
              best = pv[i + 1];
              m = 1;
            }
            float xs = xb;
            if (s & 1) {
              const int j = s >> 1;
              const int cl = j == j0 ? l0 : l1;
              const int pr = j == j0 ? lm : l0;
              xs = xt[cl];
              if (j >= 1 && pr != cl && pv[i] > best) {
                best = pv[i];
                m = 2;
              }
            }
            crow[s - lo] = best + (double)xs;
            byte |= m << (2 * i);
          }
        }
        bprow[g] = (uint8_t)byte;
      }
      if (t == t1 - 1 && t1 < F) {
        float* ns = sbuf + (cb ^ 1) * CHUNK * 5;
        if (tid < (t2 - t1) * 5) ns[tid] = nsc;
        if (LDSLAB) {
          uint8_t* nl = lbuf + (cb ^ 1) * lcap;
#pragma unroll
          for (int k = 0; k < LAB_REGS; ++k) {
            const int j = tid + k * NT;
            if (j < njcnt) nl[j] = nlab[k];
          }
        }
      }
      __syncthreads();
      double* sw = prow;
      prow = crow;
      crow = sw;
      plo = lo;
      phi = hi;
    }
    jbase = njbase;
  }
  // prow holds frame F-1, indexed by s - plo.  The end: state S-1, or S-2 when strictly better.
  if (tid == 0) {
    const double vlast = (S - 1 >= plo && S - 1 <= phi) ? prow[S - 1 - plo] : ninf();
    const double vprev = (S >= 2 && S - 2 >= plo && S - 2 <= phi) ? prow[S - 2 - plo] : ninf();
    int s = S - 1;
    double best = vlast;
    if (vprev > best) {
      best = vprev;
      s = S - 2;
    }
    int ok = best > ninf() ? 1 : 0;
    if (ok) {
      int32_t* start = p.start + rd.label0;
      int64_t q = B.c(F - 1), r = (int64_t)(F - 1) * B.num % B.den;
      for (int t = F - 1; t >= 0; --t) {
        const int ct = (int)q;
        const int lo = B.lo(ct), hi = B.hi(ct);
        if (s < lo || s > hi) {   // a path never leaves the band: its cells are finite and everything outside is -inf
          ok = -1;
          break;
        }
        if (!B.full && ((s == ct - B.w && s > 0) || (s == ct + B.w && s < S - 1))) ok = 0;   // on a clipped edge: rejected, but finish the walk
        unsigned m = 0;
        if (t > 0) m = (bp[(int64_t)t * rowbytes + ((s - lo) >> 2)] >> (2 * ((s - lo) & 3))) & 3;
        if ((s & 1) && (m != 0 || t == 0)) start[s >> 1] = t;
        s -= (int)m;
        q -= qn;
        r -= rn;
        if (r < 0) {
          r += B.den;
          --q;
        }
      }
      if (ok >= 0 && s != 0 && s != 1) ok = -1;
    }
    *score_out = best;
    res[0] = ok;
  }
  __syncthreads();
}

__device__ int block_sum(int v, int* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int k = NT / 2; k > 0; k >>= 1) {
    if (tid < k) red[tid] += red[tid + k];
    __syncthreads();
  }
  const int out = red[0];
  __syncthreads();
  return out;
}

__global__ __launch_bounds__(CHIRON_LABEL_THREADS) void ctc_align_kernel(LabelParams p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int lcap = lab_cap(p.lds_slots);
  double* const lrow0 = lds;
  double* const lrow1 = lds + p.lds_slots;
  double* const score_s = lds + 2 * p.lds_slots;
  int* const red = reinterpret_cast<int*>(score_s + 1);             // NT ints, res after them
  int* const res = red + NT;
  float* const sbuf = reinterpret_cast<float*>(res + 2);            // 2 x CHUNK x 5
  uint8_t* const lbuf = reinterpret_cast<uint8_t*>(sbuf + 2 * CHUNK * 5);   // 2 x lcap
  double* const ws0 = p.rows ? p.rows + (int64_t)blockIdx.x * 2 * p.row_slots : nullptr;

  for (int64_t q = blockIdx.x; q < p.reads; q += gridDim.x) {
    const LabelRead rd = p.read[q];
    const int F = rd.F, L = rd.L, S = 2 * L + 1;
    const uint8_t* lab = p.labels + rd.label0;
    int rep = 0;
    for (int i = tid + 1; i < L; i += NT) rep += lab[i] == lab[i - 1];
    rep = block_sum(rep, red);
    int status = 0, band = p.band0;
    double score = 0.0;
    if ((int64_t)F < (int64_t)L + rep) {
      status = 1;
    } else if (F > 0) {   // F == 0 is L == 0 here: the empty path, score 0
      Band B;
      B.S = S;
      B.num = S - 1;
      B.den = F > 1 ? F - 1 : 1;
      int w = p.band0;
      for (;;) {
        B.w = w;
        B.full = p.band0 == 0 || w >= S - 1;
        const int width = B.full ? S : (2 * (int64_t)w + 1 < S ? 2 * w + 1 : S);
        const int rowbytes = (width + 3) >> 2;
        int r;
        if (rowbytes > rd.bp_rowbytes) {          // the host sized the back-pointers for the widest band this read can reach
          r = -1;
        } else if (width <= p.lds_slots) {
          band_pass<true>(p, rd, B, lrow0, lrow1, sbuf, lbuf, lcap, p.bp + rd.bp, rowbytes, res, score_s);
          r = res[0];
        } else if (ws0 && width <= p.row_slots) {
          band_pass<false>(p, rd, B, ws0, ws0 + p.row_slots, sbuf, lbuf, lcap, p.bp + rd.bp, rowbytes, res, score_s);
          r = res[0];
        } else {
          r = -1;
        }
        score = *score_s;
        __syncthreads();   // res and score_s are read by everyone before the next pass writes them
        if (r < 0) {
          status = STATUS_INTERNAL;
          break;
        }
        band = w;
        if (r == 1 || B.full) break;
        const int64_t next = 2 * (int64_t)w;
        if (p.max_band > 0 && next > p.max_band && next < S - 1) {
          status = 2;
          break;
        }
        w = (int)next;   // w < S - 1 <= 2^23
      }
    }
    if (status != 0) {
      for (int j = tid; j < L; j += NT) p.start[rd.label0 + j] = -1;
      score = ninf();
    }
    if (tid == 0) {
      p.score[q] = score;
      p.band[q] = band;
      p.status[q] = status;
    }
  }
}

size_t lds_bytes(int lds_slots) {
  return (size_t)(2 * lds_slots + 1) * sizeof(double) + (NT + 2) * sizeof(int) + 2 * CHUNK * 5 * sizeof(float) + 2 * (size_t)lab_cap(lds_slots) + 8;
}

// the widest band (in states) the read can reach under band0 / max_band: the width of the last pass the doubling can arrive at
int64_t widest_band(int64_t L, int32_t band0, int32_t max_band) {
  const int64_t S = 2 * L + 1;
  if (band0 == 0) return S;
  int64_t w = band0;
  for (;;) {
    if (w >= S - 1) return S;
    const int64_t next = 2 * w;
    if (max_band > 0 && next > max_band && next < S - 1) return 2 * w + 1 < S ? 2 * w + 1 : S;
    w = next;
  }
}

}  // namespace

// Validates the offsets and lays the workspace out.  frame_off / label_off: host arrays of reads + 1 entries.
chiron_status label_layout(int64_t reads, const int64_t* frame_off, const int64_t* label_off, int32_t band0, int32_t max_band, LabelLayout* l,
                           std::vector<LabelRead>* recs) {
  memset(l, 0, sizeof(*l));
  if (reads < 0) return set_error(CHIRON_ERR_INVALID, "ctc_align: reads %lld", (long long)reads);
  if (band0 < 0 || max_band < 0) return set_error(CHIRON_ERR_INVALID, "ctc_align: band0 %d / max_band %d is negative", band0, max_band);
  if (max_band > 0 && max_band < band0) return set_error(CHIRON_ERR_INVALID, "ctc_align: max_band %d below band0 %d", max_band, band0);
  if (reads == 0) return CHIRON_OK;
  if (reads > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "ctc_align: %lld reads in one call, at most 2^24", (long long)reads);
  if (!frame_off || !label_off) return set_error(CHIRON_ERR_INVALID, "ctc_align: null offsets");
  if (frame_off[0] < 0 || label_off[0] < 0) return set_error(CHIRON_ERR_INVALID, "ctc_align: a negative first offset");
  const int64_t limit = (int64_t)1 << 46;   // bytes of back-pointers in one call: keeps every sum below far from 2^63
  int64_t bp = 0, widest_lds = 1, row_slots = 0;
  if (recs) recs->resize((size_t)reads);
  for (int64_t r = 0; r < reads; ++r) {
    if (frame_off[r + 1] < frame_off[r] || label_off[r + 1] < label_off[r])
      return set_error(CHIRON_ERR_INVALID, "ctc_align: offsets of read %lld decrease", (long long)r);
    const int64_t F = frame_off[r + 1] - frame_off[r], L = label_off[r + 1] - label_off[r];
    if (F > CHIRON_LABEL_MAX_FRAMES)
      return set_error(CHIRON_ERR_OVERFLOW, "ctc_align: read %lld has %lld frames, at most %d", (long long)r, (long long)F, CHIRON_LABEL_MAX_FRAMES);
    if (L > CHIRON_LABEL_MAX_BASES)
      return set_error(CHIRON_ERR_OVERFLOW, "ctc_align: read %lld has %lld bases, at most %d", (long long)r, (long long)L, CHIRON_LABEL_MAX_BASES);
    const int64_t width = widest_band(L, band0, max_band);
    const int64_t rowbytes = (width + 3) >> 2;
    if (width <= CHIRON_LABEL_LDS_SLOTS) {
      if (width > widest_lds) widest_lds = width;
    } else {
      widest_lds = CHIRON_LABEL_LDS_SLOTS;
      if (width > row_slots) row_slots = width;
    }
    if (recs) {
      LabelRead& rec = (*recs)[(size_t)r];
      rec.frame0 = frame_off[r] - frame_off[0];
      rec.label0 = label_off[r] - label_off[0];
      rec.bp = bp;
      rec.F = (int32_t)F;
      rec.L = (int32_t)L;
      rec.bp_rowbytes = (int32_t)rowbytes;
    }
    bp += F * rowbytes;
    if (bp > limit) return set_error(CHIRON_ERR_OVERFLOW, "ctc_align: the back-pointers of the call pass 2^46 bytes: split the batch");
  }
  const int64_t frames = frame_off[reads] - frame_off[0], bases = label_off[reads] - label_off[0];
  l->groups = (int)(reads < CHIRON_LABEL_MAX_GROUPS ? reads : CHIRON_LABEL_MAX_GROUPS);
  l->lds_slots = (int)((widest_lds + 3) & ~(int64_t)3);
  l->row_slots = (row_slots + 3) & ~(int64_t)3;
  l->frames = frames;
  l->bases = bases;
  l->read = 0;
  l->scores = l->read + up256((size_t)reads * sizeof(LabelRead));
  l->labels = l->scores + up256((size_t)frames * 5 * sizeof(float));
  l->start = l->labels + up256((size_t)bases);
  l->score = l->start + up256((size_t)bases * sizeof(int32_t));
  l->band = l->score + up256((size_t)reads * sizeof(double));
  l->status = l->band + up256((size_t)reads * sizeof(int32_t));
  l->rows = l->status + up256((size_t)reads * sizeof(int32_t));
  l->bp = l->rows + up256((size_t)l->groups * 2 * (size_t)l->row_slots * sizeof(double));
  l->bytes = l->bp + up256((size_t)bp);
  return CHIRON_OK;
}

int launch_ctc_align(const LabelParams& p, int groups, hipStream_t stream) {
  if (p.reads <= 0) return 0;
  const size_t lds = lds_bytes(p.lds_slots);
  if (lds > 160 * 1024) return 1;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return 1;
  hipLaunchKernelGGL(ctc_align_kernel, dim3(groups), dim3(CHIRON_LABEL_THREADS), lds, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_ctc_align_workspace_size(int64_t reads, const int64_t* frame_off, const int64_t* label_off, int32_t band0,
                                                         int32_t max_band, size_t* bytes) {
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_align_workspace_size: null bytes");
  LabelLayout l;
  chiron_status st = label_layout(reads, frame_off, label_off, band0, max_band, &l, nullptr);
  if (st) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_ctc_align(int32_t device_id, const float* scores, const int64_t* frame_off, const uint8_t* labels,
                                          const int64_t* label_off, int64_t reads, int32_t band0, int32_t max_band, uint32_t flags,
                                          int32_t* start_out, double* score_out, int32_t* band_out, int32_t* status_out, void* workspace,
                                          void* stream_) {
  if (flags) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_align: unknown flags 0x%x", flags);
  LabelLayout l;
  std::vector<LabelRead> recs;
  chiron_status st = label_layout(reads, frame_off, label_off, band0, max_band, &l, &recs);
  if (st) return st;
  if (reads == 0) return CHIRON_OK;
  if (!score_out || !band_out || !status_out) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_align: null output");
  if (l.frames > 0 && !scores) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_align: null scores");
  if (l.bases > 0 && (!labels || !start_out)) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_align: null labels / start_out");
  const float* x = scores + frame_off[0] * 5;
  for (int64_t i = 0; i < l.frames * 5; ++i)
    if (!std::isfinite(x[i]))
      return set_error(CHIRON_ERR_INVALID, "chiron_ctc_align: score %lld of frame %lld is not finite", (long long)(i % 5), (long long)(frame_off[0] + i / 5));
  const uint8_t* lab = labels + label_off[0];
  for (int64_t i = 0; i < l.bases; ++i)
    if (lab[i] > 3) return set_error(CHIRON_ERR_INVALID, "chiron_ctc_align: code %d at base %lld outside 0..3", (int)lab[i], (long long)(label_off[0] + i));
  if ((st = use_device_workspace("chiron_ctc_align", device_id, workspace))) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  if (hipMemcpyAsync(ws + l.read, recs.data(), recs.size() * sizeof(LabelRead), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (l.frames > 0 && hipMemcpyAsync(ws + l.scores, x, (size_t)l.frames * 5 * sizeof(float), hipMemcpyHostToDevice, stream) != hipSuccess) ||
      (l.bases > 0 && hipMemcpyAsync(ws + l.labels, lab, (size_t)l.bases, hipMemcpyHostToDevice, stream) != hipSuccess))
    return set_error(CHIRON_ERR_DEVICE, "chiron_ctc_align: copying the reads to the device failed");
  LabelParams p;
  p.scores = (const float*)(ws + l.scores);
  p.labels = (const uint8_t*)(ws + l.labels);
  p.read = (const LabelRead*)(ws + l.read);
  p.reads = reads;
  p.bp = (uint8_t*)(ws + l.bp);
  p.rows = l.row_slots ? (double*)(ws + l.rows) : nullptr;
  p.row_slots = l.row_slots;
  p.lds_slots = l.lds_slots;
  p.band0 = band0;
  p.max_band = max_band;
  p.start = (int32_t*)(ws + l.start);
  p.score = (double*)(ws + l.score);
  p.band = (int32_t*)(ws + l.band);
  p.status = (int32_t*)(ws + l.status);
  if (launch_ctc_align(p, l.groups, stream) != 0) return set_error(CHIRON_ERR_DEVICE, "chiron_ctc_align: launch failed");
  if ((l.bases > 0 && hipMemcpyAsync(start_out + label_off[0], ws + l.start, (size_t)l.bases * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      hipMemcpyAsync(score_out, ws + l.score, (size_t)reads * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(band_out, ws + l.band, (size_t)reads * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(status_out, ws + l.status, (size_t)reads * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "chiron_ctc_align: the alignment kernel failed (%s)", hipGetErrorString(hipGetLastError()));
  for (int64_t r = 0; r < reads; ++r)
    if (status_out[r] == STATUS_INTERNAL) return set_error(CHIRON_ERR_STATE, "chiron_ctc_align: read %lld outgrew its workspace", (long long)r);
  return CHIRON_OK;
}
