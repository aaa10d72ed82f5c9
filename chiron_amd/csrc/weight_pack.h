// Weight preparation: from the weight blob (model_layout.h) to the byte layouts the kernels read, and the scalar geometry of every
// plan the engine launches from.  pack_weights fills the plans' scalars, leaves their device pointers null and returns one Upload per
// pointer: the bytes and the address of the pointer they belong to.  engine.hip allocates, copies and stores the pointers;
// tests/native/weight_pack_digest.cpp runs the same packer on the CPU.  Host only: no HIP runtime call.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "kernels.h"
#include "model_layout.h"

namespace chiron {

inline int roundup(int v, int m) { return (v + m - 1) / m * m; }

struct ConvGemmPlan {
  // device weights for one fused GEMM
  float* Wt = nullptr;
  float* shift = nullptr;
  float* descale = nullptr;   // dtype fp32-split: 2^-s[n] of the power-of-two row scaling (GemmParams::descale)
  void* w_bf3 = nullptr;      // fp32 LSTM projections: Wt as three bf16 planes (bf16x3_planes below; engine.hip builds them after pack_weights)
  int N = 0, Npad = 0, K = 0;
};

// f16 engine, calibration (chiron_engine_calibrate): what a plan's weights lost when they were rounded to halves.
// y[n] = sum_k x[k] f16(W[n][k]) = sum_k x[k] W[n][k] + sum_k x[k] dW[n][k]; the second sum's MEAN over the data, sum_k E[x_k] dW[n][k],
// is a constant per output channel and is taken out of the plan's shift once the input channels' means are known.
struct PlanHost {
  std::vector<float> dW;       // [Npad][K]: (float)(_Float16)W - W of the BN-folded fp32 weight (0 in the K / N padding)
  std::vector<float> shift0;   // the uncorrected shift
  int N = 0, Npad = 0, K = 0;
};

struct BlockPlan {
  bool lift = false;
  int c_in = 0, c = 0, k = 0, stride = 1, left = 0;
  int t_in = 0, t_out = 0;
  float *lift_a = nullptr, *lift_b = nullptr;  // lift: conv2a folded scale/shift
  float *res_a = nullptr, *res_b = nullptr;    // lift: branch1 folded scale and its own folded shift (kernels.h res_b)
  // lift, population BN: conv2a + conv2b as a piecewise-linear table of the signal value (pwl.hip)
  float *pwl_bp = nullptr, *pwl_ref = nullptr, *pwl_tab = nullptr, *pwl_shift = nullptr;
  int pwl_nbp = 0;
  ConvGemmPlan ga, gb, gc;                     // conv2a (non-lift), conv2b, conv2c(+conv1)
  float* wino_u = nullptr;                     // conv2b in Winograd form (wino.hip): transformed filters [4 or 6][C][C], or null
  int wino_f4 = 0;                             // 1: F(4,3) (six filters, length % 4 == 0), 0: F(2,3)
  // bn_mode = batch (cnn.py:166-188): the GEMM weights above are raw, gc holds conv2c alone, g1 the 1x1 branch1 conv;
  // scale / offset of the four BN sites (conv1 only when i_bn)
  ConvGemmPlan g1;
  bool i_bn = false;
  float *bn_scale[4] = {nullptr, nullptr, nullptr, nullptr}, *bn_offset[4] = {nullptr, nullptr, nullptr, nullptr};  // conv1, 2a, 2b, 2c
};

struct LstmPlan {
  int in_w = 0;
  ConvGemmPlan proj[2];  // STACK / layer 0: proj[0] covers both directions; MULTI l>0: one per dir
  int nproj = 1;
  float* wfrag = nullptr;
  void* wwide = nullptr;    // f16: recurrent weights in the 16x16x16 B-operand order of lstm16w_kernel
  void* whfused = nullptr;  // f16: W_hh in the 16x16x32 order of lstm16f_kernel
  void* wxwide = nullptr;   // f16: input weights in that order (lstm16f_kernel: projection fused into the recurrence)
  int wx_ksteps = 0;        //      its k-steps of 16 (16: K = 256, 13: K = 200)
  void* wsplit = nullptr;   // fp32-split: W_hh as hi + lo half pairs in the order of wwide (lstm32s_kernel)
  float* wwide32 = nullptr; // fp32: recurrent weights in the 16x16x4 B-operand order of lstm32w_kernel
  float* wlight = nullptr;  // K-split fragment of units 96..99 for the paired recurrence (fp32, H = 100)
};

// Everything the launch sequence reads that comes from the descriptor and the blob (chiron_engine is one of these)
struct NetPlans {
  int T = 0, C = 0;   // frames and channels the CNN hands to the recurrent layers
  // stem (HEAD RNA_model2 / RNA_model3): folded filter [k][C], shift [C]; batch-BN mode: raw filter + scale / offset
  int stem_k = 0, stem_stride = 1, stem_left = 0, stem_t = 0, stem_c = 0;
  float *stem_w = nullptr, *stem_shift = nullptr, *stem_scale = nullptr, *stem_offset = nullptr;
  std::vector<BlockPlan> blocks;
  std::vector<LstmPlan> lstm;
  float *fc_w = nullptr, *fc_b = nullptr, *fc_wc = nullptr, *fc_bc = nullptr;
};

// The environment switches that change what is packed; engine.hip reads them (build_plans)
struct PackSwitches {
  bool no_winograd = false;      // CHIRON_NO_WINOGRAD
  bool wino_f2 = false;          // CHIRON_WINOGRAD_F2
  bool wino_f4 = false;          // CHIRON_WINOGRAD_F4
  bool no_pwl = false;           // CHIRON_NO_PWL
  bool split_rec32 = false;      // CHIRON_SPLIT_REC32
  bool split_row_scale = true;   // off: CHIRON_SPLIT_NO_ROW_SCALE
};

struct Upload {
  void** dst;                         // the plan pointer these bytes are for, inside the NetPlans being packed
  std::shared_ptr<void> owner;        // the host vector the packer filled
  const void* data;                   // its elements
  size_t bytes;
  PlanHost host;                      // the shift of an f16 GEMM (host.Npad > 0): what calibration keeps under the device pointer
};

// ---- the layouts, each said once ----

// An exact float as two halves: v = hi + lo up to lo's own rounding (fp32-split and fp16-w2 GEMM rows, wsplit)
struct HalfPair {
  _Float16 hi, lo;
};
inline HalfPair split_half(float v) {
  const _Float16 hi = (_Float16)v;
  return {hi, (_Float16)(v - (float)hi)};
}

// An exact float as three bf16 values: w = hi + mid + lo, each part the next 8 significand bits, cut off (never rounded: FLT_MAX stays
// finite).  Every part is the fp32 number whose upper 16 bits are stored; the subtractions are exact.  The sum is w itself unless lo
// falls below fp32's subnormal spacing of bf16 (2^-133), which loses at most that much.
struct Bf16x3 {
  uint16_t hi, mid, lo;
};
inline uint32_t f32_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}
inline float bits_f32(uint32_t u) {
  float v;
  memcpy(&v, &u, 4);
  return v;
}
inline Bf16x3 split_bf16x3(float w) {
  const uint32_t hb = f32_bits(w) & 0xffff0000u;
  const float r = w - bits_f32(hb);
  const uint32_t mb = f32_bits(r) & 0xffff0000u;
  const float l = r - bits_f32(mb);
  return {(uint16_t)(hb >> 16), (uint16_t)(mb >> 16), (uint16_t)(f32_bits(l) >> 16)};
}

// The projection weights of gemm_proj_bf16x3_kernel (gemm.hip): per 160-column tile and 16-k stage one 15 KB image that the LDS-DMA
// copies as it lies, [plane hi / mid / lo][k half kh][160 columns][8 bf16].  The eight values of (stage c, kh) are
// k = 16 c + 8 (e >> 2) + 4 kh + (e & 3), e = 0 .. 7: the two 16-byte slots of the fp32 activation row that a lane of half kh splits
// into the A operand of one v_mfma_f32_32x32x16_bf16.
inline int bf16x3_stages(int cin) { return (cin + BF3_BK - 1) / BF3_BK; }
// index (in bf16 elements) of plane `plane` of weight (column n, channel k) in an array of `stages` stages per tile
inline size_t bf16x3_index(int plane, int n, int k, int stages) {
  const int tile = n / BF3_BN, col = n % BF3_BN, c = k / BF3_BK, kk = k % BF3_BK;
  const int kh = (kk >> 2) & 1, e = ((kk >> 3) << 2) | (kk & 3);
  return ((size_t)(tile * stages + c) * (BF3_STAGE_BYTES / 2)) + (size_t)(((plane * 2 + kh) * BF3_BN + col) * 8 + e);
}
// Wt [N][ld] fp32 (k contiguous, the packed fp32 projection weight), N a multiple of 160; channels >= cin are zero in every plane
inline std::vector<uint16_t> bf16x3_planes(const float* Wt, int N, int ld, int cin) {
  const int stages = bf16x3_stages(cin);
  std::vector<uint16_t> v((size_t)(N / BF3_BN) * stages * (BF3_STAGE_BYTES / 2), (uint16_t)0);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < cin; ++k) {
      const Bf16x3 s = split_bf16x3(Wt[(size_t)n * ld + k]);
      v[bf16x3_index(0, n, k, stages)] = s.hi;
      v[bf16x3_index(1, n, k, stages)] = s.mid;
      v[bf16x3_index(2, n, k, stages)] = s.lo;
    }
  return v;
}

// folded BN (cnn.py:125-163 population branch; association order of the .meta graph):
//   inv = rsqrt(var + 1e-5) * scale ; y = x*inv + (offset - mean*inv)
struct BnFold {
  std::vector<float> inv, sh;
};
inline BnFold fold_bn(const float* scale, const float* offset, const float* mean, const float* var, int n) {
  BnFold f;
  f.inv.resize(n);
  f.sh.resize(n);
  for (int i = 0; i < n; ++i) {
    const float inv = (1.0f / sqrtf(var[i] + 1e-5f)) * scale[i];
    f.inv[i] = inv;
    f.sh[i] = offset[i] - mean[i] * inv;
  }
  return f;
}

// A filter W [taps][ci][co] transposed into columns k0 .. of the GEMM weight Wt [Npad][K], each tap `cop` columns wide, folded with
// its BN: Wt[n][k0 + tap*cop + c] = W[tap][c][n] * inv[n] (inv = nullptr: raw, for batch statistics).  sh, where given, goes into the
// GEMM's shift: the first filter of a row sets it, one fused behind it along K (k0 > 0) adds its own.
inline void fold_filter(std::vector<float>& Wt, std::vector<float>& shift, int K, int k0, const float* W, int taps, int ci, int co, int cop,
                        const float* inv, const float* sh) {
  for (int n = 0; n < co; ++n) {
    for (int tap = 0; tap < taps; ++tap)
      for (int c = 0; c < ci; ++c) {
        const float v = W[((size_t)tap * ci + c) * co + n];
        Wt[(size_t)n * K + k0 + tap * cop + c] = inv ? v * inv[n] : v;
      }
    if (sh) shift[n] = k0 == 0 ? sh[n] : shift[n] + sh[n];
  }
}

// The TF kernels of one LSTM layer, kern[dir] [in_w + H][4H]; z column n of a direction: gate = n / H, unit = n % H
struct LstmKernels {
  const float* kern[2];
  int H;
  // kern[dir][k_off + k][g * H + unit], 0 outside the width x H matrix that starts at row k_off
  float at(int dir, int k_off, int width, int k, int g, int unit) const {
    return k < width && unit < H ? kern[dir][(size_t)(k_off + k) * 4 * H + g * H + unit] : 0.f;
  }
};

// MFMA B-operand fragments of the rows [k_off, k_off + width) of the kernels; put(index, weight) stores one element.
// Narrow (4-row kernels): [dir][wave LSTM_NW][k-step][lane][V], lane = gate*16 + (unit & 15), unit = 16 wave + (lane & 15), k = V ks + q.
// V = 1: lstm_kernel (fp32, LSTM_K steps); V = 4: v_mfma_f32_4x4x4_16B_f16 (LSTM_KSTEPS16 steps).
template <class Put>
inline void narrow_fragments(const LstmKernels& kn, int V, int ksteps, int k_off, int width, Put put) {
  for (int dir = 0; dir < 2; ++dir)
    for (int wv = 0; wv < LSTM_NW; ++wv)
      for (int ks = 0; ks < ksteps; ++ks)
        for (int lane = 0; lane < 64; ++lane)
          for (int q = 0; q < V; ++q) {
            const int k = V * ks + q, g = lane >> 4, unit = 16 * wv + (lane & 15);
            put(((((size_t)dir * LSTM_NW + wv) * ksteps + ks) * 64 + lane) * V + q, kn.at(dir, k_off, width, k, g, unit));
          }
}
inline size_t narrow_elems(int V, int ksteps) { return (size_t)2 * LSTM_NW * ksteps * 64 * V; }

// Wide (16-row kernels, H = 100): [dir][wave 8][slot 4][k-step][lane][V], lane = kg*16 + 4u + gate, unit = 4 (3 wave + slot) + u,
// k = V (4 ks + kg) + q; waves 0..6 own three slots, wave 7 four (the fourth slot of the others stays zero).
// V = 1: lstm32w_kernel (25 steps); V = 4: lstm16w_kernel / lstm32s_kernel (7); V = 8: lstm16f_kernel (v_mfma_f32_16x16x32_f16).
template <class Put>
inline void wide_fragments(const LstmKernels& kn, int V, int ksteps, int k_off, int width, Put put) {
  for (int dir = 0; dir < 2; ++dir)
    for (int wv = 0; wv < 8; ++wv)
      for (int slot = 0; slot < (wv == 7 ? 4 : 3); ++slot)
        for (int ks = 0; ks < ksteps; ++ks)
          for (int lane = 0; lane < 64; ++lane)
            for (int q = 0; q < V; ++q) {
              const int k = V * (4 * ks + (lane >> 4)) + q, g = lane & 3, unit = 4 * (3 * wv + slot) + ((lane >> 2) & 3);
              put((((((size_t)dir * 8 + wv) * 4 + slot) * ksteps + ks) * 64 + lane) * V + q, kn.at(dir, k_off, width, k, g, unit));
            }
}
inline size_t wide_elems(int V, int ksteps) { return (size_t)2 * 8 * 4 * ksteps * 64 * V; }

// light-wave fragment of lstm_pair_kernel: [dir][m = 4q + a][lane = kg*16 + gate*4 + j] = W_hh[16q + 4kg + a][gate*H + 96 + j]
inline std::vector<float> light_fragment(const LstmKernels& kn, int k_off) {
  std::vector<float> wl((size_t)2 * 28 * 64, 0.f);
  for (int dir = 0; dir < 2; ++dir)
    for (int m = 0; m < 28; ++m)
      for (int lane = 0; lane < 64; ++lane) {
        const int q = m >> 2, a = m & 3, kg = lane >> 4, g = (lane >> 2) & 3, j = lane & 3;
        const int k = 16 * q + 4 * kg + a;
        wl[((size_t)dir * 28 + m) * 64 + lane] = kn.at(dir, k_off, kn.H, k, g, 96 + j);
      }
  return wl;
}

// ---- the packer ----
struct WeightPacker {
  const chiron_model_desc& d;
  const BlobMap& map;
  const float* w;
  const PackSwitches sw;
  const bool f16, w2, split, batch;   // f16 covers fp16-w2, as chiron_engine::f16 does
  const int kq;                       // K padding quantum in elements: one LDS chunk = 128 bytes per row (32 floats / 64 halves)
  NetPlans* out;
  std::vector<Upload>* ups;

  template <class P, class Tp>
  Upload& put(P** dst, std::vector<Tp>&& h) {   // takes the vector over: nothing is copied
    auto v = std::make_shared<std::vector<Tp>>(std::move(h));
    ups->push_back(Upload{reinterpret_cast<void**>(dst), v, v->data(), v->size() * sizeof(Tp), PlanHost()});
    return ups->back();
  }

  // One GEMM's weight [Npad][K] and shift [Npad] in the engine's dtype
  void gemm(ConvGemmPlan* g, std::vector<float>&& Wt, std::vector<float>&& shift, int N, int Npad, int K) {
    g->N = N;
    g->Npad = Npad;
    g->K = K;
    if (split) {
      // per 32-element block of a row: 32 hi halves then 32 lo halves (K is a multiple of 32).  Row n is scaled by 2^s[n] so that its
      // largest weight lies in [2^12, 2^13): hi <= 8192 is far from a half's 65504, and lo = O(2^-11 w) is a NORMAL half for every
      // weight down to 2^-15 of the row's largest (GemmParams::descale).  CHIRON_SPLIT_NO_ROW_SCALE=1: the unscaled format of round 5 (A/B).
      std::vector<_Float16> h(2 * Wt.size());
      std::vector<float> sh2(std::move(shift)), ds((size_t)Npad + 192, 1.0f);
      for (int n = 0; n < Npad; ++n) {
        float mx = 0.f;
        for (int k = 0; k < K; ++k) mx = std::max(mx, fabsf(Wt[(size_t)n * K + k]));
        int s = 0;
        if (sw.split_row_scale && mx > 0.f && std::isfinite(mx)) {
          int ex;
          frexpf(mx, &ex);                       // mx = f * 2^ex, 0.5 <= f < 1
          s = std::min(60, std::max(-60, 13 - ex));
          if (n < (int)sh2.size() && !std::isfinite(ldexpf(sh2[n], s))) s = 0;
        }
        ds[n] = ldexpf(1.0f, -s);
        if (n < (int)sh2.size()) sh2[n] = ldexpf(sh2[n], s);
        for (int k = 0; k < K; ++k) {
          const size_t i = (size_t)n * K + k;
          const HalfPair p = split_half(ldexpf(Wt[i], s));
          const size_t blk = i / 32, el = i % 32;
          h[blk * 64 + el] = p.hi;
          h[blk * 64 + 32 + el] = p.lo;
        }
      }
      put(&g->Wt, std::move(h));
      put(&g->descale, std::move(ds));
      put(&g->shift, std::move(sh2));
    } else if (w2) {
      // every row [K hi halves | K lo halves]: launch() runs the K-segments of a GEMM twice, the second time against the lo columns
      std::vector<_Float16> h(2 * Wt.size());
      for (int n = 0; n < Npad; ++n)
        for (int k = 0; k < K; ++k) {
          const HalfPair p = split_half(Wt[(size_t)n * K + k]);
          h[(size_t)n * 2 * K + k] = p.hi;
          h[(size_t)n * 2 * K + K + k] = p.lo;
        }
      put(&g->Wt, std::move(h));
      put(&g->shift, std::move(shift));
    } else if (f16) {
      std::vector<_Float16> h(Wt.size());
      for (size_t i = 0; i < Wt.size(); ++i) h[i] = (_Float16)Wt[i];
      PlanHost ph;
      ph.dW.resize(Wt.size());
      for (size_t i = 0; i < Wt.size(); ++i) ph.dW[i] = (float)h[i] - Wt[i];
      ph.shift0 = shift;
      ph.N = N, ph.Npad = Npad, ph.K = K;
      put(&g->Wt, std::move(h));
      put(&g->shift, std::move(shift)).host = std::move(ph);
    } else {
      put(&g->Wt, std::move(Wt));
      put(&g->shift, std::move(shift));
    }
  }
  // the common case: one filter is the whole GEMM
  void gemm_of_filter(ConvGemmPlan* g, const float* W, int taps, int ci, int co, int cop, const float* inv, const float* sh) {
    const int Npad = roundup(co, GEMM_BN), K = taps * cop;
    std::vector<float> Wt((size_t)Npad * K, 0.f), shift(Npad, 0.f);
    fold_filter(Wt, shift, K, 0, W, taps, ci, co, cop, inv, sh);
    gemm(g, std::move(Wt), std::move(shift), co, Npad, K);
  }

  // Stem and residual blocks: BN folded into (population) or kept beside (batch) the weights, in the layouts the convolution kernels read
  void stem_and_blocks(int segment_len) {
    SiteFrames fr[MAX_SITES];
    out->T = frames(map, segment_len, fr);
    out->C = d.blocks[d.n_blocks - 1].out_channels;
    if (map.has_stem) {
      const ConvSite& s = map.site[0];
      const int k = s.k, co = s.co;
      const float *Ws = w + s.w_off, *bn = w + s.bn_off;  // [k][1][co]
      std::vector<float> wf((size_t)k * co), sh(co, 0.f);
      if (batch) {
        std::vector<float> sc(bn, bn + co), of(bn + co, bn + 2 * co);
        for (size_t i = 0; i < wf.size(); ++i) wf[i] = Ws[i];
        put(&out->stem_scale, std::move(sc));
        put(&out->stem_offset, std::move(of));
      } else {
        const BnFold f = fold_bn(bn, bn + co, bn + 2 * co, bn + 3 * co, co);
        for (int tap = 0; tap < k; ++tap)
          for (int c = 0; c < co; ++c) wf[(size_t)tap * co + c] = Ws[(size_t)tap * co + c] * f.inv[c];
        sh = f.sh;
      }
      put(&out->stem_w, std::move(wf));
      put(&out->stem_shift, std::move(sh));
      out->stem_k = k;
      out->stem_stride = s.stride;
      out->stem_c = co;
      out->stem_t = fr[0].tout;
      out->stem_left = fr[0].pad;
    }
    out->blocks.reserve(d.n_blocks);   // the uploads hold addresses inside the plans
    for (int bi = 0; bi < d.n_blocks; ++bi) {
      const chiron_res_block& b = d.blocks[bi];
      const ConvSite* site = map.site + map.has_stem + 4 * bi;   // site[SITE_BRANCH1 .. SITE_CONV2C]
      const SiteFrames& f2 = fr[map.has_stem + 4 * bi + SITE_CONV2B];
      out->blocks.emplace_back();
      BlockPlan& bp = out->blocks.back();
      bp.lift = b.in_channels == 1;
      bp.c_in = b.in_channels;
      bp.c = b.out_channels;
      bp.k = b.k;
      bp.stride = b.stride;
      bp.t_in = f2.tin;
      bp.t_out = f2.tout;
      bp.left = f2.pad;
      const int t = bp.t_in;
      const int ci = b.in_channels, co = b.out_channels;
      bp.i_bn = b.i_bn != 0;
      // one BN site: population statistics fold into the weights; batch statistics leave the weights raw and keep
      // scale / offset for bn_batch.hip; a site without BN (branch1 unless i_bn) folds to 1 / 0
      auto bn_site = [&](int which, bool has_bn) {
        const float* bn = w + site[which].bn_off;
        if (has_bn && !batch) return fold_bn(bn, bn + co, bn + 2 * co, bn + 3 * co, co);
        if (has_bn) {
          put(&bp.bn_scale[which], std::vector<float>(bn, bn + co));
          put(&bp.bn_offset[which], std::vector<float>(bn + co, bn + 2 * co));
        }
        return BnFold{std::vector<float>(co, 1.0f), std::vector<float>(co, 0.0f)};
      };
      const float *W1 = w + site[SITE_BRANCH1].w_off, *W2a = w + site[SITE_CONV2A].w_off, *W2b = w + site[SITE_CONV2B].w_off,
                  *W2c = w + site[SITE_CONV2C].w_off;
      const BnFold f1 = bn_site(SITE_BRANCH1, bp.i_bn), f2a = bn_site(SITE_CONV2A, true), f2b = bn_site(SITE_CONV2B, true),
                   f2c = bn_site(SITE_CONV2C, true);

      const int Npad = roundup(co, GEMM_BN);
      const int cop = roundup(co, kq);
      gemm_of_filter(&bp.gb, W2b, b.k, co, co, cop, f2b.inv.data(), f2b.sh.data());
      // 1 x 3, stride 1 over C = co channels, fp32, population BN, even length: Winograd F(2,3) (wino.hip) -- four
      // products per output pair instead of six.  U_j[n][c] in float64 from the folded taps g_tap = W2b[tap][c][n]*inv[n].
      if (!bp.lift && !batch && !f16 && !split && b.k == 3 && b.stride == 1 && (t % 2) == 0 && co % 64 == 0 && ci == co && !sw.no_winograd) {
        // F(4,3) from 256 frames per window on (round 6): its rounding error is correlated over the four frames of a quad and, measured
        // against the float32 ensembles of tests/golden/parity_dist, costs the short strided topology more than it saves -- RNA_default
        // (T = 100): typical window 1.32 .. 1.45 -> 1.13 .. 1.20 x the ensemble's median, tail 7 .. 9 % -> 2 .. 5 % with F(2,3), for 0.04 ms
        // of its 1.7 ms batch; DNA_default (T = 400): parity within the noise of F(2,3)'s, F(4,3) worth 4.1 % of the headline.
        // CHIRON_WINOGRAD_F4=1 / CHIRON_WINOGRAD_F2=1 force either form.
        const bool f4 = (t % 4) == 0 && !sw.wino_f2 && (t >= 256 || sw.wino_f4);
        const int nu = f4 ? 6 : 4;
        // F(4,3): U = G g;  F(2,3): g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2
        static const double G4[6][3] = {{0.25, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                        {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
        static const double G2[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
        std::vector<float> U((size_t)nu * co * co);
        for (int n = 0; n < co; ++n)
          for (int c = 0; c < co; ++c) {
            double gt[3];
            for (int tap = 0; tap < 3; ++tap) gt[tap] = (double)W2b[((size_t)tap * co + c) * co + n] * f2b.inv[n];
            for (int j = 0; j < nu; ++j) {
              const double* gj = f4 ? G4[j] : G2[j];
              U[((size_t)j * co + n) * co + c] = (float)(gj[0] * gt[0] + gj[1] * gt[1] + gj[2] * gt[2]);
            }
          }
        bp.wino_f4 = f4 ? 1 : 0;
        put(&bp.wino_u, std::move(U));
      }
      if (bp.lift) {
        std::vector<float> la(cop, 0.f), lb(cop, 0.f), ra(Npad, 0.f), rb(Npad, 0.f);
        for (int c = 0; c < co; ++c) {
          la[c] = W2a[c] * f2a.inv[c];
          lb[c] = f2a.sh[c];
          ra[c] = W1[c] * f1.inv[c];
          rb[c] = f16 ? 0.f : f1.sh[c];   // the f16 engines keep round 4's arithmetic (shift folded): halves' rounding dominates there
        }
        if (!batch && !sw.no_pwl && pwl_covers(co, b.k, b.stride)) {
          // f[tap][n](s) = sum_c W2b'[tap][c][n] * relu(s*a[c] + b[c]) is piecewise linear in the signal value s:
          // tabulate (alpha, beta) per interval between consecutive breakpoints -b[c]/a[c] (pwl.hip).  float64 sums.
          std::vector<std::pair<double, int>> brk;  // (breakpoint, channel)
          for (int c = 0; c < co; ++c)
            if (la[c] != 0.f) brk.emplace_back(-(double)lb[c] / (double)la[c], c);
          std::sort(brk.begin(), brk.end());
          const int nb = (int)brk.size(), kk = b.k;
          std::vector<double> al((size_t)kk * co, 0.0), be((size_t)kk * co, 0.0);
          auto toggle = [&](int c, double sign) {
            for (int tap = 0; tap < kk; ++tap)
              for (int n = 0; n < co; ++n) {
                const double wv = (double)(W2b[((size_t)tap * co + c) * co + n] * f2b.inv[n]) * sign;
                al[(size_t)tap * co + n] += wv * (double)la[c];
                be[(size_t)tap * co + n] += wv * (double)lb[c];
              }
          };
          // s -> -inf: a channel is active iff a < 0, or a == 0 and b > 0
          for (int c = 0; c < co; ++c)
            if (la[c] < 0.f || (la[c] == 0.f && lb[c] > 0.f)) toggle(c, 1.0);
          std::vector<float> tab((size_t)(nb + 1) * kk * co * 2), bpf(std::max(nb, 1), 0.f), reff(nb + 1, 0.f);
          for (int iv = 0; iv < nb; ++iv) bpf[iv] = (float)brk[iv].first;   // may round to +-inf: such a breakpoint is simply never crossed
          for (int iv = 0; iv <= nb; ++iv) {
            if (iv > 0) {
              const int c = brk[iv - 1].second;
              toggle(c, la[c] > 0.f ? 1.0 : -1.0);  // crossing its breakpoint upwards switches a channel on (a > 0) or off (a < 0)
            }
            // The table stores the slope and the value at a reference point of the interval, f = alpha*(s - ref) + f(ref).
            // ref = the point of the interval nearest to 0 (0 itself when the interval contains it): |s - ref| <= |s| for
            // every s the interval can receive, so a breakpoint far outside the signal range (a near-dead channel: tiny
            // folded scale, breakpoint at -1e6 or beyond float range) never makes alpha*(s - ref) cancel against f(ref).
            const double lower = iv > 0 ? (double)bpf[iv - 1] : -(double)INFINITY, upper = iv < nb ? (double)bpf[iv] : (double)INFINITY;
            double ref = std::min(std::max(0.0, lower), upper);
            ref = std::min(std::max(ref, -(double)FLT_MAX), (double)FLT_MAX);
            reff[iv] = (float)ref;
            for (size_t i = 0; i < (size_t)kk * co; ++i) {
              tab[((size_t)iv * kk * co + i) * 2] = (float)al[i];
              tab[((size_t)iv * kk * co + i) * 2 + 1] = (float)(al[i] * (double)reff[iv] + be[i]);
            }
          }
          bp.pwl_nbp = nb;
          put(&bp.pwl_bp, std::move(bpf));
          put(&bp.pwl_ref, std::move(reff));
          put(&bp.pwl_tab, std::move(tab));
          put(&bp.pwl_shift, std::vector<float>(f2b.sh.begin(), f2b.sh.begin() + co));
        }
        put(&bp.res_b, std::move(rb));
        put(&bp.lift_a, std::move(la));
        put(&bp.lift_b, std::move(lb));
        put(&bp.res_a, std::move(ra));
        // conv2c; the signal branch (scale res_a, shift res_b) is evaluated by the epilogue as one fmaf and added to the finished sum
        // (batch-statistics BN: both fold to 1 / 0 here and the branch is normalised by bn_batch.hip)
        std::vector<float> shc(f2c.sh);
        if (f16)
          for (int n = 0; n < co; ++n) shc[n] = f2c.sh[n] + f1.sh[n];
        gemm_of_filter(&bp.gc, W2c, 1, co, co, cop, f2c.inv.data(), shc.data());
      } else {
        const int cip = roundup(ci, kq);
        gemm_of_filter(&bp.ga, W2a, 1, ci, co, cip, f2a.inv.data(), f2a.sh.data());
        if (batch) {
          // separate GEMMs: each branch is normalised with its own batch statistics before the add
          gemm_of_filter(&bp.gc, W2c, 1, co, co, cop, nullptr, nullptr);
          gemm_of_filter(&bp.g1, W1, 1, ci, co, cip, nullptr, nullptr);
        } else {
          // conv2c and branch1/conv1 fused along K: [conv2b output | block input]
          const int K = cop + cip;
          std::vector<float> Wt((size_t)Npad * K, 0.f), sh(Npad, 0.f);
          fold_filter(Wt, sh, K, 0, W2c, 1, co, co, cop, f2c.inv.data(), f2c.sh.data());
          fold_filter(Wt, sh, K, cop, W1, 1, ci, co, cip, f1.inv.data(), f1.sh.data());
          gemm(&bp.gc, std::move(Wt), std::move(sh), co, Npad, K);
        }
      }
    }
  }

  // One LSTM layer from the TF kernels kern[dir] [in_w + H][4H] and biases bias[dir] [4H]: the x-projection GEMMs and W_hh in the
  // operand order of every recurrence kernel the dtype can run
  chiron_status lstm_layer(int l) {
    const int H = d.hidden;
    const int zc = 4 * H;
    const LstmKernels kn{{w + map.lstm_kernel[l][0], w + map.lstm_kernel[l][1]}, H};
    const float* const bias[2] = {w + map.lstm_bias[l][0], w + map.lstm_bias[l][1]};
    out->lstm.emplace_back();
    LstmPlan& lp = out->lstm.back();
    lp.in_w = map.lstm_in[l];
    const int in_w = lp.in_w;   // W_hh is the H rows below W_x's in_w
    const bool per_dir = d.rnn_kind == CHIRON_RNN_MULTI && l > 0;
    lp.nproj = per_dir ? 2 : 1;
    const int Kp = roundup(in_w, kq);
    for (int pj = 0; pj < lp.nproj; ++pj) {
      const int ndir = per_dir ? 1 : 2;
      const int N = ndir * zc;
      const int Npad = std::max(roundup(N, GEMM_BN), roundup(N, 160));  // the DMA kernel reads whole 160-row weight tiles
      std::vector<float> Wt((size_t)Npad * Kp, 0.f), sh(Npad, 0.f);
      for (int n = 0; n < N; ++n) {
        const int dir = per_dir ? pj : n / zc;
        const int nl = n % zc;
        const int g = nl / H, unit = nl % H;
        for (int k = 0; k < in_w; ++k) Wt[(size_t)n * Kp + k] = kn.kern[dir][(size_t)k * 4 * H + g * H + unit];
        // forget_bias = 1.0 (TF LSTMCell default; Add(+1.0) const in the .meta while-body) folded here
        sh[n] = bias[dir][g * H + unit] + (g == 2 ? 1.0f : 0.0f);
      }
      gemm(&lp.proj[pj], std::move(Wt), std::move(sh), N, Npad, Kp);
    }
    auto halves = [&](bool wide, int V, int ksteps, int k_off, int width) {
      std::vector<_Float16> v(wide ? wide_elems(V, ksteps) : narrow_elems(V, ksteps), (_Float16)0.f);
      auto store = [&](size_t at, float x) { v[at] = (_Float16)x; };
      if (wide) wide_fragments(kn, V, ksteps, k_off, width, store);
      else narrow_fragments(kn, V, ksteps, k_off, width, store);
      return v;
    };
    if (f16) {
      put(&lp.wfrag, halves(false, 4, LSTM_KSTEPS16, in_w, H));
      if (H == 100) {
        put(&lp.wwide, halves(true, 4, 7, in_w, H));   // lstm16w_kernel
        if (lp.nproj == 1 && (in_w == 256 || in_w == 200)) {
          // lstm16f_kernel: W_x and W_hh, zero past the width
          lp.wx_ksteps = in_w == 256 ? 8 : 7;
          put(&lp.wxwide, halves(true, 8, lp.wx_ksteps, 0, in_w));
          put(&lp.whfused, halves(true, 8, 4, in_w, H));
        }
      }
    } else {
      std::vector<float> wf(narrow_elems(1, LSTM_K), 0.f);
      narrow_fragments(kn, 1, LSTM_K, in_w, H, [&](size_t at, float x) { wf[at] = x; });
      put(&lp.wfrag, std::move(wf));
    }
    if (w2 && H != 100) return set_error(CHIRON_ERR_INVALID, "dtype f16-w2: the recurrence kernel is built for hidden=100");
    if ((w2 || (split && !sw.split_rec32)) && H == 100) {
      // lstm32s_kernel: [hi | lo] of the fragments of lstm16w_kernel, every weight as an exact hi + lo half pair
      const size_t half = wide_elems(4, 7);
      std::vector<_Float16> ws(2 * half, (_Float16)0.f);
      wide_fragments(kn, 4, 7, in_w, H, [&](size_t at, float x) {
        const HalfPair p = split_half(x);
        ws[at] = p.hi;
        ws[half + at] = p.lo;
      });
      put(&lp.wsplit, std::move(ws));
    }
    if (!f16) {
      put(&lp.wlight, light_fragment(kn, in_w));
      if (H == 100) {
        std::vector<float> ww(wide_elems(1, 25), 0.f);   // lstm32w_kernel
        wide_fragments(kn, 1, 25, in_w, H, [&](size_t at, float x) { ww[at] = x; });
        put(&lp.wwide32, std::move(ww));
      }
    }
    return CHIRON_OK;
  }

  // FC head (raw)
  void head() {
    put(&out->fc_w, std::vector<float>(w + map.head_w, w + map.head_b));
    put(&out->fc_b, std::vector<float>(w + map.head_b, w + map.head_wc));
    put(&out->fc_wc, std::vector<float>(w + map.head_wc, w + map.head_bc));
    put(&out->fc_bc, std::vector<float>(w + map.head_bc, w + map.total));
  }
};

// Packs the blob `w` (map.total floats) of descriptor `d` for an engine of `dtype` on windows of segment_len samples: out's scalars,
// and one Upload per device pointer of out.  out must stay where it is until the uploads have been stored.
inline chiron_status pack_weights(const chiron_model_desc& d, const BlobMap& map, const float* w, int segment_len, int dtype,
                                  const PackSwitches& sw, NetPlans* out, std::vector<Upload>* ups) {
  const bool w2 = dtype == CHIRON_F16_W2, f16 = dtype == CHIRON_F16 || w2, split = dtype == CHIRON_F32_SPLIT;
  const bool batch = d.bn_mode == CHIRON_BN_BATCH;
  if (batch && (f16 || split)) return set_error(CHIRON_ERR_INVALID, "bn_mode=batch is implemented for dtype f32 only");
  if (f16 || split) {
    for (int bi = 0; bi < d.n_blocks; ++bi)
      if (d.blocks[bi].out_channels % GEMM_BN || (d.blocks[bi].in_channels != 1 && d.blocks[bi].in_channels % 64))
        return set_error(CHIRON_ERR_INVALID, "dtype f16: block %d has %d -> %d channels; the f16 kernels need multiples of 64 / 128", bi,
                         d.blocks[bi].in_channels, d.blocks[bi].out_channels);
    // the convolution forms of the DMA GEMM exist for K-segments of 256 channels only in these dtypes (gemm.hip launch_dma): any other
    // width would pack and then find no kernel at the first batch
    for (int bi = 0; bi < d.n_blocks; ++bi)
      if (d.blocks[bi].out_channels != 256 || (d.blocks[bi].in_channels != 1 && d.blocks[bi].in_channels != 256))
        return set_error(CHIRON_ERR_INVALID, "dtype %s: block %d has %d -> %d channels; its convolution kernels are built for 1 -> 256 and 256 -> 256",
                         split ? "f32-split" : "f16", bi, d.blocks[bi].in_channels, d.blocks[bi].out_channels);
    // fp16-w2 runs every K-segment twice (hi and lo weight columns): a conv2b on the GEMM has 2 k segments of the GEMM_MAX_SEG
    for (int bi = 0; bi < d.n_blocks; ++bi) {
      const chiron_res_block& b = d.blocks[bi];
      const bool table = b.in_channels == 1 && !sw.no_pwl && pwl_covers(b.out_channels, b.k, b.stride);   // conv2b without a GEMM
      if (w2 && !table && 2 * b.k > GEMM_MAX_SEG)
        return set_error(CHIRON_ERR_INVALID, "dtype f16-w2: block %d: conv2b width %d unsupported (1..%d: hi and lo weights take two K-segments per tap)",
                         bi, b.k, GEMM_MAX_SEG / 2);
    }
  }
  WeightPacker p{d, map, w, sw, f16, w2, split, batch, f16 ? 2 * GEMM_BK : GEMM_BK, out, ups};
  p.stem_and_blocks(segment_len);
  out->lstm.reserve(d.rnn_layers);
  for (int l = 0; l < d.rnn_layers; ++l) {
    const chiron_status st = p.lstm_layer(l);
    if (st) return st;
  }
  p.head();
  return CHIRON_OK;
}

}  // namespace chiron
