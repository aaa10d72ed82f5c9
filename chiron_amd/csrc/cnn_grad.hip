// Training seam of the CNN (fp32, gfx950): forward with a tape on the batch's own BN moments, and the full backward.
//
// Reference: chiron/cnn.py:15-83 (conv_layer), :125-188 (batchnorm training branch / simple_global_bn), :234-262 (residual_layer),
// :334-371 (getcnnfeature), as chiron_rcnn_train.py:30-136 trains them; semantics of oracle/nn_oracle.py:40-119 with bn_mode "batch".
// The seam's output is the feature tensor [B, T, C] that chiron_rnn_train_forward takes; its backward consumes that call's dfeatures.
//
// Activations are batch-major rows m = b * T_site + t of C floats.  A site is one convolution with its optional BN:
//   tape      Y    [rows][C]   every BN site's convolution output (xhat and the ReLU mask are recomputed from it)
//             R    [rows][C]   every ReLU output: conv2a's, conv2b's, the block's (and the stem's) -- the next site's input
//             stat [4][C]      per BN site: mean, invstd, inv = invstd * scale, shift = offset - mean * inv
//   workspace four activation-sized buffers, per-slice partial sums, per-channel BN-backward sums.  The forward uses the first
//             buffer only (the un-normalised shortcut) and the partial sums; the backward all four (dOut / dY rotation, the masked
//             residual gradient)
//
// Kernels (one form of each):
//   cg_conv_kernel   implicit GEMM over rows on v_mfma_f32_32x32x2_f32, 128 x 128 x 16 tiles, the tap loop inside the K loop:
//                    Y = sum_tap X_tap W_tap (forward) and dX = sum_tap dY_tap W_tap^T (backward); a tap is a row shift inside
//                    the window (rows outside [0, T) read zero), a stride is a row stride (CgRows).
//   cg_dw_kernel     dW_tap = X_tap^T dY on the same tiles, reduction over the rows split into slices, one partial per slice,
//                    cg_reduce_kernel sums them in slice order.
//   cg_rank1_*       convolutions with one input channel: forward on the VALU, weight gradient a row reduction of x * dy.
//   cg_sum_kernel / cg_bn_bwd_sum_kernel   per-channel row reductions (moments; sum dy, sum dy * xhat and sum xhat with the ReLU
//                    mask fused).
//   cg_bn_apply_kernel / cg_bn_bwd_apply_kernel   BN + residual add + ReLU forward; ReLU mask + BN backward.
// Every reduction over rows goes through per-slice partials whose slice count depends on the shape alone and a second pass in
// slice order: no float atomics, the same bits run to run.
#include "kernels.h"
#include "model_layout.h"

#include <cstdio>

namespace chiron {

typedef float cg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int CT = 128, CK = 16, CLD = CT + 4;
constexpr int CG_RED_THREADS = 512;    // threads of a row-reduction workgroup: C / 4 channel lanes x row lanes
constexpr int CG_SLICE_ROWS = 256;     // least rows per slice of a row reduction
constexpr int CG_MAX_SLICES = 512;
constexpr int CG_DW_SPLIT_ROWS = 2048; // reduction rows per slice of cg_dw_kernel
constexpr int CG_DW_MAX_SPLIT = 64;
constexpr int CG_R1_TAPS = 8;          // taps per pass of cg_rank1_dw_kernel
constexpr float CG_BN_EPS = 1e-5f;     // cnn.py:125, :188

// row (b, t) of the logical side and a tap -> row of the source side, or -1: num = t * mul + off0 + offs * tap must be a
// non-negative multiple of div with num / div < Tsrc.  Forward and dW: mul = stride, off0 = -pad, offs = 1, div = 1.
// dX: mul = 1, off0 = pad, offs = -1, div = stride.
struct CgRows {
  int Tl, Tsrc, mul, div, off0, offs;
};

__device__ __forceinline__ long cg_src_row(const CgRows& g, int b, int t, int tap) {
  const int num = t * g.mul + g.off0 + g.offs * tap;
  if (num < 0) return -1;
  const int q = num / g.div;
  if (q * g.div != num || q >= g.Tsrc) return -1;
  return (long)b * g.Tsrc + q;
}

__device__ __forceinline__ void cg_zero(cg_f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
}

// one K = 16 step of the 128 x 128 tile: wave (wm, wn) owns 64 x 64 of it as 2 x 2 MFMA blocks
__device__ __forceinline__ void cg_tile_step(const float (&As)[CK][CLD], const float (&Bs)[CK][CLD], cg_f32x16 (&acc)[2][2], int lane, int wm,
                                             int wn) {
#pragma unroll
  for (int k2 = 0; k2 < CK / 2; ++k2) {
    const int kk = 2 * k2 + (lane >> 5);
    float a[2], b[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) a[m] = As[kk][wm * 64 + m * 32 + (lane & 31)];
#pragma unroll
    for (int n = 0; n < 2; ++n) b[n] = Bs[kk][wn * 64 + n * 32 + (lane & 31)];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[n], acc[m][n], 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------------------------
// C[i][j] (+)= sum_tap sum_r A[src(i, tap)][r] B[tap][r][j]: rows along i
// ---------------------------------------------------------------------------------------------
struct CgConv {
  const float* A; int lda;
  CgRows g;
  int ntaps;
  const float* B; long sbt, sbr, sbj;
  float* C; long ldc;
  int I, J, R;
  int accumulate;
};

__global__ __launch_bounds__(256) void cg_conv_kernel(const CgConv p) {
  __shared__ float As[CK][CLD];
  __shared__ float Bs[CK][CLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * CT, j0 = blockIdx.y * CT;
  const int wm = wave >> 1, wn = wave & 1;
  const bool b_r = p.sbr == 1;
  int rb[8], rt[8];
  bool rv[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int gi = i0 + (tid >> 4) + 16 * q;
    rv[q] = gi < p.I;
    rb[q] = rv[q] ? gi / p.g.Tl : 0;
    rt[q] = rv[q] ? gi - rb[q] * p.g.Tl : 0;
  }
  long src[8];
  int cur_tap = -1;
  const int nR = (p.R + CK - 1) / CK;
  const int nsteps = p.ntaps * nR;
  float ra[8], rbv[8];
  auto load = [&](int ks) {
    const int tap = ks / nR;
    const int r0 = (ks - tap * nR) * CK;
    if (tap != cur_tap) {
      cur_tap = tap;
#pragma unroll
      for (int q = 0; q < 8; ++q) src[q] = rv[q] ? cg_src_row(p.g, rb[q], rt[q], tap) : -1;
    }
    const int gr = r0 + (tid & 15);
    const float* Bt = p.B + (long)tap * p.sbt;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      ra[q] = (src[q] >= 0 && gr < p.R) ? p.A[src[q] * p.lda + gr] : 0.f;
      int jj, r2;
      if (b_r) { r2 = tid & 15; jj = (tid >> 4) + 16 * q; } else { jj = tid & 127; r2 = (tid >> 7) + 2 * q; }
      const int gj = j0 + jj, gr2 = r0 + r2;
      rbv[q] = (gj < p.J && gr2 < p.R) ? Bt[(long)gr2 * p.sbr + (long)gj * p.sbj] : 0.f;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      As[tid & 15][(tid >> 4) + 16 * q] = ra[q];
      if (b_r) Bs[tid & 15][(tid >> 4) + 16 * q] = rbv[q]; else Bs[(tid >> 7) + 2 * q][tid & 127] = rbv[q];
    }
  };
  cg_f32x16 acc[2][2];
  cg_zero(acc);
  if (nsteps > 0) load(0);
  for (int ks = 0; ks < nsteps; ++ks) {
    stash();
    __syncthreads();
    if (ks + 1 < nsteps) load(ks + 1);
    cg_tile_step(As, Bs, acc, lane, wm, wn);
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int gi = i0 + wm * 64 + m * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
        const int gj = j0 + wn * 64 + n * 32 + (lane & 31);
        if (gi < p.I && gj < p.J) {
          float* dst = p.C + (long)gi * p.ldc + gj;
          *dst = p.accumulate ? *dst + acc[m][n][e] : acc[m][n][e];
        }
      }
}

// ---------------------------------------------------------------------------------------------
// part[tap][z][i][j] = sum over the rows r of slice z of X[src(r, tap)][i] dY[r][j]: rows along the reduction
// ---------------------------------------------------------------------------------------------
struct CgDw {
  const float* X; int ldx;
  CgRows g;
  const float* dY; int ldy;
  float* part;
  int I, J, R;      // input channels, output channels, logical rows
  int nsplit, chunk;
};

__global__ __launch_bounds__(256) void cg_dw_kernel(const CgDw p) {
  __shared__ float As[CK][CLD];
  __shared__ float Bs[CK][CLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;
  const int tap = blockIdx.z / p.nsplit, z = blockIdx.z - tap * p.nsplit;
  const int r_begin = z * p.chunk;
  const int r_end = min(p.R, r_begin + p.chunk);
  const int wm = wave >> 1, wn = wave & 1;
  const int gi = i0 + (tid & 127), gj = j0 + (tid & 127);
  int rb[8], rt[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int gr = r_begin + (tid >> 7) + 2 * q;
    rb[q] = gr / p.g.Tl;
    rt[q] = gr - rb[q] * p.g.Tl;
  }
  float ra[8], rbv[8];
  auto load = [&](int r0) {   // called once per r0, in order: (rb, rt) walk along with it
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int gr = r0 + (tid >> 7) + 2 * q;
      const bool live = gr < r_end;
      const long s = live ? cg_src_row(p.g, rb[q], rt[q], tap) : -1;
      ra[q] = (s >= 0 && gi < p.I) ? p.X[s * p.ldx + gi] : 0.f;
      rbv[q] = (live && gj < p.J) ? p.dY[(long)gr * p.ldy + gj] : 0.f;
      rt[q] += CK;
      while (rt[q] >= p.g.Tl) {
        rt[q] -= p.g.Tl;
        ++rb[q];
      }
    }
  };
  cg_f32x16 acc[2][2];
  cg_zero(acc);
  if (r_begin < r_end) load(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += CK) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      As[(tid >> 7) + 2 * q][tid & 127] = ra[q];
      Bs[(tid >> 7) + 2 * q][tid & 127] = rbv[q];
    }
    __syncthreads();
    if (r0 + CK < r_end) load(r0 + CK);
    cg_tile_step(As, Bs, acc, lane, wm, wn);
    __syncthreads();
  }
  float* C = p.part + (long)blockIdx.z * p.I * p.J;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ci = i0 + wm * 64 + m * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
        const int cj = j0 + wn * 64 + n * 32 + (lane & 31);
        if (ci < p.I && cj < p.J) C[(long)ci * p.J + cj] = acc[m][n][e];
      }
}

// out[g * n + e] = sum over the slices z of part[(g * nslices + z) * n + e], in slice order
__global__ __launch_bounds__(256) void cg_reduce_kernel(const float* part, int nslices, long n, long total, float* out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long g = idx / n, e = idx - g * n;
  const float* src = part + g * nslices * n + e;
  float s = src[0];
  for (int z = 1; z < nslices; ++z) s += src[(long)z * n];
  out[idx] = s;
}

// ---------------------------------------------------------------------------------------------
// row reductions: C / 4 channel lanes x row lanes per workgroup, one slice of rows per workgroup
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 cg_add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// the row lanes' sums, added in row-lane order -> out[4 c4 .. 4 c4 + 3]
__device__ __forceinline__ void cg_block_sum(float4 v, float4* sh, int cl, int nrl, float* out) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  if (tid < cl) {
    float4 s = sh[tid];
    for (int r = 1; r < nrl; ++r) s = cg_add4(s, sh[r * cl + tid]);
    reinterpret_cast<float4*>(out)[tid] = s;
  }
  __syncthreads();
}

// part[slice][c] = sum over the slice's rows of y (mean == nullptr) or of (y - mean)^2
__global__ __launch_bounds__(CG_RED_THREADS) void cg_sum_kernel(const float* y, long rows, int C, long chunk, const float* mean, float* part) {
  __shared__ float4 sh[CG_RED_THREADS];
  const int cl = C / 4, nrl = CG_RED_THREADS / cl;
  const int tid = threadIdx.x, c4 = tid % cl, rl = tid / cl;
  const long m0 = (long)blockIdx.x * chunk;
  const long m1 = m0 + chunk < rows ? m0 + chunk : rows;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (rl < nrl) {
    const float4 mu = mean ? reinterpret_cast<const float4*>(mean)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool sq = mean != nullptr;
#pragma unroll 4
    for (long m = m0 + rl; m < m1; m += nrl) {
      float4 v = reinterpret_cast<const float4*>(y + m * C)[c4];
      if (sq) {
        v.x -= mu.x; v.y -= mu.y; v.z -= mu.z; v.w -= mu.w;
        v = make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w);
      }
      s = cg_add4(s, v);
    }
  }
  cg_block_sum(s, sh, cl, nrl, part + (long)blockIdx.x * C);
}

// stat: [4][C] = mean, invstd, inv, shift
__global__ __launch_bounds__(256) void cg_mean_finish_kernel(const float* part, int nslices, int C, float n, float* stat) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = part[c];
  for (int z = 1; z < nslices; ++z) s += part[(long)z * C + c];
  stat[c] = s / n;
}

// bn: the site's four blob slots scale, offset, pop_mean, pop_var; mom: the same slots of moments_out
__global__ __launch_bounds__(256) void cg_var_finish_kernel(const float* part, int nslices, int C, float n, const float* bn, float* stat,
                                                            float* mom) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = part[c];
  for (int z = 1; z < nslices; ++z) s += part[(long)z * C + c];
  const float var = s / n, mean = stat[c];
  const float invstd = 1.0f / sqrtf(var + CG_BN_EPS);
  const float inv = invstd * bn[c];   // tf.nn.batch_normalization: inv = rsqrt(var + eps) * scale; y = x * inv + (offset - mean * inv)
  stat[C + c] = invstd;
  stat[2 * C + c] = inv;
  stat[3 * C + c] = bn[C + c] - mean * inv;
  mom[2 * C + c] = mean;
  mom[3 * C + c] = var;
}

// out = [relu]( y * inv + shift  [+ y2 * inv2 + shift2 | + y2] )
struct CgApply {
  const float* y; const float* stat;
  const float* y2; const float* stat2;   // y2 == nullptr: no second term; stat2 == nullptr: y2 is added as it is
  float* out;
  float* out2;                           // optional second copy (features_out)
  long n4;
  int C, relu;
};

__global__ __launch_bounds__(256) void cg_bn_apply_kernel(const CgApply p) {
  const int cl = p.C / 4;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.n4; idx += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(idx % cl);
    const float4 v = reinterpret_cast<const float4*>(p.y)[idx];
    const float4 a = reinterpret_cast<const float4*>(p.stat + 2 * p.C)[c4], s = reinterpret_cast<const float4*>(p.stat + 3 * p.C)[c4];
    float4 o = make_float4(v.x * a.x + s.x, v.y * a.y + s.y, v.z * a.z + s.z, v.w * a.w + s.w);
    if (p.y2) {
      float4 w = reinterpret_cast<const float4*>(p.y2)[idx];
      if (p.stat2) {
        const float4 a2 = reinterpret_cast<const float4*>(p.stat2 + 2 * p.C)[c4], s2 = reinterpret_cast<const float4*>(p.stat2 + 3 * p.C)[c4];
        w = make_float4(w.x * a2.x + s2.x, w.y * a2.y + s2.y, w.z * a2.z + s2.z, w.w * a2.w + s2.w);
      }
      o = make_float4(w.x + o.x, w.y + o.y, w.z + o.z, w.w + o.w);
    }
    if (p.relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    reinterpret_cast<float4*>(p.out)[idx] = o;
    if (p.out2) reinterpret_cast<float4*>(p.out2)[idx] = o;
  }
}

__device__ __forceinline__ float4 cg_masked(float4 d, float4 r) {
  return make_float4(r.x > 0.f ? d.x : 0.f, r.y > 0.f ? d.y : 0.f, r.z > 0.f ? d.z : 0.f, r.w > 0.f ? d.w : 0.f);
}
__device__ __forceinline__ float4 cg_xhat(float4 y, float4 mu, float4 is) {
  return make_float4((y.x - mu.x) * is.x, (y.y - mu.y) * is.y, (y.z - mu.z) * is.z, (y.w - mu.w) * is.w);
}

// part[slice][0][c] = sum dy, part[slice][1][c] = sum dy * xhat, part[slice][2][c] = sum xhat, dy = din where relu_out > 0
// (relu_out == nullptr: dy = din).  xhat is recomputed with the tape's float32 mean, so it is centred only up to that mean's
// rounding; the backward's formula assumes sum xhat = 0, and where the site's input has a large mean (the raw signal) the residue is
// amplified a hundredfold in dW.  The third sum measures it, and cg_bn_bwd_finish_kernel / cg_bn_bwd_apply_kernel take it out.
__global__ __launch_bounds__(CG_RED_THREADS) void cg_bn_bwd_sum_kernel(const float* din, const float* relu_out, const float* y, const float* stat,
                                                                       long rows, int C, long chunk, float* part) {
  __shared__ float4 sh[CG_RED_THREADS];
  const int cl = C / 4, nrl = CG_RED_THREADS / cl;
  const int tid = threadIdx.x, c4 = tid % cl, rl = tid / cl;
  const long m0 = (long)blockIdx.x * chunk;
  const long m1 = m0 + chunk < rows ? m0 + chunk : rows;
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1, s3 = s1;
  if (rl < nrl) {
    const float4 mu = reinterpret_cast<const float4*>(stat)[c4], is = reinterpret_cast<const float4*>(stat + C)[c4];
#pragma unroll 4
    for (long m = m0 + rl; m < m1; m += nrl) {
      float4 d = reinterpret_cast<const float4*>(din + m * C)[c4];
      if (relu_out) d = cg_masked(d, reinterpret_cast<const float4*>(relu_out + m * C)[c4]);
      const float4 xh = cg_xhat(reinterpret_cast<const float4*>(y + m * C)[c4], mu, is);
      s1 = cg_add4(s1, d);
      s2 = cg_add4(s2, make_float4(d.x * xh.x, d.y * xh.y, d.z * xh.z, d.w * xh.w));
      s3 = cg_add4(s3, xh);
    }
  }
  cg_block_sum(s1, sh, cl, nrl, part + (long)blockIdx.x * 3 * C);
  cg_block_sum(s2, sh, cl, nrl, part + (long)blockIdx.x * 3 * C + C);
  cg_block_sum(s3, sh, cl, nrl, part + (long)blockIdx.x * 3 * C + 2 * C);
}

// sum dy -> d offset; sum dy * (xhat - mean xhat) -> d scale; the statistics' slots get exactly 0.
// sums[0][c] = mean dy, sums[1][c] = mean dy * (xhat - mean xhat), sums[2][c] = mean xhat
__global__ __launch_bounds__(256) void cg_bn_bwd_finish_kernel(const float* part, int nslices, int C, float n, float* sums, float* dbn) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s1 = part[c], s2 = part[C + c], s3 = part[2 * C + c];
  for (int z = 1; z < nslices; ++z) {
    s1 += part[(long)z * 3 * C + c];
    s2 += part[(long)z * 3 * C + C + c];
    s3 += part[(long)z * 3 * C + 2 * C + c];
  }
  const float m3 = s3 / n;
  s2 -= m3 * s1;
  sums[c] = s1 / n;
  sums[C + c] = s2 / n;
  sums[2 * C + c] = m3;
  dbn[c] = s2;
  dbn[C + c] = s1;
  dbn[2 * C + c] = 0.f;
  dbn[3 * C + c] = 0.f;
}

// dy_out = scale * invstd * (dy - mean(dy) - xhat * mean(dy * xhat)), xhat centred by its measured mean; g_out (optional) = dy, the
// masked incoming gradient
struct CgBnBwd {
  const float* din; const float* relu_out; const float* y; const float* stat; const float* scale; const float* sums;
  float* dy_out; float* g_out;
  long n4;
  int C;
};

__global__ __launch_bounds__(256) void cg_bn_bwd_apply_kernel(const CgBnBwd p) {
  const int cl = p.C / 4;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.n4; idx += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(idx % cl);
    float4 d = reinterpret_cast<const float4*>(p.din)[idx];
    if (p.relu_out) d = cg_masked(d, reinterpret_cast<const float4*>(p.relu_out)[idx]);
    const float4 mu = reinterpret_cast<const float4*>(p.stat)[c4], is = reinterpret_cast<const float4*>(p.stat + p.C)[c4];
    float4 xh = cg_xhat(reinterpret_cast<const float4*>(p.y)[idx], mu, is);
    const float4 sc = reinterpret_cast<const float4*>(p.scale)[c4];
    const float4 a = reinterpret_cast<const float4*>(p.sums)[c4], b = reinterpret_cast<const float4*>(p.sums + p.C)[c4];
    const float4 m3 = reinterpret_cast<const float4*>(p.sums + 2 * p.C)[c4];
    xh = make_float4(xh.x - m3.x, xh.y - m3.y, xh.z - m3.z, xh.w - m3.w);
    float4 o;
    o.x = sc.x * is.x * (d.x - a.x - xh.x * b.x);
    o.y = sc.y * is.y * (d.y - a.y - xh.y * b.y);
    o.z = sc.z * is.z * (d.z - a.z - xh.z * b.z);
    o.w = sc.w * is.w * (d.w - a.w - xh.w * b.w);
    if (p.g_out) reinterpret_cast<float4*>(p.g_out)[idx] = d;
    reinterpret_cast<float4*>(p.dy_out)[idx] = o;
  }
}

// ---------------------------------------------------------------------------------------------
// one input channel: y[b, t, c] = sum_tap x[b, t s + tap - pad] w[tap, c]
// ---------------------------------------------------------------------------------------------
struct CgRank1 {
  const float* x;     // [B][Tsrc]
  const float* w;     // [k][C]
  float* y;           // [B * Tl][C]
  const float* dy;    // backward
  float* part;        // backward: [slice][nt][C]
  CgRows g;
  int k, C;
  long rows, chunk;
  int tap0, nt;       // backward: this pass's taps
};

__global__ __launch_bounds__(256) void cg_rank1_fwd_kernel(const CgRank1 p) {
  const int cl = p.C / 4;
  const long n4 = p.rows * cl;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n4; idx += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(idx % cl);
    const long m = idx / cl;
    const int b = (int)(m / p.g.Tl), t = (int)(m - (long)b * p.g.Tl);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int tap = 0; tap < p.k; ++tap) {
      const long s = cg_src_row(p.g, b, t, tap);
      const float xv = s >= 0 ? p.x[s] : 0.f;
      const float4 w = reinterpret_cast<const float4*>(p.w + (long)tap * p.C)[c4];
      acc = make_float4(acc.x + xv * w.x, acc.y + xv * w.y, acc.z + xv * w.z, acc.w + xv * w.w);
    }
    reinterpret_cast<float4*>(p.y)[idx] = acc;
  }
}

__global__ __launch_bounds__(CG_RED_THREADS) void cg_rank1_dw_kernel(const CgRank1 p) {
  __shared__ float4 sh[CG_RED_THREADS];
  const int cl = p.C / 4, nrl = CG_RED_THREADS / cl;
  const int tid = threadIdx.x, c4 = tid % cl, rl = tid / cl;
  const long m0 = (long)blockIdx.x * p.chunk;
  const long m1 = m0 + p.chunk < p.rows ? m0 + p.chunk : p.rows;
  float4 acc[CG_R1_TAPS];
#pragma unroll
  for (int j = 0; j < CG_R1_TAPS; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (rl < nrl) {
    for (long m = m0 + rl; m < m1; m += nrl) {
      const float4 d = reinterpret_cast<const float4*>(p.dy + m * p.C)[c4];
      const int b = (int)(m / p.g.Tl), t = (int)(m - (long)b * p.g.Tl);
#pragma unroll
      for (int j = 0; j < CG_R1_TAPS; ++j) {
        if (j < p.nt) {
          const long s = cg_src_row(p.g, b, t, p.tap0 + j);
          const float xv = s >= 0 ? p.x[s] : 0.f;
          acc[j] = make_float4(acc[j].x + xv * d.x, acc[j].y + xv * d.y, acc[j].z + xv * d.z, acc[j].w + xv * d.w);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CG_R1_TAPS; ++j)
    if (j < p.nt) cg_block_sum(acc[j], sh, cl, nrl, p.part + ((long)blockIdx.x * p.nt + j) * p.C);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct CgSite : ConvSite {    // w_off / bn_off: the CNN section starts the blob, so they index params as they are
  int pad, tin, tout;
  size_t y, r, stat;          // tape offsets (floats): convolution output, ReLU output (relu sites), statistics (bn sites)
  bool y_in_ws;               // the un-normalised shortcut lives in the workspace
  long rows;                  // B * tout
};

struct CgLayout {
  int n_sites, n_blocks, has_stem;
  CgSite s[MAX_SITES];
  int B, L, T, C;
  size_t n_params;
  size_t tape_floats;
  size_t buf[4], part, sums, ws_floats;   // workspace offsets (floats)
};

// the slices of a row reduction: at most CG_MAX_SLICES of `chunk` rows, and no more than hold a row (just past the cap,
// CG_MAX_SLICES slices of the rounded-up chunk would leave the last ones empty)
struct CgSlices { int n; long chunk; };
static CgSlices cg_slices(long rows) {
  long n = (rows + CG_SLICE_ROWS - 1) / CG_SLICE_ROWS;
  n = n < 1 ? 1 : n > CG_MAX_SLICES ? CG_MAX_SLICES : n;
  const long chunk = (rows + n - 1) / n;
  return CgSlices{(int)((rows + chunk - 1) / chunk), chunk};
}
static int cg_nsplit(long rows) {
  long n = (rows + CG_DW_SPLIT_ROWS - 1) / CG_DW_SPLIT_ROWS;
  return (int)(n < 1 ? 1 : n > CG_DW_MAX_SPLIT ? CG_DW_MAX_SPLIT : n);
}

// conv2c: what its r holds is the block's output
static bool cg_block_out(const CgLayout& L, int site) { return site >= L.has_stem && (site - L.has_stem) % 4 == SITE_CONV2C; }

static chiron_status cg_layout(const chiron_model_desc* d, int64_t batch, int64_t seg, bool want_shape, CgLayout* o) {
  BlobMap map;
  chiron_status st = blob_map(d, &map);
  if (st) return st;
  CgLayout& L = *o;
  L = CgLayout();
  L.n_blocks = d->n_blocks;
  L.has_stem = map.has_stem;
  const int ns = L.n_sites = map.n_sites;
  for (int i = 0; i < ns; ++i) static_cast<ConvSite&>(L.s[i]) = map.site[i];
  L.n_params = map.cnn_floats;
  L.C = d->blocks[d->n_blocks - 1].out_channels;
  for (int i = 0; i < ns; ++i) {
    if (L.s[i].co > 4 * CG_RED_THREADS) return set_error(CHIRON_ERR_INVALID, "the CNN training kernels take at most %d channels, not %d", 4 * CG_RED_THREADS, L.s[i].co);
    if (L.s[i].ci != 1 && L.s[i].ci % 4) return set_error(CHIRON_ERR_INVALID, "the CNN training kernels need channel counts that are multiples of 4, not %d", L.s[i].ci);
  }
  if (!want_shape) return CHIRON_OK;
  if (batch < 1 || seg < 1) return set_error(CHIRON_ERR_INVALID, "batch %lld, segment_len %lld: both must be positive", (long long)batch, (long long)seg);
  if (batch > (1 << 20) || seg > (1 << 24) || batch * seg > (1LL << 24))
    return set_error(CHIRON_ERR_OVERFLOW, "batch %lld x segment_len %lld beyond the training kernels' range (batch 2^20, 2^24 rows)", (long long)batch, (long long)seg);
  L.B = (int)batch;
  L.L = (int)seg;
  SiteFrames fr[MAX_SITES];
  const int t = L.T = frames(map, (int)seg, fr);
  size_t f = 0, big = 0;
  for (int i = 0; i < ns; ++i) {
    CgSite& s = L.s[i];
    s.tin = fr[i].tin; s.tout = fr[i].tout; s.pad = fr[i].pad;
    s.rows = (long)L.B * s.tout;
    const size_t act = (size_t)s.rows * s.co;
    if (act > big) big = act;
    s.y_in_ws = !s.bn;
    if (s.bn) { s.y = f; f += act; s.stat = f; f += 4 * (size_t)s.co; }
    if (s.relu || cg_block_out(L, i)) { s.r = f; f += act; }
  }
  if (t > CHIRON_CTC_MAX_T) return set_error(CHIRON_ERR_OVERFLOW, "%d frames: the training kernels take at most %d", t, CHIRON_CTC_MAX_T);
  L.tape_floats = f;
  f = 0;
  for (int i = 0; i < 4; ++i) { L.buf[i] = f; f += big; }
  size_t part = 0;
  for (int i = 0; i < ns; ++i) {
    const CgSite& s = L.s[i];
    size_t p = (size_t)cg_slices(s.rows).n * 3 * s.co;
    if (p > part) part = p;
    p = s.ci == 1 ? (size_t)cg_slices(s.rows).n * CG_R1_TAPS * s.co : (size_t)s.k * cg_nsplit(s.rows) * s.ci * s.co;
    if (p > part) part = p;
  }
  L.part = f; f += part;
  L.sums = f; f += 3 * (size_t)(4 * CG_RED_THREADS);
  L.ws_floats = f;
  return CHIRON_OK;
}

static unsigned cg_grid(long n, int threads) {
  long g = (n + threads - 1) / threads;
  return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

static CgRows cg_rows_fwd(const CgSite& s) { return CgRows{s.tout, s.tin, s.stride, 1, -s.pad, 1}; }
static CgRows cg_rows_dx(const CgSite& s) { return CgRows{s.tin, s.tout, 1, s.stride, s.pad, -1}; }

// y = conv(x): x [B * tin][ci] (the signal when ci == 1)
static void cg_conv_forward(const CgSite& s, const float* x, const float* w, float* y, hipStream_t stream) {
  if (s.ci == 1) {
    CgRank1 p = {};
    p.x = x; p.w = w; p.y = y; p.g = cg_rows_fwd(s); p.k = s.k; p.C = s.co; p.rows = s.rows;
    hipLaunchKernelGGL(cg_rank1_fwd_kernel, dim3(cg_grid(s.rows * (s.co / 4), 256)), dim3(256), 0, stream, p);
    return;
  }
  CgConv p = {};
  p.A = x; p.lda = s.ci; p.g = cg_rows_fwd(s); p.ntaps = s.k;
  p.B = w; p.sbt = (long)s.ci * s.co; p.sbr = s.co; p.sbj = 1;
  p.C = y; p.ldc = s.co; p.I = (int)s.rows; p.J = s.co; p.R = s.ci;
  hipLaunchKernelGGL(cg_conv_kernel, dim3((p.I + CT - 1) / CT, (p.J + CT - 1) / CT), dim3(256), 0, stream, p);
}

// dx (+)= conv^T(dy): dx [B * tin][ci]
static void cg_conv_dx(const CgSite& s, const float* dy, const float* w, float* dx, bool accumulate, hipStream_t stream) {
  CgConv p = {};
  p.A = dy; p.lda = s.co; p.g = cg_rows_dx(s); p.ntaps = s.k;
  p.B = w; p.sbt = (long)s.ci * s.co; p.sbr = 1; p.sbj = s.co;
  p.C = dx; p.ldc = s.ci; p.I = (int)((long)s.rows / s.tout * s.tin); p.J = s.ci; p.R = s.co;
  p.accumulate = accumulate ? 1 : 0;
  hipLaunchKernelGGL(cg_conv_kernel, dim3((p.I + CT - 1) / CT, (p.J + CT - 1) / CT), dim3(256), 0, stream, p);
}

// dw [k][ci][co] = sum over rows of x_tap^T dy
static void cg_conv_dw(const CgSite& s, const float* x, const float* dy, float* part, float* dw, hipStream_t stream) {
  if (s.ci == 1) {
    const CgSlices sl = cg_slices(s.rows);
    const int nsl = sl.n;
    for (int tap0 = 0; tap0 < s.k; tap0 += CG_R1_TAPS) {
      CgRank1 p = {};
      p.x = x; p.dy = dy; p.part = part; p.g = cg_rows_fwd(s); p.k = s.k; p.C = s.co; p.rows = s.rows;
      p.chunk = sl.chunk;
      p.tap0 = tap0;
      p.nt = s.k - tap0 < CG_R1_TAPS ? s.k - tap0 : CG_R1_TAPS;
      hipLaunchKernelGGL(cg_rank1_dw_kernel, dim3(nsl), dim3(CG_RED_THREADS), 0, stream, p);
      const long n = (long)p.nt * s.co;
      hipLaunchKernelGGL(cg_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part, nsl, n, n, dw + (size_t)tap0 * s.co);
    }
    return;
  }
  CgDw p = {};
  p.X = x; p.ldx = s.ci; p.g = cg_rows_fwd(s); p.dY = dy; p.ldy = s.co; p.part = part;
  p.I = s.ci; p.J = s.co; p.R = (int)s.rows;
  p.nsplit = cg_nsplit(s.rows);
  p.chunk = (int)(((s.rows + p.nsplit - 1) / p.nsplit + CK - 1) / CK * CK);
  hipLaunchKernelGGL(cg_dw_kernel, dim3((p.J + CT - 1) / CT, (p.I + CT - 1) / CT, s.k * p.nsplit), dim3(256), 0, stream, p);
  const long n = (long)s.ci * s.co, tot = n * s.k;
  hipLaunchKernelGGL(cg_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, part, p.nsplit, n, tot, dw);
}

// the batch's moments of y -> stat, moments_out
static void cg_moments(const CgSite& s, const float* y, const float* bn, float* stat, float* mom, float* part, hipStream_t stream) {
  const CgSlices sl = cg_slices(s.rows);
  const int nsl = sl.n;
  const long chunk = sl.chunk;
  const unsigned g = (s.co + 255) / 256;
  hipLaunchKernelGGL(cg_sum_kernel, dim3(nsl), dim3(CG_RED_THREADS), 0, stream, y, s.rows, s.co, chunk, (const float*)nullptr, part);
  hipLaunchKernelGGL(cg_mean_finish_kernel, dim3(g), dim3(256), 0, stream, part, nsl, s.co, (float)s.rows, stat);
  hipLaunchKernelGGL(cg_sum_kernel, dim3(nsl), dim3(CG_RED_THREADS), 0, stream, y, s.rows, s.co, chunk, (const float*)stat, part);
  hipLaunchKernelGGL(cg_var_finish_kernel, dim3(g), dim3(256), 0, stream, part, nsl, s.co, (float)s.rows, bn, stat, mom);
}

// ReLU mask + BN backward of one site: din (gradient at the BN / ReLU output) -> dy_out (gradient at the convolution output)
static void cg_bn_backward(const CgSite& s, const float* din, const float* relu_out, const float* tape, const float* params, float* dparams,
                           float* part, float* sums, float* dy_out, float* g_out, hipStream_t stream) {
  const CgSlices sl = cg_slices(s.rows);
  const int nsl = sl.n;
  const long chunk = sl.chunk;
  const float* stat = tape + s.stat;
  hipLaunchKernelGGL(cg_bn_bwd_sum_kernel, dim3(nsl), dim3(CG_RED_THREADS), 0, stream, din, relu_out, tape + s.y, stat, s.rows, s.co, chunk, part);
  hipLaunchKernelGGL(cg_bn_bwd_finish_kernel, dim3((s.co + 255) / 256), dim3(256), 0, stream, part, nsl, s.co, (float)s.rows, sums, dparams + s.bn_off);
  CgBnBwd p = {};
  p.din = din; p.relu_out = relu_out; p.y = tape + s.y; p.stat = stat; p.scale = params + s.bn_off; p.sums = sums;
  p.dy_out = dy_out; p.g_out = g_out;
  p.n4 = s.rows * (s.co / 4);
  p.C = s.co;
  hipLaunchKernelGGL(cg_bn_bwd_apply_kernel, dim3(cg_grid(p.n4, 256)), dim3(256), 0, stream, p);
}

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_cnn_params_range(const chiron_model_desc* desc, size_t* first_float, size_t* n_floats) {
  CgLayout L;
  chiron_status st = cg_layout(desc, 0, 0, false, &L);
  if (st) return st;
  if (!first_float || !n_floats) return set_error(CHIRON_ERR_INVALID, "chiron_cnn_params_range: null output");
  *first_float = 0;
  *n_floats = L.n_params;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_cnn_train_sizes(const chiron_model_desc* desc, int32_t batch, int32_t segment_len, size_t* tape_bytes,
                                                size_t* workspace_bytes) {
  CgLayout L;
  chiron_status st = cg_layout(desc, batch, segment_len, true, &L);
  if (st) return st;
  if (!tape_bytes || !workspace_bytes) return set_error(CHIRON_ERR_INVALID, "chiron_cnn_train_sizes: null output");
  *tape_bytes = L.tape_floats * sizeof(float);
  *workspace_bytes = L.ws_floats * sizeof(float);
  return CHIRON_OK;
}

extern "C" chiron_status chiron_cnn_train_tape_relu(const chiron_model_desc* desc, int32_t batch, int32_t segment_len, int32_t index,
                                                    size_t* offset_floats, int32_t* frames, int32_t* channels) {
  CgLayout L;
  chiron_status st = cg_layout(desc, batch, segment_len, true, &L);
  if (st) return st;
  if (!offset_floats || !frames || !channels) return set_error(CHIRON_ERR_INVALID, "chiron_cnn_train_tape_relu: null output");
  int seen = 0;
  for (int i = 0; i < L.n_sites; ++i) {
    const CgSite& s = L.s[i];
    if (!(s.relu || cg_block_out(L, i))) continue;
    if (seen++ == index) {
      *offset_floats = s.r;
      *frames = s.tout;
      *channels = s.co;
      return CHIRON_OK;
    }
  }
  return set_error(CHIRON_ERR_INVALID, "chiron_cnn_train_tape_relu: index %d outside the %d ReLU outputs", index, seen);
}

extern "C" chiron_status chiron_cnn_train_forward(int32_t device_id, const chiron_model_desc* desc, const float* params, const float* signal,
                                                  int32_t batch, int32_t segment_len, float* features_out, float* moments_out, void* tape_,
                                                  void* workspace_, void* stream_) {
  const char* who = "chiron_cnn_train_forward";
  CgLayout L;
  chiron_status st = cg_layout(desc, batch, segment_len, true, &L);
  if (st) return st;
  if (!params || !signal || !features_out || !moments_out || !tape_ || !workspace_) return set_error(CHIRON_ERR_INVALID, "%s: null operand", who);
  if ((st = enter_device(who, device_id))) return st;
  if (!(on_device(params) && on_device(signal) && on_device(features_out) && on_device(moments_out) && on_device(tape_) &&
        on_device(workspace_)))
    return set_error(CHIRON_ERR_INVALID, "%s: every operand must be device memory on device %d", who, device_id);
  hipStream_t stream = (hipStream_t)stream_;
  float* tape = (float*)tape_;
  float* ws = (float*)workspace_;
  float* part = ws + L.part;
  // one site: convolution, and with BN the batch's moments; the BN itself is applied by the caller below
  auto conv = [&](const CgSite& s, const float* x) -> float* {
    float* y = s.y_in_ws ? ws + L.buf[0] : tape + s.y;
    cg_conv_forward(s, x, params + s.w_off, y, stream);
    if (s.bn) cg_moments(s, y, params + s.bn_off, tape + s.stat, moments_out + s.bn_off, part, stream);
    return y;
  };
  auto apply = [&](const CgSite& s, const float* y, const float* y2, const float* stat2, float* out2) {
    const int relu = 1;
    CgApply p = {};
    p.y = y; p.stat = tape + s.stat; p.y2 = y2; p.stat2 = stat2; p.out = tape + s.r; p.out2 = out2;
    p.n4 = s.rows * (s.co / 4);
    p.C = s.co;
    p.relu = relu;
    hipLaunchKernelGGL(cg_bn_apply_kernel, dim3(cg_grid(p.n4, 256)), dim3(256), 0, stream, p);
  };
  const float* x = signal;
  int si = 0;
  if (L.has_stem) {
    const CgSite& s = L.s[si++];
    apply(s, conv(s, x), nullptr, nullptr, nullptr);
    x = tape + s.r;
  }
  for (int i = 0; i < L.n_blocks; ++i, si += 4) {
    const CgSite &b1 = L.s[si], &a = L.s[si + 1], &b = L.s[si + 2], &c = L.s[si + 3];
    const float* y1 = conv(b1, x);
    apply(a, conv(a, x), nullptr, nullptr, nullptr);
    apply(b, conv(b, tape + a.r), nullptr, nullptr, nullptr);
    // relu(b1 + bn(conv2c)); the last block's output goes to the tape (the backward's mask) and to features_out in the same pass
    apply(c, conv(c, tape + b.r), y1, b1.bn ? tape + b1.stat : nullptr, i == L.n_blocks - 1 ? features_out : nullptr);
    x = tape + c.r;
  }
  return launched(who);
}

extern "C" chiron_status chiron_cnn_train_backward(int32_t device_id, const chiron_model_desc* desc, const float* params, const float* signal,
                                                   const float* dfeatures, int32_t batch, int32_t segment_len, const void* tape_,
                                                   void* workspace_, float* dparams_out, void* stream_) {
  const char* who = "chiron_cnn_train_backward";
  CgLayout L;
  chiron_status st = cg_layout(desc, batch, segment_len, true, &L);
  if (st) return st;
  if (!params || !signal || !dfeatures || !tape_ || !workspace_ || !dparams_out) return set_error(CHIRON_ERR_INVALID, "%s: null operand", who);
  if ((st = enter_device(who, device_id))) return st;
  if (!(on_device(params) && on_device(signal) && on_device(dfeatures) && on_device(tape_) && on_device(workspace_) &&
        on_device(dparams_out)))
    return set_error(CHIRON_ERR_INVALID, "%s: every operand must be device memory on device %d", who, device_id);
  hipStream_t stream = (hipStream_t)stream_;
  const float* tape = (const float*)tape_;
  float* ws = (float*)workspace_;
  float* part = ws + L.part;
  float* sums = ws + L.sums;
  float *P = ws + L.buf[0], *Q = ws + L.buf[1], *Rr = ws + L.buf[2], *G = ws + L.buf[3];
  const float* dcur = dfeatures;
  for (int i = L.n_blocks - 1; i >= 0; --i) {
    const int si = (L.has_stem ? 1 : 0) + 4 * i;
    const CgSite &b1 = L.s[si], &a = L.s[si + 1], &b = L.s[si + 2], &c = L.s[si + 3];
    const float* x = si == 0 ? signal : tape + L.s[si - 1].r;   // the block's input: the signal, the stem's or the previous block's output
    const float* out = tape + c.r;
    // the final ReLU's mask and the residual fan-out: conv2c's BN backward reads dcur under the mask; the shortcut gets the masked
    // gradient itself (no BN) or its own BN backward under the same mask
    cg_bn_backward(c, dcur, out, tape, params, dparams_out, part, sums, Q, b1.bn ? nullptr : G, stream);
    if (b1.bn) cg_bn_backward(b1, dcur, out, tape, params, dparams_out, part, sums, G, nullptr, stream);
    cg_conv_dw(c, tape + b.r, Q, part, dparams_out + c.w_off, stream);
    cg_conv_dx(c, Q, params + c.w_off, Rr, false, stream);
    cg_bn_backward(b, Rr, tape + b.r, tape, params, dparams_out, part, sums, Rr, nullptr, stream);
    cg_conv_dw(b, tape + a.r, Rr, part, dparams_out + b.w_off, stream);
    cg_conv_dx(b, Rr, params + b.w_off, Q, false, stream);
    cg_bn_backward(a, Q, tape + a.r, tape, params, dparams_out, part, sums, Q, nullptr, stream);
    cg_conv_dw(a, x, Q, part, dparams_out + a.w_off, stream);
    cg_conv_dw(b1, x, G, part, dparams_out + b1.w_off, stream);
    if (a.ci != 1) {   // no gradient with respect to the signal
      cg_conv_dx(a, Q, params + a.w_off, P, false, stream);
      cg_conv_dx(b1, G, params + b1.w_off, P, true, stream);
      dcur = P;
    }
  }
  if (L.has_stem) {
    const CgSite& s = L.s[0];
    cg_bn_backward(s, dcur, tape + s.r, tape, params, dparams_out, part, sums, Q, nullptr, stream);
    cg_conv_dw(s, signal, Q, part, dparams_out + s.w_off, stream);
  }
  return launched(who);
}
