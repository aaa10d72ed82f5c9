// Training seam of the recurrent stack and the FC head (fp32, gfx950): forward with a tape, BPTT, weight / input gradients.
//
// Reference: chiron/chiron_rcnn_train.py:99-109 (sess.run([net.ctc_loss, net.step])) restricted to the variables of rnn.py:20-97
// (DNA, stack_bidirectional_dynamic_rnn), :99-174 (RNA, MultiRNNCell) and the head :72-96; semantics of oracle/nn_oracle.py:lstm_direction.
// The CNN is frozen: the seam is its feature tensor [B, T, C], and the backward pass returns d loss / d features.
//
// Buffers (all fp32, time-major rows m = t * BP + b, BP = batch rounded up to RG_ROWS; rows b >= B carry seq_len 0 and zeros):
//   tape      Xt [T][BP][C]            the features, transposed            (x-projection of layer 0, dWx of layer 0)
//             Hout[l] [T][BP][2H]      every layer's output by FRAME       (input of layer l + 1, Hprev of dWh, head)
//             G[l][d] [T][BP][5][H]    by STEP: gates i, tanh(j), f, o after their activation, and the cell state c
//   workspace Zx, dZ [T][BP][2][4H]    x-projection / gate derivatives by FRAME, both directions side by side
//             dH[2] [T][BP][2H]        d loss / d Hout of the layer being walked and of the one below it
//             dXt [T][BP][C]           d loss / d Xt, transposed into dfeatures at the end
//             part                     split-K partial sums + the head's per-workgroup partial sums
//
// Kernels:
//   rg_gemm_kernel    C[i][j] (+)= sum_r A[i sai + r sar] B[r sbr + j sbj] on v_mfma_f32_32x32x2_f32, 128 x 128 x 16 tiles; every product of
//                     this file is one instance (strides make the transposes).  gridDim.z > 1: split-K over r into per-split partials,
//                     summed by rg_reduce_kernel in split order -- no float atomics, the same bits run to run.
//   rg_lstm_fwd       16 rows x one direction x all steps per workgroup: z = h W_hh on v_mfma_f32_16x16x4_f32 with W_hh resident in
//                     registers (5 waves x 5 column tiles x 25 k-steps = 125 VGPRs a lane), gates on the VALU, tape written per step.
//   rg_lstm_bwd       the same rows walked backwards: dz from the tape, dh_rec = dz W_hh^T on the same instruction with W_hh^T resident
//                     (7 waves x one 16-unit tile x 100 k-steps = 100 VGPRs a lane), dc carried in registers.
//   rg_head_bwd       FC head gradients, per-workgroup partials in row order + the same fixed-order second pass.
#include "kernels.h"
#include "model_layout.h"

#include <cstdio>

namespace chiron {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RG_ROWS = 16;        // batch rows per recurrence workgroup = M of v_mfma_f32_16x16x4_f32
constexpr int RG_H = LSTM_K;       // 100
constexpr int RG_G = 4 * RG_H;     // 400 gate columns, i | j | f | o
constexpr int RG_ZLD = RG_G + 4;   // LDS row stride of z / dz
constexpr int RG_HLD = RG_H + 1;   // LDS row stride of h / dh_rec
constexpr int RG_FWD_WAVES = 5, RG_BWD_WAVES = 7;
constexpr int RG_MAX_SPLIT = 64;
constexpr int RG_SPLIT_ROWS = 2048;  // reduction rows per split-K slice
constexpr int RG_HEAD_WG = 256;      // most workgroups of the head backward
constexpr int RG_HEAD_ROWS = 128;    // least rows per workgroup of the head backward

// ---------------------------------------------------------------------------------------------
// generic strided GEMM
// ---------------------------------------------------------------------------------------------
struct RgGemm {
  const float* A; long sai, sar;
  const float* B; long sbr, sbj;
  float* C; long ldc;          // nsplit == 1: C[i * ldc + j]; else partial slice z at C + z * I * J, row stride J
  int I, J, R;
  int accumulate;              // nsplit == 1: C += product
  int chunk;                   // reduction rows per split (multiple of 16)
};

constexpr int GT = 128, GK = 16, GLD = GT + 4;
constexpr int RG_MAX_GRID_Y = 65535;   // a grid's y extent: HIP documents 65535, the MI355X reports 65536

__global__ __launch_bounds__(256) void rg_gemm_kernel(const RgGemm p) {
  __shared__ float As[GK][GLD];
  __shared__ float Bs[GK][GLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.y * GT, j0 = blockIdx.x * GT;
  const int r_begin = blockIdx.z * p.chunk;
  const int r_end = min(p.R, r_begin + p.chunk);
  const int wm = wave >> 1, wn = wave & 1;
  // loader geometry: the contiguous index of each operand runs along the lanes
  const bool a_r = p.sar == 1, b_r = p.sbr == 1;
  float ra[8], rb[8];
  auto load = [&](int r0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      int ii, rr;
      if (a_r) { rr = tid & 15; ii = (tid >> 4) + 16 * q; } else { ii = tid & 127; rr = (tid >> 7) + 2 * q; }
      const int gi = i0 + ii, gr = r0 + rr;
      ra[q] = (gi < p.I && gr < r_end) ? p.A[(long)gi * p.sai + (long)gr * p.sar] : 0.f;
      int jj;
      if (b_r) { rr = tid & 15; jj = (tid >> 4) + 16 * q; } else { jj = tid & 127; rr = (tid >> 7) + 2 * q; }
      const int gj = j0 + jj;
      const int gr2 = r0 + rr;
      rb[q] = (gj < p.J && gr2 < r_end) ? p.B[(long)gr2 * p.sbr + (long)gj * p.sbj] : 0.f;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (a_r) As[tid & 15][(tid >> 4) + 16 * q] = ra[q]; else As[(tid >> 7) + 2 * q][tid & 127] = ra[q];
      if (b_r) Bs[tid & 15][(tid >> 4) + 16 * q] = rb[q]; else Bs[(tid >> 7) + 2 * q][tid & 127] = rb[q];
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  if (r_begin < r_end) load(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += GK) {
    stash();
    __syncthreads();
    if (r0 + GK < r_end) load(r0 + GK);
#pragma unroll
    for (int k2 = 0; k2 < GK / 2; ++k2) {
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
    __syncthreads();
  }
  const bool split = gridDim.z > 1;
  float* C = split ? p.C + (long)blockIdx.z * p.I * p.J : p.C;
  const long ldc = split ? p.J : p.ldc;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int gi = i0 + wm * 64 + m * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
        const int gj = j0 + wn * 64 + n * 32 + (lane & 31);
        if (gi < p.I && gj < p.J) {
          float* dst = C + (long)gi * ldc + gj;
          *dst = (!split && p.accumulate) ? *dst + acc[m][n][e] : acc[m][n][e];
        }
      }
}

// out[i * ldo + j] = sum over the slices, in slice order
__global__ __launch_bounds__(256) void rg_reduce_kernel(const float* part, int nsplit, long n, int J, float* out, long ldo) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  float s = part[idx];
  for (int z = 1; z < nsplit; ++z) s += part[(long)z * n + idx];
  out[(idx / J) * ldo + idx % J] = s;
}

// part[z][j] = sum of x[m * ld + j] over the rows of slice z, in row order (400 columns)
__global__ __launch_bounds__(512) void rg_colsum_kernel(const float* x, long ld, long M, long chunk, float* part) {
  const int j = threadIdx.x;
  if (j >= RG_G) return;
  const long m0 = (long)blockIdx.x * chunk;
  const long m1 = m0 + chunk < M ? m0 + chunk : M;
  float s = 0.f;
  for (long m = m0; m < m1; ++m) s += x[m * ld + j];
  part[(long)blockIdx.x * RG_G + j] = s;
}

static int rg_nsplit(long R) {
  long n = (R + RG_SPLIT_ROWS - 1) / RG_SPLIT_ROWS;
  return (int)(n < 1 ? 1 : n > RG_MAX_SPLIT ? RG_MAX_SPLIT : n);
}

// split = true: reduction over the T * BP rows, through `part`
static void rg_gemm(RgGemm g, bool split, float* part, hipStream_t stream) {
  const int nsplit = split ? rg_nsplit(g.R) : 1;
  g.chunk = ((g.R + nsplit - 1) / nsplit + GK - 1) / GK * GK;
  float* out = g.C;
  const long ldo = g.ldc;
  if (nsplit > 1) g.C = part;
  dim3 grid((g.J + GT - 1) / GT, (g.I + GT - 1) / GT, nsplit);
  hipLaunchKernelGGL(rg_gemm_kernel, grid, dim3(256), 0, stream, g);
  if (nsplit > 1) {
    const long n = (long)g.I * g.J;
    hipLaunchKernelGGL(rg_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part, nsplit, n, g.J, out, ldo);
  }
}

// ---------------------------------------------------------------------------------------------
// [B][T][C] <-> [T][BP][C]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_to_time_major(const float* src, float* dst, int B, int BP, int T, int C) {
  const long n = (long)T * BP * C;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const long m = idx / C;
    const int b = (int)(m % BP), t = (int)(m / BP);
    dst[idx] = b < B ? src[((long)b * T + t) * C + c] : 0.f;
  }
}
__global__ __launch_bounds__(256) void rg_to_batch_major(const float* src, float* dst, int B, int BP, int T, int C) {
  const long n = (long)B * T * C;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const long m = idx / C;
    const int t = (int)(m % T), b = (int)(m / T);
    dst[idx] = src[((long)t * BP + b) * C + c];
  }
}

// ---------------------------------------------------------------------------------------------
// forward recurrence with tape
// ---------------------------------------------------------------------------------------------
struct RgLstm {
  const float* kernel[2];   // per direction: lstm_cell/kernel [(in + H)][4H]; the recurrent rows start at row `in`
  const float* bias[2];     // [4H]
  int in;
  const int32_t* seq_len;   // [B]
  const float* zx;          // [T][BP][2][4H] by frame (forward: input; backward: unused)
  float* hout;              // [T][BP][2H] by frame
  float* tape[2];           // [T][BP][5][H] by step
  const float* dhout;       // backward: [T][BP][2H] by frame
  float* dz;                // backward: [T][BP][2][4H] by frame
  int T, B, BP;
};

__device__ __forceinline__ float rg_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
// tanhf, not (1 - e) / (1 + e): a closed input gate leaves c of the order of 1e-22, where 1 - exp(-2c) is 0 and the gradient of
// everything downstream with it
__device__ __forceinline__ float rg_tanh(float v) { return tanhf(v); }

__global__ __launch_bounds__(RG_FWD_WAVES * 64) void rg_lstm_fwd(const RgLstm p) {
  __shared__ float zs[RG_ROWS][RG_ZLD];
  __shared__ float hs[RG_ROWS][RG_HLD];
  __shared__ int lens[RG_ROWS];
  __shared__ float bsh[RG_G];   // bias, the forget gate's with its +1.0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dir = blockIdx.y, b0 = blockIdx.x * RG_ROWS;
  const int kq = lane >> 4, ln = lane & 15;
  const float* whh = p.kernel[dir] + (long)p.in * RG_G;
  // resident W_hh: k-step ks of lane group kq multiplies k = 25 kq + ks (any fixed permutation of k serves A and B alike)
  float w[5][25];
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int ks = 0; ks < 25; ++ks) w[t][ks] = whh[(long)(25 * kq + ks) * RG_G + 80 * wave + 16 * t + ln];
  if (tid < RG_ROWS) {
    const int b = b0 + tid;
    int n = b < p.B ? p.seq_len[b] : 0;
    lens[tid] = n < 0 ? 0 : n > p.T ? p.T : n;
  }
  for (int e = tid; e < RG_ROWS * RG_HLD; e += blockDim.x) (&hs[0][0])[e] = 0.f;
  for (int e = tid; e < RG_G; e += blockDim.x) bsh[e] = p.bias[dir][e] + (e / RG_H == 2 ? 1.0f : 0.f);
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int r = 0; r < RG_ROWS; ++r) maxlen = max(maxlen, lens[r]);
  // element ownership: 1600 (row, unit) pairs over 320 threads
  int row[5], unit[5], len[5];
  float c[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int e = tid + 320 * q;
    row[q] = e / RG_H;
    unit[q] = e - row[q] * RG_H;
    len[q] = lens[row[q]];
    c[q] = 0.f;
  }
  float zx[5][4];
  auto load_zx = [&](int s) {
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const bool act = s < len[q];
      const int frame = dir ? len[q] - 1 - s : s;
      const float* src = p.zx + (((long)(act ? frame : 0) * p.BP + b0 + row[q]) * 2 + dir) * RG_G + unit[q];
#pragma unroll
      for (int g = 0; g < 4; ++g) zx[q][g] = act ? src[g * RG_H] : 0.f;
    }
  };
  load_zx(0);
  for (int s = 0; s < p.T; ++s) {
    if (s >= maxlen) {   // every row of the group is past its end: frames s .. T-1 emit 0
#pragma unroll
      for (int q = 0; q < 5; ++q) p.hout[((long)s * p.BP + b0 + row[q]) * (2 * RG_H) + dir * RG_H + unit[q]] = 0.f;
      continue;
    }
    f32x4 acc[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 25; ++ks) {
      const float a = hs[ln][25 * kq + ks];
#pragma unroll
      for (int t = 0; t < 5; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w[t][ks], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) zs[4 * kq + i][80 * wave + 16 * t + ln] = acc[t][i];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const bool act = s < len[q];
      const int frame = (dir && act) ? len[q] - 1 - s : s;
      float hv = 0.f;
      if (act) {
        const float gi = rg_sigmoid(zs[row[q]][unit[q]] + zx[q][0] + bsh[unit[q]]);
        const float gj = rg_tanh(zs[row[q]][RG_H + unit[q]] + zx[q][1] + bsh[RG_H + unit[q]]);
        const float gf = rg_sigmoid(zs[row[q]][2 * RG_H + unit[q]] + zx[q][2] + bsh[2 * RG_H + unit[q]]);
        const float go = rg_sigmoid(zs[row[q]][3 * RG_H + unit[q]] + zx[q][3] + bsh[3 * RG_H + unit[q]]);
        c[q] = gf * c[q] + gi * gj;
        hv = go * rg_tanh(c[q]);
        float* tp = p.tape[dir] + ((long)s * p.BP + b0 + row[q]) * (5 * RG_H) + unit[q];
        tp[0] = gi;
        tp[RG_H] = gj;
        tp[2 * RG_H] = gf;
        tp[3 * RG_H] = go;
        tp[4 * RG_H] = c[q];
        hs[row[q]][unit[q]] = hv;
      }
      // an ended row's frame s (>= its length) emits 0 in both directions
      p.hout[((long)frame * p.BP + b0 + row[q]) * (2 * RG_H) + dir * RG_H + unit[q]] = hv;
    }
    if (s + 1 < maxlen) load_zx(s + 1);   // in flight across the barrier and the next step's matrix phase
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// BPTT recurrence
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_BWD_WAVES * 64) void rg_lstm_bwd(const RgLstm p) {
  __shared__ float dzs[RG_ROWS][RG_ZLD];
  __shared__ float dhs[RG_ROWS][RG_HLD];
  __shared__ int lens[RG_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dir = blockIdx.y, b0 = blockIdx.x * RG_ROWS;
  const int kq = lane >> 4, ln = lane & 15;
  const float* whh = p.kernel[dir] + (long)p.in * RG_G;
  // resident W_hh^T: this wave's 16 hidden units [16 wave, 16 wave + 16); lane group kq multiplies the gate columns k = 100 kq + ks
  float w[100];
  {
    const int n = 16 * wave + ln;
#pragma unroll
    for (int ks = 0; ks < 100; ++ks) w[ks] = n < RG_H ? whh[(long)n * RG_G + 100 * kq + ks] : 0.f;
  }
  if (tid < RG_ROWS) {
    const int b = b0 + tid;
    int n = b < p.B ? p.seq_len[b] : 0;
    lens[tid] = n < 0 ? 0 : n > p.T ? p.T : n;
  }
  for (int e = tid; e < RG_ROWS * RG_HLD; e += blockDim.x) (&dhs[0][0])[e] = 0.f;
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int r = 0; r < RG_ROWS; ++r) maxlen = max(maxlen, lens[r]);
  constexpr int NT = RG_BWD_WAVES * 64;   // 448 threads, 1600 elements: four a thread, the last ones idle
  int row[4], unit[4], len[4];
  bool own[4];
  float dc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + NT * q;
    own[q] = e < RG_ROWS * RG_H;
    row[q] = own[q] ? e / RG_H : 0;
    unit[q] = own[q] ? e - row[q] * RG_H : 0;
    len[q] = own[q] ? lens[row[q]] : 0;
    dc[q] = 0.f;
  }
  for (int s = p.T - 1; s >= 0; --s) {
    if (s >= maxlen) {   // nothing of this group lives at step s: dz of frame s is 0, dh_rec and dc stay 0
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (own[q]) {
          float* dst = p.dz + (((long)s * p.BP + b0 + row[q]) * 2 + dir) * RG_G + unit[q];
#pragma unroll
          for (int g = 0; g < 4; ++g) dst[g * RG_H] = 0.f;
        }
      continue;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!own[q]) continue;
      const bool act = s < len[q];
      const int frame = (dir && act) ? len[q] - 1 - s : s;
      float d[4] = {0.f, 0.f, 0.f, 0.f};
      if (act) {
        const float* tp = p.tape[dir] + ((long)s * p.BP + b0 + row[q]) * (5 * RG_H) + unit[q];
        const float gi = tp[0], gj = tp[RG_H], gf = tp[2 * RG_H], go = tp[3 * RG_H], cc = tp[4 * RG_H];
        const float cprev = s > 0 ? (tp - (long)p.BP * (5 * RG_H))[4 * RG_H] : 0.f;
        const float dh = p.dhout[((long)frame * p.BP + b0 + row[q]) * (2 * RG_H) + dir * RG_H + unit[q]] + dhs[row[q]][unit[q]];
        const float tc = rg_tanh(cc);
        const float dct = dc[q] + dh * go * (1.f - tc * tc);
        d[0] = dct * gj * gi * (1.f - gi);
        d[1] = dct * gi * (1.f - gj * gj);
        d[2] = dct * cprev * gf * (1.f - gf);
        d[3] = dh * tc * go * (1.f - go);
        dc[q] = dct * gf;
      }
      // a step past the row's end: dz = 0; its dh_rec and dc are still 0 (ended steps come first in this walk), which is "unchanged"
      float* dst = p.dz + (((long)frame * p.BP + b0 + row[q]) * 2 + dir) * RG_G + unit[q];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        dst[g * RG_H] = d[g];
        dzs[row[q]][g * RG_H + unit[q]] = d[g];
      }
    }
    __syncthreads();
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 100; ++ks) {
      const float a = dzs[ln][100 * kq + ks];
      acc[ks & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w[ks], acc[ks & 3], 0, 0, 0);
    }
    const f32x4 r = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    // the readers of dhs (the gate phase) finished before the barrier above; the one below also frees dzs for the next step
    if (16 * wave + ln < RG_H) {
#pragma unroll
      for (int i = 0; i < 4; ++i) dhs[4 * kq + i][16 * wave + ln] = r[i];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// FC head backward (rnn.py:72-96)
// ---------------------------------------------------------------------------------------------
struct RgHead {
  const float* lasth;    // [T][BP][2H]
  const float* dlogits;  // [B][T][5]
  const float* w;        // [2][H]
  const float* bias;     // [H]
  const float* wc;       // [H][5]
  float* dlasth;         // [T][BP][2H]
  float* part;           // [nwg][RG_HEAD_N]
  int T, B, BP, rows_per_wg;
};
constexpr int RG_HEAD_N = 2 * RG_H + RG_H + RG_H * 5 + 5;   // gradient floats of the head, in blob order

__global__ __launch_bounds__(128) void rg_head_bwd(const RgHead p) {
  const int u = threadIdx.x;
  const long M = (long)p.T * p.BP;
  const long m0 = (long)blockIdx.x * p.rows_per_wg;
  const long m1 = m0 + p.rows_per_wg < M ? m0 + p.rows_per_wg : M;
  const bool live = u < RG_H;
  const int uu = live ? u : 0;
  const float w0 = p.w[uu], w1 = p.w[RG_H + uu], bu = p.bias[uu];
  float wc[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) wc[k] = p.wc[uu * 5 + k];
  float g_w0 = 0.f, g_w1 = 0.f, g_b = 0.f, g_wc[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, g_bc = 0.f;
  for (long m = m0; m < m1; ++m) {
    const int t = (int)(m / p.BP), b = (int)(m % p.BP);
    float* dl = p.dlasth + m * (2 * RG_H);
    if (b >= p.B) {   // padding row: no gradient in, none out
      if (live) { dl[u] = 0.f; dl[RG_H + u] = 0.f; }
      continue;
    }
    const float* g = p.dlogits + ((long)b * p.T + t) * 5;
    float gl[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) gl[k] = g[k];
    if (u >= RG_H && u < RG_H + 5) g_bc += gl[u - RG_H];
    if (!live) continue;
    const float hf = p.lasth[m * (2 * RG_H) + u], hb = p.lasth[m * (2 * RG_H) + RG_H + u];
    const float v = hf * w0 + hb * w1 + bu;
    float dv = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      dv += gl[k] * wc[k];
      g_wc[k] += v * gl[k];
    }
    g_b += dv;
    g_w0 += dv * hf;
    g_w1 += dv * hb;
    dl[u] = dv * w0;
    dl[RG_H + u] = dv * w1;
  }
  float* out = p.part + (long)blockIdx.x * RG_HEAD_N;
  if (live) {
    out[u] = g_w0;
    out[RG_H + u] = g_w1;
    out[2 * RG_H + u] = g_b;
#pragma unroll
    for (int k = 0; k < 5; ++k) out[3 * RG_H + u * 5 + k] = g_wc[k];
  } else if (u < RG_H + 5) {
    out[3 * RG_H + 5 * RG_H + (u - RG_H)] = g_bc;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct RgLayout {
  int L, H, C, K, multi;
  int B, BP, T;
  long M;                              // T * BP
  size_t kernel_off[8][2], bias_off[8][2], head_off, n_params;   // floats from the start of the parameter slice
  int in[8];
  size_t first_float;                  // of the slice inside the weight blob
  // tape (floats)
  size_t xt, hout[8], gates[8][2], tape_floats;
  // workspace (floats)
  size_t zx, dz, dh[2], dxt, part, ws_floats;
  int head_wg, head_rows;
};

static chiron_status rg_layout(const chiron_model_desc* d, int64_t batch, int64_t T, bool want_shape, RgLayout* o) {
  BlobMap map;
  chiron_status st = blob_map(d, &map);
  if (st) return st;
  if (d->hidden != RG_H) return set_error(CHIRON_ERR_INVALID, "the training kernels are built for hidden 100, not %d", d->hidden);
  if (d->classes != CHIRON_CLASSES) return set_error(CHIRON_ERR_INVALID, "the training kernels are built for 5 classes, not %d", d->classes);
  RgLayout& L = *o;
  L.L = d->rnn_layers;
  L.H = RG_H;
  L.K = 5;
  L.C = d->blocks[d->n_blocks - 1].out_channels;
  L.multi = d->rnn_kind == CHIRON_RNN_MULTI;
  // the training ABI's params point at the recurrent slice, not at the blob
  L.first_float = map.cnn_floats;
  L.n_params = map.total - map.cnn_floats;
  for (int l = 0; l < L.L; ++l) {
    L.in[l] = map.lstm_in[l];
    for (int dir = 0; dir < 2; ++dir) {
      L.kernel_off[l][dir] = map.lstm_kernel[l][dir] - map.cnn_floats;
      L.bias_off[l][dir] = map.lstm_bias[l][dir] - map.cnn_floats;
    }
  }
  L.head_off = map.head_w - map.cnn_floats;
  if (!want_shape) return CHIRON_OK;
  if (batch < 1 || T < 1) return set_error(CHIRON_ERR_INVALID, "batch %lld, T %lld: both must be positive", (long long)batch, (long long)T);
  if (batch > (1 << 20) || T > CHIRON_CTC_MAX_T) return set_error(CHIRON_ERR_OVERFLOW, "batch %lld / T %lld beyond the training kernels' range (2^20 rows, %d frames)", (long long)batch, (long long)T, CHIRON_CTC_MAX_T);
  const int64_t BP = (batch + RG_ROWS - 1) / RG_ROWS * RG_ROWS;
  if (BP * T > (1 << 24)) return set_error(CHIRON_ERR_OVERFLOW, "T * padded batch = %lld rows: the training kernels index at most 2^24", (long long)(BP * T));
  // the x-projection and dX GEMMs put their T * BP / GT row tiles on grid.y (the tighter of the two bounds as the constants stand)
  if (BP * T > (int64_t)GT * RG_MAX_GRID_Y)
    return set_error(CHIRON_ERR_OVERFLOW, "T * padded batch = %lld rows: the training GEMMs launch at most %d row tiles of %d rows (%lld rows)",
                     (long long)(BP * T), RG_MAX_GRID_Y, GT, (long long)GT * RG_MAX_GRID_Y);
  L.B = (int)batch;
  L.BP = (int)BP;
  L.T = (int)T;
  L.M = BP * T;
  const size_t M = (size_t)L.M;
  size_t f = 0;
  L.xt = f; f += M * L.C;
  for (int l = 0; l < L.L; ++l) { L.hout[l] = f; f += M * 2 * RG_H; }
  for (int l = 0; l < L.L; ++l)
    for (int dir = 0; dir < 2; ++dir) { L.gates[l][dir] = f; f += M * 5 * RG_H; }
  L.tape_floats = f;
  f = 0;
  L.zx = f; f += M * 2 * RG_G;
  L.dz = f; f += M * 2 * RG_G;
  L.dh[0] = f; f += M * 2 * RG_H;
  L.dh[1] = f; f += M * 2 * RG_H;
  L.dxt = f; f += M * L.C;
  L.head_rows = (int)((L.M + RG_HEAD_WG - 1) / RG_HEAD_WG);
  if (L.head_rows < RG_HEAD_ROWS) L.head_rows = RG_HEAD_ROWS;
  L.head_wg = (int)((L.M + L.head_rows - 1) / L.head_rows);
  const int kmax = L.C > 2 * RG_H ? L.C : 2 * RG_H;
  size_t part = (size_t)rg_nsplit(L.M) * kmax * RG_G;
  const size_t hp = (size_t)L.head_wg * RG_HEAD_N;
  L.part = f; f += part > hp ? part : hp;
  L.ws_floats = f;
  return CHIRON_OK;
}

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_rnn_params_range(const chiron_model_desc* desc, size_t* first_float, size_t* n_floats) {
  RgLayout L;
  chiron_status st = rg_layout(desc, 0, 0, false, &L);
  if (st) return st;
  if (!first_float || !n_floats) return set_error(CHIRON_ERR_INVALID, "chiron_rnn_params_range: null output");
  *first_float = L.first_float;
  *n_floats = L.n_params;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_rnn_train_sizes(const chiron_model_desc* desc, int32_t batch, int32_t T, size_t* tape_bytes,
                                                size_t* workspace_bytes) {
  RgLayout L;
  chiron_status st = rg_layout(desc, batch, T, true, &L);
  if (st) return st;
  if (!tape_bytes || !workspace_bytes) return set_error(CHIRON_ERR_INVALID, "chiron_rnn_train_sizes: null output");
  *tape_bytes = L.tape_floats * sizeof(float);
  *workspace_bytes = L.ws_floats * sizeof(float);
  return CHIRON_OK;
}

extern "C" chiron_status chiron_rnn_train_forward(int32_t device_id, const chiron_model_desc* desc, const float* params, const float* features,
                                                  const int32_t* seq_len, int32_t batch, int32_t T, float* logits_out, void* tape_,
                                                  void* workspace_, void* stream_) {
  const char* who = "chiron_rnn_train_forward";
  RgLayout L;
  chiron_status st = rg_layout(desc, batch, T, true, &L);
  if (st) return st;
  if (!params || !features || !seq_len || !logits_out || !tape_ || !workspace_) return set_error(CHIRON_ERR_INVALID, "%s: null operand", who);
  if ((st = enter_device(who, device_id))) return st;
  if (!(on_device(params) && on_device(features) && on_device(seq_len) && on_device(logits_out) && on_device(tape_) &&
        on_device(workspace_)))
    return set_error(CHIRON_ERR_INVALID, "%s: every operand must be device memory on device %d", who, device_id);
  hipStream_t stream = (hipStream_t)stream_;
  float* tape = (float*)tape_;
  float* ws = (float*)workspace_;
  const int BP = L.BP;
  hipLaunchKernelGGL(rg_to_time_major, dim3(2048), dim3(256), 0, stream, features, tape + L.xt, L.B, BP, L.T, L.C);
  for (int l = 0; l < L.L; ++l) {
    const float* x = l == 0 ? tape + L.xt : tape + L.hout[l - 1];
    const int ldx = l == 0 ? L.C : 2 * RG_H;
    for (int dir = 0; dir < 2; ++dir) {
      RgGemm g = {};
      g.A = x + ((L.multi && l > 0) ? dir * RG_H : 0);
      g.sai = ldx;
      g.sar = 1;
      g.B = params + L.kernel_off[l][dir];
      g.sbr = RG_G;
      g.sbj = 1;
      g.C = ws + L.zx + (size_t)dir * RG_G;
      g.ldc = 2 * RG_G;
      g.I = (int)L.M;
      g.J = RG_G;
      g.R = L.in[l];
      rg_gemm(g, false, nullptr, stream);
    }
    RgLstm p = {};
    for (int dir = 0; dir < 2; ++dir) {
      p.kernel[dir] = params + L.kernel_off[l][dir];
      p.bias[dir] = params + L.bias_off[l][dir];
      p.tape[dir] = tape + L.gates[l][dir];
    }
    p.in = L.in[l];
    p.seq_len = seq_len;
    p.zx = ws + L.zx;
    p.hout = tape + L.hout[l];
    p.T = L.T;
    p.B = L.B;
    p.BP = BP;
    hipLaunchKernelGGL(rg_lstm_fwd, dim3(BP / RG_ROWS, 2), dim3(RG_FWD_WAVES * 64), 0, stream, p);
  }
  const float* head = params + L.head_off;
  FcParams f = {};
  f.lasth = tape + L.hout[L.L - 1];
  f.w = head;
  f.bias = head + 2 * RG_H;
  f.wc = head + 3 * RG_H;
  f.bc = head + 3 * RG_H + 5 * RG_H;
  f.logits = logits_out;
  f.T = L.T;
  f.B = L.B;
  f.BP = BP;
  f.H = RG_H;
  f.K = 5;
  launch_fc(f, stream);
  return launched(who);
}

extern "C" chiron_status chiron_rnn_train_backward(int32_t device_id, const chiron_model_desc* desc, const float* params, const float* features,
                                                   const int32_t* seq_len, const float* dlogits, int32_t batch, int32_t T, const void* tape_,
                                                   void* workspace_, float* dparams_out, float* dfeatures_out, void* stream_) {
  const char* who = "chiron_rnn_train_backward";
  RgLayout L;
  chiron_status st = rg_layout(desc, batch, T, true, &L);
  if (st) return st;
  if (!params || !features || !seq_len || !dlogits || !tape_ || !workspace_ || !dparams_out) return set_error(CHIRON_ERR_INVALID, "%s: null operand", who);
  if ((st = enter_device(who, device_id))) return st;
  if (!(on_device(params) && on_device(features) && on_device(seq_len) && on_device(dlogits) && on_device(tape_) &&
        on_device(workspace_) && on_device(dparams_out) && (!dfeatures_out || on_device(dfeatures_out))))
    return set_error(CHIRON_ERR_INVALID, "%s: every operand must be device memory on device %d", who, device_id);
  hipStream_t stream = (hipStream_t)stream_;
  const float* tape = (const float*)tape_;
  float* ws = (float*)workspace_;
  const int BP = L.BP;
  const long M = L.M;
  float* part = ws + L.part;
  // head: dlasth -> dH[0], head gradients -> the tail of dparams
  {
    const float* head = params + L.head_off;
    RgHead h = {};
    h.lasth = tape + L.hout[L.L - 1];
    h.dlogits = dlogits;
    h.w = head;
    h.bias = head + 2 * RG_H;
    h.wc = head + 3 * RG_H;
    h.dlasth = ws + L.dh[0];
    h.part = part;
    h.T = L.T;
    h.B = L.B;
    h.BP = BP;
    h.rows_per_wg = L.head_rows;
    hipLaunchKernelGGL(rg_head_bwd, dim3(L.head_wg), dim3(128), 0, stream, h);
    hipLaunchKernelGGL(rg_reduce_kernel, dim3((RG_HEAD_N + 255) / 256), dim3(256), 0, stream, part, L.head_wg, (long)RG_HEAD_N, RG_HEAD_N,
                       dparams_out + L.head_off, (long)RG_HEAD_N);
  }
  int cur = 0;
  for (int l = L.L - 1; l >= 0; --l) {
    const float* x = l == 0 ? tape + L.xt : tape + L.hout[l - 1];
    const int ldx = l == 0 ? L.C : 2 * RG_H;
    const bool halves = L.multi && l > 0;   // MultiRNNCell above layer 0: each direction reads, and feeds, its own half
    RgLstm p = {};
    for (int dir = 0; dir < 2; ++dir) {
      p.kernel[dir] = params + L.kernel_off[l][dir];
      p.bias[dir] = params + L.bias_off[l][dir];
      p.tape[dir] = const_cast<float*>(tape) + L.gates[l][dir];
    }
    p.in = L.in[l];
    p.seq_len = seq_len;
    p.dhout = ws + L.dh[cur];
    p.dz = ws + L.dz;
    p.T = L.T;
    p.B = L.B;
    p.BP = BP;
    hipLaunchKernelGGL(rg_lstm_bwd, dim3(BP / RG_ROWS, 2), dim3(RG_BWD_WAVES * 64), 0, stream, p);
    const float* hout = tape + L.hout[l];
    for (int dir = 0; dir < 2; ++dir) {
      const float* dz = ws + L.dz + (size_t)dir * RG_G;
      float* dk = dparams_out + L.kernel_off[l][dir];
      RgGemm g = {};
      // dWx = X^T dZ
      g.A = x + (halves ? dir * RG_H : 0);
      g.sai = 1;
      g.sar = ldx;
      g.B = dz;
      g.sbr = 2 * RG_G;
      g.sbj = 1;
      g.C = dk;
      g.ldc = RG_G;
      g.I = L.in[l];
      g.J = RG_G;
      g.R = (int)M;
      rg_gemm(g, true, part, stream);
      // dWh = Hprev^T dZ: forward direction Hprev(t) = Hout(t - 1), backward direction Hout(t + 1) (0 past the row's end, as stored)
      if (L.T > 1) {
        g.A = hout + dir * RG_H + (dir ? (size_t)BP * 2 * RG_H : 0);
        g.sai = 1;
        g.sar = 2 * RG_H;
        g.B = dz + (dir ? 0 : (size_t)BP * 2 * RG_G);
        g.C = dk + (size_t)L.in[l] * RG_G;
        g.I = RG_H;
        g.R = (int)(M - BP);
        rg_gemm(g, true, part, stream);
      } else {
        hipMemsetAsync(dk + (size_t)L.in[l] * RG_G, 0, (size_t)RG_H * RG_G * sizeof(float), stream);
      }
      // db = column sums of dZ, through the same per-slice partials
      {
        const int nsplit = rg_nsplit(M);
        const long chunk = (M + nsplit - 1) / nsplit;
        hipLaunchKernelGGL(rg_colsum_kernel, dim3(nsplit), dim3(512), 0, stream, dz, (long)2 * RG_G, M, chunk, part);
        hipLaunchKernelGGL(rg_reduce_kernel, dim3((RG_G + 255) / 256), dim3(256), 0, stream, part, nsplit, (long)RG_G, RG_G,
                           dparams_out + L.bias_off[l][dir], (long)RG_G);
      }
      // dX = dZ Wx^T: dh_out of the layer below (stack: the directions add; multi above layer 0: each its own half), or d features
      if (l > 0 || dfeatures_out) {
        RgGemm gx = {};
        gx.A = dz;
        gx.sai = 2 * RG_G;
        gx.sar = 1;
        gx.B = params + L.kernel_off[l][dir];
        gx.sbr = 1;
        gx.sbj = RG_G;
        gx.C = l == 0 ? ws + L.dxt : ws + L.dh[cur ^ 1] + (halves ? dir * RG_H : 0);
        gx.ldc = ldx;
        gx.I = (int)M;
        gx.J = L.in[l];
        gx.R = RG_G;
        gx.accumulate = (!halves && dir == 1) ? 1 : 0;
        rg_gemm(gx, false, nullptr, stream);
      }
    }
    cur ^= 1;
  }
  if (dfeatures_out) hipLaunchKernelGGL(rg_to_batch_major, dim3(2048), dim3(256), 0, stream, ws + L.dxt, dfeatures_out, L.B, BP, L.T, L.C);
  return launched(who);
}
