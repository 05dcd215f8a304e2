// The pieces a row-tile forward of the fp32 traversability MLPs is made of, stated once for seg_table_kernel (segment_predict.hip,
// 16 rows), mlp_train_fwd_kernel (mlp_train.hip, 32 rows) and dmlp_fwd_kernel (double_mlp.hip, 16 rows): the x-tile load, the three
// SimpleMLP layers (D -> 256 -> 32 -> 1 + D) on a tile held in LDS, the row sum of 256 squared-error partials and the write of a
// table row.  Workgroups of 256 threads.  A kernel keeps its tile height, its LDS layout and what it does with each finished value:
// it passes that as a callable, and the ReLU form and the confidence function as template arguments.  Every dot product is ONE
// ascending fp32 FMA chain from the bias, the same for every row wherever it sits in a tile.
// The pieces are __forceinline__ and the callables capture plain values (pointers, row0, R), never the kernel's argument block by
// reference: a kernel is then compiled as if the text stood in it.  Left to the inliner's order, mlp_train_fwd_kernel came out at
// 140 VGPRs (3 waves per SIMD) instead of 116 (4), and with the block captured by reference its layer-2 loop unrolled by 4, not 8.
#pragma once
#include "mlp_device.h"

namespace simple_mlp {
constexpr int H1 = 256, H2 = 32;
constexpr int H1P = H1 + 4;   // LDS pitch of the h1 tile (bank spread for the 8 rows a wave reads at once)
}  // namespace simple_mlp

__host__ __device__ inline int x_pitch(int D) { return (D + 3) / 4 * 4 + 4; }   // LDS pitch of the x tile: 16-byte rows

// the two ReLU forms in use.  torch.relu keeps NaN; fmaxf turns a NaN into 0
__device__ inline float relu_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ inline float relu_fmax(float v) { return fmaxf(v, 0.f); }

// x tile: rows row0 .. row0 + TR - 1 into xs[TR][x_pitch(D)]; rows at or past `rows` are zeros.  FRAMES: row g is row g % S of
// frame g / S.  Otherwise x is one flat matrix of rows ld_row apart: the same case with one frame (dmlp_fwd_kernel trains that way,
// S = R), stated without its division per element for the SimpleMLP training kernel.
template <int TR, bool FRAMES>
__device__ __forceinline__ void load_x_tile(float* xs, const float* x, int ld_row, long long ld_frame, int S, int D, int row0, int rows) {
  const int DP = x_pitch(D);
  for (int i = threadIdx.x; i < TR * D; i += 256) {
    const int r = i / D, k = i - r * D, g = row0 + r;
    float v = 0.f;
    if (g < rows) {
      if constexpr (FRAMES) {
        const int b = g / S, s = g - b * S;
        v = x[b * ld_frame + (long long)s * ld_row + k];
      } else {
        v = x[(size_t)g * ld_row + k];
      }
    }
    xs[r * DP + k] = v;
  }
}

// layer 1: h1 = relu(W1 x + b1) on a tile of 2 RPT rows.  thread -> columns n0, n0 + 1, rows RPT rh .. + RPT - 1 (a wave shares
// rh: x reads broadcast).  put(r, n0, v0, v1) takes the two finished values of tile row r.
template <int RPT, float (*RELU)(float), typename Put>
__device__ __forceinline__ void smlp_layer1(const float* P, size_t oW1, size_t ob1, int D, const float* xs, Put put) {
  const int tid = threadIdx.x, DP = x_pitch(D);
  const int n0 = (tid & 127) * 2, rh = tid >> 7;
  const float* w0 = P + oW1 + (size_t)n0 * D;
  const float* w1 = w0 + D;
  float a0[RPT], a1[RPT];
  const float b0 = P[ob1 + n0], b1 = P[ob1 + n0 + 1];
#pragma unroll
  for (int r = 0; r < RPT; ++r) { a0[r] = b0; a1[r] = b1; }
  const float* xr = xs + (RPT * rh) * DP;
  for (int k = 0; k + 1 < D; k += 2) {
    const float wa0 = w0[k], wa1 = w0[k + 1], wb0 = w1[k], wb1 = w1[k + 1];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const float x0 = xr[r * DP + k], x1 = xr[r * DP + k + 1];
      a0[r] = fmaf(x1, wa1, fmaf(x0, wa0, a0[r]));
      a1[r] = fmaf(x1, wb1, fmaf(x0, wb0, a1[r]));
    }
  }
  if (D & 1) {
    const int k = D - 1;
    const float wa0 = w0[k], wb0 = w1[k];
#pragma unroll
    for (int r = 0; r < RPT; ++r) { a0[r] = fmaf(xr[r * DP + k], wa0, a0[r]); a1[r] = fmaf(xr[r * DP + k], wb0, a1[r]); }
  }
#pragma unroll
  for (int r = 0; r < RPT; ++r) put(RPT * rh + r, n0, RELU(a0[r]), RELU(a1[r]));
}

// layer 2: h2 = relu(W2 h1 + b2) on a tile of 8 RPT rows, h1s [.][H1P].  thread -> column j, rows RPT rg .. + RPT - 1.
// put(r, j, v) takes the finished value of tile row r.
template <int RPT, float (*RELU)(float), typename Put>
__device__ __forceinline__ void smlp_layer2(const float* P, size_t oW2, size_t ob2, const float* h1s, Put put) {
  using namespace simple_mlp;
  const int tid = threadIdx.x, j = tid & 31, rg = tid >> 5;
  const float* w = P + oW2 + (size_t)j * H1;
  float a[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r) a[r] = P[ob2 + j];
  for (int k = 0; k < H1; k += 4) {
    const f32x4_t w4 = *(const f32x4_t*)(w + k);
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const f32x4_t h4 = *(const f32x4_t*)(h1s + (RPT * rg + r) * H1P + k);
      a[r] = fmaf(h4[3], w4[3], fmaf(h4[2], w4[2], fmaf(h4[1], w4[1], fmaf(h4[0], w4[0], a[r]))));
    }
  }
#pragma unroll
  for (int r = 0; r < RPT; ++r) put(RPT * rg + r, j, RELU(a[r]));
}

// layer 3: out = W3 h2 + b3 on a tile of TR rows, h2s [TR][H2].  thread -> columns n = tid, tid + 256, ... (ascending), the 32
// weights of a column in registers.  visit(r, n, a) takes the value of tile row r, column n, in front of any sigmoid.
// UNROLL_ROWS: the row loop is unrolled (the visitor keeps per-row registers) or left to the compiler.
template <int TR, bool UNROLL_ROWS, typename Visit>
__device__ __forceinline__ void smlp_layer3(const float* P, size_t oW3, size_t ob3, int D, const float* h2s, Visit visit) {
  using namespace simple_mlp;
  for (int n = threadIdx.x; n <= D; n += 256) {
    float w[H2];
#pragma unroll
    for (int j = 0; j < H2; j += 4) {
      const f32x4_t w4 = *(const f32x4_t*)(P + oW3 + (size_t)n * H2 + j);
      w[j] = w4[0]; w[j + 1] = w4[1]; w[j + 2] = w4[2]; w[j + 3] = w4[3];
    }
    const float b = P[ob3 + n];
    auto row = [&](int r) {
      float a = b;
#pragma unroll
      for (int j = 0; j < H2; ++j) a = fmaf(h2s[r * H2 + j], w[j], a);
      visit(r, n, a);
    };
    if constexpr (UNROLL_ROWS) {
#pragma unroll
      for (int r = 0; r < TR; ++r) row(r);
    } else {
      for (int r = 0; r < TR; ++r) row(r);
    }
  }
}

// sum of the 256 partials part[r][0 .. 255] of tile row r = tid >> 4 (16 rows): lane q = tid & 15 adds partials q, q + 16, ... in
// order, then a butterfly; every lane of the row gets the total
__device__ __forceinline__ float row_sum_256(const float* part) {
  const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += part[r * 256 + q + 16 * i];
  s += __shfl_xor(s, 8, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 1, 64);
  return s;
}

// one row {trav, conf, loss, 0} of the per-segment table (one 16-byte write); conf_dev: optional {mean, std, std_factor} in device
// memory, which overrides the three scalars
template <float (*CONF)(float, float, float, float)>
__device__ __forceinline__ void table_row_write(float* row, float trav, float loss, const float* conf_dev, float mean, float std, float std_factor) {
  const float cm = conf_dev ? conf_dev[0] : mean, cs = conf_dev ? conf_dev[1] : std;
  const float cf = conf_dev ? conf_dev[2] : std_factor;
  *(f32x4_t*)row = f32x4_t{trav, CONF(loss, cm, cs, cf), loss, 0.f};
}
