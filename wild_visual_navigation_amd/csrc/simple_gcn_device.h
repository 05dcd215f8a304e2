// The pieces the SimpleGCN inference kernels (simple_gcn.hip) and the training step (simple_gcn_train.hip) share: the tile
// geometry, the row-pointer scan of the graph preparation, the gather of a 16-row tile through one form of the graph (target-major
// {rowptr, src, coef} in the forward, source-major {colptr, dst, coef} in the backward), the tile product of the forward with its
// column / row split, and the layout of the workspace both units address.  Everything sits in an unnamed namespace: each unit
// compiles its own copy, as if the text stood in it.
#pragma once
#include "common.h"
#include "mlp_tile_device.h"
#include "wvn_internal.h"

namespace {

constexpr int TR = 16;            // rows per layer workgroup
constexpr int DMAX = 1024, HMAX = 256;
constexpr int TCOLS = 4;          // table row: trav, conf, loss, (pad)
constexpr int ROW_WAVES = 4;      // rows (one wave each) per workgroup of the row-wise graph kernels

__device__ inline float dinv_sqrt(int deg) { return 1.0f / sqrtf((float)deg); }

// single workgroup: rowptr = exclusive sums of cnt[i] + 1 (the self loop).  self_slots != nullptr (edge lists, and the transposed
// graph): node i goes into slot 0 of its row there and cnt[i] becomes the next free slot of the row, 1.
__global__ __launch_bounds__(1024) void gcn_scan_rows(int* __restrict__ cnt, int* __restrict__ rowptr, int* __restrict__ self_slots, int N) {
  __shared__ int part[1024];
  const int per = (N + 1023) / 1024;
  const int beg = min(N, (int)threadIdx.x * per), end = min(N, beg + per);
  int c = 0;
  for (int i = beg; i < end; ++i) c += cnt[i] + 1;
  part[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < 1024; ++t) { const int v = part[t]; part[t] = run; run += v; }
    rowptr[N] = run;
  }
  __syncthreads();
  int o = part[threadIdx.x];
  for (int i = beg; i < end; ++i) {
    rowptr[i] = o;
    const int d = cnt[i] + 1;
    if (self_slots) { self_slots[o] = i; cnt[i] = 1; }
    o += d;
  }
}

// ---- one layer ----------------------------------------------------------------------------------------------------------
struct LayerParams {
  const float* W; const float* b; int K, M;     // W [M][K], b [M]
  const float* x; int ldx;                      // the layer's input rows [N][ldx]
  const int* rowptr; const int* src; const float* coef;
  int N;
  float* out; int ldo;                          // [N][ldo]; may be NULL in the table form
  // the table form of the last layer
  const float* x0; int ldx0;                    // the network's input rows (the reconstruction target), M = 1 + D
  float* table; float mean, std, std_factor; const float* conf_dev;
};

__host__ __device__ inline int out_pitch(int M) { return (M + 3) / 4 * 4 + 4; }

// xs[r][k] = sum over the entries e of graph row row0 + r of coef[e] x[idx[e]][k], one ascending fp32 FMA chain per value (rows
// past N: zeros).  xs [TR][KP]
__device__ __forceinline__ void gather_tile(float* xs, int KP, int K, const int* ptr, const int* idx, const float* coef, const float* x, int ldx,
                                            int row0, int N) {
  for (int i = threadIdx.x; i < TR * K; i += 256) {
    const int r = i / K, k = i - r * K, g = row0 + r;
    float a = 0.f;
    if (g < N) {
      const int e1 = ptr[g + 1];
      for (int e = ptr[g]; e < e1; ++e) a = fmaf(coef[e], x[(size_t)idx[e] * ldx + k], a);
    }
    xs[r * KP + k] = a;
  }
}

// out[r][m] = b[m] + sum_k xs[r][k] W[m][k], one ascending FMA chain per value.  thread -> column lane c of 256 RPT / TR, rows
// RPT g .. + RPT - 1: narrow layers spread their rows over the threads a wide one spends on columns.
template <int RPT, typename Put>
__device__ __forceinline__ void tile_linear(const float* __restrict__ W, const float* __restrict__ bias, int K, int M, const float* xs, Put put) {
  constexpr int CL = 256 * RPT / TR;
  const int c = threadIdx.x % CL, g = threadIdx.x / CL, KP = x_pitch(K);
  const float* xr = xs + g * RPT * KP;
  for (int m = c; m < M; m += CL) {
    const float* w = W + (size_t)m * K;
    float a[RPT];
    const float bm = bias[m];
#pragma unroll
    for (int r = 0; r < RPT; ++r) a[r] = bm;
    int k = 0;
    for (; k + 3 < K; k += 4) {
      const float w0 = w[k], w1 = w[k + 1], w2 = w[k + 2], w3 = w[k + 3];
#pragma unroll
      for (int r = 0; r < RPT; ++r) {
        const f32x4_t x4 = *(const f32x4_t*)(xr + r * KP + k);
        a[r] = fmaf(x4[3], w3, fmaf(x4[2], w2, fmaf(x4[1], w1, fmaf(x4[0], w0, a[r]))));
      }
    }
    for (; k < K; ++k) {
      const float w0 = w[k];
#pragma unroll
      for (int r = 0; r < RPT; ++r) a[r] = fmaf(xr[r * KP + k], w0, a[r]);
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) put(g * RPT + r, m, a[r]);
  }
}

// the forward's split of a tile product by the layer's width
template <typename Put>
__device__ __forceinline__ void tile_linear_by_width(const float* W, const float* bias, int K, int M, const float* xs, Put put) {
  if (M > 128) tile_linear<16>(W, bias, K, M, xs, put);
  else if (M > 64) tile_linear<8>(W, bias, K, M, xs, put);
  else if (M > 32) tile_linear<4>(W, bias, K, M, xs, put);
  else if (M > 16) tile_linear<2>(W, bias, K, M, xs, put);
  else tile_linear<1>(W, bias, K, M, xs, put);
}

// the workspace: the graph first (its layout needs N and cap only), the activations behind it
struct GcnWs { int *rowptr, *cnt, *slots, *src; float *coef, *h1, *h2, *table; size_t total; };
inline GcnWs carve(void* base, int h1, int h2, int N, long long cap) {
  GcnWs w{};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return (char*)base + at; };
  w.rowptr = (int*)take(((size_t)N + 1) * sizeof(int));
  w.cnt = (int*)take((size_t)N * sizeof(int));
  w.slots = (int*)take((size_t)cap * sizeof(int));
  w.src = (int*)take((size_t)cap * sizeof(int));
  w.coef = (float*)take((size_t)cap * sizeof(float));
  w.h1 = (float*)take((size_t)N * h1 * sizeof(float));
  w.h2 = (float*)take((size_t)N * h2 * sizeof(float));
  w.table = (float*)take((size_t)N * TCOLS * sizeof(float));
  w.total = o;
  return w;
}

}  // namespace
