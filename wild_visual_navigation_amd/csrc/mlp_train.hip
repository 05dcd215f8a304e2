// One optimisation step of the online traversability MLP (SimpleMLP D -> 256 -> 32 -> 1 + D) in FOUR launches, for the batch sizes
// the learning node actually trains on (8 mission nodes x <= 100 segments = a few hundred rows, traversability_estimator.py:
// 432-446; bench.py: 1280 rows):
//     fwd   : x -> h1 -> h2 -> out (sigmoid on column 0), per-row reconstruction loss, LOCAL statistic {n_lab, sum, sum^2, R}
//             -- phase A of trainer.py; the multi-GPU statistics all-reduce sits behind it
//     bwd   : loss gradient seed, dL/dh2, dL/dh1 (ReLU masks), per-row loss terms               -- phase B, data path
//     wgrad : dW3, dW2, dW1 and the three bias gradients; the loss sums join the flat gradient    -- phase B, reductions
//             (the gradient all-reduce sits behind it)
//     adam  : Adam update + the step's losses                                                     -- phase C (mlp.hip)
// The general path (mlp.hip + gemm_f32.hip) spends 17-20 launches on the same step: at these sizes every one of them is a
// launch latency.  Same arithmetic (fp32 FMA, loss.py:93-160, confidence_generator.py:78-82,182-193), other summation orders:
// every reduction here has ONE fixed order (row tiles in ascending order, rows in ascending order inside a tile, fp64 for the
// statistics), so runs are bit-reproducible and replicas of a data-parallel job stay identical.
// A workgroup owns 32 consecutive rows through all layers; weights stream from L2 (478 KB for D = 384), activations of the
// tile live in LDS.
// Shared with the DoubleMLP step (double_mlp.hip): the argument block (wvn_internal.h: TrainArgs), the statistic's publish / fold
// the gradient-seed block and the loss-sum partial (mlp_train_device.h), and the weight-gradient kernel, which lives here and takes
// its matrices from a table (wvn_train_wgrad_launch).  The forward's x-tile load and its three layers are the text the per-segment
// table kernel (segment_predict.hip) runs too: mlp_tile_device.h.  Tile height, ReLU form, what is stored and the loss reduction
// are this kernel's.
#include "common.h"
#include "mlp_train_device.h"

namespace {

using namespace simple_mlp;   // H1, H2, H1P
constexpr int TR = 32;        // rows per workgroup

// ---------------------------------------------------------------------------------------------------------------------------
// fwd
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mlp_train_fwd_kernel(MlpTrainArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int D = p.D, O = D + 1, DP = x_pitch(D);
  float* xs = sm;                       // [TR][DP]
  float* h1s = xs + TR * DP;            // [TR][H1P]
  float* h2s = h1s + TR * H1P;          // [TR][H2]
  float* outs = h2s + TR * H2;          // [TR][O]
  const int tid = threadIdx.x, row0 = blockIdx.x * TR;
  const int Rr = real_rows(p);
  // ---- x tile (rows past R / past the device-side count: zeros); a flat [R][D] matrix ----
  load_x_tile<TR, false>(xs, p.x, p.ld_row, 0, p.R, D, row0, Rr);
  __syncthreads();
  // ---- layers 1 and 2, 16 and 4 rows per thread; the activations also go to HBM for the backward pass.
  //      relu_fmax: a NaN activation becomes 0 here (the table kernels keep it with relu_nan) ----
  float* const h1g = p.h1, * const h2g = p.h2, * const outg = p.out;
  const int R = p.R;
  smlp_layer1<TR / 2, relu_fmax>(p.P, p.o.W1, p.o.b1, D, xs, [=](int r, int n0, float v0, float v1) {
    h1s[r * H1P + n0] = v0;
    h1s[r * H1P + n0 + 1] = v1;
    if (row0 + r < R) *(float2*)(h1g + (size_t)(row0 + r) * H1 + n0) = float2{v0, v1};
  });
  __syncthreads();
  smlp_layer2<TR / 8, relu_fmax>(p.P, p.o.W2, p.o.b2, h1s, [=](int r, int j, float v) {
    h2s[r * H2 + j] = v;
    if (row0 + r < R) h2g[(size_t)(row0 + r) * H2 + j] = v;
  });
  __syncthreads();
  // ---- layer 3, sigmoid on column 0 ----
  smlp_layer3<TR, false>(p.P, p.o.W3, p.o.b3, D, h2s, [=](int r, int n, float a) {
    if (n == 0) a = sigmoid_f(a);
    outs[r * O + n] = a;
    if (row0 + r < R) outg[(size_t)(row0 + r) * O + n] = a;
  });
  __syncthreads();
  // ---- per-row reconstruction loss: 8 threads per row, fixed order ----
  {
    const int r = tid >> 3, q = tid & 7;
    float s = 0.f;
    for (int d = q; d < D; d += 8) {
      const float e = outs[r * O + 1 + d] - xs[r * DP + d];
      s = fmaf(e, e, s);
    }
    s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
    const float lr = (row0 + r < Rr) ? s / (float)D : 0.f;
    if (q == 0 && row0 + r < p.R) p.lr[row0 + r] = lr;
    if (q == 0) h2s[r] = lr;     // (h2s is dead: reuse as the tile's lr vector for the statistic)
  }
  __syncthreads();
  if (tid < 64) stat_publish_fold<TR>(p, h2s, row0, Rr);
}

// ---------------------------------------------------------------------------------------------------------------------------
// bwd (data path)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mlp_train_bwd_kernel(MlpTrainArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int D = p.D, O = D + 1;
  float* gos = sm;                     // [TR][O]   gradient seed of the tile
  float* gh2s = gos + TR * O;          // [TR][H2]
  float* tw = gh2s + TR * H2;          // [TR] trav_w, [TR] trav_raw
  const int tid = threadIdx.x, row0 = blockIdx.x * TR;
  const int Rr = real_rows(p);
  seed_tile<256 / TR>(p, D, row0, Rr, gos, tw);   // 8 lanes per row
  __syncthreads();
  if (tid < 64) loss_sums_partial<TR>(p, tw);
  // ---- g_h2 = (g_out W3) masked by h2 > 0.  thread -> row r, columns j0 .. j0 + 3; W3 [O][32] ----
  {
    const int r = tid >> 3, j0 = (tid & 7) * 4, row = row0 + r;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < O; ++n) {
      const f32x4_t w4 = *(const f32x4_t*)(p.P + p.o.W3 + (size_t)n * H2 + j0);
      const float g = gos[r * O + n];
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = fmaf(g, w4[e], a[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float m = row < p.R ? p.h2[(size_t)row * H2 + j0 + e] : 0.f;
      const float v = m > 0.f ? a[e] : 0.f;
      gh2s[r * H2 + j0 + e] = v;
      if (row < p.R) p.g_h2[(size_t)row * H2 + j0 + e] = v;
    }
  }
  __syncthreads();
  // ---- g_h1 = (g_h2 W2) masked by h1 > 0.  thread -> column i = tid, all 32 rows; W2 [32][256] ----
  {
    float w[H2];
#pragma unroll
    for (int j = 0; j < H2; ++j) w[j] = p.P[p.o.W2 + (size_t)j * H1 + tid];
    for (int r = 0; r < TR; ++r) {
      if (row0 + r >= p.R) break;
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < H2; ++j) a = fmaf(gh2s[r * H2 + j], w[j], a);
      const float m = p.h1[(size_t)(row0 + r) * H1 + tid];
      p.g_h1[(size_t)(row0 + r) * H1 + tid] = m > 0.f ? a : 0.f;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// wgrad: dW[m][n] = sum_r G[r][m] Hm[r][n], 32 x 32 output tiles, rows in ascending order (no split-K: one fixed order);
// the first column tile of every matrix also forms the bias gradient sum_r G[r][m]; workgroup 0 folds the loss sums
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mlp_train_wgrad_kernel(WTable tab, const int* rows_dev, int R, const double* part, int ntiles_rows,
                                                          float* sums) {
  __shared__ float Gs[32][33], Hs[32][33];
  int k = 0;
  while (k < tab.n - 1 && (int)blockIdx.x >= tab.first[k + 1]) ++k;
  const WTile w = tab.t[k];
  const int b = blockIdx.x - tab.first[k];
  const int ntn = (w.N + 31) / 32, tm = b / ntn, tn = b - tm * ntn;
  const int m0 = tm * 32, n0 = tn * 32;
  const int tid = threadIdx.x, lr_ = tid >> 5, lc = tid & 31;   // loader: row lr_ + 8 i, column lc
  const int om = tid >> 4, on = (tid & 15) * 2;                 // outputs: rows om, om + 16; columns on, on + 1
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  float bsum = 0.f;                                             // tn == 0, tid < 32: sum_r G[r][m0 + tid]
  const int Rr = rows_dev ? min(R, *rows_dev) : R;
  for (int r0 = 0; r0 < Rr; r0 += 32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + lr_ + 8 * i;
      Gs[lr_ + 8 * i][lc] = (r < Rr && m0 + lc < w.M) ? w.G[(size_t)r * w.ldg + m0 + lc] : 0.f;
      Hs[lr_ + 8 * i][lc] = (r < Rr && n0 + lc < w.N) ? w.Hm[(size_t)r * w.ldh + n0 + lc] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 32; ++r) {
      const float g0 = Gs[r][om], g1 = Gs[r][om + 16], h0 = Hs[r][on], h1 = Hs[r][on + 1];
      acc[0][0] = fmaf(g0, h0, acc[0][0]); acc[0][1] = fmaf(g0, h1, acc[0][1]);
      acc[1][0] = fmaf(g1, h0, acc[1][0]); acc[1][1] = fmaf(g1, h1, acc[1][1]);
    }
    if (tn == 0 && tid < 32)
      for (int r = 0; r < 32; ++r) bsum += Gs[r][tid];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) {
      const int m = m0 + om + 16 * i, n = n0 + on + jn;
      if (m < w.M && n < w.N) w.dW[(size_t)m * w.N + n] = acc[i][jn];
    }
  if (tn == 0 && tid < 32 && m0 + tid < w.M) w.db[m0 + tid] = bsum;
  if (blockIdx.x == 0 && tid == 0) {   // the loss sums of the bwd launch, tiles in ascending order
    double a = 0, c = 0;
    for (int i = 0; i < ntiles_rows; ++i) { a += part[(size_t)i * 4]; c += part[(size_t)i * 4 + 1]; }
    sums[0] = (float)a;
    sums[1] = (float)c;
  }
}

constexpr size_t FUSED_LDS_MAX = 156 * 1024;
size_t fwd_lds(int D) { return (size_t)(TR * x_pitch(D) + TR * H1P + TR * H2 + TR * (D + 1)) * sizeof(float); }
size_t bwd_lds(int D) { return (size_t)(TR * (D + 1) + TR * H2 + 2 * TR) * sizeof(float); }

}  // namespace

// Eligibility of the four-launch step: the SimpleMLP geometry (256, 32), any D whose row tiles fit the LDS (<= 460), at most 2048 rows (the wgrad
// launch walks the rows without split-K).
bool wvn_mlp_train_fused_ok(int D, int H1_, int H2_, int R) {
  // measured (MI355X, D = 384 / 90): 75 vs 152 us per step at 160 rows, 196 vs 312 at 800, 185 vs 251 at 1280; the un-split weight
  // gradients lose from about 3000 rows on (792 vs 504 us at 6400), where the general path's split-K GEMMs take over
  return H1_ == H1 && H2_ == H2 && D > 0 && fwd_lds(D) <= FUSED_LDS_MAX && R > 0 && R <= 2048;   // D <= 460
}
int wvn_mlp_train_row_tile() { return TR; }
// the scratch behind the MLP workspace: part [ceil(R / tile)][4] doubles, part_mm [ceil(R / tile)][2] floats
size_t wvn_train_scratch_bytes(int R, int tile) { return (size_t)ceil_div(R, tile) * (4 * sizeof(double) + 2 * sizeof(float)); }
void wvn_train_scratch_carve(void* scratch, int R, int tile, double** part, float** part_mm) {
  *part = (double*)scratch;
  *part_mm = (float*)(*part + (size_t)ceil_div(R, tile) * 4);
}

static int opt_in() {
  static LdsOptIn lds_opt_in;   // (the kernels also hold a few bytes of static LDS: the dynamic limit must stay below 160 KB)
  return lds_opt_in((int)FUSED_LDS_MAX, (const void*)mlp_train_fwd_kernel, (const void*)mlp_train_bwd_kernel);
}

int wvn_mlp_train_fwd_launch(const MlpTrainArgs& p, hipStream_t st) {
  if (fwd_lds(p.D) > FUSED_LDS_MAX) return WVN_ERR_ARG;
  if (const int rc = opt_in()) return rc;
  // the arrival counter is zeroed on the stream in front of every launch (a count left over by an aborted launch, or a
  // sync word the caller shares, would leave no tile "last" and the step would train on stale statistics without an error)
  if (const hipError_t e = hipMemsetAsync(p.ticket, 0, sizeof(unsigned), st); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(mlp_train_fwd_kernel, dim3(ceil_div(p.R, TR)), dim3(256), fwd_lds(p.D), st, p);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_mlp_train_bwd_launch(const MlpTrainArgs& p, hipStream_t st) {
  if (const int rc = opt_in()) return rc;
  const int ntiles = ceil_div(p.R, TR), D = p.D, O = D + 1;
  hipLaunchKernelGGL(mlp_train_bwd_kernel, dim3(ntiles), dim3(256), bwd_lds(D), st, p);
  WVN_LAUNCH_CHECK();
  WTable tab{};
  tab.n = 3;
  tab.t[0] = WTile{p.g_out, O, p.h2, H2, O, H2, p.grads + p.o.W3, p.grads + p.o.b3};
  tab.t[1] = WTile{p.g_h2, H2, p.h1, H1, H2, H1, p.grads + p.o.W2, p.grads + p.o.b2};
  tab.t[2] = WTile{p.g_h1, H1, p.x, p.ld_row, H1, D, p.grads + p.o.W1, p.grads + p.o.b1};
  return wvn_train_wgrad_launch(tab, p.rows_dev, p.R, p.part, ntiles, p.grads + p.o.total, st);
}

int wvn_train_wgrad_launch(WTable tab, const int* rows_dev, int R, const double* part, int ntiles_rows, float* sums, hipStream_t st) {
  tab.first[0] = 0;
  for (int k = 0; k < tab.n; ++k) tab.first[k + 1] = tab.first[k] + ceil_div(tab.t[k].M, 32) * ceil_div(tab.t[k].N, 32);
  hipLaunchKernelGGL(mlp_train_wgrad_kernel, dim3(tab.first[tab.n]), dim3(256), 0, st, tab, rows_dev, R, part, ntiles_rows, sums);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
