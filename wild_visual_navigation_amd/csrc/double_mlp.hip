// DoubleMLP (wild_visual_navigation/model/double_mlp.py): two independent three-layer networks that share only the input,
//     networks.0 : D -> h1 -> ReLU -> h2 -> ReLU -> 1 -> sigmoid        (traversability, column 0 of the output)
//     networks.1 : D -> h1 -> ReLU -> h2 -> ReLU -> D                   (reconstruction, columns 1 .. D)
// on ONE flat fp32 parameter buffer [W1a|b1a|W2a|b2a|W3a|b3a|W1b|b1b|W2b|b2b|W3b|b3b] (a = networks.0, b = networks.1, Wi in Linear
// layout).  Three kernels, each over row tiles of TR rows, serve the forward, the training step and the per-segment prediction:
//     dmlp_fwd_kernel   : x tile -> both h1 (ONE pass over x: the 2 h1 first-layer columns of the pair form one product) -> both h2 ->
//                         out, the per-row reconstruction loss and, for the fused step, the statistic {n_lab, sum, sum^2, R}: the last
//                         tile to arrive folds the per-tile partials in tile order (mlp_train_device.h: stat_publish_fold, shared
//                         with mlp_train.hip).  The same kernel fills the per-segment table {trav, conf, loss, 0} of
//                         segment_predict.hip's paint kernel; the x-tile load, the row sum of the loss partials and the table
//                         write are the text of that file's table kernel (mlp_tile_device.h).  The pair layers are this file's.
//     dmlp_bwd_kernel   : gradient seed (mlp_train_device.h: seed_tile, shared with mlp_train.hip), dL/dh2 and dL/dh1 of both
//                         networks (ReLU masks), per-tile loss sums (mlp_train_device.h)
//     weight gradients  : mlp_train.hip's table-driven kernel (wvn_train_wgrad_launch) on the six matrices of the pair; this
//                         file only fills the table
// With Adam (mlp.hip) the fused step is FOUR launches, as the fused SimpleMLP step.  The general path (any h1, h2 <= 256, any row
// count) runs the same forward and data-path kernels with the stage kernels of mlp.hip and the split-K GEMMs of gemm_f32.hip around
// them (api.hip).  fp32 operands, fp32 FMA chains in one fixed order per output, fp64 statistics: a row's results depend on its
// features and the parameters only, and a step is bit-reproducible.
// Under TraversabilityLoss the two networks decouple: column 0 of the gradient seed reaches networks.0 only, columns 1 .. D reach
// networks.1 only; the reconstruction loss of networks.1 still sets the confidence that weights the loss of networks.0.
#include "common.h"
#include "mlp_train_device.h"

namespace {

constexpr int TR = 16;       // rows per workgroup
constexpr int HMAX = 256, DMAX = 1024;
constexpr int FUSED_H1 = 64, FUSED_H2 = 32, FUSED_RMAX = 2048;

size_t fwd_lds(const DmlpGeom& g) {
  return ((size_t)TR * x_pitch(g.D) + (size_t)TR * 2 * g.H1 + (size_t)TR * 2 * g.H2 + (size_t)TR * 256 + 2 * TR) * sizeof(float);
}
size_t bwd_lds(const DmlpGeom& g) { return ((size_t)TR * (g.D + 1) + (size_t)TR * 2 * g.H2 + 2 * TR) * sizeof(float); }
size_t fwd_lds_max() { return fwd_lds(wvn_dmlp_geom(DMAX, HMAX, HMAX)); }
size_t bwd_lds_max() { return bwd_lds(wvn_dmlp_geom(DMAX, HMAX, HMAX)); }

// ---------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------
// one layer of the pair on the tile: out[r][c] = relu(b[c] + sum_k in[r][net(c) * in_off + k] * W_net(c)[c'][k]) for the 2 * N columns
// of both networks.  A work item is (column, row half): 8 accumulators, one ascending FMA chain each.  relu_nan: a NaN feature row
// of the per-segment table must not turn into a finite prediction.
__device__ inline void pair_layer(const float* __restrict__ P, size_t oWa, size_t oWb, size_t oba, size_t obb, int N, int K,
                                  const float* __restrict__ in, int in_pitch, int in_off, float* __restrict__ outs, int tid) {
  const int N2 = 2 * N;
  for (int item = tid; item < 2 * N2; item += 256) {
    const int rh = item / N2, c = item - rh * N2;
    const int net = c >= N, cc = c - net * N;
    const float* w = P + (net ? oWb : oWa) + (size_t)cc * K;
    const float b = P[(net ? obb : oba) + cc];
    const float* xr = in + (size_t)(8 * rh) * in_pitch + net * in_off;
    float a[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) a[r] = b;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const float wk = w[k];
#pragma unroll
      for (int r = 0; r < 8; ++r) a[r] = fmaf(xr[r * in_pitch + k], wk, a[r]);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) outs[(8 * rh + r) * N2 + c] = relu_nan(a[r]);
  }
}

__global__ __launch_bounds__(256) void dmlp_fwd_kernel(DmlpArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const DmlpGeom& g = p.g;
  const int D = g.D, H1 = g.H1, H2 = g.H2, O = D + 1, DP = x_pitch(D), N1 = 2 * H1, N2 = 2 * H2;
  float* xs = sm;                      // [TR][DP]
  float* h1s = xs + TR * DP;           // [TR][2 H1]   networks.0 | networks.1
  float* h2s = h1s + TR * N1;          // [TR][2 H2]
  float* part = h2s + TR * N2;         // [TR][256] per-thread squared-error partials
  float* trav_s = part + TR * 256;     // [TR]
  float* lr_s = trav_s + TR;           // [TR]
  const int tid = threadIdx.x, row0 = blockIdx.x * TR;
  const int Rr = real_rows(p);
  // ---- x tile (rows past R / past the device-side count: zeros) ----
  load_x_tile<TR, true>(xs, p.x, p.ld_row, p.ld_frame, p.S, D, row0, Rr);
  __syncthreads();
  pair_layer(p.P, g.W1[0], g.W1[1], g.b1[0], g.b1[1], H1, D, xs, DP, 0, h1s, tid);
  __syncthreads();
  pair_layer(p.P, g.W2[0], g.W2[1], g.b2[0], g.b2[1], H2, H1, h1s, N1, H1, h2s, tid);
  __syncthreads();
  if (p.h1) {   // training: the activations of the tile for the backward pass
    for (int i = tid; i < TR * N1; i += 256) {
      const int r = i / N1;
      if (row0 + r < p.R) p.h1[(size_t)row0 * N1 + i] = h1s[i];
    }
    for (int i = tid; i < TR * N2; i += 256) {
      const int r = i / N2;
      if (row0 + r < p.R) p.h2[(size_t)row0 * N2 + i] = h2s[i];
    }
  }
  // ---- layer 3 + reconstruction error.  thread -> output columns n = tid, tid + 256, ... (ascending); column 0 is networks.0 ----
  {
    float s[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r) s[r] = 0.f;
    for (int n = tid; n < O; n += 256) {
      const int net = n > 0;
      const float* w = p.P + (net ? g.W3[1] + (size_t)(n - 1) * H2 : g.W3[0]);
      const float b = p.P[net ? g.b3[1] + (n - 1) : g.b3[0]];
      const float* hr = h2s + net * H2;
      float a[TR];
#pragma unroll
      for (int r = 0; r < TR; ++r) a[r] = b;
#pragma unroll 4
      for (int k = 0; k < H2; ++k) {
        const float wk = w[k];
#pragma unroll
        for (int r = 0; r < TR; ++r) a[r] = fmaf(hr[r * N2 + k], wk, a[r]);
      }
#pragma unroll
      for (int r = 0; r < TR; ++r) {
        float v = a[r];
        if (n == 0) {
          v = sigmoid_f(v);
          trav_s[r] = v;
        } else {
          const float e = v - xs[r * DP + n - 1];
          s[r] = fmaf(e, e, s[r]);
        }
        if (p.out && row0 + r < p.R) p.out[(size_t)(row0 + r) * O + n] = v;
      }
    }
#pragma unroll
    for (int r = 0; r < TR; ++r) part[r * 256 + tid] = s[r];
  }
  __syncthreads();
  {
    const int r = tid >> 4, q = tid & 15, row = row0 + r;
    const float loss = row_sum_256(part) / (float)D;
    if (q == 0) {
      const float lr = row < Rr ? loss : 0.f;
      lr_s[r] = lr;
      if (p.lr && row < p.R) p.lr[row] = lr;
      // confidence_of_nan: a NaN loss keeps a NaN confidence (seg_table_kernel writes confidence_of)
      if (p.table && row < p.R)
        table_row_write<confidence_of_nan>(p.table + (size_t)row * 4, trav_s[r], loss, p.conf_dev, p.mean, p.std, p.std_factor);
    }
  }
  if (!p.part) return;   // (uniform) no statistic asked for: inference, the table, the general training path
  __syncthreads();
  if (tid < 64) stat_publish_fold<TR>(p, lr_s, row0, Rr);
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, data path
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dmlp_bwd_kernel(DmlpArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const DmlpGeom& g = p.g;
  const int D = g.D, H1 = g.H1, H2 = g.H2, O = D + 1, N1 = 2 * H1, N2 = 2 * H2;
  float* gos = sm;                     // [TR][O]   gradient seed of the tile
  float* gh2s = gos + TR * O;          // [TR][2 H2]
  float* tw = gh2s + TR * N2;          // [TR] trav_w, [TR] trav_raw
  const int tid = threadIdx.x, row0 = blockIdx.x * TR;
  const int Rr = real_rows(p);
  if (p.seed_given) {   // general path: the seed was formed by mlp.hip's gradout kernel (zero rows behind the device-side count)
    for (int i = tid; i < TR * O; i += 256) {
      const int r = i / O;
      gos[i] = row0 + r < p.R ? p.g_out[(size_t)row0 * O + i] : 0.f;
    }
  } else {
    seed_tile<256 / TR>(p, D, row0, Rr, gos, tw);   // 16 lanes per row
  }
  __syncthreads();
  if (!p.seed_given && tid < 64) loss_sums_partial<TR>(p, tw);
  // ---- g_h2 of both networks, masked by h2 > 0: networks.0 from seed column 0 (W3a [1][H2]), networks.1 from columns 1 .. D (W3b [D][H2]) ----
  for (int item = tid; item < TR * N2; item += 256) {
    const int r = item / N2, c = item - r * N2, row = row0 + r;
    const int net = c >= H2, j = c - net * H2;
    float a = 0.f;
    if (net) {
      const float* w = p.P + g.W3[1] + j;
      const float* gr = gos + r * O + 1;
#pragma unroll 8
      for (int n = 0; n < D; ++n) a = fmaf(gr[n], w[(size_t)n * H2], a);
    } else {
      a = gos[r * O] * p.P[g.W3[0] + j];
    }
    const float m = row < p.R ? p.h2[(size_t)row * N2 + c] : 0.f;
    const float v = m > 0.f ? a : 0.f;
    gh2s[item] = v;
    if (row < p.R) p.g_h2[(size_t)row * N2 + c] = v;
  }
  __syncthreads();
  // ---- g_h1 of both networks, masked by h1 > 0; W2 [H2][H1] ----
  for (int item = tid; item < TR * N1; item += 256) {
    const int r = item / N1, c = item - r * N1, row = row0 + r;
    if (row >= p.R) continue;
    const int net = c >= H1, i = c - net * H1;
    const float* w = p.P + g.W2[net] + i;
    const float* gr = gh2s + r * N2 + net * H2;
    float a = 0.f;
#pragma unroll 8
    for (int j = 0; j < H2; ++j) a = fmaf(gr[j], w[(size_t)j * H1], a);
    const float m = p.h1[(size_t)row * N1 + c];
    p.g_h1[(size_t)row * N1 + c] = m > 0.f ? a : 0.f;
  }
}

int opt_in() {
  static LdsOptIn lds_opt_in;   // the largest geometry needs more than 64 KB of dynamic LDS (common.h)
  const int bytes = (int)(fwd_lds_max() > bwd_lds_max() ? fwd_lds_max() : bwd_lds_max());
  return lds_opt_in(bytes, (const void*)dmlp_fwd_kernel, (const void*)dmlp_bwd_kernel);
}

}  // namespace

DmlpGeom wvn_dmlp_geom(int D, int H1, int H2) {
  DmlpGeom g{};
  g.D = D; g.H1 = H1; g.H2 = H2;
  size_t off = 0;
  for (int net = 0; net < 2; ++net) {
    const int O = net ? D : 1;
    g.W1[net] = off; off += (size_t)H1 * D;
    g.b1[net] = off; off += H1;
    g.W2[net] = off; off += (size_t)H2 * H1;
    g.b2[net] = off; off += H2;
    g.W3[net] = off; off += (size_t)O * H2;
    g.b3[net] = off; off += O;
  }
  g.total = off;
  return g;
}

bool wvn_dmlp_supported(int D, int H1, int H2) { return D >= 1 && D <= DMAX && H1 >= 1 && H1 <= HMAX && H2 >= 1 && H2 <= HMAX; }
int wvn_dmlp_row_tile() { return TR; }
// the four-launch step: the default hidden geometry, at most 2048 rows (the wgrad launch walks the rows without split-K)
bool wvn_dmlp_fused_ok(int D, int H1, int H2, int R) {
  return wvn_dmlp_supported(D, H1, H2) && H1 == FUSED_H1 && H2 == FUSED_H2 && R > 0 && R <= FUSED_RMAX;
}

int wvn_dmlp_fwd_launch(const DmlpArgs& p, hipStream_t st) {
  if (!wvn_dmlp_supported(p.g.D, p.g.H1, p.g.H2) || p.R <= 0 || p.S <= 0) return WVN_ERR_ARG;
  if (const int rc = opt_in()) return rc;
  if (p.part) {
    if (!p.ticket || !p.stats || !p.valid) return WVN_ERR_ARG;
    // the arrival counter is zeroed on the stream in front of every launch, as in mlp_train.hip
    if (const hipError_t e = hipMemsetAsync(p.ticket, 0, sizeof(unsigned), st); e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(dmlp_fwd_kernel, dim3(ceil_div(p.R, TR)), dim3(256), fwd_lds(p.g), st, p);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_dmlp_bwd_launch(const DmlpArgs& p, hipStream_t st) {
  if (!wvn_dmlp_supported(p.g.D, p.g.H1, p.g.H2) || p.R <= 0) return WVN_ERR_ARG;
  if (const int rc = opt_in()) return rc;
  hipLaunchKernelGGL(dmlp_bwd_kernel, dim3(ceil_div(p.R, TR)), dim3(256), bwd_lds(p.g), st, p);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_dmlp_wgrad_launch(const DmlpArgs& p, hipStream_t st) {
  const DmlpGeom& g = p.g;
  const int D = g.D, H1 = g.H1, H2 = g.H2, O = D + 1, N1 = 2 * H1, N2 = 2 * H2;
  WTable tab{};
  tab.n = 6;
  for (int net = 0; net < 2; ++net) {
    const int M3 = net ? D : 1;
    tab.t[3 * net + 0] = WTile{p.g_out + net, O, p.h2 + net * H2, N2, M3, H2, p.grads + g.W3[net], p.grads + g.b3[net]};
    tab.t[3 * net + 1] = WTile{p.g_h2 + net * H2, N2, p.h1 + net * H1, N1, H2, H1, p.grads + g.W2[net], p.grads + g.b2[net]};
    tab.t[3 * net + 2] = WTile{p.g_h1 + net * H1, N1, p.x, p.ld_row, H1, D, p.grads + g.W1[net], p.grads + g.b1[net]};
  }
  return wvn_train_wgrad_launch(tab, p.rows_dev, p.R, p.part, ceil_div(p.R, TR), p.grads + g.total, st);
}
