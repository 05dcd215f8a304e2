// DoubleMLP (wild_visual_navigation/model/double_mlp.py): two independent three-layer networks that share only the input,
//     networks.0 : D -> h1 -> ReLU -> h2 -> ReLU -> 1 -> sigmoid        (traversability, column 0 of the output)
//     networks.1 : D -> h1 -> ReLU -> h2 -> ReLU -> D                   (reconstruction, columns 1 .. D)
// on ONE flat fp32 parameter buffer [W1a|b1a|W2a|b2a|W3a|b3a|W1b|b1b|W2b|b2b|W3b|b3b] (a = networks.0, b = networks.1, Wi in Linear
// layout).  Three kernels, each over row tiles of TR rows, serve the forward, the training step and the per-segment prediction:
//     dmlp_fwd_kernel   : x tile -> both h1 (ONE pass over x: the 2 h1 first-layer columns of the pair form one product) -> both h2 ->
//                         out, the per-row reconstruction loss and, for the fused step, the statistic {n_lab, sum, sum^2, R}: the last
//                         tile to arrive folds the per-tile partials in tile order (the ticket of mlp_train.hip).  The same kernel
//                         fills the per-segment table {trav, conf, loss, 0} of segment_predict.hip's paint kernel.
//     dmlp_bwd_kernel   : gradient seed (loss.py:125-147), dL/dh2 and dL/dh1 of both networks (ReLU masks), per-tile loss sums
//     dmlp_wgrad_kernel : the six weight and six bias gradients, rows in ascending order (no split-K: one fixed order); workgroup 0
//                         folds the loss sums behind the flat gradient
// With Adam (mlp.hip) the fused step is FOUR launches, as the fused SimpleMLP step.  The general path (any h1, h2 <= 256, any row
// count) runs the same forward and data-path kernels with the stage kernels of mlp.hip and the split-K GEMMs of gemm_f32.hip around
// them (api.hip).  fp32 operands, fp32 FMA chains in one fixed order per output, fp64 statistics: a row's results depend on its
// features and the parameters only, and a step is bit-reproducible.
// Under TraversabilityLoss the two networks decouple: column 0 of the gradient seed reaches networks.0 only, columns 1 .. D reach
// networks.1 only; the reconstruction loss of networks.1 still sets the confidence that weights the loss of networks.0.
#include "common.h"
#include "mlp_device.h"
#include "wvn_internal.h"

namespace {

constexpr int TR = 16;       // rows per workgroup
constexpr int HMAX = 256, DMAX = 1024;
constexpr int FUSED_H1 = 64, FUSED_H2 = 32, FUSED_RMAX = 2048;

__host__ __device__ inline int x_pitch(int D) { return (D + 3) / 4 * 4 + 4; }
// torch.relu: NaN stays NaN (a NaN feature row of the per-segment table must not turn into a finite prediction)
__device__ inline float relu_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ inline int real_rows(const DmlpArgs& p) { return p.rows_dev ? min(p.R, *p.rows_dev) : p.R; }

// fixed-order sum over the 16 lanes 0..15: butterfly, every lane gets the total
__device__ inline double sum16_d(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

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
// of both networks.  A work item is (column, row half): 8 accumulators, one ascending FMA chain each.
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
  for (int i = tid; i < TR * D; i += 256) {
    const int r = i / D, k = i - r * D, gr = row0 + r;
    float v = 0.f;
    if (gr < Rr) {
      const int b = gr / p.S, s = gr - b * p.S;
      v = p.x[b * p.ld_frame + (long long)s * p.ld_row + k];
    }
    xs[r * DP + k] = v;
  }
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
  // ---- per-row sum of the 256 partials: 16 lanes per row, lane q adds partials q, q + 16, ... in order, then a butterfly ----
  {
    const int r = tid >> 4, q = tid & 15, row = row0 + r;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += part[r * 256 + q + 16 * i];
    s += __shfl_xor(s, 8, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 1, 64);
    const float loss = s / (float)D;
    if (q == 0) {
      const float lr = row < Rr ? loss : 0.f;
      lr_s[r] = lr;
      if (p.lr && row < p.R) p.lr[row] = lr;
      if (p.table && row < p.R) {
        const float cm = p.conf_dev ? p.conf_dev[0] : p.mean, cs = p.conf_dev ? p.conf_dev[1] : p.std;
        const float cf = p.conf_dev ? p.conf_dev[2] : p.std_factor;
        // (a NaN feature row: torch.clip keeps the NaN loss, fminf / fmaxf would drop it)
        const float conf = isnan(loss) ? NAN : confidence_of(loss, cm, cs, cf);
        *(f32x4_t*)(p.table + (size_t)row * 4) = f32x4_t{trav_s[r], conf, loss, 0.f};
      }
    }
  }
  if (!p.part) return;   // (uniform) no statistic asked for: inference, the table, the general training path
  __syncthreads();
  // ---- tile partial of the confidence statistic (fp64): rows in ascending order through a butterfly over the 16 rows ----
  if (tid < 64) {
    const bool real = tid < TR && row0 + tid < Rr;
    const bool v = real && p.valid[row0 + tid] != 0;
    const double l = v ? (double)lr_s[tid] : 0.0;
    const double n = sum16_d(v ? 1.0 : 0.0), s1 = sum16_d(l), s2 = sum16_d(l * l);
    float mn = INFINITY, mx = -INFINITY;
    if (p.minmax) {   // min / max of lr over the tile's real rows (moving_average; min and max are order-free)
      if (real) mn = mx = lr_s[tid];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
    }
    if (tid == 0) {
      double* d = p.part + (size_t)blockIdx.x * 4;
      d[0] = n; d[1] = s1; d[2] = s2;
      if (p.minmax) { p.part_mm[(size_t)blockIdx.x * 2] = mn; p.part_mm[(size_t)blockIdx.x * 2 + 1] = mx; }
      // publish: the partial must be visible device-wide before the ticket (the producer form of mlp_train.hip)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned t = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t == gridDim.x - 1) {   // the last tile to arrive folds the partials in ascending tile order
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        double a = 0, b = 0, c = 0;
        for (unsigned i = 0; i < gridDim.x; ++i) {
          const double* e = p.part + (size_t)i * 4;
          a += __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          b += __hip_atomic_load(e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          c += __hip_atomic_load(e + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        p.stats[0] = a; p.stats[1] = b; p.stats[2] = c; p.stats[3] = (double)Rr;
        if (p.minmax) {
          float lo = INFINITY, hi = -INFINITY;
          for (unsigned i = 0; i < gridDim.x; ++i) {
            lo = fminf(lo, __hip_atomic_load(p.part_mm + (size_t)i * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            hi = fmaxf(hi, __hip_atomic_load(p.part_mm + (size_t)i * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          }
          p.minmax[0] = hi; p.minmax[1] = -lo;
        }
        __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next step
      }
    }
  }
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
    // ---- gradient seed (loss.py:125-147): 16 threads per row ----
    const ConfStats cs = conf_stats(p.stats);
    const float Rtot = (float)p.stats[3], nv = (float)p.stats[0];
    ConfPost cp{};
    float xmin = 0.f, xmax = 0.f;
    if (p.cstate) {   // another method: the post-update statistic from the state and this step's (global) stats
      cp = conf_post(p.method, p.stats, p.cstate);
      if (p.minmax) { xmax = p.minmax[0]; xmin = -p.minmax[1]; }
    }
    const int r = tid >> 4, q = tid & 15, row = row0 + r;
    const bool real = row < Rr;
    const bool v = real && p.valid[row] != 0;
    float diff = 0.f, s = 0.f, wrow = 0.f, conf = 0.f;
    if (real) {
      conf = p.cstate ? conf_method(p.method, p.lr[row], cp, p.std_factor, xmin, xmax)
                      : confidence_of(p.lr[row], cs.mean, cs.std, p.std_factor);
      s = p.out[(size_t)row * O];
      diff = s - p.y[row];
      wrow = (v || !p.balanced) ? 1.f : (1.f - conf);   // anomaly_balanced = False: the plain mean of the raw trav loss
    }
    if (q == 0) {
      const float raw = diff * diff;
      tw[r] = real ? raw * wrow : 0.f;
      tw[TR + r] = real ? raw : 0.f;
      if (p.conf_out && row < p.R) p.conf_out[row] = conf;
      const float g0 = real ? (p.w_trav / Rtot) * wrow * 2.f * diff * s * (1.f - s) : 0.f;
      gos[r * O] = g0;
      if (row < p.R) p.g_out[(size_t)row * O] = g0;
    }
    const float cr = v ? (p.w_reco / (nv * (float)D)) * 2.f : 0.f;
    for (int d = q; d < D; d += 16) {
      const float gv = real ? cr * (p.out[(size_t)row * O + 1 + d] - p.x[(size_t)row * p.ld_row + d]) : 0.f;
      gos[r * O + 1 + d] = gv;
      if (row < p.R) p.g_out[(size_t)row * O + 1 + d] = gv;
    }
  }
  __syncthreads();
  // ---- tile partial of the loss sums (fp64, rows in ascending order through a butterfly) ----
  if (!p.seed_given && tid < 64) {
    const double a = sum16_d(tid < TR ? (double)tw[tid] : 0.0), b = sum16_d(tid < TR ? (double)tw[TR + tid] : 0.0);
    if (tid == 0) { p.part[(size_t)blockIdx.x * 4] = a; p.part[(size_t)blockIdx.x * 4 + 1] = b; }
  }
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

// ---------------------------------------------------------------------------------------------------------------------------
// wgrad: dW[m][n] = sum_r G[r][m] Hm[r][n] for the six matrices, 32 x 32 output tiles, rows in ascending order; the first column
// tile of every matrix also forms the bias gradient sum_r G[r][m]; workgroup 0 folds the loss sums
// ---------------------------------------------------------------------------------------------------------------------------
struct WTile { const float* G; int ldg; const float* Hm; int ldh; int M, N; float* dW; float* db; };
struct WTable { WTile t[6]; int first[7]; };

__global__ __launch_bounds__(256) void dmlp_wgrad_kernel(WTable tab, const int* rows_dev, int R, const double* part, int ntiles_rows,
                                                         float* sums) {
  __shared__ float Gs[32][33], Hs[32][33];
  int k = 0;
  while (k < 5 && (int)blockIdx.x >= tab.first[k + 1]) ++k;
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
size_t wvn_dmlp_scratch_bytes(int R) { return (size_t)ceil_div(R, TR) * (4 * sizeof(double) + 2 * sizeof(float)); }
void wvn_dmlp_scratch_carve(void* scratch, int R, double** part, float** part_mm) {
  *part = (double*)scratch;
  *part_mm = (float*)(*part + (size_t)ceil_div(R, TR) * 4);
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
  for (int net = 0; net < 2; ++net) {
    const int M3 = net ? D : 1;
    tab.t[3 * net + 0] = WTile{p.g_out + net, O, p.h2 + net * H2, N2, M3, H2, p.grads + g.W3[net], p.grads + g.b3[net]};
    tab.t[3 * net + 1] = WTile{p.g_h2 + net * H2, N2, p.h1 + net * H1, N1, H2, H1, p.grads + g.W2[net], p.grads + g.b2[net]};
    tab.t[3 * net + 2] = WTile{p.g_h1 + net * H1, N1, p.x, p.ld_row, H1, D, p.grads + g.W1[net], p.grads + g.b1[net]};
  }
  tab.first[0] = 0;
  for (int k = 0; k < 6; ++k) tab.first[k + 1] = tab.first[k] + ceil_div(tab.t[k].M, 32) * ceil_div(tab.t[k].N, 32);
  hipLaunchKernelGGL(dmlp_wgrad_kernel, dim3(tab.first[6]), dim3(256), 0, st, tab, p.rows_dev, p.R, p.part, ceil_div(p.R, TR),
                     p.grads + g.total);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
