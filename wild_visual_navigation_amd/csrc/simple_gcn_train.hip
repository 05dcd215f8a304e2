// One optimisation step of SimpleGCN in the three phases of the MLP step (mlp_train.hip), on the graph kernels of simple_gcn.hip.
//
// With Z_l = A X_{l-1} W_l^T + b_l and G_l = dL/dZ_l (A[i][j] = sum of coef_e over the edges j -> i; NOT symmetric for a directed
// edge list, so the backward runs on A^T):
//     T_l = A^T G_l,   dW_l = T_l^T X_{l-1},   db_l = column sums of G_l,   G_{l-1} = (T_l W_l) masked by X_{l-1} > 0
// (the T_l^T X_{l-1} form of the weight gradient: T_l is needed for the input gradient anyway, the forward saves no gathered tile).
//
// Phase A (wvn_gcn_train_phase_a_launch), 11 launches:
//     the target-major graph {rowptr, src, coef} of simple_gcn.hip (4)
//     its transpose, the source-major form {colptr, dst, coef} with every source's targets in ASCENDING order and each edge's
//     coefficient carried with it (4): gcn_t_count (int32 atomics: a count has one value whatever the order) -> gcn_scan_rows
//     (the self loop into slot 0) -> gcn_t_fill (slots handed out by an int32 atomic) -> gcn_t_sort (one wave per source ranks its
//     targets: the arrival order is gone; equal (j, i) duplicates have equal coefficients)
//     layers 1 and 2 of the inference forward with h1, h2 kept (2), gcn_train_last_kernel (1): the last layer of the table form
//     with its tile in LDS, the row's reconstruction loss in the table form's summation order, `out` and the row losses kept, and the
//     statistic published through stat_publish_fold<16> (mlp_train_device.h).
// Phase B (wvn_gcn_train_phase_b_launch), 5 launches behind the clearing of grads:
//     gcn_seed_kernel      G_3 (seed_tile: mlp_train_device.h), confidence_out, the loss-sum partials
//     gcn_back_kernel x 3  l = 3, 2, 1: gather T_l = A^T G_l of 16 rows into LDS (one ascending FMA chain over the source's targets
//                          per value), keep T_l, and for l > 1 the tile product with W_l read along its other axis (one ascending
//                          FMA chain over m per value) and the ReLU mask
//     gcn_wgrad_kernel     every dW_l (32 x 32 tiles, rows in ONE ascending order, no split) and db_l, and the fold of the loss sums
//                          into grads[n], grads[n + 1]
// Phase C is wvn_mlp_train_phase_c(_conf).  fp32 FMA throughout, no floating-point atomics: a step is bitwise reproducible and does
// not depend on the order of the edges.  No launch count depends on N or E, and nothing is read on the host.
#include "mlp_train_device.h"
#include "simple_gcn_device.h"

namespace {

// ---- the transposed graph ------------------------------------------------------------------------------------------------------
// one wave per target row i: every entry j != i of the row is one more target of source j
__global__ __launch_bounds__(64 * ROW_WAVES) void gcn_t_count(const int* __restrict__ rowptr, const int* __restrict__ src, int* __restrict__ cnt, int N) {
  const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const int e1 = rowptr[row + 1];
  for (int e = rowptr[row] + lane; e < e1; e += 64) {
    const int j = src[e];   // in [0, N): written by the graph preparation
    if (j != row) atomicAdd(cnt + j, 1);
  }
}

// the same walk: entry (j -> row, c) into a free slot of source j (slot 0 of a source is its self loop: gcn_scan_rows)
__global__ __launch_bounds__(64 * ROW_WAVES) void gcn_t_fill(const int* __restrict__ rowptr, const int* __restrict__ src, const float* __restrict__ coef,
                                                            const int* __restrict__ colptr, int* __restrict__ next, int* __restrict__ slots,
                                                            float* __restrict__ slot_coef, int N) {
  const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const int e1 = rowptr[row + 1];
  for (int e = rowptr[row] + lane; e < e1; e += 64) {
    const int j = src[e];
    const float c = coef[e];
    if (j == row) {
      slot_coef[colptr[row]] = c;
    } else {
      const int s = colptr[j] + atomicAdd(next + j, 1);   // < colptr[j + 1]: gcn_t_count counted this entry
      slots[s] = row;
      slot_coef[s] = c;
    }
  }
}

// one wave per source: its targets by rank, each with its coefficient
__global__ __launch_bounds__(64 * ROW_WAVES) void gcn_t_sort(const int* __restrict__ colptr, const int* __restrict__ slots, const float* __restrict__ slot_coef,
                                                            int* __restrict__ dst, float* __restrict__ coef, int N) {
  const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const int beg = colptr[row], n = colptr[row + 1] - beg;
  for (int e = lane; e < n; e += 64) {
    const int v = slots[beg + e];
    int rank = 0;
    for (int f = 0; f < n; ++f) {
      const int u = slots[beg + f];
      rank += (u < v || (u == v && f < e)) ? 1 : 0;
    }
    dst[beg + rank] = v;
    coef[beg + rank] = slot_coef[beg + e];
  }
}

// ---- phase A: the last layer ---------------------------------------------------------------------------------------------------
// gcn_layer_kernel<true, true>'s arithmetic (the same gather, tile product and row loss), with `out` and the row losses kept and the
// statistic of the step published
__global__ __launch_bounds__(256) void gcn_train_last_kernel(LayerParams p, TrainArgs t) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int K = p.K, M = p.M, KP = x_pitch(K), MP = out_pitch(M), N = p.N;
  float* xs = sm;                  // [TR][KP]
  float* os = xs + TR * KP;        // [TR][MP]
  float* lrs = os + TR * MP;       // [TR] the tile's row losses
  const int tid = threadIdx.x, row0 = blockIdx.x * TR;
  gather_tile(xs, KP, K, p.rowptr, p.src, p.coef, p.x, p.ldx, row0, N);
  __syncthreads();
  float* out = p.out;
  const int ldo = p.ldo;
  tile_linear_by_width(p.W, p.b, K, M, xs, [=](int r, int m, float v) {
    if (m == 0) v = sigmoid_f(v);
    os[r * MP + m] = v;
    if (row0 + r < N) out[(size_t)(row0 + r) * ldo + m] = v;
  });
  __syncthreads();
  {
    const int r = tid >> 4, q = tid & 15, g = row0 + r, D = M - 1;
    float s = 0.f;
    if (g < N)
      for (int k = q; k < D; k += 16) {
        const float e = os[r * MP + 1 + k] - p.x0[(size_t)g * p.ldx0 + k];
        s = fmaf(e, e, s);
      }
    s += __shfl_xor(s, 8, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 1, 64);
    const float lr = g < N ? s / (float)D : 0.f;
    if (q == 0) {
      lrs[r] = lr;
      if (g < N) t.lr[g] = lr;
    }
  }
  __syncthreads();
  if (tid < 64) stat_publish_fold<TR>(t, lrs, row0, N);
}

// ---- phase B --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gcn_seed_kernel(TrainArgs t, int D) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* gos = sm;                      // [TR][1 + D]
  float* tw = gos + TR * (D + 1);       // [TR] trav_w, [TR] trav_raw
  seed_tile<256 / TR>(t, D, blockIdx.x * TR, t.R, gos, tw);
  __syncthreads();
  if (threadIdx.x < 64) loss_sums_partial<TR>(t, tw);
}

struct BackParams {
  const int* colptr; const int* dst; const float* coef; int N;   // the source-major graph
  const float* G; int M;                                         // G_l [N][M]
  float* T;                                                      // T_l = A^T G_l [N][M]
  const float* W; int K;                                         // W_l [M][K]; nullptr (layer 1): no input gradient
  const float* X;                                                // X_{l-1} [N][K], the ReLU mask
  float* Gprev;                                                  // G_{l-1} [N][K]
};

// out[r][k] = sum_m ts[r][m] W[m][k], one ascending FMA chain per value; the forward's thread split with the columns k of W along
// the lanes (consecutive lanes read consecutive words of a row of W)
template <int RPT, typename Put>
__device__ __forceinline__ void tile_linear_t(const float* __restrict__ W, int K, int M, const float* ts, int MP, Put put) {
  constexpr int CL = 256 * RPT / TR;
  const int c = threadIdx.x % CL, g = threadIdx.x / CL;
  const float* tr = ts + g * RPT * MP;
  for (int k = c; k < K; k += CL) {
    float a[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) a[r] = 0.f;
    int m = 0;
    for (; m + 3 < M; m += 4) {
      const float* w = W + (size_t)m * K + k;
      const float w0 = w[0], w1 = w[K], w2 = w[2 * (size_t)K], w3 = w[3 * (size_t)K];
#pragma unroll
      for (int r = 0; r < RPT; ++r) {
        const f32x4_t t4 = *(const f32x4_t*)(tr + r * MP + m);
        a[r] = fmaf(t4[3], w3, fmaf(t4[2], w2, fmaf(t4[1], w1, fmaf(t4[0], w0, a[r]))));
      }
    }
    for (; m < M; ++m) {
      const float w0 = W[(size_t)m * K + k];
#pragma unroll
      for (int r = 0; r < RPT; ++r) a[r] = fmaf(tr[r * MP + m], w0, a[r]);
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) put(g * RPT + r, k, a[r]);
  }
}

__global__ __launch_bounds__(256) void gcn_back_kernel(BackParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int M = p.M, MP = x_pitch(M), N = p.N, K = p.K;
  float* ts = sm;                  // [TR][MP]: T_l of the tile's rows
  const int tid = threadIdx.x, row0 = blockIdx.x * TR;
  gather_tile(ts, MP, M, p.colptr, p.dst, p.coef, p.G, M, row0, N);
  __syncthreads();
  for (int i = tid; i < TR * M; i += 256) {
    const int r = i / M, m = i - r * M;
    if (row0 + r < N) p.T[(size_t)(row0 + r) * M + m] = ts[r * MP + m];
  }
  if (!p.W) return;
  const float* X = p.X;
  float* Gprev = p.Gprev;
  auto put = [=](int r, int k, float v) {
    if (row0 + r < N) {
      const size_t at = (size_t)(row0 + r) * K + k;
      Gprev[at] = X[at] > 0.f ? v : 0.f;
    }
  };
  if (K > 128) tile_linear_t<16>(p.W, K, M, ts, MP, put);
  else if (K > 64) tile_linear_t<8>(p.W, K, M, ts, MP, put);
  else if (K > 32) tile_linear_t<4>(p.W, K, M, ts, MP, put);
  else if (K > 16) tile_linear_t<2>(p.W, K, M, ts, MP, put);
  else tile_linear_t<1>(p.W, K, M, ts, MP, put);
}

// dW[m][k] = sum_i T[i][m] X[i][k] and db[m] = sum_i G[i][m], 32 x 32 output tiles, rows in ascending order (no split: one fixed
// order); the first column tile of a matrix forms the bias gradient; workgroup 0 folds the loss sums of the seed launch
struct GTile { const float* T; const float* G; int M; const float* X; int ldx; int K; float* dW; float* db; };
struct GTable { GTile t[3]; int first[4]; };

__global__ __launch_bounds__(256) void gcn_wgrad_kernel(GTable tab, int N, const double* part, int ntiles_rows, float* sums) {
  __shared__ float Ts[32][33], Xs[32][33], Gs[32][33];
  int l = 0;
  while (l < 2 && (int)blockIdx.x >= tab.first[l + 1]) ++l;
  const GTile w = tab.t[l];
  const int b = blockIdx.x - tab.first[l];
  const int ntk = (w.K + 31) / 32, tm = b / ntk, tk = b - tm * ntk;
  const int m0 = tm * 32, k0 = tk * 32;
  const int tid = threadIdx.x, lr_ = tid >> 5, lc = tid & 31;   // loader: row lr_ + 8 i, column lc
  const int om = tid >> 4, ok = (tid & 15) * 2;                 // outputs: rows om, om + 16; columns ok, ok + 1
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  float bsum = 0.f;                                             // tk == 0, tid < 32: sum_i G[i][m0 + tid]
  for (int r0 = 0; r0 < N; r0 += 32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + lr_ + 8 * i;
      const bool in_m = r < N && m0 + lc < w.M;
      Ts[lr_ + 8 * i][lc] = in_m ? w.T[(size_t)r * w.M + m0 + lc] : 0.f;
      Xs[lr_ + 8 * i][lc] = (r < N && k0 + lc < w.K) ? w.X[(size_t)r * w.ldx + k0 + lc] : 0.f;
      if (tk == 0) Gs[lr_ + 8 * i][lc] = in_m ? w.G[(size_t)r * w.M + m0 + lc] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 32; ++r) {
      const float g0 = Ts[r][om], g1 = Ts[r][om + 16], h0 = Xs[r][ok], h1 = Xs[r][ok + 1];
      acc[0][0] = fmaf(g0, h0, acc[0][0]); acc[0][1] = fmaf(g0, h1, acc[0][1]);
      acc[1][0] = fmaf(g1, h0, acc[1][0]); acc[1][1] = fmaf(g1, h1, acc[1][1]);
    }
    if (tk == 0 && tid < 32)
      for (int r = 0; r < 32; ++r) bsum += Gs[r][tid];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) {
      const int m = m0 + om + 16 * i, k = k0 + ok + jn;
      if (m < w.M && k < w.K) w.dW[(size_t)m * w.K + k] = acc[i][jn];
    }
  if (tk == 0 && tid < 32 && m0 + tid < w.M) w.db[m0 + tid] = bsum;
  if (blockIdx.x == 0 && tid == 0) {   // the loss sums of the seed launch, tiles in ascending order
    double a = 0, c = 0;
    for (int i = 0; i < ntiles_rows; ++i) { a += part[(size_t)i * 4]; c += part[(size_t)i * 4 + 1]; }
    sums[0] = (float)a;
    sums[1] = (float)c;
  }
}

size_t last_lds(int h2, int O) { return ((size_t)TR * x_pitch(h2) + (size_t)TR * out_pitch(O) + TR) * sizeof(float); }
size_t seed_lds(int D) { return ((size_t)TR * (D + 1) + 2 * TR) * sizeof(float); }
size_t back_lds(int M) { return (size_t)TR * x_pitch(M) * sizeof(float); }

int opt_in() {
  static LdsOptIn lds_opt_in;   // D = 1024: 81 KB (last layer), 65 KB (seed, backward of layer 3)
  return lds_opt_in((int)last_lds(HMAX, 1 + DMAX), (const void*)gcn_train_last_kernel, (const void*)gcn_seed_kernel, (const void*)gcn_back_kernel);
}

// the training workspace: the inference workspace (graph, h1, h2, table), then the transposed graph, the kept forward values, the
// gradients G_l and their gathered forms T_l, the per-tile partials
struct GcnTrainWs {
  GcnWs f;
  int *colptr, *colcnt, *tslots, *dst;
  float *slot_coef, *tcoef, *out, *lr, *g3, *t3, *g2, *t2, *g1, *t1;
  void* scratch;
  size_t total;
};
GcnTrainWs carve_train(void* base, int D, int h1, int h2, int N, long long cap) {
  GcnTrainWs w{};
  w.f = carve(base, h1, h2, N, cap);
  size_t o = w.f.total;
  const size_t O = 1 + (size_t)D, n = (size_t)N;
  auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return (char*)base + at; };
  w.colptr = (int*)take((n + 1) * sizeof(int));
  w.colcnt = (int*)take(n * sizeof(int));
  w.tslots = (int*)take((size_t)cap * sizeof(int));
  w.dst = (int*)take((size_t)cap * sizeof(int));
  w.slot_coef = (float*)take((size_t)cap * sizeof(float));
  w.tcoef = (float*)take((size_t)cap * sizeof(float));
  w.out = (float*)take(n * O * sizeof(float));
  w.lr = (float*)take(n * sizeof(float));
  w.g3 = (float*)take(n * O * sizeof(float));
  w.t3 = (float*)take(n * O * sizeof(float));
  w.g2 = (float*)take(n * h2 * sizeof(float));
  w.t2 = (float*)take(n * h2 * sizeof(float));
  w.g1 = (float*)take(n * h1 * sizeof(float));
  w.t1 = (float*)take(n * h1 * sizeof(float));
  w.scratch = take(wvn_train_scratch_bytes(N, TR));
  w.total = o;
  return w;
}

void train_args(TrainArgs& a, const GcnTrainWs& w, const float* x, int ldx, const unsigned char* valid, int N, const double* stats,
                const ConfArgs& conf) {
  a.x = x; a.ld_row = ldx; a.R = N; a.valid = valid; a.stats = (double*)stats;
  a.out = w.out; a.lr = w.lr; a.g_out = w.g3;
  a.method = conf.method; a.balanced = conf.balanced; a.cstate = conf.state; a.minmax = conf.minmax;
  wvn_train_scratch_carve(w.scratch, N, TR, &a.part, &a.part_mm);
}

}  // namespace

size_t wvn_gcn_train_workspace_bytes_impl(int D, int h1, int h2, int N, long long cap) { return carve_train(nullptr, D, h1, h2, N, cap).total; }

void wvn_gcn_train_saved_offsets(int D, int h1, int h2, int N, long long cap, size_t offs[3]) {
  const GcnTrainWs w = carve_train(nullptr, D, h1, h2, N, cap);
  offs[0] = (size_t)(uintptr_t)w.f.h1;
  offs[1] = (size_t)(uintptr_t)w.f.h2;
  offs[2] = (size_t)(uintptr_t)w.out;
}

int wvn_gcn_train_phase_a_launch(int D, int h1, int h2, const float* params, const float* x, int ldx, const long long* ei, long long ld_row,
                                 long long ld_e, int E, const unsigned char* valid, int N, long long cap, double* stats, int* bad, void* ws,
                                 unsigned* ticket, const ConfArgs& conf, hipStream_t st) {
  // (every argument is checked by the caller, csrc/api.hip: cap >= E + N bounds every slot the graph kernels write)
  const GcnTrainWs w = carve_train(ws, D, h1, h2, N, cap);
  if (const int rc = opt_in()) return rc;
  if (const int rc = wvn_gcn_graph_edges_launch(ei, ld_row, ld_e, E, N, cap, bad, ws, st)) return rc;
  // ---- the transposed graph ----
  if (const hipError_t e = hipMemsetAsync(w.colcnt, 0, (size_t)N * sizeof(int), st); e != hipSuccess) return (int)e;
  const dim3 rows(ceil_div(N, ROW_WAVES)), wave_rows(64 * ROW_WAVES);
  hipLaunchKernelGGL(gcn_t_count, rows, wave_rows, 0, st, w.f.rowptr, w.f.src, w.colcnt, N);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(gcn_scan_rows, dim3(1), dim3(1024), 0, st, w.colcnt, w.colptr, w.tslots, N);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(gcn_t_fill, rows, wave_rows, 0, st, w.f.rowptr, w.f.src, w.f.coef, w.colptr, w.colcnt, w.tslots, w.slot_coef, N);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(gcn_t_sort, rows, wave_rows, 0, st, w.colptr, w.tslots, w.slot_coef, w.dst, w.tcoef, N);
  WVN_LAUNCH_CHECK();
  // ---- the forward ----
  if (const int rc = wvn_gcn_hidden_layers_launch(D, h1, h2, params, x, ldx, N, cap, ws, st)) return rc;
  const int O = 1 + D;
  const float* W3 = params + (size_t)h1 * D + h1 + (size_t)h2 * h1 + h2;
  LayerParams p{};
  p.rowptr = w.f.rowptr; p.src = w.f.src; p.coef = w.f.coef; p.N = N;
  p.W = W3; p.b = W3 + (size_t)O * h2; p.K = h2; p.M = O; p.x = w.f.h2; p.ldx = h2; p.out = w.out; p.ldo = O;
  p.x0 = x; p.ldx0 = ldx;
  TrainArgs t{};
  train_args(t, w, x, ldx, valid, N, stats, conf);
  t.ticket = ticket;
  // the arrival counter is zeroed on the stream in front of the launch (as in mlp_train.hip)
  if (const hipError_t e = hipMemsetAsync(ticket, 0, sizeof(unsigned), st); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(gcn_train_last_kernel, dim3(ceil_div(N, TR)), dim3(256), last_lds(h2, O), st, p, t);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_gcn_train_phase_b_launch(int D, int h1, int h2, const float* params, const float* x, int ldx, const float* y,
                                 const unsigned char* valid, int N, long long cap, const double* stats, float std_factor, float w_trav,
                                 float w_reco, float* grads, float* conf_out, void* ws, const ConfArgs& conf, hipStream_t st) {
  const GcnTrainWs w = carve_train(ws, D, h1, h2, N, cap);
  if (const int rc = opt_in()) return rc;
  const int O = 1 + D, ntiles = ceil_div(N, TR);
  const size_t oW1 = 0, ob1 = oW1 + (size_t)h1 * D, oW2 = ob1 + h1, ob2 = oW2 + (size_t)h2 * h1, oW3 = ob2 + h2, ob3 = oW3 + (size_t)O * h2,
               total = ob3 + O;
  if (const hipError_t e = hipMemsetAsync(grads, 0, (total + 2) * sizeof(float), st); e != hipSuccess) return (int)e;
  TrainArgs t{};
  train_args(t, w, x, ldx, valid, N, stats, conf);
  t.y = y; t.std_factor = std_factor; t.w_trav = w_trav; t.w_reco = w_reco; t.conf_out = conf_out; t.grads = grads;
  hipLaunchKernelGGL(gcn_seed_kernel, dim3(ntiles), dim3(256), seed_lds(D), st, t, D);
  WVN_LAUNCH_CHECK();
  BackParams b{};
  b.colptr = w.colptr; b.dst = w.dst; b.coef = w.tcoef; b.N = N;
  b.G = w.g3; b.M = O; b.T = w.t3; b.W = params + oW3; b.K = h2; b.X = w.f.h2; b.Gprev = w.g2;
  hipLaunchKernelGGL(gcn_back_kernel, dim3(ntiles), dim3(256), back_lds(O), st, b);
  WVN_LAUNCH_CHECK();
  b.G = w.g2; b.M = h2; b.T = w.t2; b.W = params + oW2; b.K = h1; b.X = w.f.h1; b.Gprev = w.g1;
  hipLaunchKernelGGL(gcn_back_kernel, dim3(ntiles), dim3(256), back_lds(h2), st, b);
  WVN_LAUNCH_CHECK();
  b.G = w.g1; b.M = h1; b.T = w.t1; b.W = nullptr; b.K = 0; b.X = nullptr; b.Gprev = nullptr;
  hipLaunchKernelGGL(gcn_back_kernel, dim3(ntiles), dim3(256), back_lds(h1), st, b);
  WVN_LAUNCH_CHECK();
  GTable tab{};
  tab.t[0] = GTile{w.t3, w.g3, O, w.f.h2, h2, h2, grads + oW3, grads + ob3};
  tab.t[1] = GTile{w.t2, w.g2, h2, w.f.h1, h1, h1, grads + oW2, grads + ob2};
  tab.t[2] = GTile{w.t1, w.g1, h1, x, ldx, D, grads + oW1, grads + ob1};
  tab.first[0] = 0;
  for (int l = 0; l < 3; ++l) tab.first[l + 1] = tab.first[l] + ceil_div(tab.t[l].M, 32) * ceil_div(tab.t[l].K, 32);
  hipLaunchKernelGGL(gcn_wgrad_kernel, dim3(tab.first[3]), dim3(256), 0, st, tab, N, t.part, ntiles, grads + total);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
