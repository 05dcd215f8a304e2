// SimpleGCN: three graph-convolution layers D -> h1 (ReLU) -> h2 (ReLU) -> 1 + D (sigmoid on column 0), each one GCNConv with
// torch_geometric's defaults (self loops added, symmetric normalisation, aggregation "add", flow source -> target):
//
//   edges with j == i dropped, one self loop per node added;  deg_i = edges into i (>= 1);  coef_e = deg_j^-1/2 deg_i^-1/2
//   out_i = sum_{e: j -> i} coef_e (x_j W^T) + b
//
// Graph preparation (no host reads) builds the target-major form {rowptr [N + 1], src [nnz], coef [nnz]} with every row's sources
// in ASCENDING order, the self loop among them:
//   from an edge list  : gcn_count_edges (int32 atomics: a count has one value whatever the order) -> gcn_scan_rows (row
//                        pointers; the self loop goes into slot 0 of its row) -> gcn_fill_edges (slots handed out by an int32
//                        atomic: any order) -> gcn_sort_rows (one wave per row ranks the row's sources: the arrival order is gone)
//   from [B][S][S] maps: gcn_count_bits -> gcn_scan_rows -> gcn_fill_bits (one wave per target row walks its sources in ascending
//                        order through a ballot: no sort needed)
// An edge with an endpoint outside [0, N) is counted in *bad and skipped by the same predicate in both edge kernels.
//
// A layer is ONE launch (gcn_layer_kernel): aggregation commutes with the linear map, A (X W^T) = (A X) W^T, so a workgroup
// gathers sum_e coef_e x_src(e) of its TR target rows into LDS (one ascending fp32 FMA chain over the row's neighbours per value)
// and runs the tile product with W, the bias and the activation on that tile (one ascending FMA chain over k from the bias per
// value).  Only the neighbours a row HAS are read -- a NaN row reaches the rows within one hop per layer and no others -- and no
// value depends on the row's position, its tile neighbours, the edge order or N: bit-reproducible, no floating-point atomics.
// The last layer can keep its tile in LDS, form the row's reconstruction loss against the row's own features (16 lanes per row,
// strided ascending partials + a butterfly) and write the {trav, conf, loss_reco, 0} table that seg_paint_kernel
// (segment_predict.hip) spreads onto the segment maps.
// The tile geometry, gcn_scan_rows, the gather, the tile product and the workspace layout are in simple_gcn_device.h: the training
// step (simple_gcn_train.hip) runs the same text on the transposed graph.
#include "simple_gcn_device.h"

namespace {

// ---- graph preparation -------------------------------------------------------------------------------------------------
struct EdgeList { const long long* ei; long long ld_row, ld_e; int E, N; };   // element (row, e) at ei[row * ld_row + e * ld_e]

// 1: a counted edge j -> i; 0: a self loop (dropped); -1: an endpoint outside [0, N) (dropped and counted)
__device__ inline int edge_kind(const EdgeList& g, int e, int& j, int& i) {
  const long long jj = g.ei[(long long)e * g.ld_e], ii = g.ei[g.ld_row + (long long)e * g.ld_e];
  if (jj < 0 || jj >= g.N || ii < 0 || ii >= g.N) return -1;
  j = (int)jj; i = (int)ii;
  return j != i;
}

__global__ __launch_bounds__(256) void gcn_count_edges(EdgeList g, int* __restrict__ cnt, int* __restrict__ bad) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= g.E) return;
  int j, i;
  const int kind = edge_kind(g, e, j, i);
  if (kind > 0) atomicAdd(cnt + i, 1);
  else if (kind < 0) atomicAdd(bad, 1);
}

__global__ __launch_bounds__(256) void gcn_fill_edges(EdgeList g, const int* __restrict__ rowptr, int* __restrict__ next, int* __restrict__ slots) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= g.E) return;
  int j, i;
  if (edge_kind(g, e, j, i) > 0) slots[rowptr[i] + atomicAdd(next + i, 1)] = j;   // < rowptr[i + 1]: gcn_count_edges counted this edge
}

// one wave per target row: the row's sources by rank (equal sources are interchangeable) and their coefficients
__global__ __launch_bounds__(64 * ROW_WAVES) void gcn_sort_rows(const int* __restrict__ rowptr, const int* __restrict__ slots, int* __restrict__ src,
                                                               float* __restrict__ coef, int N) {
  const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const int beg = rowptr[row], n = rowptr[row + 1] - beg;
  const float di = dinv_sqrt(n);
  for (int e = lane; e < n; e += 64) {
    const int v = slots[beg + e];
    int rank = 0;
    for (int f = 0; f < n; ++f) {
      const int u = slots[beg + f];
      rank += (u < v || (u == v && f < e)) ? 1 : 0;
    }
    src[beg + rank] = v;
    coef[beg + rank] = dinv_sqrt(rowptr[v + 1] - rowptr[v]) * di;
  }
}

struct BitMaps { const unsigned char* adj; long long ld_b, ld_l, ld_r; int B, S; };   // adj[b][l][r] != 0: an edge l -> r of frame b

__global__ __launch_bounds__(64 * ROW_WAVES) void gcn_count_bits(BitMaps g, int* __restrict__ cnt) {
  const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= g.B * g.S) return;
  const int b = row / g.S, r = row - b * g.S;
  const unsigned char* a = g.adj + b * g.ld_b + r * g.ld_r;
  int c = 0;
  for (int l0 = 0; l0 < g.S; l0 += 64) {
    const int l = l0 + lane;
    const bool on = l < g.S && l != r && a[l * g.ld_l] != 0;
    c += __popcll(__ballot(on));
  }
  if (lane == 0) cnt[row] = c;
}

__global__ __launch_bounds__(64 * ROW_WAVES) void gcn_fill_bits(BitMaps g, const int* __restrict__ rowptr, int* __restrict__ src, float* __restrict__ coef) {
  const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= g.B * g.S) return;
  const int b = row / g.S, r = row - b * g.S;
  const unsigned char* a = g.adj + b * g.ld_b + r * g.ld_r;
  int o = rowptr[row];
  const float di = dinv_sqrt(rowptr[row + 1] - o);
  for (int l0 = 0; l0 < g.S; l0 += 64) {
    const int l = l0 + lane;
    const bool on = l < g.S && (l == r || a[l * g.ld_l] != 0);
    const unsigned long long m = __ballot(on);
    if (on) {
      const int pos = o + __popcll(m & ((1ull << lane) - 1ull)), j = b * g.S + l;
      src[pos] = j;
      coef[pos] = dinv_sqrt(rowptr[j + 1] - rowptr[j]) * di;
    }
    o += __popcll(m);
  }
}

// ---- one layer (LayerParams, gather_tile, tile_linear: simple_gcn_device.h) ---------------------------------------------------
// LAST: sigmoid on column 0, no ReLU.  TABLE (LAST only): the tile stays in LDS for the row loss and the table row.
template <bool LAST, bool TABLE>
__global__ __launch_bounds__(256) void gcn_layer_kernel(LayerParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int K = p.K, M = p.M, KP = x_pitch(K), MP = out_pitch(M), N = p.N;
  float* xs = sm;                  // [TR][KP]: the aggregated inputs of the tile's rows
  float* os = xs + TR * KP;        // [TR][MP] (TABLE)
  const int tid = threadIdx.x, row0 = blockIdx.x * TR;
  // ---- gather: xs[r][k] = sum over the neighbours of row r, ascending source (rows past N: zeros, never written out) ----
  gather_tile(xs, KP, K, p.rowptr, p.src, p.coef, p.x, p.ldx, row0, N);
  __syncthreads();
  // ---- the tile product, bias and activation ----
  float* out = p.out;
  const int ldo = p.ldo;
  auto put = [=](int r, int m, float v) {
    if (LAST) { if (m == 0) v = sigmoid_f(v); }
    else v = relu_nan(v);             // torch.relu keeps NaN
    if (TABLE) os[r * MP + m] = v;
    if (out && row0 + r < N) out[(size_t)(row0 + r) * ldo + m] = v;
  };
  tile_linear_by_width(p.W, p.b, K, M, xs, put);
  if (TABLE) {
    __syncthreads();
    // ---- reconstruction loss of row r against its own features: lane q adds columns q, q + 16, ... in order, then a butterfly ----
    const int r = tid >> 4, q = tid & 15, g = row0 + r, D = M - 1;
    float s = 0.f;
    if (g < N)
      for (int k = q; k < D; k += 16) {
        const float e = os[r * MP + 1 + k] - p.x0[(size_t)g * p.ldx0 + k];
        s = fmaf(e, e, s);
      }
    s += __shfl_xor(s, 8, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 1, 64);
    if (q == 0 && g < N)
      table_row_write<confidence_of>(p.table + (size_t)g * TCOLS, os[r * MP], s / (float)D, p.conf_dev, p.mean, p.std, p.std_factor);
  }
}

size_t layer_lds_bytes(int K, int M, bool table) { return ((size_t)TR * x_pitch(K) + (table ? (size_t)TR * out_pitch(M) : 0)) * sizeof(float); }

}  // namespace

bool wvn_gcn_supported(int D, int h1, int h2) { return D >= 1 && D <= DMAX && h1 >= 1 && h1 <= HMAX && h2 >= 1 && h2 <= HMAX; }

size_t wvn_gcn_workspace_bytes_impl(int h1, int h2, int N, long long cap) { return carve(nullptr, h1, h2, N, cap).total; }

int wvn_gcn_graph_edges_launch(const long long* ei, long long ld_row, long long ld_e, int E, int N, long long cap, int* bad, void* ws,
                               hipStream_t st) {
  // (every argument is checked by the caller, csrc/api.hip: cap >= E + N bounds every slot the kernels write)
  const GcnWs w = carve(ws, 0, 0, N, cap);
  const EdgeList g{ei, ld_row, ld_e, E, N};
  hipError_t e = hipMemsetAsync(w.cnt, 0, (size_t)N * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (E > 0) {
    hipLaunchKernelGGL(gcn_count_edges, dim3(ceil_div(E, 256)), dim3(256), 0, st, g, w.cnt, bad);
    WVN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gcn_scan_rows, dim3(1), dim3(1024), 0, st, w.cnt, w.rowptr, w.slots, N);
  WVN_LAUNCH_CHECK();
  if (E > 0) {
    hipLaunchKernelGGL(gcn_fill_edges, dim3(ceil_div(E, 256)), dim3(256), 0, st, g, w.rowptr, w.cnt, w.slots);
    WVN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gcn_sort_rows, dim3(ceil_div(N, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, st, w.rowptr, w.slots, w.src, w.coef, N);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_gcn_graph_bitmaps_launch(const unsigned char* adj, long long ld_b, long long ld_l, long long ld_r, int B, int S, long long cap,
                                 int* bad, void* ws, hipStream_t st) {
  // (cap >= B * S * S, checked by the caller: a row holds at most S sources)
  const int N = B * S;
  const GcnWs w = carve(ws, 0, 0, N, cap);
  const BitMaps g{adj, ld_b, ld_l, ld_r, B, S};
  if (bad) {   // a map has no edge that leaves its frame
    const hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(gcn_count_bits, dim3(ceil_div(N, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, st, g, w.cnt);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(gcn_scan_rows, dim3(1), dim3(1024), 0, st, w.cnt, w.rowptr, (int*)nullptr, N);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(gcn_fill_bits, dim3(ceil_div(N, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, st, g, w.rowptr, w.src, w.coef);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

// the hidden layers x -> h1 -> h2 into the workspace: the first two launches of every forward, the training step's included
int wvn_gcn_hidden_layers_launch(int D, int h1, int h2, const float* params, const float* x, int ldx, int N, long long cap, void* ws,
                                 hipStream_t st) {
  const GcnWs w = carve(ws, h1, h2, N, cap);
  // flat parameters [W1|b1|W2|b2|W3|b3]: SimpleMLP's layout for the same (D, h1, h2)
  const float* W1 = params; const float* b1 = W1 + (size_t)h1 * D;
  const float* W2 = b1 + h1; const float* b2 = W2 + (size_t)h2 * h1;
  static LdsOptIn lds_opt_in;   // D = 1024 needs more than 64 KB: opted in once per device for the largest geometry (common.h)
  const size_t lds_a = layer_lds_bytes(DMAX, HMAX, false), lds_b = layer_lds_bytes(HMAX, 1 + DMAX, true);
  const int lds_max = (int)(lds_a > lds_b ? lds_a : lds_b);
  if (const int rc = lds_opt_in(lds_max, (const void*)gcn_layer_kernel<false, false>, (const void*)gcn_layer_kernel<true, false>,
                                (const void*)gcn_layer_kernel<true, true>))
    return rc;
  LayerParams p{};
  p.rowptr = w.rowptr; p.src = w.src; p.coef = w.coef; p.N = N;
  const dim3 grid(ceil_div(N, TR));
  p.W = W1; p.b = b1; p.K = D; p.M = h1; p.x = x; p.ldx = ldx; p.out = w.h1; p.ldo = h1;
  hipLaunchKernelGGL((gcn_layer_kernel<false, false>), grid, dim3(256), layer_lds_bytes(D, h1, false), st, p);
  WVN_LAUNCH_CHECK();
  p.W = W2; p.b = b2; p.K = h1; p.M = h2; p.x = w.h1; p.ldx = h1; p.out = w.h2; p.ldo = h2;
  hipLaunchKernelGGL((gcn_layer_kernel<false, false>), grid, dim3(256), layer_lds_bytes(h1, h2, false), st, p);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_gcn_layers_launch(int D, int h1, int h2, const float* params, const float* x, int ldx, int N, long long cap, float* out, int ldo,
                          int want_table, float mean, float std, float std_factor, const float* conf_state, void* ws, hipStream_t st) {
  if (const int rc = wvn_gcn_hidden_layers_launch(D, h1, h2, params, x, ldx, N, cap, ws, st)) return rc;   // (opts the kernels in)
  const GcnWs w = carve(ws, h1, h2, N, cap);
  const int O = 1 + D;
  const float* W3 = params + (size_t)h1 * D + h1 + (size_t)h2 * h1 + h2; const float* b3 = W3 + (size_t)O * h2;
  LayerParams p{};
  p.rowptr = w.rowptr; p.src = w.src; p.coef = w.coef; p.N = N;
  const dim3 grid(ceil_div(N, TR));
  p.W = W3; p.b = b3; p.K = h2; p.M = O; p.x = w.h2; p.ldx = h2; p.out = out; p.ldo = ldo;
  if (want_table) {
    p.x0 = x; p.ldx0 = ldx; p.table = w.table;
    p.mean = mean; p.std = std; p.std_factor = std_factor; p.conf_dev = conf_state;
    hipLaunchKernelGGL((gcn_layer_kernel<true, true>), grid, dim3(256), layer_lds_bytes(h2, O, true), st, p);
  } else {
    hipLaunchKernelGGL((gcn_layer_kernel<true, false>), grid, dim3(256), layer_lds_bytes(h2, O, false), st, p);
  }
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

const float* wvn_gcn_table(void* ws, int h1, int h2, int N, long long cap) { return carve(ws, h1, h2, N, cap).table; }
