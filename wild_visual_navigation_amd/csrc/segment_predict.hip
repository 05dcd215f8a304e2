// Fused per-segment traversability inference: the live node's per-frame path with prediction_per_pixel = False
// (wvn_feature_extractor_node.py:320-366, quick_start.py:184-210):
//
//   input_feat = feat[seg.reshape(-1)]                  [H*W, D] gather of the pooled segment features (308 MB/frame at 448^2)
//   prediction = SimpleMLP(input_feat)                  D -> 256 -> 32 -> 1+D on every pixel row (47.7 GFLOP/frame at D = 384)
//   trav = prediction[:, 0]; conf = confidence(mean((prediction[:, 1:] - input_feat)^2))
//
// Every pixel row is a copy of one of S segment rows, so the MLP runs once per segment and the results are painted:
//   seg_table_kernel : one row per segment -> a [B*S][4] table {trav, conf, loss, 0} in the workspace (nothing else reaches HBM).
//                      TR rows per workgroup staged in LDS, weights streamed from L2.  The x-tile load, the three layers, the
//                      row sum and the table write are the text mlp_train_fwd_kernel and dmlp_fwd_kernel run too
//                      (mlp_tile_device.h); the tile height, the ReLU form and the loss reduction are this kernel's.  Every
//                      dot product of a row is ONE fixed-order fp32 FMA chain and every reduction a fixed tree, the same for every
//                      row wherever it sits: a row's results depend on its features and the parameters only, never on B, S, the
//                      row's position or its workgroup neighbours (tests/test_gpu_segment_predict.py pins this bit for bit).
//   seg_paint_kernel : one pass over the segment maps: id -> table row -> trav / conf / loss_reco.  Bandwidth-bound: 16-byte id
//                      loads and output stores on 4-pixel quads, the frame's table in LDS when it fits, read through L2 otherwise.
// Id rule (torch indexing of feat[seg]): ids in [0, S) select their row, ids in [-S, 0) select row S + id (extract() with
// segmentation_type="random" leaves -1 ids that the reference's gather wraps to the last row), any other id gives NaN outputs.
#include "common.h"
#include "mlp_tile_device.h"
#include "wvn_internal.h"

namespace {

using namespace simple_mlp;       // H1, H2, H1P
constexpr int TR = 16;            // rows per table workgroup
constexpr int DMAX = 1024;
constexpr int TCOLS = 4;          // table row: trav, conf, loss, (pad) -- one 16-byte read per pixel
constexpr int PAINT_THREADS = 256;
constexpr int PAINT_QUADS = 4;    // quads (4 pixels) per thread and workgroup pass: 4096 pixels per workgroup
constexpr int PAINT_LDS_ROWS = 2048;   // tables up to 32 KB are staged in LDS

size_t table_lds_bytes(int D) { return ((size_t)TR * x_pitch(D) + (size_t)TR * H1P + (size_t)TR * H2 + TR) * sizeof(float); }

struct TableParams {
  const float* P;                 // flat parameters: W1 [256][D], b1, W2 [32][256], b2, W3 [1+D][32], b3
  const float* feat; int ld_row; long long ld_frame;
  int B, S, D;
  float mean, std, std_factor;
  const float* conf_dev;          // optional {mean, std, std_factor} in device memory (overrides the three scalars)
  float* table;                   // [B*S][4]
};

__global__ __launch_bounds__(256) void seg_table_kernel(TableParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int D = p.D, DP = x_pitch(D), R = p.B * p.S;
  float* xs = sm;                      // [TR][DP]
  float* h1s = xs + TR * DP;           // [TR][H1P]; after layer 2: the loss partials [TR][256]
  float* h2s = h1s + TR * H1P;         // [TR][H2]
  float* trav_s = h2s + TR * H2;       // [TR]
  const int tid = threadIdx.x, row0 = blockIdx.x * TR;
  const size_t oW1 = 0, ob1 = (size_t)H1 * D, oW2 = ob1 + H1, ob2 = oW2 + (size_t)H2 * H1, oW3 = ob2 + H2, ob3 = oW3 + (size_t)(D + 1) * H2;
  // ---- x tile (rows past R: zeros, never written out) ----
  load_x_tile<TR, true>(xs, p.feat, p.ld_row, p.ld_frame, p.S, D, row0, R);
  __syncthreads();
  // ---- layers 1 and 2, 8 and 2 rows per thread.  relu_nan: a NaN feature row stays NaN (the training forward clamps with fmaxf) ----
  smlp_layer1<TR / 2, relu_nan>(p.P, oW1, ob1, D, xs, [=](int r, int n0, float v0, float v1) {
    h1s[r * H1P + n0] = v0;
    h1s[r * H1P + n0 + 1] = v1;
  });
  __syncthreads();
  smlp_layer2<TR / 8, relu_nan>(p.P, oW2, ob2, h1s, [=](int r, int j, float v) { h2s[r * H2 + j] = v; });
  __syncthreads();
  // ---- layer 3 + reconstruction error: column 0 is the traversability, the others fold into per-thread partials ----
  float* part = h1s;                   // [TR][256] per-thread squared-error partials (h1 is dead)
  {
    float s[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r) s[r] = 0.f;
    smlp_layer3<TR, true>(p.P, oW3, ob3, D, h2s, [&](int r, int n, float a) {
      if (n == 0) {
        trav_s[r] = sigmoid_f(a);
      } else {
        const float e = a - xs[r * DP + n - 1];
        s[r] = fmaf(e, e, s[r]);
      }
    });
#pragma unroll
    for (int r = 0; r < TR; ++r) part[r * 256 + tid] = s[r];
  }
  __syncthreads();
  {
    const int r = tid >> 4, q = tid & 15;
    const float s = row_sum_256(part);
    // confidence_of: a NaN loss gets a finite confidence here (dmlp_fwd_kernel writes confidence_of_nan)
    if (q == 0 && row0 + r < R)
      table_row_write<confidence_of>(p.table + (size_t)(row0 + r) * TCOLS, trav_s[r], s / (float)D, p.conf_dev, p.mean, p.std, p.std_factor);
  }
}

struct PaintParams {
  const void* seg;                // [B][H*W] int32 or int64
  const float* table;             // [B*S][4]
  float *trav, *conf, *loss;      // [B][H*W], each may be NULL
  int B, S, P;                    // P = H * W
  int vec;                        // 1: seg and every output pointer are 16-byte aligned
};

template <typename IdT>
__device__ inline long long load_id(const IdT* s, long long f) { return (long long)s[f]; }

__device__ inline f32x4_t lookup(const float* tab, long long id, int S) {
  if (id < 0) id += S;
  if (id < 0 || id >= S) return f32x4_t{NAN, NAN, NAN, NAN};
  return *(const f32x4_t*)(tab + id * TCOLS);
}

__device__ inline void store1(const PaintParams& p, long long f, f32x4_t v) {
  if (p.trav) p.trav[f] = v[0];
  if (p.conf) p.conf[f] = v[1];
  if (p.loss) p.loss[f] = v[2];
}

// grid (ceil(P / 4096), B): workgroup (c, b) paints the 4-pixel quads c * 1024 .. + 1023 of frame b.  Quads are aligned on the FLAT
// pixel index b * P + p so that 16-byte accesses stay aligned for any H and W; the up to 3 pixels a frame has in front of its first
// whole quad and behind its last one are painted one by one by workgroup 0 of the frame.
template <typename IdT, bool IN_LDS>
__global__ __launch_bounds__(PAINT_THREADS) void seg_paint_kernel(PaintParams p) {
  extern __shared__ __attribute__((aligned(16))) float tab_s[];
  const int b = blockIdx.y, S = p.S;
  const float* tab_g = p.table + (size_t)b * S * TCOLS;
  if (IN_LDS) {
    for (int i = threadIdx.x; i < S; i += PAINT_THREADS) *(f32x4_t*)(tab_s + i * TCOLS) = *(const f32x4_t*)(tab_g + (size_t)i * TCOLS);
    __syncthreads();
  }
  const float* tab = IN_LDS ? tab_s : tab_g;
  const IdT* seg = (const IdT*)p.seg;
  const long long lo = (long long)b * p.P, hi = lo + p.P;
  const long long qa = (lo + 3) >> 2, qb = hi >> 2;     // whole quads [qa, qb) of this frame
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    // the single pixels: [lo, 4 qa) and [4 qb, hi), at most 3 + 3; a frame without a whole quad has at most 6 pixels
    const int t = threadIdx.x;
    long long f, end;
    if (qa >= qb) { f = lo + t; end = hi; }
    else if (t < 4) { f = lo + t; end = 4 * qa; }
    else { f = 4 * qb + (t - 4); end = hi; }
    if (f < end) store1(p, f, lookup(tab, load_id(seg, f), S));
  }
  const long long q0 = qa + (long long)blockIdx.x * PAINT_THREADS * PAINT_QUADS;
#pragma unroll
  for (int i = 0; i < PAINT_QUADS; ++i) {
    const long long q = q0 + i * PAINT_THREADS + threadIdx.x;
    if (q >= qb) break;
    const long long f = q * 4;
    long long id[4];
    if (p.vec) {
      if (sizeof(IdT) == 4) {
        const u32x4_t v = *(const u32x4_t*)(seg + f);
#pragma unroll
        for (int j = 0; j < 4; ++j) id[j] = (int)v[j];
      } else {
        const u32x4_t v0 = *(const u32x4_t*)(seg + f), v1 = *(const u32x4_t*)(seg + f + 2);
        id[0] = (long long)(((uint64_t)v0[1] << 32) | v0[0]); id[1] = (long long)(((uint64_t)v0[3] << 32) | v0[2]);
        id[2] = (long long)(((uint64_t)v1[1] << 32) | v1[0]); id[3] = (long long)(((uint64_t)v1[3] << 32) | v1[2]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) id[j] = load_id(seg, f + j);
    }
    f32x4_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = lookup(tab, id[j], S);
    if (p.vec) {
      if (p.trav) *(f32x4_t*)(p.trav + f) = f32x4_t{v[0][0], v[1][0], v[2][0], v[3][0]};
      if (p.conf) *(f32x4_t*)(p.conf + f) = f32x4_t{v[0][1], v[1][1], v[2][1], v[3][1]};
      if (p.loss) *(f32x4_t*)(p.loss + f) = f32x4_t{v[0][2], v[1][2], v[2][2], v[3][2]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) store1(p, f + j, v[j]);
    }
  }
}

template <typename IdT, bool IN_LDS>
int paint_launch(const PaintParams& p, hipStream_t st) {
  const int chunks = ceil_div(p.P, 4 * PAINT_THREADS * PAINT_QUADS);
  const size_t lds = IN_LDS ? (size_t)p.S * TCOLS * sizeof(float) : 0;
  hipLaunchKernelGGL((seg_paint_kernel<IdT, IN_LDS>), dim3(chunks, p.B), dim3(PAINT_THREADS), lds, st, p);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // namespace

bool wvn_segment_predict_supported(int D, int h1, int h2) { return h1 == H1 && h2 == H2 && D >= 1 && D <= DMAX; }

size_t wvn_segment_predict_workspace_bytes_impl(int B, int S) { return (size_t)B * S * TCOLS * sizeof(float); }

int wvn_segment_predict_launch(int D, const float* params, const float* feat, int ld_row, long long ld_frame, int B, int S,
                               const void* seg, int seg_bytes, int H, int W, float mean, float std, float std_factor,
                               const float* conf_state, float* trav, float* conf, float* loss, void* workspace,
                               size_t workspace_bytes, hipStream_t st) {
  // (every argument is checked by the caller, csrc/api.hip, before this point: no GPU call happens for a refused one)
  if (workspace_bytes < wvn_segment_predict_workspace_bytes_impl(B, S)) return WVN_ERR_WORKSPACE;
  TableParams t{};
  t.P = params; t.feat = feat; t.ld_row = ld_row; t.ld_frame = ld_frame;
  t.B = B; t.S = S; t.D = D;
  t.mean = mean; t.std = std; t.std_factor = std_factor; t.conf_dev = conf_state;
  t.table = (float*)workspace;
  const int lds = (int)table_lds_bytes(D);
  static LdsOptIn lds_opt_in;   // D > ~750 needs more than 64 KB: opted in once per device for the largest D (common.h)
  if (const int rc = lds_opt_in((int)table_lds_bytes(DMAX), (const void*)seg_table_kernel)) return rc;
  hipLaunchKernelGGL(seg_table_kernel, dim3(ceil_div(B * S, TR)), dim3(256), lds, st, t);
  WVN_LAUNCH_CHECK();
  return wvn_segment_paint_launch(t.table, B, S, seg, seg_bytes, H, W, trav, conf, loss, st);
}

int wvn_segment_paint_launch(const float* table, int B, int S, const void* seg, int seg_bytes, int H, int W, float* trav, float* conf,
                             float* loss, hipStream_t st) {
  PaintParams p{};
  p.seg = seg; p.table = table; p.trav = trav; p.conf = conf; p.loss = loss;
  p.B = B; p.S = S; p.P = H * W;
  uintptr_t a = (uintptr_t)seg | (uintptr_t)trav | (uintptr_t)conf | (uintptr_t)loss;
  p.vec = (a & 15) == 0;
  const bool in_lds = S <= PAINT_LDS_ROWS;
  if (seg_bytes == 4) return in_lds ? paint_launch<int, true>(p, st) : paint_launch<int, false>(p, st);
  return in_lds ? paint_launch<long long, true>(p, st) : paint_launch<long long, false>(p, st);
}
