// The ViT forward: host-side kernel routing only (no kernel lives here).  wvn_vit_forward* (api.hip) call wvn_vit_forward_impl.
//
// One call = patchify -> patch embedding -> depth x block -> final LayerNorm.  Which kernels a block launches is decided once per
// call (VitRoute, make_route) and once per layer (LayerRoute, layer_route); each precision family has its own block function.
// One block, per family and route (a step that answers WVN_ERR_ARG falls back to the step named after "else"):
//   block_fp8    LayerNorm+quantise | QKV | attention (bf16) | quantise, projection | LayerNorm+quantise |
//                fc1 with MX block scales out, fc2 on them  -- else fc1 (bf16 out), quantise, fc2.
//                The K = 768 linears run A-stationary (gemm_a768_fp8) from kRowsA768Fp8 rows on, else tiled (gemm_fp8).
//   block_lowp16 (BF16 / F16) from kRowsQkvFused / kRowsMlpFused rows on:
//                LayerNorm+QKV (qkv_fused; from the previous block's fragments after a hand-over) | attention |
//                projection + LayerNorm + MLP (proj_mlp_fused; resident form, may hand the next block's norm1 over)
//                  -- else projection | LayerNorm + MLP (mlp_fused);
//                below the thresholds: LayerNorm | QKV | attention | projection | LayerNorm | fc1 | fc2 (gemm_bf16).
//   block_split  (X3 / MIX) from kRowsSplitKernels rows on ("Round-4 entry points", has the full text):
//                MX route (MIX with *_w_mx):  a384_mx QKV (LayerNorm on load; block 0: LayerNorm + a384_x3) | fp16 attention, MX planes out |
//                                             n384_mx projection | a384_mx fc1 | n384_mx fc2;
//                fragment route:              a384_x3 QKV (LayerNorm on load) | attention (MIX: fp16, X3: attention_x3) |
//                                             n384_x3 projection (fragment form with proj_w_frag) | a384_x3 fc1 -> fragments | n384_x3 fc2;
//                below the threshold, or with WVN_VIT_NO_A384_X3: LayerNorm | QKV | attention | projection | LayerNorm | fc1 | fc2 (gemm_x3).
//   block_f32    LayerNorm | QKV | attention | projection | LayerNorm | fc1 | fc2 (gemm_f32, attention_f32).
#include <math.h>

#include <cstdlib>
#include <vector>

#include "../../include/wvn_hip.h"
#include "common.h"
#include "wvn_internal.h"

#define RET_IF(x)            \
  do {                       \
    int rc__ = (x);          \
    if (rc__ != WVN_OK) return rc__; \
  } while (0)

// ---------------------------------------------------------------------------------------------
// descriptor builders, shared with the stand-alone wvn_debug_* entries of api.hip
// ---------------------------------------------------------------------------------------------
static const float kLnEps = 1e-6f;                    // every LayerNorm of the network
static const float kLog2e = 1.44269504088896340736f;  // q leaves the QKV epilogue as an exp2 argument

void wvn_desc_qkv_epilogue(GemmBf16Params& p, void* q, void* k, void* vt, int heads, int npad, int ntok, int ntok_s, float q_scale, int qkv_f16,
                           void* q_lo, void* k_lo, void* vt_lo) {
  p.q = (bf16_t*)q; p.k = (bf16_t*)k; p.vt = (bf16_t*)vt; p.heads = heads; p.npad = npad; p.ntok = ntok; p.ntok_s = ntok_s;
  p.q_scale = q_scale; p.qkv_f16 = qkv_f16; p.q_lo = (bf16_t*)q_lo; p.k_lo = (bf16_t*)k_lo; p.vt_lo = (bf16_t*)vt_lo;
}

GemmBf16Params wvn_desc_a384(const void* A, const void* A_lo, int lda, const void* W, const void* W_lo, const float* bias, void* C, void* C_lo,
                             int ldc, int M, int N, long long* dbg, void* C_h8) {
  GemmBf16Params p{};
  p.A = (const bf16_t*)A; p.A_lo = (const bf16_t*)A_lo; p.lda = lda;
  p.W = (const bf16_t*)W; p.W_lo = W_lo ? (const bf16_t*)W_lo : (const bf16_t*)W + (size_t)N * 384; p.ldw = 384; p.bias = bias;
  p.C = C; p.C_lo = C_lo; p.C_h8 = C_h8; p.ldc = ldc; p.M = M; p.N = N; p.K = 384; p.dbg = dbg;
  return p;
}

void wvn_desc_ln_on_load(GemmBf16Params& p, const float* x, int ldx, const float* stats, const float* g, const float* b) {
  p.ln_x = x; p.ln_ldx = ldx; p.ln_stats = stats; p.ln_g = g; p.ln_b = b;
}

GemmBf16Params wvn_desc_n384(const void* A, const void* A_lo, int lda, const void* W, const void* W_lo, const float* bias, const float* ls, float* C,
                             int ldc, int M, int K, float* ln_stats_out, long long* dbg, const void* A_h8) {
  GemmBf16Params p{};
  p.A = (const bf16_t*)A; p.A_lo = (const bf16_t*)A_lo; p.A_h8 = A_h8; p.lda = lda; p.W = (const bf16_t*)W; p.W_lo = (const bf16_t*)W_lo; p.ldw = K;
  p.bias = bias; p.ls = ls; p.C = C; p.ldc = ldc; p.M = M; p.N = 384; p.K = K; p.dbg = dbg;
  if (ln_stats_out) { p.ln_stats_out = ln_stats_out; p.ln_eps = kLnEps; }
  return p;
}

// ---------------------------------------------------------------------------------------------
// profiling: HIP events around each launch category of wvn_vit_forward, on the launch stream
// ---------------------------------------------------------------------------------------------
namespace {
struct ProfSpan { hipEvent_t a, b; int cat; };
bool g_prof_on = false;
std::vector<ProfSpan> g_spans;
std::vector<hipEvent_t> g_event_pool;

hipEvent_t get_event() {
  if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
struct Span {
  hipStream_t st; hipEvent_t a{}, b{}; int cat; bool on;
  Span(int cat_, hipStream_t st_) : st(st_), cat(cat_), on(g_prof_on) {
    if (on) { a = get_event(); b = get_event(); (void)hipEventRecord(a, st); }
  }
  ~Span() {
    if (on) { (void)hipEventRecord(b, st); g_spans.push_back({a, b, cat}); }
  }
};
}  // namespace

extern "C" {

int wvn_prof_enable(int on) { g_prof_on = on != 0; return WVN_OK; }

int wvn_prof_collect(double* ms, long long* launches) {
  for (int i = 0; i < WVN_PROF_NCAT; ++i) { ms[i] = 0.0; launches[i] = 0; }
  for (auto& s : g_spans) {
    hipError_t e = hipEventSynchronize(s.b);
    if (e != hipSuccess) return (int)e;
    float t = 0.f;
    e = hipEventElapsedTime(&t, s.a, s.b);
    if (e != hipSuccess) return (int)e;
    if (s.cat >= 0 && s.cat < WVN_PROF_NCAT) { ms[s.cat] += t; launches[s.cat] += 1; }
    g_event_pool.push_back(s.a);
    g_event_pool.push_back(s.b);
  }
  g_spans.clear();
  return WVN_OK;
}

}  // extern "C"

namespace {
// ---------------------------------------------------------------------------------------------
// shapes and workspace
// ---------------------------------------------------------------------------------------------
// the launchers of the 16-bit-operand speed path, per operand format (operand.h)
struct OperandKernels {
  int fmt;  // 1 bf16, 2 fp16 (the y_fmt / out_mode codes of the elementwise launchers: patchify out_mode = fmt == 2 ? 3 : 1)
  decltype(&wvn_gemm_bf16_launch) gemm;
  decltype(&wvn_qkv_fused_launch) qkv_fused;
  decltype(&wvn_attention_bf16_launch) attention;
  decltype(&wvn_proj_mlp_fused_launch) proj_mlp_fused;
  decltype(&wvn_mlp_fused_launch) mlp_fused;
};
const OperandKernels OPK_BF16 = {1, wvn_gemm_bf16_launch, wvn_qkv_fused_launch, wvn_attention_bf16_launch, wvn_proj_mlp_fused_launch,
                                 wvn_mlp_fused_launch};
const OperandKernels OPK_F16 = {2, wvn_gemm_bf16_launch_f16, wvn_qkv_fused_launch_f16, wvn_attention_bf16_launch_f16,
                                wvn_proj_mlp_fused_launch_f16, wvn_mlp_fused_launch_f16};

struct VitDims {
  int B, S, P, G, D, H, F, KP, KPs, ntok, ntok_s, npad, npatch;
  bool fp8, planes;   // planes: WVN_PREC_X3 / WVN_PREC_MIX (hi + lo bf16 planes)
  size_t esz;
  long long M, Mp;
  // exact mode: an activation / weight "matrix" is two stacked bf16 planes, hi then lo; these are the plane distances in elements.
  // mpad32: whole 32-row groups (the fragment-major and MX layouts of w.xn / w.hid); pl_xn is the plane distance of BOTH layouts of w.xn
  size_t mpad32, pl_xn, pl_hid, pl_frag, pl_qkv, pl_pat;
};
VitDims vit_dims(const wvn_vit_model* m, int batch) {
  VitDims d;
  d.B = batch; d.S = m->img_size; d.P = m->patch; d.G = d.S / d.P; d.D = m->dim; d.H = m->heads; d.F = m->mlp_dim;
  d.KP = 3 * d.P * d.P; d.npatch = d.G * d.G; d.ntok = d.npatch + 1;
  // patch rows as the MFMA GEMMs read them: K padded to a multiple of 64 (588 -> 640 for patch 14; 192 and 768 unchanged);
  // the fp32 FMA path reads the unpadded rows
  d.KPs = m->precision == WVN_PREC_F32 ? d.KP : (d.KP + 63) / 64 * 64;
  d.fp8 = m->precision == WVN_PREC_FP8;
  d.planes = m->precision == WVN_PREC_X3 || m->precision == WVN_PREC_MIX;
  d.ntok_s = (d.ntok + 15) / 16 * 16;  // rows per frame: 8-token (16 B) chunks and the 16-token V^T permutation groups never straddle frames
  d.npad = (d.ntok + 127) / 128 * 128;
  d.esz = (m->precision == WVN_PREC_BF16 || m->precision == WVN_PREC_FP8 || m->precision == WVN_PREC_F16) ? 2 : 4;  // exact mode (X3): two bf16 planes = 4 bytes per element
  d.M = (long long)batch * d.ntok_s; d.Mp = (long long)batch * d.npatch;
  d.mpad32 = (size_t)((d.M + 31) / 32 * 32);
  d.pl_xn = (d.planes ? d.mpad32 : (size_t)d.M) * d.D; d.pl_hid = (size_t)d.M * d.F; d.pl_frag = d.mpad32 * d.F;
  d.pl_qkv = (size_t)d.B * d.H * d.npad * 64; d.pl_pat = (size_t)d.Mp * d.KPs;
  return d;
}
struct VitWs { float* x; void* xn; void* q; void* k; void* v; void* hid; void* patches; unsigned char* xq; unsigned char* hq; float* sa; float* ln_stats; size_t total; };
VitWs vit_carve(const VitDims& d, void* base) {
  VitWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes, 256); return (void*)((char*)base + o); };
  w.x = (float*)take((size_t)d.M * d.D * 4);
  w.xn = take(d.pl_xn * d.esz);
  w.q = take(d.pl_qkv * d.esz); w.k = take(d.pl_qkv * d.esz); w.v = take(d.pl_qkv * d.esz);
  w.hid = take((d.planes ? d.pl_frag : d.pl_hid) * d.esz);   // (planes: whole 32-row groups for the fragment-major MLP)
  w.patches = take(d.pl_pat * d.esz);
  w.xq = nullptr; w.hq = nullptr; w.sa = nullptr;
  if (d.fp8) {  // e4m3 images of the GEMM inputs + their per-row scales
    w.xq = (unsigned char*)take((size_t)d.M * d.D);
    w.hq = (unsigned char*)take((size_t)d.M * d.F);
    w.sa = (float*)take((size_t)d.M * 4);
  }
  w.ln_stats = d.planes ? (float*)take((size_t)d.M * 8) : nullptr;   // {mean, rstd} per row: LayerNorm across kernel boundaries (split-operand block kernels)
  w.total = off;
  return w;
}
bf16_t* lo(const void* base, size_t plane_elems) { return (bf16_t*)base + plane_elems; }

// ---------------------------------------------------------------------------------------------
// routes
// ---------------------------------------------------------------------------------------------
// Row thresholds (token rows M = B * ntok_s).  The single-kernel block stages are persistent one-workgroup-per-CU kernels (128 / 256 rows
// per workgroup): measured against the separate kernels (scripts/small_batch_latency.py, 448^2 and 224^2 frames) they win from about half a
// chip of row blocks on and lose below -- a single live frame is 25 / 13 row blocks on 256 CUs, 2.5 ms against 1.7.
const long long kRowsMlpFused = 128 * 128;      // LayerNorm + MLP (and projection + MLP) in one kernel
const long long kRowsQkvFused = 144 * 256;      // LayerNorm + QKV in one kernel
const long long kRowsSplitKernels = 64 * 128;   // split-operand A-stationary / row-panel kernels: from about a quarter chip of row blocks on
const long long kRowsA768Fp8 = 4096;            // fp8 A-stationary K = 768 kernel

enum VitFamily { FAM_F32, FAM_LOWP16, FAM_SPLIT, FAM_FP8 };

// Every per-call decision of the forward, made once (make_route).
struct VitRoute {
  VitFamily family;
  const OperandKernels* opk;   // the 16-bit launchers: fp16 operands for WVN_PREC_F16, bf16 for the rest (fp8 runs everything outside its four block linears as bf16)
  bool mix;                    // WVN_PREC_MIX: every linear as in the exact mode, the two attention products on the fp16-operand kernel
  int patch_mode;              // wvn_patchify_launch out_mode
  int ln_fmt;                  // wvn_layernorm_launch y_fmt of the block LayerNorms
  float scale, q_scale;        // softmax scale; q_scale: the same folded into q as an exp2 argument by the QKV epilogues of the 16-bit attention kernels
  // lowp16: the single-kernel block stages
  bool mlp_fused, qkv_fused, proj_in_mlp, hand_over;
  // split: the block kernels and, one piece at a time, their A/B switches
  bool split_kernels;          // the A-stationary / row-panel kernels may run (where a linear has kRowsSplitKernels rows)
  bool a_stationary, row_panel, frag_mlp, mx;
  bool x3_fast;                // ... and the blocks run them: LayerNorm-on-load QKV / fc1, fragment-major MLP
  bool ln_fuse;                // LayerNorm ACROSS kernel boundaries: the row-panel kernel that updates the residual rows (projection, fc2) leaves their
                               // {mean, rstd}, the A-stationary kernel that consumes them (fc1, next block's QKV) normalises as it loads
  int qsplit_blocks;           // the two-plane q in this many leading blocks (include/wvn_hip.h: WVN_VIT_QSPLIT_BLOCKS)
  // fp8
  bool a768;                   // the K = 768 linears on the A-stationary kernel
  bool hid_mx;                 // fc1 -> fc2 in the MX operand form (WVN_NO_FP8_MX, read per call: tests switch it between forwards)
};

bool split_kernel_rows(const VitRoute& r, long long rows) { return r.split_kernels && rows >= kRowsSplitKernels; }

int make_route(const wvn_vit_model* m, const VitDims& d, const VitWs& w, VitRoute* out) {
  VitRoute r{};
  const int prec = m->precision;
  const bool f16 = prec == WVN_PREC_F16, lowp16 = prec == WVN_PREC_BF16 || f16, x3 = d.planes, f32 = prec == WVN_PREC_F32;
  r.family = d.fp8 ? FAM_FP8 : lowp16 ? FAM_LOWP16 : x3 ? FAM_SPLIT : FAM_F32;
  r.opk = f16 ? &OPK_F16 : &OPK_BF16;
  r.mix = prec == WVN_PREC_MIX;
  r.patch_mode = f32 ? 0 : (x3 ? 2 : (f16 ? 3 : 1));
  r.ln_fmt = f32 ? 0 : r.opk->fmt;
  r.scale = 1.0f / sqrtf(64.f);
  r.q_scale = r.scale * kLog2e;
  const bool mlp_ok = (m->flags & WVN_VIT_MLP_FUSED) != 0, qkv_ok = (m->flags & WVN_VIT_QKV_FUSED) != 0;
  if (qkv_ok && (!lowp16 || d.D != 384 || d.H != 6 || (d.ntok_s % 16) != 0)) return WVN_ERR_ARG;
  if (mlp_ok && (!lowp16 || d.D != 384 || (d.F % 64) != 0)) return WVN_ERR_ARG;
  const bool any_size = (m->flags & WVN_VIT_FUSE_ANY_SIZE) != 0;
  r.mlp_fused = mlp_ok && (any_size || d.M >= kRowsMlpFused);
  r.qkv_fused = qkv_ok && (any_size || d.M >= kRowsQkvFused);
  r.proj_in_mlp = (m->flags & WVN_VIT_NO_PROJ_IN_MLP) == 0;
  r.hand_over = r.qkv_fused && !(m->flags & WVN_VIT_NO_LN_HANDOVER);
  r.split_kernels = x3 && !(m->flags & WVN_VIT_NO_A384_X3);
  r.a_stationary = !(m->flags & WVN_VIT_X3_NO_A384);
  r.row_panel = !(m->flags & WVN_VIT_X3_NO_N384);
  r.x3_fast = d.D == 384 && split_kernel_rows(r, d.M);
  r.ln_fuse = r.x3_fast && w.ln_stats && !(m->flags & WVN_VIT_X3_NO_LN_STATS);
  r.frag_mlp = r.x3_fast && !(m->flags & WVN_VIT_X3_NO_FRAG_MLP);
  r.mx = r.mix && r.ln_fuse && !(m->flags & WVN_VIT_NO_MX);   // the MX form needs the LayerNorm statistics hand-over
  const int qs_field = (m->flags >> 16) & 63;
  r.qsplit_blocks = r.mix ? (qs_field ? qs_field - 1 : WVN_VIT_QSPLIT_DEFAULT) : 0;
  r.a768 = d.fp8 && d.D == 768 && d.M >= kRowsA768Fp8;
  r.hid_mx = r.a768 && !getenv("WVN_NO_FP8_MX");
  *out = r;
  return WVN_OK;
}

// The per-layer part: what the layer's optional weights allow.
struct LayerRoute {
  bool mx;         // MX form of the block linears (round 6): fp16 hi * hi + two scaled e5m2 correction MFMAs per 64 k; the activations travel as three
                   // planes (fp16 fragments | l8 | h8) through w.xn (attention -> projection) and w.hid (fc1 -> fc2)
  bool attn_frag;  // WVN_PREC_MIX with a packed projection weight: the attention kernel writes fragments, the projection reads them
  bool qsplit;     // the attention kernel takes q as two fp16 planes
  bool frag_mlp;   // the split-operand MLP with the hidden activation handed over fragment-major
  bool hid_mx;     // fp8: fc1's GELU epilogue writes e4m3 + E8M0 block scales, fc2 multiplies with them
};
LayerRoute layer_route(const VitRoute& r, const wvn_vit_layer& L, int l) {
  LayerRoute lr;
  lr.mx = r.mx && L.qkv_w_mx && L.proj_w_mx && L.fc1_w_mx && L.fc2_w_mx;
  lr.attn_frag = r.mix && r.x3_fast && L.proj_w_frag != nullptr;
  lr.qsplit = l < r.qsplit_blocks;
  lr.frag_mlp = r.frag_mlp && L.fc2_w_fused != nullptr;
  lr.hid_mx = r.hid_mx && L.fc1_w_mx != nullptr;
  return lr;
}

// What one block leaves for the next.
struct BlockCarry {
  bool pre_qkv = false;    // lowp16: the next block's norm1 has been applied by this block's projection + MLP kernel (fragments in w.hid)
  bool ln1_stats = false;  // split: w.ln_stats holds the statistics of w.x for the next block's norm1
};

struct Fwd {
  const wvn_vit_model* m;
  VitDims d;
  VitWs w;
  VitRoute r;
  hipStream_t st;
  int M;
};

// ---------------------------------------------------------------------------------------------
// linears
// ---------------------------------------------------------------------------------------------
// One linear of the chain in the model's precision (not fp8).  A: activation matrix (bf16 | hi+lo planes | fp32), W: weight in the
// same representation ([N][K], planes stacked), epilogue codes of GemmEpilogue; extra: the epilogue's own fields.
// stats_written: set when the row-panel kernel ran and left the LayerNorm statistics extra asked for (the tiled kernel leaves none).
int linear(const Fwd& f, const void* A, size_t a_plane, int lda, const void* W, const float* bias, void* C, size_t c_plane, int ldc, int rows, int N,
           int K, int epi, const float* ls, const GemmBf16Params* extra, bool* stats_written = nullptr) {
  const VitDims& d = f.d;
  if (f.r.family == FAM_F32) {
    GemmF32Params p{};
    p.A = (const float*)A; p.lda = lda; p.B = (const float*)W; p.ldb = K; p.transB = 1; p.bias = bias;
    p.C = (float*)C; p.ldc = ldc; p.M = rows; p.N = N; p.K = K; p.batch = 1; p.splitk = 1; p.ls = ls;
    int fe = F32_EPI_NONE;
    switch (epi) {
      case EPI_GELU_BF16: fe = F32_EPI_GELU; break;
      case EPI_RESID_F32: fe = F32_EPI_RESID; break;
      case EPI_PATCH: fe = F32_EPI_PATCH; p.pos = f.m->pos; p.npatch = d.npatch; p.ntok = d.ntok; p.ntok_s = d.ntok_s; break;
      case EPI_QKV:
        fe = F32_EPI_QKV; p.C = (float*)f.w.q; p.q = (float*)f.w.q; p.k = (float*)f.w.k; p.v = (float*)f.w.v; p.heads = d.H;
        p.npad = d.npad; p.ntok = d.ntok; p.ntok_s = d.ntok_s; break;
      default: return WVN_ERR_ARG;
    }
    return wvn_gemm_f32_launch(p, fe, f.st);
  }
  GemmBf16Params p{};
  if (extra) p = *extra;
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = K; p.bias = bias; p.C = C; p.ldc = ldc;
  p.M = rows; p.N = N; p.K = K; p.ls = ls;
  if (f.r.family != FAM_SPLIT) return f.r.opk->gemm(p, epi, f.st);
  p.A_lo = lo(A, a_plane); p.W_lo = lo(W, (size_t)N * K); p.C_lo = C ? lo(C, c_plane) : nullptr;
  if (split_kernel_rows(f.r, rows)) {
    if (N == 384 && (epi == EPI_RESID_F32 || epi == EPI_PATCH) && f.r.row_panel) {   // row panel: fc2, projection, patch embedding
      const int rc = wvn_gemm_n384_x3_launch(p, epi, f.st);
      if (rc == WVN_OK && p.ln_stats_out && stats_written) *stats_written = true;
      if (rc != WVN_ERR_ARG) return rc;
    }
    if (K == 384 && f.r.a_stationary) {
      const int rc = wvn_gemm_a384_x3_launch(p, epi, f.st);
      if (rc != WVN_ERR_ARG) return rc;
    }
  }
  return wvn_gemm_x3_launch(p, epi, f.st);
}

// fp8: one of the four linears of a block on quantised rows (A rows as e4m3 + per-token scale in w.xq / w.hq / w.sa).
// Wp: the packed image of a K = 768 weight for the A-stationary kernel; elsewhere, or where that kernel declines, the tiled kernel
int linear_fp8(const Fwd& f, const unsigned char* Aq, int K, const void* W, const void* Wp, const float* sw, const float* bias, void* C, int ldc, int N,
               int epi, const float* ls, const GemmBf16Params* qkv) {
  GemmFp8Params p{};
  p.A = Aq; p.lda = K; p.W = (const unsigned char*)W; p.ldw = K; p.sa = f.w.sa; p.sw = sw; p.bias = bias; p.C = C; p.ldc = ldc;
  p.M = f.M; p.N = N; p.K = K; p.ls = ls;
  if (qkv) { p.q = qkv->q; p.k = qkv->k; p.vt = qkv->vt; p.heads = qkv->heads; p.npad = qkv->npad; p.ntok = qkv->ntok;
             p.ntok_s = qkv->ntok_s; p.q_scale = qkv->q_scale; }
  if (Wp && f.r.a768) {
    const int rc = wvn_gemm_a768_fp8_launch(p, Wp, epi, f.st);
    if (rc != WVN_ERR_ARG) return rc;
  }
  return wvn_gemm_fp8_launch(p, epi, f.st);
}

// a block LayerNorm as its own kernel: w.x -> w.xn (both planes in the split family)
int layernorm_rows(const Fwd& f, const float* g, const float* b) {
  Span s(2, f.st);
  return wvn_layernorm_launch(f.w.x, g, b, f.w.xn, f.r.ln_fmt, f.d.D, nullptr, 0, f.M, f.d.D, kLnEps, 0, f.d.ntok, f.d.ntok_s, f.st,
                              f.r.family == FAM_SPLIT ? lo(f.w.xn, f.d.pl_xn) : nullptr);
}

// the MLP as separate kernels through linear(): every family but fp8 ends here below its size thresholds
int mlp_separate(const Fwd& f, const wvn_vit_layer& L, bool ln2_done) {
  const VitDims& d = f.d;
  if (!ln2_done) RET_IF(layernorm_rows(f, L.ln2_g, L.ln2_b));
  { Span s(6, f.st); RET_IF(linear(f, f.w.xn, d.pl_xn, d.D, L.fc1_w, L.fc1_b, f.w.hid, d.pl_hid, d.F, f.M, d.F, d.D, EPI_GELU_BF16, nullptr, nullptr)); }
  Span s(7, f.st);
  return linear(f, f.w.hid, d.pl_hid, d.F, L.fc2_w, L.fc2_b, f.w.x, 0, d.D, f.M, d.D, d.F, EPI_RESID_F32, L.ls2, nullptr);
}

// ---------------------------------------------------------------------------------------------
// one block per precision family
// ---------------------------------------------------------------------------------------------
// fp8: quantise-then-GEMM for the four linears of a block
int block_fp8(const Fwd& f, const wvn_vit_layer& L, const LayerRoute& lr) {
  const VitDims& d = f.d; const VitWs& w = f.w; hipStream_t st = f.st; const int M = f.M;
  if (!L.qkv_s || !L.proj_s || !L.fc1_s || !L.fc2_s) return WVN_ERR_ARG;
  { Span s(2, st); RET_IF(wvn_layernorm_fp8_launch(w.x, L.ln1_g, L.ln1_b, w.xq, d.D, w.sa, M, d.D, kLnEps, st)); }
  {
    Span s(3, st);
    GemmBf16Params e{};
    wvn_desc_qkv_epilogue(e, w.q, w.k, w.v, d.H, d.npad, d.ntok, d.ntok_s, f.r.q_scale);
    RET_IF(linear_fp8(f, w.xq, d.D, L.qkv_w, L.qkv_w_mx, L.qkv_s, L.qkv_b, nullptr, 0, 3 * d.D, EPI_QKV, nullptr, &e));
  }
  { Span s(4, st); RET_IF(f.r.opk->attention((const bf16_t*)w.q, (const bf16_t*)w.k, (const bf16_t*)w.v, (bf16_t*)w.xn, d.B, d.H, d.ntok, d.ntok_s, d.npad, 0.f, st, nullptr, nullptr, 0, -1)); }
  {
    Span s(5, st);
    RET_IF(wvn_quantize_rows_fp8_launch(w.xn, 1, d.D, w.xq, d.D, w.sa, M, d.D, st));
    RET_IF(linear_fp8(f, w.xq, d.D, L.proj_w, L.proj_w_mx, L.proj_s, L.proj_b, w.x, d.D, d.D, EPI_RESID_F32, L.ls1, nullptr));
  }
  { Span s(2, st); RET_IF(wvn_layernorm_fp8_launch(w.x, L.ln2_g, L.ln2_b, w.xq, d.D, w.sa, M, d.D, kLnEps, st)); }
  // fc1 -> fc2 in the MX operand form where the A-stationary kernel runs fc1 (round 6): its GELU epilogue writes the hidden activation as e4m3 with ONE E8M0 block
  // scale per (row, 32 columns) -- a 32-column tile of fc1 is one scale block of fc2's K -- and fc2 multiplies with those block scales on its A operand: no row
  // quantiser (and no bf16 copy of the hidden activation) between the two.  The scales sit in w.hid, which this form does not use otherwise.
  int rc = WVN_ERR_ARG;   // of fc1 in the MX form
  {
    Span s(6, st);
    if (lr.hid_mx) {
      GemmFp8Params p{};
      p.A = w.xq; p.lda = d.D; p.sa = w.sa; p.sw = L.fc1_s; p.bias = L.fc1_b; p.C = w.hq; p.ldc = d.F; p.c_scales = (unsigned char*)w.hid;
      p.M = M; p.N = d.F; p.K = d.D;
      rc = wvn_gemm_a768_fp8_launch(p, L.fc1_w_mx, EPI_GELU_MX8, st);
      if (rc != WVN_OK && rc != WVN_ERR_ARG) return rc;
    }
    if (rc == WVN_ERR_ARG) RET_IF(linear_fp8(f, w.xq, d.D, L.fc1_w, L.fc1_w_mx, L.fc1_s, L.fc1_b, w.hid, d.F, d.F, EPI_GELU_BF16, nullptr, nullptr));
  }
  Span s(7, st);
  if (rc == WVN_OK) {
    GemmFp8Params p{};
    p.A = w.hq; p.lda = d.F; p.a_scales = (const unsigned char*)w.hid; p.W = (const unsigned char*)L.fc2_w; p.ldw = d.F; p.sw = L.fc2_s; p.bias = L.fc2_b;
    p.C = w.x; p.ldc = d.D; p.M = M; p.N = d.D; p.K = d.F; p.ls = L.ls2;
    return wvn_gemm_fp8_launch(p, EPI_RESID_F32, st);
  }
  RET_IF(wvn_quantize_rows_fp8_launch(w.hid, 1, d.F, w.hq, d.F, w.sa, M, d.F, st));   // the bf16 hidden activation, quantised by rows
  return linear_fp8(f, w.hq, d.F, L.fc2_w, nullptr, L.fc2_s, L.fc2_b, w.x, d.D, d.D, EPI_RESID_F32, L.ls2, nullptr);
}

// BF16 / F16: the single-kernel block stages where the route allows them, the separate kernels where not or where a stage declines
int block_lowp16(const Fwd& f, const wvn_vit_layer& L, const wvn_vit_layer* next, BlockCarry& carry) {
  const VitDims& d = f.d; const VitWs& w = f.w; const VitRoute& r = f.r; hipStream_t st = f.st; const int M = f.M;
  const OperandKernels& opk = *r.opk;
  const bool pre_qkv = carry.pre_qkv;
  carry.pre_qkv = false;
  int rc = WVN_ERR_ARG;
  if (r.qkv_fused) {  // LayerNorm 1 + QKV projection: one launch, no xn round trip
    Span s(3, st);
    // (pre_qkv: the previous block's projection + MLP kernel has already applied this block's norm1 to the rows as they left it,
    //  and parked the result as operand fragments in w.hid)
    rc = pre_qkv ? opk.qkv_fused(nullptr, 0, nullptr, nullptr, 0.f, (const bf16_t*)L.qkv_w_fused, L.qkv_b, (bf16_t*)w.q, (bf16_t*)w.k,
                                 (bf16_t*)w.v, d.H, d.npad, d.ntok_s, r.q_scale, M, st, (const bf16_t*)w.hid)
                 : opk.qkv_fused(w.x, d.D, L.ln1_g, L.ln1_b, kLnEps, (const bf16_t*)L.qkv_w, L.qkv_b, (bf16_t*)w.q, (bf16_t*)w.k,
                                 (bf16_t*)w.v, d.H, d.npad, d.ntok_s, r.q_scale, M, st, nullptr);
    if (rc != WVN_OK && rc != WVN_ERR_ARG) return rc;
  }
  if (rc == WVN_ERR_ARG) {   // not eligible (e.g. q / k / v beyond the 2 GB a buffer descriptor spans): the separate kernels
    RET_IF(layernorm_rows(f, L.ln1_g, L.ln1_b));
    // the softmax scale is folded into q by the QKV epilogue (q leaves it as an exp2 argument) and attention takes
    // the running max as an MFMA operand (attention_bf16.hip, PRE)
    GemmBf16Params e{};
    wvn_desc_qkv_epilogue(e, w.q, w.k, w.v, d.H, d.npad, d.ntok, d.ntok_s, r.q_scale);
    Span s(3, st);
    RET_IF(linear(f, w.xn, d.pl_xn, d.D, L.qkv_w, L.qkv_b, nullptr, 0, 0, M, 3 * d.D, d.D, EPI_QKV, nullptr, &e));
  }
  { Span s(4, st); RET_IF(opk.attention((const bf16_t*)w.q, (const bf16_t*)w.k, (const bf16_t*)w.v, (bf16_t*)w.xn, d.B, d.H, d.ntok, d.ntok_s, d.npad, 0.f, st, nullptr, nullptr, 0, -1)); }
  if (r.mlp_fused && r.proj_in_mlp) {  // attention projection + LayerNorm 2 + fc1 + GELU + fc2 + both residual updates: one launch
    Span s(6, st);
    if (!L.fc2_w_fused) return WVN_ERR_ARG;
    // the resident form may also apply the NEXT block's norm1 and hand the rows to its QKV kernel as operand fragments
    rc = WVN_ERR_ARG;
    if (r.hand_over && next && L.fc1_w_fused && next->qkv_w_fused) {
      rc = opk.proj_mlp_fused((const bf16_t*)w.xn, d.D, (const bf16_t*)L.proj_w, L.proj_b, L.ls1, L.ln2_g, L.ln2_b, kLnEps,
                              (const bf16_t*)L.fc1_w, L.fc1_b, (const bf16_t*)L.fc2_w_fused, L.fc2_b, L.ls2, w.x, d.D, M, d.F, st,
                              (const bf16_t*)L.fc1_w_fused, next->ln1_g, next->ln1_b, kLnEps, (bf16_t*)w.hid);
      carry.pre_qkv = rc == WVN_OK;
    }
    if (rc == WVN_ERR_ARG)
      rc = opk.proj_mlp_fused((const bf16_t*)w.xn, d.D, (const bf16_t*)L.proj_w, L.proj_b, L.ls1, L.ln2_g, L.ln2_b, kLnEps,
                              (const bf16_t*)L.fc1_w, L.fc1_b, (const bf16_t*)L.fc2_w_fused, L.fc2_b, L.ls2, w.x, d.D, M, d.F, st,
                              (const bf16_t*)L.fc1_w_fused, nullptr, nullptr, 0.f, nullptr);
    if (rc != WVN_ERR_ARG) return rc;   // (WVN_ERR_ARG: not eligible -- separate kernels)
  }
  { Span s(5, st); RET_IF(linear(f, w.xn, d.pl_xn, d.D, L.proj_w, L.proj_b, w.x, 0, d.D, M, d.D, d.D, EPI_RESID_F32, L.ls1, nullptr)); }
  if (r.mlp_fused) {  // LayerNorm 2 + fc1 + GELU + fc2 + residual: one launch, no xn / hid round trip
    Span s(6, st);
    if (!L.fc2_w_fused) return WVN_ERR_ARG;
    return opk.mlp_fused(nullptr, 0, L.ln2_g, L.ln2_b, kLnEps, (const bf16_t*)L.fc1_w, L.fc1_b, (const bf16_t*)L.fc2_w_fused, L.fc2_b, L.ls2, w.x, d.D, M,
                         d.F, st);
  }
  return mlp_separate(f, L, false);
}

// X3 / MIX: every linear on hi + lo bf16 planes.  From kRowsSplitKernels rows on the LayerNorms travel as row statistics between the
// row-panel kernels that write the residual rows and the A-stationary kernels that read them; lr.mx / lr.attn_frag / lr.frag_mlp
// choose the layouts in which the attention output and the hidden activation cross from one kernel to the next.
int block_split(const Fwd& f, const wvn_vit_layer& L, const LayerRoute& lr, bool last, BlockCarry& carry) {
  const VitDims& d = f.d; const VitWs& w = f.w; const VitRoute& r = f.r; hipStream_t st = f.st; const int M = f.M;
  unsigned char* xn_l8 = (unsigned char*)w.xn + d.mpad32 * d.D * 2;     // MX planes of the attention output: fp16 fragments | l8 (h8 = e5m2(h) is derived by the consumer)
  unsigned char* hid_l8 = (unsigned char*)w.hid + d.mpad32 * d.F * 2;   // ... and of the hidden activation
  bf16_t* q_lo = lr.qsplit || !r.mix ? lo(w.q, d.pl_qkv) : nullptr;
  float* next_stats = r.ln_fuse && !last ? w.ln_stats : nullptr;        // fc2 leaves the next block's norm1 statistics
  const bool ln1_stats = carry.ln1_stats;
  carry.ln1_stats = false;

  // QKV.  MIX: one fp16 plane each for k and v^T, q pre-scaled and in TWO fp16 planes where lr.qsplit (its rounding residue behind it): the
  // fp16 attention kernel's operands.  X3: hi / lo planes of all three
  auto qkv_epilogue = [&](GemmBf16Params& p) {
    if (r.mix) wvn_desc_qkv_epilogue(p, w.q, w.k, w.v, d.H, d.npad, d.ntok, d.ntok_s, r.q_scale, 1, q_lo);
    else wvn_desc_qkv_epilogue(p, w.q, w.k, w.v, d.H, d.npad, d.ntok, d.ntok_s, 0.f, 0, q_lo, lo(w.k, d.pl_qkv), lo(w.v, d.pl_qkv));
  };
  int rc = WVN_ERR_ARG;
  if (ln1_stats) {   // norm1 on load, from the statistics the previous block's fc2 kernel left: the MX kernel, else the bf16 x 3 one
    Span s(3, st);
    auto desc = [&](const void* W) {   // W: both planes / both MX images, stacked
      GemmBf16Params q = wvn_desc_a384(nullptr, nullptr, 0, W, nullptr, L.qkv_b, nullptr, nullptr, 0, M, 3 * d.D);
      wvn_desc_ln_on_load(q, w.x, d.D, w.ln_stats, L.ln1_g, L.ln1_b);
      qkv_epilogue(q);
      return q;
    };
    if (lr.mx) rc = wvn_gemm_a384_mx_launch(desc(L.qkv_w_mx), EPI_QKV, st);
    if (rc == WVN_ERR_ARG) rc = wvn_gemm_a384_x3_launch(desc(L.qkv_w), EPI_QKV, st);
    if (rc != WVN_OK && rc != WVN_ERR_ARG) return rc;
  }
  if (rc == WVN_ERR_ARG) {   // no statistics (block 0, tiled route), or the A-stationary kernel declined
    RET_IF(layernorm_rows(f, L.ln1_g, L.ln1_b));
    GemmBf16Params e{};
    qkv_epilogue(e);
    Span s(3, st);
    RET_IF(linear(f, w.xn, d.pl_xn, d.D, L.qkv_w, L.qkv_b, nullptr, 0, 0, M, 3 * d.D, d.D, EPI_QKV, nullptr, &e));
  }

  {
    Span s(4, st);
    if (r.mix)   // output: MX planes (2) | operand fragments (1) | row-major hi / lo planes (0)
      RET_IF(wvn_attention_bf16_launch_f16((const bf16_t*)w.q, (const bf16_t*)w.k, (const bf16_t*)w.v, (bf16_t*)w.xn, d.B, d.H, d.ntok, d.ntok_s, d.npad, 0.f, st,
                                           lr.mx ? (bf16_t*)xn_l8 : lo(w.xn, d.pl_xn), q_lo, lr.mx ? 2 : lr.attn_frag ? 1 : 0));
    else
      RET_IF(wvn_attention_x3_launch((const bf16_t*)w.q, q_lo, (const bf16_t*)w.k, lo(w.k, d.pl_qkv), (const bf16_t*)w.v, lo(w.v, d.pl_qkv), (bf16_t*)w.xn,
                                     lo(w.xn, d.pl_xn), d.B, d.H, d.ntok, d.ntok_s, d.npad, r.scale, st));
  }

  bool ln2_stats = false;   // w.ln_stats holds the statistics of w.x for this block's norm2
  {
    Span s(5, st);
    if (lr.mx) {   // the attention output arrived as MX operand planes: the projection on the MX row-panel kernel
      RET_IF(wvn_gemm_n384_mx_launch(wvn_desc_n384(w.xn, xn_l8, d.D, L.proj_w_mx, nullptr, L.proj_b, L.ls1, w.x, d.D, M, d.D, w.ln_stats), EPI_RESID_F32, st));
      ln2_stats = true;
    } else if (lr.attn_frag) {   // ... as operand fragments: the fragment form of the row-panel kernel
      float* stats = r.ln_fuse ? w.ln_stats : nullptr;
      RET_IF(wvn_gemm_n384_x3_frag_launch(wvn_desc_n384(w.xn, lo(w.xn, d.pl_xn), d.D, L.proj_w_frag, nullptr, L.proj_b, L.ls1, w.x, d.D, M, d.D, stats), EPI_RESID_F32, st));
      ln2_stats = r.ln_fuse;
    } else {
      GemmBf16Params se{};
      if (r.ln_fuse) { se.ln_stats_out = w.ln_stats; se.ln_eps = kLnEps; }
      RET_IF(linear(f, w.xn, d.pl_xn, d.D, L.proj_w, L.proj_b, w.x, 0, d.D, M, d.D, d.D, EPI_RESID_F32, L.ls1, r.ln_fuse ? &se : nullptr, &ln2_stats));
    }
  }

  if (lr.mx) {   // LayerNorm-on-load fc1 + GELU -> MX operand planes -> MX row-panel fc2 (+ the next block's LayerNorm statistics)
    GemmBf16Params p1 = wvn_desc_a384(nullptr, nullptr, 0, L.fc1_w_mx, nullptr, L.fc1_b, w.hid, hid_l8, d.F, M, d.F);
    wvn_desc_ln_on_load(p1, w.x, d.D, w.ln_stats, L.ln2_g, L.ln2_b);
    { Span s(6, st); RET_IF(wvn_gemm_a384_mx_launch(p1, EPI_GELU_FRAG, st)); }
    Span s(7, st);
    RET_IF(wvn_gemm_n384_mx_launch(wvn_desc_n384(w.hid, hid_l8, d.F, L.fc2_w_mx, nullptr, L.fc2_b, L.ls2, w.x, d.D, M, d.F, next_stats), EPI_RESID_F32, st));
    carry.ln1_stats = next_stats != nullptr;
    return WVN_OK;
  }
  bool ln2_done = false;
  if (lr.frag_mlp) {
    // the split-operand MLP with the hidden activation handed over FRAGMENT-MAJOR: fc1 (gemm_a384_x3, EPI_GELU_FRAG) writes the
    // MFMA operand fragments of fc2 straight from its accumulators, fc2 (gemm_n384_x3, AFRAG) fetches them with one coalesced load
    // per lane and plane -- no LDS transpose on either side, every access a contiguous kilobyte
    rc = WVN_ERR_ARG;
    if (ln2_stats) {   // norm2 on load, from the statistics the projection kernel left
      GemmBf16Params p1 = wvn_desc_a384(nullptr, nullptr, 0, L.fc1_w, nullptr, L.fc1_b, w.hid, lo(w.hid, d.pl_frag), d.F, M, d.F);
      wvn_desc_ln_on_load(p1, w.x, d.D, w.ln_stats, L.ln2_g, L.ln2_b);
      Span s(6, st);
      rc = wvn_gemm_a384_x3_launch(p1, EPI_GELU_FRAG, st);
      if (rc != WVN_OK && rc != WVN_ERR_ARG) return rc;
    }
    if (rc == WVN_ERR_ARG) {
      RET_IF(layernorm_rows(f, L.ln2_g, L.ln2_b));
      ln2_done = true;
      Span s(6, st);
      rc = wvn_gemm_a384_x3_launch(wvn_desc_a384(w.xn, lo(w.xn, d.pl_xn), d.D, L.fc1_w, nullptr, L.fc1_b, w.hid, lo(w.hid, d.pl_frag), d.F, M, d.F), EPI_GELU_FRAG, st);
      if (rc != WVN_OK && rc != WVN_ERR_ARG) return rc;
    }
    if (rc == WVN_OK) {
      Span s(7, st);
      RET_IF(wvn_gemm_n384_x3_frag_launch(wvn_desc_n384(w.hid, lo(w.hid, d.pl_frag), d.F, L.fc2_w_fused, nullptr, L.fc2_b, L.ls2, w.x, d.D, M, d.F, next_stats), EPI_RESID_F32, st));
      carry.ln1_stats = next_stats != nullptr;
      return WVN_OK;
    }
  }
  return mlp_separate(f, L, ln2_done);   // (fc2 through linear() asks for no statistics: the next block runs its LayerNorm kernel)
}

int block_f32(const Fwd& f, const wvn_vit_layer& L) {
  const VitDims& d = f.d; const VitWs& w = f.w; hipStream_t st = f.st; const int M = f.M;
  RET_IF(layernorm_rows(f, L.ln1_g, L.ln1_b));
  { Span s(3, st); RET_IF(linear(f, w.xn, 0, d.D, L.qkv_w, L.qkv_b, nullptr, 0, 0, M, 3 * d.D, d.D, EPI_QKV, nullptr, nullptr)); }
  { Span s(4, st); RET_IF(wvn_attention_f32_launch((const float*)w.q, (const float*)w.k, (const float*)w.v, (float*)w.xn, d.B, d.H, d.ntok, d.ntok_s, d.npad, f.r.scale, st)); }
  { Span s(5, st); RET_IF(linear(f, w.xn, 0, d.D, L.proj_w, L.proj_b, w.x, 0, d.D, M, d.D, d.D, EPI_RESID_F32, L.ls1, nullptr)); }
  return mlp_separate(f, L, false);
}
}  // namespace

size_t wvn_vit_workspace_bytes_impl(const wvn_vit_model* m, int batch) { return vit_carve(vit_dims(m, batch), nullptr).total; }

// cols_mirror (with ing): the `batch` frames go through the network TWICE in one launch sequence of 2 * batch frames -- frame
// batch + i is frame i gathered through the second column table (its mirror image: the flip pass of the upstream Stego.get_code).
// Twice the rows per launch: the persistent block kernels end on a thinner partial round (6.2 -> 12.3 rounds of row blocks).
int wvn_vit_forward_impl(const wvn_vit_model* m, const void* img, int img_u8, const WvnIngest* ing, int batch, float* tokens_f32, void* tokens_lowp,
                         int ld_lowp, void* workspace, size_t workspace_bytes, void* stream, const int* cols_mirror, const wvn_stego_head* head) {
  if (!m || !img || !workspace || batch <= 0 || (cols_mirror && !ing)) return WVN_ERR_ARG;
  if (head && (tokens_f32 || tokens_lowp)) return WVN_ERR_ARG;   // the code INSTEAD of the tokens: a caller that needs both runs the head itself
  const int frames_in = batch;
  if (cols_mirror) batch *= 2;
  if (m->dim != m->heads * 64 || m->depth <= 0 || m->depth > WVN_MAX_DEPTH || m->img_size % m->patch) return WVN_ERR_ARG;
  if (m->dim % 128 || m->mlp_dim % 128) return WVN_ERR_ARG;
  if (m->precision < WVN_PREC_F32 || m->precision > WVN_PREC_MIX) return WVN_ERR_ARG;
  Fwd f;
  f.m = m; f.st = (hipStream_t)stream; f.d = vit_dims(m, batch); f.w = vit_carve(f.d, workspace); f.M = (int)f.d.M;
  if (f.w.total > workspace_bytes) return WVN_ERR_WORKSPACE;
  RET_IF(make_route(m, f.d, f.w, &f.r));
  const VitDims& d = f.d; const VitWs& w = f.w; const VitRoute& r = f.r; hipStream_t st = f.st;
  const bool split = r.family == FAM_SPLIT, f32 = r.family == FAM_F32;
  if (split && tokens_lowp) return WVN_ERR_ARG;  // exact mode hands out fp32 tokens only (callers split with wvn_split_planes)
  const int Mp = (int)d.Mp;
  bf16_t* head_hid = (bf16_t*)w.hid;   // the head's hidden planes [2][Mp][384]: the hidden-activation region is free once the last fc2 has run
  if (head) {
    // Eligible on the route of the split-operand block kernels with the statistics buffer (D = 384, r.ln_fuse, from kRowsSplitKernels rows on) where the head
    // launch takes the shapes; decided here, before anything is launched
    if (!split || d.D != 384 || !r.ln_fuse) return WVN_ERR_ARG;
    if (!head->w_cat || !head->b_cat || !head->w_nl || !head->b_nl || !head->code || head->code_dim <= 0 || head->code_dim > 128 || head->ld_code < 128 ||
        (head->ld_code % 4))
      return WVN_ERR_ARG;
    if ((((uintptr_t)head->w_cat | (uintptr_t)head->w_nl | (uintptr_t)head->code) & 15) || (size_t)d.Mp * 384 * 2 >= (1ull << 31) ||
        (size_t)d.Mp * head->ld_code * 4 >= (1ull << 31) || (size_t)2 * d.Mp * 384 > d.pl_frag * 2)
      return WVN_ERR_ARG;
  }

  {
    Span s(0, st);
    // patch rows of frames_in frames gathered through `in`, from element offset `off` of the patch matrix on
    auto patchify = [&](size_t off, const WvnIngest* in) {
      return wvn_patchify_launch(img, img_u8, (char*)w.patches + off * (f32 ? 4 : 2), split ? lo(w.patches, d.pl_pat) + off : nullptr, r.patch_mode, d.KPs,
                                 frames_in, d.S, d.P, st, in);
    };
    RET_IF(patchify(0, ing));
    if (cols_mirror) {   // the mirror images' patch rows behind the frames'
      WvnIngest ing2 = *ing;
      ing2.cols = cols_mirror;
      RET_IF(patchify((size_t)frames_in * d.npatch * d.KPs, &ing2));
    }
    if (d.KPs != d.KP) {  // zero the K padding of the patch rows (weights are zero there too, but NaN * 0 must not happen)
      RET_IF(wvn_pad_zero_launch(w.patches, (long long)Mp * (split ? 2 : 1), (long long)d.KPs * 2, (long long)d.KP * 2,
                                 (long long)(d.KPs - d.KP) * 2, st));
    }
  }
  RET_IF(wvn_cls_rows_launch(m->cls_pos, w.x, d.B, d.ntok_s, d.D, st));
  {
    // Padding hygiene, every call (the carve depends on the batch, so a reused workspace holds stale bytes):
    // residual-stream rows [ntok, ntok_s) start at zero (they then carry finite values through the blocks), and the
    // never-written key/value slots [ntok_s, npad) are zero.  The attention kernels mask padded keys by score, but
    // their V^T / K bytes still enter MFMAs and must be finite.
    RET_IF(wvn_pad_zero_launch(w.x, d.B, (long long)d.ntok_s * d.D * 4, (long long)d.ntok * d.D * 4,
                               (long long)(d.ntok_s - d.ntok) * d.D * 4, st));
    // with the fused LayerNorm + QKV kernel nothing writes the padding rows of xn (the attention output buffer the projection
    // GEMM reads whole): they used to hold LayerNorm 1's output
    if (r.qkv_fused)
      RET_IF(wvn_pad_zero_launch(w.xn, d.B, (long long)d.ntok_s * d.D * 2, (long long)d.ntok * d.D * 2, (long long)(d.ntok_s - d.ntok) * d.D * 2, st));
    const long long nbh = (long long)d.B * d.H;
    const long long tokb = f32 ? 256 : 128, npl = (split && !r.mix) ? 2 : 1;  // bytes per token row of q / k; planes per tensor
    RET_IF(wvn_pad_zero_launch(w.q, nbh * (split ? 2 : 1), d.npad * tokb, d.ntok_s * tokb, (d.npad - d.ntok_s) * tokb, st));   // (mix: q has two fp16 planes)
    RET_IF(wvn_pad_zero_launch(w.k, nbh * npl, d.npad * tokb, d.ntok_s * tokb, (d.npad - d.ntok_s) * tokb, st));
    if (!f32)  // V^T [B*h*64][npad] (bf16, or hi / lo planes)
      RET_IF(wvn_pad_zero_launch(w.v, nbh * 64 * npl, (long long)d.npad * 2, (long long)d.ntok_s * 2, (long long)(d.npad - d.ntok_s) * 2, st));
    else     // V [B*h][npad][64]
      RET_IF(wvn_pad_zero_launch(w.v, nbh, d.npad * tokb, d.ntok_s * tokb, (d.npad - d.ntok_s) * tokb, st));
  }
  {
    Span s(1, st);
    GemmBf16Params e{};
    e.pos = m->pos; e.npatch = d.npatch; e.ntok = d.ntok; e.ntok_s = d.ntok_s;
    RET_IF(linear(f, w.patches, d.pl_pat, d.KPs, m->patch_w, m->patch_b, w.x, 0, d.D, Mp, d.D, d.KPs, EPI_PATCH, nullptr, &e));
  }
  BlockCarry carry;
  for (int l = 0; l < m->depth; ++l) {
    const wvn_vit_layer& L = m->layers[l];
    const bool last = l + 1 == m->depth;
    const LayerRoute lr = layer_route(r, L, l);
    switch (r.family) {
      case FAM_FP8: RET_IF(block_fp8(f, L, lr)); break;
      case FAM_LOWP16: RET_IF(block_lowp16(f, L, last ? nullptr : &m->layers[l + 1], carry)); break;
      case FAM_SPLIT: RET_IF(block_split(f, L, lr, last, carry)); break;
      case FAM_F32: RET_IF(block_f32(f, L)); break;
    }
  }
  if (head) {
    // the STEGO head off the residual rows: LayerNorm on load + [W_hid; W_lin] in one A-stationary launch, then code += hid W_nl^T + b_nl on the tiled kernel
    // The final LayerNorm's {mean, rstd} come from a statistics pass with the LayerNorm kernel's own arithmetic, not from the last fc2's one-pass sums: the
    // tokens formed on load are then the ones that kernel writes, and the code is the separate launches' bit for bit
    RET_IF(wvn_layernorm_patch_stats_launch(w.x, w.ln_stats, d.B, d.npatch, d.ntok_s, kLnEps, st));
    bf16_t* hid_lo = head_hid + (size_t)Mp * 384;
    RET_IF(wvn_gemm_a384_head_launch(w.x, d.D, w.ln_stats, m->norm_g, m->norm_b, (const bf16_t*)head->w_cat, (const bf16_t*)head->w_cat + (size_t)512 * 384, head->b_cat,
                                     head_hid, hid_lo, head->code, head->ld_code, d.B, d.npatch, d.ntok_s, st));
    GemmBf16Params p{};
    p.A = head_hid; p.A_lo = hid_lo; p.lda = 384; p.W = (const bf16_t*)head->w_nl; p.W_lo = (const bf16_t*)head->w_nl + (size_t)head->code_dim * 384; p.ldw = 384;
    p.bias = head->b_nl; p.C = head->code; p.ldc = head->ld_code; p.M = Mp; p.N = head->code_dim; p.K = 384;
    return wvn_gemm_x3_launch(p, EPI_RESID_F32, st);
  }
  Span s(2, st);
  return wvn_layernorm_launch(w.x, m->norm_g, m->norm_b, tokens_lowp, split || f32 ? 0 : r.opk->fmt, ld_lowp, tokens_f32, d.D, Mp, d.D, kLnEps, 1, d.ntok,
                              d.ntok_s, st);
}
