// C-ABI of libwvn_hip.so (see include/wvn_hip.h) and the host-side launch sequence of the three phases of the
// traversability-MLP optimisation step.  The ViT forward chain behind wvn_vit_forward* is vit_forward.hip.
#include <math.h>
#include <string.h>

#include "../../include/wvn_hip.h"

#include "common.h"
#include "wvn_internal.h"

#define RET_IF(x)            \
  do {                       \
    int rc__ = (x);          \
    if (rc__ != WVN_OK) return rc__; \
  } while (0)

int wvn_num_cus() {   // (common.h)
  static std::atomic<int> count[64];   // per device ordinal; 0: not asked yet (two host threads racing here ask twice and store the same number)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::atomic<int>& c = count[dev & 63];
  int n = c.load(std::memory_order_relaxed);
  if (n == 0) {
    hipDeviceProp_t prop;
    n = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c.store(n, std::memory_order_relaxed);
  }
  return n;
}

extern "C" {

int wvn_version(void) { return 103; }   // 103: wvn_debug_slic_lab; 102: wvn_gcn_train_*; 101: wvn_flip_average takes the source row stride; wvn_vit_forward_frames_head

size_t wvn_vit_workspace_bytes(const wvn_vit_model* m, int batch) {
  if (!m || batch <= 0) return 0;
  return wvn_vit_workspace_bytes_impl(m, batch);
}

int wvn_vit_forward(const wvn_vit_model* m, const float* img, int batch, float* tokens_f32, void* tokens_lowp,
                    int ld_lowp, void* workspace, size_t workspace_bytes, void* stream) {
  return wvn_vit_forward_impl(m, img, 0, nullptr, batch, tokens_f32, tokens_lowp, ld_lowp, workspace, workspace_bytes, stream);
}

int wvn_vit_forward_u8(const wvn_vit_model* m, const unsigned char* img, int batch, float* tokens_f32, void* tokens_lowp,
                       int ld_lowp, void* workspace, size_t workspace_bytes, void* stream) {
  if (m && ((m->precision != WVN_PREC_BF16 && m->precision != WVN_PREC_FP8 && m->precision != WVN_PREC_F16) || m->patch != 8)) return WVN_ERR_ARG;
  return wvn_vit_forward_impl(m, img, 1, nullptr, batch, tokens_f32, tokens_lowp, ld_lowp, workspace, workspace_bytes, stream);
}

int wvn_vit_forward_frames(const wvn_vit_model* m, const void* frames, int frames_u8, int src_h, int src_w, const int* rows,
                           const int* cols, int batch, float* tokens_f32, void* tokens_lowp, int ld_lowp, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (!rows || !cols || src_h <= 0 || src_w <= 0) return WVN_ERR_ARG;
  const WvnIngest ing{rows, cols, src_h, src_w};
  return wvn_vit_forward_impl(m, frames, frames_u8 != 0, &ing, batch, tokens_f32, tokens_lowp, ld_lowp, workspace, workspace_bytes, stream);
}

int wvn_vit_forward_frames_pair(const wvn_vit_model* m, const void* frames, int frames_u8, int src_h, int src_w, const int* rows,
                                const int* cols, const int* cols_mirror, int batch, float* tokens_f32, void* tokens_lowp, int ld_lowp,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!rows || !cols || !cols_mirror || src_h <= 0 || src_w <= 0) return WVN_ERR_ARG;
  const WvnIngest ing{rows, cols, src_h, src_w};
  return wvn_vit_forward_impl(m, frames, frames_u8 != 0, &ing, batch, tokens_f32, tokens_lowp, ld_lowp, workspace, workspace_bytes, stream,
                              cols_mirror);
}

int wvn_vit_forward_frames_head(const wvn_vit_model* m, const void* frames, int frames_u8, int src_h, int src_w, const int* rows,
                                const int* cols, const int* cols_mirror, int batch, const wvn_stego_head* head, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!rows || !cols || !head || src_h <= 0 || src_w <= 0) return WVN_ERR_ARG;
  const WvnIngest ing{rows, cols, src_h, src_w};
  return wvn_vit_forward_impl(m, frames, frames_u8 != 0, &ing, batch, nullptr, nullptr, 0, workspace, workspace_bytes, stream, cols_mirror, head);
}

int wvn_debug_stego_head_fused(const float* x, int ldx, const float* stats, const float* ln_g, const float* ln_b, const void* w_cat, const float* b_cat,
                               void* hid, void* hid_lo, float* code, int ld_code, int frames, int npatch, int ntok_s, void* stream) {
  if (!w_cat) return WVN_ERR_ARG;
  return wvn_gemm_a384_head_launch(x, ldx, stats, ln_g, ln_b, (const bf16_t*)w_cat, (const bf16_t*)w_cat + (size_t)512 * 384, b_cat, (bf16_t*)hid,
                                   (bf16_t*)hid_lo, code, ld_code, frames, npatch, ntok_s, (hipStream_t)stream);
}

int wvn_resize_nearest_crop(const void* in, void* out, long long planes, int src_h, int src_w, const int* rows, const int* cols,
                            int out_h, int out_w, int elem_bytes, void* stream) {
  const WvnIngest ing{rows, cols, src_h, src_w};
  return wvn_gather_image_launch(in, out, planes, out_h, out_w, elem_bytes, &ing, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// building blocks
// ---------------------------------------------------------------------------------------------
int wvn_gemm_bf16(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N,
                  int K, int epi, void* stream) {
  if (epi < 0 || epi > EPI_ACCUM_F32 || !C) return WVN_ERR_ARG;
  GemmBf16Params p{};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K;
  return wvn_gemm_bf16_launch(p, epi, (hipStream_t)stream);
}

int wvn_gemm_f16(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N,
                 int K, int epi, void* stream) {
  if (epi < 0 || epi > EPI_ACCUM_F32 || !C) return WVN_ERR_ARG;
  GemmBf16Params p{};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K;
  return wvn_gemm_bf16_launch_f16(p, epi, (hipStream_t)stream);
}
int wvn_qkv_fused_f16(const float* x, int ldx, const float* ln_g, const float* ln_b, float ln_eps, const void* W, const float* bias,
                      void* q, void* k, void* vt, int heads, int npad, int ntok_s, float q_scale, int M, void* stream) {
  return wvn_qkv_fused_launch_f16(x, ldx, ln_g, ln_b, ln_eps, (const bf16_t*)W, bias, (bf16_t*)q, (bf16_t*)k, (bf16_t*)vt, heads, npad,
                                  ntok_s, q_scale, M, (hipStream_t)stream, nullptr);
}
int wvn_qkv_prenorm_f16(const void* xn_frag, const void* Wperm, const float* bias, void* q, void* k, void* vt, int heads, int npad,
                        int ntok_s, float q_scale, int M, void* stream) {
  if (!xn_frag) return WVN_ERR_ARG;
  return wvn_qkv_fused_launch_f16(nullptr, 0, nullptr, nullptr, 0.f, (const bf16_t*)Wperm, bias, (bf16_t*)q, (bf16_t*)k, (bf16_t*)vt, heads,
                                  npad, ntok_s, q_scale, M, (hipStream_t)stream, (const bf16_t*)xn_frag);
}
int wvn_proj_mlp_fused_f16(const void* attn, int lda, const void* Wp, const float* bp, const float* ls1, const float* ln_g,
                           const float* ln_b, float ln_eps, const void* W1, const float* b1, const void* W2p, const float* b2,
                           const float* ls2, float* x, int ldx, int M, int F, void* stream) {
  return wvn_proj_mlp_fused_launch_f16((const bf16_t*)attn, lda, (const bf16_t*)Wp, bp, ls1, ln_g, ln_b, ln_eps, (const bf16_t*)W1, b1,
                                       (const bf16_t*)W2p, b2, ls2, x, ldx, M, F, (hipStream_t)stream, nullptr, nullptr, nullptr, 0.f, nullptr);
}
int wvn_proj_mlp_resident_f16(const void* attn, int lda, const void* Wp, const float* bp, const float* ln_g, const float* ln_b,
                              float ln_eps, const void* W1p, const float* b1, const void* W2p, const float* b2, float* x, int ldx,
                              int M, int F, const float* next_ln_g, const float* next_ln_b, float next_ln_eps, void* xn_next,
                              void* stream) {
  if (!W1p) return WVN_ERR_ARG;
  return wvn_proj_mlp_fused_launch_f16((const bf16_t*)attn, lda, (const bf16_t*)Wp, bp, nullptr, ln_g, ln_b, ln_eps, nullptr, b1,
                                       (const bf16_t*)W2p, b2, nullptr, x, ldx, M, F, (hipStream_t)stream, (const bf16_t*)W1p, next_ln_g, next_ln_b,
                                   next_ln_eps, (bf16_t*)xn_next);
}
int wvn_mlp_fused_f16(const void* xn, int lda, const float* ln_g, const float* ln_b, float ln_eps, const void* W1, const float* b1,
                      const void* W2p, const float* b2, const float* ls, float* x, int ldx, int M, int F, void* stream) {
  return wvn_mlp_fused_launch_f16((const bf16_t*)xn, lda, ln_g, ln_b, ln_eps, (const bf16_t*)W1, b1, (const bf16_t*)W2p, b2, ls, x,
                                  ldx, M, F, (hipStream_t)stream);
}
int wvn_attention_f16(const void* q, const void* k, const void* vt, void* out, int B, int heads, int ntok, int npad, float scale,
                      void* stream) {
  return wvn_attention_bf16_launch_f16((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)out, B, heads, ntok, ntok,
                                       npad, scale, (hipStream_t)stream);
}

int wvn_qkv_fused(const float* x, int ldx, const float* ln_g, const float* ln_b, float ln_eps, const void* W, const float* bias,
                  void* q, void* k, void* vt, int heads, int npad, int ntok_s, float q_scale, int M, void* stream) {
  return wvn_qkv_fused_launch(x, ldx, ln_g, ln_b, ln_eps, (const bf16_t*)W, bias, (bf16_t*)q, (bf16_t*)k, (bf16_t*)vt, heads, npad, ntok_s,
                              q_scale, M, (hipStream_t)stream, nullptr);
}
int wvn_qkv_prenorm(const void* xn_frag, const void* Wperm, const float* bias, void* q, void* k, void* vt, int heads, int npad, int ntok_s,
                    float q_scale, int M, void* stream) {
  if (!xn_frag) return WVN_ERR_ARG;
  return wvn_qkv_fused_launch(nullptr, 0, nullptr, nullptr, 0.f, (const bf16_t*)Wperm, bias, (bf16_t*)q, (bf16_t*)k, (bf16_t*)vt, heads, npad,
                              ntok_s, q_scale, M, (hipStream_t)stream, (const bf16_t*)xn_frag);
}

int wvn_proj_mlp_fused(const void* attn, int lda, const void* Wp, const float* bp, const float* ls1, const float* ln_g,
                       const float* ln_b, float ln_eps, const void* W1, const float* b1, const void* W2p, const float* b2,
                       const float* ls2, float* x, int ldx, int M, int F, void* stream) {
  return wvn_proj_mlp_fused_launch((const bf16_t*)attn, lda, (const bf16_t*)Wp, bp, ls1, ln_g, ln_b, ln_eps, (const bf16_t*)W1, b1,
                                   (const bf16_t*)W2p, b2, ls2, x, ldx, M, F, (hipStream_t)stream, nullptr, nullptr, nullptr, 0.f, nullptr);
}
int wvn_proj_mlp_resident(const void* attn, int lda, const void* Wp, const float* bp, const float* ln_g, const float* ln_b,
                          float ln_eps, const void* W1p, const float* b1, const void* W2p, const float* b2, float* x, int ldx, int M,
                          int F, const float* next_ln_g, const float* next_ln_b, float next_ln_eps, void* xn_next, void* stream) {
  if (!W1p) return WVN_ERR_ARG;
  return wvn_proj_mlp_fused_launch((const bf16_t*)attn, lda, (const bf16_t*)Wp, bp, nullptr, ln_g, ln_b, ln_eps, nullptr, b1,
                                   (const bf16_t*)W2p, b2, nullptr, x, ldx, M, F, (hipStream_t)stream, (const bf16_t*)W1p, next_ln_g, next_ln_b,
                                   next_ln_eps, (bf16_t*)xn_next);
}

int wvn_mlp_fused(const void* xn, int lda, const float* ln_g, const float* ln_b, float ln_eps, const void* W1, const float* b1,
                  const void* W2p, const float* b2, const float* ls, float* x, int ldx, int M, int F, void* stream) {
  return wvn_mlp_fused_launch((const bf16_t*)xn, lda, ln_g, ln_b, ln_eps, (const bf16_t*)W1, b1, (const bf16_t*)W2p, b2, ls, x, ldx,
                              M, F, (hipStream_t)stream);
}

int wvn_gemm_x3(const void* A_hi, const void* A_lo, int lda, const void* W_hi, const void* W_lo, int ldw, const float* bias,
                void* C, void* C_lo, int ldc, int M, int N, int K, int epi, void* stream) {
  if (epi < 0 || epi > EPI_ACCUM_F32 || !C) return WVN_ERR_ARG;
  GemmBf16Params p{};
  p.A = (const bf16_t*)A_hi; p.A_lo = (const bf16_t*)A_lo; p.lda = lda; p.W = (const bf16_t*)W_hi; p.W_lo = (const bf16_t*)W_lo;
  p.ldw = ldw; p.bias = bias; p.C = C; p.C_lo = C_lo; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  return wvn_gemm_x3_launch(p, epi, (hipStream_t)stream);
}
int wvn_quantize_rows_fp8(const void* src, int src_is_bf16, int lds, void* q, int ldq, float* scale, int rows, int cols,
                          void* stream) {
  return wvn_quantize_rows_fp8_launch(src, src_is_bf16, lds, (unsigned char*)q, ldq, scale, rows, cols, (hipStream_t)stream);
}
int wvn_layernorm_fp8(const float* x, const float* gamma, const float* beta, void* q, int ldq, float* scale, int rows, int D,
                      float eps, void* stream) {
  return wvn_layernorm_fp8_launch(x, gamma, beta, (unsigned char*)q, ldq, scale, rows, D, eps, (hipStream_t)stream);
}
int wvn_gemm_fp8(const void* A_q, int lda, const void* W_q, int ldw, const float* sa, const float* sw, const float* bias,
                 void* C, int ldc, int M, int N, int K, int epi, void* stream) {
  if (epi != EPI_BF16 && epi != EPI_GELU_BF16 && epi != EPI_F32 && epi != EPI_RESID_F32) return WVN_ERR_ARG;
  GemmFp8Params p{};
  p.A = (const unsigned char*)A_q; p.lda = lda; p.W = (const unsigned char*)W_q; p.ldw = ldw; p.sa = sa; p.sw = sw; p.bias = bias;
  p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  return wvn_gemm_fp8_launch(p, epi, (hipStream_t)stream);
}
int wvn_gemm_a768_fp8(const void* A_q, int lda, const void* W_packed, const float* sa, const float* sw, const float* bias, const float* ls, void* C, int ldc,
                      int M, int N, int epi, void* q, void* k, void* vt, int heads, int npad, int ntok_s, float q_scale, void* stream) {
  GemmFp8Params p{};
  p.A = (const unsigned char*)A_q; p.lda = lda; p.sa = sa; p.sw = sw; p.bias = bias; p.ls = ls; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = 768;
  p.q = (bf16_t*)q; p.k = (bf16_t*)k; p.vt = (bf16_t*)vt; p.heads = heads; p.npad = npad; p.ntok_s = ntok_s; p.q_scale = q_scale;
  if (epi == EPI_GELU_MX8) p.c_scales = (unsigned char*)q;   // (epi 9: C = e4m3 [M][ldc], q = its E8M0 block scales [M][N / 32])
  return wvn_gemm_a768_fp8_launch(p, W_packed, epi, (hipStream_t)stream);
}
int wvn_gemm_fp8_mx(const void* A_q, int lda, const void* a_scales, const void* W_q, int ldw, const float* sw, const float* bias, const float* ls,
                    void* C, int ldc, int M, int N, int K, int epi, void* stream) {
  if (!a_scales || (epi != EPI_F32 && epi != EPI_RESID_F32)) return WVN_ERR_ARG;
  GemmFp8Params p{};
  p.A = (const unsigned char*)A_q; p.lda = lda; p.a_scales = (const unsigned char*)a_scales; p.W = (const unsigned char*)W_q; p.ldw = ldw; p.sw = sw; p.bias = bias;
  p.ls = ls; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  return wvn_gemm_fp8_launch(p, epi, (hipStream_t)stream);
}
int wvn_split_planes(const float* src, int lds, void* hi, void* lo, int ldd, int rows, int cols, void* stream) {
  return wvn_split_planes_launch(src, lds, (bf16_t*)hi, (bf16_t*)lo, ldd, rows, cols, (hipStream_t)stream);
}
int wvn_attention_x3(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* vt_hi,
                     const void* vt_lo, void* out_hi, void* out_lo, int B, int heads, int ntok, int npad, float scale,
                     void* stream) {
  return wvn_attention_x3_launch((const bf16_t*)q_hi, (const bf16_t*)q_lo, (const bf16_t*)k_hi, (const bf16_t*)k_lo,
                                 (const bf16_t*)vt_hi, (const bf16_t*)vt_lo, (bf16_t*)out_hi, (bf16_t*)out_lo, B, heads, ntok,
                                 ntok, npad, scale, (hipStream_t)stream);
}

int wvn_debug_f16_saturate(const float* in, void* out_f16, int n, void* stream) {
  return (in && out_f16 && n > 0) ? wvn_f16_saturate_probe_launch(in, (uint16_t*)out_f16, n, (hipStream_t)stream) : WVN_ERR_ARG;
}
int wvn_debug_slic_lab(const void* img, int img_is_u8, int npix, const int* lut_lin, const int* lut_f, int* lab, void* stream) {
  return wvn_slic_lab_launch(img, img_is_u8, npix, lut_lin, lut_f, lab, (hipStream_t)stream);
}
int wvn_debug_attention_timing(long long* dbg) { wvn_attention_bf16_set_debug(dbg); return WVN_OK; }
int wvn_debug_mlp_fused_timing(long long* dbg) { g_mlp_fused_dbg = dbg; return WVN_OK; }
int wvn_debug_qkv_fused_timing(long long* dbg) { g_qkv_fused_dbg = dbg; return WVN_OK; }
int wvn_stream_create_cu_mask(void** stream, const unsigned int* mask, int words) {
  if (!stream || !mask || words <= 0) return WVN_ERR_ARG;
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask);
  if (e != hipSuccess) return (int)e;
  *stream = (void*)st;
  return WVN_OK;
}
int wvn_stream_destroy(void* stream) {
  if (!stream) return WVN_ERR_ARG;
  const hipError_t e = hipStreamDestroy((hipStream_t)stream);
  return e == hipSuccess ? WVN_OK : (int)e;
}

// The stand-alone entries of the split-operand / MX block kernels build their descriptors with the builders the forward uses (vit_forward.hip).
int wvn_debug_gemm_a384_x3(const void* A, const void* A_lo, int lda, const void* W, const void* W_lo, const float* bias, void* C,
                           void* C_lo, int ldc, int M, int N, int epi, long long* dbg, void* stream) {
  if (epi != EPI_GELU_BF16 && epi != EPI_RESID_F32) return WVN_ERR_ARG;
  return wvn_gemm_a384_x3_launch(wvn_desc_a384(A, A_lo, lda, W, W_lo, bias, C, C_lo, ldc, M, N, dbg), epi, (hipStream_t)stream);
}
int wvn_debug_gemm_n384_x3(const void* A, const void* A_lo, int lda, const void* W, const void* W_lo, const float* bias, const float* ls,
                           float* C, int ldc, int M, int K, long long* dbg, void* stream) {
  return wvn_gemm_n384_x3_launch(wvn_desc_n384(A, A_lo, lda, W, W_lo, bias, ls, C, ldc, M, K, nullptr, dbg), EPI_RESID_F32, (hipStream_t)stream);
}
int wvn_debug_mlp_x3_frag(const void* xn, const void* xn_lo, const void* W1, const void* W1_lo, const float* b1, void* hid, void* hid_lo,
                          const void* W2p, const float* b2, float* x, int M, int F, long long* dbg1, long long* dbg2, void* stream) {
  RET_IF(wvn_gemm_a384_x3_launch(wvn_desc_a384(xn, xn_lo, 384, W1, W1_lo, b1, hid, hid_lo, F, M, F, dbg1), EPI_GELU_FRAG, (hipStream_t)stream));
  return wvn_gemm_n384_x3_frag_launch(wvn_desc_n384(hid, hid_lo, F, W2p, nullptr, b2, nullptr, x, 384, M, F, nullptr, dbg2), EPI_RESID_F32, (hipStream_t)stream);
}
int wvn_debug_gemm_n384_mx(const void* A_h, const void* A_l8, const void* A_h8, const void* Wp, const float* bias, const float* ls, float* C,
                           int ldc, int M, int K, long long* dbg, void* stream) {
  return wvn_gemm_n384_mx_launch(wvn_desc_n384(A_h, A_l8, K, Wp, nullptr, bias, ls, C, ldc, M, K, nullptr, dbg, A_h8), EPI_RESID_F32, (hipStream_t)stream);
}
int wvn_debug_mlp_mx(const float* x, int ldx, const float* ln_stats, const float* ln_g, const float* ln_b, const void* W1p, const float* b1,
                     void* hid_h, void* hid_l8, void* hid_h8, const void* W2p, const float* b2, float* xout, int M, int F, long long* dbg1,
                     long long* dbg2, void* stream) {
  GemmBf16Params p1 = wvn_desc_a384(nullptr, nullptr, 0, W1p, nullptr, b1, hid_h, hid_l8, F, M, F, dbg1, hid_h8);
  wvn_desc_ln_on_load(p1, x, ldx, ln_stats, ln_g, ln_b);
  RET_IF(wvn_gemm_a384_mx_launch(p1, EPI_GELU_FRAG, (hipStream_t)stream));
  if (!W2p) return WVN_OK;
  return wvn_gemm_n384_mx_launch(wvn_desc_n384(hid_h, hid_l8, F, W2p, nullptr, b2, nullptr, xout, 384, M, F, nullptr, dbg2, hid_h8), EPI_RESID_F32, (hipStream_t)stream);
}
int wvn_debug_qkv_mx(const float* x, int ldx, const float* ln_stats, const float* ln_g, const float* ln_b, const void* Wp, const float* bias, void* q,
                     void* q_lo, void* k, void* vt, int heads, int npad, int ntok_s, float q_scale, int M, long long* dbg, void* stream) {
  GemmBf16Params p = wvn_desc_a384(nullptr, nullptr, 0, Wp, nullptr, bias, nullptr, nullptr, 0, M, 3 * heads * 64, dbg);
  wvn_desc_ln_on_load(p, x, ldx, ln_stats, ln_g, ln_b);
  wvn_desc_qkv_epilogue(p, q, k, vt, heads, npad, 0, ntok_s, q_scale, 1, q_lo);
  return wvn_gemm_a384_mx_launch(p, EPI_QKV, (hipStream_t)stream);
}
int wvn_debug_n384_pair(int on) {
  if (on >= 32) { wvn_gemm_a384_mx_set_form(on - 32); return WVN_OK; }   // 33 / 34: form 1 / 2 of the A-stationary MX kernel
  wvn_gemm_n384_x3_set_pair(on);
  return WVN_OK;
}
int wvn_debug_kmeans_screen_stats(unsigned long long* out, int reset) { return out ? wvn_kmeans_pixels_screen_stats(out, reset) : WVN_ERR_ARG; }
int wvn_debug_kmeans_assign_form(int form) { wvn_kmeans_pixels_set_assign_form(form); return WVN_OK; }
int wvn_debug_attention_variant(int v) { wvn_attention_bf16_set_variant(v); wvn_attention_bf16_set_variant_f16(v); return WVN_OK; }
int wvn_debug_attention_planes(const void* q, const void* q_lo, const void* k, const void* vt, void* out, void* out_lo, int B, int heads, int ntok,
                               int ntok_s, int npad, int out_frag, int qsplit_form, void* stream) {
  // the combinations wvn_vit_forward launches in WVN_PREC_MIX (plus the single row-major output of wvn_attention_f16), nothing else
  if (!q || !k || !vt || !out || B < 1 || heads < 1 || ntok < 1 || ntok_s < ntok || ntok_s > npad) return WVN_ERR_ARG;
  if (qsplit_form < 0 || qsplit_form > 2 || (qsplit_form == 0) != (q_lo == nullptr)) return WVN_ERR_ARG;
  if (out_frag < 0 || out_frag > 2 || (out_frag != 0 && (!out_lo || heads != 6))) return WVN_ERR_ARG;
  return wvn_attention_bf16_launch_f16((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)out, B, heads, ntok, ntok_s, npad, 0.f,
                                       (hipStream_t)stream, (bf16_t*)out_lo, (const bf16_t*)q_lo, out_frag, qsplit_form);
}

int wvn_debug_gemm_bf16_timed(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M,
                              int N, int K, int epi, long long* dbg, void* stream) {
  if (epi < 0 || epi > EPI_ACCUM_F32 || !C) return WVN_ERR_ARG;
  GemmBf16Params p{};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.dbg = dbg;
  return wvn_gemm_bf16_launch(p, epi, (hipStream_t)stream);
}

int wvn_debug_gemm_n384(const void* A, int lda, const void* W, int ldw, const float* bias, float* C, int ldc, int M, int K,
                        void* stream) {
  GemmBf16Params p{};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias; p.C = C; p.ldc = ldc;
  p.M = M; p.N = 384; p.K = K;
  return wvn_gemm_n384_launch(p, EPI_RESID_F32, (hipStream_t)stream, nullptr, 1);
}

int wvn_gemm_f32(const float* A, int lda, int transA, const float* B, int ldb, int transB, const float* bias, float* C,
                 int ldc, int M, int N, int K, int epi, const float* mask, int ldmask, void* stream) {
  if (epi < 0 || epi > F32_EPI_RELUMASK) return WVN_ERR_ARG;
  GemmF32Params p{};
  p.A = A; p.lda = lda; p.transA = transA; p.B = B; p.ldb = ldb; p.transB = transB; p.bias = bias; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.batch = 1; p.splitk = 1; p.mask = mask; p.ldmask = ldmask;
  return wvn_gemm_f32_launch(p, epi, (hipStream_t)stream);
}

int wvn_layernorm(const float* x, const float* gamma, const float* beta, void* y, int y_is_bf16, int rows, int D,
                  float eps, void* stream) {
  if (!y) return WVN_ERR_ARG;
  return wvn_layernorm_launch(x, gamma, beta, y, y_is_bf16 ? 1 : 0, D, nullptr, 0, rows, D, eps, 0, 0, 0, (hipStream_t)stream);
}

int wvn_attention_bf16(const void* q, const void* k, const void* vt, void* out, int B, int heads, int ntok, int npad,
                       float scale, void* stream) {
  return wvn_attention_bf16_launch((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)out, B, heads, ntok,
                                   ntok, npad, scale, (hipStream_t)stream);
}
int wvn_attention_f32(const float* q, const float* k, const float* v, float* out, int B, int heads, int ntok, int npad,
                      float scale, void* stream) {
  return wvn_attention_f32_launch(q, k, v, out, B, heads, ntok, ntok, npad, scale, (hipStream_t)stream);
}
int wvn_patchify(const float* img, void* patches, int out_is_bf16, int B, int S, int P, void* stream) {
  return wvn_patchify_launch(img, 0, patches, nullptr, out_is_bf16 ? 1 : 0, 0, B, S, P, (hipStream_t)stream);
}

int wvn_patchify_u8(const unsigned char* img, void* patches_bf16, int B, int S, int P, void* stream) {
  return wvn_patchify_launch(img, 1, patches_bf16, nullptr, 1, 0, B, S, P, (hipStream_t)stream);
}
int wvn_cast_f32_to_bf16(const float* src, void* dst, long long n, void* stream) {
  if (!src || !dst || n <= 0 || n > 0x7fffffffll) return WVN_ERR_ARG;
  return wvn_cast_f32_bf16_launch(src, (int)n, (bf16_t*)dst, (int)n, 1, (int)n, (hipStream_t)stream);
}
int wvn_cast_rows(const float* src, int lds, void* dst, int ldd, int rows, int cols, int to_f16, void* stream) {
  if (!src || !dst || rows <= 0 || cols <= 0 || lds < cols || ldd < cols) return WVN_ERR_ARG;
  return wvn_cast_f32_bf16_launch(src, lds, (bf16_t*)dst, ldd, rows, cols, (hipStream_t)stream, to_f16 != 0);
}
int wvn_upsample_bilinear(const float* tokens, float* dense, int B, int G, int D, int H, void* stream) {
  return wvn_upsample_bilinear_launch(tokens, dense, B, G, D, H, (hipStream_t)stream);
}
int wvn_upsample_nearest_i32(const int* labels, int* out, int B, int G, int H, void* stream) {
  if (!labels || !out) return WVN_ERR_ARG;
  return wvn_upsample_nearest_i32_launch(labels, out, B, G, H, (hipStream_t)stream);
}
int wvn_segpool_bilinear_mean(const int* seg, const float* tokens, int ld, float* feat, void* scratch_w,
                              int* scratch_cnt, int B, int H, int W, int G, int S, int D, void* stream) {
  return wvn_segpool_launch(seg, tokens, ld, feat, scratch_w, scratch_cnt, B, H, W, G, S, D, (hipStream_t)stream);
}
int wvn_segpool_patch_labels(const int* labels, const float* tokens, int ld, const float* wy, const float* wx,
                             float* feat, int B, int G, int S, int D, void* stream) {
  return wvn_segpool_patch_launch(labels, tokens, ld, wy, wx, feat, B, G, S, D, (hipStream_t)stream);
}
size_t wvn_segmean_scratch_bytes(int B, int P, int S, int D) {
  return (B > 0 && P > 0 && S > 0 && D > 0) ? wvn_segmean_scratch_bytes_impl(B, P, S, D) : 0;
}
int wvn_segmean_tokens(const int* seg, const float* tokens, float* feat, int* scratch_cnt, void* scratch, size_t scratch_bytes,
                       int B, int P, int S, int D, void* stream) {
  return wvn_segmean_tokens_launch(seg, tokens, feat, scratch_cnt, scratch, scratch_bytes, B, P, S, D, (hipStream_t)stream);
}
int wvn_label_pool(const float* mask, int C, const int* seg, float* signal, unsigned char* valid, void* scratch_sum,
                   int* scratch_cnt, int H, int W, int S, void* stream) {
  return wvn_label_pool_launch(mask, C, seg, signal, valid, scratch_sum, scratch_cnt, H, W, S, (hipStream_t)stream);
}
int wvn_label_pool_batched(const wvn_label_pool_node* nodes_dev, int n, int C, int H, int W, int Smax, void* scratch_sum,
                           int* scratch_cnt, void* stream) {
  return wvn_label_pool_batched_launch(nodes_dev, n, C, H, W, Smax, (long long*)scratch_sum, scratch_cnt, (hipStream_t)stream);
}
int wvn_project_render_fmin(const wvn_render_node* nodes_dev, int n, const float* points, int points_batched, int npts, int C,
                            int H, int W, const float* value_dev, float value, void* stream) {
  return wvn_project_render_fmin_launch(nodes_dev, n, points, points_batched, npts, C, H, W, value_dev, value, (hipStream_t)stream);
}
size_t wvn_wire_bytes(int H, int W, int S, int D) { return (H > 0 && W > 0 && S > 0 && D > 0) ? wvn_wire_bytes_impl(H, W, S, D) : 0; }
int wvn_wire_pack(const void* seg, int seg_is_i64, const float* feat, int ldf, void* out, int H, int W, int S, int D, void* stream) {
  return wvn_wire_pack_launch(seg, seg_is_i64, feat, ldf, out, H, W, S, D, (hipStream_t)stream);
}
int wvn_wire_unpack(const void* in, long long* seg_i64, int* seg_i32, float* feat, int H, int W, int S, int D, void* stream) {
  return wvn_wire_unpack_launch(in, seg_i64, seg_i32, feat, H, W, S, D, (hipStream_t)stream);
}
int wvn_slic_num_clusters(int H, int W, int num_components) {
  return (H > 0 && W > 0 && num_components > 0) ? wvn_slic_num_clusters_impl(H, W, num_components) : 0;
}
size_t wvn_slic_scratch_bytes(int H, int W, int num_components) {
  return (H > 0 && W > 0 && num_components > 0) ? wvn_slic_scratch_bytes_impl(H, W, num_components) : 0;
}
int wvn_slic(const void* img, int img_is_u8, int H, int W, int num_components, float compactness, int iters, const int* lut_lin,
             const int* lut_f, int* labels, void* scratch, size_t scratch_bytes, void* stream) {
  return wvn_slic_launch(img, img_is_u8, H, W, num_components, compactness, iters, lut_lin, lut_f, labels, scratch, scratch_bytes,
                         (hipStream_t)stream);
}
size_t wvn_slic_connectivity_scratch_bytes(int B, int H, int W, int K) { return wvn_slic_connectivity_scratch_bytes_impl(B, H, W, K); }
int wvn_slic_connectivity(const int* labels_in, int* labels_out, int B, int H, int W, int K, int min_size, void* scratch,
                          size_t scratch_bytes, void* stream) {
  return wvn_slic_connectivity_launch(labels_in, labels_out, B, H, W, K, min_size, scratch, scratch_bytes, (hipStream_t)stream);
}
int wvn_dense_sift(const void* img, int img_is_u8, float* out, int B, int C, int H, int W, void* stream) {
  return wvn_dense_sift_launch(img, img_is_u8, out, B, C, H, W, (hipStream_t)stream);
}
int wvn_dense_sift_segpool(const void* img, int img_is_u8, const int* seg, float* feat, int* cnt, void* scratch_sum, int B, int C,
                           int H, int W, int S, void* stream) {
  return wvn_dense_sift_segpool_launch(img, img_is_u8, seg, feat, cnt, scratch_sum, B, C, H, W, S, (hipStream_t)stream);
}
int wvn_seg_centers(const int* seg, float* centers, void* scratch, int H, int W, int S, void* stream) {
  return wvn_centers_launch(seg, centers, (unsigned long long*)scratch, H, W, S, (hipStream_t)stream);
}
int wvn_seg_adjacency(const int* seg, long long* edges, int* count, unsigned char* scratch_bitmap, int H, int W, int S,
                      int max_edges, void* stream) {
  return wvn_adjacency_launch(seg, edges, count, scratch_bitmap, H, W, S, max_edges, (hipStream_t)stream);
}
int wvn_seg_adjacency_batched(const int* seg, unsigned char* adj, int B, int H, int W, int S, void* stream) {
  return wvn_adjacency_batched_launch(seg, adj, B, H, W, S, (hipStream_t)stream);
}
int wvn_normalize_rows(const float* code, int ldc, float* xn, int rows, int C, void* stream) {
  return wvn_normalize_rows_launch(code, ldc, xn, rows, C, (hipStream_t)stream);
}
int wvn_argmax_rows(const float* x, int ld, int rows, int cols, int* out, void* stream) {
  return wvn_argmax_rows_launch(x, ld, rows, cols, out, (hipStream_t)stream);
}
size_t wvn_kmeans_scratch_bytes(int B, int P, int C, int K) {
  return (B > 0 && P > 0 && C > 0 && K > 0) ? wvn_kmeans_scratch_floats(B, P, C, K) * sizeof(float) : 0;
}
size_t wvn_kmeans_pixels_scratch_bytes(int B, int G, int H, int C, int K) {
  return (B > 0 && G > 0 && H > 0 && C > 0 && K > 0) ? wvn_kmeans_pixels_scratch_floats(B, G, H, C, K) * sizeof(float) : 0;
}
int wvn_kmeans_cosine_pixels(const float* code, int* labels, int* nseg, void* scratch, int B, int G, int H, int C, int K, int iters,
                             int relabel, void* stream) {
  return wvn_kmeans_pixels_launch(code, labels, nseg, (float*)scratch, B, G, H, C, K, iters, relabel, (hipStream_t)stream);
}
int wvn_kmeans_pixels_linear_supported_shape(int G, int H, int C, int K) { return wvn_kmeans_pixels_linear_supported(G, H, C, K); }
size_t wvn_kmeans_pixels_linear_scratch_bytes(int B, int G, int H, int C, int K) {
  return (B > 0 && wvn_kmeans_pixels_linear_supported(G, H, C, K)) ? wvn_kmeans_pixels_linear_scratch_floats(B, G, H, C, K) * sizeof(float) : 0;
}
int wvn_kmeans_cosine_pixels_linear(const float* code, int* labels, int* nseg, void* scratch, int B, int G, int H, int C, int K,
                                    int iters, int relabel, void* stream) {
  return wvn_kmeans_pixels_linear_launch(code, labels, nseg, (float*)scratch, B, G, H, C, K, iters, relabel, (hipStream_t)stream);
}
int wvn_kmeans_cosine_pixels_linear_ac(const float* code, int* labels, int* nseg, void* scratch, int B, int G, int H, int C, int K,
                                       int iters, int relabel, int align_corners, void* stream) {
  return wvn_kmeans_pixels_linear_launch(code, labels, nseg, (float*)scratch, B, G, H, C, K, iters, relabel, (hipStream_t)stream, align_corners ? 1 : 0);
}
int wvn_table_bilerp_argmax_ac(const float* table, int* labels, int B, int G, int H, int K, int align_corners, void* stream) {
  return wvn_table_bilerp_argmax_launch(table, labels, B, G, H, K, (hipStream_t)stream, align_corners ? 1 : 0);
}
int wvn_table_argmax_slots(int K) { return wvn_table_slots(K); }
int wvn_table_bilerp_argmax(const float* table, int* labels, int B, int G, int H, int K, void* stream) {
  return wvn_table_bilerp_argmax_launch(table, labels, B, G, H, K, (hipStream_t)stream);
}
int wvn_debug_kmeans_linear_rows(int rc) { wvn_kmeans_pixels_linear_set_rows(rc); return WVN_OK; }
int wvn_flip_average(const float* a, const float* mirrored, float* out, int B, int G, int C, int ld_src, void* stream) {
  return wvn_flip_average_launch(a, mirrored, out, B, G, C, ld_src, (hipStream_t)stream);
}
int wvn_kmeans_cosine(const float* xn, int* labels, int* nseg, void* scratch, int B, int P, int C, int K, int iters,
                      int relabel, void* stream) {
  return wvn_kmeans_launch(xn, labels, nseg, (float*)scratch, B, P, C, K, iters, relabel, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// traversability MLP
// ---------------------------------------------------------------------------------------------
namespace {
MlpOff mlp_off(const wvn_mlp_desc* d) {
  MlpOff o;
  o.O = 1 + d->D;
  o.W1 = 0; o.b1 = o.W1 + (size_t)d->H1 * d->D; o.W2 = o.b1 + d->H1; o.b2 = o.W2 + (size_t)d->H2 * d->H1;
  o.W3 = o.b2 + d->H2; o.b3 = o.W3 + (size_t)o.O * d->H2; o.total = o.b3 + o.O;
  return o;
}
int mlp_splitk(int R) { int s = (R + 511) / 512; return s < 1 ? 1 : (s > 32 ? 32 : s); }
bool is_double(const wvn_mlp_desc* d) { return d->reserved == WVN_MLP_KIND_DOUBLE; }   // DoubleMLP (kernels in double_mlp.hip)
// The workspace of a step, for both models: DoubleMLP's activations hold the two networks side by side, [R][2 h1] and [R][2 h2]
struct MlpWs { float *h1, *h2, *out, *lr, *g_out, *g_h2, *g_h1, *trav_w, *trav_raw, *part; void* fused; size_t total; };
int mlp_row_tile(const wvn_mlp_desc* d) { return is_double(d) ? wvn_dmlp_row_tile() : wvn_mlp_train_row_tile(); }
MlpWs mlp_carve(const wvn_mlp_desc* d, int R, void* base) {
  MlpWs w;
  size_t off = 0;
  const int nets = is_double(d) ? 2 : 1, O = 1 + d->D, N1 = nets * d->H1, N2 = nets * d->H2;
  auto take = [&](size_t n) { size_t o = off; off += align_up(n * sizeof(float), 256); return (float*)((char*)base + o); };
  w.h1 = take((size_t)R * N1); w.h2 = take((size_t)R * N2); w.out = take((size_t)R * O); w.lr = take(R);
  w.g_out = take((size_t)R * O); w.g_h2 = take((size_t)R * N2); w.g_h1 = take((size_t)R * N1);
  w.trav_w = take(R); w.trav_raw = take(R);
  size_t mx = (size_t)d->H1 * d->D;
  if ((size_t)d->H2 * d->H1 > mx) mx = (size_t)d->H2 * d->H1;
  const size_t m3 = (size_t)(is_double(d) ? d->D : O) * d->H2;   // the largest third-layer matrix: [1 + D][h2], DoubleMLP: networks.1's [D][h2]
  if (m3 > mx) mx = m3;
  w.part = take(mx * mlp_splitk(R));                                                      // split-K slabs of the general path
  w.fused = take(wvn_train_scratch_bytes(R, mlp_row_tile(d)) / sizeof(float) + 1);        // per-tile partials of the four-launch step
  w.total = off;
  return w;
}
// The fields of a step's argument block that both models fill alike (phase A stops at `fused`); fused: the per-tile partials of
// the four-launch step too
void train_args(TrainArgs& a, const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const unsigned char* y_valid, int R,
                const int* rows_dev, const double* stats, const MlpWs& w, const ConfArgs& conf, bool fused, const float* y = nullptr,
                float std_factor = 0.f, float w_trav = 0.f, float w_reco = 0.f, float* conf_out = nullptr, float* grads = nullptr) {
  a.P = params; a.x = x; a.ld_row = ldx; a.R = R; a.rows_dev = rows_dev; a.valid = y_valid; a.stats = (double*)stats;
  a.y = y; a.std_factor = std_factor; a.w_trav = w_trav; a.w_reco = w_reco; a.conf_out = conf_out; a.grads = grads;
  a.h1 = w.h1; a.h2 = w.h2; a.out = w.out; a.lr = w.lr; a.g_out = w.g_out; a.g_h2 = w.g_h2; a.g_h1 = w.g_h1;
  a.method = conf.method; a.balanced = conf.balanced; a.cstate = conf.state; a.minmax = conf.minmax;
  if (fused) wvn_train_scratch_carve(w.fused, R, mlp_row_tile(d), &a.part, &a.part_mm);
}
bool fused_ok(const wvn_mlp_desc* d, int R) {
  return is_double(d) ? wvn_dmlp_fused_ok(d->D, d->H1, d->H2, R) : wvn_mlp_train_fused_ok(d->D, d->H1, d->H2, R);
}
int mlp_fwd(const wvn_mlp_desc* d, const float* P, const float* x, int ldx, int R, float* out, float* h1, float* h2,
            hipStream_t st) {
  const MlpOff o = mlp_off(d);
  GemmF32Params p{};
  p.batch = 1; p.splitk = 1; p.transB = 1;
  p.A = x; p.lda = ldx; p.B = P + o.W1; p.ldb = d->D; p.bias = P + o.b1; p.C = h1; p.ldc = d->H1; p.M = R; p.N = d->H1; p.K = d->D;
  RET_IF(wvn_gemm_f32_launch(p, F32_EPI_RELU, st));
  p.A = h1; p.lda = d->H1; p.B = P + o.W2; p.ldb = d->H1; p.bias = P + o.b2; p.C = h2; p.ldc = d->H2; p.N = d->H2; p.K = d->H1;
  RET_IF(wvn_gemm_f32_launch(p, F32_EPI_RELU, st));
  p.A = h2; p.lda = d->H2; p.B = P + o.W3; p.ldb = d->H2; p.bias = P + o.b3; p.C = out; p.ldc = o.O; p.N = o.O; p.K = d->H2;
  RET_IF(wvn_gemm_f32_launch(p, F32_EPI_SIGMOID0, st));
  return WVN_OK;
}
// dW[M,N] = G^T[M,R] * Hm[R,N] via deterministic split-K
int mlp_wgrad(const float* G, int ldg, const float* Hm, int ldh, int M, int N, int R, float* part, float* dst,
              hipStream_t st) {
  const int sk = mlp_splitk(R);
  GemmF32Params p{};
  p.batch = 1; p.splitk = sk; p.A = G; p.lda = ldg; p.transA = 1; p.B = Hm; p.ldb = ldh; p.transB = 0;
  p.C = sk > 1 ? part : dst; p.ldc = N; p.M = M; p.N = N; p.K = R;
  RET_IF(wvn_gemm_f32_launch(p, F32_EPI_NONE, st));
  if (sk > 1) RET_IF(wvn_splitk_reduce_launch(part, sk, (size_t)M * N, nullptr, N, dst, st));
  return WVN_OK;
}

// the general path of DoubleMLP's phase B behind the gradient seed: its own data-path kernel, split-K GEMMs per network
int dmlp_general_bwd(DmlpArgs& a, const MlpWs& w, int ldx, hipStream_t st) {
  const DmlpGeom& g = a.g;
  const int D = g.D, O = 1 + D, H1 = g.H1, H2 = g.H2, R = a.R;
  a.seed_given = 1;
  RET_IF(wvn_dmlp_bwd_launch(a, st));
  for (int net = 0; net < 2; ++net) {   // column 0 of the seed belongs to networks.0, columns 1 .. D to networks.1
    const int M3 = net ? D : 1;
    RET_IF(mlp_wgrad(w.g_out + net, O, w.h2 + net * H2, 2 * H2, M3, H2, R, w.part, a.grads + g.W3[net], st));
    RET_IF(wvn_colsum_launch(w.g_out + net, O, R, M3, a.grads + g.b3[net], st));
    RET_IF(mlp_wgrad(w.g_h2 + net * H2, 2 * H2, w.h1 + net * H1, 2 * H1, H2, H1, R, w.part, a.grads + g.W2[net], st));
    RET_IF(wvn_colsum_launch(w.g_h2 + net * H2, 2 * H2, R, H2, a.grads + g.b2[net], st));
    RET_IF(mlp_wgrad(w.g_h1 + net * H1, 2 * H1, a.x, ldx, H1, D, R, w.part, a.grads + g.W1[net], st));
    RET_IF(wvn_colsum_launch(w.g_h1 + net * H1, 2 * H1, R, H1, a.grads + g.b1[net], st));
  }
  return WVN_OK;
}
size_t mlp_total(const wvn_mlp_desc* d) { return is_double(d) ? wvn_dmlp_geom(d->D, d->H1, d->H2).total : mlp_off(d).total; }
}  // namespace

int wvn_double_mlp_row_tile(void) { return wvn_dmlp_row_tile(); }
int wvn_double_mlp_fused_ok(const wvn_mlp_desc* d, int rows) {
  return d && is_double(d) && wvn_dmlp_fused_ok(d->D, d->H1, d->H2, rows) ? 1 : 0;
}

size_t wvn_mlp_param_count(const wvn_mlp_desc* d) { return d ? mlp_total(d) : 0; }
size_t wvn_mlp_workspace_bytes(const wvn_mlp_desc* d, int rows) {
  if (!d || rows <= 0) return 0;
  if (is_double(d) && !wvn_dmlp_supported(d->D, d->H1, d->H2)) return 0;
  return mlp_carve(d, rows, nullptr).total;
}

int wvn_mlp_forward(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, int R, float* out, float* h1,
                    float* h2, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !params || !x || !out || R <= 0) return WVN_ERR_ARG;
  if (is_double(d)) {   // one launch, nothing but out (and h1 [R][2 H1] / h2 [R][2 H2] where asked for) leaves the chip
    if (ldx < d->D || (h1 == nullptr) != (h2 == nullptr)) return WVN_ERR_ARG;
    DmlpArgs a{};
    a.P = params; a.g = wvn_dmlp_geom(d->D, d->H1, d->H2);
    a.x = x; a.ld_row = ldx; a.S = R; a.R = R; a.out = out; a.h1 = h1; a.h2 = h2;
    return wvn_dmlp_fwd_launch(a, (hipStream_t)stream);
  }
  if (!h1 || !h2) {
    if (!workspace) return WVN_ERR_ARG;
    MlpWs w = mlp_carve(d, R, workspace);
    if (w.total > workspace_bytes) return WVN_ERR_WORKSPACE;
    if (!h1) h1 = w.h1;
    if (!h2) h2 = w.h2;
  }
  return mlp_fwd(d, params, x, ldx, R, out, h1, h2, (hipStream_t)stream);
}

int wvn_compact_segment_rows(const float* feat, int D, const float* side, int Dside, const int* nseg, int B, int S, float* x_out,
                             float* side_out, int* rows_dev, void* stream) {
  return wvn_compact_segment_rows_launch(feat, D, side, Dside, nseg, B, S, x_out, side_out, rows_dev, (hipStream_t)stream);
}

namespace {
int mlp_phase_a(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const unsigned char* y_valid, int R,
                const int* rows_dev, double* stats, void* workspace, size_t workspace_bytes, unsigned int* sync_word, void* stream,
                const ConfArgs& conf) {
  if (!d || !params || !x || !y_valid || !stats || !workspace || R <= 0) return WVN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (is_double(d) && (!wvn_dmlp_supported(d->D, d->H1, d->H2) || ldx < d->D)) return WVN_ERR_ARG;
  const MlpWs w = mlp_carve(d, R, workspace);
  if (w.total > workspace_bytes) return WVN_ERR_WORKSPACE;
  const bool fused = sync_word && fused_ok(d, R);   // the four-launch step: forward + statistic in one launch
  if (is_double(d)) {
    DmlpArgs a{};
    train_args(a, d, params, x, ldx, y_valid, R, rows_dev, stats, w, conf, fused);
    a.g = wvn_dmlp_geom(d->D, d->H1, d->H2); a.S = R; a.ticket = sync_word;
    if (!fused) a.lr = nullptr;   // (the stage kernel below forms the row losses)
    RET_IF(wvn_dmlp_fwd_launch(a, st));
  } else if (fused) {
    MlpTrainArgs a{};
    train_args(a, d, params, x, ldx, y_valid, R, rows_dev, stats, w, conf, fused);
    a.o = mlp_off(d); a.D = d->D; a.ticket = sync_word;
    RET_IF(wvn_mlp_train_fwd_launch(a, st));
  } else {
    RET_IF(mlp_fwd(d, params, x, ldx, R, w.out, w.h1, w.h2, st));
  }
  return fused ? WVN_OK : wvn_mlp_rowloss_stats_launch(w.out, 1 + d->D, x, ldx, y_valid, w.lr, stats, R, d->D, st, rows_dev, conf);
}

// wvn_conf_desc -> ConfArgs, checked on the host before any GPU call
int conf_args(const wvn_conf_desc* c, ConfArgs* a) {
  if (!c || !c->state || c->method < WVN_CONF_LATEST_MEASUREMENT || c->method > WVN_CONF_MOVING_AVERAGE) return WVN_ERR_ARG;
  if (c->method == WVN_CONF_MOVING_AVERAGE && !c->minmax) return WVN_ERR_ARG;
  a->method = c->method;
  a->balanced = c->balanced != 0;
  a->state = c->state;
  a->minmax = c->method == WVN_CONF_MOVING_AVERAGE ? c->minmax : nullptr;
  return WVN_OK;
}
}  // namespace

int wvn_mlp_train_phase_a_rows(const wvn_mlp_desc* d, const float* params, const float* x, int ldx,
                               const unsigned char* y_valid, int R, const int* rows_dev, double* stats, void* workspace,
                               size_t workspace_bytes, unsigned int* sync_word, void* stream) {
  return mlp_phase_a(d, params, x, ldx, y_valid, R, rows_dev, stats, workspace, workspace_bytes, sync_word, stream, ConfArgs());
}
int wvn_mlp_train_phase_a_conf(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const unsigned char* y_valid,
                               int R, const int* rows_dev, double* stats, void* workspace, size_t workspace_bytes,
                               unsigned int* sync_word, const wvn_conf_desc* conf, void* stream) {
  ConfArgs a;
  RET_IF(conf_args(conf, &a));
  return mlp_phase_a(d, params, x, ldx, y_valid, R, rows_dev, stats, workspace, workspace_bytes, sync_word, stream, a);
}
int wvn_mlp_train_phase_a(const wvn_mlp_desc* d, const float* params, const float* x, int ldx,
                          const unsigned char* y_valid, int R, double* stats, void* workspace, size_t workspace_bytes,
                          void* stream) {
  return wvn_mlp_train_phase_a_rows(d, params, x, ldx, y_valid, R, nullptr, stats, workspace, workspace_bytes, nullptr, stream);
}

int wvn_mlp_train_phase_b(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const float* y,
                          const unsigned char* y_valid, int R, const double* stats, float std_factor, float w_trav,
                          float w_reco, float* grads, float* confidence_out, void* workspace, size_t workspace_bytes,
                          void* stream) {
  return wvn_mlp_train_phase_b_rows(d, params, x, ldx, y, y_valid, R, nullptr, stats, std_factor, w_trav, w_reco, grads,
                                    confidence_out, workspace, workspace_bytes, 0, stream);
}

namespace {
int mlp_phase_b(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const float* y, const unsigned char* y_valid,
                int R, const int* rows_dev, const double* stats, float std_factor, float w_trav, float w_reco, float* grads,
                float* confidence_out, void* workspace, size_t workspace_bytes, int fused, void* stream, const ConfArgs& conf) {
  if (!d || !params || !x || !y || !y_valid || !stats || !grads || !workspace || R <= 0) return WVN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool dbl = is_double(d);
  if (dbl && (!wvn_dmlp_supported(d->D, d->H1, d->H2) || ldx < d->D)) return WVN_ERR_ARG;
  const MlpWs w = mlp_carve(d, R, workspace);
  if (w.total > workspace_bytes) return WVN_ERR_WORKSPACE;
  const bool four = fused && fused_ok(d, R);   // (phase A of this step ran the fused forward on this workspace)
  const MlpOff o = mlp_off(d);
  const int O = o.O;
  if (!four)   // the general path of both models starts from the stage kernel's gradient seed and loss sums
    RET_IF(wvn_mlp_gradout_launch(w.out, O, x, ldx, y, y_valid, w.lr, stats, std_factor, w_trav, w_reco, w.g_out, O, w.trav_w,
                                  w.trav_raw, confidence_out, grads + mlp_total(d), R, d->D, st, rows_dev, conf));
  if (dbl) {
    DmlpArgs a{};
    train_args(a, d, params, x, ldx, y_valid, R, rows_dev, stats, w, conf, four, y, std_factor, w_trav, w_reco, confidence_out, grads);
    a.g = wvn_dmlp_geom(d->D, d->H1, d->H2); a.S = R;
    if (!four) return dmlp_general_bwd(a, w, ldx, st);
    RET_IF(wvn_dmlp_bwd_launch(a, st));
    return wvn_dmlp_wgrad_launch(a, st);
  }
  if (four) {
    MlpTrainArgs a{};
    train_args(a, d, params, x, ldx, y_valid, R, rows_dev, stats, w, conf, four, y, std_factor, w_trav, w_reco, confidence_out, grads);
    a.o = o; a.D = d->D;
    return wvn_mlp_train_bwd_launch(a, st);
  }
  // layer 3
  RET_IF(mlp_wgrad(w.g_out, O, w.h2, d->H2, O, d->H2, R, w.part, grads + o.W3, st));
  RET_IF(wvn_colsum_launch(w.g_out, O, R, O, grads + o.b3, st));
  {
    GemmF32Params p{};
    p.batch = 1; p.splitk = 1; p.A = w.g_out; p.lda = O; p.B = params + o.W3; p.ldb = d->H2; p.transB = 0;
    p.C = w.g_h2; p.ldc = d->H2; p.M = R; p.N = d->H2; p.K = O; p.mask = w.h2; p.ldmask = d->H2;
    RET_IF(wvn_gemm_f32_launch(p, F32_EPI_RELUMASK, st));
  }
  // layer 2
  RET_IF(mlp_wgrad(w.g_h2, d->H2, w.h1, d->H1, d->H2, d->H1, R, w.part, grads + o.W2, st));
  RET_IF(wvn_colsum_launch(w.g_h2, d->H2, R, d->H2, grads + o.b2, st));
  {
    GemmF32Params p{};
    p.batch = 1; p.splitk = 1; p.A = w.g_h2; p.lda = d->H2; p.B = params + o.W2; p.ldb = d->H1; p.transB = 0;
    p.C = w.g_h1; p.ldc = d->H1; p.M = R; p.N = d->H1; p.K = d->H2; p.mask = w.h1; p.ldmask = d->H1;
    RET_IF(wvn_gemm_f32_launch(p, F32_EPI_RELUMASK, st));
  }
  // layer 1
  RET_IF(mlp_wgrad(w.g_h1, d->H1, x, ldx, d->H1, d->D, R, w.part, grads + o.W1, st));
  RET_IF(wvn_colsum_launch(w.g_h1, d->H1, R, d->H1, grads + o.b1, st));
  return WVN_OK;
}
}  // namespace

int wvn_mlp_train_phase_b_rows(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const float* y,
                               const unsigned char* y_valid, int R, const int* rows_dev, const double* stats, float std_factor,
                               float w_trav, float w_reco, float* grads, float* confidence_out, void* workspace,
                               size_t workspace_bytes, int fused, void* stream) {
  return mlp_phase_b(d, params, x, ldx, y, y_valid, R, rows_dev, stats, std_factor, w_trav, w_reco, grads, confidence_out, workspace,
                     workspace_bytes, fused, stream, ConfArgs());
}
int wvn_mlp_train_phase_b_conf(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const float* y,
                               const unsigned char* y_valid, int R, const int* rows_dev, const double* stats, float std_factor,
                               float w_trav, float w_reco, float* grads, float* confidence_out, void* workspace,
                               size_t workspace_bytes, int fused, const wvn_conf_desc* conf, void* stream) {
  ConfArgs a;
  RET_IF(conf_args(conf, &a));
  return mlp_phase_b(d, params, x, ldx, y, y_valid, R, rows_dev, stats, std_factor, w_trav, w_reco, grads, confidence_out, workspace,
                     workspace_bytes, fused, stream, a);
}

int wvn_mlp_train_phase_c(const wvn_mlp_desc* d, float* params, const float* grads, float* adam_m, float* adam_v,
                          int step, float lr, const double* stats, float w_trav, float w_reco, float* losses,
                          void* stream) {
  if (!d || !params || !grads || !adam_m || !adam_v || !stats || step <= 0) return WVN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t total = mlp_total(d);
  // Adam and the step's losses in ONE launch
  return wvn_adam_launch(params, grads, adam_m, adam_v, (int)total, step, lr, 0.9f, 0.999f, 1e-8f, st, stats, grads + total, w_trav,
                         w_reco, losses);
}
int wvn_mlp_train_phase_c_conf(const wvn_mlp_desc* d, float* params, const float* grads, float* adam_m, float* adam_v, int step,
                               float lr, const double* stats, float w_trav, float w_reco, float* losses, const wvn_conf_desc* conf,
                               void* stream) {
  ConfArgs a;
  RET_IF(conf_args(conf, &a));
  if (!d || !params || !grads || !adam_m || !adam_v || !stats || !losses || step <= 0) return WVN_ERR_ARG;   // (losses: the commit rides on it)
  const size_t total = mlp_total(d);
  return wvn_adam_launch(params, grads, adam_m, adam_v, (int)total, step, lr, 0.9f, 0.999f, 1e-8f, (hipStream_t)stream, stats,
                         grads + total, w_trav, w_reco, losses, a);
}

// fused per-pixel inference (pixel_mlp.hip)
size_t wvn_pixel_mlp_pack_bytes(const wvn_mlp_desc* d) {
  if (!d || d->reserved != 0 || d->H1 != 256 || d->H2 != 32) return 0;
  return wvn_pixel_mlp_pack_bytes_impl(d->D);
}
int wvn_pixel_mlp_zx_cols(const wvn_mlp_desc* d) {
  if (!d || d->reserved != 0 || d->H1 != 256 || d->H2 != 32) return 0;
  return wvn_pixel_mlp_zx_cols_impl(d->D);
}
int wvn_pixel_mlp_pack(const wvn_mlp_desc* d, const float* params, void* packed, void* stream) {
  if (!d || d->reserved != 0) return WVN_ERR_ARG;
  return wvn_pixel_mlp_pack_launch(d->D, d->H1, d->H2, params, packed, (hipStream_t)stream);
}
int wvn_pixel_mlp_infer(const wvn_mlp_desc* d, const void* packed, void* zx, int ldzx, int batch, int grid, int out_h,
                        int out_w, float mean, float std, float std_factor, const float* conf_state, float* trav,
                        float* conf, float* loss_reco, void* stream) {
  if (!d || d->reserved != 0) return WVN_ERR_ARG;
  return wvn_pixel_mlp_infer_launch(d->D, d->H1, d->H2, packed, zx, ldzx, batch, grid, out_h, out_w, mean, std, std_factor,
                                    conf_state, trav, conf, loss_reco, (hipStream_t)stream);
}

size_t wvn_pixel_mlp_exact_pack_bytes(const wvn_mlp_desc* d) {
  if (!d || d->reserved != 0 || d->H1 != 256 || d->H2 != 32) return 0;
  return wvn_pixel_mlp_exact_pack_bytes_impl(d->D);
}
size_t wvn_pixel_mlp_exact_workspace_bytes(const wvn_mlp_desc* d, int batch, int grid) {
  if (!d || d->reserved != 0 || d->H1 != 256 || d->H2 != 32 || batch <= 0 || grid <= 0) return 0;
  return wvn_pixel_mlp_exact_workspace_bytes_impl(d->D, batch, grid);
}
int wvn_pixel_mlp_exact_pack(const wvn_mlp_desc* d, const float* params, void* packed, void* stream) {
  if (!d || d->reserved != 0) return WVN_ERR_ARG;
  return wvn_pixel_mlp_exact_pack_launch(d->D, d->H1, d->H2, params, packed, (hipStream_t)stream);
}
int wvn_pixel_mlp_infer_exact(const wvn_mlp_desc* d, const float* params, const void* packed, const float* tokens,
                              int ld_tokens, int batch, int grid, int out_h, int out_w, float mean, float std,
                              float std_factor, const float* conf_state, float* trav, float* conf, float* loss_reco,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || d->reserved != 0) return WVN_ERR_ARG;
  return wvn_pixel_mlp_infer_exact_launch(d->D, d->H1, d->H2, params, packed, tokens, ld_tokens, batch, grid, out_h, out_w,
                                          mean, std, std_factor, conf_state, trav, conf, loss_reco, workspace,
                                          workspace_bytes, (hipStream_t)stream);
}

// LinearRnvp forward flow (rnvp.hip): every check is host arithmetic, a refused call launches nothing
size_t wvn_rnvp_pack_bytes(const wvn_rnvp_desc* d) {
  if (!d || !wvn_rnvp_supported(d->D, d->h, d->flows)) return 0;
  return wvn_rnvp_pack_bytes_impl(d->D, d->h);
}
int wvn_rnvp_row_tile(void) { return wvn_rnvp_row_tile_impl(); }
int wvn_rnvp_pack(const wvn_rnvp_desc* d, const float* params, const float* mask, const long long* perm, void* packed, void* stream) {
  if (!d || !wvn_rnvp_supported(d->D, d->h, d->flows) || !params || !mask || !perm || !packed || ((uintptr_t)packed & 15)) return WVN_ERR_ARG;
  return wvn_rnvp_pack_launch(d->D, d->h, params, mask, perm, packed, (hipStream_t)stream);
}
int wvn_rnvp_forward_rows(const wvn_rnvp_desc* d, const void* packed, const float* x, int ldx, long long R, float mean, float std,
                          float std_factor, const float* conf_state, float* score, float* conf, float* log_det, float* z, int ldz,
                          void* stream) {
  if (!d || !wvn_rnvp_supported(d->D, d->h, d->flows) || !packed || ((uintptr_t)packed & 15) || !x || !score) return WVN_ERR_ARG;
  if (ldx < d->D || R <= 0 || R > 0x7fffffffll || (z && ldz < d->D)) return WVN_ERR_ARG;
  RnvpCall c{};
  c.D = d->D; c.h = d->h; c.packed = packed;
  c.x = x; c.ldx = ldx; c.R = R;
  c.mean = mean; c.std = std; c.std_factor = std_factor; c.conf_dev = conf_state;
  c.score = score; c.conf = conf; c.log_det = log_det; c.z = z; c.ldz = ldz;
  return wvn_rnvp_forward_launch(c, (hipStream_t)stream);
}
int wvn_rnvp_forward_pixels(const wvn_rnvp_desc* d, const void* packed, const float* tokens, int ld_tokens, int batch, int grid,
                            int out_h, int out_w, float mean, float std, float std_factor, const float* conf_state, float* score,
                            float* conf, float* log_det, float* z, int ldz, void* stream) {
  if (!d || !wvn_rnvp_supported(d->D, d->h, d->flows) || !packed || ((uintptr_t)packed & 15) || !tokens || !score) return WVN_ERR_ARG;
  if (ld_tokens < d->D || batch <= 0 || grid < 2 || grid > 4096 || out_h < 2 || out_w < 2 || (z && ldz < d->D)) return WVN_ERR_ARG;
  const long long R = (long long)batch * out_h * out_w;
  if (R > 0x7fffffffll) return WVN_ERR_ARG;
  RnvpCall c{};
  c.D = d->D; c.h = d->h; c.packed = packed;
  c.tokens = tokens; c.ldt = ld_tokens; c.B = batch; c.G = grid; c.Ho = out_h; c.Wo = out_w; c.R = R;
  c.mean = mean; c.std = std; c.std_factor = std_factor; c.conf_dev = conf_state;
  c.score = score; c.conf = conf; c.log_det = log_det; c.z = z; c.ldz = ldz;
  return wvn_rnvp_forward_launch(c, (hipStream_t)stream);
}

// LinearRnvp training step (rnvp_train.hip): every check is host arithmetic, a refused call launches nothing
static bool rnvp_ok(const wvn_rnvp_desc* d) { return d && wvn_rnvp_supported(d->D, d->h, d->flows); }
static const long long RNVP_TRAIN_MAX_ROWS = 1ll << 16;   // the weight gradients walk the row tiles un-split
size_t wvn_rnvp_train_param_count(const wvn_rnvp_desc* d) { return rnvp_ok(d) ? wvn_rnvp_train_param_count_impl(d->D, d->h) : 0; }
size_t wvn_rnvp_train_workspace_bytes(const wvn_rnvp_desc* d, long long R) {
  if (!rnvp_ok(d) || R < 0 || R > RNVP_TRAIN_MAX_ROWS) return 0;
  return wvn_rnvp_train_workspace_bytes_impl(d->D, d->h, R);
}
size_t wvn_rnvp_train_pack_bytes(const wvn_rnvp_desc* d) { return rnvp_ok(d) ? wvn_rnvp_train_pack_bytes_impl(d->D, d->h) : 0; }
int wvn_rnvp_train_pack(const wvn_rnvp_desc* d, const float* params, const void* packed, void* train_packed, void* stream) {
  if (!rnvp_ok(d) || !params || !packed || !train_packed || (((uintptr_t)packed | (uintptr_t)train_packed) & 15)) return WVN_ERR_ARG;
  return wvn_rnvp_train_pack_launch(d->D, d->h, params, packed, train_packed, (hipStream_t)stream);
}
int wvn_rnvp_train_phase_a(const wvn_rnvp_desc* d, const void* packed, const float* x, int ldx, long long R, float* score,
                           double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (!rnvp_ok(d) || !packed || ((uintptr_t)packed & 15) || !stats || !workspace || ((uintptr_t)workspace & 15)) return WVN_ERR_ARG;
  if (R < 0 || R > RNVP_TRAIN_MAX_ROWS || (R > 0 && (!x || !score || ldx < d->D))) return WVN_ERR_ARG;
  if (workspace_bytes < wvn_rnvp_train_workspace_bytes_impl(d->D, d->h, R)) return WVN_ERR_ARG;
  RnvpCall c{};
  c.D = d->D; c.h = d->h; c.packed = packed;
  c.x = x; c.ldx = ldx; c.R = R; c.score = score;
  return wvn_rnvp_train_phase_a_launch(c, stats, workspace, (hipStream_t)stream);
}
int wvn_rnvp_train_phase_b(const wvn_rnvp_desc* d, const void* packed, const void* train_packed, long long R, const double* stats,
                           float* grads, void* workspace, size_t workspace_bytes, void* stream) {
  if (!rnvp_ok(d) || !packed || !train_packed || (((uintptr_t)packed | (uintptr_t)train_packed) & 15) || !stats || !grads ||
      !workspace || ((uintptr_t)workspace & 15))
    return WVN_ERR_ARG;
  if (R < 0 || R > RNVP_TRAIN_MAX_ROWS || workspace_bytes < wvn_rnvp_train_workspace_bytes_impl(d->D, d->h, R)) return WVN_ERR_ARG;
  return wvn_rnvp_train_phase_b_launch(d->D, d->h, packed, train_packed, R, stats, grads, workspace, (hipStream_t)stream);
}
int wvn_rnvp_train_phase_c(const wvn_rnvp_desc* d, float* params, const float* grads, float* adam_m, float* adam_v, int step, float lr,
                           const double* stats, int method, double* conf_state, float* losses, const float* mask,
                           const long long* perm, void* packed, void* train_packed, void* stream) {
  if (!rnvp_ok(d) || !params || !grads || !adam_m || !adam_v || step <= 0 || !stats || !conf_state || !losses || !mask || !perm ||
      !packed || !train_packed || (((uintptr_t)packed | (uintptr_t)train_packed) & 15))
    return WVN_ERR_ARG;
  if (method < WVN_CONF_LATEST_MEASUREMENT || method > WVN_CONF_MOVING_AVERAGE) return WVN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = wvn_rnvp_train_param_count_impl(d->D, d->h);
  RET_IF(wvn_adam_launch(params, grads, adam_m, adam_v, (int)n, step, lr, 0.9f, 0.999f, 1e-8f, st, nullptr, nullptr, 0.f, 0.f, nullptr));
  RET_IF(wvn_rnvp_train_commit_launch(stats, method, conf_state, losses, st));
  RET_IF(wvn_rnvp_pack_launch(d->D, d->h, params, mask, perm, packed, st));
  return wvn_rnvp_train_pack_launch(d->D, d->h, params, packed, train_packed, st);
}

// fused per-segment inference (segment_predict.hip)
size_t wvn_segment_predict_workspace_bytes(const wvn_mlp_desc* d, int B, int S) {
  if (!d || B <= 0 || S <= 0) return 0;
  if (!(is_double(d) ? wvn_dmlp_supported(d->D, d->H1, d->H2) : wvn_segment_predict_supported(d->D, d->H1, d->H2))) return 0;
  if ((long long)B * S > (1ll << 26)) return 0;
  return wvn_segment_predict_workspace_bytes_impl(B, S);
}
int wvn_segment_predict(const wvn_mlp_desc* d, const float* params, const float* feat, int ld_row, long long ld_frame,
                        int B, int S, const void* seg, int seg_bytes, int H, int W, float mean, float std, float std_factor,
                        const float* conf_state, float* trav, float* conf, float* loss_reco, void* workspace,
                        size_t workspace_bytes, void* stream) {
  // every check is host arithmetic: a refused call touches no GPU state
  if (!d || !params || !feat || !seg || !workspace) return WVN_ERR_ARG;
  if (!(is_double(d) ? wvn_dmlp_supported(d->D, d->H1, d->H2) : wvn_segment_predict_supported(d->D, d->H1, d->H2))) return WVN_ERR_ARG;
  if (B <= 0 || S <= 0 || H <= 0 || W <= 0 || B > 65535) return WVN_ERR_ARG;
  if ((long long)B * S > (1ll << 26) || (long long)H * W > 0x7fffffffll) return WVN_ERR_ARG;
  if (seg_bytes != 4 && seg_bytes != 8) return WVN_ERR_ARG;
  if (ld_row < d->D || ld_frame < 0) return WVN_ERR_ARG;
  if (((uintptr_t)params | (uintptr_t)workspace) & 15) return WVN_ERR_ARG;
  if (((uintptr_t)seg & (seg_bytes - 1)) || ((uintptr_t)feat & 3)) return WVN_ERR_ARG;
  if (workspace_bytes < wvn_segment_predict_workspace_bytes_impl(B, S)) return WVN_ERR_WORKSPACE;
  if (is_double(d)) {   // the table from double_mlp.hip's forward, the paint of segment_predict.hip: two launches as well
    DmlpArgs a{};
    a.P = params; a.g = wvn_dmlp_geom(d->D, d->H1, d->H2);
    a.x = feat; a.ld_row = ld_row; a.ld_frame = ld_frame; a.S = S; a.R = B * S;
    a.table = (float*)workspace; a.mean = mean; a.std = std; a.std_factor = std_factor; a.conf_dev = conf_state;
    RET_IF(wvn_dmlp_fwd_launch(a, (hipStream_t)stream));
    return wvn_segment_paint_launch(a.table, B, S, seg, seg_bytes, H, W, trav, conf, loss_reco, (hipStream_t)stream);
  }
  return wvn_segment_predict_launch(d->D, params, feat, ld_row, ld_frame, B, S, seg, seg_bytes, H, W, mean, std, std_factor,
                                    conf_state, trav, conf, loss_reco, workspace, workspace_bytes, (hipStream_t)stream);
}

// SimpleGCN (simple_gcn.hip).  Every check is host arithmetic: a refused call touches no GPU state
namespace {
bool gcn_ok(const wvn_mlp_desc* d) { return d && d->reserved == 0 && wvn_gcn_supported(d->D, d->H1, d->H2); }
bool gcn_size_ok(long long nodes, long long capacity) { return nodes >= 1 && nodes <= (1ll << 26) && capacity >= nodes && capacity <= (1ll << 30); }
}  // namespace
size_t wvn_gcn_workspace_bytes(const wvn_mlp_desc* d, int nodes, long long capacity) {
  if (!gcn_ok(d) || !gcn_size_ok(nodes, capacity)) return 0;
  return wvn_gcn_workspace_bytes_impl(d->H1, d->H2, nodes, capacity);
}
int wvn_gcn_graph_from_edges(const long long* edge_index, long long ld_row, long long ld_edge, int E, int nodes, long long capacity,
                             int* bad_edges, void* workspace, size_t workspace_bytes, void* stream) {
  if (!bad_edges || !workspace || E < 0 || (E > 0 && !edge_index) || !gcn_size_ok(nodes, capacity)) return WVN_ERR_ARG;
  if (capacity < (long long)E + nodes) return WVN_ERR_ARG;
  if (((uintptr_t)edge_index & 7) || ((uintptr_t)workspace & 15) || ((uintptr_t)bad_edges & 3)) return WVN_ERR_ARG;
  if (workspace_bytes < wvn_gcn_workspace_bytes_impl(0, 0, nodes, capacity)) return WVN_ERR_WORKSPACE;
  return wvn_gcn_graph_edges_launch(edge_index, ld_row, ld_edge, E, nodes, capacity, bad_edges, workspace, (hipStream_t)stream);
}
int wvn_gcn_graph_from_bitmaps(const unsigned char* adj, long long ld_b, long long ld_l, long long ld_r, int B, int S, long long capacity,
                               int* bad_edges, void* workspace, size_t workspace_bytes, void* stream) {
  if (!adj || !workspace || B < 1 || S < 1 || ld_b < 0 || ld_l < 0 || ld_r < 0) return WVN_ERR_ARG;
  if (!gcn_size_ok((long long)B * S, capacity) || capacity < (long long)B * S * S) return WVN_ERR_ARG;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)bad_edges & 3)) return WVN_ERR_ARG;
  if (workspace_bytes < wvn_gcn_workspace_bytes_impl(0, 0, B * S, capacity)) return WVN_ERR_WORKSPACE;
  return wvn_gcn_graph_bitmaps_launch(adj, ld_b, ld_l, ld_r, B, S, capacity, bad_edges, workspace, (hipStream_t)stream);
}
int wvn_gcn_forward(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, int nodes, long long capacity, float* out,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!gcn_ok(d) || !params || !x || !out || !workspace || !gcn_size_ok(nodes, capacity) || ldx < d->D) return WVN_ERR_ARG;
  if (((uintptr_t)workspace & 15) || (((uintptr_t)params | (uintptr_t)x | (uintptr_t)out) & 3)) return WVN_ERR_ARG;
  if (workspace_bytes < wvn_gcn_workspace_bytes_impl(d->H1, d->H2, nodes, capacity)) return WVN_ERR_WORKSPACE;
  return wvn_gcn_layers_launch(d->D, d->H1, d->H2, params, x, ldx, nodes, capacity, out, 1 + d->D, 0, 0.f, 1.f, 0.f, nullptr, workspace,
                               (hipStream_t)stream);
}
int wvn_gcn_segment_predict(const wvn_mlp_desc* d, const float* params, const float* feat, int ld_row, int B, int S, long long capacity,
                            const void* seg, int seg_bytes, int H, int W, float mean, float std, float std_factor,
                            const float* conf_state, float* trav, float* conf, float* loss_reco, void* workspace, size_t workspace_bytes,
                            void* stream) {
  if (!gcn_ok(d) || !params || !feat || !seg || !workspace) return WVN_ERR_ARG;
  if (B <= 0 || S <= 0 || H <= 0 || W <= 0 || B > 65535 || (long long)H * W > 0x7fffffffll) return WVN_ERR_ARG;
  if (!gcn_size_ok((long long)B * S, capacity) || ld_row < d->D) return WVN_ERR_ARG;
  if (seg_bytes != 4 && seg_bytes != 8) return WVN_ERR_ARG;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)seg & (seg_bytes - 1)) || (((uintptr_t)feat | (uintptr_t)params) & 3)) return WVN_ERR_ARG;
  if (workspace_bytes < wvn_gcn_workspace_bytes_impl(d->H1, d->H2, B * S, capacity)) return WVN_ERR_WORKSPACE;
  RET_IF(wvn_gcn_layers_launch(d->D, d->H1, d->H2, params, feat, ld_row, B * S, capacity, nullptr, 0, 1, mean, std, std_factor, conf_state,
                               workspace, (hipStream_t)stream));
  return wvn_segment_paint_launch(wvn_gcn_table(workspace, d->H1, d->H2, B * S, capacity), B, S, seg, seg_bytes, H, W, trav, conf,
                                  loss_reco, (hipStream_t)stream);
}

// SimpleGCN training step (simple_gcn_train.hip): phases A and B; phase C is wvn_mlp_train_phase_c(_conf) on the same descriptor
namespace {
const int GCN_TRAIN_MAX_NODES = 1 << 16;   // the weight gradients walk the rows un-split
bool gcn_train_size_ok(long long nodes, long long capacity) { return gcn_size_ok(nodes, capacity) && nodes <= GCN_TRAIN_MAX_NODES; }
int gcn_conf_args(const wvn_conf_desc* c, ConfArgs* a) { return c ? conf_args(c, a) : WVN_OK; }   // NULL: latest_measurement, balanced
}  // namespace
size_t wvn_gcn_train_workspace_bytes(const wvn_mlp_desc* d, int nodes, long long capacity) {
  if (!gcn_ok(d) || !gcn_train_size_ok(nodes, capacity)) return 0;
  return wvn_gcn_train_workspace_bytes_impl(d->D, d->H1, d->H2, nodes, capacity);
}
int wvn_gcn_train_saved(const wvn_mlp_desc* d, int nodes, long long capacity, size_t* offsets) {
  if (!gcn_ok(d) || !gcn_train_size_ok(nodes, capacity) || !offsets) return WVN_ERR_ARG;
  wvn_gcn_train_saved_offsets(d->D, d->H1, d->H2, nodes, capacity, offsets);
  return WVN_OK;
}
int wvn_gcn_train_phase_a(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const long long* edge_index, long long ld_row,
                          long long ld_edge, int E, const unsigned char* y_valid, int nodes, long long capacity, double* stats,
                          int* bad_edges, void* workspace, size_t workspace_bytes, unsigned int* sync_word, const wvn_conf_desc* conf,
                          void* stream) {
  ConfArgs a;
  RET_IF(gcn_conf_args(conf, &a));
  if (!gcn_ok(d) || !params || !x || !y_valid || !stats || !bad_edges || !workspace || !sync_word) return WVN_ERR_ARG;
  if (!gcn_train_size_ok(nodes, capacity) || ldx < d->D || E < 0 || (E > 0 && !edge_index) || capacity < (long long)E + nodes) return WVN_ERR_ARG;
  if (((uintptr_t)edge_index & 7) || ((uintptr_t)workspace & 15) || ((uintptr_t)stats & 7)) return WVN_ERR_ARG;
  if (((uintptr_t)params | (uintptr_t)x | (uintptr_t)bad_edges | (uintptr_t)sync_word) & 3) return WVN_ERR_ARG;
  if (workspace_bytes < wvn_gcn_train_workspace_bytes_impl(d->D, d->H1, d->H2, nodes, capacity)) return WVN_ERR_ARG;
  return wvn_gcn_train_phase_a_launch(d->D, d->H1, d->H2, params, x, ldx, edge_index, ld_row, ld_edge, E, y_valid, nodes, capacity, stats,
                                      bad_edges, workspace, sync_word, a, (hipStream_t)stream);
}
int wvn_gcn_train_phase_b(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const float* y, const unsigned char* y_valid,
                          int nodes, long long capacity, const double* stats, float std_factor, float w_trav, float w_reco, float* grads,
                          float* confidence_out, void* workspace, size_t workspace_bytes, const wvn_conf_desc* conf, void* stream) {
  ConfArgs a;
  RET_IF(gcn_conf_args(conf, &a));
  if (!gcn_ok(d) || !params || !x || !y || !y_valid || !stats || !grads || !workspace) return WVN_ERR_ARG;
  if (!gcn_train_size_ok(nodes, capacity) || ldx < d->D) return WVN_ERR_ARG;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)stats & 7)) return WVN_ERR_ARG;
  if (((uintptr_t)params | (uintptr_t)x | (uintptr_t)y | (uintptr_t)grads | (uintptr_t)confidence_out) & 3) return WVN_ERR_ARG;
  if (workspace_bytes < wvn_gcn_train_workspace_bytes_impl(d->D, d->H1, d->H2, nodes, capacity)) return WVN_ERR_ARG;
  return wvn_gcn_train_phase_b_launch(d->D, d->H1, d->H2, params, x, ldx, y, y_valid, nodes, capacity, stats, std_factor, w_trav, w_reco,
                                      grads, confidence_out, workspace, a, (hipStream_t)stream);
}

int wvn_mlp_confidence(const float* out, int ldo, const float* x, int ldx, float mean, float std, float std_factor,
                       float* trav, float* conf, int R, int D, void* stream) {
  if (!out || !x) return WVN_ERR_ARG;
  return wvn_mlp_confidence_launch(out, ldo, x, ldx, mean, std, std_factor, trav, conf, R, D, (hipStream_t)stream);
}

}  // extern "C"
