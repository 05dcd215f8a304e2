/*
 * wvn_hip.h -- C-ABI of libwvn_hip.so: the MI355X (gfx950) native implementation of Wild Visual
 * Navigation's  feature_extractor -> traversability_estimator  hot path.
 *
 * The reference (leggedrobotics/wild_visual_navigation) has no FFI layer: the path sits behind plain
 * Python classes that issue stock PyTorch ops.  Each entry point below replaces the arithmetic of
 * one reference function (cited as file:line, relative to the reference root) and is what a
 * maintainer binds with ctypes.  Conventions:
 *   - every pointer is a DEVICE pointer unless the name ends in _host; no allocation happens inside
 *     the library (callers own memory -- torch.empty in the Python host layer);
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work
 *     is stream-ordered and asynchronous;
 *   - return value: 0 = ok, 1001 = bad argument, 1002 = workspace too small, otherwise a hipError_t;
 *   - tensors are dense row-major; "tokens" are [B, G*G, D] (patch-major == NHWC feature map).
 */
#ifndef WVN_HIP_H
#define WVN_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WVN_MAX_DEPTH 32
#define WVN_PREC_F32 0  /* exact mode: fp32 storage + fp32 FMA everywhere (parity gate, <= 1e-3) */
#define WVN_PREC_BF16 1 /* fast mode: bf16 operands on MFMA, fp32 accumulate / statistics / residual */
#define WVN_PREC_X3 2   /* exact mode ON THE MATRIX PIPE: every MFMA operand is two bf16 planes (hi + lo, 16 significant bits),  \
                           every product hi*hi + hi*lo + lo*hi in fp32 accumulators (fp32-class results, <= 1e-3 gate), erf GELU, \
                           fp32 residual / LayerNorm / softmax */
#define WVN_PREC_FP8 3  /* BASELINE configs[4]: the four linears of every block on fp8 (OCP e4m3) MFMA at twice the bf16 rate --    \
                           per-token scales of the activations (computed by the LayerNorm / row-quantise kernels), per-output-channel \
                           scales of the weights, fp32 accumulate; attention, patch embedding, LayerNorm and the residual stream as   \
                           in WVN_PREC_BF16 */
#define WVN_PREC_F16 4  /* the WVN_PREC_BF16 path with fp16 operands: the same kernels compiled for v_mfma_f32_32x32x16_f16 /      \
                           v_cvt_pk_f16_f32 / v_dot2c_f32_f16 (same matrix rate and instruction counts), 11 significand bits        \
                           instead of 8 -- 8x less operand rounding; accumulation, residual stream, LayerNorm and softmax            \
                           statistics are fp32 in both.  Range: csrc/operand.h.  Weights: fp16 bits in the bf16 layouts */

#define WVN_PREC_MIX 5  /* the <= 1e-3 parity mode sized by the error budget (profiles/r04a_error_budget_*.md): every LINEAR of the   \
                           network (patch embedding, QKV, projection, fc1, fc2) exactly as in WVN_PREC_X3 -- hi + lo bf16 planes,    \
                           three MFMAs per product, erf GELU -- because each of them alone spends a third of the 1e-3 budget at one  \
                           16-bit value per operand; the two attention products (Q K^T, P V: 58 % of the multiply-adds, 3 % of the  \
                           error) on the fp16-operand kernel of WVN_PREC_F16, fed fp16 q / k / v^T by the QKV epilogue and writing  \
                           its output as hi + lo planes from its fp32 accumulators.  Weights as for WVN_PREC_X3 */

int wvn_version(void); /* 103 (100 -> 101: wvn_flip_average gained ld_src; wvn_vit_forward_frames_head, wvn_stego_head added; 102: wvn_gcn_train_*;
                          103: wvn_debug_slic_lab) */

/* ---------------------------------------------------------------------------------------------
 * DINO ViT backbone  (replaces stego.backbones.backbone.get_backbone(cfg)(img), called from
 * wild_visual_navigation/feature_extractor/dino_interface.py:45,84, plus the T.Normalize of :52).
 * Weights: matrices in torch.nn.Linear layout [out][in]; bf16 bits (uint16) when precision == WVN_PREC_BF16, float for
 * WVN_PREC_F32, for WVN_PREC_X3 TWO stacked bf16 planes [2][out][in]: hi = bf16(w), lo = bf16(w - hi), and for WVN_PREC_FP8
 * e4m3 bytes with the row scales in qkv_s .. fc2_s (the patch weight stays bf16).  For the MFMA precisions the patch weight
 * rows are zero-padded to a multiple of 64 columns (588 -> 640 for patch 14).
 * Biases, LayerNorm affine, LayerScale and the position table are always fp32.
 * ------------------------------------------------------------------------------------------- */
/* wvn_vit_model.flags: which single-kernel forms of the block stages wvn_vit_forward MAY use (WVN_PREC_BF16, D = 384).  They are
 * persistent one-workgroup-per-CU kernels and pay off once the token matrix fills the chip; below that (a single live frame)
 * wvn_vit_forward runs the separate LayerNorm / GEMM kernels whatever the flags say (thresholds: csrc/vit_forward.hip).
 * WVN_VIT_MLP_FUSED (F % 64 == 0): every layer also carries fc2_w_fused = fc2.weight with the hidden (input) index permuted --
 * bits 2 and 3 swapped inside each aligned group of 16, fc2_w_fused[n][k] = fc2.weight[n][swap23(k)] -- and the block MLP,
 * including its LayerNorm (blocks.i.norm2), runs as ONE kernel that keeps the normalised rows and the hidden activation in
 * registers (csrc/mlp_fused.hip). */
#define WVN_VIT_MLP_FUSED 1
/* WVN_VIT_QKV_FUSED (WVN_PREC_BF16, D = 384, heads = 6): blocks.i.norm1 and the QKV projection run as ONE kernel that normalises the
 * residual rows in registers (csrc/qkv_fused.hip); no weight re-layout. */
#define WVN_VIT_QKV_FUSED 2
/* use the allowed single-kernel forms at every size (tests, A/B runs), not only where they pay */
#define WVN_VIT_FUSE_ANY_SIZE 4
/* keep the attention projection a separate kernel where the fused MLP kernel runs (A/B runs; default: it is folded into that kernel) */
#define WVN_VIT_NO_PROJ_IN_MLP 8
/* A/B runs: do not let the projection + MLP kernel of a block apply the NEXT block's norm1 (default where fc1_w_fused and the next
 * layer's qkv_w_fused are given: the rows leave that kernel a second time as LayerNorm'ed operand fragments and the next QKV
 * kernel starts from those -- no second pass over the fp32 residual stream, no statistics, half the bytes) */
#define WVN_VIT_NO_LN_HANDOVER 16
#define WVN_VIT_NO_A384_X3 32     /* A/B and tests: the K = 384 linears of WVN_PREC_X3 / WVN_PREC_MIX on the tiled gemm_x3 kernel instead of the A-stationary one */
/* A/B and tests of the split-operand block kernels, one piece at a time (python: WVN_X3_DEBUG_BITS): 64 no A-stationary kernel, 128 no
 * row-panel kernel, 256 no fragment-major MLP hand-over */
#define WVN_VIT_X3_NO_A384 64
#define WVN_VIT_X3_NO_N384 128
#define WVN_VIT_X3_NO_FRAG_MLP 256
/* ... and: no LayerNorm across kernel boundaries (default for WVN_PREC_MIX / WVN_PREC_X3 from 8192 rows on: the row-panel kernels leave
 * {mean, rstd} of the rows they update, the A-stationary kernels normalise as they load; with this flag every LayerNorm is its own
 * kernel writing hi / lo planes again) */
#define WVN_VIT_X3_NO_LN_STATS 512
/* WVN_PREC_MIX: do NOT use the MX form of the block linears (round 6) even where the layer carries the packed weights *_w_mx: the bf16 x 3
 * kernels of rounds 4 / 5 (A/B runs and tests) */
#define WVN_VIT_NO_MX 1024
/* WVN_PREC_MIX: in how many LEADING blocks the attention kernel takes q as two fp16 planes (8 more MFMAs per tile, three workgroups per CU
 * instead of four: 3.08 against 2.05 ms per 128-frame launch).  The query's rounding is the one attention operand error that does not
 * average out over a row's keys, and it is injected in the EARLY blocks: on the reference's real 448^2 frame the token error is 1.05e-3
 * with no block split, 5.1e-4 / 4.3e-4 / 2.3e-4 with the first 2 / 4 / 6, 7.6e-5 with all twelve -- and still 1.05e-3 with only the LAST six
 * (profiles/r05_qsplit_blocks.md).  Bits 16 - 21 of flags hold n + 1; the field left 0 selects the default (6).  WVN_VIT_QSPLIT_BLOCKS(12)
 * is the round-4 behaviour. */
#define WVN_VIT_QSPLIT_BLOCKS(n) ((((n) + 1) & 63) << 16)
#define WVN_VIT_QSPLIT_DEFAULT 6
typedef struct wvn_vit_layer {
  const void* qkv_w;  /* [3D][D]   blocks.i.attn.qkv.weight  */
  const void* proj_w; /* [D][D]    blocks.i.attn.proj.weight */
  const void* fc1_w;  /* [F][D]    blocks.i.mlp.fc1.weight   */
  const void* fc2_w;  /* [D][F]    blocks.i.mlp.fc2.weight   */
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  const float *ls1, *ls2; /* [D] LayerScale of the attention / MLP branch (DINOv2 blocks.i.ls{1,2}.gamma); NULL = none (DINO) */
  const float *qkv_s, *proj_s, *fc1_s, *fc2_s; /* WVN_PREC_FP8: per-output-channel scale of each e4m3 weight row (w = q * s) */
  const void* fc2_w_fused;                     /* WVN_VIT_MLP_FUSED: fc2.weight with the permuted hidden index (see above); else NULL.
                                                * WVN_PREC_X3 / WVN_PREC_MIX (optional, D = 384): fc2.weight packed for the fragment-major MLP
                                                * (csrc/gemm_n384_x3.hip, AFRAG): bf16 [F / 16 k-steps][2 planes hi, lo][384 rows n][2 chunks][8],
                                                * chunk position cp of row n holds chunk c = cp ^ ((n >> 3) & 1), element j of chunk c =
                                                * fc2.weight[n][16 s + swap23(8 c + j)] (swap23: bits 2 and 3 exchanged); NULL: the row-major MLP */
  const void* fc1_w_fused; /* optional with WVN_VIT_MLP_FUSED: fc1.weight with its COLUMN (input) index permuted the same way,
                            * fc1_w_fused[f][k] = fc1.weight[f][swap23(k)].  With it (and no LayerScale) the block's projection + MLP
                            * kernel keeps the residual rows in its accumulator registers: one read and one write of the residual
                            * stream per block instead of two and two (wvn_proj_mlp_resident).  NULL: the form without it */
  const void* qkv_w_fused; /* optional with WVN_VIT_QKV_FUSED: qkv.weight with its column index permuted the same way: the QKV kernel
                            * of this block can then start from the fragments the previous block's kernel left (wvn_qkv_prenorm) */
  const void* proj_w_frag; /* WVN_PREC_X3 / WVN_PREC_MIX (optional, D = 384): attn.proj.weight in the packed layout of fc2_w_fused's
                            * split-operand form.  With it, WVN_PREC_MIX's attention kernel writes its output as MFMA operand fragments
                            * and the projection runs on the fragment form of csrc/gemm_n384_x3.hip.  NULL: the row-major projection */
  /* WVN_PREC_MIX, D = 384 (optional, all four or none): the weights in the MX operand representation -- per element h = fp16(w), l8 = e5m2((w - h) * 2^12),
   * h8 = e5m2(w) -- packed for the MX kernels (round 6): qkv / fc1 by backbone.pack_a384_mx (TWO images of N * 1536 bytes each, back to back: the planes of the
   * one-wave-per-SIMD kernel, then the chunk images of the two-workgroups-per-CU kernel that runs by default -- csrc/gemm_a384_x3.hip), proj / fc2 by
   * backbone.pack_n384_mx ([K / 64][4 stages][24 KB], csrc/gemm_n384_x3.hip).  With them every block linear from block 1 on (block 0's QKV has no producer
   * of LayerNorm statistics in front of it) computes a w = a_h w_h (fp16 MFMAs) + 2^-12 (a_h8 w_l8 + a_l8 w_h8) (scaled e5m2 MFMAs of K = 64): two thirds of
   * the matrix-pipe time of the bf16 x 3 products; the activations travel between the kernels as the h and l8 planes (h8 is derived in registers).
   * WVN_PREC_FP8, D = 768 (optional, each on its own): qkv_w_mx / proj_w_mx / fc1_w_mx = backbone.pack_a768_fp8 of the e4m3 weight -- with them these three
   * linears run on the A-stationary kernel (csrc/gemm_a768_fp8.hip) from 4096 rows on; fc2_w_mx is not read in this precision */
  const void* qkv_w_mx;
  const void* proj_w_mx;
  const void* fc1_w_mx;
  const void* fc2_w_mx;
} wvn_vit_layer;

typedef struct wvn_vit_model {
  int img_size; /* network input side S (448)            */
  int patch;    /* P (8, 14 or 16)                       */
  int dim;      /* D (384); heads * 64                   */
  int depth;    /* number of blocks (12)                 */
  int heads;    /* h (6); head dim is fixed at 64        */
  int mlp_dim;  /* F (1536)                              */
  int precision;
  int flags;    /* WVN_VIT_* bits */
  const void* patch_w;  /* [D][3*P*P (padded, see above)] conv weight flattened (c, py, px) */
  const float* patch_b; /* [D]                                                      */
  const float* cls_pos; /* [D]  = cls_token + pos_embed[0]                          */
  const float* pos;     /* [1+G*G][D] position table already resampled to the grid  */
  const float *norm_g, *norm_b;
  wvn_vit_layer layers[WVN_MAX_DEPTH];
} wvn_vit_model;

size_t wvn_vit_workspace_bytes(const wvn_vit_model* m, int batch);

/* img [B,3,S,S] fp32 in [0,1] (already resized/cropped, dino_interface.py:54-57) ->
 *   tokens_f32  [B, G*G, D]  final-LayerNorm'ed patch tokens (class token dropped), may be NULL
 *   tokens_lowp [B*G*G rows, ld_lowp] same values in the model precision (bf16 / fp16 / f32), may be NULL (must be NULL for
 *               WVN_PREC_X3: split the fp32 tokens with wvn_split_planes where planes are needed)
 * The workspace needs no initialisation (padding rows are reset by every call). */
int wvn_vit_forward(const wvn_vit_model* m, const float* img, int batch, float* tokens_f32, void* tokens_lowp,
                    int ld_lowp, void* workspace, size_t workspace_bytes, void* stream);

/* Same, for raw 8-bit frames: img [B,3,S,S] uint8 (4-byte aligned).  x/255 is fused into the patch gather, bit-identical
 * to wvn_vit_forward on img.float()/255 (what quick_start.py:160-161 and ros_converter.py:113-126 hand the reference),
 * with a quarter of the upload/HBM bytes.  bf16 / fp16 / fp8 models with patch 8 only (WVN_ERR_ARG otherwise; the general
 * form is wvn_vit_forward_frames). */
int wvn_vit_forward_u8(const wvn_vit_model* m, const unsigned char* img, int batch, float* tokens_f32, void* tokens_lowp,
                       int ld_lowp, void* workspace, size_t workspace_bytes, void* stream);

/* Frame ingest fused into the patch gather: frames [B,3,src_h,src_w] (fp32 in [0,1], or raw uint8 when
 * frames_u8) straight from the camera; network pixel (y, x) of frame b is frame pixel (rows[y], cols[x]).  rows / cols: device
 * int32 [S] -- the composition of T.Resize(input_size, NEAREST) and T.CenterCrop(input_size) (dino_interface.py:52-59,
 * stego_interface.py:51-58) or of ImageProjector.resize_image (image_projector.py:56-59, 199-200) as index tables, built once
 * per camera geometry by the host layer (feature_extractor/transforms.py).  Bit-identical to wvn_vit_forward on the resized /
 * cropped image; the resized image never exists.  Every precision and patch size. */
int wvn_vit_forward_frames(const wvn_vit_model* m, const void* frames, int frames_u8, int src_h, int src_w, const int* rows,
                           const int* cols, int batch, float* tokens_f32, void* tokens_lowp, int ld_lowp, void* workspace,
                           size_t workspace_bytes, void* stream);
/* The same for the frames AND their mirror images in ONE launch sequence of 2 * batch frames (the flip pass of the upstream
 * Stego.get_code, stego_interface.py:91): frame batch + i of the outputs is frame i gathered through cols_mirror (the reversed
 * column table).  tokens_f32 [2 * batch, G*G, D]; the workspace is that of wvn_vit_workspace_bytes(m, 2 * batch).  Bit-identical to two
 * calls of wvn_vit_forward_frames, and faster than them where the persistent block kernels run: twice the rows per launch. */
int wvn_vit_forward_frames_pair(const wvn_vit_model* m, const void* frames, int frames_u8, int src_h, int src_w, const int* rows,
                                const int* cols, const int* cols_mirror, int batch, float* tokens_f32, void* tokens_lowp, int ld_lowp,
                                void* workspace, size_t workspace_bytes, void* stream);
/* The STEGO segmentation head (code = tok W_lin^T + b_lin + ReLU(tok W_hid^T + b_hid) W_nl^T + b_nl) as wvn_vit_forward_frames_head
 * takes it.  It travels in a struct of its own: wvn_vit_model keeps its size.  All pointers are device pointers, 16-byte aligned.
 *   w_cat  hi / lo bf16 planes [2][512][384]: rows 0 .. 383 W_hid, rows 384 .. 384 + code_dim - 1 W_lin, the rest zero
 *   b_cat  [512] fp32: b_hid, b_lin, zeros
 *   w_nl   hi / lo bf16 planes [2][code_dim][384];  b_nl [code_dim] fp32
 *   code   OUT fp32 [rows][ld_code], rows = frames * G * G patch rows; ld_code % 4 == 0, >= 128: columns 0 .. code_dim - 1 hold the
 *          code, columns up to 127 zeros (the padded stride keeps every row 16-byte aligned; narrow with wvn_flip_average) */
typedef struct wvn_stego_head {
  const void* w_cat;
  const float* b_cat;
  const void* w_nl;
  const float* b_nl;
  float* code;
  int code_dim; /* <= 128 */
  int ld_code;
} wvn_stego_head;
/* wvn_vit_forward_frames (cols_mirror == NULL: `batch` frames) or wvn_vit_forward_frames_pair (2 * batch frames, the mirrors behind the
 * frames) with the STEGO head run off the residual rows: a statistics pass leaves {mean, rstd} of the final LayerNorm, ONE
 * A-stationary launch forms LayerNorm(x) as it loads the rows and writes the hidden planes (into the workspace) and the linear
 * branch's code rows, a third product adds the non-linear branch.  No token tensor is written; the code is bit-identical to
 * wvn_vit_forward_frames(_pair) + wvn_split_planes + three wvn_gemm_x3.  WVN_PREC_X3 / WVN_PREC_MIX, D = 384,
 * from 8192 token rows on (the route of the split-operand block kernels); everywhere else it
 * returns WVN_ERR_ARG BEFORE launching anything and the caller runs wvn_vit_forward_frames(_pair) and the head's three products. */
int wvn_vit_forward_frames_head(const wvn_vit_model* m, const void* frames, int frames_u8, int src_h, int src_w, const int* rows,
                                const int* cols, const int* cols_mirror, int batch, const wvn_stego_head* head, void* workspace,
                                size_t workspace_bytes, void* stream);
/* The same gather as an image op (ImageProjector.resize_image, image_projector.py:199-200, whose result the callers also
 * display): out [planes, out_h, out_w] = in [planes, src_h, src_w][.., rows[y], cols[x]]; elem_bytes 1 (uint8) or 4 (fp32, int32). */
int wvn_resize_nearest_crop(const void* in, void* out, long long planes, int src_h, int src_w, const int* rows, const int* cols,
                            int out_h, int out_w, int elem_bytes, void* stream);

/* Per-kernel-category HIP-event timing of wvn_vit_forward (bench.py roofline leg).  Categories:
 * 0 patchify 1 patch_gemm 2 layernorm 3 qkv_gemm 4 attention 5 proj_gemm 6 fc1_gemm 7 fc2_gemm */
#define WVN_PROF_NCAT 8
int wvn_prof_enable(int on);
int wvn_prof_collect(double* ms_by_cat_host, long long* launches_by_cat_host); /* syncs recorded events, resets */

/* ---------------------------------------------------------------------------------------------
 * Building blocks, exported so tests/ can check each kernel against the oracle.
 * ------------------------------------------------------------------------------------------- */
/* LayerNorm + QKV projection in one launch: x [M,ldx] fp32 (rows b * ntok_s + t) -> q, k [B*heads][npad][64] and
 * v^T [B*heads][64][npad] (token order of wvn_attention_bf16) in bf16; W [3*heads*64][384] bf16 in qkv.weight row order, q rows
 * multiplied by q_scale before rounding (0 = 1).  heads == 6, ntok_s % 16 == 0, M % 16 == 0, npad % 16 == 0. */
int wvn_qkv_fused(const float* x, int ldx, const float* ln_g, const float* ln_b, float ln_eps, const void* W, const float* bias,
                  void* q, void* k, void* vt, int heads, int npad, int ntok_s, float q_scale, int M, void* stream);
/* Attention projection + block MLP in one launch: x += (attn [M,lda] bf16 * Wp[384,384]^T + bp) (* ls1), then the block MLP of
 * wvn_mlp_fused with the LayerNorm inside on the updated rows.  What wvn_vit_forward uses where WVN_VIT_MLP_FUSED applies: the
 * projection's separate pass over the residual stream disappears (the updated rows stay in registers for the LayerNorm). */
int wvn_proj_mlp_fused(const void* attn, int lda, const void* Wp, const float* bp, const float* ls1, const float* ln_g,
                       const float* ln_b, float ln_eps, const void* W1, const float* b1, const void* W2p, const float* b2,
                       const float* ls2, float* x, int ldx, int M, int F, void* stream);
/* The same result (no LayerScale) with the residual rows RESIDENT in the accumulator registers of the kernel for the whole block:
 * x is read once and written once (wvn_proj_mlp_fused: twice and twice), the LayerNorm reads the rows where the projection MFMAs
 * left them, and fc2 accumulates on top of them.  W1p = fc1.weight with bits 2 and 3 of its column index swapped inside every
 * aligned group of 16 (wvn_vit_layer.fc1_w_fused), W2p as above.  Differs from wvn_proj_mlp_fused by fp32 summation order only
 * (the products are accumulated onto x + bias instead of being added to it at the end). */
int wvn_proj_mlp_resident(const void* attn, int lda, const void* Wp, const float* bp, const float* ln_g, const float* ln_b,
                          float ln_eps, const void* W1p, const float* b1, const void* W2p, const float* b2, float* x, int ldx, int M,
                          int F, const float* next_ln_g, const float* next_ln_b, float next_ln_eps, void* xn_next, void* stream);
/* xn_next != NULL: the kernel also applies LayerNorm(next_ln_g, next_ln_b, next_ln_eps) -- blocks.(i+1).norm1 -- to the finished rows
 * and writes the result as MFMA operand fragments: fragment (32-row group R, k-step s) = 1 KB at xn_next + (R * 24 + s) * 1024
 * bytes, lane l's 16 bytes at l * 16 = the 8 values of row 32 R + (l & 31) at columns 16 s + 4 (l >> 5) + {0..3} and
 * 16 s + 8 + 4 (l >> 5) + {0..3}; (M + 31) / 32 * 24 KB.  wvn_qkv_prenorm is the QKV projection that starts from them (Wperm =
 * qkv.weight with bits 2 and 3 of its column index swapped, wvn_vit_layer.qkv_w_fused): = wvn_qkv_fused on the same rows up to
 * fp32 summation order.  b2 then joins the rows as two operand-format terms through the matrix pipe, like bp. */
int wvn_qkv_prenorm(const void* xn_frag, const void* Wperm, const float* bias, void* q, void* k, void* vt, int heads, int npad, int ntok_s,
                    float q_scale, int M, void* stream);
/* Block MLP in one launch: x [M,ldx] fp32 += gelu(xn [M,lda] bf16 * W1[F,384]^T + b1) * W2[384,F]^T + b2  (optionally
 * times LayerScale ls [384]).  W2p = W2 with the hidden index permuted as WVN_VIT_MLP_FUSED describes.  xn == NULL: the kernel
 * computes xn = LayerNorm(x; ln_g, ln_b, ln_eps) itself (what wvn_vit_forward uses: blocks.i.norm2 never touches memory).
 * D is fixed at 384, F % 64 == 0, F <= 1536.  Same arithmetic as wvn_gemm_bf16(epi 1) followed by wvn_gemm_bf16(epi 4) except
 * the summation order inside an MFMA (and inside the LayerNorm statistics). */
int wvn_mlp_fused(const void* xn, int lda, const float* ln_g, const float* ln_b, float ln_eps, const void* W1, const float* b1,
                  const void* W2p, const float* b2, const float* ls, float* x, int ldx, int M, int F, void* stream);
/* C = epilogue(A[M,K] * W[N,K]^T + bias).  epi: 0 bf16 out, 1 gelu->bf16, 2 relu->bf16, 3 f32 out,
 * 4 f32 out += (residual), 5 same as 4.  A/W bf16, K % 64 == 0. */
int wvn_gemm_bf16(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N,
                  int K, int epi, void* stream);
/* fp16-operand twins of the five entries above and of wvn_attention_bf16 below (WVN_PREC_F16: same layouts with fp16 bits, same
 * epilogue codes -- "bf16 out" reads "fp16 out") */
int wvn_gemm_f16(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N, int K, int epi,
                 void* stream);
int wvn_qkv_fused_f16(const float* x, int ldx, const float* ln_g, const float* ln_b, float ln_eps, const void* W, const float* bias,
                      void* q, void* k, void* vt, int heads, int npad, int ntok_s, float q_scale, int M, void* stream);
int wvn_proj_mlp_fused_f16(const void* attn, int lda, const void* Wp, const float* bp, const float* ls1, const float* ln_g,
                           const float* ln_b, float ln_eps, const void* W1, const float* b1, const void* W2p, const float* b2,
                           const float* ls2, float* x, int ldx, int M, int F, void* stream);
int wvn_proj_mlp_resident_f16(const void* attn, int lda, const void* Wp, const float* bp, const float* ln_g, const float* ln_b,
                              float ln_eps, const void* W1p, const float* b1, const void* W2p, const float* b2, float* x, int ldx,
                              int M, int F, const float* next_ln_g, const float* next_ln_b, float next_ln_eps, void* xn_next,
                              void* stream);
int wvn_qkv_prenorm_f16(const void* xn_frag, const void* Wperm, const float* bias, void* q, void* k, void* vt, int heads, int npad,
                        int ntok_s, float q_scale, int M, void* stream);
int wvn_mlp_fused_f16(const void* xn, int lda, const float* ln_g, const float* ln_b, float ln_eps, const void* W1, const float* b1,
                      const void* W2p, const float* b2, const float* ls, float* x, int ldx, int M, int F, void* stream);
int wvn_attention_f16(const void* q, const void* k, const void* vt, void* out, int B, int heads, int ntok, int npad, float scale,
                      void* stream);
/* The same GEMM in exact mode (WVN_PREC_X3): A and W as hi / lo bf16 planes (same leading dimensions), three MFMAs per
 * product.  epi 0-2 write C as hi / lo planes (C, C_lo, bf16 [M, ldc] each; gelu = exact erf form), epi 3-5 write fp32 C
 * (C_lo ignored). */
int wvn_gemm_x3(const void* A_hi, const void* A_lo, int lda, const void* W_hi, const void* W_lo, int ldw, const float* bias,
                void* C, void* C_lo, int ldc, int M, int N, int K, int epi, void* stream);
/* The fp8 building blocks (WVN_PREC_FP8): rows of src (fp32, or bf16 when src_is_bf16) -> e4m3 rows q [rows, ldq] + scale[rows]
 * (= amax / 448, 1 for a zero row);  C = epilogue((A_q W_q^T) sa[m] sw[n] + bias) on v_mfma_scale_f32_32x32x64_f8f6f4 with
 * epi 0 (bf16 out), 1 (gelu -> bf16), 3 (fp32 out), 4 (fp32 +=).  K % 128 == 0, lda / ldw % 16 == 0. */
int wvn_quantize_rows_fp8(const void* src, int src_is_bf16, int lds, void* q, int ldq, float* scale, int rows, int cols,
                          void* stream);
/* LayerNorm (fp32 rows of x [rows, D], D % 64 == 0, biased variance, eps inside the sqrt) fused with the row quantiser: q [rows, ldq]
 * e4m3 + scale [rows] of the NORMALISED rows -- what every fp8 block runs in front of its QKV / fc1 GEMM */
int wvn_layernorm_fp8(const float* x, const float* gamma, const float* beta, void* q, int ldq, float* scale, int rows, int D,
                      float eps, void* stream);
int wvn_gemm_fp8(const void* A_q, int lda, const void* W_q, int ldw, const float* sa, const float* sw, const float* bias,
                 void* C, int ldc, int M, int N, int K, int epi, void* stream);
/* The A-stationary form of the same product for K == 768 (csrc/gemm_a768_fp8.hip; what WVN_PREC_FP8 runs for the QKV, projection and fc1 linears of
 * ViT-Base from 4096 rows on -- the layer's qkv_w_mx / proj_w_mx / fc1_w_mx fields carry the packed weights in that precision): a workgroup keeps 128 rows of
 * A in registers and streams 32-column tiles of the weight, packed by backbone.pack_a768_fp8 as [N / 32][12 k-steps][2 halves][64 lanes][16 B].
 * epi (the numbers of wvn_gemm_fp8): 0 | 1 (C bf16 [M][ldc], 1 = gelu), 4 (C fp32 += ls * (...), ls optional), 7 (q | k | v^T bf16 in the
 * layouts of wvn_attention_bf16, inside one 2 GB span; q scaled by q_scale when it is not 0), 9 (gelu -> C = e4m3 [M][ldc] with MX block scales: one E8M0 byte per
 * (row, 32 columns) written to q [M][N / 32] -- the A operand of wvn_gemm_fp8_mx).  N % 32 == 0; WVN_ERR_ARG for any other shape. */
int wvn_gemm_a768_fp8(const void* A_q, int lda, const void* W_packed, const float* sa, const float* sw, const float* bias, const float* ls, void* C, int ldc,
                      int M, int N, int epi, void* q, void* k, void* vt, int heads, int npad, int ntok_s, float q_scale, void* stream);
/* wvn_gemm_fp8 with MX block scales on the A operand: A_q e4m3 [M][lda], a_scales [M][K / 32] E8M0 bytes (value = q * 2^(byte - 127) per 32 consecutive k; what epi 9
 * above writes), W_q with one fp32 scale per row as before; epi 3 (C fp32 =) | 4 (C fp32 += ls * (...)).  K % 128 == 0.  WVN_PREC_FP8 runs ViT-Base's fc2 this way
 * behind the A-stationary fc1 (no row quantiser between them; WVN_NO_FP8_MX=1 in the environment: the bf16 hidden activation and the row quantiser again) */
int wvn_gemm_fp8_mx(const void* A_q, int lda, const void* a_scales, const void* W_q, int ldw, const float* sw, const float* bias, const float* ls,
                    void* C, int ldc, int M, int N, int K, int epi, void* stream);
/* fp32 [rows, lds] -> hi = bf16(x), lo = bf16(x - hi), both [rows, ldd] */
int wvn_split_planes(const float* src, int lds, void* hi, void* lo, int ldd, int rows, int cols, void* stream);
/* exact-mode attention: q / k planes [B,h,npad,64], V^T planes [B,h,64,npad] (token permutation of the bf16 path),
 * out planes [B*ntok, h*64]; scale > 0 */
int wvn_attention_x3(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* vt_hi,
                     const void* vt_lo, void* out_hi, void* out_lo, int B, int heads, int ntok, int npad, float scale,
                     void* stream);
/* fp32 GEMM C = epilogue(op(A) op(B) + bias); transA: A stored [K,M]; transB: B stored [N,K].
 * epi: 0 none, 1 relu, 2 gelu, 3 C +=, 4 sigmoid on column 0, 5 relu-mask (mask > 0 ? acc : 0). */
int wvn_gemm_f32(const float* A, int lda, int transA, const float* B, int ldb, int transB, const float* bias, float* C,
                 int ldc, int M, int N, int K, int epi, const float* mask, int ldmask, void* stream);
int wvn_layernorm(const float* x, const float* gamma, const float* beta, void* y, int y_is_bf16, int rows, int D,
                  float eps, void* stream);
/* q,k [B,h,npad,64]; v: bf16 path takes V^T [B,h,64,npad], f32 path takes V [B,h,npad,64];
 * out [B*ntok, h*64].  npad % 128 == 0, pad rows must be finite.
 * bf16 path: V^T is stored with the tokens of every aligned group of 16 permuted -- position
 * 16G + 8h + 4a + e holds token 16G + 8a + 4h + e (bits 2 and 3 of the token index swapped; order
 * 0-3, 8-11, 4-7, 12-15) -- so that the 8 keys a half-wave multiplies with are one 16-byte LDS read.
 * The QKV projection epilogues of wvn_vit_forward write this layout.
 * scale > 0: q holds the raw projections, scores = scale * q.k.  scale == 0 (bf16 path only): q is already multiplied by
 * softmax_scale * log2(e) (wvn_vit_forward's QKV epilogue does that before rounding q to bf16); the kernel then feeds the
 * running max into the S^T MFMA chain as its C operand and the accumulators come out as exp2 arguments. */
int wvn_attention_bf16(const void* q, const void* k, const void* vt, void* out, int B, int heads, int ntok, int npad,
                       float scale, void* stream);
int wvn_attention_f32(const float* q, const float* k, const float* v, float* out, int B, int heads, int ntok, int npad,
                      float scale, void* stream);
int wvn_patchify(const float* img, void* patches, int out_is_bf16, int B, int S, int P, void* stream);
int wvn_patchify_u8(const unsigned char* img, void* patches_bf16, int B, int S, int P, void* stream); /* P in {8, 14, 16} */
int wvn_cast_f32_to_bf16(const float* src, void* dst, long long n, void* stream);
/* strided rows: dst[r][c] = (bf16 | fp16 when to_f16) src[r][c], fp32 src with leading dimension lds, 16-bit dst with ldd */
int wvn_cast_rows(const float* src, int lds, void* dst, int ldd, int rows, int cols, int to_f16, void* stream);

/* F.interpolate(features, (H,H), mode="bilinear", align_corners=True) of dino_interface.py:87-90 /
 * stego_interface.py:107: tokens [B,G*G,D] -> dense [B,D,H,H] fp32. */
int wvn_upsample_bilinear(const float* tokens, float* dense, int B, int G, int D, int H, void* stream);
/* F.interpolate(pred[None].float(), (H,H), mode="nearest").int()  (stego_interface.py:108-109) */
int wvn_upsample_nearest_i32(const int* labels, int* out, int B, int G, int H, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Segments
 * ------------------------------------------------------------------------------------------- */
/* FeatureExtractor.sparsify_features (feature_extractor.py:390-396) fused with the bilinear
 * up-sampling that precedes it: feat[b][s][:] = mean over {seg[b]==s} of upsample(tokens[b]).
 * seg [B,H,W] int32 (-1 = ignore), tokens [B,G*G,ld] fp32, feat [B,S,D].
 * Square frames only: H == W.  Both axes are resampled with the tap scale (G-1)/(H-1), as the reference's H x H dense map
 * is; H != W returns WVN_ERR_ARG before anything is written or launched.  Also WVN_ERR_ARG: null pointer, S < 1, D < 1,
 * D > 1024, scratch_w not 8-byte aligned.
 * scratch_w: B*S*G*G 8-byte words (the tap weights accumulate in 64-bit fixed point: integer atomics are order-independent,
 * so the result is deterministic), scratch_cnt: B*S ints (receives the pixel count per segment). */
int wvn_segpool_bilinear_mean(const int* seg, const float* tokens, int ld, float* feat, void* scratch_w,
                              int* scratch_cnt, int B, int H, int W, int G, int S, int D, void* stream);
/* Same result as wvn_segpool_bilinear_mean for PATCH-ALIGNED segment maps (a [B,G,G] label grid that
 * the caller would nearest-upsample by exactly the patch size: k-means clusters, grid cells that are a
 * multiple of the patch): mean over a segment's patches of a separable 3x3 stencil of the patch map.
 * wy, wx: [G][3] fp32 stencil weights for offsets -1,0,+1 (per-patch-row sums of the align_corners
 * tap weights / P).  Deterministic, no atomics.  labels [B,G*G] int32, feat [B,S,D]. */
int wvn_segpool_patch_labels(const int* labels, const float* tokens, int ld, const float* wy, const float* wx,
                             float* feat, int B, int G, int S, int D, void* stream);
/* FeatureExtractor.sparsify_features on an explicit pixel-resolution map (no resampling):
 * tokens [B,P,D] pixel-major, seg [B,P] -> feat [B,S,D] = per-segment mean (0/0 = NaN). S <= 236.  Deterministic (fixed
 * summation order, no atomics); scratch: wvn_segmean_scratch_bytes() bytes; scratch_cnt [B*S] receives the pixel counts. */
size_t wvn_segmean_scratch_bytes(int B, int P, int S, int D);
int wvn_segmean_tokens(const int* seg, const float* tokens, float* feat, int* scratch_cnt, void* scratch, size_t scratch_bytes,
                       int B, int P, int S, int D, void* stream);
/* MissionNode.update_supervision_signal (traversability_estimator/nodes.py:400-440).
 * mask [C,H,W] fp32 (NaN = unlabeled), seg [H,W] int32 -> signal [S] fp32, valid [S] uint8.
 * scratch_sum: S 8-byte words (2^-32 fixed-point sums: deterministic), scratch_cnt: S ints. */
int wvn_label_pool(const float* mask, int C, const int* seg, float* signal, unsigned char* valid, void* scratch_sum,
                   int* scratch_cnt, int H, int W, int S, void* stream);
/* The same for n nodes in ONE launch pair (TraversabilityEstimator.add_supervision_node re-pools every mission node in
 * range, traversability_estimator.py:287-289).  nodes_dev: DEVICE array of n records; scratch_sum: n*Smax 8-byte words,
 * scratch_cnt: n*Smax ints; all masks [C,H,W], all segment maps [H,W]. */
typedef struct wvn_label_pool_node {
  const float* mask;    /* [C][H][W] */
  const int* seg;       /* [H][W]    */
  float* signal;        /* [S] out   */
  unsigned char* valid; /* [S] out   */
  int S;
  int reserved;
} wvn_label_pool_node;
int wvn_label_pool_batched(const wvn_label_pool_node* nodes_dev, int n, int C, int H, int W, int Smax, void* scratch_sum,
                           int* scratch_cnt, void* stream);

/* segmentation_type "random" (feature_extractor.py:96-111, 227-235: nr pixels of the frame are the segments) for a batch, csrc/random_pixels.hip.
 * Frame b draws with the key (seed, frame0 + b), both unsigned 32-bit (the frame index wraps); the key defines a bijection pi of
 * [0, H*W) -- a four-round balanced Feistel network on the smallest even number of bits that holds H*W, cycle-walked into range;
 * round keys from splitmix64 of seed << 32 ^ frame, murmur3's 32-bit finaliser as the round function (tests/random_pixels_ref.py
 * states it in integers) -- and
 *   idx [B][nr]   int32: idx[b][j] = pi(j), nr distinct pixels (row-major y * W + x), O(nr) work;
 *   seg [B][H][W] int32: pi^-1(p) where that is < nr, -1 elsewhere (sample j carries id j).
 * Every thread evaluates pi or pi^-1 for its own element: no sort, no atomics, no host synchronisation, the same values for any
 * launch geometry.  idx or seg may be NULL (not both).  WVN_ERR_ARG: nr < 1, nr > H*W, H*W > 2^30, B < 1, B > 65535. */
int wvn_random_pixels(unsigned seed, unsigned frame0, int B, int H, int W, int nr, int* idx, int* seg, void* stream);
/* feat[b][j][:] (fp32 [B][nr][D]) = the bilinear (align_corners=True) value of tokens[b] ([G*G][D] fp32) at pixel idx[b][j] = y * H + x
 * of the H x H map: bit-identical to wvn_upsample_bilinear's dense[b][:][y][x] -- the reference's dense.reshape(D, H*H)[:, idx].T --
 * from four token rows per sample.  idx is arbitrary (duplicates allowed); an index outside [0, H*H) gives a NaN row.  Any D >= 1.
 * WVN_ERR_ARG: null pointer, B < 1, B > 65535, G < 1, H < 1, H > 32768, D < 1, nr < 1. */
int wvn_gather_bilinear(const float* tokens, const int* idx, float* feat, int B, int G, int H, int D, int nr, void* stream);

/* feature_type "sift" (feature_extractor.py:65-67, 276-286 of the reference: kornia's DenseSIFTDescriptor per colour channel, 8 + 1
 * convolutions, then the per-segment means of the [1, 128 C, H, W] map), csrc/dense_sift.hip.  fp32.  The definition the kernels are
 * held to (tests/dense_sift_ref.py states it in float64; PARITY WITH THE kornia PACKAGE ITSELF IS UNPINNED, the package is absent), for
 * one channel I [H][W] in [0, 1], eps = 1e-10:
 *   1. gx[y][x] = (I[y][x+1] - I[y][x-1]) / 2, gy[y][x] = (I[y+1][x] - I[y-1][x]) / 2, replicate padding by one pixel;
 *   2. mag = sqrt(gx^2 + gy^2 + eps), ori = atan2(gy, gx + eps) + 2 pi, o = 8 ori / (2 pi), b0 = floor(o) mod 8, b1 = (b0 + 1) mod 8,
 *      w1 = o - floor(o); plane P_a = [b0 = a] (1 - w1) mag + [b1 = a] w1 mag, a = 0..7;
 *   3. Q_a [H+1][W+1]: Q_a[p][q] = sum_{i,j=0..3} k[i] k[j] P_a[p-2+i][q-2+j], k = [0.25, 0.75, 0.75, 0.25], terms outside the image 0;
 *   4. d[a*16 + i*4 + j][y][x] = Q_a[y-1+i][x-1+j], i, j = 0..3, terms outside Q 0;
 *   5. per pixel over the 128 values: d /= max(|d|_2, 1e-12); d = clamp(d, 0, 0.2); d /= max(|d|_2, 1e-12); d = sqrt(d / max(|d|_1, 1e-12) + eps).
 * img [B][C][H][W] fp32, or uint8 (img_is_u8: x / 255 in fp32, fused into the load); C = 1 or 3; no resize, crop or normalisation.
 * wvn_dense_sift: out [B][128 C][H][W] fp32, channel c of the frame in out[b][128 c .. 128 c + 127].
 * wvn_dense_sift_segpool: feat [B][S][128 C] fp32 = the per-segment means of that map over seg [B][H][W] int32, WITHOUT writing the map,
 *   from the same per-pixel arithmetic: feat = float(double(sum trunc(v 2^32)) / (double(count) 2^32)) (64-bit integer sums: no
 *   dependence on the order of the atomics; v <= 1, so the product is exact).  Ids outside [0, S) (-1 included) are ignored, an id without
 *   a pixel gives a NaN row, a tile without a labelled pixel costs a read of its labels.  cnt [B][S] int32 out (pixels per id);
 *   scratch_sum: B * S * 128 C 8-byte words.  Both are cleared by the call.
 * WVN_ERR_ARG before any launch: null pointer, B < 1, B * C > 65535, C not 1 or 3, H or W < 4 or > WVN_DENSE_SIFT_MAX_SIDE, S < 1,
 * S > WVN_DENSE_SIFT_MAX_SEGMENTS, B * S * 128 C >= 2^31. */
#define WVN_DENSE_SIFT_MAX_SIDE 16384
#define WVN_DENSE_SIFT_MAX_SEGMENTS (1 << 20)
int wvn_dense_sift(const void* img, int img_is_u8, float* out, int B, int C, int H, int W, void* stream);
int wvn_dense_sift_segpool(const void* img, int img_is_u8, const int* seg, float* feat, int* cnt, void* scratch_sum, int B, int C,
                           int H, int W, int S, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Supervision masks: ImageProjector.project_and_render (image_projector.py:126-197: pinhole projection +
 * kornia draw_convex_polygon) fused with the torch.fmin merge of traversability_estimator.py:281-286, for n mission nodes in
 * one launch.  Per node: K [4][4] (the projector's scaled camera matrix), pose [4][4] = pose_cam_in_world, mask [C][H][W]
 * updated IN PLACE (inside the projected polygon: fmin(old, value); elsewhere untouched = fmin(old, NaN)), projected [npts][2]
 * + depth [npts] (optional outs; the polygon itself is drawn with the behind-the-camera vertices set to NaN, :180).  points: [npts][3] world coordinates shared by all nodes, or
 * [n][npts][3] when points_batched.  value = colour * traversability, read from value_dev[0] if non-NULL (no host sync when
 * the traversability lives on the GPU).  npts: any count whose vertex arrays fit the 64 KB of LDS beside the 2*H row limits (npts <= 8191 - H; H = 448: 7743; the
 * untraversable plane of SupervisionNode.make_footprint_with_node has 1000).  Scan lines touched by a NaN edge stay unfilled (torch min / max).  Arithmetic order: csrc/supervision.hip header.
 * ------------------------------------------------------------------------------------------- */
typedef struct wvn_render_node {
  const float* K;
  const float* pose;
  float* mask;
  float* projected; /* [npts][2] out, optional: the RAW pinhole coordinates of every point (finite also behind the camera, as
                       ImageProjector.project returns them, image_projector.py:126-150) */
  float* depth;     /* [npts] out, optional: camera-frame z of every point (valid_z = depth >= 0, check_validity :112-124) */
} wvn_render_node;
int wvn_project_render_fmin(const wvn_render_node* nodes_dev, int n, const float* points, int points_batched, int npts, int C,
                            int H, int W, const float* value_dev, float value, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SLIC superpixels (FeatureExtractor default segmentation_type, feature_extractor.py:84-90,221-225: fast_slic on the CPU in
 * the reference).  Integer-arithmetic SLIC (csrc/slic.hip): img [3][H][W] uint8 or float in [0,1]; labels [H][W] int32 in
 * [0, wvn_slic_num_clusters()).  lut_lin [256], lut_f [4096]: sRGB->linear and CIELAB f(t) tables (device, int32; built by the
 * caller in double precision: wild_visual_navigation_amd/ops.py slic_tables).  Parity with fast_slic is unpinned.  The map is the
 * k-means result; fast_slic's connectivity post-pass is the separate, opt-in wvn_slic_connectivity below.
 * ------------------------------------------------------------------------------------------- */
int wvn_slic_num_clusters(int H, int W, int num_components);
size_t wvn_slic_scratch_bytes(int H, int W, int num_components);
int wvn_slic(const void* img, int img_is_u8, int H, int W, int num_components, float compactness, int iters, const int* lut_lin,
             const int* lut_f, int* labels, void* scratch, size_t scratch_bytes, void* stream);
/* Connectivity enforcement (csrc/slic_connectivity.hip): the post-processing step of SLIC (Achanta et al. 2012; fast_slic's Slic(...)
 * does it by default) as an opt-in pass over [B][H][W] int32 label maps with ids in [0, K) -- SLIC's or any other.  The definition the
 * kernels are held to, bit for bit (tests/slic_connectivity_ref.py):
 *   1. A component is a maximal 4-connected set of pixels with equal label; its size is its pixel count.
 *   2. A component is anchored if its size is >= min_size.  If no component is anchored, the output is the input.
 *   3. Round: all decisions read the state at the start of the round.  For every component C that is not yet anchored, take all
 *      pairs (p, q) with p in C, q a 4-neighbour of p inside the frame, q anchored.  No such pair: C waits.  Otherwise count the pairs
 *      per current label of q; C takes the label with the highest count, the lowest id on a tie; all its pixels are anchored from
 *      the next round on.
 *   4. Rounds repeat until every pixel is anchored.
 * The result is a pure function of (labels, min_size): no dependence on launch geometry, on the order of atomics or on the batch
 * position.  Ids stay in [0, K): an id that lost all its pixels behaves as an empty id does.  This is an order-independent form of
 * Achanta's sequential scan; PARITY WITH fast_slic's OWN POST-PASS IS UNPINNED (the package is absent, as for the SLIC itself).
 * min_size: the caller's integer (ops.py: max(1, int(0.25 * H * W / K)), fast_slic's default factor).  labels_out may be labels_in.
 * The launch sequence contains no host read: WVN_SLIC_CC_PAR_ROUNDS rounds run one wave per waiting component across the GPU, then one
 * workgroup per image runs rounds until the image's counter of waiting components is zero.  That counter is the int32 at
 * scratch + 16 * b for image b: zero after the call (in stream order) whatever the input.  K is validated (>= 1) and otherwise unused:
 * labels are only ever compared.  WVN_ERR_ARG: null pointer, B / H / W / K / min_size < 1, B * H * W >= 2^29, short scratch.
 * The component labelling works on WVN_SLIC_CC_TILE_H x WVN_SLIC_CC_TILE_W tiles in LDS, merged across tile borders. */
#define WVN_SLIC_CC_TILE_W 32
#define WVN_SLIC_CC_TILE_H 8
#define WVN_SLIC_CC_PAR_ROUNDS 8
size_t wvn_slic_connectivity_scratch_bytes(int B, int H, int W, int K);
int wvn_slic_connectivity(const int* labels_in, int* labels_out, int B, int H, int W, int K, int min_size, void* scratch,
                          size_t scratch_bytes, void* stream);
/* SegmentExtractor.centers (segment_extractor.py:70-92): centers [S,2] fp32 (x,y). scratch: 3*S u64. */
int wvn_seg_centers(const int* seg, float* centers, void* scratch, int H, int W, int S, void* stream);
/* SegmentExtractor.adjacency_list (segment_extractor.py:39-67): edges [max_edges,2] int64 sorted by
 * key = left + right*S, *count = E (device int).  scratch_bitmap: S*S bytes. */
int wvn_seg_adjacency(const int* seg, long long* edges, int* count, unsigned char* scratch_bitmap, int H, int W, int S,
                      int max_edges, void* stream);

/* ---------------------------------------------------------------------------------------------
 * STEGO head + clustering  (stego.stego.Stego.get_code / postprocess, stego_interface.py:91-100)
 * ------------------------------------------------------------------------------------------- */
/* rows of code [rows, ldc] -> xn [rows, C] = code / max(||code||, 1e-12), sequential fp32 */
int wvn_normalize_rows(const float* code, int ldc, float* xn, int rows, int C, void* stream);
/* out[r] = argmax over the cols of row r (lowest index wins ties): label maps of the STEGO cluster probe (cosine similarity
 * against the checkpoint's learned centroids, run_clustering=False) and linear probe (stego_interface.py:94-100) */
int wvn_argmax_rows(const float* x, int ld, int rows, int cols, int* out, void* stream);
/* deterministic cosine k-means per image on xn [B,P,C]; labels [B,P] int32; nseg [B] distinct ids;
 * relabel != 0 compacts ids to 0..K'-1 ascending (feature_extractor.py:245-246). C in {16,64,90}.
 * scratch: wvn_kmeans_scratch_bytes(B,P,C,K) bytes (centroids + per-chunk partial sums); on return its first B*K*C floats hold the
 * final centroids [B][K][C] (both forms). */
/* Summation order of the centroid update (both forms): chunks of 64 consecutive points, members of a cluster in ascending point
 * order; chunk partials in ascending order inside groups of 8 chunks; group partials in ascending order; every chain starts from
 * +0.  Normalisation: x * (1 / max(||x||, 1e-12)) with one correctly rounded reciprocal per row. */
size_t wvn_kmeans_scratch_bytes(int B, int P, int C, int K);
/* The same k-means over the H x H code PIXELS of every frame (stego_interface.py:94-109 read as "postprocess clusters the
 * up-sampled code"): code [B, G*G, C] fp32 patch codes (NOT normalised); the points are the rows of
 * normalise(F.interpolate(code, (H,H), bilinear, align_corners=True)), re-created on the fly in every pass from the L2-resident
 * patch codes -- the [B, H*H, C] array (4.6 GB per 64 frames at 448^2) never exists.  labels [B, H*H] int32.  Bit-identical to
 * wvn_upsample_bilinear + wvn_normalize_rows + wvn_kmeans_cosine on the materialised rows.  C in {16, 90}. */
size_t wvn_kmeans_pixels_scratch_bytes(int B, int G, int H, int C, int K);
int wvn_kmeans_cosine_pixels(const float* code, int* labels, int* nseg, void* scratch, int B, int G, int H, int C, int K, int iters,
                             int relabel, void* stream);
/* The pixel-resolution k-means through its LINEARITY (round 5; the form StegoInterface uses, stego_interface.py:94-109): the same
 * clustering -- same points, same initial centroids, same iteration count, same tie rule -- with the assignment taken from a per-pass
 * similarity table S = code . c^T interpolated per pixel (rinv_p > 0 moves no argmax, <., c_k> is linear in the four taps) and the
 * centroid sums from per-(cluster, patch) summed tap weights times the patch codes (SURVEY.md 8(a7)'s pooling identity): ~1/20 of the
 * arithmetic of wvn_kmeans_cosine_pixels.  Every summation order is fixed (csrc/stego_linear.hip; oracle/kmeans_linear.py states them), so
 * labels and centroids are reproducible bit for bit; against wvn_kmeans_cosine_pixels they differ only at pixels whose two best
 * similarities are closer than fp32 rounding.  C in {16, 90}, K <= 32 (wvn_kmeans_pixels_linear_supported_shape); scratch as above: its
 * first B*K*C floats hold the final centroids on return. */
int wvn_kmeans_pixels_linear_supported_shape(int G, int H, int C, int K);
size_t wvn_kmeans_pixels_linear_scratch_bytes(int B, int G, int H, int C, int K);
int wvn_kmeans_cosine_pixels_linear(const float* code, int* labels, int* nseg, void* scratch, int B, int G, int H, int C, int K,
                                    int iters, int relabel, void* stream);
/* The same with the OTHER reading of how the code is interpolated before it is clustered (round 6): align_corners = 0 takes ATen's half-pixel taps
 * (F.interpolate(code, size, mode="bilinear", align_corners=False): what the public STEGO evaluation code uses) instead of the align_corners=True
 * taps WVN's own later up-sample uses (stego_interface.py:107).  The reference hands postprocess() to an absent package (stego_interface.py:94-100), so
 * which one runs upstream cannot be decided here: StegoInterface(code_align_corners=...) selects it, oracle/kmeans_linear.py states both, the GPU is
 * bit-exact against either.  align_corners != 0: identical to wvn_kmeans_cosine_pixels_linear. */
int wvn_kmeans_cosine_pixels_linear_ac(const float* code, int* labels, int* nseg, void* scratch, int B, int G, int H, int C, int K,
                                       int iters, int relabel, int align_corners, void* stream);
/* labels[b][y][x] (int32, [B, H, H]) = argmax over k < K (lowest k wins ties) of the bilinear interpolation (align_corners=True, the
 * fixed operation order of wvn_upsample_bilinear) of table[b][.][k] to H x H: the STEGO cluster probe / linear probe applied at PIXEL
 * resolution (stego_interface.py:94-100, 107-109: postprocess acts on the up-sampled code; a probe is linear in the code and the
 * interpolation weights sum to one, so interpolating its K outputs per patch equals evaluating it on the interpolated code).
 * table: [B, G*G, wvn_table_argmax_slots(K)] fp32, 16-byte aligned, slots >= K ignored; K <= 32. */
int wvn_table_argmax_slots(int K);
int wvn_table_bilerp_argmax(const float* table, int* labels, int B, int G, int H, int K, void* stream);
/* the same with the taps of align_corners (0: half-pixel coordinates; see wvn_kmeans_cosine_pixels_linear_ac) */
int wvn_table_bilerp_argmax_ac(const float* table, int* labels, int B, int G, int H, int K, int align_corners, void* stream);
/* out = 0.5 * (a + flip_x(mirrored)) on [B, G, G, C] fp32 patch maps: the code of a frame averaged with the flipped-back code of
 * its mirror image (the second pass of the upstream Stego.get_code; the mirror pass itself is wvn_vit_forward_frames with a
 * reversed column table).  ld_src: row stride (floats, >= C) of a and mirrored -- C for contiguous maps, 128 for the padded code
 * rows of wvn_vit_forward_frames_head; out is [B, G, G, C] contiguous and may alias a where ld_src == C.  mirrored == NULL: out = a
 * (the padded rows narrowed: the single-pass form). */
int wvn_flip_average(const float* a, const float* mirrored, float* out, int B, int G, int C, int ld_src, void* stream);
int wvn_kmeans_cosine(const float* xn, int* labels, int* nseg, void* scratch, int B, int P, int C, int K, int iters,
                      int relabel, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Traversability MLP  (model/simple_mlp.py:10-39, utils/loss.py:93-160,
 * utils/confidence_generator.py:78-82,182-193, traversability_estimator.py:100,464-477)
 * Parameters live in ONE flat fp32 buffer [W1 | b1 | W2 | b2 | W3 | b3], Wi in Linear layout;
 * gradients / Adam moments use the same layout (so the data-parallel exchange is one all-reduce).
 * ------------------------------------------------------------------------------------------- */
typedef struct wvn_mlp_desc {
  int D;  /* input features (384 dino / 90 stego) */
  int H1; /* 256 */
  int H2; /* 32  */
  int reserved; /* model kind: 0 = SimpleMLP, WVN_MLP_KIND_DOUBLE = DoubleMLP (below) */
} wvn_mlp_desc;
/* DoubleMLP (model/double_mlp.py): two independent networks on one input, networks.0 : D -> H1 -> H2 -> 1 (sigmoid, column 0 of
 * the output) and networks.1 : D -> H1 -> H2 -> D (columns 1 .. D), same [R, 1 + D] output as SimpleMLP.  A desc with
 * reserved = WVN_MLP_KIND_DOUBLE selects it in wvn_mlp_param_count, wvn_mlp_workspace_bytes, wvn_mlp_forward (h1 / h2: both NULL or
 * [R][2 H1] / [R][2 H2], networks.0 first; no workspace needed), every wvn_mlp_train_phase_* entry point and wvn_segment_predict
 * (csrc/double_mlp.hip).  Flat layout of parameters, gradients and Adam moments:
 *   [W1a | b1a | W2a | b2a | W3a | b3a | W1b | b1b | W2b | b2b | W3b | b3b],  a = networks.0, b = networks.1, Wi in Linear layout
 * so the data-parallel exchange stays one all-reduce of param_count + 2 floats.  Limits: 1 <= D <= 1024, 1 <= H1, H2 <= 256
 * (WVN_ERR_ARG / 0 otherwise).  The four-launch step (sync_word / fused, as for SimpleMLP) applies to H1 = 64, H2 = 32 and
 * rows <= 2048: wvn_double_mlp_fused_ok; other shapes take the general path whatever the flags say.  wvn_double_mlp_row_tile: the
 * rows one workgroup of these kernels owns.  The wvn_pixel_mlp_* entry points refuse such a desc (0 / WVN_ERR_ARG).
 * reserved = 0 is the SimpleMLP, unchanged. */
#define WVN_MLP_KIND_DOUBLE 1
int wvn_double_mlp_row_tile(void);
int wvn_double_mlp_fused_ok(const wvn_mlp_desc* d, int rows);
size_t wvn_mlp_param_count(const wvn_mlp_desc* d);
size_t wvn_mlp_workspace_bytes(const wvn_mlp_desc* d, int rows);

/* SimpleMLP.forward: x [R,D] -> out [R,1+D] (sigmoid on column 0).  h1/h2 (post-ReLU) may be NULL
 * for inference, in which case they are carved from the workspace. */
int wvn_mlp_forward(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, int R, float* out, float* h1,
                    float* h2, void* workspace, size_t workspace_bytes, void* stream);
/* One optimisation step, split at the two points where data-parallel ranks exchange:
 *  A: forward + per-row reconstruction loss + local statistic  stats[4] (double) =
 *     { n_labelled, sum loss_reco, sum loss_reco^2, R }                    -> all-reduce(sum) stats
 *  B: loss gradient + backward: grads[param_count + 2] (last two = sum weighted trav loss, sum raw
 *     trav loss)                                                            -> all-reduce(sum) grads
 *  C: Adam (lr, betas (0.9,0.999), eps 1e-8) + losses[5] = {total, trav, reco, conf mean, conf std} */
int wvn_mlp_train_phase_a(const wvn_mlp_desc* d, const float* params, const float* x, int ldx,
                          const unsigned char* y_valid, int R, double* stats, void* workspace, size_t workspace_bytes,
                          void* stream);
int wvn_mlp_train_phase_b(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const float* y,
                          const unsigned char* y_valid, int R, const double* stats, float std_factor, float w_trav,
                          float w_reco, float* grads, float* confidence_out, void* workspace, size_t workspace_bytes,
                          void* stream);
int wvn_mlp_train_phase_c(const wvn_mlp_desc* d, float* params, const float* grads, float* adam_m, float* adam_v,
                          int step, float lr, const double* stats, float w_trav, float w_reco, float* losses,
                          void* stream);
/* The step on a COMPACTED batch whose row count lives in device memory (no host synchronisation between segmentation and
 * training): R rows are passed, the first *rows_dev of them are real; the others contribute nothing to statistics, losses or
 * gradients (rows_dev == NULL: all R rows, = the entry points above).  wvn_compact_segment_rows builds such a batch from the
 * pooled features of a frame batch: feat [B][S][D] (+ optional per-row side data [B][S][Dside], e.g. labels), nseg [B] = number
 * of segments that exist per frame -> x_out [B*S][D] / side_out [B*S][Dside] holding the rows (b, s < nseg[b]) front to back in
 * (b, s) order, zeros behind them, and *rows_dev = sum(nseg).  Replaces feat[keep] (traversability_estimator.py:432-446 builds
 * the batch from nodes that all exist; a batched extractor has to drop the ids a frame did not produce). */
int wvn_compact_segment_rows(const float* feat, int D, const float* side, int Dside, const int* nseg, int B, int S, float* x_out,
                             float* side_out, int* rows_dev, void* stream);
/* sync_word (phase A) != NULL and fused (phase B) != 0 select the FOUR-LAUNCH step for the SimpleMLP geometry (H1 = 256, H2 = 32, R <=
 * 2048; csrc/mlp_train.hip): phase A = one launch (all three layers, row losses, statistic -- the last row tile to arrive folds the
 * per-tile partials in tile order; sync_word: a device word that is ZERO on first use and is left at zero), phase B = two launches
 * (gradient seed + dL/dh2 + dL/dh1; the three weight / bias gradients and the loss sums), phase C = one launch (Adam + losses)
 * against 17-20 launches of the general path.  Both phases of a step must take the same path and the same workspace; other
 * geometries fall back to the general path whatever the flags say.  Fixed summation orders: bit-reproducible. */
int wvn_mlp_train_phase_a_rows(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const unsigned char* y_valid,
                               int R, const int* rows_dev, double* stats, void* workspace, size_t workspace_bytes,
                               unsigned int* sync_word, void* stream);
int wvn_mlp_train_phase_b_rows(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const float* y,
                               const unsigned char* y_valid, int R, const int* rows_dev, const double* stats, float std_factor,
                               float w_trav, float w_reco, float* grads, float* confidence_out, void* workspace,
                               size_t workspace_bytes, int fused, void* stream);
/* The step with any ConfidenceGenerator method (utils/confidence_generator.py) and either loss form (utils/loss.py:138-143,
 * anomaly_balanced).  The _rows entry points above are these with method = WVN_CONF_LATEST_MEASUREMENT, balanced = 1 and no
 * state, and give the same bits as these with that configuration.
 *   method   : WVN_CONF_* below.  Every method's update runs before the loss, on this step's positives (the global stats).
 *   balanced : 1 = anomaly_balanced (unlabelled rows weighted by 1 - confidence), 0 = the plain mean of the raw trav loss.
 *   state    : [WVN_CONF_STATE_DOUBLES] device doubles, persistent across steps and owned by the caller.  Layout (WVN_CONF_S_*):
 *              the ConfidenceGenerator parameters mean / var / std (fp32 values), the running_mean sums running_n / sum /
 *              sum_of_squares, and the moving_average window: a ring of WVN_CONF_WINDOW per-step {n, sum, sum^2} with its head
 *              and fill count.  Phases A and B only read it; phase C commits the post-update statistic.  Initial value for a
 *              fresh ConfidenceGenerator: all zeros except var = std = 1.
 *   minmax   : [2] device floats; phase A writes {max, -min} of the reconstruction loss over the real rows of the shard (-inf for
 *              an empty one).  Data-parallel ranks all-reduce it with MAX between phases A and B.  Required for
 *              WVN_CONF_MOVING_AVERAGE (its confidence is min-max scaled over all rows of the step), ignored otherwise.
 * Same launches as the _rows entry points for every method; no host synchronisation.  WVN_ERR_ARG (before any GPU call) for an
 * unknown method, a NULL desc or state, or a NULL minmax with WVN_CONF_MOVING_AVERAGE. */
#define WVN_CONF_LATEST_MEASUREMENT 0
#define WVN_CONF_RUNNING_MEAN 1
#define WVN_CONF_KALMAN_FILTER 2
#define WVN_CONF_MOVING_AVERAGE 3
#define WVN_CONF_WINDOW 5
#define WVN_CONF_STATE_DOUBLES 32
#define WVN_CONF_S_MEAN 0
#define WVN_CONF_S_VAR 1
#define WVN_CONF_S_STD 2
#define WVN_CONF_S_RUN_N 3
#define WVN_CONF_S_RUN_SUM 4
#define WVN_CONF_S_RUN_SUMSQ 5
#define WVN_CONF_S_HEAD 6
#define WVN_CONF_S_FILL 7
#define WVN_CONF_S_RING 8 /* [WVN_CONF_WINDOW][3]; slots 23..31 reserved */
typedef struct wvn_conf_desc {
  int method;
  int balanced;
  double* state;
  float* minmax;
} wvn_conf_desc;
int wvn_mlp_train_phase_a_conf(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const unsigned char* y_valid,
                               int R, const int* rows_dev, double* stats, void* workspace, size_t workspace_bytes,
                               unsigned int* sync_word, const wvn_conf_desc* conf, void* stream);
int wvn_mlp_train_phase_b_conf(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const float* y,
                               const unsigned char* y_valid, int R, const int* rows_dev, const double* stats, float std_factor,
                               float w_trav, float w_reco, float* grads, float* confidence_out, void* workspace,
                               size_t workspace_bytes, int fused, const wvn_conf_desc* conf, void* stream);
/* phase C of such a step: Adam + losses[5] (conf mean / std = the method's post-update statistic) + the state commit */
int wvn_mlp_train_phase_c_conf(const wvn_mlp_desc* d, float* params, const float* grads, float* adam_m, float* adam_v, int step,
                               float lr, const double* stats, float w_trav, float w_reco, float* losses, const wvn_conf_desc* conf,
                               void* stream);
/* quick_start.py:194-210 / loss.py:162-164: trav[r] = out[r][0], conf[r] = confidence(mse(out[r][1:], x[r])) */
int wvn_mlp_confidence(const float* out, int ldo, const float* x, int ldx, float mean, float std, float std_factor,
                       float* trav, float* conf, int R, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused per-pixel traversability inference: the live node's per-frame path with prediction_per_pixel
 * (wvn_feature_extractor_node.py:319-363, quick_start.py:183-210):
 *   dense = bilinear(align_corners) upsample of the patch tokens to [out_h,out_w]  (dino_interface.py:87-90)
 *   out   = SimpleMLP(dense rows); trav = out[:,0] (after its sigmoid); conf = confidence(mse(out[:,1:], dense))
 * without building the dense tensor (308 MB / frame at 448^2) and with layer 1 evaluated at token resolution
 * (csrc/pixel_mlp.hip).  bf16 MFMA operands, fp32 accumulation: the speed mode; the exact mode is
 * wvn_upsample_bilinear + wvn_mlp_forward + wvn_mlp_confidence (or the exact-mode form below).  H1 = 256, H2 = 32 and D = 384 (DINO
 * ViT-S features), D = 768 (ViT-Base features: DINO ViT-B/8, DINOv2 ViT-B/14) or D = 90 (STEGO code, the live node's default
 * feature_type); 0 / WVN_ERR_ARG otherwise.
 * Sizes, with T = ceil(D / 32) + 1 W3 tiles (13 / 25 / 4) and DX = the x columns of a zx row (384 / 768 / 128):
 *   W23 = 16384 + T * 2048 bytes (W2 and W3 fragment images, bf16), NBIAS = 256 + 32 + 32 * T floats
 *   wvn_pixel_mlp_pack_bytes             = 256 * DX * 2 + W23 + 4 * NBIAS
 *   wvn_pixel_mlp_zx_cols                = 256 + DX
 *   wvn_pixel_mlp_exact_pack_bytes       = 2 * W23 + 4 * NBIAS                    (hi and lo images)
 *   wvn_pixel_mlp_exact_workspace_bytes  = rows * 256 * 4 + 2 * rows * (256 + 32 * (T - 1)) * 2 + 256,  rows = batch * grid^2
 *
 * packed : wvn_pixel_mlp_pack_bytes() bytes, rebuilt by wvn_pixel_mlp_pack whenever the parameters change
 *          (the node reloads them at 1 Hz, wvn_feature_extractor_node.py:407-432).
 * zx     : [batch*grid*grid rows][ldzx >= wvn_pixel_mlp_zx_cols()] bf16 (640 for D = 384, 1024 for D = 768, 384 for D = 90).  Columns from 256 on
 *          hold the features on entry (D = 384 / 768: hand wvn_vit_forward tokens_lowp = zx + 256, ld_lowp = ldzx; D = 90: the 90
 *          code values followed by ZEROS up to column 384); columns [0,256) are scratch (layer-1 pre-activations).
 * trav / conf / loss_reco : [batch][out_h][out_w] fp32, each may be NULL.  mean/std/std_factor: ConfidenceGenerator state;
 * conf_state (may be NULL): the same three floats in DEVICE memory, read by the kernel instead of the scalars -- lets the call
 * sit in a captured HIP graph while the confidence statistics keep moving.
 * Requires 15*(grid-1)/(out-1) < 2 in both directions (out >= ~7.5 x grid: 224/28, 448/56 ...), WVN_ERR_ARG otherwise.
 * ------------------------------------------------------------------------------------------- */
#define WVN_PIXEL_ZX_COLS 640   /* D = 384; wvn_pixel_mlp_zx_cols() for any supported D */
#define WVN_PIXEL_X_COL 256
size_t wvn_pixel_mlp_pack_bytes(const wvn_mlp_desc* d);
int wvn_pixel_mlp_zx_cols(const wvn_mlp_desc* d);
int wvn_pixel_mlp_pack(const wvn_mlp_desc* d, const float* params, void* packed, void* stream);
int wvn_pixel_mlp_infer(const wvn_mlp_desc* d, const void* packed, void* zx, int ldzx, int batch, int grid, int out_h,
                        int out_w, float mean, float std, float std_factor, const float* conf_state, float* trav,
                        float* conf, float* loss_reco, void* stream);

/* Exact-mode form of the same fused kernel: every MFMA operand is split into hi + lo bf16 parts and every product is formed
 * as hi*hi + hi*lo + lo*hi (fp32 accumulation), the token-resolution layer-1 GEMM runs on the fp32 FMA path: results agree
 * with the fp32 reference sequence to ~1e-5 relative (the 1e-3 bar of the exact mode), at 2.3x the MFMA work of the bf16
 * form.  tokens: [batch*grid*grid][ld_tokens >= D] fp32 features (D = 384 / 768: wvn_vit_forward tokens_f32; D = 90: the STEGO code);
 * params: the flat fp32 parameter buffer (W1 is read from it); packed: wvn_pixel_mlp_exact_pack_bytes() bytes from
 * wvn_pixel_mlp_exact_pack; workspace: wvn_pixel_mlp_exact_workspace_bytes() bytes, no initialisation needed. */
size_t wvn_pixel_mlp_exact_pack_bytes(const wvn_mlp_desc* d);
size_t wvn_pixel_mlp_exact_workspace_bytes(const wvn_mlp_desc* d, int batch, int grid);
int wvn_pixel_mlp_exact_pack(const wvn_mlp_desc* d, const float* params, void* packed, void* stream);
int wvn_pixel_mlp_infer_exact(const wvn_mlp_desc* d, const float* params, const void* packed, const float* tokens,
                              int ld_tokens, int batch, int grid, int out_h, int out_w, float mean, float std,
                              float std_factor, const float* conf_state, float* trav, float* conf, float* loss_reco,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Anomaly detection: the forward pass of the LinearRnvp flow (model/linear_rnvp.py:216-296 as get_model builds it: two coupling
 * layers with separate s and t networks D -> h -> h -> D, each followed by a permutation; csrc/rnvp.hip).  Per coupling layer,
 * m = mask:  mu = u*m;  s = tanh(S(mu));  t = T(mu);  x = mu + (1-m)*(u*exp(s) + t);  log_det += sum((1-m)*s);  then x = x[:, p].
 *   score[r] = sum_c(-z[r][c]^2 / 2 - log(sqrt(2 pi))) + log_det[r]      (AnomalyLoss: logprob.sum(1) + log_det, unit normal prior)
 * Every matrix product is formed from hi + lo bf16 operand pairs (three MFMAs, fp32 accumulation): the fp32 reference to ~2^-16.
 * D = 384 or 90, 1 <= h <= 256, flows = 2; 0 / WVN_ERR_ARG otherwise.
 *
 * params : fp32, per flow and per network (s, then t): W1 [h][D] | b1 [h] | W2 [h][h] | b2 [h] | W3 [D][h] | b3 [D]  (Linear layout)
 * mask   : [flows][D] fp32 zeros and ones, D/2 ones per flow;  perm: [flows][D] int64, the permutation buffers p
 * packed : wvn_rnvp_pack_bytes() bytes, 16-byte aligned, rebuilt by wvn_rnvp_pack whenever parameters, masks or permutations change
 * rows   : x [R][ldx >= D] fp32.  pixels: tokens [batch*grid*grid][ld_tokens >= D] fp32; row (b, y, x) is the align_corners=True
 *          bilinear blend of its four tokens, formed in fp32 inside the kernel (the dense tensor is never written), R = batch*out_h*out_w
 *          (2 <= grid <= 4096, out_h, out_w >= 2, R < 2^31)
 * score  : [R].  log_det: [R] or NULL.  z: [R][ldz >= D] in the reference's column order, or NULL.
 * conf   : [R] or NULL: confidence(-score) with the interval formula of ConfidenceGenerator; mean / std / std_factor as
 *          scalars, or conf_state (may be NULL): the same three floats in device memory, read instead.
 * wvn_rnvp_row_tile(): the rows one workgroup processes at a time (callers need it for nothing; tests place R around it).
 * ------------------------------------------------------------------------------------------- */
typedef struct wvn_rnvp_desc {
  int D;
  int h;
  int flows;
} wvn_rnvp_desc;
size_t wvn_rnvp_pack_bytes(const wvn_rnvp_desc* d);
int wvn_rnvp_row_tile(void);
int wvn_rnvp_pack(const wvn_rnvp_desc* d, const float* params, const float* mask, const long long* perm, void* packed, void* stream);
int wvn_rnvp_forward_rows(const wvn_rnvp_desc* d, const void* packed, const float* x, int ldx, long long R, float mean, float std,
                          float std_factor, const float* conf_state, float* score, float* conf, float* log_det, float* z, int ldz,
                          void* stream);
int wvn_rnvp_forward_pixels(const wvn_rnvp_desc* d, const void* packed, const float* tokens, int ld_tokens, int batch, int grid,
                            int out_h, int out_w, float mean, float std, float std_factor, const float* conf_state, float* score,
                            float* conf, float* log_det, float* z, int ldz, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Anomaly detection: one optimisation step of the flow (AnomalyLoss: loss = -mean(score) over ALL ranks' rows, torch.optim.Adam
 * defaults; csrc/rnvp_train.hip), in the three phases of the traversability MLPs' step with the same two exchanges:
 *   phase_a : forward on this rank's rows x [R][ldx >= D] -> score [R], the backward pass's activations -> workspace, and the
 *             LOCAL statistic stats[4] = {n, sum x, sum x^2, n} of x = -score (fp64)            -> all-reduce(sum) of stats
 *   phase_b : grads [param_count] fp32 in params order from the workspace phase_a filled and the GLOBAL stats (seed -1/n);
 *             parameters the masks disconnect get exact zeros                                   -> all-reduce(sum) of grads
 *   phase_c : Adam step `step` (>= 1) on params with moments adam_m / adam_v; losses[3] = {loss, mean, std}; the confidence
 *             statistic of `method` (WVN_CONF_*) is committed to conf_state [WVN_CONF_STATE_DOUBLES] from the global stats (every
 *             row is a positive); packed and train_packed are rebuilt from the new params.
 * R = 0 is legal in phase_a / phase_b (an empty shard contributes zeros); R <= 65536.  One fixed summation order, no atomics:
 * bitwise reproducible.  No host synchronisation; the launch count does not depend on R.
 * train_packed : wvn_rnvp_train_pack_bytes() bytes, 16-byte aligned: the transposed weight images, built by wvn_rnvp_train_pack
 *                from params and the forward blob `packed` (whose column tables it reads).
 * workspace    : wvn_rnvp_train_workspace_bytes(d, R) bytes, 16-byte aligned, the same memory in phase_a and phase_b.
 * Sizes are 0 and calls return WVN_ERR_ARG, before any launch, for NULL pointers, R < 0, an unsupported (D, h) or a workspace
 * that is too small.
 * ------------------------------------------------------------------------------------------- */
size_t wvn_rnvp_train_param_count(const wvn_rnvp_desc* d);
size_t wvn_rnvp_train_workspace_bytes(const wvn_rnvp_desc* d, long long R);
size_t wvn_rnvp_train_pack_bytes(const wvn_rnvp_desc* d);
int wvn_rnvp_train_pack(const wvn_rnvp_desc* d, const float* params, const void* packed, void* train_packed, void* stream);
int wvn_rnvp_train_phase_a(const wvn_rnvp_desc* d, const void* packed, const float* x, int ldx, long long R, float* score,
                           double* stats, void* workspace, size_t workspace_bytes, void* stream);
int wvn_rnvp_train_phase_b(const wvn_rnvp_desc* d, const void* packed, const void* train_packed, long long R, const double* stats,
                           float* grads, void* workspace, size_t workspace_bytes, void* stream);
int wvn_rnvp_train_phase_c(const wvn_rnvp_desc* d, float* params, const float* grads, float* adam_m, float* adam_v, int step, float lr,
                           const double* stats, int method, double* conf_state, float* losses, const float* mask,
                           const long long* perm, void* packed, void* train_packed, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused per-segment traversability inference: the node's per-frame path with prediction_per_pixel = False
 * (wvn_feature_extractor_node.py:320-366, quick_start.py:184-210):
 *   input_feat = feat[seg.reshape(-1)];  out = SimpleMLP(input_feat)
 *   trav = out[:,0] (after its sigmoid);  loss_reco = mse(out[:,1:], input_feat);  conf = confidence(loss_reco)
 * with the MLP evaluated once per SEGMENT row and the results painted onto the segment maps (csrc/segment_predict.hip):
 * no [H*W, D] gather, two launches, no host synchronisation.  fp32 FMA throughout, one fixed summation order per row: a
 * pixel's outputs depend on its segment's features and the parameters only (not on B, S or the row's position).
 *
 * feat     : [B][S][D] fp32, element (b, s, k) at feat[b * ld_frame + s * ld_row + k]; ld_row >= D, ld_frame >= 0 (0: every
 *            frame shares one table).  NaN rows are allowed (extract_batch writes them for ids a frame does not contain): they
 *            give NaN at the pixels that reference them and nowhere else.
 * seg      : [B][H][W] segment ids, int32 (seg_bytes = 4, extract_batch) or int64 (seg_bytes = 8, extract).  Id rule of torch
 *            indexing: ids in [0, S) select row id, ids in [-S, 0) select row S + id (the -1 ids of segmentation_type
 *            "random"), any other id gives NaN in every output.
 * trav / conf / loss_reco : [B][H][W] fp32, each may be NULL.  mean/std/std_factor: ConfidenceGenerator state; conf_state
 *            (may be NULL): the same three floats in DEVICE memory, read instead of the scalars (HIP-graph capture).
 * workspace: wvn_segment_predict_workspace_bytes() bytes, 16-byte aligned, no initialisation needed (receives the per-segment
 *            table {trav, conf, loss_reco, 0}, [B*S][4] fp32).  params: the flat parameter buffer, 16-byte aligned.
 * Limits: H1 = 256, H2 = 32, 1 <= D <= 1024; B <= 65535, B*S <= 2^26, H*W < 2^31.  WVN_ERR_ARG otherwise (and for NULL
 * params / feat / seg / workspace or seg_bytes other than 4 or 8), checked on the host before any GPU call; the workspace
 * query returns 0 for an unsupported geometry.
 * ------------------------------------------------------------------------------------------- */
size_t wvn_segment_predict_workspace_bytes(const wvn_mlp_desc* d, int B, int S);
int wvn_segment_predict(const wvn_mlp_desc* d, const float* params, const float* feat, int ld_row, long long ld_frame,
                        int B, int S, const void* seg, int seg_bytes, int H, int W, float mean, float std, float std_factor,
                        const float* conf_state, float* trav, float* conf, float* loss_reco, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SimpleGCN (model/simple_gcn.py, csrc/simple_gcn.hip): three graph-convolution layers D -> H1 (ReLU) -> H2 (ReLU) -> 1 + D
 * (sigmoid on column 0), each one GCNConv with torch_geometric's defaults: edges with source == target dropped, one self loop
 * per node added, deg_i = edges into i, out_i = sum_{e: j -> i} deg_j^-1/2 deg_i^-1/2 (x_j W^T) + b.  The edge list is used as
 * given (not symmetrised, duplicates kept).  desc: D, H1, H2 with reserved = 0; the flat parameter layout [W1|b1|W2|b2|W3|b3] and
 * wvn_mlp_param_count are SimpleMLP's for the same (D, H1, H2).  Limits: 1 <= D <= 1024, 1 <= H1, H2 <= 256, nodes <= 2^26,
 * capacity <= 2^30 (WVN_ERR_ARG otherwise, checked on the host before any GPU call; the workspace query returns 0).
 *
 * A call sequence shares ONE workspace and the same (nodes, capacity): a graph preparation, then any number of forwards on it.
 *   capacity : neighbour entries the workspace holds, >= E + nodes for an edge list, >= B * S * S for bitmaps.
 *   wvn_gcn_graph_from_edges   : edge_index int64, element (row, e) at edge_index[row * ld_row + e * ld_edge], row 0 = source,
 *                                row 1 = target.  An edge with an endpoint outside [0, nodes) is dropped, never dereferenced, and
 *                                counted in *bad_edges (device int32, reset by the call).  No host reads; 4 launches.
 *   wvn_gcn_graph_from_bitmaps : adj uint8, element (b, l, r) at adj[b * ld_b + l * ld_l + r * ld_r], nonzero = an edge from node
 *                                b * S + l to node b * S + r (ops.seg_adjacency_batched); the diagonal is ignored.  bad_edges
 *                                (may be NULL) is reset.  3 launches.
 *   Both leave the target-major form {row pointers, sources in ASCENDING order with the self loop among them, coefficients}.
 *   wvn_gcn_forward            : x [nodes][ldx >= D] -> out [nodes][1 + D]; 3 launches, one per layer.
 *   wvn_gcn_segment_predict    : wvn_segment_predict for this model on feat [B * S][ld_row] (node b * S + s): the last layer forms
 *                                the row's reconstruction loss and confidence and fills the {trav, conf, loss_reco, 0} table, the
 *                                paint kernel of segment_predict.hip spreads it (same seg id rule); 3 + 1 launches.
 * fp32 FMA throughout, no floating-point atomics: every sum has one fixed ascending order, so a row's results do not depend on
 * the edge order, the row's position or the batch around it, and a NaN row reaches only the rows within three hops.
 * ------------------------------------------------------------------------------------------- */
size_t wvn_gcn_workspace_bytes(const wvn_mlp_desc* d, int nodes, long long capacity);
int wvn_gcn_graph_from_edges(const long long* edge_index, long long ld_row, long long ld_edge, int E, int nodes, long long capacity,
                             int* bad_edges, void* workspace, size_t workspace_bytes, void* stream);
int wvn_gcn_graph_from_bitmaps(const unsigned char* adj, long long ld_b, long long ld_l, long long ld_r, int B, int S, long long capacity,
                               int* bad_edges, void* workspace, size_t workspace_bytes, void* stream);
int wvn_gcn_forward(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, int nodes, long long capacity, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);
int wvn_gcn_segment_predict(const wvn_mlp_desc* d, const float* params, const float* feat, int ld_row, int B, int S, long long capacity,
                            const void* seg, int seg_bytes, int H, int W, float mean, float std, float std_factor,
                            const float* conf_state, float* trav, float* conf, float* loss_reco, void* workspace, size_t workspace_bytes,
                            void* stream);
/* The SimpleGCN training step (csrc/simple_gcn_train.hip) in the three phases of the MLP step: the same statistic
 * stats = {n_lab, sum, sum^2, R}, the same grads [wvn_mlp_param_count + 2] with the two loss sums behind the gradient, the same
 * wvn_conf_desc.  Phase C is wvn_mlp_train_phase_c / wvn_mlp_train_phase_c_conf on the same descriptor.  The caller all-reduces
 * stats (and MAX-reduces conf->minmax for moving_average) between A and B, and grads between B and C.
 *   wvn_gcn_train_workspace_bytes : the step's workspace for (nodes, capacity >= E + nodes); nodes <= 65536 (0 otherwise).  Its head is
 *                                   the inference workspace of the same (nodes, capacity).
 *   wvn_gcn_train_phase_a : graph preparation from the edge list (the rule for bad edges and *bad_edges as in
 *                           wvn_gcn_graph_from_edges), its transpose (every source's targets ascending, the coefficient carried
 *                           with its edge), the three layers with h1, h2 and out kept (the forward values are bit for bit those
 *                           of wvn_gcn_forward), the rows' reconstruction losses and the local statistic.  sync_word: a device
 *                           word, zeroed by the call.  conf may be NULL: latest_measurement, anomaly_balanced.  11 launches.
 *   wvn_gcn_train_phase_b : clears grads; the gradient seed (confidence_out [nodes], optional), the backward layers on the
 *                           transposed graph, all weight and bias gradients and the loss sums.  5 launches.
 *   wvn_gcn_train_saved   : byte offsets {h1 [nodes][H1], h2 [nodes][H2], out [nodes][1 + D]} of the values phase A keeps in the
 *                           workspace (a test and debug accessor; host arithmetic).
 * Every check is made on the host: a NULL pointer, nodes < 1, an unsupported width or a workspace that is too small gives
 * WVN_ERR_ARG before any launch.  No floating-point atomics; every sum has one fixed ascending order: a step is bitwise
 * reproducible and does not depend on the order of the edges.  No launch count depends on nodes or E; nothing is read on the host. */
size_t wvn_gcn_train_workspace_bytes(const wvn_mlp_desc* d, int nodes, long long capacity);
int wvn_gcn_train_saved(const wvn_mlp_desc* d, int nodes, long long capacity, size_t* offsets);
int wvn_gcn_train_phase_a(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const long long* edge_index, long long ld_row,
                          long long ld_edge, int E, const unsigned char* y_valid, int nodes, long long capacity, double* stats,
                          int* bad_edges, void* workspace, size_t workspace_bytes, unsigned int* sync_word, const wvn_conf_desc* conf,
                          void* stream);
int wvn_gcn_train_phase_b(const wvn_mlp_desc* d, const float* params, const float* x, int ldx, const float* y, const unsigned char* y_valid,
                          int nodes, long long capacity, const double* stats, float std_factor, float w_trav, float w_reco, float* grads,
                          float* confidence_out, void* workspace, size_t workspace_bytes, const wvn_conf_desc* conf, void* stream);
/* wvn_seg_adjacency's bitmap for a batch of frames, without the edge list: adj [B][S][S] uint8, adj[b][r * S + l] = 1 exactly for
 * the (left l, right r) pairs wvn_seg_adjacency returns for frame b (its transposed view is wvn_gcn_graph_from_bitmaps' (b, l, r)
 * element).  No host synchronisation. */
int wvn_seg_adjacency_batched(const int* seg, unsigned char* adj, int B, int H, int W, int S, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A -> B wire format: the per-frame wild_visual_navigation_msgs/ImageFeatures message built at
 * wvn_feature_extractor_node.py:373-393 (seg.cpu().numpy().astype(np.int32) + feat.cpu().numpy().flatten().tolist()) and
 * decoded at wvn_learning_node.py:651-656.  wvn_wire_pack lays the frame out on the device as the message carries it:
 *   [ 64-byte header {magic "WVNF", version, H, W, S, D, seg_offset, feat_offset} | int32 seg[H*W] | float32 feat[S*D] ]
 * (the two payload sections are the byte arrays of Image.data, step 4*W, and Float32MultiArray.data): one contiguous
 * device->host copy per frame instead of two copies, a host cast and a Python list.  wvn_wire_unpack is the inverse on the
 * learner's GPU (segments as int64, what MissionNode stores, and/or int32).  out / in: 16-byte aligned, wvn_wire_bytes() bytes.
 * ------------------------------------------------------------------------------------------- */
size_t wvn_wire_bytes(int H, int W, int S, int D);
int wvn_wire_pack(const void* seg, int seg_is_i64, const float* feat, int ldf, void* out, int H, int W, int S, int D, void* stream);
int wvn_wire_unpack(const void* in, long long* seg_i64, int* seg_i32, float* feat, int H, int W, int S, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Instrumentation (scripts/a384_timing.py, scripts/attn_timing.py): in-kernel s_memtime phase timings of
 * the two MFMA kernels.  Not part of the drop-in surface.
 * ------------------------------------------------------------------------------------------- */
/* wvn_gemm_bf16 with per-wave phase counters: dbg[(workgroup * 8 + wave) * 4 + {0 wait+barrier, 1 MFMA block,
 * 2 epilogue part, 3 total}] in shader cycles (K == 384 shapes only; dbg may be NULL). */
int wvn_debug_gemm_bf16_timed(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M,
                              int N, int K, int epi, long long* dbg, void* stream);
/* The A-stationary split-operand GEMM for K = 384 (csrc/gemm_a384_x3.hip: what WVN_PREC_MIX / WVN_PREC_X3 run for QKV, projection
 * and fc1 from 8192 rows on), callable on its own: A / W as hi + lo bf16 planes ([M][384], [N][384]; the lo planes at A_lo / W_lo,
 * W_lo behind W in one allocation), epi = 1 (erf GELU, hi / lo bf16 planes C / C_lo [M][ldc]) or 4 (fp32 C [M][ldc] += result).
 * dbg != NULL: the instrumented build writes dbg[(workgroup * 4 + wave) * 4 + {0 wait + barrier, 1 DMA issue, 2 MFMA steps with the
 * epilogue chunks, 3 total}] in shader cycles (scripts/bench_a384_x3.py).  WVN_ERR_ARG when the shape is not eligible. */
int wvn_debug_gemm_a384_x3(const void* A, const void* A_lo, int lda, const void* W, const void* W_lo, const float* bias, void* C,
                           void* C_lo, int ldc, int M, int N, int epi, long long* dbg, void* stream);
/* The row-panel split-operand GEMM for N = 384 residual updates (csrc/gemm_n384_x3.hip: fc2 and the attention projection of
 * WVN_PREC_MIX / WVN_PREC_X3 from 8192 rows on): C [M][ldc] fp32 += (A W^T + bias) (* ls), A [M][lda] / W [384][K] as hi + lo bf16 planes
 * (lo planes behind the hi planes in one allocation each), K % 32 == 0.  dbg != NULL: the instrumented build writes
 * dbg[(workgroup * 4 + wave) * 4 + {0 wait + barrier, 1 k-steps, 2 epilogue, 3 total}] in shader cycles. */
int wvn_debug_gemm_n384_x3(const void* A, const void* A_lo, int lda, const void* W, const void* W_lo, const float* bias, const float* ls,
                           float* C, int ldc, int M, int K, long long* dbg, void* stream);
/* The split-operand block MLP with the fragment-major hand-over (what WVN_PREC_MIX / WVN_PREC_X3 run at D = 384 from 8192 rows on):
 * hid = gelu(xn W1^T + b1) written by csrc/gemm_a384_x3.hip as MFMA operand fragments (hi / lo planes, ceil(M / 32) * 32 rows of F each),
 * x [M][384] fp32 += hid W2^T + b2 by csrc/gemm_n384_x3.hip; xn / W1: hi + lo bf16 planes, W2p: wvn_vit_layer.fc2_w_fused in its
 * WVN_PREC_X3 / WVN_PREC_MIX layout.  dbg1 / dbg2 (optional): per-wave cycle counters of the two instrumented builds. */
int wvn_debug_mlp_x3_frag(const void* xn, const void* xn_lo, const void* W1, const void* W1_lo, const float* b1, void* hid, void* hid_lo,
                          const void* W2p, const float* b2, float* x, int M, int F, long long* dbg1, long long* dbg2, void* stream);
/* The MX form of the row-panel kernel (round 6; what WVN_PREC_MIX runs for fc2 and the attention projection by default): every operand as
 * an fp16 value h, the e5m2 image l8 of its rounding residue * 2^12 and the e5m2 image h8 of the value; the product = A_h W_h on fp16 MFMAs
 * + 2^-12 (A_h8 W_l8 + A_l8 W_h8) on scaled 8-bit MFMAs of K = 64 (csrc/gemm_n384_x3.hip: gemm_n384_mx_pair_kernel).  A_h: fragment-major
 * fp16 [ceil(M / 32)][K / 16][64 lanes][8]; A_l8: [ceil(M / 32)][K / 64][2 halves][64 lanes][16 bytes] (backbone.mx_fragments states
 * the element order), behind A_h inside one 4 GB span; A_h8 is ignored (may be NULL): the kernel derives e5m2(A_h) in registers; Wp: backbone.pack_n384_mx(W [384][K]); C [M][ldc] fp32 += (A W^T + bias) (* ls);
 * K % 128 == 0.  dbg as wvn_debug_gemm_n384_x3. */
int wvn_debug_gemm_n384_mx(const void* A_h, const void* A_l8, const void* A_h8, const void* Wp, const float* bias, const float* ls, float* C,
                           int ldc, int M, int K, long long* dbg, void* stream);
/* The block MLP of WVN_PREC_MIX in its MX form: hid = gelu(LayerNorm(x) W1^T + b1) by csrc/gemm_a384_x3.hip (LayerNorm formed on load from
 * ln_stats[m] = {mean, 1 / sqrt(var + eps)}; W1p = backbone.pack_a384_mx(fc1.weight)), written as the MX operand planes hid_h / hid_l8 (hid_h8 is
 * ignored and may be NULL) (fragment-major, ceil(M / 32) * 32 rows of F), then xout [M][384] fp32 += hid W2^T + b2 by the MX row-panel kernel (W2p =
 * backbone.pack_n384_mx(fc2.weight)).  W2p == NULL: fc1 only.  dbg1 / dbg2: per-wave cycle counters of the instrumented builds. */
int wvn_debug_mlp_mx(const float* x, int ldx, const float* ln_stats, const float* ln_g, const float* ln_b, const void* W1p, const float* b1,
                     void* hid_h, void* hid_l8, void* hid_h8, const void* W2p, const float* b2, float* xout, int M, int F, long long* dbg1,
                     long long* dbg2, void* stream);
/* LayerNorm-on-load + QKV in the MX form: q (pre-scaled by q_scale; q_lo != NULL: its fp16 rounding residue as a second plane) | k | v^T fp16 in
 * the layouts of wvn_attention_f16 (Wp = backbone.pack_a384_mx(qkv.weight)). */
int wvn_debug_qkv_mx(const float* x, int ldx, const float* ln_stats, const float* ln_g, const float* ln_b, const void* Wp, const float* bias, void* q,
                     void* q_lo, void* k, void* vt, int heads, int npad, int ntok_s, float q_scale, int M, long long* dbg, void* stream);
/* The first launch of wvn_vit_forward_frames_head's head alone (gemm_a384_x3.hip, X_HEAD): x [frames * ntok_s][ldx] fp32 residual rows (patch p of
 * frame f is row f * ntok_s + 1 + p; the other rows are never read), stats[row] = {mean, rstd}; w_cat / b_cat as in wvn_stego_head; hid / hid_lo: the hi / lo
 * bf16 planes [frames * npatch][384] of ReLU(LayerNorm(x) W_hid^T + b_hid); code [frames * npatch][ld_code] fp32: columns 0 .. 127 = LayerNorm(x) W_lin^T + b_lin. */
int wvn_debug_stego_head_fused(const float* x, int ldx, const float* stats, const float* ln_g, const float* ln_b, const void* w_cat, const float* b_cat,
                               void* hid, void* hid_lo, float* code, int ld_code, int frames, int npatch, int ntok_s, void* stream);
/* subsequent wvn_attention_bf16 launches write dbg[(workgroup * 4 + wave) * 5 + {0 wait, 1 QK^T, 2 softmax, 3 PV,
 * 4 total}]; NULL switches the instrumented build off again. */
/* (test hook) out_f16[i] = fp16(in[i]) as the kernels convert: finite values beyond the fp16 range saturate to +-65504 (MODE.FP16_OVFL) */
int wvn_debug_f16_saturate(const float* in, void* out_f16, int n, void* stream);
/* (test hook) the Lab conversion of wvn_slic alone (slic_lab_kernel, one launch): img [3][npix] planar, uint8 (img_is_u8) or float;
 * lut_lin / lut_f as for wvn_slic; lab [3][npix] int32 = (L, a, b) * 64.  WVN_ERR_ARG for a NULL pointer or npix <= 0. */
int wvn_debug_slic_lab(const void* img, int img_is_u8, int npix, const int* lut_lin, const int* lut_f, int* lab, void* stream);
int wvn_debug_attention_timing(long long* dbg);
/* which form of the pre-scaled (scale == 0) attention kernel subsequent launches use: 0 = exact per-tile row max, 1 = lazy (no
 * per-tile max; the row sums raise the alarm and the tile is redone exactly -- the default), < 0 = back to the default.  Same
 * results within the kernel's tolerance; tests/test_gpu_attention_lazy.py runs both, bench.py --attn-variant A/Bs them.  Any other
 * value below 16 selects the default lazy form, bit for bit (2 once selected a lazy form with fp32-add row sums, which is retired);
 * 17 / 18 select the form of the two-plane q instead. */
int wvn_debug_attention_variant(int variant);
/* The fp16-operand attention kernel exactly as WVN_PREC_MIX's wvn_vit_forward launches it, with the form of the two-plane q as an argument
 * (no process setting is read or changed for it; form 0 runs the single-plane form wvn_debug_attention_variant selects).  q pre-scaled by softmax_scale * log2(e) (the kernel runs with scale = 0), q / q_lo / k
 * fp16 [B * heads][npad][64], vt fp16 [B * heads][64][npad] in the token order of wvn_attention_bf16; rows [ntok, npad) finite.
 * qsplit_form: 0 = one q plane (q_lo must be NULL), 1 = q + q_lo on fp16 MFMAs, 2 = q_lo as e5m2(q_lo * 2^12) on one scaled 8-bit MFMA
 * per 32 keys (what ships).  Output row of query t of frame b: m = b * ntok_s + t (ntok <= ntok_s <= npad):
 *   out_frag 0, out_lo NULL: out fp16 [B * ntok_s][heads * 64] row-major;
 *   out_frag 0, out_lo set:  out / out_lo bf16 hi / lo planes (o = hi + lo), [B * ntok_s][heads * 64] row-major each;
 *   out_frag 1 (heads = 6):  out / out_lo bf16 hi / lo planes, fragment-major [ceil(B * ntok_s / 32)][24 k-steps][64 lanes][8]
 *                            (ops.unpack_row_fragments);
 *   out_frag 2 (heads = 6):  the MX operand planes of wvn_debug_gemm_n384_mx: out = h fp16 [ceil(B * ntok_s / 32)][24][64][8], out_lo = l8
 *                            [ceil(B * ntok_s / 32)][6][2][64][16] bytes (backbone.mx_fragments / mx_unfragments); rows t in [ntok, ntok_s)
 *                            of every frame are written as zeros in both planes.
 * Forms 0 / 1 write only rows t < ntok; no form writes rows past B * ntok_s.  WVN_ERR_ARG for any other combination. */
int wvn_debug_attention_planes(const void* q, const void* q_lo, const void* k, const void* vt, void* out, void* out_lo, int B, int heads,
                               int ntok, int ntok_s, int npad, int out_frag, int qsplit_form, void* stream);
/* which assignment kernel subsequent wvn_kmeans_cosine_pixels calls use: -1 / 5 = the PACKED VALU form where it is eligible (K <= 20;
 * default): the fmaf chains of two clusters ride in the two halves of v_pk_fma_f32, the interpolation runs on channel pairs; 4 = packed
 * dot products, plain interpolation; 0 = the plain VALU form (one v_fma_f32 per cluster and channel); 1 = the SCREENED form where it is
 * eligible (K <= 20): similarities from split-operand bf16 MFMAs decide every pixel whose best beats the runner-up by more than the
 * proven error bound, the exact fmaf chains of the definition decide the rest -- faster where the code has cluster structure, slower
 * on structure-less code (csrc/stego.hip); 2 = the screened kernel with every row sent down its exact path (tests); 3 = the screened
 * kernel counting its exact rows (wvn_debug_kmeans_screen_stats).  Bit-identical labels and centroids in all of them;
 * tests/test_gpu_stego_pixels.py runs them, scripts/bench_pixel_kmeans.py A/Bs them. */
/* the fragment form of the split-operand row-panel kernel (fc2 / projection of WVN_PREC_MIX / WVN_PREC_X3): 1 = a wave PAIR per 32 rows, two waves per
 * SIMD (round 5, default: 12 % fewer cycles per k-step, fc2 -4 % wall time), 0 = one wave per SIMD (round 4).  Bit-identical C; A/B and tests */
int wvn_debug_n384_pair(int on);
int wvn_debug_kmeans_assign_form(int form);
/* image rows of a band the linear form's assign kernel works on at a time (LDS per workgroup against barriers per band; default 4) */
int wvn_debug_kmeans_linear_rows(int rows);

/* statistics of the screened kernel (synchronises the device): out[0] = 64-pixel row groups it re-did with the exact chains, out[1] = row
 * groups it saw, since the last call with reset != 0 */
int wvn_debug_kmeans_screen_stats(unsigned long long* out, int reset);
/* subsequent wvn_qkv_fused launches write dbg[(workgroup * 4 + wave) * 4 + {0 LayerNorm prologue, 1 MFMA slices, 2 tile epilogues,
 * 3 total}] in shader cycles (scripts/bench_qkv_fused.py); NULL switches the instrumented build off again. */
int wvn_debug_qkv_fused_timing(long long* dbg);
/* the same for wvn_mlp_fused with the LayerNorm inside: dbg[(workgroup * 4 + wave) * 6 + {0 row prologue (LayerNorm), 1 fc1 slices,
 * 2 GELU + pack, 3 fc2 slices, 4 epilogue, 5 total}] (scripts/bench_mlp_fused.py) */
int wvn_debug_mlp_fused_timing(long long* dbg);
/* the row-panel N = 384 residual GEMM on every row block, whatever M (the dispatcher of wvn_gemm_bf16 only uses it from about
 * 0.75 x #CU row blocks of 256 on); tests */
int wvn_debug_gemm_n384(const void* A, int lda, const void* W, int ldw, const float* bias, float* C, int ldc, int M, int K,
                        void* stream);


/* ---- exact dense CRF (csrc/dense_crf.hip; DESIGN.md "Dense CRF") ----
 * Mean-field inference of the fully connected CRF of the public STEGO crf.py / pydensecrf DenseCRF2D recipe with every pixel pair
 * evaluated: unary -log(clip(softmax(logits), 1e-5, 1)), smoothness kernel exp(-|dp|^2 / (2 pos_xy_std^2)) (weight pos_w; radius
 * ceil(8 pos_xy_std), pos_xy_std <= 4), appearance kernel exp(-|dp|^2 / (2 bi_xy_std^2) - |dI|^2 / (2 bi_rgb_std^2)) (weight bi_w),
 * symmetric normalisation, Potts compatibility, `iterations` (1..1000) updates.  Two CRFs on the same image may share the pass:
 * logits1 (K1 >= 1 columns) and logits2 (K2 >= 0; NULL iff K2 == 0), K1 + K2 <= 64, each addressed as p[b * sb + k * sc + pixel * sp]
 * (fp32; pixel = y * W + x).  image: u8 [B][H][W][3].  Outputs (any may be NULL, not all): labels int32 [B][1 or 2][H][W] (first
 * maximum of the final Q, ids within each group; nseg_last non-NULL (needs labels): the last group's ids are compacted to ascending
 * contiguous ids as the k-means relabel does and nseg_last [B] receives their count), probs fp32 [B][K1 + K2][H][W] (final Q), debug fp32 [B][2 KP + 2][H][W] with
 * KP = 32 (K1 + K2 <= 32) or 64: rows 0..KP-1 the last iteration's bilateral message n_b(i) sum_j k_b n_b(j) Q_j, rows KP..2KP-1 the
 * smoothness message, row 2 KP n_b, row 2 KP + 1 n_g (tests).  workspace: wvn_dense_crf_workspace_bytes(B, H, W, K1 + K2) bytes,
 * 256-byte aligned, no initialisation.  B <= 65535, H, W <= 2048.  WVN_ERR_ARG (before any GPU call) for any other shape, a NULL
 * input, non-positive standard deviations or non-finite weights; WVN_ERR_WORKSPACE when the workspace is too small. */
size_t wvn_dense_crf_workspace_bytes(int B, int H, int W, int K);
int wvn_dense_crf(const float* logits1, int K1, long long s1b, long long s1c, long long s1p, const float* logits2, int K2, long long s2b,
                  long long s2c, long long s2p, const unsigned char* image, int B, int H, int W, int iterations, float pos_w, float pos_xy_std,
                  float bi_w, float bi_xy_std, float bi_rgb_std, int* labels, int* nseg_last, float* probs, float* debug, void* workspace,
                  size_t workspace_bytes, void* stream);
/* the image STEGO's dense_crf rebuilds from the normalised frame: out u8 [B][out_h][out_w][3] =
 * u8(trunc(255 * ((((x - mean) / std) * std) + mean))) with x the fp32 [0,1] frame (frame_u8: u8 / 255) [B][3][src_h][src_w] sampled
 * through the ingest tables rows [out_h] / cols [out_w] (both NULL: identity, out == src size). */
int wvn_crf_image(const void* frame, int frame_u8, int B, int src_h, int src_w, const int* rows, const int* cols, int out_h, int out_w,
                  unsigned char* out, void* stream);

/* ---- permutohedral-lattice dense CRF (csrc/dense_crf_permutohedral.hip; DESIGN.md "Permutohedral dense CRF") ----
 * The CRF of wvn_dense_crf (same unary, Potts update, symmetric normalisation, softmax, tie rule, arguments and outputs) with both
 * kernel sums computed by the permutohedral-lattice filter pydensecrf's DenseCRF2D runs (Adams et al. 2010): Gaussian features
 * (x / pos_xy_std, y / pos_xy_std), bilateral features (x / bi_xy_std, y / bi_xy_std, r / bi_rgb_std, g / bi_rgb_std, b / bi_rgb_std),
 * splat, blur along the d + 1 axes, slice scaled by 1 / (1 + 2^-d).  debug rows as wvn_dense_crf (the lattice messages and
 * normalisers).  Bitwise reproducible and independent of the batch.  No pos_xy_std limit, but WVN_ERR_ARG when the lattice
 * coordinates the shape and standard deviations allow do not fit 16-bit keys (pydensecrf's) or, packed, 64 bits.  workspace:
 * wvn_dense_crf_permutohedral_workspace_bytes(B, H, W, K1 + K2) bytes (sized by the bound of N (d + 1) lattice points per frame and
 * lattice), 256-byte aligned, no initialisation; the call is stream-ordered with no host synchronisation. */
size_t wvn_dense_crf_permutohedral_workspace_bytes(int B, int H, int W, int K);
int wvn_dense_crf_permutohedral(const float* logits1, int K1, long long s1b, long long s1c, long long s1p, const float* logits2, int K2,
                                long long s2b, long long s2c, long long s2p, const unsigned char* image, int B, int H, int W, int iterations,
                                float pos_w, float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, int* labels, int* nseg_last,
                                float* probs, float* debug, void* workspace, size_t workspace_bytes, void* stream);
/* tests: the lattice of one kernel (bilateral = 0: Gaussian, d = 2, features of xy_std; 1: bilateral, d = 5) for every frame.  With
 * E = H W (d + 1): M int [B]; keys int [B][E][d] (rows 0..M-1: the lattice points' keys, ascending lexicographically); bary fp32 and
 * vert int [B][E] (vertex pixel (d + 1) + r: its weight and its table row 1..M); nbr int [B][d + 1][E][2] (rows 0..M-1: the rows of
 * the blur neighbours n1, n2 along each axis, 0 = absent).  workspace: wvn_dense_crf_permutohedral_workspace_bytes(B, H, W, 1). */
int wvn_debug_permutohedral_lattice(const unsigned char* image, int B, int H, int W, int bilateral, float xy_std, float rgb_std, int* M,
                                    int* keys, float* bary, int* vert, int* nbr, void* workspace, size_t workspace_bytes, void* stream);

/* ---- overlays (csrc/overlay.hip; DESIGN.md section 4 "Overlays"; tests/visu_ref.py is the same statement on the CPU) ----
 * The pictures of visu/visualizer.py of the reference -- plot_image, plot_segmentation, plot_detectron,
 * plot_detectron_classification, plot_traversability_graph_on_seg, plot_list -- as one pass per output pixel, defined bit for bit.
 *
 * Frame -> 8 bits: img [B][3][H][W] fp32 or u8 (img_u8).  unit_range 1: multiplied by 255 (fp32, rounded on its own); 0: taken as
 * is; < 0: per frame, multiplied iff frame_max[b] <= 1 (frame_max from wvn_frame_max; plot_image's `img.max() <= 1`).  Then
 * truncated toward zero; outside [0, 255] clamped, NaN -> 0.  (u8 frames: x * 255 saturates, i.e. non-zero -> 255.)
 * Colour index of pixel p of map m, by `kind`:
 *   WVN_OVERLAY_VALUES    maps[m] fp32 [B][H][W]: (v * 255) truncated, clipped to [0, 255]; a non-finite product gives 0;
 *   WVN_OVERLAY_LABELS    maps[m] ids [B][H][W] (id_bytes 4 or 8, signed), used as they are;
 *   WVN_OVERLAY_SEGMENTS  maps[m] fp32 [B][S] and seg ids [B][H][W] (seg_bytes 4 or 8): s = seg[p], ids in [-S, 0) wrap to s + S,
 *                         index = (maps[m][b][s] * 255) truncated toward zero (not clipped).
 * An index outside [0, N) -- and a segment id outside [-S, S), a non-finite per-segment product -- paints the plain frame pixel.
 * Colour table lut [N][3], N <= WVN_OVERLAY_MAX_COLOURS: u8 (lut_u8), or fp32 converted as (c * 255) -> u8 by the frame's rule.
 * Blend per channel, source colour s over frame byte d with the alpha byte a (`alpha`; 0 where mask [B][H][W] bytes, optional,
 * is non-zero): a == 0: d; else t = s (128 a) + d (128 (255 - a)) + (0x80 << 7), out = ((((t >> 8) + t) >> 8) >> 7) --
 * PIL.Image.alpha_composite over an opaque image.  boundary_seg (optional ids [B][H][W], boundary_bytes 4 or 8) with
 * boundary_alpha > 0: a pixel one of whose in-image 4-neighbours carries another id gets white composited over the result with
 * that alpha by the same formula; boundary_alpha == 0 is the identity (the reference's default) and reads nothing.
 * Output: packed RGB bytes; pixel (y, x) of panel k of frame b at out[b * out_frame_bytes + y * out_row_bytes + 3 * (k * W + x)];
 * out itself may sit at any byte address (a column offset into a wider image).  Panels: `plain` (0 / 1) plain-frame panel first,
 * then one per map, nmaps <= WVN_OVERLAY_MAX_MAPS; the frame is converted once.
 * wvn_overlay: plain == 0 and nmaps == 1.  wvn_overlay_panels: plain == 1, nmaps >= 0 (0: the 8-bit frame alone).  Both are one
 * launch, stream-ordered, no host synchronisation.  WVN_ERR_ARG before anything is launched for a NULL input, B outside
 * [1, 65535], H or W < 1, N outside [1, 1024], more than 4 maps, alpha bytes outside [0, 255], id sizes other than 4 / 8, an
 * unknown kind, or a row pitch smaller than the panels. */
#define WVN_OVERLAY_MAX_COLOURS 1024
#define WVN_OVERLAY_MAX_MAPS 4
#define WVN_OVERLAY_VALUES 0
#define WVN_OVERLAY_LABELS 1
#define WVN_OVERLAY_SEGMENTS 2
typedef struct {
  const void* img;
  const float* frame_max;
  const void* maps[WVN_OVERLAY_MAX_MAPS];
  const void* seg;
  const void* lut;
  const unsigned char* mask;
  const void* boundary_seg;
  unsigned char* out;
  long long out_row_bytes, out_frame_bytes;
  int img_u8, unit_range, B, H, W;
  int kind, nmaps, plain, id_bytes, seg_bytes, boundary_bytes, S, lut_u8, N, alpha, boundary_alpha;
} wvn_overlay_desc;
/* frame_max[b] = max(0, largest of the n values of frame b) as fp32, NaN when the frame holds a NaN (fp32 frames; n = 3 H W).
 * A clear and one launch on the stream. */
int wvn_frame_max(const void* img, int img_u8, int B, long long n, float* frame_max, void* stream);
int wvn_overlay(const wvn_overlay_desc* d, void* stream);
int wvn_overlay_panels(const wvn_overlay_desc* d, void* stream);

/* ---- overlays: vector primitives (csrc/draw.hip; DESIGN.md section 4 "Overlays: vector primitives"; tests/visu_draw_ref.py is
 * the same statement in plain loops, tests/test_visu_draw_host.py holds it to PIL.ImageDraw) ----
 * What plot_traversability_graph, plot_graph_result, plot_optical_flow and plot_sparse_optical_flow of the reference draw with
 * PIL.ImageDraw, painted in place on a canvas of packed RGB bytes: pixel (y, x) of panel k of frame b at
 * canvas[b * frame_bytes + y * row_bytes + 3 * (k * Wp + x)], P panels of width Wp, canvas at any byte address (the layout of
 * wvn_overlay's `out`: a draw can run on an overlay result or on a column slice of a wider image).
 * Primitive i of N: kinds[i], points[i] = {x0, y0, x1, y1} fp32 in PANEL-LOCAL pixel coordinates, colours[i] = {r, g, b} bytes,
 * frame[i] in [0, B), panel[i] in [0, P).  Every coordinate is truncated toward zero as a double, as PIL's (int) cast does.
 *   WVN_DRAW_LINE   ImageDraw.line(width 0 / 1): Bresenham from the first to the second truncated end point, both painted, no swap;
 *                   the major axis is x when |dx| > |dy|; error 2 minor - major, a minor step when it is >= 0.
 *   WVN_DRAW_LINE2  ImageDraw.line(width 2): the polygon (x0, y0 + ey), (x1, y1 + ey), (x1 + ex, y1), (x0 + ex, y0) with
 *                   ex = sign(dy) if 3 dy^2 > dx^2 else 0, ey = sign(dx) if 3 dx^2 > dy^2 else 0, filled by Pillow's scanline rule
 *                   (fp32 edge slopes); zero length: one pixel.
 *   WVN_DRAW_DISC   ImageDraw.ellipse([cx - 5, cy - 5, cx + 5, cy + 5], fill): the centre is (x0, y0), (x1, y1) is not read; the
 *                   corners are computed in double from the fp32 centre and truncated; the box is 9 or 10 wide and high, and pixel
 *                   (u, v) of a box (w, h) is painted iff min(u, w - u) + min(v, h - v) >= 3.
 * A primitive paints only inside its own panel.  A pixel gets the colour of the highest-index primitive that covers it; a pixel no
 * primitive covers is not written.  Defined beyond PIL: a primitive one of whose coordinates is not finite or truncates outside
 * [-32768, 32767] (for a disc: the box corners), of an unknown kind, or with frame / panel outside the canvas is skipped, and
 * *skipped (int, optional) is incremented once for it.
 * One launch, stream-ordered, no host synchronisation, no workspace; N == 0 launches nothing.  WVN_ERR_ARG before anything is
 * launched: a NULL canvas (or list, when N > 0), N outside [0, WVN_DRAW_MAX_PRIMITIVES], B outside [1, 65535], P outside
 * [1, WVN_OVERLAY_MAX_MAPS + 1], H or Wp < 1, a row pitch smaller than the panels, a frame pitch smaller than a frame. */
#define WVN_DRAW_MAX_PRIMITIVES 65536
#define WVN_DRAW_LINE 0
#define WVN_DRAW_LINE2 1
#define WVN_DRAW_DISC 2
typedef struct {
  unsigned char* canvas;
  const int* kinds;
  const float* points;
  const unsigned char* colours;
  const int* frame;
  const int* panel;
  int* skipped;
  long long row_bytes, frame_bytes;
  int B, H, P, Wp, N;
} wvn_draw_desc;
int wvn_draw(const wvn_draw_desc* d, void* stream);

/* ---- evaluation metrics (csrc/metrics.hip; DESIGN.md section 4 "Evaluation metrics"; tests/metrics_ref.py is the definition) ----
 * ROC at T thresholds, binned and exact AUROC, accuracy -- what the reference's MetricLogger takes from torchmetrics -- from integer
 * counts.  PARITY WITH THE torchmetrics PACKAGE IS UNPINNED (the package is absent); the definitions restate its published behaviour.
 *
 * thresholds: fp32 [T], ascending, 2 <= T <= WVN_METRIC_MAX_T -- torch.linspace(0, 1, T) made on the CPU; an input, never recomputed.
 * Bin of a score p: k(p) = #{t : thresholds[t] <= p} in 0..T (fp32 comparisons against the table; -inf -> 0, +inf -> T).
 * Target value: u8 / i32 as they are, fp32 truncated toward zero (`.type(torch.long)`); 1 positive, 0 negative, everything else
 * (NaN, other integers, ignore_index when has_ignore) skipped.
 * A source is WVN_METRIC_DENSE ([B][H][W]) or WVN_METRIC_PER_SEGMENT: element (row(b, s) * stride) of a table, s = seg[b][y][x] (seg_bytes 4: int32 ids, 8: int64 ids),
 * row(b, s) = seg_off[b] + s with seg_off[b + 1] - seg_off[b] segments in frame b (seg_off int64 [B + 1], ragged graphs), or
 * b * S + s with S segments (seg_off NULL).  Where any source of the call is per-segment, a pixel whose id is < 0 or >= the frame's
 * segment count is skipped for every pair.
 * State of pair (i, j) = score i x target j, int64 words at state + (i * n_targets + j) * state_stride, ADDED INTO:
 *   [0, 2 (T + 1))     hist[k][c]: pixels of bin k and class c
 *   + 0..3             cm[c][p > tau] (strict)
 *   + 4, 5, 6          n_nan (NaN score: not binned), n_ignored (target or segment skipped), n_out_of_range (p < 0 or p > 1: binned all the same)
 *   + 7                reserved            (state_stride >= 2 (T + 1) + WVN_METRIC_STATE_TAIL)
 * A skipped pixel is counted once, in n_ignored, whatever its score; sum(hist) + n_nan + n_ignored = pixels.
 * seg_counts (optional, needs seg): int32 [rows][n_targets][2], ADDED INTO: pixels of segment row with target j in class c.
 * wvn_metric_accumulate: one launch, integer atomics only, no host synchronisation; the result depends on neither the launch
 * geometry nor the arrival order.  WVN_ERR_ARG before the launch: B H W outside [1, 2^31), T out of range, a per-segment source
 * without seg, a NULL or misaligned required pointer, counts outside 1..2, B S >= 2^27, seg with seg_bytes other than 4 / 8.
 *
 * wvn_metric_curve: one pair state -> fpr, tpr, thr fp64 [T] in ascending fpr (index i is threshold T - 1 - i):
 * tps[t] = sum_{k > t} hist[k][1], fps likewise, tpr = tps / P (0 where P == 0), fpr = fps / N; scal[0] = the binned AUROC =
 * sum_{i = 1}^{T - 1} ((fpr[i] - fpr[i-1]) * (tpr[i] + tpr[i-1])) * 0.5 added in ascending i (0 when degenerate), scal[1] = the
 * accuracy (cm[1][1] + cm[0][0]) / sum cm (0 when empty); cnt = {P, N, degenerate (P == 0 or N == 0)}.  One launch.
 *
 * wvn_metric_auroc_weighted: E <= 2^24 entries (score fp32, pos, neg int64 >= 0) SORTED by score (either direction); entries of equal
 * score form a group; U2 = sum_groups neg_g (2 pos_before_g + pos_g); scal[0] = double(U2) / double(2 P N) -- for descending scores the
 * AUROC -- 0 when degenerate; cnt = {U2, P, N, degenerate}.  NaN-scored entries count nothing.  One launch, no atomics. */
#define WVN_METRIC_MAX_T 8192
#define WVN_METRIC_STATE_TAIL 8
#define WVN_METRIC_DENSE 0
#define WVN_METRIC_PER_SEGMENT 1
#define WVN_METRIC_U8 0
#define WVN_METRIC_I32 1
#define WVN_METRIC_F32 2
typedef struct {
  const float* score[2];
  const void* target[2];
  const void* seg;
  const long long* seg_off;
  const float* thresholds;
  long long* state;
  int* seg_counts;
  long long score_stride[2], target_stride[2], state_stride;
  float tau;
  int score_kind[2], target_kind[2], target_dtype[2];
  int n_scores, n_targets, B, H, W, S, T, has_ignore, ignore_index, seg_bytes;
} wvn_metric_desc;
int wvn_metric_accumulate(const wvn_metric_desc* d, void* stream);
int wvn_metric_curve(const long long* state, const float* thresholds, int T, double* fpr, double* tpr, double* thr, double* scal,
                     long long* cnt, void* stream);
int wvn_metric_auroc_weighted(const float* score, const long long* pos, const long long* neg, long long E, double* scal,
                              long long* cnt, void* stream);

/* ---- step scheduling (no reference counterpart: the reference runs one frame at a time on one CUDA stream,
 * wild_visual_navigation_ros/scripts/wvn_feature_extractor_node.py:319-363) ----
 * A HIP stream whose kernels may only occupy the compute units named by `mask` (bit i of the `words` 32-bit words = CU i in the
 * driver's numbering, which interleaves the 8 XCDs of an MI355X: bit i lies on XCD i mod 8), so that the persistent backbone
 * kernels and the many small kernels of clustering / pooling / the learner PARTITION the chip instead of sharing every CU
 * (bench.py's two-stream schedule; scripts/ab_cu_mask.py measures the split).  The handle is a hipStream_t: pass it wherever this
 * header takes `void* stream` (PyTorch: torch.cuda.ExternalStream(handle)).  wvn_stream_destroy releases it. */
int wvn_stream_create_cu_mask(void** stream, const unsigned int* mask, int words);
int wvn_stream_destroy(void* stream);

/* ---------------------------------------------------------------------------------------------
 * feature_type "torchvision" (torchvision_interface.py of the reference: resnet18, eval mode, return nodes layer{1,2,3,4}.1.relu_1;
 * feature_extractor.py:314-366: the multi-scale segment pooling), csrc/resnet.hip and csrc/pyramid_pool.hip.  Exact fp32 on the
 * fp32-input MFMA.  tests/resnet_ref.py states network and pooling in float64; PARITY WITH THE torchvision PACKAGE AND WITH A RELEASED
 * CHECKPOINT IS UNPINNED (both are absent).
 *
 * Activations are NHWC fp32 [B][h][w][C].  A convolution is out[b][oy][ox][n] = epilogue(sum_k A[k] Wp[k][n]), k = (ky * ksize + kx) *
 * Cin + cin ascending in ONE fmaf chain from 0 (terms outside the input are 0): the bits of an element depend on neither the batch nor
 * the launch geometry.  epilogue(v) = fmaf(v, scale[n], shift[n]) (+ residual[b][oy][ox][n]) (then v < 0 ? 0 : v when relu): eval-mode
 * BatchNorm folded to scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale, formed by the caller in float64.
 *   wvn_conv2d_pack_floats / wvn_conv2d_pack: w [Cout][Cin][ksize][ksize] -> packed [Kpad][Cout], Kpad = Cin ksize^2 rounded up to 32.
 *   wvn_conv2d_bn_act: in_kind WVN_CONV_IN_NHWC: in is an activation [B][H][W][Cin], Cin % 32 == 0;
 *       WVN_CONV_IN_FRAME_F32 / _U8: in is a frame [B][3][H][W] (fp32 in [0, 1] / uint8 as v / 255), read as (v - mean[c]) / std[c] with
 *       T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]) -- the stem; a uint8 frame gives the bits of its fp32 twin.
 *       Cout % 64 == 0, ksize 1..7 (square), stride 1 or 2, pad 0..3.  residual may be NULL.
 *   wvn_maxpool3x3s2: 3 x 3, stride 2, pad 1 with -inf padding, NHWC [B][H][W][C] -> [B][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C].
 * The whole network: the 20 convolutions in the order
 *   conv1; layer1.0.conv1, layer1.0.conv2, layer1.1.conv1, layer1.1.conv2;
 *   layerL.0.conv1, layerL.0.conv2, layerL.0.downsample.0, layerL.1.conv1, layerL.1.conv2   for L = 2, 3, 4
 * (each with the BatchNorm that follows it).  wvn_resnet18_pack takes three HOST arrays of WVN_RESNET18_NCONV device pointers (weights
 * [Cout][Cin][k][k], scale [Cout], shift [Cout]) and writes one packed image of wvn_resnet18_pack_bytes() bytes.
 * wvn_resnet18_forward: frames [B][3][H][W] (fp32, or uint8 when frames_u8), H and W multiples of 32 -> the four level maps in the
 * workspace, level l = 1..4 (stride 2^(l+1), 32 * 2^l channels, NHWC) at byte offset wvn_resnet18_level_offset(B, H, W, l); the rest
 * of the workspace holds temporaries.  21 launches on the stream, no allocation.
 *
 * wvn_segpool_pyramid: feat [B][S][960] fp32 from the four level maps and seg [B][H][W] int32, columns [0, 64) [64, 192) [192, 448)
 * [448, 960) for levels 1..4.  Per level with stride s (h = H / s, w = W / s): row i = the mean of the level's vectors over the cells
 * (cy, cx) with seg[cy s][cx s] == i (summed in float64 in raster order, rounded once: reproducible bit for bit and independent of the
 * batch; no floating-point atomics).  Where no cell carries id i -- the published code raises there -- the row is the vector of the
 * cell (min(Cy / s, h - 1), min(Cx / s, w - 1)), Cy = floor(sum of the segment's pixel rows / its pixel count), Cx likewise (integers,
 * full resolution), copied bit for bit.  An id below S without a pixel gives NaN in all four blocks; ids outside [0, S) are ignored.
 * scratch: wvn_segpool_pyramid_scratch_bytes(B, S) bytes, cleared by the call.
 *
 * Every function returns WVN_ERR_ARG before any launch for a null pointer or a shape outside the above (the size queries return 0),
 * WVN_ERR_WORKSPACE for a workspace or scratch buffer that is too small.
 * ------------------------------------------------------------------------------------------- */
#define WVN_CONV_IN_NHWC 0
#define WVN_CONV_IN_FRAME_F32 1
#define WVN_CONV_IN_FRAME_U8 2
#define WVN_RESNET18_NCONV 20
#define WVN_SEGPOOL_PYRAMID_MAX_SEGMENTS (1 << 20)
size_t wvn_conv2d_pack_floats(int Cout, int Cin, int ksize);
int wvn_conv2d_pack(const float* w, float* packed, int Cout, int Cin, int ksize, void* stream);
int wvn_conv2d_bn_act(const void* in, int in_kind, const float* packed, const float* scale, const float* shift, const float* residual,
                      int relu, float* out, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, void* stream);
int wvn_maxpool3x3s2(const float* in, float* out, int B, int H, int W, int C, void* stream);
size_t wvn_resnet18_pack_bytes(void);
int wvn_resnet18_pack(const void* const* conv_w, const void* const* scale, const void* const* shift, void* packed, size_t packed_bytes,
                      void* stream);
size_t wvn_resnet18_workspace_bytes(int B, int H, int W);
size_t wvn_resnet18_level_offset(int B, int H, int W, int level);
int wvn_resnet18_forward(const void* packed, const void* frames, int frames_u8, int B, int H, int W, void* workspace,
                         size_t workspace_bytes, void* stream);
size_t wvn_segpool_pyramid_scratch_bytes(int B, int S);
int wvn_segpool_pyramid(const float* feat1, const float* feat2, const float* feat3, const float* feat4, const int* seg, float* feat,
                        void* scratch, size_t scratch_bytes, int B, int H, int W, int S, void* stream);

/* ---------------------------------------------------------------------------------------------
 * JPEG ingest (the CompressedImage branch of the reference's ros_image_to_torch, ros_converter.py:117-121: cv2.imdecode): compressed
 * camera frames -> uint8 [B][3][H][W] in device memory, BIT-IDENTICAL to what libjpeg(-turbo) with default settings decodes from the
 * same bytes (islow IDCT, fancy upsampling, 16-bit colour tables).  tests/jpeg_ref.py states the whole decoder in numpy.
 *
 * Host stage (csrc/jpeg_host.cpp, no HIP): marker parser (SOI, APPn, COM, DQT with 8- and 16-bit tables, SOF0 / SOF1 with 8-bit
 * samples, DHT, DRI, SOS, RSTn, EOI, byte stuffing) and the sequential Huffman decoder.  Accepted: 1 component (any sampling
 * factor), or 3 components YCbCr with luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and chroma 1x1, in ONE interleaved scan.
 * Refused with WVN_JPEG_UNSUPPORTED: progressive, lossless, hierarchical, arithmetic coding, 12-bit samples, 2 or 4 components, any
 * other sampling (4:4:0 and 4:1:1 included), RGB-coded files (Adobe transform 0, or ids 'R' 'G' 'B' without JFIF), several scans,
 * DNL, a side above WVN_JPEG_MAX_DIM.  The input is untrusted: a short stream is WVN_JPEG_TRUNCATED, a wrong marker, length or RSTn
 * WVN_JPEG_BAD_MARKER, a bad DQT / DHT or a missing table WVN_JPEG_BAD_TABLE, a bit pattern that is no code WVN_JPEG_BAD_HUFFMAN, a
 * run past coefficient 63 or a DC value outside int16 WVN_JPEG_BAD_COEFFICIENT.  Nothing is padded or guessed: such a frame has a
 * status and no pixels.  EOI must follow the scan; bytes after it are ignored.  Whole bytes left between the last coded bit and an RSTn
 * or EOI are WVN_JPEG_BAD_MARKER (libjpeg skips such "extraneous bytes"); only the fewer than 8 padding bits are dropped.
 * Precedence: the first error met in stream order decides; WVN_JPEG_OUT_OF_RANGE is given only to a stream that is otherwise whole.
 * wvn_jpeg_info walks the whole header (tables and scan header included).  wvn_jpeg_probe_batch is the cheap form a batch uses to learn
 * its geometries in one call: markers and lengths up to SOS, Huffman codes not built; g [B] and status [B] are host arrays.
 * WVN_JPEG_OUT_OF_RANGE: a block whose dequantised coefficients or first-pass values leave int16, or whose samples before the + 128
 * leave [-512, 511].  There libjpeg has no single answer -- its C code and its SIMD code wrap and saturate differently -- so the
 * frame is refused.  Streams encoded from 8-bit pictures stay inside (the widest sample met in the tests: 338, a saturated checkerboard at quality 1).  The host checks it exactly: blocks
 * with sum |coef q| <= 2000 cannot leave the range, the others run the integer IDCT once on the host.
 *
 * Coefficients: int16 [blocks][64], quantised (NOT dequantised), natural order (index 8 v + u), component after component, each
 * component a raster of bw x bh blocks padded to whole MCUs: with hmax x vmax the luma factors, mcus_x = ceil(width / (8 hmax)),
 * bw = mcus_x h_c, likewise bh.  4:2:0 is 1.5 samples per pixel x 2 B = 3 B per pixel: the upload is the size of the RGB8 frame.
 * wvn_jpeg_coefficients is the host stage alone for one frame: coef (coef_bytes >= wvn_jpeg_coef_bytes(g)) and the quantisation
 * tables of the components, uint16 [3][64] in natural order; both are all zero unless the status is WVN_JPEG_OK.
 * wvn_jpeg_coefficients_batch is the host stage of wvn_jpeg_decode_batch without the device: B frames of geometry g on the same
 * workers into HOST arrays coef [B][blocks][64] (coef_bytes >= B wvn_jpeg_coef_bytes(g)) and qtables [B][3][64], status [B].
 *
 * Device stage (csrc/jpeg.hip), integers only:
 *   1. dequantise (coef * q in 32 bits) + libjpeg's jidctint "islow" 8 x 8 inverse DCT (CONST_BITS 13, PASS1_BITS 2, descale with
 *      round-half-up, + 128, range limit through libjpeg's 10-bit mask) -> component planes uint8 [bh 8][bw 8];
 *   2. fancy upsampling + YCbCr -> RGB per output pixel.  h2v1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2)
 *      >> 2; h2v2: with t[i] = 3 near[i] + far[i] over the nearer and farther chroma row, out[2i] = (3 t[i] + t[i-1] + 8) >> 4,
 *      out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4; at the first and last column of the component's REAL width cw = ceil(width / 2) the
 *      missing neighbour is the sample itself; above the first and below the last real row (ch = ceil(height / 2)) the row itself.
 *      A component of real width <= 2 is replicated (libjpeg switches fancy upsampling off there).  Colour: R = Y + ((91881 (Cr -
 *      128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768) >> 16), G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768)
 *      >> 16), clamped to [0, 255].  One component: the luma plane replicated (or one channel with gray_out).
 *
 * wvn_jpeg_decode_batch: B frames of ONE geometry g (a frame of another geometry: WVN_JPEG_GEOMETRY_MISMATCH) ->
 * out_u8 [B][gray_out ? 1 : 3][height][width].  gray_out needs a one-component geometry.  The host stage runs on
 * min(threads, B, WVN_JPEG_MAX_THREADS) workers (threads < 1 counts as 1) and writes into a pinned staging buffer owned by the
 * library; one asynchronous upload and two launches follow on the stream.  Two staging buffers alternate, each guarded by an event
 * recorded behind its upload, so a call never overwrites bytes a previous call's upload still reads.  status: HOST int [B], valid on
 * return; a frame with a status other than WVN_JPEG_OK is ALL ZERO in out_u8 and does not disturb its neighbours.  workspace: device
 * memory of wvn_jpeg_workspace_bytes(g, B) bytes (per frame 512 B of tables + the coefficients + the planes, 256-byte aligned).
 * wvn_jpeg_device_stage is the second half alone, for coefficients that are already in the workspace (laid out as above: frame b at
 * byte b (512 + wvn_jpeg_coef_bytes(g)): uint16 q[3][64], uint16 valid, padding to 512 B, then the coefficients): the two launches.
 * Returns WVN_ERR_ARG before anything runs for a null pointer, B < 1, B > WVN_JPEG_MAX_BATCH, a geometry wvn_jpeg_info does not
 * produce or gray_out on a colour geometry; per-frame failures are statuses, not a return value.  The size queries return 0 for
 * such a geometry.
 * ------------------------------------------------------------------------------------------- */
#define WVN_JPEG_OK 0
#define WVN_JPEG_TRUNCATED 1
#define WVN_JPEG_BAD_MARKER 2
#define WVN_JPEG_BAD_TABLE 3
#define WVN_JPEG_BAD_HUFFMAN 4
#define WVN_JPEG_BAD_COEFFICIENT 5
#define WVN_JPEG_UNSUPPORTED 6
#define WVN_JPEG_GEOMETRY_MISMATCH 7
#define WVN_JPEG_BAD_GEOMETRY 8
#define WVN_JPEG_OUT_OF_RANGE 9
#define WVN_JPEG_GRAY 0
#define WVN_JPEG_444 1
#define WVN_JPEG_422 2
#define WVN_JPEG_420 3
#define WVN_JPEG_MAX_DIM 16384
#define WVN_JPEG_MAX_THREADS 16
#define WVN_JPEG_MAX_BATCH 4096
typedef struct {
  int width, height, components, sampling, restart_interval;
} wvn_jpeg_geometry;
int wvn_jpeg_info(const void* data, size_t n, wvn_jpeg_geometry* out);
int wvn_jpeg_probe_batch(const void* const* data, const size_t* sizes, int B, wvn_jpeg_geometry* g, int* status);
size_t wvn_jpeg_coef_bytes(const wvn_jpeg_geometry* g);
size_t wvn_jpeg_plane_bytes(const wvn_jpeg_geometry* g);
size_t wvn_jpeg_workspace_bytes(const wvn_jpeg_geometry* g, int B);
int wvn_jpeg_coefficients(const void* data, size_t n, const wvn_jpeg_geometry* g, short* coef, size_t coef_bytes,
                          unsigned short* qtables);
int wvn_jpeg_coefficients_batch(const void* const* data, const size_t* sizes, int B, const wvn_jpeg_geometry* g, short* coef,
                                size_t coef_bytes, unsigned short* qtables, int threads, int* status);
int wvn_jpeg_device_stage(const wvn_jpeg_geometry* g, int B, void* workspace, void* out_u8, int gray_out, void* stream);
int wvn_jpeg_decode_batch(const void* const* data, const size_t* sizes, int B, const wvn_jpeg_geometry* g, void* out_u8, int gray_out,
                          void* workspace, int threads, int* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Raw camera ingest (the sensor_msgs/Image branch of the reference's ros_image_to_torch, ros_converter.py:113-126, and the debayer +
 * undistortion its launch files hand to image_proc_cuda_ros): a frame as the camera driver publishes it -> planar uint8 frames in
 * device memory, at full resolution (wvn_unpack_frames) or rectified through a fixed-point map (wvn_rectify_frames).  Integers only;
 * tests/rectify_ref.py states both in numpy and the result is that statement BIT FOR BIT.  The rules aim at cv2.cvtColor(Bayer),
 * cv2.initUndistortRectifyMap / cv2.fisheye and cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0); that parity is NOT pinned.
 *
 * Source: uint8, B frames `frame_stride` bytes apart, each H rows (WVN_SRC_PLANAR: 3 H rows, plane after plane: what
 * wvn_jpeg_decode_batch writes, step = W) of `step` >= W bytes_per_pixel bytes; the padding of a row is never read.  Kinds:
 * WVN_SRC_MONO8; WVN_SRC_RGB8 / WVN_SRC_BGR8 (packed, 3 bytes per pixel); WVN_SRC_PLANAR (R, G, B planes); the four mosaics, named by
 * their 2 x 2 tile row by row: RGGB = R G / G B, BGGR = B G / G R, GBRG = G B / R G, GRBG = G R / B G.
 *
 * Demosaic (bilinear): at an interior site the site's own colour is the raw byte; at an R or B site G = (N + S + E + W + 2) >> 2 and
 * the opposite colour = (NW + NE + SW + SE + 2) >> 2; at a G site the colour of its horizontal neighbours = (W + E + 1) >> 1, that of
 * its vertical neighbours = (N + S + 1) >> 1.  The one-pixel ring: columns 0 and W - 1 take the result of columns 1 and W - 2, then
 * rows 0 and H - 1 those of rows 1 and H - 2.  H, W >= 3, odd sizes included.
 *
 * Map: two int32 [h][w] planes in device memory, the source coordinates of every output pixel in Q5 (x 32, OpenCV's INTER_BITS),
 * computed by the caller once per camera geometry (ops.rectify_map: float64 on the host).  Sampling: ix = qx >> 5 (arithmetic),
 * ax = qx & 31, likewise y; p00, p01, p10, p11 the source values at (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1), a tap
 * outside the frame 0; out = ((32 - ax)(32 - ay) p00 + ax (32 - ay) p01 + (32 - ax) ay p10 + ax ay p11 + 512) >> 10 per channel.
 * Any int32 is a valid map entry: every tap is bounds-checked.  For a mosaic the source value of a channel is the demosaic above,
 * ring included, so the one launch equals wvn_unpack_frames followed by wvn_rectify_frames on its planar result.
 *
 * Output: out_u8 [B][3][rows][cols] planar, R, G, B with WVN_ORDER_RGB and B, G, R with WVN_ORDER_BGR; a WVN_SRC_MONO8 source gives the
 * plane three times, or [B][1][rows][cols] with WVN_ORDER_GRAY (mono8 only).  One launch on `stream`, no atomics, no host
 * synchronisation, no workspace.  One thread writes four adjacent pixels of a row as one dword per plane; a group cut by the end of
 * the row or not dword aligned is stored byte by byte.
 * WVN_ERR_ARG before any launch: a null pointer, B < 1 or B > 65535, H or W < 3 for a mosaic and < 1 otherwise, h or w < 1, a side above
 * WVN_FRAME_MAX_DIM, step < W bytes_per_pixel, frame_stride smaller than the bytes read of one frame, an unknown kind or order,
 * WVN_ORDER_GRAY on a colour source, and sizes whose byte counts (B frame_stride, the output, one map plane) leave 31 bits.
 * ------------------------------------------------------------------------------------------- */
#define WVN_SRC_MONO8 0
#define WVN_SRC_RGB8 1
#define WVN_SRC_BGR8 2
#define WVN_SRC_PLANAR 3
#define WVN_SRC_BAYER_RGGB8 4
#define WVN_SRC_BAYER_BGGR8 5
#define WVN_SRC_BAYER_GBRG8 6
#define WVN_SRC_BAYER_GRBG8 7
#define WVN_ORDER_RGB 0
#define WVN_ORDER_BGR 1
#define WVN_ORDER_GRAY 2
#define WVN_FRAME_MAX_DIM 65535
int wvn_unpack_frames(const void* src, int kind, int B, int H, int W, long long step, long long frame_stride, void* out_u8, int order,
                      void* stream);
int wvn_rectify_frames(const void* src, int kind, int B, int H, int W, long long step, long long frame_stride, const int* map_qx,
                       const int* map_qy, int h, int w, void* out_u8, int order, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Traversability grid map: what the reference hands to elevation_mapping_cupy (the sem_wvn_*_traversability image subscribers with
 * image_channel_fusions: exponential, anymal_sensor_parameter.yaml / anymal_parameters.yaml) and to smart_carrot.py.  Three launches,
 * each on `stream`, without atomics, workspace or host synchronisation; tests/grid_map_ref.py states them in numpy and the results are
 * that statement BIT FOR BIT (fp32, every operation rounded on its own, in the order csrc/grid_map.hip writes out).  Parity with
 * elevation_mapping_cupy's own kernels and with cv2.circle's rasterisation is NOT pinned: neither package is available.
 *
 * Grid: square, N x N (N <= WVN_GRID_MAX_N), axis 0 = map x, axis 1 = map y, row-major fp32 layers, NaN = unknown; cell (i, j) is
 * centred at (cx + (i - N/2) r, cy + (j - N/2) r)  (smart_carrot.py:145-150).
 *
 * wvn_grid_fuse_images: maps [B][C][H][W] fp32 (C <= 4, B <= WVN_GRID_MAX_CAMERAS), per camera the scaled 4 x 4 intrinsics and
 * pose_cam_in_world (device, [B][4][4]); `layers`: a HOST array of C device pointers, the target layers, updated in place; `hits`
 * int32 [N][N].  One thread owns a cell and applies the cameras in order b = 0 .. B-1: the cell (x, y, elevation) is projected
 * (rigid inverse + pinhole), the camera is skipped unless the depth is > min_depth, the nearest pixel (floor(u + 0.5), floor(v + 0.5))
 * lies inside the image and the horizontal distance to the camera is <= max_range (INFINITY: no limit); the ray to the camera is walked
 * in steps of one resolution in the xy-plane and the cell is hidden when a cell under the ray is finite and higher than the ray by more
 * than occlusion_margin; each channel whose sample is not NaN is fused, new = old is NaN ? value : old (1 - alpha) + alpha value, and
 * hits counts the cameras that fused.  Cells with NaN elevation and cells no camera reaches are not written.
 *
 * wvn_grid_sdf: exact Euclidean signed distance field of the set {layer < threshold}; unknown cells (NaN) count as obstacle, free or
 * neither (WVN_GRID_UNKNOWN_*).  d2 int32 [N][N]: squared distance in cells to the nearest cell of the other set, > 0 free, < 0
 * obstacle, 0 for a cell in neither set, +-INT32_MAX where the other set is empty; sdf fp32 = +-(resolution * sqrtf(float(|d2|))), NaN
 * for a cell in neither set, +-inf where the other set is empty.
 *
 * wvn_grid_carrot: smart_carrot.py:53-94, 126-150.  score = sdf (+ distance force if its factor > 0) (- centre force if its factor > 0);
 * -inf outside the discs, where the 3 x 3 neighbourhood holds a NaN elevation, and where the score is NaN; arg-max, ties to the lowest
 * row-major index.  `discs`: a HOST array of n_discs (distance, radius) pairs in cells (n_discs <= WVN_GRID_MAX_DISCS; the reference's
 * are (30, 15), (55, 20), (90, 25) on its 200-cell map); disc d is (i - ci)^2 + (j - cj)^2 <= radius^2 with ci = int(N/2 + cos_yaw
 * distance), cj = int(N/2 + sin_yaw distance), computed on the host in double; the kernel uses cos_yaw and sin_yaw rounded to fp32.
 * Out (device): goal_cell int32 [3] = {i, j, found}, goal fp32 [3] = {score, x, y} with x = (i - N/2) r + cx; masked [N][N] (may be
 * NULL): the masked score layer.
 *
 * WVN_ERR_ARG before any launch: a null pointer (masked excepted), N < 1 or above WVN_GRID_MAX_N, B, C, H, W, n_discs out of range, a
 * resolution that is not positive and finite, alpha outside [0, 1], a NaN parameter, |cos_yaw| or |sin_yaw| > 1, a negative or
 * oversized disc entry, an unknown `unknown` mode.
 * ------------------------------------------------------------------------------------------- */
#define WVN_GRID_MAX_N 4096
#define WVN_GRID_MAX_CHANNELS 4
#define WVN_GRID_MAX_CAMERAS 64
#define WVN_GRID_MAX_DISCS 8
#define WVN_GRID_MAX_DISC_DISTANCE 1048576
#define WVN_GRID_UNKNOWN_OBSTACLE 0
#define WVN_GRID_UNKNOWN_FREE 1
#define WVN_GRID_UNKNOWN_NEITHER 2
int wvn_grid_fuse_images(const float* maps, int B, int C, int H, int W, const float* intrinsics, const float* poses,
                         const float* elevation, int N, float cx, float cy, float resolution, float* const* layers, int* hits,
                         float alpha, float min_depth, float max_range, float occlusion_margin, void* stream);
int wvn_grid_sdf(const float* layer, int N, float threshold, int unknown, float resolution, int* d2, float* sdf, void* stream);
int wvn_grid_carrot(const float* sdf, const float* elevation, int N, double cos_yaw, double sin_yaw, float distance_force_factor,
                    float center_force_factor, const int* discs, int n_discs, float cx, float cy, float resolution, int* goal_cell,
                    float* goal, float* masked, void* stream);

/* Elevation from depth: the elevation and variance layers from the depth images and point clouds of one callback (the geometric half
 * of elevation_mapping_cupy; csrc/elevation.hip).  accumulate (any number of calls, both forms) then finalise: one launch each, integer
 * atomics only, no host synchronisation; tests/elevation_ref.py states them in numpy and the results are that statement BIT FOR BIT,
 * whatever the order of the points and of the sensors -- every point is judged against the layers as they were on entry.
 *
 * Sources: `points` [B][Pmax][3] fp32 in the sensor frame with `counts` [B] int32 (NULL: every slot is a point), or `depth` [B][H][W],
 * WVN_GRID_DEPTH_F32 metres or WVN_GRID_DEPTH_U16 millimetres (0, NaN, inf: no point), with the scaled 4 x 4 intrinsics as for
 * wvn_grid_fuse_images: pixel (v, u) is ((u - K[0][2]) (z / K[0][0]), (v - K[1][2]) (z / K[1][1]), z), formed on load.  `poses`
 * [B][4][4]: pose_sensor_in_map.  All device pointers.
 *
 * A point is rejected (first match) when a coordinate is not finite, its squared range d2 is below min_valid_distance^2, it is more than
 * max_height_range above its sensor, more than fmaxf(L - ramp_b, 0) ramp_a + ramp_c above it (L: horizontal distance to the sensor), or
 * its nearest cell is outside the map.  It is gated (the cell's outlier count += 1) when the cell's elevation h is finite and
 * |q_z - h| > mahalanobis_thresh sqrtf(variance).  Otherwise it is an inlier of noise v = sensor_noise_factor d2 and enters the cell's
 * integer sums with the weight floor(min(1 / v, 4096 - 1/256) 256) and the height rint((q_z - z_ref) 16384); an inlier with
 * |q_z - z_ref| > 128 or a zero weight is dropped ("unrepresentable").  With at most WVN_GRID_ELEVATION_MAX_POINTS point slots per call
 * (B Pmax, B H W; more is refused) the 64-bit sums cannot overflow; a caller that accumulates several calls before one finalise keeps
 * their total within the same bound.  WVN_GRID_ELEVATION_CLEAR_RAYS: every point that passed rejection walks towards its sensor in
 * steps of one resolution (at most max_ray_length) and a cell under the ray, other than its own, whose elevation is finite and higher
 * than the ray by more than clear_margin is counted as contradicted.
 *
 * finalise, per cell, in fp64: the information-form Kalman update of (elevation, variance) with the cell's sums, variance +=
 * outlier_variance x outliers, clamped to max_variance; with CLEAR_RAYS a cell without an inlier and with at least clear_min_rays
 * contradicting rays becomes unknown: elevation NaN, variance = initial_variance, the C image `layers` (HOST array of device pointers,
 * as for wvn_grid_fuse_images; C may be 0) NaN, hits 0.  `stats` int32 [WVN_GRID_ELEVATION_STATS] (device): the points of the calls
 * since the last finalise by class -- invalid, near, high, ramp, outside, gated, unrepresentable, inliers.
 *
 * `z_ref`: one fp32 ON THE DEVICE, the height the fixed-point sums are relative to (e.g. &poses[11], sensor 0's t_z: nothing is read back
 * to choose it); accumulate and finalise of one callback take the same value.
 * `workspace`: wvn_grid_elevation_workspace_bytes(N) bytes (0 for N out of range), 8-byte aligned (its records take 64-bit atomics),
 * zero before the first call; finalise leaves it zero.
 * WVN_ERR_ARG before any launch: a null pointer (counts excepted), a workspace that is not 8-byte aligned, N, B, H, W, Pmax, C or dtype out of range, more than
 * WVN_GRID_ELEVATION_MAX_POINTS point slots, unknown flags, a resolution or sensor_noise_factor that is not positive and finite, a NaN
 * parameter, a negative min_valid_distance, mahalanobis_thresh, outlier_variance or max_ray_length, max_ray_length / resolution
 * above 2^20, max_variance <= 0, clear_min_rays < 1. */
#define WVN_GRID_ELEVATION_MAX_POINTS 4194304
#define WVN_GRID_ELEVATION_STATS 8
#define WVN_GRID_DEPTH_F32 0
#define WVN_GRID_DEPTH_U16 1
#define WVN_GRID_ELEVATION_CLEAR_RAYS 1
typedef struct {
  float sensor_noise_factor, mahalanobis_thresh, outlier_variance, min_valid_distance, max_height_range;
  float ramp_a, ramp_b, ramp_c;   /* ramped_height_range_a / _b / _c of anymal_parameters.yaml */
  float initial_variance, max_variance, max_ray_length, clear_margin;
  int clear_min_rays;
} wvn_grid_elevation_params;
size_t wvn_grid_elevation_workspace_bytes(int N);
int wvn_grid_elevation_accumulate_points(const float* points, const int* counts, int B, int Pmax, const float* poses,
                                         const float* elevation, const float* variance, int N, float cx, float cy, float resolution,
                                         const wvn_grid_elevation_params* params, const float* z_ref, int flags, void* workspace, void* stream);
int wvn_grid_elevation_accumulate_depth(const void* depth, int dtype, int B, int H, int W, const float* intrinsics, const float* poses,
                                        const float* elevation, const float* variance, int N, float cx, float cy, float resolution,
                                        const wvn_grid_elevation_params* params, const float* z_ref, int flags, void* workspace, void* stream);
int wvn_grid_elevation_finalise(float* elevation, float* variance, float* const* layers, int C, int* hits, int N,
                                const wvn_grid_elevation_params* params, const float* z_ref, int flags, void* workspace, int* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WVN_HIP_H */
