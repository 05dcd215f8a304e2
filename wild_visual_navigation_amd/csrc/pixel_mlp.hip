// Fused per-pixel traversability inference: what the live node runs for every camera frame with
// prediction_per_pixel (wvn_feature_extractor_node.py:319-363, quick_start.py:183-210):
//
//   dense = bilinear_align_corners(tokens [G,G,384] -> [H,W,384])       (dino_interface.py:87-90, 308 MB/frame at 448^2)
//   out   = SimpleMLP(dense rows)   384 -> 256 -> 32 -> 1+384            (simple_mlp.py:10-39, 47.7 GFLOP/frame)
//   trav  = sigmoid(out[:,0]);  conf = confidence(mean((out[:,1:] - dense)^2))   (confidence_generator.py:182-193)
//
// Here the dense tensor is never built and the 384->256 layer never runs per pixel:
//   * layer 1 is linear before its ReLU, and bilinear weights are a convex combination, so
//       W1 * interp(tokens) + b1 == interp(W1 * tokens) + b1:
//     Z = tokens * W1^T is one [G*G,384]x[384,256] GEMM at TOKEN resolution (64x fewer rows), written next to the tokens
//     (row layout  [ Z 256 | x 384 ]  bf16, "zx");
//   * the interpolation itself is an MFMA: a 16x16-pixel tile touches at most 4x4 tokens (checked on the host), so
//       interp^T [channels x pixels] = zx_window^T [channels x 16 tokens] * weights [16 tokens x pixels]
//     is ONE K=16 step of v_mfma_f32_32x32x16_bf16 per 32 channels, with the bilinear weights (4 non-zeros per pixel)
//     built in registers.  Weights are split hi+lo (two MFMAs) so that they carry 16 mantissa bits: the interpolation
//     stays a partition of unity to 2^-17 instead of 2^-9;
//   * everything is kept TRANSPOSED (lane = pixel, registers = channels).  The accumulator layout of one MFMA is then
//     exactly the B-operand layout of the next one up to a fixed permutation of k, which is folded into the packed
//     weight images (wvn_pixel_mlp_pack) -- activations never leave registers, there is no LDS round trip between layers;
//   * the reconstruction error comes out of the MFMA chain directly: acc = b3 + W3 h2 - interp(x) (negated weights), so the
//     epilogue per 32 channels is 16 squares.
//
// One kernel body, pixel_mlp_kernel<EXACT, D>, in two forms that differ in their MFMA operands only (Single / Split, mma()):
//   bf16 form  (EXACT = 0): bf16 operands, fp32 accumulation -- the speed mode.  A product is one MFMA, two where the split bilinear
//     weights are an operand.  Per 32 pixels (one wave): 16 (Z interp) + 16 (layer 2) + NT x 4 (layer 3 + x interp) + 2
//     (traversability row) = 82 MFMAs at D = 384 = 2.7 MFLOP of MFMA work instead of 7.6 MFLOP, and ~20 KB of L2 reads per 256
//     pixels instead of 1.5 KB of HBM per pixel.  The Z GEMM is a bf16 GEMM into columns [0,256) of the caller's zx rows.
//   exact form (EXACT = 1): every operand is split into hi + lo (v = hi + lo to 16 mantissa bits) and every product is formed as
//     hi*hi + hi*lo + lo*hi (three MFMAs, fp32 accumulation): the result matches the fp32 reference sequence to ~1e-5 relative,
//     inside the 1e-3 bar of the exact mode, at 24 + 48 + NT x 9 + 6 = 186 MFMAs per 32 pixels at D = 384.  The Z GEMM runs on the
//     exact fp32 FMA path; pixel_split_rows_kernel writes the hi / lo planes of [ Z | x ] (zx / zxl) into the workspace.
//
// D = 768 (ViT-Base features: DINO ViT-B/8, DINOv2 ViT-B/14): 24 reconstruction tiles, zx rows of 1024 columns, 130 (bf16) / 294
// (exact) MFMAs per 32 pixels.
//   bf16 form : token planes 32,896 + W2 16,384 + W3 (25 tiles) 51,200 + biases 4,352 = 104,832 bytes of LDS: ONE workgroup per CU
//               (Form::WGS_PER_CU sets __launch_bounds__ and the grid cap; 384 and 90 keep two), no scratch.
//   exact form: hi + lo token planes 65,792 + W2 hi/lo 32,768 + W3 hi/lo 102,400 + biases 4,352 = 205,312 > 160 KB.  The W3 lo
//               image (51,200 bytes) stays in the packed blob in global memory (Form::W3L_STREAM); each wave reads its two 1 KB
//               fragments per reconstruction tile with 16-byte global loads, requested one tile (9 MFMAs) ahead.  LDS 154,112 bytes,
//               no scratch, one workgroup per CU.  The blob is the same 50 KB for every wave on the chip (L2-resident), at the
//               price of 50 KB of L2 / L1 reads per wave per 16x16-pixel tile (400 KB per workgroup and tile).
#include <cstdlib>

#include "common.h"
#include "mlp_device.h"
#include "split_operand.h"
#include "wvn_internal.h"

namespace {

constexpr int H1 = 256, H2 = 32;
constexpr int W2_BYTES = 16 * 2 * 32 * 16;          // [16 k-steps][2 lane halves][32 rows][8 bf16] = 16,384
constexpr int TILE = 16;                            // pixels per tile edge; a wave owns 2 rows x 16 columns

// D = MLP input size: 384 (DINO ViT-S features), 768 (DINO ViT-B/8, DINOv2 ViT-B/14) or 90 (STEGO code, the live node's default
// feature_type).  For D = 90 the x part of a zx row is zero-padded to 128 columns (K of the layer-1 GEMM) and three 32-channel
// blocks are interpolated.
constexpr int LDS_PER_CU = 160 * 1024;
template <int D>
struct Cfg {
  static constexpr int DREAL = D;
  static constexpr int NT = (D + 31) / 32;              // 32-channel reconstruction tiles (12 / 24 / 3)
  static constexpr int DX = D == 384 || D == 768 ? D : 128;  // x columns of a zx row
  static constexpr int ZXC = H1 + DX;                   // zx row length the caller provides (640 / 1024 / 384)
  static constexpr int NCH = H1 + 32 * NT;              // channels staged and interpolated per token (640 / 1024 / 352)
  static constexpr int PLANE = NCH * 16 + 64;           // bytes of one 8-token plane [NCH ch][8 tok] (+64: planes 16 banks apart)
  static constexpr int TOK_BYTES = 2 * PLANE;
  static constexpr int W3_TILES = NT + 1;               // + 1 tile whose row 0 is the traversability unit
  static constexpr int W3_BYTES = W3_TILES * 2 * 2 * 32 * 16;
  static constexpr int IMG_BYTES = W2_BYTES + W3_BYTES; // W2 image | W3 image: one part (hi or lo) of the weights
  static constexpr int NBIAS = H1 + H2 + W3_TILES * 32; // b1 | b2 | b3[1:] (padded) | (b3[0], 31 zeros)
  static constexpr int W1_BYTES = H1 * DX * 2;          // the bf16 blob starts with W1 as bf16 [256][DX] (the Z GEMM's weight)
  static constexpr int NFETCH = 16 * (NCH / 8);          // 16-byte chunks of one part of a token window
};
// What depends on the form.  NPART parts (hi, or hi + lo) of the tokens and of the weights.  Packed image ("wimg"; the bf16 blob
// holds it behind W1):  W2 hi | W3 hi | (W2 lo | W3 lo |) biases.  LDS: token parts, then the image -- without its W3 lo part
// where hi + lo exceed the CU's LDS (exact D = 768: 205,312 bytes); that part stays in global memory and is streamed from L2.
template <bool EXACT, int D>
struct Form : Cfg<D> {
  using K = Cfg<D>;
  static constexpr int NPART = EXACT ? 2 : 1;
  static constexpr int WIMG_BYTES = NPART * K::IMG_BYTES + K::NBIAS * 4;
  static constexpr int OFF_W = NPART * K::TOK_BYTES;     // W2 hi; W3 hi at + W2_BYTES; the lo part of either at + IMG_BYTES
  static constexpr bool W3L_STREAM = OFF_W + WIMG_BYTES > LDS_PER_CU;
  static constexpr int OFF_BIAS = OFF_W + NPART * K::IMG_BYTES - (W3L_STREAM ? K::W3_BYTES : 0);
  static constexpr int LDS_BYTES = OFF_BIAS + K::NBIAS * 4;  // bf16 66,432 / 104,832 at D = 384 / 768; exact 130,048 / 154,112
  // occupancy bound and grid cap: two workgroups per CU where the bf16 form fits twice (D = 384, 90)
  static constexpr int WGS_PER_CU = !EXACT && 2 * LDS_BYTES <= LDS_PER_CU ? 2 : 1;
  static constexpr int NPRE = (NPART * K::NFETCH + 511) / 512;
};

struct PixParams {
  const bf16_t* zx; const bf16_t* zxl; int ldzx;   // [B*G*G][ldzx]: columns [0,256) = Z, [256, NCH) = tokens; zxl = lo parts (exact) or nullptr
  const unsigned char* wimg;        // Form::WIMG_BYTES
  float* trav; float* conf; float* loss;
  int B, G, Ho, Wo, nty, ntx;
  float sy, sx;                     // (G-1)/(Ho-1), (G-1)/(Wo-1)
  float mean, std, std_factor;
  const float* conf_dev;            // optional {mean, std, std_factor} in device memory (overrides the three scalars)
};

// ---- MFMA operands (Single / Split, mma, relu_frag, bias16): split_operand.h

// tile index -> frame, tile row / column, and the top-left token (by, bx) of its 4x4 token window
struct TileAt { int b, tyi, txi, by, bx; };
__device__ inline TileAt tile_at(const PixParams& p, int tile) {
  const int tiles_per_frame = p.nty * p.ntx;
  TileAt t;
  t.b = tile / tiles_per_frame;
  const int r = tile - t.b * tiles_per_frame;
  t.tyi = r / p.ntx; t.txi = r - t.tyi * p.ntx;
  t.by = (int)(p.sy * (float)(t.tyi * TILE)); t.bx = (int)(p.sx * (float)(t.txi * TILE));
  return t;
}

// ---- token staging.  A window is NPART parts x [16 tokens][NCH / 8 chunks of 16 B]; thread tid owns chunks tid, tid + 512, ...
// (slots past the end stay idle).  fetch: global -> registers; stash: registers -> the LDS planes [part][tok >> 3][NCH ch][8 tok].
template <class F>
__device__ inline void fetch_tokens(const PixParams& p, int tile, int tid, u32x4_t (&pre)[F::NPRE]) {
  const TileAt t = tile_at(p, tile);
#pragma unroll
  for (int k = 0; k < F::NPRE; ++k) {
    const int idx = tid + 512 * k;
    if (idx < F::NPART * F::NFETCH) {
      const int part = F::NPART == 2 && idx >= F::NFETCH, id = idx - part * F::NFETCH;
      const int tok = id & 15, chunk = id >> 4;
      const int gy = min(t.by + (tok >> 2), p.G - 1), gx = min(t.bx + (tok & 3), p.G - 1);
      const bf16_t* src = part ? p.zxl : p.zx;
      pre[k] = *(const u32x4_t*)(src + ((size_t)t.b * p.G * p.G + (size_t)gy * p.G + gx) * p.ldzx + chunk * 8);
    }
  }
}
template <class F>
__device__ inline void stash_tokens(unsigned char* smem, int tid, const u32x4_t (&pre)[F::NPRE]) {
#pragma unroll
  for (int k = 0; k < F::NPRE; ++k) {
    const int idx = tid + 512 * k;
    if (idx < F::NPART * F::NFETCH) {
      const int part = F::NPART == 2 && idx >= F::NFETCH, id = idx - part * F::NFETCH;
      const int tok = id & 15, chunk = id >> 4;
      unsigned char* dst = smem + part * F::TOK_BYTES + (tok >> 3) * F::PLANE + chunk * 128 + (tok & 7) * 2;
#pragma unroll
      for (int e = 0; e < 8; ++e) *(bf16_t*)(dst + e * 16) = (bf16_t)(pre[k][e >> 1] >> ((e & 1) * 16));
    }
  }
}

// B fragments of the interpolation for pixel (py, px), lane half h: k slot 8h + e = token (row 2h + (e >> 2), column e & 3) of the
// tile's 4x4 window.  w: the bilinear weights; neg: their negation (the reconstruction error subtracts interp(x)).
struct Bilinear { Split w, neg; };
__device__ inline Bilinear bilinear_frags(const PixParams& p, const TileAt& t, int py, int px, int h) {
  // every operation here is rounded as written (the one fma below is written out): what the weights are must not depend on which
  // multiply-add pairs the compiler happens to contract
#pragma clang fp contract(off)
  // ATen's align_corners bilinear: src = dst * (G-1)/(H-1), i0 = (int)src, w1 = src - i0, w0 = 1 - w1
  const float fsy = p.sy * (float)min(py, p.Ho - 1), fsx = p.sx * (float)min(px, p.Wo - 1);
  const int gy0 = (int)fsy, gx0 = (int)fsx;
  const float wy1 = fsy - (float)gy0, wx1 = fsx - (float)gx0;
  const int ty0 = gy0 - t.by, tx0 = gx0 - t.bx;
  float wyv[2], wxv[4];
#pragma unroll
  for (int q = 0; q < 2; ++q) wyv[q] = ((2 * h + q) == ty0 ? 1.f - wy1 : 0.f) + ((2 * h + q) == ty0 + 1 ? wy1 : 0.f);
#pragma unroll
  for (int q = 0; q < 4; ++q) wxv[q] = (q == tx0 ? 1.f - wx1 : 0.f) + (q == tx0 + 1 ? wx1 : 0.f);
  u32x4_t whi, wlo;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float wy = wyv[q >> 1], wxa = wxv[(2 * q) & 3], wxb = wxv[(2 * q + 1) & 3];
    whi[q] = pack_bf16x2(wy * wxa, wy * wxb);
    // lo = the product before its rounding - hi
    wlo[q] = pack_bf16x2(fmaf(wy, wxa, -__uint_as_float(whi[q] << 16)), fmaf(wy, wxb, -__uint_as_float(whi[q] & 0xffff0000u)));
  }
  return {Split::from(whi, wlo), Split::from(whi ^ 0x80008000u, wlo ^ 0x80008000u)};
}

// The A fragments of layers 2 and 3 of this lane (lw = its offset inside one 1 KB [k-step] block): W2 k-step s, and the two k-steps
// of W3 tile t.  The parts come from LDS, except the W3 lo part where it is streamed (W3L_STREAM): from the packed image in global
// memory -- the same 50 KB for every wave of every workgroup, L2-resident -- with tile t + 1's pair requested before tile t's is
// handed out, so that the loads fly during tile t's MFMAs.  Call w3 with t = 0, 1, ..., NT in order.
template <class F>
struct WeightImages {
  using Op = typename OperandOf<F::NPART == 2>::type;
  const unsigned char* lds;    // W2 hi image in LDS + lw
  const unsigned char* w3lo;   // W3 lo image in global memory + lw
  bf16x8_t ahead[2];
  __device__ WeightImages(const unsigned char* smem, const unsigned char* wimg, unsigned lw)
      : lds(smem + F::OFF_W + lw), w3lo(wimg + F::IMG_BYTES + W2_BYTES + lw) {}
  __device__ Op w2(int s) const { return Op::load(lds + s * 1024, F::IMG_BYTES); }
  __device__ void w3(int t, Op (&w)[2]) {
    const unsigned char* hi = lds + W2_BYTES + 2 * t * 1024;
    if constexpr (F::W3L_STREAM) {
#pragma unroll
      for (int u = 0; u < 2; ++u) w[u] = Op{frag_at(hi + u * 1024), t == 0 ? frag_at(w3lo + u * 1024) : ahead[u]};
      if (t < F::NT) {   // (t + 1 == NT: the traversability tile)
#pragma unroll
        for (int u = 0; u < 2; ++u) ahead[u] = frag_at(w3lo + (2 * t + 2 + u) * 1024);
      }
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u) w[u] = Op::load(hi + u * 1024, F::IMG_BYTES);
    }
  }
};

__device__ inline void write_pixel(const PixParams& p, size_t o, float logit, float lr) {
  if (p.trav) p.trav[o] = sigmoid_f(logit);
  if (p.loss) p.loss[o] = lr;
  if (p.conf) {
    const float cm = p.conf_dev ? p.conf_dev[0] : p.mean, cs = p.conf_dev ? p.conf_dev[1] : p.std;
    const float cf = p.conf_dev ? p.conf_dev[2] : p.std_factor;
    p.conf[o] = confidence_of_nan(lr, cm, cs, cf);
  }
}

template <bool EXACT, int D>
__global__ __launch_bounds__(512, (Form<EXACT, D>::WGS_PER_CU)) void pixel_mlp_kernel(PixParams p) {
  using F = Form<EXACT, D>;
  using Op = typename OperandOf<EXACT>::type;   // tokens, weights and activations; the bilinear weights are Split in both forms
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 31, h = lane >> 5;
  const int ntiles = p.B * p.nty * p.ntx;

  // resident weight image: all of it, or what lies before the W3 lo part and the biases from behind it
  constexpr int NRES = F::W3L_STREAM ? F::OFF_BIAS - F::OFF_W : F::WIMG_BYTES;
  for (int i = tid; i < NRES / 16; i += 512) *(u32x4_t*)(smem + F::OFF_W + i * 16) = ((const u32x4_t*)p.wimg)[i];
  if constexpr (F::W3L_STREAM)
    for (int i = tid; i < F::NBIAS * 4 / 16; i += 512)
      *(u32x4_t*)(smem + F::OFF_BIAS + i * 16) = ((const u32x4_t*)(p.wimg + F::WIMG_BYTES - F::NBIAS * 4))[i];
  const float* bias_l = (const float*)(smem + F::OFF_BIAS);

  u32x4_t pre[F::NPRE];
  int tile = blockIdx.x;
  if (tile < ntiles) fetch_tokens<F>(p, tile, tid, pre);
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    stash_tokens<F>(smem, tid, pre);
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) fetch_tokens<F>(p, tile + gridDim.x, tid, pre);

    const TileAt ta = tile_at(p, tile);
    const int py = ta.tyi * TILE + 2 * wave + (n >> 4), px = ta.txi * TILE + (n & 15);
    const Bilinear bil = bilinear_frags(p, ta, py, px, h);
    const unsigned char* tokl = smem + h * F::PLANE + n * 16;         // + 512 per 32-channel block
    auto tok = [&](int blk) { return Op::load(tokl + blk * 512, F::TOK_BYTES); };
    WeightImages<F> wts(smem, p.wimg, (h * 32 + n) * 16);

    // ---- layers 1 + 2: h1 block = relu(b1 + interp(Z block)); a2 += W2[:, block] * h1 block
    f32x16_t a2 = bias16(bias_l + H1, h);
#pragma unroll
    for (int blk = 0; blk < H1 / 32; ++blk) {
      f32x16_t az = bias16(bias_l + 32 * blk, h);
      mma(az, tok(blk), bil.w);
      const Op h1v[2] = {relu_frag<Op>(az, 0), relu_frag<Op>(az, 8)};
#pragma unroll
      for (int u = 0; u < 2; ++u) mma(a2, wts.w2(2 * blk + u), h1v[u]);
    }
    const Op h2v[2] = {relu_frag<Op>(a2, 0), relu_frag<Op>(a2, 8)};

    // ---- layer 3 + reconstruction error, 32 channels at a time: a3 = b3 + W3 h2 - interp(x); tile NT: the traversability row
    float lsum = 0.f;
    Op w3[2];
#pragma unroll
    for (int t = 0; t < F::NT; ++t) {
      f32x16_t a3 = bias16(bias_l + H1 + H2 + 32 * t, h);
      wts.w3(t, w3);
#pragma unroll
      for (int u = 0; u < 2; ++u) mma(a3, w3[u], h2v[u]);
      mma(a3, tok(H1 / 32 + t), bil.neg);
#pragma unroll
      for (int q = 0; q < 16; ++q) lsum = fmaf(a3[q], a3[q], lsum);
    }
    f32x16_t at = bias16(bias_l + H1 + H2 + 32 * F::NT, h);
    wts.w3(F::NT, w3);
#pragma unroll
    for (int u = 0; u < 2; ++u) mma(at, w3[u], h2v[u]);

    lsum += __shfl_xor(lsum, 32, 64);
    if (h == 0 && py < p.Ho && px < p.Wo)   // (padded channels contribute exact zeros to lsum)
      write_pixel(p, ((size_t)ta.b * p.Ho + py) * p.Wo + px, at[0], lsum / (float)F::DREAL);
    __syncthreads();  // every wave is done with this tile's token image
  }
}

// ---- packing.  k permutations (see the file header): the B fragment of k-step u built from an accumulator holds, in slot (h, e),
// row   16u + 8(e >> 2) + 4h + (e & 3)   of the 32-row block the accumulator covers.
// element i of the W2 image [s][h][m][e] -> its index in W2 [32][256]
__device__ inline int w2_source(int i) {
  const int e = i & 7, m = (i >> 3) & 31, hh = (i >> 8) & 1, s = i >> 9;
  return m * H1 + 32 * (s >> 1) + 16 * (s & 1) + 8 * (e >> 2) + 4 * hh + (e & 3);
}
// element i of the W3 image [t][u][h][m][e] -> its index in W3 [1 + D][32], or -1 for a zero (rows past D; the last tile holds row 0 only)
template <int D>
__device__ inline int w3_source(int i) {
  const int e = i & 7, m = (i >> 3) & 31, hh = (i >> 8) & 1, u = (i >> 9) & 1, t = i >> 10;
  const int row = t < Cfg<D>::NT ? (32 * t + m < D ? 1 + 32 * t + m : -1) : (m == 0 ? 0 : -1);
  return row < 0 ? -1 : row * H2 + 16 * u + 8 * (e >> 2) + 4 * hh + (e & 3);
}
// entry i of the bias table: b1 | b2 | b3[1:] (zero-padded to 32 NT) | (b3[0], 31 zeros)
template <int D>
__device__ inline float bias_entry(const float* b1, const float* b2, const float* b3, int i) {
  constexpr int NT = Cfg<D>::NT;
  if (i < H1) return b1[i];
  if (i < H1 + H2) return b2[i - H1];
  if (i < H1 + H2 + 32 * NT) return (i - H1 - H2 < D) ? b3[1 + i - H1 - H2] : 0.f;
  return (i == H1 + H2 + 32 * NT) ? b3[0] : 0.f;
}

// fp32 flat parameters [W1 | b1 | W2 | b2 | W3 | b3] (Linear layout) -> packed blob: Form's weight image, in the bf16 form behind
// W1 as bf16 [256][DX] (zero beyond column D)
template <bool EXACT, int D>
__global__ void pixel_mlp_pack_kernel(const float* __restrict__ prm, unsigned char* __restrict__ out) {
  using F = Form<EXACT, D>;
  const float* W1 = prm;
  const float* b1 = W1 + H1 * D;
  const float* W2 = b1 + H1;
  const float* b2 = W2 + H2 * H1;
  const float* W3 = b2 + H2;
  const float* b3 = W3 + (1 + D) * H2;
  const int gsz = gridDim.x * blockDim.x, g0 = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (!EXACT) {
    bf16_t* w1o = (bf16_t*)out;
    for (int i = g0; i < H1 * F::DX; i += gsz) {
      const int r = i / F::DX, c = i - r * F::DX;
      w1o[i] = c < D ? f32_to_bf16(W1[r * D + c]) : (bf16_t)0;
    }
    out += F::W1_BYTES;
  }
  bf16_t* img = (bf16_t*)out;
  for (int i = g0; i < F::IMG_BYTES / 2; i += gsz) {
    const int s3 = i < W2_BYTES / 2 ? -1 : w3_source<D>(i - W2_BYTES / 2);
    const float v = i < W2_BYTES / 2 ? W2[w2_source(i)] : (s3 < 0 ? 0.f : W3[s3]);
    const bf16_t hi = f32_to_bf16(v);
    img[i] = hi;
    if (EXACT) img[F::IMG_BYTES / 2 + i] = f32_to_bf16(v - bf16_to_f32(hi));
  }
  float* bo = (float*)(out + F::NPART * F::IMG_BYTES);
  for (int i = g0; i < F::NBIAS; i += gsz) bo[i] = bias_entry<D>(b1, b2, b3, i);
}

// zf [rows][256] fp32 (layer-1 pre-activations) and tokens [rows][ldt] fp32 -> hi / lo rows [ Z | x ] of NCH bf16
template <int D>
__global__ void pixel_split_rows_kernel(const float* __restrict__ zf, const float* __restrict__ tok, int ldt,
                                        bf16_t* __restrict__ zxh, bf16_t* __restrict__ zxl, long long rows) {
  using K = Cfg<D>;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * K::NCH) return;
  const long long r = i / K::NCH;
  const int c = (int)(i - r * K::NCH);
  const float v = c < H1 ? zf[r * H1 + c] : (c - H1 < D ? tok[r * ldt + (c - H1)] : 0.f);
  const bf16_t hi = f32_to_bf16(v);
  zxh[i] = hi;
  zxl[i] = f32_to_bf16(v - bf16_to_f32(hi));
}

// ---- host side
template <int D> struct Dim { static constexpr int value = D; };
// f(Dim<D>{}) for a supported D; a zero of f's result type for anything else
template <class Fn>
auto dispatch_D(int D, Fn f) -> decltype(f(Dim<384>{})) {
  return D == 384 ? f(Dim<384>{}) : D == 768 ? f(Dim<768>{}) : D == 90 ? f(Dim<90>{}) : decltype(f(Dim<384>{})){};
}
bool pix_supported(int D, int h1, int h2) { return (D == 384 || D == 768 || D == 90) && h1 == H1 && h2 == H2; }

// what the caller asks for (the entry points' common arguments)
PixParams pix_request(int B, int G, int out_h, int out_w, float mean, float std, float std_factor, const float* conf_state,
                      float* trav, float* conf, float* loss) {
  PixParams p{};
  p.trav = trav; p.conf = conf; p.loss = loss;
  p.B = B; p.G = G; p.Ho = out_h; p.Wo = out_w;
  p.mean = mean; p.std = std; p.std_factor = std_factor; p.conf_dev = conf_state;
  return p;
}
// scales and tile counts; a 16-pixel span must stay inside 3 consecutive source cells (4 tokens): 15 * scale < 2
int pix_window(PixParams& p) {
  p.sy = (float)(p.G - 1) / (float)(p.Ho - 1); p.sx = (float)(p.G - 1) / (float)(p.Wo - 1);
  if (15.f * p.sy > 1.99f || 15.f * p.sx > 1.99f) return WVN_ERR_ARG;
  p.nty = ceil_div(p.Ho, TILE); p.ntx = ceil_div(p.Wo, TILE);
  return WVN_OK;
}
// p complete: persistent workgroups, WGS_PER_CU per CU at most
template <bool EXACT, int D>
int pix_launch(const PixParams& p, hipStream_t st) {
  using F = Form<EXACT, D>;
  auto kern = pixel_mlp_kernel<EXACT, D>;
  static LdsOptIn lds_opt_in;   // per device (common.h)
  if (const int rc = lds_opt_in(F::LDS_BYTES, (const void*)kern)) return rc;
  const int ntiles = p.B * p.nty * p.ntx;
  const int cap = F::WGS_PER_CU * wvn_num_cus();
  hipLaunchKernelGGL(kern, dim3(ntiles < cap ? ntiles : cap), dim3(512), F::LDS_BYTES, st, p);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

template <int D>
int pix_infer(const void* packed, void* zx, int ldzx, PixParams p, hipStream_t st) {
  using K = Cfg<D>;
  if (ldzx < K::ZXC || (ldzx % 8) || ((uintptr_t)zx & 15) || ((uintptr_t)packed & 15)) return WVN_ERR_ARG;
  if (const int rc = pix_window(p)) return rc;
  // Z = x * W1^T, bf16, into columns [0,256) of the same rows (K = the zero-padded x width)
  GemmBf16Params g{};
  g.A = (const bf16_t*)zx + H1; g.lda = ldzx;
  g.W = (const bf16_t*)packed; g.ldw = K::DX;
  g.bias = nullptr;
  g.C = zx; g.ldc = ldzx;
  g.M = p.B * p.G * p.G; g.N = H1; g.K = K::DX;
  if (const int rc = wvn_gemm_bf16_launch(g, EPI_BF16, st)) return rc;
  p.zx = (const bf16_t*)zx; p.ldzx = ldzx;
  p.wimg = (const unsigned char*)packed + K::W1_BYTES;
  return pix_launch<false, D>(p, st);
}

template <int D>
size_t pix_exact_ws(int B, int G) {
  const size_t rows = (size_t)B * G * G;
  return rows * H1 * 4 + 2 * rows * Cfg<D>::NCH * 2 + 256;
}

template <int D>
int pix_infer_exact(const float* params, const void* packed, const float* tokens, int ldt, void* workspace, size_t workspace_bytes,
                    PixParams p, hipStream_t st) {
  using K = Cfg<D>;
  if (ldt < D || ((uintptr_t)workspace & 15) || ((uintptr_t)packed & 15)) return WVN_ERR_ARG;
  if (workspace_bytes < pix_exact_ws<D>(p.B, p.G)) return WVN_ERR_WORKSPACE;
  if (const int rc = pix_window(p)) return rc;
  const long long rows = (long long)p.B * p.G * p.G;
  float* zf = (float*)workspace;
  bf16_t* zxh = (bf16_t*)(zf + rows * H1);
  bf16_t* zxl = zxh + rows * K::NCH;
  // layer 1 at token resolution on the exact fp32 path: Z = x * W1^T (bias is added after the interpolation)
  GemmF32Params g{};
  g.A = tokens; g.lda = ldt; g.transA = 0;
  g.B = params; g.ldb = D; g.transB = 1;   // W1 [256][D], Linear layout, first in the flat parameter buffer
  g.bias = nullptr;
  g.C = zf; g.ldc = H1; g.M = (int)rows; g.N = H1; g.K = D; g.batch = 1; g.splitk = 1;
  if (const int rc = wvn_gemm_f32_launch(g, F32_EPI_NONE, st)) return rc;
  const long long nel = rows * K::NCH;
  hipLaunchKernelGGL(pixel_split_rows_kernel<D>, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st, zf, tokens, ldt, zxh, zxl, rows);
  WVN_LAUNCH_CHECK();
  p.zx = zxh; p.zxl = zxl; p.ldzx = K::NCH;
  p.wimg = (const unsigned char*)packed;
  return pix_launch<true, D>(p, st);
}

template <bool EXACT>
int pix_pack(int D, int h1, int h2, const float* params, void* packed, hipStream_t st) {
  if (!pix_supported(D, h1, h2) || !params || !packed || ((uintptr_t)packed & 15)) return WVN_ERR_ARG;
  dispatch_D(D, [&](auto d) {
    hipLaunchKernelGGL((pixel_mlp_pack_kernel<EXACT, decltype(d)::value>), dim3(96), dim3(256), 0, st, params, (unsigned char*)packed);
    return 0;
  });
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // namespace

// D = 384 (DINO ViT-S features), 768 (ViT-B features) or 90 (STEGO code); 0 / WVN_ERR_ARG for anything else
size_t wvn_pixel_mlp_pack_bytes_impl(int D) {
  return dispatch_D(D, [](auto d) { using F = Form<false, decltype(d)::value>; return (size_t)F::W1_BYTES + F::WIMG_BYTES; });
}
int wvn_pixel_mlp_zx_cols_impl(int D) { return dispatch_D(D, [](auto d) { return (int)Cfg<decltype(d)::value>::ZXC; }); }
size_t wvn_pixel_mlp_exact_pack_bytes_impl(int D) {
  return dispatch_D(D, [](auto d) { return (size_t)Form<true, decltype(d)::value>::WIMG_BYTES; });
}
size_t wvn_pixel_mlp_exact_workspace_bytes_impl(int D, int B, int G) {
  return dispatch_D(D, [&](auto d) { return pix_exact_ws<decltype(d)::value>(B, G); });
}

int wvn_pixel_mlp_pack_launch(int D, int h1, int h2, const float* params, void* packed, hipStream_t st) {
  return pix_pack<false>(D, h1, h2, params, packed, st);
}
int wvn_pixel_mlp_exact_pack_launch(int D, int h1, int h2, const float* params, void* packed, hipStream_t st) {
  return pix_pack<true>(D, h1, h2, params, packed, st);
}

int wvn_pixel_mlp_infer_launch(int D, int h1, int h2, const void* packed, void* zx, int ldzx, int B, int G, int out_h,
                               int out_w, float mean, float std, float std_factor, const float* conf_state, float* trav,
                               float* conf, float* loss, hipStream_t st) {
  if (!pix_supported(D, h1, h2) || !packed || !zx || B <= 0 || G < 2 || out_h < 2 || out_w < 2) return WVN_ERR_ARG;
  const PixParams p = pix_request(B, G, out_h, out_w, mean, std, std_factor, conf_state, trav, conf, loss);
  return dispatch_D(D, [&](auto d) { return pix_infer<decltype(d)::value>(packed, zx, ldzx, p, st); });
}

int wvn_pixel_mlp_infer_exact_launch(int D, int h1, int h2, const float* params, const void* packed, const float* tokens,
                                     int ldt, int B, int G, int out_h, int out_w, float mean, float std, float std_factor,
                                     const float* conf_state, float* trav, float* conf, float* loss, void* workspace,
                                     size_t workspace_bytes, hipStream_t st) {
  if (!pix_supported(D, h1, h2) || !params || !packed || !tokens || !workspace || B <= 0 || G < 2 || out_h < 2 || out_w < 2)
    return WVN_ERR_ARG;
  const PixParams p = pix_request(B, G, out_h, out_w, mean, std, std_factor, conf_state, trav, conf, loss);
  return dispatch_D(D, [&](auto d) { return pix_infer_exact<decltype(d)::value>(params, packed, tokens, ldt, workspace, workspace_bytes, p, st); });
}
