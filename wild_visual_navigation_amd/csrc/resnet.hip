// feature_type "torchvision" of the feature extractor (torchvision_interface.py of the reference: resnet18 in eval mode, return nodes
// layer{1,2,3,4}.1.relu_1) in exact fp32: every convolution is an implicit GEMM on the fp32-input MFMA of gfx950
// (__builtin_amdgcn_mfma_f32_32x32x2f32: bit for bit a k-ordered fmaf chain), with eval-mode BatchNorm, the residual add and the ReLU in
// its epilogue.  tests/resnet_ref.py states the network in float64.
//
// Layout.  Activations are NHWC fp32 ([B][h][w][C]): the GEMM's K index (ky, kx, cin) is then contiguous in cin, and an output tile's
// stores are runs of 128 bytes along Cout.  Weights are packed once to Wp [Kpad][Cout], k = (ky * KW + kx) * Cin + cin, Kpad = K rounded
// up to 32 with zero rows.  The stem reads the frame itself ([B][3][H][W], fp32 in [0, 1] or uint8 as v / 255) and applies
// (v - mean[c]) / std[c] on load; the zero padding of the convolution is applied after it, as T.Normalize followed by conv2d does.
//
// Tile.  One workgroup of four waves computes 64 output pixels x 64 output channels; a wave owns one 32 x 32 accumulator tile.  Cout of
// every ResNet-18 layer is a multiple of 64 and the first stage has exactly 64, so a wider N tile would idle there, while M = B h w
// supplies the parallelism (12544 rows per 448^2 frame in stage 1).  K advances in chunks of 32 through LDS, both operands k-major
// ([k][64 + 4]): lane l of the MFMA reads A[k = l >> 5][m = l & 31] and B[k = l >> 5][n = l & 31], 32 consecutive floats per half wave.
// The next chunk's global loads are issued before the 16 MFMAs of the current one.  (The same tile as 2 x 2 accumulators of the 16x16x4
// form -- a shorter dependent chain per k -- was measured and is slower: 1.10 against 0.96 ms for a 448^2 frame, 3.01 against 2.89 ms
// at B = 16; it needs twice the LDS operand reads per FLOP.  Two LDS buffers with one barrier per chunk were measured too: 1.04 and
// 3.21 ms.  profiles/resnet_pyramid.md.)  Every output element is ONE accumulator chain over
// k = 0 .. Kpad - 1 in ascending order, whatever the tile it falls into: its bits depend on neither the batch nor the launch geometry.
//
// Epilogue: v = fmaf(acc, scale[c], shift[c]); v += residual (optional); v = v < 0 ? 0 : v (optional).  scale / shift are the folded
// BatchNorm terms, formed on the host in float64 (ops.bn_scale_shift).
#include "../../include/wvn_hip.h"

#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 64, BN = 64, BK = 32;
constexpr int LD = BM + 4;   // LDS row stride (floats): 16-byte aligned rows, the four k rows a lane quad writes fall into distinct banks
constexpr int NCONV = WVN_RESNET18_NCONV;

struct ConvArgs {
  const void* in;
  const float* w;
  const float* scale;
  const float* shift;
  const float* resid;
  float* out;
  int B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, K, Kpad, relu, M;
};

__device__ inline float frame_value(const void* in, int kind, size_t i, int c) {
  // T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]); uint8 frames are v / 255 first: the same bits as the fp32 twin
  const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
  const float sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
  const float v = kind == WVN_CONV_IN_FRAME_U8 ? (float)((const unsigned char*)in)[i] / 255.f : ((const float*)in)[i];
  return (v - mean) / sd;
}

// grid (ceil(M / 64), Cout / 64), 256 threads
template <int KIND>
__global__ __launch_bounds__(256) void conv_bn_act_kernel(const ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float As[BK * LD];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

  // the loading role for A: NHWC -> output pixel tid / 4, two float4 (k = 4 q .. 4 q + 3 and 16 + the same) of its cin run;
  //                          frame -> output pixel tid % 64, k = tid / 64 + 4 i (the frame is read element by element)
  const int am = KIND == WVN_CONV_IN_NHWC ? (tid >> 2) : (tid & 63);
  const bool avalid = m0 + am < a.M;
  int ab, aiy0, aix0;
  {
    const int mm = avalid ? m0 + am : 0;
    const int ox = mm % a.OW, t = mm / a.OW, oy = t % a.OH;
    ab = t / a.OH;
    aiy0 = oy * a.stride - a.pad;
    aix0 = ox * a.stride - a.pad;
  }
  const int bk = tid >> 4, bn4 = (tid & 15) * 4;
  float areg[8];
  float4 breg0, breg1;   // (two scalars, not an array: an array captured by reference stays in memory)
  // (the fields the loads read, as values: a lambda that captured the argument block by reference would force it into scratch memory)
  const void* const in = a.in;
  const float* const wgt = a.w;
  const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout, KW = a.KW, K = a.K;

  auto load = [&areg, &breg0, &breg1, in, wgt, H, W, Cin, Cout, KW, K, tid, avalid, ab, aiy0, aix0, bk, bn4, n0](int k0) {
    if (KIND == WVN_CONV_IN_NHWC) {
      const int tap = k0 / Cin, c0 = k0 - tap * Cin;   // Cin % 32 == 0: one chunk lies within one tap
      const int ky = tap / KW, kx = tap - ky * KW;
      const int iy = aiy0 + ky, ix = aix0 + kx;
      const bool ok = avalid && iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float* p = (const float*)in + (((size_t)ab * H + (ok ? iy : 0)) * W + (ok ? ix : 0)) * Cin + c0 + (tid & 3) * 4;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float4 v = ok ? *(const float4*)(p + 16 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        areg[4 * j + 0] = v.x;
        areg[4 * j + 1] = v.y;
        areg[4 * j + 2] = v.z;
        areg[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = k0 + (tid >> 6) + 4 * i;
        float v = 0.f;
        if (avalid && k < K) {
          const int tap = k / Cin, c = k - tap * Cin;
          const int ky = tap / KW, kx = tap - ky * KW;
          const int iy = aiy0 + ky, ix = aix0 + kx;
          if (iy >= 0 && iy < H && ix >= 0 && ix < W)
            v = frame_value(in, KIND, (((size_t)ab * Cin + c) * H + iy) * W + ix, c);
        }
        areg[i] = v;
      }
    }
    breg0 = *(const float4*)(wgt + (size_t)(k0 + bk) * Cout + n0 + bn4);
    breg1 = *(const float4*)(wgt + (size_t)(k0 + bk + 16) * Cout + n0 + bn4);
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  load(0);
  for (int k0 = 0; k0 < a.Kpad; k0 += BK) {
    if (KIND == WVN_CONV_IN_NHWC) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) As[(16 * j + (tid & 3) * 4 + e) * LD + am] = areg[4 * j + e];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) As[((tid >> 6) + 4 * i) * LD + am] = areg[i];
    }
    *(float4*)&Bs[bk * LD + bn4] = breg0;
    *(float4*)&Bs[(bk + 16) * LD + bn4] = breg1;
    __syncthreads();
    if (k0 + BK < a.Kpad) load(k0 + BK);
    const float* pa = As + (lane >> 5) * LD + wm * 32 + (lane & 31);
    const float* pb = Bs + (lane >> 5) * LD + wn * 32 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * kk * LD], pb[2 * kk * LD], acc, 0, 0, 0);
    __syncthreads();
  }

  const int n = n0 + wn * 32 + (lane & 31);
  const float sc = a.scale[n], sh = a.shift[n];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (m < a.M) {
      const size_t o = (size_t)m * a.Cout + n;
      float v = fmaf(acc[r], sc, sh);
      if (a.resid) v += a.resid[o];
      if (a.relu) v = v < 0.f ? 0.f : v;
      a.out[o] = v;
    }
  }
}

// w [Cout][Cin][KH][KW] -> wp [Kpad][Cout]
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int KH,
                                                        int KW, int K, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = (int)(i % Cout), k = (int)(i / Cout);
  float v = 0.f;
  if (k < K) {
    const int tap = k / Cin, c = k - tap * Cin;
    const int ky = tap / KW, kx = tap - ky * KW;
    v = w[(((size_t)n * Cin + c) * KH + ky) * KW + kx];
  }
  wp[i] = v;
}

// 3 x 3, stride 2, pad 1 over NHWC; the padding is -inf
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int OH,
                                                      int OW, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  long long t = i / C;
  const int ox = (int)(t % OW);
  t /= OW;
  const int oy = (int)(t % OH);
  const long long b = t / OH;
  float best = -__builtin_inff();
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int iy = 2 * oy - 1 + dy;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int ix = 2 * ox - 1 + dx;
      if (ix < 0 || ix >= W) continue;
      const float v = in[((size_t)(b * H + iy) * W + ix) * C + c];
      best = v > best ? v : best;
    }
  }
  out[i] = best;
}

int kpad_of(int Cin, int k) { return (Cin * k * k + BK - 1) / BK * BK; }

bool conv_shape_ok(int in_kind, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad) {
  if (B < 1 || H < 1 || W < 1 || H > 32768 || W > 32768 || Cin < 1 || Cout < BN || Cout % BN || Cout > 4096 || k < 1 || k > 7 ||
      (stride != 1 && stride != 2) || pad < 0 || pad > 3)
    return false;
  if (in_kind == WVN_CONV_IN_NHWC ? (Cin % BK != 0 || Cin > 4096) : Cin != 3) return false;
  if (in_kind != WVN_CONV_IN_NHWC && in_kind != WVN_CONV_IN_FRAME_F32 && in_kind != WVN_CONV_IN_FRAME_U8) return false;
  if (H + 2 * pad < k || W + 2 * pad < k) return false;
  const long long OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
  return (long long)B * OH * OW < (1ll << 31) - BM && (long long)B * H * W < (1ll << 31);
}

int conv_launch(const void* in, int in_kind, const float* wp, const float* scale, const float* shift, const float* resid, int relu,
                float* out, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad, hipStream_t st) {
  if (!in || !wp || !scale || !shift || !out || !conv_shape_ok(in_kind, B, H, W, Cin, Cout, k, stride, pad)) return WVN_ERR_ARG;
  ConvArgs a;
  a.in = in; a.w = wp; a.scale = scale; a.shift = shift; a.resid = resid; a.out = out;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KH = k; a.KW = k; a.stride = stride; a.pad = pad;
  a.OH = (H + 2 * pad - k) / stride + 1;
  a.OW = (W + 2 * pad - k) / stride + 1;
  a.K = Cin * k * k;
  a.Kpad = kpad_of(Cin, k);
  a.relu = relu;
  a.M = B * a.OH * a.OW;
  const dim3 grid(ceil_div(a.M, BM), Cout / BN);
  if (in_kind == WVN_CONV_IN_NHWC)
    hipLaunchKernelGGL(conv_bn_act_kernel<WVN_CONV_IN_NHWC>, grid, dim3(256), 0, st, a);
  else if (in_kind == WVN_CONV_IN_FRAME_F32)
    hipLaunchKernelGGL(conv_bn_act_kernel<WVN_CONV_IN_FRAME_F32>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(conv_bn_act_kernel<WVN_CONV_IN_FRAME_U8>, grid, dim3(256), 0, st, a);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int pack_launch(const float* w, float* wp, int Cout, int Cin, int k, hipStream_t st) {
  const long long total = (long long)kpad_of(Cin, k) * Cout;
  hipLaunchKernelGGL(conv_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, wp, Cout, Cin, k, k, Cin * k * k, total);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int maxpool_launch(const float* in, float* out, int B, int H, int W, int C, hipStream_t st) {
  if (!in || !out || B < 1 || H < 1 || W < 1 || C < 1 || H > 32768 || W > 32768 || C > 4096) return WVN_ERR_ARG;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const long long total = (long long)B * OH * OW * C;
  if (total >= (1ll << 39) || (long long)B * H * W >= (1ll << 31)) return WVN_ERR_ARG;
  hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, out, H, W, C, OH, OW, total);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

// The 20 convolutions of ResNet-18 in the order of include/wvn_hip.h
struct ConvSpec {
  int cin, cout, k, stride, pad;
};

void resnet18_specs(ConvSpec (&s)[NCONV]) {
  int i = 0;
  s[i++] = {3, 64, 7, 2, 3};
  for (int L = 1; L <= 4; ++L) {
    const int c = 64 << (L - 1), cin = L == 1 ? 64 : c / 2;
    s[i++] = {cin, c, 3, L == 1 ? 1 : 2, 1};
    s[i++] = {c, c, 3, 1, 1};
    if (L > 1) s[i++] = {cin, c, 1, 2, 0};
    s[i++] = {c, c, 3, 1, 1};
    s[i++] = {c, c, 3, 1, 1};
  }
}

size_t conv_pack_floats(const ConvSpec& s) { return (size_t)kpad_of(s.cin, s.k) * s.cout + 2 * (size_t)s.cout; }

bool frames_ok(int B, int H, int W) {
  return B >= 1 && B <= 4096 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0 && H <= 8192 && W <= 8192 &&
         (long long)B * H * W <= (1ll << 30);
}

size_t level_bytes(int B, int H, int W, int level) {   // level 1..4: stride 2^(level + 1), 32 * 2^level channels
  const int s = 2 << level;
  return (size_t)B * (H / s) * (W / s) * (32u << level) * sizeof(float);
}

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

}  // namespace

size_t wvn_conv2d_pack_floats(int Cout, int Cin, int ksize) {
  if (Cout < 1 || Cin < 1 || ksize < 1 || ksize > 7 || Cout > 4096 || Cin > 4096) return 0;
  return (size_t)kpad_of(Cin, ksize) * Cout;
}

int wvn_conv2d_pack(const float* w, float* packed, int Cout, int Cin, int ksize, void* stream) {
  if (!w || !packed || wvn_conv2d_pack_floats(Cout, Cin, ksize) == 0) return WVN_ERR_ARG;
  return pack_launch(w, packed, Cout, Cin, ksize, (hipStream_t)stream);
}

int wvn_conv2d_bn_act(const void* in, int in_kind, const float* packed, const float* scale, const float* shift, const float* residual,
                      int relu, float* out, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, void* stream) {
  return conv_launch(in, in_kind, packed, scale, shift, residual, relu, out, B, H, W, Cin, Cout, ksize, stride, pad, (hipStream_t)stream);
}

int wvn_maxpool3x3s2(const float* in, float* out, int B, int H, int W, int C, void* stream) {
  return maxpool_launch(in, out, B, H, W, C, (hipStream_t)stream);
}

size_t wvn_resnet18_pack_bytes(void) {
  ConvSpec s[NCONV];
  resnet18_specs(s);
  size_t n = 0;
  for (int i = 0; i < NCONV; ++i) n += conv_pack_floats(s[i]);
  return n * sizeof(float);
}

int wvn_resnet18_pack(const void* const* conv_w, const void* const* scale, const void* const* shift, void* packed, size_t packed_bytes,
                      void* stream) {
  if (!conv_w || !scale || !shift || !packed || packed_bytes < wvn_resnet18_pack_bytes()) return WVN_ERR_ARG;
  for (int i = 0; i < NCONV; ++i)
    if (!conv_w[i] || !scale[i] || !shift[i]) return WVN_ERR_ARG;
  ConvSpec s[NCONV];
  resnet18_specs(s);
  float* p = (float*)packed;
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < NCONV; ++i) {
    const int rc = pack_launch((const float*)conv_w[i], p, s[i].cout, s[i].cin, s[i].k, st);
    if (rc != WVN_OK) return rc;
    p += (size_t)kpad_of(s[i].cin, s[i].k) * s[i].cout;
    hipError_t e = hipMemcpyAsync(p, scale[i], s[i].cout * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
    p += s[i].cout;
    e = hipMemcpyAsync(p, shift[i], s[i].cout * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
    p += s[i].cout;
  }
  return WVN_OK;
}

size_t wvn_resnet18_level_offset(int B, int H, int W, int level) {
  if (!frames_ok(B, H, W) || level < 1 || level > 5) return 0;
  size_t off = 0;
  for (int l = 1; l < level; ++l) off += align256(level_bytes(B, H, W, l));
  return off;   // (level 5: the end of the four maps = the start of the temporaries)
}

size_t wvn_resnet18_workspace_bytes(int B, int H, int W) {
  if (!frames_ok(B, H, W)) return 0;
  // four level maps | the stem's output (later: three stage-sized temporaries) | the max-pooled map
  return wvn_resnet18_level_offset(B, H, W, 5) + 5 * align256(level_bytes(B, H, W, 1));
}

int wvn_resnet18_forward(const void* packed, const void* frames, int frames_u8, int B, int H, int W, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!packed || !frames || !workspace || !frames_ok(B, H, W)) return WVN_ERR_ARG;
  if (workspace_bytes < wvn_resnet18_workspace_bytes(B, H, W)) return WVN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  ConvSpec s[NCONV];
  resnet18_specs(s);
  const float* wp[NCONV];
  {
    const float* p = (const float*)packed;
    for (int i = 0; i < NCONV; ++i) {
      wp[i] = p;
      p += conv_pack_floats(s[i]);
    }
  }
  char* ws = (char*)workspace;
  float* level[5];
  for (int l = 1; l <= 4; ++l) level[l] = (float*)(ws + wvn_resnet18_level_offset(B, H, W, l));
  const size_t l1 = align256(level_bytes(B, H, W, 1));
  char* tmp = ws + wvn_resnet18_level_offset(B, H, W, 5);
  float* t0 = (float*)tmp;                      // stem output [B][H/2][W/2][64] = 4 x the size of level 1
  float* t1 = (float*)tmp;                      // after the max-pool the stem output is dead: its room holds the block temporaries
  float* t2 = (float*)(tmp + l1);
  float* t3 = (float*)(tmp + 2 * l1);
  float* pooled = (float*)(tmp + 4 * l1);

  auto conv = [&](int i, const void* in, int kind, const float* resid, int relu, float* out, int h, int w) {
    const float* scale = wp[i] + (size_t)kpad_of(s[i].cin, s[i].k) * s[i].cout;
    return conv_launch(in, kind, wp[i], scale, scale + s[i].cout, resid, relu, out, B, h, w, s[i].cin, s[i].cout, s[i].k, s[i].stride,
                       s[i].pad, st);
  };
  int rc = conv(0, frames, frames_u8 ? WVN_CONV_IN_FRAME_U8 : WVN_CONV_IN_FRAME_F32, nullptr, 1, t0, H, W);
  if (rc != WVN_OK) return rc;
  rc = maxpool_launch(t0, pooled, B, H / 2, W / 2, 64, st);
  if (rc != WVN_OK) return rc;
  const float* x = pooled;
  int h = H / 4, w = W / 4, i = 1;
  for (int L = 1; L <= 4; ++L) {
    // block 0 (stride 2 and a 1 x 1 downsample branch from stage 2 on)
    const float* ident = x;
    if ((rc = conv(i, x, WVN_CONV_IN_NHWC, nullptr, 1, t1, h, w)) != WVN_OK) return rc;
    const int c2 = i + 1;
    i += 2;
    if (L > 1) {
      if ((rc = conv(i, x, WVN_CONV_IN_NHWC, nullptr, 0, t3, h, w)) != WVN_OK) return rc;
      ++i;
      ident = t3;
      h /= 2;
      w /= 2;
    }
    if ((rc = conv(c2, t1, WVN_CONV_IN_NHWC, ident, 1, t2, h, w)) != WVN_OK) return rc;
    // block 1
    if ((rc = conv(i++, t2, WVN_CONV_IN_NHWC, nullptr, 1, t1, h, w)) != WVN_OK) return rc;
    if ((rc = conv(i++, t1, WVN_CONV_IN_NHWC, t2, 1, level[L], h, w)) != WVN_OK) return rc;
    x = level[L];
  }
  return WVN_OK;
}
