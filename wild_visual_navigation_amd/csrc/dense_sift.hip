// feature_type "sift" of the feature extractor (feature_extractor.py:65-67, 276-286 of the reference: kornia's DenseSIFTDescriptor run
// per colour channel as 8 + 1 convolutions, then the per-segment means of the [1, 384, H, W] map) as two fused kernels, fp32.
// The definition (include/wvn_hip.h; tests/dense_sift_ref.py states it in float64), for one channel I [H][W] in [0, 1]:
//   1. gx, gy: central differences / 2 with replicate padding;   2. mag = sqrt(gx^2 + gy^2 + eps), ori = atan2(gy, gx + eps) + 2 pi,
//      o = 8 ori / (2 pi), b0 = floor(o) mod 8, b1 = (b0 + 1) mod 8, w1 = o - floor(o): planes P_a = [b0 = a](1 - w1) mag + [b1 = a] w1 mag;
//   3. Q_a [H+1][W+1] = P_a (zero padding 2) cross-correlated with k (x) k, k = [0.25, 0.75, 0.75, 0.25];
//   4. d[a * 16 + i * 4 + j][y][x] = Q_a[y - 1 + i][x - 1 + j] (0 outside Q);   5. L2 normalise, clamp to [0, 0.2], L2 normalise, rootsift.
//
// One workgroup = one 8 x 32 tile of one channel of one image.  A wave is two tile rows of 32 pixels, so the 32 lanes one LDS cycle
// serves read 32 consecutive floats whatever the row stride: the 128-value gather of step 4 and the 16-tap sums of step 3 are free of
// bank conflicts, and every global store of the dense map is two runs of 128 bytes.  (A 16 x 16 tile puts two rows into each 32-lane
// group; rows 19 floats apart collide on three banks.)  Stages, each separated by a barrier:
//   image window 16 x 40 (tile + halo 4, coordinates clamped: the replicate padding) -> LDS
//   planes P, window 14 x 38 (tile + halo 3; 0 outside the image: the zero padding of step 3), 8 planes                 -> LDS, 17 KB
//   pooled   Q, window 11 x 35 (0 outside [0, H] x [0, W]: the zero padding of step 4), 8 planes                        -> LDS, 12 KB
//   sift_descriptor(): each lane gathers its 128 values and runs step 5 in registers.
// sift_descriptor() is the ONE statement of the per-pixel arithmetic; the two kernels below are its consumers, so the pooled features
// are sums of exactly the bits the dense map holds.  The unit is compiled with -ffp-contract=off: every fused multiply-add is written.
//
//   dense_sift_kernel          stores the 128 values to out [B][128 C][H][W].
//   dense_sift_segpool_kernel  never writes the map: per-segment sums of trunc(v * 2^32) (exact in fp32, v <= 1; integer, so order-free)
//       * a tile without a labelled pixel returns before any arithmetic (segmentation_type "random": 100 labelled pixels per frame);
//       * the labels of the tile are entered into a 16-slot hash table in LDS;
//       * 16 channels at a time the values go through LDS ([pixel][16 + 1]: conflict-free both ways), thread (channel, 16-pixel half row)
//         adds up each run of equal labels in a register and adds the run to its label's slot (LDS 64-bit integer atomic; a label that
//         found no slot goes to the global sum directly);
//       * the slots are added to the global sums [B][S][128 C] with one 64-bit atomic per (label present in the tile, channel).
//   dense_sift_segpool_final_kernel  feat = float(double(sum) / (double(count) * 2^32)), NaN for an id without a pixel.
#include "../../include/wvn_hip.h"

#include "common.h"
#include "wvn_internal.h"

namespace {

constexpr int TW = 32, TH = 8;                       // tile (pixels); TW * TH = the 256 threads of the workgroup
constexpr int IW = TW + 8, IH = TH + 8;              // image window: halo 4
constexpr int PW = TW + 6, PH = TH + 6;              // gradient planes: halo 3
constexpr int QW = TW + 3, QH = TH + 3;              // pooled window: rows y0 - 1 .. y0 + TH + 1
constexpr int NA = 8;                                // angular bins
constexpr int ND = 128;                              // descriptor length
constexpr int CH = 16;                               // channels per pass of the pooling
constexpr int LDB = CH + 1;                          // row stride of the pooling buffer
constexpr int NSLOT = 16;                            // labels a tile pre-reduces in LDS
constexpr int PLANE_FLOATS = (NA * PH * PW > TW * TH * LDB) ? NA * PH * PW : TW * TH * LDB;   // P, later the pooling buffer
constexpr float SIFT_EPS = 1e-10f;
constexpr float TWO_PI_F = 6.283185307179586f;
constexpr float FIX32 = 4294967296.0f;               // 2^32

struct SiftLds {
  float img[IH * IW];
  float plane[PLANE_FLOATS];
  float q[NA * QH * QW];
};

template <bool U8>
__device__ inline float sift_load(const void* img, size_t i) {
  if (U8) return (float)((const unsigned char*)img)[i] / 255.f;
  return ((const float*)img)[i];
}

// Stages 1-3 for the tile at (y0, x0) of the channel plane `img` [H][W]: leaves Q in lds.q (the caller's barrier included).
template <bool U8>
__device__ inline void sift_stage(const void* img, int H, int W, int y0, int x0, SiftLds& lds) {
  const int tid = threadIdx.x;
  for (int e = tid; e < IH * IW; e += TW * TH) {
    const int r = e / IW, c = e - r * IW;
    const int y = min(max(y0 - 4 + r, 0), H - 1), x = min(max(x0 - 4 + c, 0), W - 1);
    lds.img[e] = sift_load<U8>(img, (size_t)y * W + x);
  }
  __syncthreads();
  for (int e = tid; e < PH * PW; e += TW * TH) {
    const int r = e / PW, c = e - r * PW;
    const int y = y0 - 3 + r, x = x0 - 3 + c;
    float v0 = 0.f, v1 = 0.f;
    int b0 = 0, b1 = 1;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const float* p = lds.img + (r + 1) * IW + (c + 1);
      // at the image border the clamped window already holds the replicated neighbour
      const float gx = (p[1] - p[-1]) * 0.5f, gy = (p[IW] - p[-IW]) * 0.5f;
      const float mag = sqrtf(fmaf(gy, gy, gx * gx) + SIFT_EPS);
      const float ori = atan2f(gy, gx + SIFT_EPS) + TWO_PI_F;
      const float o = (8.f * ori) / TWO_PI_F;
      const float fl = floorf(o);
      const float w1 = o - fl;
      b0 = ((int)fl) & (NA - 1);
      b1 = (b0 + 1) & (NA - 1);
      v0 = (1.f - w1) * mag;
      v1 = w1 * mag;
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) lds.plane[a * PH * PW + e] = (a == b0 ? v0 : 0.f) + (a == b1 ? v1 : 0.f);
  }
  __syncthreads();
  for (int e = tid; e < NA * QH * QW; e += TW * TH) {
    const int a = e / (QH * QW), rem = e - a * QH * QW;
    const int u = rem / QW, v = rem - u * QW;
    const int p = y0 - 1 + u, q = x0 - 1 + v;
    float s = 0.f;
    if (p >= 0 && p <= H && q >= 0 && q <= W) {
      const float* src = lds.plane + a * PH * PW + u * PW + v;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ki = (i == 0 || i == 3) ? 0.25f : 0.75f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(ki * ((j == 0 || j == 3) ? 0.25f : 0.75f), src[i * PW + j], s);
      }
    }
    lds.q[e] = s;
  }
  __syncthreads();
}

// sum of the 128 values in four interleaved partial sums (a fixed order)
__device__ inline float sift_sum(const float (&d)[ND], bool squares) {
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < ND; ++i) s[i & 3] = squares ? fmaf(d[i], d[i], s[i & 3]) : s[i & 3] + d[i];
  return (s[0] + s[1]) + (s[2] + s[3]);
}

// Steps 4 and 5 for the pixel (ty, tx) of the tile whose Q window is in LDS
__device__ inline void sift_descriptor(const float* q, int ty, int tx, float (&d)[ND]) {
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) d[a * 16 + i * 4 + j] = q[a * QH * QW + (ty + i) * QW + tx + j];
  float r = 1.f / fmaxf(sqrtf(sift_sum(d, true)), 1e-12f);
#pragma unroll
  for (int i = 0; i < ND; ++i) d[i] = fminf(fmaxf(d[i] * r, 0.f), 0.2f);
  r = 1.f / fmaxf(sqrtf(sift_sum(d, true)), 1e-12f);
#pragma unroll
  for (int i = 0; i < ND; ++i) d[i] *= r;
  r = 1.f / fmaxf(sift_sum(d, false), 1e-12f);   // (d >= 0: the L1 norm is the sum)
#pragma unroll
  for (int i = 0; i < ND; ++i) d[i] = sqrtf(fmaf(d[i], r, SIFT_EPS));
}

// grid (ceil(W / TW), ceil(H / TH), B * C)
template <bool U8>
__global__ __launch_bounds__(TW * TH) void dense_sift_kernel(const void* __restrict__ img, float* __restrict__ out, int H, int W) {
  __shared__ SiftLds lds;
  const size_t npix = (size_t)H * W;
  const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const size_t plane = blockIdx.z;                     // b * C + c: the map's channel block is [b][c * 128 ..]
  sift_stage<U8>(U8 ? (const void*)((const unsigned char*)img + plane * npix) : (const void*)((const float*)img + plane * npix), H, W,
                 y0, x0, lds);
  const int ty = threadIdx.x / TW, tx = threadIdx.x % TW;
  float d[ND];
  sift_descriptor(lds.q, ty, tx, d);
  const int y = y0 + ty, x = x0 + tx;
  if (y >= H || x >= W) return;
  float* o = out + plane * ND * npix + (size_t)y * W + x;
#pragma unroll
  for (int i = 0; i < ND; ++i) o[(size_t)i * npix] = d[i];
}

// slot of `label` in the tile's table, -1 if it found none (the table only ever grows before the barrier that precedes every lookup)
__device__ inline int sift_slot(const int* keys, int label) {
  unsigned h = ((unsigned)label * 0x9E3779B1u) >> 28;
  for (int probe = 0; probe < NSLOT; ++probe) {
    const int k = keys[h];
    if (k == label) return (int)h;
    if (k < 0) return -1;
    h = (h + 1) & (NSLOT - 1);
  }
  return -1;
}

// grid as above.  sum [B][S][128 C] and cnt [B][S] are zero on entry; counts are added by the blocks of channel 0 only.
template <bool U8>
__global__ __launch_bounds__(TW * TH) void dense_sift_segpool_kernel(const void* __restrict__ img, const int* __restrict__ seg,
                                                                     unsigned long long* __restrict__ sum, int* __restrict__ cnt, int C,
                                                                     int H, int W, int S) {
  __shared__ SiftLds lds;
  __shared__ unsigned long long acc[NSLOT * ND];
  __shared__ int lab[TW * TH];
  __shared__ int keys[NSLOT];
  __shared__ int slot_cnt[NSLOT];
  const int tid = threadIdx.x;
  const size_t npix = (size_t)H * W;
  const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const int b = blockIdx.z / C, c = blockIdx.z - b * C;
  const int ty = tid / TW, tx = tid % TW;
  int label = -1;
  if (y0 + ty < H && x0 + tx < W) {
    label = seg[(size_t)b * npix + (size_t)(y0 + ty) * W + x0 + tx];
    if (label < 0 || label >= S) label = -1;
  }
  if (!__syncthreads_or(label >= 0)) return;           // nothing to pool here: no load of the image, no arithmetic
  lab[tid] = label;
  if (tid < NSLOT) { keys[tid] = -1; slot_cnt[tid] = 0; }
  for (int e = tid; e < NSLOT * ND; e += TW * TH) acc[e] = 0ull;
  __syncthreads();
  if (label >= 0) {
    unsigned h = ((unsigned)label * 0x9E3779B1u) >> 28;
    for (int probe = 0; probe < NSLOT; ++probe) {
      const int old = atomicCAS(&keys[h], -1, label);
      if (old == -1 || old == label) break;
      h = (h + 1) & (NSLOT - 1);
    }
  }
  const size_t plane = blockIdx.z;
  sift_stage<U8>(U8 ? (const void*)((const unsigned char*)img + plane * npix) : (const void*)((const float*)img + plane * npix), H, W,
                 y0, x0, lds);                          // (its barriers also publish lab and keys)
  float d[ND];
  sift_descriptor(lds.q, ty, tx, d);

  const int CD = ND * C;
  unsigned long long* gsum = sum + (size_t)b * S * CD + (size_t)c * ND;
  int* gcnt = cnt + (size_t)b * S;
  float* buf = lds.plane;                               // P is dead: every lane has formed Q (sift_stage's last barrier)
  const int rc = tid % CH, rp0 = (tid / CH) * CH;       // the reducing role: channel rc of the pass, pixels rp0 .. rp0 + 15
#pragma unroll
  for (int pass = 0; pass < ND / CH; ++pass) {
    if (pass) __syncthreads();                          // the readers of the previous pass are done
#pragma unroll
    for (int k = 0; k < CH; ++k) buf[tid * LDB + k] = d[pass * CH + k];
    __syncthreads();
    const int ch = pass * CH + rc;
    int cur = -1, run = 0;
    unsigned long long a = 0ull;
    for (int i = 0; i <= CH; ++i) {
      const int l = i < CH ? lab[rp0 + i] : -1;
      if (l != cur) {
        if (cur >= 0) {
          const int slot = sift_slot(keys, cur);
          if (slot >= 0) {
            atomicAdd(&acc[slot * ND + ch], a);
            if (pass == 0 && rc == 0 && c == 0) atomicAdd(&slot_cnt[slot], run);
          } else {
            atomicAdd(gsum + (size_t)cur * CD + ch, a);
            if (pass == 0 && rc == 0 && c == 0) atomicAdd(gcnt + cur, run);
          }
        }
        cur = l;
        a = 0ull;
        run = 0;
      }
      if (l >= 0) {
        a += (unsigned long long)(buf[(rp0 + i) * LDB + rc] * FIX32);   // trunc(v * 2^32), v in [0, 1]: exact
        ++run;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < NSLOT * ND; e += TW * TH) {
    const int k = keys[e / ND];
    const unsigned long long v = acc[e];
    if (k >= 0 && v) atomicAdd(gsum + (size_t)k * CD + (e % ND), v);
  }
  if (tid < NSLOT && keys[tid] >= 0 && slot_cnt[tid]) atomicAdd(gcnt + keys[tid], slot_cnt[tid]);
}

__global__ __launch_bounds__(256) void dense_sift_segpool_final_kernel(const unsigned long long* __restrict__ sum, const int* __restrict__ cnt,
                                                                       float* __restrict__ feat, long long total, int CD) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = cnt[i / CD];
  feat[i] = n > 0 ? (float)((double)sum[i] / ((double)n * 4294967296.0)) : __builtin_nanf("");
}

bool sift_shape_ok(int B, int C, int H, int W) {
  return B >= 1 && (C == 1 || C == 3) && (long long)B * C <= 65535 && H >= 4 && W >= 4 && H <= WVN_DENSE_SIFT_MAX_SIDE &&
         W <= WVN_DENSE_SIFT_MAX_SIDE;
}

}  // namespace

int wvn_dense_sift_launch(const void* img, int img_is_u8, float* out, int B, int C, int H, int W, hipStream_t st) {
  if (!img || !out || !sift_shape_ok(B, C, H, W)) return WVN_ERR_ARG;
  const dim3 grid(ceil_div(W, TW), ceil_div(H, TH), B * C);
  if (img_is_u8)
    hipLaunchKernelGGL(dense_sift_kernel<true>, grid, dim3(TW * TH), 0, st, img, out, H, W);
  else
    hipLaunchKernelGGL(dense_sift_kernel<false>, grid, dim3(TW * TH), 0, st, img, out, H, W);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_dense_sift_segpool_launch(const void* img, int img_is_u8, const int* seg, float* feat, int* cnt, void* scratch_sum, int B, int C,
                                  int H, int W, int S, hipStream_t st) {
  if (!img || !seg || !feat || !cnt || !scratch_sum || !sift_shape_ok(B, C, H, W) || S < 1 || S > WVN_DENSE_SIFT_MAX_SEGMENTS)
    return WVN_ERR_ARG;
  const int CD = ND * C;
  const long long total = (long long)B * S * CD;
  if (total >= (1ll << 31)) return WVN_ERR_ARG;
  hipError_t e = hipMemsetAsync(scratch_sum, 0, (size_t)total * sizeof(unsigned long long), st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(cnt, 0, (size_t)B * S * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(ceil_div(W, TW), ceil_div(H, TH), B * C);
  if (img_is_u8)
    hipLaunchKernelGGL(dense_sift_segpool_kernel<true>, grid, dim3(TW * TH), 0, st, img, seg, (unsigned long long*)scratch_sum, cnt, C, H,
                       W, S);
  else
    hipLaunchKernelGGL(dense_sift_segpool_kernel<false>, grid, dim3(TW * TH), 0, st, img, seg, (unsigned long long*)scratch_sum, cnt, C,
                       H, W, S);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(dense_sift_segpool_final_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     (const unsigned long long*)scratch_sum, (const int*)cnt, feat, total, CD);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
