// segmentation_type "random" of the feature extractor (feature_extractor.py:96-111 of the reference: draw nr pixels of the frame,
// index the dense feature map there) without a host-side permutation, a pooling pass or the dense map.
//
//   random_pixels_kernel    idx[b][j] = pi(j) (j < nr) and seg[b][p] = pi^-1(p) < nr ? pi^-1(p) : -1 in one launch
//   gather_bilinear_kernel  feat[b][j][:] = the align_corners bilinear value of the patch tokens at pixel idx[b][j]
//
// pi is a keyed bijection of [0, H*W): a balanced four-round Feistel network on 2n bits (4^n the smallest such power >= H*W),
// restricted to [0, H*W) by cycle walking (the network is applied until the value falls inside; 4^n < 4 H*W, so fewer than four
// applications are expected).  Round keys: the high words of four splitmix64 outputs from the state seed << 32 ^ frame; round
// function: murmur3's 32-bit finaliser of R ^ key.  Every thread evaluates pi or pi^-1 on its own argument: distinct samples
// follow from pi being a bijection, never from what another thread drew, so there is no sort, no atomic and no dependence on
// the launch geometry.  tests/random_pixels_ref.py is the same statement in numpy integers.
#include "../../include/wvn_hip.h"

#include "common.h"
#include "wvn_internal.h"

namespace {

constexpr int RP_ROUNDS = 4;
struct RpKeys { uint32_t k[RP_ROUNDS]; };

__host__ __device__ inline RpKeys rp_keys(uint32_t seed, uint32_t frame) {
  uint64_t state = ((uint64_t)seed << 32) ^ (uint64_t)frame;
  RpKeys r;
  for (int i = 0; i < RP_ROUNDS; ++i) {   // splitmix64
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    r.k[i] = (uint32_t)(z >> 32);
  }
  return r;
}

__host__ __device__ inline uint32_t rp_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

// x < npix <= 4^n <= 2^30.  The walk ends: it follows the cycle of x under a bijection of [0, 4^n), which returns to x < npix.
__host__ __device__ inline uint32_t rp_forward(uint32_t x, const RpKeys& key, int n, uint32_t npix) {
  const uint32_t mask = (1u << n) - 1u;
  do {
    uint32_t L = x >> n, R = x & mask;
#pragma unroll
    for (int i = 0; i < RP_ROUNDS; ++i) {
      const uint32_t t = L ^ (rp_fmix32(R ^ key.k[i]) & mask);
      L = R;
      R = t;
    }
    x = (L << n) | R;
  } while (x >= npix);
  return x;
}
__host__ __device__ inline uint32_t rp_inverse(uint32_t x, const RpKeys& key, int n, uint32_t npix) {
  const uint32_t mask = (1u << n) - 1u;
  do {
    uint32_t L = x >> n, R = x & mask;
#pragma unroll
    for (int i = RP_ROUNDS - 1; i >= 0; --i) {
      const uint32_t t = R ^ (rp_fmix32(L ^ key.k[i]) & mask);
      R = L;
      L = t;
    }
    x = (L << n) | R;
  } while (x >= npix);
  return x;
}

// grid (ceil(count / 256), B), count = npix when the map is wanted, nr otherwise: thread t writes seg[b][t], and idx[b][t] if t < nr
__global__ __launch_bounds__(256) void random_pixels_kernel(uint32_t seed, uint32_t frame0, int n, uint32_t npix, uint32_t nr,
                                                            int* __restrict__ idx, int* __restrict__ seg) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t b = blockIdx.y;
  if (t >= npix) return;
  const RpKeys key = rp_keys(seed, frame0 + b);   // (unsigned: the frame index wraps at 2^32)
  if (seg) {
    const uint32_t q = rp_inverse(t, key, n, npix);
    seg[(size_t)b * npix + t] = q < nr ? (int)q : -1;
  }
  if (idx && t < nr) idx[(size_t)b * nr + t] = (int)rp_forward(t, key, n, npix);
}

// One wave per sample, lanes over channels: the four token rows are read as runs of 64 consecutive floats.  The taps and the
// operation order are those of upsample_kernel (elementwise.hip), so feat is bit-identical to the dense map at that pixel.
// An index outside [0, H*H) gives a NaN row (idx is the caller's: nothing is read through it unchecked).
constexpr int GB_WAVES = 4;
__global__ __launch_bounds__(GB_WAVES * WVN_WAVE) void gather_bilinear_kernel(const float* __restrict__ tok, const int* __restrict__ idx,
                                                                              float* __restrict__ feat, int G, int H, int D, int nr) {
  const int lane = threadIdx.x & (WVN_WAVE - 1);
  const int j = blockIdx.x * GB_WAVES + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  if (j >= nr) return;
  const int p = idx[(size_t)b * nr + j];
  float* out = feat + ((size_t)b * nr + j) * D;
  if (p < 0 || p >= H * H) {
    for (int c = lane; c < D; c += WVN_WAVE) out[c] = __builtin_nanf("");
    return;
  }
  const float scale = lerp_scale(G, H);
  const LerpTap ty = lerp_tap(p / H, G, scale), tx = lerp_tap(p % H, G, scale);
  const float* base = tok + (size_t)b * G * G * D;
  const float* r00 = base + (size_t)(ty.i0 * G + tx.i0) * D;
  const float* r01 = base + (size_t)(ty.i0 * G + tx.i1) * D;
  const float* r10 = base + (size_t)(ty.i1 * G + tx.i0) * D;
  const float* r11 = base + (size_t)(ty.i1 * G + tx.i1) * D;
  for (int c = lane; c < D; c += WVN_WAVE)
    out[c] = bilerp_fixed(r00[c], r01[c], r10[c], r11[c], tx.w0, tx.w1, ty.w0, ty.w1);
}

}  // namespace

extern "C" int wvn_random_pixels(unsigned seed, unsigned frame0, int B, int H, int W, int nr, int* idx, int* seg, void* stream) {
  if ((!idx && !seg) || B < 1 || B > 65535 || H < 1 || W < 1 || nr < 1) return WVN_ERR_ARG;
  const long long npix = (long long)H * W;
  if (npix > (1ll << 30) || nr > npix) return WVN_ERR_ARG;
  int n = 0;
  while ((1ll << (2 * n)) < npix) ++n;
  const long long count = seg ? npix : nr;
  hipLaunchKernelGGL(random_pixels_kernel, dim3((unsigned)((count + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, (uint32_t)seed,
                     (uint32_t)frame0, n, (uint32_t)npix, (uint32_t)nr, idx, seg);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

extern "C" int wvn_gather_bilinear(const float* tokens, const int* idx, float* feat, int B, int G, int H, int D, int nr, void* stream) {
  if (!tokens || !idx || !feat || B < 1 || B > 65535 || G < 1 || H < 1 || H > 32768 || D < 1 || nr < 1) return WVN_ERR_ARG;
  hipLaunchKernelGGL(gather_bilinear_kernel, dim3(ceil_div(nr, GB_WAVES), B), dim3(GB_WAVES * WVN_WAVE), 0, (hipStream_t)stream, tokens, idx,
                     feat, G, H, D, nr);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
