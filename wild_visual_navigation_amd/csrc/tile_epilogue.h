// The store epilogue of the 128 x 128 tiled MFMA GEMMs (gemm_bf16.hip in both operand formats, gemm_x3.hip, gemm_fp8.hip).
//
// Each of those kernels ends in two parts.  Part 1 (registers -> a row-major image of the output tile in the now idle operand LDS, bias /
// scales / activation applied) differs per kernel and stays there.  Part 2 (image -> global memory as 16-byte, fully coalesced stores:
// 256 contiguous bytes per 16 lanes) is the same everywhere and lives here, with the activation and the image geometry part 1 needs.
// The caller has a __syncthreads() between the two parts; 256 threads.
//
// Format-neutral: this header does not know operand.h.  16-bit images (bf16, fp16 or one plane of a split value) move as raw uint16_t /
// u32x4_t, so the objects of a source that is compiled once per operand format agree on every function defined here.
#pragma once
#include "wvn_internal.h"

constexpr int CT_16_STRIDE = 128 + 8;    // output-tile image of 16-bit elements: elements per row (272 B)
constexpr int CT_F32_STRIDE = 128 + 4;   // output-tile image of floats: floats per row (528 B)

// exact erf GELU (torch.nn.GELU default) with erf by Abramowitz-Stegun 7.1.26 (|abs err| < 1.5e-7: fp32-class for the split-operand
// kernel, far below the resolution of a 16-bit output) instead of libm's erff, whose ~40 VALU per element doubled an fc1 kernel's time
__device__ inline float gelu_as(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __frcp_rn(fmaf(0.3275911f, z, 1.0f));
  float p = fmaf(t, 1.061405429f, -1.453152027f);
  p = fmaf(t, p, 1.421413741f);
  p = fmaf(t, p, -0.284496736f);
  p = fmaf(t, p, 0.254829592f);
  const float e = 1.0f - p * t * __expf(-z * z);
  return 0.5f * x * (1.0f + copysignf(e, x));
}

template <int EPI>
__device__ inline float activate(float v) {
  if constexpr (EPI == EPI_GELU_BF16) return gelu_as(v);
  if constexpr (EPI == EPI_RELU_BF16) return fmaxf(v, 0.f);
  return v;
}

// the epilogues whose image is 16-bit (one image, or the hi / lo plane images of gemm_x3.hip); the others stage fp32
template <int EPI>
constexpr bool out_is_16bit() {
  return EPI == EPI_BF16 || EPI == EPI_GELU_BF16 || EPI == EPI_RELU_BF16 || EPI == EPI_QKV;
}

// EPI_QKV: one 16-bit image of the tile at rows m0.., columns cbase.. of its third (q, k or v) -> the attention kernels' layouts.
//   TR = true : q / k, image [m][n]            -> dst[(b*h + head)*npad + t][d]
//   TR = false: v,     image [n = (head, d)][m] -> dst[(b*h + head)*64 + d][t] (V^T), 8 tokens per store
template <bool TR, typename Params>
__device__ inline void tile_store_qkv(const Params& p, const uint16_t* img, uint16_t* dst, int m0, int cbase) {
  const int tid = threadIdx.x;
  if constexpr (TR) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int ch = tid + 256 * it, row = ch >> 4, c8 = (ch & 15) * 8;
      const int m = m0 + row;
      if (m >= p.M) continue;
      const int b = m / p.ntok_s, t = m - b * p.ntok_s;
      const int cc = cbase + c8, head = cc >> 6, d = cc & 63;
      const u32x4_t val = *(const u32x4_t*)(img + row * CT_16_STRIDE + c8);
      *(u32x4_t*)(dst + (((size_t)b * p.heads + head) * p.npad + t) * 64 + d) = val;
    }
  } else {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int ch = tid + 256 * it, row = ch >> 4, c8 = (ch & 15) * 8;
      const int m = m0 + c8;
      if (m >= p.M) continue;  // M % 16 == 0 (ntok_s % 16 == 0): a chunk (and its permutation group of 16) is entirely in or out
      const int b = m / p.ntok_s, t = m - b * p.ntok_s;
      const int cc = cbase + row, head = cc >> 6, d = cc & 63;
      const u32x4_t val = *(const u32x4_t*)(img + row * CT_16_STRIDE + c8);
      *(u32x4_t*)(dst + (((size_t)b * p.heads + head) * 64 + d) * p.npad + t) = val;
    }
  }
}

// one 16-bit image [m][n] -> C[M][ldc]; element by element where C is not 16-byte aligned, ldc % 8 != 0, or at the N edge
template <typename Params>
__device__ inline void tile_store_16bit(const Params& p, const uint16_t* img, uint16_t* C, int m0, int n0) {
  const int tid = threadIdx.x;
  const bool vec_ok = ((p.ldc & 7) == 0) && (((uintptr_t)C & 15) == 0);
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int ch = tid + 256 * it, row = ch >> 4, c8 = (ch & 15) * 8;
    const int m = m0 + row, n = n0 + c8;
    if (m >= p.M || n >= p.N) continue;
    const uint16_t* src = img + row * CT_16_STRIDE + c8;
    if (vec_ok && n + 8 <= p.N) {
      *(u32x4_t*)(C + (size_t)m * p.ldc + n) = *(const u32x4_t*)src;
    } else {
      for (int e = 0; e < 8 && n + e < p.N; ++e) C[(size_t)m * p.ldc + n + e] = src[e];
    }
  }
}

// the fp32 image [m][n] -> C[M][ldc]: EPI_F32 stores, EPI_RESID_F32 / EPI_ACCUM_F32 add to what is there, EPI_PATCH remaps the row
// (b, patch) -> b * ntok_s + 1 + patch and adds the position embedding; the same fallback to single elements as above (ldc % 4)
template <int EPI, typename Params>
__device__ inline void tile_store_f32(const Params& p, const float* img, float* C, int m0, int n0) {
  const int tid = threadIdx.x;
  const bool vec_ok = ((p.ldc & 3) == 0) && (((uintptr_t)C & 15) == 0);
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int ch = tid + 256 * it, row = ch >> 5, c4 = (ch & 31) * 4;
    const int m = m0 + row, n = n0 + c4;
    if (m >= p.M || n >= p.N) continue;
    f32x4_t v = *(const f32x4_t*)(img + row * CT_F32_STRIDE + c4);
    size_t orow = (size_t)m;
    if constexpr (EPI == EPI_PATCH) {
      const int b = m / p.npatch, pp = m - b * p.npatch;
      orow = (size_t)b * p.ntok_s + 1 + pp;
      const f32x4_t pe = *(const f32x4_t*)(p.pos + (size_t)(1 + pp) * p.ldc + n);  // ldc == D, n % 4 == 0
      v += pe;
    }
    float* dst = C + orow * p.ldc + n;
    if (vec_ok && n + 4 <= p.N) {
      if constexpr (EPI == EPI_RESID_F32 || EPI == EPI_ACCUM_F32) v += *(const f32x4_t*)dst;
      *(f32x4_t*)dst = v;
    } else {
      for (int e = 0; e < 4 && n + e < p.N; ++e) {
        float o = v[e];
        if constexpr (EPI == EPI_RESID_F32 || EPI == EPI_ACCUM_F32) o += dst[e];
        dst[e] = o;
      }
    }
  }
}
