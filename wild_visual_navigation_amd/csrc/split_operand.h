// MFMA operands of the transposed chains (pixel_mlp.hip, rnvp.hip: lane = row, registers = channels): a bf16 fragment of
// v_mfma_f32_32x32x16_bf16, or the hi + lo parts of one (v = hi + lo to 16 mantissa bits), and the products formed from them.
#pragma once
#include "common.h"

// from(hi, lo) takes both packed parts, load() reads the lo part lo_off bytes behind the hi part
__device__ inline bf16x8_t frag_at(const unsigned char* p) { return *(const bf16x8_t*)p; }
struct Single {
  bf16x8_t hi;
  __device__ static Single from(u32x4_t h, u32x4_t) { return {__builtin_bit_cast(bf16x8_t, h)}; }
  __device__ static Single load(const unsigned char* p, int) { return {frag_at(p)}; }
};
struct Split {
  bf16x8_t hi, lo;
  __device__ static Split from(u32x4_t h, u32x4_t l) { return {__builtin_bit_cast(bf16x8_t, h), __builtin_bit_cast(bf16x8_t, l)}; }
  __device__ static Split load(const unsigned char* p, int lo_off) { return {frag_at(p), frag_at(p + lo_off)}; }
};
template <bool EXACT> struct OperandOf { using type = Single; };
template <> struct OperandOf<true> { using type = Split; };

// acc += A * B:  hi*hi, then hi*lo if B is split, then lo*hi if A is split (lo*lo is below fp32 resolution)
__device__ inline void mma(f32x16_t& acc, const Single& a, const Single& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, acc, 0, 0, 0);
}
__device__ inline void mma(f32x16_t& acc, const Single& a, const Split& b) {
  mma(acc, a, Single{b.hi});
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, acc, 0, 0, 0);
}
__device__ inline void mma(f32x16_t& acc, const Split& a, const Split& b) {
  mma(acc, Single{a.hi}, b);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, acc, 0, 0, 0);
}

__device__ inline uint32_t split_lo(float v0, float v1, uint32_t hi) {
  return pack_bf16x2(v0 - __uint_as_float(hi << 16), v1 - __uint_as_float(hi & 0xffff0000u));
}
// relu + bf16 pack (Single) or hi / lo split (Split) of 8 accumulator registers: element e of the B fragment = register r0 + e
template <class Op>
__device__ inline Op relu_frag(const f32x16_t& a, int r0) {
  u32x4_t uh, ul;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float v0 = fmaxf(a[r0 + 2 * q], 0.f), v1 = fmaxf(a[r0 + 2 * q + 1], 0.f);
    uh[q] = pack_bf16x2(v0, v1);
    ul[q] = split_lo(v0, v1, uh[q]);
  }
  return Op::from(uh, ul);
}

__device__ inline f32x16_t bias16(const float* b, int h) {  // accumulator register 4i+j <-> row 8i + 4h + j
  f32x16_t a;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4_t v = *(const f32x4_t*)(b + 8 * i + 4 * h);
    a[4 * i + 0] = v[0]; a[4 * i + 1] = v[1]; a[4 * i + 2] = v[2]; a[4 * i + 3] = v[3];
  }
  return a;
}
