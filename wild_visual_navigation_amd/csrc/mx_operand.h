// The MX operand form of the mixed / exact route, stated once for its producers (the epilogues of gemm_a384_x3.hip, the output planes of
// attention_bf16.hip) and its consumers (gemm_n384_x3.hip, gemm_a384_x3.hip, the two-plane q of attention_bf16.hip):
//     h = fp16(v),   l8 = e5m2((v - h) * 2^12),   h8 = e5m2(v)   (of an activation: e5m2(h), derived in registers from the fp16 fragments)
// and  sum a w  ~=  sum a_h w_h  +  2^-12 (sum a_h8 w_l8 + sum a_l8 w_h8):  the first sum on fp16 MFMAs, the two correction products on
// v_mfma_scale_f32_32x32x64_f8f6f4.  e5m2 IS the top byte of an fp16, so the 8-bit planes need no block scales: the residues carry ONE
// constant factor 2^12, undone by the instruction's E8M0 scale operand.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) int i32x8_t;        // the 32 bytes a lane gives a K = 64 8-bit MFMA
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(2))) short mx_s16x2_t;   // the dword a pair conversion writes one half of

// E8M0 scale bytes 2^0 and 2^-12 (115 = 127 - 12).  Every byte of a scale operand is alike and every lane passes the same one, so the hardware's
// assignment of scale bytes to 32-k blocks (registers 0-3 of both half-waves = block 0, scripts/ubench/mx_formats.hip) and op_sel never matter.
constexpr int MX_SC_ONE = 0x7f7f7f7f, MX_SC_RES = 0x73737373;
// what the producers scale a residue by: v_cvt_scalef32_* DIVIDES by its scale operand (scripts/ubench/mx_formats.hip), so 2^-12 here is the
// 2^12 that MX_SC_RES undoes
constexpr float MX_RES_INV = 1.0f / 4096.0f;

// (a / inv_scale, b / inv_scale) as two e5m2 bytes into the low or high half of `old`
__device__ inline uint32_t mx_pk8(uint32_t old, float a, float b, float inv_scale, bool hi_word) {
  const mx_s16x2_t o = __builtin_bit_cast(mx_s16x2_t, old);
  return __builtin_bit_cast(uint32_t, hi_word ? __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(o, a, b, inv_scale, true)
                                              : __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(o, a, b, inv_scale, false));
}

// e5m2(x / inv_scale) of the four fp16 fragments of a 64-k step (h[s]: k-step s, eight values per lane) as the two 16-byte halves of the 8-bit
// operand: byte (s, j) = element j of k-step s.  inv_scale = 1 gives h8 of an operand's fp16 plane (sixteen v_cvt_scalef32_pk_bf8_f16 per lane);
// MX_RES_INV gives l8 of a residue that is held as fp16 (attention's q_lo).
__device__ __forceinline__ void mx_e5m2_of_f16(const u32x4_t* h, u32x4_t (&out)[2], float inv_scale = 1.0f) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    uint32_t d[2] = {0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t pr = h[s][e];   // (scalar copy: clang's bit_cast of a vector element reads element 0)
      const mx_s16x2_t o = __builtin_bit_cast(mx_s16x2_t, d[e >> 1]);
      d[e >> 1] = __builtin_bit_cast(uint32_t, (e & 1) ? __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(o, __builtin_bit_cast(wvn_f16x2_t, pr), inv_scale, true)
                                                       : __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(o, __builtin_bit_cast(wvn_f16x2_t, pr), inv_scale, false));
    }
    out[s >> 1][2 * (s & 1)] = d[0];
    out[s >> 1][2 * (s & 1) + 1] = d[1];
  }
}

// the two 16-byte halves of an 8-bit operand as the MFMA's eight dwords
__device__ __forceinline__ i32x8_t mx_pack(u32x4_t a, u32x4_t b) {
  return i32x8_t{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}

// acc += 2^-12 (w8 . a8), one of the two correction products of a 64-k step:
//     which = 0:  w8 = W_l8 (carries 2^12),  a8 = a_h8          which = 1:  w8 = W_h8,  a8 = a_l8 (carries 2^12)
// TR: the tile is held transposed (W rows are the MFMA's first operand, as in every fp16 / bf16 MFMA of the same tile); the scale operands
// follow their matrices.
template <bool TR>
__device__ __forceinline__ f32x16_t mx_correction(i32x8_t w8, i32x8_t a8, f32x16_t acc, int which) {
  const int sc_w = which ? MX_SC_ONE : MX_SC_RES, sc_a = which ? MX_SC_RES : MX_SC_ONE;
  if constexpr (TR) return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w8, a8, acc, 1, 1, 0, sc_w, 0, sc_a);
  else return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, w8, acc, 1, 1, 0, sc_a, 0, sc_w);
}
