// The 16-bit MFMA operand format of a translation unit.
//
// The speed path of wvn_vit_forward exists in two operand formats with identical kernels, instruction counts and matrix
// rates (v_mfma_f32_32x32x16_{bf16,f16}, v_cvt_pk_{bf16,f16}_f32, v_dot2c_f32_{bf16,f16}):
//   bf16 (WVN_PREC_BF16): 8 significand bits, fp32's exponent range -- no range analysis needed;
//   fp16 (WVN_PREC_F16) : 11 significand bits, 8x less operand rounding -- the form whose token error sits inside the
//                         north_star's parity budget; its range (65504, subnormals below 6.1e-5) is safe for this path:
//                         LayerNorm outputs, q / k / v, GELU outputs and softmax probabilities (<= 2^12 under the lazy running
//                         max, attention_bf16.hip) are O(1..1e3), and all accumulation, residuals and statistics stay fp32.
// Every source that includes this header is compiled twice by csrc/build.py (the second time with -DWVN_OPERAND_F16=1); its
// launchers are named through WVN_OPSYM so that both sets link into one library and vit_forward.hip picks by precision.  Storage in
// HBM / LDS is raw 16-bit words (op16_t) in both cases.
#pragma once
#include "common.h"

#ifndef WVN_OPERAND_F16
#define WVN_OPERAND_F16 0
#endif

typedef uint16_t op16_t;  // raw operand bits
#if WVN_OPERAND_F16
typedef _Float16 wvn_op_elem_t;
#define WVN_OPSYM(name) name##_f16
#define wvn_mfma_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_f16
#define WVN_OP_ONE2 0x3c003c00u  // packed {1.0, 1.0}
#else
typedef __bf16 wvn_op_elem_t;
#define WVN_OPSYM(name) name
#define wvn_mfma_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_bf16
#define WVN_OP_ONE2 0x3f803f80u
#endif
typedef __attribute__((ext_vector_type(8))) wvn_op_elem_t opx8_t;
typedef __attribute__((ext_vector_type(4))) wvn_op_elem_t opx4_t;
typedef __attribute__((ext_vector_type(2))) wvn_op_elem_t opx2_t;

// two floats -> packed operand pair (lo in bits 0..15), round-to-nearest-even by the hardware converter (v_cvt_pk_bf16_f32 /
// v_cvt_pk_f16_f32).  A builtin conversion, not inline asm: see pack_bf16x2 in common.h.
__device__ inline uint32_t pack_op2(float lo, float hi) { return WVN_OPERAND_F16 ? pack_f16x2(lo, hi) : pack_bf16x2(lo, hi); }
// acc + p.lo + p.hi of a packed operand pair (v_dot2c_f32_{bf16,f16} against packed ones)
__device__ inline float dot2_ones_op(uint32_t pk, float acc) {
  const opx2_t pp = __builtin_bit_cast(opx2_t, pk), one2 = __builtin_bit_cast(opx2_t, WVN_OP_ONE2);
#if WVN_OPERAND_F16
  return __builtin_amdgcn_fdot2(pp, one2, acc, false);
#else
  return __builtin_amdgcn_fdot2_f32_bf16(pp, one2, acc, false);
#endif
}
// scalar conversions (round-to-nearest-even; host and device)
__host__ __device__ inline op16_t f32_to_op(float f) { return WVN_OPERAND_F16 ? f32_to_f16(f) : f32_to_bf16(f); }
__host__ __device__ inline float op_to_f32(op16_t h) { return WVN_OPERAND_F16 ? f16_to_f32(h) : bf16_to_f32(h); }
