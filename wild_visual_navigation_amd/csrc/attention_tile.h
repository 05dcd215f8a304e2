// The tile scheme the matrix-pipe attention kernels share (attention_bf16.hip: 16-bit operands; attention_x3.hip: hi + lo bf16
// planes); attention_bf16.hip's header comment describes it.  One workgroup = 128 queries of one (frame, head), 4 waves x 32
// queries, K / V^T tiles of 64 keys in an XOR-swizzled LDS ring, everything transposed: lane l holds query l & 31.  Whoever
// changes the key mask, the swizzle or the V^T token permutation changes it here, for both kernels.
// Every piece is __forceinline__, takes its arguments by value where it can and was checked to leave the compiled kernels as they
// were (profiles/attention_refactor.md: which forms did, which did not).
#pragma once
#include "split_operand.h"

constexpr int QB = 128;                   // queries per workgroup (4 waves x 32)
constexpr int KVB = 64;                   // keys per tile
constexpr int DH = 64;                    // head dim
constexpr int TILE_BYTES = KVB * DH * 2;  // 8 KB (K tile; V^T tile is the same size)

// The softmax is bounded by per-wave VALU issue, so instruction count matters: the row max uses 3-input max.
// The attention units are compiled with -fno-honor-nans so that fmaxf on MFMA results needs no canonicalising v_max (scores
// are finite; masking uses -1e30, not infinities).  NOT inline asm: hipcc pads no MFMA-result hazards for an asm
// statement's operands (a v_max3 in asm read accumulator registers before the MFMA had written them).
__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// ---- which (frame, head) pair bh and which 128-query block qb a workgroup serves --------------------------------------------
// XCDMAP (nbh % 8 == 0, checked by the launchers): the dispatcher puts workgroup b on XCD b % 8, so the 1-D grid is decoded
// such that all query blocks of a (frame, head) land on one XCD, consecutively.  Speed only: the arithmetic is the same.
struct AttnBlock { int bh, qb; };
template <bool XCDMAP>
__device__ __forceinline__ AttnBlock attn_block(int nqb) {
  AttnBlock w;
  if constexpr (XCDMAP) {
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    w.bh = (idx / nqb) * 8 + xcd;
    w.qb = idx % nqb;
  } else {
    w.bh = blockIdx.x / nqb;
    w.qb = blockIdx.x - w.bh * nqb;
  }
  return w;
}

// ---- K / V^T DMA: per tile (and plane) 8 wave-instructions of 1 KB (8 rows x 128 B); each wave issues 2 ----------------------
// The per-lane SOURCE byte offsets of one instruction: row = (wave * 2 + u) * 8 + (lane >> 3) is the key (K tile) or d (V^T
// tile) the lane fetches 16 bytes of.  The DMA writes lane-linear, so the chunk that lands in LDS chunk lane & 7 of its row is
// the source chunk (lane & 7) ^ ((row >> 1) & 7).  The tile's own offset is the scalar part of the load: + kv0 * 128 bytes for
// K ([npad][64]), + kv0 * 2 for V^T ([64][npad]).  (The caller forms row: it knows the range of wave and lane, and the
// optimiser simplifies this function before it sees the caller.)
struct AttnDmaOffset { unsigned k, v; };
__device__ __forceinline__ AttnDmaOffset attn_dma_offset(int bh, int npad, int row, int lane) {
  const int chunk = (lane & 7) ^ ((row >> 1) & 7);           // source chunk that lands in LDS chunk lane & 7
  return {(unsigned)((((size_t)bh * npad + row) * DH + chunk * 8) * 2), (unsigned)((((size_t)bh * DH + row) * npad + chunk * 8) * 2)};
}

// per-lane read offset of fragment s inside a tile: row l31 (+32 per sub-tile), chunk 2 s + hi XOR key (row >> 1) & 7 (same for row+32)
__device__ __forceinline__ unsigned attn_read_offset(int l31, int hi, int s) {
  const unsigned rd_row = l31 * 128;
  const int xorc = (l31 >> 1) & 7;
  return rd_row + (((2 * s + hi) ^ xorc) << 4);
}

// four per-lane addresses per tile (stage base + swizzled chunk of row l31); every fragment read of the tile is one of them
// plus an immediate (K sub-tile +4096, the next plane or V^T +TILE_BYTES ...).  Opaque to the optimiser, which otherwise
// re-derives an address per ds_read (16 v_add3_u32 per tile).
__device__ __forceinline__ void attn_tile_addresses(const unsigned (&rdo)[4], unsigned so, unsigned (&fa)[4]) {
  asm volatile("" : "+s"(so));  // keep the stage offset a scalar: one v_add per address, no loop-carried vector adds
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    fa[s] = rdo[s] + so;
    asm volatile("" : "+v"(fa[s]));
  }
}

// ---- Q^T fragments (B operand): qg points at query l31, d = 8 hi; fragment s holds d = 16 s + 8 hi .. + 7 --------------------
template <class Frag, class T>
__device__ __forceinline__ void attn_load_q(const T* qg, Frag (&qf)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *(const Frag*)(qg + s * 16);
}
// Make a Q fragment "used" where this is called, right after the loads: otherwise hipcc places their vmcnt wait at the first
// use INSIDE the tile loop, where it would also drain the K/V DMA queue on every trip.
template <class Frag>
__device__ __forceinline__ Frag attn_used(Frag f) {
  asm volatile("" : "+v"(f));
  return f;
}

// ---- which key of a 32-key sub-tile S^T accumulator register r of half-wave hi holds ------------------------------------------
__device__ __forceinline__ int attn_key_of(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ---- the tail of the last tile: keys >= ntok are neutralised by a select on their scores (p = 0) ----------------------------
// one sub-tile, whose first key is key0 = kv0 + 32 t
__device__ __forceinline__ f32x16_t attn_mask_tail(f32x16_t s, int key0, int ntok, int hi) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int key = key0 + attn_key_of(r, hi);
    if (key >= ntok) s[r] = -1e30f;
  }
  return s;
}

// ---- row max of a tile: 16 three-input max (two independent chains), then the other half-wave's ------------------------------
__device__ __forceinline__ float attn_row_max(const f32x16_t (&st)[2]) {
  float ma = max3f(st[0][0], st[0][1], st[0][2]), mb = max3f(st[1][0], st[1][1], st[1][2]);
  ma = max3f(ma, st[0][3], st[0][4]); mb = max3f(mb, st[1][3], st[1][4]);
#pragma unroll
  for (int r = 5; r < 15; r += 2) { ma = max3f(ma, st[0][r], st[0][r + 1]); mb = max3f(mb, st[1][r], st[1][r + 1]); }
  float mt = max3f(ma, mb, st[0][15]);
  mt = fmaxf(mt, st[1][15]);
  // the other half-wave's max of the same query: v_permlane32_swap (VALU) instead of a ds_bpermute LDS round trip
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mt), __float_as_uint(mt), false, false);
  return max3f(mt, __uint_as_float(sw[0]), __uint_as_float(sw[1]));  // one of the two is this lane's own value
}

// Deferred rescale: the running max only follows when some row's scores outgrow it by more than THR (in
// exp2 units).  P is then bounded by 2^THR instead of 1 -- harmless in fp32 accumulators, and P / l cancel
// exactly the same factor -- and the wave-uniform O rescale almost never runs after the first tiles.
constexpr float ATTN_THR = 6.0f;

// raw q: scores in the caller's units, c_exp = scale * log2(e)
__device__ __forceinline__ void attn_rescale_raw(float mt, float c_exp, float& m_run, float& l_run, float& l_run1, f32x16_t (&ot)[2]) {
  if (__any((mt - m_run) * c_exp > ATTN_THR)) {
    const float m_new = fmaxf(m_run, mt);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c_exp);
    m_run = m_new;
    l_run *= alpha;
    l_run1 *= alpha;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) ot[dt][r] *= alpha;
  }
}

// 1 / (the row sum): the two chains of the lane plus the other half-wave's
__device__ __forceinline__ float attn_inv_row_sum(float l_run, float l_run1) {
  l_run += l_run1;
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  return 1.0f / l_tot;
}

// a pair of floats as hi + lo bf16 pairs (a in bits 0..15): hi = bf16(v), lo = bf16(v - hi).  The two words come back as
// SCALARS for the caller to put into its fragment vector (the residue is formed from the scalar hi, not from the vector
// element it was stored to: clang's bit_cast of a vector element reads element 0).
struct Bf16Split { uint32_t hi, lo; };
__device__ __forceinline__ Bf16Split attn_split_bf16x2(float a, float c) {
  const uint32_t hw = pack_bf16x2(a, c);
  return {hw, split_lo(a, c, hw)};
}
