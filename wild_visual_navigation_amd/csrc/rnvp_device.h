// The LinearRnvp flow on a 32-row tile, stated once for inference (rnvp.hip: rnvp_kernel<D, HB, false>) and for phase A of the
// training step (rnvp_train.hip: rnvp_kernel<D, HB, true>, which also writes what the backward pass needs to a workspace).
// The layout of the packed blob (Geo), of the training workspace (TrainGeo) and the fragment helpers live here too.
// See rnvp.hip for the kernel's structure and budget.
#pragma once
#include "common.h"
#include "mlp_device.h"
#include "split_operand.h"
#include "wvn_internal.h"

namespace rnvp {

constexpr int TILE_ROWS = 32;
constexpr int NTHR = 512, NWAVE = NTHR / 64;
constexpr int US = TILE_ROWS + 1;        // floats between two columns of u (33: column-major and row-major sweeps both spread over the banks)
constexpr int FRAG = 1024;               // one fragment: [2 lane halves][32][8 bf16]
constexpr int NFLOW = 2;
constexpr float HALF_LOG_2PI = 0.91893853320467274178f;

template <int D_, int HB_>
struct Geo {
  static constexpr int D = D_, HB = HB_;
  static constexpr int NB = (D / 2 + 31) / 32;        // 32-column blocks of either half (6 / 2)
  static constexpr int NSLOT = NB * 32;               // column slots of a half, the tail past D/2 is padding
  static constexpr int KA = 2 * NB, KH = 2 * HB;      // k-steps of layer 1, of layers 2 and 3
  static constexpr int DP = (D + 3) / 4 * 4;
  // packed blob: int tables | fp32 biases | hi images | lo images
  static constexpr int OFF_CHAN_A = 0;                          // [flow][slot] -> column of u that feeds the slot, or -1
  static constexpr int OFF_CHAN_B = OFF_CHAN_A + NFLOW * NSLOT * 4;   // [flow][slot] -> column of u the slot transforms, or -1
  static constexpr int OFF_COL_A = OFF_CHAN_B + NFLOW * NSLOT * 4;    // the same two in the flow's own (weight) column numbering
  static constexpr int OFF_COL_B = OFF_COL_A + NFLOW * NSLOT * 4;
  static constexpr int OFF_ZSRC = OFF_COL_B + NFLOW * NSLOT * 4;      // [D] column of u that is column j of z
  static constexpr int NBIAS_NET = 64 * HB + NSLOT;             // b1 | b2 (padded to 32 HB) | b3 in slot order
  static constexpr int OFF_BIAS = OFF_ZSRC + DP * 4;
  static constexpr int NET_FRAGS = HB * KA + HB * KH + NB * KH; // layer 1 [HB][KA] | layer 2 [HB][KH] | layer 3 [NB][KH]
  static constexpr int IMG_BYTES = NFLOW * 2 * NET_FRAGS * FRAG;
  static constexpr int OFF_IMG = OFF_BIAS + NFLOW * 2 * NBIAS_NET * 4;
  static constexpr size_t BLOB_BYTES = (size_t)OFF_IMG + 2 * (size_t)IMG_BYTES;
  // LDS
  static constexpr int HPLANE = KH * FRAG;                      // hi part of a fragment buffer; the lo part follows
  static constexpr int HBUF = 2 * HPLANE;
  static constexpr int L_U = 0;
  static constexpr int L_HA = (D * US * 4 + 15) / 16 * 16;
  static constexpr int L_HB = L_HA + HBUF;
  static constexpr int L_HC = L_HB + HBUF;                      // also XA, the split m = 1 columns (KA <= KH k-steps)
  static constexpr int L_TAP = L_HC + HBUF;                     // [32 rows]{4 token offsets, wx0, wx1, wy0, wy1}
  static constexpr int L_LD = L_TAP + TILE_ROWS * 32;           // [flow][NB][2][32] log_det partials
  static constexpr int L_SC = L_LD + NFLOW * NB * 2 * TILE_ROWS * 4;   // [16][32] score partials
  static constexpr int LDS_BYTES = L_SC + 16 * TILE_ROWS * 4;
  static_assert(KA <= KH, "XA shares the third fragment buffer");
  static_assert(OFF_BIAS % 16 == 0 && OFF_IMG % 16 == 0, "16-byte loads");
  static_assert(LDS_BYTES <= 160 * 1024, "one workgroup per CU");
};

// The training workspace: per 32-row tile, "channels" of 32 floats (one per row of the tile; 8 consecutive rows of a channel are
// one operand fragment of the weight-gradient products, whose contraction runs over rows).  Per flow: the network inputs XA (slot
// order), the hidden activations H1 / H2 and the gradients G1 / G2 / G3 of the three linears' outputs for the s (0) and t (1)
// networks, s = tanh(.) and u_in of the transformed columns (slot order); behind the two flows the tile's final u (column order).
template <int D, int HB>
struct TrainGeo {
  using G = Geo<D, HB>;
  static constexpr int HC = 32 * HB;
  static constexpr int C_XA = 0;
  static constexpr int C_H1 = C_XA + G::NSLOT;      // [net][HC]
  static constexpr int C_H2 = C_H1 + 2 * HC;
  static constexpr int C_S = C_H2 + 2 * HC;
  static constexpr int C_UIN = C_S + G::NSLOT;
  static constexpr int C_G3 = C_UIN + G::NSLOT;     // [net][NSLOT]
  static constexpr int C_G2 = C_G3 + 2 * G::NSLOT;  // [net][HC]
  static constexpr int C_G1 = C_G2 + 2 * HC;
  static constexpr int FLOW_CH = C_G1 + 2 * HC;
  static constexpr int C_Z = NFLOW * FLOW_CH;
  static constexpr int TILE_CH = C_Z + D;
  static constexpr size_t TILE_FLOATS = (size_t)TILE_CH * TILE_ROWS;
};

struct RnvpK {
  const unsigned char* blob;
  const float* x; int ldx;
  const float* tok; int ldt, G, Ho, Wo;
  float sy, sx;
  long long R;
  float mean, std, std_factor; const float* conf_dev;
  float* score; float* conf; float* log_det; float* z; int ldz;
  float* ws;   // the training workspace (TRAIN kernels only)
};

// hidden unit held by slot (h, e) of k-step ks: what the accumulator layout of the producing 32-row block makes it
__host__ __device__ inline int hidden_of(int ks, int h, int e) { return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (e >> 2) + 4 * h + (e & 3); }

__device__ inline void split8(const float (&v)[8], u32x4_t& uh, u32x4_t& ul) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uh[q] = pack_bf16x2(v[2 * q], v[2 * q + 1]);
    ul[q] = split_lo(v[2 * q], v[2 * q + 1], uh[q]);
  }
}

// acc += W[block][:] * act for NK k-steps: A fragments from the packed blob (wf: this lane's 16 bytes of the block's first
// fragment, lo part lo_off behind), B fragments from an LDS fragment buffer (bl: this lane's 16 bytes of k-step 0)
template <int NK>
__device__ inline void gemm_block(f32x16_t& acc, const unsigned char* wf, int lo_off, const unsigned char* bl, int plane) {
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) mma(acc, Split::load(wf + ks * FRAG, lo_off), Split::load(bl + ks * FRAG, plane));
}

// relu(acc) of output block nb -> k-steps 2 nb, 2 nb + 1 of a fragment buffer
__device__ inline void store_hidden(unsigned char* buf, int plane, int nb, int lane, const f32x16_t& acc) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const Split f = relu_frag<Split>(acc, 8 * u);
    unsigned char* dst = buf + (2 * nb + u) * FRAG + lane * 16;
    *(bf16x8_t*)dst = f.hi;
    *(bf16x8_t*)(dst + plane) = f.lo;
  }
}

// channel of a 32-channel block that accumulator register r of lane half h holds
__device__ inline int acc_chan(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

template <int D, int HB, bool TRAIN>
__global__ __launch_bounds__(NTHR, 1) void rnvp_kernel(RnvpK p) {
  using G = Geo<D, HB>;
  using T = TrainGeo<D, HB>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* U = (float*)(smem + G::L_U);
  unsigned char* bufA = smem + G::L_HA;
  unsigned char* bufB = smem + G::L_HB;
  unsigned char* bufC = smem + G::L_HC;
  int* tapi = (int*)(smem + G::L_TAP);
  float* LD = (float*)(smem + G::L_LD);
  float* SC = (float*)(smem + G::L_SC);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 31, h = lane >> 5;
  const int* chanA = (const int*)(p.blob + G::OFF_CHAN_A);
  const int* chanB = (const int*)(p.blob + G::OFF_CHAN_B);
  const int* zsrc = (const int*)(p.blob + G::OFF_ZSRC);
  const float* biases = (const float*)(p.blob + G::OFF_BIAS);
  const unsigned char* img = p.blob + G::OFF_IMG + lane * 16;
  const int ntiles = (int)((p.R + TILE_ROWS - 1) / TILE_ROWS);

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long r0 = (long long)tile * TILE_ROWS;
    float* wst = TRAIN ? p.ws + (size_t)tile * T::TILE_FLOATS : nullptr;
    // ---- the tile's rows -> U [column][row]; rows past R are zeros (finite, never stored)
    if (p.x) {
      for (int i = tid; i < TILE_ROWS * D; i += NTHR) {
        const int rr = i / D, c = i - rr * D;
        U[c * US + rr] = r0 + rr < p.R ? p.x[(size_t)(r0 + rr) * p.ldx + c] : 0.f;
      }
    } else {
      if (tid < TILE_ROWS) {
        const long long r = r0 + tid < p.R ? r0 + tid : p.R - 1;
        const int hw = p.Ho * p.Wo;
        const int b = (int)(r / hw), q = (int)(r - (long long)b * hw);
        const int y = q / p.Wo, xo = q - y * p.Wo;
        const LerpTap ty = lerp_tap(y, p.G, p.sy), tx = lerp_tap(xo, p.G, p.sx);
        const int y0 = min(ty.i0, p.G - 1), y1 = min(ty.i1, p.G - 1), x0 = min(tx.i0, p.G - 1), x1 = min(tx.i1, p.G - 1);
        const int base = b * p.G * p.G;
        int* t = tapi + tid * 8;
        t[0] = base + y0 * p.G + x0; t[1] = base + y0 * p.G + x1; t[2] = base + y1 * p.G + x0; t[3] = base + y1 * p.G + x1;
        float* w = (float*)(t + 4);
        w[0] = tx.w0; w[1] = tx.w1; w[2] = ty.w0; w[3] = ty.w1;
      }
      __syncthreads();
      for (int i = tid; i < TILE_ROWS * D; i += NTHR) {
        const int rr = i / D, c = i - rr * D;
        const int* t = tapi + rr * 8;
        const float* w = (const float*)(t + 4);
        U[c * US + rr] = bilerp_fixed(p.tok[(size_t)t[0] * p.ldt + c], p.tok[(size_t)t[1] * p.ldt + c], p.tok[(size_t)t[2] * p.ldt + c],
                                      p.tok[(size_t)t[3] * p.ldt + c], w[0], w[1], w[2], w[3]);
      }
    }
    __syncthreads();

#pragma unroll 1
    for (int f = 0; f < NFLOW; ++f) {
      float* wsf = TRAIN ? wst + (size_t)f * T::FLOW_CH * TILE_ROWS : nullptr;
      // ---- the m = 1 columns, split into hi / lo B fragments: XA (in the third buffer), slot a = 16 ks + 8 h + e
      for (int it = tid; it < G::KA * 64; it += NTHR) {
        const int ks = it >> 6, l = it & 63;
        const int* ca = chanA + f * G::NSLOT + ks * 16 + (l >> 5) * 8;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { const int c = ca[e]; v[e] = c >= 0 ? U[c * US + (l & 31)] : 0.f; }
        u32x4_t uh, ul;
        split8(v, uh, ul);
        *(u32x4_t*)(bufC + ks * FRAG + l * 16) = uh;
        *(u32x4_t*)(bufC + G::HPLANE + ks * FRAG + l * 16) = ul;
        if constexpr (TRAIN) {
#pragma unroll
          for (int e = 0; e < 8; ++e) wsf[(T::C_XA + ks * 16 + (l >> 5) * 8 + e) * TILE_ROWS + (l & 31)] = v[e];
        }
      }
      __syncthreads();
      const float* bias_f = biases + f * 2 * G::NBIAS_NET;
      const unsigned char* img_f = img + (size_t)f * 2 * G::NET_FRAGS * FRAG;
      // ---- layer 1 of s (units 0 .. HB-1 -> bufA) and of t (units HB .. 2 HB - 1 -> bufB)
      for (int u = wave; u < 2 * HB; u += NWAVE) {
        const int net = u >= HB, nb = u - net * HB;
        f32x16_t acc = bias16(bias_f + net * G::NBIAS_NET + 32 * nb, h);
        gemm_block<G::KA>(acc, img_f + (size_t)(net * G::NET_FRAGS + nb * G::KA) * FRAG, G::IMG_BYTES, bufC + lane * 16, G::HPLANE);
        store_hidden(net ? bufB : bufA, G::HPLANE, nb, lane, acc);
        if constexpr (TRAIN) {
#pragma unroll
          for (int r = 0; r < 16; ++r) wsf[(T::C_H1 + net * T::HC + 32 * nb + acc_chan(r, h)) * TILE_ROWS + n] = fmaxf(acc[r], 0.f);
        }
      }
      __syncthreads();
      // ---- layer 2 of s: bufA -> bufC, then of t: bufB -> bufA
#pragma unroll 1
      for (int net = 0; net < 2; ++net) {
        if (wave < HB) {
          const int nb = wave;
          f32x16_t acc = bias16(bias_f + net * G::NBIAS_NET + 32 * HB + 32 * nb, h);
          gemm_block<G::KH>(acc, img_f + (size_t)(net * G::NET_FRAGS + HB * G::KA + nb * G::KH) * FRAG, G::IMG_BYTES,
                            smem + (net ? G::L_HB : G::L_HA) + lane * 16, G::HPLANE);
          store_hidden(smem + (net ? G::L_HA : G::L_HC), G::HPLANE, nb, lane, acc);   // (LDS offsets, not a choice of pointers: the
                                                                                       //  compiler then keeps the address space)
          if constexpr (TRAIN) {
#pragma unroll
            for (int r = 0; r < 16; ++r) wsf[(T::C_H2 + net * T::HC + 32 * nb + acc_chan(r, h)) * TILE_ROWS + n] = fmaxf(acc[r], 0.f);
          }
        }
        __syncthreads();
      }
      // ---- layer 3 of s (from bufC) and t (from bufA), one 32-slot block of the m = 0 columns per wave, and the coupling
      if (wave < G::NB) {
        const int nb = wave;
        f32x16_t as = bias16(bias_f + 64 * HB + 32 * nb, h);
        f32x16_t at = bias16(bias_f + G::NBIAS_NET + 64 * HB + 32 * nb, h);
        const size_t w3 = (size_t)(HB * G::KA + HB * G::KH + nb * G::KH) * FRAG;
        gemm_block<G::KH>(as, img_f + w3, G::IMG_BYTES, bufC + lane * 16, G::HPLANE);
        gemm_block<G::KH>(at, img_f + (size_t)G::NET_FRAGS * FRAG + w3, G::IMG_BYTES, bufA + lane * 16, G::HPLANE);
        float ld = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int* cb = chanB + f * G::NSLOT + 32 * nb + 8 * i + 4 * h;   // accumulator register 4i+j <-> slot 8i + 4h + j
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = cb[j];
            if (c >= 0) {
              const float s = tanhf(as[4 * i + j]);
              float* up = U + c * US + n;
              if constexpr (TRAIN) {
                wsf[(T::C_S + 32 * nb + 8 * i + 4 * h + j) * TILE_ROWS + n] = s;
                wsf[(T::C_UIN + 32 * nb + 8 * i + 4 * h + j) * TILE_ROWS + n] = *up;
              }
              *up = fmaf(*up, expf(s), at[4 * i + j]);
              ld += s;
            }
          }
        }
        LD[((f * G::NB + nb) * 2 + h) * TILE_ROWS + n] = ld;
      }
      __syncthreads();
    }

    // ---- score: 16 partial sums of -u^2/2 per row, then one thread per row
    {
      const int rr = tid & 31, g = tid >> 5;
      float a = 0.f;
      for (int c = g; c < D; c += 16) { const float v = U[c * US + rr]; a = fmaf(-0.5f * v, v, a); }
      SC[g * TILE_ROWS + rr] = a;
    }
    __syncthreads();
    if (tid < TILE_ROWS && r0 + tid < p.R) {
      float a = 0.f, ld = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) a += SC[g * TILE_ROWS + tid];
#pragma unroll
      for (int k = 0; k < NFLOW * G::NB * 2; ++k) ld += LD[k * TILE_ROWS + tid];
      const float sc = (a - (float)D * HALF_LOG_2PI) + ld;
      const size_t r = (size_t)(r0 + tid);
      p.score[r] = sc;
      if (p.log_det) p.log_det[r] = ld;
      if (p.conf) {
        const float cm = p.conf_dev ? p.conf_dev[0] : p.mean, cs = p.conf_dev ? p.conf_dev[1] : p.std;
        const float cf = p.conf_dev ? p.conf_dev[2] : p.std_factor;
        p.conf[r] = confidence_of_nan(-sc, cm, cs, cf);
      }
    }
    if (p.z) {
      for (int i = tid; i < TILE_ROWS * D; i += NTHR) {
        const int rr = i / D, j = i - rr * D;
        if (r0 + rr < p.R) p.z[(size_t)(r0 + rr) * p.ldz + j] = U[zsrc[j] * US + rr];
      }
    }
    if constexpr (TRAIN) {   // the final u in column order: the seed of the backward pass is -u / N
      for (int i = tid; i < TILE_ROWS * D; i += NTHR) wst[(size_t)T::C_Z * TILE_ROWS + i] = U[(i >> 5) * US + (i & 31)];
    }
    __syncthreads();   // U, the taps and the partial sums are free for the next tile
  }
}

template <int D, int HB> struct Shape { static constexpr int d = D, hb = HB; };
// f(Shape<D, HB>{}) for a supported (D, h); a zero of f's result type for anything else.  HB: h padded to 7 or 8 blocks of 32
template <class Fn>
auto dispatch(int D, int h, Fn f) -> decltype(f(Shape<384, 7>{})) {
  if (h < 1 || h > 256) return decltype(f(Shape<384, 7>{})){};
  const bool wide = h > 224;
  if (D == 384) return wide ? f(Shape<384, 8>{}) : f(Shape<384, 7>{});
  if (D == 90) return wide ? f(Shape<90, 8>{}) : f(Shape<90, 7>{});
  return decltype(f(Shape<384, 7>{})){};
}

// the call's fields -> kernel arguments; WVN_ERR_ARG for a pixel source whose token count does not fit an int
inline int fill_args(const RnvpCall& c, RnvpK& k) {
  k.blob = (const unsigned char*)c.packed;
  k.x = c.x; k.ldx = c.ldx;
  k.tok = c.tokens; k.ldt = c.ldt; k.G = c.G; k.Ho = c.Ho; k.Wo = c.Wo;
  if (!c.x) {
    if ((long long)c.B * c.G * c.G > 0x7fffffffll) return WVN_ERR_ARG;
    k.sy = lerp_scale(c.G, c.Ho); k.sx = lerp_scale(c.G, c.Wo);
  }
  k.R = c.R;
  k.mean = c.mean; k.std = c.std; k.std_factor = c.std_factor; k.conf_dev = c.conf_dev;
  k.score = c.score; k.conf = c.conf; k.log_det = c.log_det; k.z = c.z; k.ldz = c.ldz;
  return WVN_OK;
}

}  // namespace rnvp
