// Anomaly detection: the forward pass of the LinearRnvp flow (model/linear_rnvp.py:216-296) as the live node runs it with
// params.model.name == "LinearRnvp" (wvn_feature_extractor_node.py:319-344), on every segment row or every pixel of a frame:
//
//   per coupling layer f (mask m, networks S_f, T_f: D -> h -> h -> D, ReLU after the first two linears):
//     mu = u*m;  s = tanh(S(mu));  t = T(mu);  x = mu + (1-m)*(u*exp(s) + t);  log_det += sum((1-m)*s);  then x = x[:, p_f]
//   score = sum_c(-z_c^2 / 2 - log sqrt(2 pi)) + log_det                       (loss.py:42, unit normal prior)
//
// One kernel body, rnvp_kernel<D, HB>, holds both coupling layers, with two row sources: rows x [R][D], or pixels whose row is the
// align_corners=True bilinear blend of four fp32 tokens (common.h: lerp_scale / lerp_tap / bilerp_fixed), formed in the prologue --
// the dense [H*W][D] tensor (308 MB at 448^2) is never written.
//
//   * A workgroup (8 waves) owns a tile of 32 rows.  The tile's current vector u lives in LDS in fp32, in the ORIGINAL column order
//     for the whole chain: a permutation only renames columns, so it is folded into the packed images (wvn_rnvp_pack): flow 1's
//     mask, weight columns / rows and biases are looked up through p_0, and z is un-permuted once, when it is stored (the score is
//     a sum over all columns and needs no order).
//   * Only the m = 1 columns feed the networks and only the m = 0 columns use their outputs, so layer 1 runs over K = D/2 and
//     layer 3 over N = D/2 (the masks have D/2 ones; "odds" and "half" are both just column lists here):
//     2 * 200 * 192 + 200 * 200 = 116,800 MAC per network and row instead of 193,600.
//   * Products are transposed (out^T [channels x rows] = W [channels x k] * act^T [k x rows], lane = row), so the accumulator layout
//     of one layer is the B-operand layout of the next up to a fixed permutation of k that is folded into the packed images; the
//     hidden activations pass from layer to layer through LDS as ready-made hi / lo B fragments (16-byte, conflict-free accesses).
//   * Accuracy target is the fp32 reference, not a speed mode: every operand is split into hi + lo bf16 (v = hi + lo to 16 mantissa
//     bits) and every product is hi*hi + hi*lo + lo*hi with fp32 accumulation (split_operand.h), tanh / exp and the coupling in fp32.
//   * The weight images (D = 384, h = 200: 266 fragments of 1 KB per network and part, 2.1 MB for 4 networks x hi + lo) cannot live
//     in LDS; each wave reads the A fragments of its own output block straight from the packed blob (L2-resident, the same for every
//     workgroup), fully unrolled so that the loads run ahead of the MFMAs.  A wave owns one 32-channel output block for all 32 rows,
//     so every fragment is read once per workgroup and tile: 2.1 MB per 32 rows.
//
// Per tile and flow (barriers between the steps):  gather + split the m = 1 columns -> XA | layer 1, s and t (2 HB units over 8
// waves) -> HA, HB | layer 2 of s: HA -> HC | layer 2 of t: HB -> HA | layer 3 of s and t for one 32-column block per wave, then
// the coupling on u in place and the block's log_det partial.  MFMAs per 32 rows at D = 384, h = 200 (HB = 7 blocks of 32):
// 2 flows x 3 x (14 x 12 + 14 x 14 + 12 x 14) = 3,192.
//
// Budget (D = 384, HB = 8, the largest): LDS u 384 x 33 x 4 = 50,688 + three fragment buffers 3 x 32,768 + taps 1,024 + log_det
// partials 3,072 + score partials 2,048 = 155,136 bytes of the CU's 160 KB: one workgroup of 512 threads per CU, two waves per SIMD,
// up to 256 registers each, no scratch.  log_det and the score are summed in one fixed order: a row's outputs do not depend on R,
// on the row's position or on which outputs were requested.
#include "common.h"
#include "mlp_device.h"
#include "split_operand.h"
#include "wvn_internal.h"

namespace {

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

struct RnvpK {
  const unsigned char* blob;
  const float* x; int ldx;
  const float* tok; int ldt, G, Ho, Wo;
  float sy, sx;
  long long R;
  float mean, std, std_factor; const float* conf_dev;
  float* score; float* conf; float* log_det; float* z; int ldz;
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

template <int D, int HB>
__global__ __launch_bounds__(NTHR, 1) void rnvp_kernel(RnvpK p) {
  using G = Geo<D, HB>;
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
      }
      __syncthreads();
      // ---- layer 2 of s: bufA -> bufC, then of t: bufB -> bufA
#pragma unroll 1
      for (int net = 0; net < 2; ++net) {
        if (wave < HB) {
          const int nb = wave;
          f32x16_t acc = bias16(bias_f + net * G::NBIAS_NET + 32 * HB + 32 * nb, h);
          gemm_block<G::KH>(acc, img_f + (size_t)(net * G::NET_FRAGS + HB * G::KA + nb * G::KH) * FRAG, G::IMG_BYTES,
                            (net ? bufB : bufA) + lane * 16, G::HPLANE);
          store_hidden(net ? bufA : bufC, G::HPLANE, nb, lane, acc);
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
    __syncthreads();   // U, the taps and the partial sums are free for the next tile
  }
}

// ---- packing.  Flow f numbers its columns after the permutations before it: column j of flow 1 is column p_0[j] of u.
__device__ inline int clamp_col(long long v, int D) { return v < 0 ? 0 : (v >= D ? D - 1 : (int)v); }   // a corrupt permutation cannot address past u

template <int D, int HB>
__global__ void rnvp_tables_kernel(const float* __restrict__ mask, const long long* __restrict__ perm, unsigned char* __restrict__ out) {
  using G = Geo<D, HB>;
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int* chanA = (int*)(out + G::OFF_CHAN_A);
  int* chanB = (int*)(out + G::OFF_CHAN_B);
  int* colA = (int*)(out + G::OFF_COL_A);
  int* colB = (int*)(out + G::OFF_COL_B);
  int* zsrc = (int*)(out + G::OFF_ZSRC);
  for (int f = 0; f < NFLOW; ++f) {
    int a = 0, b = 0;
    for (int j = 0; j < D; ++j) {
      const int chan = f == 0 ? j : clamp_col(perm[j], D);
      if (mask[f * D + j] != 0.f) {
        if (a < G::NSLOT) { colA[f * G::NSLOT + a] = j; chanA[f * G::NSLOT + a] = chan; ++a; }
      } else {
        if (b < G::NSLOT) { colB[f * G::NSLOT + b] = j; chanB[f * G::NSLOT + b] = chan; ++b; }
      }
    }
    for (; a < G::NSLOT; ++a) colA[f * G::NSLOT + a] = chanA[f * G::NSLOT + a] = -1;
    for (; b < G::NSLOT; ++b) colB[f * G::NSLOT + b] = chanB[f * G::NSLOT + b] = -1;
  }
  for (int j = 0; j < G::DP; ++j) zsrc[j] = j < D ? clamp_col(perm[clamp_col(perm[D + j], D)], D) : 0;   // z[:, j] = x1[:, p_1[j]], x1[:, i] = u[:, p_0[i]]
}

// params: per flow, per network: W1 [h][D] | b1 [h] | W2 [h][h] | b2 [h] | W3 [D][h] | b3 [D]
template <int D, int HB>
__global__ void rnvp_pack_kernel(const float* __restrict__ prm, int h, unsigned char* __restrict__ out) {
  using G = Geo<D, HB>;
  const int* colA = (const int*)(out + G::OFF_COL_A);
  const int* colB = (const int*)(out + G::OFF_COL_B);
  const size_t net_params = (size_t)h * D + h + (size_t)h * h + h + (size_t)D * h + D;
  const int gsz = gridDim.x * blockDim.x, g0 = blockIdx.x * blockDim.x + threadIdx.x;
  bf16_t* imgh = (bf16_t*)(out + G::OFF_IMG);
  bf16_t* imgl = (bf16_t*)(out + G::OFF_IMG + G::IMG_BYTES);
  for (int i = g0; i < G::IMG_BYTES / 2; i += gsz) {
    const int e = i & 7, m = (i >> 3) & 31, hh = (i >> 8) & 1;
    int fr = i >> 9;
    const int fn = fr / G::NET_FRAGS, f = fn >> 1;
    fr -= fn * G::NET_FRAGS;
    const float* W1 = prm + fn * net_params;
    const float* W2 = W1 + (size_t)h * D + h;
    const float* W3 = W2 + (size_t)h * h + h;
    float v = 0.f;
    if (fr < HB * G::KA) {
      const int nb = fr / G::KA, ks = fr - nb * G::KA;
      const int row = 32 * nb + m, j = colA[f * G::NSLOT + ks * 16 + 8 * hh + e];
      if (row < h && j >= 0) v = W1[(size_t)row * D + j];
    } else if (fr < HB * G::KA + HB * G::KH) {
      fr -= HB * G::KA;
      const int nb = fr / G::KH, ks = fr - nb * G::KH;
      const int row = 32 * nb + m, col = hidden_of(ks, hh, e);
      if (row < h && col < h) v = W2[(size_t)row * h + col];
    } else {
      fr -= HB * G::KA + HB * G::KH;
      const int nb = fr / G::KH, ks = fr - nb * G::KH;
      const int j = colB[f * G::NSLOT + 32 * nb + m], col = hidden_of(ks, hh, e);
      if (j >= 0 && col < h) v = W3[(size_t)j * h + col];
    }
    const bf16_t hi = f32_to_bf16(v);
    imgh[i] = hi;
    imgl[i] = f32_to_bf16(v - bf16_to_f32(hi));
  }
  float* bo = (float*)(out + G::OFF_BIAS);
  for (int i = g0; i < NFLOW * 2 * G::NBIAS_NET; i += gsz) {
    const int fn = i / G::NBIAS_NET, k = i - fn * G::NBIAS_NET, f = fn >> 1;
    const float* b1 = prm + fn * net_params + (size_t)h * D;
    const float* b2 = b1 + h + (size_t)h * h;
    const float* b3 = b2 + h + (size_t)D * h;
    float v = 0.f;
    if (k < 32 * HB) { if (k < h) v = b1[k]; }
    else if (k < 64 * HB) { if (k - 32 * HB < h) v = b2[k - 32 * HB]; }
    else { const int j = colB[f * G::NSLOT + k - 64 * HB]; if (j >= 0) v = b3[j]; }
    bo[i] = v;
  }
}

// ---- host side
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

int rnvp_num_cus() {
  int dev = 0;
  hipDeviceProp_t pr;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
    return pr.multiProcessorCount;
  return 256;
}

template <int D, int HB>
int rnvp_launch(const RnvpCall& c, hipStream_t st) {
  using G = Geo<D, HB>;
  RnvpK k{};
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
  auto kern = rnvp_kernel<D, HB>;
  static LdsOptIn lds_opt_in;   // per device (common.h)
  if (const int rc = lds_opt_in(G::LDS_BYTES, (const void*)kern)) return rc;
  static const int cus = rnvp_num_cus();
  const long long ntiles = (c.R + TILE_ROWS - 1) / TILE_ROWS;
  hipLaunchKernelGGL(kern, dim3((unsigned)(ntiles < cus ? ntiles : cus)), dim3(NTHR), G::LDS_BYTES, st, k);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // namespace

bool wvn_rnvp_supported(int D, int h, int flows) { return (D == 384 || D == 90) && h >= 1 && h <= 256 && flows == NFLOW; }
int wvn_rnvp_row_tile_impl() { return TILE_ROWS; }
size_t wvn_rnvp_pack_bytes_impl(int D, int h) {
  return dispatch(D, h, [](auto s) { return (size_t)Geo<decltype(s)::d, decltype(s)::hb>::BLOB_BYTES; });
}
int wvn_rnvp_pack_launch(int D, int h, const float* params, const float* mask, const long long* perm, void* packed, hipStream_t st) {
  if (!wvn_rnvp_supported(D, h, NFLOW)) return WVN_ERR_ARG;
  dispatch(D, h, [&](auto s) {
    constexpr int d = decltype(s)::d, hb = decltype(s)::hb;
    hipLaunchKernelGGL((rnvp_tables_kernel<d, hb>), dim3(1), dim3(64), 0, st, mask, perm, (unsigned char*)packed);
    hipLaunchKernelGGL((rnvp_pack_kernel<d, hb>), dim3(256), dim3(256), 0, st, params, h, (unsigned char*)packed);
    return 0;
  });
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
int wvn_rnvp_forward_launch(const RnvpCall& c, hipStream_t st) {
  if (!wvn_rnvp_supported(c.D, c.h, NFLOW)) return WVN_ERR_ARG;
  return dispatch(c.D, c.h, [&](auto s) { return rnvp_launch<decltype(s)::d, decltype(s)::hb>(c, st); });
}
