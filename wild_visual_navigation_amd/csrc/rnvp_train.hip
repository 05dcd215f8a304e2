// Anomaly detection: one optimisation step of the LinearRnvp flow (AnomalyLoss: loss = -mean(score), torch.optim.Adam), in three
// phases with the two data-parallel exchanges between them, as the traversability MLPs train (mlp_train.hip, trainer.py):
//
//   phase A  rnvp_kernel<D, HB, true> (rnvp_device.h): the forward flow of rnvp.hip on this rank's rows, which also writes what the
//            backward pass needs to a workspace (TrainGeo: network inputs, h1, h2, s = tanh(.), u_in, the final u), and
//            rnvp_stat_kernel: {n, sum x, sum x^2, n} of x = -score in fp64           -> all-reduce of 4 doubles
//   phase B  clear the flat gradient | rnvp_bwd_kernel: per 32-row tile, flow 1 then flow 0, the gradients G3, G2, G1 of the
//            three linears' outputs for t and s | rnvp_wgrad_kernel: dW_l = G_l^T A_{l-1} and the bias gradients
//                                                                                       -> all-reduce of the flat gradient
//   phase C  Adam (mlp.hip) | loss + commit of the confidence statistic (mlp_device.h: conf_commit) | re-pack of the forward
//            images (rnvp.hip) and of the transposed ones (here)
//   Launches: 2 + 3 + 5 = 10 for any row count.
//
// Arithmetic as in the forward kernel: every matrix product takes hi + lo bf16 split operands (hi*hi + hi*lo + lo*hi, fp32
// accumulation: split_operand.h); tanh, exp, the coupling and their derivatives are fp32; permutations and masks are the column
// tables of the packed blob, so layer 1 is differentiated over K = D/2 and layer 3 over N = D/2 columns and everything else in the
// flat gradient is the exact zero the clear left.
//
// rnvp_bwd_kernel: a workgroup (8 waves) owns a tile of 32 rows; g = dL/du of the tile lives in LDS in fp32, in the original
// column order (seed: -u_final * (-1/N); N is the global row count of the all-reduced statistic; rows past R seed zeros, so every
// gradient of such a row is an exact zero).  Per flow and network (t first: its G3 is g itself; then s, whose G3 is
// (g u_in exp(s) - 1/N)(1 - s^2) and which turns g of the transformed columns into g exp(s)):
//     G3 -> split B fragments (slot order) | G2 = (W3^T G3) [h2 > 0] | G1 = (W2^T G2) [h1 > 0] | flow 1: g[m = 1 columns] += W1^T G1
//   with the transposed products as in the forward (out^T = W^T G^T, lane = row, accumulator layout of one product = B layout of
//   the next up to the k permutation hidden_of, folded into the transposed images).  G1, G2, G3 also go to the workspace.
// rnvp_wgrad_kernel: one wave per 32 x 32 tile of a weight gradient; the contraction runs over rows, 16 per MFMA, row tiles in
//   ascending order -- one fixed summation order, no atomics: a step is bitwise reproducible.  Its operands are split into three
//   bf16 parts (six MFMAs per product, fp32 resolution): see row_frag3.  The waves of the first column tile also sum the bias
//   gradient, rows in ascending order.
//
// Budget (D = 384, HB = 8, the largest): rnvp_bwd_kernel LDS g 384 x 33 x 4 = 50,688 + two fragment buffers 2 x 32,768 = 116,224
// bytes: one workgroup of 512 threads per CU, two waves per SIMD, up to 256 registers each (one accumulator block and the
// unrolled operand loads), no scratch.  Phase A is the forward kernel's 155,136 bytes.  rnvp_wgrad_kernel: no LDS, 256 threads.
// Workspace: 3,392 channels x 128 bytes = 434 KB per tile (D = 384, HB = 8); 800 rows: 10.9 MB.
#include "rnvp_device.h"

namespace {

using namespace rnvp;

struct BwdK {
  const unsigned char* blob;    // the forward blob: column tables
  const unsigned char* timg;    // the transposed images
  float* ws;
  const double* stats;          // global {n, sum x, sum x^2, n}
  long long R;
};

// acc of output block nb -> k-steps 2 nb, 2 nb + 1 of a fragment buffer (store_hidden without the ReLU)
__device__ inline void store_grad(unsigned char* buf, int plane, int nb, int lane, const f32x16_t& acc) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = acc[8 * u + e];
    u32x4_t uh, ul;
    split8(v, uh, ul);
    unsigned char* dst = buf + (2 * nb + u) * FRAG + lane * 16;
    *(u32x4_t*)dst = uh;
    *(u32x4_t*)(dst + plane) = ul;
  }
}

// transposed images, per flow and network: W3^T [HB][KA] | W2^T [HB][KH] | W1^T [NB][KH]; the lo parts IMG_BYTES behind
template <int D, int HB>
__global__ __launch_bounds__(NTHR, 1) void rnvp_bwd_kernel(BwdK p) {
  using G = Geo<D, HB>;
  using T = TrainGeo<D, HB>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* GU = (float*)(smem + G::L_U);
  unsigned char* bufP = smem + G::L_HA;
  unsigned char* bufQ = smem + G::L_HB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 31, h = lane >> 5;
  const int* chanA = (const int*)(p.blob + G::OFF_CHAN_A);
  const int* chanB = (const int*)(p.blob + G::OFF_CHAN_B);
  const unsigned char* timg = p.timg + lane * 16;
  const int ntiles = (int)((p.R + TILE_ROWS - 1) / TILE_ROWS);
  const float gseed = (float)(-1.0 / p.stats[0]);   // dL/dscore of a real row

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long r0 = (long long)tile * TILE_ROWS;
    float* wst = p.ws + (size_t)tile * T::TILE_FLOATS;
    // ---- seed: dL/du_final = dL/dscore * (-u_final)
    for (int i = tid; i < TILE_ROWS * D; i += NTHR) {
      const int c = i >> 5, rr = i & 31;
      GU[c * US + rr] = r0 + rr < p.R ? -gseed * wst[(size_t)T::C_Z * TILE_ROWS + i] : 0.f;
    }
    __syncthreads();

#pragma unroll 1
    for (int f = NFLOW - 1; f >= 0; --f) {
      float* wsf = wst + (size_t)f * T::FLOW_CH * TILE_ROWS;
#pragma unroll 1
      for (int net = 1; net >= 0; --net) {
        const unsigned char* tf = timg + (size_t)(f * 2 + net) * G::NET_FRAGS * FRAG;
        // ---- G3 of the network -> bufP as B fragments, slot a = 16 ks + 8 h + e, and to the workspace
        for (int it = tid; it < G::KA * 64; it += NTHR) {
          const int ks = it >> 6, l = it & 63, rr = l & 31;
          const int slot0 = ks * 16 + (l >> 5) * 8;
          const float gs = r0 + rr < p.R ? gseed : 0.f;
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int c = chanB[f * G::NSLOT + slot0 + e];
            float g = 0.f;
            if (c >= 0) {
              const float go = GU[c * US + rr];
              if (net) {
                g = go;
              } else {
                const float s = wsf[(T::C_S + slot0 + e) * TILE_ROWS + rr], ui = wsf[(T::C_UIN + slot0 + e) * TILE_ROWS + rr];
                const float es = expf(s);
                g = (go * ui * es + gs) * (1.f - s * s);
                GU[c * US + rr] = go * es;
              }
            }
            v[e] = g;
            wsf[(T::C_G3 + net * G::NSLOT + slot0 + e) * TILE_ROWS + rr] = g;
          }
          u32x4_t uh, ul;
          split8(v, uh, ul);
          *(u32x4_t*)(bufP + ks * FRAG + l * 16) = uh;
          *(u32x4_t*)(bufP + G::HPLANE + ks * FRAG + l * 16) = ul;
        }
        __syncthreads();
        // ---- G2 = (W3^T G3) [h2 > 0]: bufP -> bufQ
        if (wave < HB) {
          const int nb = wave;
          f32x16_t acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
          gemm_block<G::KA>(acc, tf + (size_t)(nb * G::KA) * FRAG, G::IMG_BYTES, bufP + lane * 16, G::HPLANE);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ch = net * T::HC + 32 * nb + acc_chan(r, h);
            acc[r] = wsf[(T::C_H2 + ch) * TILE_ROWS + n] > 0.f ? acc[r] : 0.f;
            wsf[(T::C_G2 + ch) * TILE_ROWS + n] = acc[r];
          }
          store_grad(bufQ, G::HPLANE, nb, lane, acc);
        }
        __syncthreads();
        // ---- G1 = (W2^T G2) [h1 > 0]: bufQ -> bufP
        if (wave < HB) {
          const int nb = wave;
          f32x16_t acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
          gemm_block<G::KH>(acc, tf + (size_t)(HB * G::KA + nb * G::KH) * FRAG, G::IMG_BYTES, bufQ + lane * 16, G::HPLANE);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ch = net * T::HC + 32 * nb + acc_chan(r, h);
            acc[r] = wsf[(T::C_H1 + ch) * TILE_ROWS + n] > 0.f ? acc[r] : 0.f;
            wsf[(T::C_G1 + ch) * TILE_ROWS + n] = acc[r];
          }
          store_grad(bufP, G::HPLANE, nb, lane, acc);
        }
        __syncthreads();
        // ---- flow 1: the networks' input gradient joins g of the m = 1 columns (flow 0's input gradient is not needed)
        if (f > 0) {
          if (wave < G::NB) {
            const int nb = wave;
            f32x16_t acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            gemm_block<G::KH>(acc, tf + (size_t)(HB * G::KA + HB * G::KH + nb * G::KH) * FRAG, G::IMG_BYTES, bufP + lane * 16, G::HPLANE);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int c = chanA[f * G::NSLOT + 32 * nb + acc_chan(r, h)];
              if (c >= 0) GU[c * US + n] += acc[r];
            }
          }
          __syncthreads();
        }
      }
    }
    __syncthreads();   // GU is free for the next tile
  }
}

// ---- weight gradients.  Per flow and network: layer 1 [HB x NB tiles] (G1, XA), layer 2 [HB x HB] (G2, H1), layer 3 [NB x HB] (G3, H2)
struct WgradK {
  const unsigned char* blob;
  const float* ws;
  float* grads;
  int h, ntiles;
};

// 8 consecutive rows of a channel -> one lane's operand in THREE bf16 parts (v = p0 + p1 + p2 to fp32's 24 bits).  The weight
// gradients contract over rows only: with one row a gradient entry is a single product, and nothing averages the 2^-17 of a
// two-part operand pair out -- the product of two such operands alone misses 2^-16.
struct Split3 { bf16x8_t p0, p1, p2; };
__device__ inline Split3 row_frag3(const float* p) {
  const f32x4_t a = *(const f32x4_t*)p, b = *(const f32x4_t*)(p + 4);
  const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  u32x4_t u0, u1, u2;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    u0[q] = pack_bf16x2(v[2 * q], v[2 * q + 1]);
    float r0 = v[2 * q] - __uint_as_float(u0[q] << 16), r1 = v[2 * q + 1] - __uint_as_float(u0[q] & 0xffff0000u);
    u1[q] = pack_bf16x2(r0, r1);
    r0 -= __uint_as_float(u1[q] << 16);
    r1 -= __uint_as_float(u1[q] & 0xffff0000u);
    u2[q] = pack_bf16x2(r0, r1);
  }
  return {__builtin_bit_cast(bf16x8_t, u0), __builtin_bit_cast(bf16x8_t, u1), __builtin_bit_cast(bf16x8_t, u2)};
}
// acc += A * B to fp32 resolution: the six products above 2^-24 of the largest
__device__ inline void mma3(f32x16_t& acc, const Split3& a, const Split3& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p0, b.p0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p0, b.p1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p1, b.p0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p1, b.p1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p0, b.p2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p2, b.p0, acc, 0, 0, 0);
}

template <int D, int HB>
__global__ __launch_bounds__(256) void rnvp_wgrad_kernel(WgradK p) {
  using G = Geo<D, HB>;
  using T = TrainGeo<D, HB>;
  constexpr int N1 = HB * G::NB, N2 = HB * HB, PER_NET = 2 * N1 + N2;
  const int lane = threadIdx.x & 63;
  const int wt = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (wt >= NFLOW * 2 * PER_NET) return;
  const int fn = wt / PER_NET, f = fn >> 1, net = fn & 1;
  int t = wt - fn * PER_NET;
  int layer, ob, ib, gch, ach;
  if (t < N1) { layer = 1; ob = t / G::NB; ib = t - ob * G::NB; gch = T::C_G1 + net * T::HC; ach = T::C_XA; }
  else if (t < N1 + N2) { t -= N1; layer = 2; ob = t / HB; ib = t - ob * HB; gch = T::C_G2 + net * T::HC; ach = T::C_H1 + net * T::HC; }
  else { t -= N1 + N2; layer = 3; ob = t / HB; ib = t - ob * HB; gch = T::C_G3 + net * G::NSLOT; ach = T::C_H2 + net * T::HC; }
  gch += 32 * ob;
  ach += 32 * ib;
  const int n = lane & 31, hh = lane >> 5;
  const float* base = p.ws + (size_t)f * T::FLOW_CH * TILE_ROWS;
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float bsum = 0.f;
  const bool want_bias = ib == 0 && hh == 0;   // lane n of the first column tile: the bias gradient of output channel n
  for (int tile = 0; tile < p.ntiles; ++tile) {
    const float* tb = base + (size_t)tile * T::TILE_FLOATS;
    const float* gp = tb + (size_t)(gch + n) * TILE_ROWS + 8 * hh;
    const float* ap = tb + (size_t)(ach + n) * TILE_ROWS + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) mma3(acc, row_frag3(gp + 16 * ks), row_frag3(ap + 16 * ks));
    if (want_bias) {
      const float* gr = tb + (size_t)(gch + n) * TILE_ROWS;
#pragma unroll
      for (int q = 0; q < TILE_ROWS / 4; ++q) {
        const f32x4_t g4 = *(const f32x4_t*)(gr + 4 * q);
        bsum += g4[0]; bsum += g4[1]; bsum += g4[2]; bsum += g4[3];
      }
    }
  }
  const int h = p.h;
  const size_t net_params = (size_t)h * D + h + (size_t)h * h + h + (size_t)D * h + D;
  float* W1 = p.grads + fn * net_params;
  float* b1 = W1 + (size_t)h * D;
  float* W2 = b1 + h;
  float* b2 = W2 + (size_t)h * h;
  float* W3 = b2 + h;
  float* b3 = W3 + (size_t)D * h;
  const int* colA = (const int*)(p.blob + G::OFF_COL_A) + f * G::NSLOT;
  const int* colB = (const int*)(p.blob + G::OFF_COL_B) + f * G::NSLOT;
  const int in = 32 * ib + n;
  if (layer == 1) {
    const int j = colA[in];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * ob + acc_chan(r, hh);
      if (row < h && j >= 0) W1[(size_t)row * D + j] = acc[r];
    }
    if (want_bias && 32 * ob + n < h) b1[32 * ob + n] = bsum;
  } else if (layer == 2) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * ob + acc_chan(r, hh);
      if (row < h && in < h) W2[(size_t)row * h + in] = acc[r];
    }
    if (want_bias && 32 * ob + n < h) b2[32 * ob + n] = bsum;
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = colB[32 * ob + acc_chan(r, hh)];
      if (j >= 0 && in < h) W3[(size_t)j * h + in] = acc[r];
    }
    if (want_bias) {
      const int j = colB[32 * ob + n];
      if (j >= 0) b3[j] = bsum;
    }
  }
}

// ---- {n, sum x, sum x^2, n} of x = -score: one workgroup, each thread its rows in ascending order, then a fixed tree
__global__ __launch_bounds__(256) void rnvp_stat_kernel(const float* __restrict__ score, long long R, double* __restrict__ stats) {
  __shared__ double s1[256], s2[256];
  const int tid = threadIdx.x;
  double a = 0, b = 0;
  for (long long r = tid; r < R; r += 256) { const double x = -(double)score[r]; a += x; b += x * x; }
  s1[tid] = a; s2[tid] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) { s1[tid] += s1[tid + w]; s2[tid] += s2[tid + w]; }
    __syncthreads();
  }
  if (tid == 0) { stats[0] = (double)R; stats[1] = s1[0]; stats[2] = s2[0]; stats[3] = (double)R; }
}

// ---- losses = {loss, mean, std} and the commit of the confidence statistic (one thread)
__global__ void rnvp_commit_kernel(const double* __restrict__ stats, int method, double* __restrict__ cstate, float* __restrict__ losses) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const ConfPost cp = conf_commit(method, stats, cstate);
  losses[0] = (float)(stats[1] / stats[0]);
  losses[1] = cp.mean;
  losses[2] = cp.std;
}

// ---- transposed images (column tables from the forward blob)
template <int D, int HB>
__global__ void rnvp_train_pack_kernel(const float* __restrict__ prm, int h, const unsigned char* __restrict__ blob,
                                       unsigned char* __restrict__ out) {
  using G = Geo<D, HB>;
  const int* colA = (const int*)(blob + G::OFF_COL_A);
  const int* colB = (const int*)(blob + G::OFF_COL_B);
  const size_t net_params = (size_t)h * D + h + (size_t)h * h + h + (size_t)D * h + D;
  const int gsz = gridDim.x * blockDim.x, g0 = blockIdx.x * blockDim.x + threadIdx.x;
  bf16_t* imgh = (bf16_t*)out;
  bf16_t* imgl = (bf16_t*)(out + G::IMG_BYTES);
  for (int i = g0; i < G::IMG_BYTES / 2; i += gsz) {
    const int e = i & 7, m = (i >> 3) & 31, hh = (i >> 8) & 1;
    int fr = i >> 9;
    const int fn = fr / G::NET_FRAGS, f = fn >> 1;
    fr -= fn * G::NET_FRAGS;
    const float* W1 = prm + fn * net_params;
    const float* W2 = W1 + (size_t)h * D + h;
    const float* W3 = W2 + (size_t)h * h + h;
    float v = 0.f;
    if (fr < HB * G::KA) {                         // W3^T: hidden unit 32 nb + m x slot 16 ks + 8 hh + e
      const int nb = fr / G::KA, ks = fr - nb * G::KA;
      const int hid = 32 * nb + m, j = colB[f * G::NSLOT + ks * 16 + 8 * hh + e];
      if (hid < h && j >= 0) v = W3[(size_t)j * h + hid];
    } else if (fr < HB * G::KA + HB * G::KH) {     // W2^T: input unit 32 nb + m x output unit hidden_of(ks, hh, e)
      fr -= HB * G::KA;
      const int nb = fr / G::KH, ks = fr - nb * G::KH;
      const int hid = 32 * nb + m, k = hidden_of(ks, hh, e);
      if (hid < h && k < h) v = W2[(size_t)k * h + hid];
    } else {                                       // W1^T: slot 32 nb + m x hidden unit hidden_of(ks, hh, e)
      fr -= HB * G::KA + HB * G::KH;
      const int nb = fr / G::KH, ks = fr - nb * G::KH;
      const int j = colA[f * G::NSLOT + 32 * nb + m], k = hidden_of(ks, hh, e);
      if (j >= 0 && k < h) v = W1[(size_t)k * D + j];
    }
    const bf16_t hi = f32_to_bf16(v);
    imgh[i] = hi;
    imgl[i] = f32_to_bf16(v - bf16_to_f32(hi));
  }
}

template <int D, int HB>
int phase_a_launch(const RnvpCall& c, double* stats, void* ws, hipStream_t st) {
  using G = Geo<D, HB>;
  if (c.R > 0) {
    RnvpK k{};
    if (const int rc = fill_args(c, k)) return rc;
    k.ws = (float*)ws;
    auto kern = rnvp_kernel<D, HB, true>;
    static LdsOptIn lds_opt_in;   // per device (common.h)
    if (const int rc = lds_opt_in(G::LDS_BYTES, (const void*)kern)) return rc;
    const int cus = wvn_num_cus();
    const long long ntiles = (c.R + TILE_ROWS - 1) / TILE_ROWS;
    hipLaunchKernelGGL(kern, dim3((unsigned)(ntiles < cus ? ntiles : cus)), dim3(NTHR), G::LDS_BYTES, st, k);
    WVN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rnvp_stat_kernel, dim3(1), dim3(256), 0, st, c.score, c.R, stats);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

template <int D, int HB>
int phase_b_launch(int h, const void* packed, const void* tpacked, long long R, const double* stats, float* grads, void* ws, hipStream_t st) {
  using G = Geo<D, HB>;
  constexpr int LDS = G::L_HC;   // g and two fragment buffers
  const size_t nparam = wvn_rnvp_train_param_count_impl(D, h);
  if (const hipError_t e = hipMemsetAsync(grads, 0, nparam * sizeof(float), st); e != hipSuccess) return (int)e;
  if (R == 0) return WVN_OK;
  const int ntiles = (int)((R + TILE_ROWS - 1) / TILE_ROWS);
  auto kern = rnvp_bwd_kernel<D, HB>;
  static LdsOptIn lds_opt_in;
  if (const int rc = lds_opt_in(LDS, (const void*)kern)) return rc;
  const int cus = wvn_num_cus();
  const BwdK b{(const unsigned char*)packed, (const unsigned char*)tpacked, (float*)ws, stats, R};
  hipLaunchKernelGGL(kern, dim3((unsigned)(ntiles < cus ? ntiles : cus)), dim3(NTHR), LDS, st, b);
  WVN_LAUNCH_CHECK();
  constexpr int WT = NFLOW * 2 * (2 * HB * G::NB + HB * HB);
  const WgradK w{(const unsigned char*)packed, (const float*)ws, grads, h, ntiles};
  hipLaunchKernelGGL((rnvp_wgrad_kernel<D, HB>), dim3((WT + 3) / 4), dim3(256), 0, st, w);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // namespace

size_t wvn_rnvp_train_param_count_impl(int D, int h) {
  return (size_t)NFLOW * 2 * ((size_t)h * D + h + (size_t)h * h + h + (size_t)D * h + D);
}
size_t wvn_rnvp_train_workspace_bytes_impl(int D, int h, long long R) {
  const size_t ntiles = (size_t)((R + TILE_ROWS - 1) / TILE_ROWS);
  const size_t per = dispatch(D, h, [](auto s) { return (size_t)TrainGeo<decltype(s)::d, decltype(s)::hb>::TILE_FLOATS * sizeof(float); });
  return (ntiles ? ntiles : 1) * per;
}
size_t wvn_rnvp_train_pack_bytes_impl(int D, int h) {
  return dispatch(D, h, [](auto s) { return (size_t)2 * Geo<decltype(s)::d, decltype(s)::hb>::IMG_BYTES; });
}
int wvn_rnvp_train_pack_launch(int D, int h, const float* params, const void* packed, void* tpacked, hipStream_t st) {
  dispatch(D, h, [&](auto s) {
    hipLaunchKernelGGL((rnvp_train_pack_kernel<decltype(s)::d, decltype(s)::hb>), dim3(256), dim3(256), 0, st, params, h,
                       (const unsigned char*)packed, (unsigned char*)tpacked);
    return 0;
  });
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
int wvn_rnvp_train_phase_a_launch(const RnvpCall& c, double* stats, void* ws, hipStream_t st) {
  return dispatch(c.D, c.h, [&](auto s) { return phase_a_launch<decltype(s)::d, decltype(s)::hb>(c, stats, ws, st); });
}
int wvn_rnvp_train_phase_b_launch(int D, int h, const void* packed, const void* tpacked, long long R, const double* stats, float* grads,
                                  void* ws, hipStream_t st) {
  return dispatch(D, h, [&](auto s) { return phase_b_launch<decltype(s)::d, decltype(s)::hb>(h, packed, tpacked, R, stats, grads, ws, st); });
}
int wvn_rnvp_train_commit_launch(const double* stats, int method, double* cstate, float* losses, hipStream_t st) {
  hipLaunchKernelGGL(rnvp_commit_kernel, dim3(1), dim3(64), 0, st, stats, method, cstate, losses);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
