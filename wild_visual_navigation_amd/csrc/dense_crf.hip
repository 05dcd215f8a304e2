// Exact fully connected CRF (mean field, Potts compatibility): the DenseCRF2D recipe of the public STEGO crf.py, with every
// pixel pair evaluated (no permutohedral lattice).  Definition, readings and error budget: DESIGN.md section "Dense CRF".
//
//   crf_image_kernel      the u8 image STEGO's dense_crf rebuilds from the normalised frame (Normalize -> UnNormalize ->
//                         to_pil_image, one fp32 operation at a time; the unit is compiled with -ffp-contract=off)
//   crf_bilateral_kernel  flash style: a workgroup owns 128 query pixels (32 per wave) and streams every 64-key tile of its frame.
//                         Per pair the exponent is formed from exact integer distances (positions as fp32 integers, colours as
//                         c - 128 in i8 through v_dot4_i32_i8: |c_i - c_j|^2 = |c_i|^2 + |c_j|^2 - 2 c_i.c_j in i32), scaled once in
//                         fp32, exp2'd, and the weight goes to the matrix pipe as two fp16 planes (hi + lo, scaled by 2^15) against the
//                         two fp16 planes of V = n_b * Q (scaled by 2^15): V_hi P_hi + V_hi P_lo + V_lo P_hi in fp32 accumulators.
//                         NORM = the same pass with unit values on the VALU (n_b, once per frame).  UPDATE epilogue: * n_b(i),
//                         + w_g * the smoothness stencil, + (-U), softmax per CRF group, Q and the planes of the next V to the other
//                         half of the double buffers; the last iteration also writes labels / probabilities / the debug messages.
//   crf_prep_kernel       unary (-U = log clip(softmax L, 1e-5, 1)), Q^0, n_g (the stencil with unit values) and the planes of V^0.
// Two CRFs on one image share every launch: their value columns are concatenated (K1 + K2 <= 64), the softmax runs per group.
#include <cmath>

#include "common.h"
#include "wvn_internal.h"
#include "../../include/wvn_hip.h"

namespace {

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

constexpr int QB = 128;        // query pixels per workgroup (4 waves x 32)
constexpr int KB = 64;         // keys per tile
constexpr int VROW = KB + 8;   // LDS row of a value plane: 64 keys + 8 halves of padding (144 B)
constexpr float PSCALE = 32768.f, VSCALE = 32768.f, INV_PV = 1.0f / (32768.f * 32768.f);
constexpr float LOG2E = 1.44269504088896340736f;

__device__ inline float image_channel(const unsigned char* p) { return (float)*p / 255.0f; }  // == torch's x.float() / 255
__device__ inline float image_channel(const float* p) { return *p; }

// STEGO dense_crf's image: to_pil_image(UnNormalize(Normalize(x))) = u8(trunc(255 * ((((x - m) / s) * s) + m))), every step in fp32
template <typename TIN>
__global__ __launch_bounds__(256) void crf_image_kernel(const TIN* __restrict__ frame, int Hs, int Ws, const int* __restrict__ rows,
                                                        const int* __restrict__ cols, int Ho, int Wo, int B, unsigned char* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * Ho * Wo) return;
  const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho), b = (int)(i / ((long long)Wo * Ho));
  const int sy = rows ? rows[y] : y, sx = cols ? cols[x] : x;
  const float mean[3] = {0.485f, 0.456f, 0.406f};
  const float stdv[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = image_channel(frame + (((size_t)b * 3 + c) * Hs + sy) * Ws + sx);
    const float n = (v - mean[c]) / stdv[c];
    const float r = n * stdv[c] + mean[c];
    const float s = r * 255.0f;
    out[i * 3 + c] = (unsigned char)(int)fminf(fmaxf(s, 0.f), 255.f);   // (truncation toward zero, as tensor.byte())
  }
}

struct CrfArgs {
  const float* l1; long long s1b, s1c, s1p; int K1;
  const float* l2; long long s2b, s2c, s2p; int K2;
  const unsigned char* img;   // [B][N][3]
  int B, H, W, N, Npad, KT, KP, R;
  float ca, cb, cg;           // exponent scales (log2 units): position (bilateral), colour, position (smoothness)
  float w_pos, w_bi;
  float* negU;                // [B][N][KP]
  float* q[2];                // [B][N][KP]
  float* nb; float* ng;       // [B][N]
  uint16_t* vh[2]; uint16_t* vl[2];   // [B][KP][Npad] fp16 planes of V * 2^15
  int* labels; float* probs; float* dbg;
};

__device__ inline int colour_word(const unsigned char* p, int& norm) {
  const int r = (int)p[0] - 128, g = (int)p[1] - 128, b = (int)p[2] - 128;
  norm = r * r + g * g + b * b;
  return (r & 0xff) | ((g & 0xff) << 8) | ((b & 0xff) << 16);
}

// sum over the (2R+1)^2 window (clipped to the image) of k_g(i, j) * f(j), fixed order
template <typename F>
__device__ inline void stencil_walk(const CrfArgs& a, int x, int y, F&& f) {
  for (int dy = -a.R; dy <= a.R; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= a.H) continue;
    for (int dx = -a.R; dx <= a.R; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= a.W) continue;
      f(yy * a.W + xx, __builtin_amdgcn_exp2f((float)(dx * dx + dy * dy) * a.cg));
    }
  }
}

// one thread per (frame, pixel < Npad)
__global__ __launch_bounds__(256) void crf_prep_kernel(CrfArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)a.B * a.Npad) return;
  const int b = (int)(i / a.Npad), p = (int)(i % a.Npad);
  if (p >= a.N) {   // padding keys: zero values in both halves of the double buffer
    for (int c = 0; c < a.KP; ++c)
      for (int s = 0; s < 2; ++s) {
        a.vh[s][((size_t)b * a.KP + c) * a.Npad + p] = 0;
        a.vl[s][((size_t)b * a.KP + c) * a.Npad + p] = 0;
      }
    return;
  }
  const size_t row = ((size_t)b * a.N + p) * a.KP;
  float sg = 0.f;
  stencil_walk(a, p % a.W, p / a.W, [&](int, float w) { sg += w; });
  const float ng = 1.0f / sqrtf(sg + 1e-20f);
  a.ng[(size_t)b * a.N + p] = ng;
  const float nb = a.nb[(size_t)b * a.N + p];
  for (int grp = 0; grp < 2; ++grp) {
    const float* L = grp ? a.l2 : a.l1;
    const int K = grp ? a.K2 : a.K1, off = grp ? a.K1 : 0;
    if (K == 0) continue;
    const long long sb = grp ? a.s2b : a.s1b, sc = grp ? a.s2c : a.s1c, sp = grp ? a.s2p : a.s1p;
    const float* l = L + b * sb + p * sp;
    float m = -INFINITY;
    for (int k = 0; k < K; ++k) m = fmaxf(m, l[k * sc]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(l[k * sc] - m);
    float m2 = -INFINITY;
    for (int k = 0; k < K; ++k) {   // -U = log(clip(softmax(L), 1e-5, 1))   (pydensecrf.utils.unary_from_softmax)
      const float pk = expf(l[k * sc] - m) / s;
      const float u = logf(fminf(fmaxf(pk, 1e-5f), 1.0f));
      a.negU[row + off + k] = u;
      m2 = fmaxf(m2, u);
    }
    float s2 = 0.f;
    for (int k = 0; k < K; ++k) s2 += expf(a.negU[row + off + k] - m2);
    for (int k = 0; k < K; ++k) {   // Q^0 = softmax(-U)
      const float qv = expf(a.negU[row + off + k] - m2) / s2;
      a.q[0][row + off + k] = qv;
      const float v = nb * qv * VSCALE;
      const uint16_t h = f32_to_f16(v);
      a.vh[0][((size_t)b * a.KP + off + k) * a.Npad + p] = h;
      a.vl[0][((size_t)b * a.KP + off + k) * a.Npad + p] = f32_to_f16(v - f16_to_f32(h));
    }
  }
  for (int c = a.KT; c < a.KP; ++c) {
    a.negU[row + c] = 0.f;
    a.q[0][row + c] = 0.f;
    a.q[1][row + c] = 0.f;
    for (int s = 0; s < 2; ++s) {
      a.vh[s][((size_t)b * a.KP + c) * a.Npad + p] = 0;
      a.vl[s][((size_t)b * a.KP + c) * a.Npad + p] = 0;
    }
  }
}

// NCT = 0: the normaliser pass (unit values, VALU sums); 1 / 2: 32-column tiles of value columns (KP = 32 / 64)
template <int NCT>
__global__ __launch_bounds__(256) void crf_bilateral_kernel(CrfArgs a, int src, int last) {
  constexpr bool NORM = NCT == 0;
  constexpr int VR = NORM ? 1 : NCT * 32;   // value rows per plane tile
  __shared__ __attribute__((aligned(16))) f32x2_t kpos[2][KB];
  __shared__ __attribute__((aligned(16))) int kcol[2][KB];
  __shared__ __attribute__((aligned(16))) int knrm[2][KB];
  __shared__ __attribute__((aligned(16))) uint16_t vlds[NORM ? 1 : 2][2][VR][VROW];   // [buffer][plane][value column][key]
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = tid >> 6;
  const int b = blockIdx.y;
  const int q = blockIdx.x * QB + wave * 32 + l31;
  const int qc = q < a.N ? q : a.N - 1;
  const unsigned char* img = a.img + (size_t)b * a.N * 3;
  const float qx = (float)(qc % a.W), qy = (float)(qc / a.W);
  int qn;
  const int qcol = colour_word(img + (size_t)qc * 3, qn);
  const int nt = a.Npad / KB;

  // ---- staging: key features (threads 0..63) and the two value planes (16-byte chunks) of a 64-key tile ----
  constexpr int CHUNKS = NORM ? 0 : 2 * VR * (KB / 8);   // 16-byte chunks per tile
  constexpr int CPT = CHUNKS / 256;                       // per thread
  f32x2_t st_pos = {0.f, 0.f};
  int st_col = 0, st_nrm = 0;
  u32x4_t st_v[CPT > 0 ? CPT : 1];
  const uint16_t* vsrc[2] = {a.vh[src] + (size_t)b * a.KP * a.Npad, a.vl[src] + (size_t)b * a.KP * a.Npad};
  auto fetch = [&](int t) {
    if (tid < KB) {
      const int k = t * KB + tid;
      if (k < a.N) {
        st_pos = f32x2_t{(float)(k % a.W), (float)(k / a.W)};
        st_col = colour_word(img + (size_t)k * 3, st_nrm);
      } else {   // beyond the image: far away, weight exactly 0
        st_pos = f32x2_t{1e6f, 1e6f};
        st_col = 0;
        st_nrm = 0;
      }
    }
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
      const int c = tid + u * 256, pl = c / (VR * 8), r = (c / 8) % VR, ch = c % 8;
      st_v[u] = *(const u32x4_t*)(vsrc[pl] + (size_t)r * a.Npad + t * KB + ch * 8);
    }
  };
  auto stage = [&](int buf) {
    if (tid < KB) {
      kpos[buf][tid] = st_pos;
      kcol[buf][tid] = st_col;
      knrm[buf][tid] = st_nrm;
    }
    if constexpr (!NORM) {
#pragma unroll
      for (int u = 0; u < CPT; ++u) {
        const int c = tid + u * 256, pl = c / (VR * 8), r = (c / 8) % VR, ch = c % 8;
        *(u32x4_t*)&vlds[buf][pl][r][ch * 8] = st_v[u];
      }
    }
  };

  f32x16_t acc[NCT > 0 ? NCT : 1];
#pragma unroll
  for (int ct = 0; ct < (NCT > 0 ? NCT : 1); ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  float nsum = 0.f;

  fetch(0);
  stage(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) fetch(t + 1);
    f32x16_t tacc[NCT > 0 ? NCT : 1];
    float tsum = 0.f;
#pragma unroll
    for (int g = 0; g < KB / 16; ++g) {
      const int k0 = g * 16 + hi * 8;
      float p[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const f32x2_t kp = kpos[buf][k0 + e];
        const float dx = kp[0] - qx, dy = kp[1] - qy;
        const float dpos = fmaf(dx, dx, dy * dy);                                        // exact (integers < 2^24)
        const int dcol = (knrm[buf][k0 + e] - 2 * __builtin_amdgcn_sdot4(qcol, kcol[buf][k0 + e], 0, false)) + qn;   // exact
        p[e] = __builtin_amdgcn_exp2f(fmaf(dpos, a.ca, (float)dcol * a.cb));
      }
      if constexpr (NORM) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += p[e];
        tsum += s;
      } else {
        union { uint32_t u[4]; f16x8_t v; } ph, pl;
#pragma unroll
        for (int e = 0; e < 4; ++e) wvn_split2_f16(p[2 * e] * PSCALE, p[2 * e + 1] * PSCALE, ph.u[e], pl.u[e]);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const f16x8_t ah = *(const f16x8_t*)&vlds[buf][0][ct * 32 + l31][k0];
          const f16x8_t al = *(const f16x8_t*)&vlds[buf][1][ct * 32 + l31][k0];
          if (g == 0) tacc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, pl.v, (f32x16_t)(0.f), 0, 0, 0);
          else tacc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, pl.v, tacc[ct], 0, 0, 0);
          tacc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, ph.v, tacc[ct], 0, 0, 0);
          tacc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ph.v, tacc[ct], 0, 0, 0);
        }
      }
    }
    // per-tile partial sums enter the running sums once per tile (N / 64 fp32 roundings per element instead of N / 16)
    if constexpr (NORM) {
      nsum += tsum;
    } else {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[ct] += tacc[ct];
    }
    if (t + 1 < nt) stage(buf ^ 1);
    __syncthreads();
  }

  const size_t pix = (size_t)b * a.N + q;
  if constexpr (NORM) {
    const float tot = nsum + __shfl_xor(nsum, 32, 64);
    if (hi == 0 && q < a.N) a.nb[pix] = 1.0f / sqrtf(tot + 1e-20f);
    return;
  } else {
    if (q >= a.N) return;
    // lane (l31, hi) holds query q, value columns ct * 32 + 8 gg + 4 hi + e in acc[ct][4 gg + e]
    const float nbq = a.nb[pix], ngq = a.ng[pix];
    f32x16_t msg_g[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) msg_g[ct][r] = 0.f;
    const float* qsrc = a.q[src] + (size_t)b * a.N * a.KP;
    stencil_walk(a, q % a.W, q / a.W, [&](int j, float w) {
      const float wn = w * a.ng[(size_t)b * a.N + j];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
          const f32x4_t v = *(const f32x4_t*)(qsrc + (size_t)j * a.KP + ct * 32 + gg * 8 + hi * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) msg_g[ct][4 * gg + e] = fmaf(wn, v[e], msg_g[ct][4 * gg + e]);
        }
    });
    const float* nu = a.negU + pix * a.KP;
    f32x16_t lg[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        const f32x4_t u = *(const f32x4_t*)(nu + ct * 32 + gg * 8 + hi * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * gg + e;
          acc[ct][r] = acc[ct][r] * INV_PV * nbq;   // bilateral message n_b(i) sum_j k_b(i,j) n_b(j) Q_j
          msg_g[ct][r] *= ngq;                      // smoothness message
          lg[ct][r] = u[e] + a.w_bi * acc[ct][r] + a.w_pos * msg_g[ct][r];
        }
      }
    // softmax per CRF group (columns [0, K1) and [K1, KT)); the half-waves hold disjoint columns of the same pixel
    float gmax[2] = {-INFINITY, -INFINITY};
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int col = ct * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
        if (col < a.KT) {
          const int grp = col >= a.K1;
          gmax[grp] = fmaxf(gmax[grp], lg[ct][r]);
        }
      }
#pragma unroll
    for (int s = 0; s < 2; ++s) gmax[s] = fmaxf(gmax[s], __shfl_xor(gmax[s], 32, 64));
    float gsum[2] = {0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int col = ct * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
        const int grp = col >= a.K1;
        const float ev = col < a.KT ? expf(lg[ct][r] - gmax[grp]) : 0.f;
        lg[ct][r] = ev;
        gsum[grp] += ev;
      }
#pragma unroll
    for (int s = 0; s < 2; ++s) gsum[s] += __shfl_xor(gsum[s], 32, 64);
    float* qdst = a.q[src ^ 1] + pix * a.KP;
    uint16_t* vh = a.vh[src ^ 1] + (size_t)b * a.KP * a.Npad + q;
    uint16_t* vl = a.vl[src ^ 1] + (size_t)b * a.KP * a.Npad + q;
    float best[2] = {-INFINITY, -INFINITY};
    int arg[2] = {0, a.K1};
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        f32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * gg + e, col = ct * 32 + 8 * gg + 4 * hi + e;
          const int grp = col >= a.K1;
          const float qv = col < a.KT ? lg[ct][r] / gsum[grp] : 0.f;
          o[e] = qv;
          const float v = nbq * qv * VSCALE;
          const uint16_t h = f32_to_f16(v);
          vh[(size_t)col * a.Npad] = h;
          vl[(size_t)col * a.Npad] = f32_to_f16(v - f16_to_f32(h));
          if (col < a.KT && qv > best[grp]) { best[grp] = qv; arg[grp] = col; }   // (columns in increasing order: the first maximum)
          if (last && col < a.KT) {
            if (a.probs) a.probs[((size_t)b * a.KT + col) * a.N + q] = qv;
            if (a.dbg) {
              a.dbg[((size_t)b * (2 * a.KP + 2) + col) * a.N + q] = acc[ct][r];
              a.dbg[((size_t)b * (2 * a.KP + 2) + a.KP + col) * a.N + q] = msg_g[ct][r];
            }
          }
        }
        *(f32x4_t*)(qdst + ct * 32 + gg * 8 + hi * 4) = o;
      }
    if (last) {
      const int ng_ = a.K2 > 0 ? 2 : 1;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float ob = __shfl_xor(best[s], 32, 64);
        const int oa = __shfl_xor(arg[s], 32, 64);
        if (ob > best[s] || (ob == best[s] && oa < arg[s])) { best[s] = ob; arg[s] = oa; }
      }
      if (hi == 0) {
        if (a.labels)
          for (int s = 0; s < ng_; ++s) a.labels[((size_t)b * ng_ + s) * a.N + q] = arg[s] - (s ? a.K1 : 0);
        if (a.dbg) {
          a.dbg[((size_t)b * (2 * a.KP + 2) + 2 * a.KP) * a.N + q] = nbq;
          a.dbg[((size_t)b * (2 * a.KP + 2) + 2 * a.KP + 1) * a.N + q] = ngq;
        }
      }
    }
  }
}

struct CrfLayout {
  size_t negU, q0, q1, nb, ng, vh0, vl0, vh1, vl1, total;
};

CrfLayout crf_layout(int B, int N, int KT) {
  const size_t KP = KT <= 32 ? 32 : 64, Npad = (size_t)(N + KB - 1) / KB * KB;
  CrfLayout l;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
  l.negU = take((size_t)B * N * KP * 4);
  l.q0 = take((size_t)B * N * KP * 4);
  l.q1 = take((size_t)B * N * KP * 4);
  l.nb = take((size_t)B * N * 4);
  l.ng = take((size_t)B * N * 4);
  l.vh0 = take((size_t)B * KP * Npad * 2);
  l.vl0 = take((size_t)B * KP * Npad * 2);
  l.vh1 = take((size_t)B * KP * Npad * 2);
  l.vl1 = take((size_t)B * KP * Npad * 2);
  l.total = o;
  return l;
}

bool crf_shape_ok(int B, int H, int W, int K1, int K2) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 2048 && W <= 2048 && K1 >= 1 && K2 >= 0 && K1 + K2 <= 64;
}

}  // namespace

extern "C" {

size_t wvn_dense_crf_workspace_bytes(int B, int H, int W, int K) {
  if (!crf_shape_ok(B, H, W, K, 0)) return 0;
  return crf_layout(B, H * W, K).total;
}

int wvn_dense_crf(const float* logits1, int K1, long long s1b, long long s1c, long long s1p, const float* logits2, int K2, long long s2b,
                  long long s2c, long long s2p, const unsigned char* image, int B, int H, int W, int iterations, float pos_w, float pos_xy_std,
                  float bi_w, float bi_xy_std, float bi_rgb_std, int* labels, int* nseg_last, float* probs, float* debug, void* workspace,
                  size_t workspace_bytes, void* stream) {
  if (!logits1 || !image || !workspace || !crf_shape_ok(B, H, W, K1, K2) || (K2 > 0) != (logits2 != nullptr)) return WVN_ERR_ARG;
  if (nseg_last && !labels) return WVN_ERR_ARG;
  if (!labels && !probs && !debug) return WVN_ERR_ARG;
  if (iterations < 1 || iterations > 1000) return WVN_ERR_ARG;
  if (!(pos_xy_std > 0.f && pos_xy_std <= 4.f && bi_xy_std > 0.f && bi_rgb_std > 0.f) || !std::isfinite(bi_xy_std) || !std::isfinite(bi_rgb_std))
    return WVN_ERR_ARG;
  if (!std::isfinite(pos_w) || !std::isfinite(bi_w)) return WVN_ERR_ARG;
  const int N = H * W, KT = K1 + K2;
  const CrfLayout l = crf_layout(B, N, KT);
  if (workspace_bytes < l.total) return WVN_ERR_WORKSPACE;
  unsigned char* ws = (unsigned char*)workspace;
  CrfArgs a;
  a.l1 = logits1; a.s1b = s1b; a.s1c = s1c; a.s1p = s1p; a.K1 = K1;
  a.l2 = logits2; a.s2b = s2b; a.s2c = s2c; a.s2p = s2p; a.K2 = K2;
  a.img = image;
  a.B = B; a.H = H; a.W = W; a.N = N; a.Npad = (N + KB - 1) / KB * KB; a.KT = KT; a.KP = KT <= 32 ? 32 : 64;
  a.R = (int)ceilf(8.f * pos_xy_std);   // radius 8 sigma: every dropped smoothness weight is < e^-40.5 of the self term
  a.ca = (float)(-(double)LOG2E / (2.0 * (double)bi_xy_std * bi_xy_std));
  a.cb = (float)(-(double)LOG2E / (2.0 * (double)bi_rgb_std * bi_rgb_std));
  a.cg = (float)(-(double)LOG2E / (2.0 * (double)pos_xy_std * pos_xy_std));
  a.w_pos = pos_w; a.w_bi = bi_w;
  a.negU = (float*)(ws + l.negU);
  a.q[0] = (float*)(ws + l.q0); a.q[1] = (float*)(ws + l.q1);
  a.nb = (float*)(ws + l.nb); a.ng = (float*)(ws + l.ng);
  a.vh[0] = (uint16_t*)(ws + l.vh0); a.vl[0] = (uint16_t*)(ws + l.vl0);
  a.vh[1] = (uint16_t*)(ws + l.vh1); a.vl[1] = (uint16_t*)(ws + l.vl1);
  a.labels = labels; a.probs = probs; a.dbg = debug;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ceil_div(N, QB), B);
  hipLaunchKernelGGL(crf_bilateral_kernel<0>, grid, dim3(256), 0, st, a, 0, 0);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(crf_prep_kernel, dim3((unsigned)(((long long)B * a.Npad + 255) / 256)), dim3(256), 0, st, a);
  WVN_LAUNCH_CHECK();
  for (int t = 1; t <= iterations; ++t) {
    const int src = (t - 1) & 1, last = t == iterations;
    if (a.KP == 32) hipLaunchKernelGGL(crf_bilateral_kernel<1>, grid, dim3(256), 0, st, a, src, last);
    else hipLaunchKernelGGL(crf_bilateral_kernel<2>, grid, dim3(256), 0, st, a, src, last);
    WVN_LAUNCH_CHECK();
  }
  if (nseg_last) {   // the k-means relabel rule on the last group: used ids compacted to 0..n-1 in ascending order, n per frame
    const int ng = K2 > 0 ? 2 : 1;
    for (int b = 0; b < B; ++b) {
      const int rc = wvn_km_relabel_launch(labels + ((size_t)b * ng + ng - 1) * N, nseg_last + b, 1, N, ng == 2 ? K2 : K1, 1, st);
      if (rc) return rc;
    }
  }
  return WVN_OK;
}

int wvn_crf_image(const void* frame, int frame_u8, int B, int src_h, int src_w, const int* rows, const int* cols, int out_h, int out_w,
                  unsigned char* out, void* stream) {
  if (!frame || !out || B < 1 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 || (!rows) != (!cols)) return WVN_ERR_ARG;
  if (!rows && (out_h != src_h || out_w != src_w)) return WVN_ERR_ARG;
  const long long n = (long long)B * out_h * out_w;
  if (n >= (1ll << 31) * 256) return WVN_ERR_ARG;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (frame_u8)
    hipLaunchKernelGGL(crf_image_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)frame, src_h, src_w,
                       rows, cols, out_h, out_w, B, out);
  else
    hipLaunchKernelGGL(crf_image_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)frame, src_h, src_w, rows, cols,
                       out_h, out_w, B, out);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // extern "C"
