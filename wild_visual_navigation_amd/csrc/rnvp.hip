// Anomaly detection: the forward pass of the LinearRnvp flow (model/linear_rnvp.py:216-296) as the live node runs it with
// params.model.name == "LinearRnvp" (wvn_feature_extractor_node.py:319-344), on every segment row or every pixel of a frame:
//
//   per coupling layer f (mask m, networks S_f, T_f: D -> h -> h -> D, ReLU after the first two linears):
//     mu = u*m;  s = tanh(S(mu));  t = T(mu);  x = mu + (1-m)*(u*exp(s) + t);  log_det += sum((1-m)*s);  then x = x[:, p_f]
//   score = sum_c(-z_c^2 / 2 - log sqrt(2 pi)) + log_det                       (loss.py:42, unit normal prior)
//
// One kernel body, rnvp_kernel<D, HB, TRAIN> (rnvp_device.h; TRAIN = false here, true in phase A of the training step,
// rnvp_train.hip), holds both coupling layers, with two row sources: rows x [R][D], or pixels whose row is the
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
#include "rnvp_device.h"

namespace {

using namespace rnvp;

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
template <int D, int HB>
int rnvp_launch(const RnvpCall& c, hipStream_t st) {
  using G = Geo<D, HB>;
  RnvpK k{};
  if (const int rc = fill_args(c, k)) return rc;
  auto kern = rnvp_kernel<D, HB, false>;
  static LdsOptIn lds_opt_in;   // per device (common.h)
  if (const int rc = lds_opt_in(G::LDS_BYTES, (const void*)kern)) return rc;
  const int cus = wvn_num_cus();
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
