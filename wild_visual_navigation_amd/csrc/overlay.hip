// Traversability / confidence / segmentation overlays (visu/visualizer.py of the reference: plot_image, plot_segmentation,
// plot_detectron, plot_detectron_classification, plot_traversability_graph_on_seg, plot_list) as ONE pass per output pixel.
//
//   frame_max_kernel   fmax[b] = max(0, max of frame b), NaN when the frame holds a NaN: the "multiply by 255 iff max <= 1" decision
//                      of plot_image without a host read (skipped when the caller states the range)
//   overlay_kernel     frame -> 8 bits, value / label / per-segment value -> colour index -> colour table (LDS) -> alpha composite
//                      (-> white boundary composite) -> packed RGB bytes at a column offset of a pitched destination; a panel call
//                      converts the frame once and writes [plain | overlay 0 | overlay 1 | ...] side by side
//
// Everything is integer arithmetic on bytes apart from two fp32 multiplications by 255 (frame, value), each rounded on its own
// (this unit is compiled with -ffp-contract=off): the output is defined bit for bit, tests/visu_ref.py is the same statement in
// numpy / torch.  DESIGN.md section 4 "Overlays" has the arithmetic and the defined out-of-range behaviour.
//
// Stores: a thread owns 4 consecutive pixels of a row = 12 bytes = three whole dwords when the row starts on a 4-byte boundary
// (the thread's own offset 12 t always is one); it then writes them as one 12-byte vector store.  Row tails and rows that start off
// a 4-byte boundary are written byte by byte.  No dword is ever written by two threads with a dword store.
#include "../../include/wvn_hip.h"

#include "common.h"
#include "wvn_internal.h"

namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_PIX = 4;   // pixels per thread

struct OvArgs {
  wvn_overlay_desc d;
  int npanels;   // plain + nmaps
};

__device__ inline long long ov_id(const void* p, int bytes, size_t i) {
  return bytes == 8 ? ((const long long*)p)[i] : (long long)((const int*)p)[i];
}
// np.uint8(v) where it is defined (truncation inside [0, 255]); outside: clamp, NaN -> 0
__device__ inline unsigned ov_to_u8(float v) { return v >= 255.f ? 255u : (v > 0.f ? (unsigned)v : 0u); }

// PIL.Image.alpha_composite of an opaque destination d with a source s of alpha byte a, per channel
__device__ inline unsigned ov_blend(unsigned s, unsigned d, unsigned a) {
  if (a == 0u) return d;
  const unsigned t = s * (a * 128u) + d * ((255u - a) * 128u) + (0x80u << 7);
  return (((t >> 8) + t) >> 8) >> 7;
}

// (v * 255) truncated and clipped to [0, 255]; a non-finite product gives 0
__device__ inline int ov_index_clipped(float v) {
  const float t = __fmul_rn(v, 255.f);
  if (!(__builtin_fabsf(t) < __builtin_inff())) return 0;
  return t >= 255.f ? 255 : (t > 0.f ? (int)t : 0);
}
// (v * 255) truncated toward zero, not clipped: -1 (no colour) when it is not finite or falls outside [0, N)
__device__ inline int ov_index_open(float v, int N) {
  const float t = __fmul_rn(v, 255.f);
  if (!(__builtin_fabsf(t) < __builtin_inff())) return -1;
  const float tt = truncf(t);
  if (tt < 0.f || tt >= (float)N) return -1;
  return (int)tt;
}

// grid (min(FM_MAX_BLOCKS, ceil(vectors / (256 * FM_ROUNDS))), B): a frame is walked in 16-byte vectors, consecutive lanes on consecutive
// vectors, a block striding over the frame; the last, partial vector and every vector of a frame that does not start on a 16-byte
// boundary are read element by element.  At most FM_MAX_BLOCKS atomics per frame: atomics on one address serialise (one per block of
// 4096 vectors took 30 us for 16 frames of 448 x 448, twice the main kernel).
constexpr int FM_ROUNDS = 4;
constexpr int FM_MAX_BLOCKS = 16;
__global__ __launch_bounds__(OV_THREADS) void frame_max_kernel(const void* __restrict__ img, int img_u8, size_t n, float* __restrict__ fmax) {
  __shared__ int part[OV_THREADS / WVN_WAVE];
  const int b = blockIdx.y;
  const size_t per = img_u8 ? 16 : 4;   // elements per vector
  const unsigned char* base = (const unsigned char*)img + (size_t)b * n * (img_u8 ? 1 : 4);
  const bool aligned = ((uintptr_t)base & 15) == 0;
  const size_t nvec = (n + per - 1) / per;
  float m = 0.f;
  bool nan = false;
  const size_t stride = (size_t)gridDim.x * FM_ROUNDS * OV_THREADS;
  for (size_t v0 = (size_t)blockIdx.x * FM_ROUNDS * OV_THREADS; v0 < nvec; v0 += stride)
#pragma unroll
  for (int r = 0; r < FM_ROUNDS; ++r) {
    const size_t v = v0 + (size_t)r * OV_THREADS + threadIdx.x;
    if (v >= nvec) break;
    const size_t e0 = v * per;
    const size_t e1 = e0 + per < n ? e0 + per : n;
    const bool full = aligned && e0 + per <= n;
    if (img_u8) {
      if (full) {
        const u32x4_t w = *(const u32x4_t*)(base + e0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int k = 0; k < 4; ++k) m = fmaxf(m, (float)((w[j] >> (8 * k)) & 255u));
      } else {
        for (size_t e = e0; e < e1; ++e) m = fmaxf(m, (float)base[e]);
      }
    } else {
      const float* p = (const float*)base;
      if (full) {
        const f32x4_t w = *(const f32x4_t*)(p + e0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          nan |= w[k] != w[k];
          m = w[k] > m ? w[k] : m;
        }
      } else {
        for (size_t e = e0; e < e1; ++e) {
          const float x = p[e];
          nan |= x != x;
          m = x > m ? x : m;
        }
      }
    }
  }
  // m >= +0 or NaN-flagged: the bit patterns order as signed integers, a quiet NaN above +inf
  int key = nan ? 0x7fc00000 : __float_as_int(m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & (WVN_WAVE - 1)) == 0) part[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < OV_THREADS / WVN_WAVE; ++w) key = part[w] > key ? part[w] : key;
    atomicMax((int*)fmax + b, key);
  }
}

__device__ inline void ov_store4(unsigned char* p, const unsigned (&o)[OV_PIX][3], int nv) {
  if (nv == OV_PIX && ((uintptr_t)p & 3) == 0) {
    struct alignas(4) W3 { uint32_t a, b, c; };
    W3 w;
    w.a = o[0][0] | (o[0][1] << 8) | (o[0][2] << 16) | (o[1][0] << 24);
    w.b = o[1][1] | (o[1][2] << 8) | (o[2][0] << 16) | (o[2][1] << 24);
    w.c = o[2][2] | (o[3][0] << 8) | (o[3][1] << 16) | (o[3][2] << 24);
    *(W3*)p = w;
  } else {
#pragma unroll
    for (int j = 0; j < OV_PIX; ++j) {
      if (j >= nv) continue;
      p[3 * j + 0] = (unsigned char)o[j][0];
      p[3 * j + 1] = (unsigned char)o[j][1];
      p[3 * j + 2] = (unsigned char)o[j][2];
    }
  }
}

// grid (ceil(H * ceil(W / 4) / 256), B)
__global__ __launch_bounds__(OV_THREADS) void overlay_kernel(const OvArgs a) {
  __shared__ uint32_t lut[WVN_OVERLAY_MAX_COLOURS];
  const wvn_overlay_desc& d = a.d;
  if (d.nmaps > 0) {
    for (int i = threadIdx.x; i < d.N; i += OV_THREADS) {
      unsigned c[3];
      if (d.lut_u8) {
        const unsigned char* t = (const unsigned char*)d.lut + 3 * (size_t)i;
        c[0] = t[0]; c[1] = t[1]; c[2] = t[2];
      } else {
        const float* t = (const float*)d.lut + 3 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = ov_to_u8(__fmul_rn(t[k], 255.f));
      }
      lut[i] = c[0] | (c[1] << 8) | (c[2] << 16);
    }
    __syncthreads();
  }
  const int W = d.W, H = d.H;
  const int W4 = (W + OV_PIX - 1) / OV_PIX;
  const size_t q = (size_t)blockIdx.x * OV_THREADS + threadIdx.x;
  if (q >= (size_t)H * W4) return;
  const int y = (int)(q / W4), x0 = (int)(q % W4) * OV_PIX;
  const int b = blockIdx.y;
  const int nv = W - x0 < OV_PIX ? W - x0 : OV_PIX;
  const size_t plane = (size_t)H * W;
  const size_t pix = (size_t)b * plane + (size_t)y * W + x0;   // this thread's first pixel in a [B][H][W] map

  // ---- the frame as 8 bits ----
  unsigned px[OV_PIX][3];
  {
    bool scale = d.unit_range > 0;
    if (d.unit_range < 0) scale = d.frame_max[b] <= 1.f;   // (false for the NaN of a frame that holds one, as numpy's max)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t off = ((size_t)b * 3 + c) * plane + (size_t)y * W + x0;
      if (d.img_u8) {
        const unsigned char* p = (const unsigned char*)d.img + off;
        unsigned v[OV_PIX] = {0u, 0u, 0u, 0u};
        if (nv == OV_PIX && ((uintptr_t)p & 3) == 0) {
          const uint32_t w = *(const uint32_t*)p;
#pragma unroll
          for (int j = 0; j < OV_PIX; ++j) v[j] = (w >> (8 * j)) & 255u;
        } else {
#pragma unroll
          for (int j = 0; j < OV_PIX; ++j)
            if (j < nv) v[j] = p[j];
        }
#pragma unroll
        for (int j = 0; j < OV_PIX; ++j) px[j][c] = scale ? (v[j] ? 255u : 0u) : v[j];
      } else {
        const float* p = (const float*)d.img + off;
        float v[OV_PIX] = {0.f, 0.f, 0.f, 0.f};
        if (nv == OV_PIX && ((uintptr_t)p & 15) == 0) {
          const f32x4_t w = *(const f32x4_t*)p;
#pragma unroll
          for (int j = 0; j < OV_PIX; ++j) v[j] = w[j];
        } else {
#pragma unroll
          for (int j = 0; j < OV_PIX; ++j)
            if (j < nv) v[j] = p[j];
        }
#pragma unroll
        for (int j = 0; j < OV_PIX; ++j) px[j][c] = ov_to_u8(scale ? __fmul_rn(v[j], 255.f) : v[j]);
      }
    }
  }

  // ---- what every overlay panel shares: the foreground alpha under the mask, the segment ids, the boundary pixels ----
  unsigned alpha[OV_PIX] = {0u, 0u, 0u, 0u};
  bool bound[OV_PIX] = {false, false, false, false};
  long long sid[OV_PIX] = {-1, -1, -1, -1};
  if (d.nmaps > 0) {
#pragma unroll
    for (int j = 0; j < OV_PIX; ++j)
      if (j < nv) alpha[j] = (d.mask && d.mask[pix + j]) ? 0u : (unsigned)d.alpha;
    if (d.kind == WVN_OVERLAY_SEGMENTS) {
#pragma unroll
      for (int j = 0; j < OV_PIX; ++j) {
        if (j >= nv) continue;
        long long s = ov_id(d.seg, d.seg_bytes, pix + j);
        if (s < 0) s += d.S;                       // ids in [-S, 0) wrap as torch indexing does
        sid[j] = (s >= 0 && s < d.S) ? s : -1;
      }
    }
    if (d.boundary_seg && d.boundary_alpha > 0) {
      const void* bs = d.boundary_seg;
      const int bb = d.boundary_bytes;
#pragma unroll
      for (int j = 0; j < OV_PIX; ++j) {
        if (j >= nv) continue;
        const int x = x0 + j;
        const long long me = ov_id(bs, bb, pix + j);
        bool e = false;
        if (x > 0) e |= ov_id(bs, bb, pix + j - 1) != me;
        if (x + 1 < W) e |= ov_id(bs, bb, pix + j + 1) != me;
        if (y > 0) e |= ov_id(bs, bb, pix + j - W) != me;
        if (y + 1 < H) e |= ov_id(bs, bb, pix + j + W) != me;
        bound[j] = e;
      }
    }
  }

  unsigned char* row = d.out + (size_t)b * (size_t)d.out_frame_bytes + (size_t)y * (size_t)d.out_row_bytes + 3 * (size_t)x0;
  for (int k = 0; k < a.npanels; ++k) {
    unsigned char* dst = row + 3 * (size_t)W * k;
    const int m = k - d.plain;
    if (m < 0) {
      ov_store4(dst, px, nv);
      continue;
    }
    unsigned o[OV_PIX][3];
    u32x4_t raw = {0u, 0u, 0u, 0u};   // the four fp32 values / 32-bit labels of this thread: one 16-byte load where aligned
    const bool words = d.kind == WVN_OVERLAY_VALUES || (d.kind == WVN_OVERLAY_LABELS && d.id_bytes == 4);
    if (words) {
      const uint32_t* p = (const uint32_t*)d.maps[m] + pix;
      if (nv == OV_PIX && ((uintptr_t)p & 15) == 0) {
        raw = *(const u32x4_t*)p;
      } else {
#pragma unroll
        for (int j = 0; j < OV_PIX; ++j)
          if (j < nv) raw[j] = p[j];
      }
    }
#pragma unroll
    for (int j = 0; j < OV_PIX; ++j) {
      long long idx = -1;
      if (j < nv) {
        if (d.kind == WVN_OVERLAY_VALUES) {
          idx = ov_index_clipped(__uint_as_float(raw[j]));
        } else if (d.kind == WVN_OVERLAY_LABELS) {
          idx = words ? (long long)(int)raw[j] : ov_id(d.maps[m], 8, pix + j);
        } else if (sid[j] >= 0) {
          idx = ov_index_open(((const float*)d.maps[m])[(size_t)b * d.S + (size_t)sid[j]], d.N);
        }
      }
      const bool painted = idx >= 0 && idx < d.N;   // an index outside the table: the plain pixel
      const uint32_t col = painted ? lut[idx] : 0u;
      const unsigned al = painted ? alpha[j] : 0u;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        unsigned v = ov_blend((col >> (8 * c)) & 255u, px[j][c], al);
        if (bound[j]) v = ov_blend(255u, v, (unsigned)d.boundary_alpha);
        o[j][c] = v;
      }
    }
    ov_store4(dst, o, nv);
  }
}

int ov_check(const wvn_overlay_desc* d) {
  if (!d || !d->img || !d->out) return WVN_ERR_ARG;
  if (d->B < 1 || d->B > 65535 || d->H < 1 || d->W < 1) return WVN_ERR_ARG;
  if ((long long)d->H * ((d->W + OV_PIX - 1) / OV_PIX) > (long long)0x7fffffff * OV_THREADS) return WVN_ERR_ARG;
  if (d->unit_range < 0 && !d->frame_max) return WVN_ERR_ARG;
  if (d->nmaps < 0 || d->nmaps > WVN_OVERLAY_MAX_MAPS || (d->plain != 0 && d->plain != 1) || d->plain + d->nmaps < 1) return WVN_ERR_ARG;
  if (d->out_row_bytes < 3ll * d->W * (d->plain + d->nmaps) || d->out_frame_bytes < 0) return WVN_ERR_ARG;
  if (d->B > 1 && d->out_frame_bytes < d->out_row_bytes * (long long)(d->H - 1) + 3ll * d->W * (d->plain + d->nmaps)) return WVN_ERR_ARG;
  if (d->nmaps > 0) {
    if (!d->lut || d->N < 1 || d->N > WVN_OVERLAY_MAX_COLOURS) return WVN_ERR_ARG;
    if (d->alpha < 0 || d->alpha > 255 || d->boundary_alpha < 0 || d->boundary_alpha > 255) return WVN_ERR_ARG;
    if (d->kind != WVN_OVERLAY_VALUES && d->kind != WVN_OVERLAY_LABELS && d->kind != WVN_OVERLAY_SEGMENTS) return WVN_ERR_ARG;
    for (int m = 0; m < d->nmaps; ++m)
      if (!d->maps[m]) return WVN_ERR_ARG;
    if (d->kind == WVN_OVERLAY_LABELS && d->id_bytes != 4 && d->id_bytes != 8) return WVN_ERR_ARG;
    if (d->kind == WVN_OVERLAY_SEGMENTS && (!d->seg || d->S < 1 || (d->seg_bytes != 4 && d->seg_bytes != 8))) return WVN_ERR_ARG;
    if (d->boundary_seg && d->boundary_bytes != 4 && d->boundary_bytes != 8) return WVN_ERR_ARG;
  }
  return WVN_OK;
}

int ov_launch(const wvn_overlay_desc* d, void* stream) {
  OvArgs a;
  a.d = *d;
  a.npanels = d->plain + d->nmaps;
  const long long groups = (long long)d->H * ((d->W + OV_PIX - 1) / OV_PIX);
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)((groups + OV_THREADS - 1) / OV_THREADS), d->B), dim3(OV_THREADS), 0, (hipStream_t)stream, a);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // namespace

extern "C" int wvn_frame_max(const void* img, int img_u8, int B, long long n, float* frame_max, void* stream) {
  if (!img || !frame_max || B < 1 || B > 65535 || n < 1) return WVN_ERR_ARG;
  const long long per = img_u8 ? 16 : 4, nvec = (n + per - 1) / per;
  long long blocks = (nvec + OV_THREADS * FM_ROUNDS - 1) / (OV_THREADS * FM_ROUNDS);
  if (blocks > FM_MAX_BLOCKS) blocks = FM_MAX_BLOCKS;
  hipError_t e = hipMemsetAsync(frame_max, 0, sizeof(float) * (size_t)B, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(frame_max_kernel, dim3((unsigned)blocks, B), dim3(OV_THREADS), 0, (hipStream_t)stream, img, img_u8, (size_t)n, frame_max);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

extern "C" int wvn_overlay(const wvn_overlay_desc* d, void* stream) {
  const int rc = ov_check(d);
  if (rc != WVN_OK) return rc;
  if (d->plain != 0 || d->nmaps != 1) return WVN_ERR_ARG;
  return ov_launch(d, stream);
}

extern "C" int wvn_overlay_panels(const wvn_overlay_desc* d, void* stream) {
  const int rc = ov_check(d);
  if (rc != WVN_OK) return rc;
  if (d->plain != 1) return WVN_ERR_ARG;
  return ov_launch(d, stream);
}
