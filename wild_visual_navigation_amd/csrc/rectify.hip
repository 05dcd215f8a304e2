// Raw camera ingest (include/wvn_hip.h: "Raw camera ingest"): source frames as the camera driver publishes them (mono8, packed rgb8 /
// bgr8, planar, the four 8-bit Bayer mosaics; rows of `step` bytes) -> planar uint8 frames, either at full resolution
// (wvn_unpack_frames: the demosaic / the HWC -> planar unpack on its own) or resampled through a Q5 rectification map
// (wvn_rectify_frames: demosaic at the taps + bilinear remap in one launch, no full-resolution RGB frame in between).
// Integers only, no atomics, no host synchronisation; tests/rectify_ref.py is the definition, bit for bit.
//
// Thread-to-pixel mapping: one thread owns PX = 4 horizontally adjacent output pixels of one row, so each output plane gets ONE dword
// store per thread (a wave stores 256 contiguous bytes per plane and row) where byte-wide stores would issue four; the map is read as
// two 16-byte loads per thread.  A group that crosses the end of the row, or whose address is not dword aligned (w % 4 != 0 moves
// the rows), takes the scalar path.  The source window of a tile is NOT staged in LDS: under a fisheye map its footprint is data
// dependent (a 256 x 4 output tile of the 448 x 448 crop covers some 600 x 10 source pixels at the centre and far fewer at the rim),
// the 1.5 MB raw frame stays resident in every XCD's 4 MiB L2, and neighbouring lanes read neighbouring bytes, so the vector cache
// serves the 16 raw bytes of a pixel's 4 x 4 window, read as four 4-byte loads of any alignment (one per window row: byte-wide loads
// made the kernel load-issue bound and 1.4 - 1.7x slower); there is no reuse LDS would add that L1 / L2 do not already give.
#include <stdint.h>

#ifndef WVN_RECTIFY_HOST_BUILD   // (tests/rectify_host_main.cpp compiles this file as plain C++, every thread in turn, under the sanitizers)
#include "common.h"
#include "wvn_internal.h"
#endif
#include "../../include/wvn_hip.h"

namespace {

constexpr int PX = 4;                // output pixels per thread: one dword per plane
constexpr int TX = 64, TY = 4;       // threads per workgroup: 256 x 4 pixels

enum SrcClass { SRC_MONO = 0, SRC_PACKED = 1, SRC_PLANAR = 2, SRC_BAYER = 3 };

struct Source {
  const uint8_t* p;        // frame 0
  long long frame_stride;  // bytes between frames
  int H, W, step;
  int c0;                  // packed: byte of R inside a pixel (0 rgb8, 2 bgr8)
  int ry, rx;              // Bayer: row and column parity of the R sites
};

struct OutOrder {
  int nout;    // output planes: 1 (mono8 kept as one plane) or 3
  int ch[3];   // the source channel of output plane k
};

// bilinear demosaic of an interior site from its 3 x 3 raw neighbourhood (n[1][1] is the site)
__device__ __forceinline__ void demosaic9(const int n[3][3], bool red_row, bool own, int rgb[3]) {
  const int c = n[1][1];
  // an R / B site: its own colour, G from the cross, the opposite colour from the diagonals; a G site: its row's colour from left and
  // right, the other from above and below.  `mine`: the colour of this row's R / B sites, `other`: the other of R and B
  const int g = own ? (n[0][1] + n[2][1] + n[1][0] + n[1][2] + 2) >> 2 : c;
  const int mine = own ? c : (n[1][0] + n[1][2] + 1) >> 1;
  const int other = own ? (n[0][0] + n[0][2] + n[2][0] + n[2][2] + 2) >> 2 : (n[0][1] + n[2][1] + 1) >> 1;
  rgb[0] = red_row ? mine : other;
  rgb[1] = g;
  rgb[2] = red_row ? other : mine;
}

// the source value of every channel at (y, x); a pixel outside the frame is 0.  NC = 1 for SRC_MONO, 3 otherwise.
template <int KIND>
__device__ __forceinline__ void fetch(const Source& s, const uint8_t* f, int y, int x, int rgb[3]) {
  rgb[0] = rgb[1] = rgb[2] = 0;
  if (y < 0 || y >= s.H || x < 0 || x >= s.W) return;
  if (KIND == SRC_MONO) {
    rgb[0] = f[y * s.step + x];
  } else if (KIND == SRC_PACKED) {
    const uint8_t* q = f + y * s.step + 3 * x;
    rgb[0] = q[s.c0];
    rgb[1] = q[1];
    rgb[2] = q[2 - s.c0];
  } else if (KIND == SRC_PLANAR) {
    const int o = y * s.step + x, plane = s.H * s.step;
    rgb[0] = f[o];
    rgb[1] = f[o + plane];
    rgb[2] = f[o + 2 * plane];
  } else {
    // the one-pixel ring takes the RESULT of its inner neighbour (columns first, then rows: a corner takes the diagonal one)
    const int cy = min(max(y, 1), s.H - 2), cx = min(max(x, 1), s.W - 2);
    int n[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) n[a][b] = f[(cy - 1 + a) * s.step + cx - 1 + b];
    const bool red_row = (cy & 1) == s.ry;
    demosaic9(n, red_row, ((cx & 1) == s.rx) == red_row, rgb);
  }
}

// PX results of one thread -> the output planes
__device__ __forceinline__ void store_group(uint8_t* out, size_t plane_elems, size_t o, const OutOrder& oo, int valid,
                                            const int res[PX][3]) {
  uint32_t packed[3];   // the PX bytes of every source channel, pixel 0 in the low byte
#pragma unroll
  for (int c = 0; c < 3; ++c)
    packed[c] = (uint32_t)res[0][c] | ((uint32_t)res[1][c] << 8) | ((uint32_t)res[2][c] << 16) | ((uint32_t)res[3][c] << 24);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k >= oo.nout) break;
    uint8_t* q = out + (size_t)k * plane_elems + o;
    const uint32_t v = oo.ch[k] == 0 ? packed[0] : oo.ch[k] == 1 ? packed[1] : packed[2];
    if (valid == PX && (reinterpret_cast<uintptr_t>(q) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(q) = v;
    } else {
      for (int j = 0; j < valid; ++j) q[j] = (uint8_t)(v >> (8 * j));
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(TX* TY) void unpack_kernel(Source s, uint8_t* out, OutOrder oo) {
  const int x0 = (blockIdx.x * TX + threadIdx.x) * PX, y = blockIdx.y * TY + threadIdx.y, b = blockIdx.z;
  if (x0 >= s.W || y >= s.H) return;
  const uint8_t* f = s.p + (size_t)b * s.frame_stride;
  const int valid = min(PX, s.W - x0);
  int res[PX][3];
  if (KIND == SRC_BAYER && y >= 1 && y <= s.H - 2 && x0 >= 1 && x0 + PX - 1 <= s.W - 2) {
    int win[3][PX + 2];   // the interior: the PX sites share a 3 x (PX + 2) window
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      uint32_t lo;   // the six bytes of a window row in two loads (any alignment; memcpy keeps it plain C++)
      uint16_t hi;
      __builtin_memcpy(&lo, f + (y - 1 + a) * s.step + x0 - 1, 4);
      __builtin_memcpy(&hi, f + (y - 1 + a) * s.step + x0 + 3, 2);
#pragma unroll
      for (int i = 0; i < 4; ++i) win[a][i] = (lo >> (8 * i)) & 0xff;
      win[a][4] = hi & 0xff;
      win[a][5] = hi >> 8;
    }
    const bool red_row = (y & 1) == s.ry;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      int n[3][3];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int i = 0; i < 3; ++i) n[a][i] = win[a][j + i];
      demosaic9(n, red_row, (((x0 + j) & 1) == s.rx) == red_row, res[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < PX; ++j) fetch<KIND>(s, f, y, x0 + j, res[j]);   // (x0 + j >= W gives 0 and is not stored)
  }
  const size_t plane = (size_t)s.H * s.W;
  store_group(out, plane, (size_t)b * oo.nout * plane + (size_t)y * s.W + x0, oo, valid, res);
}

template <int KIND>
__global__ __launch_bounds__(TX* TY) void rectify_kernel(Source s, const int* __restrict__ qx, const int* __restrict__ qy, int h,
                                                         int w, uint8_t* out, OutOrder oo) {
  const int x0 = (blockIdx.x * TX + threadIdx.x) * PX, v = blockIdx.y * TY + threadIdx.y, b = blockIdx.z;
  if (x0 >= w || v >= h) return;
  const uint8_t* f = s.p + (size_t)b * s.frame_stride;
  const int valid = min(PX, w - x0);
  const size_t m = (size_t)v * w + x0;
  int mx[PX], my[PX];
  if (valid == PX && ((reinterpret_cast<uintptr_t>(qx + m) | reinterpret_cast<uintptr_t>(qy + m)) & 15) == 0) {
    const int4 a = *reinterpret_cast<const int4*>(qx + m), c = *reinterpret_cast<const int4*>(qy + m);
    mx[0] = a.x, mx[1] = a.y, mx[2] = a.z, mx[3] = a.w;
    my[0] = c.x, my[1] = c.y, my[2] = c.z, my[3] = c.w;
  } else {
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      mx[j] = j < valid ? qx[m + j] : -64;   // (-2 in Q5: all taps outside; never stored)
      my[j] = j < valid ? qy[m + j] : -64;
    }
  }
  constexpr int NC = KIND == SRC_MONO ? 1 : 3;
  int res[PX][3];
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const int ix = mx[j] >> 5, iy = my[j] >> 5, ax = mx[j] & 31, ay = my[j] & 31;
    const int wt[2][2] = {{(32 - ax) * (32 - ay), ax * (32 - ay)}, {(32 - ax) * ay, ax * ay}};   // sums to 1024
    int acc[3] = {512, 512, 512};
    if (KIND == SRC_BAYER && iy >= 1 && iy + 1 <= s.H - 2 && ix >= 1 && ix + 1 <= s.W - 2) {
      int win[4][4];   // four interior taps: their 3 x 3 neighbourhoods are one 4 x 4 raw window
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        uint32_t row;   // the four bytes of a window row in one load (any alignment; memcpy keeps it plain C++)
        __builtin_memcpy(&row, f + (iy - 1 + a) * s.step + ix - 1, 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) win[a][i] = (row >> (8 * i)) & 0xff;
      }
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          int n[3][3], rgb[3];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i) n[a][i] = win[dy + a][dx + i];
          const bool red_row = ((iy + dy) & 1) == s.ry;
          demosaic9(n, red_row, (((ix + dx) & 1) == s.rx) == red_row, rgb);
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += wt[dy][dx] * rgb[c];
        }
    } else {
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          int rgb[3];
          fetch<KIND>(s, f, iy + dy, ix + dx, rgb);
#pragma unroll
          for (int c = 0; c < NC; ++c) acc[c] += wt[dy][dx] * rgb[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) res[j][c] = acc[c] >> 10;   // <= (1024 * 255 + 512) >> 10 = 255
  }
  const size_t plane = (size_t)h * w;
  store_group(out, plane, (size_t)b * oo.nout * plane + m, oo, valid, res);
}

// argument checks shared by the two entry points: the source description and the output order
int describe(const void* src, int kind, int B, int H, int W, long long step, long long frame_stride, int order, Source* s, OutOrder* oo,
             int* cls) {
  if (!src || B < 1 || B > 65535 || H > WVN_FRAME_MAX_DIM || W > WVN_FRAME_MAX_DIM) return WVN_ERR_ARG;
  if (kind < WVN_SRC_MONO8 || kind > WVN_SRC_BAYER_GRBG8) return WVN_ERR_ARG;
  const bool bayer = kind >= WVN_SRC_BAYER_RGGB8;
  const int least = bayer ? 3 : 1;
  if (H < least || W < least) return WVN_ERR_ARG;
  const int bpp = (kind == WVN_SRC_RGB8 || kind == WVN_SRC_BGR8) ? 3 : 1;
  const long long rows = kind == WVN_SRC_PLANAR ? 3ll * H : H;
  if (step < (long long)W * bpp || step > INT32_MAX) return WVN_ERR_ARG;
  const long long frame_bytes = (rows - 1) * step + (long long)W * bpp;   // what the kernels read of one frame
  if (frame_bytes > INT32_MAX || frame_stride < frame_bytes || frame_stride > INT32_MAX || frame_stride * B > INT32_MAX)
    return WVN_ERR_ARG;
  const bool mono = kind == WVN_SRC_MONO8;
  if (order != WVN_ORDER_RGB && order != WVN_ORDER_BGR && !(order == WVN_ORDER_GRAY && mono)) return WVN_ERR_ARG;
  s->p = (const uint8_t*)src;
  s->frame_stride = frame_stride;
  s->H = H, s->W = W, s->step = (int)step;
  s->c0 = kind == WVN_SRC_BGR8 ? 2 : 0;
  s->ry = (kind == WVN_SRC_BAYER_BGGR8 || kind == WVN_SRC_BAYER_GBRG8) ? 1 : 0;
  s->rx = (kind == WVN_SRC_BAYER_BGGR8 || kind == WVN_SRC_BAYER_GRBG8) ? 1 : 0;
  oo->nout = order == WVN_ORDER_GRAY ? 1 : 3;
  for (int k = 0; k < 3; ++k) oo->ch[k] = mono ? 0 : (order == WVN_ORDER_BGR ? 2 - k : k);
  *cls = mono ? SRC_MONO : bayer ? SRC_BAYER : kind == WVN_SRC_PLANAR ? SRC_PLANAR : SRC_PACKED;
  return WVN_OK;
}

dim3 grid_of(int h, int w, int B) { return dim3((unsigned)((w + TX * PX - 1) / (TX * PX)), (unsigned)((h + TY - 1) / TY), (unsigned)B); }

}  // namespace

extern "C" {

int wvn_unpack_frames(const void* src, int kind, int B, int H, int W, long long step, long long frame_stride, void* out_u8, int order,
                      void* stream) {
  Source s;
  OutOrder oo;
  int cls;
  if (!out_u8 || describe(src, kind, B, H, W, step, frame_stride, order, &s, &oo, &cls)) return WVN_ERR_ARG;
  if ((long long)B * oo.nout * H * W > INT32_MAX) return WVN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* out = (uint8_t*)out_u8;
  const dim3 grid = grid_of(H, W, B), block(TX, TY);
  switch (cls) {
    case SRC_MONO: hipLaunchKernelGGL(unpack_kernel<SRC_MONO>, grid, block, 0, st, s, out, oo); break;
    case SRC_PACKED: hipLaunchKernelGGL(unpack_kernel<SRC_PACKED>, grid, block, 0, st, s, out, oo); break;
    case SRC_PLANAR: hipLaunchKernelGGL(unpack_kernel<SRC_PLANAR>, grid, block, 0, st, s, out, oo); break;
    default: hipLaunchKernelGGL(unpack_kernel<SRC_BAYER>, grid, block, 0, st, s, out, oo); break;
  }
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_rectify_frames(const void* src, int kind, int B, int H, int W, long long step, long long frame_stride, const int* map_qx,
                       const int* map_qy, int h, int w, void* out_u8, int order, void* stream) {
  Source s;
  OutOrder oo;
  int cls;
  if (!out_u8 || !map_qx || !map_qy || h < 1 || w < 1 || h > WVN_FRAME_MAX_DIM || w > WVN_FRAME_MAX_DIM || describe(src, kind, B, H, W, step, frame_stride, order, &s, &oo, &cls))
    return WVN_ERR_ARG;
  if ((long long)h * w * 4 > INT32_MAX || (long long)B * oo.nout * h * w > INT32_MAX) return WVN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* out = (uint8_t*)out_u8;
  const dim3 grid = grid_of(h, w, B), block(TX, TY);
  switch (cls) {
    case SRC_MONO: hipLaunchKernelGGL(rectify_kernel<SRC_MONO>, grid, block, 0, st, s, map_qx, map_qy, h, w, out, oo); break;
    case SRC_PACKED: hipLaunchKernelGGL(rectify_kernel<SRC_PACKED>, grid, block, 0, st, s, map_qx, map_qy, h, w, out, oo); break;
    case SRC_PLANAR: hipLaunchKernelGGL(rectify_kernel<SRC_PLANAR>, grid, block, 0, st, s, map_qx, map_qy, h, w, out, oo); break;
    default: hipLaunchKernelGGL(rectify_kernel<SRC_BAYER>, grid, block, 0, st, s, map_qx, map_qy, h, w, out, oo); break;
  }
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // extern "C"
