// The multi-scale branch of sparsify_features (feature_extractor.py:314-366 of the reference) for the four ResNet-18 level maps: the
// four pooled blocks of feat [B][S][960] written directly from the NHWC level maps (64, 128, 256, 512 channels at strides 4, 8, 16, 32)
// and the int32 segment map [B][H][W].  No full-resolution tensor, no floating-point atomics.  The definition (include/wvn_hip.h;
// tests/resnet_ref.py states it in float64), per level with stride s and grid h x w = H / s x W / s:
//   row i = the mean of the level's vectors over the cells (cy, cx) with seg[cy s][cx s] == i   (F.interpolate(seg, scale_factor=1/s));
//   no such cell (the published code cannot run then): the vector of the cell (min(Cy / s, h - 1), min(Cx / s, w - 1)) that holds the
//   segment's centroid Cy = floor(sum of its pixel rows / its pixel count), Cx likewise, in integers at full resolution;
//   an id without a pixel: NaN.  Ids outside [0, S) are ignored.
//
//   pyramid_stats_kernel  one pass over seg: per (frame, id) the pixel count, the row and column sums and the bounding box.  A thread
//       walks 16 pixels of a row and issues one set of INTEGER atomics per run of equal ids (order-free).
//   pyramid_pool_kernel   one wave per (id, level, frame).  It walks the level's cells inside the id's bounding box in raster order, 64
//       at a time: each lane tests one cell's sample pixel, the ballot of the matches is then consumed bit by bit in ascending order, the
//       lanes adding channels lane, lane + 64, ... of that cell in float64.  The order of the additions is the raster order of the cells,
//       whatever the batch or the other segments: the means are reproducible bit for bit, and float(float64 sum / count) is within half
//       an ulp of the exact mean.  A fallback row is a copy of the level map's cell.
#include "../../include/wvn_hip.h"

#include "common.h"

namespace {

constexpr int RUN = 16;       // pixels per thread of the statistics pass
constexpr int FEAT = 960;     // 64 + 128 + 256 + 512

struct Levels {
  const float* map[4];
};

// st [B * S][3] = {count, sum of rows, sum of columns}; lo [B * S][2] = {min row, min column} (preset to 0x7f7f7f7f); hi likewise (0)
__global__ __launch_bounds__(256) void pyramid_stats_kernel(const int* __restrict__ seg, unsigned long long* __restrict__ st,
                                                            int* __restrict__ lo, int* __restrict__ hi, int H, int W, int S,
                                                            int chunks, long long total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int xc = (int)(t % chunks);
  const long long row = t / chunks;           // b * H + y
  const int y = (int)(row % H);
  const long long b = row / H;
  const int x0 = xc * RUN, x1 = min(x0 + RUN, W);
  const int* p = seg + (size_t)row * W;
  int cur = -1, n = 0, xs = 0;
  unsigned long long sx = 0;
  for (int x = x0; x <= x1; ++x) {
    int l = -1;
    if (x < x1) {
      l = p[x];
      if (l < 0 || l >= S) l = -1;
    }
    if (l != cur) {
      if (cur >= 0) {
        const size_t e = (size_t)b * S + cur;
        atomicAdd(st + 3 * e, (unsigned long long)n);
        atomicAdd(st + 3 * e + 1, (unsigned long long)n * (unsigned long long)y);
        atomicAdd(st + 3 * e + 2, sx);
        atomicMin(lo + 2 * e, y);
        atomicMin(lo + 2 * e + 1, xs);
        atomicMax(hi + 2 * e, y);
        atomicMax(hi + 2 * e + 1, x - 1);
      }
      cur = l;
      n = 0;
      sx = 0;
      xs = x;
    }
    if (l >= 0) {
      ++n;
      sx += (unsigned long long)x;
    }
  }
}

// grid (S, 4, B), one wave
__global__ __launch_bounds__(64) void pyramid_pool_kernel(const Levels lv, const int* __restrict__ seg,
                                                          const unsigned long long* __restrict__ st, const int* __restrict__ lo,
                                                          const int* __restrict__ hi, float* __restrict__ feat, int H, int W, int S) {
  const int lane = threadIdx.x;
  const int id = blockIdx.x, level = blockIdx.y, b = blockIdx.z;
  const int s = 4 << level, C = 64 << level, nper = 1 << level;
  const int h = H / s, w = W / s;
  const float* map = lv.map[level] + (size_t)b * h * w * C;
  const int* sg = seg + (size_t)b * H * W;
  const size_t e = (size_t)b * S + id;
  float* out = feat + e * FEAT + (C - 64);     // column offsets 0, 64, 192, 448
  const unsigned long long n = st[3 * e];
  if (n == 0) {
    for (int q = 0; q < nper; ++q) out[lane + 64 * q] = __builtin_nanf("");
    return;
  }
  const int cy0 = (lo[2 * e] + s - 1) / s, cx0 = (lo[2 * e + 1] + s - 1) / s;   // the cells whose sample pixel lies in the bounding box
  const int cy1 = hi[2 * e] / s, cx1 = hi[2 * e + 1] / s;
  double acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.0;
  int count = 0;
  if (cy0 <= cy1 && cx0 <= cx1) {
    const int bw = cx1 - cx0 + 1;
    const int ncell = bw * (cy1 - cy0 + 1);
    for (int base = 0; base < ncell; base += 64) {
      const int c = base + lane;
      bool match = false;
      if (c < ncell) {
        const int cy = cy0 + c / bw, cx = cx0 + c % bw;
        match = sg[(size_t)cy * s * W + cx * s] == id;
      }
      unsigned long long mask = __ballot(match);
      count += __popcll(mask);
      while (mask) {
        const int j = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const int cj = base + j;
        const float* p = map + ((size_t)(cy0 + cj / bw) * w + cx0 + cj % bw) * C + lane;
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (q < nper) acc[q] += (double)p[64 * q];
      }
    }
  }
  if (count > 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (q < nper) out[lane + 64 * q] = (float)(acc[q] / (double)count);
  } else {
    const int cy = min((int)(st[3 * e + 1] / n) / s, h - 1), cx = min((int)(st[3 * e + 2] / n) / s, w - 1);
    const float* p = map + ((size_t)cy * w + cx) * C + lane;
    for (int q = 0; q < nper; ++q) out[lane + 64 * q] = p[64 * q];
  }
}

bool pool_shape_ok(int B, int H, int W, int S) {
  return B >= 1 && B <= 65535 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0 && H <= 8192 && W <= 8192 && S >= 1 &&
         S <= WVN_SEGPOOL_PYRAMID_MAX_SEGMENTS && (long long)B * S * FEAT < (1ll << 31);
}

}  // namespace

size_t wvn_segpool_pyramid_scratch_bytes(int B, int S) {
  if (B < 1 || S < 1 || B > 65535 || S > WVN_SEGPOOL_PYRAMID_MAX_SEGMENTS) return 0;
  return (size_t)B * S * (3 * sizeof(unsigned long long) + 4 * sizeof(int));
}

int wvn_segpool_pyramid(const float* feat1, const float* feat2, const float* feat3, const float* feat4, const int* seg, float* feat,
                        void* scratch, size_t scratch_bytes, int B, int H, int W, int S, void* stream) {
  if (!feat1 || !feat2 || !feat3 || !feat4 || !seg || !feat || !scratch || !pool_shape_ok(B, H, W, S)) return WVN_ERR_ARG;
  if (scratch_bytes < wvn_segpool_pyramid_scratch_bytes(B, S)) return WVN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const size_t ns = (size_t)B * S;
  unsigned long long* stats = (unsigned long long*)scratch;
  int* hi = (int*)(stats + 3 * ns);
  int* lo = hi + 2 * ns;
  hipError_t e = hipMemsetAsync(stats, 0, ns * (3 * sizeof(unsigned long long) + 2 * sizeof(int)), st);   // the sums and hi
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(lo, 0x7f, ns * 2 * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const int chunks = ceil_div(W, RUN);
  const long long total = (long long)B * H * chunks;
  hipLaunchKernelGGL(pyramid_stats_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, seg, stats, lo, hi, H, W, S, chunks,
                     total);
  WVN_LAUNCH_CHECK();
  Levels lv;
  lv.map[0] = feat1;
  lv.map[1] = feat2;
  lv.map[2] = feat3;
  lv.map[3] = feat4;
  hipLaunchKernelGGL(pyramid_pool_kernel, dim3(S, 4, B), dim3(64), 0, st, lv, seg, (const unsigned long long*)stats, (const int*)lo,
                     (const int*)hi, feat, H, W, S);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
