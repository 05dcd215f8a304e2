// Traversability grid map (include/wvn_hip.h: "Traversability grid map"): the per-pixel traversability / confidence images of the
// cameras painted onto the robot-centric elevation grid (wvn_grid_fuse_images), the exact signed distance field of a thresholded
// layer (wvn_grid_sdf) and the goal selection of the reference's smart_carrot.py on that field (wvn_grid_carrot).  One launch each,
// no atomics, no workspace, no host synchronisation; tests/grid_map_ref.py states all three in numpy and the results are that
// statement BIT FOR BIT (this file is compiled with -ffp-contract=off: every fp32 operation below is rounded on its own).
//
// Grid: square, N x N, axis 0 = map x, axis 1 = map y, row-major; cell (i, j) is centred at
//   x = cx + (float(i) - N * 0.5f) * r,   y = cy + (float(j) - N * 0.5f) * r            (smart_carrot.py:145-150)
// A layer is fp32 [N][N]; NaN = unknown.
//
// ---- fusion: one thread owns one cell and applies the cameras b = 0 .. B-1 in order ----
// The projection is the fp32 order csrc/supervision.hip documents (kornia's transform_points / PinholeCamera.project), restated:
//   T_cw         = rigid inverse of pose_cam_in_world T: row k of R^T is column k of R, t_cw[k] = -((R[0][k] t0 + R[1][k] t1) + R[2][k] t2)
//   p_c[k]       = ((R[0][k] X + R[1][k] Y) + R[2][k] Z) + t_cw[k]                       with (X, Y, Z) = (x, y, elevation)
//   (x', y', z') = ((K[m][0] p_c0 + K[m][1] p_c1) + K[m][2] p_c2) + K[m][3],  m = 0, 1, 2
//   u = x' * s, v = y' * s,  s = |z'| > 1e-8 ? 1 / (z' + 1e-8) : 1
// The camera is skipped unless p_c2 > min_depth, the nearest pixel (floorf(u + 0.5f), floorf(v + 0.5f)) lies inside the image and the
// horizontal distance L = sqrtf(dx dx + dy dy), (dx, dy, dz) = camera position - (x, y, elevation), is <= max_range.
// Visibility: step = r / L;  for s = 1 .. (int)floorf(L / r):  t = float(s) * step,  q = (x + t dx, y + t dy, elevation + t dz);
//   the nearest cell (floorf((q_x - cx) * (1 / r) + (N * 0.5f + 0.5f)), likewise y); outside the map -> the walk ends, visible;
//   that cell's elevation finite and (elevation - q_z) > occlusion_margin -> occluded.
// Fusion, per channel c whose sample is not NaN:  new = old is NaN ? value : old * (1 - alpha) + alpha * value;  hits += 1 when a
// channel was fused.  (A camera whose samples are all NaN changes nothing, so its walk is not taken.)
//
// The elevation layer is read through the caches, not staged in LDS: one 8 x 8 tile of cells per wave walks a narrow fan of rays, so
// the lines it touches are few and shared between its lanes.  The staged form (32 x 32 cells per 1024-thread workgroup, the 160 000-byte
// layer copied to LDS first, the walk reading it there; the same bits) was measured at N = 200, two 448 x 448 cameras: 67 us against
// 60 us for this one (profiles/grid_map.md) -- 49 fat workgroups on 49 of 256 CUs, each paying the copy, and no layer above N = 202.
//
// ---- signed distance field: separable exact Euclidean distance transform in integers, one workgroup per grid row ----
// Obstacle set O = {value < threshold}; an unknown (NaN) cell joins O, the free set F, or neither (unknown = 0, 1, 2).  For row i,
// thread k scans column k and keeps the smallest (i' - i)^2 over the cells of O and of F (the column pass, recomputed per row instead of
// stored: no workspace, no grid-wide boundary, the layer is L2 resident), the two rows g_O, g_F go to LDS, and cell (i, j) takes
// min over k of (j - k)^2 + g(k) against the OTHER set.  d2 > 0 free, < 0 obstacle, 0 = in neither set (sdf NaN);
// no cell in the other set: d2 = +-INT32_MAX, sdf = +-inf.  sdf = +-(r * sqrtf(float(|d2|))).
//
// ---- smart carrot (smart_carrot.py:53-94, 126-150), ONE workgroup ----
// score = sdf;  c = N / 2 (integer)
//   distance force (factor > 0):  score = score + (sqrtf(float((i-c)^2 + (j-c)^2)) / sqrtf(float(2 c c))) * factor
//   centre force   (factor > 0):  score = score - fabsf(cos * float(j-c) - sin * float(i-c)) * factor     [np.meshgrid: x is the column]
//   outside every disc (i - ci)^2 + (j - cj)^2 <= radius^2, ci = int(N/2 + cos * distance), cj = int(N/2 + sin * distance)
//   [cv2.circle's point is (column, row)], or a NaN elevation in the 3 x 3 neighbourhood (cells outside the grid ignored), or NaN -> -inf
// arg-max with ties to the lowest row-major index: a 64-bit key (order-preserving image of the score, ~index) reduced by max.
// A 200 x 200 map is 40 cells per thread of one 1024-thread workgroup; a second launch or an atomic with its memset would cost more
// than the loop.
#include <stdint.h>
#include <math.h>

#include "common.h"
#include "wvn_internal.h"
#include "../../include/wvn_hip.h"

namespace {

constexpr int TILE = 8;   // fusion: 8 x 8 cells per wave

struct FuseArgs {
  const float* maps;    // [B][C][H][W]
  const float* K;       // [B][4][4]
  const float* pose;    // [B][4][4]
  const float* elev;    // [N][N]
  float* layers[WVN_GRID_MAX_CHANNELS];
  int* hits;
  int B, C, H, W, N;
  float cx, cy, r, alpha, min_depth, max_range, margin;
};

__global__ __launch_bounds__(TILE * TILE) void grid_fuse_kernel(const FuseArgs a) {
  const int N = a.N;
  const int i = blockIdx.y * TILE + (threadIdx.x >> 3), j = blockIdx.x * TILE + (threadIdx.x & 7);
  if (i >= N || j >= N) return;
  const size_t cell = (size_t)i * N + j;
  const float e = a.elev[cell];
  if (e != e) return;
  const float half = (float)N * 0.5f, hp = half + 0.5f, inv_r = 1.0f / a.r, oma = 1.0f - a.alpha;
  const float x = a.cx + ((float)i - half) * a.r, y = a.cy + ((float)j - half) * a.r;
  float old[WVN_GRID_MAX_CHANNELS];
#pragma unroll
  for (int c = 0; c < WVN_GRID_MAX_CHANNELS; ++c) old[c] = c < a.C ? a.layers[c][cell] : 0.f;
  int nhits = 0;
  for (int b = 0; b < a.B; ++b) {
    const float* T = a.pose + (size_t)b * 16;
    const float* K = a.K + (size_t)b * 16;
    float pc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float r0 = T[0 * 4 + k], r1 = T[1 * 4 + k], r2 = T[2 * 4 + k];
      const float tc = -((r0 * T[3] + r1 * T[7]) + r2 * T[11]);
      pc[k] = ((r0 * x + r1 * y) + r2 * e) + tc;
    }
    if (!(pc[2] > a.min_depth)) continue;
    const float xp = ((K[0] * pc[0] + K[1] * pc[1]) + K[2] * pc[2]) + K[3];
    const float yp = ((K[4] * pc[0] + K[5] * pc[1]) + K[6] * pc[2]) + K[7];
    const float zp = ((K[8] * pc[0] + K[9] * pc[1]) + K[10] * pc[2]) + K[11];
    const float s = fabsf(zp) > 1e-8f ? 1.0f / (zp + 1e-8f) : 1.0f;
    const float pu = floorf(xp * s + 0.5f), pv = floorf(yp * s + 0.5f);
    if (!(pu >= 0.f && pu < (float)a.W && pv >= 0.f && pv < (float)a.H)) continue;
    const float dx = T[3] - x, dy = T[7] - y, dz = T[11] - e;
    const float L = sqrtf(dx * dx + dy * dy);
    if (!(L <= a.max_range)) continue;
    const float* px = a.maps + (((size_t)b * a.C) * a.H + (size_t)(int)pv) * a.W + (size_t)(int)pu;
    const size_t plane = (size_t)a.H * a.W;
    float val[WVN_GRID_MAX_CHANNELS];
    bool any = false;
#pragma unroll
    for (int c = 0; c < WVN_GRID_MAX_CHANNELS; ++c) {
      val[c] = c < a.C ? px[c * plane] : __builtin_nanf("");
      any |= val[c] == val[c];
    }
    if (!any) continue;
    const float step = a.r / L;
    const int nsteps = (int)floorf(L / a.r);   // (L == 0: step is inf and L / r is 0 -- no step is taken)
    bool visible = true;
    for (int k = 1; k <= nsteps; ++k) {
      const float t = (float)k * step;
      const float qx = x + t * dx, qy = y + t * dy, qz = e + t * dz;
      const float fi = floorf((qx - a.cx) * inv_r + hp), fj = floorf((qy - a.cy) * inv_r + hp);
      if (!(fi >= 0.f && fi < (float)N && fj >= 0.f && fj < (float)N)) break;
      const float he = a.elev[(int)fi * N + (int)fj];
      if (fabsf(he) <= 3.402823466e+38f && he - qz > a.margin) { visible = false; break; }
    }
    if (!visible) continue;
#pragma unroll
    for (int c = 0; c < WVN_GRID_MAX_CHANNELS; ++c)
      if (val[c] == val[c]) old[c] = old[c] != old[c] ? val[c] : old[c] * oma + a.alpha * val[c];
    ++nhits;
  }
  if (nhits) {
#pragma unroll
    for (int c = 0; c < WVN_GRID_MAX_CHANNELS; ++c)
      if (c < a.C) a.layers[c][cell] = old[c];
    a.hits[cell] += nhits;
  }
}

// ------------------------------------------------------------------------------------------------------------------------- sdf
constexpr int SDF_THREADS = 256;
constexpr int SDF_FAR = 1 << 29;   // "no such cell": above every real squared distance (2 * 4095^2 < 2^26), and two of them still fit an int

// 1 = obstacle, 0 = free, -1 = neither
__device__ __forceinline__ int sdf_class(float v, float threshold, int unknown) {
  if (v != v) return unknown == WVN_GRID_UNKNOWN_OBSTACLE ? 1 : unknown == WVN_GRID_UNKNOWN_FREE ? 0 : -1;
  return v < threshold ? 1 : 0;
}

__global__ __launch_bounds__(SDF_THREADS) void grid_sdf_kernel(const float* __restrict__ layer, int N, float threshold, int unknown,
                                                               float r, int* __restrict__ d2, float* __restrict__ sdf) {
  extern __shared__ int g[];   // [N] g_O, [N] g_F
  int* gO = g;
  int* gF = g + N;
  const int i = blockIdx.x;
  for (int k = threadIdx.x; k < N; k += SDF_THREADS) {
    int bo = SDF_FAR, bf = SDF_FAR;
    for (int ii = 0; ii < N; ++ii) {
      const int cls = sdf_class(layer[(size_t)ii * N + k], threshold, unknown);
      const int d = (ii - i) * (ii - i);
      if (cls == 1) bo = min(bo, d);
      if (cls == 0) bf = min(bf, d);
    }
    gO[k] = bo;
    gF[k] = bf;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < N; j += SDF_THREADS) {
    const size_t cell = (size_t)i * N + j;
    const int cls = sdf_class(layer[cell], threshold, unknown);
    if (cls < 0) {
      d2[cell] = 0;
      sdf[cell] = __builtin_nanf("");
      continue;
    }
    const int* other = cls == 1 ? gF : gO;
    int best = SDF_FAR;
    for (int k = 0; k < N; ++k) best = min(best, (j - k) * (j - k) + other[k]);
    const bool none = best >= SDF_FAR;
    const int m = none ? INT32_MAX : best;
    const float dist = none ? __builtin_inff() : r * sqrtf((float)best);
    d2[cell] = cls == 1 ? -m : m;
    sdf[cell] = cls == 1 ? -dist : dist;
  }
}

// ---------------------------------------------------------------------------------------------------------------------- carrot
constexpr int CARROT_THREADS = 1024;

struct CarrotArgs {
  const float* sdf;
  const float* elev;
  int* goal_cell;   // [3] i, j, found
  float* goal;      // [3] score, x, y
  float* masked;    // [N][N] or null
  int N, n_discs;
  int ci[WVN_GRID_MAX_DISCS], cj[WVN_GRID_MAX_DISCS], rad[WVN_GRID_MAX_DISCS];
  float cosy, siny, dff, cff, cx, cy, r;
};

__device__ __forceinline__ unsigned long long carrot_key(float s, unsigned idx) {
  unsigned u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // order-preserving on the non-NaN floats (-inf lowest)
  return ((unsigned long long)u << 32) | (0xFFFFFFFFu - idx);
}

__global__ __launch_bounds__(CARROT_THREADS) void grid_carrot_kernel(const CarrotArgs a) {
  __shared__ unsigned long long wave_best[CARROT_THREADS / WVN_WAVE];
  const int N = a.N, c = N / 2;
  const float dmax = sqrtf((float)(2 * c * c));
  const float ninf = -__builtin_inff();
  unsigned long long best = 0;   // below every key
  for (int idx = threadIdx.x; idx < N * N; idx += CARROT_THREADS) {
    const int i = idx / N, j = idx - i * N;
    float s = a.sdf[idx];
    if (a.dff > 0.f) {
      float d = sqrtf((float)((i - c) * (i - c) + (j - c) * (j - c)));
      d = d / dmax;
      d = d * a.dff;
      s = s + d;
    }
    if (a.cff > 0.f) {
      const float cf = fabsf(a.cosy * (float)(j - c) - a.siny * (float)(i - c));
      s = s - cf * a.cff;
    }
    bool keep = false;
    for (int d = 0; d < a.n_discs; ++d) {
      const long long di = i - a.ci[d], dj = j - a.cj[d], rr = a.rad[d];
      keep |= di * di + dj * dj <= rr * rr;
    }
    if (keep) {
      for (int ii = max(i - 1, 0); ii <= min(i + 1, N - 1); ++ii)
        for (int jj = max(j - 1, 0); jj <= min(j + 1, N - 1); ++jj) {
          const float e = a.elev[(size_t)ii * N + jj];
          keep &= e == e;
        }
    }
    if (!keep || s != s) s = ninf;
    if (a.masked) a.masked[idx] = s;
    const unsigned long long key = carrot_key(s, (unsigned)idx);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int off = WVN_WAVE / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(best, off, WVN_WAVE);
    best = o > best ? o : best;
  }
  if ((threadIdx.x & (WVN_WAVE - 1)) == 0) wave_best[threadIdx.x / WVN_WAVE] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < CARROT_THREADS / WVN_WAVE; ++w) best = wave_best[w] > best ? wave_best[w] : best;
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu);
    unsigned u = (unsigned)(best >> 32);
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    const float s = __uint_as_float(u);
    const int i = (int)idx / N, j = (int)idx - i * N;
    const float half = (float)N * 0.5f;
    a.goal_cell[0] = i;
    a.goal_cell[1] = j;
    a.goal_cell[2] = s > ninf ? 1 : 0;
    a.goal[0] = s;
    a.goal[1] = ((float)i - half) * a.r + a.cx;   // smart_carrot.py:145-150
    a.goal[2] = ((float)j - half) * a.r + a.cy;
  }
}

}  // namespace

extern "C" {

int wvn_grid_fuse_images(const float* maps, int B, int C, int H, int W, const float* intrinsics, const float* poses,
                         const float* elevation, int N, float cx, float cy, float resolution, float* const* layers, int* hits,
                         float alpha, float min_depth, float max_range, float occlusion_margin, void* stream) {
  if (!maps || !intrinsics || !poses || !elevation || !layers || !hits) return WVN_ERR_ARG;
  if (B < 1 || B > WVN_GRID_MAX_CAMERAS || C < 1 || C > WVN_GRID_MAX_CHANNELS || H < 1 || W < 1 || N < 1 || N > WVN_GRID_MAX_N) return WVN_ERR_ARG;
  if ((long long)B * C * H * W > INT32_MAX) return WVN_ERR_ARG;
  if (!(resolution > 0.f) || !(fabsf(resolution) <= 3.402823466e+38f) || !(alpha >= 0.f && alpha <= 1.f) || max_range != max_range || min_depth != min_depth ||
      occlusion_margin != occlusion_margin || !(fabsf(cx) <= 3.402823466e+38f) || !(fabsf(cy) <= 3.402823466e+38f))
    return WVN_ERR_ARG;
  FuseArgs a;
  for (int c = 0; c < WVN_GRID_MAX_CHANNELS; ++c) {
    a.layers[c] = c < C ? layers[c] : nullptr;
    if (c < C && !a.layers[c]) return WVN_ERR_ARG;
  }
  a.maps = maps, a.K = intrinsics, a.pose = poses, a.elev = elevation, a.hits = hits;
  a.B = B, a.C = C, a.H = H, a.W = W, a.N = N;
  a.cx = cx, a.cy = cy, a.r = resolution, a.alpha = alpha, a.min_depth = min_depth, a.max_range = max_range, a.margin = occlusion_margin;
  const unsigned tiles = (unsigned)((N + TILE - 1) / TILE);
  hipLaunchKernelGGL(grid_fuse_kernel, dim3(tiles, tiles), dim3(TILE * TILE), 0, (hipStream_t)stream, a);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_grid_sdf(const float* layer, int N, float threshold, int unknown, float resolution, int* d2, float* sdf, void* stream) {
  if (!layer || !d2 || !sdf || N < 1 || N > WVN_GRID_MAX_N) return WVN_ERR_ARG;
  if (unknown != WVN_GRID_UNKNOWN_OBSTACLE && unknown != WVN_GRID_UNKNOWN_FREE && unknown != WVN_GRID_UNKNOWN_NEITHER) return WVN_ERR_ARG;
  if (!(resolution > 0.f) || !(fabsf(resolution) <= 3.402823466e+38f)) return WVN_ERR_ARG;
  hipLaunchKernelGGL(grid_sdf_kernel, dim3((unsigned)N), dim3(SDF_THREADS), (size_t)N * 2 * sizeof(int), (hipStream_t)stream, layer, N,
                     threshold, unknown, resolution, d2, sdf);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_grid_carrot(const float* sdf, const float* elevation, int N, double cos_yaw, double sin_yaw, float distance_force_factor,
                    float center_force_factor, const int* discs, int n_discs, float cx, float cy, float resolution, int* goal_cell,
                    float* goal, float* masked, void* stream) {
  if (!sdf || !elevation || !discs || !goal_cell || !goal || N < 1 || N > WVN_GRID_MAX_N) return WVN_ERR_ARG;
  if (n_discs < 1 || n_discs > WVN_GRID_MAX_DISCS) return WVN_ERR_ARG;
  if (!(fabs(cos_yaw) <= 1.0 + 1e-9) || !(fabs(sin_yaw) <= 1.0 + 1e-9)) return WVN_ERR_ARG;
  if (distance_force_factor != distance_force_factor || center_force_factor != center_force_factor || !(resolution > 0.f) ||
      !(fabsf(resolution) <= 3.402823466e+38f) || !(fabsf(cx) <= 3.402823466e+38f) || !(fabsf(cy) <= 3.402823466e+38f))
    return WVN_ERR_ARG;
  CarrotArgs a;
  for (int d = 0; d < n_discs; ++d) {
    const int distance = discs[2 * d], radius = discs[2 * d + 1];
    if (distance < 0 || distance > WVN_GRID_MAX_DISC_DISTANCE || radius < 0 || radius > WVN_GRID_MAX_DISC_DISTANCE) return WVN_ERR_ARG;
    a.ci[d] = (int)((double)N / 2 + cos_yaw * distance);   // the row: cv2.circle's centre is (column, row) = (center_x, center_y)
    a.cj[d] = (int)((double)N / 2 + sin_yaw * distance);
    a.rad[d] = radius;
  }
  a.sdf = sdf, a.elev = elevation, a.goal_cell = goal_cell, a.goal = goal, a.masked = masked;
  a.N = N, a.n_discs = n_discs;
  a.cosy = (float)cos_yaw, a.siny = (float)sin_yaw, a.dff = distance_force_factor, a.cff = center_force_factor;
  a.cx = cx, a.cy = cy, a.r = resolution;
  hipLaunchKernelGGL(grid_carrot_kernel, dim3(1), dim3(CARROT_THREADS), 0, (hipStream_t)stream, a);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // extern "C"
