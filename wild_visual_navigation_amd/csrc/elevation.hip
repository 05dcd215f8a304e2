// Elevation from depth (include/wvn_hip.h: "Traversability grid map", wvn_grid_elevation_*): the elevation and variance layers of the
// grid map built from the depth images and point clouds of one callback -- the geometric half that csrc/grid_map.hip's fusion, SDF and
// carrot start from.  Two launches for all sensors, no host synchronisation, INTEGER atomics only: tests/elevation_ref.py states both
// kernels in numpy and the results are that statement BIT FOR BIT, whatever the order of the points, the sensors or the waves (this file
// is compiled with -ffp-contract=off: every fp32 and fp64 operation below is rounded on its own).
//
// Grid as csrc/grid_map.hip.  Every point is judged against the map AS IT WAS ON ENTRY (the accumulate kernel only reads the layers).
//
// ---- elev_accumulate_kernel<SRC>: one thread per point slot (SRC_POINTS: b * Pmax + p) or pixel (b * H * W + v * W + u) ----
// The poses, the four intrinsics and the counts of all B <= 64 sensors are staged in LDS by the workgroup (6 KB at the most).
//   depth form: z = depth (u16: float(mm) / 1000.0f);  p = ((float(u) - K[0][2]) * (z / K[0][0]), (float(v) - K[1][2]) * (z / K[1][1]), z)
//     formed on load -- no cloud is written; z == 0, NaN or inf: class "invalid".
//   rejection, first match:  invalid (a coordinate not finite);  near: d2 = (x x + y y) + z z < min_valid_distance^2;
//     q[k] = ((T[k][0] x + T[k][1] y) + T[k][2] z) + t[k];  high: q_z - t_z > max_height_range;
//     ramp: q_z - t_z > fmaxf(L - ramp_b, 0) * ramp_a + ramp_c with L = sqrtf(dx dx + dy dy), (dx, dy, dz) = t - q;
//     outside: the nearest cell (floorf((q_x - cx) * (1 / r) + (N * 0.5f + 0.5f)), likewise y) is not in the map.
//   gate:  h finite and fabsf(q_z - h) > mahalanobis_thresh * sqrtf(var)  ->  n_out += 1, nothing else.
//   inlier:  v = sensor_noise_factor * d2, w = 1.0f / v, wq = (int64)floorf(fminf(w, 4096 - 1/256) * 256), zq = (int64)rintf((q_z - z_ref)
//     * 16384);  not (fabsf(q_z - z_ref) <= 128) or wq == 0: class "unrepresentable", dropped;  else S_w += wq, S_wz += wq * zq, n += 1.
//   FORMAT BOUND: wq <= 2^20 - 1 and |zq| <= 2^21, so |wq zq| < 2^41 and with at most WVN_GRID_ELEVATION_MAX_POINTS = 2^22 point slots per
//     call |S_wz| < 2^63, S_w < 2^42: the int64 sums cannot overflow.  The entry points refuse more slots before any launch.
//   ray clearing (flag): every point that passed rejection walks towards its sensor, step = r / L, s = 1 .. min(floorf(L / r),
//     floorf(max_ray_length / r)): t = float(s) * step, c = q + t (dx, dy, dz); outside the map: the walk ends; a visited cell other than
//     the point's own whose entry elevation is finite and he - c_z > clear_margin gets contradicted += 1.
// Workspace (int, zero on first use, left zero by the finalise kernel): 8 int32 class counters, then per cell 32 bytes
//     { int64 S_w, int64 S_wz, uint64 (n | n_out << 32), int32 contradicted, int32 pad }     -- one 32-byte sector per cell.
// Wave-level combining: a depth image lands thousands of neighbouring pixels in a few cells, and the lanes of a wave are neighbours along
// an image row (or along the scan of a LiDAR), so equal cells arrive as RUNS of consecutive lanes.  The run form was chosen over a
// wave-level match (readfirstlane + ballot per distinct cell): it costs a fixed six shuffle steps whatever the number of distinct cells
// in the wave, where the match loop costs one masked reduction per distinct cell and a scattered cloud has up to 64 of them.  The head
// lane of each run issues the run's sums: two 64-bit adds and one for the counts.  Within a wave the partial sums are integers
// (S_w <= 64 (2^20 - 1) fits 32 bits), so combining cannot change a bit.  A build with -DWVN_ELEV_NO_COMBINE=1 is the same kernel with one
// run per lane: the measurement's other side (profiles/elevation.md), loaded through WVN_LIB_PATH; it is not part of the library.
//
// ---- elev_finalise_kernel: one thread per cell, fp64 ----
//   n > 0:  v_m = 256.0 / double(S_w);  z_m = double(z_ref) + (double(S_wz) / double(S_w)) / 16384.0;
//           h not finite: h' = z_m, var' = v_m;  else h' = (h v_m + z_m var) / (var + v_m), var' = (var v_m) / (var + v_m)
//   n == 0, n_out > 0:  h keeps its bits, var' = var
//   both:  var' = fmin(var' + double(outlier_variance) * double(n_out), double(max_variance));  h', var' rounded to fp32 once
//   n == 0 and clearing and contradicted >= clear_min_rays:  elevation NaN, variance = initial_variance, image layers NaN, hits 0.
// The kernel zeroes the cell's workspace, copies the class counters to `stats` and zeroes them: no memset launch between callbacks.
#include <stdint.h>
#include <math.h>

#include "common.h"
#include "wvn_internal.h"
#include "../../include/wvn_hip.h"

namespace {

constexpr int ACC_THREADS = 256;
// a workgroup takes ACC_CHUNKS consecutive groups of 256 point slots: the sensors' constants are staged once and the class counters reach
// the eight global words once per 1024 slots -- adds to ONE word serialise, and at one add per class and 256 slots they set the kernel's time
constexpr int ACC_CHUNKS = 4;
constexpr int SRC_POINTS = 0, SRC_DEPTH_F32 = 1, SRC_DEPTH_U16 = 2;
constexpr int N_STATS = WVN_GRID_ELEVATION_STATS;
enum { CLS_INVALID = 0, CLS_NEAR, CLS_HIGH, CLS_RAMP, CLS_OUTSIDE, CLS_GATED, CLS_UNREPRESENTABLE, CLS_INLIER, CLS_NONE };
constexpr float FLT_BIG = 3.402823466e+38f;

struct ElevCell {
  long long S_w, S_wz;
  unsigned long long counts;   // n | n_out << 32
  int contradicted, pad;
};
static_assert(sizeof(ElevCell) == 32, "one 32-byte sector per cell");

struct AccArgs {
  const void* src;       // [B][Pmax][3] fp32, or [B][H][W] fp32 / u16
  const int* counts;     // [B] or null (points form)
  const float* K;        // [B][4][4] (depth forms)
  const float* pose;     // [B][4][4]
  const float* elev;     // [N][N]
  const float* var;      // [N][N]
  int* stats;            // workspace head: [N_STATS]
  ElevCell* cells;       // [N][N]
  const float* z_ref;    // one fp32 on the device
  int B, per, W, N, clear;   // per = Pmax or H * W
  float cx, cy, r, noise, maha, min_d2, max_height, ramp_a, ramp_b, ramp_c, max_steps, margin;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_BIG; }

#if defined(WVN_ELEV_NO_COMBINE) && WVN_ELEV_NO_COMBINE
constexpr bool COMBINE = false;
#else
constexpr bool COMBINE = true;
#endif

template <int SRC>
__global__ __launch_bounds__(ACC_THREADS) void elev_accumulate_kernel(const AccArgs a) {
  __shared__ float s_pose[WVN_GRID_MAX_CAMERAS][12];
  __shared__ float s_K[WVN_GRID_MAX_CAMERAS][4];
  __shared__ int s_count[WVN_GRID_MAX_CAMERAS];
  __shared__ int s_stats[N_STATS];
  const int tid = threadIdx.x, lane = tid & (WVN_WAVE - 1);
  for (int e = tid; e < a.B * 12; e += ACC_THREADS) s_pose[e / 12][e % 12] = a.pose[(size_t)(e / 12) * 16 + (e % 12)];
  if (SRC != SRC_POINTS)
    for (int e = tid; e < a.B * 4; e += ACC_THREADS) {
      const int b = e >> 2, k = e & 3;   // fx, fy, cx, cy
      s_K[b][k] = a.K[(size_t)b * 16 + (k == 0 ? 0 : k == 1 ? 5 : k == 2 ? 2 : 6)];
    }
  for (int e = tid; e < a.B; e += ACC_THREADS) s_count[e] = a.counts ? a.counts[e] : a.per;
  if (tid < N_STATS) s_stats[tid] = 0;
  __syncthreads();

  const int N = a.N;
  const long long total = (long long)a.B * a.per;
#pragma unroll 1
  for (int chunk = 0; chunk < ACC_CHUNKS; ++chunk) {   // (no lane leaves early: every lane of a wave takes part in the shuffles)
    const long long idx = ((long long)blockIdx.x * ACC_CHUNKS + chunk) * ACC_THREADS + tid;
    int cls = CLS_NONE, cell = -1;
    float qx = 0.f, qy = 0.f, qz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, L = 0.f;
    unsigned wq = 0;
    long long wz = 0;
    if (idx < total) {
      const int b = (int)(idx / a.per), k = (int)(idx - (long long)b * a.per);
      float x, y, z;
      bool live = true, have = true;
      if (SRC == SRC_POINTS) {
        live = k < s_count[b];
        const float* p = (const float*)a.src + (size_t)idx * 3;
        x = live ? p[0] : 0.f, y = live ? p[1] : 0.f, z = live ? p[2] : 0.f;
      } else {
        const int v = k / a.W, u = k - v * a.W;
        z = SRC == SRC_DEPTH_U16 ? (float)((const uint16_t*)a.src)[idx] / 1000.0f : ((const float*)a.src)[idx];
        have = z != 0.f;
        x = ((float)u - s_K[b][2]) * (z / s_K[b][0]);
        y = ((float)v - s_K[b][3]) * (z / s_K[b][1]);
      }
      if (live) {
        const float* T = s_pose[b];
        const float d2 = (x * x + y * y) + z * z;
        qx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
        qy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
        qz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
        dx = T[3] - qx, dy = T[7] - qy, dz = T[11] - qz;
        L = sqrtf(dx * dx + dy * dy);
        const float up = qz - T[11];
        const float half_p = (float)N * 0.5f + 0.5f, inv_r = 1.0f / a.r;
        const float fi = floorf((qx - a.cx) * inv_r + half_p), fj = floorf((qy - a.cy) * inv_r + half_p);
        if (!(have && finite_f(x) && finite_f(y) && finite_f(z))) cls = CLS_INVALID;
        else if (d2 < a.min_d2) cls = CLS_NEAR;
        else if (up > a.max_height) cls = CLS_HIGH;
        else if (up > fmaxf(L - a.ramp_b, 0.f) * a.ramp_a + a.ramp_c) cls = CLS_RAMP;
        else if (!(fi >= 0.f && fi < (float)N && fj >= 0.f && fj < (float)N)) cls = CLS_OUTSIDE;
        else {
          cell = (int)fi * N + (int)fj;
          const float h = a.elev[cell], hv = a.var[cell];
          const float rel = qz - *a.z_ref;
          const float v = a.noise * d2;
          const float w = 1.0f / v;
          const float wqf = floorf(fminf(w, 4095.99609375f) * 256.0f);
          if (finite_f(h) && fabsf(qz - h) > a.maha * sqrtf(hv)) cls = CLS_GATED;
          else if (!(fabsf(rel) <= 128.0f) || !(wqf > 0.f)) cls = CLS_UNREPRESENTABLE;
          else {
            cls = CLS_INLIER;
            wq = (unsigned)wqf;
            wz = (long long)wq * (long long)rintf(rel * 16384.0f);
          }
        }
      }
    }

    // class counters: one ballot per class and wave -> LDS -> one global integer add per class and workgroup
  #pragma unroll
    for (int c = 0; c < N_STATS; ++c) {
      const unsigned long long m = __ballot(cls == c);
      if (lane == 0 && m) atomicAdd(&s_stats[c], __popcll(m));
    }

    // the sums: runs of equal cells along the wave, the head lane of a run adds the run
    const bool contributes = cls == CLS_INLIER || cls == CLS_GATED;
    const int key = contributes ? cell : -1;
    unsigned sw = wq;                                                        // <= 64 (2^20 - 1): 32 bits
    unsigned cnt = cls == CLS_INLIER ? 1u : cls == CLS_GATED ? 0x10000u : 0u;   // n | n_out << 16 within the wave (each <= 64)
    long long swz = wz;
    bool head = true;
    if (COMBINE) {
      const int prev = __shfl_up(key, 1, WVN_WAVE);
      const unsigned long long heads = __ballot(lane == 0 || prev != key);
      const int my_head = 63 - __clzll(heads & (~0ull >> (63 - lane)));      // the highest head at or below this lane
      head = my_head == lane;
  #pragma unroll
      for (int off = 1; off < WVN_WAVE; off <<= 1) {
        const int oh = __shfl_down(my_head, off, WVN_WAVE);
        const unsigned osw = __shfl_down(sw, off, WVN_WAVE), ocnt = __shfl_down(cnt, off, WVN_WAVE);
        const long long oswz = __shfl_down(swz, off, WVN_WAVE);
        // heads are monotone along the wave: lane + off is in this lane's run exactly when its head is this lane's head.  A lane's
        // partial sum after the step covers [lane, lane + 2 off) clipped to its run, as in any segmented suffix sum
        if (lane + off < WVN_WAVE && oh == my_head) sw += osw, cnt += ocnt, swz += oswz;
      }
    }
    if (head && key >= 0) {
      ElevCell* c = a.cells + key;
      const unsigned n = cnt & 0xFFFFu, n_out = cnt >> 16;
      if (n) {
        atomicAdd((unsigned long long*)&c->S_w, (unsigned long long)sw);
        atomicAdd((unsigned long long*)&c->S_wz, (unsigned long long)swz);   // two's complement: the unsigned add is the signed add
      }
      atomicAdd(&c->counts, (unsigned long long)n | ((unsigned long long)n_out << 32));
    }

    if (a.clear && cls >= CLS_GATED && cls <= CLS_INLIER) {
      const float half_p = (float)N * 0.5f + 0.5f, inv_r = 1.0f / a.r;
      const float step = a.r / L;
      const int nsteps = (int)fminf(floorf(L / a.r), a.max_steps);   // (L == 0: step is inf and L / r is 0 -- no step is taken)
      for (int s = 1; s <= nsteps; ++s) {
        const float t = (float)s * step;
        const float px = qx + t * dx, py = qy + t * dy, pz = qz + t * dz;
        const float fi = floorf((px - a.cx) * inv_r + half_p), fj = floorf((py - a.cy) * inv_r + half_p);
        if (!(fi >= 0.f && fi < (float)N && fj >= 0.f && fj < (float)N)) break;
        const int at = (int)fi * N + (int)fj;
        const float he = a.elev[at];
        if (at != cell && finite_f(he) && he - pz > a.margin) atomicAdd(&a.cells[at].contradicted, 1);
      }
    }
  }

  __syncthreads();
  if (tid < N_STATS && s_stats[tid]) atomicAdd(a.stats + tid, s_stats[tid]);
}

struct FinArgs {
  float* elev;
  float* var;
  float* layers[WVN_GRID_MAX_CHANNELS];
  int* hits;
  int* ws_stats;
  ElevCell* cells;
  int* stats;   // [N_STATS] out
  const float* z_ref;
  int N, C, clear, min_rays;
  float outlier_var, max_var, initial_var;
};

__global__ __launch_bounds__(256) void elev_finalise_kernel(const FinArgs a) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < N_STATS) {
    a.stats[threadIdx.x] = a.ws_stats[threadIdx.x];
    a.ws_stats[threadIdx.x] = 0;
  }
  if (idx >= a.N * a.N) return;
  ElevCell* cp = a.cells + idx;
  const ElevCell c = *cp;
  const unsigned n = (unsigned)(c.counts & 0xFFFFFFFFull), n_out = (unsigned)(c.counts >> 32);
  if (!n && !n_out && !c.contradicted) return;   // the workspace of this cell is zero already
  ElevCell zero;
  zero.S_w = 0, zero.S_wz = 0, zero.counts = 0, zero.contradicted = 0, zero.pad = 0;
  *cp = zero;
  if (a.clear && !n && c.contradicted >= a.min_rays) {   // (wins over the outlier rule)
    const float nan = __builtin_nanf("");
    a.elev[idx] = nan;
    a.var[idx] = a.initial_var;
#pragma unroll
    for (int k = 0; k < WVN_GRID_MAX_CHANNELS; ++k)
      if (k < a.C) a.layers[k][idx] = nan;
    a.hits[idx] = 0;
  } else if (n || n_out) {
    const float h = a.elev[idx];
    const double var = (double)a.var[idx];
    double var_new = var;
    if (n) {
      const double Sw = (double)c.S_w;
      const double v_m = 256.0 / Sw;
      const double ratio = (double)c.S_wz / Sw;
      const double z_m = (double)*a.z_ref + ratio / 16384.0;
      double h_new;
      if (finite_f(h)) {
        const double den = var + v_m;
        h_new = ((double)h * v_m + z_m * var) / den;
        var_new = (var * v_m) / den;
      } else {
        h_new = z_m;
        var_new = v_m;
      }
      a.elev[idx] = (float)h_new;
    }
    var_new = fmin(var_new + (double)a.outlier_var * (double)n_out, (double)a.max_var);
    a.var[idx] = (float)var_new;
  }
}

bool finite_h(float v) { return fabsf(v) <= FLT_BIG; }

// the checks the three entry points share; the accumulate arguments that depend on them
int elev_common(AccArgs& a, const float* poses, const float* elevation, const float* variance, int N, float cx, float cy, float r,
                void* workspace, int B, long long per, const wvn_grid_elevation_params* p, const float* z_ref, int flags) {
  if (!poses || !elevation || !variance || !workspace || !p || !z_ref) return WVN_ERR_ARG;
  if ((uintptr_t)workspace & 7) return WVN_ERR_ARG;   // the records take 64-bit atomics
  if (N < 1 || N > WVN_GRID_MAX_N || B < 1 || B > WVN_GRID_MAX_CAMERAS || per < 1) return WVN_ERR_ARG;
  if ((long long)B * per > WVN_GRID_ELEVATION_MAX_POINTS) return WVN_ERR_ARG;
  if (flags & ~WVN_GRID_ELEVATION_CLEAR_RAYS) return WVN_ERR_ARG;
  if (!(r > 0.f) || !finite_h(r) || !finite_h(cx) || !finite_h(cy)) return WVN_ERR_ARG;
  if (!(p->sensor_noise_factor > 0.f) || !finite_h(p->sensor_noise_factor)) return WVN_ERR_ARG;
  if (!(p->min_valid_distance >= 0.f) || !finite_h(p->min_valid_distance) || !(p->mahalanobis_thresh >= 0.f)) return WVN_ERR_ARG;
  if (p->max_height_range != p->max_height_range || p->ramp_a != p->ramp_a || p->ramp_b != p->ramp_b || p->ramp_c != p->ramp_c ||
      p->clear_margin != p->clear_margin)
    return WVN_ERR_ARG;
  if (!(p->max_ray_length >= 0.f) || !finite_h(p->max_ray_length) || !(p->max_ray_length / r <= 1048576.f)) return WVN_ERR_ARG;
  a.pose = poses, a.elev = elevation, a.var = variance;
  a.stats = (int*)workspace;
  a.cells = (ElevCell*)((char*)workspace + N_STATS * sizeof(int));
  a.B = B, a.per = (int)per, a.N = N, a.clear = (flags & WVN_GRID_ELEVATION_CLEAR_RAYS) ? 1 : 0;
  a.cx = cx, a.cy = cy, a.r = r, a.z_ref = z_ref, a.noise = p->sensor_noise_factor, a.maha = p->mahalanobis_thresh;
  a.min_d2 = p->min_valid_distance * p->min_valid_distance, a.max_height = p->max_height_range;
  a.ramp_a = p->ramp_a, a.ramp_b = p->ramp_b, a.ramp_c = p->ramp_c;
  a.max_steps = floorf(p->max_ray_length / r), a.margin = p->clear_margin;
  return WVN_OK;
}

template <int SRC>
void elev_launch(const AccArgs& a, hipStream_t st) {
  const long long per_block = (long long)ACC_THREADS * ACC_CHUNKS;
  const unsigned blocks = (unsigned)(((long long)a.B * a.per + per_block - 1) / per_block);
  hipLaunchKernelGGL(elev_accumulate_kernel<SRC>, dim3(blocks), dim3(ACC_THREADS), 0, st, a);
}

}  // namespace

extern "C" {

size_t wvn_grid_elevation_workspace_bytes(int N) {
  if (N < 1 || N > WVN_GRID_MAX_N) return 0;
  return N_STATS * sizeof(int) + (size_t)N * N * sizeof(ElevCell);
}

int wvn_grid_elevation_accumulate_points(const float* points, const int* counts, int B, int Pmax, const float* poses,
                                         const float* elevation, const float* variance, int N, float cx, float cy, float resolution,
                                         const wvn_grid_elevation_params* params, const float* z_ref, int flags, void* workspace, void* stream) {
  AccArgs a;
  if (!points || Pmax < 1) return WVN_ERR_ARG;
  const int rc = elev_common(a, poses, elevation, variance, N, cx, cy, resolution, workspace, B, Pmax, params, z_ref, flags);
  if (rc != WVN_OK) return rc;
  a.src = points, a.counts = counts, a.K = nullptr, a.W = 1;
  elev_launch<SRC_POINTS>(a, (hipStream_t)stream);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_grid_elevation_accumulate_depth(const void* depth, int dtype, int B, int H, int W, const float* intrinsics, const float* poses,
                                        const float* elevation, const float* variance, int N, float cx, float cy, float resolution,
                                        const wvn_grid_elevation_params* params, const float* z_ref, int flags, void* workspace, void* stream) {
  AccArgs a;
  if (!depth || !intrinsics || H < 1 || W < 1 || H > WVN_GRID_ELEVATION_MAX_POINTS || W > WVN_GRID_ELEVATION_MAX_POINTS) return WVN_ERR_ARG;
  if (dtype != WVN_GRID_DEPTH_F32 && dtype != WVN_GRID_DEPTH_U16) return WVN_ERR_ARG;
  const int rc = elev_common(a, poses, elevation, variance, N, cx, cy, resolution, workspace, B, (long long)H * W, params, z_ref, flags);
  if (rc != WVN_OK) return rc;
  a.src = depth, a.counts = nullptr, a.K = intrinsics, a.W = W;
  if (dtype == WVN_GRID_DEPTH_U16)
    elev_launch<SRC_DEPTH_U16>(a, (hipStream_t)stream);
  else
    elev_launch<SRC_DEPTH_F32>(a, (hipStream_t)stream);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_grid_elevation_finalise(float* elevation, float* variance, float* const* layers, int C, int* hits, int N,
                                const wvn_grid_elevation_params* params, const float* z_ref, int flags, void* workspace, int* stats, void* stream) {
  if (!elevation || !variance || !hits || !params || !workspace || !stats || !z_ref || N < 1 || N > WVN_GRID_MAX_N) return WVN_ERR_ARG;
  if (C < 0 || C > WVN_GRID_MAX_CHANNELS || (C > 0 && !layers) || ((uintptr_t)workspace & 7)) return WVN_ERR_ARG;
  if (flags & ~WVN_GRID_ELEVATION_CLEAR_RAYS) return WVN_ERR_ARG;
  if (!(params->outlier_variance >= 0.f) || !(params->max_variance > 0.f) || params->initial_variance != params->initial_variance ||
      params->clear_min_rays < 1)
    return WVN_ERR_ARG;
  FinArgs a;
  for (int c = 0; c < WVN_GRID_MAX_CHANNELS; ++c) {
    a.layers[c] = c < C ? layers[c] : nullptr;
    if (c < C && !a.layers[c]) return WVN_ERR_ARG;
  }
  a.elev = elevation, a.var = variance, a.hits = hits, a.stats = stats;
  a.ws_stats = (int*)workspace;
  a.cells = (ElevCell*)((char*)workspace + N_STATS * sizeof(int));
  a.N = N, a.C = C, a.clear = (flags & WVN_GRID_ELEVATION_CLEAR_RAYS) ? 1 : 0, a.min_rays = params->clear_min_rays;
  a.z_ref = z_ref, a.outlier_var = params->outlier_variance, a.max_var = params->max_variance, a.initial_var = params->initial_variance;
  hipLaunchKernelGGL(elev_finalise_kernel, dim3((unsigned)(((long long)N * N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // extern "C"
