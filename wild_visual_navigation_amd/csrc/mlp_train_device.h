// Device code the two four-launch training steps share (mlp_train.hip: SimpleMLP, row tiles of 32; double_mlp.hip: DoubleMLP,
// row tiles of 16): the row count, the fixed-order tile sums, the statistic a forward launch publishes and its last tile folds --
// the one piece of inter-workgroup synchronisation in the training path --, the gradient-seed block of a backward tile and the
// loss-sum partial of a backward launch.  The pieces of a tile forward (x-tile load and pitch, the SimpleMLP layers, which the
// per-segment table kernel runs too) are in mlp_tile_device.h; DoubleMLP's pair layers are its own.
#pragma once
#include "mlp_tile_device.h"
#include "wvn_internal.h"

__device__ inline int real_rows(const TrainArgs& p) { return p.rows_dev ? min(p.R, *p.rows_dev) : p.R; }
__device__ inline LossStep loss_step(const TrainArgs& p, int D) {
  return LossStep{p.stats, p.cstate, p.minmax, p.method, p.balanced, p.std_factor, p.w_trav, p.w_reco, D};
}

// fixed-order sum over lanes 0 .. N - 1 of a wave: butterfly, every one of them gets the total
template <int N> __device__ inline double tile_sum_d(double v) {
#pragma unroll
  for (int o = N / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// End of a forward launch, called by the first wave (tid < 64) of every tile behind a barrier; lr_s: the TR row losses of the tile
// in LDS (0 for absent rows).  The tile's partial of the confidence statistic {n_lab, sum, sum^2} (fp64, rows in ascending order
// through a butterfly) and {min, max} of lr go to part / part_mm; the last tile to arrive folds all partials in ascending tile
// order into stats = {n_lab, sum, sum^2, Rr} and minmax = {max, -min}, and leaves the ticket at zero for the next step.
template <int TR> __device__ inline void stat_publish_fold(const TrainArgs& p, const float* lr_s, int row0, int Rr) {
  const int tid = threadIdx.x;
  const bool real = tid < TR && row0 + tid < Rr;
  const bool v = real && p.valid[row0 + tid] != 0;
  const double l = v ? (double)lr_s[tid] : 0.0;
  const double n = tile_sum_d<TR>(v ? 1.0 : 0.0), s1 = tile_sum_d<TR>(l), s2 = tile_sum_d<TR>(l * l);
  float mn = INFINITY, mx = -INFINITY;
  if (p.minmax) {   // min / max of lr over the tile's real rows (moving_average; min and max are order-free)
    if (real) mn = mx = lr_s[tid];
#pragma unroll
    for (int o = TR / 2; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
  }
  if (tid != 0) return;
  double* d = p.part + (size_t)blockIdx.x * 4;
  d[0] = n; d[1] = s1; d[2] = s2;
  if (p.minmax) { p.part_mm[(size_t)blockIdx.x * 2] = mn; p.part_mm[(size_t)blockIdx.x * 2 + 1] = mx; }
  // publish: the partial must be visible device-wide before the ticket (MI355X_MICROARCH.md, producer form)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned t = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t != gridDim.x - 1) return;
  // the last tile to arrive folds the partials in ascending tile order
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double a = 0, b = 0, c = 0;
  for (unsigned i = 0; i < gridDim.x; ++i) {
    const double* e = p.part + (size_t)i * 4;
    a += __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b += __hip_atomic_load(e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c += __hip_atomic_load(e + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  p.stats[0] = a; p.stats[1] = b; p.stats[2] = c; p.stats[3] = (double)Rr;
  if (p.minmax) {
    float lo = INFINITY, hi = -INFINITY;
    for (unsigned i = 0; i < gridDim.x; ++i) {
      lo = fminf(lo, __hip_atomic_load(p.part_mm + (size_t)i * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      hi = fmaxf(hi, __hip_atomic_load(p.part_mm + (size_t)i * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    p.minmax[0] = hi; p.minmax[1] = -lo;
  }
  __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next step
}

// Start of a backward launch: the gradient seed of the tile (mlp_device.h: grad_seed), LPR lanes per row, 256 / LPR rows.  Fills
// gos [TR][1 + D] and tw ([TR] trav_w, [TR] trav_raw) in LDS, g_out and, if asked for, conf_out for the rows below p.R.
template <int LPR> __device__ __forceinline__ void seed_tile(const TrainArgs& p, int D, int row0, int Rr, float* gos, float* tw) {
  constexpr int TR = 256 / LPR;
  const int O = D + 1, tid = threadIdx.x;
  const int r = tid / LPR, q = tid % LPR, row = row0 + r;
  const bool real = row < Rr;
  const Seed sd = real ? grad_seed(loss_step(p, D), p.lr[row], p.out[(size_t)row * O], p.y[row], p.valid[row] != 0) : Seed{};
  if (q == 0) {
    tw[r] = sd.raw * sd.wrow;
    tw[TR + r] = sd.raw;
    if (p.conf_out && row < p.R) p.conf_out[row] = sd.conf;
    gos[r * O] = sd.g0;
    if (row < p.R) p.g_out[(size_t)row * O] = sd.g0;
  }
  for (int d = q; d < D; d += LPR) {
    const float g = real ? seed_elem(sd, p.out[(size_t)row * O + 1 + d], p.x[(size_t)row * p.ld_row + d]) : 0.f;
    gos[r * O + 1 + d] = g;
    if (row < p.R) p.g_out[(size_t)row * O + 1 + d] = g;
  }
}

// Backward launch, first wave (tid < 64) behind a barrier; tw: [TR] trav_w, [TR] trav_raw of the tile in LDS.  The tile's partial
// of the two loss sums (fp64, rows in ascending order through a butterfly) goes to part; the wgrad launch folds the partials.
template <int TR> __device__ inline void loss_sums_partial(const TrainArgs& p, const float* tw) {
  const int tid = threadIdx.x;
  const double a = tile_sum_d<TR>(tid < TR ? (double)tw[tid] : 0.0), b = tile_sum_d<TR>(tid < TR ? (double)tw[TR + tid] : 0.0);
  if (tid == 0) { p.part[(size_t)blockIdx.x * 4] = a; p.part[(size_t)blockIdx.x * 4 + 1] = b; }
}
