// Device helpers shared by the traversability-MLP training kernels (mlp.hip: one kernel per stage; mlp_train.hip and
// double_mlp.hip: the four-launch steps): the confidence statistic and the confidence of a reconstruction loss, for the four
// ConfidenceGenerator methods, and the gradient seed of TraversabilityLoss that is built on them.
// Reference: wild_visual_navigation/utils/confidence_generator.py, kalman_filter.py, loss.py.
#pragma once
#include "common.h"
#include "../../include/wvn_hip.h"

struct ConfStats { float mean, std; };
__device__ inline ConfStats conf_stats(const double* st) {
  const double n = st[0];
  const double mean = st[1] / n;
  const double var = (st[2] - st[1] * st[1] / n) / (n - 1.0);  // unbiased (torch.std); NaN for n < 2
  ConfStats c;
  c.mean = (float)mean;
  c.std = (float)sqrt(var > 0.0 || !(var == var) ? var : 0.0);
  return c;
}
// confidence_generator.py:182-193
__device__ inline float confidence_of(float x, float mean, float std, float f) {
  const float shifted = mean + std * f;
  float lo = shifted - std;
  lo = (lo > 0.f || isnan(lo)) ? lo : 0.f;  // python max(lo, 0): NaN stays NaN
  const float hi = shifted + std;
  float xc = fminf(fmaxf(x, lo), hi);
  if (isnan(lo) || isnan(hi)) xc = NAN;
  return 1.f - (xc - lo) / (hi - lo);
}
// the same for a loss that may be NaN (a NaN feature row): torch.clip keeps the NaN, fminf / fmaxf would drop it
__device__ inline float confidence_of_nan(float x, float mean, float std, float f) {
  return isnan(x) ? NAN : confidence_of(x, mean, std, f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The other ConfidenceGenerator methods (confidence_generator.py:87-151).  Their statistic has a memory: the persistent device
// state cs[WVN_CONF_STATE_DOUBLES] (layout in include/wvn_hip.h) plus this step's global stats {n_lab, sum, sum^2, R}.  Phase B
// evaluates the post-update statistic from (cs, stats) in every workgroup; phase C evaluates it once more and commits it.
// ---------------------------------------------------------------------------------------------------------------------------
struct ConfPost { float mean, var, std; };

// the ring head / fill count read from the state, clamped to [0, hi] (NaN -> 0): a corrupted state cannot address past the ring
__device__ inline int state_int(double v, int hi) { return v >= 1.0 ? (v < hi ? (int)v : hi) : 0; }

__device__ inline ConfPost conf_post(int method, const double* st, const double* cs) {
  ConfPost c;
  c.var = (float)cs[WVN_CONF_S_VAR];
  if (method == WVN_CONF_RUNNING_MEAN) {          // update_running_mean: fp64 running sums, fp32 mean, population variance
    const double n = cs[WVN_CONF_S_RUN_N] + st[0], s = cs[WVN_CONF_S_RUN_SUM] + st[1], s2 = cs[WVN_CONF_S_RUN_SUMSQ] + st[2];
    c.mean = (float)(s / n);
    const float m2 = c.mean * c.mean;              // self.mean ** 2 in fp32, promoted against the fp64 sum
    c.var = (float)(s2 / n - (double)m2);
    c.std = sqrtf(c.var);
  } else if (method == WVN_CONF_KALMAN_FILTER) {  // update_kalman_filter: scalar KF, process noise 0.2, measurement noise 1
    float m = (float)cs[WVN_CONF_S_MEAN], v = c.var;
    if (st[0] > 0.0) {                             // a step without positives leaves the filter where it is
      const float z = (float)(st[1] / st[0]);
      const float vp = v + 0.2f;
      const float k = vp * (1.f / (vp + 1.f));
      m = m + k * (z - m);
      v = (1.f - k) * vp;
    }
    c.mean = m; c.var = v; c.std = sqrtf(v);
  } else if (method == WVN_CONF_MOVING_AVERAGE) {  // update_moving_average: the positives of the last 5 steps (this one included)
    const int head = state_int(cs[WVN_CONF_S_HEAD], WVN_CONF_WINDOW - 1), fill = state_int(cs[WVN_CONF_S_FILL], WVN_CONF_WINDOW);
    const int keep = fill < WVN_CONF_WINDOW - 1 ? fill : WVN_CONF_WINDOW - 1;
    double n = 0, s = 0, s2 = 0;
    for (int i = keep; i >= 1; --i) {              // oldest first, then this step
      const double* e = cs + WVN_CONF_S_RING + 3 * ((head - i + WVN_CONF_WINDOW) % WVN_CONF_WINDOW);
      n += e[0]; s += e[1]; s2 += e[2];
    }
    n += st[0]; s += st[1]; s2 += st[2];
    const double sn[3] = {n, s, s2};
    const ConfStats cw = conf_stats(sn);
    c.mean = cw.mean; c.std = cw.std;
  } else {                                         // latest_measurement: this step's positives (var untouched)
    const ConfStats cl = conf_stats(st);
    c.mean = cl.mean; c.std = cl.std;
  }
  return c;
}

// phase C: commit the post-update statistic (one thread)
__device__ inline ConfPost conf_commit(int method, const double* st, double* cs) {
  const ConfPost c = conf_post(method, st, cs);
  if (method == WVN_CONF_RUNNING_MEAN) {
    cs[WVN_CONF_S_RUN_N] += st[0]; cs[WVN_CONF_S_RUN_SUM] += st[1]; cs[WVN_CONF_S_RUN_SUMSQ] += st[2];
  } else if (method == WVN_CONF_MOVING_AVERAGE) {
    const int head = state_int(cs[WVN_CONF_S_HEAD], WVN_CONF_WINDOW - 1), fill = state_int(cs[WVN_CONF_S_FILL], WVN_CONF_WINDOW);
    double* e = cs + WVN_CONF_S_RING + 3 * head;
    e[0] = st[0]; e[1] = st[1]; e[2] = st[2];
    cs[WVN_CONF_S_HEAD] = (double)((head + 1) % WVN_CONF_WINDOW);
    cs[WVN_CONF_S_FILL] = (double)(fill < WVN_CONF_WINDOW ? fill + 1 : WVN_CONF_WINDOW);
  }
  cs[WVN_CONF_S_MEAN] = c.mean; cs[WVN_CONF_S_VAR] = c.var; cs[WVN_CONF_S_STD] = c.std;
  return c;
}

// the training-row confidence returned by update(); xmin / xmax: min / max of loss_reco over all rows of the step (moving_average)
__device__ inline float conf_method(int method, float x, const ConfPost& c, float f, float xmin, float xmax) {
  if (method == WVN_CONF_KALMAN_FILTER) {
    if (x < c.mean) return 1.f;
    const float d = (x - c.mean) / (c.std * f);
    return expf(-(d * d) * 0.5f);
  }
  if (method == WVN_CONF_MOVING_AVERAGE) {   // clip to mean +- 2 std, then min-max scale over the step (clip is monotone)
    const float lo = c.mean - 2.f * c.std, hi = c.mean + 2.f * c.std;
    if (isnan(lo) || isnan(hi)) return NAN;  // torch.clip with a NaN bound
    const float xc = fminf(fmaxf(x, lo), hi), a = fminf(fmaxf(xmin, lo), hi), b = fminf(fmaxf(xmax, lo), hi);
    return (xc - a) / (b - a);
  }
  return confidence_of(x, c.mean, c.std, f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The gradient seed of TraversabilityLoss (loss.py:125-147), per row.  Every training kernel forms it here, with its own thread
// mapping and destinations: mlp_gradout_kernel (64 lanes per row), mlp_train_bwd_kernel (8), dmlp_bwd_kernel (16).
// ---------------------------------------------------------------------------------------------------------------------------
struct LossStep {                  // the constants of a step
  const double* stats;             // [4] the (global) statistic {n_lab, sum, sum^2, R}
  const double* cstate;            // nullptr: latest_measurement from stats alone; else the method's state
  const float* minmax;             // {max, -min} of loss_reco over the step (moving_average), or nullptr
  int method, balanced;
  float std_factor, w_trav, w_reco;
  int D;
};
struct Seed { float conf, wrow, raw, g0, cr; };   // confidence, weight and raw value of the row's trav loss, d/d(out[0]), factor of the reco gradient

// a real row: lr = its reconstruction loss, s = out[row][0] (behind the sigmoid); an absent row's seed is Seed{} (all zero)
__device__ inline Seed grad_seed(const LossStep& c, float lr, float s, float y, bool valid) {
  Seed o;
  const ConfStats cs = conf_stats(c.stats);
  if (c.cstate) {   // another method: the post-update statistic from the state and this step's (global) stats
    const ConfPost cp = conf_post(c.method, c.stats, c.cstate);
    const float xmax = c.minmax ? c.minmax[0] : 0.f, xmin = c.minmax ? -c.minmax[1] : 0.f;
    o.conf = conf_method(c.method, lr, cp, c.std_factor, xmin, xmax);
  } else {
    o.conf = confidence_of(lr, cs.mean, cs.std, c.std_factor);
  }
  const float Rtot = (float)c.stats[3], nv = (float)c.stats[0];
  const float diff = s - y;
  o.wrow = (valid || !c.balanced) ? 1.f : (1.f - o.conf);   // anomaly_balanced = False: the plain mean of the raw trav loss
  o.raw = diff * diff;
  o.g0 = (c.w_trav / Rtot) * o.wrow * 2.f * diff * s * (1.f - s);
  o.cr = valid ? (c.w_reco / (nv * (float)c.D)) * 2.f : 0.f;
  return o;
}
// element d of the seed: d/d(out[1 + d])
__device__ inline float seed_elem(const Seed& sd, float out, float x) { return sd.cr * (out - x); }
