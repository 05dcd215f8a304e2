"""Elevation from depth (csrc/elevation.hip) at the reference's configuration, one JSON line: an 8 m map at 0.04 m (N = 200), six depth
cameras at 640 x 480 around the robot (anymal_sensor_parameter.yaml feeds elevation_mapping_cupy from six depth cameras), one callback =
all six images in two launches.  Per callback, on the same GPU:

    hip          ops.grid_elevation_depth: fp32 metres and uint16 millimetres, without and with ray clearing; and with every point
                 rejected as "near" (min_valid_distance = 1 km: the loads, the back-projection and the rejection arithmetic without
                 gate reads, combining or sums), which bounds the share of the time that the gate, the combining and the atomics take.
                 The wave-level combining of equal cells is judged by running this script on a second build of the library with
                 csrc/elevation.hip compiled with -DWVN_ELEV_NO_COMBINE=1 (one set of atomics per point), loaded through WVN_LIB_PATH:
                 ``digest*`` (SHA-256 of the resulting elevation and variance layers) must agree between the two builds.
    torch        the same definition as torch operations: vectorised back-projection and rejection, ``index_add_`` of fp32 weights
                 (floating-point atomics: NOT reproducible from run to run, and not the kernels' fixed-point sums), an element-wise
                 fusion; ray clearing as a loop of vectorised steps.  Compared (``torch_*``), not asserted.

The layers are reset to the same prior before every callback (two 160 KB device copies), so that every timed callback does the same
work; ``reset_ms`` is that reset alone and is subtracted in ``*_net_ms``.  HIP-event timed after warm-up on one stream; every figure is
the median over ``--repeats`` windows of ``--iters`` callbacks, ms per callback.  ``bytes_min`` is what a callback must move at least once.
``--trace FORM`` runs 20 callbacks of one form (f32, u16, f32_clear, u16_clear, f32_all_rejected) and nothing else, for
``rocprofv3 --kernel-trace --stats``.

    python scripts/bench_elevation.py [--iters N] [--warmup N] [--repeats N] [--label TEXT] [--trace FORM]
"""
import argparse
import hashlib
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid_map_cases as GC  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s (MI355X)


def timed(fn, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out)


def scene(N=200, r=0.04, H=480, W=640, cameras=6):
    """Six cameras 0.55 m above flat ground, looking outwards and down, 1 cm depth noise; a prior map that knows 70 % of the ground
    and holds clutter 0.4 m high that the rays see through (work for the ray clearing)."""
    rng = np.random.default_rng(11)
    ctr = (12.0, -7.0)
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 380.0
    K[0, 2], K[1, 2] = W / 2 - 0.5, H / 2 - 0.5
    poses, depth = [], []
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    for k in range(cameras):
        a = 2 * math.pi * k / cameras
        T = GC.look_at((ctr[0] + 0.3 * math.cos(a), ctr[1] + 0.3 * math.sin(a), 0.55), (ctr[0] + 2.0 * math.cos(a), ctr[1] + 2.0 * math.sin(a), 0.0))
        d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1) @ T[:3, :3].astype(np.float64).T
        with np.errstate(all="ignore"):
            z = np.where(d[..., 2] < -1e-3, -float(T[2, 3]) / d[..., 2], 0.0)
        z = np.where((z > 0) & (z < 10.0), z + rng.normal(0, 0.01, z.shape), 0.0)
        poses.append(T)
        depth.append(z.astype(np.float32))
    elev = rng.uniform(-0.01, 0.01, (N, N)).astype(np.float32)
    elev[rng.uniform(size=(N, N)) < 0.02] = 0.4
    elev[rng.uniform(size=(N, N)) < 0.3] = np.nan
    var = np.where(np.isfinite(elev), 0.01, 1000.0).astype(np.float32)
    return ctr, np.stack(depth), np.stack([K] * cameras), np.stack(poses), elev, var


class TorchForm:
    """The definition as torch operations on fp32, sums by index_add_ (floating-point atomics)."""

    def __init__(self, N, r, ctr, H, W, dev, p):
        self.N, self.r, self.ctr, self.p = N, r, ctr, p
        self.u = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
        self.v = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
        self.max_steps = int(min(p["max_ray_length"], N * r * math.sqrt(2)) / r)

    def callback(self, depth, K, T, elev, var, clear_rays):
        N, r, p = self.N, self.r, self.p
        z = depth
        x = (self.u - K[:, 0, 2, None, None]) * (z / K[:, 0, 0, None, None])
        y = (self.v - K[:, 1, 2, None, None]) * (z / K[:, 1, 1, None, None])
        pts = torch.stack([x, y, z], -1)                                                      # [B,H,W,3]
        q = torch.einsum("bij,bhwj->bhwi", T[:, :3, :3], pts) + T[:, None, None, :3, 3]
        t = T[:, None, None, :3, 3]
        d = t - q
        L = torch.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
        up = q[..., 2] - t[..., 2]
        d2 = (pts ** 2).sum(-1)
        ok = torch.isfinite(z) & (z != 0) & (d2 >= p["min_valid_distance"] ** 2) & (up <= p["max_height_range"]) & \
            (up <= torch.clamp(L - p["ramped_height_range_b"], min=0) * p["ramped_height_range_a"] + p["ramped_height_range_c"])
        fi = torch.floor((q[..., 0] - self.ctr[0]) / r + (N * 0.5 + 0.5))
        fj = torch.floor((q[..., 1] - self.ctr[1]) / r + (N * 0.5 + 0.5))
        ok &= (fi >= 0) & (fi < N) & (fj >= 0) & (fj < N)
        cell = (fi.clamp(0, N - 1) * N + fj.clamp(0, N - 1)).long()
        h, hv = elev.reshape(-1)[cell], var.reshape(-1)[cell]
        gated = ok & torch.isfinite(h) & ((q[..., 2] - h).abs() > p["mahalanobis_thresh"] * torch.sqrt(hv))
        inl = ok & ~gated
        w = torch.where(inl, 1.0 / (p["sensor_noise_factor"] * d2), torch.zeros_like(d2))
        flat = cell.reshape(-1)
        Sw = torch.zeros(N * N, device=z.device).index_add_(0, flat, w.reshape(-1))
        Swz = torch.zeros(N * N, device=z.device).index_add_(0, flat, (w * q[..., 2]).reshape(-1))
        n_out = torch.zeros(N * N, device=z.device).index_add_(0, flat, gated.reshape(-1).float())
        Sw, Swz, n_out = Sw.reshape(N, N), Swz.reshape(N, N), n_out.reshape(N, N)
        got = Sw > 0
        v_m, z_m = 1.0 / Sw, Swz / Sw
        known = torch.isfinite(elev)
        h_new = torch.where(known, (elev * v_m + z_m * var) / (var + v_m), z_m)
        var_new = torch.where(known, (var * v_m) / (var + v_m), v_m)
        out_h = torch.where(got, h_new, elev)
        out_v = torch.where(got | (n_out > 0), torch.clamp(torch.where(got, var_new, var) + p["outlier_variance"] * n_out, max=p["max_variance"]), var)
        if clear_rays:
            walk = (ok).reshape(-1)
            qq, dd, LL = q.reshape(-1, 3), d.reshape(-1, 3), L.reshape(-1)
            step, nsteps = r / LL, torch.clamp(torch.floor(LL / r), max=math.floor(p["max_ray_length"] / r))
            contradicted = torch.zeros(N * N, device=z.device)
            alive = walk.clone()
            for s in range(1, self.max_steps + 1):
                alive = alive & (nsteps >= s)
                c = qq + (s * step)[:, None] * dd
                ci = torch.floor((c[:, 0] - self.ctr[0]) / r + (N * 0.5 + 0.5))
                cj = torch.floor((c[:, 1] - self.ctr[1]) / r + (N * 0.5 + 0.5))
                alive = alive & (ci >= 0) & (ci < N) & (cj >= 0) & (cj < N)
                at = (ci.clamp(0, N - 1) * N + cj.clamp(0, N - 1)).long()
                he = elev.reshape(-1)[at]
                hit = alive & (at != flat) & torch.isfinite(he) & (he - c[:, 2] > p["clear_margin"])
                contradicted.index_add_(0, at, hit.float())
            cleared = (~got) & (contradicted.reshape(N, N) >= p["clear_min_rays"])
            out_h = torch.where(cleared, torch.full_like(out_h, float("nan")), out_h)
            out_v = torch.where(cleared, torch.full_like(out_v, p["initial_variance"]), out_v)
        return out_h, out_v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--label", default="", help="copied into the JSON line (which build of the library this is)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_elevation: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    N, r, H, W, B = 200, 0.04, 480, 640, 6
    ctr, depth_h, K_h, T_h, elev_h, var_h = scene(N, r, H, W, B)
    depth, K, T, elev0, var0 = (torch.from_numpy(v).to(dev) for v in (depth_h, K_h, T_h, elev_h, var_h))
    depth_u16 = torch.from_numpy(np.clip(np.rint(depth_h * 1000.0), 0, 65535).astype(np.uint16)).to(dev)
    elev, var = elev0.clone(), var0.clone()
    nan = float("nan")
    layers = [torch.full((N, N), nan, device=dev) for _ in range(2)]
    hits = torch.zeros(N, N, dtype=torch.int32, device=dev)
    ws = ops.grid_elevation_workspace(N, dev)
    params = ops.grid_elevation_params()
    far = ops.grid_elevation_params(min_valid_distance=1000.0)

    def reset():
        elev.copy_(elev0)
        var.copy_(var0)

    def hip(d=depth, clear=False, p=params):
        reset()
        return ops.grid_elevation_depth(d, K, T, elev, var, layers, hits, ctr, r, clear_rays=clear, params=p, workspace=ws)

    forms = {"f32": dict(), "u16": dict(d=depth_u16), "f32_clear": dict(clear=True), "u16_clear": dict(d=depth_u16, clear=True),
             "f32_all_rejected": dict(p=far)}
    if a.trace is not None:
        for _ in range(20):
            hip(**forms[a.trace])
        torch.cuda.synchronize()
        return

    tf = TorchForm(N, r, ctr, H, W, dev, dict(ops.GRID_ELEVATION_DEFAULTS))
    res = {"bench": "elevation", "label": a.label, "library": os.path.basename(os.path.dirname(_lib.LIB_PATH)), "device": torch.cuda.get_device_name(0), "N": N, "resolution": r, "cameras": B, "image": [H, W],
           "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats}
    # results first: the class counters, a digest of the layers, and the agreement of the torch form
    for name, clear in (("", False), ("_clear", True)):
        stats = hip(clear=clear)
        res["stats" + name] = dict(zip(_lib.GRID_ELEVATION_STATS, stats.tolist()))
        got_h, got_v = elev.clone(), var.clone()
        res["digest" + name] = hashlib.sha256(got_h.cpu().numpy().tobytes() + got_v.cpu().numpy().tobytes()).hexdigest()[:16]
        t_h, t_v = tf.callback(depth, K, T, elev0, var0, clear)
        both = torch.isfinite(got_h) & torch.isfinite(t_h)
        res["torch_known_differing" + name] = int((torch.isfinite(got_h) != torch.isfinite(t_h)).sum())
        res["torch_max_abs_diff_elevation" + name] = float((got_h - t_h)[both].abs().max())
        res["cells_known_after" + name] = int(torch.isfinite(got_h).sum())
        res["cells_cleared" + name] = int((torch.isfinite(elev0) & ~torch.isfinite(got_h)).sum())
    t1 = tf.callback(depth, K, T, elev0, var0, False)[0]
    t2 = tf.callback(depth, K, T, elev0, var0, False)[0]
    res["torch_run_to_run_differing_bits"] = int((t1.view(torch.int32) != t2.view(torch.int32)).sum())
    w, it, rp = a.warmup, a.iters, a.repeats
    t = {"reset_ms": timed(reset, w, it, rp)}
    for name, kw in forms.items():
        t[name + "_ms"] = timed(lambda kw=kw: hip(**kw), w, it, rp)
    t["torch_ms"] = timed(lambda: tf.callback(depth, K, T, elev0, var0, False), 2, max(1, it // 10), rp)
    t["torch_clear_ms"] = timed(lambda: tf.callback(depth, K, T, elev0, var0, True), 1, 1, max(3, rp // 2 + 1))
    res.update({k: round(v, 4) for k, v in t.items()})
    for name in forms:
        res[name + "_net_ms"] = round(t[name + "_ms"] - t["reset_ms"], 4)
    # depth read once, elevation + variance read and written, the touched workspace cells written and read and zeroed (at most all)
    cell_bytes = N * N * (4 * 2 * 2 + 32 * 3)
    res["bytes_min_f32"], res["bytes_min_u16"] = B * H * W * 4 + cell_bytes, B * H * W * 2 + cell_bytes
    res["hbm_floor_us_f32"] = round(res["bytes_min_f32"] / HBM_PEAK * 1e6, 3)
    res["share_of_hbm_peak_f32"] = round(res["bytes_min_f32"] / HBM_PEAK / (res["f32_net_ms"] * 1e-3), 4)
    res["share_of_hbm_peak_u16"] = round(res["bytes_min_u16"] / HBM_PEAK / (res["u16_net_ms"] * 1e-3), 4)
    res["gate_combine_atomics_share_upper_bound"] = round(1 - res["f32_all_rejected_net_ms"] / res["f32_net_ms"], 3)
    res["torch_over_hip"] = round(t["torch_ms"] / res["f32_net_ms"], 1)
    res["torch_over_hip_clear"] = round(t["torch_clear_ms"] / res["f32_clear_net_ms"], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
