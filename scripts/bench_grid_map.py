"""The traversability grid map (csrc/grid_map.hip) at the reference's configuration, one JSON line: an 8 m map at 0.04 m (N = 200),
two cameras at 448 x 448, C = 2 (traversability, confidence).  Per call and per kernel, on the same GPU:

    hip          ops.grid_fuse_images, ops.grid_sdf, ops.grid_carrot, and the callback gm.fuse_images -> gm.sdf -> carrot.goal
    torch        the same definitions as torch operations: a vectorised projection, the occlusion walk as a loop of vectorised steps
                 (as many as the farthest cell needs: known on the host from the poses), the EDT's two passes as [N,N,N] broadcast
                 minima, the carrot as element-wise operations + max_pool2d + argmax.  Its results are compared (``*_differing``),
                 not asserted: torch fuses multiply-adds where the kernels do not.
    scipy        scipy.ndimage.distance_transform_edt on the host for the SDF, with the download of the layer and the upload of the
                 result it would need (host clock around a synchronise).

HIP-event timed after warm-up on one stream; every figure is the median over ``--repeats`` windows of ``--iters`` calls, ms per call.
``bytes_*`` is what each kernel must move at least once (inputs read once, outputs written once).

    python scripts/bench_grid_map.py [--iters N] [--warmup N] [--repeats N]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid_map_cases as GC  # noqa: E402
import grid_map_ref as G  # noqa: E402

from wild_visual_navigation_amd import ops  # noqa: E402
from wild_visual_navigation_amd.grid_map import SmartCarrot, TraversabilityGridMap  # noqa: E402


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


def host_timed(fn, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return statistics.median(out)


def scene(dev, N=200, r=0.04, HW=448):
    """Rolling ground with a wall, a block and unknown cells; two cameras on the robot at the map centre, front and front-left."""
    rng = np.random.default_rng(7)
    ctr = (12.0, -7.0)
    i, j = np.mgrid[0:N, 0:N]
    elev = (0.1 * np.sin(i / 23.0) * np.cos(j / 31.0) + rng.uniform(-0.005, 0.005, (N, N))).astype(np.float32)
    elev[130, 40:160] = 0.8
    elev[60:70, 150:165] = 0.5
    elev[rng.uniform(size=(N, N)) < 0.02] = np.nan
    maps = rng.uniform(0, 1, (2, 2, HW, HW)).astype(np.float32)
    K = np.stack([GC.intrinsics(170.0, 170.0, HW, HW), GC.intrinsics(140.0, 140.0, HW, HW)])
    poses = np.stack([GC.look_at((ctr[0] - 0.4, ctr[1] + 0.013, 0.7), (ctr[0] + 2.0, ctr[1], 0.0)),
                      GC.look_at((ctr[0] - 0.3, ctr[1] - 0.3, 0.75), (ctr[0] + 1.0, ctr[1] + 1.8, 0.0))])
    return ctr, elev, maps, K, poses


class TorchForm:
    def __init__(self, N, r, ctr, poses, dev):
        self.N, self.r, self.ctr, self.dev = N, r, ctr, dev
        idx = torch.arange(N, device=dev, dtype=torch.float32)
        self.x = (ctr[0] + (idx - N * 0.5) * r)[:, None].expand(N, N)
        self.y = (ctr[1] + (idx - N * 0.5) * r)[None, :].expand(N, N)
        corners = [(ctr[0] + sx * N * r / 2, ctr[1] + sy * N * r / 2) for sx in (-1, 1) for sy in (-1, 1)]
        self.max_steps = [int(max(math.hypot(p[0, 3] - cx, p[1, 3] - cy) for cx, cy in corners) / r) + 1 for p in poses]
        k = torch.arange(N, device=dev)
        self.dk2 = ((k[:, None] - k[None, :]) ** 2).to(torch.int32)            # [a, b] = (a - b)^2
        self.ii, self.jj = torch.meshgrid(k, k, indexing="ij")

    def fuse(self, maps, K, T, elev, layers, hits, alpha=0.5, min_depth=0.1, margin=0.05):
        N, r = self.N, self.r
        B, C, H, W = maps.shape
        known = ~torch.isnan(elev)
        e = torch.where(known, elev, torch.zeros_like(elev))
        pts = torch.stack([self.x, self.y, e, torch.ones_like(e)], -1)                       # [N,N,4]
        out = [l.clone() for l in layers]
        hits = hits.clone()
        for b in range(B):
            Rt = T[b, :3, :3].T                                                               # rigid inverse: R^T, -R^T t
            pc = pts[..., :3] @ Rt.T - Rt @ T[b, :3, 3]
            pc = torch.cat([pc, torch.ones_like(pc[..., :1])], -1)
            q = pc @ K[b].T
            u, v = torch.floor(q[..., 0] / q[..., 2] + 0.5), torch.floor(q[..., 1] / q[..., 2] + 0.5)
            ok = known & (pc[..., 2] > min_depth) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
            iu, iv = u.clamp(0, W - 1).long(), v.clamp(0, H - 1).long()
            val = maps[b][:, iv, iu]
            ok &= ~torch.isnan(val).all(0)
            dx, dy, dz = T[b, 0, 3] - self.x, T[b, 1, 3] - self.y, T[b, 2, 3] - e
            L = torch.sqrt(dx * dx + dy * dy)
            nsteps = torch.floor(L / r)
            step = r / L
            alive, visible = ok.clone(), torch.ones_like(ok)
            for k in range(1, self.max_steps[b] + 1):
                alive = alive & (nsteps >= k)
                t = k * step
                fi = torch.floor((self.x + t * dx - self.ctr[0]) / r + (N * 0.5 + 0.5))
                fj = torch.floor((self.y + t * dy - self.ctr[1]) / r + (N * 0.5 + 0.5))
                alive = alive & (fi >= 0) & (fi < N) & (fj >= 0) & (fj < N)
                he = elev[fi.clamp(0, N - 1).long(), fj.clamp(0, N - 1).long()]
                occluded = alive & torch.isfinite(he) & (he - (e + t * dz) > margin)
                visible = visible & ~occluded
                alive = alive & ~occluded
            fused = ok & visible
            for c in range(C):
                take = fused & ~torch.isnan(val[c])
                out[c] = torch.where(take, torch.where(torch.isnan(out[c]), val[c], out[c] * (1 - alpha) + alpha * val[c]), out[c])
            hits = hits + fused.int()
        return out, hits

    def _edt2(self, member):
        far = 1 << 29
        g = torch.where(member[None, :, :], self.dk2[:, :, None], far).amin(1)              # [i, k]: nearest member of column k
        return (self.dk2[None, :, :] + g[:, None, :]).amin(2)                               # [i, j]: min over k of (j - k)^2 + g[i, k]

    def sdf(self, layer, threshold, r):
        nan = torch.isnan(layer)
        obstacle = (layer < threshold) | nan
        free = ~obstacle
        d2 = torch.where(free, self._edt2(obstacle), -self._edt2(free))
        return torch.sign(d2) * r * torch.sqrt(d2.abs().float()), d2

    def carrot(self, sdf, elev, yaw, dff, cff, discs=G.DEFAULT_DISCS):
        N = self.N
        c = N // 2
        s = sdf
        if dff > 0:
            d = torch.sqrt(((self.ii - c) ** 2 + (self.jj - c) ** 2).float())
            s = s + d / math.sqrt(2 * c * c) * dff
        if cff > 0:
            s = s - torch.abs(math.cos(yaw) * (self.jj - c).float() - math.sin(yaw) * (self.ii - c).float()) * cff
        keep = torch.zeros_like(s, dtype=torch.bool)
        for ci, cj, rad in G.disc_centres(N, yaw, discs):
            keep |= (self.ii - ci) ** 2 + (self.jj - cj) ** 2 <= rad * rad
        bad = F.max_pool2d(torch.isnan(elev).float()[None, None], 3, 1, 1)[0, 0] > 0
        s = torch.where(keep & ~bad & ~torch.isnan(s), s, torch.full_like(s, -math.inf))
        idx = torch.argmax(s)
        return idx, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, r, HW = 200, 0.04, 448
    ctr, elev_h, maps_h, K_h, poses_h = scene(dev, N, r, HW)
    elev, maps, K, T = (torch.from_numpy(v).to(dev) for v in (elev_h, maps_h, K_h, poses_h))
    nan = float("nan")
    layers = [torch.full((N, N), nan, device=dev) for _ in range(2)]
    hits = torch.zeros(N, N, dtype=torch.int32, device=dev)
    tf = TorchForm(N, r, ctr, poses_h, dev)

    def fuse():
        ops.grid_fuse_images(maps, K, T, elev, layers, hits, ctr, r)

    # results first: the torch form is compared
    fuse()
    got = [l.clone() for l in layers], hits.clone()
    blank = [torch.full((N, N), nan, device=dev) for _ in range(2)]
    t_layers, t_hits = tf.fuse(maps, K, T, elev, blank, torch.zeros_like(hits))
    fuse_diff = int((t_hits != got[1]).sum())
    fuse_err = float(torch.nan_to_num(t_layers[0] - got[0][0]).abs().max())
    trav = got[0][0]
    sdf, d2 = ops.grid_sdf(trav, 0.5, r)
    t_sdf, t_d2 = tf.sdf(trav, 0.5, r)
    sdf_diff = int((t_d2 != d2).sum())
    yaw, dff, cff = 0.3, 0.1, 0.001
    cell, goal, _ = ops.grid_carrot(sdf, elev, yaw, ctr, r, dff, cff)
    t_idx, _ = tf.carrot(sdf, elev, yaw, dff, cff)
    carrot_same = int(t_idx.item() == cell[0].item() * N + cell[1].item())

    gm = TraversabilityGridMap(length=N * r, resolution=r, device=dev, center=ctr)
    gm.set_elevation(elev)
    carrot = SmartCarrot(dff, cff)

    def callback():
        gm.fuse_images(maps, K, T)
        gm.sdf()
        return carrot.goal(gm, yaw)

    def scipy_sdf():
        from scipy import ndimage

        layer = trav.cpu().numpy()
        obstacle = (layer < 0.5) | np.isnan(layer)
        out = np.where(obstacle, -ndimage.distance_transform_edt(obstacle), ndimage.distance_transform_edt(~obstacle)) * r
        return torch.from_numpy(out.astype(np.float32)).to(dev)

    w, it, rp = a.warmup, a.iters, a.repeats
    t = {"fuse_ms": timed(fuse, w, it, rp)}
    t["sdf_ms"] = timed(lambda: ops.grid_sdf(trav, 0.5, r, out=(sdf, d2)), w, it, rp)
    t["carrot_ms"] = timed(lambda: ops.grid_carrot(sdf, elev, yaw, ctr, r, dff, cff), w, it, rp)
    t["callback_ms"] = timed(callback, w, it, rp)
    t["callback_host_ms"] = host_timed(callback, w, it, rp)
    t["torch_fuse_ms"] = timed(lambda: tf.fuse(maps, K, T, elev, blank, hits), 2, max(1, it // 40), rp)
    t["torch_sdf_ms"] = timed(lambda: tf.sdf(trav, 0.5, r), w, max(1, it // 10), rp)
    t["torch_carrot_ms"] = timed(lambda: tf.carrot(sdf, elev, yaw, dff, cff), w, max(1, it // 4), rp)
    t["scipy_sdf_with_transfers_ms"] = host_timed(scipy_sdf, 2, max(1, it // 20), rp)
    layer_bytes = N * N * 4
    res = {"bench": "grid_map", "device": torch.cuda.get_device_name(0), "N": N, "resolution": r, "cameras": 2, "image": [HW, HW],
           "channels": 2, "iters": it, "warmup": w, "repeats": rp,
           # elevation + 2 layers read and written + hits read and written + the sampled pixels (at most one per cell, camera and channel)
           "bytes_fuse": layer_bytes * (1 + 2 * 2 + 2) + int(got[1].sum().item()) * 2 * 4 + 2 * 2 * 64,
           "bytes_sdf": layer_bytes * 3, "bytes_carrot": layer_bytes * 2,
           "cells_fused": int((got[1] > 0).sum()), "camera_cell_pairs_fused": int(got[1].sum()),
           "torch_fuse_hits_differing": fuse_diff, "torch_fuse_max_abs_diff": fuse_err, "torch_sdf_d2_differing": sdf_diff,
           "torch_carrot_same_cell": carrot_same, "torch_walk_steps": tf.max_steps}
    res.update({k: round(v, 4) for k, v in t.items()})
    res["torch_over_hip_fuse"] = round(t["torch_fuse_ms"] / t["fuse_ms"], 1)
    res["torch_over_hip_sdf"] = round(t["torch_sdf_ms"] / t["sdf_ms"], 1)
    res["torch_over_hip_carrot"] = round(t["torch_carrot_ms"] / t["carrot_ms"], 1)
    res["scipy_over_hip_sdf"] = round(t["scipy_sdf_with_transfers_ms"] / t["sdf_ms"], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
