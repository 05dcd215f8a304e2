"""The traversability grid map in plain numpy: the definition csrc/grid_map.hip is held to bit for bit (ops.grid_fuse_images,
ops.grid_sdf, ops.grid_carrot), and the float64 restatements tests/test_grid_map_host.py holds that definition to.

Grid convention (smart_carrot.py:140-150): N x N, axis 0 = map x, axis 1 = map y, cell (i, j) centred at
(cx + (i - N/2) r, cy + (j - N/2) r); NaN = unknown.  Every fp32 statement below is one rounding per operation, in the order the
kernel's header comment gives; the same function run with dtype=np.float64 is the restatement of the same rules."""
import math

import numpy as np

DEFAULT_DISCS = ((30, 15), (55, 20), (90, 25))   # smart_carrot.py:74-85 (distance, thickness / 2)
UNKNOWN = ("obstacle", "free", "neither")
FAR = 1 << 29
I32_MAX = np.iinfo(np.int32).max


# ------------------------------------------------------------------------------------------------------------------ message order
def layer_from_message(data, n_rows, n_cols):
    """smart_carrot.py:106-107."""
    return np.reshape(np.array(data), (n_rows, n_cols))[::-1, ::-1].transpose()


def layer_to_message(layer):
    """smart_carrot.py:164."""
    return np.asarray(layer)[::-1, ::-1].transpose().ravel()


# ------------------------------------------------------------------------------------------------------------------------ fusion
def fuse(maps, intrinsics, poses, elevation, layers, hits, center, resolution, alpha=0.5, min_depth=0.1, max_range=None,
         occlusion_margin=0.05, dtype=np.float32):
    """-> (layers [C,N,N], hits [N,N], info); the inputs are not modified.  ``info`` per camera: "fused" [N,N] bool (the camera changed the
    cell), "visible" [N,N] bool (the walk's verdict; True where no walk was taken), "pixel" [N,N] int (row-major pixel index, -1 where
    the projection was refused) and "boundary" [N,N]: the distance of the cell's decisions to the nearest decision boundary -- pixel
    rounding (pixels), depth limit (metres), occlusion margin (metres) -- and "range_gap" [N,N] = |L - max_range|."""
    f = dtype
    maps = np.asarray(maps, dtype=np.float32)
    B, C, H, W = maps.shape
    elev = np.asarray(elevation, dtype=np.float32).astype(f)
    N = elev.shape[0]
    out = np.array(layers, dtype=np.float32).astype(f).reshape(C, N, N)
    hits = np.array(hits, dtype=np.int32)
    cx, cy, r = f(np.float32(center[0])), f(np.float32(center[1])), f(np.float32(resolution))
    al, mind, marg = f(np.float32(alpha)), f(np.float32(min_depth)), f(np.float32(occlusion_margin))
    maxr = f(np.inf) if max_range is None else f(np.float32(max_range))
    half = f(N) * f(0.5)
    hp = half + f(0.5)
    inv_r = f(1.0) / r
    oma = f(1.0) - al
    idx = np.arange(N).astype(f)
    x = np.broadcast_to((cx + (idx - half) * r)[:, None], (N, N)).astype(f)
    y = np.broadcast_to((cy + (idx - half) * r)[None, :], (N, N)).astype(f)
    known = ~np.isnan(elev)
    e = np.where(known, elev, f(0))
    info = []
    with np.errstate(all="ignore"):
        for b in range(B):
            T = np.asarray(poses[b], dtype=np.float32).astype(f)
            K = np.asarray(intrinsics[b], dtype=np.float32).astype(f)
            pc = []
            for k in range(3):
                r0, r1, r2 = T[0, k], T[1, k], T[2, k]
                tc = -((r0 * T[0, 3] + r1 * T[1, 3]) + r2 * T[2, 3])
                pc.append(((r0 * x + r1 * y) + r2 * e) + tc)
            ok = known & (pc[2] > mind)
            boundary = np.where(known, np.abs(pc[2] - mind), np.inf)
            xp = ((K[0, 0] * pc[0] + K[0, 1] * pc[1]) + K[0, 2] * pc[2]) + K[0, 3]
            yp = ((K[1, 0] * pc[0] + K[1, 1] * pc[1]) + K[1, 2] * pc[2]) + K[1, 3]
            zp = ((K[2, 0] * pc[0] + K[2, 1] * pc[1]) + K[2, 2] * pc[2]) + K[2, 3]
            s = np.where(np.abs(zp) > f(1e-8), f(1.0) / (zp + f(1e-8)), f(1.0)).astype(f)
            uh, vh = xp * s + f(0.5), yp * s + f(0.5)
            pu, pv = np.floor(uh), np.floor(vh)
            boundary = np.where(ok, np.minimum(boundary, np.minimum(np.abs(uh - np.round(uh)), np.abs(vh - np.round(vh)))), boundary)
            ok &= (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
            dx, dy, dz = T[0, 3] - x, T[1, 3] - y, T[2, 3] - e
            L = np.sqrt(dx * dx + dy * dy)
            range_gap = np.where(ok, np.abs(L - maxr), np.inf)
            ok &= L <= maxr
            iu, iv = np.where(ok, pu, 0).astype(np.int64), np.where(ok, pv, 0).astype(np.int64)
            val = maps[b][:, iv, iu].astype(f)                      # [C,N,N]
            ok &= (~np.isnan(val)).any(0)
            pixel = np.where(ok, iv * W + iu, -1)
            step = r / L
            nsteps = np.where(ok, np.floor(L / r), 0).astype(np.int64)
            visible = np.ones((N, N), dtype=bool)
            alive = ok.copy()
            for k in range(1, int(nsteps.max()) + 1 if ok.any() else 1):
                alive &= k <= nsteps
                if not alive.any():
                    break
                t = f(k) * step
                qx, qy, qz = x + t * dx, y + t * dy, e + t * dz
                fi, fj = np.floor((qx - cx) * inv_r + hp), np.floor((qy - cy) * inv_r + hp)
                inside = (fi >= 0) & (fi < N) & (fj >= 0) & (fj < N)
                alive &= inside
                he = elev[np.where(alive, fi, 0).astype(np.int64), np.where(alive, fj, 0).astype(np.int64)]
                fin = alive & np.isfinite(he)
                boundary = np.where(fin, np.minimum(boundary, np.abs((he - qz) - marg)), boundary)
                occluded = fin & ((he - qz) > marg)
                visible &= ~occluded
                alive &= ~occluded
            fused = ok & visible
            for c in range(C):
                take = fused & ~np.isnan(val[c])
                old = out[c]
                out[c] = np.where(take, np.where(np.isnan(old), val[c], old * oma + al * val[c]), old)
            hits = hits + fused.astype(np.int32)
            info.append({"fused": fused, "visible": visible, "pixel": pixel, "boundary": boundary, "range_gap": range_gap})
    return out, hits, info


# --------------------------------------------------------------------------------------------------------------------------- sdf
def classify(layer, threshold, unknown):
    """-> (obstacle, free) bool [N,N]."""
    layer = np.asarray(layer, dtype=np.float32)
    nan = np.isnan(layer)
    with np.errstate(invalid="ignore"):
        below = layer < np.float32(threshold)
    obstacle = (below & ~nan) | (nan & (unknown == "obstacle"))
    free = (~below & ~nan) | (nan & (unknown == "free"))
    return obstacle, free


def edt_squared(member):
    """Exact squared Euclidean distance (in cells, int64 [N,N]) of every cell to the nearest cell of ``member``; FAR or more where the set
    is empty.  The separable two-pass integer form: the nearest member of the same column, then per row min over k of (j - k)^2 + g(k)."""
    N = member.shape[0]
    rows = np.arange(N)[:, None]
    up = np.maximum.accumulate(np.where(member, rows, -FAR), axis=0)                      # nearest member row at or above
    down = np.minimum.accumulate(np.where(member, rows, FAR)[::-1], axis=0)[::-1]         # at or below
    g = np.minimum(rows - up, down - rows).astype(np.int64)
    g = np.where(g >= N, FAR, g * g)
    jk = (np.arange(N)[:, None] - np.arange(N)[None, :]) ** 2                            # [j, k]
    out = np.empty((N, N), dtype=np.int64)
    for i in range(N):
        out[i] = (jk + g[i][None, :]).min(1)
    return out


def sdf(layer, threshold, resolution, unknown="obstacle"):
    """-> (sdf fp32 [N,N], d2 int32 [N,N])."""
    obstacle, free = classify(layer, threshold, unknown)
    to_obstacle, to_free = edt_squared(obstacle), edt_squared(free)
    mag = np.where(free, to_obstacle, np.where(obstacle, to_free, 0))
    none = mag >= FAR
    sign = np.where(free, 1, np.where(obstacle, -1, 0))
    d2 = (sign * np.where(none, I32_MAX, mag)).astype(np.int32)
    with np.errstate(invalid="ignore"):
        dist = np.float32(resolution) * np.sqrt(np.where(none, 0, mag).astype(np.float32))
    dist = np.where(none, np.float32(np.inf), dist).astype(np.float32)
    out = np.where(sign > 0, dist, np.where(sign < 0, -dist, np.float32(np.nan))).astype(np.float32)
    return out, d2


def edt_squared_brute(member):
    """O(N^4) minimum over the members."""
    N = member.shape[0]
    ii, jj = np.nonzero(member)
    if ii.size == 0:
        return np.full((N, N), FAR, dtype=np.int64)
    a, b = np.mgrid[0:N, 0:N]
    return ((a[..., None] - ii) ** 2 + (b[..., None] - jj) ** 2).min(-1)


# ------------------------------------------------------------------------------------------------------------------------ carrot
def disc_centres(N, yaw, discs=DEFAULT_DISCS):
    """[(row, column, radius)]: smart_carrot.py:74-85 -- cv2.circle's centre (center_x, center_y) is (column, row)."""
    return [(int(N / 2 + math.cos(yaw) * d), int(N / 2 + math.sin(yaw) * d), rad) for d, rad in discs]


def pattern(N, yaw, discs=DEFAULT_DISCS):
    """True inside the search pattern; cv2.circle(radius 0, thickness t) is taken to be the disc di^2 + dj^2 <= (t/2)^2."""
    i, j = np.mgrid[0:N, 0:N]
    keep = np.zeros((N, N), dtype=bool)
    for ci, cj, rad in disc_centres(N, yaw, discs):
        keep |= (i - ci) ** 2 + (j - cj) ** 2 <= rad * rad
    return keep


def elevation_mask(elevation):
    """smart_carrot.py:89-94: NaN elevation dilated by a 3 x 3 kernel; cells outside the grid are ignored."""
    bad = np.isnan(np.asarray(elevation))
    N = bad.shape[0]
    p = np.zeros((N + 2, N + 2), dtype=bool)
    p[1:-1, 1:-1] = bad
    out = np.zeros_like(bad)
    for di in range(3):
        for dj in range(3):
            out |= p[di:di + N, dj:dj + N]
    return out


def _select(score, center, resolution, N, f):
    ninf = -np.inf
    flat = score.ravel()
    best = flat.max()
    idx = int(np.nonzero(flat == best)[0][0])       # np.where(...)[0]: the lowest row-major index
    i, j = divmod(idx, N)
    half = f(N) * f(0.5)
    r = f(np.float32(resolution))
    x = (f(i) - half) * r + f(np.float32(center[0]))
    y = (f(j) - half) * r + f(np.float32(center[1]))
    return {"i": i, "j": j, "found": int(best > ninf), "score": best, "x": x, "y": y, "masked": score}


def carrot(sdf, elevation, yaw, center, resolution, distance_force_factor=0.0, center_force_factor=0.0, discs=DEFAULT_DISCS):
    """The fp32 statement the kernel reproduces -> dict(i, j, found, score, x, y, masked)."""
    f = np.float32
    s = np.asarray(sdf, dtype=np.float32).copy()
    N = s.shape[0]
    c = N // 2
    i, j = np.mgrid[0:N, 0:N]
    with np.errstate(all="ignore"):
        if distance_force_factor > 0:
            d = np.sqrt(((i - c) ** 2 + (j - c) ** 2).astype(f))
            d = d / np.sqrt(f(2 * c * c))
            d = d * f(distance_force_factor)
            s = s + d
        if center_force_factor > 0:
            cf = np.abs(f(math.cos(yaw)) * (j - c).astype(f) - f(math.sin(yaw)) * (i - c).astype(f))
            s = s - cf * f(center_force_factor)
    s = s.astype(f)
    s[~pattern(N, yaw, discs)] = -np.inf
    s[elevation_mask(elevation)] = -np.inf
    s[np.isnan(s)] = -np.inf
    return _select(s, center, resolution, N, f)


def carrot_float64(sdf, elevation, yaw, center, resolution, distance_force_factor=0.0, center_force_factor=0.0, discs=DEFAULT_DISCS):
    """smart_carrot.py:53-69, 126-150 transcribed line by line (float64, as numpy promotes there), with the disc rule above in cv2's
    place and NaN scores sent to -inf."""
    s = np.asarray(sdf, dtype=np.float32)
    H, W = s.shape
    with np.errstate(all="ignore"):
        if distance_force_factor > 0:
            distance_force = np.zeros((H, W))
            for xx in range(H):
                for yy in range(W):
                    distance_force[xx, yy] = math.sqrt((xx - int(H / 2)) ** 2 + (yy - int(W / 2)) ** 2)
            distance_force /= distance_force.max()
            distance_force *= distance_force_factor
            s = s + distance_force
        if center_force_factor > 0:
            xv, yv = np.meshgrid(np.arange(0, H), np.arange(0, W))
            center_force = np.abs(np.cos(yaw) * (xv - int(H / 2)) - np.sin(yaw) * (yv - int(W / 2)))
            s = s - center_force * center_force_factor
    s = np.array(s, dtype=np.float64)
    s[~pattern(H, yaw, discs)] = -np.inf
    s[elevation_mask(elevation)] = -np.inf
    s[np.isnan(s)] = -np.inf
    return _select(s, center, resolution, H, np.float64)
