"""The elevation layer of the traversability grid map from depth images and point clouds, in plain numpy: the definition
csrc/elevation.hip is held to BIT FOR BIT (ops.grid_elevation_points / ops.grid_elevation_depth, TraversabilityGridMap.add_points /
add_depth), and the float64 sequential Kalman restatement tests/test_elevation_host.py holds that definition to.

Grid convention as tests/grid_map_ref.py: N x N, axis 0 = map x, axis 1 = map y, cell (i, j) centred at (cx + (i - N/2) r,
cy + (j - N/2) r); NaN elevation = unknown.  One call fuses every sensor b = 0 .. B-1 of a callback, and every point is judged against
the map AS IT WAS ON ENTRY, so the result does not depend on the order of the points or of the sensors.  Every fp32 statement below is
one rounding per operation, in the order written (the kernel's unit is compiled with -ffp-contract=off).

Per point p = (x, y, z) of sensor b (pose T = pose_sensor_in_map[b], t = its translation):
  depth form: pixel (v, u) with depth z (uint16: z = float(mm) / 1000.0f) is p = ((float(u) - K[0][2]) * (z / K[0][0]),
              (float(v) - K[1][2]) * (z / K[1][1]), z); z == 0, NaN or inf is no point (class "invalid").
  rejection, first match:
    invalid   a coordinate is not finite
    near      d2 = (x x + y y) + z z  <  min_valid_distance * min_valid_distance
    q[k] = ((T[k][0] x + T[k][1] y) + T[k][2] z) + t[k]                                 (the order csrc/grid_map.hip documents)
    high      q_z - t_z > max_height_range
    ramp      q_z - t_z > fmaxf(L - ramp_b, 0) * ramp_a + ramp_c,   L = sqrtf(dx dx + dy dy), (dx, dy, dz) = t - q
    outside   the nearest cell (floorf((q_x - cx) * (1 / r) + (N * 0.5f + 0.5f)), likewise y) is not inside the map
  gate: h, var = the cell's elevation and variance on entry; h finite and fabsf(q_z - h) > mahalanobis_thresh * sqrtf(var) -> the
    point is "gated": n_out[cell] += 1 and nothing else.
  otherwise (inlier):  v = sensor_noise_factor * d2,  w = 1.0f / v,
    wq = (int64) floorf(fminf(w, 4096 - 1/256) * 256)              0 <= wq <= 2^20 - 1
    zq = (int64) rintf((q_z - z_ref) * 16384)                      |zq| <= 2^21
    not (fabsf(q_z - z_ref) <= 128), or wq == 0 (a point more than ~71 m away at the default noise): class "unrepresentable", dropped;
    else S_w[cell] += wq, S_wz[cell] += wq * zq, n[cell] += 1.
  FORMAT BOUND: |wq zq| <= (2^20 - 1) 2^21 < 2^41, so with at most MAX_POINTS = 2^22 points per call |S_wz| < 2^63 and S_w < 2^42:
  int64 sums cannot overflow.  The entry points refuse more than 2^22 points (B * Pmax, B * H * W) before any launch.
  ray clearing (clear_rays): every point that passed rejection (gated, inlier or unrepresentable) walks towards its sensor,
    step = r / L,  s = 1 .. min(floorf(L / r), floorf(max_ray_length / r)):  t = float(s) * step,  c = (q_x + t dx, q_y + t dy,
    q_z + t dz); nearest cell as above, outside the map -> the walk ends; a visited cell that is not the point's own cell, whose entry
    elevation is finite and he - c_z > clear_margin, gets contradicted[cell] += 1 (once per step that lands on it).

Finalise, once per cell, float64, every operation rounded on its own (int64 -> float64 conversions round to nearest even):
  n > 0:   v_m = 256.0 / double(S_w);   z_m = double(z_ref) + (double(S_wz) / double(S_w)) / 16384.0
           h not finite:  h' = z_m, var' = v_m;      else  h' = (h v_m + z_m var) / (var + v_m),  var' = (var v_m) / (var + v_m)
  n == 0 and n_out > 0:  h' = h (its bits are kept), var' = var
  in both cases  var' = fmin(var' + double(outlier_variance) * double(n_out), double(max_variance)); h', var' rounded to fp32 once.
  n == 0 and clear_rays and contradicted >= clear_min_rays:  elevation NaN, variance = initial_variance, every image layer NaN, hits 0
  (this wins over the outlier rule).  Every other cell keeps all its bits."""
import numpy as np

MAX_POINTS = 1 << 22
WQ_SCALE, WQ_CAP = np.float32(256.0), np.float32(4096.0 - 1.0 / 256.0)
ZQ_SCALE, ZQ_RANGE = np.float32(16384.0), np.float32(128.0)
STATS = ("invalid", "near", "high", "ramp", "outside", "gated", "unrepresentable", "inliers")
# anymal_parameters.yaml of the reference's elevation_mapping_cupy configuration; clear_margin / clear_min_rays are this project's
DEFAULTS = dict(sensor_noise_factor=0.05, mahalanobis_thresh=2.0, outlier_variance=0.01, min_valid_distance=0.5, max_height_range=1.0,
                ramped_height_range_a=0.3, ramped_height_range_b=1.0, ramped_height_range_c=0.2, initial_variance=1000.0,
                max_variance=100.0, time_variance=1e-4, max_ray_length=10.0, clear_margin=0.05, clear_min_rays=1)


def params(**kw):
    p = dict(DEFAULTS)
    unknown = set(kw) - set(p)
    assert not unknown, unknown
    p.update(kw)
    return p


def backproject(depth, intrinsics):
    """depth [B,H,W] fp32 metres or uint16 millimetres -> (points [B,H*W,3] fp32, valid [B,H*W] bool): the depth form's points."""
    f = np.float32
    depth = np.asarray(depth)
    B, H, W = depth.shape
    with np.errstate(all="ignore"):
        z = depth.astype(f) / f(1000.0) if depth.dtype == np.uint16 else depth.astype(f)
        valid = np.isfinite(z) & (z != 0)
        K = np.asarray(intrinsics, dtype=f)
        u = np.broadcast_to(np.arange(W, dtype=f)[None, None, :], (B, H, W))
        v = np.broadcast_to(np.arange(H, dtype=f)[None, :, None], (B, H, W))
        x = (u - K[:, 0, 2][:, None, None]) * (z / K[:, 0, 0][:, None, None])
        y = (v - K[:, 1, 2][:, None, None]) * (z / K[:, 1, 1][:, None, None])
    pts = np.stack([x, y, z], -1).astype(f).reshape(B, H * W, 3)
    return pts, valid.reshape(B, H * W)


def classify(points, poses, counts, elevation, variance, center, resolution, z_ref, p, depth_valid=None):
    """The per-point half of the definition -> dict of flat arrays over the B * Pmax slots: "live" (slot holds a point), "cls" (index
    into STATS), "cell" (row-major, -1 when none), "wq", "zq" (int64), "w", "qz" (fp32) and "q", "d" (the map-frame point and t - q)."""
    f = np.float32
    pts = np.asarray(points, dtype=f)
    B, Pmax, _ = pts.shape
    T = np.asarray(poses, dtype=f)
    elev = np.asarray(elevation, dtype=f)
    var = np.asarray(variance, dtype=f)
    N = elev.shape[0]
    cx, cy, r = f(center[0]), f(center[1]), f(resolution)
    live = np.ones((B, Pmax), bool) if counts is None else np.arange(Pmax)[None, :] < np.asarray(counts)[:, None]
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        if depth_valid is not None:
            finite &= depth_valid
        d2 = (x * x + y * y) + z * z
        mind = f(p["min_valid_distance"])
        near = d2 < mind * mind
        q = [((T[:, k, 0][:, None] * x + T[:, k, 1][:, None] * y) + T[:, k, 2][:, None] * z) + T[:, k, 3][:, None] for k in range(3)]
        t = [np.broadcast_to(T[:, k, 3][:, None], (B, Pmax)) for k in range(3)]
        dx, dy, dz = t[0] - q[0], t[1] - q[1], t[2] - q[2]
        L = np.sqrt(dx * dx + dy * dy)
        up = q[2] - t[2]
        high = up > f(p["max_height_range"])
        ramp = up > np.maximum(L - f(p["ramped_height_range_b"]), f(0)) * f(p["ramped_height_range_a"]) + f(p["ramped_height_range_c"])
        inv_r = f(1.0) / r
        hp = f(N) * f(0.5) + f(0.5)
        fi, fj = np.floor((q[0] - cx) * inv_r + hp), np.floor((q[1] - cy) * inv_r + hp)
        inside = (fi >= 0) & (fi < N) & (fj >= 0) & (fj < N)
        cell = np.where(inside, np.where(inside, fi, 0).astype(np.int64) * N + np.where(inside, fj, 0).astype(np.int64), -1)
        h, hv = elev.ravel()[np.maximum(cell, 0)], var.ravel()[np.maximum(cell, 0)]
        gated = np.isfinite(h) & (np.abs(q[2] - h) > f(p["mahalanobis_thresh"]) * np.sqrt(hv))
        v = f(p["sensor_noise_factor"]) * d2
        w = f(1.0) / v
        wqf = np.floor(np.minimum(w, WQ_CAP) * WQ_SCALE)
        rel = q[2] - f(z_ref)
        representable = (np.abs(rel) <= ZQ_RANGE) & (wqf > 0)
        zqf = np.rint(rel * ZQ_SCALE)
    cls = np.full((B, Pmax), 7)
    for k, m in reversed(list(enumerate((~finite, near, high, ramp, ~inside, gated, ~representable)))):
        cls = np.where(m, k, cls)
    ok = cls == 7
    cell = np.where(cls >= 5, cell, -1)
    return {"live": live.ravel(), "cls": cls.ravel(), "cell": cell.ravel(), "wq": np.where(ok, wqf, 0).astype(np.int64).ravel(),
            "zq": np.where(ok, zqf, 0).astype(np.int64).ravel(), "w": w.ravel(), "qz": q[2].ravel(),
            "q": np.stack([a.ravel() for a in q], -1), "d": np.stack([dx.ravel(), dy.ravel(), dz.ravel()], -1), "L": L.ravel()}


def accumulate(points, poses, counts, elevation, variance, center, resolution, z_ref, p, clear_rays=False, depth_valid=None):
    """-> (sums dict of [N,N] integer arrays S_w, S_wz, n, n_out, contradicted; stats dict; the classify() record)."""
    f = np.float32
    slots = int(np.shape(points)[0]) * int(np.shape(points)[1])
    if slots > MAX_POINTS:
        raise ValueError(f"{slots} point slots; at most {MAX_POINTS} per call (the bound of the int64 sums)")
    c = classify(points, poses, counts, elevation, variance, center, resolution, z_ref, p, depth_valid)
    elev = np.asarray(elevation, dtype=f)
    N = elev.shape[0]
    live, cls, cell = c["live"], c["cls"], c["cell"]
    sums = {k: np.zeros(N * N, dtype=np.int64) for k in ("S_w", "S_wz", "n", "n_out", "contradicted")}
    inl = live & (cls == 7)
    np.add.at(sums["S_w"], cell[inl], c["wq"][inl])
    np.add.at(sums["S_wz"], cell[inl], c["wq"][inl] * c["zq"][inl])
    np.add.at(sums["n"], cell[inl], 1)
    np.add.at(sums["n_out"], cell[live & (cls == 5)], 1)
    stats = {name: int((live & (cls == k)).sum()) for k, name in enumerate(STATS)}
    if clear_rays:
        cx, cy, r = f(center[0]), f(center[1]), f(resolution)
        inv_r = f(1.0) / r
        hp = f(N) * f(0.5) + f(0.5)
        walk = live & (cls >= 5)
        q, d, L, own = c["q"][walk], c["d"][walk], c["L"][walk], cell[walk]
        with np.errstate(all="ignore"):
            step = r / L
            nsteps = np.minimum(np.floor(L / r), np.floor(f(p["max_ray_length"]) / r)).astype(np.int64)
            alive = np.ones(own.shape, bool)
            for s in range(1, int(nsteps.max()) + 1 if own.size else 1):
                alive &= s <= nsteps
                if not alive.any():
                    break
                t = f(s) * step
                px, py, pz = q[:, 0] + t * d[:, 0], q[:, 1] + t * d[:, 1], q[:, 2] + t * d[:, 2]
                fi, fj = np.floor((px - cx) * inv_r + hp), np.floor((py - cy) * inv_r + hp)
                alive &= (fi >= 0) & (fi < N) & (fj >= 0) & (fj < N)
                at = np.where(alive, fi, 0).astype(np.int64) * N + np.where(alive, fj, 0).astype(np.int64)
                he = elev.ravel()[at]
                hit = alive & (at != own) & np.isfinite(he) & ((he - pz) > f(p["clear_margin"]))
                np.add.at(sums["contradicted"], at[hit], 1)
    return {k: a.reshape(N, N) for k, a in sums.items()}, stats, c


def finalise(sums, elevation, variance, layers, hits, z_ref, p, clear_rays=False):
    """-> (elevation, variance [N,N] fp32, layers [C,N,N] fp32, hits [N,N] int32); the inputs are not modified."""
    f, d = np.float32, np.float64
    h = np.asarray(elevation, dtype=f)
    var = np.asarray(variance, dtype=f)
    layers = np.array(layers, dtype=f)
    hits = np.array(hits, dtype=np.int32)
    n, n_out = sums["n"], sums["n_out"]
    with np.errstate(all="ignore"):
        Sw, Swz = sums["S_w"].astype(d), sums["S_wz"].astype(d)
        v_m = d(256.0) / Sw
        z_m = d(f(z_ref)) + (Swz / Sw) / d(16384.0)
        h64, var64 = h.astype(d), var.astype(d)
        known = np.isfinite(h)
        h_new = np.where(known, (h64 * v_m + z_m * var64) / (var64 + v_m), z_m)
        var_new = np.where(known, (var64 * v_m) / (var64 + v_m), v_m)
        var_new = np.where(n > 0, var_new, var64)
        var_new = np.fmin(var_new + d(f(p["outlier_variance"])) * n_out.astype(d), d(f(p["max_variance"])))
    touched = (n > 0) | (n_out > 0)
    out_h = np.where(n > 0, h_new.astype(f), h)
    out_var = np.where(touched, var_new.astype(f), var)
    if clear_rays:
        cleared = (n == 0) & (sums["contradicted"] >= int(p["clear_min_rays"]))
        out_h = np.where(cleared, f(np.nan), out_h)
        out_var = np.where(cleared, f(p["initial_variance"]), out_var)
        layers = np.where(cleared[None], f(np.nan), layers)
        hits = np.where(cleared, 0, hits).astype(np.int32)
    return out_h.astype(f), out_var.astype(f), layers.astype(f), hits


def default_z_ref(poses):
    return np.float32(np.asarray(poses, dtype=np.float32)[0, 2, 3])


def add_points(points, poses, elevation, variance, layers, hits, center, resolution, counts=None, z_ref=None, clear_rays=False, p=None,
               depth_valid=None):
    """One callback in the point form -> (elevation, variance, layers, hits, stats, sums)."""
    p = params() if p is None else p
    z_ref = default_z_ref(poses) if z_ref is None else np.float32(z_ref)
    sums, stats, _ = accumulate(points, poses, counts, elevation, variance, center, resolution, z_ref, p, clear_rays, depth_valid)
    return finalise(sums, elevation, variance, layers, hits, z_ref, p, clear_rays) + (stats, sums)


def add_depth(depth, intrinsics, poses, elevation, variance, layers, hits, center, resolution, z_ref=None, clear_rays=False, p=None):
    """One callback in the depth form: the point form on the back-projected pixels, a pixel without a depth counted "invalid"."""
    pts, valid = backproject(depth, intrinsics)
    return add_points(pts, poses, elevation, variance, layers, hits, center, resolution, None, z_ref, clear_rays, p, depth_valid=valid)


def update_variance(elevation, variance, p=None):
    p = params() if p is None else p
    f = np.float32
    var = np.asarray(variance, dtype=f)
    return np.where(np.isfinite(np.asarray(elevation)), np.minimum(var + f(p["time_variance"]), f(p["max_variance"])), var).astype(f)


# ---------------------------------------------------------------------------------------------------- float64 sequential restatement
def kalman_sequential(c, elevation, variance, z_ref, p, order):
    """The exact sequential Kalman update in float64, applied inlier by inlier in ``order`` (indices into the classify() record) with the
    UNQUANTISED weights 1 / v and heights, every point still judged against the entry map -> (h [N,N], var [N,N]) float64 before the
    outlier term; NaN where no inlier fell."""
    N = np.asarray(elevation).shape[0]
    h = np.full(N * N, np.nan)
    var = np.full(N * N, np.nan)
    e0, v0 = np.asarray(elevation, dtype=np.float64).ravel(), np.asarray(variance, dtype=np.float64).ravel()
    for k in order:
        if not (c["live"][k] and c["cls"][k] == 7):
            continue
        cell, z, v = int(c["cell"][k]), float(c["qz"][k]), 1.0 / float(c["w"][k])
        if np.isnan(h[cell]):
            if np.isfinite(e0[cell]):
                h[cell], var[cell] = e0[cell], v0[cell]
            else:
                h[cell], var[cell] = z, v
                continue
        gain = var[cell] / (var[cell] + v)
        h[cell] = h[cell] + gain * (z - h[cell])
        var[cell] = (1.0 - gain) * var[cell]
    return h.reshape(N, N), var.reshape(N, N)
