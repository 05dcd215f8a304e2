"""The case table of the elevation-from-depth tests (tests/test_elevation_host.py, tests/test_gpu_elevation.py): small deterministic
scenes for tests/elevation_ref.py and csrc/elevation.hip.  A case is a dict: "kind" ("points" / "depth"), the source ("points" [B,Pmax,3],
"counts" or None | "depth" [B,H,W] fp32 or uint16, "intrinsics" [B,4,4]), "poses" [B,4,4], the map on entry ("elevation", "variance",
"layers" [C,N,N], "hits"), "center", "resolution", "N", "z_ref" (None: sensor 0's t_z), "clear_rays", "params" (overrides of
elevation_ref.DEFAULTS) and "has_inliers" (False for the cases built so that no point is accumulated)."""
import functools

import numpy as np

import elevation_ref as E
from grid_map_cases import look_at

NAN = np.float32(np.nan)
RES = {8: 0.5, 33: 0.1, 200: 0.04}            # N -> resolution: maps of 4 m, 3.3 m and the reference's 8 m
SHAPE_N, SHAPE_P = (8, 33, 200), (1, 63, 64, 65, 1000)
DEPTH_SHAPES = ((8, 8), (17, 31), (64, 48))   # H, W


def prior(rng, N, known=0.5, var=(0.005, 0.05), C=2):
    """A bumpy ground known on a random part of the map, with image layers and hits on the known cells."""
    elev = rng.uniform(-0.03, 0.03, (N, N)).astype(np.float32)
    mask = rng.uniform(size=(N, N)) < known
    elev[~mask] = NAN
    variance = np.where(mask, rng.uniform(var[0], var[1], (N, N)), 1000.0).astype(np.float32)
    layers = np.where(mask[None], rng.uniform(0, 1, (C, N, N)), NAN).astype(np.float32)
    hits = np.where(mask, rng.integers(1, 5, (N, N)), 0).astype(np.int32)
    return elev, variance, layers, hits


def blank(N, C=2):
    return (np.full((N, N), NAN, np.float32), np.full((N, N), 1000.0, np.float32), np.full((C, N, N), NAN, np.float32),
            np.zeros((N, N), np.int32))


def sensor_pose(rng, xyz):
    """A LiDAR-like pose: yaw anywhere, a few degrees of roll and pitch."""
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)
    cz, sz, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ \
        np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, xyz
    return T.astype(np.float32)


def to_sensor(T, q):
    """Map-frame points -> the sensor frame of pose T (float64 inverse, rounded to fp32: the sensor's data)."""
    T = T.astype(np.float64)
    return ((q - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


def ground_points(rng, T, P, half, center, spread=1.15, height=0.0, noise=0.02):
    """P points on the ground (z = height + noise) spread over a little more than the map, in the sensor frame of T."""
    q = np.stack([center[0] + rng.uniform(-half, half, P) * spread, center[1] + rng.uniform(-half, half, P) * spread,
                  height + rng.normal(0, noise, P)], -1)
    return to_sensor(T, q)


def _case(name, kind, N, center, state, poses, z_ref=None, clear_rays=False, params=None, has_inliers=True, **source):
    elev, variance, layers, hits = state
    c = {"name": name, "kind": kind, "N": N, "resolution": RES[N], "center": center, "elevation": elev, "variance": variance,
         "layers": layers, "hits": hits, "poses": np.stack(poses).astype(np.float32), "z_ref": z_ref, "clear_rays": clear_rays,
         "params": dict(params or {}), "counts": None, "has_inliers": has_inliers}
    c.update(source)
    return c


def depth_of_ground(rng, T, K, H, W, dtype, holes=True):
    """The depth image a camera of pose T sees of the plane z = 0 (+ 1 cm noise), 0 where the ray misses it; ``holes`` sprinkles the
    values that are no point (fp32: 0, NaN, inf, -inf; uint16: 0)."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1) @ T[:3, :3].astype(np.float64).T
    with np.errstate(all="ignore"):
        z = np.where(d[..., 2] < -1e-3, -float(T[2, 3]) / d[..., 2], 0.0)
    z = np.where(z > 0, z + rng.normal(0, 0.01, z.shape), 0.0)
    if dtype == np.uint16:
        out = np.clip(np.rint(z * 1000.0), 0, 65535).astype(np.uint16)
        if holes:
            out.ravel()[rng.choice(H * W, max(H * W // 16, 1), replace=False)] = 0
        return out
    out = z.astype(np.float32)
    if holes:
        idx = rng.choice(H * W, max(H * W // 8, 4), replace=False)
        out.ravel()[idx] = np.resize(np.float32([0.0, np.nan, np.inf, -np.inf]), idx.size)
    return out


def pinhole(f, H, W):
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = f, f, W / 2 - 0.5, H / 2 - 0.25
    return K


@functools.lru_cache(maxsize=None)
def cases():
    out = {}

    def add(c):
        assert c["name"] not in out
        out[c["name"]] = c

    # ---- shapes: every N with every P; two sensors, the second one padded to Pmax with counts
    # (P = 1024 and 1025 at N = 33: two sensors fill two workgroups' 1024 point slots each exactly, and spill two slots into a third)
    for N in SHAPE_N:
        for P in SHAPE_P + ((1024, 1025) if N == 33 else ()):
            rng = np.random.default_rng(1000 * N + P)
            center = (1.5, -2.25)
            half = N * RES[N] / 2
            poses = [sensor_pose(rng, (center[0] + 0.1, center[1] - 0.2, 0.62)), sensor_pose(rng, (center[0] - 0.3, center[1] + 0.1, 0.55))]
            pts = np.stack([ground_points(rng, T, P, half, center) for T in poses])
            counts = np.array([P, max(P - 3, 0)], np.int32)
            pts[1, counts[1]:] = 7.0           # padding: never read as points
            add(_case(f"shape_n{N}_p{P}", "points", N, center, prior(rng, N), poses, points=pts, counts=counts,
                      has_inliers=(N, P) != (33, 1)))       # (that single point falls outside the map)

    # ---- depth images, both encodings; two cameras that look down at the ground from either side, holes included
    for H, W in DEPTH_SHAPES:
        for dtype, tag in ((np.float32, "f32"), (np.uint16, "u16")):
            rng = np.random.default_rng(H * 100 + W + (dtype == np.uint16))
            N, center = 33, (0.4, 0.2)
            poses = [look_at((center[0] - 1.0, center[1] - 0.1, 1.1), (center[0] + 0.4, center[1], 0.0)),
                     look_at((center[0] + 0.9, center[1] + 0.6, 0.9), (center[0] - 0.3, center[1] - 0.2, 0.0))]
            K = [pinhole(0.9 * W, H, W), pinhole(0.7 * W, H, W)]
            depth = np.stack([depth_of_ground(rng, T, k, H, W, dtype) for T, k in zip(poses, K)])
            add(_case(f"depth_{H}x{W}_{tag}", "depth", N, center, prior(rng, N, known=0.6), poses, depth=depth, intrinsics=np.stack(K),
                      params=dict(max_height_range=2.0)))

    # ---- contention: 65 536 points in ONE cell at the largest weight (w >= 4096 - 1/256: d2 <= 1 / 204.8) and the largest |zq| = 2^21
    # (q_z - z_ref = +-128 exactly: q_z = -2^-5, z_ref = -2^-5 -+ 128, both fp32 numbers)
    for sign, state_name in ((1, "unknown"), (-1, "known")):
        N, center = 8, (0.0, 0.0)
        P = 65536
        rng = np.random.default_rng(65536 + sign)
        pts = np.empty((1, P, 3), np.float32)
        pts[0, :, 0], pts[0, :, 1], pts[0, :, 2] = rng.uniform(0.01, 0.04, P), rng.uniform(0.01, 0.04, P), -0.03125
        state = blank(N)
        if state_name == "known":
            state[0][4, 4], state[1][4, 4] = -0.03, 0.02
        add(_case(f"contention_{state_name}", "points", N, center, state, [np.eye(4, dtype=np.float32)], points=pts,
                  z_ref=np.float32(-0.03125 - sign * 128.0), params=dict(min_valid_distance=0.0)))

    # ---- rejection: every class, cell borders and the map's edge (N = 8, r = 0.5, centre 0: cell i covers [-2.25 + i/2, -1.75 + i/2))
    N, center = 8, (0.0, 0.0)
    T = np.eye(4, dtype=np.float32)
    T[2, 3] = 0.5
    below = np.float32(np.nextafter(np.float32(-2.25), np.float32(-3)))
    rows = [
        (np.nan, 1.0, -0.5), (1.0, np.inf, -0.5), (1.0, 1.0, -np.inf),                      # invalid
        (0.0, 0.0, 0.0), (0.2, 0.2, -0.3),                                                    # near (|p| < 0.5)
        (1.0, 0.0, 1.01), (0.0, 1.5, 3.0),                                                    # high (> 1.0 above the sensor)
        (0.6, 0.0, 0.21), (2.0, 0.0, 0.51), (0.0, -1.2, 0.3),                                 # ramp (0.2 up to 1 m, then 0.3 per metre)
        (1.5, 0.0, 0.34), (0.6, 0.0, 0.19),                                                   # ... just under the ramp: inliers
        (below, 0.0, -0.5), (1.75, 0.0, -0.5), (0.0, 1.75, -0.5), (0.0, -2.26, -0.5), (30.0, 0.0, -0.5),   # outside
        (-2.25, 0.0, -0.5), (0.0, -2.25, -0.5),                                               # on the map's lower edge: inside
        (1.7499999, 0.0, -0.5),                            # one ulp inside the upper edge: the fp32 cell coordinate rounds to 8.0, outside
        (-0.25, 0.75, -0.5), (0.25, -0.75, -0.5), (-1.75, -1.75, -0.5), (1.25, 1.25, -0.5),   # exactly on cell borders
        (1.0, 1.0, -0.5), (1.0, 1.05, -0.45), (1.0, 1.1, 0.2),                                # a known cell: two inliers, one gated
        (-1.0, -1.0, 0.1), (-1.0, -1.1, -1.2),                                                # a known cell that only gets outliers
        (0.9, -1.0, -0.5),                                                                    # |q_z - z_ref| > 128 with the z_ref below
    ]
    state = blank(N)
    for i, j, h, v in ((6, 6, 0.02, 0.01), (2, 2, -0.4, 0.0025)):
        state[0][i, j], state[1][i, j] = h, v
    add(_case("rejection_classes", "points", N, center, state, [T], points=np.float32(rows)[None]))
    add(_case("rejection_unrepresentable", "points", N, center, state, [T], points=np.float32(rows)[None], z_ref=np.float32(200.0), has_inliers=False))
    far = np.float32([[80.0, 0.0, -0.5], [79.0, 1.0, -0.5], [81.0, -1.0, -0.5]])              # w < 1/256 beyond ~71.6 m: weight 0
    Tfar = np.eye(4, dtype=np.float32)
    Tfar[:3, 3] = (-80.0, 0.0, 0.5)
    add(_case("rejection_zero_weight", "points", N, center, blank(N), [Tfar], points=far[None],
              params=dict(max_height_range=100.0, ramped_height_range_c=100.0), has_inliers=False))

    # ---- gate: small prior variances, so that a share of the points is gated; some cells receive only outliers
    rng = np.random.default_rng(77)
    N, center = 33, (0.0, 0.0)
    poses = [sensor_pose(rng, (0.2, 0.1, 0.6))]
    pts = ground_points(rng, poses[0], 3000, N * RES[N] / 2, center, noise=0.05)[None]
    state = prior(rng, N, known=0.7, var=(1e-5, 2e-3))
    add(_case("gate", "points", N, center, state, poses, points=pts))

    # ---- order: three sensors with clouds of their own (the tests permute points and sensors)
    rng = np.random.default_rng(5)
    poses = [sensor_pose(rng, (0.3 * k - 0.3, 0.2 - 0.2 * k, 0.5 + 0.1 * k)) for k in range(3)]
    pts = np.stack([ground_points(rng, T, 700, N * RES[N] / 2, center) for T in poses])
    add(_case("order", "points", N, center, prior(rng, N), poses, points=pts, clear_rays=True))

    # ---- ray clearing: flat known ground; a wall (0.45 high) at row 20 that the rays to the ground behind it cross, and a wall at row
    # 26 whose top is hit by inliers.  The sensor stands at row ~6, 0.6 above the ground.
    def walls(clear_rays):
        rng = np.random.default_rng(9)
        N, center = 33, (0.0, 0.0)
        r = RES[N]
        elev = np.zeros((N, N), np.float32)
        elev[20, 8:25] = 0.45
        elev[26, 8:25] = 0.45
        variance = np.full((N, N), 0.01, np.float32)
        layers = rng.uniform(0, 1, (2, N, N)).astype(np.float32)
        hits = rng.integers(1, 4, (N, N)).astype(np.int32)
        T = sensor_pose(rng, ((6 - N / 2) * r, 0.0, 0.6))
        jj = np.arange(10, 23)
        behind = np.array([[(i - N / 2) * r, (j - N / 2) * r, 0.0] for i in (22, 23, 24, 28, 29) for j in jj])   # ground behind the walls
        top = np.array([[(26 - N / 2) * r, (j - N / 2) * r, 0.45] for j in jj])                              # the far wall's top
        q = np.concatenate([behind, top]) + rng.normal(0, 0.003, (len(behind) + len(top), 3))
        return _case(f"walls_clear_{int(clear_rays)}", "points", N, center, (elev, variance, layers, hits), [T],
                     points=to_sensor(T, q)[None], clear_rays=clear_rays, params=dict(clear_min_rays=2))

    add(walls(True))
    add(walls(False))
    # the same through depth images, with clearing
    rng = np.random.default_rng(11)
    H, W = 17, 31
    poses = [look_at((-1.0, 0.0, 1.0), (0.5, 0.0, 0.0))]
    K = [pinhole(0.8 * W, H, W)]
    state = prior(rng, N, known=0.8)
    state[0][np.isfinite(state[0]) & (rng.uniform(size=(N, N)) < 0.3)] = 0.5     # clutter the rays see through
    add(_case("depth_clear", "depth", N, center, state, poses, depth=np.stack([depth_of_ground(rng, poses[0], K[0], H, W, np.float32)]),
              intrinsics=np.stack(K), clear_rays=True, params=dict(max_height_range=2.0)))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """elevation_ref on a case, computed once -> (elevation, variance, layers, hits, stats, sums)."""
    c = cases()[name]
    p = E.params(**c["params"])
    kw = dict(z_ref=c["z_ref"], clear_rays=c["clear_rays"], p=p)
    if c["kind"] == "depth":
        return E.add_depth(c["depth"], c["intrinsics"], c["poses"], c["elevation"], c["variance"], c["layers"], c["hits"], c["center"],
                           c["resolution"], **kw)
    return E.add_points(c["points"], c["poses"], c["elevation"], c["variance"], c["layers"], c["hits"], c["center"], c["resolution"],
                        counts=c["counts"], **kw)
