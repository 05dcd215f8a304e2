"""The case tables of the grid-map tests (tests/test_grid_map_host.py, tests/test_gpu_grid_map.py).  Everything is seeded and fixed; the
shapes are the smallest at which each kernel can go wrong: N = 16 and 33 (one and several 8 x 8 tiles, the second with a ragged edge),
one production-sized map, a non-square 24 x 40 image."""
import math

import numpy as np

IMG = (24, 40)   # H, W
NAN = np.float32(np.nan)


def intrinsics(fx, fy, H=IMG[0], W=IMG[1]):
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, W / 2, H / 2
    return K


def look_at(position, target, up=(0.0, 0.0, 1.0)):
    """pose_cam_in_world [4,4] of a camera at ``position`` whose z axis points at ``target`` (x right, y down)."""
    p, t, u = (np.asarray(v, dtype=np.float64) for v in (position, target, up))
    z = (t - p) / np.linalg.norm(t - p)
    if abs(z @ u) > 0.999:
        u = np.array([1.0, 0.0, 0.0])
    x = np.cross(z, u)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, p
    return T.astype(np.float32)


def cell_xy(N, r, center, i, j):
    return center[0] + (i - N / 2) * r, center[1] + (j - N / 2) * r


def image(rng, C, nan_blocks=False):
    m = rng.uniform(0.0, 1.0, (C,) + IMG).astype(np.float32)
    if nan_blocks:
        m[:, 4:9, 10:22] = NAN          # every channel: the camera is skipped there
        m[0, 14:20, 3:12] = NAN         # one channel only: the others are still fused
    return m


def _case(name, N, r, center, elev, maps, K, poses, layers=None, hits=None, **params):
    C = maps.shape[1]
    if layers is None:
        layers = np.full((C, N, N), NAN, dtype=np.float32)
    if hits is None:
        hits = np.zeros((N, N), dtype=np.int32)
    return {"name": name, "N": N, "resolution": r, "center": center, "elevation": elev.astype(np.float32), "maps": maps,
            "intrinsics": np.stack(K), "poses": np.stack(poses), "layers": layers.astype(np.float32), "hits": hits, "params": params}


def _ground(rng, N, bumps=0.02):
    return (rng.uniform(-bumps, bumps, (N, N))).astype(np.float32)


def fusion_cases():
    """{name: case}.  ``params`` are the keyword arguments of the fusion (alpha, min_depth, max_range, occlusion_margin) that differ from
    the defaults."""
    out = {}

    def add(c):
        out[c["name"]] = c

    rng = np.random.default_rng(20)
    # one tile, one camera, one channel
    N, r, ctr = 16, 0.1, (0.3, -0.2)
    add(_case("n16_one_camera", N, r, ctr, _ground(rng, N), image(rng, 1)[None], [intrinsics(18, 18)],
              [look_at((ctr[0] - 0.63, ctr[1] + 0.07, 0.55), (ctr[0] + 0.4, ctr[1], 0.0))]))
    # all-NaN elevation: nothing may be written
    add(_case("all_nan_elevation", N, r, ctr, np.full((N, N), NAN), image(rng, 2)[None], [intrinsics(18, 18)],
              [look_at((ctr[0] - 0.63, ctr[1] + 0.07, 0.55), (ctr[0] + 0.4, ctr[1], 0.0))]))
    # two cameras that both see the middle of the map, a first touch against existing values (half the target cells hold a value)
    N, r, ctr = 33, 0.1, (-1.0, 2.0)
    elev = _ground(rng, N)
    elev[rng.uniform(size=(N, N)) < 0.05] = NAN
    maps = np.stack([image(rng, 2), image(rng, 2)])
    poses = [look_at((ctr[0] - 1.21, ctr[1] - 0.33, 0.8), (ctr[0] + 0.3, ctr[1], 0.0)),
             look_at((ctr[0] + 0.17, ctr[1] + 1.42, 0.7), (ctr[0], ctr[1] - 0.2, 0.0))]
    Ks = [intrinsics(16, 16), intrinsics(14, 15)]
    layers = rng.uniform(0, 1, (2, N, N)).astype(np.float32)
    layers[:, rng.uniform(size=(N, N)) < 0.5] = NAN
    hits = rng.integers(0, 5, (N, N)).astype(np.int32)
    add(_case("n33_two_cameras", N, r, ctr, elev, maps, Ks, poses, layers, hits, alpha=0.3))
    add(_case("n33_two_cameras_swapped", N, r, ctr, elev, maps[::-1].copy(), Ks[::-1], poses[::-1], layers, hits, alpha=0.3))
    # a camera looking away from the map (every cell behind it) and one below the surface looking up
    add(_case("behind_and_below", N, r, ctr, _ground(rng, N), np.stack([image(rng, 1), image(rng, 1)]), [intrinsics(16, 16)] * 2,
              [look_at((ctr[0] - 1.7, ctr[1], 0.5), (ctr[0] - 3.0, ctr[1], 0.3)),
               look_at((ctr[0] - 0.52, ctr[1] + 0.11, -0.5), (ctr[0] + 0.5, ctr[1], 0.0))]))
    # straight down from above a cell centre: the cell underneath has L < r (no step), and the rays of its row, its column and its
    # diagonals run along the axes and the diagonals; four posts make those rays matter
    elev = _ground(rng, N, 0.0)
    for (pi, pj) in ((16, 22), (10, 16), (21, 21), (12, 20), (16, 9)):
        elev[pi, pj] = 0.9
    cam = cell_xy(N, r, ctr, 16, 16)
    add(_case("straight_down_axes_diagonals", N, r, ctr, elev, image(rng, 1)[None], [intrinsics(5, 5)],
              [look_at((cam[0], cam[1], 1.3), (cam[0], cam[1], 0.0))]))
    # a wall that hides the cells behind it (and not the ones in front or beside)
    elev = _ground(rng, N)
    elev[20, 5:28] = 1.0
    add(_case("wall", N, r, ctr, elev, image(rng, 2)[None], [intrinsics(14, 14)],
              [look_at((ctr[0] - 1.13, ctr[1] + 0.04, 0.6), (ctr[0] + 1.0, ctr[1], 0.0))]))
    # a wall on the map edge, seen from a camera outside the footprint behind it: the walk crosses the wall row, then leaves the map
    elev = _ground(rng, N)
    elev[0, :] = 1.2
    elev[:, N - 1] = 1.2
    add(_case("wall_on_edge_camera_outside", N, r, ctr, elev, np.stack([image(rng, 1), image(rng, 1)]), [intrinsics(15, 15)] * 2,
              [look_at((ctr[0] - 2.6, ctr[1] + 0.23, 0.9), (ctr[0], ctr[1], 0.0)),
               look_at((ctr[0] + 0.31, ctr[1] + 2.9, 2.5), (ctr[0], ctr[1], 0.0))]))
    # NaN pixels
    add(_case("nan_pixels", N, r, ctr, _ground(rng, N), image(rng, 3, nan_blocks=True)[None], [intrinsics(12, 12)],
              [look_at((ctr[0] - 1.3, ctr[1] - 0.21, 1.0), (ctr[0] + 0.2, ctr[1], 0.0))]))
    # max_range, from a camera above a cell centre: L^2 / r^2 is an integer there and the range sits between two of them
    cam = cell_xy(N, r, ctr, 12, 15)
    add(_case("max_range", N, r, ctr, _ground(rng, N, 0.0), image(rng, 1)[None], [intrinsics(5, 5)],
              [look_at((cam[0], cam[1], 1.5), (cam[0], cam[1], 0.0))], max_range=r * math.sqrt(40.5)))
    # C = 4, B = 3
    add(_case("four_channels_three_cameras", N, r, ctr, _ground(rng, N), np.stack([image(rng, 4) for _ in range(3)]),
              [intrinsics(16, 16), intrinsics(13, 13), intrinsics(10, 12)],
              [look_at((ctr[0] - 1.21, ctr[1] - 0.33, 0.8), (ctr[0] + 0.3, ctr[1], 0.0)),
               look_at((ctr[0] + 0.17, ctr[1] + 1.42, 0.7), (ctr[0], ctr[1] - 0.2, 0.0)),
               look_at((ctr[0] + 0.9, ctr[1] - 1.1, 1.1), (ctr[0], ctr[1], 0.0))], min_depth=0.4, occlusion_margin=0.02))
    # the production map: 8 m at 0.04 m, rolling ground, a wall and a block, two cameras
    N, r, ctr = 200, 0.04, (12.0, -7.0)
    i, j = np.mgrid[0:N, 0:N]
    elev = (0.1 * np.sin(i / 23.0) * np.cos(j / 31.0)).astype(np.float32) + _ground(rng, N, 0.005)
    elev[130, 40:160] = 0.8
    elev[60:70, 150:165] = 0.5
    elev[rng.uniform(size=(N, N)) < 0.02] = NAN
    add(_case("n200_production", N, r, ctr, elev, np.stack([image(rng, 2), image(rng, 2, nan_blocks=True)]),
              [intrinsics(15, 15), intrinsics(12, 12)],
              [look_at((ctr[0] - 0.4, ctr[1] + 0.013, 0.7), (ctr[0] + 2.0, ctr[1], 0.0)),
               look_at((ctr[0] - 0.3, ctr[1] - 0.3, 0.75), (ctr[0] + 1.0, ctr[1] + 1.8, 0.0))]))
    return out


# --------------------------------------------------------------------------------------------------------------------------- sdf
SDF_SIZES = (1, 2, 7, 31, 64, 65, 200, 512)


def sdf_layers(N):
    """{name: fp32 [N,N] layer}; the obstacle set is value < 0.5."""
    rng = np.random.default_rng(1000 + N)
    free, obst = np.float32(0.9), np.float32(0.1)
    out = {"empty": np.full((N, N), free), "full": np.full((N, N), obst)}
    for name, (ci, cj) in (("corner00", (0, 0)), ("corner0n", (0, N - 1)), ("cornern0", (N - 1, 0)), ("cornernn", (N - 1, N - 1))):
        a = np.full((N, N), free)
        a[ci, cj] = obst
        out[name] = a
    i, j = np.mgrid[0:N, 0:N]
    out["checkerboard"] = np.where((i + j) % 2 == 0, obst, free).astype(np.float32)
    a = np.full((N, N), free)
    a[N // 3, :] = obst
    out["one_row"] = a
    for name, p in (("random01", 0.01), ("random50", 0.5), ("random99", 0.99)):
        out[name] = np.where(rng.uniform(size=(N, N)) < p, obst, free).astype(np.float32)
    a = rng.uniform(0, 1, (N, N)).astype(np.float32)        # values on both sides of the threshold, NaN cells present
    a[rng.uniform(size=(N, N)) < 0.2] = NAN
    out["values_with_nan"] = a
    a = np.full((N, N), NAN)                                # only unknown cells and one known one
    a[N // 2, N // 2] = free
    out["nan_but_one"] = a
    return out


def sdf_cases():
    """[(N, layer name, unknown)]: every layer at the small sizes with the default mode, the NaN layers with all three modes at every size,
    and at the two largest sizes only the layers whose reference is cheap to state once."""
    cases = []
    for N in SDF_SIZES:
        names = list(sdf_layers(N)) if N <= 65 else ["empty", "full", "cornernn", "one_row", "random01", "random50", "values_with_nan"]
        for name in names:
            modes = ("obstacle", "free", "neither") if name in ("values_with_nan", "nan_but_one") else ("obstacle",)
            cases += [(N, name, m) for m in modes]
    return cases


# ------------------------------------------------------------------------------------------------------------------------ carrot
YAWS = (0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, 0.3, -0.3, 1.0, 2.0, -2.5, 3.0, math.pi / 4, -3 * math.pi / 4,
        # int() truncates toward zero: N/2 + sin(yaw) * 30 sits just below and just above a whole number around these two
        math.asin(0.1) - 1e-9, math.asin(0.1) + 1e-9, math.pi / 2 + 1e-7)
DEFAULT_DISCS = ((30, 15), (55, 20), (90, 25))   # smart_carrot.py:74-85, for its 200-cell map
SCALED_DISCS = ((10, 5), (18, 6), (28, 8))   # the reference's pattern at about a third: a 64-cell map
FACTORS = ((0.0, 0.0), (0.7, 0.0), (0.0, 0.05), (0.7, 0.05))


def carrot_field(N, seed=0):
    """A smooth sdf-like field plus seeded exponential noise (the gap between the two largest draws of an exponential does not shrink with
    the number of cells: the best and the second-best score stay far apart in units of fp32 rounding), and an elevation layer with NaN cells at the border and a
    few inside."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:N, 0:N]
    s = (0.5 * np.sin(i / (N / 9.0)) * np.cos(j / (N / 7.0)) + rng.exponential(0.3, (N, N))).astype(np.float32)
    elev = rng.uniform(-0.05, 0.05, (N, N)).astype(np.float32)
    elev[0, :] = NAN
    elev[:, N - 1] = NAN
    elev[N - 1, N // 2] = NAN
    elev[rng.uniform(size=(N, N)) < 0.01] = NAN
    return s, elev


def carrot_cases():
    """[(name, dict(sdf, elevation, yaw, center, resolution, distance_force_factor, center_force_factor, discs))]."""
    out = []
    for N, discs, res in ((200, DEFAULT_DISCS, 0.04), (64, SCALED_DISCS, 0.125)):
        s, elev = carrot_field(N, seed=N)
        for k, yaw in enumerate(YAWS):
            dff, cff = FACTORS[k % 4]
            out.append((f"n{N}_yaw{k}", dict(sdf=s, elevation=elev, yaw=yaw, center=(3.0, -1.5), resolution=res,
                                            distance_force_factor=dff, center_force_factor=cff, discs=discs)))
        for dff, cff in FACTORS:
            out.append((f"n{N}_factors_{dff}_{cff}", dict(sdf=s, elevation=elev, yaw=0.8, center=(0.0, 0.0), resolution=res,
                                                         distance_force_factor=dff, center_force_factor=cff, discs=discs)))
        flat = np.full((N, N), np.float32(2.0))
        clean = np.zeros((N, N), dtype=np.float32)
        out.append((f"n{N}_constant_first_index_wins", dict(sdf=flat, elevation=clean, yaw=0.4, center=(1.0, 1.0), resolution=res,
                                                           distance_force_factor=0.0, center_force_factor=0.0, discs=discs)))
        steps = np.minimum(np.floor(s * 4), 1.0).astype(np.float32)       # integer-valued scores, capped: many exact ties at the top
        out.append((f"n{N}_integer_ties", dict(sdf=steps, elevation=clean, yaw=-1.2, center=(1.0, 1.0), resolution=res,
                                              distance_force_factor=0.0, center_force_factor=0.0, discs=discs)))
        out.append((f"n{N}_all_masked", dict(sdf=s, elevation=np.full((N, N), NAN), yaw=0.4, center=(1.0, 1.0), resolution=res,
                                            distance_force_factor=0.7, center_force_factor=0.05, discs=discs)))
        holes = s.copy()
        holes[np.random.default_rng(5).uniform(size=(N, N)) < 0.3] = NAN
        holes[pattern_peak(N, 0.0, discs)] = NAN         # the unmasked maximum itself is NaN
        out.append((f"n{N}_nan_scores", dict(sdf=holes, elevation=clean, yaw=0.0, center=(1.0, 1.0), resolution=res,
                                            distance_force_factor=0.0, center_force_factor=0.05, discs=discs)))
        border = clean.copy()                            # NaN elevation on the whole border: the 3 x 3 window leaves the grid there
        border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = NAN
        out.append((f"n{N}_nan_border", dict(sdf=s, elevation=border, yaw=math.pi, center=(1.0, 1.0), resolution=res,
                                            distance_force_factor=0.7, center_force_factor=0.0, discs=discs)))
    return out


def pattern_peak(N, yaw, discs):
    import grid_map_ref as G

    s, _ = carrot_field(N, seed=N)
    keep = G.pattern(N, yaw, discs)
    masked = np.where(keep, s, -np.inf)
    return np.unravel_index(int(masked.argmax()), masked.shape)
