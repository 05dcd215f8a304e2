"""Inputs shared by tests/test_supervision_host.py and tests/test_gpu_supervision_edges.py: the case table of the supervision rasteriser
(csrc/supervision.hip), seeded and built with numpy.  A case is one polygon in one camera on one frame shape; the host file holds the
coverage claims made here on the CPU oracle (oracle/supervision.py), so the GPU file can rely on them.

Polygons "in pixel coordinates" go through the identity camera (K = pose = eye(4), points (x, y, 1)): in fp32 that projection is exact
(u = x, v = y, s = 1 / (1 + 1e-8) = 1), which the host file asserts.

Frame shapes (C, H, W) and what each is for -- the kernel is one 256-thread workgroup per node, four waves of 64 lanes:
  (1, 257, 65)   one row past the 256-thread block (second trip of the scan loop), one column past a 64-lane wave (second trip of the fill)
  (2, 300, 500)  non-square, W not a multiple of 64
  (3, 448, 448)  production
  (1, 513, 40)   third trip of the scan loop, W < 64 (lanes 40 .. 63 idle)
  (1, 1, 1)      smallest frame
  (1, 4, 40)     small frame for the extreme-coordinate cases"""
import math
from collections import namedtuple

import numpy as np

f32 = np.float32
VALUE = 0.65                    # colour * traversability of the merge; the mixed start mask holds values on both sides of it
LDS_MAX_H = 448
LDS_MAX_N = 8191 - LDS_MAX_H    # 7743: the most points the launcher accepts at 448 rows ([H] + [H] + 2 [N + 1] floats in 64 KB)

# expect: None, or the hand-stated closed pixel rectangle (x0, y0, x1, y1) of the fill, or "empty"
Case = namedtuple("Case", "name family shape K pose points expect conditions")

S_TALL, S_WIDE, S_PROD, S_TALL3, S_ONE, S_TINY = (1, 257, 65), (2, 300, 500), (3, 448, 448), (1, 513, 40), (1, 1, 1), (1, 4, 40)
SHAPES = (S_TALL, S_WIDE, S_PROD, S_TALL3, S_ONE, S_TINY)
EYE = np.eye(4, dtype=f32)


def pixel_points(xy):
    """[N,2] pixel coordinates -> [N,3] fp32 world points the identity camera projects onto them."""
    xy = np.asarray(xy, dtype=f32).reshape(-1, 2)
    return np.concatenate([xy, np.ones((len(xy), 1), dtype=f32)], axis=1)


def _pixel_case(name, family, shape, xy, expect=None, conditions=()):
    return Case(name, family, shape, EYE, EYE, pixel_points(xy), expect, tuple(conditions))


# ---------------------------------------------------------------------------------------------------------- integer rectangles
RECTANGLES = {
    S_WIDE: ((-5, -5, 40, 30), (460, 280, 520, 320), (0, 0, 499, 299), (-1, 10, -1, 20), (500, 10, 600, 20), (10, 299, 20, 400),
             (63, 255, 64, 256)),
    S_ONE: ((0, 0, 0, 0),),
    # straddling row 256 (the scan loop's second trip) and column 64 (the fill's second trip); the last row and column alone
    S_TALL: ((60, 250, 70, 260), (63, 255, 64, 256), (0, 256, 64, 256), (64, 0, 64, 256), (3, 200, 61, 257)),
    # straddling row 512 (third trip) and rows 255 / 256; the whole frame
    S_TALL3: ((5, 510, 30, 520), (0, 512, 39, 512), (10, 250, 20, 513), (0, 0, 39, 512)),
}


def clipped_rectangle(rect, H, W):
    """The closed rectangle clipped to the frame, or "empty"."""
    x0, y0, x1, y1 = rect
    a, b, c, d = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    return (a, b, c, d) if a <= c and b <= d else "empty"


def rectangle_mask(expect, H, W):
    m = np.zeros((H, W), dtype=bool)
    if expect != "empty":
        x0, y0, x1, y1 = expect
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def rectangle_cases():
    """Every rectangle from each of its four start vertices, in both orientations."""
    out = []
    for shape, rects in RECTANGLES.items():
        _, H, W = shape
        for (x0, y0, x1, y1) in rects:
            ring = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
            for start in range(4):
                for rev in (False, True):
                    v = ring[start:] + ring[:start]
                    if rev:
                        v = v[:1] + v[:0:-1]
                    name = f"rect_{H}x{W}_{x0}_{y0}_{x1}_{y1}_s{start}{'r' if rev else 'f'}"
                    out.append(_pixel_case(name, "rectangle", shape, v, clipped_rectangle((x0, y0, x1, y1), H, W)))
    return out


# ---------------------------------------------------------------------------------------------------------- ellipse polygons
ELLIPSE_SHAPES = (S_PROD, S_WIDE, S_TALL)
ELLIPSES_PER_SHAPE = 12


def ellipse_polygons(H, W, count=ELLIPSES_PER_SHAPE):
    """Convex polygons with 3 .. 8 vertices on random ellipses, many of them cut by a border; every third one reversed."""
    rng = np.random.default_rng(1000 + H)
    polys = []
    for t in range(count):
        n = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        a = rng.uniform(10, 0.6 * W)
        b = rng.uniform(10, 0.6 * H)
        c = np.array([rng.uniform(-0.3 * W, 1.3 * W), rng.uniform(-0.3 * H, 1.3 * H)])
        poly = (c + np.stack([a * np.cos(ang), b * np.sin(ang)], 1)).astype(f32)
        if t % 3 == 0:
            poly = poly[::-1].copy()
        polys.append(poly)
    return polys


def ellipse_cases():
    return [_pixel_case(f"ellipse_{shape[1]}x{shape[2]}_{t}", "ellipse", shape, poly)
            for shape in ELLIPSE_SHAPES for t, poly in enumerate(ellipse_polygons(shape[1], shape[2]))]


# ---------------------------------------------------------------------------------------------------------- degenerate polygons
QUAD = ((30.5, 40.5), (120.25, 50.0), (110.0, 140.75), (25.0, 120.0))
ONE_PIXEL = (17, 23)


def degenerate_cases():
    s = S_WIDE
    nan = float("nan")
    behind = pixel_points(QUAD)
    behind[:, 2] = -1.0
    return [
        _pixel_case("segment_n2", "degenerate", s, ((10.5, 20.25), (200.75, 130.5))),                     # the minimum N
        _pixel_case("quad_open", "degenerate", s, QUAD),                                                  # first vertex appended
        _pixel_case("quad_closed", "degenerate", s, QUAD + QUAD[:1]),                                     # closed: nothing appended
        _pixel_case("one_pixel", "degenerate", s, (ONE_PIXEL,) * 4, ONE_PIXEL + ONE_PIXEL),
        _pixel_case("collinear", "degenerate", s, ((10, 10), (50, 50), (90, 90))),
        _pixel_case("duplicates", "degenerate", s, ((30, 30), (30, 30), (200, 40), (200, 40), (100, 200), (100, 200))),
        _pixel_case("nan_vertex", "degenerate", s, ((40, 40), (nan, 100), (200, 60), (150, 200))),
        Case("all_behind", "degenerate", s, EYE, EYE, behind, "empty", ()),
    ]


# ---------------------------------------------------------------------------------------------------------- extreme coordinates
def _K(f, cx, cy):
    K = np.eye(4, dtype=f32)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = cx, cy
    return K


def extreme_cases():
    """Row bounds at and beyond 2^31 on either side of the frame: what the fill converts to int must stay in range (x_left starts at
    W and is only lowered, x_right starts at -1 and is only raised), and such rows are left unfilled."""
    s = S_TINY
    big = ((3e9, 1), (4e9, 1), (4e9, 2), (3e9, 2))
    tall = ((1, 3e9), (2, 3e9), (2, 4e9), (1, 4e9))
    out = [
        _pixel_case("x_plus_3e9", "extreme", s, big, "empty"),
        _pixel_case("x_minus_3e9", "extreme", s, [(-x, y) for x, y in big], "empty"),
        _pixel_case("y_plus_3e9", "extreme", s, tall, "empty"),
        _pixel_case("y_minus_3e9", "extreme", s, [(x, -y) for x, y in tall], "empty"),
        # one polygon from x = -3e9 to +3e9 and one from y = -3e9 to +3e9: both bounds are clamped to the frame, nothing is skipped
        _pixel_case("x_span_6e9", "extreme", s, ((-3e9, 1), (3e9, 1), (3e9, 2), (-3e9, 2)), (0, 1, 39, 2)),
        _pixel_case("y_span_6e9", "extreme", s, ((5, -3e9), (10, -3e9), (10, 3e9), (5, 3e9)), (5, 0, 10, 3)),
        # a left bound of exactly 2^31 and a right bound of exactly -2^31
        _pixel_case("x_plus_2p31", "extreme", s, ((2.0 ** 31, 0), (2.0 ** 32, 0), (2.0 ** 32, 3), (2.0 ** 31, 3)), "empty"),
        _pixel_case("x_minus_2p31", "extreme", s, ((-2.0 ** 32, 0), (-2.0 ** 31, 0), (-2.0 ** 31, 3), (-2.0 ** 32, 3)), "empty"),
    ]
    # a vertex that projects to v = +inf (y = 1e38 overflows the projection): the edge that STARTS at it is NaN on every row it is
    # active on, and those scan lines stay unfilled (rows 2 and 3 here; rows 0 and 1 are filled)
    pts = np.array([[-0.3, -0.2, 1.0], [0.3, -0.2, 1.0], [0.1, 1e38, 1.0], [-0.3, -0.05, 1.0]], dtype=f32)
    out.append(Case("v_inf_vertex", "extreme", s, _K(10.0, 20.0, 2.0), EYE, pts, None, ("v_inf",)))
    # vertices a hair in front of the camera plane (z = 3e-8: s = 1 / 4e-8): u = 2.5e9 and 5e9 on rows 2 and 3
    z = 3e-8
    pts = np.array([[1.0, 0.0, z], [2.0, 0.0, z], [2.0, 4e-8, z], [1.0, 4e-8, z]], dtype=f32)
    out.append(Case("hair_in_front", "extreme", s, _K(100.0, 20.0, 2.0), EYE, pts, "empty", ("u_past_2p31",)))
    return out


# ---------------------------------------------------------------------------------------------------------- cameras
def pose2d(x, y, yaw, z=0.0):
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = math.cos(yaw), -math.sin(yaw), math.sin(yaw), math.cos(yaw)
    T[0, 3], T[1, 3], T[2, 3] = x, y, z
    return T


def camera_pose(x, y, yaw, pitch=0.5, roll=0.0, h=0.8):
    """pose_cam_in_world of a camera (z forward, x right, y down) at height h above (x, y), pitched down, rolled about its axis."""
    R = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    cp, sp, cr, sr = math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rp = np.array([[1.0, 0, 0], [0, cp, sp], [0, -sp, cp]])
    Rr = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1.0]])
    T = np.eye(4)
    T[:3, :3] = R @ Rp @ Rr
    return (pose2d(x, y, yaw, h) @ T).astype(f32)


def footprints():
    """(the 40-point footprint of make_polygon_from_points, the 1000-point plane of make_footprint_with_node), as fp32 arrays."""
    import torch

    from wild_visual_navigation_amd.traversability_estimator import SupervisionNode
    from wild_visual_navigation_amd.utils import make_polygon_from_points

    quad = torch.tensor([[1.2, 0.35, 0.0], [1.2, -0.35, 0.0], [2.4, -0.45, 0.0], [2.4, 0.45, 0.0]])

    def sup(t, x, untrav):
        return SupervisionNode(timestamp=t, pose_base_in_world=torch.from_numpy(pose2d(x, 0, 0)).float(),
                               pose_footprint_in_base=torch.eye(4), width=0.7, length=1.0, height=0.4, supervision=torch.ones(1),
                               traversability=torch.tensor([0.2]), traversability_var=torch.tensor([0.1]), is_untraversable=untrav,
                               twist_in_base=torch.tensor([0.8, 0.1, 0.0]))

    plane = sup(1.0, 2.4, True).make_footprint_with_node(sup(0.0, 1.6, False))
    return make_polygon_from_points(quad, grid_size=10).numpy().astype(f32), plane.numpy().astype(f32)


# name -> (K, pose, conditions the host file holds on the oracle for the 40-point footprint)
CAMERAS = {
    "pitched": (_K(300.0, 224.0, 224.0), camera_pose(0.0, 0.0, 0.0, pitch=0.5), ("horizontal_edge", "fills")),
    "rolled": (_K(300.0, 224.0, 224.0), camera_pose(0.1, -0.05, 0.15, pitch=0.5, roll=0.3), ("no_horizontal_edge", "fills")),
    "standing_on_it": (_K(300.0, 224.0, 224.0), camera_pose(1.8, 0.0, 0.0, pitch=0.5), ("behind_and_in_front", "fills")),
    "out_bottom_and_side": (_K(300.0, 224.0, 224.0), camera_pose(1.0, 0.0, 0.45, pitch=0.8), ("touches_bottom", "touches_side", "fills")),
    "beside": (_K(300.0, 224.0, 224.0), camera_pose(0.0, 0.0, 1.2, pitch=0.5), ("in_front", "empty")),
}


def camera_cases():
    fp40, plane = footprints()
    assert fp40.shape == (40, 3) and plane.shape == (1000, 3)
    out = []
    for name, (K, pose, cond) in CAMERAS.items():
        out.append(Case(f"camera_{name}_40", "camera", S_PROD, K, pose, fp40, None, cond))
        out.append(Case(f"camera_{name}_1000", "camera", S_PROD, K, pose, plane, None, ()))
    return out


# ---------------------------------------------------------------------------------------------------------- LDS bound
def lds_polygon(n):
    ang = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    return np.stack([224.0 + 200.0 * np.cos(ang), 224.0 + 150.0 * np.sin(ang)], 1).astype(f32)


def lds_cases():
    """The most points the launcher accepts at 448 rows (renders), and one more (refused, mask untouched)."""
    s = (1, LDS_MAX_H, 448)
    return [_pixel_case(f"lds_{LDS_MAX_N}", "lds", s, lds_polygon(LDS_MAX_N), None, ("fills",)),
            _pixel_case(f"lds_{LDS_MAX_N + 1}", "lds", s, lds_polygon(LDS_MAX_N + 1), None, ("refused",))]


_TABLE = []


def all_cases():
    if not _TABLE:
        _TABLE.extend(rectangle_cases() + ellipse_cases() + degenerate_cases() + extreme_cases() + camera_cases() + lds_cases())
        assert len({c.name for c in _TABLE}) == len(_TABLE)
    return list(_TABLE)


def family(name):
    return [c for c in all_cases() if c.family == name]


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


def three_polygons():
    """(three camera cases, points [3, 40, 3]): a different polygon for each of three nodes -- the 40-point footprint as it is,
    reversed and moved, and moved the other way -- for the batched-points branch."""
    cams = [by_name(f"camera_{k}_40") for k in ("pitched", "rolled", "out_bottom_and_side")]
    move = np.array([[0.0, 0.0, 0.0], [0.15, -0.1, 0.0], [-0.05, 0.2, 0.0]], dtype=f32)
    pts = np.stack([cams[0].points, cams[1].points[::-1], cams[2].points]) + move[:, None]
    return cams, pts.astype(f32)


# ---------------------------------------------------------------------------------------------------------- start masks
QUIET_NANS = (0x7FC00000, 0x7FC00123, 0xFFC00000, 0xFFC54321)     # quiet NaNs with payloads and both signs


def start_mask(shape, kind, seed=0):
    """"nan": every pixel the default NaN.  "mix": a seeded mix of NaNs (payloads included), values on both sides of VALUE, VALUE
    itself and +-inf."""
    C, H, W = shape
    if kind == "nan":
        return np.full(shape, np.nan, dtype=f32)
    assert kind == "mix"
    rng = np.random.default_rng([seed, C, H, W])
    m = rng.uniform(0.0, 1.3, shape).astype(f32)
    pick = rng.integers(0, 10, shape)
    bits = m.view(np.uint32)
    nans = np.array(QUIET_NANS, dtype=np.uint32)[rng.integers(0, len(QUIET_NANS), shape)]
    bits[pick < 4] = nans[pick < 4]
    m[pick == 4] = np.inf
    m[pick == 5] = -np.inf
    m[pick == 6] = f32(VALUE)
    return m
