"""The traversability grid map without a GPU: tests/grid_map_ref.py (the definition ops.grid_fuse_images / ops.grid_sdf / ops.grid_carrot
are held to bit for bit in tests/test_gpu_grid_map.py) against independent statements -- a brute-force minimum and scipy's distance
transform for the EDT, float64 restatements for the fusion and the goal selection --, the message-order helpers, and every refusal of
the Python surface and the C-ABI that happens before a device is touched."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_map_cases as GC  # noqa: E402
import grid_map_ref as G  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wvn_grid_fuse_images", "wvn_grid_sdf", "wvn_grid_carrot")
FUSION = GC.fusion_cases()


# ------------------------------------------------------------------------------------------------------------------ the surface
def test_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wvn_hip.h")).read(), flags=re.S)
    h = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in wvn_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(h, name)
        assert getattr(h, name).argtypes is not None
    for name, value in (("WVN_GRID_MAX_N", _lib.GRID_MAX_N), ("WVN_GRID_MAX_CHANNELS", _lib.GRID_MAX_CHANNELS),
                        ("WVN_GRID_MAX_CAMERAS", _lib.GRID_MAX_CAMERAS), ("WVN_GRID_MAX_DISCS", _lib.GRID_MAX_DISCS)):
        assert re.search(rf"#define {name} {value}\b", src)
    for mode, value in _lib.GRID_UNKNOWN.items():
        assert re.search(rf"#define WVN_GRID_UNKNOWN_{mode.upper()} {value}\b", src)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every pointer below is host memory (never dereferenced by a refused call) and no stream exists: 1001 comes back without a GPU."""
    h = _lib.lib()
    words = (C.c_longlong * 64)()
    p = C.addressof(words)
    table = (C.c_void_p * 4)(p, p, p, p)
    inf = float("inf")

    def fuse(maps=p, B=1, Cc=2, H=24, W=40, K=p, T=p, elev=p, N=16, r=0.1, layers=table, hits=p, alpha=0.5, min_depth=0.1,
             max_range=inf, margin=0.05):
        return h.wvn_grid_fuse_images(maps, B, Cc, H, W, K, T, elev, N, 0.0, 0.0, r, layers, hits, alpha, min_depth, max_range, margin, None)

    for kw in (dict(maps=None), dict(K=None), dict(T=None), dict(elev=None), dict(layers=None), dict(hits=None), dict(N=0), dict(N=-3),
               dict(N=_lib.GRID_MAX_N + 1), dict(Cc=0), dict(Cc=5), dict(B=0), dict(B=-1), dict(B=_lib.GRID_MAX_CAMERAS + 1), dict(H=0),
               dict(W=-2), dict(H=1 << 16, W=1 << 16), dict(r=0.0), dict(r=-0.1), dict(r=float("nan")), dict(r=inf), dict(alpha=-0.1),
               dict(alpha=1.5), dict(alpha=float("nan")), dict(max_range=float("nan")), dict(min_depth=float("nan")),
               dict(margin=float("nan")), dict(layers=(C.c_void_p * 4)(p, None, p, p))):
        assert fuse(**kw) == _lib.ERR_ARG, kw

    def sdf(layer=p, N=16, unknown=0, r=0.1, d2=p, out=p):
        return h.wvn_grid_sdf(layer, N, 0.5, unknown, r, d2, out, None)

    for kw in (dict(layer=None), dict(d2=None), dict(out=None), dict(N=0), dict(N=-1), dict(N=_lib.GRID_MAX_N + 1), dict(unknown=3),
               dict(unknown=-1), dict(r=0.0), dict(r=float("nan"))):
        assert sdf(**kw) == _lib.ERR_ARG, kw

    def carrot(s=p, elev=p, N=200, cos=1.0, sin=0.0, dff=0.0, cff=0.0, discs=(30, 15, 55, 20, 90, 25), n=None, r=0.04, cell=p, goal=p):
        t = (C.c_int * max(len(discs), 1))(*discs) if discs is not None else None
        return h.wvn_grid_carrot(s, elev, N, cos, sin, dff, cff, t, len(discs) // 2 if n is None else n, 0.0, 0.0, r, cell, goal, None, None)

    for kw in (dict(s=None), dict(elev=None), dict(cell=None), dict(goal=None), dict(discs=None, n=3), dict(N=0), dict(N=-5),
               dict(N=_lib.GRID_MAX_N + 1), dict(n=0), dict(n=-1), dict(discs=(1, 1) * (_lib.GRID_MAX_DISCS + 1)), dict(discs=(-1, 5)),
               dict(discs=(5, -1)), dict(discs=(1 << 21, 5)), dict(cos=1.5), dict(sin=float("nan")), dict(dff=float("nan")),
               dict(cff=float("nan")), dict(r=0.0)):
        assert carrot(**kw) == _lib.ERR_ARG, kw
    assert all(w == 0 for w in words)


def test_ops_refuse_cpu_tensors():
    N = 8
    f = torch.zeros(N, N)
    i = torch.zeros(N, N, dtype=torch.int32)
    with pytest.raises(_lib.WvnError):
        ops.grid_fuse_images(torch.zeros(1, 1, 4, 4), torch.eye(4)[None], torch.eye(4)[None], f, [f.clone()], i, (0.0, 0.0), 0.1)
    with pytest.raises(_lib.WvnError):
        ops.grid_sdf(f, 0.5, 0.1)
    with pytest.raises(_lib.WvnError):
        ops.grid_carrot(f, f, 0.0, (0.0, 0.0), 0.1)
    from wild_visual_navigation_amd.grid_map import SmartCarrot, TraversabilityGridMap  # noqa: F401

    with pytest.raises(_lib.WvnError):
        TraversabilityGridMap(device="cpu")


def test_message_order_helpers_round_trip_and_match_the_reference_expression():
    from wild_visual_navigation_amd.grid_map import layer_from_message, layer_to_message

    rng = np.random.default_rng(0)
    n_rows = n_cols = 7
    data = rng.uniform(size=n_rows * n_cols).astype(np.float32)
    want = np.reshape(np.array(list(data)), (n_rows, n_cols))[::-1, ::-1].transpose().astype(np.float32)   # smart_carrot.py:106-107
    got = layer_from_message(data, n_rows, n_cols)
    assert got.is_contiguous() and np.array_equal(got.numpy(), want) and np.array_equal(G.layer_from_message(data, n_rows, n_cols), want)
    back = layer_to_message(got)
    assert np.array_equal(back.numpy(), data) and np.array_equal(back.numpy(), want[::-1, ::-1].transpose().ravel())    # :164
    assert np.array_equal(G.layer_to_message(want), data)
    assert got[0, 0] == data[-1] and got[0, 1] == data[-1 - n_cols]     # the first map cell is the message's last; axis 1 walks its rows


# -------------------------------------------------------------------------------------------------------------------------- EDT
def _members(N, seed):
    rng = np.random.default_rng(seed)
    sets = [np.zeros((N, N), bool), np.ones((N, N), bool), rng.uniform(size=(N, N)) < 0.5, rng.uniform(size=(N, N)) < 0.03,
            rng.uniform(size=(N, N)) < 0.97]
    one = np.zeros((N, N), bool)
    one[N - 1, 0] = True
    return sets + [one]


@pytest.mark.parametrize("N", [1, 2, 3, 7, 16, 33])
def test_edt_equals_the_brute_force_minimum(N):
    for member in _members(N, N):
        got, want = G.edt_squared(member), G.edt_squared_brute(member)
        assert np.array_equal(np.minimum(got, G.FAR), np.minimum(want, G.FAR))


def test_edt_equals_scipy_at_production_size():
    from scipy import ndimage
    N = 200
    for member in _members(N, 200)[2:]:
        want = np.rint(ndimage.distance_transform_edt(~member) ** 2).astype(np.int64)   # distance of the non-members to the set
        assert int((G.edt_squared(member) != want).sum()) == 0


def test_sdf_signs_modes_and_empty_sets():
    from scipy import ndimage
    layer = GC.sdf_layers(65)["values_with_nan"]
    nan = np.isnan(layer)
    for unknown in G.UNKNOWN:
        s, d2 = G.sdf(layer, 0.5, 0.04, unknown)
        obstacle, free = G.classify(layer, 0.5, unknown)
        assert not (obstacle & free).any() and ((obstacle | free) == (~nan if unknown == "neither" else True)).all()
        assert (d2[free] > 0).all() and (d2[obstacle] < 0).all() and (d2[~(free | obstacle)] == 0).all()
        assert np.isnan(s[~(free | obstacle)]).all() and s.dtype == np.float32 and d2.dtype == np.int32
        want = np.where(free, np.rint(ndimage.distance_transform_edt(~obstacle) ** 2), -np.rint(ndimage.distance_transform_edt(~free) ** 2))
        assert int((d2[free | obstacle] != want[free | obstacle]).sum()) == 0
        assert np.array_equal(np.abs(s[free | obstacle]), np.float32(0.04) * np.sqrt(np.abs(d2[free | obstacle]).astype(np.float32)))
    s, d2 = G.sdf(np.full((5, 5), np.float32(0.9)), 0.5, 0.1)
    assert (s == np.inf).all() and (d2 == G.I32_MAX).all()
    s, d2 = G.sdf(np.full((5, 5), np.float32(0.1)), 0.5, 0.1)
    assert (s == -np.inf).all() and (d2 == -G.I32_MAX).all()
    s, d2 = G.sdf(np.full((5, 5), np.float32(np.nan)), 0.5, 0.1, "neither")
    assert np.isnan(s).all() and (d2 == 0).all()


# ----------------------------------------------------------------------------------------------------------------------- fusion
def _fuse(case, dtype):
    return G.fuse(case["maps"], case["intrinsics"], case["poses"], case["elevation"], case["layers"], case["hits"], case["center"],
                  case["resolution"], dtype=dtype, **case["params"])


def _fuse_scalar_float64(case):
    """The rules of the issue cell by cell in Python floats, written without looking at the array form: the camera matrix is inverted
    by numpy, the pixel is rounded with math.floor, the walk is a while loop.  -> (layers, hits, fused [B,N,N], pixel [B,N,N])."""
    p = dict(alpha=0.5, min_depth=0.1, max_range=None, occlusion_margin=0.05)
    p.update(case["params"])
    alpha, margin = float(np.float32(p["alpha"])), float(np.float32(p["occlusion_margin"]))
    min_depth = float(np.float32(p["min_depth"]))
    max_range = math.inf if p["max_range"] is None else float(np.float32(p["max_range"]))
    maps, elev = case["maps"].astype(np.float64), case["elevation"].astype(np.float64)
    B, Cc, H, W = maps.shape
    N, r = case["N"], float(np.float32(case["resolution"]))
    cx, cy = float(np.float32(case["center"][0])), float(np.float32(case["center"][1]))
    layers, hits = case["layers"].astype(np.float64).copy(), case["hits"].copy()
    fused, pixel = np.zeros((B, N, N), bool), np.full((B, N, N), -1)
    world_to_cam = [np.linalg.inv(T.astype(np.float64)) for T in case["poses"]]
    for i in range(N):
        for j in range(N):
            z = elev[i, j]
            if math.isnan(z):
                continue
            x, y = cx + (i - N / 2) * r, cy + (j - N / 2) * r
            for b in range(B):
                pc = world_to_cam[b] @ np.array([x, y, z, 1.0])
                if not pc[2] > min_depth:
                    continue
                q = case["intrinsics"][b].astype(np.float64) @ pc
                u, v = q[0] / q[2], q[1] / q[2]
                iu, iv = math.floor(u + 0.5), math.floor(v + 0.5)
                if not (0 <= iu < W and 0 <= iv < H):
                    continue
                cam = case["poses"][b].astype(np.float64)[:3, 3]
                L = math.hypot(cam[0] - x, cam[1] - y)
                if L > max_range:
                    continue
                val = maps[b, :, iv, iu]
                if np.isnan(val).all():
                    continue
                pixel[b, i, j] = iv * W + iu
                visible, s = True, 1
                while s <= math.floor(L / r):
                    t = s * r / L
                    qx, qy, qz = x + t * (cam[0] - x), y + t * (cam[1] - y), z + t * (cam[2] - z)
                    ni, nj = math.floor((qx - cx) / r + N / 2 + 0.5), math.floor((qy - cy) / r + N / 2 + 0.5)
                    if not (0 <= ni < N and 0 <= nj < N):
                        break
                    if math.isfinite(elev[ni, nj]) and elev[ni, nj] - qz > margin:
                        visible = False
                        break
                    s += 1
                if not visible:
                    continue
                for c in range(Cc):
                    if not math.isnan(val[c]):
                        layers[c, i, j] = val[c] if math.isnan(layers[c, i, j]) else layers[c, i, j] * (1 - alpha) + alpha * val[c]
                hits[i, j] += 1
                fused[b, i, j] = True
    return layers, hits, fused, pixel


@pytest.mark.parametrize("name", list(FUSION))
def test_fp32_fusion_statement_against_float64(name):
    """The fp32 statement and the float64 restatement agree exactly on visible / hidden and on the pixel, and within 1e-6 on the fused
    values, on every cell that is not within 1e-3 of a decision boundary in float64 (pixel rounding in pixels, depth limit and
    occlusion margin in metres); at most 5 % of the valid cells of a case may be left out."""
    case = FUSION[name]
    l32, h32, i32 = _fuse(case, np.float32)
    l64, h64, i64 = _fuse(case, np.float64)
    valid = ~np.isnan(case["elevation"])
    near = np.zeros_like(valid)
    for cam in i64:
        near |= cam["boundary"] < 1e-3
        assert cam["range_gap"].min() > 1e-3, "the case puts a cell on the max_range boundary: change the case"
    keep = valid & ~near
    print(f"{name}: {int(near.sum())} of {int(valid.sum())} valid cells within 1e-3 of a boundary")
    assert near.sum() <= 0.05 * valid.sum()
    for a, b in zip(i32, i64):
        for key in ("visible", "pixel", "fused"):
            assert np.array_equal(a[key][keep], b[key][keep]), key
    assert np.array_equal(h32[keep], h64[keep])
    assert np.array_equal(np.isnan(l32)[:, keep], np.isnan(l64)[:, keep])
    err = np.abs(l32.astype(np.float64) - l64)[:, keep]
    print(f"{name}: max |fp32 - float64| on the fused values = {np.nanmax(err) if np.isfinite(err).any() else 0.0:.3e}")
    assert not (err > 1e-6).any()
    # untouched cells keep their bits; nothing is written where the elevation is unknown
    untouched = h32 == case["hits"]
    assert np.array_equal(l32[:, untouched], case["layers"][:, untouched], equal_nan=True) and untouched[~valid].all()
    assert l32.dtype == np.float32


@pytest.mark.parametrize("name", [n for n, c in FUSION.items() if c["N"] <= 33])
def test_float64_fusion_statement_against_a_cell_by_cell_restatement(name):
    case = FUSION[name]
    l64, h64, i64 = _fuse(case, np.float64)
    layers, hits, fused, pixel = _fuse_scalar_float64(case)
    near = np.zeros((case["N"],) * 2, bool)
    for cam in i64:
        near |= cam["boundary"] < 1e-3
    keep = ~near
    for b, cam in enumerate(i64):
        assert np.array_equal(cam["fused"][keep], fused[b][keep]) and np.array_equal(cam["pixel"][keep], pixel[b][keep])
    assert np.array_equal(h64[keep], hits[keep])
    assert np.allclose(l64[:, keep], layers[:, keep], rtol=0, atol=1e-9, equal_nan=True)


def test_fusion_cases_cover_what_they_claim():
    res = {name: _fuse(c, np.float32) for name, c in FUSION.items()}
    hits = {name: res[name][1] - FUSION[name]["hits"] for name in FUSION}
    assert (hits["all_nan_elevation"] == 0).all() and (hits["behind_and_below"] == 0).all()
    assert not res["behind_and_below"][2][1]["visible"].all()            # the camera below the surface is refused by the walk
    # both orders of the two cameras: the same cells, other values where both cameras fuse, and the defined order
    a, b = res["n33_two_cameras"], res["n33_two_cameras_swapped"]
    both = hits["n33_two_cameras"] == 2
    assert both.sum() > 100 and np.array_equal(hits["n33_two_cameras"], hits["n33_two_cameras_swapped"])
    assert (a[0][:, both] != b[0][:, both]).mean() > 0.9 and np.array_equal(a[0][:, ~both], b[0][:, ~both], equal_nan=True)
    c = FUSION["n33_two_cameras"]
    al = np.float32(0.3)
    first_touch = both & np.isnan(c["layers"][0])
    existing = both & ~np.isnan(c["layers"][0])
    assert first_touch.sum() > 20 and existing.sum() > 20
    px0, px1 = a[2][0]["pixel"], a[2][1]["pixel"]
    v0, v1 = c["maps"][0, 0].ravel()[px0[both]], c["maps"][1, 0].ravel()[px1[both]]
    old = c["layers"][0][both]
    step0 = np.where(np.isnan(old), v0, old * (np.float32(1) - al) + al * v0)
    assert np.array_equal(a[0][0][both], step0 * (np.float32(1) - al) + al * v1)
    # straight down: the cell under the camera takes no step and is fused; the posts hide cells on the axes and on the diagonals
    sd = res["straight_down_axes_diagonals"]
    assert hits["straight_down_axes_diagonals"][16, 16] == 1
    hidden = ~sd[2][0]["visible"]
    assert hidden[16, 23:].all() and hidden[:10, 16].all() and hidden[22, 22] and not hidden[16, 17:22].any() and hidden[16, :9].all()
    # the wall hides cells behind it, not in front of it
    hidden = ~res["wall"][2][0]["visible"]
    assert hidden[21:, 12:20].all() and not hidden[:20].any()
    w = res["wall_on_edge_camera_outside"][2]
    assert (~w[0]["visible"]).sum() > 500 and 0 < (~w[1]["visible"]).sum() < 500
    # NaN pixels: cells whose pixel is NaN in every channel are skipped, those with one NaN channel keep that layer only
    n = res["nan_pixels"]
    c = FUSION["nan_pixels"]
    px = n[2][0]["pixel"]
    seen = px >= 0
    one = seen & np.isnan(c["maps"][0, 0].ravel()[np.maximum(px, 0)])
    assert one.sum() > 5 and np.isnan(n[0][0][one]).all() and not np.isnan(n[0][1][one]).any() and (hits["nan_pixels"][one] == 1).all()
    assert (hits["max_range"] == 1).sum() == 129                           # the lattice points with a^2 + b^2 <= 40
    assert set(np.unique(hits["four_channels_three_cameras"])) >= {1, 2, 3}
    assert FUSION["n200_production"]["N"] == 200 and (hits["n200_production"] == 2).sum() > 1000


# ------------------------------------------------------------------------------------------------------------------------ carrot
CARROT = GC.carrot_cases()


@pytest.mark.parametrize("name", [n for n, _ in CARROT])
def test_fp32_carrot_statement_picks_the_float64_cell(name):
    kw = dict(CARROT)[name]
    a, b = G.carrot(**kw), G.carrot_float64(**kw)
    assert (a["i"], a["j"], a["found"]) == (b["i"], b["j"], b["found"])
    assert np.array_equal(np.isneginf(a["masked"]), np.isneginf(b["masked"]))
    top = np.sort(b["masked"].ravel())[-2:]
    if "ties" in name or "constant" in name:
        assert top[0] == top[1] and np.array_equal(a["masked"].astype(np.float64), b["masked"])      # exact in both precisions
        assert a["i"] * kw["sdf"].shape[0] + a["j"] == np.flatnonzero(b["masked"].ravel() == top[1])[0]
    elif "all_masked" in name:
        assert a["found"] == 0 and (a["i"], a["j"]) == (0, 0) and np.isneginf(a["masked"]).all()
    else:
        assert a["found"] == 1 and top[1] - top[0] > 1e-4, "best and second best too close: change the case"
        assert abs(float(a["score"]) - b["score"]) < 1e-4
    N, r = kw["sdf"].shape[0], kw["resolution"]
    assert abs(float(a["x"]) - ((a["i"] - N / 2) * r + kw["center"][0])) < 1e-5          # smart_carrot.py:145-150
    assert abs(float(a["y"]) - ((a["j"] - N / 2) * r + kw["center"][1])) < 1e-5
    if a["found"]:
        assert G.pattern(N, kw["yaw"], kw["discs"])[a["i"], a["j"]] and not G.elevation_mask(kw["elevation"])[a["i"], a["j"]]


def test_carrot_cases_cover_what_they_claim():
    assert len(GC.YAWS) == 16
    # the two yaws around asin(0.1) put the first disc's column centre on either side of a whole number
    lo, hi = (G.disc_centres(200, y)[0][1] for y in GC.YAWS[13:15])
    assert (lo, hi) == (102, 103)
    assert G.disc_centres(200, GC.YAWS[15])[0][0] == 99 and G.disc_centres(200, math.pi / 2)[0][0] == 100   # cos just below / above 0
    # cv2.circle's (x, y) is (column, row): at yaw 0 the pattern runs along axis 0
    keep = G.pattern(200, 0.0)
    assert keep[130, 100] and keep[190, 100] and not keep[100, 130] and keep.sum() > 3000
    # the dilation reaches one cell and stays inside the grid
    e = np.zeros((5, 5), np.float32)
    e[0, 0] = e[4, 2] = np.nan
    m = G.elevation_mask(e)
    assert m.sum() == 4 + 6 and m[1, 1] and m[3, 1] and m[3, 3] and not m[2, 2]
    names = [n for n, _ in CARROT]
    assert any("nan_border" in n for n in names) and any("nan_scores" in n for n in names)
    kw = dict(CARROT)["n200_nan_scores"]
    assert np.isnan(kw["sdf"][GC.pattern_peak(200, 0.0, kw["discs"])])
