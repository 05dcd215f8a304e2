"""Elevation from depth without a GPU: tests/elevation_ref.py (the definition csrc/elevation.hip is held to bit for bit in
tests/test_gpu_elevation.py) against a float64 restatement that applies the exact sequential Kalman update point by point in a random
order, the overflow bound of its integer sums by arithmetic, the depth form against the point form, what the case table claims to cover,
and every refusal of the C-ABI and of the Python surface that happens before a device is touched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_cases as EC  # noqa: E402
import elevation_ref as E  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wvn_grid_elevation_workspace_bytes", "wvn_grid_elevation_accumulate_points", "wvn_grid_elevation_accumulate_depth",
               "wvn_grid_elevation_finalise")
CASES = EC.cases()
EPS64 = np.finfo(np.float64).eps


def _record(c):
    """The classify() record of a case (depth cases through their back-projected cloud)."""
    p = E.params(**c["params"])
    z_ref = E.default_z_ref(c["poses"]) if c["z_ref"] is None else np.float32(c["z_ref"])
    if c["kind"] == "depth":
        pts, valid = E.backproject(c["depth"], c["intrinsics"])
        counts = None
    else:
        pts, valid, counts = c["points"], None, c["counts"]
    return E.classify(pts, c["poses"], counts, c["elevation"], c["variance"], c["center"], c["resolution"], z_ref, p, valid), z_ref, p


# ---------------------------------------------------------------------------------------------- the definition against float64 Kalman
@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("contention")] + ["contention_known"])
def test_reference_agrees_with_the_sequential_kalman_update(name):
    """Per cell with inliers, the fixed-point information form against the exact sequential update in float64 (unquantised weights
    w_i = the fp32 1 / v_i, heights q_z, random order).  With the prior as one more exact measurement (w_0 = 1 / var, z_0 = h), both are
    weighted means, so the allowed difference follows from the format and is evaluated here in float64, per cell:
      heights:  half an LSB of zq (2^-15 m)  +  half an ulp of the fp32 difference q_z - z_ref (the largest of the cell)
                +  sum_i |w_i - wq_i / 256| |z_i - z_mean| / sum w        (truncated weights move a weighted mean by at most this)
      variance: var_ref var_seq sum_i |w_i - wq_i / 256|                  (1 / W' - 1 / W = (W - W') / (W W'))
      both:     half an ulp of the fp32 result, and (8 + 4 n) float64 roundings of the magnitudes involved (the 8 operations of the
                finalise step, 4 per point of the sequential update)."""
    c = CASES[name]
    rec, z_ref, p = _record(c)
    h_ref, var_ref, _, _, _, sums = EC.reference(name)
    order = np.random.default_rng(len(name)).permutation(rec["live"].size)
    h_seq, var_seq = E.kalman_sequential(rec, c["elevation"], c["variance"], z_ref, p, order)
    inl = rec["live"] & (rec["cls"] == 7)
    N = c["N"]
    checked = 0
    worst = [0.0, 0.0]
    for cell in np.unique(rec["cell"][inl]):
        i, j = divmod(int(cell), N)
        m = inl & (rec["cell"] == cell)
        w = rec["w"][m].astype(np.float64)
        z = rec["qz"][m].astype(np.float64)
        delta = np.abs(w - rec["wq"][m] / 256.0)
        n = int(m.sum())
        W = w.sum()
        zs = z
        h0, v0 = float(c["elevation"][i, j]), float(c["variance"][i, j])
        if np.isfinite(h0):
            W += 1.0 / v0
            zs = np.append(z, h0)
        mean = h_seq[i, j]
        rel = np.abs(rec["qz"][m] - np.float32(z_ref)).astype(np.float32)
        rounding = (8 + 4 * n) * EPS64
        bound_h = 2.0 ** -15 + float(np.spacing(rel.max())) / 2 + float((delta * np.abs(z - mean)).sum() / W) \
            + float(np.spacing(np.float32(abs(mean)))) / 2 + rounding * (np.abs(zs).max() + abs(float(z_ref)))
        want_var = min(var_seq[i, j] + float(np.float32(p["outlier_variance"])) * int(sums["n_out"][i, j]), float(np.float32(p["max_variance"])))
        bound_v = float(var_ref[i, j]) * var_seq[i, j] * delta.sum() + float(np.spacing(np.float32(want_var))) / 2 + rounding * want_var
        err_h, err_v = abs(float(h_ref[i, j]) - mean), abs(float(var_ref[i, j]) - want_var)
        worst = [max(worst[0], err_h / bound_h), max(worst[1], err_v / bound_v)]
        assert err_h <= bound_h, (name, i, j, err_h, bound_h)
        assert err_v <= bound_v, (name, i, j, err_v, bound_v)
        checked += 1
    print(f"{name}: {checked} cells, largest error / bound = {worst[0]:.3f} (height), {worst[1]:.3f} (variance)")
    assert checked == int((sums["n"] > 0).sum()) and (checked > 0) == c["has_inliers"]


def test_the_integer_sums_cannot_overflow():
    """By arithmetic, not by running 2^22 points: the largest weight and height the format produces, times the largest call."""
    f = np.float32
    wq_max = int(np.floor(np.minimum(f(np.inf), E.WQ_CAP) * E.WQ_SCALE))
    zq_max = int(np.rint(E.ZQ_RANGE * E.ZQ_SCALE))
    assert wq_max == 2 ** 20 - 1 and zq_max == 2 ** 21
    assert float(E.WQ_CAP) == 4096 - 1 / 256 and float(E.WQ_CAP * E.WQ_SCALE) == 2 ** 20 - 1     # both exact in fp32
    assert E.MAX_POINTS == 2 ** 22 == _lib.GRID_ELEVATION_MAX_POINTS
    assert E.MAX_POINTS * wq_max * zq_max < 2 ** 63 and E.MAX_POINTS * wq_max < 2 ** 42
    assert (E.MAX_POINTS + 1) * 2 ** 20 * zq_max > 2 ** 63                                       # ... and the bound is not slack by 2x
    # the contention case sits on both extremes
    rec, _, _ = _record(CASES["contention_unknown"])
    assert (rec["wq"] == wq_max).all() and (rec["zq"] == zq_max).all()
    rec, _, _ = _record(CASES["contention_known"])
    assert (rec["wq"] == wq_max).all() and (rec["zq"] == -zq_max).all()
    # the reference refuses a larger call (a zero-stride view: nothing of that size is allocated)
    big = np.broadcast_to(np.float32([[[1.0, 0.0, 0.0]]]), (1, E.MAX_POINTS + 1, 3))
    blank = EC.blank(8)
    with pytest.raises(ValueError):
        E.accumulate(big, np.eye(4, dtype=np.float32)[None], None, blank[0], blank[1], (0.0, 0.0), 0.5, 0.0, E.params())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wvn_hip.h")).read(), flags=re.S)
    assert re.search(rf"#define WVN_GRID_ELEVATION_MAX_POINTS {2 ** 22}\b", src)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] == "depth"])
def test_depth_form_equals_point_form_on_the_backprojected_cloud(name):
    """The cloud is written out here, pixels without a depth as NaN points; the point form on it gives the depth form's bits."""
    c = CASES[name]
    pts, valid = E.backproject(c["depth"], c["intrinsics"])
    z = c["depth"].astype(np.float32) / np.float32(1000.0) if c["depth"].dtype == np.uint16 else c["depth"]
    H, W = c["depth"].shape[1:]
    K = c["intrinsics"]
    for b, v, u in ((0, 0, 0), (K.shape[0] - 1, H - 1, W - 1), (0, H // 2, W // 3)):       # the issue's formula, pixel by pixel
        want = ((np.float32(u) - K[b, 0, 2]) * (z[b, v, u] / K[b, 0, 0]), (np.float32(v) - K[b, 1, 2]) * (z[b, v, u] / K[b, 1, 1]), z[b, v, u])
        assert np.array_equal(pts[b, v * W + u], np.float32(want), equal_nan=True)
    assert np.array_equal(valid, (np.isfinite(z) & (z != 0)).reshape(valid.shape)) and 0 < (~valid).sum() < valid.size
    cloud = np.where(valid[..., None], pts, np.float32(np.nan))
    want = EC.reference(name)
    got = E.add_points(cloud, c["poses"], c["elevation"], c["variance"], c["layers"], c["hits"], c["center"], c["resolution"],
                       z_ref=c["z_ref"], clear_rays=c["clear_rays"], p=E.params(**c["params"]))
    for a, b in zip(got[:4], want[:4]):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))
    assert got[4] == want[4] and got[4]["invalid"] == int((~valid).sum())


# --------------------------------------------------------------------------------------------------------- what the table covers
def test_case_table_covers_what_it_claims():
    names = set(CASES)
    assert {f"shape_n{N}_p{P}" for N in (8, 33, 200) for P in (1, 63, 64, 65, 1000)} <= names
    assert {f"depth_{H}x{W}_{t}" for H, W in ((8, 8), (17, 31), (64, 48)) for t in ("f32", "u16")} <= names
    for n in names:
        if n.startswith("depth_") and n.endswith("u16"):
            assert CASES[n]["depth"].dtype == np.uint16
    assert CASES["contention_unknown"]["points"].shape[1] == 65536 and EC.reference("contention_unknown")[5]["n"].max() == 65536
    # every rejection class, with its counter
    assert EC.reference("rejection_classes")[4] == dict(invalid=3, near=2, high=2, ramp=3, outside=6, gated=3, unrepresentable=0, inliers=11)
    assert EC.reference("rejection_unrepresentable")[4] == dict(invalid=3, near=2, high=2, ramp=3, outside=6, gated=3, unrepresentable=11, inliers=0)
    assert EC.reference("rejection_zero_weight")[4]["unrepresentable"] == 3
    # borders: a point exactly on a border belongs to the upper cell; the map's lower edge is inside, its upper edge outside
    c = CASES["rejection_classes"]
    rec, _, _ = _record(c)
    rows = c["points"][0]
    cell_of = {tuple(r): int(k) for r, k in zip(rows.tolist(), rec["cell"])}
    assert cell_of[(-0.25, 0.75, -0.5)] == 4 * 8 + 6 and cell_of[(0.25, -0.75, -0.5)] == 5 * 8 + 3
    assert cell_of[(-2.25, 0.0, -0.5)] == 0 * 8 + 4 and cell_of[(0.0, -2.25, -0.5)] == 4 * 8 + 0
    assert rec["cls"][[tuple(r) == (1.75, 0.0, -0.5) for r in rows.tolist()]].tolist() == [4]
    # gate: known and unknown prior cells; a cell that receives only outliers keeps its elevation bits and grows by n_out * outlier_variance
    for name in ("gate", "rejection_classes"):
        c = CASES[name]
        h, var, _, _, stats, sums = EC.reference(name)
        only_out = (sums["n"] == 0) & (sums["n_out"] > 0)
        assert only_out.sum() >= 1 and stats["gated"] >= 3
        assert np.array_equal(h.view(np.int32)[only_out], c["elevation"].view(np.int32)[only_out])
        want = (c["variance"][only_out].astype(np.float64) + np.float64(np.float32(0.01)) * sums["n_out"][only_out]).astype(np.float32)
        assert np.array_equal(var[only_out], want) and (var[only_out] > c["variance"][only_out]).all()
    known, n = np.isfinite(CASES["gate"]["elevation"]), EC.reference("gate")[5]["n"]
    assert (n[known] > 0).sum() > 100 and (n[~known] > 0).sum() > 100
    untouched = (n == 0) & (EC.reference("gate")[5]["n_out"] == 0)
    assert untouched.sum() > 10 and np.array_equal(EC.reference("gate")[1].view(np.int32)[untouched], CASES["gate"]["variance"].view(np.int32)[untouched])
    # ray clearing: the near wall (row 20) is crossed and cleared with its image layers and hits; the far wall (row 26) is crossed too
    # but hit by inliers and stays; without clear_rays every count stays zero
    c = CASES["walls_clear_1"]
    h, var, layers, hits, _, sums = EC.reference("walls_clear_1")
    cleared = np.isnan(h) & np.isfinite(c["elevation"])
    assert cleared.sum() >= 8 and cleared[20, 8:25].sum() == cleared.sum()
    assert np.isnan(layers[:, cleared]).all() and (hits[cleared] == 0).all() and (var[cleared] == 1000.0).all() and (c["hits"][cleared] > 0).all()
    far = sums["n"][26] > 0
    assert far.sum() >= 10 and (sums["contradicted"][26][far] >= 2).sum() >= 5 and np.isfinite(h[26][far]).all()
    assert np.array_equal(layers[:, ~cleared], c["layers"][:, ~cleared]) and np.array_equal(hits[~cleared], c["hits"][~cleared])
    h0, _, layers0, hits0, _, sums0 = EC.reference("walls_clear_0")
    assert (sums0["contradicted"] == 0).all() and np.isfinite(h0).all() and np.array_equal(hits0, c["hits"])
    assert np.array_equal(sums0["n"], sums["n"]) and np.array_equal(layers0, c["layers"])
    assert (np.isnan(EC.reference("depth_clear")[0]) & np.isfinite(CASES["depth_clear"]["elevation"])).sum() > 20


def test_order_of_points_and_sensors_does_not_matter_in_the_reference():
    c = CASES["order"]
    want = EC.reference("order")
    rng = np.random.default_rng(3)
    pts = np.stack([p[rng.permutation(p.shape[0])] for p in c["points"]])
    sensors = [2, 0, 1]
    got = E.add_points(pts[sensors], c["poses"][sensors], c["elevation"], c["variance"], c["layers"], c["hits"], c["center"], c["resolution"],
                       z_ref=E.default_z_ref(c["poses"]), clear_rays=True)
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert got[4] == want[4]


def test_update_variance_reference():
    c = CASES["gate"]
    v = E.update_variance(c["elevation"], c["variance"])
    known = np.isfinite(c["elevation"])
    assert np.array_equal(v[known], np.minimum(c["variance"][known] + np.float32(1e-4), np.float32(100.0))) and (v[~known] == 1000.0).all()


# ------------------------------------------------------------------------------------------------------------------ the surface
def test_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wvn_hip.h")).read(), flags=re.S)
    h = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in wvn_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(h, name)
    for name, value in (("WVN_GRID_ELEVATION_STATS", len(_lib.GRID_ELEVATION_STATS)), ("WVN_GRID_DEPTH_F32", _lib.GRID_DEPTH_F32),
                        ("WVN_GRID_DEPTH_U16", _lib.GRID_DEPTH_U16), ("WVN_GRID_ELEVATION_CLEAR_RAYS", _lib.GRID_ELEVATION_CLEAR_RAYS)):
        assert re.search(rf"#define {name} {value}\b", src)
    assert _lib.GRID_ELEVATION_STATS == E.STATS
    assert C.sizeof(_lib.GridElevationParams) == 13 * 4
    assert h.wvn_grid_elevation_workspace_bytes(200) == 32 + 200 * 200 * 32
    assert h.wvn_grid_elevation_workspace_bytes(0) == 0 and h.wvn_grid_elevation_workspace_bytes(_lib.GRID_MAX_N + 1) == 0
    d = {k: v for k, v in E.DEFAULTS.items() if k != "time_variance"}
    assert d == ops.GRID_ELEVATION_DEFAULTS


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every pointer below is host memory (never dereferenced by a refused call) and no stream exists: 1001 comes back without a GPU."""
    h = _lib.lib()
    words = (C.c_longlong * 64)()
    p = C.addressof(words)
    table = (C.c_void_p * 4)(p, p, p, p)
    nan, inf = float("nan"), float("inf")

    def prm(**kw):
        return C.byref(ops.grid_elevation_params(**kw))

    def points(pts=p, counts=None, B=2, Pmax=100, poses=p, elev=p, var=p, N=16, cx=0.0, r=0.1, params=None, z=p, flags=0, ws=p, **kw):
        return h.wvn_grid_elevation_accumulate_points(pts, counts, B, Pmax, poses, elev, var, N, cx, 0.0, r, prm(**kw) if params is None else params,
                                                      z, flags, ws, None)

    def depth(d=p, dtype=0, B=2, H=24, W=40, K=p, poses=p, elev=p, var=p, N=16, r=0.1, params=None, z=p, flags=1, ws=p, **kw):
        return h.wvn_grid_elevation_accumulate_depth(d, dtype, B, H, W, K, poses, elev, var, N, 0.0, 0.0, r, prm(**kw) if params is None else params,
                                                     z, flags, ws, None)

    def finalise(elev=p, var=p, layers=table, Cc=2, hits=p, N=16, params=None, z=p, flags=0, ws=p, stats=p, **kw):
        return h.wvn_grid_elevation_finalise(elev, var, layers, Cc, hits, N, prm(**kw) if params is None else params, z, flags, ws, stats, None)

    common = (dict(poses=None), dict(elev=None), dict(var=None), dict(ws=None), dict(ws=p + 4), dict(z=None), dict(params=C.c_void_p(0)), dict(N=0), dict(N=-2),
              dict(N=_lib.GRID_MAX_N + 1), dict(B=0), dict(B=-1), dict(B=_lib.GRID_MAX_CAMERAS + 1), dict(r=0.0), dict(r=-0.1), dict(r=nan),
              dict(r=inf), dict(flags=2), dict(flags=-1), dict(sensor_noise_factor=0.0), dict(sensor_noise_factor=-0.05),
              dict(sensor_noise_factor=nan), dict(sensor_noise_factor=inf), dict(min_valid_distance=-0.5), dict(min_valid_distance=nan),
              dict(mahalanobis_thresh=-1.0), dict(mahalanobis_thresh=nan), dict(max_height_range=nan), dict(ramped_height_range_a=nan),
              dict(ramped_height_range_b=nan), dict(ramped_height_range_c=nan), dict(clear_margin=nan), dict(max_ray_length=-1.0),
              dict(max_ray_length=nan), dict(max_ray_length=inf), dict(max_ray_length=2.0e5))
    for kw in common + (dict(pts=None), dict(Pmax=0), dict(Pmax=-4), dict(B=2, Pmax=2 ** 21 + 1), dict(B=64, Pmax=2 ** 16 + 1), dict(cx=inf)):
        assert points(**kw) == _lib.ERR_ARG, kw
    for kw in common + (dict(d=None), dict(K=None), dict(dtype=2), dict(dtype=-1), dict(H=0), dict(W=-3), dict(B=2, H=2048, W=1025),
                        dict(B=1, H=1 << 16, W=1 << 16), dict(B=1, H=1 << 30, W=4)):
        assert depth(**kw) == _lib.ERR_ARG, kw
    for kw in (dict(elev=None), dict(var=None), dict(hits=None), dict(ws=None), dict(ws=p + 4), dict(stats=None), dict(z=None), dict(params=C.c_void_p(0)),
               dict(layers=None), dict(layers=(C.c_void_p * 4)(p, None, p, p)), dict(Cc=-1), dict(Cc=5), dict(N=0), dict(N=_lib.GRID_MAX_N + 1),
               dict(flags=2), dict(flags=8), dict(outlier_variance=-0.01), dict(outlier_variance=nan), dict(max_variance=0.0), dict(max_variance=nan),
               dict(initial_variance=nan), dict(clear_min_rays=0), dict(clear_min_rays=-2)):
        assert finalise(**kw) == _lib.ERR_ARG, kw
    assert all(w == 0 for w in words)


def test_ops_refuse_cpu_tensors_and_oversized_calls():
    N = 8
    f = torch.zeros(N, N)
    i = torch.zeros(N, N, dtype=torch.int32)
    eye = torch.eye(4)[None]
    with pytest.raises(_lib.WvnError):
        ops.grid_elevation_points(torch.zeros(1, 5, 3), eye, f, f.clone(), [], i, (0.0, 0.0), 0.5)
    with pytest.raises(_lib.WvnError):
        ops.grid_elevation_depth(torch.zeros(1, 4, 4), eye, eye, f, f.clone(), [], i, (0.0, 0.0), 0.5)
    with pytest.raises(_lib.WvnError):
        ops.grid_elevation_params(sensor_noise=0.1)
