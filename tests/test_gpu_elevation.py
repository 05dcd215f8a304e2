"""Elevation from depth on the GPU: ops.grid_elevation_points / ops.grid_elevation_depth against tests/elevation_ref.py with ZERO differing
bits (elevation, variance, image layers, hits, the class counters, and the workspace left zero), on every case of
tests/elevation_cases.py (tests/test_elevation_host.py holds what the table covers and checks the definition itself), run twice; then
TraversabilityGridMap.add_points / add_depth / update_variance / move_to and the whole callback chain end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_cases as EC  # noqa: E402
import elevation_ref as E  # noqa: E402
import grid_map_cases as GC  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402
from wild_visual_navigation_amd.grid_map import SmartCarrot, TraversabilityGridMap  # noqa: E402
from wild_visual_navigation_amd.image_projector import ImageProjector  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = EC.cases()


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _run(c, dev, workspace=None, points=None, poses=None, counts="case", z_ref="case"):
    """One callback of case ``c`` on the device -> (elevation, variance, layers, hits, stats dict, workspace)."""
    state = [torch.from_numpy(c[k].copy()).to(dev) for k in ("elevation", "variance")]
    layers = [torch.from_numpy(l.copy()).to(dev) for l in c["layers"]]
    hits = torch.from_numpy(c["hits"].copy()).to(dev)
    workspace = ops.grid_elevation_workspace(c["N"], dev) if workspace is None else workspace
    z_ref = c["z_ref"] if isinstance(z_ref, str) else z_ref
    kw = dict(z_ref=None if z_ref is None else float(z_ref), clear_rays=c["clear_rays"], params=ops.grid_elevation_params(
        **{k: v for k, v in c["params"].items() if k != "time_variance"}), workspace=workspace)
    poses = torch.from_numpy(c["poses"] if poses is None else poses).to(dev)
    if c["kind"] == "depth":
        stats = ops.grid_elevation_depth(torch.from_numpy(c["depth"]).to(dev), torch.from_numpy(c["intrinsics"]).to(dev), poses, state[0],
                                         state[1], layers, hits, c["center"], c["resolution"], **kw)
    else:
        counts = c["counts"] if isinstance(counts, str) else counts
        stats = ops.grid_elevation_points(torch.from_numpy(c["points"] if points is None else points).to(dev), poses, state[0], state[1],
                                          layers, hits, c["center"], c["resolution"],
                                          counts=None if counts is None else torch.from_numpy(counts).to(dev), **kw)
    return state[0], state[1], layers, hits, dict(zip(_lib.GRID_ELEVATION_STATS, stats.tolist())), workspace


def _assert_is_reference(got, want, what=""):
    h, var, layers, hits, stats, ws = got
    assert stats == want[4], (what, stats, want[4])
    for name, a, b in (("elevation", h, want[0]), ("variance", var, want[1]), ("hits", hits, want[3])):
        diff = int((_bits(a) != _bits(b)).sum())
        assert a.cpu().numpy().dtype == b.dtype and diff == 0, f"{what}{name}: {diff} cells differ"
    for k, layer in enumerate(layers):
        assert int((_bits(layer) != _bits(want[2][k])).sum()) == 0, f"{what}layer {k}"
    assert int(torch.count_nonzero(ws)) == 0, f"{what}the workspace is not left zero"


# -------------------------------------------------------------------------------------------------- every case, bit for bit, twice
@pytest.mark.parametrize("name", list(CASES))
def test_elevation_is_the_reference_bit_for_bit(dev, name):
    """Shapes (N in {8, 33, 200} x P in {1, 63, 64, 65, 1000}; depth 8 x 8, 17 x 31, 64 x 48 in fp32 and uint16), contention (65 536
    points in one cell at the largest wq and |zq|), every rejection class with its counter, the gate, ray clearing.  The second run
    reuses the first one's workspace: the same bits again, so the kernels left it zero and nothing depends on arrival order."""
    c = CASES[name]
    want = EC.reference(name)
    first = _run(c, dev)
    _assert_is_reference(first, want, "first run: ")
    _assert_is_reference(_run(c, dev, workspace=first[5]), want, "second run: ")


def test_contention_lands_in_one_cell(dev):
    c = CASES["contention_unknown"]
    h, var, _, _, stats, _ = _run(c, dev)
    assert stats["inliers"] == 65536 and int(torch.isfinite(h).sum()) == 1
    assert h[4, 4].item() == -0.03125 and var[4, 4].item() == np.float32(256.0 / (65536 * (2 ** 20 - 1)))


# ----------------------------------------------------------------------------------------------------------------------- order
def test_a_permutation_of_points_or_of_sensors_gives_identical_bits(dev):
    c = CASES["order"]
    want = EC.reference("order")
    rng = np.random.default_rng(17)
    z_ref = float(E.default_z_ref(c["poses"]))
    shuffled = np.stack([p[rng.permutation(p.shape[0])] for p in c["points"]])
    _assert_is_reference(_run(c, dev, points=shuffled), want, "points permuted: ")
    for sensors in ([2, 0, 1], [1, 2, 0]):
        got = _run(c, dev, points=np.ascontiguousarray(shuffled[sensors]), poses=np.ascontiguousarray(c["poses"][sensors]), z_ref=z_ref)
        _assert_is_reference(got, want, f"sensors {sensors}: ")


# ---------------------------------------------------------------------------------------------------- gate, rejection, clearing
def test_a_cell_with_only_outliers_keeps_its_elevation_bits(dev):
    c = CASES["gate"]
    sums = EC.reference("gate")[5]
    only_out = (sums["n"] == 0) & (sums["n_out"] > 0)
    h, var, _, _, stats, _ = _run(c, dev)
    assert only_out.sum() > 0 and stats["gated"] == int(sums["n_out"].sum())
    assert np.array_equal(_bits(h)[only_out], _bits(c["elevation"])[only_out])
    want = (c["variance"][only_out].astype(np.float64) + np.float64(np.float32(0.01)) * sums["n_out"][only_out]).astype(np.float32)
    assert np.array_equal(var.cpu().numpy()[only_out], want)


def test_every_rejection_class_is_counted(dev):
    stats = _run(CASES["rejection_classes"], dev)[4]
    assert stats == dict(invalid=3, near=2, high=2, ramp=3, outside=6, gated=3, unrepresentable=0, inliers=11)
    stats = _run(CASES["rejection_unrepresentable"], dev)[4]
    assert stats["unrepresentable"] == 11 and stats["inliers"] == 0
    c = CASES["depth_17x31_f32"]
    d = c["depth"]
    assert _run(c, dev)[4]["invalid"] == int((~np.isfinite(d) | (d == 0)).sum()) > 0


def test_ray_clearing_clears_the_crossed_wall_and_keeps_the_hit_one(dev):
    c = CASES["walls_clear_1"]
    h, var, layers, hits, _, _ = _run(c, dev)
    h, var, hits = h.cpu().numpy(), var.cpu().numpy(), hits.cpu().numpy()
    cleared = np.isnan(h)
    assert cleared.sum() >= 8 and cleared[20, 8:25].sum() == cleared.sum()          # only cells of the near wall
    assert (var[cleared] == 1000.0).all() and (hits[cleared] == 0).all() and all(np.isnan(l.cpu().numpy()[cleared]).all() for l in layers)
    assert np.isfinite(h[26]).all() and (np.abs(h[26, 10:23] - 0.45) < 0.01).all()    # the far wall is crossed too, but hit by inliers
    assert np.array_equal(hits[~cleared], c["hits"][~cleared])
    h0, _, layers0, hits0, _, _ = _run(CASES["walls_clear_0"], dev)                   # clear_rays=False: nothing is cleared
    assert bool(torch.isfinite(h0).all()) and np.array_equal(hits0.cpu().numpy(), c["hits"])
    assert all(np.array_equal(l.cpu().numpy(), c["layers"][k]) for k, l in enumerate(layers0))


# ----------------------------------------------------------------------------------------------------------------- class level
def _ramp_scene(dev):
    """A camera 1 m above a ground that rises along +x (a ramp: 10 cm per metre), looking ahead and down; its depth image of that ramp,
    and a traversability image whose left half is 0.1 and right half 0.9."""
    gm = TraversabilityGridMap(length=8.0, resolution=0.04, device=dev, center=(5.0, -3.0), max_height_range=2.0)
    H, W = 96, 128
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 70.0
    K[0, 2], K[1, 2] = W / 2 - 0.5, H / 2 - 0.5
    T = GC.look_at((5.0 - 0.5, -3.02, 1.0), (5.0 + 2.0, -3.02, 0.2))
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1) @ T[:3, :3].astype(np.float64).T
    t = T[:3, 3].astype(np.float64)
    # the ramp z = 0.1 (x - 4.5): t_z + s d_z = 0.1 (t_x + s d_x - 4.5)
    with np.errstate(all="ignore"):
        s = (0.1 * (t[0] - 4.5) - t[2]) / (d[..., 2] - 0.1 * d[..., 0])
    depth = np.where((s > 0) & (s < 12.0), s, 0.0).astype(np.float32)
    trav = torch.full((H, W), 0.9)
    trav[:, :W // 2] = 0.1
    conf = torch.full((H, W), 0.75)
    Kt = torch.from_numpy(K)[None].to(dev)
    return gm, torch.from_numpy(depth).to(dev), Kt, torch.from_numpy(T).to(dev), ImageProjector(Kt, H, W), trav.to(dev), conf.to(dev)


def test_callback_chain_end_to_end_without_host_synchronisation(dev):
    """add_depth -> fuse_prediction -> sdf -> SmartCarrot.goal on the ramp scene; the second round runs under
    torch.cuda.set_sync_debug_mode("error") (the first loads the library and warms the allocator); results are read afterwards."""
    gm, depth, K, pose, projector, trav, conf = _ramp_scene(dev)
    carrot = SmartCarrot(distance_force_factor=0.1, center_force_factor=0.001)

    def callback():
        gm.add_depth(depth, K, pose, clear_rays=True)
        gm.update_variance()
        gm.fuse_prediction(trav, conf, projector, pose)
        gm.sdf()
        return carrot.goal(gm, 0.0)

    callback()
    torch.cuda.synchronize()
    first = gm["elevation"].clone()
    torch.cuda.set_sync_debug_mode("error")
    try:
        goal = callback()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert goal.cell.is_cuda and goal.found
    elev, var = gm["elevation"].cpu().numpy(), gm["variance"].cpu().numpy()
    known = np.isfinite(elev)
    N = gm.N
    x = 5.0 + (np.arange(N) - N / 2) * 0.04
    want = np.broadcast_to((0.1 * (x - 4.5))[:, None], (N, N))
    assert known.sum() > 3000 and np.abs(elev - want)[known].max() < 0.02            # the ramp, within half a cell's rise + rounding
    assert (var[known] < 100.0).all() and np.median(var[known]) < 1.0 and (var[~known] == 1000.0).all()
    assert known[torch.isfinite(first).cpu().numpy()].all()
    stats = gm.elevation_stats
    assert sum(stats.values()) == depth.numel() and stats["inliers"] > 5000 and stats["invalid"] == int((depth == 0).sum())
    i, j = goal.index
    t = gm["visual_traversability"].cpu().numpy()
    assert known[i, j] and t[i, j] == np.float32(0.9) and gm["sdf"][i, j].item() > 0
    assert (gm["hits"].cpu().numpy()[known] > 0).sum() > 2000 and (gm["hits"].cpu().numpy()[~known] == 0).all()


def test_grid_map_add_points_is_the_reference_and_move_to_carries_variance(dev):
    c = CASES["shape_n33_p1000"]
    gm = TraversabilityGridMap(length=c["N"] * c["resolution"], resolution=c["resolution"], device=dev, center=c["center"])
    assert gm.N == c["N"] and "variance" in gm and (gm["variance"] == 1000.0).all()
    gm.add_points(torch.from_numpy(c["points"]).to(dev), torch.from_numpy(c["poses"]).to(dev), counts=torch.from_numpy(c["counts"]).to(dev))
    blank = EC.blank(c["N"])
    want = E.add_points(c["points"], c["poses"], *blank, c["center"], c["resolution"], counts=c["counts"])
    assert np.array_equal(_bits(gm["elevation"]), _bits(want[0])) and np.array_equal(_bits(gm["variance"]), _bits(want[1]))
    assert gm.elevation_stats == want[4]
    # update_variance: known cells grow by time_variance, unknown ones keep initial_variance
    gm.update_variance()
    assert np.array_equal(_bits(gm["variance"]), _bits(E.update_variance(want[0], want[1])))
    # move by (3, -2) cells: variance shifts with elevation, vacated cells get initial_variance
    N, r = c["N"], c["resolution"]
    before = {k: gm[k].cpu().numpy() for k in ("elevation", "variance")}
    gm.move_to(c["center"][0] + 3 * r + 0.01, c["center"][1] - 2 * r - 0.01)
    vacated = np.ones((N, N), bool)
    vacated[:N - 3, 2:] = False
    for k, old in before.items():
        new = gm[k].cpu().numpy()
        assert np.array_equal(new[:N - 3, 2:], old[3:, :N - 2], equal_nan=True), k
    assert np.isnan(gm["elevation"].cpu().numpy()[vacated]).all() and (gm["variance"].cpu().numpy()[vacated] == 1000.0).all()
    # a second cloud onto the moved map: the reference on the moved layers
    c2 = CASES["shape_n33_p65"]
    moved = (gm["elevation"].cpu().numpy(), gm["variance"].cpu().numpy(), blank[2], blank[3])
    want2 = E.add_points(c2["points"], c2["poses"], *moved, gm.center, r, counts=c2["counts"])
    gm.add_points(torch.from_numpy(c2["points"]).to(dev), torch.from_numpy(c2["poses"]).to(dev), counts=torch.from_numpy(c2["counts"]).to(dev))
    assert np.array_equal(_bits(gm["elevation"]), _bits(want2[0])) and np.array_equal(_bits(gm["variance"]), _bits(want2[1]))


def test_set_elevation_route_is_unchanged_and_sets_variance(dev):
    """The layers the existing route gave (tests/test_gpu_grid_map.py holds them to the fusion reference) plus the variance layer."""
    gm = TraversabilityGridMap(length=8 * 0.5, resolution=0.5, device=dev)
    elev = torch.zeros(8, 8)
    elev[2, 3] = float("nan")
    elev[5, 5] = 0.7
    gm.set_elevation(elev)
    assert np.array_equal(gm["elevation"].cpu().numpy(), elev.numpy(), equal_nan=True)
    var = gm["variance"].cpu().numpy()
    assert var[2, 3] == 1000.0 and (np.delete(var.ravel(), 2 * 8 + 3) == 100.0).all()          # initial_variance clamped to max_variance
    gm.set_elevation(elev, variance=0.04)
    var = gm["variance"].cpu().numpy()
    assert var[2, 3] == 1000.0 and (np.delete(var.ravel(), 2 * 8 + 3) == np.float32(0.04)).all()
    assert all(np.isnan(gm[k].cpu().numpy()).all() for k in ("visual_traversability", "visual_confidence", "sdf")) and not gm["hits"].any()
    # a supplied layer with its variance is a prior like any other: one point on the known cell (5, 5), one on the unknown (2, 3)
    pts = torch.tensor([[[0.5 - 0.25, 0.5 - 0.25, 0.75 - 1.5], [-1.0 - 0.25, -0.5 - 0.25, 0.1 - 1.5]]])     # q = p + t: cell centres
    pose = torch.eye(4)[None].clone()
    pose[0, :3, 3] = torch.tensor([0.25, 0.25, 1.5])
    gm.add_points(pts.to(dev), pose.to(dev))
    want = E.add_points(pts.numpy(), pose.numpy(), elev.numpy(), np.where(np.isnan(elev.numpy()), 1000.0, 0.04).astype(np.float32),
                        np.full((2, 8, 8), np.nan, np.float32), np.zeros((8, 8), np.int32), (0.0, 0.0), 0.5)
    assert want[4]["inliers"] == 2 and np.array_equal(_bits(gm["elevation"]), _bits(want[0])) and np.array_equal(_bits(gm["variance"]), _bits(want[1]))
    assert 0.7 < gm["elevation"][5, 5].item() < 0.75 and abs(gm["elevation"][2, 3].item() - 0.1) < 1e-4
