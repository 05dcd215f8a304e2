"""The supervision rasteriser (csrc/supervision.hip, project_render_fmin_kernel) on the GPU at the edges of its loops and branches, bit
for bit against the CPU oracle (oracle/supervision.py): every case of tests/supervision_cases.py, whose coverage claims
tests/test_supervision_host.py holds on the oracle.  Masks are compared as int32 words: a pixel outside the polygon keeps its exact
bits, NaN payload included.

Which cases exist for which loop or branch of the kernel (one 256-thread workgroup per node, four waves of 64 lanes):
  projection loop  `for (i = tid; i < N; i += 256)`: N = 2 (segment_n2), N < 256 (most), N = 1000 (camera_*_1000: four trips),
      N = 7743 (lds_7743: 31 trips); `pts_batched`: test_batched_points and the ImageProjector test ([B, N, 3]); `projected` / `depth`
      written for every node (test_batched_points, ImageProjector) or null (all other calls); behind the camera -> NaN vertex:
      all_behind, camera_standing_on_it_*; NaN / infinite input: nan_vertex, v_inf_vertex
  closing rule (thread 0): first vertex appended (every open polygon) or not (quad_closed, one_pixel: last vertex allclose to first)
  scan loop  `for (y = tid; y < H; y += 256)`: one trip (H = 1 and 4), second trip at H = 257 (rectangles straddling row 256, the
      last row alone), at H = 300 and at H = 448 (ellipses, cameras), third trip at H = 513 (rectangles straddling row 512);
      edge activity and dx clamp: exactly horizontal edges (integer rectangles, camera_pitched_40), none (camera_rolled_40),
      vertical edges, duplicate vertices (dx = 0 / 1e-12), collinear points; poisoned rows: v_inf_vertex
  row range: no active edge (rows above / below every polygon), x_left > W - 1 (rect 500..600, camera_beside_*, x_plus_3e9, x_plus_2p31,
      hair_in_front: bounds past 2^31), x_right < 0 (rect -1..-1, x_minus_3e9, x_minus_2p31), both clamps at once (x_span_6e9, the whole
      frame), xa / xb on integer pixels (integer rectangles: the closed x_left <= x <= x_right comparison on both ends)
  fill loop  `for (x = xa + lane; x <= xb; x += 64)`: W < 64 (513 x 40, 4 x 40, 1 x 1: idle lanes), second trip at W = 65 (column 64),
      W = 500 and 448 (eight and seven trips); `for (y = wave; y < H; y += 4)`: every H above; C = 1, 2, 3
  merge: fmin with NaN (payloads), values on both sides of `value`, `value` itself, +-inf; value as a float and from device memory;
      value = NaN leaves the mask as it is
  launcher: the LDS bound at 448 rows (N = 7743 renders, N = 7744 is refused), non-contiguous and unequal masks refused"""
import numpy as np
import pytest
import torch

import supervision_cases as SC
from oracle import supervision as OSV
from wild_visual_navigation_amd import _lib, ops
from wild_visual_navigation_amd.image_projector import ImageProjector

pytestmark = pytest.mark.gpu

GROUPS = sorted({(c.family, c.shape) for c in SC.all_cases() if c.family != "lds"})


def _words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _render(dev, Ks, poses, masks, points, value, value_on_device=False, want_projected=False):
    """ops.project_render_fmin on copies of the numpy start masks -> (masks after, projected, depth) as numpy."""
    m = [_t(x, dev) for x in masks]
    v = torch.tensor([value], dtype=torch.float32, device=dev) if value_on_device else value
    out = ops.project_render_fmin([_t(k, dev) for k in Ks], [_t(p, dev) for p in poses], m, _t(points, dev), v, want_projected=want_projected)
    got = [x.cpu().numpy() for x in m]
    return (got, out[0].cpu().numpy(), out[1].cpu().numpy()) if want_projected else (got, None, None)


def _oracle(mask, K, pose, pts, value):
    with np.errstate(all="ignore"):
        return OSV.render_fmin(mask, K, pose, pts, value)


@pytest.mark.parametrize("family,shape", GROUPS, ids=[f"{f}-{s[0]}x{s[1]}x{s[2]}" for f, s in GROUPS])
def test_every_case_matches_the_oracle_bit_for_bit(dev, family, shape):
    cases = [c for c in SC.family(family) if c.shape == shape]
    assert cases
    starts = {kind: SC.start_mask(shape, kind) for kind in ("nan", "mix")}
    differing = 0
    for c in cases:
        for kind, start in starts.items():
            want = _words(_oracle(start, c.K, c.pose, c.points, SC.VALUE))
            for on_device in (False, True):
                got = _words(_render(dev, [c.K], [c.pose], [start], c.points, SC.VALUE, value_on_device=on_device)[0][0])
                bad = int((got != want).sum())
                print(f"{c.name} start={kind} value_on_device={on_device}: {bad} differing words")
                differing += bad
                assert bad == 0, (c.name, kind, on_device)
            if kind == "nan" and c.expect is not None:        # the hand-stated rectangle, without the oracle
                assert np.array_equal(~np.isnan(got.view(np.float32)[0]), SC.rectangle_mask(c.expect, shape[1], shape[2])), c.name
        got = _words(_render(dev, [c.K], [c.pose], [starts["mix"]], c.points, float("nan"))[0][0])        # fmin(old, NaN) = old
        assert np.array_equal(got, _words(starts["mix"])), c.name
    assert differing == 0


def test_batched_points(dev):
    """points [n, N, 3] (the pts_batched branch): three different polygons for three nodes equal the oracle per node and three
    single-node calls; projected and depth equal project_points_raw."""
    cams, pts = SC.three_polygons()
    Ks, poses = [c.K for c in cams], [c.pose for c in cams]
    starts = [SC.start_mask(SC.S_PROD, "mix", seed=i) for i in range(3)]
    got, proj, depth = _render(dev, Ks, poses, starts, pts, SC.VALUE, want_projected=True)
    assert proj.shape == (3, 40, 2) and depth.shape == (3, 40)
    for i in range(3):
        want = _oracle(starts[i], Ks[i], poses[i], pts[i], SC.VALUE)
        assert int((_words(want) != _words(starts[i])).sum()) > 5000                                        # the polygon is in view
        assert np.array_equal(_words(got[i]), _words(want)), i
        single = _render(dev, [Ks[i]], [poses[i]], [starts[i]], pts[i], SC.VALUE)[0][0]
        assert np.array_equal(_words(single), _words(got[i])), i
        with np.errstate(all="ignore"):
            uv, z = OSV.project_points_raw(Ks[i], poses[i], pts[i])
        assert np.array_equal(_words(proj[i]), _words(uv)) and np.array_equal(_words(depth[i]), _words(z)), i
    # the three polygons differ: a node rendered with another node's points is something else
    for i in range(3):
        assert not np.array_equal(_words(_oracle(starts[i], Ks[i], poses[i], pts[(i + 1) % 3], SC.VALUE)), _words(got[i])), i


def test_run_to_run_and_one_call_for_five_nodes(dev):
    """Two runs give the same bytes; one call with five nodes (shared points) equals five calls."""
    names = ("pitched", "rolled", "standing_on_it", "out_bottom_and_side", "beside")
    cams = [SC.by_name(f"camera_{k}_1000") for k in names]
    Ks, poses, pts = [c.K for c in cams], [c.pose for c in cams], cams[0].points
    starts = [SC.start_mask(SC.S_PROD, "mix", seed=10 + i) for i in range(5)]
    a = _render(dev, Ks, poses, starts, pts, SC.VALUE)[0]
    b = _render(dev, Ks, poses, starts, pts, SC.VALUE)[0]
    for i in range(5):
        assert np.array_equal(_words(a[i]), _words(b[i])), i
        single = _render(dev, [Ks[i]], [poses[i]], [starts[i]], pts, SC.VALUE)[0][0]
        assert np.array_equal(_words(single), _words(a[i])), i
        assert np.array_equal(_words(a[i]), _words(_oracle(starts[i], Ks[i], poses[i], pts, SC.VALUE))), i
    assert sum(int((_words(a[i]) != _words(starts[i])).any()) for i in range(5)) >= 4


def test_image_projector_with_two_cameras_and_batched_points(dev):
    """ImageProjector with B = 2 cameras and [2, N, 3] points at 448 x 448: project equals the oracle per element, and
    project_and_render's masks equal fill_mask per element, with a polygon that leaves the frame."""
    cams = [SC.by_name("camera_out_bottom_and_side_40"), SC.by_name("camera_standing_on_it_40")]
    K = torch.from_numpy(np.stack([c.K for c in cams])).to(dev)
    ip = ImageProjector(K, torch.tensor(448), torch.tensor(448))
    assert ip.camera.batch_size == 2
    pose = torch.from_numpy(np.stack([c.pose for c in cams])).to(dev)
    pts = np.stack([cams[0].points, cams[1].points[::-1] + np.array([0.1, 0.05, 0.0], dtype=np.float32)]).astype(np.float32)
    sK = ip.camera.intrinsics.cpu().numpy()
    proj, valid, valid_z = ip.project(pose, torch.from_numpy(pts).to(dev))
    colors = torch.tensor([1.0, 0.5, 0.25])
    masks, _, proj2, valid2 = ip.project_and_render(pose, torch.from_numpy(pts).to(dev), colors)
    assert masks.shape == (2, 3, 448, 448)
    for i in range(2):
        with np.errstate(all="ignore"):
            uv, z = OSV.project_points_raw(sK[i], cams[i].pose, pts[i])
            inside = OSV.fill_mask(OSV.project_points(sK[i], cams[i].pose, pts[i]), 448, 448)
        assert np.array_equal(_words(proj[i].cpu().numpy()), _words(uv)), i
        assert np.array_equal(valid_z[i].cpu().numpy(), z >= 0), i
        want_valid = (z >= 0) & (uv[:, 0] >= 0) & (uv[:, 0] <= 448) & (uv[:, 1] >= 0) & (uv[:, 1] <= 448)
        assert np.array_equal(valid[i].cpu().numpy(), want_valid) and np.array_equal(valid2[i].cpu().numpy(), want_valid), i
        m = masks[i].cpu().numpy()
        assert inside.sum() > 20000 and (inside[-1].any() or inside[:, -1].any())                           # it leaves the frame
        for ch in range(3):
            assert np.array_equal(~np.isnan(m[ch]), inside), (i, ch)
            assert (m[ch][inside] == float(colors[ch])).all(), (i, ch)
        want_p2 = np.where((z >= 0)[:, None], uv, np.float32(np.nan))
        assert np.array_equal(proj2[i].cpu().numpy(), want_p2, equal_nan=True), i
    assert not valid_z[1].all() and valid_z[0].all()                                                        # element 1 stands on its footprint


def test_refusals_that_need_a_gpu_mask(dev):
    """Non-contiguous masks and masks of unequal shape still raise, and nothing is written."""
    eye = torch.eye(4, device=dev)
    pts = torch.from_numpy(SC.by_name("quad_open").points).to(dev)
    base = torch.full((2, 300, 1000), float("nan"), device=dev)
    with pytest.raises(_lib.WvnError, match="contiguous fp32"):
        ops.project_render_fmin([eye], [eye], [base[:, :, ::2]], pts, 0.5)
    good = torch.full((2, 300, 500), float("nan"), device=dev)
    with pytest.raises(_lib.WvnError, match="contiguous fp32"):
        ops.project_render_fmin([eye, eye], [eye, eye], [good, torch.full((2, 300, 499), float("nan"), device=dev)], pts, 0.5)
    with pytest.raises(_lib.WvnError, match="contiguous fp32"):
        ops.project_render_fmin([eye], [eye], [good.double()], pts, 0.5)
    assert torch.isnan(base).all() and torch.isnan(good).all()


def test_lds_bound(dev):
    """The launcher accepts N <= 8191 - H points (7743 at 448 rows: 64 KB of dynamic LDS): that many render and equal the oracle,
    one more is refused as a bad argument and the mask is untouched."""
    ok, over = SC.family("lds")
    assert len(ok.points) == SC.LDS_MAX_N == 7743 and len(over.points) == 7744
    start = SC.start_mask(ok.shape, "mix")
    got = _render(dev, [ok.K], [ok.pose], [start], ok.points, SC.VALUE)[0][0]
    want = _oracle(start, ok.K, ok.pose, ok.points, SC.VALUE)
    assert int((_words(want) != _words(start)).sum()) > 30000
    assert np.array_equal(_words(got), _words(want))
    m = _t(start, dev)
    with pytest.raises(_lib.WvnError, match="bad argument"):
        ops.project_render_fmin([_t(over.K, dev)], [_t(over.pose, dev)], [m], _t(over.points, dev), SC.VALUE)
    assert np.array_equal(_words(m.cpu().numpy()), _words(start))
