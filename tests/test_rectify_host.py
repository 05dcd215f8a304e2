"""The raw camera ingest without a GPU: tests/rectify_ref.py (the definition ops.unpack_frames / ops.rectify are held to) against
independent statements -- constant and linear pictures through the demosaic, a scalar re-statement of the map in `math`,
scipy.ndimage.map_coordinates for the sampling -- the coverage claims of the maps tests/test_gpu_rectify.py uses, and every refusal of
the Python surface and the C-ABI that happens before a device is touched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_cases as RC  # noqa: E402
import rectify_ref as R  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402
from wild_visual_navigation_amd.utils import image_io  # noqa: E402

PATTERNS = tuple(R.BAYER)
H, W = RC.SRC


# ------------------------------------------------------------------------------------------------------------------ demosaic
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("size", [(3, 3), (4, 6), (7, 5)])
def test_a_constant_colour_survives_the_demosaic(pattern, size):
    for colour in ((200, 30, 90), (0, 255, 1), (255, 255, 255)):
        rgb = np.broadcast_to(np.array(colour, dtype=np.uint8)[:, None, None], (3,) + size)
        assert np.array_equal(R.demosaic(RC.mosaic_of(rgb, pattern), pattern), rgb), colour


@pytest.mark.parametrize("pattern", PATTERNS)
def test_linear_planes_with_even_slopes_are_exact_on_the_interior(pattern):
    """Planes 2a x + 2b y + c: every average of the rule is over points symmetric about the site, and the even slopes keep it whole."""
    for (h, w) in ((7, 5), (9, 12)):
        yy, xx = np.mgrid[0:h, 0:w]
        rgb = np.stack([2 * 3 * xx + 2 * 5 * yy + 10, 2 * 2 * xx + 2 * 1 * yy + 3, 2 * 1 * xx + 2 * 4 * yy + 7]).astype(np.uint8)
        assert rgb.max() < 255
        got = R.demosaic(RC.mosaic_of(rgb, pattern), pattern)
        assert np.array_equal(got[:, 1:-1, 1:-1], rgb[:, 1:-1, 1:-1])


@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_ring_and_the_array_form(pattern):
    rng = np.random.default_rng(5)
    for (h, w) in ((3, 3), (4, 6), (7, 5), (33, 47)):
        raw = rng.integers(0, 256, (h, w), dtype=np.uint8)
        out = R.demosaic(raw, pattern)
        assert np.array_equal(out, R.demosaic_scalar(raw, pattern))
        assert np.array_equal(out[:, 1:-1, 0], out[:, 1:-1, 1]) and np.array_equal(out[:, 1:-1, w - 1], out[:, 1:-1, w - 2])
        assert np.array_equal(out[:, 0, :], out[:, 1, :]) and np.array_equal(out[:, h - 1, :], out[:, h - 2, :])
        assert np.array_equal(out[:, 0, 0], out[:, 1, 1]) and np.array_equal(out[:, h - 1, w - 1], out[:, h - 2, w - 2])
        # an R / B site keeps its byte, a G site too
        ry, rx = R.BAYER[pattern]
        yy, xx = np.mgrid[1:h - 1, 1:w - 1]
        red_row = (yy & 1) == ry
        own = ((xx & 1) == rx) == red_row
        site = np.where(own, np.where(red_row, 0, 2), 1)
        assert np.array_equal(np.take_along_axis(out[:, 1:-1, 1:-1], site[None], 0)[0], raw[1:-1, 1:-1])


def test_unpack_of_the_plain_kinds():
    data, step = RC.source_frames("rgb8", 1, 4, 6, pad=5)
    rows = R.rows_of(data[0], "rgb8", 4, 6, step)
    assert np.array_equal(R.unpack(data[0], "rgb8", 4, 6, step), rows.reshape(4, 6, 3).transpose(2, 0, 1))
    assert np.array_equal(R.unpack(data[0], "bgr8", 4, 6, step), R.unpack(data[0], "rgb8", 4, 6, step)[::-1])
    assert np.array_equal(R.unpack(data[0], "rgb8", 4, 6, step, bgr=True), R.unpack(data[0], "bgr8", 4, 6, step))
    mono, step = RC.source_frames("mono8", 1, 7, 5, pad=5)
    assert R.unpack(mono[0], "mono8", 7, 5, step).shape == (1, 7, 5) and R.unpack(mono[0], "mono8", 7, 5, step, channels=3).shape == (3, 7, 5)


# ----------------------------------------------------------------------------------------------------------------------- map
def _rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


@pytest.mark.parametrize("case", ["hoengg", "hoengg_half_rotated", "plumb_bob", "plumb_bob_four"])
def test_the_map_agrees_with_a_scalar_restatement(case):
    K = R.hoengg(W, H)
    if case == "hoengg":
        args = (K, R.HOENGG_D, "equidistant", (H, W), K, None)
    elif case == "hoengg_half_rotated":
        args = (K, R.HOENGG_D, "equidistant", (H, W), RC.halved(K), _rot(0.05, -0.1))
    elif case == "plumb_bob":
        args = (RC.plumb_bob_K(H, W), RC.PLUMB_BOB_D[:4] + (0.013,), "plumb_bob", (H, W), RC.plumb_bob_K(H, W), _rot(-0.02, 0.03))
    else:
        args = (RC.plumb_bob_K(H, W), RC.PLUMB_BOB_D[:4], "plumb_bob", (H, W), RC.plumb_bob_K(H, W), None)
    Kc, D, model, src, Kn, Rm = args
    qx, qy = R.rectify_map(Kc, D, model, src, src, Kn, Rm)
    assert qx.dtype == np.int32 and qx.shape == (H, W)
    for v in range(H):
        for u in range(W):
            assert (qx[v, u], qy[v, u]) == R.map_point(Kc, list(D), model, src, Kn, Rm, u, v), (u, v)
    # the package computes the same integers (ops.rectify_map's host half)
    Dv = list(D) + [0.0] if model == "plumb_bob" and len(D) == 4 else list(D)
    px, py = ops._rectify_map_host(np.asarray(Kc), Dv, model, src, src, np.asarray(Kn), np.eye(3) if Rm is None else Rm)
    assert np.array_equal(px, qx) and np.array_equal(py, qy)


def test_no_distortion_and_the_same_matrix_is_the_identity_map():
    # (plumb_bob: with D = 0 the equidistant model is still the ideal fisheye, r -> atan r, not the identity)
    for K, model, D in ((R.hoengg(W, H), "plumb_bob", (0, 0, 0, 0)), (RC.plumb_bob_K(H, W), "plumb_bob", (0, 0, 0, 0, 0))):
        qx, qy = R.rectify_map(K, D, model, (H, W), None, K)
        u, v = np.meshgrid(np.arange(W), np.arange(H))
        assert np.array_equal(qx, 32 * u) and np.array_equal(qy, 32 * v)
    qx, qy = R.rectify_map(K, D, model, (H, W))          # the default new_K at the source size is K
    assert np.array_equal(qx, 32 * u) and np.array_equal(qy, 32 * v)


def test_non_finite_and_overflowing_coordinates_land_on_the_sentinel():
    K = R.hoengg(W, H)
    qx, qy = R.rectify_map(K, (float("nan"), 0, 0, 0), "equidistant", (H, W))
    assert (qx == -64).sum() >= H * W - 1 and (qy == -64).sum() >= H * W - 1     # (the principal point itself may have r = 0)
    qx, qy = R.rectify_map(K, (1e308, 1e308, 0, 0, 1e308), "plumb_bob", (H, W))   # r2 k overflows: +-inf, or inf - inf = NaN
    assert ((qx == -64) | (qx == 32 * (W + 1)) | (np.abs(qx - 32 * K[0, 2]) < 64)).all()
    assert ((qx == -64).sum() + (qx == 32 * (W + 1)).sum()) > H * W - 40
    # a ray parallel to the image plane (Z = 0 after the rotation): x = inf, atan = pi / 2, td / r = 0, inf * 0 = NaN
    Rm = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    qx, qy = R.rectify_map(K, R.HOENGG_D, "equidistant", (H, W), (3, 3), np.eye(3), Rm)     # Z = u: column 0 has Z = 0
    assert (qx[:, 0] == -64).all() and (qy[:, 0] == -64).all()
    for q, lim in ((qx, W), (qy, H)):
        assert q.min() >= -64 and q.max() <= 32 * (lim + 1)
    full, part, none = R.tap_classes(np.full((2, 2), -64, np.int32), np.full((2, 2), -64, np.int32), H, W)
    assert none.all()


# ------------------------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("name", ["K", "half", "plumb_bob"])
def test_sampling_against_scipy(name):
    from scipy.ndimage import map_coordinates

    qx, qy = R.rectify_map(**RC.camera_maps()[name][0])
    data, step = RC.source_frames("planar", 1, H, W)
    planes = R.unpack(data[0], "planar", H, W, step)
    got = R.sample(planes, qx, qy).astype(np.float64)
    for c in range(3):
        exact = map_coordinates(planes[c].astype(np.float64), [qy / 32.0, qx / 32.0], order=1, mode="grid-constant", cval=0.0)
        assert np.abs(got[c] - exact).max() <= 0.5 + 1e-6
    ones = R.sample(np.full((1, H, W), 255, np.uint8), np.full((4, 4), 31 + 32 * 3, np.int32), np.full((4, 4), 31 + 32 * 5, np.int32))
    assert (ones == 255).all()                                      # the weights sum to 1024: no overflow, no loss


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_the_maps_cover_the_tap_classes_they_claim():
    counts = {}
    for name, (args, claims) in RC.camera_maps().items():
        qx, qy = R.rectify_map(**args)
        full, part, none = (int(m.sum()) for m in R.tap_classes(qx, qy, H, W))
        counts[name] = (full, part, none)
        for cls, n in zip(("full", "partial", "none"), (full, part, none)):
            if cls in claims:
                assert n >= RC.MIN_CLASS, (name, cls, n)
    # 47 x 33: 90.6 % / 9.4 % / none with K_new = K; 23.5 % / 2.8 % / 73.8 % with its focal lengths halved
    assert counts["K"] == (1405, 146, 0) and counts["half"] == (364, 43, 1144)
    assert counts["K_28x20"] == (519, 41, 0) and counts["half_28x20"] == (130, 13, 417)
    assert counts["plumb_bob"][0] == H * W
    # 40 x 30: 89.6 % / 10.4 %, and 22.2 % / 5.2 % / 72.7 %
    m = RC.camera_maps(30, 40)
    c40 = {n: tuple(int(x.sum()) for x in R.tap_classes(*R.rectify_map(**m[n][0]), 30, 40)) for n in ("K", "half")}
    assert c40 == {"K": (1075, 125, 0), "half": (266, 62, 872)}
    # the full-size case: the real camera, centre crop to 448 x 448
    K = R.hoengg(1440, 1080)
    qx, qy = R.rectify_map(K, R.HOENGG_D, "equidistant", R.HOENGG_SIZE, (448, 448), RC.crop_448(K))
    assert tuple(int(x.sum()) for x in R.tap_classes(qx, qy, 1080, 1440)) == (200037, 379, 288)


# ------------------------------------------------------------------------------------------------------------ Python surface
def test_image_plan_channel_orders():
    P = image_io.image_plan
    assert P("mono8") == (3, False) and P("mono8", "bgr8") == (3, True) and P("mono8", "passthrough") == (1, False)
    assert P("rgb8") == (3, False) and P("rgb8", "bgr8") == (3, True) and P("rgb8", "passthrough") == (3, False)
    assert P("bgr8") == (3, False) and P("bgr8", "bgr8") == (3, True) and P("bgr8", "passthrough") == (3, True)
    for b in PATTERNS:
        assert P(b) == (3, False) and P(b, "bgr8") == (3, True) and P(b, "passthrough") == (3, False)


@pytest.mark.parametrize("encoding", ["mono16", "rgb16", "bgr16", "rgba8", "bgra8", "rgba16", "32FC1", "16UC1", "8UC3", "bayer_rggb16",
                                      "bayer_gbrg16", "yuv422", "planar", ""])
def test_encodings_that_are_refused_by_name(encoding):
    with pytest.raises(_lib.WvnError, match=repr(encoding)):
        image_io.image_to_torch(b"\0" * 64, encoding, 4, 4, device="cpu")
    with pytest.raises(_lib.WvnError, match=repr(encoding)):
        image_io.check_raw_geometry(encoding, 4, 4, who="decode_raw")


def test_image_to_torch_refuses_before_anything_runs():
    I2T = image_io.image_to_torch
    with pytest.raises(_lib.WvnError, match="desired_encoding 'mono8'"):
        I2T(b"\0" * 16, "mono8", 4, 4, desired_encoding="mono8")
    with pytest.raises(_lib.WvnError, match="step=11"):
        I2T(b"\0" * 64, "rgb8", 4, 4, step=11)
    with pytest.raises(_lib.WvnError, match="step=3"):
        I2T(b"\0" * 64, "bayer_gbrg8", 4, 4, step=3)
    with pytest.raises(_lib.WvnError, match="2 x 4"):
        I2T(b"\0" * 64, "bayer_gbrg8", 2, 4)
    with pytest.raises(_lib.WvnError, match="0 x 4"):
        I2T(b"\0" * 64, "mono8", 0, 4)
    with pytest.raises(_lib.WvnError, match="31 bits"):
        I2T(b"\0" * 64, "mono8", 65535, 65535)
    with pytest.raises(_lib.WvnError, match="holds 15 bytes"):
        I2T(b"\0" * 15, "mono8", 4, 4)
    with pytest.raises(_lib.WvnError, match="RectifyMap"):
        I2T(b"\0" * 16, "mono8", 4, 4, rectify=(1, 2))
    m = ops.RectifyMap(torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32), (5, 4), (2, 2), np.eye(3))
    with pytest.raises(_lib.WvnError, match="5 x 4"):
        I2T(b"\0" * 16, "mono8", 4, 4, rectify=m)
    with pytest.raises(_lib.WvnError, match="no CPU fallback"):           # everything is in order, but there is no GPU to run on
        I2T(b"\0" * 16, "mono8", 4, 4, device="cpu")
    assert m.K_tensor.shape == (1, 4, 4) and m.K_tensor.dtype == torch.float32 and torch.equal(m.K_tensor[0], torch.eye(4))


def test_rectify_map_refusals():
    K = R.hoengg(W, H)
    with pytest.raises(_lib.WvnError, match="'rational_polynomial'"):
        ops.rectify_map(K, [0.0] * 8, "rational_polynomial", (H, W))
    with pytest.raises(_lib.WvnError, match="'thin_prism'"):
        ops.rectify_map_from_camera_info(H, W, "thin_prism", [0.1] * 12, K.ravel(), [], [0.0] * 12)
    with pytest.raises(_lib.WvnError, match="'fisheye'"):
        ops.rectify_map_from_camera_info(H, W, "fisheye", [0.0] * 4, K.ravel(), [], [0.0] * 12)
    with pytest.raises(_lib.WvnError, match="equidistant takes 4"):
        ops.rectify_map(K, [0.1] * 5, "equidistant", (H, W))
    with pytest.raises(_lib.WvnError, match="plumb_bob takes 4 or 5"):
        ops.rectify_map(K, [0.1] * 3, "plumb_bob", (H, W))
    with pytest.raises(_lib.WvnError, match="finite"):
        ops.rectify_map(K, [float("nan")] * 4, "equidistant", (H, W))
    with pytest.raises(_lib.WvnError, match="src_size"):
        ops.rectify_map(K, R.HOENGG_D, "equidistant", (0, W))
    with pytest.raises(_lib.WvnError, match="out_size"):
        ops.rectify_map(K, R.HOENGG_D, "equidistant", (H, W), (70000, 4))
    with pytest.raises(_lib.WvnError, match="K must hold 9"):
        ops.rectify_map(K[:2], R.HOENGG_D, "equidistant", (H, W))
    with pytest.raises(_lib.WvnError, match="singular"):
        ops.rectify_map(K, R.HOENGG_D, "equidistant", (H, W), new_K=np.zeros((3, 3)))
    with pytest.raises(_lib.WvnError, match="P must hold 12"):
        ops.rectify_map_from_camera_info(H, W, "equidistant", R.HOENGG_D, K.ravel(), [], [0.0] * 9)
    with pytest.raises(_lib.WvnError, match="no CPU fallback"):
        ops.rectify_map(K, R.HOENGG_D, "equidistant", (H, W), device="cpu")


def test_ops_refuse_bad_frames_before_the_device():
    z = torch.zeros
    with pytest.raises(_lib.WvnError, match="'bayer_rggb16'"):
        ops.unpack_frames(z(4, 4, dtype=torch.uint8), "bayer_rggb16")
    with pytest.raises(_lib.WvnError, match="uint8"):
        ops.unpack_frames(z(4, 4), "mono8")
    with pytest.raises(_lib.WvnError, match=r"\[B,H,W,3\]"):
        ops.unpack_frames(z(4, 4, dtype=torch.uint8), "rgb8")
    with pytest.raises(_lib.WvnError, match=r"\[B,3,H,W\]"):
        ops.unpack_frames(z(1, 4, 4, 3, dtype=torch.uint8), "planar")
    with pytest.raises(_lib.WvnError, match="H, W >= 3"):
        ops.unpack_frames(z(2, 5, dtype=torch.uint8), "bayer_grbg8")
    with pytest.raises(_lib.WvnError, match="step=5 is smaller"):
        ops.unpack_frames(z(1, 4, 5, dtype=torch.uint8), "rgb8", step=5, width=2)
    with pytest.raises(_lib.WvnError, match="step needs width"):
        ops.unpack_frames(z(1, 4, 5, dtype=torch.uint8), "mono8", step=5)
    with pytest.raises(_lib.WvnError, match="rows of 5 bytes"):
        ops.unpack_frames(z(1, 4, 5, dtype=torch.uint8), "mono8", step=6, width=4)
    with pytest.raises(_lib.WvnError, match="channels=1"):
        ops.unpack_frames(z(4, 4, 3, dtype=torch.uint8), "rgb8", channels=1)
    with pytest.raises(_lib.WvnError, match="not one of rggb"):
        ops.debayer(z(4, 4, dtype=torch.uint8), "rgbg")
    with pytest.raises(_lib.WvnError, match="no CPU fallback"):
        ops.debayer(z(4, 4, dtype=torch.uint8), "rggb")
    m = ops.RectifyMap(z(2, 2, dtype=torch.int32), z(2, 2, dtype=torch.int32), (4, 4), (2, 2), np.eye(3))
    with pytest.raises(_lib.WvnError, match="RectifyMap"):
        ops.rectify(z(3, 4, 4, dtype=torch.uint8), None)
    with pytest.raises(_lib.WvnError, match="route"):
        ops.rectify(z(3, 4, 4, dtype=torch.uint8), m, route="fast")
    with pytest.raises(_lib.WvnError, match="no CPU fallback"):
        ops.rectify(z(3, 4, 4, dtype=torch.uint8), m)


def test_the_c_abi_refuses_before_any_launch():
    """Return codes only: no GPU is needed to see WVN_ERR_ARG, and the buffers of a refused call are never touched."""
    calls = RC.abi_refusals(_lib.lib())
    assert len(calls) >= 40
    for what, rc in calls:
        assert rc == _lib.ERR_ARG, what


# ------------------------------------------------------------------------------------------- sanitizer run of the kernels' code
def test_the_kernels_run_clean_on_the_host_under_the_sanitizers(tmp_path):
    """tests/rectify_host_main.cpp compiles csrc/rectify.hip as plain C++ (every thread in turn) with -fsanitize=address,undefined:
    every kind through unpack and through maps that cover the three tap classes, a short row tail, arbitrary int32 entries and
    coordinates far outside, on buffers of exactly the stated size (frame stride = the bytes of a frame without the last row's
    padding).  The outputs are the definition's, and no byte outside a buffer is touched.  A stand-alone program: nothing is loaded
    into Python."""
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ / clang++ / c++): the sanitizer run of the kernels cannot be skipped"
    exe = tmp_path / "rectify_host"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                        os.path.join(root, "tests", "rectify_host_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(11)
    named = RC.camera_maps()
    maps = [R.rectify_map(**named[n][0]) for n in ("half", "K_w3", "K_28x20")]
    maps.append(tuple(rng.integers(-2 ** 31, 2 ** 31 - 1, (5, 13)).astype(np.int32) for _ in range(2)))           # any int32 is valid
    maps.append((rng.integers(-300, 32 * W + 300, (9, 11)).astype(np.int32), rng.integers(-300, 32 * H + 300, (9, 11)).astype(np.int32)))
    kinds = _lib.SRC_KINDS
    blob, want = [], []

    def case(mode, enc, B, h, w, pad, bgr, qmap=None):
        data, step = RC.source_frames(enc, B, h, w, pad)
        rows = 3 * h if enc == "planar" else h
        stride = (rows - 1) * step + w * R.bytes_per_pixel(enc)          # tight: a read of the last row's padding is out of bounds
        data = np.ascontiguousarray(data[:, :stride])
        planes = 1 if enc == "mono8" and not bgr else 3
        order = _lib.ORDER_GRAY if planes == 1 else int(bgr)
        oh, ow = qmap[0].shape if mode else (h, w)
        blob.append(np.array([mode, kinds[enc], B, h, w, step, stride, oh, ow, order, planes, 0], dtype=np.int32).tobytes())
        blob.append(data.tobytes())
        if mode:
            blob.extend(q.astype(np.int32).tobytes() for q in qmap)
            want.append(np.stack([R.rectify(data[b], enc, h, w, qmap[0], qmap[1], step, bgr, planes) for b in range(B)]))
        else:
            want.append(np.stack([R.unpack(data[b], enc, h, w, step, bgr, planes) for b in range(B)]))

    for enc in kinds:
        for (h, w), pad, bgr in (((3, 3), 0, False), ((4, 6), 5, True), ((7, 5), 5, False), ((33, 47), 5, True)):
            case(0, enc, 2, h, w, 0 if enc == "planar" else pad, bgr)
        for i, qmap in enumerate(maps):
            case(1, enc, 2, H, W, 0 if enc == "planar" else 5, bool(i & 1), qmap)
    corpus, result = tmp_path / "corpus.bin", tmp_path / "result.bin"
    with open(corpus, "wb") as f:
        f.write(np.uint32(len(want)).tobytes())
        for b in blob:
            f.write(b)
    r = subprocess.run([str(exe), str(corpus), str(result)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got = np.fromfile(result, dtype=np.uint8)
    p = 0
    for i, wnt in enumerate(want):
        assert int(np.frombuffer(got[p:p + 4].tobytes(), dtype=np.int32)[0]) == 0, i
        assert np.array_equal(got[p + 4:p + 4 + wnt.size], wnt.reshape(-1)), i
        p += 4 + wnt.size
    assert p == got.size
