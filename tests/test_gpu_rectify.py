"""Raw camera ingest on the GPU: ops.unpack_frames / ops.debayer / ops.rectify, the raw C-ABI and the callback forms
(utils.image_to_torch, compressed_image_to_torch(rectify=), FeatureExtractor.decode_raw / decode) against tests/rectify_ref.py with
ZERO differing bytes.  The maps and the tap classes they cover come from tests/rectify_cases.py (tests/test_rectify_host.py holds the
coverage claims and the definition itself)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref  # noqa: E402
import rectify_cases as RC  # noqa: E402
import rectify_ref as R  # noqa: E402

from oracle import vit as OV  # noqa: E402
from wild_visual_navigation_amd import _lib, ops  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor  # noqa: E402
from wild_visual_navigation_amd.utils.image_io import compressed_image_to_torch, image_to_torch  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = RC.SRC
KINDS = R.ENCODINGS
PATTERNS = tuple(R.BAYER)


def _shape(data, encoding, B, h, w, step):
    """The bytes of B frames as the tensor ops.* takes with step= / width= (planar: dense [B,3,H,W])."""
    t = torch.from_numpy(data)
    return t.view(B, 3, h, w) if encoding == "planar" else t.view(B, h, step)


def _unpack(dev, data, encoding, B, h, w, step, **kw):
    t = _shape(data, encoding, B, h, w, step).to(dev)
    return ops.unpack_frames(t, encoding, **kw) if encoding == "planar" else ops.unpack_frames(t, encoding, step=step, width=w, **kw)


def _rectify(dev, data, encoding, B, h, w, step, m, **kw):
    t = _shape(data, encoding, B, h, w, step).to(dev)
    return ops.rectify(t, m, encoding, **kw) if encoding == "planar" else ops.rectify(t, m, encoding, step=step, width=w, **kw)


@pytest.fixture(scope="module")
def maps(dev):
    """{name: (RectifyMap on the device, qx, qy of the reference)}; the two must hold the same integers."""
    out = {}
    for name, (args, _) in RC.camera_maps().items():
        m = ops.rectify_map(device=dev, **args)
        qx, qy = R.rectify_map(**args)
        assert np.array_equal(m.qx.cpu().numpy(), qx) and np.array_equal(m.qy.cpu().numpy(), qy), name
        out[name] = (m, qx, qy)
    return out


@pytest.fixture(scope="module")
def frames47():
    """{encoding: (bytes [2, .], step)} at 33 x 47 with 5 bytes of row padding (planar: dense), two different frames each."""
    return {e: RC.source_frames(e, 2, H, W, pad=0 if e == "planar" else 5) for e in KINDS}


# ----------------------------------------------------------------------------------------------------------------- unpack
@pytest.mark.parametrize("encoding", KINDS)
def test_unpack_frames(dev, encoding):
    for (h, w) in RC.SIZES:
        for pad in ((0,) if encoding == "planar" else (0, 5)):
            for B in (1, 3):
                data, step = RC.source_frames(encoding, B, h, w, pad)
                for bgr in (False, True):
                    got = _unpack(dev, data, encoding, B, h, w, step, bgr=bgr)
                    want = np.stack([R.unpack(data[b], encoding, h, w, step, bgr) for b in range(B)])
                    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (h, w, pad, B, bgr)
                    assert np.array_equal(got.cpu().numpy(), want), (h, w, pad, B, bgr)
    if encoding == "mono8":
        got = _unpack(dev, data, encoding, B, h, w, step, channels=3)
        assert np.array_equal(got.cpu().numpy(), np.stack([R.unpack(data[b], encoding, h, w, step, channels=3) for b in range(B)]))
    if encoding in PATTERNS:   # the dense forms: [B,H,W] and one frame without B
        dense, _ = RC.source_frames(encoding, 2, 7, 5)
        want = np.stack([R.demosaic(dense[b].reshape(7, 5), encoding) for b in range(2)])
        assert np.array_equal(ops.debayer(torch.from_numpy(dense).view(2, 7, 5).to(dev), encoding[6:10]).cpu().numpy(), want)
        assert np.array_equal(ops.debayer(torch.from_numpy(dense[1]).view(7, 5).to(dev), encoding).cpu().numpy(), want[1:])


def test_unpack_packed_dense_shape(dev):
    data, _ = RC.source_frames("bgr8", 2, 7, 5)
    got = ops.unpack_frames(torch.from_numpy(data).view(2, 7, 5, 3).to(dev), "bgr8")
    assert np.array_equal(got.cpu().numpy(), np.stack([R.unpack(data[b], "bgr8", 7, 5) for b in range(2)]))


# ---------------------------------------------------------------------------------------------------------------- rectify
@pytest.mark.parametrize("encoding", KINDS)
def test_rectify_every_kind_through_every_map(dev, maps, frames47, encoding):
    data, step = frames47[encoding]
    planes = {bgr: [R.unpack(data[b], encoding, H, W, step, bgr) for b in range(2)] for bgr in (False, True)}   # once per kind
    for name, (m, qx, qy) in maps.items():
        for bgr in (False, True):
            got = _rectify(dev, data, encoding, 2, H, W, step, m, bgr=bgr)
            want = np.stack([R.sample(p, qx, qy) for p in planes[bgr]])
            assert tuple(got.shape) == want.shape == (2, 1 if encoding == "mono8" else 3) + qx.shape, name
            assert np.array_equal(got.cpu().numpy(), want), (name, bgr)
    if encoding == "mono8":
        m, qx, qy = maps["half"]
        got = _rectify(dev, data, encoding, 2, H, W, step, m, channels=3)
        assert np.array_equal(got.cpu().numpy(), np.stack([R.sample(np.repeat(p, 3, 0), qx, qy) for p in planes[False]]))


@pytest.mark.parametrize("encoding", KINDS)
def test_the_identity_map_is_unpack_frames(dev, frames47, encoding):
    K = R.hoengg(W, H)
    m = ops.rectify_map(K, (0, 0, 0, 0, 0), "plumb_bob", (H, W), device=dev)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    assert np.array_equal(m.qx.cpu().numpy(), 32 * u) and np.array_equal(m.qy.cpu().numpy(), 32 * v)
    data, step = frames47[encoding]
    assert torch.equal(_rectify(dev, data, encoding, 2, H, W, step, m), _unpack(dev, data, encoding, 2, H, W, step))


@pytest.mark.parametrize("encoding", KINDS)
def test_constant_maps(dev, encoding):
    """ax = ay = 31 on an all-255 frame: the weights sum to 1024, so no overflow and 255 where the four taps are inside (a mosaic of
    255 demosaics to 255); the all-sentinel map: every tap outside, all zero."""
    rows = (3 * H if encoding == "planar" else H) * (W * R.bytes_per_pixel(encoding))
    white = np.full((2, rows), 255, dtype=np.uint8)
    step = W * R.bytes_per_pixel(encoding)

    def const(qx, qy, shape=(6, 9)):
        return ops.RectifyMap(torch.full(shape, qx, dtype=torch.int32, device=dev), torch.full(shape, qy, dtype=torch.int32, device=dev),
                              (H, W), shape, np.eye(3))

    got = _rectify(dev, white, encoding, 2, H, W, step, const(32 * 7 + 31, 32 * 5 + 31))
    assert (got == 255).all()
    got = _rectify(dev, white, encoding, 2, H, W, step, const(32 * (W - 1) + 31, 32 * 5 + 31))   # the right taps are outside
    assert (got == (1 * 255 * 32 + 512) >> 10).all()
    got = _rectify(dev, white, encoding, 2, H, W, step, const(32 * R.SENTINEL, 32 * R.SENTINEL))
    assert (got == 0).all()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_fused_equals_two_step(dev, maps, frames47, pattern):
    data, step = frames47[pattern]
    raw = _shape(data, pattern, 2, H, W, step).to(dev)
    rgb = ops.unpack_frames(raw, pattern, step=step, width=W)
    for name in ("K", "half", "K_28x20", "half_w3", "plumb_bob"):
        m = maps[name][0]
        fused = ops.rectify(raw, m, pattern, step=step, width=W, route="fused")
        assert torch.equal(fused, ops.rectify(rgb, m, "planar")), name
        assert torch.equal(fused, ops.rectify(raw, m, pattern, step=step, width=W, route="two_step")), name
        assert torch.equal(fused, ops.rectify(raw, m, pattern, step=step, width=W)), name               # the default route
        assert torch.equal(fused.flip(1), ops.rectify(raw, m, pattern, step=step, width=W, bgr=True, route="two_step")), name


def test_the_real_camera_at_full_size(dev):
    """1080 x 1440 bayer_gbrg8 random bytes through the real Hoengg camera to the 448 x 448 centre crop, two frames."""
    Hs, Ws = R.HOENGG_SIZE
    K = R.hoengg(Ws, Hs)
    args = dict(K=K, D=R.HOENGG_D, model="equidistant", src_size=(Hs, Ws), out_size=(448, 448), new_K=RC.crop_448(K))
    m = ops.rectify_map(device=dev, **args)
    qx, qy = R.rectify_map(**args)
    assert np.array_equal(m.qx.cpu().numpy(), qx) and np.array_equal(m.qy.cpu().numpy(), qy)
    assert ops.rectify_map(device=dev, **args) is m                                                  # cached per geometry
    assert np.array_equal(m.K_new, RC.crop_448(K)) and torch.equal(m.K_tensor[0, :3, :3].cpu(), torch.from_numpy(m.K_new).float())
    data, step = RC.source_frames("bayer_gbrg8", 2, Hs, Ws)
    got = ops.rectify(torch.from_numpy(data).view(2, Hs, Ws).to(dev), m, "bayer_gbrg8")
    want = np.stack([R.rectify(data[b], "bayer_gbrg8", Hs, Ws, qx, qy) for b in range(2)])
    assert tuple(got.shape) == (2, 3, 448, 448) and np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------- end to end
def test_image_to_torch(dev, maps, frames47):
    m, qx, qy = maps["half"]
    for encoding in R.ENCODINGS:
        if encoding == "planar":
            continue
        data, step = frames47[encoding]
        msg = data[1].tobytes()
        for desired, bgr, ch in (("rgb8", False, 3), ("bgr8", True, 3), ("passthrough", encoding == "bgr8", None)):
            got = image_to_torch(msg, encoding, H, W, step, device=dev, desired_encoding=desired)
            assert got.dtype == torch.uint8 and got.is_contiguous()
            assert np.array_equal(got.cpu().numpy(), R.unpack(msg, encoding, H, W, step, bgr, ch)), (encoding, desired)
            got = image_to_torch(bytearray(msg), encoding, H, W, step, device=dev, desired_encoding=desired, rectify=m)
            assert np.array_equal(got.cpu().numpy(), R.rectify(msg, encoding, H, W, qx, qy, step, bgr, ch)), (encoding, desired)
    dense, step = RC.source_frames("bayer_gbrg8", 1, H, W)
    got = image_to_torch(torch.from_numpy(dense[0]), "bayer_gbrg8", H, W, device=dev)                 # step defaults to the dense row
    assert np.array_equal(got.cpu().numpy(), R.unpack(dense[0], "bayer_gbrg8", H, W))
    with pytest.raises(_lib.WvnError, match="one message"):
        image_to_torch([dense[0].tobytes()] * 2, "bayer_gbrg8", H, W, device=dev)


def test_rectify_map_from_camera_info(dev):
    K = R.hoengg(W, H)
    P = np.concatenate([RC.halved(K), np.zeros((3, 1))], axis=1)
    m = ops.rectify_map_from_camera_info(H, W, "equidistant", list(R.HOENGG_D), list(K.ravel()), [1, 0, 0, 0, 1, 0, 0, 0, 1],
                                         list(P.ravel()), device=dev)
    qx, qy = R.rectify_map(K, R.HOENGG_D, "equidistant", (H, W), None, RC.halved(K))
    assert np.array_equal(m.qx.cpu().numpy(), qx) and np.array_equal(m.qy.cpu().numpy(), qy) and np.array_equal(m.K_new, RC.halved(K))
    assert m.K_tensor.shape == (1, 4, 4) and m.K_tensor.device.type == "cuda"
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    for model, D in (("", []), ("equidistant", [0.0] * 4), ("plumb_bob", [0.0] * 5)):                # the identity distortion
        ident = ops.rectify_map_from_camera_info(H, W, model, D, list(K.ravel()), [], list(np.concatenate([K, np.zeros((3, 1))], 1).ravel()),
                                                 device=dev)
        assert np.array_equal(ident.qx.cpu().numpy(), 32 * u) and np.array_equal(ident.qy.cpu().numpy(), 32 * v)
    small = ops.rectify_map_from_camera_info(H, W, "equidistant", R.HOENGG_D, K.ravel(), [], P.ravel(), out_size=(20, 28), device=dev)
    assert small.out_size == (20, 28) and np.array_equal(small.K_new, np.diag([28 / W, 20 / H, 1.0]) @ RC.halved(K))


def test_compressed_image_to_torch_rectified_and_decode(dev, golden):
    cases = golden("jpeg_cases.pt")["cases"]
    names = ["299x224_4:2:0_q75", "299x224_4:2:0_q95"]
    data = [next(c for c in cases if c["name"] == n)["data"] for n in names]
    rgb = [jpeg_ref.decode(d) for d in data]
    Hj, Wj = rgb[0].shape[1:]
    K = R.hoengg(Wj, Hj)
    args = dict(K=K, D=R.HOENGG_D, model="equidistant", src_size=(Hj, Wj), out_size=(64, 64), new_K=np.diag([64 / Wj, 64 / Hj, 1.0]) @ RC.halved(K))
    m, (qx, qy) = ops.rectify_map(device=dev, **args), R.rectify_map(**args)
    want = np.stack([R.sample(p, qx, qy) for p in rgb])
    got = compressed_image_to_torch(data[0], "bgr8; jpeg compressed bgr8", device=dev, rectify=m)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want[0])
    assert np.array_equal(compressed_image_to_torch(data[0], "rgb8; jpeg compressed", device=dev, rectify=m).cpu().numpy(), want[0][::-1])
    f = compressed_image_to_torch(data[0], "bgr8; jpeg compressed bgr8", device=dev, as_float=True, rectify=m)
    assert f.dtype == torch.float32 and torch.equal(f.cpu(), torch.from_numpy(want[0]).float() / 255)
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=11, depth=2)
    fe = FeatureExtractor(device=dev, segmentation_type="grid", feature_type="dino", patch_size=8, backbone_type="vit_small", input_size=64,
                          pretrained_weights=sd, precision="bf16", allow_synthetic=True)
    assert np.array_equal(fe.decode(data, rectify=m).cpu().numpy(), want)
    # unchanged defaults: without rectify, decode is ops.jpeg_decode and compressed_image_to_torch what it was
    plain = fe.decode(data)
    assert torch.equal(plain, ops.jpeg_decode(data, dev)[0]) and np.array_equal(plain.cpu().numpy(), np.stack(rgb))
    assert np.array_equal(compressed_image_to_torch(data[1], device=dev).cpu().numpy(), rgb[1][::-1])
    # the raw topic of the same camera: a list of bayer_gbrg8 messages -> frames the extractor takes
    raw = [RC.mosaic_of(p, "bayer_gbrg8") for p in rgb]
    step = Wj + 5
    msgs = [np.pad(r, ((0, 0), (0, 5)), constant_values=77).tobytes() for r in raw]
    frames = fe.decode_raw(msgs, "bayer_gbrg8", Hj, Wj, step, rectify=m)
    want_raw = np.stack([R.rectify(b, "bayer_gbrg8", Hj, Wj, qx, qy, step) for b in msgs])
    assert tuple(frames.shape) == (2, 3, 64, 64) and np.array_equal(frames.cpu().numpy(), want_raw)
    full = fe.decode_raw(msgs, "bayer_gbrg8", Hj, Wj, step)
    assert np.array_equal(full.cpu().numpy(), np.stack([R.unpack(b, "bayer_gbrg8", Hj, Wj, step) for b in msgs]))
    mono = fe.decode_raw(msgs[0], "mono8", Hj, Wj, step, rectify=m)                                 # mono8: replicated to what extract takes
    assert np.array_equal(mono.cpu().numpy(), R.rectify(msgs[0], "mono8", Hj, Wj, qx, qy, step, channels=3)[None])
    feat, seg, nseg = fe.extract_batch(frames, cell_size=16)
    f1, s1, n1 = fe.extract_batch(torch.from_numpy(want_raw).to(dev), cell_size=16)
    assert feat.shape == (2, 16, 384) and torch.isfinite(feat).all() and torch.equal(feat, f1) and torch.equal(seg, s1)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(dev, maps):
    """WVN_ERR_ARG from the C-ABI (the buffers of a refused call are host words: nothing may touch them) and WvnError from ops."""
    for what, rc in RC.abi_refusals(_lib.lib()):
        assert rc == _lib.ERR_ARG, what
    m = maps["K"][0]
    z = torch.zeros(1, 8, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.WvnError, match="33 x 47"):
        ops.rectify(z, m, "mono8")
    with pytest.raises(_lib.WvnError, match="H, W >= 3"):
        ops.debayer(z[:, :2], "gbrg")
    with pytest.raises(_lib.WvnError, match="lives on"):
        ops.rectify(torch.zeros(1, H, W, dtype=torch.uint8, device=dev),
                    ops.RectifyMap(m.qx.cpu(), m.qy.cpu(), m.src_size, m.out_size, m.K_new), "mono8")
    torch.cuda.synchronize()
