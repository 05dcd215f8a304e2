"""JPEG ingest on the GPU: ops.jpeg_decode (host Huffman stage, HIP inverse DCT + fancy upsampling + colour) against tests/jpeg_ref.py,
byte for byte, on the streams of tests/golden/jpeg_cases.pt.  jpeg_ref itself is pinned to Pillow in tests/test_jpeg_host.py; nothing
here needs Pillow."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref  # noqa: E402

from oracle import vit as OV  # noqa: E402
from wild_visual_navigation_amd import _lib, ops  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor  # noqa: E402
from wild_visual_navigation_amd.utils.image_io import compressed_image_to_torch  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden):
    return golden("jpeg_cases.pt")["cases"]


@pytest.fixture(scope="module")
def want(cases):
    """jpeg_ref's frame of every valid stream, computed once: {name: uint8 [3,H,W]}."""
    return {c["name"]: torch.from_numpy(jpeg_ref.decode(c["data"])) for c in cases if c["status"] == "OK"}


def _groups(cases):
    """Valid streams by geometry."""
    out = {}
    for c in cases:
        if c["status"] == "OK":
            out.setdefault((c["size"], c["sampling"]), []).append(c)
    return out


def test_every_fixture_alone(dev, cases, want):
    assert len(want) >= 80
    for c in cases:
        if c["status"] != "OK":
            continue
        out, status = ops.jpeg_decode(c["data"], dev)
        W, H = c["size"]
        assert out.shape == (1, 3, H, W) and out.dtype == torch.uint8 and out.device.type == "cuda", c["name"]
        assert status.tolist() == [0]
        assert torch.equal(out[0].cpu(), want[c["name"]]), c["name"]


def test_batches_of_three_with_equal_geometry(dev, cases, want):
    """Every valid stream as a member of a batch of 3 of its geometry (groups smaller than 3 repeat their members)."""
    n = 0
    for (size, sampling), group in _groups(cases).items():
        for i in range(0, len(group), 3):
            batch = [group[(i + k) % len(group)] for k in range(3)]
            out, status = ops.jpeg_decode([c["data"] for c in batch], dev, threads=3)
            assert status.tolist() == [0, 0, 0]
            got = out.cpu()
            for k, c in enumerate(batch):
                assert torch.equal(got[k], want[c["name"]]), (c["name"], k)
            n += 1
    assert n >= 28


def test_input_kinds_and_threads(dev, cases, want):
    group = _groups(cases)[((33, 47), "4:2:0")]
    names = [c["name"] for c in group]
    ref = torch.stack([want[n] for n in names])
    as_bytes = [c["data"] for c in group]
    kinds = [as_bytes[0], bytearray(as_bytes[1]), torch.frombuffer(bytearray(as_bytes[2]), dtype=torch.uint8), memoryview(as_bytes[3])] + as_bytes[4:]
    for threads in (1, 8, 16):
        out, _ = ops.jpeg_decode(kinds, dev, threads=threads)
        assert torch.equal(out.cpu(), ref), threads


def test_gray_output(dev, cases, want):
    for name in ("17x23_gray_q75", "33x47_gray_rst_rows1", "299x224_gray_q75", "17x23_gray_factors2x2", "1x1_gray_q75"):
        c = next(c for c in cases if c["name"] == name)
        out, _ = ops.jpeg_decode([c["data"]] * 2, dev, gray=True)
        W, H = c["size"]
        assert out.shape == (2, 1, H, W)
        assert torch.equal(out[1, 0].cpu(), want[name][0]) and torch.equal(out[0], out[1])
        assert torch.equal(torch.from_numpy(jpeg_ref.decode(c["data"], gray=True)), out[0].cpu())
    with pytest.raises(_lib.WvnError, match="gray=True"):
        ops.jpeg_decode(next(c for c in cases if c["name"] == "17x23_4:2:0_q75")["data"], dev, gray=True)


def test_a_corrupt_member_is_zero_and_leaves_its_neighbours_alone(dev, cases, want):
    good = [c for c in _groups(cases)[((33, 47), "4:2:0")]][:2]
    for bad_name in ("truncated_mid_scan", "bad_huffman", "truncated_at_marker", "refuse_progressive", "out_of_range_qt16",
                     "17x23_4:2:0_q75"):
        bad = next(c for c in cases if c["name"] == bad_name)
        code = _lib.JPEG_GEOMETRY_MISMATCH if bad["status"] == "OK" else _lib.JPEG_STATUS.index(bad["status"])
        if bad["status"] == "OK":
            # a readable frame of another geometry is refused in Python, whatever `strict` says
            with pytest.raises(_lib.WvnError, match="mixed geometry"):
                ops.jpeg_decode([good[0]["data"], bad["data"], good[1]["data"]], dev, strict=False)
            continue
        out, status = ops.jpeg_decode([good[0]["data"], bad["data"], good[1]["data"]], dev, strict=False)
        assert status.tolist() == [0, code, 0], bad_name
        got = out.cpu()
        assert torch.equal(got[0], want[good[0]["name"]]) and torch.equal(got[2], want[good[1]["name"]]), bad_name
        assert int(got[1].max()) == 0, bad_name
        with pytest.raises(_lib.WvnError, match=f"frame 1: WVN_JPEG_{bad['status']}"):
            ops.jpeg_decode([good[0]["data"], bad["data"], good[1]["data"]], dev)
        assert ops.jpeg_status_name(code) == "WVN_JPEG_" + bad["status"]


def test_calls_back_to_back_reuse_the_staging_buffers(dev, cases, want):
    """Five calls on one stream without a synchronisation between them: the two pinned staging buffers are each written again while
    earlier uploads may still be in flight; every result must be its own."""
    a = _groups(cases)[((299, 224), "4:2:0")]
    b = _groups(cases)[((33, 47), "4:4:4")]
    order = [a, b, a[::-1], b[::-1], a]
    outs = [ops.jpeg_decode([c["data"] for c in grp], dev)[0] for grp in order]
    torch.cuda.synchronize()
    for grp, out in zip(order, outs):
        assert torch.equal(out.cpu(), torch.stack([want[c["name"]] for c in grp]))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        o1 = ops.jpeg_decode([c["data"] for c in a], dev)[0]
        o2 = ops.jpeg_decode([c["data"] for c in a[::-1]], dev)[0]
    side.synchronize()
    assert torch.equal(o1.cpu(), torch.stack([want[c["name"]] for c in a]))
    assert torch.equal(o2.cpu(), torch.stack([want[c["name"]] for c in a[::-1]]))


def test_compressed_image_to_torch(dev, cases, want):
    for name in ("299x224_4:2:0_q75", "33x47_4:2:2_q95", "17x23_gray_q75"):
        data = next(c for c in cases if c["name"] == name)["data"]
        rgb = compressed_image_to_torch(data, "bgr8; jpeg compressed bgr8", device=dev)
        assert rgb.dtype == torch.uint8 and rgb.dim() == 3 and torch.equal(rgb.cpu(), want[name])
        swapped = compressed_image_to_torch(data, "rgb8; jpeg compressed", device=dev)
        assert swapped.is_contiguous() and torch.equal(swapped.cpu(), want[name].flip(0))
        assert torch.equal(compressed_image_to_torch(data, device=dev).cpu(), want[name].flip(0))     # no format: cv2's BGR, as the reference
        f = compressed_image_to_torch(data, "bgr8; jpeg compressed bgr8", device=dev, as_float=True)
        assert f.dtype == torch.float32 and torch.equal(f.cpu(), want[name].float() / 255)
    with pytest.raises(_lib.WvnError, match="WVN_JPEG_UNSUPPORTED"):
        compressed_image_to_torch(next(c for c in cases if c["name"] == "refuse_cmyk")["data"], device=dev)


def test_decode_then_extract_equals_extract_on_the_reference_frames(dev, cases, want):
    S = 64
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=11, depth=2)
    fe = FeatureExtractor(device=dev, segmentation_type="grid", feature_type="dino", patch_size=8, backbone_type="vit_small", input_size=S,
                          pretrained_weights=sd, precision="bf16", allow_synthetic=True)
    names = ["299x224_4:2:0_q75", "299x224_4:2:0_q95"]
    frames = fe.decode([next(c for c in cases if c["name"] == n)["data"] for n in names])
    assert frames.shape == (2, 3, 224, 299) and frames.device.type == "cuda"
    ref = torch.stack([want[n] for n in names])
    assert torch.equal(frames.cpu(), ref)

    def square(x):
        return x[:, :, 80:80 + S, 120:120 + S].contiguous()

    f0, s0, n0 = fe.extract_batch(square(frames), cell_size=16)
    f1, s1, n1 = fe.extract_batch(square(ref.to(dev)), cell_size=16)
    assert f0.shape == (2, 16, 384) and torch.isfinite(f0).all()
    assert torch.equal(f0, f1) and torch.equal(s0, s1) and torch.equal(n0, n1)
