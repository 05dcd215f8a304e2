"""csrc/overlay.hip through ops.overlay / overlay_panels / image_to_u8, the visu package, the drop-in and the estimator, against
tests/visu_ref.py (the same pictures stated in torch on the CPU).  Every comparison is torch.equal on uint8."""
import os

import pytest
import torch

import visu_ref as VR
from wild_visual_navigation_amd import ops
from wild_visual_navigation_amd.visu import LearningVisualizer, colour_table, default_classification_table

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _same(got, want):
    assert got.dtype == torch.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert torch.equal(got.cpu(), want)


def _lut(N, seed=5):
    return torch.randint(0, 256, (N, 3), generator=_gen(seed), dtype=torch.uint8)


@pytest.fixture(scope="module")
def demo(golden):
    return golden("demo_frames_224.pt")["frames_u8"]          # [n,3,224,224] uint8


# ---- blend ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0, 0.3, 0.5, 0.6, 1.0])
def test_every_byte_pair_blends_as_the_formula(dev, alpha):
    """Identity table, frame byte = row, label = column: out[y, x] = blend(x over y) for all 65536 pairs."""
    r = torch.arange(256, dtype=torch.uint8)
    lut = r[:, None].expand(256, 3).contiguous()
    img = r[None, :, None].expand(3, 256, 256).contiguous()[None]
    labels = torch.arange(256, dtype=torch.int32)[None, :].expand(256, 256).contiguous()[None]
    got = ops.overlay(img.to(dev), labels=labels.to(dev), lut=lut.to(dev), alpha=alpha)
    want = VR.overlay(img, labels=labels, lut=lut, alpha=alpha)
    _same(got, want)
    a = VR.alpha_byte(alpha)
    assert torch.equal(want[0, :, :, 0], VR.blend(r[None, :].expand(256, 256), r[:, None].expand(256, 256), a))


# ---- shapes that hit the store paths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (17, 33), (16, 64), (224, 224)])
def test_shapes_vector_rows_byte_rows_and_tails(dev, H, W, B):
    """W % 4 == 0: every row on the 12-byte vector store; W = 33 / 5 / 1: rows that start off a 4-byte boundary and row tails on
    byte stores; several blocks (224 x 224) and several frames."""
    g = _gen(H * 1000 + W + B)
    img = torch.rand(B, 3, H, W, generator=g)
    val = torch.rand(B, H, W, generator=g) * 1.2 - 0.1
    mask = torch.rand(B, H, W, generator=g) < 0.2
    lut = torch.rand(256, 3, generator=g)
    got = ops.overlay(img.to(dev), values=val.to(dev), lut=lut.to(dev), alpha=0.5, overlay_mask=mask.to(dev))
    _same(got, VR.overlay(img, values=val, lut=lut, alpha=0.5, overlay_mask=mask))
    _same(ops.image_to_u8(img.to(dev)), VR.image_to_u8(img))


@pytest.mark.parametrize("nmaps", [1, 2, 4])
def test_panels_at_odd_width(dev, nmaps):
    """W = 33: row pitch 198 (2 panels: 4-misaligned on odd rows), 297 (3 panels: on most rows), 495 bytes; one launch, the frame
    converted once; equal to the separate pictures side by side."""
    B, H, W = 2, 17, 33
    g = _gen(nmaps)
    img = torch.rand(B, 3, H, W, generator=g)
    maps = [torch.rand(B, H, W, generator=g) for _ in range(nmaps)]
    lut = _lut(256)
    got = ops.overlay_panels(img.to(dev), [m.to(dev) for m in maps], lut.to(dev), 0.5)
    assert got.shape == (B, H, (1 + nmaps) * W, 3) and got.stride(1) == 3 * (1 + nmaps) * W
    want = VR.overlay_panels(img, maps, lut, 0.5)
    _same(got, want)
    parts = [ops.image_to_u8(img.to(dev))] + [ops.overlay(img.to(dev), values=m.to(dev), lut=lut.to(dev), alpha=0.5) for m in maps]
    assert torch.equal(got, torch.cat(parts, dim=2))


@pytest.mark.parametrize("c0", [0, 1, 2, 3, 7])
def test_out_is_a_column_slice_of_a_wider_image(dev, c0):
    B, H, W, WT = 2, 9, 20, 41
    g = _gen(c0)
    img = torch.rand(B, 3, H, W, generator=g)
    val = torch.rand(B, H, W, generator=g)
    lut = _lut(256)
    wide = torch.full((B, H, WT, 3), 77, dtype=torch.uint8, device=dev)
    ret = ops.overlay(img.to(dev), values=val.to(dev), lut=lut.to(dev), alpha=0.3, out=wide[:, :, c0:c0 + W])
    assert ret.data_ptr() == wide[:, :, c0:c0 + W].data_ptr()
    want = torch.full((B, H, WT, 3), 77, dtype=torch.uint8)
    want[:, :, c0:c0 + W] = VR.overlay(img, values=val, lut=lut, alpha=0.3)
    _same(wide, want)                                              # the picture in place, not a byte beside it touched


# ---- image rules ----------------------------------------------------------------------------------------------------------------
def _image_cases():
    g = _gen(11)
    H, W = 6, 10
    below = torch.rand(3, H, W, generator=g) * 0.999
    exact = below.clone()
    exact[1, 2, 3] = 1.0
    above = below.clone()
    above[2, 0, 0] = 1.5
    bytes_f = torch.rand(3, H, W, generator=g) * 255
    u8 = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
    bits = torch.randint(0, 2, (3, H, W), generator=g, dtype=torch.uint8)
    wild = bytes_f.clone()
    wild.view(-1)[:8] = torch.tensor([-3.0, 300.0, float("nan"), float("inf"), float("-inf"), 255.0, 255.9, -0.0])
    wild_nonan = torch.nan_to_num(wild, nan=17.0)
    small_wild = below.clone()
    small_wild.view(-1)[:3] = torch.tensor([-0.5, float("-inf"), -1e30])      # max <= 1: scaled; negatives clamp to 0
    return {"below_1": below, "exactly_1": exact, "max_1.5": above, "bytes_as_float": bytes_f, "uint8": u8, "uint8_bits": bits,
            "nan_inf_out_of_range": wild, "out_of_range": wild_nonan, "negative_unit": small_wild}


@pytest.mark.parametrize("name", list(_image_cases()))
def test_image_to_8_bits(dev, name):
    img = _image_cases()[name]
    for unit_range in (None, True, False):
        _same(ops.image_to_u8(img.to(dev), unit_range=unit_range), VR.image_to_u8(img, unit_range))
    if name in ("below_1", "exactly_1", "uint8_bits", "negative_unit"):      # the decision itself, not only agreement
        assert torch.equal(VR.image_to_u8(img), VR.image_to_u8(img, True))
    else:
        assert torch.equal(VR.image_to_u8(img), VR.image_to_u8(img, False))


def test_the_scaling_decision_is_per_frame(dev):
    c = _image_cases()
    img = torch.stack([c["below_1"], c["max_1.5"], c["nan_inf_out_of_range"], c["exactly_1"]])
    got = ops.image_to_u8(img.to(dev))
    _same(got, VR.image_to_u8(img))
    _same(got[0:1], VR.image_to_u8(img[0], True))
    _same(got[1:2], VR.image_to_u8(img[1], False))
    fm = ops.frame_max(img.to(dev)).cpu()
    assert fm[0] == img[0].max() and fm[1] == 1.5 and torch.isnan(fm[2]) and fm[3] == 1.0
    big = torch.rand(2, 3, 61, 67, generator=_gen(3)) - 0.5            # several blocks, n % 16 != 0, a misaligned second frame
    big[1, 2, 60, 66] = 7.25
    assert torch.equal(ops.frame_max(big.to(dev)).cpu(), torch.stack([big[0].max(), big[1].max()]))
    assert torch.equal(ops.frame_max((big - 5).clamp(max=-1).to(dev)).cpu(), torch.zeros(2))       # max(0, .)
    u8 = torch.randint(0, 200, (2, 3, 61, 67), generator=_gen(4), dtype=torch.uint8)
    assert torch.equal(ops.frame_max(u8.to(dev)).cpu(), torch.stack([u8[0].max(), u8[1].max()]).float())


# ---- value rules ----------------------------------------------------------------------------------------------------------------
def test_value_map_index_rule(dev):
    k = torch.arange(256, dtype=torch.float32) / 255
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.5, 0.0, -0.0, 1.0, 2.0, 1e38, -1e38, 3e36, 1.0039216])
    vals = torch.cat([k, torch.nextafter(k, torch.zeros_like(k)), torch.nextafter(k, torch.ones_like(k) * 2), special])
    W = 65
    H = (vals.numel() + W - 1) // W
    val = torch.zeros(H * W)
    val[:vals.numel()] = vals
    val = val.reshape(1, H, W)
    img = torch.rand(1, 3, H, W, generator=_gen(1))
    lut = _lut(256)
    got = ops.overlay(img.to(dev), values=val.to(dev), lut=lut.to(dev), alpha=1.0)
    _same(got, VR.overlay(img, values=val, lut=lut, alpha=1.0))
    idx = VR.index_values(val)[0].reshape(-1)
    assert (idx[:256] - torch.arange(256)).abs().max() <= 1 and idx[256:512].max() < 255          # fp32(k / 255) * 255: k or just below it
    assert idx[768:768 + 12].tolist()[:8] == [0, 0, 0, 0, 0, 0, 255, 255]
    assert torch.equal(got.cpu()[0].reshape(-1, 3)[:vals.numel()], lut[idx[:vals.numel()]])          # alpha 1: the table colour itself


@pytest.mark.parametrize("N", [40, 1024])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_label_maps_and_ids_outside_the_table(dev, N, dtype):
    g = _gen(N)
    B, H, W = 2, 13, 21
    lab = torch.randint(0, N, (B, H, W), generator=g, dtype=torch.int64)
    odd = [-1, N, 2 ** 31 - 1, -N, N - 1, 0] + ([2 ** 32 + 5, -2 ** 40, 2 ** 31] if dtype == torch.int64 else [-2 ** 31])
    lab.view(-1)[:len(odd)] = torch.tensor(odd)
    lab.view(-1)[-len(odd):] = torch.tensor(odd)
    lab = lab.to(dtype)
    img = torch.rand(B, 3, H, W, generator=g)
    lut = _lut(N)
    got = ops.overlay(img.to(dev), labels=lab.to(dev), lut=lut.to(dev), alpha=0.5)
    want = VR.overlay(img, labels=lab, lut=lut, alpha=0.5)
    _same(got, want)
    plain = VR.image_to_u8(img)
    assert torch.equal(want[0, 0, 0], plain[0, 0, 0]) and torch.equal(want[0, 0, 1], plain[0, 0, 1])   # -1 and N: the plain pixel
    for bad_n in (1025, 0):
        with pytest.raises(ops._lib.WvnError):
            ops.overlay(img.to(dev), labels=lab.to(dev), lut=torch.zeros(bad_n, 3, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_per_segment_values(dev, dtype):
    g = _gen(7)
    B, H, W, S = 2, 19, 27, 100
    seg = torch.randint(0, S, (B, H, W), generator=g, dtype=torch.int64)
    odd = [-1, -S, S, -S - 1, S + 5, S - 1, 0]
    seg.view(-1)[:len(odd)] = torch.tensor(odd)
    seg[1].view(-1)[:len(odd)] = torch.tensor(odd)
    pred = torch.rand(B, S, generator=g)
    pred[0, :8] = torch.tensor([float("nan"), float("inf"), -0.5, 1.0, 1.01, -0.001, 0.0, float("-inf")])
    pred[1, S - 1] = float("nan")          # what id -1 wraps to
    pred[1, 0] = 1.0                       # what id -S wraps to
    img = torch.rand(B, 3, H, W, generator=g)
    lut = _lut(256)
    got = ops.overlay(img.to(dev), values=pred.to(dev), seg=seg.to(dtype).to(dev), lut=lut.to(dev), alpha=0.6)
    want = VR.overlay(img, values=pred, seg=seg.to(dtype), lut=lut, alpha=0.6)
    _same(got, want)
    plain = VR.image_to_u8(img)
    assert torch.equal(want[1, 0, 0], plain[1, 0, 0])                                        # id -1 -> S - 1 -> NaN: plain
    assert torch.equal(want[1, 0, 1], VR.blend(lut[255], plain[1, 0, 1], 153))               # id -S -> 0 -> 1.0 -> index 255
    assert torch.equal(want[0, 0, 2], plain[0, 0, 2]) and torch.equal(want[0, 0, 3], plain[0, 0, 3])   # S, -S - 1: out of range
    # one frame, a vector without the batch axis
    _same(ops.overlay(img[0].to(dev), values=pred[0].to(dev), seg=seg[0].to(dev), lut=lut.to(dev), alpha=0.6), want[:1])


def test_float_tables_convert_as_the_reference_does(dev):
    g = _gen(9)
    B, H, W = 1, 8, 12
    img = torch.rand(B, 3, H, W, generator=g)
    lab = torch.randint(0, 300, (B, H, W), generator=g, dtype=torch.int32)
    lut = torch.rand(300, 3, generator=g)
    lut[:4] = torch.tensor([[0.0, 1.0, 0.5], [-0.1, 1.2, float("nan")], [1 / 255, 254.999 / 255, 0.999999], [float("inf"), float("-inf"), 1e-9]])
    want = VR.overlay(img, labels=lab, lut=lut, alpha=0.5)
    _same(ops.overlay(img.to(dev), labels=lab.to(dev), lut=lut.to(dev), alpha=0.5), want)
    _same(ops.overlay(img.to(dev), labels=lab.to(dev), lut=VR.lut_u8(lut).to(dev), alpha=0.5), want)
    lut64 = torch.rand(300, 3, generator=g, dtype=torch.float64)
    _same(ops.overlay(img.to(dev), labels=lab.to(dev), lut=lut64.to(dev), alpha=0.5),
          VR.overlay(img, labels=lab, lut=(lut64 * 255).to(torch.uint8), alpha=0.5))      # (c * 255) in the table's own precision


# ---- mask and boundaries ---------------------------------------------------------------------------------------------------------
def test_overlay_mask_dtypes(dev):
    g = _gen(13)
    B, H, W = 2, 10, 14
    img = torch.rand(B, 3, H, W, generator=g)
    val = torch.rand(B, H, W, generator=g)
    mask = torch.rand(B, H, W, generator=g) < 0.5
    lut = _lut(256)
    want = VR.overlay(img, values=val, lut=lut, alpha=0.5, overlay_mask=mask)
    for m in (mask, mask.to(torch.uint8) * 3, mask.float()):
        _same(ops.overlay(img.to(dev), values=val.to(dev), lut=lut.to(dev), alpha=0.5, overlay_mask=m.to(dev)), want)
    assert not torch.equal(want, VR.overlay(img, values=val, lut=lut, alpha=0.5))


@pytest.mark.parametrize("boundary_alpha", [0, 128, 255])
def test_boundaries_grid_slic_border_and_single_label(dev, demo, boundary_alpha):
    frame = demo[0]
    H = W = 224
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid = ((yy // 32) * 7 + xx // 32).to(torch.int64)
    corner = torch.zeros(H, W, dtype=torch.int32)
    corner[0, 0], corner[H - 1, W - 1], corner[0, 100], corner[77, 0] = 1, 2, 3, 4          # boundary pixels on the image border
    single = torch.full((H, W), 5, dtype=torch.int32)
    slic = ops.slic(frame.to(dev), 100).cpu()
    lut = _lut(128)
    for seg in (grid, corner, single, slic):
        got = ops.overlay(frame.to(dev), labels=seg.to(dev), lut=lut.to(dev), alpha=0.5, boundary_seg=seg.to(dev),
                          boundary_alpha=boundary_alpha)
        want = VR.overlay(frame, labels=seg, lut=lut, alpha=0.5, boundary_seg=seg, boundary_alpha=boundary_alpha)
        _same(got, want)
        if boundary_alpha == 0 or seg is single:
            assert torch.equal(want, VR.overlay(frame, labels=seg, lut=lut, alpha=0.5))   # the identity: no boundary at all
    e = VR.boundaries(corner)
    assert e[0, 0] and e[0, 1] and e[1, 0] and e[H - 1, W - 2] and e[76, 0] and e[78, 0] and e[77, 1] and int(e.sum()) == 3 + 3 + 4 + 4
    if boundary_alpha == 255:
        assert bool((want[0][VR.boundaries(slic)] == 255).all())                              # white, opaque
    # another map for the boundaries than for the colours, on a value overlay
    val = torch.rand(1, H, W, generator=_gen(2))
    _same(ops.overlay(frame.to(dev), values=val.to(dev), lut=lut.to(dev), alpha=0.5, boundary_seg=grid.to(dev), boundary_alpha=boundary_alpha),
          VR.overlay(frame, values=val, lut=lut, alpha=0.5, boundary_seg=grid, boundary_alpha=boundary_alpha))


# ---- the visualizer ---------------------------------------------------------------------------------------------------------------
def test_visualizer_methods_restate_the_reference_calls(dev, demo):
    import numpy as np

    vis = LearningVisualizer()
    g = _gen(21)
    frame = demo[1].float() / 255                                     # quick_start.py:160-161
    H = W = 224
    fd = frame.to(dev)
    default = default_classification_table()
    rdylbu = colour_table("RdYlBu", 256)
    # plot_image: CHW, HWC, numpy, 0-255 floats, uint8
    want = VR.image_to_u8(frame)[0]
    for im in (fd, fd.permute(1, 2, 0), frame.numpy(), frame * 255, demo[1]):
        got = vis.plot_image(im)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (H, W, 3)
    assert torch.equal(torch.from_numpy(vis.plot_image(fd)), want)
    assert torch.equal(torch.from_numpy(vis.plot_image(fd.permute(1, 2, 0))), want)
    assert torch.equal(torch.from_numpy(vis.plot_image(frame.numpy())), want)
    assert torch.equal(torch.from_numpy(vis.plot_image(demo[1])), demo[1].permute(1, 2, 0))
    assert torch.equal(torch.from_numpy(vis.plot_image(frame * 255)), VR.image_to_u8(frame * 255)[0])
    # plot_segmentation: c_map[seg], a table given as a tensor, [1,H,W] and bool maps
    seg = torch.randint(0, 40, (H, W), generator=g)
    table = torch.rand(40, 3, generator=g)
    assert torch.equal(torch.from_numpy(vis.plot_segmentation(seg.to(dev), max_seg=40, colormap=table.to(dev))), VR.lut_u8(table)[seg])
    assert torch.equal(torch.from_numpy(vis.plot_segmentation(seg[None].to(dev), max_seg=40, colormap=table.to(dev))), VR.lut_u8(table)[seg])
    assert torch.equal(torch.from_numpy(vis.plot_segmentation((seg > 20).to(dev), colormap=table[:2].to(dev))), VR.lut_u8(table)[(seg > 20).long()])
    # plot_detectron: plot_image, plot_segmentation, composite (+ boundaries)
    mask = torch.rand(H, W, generator=g) < 0.3
    got = vis.plot_detectron(fd, seg.to(dev), alpha=0.5, max_seg=40, colormap=table.to(dev), overlay_mask=mask.to(dev))
    assert torch.equal(torch.from_numpy(got), VR.overlay(frame, labels=seg, lut=table, alpha=0.5, overlay_mask=mask)[0])
    got = vis.plot_detectron(fd, seg.to(dev), alpha=0.6, max_seg=40, colormap=table.to(dev), boundary_alpha=200)
    assert torch.equal(torch.from_numpy(got), VR.overlay(frame, labels=seg, lut=table, alpha=0.6, boundary_seg=seg, boundary_alpha=200)[0])
    got = vis.plot_detectron(fd, seg.to(dev), max_seg=40, colormap=table.to(dev), boundary_alpha=200, draw_bound=False)
    assert torch.equal(torch.from_numpy(got), VR.overlay(frame, labels=seg, lut=table, alpha=0.5)[0])
    got = vis.plot_detectron(fd, seg.to(dev) * 6, max_seg=256, colormap="RdYlBu", draw_bound=False)
    assert torch.equal(torch.from_numpy(got), VR.overlay(frame, labels=seg * 6, lut=rdylbu, alpha=0.5)[0])
    # plot_detectron_classification: the default table, cmap= as a tensor, overlay_mask
    val = torch.rand(H, W, generator=g) * 1.1 - 0.05
    got = vis.plot_detectron_classification(fd, val.to(dev))
    assert torch.equal(torch.from_numpy(got), VR.overlay(frame, values=val, lut=default, alpha=0.5)[0])
    got = vis.plot_detectron_classification(fd, val.to(dev), alpha=0.3, overlay_mask=mask.to(dev), cmap=torch.rand(256, 3, generator=_gen(5)).to(dev))
    assert torch.equal(torch.from_numpy(got), VR.overlay(frame, values=val, lut=torch.rand(256, 3, generator=_gen(5)), alpha=0.3, overlay_mask=mask)[0])
    # plot_traversability_graph_on_seg: (prediction[seg] * 255) through sns.color_palette("RdYlBu", 256) at alpha 0.6
    pred = torch.rand(40, generator=g)
    got = vis.plot_traversability_graph_on_seg(pred.to(dev), seg.to(dev), None, None, fd)
    assert torch.equal(torch.from_numpy(got), VR.overlay(frame, values=pred, seg=seg, lut=rdylbu, alpha=0.6)[0])
    # plot_list of three plots == one panel launch; as_tensor keeps the same bytes on the device
    conf = torch.rand(H, W, generator=g)
    panel = vis.plot_list([vis.plot_image(fd), vis.plot_detectron_classification(fd, conf.to(dev)), vis.plot_detectron_classification(fd, val.to(dev))])
    one = ops.overlay_panels(fd, [conf.to(dev), val.to(dev)], default.to(dev), 0.5)
    assert panel.shape == (H, 3 * W, 3) and torch.equal(torch.from_numpy(panel), one[0].cpu())
    _same(one, VR.overlay_panels(frame, [conf, val], default, 0.5))
    t = vis.plot_detectron_classification(fd, val.to(dev), as_tensor=True)
    assert t.is_cuda and t.dtype == torch.uint8 and torch.equal(t.cpu(), torch.from_numpy(vis.plot_detectron_classification(fd, val.to(dev))))
    tl = vis.plot_list([vis.plot_image(fd, as_tensor=True), t], as_tensor=True)
    assert tl.is_cuda and torch.equal(tl.cpu(), torch.cat([want, t.cpu()], dim=1))
    assert all(k[2].startswith("cuda") for k in vis._tables)          # colour tables cached on the device, by name


# ---- the drop-in ------------------------------------------------------------------------------------------------------------------
def test_quick_start_visualisation_lines_through_the_drop_in(dev, demo, tmp_path):
    """quick_start.py:108 and :205-221 as written there, against ``wild_visual_navigation.visu`` as the drop-in aliases it, on the
    per-pixel maps of a demo frame."""
    import wild_visual_navigation_amd.dropin as dropin

    dropin.install(force_synthetic=True)
    from wild_visual_navigation.visu import LearningVisualizer as LV                     # quick_start.py:19
    from oracle import mlp as OM, vit as OV
    from wild_visual_navigation_amd.cfg import ExperimentParams
    from wild_visual_navigation_amd.feature_extractor import FeatureExtractor
    from wild_visual_navigation_amd.model import get_model
    from wild_visual_navigation_amd.utils import ConfidenceGenerator

    output_folder = str(tmp_path)
    visualizer = LV(p_visu=output_folder, store=True)                                     # :108
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=21, depth=2)
    fe = FeatureExtractor(device=dev, segmentation_type="grid", feature_type="dino", patch_size=8, backbone_type="vit_small",
                          input_size=224, pretrained_weights=sd, precision="bf16")
    params = ExperimentParams()
    params.model.simple_mlp_cfg.input_size = fe.feature_dim
    model = get_model(params.model).to(dev)
    model.eval()
    model.load_state_dict(OM.make_mlp_state_dict(384, seed=42), strict=False)
    cg = ConfidenceGenerator(method=params.loss.method, std_factor=params.loss.confidence_std_factor).to(dev)
    cg.mean[0], cg.std[0] = 0.9, 0.25
    torch_image = demo[0].to(dev).float() / 255.0                                         # :160-161
    trav, conf, _ = fe.predict_per_pixel(torch_image[None], model, cg)
    out_trav, out_confidence = trav[0], conf[0]
    img_p = "/some/folder/demo_frame.png"

    original_img = visualizer.plot_image(torch_image, store=False)                        # :205
    img_ls = [original_img]
    conf_img = visualizer.plot_detectron_classification(torch_image, out_confidence, store=False)   # :213
    img_ls.append(conf_img)
    name = img_p.split("/")[-1].split(".")[0]                                             # :216
    trav_img = visualizer.plot_detectron_classification(torch_image, out_trav, store=False)         # :217
    img_ls.append(trav_img)
    res = visualizer.plot_list(img_ls, tag=f"{name}_original_conf_trav", store=True)      # :221

    want = VR.overlay_panels(torch_image.cpu(), [out_confidence.cpu(), out_trav.cpu()], default_classification_table(), 0.5)[0]
    assert res.dtype.name == "uint8" and res.shape == (224, 3 * 224, 3)
    assert torch.equal(torch.from_numpy(res), want)
    assert not torch.equal(want[:, 224:448], want[:, :224]) and not torch.equal(want[:, 224:448], want[:, 448:])
    path = os.path.join(output_folder, "0_demo_frame_original_conf_trav.png")
    Image = pytest.importorskip("PIL.Image")
    import numpy as np

    assert os.listdir(output_folder) == ["0_demo_frame_original_conf_trav.png"]          # store=False wrote nothing
    assert torch.equal(torch.from_numpy(np.array(Image.open(path))), want)


# ---- the estimator ----------------------------------------------------------------------------------------------------------------
def _node(dev, g, S=12, H=48, D=90):
    from wild_visual_navigation_amd.traversability_estimator import MissionNode

    n = MissionNode(timestamp=1.0)
    n.features = torch.randn(S, D, generator=g).to(dev)
    n.feature_segments = (torch.arange(H * H).reshape(H, H) * S // (H * H)).to(dev)
    n.image = torch.rand(3, H, H, generator=g).to(dev)
    n.feature_positions = (torch.rand(S, 2, generator=g) * (H - 1)).to(dev)
    n.feature_edges = torch.stack([torch.arange(S - 1), torch.arange(1, S)]).to(dev)
    return n


def test_estimator_plots_mission_nodes(dev, tmp_path):
    from wild_visual_navigation_amd.cfg import ExperimentParams
    from wild_visual_navigation_amd.traversability_estimator import TraversabilityEstimator
    from wild_visual_navigation_amd.utils import Data

    p = ExperimentParams()
    p.model.simple_mlp_cfg.input_size = 90
    te = TraversabilityEstimator(p, device=dev, min_samples_for_training=2)
    assert isinstance(te._visualizer, LearningVisualizer) and te._visualizer._tables == {}
    g = _gen(0)
    S, H = 12, 48
    n = _node(dev, g, S, H)
    assert te.plot_mission_node_prediction(n) is None                                  # no prediction yet: as the reference
    assert te.add_mission_node(n)
    mask = torch.full((3, H, H), float("nan"))
    mask[:, : H // 2] = 0.5 + 0.5 * torch.rand(3, H // 2, H, generator=g)
    te.update_supervision(n, mask.to(dev))
    with torch.no_grad():
        n.prediction = te._model.forward(Data(x=n.features))
    rdylbu = colour_table("RdYlBu", 256)
    img, seg, pred, feat = n.image.cpu(), n.feature_segments.cpu(), n.prediction.cpu(), n.features.cpu()
    trav_img, conf_img = te.plot_mission_node_prediction(n)
    res = ((pred[:, 1:] - feat) ** 2).mean(1)                                         # get_confidence
    res = res - res.min()
    conf = 1 - res / res.max()
    assert torch.equal(torch.from_numpy(trav_img), VR.overlay(img, values=pred[:, 0], seg=seg, lut=rdylbu, alpha=0.6)[0])
    conf_dev = 1 - (lambda r: (r - r.min()) / (r - r.min()).max())(torch.nn.functional.mse_loss(n.prediction[:, 1:], n.features, reduction="none").mean(1))
    assert torch.equal(torch.from_numpy(conf_img), VR.overlay(img, values=conf_dev.cpu(), seg=seg, lut=rdylbu, alpha=0.6)[0])
    assert (conf - conf_dev.cpu()).abs().max() < 1e-5
    assert te._visualizer._tables                                                         # uploaded on first use ...
    # plot_mission_node_training: the supervision-mask picture (plot_detectron of the rounded mask under its NaN mask)
    sm = n.supervision_mask.cpu()
    nan = torch.isnan(sm)
    labels = torch.round(torch.clamp(255 * torch.where(nan, torch.zeros_like(sm), sm)[0], 0, 255)).long()
    want_mask = VR.overlay(img, labels=labels, lut=rdylbu, alpha=0.5, overlay_mask=nan[0])[0]
    pytest.importorskip("PIL")                                                            # the graph picture is drawn with PIL.ImageDraw
    sup_img, mask_img = te.plot_mission_node_training(n)
    assert torch.equal(torch.from_numpy(mask_img), want_mask)
    plain = VR.image_to_u8(img, True)[0]
    assert sup_img.shape == (H, H, 3) and sup_img.dtype.name == "uint8" and not torch.equal(torch.from_numpy(sup_img), plain)
    pos = n.feature_positions.cpu()                                                       # pixels no line or ellipse can reach:
    lo, hi = pos.min(0).values - 7, pos.max(0).values + 7
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(H), indexing="ij")
    outside = (xx < lo[0]) | (xx > hi[0]) | (yy < lo[1]) | (yy > hi[1])
    assert torch.equal(torch.from_numpy(sup_img)[outside], plain[outside])
    # checkpoints round-trip as before, and a pickled visualizer carries no device cache
    import pickle

    f = te.save_checkpoint(str(tmp_path))
    te2 = TraversabilityEstimator(p, device=dev, min_samples_for_training=2)
    te2.load_checkpoint(f)
    for k, v in te._model.state_dict().items():
        assert torch.equal(v, te2._model.state_dict()[k])
    assert pickle.loads(pickle.dumps(te._visualizer))._tables == {}
