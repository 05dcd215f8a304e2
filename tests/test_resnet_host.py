"""The ResNet-18 pyramid without a GPU: the float64 statement (tests/resnet_ref.py) against itself -- its pooling against a naive
per-segment loop over F.interpolate'd maps, its fallback cell against a map worked out by hand, BatchNorm's folded scale / shift
against F.batch_norm -- and the host logic: state-dict keys, the refusals (each raised before anything touches a GPU), the C entry
points' argument checks."""
import ctypes as C
import os
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_ref as REF  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor, TorchVisionInterface  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import torchvision_interface as TVI  # noqa: E402


def g(seed):
    return torch.Generator().manual_seed(seed)


def _levels(H, W, seed, dtype=torch.float64):
    return [torch.randn(c, H // s, W // s, generator=g(seed + s), dtype=dtype) for c, s in zip(REF.CHANNELS, REF.STRIDES)]


# ------------------------------------------------------------------------------------------ the statement against itself
def test_pooling_equals_a_naive_loop_where_no_segment_vanishes():
    """32-pixel grid cells on a 96 x 64 frame: every id keeps a cell at every stride, so the published loop runs as it stands."""
    H, W, cell = 96, 64, 32
    seg = (torch.arange(H)[:, None] // cell) * (W // cell) + torch.arange(W)[None] // cell
    S = int(seg.max()) + 1
    levels = _levels(H, W, 0)
    got, fallback = REF.pyramid_pool(levels, seg, S)
    assert got.shape == (S, 960) and not fallback.any() and torch.isfinite(got).all()
    col = 0
    for m, s in zip(levels, REF.STRIDES):
        seg_s = F.interpolate(seg[None, None].double(), scale_factor=1 / s)[0, 0].long()
        for i in range(S):
            ys, xs = torch.nonzero(seg_s == i, as_tuple=True)
            acc = torch.zeros(m.shape[0], dtype=torch.float64)
            for y, x in zip(ys.tolist(), xs.tolist()):
                acc += m[:, y, x]
            assert (got[i, col: col + m.shape[0]] - acc / len(ys)).abs().max().item() <= 1e-14
        col += m.shape[0]


def test_fallback_cell_by_hand():
    """Three segments on a 32 x 64 map.  Id 1 is the single pixel (5, 7): on no stride's sample lattice, centroid (5, 7) -> cells
    (1, 1), (0, 0), (0, 0), (0, 0).  Id 2 is the last two rows and columns' corner block rows 30-31 x columns 62-63: absent from every
    lattice too (the last samples are row 28 / column 60), centroid (30, 62) -> cells (7, 15), (3, 7), (1, 3), (0, 1): the last cell of
    every grid.
    Id 0 is everything else and is present at every level.  Id 3 has no pixel: NaN."""
    H, W = 32, 64
    seg = torch.zeros(H, W, dtype=torch.int64)
    seg[5, 7] = 1
    seg[30:, 62:] = 2
    levels = _levels(H, W, 1)
    feat, fallback = REF.pyramid_pool(levels, seg, 4)
    assert REF.centroid(seg, 1) == (5, 7) and REF.centroid(seg, 2) == (30, 62) and REF.centroid(seg, 3) is None
    assert fallback.tolist() == [[False] * 4, [True] * 4, [True] * 4, [False] * 4]
    cells = {1: [(1, 1), (0, 0), (0, 0), (0, 0)], 2: [(7, 15), (3, 7), (1, 3), (0, 1)]}
    col = 0
    for l, m in enumerate(levels):
        for i, cs in cells.items():
            assert torch.equal(feat[i, col: col + m.shape[0]], m[:, cs[l][0], cs[l][1]])
        col += m.shape[0]
    assert torch.isnan(feat[3]).all() and torch.isfinite(feat[:3]).all()
    # id 0 at stride 32: the one sample (0, 0) of the 1 x 2 grid's first cell and (0, 32) of the second, both id 0
    assert (feat[0, 448:] - levels[3].reshape(512, -1).mean(1)).abs().max().item() <= 1e-14


def test_negative_ids_are_ignored():
    H, W = 32, 32
    seg = torch.zeros(H, W, dtype=torch.int64)
    seg[::4, ::4] = -1          # every sample of every lattice
    seg[0, 0] = 0
    levels = _levels(H, W, 2)
    feat, fallback = REF.pyramid_pool(levels, seg, 1)
    assert not fallback.any()   # id 0 keeps the cell (0, 0) at every level: its row is that cell's vector
    assert torch.equal(feat[0, :64], levels[0][:, 0, 0]) and torch.equal(feat[0, 448:], levels[3][:, 0, 0])


def test_bn_scale_shift_equals_batch_norm():
    Cc = 16
    w, b = 0.5 + torch.rand(Cc, generator=g(3)), torch.randn(Cc, generator=g(4))
    m, v = torch.randn(Cc, generator=g(5)), 0.5 + torch.rand(Cc, generator=g(6))
    x = torch.randn(2, Cc, 5, 7, generator=g(7), dtype=torch.float64)
    want = F.batch_norm(x, m.double(), v.double(), w.double(), b.double(), training=False, eps=REF.BN_EPS)
    scale, shift = REF.bn_scale_shift(w, b, m, v)
    assert (x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) - want).abs().max().item() <= 1e-13
    s32, h32 = ops.bn_scale_shift(w, b, m, v, REF.BN_EPS)   # what the kernels are given: the float64 terms rounded once
    assert s32.dtype == torch.float32 and torch.equal(s32, scale.float()) and torch.equal(h32, shift.float())


def test_network_statement_shapes_and_uint8():
    sd = TVI.synthetic_resnet18_state_dict(0)
    img = torch.randint(0, 256, (1, 3, 64, 64), generator=g(8), dtype=torch.uint8)
    out = REF.resnet18(sd, img)
    assert list(out) == ["feat1", "feat2", "feat3", "feat4"]
    assert [tuple(v.shape) for v in out.values()] == [(1, 64, 16, 16), (1, 128, 8, 8), (1, 256, 4, 4), (1, 512, 2, 2)]
    twin = REF.resnet18(sd, img.float() / 255)
    assert all((out[k] - twin[k]).abs().max().item() <= 1e-6 * out[k].abs().max().item() for k in out)
    assert all(v.dtype == torch.float64 and (v >= 0).all() and v.max() > 0 for v in out.values())


# ------------------------------------------------------------------------------------------ host logic
def test_state_dict_keys():
    sd = TVI.synthetic_resnet18_state_dict(0)
    names = TVI.resnet18_conv_names()
    assert len(names) == ops.RESNET18_NCONV == 20 and len(sd) == 100
    assert "layer1.0.downsample.0.weight" not in sd and sd["layer3.0.downsample.0.weight"].shape == (256, 128, 1, 1)
    # synthetic BatchNorm is not the identity: running statistics and affine terms all vary
    for p in ("weight", "bias", "running_mean", "running_var"):
        assert sd[f"layer2.1.bn2.{p}"].std().item() > 0.05
    full = dict(sd)
    full["fc.weight"], full["fc.bias"] = torch.zeros(1000, 512), torch.zeros(1000)
    full["bn1.num_batches_tracked"] = torch.tensor(7)
    full = {"module." + k: v for k, v in full.items()}           # a DataParallel checkpoint
    loaded = TVI.load_resnet18_state_dict(full)
    assert list(loaded) == list(sd) and all(torch.equal(loaded[k], sd[k]) for k in sd)
    broken = dict(sd)
    del broken["layer4.0.downsample.1.running_var"]
    with pytest.raises(_lib.WvnError, match=r"layer4\.0\.downsample\.1\.running_var"):
        TVI.load_resnet18_state_dict(broken)
    broken = dict(sd)
    broken["layer2.0.conv1.weight"] = torch.zeros(128, 128, 3, 3)
    with pytest.raises(_lib.WvnError, match=r"layer2\.0\.conv1\.weight"):
        TVI.load_resnet18_state_dict(broken)
    with pytest.raises(_lib.WvnError, match="pretrained_weights"):
        TVI.load_resnet18_state_dict(3)


def test_checkpoint_path_loads(tmp_path):
    sd = TVI.synthetic_resnet18_state_dict(1)
    f = str(tmp_path / "resnet18.pth")
    torch.save(sd, f)
    t = TorchVisionInterface("cuda", "resnet18", input_size=64, pretrained_weights=f)
    assert all(torch.equal(t._state_dict[k], sd[k]) for k in sd) and t._packed is None   # construction is host-only


def test_synthetic_weights_warn_unless_allowed():
    with pytest.warns(UserWarning, match="SYNTHETIC"):
        TorchVisionInterface("cuda", "resnet18", input_size=64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t = TorchVisionInterface("cuda", "resnet18", input_size=64, allow_synthetic=True)
    assert t.input_size == 64 and t.model_type == "resnet18" and t.feature_dim == 960


def _fe(**kw):
    a = dict(device="cuda", segmentation_type="grid", feature_type="torchvision", model_type="resnet18", input_size=64, allow_synthetic=True)
    a.update(kw)
    return FeatureExtractor(**a)


@pytest.mark.parametrize("kw, word", [
    (dict(model_type="resnet50"), "model_type"), (dict(model_type="efficientnet_b0"), "model_type"),
    (dict(input_size=100), "input_size"), (dict(input_size=0), "input_size"),
    (dict(segmentation_type="random"), "segmentation_type"), (dict(segmentation_type="stego"), "segmentation_type"),
    (dict(segmentation_type="none"), "segmentation_type"), (dict(device="cpu"), "device"),
])
def test_constructor_refusals(kw, word):
    """Raised before anything is moved to a GPU: this machine has none."""
    with pytest.raises(_lib.WvnError, match=word):
        _fe(**kw)
    if word in ("model_type", "input_size", "device"):
        a = dict(device="cuda", model_type="resnet18", input_size=64, allow_synthetic=True)
        a.update(kw)
        with pytest.raises(_lib.WvnError, match=word):
            TorchVisionInterface(**a)


def _host_extractor():
    """A FeatureExtractor(feature_type="torchvision") without its GPU members: what the method-level refusals may touch."""
    fe = FeatureExtractor.__new__(FeatureExtractor)
    fe._device = torch.device("cuda")
    fe._feature_type = "torchvision"
    fe._segmentation_type = "grid"
    fe._feature_dim = 960
    fe._extractor = TorchVisionInterface("cuda", "resnet18", input_size=64, allow_synthetic=True)
    return fe


def test_method_refusals_before_any_launch():
    fe = _host_extractor()
    img = torch.zeros(1, 3, 64, 64)
    for call in (lambda: fe.backbone_stage(img), lambda: fe.predict_per_pixel(img, None), lambda: fe.predict_and_extract(img, None),
                 lambda: fe.extract_batch(img, backbone_out=torch.zeros(1, 4, 960))):
        with pytest.raises(_lib.WvnError, match="torchvision"):
            call()
    for bad in (torch.zeros(1, 3, 64, 96), torch.zeros(1, 3, 32, 32), torch.zeros(1, 1, 64, 64)):
        with pytest.raises(_lib.WvnError, match="input_size"):
            fe.extract(bad)
        with pytest.raises(_lib.WvnError, match="input_size"):
            fe.extract_batch(bad)
        with pytest.raises(_lib.WvnError, match="input_size"):
            fe._extractor.inference(bad)


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    h = _lib.lib()
    words = (C.c_longlong * 64)()
    p = C.addressof(words)   # never dereferenced: every call below is refused first
    assert h.wvn_conv2d_pack_floats(64, 3, 7) == 160 * 64 and h.wvn_conv2d_pack_floats(128, 64, 3) == 576 * 128
    assert h.wvn_conv2d_pack_floats(64, 64, 8) == 0 and h.wvn_conv2d_pack_floats(0, 64, 3) == 0
    ok = dict(B=2, H=9, W=9, Cin=64, Cout=128, k=3, stride=1, pad=1, kind=ops.CONV_IN_NHWC, inp=p)

    def conv(**kw):
        a = dict(ok)
        a.update(kw)
        return h.wvn_conv2d_bn_act(a["inp"], a["kind"], p, p, p, None, 1, p, a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["k"],
                                   a["stride"], a["pad"], None)

    for bad in (dict(inp=None), dict(B=0), dict(Cin=48), dict(Cout=96), dict(k=8), dict(k=0), dict(stride=3), dict(pad=4), dict(kind=3),
                dict(kind=ops.CONV_IN_FRAME_F32), dict(kind=ops.CONV_IN_FRAME_U8, Cin=4), dict(H=1, W=1, k=5, pad=1)):
        assert conv(**bad) == _lib.ERR_ARG, bad
    assert h.wvn_conv2d_pack(None, p, 64, 64, 3, None) == _lib.ERR_ARG and h.wvn_conv2d_pack(p, p, 64, 64, 9, None) == _lib.ERR_ARG
    assert h.wvn_maxpool3x3s2(None, p, 1, 8, 8, 64, None) == _lib.ERR_ARG and h.wvn_maxpool3x3s2(p, p, 1, 0, 8, 64, None) == _lib.ERR_ARG
    # the whole network
    floats = sum(h.wvn_conv2d_pack_floats(*TVI.resnet18_conv_shapes()[c][:3]) + 2 * TVI.resnet18_conv_shapes()[c][0]
                 for c, _ in TVI.resnet18_conv_names())
    assert h.wvn_resnet18_pack_bytes() == 4 * floats
    assert h.wvn_resnet18_workspace_bytes(1, 100, 64) == 0 and h.wvn_resnet18_workspace_bytes(0, 64, 64) == 0
    lv = [2 * (64 // s) * (64 // s) * c * 4 for c, s in zip(REF.CHANNELS, REF.STRIDES)]
    assert [h.wvn_resnet18_level_offset(2, 64, 64, l) for l in (1, 2, 3, 4)] == [0, lv[0], lv[0] + lv[1], lv[0] + lv[1] + lv[2]]
    assert h.wvn_resnet18_workspace_bytes(2, 64, 64) == sum(lv) + 5 * lv[0]
    assert h.wvn_resnet18_forward(p, p, 0, 1, 64, 48, p, 1 << 30, None) == _lib.ERR_ARG
    assert h.wvn_resnet18_forward(None, p, 0, 1, 64, 64, p, 1 << 30, None) == _lib.ERR_ARG
    assert h.wvn_resnet18_forward(p, p, 0, 1, 64, 64, p, 16, None) == 1002
    assert h.wvn_resnet18_pack(None, p, p, p, 1 << 30, None) == _lib.ERR_ARG and h.wvn_resnet18_pack(p, p, p, p, 16, None) == _lib.ERR_ARG
    # the pooling
    assert h.wvn_segpool_pyramid_scratch_bytes(2, 16) == 2 * 16 * 40 and h.wvn_segpool_pyramid_scratch_bytes(2, 0) == 0
    assert h.wvn_segpool_pyramid(p, p, p, p, p, p, p, 1 << 20, 2, 64, 48, 16, None) == _lib.ERR_ARG
    assert h.wvn_segpool_pyramid(p, p, p, None, p, p, p, 1 << 20, 2, 64, 64, 16, None) == _lib.ERR_ARG
    assert h.wvn_segpool_pyramid(p, p, p, p, p, p, p, 1 << 20, 2, 64, 64, 0, None) == _lib.ERR_ARG
    assert h.wvn_segpool_pyramid(p, p, p, p, p, p, p, 8, 2, 64, 64, 16, None) == 1002
    assert all(w == 0 for w in words)


def test_ops_refuse_cpu_tensors():
    with pytest.raises(_lib.WvnError):
        ops.conv2d_pack(torch.zeros(64, 64, 3, 3))
    with pytest.raises(_lib.WvnError):
        ops.maxpool3x3s2(torch.zeros(1, 8, 8, 64))
    with pytest.raises(_lib.WvnError):
        ops.resnet18_forward(torch.zeros(8), torch.zeros(1, 3, 64, 64))
    with pytest.raises(_lib.WvnError):
        ops.segpool_pyramid([torch.zeros(1, 16, 16, 64)] * 4, torch.zeros(1, 64, 64, dtype=torch.int32), 4)


def test_drop_in_import_line_resolves():
    import wild_visual_navigation_amd.dropin as dropin

    dropin.install()
    from wild_visual_navigation.feature_extractor import TorchVisionInterface as Aliased

    assert Aliased is TorchVisionInterface
