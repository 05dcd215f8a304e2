"""csrc/resnet.hip and csrc/pyramid_pool.hip on the GPU against the float64 statement of tests/resnet_ref.py, and
FeatureExtractor(feature_type="torchvision") on top of both.

Gates, none of them taken from the kernels' output:
  * whole network and pooled means: per level (per block of the 960 columns) err = max|gpu - f64| / max|f64|.  The same statement is run on
    the CPU in fp32; the GPU may be at most 4 x as far from float64 as that run (both are fp32 chains that differ only in summation
    order, at K up to 4608).  The measured pairs are printed and recorded in DESIGN.md.
  * the stand-alone convolution: the forward error bound of an fp32 fmaf chain, elementwise.  With u = 2^-24 a chain of K products is
    within K u sum|a w| of the exact sum (Higham, gamma_K ~ K u); the epilogue adds one rounding each for the scale product, the shift
    and the residual, the folded terms carry one rounding each, and the stem's (v - mean) / std two roundings on v and one on each
    constant.  Bound = (K + 10) u (|scale| conv(|x| + c, |w|) + |shift| + |residual|), c = mean / std for the stem and 0 otherwise.
  * max-pool, fallback rows, uint8 twins, repeated runs, batch positions: bit for bit."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_ref as REF  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402
from wild_visual_navigation_amd.cfg import ExperimentParams  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor, TorchVisionInterface  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import torchvision_interface as TVI  # noqa: E402
from wild_visual_navigation_amd.model import SimpleMLP  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import MissionNode, TraversabilityEstimator  # noqa: E402
from wild_visual_navigation_amd.utils import Data  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FACTOR = 4.0


def g(seed):
    return torch.Generator().manual_seed(seed)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def rel_err(got, want):
    return ((got.double() - want).abs().max() / want.abs().max()).item()


# ---------------------------------------------------------------------------------------------------- convolution entry point
CONVS = {"3x3s1": (64, 128, 3, 1, 1), "3x3s2": (64, 128, 3, 2, 1), "1x1s2": (64, 128, 1, 2, 0), "stem7x7": (3, 64, 7, 2, 3)}
CONV_CASES = [(n, s) for n in CONVS for s in (9, 7)] + [("3x3s1", 16)]


@functools.lru_cache(maxsize=None)
def _conv_case(name, size):
    """Inputs and the float64 results of one configuration, computed once on the CPU and never modified."""
    cin, cout, k, stride, pad = CONVS[name]
    seed = size * 131 + k * 7 + stride
    stem = name.startswith("stem")
    x = torch.rand(2, cin, size, size, generator=g(seed)) if stem else torch.randn(2, cin, size, size, generator=g(seed))
    w = torch.randn(cout, cin, k, k, generator=g(seed + 1)) * (2.0 / (cin * k * k)) ** 0.5
    bn = (0.5 + torch.rand(cout, generator=g(seed + 2)), torch.randn(cout, generator=g(seed + 3)),
          torch.randn(cout, generator=g(seed + 4)), 0.5 + torch.rand(cout, generator=g(seed + 5)))
    oh = (size + 2 * pad - k) // stride + 1
    resid = torch.randn(2, cout, oh, oh, generator=g(seed + 6))
    xin = REF.normalize(x) if stem else x.double()
    want = {(r, a): REF.conv_bn_act(xin, w, bn, stride, pad, resid if r else None, a) for r in (False, True) for a in (False, True)}
    scale, shift = REF.bn_scale_shift(*bn)
    c = (torch.tensor(REF.MEAN) / torch.tensor(REF.STD)).double().view(1, 3, 1, 1) if stem else 0.0
    mag = F.conv2d(xin.abs() + c, w.double().abs(), stride=stride, padding=pad) * scale.abs().view(1, -1, 1, 1) + shift.abs().view(1, -1, 1, 1)
    bound = {r: (cin * k * k + 10) * U * (mag + (resid.double().abs() if r else 0.0)) for r in (False, True)}
    return x, w, bn, resid, want, bound


@pytest.mark.parametrize("name, size", CONV_CASES)
def test_convolution_against_float64(dev, name, size):
    cin, cout, k, stride, pad = CONVS[name]
    stem = name.startswith("stem")
    x, w, bn, resid, want, bound = _conv_case(name, size)
    packed = ops.conv2d_pack(w.to(dev))
    scale, shift = (t.to(dev) for t in ops.bn_scale_shift(*bn, REF.BN_EPS))
    xin = x.to(dev) if stem else nhwc(x).to(dev)
    for (r, a), ref in want.items():
        got = ops.conv2d_bn_act(xin, packed, scale, shift, k, stride, pad, residual=nhwc(resid).to(dev) if r else None, relu=a, frame=stem)
        assert got.shape == (2, ref.shape[2], ref.shape[3], cout)
        diff = (nchw(got.cpu()).double() - ref).abs()
        worst = (diff / bound[r]).max().item()
        print(f"conv {name} {size}x{size} residual={r} relu={a}: max|err| = {diff.max().item():.3e}, worst err / bound = {worst:.3f}")
        assert worst <= 1.0
    if stem:   # a uint8 frame gives the bits of its float() / 255 twin
        u8 = torch.randint(0, 256, x.shape, generator=g(size), dtype=torch.uint8)
        a = ops.conv2d_bn_act(u8.to(dev), packed, scale, shift, k, stride, pad, frame=True)
        b = ops.conv2d_bn_act((u8.float() / 255).to(dev), packed, scale, shift, k, stride, pad, frame=True)
        assert same_bits(a, b)


def test_convolution_bits_do_not_depend_on_the_batch(dev):
    x, w, bn, resid, _, _ = _conv_case("3x3s2", 9)
    packed = ops.conv2d_pack(w.to(dev))
    scale, shift = (t.to(dev) for t in ops.bn_scale_shift(*bn, REF.BN_EPS))
    both = ops.conv2d_bn_act(nhwc(x).to(dev), packed, scale, shift, 3, 2, 1)
    alone = ops.conv2d_bn_act(nhwc(x[1:]).to(dev), packed, scale, shift, 3, 2, 1)
    assert same_bits(both[1:], alone) and same_bits(both, ops.conv2d_bn_act(nhwc(x).to(dev), packed, scale, shift, 3, 2, 1))


@pytest.mark.parametrize("size", [9, 16])
def test_max_pool_pads_with_minus_infinity(dev, size):
    """All-negative input: a zero padding would win every border window."""
    x = -0.5 - torch.rand(2, 64, size, size, generator=g(size))
    want = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    got = nchw(ops.maxpool3x3s2(nhwc(x).to(dev)).cpu())
    assert (want < 0).all() and same_bits(got, want)


# ---------------------------------------------------------------------------------------------------- whole network
@functools.lru_cache(maxsize=None)
def _sd():
    return TVI.synthetic_resnet18_state_dict(0)


@functools.lru_cache(maxsize=None)
def _net_case(size):
    """(frames fp32 [3,3,S,S], float64 maps, yardstick per level: the fp32 CPU run's distance from float64)."""
    img = torch.rand(3, 3, size, size, generator=g(size))
    f64 = REF.resnet18(_sd(), img)
    f32 = REF.resnet18(_sd(), img, dtype=torch.float32)
    return img, f64, {k: rel_err(f32[k], f64[k]) for k in f64}


@functools.lru_cache(maxsize=None)
def _interface(size):
    return TorchVisionInterface("cuda:0", "resnet18", input_size=size, pretrained_weights=_sd())


@pytest.mark.parametrize("size", [64, 96])
def test_network_against_float64(dev, size):
    img, f64, yard = _net_case(size)
    net = _interface(size)
    got = net.inference(img.to(dev))
    assert list(got) == ["feat1", "feat2", "feat3", "feat4"]
    for l, (k, v) in enumerate(got.items()):
        s = REF.STRIDES[l]
        assert v.shape == (3, REF.CHANNELS[l], size // s, size // s) and v.dtype == torch.float32
        err = rel_err(v.cpu(), f64[k])
        print(f"resnet18 {size}^2 {k}: gpu err {err:.3e}, fp32 cpu err {yard[k]:.3e}, ratio {err / yard[k]:.2f}")
        assert err <= FACTOR * yard[k]
    # bits: a second run, frame 1 alone
    again = net.inference(img.to(dev))
    alone = net.inference(img[1:2].to(dev))
    for k in got:
        assert same_bits(got[k], again[k]) and same_bits(got[k][1:2], alone[k])


@pytest.mark.parametrize("size", [64, 96])
def test_network_on_a_uint8_frame(dev, size):
    net = _interface(size)
    u8 = torch.randint(0, 256, (1, 3, size, size), generator=g(size + 1), dtype=torch.uint8)
    f64 = REF.resnet18(_sd(), u8)
    f32 = REF.resnet18(_sd(), u8, dtype=torch.float32)
    got = net.inference(u8.to(dev))
    twin = net.inference((u8.float() / 255).to(dev))
    for k in got:
        err, yard = rel_err(got[k].cpu(), f64[k]), rel_err(f32[k], f64[k])
        print(f"resnet18 {size}^2 uint8 {k}: gpu err {err:.3e}, fp32 cpu err {yard:.3e}, ratio {err / yard:.2f}")
        assert err <= FACTOR * yard and same_bits(got[k], twin[k])


# ---------------------------------------------------------------------------------------------------- pooling
def _grid_map():
    return (torch.arange(64)[:, None] // 16) * 4 + torch.arange(64)[None] // 16


def _hand_map():
    """Ids 0..19 on 64 x 64: 0 the background; 1..15 single pixels at odd coordinates (absent from every level); 16 a block that
    touches the last row and column (present at strides 4 to 16, absent at 32); 17 without a pixel; 18 a 3 x 3 block between the
    stride-4 samples; 19 a block that holds a sample of every level; a patch and a sprinkle of -1."""
    seg = torch.zeros(64, 64, dtype=torch.int64)
    seg[0:8, 56:64] = -1
    seg[33, ::5] = -1
    seg[30:48, 30:48] = 19
    seg[48:64, 40:64] = 16
    seg[17:20, 21:24] = 18
    for i in range(1, 16):
        seg[2 * i + 1, (7 * i) % 29 * 2 + 1] = i
    return seg


@functools.lru_cache(maxsize=None)
def _pool_inputs():
    segs = torch.stack([_grid_map(), _hand_map()])
    assert (segs[0, ::32, ::32].unique().numel(), segs[0].max().item()) == (4, 15)      # 16 ids, 12 vanish at stride 32
    assert (segs[1] == 17).sum() == 0 and (segs[1] == -1).sum() > 64 and segs[1, 63, 63] == 16 and all((segs[1] == i).sum() == 1 for i in range(1, 16))
    return segs, 20


def test_pyramid_pooling_against_the_statement(dev):
    segs, S = _pool_inputs()
    net = _interface(64)
    img = torch.rand(2, 3, 64, 64, generator=g(11))
    levels = [m.clone() for m in net.forward_levels(img.to(dev))]                  # NHWC fp32 on the GPU
    cpu = [nchw(m.cpu()) for m in levels]
    feat = ops.segpool_pyramid(levels, segs.to(dev), S)
    assert feat.shape == (2, S, 960) and feat.dtype == torch.float32
    swapped = ops.segpool_pyramid([m.flip(0).contiguous() for m in levels], segs.flip(0).to(dev), S)
    assert same_bits(feat, ops.segpool_pyramid(levels, segs.to(dev), S)) and same_bits(feat, swapped.flip(0))
    n_fall = n_mean = 0
    for b in range(2):
        maps = [m[b] for m in cpu]
        want, fallback = REF.pyramid_pool(maps, segs[b], S)
        w32, _ = REF.pyramid_pool(maps, segs[b], S, dtype=torch.float32)
        present = torch.tensor([(segs[b] == i).any().item() for i in range(S)])
        n_fall += int(fallback.sum())
        n_mean += int((present[:, None] & ~fallback).sum())
        got = feat[b].cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isnan(got).all(1), ~present)
        col = 0
        for l, c in enumerate(REF.CHANNELS):
            blk = slice(col, col + c)
            rows = present & ~fallback[:, l]
            err, yard = rel_err(got[rows, blk], want[rows, blk]), rel_err(w32[rows, blk], want[rows, blk])
            print(f"pyramid pooling frame {b} level {l + 1}: gpu err {err:.3e}, fp32 cpu err {yard:.3e}")
            assert err <= FACTOR * yard
            fb = fallback[:, l]
            assert same_bits(got[fb, blk], want[fb, blk].float())                   # the level map's cell, bit for bit
            col += c
    # conditions on the inputs (the statement alone): both branches carry at least a third of the (segment, level) pairs
    assert 3 * n_fall >= n_fall + n_mean and 3 * n_mean >= n_fall + n_mean, (n_fall, n_mean)


# ---------------------------------------------------------------------------------------------------- classes
def _fe(dev, seg_type):
    return FeatureExtractor(dev, segmentation_type=seg_type, feature_type="torchvision", model_type="resnet18", input_size=64,
                            allow_synthetic=True, slic_num_components=16)


def _frames(golden, n=2):
    return golden("demo_frames_224.pt")["frames_u8"][:n, :, 80:144, 100:164].contiguous()


@pytest.mark.parametrize("seg_type", ["grid", "slic"])
def test_extract_matches_extract_batch(dev, golden, seg_type):
    fe = _fe(dev, seg_type)
    assert fe.feature_dim == 960 and fe.feature_type == "torchvision"
    frames = (_frames(golden).float() / 255).to(dev)
    fb, sb, nb = fe.extract_batch(frames, cell_size=16)
    assert fb.shape[0] == 2 and fb.shape[2] == 960 and sb.shape == (2, 64, 64) and sb.dtype == torch.int32 and nb.tolist() == [fb.shape[1]] * 2
    for b in range(2):
        edges, feat, seg, center, dense = fe.extract(frames[b:b + 1], cell_size=16, return_dense_features=True)
        assert seg.dtype == torch.int64 and torch.equal(seg, sb[b].long()) and edges.shape[0] == 2 and center.shape[1] == 2
        n = feat.shape[0]
        assert same_bits(feat, fb[b, :n]) and torch.isnan(fb[b, n:]).all()         # (slic: trailing cluster ids without a pixel)
        want = fe._extractor.inference(frames[b:b + 1])
        assert list(dense) == ["feat1", "feat2", "feat3", "feat4"] and all(same_bits(dense[k], want[k]) for k in want)
        assert dense["feat2"].shape == (1, 128, 8, 8)
        comp = fe.compute_features(frames[b:b + 1], seg, center)
        assert all(same_bits(comp[k], want[k]) for k in want)
        assert same_bits(fe.sparsify_features(dense, seg), feat)
        assert fe.extract(frames[b:b + 1], cell_size=16)[4] is None
    # the statement on the same maps
    levels = [m.clone() for m in fe._extractor.forward_levels(frames)]
    want, _ = REF.pyramid_pool([nchw(m.cpu())[0] for m in levels], sb[0].cpu(), fb.shape[1])
    ok = ~torch.isnan(want)
    assert torch.equal(torch.isnan(fb[0].cpu()), ~ok) and (fb[0].cpu().double()[ok] - want[ok]).abs().max().item() <= U * want[ok].abs().max().item()   # one rounding of an exact mean: half an ulp
    fe.change_device(dev)
    assert same_bits(fe.extract_batch(frames, cell_size=16)[0], fb)


def test_predict_per_segment_on_pyramid_features(dev, golden):
    """quick_start.py:184-210: feat[seg] -> model.forward -> column 0, against the fused per-segment kernel (the 1e-5 of
    tests/test_gpu_segment_predict.py)."""
    fe = _fe(dev, "grid")
    torch.manual_seed(5)
    model = SimpleMLP(960, [256, 32, 1], True).to(dev)
    model.eval()
    frames = _frames(golden).to(dev)
    trav, conf, loss, feat, seg, nseg = fe.predict_per_segment(frames, model, cell_size=16)
    assert trav.shape == (2, 64, 64) and feat.shape == (2, 16, 960)
    fb, sb, _ = fe.extract_batch(frames, cell_size=16)
    assert same_bits(feat, fb) and torch.equal(seg, sb)
    for b in range(2):
        pred = model.forward(Data(x=feat[b][seg[b].reshape(-1).long()]))
        assert (trav[b].reshape(-1) - pred[:, 0]).abs().max().item() <= 1e-5


def test_what_pyramid_features_cannot_serve_is_refused(dev, golden):
    fe = _fe(dev, "grid")
    model = SimpleMLP(960, [256, 32, 1], True).to(dev)
    frames = _frames(golden, 1).to(dev)
    for call in (lambda: fe.predict_per_pixel(frames, model), lambda: fe.predict_and_extract(frames, model), lambda: fe.backbone_stage(frames),
                 lambda: fe.extract_batch(frames, backbone_out=torch.zeros(1, 64, 960, device=dev))):
        with pytest.raises(_lib.WvnError, match="torchvision"):
            call()
    with pytest.raises(_lib.WvnError, match="input_size"):
        fe.extract_batch(torch.zeros(1, 3, 96, 96, device=dev))
    with pytest.raises(_lib.WvnError, match="model_type"):
        FeatureExtractor(dev, segmentation_type="grid", feature_type="torchvision", model_type="resnet50", input_size=64)


def test_three_training_steps_on_pyramid_rows(dev, golden):
    fe = _fe(dev, "grid")
    frames = _frames(golden).to(dev)
    feat, seg, _ = fe.extract_batch(frames, cell_size=16)
    p = ExperimentParams()
    p.model.simple_mlp_cfg.input_size = 960
    te = TraversabilityEstimator(p, device=dev, min_samples_for_training=2)
    gen = g(0)
    for i in range(4):
        n = MissionNode(timestamp=float(i))
        n.features = (feat[i % 2] * (1.0 + 0.01 * i)).contiguous()
        n.feature_segments = seg[i % 2].long()
        mask = torch.full((3, 64, 64), float("nan"))
        mask[:, :32] = 0.5 + 0.5 * torch.rand(3, 32, 64, generator=gen)
        assert te.add_mission_node(n)
        te.update_supervision(n, mask.to(dev))
        assert n.is_valid()
    losses = [te.train()["loss_total"] for _ in range(3)]
    print("pyramid rows, three training steps:", losses)
    assert all(torch.isfinite(torch.as_tensor(float(v))) for v in losses) and te.step == 3


def test_drop_in_import_line_resolves(dev):
    import wild_visual_navigation_amd.dropin as dropin

    dropin.install()
    from wild_visual_navigation.feature_extractor import TorchVisionInterface as Aliased

    assert Aliased is TorchVisionInterface
