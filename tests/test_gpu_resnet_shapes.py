"""csrc/resnet.hip and csrc/pyramid_pool.hip on the GPU away from square frames: the cases of tests/resnet_cases.py (whose conditions
tests/test_resnet_cases_host.py asserts on the CPU) against the float64 statement tests/resnet_ref.py, through the ops wrappers
directly (conv2d_pack / conv2d_bn_act, maxpool3x3s2, resnet18_pack / _workspace / _forward / _levels, segpool_pyramid).

Gates, none of them taken from the kernels' output:
  * convolution, random inputs: the forward error bound of tests/test_gpu_resnet.py unchanged, elementwise,
    (K + 10) 2^-24 (|scale| conv(|x| + c, |w|) + |shift| + |residual|); uint8 frames also give the bits of their float() / 255 twin.
  * convolution, exact twin: integer inputs, weights in {-1, 0, 1}, scale in {0.5, 1, 2, -1}, integer shift: no operation of the fp32
    chain rounds, the output equals the float64 statement.
  * max-pool: the bits of F.max_pool2d.
  * whole network: per level max|gpu - f64| / max|f64| <= 4 x the same figure of the fp32 CPU run of the statement; repeats, batch
    positions, uint8 twins and foreign workspaces bit for bit.
  * pooling on integer-valued level maps: float64 sums are exact in any order, so feat equals float(statement) bit for bit, NaN rows
    included; on randn maps the 4 x rule of tests/test_gpu_resnet.py."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_cases as RC  # noqa: E402
import resnet_ref as REF  # noqa: E402
from resnet_cases import nchw, nhwc  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import torchvision_interface as TVI  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0   # tests/test_gpu_resnet.py


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------- convolution
@pytest.mark.parametrize("case", RC.NHWC_CASES + RC.FRAME_CASES, ids=lambda c: c.name)
def test_convolution_against_float64(dev, case):
    stem = case.cin == 3
    OH, OW = RC.out_hw(case)
    for u8 in ((False, True) if stem else (False,)):
        x, w, bn, resid, want, bound = RC.conv_float_case(case.name, u8)
        packed = ops.conv2d_pack(w.to(dev))
        scale, shift = (t.to(dev) for t in ops.bn_scale_shift(*bn, REF.BN_EPS))
        xin = x.to(dev) if stem else nhwc(x).to(dev)
        worst = 0.0
        for (r, a), ref in want.items():
            got = ops.conv2d_bn_act(xin, packed, scale, shift, case.k, case.stride, case.pad, residual=nhwc(resid).to(dev) if r else None,
                                    relu=a, frame=stem)
            assert got.shape == (case.B, OH, OW, case.cout)
            ratio = ((nchw(got.cpu()).double() - ref).abs() / bound[r]).max().item()
            worst = max(worst, ratio)
            if u8:   # the same bits as the fp32 frame float() / 255
                twin = ops.conv2d_bn_act((x.float() / 255).to(dev), packed, scale, shift, case.k, case.stride, case.pad,
                                         residual=nhwc(resid).to(dev) if r else None, relu=a, frame=True)
                assert same_bits(got, twin)
        print(f"conv {case.name}{' uint8' if u8 else ''}: worst err / bound = {worst:.4f}")
        assert worst <= 1.0


@pytest.mark.parametrize("case", RC.NHWC_CASES, ids=lambda c: c.name)
def test_convolution_exact_twin(dev, case):
    x, w, scale, shift, resid, want = RC.conv_exact_case(case.name)
    packed = ops.conv2d_pack(w.to(dev))
    xin, rin = nhwc(x).to(dev), nhwc(resid).to(dev)
    for (r, a), ref in want.items():
        got = ops.conv2d_bn_act(xin, packed, scale.to(dev), shift.to(dev), case.k, case.stride, case.pad, residual=rin if r else None, relu=a)
        got = nchw(got.cpu()).double()
        wrong = int((got != ref).sum())
        assert got.shape == ref.shape and wrong == 0, f"{case.name} residual={r} relu={a}: {wrong} of {ref.numel()} elements differ"


@pytest.mark.parametrize("name", list(RC.CONV_REFUSALS))
def test_convolution_refusals(dev, name):
    cin, cout, k, stride, pad, frame = RC.CONV_REFUSALS[name]
    x = torch.zeros((2, cin, 10, 15) if frame else (2, 10, 15, cin), device=dev)
    kpad = (cin * k * k + 31) // 32 * 32
    ones = torch.ones(cout, device=dev)
    with pytest.raises(_lib.WvnError):
        ops.conv2d_bn_act(x, torch.zeros(kpad, cout, device=dev), ones, ones, k, stride, pad, frame=frame)
    if name == "k8":
        with pytest.raises(_lib.WvnError):
            ops.conv2d_pack(torch.zeros(cout, cin, 8, 8, device=dev))


# ---------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("H, W, Cc", RC.MAXPOOL_SHAPES)
def test_max_pool_on_rectangles(dev, H, W, Cc):
    """All-negative input, so that a zero padding would win every border window.  NaN inputs are out of scope: the kernel keeps the
    best value with ``v > best``, which a NaN never wins, while torch propagates it -- by design of the comparison."""
    x, want = RC.maxpool_case(H, W, Cc)
    got = ops.maxpool3x3s2(nhwc(x).to(dev))
    assert got.shape == (2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc) and same_bits(nchw(got.cpu()), want)


# ---------------------------------------------------------------------------------------------------- whole network
@functools.lru_cache(maxsize=None)
def _packed():
    sd = RC.net_state_dict()
    weights, scales, shifts = [], [], []
    for conv, bn in TVI.resnet18_conv_names():
        scale, shift = ops.bn_scale_shift(sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"], REF.BN_EPS)
        weights.append(sd[conv + ".weight"].cuda())
        scales.append(scale.cuda())
        shifts.append(shift.cuda())
    return ops.resnet18_pack(weights, scales, shifts)


def _forward(img, workspace=None):
    """The four level maps as copies (the views die with the workspace)."""
    levels, ws = ops.resnet18_forward(_packed(), img, workspace)
    return [m.clone() for m in levels]


@pytest.mark.parametrize("B, H, W", RC.NET_FRAMES)
def test_network_on_rectangular_frames(dev, B, H, W):
    img, f64, yard = RC.net_case(B, H, W)
    got = _forward(img.to(dev))
    for l, (k, ref) in enumerate(f64.items()):
        s = REF.STRIDES[l]
        assert got[l].shape == (B, H // s, W // s, REF.CHANNELS[l]) and got[l].dtype == torch.float32
        err = RC.rel_err(nchw(got[l].cpu()), ref)
        print(f"resnet18 [{B},3,{H},{W}] {k}: gpu err {err:.3e}, fp32 cpu err {yard[k]:.3e}, ratio {err / yard[k]:.2f}")
        assert err <= FACTOR * yard[k]
    # bits: a second run; the last frame of the batch alone; a workspace made for three frames (and full of NaN) serving the call
    again = _forward(img.to(dev))
    alone = _forward(img[B - 1:].to(dev))
    big = ops.resnet18_workspace(3, H, W, dev).fill_(float("nan"))
    assert big.numel() > ops.resnet18_workspace(1, H, W, dev).numel()
    foreign = _forward(img[:1].to(dev), big)
    for l in range(4):
        assert same_bits(got[l], again[l]) and same_bits(got[l][B - 1:], alone[l]) and same_bits(got[l][:1], foreign[l])


def test_network_on_a_rectangular_uint8_frame(dev):
    u8 = torch.randint(0, 256, (1, 3, 96, 64), generator=RC.g(97), dtype=torch.uint8)
    f64 = REF.resnet18(RC.net_state_dict(), u8)
    f32 = REF.resnet18(RC.net_state_dict(), u8, dtype=torch.float32)
    got = _forward(u8.to(dev))
    twin = _forward((u8.float() / 255).to(dev))
    for l, k in enumerate(f64):
        err, yard = RC.rel_err(nchw(got[l].cpu()), f64[k]), RC.rel_err(f32[k], f64[k])
        print(f"resnet18 [1,3,96,64] uint8 {k}: gpu err {err:.3e}, fp32 cpu err {yard:.3e}, ratio {err / yard:.2f}")
        assert err <= FACTOR * yard and same_bits(got[l], twin[l])


def test_network_refusals(dev):
    img = torch.zeros(1, 3, 64, 96, device=dev)
    need = ops.resnet18_workspace(1, 64, 96, dev).numel()
    with pytest.raises(_lib.WvnError, match="workspace"):
        ops.resnet18_forward(_packed(), img, torch.empty(need - 1, device=dev))
    with pytest.raises(_lib.WvnError, match="multiples of 32"):
        ops.resnet18_forward(_packed(), torch.zeros(1, 3, 48, 64, device=dev))
    with pytest.raises(_lib.WvnError, match="bad argument"):
        ops.resnet18_forward(_packed(), torch.zeros(1, 3, 48, 64, device=dev), torch.empty(1 << 22, device=dev))


# ---------------------------------------------------------------------------------------------------- pooling
def _pool(dev, levels, segs, S, dtype):
    return ops.segpool_pyramid([nhwc(m).to(dev) for m in levels], segs.to(dtype).to(dev), S)


@pytest.mark.parametrize("name", list(RC.POOL_FRAMES))
def test_pyramid_pooling_bit_for_bit_on_integer_maps(dev, name):
    segs, S, dtype, levels, want, fallback = RC.pool_case(name)
    B = segs.shape[0]
    feat = _pool(dev, levels, segs, S, dtype)
    assert feat.shape == (B, S, 960) and feat.dtype == torch.float32
    got, ref = feat.cpu(), want.float()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    wrong = (torch.nan_to_num(got, nan=0.0).view(torch.int32) != torch.nan_to_num(ref, nan=0.0).view(torch.int32))
    rows = sorted({(b, i) for b, i, _ in torch.nonzero(wrong).tolist()})
    assert not rows, f"{name}: {int(wrong.sum())} elements differ, (frame, id) rows {rows[:12]}"
    assert same_bits(feat, _pool(dev, levels, segs, S, dtype))                                  # a repeat run
    if B == 2:                                                                                   # batch positions swapped
        swapped = _pool(dev, [m.flip(0) for m in levels], segs.flip(0), S, dtype)
        assert same_bits(feat, swapped.flip(0))


def test_pyramid_pooling_on_randn_maps(dev):
    segs, S, dtype, levels, want, fallback = RC.pool_case("wide", "randn")
    got = _pool(dev, levels, segs, S, dtype).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    for b in range(2):
        w32, _ = REF.pyramid_pool([m[b] for m in levels], segs[b], S, dtype=torch.float32)
        present = ~torch.isnan(want[b]).all(1)
        col = 0
        for l, c in enumerate(REF.CHANNELS):
            blk = slice(col, col + c)
            rows = present & ~fallback[b, :, l]
            err, yard = RC.rel_err(got[b][rows, blk], want[b][rows, blk]), RC.rel_err(w32[rows, blk], want[b][rows, blk])
            print(f"pyramid pooling 256x288 frame {b} level {l + 1}: gpu err {err:.3e}, fp32 cpu err {yard:.3e}")
            assert err <= FACTOR * yard
            fb = fallback[b, :, l]
            assert same_bits(got[b][fb, blk], want[b][fb, blk].float())                          # the level map's cell, bit for bit
            col += c
