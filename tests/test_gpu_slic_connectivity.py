"""Connectivity enforcement on the GPU (csrc/slic_connectivity.hip, ops.slic_enforce_connectivity, ops.slic(enforce_connectivity=True),
FeatureExtractor(slic_enforce_connectivity=True)) against the plain statement of its definition (tests/slic_connectivity_ref.py).
Everything is integer: every comparison is bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_connectivity_ref as REF  # noqa: E402

from oracle import segments as OS, slic as OSL  # noqa: E402
from wild_visual_navigation_amd import ops  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor  # noqa: E402

pytestmark = pytest.mark.gpu

TH, TW = ops.SLIC_CC_TILE


def gpu(dev, labels, n_clusters, min_size):
    """One call, with the kernels' own end flag checked: no component is left waiting."""
    out, waiting = ops.slic_enforce_connectivity(torch.from_numpy(np.ascontiguousarray(labels)).to(dev), n_clusters, min_size,
                                                 return_waiting=True)
    assert int(waiting.abs().sum()) == 0, f"components left waiting: {waiting.tolist()}"
    return out.cpu().numpy()


def check(dev, labels, n_clusters, min_size, what):
    want = REF.enforce_connectivity(labels, min_size)
    got = gpu(dev, labels, n_clusters, min_size)
    assert got.dtype == np.int32 and got.shape == labels.shape
    assert np.array_equal(got, want), f"{what}: {(got != want).sum()} of {got.size} labels differ"
    return got


def random_with_blocks(seed):
    """Uniform random labels over 8 ids at 64 x 64 with two solid 16 x 16 blocks: with min_size 64 only the blocks are anchored."""
    L = np.random.default_rng(seed).integers(0, 8, size=(64, 64)).astype(np.int32)
    L[4:20, 4:20] = 0
    L[40:56, 36:52] = 5
    return L


def snake(H, W, seed):
    """Label 1 winds through the whole frame (every even row, joined at alternating ends), so one component crosses every border
    between tiles of the labelling kernel, in both directions; the rows in between hold random fragments of other ids."""
    L = np.random.default_rng(seed).choice(np.array([0, 2, 3], dtype=np.int32), size=(H, W))
    L[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        L[y, W - 1 if k % 2 == 0 else 0] = 1
    return L


def slic_map(golden, i):
    u8 = golden("demo_frames_224.pt")["frames_u8"][i, :, :, :224].contiguous()
    return u8, OSL.slic(u8.numpy(), 100, 10.0)


def test_hand_written_maps(dev):
    for name, labels, min_size, expected in REF.hand_cases():
        assert np.array_equal(gpu(dev, labels, 10, min_size), expected), name


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_long_chains_random_labels_two_anchors(dev, seed):
    L = random_with_blocks(seed)
    want, rounds = REF.enforce_connectivity(L, 64, return_rounds=True)
    print(f"seed {seed}: {REF.small_components(L, 64)} components below 64, {rounds} rounds")
    assert rounds >= 20                      # (measured 31 - 33) a fixed small number of rounds cannot pass
    got = gpu(dev, L, 8, 64)
    assert np.array_equal(got, want), f"{(got != want).sum()} labels differ"
    assert REF.small_components(got, 64) == 0


def test_slic_map_with_salt_noise(dev, golden):
    _, L = slic_map(golden, 2)
    rng = np.random.default_rng(7)
    L = L.copy()
    for _ in range(400):                     # islands of 1 - 3 pixels with arbitrary ids
        y, x, n, k = rng.integers(0, 223), rng.integers(0, 222), rng.integers(1, 4), rng.integers(0, 100)
        L[y, x:x + n] = k
    check(dev, L, 100, 125, "salted SLIC map")


@pytest.mark.parametrize("H,W", [(33, 47), (1, 130), (130, 1), (1, 1), (2, 3)])
def test_odd_sizes(dev, H, W):
    L = np.random.default_rng(H * 1000 + W).integers(0, 3, size=(H, W)).astype(np.int32)
    if H * W >= 64:
        L.reshape(-1)[: H * W // 3] = 1      # a long run that is anchored
    for min_size in (1, 2, 5, 40):
        check(dev, L, 3, min_size, f"{H}x{W} min_size {min_size}")


@pytest.mark.parametrize("H", [TH - 1, TH, TH + 1, 2 * TH + 1])
@pytest.mark.parametrize("W", [TW - 1, TW, TW + 1, 2 * TW + 1])
def test_sizes_around_the_labelling_tile_with_a_snake(dev, H, W):
    L = snake(H, W, H * 100 + W)
    comp, sizes = REF.components(L)
    assert sizes[comp[0, 0]] == (L == 1).sum()          # the snake is ONE component
    for min_size in (3, W):                              # W: every fragment between the snake's rows waits
        check(dev, L, 4, min_size, f"snake {H}x{W} min_size {min_size}")
        check(dev, np.ascontiguousarray(L.T), 4, min_size, f"snake {W}x{H} min_size {min_size}")


def test_slic_with_enforcement_on_demo_frames(dev, golden):
    for i in range(4):
        u8, L = slic_map(golden, i)
        want = REF.enforce_connectivity(L, 125)
        got = ops.slic(u8.to(dev), 100, 10.0, enforce_connectivity=True)
        assert got.shape == (224, 224) and got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), want), f"frame {i}: {(got.cpu().numpy() != want).sum()} labels differ"
        assert np.array_equal(ops.slic(u8.to(dev), 100, 10.0).cpu().numpy(), L)      # off: the k-means result as before


def test_slic_with_enforcement_at_448(dev, golden):
    u8 = golden("graph_img_448.pt")["frame_u8"]
    u8 = u8.reshape(-1, *u8.shape[-2:])[:3, :448, :448].contiguous()
    L = OSL.slic(u8.numpy(), 100, 10.0)
    K = ops.slic_num_clusters(448, 448, 100)
    min_size = REF.min_size_for(448, 448, K)
    assert min_size == ops.slic_min_size(448, 448, K) == 501
    want = REF.enforce_connectivity(L, min_size)
    got = ops.slic(u8.to(dev), 100, 10.0, enforce_connectivity=True).cpu().numpy()
    assert np.array_equal(got, want), f"{(got != want).sum()} labels differ"
    # another factor reaches the kernel
    got = ops.slic(u8.to(dev), 100, 10.0, enforce_connectivity=True, min_size_factor=0.05).cpu().numpy()
    assert np.array_equal(got, REF.enforce_connectivity(L, REF.min_size_for(448, 448, K, 0.05)))


def test_batch_in_place_and_repeatability(dev, golden):
    maps = [slic_map(golden, i)[1] for i in range(4)]
    maps.append(np.random.default_rng(11).integers(0, 100, size=(224, 224)).astype(np.int32))
    maps[-1][50:120, 30:90] = 17
    batch = torch.from_numpy(np.stack(maps)).to(dev)
    singles = [ops.slic_enforce_connectivity(batch[b], 100, 125) for b in range(5)]
    out, waiting = ops.slic_enforce_connectivity(batch, 100, 125, return_waiting=True)
    assert out.shape == (5, 224, 224) and int(waiting.abs().sum()) == 0
    for b in range(5):
        assert torch.equal(out[b], singles[b]), b
    assert np.array_equal(out[4].cpu().numpy(), REF.enforce_connectivity(maps[4], 125))
    assert torch.equal(out, ops.slic_enforce_connectivity(batch, 100, 125))                     # two runs are identical
    # the same map at different batch positions
    perm = [3, 0, 4, 1, 2, 3, 3]
    outp = ops.slic_enforce_connectivity(batch[perm].contiguous(), 100, 125)
    for j, b in enumerate(perm):
        assert torch.equal(outp[j], singles[b]), (j, b)
    # in place
    work = batch.clone()
    ret = ops.slic_enforce_connectivity(work, 100, 125, out=work)
    assert ret.data_ptr() == work.data_ptr() and torch.equal(work, out)
    # ops.slic on a batch of frames == the single calls
    frames = golden("demo_frames_224.pt")["frames_u8"][:, :, :, :224].contiguous().to(dev)
    for flag in (False, True):
        sb = ops.slic(frames, 100, 10.0, enforce_connectivity=flag)
        assert sb.shape == (4, 224, 224)
        for b in range(4):
            assert torch.equal(sb[b], ops.slic(frames[b], 100, 10.0, enforce_connectivity=flag)), (flag, b)


def test_feature_extractor_with_and_without_enforcement(dev, golden):
    u8 = golden("graph_img_448.pt")["frame_u8"]
    u8 = u8.reshape(-1, *u8.shape[-2:])[:3, :448, :448].contiguous()
    img = (u8.float() / 255)[None].to(dev)
    L = OSL.slic(img[0].cpu().numpy(), 100, 10.0)
    K = ops.slic_num_clusters(448, 448, 100)
    want = torch.from_numpy(REF.enforce_connectivity(L, REF.min_size_for(448, 448, K))).long()

    fe = FeatureExtractor(dev, slic_enforce_connectivity=True, allow_synthetic=True)
    assert fe.segmentation_type == "slic"
    edges, feat, seg, center, _ = fe.extract(img)
    assert seg.dtype == torch.int64 and torch.equal(seg.cpu(), want)
    assert torch.equal(edges.cpu(), OS.adjacency_list(want[None, None]).T)
    assert torch.allclose(center.cpu(), OS.centers(want[None, None]), atol=1e-4, equal_nan=True)
    assert feat.shape == (center.shape[0], fe.feature_dim)
    fb, sb, nb = fe.extract_batch(img.expand(3, -1, -1, -1).contiguous())
    assert sb.shape == (3, 448, 448) and fb.shape[:2] == (3, K) and nb.tolist() == [K] * 3
    for b in range(3):
        assert torch.equal(sb[b].long().cpu(), want), b

    from oracle import mlp as OM
    from wild_visual_navigation_amd.cfg import ExperimentParams
    from wild_visual_navigation_amd.model import get_model

    params = ExperimentParams()
    params.model.simple_mlp_cfg.input_size = fe.feature_dim
    model = get_model(params.model).to(dev)
    model.eval()
    model.load_state_dict(OM.make_mlp_state_dict(fe.feature_dim, seed=3), strict=False)
    trav, conf, _, featp, segp, _ = fe.predict_per_segment(img.expand(2, -1, -1, -1).contiguous(), model)
    assert trav.shape == (2, 448, 448) and conf.shape == (2, 448, 448) and torch.equal(segp[1].long().cpu(), want)
    assert torch.isfinite(trav).all()
    # a segment's prediction is constant on the segment
    ids = segp[0].reshape(-1).long()
    first = torch.zeros(K, device=dev).scatter_(0, ids, trav[0].reshape(-1))
    assert torch.equal(first[ids], trav[0].reshape(-1))

    # the switch off (the default): today's map, oracle/slic.py alone
    off = FeatureExtractor(dev, allow_synthetic=True)
    _, _, seg0, _, _ = off.extract(img)
    assert torch.equal(seg0.cpu(), torch.from_numpy(L).long())
    _, sb0, _ = off.extract_batch(img.expand(2, -1, -1, -1).contiguous())
    assert torch.equal(sb0[0].long().cpu(), torch.from_numpy(L).long()) and torch.equal(sb0[1], sb0[0])
