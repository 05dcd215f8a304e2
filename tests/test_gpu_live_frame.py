"""The live node's image callback with prediction_per_pixel from ONE backbone pass (wvn_feature_extractor_node.py:305-393):
FeatureExtractor.predict_and_extract against its two halves, predict_per_pixel and extract_batch, bit for bit, with the backbone
runs counted; and extract_batch's random segmentation (ops.random_pixels + ops.gather_bilinear) against the dense map it samples."""
import pytest
import torch

from oracle import mlp as OM, vit as OV
from wild_visual_navigation_amd import _lib, ops
from wild_visual_navigation_amd.backbone import VitBackbone
from wild_visual_navigation_amd.cfg import ExperimentParams
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor
from wild_visual_navigation_amd.model import DoubleMLP, get_model
from wild_visual_navigation_amd.utils import ConfidenceGenerator

pytestmark = pytest.mark.gpu

S, B, NR = 64, 2, 23   # input_size 64 at patch 8: an 8 x 8 token grid


def g(seed):
    return torch.Generator().manual_seed(seed)


def _extractor(dev, ftype, seg, prec, **kw):
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=11, depth=2)
    return FeatureExtractor(device=dev, segmentation_type=seg, feature_type=ftype, patch_size=8, backbone_type="vit_small", input_size=S,
                            pretrained_weights=sd, precision=prec, n_image_clusters=5, allow_synthetic=True, **kw)


def _model(dev, D, seed=7):
    params = ExperimentParams()
    params.model.simple_mlp_cfg.input_size = D
    model = get_model(params.model).to(dev)
    model.eval()
    model.load_state_dict(OM.make_mlp_state_dict(D, seed=seed), strict=False)
    return model


def _cg(dev):
    cg = ConfidenceGenerator(method="latest_measurement", std_factor=0.5).to(dev)
    cg.mean[0], cg.std[0] = 0.9, 0.25
    return cg


def _img(dev):
    return torch.rand(B, 3, S, S, generator=g(12)).to(dev)


@pytest.fixture
def backbone_runs(monkeypatch):
    """Counts the calls of VitBackbone.forward_tokens and VitBackbone.forward_tokens_pair: every backbone pass is one of them."""
    calls = []
    one, pair = VitBackbone.forward_tokens, VitBackbone.forward_tokens_pair

    def count_one(self, *a, **k):
        calls.append("forward_tokens")
        return one(self, *a, **k)

    def count_pair(self, *a, **k):
        calls.append("forward_tokens_pair")
        return pair(self, *a, **k)

    monkeypatch.setattr(VitBackbone, "forward_tokens", count_one)
    monkeypatch.setattr(VitBackbone, "forward_tokens_pair", count_pair)
    return calls


def _same(a, b):
    """torch.equal with NaN rows (ids that do not occur in an image: the reference's empty mean) in the same places."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.parametrize("ftype,seg,prec", [
    ("dino", "grid", "mixed"),
    ("dino", "random", "bf16"),
    ("stego", "stego", "mixed"),
    ("stego", "random", "fp16"),
    ("dino", "slic", "mixed"),
])
def test_one_pass_equals_the_two_calls(dev, backbone_runs, ftype, seg, prec):
    kw = {"random_seed": 5} if seg == "random" else {}
    call_kw = {"n_random_pixels": NR, "frame_index": 40} if seg == "random" else {}
    fe = _extractor(dev, ftype, seg, prec, **kw)
    two = _extractor(dev, ftype, seg, prec, **kw) if seg == "random" else fe   # (random: the pair comes from a second extractor, same seed)
    model, cg, img = _model(dev, fe.feature_dim), _cg(dev), _img(dev)

    del backbone_runs[:]
    trav, conf, loss, feat, segm, nseg = fe.predict_and_extract(img, model, cg, want_loss=True, **call_kw)
    assert len(backbone_runs) == 1, backbone_runs
    if ftype == "stego":
        assert backbone_runs == ["forward_tokens_pair"]          # flip TTA: the frames and their mirrors in one paired run

    del backbone_runs[:]
    t2, c2, l2 = two.predict_per_pixel(img, model, cg, want_loss=True)
    f2, s2, n2 = two.extract_batch(img, **call_kw)
    assert len(backbone_runs) == 2, backbone_runs

    assert trav.shape == (B, S, S) and torch.isfinite(trav).all() and torch.isfinite(conf).all()
    assert torch.equal(trav, t2) and torch.equal(conf, c2) and torch.equal(loss, l2)
    assert segm.dtype == torch.int32 and segm.shape == (B, S, S)
    assert torch.equal(segm, s2) and torch.equal(nseg, n2)
    assert torch.isfinite(feat).any() and _same(feat, f2)
    if seg == "random":
        assert feat.shape == (B, NR, fe.feature_dim) and (nseg == NR).all() and torch.isfinite(feat).all()


def test_one_pass_without_loss_or_confidence_generator(dev):
    fe = _extractor(dev, "dino", "grid", "bf16")
    model, img = _model(dev, fe.feature_dim), _img(dev)
    trav, conf, loss, feat, segm, nseg = fe.predict_and_extract(img, model)
    t2, c2, l2 = fe.predict_per_pixel(img, model)
    assert loss is None and l2 is None
    assert torch.equal(trav, t2) and torch.equal(conf, c2)
    f2, s2, n2 = fe.extract_batch(img)
    assert _same(feat, f2) and torch.equal(segm, s2) and torch.equal(nseg, n2)


def test_double_mlp_is_refused_before_the_backbone_runs(dev, backbone_runs):
    fe = _extractor(dev, "dino", "grid", "mixed")
    m = DoubleMLP(fe.feature_dim, [64, 32, 1]).to(dev)
    del backbone_runs[:]
    with pytest.raises(_lib.WvnError, match="DoubleMLP"):
        fe.predict_and_extract(_img(dev), m)
    assert backbone_runs == []


@pytest.mark.parametrize("ftype,prec", [("dino", "mixed"), ("stego", "bf16")])
def test_random_extract_batch_samples_the_dense_map(dev, ftype, prec):
    fe = _extractor(dev, ftype, "random", prec, random_seed=3)
    img = _img(dev)
    G, D = S // 8, fe.feature_dim
    tokens = fe.backbone_stage(img)
    dense = ops.upsample_bilinear(tokens, G, S).reshape(B, D, S * S)
    feat, seg, nseg = fe.extract_batch(img, n_random_pixels=NR)
    assert feat.shape == (B, NR, D) and seg.shape == (B, S, S) and seg.dtype == torch.int32
    assert nseg.dtype == torch.int32 and nseg.tolist() == [NR] * B
    for b in range(B):
        flat = seg[b].reshape(-1)
        px = torch.nonzero(flat >= 0).reshape(-1)
        assert px.numel() == NR and (flat[flat < 0] == -1).all()
        assert torch.equal(flat[px].sort().values, torch.arange(NR, dtype=torch.int32, device=dev))
        want = torch.empty(NR, D, device=dev)
        want[flat[px].long()] = dense[b][:, px].T                # sample j sits at the pixel that carries id j
        assert torch.equal(feat[b], want)


def test_random_draws_advance_and_reproduce(dev):
    fe = _extractor(dev, "dino", "random", "bf16", random_seed=9)
    img = _img(dev)
    tokens = fe.backbone_stage(img)
    # the internal counter starts at 0 and advances by B per call
    _, s0, _ = fe.extract_batch(img, backbone_out=tokens, n_random_pixels=NR)
    _, s1, _ = fe.extract_batch(img, backbone_out=tokens, n_random_pixels=NR)
    assert not torch.equal(s0, s1) and not torch.equal(s0[0], s0[1])
    f0, r0, _ = fe.extract_batch(img, backbone_out=tokens, n_random_pixels=NR, frame_index=0)
    f1, r1, _ = fe.extract_batch(img, backbone_out=tokens, n_random_pixels=NR, frame_index=B)
    assert torch.equal(r0, s0) and torch.equal(r1, s1)
    # an explicit frame index leaves the counter alone: the next call is frames 2B, 2B + 1
    _, s2, _ = fe.extract_batch(img, backbone_out=tokens, n_random_pixels=NR)
    _, r2, _ = fe.extract_batch(img, backbone_out=tokens, n_random_pixels=NR, frame_index=2 * B)
    assert torch.equal(s2, r2)
    # frame_index = k reproduces a draw, features included
    k = 1234
    fa, sa, _ = fe.extract_batch(img, backbone_out=tokens, n_random_pixels=NR, frame_index=k)
    fb, sb, _ = fe.extract_batch(img, backbone_out=tokens, n_random_pixels=NR, frame_index=k)
    assert torch.equal(sa, sb) and torch.equal(fa, fb) and not torch.equal(sa, r0)
    # a B = 2 call with frame_index = k is two B = 1 calls with k and k + 1
    for b in range(B):
        f1b, s1b, n1b = fe.extract_batch(img[b:b + 1], backbone_out=tokens[b:b + 1], n_random_pixels=NR, frame_index=k + b)
        assert torch.equal(s1b[0], sa[b]) and torch.equal(f1b[0], fa[b]) and n1b.tolist() == [NR]
    # another seed draws other pixels for the same frames
    other = _extractor(dev, "dino", "random", "bf16", random_seed=10)
    _, so, _ = other.extract_batch(img, backbone_out=tokens, n_random_pixels=NR, frame_index=k)
    assert not torch.equal(so, sa)


def test_random_extract_batch_refuses_non_square_frames(dev):
    fe = _extractor(dev, "dino", "random", "bf16")
    with pytest.raises(_lib.WvnError, match="square"):
        fe.extract_batch(torch.rand(1, 3, 64, 96, generator=g(1)).to(dev), n_random_pixels=NR)
    with pytest.raises(_lib.WvnError):
        fe.extract_batch(_img(dev), n_random_pixels=S * S + 1)


def test_predict_per_segment_takes_random_segmentation(dev):
    """extract_batch's random maps through the per-segment mode: the -1 pixels wrap onto the last sample's row, as the reference's feat[seg] does."""
    fe = _extractor(dev, "dino", "random", "bf16", random_seed=2)
    model, cg, img = _model(dev, fe.feature_dim), _cg(dev), _img(dev)
    trav, conf, _, feat, seg, nseg = fe.predict_per_segment(img, model, cg, n_random_pixels=NR, frame_index=3)
    f2, s2, _ = fe.extract_batch(img, n_random_pixels=NR, frame_index=3)
    assert torch.equal(seg, s2) and torch.equal(feat, f2) and nseg.tolist() == [NR] * B
    t2, c2, _ = model.forward_per_segment(feat, seg, float(cg.mean), float(cg.std), float(cg.std_factor))
    assert torch.allclose(trav, t2, atol=1e-6) and torch.allclose(conf, c2, atol=1e-6) and torch.isfinite(trav).all()
    for b in range(B):
        assert (trav[b][seg[b] == -1] == trav[b][seg[b] == NR - 1]).all()
