"""The anomaly-detection mode on the GPU (csrc/rnvp.hip): the flow kernel on rows and on pixels against the float64 statement
(tests/linear_rnvp_ref.py) and the reference's own numbers (tests/golden/linear_rnvp.pt), the model's two routes, the
TraversabilityEstimator loop and the FeatureExtractor entry points.

Tolerances (shared by the kernel cases):
  score   max(4 x own_err, 2^-16 x max|score|).  own_err is the reference's own fp32 score against the float64 statement, recorded
          in the fixture: another fp32 summation order errs about as much as the reference does (the rule scripts/pin_double_mlp.py
          states).  2^-16 is the resolution of a hi + lo 16-bit operand pair; one bf16 operand (2^-9) misses it by two orders.
  log_det the score's: it is one addend of the score, formed by the same products.
  z       2^-16 x max|z|.
  conf    score tolerance / (2 std): conf = 1 - (x - lo) / (hi - lo) with hi - lo = 2 std, so an error e in x = -score moves it
          by e / (2 std) (the clip only shrinks it); + 2^-22 for the fp32 rounding of a value in [0, 1].
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_rnvp_ref as REF  # noqa: E402

from oracle import vit as OV  # noqa: E402
from wild_visual_navigation_amd import _lib  # noqa: E402
from wild_visual_navigation_amd.cfg import ExperimentParams  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor  # noqa: E402
from wild_visual_navigation_amd.model import DoubleMLP, LinearRnvp  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import MissionNode, TraversabilityEstimator  # noqa: E402
from wild_visual_navigation_amd.utils import AnomalyLoss, ConfidenceGenerator, Data  # noqa: E402

pytestmark = pytest.mark.gpu

H = 200
_CACHE = {}


def _tile():
    return int(_lib.lib().wvn_rnvp_row_tile())


def _sd(golden, D, mask_type):
    """The state dict of a case: at D = 90 with the "odds" mask the fixture's (the reference's seeded one), else seeded here."""
    key = ("sd", D, mask_type)
    if key not in _CACHE:
        if D == 90 and mask_type == "odds":
            _CACHE[key] = REF.expand_sd0(golden("linear_rnvp.pt")["d90"]["sd0"])
        else:
            _CACHE[key] = REF.seeded_sd(D, H, seed=11 + D, mask_type=mask_type)
    return _CACHE[key]


def _rows(golden, D):
    src = golden("mlp_train.pt")
    return src["graph_pt_D90"]["x"] if D == 90 else src["synthetic_D384"]["x"]


def _ref(golden, D, mask_type):
    """(z, log_det, score) of the float64 statement on all rows of the case, computed once."""
    key = ("ref", D, mask_type)
    if key not in _CACHE:
        with torch.no_grad():
            _CACHE[key] = REF.flow(_sd(golden, D, mask_type), _rows(golden, D))
    return _CACHE[key]


def _model(sd, D, dev, mask_type="odds", h=H):
    m = LinearRnvp(D, [h], use_permutation=True, mask_type=mask_type)
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


def _score_tol(golden, D, score64):
    own = golden("linear_rnvp.pt")["d90" if D == 90 else "d384"]["own_err"]["abs"]
    return max(4 * own, 2.0 ** -16 * score64.abs().max().item())


# ---- rows kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_type", ["odds", "half"])
@pytest.mark.parametrize("D", [90, 384])
def test_rows_match_float64_statement(dev, golden, D, mask_type):
    T = _tile()
    x = _rows(golden, D)
    z64, ld64, sc64 = _ref(golden, D, mask_type)
    m = _model(_sd(golden, D, mask_type), D, dev, mask_type)
    for R in (1, 33, T - 1, T + 1, 2 * T + 5):
        score, log_det, z, _ = m.forward_rows(x[:R].to(dev))
        tol = _score_tol(golden, D, sc64[:R])
        es = (score.cpu().double() - sc64[:R]).abs().max().item()
        el = (log_det.cpu().double() - ld64[:R]).abs().max().item()
        ez = (z.cpu().double() - z64[:R]).abs().max().item()
        print(f"D {D} {mask_type} R {R}: score err {es:.3e} (tol {tol:.3e}, max |score| {sc64[:R].abs().max():.1f}) "
              f"log_det err {el:.3e} z err {ez:.3e} (tol {2.0 ** -16 * z64[:R].abs().max().item():.3e})")
        assert score.shape == (R,) and log_det.shape == (R,) and z.shape == (R, D)
        assert es <= tol                                                   # module docstring: score
        assert el <= tol                                                   # log_det: one addend of the score
        assert ez <= 2.0 ** -16 * z64[:R].abs().max().item()               # z
    # a strided x (ldx > D), without z: the score does not depend on which outputs are asked for
    wide = torch.zeros(2 * T + 5, D + 7)
    wide[:, :D] = x[: 2 * T + 5]
    xs = wide.to(dev)[:, :D]
    assert xs.stride(0) == D + 7
    s2, l2, z2, _ = m.forward_rows(xs, want_z=False)
    assert z2 is None and torch.equal(s2, score) and torch.equal(l2, log_det)


@pytest.mark.parametrize("D,h", [(90, 256), (384, 256), (90, 48), (384, 225)])
def test_rows_at_other_hidden_sizes(dev, golden, D, h):
    """h up to 224 runs in seven 32-unit blocks, above in eight (zero-padded either way): the widest, the first of the second form
    and a small one."""
    sd = REF.seeded_sd(D, h, seed=h + D)
    x = _rows(golden, D)[: _tile() + 1]
    with torch.no_grad():
        z64, ld64, sc64 = REF.flow(sd, x)
    score, log_det, z, _ = _model(sd, D, dev, h=h).forward_rows(x.to(dev))
    tol = _score_tol(golden, D, sc64)
    assert (score.cpu().double() - sc64).abs().max().item() <= tol          # module docstring: score
    assert (log_det.cpu().double() - ld64).abs().max().item() <= tol        # log_det
    assert (z.cpu().double() - z64).abs().max().item() <= 2.0 ** -16 * z64.abs().max().item()   # z


def test_rows_match_reference_fixture(dev, golden):
    fx = golden("linear_rnvp.pt")["d90"]
    x = _rows(golden, 90)
    score, log_det, z, _ = _model(_sd(golden, 90, "odds"), 90, dev).forward_rows(x.to(dev))
    want = (fx["logprob_sum"] + fx["log_det"]).double()
    tol = max(4 * fx["own_err"]["abs"], 2.0 ** -16 * want.abs().max().item())
    # (the reference itself is own_err away from the float64 statement the tolerance is stated for)
    assert (score.cpu().double() - want).abs().max().item() <= tol + fx["own_err"]["abs"]
    assert (log_det.cpu().double() - fx["log_det"].double()).abs().max().item() <= tol + fx["own_err"]["abs"]
    assert (z.cpu() - fx["z"]).abs().max().item() <= 2.0 ** -16 * fx["z"].abs().max().item() + 1e-6


@pytest.mark.parametrize("mask_type", ["odds", "half"])
@pytest.mark.parametrize("D", [90, 384])
def test_zeroed_last_layers_pin_the_bookkeeping(dev, golden, D, mask_type):
    """s = 0 and t = bias: z = (x + (1 - m) b)[:, p], chained, and log_det = 0 exactly -- masks and permutations without the MFMA path
    mattering (its products are all multiplied by zero weights)."""
    sd = {k: v.clone() for k, v in _sd(golden, D, mask_type).items()}
    for f in (0, 2):
        for n in ("s", "t"):
            sd[f"flows.{f}.{n}.4.weight"].zero_()
        sd[f"flows.{f}.s.4.bias"].zero_()
    x = _rows(golden, D)[: _tile() + 1]
    u = x.double()
    for f in (0, 2):
        u = (u + (1 - sd[f"flows.{f}.mask"].double()) * sd[f"flows.{f}.t.4.bias"].double())[:, sd[f"flows.{f + 1}.p"]]
    score, log_det, z, _ = _model(sd, D, dev, mask_type).forward_rows(x.to(dev))
    assert torch.equal(log_det.cpu(), torch.zeros(x.shape[0]))
    assert (z.cpu().double() - u).abs().max().item() <= 2.0 ** -16 * u.abs().max().item()
    want = (-0.5 * u * u).sum(1) - D * 0.5 * np.log(2 * np.pi)
    assert (score.cpu().double() - want).abs().max().item() <= 2.0 ** -16 * want.abs().max().item()


# ---- pixels source ---------------------------------------------------------------------------------------------------------------
def _taps(G, Ho):
    """ATen's align_corners taps in fp32: src = o * (G-1)/(Ho-1), i0 = int(src), w1 = src - i0, w0 = 1 - w1."""
    scale = torch.tensor((G - 1) / (Ho - 1), dtype=torch.float32) if Ho > 1 else torch.tensor(0.0)
    s = scale * torch.arange(Ho, dtype=torch.float32)
    i0 = s.to(torch.int64)
    i1 = i0 + (i0 < G - 1).to(torch.int64)
    w1 = s - i0.float()
    return i0, i1, 1 - w1, w1


def _interp_fp32(tok, B, G, Ho):
    """The rows the kernel forms, in torch fp32 with the same taps and the same order (x first, then y)."""
    t = tok.view(B, G, G, -1)
    i0, i1, w0, w1 = _taps(G, Ho)
    a = t[:, :, i0] * w0[None, None, :, None] + t[:, :, i1] * w1[None, None, :, None]      # [B, G, Ho, D]
    out = a[:, i0] * w0[None, :, None, None] + a[:, i1] * w1[None, :, None, None]          # [B, Ho, Ho, D]
    return out.reshape(B * Ho * Ho, -1)


@pytest.mark.parametrize("D", [90, 384])
@pytest.mark.parametrize("B,G,Ho", [(2, 7, 56), (1, 5, 37)])
def test_pixels_match_float64_interpolation_and_flow(dev, golden, B, G, Ho, D):
    sd = _sd(golden, D, "odds")
    m = _model(sd, D, dev)
    tok = torch.randn(B * G * G, D, generator=torch.Generator().manual_seed(G + D))
    dense = F.interpolate(tok.double().view(B, G, G, D).permute(0, 3, 1, 2), size=(Ho, Ho), mode="bilinear", align_corners=True)
    with torch.no_grad():
        z64, _, sc64 = REF.flow(sd, dense.permute(0, 2, 3, 1).reshape(B * Ho * Ho, D))
    tol = _score_tol(golden, D, sc64)
    x64 = -sc64
    mean, std, f = torch.tensor(x64.mean().item(), dtype=torch.float32), torch.tensor(x64.std().item(), dtype=torch.float32), 0.5
    trav, conf, loss, z = m.forward_per_pixel_exact(tok.to(dev), B, G, (Ho, Ho), mean.item(), std.item(), f, want_loss=True, want_z=True)
    assert trav is conf and conf.shape == loss.shape == (B, Ho, Ho)
    es = (loss.cpu().double().reshape(-1) - x64).abs().max().item()
    ez = (z.cpu().double() - z64).abs().max().item()
    want_conf = REF.interval_confidence(x64, mean.double().item(), std.double().item(), f)
    ec = (conf.cpu().double().reshape(-1) - want_conf).abs().max().item()
    print(f"pixels B {B} G {G} H {Ho} D {D}: score err {es:.3e} (tol {tol:.3e}) z err {ez:.3e} conf err {ec:.3e} "
          f"(tol {tol / (2 * std.item()) + 2.0 ** -22:.3e})")
    assert es <= tol                                                       # module docstring: score
    assert ez <= 2.0 ** -16 * z64.abs().max().item()                       # z
    assert ec <= tol / (2 * std.item()) + 2.0 ** -22                       # conf = 1 - (x - lo) / (2 std)
    assert 0.05 < want_conf.mean().item() < 0.95                           # (the state puts the map inside the interval)
    # the statistic from device memory: the same bits
    state = torch.stack([mean, std, torch.tensor(f)]).to(dev)
    _, conf_dev, loss_dev = m.forward_per_pixel_exact(tok.to(dev), B, G, (Ho, Ho), 9.0, 9.0, 9.0, want_loss=True, conf_state=state)
    assert torch.equal(conf_dev, conf) and torch.equal(loss_dev, loss)
    # the row source on rows interpolated in fp32 with the same taps
    score_rows, _, _, _ = m.forward_rows(_interp_fp32(tok, B, G, Ho).to(dev), want_z=False)
    assert (score_rows.cpu().double() + loss.cpu().double().reshape(-1)).abs().max().item() <= tol


# ---- model.forward routes ----------------------------------------------------------------------------------------------------------
def test_forward_routes_and_repack(dev, golden):
    fx = golden("linear_rnvp.pt")["d90"]
    x = _rows(golden, 90).to(dev)
    m = _model(_sd(golden, 90, "odds"), 90, dev)
    score, log_det, z, _ = m.forward_rows(x)
    res = m(Data(x=x))                                   # eval: the kernel
    assert torch.equal(res["z"], z) and torch.equal(res["log_det"], log_det) and not res["z"].requires_grad
    assert res["logprob"].shape == (100, 90)
    assert (res["logprob"].sum(1) + res["log_det"] - score).abs().max().item() <= 2.0 ** -16 * score.abs().max().item()
    m.train()
    with torch.no_grad():                                # train, but no gradient asked for: still the kernel
        assert torch.equal(m(Data(x=x))["z"], z)
    res_t = m(Data(x=x))                                 # the torch statement
    assert res_t["z"].requires_grad
    ztol = 2.0 ** -16 * fx["z"].abs().max().item()
    assert (res_t["z"].detach().cpu() - fx["z"]).abs().max().item() <= ztol
    assert (res_t["log_det"].detach().cpu() - fx["log_det"]).abs().max().item() <= 1e-4
    # an optimizer step: the kernel route sees the new weights
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    loss, _, _ = AnomalyLoss(0.5, "latest_measurement").to(dev)(None, res_t)
    opt.zero_grad()
    loss.backward()
    opt.step()
    after_t = m(Data(x=x))["z"].detach()
    m.eval()
    after = m(Data(x=x))["z"]
    assert (after - z).abs().max().item() > 100 * ztol                      # the weights moved ...
    assert (after - after_t).abs().max().item() <= 2 * 2.0 ** -16 * after_t.abs().max().item()   # ... and both routes follow
    packed = m._packed
    m(Data(x=x))
    assert m._packed is packed and m._packed_key is not None               # unchanged parameters: no re-pack
    m.flows[0].mask[0] = 1.0                                               # D/2 + 1 ones
    with pytest.raises(_lib.WvnError, match="mask"):
        m(Data(x=x))
    m.flows[0].mask[0] = 0.0
    m.prior_var[3] = 2.0
    with pytest.raises(_lib.WvnError, match="prior"):
        m(Data(x=x))


# ---- TraversabilityEstimator ------------------------------------------------------------------------------------------------------
def _estimator(dev, method):
    p = ExperimentParams()
    p.model.name = "LinearRnvp"
    p.model.linear_rnvp_cfg.input_size = 90
    p.loss_anomaly.method = method
    return TraversabilityEstimator(p, device=dev, min_samples_for_training=2, anomaly_detection=True)


def _add_nodes(te, x, dev, t0=0.0):
    S, Hs = 25, 50
    for i in range(4):   # the 100 fixture rows as four nodes of 25 labelled segments: a batch holds all of them, in some order
        n = MissionNode(timestamp=t0 + float(i))
        n.features = x[25 * i: 25 * i + 25].to(dev)
        n.feature_segments = (torch.arange(Hs * Hs).reshape(Hs, Hs) * S // (Hs * Hs)).to(dev)
        assert te.add_mission_node(n)
        te.update_supervision(n, torch.full((3, Hs, Hs), 0.7, device=dev))


@pytest.mark.parametrize("method", ["latest_measurement", "running_mean"])
def test_estimator_reproduces_reference_trajectory(dev, golden, tmp_path, method):
    fx = golden("linear_rnvp.pt")["d90"]
    c = fx["cases"][method]
    te = _estimator(dev, method)
    sd0 = REF.expand_sd0(fx["sd0"])
    for k, v in te._model.state_dict().items():   # seed_everything(42) + get_model: the reference's initial state
        assert torch.equal(v.cpu(), sd0[k]), k
    _add_nodes(te, _rows(golden, 90), dev)
    cg = te._traversability_loss._confidence_generator
    traj = []
    for step in range(12):
        out = te.train()
        assert out["loss_trav"] == 0.0 and out["loss_reco"] == 0.0 and out["mission_graph_num_valid_node"] == 4
        traj.append([out["loss_total"], cg.mean.item(), cg.std.item()])
    traj = np.array(traj)
    print(f"{method}: max traj err {np.abs(traj - c['traj'].numpy()).max():.3e}")
    assert te.step == 12
    assert np.allclose(traj, c["traj"].numpy(), rtol=3e-4, atol=2e-6), np.abs(traj - c["traj"].numpy()).max()   # tests/test_gpu_double_mlp.py's
    for k, v in te._traversability_loss.state_dict().items():
        want = c["loss_sd12"][k]
        assert v.dtype == want.dtype and torch.allclose(v.cpu().double(), want.double(), rtol=3e-4, atol=2e-6), k
    # what the trained weights compute (the kernel route) against what the reference's trained weights compute: the 13th loss
    te._model.eval()
    score, _, _, _ = te._model.forward_rows(_rows(golden, 90).to(dev), want_z=False)
    te._model.train()
    want = (c["final"]["logprob_sum"] + c["final"]["log_det"]).mean().item()
    assert abs(score.mean().item() - want) <= 3e-4 * abs(want)
    # checkpoint round trip: the reference's five keys, torch's optimizer state
    f = te.save_checkpoint(str(tmp_path))
    ck = torch.load(f, weights_only=False)
    assert sorted(ck) == ["loss", "model_state_dict", "optimizer_state_dict", "step", "traversability_loss_state_dict"]
    assert list(ck["model_state_dict"]) == REF.KEYS and sorted(ck["optimizer_state_dict"]["state"]) == list(range(24))
    te2 = _estimator(dev, method)
    te2.load_checkpoint(f)
    _add_nodes(te2, _rows(golden, 90), dev)
    assert te2.step == 12 and te2.loss == te.loss
    a, b = te.train(), te2.train()   # (the node order of a batch is drawn at random: same rows, another summation order)
    assert abs(a["loss_total"] - b["loss_total"]) <= 1e-5 * abs(a["loss_total"])
    # a state dict with the keys and shapes of the reference's trained model loads strictly
    like = {k: (sd0[k] if not sd0[k].is_floating_point() else torch.zeros(s)) for k, s in c["sd12_shapes"].items()}
    assert not te2._model.load_state_dict(like, strict=True).unexpected_keys


# ---- FeatureExtractor ----------------------------------------------------------------------------------------------------------------
def test_feature_extractor_entry_points(dev, golden):
    frames = golden("demo_frames_224.pt")["frames_u8"][:1].to(dev)
    vit = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=21, depth=2)
    fe = FeatureExtractor(device=dev, segmentation_type="slic", feature_type="dino", patch_size=8, backbone_type="vit_small",
                          input_size=224, pretrained_weights=vit)
    sd = _sd(golden, 384, "odds")
    m = _model(sd, 384, dev)
    tokens = fe.backbone_stage(frames)
    B, G, Ho = 1, 28, 224
    assert tokens.shape == (B, G * G, 384) and tokens.dtype == torch.float32
    dense = F.interpolate(tokens.cpu().double().view(B, G, G, 384).permute(0, 3, 1, 2), size=(Ho, Ho), mode="bilinear", align_corners=True)
    with torch.no_grad():
        _, _, sc64 = REF.flow(sd, dense.permute(0, 2, 3, 1).reshape(-1, 384))
    tol = _score_tol(golden, 384, sc64)
    cg = ConfidenceGenerator(method="latest_measurement", std_factor=0.5).to(dev)
    cg.mean[0], cg.std[0] = (-sc64).mean().item(), (-sc64).std().item()
    trav, conf, loss = fe.predict_per_pixel(frames, m, cg, want_loss=True)
    es = (loss.cpu().double().reshape(-1) + sc64).abs().max().item()
    want_conf = REF.interval_confidence(-sc64, cg.mean.double().item(), cg.std.double().item(), 0.5)
    ec = (conf.cpu().double().reshape(-1) - want_conf).abs().max().item()
    print(f"predict_per_pixel: score err {es:.3e} (tol {tol:.3e}) conf err {ec:.3e}")
    assert trav.shape == (1, 224, 224) and torch.equal(trav, conf)
    assert es <= tol                                                       # module docstring: score
    assert ec <= tol / (2 * cg.std.item()) + 2.0 ** -22                    # conf
    # the one-pass frame: the same maps and the same training message, bit for bit
    t2, c2, l2, feat, seg, nseg = fe.predict_and_extract(frames, m, cg, want_loss=True)
    assert torch.equal(t2, trav) and torch.equal(c2, conf) and torch.equal(l2, loss)
    f3, s3, n3 = fe.extract_batch(frames)
    assert torch.equal(feat, f3) and torch.equal(seg, s3) and torch.equal(nseg, n3)
    # per segment: the rows kernel once per segment, painted through seg
    ts, cs, ls, f4, s4, _ = fe.predict_per_segment(frames, m, cg, want_loss=True)
    assert torch.equal(f4, f3) and torch.equal(s4, s3)
    score_seg, _, _, conf_seg = m.forward_rows(f3[0], want_z=False, want_conf=True, mean=cg.mean.item(), std=cg.std.item(), std_factor=0.5)
    assert torch.equal(cs[0], conf_seg[s3[0].long()]) and torch.equal(ts, cs) and torch.equal(ls[0], -score_seg[s3[0].long()])
    # refused before the backbone runs: a feature-dim mismatch, and DoubleMLP as before
    calls = []
    fe.backbone_stage = lambda img: calls.append(1)
    with pytest.raises(_lib.WvnError, match="feature_dim"):
        fe.predict_per_pixel(frames, _model(_sd(golden, 90, "odds"), 90, dev))
    with pytest.raises(_lib.WvnError, match="DoubleMLP"):
        fe.predict_per_pixel(frames, DoubleMLP(384, [64, 32, 1]).to(dev))
    assert not calls
