"""DoubleMLP on the GPU (csrc/double_mlp.hip): the forward, twelve training steps against the reference's own numbers
(tests/golden/double_mlp_train.pt) on the four-launch and on the general path, the decoupling of the two networks, bit-level
contracts (reproducible steps, compacted batches, an empty shard), the path limits against the float64 restatement
(tests/double_mlp_ref.py), the per-segment prediction and the TraversabilityEstimator loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import double_mlp_ref as REF  # noqa: E402

from wild_visual_navigation_amd import _lib  # noqa: E402
from wild_visual_navigation_amd.bridge import DeviceWeightsHandoff  # noqa: E402
from wild_visual_navigation_amd.cfg import ExperimentParams  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor  # noqa: E402
from wild_visual_navigation_amd.model import DoubleMLP  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import MissionNode, MlpTrainer, TraversabilityEstimator  # noqa: E402
from wild_visual_navigation_amd.utils import ConfidenceGenerator, Data  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ["latest_measurement_balanced", "running_mean_balanced", "kalman_filter_balanced", "moving_average_balanced",
         "latest_measurement_unbalanced", "running_mean_unbalanced"]
HIDDEN = [64, 32, 1]


def _tile():
    return int(_lib.lib().wvn_double_mlp_row_tile())


def _model(sd0, D, dev, hidden=HIDDEN):
    m = DoubleMLP(D, hidden)
    m.load_state_dict(sd0)
    return m.to(dev)


def _seeded_sd(D, hidden, seed):
    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in DoubleMLP(D, hidden).state_dict().items()}


def _conf_atol(c, step):
    """The rule of tests/test_gpu_train_methods.py: running_mean keeps the population variance as sum_sq / n - mean^2, the reference
    forms the two sums in fp32 and the step in fp64; the cancellation scales their ~1 ulp difference by (mean^2 + var) / var.
    Every other method: 1e-5."""
    if c["method"] != "running_mean":
        return 1e-5
    m, v = c["traj"][step, 3].item(), c["traj"][step, 4].item()
    return 1e-5 + 2.0 ** -22 * (m * m + v) / v


def _row(tr, losses):
    lo = losses.cpu()
    return [lo[0].item(), lo[1].item(), lo[2].item(), lo[3].item(), tr.conf_state[1].item(), lo[4].item()]


# ---- forward ----------------------------------------------------------------------------------------------------------------
def test_forward_matches_the_reference_output(dev, golden):
    fx = golden("double_mlp_train.pt")["d90"]
    x = golden("mlp_train.pt")["graph_pt_D90"]["x"]
    out = _model(fx["sd0"], 90, dev).forward(Data(x=x.to(dev)))
    assert out.shape == fx["res0"].shape == (x.shape[0], 91)
    assert torch.allclose(out.cpu(), fx["res0"], atol=1e-5), (out.cpu() - fx["res0"]).abs().max()


@pytest.mark.parametrize("D,hidden", [(90, HIDDEN), (384, HIDDEN), (90, [48, 16, 1])])
def test_forward_matches_fp64_restatement(dev, D, hidden):
    T = _tile()
    sd = _seeded_sd(D, hidden, 3)
    m = _model(sd, D, dev, hidden)
    g = torch.Generator().manual_seed(5)
    for R in (1, T - 1, T, T + 1, 2 * T + 3):
        x = torch.randn(R, D, generator=g)
        out = m.forward(Data(x=x.to(dev)))
        err = (out.cpu().double() - REF.forward(sd, x)).abs().max().item()
        print(f"D {D} hidden {hidden} R {R}: max err {err:.3e}")
        assert out.shape == (R, D + 1) and err < 1e-5
    wide = torch.randn(2 * T + 3, D + 7, generator=g).to(dev)   # a strided x: ldx > D
    xs = wide[:, :D]
    assert xs.stride(0) == D + 7
    out = m.forward(Data(x=xs))
    assert (out.cpu().double() - REF.forward(sd, xs.cpu())).abs().max().item() < 1e-5


# ---- twelve steps against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_twelve_steps_match_reference(dev, golden, case, fused):
    fx = golden("double_mlp_train.pt")["d90"]
    c = fx["cases"][case]
    src = golden("mlp_train.pt")["graph_pt_D90"]
    m = _model(fx["sd0"], 90, dev)
    tr = MlpTrainer(m, lr=1e-3, std_factor=0.5, w_trav=0.03, w_reco=0.5, fused=fused, method=c["method"],
                    anomaly_balanced=c["balanced"])
    tr._conf = True   # (latest_measurement too keeps its variance in the device state)
    traj = []
    for step, r in enumerate(c["rows"]):
        losses = tr.train_step(src["x"][r].to(dev), src["y"][r].to(dev), src["y_valid"][r].to(dev), want_confidence=True)
        traj.append(_row(tr, losses))
        err = (tr.last_confidence.cpu() - c["conf"][step]).abs().max().item()
        assert torch.allclose(tr.last_confidence.cpu(), c["conf"][step], atol=_conf_atol(c, step)), (step, err)
    traj = np.array(traj)
    print(f"{case} fused {fused}: max traj err {np.abs(traj - c['traj'].numpy()).max():.3e}")
    assert np.allclose(traj, c["traj"].numpy(), rtol=3e-4, atol=2e-6), np.abs(traj - c["traj"].numpy()).max()
    for k, v in m.state_dict().items():
        assert torch.allclose(v.cpu(), c["sd12"][k], atol=3e-5), (k, (v.cpu() - c["sd12"][k]).abs().max())
    cg = ConfidenceGenerator(0.5, c["method"]).to(dev)
    tr.store_confidence_state(cg)
    for k, v in cg.state_dict().items():
        want = c["cg12"][k]
        assert v.dtype == want.dtype and torch.allclose(v.cpu().double(), want.double(), rtol=1e-5, atol=1e-6), k


@pytest.mark.parametrize("method", ["latest_measurement", "moving_average"])
def test_d384_trajectories(dev, golden, method):
    fx = golden("double_mlp_train.pt")["d384"]
    c = fx["cases"][method]
    src = golden("mlp_train.pt")["synthetic_D384"]
    for fused in (True, False):
        tr = MlpTrainer(_model(fx["sd0"], 384, dev), fused=fused, method=method)
        tr._conf = True
        traj = [_row(tr, tr.train_step(src["x"][r].to(dev), src["y"][r].to(dev), src["y_valid"][r].to(dev))) for r in c["rows"]]
        assert np.allclose(np.array(traj), c["traj"].numpy(), rtol=3e-4, atol=2e-6), (fused, np.abs(np.array(traj) - c["traj"].numpy()).max())


def test_default_configuration_through_the_plain_entry_points(dev, golden):
    """latest_measurement + anomaly_balanced through the entry points without a state gives the bits of the *_conf ones."""
    fx = golden("double_mlp_train.pt")["d90"]
    src = golden("mlp_train.pt")["graph_pt_D90"]
    x, y, yv = src["x"].to(dev), src["y"].to(dev), src["y_valid"].to(dev)
    for fused in (True, False):
        ma, mb = _model(fx["sd0"], 90, dev), _model(fx["sd0"], 90, dev)
        ta, tb = MlpTrainer(ma, fused=fused), MlpTrainer(mb, fused=fused)
        assert not ta._conf
        tb._conf = True
        for _ in range(3):
            la = ta.train_step(x, y, yv, want_confidence=True).clone()
            lb = tb.train_step(x, y, yv, want_confidence=True).clone()
            assert torch.equal(la, lb) and torch.equal(ta.last_confidence, tb.last_confidence)
        assert all(torch.equal(v, mb.state_dict()[k]) for k, v in ma.state_dict().items())


# ---- structure ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_the_two_networks_decouple(dev, golden, fused):
    fx = golden("double_mlp_train.pt")["d90"]
    src = golden("mlp_train.pt")["graph_pt_D90"]
    x, y, yv = src["x"].to(dev), src["y"].to(dev), src["y_valid"].to(dev)
    for w_trav, w_reco, frozen in ((0.03, 0.0, "networks.1."), (0.0, 0.5, "networks.0.")):
        m = _model(fx["sd0"], 90, dev)
        tr = MlpTrainer(m, w_trav=w_trav, w_reco=w_reco, fused=fused)
        for _ in range(5):
            tr.train_step(x, y, yv)
        for k, v in m.state_dict().items():
            same = torch.equal(v.cpu(), fx["sd0"][k])
            assert same == k.startswith(frozen), (k, w_trav, w_reco)


@pytest.mark.parametrize("fused", [True, False])
def test_gradients_are_finite_with_zero_feature_rows(dev, golden, fused):
    """The gradient buffer between phases B and C (ReLU-masked, all twelve tensors + the two loss sums) against float64."""
    fx = golden("double_mlp_train.pt")["d90"]
    src = golden("mlp_train.pt")["graph_pt_D90"]
    x, y, yv = src["x"].clone(), src["y"], src["y_valid"]
    x[::7] = 0.0
    m = _model(fx["sd0"], 90, dev)
    tr = MlpTrainer(m, fused=fused)
    tr.train_step(x.to(dev), y.to(dev), yv.to(dev))   # (grads holds the step's gradient: phase C only reads it)
    grads = tr.grads.cpu()
    assert torch.isfinite(grads).all()
    ref = REF.F64Step(fx["sd0"])
    ref.step(x, y, yv)
    want = torch.cat([ref.grads[k].reshape(-1) for k in REF.KEYS])
    assert torch.allclose(grads[:-2].double(), want, rtol=1e-4, atol=1e-7), (grads[:-2].double() - want).abs().max()


# ---- fixed summation orders ---------------------------------------------------------------------------------------------------
def test_fused_steps_are_bit_reproducible(dev, golden):
    fx = golden("double_mlp_train.pt")["d90"]
    src = golden("mlp_train.pt")["graph_pt_D90"]
    x, y, yv = src["x"].to(dev), src["y"].to(dev), src["y_valid"].to(dev)
    runs = []
    for _ in range(2):
        m = _model(fx["sd0"], 90, dev)
        tr = MlpTrainer(m, fused=True, method="running_mean")
        losses = [tr.train_step(x, y, yv).clone() for _ in range(5)]
        runs.append((torch.stack(losses), m.flat_params().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("method", ["latest_measurement", "moving_average"])
def test_compacted_batch_gives_the_same_bits(dev, method):
    T, D = _tile(), 90
    n, R = T + 5, 2 * T
    sd = _seeded_sd(D, HIDDEN, 4)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(R, D, generator=g)
    yv = torch.rand(R, generator=g) < 0.3
    yv[:2] = True
    y = yv.float() * 0.7
    xg = x.clone()
    xg[n:] = 0.0   # zero rows behind the count (what compact_segment_rows leaves)
    rows_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    for fused in (True, False):
        ma, mb = _model(sd, D, dev), _model(sd, D, dev)
        ta, tb = MlpTrainer(ma, fused=fused, method=method), MlpTrainer(mb, fused=fused, method=method)
        ta._conf = tb._conf = True
        for _ in range(3):
            la = ta.train_step(xg.to(dev), y.to(dev), yv.to(dev), rows_dev=rows_dev, want_confidence=True).cpu()
            lb = tb.train_step(x[:n].to(dev), y[:n].to(dev), yv[:n].to(dev), want_confidence=True).cpu()
            if fused:   # the four-launch step walks the same tiles
                assert torch.equal(la, lb) and torch.equal(ta.conf_state, tb.conf_state)
                assert torch.equal(ta.last_confidence[:n], tb.last_confidence)
            else:       # the general path's GEMMs see R rows
                assert torch.allclose(la, lb, rtol=1e-5, atol=2e-6)
                assert torch.allclose(ta.last_confidence[:n], tb.last_confidence, atol=1e-5)
        for k, v in ma.state_dict().items():
            assert torch.equal(v, mb.state_dict()[k]) if fused else torch.allclose(v, mb.state_dict()[k], atol=1e-5), k


@pytest.mark.parametrize("R,D", [(33, 90), (17, 91)])
def test_four_launch_step_equals_general_path(dev, R, D):
    """The counterpart of tests/test_gpu_mlp.py::test_four_launch_step_equals_general_path_and_oracle at the 16-row tile: the
    statistic's ticket and the table-driven weight gradients (shared with the SimpleMLP step) from the DoubleMLP side, ragged last
    row tile, odd D; then a compacted batch (rows_dev) with garbage behind the count gives the bits of the truncated batch."""
    g = torch.Generator().manual_seed(R + D)
    x = torch.randn(R, D, generator=g)
    yv = torch.rand(R, generator=g) < 0.16
    yv[:2] = True
    y = yv.float() * (0.5 + 0.5 * torch.rand(R, generator=g))
    sd0 = _seeded_sd(D, HIDDEN, 42)
    ma, mb = _model(sd0, D, dev), _model(sd0, D, dev)
    assert _lib.lib().wvn_double_mlp_fused_ok(C.byref(ma.desc), R)
    ta, tb = MlpTrainer(ma, fused=True), MlpTrainer(mb, fused=False)
    for _ in range(3):
        la = ta.train_step(x.to(dev), y.to(dev), yv.to(dev), want_confidence=True).cpu()
        lb = tb.train_step(x.to(dev), y.to(dev), yv.to(dev), want_confidence=True).cpu()
        assert torch.allclose(ta.last_confidence, tb.last_confidence, atol=1e-5)
    print(f"R {R} D {D}: losses fused {la.tolist()} general {lb.tolist()}")
    assert torch.allclose(la, lb, rtol=1e-5, atol=2e-6), (la, lb)
    for k, v in ma.state_dict().items():
        assert torch.allclose(v, mb.state_dict()[k], atol=1e-5), (k, (v - mb.state_dict()[k]).abs().max())
    assert int(ta.sync_word.item()) == 0                                      # the arrival counter is back at zero
    n = R - R // 3
    rows_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    xg = x.clone()
    xg[n:] = 1e6
    mc, md = _model(sd0, D, dev), _model(sd0, D, dev)
    tc, td = MlpTrainer(mc, fused=True), MlpTrainer(md, fused=True)
    for _ in range(3):
        lc = tc.train_step(xg.to(dev), y.to(dev), yv.to(dev), rows_dev=rows_dev).cpu()
        ld = td.train_step(x[:n].to(dev), y[:n].to(dev), yv[:n].to(dev)).cpu()
    assert torch.equal(lc, ld)                                                # the same tiles in the same order: identical bits
    for k, v in mc.state_dict().items():
        assert torch.equal(v, md.state_dict()[k]), k
    assert int(tc.sync_word.item()) == 0


# ---- path limits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2048, 2049])
def test_path_limit_matches_fp64_restatement(dev, R):
    D = 90
    sd0 = _seeded_sd(D, HIDDEN, 42)
    m = _model(sd0, D, dev)
    assert bool(_lib.lib().wvn_double_mlp_fused_ok(C.byref(m.desc), R)) == (R == 2048)   # 2048: four launches, 2049: the general path
    ref = REF.F64Step(sd0, "running_mean", balanced=True)
    tr = MlpTrainer(m, fused=True, method="running_mean")
    g = torch.Generator().manual_seed(21)
    for _ in range(3):
        x = torch.randn(R, D, generator=g)
        yv = torch.rand(R, generator=g) < 0.2
        y = yv.float() * (0.5 + 0.5 * torch.rand(R, generator=g))
        want, wconf = ref.step(x, y, yv)
        got = tr.train_step(x.to(dev), y.to(dev), yv.to(dev), want_confidence=True).cpu()
        print(f"R {R}: losses {got.tolist()} want {want}")
        assert np.allclose(got.numpy(), np.array(want), rtol=1e-4, atol=1e-6), (got, want)
        assert torch.allclose(tr.last_confidence.cpu().double(), wconf, atol=1e-4)
    for k, v in m.state_dict().items():
        assert torch.allclose(v.cpu().double(), ref.p[k], atol=2e-5), (k, (v.cpu().double() - ref.p[k]).abs().max())


# ---- empty shard ----------------------------------------------------------------------------------------------------------------
def test_empty_shard_leaves_the_parameters(dev, golden):
    fx = golden("double_mlp_train.pt")["d90"]
    m = _model(fx["sd0"], 90, dev)
    tr = MlpTrainer(m, fused=True)
    before = m.flat_params().clone()
    tr.train_step(torch.zeros(0, 90, device=dev), torch.zeros(0, device=dev), torch.zeros(0, dtype=torch.bool, device=dev))
    assert torch.equal(m.flat_params(), before)
    assert int(tr.sync_word.item()) == 0
    src = golden("mlp_train.pt")["graph_pt_D90"]
    tr.train_step(src["x"].to(dev), src["y"].to(dev), src["y_valid"].to(dev))
    assert int(tr.sync_word.item()) == 0 and not torch.equal(m.flat_params(), before)


# ---- per-segment prediction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("D,hidden", [(90, HIDDEN), (384, [48, 16, 1])])
def test_forward_per_segment(dev, seg_dtype, D, hidden):
    B, S, H, W = 2, 7, 24, 24
    sd = _seeded_sd(D, hidden, 6)
    m = _model(sd, D, dev, hidden)
    g = torch.Generator().manual_seed(2)
    feat = torch.randn(B, S, D, generator=g)
    feat[1, 3] = float("nan")
    seg = torch.randint(0, S, (B, H, W), generator=g)
    seg[0, 0, 0], seg[0, 0, 1], seg[0, 0, 2], seg[1, 5, 5] = -1, -S, S, -S - 1
    seg = seg.to(seg_dtype)
    mean, std, f = 1.2, 0.4, 0.5
    wt, wc, wl = REF.per_segment(sd, feat, seg, mean, std, f)
    assert torch.isnan(wt[0, 0, 2]) and torch.isnan(wt[1, 5, 5]) and not torch.isnan(wt[0, 0, 0]) and not torch.isnan(wt[0, 0, 1])
    state = torch.tensor([mean, std, f], dtype=torch.float32, device=dev)
    for want_loss, conf_state in ((True, None), (False, None), (True, state)):
        scal = (0.0, 1.0, 0.5) if conf_state is not None else (mean, std, f)   # the device state overrides the three floats
        trav, conf, loss = m.forward_per_segment(feat.to(dev), seg.to(dev), *scal, want_loss=want_loss, conf_state=conf_state)
        assert trav.shape == conf.shape == (B, H, W) and (loss is None) == (not want_loss)
        pairs = [(trav, wt), (conf, wc)] + ([(loss, wl)] if want_loss else [])
        for got, want in pairs:
            got = got.cpu().double()
            assert torch.equal(torch.isnan(got), torch.isnan(want))
            assert torch.allclose(got, want, atol=1e-5, equal_nan=True), (got - want).abs().nan_to_num().max()


def test_predict_per_segment_equals_its_pieces(dev):
    fe = FeatureExtractor(dev, segmentation_type="grid", feature_type="dino", input_size=64, allow_synthetic=True)
    m = _model(_seeded_sd(fe.feature_dim, HIDDEN, 1), fe.feature_dim, dev)
    img = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(dev)
    trav, conf, loss, feat, seg, nseg = fe.predict_per_segment(img, m, want_loss=True)
    assert torch.isfinite(trav).all() and torch.isfinite(conf).all() and torch.isfinite(loss).all()
    f2, s2, _ = fe.extract_batch(img)
    t2, c2, l2 = m.forward_per_segment(f2, s2, want_loss=True)
    assert torch.equal(trav, t2) and torch.equal(conf, c2) and torch.equal(loss, l2)


def test_predict_per_pixel_is_refused(dev):
    fe = FeatureExtractor(dev, segmentation_type="grid", feature_type="dino", input_size=64, allow_synthetic=True)
    m = DoubleMLP(fe.feature_dim, HIDDEN).to(dev)
    with pytest.raises(_lib.WvnError, match="DoubleMLP"):
        fe.predict_per_pixel(torch.rand(1, 3, 64, 64), m)
    with pytest.raises(_lib.WvnError, match="DoubleMLP"):
        m.pack_per_pixel()


# ---- TraversabilityEstimator ------------------------------------------------------------------------------------------------------
def _estimator(dev):
    p = ExperimentParams()
    p.model.name = "DoubleMLP"
    p.model.double_mlp_cfg.input_size = 90
    p.loss.method = "running_mean"
    return TraversabilityEstimator(p, device=dev, min_samples_for_training=2)


def test_estimator_loop_checkpoint_and_handoff(dev, tmp_path):
    te = _estimator(dev)
    assert isinstance(te._model, DoubleMLP)
    g = torch.Generator().manual_seed(0)
    S, H = 12, 48
    for i in range(6):
        n = MissionNode(timestamp=float(i))
        n.features = torch.randn(S, 90, generator=g).to(dev)
        n.feature_segments = (torch.arange(H * H).reshape(H, H) * S // (H * H)).to(dev)
        mask = torch.full((3, H, H), float("nan"))
        mask[:, : H // 2] = 0.5 + 0.5 * torch.rand(3, H // 2, H, generator=g)
        assert te.add_mission_node(n)
        te.update_supervision(n, mask.to(dev))
    steps = [te.train() for _ in range(6)]
    totals = [s["loss_total"] for s in steps]
    assert all(np.isfinite(t) and t > 0 for t in totals) and totals[-1] < totals[0], totals
    f = te.save_checkpoint(str(tmp_path))
    ck = torch.load(f, weights_only=False)
    assert list(ck["model_state_dict"]) == REF.KEYS
    loss_keys = [k for k in ck["traversability_loss_state_dict"] if k.startswith("_model.")]
    assert loss_keys == ["_model." + k for k in REF.KEYS]
    assert sorted(ck["optimizer_state_dict"]["state"]) == list(range(12))
    te2 = _estimator(dev)
    te2.load_checkpoint(f)
    x = torch.randn(60, 90, generator=g).to(dev)
    yv = torch.rand(60, generator=g) < 0.3
    yv[:2] = True
    batch = (x, (yv.float() * 0.8).to(dev), yv.to(dev))
    l1 = te.train_on_batch(*batch).clone()
    l2 = te2.train_on_batch(*batch).clone()
    assert torch.equal(l1, l2) and torch.equal(te._optimizer.conf_state, te2._optimizer.conf_state)
    for k, v in te._model.state_dict().items():
        assert torch.equal(v, te2._model.state_dict()[k]), k
    # the weights hand-off into a second model
    cg = te._traversability_loss._confidence_generator
    other, cg2 = DoubleMLP(90, HIDDEN).to(dev), ConfidenceGenerator(0.5, "running_mean").to(dev)
    ho = DeviceWeightsHandoff(te._model.flat_params().numel(), dev)
    ho.publish(te._model, cg)
    assert ho.consume(other, cg2)
    for k, v in te._model.state_dict().items():
        assert torch.equal(v, other.state_dict()[k]), k
