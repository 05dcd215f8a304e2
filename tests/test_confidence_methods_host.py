"""Every ConfidenceGenerator method and anomaly_balanced=False, host side (no GPU): the caller-facing torch API against the
reference's own code (tests/golden/mlp_train_methods.pt, written by scripts/pin_train_methods.py), construction through
ExperimentParams, and the argument checks of the *_conf training entry points, which refuse before any GPU call."""
import ctypes as C

import pytest
import torch

from oracle import mlp as OM
from wild_visual_navigation_amd import _lib
from wild_visual_navigation_amd.cfg import ExperimentParams
from wild_visual_navigation_amd.model import SimpleMLP
from wild_visual_navigation_amd.traversability_estimator import MlpTrainer, TraversabilityEstimator
from wild_visual_navigation_amd.utils import ConfidenceGenerator, Data, TraversabilityLoss

METHODS = ["latest_measurement", "running_mean", "kalman_filter", "moving_average"]
CASES = ["running_mean_balanced", "running_mean_unbalanced", "kalman_filter_balanced", "kalman_filter_unbalanced",
         "moving_average_balanced", "moving_average_unbalanced", "latest_measurement_unbalanced"]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("mlp_train_methods.pt")


def _close(a, b, atol=1e-6):
    return torch.allclose(a.float(), b.float(), atol=atol, rtol=0, equal_nan=True)


@pytest.mark.parametrize("method", METHODS)
def test_update_sequence_matches_reference(fx, method):
    u = fx["updates"][method]
    assert any(xp.numel() == 0 for xp in u["xps"])
    cg = ConfidenceGenerator(std_factor=0.5, method=method)
    for i, (x, xp) in enumerate(zip(u["xs"], u["xps"])):
        c = cg.update(x, xp, step=i)
        assert c.dtype == torch.float32 and _close(c, u["conf"][i]), (i, c, u["conf"][i])
        for k in ("mean", "var", "std"):
            assert _close(getattr(cg, k).detach(), u[k][i]), (i, k)


@pytest.mark.parametrize("method", METHODS)
def test_state_dict_keys_shapes_dtypes(fx, method):
    cg = ConfidenceGenerator(std_factor=0.5, method=method)
    got = [(k, tuple(v.shape), str(v.dtype)) for k, v in cg.state_dict().items()]
    assert got == fx["keys"][method]


def test_reset_rules():
    for method in METHODS:
        cg = ConfidenceGenerator(std_factor=0.5, method=method)
        x = torch.tensor([0.5, 1.0, 2.0, 3.0])
        cg.update(x, x[:3])
        mean = cg.mean.clone()
        cg.reset()
        if method == "running_mean":   # the running sums only
            assert float(cg.running_n) == 0 and float(cg.running_sum) == 0 and float(cg.running_sum_of_squares) == 0
            assert torch.equal(cg.mean, mean)
        else:
            assert float(cg.mean) == 0 and float(cg.var) == 1 and float(cg.std) == 1
        if method == "moving_average":
            assert len(cg.data_window) == 0
    # anomaly_balanced=False: TraversabilityLoss.reset is a no-op (loss.py:88-90)
    loss = TraversabilityLoss(0.03, 0.5, 0.0, False, SimpleMLP(90, [256, 32, 1], True), "kalman_filter", 0.5)
    cg = loss._confidence_generator
    cg.update(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0]))
    mean = cg.mean.clone()
    loss.reset()
    assert torch.equal(cg.mean, mean)


def test_load_clears_moving_average_window_and_keeps_reference_keys(fx):
    for method in ("running_mean", "kalman_filter"):
        sd = fx["ref_loss_sd"][method]
        loss = TraversabilityLoss(0.03, 0.5, 0.0, True, SimpleMLP(90, [256, 32, 1], True), method, 0.5)
        loss.load_state_dict(sd, strict=True)
        own = {k: v for k, v in sd.items() if k.startswith("_confidence_generator.")}
        for k, v in loss.state_dict().items():
            if k in own:
                assert torch.equal(v, own[k]) and v.dtype == own[k].dtype, k
    cg = ConfidenceGenerator(std_factor=0.5, method="moving_average")
    cg.update(torch.ones(3), torch.ones(3))
    cg.load_state_dict(cg.state_dict())
    assert len(cg.data_window) == 0


@pytest.mark.parametrize("case", CASES)
def test_loss_forward_matches_reference_step0(fx, golden, case):
    c = fx["cases"][case]
    src = golden("mlp_train.pt")["graph_pt_D90"]
    r = c["rows"][0]
    x, y, yv = src["x"][r], src["y"][r], src["y_valid"][r]
    res = OM.mlp_forward(src["sd0"], x)
    loss_fn = TraversabilityLoss(0.03, 0.5, 0.0, c["balanced"], SimpleMLP(90, [256, 32, 1], True), c["method"], 0.5)
    loss, aux, _ = loss_fn(Data(x=x, y=y, y_valid=yv), res)
    cg = loss_fn._confidence_generator
    got = torch.tensor([loss.item(), aux["loss_trav"].item(), aux["loss_reco"].item(), cg.mean.item(), cg.var.item(), cg.std.item()])
    assert torch.allclose(got, c["traj"][0], rtol=1e-5, atol=1e-6), (got, c["traj"][0])
    assert torch.allclose(aux["confidence"], c["conf"][0], atol=1e-5)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("balanced", [True, False])
def test_estimator_constructs_for_every_method(method, balanced):
    p = ExperimentParams()
    p.loss.method = method
    p.loss.anomaly_balanced = balanced
    te = TraversabilityEstimator(p, device="cpu")
    assert te._traversability_loss._confidence_generator.method == method
    assert te._optimizer.method == method and te._optimizer.anomaly_balanced == balanced


def test_cross_entropy_and_unknown_method_still_refused():
    with pytest.raises(ValueError, match="trav_cross_entropy"):
        TraversabilityLoss(0.03, 0.5, 0.0, True, SimpleMLP(90, [256, 32, 1], True), "latest_measurement", 0.5,
                           trav_cross_entropy=True)
    with pytest.raises(ValueError):
        ConfidenceGenerator(0.5, method="median")
    with pytest.raises(ValueError):
        MlpTrainer(SimpleMLP(90, [256, 32, 1], True), method="median")


# ---- C-ABI: argument checks of the *_conf entry points, before any GPU call -----------------------------------------------
ERR_ARG = 1001
P = 1 << 20   # a stand-in device pointer (never dereferenced: every call below is refused first)


def _calls(conf):
    h = _lib.lib()
    d = _lib.MlpDesc(90, 256, 32, 0)
    cp = C.byref(conf) if conf is not None else None
    return [
        h.wvn_mlp_train_phase_a_conf(C.byref(d), P, P, 90, P, 32, None, P, P, 1 << 24, P, cp, None),
        h.wvn_mlp_train_phase_b_conf(C.byref(d), P, P, 90, P, P, 32, None, P, 0.5, 0.03, 0.5, P, None, P, 1 << 24, 1, cp, None),
        h.wvn_mlp_train_phase_c_conf(C.byref(d), P, P, P, P, 1, 1e-3, P, 0.03, 0.5, P, cp, None),
    ]


def test_conf_entry_points_check_arguments_on_the_host():
    bad = [None,
           _lib.ConfDesc(4, 1, P, P),                                          # unknown method
           _lib.ConfDesc(-1, 1, P, P),
           _lib.ConfDesc(_lib.CONF_METHODS["running_mean"], 1, None, P),       # no state
           _lib.ConfDesc(_lib.CONF_METHODS["latest_measurement"], 0, None, None),
           _lib.ConfDesc(_lib.CONF_METHODS["moving_average"], 1, P, None)]     # moving_average without its min / max
    for conf in bad:
        assert _calls(conf) == [ERR_ARG] * 3, conf and (conf.method, conf.state, conf.minmax)
    # a valid descriptor reaches the step's own checks (R = 0 / step = 0 / NULL losses: still refused on the host)
    h = _lib.lib()
    d = _lib.MlpDesc(90, 256, 32, 0)
    ok = _lib.ConfDesc(_lib.CONF_METHODS["kalman_filter"], 1, P, None)
    assert h.wvn_mlp_train_phase_a_conf(C.byref(d), P, P, 90, P, 0, None, P, P, 1 << 24, P, C.byref(ok), None) == ERR_ARG
    assert h.wvn_mlp_train_phase_c_conf(C.byref(d), P, P, P, P, 0, 1e-3, P, 0.03, 0.5, P, C.byref(ok), None) == ERR_ARG
    assert h.wvn_mlp_train_phase_c_conf(C.byref(d), P, P, P, P, 1, 1e-3, P, 0.03, 0.5, None, C.byref(ok), None) == ERR_ARG
