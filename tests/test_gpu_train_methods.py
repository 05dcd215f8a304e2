"""The training step with every ConfidenceGenerator method and anomaly_balanced=False on the GPU (the *_conf entry points of
csrc/mlp_train.hip and csrc/mlp.hip):

* 12 steps of each case of tests/golden/mlp_train_methods.pt -- the reference's SimpleMLP + TraversabilityLoss + Adam on a
  varying row subset -- on the four-launch and on the general path;
* bit-level contracts: a compacted batch (rows_dev) equals the uncompacted one, and the default configuration through the
  new entry points equals the original entry points;
* R = 2048 (four-launch) and R = 5000 (general) against an fp64 restatement of the step kept below;
* TraversabilityEstimator: 30 steps, save / load, the ConfidenceGenerator hand-off and the per-segment inference."""
import numpy as np
import pytest
import torch

from wild_visual_navigation_amd.cfg import ExperimentParams
from wild_visual_navigation_amd.model import SimpleMLP
from wild_visual_navigation_amd.traversability_estimator import MlpTrainer, TraversabilityEstimator
from wild_visual_navigation_amd.utils import ConfidenceGenerator, Data

pytestmark = pytest.mark.gpu

CASES = ["running_mean_balanced", "running_mean_unbalanced", "kalman_filter_balanced", "kalman_filter_unbalanced",
         "moving_average_balanced", "moving_average_unbalanced", "latest_measurement_unbalanced"]
METHODS = ["latest_measurement", "running_mean", "kalman_filter", "moving_average"]


def _model(sd0, D, dev):
    m = SimpleMLP(D, [256, 32, 1], True)
    m.load_state_dict(sd0)
    return m.to(dev)


def _conf_atol(c, step):
    """running_mean keeps the population variance as sum_sq / n - mean^2.  The reference forms the two sums in fp32
    (x_positive.sum(), (x_positive ** 2).sum()), the step in fp64: they differ by ~1 ulp of mean^2 + var, which the cancellation
    scales by (mean^2 + var) / var in var (half of it in std), and conf = 1 - (x - lo) / (2 std) inherits it.  Step 0 has two
    positives 0.075 apart around 1.55: (mean^2 + var) / var ~ 1700.  Every other method: the usual 1e-5."""
    if c["method"] != "running_mean":
        return 1e-5
    m, v = c["traj"][step, 3].item(), c["traj"][step, 4].item()
    return 1e-5 + 2.0 ** -22 * (m * m + v) / v


def _row(tr, losses):
    lo = losses.cpu()
    return [lo[0].item(), lo[1].item(), lo[2].item(), lo[3].item(), tr.conf_state[1].item(), lo[4].item()]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_twelve_steps_match_reference(dev, golden, case, fused):
    c = golden("mlp_train_methods.pt")["cases"][case]
    src = golden("mlp_train.pt")["graph_pt_D90"]
    m = _model(src["sd0"], 90, dev)
    tr = MlpTrainer(m, lr=1e-3, std_factor=0.5, w_trav=0.03, w_reco=0.5, fused=fused, method=c["method"],
                    anomaly_balanced=c["balanced"])
    traj = []
    for step, r in enumerate(c["rows"]):
        losses = tr.train_step(src["x"][r].to(dev), src["y"][r].to(dev), src["y_valid"][r].to(dev), want_confidence=True)
        traj.append(_row(tr, losses))
        assert torch.allclose(tr.last_confidence.cpu(), c["conf"][step], atol=_conf_atol(c, step)), \
            (step, (tr.last_confidence.cpu() - c["conf"][step]).abs().max())
    traj = np.array(traj)
    assert np.allclose(traj, c["traj"].numpy(), rtol=3e-4, atol=2e-6), np.abs(traj - c["traj"].numpy()).max()
    for k, v in m.state_dict().items():
        assert torch.allclose(v.cpu(), c["sd12"][k], atol=3e-5), (k, (v.cpu() - c["sd12"][k]).abs().max())
    cg = ConfidenceGenerator(0.5, c["method"]).to(dev)
    tr.store_confidence_state(cg)
    for k, v in cg.state_dict().items():
        want = c["cg12"][k]
        assert v.dtype == want.dtype and torch.allclose(v.cpu().double(), want.double(), rtol=1e-5, atol=1e-6), k


@pytest.mark.parametrize("method", METHODS[1:])
def test_d384_trajectories(dev, golden, method):
    c = golden("mlp_train_methods.pt")["d384"][method]
    src = golden("mlp_train.pt")["synthetic_D384"]
    for fused in (True, False):
        tr = MlpTrainer(_model(src["sd0"], 384, dev), fused=fused, method=method)
        traj = [_row(tr, tr.train_step(src["x"][r].to(dev), src["y"][r].to(dev), src["y_valid"][r].to(dev))) for r in c["rows"]]
        assert np.allclose(np.array(traj), c["traj"].numpy(), rtol=3e-4, atol=2e-6), (fused, np.abs(np.array(traj) - c["traj"].numpy()).max())


@pytest.mark.parametrize("method", METHODS)
def test_compacted_batch_gives_the_same_bits(dev, golden, method):
    src = golden("mlp_train.pt")["graph_pt_D90"]
    x, y, yv = src["x"], src["y"], src["y_valid"]
    n = 70
    xg, yg = x.clone(), y.clone()
    xg[n:] = 5.0                      # rows past the count: their loss would be the step's max if it were counted
    rows_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    for fused in (True, False):
        ma, mb = _model(src["sd0"], 90, dev), _model(src["sd0"], 90, dev)
        ta, tb = MlpTrainer(ma, fused=fused, method=method), MlpTrainer(mb, fused=fused, method=method)
        ta._conf = tb._conf = True   # (latest_measurement too: through the *_conf entry points)
        for _ in range(3):
            la = ta.train_step(xg.to(dev), yg.to(dev), yv.to(dev), rows_dev=rows_dev, want_confidence=True).cpu()
            lb = tb.train_step(x[:n].to(dev), y[:n].to(dev), yv[:n].to(dev), want_confidence=True).cpu()
            if fused:   # the four-launch step walks the same tiles
                assert torch.equal(la, lb) and torch.equal(ta.conf_state, tb.conf_state)
                assert torch.equal(ta.last_confidence[:n], tb.last_confidence)
            else:       # the general path's GEMMs see R rows (another split-K)
                assert torch.allclose(la, lb, rtol=1e-5, atol=2e-6)
                assert torch.allclose(ta.conf_state, tb.conf_state, rtol=1e-6, atol=1e-9)
                assert torch.allclose(ta.last_confidence[:n], tb.last_confidence, atol=1e-5)
        for k, v in ma.state_dict().items():
            assert torch.equal(v, mb.state_dict()[k]) if fused else torch.allclose(v, mb.state_dict()[k], atol=1e-5), k


def test_default_configuration_through_the_conf_entry_points_gives_the_same_bits(dev, golden):
    src = golden("mlp_train.pt")["graph_pt_D90"]
    x, y, yv = src["x"].to(dev), src["y"].to(dev), src["y_valid"].to(dev)
    for fused in (True, False):
        ma, mb = _model(src["sd0"], 90, dev), _model(src["sd0"], 90, dev)
        ta, tb = MlpTrainer(ma, fused=fused), MlpTrainer(mb, fused=fused)
        assert not ta._conf
        tb._conf = True   # latest_measurement + anomaly_balanced through wvn_mlp_train_phase_*_conf
        for _ in range(5):
            la = ta.train_step(x, y, yv, want_confidence=True).clone()
            lb = tb.train_step(x, y, yv, want_confidence=True).clone()
            assert torch.equal(la, lb) and torch.equal(ta.last_confidence, tb.last_confidence)
        assert all(torch.equal(v, mb.state_dict()[k]) for k, v in ma.state_dict().items())
        assert torch.equal(tb.conf_state[0].float(), la[3]) and torch.equal(tb.conf_state[2].float(), la[4])


# ---- fp64 restatement of the step (reference arithmetic: loss.py:93-160, confidence_generator.py, torch.optim.Adam) -----------
class F64Step:
    def __init__(self, sd, method, balanced, f=0.5, w_trav=0.03, w_reco=0.5, lr=1e-3):
        self.p = {k: v.double().clone() for k, v in sd.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.method, self.balanced, self.f, self.w_trav, self.w_reco, self.lr, self.t = method, balanced, f, w_trav, w_reco, lr, 0
        self.mean, self.var, self.std = 0.0, 1.0, 1.0
        self.run = [0.0, 0.0, 0.0]
        self.window = []

    def _update(self, lr, pos):
        n, s, s2 = float(pos.numel()), float(pos.sum()), float((pos ** 2).sum())
        if self.method == "running_mean":
            self.run = [self.run[0] + n, self.run[1] + s, self.run[2] + s2]
            self.mean = self.run[1] / self.run[0]
            self.var = self.run[2] / self.run[0] - self.mean ** 2
            self.std = self.var ** 0.5
        elif self.method == "kalman_filter":
            if n > 0:
                vp = self.var + 0.2
                k = vp / (vp + 1.0)
                self.mean += k * (s / n - self.mean)
                self.var = (1 - k) * vp
            self.std = self.var ** 0.5
        elif self.method == "moving_average":
            self.window = (self.window + [pos])[-5:]
            w = torch.cat(self.window)
            self.mean, self.std = float(w.mean()), float(w.std())
        else:
            self.mean, self.std = float(pos.mean()), float(pos.std())
        if self.method == "kalman_filter":
            c = torch.exp(-0.5 * ((lr - self.mean) / (self.std * self.f)) ** 2)
            return torch.where(lr < self.mean, torch.ones_like(c), c)
        if self.method == "moving_average":
            xc = lr.clamp(self.mean - 2 * self.std, self.mean + 2 * self.std)
            return (xc - xc.min()) / (xc.max() - xc.min())
        sh = self.mean + self.std * self.f
        lo, hi = max(sh - self.std, 0.0), sh + self.std
        return 1 - (lr.clamp(lo, hi) - lo) / (hi - lo)

    def step(self, x, y, yv):
        x, y = x.double(), y.double()
        p = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        ks = list(p)
        h = x
        for i in range(0, len(ks) - 2, 2):
            h = torch.relu(h @ p[ks[i]].T + p[ks[i + 1]])
        out = h @ p[ks[-2]].T + p[ks[-1]]
        s = torch.sigmoid(out[:, 0])
        lr = ((out[:, 1:] - x) ** 2).mean(1)
        conf = self._update(lr.detach(), lr.detach()[yv])
        raw = (s - y) ** 2
        trav = torch.where(yv, raw, raw * (1 - conf)).sum() / len(y) if self.balanced else raw.mean()
        loss = self.w_trav * trav + self.w_reco * lr[yv].mean()
        loss.backward()
        self.t += 1
        for k in ks:
            g = p[k].grad
            self.m[k] = 0.9 * self.m[k] + 0.1 * g
            self.v[k] = 0.999 * self.v[k] + 0.001 * g * g
            den = (self.v[k] / (1 - 0.999 ** self.t)).sqrt() + 1e-8
            self.p[k] = self.p[k] - self.lr / (1 - 0.9 ** self.t) * self.m[k] / den
        return [loss.item(), raw.mean().item(), lr[yv].mean().item(), self.mean, self.std], conf


@pytest.mark.parametrize("R,fused", [(2048, True), (5000, False)])
@pytest.mark.parametrize("method", METHODS[1:])
def test_large_batches_match_fp64_restatement(dev, method, R, fused):
    D = 90
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(42)
    sd0 = SimpleMLP(D, [256, 32, 1], True).state_dict()
    m = _model(sd0, D, dev)
    ref = F64Step(sd0, method, balanced=(R == 2048))
    tr = MlpTrainer(m, fused=fused, method=method, anomaly_balanced=(R == 2048))
    for _ in range(3):
        x = torch.randn(R, D, generator=g)
        yv = torch.rand(R, generator=g) < 0.2
        y = yv.float() * (0.5 + 0.5 * torch.rand(R, generator=g))
        want, wconf = ref.step(x, y, yv)
        got = tr.train_step(x.to(dev), y.to(dev), yv.to(dev), want_confidence=True).cpu()
        assert np.allclose(got.numpy(), np.array(want), rtol=1e-4, atol=1e-6), (got, want)
        assert torch.allclose(tr.last_confidence.cpu().double(), wconf, atol=1e-4)
    for k, v in m.state_dict().items():
        assert torch.allclose(v.cpu().double(), ref.p[k], atol=2e-5), (k, (v.cpu().double() - ref.p[k]).abs().max())


# ---- TraversabilityEstimator ----------------------------------------------------------------------------------------------
def _estimator(method, dev):
    p = ExperimentParams()
    p.model.simple_mlp_cfg.input_size = 90
    p.loss.method = method
    return TraversabilityEstimator(p, device=dev, min_samples_for_training=2)


@pytest.mark.parametrize("method", METHODS[1:])
def test_estimator_loop_checkpoint_and_handoff(dev, tmp_path, method):
    te = _estimator(method, dev)
    g = torch.Generator().manual_seed(0)
    batches = []
    for _ in range(31):
        x = torch.randn(60, 90, generator=g)
        yv = torch.rand(60, generator=g) < 0.3
        yv[:2] = True
        batches.append((x.to(dev), (yv.float() * 0.8).to(dev), yv.to(dev)))
    for b in batches[:30]:
        last = te.train_on_batch(*b)
    assert torch.isfinite(last).all()
    cg = te._traversability_loss._confidence_generator
    d = cg.get_dict()
    tr = te._optimizer
    assert float(d["mean"]) == float(tr.conf_state[0]) and float(d["std"]) == float(tr.conf_state[2])
    assert float(d["var"]) == float(tr.conf_state[1]) and float(d["mean"]) != 0.0
    if method == "kalman_filter":   # the variance recursion does not depend on the data when every step has positives
        v = torch.ones(1)
        for _ in range(30):
            vp = v + 0.2
            v = (1 - vp * (1 / (vp + 1))) * vp
        assert torch.allclose(d["var"].cpu().reshape(1), v, rtol=1e-6)
    elif method == "running_mean":
        n, s, s2 = (float(getattr(cg, k)) for k in ("running_n", "running_sum", "running_sum_of_squares"))
        assert n == sum(int(b[2].sum()) for b in batches[:30])
        assert abs(float(d["var"]) - (s2 / n - float(d["mean"]) ** 2)) < 1e-6
    else:
        assert float(d["var"]) == 1.0
    # the per-segment inference reads the updated statistic from the generator
    feat = torch.randn(12, 90, generator=g).to(dev)
    seg = (torch.arange(24 * 24).reshape(24, 24) * 12 // (24 * 24)).to(dev)
    conf_state = torch.cat([cg.mean.detach().float(), cg.std.detach().float(), torch.tensor([0.5], device=dev)])
    trav, conf, loss = te._model.forward_per_segment(feat, seg, want_loss=True, conf_state=conf_state)
    assert torch.allclose(conf, cg.inference_without_update(loss), atol=1e-5)
    # save / load: the next step after a load equals the next step without one (moving_average: its window is not saved,
    # so the comparison run empties its window the same way -- reset() leaves nothing else the update reads)
    f = te.save_checkpoint(str(tmp_path))
    te2 = _estimator(method, dev)
    te2.load_checkpoint(f)
    if method == "moving_average":
        te._traversability_loss.reset()
    l1 = te.train_on_batch(*batches[30]).clone()
    l2 = te2.train_on_batch(*batches[30]).clone()
    assert torch.equal(l1, l2)
    assert torch.equal(te._optimizer.conf_state, te2._optimizer.conf_state)
    for k, v in te._model.state_dict().items():
        assert torch.equal(v, te2._model.state_dict()[k]), k


def test_reference_loss_state_loads_into_the_estimator(dev, golden):
    """A reference traversability_loss_state_dict with running_mean / kalman_filter keys loads strictly, and the next step
    continues from the loaded statistic: it equals the host generator loaded with the same state and fed this step's losses."""
    fx = golden("mlp_train_methods.pt")
    src = golden("mlp_train.pt")["graph_pt_D90"]
    for method in ("running_mean", "kalman_filter"):
        sd = fx["ref_loss_sd"][method]
        te = _estimator(method, dev)
        te._traversability_loss.load_state_dict(sd, strict=True)
        ref = ConfidenceGenerator(0.5, method)
        ref.load_state_dict({k[len("_confidence_generator."):]: v for k, v in sd.items() if k.startswith("_confidence_generator.")})
        r = fx["cases"][f"{method}_balanced"]["rows"][0]
        x, y, yv = src["x"][r].to(dev), src["y"][r].to(dev), src["y_valid"][r].to(dev)
        res = te._model.forward(Data(x=x))
        lr = ((res[:, 1:] - x) ** 2).mean(1).cpu()
        ref.update(lr, lr[yv.cpu()])
        te.train_on_batch(x, y, yv)
        cg = te._traversability_loss._confidence_generator
        for k, v in ref.state_dict().items():
            assert torch.allclose(cg.state_dict()[k].cpu(), v, rtol=1e-5, atol=1e-6), (method, k)
