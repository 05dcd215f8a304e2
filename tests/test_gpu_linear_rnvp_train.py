"""The fused training step of the anomaly-detection mode (csrc/rnvp_train.hip, RnvpTrainer) on the GPU: the flat gradient
against the float64 statement (tests/linear_rnvp_ref.py), the structural zeros, reproducibility, one step and the estimator's
trajectory against the float64 step and the reference's own numbers (tests/golden/linear_rnvp_train.pt), checkpoints in both
directions with ``torch.optim.Adam``, and two data-parallel ranks.

Tolerances:
  gradient, per parameter tensor   max(4 x own_err_t, 2^-16 x max|g64_t|): own_err_t is the reference's own fp32 autograd gradient
          against the float64 statement, recorded per case, row count and tensor in the fixture; 2^-16 is the resolution of a
          hi + lo 16-bit operand pair (the rule of tests/test_gpu_linear_rnvp.py's docstring).
  loss / mean / std trajectories   rtol 3e-4, atol 2e-6 (the estimator tests' trajectory tolerance).
"""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_rnvp_ref as REF  # noqa: E402
import linear_rnvp_train_cases as CASES  # noqa: E402

from wild_visual_navigation_amd import _lib  # noqa: E402
from wild_visual_navigation_amd.cfg import ExperimentParams  # noqa: E402
from wild_visual_navigation_amd.model import LinearRnvp  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import MissionNode, RnvpTrainer, TraversabilityEstimator  # noqa: E402
from wild_visual_navigation_amd.utils import AnomalyLoss, ConfidenceGenerator, Data  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 3e-4, 2e-6


def _trainer(sd, D, h, mask_type, dev, method="latest_measurement", lr=1e-3):
    m = LinearRnvp(D, [h], use_permutation=True, mask_type=mask_type)
    m.load_state_dict(sd, strict=True)
    m.to(dev).train()
    return RnvpTrainer(m, lr=lr, method=method)


def _grad64(sd, x, flips=None, record=None):
    """The float64 gradient of -mean(score), per parameter tensor in PARAM_KEYS order.  ``record``: a list that receives the
    pre-activation of every ReLU of REF.flow, in call order.  ``flips``: {call index: [(row, unit), ...]} -- the ReLUs whose
    OTHER one-sided derivative is taken (see _kink_alternatives)."""
    sd64 = {k: (v.double().clone().requires_grad_(k in REF.PARAM_KEYS) if v.is_floating_point() else v) for k, v in sd.items()}
    calls, orig = [0], torch.relu

    def relu(a):
        i = calls[0]
        calls[0] += 1
        if record is not None:
            record.append(a.detach())
        if not flips or i not in flips:
            return orig(a)
        mask = a.detach() > 0
        for r, u in flips[i]:
            mask[r, u] = ~mask[r, u]
        return a * mask

    torch.relu = relu   # (REF._net calls torch.relu: the statement itself stays as it is)
    try:
        return torch.autograd.grad(-REF.flow(sd64, x)[2].mean(), [sd64[k] for k in REF.PARAM_KEYS])
    finally:
        torch.relu = orig


def _kink_units(sd, x):
    """A ReLU network's gradient is discontinuous where a pre-activation crosses zero.  The kernel's pre-activations are the
    float64 ones to 2^-16 x max|a| of their layer (the forward rule of tests/test_gpu_linear_rnvp.py), so for a unit whose float64
    pre-activation lies within that distance of zero the kernel may rightly stand on either side of the kink, and the gradient
    it then owes is the one-sided one of ITS side.  Returns those units as (ReLU call index, row, unit)."""
    rec = []
    _grad64(sd, x, record=rec)
    return [(i, r, u) for i, a in enumerate(rec) for r, u in (a.abs() <= 2.0 ** -16 * a.abs().max()).nonzero().tolist()]


def _grad_misses(g, g64, own_err, R):
    """([(R, key, err, tol)] of the tensors that miss max(4 own_err, 2^-16 max|g64|), max over tensors of err / tol, of err / max|g64|)."""
    miss, worst, rel = [], 0.0, 0.0
    for i, k in enumerate(REF.PARAM_KEYS):
        err = (g[i].double() - g64[i]).abs().max().item()
        gmax = g64[i].abs().max().item()
        tol = max(4 * own_err[i], 2.0 ** -16 * gmax)
        worst, rel = max(worst, err / tol), max(rel, err / gmax)
        if not err <= tol:
            miss.append((R, k, err, tol))
    return miss, worst, rel


def _compare_gradient(g, sd, x, own_err, R):
    """The kernel's gradient against the float64 one; where that misses, against the one-sided float64 gradients of the units at a
    kink (_kink_units), taken one unit at a time and kept where the side fits the kernel's better.  Returns (misses against the
    PLAIN float64 gradient unless an admissible one fits, err / max|g64| of the reference used, the flips used)."""
    plain = _grad_misses(g, _grad64(sd, x), own_err, R)
    if not plain[0]:
        return [], plain[2], {}
    flips, best = {}, plain
    for i, r, u in _kink_units(sd, x):
        trial = {k: list(v) for k, v in flips.items()}
        trial.setdefault(i, []).append((r, u))
        res = _grad_misses(g, _grad64(sd, x, flips=trial), own_err, R)
        if res[1] < best[1]:
            flips, best = trial, res
    return (best[0], best[2], flips) if not best[0] else (plain[0], plain[2], {})


def _split(flat, sd):
    out, off = [], 0
    for k in REF.PARAM_KEYS:
        n = sd[k].numel()
        out.append(flat[off: off + n].view(sd[k].shape))
        off += n
    assert off == flat.numel()
    return out


def _structural_zero_masks(sd):
    """Per PARAM_KEYS tensor: a bool tensor of the entries the masks disconnect (None: none)."""
    out = []
    for k in REF.PARAM_KEYS:
        m = sd[k.split(".")[0] + "." + k.split(".")[1] + ".mask"]
        z = None
        if k.endswith(".0.weight"):
            z = (m == 0)[None, :].expand_as(sd[k])      # layer-1 columns at m = 0 positions
        elif k.endswith(".4.weight"):
            z = (m == 1)[:, None].expand_as(sd[k])      # layer-3 rows at m = 1 positions
        elif k.endswith(".4.bias"):
            z = m == 1
        out.append(z)
    return out


# ---- 1, 2: gradient against float64, structural zeros ------------------------------------------------------------------------
@pytest.mark.parametrize("D,mask_type,h", CASES.GRAD_CASES)
def test_gradient_matches_float64_and_structural_zeros(dev, golden, D, mask_type, h):
    assert int(_lib.lib().wvn_rnvp_row_tile()) == CASES.TILE
    fx = golden("linear_rnvp_train.pt")["grad"][CASES.case_key(D, mask_type, h)]
    sd = CASES.case_sd(D, mask_type, h)
    x = CASES.case_rows(golden("mlp_train.pt"), D)
    zero_at = _structural_zero_masks(sd)
    tr = _trainer(sd, D, h, mask_type, dev)
    n = _lib.lib().wvn_rnvp_train_param_count(C.byref(tr.model.desc))
    assert n == sum(sd[k].numel() for k in REF.PARAM_KEYS)
    bad = []
    for R in CASES.ROW_COUNTS:
        g = _split(tr.forward_backward(x[:R].to(dev)).cpu(), sd)
        for i in range(len(g)):
            if zero_at[i] is not None:
                assert torch.equal(g[i][zero_at[i]], torch.zeros(int(zero_at[i].sum()))), (R, REF.PARAM_KEYS[i])   # exactly 0.0
                assert g[i][~zero_at[i]].abs().max().item() > 0
        miss, rel, flips = _compare_gradient(g, sd, x[:R], fx[R]["own_err"], R)
        bad += miss
        print(f"grad D {D} {mask_type} h {h} R {R}: max over tensors of err / max|g64| = {rel:.3e} (2^-16 = {2.0 ** -16:.3e})"
              + (f"  [one-sided at (relu call, row, unit) {flips}]" if flips else ""))
    assert not bad, bad
    # three full steps: Adam on a zero gradient moves nothing
    for _ in range(3):
        tr.train_step(x[:33].to(dev))
    after = _split(tr.model.flat_params().cpu(), sd)
    moved = 0.0
    for i, k in enumerate(REF.PARAM_KEYS):
        if zero_at[i] is not None:
            assert torch.equal(after[i][zero_at[i]], sd[k][zero_at[i]]), k
            moved = max(moved, (after[i][~zero_at[i]] - sd[k][~zero_at[i]]).abs().max().item())
    assert moved > 1e-4   # (lr 1e-3: the connected parameters did move)


# ---- 3: row independence and reproducibility ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [90, 384])
def test_step_is_reproducible_and_scores_match_forward(dev, golden, D):
    sd = CASES.case_sd(D, "odds", 200)
    R = 2 * CASES.TILE + 5
    x = CASES.case_rows(golden("mlp_train.pt"), D)[:R].to(dev)
    wide = torch.zeros(R, D + 7, device=dev)
    wide[:, :D] = x
    xs = wide[:, :D]
    assert xs.stride(0) == D + 7
    runs = []
    for rows in (x, x, xs):
        tr = _trainer(sd, D, 200, "odds", dev)
        fwd_score = tr.model.forward_rows(x, want_z=False)[0]
        losses = tr.train_step(rows).clone()
        assert torch.equal(tr.last_score, fwd_score)          # phase A's score is the forward kernel's
        runs.append((tr.model.flat_params().clone(), tr.m.clone(), tr.v.clone(), losses, tr.grads.clone()))
    for other in runs[1:]:                                     # the same state twice, and a strided x: the same bits
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert torch.isfinite(runs[0][3]).all()


# ---- 4: one step against the float64 step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["latest_measurement", "running_mean"])
@pytest.mark.parametrize("D", [90, 384])
def test_one_step_matches_float64_step(dev, golden, D, method):
    src = golden("mlp_train.pt")
    if D == 90:
        sd, x = REF.expand_sd0(golden("linear_rnvp.pt")["d90"]["sd0"]), src["graph_pt_D90"]["x"]
    else:
        sd, x = CASES.traj_sd(), CASES.traj_rows(src)
    ref = REF.F64Step(sd, method, lr=1e-3)
    want_loss, _ = ref.step(x)
    tr = _trainer(sd, D, 200, "odds", dev, method=method, lr=1e-3)
    cg = ConfidenceGenerator(std_factor=0.5, method=method).to(dev)
    tr.load_confidence_state(cg)
    got = tr.train_step(x.to(dev)).cpu().tolist()
    print(f"one step D {D} {method}: loss {got[0]:.6f} / {want_loss:.6f}  mean {got[1]:.6f} / {ref.mean:.6f}  std {got[2]:.6f} / {ref.std:.6f}")
    assert np.allclose(got, [want_loss, ref.mean, ref.std], rtol=RTOL, atol=ATOL)
    tr.store_confidence_state(cg)
    assert np.allclose([cg.mean.item(), cg.std.item()], [ref.mean, ref.std], rtol=RTOL, atol=ATOL)
    # the kernel route on the updated weights: the re-pack of phase C
    tr.model.eval()
    score = tr.model.forward_rows(x.to(dev), want_z=False)[0]
    with torch.no_grad():
        want = REF.flow(ref.sd, x)[2].mean().item()
    assert abs(score.mean().item() - want) <= 3e-4 * abs(want)
    assert not torch.equal(score, tr.last_score)              # (the images are those of the new weights)
    packed = tr.model._packed
    tr.model.forward_rows(x.to(dev), want_z=False)
    assert tr.model._packed is packed


# ---- 5: the estimator ---------------------------------------------------------------------------------------------------------
def _estimator(dev, method, D=384, sd=None):
    p = ExperimentParams()
    p.model.name = "LinearRnvp"
    p.model.linear_rnvp_cfg.input_size = D
    p.loss_anomaly.method = method
    te = TraversabilityEstimator(p, device=dev, min_samples_for_training=2, anomaly_detection=True)
    if sd is not None:
        te._model.load_state_dict(sd, strict=True)
    return te


def _add_nodes(te, x, dev, t0=0.0):
    S, Hs = 25, 50
    for i in range(4):   # 100 rows as four nodes of 25 labelled segments: a batch holds all of them, in some order
        n = MissionNode(timestamp=t0 + float(i))
        n.features = x[25 * i: 25 * i + 25].to(dev)
        n.feature_segments = (torch.arange(Hs * Hs).reshape(Hs, Hs) * S // (Hs * Hs)).to(dev)
        assert te.add_mission_node(n)
        te.update_supervision(n, torch.full((3, Hs, Hs), 0.7, device=dev))


def test_estimator_reproduces_reference_trajectory_d384(dev, golden):
    want = golden("linear_rnvp_train.pt")["traj"].numpy()
    te = _estimator(dev, "latest_measurement", sd=CASES.traj_sd())
    assert isinstance(te._optimizer, RnvpTrainer)
    _add_nodes(te, CASES.traj_rows(golden("mlp_train.pt")), dev)
    cg = te._traversability_loss._confidence_generator
    traj = []
    for _ in range(CASES.TRAJ_STEPS):
        out = te.train()
        assert out["loss_trav"] == 0.0 and out["loss_reco"] == 0.0 and out["mission_graph_num_valid_node"] == 4
        traj.append([out["loss_total"], cg.mean.item(), cg.std.item()])
    traj = np.array(traj)
    print(f"estimator D 384: max traj err {np.abs(traj - want).max():.3e}")
    assert te.step == CASES.TRAJ_STEPS and abs(te.loss - traj[-1][0]) <= 1e-6 * abs(traj[-1][0])
    assert np.allclose(traj, want, rtol=RTOL, atol=ATOL), np.abs(traj - want).max()


@pytest.mark.parametrize("method", ["kalman_filter", "moving_average"])
def test_estimator_other_methods_match_host_generator(dev, golden, method):
    """The statistic committed on the device against AnomalyLoss + ConfidenceGenerator driven on the host with the same scores."""
    te = _estimator(dev, method, sd=CASES.traj_sd())
    _add_nodes(te, CASES.traj_rows(golden("mlp_train.pt")), dev)
    cg = te._traversability_loss._confidence_generator
    host = AnomalyLoss(0.5, method).to(dev)
    hcg = host._confidence_generator
    for step in range(3):
        out = te.train()
        score = te._optimizer.last_score
        assert score.shape == (100,)
        loss, _, _ = host(None, {"logprob": score[:, None], "log_det": torch.zeros_like(score)}, step=step)
        got = [out["loss_total"], cg.mean.item(), cg.std.item()]
        want = [loss.item(), hcg.mean.item(), hcg.std.item()]
        print(f"{method} step {step}: {got} / {want}")
        assert np.allclose(got, want, rtol=RTOL, atol=ATOL)
    for k, v in te._traversability_loss.state_dict().items():
        if k in ("_confidence_generator.mean", "_confidence_generator.var", "_confidence_generator.std"):
            assert torch.allclose(v.double().cpu(), host.state_dict()[k].double().cpu(), rtol=RTOL, atol=ATOL), k


# ---- 6: checkpoints both ways -------------------------------------------------------------------------------------------------
def _autograd_step(model, opt, x):
    loss, _, _ = AnomalyLoss(0.5, "latest_measurement").to(x.device)(None, model(Data(x=x)))
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.item()


def _score_mean(model, x):
    model.eval()
    s = model.forward_rows(x, want_z=False)[0].mean().item()
    model.train()
    return s


def test_checkpoints_load_both_ways(dev, golden, tmp_path):
    x = golden("mlp_train.pt")["graph_pt_D90"]["x"]
    xd = x.to(dev)
    te = _estimator(dev, "latest_measurement", D=90)
    _add_nodes(te, x, dev)
    for _ in range(2):
        te.train()
    f = te.save_checkpoint(str(tmp_path))
    ck = torch.load(f, weights_only=False)
    assert sorted(ck["optimizer_state_dict"]["state"]) == list(range(24))
    assert int(ck["optimizer_state_dict"]["state"][0]["step"]) == 2
    # fused -> torch.optim.Adam over a fresh model's parameters
    fresh = LinearRnvp(90, [200], use_permutation=True).to(dev).train()
    fresh.load_state_dict(ck["model_state_dict"])
    opt = torch.optim.Adam(fresh.parameters(), lr=1e-3)
    opt.load_state_dict(ck["optimizer_state_dict"])
    la = _autograd_step(fresh, opt, xd)
    lf = te.train()["loss_total"]
    assert abs(la - lf) <= 1e-5 * abs(lf)
    sa, sf = _score_mean(fresh, xd), _score_mean(te._model, xd)
    print(f"checkpoint fused -> Adam: score mean after one more step {sa:.6f} / {sf:.6f}")
    assert abs(sa - sf) <= 1e-5 * abs(sf)
    # torch.optim.Adam -> fused
    ck2 = dict(ck, step=3, model_state_dict={k: v.detach().clone() for k, v in fresh.state_dict().items()},
               optimizer_state_dict=opt.state_dict())
    f2 = os.path.join(str(tmp_path), "from_adam.pt")
    torch.save(ck2, f2)
    te2 = _estimator(dev, "latest_measurement", D=90)
    te2.load_checkpoint(f2)
    _add_nodes(te2, x, dev)
    assert te2.step == 3 and te2._optimizer.step == 3
    lf2 = te2.train()["loss_total"]
    la2 = _autograd_step(fresh, opt, xd)
    assert abs(la2 - lf2) <= 1e-5 * abs(lf2)
    sa, sf = _score_mean(fresh, xd), _score_mean(te2._model, xd)
    print(f"checkpoint Adam -> fused: score mean after one more step {sa:.6f} / {sf:.6f}")
    assert abs(sa - sf) <= 1e-5 * abs(sf)


# ---- 7: two ranks ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from wild_visual_navigation_amd import distributed as Dist

    Dist.init_from_env(backend="gloo")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    x = torch.load(os.path.join(ROOT, "tests", "golden", "mlp_train.pt"), weights_only=False)["graph_pt_D90"]["x"].to(dev)
    sd = REF.expand_sd0(torch.load(os.path.join(ROOT, "tests", "golden", "linear_rnvp.pt"), weights_only=False)["d90"]["sd0"])
    tr = _trainer(sd, 90, 200, "odds", dev)
    tr.comm_events = []
    traj = []
    for step in range(6):
        if step % 2 == 0:
            lo, hi = (0, 60) if rank == 0 else (60, 100)
        else:                  # rank 1's shard is EMPTY: it still takes part in both collectives
            lo, hi = (0, 100) if rank == 0 else (100, 100)
        traj.append(tr.train_step(x[lo:hi]).cpu().tolist())
    assert len(tr.comm_events) == 12
    p = ExperimentParams()
    p.model.name = "LinearRnvp"
    p.model.linear_rnvp_cfg.input_size = 90
    te = TraversabilityEstimator(p, device=dev, min_samples_for_training=2, anomaly_detection=True)   # world size 2: no refusal
    ok = isinstance(te._optimizer, RnvpTrainer)
    torch.cuda.synchronize()
    Dist.barrier()
    q.put((rank, traj, [t.cpu().numpy().copy() for t in (tr.model.flat_params(), tr.m, tr.v)], ok))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(400)
def test_two_ranks_match_one_rank(dev, golden):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=280) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, t0, s0, ok0), (_, t1, s1, ok1) = res
    assert ok0 and ok1
    assert t0 == t1, "ranks disagree on the losses"
    for a, b in zip(s0, s1):
        assert (a.view(np.int32) == b.view(np.int32)).all(), "replicas diverged"
    x = golden("mlp_train.pt")["graph_pt_D90"]["x"].to(dev)
    tr = _trainer(REF.expand_sd0(golden("linear_rnvp.pt")["d90"]["sd0"]), 90, 200, "odds", dev)
    one = [tr.train_step(x).cpu().tolist() for _ in range(6)]
    print(f"two ranks vs one: max traj err {np.abs(np.array(t0) - np.array(one)).max():.3e}")
    assert np.allclose(np.array(t0), np.array(one), rtol=RTOL, atol=ATOL)
