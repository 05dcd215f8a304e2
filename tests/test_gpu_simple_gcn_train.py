"""The fused SimpleGCN training step (csrc/simple_gcn_train.hip, traversability_estimator/gcn_trainer.py) on the GPU against the
float64 statement of the step (tests/simple_gcn_train_ref.py).

Gradient rule, per tensor (the forward's own, REF.rule): max|g - g64| <= max(8 x the error of the float32 statement's autograd
gradient on the CPU on the same inputs, 2^-16 x max|g64|).  Inputs: x = 2 randn, glorot_state_dict(seed 7), w_trav = 0.03,
w_reco = 0.5, every second row labelled.  Every case prints error, bound and yardstick.

ReLU kinks: a hidden unit is at a kink when its float64 pre-activation lies within 2^-16 x max|pre-activation| of its layer (the
forward's accuracy rule): there the kernel may rightly stand on either side, and the float64 gradient it owes takes that unit's mask
from ``saved_activations()``.  For every other unit the mask is float64's, and the kernel's ``h > 0`` must agree with it.  A case may
admit at most max(2, 1e-3 x its hidden units) units this way; the count is printed.

running_mean's training confidence is compared with the widened tolerance of tests/test_gpu_train_methods.py (``_conf_atol``: the
reference forms its two running sums in fp32, the step in fp64, and the population variance cancels), every other method with 1e-5.

Two ranks against one (test_two_ranks_match_one_rank): the bound is max(8 x the deviation of the float32 CPU autograd trajectory from
the float64 one, per loss, 2^-16 x |loss|).

Measured on an MI355X.  Gradient, error / bound: definition cases at most 2.6e-07 / 1.4e-05; the star with the hub as the only
source 1.3e-06 / 1.7e-05 at max|g64| 1.1, THE WORST (the float32 autograd gradient itself errs by 1.4e-06 there); widths and row
counts at most 3.7e-09 / 7.7e-08.  Kink units: 1 of 38,400 at (90, wide, 100), 4 at (384, wide, 100), 2 of 9,600 at (384, [64, 32, 1],
100), 37 of 307,584 at (384, wide, 801), none elsewhere; the kernel stood on float64's side at every one of them.  One step:
2.8e-08 against a parameter change of 5.0e-02 (bar 7.6e-07), losses within 6e-08 relative.  Methods: losses within 9.6e-07,
training confidence within 1.4e-06.  Two ranks against one: error 0 (the losses agree bit for bit); the float32 CPU trajectory
deviates from the float64 one by {3.8e-07, 2.6e-08, 2.1e-07} for {total, trav, reco}, the one-rank step by 3.8e-07."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_gcn_ref as REF  # noqa: E402
import simple_gcn_train_ref as TREF  # noqa: E402

from wild_visual_navigation_amd.cfg import ExperimentParams  # noqa: E402
from wild_visual_navigation_amd.model import SimpleGCN  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import GcnTrainer, MissionNode, TraversabilityEstimator  # noqa: E402
from wild_visual_navigation_amd.utils import Batch, Data, TraversabilityLoss  # noqa: E402

pytestmark = pytest.mark.gpu

WIDE = [256, 128, 1]
W_TRAV, W_RECO, FAC = 0.03, 0.5, 0.5


def g(seed):
    return torch.Generator().manual_seed(seed)


def _model(dev, D, hidden, seed=7):
    sd = REF.glorot_state_dict(D, hidden, seed)
    m = SimpleGCN(D, True, hidden)
    m.load_state_dict(sd)
    return m.to(dev), sd


def _labels(N, seed):
    yv = torch.arange(N) % 2 == 0
    return yv.float() * (0.5 + 0.5 * torch.rand(N, generator=g(seed))), yv


def _random_edges(N, mean_in_degree, seed):
    return torch.randint(0, N, (2, mean_in_degree * N), generator=g(seed))


def _edges(pairs):
    return torch.tensor(pairs, dtype=torch.long).reshape(-1, 2).t().contiguous()


def _star(N, into_hub):
    k = torch.arange(1, N)
    z = torch.zeros_like(k)
    return torch.stack([k, z]) if into_hub else torch.stack([z, k])


def _run(tr, x, ei, y, yv, dev, step=False, **kw):
    f = tr.train_step if step else tr.forward_backward
    return f(x.to(dev), ei.to(dev), y.to(dev), yv.to(dev), **kw)


# ---- 1: the gradient against float64 -----------------------------------------------------------------------------------------------
GRAD_CASES = {
    "single node": (5, [7, 3, 1], 1, lambda N: _edges([])),
    "path": (5, [7, 3, 1], 3, lambda N: _edges([(0, 1), (1, 2)])),
    "path and back": (5, [7, 3, 1], 3, lambda N: _edges([(0, 1), (1, 2), (1, 0), (2, 1)])),
    "duplicate and self loop": (5, [7, 3, 1], 3, lambda N: _edges([(0, 1), (0, 1), (1, 1), (2, 1)])),
    "isolated node": (5, [7, 3, 1], 4, lambda N: _edges([(0, 1), (1, 2)])),
    "star, hub the only target": (5, [7, 3, 1], 301, lambda N: _star(N, True)),
    "star, hub the only source": (5, [7, 3, 1], 301, lambda N: _star(N, False)),
    "D=5 N=1": (5, [7, 3, 1], 1, lambda N: _random_edges(N, 6, N)),
    "D=5 N=15": (5, [7, 3, 1], 15, lambda N: _random_edges(N, 6, N)),
    "D=5 N=17": (5, [7, 3, 1], 17, lambda N: _random_edges(N, 6, N)),
    "D=5 N=33": (5, [7, 3, 1], 33, lambda N: _random_edges(N, 6, N)),
    "D=90 wide N=100": (90, WIDE, 100, lambda N: _random_edges(N, 6, N)),
    "D=384 wide N=100": (384, WIDE, 100, lambda N: _random_edges(N, 6, N)),
    "D=384 [64,32,1] N=100": (384, [64, 32, 1], 100, lambda N: _random_edges(N, 6, N)),
    "D=384 wide N=801": (384, WIDE, 801, lambda N: _random_edges(N, 6, N)),
    "D=768 wide N=33": (768, WIDE, 33, lambda N: _random_edges(N, 6, N)),
}


@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_gradient_against_float64(dev, name):
    D, hidden, N, make = GRAD_CASES[name]
    ei = make(N)
    x = 2 * torch.randn(N, D, generator=g(D + N))
    y, yv = _labels(N, N)
    m, sd = _model(dev, D, hidden)
    tr = GcnTrainer(m, w_trav=W_TRAV, w_reco=W_RECO, std_factor=FAC)
    got = TREF.flat_to_dict(_run(tr, x, ei, y, yv, dev)[:-2].cpu().double(), sd)
    h1, h2 = (h.cpu() for h in tr.saved_activations())
    # float64: its own masks, and the masks the kernel is owed at the kinks
    A = TREF.dense_adjacency(ei, N)
    z = TREF.preactivations(sd, x, A)
    kink = [zl.abs() <= 2.0 ** -16 * zl.abs().max() for zl in z]
    own = [zl > 0 for zl in z]
    owed = [torch.where(k, h > 0, o) for k, h, o in zip(kink, (h1, h2), own)]
    n_kink, units = sum(int(k.sum()) for k in kink), N * (hidden[0] + hidden[1])
    flipped = sum(int((a != b).sum()) for a, b in zip(owed, own))
    print(f"{name}: {n_kink} kink units of {units} ({flipped} on the other side in the kernel)")
    assert n_kink <= max(2, 1e-3 * units), (n_kink, units)
    for k, h, o in zip(kink, (h1, h2), own):
        assert torch.equal((h > 0)[~k], o[~k]), "the kernel's ReLU mask differs from float64's away from a kink"

    def loss_fn(out):
        dt = out.dtype
        return TREF.loss64(out, x.to(dt), y.to(dt), yv, W_TRAV, W_RECO, FAC)

    g64, _, _ = TREF.backward(sd, x, A, A.t(), owed, loss_fn)
    g64_own = g64 if flipped == 0 else TREF.backward(sd, x, A, A.t(), own, loss_fn)[0]
    sd32 = {k: v.float().requires_grad_() for k, v in sd.items()}
    g32 = dict(zip(sd32, torch.autograd.grad(loss_fn(REF.forward(sd32, x, ei, torch.float32))[0], list(sd32.values()))))
    for k in sd:
        err = (got[k] - g64[k]).abs().max().item()
        err32 = (g32[k].double() - g64_own[k]).abs().max().item()
        bound = max(8 * err32, 2.0 ** -16 * g64[k].abs().max().item())
        print(f"  {k}: err {err:.3e} bound {bound:.3e} (float32 autograd {err32:.3e}, max|g64| {g64[k].abs().max().item():.3e})")
        assert err <= bound, (name, k, err, bound)


# ---- 2: bits ------------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_run_or_edge_order(dev):
    D, N = 90, 100
    x, ei = 2 * torch.randn(N, D, generator=g(1)), _random_edges(N, 6, 2)
    y, yv = _labels(N, 3)
    perm = torch.randperm(ei.shape[1], generator=g(4))
    runs = []
    for edges in (ei, ei, ei[:, perm]):
        m, _ = _model(dev, D, WIDE)
        tr = GcnTrainer(m, lr=1e-3)
        grads = _run(tr, x, edges, y, yv, dev).clone()
        assert torch.equal(grads, _run(tr, x, edges, y, yv, dev))                     # a second call
        out = tr.saved_output()
        losses = [_run(tr, x, edges, y, yv, dev, step=True).clone() for _ in range(3)]
        runs.append((grads, torch.stack(losses), m.flat_params().clone(), out))
        assert int(tr.bad_edges.item()) == 0
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    # phase A's out is the inference forward's, bit for bit
    m, _ = _model(dev, D, WIDE)
    with torch.no_grad():
        assert torch.equal(m.eval()(Data(x=x.to(dev), edge_index=ei.to(dev))), runs[0][3])


# ---- 3: bad edges -------------------------------------------------------------------------------------------------------------------
def test_bad_edges_are_dropped_and_counted(dev):
    D, N = 90, 23
    x, ei = 2 * torch.randn(N, D, generator=g(5)), _random_edges(N, 4, 6)
    y, yv = _labels(N, 7)
    m, _ = _model(dev, D, WIDE)
    tr = GcnTrainer(m)
    clean = _run(tr, x, ei, y, yv, dev).clone()
    assert int(tr.bad_edges.item()) == 0
    bad = torch.cat([ei[:, :10], torch.tensor([[3, -1], [N, 5]]), ei[:, 10:]], dim=1)   # 3 -> N and -1 -> 5
    assert torch.equal(_run(tr, x, bad, y, yv, dev), clean)
    assert int(tr.bad_edges.item()) == 2


# ---- 4: one step against the float64 step -------------------------------------------------------------------------------------------
def test_one_step_against_the_float64_step(dev):
    """The well-conditioned configuration of tests/test_gpu_simple_gcn.py (hidden [8, 4, 1], lr = 0.05, unit loss weights)."""
    D, N, lr = 12, 48, 0.05
    x, ei = 2 * torch.randn(N, D, generator=g(11)), _random_edges(N, 3, 12)
    y, yv = _labels(N, 13)
    m, sd = _model(dev, D, [8, 4, 1])
    tr = GcnTrainer(m, lr=lr, w_trav=1.0, w_reco=1.0, std_factor=FAC)
    losses = _run(tr, x, ei, y, yv, dev, step=True).cpu().double()
    x64, y64 = x.double(), y.double()
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    total, l_trav, l_reco, _ = TREF.loss64(REF.forward(sd64, x64, ei), x64, y64, yv, 1.0, 1.0, FAC)
    grads = dict(zip(sd64, torch.autograd.grad(total, list(sd64.values()))))
    want, _, _ = TREF.adam_steps(sd, lambda p: grads, lr, 1)
    for name, a, b in zip(("total", "trav", "reco"), losses[:3].tolist(), (total, l_trav, l_reco)):
        print(f"loss {name}: {a:.9f} / {b.item():.9f}")
        assert abs(a - b.item()) <= 2.0 ** -16 * abs(b.item()), (name, a, b.item())
    new = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    change = max((want[k] - sd[k].double()).abs().max().item() for k in sd)
    err = max((new[k] - want[k]).abs().max().item() for k in sd)
    print(f"one Adam step: err {err:.3e}, max|param change| {change:.3e}")
    assert change > 0 and err <= 2.0 ** -16 * change


# ---- 5: methods ---------------------------------------------------------------------------------------------------------------------
METHOD_CASES = [(m, b) for m in ("running_mean", "kalman_filter", "moving_average") for b in (True, False)] + [("latest_measurement", False)]


@pytest.mark.parametrize("method,balanced", METHOD_CASES)
def test_methods_against_the_autograd_step(dev, method, balanced):
    D, N, hidden = 12, 60, [8, 4, 1]
    m, sd = _model(dev, D, hidden)
    tr = GcnTrainer(m, method=method, anomaly_balanced=balanced, w_trav=W_TRAV, w_reco=W_RECO, std_factor=FAC)
    cpu = SimpleGCN(D, True, hidden)
    cpu.load_state_dict(sd)
    loss = TraversabilityLoss(w_trav=W_TRAV, w_reco=W_RECO, w_temp=0.0, anomaly_balanced=balanced, model=cpu, method=method,
                              confidence_std_factor=FAC)
    opt = torch.optim.Adam(cpu.parameters(), lr=1e-3)
    for step in range(3):
        x, ei = 2 * torch.randn(N, D, generator=g(20 + step)), _random_edges(N, 4, 30 + step)
        y, yv = _labels(N, 40 + step)
        got = _run(tr, x, ei, y, yv, dev, step=True, want_confidence=True).cpu().numpy()
        graph = Data(x=x, edge_index=ei, y=y, y_valid=yv)
        total, aux, _ = loss(graph, cpu.forward_torch(x, ei), step=step)
        opt.zero_grad()
        total.backward()
        opt.step()
        cg = loss._confidence_generator
        want = np.array([total.item(), aux["loss_trav"].item(), aux["loss_reco"].item(), cg.mean.item(), cg.std.item()])
        atol = 1e-5
        if method == "running_mean":   # tests/test_gpu_train_methods.py: _conf_atol
            atol += 2.0 ** -22 * (want[3] * want[3] + want[4]) / want[4]
        cerr = (tr.last_confidence.cpu() - aux["confidence"]).abs().max().item()
        print(f"{method} balanced={balanced} step {step}: losses {np.abs(got - want).max():.3e}, confidence {cerr:.3e} (atol {atol:.3e})")
        assert np.allclose(got, want, rtol=3e-4, atol=2e-6), (step, got, want)
        assert cerr <= atol, (step, cerr, atol)


# ---- 6: the estimator ---------------------------------------------------------------------------------------------------------------
def _estimator(dev, D=12):
    p = ExperimentParams()
    p.model.name = "SimpleGCN"
    p.model.simple_gcn_cfg.input_size = D
    p.model.simple_gcn_cfg.hidden_sizes = [8, 4, 1]
    p.optimizer.lr, p.loss.w_trav, p.loss.w_reco = 0.05, 1.0, 1.0
    return TraversabilityEstimator(p, device=dev, min_samples_for_training=2)


def _add_nodes(te, dev, D=12, S=12, H=48):
    gen = g(0)
    for i in range(4):
        n = MissionNode(timestamp=float(i))
        n.features = (2 * torch.randn(S, D, generator=gen)).to(dev)
        n.feature_edges = _random_edges(S, 3, 20 + i).to(dev)
        n.feature_segments = (torch.arange(H * H).reshape(H, H) * S // (H * H)).to(dev)
        mask = torch.full((3, H, H), float("nan"))
        mask[:, : H // 2] = 0.5 + 0.5 * torch.rand(3, H // 2, H, generator=gen)
        assert te.add_mission_node(n)
        te.update_supervision(n, mask.to(dev))


def test_estimator_holds_the_fused_trainer_and_checkpoints(dev, tmp_path):
    assert isinstance(_estimator("cpu")._optimizer, torch.optim.Adam)
    te = _estimator(dev)
    assert isinstance(te._optimizer, GcnTrainer)
    _add_nodes(te, dev)
    for _ in range(6):
        assert te.train()["loss_total"] > 0
    f = te.save_checkpoint(str(tmp_path))
    te2 = _estimator(dev)
    te2.load_checkpoint(f)
    _add_nodes(te2, dev)
    assert te2.step == te.step == 6 and te2._optimizer.step == te._optimizer.step == 6

    def state(e):
        return [e._model.flat_params(), e._optimizer.m, e._optimizer.v]

    for a, b in zip(state(te), state(te2)):
        assert torch.equal(a, b)
    batch = te.make_batch(8)
    te.make_batch = te2.make_batch = lambda bs: batch
    r1, r2 = te.train(), te2.train()
    assert r1 == r2 and te.step == 7
    for a, b in zip(state(te), state(te2)):
        assert torch.equal(a, b)
    te.change_device(str(dev))
    r3 = te.train()
    assert te.step == 8 and np.isfinite(r3["loss_total"]) and te._optimizer.step == 8


# ---- 7: two ranks -------------------------------------------------------------------------------------------------------------------
def _graphs():
    D, S = 12, 20
    out = []
    for i in range(5):
        y, yv = _labels(S, 60 + i)
        out.append(Data(x=2 * torch.randn(S, D, generator=g(50 + i)), edge_index=_random_edges(S, 3, 70 + i), y=y, y_valid=yv))
    return out


def _shard(graphs, dev):
    if not graphs:
        return (torch.zeros(0, 12, device=dev), torch.zeros(2, 0, dtype=torch.long, device=dev), torch.zeros(0, device=dev),
                torch.zeros(0, dtype=torch.bool, device=dev))
    b = Batch.from_data_list(graphs)
    return b.x.to(dev), b.edge_index.to(dev), b.y.to(dev), b.y_valid.to(dev)


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
    graphs = _graphs()
    m, _ = _model(dev, 12, [8, 4, 1])
    tr = GcnTrainer(m, lr=0.05, w_trav=1.0, w_reco=1.0)
    tr.comm_events = []
    traj = []
    for step in range(4):
        if step % 2 == 0:
            mine = graphs[:3] if rank == 0 else graphs[3:]
        else:                  # rank 1's shard is EMPTY: it still takes part in both collectives
            mine = graphs if rank == 0 else []
        traj.append(tr.train_step(*_shard(mine, dev)).cpu().tolist())
    assert len(tr.comm_events) == 8
    te = _estimator(dev)   # world size 2: no refusal
    ok = isinstance(te._optimizer, GcnTrainer)
    torch.cuda.synchronize()
    Dist.barrier()
    q.put((rank, traj, [t.cpu().numpy().copy() for t in (m.flat_params(), tr.m, tr.v)], ok))
    torch.distributed.destroy_process_group()


def _cpu_trajectory(dtype):
    graphs = _graphs()
    b = Batch.from_data_list(graphs)
    x, ei, y, yv = b.x.to(dtype), b.edge_index, b.y.to(dtype), b.y_valid
    ps = {k: v.to(dtype).clone().requires_grad_() for k, v in REF.glorot_state_dict(12, [8, 4, 1], 7).items()}
    opt = torch.optim.Adam(list(ps.values()), lr=0.05)
    traj = []
    for _ in range(4):
        res = TREF.loss64(REF.forward(ps, x, ei, dtype), x, y, yv, 1.0, 1.0, FAC)
        opt.zero_grad()
        res[0].backward()
        opt.step()
        traj.append([r.item() for r in res[:3]])
    return np.array(traj)


@pytest.mark.timeout(400)
def test_two_ranks_match_one_rank(dev):
    """Measured on an MI355X: two ranks against one rank 0.0 (bit for bit); the float32 CPU autograd trajectory deviates from the
    float64 one by 3.8e-07 (total), 2.6e-08 (trav), 2.1e-07 (reco); the one-rank fused step from float64 by 3.8e-07."""
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
    m, _ = _model(dev, 12, [8, 4, 1])
    tr = GcnTrainer(m, lr=0.05, w_trav=1.0, w_reco=1.0)
    one = np.array([tr.train_step(*_shard(_graphs(), dev)).cpu().tolist() for _ in range(4)])[:, :3]
    two = np.array(t0)[:, :3]
    t64, t32 = _cpu_trajectory(torch.float64), _cpu_trajectory(torch.float32)
    dev32 = np.abs(t32 - t64).max(axis=0)
    bound = np.maximum(8 * dev32[None, :], 2.0 ** -16 * np.abs(t64))
    print(f"two ranks vs one: max err {np.abs(two - one).max():.3e}; float32 CPU trajectory deviates by {dev32} from float64; "
          f"one rank vs float64 {np.abs(one - t64).max():.3e}")
    assert (np.abs(two - one) <= bound).all(), (np.abs(two - one), bound)
