"""Two-rank data-parallel training steps with the moving_average and running_mean confidence methods (backend "gloo" with
CUDA tensors, both ranks on cuda:0, as tests/test_gpu_distributed.py does), on ragged and EMPTY shards.  The statistic's
memory is committed by phase C on every rank alike, and moving_average adds one MAX collective of {max, -min}.  Pass
criteria: the 2-rank trajectory equals the reference's single-process trajectory on the concatenated batch
(tests/golden/mlp_train_methods.pt), and the replicas -- losses, parameters, device state -- stay bit-identical."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, case, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from wild_visual_navigation_amd import distributed as D
    from wild_visual_navigation_amd.model import SimpleMLP
    from wild_visual_navigation_amd.traversability_estimator import MlpTrainer

    D.init_from_env(backend="gloo")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    golden = os.path.join(ROOT, "tests", "golden")
    src = torch.load(os.path.join(golden, "mlp_train.pt"), weights_only=False)["graph_pt_D90"]
    c = torch.load(os.path.join(golden, "mlp_train_methods.pt"), weights_only=False)["cases"][case]
    model = SimpleMLP(90, [256, 32, 1], True)
    model.load_state_dict(src["sd0"])
    model.to(dev)
    tr = MlpTrainer(model, method=c["method"], anomaly_balanced=c["balanced"])
    traj = []
    for step, rows in enumerate(c["rows"]):
        if step % 3 == 2:      # rank 1's shard is EMPTY: it still takes part in every collective
            lo, hi = (0, len(rows)) if rank == 0 else (len(rows), len(rows))
        else:                  # ragged halves
            lo, hi = D.shard_range(len(rows), rank, world)
        r = rows[lo:hi]
        losses = tr.train_step(src["x"][r].to(dev), src["y"][r].to(dev), src["y_valid"][r].to(dev))
        lo_ = losses.cpu().tolist()
        traj.append(lo_[:4] + [tr.conf_state[1].item(), lo_[4]])
    torch.cuda.synchronize()
    D.barrier()
    q.put((rank, traj, {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()},
           tr.conf_state.cpu().numpy().copy()))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(400)
@pytest.mark.parametrize("case", ["moving_average_balanced", "running_mean_unbalanced"])
def test_two_ranks_gloo_on_one_gpu(dev, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, case, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=280) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, t0, sd0, cs0), (_, t1, sd1, cs1) = res
    assert t0 == t1, "ranks disagree on the losses"
    assert (cs0 == cs1).all(), "ranks disagree on the confidence state"
    for k in sd0:
        assert (sd0[k] == sd1[k]).all(), f"replicas diverged on {k}"
    c = torch.load(os.path.join(ROOT, "tests", "golden", "mlp_train_methods.pt"), weights_only=False)["cases"][case]
    got = torch.tensor(t0)
    assert torch.allclose(got, c["traj"], rtol=3e-4, atol=2e-6), (got - c["traj"]).abs().max()
    for k in sd0:
        assert torch.allclose(torch.from_numpy(sd0[k]), c["sd12"][k], atol=3e-5), k
