"""SHA-256 digests of three seeded training steps, for bit-identity checks of changes that must not reorder any arithmetic in
the fused training paths (csrc/mlp.hip, mlp_train.hip, double_mlp.hip, simple_gcn_train.hip, rnvp_train.hip) or change what
their trainers and the estimator hand them.  One line per output, `<case> <output> <digest>`; run it on two builds (WVN_LIB_PATH
selects another build of the library) or two trees and compare the files.

    python scripts/train_step_digests.py > branch.txt
    WVN_LIB_PATH=/path/to/other/libwvn_hip.so python scripts/train_step_digests.py > other.txt && cmp branch.txt other.txt

Cases: SimpleMLP [256, 32] and DoubleMLP [64, 32] on the four-launch and on the general path, DoubleMLP [48, 16] (general path
only, weight-gradient tiles with M < 32); the four ConfidenceGenerator methods with anomaly_balanced on and off; R = 17, 33, 77 (a
ragged last tile for the row tiles of 32 and of 16, more than one 32-row chunk in the weight gradients) x D = 90, 91 (odd D, 1 + D
no multiple of 32); R = 2048 (the limit of the four-launch steps); a batch compacted with rows_dev.
GcnTrainer: SimpleGCN [8, 4, 1] at D = 12 on 20 nodes with about 3 in-edges each; RnvpTrainer: LinearRnvp D = 90, h = 200 at
R = 17 and 100; the four methods each (GcnTrainer: anomaly_balanced on and off).  TraversabilityEstimator: three train() steps
in each fused mode (and train_on_batch for the MLP), with the ConfidenceGenerator's mean / var / std behind them.
Outputs: the parameters after three steps, the Adam moments, the last gradient buffer, stats, the three steps' losses, the
confidence state, the last confidence (or score) vector.
"""
import hashlib
import itertools
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd import _lib  # noqa: E402
from wild_visual_navigation_amd.cfg import ExperimentParams  # noqa: E402
from wild_visual_navigation_amd.model import DoubleMLP, LinearRnvp, SimpleGCN, SimpleMLP  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import (GcnTrainer, MissionNode, MlpTrainer, RnvpTrainer,  # noqa: E402
                                                                 TraversabilityEstimator)

MODELS = {"simple": lambda D: SimpleMLP(D, [256, 32, 1], True), "double": lambda D: DoubleMLP(D, [64, 32, 1]),
          "double48": lambda D: DoubleMLP(D, [48, 16, 1])}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(dev, model, R, D, fused, method, balanced, compact):
    g = torch.Generator().manual_seed(1000 * R + D)
    x = torch.randn(R, D, generator=g)
    yv = torch.rand(R, generator=g) < 0.3
    yv[:2] = True
    y = yv.float() * (0.5 + 0.5 * torch.rand(R, generator=g))
    rows_dev = None
    if compact:   # the first n rows are real, zero rows behind them (what ops.compact_segment_rows leaves)
        n = R - R // 3
        x[n:] = 0.0
        rows_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    torch.manual_seed(42)
    m = MODELS[model](D).to(dev)
    tr = MlpTrainer(m, fused=fused, method=method, anomaly_balanced=balanced)
    losses = [tr.train_step(x.to(dev), y.to(dev), yv.to(dev), want_confidence=True, rows_dev=rows_dev).clone() for _ in range(3)]
    assert int(tr.sync_word.item()) == 0
    case = f"{model}/R{R}/D{D}/{'fused' if fused else 'general'}/{method}/{'bal' if balanced else 'unbal'}{'/compact' if compact else ''}"
    outs = {"params": m.flat_params(), "grads": tr.grads, "losses": torch.stack(losses), "confidence": tr.last_confidence,
            "stats": tr.stats}
    for k, v in outs.items():
        print(case, k, sha(v), flush=True)
    emit_state(case, tr)


def emit_state(case, tr):
    for k in ("m", "v", "conf_state"):
        print(case, k, sha(getattr(tr, k)), flush=True)


def emit_trainer(case, tr, losses, last):
    outs = {"params": tr.model.flat_params(), "grads": tr.grads, "losses": torch.stack(losses), "last": last, "stats": tr.stats}
    for k, v in outs.items():
        print(case, k, sha(v), flush=True)
    emit_state(case, tr)


def run_gcn(dev, method, balanced):
    N, D = 20, 12
    g = torch.Generator().manual_seed(7)
    x = 2 * torch.randn(N, D, generator=g)
    ei = torch.randint(0, N, (2, 3 * N), generator=g)
    yv = torch.rand(N, generator=g) < 0.5
    yv[:2] = True
    y = yv.float() * (0.5 + 0.5 * torch.rand(N, generator=g))
    torch.manual_seed(42)
    tr = GcnTrainer(SimpleGCN(D, True, [8, 4, 1]).to(dev), method=method, anomaly_balanced=balanced)
    losses = [tr.train_step(x.to(dev), ei.to(dev), y.to(dev), yv.to(dev), want_confidence=True).clone() for _ in range(3)]
    assert int(tr.sync_word.item()) == 0 and int(tr.bad_edges.item()) == 0
    emit_trainer(f"gcn/N{N}/D{D}/{method}/{'bal' if balanced else 'unbal'}", tr, losses, tr.last_confidence)


def run_rnvp(dev, R, method):
    D = 90
    x = torch.randn(R, D, generator=torch.Generator().manual_seed(1000 * R + D))
    torch.manual_seed(42)
    tr = RnvpTrainer(LinearRnvp(D, [200], use_permutation=True).to(dev).train(), method=method)
    losses = [tr.train_step(x.to(dev)).clone() for _ in range(3)]
    emit_trainer(f"rnvp/R{R}/D{D}/{method}", tr, losses, tr.last_score)


def run_estimator(dev, mode, method, on_batch=False):
    """Three steps of the estimator on four mission nodes of 12 half-labelled segments (25 all-labelled ones for the anomaly mode)."""
    p = ExperimentParams()
    D = 12 if mode == "gcn" else 90
    if mode == "gcn":
        p.model.name = "SimpleGCN"
        p.model.simple_gcn_cfg.input_size = D
        p.model.simple_gcn_cfg.hidden_sizes = [8, 4, 1]
    elif mode == "rnvp":
        p.model.name = "LinearRnvp"
        p.model.linear_rnvp_cfg.input_size = D
        p.loss_anomaly.method = method
    else:
        p.model.simple_mlp_cfg.input_size = D
    p.loss.method = method
    te = TraversabilityEstimator(p, device=dev, min_samples_for_training=2, anomaly_detection=mode == "rnvp")
    g = torch.Generator().manual_seed(3)
    S, H = (25, 50) if mode == "rnvp" else (12, 48)
    for i in range(4):
        n = MissionNode(timestamp=float(i))
        n.features = torch.randn(S, D, generator=g).to(dev)
        n.feature_segments = (torch.arange(H * H).reshape(H, H) * S // (H * H)).to(dev)
        if mode == "gcn":
            n.feature_edges = torch.randint(0, S, (2, 3 * S), generator=g).to(dev)
        mask = torch.full((3, H, H), 0.7)
        if mode != "rnvp":
            mask[:, : H // 2] = 0.5 + 0.5 * torch.rand(3, H // 2, H, generator=g)
            mask[:, H // 2:] = float("nan")
        assert te.add_mission_node(n)
        te.update_supervision(n, mask.to(dev))
    random.seed(5)   # make_batch shuffles the nodes
    case = f"estimator/{mode}/{method}{'/train_on_batch' if on_batch else ''}"
    for step in range(3):
        if on_batch:
            b = te.make_batch(8)
            losses = te.train_on_batch(b.x, b.y, b.y_valid)
        else:
            out = te.train()
            print(case, f"step{step}", " ".join(f"{k}={float(out[k]).hex()}" for k in sorted(out)), flush=True)
            losses = te._optimizer.losses
        print(case, f"losses{step}", sha(losses), flush=True)
    tr, cg = te._optimizer, te._traversability_loss._confidence_generator
    outs = {"params": te._model.flat_params(), "grads": tr.grads, "stats": tr.stats, "cg_mean": cg.mean, "cg_var": cg.var, "cg_std": cg.std,
            "last": tr.last_score if mode == "rnvp" else tr.last_confidence, "loss": torch.tensor(te.loss)}
    for k, v in outs.items():
        if v is not None:
            print(case, k, sha(v), flush=True)
    emit_state(case, tr)
    print(case, "steps", te.step, tr.step, flush=True)


def main():
    dev = torch.device("cuda:0")
    shapes = list(itertools.product((17, 33, 77), (90, 91)))
    for model in MODELS:
        paths = (False,) if model == "double48" else (True, False)
        for (R, D), fused in itertools.product(shapes, paths):
            for method, balanced in itertools.product(_lib.CONF_METHODS, (True, False)):
                run(dev, model, R, D, fused, method, balanced, False)
            for method in ("latest_measurement", "moving_average"):
                run(dev, model, R, D, fused, method, True, True)
        if model != "double48":
            for fused, method in itertools.product(paths, _lib.CONF_METHODS):
                run(dev, model, 2048, 90, fused, method, True, False)
    for method, balanced in itertools.product(_lib.CONF_METHODS, (True, False)):
        run_gcn(dev, method, balanced)
    for R, method in itertools.product((17, 100), _lib.CONF_METHODS):
        run_rnvp(dev, R, method)
    for mode in ("mlp", "gcn", "rnvp"):
        for method in _lib.CONF_METHODS:
            run_estimator(dev, mode, method)
    run_estimator(dev, "mlp", "latest_measurement", on_batch=True)
    run_estimator(dev, "mlp", "moving_average", on_batch=True)


if __name__ == "__main__":
    main()
