"""SHA-256 digests of three seeded training steps, for bit-identity checks of changes that must not reorder any arithmetic in
the MLP training path (csrc/mlp.hip, mlp_train.hip, double_mlp.hip).  One line per output, `<case> <output> <digest>`; run it on
two builds (WVN_LIB_PATH selects another build of the library) and compare the files.

    python scripts/train_step_digests.py > branch.txt
    WVN_LIB_PATH=/path/to/other/libwvn_hip.so python scripts/train_step_digests.py > other.txt && cmp branch.txt other.txt

Cases: SimpleMLP [256, 32] and DoubleMLP [64, 32] on the four-launch and on the general path, DoubleMLP [48, 16] (general path
only, weight-gradient tiles with M < 32); the four ConfidenceGenerator methods with anomaly_balanced on and off; R = 17, 33, 77 (a
ragged last tile for the row tiles of 32 and of 16, more than one 32-row chunk in the weight gradients) x D = 90, 91 (odd D, 1 + D
no multiple of 32); R = 2048 (the limit of the four-launch steps); a batch compacted with rows_dev.
Outputs: the parameters after three steps, the last gradient buffer, the three steps' losses, the last confidence vector, stats.
"""
import hashlib
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd import _lib  # noqa: E402
from wild_visual_navigation_amd.model import DoubleMLP, SimpleMLP  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import MlpTrainer  # noqa: E402

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


if __name__ == "__main__":
    main()
