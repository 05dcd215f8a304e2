"""Per-step time of MlpTrainer.train_step for DoubleMLP(384, [64, 32, 1]) beside the fused SimpleMLP(384, [256, 32, 1]) step at the
same row counts (default R = 800 and R = 2048: both take their four-launch steps).  One JSON line per (model, R): ms per step from
CUDA events around `--steps` back-to-back steps, median of `--repeats` such blocks.

    python scripts/bench_double_mlp.py [--rows 800,2048] [--steps 200] [--general]

Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_double_mlp.py --steps 20` the kernel counts divided by the steps
run (warm-up included: `steps_run` in the output) give the launches per step.  --general times the general paths (fused=False).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd.model import DoubleMLP, SimpleMLP  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import MlpTrainer  # noqa: E402


def batch(R, D, dev):
    g = torch.Generator().manual_seed(R)
    yv = torch.rand(R, generator=g) < 0.2
    return (torch.randn(R, D, generator=g).to(dev), (yv.float() * (0.5 + 0.5 * torch.rand(R, generator=g))).to(dev), yv.to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="800,2048")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--D", type=int, default=384)
    ap.add_argument("--general", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    models = (("DoubleMLP", lambda: DoubleMLP(a.D, [64, 32, 1])), ("SimpleMLP", lambda: SimpleMLP(a.D, [256, 32, 1], True)))
    for R in (int(r) for r in a.rows.split(",")):
        x, y, yv = batch(R, a.D, dev)
        for name, make in models:
            torch.manual_seed(42)
            tr = MlpTrainer(make().to(dev), fused=not a.general)
            for _ in range(a.warmup):
                tr.train_step(x, y, yv)
            torch.cuda.synchronize()
            times = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    tr.train_step(x, y, yv)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) / a.steps)
            print(json.dumps({"model": name, "R": R, "D": a.D, "fused": not a.general, "steps": a.steps, "repeats": a.repeats,
                              "steps_run": a.warmup + a.steps * a.repeats, "ms_per_step": round(statistics.median(times), 4),
                              "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
                              "loss_finite": bool(torch.isfinite(tr.losses).all())}), flush=True)


if __name__ == "__main__":
    main()
