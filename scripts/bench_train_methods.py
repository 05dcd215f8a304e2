"""Per-step time of MlpTrainer.train_step for every ConfidenceGenerator method (anomaly_balanced = True) at several row counts,
D = 384.  R <= 2048 runs the four-launch step (csrc/mlp_train.hip), larger R the general path.  "latest_measurement" is the
original step (its original entry points); the other methods go through the *_conf entry points.  One JSON line per (R, method),
time in ms per step from CUDA events around `--iters` back-to-back steps.

    python scripts/bench_train_methods.py [--rows 100,2048,12544] [--iters 200]

With --trace-steps N it instead runs N steps per (R, method) with a device synchronisation between the blocks, in the order
rows x methods -- the shape of run to put under `rocprofv3 --kernel-trace --stats` to see which kernels each method launches:

    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python scripts/bench_train_methods.py --rows 100,12544 --trace-steps 5
    python scripts/bench_train_methods.py --summarize OUT/trace_results.db --rows 100,12544 --trace-steps 5

--summarize prints, per (R, method), the kernels of one traced step (the sequence up to and including Adam) as a markdown table.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd.model import SimpleMLP  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import MlpTrainer  # noqa: E402

METHODS = ("latest_measurement", "running_mean", "kalman_filter", "moving_average")


def batch(R, D, dev):
    g = torch.Generator().manual_seed(R)
    yv = torch.rand(R, generator=g) < 0.2
    return (torch.randn(R, D, generator=g).to(dev), (yv.float() * (0.5 + 0.5 * torch.rand(R, generator=g))).to(dev), yv.to(dev))


def summarize(db, rows, steps):
    import re
    import sqlite3

    names = [n for (n,) in sqlite3.connect(db).execute("select name from kernels order by start")]
    short = [re.sub(r"\(anonymous namespace\)::", "", n).replace("void ", "").split("(")[0].split("<")[0] for n in names]
    # the MLP step's kernels: everything from the first training kernel of a step up to Adam (torch's set-up fills and copies
    # at trainer construction fall outside)
    seqs, cur = [], None
    for k in short:
        if cur is None and k in ("mlp_train_fwd_kernel", "gemm_f32_kernel"):
            cur = []
        if cur is not None:
            cur.append(k)
            if k == "adam_kernel":
                seqs.append(cur)
                cur = None
    blocks = [(R, m) for R in rows for m in METHODS]
    assert len(seqs) == len(blocks) * steps, (len(seqs), len(blocks), steps)
    print("| R | method | launches per step | kernels of one step (in order) | all traced steps identical |")
    print("|---|---|---|---|---|")
    for i, (R, m) in enumerate(blocks):
        block = seqs[i * steps:(i + 1) * steps]
        print(f"| {R} | {m} | {len(block[0])} | {' '.join(block[0])} | {all(b == block[0] for b in block)} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100,2048,12544")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--D", type=int, default=384)
    ap.add_argument("--summarize", default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, [int(r) for r in a.rows.split(",")], a.trace_steps)
    dev = torch.device("cuda:0")
    for R in (int(r) for r in a.rows.split(",")):
        x, y, yv = batch(R, a.D, dev)
        for method in METHODS:
            torch.manual_seed(42)
            tr = MlpTrainer(SimpleMLP(a.D, [256, 32, 1], True).to(dev), method=method)
            if a.trace_steps:
                for _ in range(a.trace_steps):
                    tr.train_step(x, y, yv)
                torch.cuda.synchronize()
                print(json.dumps({"R": R, "method": method, "traced_steps": a.trace_steps}), flush=True)
                continue
            for _ in range(10):
                tr.train_step(x, y, yv)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                tr.train_step(x, y, yv)
            e1.record()
            torch.cuda.synchronize()
            print(json.dumps({"R": R, "D": a.D, "method": method, "fused": R <= 2048, "iters": a.iters,
                              "ms_per_step": round(e0.elapsed_time(e1) / a.iters, 4),
                              "loss_finite": bool(torch.isfinite(tr.losses).all())}), flush=True)


if __name__ == "__main__":
    main()
