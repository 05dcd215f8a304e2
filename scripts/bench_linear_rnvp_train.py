"""Anomaly-detection training: the fused HIP step (RnvpTrainer: csrc/rnvp_train.hip) beside the autograd step it replaces on a GPU
device (LinearRnvp's torch statement -> AnomalyLoss -> backward -> torch.optim.Adam), in one process, on the same rows: 8 x 100
segment rows at D = 384, h = 200 and at D = 90, seeded weights.

Each step is timed on the host clock and ends in the one host read the estimator makes (the loss); the two paths alternate step
by step after a warm-up, so both see the same machine.  Reported: median, the 10th / 90th percentile as the spread, the ratio of
the medians, and the GPU kernels one step launches (torch.profiler; "not measured" where the profiler is unavailable).

One JSON line; --markdown FILE also writes the table of profiles/anomaly_training.md.

    python scripts/bench_linear_rnvp_train.py [--steps 60] [--warmup 10] [--markdown FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd.model import LinearRnvp  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import RnvpTrainer  # noqa: E402
from wild_visual_navigation_amd.utils import AnomalyLoss, Data  # noqa: E402


def kernels_per_step(step):
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n if n > 0 else "not measured"
    except Exception:  # noqa: BLE001
        return "not measured"


def case(D, h, steps, warmup, dev):
    g = torch.Generator().manual_seed(D)
    x = torch.randn(800, D, generator=g).to(dev)
    torch.manual_seed(D)
    fused_model = LinearRnvp(D, [h], use_permutation=True).to(dev).train()
    auto_model = LinearRnvp(D, [h], use_permutation=True).to(dev).train()
    auto_model.load_state_dict(fused_model.state_dict())
    tr = RnvpTrainer(fused_model, lr=1e-3)
    loss_fn = AnomalyLoss(0.5, "latest_measurement").to(dev)
    opt = torch.optim.Adam(auto_model.parameters(), lr=1e-3)

    def fused():
        return tr.train_step(x)[0].item()

    def autograd():
        loss, _, _ = loss_fn(None, auto_model(Data(x=x)))
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.item()

    first = (fused(), autograd())
    for _ in range(warmup):
        fused()
        autograd()
    times = {"fused": [], "autograd": []}
    last = {}
    for _ in range(steps):
        for name, fn in (("fused", fused), ("autograd", autograd)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"D": D, "h": h, "rows": 800, "steps": steps, "first_loss": first, "last_loss": (last["fused"], last["autograd"])}
    for name, t in times.items():
        q = statistics.quantiles(t, n=10)
        out[name] = {"median_ms": statistics.median(t), "p10_ms": q[0], "p90_ms": q[-1]}
    out["ratio_autograd_over_fused"] = out["autograd"]["median_ms"] / out["fused"]["median_ms"]
    out["kernels_per_step"] = {"fused": kernels_per_step(fused), "autograd": kernels_per_step(autograd)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_rnvp_train.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    res = [case(D, 200, args.steps, args.warmup, dev) for D in (384, 90)]
    print(json.dumps({"bench": "linear_rnvp_train", "device": torch.cuda.get_device_name(0), "cases": res}))
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("| D | h | rows | fused step, median [p10, p90] ms | autograd step, median [p10, p90] ms | autograd / fused | "
                    "kernels per step, fused | autograd |\n|---|---|---|---|---|---|---|---|\n")
            for r in res:
                a, b = r["fused"], r["autograd"]
                f.write(f"| {r['D']} | {r['h']} | {r['rows']} | {a['median_ms']:.3f} [{a['p10_ms']:.3f}, {a['p90_ms']:.3f}] | "
                        f"{b['median_ms']:.3f} [{b['p10_ms']:.3f}, {b['p90_ms']:.3f}] | {r['ratio_autograd_over_fused']:.2f} | "
                        f"{r['kernels_per_step']['fused']} | {r['kernels_per_step']['autograd']} |\n")


if __name__ == "__main__":
    main()
