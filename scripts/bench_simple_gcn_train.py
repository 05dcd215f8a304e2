"""SimpleGCN training: the fused HIP step (GcnTrainer: csrc/simple_gcn_train.hip) beside the autograd step it replaces on a GPU
device (SimpleGCN's torch statement -> TraversabilityLoss -> backward -> torch.optim.Adam), in one process, on the same batch:
8 graphs x 100 nodes with 4800 edges, hidden [256, 128, 1], at D = 384 and at D = 90, seeded weights.

Each step is timed on the host clock and ends in the one host read the estimator makes (the losses); the two paths alternate step
by step after a warm-up, so both see the same machine.  Reported: median, the 10th / 90th percentile as the spread, the ratio of
the medians, the GPU kernels one step launches and the fused step's five longest kernels (torch.profiler; "not measured" where the
profiler is unavailable).

One JSON line; --markdown FILE also writes the table of profiles/simple_gcn_train.md.

    python scripts/bench_simple_gcn_train.py [--steps 60] [--warmup 10] [--markdown FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd.model import SimpleGCN  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import GcnTrainer  # noqa: E402
from wild_visual_navigation_amd.utils import Batch, Data, TraversabilityLoss  # noqa: E402

HIDDEN = [256, 128, 1]


def kernels_per_step(step):
    """-> (kernel launches of one step, its five longest kernels as (name, microseconds))."""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
              and "memset" not in e.name.lower()]
        if not ev:
            return "not measured", []

        def us(e):
            return getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)

        def short(name):   # "void (anonymous namespace)::gcn_back_kernel(...)" -> "gcn_back_kernel"
            name = name.replace("(anonymous namespace)::", "").replace("void ", "")
            return name.split("(")[0].split("<")[0][-60:]

        top = sorted(ev, key=lambda e: -us(e))[:5]
        return len(ev), [(short(e.name), round(us(e), 1)) for e in top]
    except Exception:  # noqa: BLE001
        return "not measured", []


def case(D, steps, warmup, dev):
    g = torch.Generator().manual_seed(D)
    graphs = []
    for _ in range(8):
        yv = torch.rand(100, generator=g) < 0.5
        graphs.append(Data(x=2 * torch.randn(100, D, generator=g), edge_index=torch.randint(0, 100, (2, 600), generator=g),
                           y=yv.float() * (0.5 + 0.5 * torch.rand(100, generator=g)), y_valid=yv))
    b = Batch.from_data_list(graphs)
    x, ei, y, yv = b.x.to(dev), b.edge_index.to(dev), b.y.to(dev), b.y_valid.to(dev)
    torch.manual_seed(D)
    fused_model = SimpleGCN(D, True, HIDDEN).to(dev).train()
    auto_model = SimpleGCN(D, True, HIDDEN).to(dev).train()
    auto_model.load_state_dict(fused_model.state_dict())
    tr = GcnTrainer(fused_model, lr=1e-3)
    loss_fn = TraversabilityLoss(w_trav=0.03, w_reco=0.5, w_temp=0.0, anomaly_balanced=True, model=auto_model,
                                 method="latest_measurement", confidence_std_factor=0.5).to(dev)
    opt = torch.optim.Adam(auto_model.parameters(), lr=1e-3)
    graph = Data(x=x, edge_index=ei, y=y, y_valid=yv)

    def fused():
        return tr.train_step(x, ei, y, yv).tolist()[0]

    def autograd():
        loss, aux, _ = loss_fn(graph, auto_model.forward_torch(x, ei))
        opt.zero_grad()
        loss.backward()
        opt.step()
        return torch.stack([loss.detach().reshape(()), aux["loss_trav"].detach(), aux["loss_reco"].detach()]).tolist()[0]

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
    out = {"D": D, "hidden": HIDDEN, "nodes": 800, "edges": int(ei.shape[1]), "steps": steps, "first_loss": first,
           "last_loss": (last["fused"], last["autograd"])}
    for name, t in times.items():
        q = statistics.quantiles(t, n=10)
        out[name] = {"median_ms": statistics.median(t), "p10_ms": q[0], "p90_ms": q[-1]}
    out["ratio_autograd_over_fused"] = out["autograd"]["median_ms"] / out["fused"]["median_ms"]
    nf, top = kernels_per_step(fused)
    out["kernels_per_step"] = {"fused": nf, "autograd": kernels_per_step(autograd)[0]}
    out["fused_longest_kernels_us"] = top
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simple_gcn_train.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    res = [case(D, args.steps, args.warmup, dev) for D in (384, 90)]
    print(json.dumps({"bench": "simple_gcn_train", "device": torch.cuda.get_device_name(0), "cases": res}))
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("| D | hidden | nodes | edges | fused step, median [p10, p90] ms | autograd step, median [p10, p90] ms | autograd / fused | "
                    "kernels per step, fused | autograd |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in res:
                a, b = r["fused"], r["autograd"]
                f.write(f"| {r['D']} | {r['hidden']} | {r['nodes']} | {r['edges']} | {a['median_ms']:.3f} [{a['p10_ms']:.3f}, {a['p90_ms']:.3f}] | "
                        f"{b['median_ms']:.3f} [{b['p10_ms']:.3f}, {b['p90_ms']:.3f}] | {r['ratio_autograd_over_fused']:.2f} | "
                        f"{r['kernels_per_step']['fused']} | {r['kernels_per_step']['autograd']} |\n")
            f.write("\nThe fused step's five longest kernels (microseconds):\n\n")
            for r in res:
                f.write(f"- D = {r['D']}: " + "; ".join(f"`{n}` {t}" for n, t in r["fused_longest_kernels_us"]) + "\n")


if __name__ == "__main__":
    main()
