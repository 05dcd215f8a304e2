"""SimpleGCN(384, hidden [256, 128, 1]) on the HIP graph kernels beside the same plain-torch statement (``index_add_``) on the same
GPU, at the two sizes the model runs at:

  train : a training-size batch, 8 graphs x 100 nodes, random directed edges with mean in-degree 6 per graph --
          ``model(Data)`` in eval mode (graph preparation from the edge list + three layer launches) against
          ``model.forward_torch`` under no_grad.
  live  : a live batch, B = 16 frames of S = 196 grid segments on 224 x 224 maps -- ``forward_per_segment(feat, seg,
          adjacency=...)`` (graph preparation from the bitmaps + three layer launches + paint) against the torch statement
          followed by column 0 / reconstruction confidence / ``table[seg]``.  The bitmaps (``ops.seg_adjacency_batched``) and
          the torch side's edge list are built outside the timed region.

One JSON line per case: ms per call from CUDA events around ``--steps`` back-to-back calls, median of ``--repeats`` such blocks.

    python scripts/bench_simple_gcn.py [--steps 200] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd import ops  # noqa: E402
from wild_visual_navigation_amd.model import SimpleGCN  # noqa: E402
from wild_visual_navigation_amd.utils import Data  # noqa: E402


def timed(fn, steps, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / steps)
    return {"ms_per_call": round(statistics.median(times), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--D", type=int, default=384)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    model = SimpleGCN(a.D, True, [256, 128, 1]).to(dev).eval()
    g = torch.Generator().manual_seed(0)
    mean, std, fac = 1.0, 0.5, 0.5

    # ---- train: 8 graphs x 100 nodes ----
    graphs, n = 8, 100
    x = torch.randn(graphs * n, a.D, generator=g).to(dev)
    ei = torch.cat([torch.randint(0, n, (2, 6 * n), generator=g) + k * n for k in range(graphs)], dim=1).to(dev)
    data = Data(x=x, edge_index=ei)
    with torch.no_grad():
        err = (model(data) - model.forward_torch(x, ei)).abs().max().item()
        for name, fn in (("hip", lambda: model(data)), ("torch", lambda: model.forward_torch(x, ei))):
            print(json.dumps({"case": "train", "path": name, "nodes": graphs * n, "edges": ei.shape[1], "D": a.D, "steps": a.steps,
                              "repeats": a.repeats, "max_abs_diff_hip_torch": err, **timed(fn, a.steps, a.warmup, a.repeats)}), flush=True)

    # ---- live: B = 16, S = 196 ----
    B, H, cell = 16, 224, 16
    S = (H // cell) ** 2
    ids = torch.arange(H) // cell
    seg = (ids[:, None] * (H // cell) + ids[None, :]).to(torch.int32)[None].expand(B, H, H).contiguous().to(dev)
    feat = torch.randn(B, S, a.D, generator=g).to(dev)
    adj = ops.seg_adjacency_batched(seg, S)
    nz = adj.nonzero()                                              # (b, l, r)
    ei_live = torch.stack([nz[:, 0] * S + nz[:, 1], nz[:, 0] * S + nz[:, 2]])
    flat, seg_flat = feat.reshape(B * S, a.D), (seg.long() + (torch.arange(B, device=dev) * S)[:, None, None])

    def live_torch():
        out = model.forward_torch(flat, ei_live)
        loss = ((out[:, 1:] - flat) ** 2).mean(1)
        lo, hi = max(mean + std * fac - std, 0.0), mean + std * fac + std
        conf = 1 - (loss.clamp(lo, hi) - lo) / (hi - lo)
        return out[:, 0][seg_flat], conf[seg_flat]

    def live_hip():
        return model.forward_per_segment(feat, seg, mean, std, fac, adjacency=adj)

    with torch.no_grad():
        th, ch, _ = live_hip()
        tt, ct = live_torch()
        err = max((th - tt).abs().max().item(), (ch - ct).abs().max().item())
        for name, fn in (("hip", live_hip), ("torch", live_torch)):
            print(json.dumps({"case": "live", "path": name, "B": B, "S": S, "edges": ei_live.shape[1], "D": a.D, "map": [H, H],
                              "steps": a.steps, "repeats": a.repeats, "max_abs_diff_hip_torch": err,
                              **timed(fn, a.steps, a.warmup, a.repeats)}), flush=True)


if __name__ == "__main__":
    main()
