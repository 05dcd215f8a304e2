"""One image-space metric update (MetricLogger.log_image + log_confidence as one call: four pairs {traversability, confidence} x
{hand labels, self labels}) on 64 frames of 448 x 448 with 100 segments per frame and T = 5000 thresholds, two ways, one JSON line:

    fused   ops.metric_accumulate (csrc/metrics.hip): one launch, scores and self labels gathered through seg on load
    torch   the same definition as torch operations on the same GPU: gather, bucketize, bincount per pair, comparisons for the
            confusion matrices and counters (what a binned torchmetrics update does, without its host checks)

in three cases: "segments" (per-segment scores and self labels, hand labels a uint8 map, int32 segment ids: what log_image feeds),
"segments_i64" (the same with int64 segment ids, as the reference's graphs carry them: the kernel reads them as they are) and "dense" (both scores
fp32 maps of independent random values, both label maps uint8: what log_maps feeds after predict_per_pixel; every pixel its own bin, the
case the wave pre-aggregation cannot help).  Both routes stay on the device; they are timed between HIP events over ``iters`` calls after
``warmup``, alternating in ``rounds`` rounds (the median round is reported, the spread beside it).  The states of the two routes are
compared before anything is timed.  ``fused_GBps`` = the pass's compulsory traffic (every input map read once: 5 bytes per pixel for
"segments" = seg + hand labels, 9 with int64 ids, 14 for "dense" = seg + 2 scores + 2 labels; tables and states are negligible) over the fused time.
``curve_ms`` / ``exact_auroc_ms``: wvn_metric_curve on one pair state, ops.metric_auroc_weighted (with its sort) on the batch's
6400 entries; ``exact_auroc_max_ms``: the same call at the interface's limit of 2^24 entries, ``sort_max_ms`` its torch.sort alone.

    python scripts/bench_metrics.py [--iters N] [--warmup N] [--rounds N]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from wild_visual_navigation_amd import ops  # noqa: E402
from wild_visual_navigation_amd.ops import PerSegment  # noqa: E402

B, H, W, S, T = 64, 448, 448, 100, 5000


def timed_events(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def segment_maps(g):
    """Superpixel-like maps: a 10 x 10 grid of cells whose borders wander by a few pixels per row / column."""
    ys = torch.arange(H).view(1, H, 1) + torch.randint(-6, 7, (B, 1, W), generator=g)
    xs = torch.arange(W).view(1, 1, W) + torch.randint(-6, 7, (B, H, 1), generator=g)
    cy = (ys.clamp(0, H - 1) * 10 // H).clamp(0, 9)
    cx = (xs.clamp(0, W - 1) * 10 // W).clamp(0, 9)
    return (cy * 10 + cx).to(torch.int32)


def torch_update(state, th, scores, targets, tau):
    """The definition as torch ops on dense [N] sources (already gathered): adds into state [len(scores) * len(targets)][words]."""
    nb = 2 * (T + 1)
    for i, p in enumerate(scores):
        nan = torch.isnan(p)
        k = torch.bucketize(p, th, right=True)
        pred = (p > tau).to(torch.int64)
        oor = (p < 0) | (p > 1)
        for j, c in enumerate(targets):
            st = state[i * len(targets) + j]
            use = (c < 2) & ~nan
            cu = c[use].to(torch.int64)
            st[:nb] += torch.bincount(k[use] * 2 + cu, minlength=nb)
            st[nb:nb + 4] += torch.bincount(cu * 2 + pred[use], minlength=4)
            st[nb + 4] += (nan & (c < 2)).sum()
            st[nb + 5] += (c == 2).sum()
            st[nb + 6] += (oor & use).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    seg = segment_maps(g).to(dev)
    trav = torch.rand(B, S, generator=g).to(dev)
    conf = torch.rand(B, S, generator=g).to(dev)
    y = (torch.rand(B, S, generator=g) < 0.5).float().to(dev)
    label = (torch.rand(B, 1, 1, generator=g) * 0.6 + 0.2 > torch.rand(B, H, W, generator=g)).to(torch.uint8).to(dev)
    th = torch.linspace(0, 1, T, dtype=torch.float32).to(dev)   # made on the CPU, uploaded
    rows = (torch.arange(B, device=dev).view(B, 1, 1) * S + seg.long()).reshape(-1)
    npix = B * H * W
    cases = []
    seg32 = seg
    for name in ("segments", "segments_i64", "dense"):
        seg = seg32.long() if name == "segments_i64" else seg32
        if name != "dense":
            scores, targets, bytes_pp = [PerSegment(trav), PerSegment(conf)], [label, PerSegment(y)], 5 if name == "segments" else 9

            def torch_route(state):
                sc = [trav.reshape(-1)[rows], conf.reshape(-1)[rows]]                      # the projected maps torchmetrics is fed
                tg = [label.reshape(-1), y.reshape(-1)[rows].to(torch.uint8)]
                torch_update(state, th, sc, tg, 0.5)
        else:
            dt = torch.rand(B, H, W, generator=g).to(dev)
            dc = torch.rand(B, H, W, generator=g).to(dev)
            dy = y.reshape(-1)[rows].view(B, H, W).to(torch.uint8)
            scores, targets, bytes_pp = [dt, dc], [label, dy], 14

            def torch_route(state, dt=dt, dc=dc, dy=dy):
                torch_update(state, th, [dt.reshape(-1), dc.reshape(-1)], [label.reshape(-1), dy.reshape(-1)], 0.5)

        cnt = torch.zeros(B * S, 2, 2, dtype=torch.int32, device=dev)

        def fused_route(state, scores=scores, targets=targets, seg=seg):
            ops.metric_accumulate(state, th, scores, targets, seg=seg, tau=0.5, seg_counts=cnt)

        s1, s2 = ops.metric_state(4, T, dev), ops.metric_state(4, T, dev)
        fused_route(s1)
        torch_route(s2)
        assert torch.equal(s1, s2), "the fused pass and the torch statement disagree"
        fused, ref = [], []
        for _ in range(a.rounds):
            fused.append(timed_events(lambda: fused_route(s1), a.warmup, a.iters))
            ref.append(timed_events(lambda: torch_route(s2), a.warmup, max(2, a.iters // 4)))
        fm, rm = statistics.median(fused), statistics.median(ref)
        cases.append({"case": name, "pixels": npix, "pairs": 4, "T": T, "fused_ms": round(fm, 4), "fused_ms_min_max": [round(min(fused), 4), round(max(fused), 4)],
                      "torch_ms": round(rm, 3), "torch_ms_min_max": [round(min(ref), 3), round(max(ref), 3)], "torch_over_fused": round(rm / fm, 1),
                      "compulsory_bytes": bytes_pp * npix, "fused_GBps": round(bytes_pp * npix / fm / 1e6, 1)})
    seg = seg32
    state = ops.metric_state(4, T, dev)
    cnt = torch.zeros(B * S, 2, 2, dtype=torch.int32, device=dev)
    ops.metric_accumulate(state, th, [PerSegment(trav), PerSegment(conf)], [label, PerSegment(y)], seg=seg, seg_counts=cnt)
    curve_ms = timed_events(lambda: ops.metric_curve(state[0], th), a.warmup, a.iters)
    pos, neg = cnt[:, 0, 1].contiguous(), cnt[:, 0, 0].contiguous()
    exact_ms = timed_events(lambda: ops.metric_auroc_weighted(trav.reshape(-1), pos, neg), a.warmup, a.iters)
    E = 1 << 24
    big = (torch.rand(E, generator=g) * 4096).round().div(4096).to(dev)   # ties
    bp = torch.randint(0, 50, (E,), generator=g).to(dev)
    bn = torch.randint(0, 50, (E,), generator=g).to(dev)
    exact_max_ms = timed_events(lambda: ops.metric_auroc_weighted(big, bp, bn), 1, 3)
    sort_max_ms = timed_events(lambda: torch.sort(big, descending=True), 1, 3)
    print(json.dumps({"bench": "metrics", "device": torch.cuda.get_device_name(0), "frames": B, "frame": f"{H}x{W}", "segments": S,
                      "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds, "cases": cases, "curve_ms": round(curve_ms, 4),
                      "exact_auroc_entries": B * S, "exact_auroc_ms": round(exact_ms, 4),
                      "exact_auroc_max_entries": E, "exact_auroc_max_ms": round(exact_max_ms, 3), "sort_max_ms": round(sort_max_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
