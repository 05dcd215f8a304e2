"""The graph and flow views (csrc/draw.hip through LearningVisualizer) against the PIL.ImageDraw loops they replace, one JSON line:

    graph   plot_traversability_graph on a 448 x 448 frame, 100 nodes, 600 edges: the device route (list assembled with torch
            operations, one draw launch, the finished uint8 picture copied to the host) against the PIL route of the reference
            (download the frame, one ImageDraw call per edge and node), restated below; device time of the draw launch alone
    flow    plot_optical_flow at 448 x 448, s = 10 (1936 lines) against the reference's PIL loop
    batch   plot_traversability_graph on 16 frames in one call against 16 single-frame calls and 16 runs of the PIL route

Every pair is compared for equality before it is timed.  Needs PIL (for the routes it is measured against).

    python scripts/bench_draw.py [--iters N] [--warmup N] [--host-iters N]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from wild_visual_navigation_amd import ops  # noqa: E402
from wild_visual_navigation_amd.visu import LearningVisualizer, colour_table  # noqa: E402


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


def timed_wall(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def pil_graph(prediction, graph, center, img, table):
    """plot_traversability_graph as it was: the frame as 8 bits on the device, downloaded, then PIL per edge and node."""
    from PIL import Image, ImageDraw

    prediction = prediction.detach().cpu()
    index = (prediction.float() * 255).to(torch.uint8)
    pil = Image.fromarray(ops.image_to_u8(img, unit_range=True)[0].cpu().numpy())
    draw = ImageDraw.Draw(pil)
    edges, center = graph.edge_index.cpu(), center.cpu()
    valid = graph.y_valid.cpu().tolist()
    for i in range(edges.shape[1]):
        a, b = int(edges[0, i]), int(edges[1, i])
        draw.line(center[a].tolist() + center[b].tolist(), fill=(127, 127, 127))
    for i in range(center.shape[0]):
        c = center[i].tolist()
        box = [p - 5 for p in c] + [p + 5 for p in c]
        if valid[i]:
            draw.ellipse(box, width=10, fill=tuple(table[int(index[i])].tolist()))
        else:
            draw.ellipse(box, width=1, fill=(127, 127, 127))
    return np.array(pil)


def pil_flow(flow, img1, img2, s):
    """plot_optical_flow of the reference (visualizer.py:552-570) on host tensors."""
    from PIL import Image, ImageDraw

    i1, i2 = np.uint8((img1.permute(1, 2, 0) * 255).numpy()), np.uint8((img2.permute(1, 2, 0) * 255).numpy())
    pil = Image.fromarray(np.concatenate([i1, i2], axis=1))
    draw = ImageDraw.Draw(pil)
    for u in range(int(flow.shape[1] / s)):
        u = int(u * s)
        for v in range(int(flow.shape[2] / s)):
            v = int(v * s)
            du = (flow[0, u, v]).item()
            dv = (flow[1, u, v] + i2.shape[1]).item()
            draw.line([(v, u), (v + dv, u + du)], fill=(0, 255, 0), width=2)
    return np.array(pil).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    S, N, E, B = 448, 100, 600, 16
    vis = LearningVisualizer()
    table = colour_table("RdYlBu", 256)
    imgs = torch.rand(B, 3, S, S, generator=g).to(dev)
    centers = (torch.rand(B, N, 2, generator=g) * (S - 1)).to(dev)
    preds = torch.rand(B, N, generator=g).to(dev)
    graph = types.SimpleNamespace(edge_index=torch.randint(0, N, (2, E), generator=g).to(dev), y_valid=(torch.rand(N, generator=g) > 0.2).to(dev))
    out = {}

    # ---- graph view, one frame ----
    img, center, pred = imgs[0], centers[0], preds[0]
    want = pil_graph(pred, graph, center, img, table)
    assert np.array_equal(vis.plot_traversability_graph(pred, graph, center, img), want)
    lists = vis._traversability_graph_list(pred, graph, center, 1.0, "RdYlBu", False, 1)
    canvas = ops.image_to_u8(img, unit_range=True)
    out["graph"] = {
        "primitives": int(lists[0].shape[0]),
        "device_route_ms": timed_wall(lambda: vis.plot_traversability_graph(pred, graph, center, img), a.warmup, a.iters),
        "device_route_as_tensor_ms": timed_wall(lambda: vis.plot_traversability_graph(pred, graph, center, img, as_tensor=True), a.warmup, a.iters),
        "pil_route_ms": timed_wall(lambda: pil_graph(pred, graph, center, img, table), 1, a.host_iters),
        "draw_launch_device_ms": timed_events(lambda: ops.draw(canvas, *lists), a.warmup, a.iters),
    }

    # ---- dense flow ----
    flow = (torch.randn(2, S, S, generator=g) * 15)
    img2 = imgs[1]
    want = pil_flow(flow, img.cpu(), img2.cpu(), 10)
    flow_d = flow.to(dev)
    assert np.array_equal(vis.plot_optical_flow(flow_d, img, img2, s=10), want)
    out["flow"] = {
        "lines": int(S / 10) ** 2,
        "device_route_ms": timed_wall(lambda: vis.plot_optical_flow(flow_d, img, img2, s=10), a.warmup, a.iters),
        "device_route_as_tensor_ms": timed_wall(lambda: vis.plot_optical_flow(flow_d, img, img2, s=10, as_tensor=True), a.warmup, a.iters),
        "pil_route_ms": timed_wall(lambda: pil_flow(flow, img.cpu(), img2.cpu(), 10), 1, a.host_iters),
    }

    # ---- a batch of 16 frames ----
    both = vis.plot_traversability_graph(preds, graph, centers, imgs)
    for b in range(B):
        assert np.array_equal(both[b], pil_graph(preds[b], graph, centers[b], imgs[b], table))
    blists = vis._traversability_graph_list(preds, graph, centers, 1.0, "RdYlBu", False, B)
    bcanvas = ops.image_to_u8(imgs, unit_range=True)
    out["batch"] = {
        "frames": B, "primitives": int(blists[0].shape[0]),
        "one_call_ms": timed_wall(lambda: vis.plot_traversability_graph(preds, graph, centers, imgs), a.warmup, a.iters),
        "one_call_as_tensor_ms": timed_wall(lambda: vis.plot_traversability_graph(preds, graph, centers, imgs, as_tensor=True), a.warmup, a.iters),
        "single_frame_calls_ms": timed_wall(lambda: [vis.plot_traversability_graph(preds[b], graph, centers[b], imgs[b]) for b in range(B)],
                                            2, max(1, a.iters // 10)),
        "pil_route_ms": timed_wall(lambda: [pil_graph(preds[b], graph, centers[b], imgs[b], table) for b in range(B)], 1, max(1, a.host_iters // 2)),
        "draw_launch_device_ms": timed_events(lambda: ops.draw(bcanvas, *blists), a.warmup, a.iters),
    }
    print(json.dumps({"bench": "draw", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
                      "host_iters": a.host_iters, **out}))


if __name__ == "__main__":
    main()
