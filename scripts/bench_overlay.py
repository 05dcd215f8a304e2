"""The traversability overlay (plot_detectron_classification) three ways, one JSON line:

    fused      ops.overlay (csrc/overlay.hip) + the device -> host copy of the finished uint8 picture
    torch_gpu  the same composition as torch operations on the GPU (tests/visu_ref.py run on the device) + that copy
    host       the reference's route: frame and map copied to the host, tests/visu_ref.py on the CPU

at 224 x 224 B = 1, 448 x 448 B = 1 and 448 x 448 B = 16, and quick_start.py's three-panel picture [frame | confidence |
traversability]: ops.overlay_panels (one launch) against three separate calls plus a concatenate.

Frames: the demo frames of tests/golden tiled, fp32 in [0, 1] on the device; the map: random values in [0, 1]; the default colour
table.  The three routes end on the host, so they are timed with the wall clock around ``iters`` calls after ``warmup`` (the device
idle before and after); ``fused_device_ms`` is the fused call alone between HIP events (with the frame-maximum reduction;
``fused_device_unit_ms`` with unit_range=True, the main kernel alone; ``fused_device_unit_out_ms`` the same into a preallocated
picture, no allocation), and ``fused_GBps`` = 19 bytes per pixel (12 frame + 4 map + 3 out) over ``fused_device_unit_out_ms``.

    python scripts/bench_overlay.py [--iters N] [--warmup N] [--host-iters N]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import visu_ref as VR  # noqa: E402

from wild_visual_navigation_amd import ops  # noqa: E402
from wild_visual_navigation_amd.visu import default_classification_table  # noqa: E402


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


def frames_for(size, B, dev):
    f = torch.load(os.path.join(ROOT, "tests", "golden", "demo_frames_224.pt"), map_location="cpu", weights_only=False)["frames_u8"]
    rep = (size + 223) // 224
    f = f.repeat(1, 1, rep, rep)[:, :, :size, :size]
    return (torch.stack([f[b % f.shape[0]] for b in range(B)]).float() / 255).contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lut_cpu = default_classification_table()
    lut = lut_cpu.to(dev)
    cases = []
    for size, B in ((224, 1), (448, 1), (448, 16)):
        img = frames_for(size, B, dev)
        g = torch.Generator().manual_seed(size + B)
        val = torch.rand(B, size, size, generator=g).to(dev)
        conf = torch.rand(B, size, size, generator=g).to(dev)
        want = VR.overlay(img.cpu(), values=val.cpu(), lut=lut_cpu, alpha=0.5)
        assert torch.equal(ops.overlay(img, values=val, lut=lut, alpha=0.5).cpu(), want)
        assert torch.equal(VR.overlay(img, values=val, lut=lut, alpha=0.5).cpu(), want)
        t = {
            "fused_ms": timed_wall(lambda: ops.overlay(img, values=val, lut=lut, alpha=0.5).cpu(), a.warmup, a.iters),
            "torch_gpu_ms": timed_wall(lambda: VR.overlay(img, values=val, lut=lut, alpha=0.5).cpu(), a.warmup, a.iters),
            "host_ms": timed_wall(lambda: VR.overlay(img.cpu(), values=val.cpu(), lut=lut_cpu, alpha=0.5), 1, a.host_iters),
            "fused_device_ms": timed_events(lambda: ops.overlay(img, values=val, lut=lut, alpha=0.5), a.warmup, a.iters),
            "fused_device_unit_ms": timed_events(lambda: ops.overlay(img, values=val, lut=lut, alpha=0.5, unit_range=True), a.warmup, a.iters),
        }
        out = torch.empty(B, size, size, 3, dtype=torch.uint8, device=dev)
        t["fused_device_unit_out_ms"] = timed_events(lambda: ops.overlay(img, values=val, lut=lut, alpha=0.5, unit_range=True, out=out),
                                                     a.warmup, a.iters)

        def three_calls():
            return torch.cat([ops.image_to_u8(img), ops.overlay(img, values=conf, lut=lut, alpha=0.5),
                              ops.overlay(img, values=val, lut=lut, alpha=0.5)], dim=2)

        assert torch.equal(ops.overlay_panels(img, [conf, val], lut, 0.5), three_calls())
        t["panel_ms"] = timed_wall(lambda: ops.overlay_panels(img, [conf, val], lut, 0.5).cpu(), a.warmup, a.iters)
        t["three_calls_ms"] = timed_wall(lambda: three_calls().cpu(), a.warmup, a.iters)
        t["panel_device_ms"] = timed_events(lambda: ops.overlay_panels(img, [conf, val], lut, 0.5), a.warmup, a.iters)
        t["three_calls_device_ms"] = timed_events(three_calls, a.warmup, a.iters)
        case = {"frame": f"{size}x{size}", "batch": B, "bytes_per_call": 19 * B * size * size}
        case.update({k: round(v, 4) for k, v in t.items()})
        case["fused_GBps"] = round(case["bytes_per_call"] / t["fused_device_unit_out_ms"] / 1e6, 1)
        case["torch_gpu_over_fused"] = round(t["torch_gpu_ms"] / t["fused_ms"], 2)
        case["host_over_fused"] = round(t["host_ms"] / t["fused_ms"], 2)
        case["three_calls_over_panel"] = round(t["three_calls_ms"] / t["panel_ms"], 2)
        cases.append(case)
    print(json.dumps({"bench": "overlay", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
                      "host_iters": a.host_iters, "cases": cases}), flush=True)


if __name__ == "__main__":
    main()
