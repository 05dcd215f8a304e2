"""ResNet-18 pyramid features (feature_type "torchvision") against the same network run as torch fp32 ops on the same GPU, one JSON line:

    hip_forward    ops.resnet18_forward        csrc/resnet.hip: 20 implicit-GEMM convolutions on the fp32-input MFMA + the max-pool
    torch_forward  tests/resnet_ref.py in float32 on the GPU (F.conv2d / F.batch_norm / F.max_pool2d / relu: torch's own convolutions)
    hip_pool       ops.segpool_pyramid         csrc/pyramid_pool.hip on the level maps, SLIC map with 100 components
    hip_total      forward + pooling, the work of FeatureExtractor.extract_batch without the SLIC call

Frames: the demo frames of tests/golden tiled to 448 x 448 RGB (uint8 for the HIP path, their float image for torch, converted outside
the timed region); seeded synthetic weights; B = 1 and B = 16.  Every shape is warmed up; then ``--rounds`` rounds alternate the routes,
each timed with HIP events around ``--iters`` calls; the median over the rounds and the (min, max) are reported, ms per call (the
whole batch).  ``forward_flop`` is 2 x the multiply-adds of the 20 convolutions, computed from the shapes; ``hip_forward_tflops`` is
that over the median time (an end-to-end rate of 21 launches, not a kernel's share of peak).

    python scripts/bench_resnet_pyramid.py [--iters N] [--warmup N] [--rounds N] [--size 448] [--batches 1,16]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resnet_ref as REF  # noqa: E402

from wild_visual_navigation_amd import ops  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import torchvision_interface as TVI  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def frames_for(size, B, dev):
    f = torch.load(os.path.join(ROOT, "tests", "golden", "demo_frames_224.pt"), map_location="cpu", weights_only=False)["frames_u8"]
    rep = (size + 223) // 224
    f = f.repeat(1, 1, rep, rep)[:, :, :size, :size]
    return torch.stack([f[b % f.shape[0]] for b in range(B)]).contiguous().to(dev)


def forward_flop(size, B):
    """2 x multiply-adds of the 20 convolutions on B frames of size x size."""
    shapes = TVI.resnet18_conv_shapes()
    total = 0
    for conv, _ in TVI.resnet18_conv_names():
        co, ci, k, _ = shapes[conv]
        if conv == "conv1":
            out = size // 2
        else:
            L = int(conv[5])
            out = size // (2 << L)
        total += 2 * co * ci * k * k * out * out
    return total * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--batches", default="1,16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resnet_pyramid.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    sd = TVI.synthetic_resnet18_state_dict(0)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    net = TVI.TorchVisionInterface(dev, "resnet18", input_size=a.size, pretrained_weights=sd)
    cases = []
    for B in (int(b) for b in a.batches.split(",")):
        img = frames_for(a.size, B, dev)
        img_f = img.float() / 255
        seg = ops.slic(img, 100, 10.0)
        S = ops.slic_num_clusters(a.size, a.size, 100)
        with torch.no_grad():
            levels = net.forward_levels(img)
            routes = {
                "hip_forward_ms": lambda: net.forward_levels(img),
                "torch_forward_ms": lambda: REF.resnet18(sd_dev, img_f, dtype=torch.float32),
                "hip_pool_ms": lambda: ops.segpool_pyramid(levels, seg, S),
                "hip_total_ms": lambda: ops.segpool_pyramid(net.forward_levels(img), seg, S),
            }
            want = REF.resnet18(sd_dev, img_f, dtype=torch.float32)
            diff = {f"feat{l + 1}": ((levels[l].permute(0, 3, 1, 2) - want[f"feat{l + 1}"]).abs().max() / want[f"feat{l + 1}"].abs().max()).item()
                    for l in range(4)}
            for fn in routes.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            samples = {k: [] for k in routes}
            for _ in range(a.rounds):
                for k, fn in routes.items():
                    samples[k].append(timed(fn, a.iters))
        flop = forward_flop(a.size, B)
        case = {"frame": f"{a.size}x{a.size}", "batch": B, "segments": S, "forward_flop": flop,
                "max_rel_hip_minus_torch": {k: float(f"{v:.3e}") for k, v in diff.items()}}
        for k, v in samples.items():
            case[k] = round(statistics.median(v), 4)
            case[k.replace("_ms", "_min_max_ms")] = [round(min(v), 4), round(max(v), 4)]
        case["hip_forward_tflops"] = round(flop / case["hip_forward_ms"] / 1e9, 2)
        case["torch_forward_tflops"] = round(flop / case["torch_forward_ms"] / 1e9, 2)
        case["torch_over_hip_forward"] = round(case["torch_forward_ms"] / case["hip_forward_ms"], 2)
        cases.append(case)
    print(json.dumps({"bench": "resnet_pyramid", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
                      "rounds": a.rounds, "cases": cases}), flush=True)


if __name__ == "__main__":
    main()
