"""Per-segment dense-SIFT features (feature_type "sift") three ways on the same GPU, one JSON line:

    fused        ops.dense_sift_segpool                      (csrc/dense_sift.hip: the [B,384,H,W] map is never written)
    dense_pool   ops.dense_sift -> [B,H*W,384] -> ops.segmean_tokens     (the map written once, transposed, re-read)
    torch_pool   the float32 torch statement of the definition (tests/dense_sift_ref.py: 8 + 1 conv2d per channel and the
                 normalisations as torch operations: the reference's route) -> [B,H*W,384] -> ops.segmean_tokens
    dense_only / torch_only: the two ways to the dense map without the pooling.

Frames: the demo frames of tests/golden tiled to 448 x 448 RGB uint8 (the fused and dense kernels read uint8; the torch statement
gets the float image, converted outside the timed region); segment map: SLIC with 100 components (computed once, outside the timed
region); B = 1 and B = 8.  HIP-event timed after warm-up, ms per call (the whole batch).  ``bytes_dense_map`` is the size of the fp32
map; the torch route writes and re-reads several tensors of that size.

    python scripts/bench_dense_sift.py [--iters N] [--warmup N] [--size 448] [--batches 1,8]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_sift_ref as REF  # noqa: E402

from wild_visual_navigation_amd import ops  # noqa: E402


def timed(fn, warmup, iters):
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


def frames_for(size, B, dev):
    f = torch.load(os.path.join(ROOT, "tests", "golden", "demo_frames_224.pt"), map_location="cpu", weights_only=False)["frames_u8"]
    rep = (size + 223) // 224
    f = f.repeat(1, 1, rep, rep)[:, :, :size, :size]
    return torch.stack([f[b % f.shape[0]] for b in range(B)]).contiguous().to(dev)


def rows(dense):
    B, D, H, W = dense.shape
    return dense.reshape(B, D, H * W).transpose(1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--batches", default="1,8")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = []
    for B in (int(b) for b in a.batches.split(",")):
        img = frames_for(a.size, B, dev)
        img_f = img.float() / 255
        seg = ops.slic(img, 100, 10.0)
        S = ops.slic_num_clusters(a.size, a.size, 100)
        with torch.no_grad():
            fused = ops.dense_sift_segpool(img, seg, S)
            pooled = ops.segmean_tokens(seg, rows(ops.dense_sift(img)), S)
            torch_pooled = ops.segmean_tokens(seg, rows(REF.dense_sift(img_f, dtype=torch.float32)), S)
            t = {
                "fused_ms": timed(lambda: ops.dense_sift_segpool(img, seg, S), a.warmup, a.iters),
                "dense_only_ms": timed(lambda: ops.dense_sift(img), a.warmup, a.iters),
                "dense_pool_ms": timed(lambda: ops.segmean_tokens(seg, rows(ops.dense_sift(img)), S), a.warmup, a.iters),
                "torch_only_ms": timed(lambda: REF.dense_sift(img_f, dtype=torch.float32), a.warmup, a.iters),
                "torch_pool_ms": timed(lambda: ops.segmean_tokens(seg, rows(REF.dense_sift(img_f, dtype=torch.float32)), S), a.warmup,
                                       a.iters),
            }
        ok = torch.isfinite(fused)
        case = {"frame": f"{a.size}x{a.size}", "batch": B, "segments": S, "bytes_dense_map": B * 384 * a.size * a.size * 4,
                "max_abs_fused_minus_dense_pool": (fused - pooled)[ok].abs().max().item(),
                "max_abs_fused_minus_torch_pool": (fused - torch_pooled)[ok].abs().max().item()}
        case.update({k: round(v, 4) for k, v in t.items()})
        case["dense_pool_over_fused"] = round(t["dense_pool_ms"] / t["fused_ms"], 2)
        case["torch_pool_over_fused"] = round(t["torch_pool_ms"] / t["fused_ms"], 2)
        case["dense_map_write_GBps"] = round(case["bytes_dense_map"] / t["dense_only_ms"] / 1e6, 1)
        cases.append(case)
    print(json.dumps({"bench": "dense_sift", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
                      "cases": cases}), flush=True)


if __name__ == "__main__":
    main()
