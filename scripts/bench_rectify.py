"""Raw camera ingest (csrc/rectify.hip) on the robot's own frames, one JSON line: 1080 x 1440 bayer_gbrg8 through the Hoengg camera's
equidistant map to 1080 x 1440 (K_new = K) and to the 448 x 448 centre crop, B = 1 and B = 16, four ways on the same GPU:

    fused        ops.rectify(raw, m, "bayer_gbrg8", route="fused")      demosaic at the taps, one launch, no RGB frame in between
    two_step     ops.debayer(raw) + ops.rectify(rgb, m, "planar")        this library's own two launches (route="two_step")
    debayer      ops.debayer(raw) alone
    torch        the same definition as a torch user writes it, in float: masked mosaic planes through conv2d (the bilinear
                 kernels) + F.grid_sample(bilinear, zeros, align_corners=True) on the float map; its bytes differ in the last
                 bit and on the ring (``max_abs_torch_minus_fused`` is reported, not asserted)

and the callback forms with their upload: utils.image_to_torch (B = 1) and FeatureExtractor-style decode (ops.upload_raw_frames +
ops.rectify) on host bytes, host clock around a synchronise, with the upload alone beside it.

HIP-event timed after warm-up on one stream; every figure is the median over ``--repeats`` windows of ``--iters`` calls, ms per call
(the whole batch).  ``bytes_*`` is what each form must move (raw frame read once, map planes, output; two_step: + the RGB frame
written and read); ``*_share_of_hbm`` is those bytes over the time against the 8 TB/s HBM peak -- a floor on the traffic, the
raw frame is re-read from L2.

    python scripts/bench_rectify.py [--iters N] [--warmup N] [--repeats N] [--batches 1,16]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rectify_cases as RC  # noqa: E402
import rectify_ref as R  # noqa: E402

from wild_visual_navigation_amd import ops  # noqa: E402
from wild_visual_navigation_amd.utils.image_io import image_to_torch  # noqa: E402

HBM_PEAK = 8.0e12   # B/s, MI355X HBM3E


def timed(fn, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out)


def host_timed(fn, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return statistics.median(out)


class TorchForm:
    """bayer_gbrg8 (G B / R G) -> float RGB by conv2d on the masked planes, then grid_sample on the float map."""

    def __init__(self, H, W, qx, qy, dev):
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        red = ((yy & 1) == 1) & ((xx & 1) == 0)
        blue = ((yy & 1) == 0) & ((xx & 1) == 1)
        self.mask = torch.stack([red, ~(red | blue), blue]).float().to(dev)[None]                    # [1,3,H,W]
        rb = torch.tensor([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=torch.float32) / 4
        g = torch.tensor([[0, 1, 0], [1, 4, 1], [0, 1, 0]], dtype=torch.float32) / 4
        self.k = torch.stack([rb, g, rb])[:, None].to(dev)                                          # depthwise [3,1,3,3]
        gx = torch.from_numpy(qx / 32.0).float() * (2.0 / (W - 1)) - 1
        gy = torch.from_numpy(qy / 32.0).float() * (2.0 / (H - 1)) - 1
        self.grid = torch.stack([gx, gy], -1)[None].to(dev)

    def __call__(self, raw):
        B = raw.shape[0]
        rgb = F.conv2d(raw[:, None].float() * self.mask, self.k, padding=1, groups=3)
        out = F.grid_sample(rgb, self.grid.expand(B, -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=True)
        return (out + 0.5).clamp_(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,16")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = R.HOENGG_SIZE
    K = R.hoengg(W, H)
    outs = {"1080x1440": dict(out_size=(H, W), new_K=K), "448x448": dict(out_size=(448, 448), new_K=RC.crop_448(K))}
    cases = []
    for B in (int(b) for b in a.batches.split(",")):
        data, _ = RC.source_frames("bayer_gbrg8", B, H, W)
        raw = torch.from_numpy(data).view(B, H, W).to(dev)
        msgs = [data[b].tobytes() for b in range(B)]
        t_debayer = timed(lambda: ops.debayer(raw, "gbrg"), a.warmup, a.iters, a.repeats)
        t_upload = host_timed(lambda: ops.upload_raw_frames(msgs, H * W, dev), a.warmup, a.iters, a.repeats)
        for name, o in outs.items():
            m = ops.rectify_map(K, R.HOENGG_D, "equidistant", (H, W), device=dev, **o)
            h, w = m.out_size
            tf = TorchForm(H, W, m.qx.cpu().numpy(), m.qy.cpu().numpy(), dev)
            fused = ops.rectify(raw, m, "bayer_gbrg8", route="fused")
            assert torch.equal(fused, ops.rectify(raw, m, "bayer_gbrg8", route="two_step"))
            diff = (tf(raw).int() - fused.int()).abs()
            t = {
                "fused_ms": timed(lambda: ops.rectify(raw, m, "bayer_gbrg8", route="fused"), a.warmup, a.iters, a.repeats),
                "two_step_ms": timed(lambda: ops.rectify(raw, m, "bayer_gbrg8", route="two_step"), a.warmup, a.iters, a.repeats),
                "torch_ms": timed(lambda: tf(raw), a.warmup, max(1, a.iters // 5), a.repeats),
                "callback_ms": host_timed(lambda: ops.rectify(ops.upload_raw_frames(msgs, H * W, dev).view(B, H, W), m, "bayer_gbrg8"),
                                          a.warmup, a.iters, a.repeats),
            }
            if B == 1:
                t["image_to_torch_ms"] = host_timed(lambda: image_to_torch(msgs[0], "bayer_gbrg8", H, W, device=dev, rectify=m),
                                                    a.warmup, a.iters, a.repeats)
            bytes_fused = B * H * W + 8 * h * w + 3 * B * h * w
            bytes_two = bytes_fused + 2 * 3 * B * H * W
            case = {"source": f"{H}x{W} bayer_gbrg8", "out": name, "batch": B, "bytes_fused": bytes_fused, "bytes_two_step": bytes_two, "debayer_ms": round(t_debayer, 4),
                    "upload_ms": round(t_upload, 4)}
            case.update({k: round(v, 4) for k, v in t.items()})
            case["two_step_over_fused"] = round(t["two_step_ms"] / t["fused_ms"], 2)
            case["torch_over_fused"] = round(t["torch_ms"] / t["fused_ms"], 2)
            case["fused_share_of_hbm"] = round(bytes_fused / (t["fused_ms"] * 1e-3) / HBM_PEAK, 4)
            case["two_step_share_of_hbm"] = round(bytes_two / (t["two_step_ms"] * 1e-3) / HBM_PEAK, 4)
            case["debayer_share_of_hbm"] = round(4 * B * H * W / (t_debayer * 1e-3) / HBM_PEAK, 4)
            case["max_abs_torch_minus_fused"] = int(diff.max())
            case["torch_differing_fraction"] = round(float((diff > 0).float().mean()), 4)
            cases.append(case)
    print(json.dumps({"bench": "rectify", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
                      "repeats": a.repeats, "cases": cases}), flush=True)


if __name__ == "__main__":
    main()
