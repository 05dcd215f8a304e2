"""Anomaly-detection inference: the fused LinearRnvp flow kernel (csrc/rnvp.hip) beside the same flow as torch fp32 ops on the same
GPU -- the only baseline there is, since the mode did not exist before.  LinearRnvp(384, [200]), seeded weights.

  per pixel   one 448^2 frame from its 56 x 56 patch tokens: forward_per_pixel_exact (up-sample inside the kernel) against
              F.interpolate(align_corners=True) to the dense [200704, 384] rows -> the model's torch statement -> confidence
  per segment 8 x 100 segment rows: forward_rows against the torch statement

One JSON line: times in ms, the kernel's MFMA count per 32 rows, and the share of the matrix pipes' cycles those MFMAs fill
(v_mfma_f32_32x32x16_bf16 issues every 32 cycles per SIMD; 4 SIMDs per CU; --clock-ghz, default the 2.4 GHz peak clock, so the
share is a lower bound when the chip holds less under load).

    python scripts/bench_linear_rnvp.py [--iters N] [--size 448]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd.model import LinearRnvp  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def mfma_per_32_rows(D, h):
    """csrc/rnvp.hip: per flow, layer 1 of s and t (2 HB blocks x KA k-steps), layer 2 (2 HB x KH), layer 3 (2 NB x KH), three
    MFMAs per hi + lo product."""
    hb = 7 if h <= 224 else 8
    nb = (D // 2 + 31) // 32
    ka, kh = 2 * nb, 2 * hb
    return 2 * 3 * (2 * hb * ka + 2 * hb * kh + 2 * nb * kh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    D, h, H = 384, 200, args.size
    G = H // 8
    torch.manual_seed(0)
    m = LinearRnvp(D, [h], use_permutation=True).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    tokens = torch.randn(1, G * G, D, generator=g).to(dev)
    rows = torch.randn(800, D, generator=g).to(dev)
    mean, std, f = 550.0, 20.0, 0.5

    def kernel_pixels():
        return m.forward_per_pixel_exact(tokens[0], 1, G, (H, H), mean, std, f, want_loss=True)

    @torch.no_grad()
    def torch_pixels():
        dense = F.interpolate(tokens.view(1, G, G, D).permute(0, 3, 1, 2), size=(H, H), mode="bilinear", align_corners=True)
        z, log_det, logprob = m.flow_torch(dense.permute(0, 2, 3, 1).reshape(H * H, D))
        x = -(logprob.sum(1) + log_det)
        lo, hi = max(mean + std * f - std, 0.0), mean + std * f + std
        return 1 - (x.clamp(lo, hi) - lo) / (hi - lo), x

    @torch.no_grad()
    def torch_rows():
        z, log_det, logprob = m.flow_torch(rows)
        return logprob.sum(1) + log_det

    conf_k, _, loss_k = kernel_pixels()
    conf_t, loss_t = torch_pixels()
    props = torch.cuda.get_device_properties(0)
    t_kp, t_tp = timed(kernel_pixels, args.iters), timed(torch_pixels, args.iters)
    t_kr, t_tr = timed(lambda: m.forward_rows(rows, want_z=False), args.iters), timed(torch_rows, args.iters)
    n_mfma = mfma_per_32_rows(D, h)
    tiles = (H * H + 31) // 32
    pipe = tiles * n_mfma * 32 / (t_kp * 1e-3 * args.clock_ghz * 1e9 * 4 * props.multi_processor_count)
    print(json.dumps({
        "model": f"LinearRnvp({D}, [{h}])", "frame": f"{H}x{H}", "rows_per_frame": H * H,
        "pixel_kernel_ms": round(t_kp, 4), "pixel_torch_ms": round(t_tp, 4), "pixel_speedup": round(t_tp / t_kp, 2),
        "segment_rows": 800, "segment_kernel_ms": round(t_kr, 5), "segment_torch_ms": round(t_tr, 5),
        "mfma_per_32_rows": n_mfma, "matrix_pipe_share": round(pipe, 4), "clock_ghz_assumed": args.clock_ghz,
        "compute_units": props.multi_processor_count,
        "max_abs_diff_score": float((loss_k.reshape(-1) - loss_t).abs().max()),
        "max_abs_diff_conf": float((conf_k.reshape(-1) - conf_t).abs().max())}), flush=True)


if __name__ == "__main__":
    main()
